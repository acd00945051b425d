// The brute-force matcher on the FP4 matrix cores: kernel, launcher and C entries.
namespace rumi {

// ---- brute force on the FP4 matrix cores -----------------------------------------------------------------------------
// With train bits t and query bits q (popcount pq): Ham(t, q) = pq + X, X = sum_k t_k (1 - 2 q_k), a GEMM of trains (A, values 0 / 1)
// by queries (B, values +1 / -1) over K = 256.  0, +1 and -1 are the E2M1 nibbles 0x0, 0x2 and 0xA, so the product runs on
// v_mfma_f32_32x32x64_f8f6f4 with FP4 operands and no block scale (4 per 32 x 32 tile, 4 VGPRs per fragment); sums of at most 256
// such products are exact in f32.  For one query pq is a constant, so the running (best, second) are kept on X and pq is added once at
// the end.  The key is the f32 number X + index / 65536 and it comes out of the MFMA itself: the chain's C operand starts at
// index / 65536.  |X| <= 255 leaves 16 fraction bits, X = -256 still does ([-256, -255) has ulp 2^-16), so every key of a pair at
// Ham < 256 is exact, and so is every partial sum (a partial X reaches 256 only as the whole sum).  X = 256 happens only at pq = 0,
// Ham = 256: the index rounds to even there, the key stays in [256, 257) because cap <= 65535 keeps the index at or below 65534 (the
// entries reject a larger cap), and such a pair is never a reported index.  f32 min and med3
// then order the keys exactly as (Ham << 16 | index) would: "first minimum wins, a tie goes to the second place" is
// best = min(best, key), second = med3(best, second, key): two v_med3_f32 per key (the min is med3 with -inf, see bfm_neg_inf).  The index field is 16 bits wide: cap <= 65535 runs through this one kernel.
//
// Fragment maps.  C/D of 32x32: column = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 h, h = lane >> 5.  A and B: lane l
// holds row (A) / column (B) l & 31 and 32 k-values that depend only on (h, nibble); the Hamming sum does not depend on the order
// of k, so both operands take the same bit -> nibble expansion and the hardware's k order never matters: k-step s, lane half h,
// fragment dword i, nibble j holds bit 4 j + s of descriptor dword 4 h + i.
//
// Workgroup: 4 waves, 64 queries each as two B-fragment sets (2 x 16 VGPRs, expanded once) and two accumulators, so one A fragment
// read feeds two MFMAs; train rows staged 64 at a time (two tiles), expanded into LDS as ready A fragments [tile][s][lane] (16 B
// each: one conflict-free ds_read_b128 per MFMA pair), double-buffered (2 x 8 KiB), one barrier per stage.  Per lane the 16
// accumulator rows belong to ONE query, so the reduction needs no cross-lane traffic until the end, where the two lane halves
// (lanes l and l + 32: same query) merge.  While looping a key carries the row WITHOUT the half's + 4 (a constant per lane keeps
// the argmin, and the index term is then wave-uniform: 16 VGPRs advanced by one v_add_f32 each per tile, shared by both
// accumulators); the merge adds it.  Padded train rows of the last tile are zero in LDS (X = 0) and their keys are replaced by 1024 (never beats
// the initial distance 256); padded query columns are computed and not written.
// Registers: 32 (B) + 32 (two accumulators) + 16 (index term) + fragments and addresses = 108 VGPRs, four waves a SIMD.  Held to 96 (five waves)
// the compiler spills B fragments into the loop and the launch is slower (66 against 58 us per 256 pairs, profiles/r08_bruteforce_stamps.txt).
typedef int32_t bfm_v4i __attribute__((ext_vector_type(4)));
typedef int32_t bfm_v8i __attribute__((ext_vector_type(8)));
typedef float bfm_v16f __attribute__((ext_vector_type(16)));
constexpr int kBfmWaves = 4, kBfmWaveQueries = 64, kBfmQueries = kBfmWaveQueries * kBfmWaves, kBfmStage = 64;
constexpr float kBfmIdx = 1.0f / 65536.0f;

__device__ __forceinline__ uint32_t bfm_expand(uint32_t x, int s) { return (x >> s) & 0x11111111u; }
// min as v_med3_f32(a, b, -inf): fminf would first quiet a possible signalling NaN in each MFMA result (one v_max_f32 x, x per key; keys are
// never NaN), and so would a med3 whose -inf the optimiser can see, which it turns back into fminf: the constant comes out of an asm
__device__ __forceinline__ float bfm_neg_inf() {
    float r;
    asm("s_mov_b32 %0, 0xff800000" : "=s"(r));
    return r;
}

#ifdef RUMI_BFM_STAMP
// cycle stamps (tools/build_stamp_lib.sh): wave 0 of the first workgroup of pair 0 sums its phases and prints them once
#define BFM_T(x) const long long x = clock64()
#define BFM_VAR(x) long long x = 0
#define BFM_FIRST(g, x) if ((g) == 0) x = clock64()
#define BFM_ADD(acc, a, b) acc += (b) - (a)
#else
#define BFM_T(x)
#define BFM_VAR(x)
#define BFM_FIRST(g, x)
#define BFM_ADD(acc, a, b)
#endif

__global__ __launch_bounds__(64 * kBfmWaves) __attribute__((amdgpu_waves_per_eu(4))) void k_bruteforce_mfma(const uint8_t *__restrict__ qd, const int32_t *__restrict__ nqArr,
                                                         const uint8_t *__restrict__ td, const int32_t *__restrict__ ntArr,
                                                         int countStride, long long qStride, long long tStride, int cap, int32_t *__restrict__ bestIdx,
                                                         int32_t *__restrict__ bestDist, int32_t *__restrict__ secondDist, int ring) {
    __shared__ bfm_v4i frag[2][2 * 4 * 64];                           // [buffer][tile * 4 + s][lane]
    const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, h = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int tb = ring > 0 ? (b + 1 == ring ? 0 : b + 1) : b;       // ring: frame b against its successor in the same buffer, the last against the first
    const int nq = min(nqArr[(size_t)b * countStride], cap), nt = min(ntArr[(size_t)tb * countStride], cap);
    const int q0 = blockIdx.x * kBfmQueries;
    if (q0 >= nq) return;
    const int qw = q0 + wave * kBfmWaveQueries;
    const bool waveLive = qw < nq;
    const float ninf = bfm_neg_inf();
#ifdef RUMI_BFM_STAMP
    long long cLoad = 0, cMfma = 0, cWait = 0, cKeys = 0, cStore = 0, cBar = 0;
    const long long cStart = clock64();
#endif

    // the queries: nibbles 0x2 (+1) / 0xA (-1) of this lane's half, and each one's popcount over both halves
    bfm_v8i bq[2][4];
    float best[2], second[2];
    auto query = [&](int u, uint32_t (&qa)[4]) -> int {              // this lane's half of query u of the wave; returns the popcount over both halves
        const int qi = qw + u * 32 + (lane & 31);
#pragma unroll
        for (int i = 0; i < 4; i++) qa[i] = 0;
        if (qi < nq) {
            const uint32_t *src = reinterpret_cast<const uint32_t *>(qd + (size_t)b * qStride + (size_t)qi * 32) + 4 * h;   // 4-byte aligned only
#pragma unroll
            for (int i = 0; i < 4; i++) qa[i] = src[i];
        }
        const int p = __popc(qa[0]) + __popc(qa[1]) + __popc(qa[2]) + __popc(qa[3]);
        return p + __shfl_xor(p, 32);
    };
#pragma unroll
    for (int u = 0; u < 2; u++) {
        uint32_t qa[4];
        const int pq = query(u, qa);
#pragma unroll
        for (int s = 0; s < 4; s++) {
            bq[u][s] = bfm_v8i{};
#pragma unroll
            for (int i = 0; i < 4; i++) bq[u][s][i] = (int32_t)((bfm_expand(qa[i], s) << 3) | 0x22222222u);
        }
        // X = 256 - pq is Ham = 256: the initial best and second (index 0; only the second's distance is ever read)
        best[u] = second[u] = (float)(256 - pq);
    }
    // the index term of the keys: rows of the tile at hand without the half's + 4
    bfm_v16f idxf;
#pragma unroll
    for (int g = 0; g < 16; g++) idxf[g] = (float)((g & 3) + 8 * (g >> 2)) * kBfmIdx;

    // staging: thread -> (fragment lane sl, dword i) of both tiles of the stage; per tile one source dword, four expanded dwords
    const int si = tid & 3, sl = tid >> 2;
    const int srow = sl & 31, sdw = 4 * (sl >> 5) + si;
    const uint32_t *tsrc = reinterpret_cast<const uint32_t *>(td + (size_t)tb * tStride) + sdw;
    auto load = [&](int r0, int tt) -> uint32_t { const int r = r0 + tt * 32 + srow; return r < nt ? tsrc[(size_t)r * 8] : 0u; };
    auto store = [&](int buf, int tt, uint32_t x) {
        uint32_t *dst = reinterpret_cast<uint32_t *>(&frag[buf][tt * 4 * 64 + sl]) + si;
#pragma unroll
        for (int s = 0; s < 4; s++) dst[s * 64 * 4] = bfm_expand(x, s) << 1;
    };
    if (nt > 0) { store(0, 0, load(0, 0)); store(0, 1, load(0, 1)); }
    __syncthreads();
    for (int r0 = 0, buf = 0; r0 < nt; r0 += kBfmStage, buf ^= 1) {
        const bool more = r0 + kBfmStage < nt;
        BFM_T(c0);
        const uint32_t next0 = more ? load(r0 + kBfmStage, 0) : 0u;   // in flight under this stage's MFMAs
        const uint32_t next1 = more ? load(r0 + kBfmStage, 1) : 0u;
        BFM_T(c1); BFM_ADD(cLoad, c0, c1);
        if (waveLive) {
#pragma unroll
            for (int tt = 0; tt < 2; tt++) {
                const int t0 = r0 + tt * 32;
                if (t0 >= nt) break;
                const bool partial = t0 + 32 > nt;                   // the last tile: rows at or past nt are zero in LDS (X = 0) and must not win
                BFM_T(m0); BFM_VAR(mw);
                bfm_v16f acc0 = idxf, acc1 = idxf;
#pragma unroll
                for (int s = 0; s < 4; s++) {
                    const bfm_v4i a4 = frag[buf][(tt * 4 + s) * 64 + lane];
                    const bfm_v8i a = {a4[0], a4[1], a4[2], a4[3], 0, 0, 0, 0};
                    acc0 = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a, bq[0][s], acc0, 4, 4, 0, 0, 0, 0);
                    acc1 = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a, bq[1][s], acc1, 4, 4, 0, 0, 0, 0);
                }
                BFM_T(m1); BFM_ADD(cMfma, m0, m1);
                if (partial) {
#pragma unroll
                    for (int g = 0; g < 16; g++) {
                        const bool live = t0 + (g & 3) + 8 * (g >> 2) + 4 * h < nt;
                        acc0[g] = live ? acc0[g] : 1024.0f; acc1[g] = live ? acc1[g] : 1024.0f;
                    }
                }
                // (plain code, not asm: the compiler pads the MFMA -> VALU read hazard)
#pragma unroll
                for (int g = 0; g < 16; g++) {
#pragma unroll
                    for (int u = 0; u < 2; u++) {
                        const float key = u ? acc1[g] : acc0[g];
                        second[u] = __builtin_amdgcn_fmed3f(best[u], second[u], key);
                        best[u] = __builtin_amdgcn_fmed3f(best[u], key, ninf);
                    }
                    BFM_FIRST(g, mw);                                // the first keys have waited for the MFMA results
                }
                BFM_T(m2); BFM_ADD(cWait, m1, mw); BFM_ADD(cKeys, mw, m2);
#pragma unroll
                for (int g = 0; g < 16; g++) idxf[g] += 32.0f * kBfmIdx;
            }
        }
        BFM_T(c2);
        if (more) { store(buf ^ 1, 0, next0); store(buf ^ 1, 1, next1); }
        BFM_T(c3); BFM_ADD(cStore, c2, c3);
        __syncthreads();
        BFM_T(c4); BFM_ADD(cBar, c3, c4);
    }
#ifdef RUMI_BFM_STAMP
    if (blockIdx.x == 0 && blockIdx.y == 0 && tid == 0)
        printf("bfm_stamp nq %d nt %d total %lld load %lld mfma %lld wait %lld keys %lld store %lld barrier %lld\n", nq, nt, clock64() - cStart, cLoad, cMfma, cWait, cKeys,
               cStore, cBar);
#endif
    // merge the halves: lane l + 32 holds the same query over rows + 4 (the popcount is read again: two registers less across the loop)
#pragma unroll
    for (int u = 0; u < 2; u++) {
        uint32_t qa[4];
        const int pq = query(u, qa), qi = qw + u * 32 + (lane & 31);
        const float ob = __shfl_xor(best[u], 32) + 4.0f * kBfmIdx, os = __shfl_xor(second[u], 32);
        if (h == 0 && qi < nq) {
            const float b2 = fminf(best[u], ob), s2 = fminf(fminf(second[u], os), fmaxf(best[u], ob));
            const size_t o = (size_t)b * cap + qi;
            const float fl = floorf(b2);
            const int d1 = (int)fl + pq;
            bestIdx[o] = d1 < 256 ? (int)((b2 - fl) * 65536.0f) : -1;
            bestDist[o] = d1; secondDist[o] = (int)floorf(s2) + pq;
        }
    }
}

// the blocking of k_bruteforce_mfma, for tests that place cases on its edges: queries per wave, queries per workgroup, train rows per stage
extern "C" void rumi_match_bruteforce_shape(int32_t *out3) { out3[0] = kBfmWaveQueries; out3[1] = kBfmQueries; out3[2] = kBfmStage; }

static int launch_bruteforce(const void *qd, const void *nq, const void *td, const void *nt, int count_stride, long long q_stride, long long t_stride,
                             int cap, int nrows, void *best_idx, void *best_dist, void *second_dist, int ring, hipStream_t st) {
    const dim3 grid((cap + kBfmQueries - 1) / kBfmQueries, nrows);
    hipLaunchKernelGGL(k_bruteforce_mfma, grid, dim3(64 * kBfmWaves), 0, st, (const uint8_t *)qd, (const int32_t *)nq, (const uint8_t *)td, (const int32_t *)nt,
                       count_stride, q_stride, t_stride, cap, (int32_t *)best_idx, (int32_t *)best_dist, (int32_t *)second_dist, ring);
    HIP_TRY(hipGetLastError());
    return RUMI_OK;
}

}  // namespace rumi

extern "C" int rumi_match_bruteforce_batch_device_strided(const void *d_query, const void *d_nq, const void *d_train, const void *d_nt,
                                                          int32_t count_stride, int64_t query_stride, int64_t train_stride, int32_t cap, int32_t nbatch,
                                                          void *d_best_idx, void *d_best_dist, void *d_second_dist, void *hip_stream) {
    if (!d_query || !d_nq || !d_train || !d_nt || !d_best_idx || !d_best_dist || !d_second_dist || cap < 1 || cap > 65535 || nbatch < 1 || count_stride < 1 ||
        query_stride < 32ll * cap || train_stride < 32ll * cap || (query_stride & 3) || (train_stride & 3) ||
        (reinterpret_cast<uintptr_t>(d_query) & 3) || (reinterpret_cast<uintptr_t>(d_train) & 3))
        return RUMI_E_INVALID;                                 // the kernel packs the train index into 16 bits next to the distance
    return launch_bruteforce(d_query, d_nq, d_train, d_nt, count_stride, (long long)query_stride, (long long)train_stride, cap, nbatch, d_best_idx, d_best_dist,
                             d_second_dist, 0, (hipStream_t)hip_stream);
}

extern "C" int rumi_match_bruteforce_ring_device(const void *d_desc, const void *d_n, int32_t count_stride, int64_t frame_stride, int32_t cap, int32_t nframes,
                                                 void *d_best_idx, void *d_best_dist, void *d_second_dist, void *hip_stream) {
    if (!d_desc || !d_n || !d_best_idx || !d_best_dist || !d_second_dist || cap < 1 || cap > 65535 || nframes < 1 || count_stride < 1 ||
        frame_stride < 32ll * cap || (frame_stride & 3) || (reinterpret_cast<uintptr_t>(d_desc) & 3))
        return RUMI_E_INVALID;
    return launch_bruteforce(d_desc, d_n, d_desc, d_n, count_stride, (long long)frame_stride, (long long)frame_stride, cap, nframes, d_best_idx, d_best_dist,
                             d_second_dist, nframes, (hipStream_t)hip_stream);
}

extern "C" int rumi_match_bruteforce_batch_device(const void *d_query, const void *d_nq, const void *d_train, const void *d_nt,
                                                  int32_t count_stride, int32_t cap, int32_t nbatch, void *d_best_idx,
                                                  void *d_best_dist, void *d_second_dist, void *hip_stream) {
    return rumi_match_bruteforce_batch_device_strided(d_query, d_nq, d_train, d_nt, count_stride, 32ll * cap, 32ll * cap, cap, nbatch, d_best_idx, d_best_dist,
                                                      d_second_dist, hip_stream);
}
