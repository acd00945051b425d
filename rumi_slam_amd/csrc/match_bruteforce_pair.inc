// The brute-force matcher for ONE pair, latency form: k_bruteforce_pair, its launcher (rumi_internal.h) and the rumi_match_bruteforce_pair_* entries.
namespace rumi {

// ---- one pair, train rows split over workgroups ------------------------------------------------------------------------
// k_bruteforce_mfma (match_bruteforce.inc) launches (query blocks, pairs): one pair of 1000 x 1000 descriptors is 4 workgroups that each walk all 16
// train stages one after the other.  Here the grid is (query blocks of kBfmQueries, S train slices); a slice is a whole number of kBfmStage-row
// stages, so no tile straddles two slices.  Workgroup (qb, s) runs the same stage loop over rows [s R, min(nt, (s + 1) R)) only, with the index
// term of the keys started at s R: its keys are the batch kernel's keys for those rows, bit for bit (same FP4 operands, same MFMA chain, same C
// operand), and it leaves one (best key, second key) pair of f32 per query, merged over the two lane halves as the batch kernel's epilogue does.
//
// Combine.  Per query the batch kernel reduces the multiset {I, I, every key}, I = 256 - pq (the initial best and second), to its smallest
// element and the floor of its second smallest.  Slice s reduces {I, I, keys of slice s}.  The union over the slices holds the same keys and 2 S
// copies of I instead of 2; both multisets hold I at least twice, so their two smallest elements agree.  For two partial results (a1, a2), (b1, b2) the
// union's are best = min(a1, b1), second = min(max(a1, b1), a2, b2): min and max of exact f32 numbers, associative and commutative, so the result
// does not depend on how many slices there are or in which order they arrive.  (Second keys may lack the lane half's + 4 in their index field, as
// in the batch kernel: only their floor is read.)
//
// Last arriver.  Partials go to scratch [S][cap][2] f32 by plain stores; every storing wave drains its stores, the workgroup meets at a barrier, one
// lane releases at agent scope (and waits: the compiler may drop the fence's own wait) and draws a ticket from the query block's word by a
// returning relaxed agent-scope add.  The workgroup that draws S - 1 acquires at agent scope, waits, tells its other waves through LDS behind
// a barrier, reads all S partials with plain vector loads, converts exactly as the batch kernel does, writes the outputs and puts the ticket
// back to 0, so the scratch needs no clearing between calls.  No workgroup waits for another one: there is no loop on a memory word.
// S = 1 touches neither scratch nor ticket.
//
// Mirror (the streaming front-end, orb_host.hip): the workgroups of slice 0 copy the query descriptor rows they load and their queries' key-points,
// workgroup (0, 0) the counts, and the merging workgroup its three result rows to a second set of pointers -- the device's view of a pinned
// host block -- so the resident copy and the host copy of a frame come out of one launch.
struct PairMirror {
    int32_t *counts;                 // {n, monoIndex, n_prev}; nullptr = no mirror
    const uint32_t *kpSrc;           // the query frame's key-points (7 dwords each)
    uint32_t *kp;
    uint8_t *desc;                   // 16-byte aligned
    int32_t *bestIdx, *bestDist, *secondDist;
};
constexpr int kBfpMaxSlices = 64;       // bounds the scratch; a forced count may not exceed min(stages in cap, this)
constexpr int kBfpAutoStages = 2;       // slices = 0: this many stages per slice (DESIGN.md section 4m has the sweep)

__global__ __launch_bounds__(64 * kBfmWaves) void k_bruteforce_pair(const uint8_t *__restrict__ qd, const int32_t *__restrict__ nqPtr, const uint8_t *__restrict__ td,
                                                                    const int32_t *__restrict__ ntPtr, int cap, int sliceRows, float *scratch, unsigned *tickets,
                                                                    int32_t *__restrict__ bestIdx, int32_t *__restrict__ bestDist, int32_t *__restrict__ secondDist,
                                                                    PairMirror mir) {
    __shared__ bfm_v4i frag[2][2 * 4 * 64];                           // [buffer][tile * 4 + s][lane]; word 0 carries "this workgroup merges" at the end
    const int tid = threadIdx.x, lane = tid & 63, h = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int slice = blockIdx.y, S = gridDim.y;
    const int nq = min(nqPtr[0], cap), nt = min(ntPtr[0], cap);
    const int q0 = blockIdx.x * kBfmQueries;
    const bool mirror = mir.counts != nullptr && slice == 0;
    if (mirror && blockIdx.x == 0 && tid == 0) { mir.counts[0] = nqPtr[0]; mir.counts[1] = nqPtr[1]; mir.counts[2] = nt; }
    if (q0 >= nq) return;                                             // (every slice of the query block decides the same: its ticket stays untouched)
    const int qw = q0 + wave * kBfmWaveQueries;
    const bool waveLive = qw < nq;
    const float ninf = bfm_neg_inf();
    const int rBegin = min(slice * sliceRows, nt), rEnd = min(rBegin + sliceRows, nt);   // this slice's train rows

    bfm_v8i bq[2][4];
    float best[2], second[2];
    auto query = [&](int u, uint32_t (&qa)[4]) -> int {              // this lane's half of query u of the wave; returns the popcount over both halves
        const int qi = qw + u * 32 + (lane & 31);
#pragma unroll
        for (int i = 0; i < 4; i++) qa[i] = 0;
        if (qi < nq) {
            const uint32_t *src = reinterpret_cast<const uint32_t *>(qd + (size_t)qi * 32) + 4 * h;   // 4-byte aligned only
#pragma unroll
            for (int i = 0; i < 4; i++) qa[i] = src[i];
        }
        const int p = __popc(qa[0]) + __popc(qa[1]) + __popc(qa[2]) + __popc(qa[3]);
        return p + __shfl_xor(p, 32);
    };
#pragma unroll
    for (int u = 0; u < 2; u++) {
        uint32_t qa[4];
        const int pq = query(u, qa), qi = qw + u * 32 + (lane & 31);
        if (mirror && qi < nq) *reinterpret_cast<uint4 *>(mir.desc + (size_t)qi * 32 + 16 * h) = make_uint4(qa[0], qa[1], qa[2], qa[3]);
#pragma unroll
        for (int s = 0; s < 4; s++) {
            bq[u][s] = bfm_v8i{};
#pragma unroll
            for (int i = 0; i < 4; i++) bq[u][s][i] = (int32_t)((bfm_expand(qa[i], s) << 3) | 0x22222222u);
        }
        best[u] = second[u] = (float)(256 - pq);
    }
    // the index term of the keys: rows of the tile at hand without the half's + 4, from the slice's first row on
    bfm_v16f idxf;
#pragma unroll
    for (int g = 0; g < 16; g++) idxf[g] = (float)(rBegin + (g & 3) + 8 * (g >> 2)) * kBfmIdx;

    const int si = tid & 3, sl = tid >> 2;
    const int srow = sl & 31, sdw = 4 * (sl >> 5) + si;
    const uint32_t *tsrc = reinterpret_cast<const uint32_t *>(td) + sdw;
    auto load = [&](int r0, int tt) -> uint32_t { const int r = r0 + tt * 32 + srow; return r < rEnd ? tsrc[(size_t)r * 8] : 0u; };
    auto store = [&](int buf, int tt, uint32_t x) {
        uint32_t *dst = reinterpret_cast<uint32_t *>(&frag[buf][tt * 4 * 64 + sl]) + si;
#pragma unroll
        for (int s = 0; s < 4; s++) dst[s * 64 * 4] = bfm_expand(x, s) << 1;
    };
    if (rBegin < rEnd) { store(0, 0, load(rBegin, 0)); store(0, 1, load(rBegin, 1)); }
    __syncthreads();
    for (int r0 = rBegin, buf = 0; r0 < rEnd; r0 += kBfmStage, buf ^= 1) {
        const bool more = r0 + kBfmStage < rEnd;
        const uint32_t next0 = more ? load(r0 + kBfmStage, 0) : 0u;   // in flight under this stage's MFMAs
        const uint32_t next1 = more ? load(r0 + kBfmStage, 1) : 0u;
        if (waveLive) {
#pragma unroll
            for (int tt = 0; tt < 2; tt++) {
                const int t0 = r0 + tt * 32;
                if (t0 >= rEnd) break;
                const bool partial = t0 + 32 > rEnd;                 // only the pair's last tile: a slice ends on a stage or at nt
                bfm_v16f acc0 = idxf, acc1 = idxf;
#pragma unroll
                for (int s = 0; s < 4; s++) {
                    const bfm_v4i a4 = frag[buf][(tt * 4 + s) * 64 + lane];
                    const bfm_v8i a = {a4[0], a4[1], a4[2], a4[3], 0, 0, 0, 0};
                    acc0 = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a, bq[0][s], acc0, 4, 4, 0, 0, 0, 0);
                    acc1 = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a, bq[1][s], acc1, 4, 4, 0, 0, 0, 0);
                }
                if (partial) {
#pragma unroll
                    for (int g = 0; g < 16; g++) {
                        const bool live = t0 + (g & 3) + 8 * (g >> 2) + 4 * h < rEnd;
                        acc0[g] = live ? acc0[g] : 1024.0f; acc1[g] = live ? acc1[g] : 1024.0f;
                    }
                }
#pragma unroll
                for (int g = 0; g < 16; g++) {
#pragma unroll
                    for (int u = 0; u < 2; u++) {
                        const float key = u ? acc1[g] : acc0[g];
                        second[u] = __builtin_amdgcn_fmed3f(best[u], second[u], key);
                        best[u] = __builtin_amdgcn_fmed3f(best[u], key, ninf);
                    }
                }
#pragma unroll
                for (int g = 0; g < 16; g++) idxf[g] += 32.0f * kBfmIdx;
            }
        }
        if (more) { store(buf ^ 1, 0, next0); store(buf ^ 1, 1, next1); }
        __syncthreads();
    }
    // the key-points of this block's queries, for the mirror: 7 dwords each
    if (mirror) {
        const int d0 = q0 * 7, d1 = min(q0 + kBfmQueries, nq) * 7;
        for (int i = d0 + tid; i < d1; i += 64 * kBfmWaves) mir.kp[i] = mir.kpSrc[i];
    }

    // merge the halves (lane l + 32 holds the same query over rows + 4), then either finish (S = 1) or publish the partial
    float b2[2], s2[2];
    int pqs[2];
#pragma unroll
    for (int u = 0; u < 2; u++) {
        uint32_t qa[4];
        pqs[u] = query(u, qa);
        const float ob = __shfl_xor(best[u], 32) + 4.0f * kBfmIdx, os = __shfl_xor(second[u], 32);
        b2[u] = fminf(best[u], ob); s2[u] = fminf(fminf(second[u], os), fmaxf(best[u], ob));
    }
    if (S > 1) {
#pragma unroll
        for (int u = 0; u < 2; u++) {
            const int qi = qw + u * 32 + (lane & 31);
            if (h == 0 && qi < nq) *reinterpret_cast<float2 *>(scratch + ((size_t)slice * cap + qi) * 2) = make_float2(b2[u], s2[u]);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");             // every storing wave drains its stores
        __syncthreads();                                             // (the stage loop's last barrier is behind every LDS read: word 0 is free)
        int *flag = reinterpret_cast<int *>(&frag[0][0]);
        if (tid == 0) {
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");         // (the fence's own wait may be dropped by the compiler)
            const unsigned t = __hip_atomic_fetch_add(tickets + blockIdx.x, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const int last = t == (unsigned)(S - 1);
            if (last) {
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            }
            *flag = last;
        }
        __syncthreads();
        if (*flag == 0) return;
#pragma unroll
        for (int u = 0; u < 2; u++) {
            const int qi = qw + u * 32 + (lane & 31);
            if (h == 0 && qi < nq) {
                // eight partials in flight at a time (one after the other each costs a trip to L2); +inf is the rule's neutral element
                float mb = INFINITY, ms = INFINITY;
                for (int s0 = 0; s0 < S; s0 += 8) {
                    float2 p[8];
#pragma unroll
                    for (int k = 0; k < 8; k++)
                        p[k] = s0 + k < S ? *reinterpret_cast<const float2 *>(scratch + ((size_t)(s0 + k) * cap + qi) * 2) : make_float2(INFINITY, INFINITY);
#pragma unroll
                    for (int k = 0; k < 8; k++) { ms = fminf(fminf(ms, p[k].y), fmaxf(mb, p[k].x)); mb = fminf(mb, p[k].x); }
                }
                b2[u] = mb; s2[u] = ms;
            }
        }
        if (tid == 0) __hip_atomic_store(tickets + blockIdx.x, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // the next call finds it at 0
    }
#pragma unroll
    for (int u = 0; u < 2; u++) {
        const int qi = qw + u * 32 + (lane & 31);
        if (h == 0 && qi < nq) {
            const float fl = floorf(b2[u]);
            const int d1 = (int)fl + pqs[u];
            const int bi = d1 < 256 ? (int)((b2[u] - fl) * 65536.0f) : -1, sd = (int)floorf(s2[u]) + pqs[u];
            bestIdx[qi] = bi; bestDist[qi] = d1; secondDist[qi] = sd;
            if (mir.counts) { mir.bestIdx[qi] = bi; mir.bestDist[qi] = d1; mir.secondDist[qi] = sd; }
        }
    }
}

static int bfp_stages(int rows) { return (rows + kBfmStage - 1) / kBfmStage; }
static int bfp_max_slices(int cap) { return std::min(bfp_stages(cap), kBfpMaxSlices); }
static size_t bfp_partial_bytes(int cap) { return ((size_t)bfp_max_slices(cap) * cap * 2 * sizeof(float) + 15) & ~(size_t)15; }

// {slices used, rows per slice} for up to nt train rows (nt clipped to 1..cap); slices = 0: the automatic choice.  {0, 0}: refused.
static void bfp_shape(int cap, int nt, int slices, int32_t *out2) {
    out2[0] = out2[1] = 0;
    if (cap < 1 || cap > 65535 || slices < 0 || slices > bfp_max_slices(cap)) return;
    const int stages = bfp_stages(std::max(1, std::min(nt, cap)));
    if (slices == 0) slices = std::min((stages + kBfpAutoStages - 1) / kBfpAutoStages, kBfpMaxSlices);
    out2[0] = slices;
    out2[1] = (stages + slices - 1) / slices * kBfmStage;
}

int launch_bruteforce_pair(const void *qd, const void *nq, const void *td, const void *nt, int cap, int nt_bound, int slices, void *scratch, void *best_idx,
                           void *best_dist, void *second_dist, const PairMirrorArgs *mirror, hipStream_t st) {
    int32_t shape[2];
    bfp_shape(cap, nt_bound, slices, shape);
    if (shape[0] < 1) return RUMI_E_INVALID;
    PairMirror mir{};
    if (mirror)
        mir = PairMirror{(int32_t *)mirror->counts, (const uint32_t *)mirror->kp_src, (uint32_t *)mirror->kp, (uint8_t *)mirror->desc, (int32_t *)mirror->best_idx,
                         (int32_t *)mirror->best_dist, (int32_t *)mirror->second_dist};
    const dim3 grid((cap + kBfmQueries - 1) / kBfmQueries, shape[0]);
    hipLaunchKernelGGL(k_bruteforce_pair, grid, dim3(64 * kBfmWaves), 0, st, (const uint8_t *)qd, (const int32_t *)nq, (const uint8_t *)td, (const int32_t *)nt, cap,
                       shape[1], (float *)scratch, (unsigned *)((uint8_t *)scratch + bfp_partial_bytes(cap)), (int32_t *)best_idx, (int32_t *)best_dist,
                       (int32_t *)second_dist, mir);
    HIP_TRY(hipGetLastError());
    return RUMI_OK;
}

}  // namespace rumi

extern "C" int64_t rumi_match_bruteforce_pair_scratch_bytes(int32_t cap) {
    if (cap < 1 || cap > 65535) return 0;
    return (int64_t)(bfp_partial_bytes(cap) + (((size_t)(cap + kBfmQueries - 1) / kBfmQueries * sizeof(unsigned) + 15) & ~(size_t)15));
}

extern "C" void rumi_match_bruteforce_pair_shape(int32_t cap, int32_t nt, int32_t slices, int32_t *out2) { if (out2) bfp_shape(cap, nt, slices, out2); }

extern "C" int rumi_match_bruteforce_pair_device(const void *d_query, const void *d_nq, const void *d_train, const void *d_nt, int32_t cap, int32_t slices,
                                                 void *d_scratch, void *d_best_idx, void *d_best_dist, void *d_second_dist, void *hip_stream) {
    if (!d_query || !d_nq || !d_train || !d_nt || !d_scratch || !d_best_idx || !d_best_dist || !d_second_dist || cap < 1 || cap > 65535 || slices < 0 ||
        slices > bfp_max_slices(cap) || (reinterpret_cast<uintptr_t>(d_query) & 3) || (reinterpret_cast<uintptr_t>(d_train) & 3) ||
        (reinterpret_cast<uintptr_t>(d_scratch) & 15)) {
        g_lastError = "rumi_match_bruteforce_pair_device: null pointer, cap outside 1..65535, slices outside 0..min(stages in cap, 64), or misaligned descriptors / scratch";
        return RUMI_E_INVALID;
    }
    return launch_bruteforce_pair(d_query, d_nq, d_train, d_nt, cap, cap, slices, d_scratch, d_best_idx, d_best_dist, d_second_dist, nullptr, (hipStream_t)hip_stream);
}
