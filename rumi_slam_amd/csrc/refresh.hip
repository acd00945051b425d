// MapPoint::ComputeDistinctiveDescriptors (R/lib_src/MapPoint.cc:353-427) and MapPoint::UpdateNormalAndDepth (:450-518) for a batch of points
// (include/rumi_mapping.h, rumi_refresh_map_points).
//
// The host validates, drops the observations of bad key-frames for the descriptor part (:376), gathers the remaining descriptor rows point by
// point into one pinned block and bins the points by the number N of rows left:
//   N  1..16   k_refresh_desc_group<16>   four points a wave, one DPP row of 16 lanes each
//   N 17..32   k_refresh_desc_group<32>   two points a wave
//   N 33..64   k_refresh_desc_group<64>   a wave a point
//   N 65..     k_refresh_desc_block       a workgroup of four waves a point, the rows in LDS, a wave a row
// A lane of a group holds descriptor j of its point in 8 dwords; row i is read from LDS at one address per group (a broadcast); the lane forms
// d[i][j] by xor + v_bcnt.  The median is the element of rank (N-1)/2 of the row: the groups find it by nine ballot + popcount steps over the
// bits of the distance (0..256) from the top, the workgroup kernel by a 257-bin count in LDS and a prefix sum across the wave.  Nothing is
// sorted.  Rows are visited in ascending order and a median replaces the best only when strictly smaller (:416).
// k_refresh_normal: a lane a point walks the point's observations in list order -- the order of the float sum is part of the definition, so
// nothing is reduced across lanes.  Integer LDS atomics only (the count), no float atomics: the same bytes on every run.
// rumi_refresh_map_points_resident (refresh_resident.inc) runs the same two walks over rows it fetches from the covisibility store in place.
#include <algorithm>
#include <climits>
#include <cstring>
#include <vector>

#include "rumi_common.h"
#include "covis_view.h"
#include "rumi_mapping.h"

namespace rumi {
namespace {

struct PtDev {
    float pos[3];
    int32_t refKf;
    float scaleRef, scaleLast;   // mvScaleFactors[level], mvScaleFactors[nLevels - 1] of the reference key-frame
    int32_t obsOff, nObs;        // the point's slice of the key-frame index list (all observations)
    int32_t descOff, nGood;      // its gathered rows (observations of good key-frames)
};
struct OutDev {
    int32_t bestObs, bestMedian;
    float normal[3], minD, maxD;
    int32_t updated;
};
static_assert(sizeof(PtDev) == 40 && sizeof(OutDev) == 32, "block layouts");

constexpr int kHistStride = 264;     // 257 bins a wave, rounded up to a multiple of 4 (int4 reads)

__device__ __forceinline__ int hamming(const uint4 &a0, const uint4 &a1, const uint4 &b0, const uint4 &b1) {
    return __popc(a0.x ^ b0.x) + __popc(a0.y ^ b0.y) + __popc(a0.z ^ b0.z) + __popc(a0.w ^ b0.w) + __popc(a1.x ^ b1.x) + __popc(a1.y ^ b1.y) +
           __popc(a1.z ^ b1.z) + __popc(a1.w ^ b1.w);
}

// The walk of a group of G lanes over its point's N rows (rows: the group's rows in LDS; a0, a1: row `sub` in registers, zero from N on):
// best = the smallest median, bestIdx = the first row that has it.  Both entries' group kernels end in this walk.
template <int G>
__device__ __forceinline__ void desc_group_best(const uint4 &a0, const uint4 &a1, const uint4 *rows, int N, int sub, int lane, int &best, int &bestIdx) {
    const int gbase = lane & ~(G - 1);
    const unsigned long long gmask = G == 64 ? ~0ull : (1ull << (G & 63)) - 1;
    const int rank = (N - 1) >> 1;                               // vDists[0.5*(N-1)], :414
    int nmax = 0;
    for (int k = 0; k < 64; k += G) nmax = max(nmax, __shfl(N, k));
    nmax = __builtin_amdgcn_readfirstlane(nmax);
    best = INT_MAX; bestIdx = 0;
    for (int i = 0; i < nmax; i++) {                             // wave-uniform trip count: the ballots below see every lane
        const int ii = i < N ? i : 0;
        const int d = hamming(a0, a1, rows[2 * ii], rows[2 * ii + 1]);
        bool cand = sub < N;
        int r = rank, med = 0;
#pragma unroll
        for (int bit = 8; bit >= 0; bit--) {                     // the value of rank r among the candidates, from the top bit down
            const bool zero = ((d >> bit) & 1) == 0;
            const int zeros = __popcll((__ballot(cand && zero) >> gbase) & gmask);
            if (r < zeros) cand = cand && zero;
            else { r -= zeros; med |= 1 << bit; cand = cand && !zero; }
        }
        if (i < N && med < best) { best = med; bestIdx = i; }    // :416
    }
}

// Points of 1..G rows, a group of G lanes each (G = 16, 32, 64; 256 / G points a workgroup).  list [nList] = the points of this bin.
template <int G>
__global__ __launch_bounds__(256) void k_refresh_desc_group(const PtDev *__restrict__ pts, const int32_t *__restrict__ list, int nList,
                                                            const uint4 *__restrict__ desc, const int32_t *__restrict__ goodPos,
                                                            OutDev *__restrict__ out) {
    __shared__ uint4 sRow[256 * 2];
    const int tid = threadIdx.x, lane = tid & 63, sub = tid & (G - 1);
    const int g = blockIdx.x * (256 / G) + tid / G;
    const bool live = g < nList;
    const int p = live ? list[g] : 0;
    const int N = live ? pts[p].nGood : 0, off = live ? pts[p].descOff : 0;
    uint4 a0 = make_uint4(0, 0, 0, 0), a1 = a0;
    if (sub < N) { a0 = desc[2 * (size_t)(off + sub)]; a1 = desc[2 * (size_t)(off + sub) + 1]; }
    sRow[2 * tid] = a0; sRow[2 * tid + 1] = a1;
    __syncthreads();
    int best, bestIdx;
    desc_group_best<G>(a0, a1, sRow + 2 * (tid - sub), N, sub, lane, best, bestIdx);
    if (live && sub == 0) { out[p].bestObs = goodPos[off + bestIdx]; out[p].bestMedian = best; }
}

// The walk of a workgroup of four waves over its point's N rows in LDS, a wave a row, against a 257-bin count per wave (hist: this wave's,
// zeroed, and a barrier passed since).  On thread 0: best = the smallest median, bestIdx = the first row that has it.  Both entries'
// workgroup kernels end in this walk.
__device__ __forceinline__ void desc_block_best(const uint4 *sRow, int *hist, int N, int tid, int lane, int wave, int *sBest, int *sBestIdx, int &best,
                                                int &bestIdx) {
    const int rank = (N - 1) >> 1;
    best = INT_MAX; bestIdx = 0;
    for (int i = wave; i < N; i += 4) {                          // ascending within the wave
        const uint4 r0 = sRow[2 * i], r1 = sRow[2 * i + 1];
        for (int j = lane; j < N; j += 64) atomicAdd(&hist[hamming(r0, r1, sRow[2 * j], sRow[2 * j + 1])], 1);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        // the first bin whose running count exceeds the rank: lane l owns bins 4l .. 4l+3, bin 256 is what is left
        const int4 h = *reinterpret_cast<const int4 *>(hist + 4 * lane);
        const int s = h.x + h.y + h.z + h.w;
        int incl = s;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) { const int t = __shfl_up(incl, o); if (lane >= o) incl += t; }
        const unsigned long long over = __ballot(incl > rank);
        int med = 256;
        if (over) {
            int m = 4 * lane, c = incl - s + h.x;
            if (rank >= c) { m++; c += h.y; if (rank >= c) { m++; c += h.z; if (rank >= c) m++; } }
            med = __shfl(m, __ffsll((long long)over) - 1);
        }
        __builtin_amdgcn_wave_barrier();
        *reinterpret_cast<int4 *>(hist + 4 * lane) = make_int4(0, 0, 0, 0);
        if (lane == 0) hist[256] = 0;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        if (med < best) { best = med; bestIdx = i; }
    }
    if (lane == 0) { sBest[wave] = best; sBestIdx[wave] = bestIdx; }
    __syncthreads();
    if (tid == 0)                                                // the first row of the smallest median over the four interleaved walks
        for (int w = 1; w < 4; w++)
            if (sBest[w] < best || (sBest[w] == best && sBestIdx[w] < bestIdx)) { best = sBest[w]; bestIdx = sBestIdx[w]; }
}

// Points of more than 64 rows: a workgroup a point.  Dynamic LDS: nAlloc rows of 32 bytes (nAlloc >= every N of the launch), then a 257-bin
// count per wave.
__global__ __launch_bounds__(256) void k_refresh_desc_block(const PtDev *__restrict__ pts, const int32_t *__restrict__ list, int nAlloc,
                                                            const uint4 *__restrict__ desc, const int32_t *__restrict__ goodPos,
                                                            OutDev *__restrict__ out) {
    extern __shared__ uint4 smem[];
    __shared__ int sBest[4], sBestIdx[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int p = list[blockIdx.x];
    const int N = min(pts[p].nGood, nAlloc), off = pts[p].descOff;
    uint4 *sRow = smem;
    int *hist = reinterpret_cast<int *>(smem + 2 * (size_t)nAlloc) + wave * kHistStride;
    for (int j = tid; j < 2 * N; j += 256) sRow[j] = desc[2 * (size_t)off + j];
    for (int k = lane; k < kHistStride; k += 64) hist[k] = 0;
    __syncthreads();
    int best, bestIdx;
    desc_block_best(sRow, hist, N, tid, lane, wave, sBest, sBestIdx, best, bestIdx);
    if (tid == 0) { out[p].bestObs = goodPos[off + bestIdx]; out[p].bestMedian = best; }
}

// The operation order rumi_mapping.h defines: differences per component, (x*x + y*y) + z*z, IEEE sqrtf, true division (the library is built
// with -ffp-contract=off).
__global__ __launch_bounds__(256) void k_refresh_normal(const PtDev *__restrict__ pts, int nPts, const float *__restrict__ kfOw,
                                                        const int32_t *__restrict__ obsKf, OutDev *__restrict__ out) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= nPts) return;
    const PtDev P = pts[p];
    if (P.nObs == 0) { out[p].updated = 0; return; }             // :465
    float nx = 0.f, ny = 0.f, nz = 0.f;
    for (int k = 0; k < P.nObs; k++) {                           // :471-483, bad key-frames included
        const float *O = kfOw + 3 * (size_t)obsKf[P.obsOff + k];
        const float dx = P.pos[0] - O[0], dy = P.pos[1] - O[1], dz = P.pos[2] - O[2];
        const float nrm = __builtin_sqrtf((dx * dx + dy * dy) + dz * dz);
        nx = nx + dx / nrm; ny = ny + dy / nrm; nz = nz + dz / nrm;
    }
    const float *R = kfOw + 3 * (size_t)P.refKf;
    const float cx = P.pos[0] - R[0], cy = P.pos[1] - R[1], cz = P.pos[2] - R[2];
    const float dist = __builtin_sqrtf((cx * cx + cy * cy) + cz * cz);   // :492-493
    const float maxD = dist * P.scaleRef;                        // :514
    const float n = (float)P.nObs;
    out[p].maxD = maxD; out[p].minD = maxD / P.scaleLast;       // :515
    out[p].normal[0] = nx / n; out[p].normal[1] = ny / n; out[p].normal[2] = nz / n;   // :516
    out[p].updated = 1;
}

}  // namespace
}  // namespace rumi

using namespace rumi;

struct RumiRefresh {
    DeviceBinding dev;
    MirrorBuf<uint8_t> blk, out;          // the upload block; the results, an OutDev a point
    std::vector<PtDev> pt;
    std::vector<int32_t> bins[4];
    std::vector<int32_t> rowLen;          // the resident entry: the observer-row length of every point of the call
    int launches = 0;                     // kernels of the last resident call
    StageClock clock;
    float stageMs[3] = {0.f, 0.f, 0.f};   // the last call: validation + gather | upload, kernels, download | write-out
};

extern "C" int rumi_refresh_create(int32_t device, RumiRefresh **out) {
    if (!out) return RUMI_E_INVALID;
    *out = new RumiRefresh();
    (*out)->dev.device = device;
    return RUMI_OK;
}

extern "C" void rumi_refresh_destroy(RumiRefresh *r) {
    if (!r) return;
    if (r->dev.bound) (void)hipSetDevice(r->dev.device);
    delete r;
}

extern "C" int rumi_refresh_map_points(RumiRefresh *r, const RumiRefreshKF *kf, int32_t n_kf, const RumiRefreshPoint *pts, int32_t n_pts,
                                       const int32_t *obs_kf, const int32_t *obs_feature, int32_t n_obs, int32_t what, int32_t *best_obs,
                                       int32_t *best_median, float *normal, float *min_distance, float *max_distance, uint8_t *updated) {
    const bool wantDesc = (what & RUMI_REFRESH_DESCRIPTOR) != 0, wantNormal = (what & RUMI_REFRESH_NORMAL_DEPTH) != 0;
    if (!r || n_kf < 0 || n_pts < 0 || n_obs < 0 || (what & ~(RUMI_REFRESH_DESCRIPTOR | RUMI_REFRESH_NORMAL_DEPTH)) || !(wantDesc || wantNormal) ||
        (n_kf > 0 && !kf) || (n_pts > 0 && !pts) || (n_obs > 0 && (!obs_kf || !obs_feature)) ||
        (n_pts > 0 && wantDesc && (!best_obs || !best_median)) ||
        (n_pts > 0 && wantNormal && (!normal || !min_distance || !max_distance || !updated))) {
        g_lastError = "rumi_refresh_map_points: missing argument, negative count, or `what` without a known mode bit";
        return RUMI_E_INVALID;
    }
    r->clock.start();
    // ---- validation, all of it before anything is written or uploaded
    for (int k = 0; k < n_kf; k++)
        if (kf[k].n < 0 || (wantDesc && kf[k].n > 0 && !kf[k].desc)) {
            g_lastError = "rumi_refresh_map_points: a key-frame with a negative feature count or without descriptors";
            return RUMI_E_INVALID;
        }
    bool tooMany = false;
    auto reference_ok = [&](int i) -> int {
        const RumiRefreshPoint &P = pts[i];
        if (P.obs_end == P.obs_begin) return RUMI_OK;            // both members return before they read the reference key-frame
        if (P.ref_kf < 0 || P.ref_kf >= n_kf || P.ref_feature < 0 || P.ref_feature >= kf[P.ref_kf].n || kf[P.ref_kf].nlevels < 1 ||
            !kf[P.ref_kf].scale_factors || P.ref_level < 0 || P.ref_level >= kf[P.ref_kf].nlevels) {
            g_lastError = "rumi_refresh_map_points: reference key-frame outside the table, ref_feature outside it, or ref_level outside its scale table";
            return RUMI_E_INVALID;
        }
        return RUMI_OK;
    };
    int rc = check_observation_table("rumi_refresh_map_points", n_kf, [&](int k) { return kf[k].n; }, pts, n_pts, obs_kf, obs_feature, n_obs,
                                     RUMI_REFRESH_MAX_OBS, &tooMany, reference_ok);
    if (rc != RUMI_OK) return rc;
    if (tooMany) {
        g_lastError = "rumi_refresh_map_points: a point has more than RUMI_REFRESH_MAX_OBS observations";
        return RUMI_E_CAPACITY;
    }
    if (n_pts == 0) return RUMI_OK;

    // ---- per-point records, bins by the number of rows left
    r->pt.resize(n_pts);
    for (auto &b : r->bins) b.clear();
    size_t nGoodAll = 0;
    int maxGood = 0;
    for (int i = 0; i < n_pts; i++) {
        const RumiRefreshPoint &P = pts[i];
        PtDev &d = r->pt[i];
        std::memcpy(d.pos, P.pos, 12);
        d.obsOff = P.obs_begin; d.nObs = P.obs_end - P.obs_begin;
        d.refKf = 0; d.scaleRef = d.scaleLast = 1.f;
        if (d.nObs > 0) {
            const RumiRefreshKF &R = kf[P.ref_kf];
            d.refKf = P.ref_kf; d.scaleRef = R.scale_factors[P.ref_level]; d.scaleLast = R.scale_factors[R.nlevels - 1];
        }
        d.descOff = (int32_t)nGoodAll; d.nGood = 0;
        if (wantDesc) {
            for (int o = P.obs_begin; o < P.obs_end; o++) d.nGood += !kf[obs_kf[o]].is_bad;
            nGoodAll += d.nGood;
            maxGood = std::max(maxGood, d.nGood);
            if (d.nGood > 0) r->bins[d.nGood <= 16 ? 0 : d.nGood <= 32 ? 1 : d.nGood <= 64 ? 2 : 3].push_back(i);
        }
    }
    size_t nBinned = 0;
    for (auto &b : r->bins) nBinned += b.size();
    // the workgroup kernel's points longest first: the long ones start early and the short ones fill in behind them
    std::stable_sort(r->bins[3].begin(), r->bins[3].end(), [&](int a, int b) { return r->pt[a].nGood > r->pt[b].nGood; });

    // ---- one block: points | camera centres | key-frame index of every observation | bin lists | position of every gathered row | rows
    const size_t offPts = 0, offOw = up16((size_t)n_pts * sizeof(PtDev)), offObs = offOw + up16((size_t)n_kf * 12),
                 offList = offObs + up16(wantNormal ? (size_t)n_obs * 4 : 0), offPos = offList + up16(nBinned * 4), offDesc = offPos + up16(nGoodAll * 4),
                 blkBytes = offDesc + nGoodAll * 32;
    const size_t outBytes = (size_t)n_pts * sizeof(OutDev);
    if ((rc = r->dev.bind()) != RUMI_OK || (rc = r->blk.reserve(blkBytes, blkBytes + blkBytes / 4)) != RUMI_OK ||
        (rc = r->out.reserve(outBytes, outBytes + outBytes / 4)) != RUMI_OK)
        return rc;
    OutDev *dOut = reinterpret_cast<OutDev *>(r->out.d);
    const OutDev *hOut = reinterpret_cast<const OutDev *>(r->out.h);
    uint8_t *h = r->blk.h;
    std::memcpy(h + offPts, r->pt.data(), (size_t)n_pts * sizeof(PtDev));
    float *hOw = reinterpret_cast<float *>(h + offOw);
    for (int k = 0; k < n_kf; k++) std::memcpy(hOw + 3 * k, kf[k].Ow, 12);
    if (wantNormal && n_obs > 0) std::memcpy(h + offObs, obs_kf, (size_t)n_obs * 4);
    int32_t *hList = reinterpret_cast<int32_t *>(h + offList);
    size_t binOff[4], at = 0;
    for (int b = 0; b < 4; b++) {
        binOff[b] = at;
        if (!r->bins[b].empty()) std::memcpy(hList + at, r->bins[b].data(), r->bins[b].size() * 4);
        at += r->bins[b].size();
    }
    if (wantDesc) {
        int32_t *hPos = reinterpret_cast<int32_t *>(h + offPos);
        uint8_t *hDesc = h + offDesc;
        size_t g = 0;
        for (int i = 0; i < n_pts; i++)
            for (int o = pts[i].obs_begin; o < pts[i].obs_end; o++) {
                const RumiRefreshKF &K = kf[obs_kf[o]];
                if (K.is_bad) continue;                          // :376
                hPos[g] = o - pts[i].obs_begin;
                std::memcpy(hDesc + 32 * g, K.desc + 32 * (size_t)obs_feature[o], 32);
                g++;
            }
    }
    r->clock.mark();
    HIP_TRY(hipMemcpyAsync(r->blk.d, r->blk.h, blkBytes, hipMemcpyHostToDevice, nullptr));

    // ---- the launches
    const PtDev *dPts = reinterpret_cast<const PtDev *>(r->blk.d + offPts);
    const int32_t *dList = reinterpret_cast<const int32_t *>(r->blk.d + offList), *dPos = reinterpret_cast<const int32_t *>(r->blk.d + offPos);
    const uint4 *dDesc = reinterpret_cast<const uint4 *>(r->blk.d + offDesc);
    if (wantDesc) {
        const int n0 = (int)r->bins[0].size(), n1 = (int)r->bins[1].size(), n2 = (int)r->bins[2].size(), n3 = (int)r->bins[3].size();
        if (n0) hipLaunchKernelGGL(k_refresh_desc_group<16>, dim3((n0 + 15) / 16), dim3(256), 0, nullptr, dPts, dList + binOff[0], n0, dDesc, dPos, dOut);
        if (n1) hipLaunchKernelGGL(k_refresh_desc_group<32>, dim3((n1 + 7) / 8), dim3(256), 0, nullptr, dPts, dList + binOff[1], n1, dDesc, dPos, dOut);
        if (n2) hipLaunchKernelGGL(k_refresh_desc_group<64>, dim3((n2 + 3) / 4), dim3(256), 0, nullptr, dPts, dList + binOff[2], n2, dDesc, dPos, dOut);
        if (n3) {
            const size_t lds = (size_t)maxGood * 32 + 4 * kHistStride * sizeof(int);     // at most 64 KiB + 4224 bytes
            if (lds > 64 * 1024) HIP_TRY(raise_lds_limit(reinterpret_cast<const void *>(k_refresh_desc_block), lds));
            hipLaunchKernelGGL(k_refresh_desc_block, dim3(n3), dim3(256), lds, nullptr, dPts, dList + binOff[3], maxGood, dDesc, dPos, dOut);
        }
    }
    if (wantNormal)
        hipLaunchKernelGGL(k_refresh_normal, dim3((n_pts + 255) / 256), dim3(256), 0, nullptr, dPts, n_pts, reinterpret_cast<const float *>(r->blk.d + offOw),
                           reinterpret_cast<const int32_t *>(r->blk.d + offObs), dOut);
    HIP_TRY(hipGetLastError());

    // ---- one block back; only the arrays of the modes asked for are written
    HIP_TRY(hipMemcpy(r->out.h, r->out.d, outBytes, hipMemcpyDeviceToHost));
    r->clock.mark();
    for (int i = 0; i < n_pts; i++) {
        const OutDev &o = hOut[i];
        if (wantDesc) {
            const bool has = r->pt[i].nGood > 0;                 // :367, :389: nothing is written for a point without a good observation
            best_obs[i] = has ? o.bestObs : -1;
            best_median[i] = has ? o.bestMedian : -1;
        }
        if (wantNormal) {
            updated[i] = r->pt[i].nObs > 0;
            if (r->pt[i].nObs > 0) {
                std::memcpy(normal + 3 * i, o.normal, 12);
                min_distance[i] = o.minD; max_distance[i] = o.maxD;
            }
        }
    }
    r->clock.finish(r->stageMs);
    return RUMI_OK;
}

extern "C" int rumi_refresh_stage_ms(const RumiRefresh *r, float *out3) {
    if (!r || !out3) return RUMI_E_INVALID;
    std::memcpy(out3, r->stageMs, sizeof r->stageMs);
    return RUMI_OK;
}

#include "refresh_resident.inc"
