// MI355X-native Hamming matchers behind include/rumi_match.h.  One translation unit (the library is built without relocatable device code, so a
// kernel is launched from the unit that defines it): this file holds the matcher handle (RumiMatcher, create / destroy), the upload queue (stage_add,
// flush_uploads, reset_uploads, upload_frame with k_scatter and k_grid), track_speculation and the launchers match_host.h exports, and includes the
// kernels and the C entries by job.
//
// The reference walks map points / key-frame features one after another and lets each one see the
// assignments of the ones before it (ORBmatcher.cc:80-82, :248-249, :1556-1558).  GPU formulation, exact:
//   1. k_grid        Frame::AssignFeaturesToGrid as a key sort: (cell << 16 | feature) ascending, cell = ix*48+iy, so
//                    the cells GetFeaturesInArea visits for one ix are one contiguous range, already in its order.
//   2. k_queries_*   one query per map point / last-frame feature / key-frame feature (projection, window, levels).
//   3. k_candidates  one wave per query: enumerate candidates in the reference's order, 256-bit Hamming by
//                    xor + popcount, ballot-compacted into a per-query list (count pass, scan, fill pass).
//   4. k_resolve     one workgroup: every query picks its best candidate given "feature f is taken by an earlier
//                    query" (blockedFrom[f] = smallest blocking query index); iterate to the fix point.  After
//                    round k queries 0..k-1 hold their sequential result, and a fix point is the sequential result
//                    (induction on the query index), so the outcome equals the reference's loop bit for bit.
//                    Then the rotation histogram / ComputeThreeMaxima filter and the result arrays.
//   k_bruteforce_mfma  all-pairs best / second-best as an FP4 GEMM on the matrix cores.
//
//   match_queries.inc     k_queries_mappoints / frame / bow / sim3 / campoints / reloc / init, k_is_in_frustum (gates with one caller are written
//                         out here; the shared ones are match_device.h's)
//   match_candidates.inc  k_candidates<0 | 1 | 2> (candidates_walk, wave_bitonic_store, offsets_of), k_scan
//   match_resolve.inc     k_resolve (ResolveArgs, match_host.h), k_resolve_init (InitArgs)
//   match_reloc_batch.inc  k_reloc_walk<count | fill>, k_reloc_resolve: the relocalisation searches of every pose hypothesis (launch_reloc_search)
//   match_search.inc      host: build_lists, the list / resolve / retry loop, run_search; the rumi_search_* entries built on them,
//                         rumi_fuse_candidates, rumi_frame_is_in_frustum
//   match_tri.inc         k_tri_match, k_tri_filter (TriArgs) and rumi_search_for_triangulation
//   match_bruteforce.inc  k_bruteforce_mfma with its derivation, launch_bruteforce, rumi_match_bruteforce_*
//   match_bruteforce_pair.inc  k_bruteforce_pair (one pair, train rows split over workgroups, last-arriver merge), launch_bruteforce_pair,
//                         rumi_match_bruteforce_pair_*
//   match_bow_batch.inc   rumi_search_by_bow_batch: k_bowf_match and k_bow_rows_finish over the packed view
//   match_bow_kf_batch.inc  rumi_common_regions_bow: k_cr_match, k_bow_rows_finish and k_cr_union over the packed view, `first` cleared per call
//   match_submap.inc      k_grid_batch, k_submap_match, k_submap_compact (SubFrame, SubPair) and rumi_submap_match
//   match_device.h        what the kernels of match.hip, track.hip and mapping.hip share: Query, hamming256, the wave scans, rot_bin, one body per
//                         projection gate that has more than one caller (sim3_query, reloc_query, frustum_gate; se3f_camera_centre, pose_matrices19),
//                         ComputeThreeMaxima (three_maxima_keep by one thread, three_maxima_wave by one wave), bow_finish, block_ordered_slot
//   match_bow.h           the FeatureVector side of SearchByBoW: fv_find_node, bow_reduce16, bow_node_walk over a TakenMask or TakenLds
//   match_bow_stage.h     the two BoW batch stages, one body each for the host-pointer and the by-slot entries (track.hip, mapping.hip): the key-frame
//                         views, k_bowf_match, k_cr_match, k_bow_rows_finish, k_cr_union with its two `first` tables, and the host staging the two
//                         common-regions entries share
//   match_grid.h          grid_build_xy, the one-workgroup grid of k_grid_batch (shared with mapping.hip's k_sin_grid); the GetFeaturesInArea window of
//                         every walk: cell_window, window_gate, reproj_gate, and walk_window (16 lanes an item: mapping.hip's searches)
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "match_host.h"
#include "match_grid.h"
#include "match_bow_stage.h"

namespace rumi {

// ---- 1. grid -----------------------------------------------------------------------------------------------
// Frame::AssignFeaturesToGrid as a counting sort by cell (cell = column-major ix*48+iy, the order GetFeaturesInArea walks),
// ascending key-point index inside a cell (= push_back order).  One workgroup; the per-cell segments (a handful of entries) are
// put in index order by an insertion sort after an unordered atomic placement.
// (nDev: the feature count where the extractor left it, when the host has not read it yet; n is then its upper bound)
__global__ __launch_bounds__(1024) void k_grid(int n, const RumiKeyPoint *__restrict__ keys, float minX, float minY, float wInv,
                                               float hInv, uint16_t *__restrict__ sortedIdx, int32_t *__restrict__ cellStart, const int32_t *__restrict__ nDev) {
    if (nDev) n = min(n, *nDev);
    __shared__ int32_t sCnt[kGridCells + 1];
    __shared__ uint16_t sCell[kMaxSortN], sOut[kMaxSortN];
    __shared__ int32_t sWave[16];
    const int tid = threadIdx.x;
    for (int c = tid; c <= kGridCells; c += 1024) sCnt[c] = 0;
    __syncthreads();
    for (int i = tid; i < n; i += 1024) {
        // Frame::PosInGrid: round() of the float expression, dropped when outside the grid
        const int px = (int)__builtin_roundf((keys[i].x - minX) * wInv);
        const int py = (int)__builtin_roundf((keys[i].y - minY) * hInv);
        uint16_t cell = 0xFFFF;
        if (px >= 0 && px < kGridCols && py >= 0 && py < kGridRows) { cell = (uint16_t)(px * kGridRows + py); atomicAdd(&sCnt[cell], 1); }
        sCell[i] = cell;
    }
    __syncthreads();
    // exclusive scan of the 3072 counts: 3 cells per thread, a DPP scan inside each wave, the 16 wave totals through LDS (one barrier)
    constexpr int kPer = (kGridCells + 1023) / 1024;
    int loc[kPer], sum = 0;
#pragma unroll
    for (int k = 0; k < kPer; k++) { const int c = tid * kPer + k; loc[k] = c < kGridCells ? sCnt[c] : 0; sum += loc[k]; }
    const int incl = wave_scan_incl_i32(sum);
    if ((tid & 63) == 63) sWave[tid >> 6] = incl;
    __syncthreads();
    int before = 0, total = 0;
#pragma unroll
    for (int w = 0; w < 16; w++) { const int t = sWave[w]; total += t; if (w < (tid >> 6)) before += t; }
    int run = before + incl - sum;
#pragma unroll
    for (int k = 0; k < kPer; k++) {
        const int c = tid * kPer + k;
        if (c < kGridCells) { cellStart[c] = run; sCnt[c] = run; run += loc[k]; }
    }
    if (tid == 1023) cellStart[kGridCells] = total;
    __syncthreads();
    for (int i = tid; i < n; i += 1024) {
        const uint16_t cell = sCell[i];
        if (cell != 0xFFFF) sOut[atomicAdd(&sCnt[cell], 1)] = (uint16_t)i;
    }
    __syncthreads();
    // sCnt[c] is now the END of cell c; its start is the end of cell c-1 (or 0)
#pragma unroll
    for (int k = 0; k < kPer; k++) {
        const int c = tid * kPer + k;
        if (c >= kGridCells) continue;
        const int e = sCnt[c], b0 = e - loc[k];
        for (int i = b0 + 1; i < e; i++) {
            const uint16_t v = sOut[i];
            int j = i - 1;
            while (j >= b0 && sOut[j] > v) { sOut[j + 1] = sOut[j]; j--; }
            sOut[j + 1] = v;
        }
    }
    __syncthreads();
    for (int i = tid; i < total; i += 1024) sortedIdx[i] = sOut[i];
}

// ---- uploads: one pinned block per call, scattered to the arrays on the device ---------------------------------------------
__global__ __launch_bounds__(256) void k_scatter(const uint8_t *__restrict__ mirror, int nseg) {
    const Segment sg = reinterpret_cast<const Segment *>(mirror)[blockIdx.y];
    if ((int)blockIdx.y >= nseg) return;
    const uint32_t words = sg.bytes >> 2;
    const uint32_t *src = reinterpret_cast<const uint32_t *>(mirror + sg.off);
    uint32_t *dst = reinterpret_cast<uint32_t *>(sg.dst);
    for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < words; i += gridDim.x * 256) dst[i] = src[i];
    if (blockIdx.x == 0 && threadIdx.x < (sg.bytes & 3)) {
        const uint32_t k = (words << 2) + threadIdx.x;
        reinterpret_cast<uint8_t *>(sg.dst)[k] = mirror[sg.off + k];
    }
}

#include "match_queries.inc"
#include "match_candidates.inc"
#include "match_resolve.inc"
#include "match_reloc_batch.inc"

}  // namespace rumi

using namespace rumi;

// ================================================ host side =======================================================
extern "C" int rumi_descriptor_distance(const uint8_t *a, const uint8_t *b) {
    uint64_t x[4], y[4];
    std::memcpy(x, a, 32); std::memcpy(y, b, 32);
    return __builtin_popcountll(x[0] ^ y[0]) + __builtin_popcountll(x[1] ^ y[1]) + __builtin_popcountll(x[2] ^ y[2]) +
           __builtin_popcountll(x[3] ^ y[3]);
}

extern "C" void rumi_match_destroy(RumiMatcher *m) {
    if (!m) return;
    (void)hipSetDevice(m->device);
    if (m->ext.state && m->ext.destroy) m->ext.destroy(m->ext.state);
    void *p[] = {m->dKeys, m->dDesc, m->dScale, m->dSorted, m->dCellStart, m->dFvIdx, m->dQ, m->dQDesc, m->dCounts,
                 m->dOffsets, m->dOut, m->dU8a, m->dU8b, m->dF[0], m->dF[1], m->dF[2], m->dF[3],
                 m->dI[0], m->dI[1], m->dQKeys, m->dNodesA, m->dNodesB, m->dIdxA, m->dOffA, m->dOffB, m->dPose};
    for (void *q : p) if (q) (void)hipFree(q);
    if (m->hOut) (void)hipHostFree(m->hOut);
    delete m;
}

extern "C" int rumi_match_create(int32_t max_features, int32_t max_queries, int32_t device, RumiMatcher **out) {
    if (!out) return RUMI_E_INVALID;
    *out = nullptr;
    if (max_features < 1 || max_features > kMaxSortN || max_queries < 1) {
        g_lastError = "rumi_match_create: max_features must be in 1..16384, max_queries >= 1";
        return RUMI_E_INVALID;
    }
    int rc = require_device();
    if (rc != RUMI_OK) return rc;
    RumiMatcher *m = new RumiMatcher();
    if (device >= 0) m->device = device; else if (hipGetDevice(&m->device) != hipSuccess) m->device = 0;
    if (hipSetDevice(m->device) != hipSuccess) { delete m; return RUMI_E_NO_DEVICE; }
    m->maxFeat = max_features; m->maxQ = max_queries;
    const size_t F = max_features, Q = max_queries;
#define TRYA(x) if ((rc = (x)) != RUMI_OK) { rumi_match_destroy(m); return rc; }
    TRYA(dev_alloc(&m->dKeys, F)); TRYA(dev_alloc(&m->dDesc, F * 32)); TRYA(dev_alloc(&m->dScale, 64));
    TRYA(dev_alloc(&m->dSorted, F)); TRYA(dev_alloc(&m->dCellStart, kGridCells + 2));
    TRYA(dev_alloc(&m->dFvIdx, F));
    TRYA(dev_alloc(&m->dQ, Q)); TRYA(dev_alloc(&m->dQDesc, Q * 32)); TRYA(dev_alloc(&m->dCounts, Q + 1)); TRYA(dev_alloc(&m->dOffsets, Q + 1));
    const size_t listCap = (size_t)max_queries * 256 + 65536;     // grown on demand
    TRYA(m->lists.reserve(listCap, listCap));
    TRYA(dev_alloc(&m->dOut, 4 + F + Q));
    m->dNmatches = m->dOut; m->dOverflow = m->dOut + 1; m->dFeatMp = m->dOut + 4; m->dAssign = m->dOut + 4 + F;
    TRYA(dev_alloc(&m->dU8a, Q)); TRYA(dev_alloc(&m->dU8b, std::max(Q, F)));
    for (auto &f : m->dF) TRYA(dev_alloc(&f, Q * 3));
    for (auto &i : m->dI) TRYA(dev_alloc(&i, Q + 1));
    TRYA(dev_alloc(&m->dQKeys, Q)); TRYA(dev_alloc(&m->dNodesA, Q)); TRYA(dev_alloc(&m->dNodesB, F)); TRYA(dev_alloc(&m->dIdxA, Q));
    TRYA(dev_alloc(&m->dOffA, Q + 1)); TRYA(dev_alloc(&m->dOffB, F + 1)); TRYA(dev_alloc(&m->dPose, 32));
    const size_t stageBytes = kStageHeader + F * 112 + Q * 224 + 65536;
    TRYA(m->stage.reserve(stageBytes, stageBytes));
    if (hipHostMalloc((void **)&m->hOut, (4 + F + Q) * sizeof(int32_t), hipHostMallocDefault) != hipSuccess) {
        g_lastError = "rumi_match_create: pinned host allocation failed";
        rumi_match_destroy(m);
        return RUMI_E_NO_DEVICE;
    }
    m->stageUsed = kStageHeader;
#undef TRYA
    *out = m;
    return RUMI_OK;
}

namespace rumi {

uint8_t *stage_reserve(RumiMatcher *m, void *dst, size_t bytes) {
    const size_t off = (m->stageUsed + 15) & ~(size_t)15;
    if (m->nseg >= kMaxSegments || off + bytes > m->stage.cap) {
        g_lastError = "matcher upload block exhausted (raise max_features / max_queries)";
        return nullptr;
    }
    reinterpret_cast<Segment *>(m->stage.h)[m->nseg++] = Segment{dst, (uint32_t)off, (uint32_t)bytes};
    m->stageUsed = off + bytes;
    return m->stage.h + off;
}

int stage_add(RumiMatcher *m, void *dst, const void *src, size_t bytes) {
    if (bytes == 0) return RUMI_OK;
    uint8_t *h = stage_reserve(m, dst, bytes);
    if (!h) return RUMI_E_CAPACITY;
    std::memcpy(h, src, bytes);
    return RUMI_OK;
}

int flush_uploads(RumiMatcher *m) {
    if (m->nseg > 0) {
        HIP_TRY(hipMemcpyAsync(m->stage.d, m->stage.h, m->stageUsed, hipMemcpyHostToDevice, m->upStream));
        hipLaunchKernelGGL(k_scatter, dim3(8, m->nseg), dim3(256), 0, m->upStream, m->stage.d, m->nseg);
        m->nseg = 0;
        m->stageUsed = kStageHeader;
    }
    if (m->gridPending) {
        hipLaunchKernelGGL(k_grid, dim3(1), dim3(1024), 0, nullptr, m->gridN, m->gridKeys ? m->gridKeys : m->dKeys, m->gridMinX, m->gridMinY, m->gridWInv, m->gridHInv,
                           m->dSorted, m->dCellStart, m->gridNDev);
        m->gridPending = false;
        m->gridNDev = nullptr;
    }
    return RUMI_OK;
}

void reset_uploads(RumiMatcher *m) { m->nseg = 0; m->stageUsed = kStageHeader; m->gridPending = false; }

int upload_frame(RumiMatcher *m, const RumiFrameFeatures *F, FrameDev *fd) {
    reset_uploads(m);
    if (!F || F->n < 0 || F->n > m->maxFeat || F->nlevels < 1 || F->nlevels > 64 || !(F->max_x > F->min_x) || !(F->max_y > F->min_y)) {
        g_lastError = "bad RumiFrameFeatures (n, nlevels or bounds)";
        return RUMI_E_INVALID;
    }
    if (F->n > 0) { H2D(m->dKeys, F->keys_un, F->n); H2D(m->dDesc, F->desc, (size_t)F->n * 32); }
    H2D(m->dScale, F->scale_factors, F->nlevels);
    static const int32_t kZeroHeader[4] = {0, 0, 0, 0};     // result header [nmatches | list overflow | - | -]: cleared by the same scatter
    H2D(m->dOut, kZeroHeader, 4);
    fd->n = F->n; fd->keys = m->dKeys; fd->desc = m->dDesc;
    fd->minX = F->min_x; fd->minY = F->min_y; fd->maxX = F->max_x; fd->maxY = F->max_y;
    fd->wInv = (float)kGridCols / (float)(F->max_x - F->min_x);     // Frame.cc:322-323
    fd->hInv = (float)kGridRows / (float)(F->max_y - F->min_y);
    fd->sortedIdx = m->dSorted; fd->cellStart = m->dCellStart; fd->scale = m->dScale;
    m->gridPending = true; m->gridKeys = nullptr; m->gridN = F->n; m->gridMinX = fd->minX; m->gridMinY = fd->minY; m->gridWInv = fd->wInv; m->gridHInv = fd->hInv;
    return RUMI_OK;
}

const SearchSwitches &track_speculation() {
    static const SearchSwitches sw = [] {
        const char *spec = std::getenv("RUMI_TRACK_SPECULATE");
        const bool fused = std::getenv("RUMI_MATCH_NO_FUSED") == nullptr;
        return SearchSwitches{fused, fused && (spec ? std::atoi(spec) : 1) != 0};
    }();
    return sw;
}

void launch_queries_frame(RumiMatcher *m, const FrameDev &fd, int nlast, float th, hipStream_t st) {
    hipLaunchKernelGGL(k_queries_frame, dim3((nlast + 255) / 256), dim3(256), 0, st, nlast, m->dQKeys, m->dI[0], m->dU8a, m->dF[0], m->dI[1], m->dPose,
                       m->dPose + 7, m->dScale, th, fd.minX, fd.minY, fd.maxX, fd.maxY, m->dQ);
}
void launch_queries_bow(RumiMatcher *m, int nEntries, int nnKF, int nnF, const int32_t *nnFdev, hipStream_t st) {
    hipLaunchKernelGGL(k_queries_bow, dim3((std::max(nEntries, 1) + 255) / 256), dim3(256), 0, st, nnKF, m->dNodesA, m->dOffA, m->dIdxA, m->dI[0], m->dU8a,
                       m->dQKeys, nnF, m->dNodesB, m->dOffB, m->dQ, nnFdev);
}
void launch_resolve(const ResolveArgs &A, hipStream_t st) {
    hipLaunchKernelGGL(k_resolve, dim3(1), dim3(1024), (size_t)std::max(A.nfeat, 1) * sizeof(int32_t), st, A);
}
void launch_reloc_search(const RelocSearchArgs &A, hipStream_t st) {
    const dim3 gWalk((std::max(A.maxNkf, 1) + 3) / 4, A.H);
    hipLaunchKernelGGL(k_reloc_walk<false>, gWalk, dim3(256), 0, st, A);
    hipLaunchKernelGGL(k_reloc_walk<true>, gWalk, dim3(256), 0, st, A);
    hipLaunchKernelGGL(k_reloc_resolve, dim3(A.H), dim3(kRelocResolveThreads), (size_t)std::max(A.nfeat, 1) * sizeof(int32_t), st, A);
}

}  // namespace rumi

#include "match_search.inc"
#include "match_tri.inc"
#include "match_bruteforce.inc"
#include "match_bruteforce_pair.inc"
#include "match_bow_batch.inc"
#include "match_bow_kf_batch.inc"
#include "match_submap.inc"
