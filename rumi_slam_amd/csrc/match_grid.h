// The 64 x 48 grid of one frame by one workgroup, for the kernels that build many grids in one launch, and the window every search walks in
// such a grid (match.hip, mapping.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "match_device.h"
#include "match_host.h"

namespace rumi {

constexpr int kMaxSortN = 16384;     // features per frame: the mono-initialisation extractor asks for 5 x nfeatures (Tracking.cc:581: 10 000 with TUM3.yaml)

// Frame::AssignFeaturesToGrid for one frame by one workgroup of 1024: k_grid's counting sort by cell (column-major, ascending key-point index inside a
// cell), restated here over x, y pairs that lie STRIDE floats apart: 2 for the packed points of rumi_submap_match (k_grid_batch, match_submap.inc), 7 for
// whole RumiKeyPoint records where the covisibility store keeps them (k_sin_grid, search_in_neighbors.inc).  (Giving k_grid and this function one
// body moved k_grid's LDS arrays and rescheduled its scan; k_grid stays as it is.)
template <int STRIDE>
__device__ __forceinline__ void grid_build_xy(int n, const float *__restrict__ xy, float minX, float minY, float wInv, float hInv, uint16_t *__restrict__ sortedIdx,
                                           int32_t *__restrict__ cellStart) {
    __shared__ int32_t sCnt[kGridCells + 1];
    __shared__ uint16_t sCell[kMaxSortN], sOut[kMaxSortN];
    __shared__ int32_t sWave[16];
    const int tid = threadIdx.x;
    for (int c = tid; c <= kGridCells; c += 1024) sCnt[c] = 0;
    __syncthreads();
    for (int i = tid; i < n; i += 1024) {
        // Frame::PosInGrid: round() of the float expression, dropped when outside the grid
        const int px = (int)__builtin_roundf((xy[STRIDE * i] - minX) * wInv);
        const int py = (int)__builtin_roundf((xy[STRIDE * i + 1] - minY) * hInv);
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

// ---- the window of Frame::GetFeaturesInArea (Frame.cc:695-750; KeyFrame.cc:887-925) and its per-candidate tests --------------------------------
// The cell range of the window (u, v) +- r, clamped, and whether the member gets past its early returns.  `any` also asks for y1 >= y0, which the
// reference does not test: cellStart is a non-decreasing prefix over column-major cells, so y1 < y0 makes a column's range [cellStart[ix * rows + y0],
// cellStart[ix * rows + y1 + 1]) end at or before its start and every walk of it empty, as the reference's two nested cell loops are.  A walk may
// therefore test it or not; the fast path of k_candidates takes the LENGTH of that range and needs it, so the one form tests it everywhere.
struct CellWindow { int x0, x1, y0, y1; bool any; };
__device__ __forceinline__ CellWindow cell_window(float u, float v, float r, float minX, float minY, float wInv, float hInv) {
    CellWindow w;
    w.x0 = max(0, (int)floorf((u - minX - r) * wInv));
    w.x1 = min(kGridCols - 1, (int)ceilf((u - minX + r) * wInv));
    w.y0 = max(0, (int)floorf((v - minY - r) * hInv));
    w.y1 = min(kGridRows - 1, (int)ceilf((v - minY + r) * hInv));
    w.any = w.x0 < kGridCols && w.x1 >= 0 && w.y0 < kGridRows && w.y1 >= 0 && w.y1 >= w.y0;
    return w;
}

// the member's own test of a candidate against the window (the cells overhang it), and with the level range of the members that have one
__device__ __forceinline__ bool window_gate(float x, float y, float u, float v, float r) {
    const float dx = x - u, dy = y - v;
    return fabsf(dx) < r && fabsf(dy) < r;
}
__device__ __forceinline__ bool window_gate(const RumiKeyPoint &kp, float u, float v, float r, int minLevel, int maxLevel) {
    return !(kp.octave < minLevel) && !(kp.octave > maxLevel) && window_gate(kp.x, kp.y, u, v, r);
}

// the monocular reprojection gate of Fuse (ORBmatcher.cc:1138-1145): chi2 at the candidate's level against 5.99, in the reference's types
__device__ __forceinline__ bool reproj_gate(const RumiKeyPoint &kp, float u, float v, const float *scale) {
    const float ex = u - kp.x, ey = v - kp.y;
    const float e2 = ex * ex + ey * ey;
    const float s2 = scale[kp.octave] * scale[kp.octave];                  // mvLevelSigma2; mvInvLevelSigma2 = 1.0f / it
    return !((double)(e2 * (1.0f / s2)) > 5.99);
}

// One frame's grid as a walk reads it.
struct GridView {
    const RumiKeyPoint *keys; const uint16_t *sorted; const int32_t *cellStart;
    float minX, minY, wInv, hInv;
};

// The window walk by LANES lanes per item (sub: this lane's place among them): the candidates in the member's order (cell column, cell row, ascending
// feature index) that pass window_gate, each handed to visit(feature, key-point, place in the walk).  The place grows along the walk (a column's
// range rounded up to whole trips of LANES), so it orders the candidates as the reference meets them, whichever lane sees which.
template <int LANES, class Visit>
__device__ __forceinline__ void walk_window(const GridView &G, float u, float v, float r, int minLevel, int maxLevel, int sub, Visit &&visit) {
    const CellWindow W = cell_window(u, v, r, G.minX, G.minY, G.wInv, G.hInv);
    if (!W.any) return;
    int order = 0;
    for (int ix = W.x0; ix <= W.x1; ix++) {
        const int p0 = G.cellStart[ix * kGridRows + W.y0], p1 = G.cellStart[ix * kGridRows + W.y1 + 1];
        for (int base = p0; base < p1; base += LANES, order += LANES) {
            const int c = base + sub;
            if (c >= p1) continue;
            const int idx = G.sorted[c];
            const RumiKeyPoint kp = G.keys[idx];
            if (window_gate(kp, u, v, r, minLevel, maxLevel)) visit(idx, kp, order + sub);
        }
    }
}

}  // namespace rumi
