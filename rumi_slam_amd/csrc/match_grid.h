// The 64 x 48 grid of one frame by one workgroup, for the kernels that build many grids in one launch (match.hip, mapping.hip).
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

}  // namespace rumi
