// Device helpers the matcher kernels (match.hip) and the mapping kernels (mapping.hip) share.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "rumi_match.h"

namespace rumi {

__device__ __forceinline__ int hamming256(const uint32_t q[8], const uint32_t *d) {
    int s = 0;
#pragma unroll
    for (int k = 0; k < 8; k++) s += __popc(q[k] ^ d[k]);
    return s;
}

// inclusive prefix sum over the lanes of a wave by DPP (row prefix, row_bcast:15, row_bcast:31); lane 63 holds the total
__device__ __forceinline__ int wave_scan_incl_i32(int v) {
#define RUMI_DPP_ADD(ctl, rows) v += __builtin_amdgcn_update_dpp(0, v, ctl, rows, 0xf, false)
    RUMI_DPP_ADD(0x111, 0xf); RUMI_DPP_ADD(0x112, 0xf); RUMI_DPP_ADD(0x114, 0xf); RUMI_DPP_ADD(0x118, 0xf);
    RUMI_DPP_ADD(0x142, 0xa); RUMI_DPP_ADD(0x143, 0xc);
#undef RUMI_DPP_ADD
    return v;
}

__device__ __forceinline__ int rot_bin(float a, float b) {          // ORBmatcher.cc:1592-1599
    const float factor = 1.0f / RUMI_HISTO_LENGTH;
    float rot = a - b;
    if (rot < 0.0f) rot += 360.0f;
    int bin = (int)__builtin_roundf(rot * factor);
    if (bin == RUMI_HISTO_LENGTH) bin = 0;
    return bin;
}

// wave-wide maximum / sum of one 32-bit value by DPP (row prefix, row_bcast:15, row_bcast:31; the total sits in lane 63)
__device__ __forceinline__ uint32_t wave_max_u32(uint32_t v) {
#define RUMI_DPP_MAX(ctl, rows) v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, ctl, rows, 0xf, false))
    RUMI_DPP_MAX(0x111, 0xf); RUMI_DPP_MAX(0x112, 0xf); RUMI_DPP_MAX(0x114, 0xf); RUMI_DPP_MAX(0x118, 0xf);
    RUMI_DPP_MAX(0x142, 0xa); RUMI_DPP_MAX(0x143, 0xc);
#undef RUMI_DPP_MAX
    return (uint32_t)__builtin_amdgcn_readlane((int)v, 63);
}
__device__ __forceinline__ int wave_sum_i32(int v) { return __builtin_amdgcn_readlane(wave_scan_incl_i32(v), 63); }

}  // namespace rumi
