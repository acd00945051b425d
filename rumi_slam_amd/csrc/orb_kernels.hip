// HIP kernels of the ORB front-end for gfx950 (wave64).  See DESIGN.md for the data layout and the
// roofline of each kernel.  Built with -ffp-contract=off: the float steering math of rBRIEF and the
// atan polynomial must round exactly like the reference's x86-64 SSE code.
//
// Reference behaviour restated per kernel (R/ = /root/reference/src/rumi-slam/):
//   k_resize        cv::resize INTER_LINEAR 8U, level l from level l-1   R/lib_src/ORBextractor.cc:1103
//   k_fast_cells    per-cell cv::FAST(iniTh | minTh, NMS)                R/lib_src/ORBextractor.cc:748-807
//   k_compact       concatenation of the cell results in cell order      R/lib_src/ORBextractor.cc:796-803
//   k_blur          cv::GaussianBlur 7x7 sigma 2, REFLECT_101             R/lib_src/ORBextractor.cc:1057-1058
//   k_orient_desc   IC_Angle + computeOrbDescriptor + output assembly    R/lib_src/ORBextractor.cc:73-143,1067-1088
//   k_disc_angle    IC_Angle and the angle's cos / sin for batches         R/lib_src/ORBextractor.cc:73-97,101-104
//
// One translation unit (the library is built without relocatable device code, so a kernel is launched from the unit that defines it).  This file
// holds what the parts share -- the rBRIEF pattern, xcd_swizzle, U32 / U64, level_base, reflect101, pack_span -- and includes the kernels by job,
// each with its launch wrappers (orb_device.h; called from orb_schedule.inc) behind it.  The order matters: k_fast_blur (orb_blur.inc) fuses
// fast_cells_body (orb_fast.inc) and blur_body.
//   orb_pyramid.inc      k_resize, k_pyramid_tiles; launch_resize, launch_pyramid_tiles
//   orb_fast.inc         FastLds, quick test, exact score, ring, k_fast_cells, k_compact; fast_lds_of, launch_fast, launch_compact
//   orb_blur.inc         BlurGrid / BlurPack, blur_body, k_blur, k_blur_packed, k_fast_blur; the grid builders, launch_blur, launch_fast_blur,
//                        fast_blur_fusable
//   orb_orient_desc.inc  k_orient_desc (AssembleArgs), k_disc_angle; launch_orient_desc, launch_disc_angle, launch_assemble_orient_desc
#include <hip/hip_runtime.h>

#include <algorithm>

#include "orb_device.h"
#include "orb_math.h"
#include "orb_octree.h"

namespace rumi {

// the 256 rBRIEF test pairs (x0, y0, x1, y1) as floats: a lane fetches its pair with one 16-byte load and no conversions
struct PatternF { float v[256 * 4]; };
constexpr PatternF make_pattern_f() {
    constexpr int8_t src[256 * 4] = {
#include "orb_pattern.inc"
    };
    PatternF p{};
    for (int i = 0; i < 256 * 4; i++) p.v[i] = (float)src[i];
    return p;
}
__constant__ PatternF c_patternF = make_pattern_f();

// XCD-aware workgroup placement (cdna_hip_programming.md T1): the dispatcher deals consecutive workgroups round-robin over
// the 8 XCDs, each with a private L2.  Remapping the linear workgroup id with this bijection gives every XCD one contiguous
// range of logical ids, so neighbouring tiles of one frame (which share 64-B lines and halo rows) meet in the same L2.
// Placement only changes speed / HBM traffic, never results.
__device__ __forceinline__ unsigned xcd_swizzle(unsigned lin, unsigned total) {
    const unsigned q = total >> 3, r = total & 7, xcd = lin & 7;
    return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (lin >> 3);
}

struct __attribute__((packed)) U32 { uint32_t v; };      // possibly unaligned 4-byte global access
struct __attribute__((packed)) U64 { uint64_t v; };      // possibly unaligned 8-byte global access
constexpr int kPyrLevels = 8, kPyrWinPasses = 20;        // k_pyramid_tiles: levels it is offered for, 4-row passes of its level-0 window

// pixel (0,0) of a pyramid level: level 0 is the caller's frame itself, the others live in the pyramid arena
__device__ __forceinline__ const uint8_t *level_base(const ImgSrc &s, const DevParams *P, int level, int frame,
                                                      int *pitch) {
    if (level == 0) {
        *pitch = s.l0Pitch;
        return s.l0 + (long long)frame * s.l0FrameStride;
    }
    *pitch = P->lv[level].pitch;
    return s.pyr + (long long)frame * P->arenaStride + P->lv[level].off;
}

__device__ __forceinline__ int reflect101(int i, int n) {
    if (n == 1) return 0;
    while (i < 0 || i >= n) i = i < 0 ? -i : 2 * (n - 1) - i;
    return i;
}

// bytes from a frame to the next for the lane packing's 32-bit frame offsets: the arena's, and the caller's frames' where level 0 is read
// (0: not packable -- a caller's stride that is not positive)
static long long pack_span(const DevParams &hP, const ImgSrc &src, bool readsLevel0) {
    if (readsLevel0 && src.l0FrameStride <= 0) return 0;
    return readsLevel0 ? std::max(hP.arenaStride, src.l0FrameStride) : hP.arenaStride;
}

}  // namespace rumi

#include "orb_pyramid.inc"
#include "orb_fast.inc"
#include "orb_blur.inc"
#include "orb_orient_desc.inc"
