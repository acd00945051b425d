// The optical-flow stage of the PD frame selector (flow.hip) as the sampler (orb_host.hip, orb_kfd.inc) sees it: where the three LK levels of a
// frame and their Scharr derivatives lie in one device block each, and the launchers.  Not part of the C ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace rumi {

constexpr int kFlowLevels = 3;          // maxLevel 2
constexpr int kFlowWin = 31;            // winSize 31 x 31
constexpr int kFlowMinSide = 128;       // level 2 is then at least 32 pixels wide: one reflection covers the window's 31-pixel overshoot

// A frame block holds level l at byte `off[l]`, rows `pitch[l]` bytes apart (a multiple of 4: the extractor reads level 0 as aligned dwords); a
// derivative block holds level l at element `doff[l]`, one uint32 per pixel (dx in the low, dy in the high int16), rows w[l] elements apart.
struct FlowGeom {
    int w[kFlowLevels], h[kFlowLevels], pitch[kFlowLevels];
    int off[kFlowLevels], doff[kFlowLevels];
    int frameBytes, derivElems;
};
FlowGeom flow_geometry(int w, int h);

// BGR rows (bstride bytes apart) -> level 0 of `frame`.
void flow_launch_grey(const uint8_t *dBgr, int bstride, uint8_t *frame, const FlowGeom &g, hipStream_t st);
// Levels 1 and 2 from level 0 (one launch), then the Scharr derivative of all three levels (one launch).
void flow_launch_prepare(uint8_t *frame, uint32_t *deriv, const FlowGeom &g, hipStream_t st);
// n points of `pts` [n][2] tracked from (prevFrame, prevDeriv) to curFrame: out = [next n x 2 float | status n bytes] at outNext / outStatus.
void flow_launch_track(const uint8_t *prevFrame, const uint32_t *prevDeriv, const uint8_t *curFrame, const FlowGeom &g, const float *pts, int n, float *outNext,
                       uint8_t *outStatus, hipStream_t st);

}  // namespace rumi
