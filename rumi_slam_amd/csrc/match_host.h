// The matcher's host side as the other translation units of librumi_hip.so drive it (track.hip, mapping.hip): the handle, the upload queue,
// the candidate-list / resolve pipeline and host launchers of the matcher kernels they need.  Definitions: match.hip.  Not part of the C ABI.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "rumi_internal.h"
#include "rumi_common.h"
#include "rumi_match.h"
#include "match_device.h"

namespace rumi {

constexpr int kGridCols = 64, kGridRows = 48, kGridCells = kGridCols * kGridRows;   // Frame.h:42-43
enum { MODE_MAPPOINTS = 0, MODE_FRAME = 1, MODE_BOW = 2, MODE_BOW_KF = 3, MODE_SIM3 = 4, MODE_RELOC = 5, MODE_INIT = 6, MODE_FUSE = 7 };

struct FrameDev {
    int n;
    const RumiKeyPoint *keys;
    const uint8_t *desc;
    float minX, minY, maxX, maxY, wInv, hInv;
    const float *scale;          // mvScaleFactors
    const uint16_t *sortedIdx;   // features sorted by (cell, index)
    const int32_t *cellStart;    // [kGridCells + 1]
};

// uploads: one pinned block per call, scattered to the arrays on the device (k_scatter)
struct Segment { void *dst; uint32_t off, bytes; };
constexpr int kMaxSegments = 32;
constexpr size_t kStageHeader = kMaxSegments * sizeof(Segment);
// k_candidates<2>: a query has more candidates than its fixed slot holds; the host repeats the search with passes 0 / scan / 1
constexpr int kFusedOverflow = -0x40000000;

struct ResolveArgs {
    int mode, nq, nfeat;
    const Query *q;
    const int32_t *counts, *offsets;
    const uint32_t *lists;
    const RumiKeyPoint *featKeys;   // angles of the frame's key-points (rotation histogram)
    const int32_t *mpObs;           // Observations() per map point id (initial occupancy), may be null (BOW)
    int32_t *featMp;                // in: initial frame_mp (MODE 0/1); out: final ids   [nfeat]
    int32_t *assign;                // scratch [nq]: feature chosen by each query or -1
    int32_t *nmatches;              // out
    float nnratio;
    int checkOri;
    const uint8_t *featBlocked0;   // optional [nfeat]: feature unavailable from the start (overrides the featMp/mpObs rule)
    float thrF;                    // MODE_SIM3: TH_LOW * ratioHamming
    int thrI;                      // MODE_RELOC: ORBdist
    const int32_t *overflow;       // set by the fill pass when the list arena is too small: nothing to resolve
    // optional tail (the Tracking step): PoseOptimization's correspondences gathered from the vector this search leaves (k_track_gather's work,
    // one launch less between the search and the optimisation); gXw == nullptr: none
    const float *gMpPos, *gInvSigma2;
    float *gXw, *gObs, *gW;
    int32_t *gIdx, *gStart, *gSnapshot;
};

}  // namespace rumi

struct RumiMatcher {
    int device = 0, maxFeat = 0, maxQ = 0;
    size_t listCap = 0;
    // frame (train) side
    RumiKeyPoint *dKeys = nullptr; uint8_t *dDesc = nullptr; float *dScale = nullptr;
    uint16_t *dSorted = nullptr; int32_t *dCellStart = nullptr;
    uint32_t *dFvIdx = nullptr;      // frame FeatureVector indices (BoW)
    // query side
    rumi::Query *dQ = nullptr; uint8_t *dQDesc = nullptr; int32_t *dCounts = nullptr, *dOffsets = nullptr;
    uint32_t *dLists = nullptr;
    // results, one block so that one copy brings them back: [nmatches, list overflow, -, -][featMp maxFeat][assign maxQ]
    int32_t *dOut = nullptr, *hOut = nullptr;
    int32_t *dNmatches = nullptr, *dOverflow = nullptr, *dFeatMp = nullptr, *dAssign = nullptr;     // views into dOut
    // raw inputs of the query builders
    uint8_t *dU8a = nullptr, *dU8b = nullptr; float *dF[6] = {nullptr}; int32_t *dI[4] = {nullptr};
    RumiKeyPoint *dQKeys = nullptr; uint32_t *dNodesA = nullptr, *dNodesB = nullptr, *dIdxA = nullptr;
    int32_t *dOffA = nullptr, *dOffB = nullptr;
    float *dPose = nullptr;
    // uploads of one call: packed into a pinned block, copied once, scattered on the device (k_scatter)
    uint8_t *hStage = nullptr, *dStage = nullptr;
    size_t stageCap = 0, stageUsed = 0;
    int nseg = 0;
    // rumi_search_by_bow_batch: one pinned block up, one result block back (grown on demand)
    uint8_t *hBow = nullptr, *dBow = nullptr; size_t bowCap = 0;
    uint8_t *hBowOut = nullptr, *dBowOut = nullptr; size_t bowOutCap = 0;
    // k_grid of the uploaded frame, launched by flush_uploads once the key-points are in place
    const int32_t *gridNDev = nullptr;     // k_grid reads the count from the device (one call only: cleared by the flush)
    hipStream_t upStream = nullptr;        // where the next flush queues its copy and scatter (the caller orders its kernels behind them)
    bool gridPending = false; int gridN = 0; float gridMinX = 0, gridMinY = 0, gridWInv = 0, gridHInv = 0;
    const RumiKeyPoint *gridKeys = nullptr;      // key-points k_grid reads: dKeys, or a frame that already lies on the device (rumi_track_frame)
    rumi::MatcherExt ext;                  // arenas of rumi_create_new_map_points (mapping.hip), released with the matcher
};

namespace rumi {

template <class T> int dalloc(T **p, size_t n) {
    *p = nullptr;
    HIP_TRY(hipMalloc((void **)p, std::max<size_t>(n, 1) * sizeof(T)));
    return RUMI_OK;
}

// Queue `bytes` of host data for the array `dst`; nothing moves until flush_uploads.
int stage_add(RumiMatcher *m, void *dst, const void *src, size_t bytes);
// One host-to-device copy for everything queued, the scatter, then the grid of the uploaded frame.
int flush_uploads(RumiMatcher *m);
// A call that fails between stage_add and flush must not leak its queue into the next one.
void reset_uploads(RumiMatcher *m);
// Queues a frame's key-points, descriptors, scale table and the cleared result header; its grid is built by the next flush.
int upload_frame(RumiMatcher *m, const RumiFrameFeatures *F, FrameDev *fd);
// count pass, scan, fill pass (fused: all three in one launch, every list in a fixed slot).  Flushes the queue first.
int build_lists(RumiMatcher *m, int mode, int nq, const FrameDev &fd, const uint8_t *dQueryDesc, bool retry, bool fused);
// candidate lists, then the fix-point resolve; brings the results to the host (and synchronises the null stream)
int run_search(RumiMatcher *m, int mode, int nq, const FrameDev &fd, const uint8_t *dQueryDesc, const int32_t *dMpObs, float nnratio, int checkOri,
               int32_t *hostFeatMp, int32_t *nmatchesOut, const uint8_t *dBlocked0 = nullptr, float thrF = 0.f, int thrI = 0, int32_t *hostAssign = nullptr);
// (`m` is the matcher in scope; both return from the calling function on failure)
#define H2D(dst, src, n) do { const int rcS_ = rumi::stage_add(m, (dst), (src), (size_t)(n) * sizeof(*(dst))); if (rcS_ != RUMI_OK) return rcS_; } while (0)
#define FLUSH(m) do { const int rcF_ = rumi::flush_uploads(m); if (rcF_ != RUMI_OK) return rcF_; } while (0)

// The two environment switches of the search pipeline, read once per process.  fused: every query's list in a fixed slot (RUMI_MATCH_NO_FUSED set:
// count / scan / fill).  speculate: the Tracking entries queue a whole step without reading a count back (RUMI_TRACK_SPECULATE=0 or not fused: no).
struct SearchSwitches { bool fused, speculate; };
const SearchSwitches &track_speculation();

// The library is built without relocatable device code: a kernel is launched from the file that defines it.  These only launch, on the
// matcher's own arrays (the staged inputs of k_queries_frame / k_queries_bow lie where every caller's uploads put them).
void launch_queries_frame(RumiMatcher *m, const FrameDev &fd, int nlast, float th, hipStream_t st);
// (nEntries = the key-frame FeatureVector's entry count as the host knows it: one thread per entry; nnFdev: the frame's node count on the device, or null)
void launch_queries_bow(RumiMatcher *m, int nEntries, int nnKF, int nnF, const int32_t *nnFdev, hipStream_t st);
void launch_resolve(const ResolveArgs &A, hipStream_t st);

}  // namespace rumi
