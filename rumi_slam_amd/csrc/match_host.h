// The matcher's host side as the other translation units of librumi_hip.so drive it (track.hip, mapping.hip): the handle, the upload queue and
// the stagers that fill it, the candidate-list / resolve pipeline and host launchers of the matcher kernels they need.  Definitions: match.hip
// (handle, queue, launchers) and match_search.inc (build_lists, run_search), which match.hip includes.  Not part of the C ABI.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstring>

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
    // frame (train) side
    RumiKeyPoint *dKeys = nullptr; uint8_t *dDesc = nullptr; float *dScale = nullptr;
    uint16_t *dSorted = nullptr; int32_t *dCellStart = nullptr;
    uint32_t *dFvIdx = nullptr;      // frame FeatureVector indices (BoW)
    // query side
    rumi::Query *dQ = nullptr; uint8_t *dQDesc = nullptr; int32_t *dCounts = nullptr, *dOffsets = nullptr;
    rumi::DevBuf<uint32_t> lists;    // the candidate lists of every query: sized by rumi_match_create, grown once by a search that overflows it
    // results, one block so that one copy brings them back: [nmatches, list overflow, -, -][featMp maxFeat][assign maxQ]
    int32_t *dOut = nullptr, *hOut = nullptr;
    int32_t *dNmatches = nullptr, *dOverflow = nullptr, *dFeatMp = nullptr, *dAssign = nullptr;     // views into dOut
    // raw inputs of the query builders
    uint8_t *dU8a = nullptr, *dU8b = nullptr; float *dF[4] = {nullptr}; int32_t *dI[2] = {nullptr};
    RumiKeyPoint *dQKeys = nullptr; uint32_t *dNodesA = nullptr, *dNodesB = nullptr, *dIdxA = nullptr;
    int32_t *dOffA = nullptr, *dOffB = nullptr;
    float *dPose = nullptr;
    // uploads of one call: packed into a pinned block, copied once, scattered on the device (k_scatter)
    rumi::MirrorBuf<uint8_t> stage;          // sized by rumi_match_create; rumi_submap_match grows it for its one block
    size_t stageUsed = 0;
    int nseg = 0;
    // rumi_search_by_bow_batch: one pinned block up, one result block back (grown on demand)
    rumi::MirrorBuf<uint8_t> bow, bowOut;
    // rumi_submap_match: frame / pair tables, uploaded key-points, grids and block counts in dSub; one result block back (grown on demand)
    rumi::DevBuf<uint8_t> sub;
    rumi::MirrorBuf<uint8_t> subOut;
    // rumi_common_regions_bow: one pinned block up, one result block back (grown on demand); the last call's event times when profiling is on
    rumi::MirrorBuf<uint8_t> crb, crbOut;
    bool crbProfile = false;
    float crbMs[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
    // k_grid of the uploaded frame, launched by flush_uploads once the key-points are in place
    const int32_t *gridNDev = nullptr;     // k_grid reads the count from the device (one call only: cleared by the flush)
    hipStream_t upStream = nullptr;        // where the next flush queues its copy and scatter (the caller orders its kernels behind them)
    bool gridPending = false; int gridN = 0; float gridMinX = 0, gridMinY = 0, gridWInv = 0, gridHInv = 0;
    const RumiKeyPoint *gridKeys = nullptr;      // key-points k_grid reads: dKeys, or a frame that already lies on the device (rumi_track_frame)
    rumi::MatcherExt ext;                  // arenas of rumi_create_new_map_points (mapping.hip), released with the matcher
};

namespace rumi {

// Queue `bytes` of host data for the array `dst`; nothing moves until flush_uploads.
int stage_add(RumiMatcher *m, void *dst, const void *src, size_t bytes);
// The same for a caller that packs the bytes itself: the place in the pinned block that will land on `dst`, or nullptr when the block is full.
uint8_t *stage_reserve(RumiMatcher *m, void *dst, size_t bytes);
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
// (`m` is the matcher in scope; all three return from the calling function on failure)
#define RC_TRY(call) do { const int rcT_ = (call); if (rcT_ != RUMI_OK) return rcT_; } while (0)
#define H2D(dst, src, n) RC_TRY(rumi::stage_add(m, (dst), (src), (size_t)(n) * sizeof(*(dst))))
#define FLUSH(m) RC_TRY(rumi::flush_uploads(m))

// ---- stagers: these only queue into the matcher's upload block; the order of the segments fixes the offsets inside the staged block ----
// The three pose packs of the query builders and the frustum test, into dPose.
inline int stage_pose(RumiMatcher *m, const float *Tcw7, const float *K4) {                                       // Tcw7 | K4
    float pose[11];
    std::memcpy(pose, Tcw7, 28); std::memcpy(pose + 7, K4, 16);
    H2D(m->dPose, pose, 11);
    return RUMI_OK;
}
inline int stage_pose_ow(RumiMatcher *m, const float *Tcw7, const float *K4, const float *Ow3) {                  // Tcw7 | K4 | Ow3
    float pose[14];
    std::memcpy(pose, Tcw7, 28); std::memcpy(pose + 7, K4, 16); std::memcpy(pose + 11, Ow3, 12);
    H2D(m->dPose, pose, 14);
    return RUMI_OK;
}
inline int stage_pose_matrices(RumiMatcher *m, const float *Rcw9, const float *tcw3, const float *Ow3, const float *K4) {   // Rcw9 | tcw3 | Ow3 | K4
    float pose[19];
    std::memcpy(pose, Rcw9, 36); std::memcpy(pose + 9, tcw3, 12); std::memcpy(pose + 12, Ow3, 12); std::memcpy(pose + 15, K4, 16);
    H2D(m->dPose, pose, 19);
    return RUMI_OK;
}
// the last frame of k_queries_frame
inline int stage_last_frame(RumiMatcher *m, const RumiKeyPoint *last_keys_un, int nlast, const int32_t *last_mp, const uint8_t *last_outlier) {
    if (nlast > 0) { H2D(m->dQKeys, last_keys_un, nlast); H2D(m->dI[0], last_mp, nlast); H2D(m->dU8a, last_outlier, nlast); }
    return RUMI_OK;
}
// The key-frame on the query side of the FeatureVector searches (k_queries_bow, k_tri_match): its features, then (behind whatever the entry queues in
// between) its FeatureVector in CSR form; and the FeatureVector of the frame side.  nEntries = offsets[n_nodes], 0 without nodes.
inline int stage_query_keyframe(RumiMatcher *m, const RumiFrameFeatures *KF, const int32_t *kf_mp) {
    if (KF->n > 0) { H2D(m->dQKeys, KF->keys_un, KF->n); H2D(m->dQDesc, KF->desc, (size_t)KF->n * 32); H2D(m->dI[0], kf_mp, KF->n); }
    return RUMI_OK;
}
inline int stage_fv(RumiMatcher *m, const RumiFeatureVector *fv, int nEntries, uint32_t *dNodes, int32_t *dOff, uint32_t *dIdx) {
    if (fv->n_nodes > 0) { H2D(dNodes, fv->node_ids, fv->n_nodes); H2D(dOff, fv->offsets, fv->n_nodes + 1); }
    if (nEntries > 0) H2D(dIdx, fv->indices, nEntries);
    return RUMI_OK;
}
inline int stage_fv_query(RumiMatcher *m, const RumiFeatureVector *fv, int nEntries) { return stage_fv(m, fv, nEntries, m->dNodesA, m->dOffA, m->dIdxA); }
inline int stage_fv_frame(RumiMatcher *m, const RumiFeatureVector *fv, int nEntries) { return stage_fv(m, fv, nEntries, m->dNodesB, m->dOffB, m->dFvIdx); }

// The result block of the frustum test for nmp points, as k_is_in_frustum and k_track_frustum write it into dStage (its uploads have been scattered
// by then) and as one copy brings it to hStage: [inView u8 | X | Y | cos | depth f32 | level i32], every array n16 = nmp rounded up to 16 entries
// long, 21 bytes a point.
struct FrustumBlock {
    size_t n16, bytes;
    uint8_t *inView; float *x, *y, *viewCos, *depth; int32_t *level;
    FrustumBlock(uint8_t *base, int nmp)
        : n16(((size_t)nmp + 15) & ~(size_t)15), bytes(n16 * 21), inView(base), x(reinterpret_cast<float *>(base + n16)), y(reinterpret_cast<float *>(base + n16 * 5)),
          viewCos(reinterpret_cast<float *>(base + n16 * 9)), depth(reinterpret_cast<float *>(base + n16 * 13)), level(reinterpret_cast<int32_t *>(base + n16 * 17)) {}
    // a host copy into the caller's arrays
    void unpack(int nmp, uint8_t *inViewOut, float *xOut, float *yOut, int32_t *levelOut, float *cosOut, float *depthOut) const {
        std::memcpy(inViewOut, inView, (size_t)nmp);
        std::memcpy(xOut, x, (size_t)nmp * 4); std::memcpy(yOut, y, (size_t)nmp * 4); std::memcpy(cosOut, viewCos, (size_t)nmp * 4);
        std::memcpy(depthOut, depth, (size_t)nmp * 4); std::memcpy(levelOut, level, (size_t)nmp * 4);
    }
};
inline bool frustum_fits(const RumiMatcher *m, int nmp) { return FrustumBlock(m->stage.d, nmp).bytes <= m->stage.cap; }

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

// ---- rumi_track_reloc_refine: what its stage kernels in track.hip (track_reloc.inc) and match.hip (match_reloc_batch.inc) share ----
enum { RELOC_LIVE_S1 = 1, RELOC_LIVE_P2 = 2, RELOC_LIVE_S2 = 4, RELOC_LIVE_P3 = 8 };     // RelocHyp.live: the stage still has this hypothesis to do
struct RelocHyp {                        // one hypothesis on the device; its first 14 words are RumiRelocResult
    int32_t ran, ngood[3], nadd[2], ngoodFinal;
    float T[7];
    int32_t cand, live;
};
static_assert(sizeof(RelocHyp) == 64, "a record of the result block");
struct RelocCand { int32_t nkf, keyOff; };               // a candidate's key-points and map-point row inside the session's concatenated arrays
// One SearchByProjection(F, pKF, sFound, th, ORBdist) stage for every hypothesis whose live bit is set (stage 0: S1, 1: S2): queries and
// candidate count, fill, one ordered resolve per hypothesis, which also takes the stage's decision (`nGood + nadditional >= enough`).
struct RelocSearchArgs {
    int H, nfeat, words, maxNkf, stage;
    RelocHyp *hyp;
    const RelocCand *cands;
    const RumiKeyPoint *kfKeys;          // all candidates' key-points, a candidate's at keyOff
    const int32_t *kfMp;                 // likewise their rows
    const float *pos, *minD, *maxD;      // the point table
    const uint8_t *desc, *bad;
    const uint32_t *found;               // [H][words] sFound as a bitmap over table ids
    const float *T;                      // [H][7] the current poses
    float K[4];
    FrameDev fd;
    int nLevels;
    float logSf, th;
    int orbDist, checkOri, enough;
    Query *q;                            // [H][maxNkf]
    int32_t *pairCount, *pairBase, *asg; // [H][maxNkf] candidates of a pair, where its list starts, the feature it holds
    int32_t *head;                       // [0 / 1] candidates of S1 / S2 in all
    uint2 *lists;
    int listCap;
    int32_t *featMp;                     // [H][nfeat]
};
void launch_reloc_search(const RelocSearchArgs &A, hipStream_t st);

}  // namespace rumi
