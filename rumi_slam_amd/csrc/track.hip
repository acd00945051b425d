// One device-resident Tracking step behind include/rumi_track.h (kernels + host side): the extractor's record, the matcher's grid and
// map-point vector (mvpMapPoints = dFeatMp) and the pose optimiser's correspondence arrays never leave HBM between the five stages.  A dispatch
// costs about 4.5 us on the device whatever it does, so the step is built from as few as the data flow allows: no device-to-device copies (the
// matcher reads the extractor's record in place, results are produced inside the block that travels back), fills and bookkeeping folded into
// neighbouring kernels.  The matcher is driven through match_host.h (upload queue and stagers, the frustum result block, run_search); its kernels are
// launched by match.hip's launchers.  track_reloc.inc (included at the end): Tracking::Relocalization's refine chain for every pose hypothesis of a
// round in one call (rumi_track_reloc_begin / rumi_track_reloc_refine).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "match_host.h"
#include "match_bow_stage.h"
#include "rumi_orb.h"
#include "rumi_track.h"
#include "rumi_voc.h"

namespace rumi {

struct TrackBlock {                  // the result block's header, device and pinned host alike (arrays follow at byte offsets of RumiTracker)
    float Tout[14];                  // pose after the motion model | after the local map
    float pose19[20];                // Rcw9 tcw3 Ow3 K4 of the first (Frame::UpdatePoseMatrices)
    int32_t nGood[2];                // PoseOptimization return values
    int32_t counters[2];             // nmatchesMap, mnMatchesInliers
    int32_t start[2];                // correspondences of the optimisation in flight: {0, count}
    int32_t spec[4];                 // speculative step: result header (matches, overflow word) of the motion search | of the local search
};

// fill(mvpMapPoints, NULL), cleared flags / counters, both poses = the prediction, result header of the search cleared
__global__ void k_track_init(int n, int nmp, int full, int32_t *featMp, int32_t *searchHeader, uint8_t *seen, uint8_t *outF, int32_t *mpOut, const float *Tpred,
                             TrackBlock *blk) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) { featMp[i] = -1; if (full) { outF[i] = 0; mpOut[i] = -1; } }
    if (full && i < nmp) seen[i] = 0;
    if (i < 4) searchHeader[i] = 0;
    if (full && i == 0) {
        for (int k = 0; k < 7; k++) { blk->Tout[k] = Tpred[k]; blk->Tout[7 + k] = Tpred[k]; }
        for (int k = 0; k < 20; k++) blk->pose19[k] = 0.f;
        blk->nGood[0] = blk->nGood[1] = 0; blk->counters[0] = blk->counters[1] = 0; blk->start[0] = blk->start[1] = 0;
    }
}

// (gather_correspondences as a launch of its own: the paths that do not end a search with it)
__global__ __launch_bounds__(1024) void k_track_gather(int n, const RumiKeyPoint *__restrict__ keys, const int32_t *__restrict__ featMp,
                                                       const float *__restrict__ mpPos, const float *__restrict__ invSigma2, float *Xw, float *obs,
                                                       float *w, int32_t *idx, int32_t *start, int32_t *snapshot = nullptr) {
    __shared__ int sWave[16], sBase;
    gather_correspondences(n, keys, featMp, mpPos, invSigma2, Xw, obs, w, idx, start, snapshot, sWave, &sBase);
}

// "Discard outliers" of TrackWithMotionModel / TrackReferenceKeyFrame alone (Tracking.cc:2489-2508, 2349-2369): the outliers of the optimisation
// leave the frame, the others count towards nmatchesMap when their point has observations.  (The step-wise entries: SearchLocalPoints' own
// loops belong to rumi_track_local.)
__global__ void k_track_discard(const int32_t *idx, const uint8_t *outlierC, int32_t *featMp, const int32_t *mpObs, TrackBlock *blk,
                                const int32_t *searchHeader = nullptr) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c == 0 && searchHeader) { blk->spec[0] = searchHeader[0]; blk->spec[1] = searchHeader[1]; }
    if (c >= blk->start[1]) return;
    const int i = idx[c], mp = featMp[i];
    if (outlierC[c]) { featMp[i] = -1; return; }
    if (mpObs[mp] > 0) atomicAdd(&blk->counters[0], 1);
}

// rumi_track_local: the pose the stage starts from and its UpdatePoseMatrices, cleared outputs and counters (the frame's map-point vector and
// the seen flags arrive with the stage's upload)
__global__ void k_track_local_init(int n, const float *Tcw7, const float *K4, uint8_t *outF, int32_t *mpOut, int32_t *searchHeader, TrackBlock *blk) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) { outF[i] = 0; mpOut[i] = -1; }
    if (i < 4) searchHeader[i] = 0;
    if (i == 0) {
        for (int k = 0; k < 7; k++) { blk->Tout[k] = Tcw7[k]; blk->Tout[7 + k] = Tcw7[k]; }
        pose_matrices19(Tcw7, K4, blk->pose19);
        blk->nGood[0] = blk->nGood[1] = 0; blk->counters[0] = blk->counters[1] = 0; blk->start[0] = blk->start[1] = 0;
    }
}

// The frame's DBoW2::FeatureVector on the device (TemplatedVocabulary.h:1147-1190, FeatureVector.cpp:31-45): the features with a positive word
// weight grouped by their node id, nodes ascending, feature indices ascending inside a node, in the CSR form the BoW search reads.
// ONE workgroup: 64-bit keys node << 32 | feature in LDS, bitonic sort, then the group boundaries by an ordered compaction.
constexpr int kFvThreads = 1024;
__global__ __launch_bounds__(kFvThreads) void k_fv_build(int n, int npad, const uint32_t *__restrict__ node, const double *__restrict__ weight,
                                                         uint32_t *fvNodes, int32_t *fvOff, uint32_t *fvIdx, int32_t *nnOut) {
    extern __shared__ unsigned long long fvKey[];          // npad keys (a power of two >= n)
    __shared__ int sCnt[kFvThreads / 64], sBase, sValid;
    const int tid = threadIdx.x;
    for (int i = tid; i < npad; i += kFvThreads)
        fvKey[i] = (i < n && weight[i] > 0.0) ? (((unsigned long long)node[i] << 32) | (unsigned)i) : ~0ull;       // stopped words and padding sort last
    __syncthreads();
    for (int k = 2; k <= npad; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < npad; i += kFvThreads) {
                const int l = i ^ j;
                if (l > i) {
                    const unsigned long long a = fvKey[i], b = fvKey[l];
                    if ((a > b) == ((i & k) == 0)) { fvKey[i] = b; fvKey[l] = a; }
                }
            }
            __syncthreads();
        }
    if (tid == 0) { sBase = 0; sValid = 0; }
    __syncthreads();
    for (int c0 = 0; c0 < npad; c0 += kFvThreads) {
        const int i = c0 + tid;
        const unsigned long long key = i < npad ? fvKey[i] : ~0ull;
        const bool valid = key != ~0ull;
        const bool first = valid && (i == 0 || (uint32_t)(fvKey[i - 1] >> 32) != (uint32_t)(key >> 32));
        if (valid) fvIdx[i] = (uint32_t)key;
        if (valid) atomicMax(&sValid, i + 1);                // (ahead of the step's first barrier; read behind its last)
        block_ordered_slot(first, sCnt, &sBase, [&](int a) { fvNodes[a] = (uint32_t)(key >> 32); fvOff[a] = i; });
    }
    if (tid == 0) { fvOff[sBase] = sValid; *nnOut = sBase; }
}

// After the first PoseOptimization (Tracking.cc:2489-2508) and the first loop of SearchLocalPoints (:2998-3010): every point the motion search
// matched has been seen in this frame (inliers by SearchLocalPoints, outliers by the discard loop); outliers and bad points leave the frame.
// Thread 0 also derives Frame::UpdatePoseMatrices (Frame.cc:522-528) of the optimised pose in Sophus' / Eigen's float arithmetic: Rcw =
// q.toRotationMatrix(), tcw, Ow = conj(q) * (-tcw) (quaternion _transformVector), as [Rcw9 | tcw3 | Ow3 | K4] for k_is_in_frustum.
__global__ void k_track_after_motion(const int32_t *idx, const uint8_t *outlierC, int32_t *featMp, const int32_t *mpObs, const uint8_t *mpBad, uint8_t *seen,
                                     const float *K4, TrackBlock *blk, const int32_t *searchHeader) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c == 0) pose_matrices19(blk->Tout, K4, blk->pose19);
    if (c == 0 && searchHeader) { blk->spec[0] = searchHeader[0]; blk->spec[1] = searchHeader[1]; }   // (the next search clears the header)
    if (c >= blk->start[1]) return;
    const int i = idx[c], mp = featMp[i];
    seen[mp] = outlierC[c] ? 2 : 1;                        // 2: discarded as an outlier (k_track_frustum: its mbTrackInView may still be set from an earlier frame)
    if (outlierC[c]) { featMp[i] = -1; return; }
    if (mpObs[mp] > 0) atomicAdd(&blk->counters[0], 1);
    if (mpBad[mp]) featMp[i] = -1;
}

// Frame::isInFrustum of the local points SearchLocalPoints' second loop evaluates (not seen in this frame, not bad), writing the skip flag the query
// builder reads as isBad; also clears the search's result header and keeps a copy of the frame's map-point vector
struct FrustumArgs {
    int nmp, n;
    const int32_t *featMp;
    int32_t *mpMotion;
    const uint8_t *local, *seen, *bad;
    uint8_t *skip;
    int32_t *searchHeader;
    const float *pose;
    float minX, minY, maxX, maxY, logScaleFactor;
    int nLevels;
    float viewingCosLimit;
    const float *mpPos, *mpNormal, *mpMinDist, *mpMaxDist;
    uint8_t *inView;
    float *projX, *projY;
    int32_t *scaleLevel;
    float *viewCosOut, *trackDepth;
    const int32_t *mpObs;
    const float *scaleFactors;
    float th;
    int farPoints;
    float thFar;
    Query *q;
    const uint8_t *staleIn;      // RumiTrackPoints.stale_in_view / stale_proj (nullptr: none)
    const float *staleProj;
};
__device__ __forceinline__ void frustum_body(int i, const FrustumArgs &F) {
    if (i < 4) F.searchHeader[i] = 0;
    if (i < F.n) F.mpMotion[i] = F.featMp[i];              // mvpMapPoints as TrackWithMotionModel leaves them (the local search may replace unobserved points)
    if (i >= F.nmp) return;
    // A discarded outlier (seen == 2) is not re-projected (mnLastFrameSeen == mnId) -- but a monocular frame's discard loop left its mbTrackInView
    // as an earlier frame set it (Nleft = -1, Tracking.cc:2489-2508), and SearchByProjection searches it at that OLD projection (ORBmatcher.cc:46-60)
    if (F.local[i] && !F.bad[i] && F.seen[i] == 2 && F.staleIn && F.staleIn[i]) {
        const float *sp = F.staleProj + (size_t)i * 5;
        F.skip[i] = 0;
        F.inView[i] = 2; F.projX[i] = sp[0]; F.projY[i] = sp[1]; F.scaleLevel[i] = (int)sp[2]; F.viewCosOut[i] = sp[3]; F.trackDepth[i] = sp[4];
        F.q[i] = mappoint_query(i, true, sp[0], sp[1], (int)sp[2], sp[3], sp[4], false, F.mpObs[i], F.scaleFactors, F.th, F.farPoints, F.thFar);
        return;
    }
    const uint8_t sk = !F.local[i] || F.seen[i] || F.bad[i];
    F.skip[i] = sk;
    // (the search's query of this point is built here too: k_queries_mappoints' work on the values at hand, one launch less)
    if (sk) {
        F.inView[i] = 0; F.projX[i] = -1; F.projY[i] = -1; F.scaleLevel[i] = 0; F.viewCosOut[i] = 0; F.trackDepth[i] = 0;
        F.q[i] = mappoint_query(i, false, -1.f, -1.f, 0, 0.f, 0.f, true, F.mpObs[i], F.scaleFactors, F.th, F.farPoints, F.thFar);
        return;
    }
    const FrustumResult f = frustum_gate(F.mpPos + (size_t)i * 3, F.mpNormal + (size_t)i * 3, F.mpMinDist + i, F.mpMaxDist + i, F.pose, F.minX, F.minY, F.maxX,
                                         F.maxY, F.logScaleFactor, F.nLevels, F.viewingCosLimit);
    F.inView[i] = f.in; F.projX[i] = f.px; F.projY[i] = f.py; F.scaleLevel[i] = f.lvl; F.viewCosOut[i] = f.viewCos; F.trackDepth[i] = f.depth;
    F.q[i] = mappoint_query(i, f.in != 0, f.px, f.py, f.lvl, f.viewCos, f.depth, false, F.mpObs[i], F.scaleFactors, F.th, F.farPoints, F.thFar);
}

__global__ void k_track_frustum(FrustumArgs F) { frustum_body(blockIdx.x * blockDim.x + threadIdx.x, F); }

#include "track_local_map.inc"

// after the last PoseOptimization: mvpMapPoints and mvbOutlier per feature into the result block, mnMatchesInliers (Tracking.cc:2573-2586)
__global__ void k_track_finish(const int32_t *idx, const uint8_t *outlierC, const int32_t *featMp, const int32_t *mpObs, uint8_t *outlierF, int32_t *mpOut,
                               int countInliers, TrackBlock *blk, const int32_t *searchHeader) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c == 0 && searchHeader) { blk->spec[2] = searchHeader[0]; blk->spec[3] = searchHeader[1]; }
    if (c >= blk->start[1]) return;
    const int i = idx[c];
    mpOut[i] = featMp[i];
    if (countInliers) {
        outlierF[i] = outlierC[c];
        if (!outlierC[c] && mpObs[featMp[i]] > 0) atomicAdd(&blk->counters[1], 1);
    }
}

}  // namespace rumi

using namespace rumi;

// Frame::UndistortKeyPoints / ComputeImageBounds (R/lib_src/Frame.cc:770-826): cv::undistortPoints(mat, mat, K, mDistCoef, cv::Mat(), mK) per point,
// in double, operation by operation as OpenCV 3.4's cvUndistortPointsInternal does it (not in the tree: restated from the published algorithm,
// parity unpinned; oracle/frame_oracle.cc is the CPU statement the tests compare with): normalise, 5 fixed-point iterations of the inverse
// radial-tangential model, project with P = K.  Terms that are zero for (k1, k2, p1, p2, k3) keep their place: 0 * r2 is not dropped.
struct UndistortArgs { double fx, fy, cx, cy, ifx, ify, k1, k2, p1, p2, k3; };
__host__ __device__ inline void undistort_point(const UndistortArgs &A, float u, float v, float *uo, float *vo) {
    double x = u, y = v;
    x = (x - A.cx) * A.ifx; y = (y - A.cy) * A.ify;
    const double x0 = x, y0 = y;
    for (int j = 0; j < 5; j++) {
        const double r2 = x * x + y * y;
        const double icdist = (1 + ((0 * r2 + 0) * r2 + 0) * r2) / (1 + ((A.k3 * r2 + A.k2) * r2 + A.k1) * r2);
        const double deltaX = 2 * A.p1 * x * y + A.p2 * (r2 + 2 * x * x) + 0 * r2 + 0 * r2 * r2;
        const double deltaY = A.p1 * (r2 + 2 * y * y) + 2 * A.p2 * x * y + 0 * r2 + 0 * r2 * r2;
        x = (x0 - deltaX) * icdist;
        y = (y0 - deltaY) * icdist;
    }
    const double xx = A.fx * x + 0 * y + A.cx, yy = 0 * x + A.fy * y + A.cy, ww = 1. / (0 * x + 0 * y + 1);
    *uo = (float)(xx * ww); *vo = (float)(yy * ww);
}
// mvKeysUn: the extractor's key-points with pt replaced (Frame.cc:791-796); the count is read where the extractor left it (nDev) or given (n)
__global__ void k_undistort_keys(const int32_t *nDev, int n, const RumiKeyPoint *__restrict__ keys, RumiKeyPoint *__restrict__ keysUn, UndistortArgs A) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (nDev ? *nDev : n)) return;
    RumiKeyPoint k = keys[i];
    undistort_point(A, k.x, k.y, &k.x, &k.y);
    keysUn[i] = k;
}

struct TrackViews {                      // the arrays behind the TrackBlock header, in the device block and in its pinned mirror
    TrackBlock *blk;
    int32_t *mpOut, *mpMotion;           // mvpMapPoints at the end | after the motion model
    uint8_t *outF, *view, *record;       // mvbOutlier, mbTrackInView, the extractor's record [n, mono | keys cap | descriptors]
    int32_t *tableIds;                   // rumi_track_local_map: the point id of every table row, behind the record
};

namespace rumi { struct RelocState; void reloc_release(RelocState *s); }      // track_reloc.inc
namespace rumi { struct RelocResident; void reloc_resident_release(RelocResident *r); }      // track_reloc_resident.inc

struct RumiTracker {
    int device = 0, cap = 0, maxPts = 0, nlevels = 0;
    RumiOrbConfig cfg{};
    RumiOrb *ext = nullptr;
    RumiMatcher *m = nullptr;
    uint8_t *dImage = nullptr; size_t imageBytes = 0;
    hipStream_t upStream = nullptr;      // the step's uploads travel beside the extraction (rumi_track_frame)
    hipEvent_t evUp = nullptr;
    uint8_t *hImage = nullptr;           // pinned staging of the caller's (pageable) image: a plain memcpy + one asynchronous copy (the runtime's own
                                         // staging of a pageable source serialises the call for ~0.1 ms)
    // ONE device block [TrackBlock | mp cap*4 | mp after the motion model cap*4 | outlier cap | in_view maxPts | record 8 + 60 cap | table ids maxPts*4] and its pinned mirror: one copy brings a frame's results back
    uint8_t *dBlk = nullptr, *hBlk = nullptr; size_t oRec = 0, oDesc = 0, oIds = 0, blkBytes = 0, recordBytes = 0;     // oDesc: the descriptors inside the record
    TrackViews d{}, h{};
    float *dInvSigma2 = nullptr, *dXw = nullptr, *dObs = nullptr, *dW = nullptr;
    int32_t *dIdx = nullptr;
    uint8_t *dOutC = nullptr, *dActive = nullptr, *dSeen = nullptr, *dBad = nullptr, *dLocal = nullptr, *dStaleIn = nullptr;
    float *dStaleProj = nullptr;
    int projN = 0;                           // the projection arrays the last SearchLocalPoints left in the matcher's staging block (rumi_track_last_projections)
    double *dChi = nullptr;
    float scale[64] = {0};
    // the step-wise entries (rumi_track_extract / _motion / _reference_keyframe / _local): the frame that is resident, and its BoW transform
    int curN = -1, curW = 0, curH = 0, curMono = -1;
    // lens distortion (rumi_track_set_distortion): mvKeysUn of the resident frame and the undistorted image bounds (mnMinX .. mnMaxY)
    bool distort = false;
    UndistortArgs ua{};
    RumiKeyPoint *dKeysUn = nullptr;
    float bounds[4] = {0, 0, 0, 0};
    // the frame's BoW transform: one block [weight f64 x cap | word u32 x cap | node u32 x cap] and its pinned mirror (one copy back)
    uint8_t *dBow = nullptr, *hBow = nullptr;
    uint32_t *dWord = nullptr, *dNode = nullptr; double *dWeight = nullptr; int32_t *dNN = nullptr;
    // rumi_track_reloc_begin / _refine (track_reloc.inc): the session's blocks; frameSerial counts the frames that became resident
    uint32_t frameSerial = 0;
    rumi::RelocState *reloc = nullptr;
    // rumi_track_compute_bow / _reloc_bow / _reloc_begin_resident (track_reloc_resident.inc): the frame's FeatureVector, the BoW walk's matches
    rumi::RelocResident *rres = nullptr;
};

extern "C" void rumi_track_destroy(RumiTracker *t) {
    if (!t) return;
    (void)hipSetDevice(t->device);
    rumi::reloc_release(t->reloc);
    rumi::reloc_resident_release(t->rres);
    rumi_orb_destroy(t->ext);
    rumi_match_destroy(t->m);
    void *p[] = {t->dImage, t->dBlk, t->dInvSigma2, t->dXw, t->dObs, t->dW, t->dIdx, t->dOutC, t->dActive, t->dSeen, t->dBad, t->dLocal, t->dChi, t->dBow, t->dNN, t->dStaleIn, t->dStaleProj, t->dKeysUn};
    for (void *q : p) if (q) (void)hipFree(q);
    if (t->hBlk) (void)hipHostFree(t->hBlk);
    if (t->hBow) (void)hipHostFree(t->hBow);
    if (t->hImage) (void)hipHostFree(t->hImage);
    if (t->upStream) (void)hipStreamDestroy(t->upStream);
    if (t->evUp) (void)hipEventDestroy(t->evUp);
    delete t;
}

extern "C" int rumi_track_create(const RumiOrbConfig *cfg, int32_t max_points, int32_t device, RumiTracker **out) {
    if (!out) return RUMI_E_INVALID;
    *out = nullptr;
    if (!cfg || max_points < 1 || cfg->nlevels < 1 || cfg->nlevels > 16) return RUMI_E_INVALID;
    RumiTracker *t = new RumiTracker();
    t->cfg = *cfg; t->cfg.max_batch = 1; t->cfg.device = device;
    t->nlevels = cfg->nlevels;
    t->cap = cfg->nfeatures + 4 * cfg->nlevels + 64;                // what the facade's ORBextractor::operator() reserves
    t->maxPts = max_points;
    int rc = rumi_orb_create(&t->cfg, &t->ext);
    if (rc == RUMI_OK) rc = rumi_match_create(t->cap, std::max(max_points, t->cap), device, &t->m);
    if (rc != RUMI_OK) { rumi_track_destroy(t); return rc; }
    t->device = t->m->device;
    const size_t C = t->cap, P = max_points;
    auto al = [](size_t x) { return (x + 63) & ~(size_t)63; };
    t->imageBytes = (size_t)((cfg->max_width + 3) & ~3) * cfg->max_height;
    t->recordBytes = 8 + 60 * C;
    t->oDesc = 8 + C * sizeof(RumiKeyPoint);
    const size_t oMp = al(sizeof(TrackBlock)), oMpM = al(oMp + C * 4), oOut = al(oMpM + C * 4), oView = al(oOut + C);
    t->oRec = al(oView + P); t->oIds = al(t->oRec + t->recordBytes); t->blkBytes = al(t->oIds + P * 4);
#define TRYA(x) if ((rc = (x)) != RUMI_OK) { rumi_track_destroy(t); return rc; }
    TRYA(dev_alloc(&t->dImage, t->imageBytes + 64)); TRYA(dev_alloc(&t->dBlk, t->blkBytes)); TRYA(dev_alloc(&t->dInvSigma2, 64));
    TRYA(dev_alloc(&t->dXw, C * 3)); TRYA(dev_alloc(&t->dObs, C * 2)); TRYA(dev_alloc(&t->dW, C)); TRYA(dev_alloc(&t->dIdx, C));
    TRYA(dev_alloc(&t->dOutC, C)); TRYA(dev_alloc(&t->dActive, C)); TRYA(dev_alloc(&t->dSeen, P)); TRYA(dev_alloc(&t->dBad, P)); TRYA(dev_alloc(&t->dLocal, P)); TRYA(dev_alloc(&t->dStaleIn, P)); TRYA(dev_alloc(&t->dStaleProj, P * 5)); TRYA(dev_alloc(&t->dChi, C));
    TRYA(dev_alloc(&t->dBow, C * 16)); TRYA(dev_alloc(&t->dNN, 4));
    t->dWeight = reinterpret_cast<double *>(t->dBow); t->dWord = reinterpret_cast<uint32_t *>(t->dBow + C * 8); t->dNode = t->dWord + C;
#undef TRYA
    if (hipHostMalloc((void **)&t->hBlk, t->blkBytes, hipHostMallocDefault) != hipSuccess || hipHostMalloc((void **)&t->hBow, C * 16, hipHostMallocDefault) != hipSuccess ||
        hipHostMalloc((void **)&t->hImage, t->imageBytes + 64, hipHostMallocDefault) != hipSuccess ||
        hipStreamCreateWithFlags(&t->upStream, hipStreamNonBlocking) != hipSuccess || hipEventCreateWithFlags(&t->evUp, hipEventDisableTiming) != hipSuccess) {
        rumi_track_destroy(t); return RUMI_E_NO_DEVICE;
    }
    auto views = [&](uint8_t *b) {
        return TrackViews{reinterpret_cast<TrackBlock *>(b), reinterpret_cast<int32_t *>(b + oMp), reinterpret_cast<int32_t *>(b + oMpM), b + oOut, b + oView, b + t->oRec, reinterpret_cast<int32_t *>(b + t->oIds)};
    };
    t->d = views(t->dBlk); t->h = views(t->hBlk);
    float inv2[64] = {0};
    rumi_orb_tables(cfg, t->scale, nullptr, nullptr, inv2, nullptr, nullptr);
    if (hipMemcpy(t->dInvSigma2, inv2, sizeof(inv2), hipMemcpyHostToDevice) != hipSuccess) { rumi_track_destroy(t); return RUMI_E_NO_DEVICE; }
    *out = t;
    return RUMI_OK;
}

// ---- the stages the entries below are made of -------------------------------------------------------------------------------------------
namespace {
enum { SLOT_NONE = -1, SLOT_MOTION = 0, SLOT_LOCAL = 1 };              // which PoseOptimization of the step: Tin / Tout / nGood of the block
enum TrackTail { TAIL_AFTER_MOTION, TAIL_DISCARD, TAIL_FINISH };       // the kernel that follows it

int grid_of(int n) { return std::max(1, (n + 255) / 256); }
int grid_items(int n, int nmp) { return grid_of(std::max(std::max(n, nmp), 4)); }     // features, table points and the 4-word result header
bool has_stale(const RumiTrackPoints *pts) { return pts && pts->stale_in_view && pts->stale_proj; }
const RumiKeyPoint *resident_keys(const RumiTracker *t) {               // mvKeysUn: what every stage reads
    return t->distort ? t->dKeysUn : reinterpret_cast<const RumiKeyPoint *>(t->d.record + 8);
}

// Frame::ComputeImageBounds (Frame.cc:799-826): the image rectangle, or the undistorted corners' hull with lens distortion
void track_bounds(RumiTracker *t, int w, int h, RumiFrameFeatures *F) {
    if (!t->distort) { t->bounds[0] = 0; t->bounds[1] = 0; t->bounds[2] = (float)w; t->bounds[3] = (float)h; }
    else {
        const float c[8] = {0, 0, (float)w, 0, 0, (float)h, (float)w, (float)h};
        float u[8];
        for (int i = 0; i < 4; i++) undistort_point(t->ua, c[2 * i], c[2 * i + 1], &u[2 * i], &u[2 * i + 1]);
        t->bounds[0] = std::min(u[0], u[4]); t->bounds[2] = std::max(u[2], u[6]);
        t->bounds[1] = std::min(u[1], u[3]); t->bounds[3] = std::max(u[5], u[7]);
    }
    F->min_x = t->bounds[0]; F->min_y = t->bounds[1]; F->max_x = t->bounds[2]; F->max_y = t->bounds[3];
}
// mvKeysUn of the frame the extractor has just been asked for (same queue, behind the extraction)
void track_undistort(RumiTracker *t) {
    if (!t->distort) return;
    hipLaunchKernelGGL(k_undistort_keys, dim3((t->cap + 255) / 256), dim3(256), 0, nullptr, reinterpret_cast<const int32_t *>(t->d.record), t->cap,
                       reinterpret_cast<const RumiKeyPoint *>(t->d.record + 8), t->dKeysUn, t->ua);
}
// ORBextractor::operator() on the device: image -> pinned -> device (async), the extraction into the block's record, mvKeysUn
int track_upload_image(RumiTracker *t, const uint8_t *img, int w, int h, int stride) {
    const int wp = (w + 3) & ~3;
    if (!(img == t->hImage && stride == wp))                // (a caller that captured straight into rumi_track_image_buffer's memory has nothing to stage)
        for (int y = 0; y < h; y++) std::memcpy(t->hImage + (size_t)y * wp, img + (size_t)y * stride, (size_t)w);
    HIP_TRY(hipMemcpyAsync(t->dImage, t->hImage, (size_t)wp * h, hipMemcpyHostToDevice, nullptr));
    const int rc = rumi_orb_extract_batch_records_async(t->ext, t->dImage, 1, w, h, wp, (int64_t)wp * h, 0, 1000, t->d.record, (int64_t)t->recordBytes, t->cap, nullptr);
    if (rc != RUMI_OK) return rc;
    track_undistort(t);
    return RUMI_OK;
}
// a w x h frame whose features lie in the block's record (upload_frame of an empty frame queues the scale table and the cleared result header)
int track_stage_frame(RumiTracker *t, int w, int h, FrameDev *fd) {
    RumiFrameFeatures F{};
    F.n = 0; F.nlevels = t->nlevels; F.scale_factors = t->scale;
    track_bounds(t, w, h, &F);
    return upload_frame(t->m, &F, fd);
}
// the resident frame as the matcher's kernels address it
int track_frame_dev(RumiTracker *t, FrameDev *fd) {
    const int rc = track_stage_frame(t, t->curW, t->curH, fd);
    if (rc != RUMI_OK) return rc;
    fd->n = t->curN; fd->keys = resident_keys(t); fd->desc = t->d.record + t->oDesc;
    t->m->gridN = t->curN; t->m->gridKeys = fd->keys;
    return RUMI_OK;
}
// a step-wise entry starts from the resident frame and the pose it was given
void begin_entry(RumiTracker *t, RumiTrackResult *res, const float *Tcw7) {
    std::memset(res, 0, sizeof(*res));
    t->projN = 0;
    res->n = t->curN; res->mono_index = t->curMono;
    std::memcpy(res->Tcw_motion, Tcw7, 28); std::memcpy(res->Tcw, Tcw7, 28);
}
int track_check_points(const RumiTrackPoints *pts, bool needFrustum) {
    if (!pts || pts->n < 0) return RUMI_E_INVALID;
    if (pts->n > 0 && (!pts->pos || !pts->desc || !pts->obs || !pts->bad)) return RUMI_E_INVALID;
    if (pts->n > 0 && needFrustum && (!pts->normal || !pts->min_dist || !pts->max_dist || !pts->local)) return RUMI_E_INVALID;
    return RUMI_OK;
}

// The point table into the matcher's upload block (like match_host.h's stagers it only queues; the order of the segments fixes the offsets
// inside the staged block)
int stage_points(RumiTracker *t, const RumiTrackPoints *pts, bool withFrustumFields) {
    RumiMatcher *m = t->m;
    const int nmp = pts->n;
    if (nmp <= 0) return RUMI_OK;
    H2D(m->dF[0], pts->pos, (size_t)nmp * 3);
    if (withFrustumFields) { H2D(m->dF[1], pts->normal, (size_t)nmp * 3); H2D(m->dF[2], pts->min_dist, nmp); H2D(m->dF[3], pts->max_dist, nmp); }
    H2D(m->dI[1], pts->obs, nmp); H2D(m->dQDesc, pts->desc, (size_t)nmp * 32);
    if (withFrustumFields) {
        H2D(t->dBad, pts->bad, nmp); H2D(t->dLocal, pts->local, nmp);
        if (has_stale(pts)) { H2D(t->dStaleIn, pts->stale_in_view, nmp); H2D(t->dStaleProj, pts->stale_proj, (size_t)nmp * 5); }
    }
    return RUMI_OK;
}

// fill(mvpMapPoints, NULL); full: also cleared flags / counters, both poses = the prediction
void track_init(RumiTracker *t, int n, int nmp, int full, hipStream_t st) {
    hipLaunchKernelGGL(k_track_init, dim3(grid_items(n, nmp)), dim3(256), 0, st, n, nmp, full, t->m->dFeatMp, t->m->dOut, t->dSeen, t->d.outF, t->d.mpOut, t->m->dPose, t->d.blk);
}
void track_local_init(RumiTracker *t, int n, int nmp) {
    hipLaunchKernelGGL(k_track_local_init, dim3(grid_items(n, nmp)), dim3(256), 0, nullptr, n, t->m->dPose, t->m->dPose + 7, t->d.outF, t->d.mpOut, t->m->dOut, t->d.blk);
}

// A search in one queue, nothing read back: fused candidate lists and the resolve, whose result header stays on the device for the stage's
// trailing kernel.  withGather: the search ends with the gather of PoseOptimization's correspondences (k_resolve's tail) and, with snap, a
// copy of the map-point vector as the search left it.
int speculative_search(RumiTracker *t, int mode, int nq, const FrameDev &fd, float nnratio, int checkOri, bool withGather, int32_t *snap) {
    RumiMatcher *m = t->m;
    const int rc = build_lists(m, mode, nq, fd, m->dQDesc, false, true);
    if (rc != RUMI_OK) return rc;
    ResolveArgs A{mode, nq, fd.n, m->dQ, m->dCounts, m->dOffsets, m->lists.p, fd.keys, m->dI[1], m->dFeatMp, m->dAssign, m->dNmatches,
                  nnratio, checkOri, nullptr, 0.f, 0, m->dOverflow};
    if (withGather) { A.gMpPos = m->dF[0]; A.gInvSigma2 = t->dInvSigma2; A.gXw = t->dXw; A.gObs = t->dObs; A.gW = t->dW; A.gIdx = t->dIdx; A.gStart = t->d.blk->start; A.gSnapshot = snap; }
    launch_resolve(A, nullptr);
    return RUMI_OK;
}
// SearchByProjection(Cur, Last, th, mono) stage by stage, once more with 2 * th below 20 matches (Tracking.cc:2466-2474)
int motion_search(RumiTracker *t, const FrameDev &fd, int nlast, int nmp, float th_motion, int32_t *hostMp, RumiTrackResult *res) {
    RumiMatcher *m = t->m;
    int nm = 0;
    for (int attempt = 0; attempt < 2 && fd.n > 0 && nlast > 0 && nmp > 0; attempt++) {
        const float th = attempt == 0 ? th_motion : 2 * th_motion;
        if (attempt == 1) track_init(t, fd.n, nmp, 0, nullptr);
        launch_queries_frame(m, fd, nlast, th, nullptr);
        const int rc = run_search(m, MODE_FRAME, nlast, fd, m->dQDesc, m->dI[1], 0.f, 1, hostMp, &nm);
        if (rc != RUMI_OK) return rc;
        res->th_motion = (int32_t)th;
        if (nm >= 20) break;
    }
    res->nmatches_motion = nm;
    return RUMI_OK;
}
// SearchByProjection(F, local points) stage by stage, on the queries k_track_frustum built
int local_search(RumiTracker *t, const FrameDev &fd, int nmp, int32_t *hostMp, RumiTrackResult *res) {
    return run_search(t->m, MODE_MAPPOINTS, nmp, fd, t->m->dQDesc, t->m->dI[1], 0.8f, 0, hostMp, &res->nmatches_local);
}

// SearchLocalPoints' second loop with the pose in the block: isInFrustum of the table's points and their queries.  The six per-point fields go
// into the matcher's (by then scattered) staging block, where rumi_track_last_projections finds them.
int launch_frustum(RumiTracker *t, const FrameDev &fd, int nmp, bool stale, int n, float th_local, int far_points, float th_far_points, const char *entry) {
    RumiMatcher *m = t->m;
    if (!frustum_fits(m, nmp)) { g_lastError = std::string(entry) + ": point table exceeds the staging block"; return RUMI_E_CAPACITY; }
    const FrustumBlock fb(m->stage.d, nmp);                  // (its flag array stays unused: mbTrackInView goes into the tracker's block)
    const FrustumArgs FA{nmp, n, m->dFeatMp, t->d.mpMotion, t->dLocal, t->dSeen, t->dBad, /*skip*/ m->dU8b, m->dOut, t->d.blk->pose19, fd.minX,
                         fd.minY, fd.maxX, fd.maxY, std::log(t->cfg.scale_factor), t->nlevels, 0.5f, m->dF[0], m->dF[1], m->dF[2], m->dF[3], t->d.view, fb.x, fb.y, fb.level, fb.viewCos, fb.depth,
                         m->dI[1], m->dScale, th_local, far_points, th_far_points, m->dQ,
                         stale ? t->dStaleIn : nullptr, stale ? t->dStaleProj : nullptr};
    hipLaunchKernelGGL(k_track_frustum, dim3(grid_items(n, nmp)), dim3(256), 0, nullptr, FA);
    t->projN = nmp;
    return RUMI_OK;
}

// One PoseOptimization of the step and the kernel that follows it.  gatherFirst: the correspondences are gathered by a launch of their own (the
// paths whose search did not end with the gather).  slot: SLOT_MOTION optimises the staged pose into Tout[0..7), SLOT_LOCAL that into
// Tout[7..14); SLOT_NONE: no optimisation, the frame keeps its matches (TAIL_FINISH without the inlier count).  searchHeader: the result header of
// a speculative search, which the trailing kernel moves into the block (nullptr: none).
int pose_stage(RumiTracker *t, const FrameDev &fd, int slot, bool gatherFirst, TrackTail tail, const int32_t *searchHeader) {
    RumiMatcher *m = t->m;
    TrackBlock *dB = t->d.blk;
    if (gatherFirst)
        hipLaunchKernelGGL(k_track_gather, dim3(1), dim3(1024), 0, nullptr, fd.n, fd.keys, m->dFeatMp, m->dF[0], t->dInvSigma2, t->dXw, t->dObs, t->dW, t->dIdx, dB->start);
    if (slot != SLOT_NONE) {
        const bool fitsLds = fd.n <= kPoseLdsEdges;        // the frame's correspondences fit the LDS instantiation of k_pose_opt for sure
        const int rc = rumi::pose_opt_device(dB->start, t->dXw, t->dObs, t->dW, m->dPose + 7, slot == SLOT_MOTION ? m->dPose : dB->Tout, dB->Tout + 7 * slot, t->dOutC,
                                             dB->nGood + slot, t->dActive, t->dChi, fitsLds, nullptr);
        if (rc != RUMI_OK) return rc;
    }
    const dim3 gC(grid_of(t->cap)), b(256);
    if (tail == TAIL_AFTER_MOTION)
        hipLaunchKernelGGL(k_track_after_motion, gC, b, 0, nullptr, t->dIdx, t->dOutC, m->dFeatMp, m->dI[1], t->dBad, t->dSeen, m->dPose + 7, dB, searchHeader);
    else if (tail == TAIL_DISCARD)
        hipLaunchKernelGGL(k_track_discard, gC, b, 0, nullptr, t->dIdx, t->dOutC, m->dFeatMp, m->dI[1], dB, searchHeader);
    else
        hipLaunchKernelGGL(k_track_finish, gC, b, 0, nullptr, t->dIdx, t->dOutC, m->dFeatMp, m->dI[1], t->d.outF, t->d.mpOut, slot != SLOT_NONE ? 1 : 0, dB, searchHeader);
    return RUMI_OK;
}

// rumi_track_frame's one copy back: header, mvpMapPoints, mvbOutlier, mbTrackInView and the extractor's record
int fetch_frame_block(RumiTracker *t, int n) {
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(t->hBlk, t->dBlk, t->oRec + t->oDesc + (size_t)n * 32, hipMemcpyDeviceToHost));
    return RUMI_OK;
}
// the motion / reference entries' copies back: the frame's vector after the discard, its snapshot before it (when the search took one), the header
int fetch_discard_block(RumiTracker *t, int n, bool withSnapshot) {
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(t->h.mpOut, t->m->dFeatMp, (size_t)n * 4, hipMemcpyDeviceToHost, nullptr));
    if (withSnapshot) HIP_TRY(hipMemcpyAsync(t->h.mpMotion, t->d.mpMotion, (size_t)n * 4, hipMemcpyDeviceToHost, nullptr));
    HIP_TRY(hipMemcpy(t->hBlk, t->dBlk, sizeof(TrackBlock), hipMemcpyDeviceToHost));
    return RUMI_OK;
}

void unpack_motion_pose(RumiTrackResult *res, const TrackBlock *hB) {
    std::memcpy(res->Tcw_motion, hB->Tout, 28); std::memcpy(res->Tcw, hB->Tout, 28);
    res->ngood_motion = hB->nGood[0]; res->nmatches_map = hB->counters[0];
}
void unpack_local_pose(RumiTrackResult *res, const TrackBlock *hB) {
    std::memcpy(res->Tcw, hB->Tout + 7, 28);
    std::memcpy(res->Rcw, hB->pose19, 36); std::memcpy(res->tcw, hB->pose19 + 9, 12); std::memcpy(res->Ow, hB->pose19 + 12, 12);
    res->ngood_local = hB->nGood[1]; res->matches_inliers = hB->counters[1];
}
// a feature that held a point before the optimisation and none after it was discarded as an outlier
void unpack_discarded(const int32_t *before, const int32_t *after, int n, int32_t *frame_mp, int32_t *discarded) {
    for (int i = 0; i < n; i++) { if (before[i] >= 0 && after[i] < 0) discarded[i] = before[i]; frame_mp[i] = after[i]; }
}
void unpack_in_view(const RumiTracker *t, int nmp, bool localRan, uint8_t *in_view, RumiTrackResult *res) {
    int nTo = 0;
    if (nmp > 0) {
        if (localRan) std::memcpy(in_view, t->h.view, (size_t)nmp); else std::memset(in_view, 0, (size_t)nmp);
        for (int j = 0; j < nmp; j++) nTo += in_view[j] == 1;         // (2: a stale flag of an earlier frame, not an isInFrustum of this one)
    }
    res->n_to_match = nTo;
}

// TrackLocalMap from the point where the table, the frame's vector and the seen flags lie on the device: SearchLocalPoints' second loop, the
// search (speculative, or sized after a list overflow), PoseOptimization and the statistics loop.  Ends with the block in the pinned mirror.
int track_local_body(RumiTracker *t, const FrameDev &fd, int n, int nmp, bool stale, float th_local, int far_points, float th_far_points, const char *entry,
                     RumiTrackResult *res) {
    RumiMatcher *m = t->m;
    int rc;
    track_local_init(t, n, nmp);
    bool speculate = false;
    std::vector<int32_t> tmpMp((size_t)std::max(n, 1));
    if (nmp > 0 && n > 0) {
        if ((rc = launch_frustum(t, fd, nmp, stale, n, th_local, far_points, th_far_points, entry)) != RUMI_OK) return rc;
        // the search's counts are not needed before the end: one queue, the result header travels in the block (a list overflow -- the resolve
        // did not run then, the frame's vector is untouched -- sends the stage through the sizing path)
        speculate = track_speculation().speculate && m->lists.cap / (size_t)nmp >= 64;
        if ((rc = speculate ? speculative_search(t, MODE_MAPPOINTS, nmp, fd, 0.8f, 0, false, nullptr) : local_search(t, fd, nmp, tmpMp.data(), res)) != RUMI_OK) return rc;
    }
    const TrackBlock *hB = t->h.blk;
    for (int pass = 0; pass < 2; pass++) {
        if ((rc = pose_stage(t, fd, SLOT_LOCAL, true, TAIL_FINISH, speculate ? m->dOut : nullptr)) != RUMI_OK) return rc;
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpy(t->hBlk, t->dBlk, t->oRec, hipMemcpyDeviceToHost));       // header, mvpMapPoints, mvbOutlier, mbTrackInView
        if (!speculate) break;
        if (hB->spec[3] == 0) { res->nmatches_local = hB->spec[2]; break; }
        // a candidate list overflowed: the search again with exact list sizes, then the optimisation on its result
        speculate = false;
        track_local_init(t, n, nmp);
        if ((rc = local_search(t, fd, nmp, tmpMp.data(), res)) != RUMI_OK) return rc;
    }
    unpack_local_pose(res, hB);
    return RUMI_OK;
}
}  // namespace

extern "C" int rumi_track_frame(RumiTracker *t, const uint8_t *img, int32_t w, int32_t h, int32_t stride, const float *K4, const float *Tcw_pred7,
                                const RumiKeyPoint *last_keys_un, int32_t nlast, const int32_t *last_mp, const uint8_t *last_outlier,
                                const RumiTrackPoints *pts, float th_motion, float th_local, int32_t far_points, float th_far_points,
                                RumiKeyPoint *keys_out, uint8_t *desc_out, int32_t cap, int32_t *frame_mp_motion, int32_t *frame_mp, uint8_t *outlier,
                                uint8_t *in_view, RumiTrackResult *res) {
    if (!t || !img || !K4 || !Tcw_pred7 || !pts || !res || !keys_out || !desc_out || !frame_mp_motion || !frame_mp || !outlier || nlast < 0 || pts->n < 0 ||
        stride < w || (nlast > 0 && (!last_keys_un || !last_mp || !last_outlier)) ||
        (pts->n > 0 && (!pts->pos || !pts->normal || !pts->min_dist || !pts->max_dist || !pts->desc || !pts->obs || !pts->bad || !pts->local || !in_view)))
        return RUMI_E_INVALID;
    if (w <= 0 || h <= 0) return RUMI_E_EMPTY;
    if (w > t->cfg.max_width || h > t->cfg.max_height) { g_lastError = "rumi_track_frame: image larger than the tracker was created for"; return RUMI_E_CAPACITY; }
    t->curN = -1;
    RumiMatcher *m = t->m;
    const int nmp = pts->n;
    if (nlast > m->maxQ || nmp > t->maxPts || cap < t->cap) { g_lastError = "rumi_track_frame: more points / features than the tracker was created for, or cap too small"; return RUMI_E_CAPACITY; }
    for (int i = 0; i < nlast; i++) if (last_mp[i] >= nmp) { g_lastError = "rumi_track_frame: last_mp index outside the point table"; return RUMI_E_INVALID; }
    HIP_TRY(hipSetDevice(t->device));
    std::memset(res, 0, sizeof(*res));
    t->projN = 0;
    res->mono_index = -1; res->th_motion = (int32_t)th_motion;

    // ---- stage 1: ORBextractor::operator() on the device; only the two counts come back (launch sizes need n)
    int rc = track_upload_image(t, img, w, h, stride);
    if (rc != RUMI_OK) return rc;
    // ---- uploads of the whole step: one pinned block, one copy, scattered on the device; the frame itself is read where the extractor left it.
    // None of it depends on the extraction: the host fills the block while the extraction runs, and only then waits for the two counts.
    FrameDev fd;
    if ((rc = track_stage_frame(t, w, h, &fd)) != RUMI_OK || (rc = stage_pose(m, Tcw_pred7, K4)) != RUMI_OK || (rc = stage_points(t, pts, true)) != RUMI_OK ||
        (rc = stage_last_frame(m, last_keys_un, nlast, last_mp, last_outlier)) != RUMI_OK)
        return rc;
    const bool gridWanted = m->gridPending;                 // (the grid needs the feature count: it is built below)
    m->gridPending = false;
    const bool canSpec = track_speculation().speculate && nlast > 0 && nmp > 0 && m->lists.cap / (size_t)std::max(nlast, nmp) >= 64 && frustum_fits(m, nmp);
    m->upStream = t->upStream;                              // the copy and the scatter, on a stream of their own beside the extraction
    const int rcUp = flush_uploads(m);
    m->upStream = nullptr;
    if (rcUp != RUMI_OK) return rcUp;
    if (canSpec) {
        // what the usual case (below) needs and the extraction does not feed: the cleared frame (sized by the capacity) and the motion-model queries
        track_init(t, t->cap, nmp, 1, t->upStream);
        launch_queries_frame(m, fd, nlast, th_motion, t->upStream);
    }
    HIP_TRY(hipEventRecord(t->evUp, t->upStream));
    HIP_TRY(hipStreamWaitEvent(nullptr, t->evUp, 0));      // (behind the extraction in the main queue: by then the event has long fired)
    // ---- the usual case in ONE queue, no host round trip: the first search finds >= 20 matches and no candidate list overflows.  Every launch
    // of stages 2-5 goes out back to back behind the extraction -- the feature count and the searches' counts stay on the device (launches are
    // sized by their upper bounds), the searches' result headers are kept in the block -- the block comes back once, and only if a header says
    // otherwise (fewer than 20 matches: the 2 th retry; a list overflow; no key-point at all) the step is redone stage by stage.
    int n = t->cap;                                          // an upper bound until the two counts have been read
    auto take_counts = [&](const int32_t *counts) {
        n = counts[0];
        res->n = n; res->mono_index = counts[1];
        t->curN = n; t->curW = w; t->curH = h; t->curMono = counts[1];      // the frame is resident for the step-wise entries too
        t->frameSerial++;
        fd.n = n; m->gridN = n;
    };
    if (!canSpec) {
        int32_t counts[2] = {0, -1};
        HIP_TRY(hipMemcpy(counts, t->d.record, 8, hipMemcpyDeviceToHost));
        if ((rc = rumi_orb_sync(t->ext)) != RUMI_OK) return rc;
        take_counts(counts);
    }
    fd.n = n; fd.keys = resident_keys(t); fd.desc = t->d.record + t->oDesc;
    m->gridN = n; m->gridKeys = fd.keys; m->gridNDev = canSpec ? reinterpret_cast<const int32_t *>(t->d.record) : nullptr;
    m->gridPending = gridWanted;
    FLUSH(m);                                               // the grid of the resident frame
    if (!canSpec) track_init(t, n, nmp, 1, nullptr);
    bool done = false;
    if (canSpec) {
        const int32_t *header = m->dOut;                     // each search's result header, moved into the block by the kernel behind its optimisation
        if ((rc = speculative_search(t, MODE_FRAME, nlast, fd, 0.f, 1, true, nullptr)) != RUMI_OK) return rc;      // (its queries were built beside the extraction, above)
        if ((rc = pose_stage(t, fd, SLOT_MOTION, false, TAIL_AFTER_MOTION, header)) != RUMI_OK) return rc;
        // (k_track_after_motion and k_track_frustum as ONE 1024-thread workgroup -- the frustum test reads the seen flags and the pose matrices the
        // first half writes -- measured: 0.427-0.436 ms against 0.430-0.431 for the frame, no gain; not kept)
        if ((rc = launch_frustum(t, fd, nmp, has_stale(pts), n, th_local, far_points, th_far_points, "rumi_track_frame")) != RUMI_OK) return rc;
        if ((rc = speculative_search(t, MODE_MAPPOINTS, nmp, fd, 0.8f, 0, true, nullptr)) != RUMI_OK) return rc;
        if ((rc = pose_stage(t, fd, SLOT_LOCAL, false, TAIL_FINISH, header)) != RUMI_OK) return rc;
        if ((rc = fetch_frame_block(t, n)) != RUMI_OK || (rc = rumi_orb_sync(t->ext)) != RUMI_OK) return rc;
        take_counts(reinterpret_cast<const int32_t *>(t->h.record));
        const TrackBlock *hS = t->h.blk;
        if (n > 0 && hS->spec[0] >= 20 && hS->spec[1] == 0 && hS->spec[3] == 0) {
            res->nmatches_motion = hS->spec[0];
            res->nmatches_local = hS->spec[2];
            done = true;
        } else {
            // not the usual case: start over from the cleared frame (the staged inputs and the frame's grid are still on the device)
            track_init(t, n, nmp, 1, nullptr);
        }
    }
    bool localRan = done;
    if (!done) {
        // ---- stage 2: SearchByProjection(Cur, Last, th, mono)
        std::vector<int32_t> tmpMp((size_t)std::max(n, 1));
        if ((rc = motion_search(t, fd, nlast, nmp, th_motion, tmpMp.data(), res)) != RUMI_OK) return rc;
        if (res->nmatches_motion >= 20) {
            // ---- stage 3: PoseOptimization on the matches, outliers leave the frame
            if ((rc = pose_stage(t, fd, SLOT_MOTION, true, TAIL_AFTER_MOTION, nullptr)) != RUMI_OK) return rc;
            // ---- stage 4: SearchLocalPoints with the optimised pose
            if ((rc = launch_frustum(t, fd, nmp, has_stale(pts), n, th_local, far_points, th_far_points, "rumi_track_frame")) != RUMI_OK) return rc;
            if ((rc = local_search(t, fd, nmp, tmpMp.data(), res)) != RUMI_OK) return rc;
            localRan = true;
            // ---- stage 5: PoseOptimization on everything the frame now holds
            if ((rc = pose_stage(t, fd, SLOT_LOCAL, true, TAIL_FINISH, nullptr)) != RUMI_OK) return rc;
        } else if (res->nmatches_motion > 0) {                 // fewer than 20 matches: the frame keeps them (the caller falls back to TrackReferenceKeyFrame)
            if ((rc = pose_stage(t, fd, SLOT_NONE, true, TAIL_FINISH, nullptr)) != RUMI_OK) return rc;
        }
        if ((rc = fetch_frame_block(t, n)) != RUMI_OK) return rc;
    }
    unpack_motion_pose(res, t->h.blk);
    unpack_local_pose(res, t->h.blk);
    if (n > 0) {
        std::memcpy(frame_mp, t->h.mpOut, (size_t)n * 4); std::memcpy(outlier, t->h.outF, (size_t)n);
        std::memcpy(keys_out, t->h.record + 8, (size_t)n * sizeof(RumiKeyPoint));
        std::memcpy(desc_out, t->h.record + t->oDesc, (size_t)n * 32);
    }
    unpack_in_view(t, nmp, localRan, in_view, res);
    if (n > 0) std::memcpy(frame_mp_motion, localRan ? t->h.mpMotion : t->h.mpOut, (size_t)n * 4);
    return RUMI_OK;
}

// ==================================================================================================================
// The same stages one member function of Tracking at a time (include/rumi_track.h, "step-wise entries"): the frame extracted by
// rumi_track_extract stays on the device -- key-points, descriptors, grid, FeatureVector -- while the host runs the reference's own control
// flow between the calls (the decisions of TrackWithMotionModel / TrackReferenceKeyFrame, UpdateLocalMap).
// ==================================================================================================================

// The tracker's pinned staging buffer for a w x h frame, for a caller that lets its camera driver / decoder write the frame there (e.g. a
// cv::Mat constructed on this memory): rumi_track_frame / rumi_track_extract called with this pointer and stride skip their staging copy.
extern "C" int rumi_track_image_buffer(RumiTracker *t, int32_t w, int32_t h, uint8_t **buf, int32_t *stride) {
    if (!t || !buf || !stride) return RUMI_E_INVALID;
    if (w <= 0 || h <= 0 || w > t->cfg.max_width || h > t->cfg.max_height) { g_lastError = "rumi_track_image_buffer: frame larger than the tracker was created for"; return RUMI_E_CAPACITY; }
    *buf = t->hImage; *stride = (w + 3) & ~3;
    return RUMI_OK;
}

extern "C" int rumi_track_extract(RumiTracker *t, const uint8_t *img, int32_t w, int32_t h, int32_t stride, RumiKeyPoint *keys_out, uint8_t *desc_out,
                                  int32_t cap, int32_t *n_out, int32_t *mono_out) {
    if (!t || !img || !keys_out || !desc_out || !n_out || !mono_out || stride < w) return RUMI_E_INVALID;
    *n_out = 0; *mono_out = -1;
    if (w <= 0 || h <= 0) return RUMI_E_EMPTY;
    if (w > t->cfg.max_width || h > t->cfg.max_height || cap < t->cap) { g_lastError = "rumi_track_extract: image larger than the tracker was created for, or cap too small"; return RUMI_E_CAPACITY; }
    HIP_TRY(hipSetDevice(t->device));
    t->curN = -1;
    int rc = track_upload_image(t, img, w, h, stride);
    if (rc != RUMI_OK) return rc;
    int32_t counts[2] = {0, -1};
    HIP_TRY(hipMemcpy(counts, t->d.record, 8, hipMemcpyDeviceToHost));
    if ((rc = rumi_orb_sync(t->ext)) != RUMI_OK) return rc;
    const int n = counts[0];
    if (n > 0) {
        HIP_TRY(hipMemcpyAsync(t->h.record + 8, t->d.record + 8, (size_t)n * sizeof(RumiKeyPoint), hipMemcpyDeviceToHost, nullptr));
        HIP_TRY(hipMemcpy(t->h.record + t->oDesc, t->d.record + t->oDesc, (size_t)n * 32, hipMemcpyDeviceToHost));
        std::memcpy(keys_out, t->h.record + 8, (size_t)n * sizeof(RumiKeyPoint));
        std::memcpy(desc_out, t->h.record + t->oDesc, (size_t)n * 32);
    }
    t->curN = n; t->curW = w; t->curH = h; t->curMono = counts[1];
    t->frameSerial++;
    { RumiFrameFeatures Fb{}; track_bounds(t, w, h, &Fb); }    // mnMinX .. mnMaxY of this frame (rumi_track_undistorted)
    *n_out = n; *mono_out = counts[1];
    return RUMI_OK;
}

extern "C" int rumi_track_motion(RumiTracker *t, const float *K4, const float *Tcw_pred7, const RumiKeyPoint *last_keys_un, int32_t nlast,
                                 const int32_t *last_mp, const uint8_t *last_outlier, const RumiTrackPoints *pts, float th_motion, int32_t *frame_mp,
                                 int32_t *discarded, RumiTrackResult *res) {
    if (!t || !K4 || !Tcw_pred7 || !res || !frame_mp || !discarded || nlast < 0 || (nlast > 0 && (!last_keys_un || !last_mp || !last_outlier)) ||
        track_check_points(pts, false) != RUMI_OK)
        return RUMI_E_INVALID;
    if (t->curN < 0) { g_lastError = "rumi_track_motion: no frame is resident (rumi_track_extract first)"; return RUMI_E_INVALID; }
    RumiMatcher *m = t->m;
    const int n = t->curN, nmp = pts->n;
    if (nlast > m->maxQ || nmp > t->maxPts) { g_lastError = "rumi_track_motion: more points / features than the tracker was created for"; return RUMI_E_CAPACITY; }
    for (int i = 0; i < nlast; i++) if (last_mp[i] >= nmp) { g_lastError = "rumi_track_motion: last_mp index outside the point table"; return RUMI_E_INVALID; }
    HIP_TRY(hipSetDevice(t->device));
    begin_entry(t, res, Tcw_pred7);
    res->th_motion = (int32_t)th_motion;
    for (int i = 0; i < n; i++) { frame_mp[i] = -1; discarded[i] = -1; }
    FrameDev fd;
    int rc;
    if ((rc = track_frame_dev(t, &fd)) != RUMI_OK || (rc = stage_pose(m, Tcw_pred7, K4)) != RUMI_OK || (rc = stage_points(t, pts, false)) != RUMI_OK ||
        (rc = stage_last_frame(m, last_keys_un, nlast, last_mp, last_outlier)) != RUMI_OK)
        return rc;
    FLUSH(m);
    track_init(t, n, nmp, 1, nullptr);
    // the usual case (>= 20 matches at th, no list overflow) in one queue, as in rumi_track_frame: the search's result header and the map-point
    // vector it leaves travel back with the results; anything else is redone stage by stage below
    if (track_speculation().speculate && n > 0 && nlast > 0 && nmp > 0 && m->lists.cap / (size_t)nlast >= 64) {
        launch_queries_frame(m, fd, nlast, th_motion, nullptr);
        if ((rc = speculative_search(t, MODE_FRAME, nlast, fd, 0.f, 1, true, t->d.mpMotion)) != RUMI_OK) return rc;
        if ((rc = pose_stage(t, fd, SLOT_MOTION, false, TAIL_DISCARD, m->dOut)) != RUMI_OK) return rc;
        if ((rc = fetch_discard_block(t, n, true)) != RUMI_OK) return rc;
        if (t->h.blk->spec[0] >= 20 && t->h.blk->spec[1] == 0) {
            res->nmatches_motion = t->h.blk->spec[0];
            unpack_motion_pose(res, t->h.blk);
            unpack_discarded(t->h.mpMotion, t->h.mpOut, n, frame_mp, discarded);
            return RUMI_OK;
        }
        track_init(t, n, nmp, 1, nullptr);
    }
    std::vector<int32_t> searched((size_t)std::max(n, 1), -1);
    if ((rc = motion_search(t, fd, nlast, nmp, th_motion, searched.data(), res)) != RUMI_OK) return rc;
    if (n > 0) std::memcpy(frame_mp, searched.data(), (size_t)n * 4);
    if (res->nmatches_motion < 20) return RUMI_OK;                // TrackWithMotionModel returns false here (:2476-2483): nothing else has happened to the frame
    if ((rc = pose_stage(t, fd, SLOT_MOTION, true, TAIL_DISCARD, nullptr)) != RUMI_OK) return rc;
    if ((rc = fetch_discard_block(t, n, false)) != RUMI_OK) return rc;
    unpack_motion_pose(res, t->h.blk);
    unpack_discarded(searched.data(), t->h.mpOut, n, frame_mp, discarded);
    return RUMI_OK;
}

extern "C" int rumi_track_reference_keyframe(RumiTracker *t, RumiVocabulary *voc, int32_t levelsup, const float *K4, const float *Tcw_init7,
                                             const RumiFrameFeatures *KF, const RumiFeatureVector *kf_fv, const int32_t *kf_mp,
                                             const RumiTrackPoints *pts, float nnratio, int32_t check_orientation, uint32_t *word_id, double *word_weight,
                                             uint32_t *node_id, int32_t *frame_mp, int32_t *discarded, RumiTrackResult *res) {
    if (!t || !voc || !K4 || !Tcw_init7 || !KF || !kf_fv || !res || !frame_mp || !discarded || !word_id || !word_weight || !node_id || KF->n < 0 ||
        kf_fv->n_nodes < 0 || (KF->n > 0 && (!kf_mp || !KF->keys_un || !KF->desc)) || track_check_points(pts, false) != RUMI_OK)
        return RUMI_E_INVALID;
    if (t->curN < 0) { g_lastError = "rumi_track_reference_keyframe: no frame is resident (rumi_track_extract first)"; return RUMI_E_INVALID; }
    RumiMatcher *m = t->m;
    const int n = t->curN, nmp = pts->n;
    const int nqe = kf_fv->n_nodes > 0 ? kf_fv->offsets[kf_fv->n_nodes] : 0;
    if (KF->n > m->maxQ || nqe > m->maxQ || nmp > t->maxPts || nmp > m->maxQ || kf_fv->n_nodes > m->maxQ) {
        g_lastError = "rumi_track_reference_keyframe: sizes exceed the tracker's capacities"; return RUMI_E_CAPACITY;
    }
    for (int i = 0; i < KF->n; i++) if (kf_mp[i] >= nmp) { g_lastError = "rumi_track_reference_keyframe: kf_mp index outside the point table"; return RUMI_E_INVALID; }
    HIP_TRY(hipSetDevice(t->device));
    begin_entry(t, res, Tcw_init7);
    for (int i = 0; i < n; i++) { frame_mp[i] = -1; discarded[i] = -1; }
    if (n == 0) return RUMI_OK;
    // ---- Frame::ComputeBoW (Frame.cc:763-768): the tree descent of every descriptor, then the FeatureVector, both on the device
    int rc = rumi_voc_transform_batch_device(voc, t->d.record + t->oDesc, t->d.record, 1, t->cap, levelsup, t->dWord, t->dWeight, t->dNode, nullptr);
    if (rc != RUMI_OK) return rc;
    int npad = 1;
    while (npad < n) npad <<= 1;
    const size_t fvLds = (size_t)npad * sizeof(unsigned long long);
    if (fvLds > 64 * 1024) HIP_TRY(raise_lds_limit(reinterpret_cast<const void *>(k_fv_build), fvLds));
    hipLaunchKernelGGL(k_fv_build, dim3(1), dim3(kFvThreads), fvLds, nullptr, n, npad, t->dNode, t->dWeight, m->dNodesB, m->dOffB, m->dFvIdx, t->dNN);
    // ---- SearchByBoW(pKF, F, vpMapPointMatches) (ORBmatcher.cc:198-370): the key-frame side comes from the host, the frame side is resident
    FrameDev fd;
    if ((rc = track_frame_dev(t, &fd)) != RUMI_OK || (rc = stage_pose(m, Tcw_init7, K4)) != RUMI_OK) return rc;
    if ((rc = stage_query_keyframe(m, KF, kf_mp)) != RUMI_OK) return rc;
    if (nmp > 0) { H2D(m->dU8a, pts->bad, nmp); H2D(m->dF[0], pts->pos, (size_t)nmp * 3); H2D(m->dI[1], pts->obs, nmp); }
    if ((rc = stage_fv_query(m, kf_fv, nqe)) != RUMI_OK) return rc;
    m->gridPending = false;                                 // candidates come from the FeatureVectors: the spatial grid is not read
    FLUSH(m);
    track_init(t, n, nmp, 1, nullptr);
    if (kf_fv->n_nodes > 0) launch_queries_bow(m, nqe, kf_fv->n_nodes, 0, t->dNN, nullptr);
    int nm = 0;
    std::vector<int32_t> searched((size_t)n, -1);
    if ((rc = run_search(m, MODE_BOW, nqe, fd, m->dQDesc, nullptr, nnratio, check_orientation, searched.data(), &nm)) != RUMI_OK) return rc;
    res->nmatches_motion = nm;
    std::memcpy(frame_mp, searched.data(), (size_t)n * 4);
    // the per-feature transform for the host's mBowVec / mFeatVec (assembled there in feature order: rumi_voc_assemble): ONE copy of the block into
    // pinned memory, queued BEHIND the pose chain (three copies into the caller's pageable arrays sat between the search and PoseOptimization)
    const size_t C = (size_t)t->cap;
    auto bow_out = [&]() {
        std::memcpy(word_weight, t->hBow, (size_t)n * 8); std::memcpy(word_id, t->hBow + C * 8, (size_t)n * 4); std::memcpy(node_id, t->hBow + C * 12, (size_t)n * 4);
    };
    if (nm < 15) {                                          // TrackReferenceKeyFrame returns false here (:2335-2338)
        HIP_TRY(hipMemcpy(t->hBow, t->dBow, C * 16, hipMemcpyDeviceToHost));
        bow_out();
        return RUMI_OK;
    }
    if ((rc = pose_stage(t, fd, SLOT_MOTION, true, TAIL_DISCARD, nullptr)) != RUMI_OK) return rc;
    HIP_TRY(hipMemcpyAsync(t->hBow, t->dBow, C * 16, hipMemcpyDeviceToHost, nullptr));
    if ((rc = fetch_discard_block(t, n, false)) != RUMI_OK) return rc;
    bow_out();
    unpack_motion_pose(res, t->h.blk);
    unpack_discarded(searched.data(), t->h.mpOut, n, frame_mp, discarded);
    return RUMI_OK;
}

extern "C" int rumi_track_local(RumiTracker *t, const float *K4, const float *Tcw7, const int32_t *frame_mp_in, const RumiTrackPoints *pts,
                                const uint8_t *seen_in, float th_local, int32_t far_points, float th_far_points, int32_t *frame_mp, uint8_t *outlier,
                                uint8_t *in_view, RumiTrackResult *res) {
    if (!t || !K4 || !Tcw7 || !res || !frame_mp || !outlier || !frame_mp_in || track_check_points(pts, true) != RUMI_OK || (pts->n > 0 && !in_view))
        return RUMI_E_INVALID;
    if (t->curN < 0) { g_lastError = "rumi_track_local: no frame is resident (rumi_track_extract first)"; return RUMI_E_INVALID; }
    RumiMatcher *m = t->m;
    const int n = t->curN, nmp = pts->n;
    if (nmp > t->maxPts) { g_lastError = "rumi_track_local: more points than the tracker was created for"; return RUMI_E_CAPACITY; }
    for (int i = 0; i < n; i++) if (frame_mp_in[i] >= nmp) { g_lastError = "rumi_track_local: frame_mp_in index outside the point table"; return RUMI_E_INVALID; }
    HIP_TRY(hipSetDevice(t->device));
    begin_entry(t, res, Tcw7);
    // SearchLocalPoints, first loop (Tracking.cc:2998-3010), on the host while the arrays are being staged: a bad point leaves the frame, the
    // others are "seen in this frame"; seen_in carries the points the caller's discard loop has marked (mnLastFrameSeen == mCurrentFrame.mnId)
    std::vector<int32_t> mpIn((size_t)std::max(n, 1), -1);
    std::vector<uint8_t> seen((size_t)std::max(nmp, 1), 0);
    if (seen_in) for (int j = 0; j < nmp; j++) seen[j] = seen_in[j] ? 2 : 0;       // the caller's discard loop: 2 (k_track_frustum tells them from the frame's own points)
    for (int i = 0; i < n; i++) {
        const int mp = frame_mp_in[i];
        if (mp < 0) continue;
        if (pts->bad[mp]) continue;
        mpIn[i] = mp; seen[mp] = 1;
    }
    FrameDev fd;
    int rc;
    if ((rc = track_frame_dev(t, &fd)) != RUMI_OK || (rc = stage_pose(m, Tcw7, K4)) != RUMI_OK) return rc;
    if (n > 0) H2D(m->dFeatMp, mpIn.data(), n);
    if ((rc = stage_points(t, pts, true)) != RUMI_OK) return rc;
    if (nmp > 0) H2D(t->dSeen, seen.data(), nmp);
    FLUSH(m);
    if ((rc = track_local_body(t, fd, n, nmp, has_stale(pts), th_local, far_points, th_far_points, "rumi_track_local", res)) != RUMI_OK) return rc;
    if (n > 0) { std::memcpy(frame_mp, t->h.mpOut, (size_t)n * 4); std::memcpy(outlier, t->h.outF, (size_t)n); }
    unpack_in_view(t, nmp, n > 0, in_view, res);
    return RUMI_OK;
}

// Tracking::UpdateLocalMap + TrackLocalMap in one call: the store's local-map kernels, the table kernels of track_local_map.inc behind them in
// the same queue, one read of the two headers (the later launches are sized by n_table), then rumi_track_local's stages on the table the
// device built.  Nothing is written to the caller before the last stage has come back.
extern "C" int rumi_track_local_map(RumiTracker *t, RumiCovis *c, const float *K4, const float *Tcw7, const int32_t *frame_points, int32_t n_discarded,
                                    const int32_t *discarded_ids, const uint8_t *discarded_in_view, const float *discarded_proj5, float th_local,
                                    int32_t far_points, float th_far_points, uint8_t *frame_point_bad, int32_t *local_kf, int32_t kf_cap, int32_t *n_k1,
                                    int32_t *n_local_kf, int32_t *ref_kf, int32_t *table_ids, int32_t table_cap, int32_t *n_local_points, int32_t *n_table,
                                    int32_t *frame_mp, uint8_t *outlier, uint8_t *in_view, RumiTrackResult *res) {
    const char *entry = "rumi_track_local_map";
    if (!t || !c || !K4 || !Tcw7 || !res || !n_k1 || !n_local_kf || !ref_kf || !n_local_points || !n_table || kf_cap < 0 || table_cap < 0 || n_discarded < 0 ||
        (n_discarded > 0 && !discarded_ids) || (kf_cap > 0 && !local_kf) || (table_cap > 0 && (!table_ids || !in_view))) {
        g_lastError = std::string(entry) + ": missing argument or negative count";
        return RUMI_E_INVALID;
    }
    if (t->curN < 0) { g_lastError = std::string(entry) + ": no frame is resident (rumi_track_extract first)"; return RUMI_E_INVALID; }
    RumiMatcher *m = t->m;
    const int n = t->curN;
    if (n > 0 && (!frame_points || !frame_point_bad || !frame_mp || !outlier)) { g_lastError = std::string(entry) + ": missing per-feature array"; return RUMI_E_INVALID; }
    HIP_TRY(hipSetDevice(t->device));
    RumiTrackResult r;
    begin_entry(t, &r, Tcw7);
    FrameDev fd;
    int rc;
    if ((rc = track_frame_dev(t, &fd)) != RUMI_OK || (rc = stage_pose(m, Tcw7, K4)) != RUMI_OK) return rc;
    FLUSH(m);
    // ---- UpdateLocalMap: the store's kernels; the lists stay on the device
    const bool stale = discarded_in_view && discarded_proj5;
    const CovisDiscarded disc{n_discarded, discarded_ids, stale ? discarded_in_view : nullptr, stale ? discarded_proj5 : nullptr};
    CovisLocalView v;
    if ((rc = covis_local_map_launch(c, n, frame_points, &disc, t->device, entry, &v)) != RUMI_OK) return rc;
    // ---- the table: id -> row, the frame's extras and the discarded outliers in order, then the gather into the stages' arrays
    const int rowCap = std::min(t->maxPts, table_cap);
    const TableArgs TA{v, rowCap, m->dF[0], m->dF[1], m->dF[2], m->dF[3], m->dI[1], reinterpret_cast<uint32_t *>(m->dQDesc), t->dBad, t->dLocal, t->dSeen,
                       t->dStaleIn, t->dStaleProj, m->dFeatMp, t->d.tableIds};
    const int gRows = std::min(std::max(grid_of(rowCap), 1), 256);
    hipLaunchKernelGGL(k_table_mark, dim3(gRows), dim3(256), 0, nullptr, TA);
    if (n + n_discarded > 0) hipLaunchKernelGGL(k_table_claim, dim3(grid_of(n + n_discarded)), dim3(256), 0, nullptr, TA);
    hipLaunchKernelGGL(k_table_extras, dim3(1), dim3(kTableThreads), 0, nullptr, TA);
    hipLaunchKernelGGL(k_table_gather, dim3(gRows), dim3(256), 0, nullptr, TA);
    const int32_t *head, *kfs;
    const uint8_t *bad;
    if ((rc = covis_local_map_read(c, v, &head, &bad, &kfs)) != RUMI_OK) return rc;
    const int nK1 = head[0], nKf = head[1], refKf = head[2], nLocal = head[3], nmp = head[4], nMissing = head[5];
    if (nMissing > 0) {
        g_lastError = std::string(entry) + ": " + std::to_string(nMissing) + " local or frame point(s) without attributes (rumi_covis_set_point_attributes)";
        return RUMI_E_INVALID;
    }
    if (nKf > kf_cap || nmp > table_cap || nmp > t->maxPts) {
        g_lastError = std::string(entry) + ": kf_cap, table_cap or the tracker's max_points is too small for the lists";
        return RUMI_E_CAPACITY;
    }
    // ---- TrackLocalMap on that table
    // (the row ids travel behind the stages and are on the host when the body's copy of the result block returns)
    if (nmp > 0) HIP_TRY(hipMemcpyAsync(t->h.tableIds, t->d.tableIds, (size_t)nmp * 4, hipMemcpyDeviceToHost, nullptr));
    if ((rc = track_local_body(t, fd, n, nmp, stale, th_local, far_points, th_far_points, entry, &r)) != RUMI_OK) return rc;
    // ---- write-out
    if (n > 0) std::memcpy(frame_point_bad, bad, (size_t)n);
    if (nKf > 0) std::memcpy(local_kf, kfs, (size_t)nKf * 4);
    *n_k1 = nK1; *n_local_kf = nKf; *ref_kf = refKf; *n_local_points = nLocal; *n_table = nmp;
    if (nmp > 0) std::memcpy(table_ids, t->h.tableIds, (size_t)nmp * 4);
    for (int i = 0; i < n; i++) { const int row = t->h.mpOut[i]; frame_mp[i] = row >= 0 ? t->h.tableIds[row] : -1; }
    if (n > 0) std::memcpy(outlier, t->h.outF, (size_t)n);
    unpack_in_view(t, nmp, n > 0, in_view, &r);
    *res = r;
    return RUMI_OK;
}

/* mTrackProjX, mTrackProjY, mnTrackScaleLevel, mTrackViewCos, mTrackDepth of every table point as the SearchLocalPoints of the LAST rumi_track_frame /
 * rumi_track_local call left them (Frame::isInFrustum writes them into the MapPoint, Frame.cc:558-630; the values of a point that is not in view are
 * not meaningful).  They are still in the matcher's staging block: one more copy brings them.  Valid until the next rumi_track_* call. */
extern "C" int rumi_track_last_projections(RumiTracker *t, int32_t n_points, float *proj5_out) {
    if (!t || !proj5_out || n_points < 0) return RUMI_E_INVALID;
    if (t->projN <= 0 || n_points != t->projN) { g_lastError = "rumi_track_last_projections: no SearchLocalPoints result of that size is resident"; return RUMI_E_INVALID; }
    HIP_TRY(hipSetDevice(t->device));
    RumiMatcher *m = t->m;
    const FrustumBlock fb(m->stage.d, n_points), h(m->stage.h, n_points);
    HIP_TRY(hipMemcpy(h.x, fb.x, 5 * fb.n16 * sizeof(float), hipMemcpyDeviceToHost));        // the five word arrays; the flags are not wanted
    for (int i = 0; i < n_points; i++) { float *o = proj5_out + (size_t)i * 5; o[0] = h.x[i]; o[1] = h.y[i]; o[2] = (float)h.level[i]; o[3] = h.viewCos[i]; o[4] = h.depth[i]; }
    return RUMI_OK;
}

/* Lens distortion of the camera (Frame::UndistortKeyPoints / ComputeImageBounds, R/lib_src/Frame.cc:770-826; R/config/euroc_ori.yaml:23-31 has
 * k1 = -0.283): K4 = fx, fy, cx, cy of mK, dist5 = mDistCoef (k1, k2, p1, p2, k3).  From the next rumi_track_extract / rumi_track_frame on the
 * resident frame carries mvKeysUn (the grid, every search and PoseOptimization read those) and the undistorted image bounds; keys_out of those calls
 * stays mvKeys, as ExtractORB returns them.  dist5 == NULL or dist5[0] == 0: none (mvKeysUn = mvKeys, the reference's own test, Frame.cc:771). */
extern "C" int rumi_track_set_distortion(RumiTracker *t, const float *K4, const float *dist5) {
    if (!t) return RUMI_E_INVALID;
    if (!dist5 || dist5[0] == 0.0f) { t->distort = false; return RUMI_OK; }
    if (!K4 || !(K4[0] != 0.0f) || !(K4[1] != 0.0f)) { g_lastError = "rumi_track_set_distortion: camera matrix"; return RUMI_E_INVALID; }
    HIP_TRY(hipSetDevice(t->device));
    if (!t->dKeysUn) HIP_TRY(hipMalloc((void **)&t->dKeysUn, (size_t)t->cap * sizeof(RumiKeyPoint)));
    UndistortArgs &A = t->ua;
    A.fx = K4[0]; A.fy = K4[1]; A.cx = K4[2]; A.cy = K4[3]; A.ifx = 1. / A.fx; A.ify = 1. / A.fy;
    A.k1 = dist5[0]; A.k2 = dist5[1]; A.p1 = dist5[2]; A.p2 = dist5[3]; A.k3 = dist5[4];
    t->distort = true;
    t->curN = -1;                                          // a frame extracted under other coefficients is not this camera's
    return RUMI_OK;
}
/* mvKeysUn of the resident frame (keys_un_out [cap >= n]) and {mnMinX, mnMinY, mnMaxX, mnMaxY} (bounds4); either may be NULL. */
extern "C" int rumi_track_undistorted(RumiTracker *t, RumiKeyPoint *keys_un_out, int32_t cap, float *bounds4) {
    if (!t) return RUMI_E_INVALID;
    if (t->curN < 0) { g_lastError = "rumi_track_undistorted: no frame is resident"; return RUMI_E_INVALID; }
    if (bounds4) std::memcpy(bounds4, t->bounds, 16);
    if (keys_un_out && t->curN > 0) {
        if (cap < t->curN) return RUMI_E_CAPACITY;
        HIP_TRY(hipSetDevice(t->device));
        HIP_TRY(hipMemcpy(keys_un_out, resident_keys(t), (size_t)t->curN * sizeof(RumiKeyPoint), hipMemcpyDeviceToHost));
    }
    return RUMI_OK;
}

#include "track_reloc.inc"
#include "track_reloc_resident.inc"
