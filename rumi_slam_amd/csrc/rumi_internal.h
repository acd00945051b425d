// Entry points one translation unit of librumi_hip.so offers another (not part of the C ABI).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

typedef struct RumiVocabulary RumiVocabulary;
typedef struct RumiMatcher RumiMatcher;
typedef struct RumiCovis RumiCovis;

namespace rumi {

// ---- the covisibility store (covis.hip) as the tracker's rumi_track_local_map drives it (track.hip, track_local_map.inc) ----
constexpr int kCovisPointWords = 4;    // pt record: observer row (offset, length), flags (bit 0 bad, bit 1 has observation features), has attributes
constexpr int kCovisAttrWords = 16;    // attr record: position 3, normal 3, min distance, max distance (f32), descriptor 8 words
constexpr int kCovisPointHasObsFeatures = 2;           // in the flags word
constexpr int kCovisObsSlotBits = 13, kCovisObsSlotMask = (1 << kCovisObsSlotBits) - 1;   // an observer entry: slot | feature << 13
constexpr int kCovisKfWords = 20, kCovisKfMpOff = 0, kCovisKfMpLen = 1;                   // kf record: where its mp row lies in the row arena
constexpr int kCovisFeatTabWords = 4;  // featTab record: byte offset of the slot's key-points in the feature arena (64-bit, -1: none), feature count, -
// The discarded outliers of the previous Tracking function: ids (distinct), and optionally what an earlier frame left in them.
struct CovisDiscarded { int n; const int32_t *ids; const uint8_t *inView; const float *proj5; };
// Where the store's tables and the lists of the local-map kernels lie on the device after covis_local_map_launch.
struct CovisLocalView {
    int device, maxPoints, nFrame, nDiscarded;
    uint32_t epoch;                    // of this query: the stamp of tag and rowOf
    const int32_t *pt, *attr;          // [max_points][kCovisPointWords], [max_points][kCovisAttrWords] (null: no point has attributes)
    unsigned long long *rowOf;         // [max_points] (epoch << 32) | value, see track_local_map.inc (null without CovisDiscarded)
    int32_t *head;                     // {n_k1, n_local_kf, ref_kf, n_local_points} {n_table, rows without attributes, -, -}
    const int32_t *localPts;           // mvpLocalMapPoints [n_local_points]
    const int32_t *framePts, *discIds; // the query's input as uploaded: [nFrame], [nDiscarded]
    const uint8_t *discInView;         // [nDiscarded] or null
    const float *discProj;             // [nDiscarded][5] or null
    size_t offBad, offKf, offPts, headBytes;      // byte offsets inside the store's output block (covis_local_map_read)
};
// Validates, uploads the staged edits and the input, launches k_covis_count<true> and k_covis_local<1..3> on the null stream and returns
// without reading anything back.  d: the table entry's discarded outliers (null: rumi_covis_local_map).  wantDevice >= 0: refused with
// RUMI_E_INVALID when the store lives on another device.
int covis_local_map_launch(RumiCovis *c, int n, const int32_t *frame_points, const CovisDiscarded *d, int wantDevice, const char *entry, CovisLocalView *view);
// Both headers, the frame's bad flags [nFrame] and the local key-frames, as host pointers into the store's pinned block (synchronises).
int covis_local_map_read(RumiCovis *c, const CovisLocalView &v, const int32_t **head8, const uint8_t **frameBad, const int32_t **localKf);

// ---- the store's key-frame features (covis_features.inc) as rumi_create_new_map_points_resident reads them (mapping.hip) ----
// A key-frame's block in the feature arena starts with this record; every array lies `its field` bytes behind the record's own address,
// 16-byte aligned: RumiKeyPoint keys [n], desc [n][32], scale [nlevels], then mFeatVec as node ids [nn], offsets [nn + 1], indices [ne].
struct CovisFeatRec {
    int32_t n, nn, ne, nlevels;
    float K[4];                        // fx fy cx cy
    uint32_t keys, desc, scale, nodes, off, idx;
    uint32_t bytes, pad;               // of the whole block, record included
};
static_assert(sizeof(CovisFeatRec) == 64, "the arrays behind the record start 16-byte aligned");
// The key-points are the first array behind the record (feat_layout refuses any other placement): a kernel that holds featTab's key-point
// offset finds the slot's record this many bytes before it (refresh_resident.inc).
constexpr uint32_t kCovisFeatKeysOffset = sizeof(CovisFeatRec);
// What the host knows of a slot without asking the device.
struct CovisSlotFeatures { int32_t n, nn, ne, mpOff, mpLen; int64_t block; };     // mp row in the row arena (entries); block in the feature arena (bytes)
struct CovisFeatureView {
    const int32_t *rows, *pt, *attr;   // the row arena, [max_points][kCovisPointWords], [max_points][kCovisAttrWords] (null: no point has attributes)
    const uint8_t *feat;               // the feature arena
    int maxKf, maxPoints;              // slots and point ids the tables hold
};
// Host only: every slot live, with features, named once, feature count == length of its mp row; with wantDevice >= 0 the store on that
// device (a store without a device yet takes it).  Refused with RUMI_E_INVALID and the message set.
int covis_features_check(RumiCovis *c, int n, const int32_t *slots, int wantDevice, const char *entry, CovisSlotFeatures *info);
// Host only: the point ids the store's tables hold (max_points of rumi_covis_create).
int covis_max_points(const RumiCovis *c);
// Sends the staged edits and the staged features; where the tables lie afterwards.  Enqueues on the null stream, does not synchronise.
int covis_features_flush(RumiCovis *c, CovisFeatureView *view);

// ---- the store as rumi_keyframe_culling_resident reads it (culling.hip) ----
struct CovisCullView {
    const int32_t *kf, *pt, *rows, *featTab;   // [max_kf][kCovisKfWords], [max_points][kCovisPointWords], the row arena, [max_kf][kCovisFeatTabWords]
    const uint8_t *oct;                        // [max_kf][octStride] keys[i].octave of every slot that holds features
    int octStride;
    int maxKf, maxPoints, device;
};
// Host only, from the store's mirror: is the slot live, its bad bit, its feature count (-1: no features), its mp row.
struct CovisCullSlot { int32_t live, bad, nFeat, mpOff, mpLen; };
void covis_cull_slot(const RumiCovis *c, int32_t slot, CovisCullSlot *out);
// Host only: the points of the row [mpOff, mpOff + mpLen): how many lack observation features, the longest observer row among them.
void covis_cull_row_points(const RumiCovis *c, int32_t mpOff, int32_t mpLen, int32_t *without, int32_t *longest);
// Binds the store (wantDevice as above), sends the staged edits and features, brings the octave table up to date; where the tables lie.
// Does not synchronise.
int covis_cull_flush(RumiCovis *c, int wantDevice, const char *entry, CovisCullView *view);

// ---- the store as rumi_refresh_map_points_resident reads and writes it (refresh.hip, refresh_resident.inc; covis_refresh.inc) ----
constexpr int kCovisKfFlags = 4;       // kf record: the flags word (bit 0 bad, bit 1 live)
constexpr int kCovisCentreWords = 4;   // centre record: GetCameraCenter() (3 x f32), has centre
struct CovisRefreshView {
    const int32_t *kf, *pt, *rows, *featTab;   // as CovisCullView
    const int32_t *centre, *ref;               // [max_kf][kCovisCentreWords], [max_points] slot + 1 (0: none); null: never set
    int32_t *attr;                             // [max_points][kCovisAttrWords], written by the write-back; null: no point has attributes
    const uint8_t *feat;                       // the feature arena (a slot's CovisFeatRec lies kCovisFeatKeysOffset bytes before its key-points)
    int device;
};
// One point's results as the kernels leave them and the host reads them back.
struct CovisRefreshOut {
    int32_t bestObs, bestMedian;
    float normal[3], minD, maxD;
    int32_t updated;
    uint32_t desc[8];                          // the winning row, where bestObs >= 0
};
static_assert(sizeof(CovisRefreshOut) == 64, "one record a point comes back");
// Host only, from the store's mirror, O(1) per id: every id in range and named once; rowLen[i] = the length of its observer row; a point with
// observers has observation features; with needAttr every point has attributes; with both devices known they are the same.  Refused with
// RUMI_E_INVALID and the message set.
int covis_refresh_check(RumiCovis *c, int n, const int32_t *ids, bool needAttr, int wantDevice, const char *entry, int32_t *rowLen);
// wantDevice: the consumer's device, resolved.  A store on another device is refused before the store makes any device call; a store without a
// device takes the consumer's.  Then binds the store, sends the staged edits and features; where the tables lie.  Does not synchronise.
int covis_refresh_flush(RumiCovis *c, int wantDevice, const char *entry, CovisRefreshView *view);
// The host half of the write-back: the mirror's attribute records take what the device's took (descriptor where bestObs >= 0, normal and
// distance range where updated; a point with an empty row is skipped).  No edit is staged.
void covis_refresh_write_mirror(RumiCovis *c, int n, const int32_t *ids, const int32_t *rowLen, const CovisRefreshOut *out, bool desc, bool normal);

// Correspondences the LDS instantiation of k_pose_opt holds (opt.hip).  The tracker (track.hip) launches ONLY that instantiation when it knows a
// frame cannot have more (nfeatures 1000 + the extractor's slack of 96 fits), so both files take the number from here.
constexpr int kPoseLdsEdges = 1152;

// Optimizer::PoseOptimization of ONE frame whose correspondences already lie on the device (opt.hip, k_pose_opt): dStart = {0, n} (n read by the
// kernel, not by the host), Xw [n][3], obs [n][2], w [n] (invLevelSigma2), K4, Tin [7] -> Tout [7], outlier [n], nGood [1].  dActive [cap] and
// dLastChi2 [cap] are scratch for frames of more than 1024 correspondences; fitsLds: the caller knows the count is at most 1024 (the second
// instantiation is then not launched).  Enqueues on `st`, does not synchronise.  nbatch > 1 (rumi_track_reloc_refine): dStart [nbatch + 1],
// problem b's correspondences at dStart[b] .. dStart[b + 1], Tin / Tout [nbatch][7], nGood [nbatch], one workgroup each; fitsLds must then
// hold for every problem.
int pose_opt_device(const int32_t *dStart, const float *dXw, const float *dObs, const float *dW, const float *dK4, const float *dTin, float *dTout,
                    uint8_t *dOutlier, int32_t *dNGood, uint8_t *dActive, double *dLastChi2, bool fitsLds, hipStream_t st, int nbatch = 1);

// Device, word count and the header's weighting / scoring types of a vocabulary (voc.hip), for the key-frame database (kfdb.hip).
void voc_params(const RumiVocabulary *v, int *device, int *nWords, int *weighting, int *scoring);

// What another translation unit hangs on a RumiMatcher (match_host.h): mapping.hip keeps the blocks of rumi_create_new_map_points here, so that
// they live and die with the handle.
struct MatcherExt { void *state = nullptr; void (*destroy)(void *) = nullptr; };

// k_bruteforce_pair (match.hip, match_bruteforce_pair.inc) for the streaming front-end (orb_host.hip): rumi_match_bruteforce_pair_device with the
// caller's bound on the train count (the slice rule sees min(nt_bound, cap) rows) and, when `mirror` is set, a second copy of the query frame and
// of the results written by the same launch: counts {n, monoIndex, n_prev} (d_nq then points at the extractor's {n, monoIndex} pair), the query's
// key-points (from kp_src) and descriptors (desc 16-byte aligned) and the three result rows -- the device's view of a pinned host block.
// The arguments are not checked.  Enqueues on `st`, does not synchronise.
struct PairMirrorArgs { void *counts; const void *kp_src; void *kp, *desc, *best_idx, *best_dist, *second_dist; };
int launch_bruteforce_pair(const void *qd, const void *nq, const void *td, const void *nt, int cap, int nt_bound, int slices, void *scratch, void *best_idx,
                           void *best_dist, void *second_dist, const PairMirrorArgs *mirror, hipStream_t st);

}  // namespace rumi
