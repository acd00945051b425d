// The covisibility store (covis.hip) as its consumers see it: the device layout of its records, the one view a kernel reads them through, and
// the host door that checks a call's slots, agrees on the device and hands the view out ("The store's device layout").  Everything a
// kernel uses here is header-inline: the library is built without relocatable device code.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "rumi_orb.h"

typedef struct RumiCovis RumiCovis;

namespace rumi {

// ---- the records, all of 32-bit words ---------------------------------------------------------------------------------------------------
//   kf      [max_kf][20]      mp row (offset, length), children row (offset, length), flags, map, parent, has pose, order_key (two words), best[10]
//   pt      [max_points][4]   observer row (offset, length), flags, has attributes
//   attr    [max_points][16]  position 3, normal 3, min distance, max distance (f32), descriptor 8 words: two 16-byte aligned halves
//   rows                      the row arena: mp rows (point ids, -1 none), children rows, observer rows (observer words)
//   featTab [max_kf][4]       byte offset of the slot's key-points in the feature arena (64-bit, -1: none), feature count, -
//   centre  [max_kf][4]       GetCameraCenter() (3 x f32), has centre
//   ref     [max_points]      GetReferenceKeyFrame() as slot + 1, 0: none
//   oct     [max_kf][stride]  keys[i].octave of every slot that holds features (bytes)
//   pose    [max_kf][16]      GetPose() as the bundle adjustment reads it: eight doubles (unit quaternion x y z w, translation, 0), what
//                             ba_stage_poses makes of the caller's seven floats; "has pose" is word 7 of the kf record
//   ptMap   [max_points]      MapPoint::GetMap() in the key-frames' map_id numbering; "has map" is a bit of the pt record's flags word
constexpr int kCovisKfWords = 20, kCovisPointWords = 4, kCovisAttrWords = 16, kCovisFeatTabWords = 4, kCovisCentreWords = 4, kCovisPoseWords = 16;
constexpr int kCovisKfMpOff = 0, kCovisKfMpLen = 1, kCovisKfChOff = 2, kCovisKfChLen = 3, kCovisKfFlags = 4, kCovisKfMap = 5, kCovisKfParent = 6,
              kCovisKfHasPose = 7, kCovisKfKey = 8, kCovisKfBest = 10;
constexpr int kCovisKfBad = 1, kCovisKfLive = 2;                       // the kf record's flags word
constexpr int kCovisPointBad = 1, kCovisPointHasObsFeatures = 2, kCovisPointHasMap = 4;       // the pt record's flags word
constexpr int kCovisAttrDesc = 8;                                      // first descriptor word of an attr record
constexpr int kCovisObsSlotBits = 13, kCovisObsSlotMask = (1 << kCovisObsSlotBits) - 1;   // an observer word: slot | feature << 13

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
// offset finds the slot's record this many bytes before it.
constexpr uint32_t kCovisFeatKeysOffset = sizeof(CovisFeatRec);

// What the host knows of a slot without asking the device (covis_features_check).
struct CovisSlotFeatures { int32_t n, nn, ne, mpOff, mpLen; int64_t block; };     // mp row in the row arena (entries); block in the feature arena (bytes)
// What a kernel needs of it: the leading fields of every per-call key-frame record (SinKF, S3pJob, ResKF, BowSlotKF).  The block offset asks
// for 4-byte alignment only, so the record has no tail padding and the embedding record's own words follow at once.
typedef int64_t __attribute__((aligned(4))) CovisBlockOffset;
struct CovisSlotRef { CovisBlockOffset block; int32_t mpOff, n, nn; };
static_assert(sizeof(CovisSlotRef) == 20 && alignof(CovisSlotRef) == 4, "five words");
inline CovisSlotRef covis_slot_ref(const CovisSlotFeatures &I) { return CovisSlotRef{I.block, I.mpOff, I.n, I.nn}; }

template <class T> __device__ __forceinline__ const T *rec_arr(const CovisFeatRec *r, uint32_t o) {
    return reinterpret_cast<const T *>(reinterpret_cast<const uint8_t *>(r) + o);
}

// A 16-byte load that asks for 4-byte alignment only (the extractor's descriptor kernel loads its rows the same way, orb_orient_desc.inc):
// one wide instruction where the address happens to be aligned, never a fault where a row is not.
struct __attribute__((packed, aligned(4))) Dword4 { uint32_t x, y, z, w; };
__device__ __forceinline__ uint4 ld16_dword(const void *q) { const Dword4 t = *reinterpret_cast<const Dword4 *>(q); return make_uint4(t.x, t.y, t.z, t.w); }

// ---- the readers ------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int covis_obs_slot(int word) { return word & kCovisObsSlotMask; }
__device__ __forceinline__ int covis_obs_feature(int word) { return word >> kCovisObsSlotBits; }

// A point record, read as one 16-byte load.
struct CovisPoint {
    int4 w;
    __device__ __forceinline__ int obs_off() const { return w.x; }            // its observer row in the row arena
    __device__ __forceinline__ int obs_len() const { return w.y; }            // Observations() of the monocular model
    __device__ __forceinline__ bool bad() const { return (w.z & kCovisPointBad) != 0; }
    __device__ __forceinline__ bool has_obs_features() const { return (w.z & kCovisPointHasObsFeatures) != 0; }
    __device__ __forceinline__ bool has_map() const { return (w.z & kCovisPointHasMap) != 0; }    // (the map itself: CovisView::point_map)
    __device__ __forceinline__ int has_attr() const { return w.w; }           // (the table itself may still be missing: CovisView::has_attr)
};
// The eight floats of an attribute record, read as two 16-byte loads.
struct CovisAttrGeom {
    float4 lo, hi;
    __device__ __forceinline__ float min_dist() const { return hi.z; }
    __device__ __forceinline__ float max_dist() const { return hi.w; }
    __device__ __forceinline__ void pos(float *p) const { p[0] = lo.x; p[1] = lo.y; p[2] = lo.z; }
    __device__ __forceinline__ void normal(float *n) const { n[0] = lo.w; n[1] = hi.x; n[2] = hi.y; }
};
// One key-frame: its record in the feature arena and its map-point row.  A consumer's key-frame type adds only what is its own.
struct CovisKeyFrame {
    const CovisFeatRec *r; const int32_t *row;
    __device__ __forceinline__ int n() const { return r->n; }
    __device__ __forceinline__ int nn() const { return r->nn; }
    __device__ __forceinline__ int nlevels() const { return r->nlevels; }
    __device__ __forceinline__ const RumiKeyPoint *keys() const { return rec_arr<RumiKeyPoint>(r, r->keys); }
    __device__ __forceinline__ const uint8_t *desc() const { return rec_arr<uint8_t>(r, r->desc); }
    __device__ __forceinline__ const float *scale() const { return rec_arr<float>(r, r->scale); }
    __device__ __forceinline__ const uint32_t *nodes() const { return rec_arr<uint32_t>(r, r->nodes); }
    __device__ __forceinline__ const int32_t *off() const { return rec_arr<int32_t>(r, r->off); }
    __device__ __forceinline__ const uint32_t *idx() const { return rec_arr<uint32_t>(r, r->idx); }
    __device__ __forceinline__ const int32_t *mp() const { return row; }
    __device__ __forceinline__ const float *K() const { return r->K; }
};

// Where the store's tables lie on the device after covis_view; passed to kernels by value.  A pointer is null until the table exists: attr
// (no point has attributes), centre and ref (never set), feat (no key-frame has features), oct (no covis_view with kCovisWantOctaves yet; up to
// date only in a view that asked for it), pose and ptMap (never set).
struct CovisView {
    const int32_t *kf, *pt, *rows;
    int32_t *attr;                     // written in place by the refresh entry's write-back only
    const int32_t *featTab;
    const uint8_t *feat;
    const int32_t *centre, *ref;
    const uint8_t *oct;
    int octStride, maxKf, maxPoints, device;
    const double *pose;
    const int32_t *ptMap;

    // point record
    __device__ __forceinline__ CovisPoint point(int p) const { return CovisPoint{*reinterpret_cast<const int4 *>(pt + (size_t)p * kCovisPointWords)}; }
    __device__ __forceinline__ int2 point_obs(int p) const { return *reinterpret_cast<const int2 *>(pt + (size_t)p * kCovisPointWords); }     // (offset, length)
    __device__ __forceinline__ int point_obs_len(int p) const { return pt[(size_t)p * kCovisPointWords + 1]; }
    __device__ __forceinline__ bool point_bad(int p) const { return (pt[(size_t)p * kCovisPointWords + 2] & kCovisPointBad) != 0; }
    __device__ __forceinline__ bool has_attr(int p) const { return attr && pt[(size_t)p * kCovisPointWords + 3]; }
    __device__ __forceinline__ bool has_attr(const CovisPoint &P) const { return attr && P.has_attr(); }
    // attribute record
    __device__ __forceinline__ int32_t *attr_rec(int p) const { return attr + (size_t)p * kCovisAttrWords; }
    __device__ __forceinline__ const float *attr_pos(int p) const { return reinterpret_cast<const float *>(attr_rec(p)); }
    __device__ __forceinline__ CovisAttrGeom attr_geom(int p) const { const float4 *A = reinterpret_cast<const float4 *>(attr_rec(p)); return CovisAttrGeom{A[0], A[1]}; }
    __device__ __forceinline__ const int32_t *attr_desc(int p) const { return attr_rec(p) + kCovisAttrDesc; }
    __device__ __forceinline__ void attr_desc(int p, uint4 &q0, uint4 &q1) const { q0 = ld16_dword(attr_desc(p)); q1 = ld16_dword(attr_desc(p) + 4); }
    // key-frame record
    __device__ __forceinline__ const int32_t *kf_row(int slot) const { return rows + kf[slot * kCovisKfWords + kCovisKfMpOff]; }
    __device__ __forceinline__ int kf_row_entry(int slot, int f) const { return rows[kf[slot * kCovisKfWords + kCovisKfMpOff] + f]; }       // one index sum
    __device__ __forceinline__ int kf_row_len(int slot) const { return kf[slot * kCovisKfWords + kCovisKfMpLen]; }
    __device__ __forceinline__ bool kf_bad(int slot) const { return (kf[slot * kCovisKfWords + kCovisKfFlags] & kCovisKfBad) != 0; }
    __device__ __forceinline__ int kf_map(int slot) const { return kf[slot * kCovisKfWords + kCovisKfMap]; }
    __device__ __forceinline__ unsigned long long kf_key(int slot) const { return *reinterpret_cast<const unsigned long long *>(kf + slot * kCovisKfWords + kCovisKfKey); }
    // featTab
    __device__ __forceinline__ long long feat_keys(int slot) const { return *reinterpret_cast<const long long *>(featTab + slot * kCovisFeatTabWords); }     // < 0: none
    __device__ __forceinline__ int feat_count(int slot) const { return featTab[slot * kCovisFeatTabWords + 2]; }
    // feature block
    __device__ __forceinline__ const CovisFeatRec *rec(long long block) const { return reinterpret_cast<const CovisFeatRec *>(feat + block); }
    __device__ __forceinline__ const CovisFeatRec *rec_of_keys(long long keys) const { return rec(keys - (long long)kCovisFeatKeysOffset); }
    __device__ __forceinline__ const RumiKeyPoint *keys_at(long long keys) const { return reinterpret_cast<const RumiKeyPoint *>(feat + keys); }
    __device__ __forceinline__ const RumiKeyPoint *keys_of(const CovisSlotRef &s) const { return keys_at(s.block + kCovisFeatKeysOffset); }
    __device__ __forceinline__ const int32_t *mp_row(const CovisSlotRef &s) const { return rows + s.mpOff; }
    __device__ __forceinline__ CovisKeyFrame key_frame(const CovisSlotRef &s) const { return CovisKeyFrame{rec(s.block), mp_row(s)}; }
    // pose (eight doubles), the point's map
    __device__ __forceinline__ bool has_pose(int slot) const { return pose && kf[slot * kCovisKfWords + kCovisKfHasPose]; }
    __device__ __forceinline__ const double *pose_of(int slot) const { return pose + (size_t)slot * (kCovisPoseWords / 2); }
    __device__ __forceinline__ int point_map(int p) const { return ptMap[p]; }                    // meaningful where the point has_map()
    // centre, reference slot, octave
    __device__ __forceinline__ float4 centre_of(int slot) const { return *reinterpret_cast<const float4 *>(centre + slot * kCovisCentreWords); }   // w != 0: has centre
    __device__ __forceinline__ int ref_slot(int p) const { return ref ? ref[p] - 1 : -1; }
    __device__ __forceinline__ int octave(int slot, int f) const { return (int)oct[(size_t)slot * octStride + f]; }
};

// ---- the host door (covis.hip, covis_features.inc, covis_refresh.inc) -------------------------------------------------------------------
// Host only, no device call by anyone: the one device rule of the by-slot entries.  A store without a device takes the consumer's; a store
// on another device is refused with RUMI_E_INVALID ("... different devices").  wantDevice < 0: the consumer has not named a device yet (it
// takes the current one when it binds) and nothing is compared; such an entry asks again once it has bound.
int covis_same_device(RumiCovis *c, int wantDevice, const char *entry);
// Host only: every slot live, with features, named once, feature count == length of its mp row.  Refused with RUMI_E_INVALID and the message set.
int covis_features_check(RumiCovis *c, int n, const int32_t *slots, const char *entry, CovisSlotFeatures *info);
// Host only: the point ids the store's tables hold (max_points of rumi_covis_create).
int covis_max_points(const RumiCovis *c);
// Binds the store, sends the staged edits, sends the staged features, with kCovisWantOctaves brings the octave table up to date (only the
// culling entry pays for that), and says where the tables lie.  Enqueues on the null stream, does not synchronise.
constexpr int kCovisWantOctaves = 1;
int covis_view(RumiCovis *c, int want, CovisView *view);

// Host only, from the store's mirror: is the slot live, its bad bit, its feature count (-1: no features), its mp row.
struct CovisCullSlot { int32_t live, bad, nFeat, mpOff, mpLen; };
void covis_cull_slot(const RumiCovis *c, int32_t slot, CovisCullSlot *out);
// Host only: the points of the row [mpOff, mpOff + mpLen): how many lack observation features, the longest observer row among them.
void covis_cull_row_points(const RumiCovis *c, int32_t mpOff, int32_t mpLen, int32_t *without, int32_t *longest);

// One point's results as the refresh kernels leave them and the host reads them back (refresh_resident.inc).
struct CovisRefreshOut {
    int32_t bestObs, bestMedian;
    float normal[3], minD, maxD;
    int32_t updated;
    uint32_t desc[8];                          // the winning row, where bestObs >= 0
};
static_assert(sizeof(CovisRefreshOut) == 64, "one record a point comes back");
// Host only, from the store's mirror, O(1) per id: every id in range and named once; rowLen[i] = the length of its observer row; a point with
// observers has observation features; with needAttr every point has attributes.  Refused with RUMI_E_INVALID and the message set.
int covis_refresh_check(RumiCovis *c, int n, const int32_t *ids, bool needAttr, const char *entry, int32_t *rowLen);
// The host half of the write-back: the mirror's attribute records take what the device's took (descriptor where bestObs >= 0, normal and
// distance range where updated; a point with an empty row is skipped).  No edit is staged.
void covis_refresh_write_mirror(RumiCovis *c, int n, const int32_t *ids, const int32_t *rowLen, const CovisRefreshOut *out, bool desc, bool normal);

// ---- the local-map query as the tracker's rumi_track_local_map drives it (track.hip, track_local_map.inc) -------------------------------
// The discarded outliers of the previous Tracking function: ids (distinct), and optionally what an earlier frame left in them.
struct CovisDiscarded { int n; const int32_t *ids; const uint8_t *inView; const float *proj5; };
// The store's tables and the lists of the local-map kernels after covis_local_map_launch.
struct CovisLocalView {
    CovisView t;
    int nFrame, nDiscarded;
    uint32_t epoch;                    // of this query: the stamp of tag and rowOf
    unsigned long long *rowOf;         // [max_points] (epoch << 32) | value, see track_local_map.inc (null without CovisDiscarded)
    int32_t *head;                     // {n_k1, n_local_kf, ref_kf, n_local_points} {n_table, rows without attributes, -, -}
    const int32_t *localPts;           // mvpLocalMapPoints [n_local_points]
    const int32_t *framePts, *discIds; // the query's input as uploaded: [nFrame], [nDiscarded]
    const uint8_t *discInView;         // [nDiscarded] or null
    const float *discProj;             // [nDiscarded][5] or null
    size_t offBad, offKf, offPts, headBytes;      // byte offsets inside the store's output block (covis_local_map_read)
};
// Validates, applies covis_same_device (wantDevice < 0: rumi_covis_local_map, no consumer), uploads the staged edits and the input, launches
// k_covis_count<true> and k_covis_local<1..3> on the null stream and returns without reading anything back.  d: the table entry's discarded
// outliers (null: rumi_covis_local_map).
int covis_local_map_launch(RumiCovis *c, int n, const int32_t *frame_points, const CovisDiscarded *d, int wantDevice, const char *entry, CovisLocalView *view);
// Both headers, the frame's bad flags [nFrame] and the local key-frames, as host pointers into the store's pinned block (synchronises).
int covis_local_map_read(RumiCovis *c, const CovisLocalView &v, const int32_t **head8, const uint8_t **frameBad, const int32_t **localKf);

// ---- the window of rumi_local_ba_resident (opt.hip, ba_resident_host.inc), host only, from the store's mirror ---------------------------
// lLocalKeyFrames (Optimizer.cc:1007-1017): the current slot, then the neighbours that are not bad and share its map, in the caller's order.
struct CovisLbaWindow { int32_t nLocal, initIdx, hiSlot, curMap, maxRow; int64_t sumRows; float K4[4]; };
// Validates (cur live with features; neighbours live, distinct, never cur; init -1 or a slot), then fills locals [n_neigh + 1], role
// [RUMI_COVIS_MAX_KEYFRAMES] (the index in locals, -1 for every other slot; hiSlot of them are meaningful.  A neighbour dropped as bad or of
// another map needs no role of its own: the tests that dropped it keep it from being a fixed camera, Optimizer.cc:1050) and *w (initIdx: where init lies in locals or -1; maxRow / sumRows: the longest local
// map-point row and their total; K4: the current slot's).  Refused with RUMI_E_INVALID and the message set.
int covis_lba_window(RumiCovis *c, int32_t cur, const int32_t *neigh, int32_t nNeigh, int32_t init, const char *entry, int32_t *locals, int32_t *role, CovisLbaWindow *w);
// The seven floats rumi_covis_set_keyframe_poses was given for the slot (zeros where it has none).
void covis_lba_pose7(const RumiCovis *c, int32_t slot, float *pose7);
// The mirror's half of the position write-back: attribute record of ids[i] takes pos3[i].  No edit is staged (the device half is the caller's kernel).
void covis_lba_write_positions(RumiCovis *c, int32_t n, const int32_t *ids, const float *pos3);

}  // namespace rumi
