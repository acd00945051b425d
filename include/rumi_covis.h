/* rumi_covis.h — C ABI of the MI355X covisibility store: KeyFrame::UpdateConnections for a batch, Tracking::UpdateLocalMap for a frame.
 *
 * Replaces the two members of the reference that histogram key-frames over observation lists:
 *   KeyFrame::UpdateConnections / UpdateCloudConnections   R/lib_src/KeyFrame.cc:487-574, :576+   (the counting and the two orderings)
 *   Tracking::UpdateLocalKeyFrames + UpdateLocalPoints     R/lib_src/Tracking.cc:3067-3210        (monocular, IMU not initialised)
 *
 * The handle keeps, on the device and between calls, what those members read and nothing else.  A key-frame is a slot 0 .. max_kf-1 chosen
 * by the caller, a map point an id 0 .. max_points-1.
 *   per key-frame slot: mp[n] (GetMapPointMatches as point ids, -1 = NULL), is_bad, map_id, order_key, best[10]
 *                       (GetBestCovisibilityKeyFrames(10) as slots, -1 padded), parent slot or -1, the children as a slot list; and
 *                       optionally its features (rumi_covis_set_keyframe_features, below), which the two members above do not read
 *   per point:          is_bad, the observers (the key-frame slots of GetObservations(), and with rumi_covis_set_point_observations the
 *                       feature index of each, plus a "has observation features" bit: rumi_keyframe_culling_resident reads the observer's
 *                       octave through it), and optionally the attributes TrackLocalMap reads: GetWorldPos, GetNormal, mfMinDistance, mfMaxDistance, GetDescriptor, and a "has
 *                       attributes" bit.  Observations() is not a field: for the monocular model it is the length of the observer row.
 *                       isBad() is the bit rumi_covis_set_points / rumi_covis_set_bad maintain.  rumi_track_local_map (rumi_track.h) builds
 *                       its point table from these on the device.
 *
 * order_key restates pointer order.  Every ordered walk in the two members is a walk of a std::map<KeyFrame*, ..> or a
 * std::set<KeyFrame*>, and every tie of sort(vPairs) is broken by the KeyFrame*: "pointer order" here is ascending order_key, distinct per
 * live slot and unrelated to slot numbers.  A C++ host passes the pointer value.
 *
 * Edits (rumi_covis_set_*) are validated, then staged on the host; the next query uploads them in one block whose size follows what
 * changed, not the map.  A slot is live once rumi_covis_set_keyframes has named it, and stays live.  Every slot a call names (observers,
 * best, parent, children, the batch) must be live, or become live in the same rumi_covis_set_keyframes call.  A refused call
 * (RUMI_E_INVALID, RUMI_E_CAPACITY) leaves the state and every output untouched.
 *
 * Both queries are integer-only: two calls on the same state return the same bytes.  They work on the default (null) stream and return
 * when their results are on the host.  Status codes as in rumi_orb.h.  No CPU fallback. */
#ifndef RUMI_COVIS_H
#define RUMI_COVIS_H
#include <stdint.h>

#include "rumi_match.h"
#include "rumi_orb.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct RumiCovis RumiCovis;

#define RUMI_COVIS_MAX_KEYFRAMES 8192 /* slots: one 32-bit LDS counter each (32 KiB of a workgroup's LDS), see DESIGN 4o */
#define RUMI_COVIS_MAX_FEATURES 65536 /* longest mp row, and the most points a frame passes */
#define RUMI_COVIS_NBEST 10           /* GetBestCovisibilityKeyFrames(10) */
#define RUMI_COVIS_TH 15              /* KeyFrame.cc:524 */
#define RUMI_COVIS_LOCAL_LIMIT 80     /* Tracking.cc:3150 */

enum { RUMI_COVIS_CONNECTED = 0, RUMI_COVIS_EMPTY = 1 }; /* EMPTY: the early return at KeyFrame.cc:519, the host writes nothing */

/* max_kf <= RUMI_COVIS_MAX_KEYFRAMES (RUMI_E_CAPACITY above).  arena_entries: first size of the row arena in 32-bit entries (0: a default);
 * it is compacted when full and doubled when the live rows fill more than three quarters of it. */
int rumi_covis_create(int32_t max_kf, int32_t max_points, int64_t arena_entries, int32_t device, RumiCovis **out);
void rumi_covis_destroy(RumiCovis *c);

/* n key-frames, each slot at most once: mp row of entry i = mp[mp_off[i] .. mp_off[i+1]), children = children[child_off[i] .. child_off[i+1])
 * (distinct slots, never the key-frame itself), best [n][10], parent [n].  order_keys distinct among the live slots after the call.
 * map_ids, is_bad as they are now. */
int rumi_covis_set_keyframes(RumiCovis *c, int32_t n, const int32_t *slots, const uint64_t *order_keys, const int32_t *map_ids, const uint8_t *is_bad,
                             const int32_t *mp_off, const int32_t *mp, const int32_t *best, const int32_t *parent, const int32_t *child_off,
                             const int32_t *children);
/* n points, each id at most once: observers of entry i = obs[obs_off[i] .. obs_off[i+1]), distinct live slots. */
int rumi_covis_set_points(RumiCovis *c, int32_t n, const int32_t *ids, const uint8_t *is_bad, const int32_t *obs_off, const int32_t *obs);
/* rumi_covis_set_points, and per observer the feature index GetObservations() holds for it (get<0> of the tuple).
 * obs_feature[j] in 0 .. RUMI_COVIS_MAX_FEATURES-1.  A point set through this entry "has observation features"; a point set
 * later through rumi_covis_set_points loses them again.  Same checks and messages as rumi_covis_set_points, plus the feature range.  Whether
 * (slot, feature) agrees with the slot's map-point row is checked by the query that reads it, not here. */
int rumi_covis_set_point_observations(RumiCovis *c, int32_t n, const int32_t *ids, const uint8_t *is_bad, const int32_t *obs_off, const int32_t *obs_slot,
                                      const int32_t *obs_feature);
/* The attributes of n points, each id at most once: pos / normal [n][3], min_dist / max_dist [n] (raw: isInFrustum applies 0.8 and 1.2),
 * desc [n][32].  To be called where the reference calls SetWorldPos, UpdateNormalAndDepth and ComputeDistinctiveDescriptors.  Staged like every
 * edit: the next query uploads the changed records.  A point keeps its attributes until they are set again. */
int rumi_covis_set_point_attributes(RumiCovis *c, int32_t n, const int32_t *ids, const float *pos, const float *normal, const float *min_dist,
                                    const float *max_dist, const uint8_t *desc);
/* GetCameraCenter() of n live slots, each at most once, Ow [n][3] finite.  To be called where the reference calls SetPose.  A slot set here
 * "has a centre" from then on.  Staged like every edit: 16 bytes a key-frame go up with the next query.  Read by
 * rumi_refresh_map_points_resident (rumi_mapping.h) and by nothing else. */
int rumi_covis_set_keyframe_centres(RumiCovis *c, int32_t n, const int32_t *slots, const float *Ow);
/* GetReferenceKeyFrame() of n points as a live slot, -1 clears it; ids each at most once and inside 0..max_points-1.  To be called wherever
 * SetReferenceKeyFrame or EraseObservation changes mpRefKF.  Staged like every edit, one word a point. */
int rumi_covis_set_point_reference(RumiCovis *c, int32_t n, const int32_t *ids, const int32_t *ref_slots);
/* GetPose() of n live slots, each at most once, as qx qy qz qw tx ty tz, all finite.  To be called where the reference calls SetPose, beside
 * rumi_covis_set_keyframe_centres.  The store keeps what the bundle adjustment makes of the seven floats before it uploads them (eight doubles,
 * 64 bytes a key-frame: the normalised quaternion, the translation, a zero), converted here on the host by the same function, so that
 * rumi_local_ba_resident (rumi_opt.h) reads the bytes rumi_local_ba would upload.  A slot set here "has a pose" from then on.  Staged like
 * every edit; the table does not exist until the first call. */
int rumi_covis_set_keyframe_poses(RumiCovis *c, int32_t n, const int32_t *slots, const float *pose7);
/* MapPoint::GetMap() of n points in the numbering of the key-frames' map_id; ids each at most once and inside 0..max_points-1.  A point set
 * here "has a map" from then on (rumi_covis_set_points keeps the bit).  Staged like every edit, one word a point.  Read by
 * rumi_local_ba_resident (Optimizer.cc:1032 asks pMP->GetMap() == pCurrentMap) and by nothing else. */
int rumi_covis_set_point_maps(RumiCovis *c, int32_t n, const int32_t *ids, const int32_t *map_ids);
/* The length of a live slot's map-point row as the last rumi_covis_set_keyframes left it (host only, no device call); -1 for a slot that is
 * not live or a missing handle.  For callers that size an output by it (rumi_search_in_neighbors_resident, rumi_mapping.h). */
int32_t rumi_covis_row_length(const RumiCovis *c, int32_t slot);
/* KeyFrame::isBad of n_kf live slots and MapPoint::isBad of n_pt points. */
int rumi_covis_set_bad(RumiCovis *c, int32_t n_kf, const int32_t *slots, const uint8_t *kf_bad, int32_t n_pt, const int32_t *ids, const uint8_t *pt_bad);
/* KeyFrame::GetMap of n live slots changed (map merge). */
int rumi_covis_set_maps(RumiCovis *c, int32_t n, const int32_t *slots, const int32_t *map_ids);

/* ---- Key-frame features: what never changes after the key-frame is built -- mvKeysUn (whole RumiKeyPoint records, angle included),
 * mDescriptors, mvScaleFactors, mFeatVec (CSR) and fx fy cx cy -- kept on the device once per key-frame, so that a consumer names slots
 * instead of uploading key-frames (rumi_create_new_map_points_resident, rumi_mapping.h).  The host keeps no copy of the feature bytes, only
 * where each block lies.
 *
 * slot must be live.  Setting a slot again replaces its features.  Validated like rumi_create_new_map_points validates a key-frame (sizes,
 * octaves inside nlevels, FeatureVector offsets and indices in range, node ids strictly ascending, no feature listed twice; the same
 * messages), and at most RUMI_COVIS_MAX_FEATURES features (RUMI_E_CAPACITY).  Staged like every edit: the call makes no device call, the
 * next consumer sends what is staged.  A refused call leaves the store untouched. */
int rumi_covis_set_keyframe_features(RumiCovis *c, int32_t slot, const RumiFrameFeatures *feat, const RumiFeatureVector *fv, const float *K4);
/* n slots inside 0..max_kf-1; a slot without features is not an error.  The blocks become free space that later key-frames reuse. */
int rumi_covis_drop_keyframe_features(RumiCovis *c, int32_t n, const int32_t *slots);
/* First size of the feature arena in bytes (0: a default); before the first rumi_covis_set_keyframe_features, RUMI_E_INVALID afterwards.
 * The arena doubles when a block fits neither a free block nor the tail; growth copies device to device. */
int rumi_covis_reserve_features(RumiCovis *c, int64_t bytes);
/* out6: arena capacity, bytes in use, slots that hold features, growths, compactions (0: freed blocks are reused through a free list),
 * bytes of feature data in the last upload. */
int rumi_covis_feature_stats(const RumiCovis *c, int64_t *out6);

/* KeyFrame::UpdateConnections for the key-frames batch[0 .. B), live slots in this order; a slot may repeat.  Per entry b:
 *   status[b]                                                  RUMI_COVIS_CONNECTED or RUMI_COVIS_EMPTY (both lists empty then)
 *   (conn_slot, conn_count)[conn_off[b] .. conn_off[b+1])      KFcounter = mConnectedKeyFrameWeights, in key order
 *   (ord_slot, ord_weight)[ord_off[b] .. ord_off[b+1])         mvpOrderedConnectedKeyFrames / mvOrderedWeights: the entries with count >= 15,
 *                                                              or the single (pKFmax, nmax); weight descending, key descending among equals
 * The counting reads no connection state, so the B results do not depend on each other; the host replays AddConnection, the member writes
 * and the parent choice in batch order.  conn_cap / ord_cap: capacities of the caller's arrays; RUMI_E_CAPACITY, nothing written, when a
 * list does not fit. */
int rumi_covis_update_connections(RumiCovis *c, int32_t B, const int32_t *batch, int32_t *status, int32_t *conn_off, int32_t *conn_slot,
                                  int32_t *conn_count, int64_t conn_cap, int32_t *ord_off, int32_t *ord_slot, int32_t *ord_weight, int64_t ord_cap);

/* Tracking::UpdateLocalKeyFrames + UpdateLocalPoints for one frame.  frame_points [n]: mCurrentFrame.mvpMapPoints as point ids, -1 = NULL.
 *   frame_point_bad [n]     1 where the point is bad: it gave no vote and the caller NULLs it (Tracking.cc:3102)
 *   local_kf [n_local_kf]   mvpLocalKeyFrames; the first n_k1 are the voted key-frames in key order
 *   ref_kf                  pKFmax, or -1 (mpReferenceKF stays)
 *   local_points            mvpLocalMapPoints
 * mnTrackReferenceForFrame of key-frames and points is the de-duplication of this call and nothing else: the coincidence of frame id 0
 * with the stamp's initial value is not reproduced.  RUMI_E_CAPACITY, nothing written, when kf_cap or pt_cap is too small. */
int rumi_covis_local_map(RumiCovis *c, int32_t n, const int32_t *frame_points, uint8_t *frame_point_bad, int32_t *local_kf, int32_t kf_cap,
                         int32_t *n_k1, int32_t *n_local_kf, int32_t *ref_kf, int32_t *local_points, int32_t pt_cap, int32_t *n_local_points);

/* The last query, in ms: validation + staging | upload, kernels, download | write-out. */
int rumi_covis_stage_ms(const RumiCovis *c, float *out3);
/* out7: arena capacity, tail, live entries (all in 32-bit entries), rows re-placed at the tail, compactions, growths, bytes of the last upload
 * (attribute, centre, reference, pose and point-map edits included). */
int rumi_covis_stats(const RumiCovis *c, int64_t *out7);

#ifdef __cplusplus
}
#endif
#endif
