/*
 * rumi_mapping.h — C ABI of the LocalMapping members that have no ORBmatcher form (librumi_hip.so).
 *
 * Drop-in boundary (R/ = the reference's src/rumi-slam/):
 *   R/lib_src/LocalMapping.cc:354-647     LocalMapping::CreateNewMapPoints, monocular pinhole branch
 *   R/lib_src/ORBmatcher.cc:806-1013      ORBmatcher::SearchForTriangulation (as rumi_search_for_triangulation, rumi_match.h)
 *   R/lib_src/KeyFrame.cc:947-978         KeyFrame::ComputeSceneMedianDepth(2)
 *   R/lib_src/GeometricTools.cc:47-66     GeometricTools::Triangulate
 *   R/lib_src/CameraModels/Pinhole.cpp:30-33,61-64   Pinhole::project / unprojectEig
 *   R/lib_src/MapPoint.cc:353-427, 450-518   MapPoint::ComputeDistinctiveDescriptors / UpdateNormalAndDepth (rumi_refresh_map_points, below)
 *   R/lib_src/LocalMapping.cc:953-1079, 820-951   LocalMapping::KeyFrameCulling / CloudKeyFrameCulling (rumi_keyframe_culling, below)
 *   R/lib_src/LocalMapping.cc:649-743, ORBmatcher.cc:1058-1161   the searches of LocalMapping::SearchInNeighbors (rumi_search_in_neighbors_resident, below)
 *
 * One call runs the whole neighbour loop: every neighbour's search, triangulation and gates in wide launches, then the only
 * order-dependent part (a feature that received a point from neighbour k is skipped for neighbour k + 1, ORBmatcher.cc:865) in
 * neighbour order.  The created points come back in the order the reference creates them; the map mutations (new MapPoint,
 * AddObservation, AddMapPoint, ComputeDistinctiveDescriptors, UpdateNormalAndDepth) stay with the caller, who owns the map.
 *
 * Monocular pinhole only: the views below carry no mvuRight, NLeft or second camera, so the stereo and two-camera branches
 * (LocalMapping.cc:457-504, 518-545, 576-585, 598-607) cannot be asked for; inertial is 0 (the 0.9998 parallax bound, :531).
 *
 * Parity.  Pairs, order, counts and skip flags are those of the reference's loop.  x3D is pinned to the oracle
 * (tests/cpp/newpoints_oracle.cc), not to Eigen::JacobiSVD: the null vector of Triangulate's 4x4 matrix A is defined as the
 * eigenvector of the smallest eigenvalue of A^T A by cyclic Jacobi rotations in double (6 sweeps, pairs (0,1) (0,2) (0,3) (1,2)
 * (1,3) (2,3); the smallest diagonal entry, the first one on ties), de-homogenised in double and cast to float.
 *
 * Status codes, error string and threading rules: rumi_orb.h.
 */
#ifndef RUMI_MAPPING_H
#define RUMI_MAPPING_H

#include <stdint.h>

#include "rumi_covis.h"
#include "rumi_match.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Neighbours of one call.  The reference asks GetBestCovisibilityKeyFrames for 30 in the monocular case (LocalMapping.cc:356-360) and the
 * inertial extension (:362-371) can append up to 30 predecessors (`vpNeighKFs.size() <= nn`, `count++ < nn`): 60 at most, rounded up to 64,
 * the size of the per-neighbour arrays in the result block. */
#define RUMI_NEWPTS_MAX_NEIGH 64
/* Features of the current key-frame (the replay kernel keeps one flag each in LDS); equal to the largest max_features rumi_match_create
 * accepts, so in practice the matcher's capacities are the limit. */
#define RUMI_NEWPTS_MAX_FEATURES 16384

/* What CreateNewMapPoints reads of a key-frame: host pointers and small matrices by value. */
typedef struct RumiNewPointsKF {
    RumiFrameFeatures feat;  /* mvKeysUn, mDescriptors, mvScaleFactors (mvLevelSigma2 = its squares); the bounds are not read */
    RumiFeatureVector fv;    /* mFeatVec: node ids strictly ascending (std::map order), every feature in at most one node; else RUMI_E_INVALID */
    const int32_t *kf_mp;    /* [feat.n] >= 0 where GetMapPoint(i) is not NULL */
    const float *mp_pos;     /* [feat.n][3] GetWorldPos() of feature i's map point, read only where kf_mp[i] >= 0.  Neighbours only
                                (the median depth); may be NULL for the current key-frame */
    float K4[4];             /* fx, fy, cx, cy */
    float Tcw[12];           /* GetPose().matrix3x4(), row-major (eigTcw) */
    float Ow[3];             /* GetCameraCenter() */
    float F12[9];            /* neighbours only: as rumi_search_for_triangulation takes it (current key-frame = 1, neighbour = 2) */
    float epipole2[2];       /* neighbours only: pKF2->mpCamera->project(T2w * Ow1) */
} RumiNewPointsKF;

typedef struct RumiNewPointsParams {
    int32_t coarse;             /* bCoarse of SearchForTriangulation (LocalMapping.cc:423) */
    int32_t check_orientation;  /* the matcher's mbCheckOrientation (the reference constructs it with false, :375) */
    int32_t far_points;         /* mbFarPoints */
    float th_far_points;        /* mThFarPoints (:619) */
    float ratio_factor;         /* 1.5f * mpCurrentKeyFrame->mfScaleFactor (:391) */
} RumiNewPointsParams;

typedef struct RumiNewPoint {
    int32_t neigh;   /* index into the neighbour list */
    int32_t idx1;    /* feature of the current key-frame */
    int32_t idx2;    /* feature of the neighbour */
    float x3D[3];
} RumiNewPoint;

/* LocalMapping::CreateNewMapPoints for one key-frame and its n_neigh neighbours (0 <= n_neigh <= RUMI_NEWPTS_MAX_NEIGH, each
 * key-frame listed once).  out [cap] receives the created points in creation order: neighbour order, then ascending idx1
 * (vMatchedIndices order); *n_out their number; per_neigh_out [n_neigh] the number per neighbour -- the results of neighbours
 * < i do not depend on later ones, so a caller that honours `if (i > 0 && CheckNewKeyFrames()) return;` applies a prefix;
 * neigh_skipped_out [n_neigh] = 1 where the baseline test skipped the neighbour (:414-418).
 * A neighbour none of whose features holds a map point: the reference indexes an empty vector there (KeyFrame.cc:977); this
 * entry takes the median depth as -1.0 (what ComputeSceneMedianDepth returns for N == 0), which skips the neighbour.
 * RUMI_E_CAPACITY: a key-frame has more features or FeatureVector entries than the matcher's max_features (the current one:
 * than max_queries as well, and than RUMI_NEWPTS_MAX_FEATURES), or cap < *n_out (then *n_out, per_neigh_out and neigh_skipped_out are valid and out holds the
 * first cap points).  A point list never needs more than cur->feat.n entries. */
int rumi_create_new_map_points(RumiMatcher *m, const RumiNewPointsKF *cur, const RumiNewPointsKF *neigh, int32_t n_neigh,
                               const RumiNewPointsParams *p, RumiNewPoint *out, int32_t cap, int32_t *n_out,
                               int32_t *per_neigh_out, uint8_t *neigh_skipped_out);

/* ---- The same member over key-frames that are resident in a covisibility store (rumi_covis.h): the caller names slots, and only what a
 * bundle adjustment changes travels per call. */
typedef struct RumiNewPointsPose {
    float Tcw[12], Ow[3];            /* as in RumiNewPointsKF */
    float F12[9], epipole2[2];       /* neighbours only, formed as for rumi_create_new_map_points */
} RumiNewPointsPose;

/* rumi_create_new_map_points with every key-frame read where the store keeps it: outputs and statuses are those of that entry on the same
 * data, byte for byte (the same kernels, instantiated over another view of the data).
 *   feat, fv, K4      the slot's features (rumi_covis_set_keyframe_features)
 *   kf_mp[i] >= 0     mp[i] >= 0 of the slot's map-point row, read in place
 *   mp_pos[i]         the position in point mp[i]'s attribute record (rumi_covis_set_point_attributes); neighbours only
 * Host to device per call: the store's staged edits and staged features, and a table of n_neigh + 1 pose records.
 * RUMI_E_INVALID, nothing written: a slot that is not live or holds no features; a slot named twice, cur_slot among the neighbours; a slot
 * whose feature count differs from the length of its map-point row; matcher and store on different devices; a neighbour entry >= 0 whose
 * point has no attributes (found on the device; the message names how many).  RUMI_E_CAPACITY as for rumi_create_new_map_points.
 * n_neigh == 0: RUMI_OK, *n_out = 0, no device call.  rumi_hook_newpts_matches does not replay a resident call (RUMI_E_INVALID). */
int rumi_create_new_map_points_resident(RumiMatcher *m, RumiCovis *c, int32_t cur_slot, const RumiNewPointsPose *cur_pose,
                                        const int32_t *neigh_slots, const RumiNewPointsPose *neigh_pose, int32_t n_neigh,
                                        const RumiNewPointsParams *p, RumiNewPoint *out, int32_t cap, int32_t *n_out,
                                        int32_t *per_neigh_out, uint8_t *neigh_skipped_out);

/* The last call of either entry on this matcher, in ms: validation + packing | upload, kernels, download | write-out. */
int rumi_newpts_stage_ms(const RumiMatcher *m, float *out3);

/* ---- The search half of LocalMapping::SearchInNeighbors (R/lib_src/LocalMapping.cc:649-743) for every target key-frame in one call, over
 * key-frames and points resident in a covisibility store.  ORBmatcher::Fuse (ORBmatcher.cc:1037-1174) first searches, then mutates; the index
 * it finds for a (key-frame, point) pair reads the point's position, normal, distance range and descriptor and the key-frame's pose,
 * key-points, descriptors, scale table and bounds.  Of these the member changes one before its final refresh (:730): MapPoint::Replace ends
 * with ComputeDistinctiveDescriptors() on the surviving point (MapPoint.cc:321).  The forward gates (NULL, isBad, IsInKeyFrame) only ever
 * close during the member, and every point the reverse pass searches stood in a target row at the call.  So the device answers both passes
 * from the store as it stands, and the caller replays AddObservation / AddMapPoint / Replace in the reference's order, re-evaluating each
 * gate when its turn comes.
 * WHAT THE CALLER MUST DO BESIDES: compare GetDescriptor() of the survivor before and after every Replace of the forward pass.  A point
 * of the current key-frame whose descriptor changed no longer has valid answers in fwd_best for the targets that follow: search it again
 * for each of them (rumi_fuse_candidates with the live descriptor) before its turn.  Without that the map can differ from the reference's.
 * The reverse answers need no second look: a forward survivor is in the current key-frame by then and is skipped, and a reverse survivor
 * has been searched already.  facade/LocalMappingStep.h SearchInNeighborsResident does all of this.  Monocular, non-inertial. */
#define RUMI_FUSE_MAX_TARGETS 640   /* 30 + 30 * 20 (LocalMapping.cc:651-677), rounded up */
typedef struct RumiFuseKF {   /* what a bundle adjustment changes, and what the store does not keep */
    float Tcw7[7];            /* as rumi_fuse_candidates takes it: qx qy qz qw tx ty tz of GetPose() */
    float Ow[3];              /* GetCameraCenter() */
    float bounds[4];          /* mnMinX, mnMinY, mnMaxX, mnMaxY */
    float log_scale_factor;   /* mfLogScaleFactor */
} RumiFuseKF;

/* fwd_best [n_targets][n_cur], n_cur = the length of cur_slot's map-point row (= its feature count): the feature of target t that the point
 * in entry i of that row fuses with: best_idx of rumi_fuse_candidates(..., check_reprojection = 1) on that target's features, pose and
 * bounds, K4 from the store, and that point's attributes, byte for byte.  -1 where the search finds none, where the entry is -1, where the
 * point is bad in the store, or where the point's observer row lists target_slots[t].
 * rev_point / rev_best [rev_cap]: one entry per distinct point that stands in some target's row, is not bad and does not list cur_slot: its
 * id and the feature of the current key-frame it fuses with (-1: none), in order of first occurrence with the targets walked in list order
 * and their rows in ascending feature order (what LocalMapping.cc:710-724 produces on the unmutated map).  *n_rev their number.  rev_cap <
 * *n_rev: RUMI_E_CAPACITY, fwd_best and *n_rev valid, the first rev_cap entries written.  The sum of the targets' feature counts always
 * suffices.
 * Host to device per call: the store's staged edits and staged features, and n_targets + 1 records of 60 bytes.  A query: the store is not
 * changed.  Integer atomics only: two calls on the same state return the same bytes.
 * RUMI_E_INVALID, nothing written: a missing argument; th <= 0; a pose, centre, bound or scale factor that is not finite, or empty bounds; a
 * slot that is not live or holds no features; a slot named twice, cur_slot among the targets; a slot whose feature count differs from the
 * length of its map-point row; matcher and store on different devices; a point that would be searched but has no attributes (found on the
 * device; the message names how many).  RUMI_E_CAPACITY, nothing written: n_targets > RUMI_FUSE_MAX_TARGETS; a key-frame above the matcher's
 * max_features.  n_targets == 0: RUMI_OK, *n_rev = 0, no device call. */
int rumi_search_in_neighbors_resident(RumiMatcher *m, RumiCovis *c, int32_t cur_slot, const RumiFuseKF *cur, const int32_t *target_slots,
                                      const RumiFuseKF *targets, int32_t n_targets, float th, int32_t *fwd_best, int32_t *rev_point,
                                      int32_t *rev_best, int32_t rev_cap, int32_t *n_rev);
/* The last call on this matcher, in ms: validation + table | upload, kernels, download | write-out. */
int rumi_search_in_neighbors_stage_ms(const RumiMatcher *m, float *out3);

/* ---- The searches of LoopClosing::SearchAndFuse (R/lib_src/LoopClosing.cc:1996-2065) for every corrected key-frame in one call, over
 * key-frames and points resident in a covisibility store.  The member calls ORBmatcher::Fuse(pKF, Scw, vpPoints, 4, vpReplacePoint)
 * (ORBmatcher.cc:1182-1291) once per key-frame: the search of a (key-frame, point) pair reads the point's position, normal, distance range
 * and descriptor and the key-frame's pose, key-points, descriptors, scale table and bounds; it has no reprojection gate.  AddObservation /
 * AddMapPoint happen inside Fuse, Replace after each key-frame (:2017-2023).  The gates (isBad, spAlreadyFound) only ever close during the
 * member, so the device answers every pair from the store as it stands and the caller replays the mutations key-frame by key-frame,
 * re-evaluating each gate and reading GetMapPoint(bestIdx) live at its turn.
 * WHAT THE CALLER MUST DO BESIDES: Replace ends with ComputeDistinctiveDescriptors() on the survivor, here always the loop point
 * (MapPoint.cc:321).  Compare its GetDescriptor() before and after; a loop point whose descriptor changed no longer has valid answers for the
 * key-frames that follow: search it again for each of them (rumi_fuse_candidates, check_reprojection = 0, live descriptor) before its turn.
 * facade/LoopClosingStep.h SearchAndFuseResident does all of this.  Monocular.
 *
 * kfs[k]: Tcw7 and Ow as ORBmatcher.cc:1190-1191 derives them from Scw -- SE3f(Scw.rotationMatrix(), Scw.translation() / Scw.scale()) and its
 * inverse's translation -- formed by the caller; no Sim3 arithmetic crosses this boundary.  bounds and log_scale_factor: the key-frame's own.
 * For key-frame k and list entry i the best feature is best_idx of rumi_fuse_candidates(..., check_reprojection = 0) on that key-frame's
 * resident features and K4, that pose, and the stored attributes of point_ids[i], byte for byte; -1 where point_ids[i] < 0, where the point is
 * bad in the store, where its observer row lists kf_slots[k], or where the search finds nothing within TH_LOW.  Duplicate ids are answered
 * independently.
 * hits [hit_cap]: only the pairs whose best feature is >= 0, in ascending (kf, point) order; kf and point index the call's lists, feature is
 * the best index, occupant the id in entry `feature` of that key-frame's map-point row at the call or -1 (a preview of GetMapPoint(bestIdx),
 * :1278; the caller re-reads the live object).  per_kf [n_kfs]: hits per key-frame; *n_hits their total.  hit_cap < *n_hits: RUMI_E_CAPACITY,
 * *n_hits and per_kf valid, the first hit_cap hits written.  The dense answer (n_kfs * n_points words) never leaves the device.
 * Host to device per call: the store's staged edits and staged features, n_kfs records of 60 bytes and 4 * n_points bytes of ids.  A query:
 * the store is not changed.  Integer atomics only: two calls on the same state return the same bytes.
 * RUMI_E_INVALID, nothing written: a missing argument; th <= 0; a pose, centre, bound or scale factor that is not finite, or empty bounds; a
 * slot that is not live or holds no features; a slot named twice; a slot whose feature count differs from the length of its map-point row;
 * matcher and store on different devices; an id at or above the store's point capacity; a list entry that would be searched and whose point
 * has no attributes (found on the device; the message names how many entries).  RUMI_E_CAPACITY, nothing written: n_kfs >
 * RUMI_FUSE_MAX_TARGETS; a key-frame above the matcher's max_features; n_kfs * n_points >= 2^31 (more pairs than a work item addresses).
 * n_kfs == 0 or n_points == 0: RUMI_OK, *n_hits = 0 (per_kf zeroed), no device call. */
typedef struct RumiFuseHit { int32_t kf, point, feature, occupant; } RumiFuseHit;
int rumi_search_and_fuse_resident(RumiMatcher *m, RumiCovis *c, const int32_t *kf_slots, const RumiFuseKF *kfs, int32_t n_kfs,
                                  const int32_t *point_ids, int32_t n_points, float th, RumiFuseHit *hits, int32_t hit_cap, int32_t *n_hits,
                                  int32_t *per_kf /* [n_kfs] */);
/* The last call on this matcher, in ms: validation + table | upload, kernels, download | write-out. */
int rumi_search_and_fuse_stage_ms(const RumiMatcher *m, float *out3);

/* ---- ORBmatcher::SearchByProjection(KeyFrame*, Sim3f&, points, ...) (R/lib_src/ORBmatcher.cc:372-471, :473-579) for every job of a
 * place-recognition stage in one call, over key-frames and points resident in a covisibility store.  The member is what
 * DetectCommonRegionsFromBoW / DetectCommonRegionsFromLastKF / DetectAndReffineSim3FromLastKF call between the Sim3 estimates
 * (LoopClosing.cc:716, :738, :773-795 through FindMatchesByProjection :868-914, :503-540; CloudMerging.cc has the same text).  A job is one
 * call of the member.  Inside a job the loop is sequential -- `vpMatched[bestIdx] = pMP` (:465, :573) hides the feature from every later
 * entry -- and the device reproduces exactly that order; jobs are independent of one another, also on the same slot.  Every call site hands
 * the member a fresh all-NULL vpMatched, so no feature is taken at entry; a caller that needs a pre-filled vector keeps
 * rumi_search_by_projection_sim3 (include/rumi_match.h).  Monocular.
 *
 * For job j and feature f, matched[matched_start[j] + f] is the POSITION inside job j's list of the point the loop leaves in vpMatched[f], or
 * -1; nmatches[j] the loop's return value: byte for byte what rumi_search_by_projection_sim3 returns for that key-frame's resident features
 * and K4, that pose, skip[i] = the point is bad in the store or the id is < 0, the stored attributes of the listed points and matched all -1.
 * A key-frame that already lists a point is NOT a gate (the member does not test it).  An id that appears twice in a list is two independent
 * entries in order, and both may match.  matched_start [n_jobs + 1]: the rows are concatenated, each the feature count of its job's slot.
 * Host to device per call: the store's staged edits and staged features, 128 bytes a job, 112 bytes a distinct slot and 4 bytes a list entry.
 * Device to host: 4 bytes a feature a job and 8 bytes a job, one blocking copy.  A query: the store is not changed.  Integer atomics only: two
 * calls on the same state return the same bytes.
 * RUMI_E_INVALID, nothing written: a missing argument; th <= 0, ratio_hamming not finite or <= 0; a pose, centre, bound or scale factor that
 * is not finite, or empty bounds; a slot that is not live or holds no features, or whose feature count differs from the length of its
 * map-point row; a list range outside [0, n_points]; an id at or above the store's point capacity; matcher and store on different devices; a
 * list entry that would be searched and whose point has no attributes (found on the device; the message names how many entries).
 * RUMI_E_CAPACITY, nothing written: n_jobs > RUMI_FUSE_MAX_TARGETS; a key-frame above the matcher's max_features; 2^31 or more (job, entry)
 * pairs (more than a work item addresses); matched_cap below the sum of the rows -- then, and only then, matched_start IS written, so that the
 * caller can size `matched` and call again.  n_jobs == 0, or every list empty: RUMI_OK, the rows all -1, the counts zero, no device call. */
typedef struct RumiSim3ProjJob {
    int32_t   kf_slot;                   /* key-frame searched; the same slot may appear in many jobs */
    RumiFuseKF kf;                       /* Tcw7 and Ow as ORBmatcher.cc:380-381 derive them from Scw (formed by the caller), bounds, mfLogScaleFactor */
    int32_t   point_start, point_count;  /* this job's list = point_ids[point_start .. +point_count); ranges of different jobs may coincide or overlap */
    int32_t   th;                        /* 8, 5, 3 upstream */
    float     ratio_hamming;             /* match iff bestDist <= TH_LOW * ratio_hamming, compared in float as :464 does */
    int32_t   explicit_invz;             /* 0 = :372-471 (mpCamera->project), 1 = :473-579 (u = fx * (x * (1/z)) + cx) */
} RumiSim3ProjJob;

int rumi_search_by_projection_sim3_resident(RumiMatcher *m, RumiCovis *c, const RumiSim3ProjJob *jobs, int32_t n_jobs,
                                            const int32_t *point_ids, int32_t n_points,
                                            int32_t *matched /* concatenated per job, feature count of its slot each */,
                                            int32_t *matched_start /* [n_jobs + 1] out */, int32_t matched_cap,
                                            int32_t *nmatches /* [n_jobs] */);
/* The last call on this matcher, in ms: validation + table | upload, kernels, download | write-out. */
int rumi_search_by_projection_sim3_stage_ms(const RumiMatcher *m, float *out3);
/* The rounds the ordered resolve of each job of the last call took (1: no entry lost a feature to an earlier one; 0 for every job of a call
 * that made no device call, whose stage times are 0 too).  n_jobs must be that call's. */
int rumi_search_by_projection_sim3_rounds(const RumiMatcher *m, int32_t *rounds, int32_t n_jobs);

/* ---- The BoW stage of LoopClosing::DetectCommonRegionsFromBoW (R/lib_src/LoopClosing.cc:576-651; CloudMerging.cc:1019-1094) by slot: what
 * rumi_common_regions_bow (include/rumi_match.h) answers from host pointers, answered from a covisibility store.  cur_slot is the current
 * key-frame; group g (one per BoW candidate) is member_slot[group_start[g] .. group_start[g + 1]), slots in vpCovKFi order.  A slot may appear
 * in several groups (and be the current key-frame's) and is read where it lies: key-points, descriptors and mFeatVec in its feature block,
 * its map points in its row, isBad() in the point records.  Both gates of ORBmatcher.cc:717-721 / :736-742 are read there -- row entry >= 0
 * and the point's bad bit clear, on the current side and on the member side -- so there is no cur_good and no mp_bad argument.
 *
 * Outputs, with n = the current slot's feature count, M = group_start[n_groups], G = n_groups: matches12 [M][n] (member feature index, -1),
 * nmatches [M], matched_point [G][n] (STORE point ids, -1), matched_member [G][n] (position j inside the group, -1), num_bow_matches [G],
 * most_matches [G][2] = (j, count), strictly greater so the first j wins a tie, (0, 0) when nothing matched.  Every array equals, byte for
 * byte, what rumi_common_regions_bow returns for the same key-frames, rows and bad bits by host pointers with the store's point ids as the
 * shared numbering.  matches12 may be NULL: the rows then stay on the device and are not copied back; the other five arrays do not change.
 * A member slot whose key-frame bad bit is set is named but not searched (as rumi_track_reloc_bow): its row is -1, its count -1, it takes no
 * part in the union or in most_matches, and the members behind it keep their j (the current slot's own bad bit is not read: the loop does
 * not ask it either).  A member FeatureVector node of any size is searched on the
 * device (the `taken` flags lie in LDS, sized by the largest member of the call): there is no host fallback.
 * Host to device per call: the store's staged edits and staged features, 24 bytes a member, 4 bytes a group.  Device to host: one blocking
 * copy of the counts and rows.  A query: the store is not changed.  Integer atomics only: two calls on the same state return the same bytes.
 * Memory the handle keeps for the union: a stamped table of 8 bytes x max_points x (the largest n_groups of any call so far), never cleared
 * between calls (a per-call epoch in the high word makes older stamps lose); clears per call are 4 bytes x (M x n + G x n + 33 M) and do not grow
 * with max_points.
 * RUMI_E_INVALID, before any device work, nothing written: a NULL handle, store or array (matches12 excepted); n_groups < 0; group_start not
 * ascending from 0; more than 65535 members; a slot outside the store or not live; the current slot or a member that is not bad without
 * features, or whose feature count differs from the length of its row; (largest group) x n above 2^31 - 1 (the union's key j * n + k);
 * matcher and store on different devices (the store is not bound first: neither handle makes a device call before this refusal, as in every
 * by-slot entry of this header).  RUMI_E_CAPACITY, likewise before any device work: a member above 65535 features; a union table above 2 GiB.
 * An empty group, n_groups == 0 and n == 0 are valid: rows -1, counts 0 (-1 for a bad member), most_matches (0, 0); with n == 0 or M == 0
 * there is no device call. */
int rumi_common_regions_bow_resident(RumiMatcher *m, RumiCovis *c, int32_t cur_slot, int32_t n_groups, const int32_t *group_start /* [n_groups + 1] */,
                                     const int32_t *member_slot /* [M] */, float nnratio, int32_t check_orientation,
                                     int32_t *matches12 /* [M][n], may be NULL */, int32_t *nmatches /* [M] */, int32_t *matched_point /* [G][n] */,
                                     int32_t *matched_member /* [G][n] */, int32_t *num_bow_matches /* [G] */, int32_t *most_matches /* [G][2] */);
/* The last call on this matcher, in ms: validation + table | store flush, upload, kernels, download | write-out (all 0 after a call
 * that made no device call). */
int rumi_common_regions_bow_resident_stage_ms(const RumiMatcher *m, float *out3);

/* ---- MapPoint::ComputeDistinctiveDescriptors (R/lib_src/MapPoint.cc:353-427) and MapPoint::UpdateNormalAndDepth (:450-518) for a batch of
 * points.  Neither member reads another MapPoint: a point's result depends on its own observation list, its position and reference
 * key-frame, and the observing key-frames' descriptors, camera centres, bad flags and scale tables.  So the per-point calls a map-changing
 * step ends with can be collected and issued as one call.  Monocular only: an observation carries a left index, so the right-camera branches
 * (:383-385, 484-489, 501-506) cannot be asked for.
 *
 * Descriptor (RUMI_REFRESH_DESCRIPTOR).  Observations whose key-frame is bad are dropped (:376); N = the rest, in the caller's order.
 * d[i][j] = Hamming distance of the 256-bit rows, d[i][i] = 0.  The median of row i is the element of rank (N-1)/2 of the ascending row,
 * its own zero included (`vDists[0.5*(N-1)]`, :414, truncates).  The winner is the first i whose median is strictly smaller than all
 * before it (:416).  best_obs is its position in the point's own observation list (the dropped entries count), best_median its median; both
 * are -1 where the reference returns without writing (:367, :389: no observation, or every observing key-frame bad).
 *
 * Normal and depth (RUMI_REFRESH_NORMAL_DEPTH).  Bad key-frames are NOT dropped here (:471-490 has no isBad test).
 * normal = sum over the list, in list order, of (Pos - Ow_i) / |Pos - Ow_i|, then divided by (float)n; dist = |Pos - Ow_ref|;
 * max_distance = dist * scale[ref_level] (:514); min_distance = max_distance / scale[nLevels - 1] (:515).  updated = 0 and nothing else
 * written where the reference returns early (:465, no observation).
 * Parity with `Eigen::Vector3f::norm()` unpinned: Eigen is not available to this project's oracle, so the float evaluation order is DEFINED
 * here and by tests/cpp/refresh_oracle.cc: differences per component, squared norm as (x*x + y*y) + z*z, IEEE sqrtf, true division per
 * component (no reciprocal), no FMA contraction, all in float.
 *
 * The order of a point's observations decides the tie between equal medians and the order of the float sums.  The reference iterates a
 * std::map<KeyFrame*, ...>, i.e. pointer order; the caller, who owns the pointers, supplies the pairs in that order. */
#define RUMI_REFRESH_DESCRIPTOR 1
#define RUMI_REFRESH_NORMAL_DEPTH 2
/* Observations of one point (the whole list, bad key-frames included).  The reference has no cap; a point above this one makes the call
 * return RUMI_E_CAPACITY with nothing written, never a truncated answer. */
#define RUMI_REFRESH_MAX_OBS 2048

/* What the two members read of a key-frame; each key-frame of the call once. */
typedef struct RumiRefreshKF {
    const uint8_t *desc;          /* mDescriptors, [n][32]; may be NULL without RUMI_REFRESH_DESCRIPTOR */
    int32_t n;                    /* N */
    int32_t nlevels;              /* mnScaleLevels */
    const float *scale_factors;   /* mvScaleFactors, [nlevels] */
    float Ow[3];                  /* GetCameraCenter() */
    uint8_t is_bad;               /* isBad() */
    uint8_t pad_[3];
} RumiRefreshKF;

typedef struct RumiRefreshPoint {
    float pos[3];                 /* GetWorldPos() */
    int32_t ref_kf;               /* GetReferenceKeyFrame(), index into the key-frame table */
    int32_t ref_feature;          /* the left index `observations[pRefKF]` yields (:495; 0 where the map has no such entry) */
    int32_t ref_level;            /* pRefKF->mvKeysUn[ref_feature].octave (:499) */
    int32_t obs_begin, obs_end;   /* the point's observations: entries obs_begin .. obs_end - 1 of obs_kf / obs_feature */
} RumiRefreshPoint;

typedef struct RumiRefresh RumiRefresh;

/* A handle owns the pinned upload block, the device blocks and the result block of its calls (grown on demand); not re-entrant, one per
 * calling thread.  device < 0: the current one.  Creation does not touch the device; the first call with work does. */
int rumi_refresh_create(int32_t device, RumiRefresh **out);
void rumi_refresh_destroy(RumiRefresh *r);

/* One batch.  kf [n_kf], pts [n_pts], obs_kf / obs_feature [n_obs] (key-frame index and feature index of every observation, the points'
 * slices in any order and possibly sharing entries).  `what` = RUMI_REFRESH_DESCRIPTOR | RUMI_REFRESH_NORMAL_DEPTH, at least one.
 * Outputs, one entry per point; the arrays of a mode that was not asked for are not touched and may be NULL:
 *   best_obs, best_median [n_pts]                         RUMI_REFRESH_DESCRIPTOR
 *   normal [n_pts][3], min_distance, max_distance, updated [n_pts]   RUMI_REFRESH_NORMAL_DEPTH
 * The library gathers the observed descriptor rows of good key-frames into its upload block: one block goes up, one comes back.
 * RUMI_E_INVALID, nothing written: a key-frame index outside the table, a feature index outside its key-frame, a slice outside
 * 0..n_obs, or -- for a point that has observations -- ref_kf outside the table, ref_feature outside the reference key-frame, ref_level
 * outside its scale table, nlevels < 1.  RUMI_E_CAPACITY, nothing written: a point with more than RUMI_REFRESH_MAX_OBS observations.
 * All of this is checked on the host before anything reaches the device.  n_pts = 0 is RUMI_OK.  No floating-point atomics: two calls
 * return the same bytes, and a point's result does not depend on its place in the batch. */
int rumi_refresh_map_points(RumiRefresh *r, const RumiRefreshKF *kf, int32_t n_kf, const RumiRefreshPoint *pts, int32_t n_pts,
                            const int32_t *obs_kf, const int32_t *obs_feature, int32_t n_obs, int32_t what, int32_t *best_obs,
                            int32_t *best_median, float *normal, float *min_distance, float *max_distance, uint8_t *updated);

/* The same two members over a covisibility store (rumi_covis.h): a list of point ids goes up and one 64-byte record a point comes back.
 * The outputs are those of rumi_refresh_map_points on the same map, byte for byte, with
 *   observation list of a point    its observer row, IN THE ORDER THE ROW IS STORED (rumi_covis_set_point_observations)
 *   is_bad of a key-frame          the slot's bit
 *   desc, n, nlevels, scale_factors   the slot's resident features (rumi_covis_set_keyframe_features)
 *   Ow                             the slot's centre (rumi_covis_set_keyframe_centres)
 *   pos                            the position in the point's attribute record (rumi_covis_set_point_attributes)
 *   ref_kf                         the point's reference slot (rumi_covis_set_point_reference)
 *   ref_feature                    the feature the row stores for that slot, 0 where the row does not list it (MapPoint.cc:495)
 *   ref_level                      the octave of that feature in the reference slot's resident key-points
 * The stored row order decides equal medians and the order of the float sums.  The reference iterates GetObservations(), a
 * std::map<KeyFrame*, ...>: pointer order.  facade/CovisibilityGraph::Sync(MapPoint*) stores the rows in that order; any other caller must too.
 * desc [n_pts][32]: the winning row's bytes, written where best_obs >= 0.  The point's own bad bit is not read (the members return for bad
 * points; the caller skips them).  Float rules as above; no floating-point atomics.
 *
 * flags = 0: a query, the store is unchanged.  RUMI_REFRESH_WRITE_BACK: when the call succeeds, each point's attribute record takes the
 * new descriptor where best_obs >= 0 and the new normal and distance range where updated, on the device and in the store's host mirror; the
 * position is untouched and no edit is staged.  rumi_track_local_map, rumi_search_in_neighbors_resident and
 * rumi_create_new_map_points_resident then read the new values without another upload.  Staged edits, these points' included, go up before
 * the kernels, so the write-back wins over an older staged value.
 *
 * RUMI_E_INVALID, nothing written (neither the outputs nor the store), on the host before any device call: a missing argument; an unknown
 * `what` or `flags` bit, or no mode; an id outside the store or named twice; the handle and the store on different devices (before any device work: neither is
 * bound first; a handle created with device < 0 learns its device by binding, which is then the only device work before this refusal); a point with
 * observers but without observation features; a point without attributes when RUMI_REFRESH_NORMAL_DEPTH or the write-back is asked for.
 * RUMI_E_INVALID, nothing written, counted on the device among what the call reads, the counts in the message (the store is legitimately
 * inconsistent between two staged edits, so the check is at the query): an observer slot without resident features (descriptor mode, good
 * observers); an observer feature outside its slot's feature count; an observer or reference slot without a centre (normal mode); for a point
 * with observers no reference slot, a reference slot without features, a reference octave outside its scale table (kept as a guard of the
 * kernel's table index: rumi_covis_set_keyframe_features refuses such key-points, so no caller of this ABI can meet it).
 * RUMI_E_CAPACITY, nothing written: a row above RUMI_REFRESH_MAX_OBS (known from the mirror).  n_pts = 0 is RUMI_OK and makes no device call.
 * A point with an empty row: best_obs = best_median = -1, updated = 0, nothing of it written back. */
#define RUMI_REFRESH_WRITE_BACK 1
struct RumiCovis;
int rumi_refresh_map_points_resident(RumiRefresh *r, struct RumiCovis *c, const int32_t *ids, int32_t n_pts, int32_t what, int32_t flags,
                                     int32_t *best_obs, int32_t *best_median, uint8_t *desc /*[n_pts][32]*/, float *normal, float *min_distance,
                                     float *max_distance, uint8_t *updated);

/* Host wall-clock of the handle's last successful call with work (either entry), in ms: out3[0] validation and gather, out3[1] upload +
 * kernels + download (the host waits for the device here), out3[2] writing the caller's arrays.  For tools/refresh_probe.py. */
int rumi_refresh_stage_ms(const RumiRefresh *r, float *out3);
/* Kernels the handle's last successful rumi_refresh_map_points_resident launched itself (the store's scatter of staged edits not counted). */
int32_t rumi_refresh_last_launches(const RumiRefresh *r);

/* ---- LocalMapping::KeyFrameCulling (R/lib_src/LocalMapping.cc:953-1079) and CloudKeyFrameCulling (:820-951) for the whole covisible list in
 * one call.  Non-inertial, monocular: the inertial branch (:1045-1070), the stereo depth gate (:1001-1004) and the NLeft != -1 octave
 * selection (:1008, :1020-1028) cannot be asked for -- the tables below carry no mPrevKF / mvDepth / right index.
 *
 * The loop takes the candidates in order.  `count` is incremented for every candidate, skipped ones included (:986).  A cloud candidate
 * (cloud variant only, :857), then the initial key-frame or a bad one (:989) is skipped by `continue`, which also skips the break test at the
 * loop's end.  For the others nMPs = the non-bad points of the key-frame (:1006); a point is redundant when Observations() > 3 (:1007) and
 * more than 3 OTHER observing key-frames see it at octave <= own octave + 1 (:1030-1037; the iteration order and the early break :1032 do
 * not change that).  The verdict is (float)nRedundant > 0.9f * (float)nMPs (:1044): one float multiply and one compare, no contraction.
 * After the verdict the loop breaks when count > 100, or count > 20 && abort_ba (:1075).
 *
 * A positive verdict calls KeyFrame::SetBadFlag() (:1072).  For a not_erase key-frame that only marks mbToBeErased (KeyFrame.cc:783):
 * status RUMI_CULL_TO_BE_ERASED, the map is unchanged and the key-frame is not bad.  Otherwise every point of the key-frame loses this
 * observation and nObs-- (MapPoint.cc:192-225); a point whose nObs is then <= 2 turns bad, drops all observations and leaves every
 * key-frame (MapPoint.cc:240-263).  So the state the loop carries is the set S of key-frames culled so far: a point's nObs is n_obs_count
 * minus its observers in S, it is bad when it was bad at the call or when it has an observer in S and that value is <= 2 (monotone), and the
 * observer count ignores observers in S.  A candidate listed twice is `skipped bad` the second time once culled.
 *
 * The map must be consistent, as KeyFrame::AddMapPoint / MapPoint::AddObservation keep it: mp[i] = p exactly when point p lists
 * (key-frame, i), and a point lists a key-frame at most once (its observations are a std::map).  MapPoint::SetBadFlag clears key-frame
 * slots BY INDEX (KeyFrame::EraseMapPointMatch(idx)), so with a dangling observation the result would depend on state outside S; such
 * tables are RUMI_E_INVALID, in both directions.
 *
 * abort_ba is sampled ONCE, at the call: the reference reads mbAbortBA anew at every candidate, from a flag another thread sets.  This is
 * the one deliberate difference. */
#define RUMI_CULL_CLOUD 1      /* flags: CloudKeyFrameCulling -- is_cloud candidates are skipped before anything else (:857) */
#define RUMI_CULL_ABORT_BA 2   /* flags: mbAbortBA */

#define RUMI_CULL_NOT_REACHED 0    /* the loop broke before this candidate */
#define RUMI_CULL_SKIPPED_CLOUD 1
#define RUMI_CULL_SKIPPED_INIT 2
#define RUMI_CULL_SKIPPED_BAD 3
#define RUMI_CULL_KEPT 4
#define RUMI_CULL_CULLED 5         /* SetBadFlag() went through: listed in culled[] */
#define RUMI_CULL_TO_BE_ERASED 6   /* positive verdict on a not_erase key-frame */

/* Key-frames of one call: the replay kernel keeps one bit each in LDS.  More is RUMI_E_CAPACITY. */
#define RUMI_CULL_MAX_KEYFRAMES 65536

/* Every key-frame that appears in an observation list, each once. */
typedef struct RumiCullKF {
    const int32_t *octave;   /* [n] mvKeysUn[i].octave, 0..127 */
    const int32_t *mp;       /* [n] GetMapPointMatches(): index into pts, -1 = NULL */
    int32_t n;
    uint8_t is_bad;          /* isBad() */
    uint8_t is_init;         /* mnId == GetMap()->GetInitKFid() */
    uint8_t not_erase;       /* mbNotErase */
    uint8_t is_cloud;        /* isCloud() */
} RumiCullKF;

typedef struct RumiCullPoint {
    int32_t obs_begin, obs_end;   /* entries obs_begin .. obs_end - 1 of obs_kf / obs_feature */
    int32_t n_obs_count;          /* Observations(): nObs, carried separately from the list length */
    uint8_t is_bad;               /* isBad() */
    uint8_t pad_[3];
} RumiCullPoint;

typedef struct RumiCull RumiCull;

/* A handle owns the pinned upload block, the device block and the result block of its calls (grown on demand); not re-entrant, one per
 * calling thread.  device < 0: the current one.  Creation does not touch the device; the first call with work does. */
int rumi_cull_create(int32_t device, RumiCull **out);
void rumi_cull_destroy(RumiCull *c);

/* One pass of the culling loop.  kfs [n_kf]; cand [n_cand] = GetVectorCovisibleKeyFrames() after UpdateBestCovisibles(), in its order, as
 * indices into kfs; pts [n_pts]; obs_kf / obs_feature [n_obs].  flags = RUMI_CULL_CLOUD | RUMI_CULL_ABORT_BA or 0.
 * Outputs: status, n_mps, n_redundant [n_cand] (the counts are 0 where the candidate was skipped or not reached); culled [n_cand] the
 * candidates (positions in cand) with status RUMI_CULL_CULLED in loop order, *n_culled their number.  Calling SetBadFlag() on them in that
 * order reproduces the reference's map; the RUMI_CULL_TO_BE_ERASED ones take SetBadFlag() too (it only sets mbToBeErased), at any time.
 * One pinned block goes up, one comes back.  Integer arithmetic but for the verdict; no floating-point atomics: two calls return the same
 * bytes, and the outputs do not depend on the order of pts or of the observations.
 * RUMI_E_INVALID, nothing written: an index outside its table (cand, mp, obs_kf, obs_feature), a slice outside 0..n_obs, an octave
 * outside 0..127, an mp[i] whose point does not list that (key-frame, feature) pair, an observation whose key-frame slot does not hold
 * the point, a point that lists a key-frame twice.  RUMI_E_CAPACITY, nothing written: a point above RUMI_REFRESH_MAX_OBS observations, or
 * n_kf above RUMI_CULL_MAX_KEYFRAMES.  All checked on the host before anything reaches the device.  n_cand = 0 is RUMI_OK (*n_culled = 0). */
int rumi_keyframe_culling(RumiCull *c, const RumiCullKF *kfs, int32_t n_kf, const int32_t *cand, int32_t n_cand, const RumiCullPoint *pts,
                          int32_t n_pts, const int32_t *obs_kf, const int32_t *obs_feature, int32_t n_obs, int32_t flags, int32_t *status,
                          int32_t *n_mps, int32_t *n_redundant, int32_t *culled, int32_t *n_culled);

/* The same loop over a covisibility store (rumi_covis.h): nothing of the map travels but the store's staged edits.  A candidate is a slot;
 * is_init, not_erase and is_cloud as in RumiCullKF.  isBad() of key-frames and points are the store's bits, a candidate's row is its map-point
 * row, Observations() the length of a point's observer row, and an observer's octave is keys[feature].octave of that slot's resident
 * features (rumi_covis_set_keyframe_features), with the feature index rumi_covis_set_point_observations stored.  Outputs and statuses are
 * those of rumi_keyframe_culling on the same map, byte for byte; the same kernels run over a view of the store.  A query: the store is not
 * changed.  The caller applies SetBadFlag() in the returned order and stages its edits for the next call.
 * RUMI_E_INVALID, nothing written: a missing argument or unknown flag; a candidate slot that is not live; a candidate that will be
 * evaluated and holds no features, or whose feature count differs from the length of its row; a point in such a row without observation
 * features (checked on the store's host mirror, with the count); the handle and the store on different devices (on the host, before either
 * binds: before any device work; a handle created with device < 0 learns its device by binding first); and, counted on the device
 * among the rows of the evaluated candidates, their points and those points' observers: an observer slot without resident features, an
 * observation (k, f) with f outside k's row or row_k[f] != p, a candidate slot i holding p where p does not list (candidate, i).  The check
 * happens at the query because the store is legitimately inconsistent between two staged edits.  RUMI_E_CAPACITY, nothing written: a point
 * of those rows above RUMI_REFRESH_MAX_OBS observers.  n_cand = 0 is RUMI_OK (*n_culled = 0) and makes no device call. */
typedef struct RumiCullCandidate { int32_t slot; uint8_t is_init, not_erase, is_cloud, pad_; } RumiCullCandidate;
int rumi_keyframe_culling_resident(RumiCull *h, RumiCovis *c, const RumiCullCandidate *cand, int32_t n_cand, int32_t flags, int32_t *status,
                                   int32_t *n_mps, int32_t *n_redundant, int32_t *culled, int32_t *n_culled);

/* Host wall-clock of the handle's last successful call with work (either entry), in ms: out3[0] validation and pack, out3[1] upload +
 * kernels + download, out3[2] writing the caller's arrays.  For tools/culling_probe.py. */
int rumi_cull_stage_ms(const RumiCull *c, float *out3);

#ifdef __cplusplus
}
#endif
#endif /* RUMI_MAPPING_H */
