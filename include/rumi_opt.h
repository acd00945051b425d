/*
 * rumi_opt.h — C ABI of the MI355X-native pose optimisation and local bundle adjustment (librumi_hip.so).
 *
 * Drop-in boundary for the two hot members of the all-static class ORB_SLAM3::Optimizer
 * (R/ = /root/reference/src/rumi-slam/, G/ = R/Thirdparty/g2o/g2o/):
 *   static int  PoseOptimization(Frame *pFrame)                                  R/include/cloud_edge_slam_lib/Optimizer.h:55, R/lib_src/Optimizer.cc:723-1001
 *   static void LocalBundleAdjustment(KeyFrame*, bool *pbStopFlag, Map*, int&x4) R/include/cloud_edge_slam_lib/Optimizer.h:53, R/lib_src/Optimizer.cc:1003-1355
 * and the g2o Levenberg-Marquardt / Huber / Schur machinery they run on (G/core/optimization_algorithm_levenberg.cpp:61-194,
 * G/core/block_solver.hpp:353-604, G/core/base_{unary,binary}_edge.hpp, G/core/robust_kernel_impl.cpp:78-91, G/types/se3quat.h).
 * The facade gathers the graph exactly as Optimizer.cc:763-897 / :1011-1271 do (under the same mutexes) and hands it over flat;
 * erasing observations and writing poses / points back (Optimizer.cc:1325-1354) stays in the facade under Map::mMutexMapUpdate.
 * Arithmetic is double precision on the device, float at both ends, as in the reference.  Results agree with the reference
 * algorithm to 1e-4 relative (the reference's own edge order is pointer-order dependent).
 *
 * Status codes, error string and threading rules: rumi_orb.h.
 */
#ifndef RUMI_OPT_H
#define RUMI_OPT_H

#include <stdint.h>

#include "rumi_orb.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct RumiOptimizer RumiOptimizer;

/* Scratch arenas: pose problems of up to max_pose_edges correspondences in total per call (all problems of a batch),
 * BA problems of up to max_kf key-frame vertices, max_mp points, max_edges observations.
 *
 * What a handle owns, in bytes (rumi_opt_footprint returns the two sums; every block has one owner, so the expressions are exact).
 * PE = max_pose_edges, PB = max_pose_batch, K = max_kf, M = max_mp, E = max_edges; r16(x), r256(x) = x rounded up to a multiple of 16, 256;
 * NP = min(r16(6 K + 1), 256), the padded width of the dense Schur panel.  Integer arithmetic throughout ("/" rounds down).
 *   pose blocks          device  34 PE + 64 PB + 532          transfer blocks in and out, active flags 1, last chi2 8 per correspondence
 *                        pinned  25 PE + 64 PB + 532          the two transfer blocks
 *   window part  W       device  233 E + 232 M + 672 K + 2560 one window's state as the window-batched kernels use it: two transfer blocks
 *                                                             of S = 48 E + 32 M + 80 K + 1024 each, pose panel rows 128 E, chi2 8 E, level
 *                                                             flags E; per point D^-1, b_l, two states, update; per key-frame two states,
 *                                                             H_pp, b_p, update
 *                        pinned  S + 64                       the upload block and the stop word
 *   host-loop part  H    device  144 E + (120 + 24 NP) M + 8 NP^2 + 8 (6 K + 2)^2 + 96 K + 64
 *                                                             what only the single-window LM loop driven from the host reads: H_pl 144 E; H_ll, L
 *                                                             and the panel Y (24 NP M: 6 KiB a point once NP = 256, from K = 40 on); its
 *                                                             Gram matrix; the dense reduced system of the large-window path (85 MB at
 *                                                             K = 544); the trial's scalars
 *                        pinned  128                          the published scalars
 *   batch extras  X      device  26088000 + 16 max(192, (M + 31) / 32) + 2 r256(4 M + 4) + 6 r256(4 E) + r256(8 E) + r256(E)
 *                                + r256(128 (M / 16 + 2))     Gram partials of the tile solver (26 MB whatever the sizes), chi2 / scale
 *                                                             partials, the graph sorted by landmark, LM control
 *                        pinned  24                           the word a window reports through
 *   runner  R            device  15616 + 32 r256(r16(r16(r16(64 K) + 24 M) + E) + 16)
 *                        pinned  the same                     what a chain of launches needs: the window table of a launch group (32 x 488)
 *                                                             and the block its results come back in, sized for 32 windows of K, M, E;
 *                                                             a stream and two events
 * rumi_opt_create allocates the pose blocks, W + H (the handle's own window) and R; nothing else.
 * First use, kept until rumi_opt_destroy:
 *   rumi_local_ba / rumi_merge_ba / rumi_bundle_adjustment: X, the first time a window of up to 29 optimised key-frames (and at most 512
 *     key-frames, handle not profiled) runs; 148 E and the co-observation pair lists of the largest window seen (growing by a quarter), the first
 *     time a window of more than 42 optimised key-frames runs.
 *   rumi_local_ba_resident: what the assembly of a window needs beyond W, growing with the store and the window: 8 bytes a point id of the
 *     store (first-occurrence stamps), 20 E (observer word, point id and erase list per edge), the lists and counts of one call (4 bytes a
 *     feature of the local rows, 16 a slot), and two small transfer blocks; the solve then takes X, or H's blocks, as rumi_local_ba does.
 *   rumi_essential_graph / rumi_sim3_correct_points: the dense matrix and one block for the rest, by problem size.
 *   rumi_local_ba_batch with n such small windows: batch arenas A = W + X, one per window of a launch wave: min(n, 32) of them (X when a
 *     window is first staged in the arena; a window that ends before staging leaves it at W); batch runners R: one per launch group after the
 *     first, which the handle's own runner drives: none below 8 windows in a wave, 1 from 8, 2 from 12 (RUMI_BAW_GROUPS = g: g - 1, at most 3).
 *     Every other window of the batch (30 or more optimised key-frames, more than 512 key-frames, a profiled handle) runs in a worker context
 *     W + H + R, one per worker thread: min(n_workers, number of such windows, 16) of them; a worker context takes X and the large-window
 *     blocks as the handle's own window does.
 * A later call with no more windows of either kind than an earlier one allocates nothing. */
int rumi_opt_create(int32_t max_pose_edges, int32_t max_pose_batch, int32_t max_kf, int32_t max_mp, int32_t max_edges,
                    int32_t device, RumiOptimizer **out);
void rumi_opt_destroy(RumiOptimizer *o);

/* Optimizer::PoseOptimization.  One entry per feature of the frame that holds a map point, in feature order:
 * Xw n x 3 (MapPoint::GetWorldPos), obs n x 2 (mvKeysUn[i].pt), inv_sigma2 n (mvInvLevelSigma2[octave]); K4 = fx,fy,cx,cy;
 * Tcw7 in/out = pFrame->GetPose() / SetPose() as (qx,qy,qz,qw,tx,ty,tz); outlier_out n (mvbOutlier).
 * *n_good_out = the reference's return value nInitialCorrespondences - nBad (0, pose untouched, when n < 3). */
int rumi_pose_optimization(RumiOptimizer *o, const float *Xw, const float *obs, const float *inv_sigma2, int32_t n,
                           const float *K4, float *Tcw7, uint8_t *outlier_out, int32_t *n_good_out);

/* The same for B independent frames in one launch (one workgroup per frame).  Problem b owns entries
 * [start[b], start[b+1]) of Xw / obs / inv_sigma2 / outlier_out; Tcw7 is B x 7, n_good_out is B. */
int rumi_pose_optimization_batch(RumiOptimizer *o, int32_t nbatch, const int32_t *start, const float *Xw, const float *obs,
                                 const float *inv_sigma2, const float *K4, float *Tcw7, uint8_t *outlier_out,
                                 int32_t *n_good_out);

/* Optimizer::LocalBundleAdjustment on the flattened graph:
 *   kf_pose7  nKF x 7 in/out  key-frame poses Tcw (local key-frames first or in any order); fixed ones are not written
 *   kf_fixed  nKF             1 = fixed vertex (lFixedCameras, or the map's initial key-frame)
 *   mp_pos3   nMP x 3 in/out  map point positions
 *   edges     nE: e_mp / e_kf indices, e_obs nE x 2 (mvKeysUn pt), e_inv_sigma2 nE     (grouped by map point, as the
 *             reference builds them; any order is accepted)
 *   stop_flag the reference's pbStopFlag (host memory written by another thread; polled between LM trials; may be NULL)
 *   erase_out nE: 1 where the reference would erase the observation (chi2 > 5.991 or depth <= 0, Optimizer.cc:1285-1297)
 *   stats[4]: LM iterations run, LM trials run, number of optimised key-frames, 1 if aborted by the stop flag before start.
 * Returns RUMI_E_INVALID when there is no fixed key-frame (the reference returns silently, Optimizer.cc:1057-1060). */
int rumi_local_ba(RumiOptimizer *o, int32_t nKF, float *kf_pose7, const uint8_t *kf_fixed, int32_t nMP, float *mp_pos3,
                  int32_t nE, const int32_t *e_mp, const int32_t *e_kf, const float *e_obs, const float *e_inv_sigma2,
                  const float *K4, const volatile uint8_t *stop_flag, uint8_t *erase_out, int32_t *stats);

/* Optimizer::LocalBundleAdjustment with the window assembled on the device from the covisibility store (rumi_covis.h): the host names slots,
 * nothing of the graph is uploaded.  For the same map state every output is, byte for byte, what rumi_local_ba returns on the graph that
 * Optimizer.cc:1003-1271 builds (monocular branch).
 *   cur_slot     pKF; K4 is its fx fy cx cy (rumi_covis_set_keyframe_features)
 *   neigh_slots  pKF->GetVectorCovisibleKeyFrames() as slots, unfiltered and in that order (live, distinct, never cur_slot)
 *   init_slot    pMap->GetInitKFid() as a slot, -1 none
 * Read in the store: map-point rows, bad bits and maps of key-frames and points (rumi_covis_set_point_maps), observer rows with feature indices
 * (rumi_covis_set_point_observations), order_key (the order of std::map<KeyFrame*, ..>), key-points, scale factors, poses
 * (rumi_covis_set_keyframe_poses) and positions (rumi_covis_set_point_attributes).
 * out: the caller sets the capacities and the pointers; the call writes
 *   kf_slots [n_kf]        lLocalKeyFrames (num_OptKF of them, the current slot first), then lFixedCameras in order of first appearance
 *   kf_pose7 [num_OptKF]   the new poses of the local key-frames (the initial key-frame keeps the floats it was set with)
 *   mp_ids, mp_pos3 [num_MPs]   lLocalMapPoints and their new positions
 *   erased [n_erased][3]   {key-frame slot, point id, feature} of the observations to erase, in edge order (Optimizer.cc:1285-1297)
 *   num_fixedKF            lFixedCameras, plus one when init_slot is local;  num_edges;  stats[4] as rumi_local_ba
 * Refused with RUMI_E_INVALID, counts from the device's check in the message, store and out untouched: a live point of a local row that was
 * never given a map; an observation whose (slot, feature) disagrees with the slot's row; a key-frame of the window without pose or features;
 * a listed point without attributes or observation features.  No fixed key-frame: RUMI_E_INVALID and rumi_local_ba's message.  Stop flag
 * raised: stats[3] = 1, nothing else written.  RUMI_E_CAPACITY when a list does not fit out or the handle's arenas.
 * One small block (counts and the key-frame list) is read back between assembly and solve.  A window the tile solver takes (at most 29
 * optimised and 512 key-frames, handle not profiled) is solved from where the fill kernels left it; any other window is assembled on the
 * device all the same, read back once and handed to the single-window host loop as rumi_local_ba does.
 * After a run that was not aborted the store takes the results: positions into the attribute records (device and mirror), the new poses as
 * rumi_covis_set_keyframe_poses of kf_pose7 would leave them (staged).  Camera centres stay the caller's rumi_covis_set_keyframe_centres. */
typedef struct RumiLbaResidentOut {
    int32_t kf_cap, mp_cap, erase_cap;             /* in: capacities of the arrays below, in entries */
    int32_t *kf_slots; float *kf_pose7;            /* [kf_cap], [kf_cap][7] */
    int32_t *mp_ids; float *mp_pos3;               /* [mp_cap], [mp_cap][3] */
    int32_t *erased;                               /* [erase_cap][3] */
    int32_t n_kf, num_OptKF, num_fixedKF, num_MPs, num_edges, n_erased;
    int32_t stats[4];
} RumiLbaResidentOut;
struct RumiCovis;
int rumi_local_ba_resident(RumiOptimizer *o, struct RumiCovis *c, int32_t cur_slot, const int32_t *neigh_slots, int32_t n_neigh, int32_t init_slot,
                           const volatile uint8_t *stop_flag, RumiLbaResidentOut *out);

/* R independent windows of Optimizer::LocalBundleAdjustment (Optimizer.cc:1003-1355) in one call.  A window does not shard over GPUs or
 * workgroups ("replicas only"), but windows are independent.  Windows of up to 29 optimised key-frames are a batch
 * dimension of the kernels: the calling thread drives all of them, each in a batch arena of the handle.  The others run one by one in worker
 * contexts on n_workers host threads that take them from a shared counter, so the kernels of one window run while another window's thread
 * waits for the scalars of its LM trial.  What the handle allocates for either kind: the paragraph above rumi_opt_create.  Per window: the
 * arguments of rumi_local_ba, stats[4] and the status of its own run.  Returns the worst status. */
typedef struct RumiBaWindow {
    int32_t n_kf; float *kf_pose7; const uint8_t *kf_fixed;
    int32_t n_mp; float *mp_pos3;
    int32_t n_edges; const int32_t *e_mp, *e_kf; const float *e_obs, *e_inv_sigma2;
    const float *K4;
    const volatile uint8_t *stop_flag;
    uint8_t *erase_out;
    int32_t stats[4];
    int32_t status;
} RumiBaWindow;
int rumi_local_ba_batch(RumiOptimizer *o, int32_t n_windows, RumiBaWindow *windows, int32_t n_workers);

/* Optimizer::LocalBundleAdjustment(KeyFrame *pMainKF, vector<KeyFrame*> vpAdjustKF, vector<KeyFrame*> vpFixedKF, bool *pbStopFlag)
 * — the merge / welding-window bundle adjustment, R/lib_src/Optimizer.cc:3768-4183 (LoopClosing::MergeLocal, CloudMerging),
 * monocular edges.  Same flattened graph and the same outputs as rumi_local_ba; what differs is the procedure: optimize(5) with
 * Huber(sqrt(5.99)), then — unless *stop_flag — edges with chi2 > 5.991 or non-positive depth leave the optimisation (level 1),
 * the robust kernels are removed and optimize(10) runs again (:3986-4031); erase_out is the final test of :4042-4056.  A graph
 * without fixed key-frames is accepted, as upstream.  stats = {iterations of the first optimize, LM trials in total, optimised
 * key-frames, iterations of the second optimize}. */
int rumi_merge_ba(RumiOptimizer *o, int32_t nKF, float *kf_pose7, const uint8_t *kf_fixed, int32_t nMP, float *mp_pos3,
                  int32_t nE, const int32_t *e_mp, const int32_t *e_kf, const float *e_obs, const float *e_inv_sigma2,
                  const float *K4, const volatile uint8_t *stop_flag, uint8_t *erase_out, int32_t *stats);

/* Device time of the last rumi_local_ba call by stage, in ms (HIP events):
 * [0] linearise+Hll/Hpl, [1] pose block J^T W J on f64 MFMA, [2] Schur complement, [3] reduced solve, [4] update+chi2, [5] total */
int rumi_opt_stage_ms(RumiOptimizer *o, float ms[8]);
/* Opt-in per-kernel timing of the bundle adjustment: with profiling on, the next rumi_local_ba / rumi_merge_ba / rumi_bundle_adjustment call on
 * the dense-panel path records HIP events around the pose-block Gram product (f64 MFMA), the Schur-complement SYRK (f64 MFMA) and the
 * reduced solve of every LM trial; rumi_opt_kernel_ms returns their sums in ms and the trial count: [0] hpp, [1] syrk, [2] solve, [3] trials. */
int rumi_opt_set_profiling(RumiOptimizer *o, int32_t on);
int rumi_opt_kernel_ms(RumiOptimizer *o, float ms[4]);

/* out2 = {device bytes, pinned host bytes} the handle owns right now: the sum of the capacities of its blocks, batch arenas, batch runners
 * and worker contexts included (the expressions above rumi_opt_create). */
int rumi_opt_footprint(const RumiOptimizer *o, int64_t out2[2]);

/* Optimizer::BundleAdjustment(vpKFs, vpMP, nIterations, pbStopFlag, nLoopKF, bRobust) — R/lib_src/Optimizer.cc:54-351, monocular edges: the
 * full BA behind GlobalBundleAdjustemnt (map initialisation, Tracking.cc CreateInitialMapMonocular: 2 key-frames, 20 iterations; loop /
 * merge correction).  Same flattened graph as rumi_local_ba (kf_fixed[k] = the key-frame is the map's first one, :116); one
 * optimize(n_iterations) with Huber(sqrt(5.99)) when robust.  Landmarks without an edge keep their position (:248-250).  As for the
 * other BA entry points, up to 42 optimised key-frames take the dense-panel path; larger windows (up to 2560 optimised key-frames, within
 * the handle's max_kf) accumulate the Schur complement block-sparsely and factor it with a multi-workgroup blocked Cholesky.
 * stats = {LM iterations, LM trials, optimised key-frames, 0}. */
int rumi_bundle_adjustment(RumiOptimizer *o, int32_t nKF, float *kf_pose7, const uint8_t *kf_fixed, int32_t nMP, float *mp_pos3, int32_t nE,
                           const int32_t *e_mp, const int32_t *e_kf, const float *e_obs, const float *e_inv_sigma2, const float *K4,
                           const volatile uint8_t *stop_flag, int32_t n_iterations, int32_t robust, int32_t *stats);

/* Sim3Solver::ComputeInliersNum(map1KFs, map2KFs, avpValidKPMatches, gSw1w2) — R/lib_src/Sim3Solver.cc:564-664, the alignment score of
 * the rumination sub-map merge (CloudMerging.cc:611,748,809).  One entry per matched key-point pair, concatenated over the key-frame
 * pairs (pair_start [n_pairs + 1]); per pair the two composed transforms gSc1w2 = gSc1w1 * gSw1w2 and gSc2w1 = gSc2w2 * gSw1w2^-1 as
 * (qx qy qz qw tx ty tz s) doubles, formed by the caller with g2o::Sim3 itself (:620-621); per match the two map points' world
 * positions, the two key-points (mvKeys), mvLevelSigma2 at their octaves and the points' isEdge flags.  pair_denominator[p] =
 * vpValidKPMatches.size() (matches skipped for NULL map points still count, :644).  Outputs: inlier flag per match, ratio per pair,
 * and the returned value: the sorted ratios' element [n/2]. */
int rumi_sim3_inliers(RumiOptimizer *o, int32_t n_pairs, const int32_t *pair_start, const int32_t *pair_denominator, const double *S_c1w2,
                      const double *S_c2w1, const float *K4_1, const float *K4_2, const float *X1, const float *X2, const float *kp1,
                      const float *kp2, const float *sigma2_1, const float *sigma2_2, const uint8_t *edge1, const uint8_t *edge2,
                      uint8_t *inlier_out, float *ratio_out, float *median_out);

/* The alignment-score data of Sim3Solver::ComputeInliersNum (see rumi_sim3_inliers) for the hypotheses of rumi_sim3_ransac: instead of the
 * composed transforms the caller passes g2o::Sim3(R, t, 1.0) of the two key-frames of every pair (Sim3Solver.cc:596-597) and of the solver's
 * own key-frames mpKF1 / mpKF2 (:342-343), as (qx qy qz qw tx ty tz s) doubles; the composition with every hypothesis happens on the device. */
typedef struct RumiSim3ScoreSet {
    int32_t n_pairs;
    const int32_t *pair_start, *pair_denominator;
    const double *S_c1w1, *S_c2w2;
    const double *S_kf1w, *S_kf2w;
    const float *K4_1, *K4_2, *X1, *X2, *kp1, *kp2, *sigma2_1, *sigma2_2;
    const uint8_t *edge1, *edge2;
} RumiSim3ScoreSet;

/* Sim3Solver::iterate — R/lib_src/Sim3Solver.cc:159-220, :222-290 and the rumination overload :292-404 (CloudMerging.cc:717): the hypotheses of one
 * block of RANSAC iterations evaluated together, one workgroup each.  The n correspondences are those the constructor keeps (:78-126): both points in
 * their own camera frames (mvX3Dc1 / mvX3Dc2) and mvLevelSigma2 at the two key-points' octaves (mvnMaxError = 9.210 * sigma2, truncated to
 * size_t as upstream's vector<size_t> does; mvP1im1 / mvP2im2 are re-projected on the device, :128-129).  triples[3h..3h+2] = the minimal set of
 * hypothesis h, drawn by the caller exactly as :181-191 (DUtils::Random::RandomInt over the shrinking vAvailableIndices) — the draws do not depend on
 * earlier results, so a block of iterations is data-parallel and the caller replays the sequential "best so far / converged" logic of :198-214,
 * :277-283 or :349-373 over the per-hypothesis outputs (rumi_slam_amd.sim3solver.Sim3Solver, facade/Sim3Solver.h).
 * Per hypothesis: ComputeSim3 (:437-540, Horn 1987) and CheckInliers (:542-562); with score != NULL also ComputeInliersNum (:564-664) under
 * gSw1w2 = gSc1w^-1 * gSc1c2 * gSc2w (:338-347).  T12_out[h] = {mR12i row-major (9), mt12i (3), ms12i, valid, 0, 0}: valid = 0 marks the
 * degenerate set on which upstream returns early and keeps the previous iteration's transform (:493-494); n_inliers_out[h] = mnInliersi;
 * inlier_out [n_hyp][n] (may be NULL) = mvbInliersi; ratio_out [n_hyp][n_pairs] (may be NULL), median_out [n_hyp] = the returned ratio.
 * Upstream solves the 4x4 eigen-problem with Eigen::EigenSolver<Matrix4f> (not in the tree); here: Jacobi rotations in double on the same
 * float matrix — the transforms agree to float rounding, not bit for bit ("parity unpinned"). */
int rumi_sim3_ransac(RumiOptimizer *o, int32_t n, const float *X3Dc1, const float *X3Dc2, const float *sigma2_1, const float *sigma2_2,
                     const float *K4_1, const float *K4_2, int32_t fix_scale, int32_t n_hyp, const int32_t *triples, const RumiSim3ScoreSet *score,
                     float *T12_out, int32_t *n_inliers_out, uint8_t *inlier_out, float *ratio_out, float *median_out);

/* Optimizer::OptimizeSim3(pKF1, pKF2, vpMatches1, g2oS12, th2, bFixScale, mAcumHessian, bAllPoints) — R/lib_src/Optimizer.cc:1920-2167
 * (LoopClosing.cc:522,728, CloudMerging.cc:965,1169) and Optimizer::OptimizeCloudSim3(map1KFs, map2KFs, avpMatches, gSw1w2, th2, bFixScale,
 * mAcumHessian, bAllPoints) — :2169-2471 (CloudMerging.cc:803): Levenberg-Marquardt over ONE Sim3 vertex with numeric Jacobians,
 * optimize(5), removal of the correspondences whose edges exceed th2, optimize(10 or 5) without robust kernel, final inlier count.
 * One entry per correspondence that reaches "nCorrespondences++" (:2035 / :2316; the caller applies the map-point / isBad / i2 /
 * depth filters before): both points in their own camera frames (P3D1c, P3D2c as float, :1986-1998), the two observations (obs1 =
 * mvKeysUn of key-frame 1; obs2 = mvKeysUn of key-frame 2 or the float-normalised projection of :2065-2071, :2354-2360), mvInvLevelSigma2 at the two
 * octaves, skip12 / skip21 = the edge is not created (pMP2->isEdge / pMP1->isEdge, :2323,:2366; NULL = none).
 * S_c1w == NULL selects EdgeSim3ProjectXYZ / EdgeInverseSim3ProjectXYZ (OptimizeSim3: the vertex maps camera 2 into camera 1); otherwise
 * the world edges of OptimizeCloudSim3 with per key-frame-pair g2o::Sim3(R, t, 1.0) of both key-frames (:2231-2232) as
 * (qx qy qz qw tx ty tz s) doubles formed by the caller, and pair_of[i] = key-frame pair of correspondence i.
 * robust_first_pass: Huber(sqrt(th2)) on the first optimize (OptimizeSim3 :2050-2052; OptimizeCloudSim3 passes none, :2335,:2378).
 * S_io8: vertex estimate in / out (on the early return it holds the estimate after the first optimize, which OptimizeCloudSim3 has
 * already published at :2397 and OptimizeSim3 discards).  status_out[i]: 0 inlier, 1 removed after the first optimize, 2 fails the final
 * test, 3 kept but uncounted (one of its edges absent).  result3 = {nIn, nBad, 1 if "nCorrespondences - nBad < 10" returned early}.
 * mAcumHessian is zeroed by the reference and never accumulated (:2144, :2446): the facade does the same. */
int rumi_optimize_sim3(RumiOptimizer *o, int32_t n, const int32_t *pair_of, int32_t n_pairs, const double *S_c1w, const double *S_c2w,
                       const float *P1c, const float *P2c, const float *obs1, const float *obs2, const float *inv_sigma2_1,
                       const float *inv_sigma2_2, const uint8_t *skip12, const uint8_t *skip21, const float *K4_1, const float *K4_2, float th2,
                       int32_t fix_scale, int32_t robust_first_pass, double *S_io8, uint8_t *status_out, int32_t *result3);

/* Sim3Solver::iterate(nIterations, bNoMore, vbInliers, nInliers, bConverge) — R/lib_src/Sim3Solver.cc:222-290 — of the J solvers that
 * DetectCommonRegionsFromBoW runs one after the other (LoopClosing.cc:655-676, CloudMerging.cc:1019 ff.), in one call.  The solvers share the
 * process-wide rand() and every iteration consumes exactly three draws (:249-259), so iteration g of the stream uses the same three numbers
 * whichever solver runs it; only the mapping to indices depends on the solver's N.  The caller takes a window of `window` iterations of the
 * stream and draws it once per solver with that solver's N: triples [J][window][3], indices relative to the solver's `first`.  The device
 * evaluates every (solver, iteration) — ComputeSim3 and CheckInliers exactly as rumi_sim3_ransac — and then applies the sequential rule in
 * solver order with pos = 0: solver j returns at the first h in [pos, min(pos + its_left, window)) that is valid and has more than min_inliers
 * inliers (upstream's ">= mnBestInliers" cannot fail there: an earlier iteration with as many would itself have returned; a degenerate set
 * keeps the previous, non-returning, count).
 *   RUMI_SIM3_CONVERGED     its = h - pos + 1, pos <- h + 1; hyp = h, n_inliers, T12 = that iteration's T12_out record, mask in inlier_out
 *   RUMI_SIM3_EXHAUSTED     no such h and pos + its_left <= window: its = its_left (the solver's bNoMore), pos <- pos + its_left
 *   RUMI_SIM3_WINDOW_ENDED  no such h and pos + its_left > window: its = window - pos; every later solver is RUMI_SIM3_NOT_REACHED, its = 0
 * The caller advances rand() by 3 * (sum of its) and calls again with what is left (rumi_slam_amd.sim3solver.Sim3SolverBatch,
 * facade/PlaceRecognitionStages.h).  Solvers with fewer correspondences than min_inliers draw nothing upstream (:228-231) and are not sent.
 * Correspondences are concatenated over the solvers (n_total entries; the ranges [first, first + n) ascend without overlap); K4_1 / K4_2 are
 * {fx fy cx cy} of the two key-frames.  inlier_out [n_total]: the mask of a converged solver in its range, 0 elsewhere.  n_inliers_all
 * [J][window] and T12_all [J][window][16] (both may be NULL): every hypothesis as rumi_sim3_ransac returns it for that solver and triple,
 * byte for byte.  RUMI_E_INVALID (n < 3, a triple index outside [0, n), its_left < 1, window < 1, ranges out of order) and RUMI_E_CAPACITY
 * (the staging does not fit the handle's arena) leave every output untouched. */
enum { RUMI_SIM3_NOT_REACHED = 0, RUMI_SIM3_CONVERGED = 1, RUMI_SIM3_EXHAUSTED = 2, RUMI_SIM3_WINDOW_ENDED = 3 };
typedef struct RumiSim3RansacSolver {
    int32_t first, n;            /* the solver's correspondences in the concatenated arrays, n >= 3 */
    int32_t min_inliers;         /* mRansacMinInliers */
    int32_t its_left;            /* mRansacMaxIts - mnIterations, >= 1 */
    int32_t fix_scale;
    float K4_1[4], K4_2[4];
} RumiSim3RansacSolver;
typedef struct RumiSim3RansacResult {
    int32_t state, its, hyp, n_inliers;
    float T12[16];
} RumiSim3RansacResult;
int rumi_sim3_ransac_batch(RumiOptimizer *o, int32_t n_solvers, const RumiSim3RansacSolver *solvers, int32_t n_total, const float *X3Dc1,
                           const float *X3Dc2, const float *sigma2_1, const float *sigma2_2, int32_t window, const int32_t *triples,
                           RumiSim3RansacResult *results, uint8_t *inlier_out, int32_t *n_inliers_all, float *T12_all);

/* CloudMerging::ComputeSubmapSim3 -- R/lib_src/CloudMerging.cc:434-825 -- as a session over one resident score set: the set of
 * Sim3Solver::ComputeInliersNum does not change during the function, so it is uploaded once (begin), scored for given transforms (score, :611, :748,
 * :809) and used by the whole RANSAC loop of :643-741 in one call (ransac).  The session lives in the handle; its blocks grow on demand.
 *   begin   validates as rumi_sim3_ransac does (n_pairs >= 1, ascending pair_start, non-NULL arrays when total > 0) and uploads the set; S_kf1w /
 *           S_kf2w of the set are not read (every solver brings its own).  A second begin replaces the set, end drops it; every other entry
 *           without a set returns RUMI_E_INVALID.  total == 0 and pairs with pair_denominator == 0 are legal: their ratios are 0 (Sim3Solver.cc:644-647).
 *   score   ComputeInliersNum for n_S transforms: S_c1w2 / S_c2w1 [n_S][n_pairs][8] are the composed transforms the caller forms as for
 *           rumi_sim3_inliers; per transform inlier_out [n_S][total] (may be NULL), ratio_out [n_S][n_pairs] (may be NULL) and median_out [n_S]
 *           hold the bytes rumi_sim3_inliers returns for the same set. */
int rumi_submap_sim3_begin(RumiOptimizer *o, const RumiSim3ScoreSet *set);
int rumi_submap_sim3_end(RumiOptimizer *o);
int rumi_submap_sim3_score(RumiOptimizer *o, int32_t n_S, const double *S_c1w2, const double *S_c2w1, uint8_t *inlier_out, float *ratio_out,
                           float *median_out);

/* The loop of CloudMerging.cc:643-741: one Sim3Solver per selected key-frame pair, each running the rumination overload of iterate
 * (Sim3Solver.cc:292-404) in blocks of 20 until it converges or has used its mRansacMaxIts iterations; the first solver that converges ends the
 * loop.  A solver that does not converge always uses all its iterations, so the iterations form one stream of the shared rand(): solver j runs
 * the positions [sum of the its before it, + its_j).  triples [sum its][3] is flat in solver order, each solver's segment drawn with that
 * solver's n exactly as :321-331, indices relative to its `first`; correspondences are concatenated as for rumi_sim3_ransac_batch.
 * The device evaluates the stream in chunks (ComputeSim3, CheckInliers and ComputeInliersNum of every iteration as rumi_sim3_ransac with
 * score = the resident set under this solver's S_kf) and applies the sequential rule in stream order: per solver mnBestInliers starts at 0,
 * bestRatio starts at best_ratio_in and is shared by the solvers; an iteration is taken when ratio >= bestRatio && nIn >= mnBestInliers (of two
 * equal ones the later is held); it converges when (double)ratio > 0.10 && nIn > min_inliers, which ends the call with the later solvers
 * RUMI_SIM3_NOT_REACHED.  A degenerate minimal set (valid == 0) repeats the solver's last valid iteration; if the solver has none yet it counts
 * 0 inliers under the ratio scored for its identity record, and later degenerate sets repeat that.
 *   results[j]   state (CONVERGED / EXHAUSTED / NOT_REACHED), its = iterations it consumed, best_hyp = stream position of the iteration whose record is
 *                held as mBest* (-1: none was taken; for a repeated degenerate set the position of the iteration it repeats), best_inliers =
 *                mnBestInliers, best_ratio_after = the shared ratio when this solver ended (NOT_REACHED: when the call ended), T12 = that
 *                iteration's record as rumi_sim3_ransac lays it out (zeros when best_hyp is -1)
 *   its_consumed the iterations consumed in all: the caller advances rand() by three times that
 *   n_inliers_all / median_all / T12_all  [sum its] / [sum its] / [sum its][16], each may be NULL: the first its_consumed entries are, per
 *                iteration, the bytes rumi_sim3_ransac returns for that solver and triple; the entries after them are not written
 * The rumination overload never fills vbInliers, so no mask comes back.  Results do not depend on the chunk length.  RUMI_E_INVALID (no set, n < 3,
 * ranges out of order, a triple outside [0, n), its < 1) and RUMI_E_CAPACITY leave every output untouched. */
typedef struct RumiSubmapSolver {
    int32_t first, n;          /* its correspondences in the concatenated X3Dc arrays, n >= 3 */
    int32_t min_inliers, its;  /* mRansacMinInliers; mRansacMaxIts after SetRansacParameters, >= 1 */
    int32_t fix_scale;
    float K4_1[4], K4_2[4];
    double S_kf1w[8], S_kf2w[8];   /* g2o::Sim3(R, t, 1.0) of the solver's mpKF1 / mpKF2 (Sim3Solver.cc:347-348) */
} RumiSubmapSolver;
typedef struct RumiSubmapSolverResult {
    int32_t state;             /* RUMI_SIM3_CONVERGED / _EXHAUSTED / _NOT_REACHED */
    int32_t its;               /* iterations it consumed */
    int32_t best_hyp;          /* stream position of the iteration held as mBest*, -1 if none was taken */
    int32_t best_inliers;      /* mnBestInliers */
    float best_ratio_after;    /* the shared bestInlierRatio when this solver ended */
    float T12[16];             /* that iteration's record as rumi_sim3_ransac lays it out */
} RumiSubmapSolverResult;
int rumi_submap_sim3_ransac(RumiOptimizer *o, int32_t n_solvers, const RumiSubmapSolver *solvers, int32_t n_total, const float *X3Dc1,
                            const float *X3Dc2, const float *sigma2_1, const float *sigma2_2, const int32_t *triples /*[sum its][3]*/,
                            float best_ratio_in, RumiSubmapSolverResult *results, int32_t *its_consumed,
                            int32_t *n_inliers_all, float *median_all, float *T12_all /* [sum its] each, may be NULL */);

/* Optimizer::OptimizeSim3 (the pair form of rumi_optimize_sim3: S_c1w == NULL, no skip flags) of J candidates in one call, one workgroup
 * per problem.  Correspondences are concatenated as above; per problem the bytes rumi_optimize_sim3 returns: S_io8 [J][8] in / out,
 * status_out [n_total], result3 [J][3].  n = 0 and "n - nBad < 10" behave as there. */
typedef struct RumiSim3OptProblem {
    int32_t first, n;
    float th2;
    int32_t fix_scale, robust_first_pass;
    float K4_1[4], K4_2[4];
} RumiSim3OptProblem;
int rumi_optimize_sim3_batch(RumiOptimizer *o, int32_t n_problems, const RumiSim3OptProblem *problems, int32_t n_total, const float *P1c,
                             const float *P2c, const float *obs1, const float *obs2, const float *inv_sigma2_1, const float *inv_sigma2_2,
                             double *S_io8, uint8_t *status_out, int32_t *result3);

/* Optimizer::OptimizeEssentialGraph(pMap, pLoopKF, pCurKF, NonCorrectedSim3, CorrectedSim3, LoopConnections, bFixScale) —
 * R/lib_src/Optimizer.cc:1357-1623 (LoopClosing::CorrectLoop) and its merge overload (pCurKF, vpFixedKFs, vpFixedCorrectedKFs, vpNonFixedKFs,
 * vpNonCorrectedMPs) — :1625-1918: the Sim3 pose graph, Levenberg-Marquardt with setUserLambdaInit(1e-16) over g2o::VertexSim3Expmap vertices
 * and g2o::EdgeSim3 edges with numeric Jacobians (G/core/base_binary_edge.hpp, central differences, delta 1e-9) and identity information.
 *   S_io8      n_v x 8 in/out  vertex estimates (qx qy qz qw tx ty tz s); fixed vertices and vertices without an active edge are not written
 *   fixed      n_v             1 = fixed vertex
 *   fix_scale  n_v             g2o's _fix_scale: the seventh update component is zeroed in oplusImpl (and with it that Jacobian column)
 *   edges      n_e: e_v0 / e_v1 = g2o's vertex 0 / vertex 1, meas8 n_e x 8 = the measurement C; error log(C * S_v0 * S_v1^-1)
 *   n_iterations  optimize(n) (20 upstream); stop_flag as for rumi_local_ba (may be NULL)
 *   stats[4]   LM iterations run, LM trials in total, vertices that took rows, how it ended: 0 ran all iterations, 1 trial limit or rho == 0,
 *              2 three iterations in a row with (iniChi - currentChi) * 1e3 < iniChi, 3 stop flag
 *   chi2_trace n_iterations + 1: the active chi2 before the first iteration (always, also with n_iterations = 0 or a raised stop flag) and
 *              after each one; entries not reached are NaN
 * Active sets as SparseOptimizer::initializeOptimization builds them: an edge whose two vertices are both fixed is NOT active (it adds
 * nothing to chi2), a vertex without an active edge takes no rows and comes back unchanged; a graph without active edges returns RUMI_OK with
 * stats = 0 and an all-NaN trace.  A graph without a fixed vertex is accepted (free gauge, result unpinned).
 * The linear system of every trial is dense: 7 x 7 blocks in vertex order, blocked Cholesky; the matrix ((7 * rows)^2 doubles) is allocated by the
 * first call.  RUMI_E_CAPACITY: n_v above the handle's max_kf or n_e above its max_edges.  Arguments
 * are validated on the host before anything is uploaded (indices, v0 != v1, finite numbers, unit quaternions to 1e-3, positive scales):
 * RUMI_E_INVALID leaves every output untouched.  A HIP error during the run (RUMI_E_NO_DEVICE) leaves S_io8 and stats untouched and
 * chi2_trace partly written (the entries reached, NaN after them).  Two calls on the same input return the same bytes.  Parity against the reference is
 * unpinned: upstream factors with Eigen's sparse Cholesky under a fill-reducing order. */
int rumi_essential_graph(RumiOptimizer *o, int32_t n_v, double *S_io8, const uint8_t *fixed, const uint8_t *fix_scale, int32_t n_e,
                         const int32_t *e_v0, const int32_t *e_v1, const double *meas8, int32_t n_iterations,
                         const volatile uint8_t *stop_flag, int32_t *stats, double *chi2_trace);

/* The map-point correction that ends both overloads.  X n x 3 float in/out; ref[n] = index of the point's reference vertex, -1 = leave the
 * point alone; two per-vertex transform tables of n_v entries.
 *   mode 0 (Optimizer.cc:1611-1616): tab_a = Srw (vScw), tab_b = correctedSwr (vCorrectedSwc), Sim3 as 8 doubles;
 *           X <- float(correctedSwr.map(Srw.map(double(X))))
 *   mode 1 (Optimizer.cc:1907-1911): tab_a = Twr (GetPoseInverse after the write-back), tab_b = TNonCorrectedwr (mTwcBefMerge), SE(3) as 7
 *           floats (qx qy qz qw tx ty tz); X <- (Twr * TNonCorrectedwr^-1) * X in float, associated as written there
 * Same validation rules as above; n within the handle's max_mp. */
int rumi_sim3_correct_points(RumiOptimizer *o, int32_t mode, int32_t n, float *X, const int32_t *ref, int32_t n_v, const void *tab_a,
                             const void *tab_b);

#ifdef __cplusplus
}
#endif
#endif /* RUMI_OPT_H */
