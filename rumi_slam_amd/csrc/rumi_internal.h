// Entry points one translation unit of librumi_hip.so offers another (not part of the C ABI).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

typedef struct RumiVocabulary RumiVocabulary;
typedef struct RumiMatcher RumiMatcher;

namespace rumi {

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
