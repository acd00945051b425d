/*
 * rumi_mapping.h — C ABI of the LocalMapping members that have no ORBmatcher form (librumi_hip.so).
 *
 * Drop-in boundary (R/ = the reference's src/rumi-slam/):
 *   R/lib_src/LocalMapping.cc:354-647     LocalMapping::CreateNewMapPoints, monocular pinhole branch
 *   R/lib_src/ORBmatcher.cc:806-1013      ORBmatcher::SearchForTriangulation (as rumi_search_for_triangulation, rumi_match.h)
 *   R/lib_src/KeyFrame.cc:947-978         KeyFrame::ComputeSceneMedianDepth(2)
 *   R/lib_src/GeometricTools.cc:47-66     GeometricTools::Triangulate
 *   R/lib_src/CameraModels/Pinhole.cpp:30-33,61-64   Pinhole::project / unprojectEig
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

#ifdef __cplusplus
}
#endif
#endif /* RUMI_MAPPING_H */
