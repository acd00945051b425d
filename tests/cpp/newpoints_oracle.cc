// Scalar restatement of LocalMapping::CreateNewMapPoints, monocular pinhole branch -- the checker of include/rumi_mapping.h.
// TEST INFRASTRUCTURE: built by tests/newpoints_scene.py with g++ -O2 -ffp-contract=off into a shared library next to the test's temporary
// files, linked against oracle/liboracle.so for ORBmatcher::SearchForTriangulation (orc_search_for_triangulation, oracle/match_oracle.cc).
//
// It runs the loop AS THE REFERENCE WRITES IT (R/ = the reference's src/rumi-slam/): neighbour by neighbour, one search per neighbour with the
// flags the earlier neighbours left behind, then one scalar pass over that neighbour's matches.  The decomposition of the device path
// (candidates independent of the order, a replay of the flags) is therefore what a comparison against this file tests.
//
// Null vector of GeometricTools::Triangulate: Eigen::JacobiSVD is not restated (parity unpinned).  It is DEFINED here: the
// eigenvector of the smallest eigenvalue of A^T A by cyclic Jacobi rotations in double, 6 sweeps over the pairs (0,1) (0,2) (0,3) (1,2)
// (1,3) (2,3), smallest diagonal entry (first on ties), de-homogenised in double, cast to float.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "rumi_mapping.h"

extern "C" int orc_search_for_triangulation(const RumiKeyPoint *keys1, const uint8_t *desc1, int n1, const int32_t *mp1, const uint32_t *nodes1,
                                            const int32_t *off1, const uint32_t *idx1, int nn1, const RumiKeyPoint *keys2, const uint8_t *desc2,
                                            int n2, const int32_t *mp2, const uint32_t *nodes2, const int32_t *off2, const uint32_t *idx2, int nn2,
                                            const float *scaleFactors2, const float *F12, const float *ep, int onlyStereo, int coarse,
                                            int checkOrientation, int32_t *matches12);

namespace {

enum { GATE_OK = 0, GATE_PARALLAX, GATE_W0, GATE_Z1, GATE_Z2, GATE_REPROJ1, GATE_REPROJ2, GATE_DIST0, GATE_FAR, GATE_SCALE };

// Eigen evaluates the 3-vector products and norms of this member coefficient by coefficient; the project restates them left to right
// (oracle/match_oracle.cc, orc_is_in_frustum).
inline float dot3(float a0, float a1, float a2, float b0, float b1, float b2) { return (a0 * b0 + a1 * b1) + a2 * b2; }
inline float norm3(float x, float y, float z) { return std::sqrt((x * x + y * y) + z * z); }

void jacobi_rotate(double M[4][4], double V[4][4], int p, int q) {
    if (M[p][q] == 0.0) return;
    const double theta = (M[q][q] - M[p][p]) / (2.0 * M[p][q]);
    const double t = (theta >= 0.0 ? 1.0 : -1.0) / (std::fabs(theta) + std::sqrt(theta * theta + 1.0));
    const double c = 1.0 / std::sqrt(t * t + 1.0), s = t * c;
    for (int r = 0; r < 4; r++) {                       // columns p, q
        const double mp = M[r][p], mq = M[r][q];
        M[r][p] = c * mp - s * mq; M[r][q] = s * mp + c * mq;
    }
    for (int r = 0; r < 4; r++) {                       // rows p, q
        const double mp = M[p][r], mq = M[q][r];
        M[p][r] = c * mp - s * mq; M[q][r] = s * mp + c * mq;
    }
    for (int r = 0; r < 4; r++) {
        const double vp = V[r][p], vq = V[r][q];
        V[r][p] = c * vp - s * vq; V[r][q] = s * vp + c * vq;
    }
}

// stands in for `Eigen::JacobiSVD<Matrix4f> svd(A, ComputeFullV); svd.matrixV().col(3)` (GeometricTools.cc:55-57)
void null_vector4(const float A[4][4], double v[4]) {
    double M[4][4], V[4][4];
    for (int i = 0; i < 4; i++)
        for (int j = 0; j < 4; j++) {
            double s = 0.0;
            for (int r = 0; r < 4; r++) s += (double)A[r][i] * (double)A[r][j];
            M[i][j] = s;
            V[i][j] = i == j ? 1.0 : 0.0;
        }
    for (int sweep = 0; sweep < 6; sweep++)
        for (int p = 0; p < 3; p++)
            for (int q = p + 1; q < 4; q++) jacobi_rotate(M, V, p, q);
    int best = 0;
    for (int j = 1; j < 4; j++) if (M[j][j] < M[best][best]) best = j;
    for (int r = 0; r < 4; r++) v[r] = V[r][best];
}

// GeometricTools::Triangulate (GeometricTools.cc:47-66); Tc1w / Tc2w row-major 3x4
bool triangulate(const float xc1[3], const float xc2[3], const float *T1, const float *T2, float A[4][4], float x3D[3]) {
    for (int j = 0; j < 4; j++) {                       // :49-53
        A[0][j] = xc1[0] * T1[8 + j] - T1[j];
        A[1][j] = xc1[1] * T1[8 + j] - T1[4 + j];
        A[2][j] = xc2[0] * T2[8 + j] - T2[j];
        A[3][j] = xc2[1] * T2[8 + j] - T2[4 + j];
    }
    double v[4];
    null_vector4(A, v);                                 // :55-57
    if ((float)v[3] == 0.f) return false;               // :59-60
    for (int i = 0; i < 3; i++) x3D[i] = (float)(v[i] / v[3]);   // :63
    return true;
}

// KeyFrame::ComputeSceneMedianDepth(q = 2) (KeyFrame.cc:947-978).  An empty vDepths is indexed by the reference (undefined); the entry point
// and this file take -1.0 there, the value the member returns for N == 0.
float scene_median_depth(const RumiNewPointsKF &kf, const int32_t *mp) {
    if (kf.feat.n == 0) return -1.0f;                   // :948-949
    std::vector<float> vDepths;
    vDepths.reserve(kf.feat.n);
    const float *T = kf.Tcw;
    for (int i = 0; i < kf.feat.n; i++)                 // :966-973
        if (mp[i] >= 0) {
            const float *X = kf.mp_pos + 3 * (size_t)i;
            vDepths.push_back(dot3(T[8], T[9], T[10], X[0], X[1], X[2]) + T[11]);
        }
    if (vDepths.empty()) return -1.0f;
    std::sort(vDepths.begin(), vDepths.end());          // :975
    return vDepths[(vDepths.size() - 1) / 2];           // :977
}

// LocalMapping.cc:506-626 for one match; returns the gate that rejected it (GATE_OK: the point is created)
int gates(const RumiNewPointsKF &C, const RumiNewPointsKF &N, int idx1, int idx2, const RumiNewPointsParams &P, float A[4][4], float x3D[3]) {
    const RumiKeyPoint &kp1 = C.feat.keys_un[idx1], &kp2 = N.feat.keys_un[idx2];
    const float *T1 = C.Tcw, *T2 = N.Tcw;
    x3D[0] = x3D[1] = x3D[2] = 0.f;
    std::memset(A, 0, 16 * sizeof(float));
    // :507-508  Pinhole::unprojectEig (Pinhole.cpp:61-64)
    const float xn1[3] = {(kp1.x - C.K4[2]) / C.K4[0], (kp1.y - C.K4[3]) / C.K4[1], 1.f};
    const float xn2[3] = {(kp2.x - N.K4[2]) / N.K4[0], (kp2.y - N.K4[3]) / N.K4[1], 1.f};
    // :510-512  ray = Rwc * xn, Rwc = Rcw^T
    float ray1[3], ray2[3];
    for (int i = 0; i < 3; i++) {
        ray1[i] = dot3(T1[i], T1[4 + i], T1[8 + i], xn1[0], xn1[1], xn1[2]);
        ray2[i] = dot3(T2[i], T2[4 + i], T2[8 + i], xn2[0], xn2[1], xn2[2]);
    }
    const float cosParallaxRays = dot3(ray1[0], ray1[1], ray1[2], ray2[0], ray2[1], ray2[2]) /
                                  (norm3(ray1[0], ray1[1], ray1[2]) * norm3(ray2[0], ray2[1], ray2[2]));
    const float cosParallaxStereo = cosParallaxRays + 1;                  // :514-525, no stereo key-point on either side
    // :531 with bStereo1 = bStereo2 = false, mbInertial = false; the other branches (:535-545) need a stereo key-point
    if (!(cosParallaxRays < cosParallaxStereo && cosParallaxRays > 0 && cosParallaxRays < 0.9998)) return GATE_PARALLAX;
    if (!triangulate(xn1, xn2, T1, T2, A, x3D)) return GATE_W0;           // :532-534
    const float z1 = dot3(T1[8], T1[9], T1[10], x3D[0], x3D[1], x3D[2]) + T1[11];     // :554-556
    if (z1 <= 0) return GATE_Z1;
    const float z2 = dot3(T2[8], T2[9], T2[10], x3D[0], x3D[1], x3D[2]) + T2[11];     // :558-560
    if (z2 <= 0) return GATE_Z2;
    const float sf1 = C.feat.scale_factors[kp1.octave], sf2 = N.feat.scale_factors[kp2.octave];
    const float sigmaSquare1 = sf1 * sf1;                                 // :563 mvLevelSigma2
    const float x1 = dot3(T1[0], T1[1], T1[2], x3D[0], x3D[1], x3D[2]) + T1[3];
    const float y1 = dot3(T1[4], T1[5], T1[6], x3D[0], x3D[1], x3D[2]) + T1[7];
    {                                                                     // :568-574, Pinhole::project (Pinhole.cpp:30-33)
        const float u = C.K4[0] * x1 / z1 + C.K4[2], v = C.K4[1] * y1 / z1 + C.K4[3];
        const float errX1 = u - kp1.x, errY1 = v - kp1.y;
        if ((errX1 * errX1 + errY1 * errY1) > 5.991 * sigmaSquare1) return GATE_REPROJ1;
    }
    const float sigmaSquare2 = sf2 * sf2;                                 // :588
    const float x2 = dot3(T2[0], T2[1], T2[2], x3D[0], x3D[1], x3D[2]) + T2[3];
    const float y2 = dot3(T2[4], T2[5], T2[6], x3D[0], x3D[1], x3D[2]) + T2[7];
    {                                                                     // :592-597
        const float u = N.K4[0] * x2 / z2 + N.K4[2], v = N.K4[1] * y2 / z2 + N.K4[3];
        const float errX2 = u - kp2.x, errY2 = v - kp2.y;
        if ((errX2 * errX2 + errY2 * errY2) > 5.991 * sigmaSquare2) return GATE_REPROJ2;
    }
    const float dist1 = norm3(x3D[0] - C.Ow[0], x3D[1] - C.Ow[1], x3D[2] - C.Ow[2]);  // :610-614
    const float dist2 = norm3(x3D[0] - N.Ow[0], x3D[1] - N.Ow[1], x3D[2] - N.Ow[2]);
    if (dist1 == 0 || dist2 == 0) return GATE_DIST0;                      // :616-617
    if (P.far_points && (dist1 >= P.th_far_points || dist2 >= P.th_far_points)) return GATE_FAR;   // :619-620
    const float ratioDist = dist2 / dist1;                                // :622-626
    const float ratioOctave = sf1 / sf2;
    if (ratioDist * P.ratio_factor < ratioOctave || ratioDist > ratioOctave * P.ratio_factor) return GATE_SCALE;
    return GATE_OK;
}

}  // namespace

extern "C" {

// One evaluated match: what happened to it, with the matrix A of its triangulation (zero when the parallax test stopped it before).
struct NpoTrace { int32_t neigh, idx1, idx2, gate; float x3D[3]; float A[16]; };

float npo_median_depth(const RumiNewPointsKF *kf) { return scene_median_depth(*kf, kf->kf_mp); }

int npo_triangulate(const float *xc1, const float *xc2, const float *T1, const float *T2, float *A16, float *x3D) {
    float A[4][4];
    const bool ok = triangulate(xc1, xc2, T1, T2, A, x3D);
    std::memcpy(A16, A, sizeof A);
    return ok ? 1 : 0;
}

// LocalMapping::CreateNewMapPoints (LocalMapping.cc:354-647).  matches [n_neigh][cur.n]: vMatchedIndices of every neighbour as idx2 per idx1
// (-1 none); flags_before [n_neigh][cur.n]: the current key-frame's map-point flags when that neighbour's search started; hist_removed
// [n_neigh]: pairs the rotation histogram took away.  Each of the four may be NULL.  Returns the number of created points (all are counted,
// the first cap are stored).
int npo_create_new_map_points(const RumiNewPointsKF *cur, const RumiNewPointsKF *neigh, int n_neigh, const RumiNewPointsParams *p,
                              RumiNewPoint *out, int cap, int32_t *per_neigh, uint8_t *skipped, int32_t *matches, int32_t *flags_before,
                              int32_t *hist_removed, NpoTrace *trace, int trace_cap, int32_t *n_trace) {
    const int n1 = cur->feat.n;
    std::vector<int32_t> mp1(cur->kf_mp, cur->kf_mp + n1), m12(std::max(n1, 1)), m12NoOri(std::max(n1, 1));
    int nOut = 0, nTrace = 0;
    for (int i = 0; i < n_neigh; i++) {                                   // :397
        const RumiNewPointsKF &N = neigh[i];
        per_neigh[i] = 0; skipped[i] = 0;
        if (hist_removed) hist_removed[i] = 0;
        if (matches) std::fill(matches + (size_t)i * n1, matches + (size_t)(i + 1) * n1, -1);
        if (flags_before) std::copy(mp1.begin(), mp1.end(), flags_before + (size_t)i * n1);
        // :405-419  baseline against the scene's median depth
        const float baseline = norm3(N.Ow[0] - cur->Ow[0], N.Ow[1] - cur->Ow[1], N.Ow[2] - cur->Ow[2]);
        const float medianDepthKF2 = scene_median_depth(N, N.kf_mp);
        const float ratioBaselineDepth = baseline / medianDepthKF2;
        if (ratioBaselineDepth < 0.01) { skipped[i] = 1; continue; }
        // :421-425  matcher.SearchForTriangulation(mpCurrentKeyFrame, pKF2, vMatchedIndices, false, bCoarse)
        std::vector<int32_t> mp2(N.kf_mp, N.kf_mp + N.feat.n);
        orc_search_for_triangulation(cur->feat.keys_un, cur->feat.desc, n1, mp1.data(), cur->fv.node_ids, cur->fv.offsets, cur->fv.indices,
                                     cur->fv.n_nodes, N.feat.keys_un, N.feat.desc, N.feat.n, mp2.data(), N.fv.node_ids, N.fv.offsets, N.fv.indices,
                                     N.fv.n_nodes, N.feat.scale_factors, N.F12, N.epipole2, 0, p->coarse, p->check_orientation, m12.data());
        if (hist_removed && p->check_orientation) {
            orc_search_for_triangulation(cur->feat.keys_un, cur->feat.desc, n1, mp1.data(), cur->fv.node_ids, cur->fv.offsets, cur->fv.indices,
                                         cur->fv.n_nodes, N.feat.keys_un, N.feat.desc, N.feat.n, mp2.data(), N.fv.node_ids, N.fv.offsets,
                                         N.fv.indices, N.fv.n_nodes, N.feat.scale_factors, N.F12, N.epipole2, 0, p->coarse, 0, m12NoOri.data());
            for (int i1 = 0; i1 < n1; i1++) hist_removed[i] += (m12NoOri[i1] >= 0 && m12[i1] < 0) ? 1 : 0;
        }
        // :440-645  vMatchedIndices is vMatches12 read in index order (ORBmatcher.cc:1003-1010)
        for (int idx1 = 0; idx1 < n1; idx1++) {
            const int idx2 = m12[idx1];
            if (idx2 < 0) continue;
            if (matches) matches[(size_t)i * n1 + idx1] = idx2;
            float A[4][4], x3D[3];
            const int g = gates(*cur, N, idx1, idx2, *p, A, x3D);
            if (trace && nTrace < trace_cap) {
                NpoTrace &t = trace[nTrace];
                t.neigh = i; t.idx1 = idx1; t.idx2 = idx2; t.gate = g;
                std::memcpy(t.x3D, x3D, sizeof x3D); std::memcpy(t.A, A, sizeof A);
            }
            nTrace++;
            if (g != GATE_OK) continue;
            // :628-644  the point is created: both key-frames now hold a map point at these features
            if (nOut < cap) { RumiNewPoint &o = out[nOut]; o.neigh = i; o.idx1 = idx1; o.idx2 = idx2; std::memcpy(o.x3D, x3D, sizeof x3D); }
            nOut++;
            per_neigh[i]++;
            mp1[idx1] = 1 << 30;                                          // mpCurrentKeyFrame->AddMapPoint(pMP, idx1)
            mp2[idx2] = 1 << 30;                                          // pKF2->AddMapPoint(pMP, idx2)
        }
    }
    if (n_trace) *n_trace = nTrace;
    return nOut;
}

}  // extern "C"
