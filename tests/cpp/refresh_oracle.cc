// Scalar restatement of MapPoint::ComputeDistinctiveDescriptors (R/lib_src/MapPoint.cc:353-427) and MapPoint::UpdateNormalAndDepth
// (:450-518) on the flat arrays of rumi_refresh_map_points (include/rumi_mapping.h), monocular (left indices only).  TEST ORACLE: it really
// builds the N x N matrix and sorts every row, so it shares nothing with the device's rank selection.  Built with -ffp-contract=off; the float
// operation order below is the definition the header states (Eigen is not available, so its norm() is not what is pinned).
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdint>
#include <vector>

#include "rumi_mapping.h"

static int descriptor_distance(const uint8_t *a, const uint8_t *b) {          // ORBmatcher::DescriptorDistance, bit by bit
    int dist = 0;
    for (int k = 0; k < 32; k++) {
        unsigned v = a[k] ^ b[k];
        while (v) { dist += v & 1; v >>= 1; }
    }
    return dist;
}

static float norm3(float x, float y, float z) { return std::sqrt((x * x + y * y) + z * z); }

// One point.  Outputs are written only where the reference writes its members.
static void distinctive(const RumiRefreshKF *kf, const RumiRefreshPoint &P, const int32_t *obs_kf, const int32_t *obs_feature, int32_t *best_obs,
                        int32_t *best_median) {
    *best_obs = -1; *best_median = -1;
    if (P.obs_end == P.obs_begin) return;                                     // :367-368
    std::vector<const uint8_t *> vDescriptors;
    std::vector<int> where;
    for (int o = P.obs_begin; o < P.obs_end; o++) {                           // :372-387, in the caller's (the map's) order
        const RumiRefreshKF &K = kf[obs_kf[o]];
        if (K.is_bad) continue;                                               // :376
        vDescriptors.push_back(K.desc + 32 * (size_t)obs_feature[o]);         // :381
        where.push_back(o - P.obs_begin);
    }
    if (vDescriptors.empty()) return;                                         // :389-390
    const size_t N = vDescriptors.size();                                     // :393
    std::vector<float> Distances(N * N);                                      // :395 float Distances[N][N]
    for (size_t i = 0; i < N; i++) {
        Distances[i * N + i] = 0;                                             // :398
        for (size_t j = i + 1; j < N; j++) {
            const int distij = descriptor_distance(vDescriptors[i], vDescriptors[j]);   // :401
            Distances[i * N + j] = distij; Distances[j * N + i] = distij;     // :402-403
        }
    }
    int BestMedian = INT_MAX, BestIdx = 0;                                    // :408-409
    for (size_t i = 0; i < N; i++) {
        std::vector<int> vDists(Distances.begin() + i * N, Distances.begin() + (i + 1) * N);   // :412
        std::sort(vDists.begin(), vDists.end());                              // :413
        const int median = vDists[0.5 * (N - 1)];                             // :414
        if (median < BestMedian) { BestMedian = median; BestIdx = (int)i; }   // :416-420
    }
    *best_obs = where[BestIdx]; *best_median = BestMedian;                    // :425 mDescriptor = vDescriptors[BestIdx].clone()
}

static void normal_and_depth(const RumiRefreshKF *kf, const RumiRefreshPoint &P, const int32_t *obs_kf, float *normal, float *min_distance,
                             float *max_distance, uint8_t *updated) {
    *updated = 0;
    if (P.obs_end == P.obs_begin) return;                                     // :465-466
    float nx = 0.f, ny = 0.f, nz = 0.f;                                       // :468-469
    int n = 0;
    for (int o = P.obs_begin; o < P.obs_end; o++) {                           // :471-490: no isBad test here
        const float *Owi = kf[obs_kf[o]].Ow;                                  // :479
        const float dx = P.pos[0] - Owi[0], dy = P.pos[1] - Owi[1], dz = P.pos[2] - Owi[2];   // :480
        const float nrm = norm3(dx, dy, dz);
        nx = nx + dx / nrm; ny = ny + dy / nrm; nz = nz + dz / nrm;           // :481
        n++;
    }
    const RumiRefreshKF &R = kf[P.ref_kf];
    const float dist = norm3(P.pos[0] - R.Ow[0], P.pos[1] - R.Ow[1], P.pos[2] - R.Ow[2]);   // :492-493
    const float levelScaleFactor = R.scale_factors[P.ref_level];              // :499, :509
    const int nLevels = R.nlevels;                                            // :510
    *max_distance = dist * levelScaleFactor;                                  // :514
    *min_distance = *max_distance / R.scale_factors[nLevels - 1];             // :515
    const float fn = (float)n;
    normal[0] = nx / fn; normal[1] = ny / fn; normal[2] = nz / fn;            // :516
    *updated = 1;
}

// The per-point loop a host caller runs today.  Same arguments as rumi_refresh_map_points, without the handle; the inputs are trusted.
extern "C" int rfo_refresh_map_points(const RumiRefreshKF *kf, int32_t n_kf, const RumiRefreshPoint *pts, int32_t n_pts, const int32_t *obs_kf,
                                      const int32_t *obs_feature, int32_t n_obs, int32_t what, int32_t *best_obs, int32_t *best_median,
                                      float *normal, float *min_distance, float *max_distance, uint8_t *updated) {
    (void)n_kf; (void)n_obs;
    for (int i = 0; i < n_pts; i++) {
        if (what & RUMI_REFRESH_DESCRIPTOR) distinctive(kf, pts[i], obs_kf, obs_feature, &best_obs[i], &best_median[i]);
        if (what & RUMI_REFRESH_NORMAL_DEPTH) normal_and_depth(kf, pts[i], obs_kf, normal + 3 * i, &min_distance[i], &max_distance[i], &updated[i]);
    }
    return 0;
}
