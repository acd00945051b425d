// Optimizer::LocalBundleAdjustmentResident (facade/Optimizer.h) over a CovisibilityGraph and the mock data model of
// tests/cpp/mock_model_lba_resident.h, against Optimizer::LocalBundleAdjustment on a copy of the same map, on the GPU.  One window: key-frame 5
// is current, 1..4 are covisible, 0 (the map's initial key-frame) sees the points from outside; every thirtieth observation lies 25 px off.
// Map A belongs to a graph and takes the resident member; map B takes the member that walks the objects, followed by the block refresh
// (rumi_facade::RefreshMapPoints, normal and depth) of the window's points, which is what UpdateNormalAndDepth computes for them.  The
// key-frames of a map lie in one array, so both maps' std::map<KeyFrame*, ...> iterate in index order and the two sides must agree bit for bit.
// Prints FAIL lines and one summary line; the exit status is the number of failed checks.
#define RUMI_HAVE_SOPHUS 1
#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>
#include <random>
#include <vector>

#include "mock_sophus.h"

#include "CovisibilityGraph.h"
#include "Optimizer.h"
#include "rumi_testhooks.h"

#include "mock_model_lba_resident.h"

static int fails = 0;
#define CHECK(c, msg) do { if (!(c)) { std::printf("FAIL: %s (%s:%d)\n", msg, __FILE__, __LINE__); fails++; } } while (0)

struct World {
    MapLR map;
    int nKf = 6;
    std::unique_ptr<KeyFrameLR[]> kf;
    std::vector<std::unique_ptr<MapPointLR>> mp;
};

static void build(World &w, int nPts) {
    std::mt19937 rng(7);
    std::normal_distribution<float> g(0.f, 1.f);
    w.kf.reset(new KeyFrameLR[w.nKf]);
    for (int p = 0; p < nPts; p++) {
        w.mp.emplace_back(new MapPointLR());
        MapPointLR *P = w.mp[p].get();
        P->map = &w.map; P->nObs = 0;
        P->pos = Eigen::Vector3f((rng() % 600) / 100.f - 3.f, (rng() % 400) / 100.f - 2.f, 3.f + (rng() % 500) / 100.f);
        P->mDescriptor.create(1, 32, CV_8U);
        std::memset(P->mDescriptor.ptr(0), 0x5A, 32);
        P->mNormalVector = Eigen::Vector3f(7.f, 7.f, 7.f);
    }
    for (int k = 0; k < w.nKf; k++) {
        KeyFrameLR &K = w.kf[k];
        K.mnId = k; K.map = &w.map; K.mnScaleLevels = 8;
        for (int l = 0; l < 8; l++) { const float s = std::pow(1.2f, (float)l); K.mvScaleFactors.push_back(s); K.mvLevelSigma2.push_back(s * s); K.mvInvLevelSigma2.push_back(1.0f / (s * s)); }
        const float a = 0.03f * (k - 3);
        K.SetPose(Sophus::SE3f(Eigen::Quaternionf(std::cos(a / 2), 0.f, std::sin(a / 2), 0.f), Eigen::Vector3f(-0.25f * k + 0.6f, 0.01f * k, 0.02f * k)));
    }
    for (int k = 1; k < w.nKf - 1; k++) w.kf[w.nKf - 1].covis.push_back(&w.kf[k]);
    for (int p = 0; p < nPts; p++)
        for (int k = 0; k < w.nKf; k++) {
            KeyFrameLR &K = w.kf[k];
            const Eigen::Vector3f Xc = K.GetPose() * w.mp[p]->pos;
            const float u = 535.4f * Xc(0) / Xc(2) + 320.1f, v = 539.2f * Xc(1) / Xc(2) + 247.6f;
            if (Xc(2) < 0.5f || u < 0 || u >= 640 || v < 0 || v >= 480) continue;
            cv::KeyPoint kp;
            kp.octave = (int)(rng() % 3);
            kp.pt.x = u + 0.7f * g(rng); kp.pt.y = v + 0.7f * g(rng);
            if (rng() % 30 == 0) kp.pt.x += 25.f;
            const int idx = (int)K.mvKeysUn.size();
            K.mvKeysUn.push_back(kp); K.mvuRight.push_back(-1.f); K.mvpMapPoints.push_back(w.mp[p].get()); K.N++;
            w.mp[p]->MapPoint::AddObservation(&K, idx);
            if (!w.mp[p]->mpRefKF) w.mp[p]->mpRefKF = &K;
        }
    for (int k = 0; k < w.nKf; k++) {
        KeyFrameLR &K = w.kf[k];
        K.mDescriptors.create(K.N > 0 ? K.N : 1, 32, CV_8U);
        std::memset(K.mDescriptors.ptr(0), 0x11 * (k + 1), (size_t)(K.N > 0 ? K.N : 1) * 32);
        if (k >= 1) {                                                       // the estimates of the local key-frames are a little off
            const Sophus::SE3f T = K.GetPose();
            K.SetPose(Sophus::SE3f(T.unit_quaternion(), T.translation() + Eigen::Vector3f(0.01f * g(rng), 0.f, 0.01f * g(rng))));
        }
    }
    for (int p = 0; p < nPts; p++) w.mp[p]->pos = w.mp[p]->pos + Eigen::Vector3f(0.02f * g(rng), 0.02f * g(rng), 0.02f * g(rng));
}

template <class T> static bool same_bits(const T &a, const T &b) { return std::memcmp(&a, &b, sizeof(T)) == 0; }

int main() {
    const int nPts = 200;
    World A, B;
    build(A, nPts);
    build(B, nPts);
    using Graph = CovisibilityGraph<KeyFrameLR, MapPointLR>;
    Graph graph(A.nKf + 2, nPts + 2);
    if (!graph.ok()) return 3;
    std::vector<KeyFrameLR *> kfsA;
    std::vector<MapPointLR *> allA;
    for (int k = 0; k < A.nKf; k++) {
        kfsA.push_back(&A.kf[k]);
        if (graph.Sync(&A.kf[k]) != RUMI_OK || graph.SyncFeatures(&A.kf[k]) != RUMI_OK) return 3;
    }
    for (auto &p : A.mp) { allA.push_back(p.get()); if (graph.Sync(p.get()) != RUMI_OK) return 3; }
    if (graph.SyncCentres(kfsA) != RUMI_OK || graph.SyncReferences(allA) != RUMI_OK || graph.SyncAttributes(allA) != RUMI_OK || graph.SyncPoses(kfsA) != RUMI_OK ||
        graph.SyncPointMaps(allA) != RUMI_OK)
        return 3;

    int cA[4] = {-1, -1, -1, -1}, cB[4] = {-1, -1, -1, -1};
    bool stop = false;
    ORB_SLAM3::Optimizer::LocalBundleAdjustmentResident(graph, &A.kf[5], &stop, &A.map, cA[0], cA[1], cA[2], cA[3]);
    ORB_SLAM3::Optimizer::LocalBundleAdjustment(&B.kf[5], &stop, &B.map, cB[0], cB[1], cB[2], cB[3]);
    std::vector<MapPointLR *> windowB;
    for (auto &p : B.mp) if (p->mnBALocalForKF == B.kf[5].mnId) windowB.push_back(p.get());
    CHECK(rumi_facade::RefreshMapPoints(windowB, RUMI_REFRESH_NORMAL_DEPTH) == (int)windowB.size(), "the block refresh of map B's window");

    CHECK(std::memcmp(cA, cB, sizeof cA) == 0 && cA[0] == 1 && cA[1] == 5 && cA[2] == (int)windowB.size() && cA[3] > 4 * cA[2], "the four counters");
    CHECK(A.map.changes == 1 && B.map.changes == 1, "IncreaseChangeIndex");
    int poses = 0, moved = 0;
    World C;
    build(C, nPts);                                                          // the map as it was
    for (int k = 0; k < A.nKf; k++) {
        const Sophus::SE3f a = A.kf[k].GetPose(), b = B.kf[k].GetPose(), c = C.kf[k].GetPose();
        poses += same_bits(a.q, b.q) && same_bits(a.t, b.t);
        moved += !(same_bits(a.q, c.q) && same_bits(a.t, c.t));
    }
    CHECK(poses == A.nKf && moved == 5, "poses: equal on both sides, the five local key-frames moved, the fixed one did not");
    int pos = 0, normals = 0, ranges = 0, obsEq = 0, written = 0;
    size_t obsLeft = 0, obsWere = 0;
    for (int p = 0; p < nPts; p++) {
        MapPointLR *a = A.mp[p].get(), *b = B.mp[p].get();
        pos += same_bits(a->pos, b->pos);
        normals += same_bits(a->mNormalVector, b->mNormalVector) && a->nSetNormal == b->nSetNormal;
        ranges += same_bits(a->mfMinDistance, b->mfMinDistance) && same_bits(a->mfMaxDistance, b->mfMaxDistance) && a->nSetRange == b->nSetRange;
        written += a->nSetNormal;
        bool eq = a->obs.size() == b->obs.size();
        for (auto &o : a->obs) {
            const int k = (int)(static_cast<KeyFrameLR *>(o.first) - A.kf.get());
            auto it = b->obs.find(&B.kf[k]);
            eq = eq && it != b->obs.end() && it->second == o.second;
        }
        obsEq += eq;
        obsLeft += a->obs.size(); obsWere += C.mp[p]->obs.size();
    }
    CHECK(pos == nPts && normals == nPts && ranges == nPts, "positions, normals and depth ranges");
    CHECK(written == cA[2], "every window point was refreshed once");
    CHECK(obsEq == nPts && obsLeft < obsWere, "the same observations were erased, and some were");
    int rows = 0;
    for (int k = 0; k < A.nKf; k++) {
        bool eq = A.kf[k].mvpMapPoints.size() == B.kf[k].mvpMapPoints.size();
        for (size_t i = 0; eq && i < A.kf[k].mvpMapPoints.size(); i++) eq = (A.kf[k].mvpMapPoints[i] == nullptr) == (B.kf[k].mvpMapPoints[i] == nullptr);
        rows += eq;
    }
    CHECK(rows == A.nKf, "EraseMapPointMatch on the same features");

    // ---- the store is current for the window without a SyncAttributes: position, normal and range of the device's records are the members
    std::vector<int32_t> ids;
    std::vector<MapPointLR *> windowA;
    for (int p = 0; p < nPts; p++) if (B.mp[p]->mnBALocalForKF == B.kf[5].mnId) { windowA.push_back(A.mp[p].get()); ids.push_back(graph.IdOf(A.mp[p].get())); }
    std::vector<uint8_t> rec(ids.size() * 64);
    int current = -1;
    if (rumi_hook_covis_read_attributes(graph.handle(), (int32_t)ids.size(), ids.data(), rec.data(), 1) == RUMI_OK) {
        current = 0;
        for (size_t i = 0; i < ids.size(); i++) {
            MapPointLR *p = windowA[i];
            const float f[8] = {p->pos(0), p->pos(1), p->pos(2), p->mNormalVector(0), p->mNormalVector(1), p->mNormalVector(2), p->mfMinDistance, p->mfMaxDistance};
            current += std::memcmp(rec.data() + 64 * i, f, 32) == 0;
        }
    }
    CHECK(current == (int)ids.size(), "the device's attribute records hold the new positions, normals and ranges");

    // ---- a second window on both sides: the graph was synced by what changed, so the two stay equal
    for (auto &p : B.mp) p->mnBALocalForKF = -1;                             // the stamps of the first window (a new key-frame has a new mnId)
    for (int k = 0; k < B.nKf; k++) B.kf[k].mnBALocalForKF = B.kf[k].mnBAFixedForKF = -1;
    ORB_SLAM3::Optimizer::LocalBundleAdjustmentResident(graph, &A.kf[5], &stop, &A.map, cA[0], cA[1], cA[2], cA[3]);
    ORB_SLAM3::Optimizer::LocalBundleAdjustment(&B.kf[5], &stop, &B.map, cB[0], cB[1], cB[2], cB[3]);
    int again = 0;
    for (int p = 0; p < nPts; p++) again += same_bits(A.mp[p]->pos, B.mp[p]->pos) && A.mp[p]->obs.size() == B.mp[p]->obs.size();
    for (int k = 0; k < A.nKf; k++) again += same_bits(A.kf[k].GetPose().q, B.kf[k].GetPose().q) && same_bits(A.kf[k].GetPose().t, B.kf[k].GetPose().t);
    CHECK(std::memcmp(cA, cB, sizeof cA) == 0 && again == nPts + A.nKf && cA[3] > 0, "the second window after the sync by what changed");

    // ---- a raised stop flag: nothing is written
    stop = true;
    const Sophus::SE3f before = A.kf[5].GetPose();
    int cS[4] = {-7, -7, -7, -7};
    ORB_SLAM3::Optimizer::LocalBundleAdjustmentResident(graph, &A.kf[5], &stop, &A.map, cS[0], cS[1], cS[2], cS[3]);
    CHECK(A.map.changes == 2 && same_bits(before.q, A.kf[5].GetPose().q) && same_bits(before.t, A.kf[5].GetPose().t) && cS[0] == -7, "stop flag");
    std::printf("done %d: fixed %d opt %d points %d edges %d, %zu of %zu observations left\n", fails, cA[0], cA[1], cA[2], cA[3], obsLeft, obsWere);
    return fails;
}
