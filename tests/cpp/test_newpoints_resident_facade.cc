// rumi::LocalMappingStep::CreateNewMapPointsResident (facade/LocalMappingStep.h) over the mock data model and a CovisibilityGraph
// (facade/CovisibilityGraph.h), on the GPU.  Reads the scene file of tests/test_newpoints_facade_gpu.py, builds mock KeyFrames and MapPoints,
// stages them through the graph (Sync, SyncFeatures, SyncAttributes), runs the member and prints, like test_newpoints_facade.cc,
//   K k  Tcw[12] Ow[3] F12[9] ep[2]    the pose-derived numbers as THIS FILE forms them from the mock poses (float bits)
//   P neigh idx1 idx2 x y z            every created point, in mlpRecentAddedMapPoints order, read back from the map objects
//   Q stop count                       a second run on a fresh scene and graph whose CheckNewKeyFrames answers true before neighbour `stop`
//   R status created                   the call made while the last neighbour's features had not been synced
//   U bytes                            feature bytes the second call on the same graph uploaded (its key-frames were resident: 0)
#define RUMI_HAVE_SOPHUS 1
#include <cstdio>
#include <cstring>
#include <list>
#include <memory>
#include <vector>

#include "mock_sophus.h"

#include "CovisibilityGraph.h"
#include "LocalMappingStep.h"

#include "mock_model_newpoints_resident.h"

static int fails = 0;
#define CHECK(c, msg) do { if (!(c)) { std::printf("FAIL: %s (%s:%d)\n", msg, __FILE__, __LINE__); fails++; } } while (0)

using Graph = CovisibilityGraph<KeyFrameRS, MapPointRS>;

struct Scene {
    int32_t nkf = 0, coarse = 0, ori = 0, far = 0; float thFar = 0;
    MapRS map;
    std::vector<std::unique_ptr<KeyFrameRS>> kf;
    std::vector<std::unique_ptr<MapPointRS>> old;                 // the points the key-frames hold before the call
};

template <class T> static bool rd(FILE *f, T *p, size_t n) { return n == 0 || std::fread(p, sizeof(T), n, f) == n; }

static bool load(const char *path, Scene &s) {
    FILE *f = std::fopen(path, "rb");
    if (!f) return false;
    int32_t h[4]; float th;
    if (!rd(f, h, 4) || !rd(f, &th, 1)) return false;
    s.nkf = h[0]; s.coarse = h[1]; s.ori = h[2]; s.far = h[3]; s.thFar = th;
    for (int k = 0; k < s.nkf; k++) {
        std::unique_ptr<KeyFrameRS> kf(new KeyFrameRS());
        int32_t n, nn;
        if (!rd(f, &n, 1)) return false;
        kf->N = n; kf->mnId = k; kf->map = &s.map;
        kf->mvKeysUn.resize(n); kf->mDescriptors.create(n > 0 ? n : 1, 32, CV_8U);
        std::vector<int32_t> mp(n); std::vector<float> pos((size_t)n * 3); float R[9], t[3];
        if (!rd(f, kf->mvKeysUn.data(), n) || !rd(f, kf->mDescriptors.ptr(0), (size_t)n * 32) || !rd(f, mp.data(), n) || !rd(f, pos.data(), (size_t)n * 3) ||
            !rd(f, R, 9) || !rd(f, t, 3) || !rd(f, &nn, 1)) return false;
        std::vector<uint32_t> nodes(nn); std::vector<int32_t> off(nn + 1);
        if (!rd(f, nodes.data(), nn) || !rd(f, off.data(), nn + 1)) return false;
        std::vector<uint32_t> idx(off[nn]);
        if (!rd(f, idx.data(), idx.size())) return false;
        for (int a = 0; a < nn; a++) kf->mFeatVec[nodes[a]] = std::vector<unsigned>(idx.begin() + off[a], idx.begin() + off[a + 1]);
        kf->mvScaleFactors.resize(8); kf->mvLevelSigma2.resize(8);
        if (!rd(f, kf->mvScaleFactors.data(), 8)) return false;
        for (int l = 0; l < 8; l++) kf->mvLevelSigma2[l] = kf->mvScaleFactors[l] * kf->mvScaleFactors[l];
        kf->mvuRight.assign(n, -1.f);
        kf->mvpMapPoints.assign(n, nullptr);
        for (int i = 0; i < n; i++)
            if (mp[i] >= 0) {                                    // a point of its own, this key-frame its one observer
                s.old.emplace_back(new MapPointRS(Eigen::Vector3f(pos[3 * i], pos[3 * i + 1], pos[3 * i + 2]), kf.get(), &s.map));
                s.old.back()->AddObservation(kf.get(), i);
                kf->mvpMapPoints[i] = s.old.back().get();
            }
        Eigen::Matrix3f Rm;
        for (int r = 0; r < 3; r++) for (int c = 0; c < 3; c++) Rm(r, c) = R[r * 3 + c];
        kf->SetPose(Sophus::SE3f(Rm, Eigen::Vector3f(t[0], t[1], t[2])));
        s.kf.push_back(std::move(kf));
    }
    std::fclose(f);
    return true;
}

// Key-frames, points and attributes into the graph; the features of every key-frame but the last `withoutFeatures`.
static bool stage(Scene &s, Graph &g, int withoutFeatures) {
    std::vector<MapPointRS *> all;
    for (auto &p : s.old) all.push_back(p.get());
    for (auto &k : s.kf) if (g.Sync(k.get()) != RUMI_OK) return false;
    for (int k = 0; k + withoutFeatures < s.nkf; k++) if (g.SyncFeatures(s.kf[k].get()) != RUMI_OK) return false;
    return g.SyncAttributes(all) == RUMI_OK;
}

static void hex(float v) { uint32_t u; std::memcpy(&u, &v, 4); std::printf(" %08x", u); }

static int64_t feature_upload(Graph &g) {
    int64_t v[6] = {0, 0, 0, 0, 0, -1};
    return rumi_covis_feature_stats(g.handle(), v) == RUMI_OK ? v[5] : -1;
}

int main(int argc, char **argv) {
    if (argc < 3) { std::printf("usage: test_newpoints_resident_facade scene.bin stop\n"); return 2; }
    const int stop = std::atoi(argv[2]);
    Scene s;
    if (!load(argv[1], s)) { std::printf("cannot read %s\n", argv[1]); return 2; }
    KeyFrameRS *cur = s.kf[0].get();
    for (int k = 0; k < s.nkf; k++) {
        KeyFrameRS *kf = s.kf[k].get();
        const Eigen::Matrix3f R = kf->GetPose().rotationMatrix();
        const Eigen::Vector3f t = kf->GetPose().translation(), Ow = kf->GetCameraCenter();
        std::printf("K %d", k);
        for (int r = 0; r < 3; r++) { for (int c = 0; c < 3; c++) hex(R(r, c)); hex(t(r)); }
        for (int r = 0; r < 3; r++) hex(Ow(r));
        Eigen::Matrix3f F; for (int r = 0; r < 3; r++) for (int c = 0; c < 3; c++) F(r, c) = 0.f;
        Eigen::Vector2f ep{{0.f, 0.f}};
        if (k > 0) {
            const Sophus::SE3f T12 = cur->GetPose() * kf->GetPoseInverse();
            F = cur->mpCamera->toK_().transpose().inverse() * Sophus::SO3f::hat(T12.translation()) * T12.rotationMatrix() * kf->mpCamera->toK_().inverse();
            ep = kf->mpCamera->project(kf->GetPose() * cur->GetCameraCenter());
        }
        for (int r = 0; r < 3; r++) for (int c = 0; c < 3; c++) hex(F(r, c));
        hex(ep(0)); hex(ep(1));
        std::printf("\n");
    }
    std::vector<KeyFrameRS *> neigh;
    for (int k = 1; k < s.nkf; k++) neigh.push_back(s.kf[k].get());
    std::vector<std::vector<MapPoint *>> before;
    for (auto &k : s.kf) before.push_back(k->mvpMapPoints);

    rumi::LocalMappingStep step(s.ori != 0);
    Graph graph(64, 1 << 18);
    CHECK(graph.ok() && stage(s, graph, 1), "the scene is staged");
    AtlasRS atlas;
    std::list<MapPoint *> recent;
    int asked = 0;
    auto never = [&] { asked++; return false; };

    // the last neighbour's features were never synced: refused with a report, nothing created, nothing uploaded behind the caller's back
    rumi_facade::clear_status();
    const int refused = step.CreateNewMapPointsResident<MapPointRS>(graph, cur, neigh, &atlas, recent, s.far != 0, s.thFar, never, s.coarse != 0);
    std::printf("R %d %d\n", rumi_facade::last_status(), (int)recent.size());
    CHECK(refused == -1 && recent.empty() && atlas.added.empty() && asked == 0, "a neighbour without resident features is refused");
    CHECK(graph.SyncFeatures(neigh.back()) == RUMI_OK, "SyncFeatures of the last neighbour");
    rumi_facade::clear_status();

    const int n = step.CreateNewMapPointsResident<MapPointRS>(graph, cur, neigh, &atlas, recent, s.far != 0, s.thFar, never, s.coarse != 0);
    CHECK(n >= 0 && n == (int)recent.size() && n == (int)atlas.added.size(), "counts of the created points agree");
    CHECK(asked == (int)neigh.size() - 1 || neigh.empty(), "CheckNewKeyFrames is asked before every neighbour but the first");
    CHECK(feature_upload(graph) > 0, "the first call carried the staged features");
    auto ra = atlas.added.begin();
    for (MapPoint *p : recent) {
        CHECK(p == *ra++, "mpAtlas->AddMapPoint and mlpRecentAddedMapPoints see the points in the same order");
        MapPointRS *q = static_cast<MapPointRS *>(p);
        CHECK(q->obs.size() == 2 && q->obs.count(cur) && q->nObs == 2, "two observations, one of them the current key-frame");
        CHECK(q->nDistinctive == 1 && q->nNormalDepth == 1 && q->mpRefKF == cur && q->map == atlas.GetCurrentMap(), "constructor arguments and the two updates");
        int kn = -1, idx2 = -1;
        for (auto &o : q->obs) if (o.first != cur) { kn = (int)o.first->mnId - 1; idx2 = std::get<0>(o.second); }
        const int idx1 = std::get<0>(q->obs[cur]);
        CHECK(kn >= 0 && cur->GetMapPoint(idx1) == p && before[0][idx1] == nullptr, "the current key-frame's free slot holds the point");
        MapPoint *held = kn >= 0 ? neigh[kn]->GetMapPoint(idx2) : nullptr;
        CHECK(held && before[1 + kn][idx2] == nullptr && std::get<0>(held->obs[neigh[kn]]) == idx2 && held->obs.count(cur), "the neighbour's free slot holds a point of this call");
        std::printf("P %d %d %d", kn, idx1, idx2);
        hex(q->pos(0)); hex(q->pos(1)); hex(q->pos(2));
        std::printf("\n");
    }
    for (size_t k = 0; k < s.kf.size(); k++)
        for (int i = 0; i < s.kf[k]->N; i++)
            if (before[k][i]) CHECK(s.kf[k]->mvpMapPoints[i] == before[k][i], "a slot that held a point is untouched");

    // the graph is current when the member returns: a second call runs on the rows and points the first one left, uploads no feature byte,
    // and no feature that received a point creates another
    std::list<MapPoint *> recentB;
    const int nB = step.CreateNewMapPointsResident<MapPointRS>(graph, cur, neigh, &atlas, recentB, s.far != 0, s.thFar, never, s.coarse != 0);
    CHECK(nB >= 0 && rumi_facade::last_status() == RUMI_OK, "a second call on the same graph goes through");
    std::printf("U %lld\n", (long long)feature_upload(graph));
    for (MapPoint *p : recentB) {
        const int idx1 = std::get<0>(p->obs[cur]);
        bool fresh = before[0][idx1] == nullptr;
        for (MapPoint *q : recent) fresh = fresh && std::get<0>(q->obs[cur]) != idx1;
        CHECK(fresh, "the second call creates points only on features that were still free");
    }

    // early return: a fresh scene and graph, CheckNewKeyFrames true before neighbour `stop`
    Scene s2;
    if (!load(argv[1], s2)) return 2;
    Graph graph2(64, 1 << 18);
    CHECK(graph2.ok() && stage(s2, graph2, 0), "the second scene is staged");
    std::vector<KeyFrameRS *> neigh2;
    for (int k = 1; k < s2.nkf; k++) neigh2.push_back(s2.kf[k].get());
    AtlasRS atlas2;
    std::list<MapPoint *> recent2;
    int i = 0;
    const int n2 = step.CreateNewMapPointsResident<MapPointRS>(graph2, s2.kf[0].get(), neigh2, &atlas2, recent2, s2.far != 0, s2.thFar, [&] { return ++i >= stop; },
                                                               s2.coarse != 0);
    CHECK(n2 == (int)recent2.size(), "the early return reports what it applied");
    auto it = recent.begin();
    for (MapPoint *p : recent2) {
        CHECK(it != recent.end() && std::memcmp(&p->pos, &(*it)->pos, sizeof p->pos) == 0, "the early return leaves a prefix of the full result");
        ++it;
    }
    std::printf("Q %d %d\n", stop, n2);
    for (MapPoint *p : recent) delete static_cast<MapPointRS *>(p);
    for (MapPoint *p : recentB) delete static_cast<MapPointRS *>(p);
    for (MapPoint *p : recent2) delete static_cast<MapPointRS *>(p);
    if (fails) { std::printf("%d checks failed\n", fails); return 1; }
    return 0;
}
