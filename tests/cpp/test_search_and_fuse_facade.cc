// LoopClosingStep::SearchAndFuseResident (facade/LoopClosingStep.h) over a CovisibilityGraph and the mock data model of
// tests/cpp/mock_model_search_and_fuse.h, against the reference's member text (LoopClosing.cc:1996-2065) over the merged
// rumi_facade::ORBmatcher::Fuse(pKF, Scw, ...) -- one call per key-frame, then the Replace loop -- on a copy of the same map, on the GPU.
// Reads a map written by tests/test_search_and_fuse_facade_gpu.py.  Map A belongs to a graph (every key-frame and point staged, features and
// attributes) and takes the resident member; map B takes the member text.  Prints
//   F map ret status searchedAgain
//   K map k | row...
//   P map i bad replaced n (kf feature)... | descriptor
#define RUMI_HAVE_SOPHUS 1
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <map>
#include <memory>
#include <vector>

#include "mock_sophus.h"

#include "CovisibilityGraph.h"
#include "LoopClosingStep.h"

#include "mock_model_search_and_fuse.h"

template <class T> static bool rd(FILE *f, T *p, size_t n) { return n == 0 || std::fread(p, sizeof(T), n, f) == n; }

struct World {
    MapKR map;
    std::vector<std::unique_ptr<KeyFrameSN>> kfs;
    std::vector<std::unique_ptr<MapPointSN>> mps;
    std::vector<std::pair<KeyFrameSN *, Sim3fQ>> poses;           // the corrected key-frames in call order
    std::vector<MapPointSN *> loop;                                // vpMapPoints
};

// header: n_kf n_pts n_corr n_ids nleftKf unsyncedKf unseenPoint mode (0: Sim3 poses, 1: the key-frame vector overload, 2: 641 key-frames)
static bool load(const char *path, int32_t *h, World &w) {
    FILE *f = std::fopen(path, "rb");
    if (!f) return false;
    if (!rd(f, h, 8)) return false;
    for (int k = 0; k < h[0]; k++) {
        std::unique_ptr<KeyFrameSN> kf(new KeyFrameSN());
        int32_t n;
        float T7[7];
        if (!rd(f, &n, 1) || !rd(f, T7, 7)) return false;
        kf->N = n; kf->mnId = k + 1; kf->map = &w.map; kf->mTimeStamp = k;
        kf->mvKeysUn.resize(n);
        kf->mDescriptors.create(n > 0 ? n : 1, 32, CV_8U);
        std::vector<int32_t> row(n);
        static_assert(sizeof(cv::KeyPoint) == 28, "the file holds 28-byte key-points");
        if (!rd(f, kf->mvKeysUn.data(), n) || !rd(f, kf->mDescriptors.ptr(0), (size_t)n * 32) || !rd(f, row.data(), n)) return false;
        kf->mvScaleFactors.assign(8, 1.f);
        for (int l = 1; l < 8; l++) kf->mvScaleFactors[l] = kf->mvScaleFactors[l - 1] * 1.2f;
        kf->mnScaleLevels = 8; kf->mfLogScaleFactor = std::log(1.2f);
        kf->fx = kf->fy = 500.f; kf->cx = 320.f; kf->cy = 240.f;
        kf->cam.fx = kf->cam.fy = 500.f; kf->cam.cx = 320.f; kf->cam.cy = 240.f;
        kf->pose = Sophus::SE3f(Eigen::Quaternionf(T7[3], T7[0], T7[1], T7[2]), Eigen::Vector3f(T7[4], T7[5], T7[6]));
        kf->mvuRight.assign(n, -1.f);
        kf->mvpMapPoints.assign(n, nullptr);
        if (k == h[4]) kf->NLeft = 0;
        w.kfs.push_back(std::move(kf));
        for (int i = 0; i < n; i++) w.kfs.back()->mvpMapPoints[i] = reinterpret_cast<MapPoint *>((intptr_t)(row[i] + 1));   // ids for now
    }
    for (int c = 0; c < h[2]; c++) {
        int32_t k;
        float a[8];                                                // q xyzw, t, s
        if (!rd(f, &k, 1) || !rd(f, a, 8) || k < 0 || k >= h[0]) return false;
        w.poses.emplace_back(w.kfs[k].get(), Sim3fQ(Eigen::Quaternionf(a[3], a[0], a[1], a[2]).toRotationMatrix(), Eigen::Vector3f(a[4], a[5], a[6]), a[7]));
    }
    std::vector<int32_t> ids(h[3]);
    if (!rd(f, ids.data(), ids.size())) return false;
    for (int i = 0; i < h[1]; i++) {
        std::unique_ptr<MapPointSN> p(new MapPointSN());
        float a[8];
        int32_t bad;
        p->desc.create(1, 32, CV_8U);
        if (!rd(f, a, 8) || !rd(f, p->desc.ptr(0), 32) || !rd(f, &bad, 1)) return false;
        p->pos = Eigen::Vector3f(a[0], a[1], a[2]); p->normal = Eigen::Vector3f(a[3], a[4], a[5]); p->minD = a[6]; p->maxD = a[7];
        p->bad = bad != 0; p->map = &w.map; p->nObs = 0;
        w.mps.push_back(std::move(p));
    }
    std::fclose(f);
    for (auto &kf : w.kfs)
        for (int i = 0; i < kf->N; i++) {
            const intptr_t id = reinterpret_cast<intptr_t>(kf->mvpMapPoints[i]) - 1;
            MapPointSN *p = id >= 0 ? w.mps[id].get() : nullptr;
            kf->mvpMapPoints[i] = p;
            if (p && !p->bad) { p->obs[kf.get()] = std::make_tuple(i, -1); p->nObs++; if (!p->mpRefKF) p->mpRefKF = kf.get(); }
        }
    for (int32_t id : ids) {
        if (id < 0 || id >= h[1]) return false;                    // the reference's list holds no NULL
        w.loop.push_back(w.mps[id].get());
    }
    return true;
}

static void print(const char *tag, World &w) {
    std::map<const void *, int> pi, ki;
    for (size_t i = 0; i < w.mps.size(); i++) pi[w.mps[i].get()] = (int)i;
    for (size_t k = 0; k < w.kfs.size(); k++) ki[w.kfs[k].get()] = (int)k;
    for (size_t k = 0; k < w.kfs.size(); k++) {
        std::printf("K %s %zu |", tag, k);
        for (MapPoint *p : w.kfs[k]->mvpMapPoints) std::printf(" %d", p ? pi[p] : -1);
        std::printf("\n");
    }
    for (size_t i = 0; i < w.mps.size(); i++) {
        MapPointSN *p = w.mps[i].get();
        std::map<int, int> o;                                      // by key-frame index: the two maps' addresses order differently
        for (auto &e : p->obs) o[ki[e.first]] = std::get<0>(e.second);
        std::printf("P %s %zu %d %d %zu", tag, i, (int)p->bad, p->mpReplaced ? pi[p->mpReplaced] : -1, o.size());
        for (auto &e : o) std::printf(" %d %d", e.first, e.second);
        std::printf(" | ");
        for (int b = 0; b < 32; b++) std::printf("%02x", p->desc.ptr(0)[b]);
        std::printf("\n");
    }
}

// LoopClosing.cc:1996-2028 as written, over the facade's Fuse; the sum of numFused is returned for the comparison
static int member_text_sim3(World &w) {
    rumi::LoopClosingStep matcher;
    std::vector<MapPointSN *> &vpMapPoints = w.loop;
    int total = 0;
    for (auto mit = w.poses.begin(), mend = w.poses.end(); mit != mend; mit++) {
        KeyFrameSN *pKFi = mit->first;
        MapKR *pMap = pKFi->GetMap();
        Sophus::Sim3f Scw = mit->second;
        std::vector<MapPointSN *> vpReplacePoints(vpMapPoints.size(), static_cast<MapPointSN *>(NULL));
        int numFused = matcher.Fuse(pKFi, Scw, vpMapPoints, 4, vpReplacePoints);
        if (numFused < 0) return -1;
        total += numFused;
        std::unique_lock<std::mutex> lock(pMap->mMutexMapUpdate);
        const int nLP = vpMapPoints.size();
        for (int i = 0; i < nLP; i++) {
            MapPointSN *pRep = vpReplacePoints[i];
            if (pRep) pRep->Replace(vpMapPoints[i]);
        }
    }
    return total;
}

// LoopClosing.cc:2030-2065 as written
static int member_text_poses(World &w, const std::vector<KeyFrameSN *> &vConectedKFs) {
    rumi::LoopClosingStep matcher;
    std::vector<MapPointSN *> &vpMapPoints = w.loop;
    int total = 0;
    for (auto mit = vConectedKFs.begin(), mend = vConectedKFs.end(); mit != mend; mit++) {
        KeyFrameSN *pKF = (*mit);
        MapKR *pMap = pKF->GetMap();
        Sophus::SE3f Tcw = pKF->GetPose();
        Sim3fQ Scw(Tcw.unit_quaternion(), Tcw.translation());
        Scw.setScale(1.f);
        std::vector<MapPointSN *> vpReplacePoints(vpMapPoints.size(), static_cast<MapPointSN *>(NULL));
        int numFused = matcher.Fuse(pKF, Scw, vpMapPoints, 4, vpReplacePoints);
        if (numFused < 0) return -1;
        total += numFused;
        std::unique_lock<std::mutex> lock(pMap->mMutexMapUpdate);
        const int nLP = vpMapPoints.size();
        for (int i = 0; i < nLP; i++) {
            MapPointSN *pRep = vpReplacePoints[i];
            if (pRep) pRep->Replace(vpMapPoints[i]);
        }
    }
    return total;
}

static std::vector<KeyFrameSN *> connected(World &w) {
    std::vector<KeyFrameSN *> v;
    for (auto &e : w.poses) v.push_back(e.first);
    return v;
}

int main(int argc, char **argv) {
    if (argc < 2) { std::printf("usage: test_search_and_fuse_facade map.bin\n"); return 2; }
    int32_t h[8];
    World A, B;
    if (!load(argv[1], h, A) || !load(argv[1], h, B)) { std::printf("cannot read %s\n", argv[1]); return 2; }
    const int mode = h[7];

    using Graph = CovisibilityGraph<KeyFrameSN, MapPointSN>;
    Graph graph(h[0] + 4, h[1] + 64);
    if (!graph.ok()) return 3;
    for (int k = 0; k < h[0]; k++)
        if (k != h[5] && (graph.Sync(A.kfs[k].get()) != RUMI_OK || graph.SyncFeatures(A.kfs[k].get()) != RUMI_OK)) return 3;
    std::vector<MapPointSN *> all;
    for (int i = 0; i < h[1]; i++) {
        if (i == h[6]) continue;                                   // a loop point the graph never sees
        if (graph.Sync(A.mps[i].get()) != RUMI_OK) return 3;
        all.push_back(A.mps[i].get());
    }
    if (graph.SyncAttributes(all) != RUMI_OK) return 3;
    A.map.hooks.keyframe = [&](KeyFrameKR *k) { graph.Sync(static_cast<KeyFrameSN *>(k)); };
    A.map.hooks.point = [&](MapPointKR *p) { graph.Sync(static_cast<MapPointSN *>(p)); };
    A.map.hooks.drop = [&](KeyFrameKR *k) { graph.DropFeatures(static_cast<KeyFrameSN *>(k)); };

    rumi::LoopClosingStep step;
    int again = -1, ret;
    rumi_facade::clear_status();
    if (mode == 1) ret = step.SearchAndFuseResident<Sim3fQ>(graph, connected(A), A.loop, &again);
    else if (mode == 2) {
        std::vector<std::pair<KeyFrameSN *, Sim3fQ>> many;
        for (int i = 0; i <= RUMI_FUSE_MAX_TARGETS; i++) many.push_back(A.poses[i % A.poses.size()]);
        ret = step.SearchAndFuseResident(graph, many, A.loop, &again);
    } else ret = step.SearchAndFuseResident(graph, A.poses, A.loop, &again);
    std::printf("F A %d %d %d\n", ret, rumi_facade::last_status(), again);
    if (ret >= 0) {                                                // a refused call: B stays as loaded, and A must equal it
        rumi_facade::clear_status();
        ret = mode == 1 ? member_text_poses(B, connected(B)) : member_text_sim3(B);
        std::printf("F B %d %d 0\n", ret, rumi_facade::last_status());
        // the store was kept current: a second call on the fused map finds what the member text's second pass finds
        rumi_facade::clear_status();
        ret = mode == 1 ? step.SearchAndFuseResident<Sim3fQ>(graph, connected(A), A.loop, &again) : step.SearchAndFuseResident(graph, A.poses, A.loop, &again);
        std::printf("G A %d %d %d\n", ret, rumi_facade::last_status(), again);
        rumi_facade::clear_status();
        ret = mode == 1 ? member_text_poses(B, connected(B)) : member_text_sim3(B);
        std::printf("G B %d %d 0\n", ret, rumi_facade::last_status());
    }
    print("A", A);
    print("B", B);
    return 0;
}
