// LocalMappingStep::SearchInNeighborsResident (facade/LocalMappingStep.h) over a CovisibilityGraph and the mock data model of
// tests/cpp/mock_model_search_in_neighbors.h, against the reference's member text (LocalMapping.cc:649-743) over the merged
// rumi_facade::ORBmatcher::Fuse -- one call per target, then the reverse call -- on a copy of the same map, on the GPU.  Reads a map written by
// tests/test_search_in_neighbors_facade_gpu.py.  Map A belongs to a graph (every key-frame and point staged, features and attributes) and takes
// the resident member; map B takes the member text.  Then both take KeyFrameCulling (A by slot, B the block member): A's on-device
// consistency check passes only if the replay kept the store current.  Prints
//   T map nTargets                         F map ret status searchedAgain contradictions        C map ret status (the culling)
//   K map k bad parent | row...            V map k (kf weight)...   the ordered covisibles
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
#include "LocalMappingStep.h"

#include "mock_model_search_in_neighbors.h"

template <class T> static bool rd(FILE *f, T *p, size_t n) { return n == 0 || std::fread(p, sizeof(T), n, f) == n; }

struct World {
    MapKR map;
    std::vector<std::unique_ptr<KeyFrameSN>> kfs;
    std::vector<std::unique_ptr<MapPointSN>> mps;
};

static bool load(const char *path, int32_t *h, World &w) {
    FILE *f = std::fopen(path, "rb");
    if (!f) return false;
    if (!rd(f, h, 8)) return false;                                // n_kf n_pts abort inertial nleftKf unsyncedKf - -
    for (int k = 0; k < h[0]; k++) {
        std::unique_ptr<KeyFrameSN> kf(new KeyFrameSN());
        int32_t n, ncov;
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
        if (!rd(f, &ncov, 1)) return false;
        std::vector<int32_t> cov(ncov);
        if (!rd(f, cov.data(), ncov)) return false;
        for (int32_t c : cov) kf->mvOrderedWeights.push_back(-c - 1);   // indices for now, resolved below
        w.kfs.push_back(std::move(kf));
        for (int i = 0; i < n; i++) w.kfs.back()->mvpMapPoints[i] = reinterpret_cast<MapPoint *>((intptr_t)(row[i] + 1));   // ids for now
    }
    for (auto &kf : w.kfs) {                                       // the covisible lists as written: weights 100, 99, ...
        std::vector<int> idx = kf->mvOrderedWeights;
        kf->mvOrderedWeights.clear();
        for (size_t i = 0; i < idx.size(); i++) {
            KeyFrameSN *o = w.kfs[-idx[i] - 1].get();
            kf->mvpOrderedConnectedKeyFrames.push_back(o); kf->mvOrderedWeights.push_back(100 - (int)i); kf->mConnectedKeyFrameWeights[o] = 100 - (int)i;
        }
        if (!idx.empty()) kf->mbFirstConnection = false;
    }
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
    return true;
}

static void print(const char *tag, World &w) {
    std::map<const void *, int> pi, ki;
    for (size_t i = 0; i < w.mps.size(); i++) pi[w.mps[i].get()] = (int)i;
    for (size_t k = 0; k < w.kfs.size(); k++) ki[w.kfs[k].get()] = (int)k;
    for (size_t k = 0; k < w.kfs.size(); k++) {
        KeyFrameSN *kf = w.kfs[k].get();
        std::printf("K %s %zu %d %d |", tag, k, (int)kf->bad, kf->mpParent ? ki[kf->mpParent] : -1);
        for (MapPoint *p : kf->mvpMapPoints) std::printf(" %d", p ? pi[p] : -1);
        std::printf("\nV %s %zu", tag, k);
        for (size_t i = 0; i < kf->mvpOrderedConnectedKeyFrames.size(); i++) std::printf(" %d %d", ki[kf->mvpOrderedConnectedKeyFrames[i]], kf->mvOrderedWeights[i]);
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

// LocalMapping.cc:649-743 as written, over the facade's Fuse and the merged replacements of its last two steps
static int member_text(rumi::LocalMappingStep &matcher, KeyFrameSN *mpCurrentKeyFrame, bool mbMonocular, const volatile bool &mbAbortBA, int *nTargets) {
    int nn = 10;
    if (mbMonocular) nn = 30;
    const std::vector<KeyFrameSN *> vpNeighKFs = mpCurrentKeyFrame->GetBestCovisibilityKeyFrames(nn);
    std::vector<KeyFrameSN *> vpTargetKFs;
    for (KeyFrameSN *pKFi : vpNeighKFs) {
        if (pKFi->isBad() || pKFi->mnFuseTargetForKF == mpCurrentKeyFrame->mnId) continue;
        vpTargetKFs.push_back(pKFi);
        pKFi->mnFuseTargetForKF = mpCurrentKeyFrame->mnId;
    }
    for (int i = 0, imax = vpTargetKFs.size(); i < imax; i++) {
        const std::vector<KeyFrameSN *> vpSecondNeighKFs = vpTargetKFs[i]->GetBestCovisibilityKeyFrames(20);
        for (KeyFrameSN *pKFi2 : vpSecondNeighKFs) {
            if (pKFi2->isBad() || pKFi2->mnFuseTargetForKF == mpCurrentKeyFrame->mnId || pKFi2->mnId == mpCurrentKeyFrame->mnId) continue;
            vpTargetKFs.push_back(pKFi2);
            pKFi2->mnFuseTargetForKF = mpCurrentKeyFrame->mnId;
        }
        if (mbAbortBA) break;
    }
    *nTargets = (int)vpTargetKFs.size();
    int nFused = 0;
    std::vector<MapPointSN *> vpMapPointMatches = mpCurrentKeyFrame->GetMapPointMatches();
    for (KeyFrameSN *pKFi : vpTargetKFs) nFused += matcher.Fuse(pKFi, vpMapPointMatches);
    if (mbAbortBA) return nFused;
    std::vector<MapPointSN *> vpFuseCandidates;
    for (KeyFrameSN *pKFi : vpTargetKFs)
        for (MapPointSN *pMP : pKFi->GetMapPointMatches()) {
            if (!pMP) continue;
            if (pMP->isBad() || pMP->mnFuseCandidateForKF == mpCurrentKeyFrame->mnId) continue;
            pMP->mnFuseCandidateForKF = mpCurrentKeyFrame->mnId;
            vpFuseCandidates.push_back(pMP);
        }
    nFused += matcher.Fuse(mpCurrentKeyFrame, vpFuseCandidates);
    rumi_facade::RefreshKeyFramePoints(mpCurrentKeyFrame);
    mpCurrentKeyFrame->UpdateConnections();
    return nFused;
}

int main(int argc, char **argv) {
    if (argc < 2) { std::printf("usage: test_search_in_neighbors_facade map.bin\n"); return 2; }
    int32_t h[8];
    World A, B;
    if (!load(argv[1], h, A) || !load(argv[1], h, B)) { std::printf("cannot read %s\n", argv[1]); return 2; }
    volatile bool abortBA = h[2] != 0;
    const bool inertial = h[3] != 0;

    using Graph = CovisibilityGraph<KeyFrameSN, MapPointSN>;
    Graph graph(h[0] + 4, h[1] + 64);
    if (!graph.ok()) return 3;
    for (int k = 0; k < h[0]; k++)
        if (k != h[5] && (graph.Sync(A.kfs[k].get()) != RUMI_OK || graph.SyncFeatures(A.kfs[k].get()) != RUMI_OK)) return 3;
    std::vector<MapPointSN *> all;
    for (auto &p : A.mps) { if (graph.Sync(p.get()) != RUMI_OK) return 3; all.push_back(p.get()); }
    if (graph.SyncAttributes(all) != RUMI_OK) return 3;
    A.map.hooks.keyframe = [&](KeyFrameKR *k) { graph.Sync(static_cast<KeyFrameSN *>(k)); };
    A.map.hooks.point = [&](MapPointKR *p) { graph.Sync(static_cast<MapPointSN *>(p)); };
    A.map.hooks.drop = [&](KeyFrameKR *k) { graph.DropFeatures(static_cast<KeyFrameSN *>(k)); };

    rumi::LocalMappingStep step;
    int again = 0, contra = 0, nTargets = 0;
    rumi_facade::clear_status();
    int ret = step.SearchInNeighborsResident<MapPointSN>(graph, A.kfs[0].get(), true, inertial, abortBA, &again, &contra);
    std::printf("F A %d %d %d %d\n", ret, rumi_facade::last_status(), again, contra);
    int stamped = 0;
    for (auto &k : A.kfs) stamped += k->mnFuseTargetForKF == A.kfs[0]->mnId;
    std::printf("T A %d\n", stamped);
    if (ret >= 0) {                                                // a refused call: B stays as loaded, and A must equal it
        rumi_facade::clear_status();
        ret = member_text(step, B.kfs[0].get(), true, abortBA, &nTargets);
        std::printf("F B %d %d 0 0\nT B %d\n", ret, rumi_facade::last_status(), nTargets);
        rumi_facade::clear_status();
        ret = step.KeyFrameCullingResident(graph, A.kfs[0].get(), false, true, false);
        std::printf("C A %d %d\n", ret, rumi_facade::last_status());
        rumi_facade::clear_status();
        ret = step.KeyFrameCulling(B.kfs[0].get(), false, true, false);
        std::printf("C B %d %d\n", ret, rumi_facade::last_status());
    }
    print("A", A);
    print("B", B);
    return 0;
}
