// rumi_facade::RefreshMapPoints (facade/MapPointRefresh.h) over the mock data model of tests/cpp/mock_model_refresh.h, on the GPU.  Reads a map
// written by tests/test_refresh_facade_gpu.py (key-frames: descriptors, octaves, camera centre, bad flag; points: position, reference
// key-frame, observations), builds mock objects, refreshes every point in one call and prints, per point,
//   P i  n kf...  desc[32] normal[3] min max  nSetDescriptor nSetNormal nSetRange
// where kf... is the order in which THIS process's std::map<KeyFrame*, ...> iterates the point's observations (pointer order), so that the
// Python side can hand the oracle the lists in the same order; the members are read back from the mock objects.  Then the refusals and the two
// LocalMapping members.
// `test_refresh_facade newpoints scene.bin` (a scene of tests/test_newpoints_facade_gpu.py): LocalMappingStep::CreateNewMapPoints with a
// deferRefresh list, then one RefreshMapPoints over it; prints
//   K k Ow[3]                                                   the camera centre the mock key-frame reports
//   N neigh idx1 idx2 curFirst pos[3] desc[32] normal[3] min max   every created point (curFirst: the current key-frame is first in its map)
#define RUMI_HAVE_SOPHUS 1
#include <cstdio>
#include <cstring>
#include <list>
#include <memory>
#include <vector>

#include "mock_sophus.h"

#include "LocalMappingStep.h"
#include "MapPointRefresh.h"

#include "mock_model_refresh.h"

static int fails = 0;
#define CHECK(c, msg) do { if (!(c)) { std::printf("FAIL: %s (%s:%d)\n", msg, __FILE__, __LINE__); fails++; } } while (0)

template <class T> static bool rd(FILE *f, T *p, size_t n) { return n == 0 || std::fread(p, sizeof(T), n, f) == n; }
static void hex(float v) { uint32_t u; std::memcpy(&u, &v, 4); std::printf(" %08x", u); }

struct World {
    std::vector<std::unique_ptr<KeyFrameRF>> kf;
    std::vector<std::unique_ptr<MapPointRF>> mp;
};

static bool load(const char *path, World &w) {
    FILE *f = std::fopen(path, "rb");
    if (!f) return false;
    int32_t h[2];
    if (!rd(f, h, 2)) return false;
    for (int k = 0; k < h[0]; k++) {
        std::unique_ptr<KeyFrameRF> kf(new KeyFrameRF());
        int32_t n, bad; float Ow[3], sf[8];
        if (!rd(f, &n, 1) || !rd(f, &bad, 1) || !rd(f, Ow, 3) || !rd(f, sf, 8)) return false;
        kf->N = n; kf->mnId = k; kf->bad = bad != 0; kf->Ow = Eigen::Vector3f(Ow[0], Ow[1], Ow[2]);
        kf->mvScaleFactors.assign(sf, sf + 8); kf->mnScaleLevels = 8;
        kf->mDescriptors.create(n > 0 ? n : 1, 32, CV_8U);
        std::vector<int32_t> oct(n);
        if (!rd(f, kf->mDescriptors.ptr(0), (size_t)n * 32) || !rd(f, oct.data(), n)) return false;
        kf->mvKeysUn.resize(n);
        for (int i = 0; i < n; i++) kf->mvKeysUn[i].octave = oct[i];
        kf->mvpMapPoints.assign(n, nullptr);
        w.kf.push_back(std::move(kf));
    }
    for (int i = 0; i < h[1]; i++) {
        std::unique_ptr<MapPointRF> p(new MapPointRF());
        float pos[3]; int32_t ref, nobs;
        if (!rd(f, pos, 3) || !rd(f, &ref, 1) || !rd(f, &nobs, 1)) return false;
        p->pos = Eigen::Vector3f(pos[0], pos[1], pos[2]); p->mpRefKF = w.kf[ref].get(); p->nObs = 0;
        std::vector<int32_t> o((size_t)nobs * 2);
        if (!rd(f, o.data(), o.size())) return false;
        for (int j = 0; j < nobs; j++) p->AddObservation(w.kf[o[2 * j]].get(), o[2 * j + 1]);
        p->mDescriptor.create(1, 32, CV_8U);
        std::memset(p->mDescriptor.ptr(0), 0xEE, 32);              // what a point keeps when the reference does not write
        p->mNormalVector = Eigen::Vector3f(7.f, 7.f, 7.f);
        w.mp.push_back(std::move(p));
    }
    std::fclose(f);
    return true;
}

// ---- CreateNewMapPoints with the refresh deferred ----
struct MapPointNP : MapPointRF {                                   // what CreateNewMapPoints constructs (MapPoint.cc:40-58)
    int nDistinctive = 0, nNormalDepth = 0;
    MapPointNP(const Eigen::Vector3f &Pos, KeyFrameRF *pRefKF, Map *pMap) { pos = Pos; mpRefKF = pRefKF; map = pMap; nObs = 0; }
    void ComputeDistinctiveDescriptors() { nDistinctive++; }
    void UpdateNormalAndDepth() { nNormalDepth++; }
};
struct AtlasRF {
    Map current;
    std::vector<MapPoint *> added;
    Map *GetCurrentMap() { return &current; }
    void AddMapPoint(MapPoint *p) { added.push_back(p); }
};

static int newpoints(const char *path) {
    FILE *f = std::fopen(path, "rb");
    if (!f) { std::printf("cannot read %s\n", path); return 2; }
    int32_t h[4]; float thFar;
    if (!rd(f, h, 4) || !rd(f, &thFar, 1)) return 2;
    std::vector<std::unique_ptr<KeyFrameRF>> kfs;
    std::vector<std::unique_ptr<MapPointRF>> old;
    for (int k = 0; k < h[0]; k++) {
        std::unique_ptr<KeyFrameRF> kf(new KeyFrameRF());
        int32_t n, nn;
        if (!rd(f, &n, 1)) return 2;
        kf->N = n; kf->mnId = k;
        kf->mvKeysUn.resize(n); kf->mDescriptors.create(n > 0 ? n : 1, 32, CV_8U);
        std::vector<int32_t> mp(n); std::vector<float> pos((size_t)n * 3); float R[9], t[3];
        if (!rd(f, kf->mvKeysUn.data(), n) || !rd(f, kf->mDescriptors.ptr(0), (size_t)n * 32) || !rd(f, mp.data(), n) || !rd(f, pos.data(), (size_t)n * 3) ||
            !rd(f, R, 9) || !rd(f, t, 3) || !rd(f, &nn, 1)) return 2;
        std::vector<uint32_t> nodes(nn); std::vector<int32_t> off(nn + 1);
        if (!rd(f, nodes.data(), nn) || !rd(f, off.data(), nn + 1)) return 2;
        std::vector<uint32_t> idx(off[nn]);
        if (!rd(f, idx.data(), idx.size())) return 2;
        for (int a = 0; a < nn; a++) kf->mFeatVec[nodes[a]] = std::vector<unsigned>(idx.begin() + off[a], idx.begin() + off[a + 1]);
        kf->mvScaleFactors.resize(8); kf->mvLevelSigma2.resize(8);
        if (!rd(f, kf->mvScaleFactors.data(), 8)) return 2;
        for (int l = 0; l < 8; l++) kf->mvLevelSigma2[l] = kf->mvScaleFactors[l] * kf->mvScaleFactors[l];
        kf->mvuRight.assign(n, -1.f);
        kf->mvpMapPoints.assign(n, nullptr);
        for (int i = 0; i < n; i++)
            if (mp[i] >= 0) {
                old.emplace_back(new MapPointRF());
                old.back()->pos = Eigen::Vector3f(pos[3 * i], pos[3 * i + 1], pos[3 * i + 2]);
                kf->mvpMapPoints[i] = old.back().get();
            }
        Eigen::Matrix3f Rm;
        for (int r = 0; r < 3; r++) for (int c = 0; c < 3; c++) Rm(r, c) = R[r * 3 + c];
        kf->SetPose(Sophus::SE3f(Rm, Eigen::Vector3f(t[0], t[1], t[2])));
        kf->Ow = kf->GetPose().inverse().translation();
        std::printf("K %d", k); hex(kf->Ow(0)); hex(kf->Ow(1)); hex(kf->Ow(2)); std::printf("\n");
        kfs.push_back(std::move(kf));
    }
    std::fclose(f);
    KeyFrameRF *cur = kfs[0].get();
    std::vector<KeyFrameRF *> neigh;
    for (size_t k = 1; k < kfs.size(); k++) neigh.push_back(kfs[k].get());
    rumi::LocalMappingStep step(h[2] != 0);
    AtlasRF atlas;
    std::list<MapPoint *> recent;
    std::vector<MapPointNP *> created;
    const int n = step.CreateNewMapPoints<MapPointNP>(cur, neigh, &atlas, recent, h[3] != 0, thFar, [] { return false; }, h[1] != 0, &created);
    CHECK(n > 0 && n == (int)created.size() && n == (int)recent.size(), "the deferred list holds every created point");
    for (MapPointNP *p : created) CHECK(p->nDistinctive == 0 && p->nNormalDepth == 0 && p->nSetDescriptor == 0, "the per-point members were not called");
    CHECK(rumi_facade::RefreshMapPoints(created) == n, "one refresh over the deferred list");
    for (MapPointNP *p : created) {
        CHECK(p->obs.size() == 2 && p->nSetDescriptor == 1 && p->nSetNormal == 1 && p->nSetRange == 1, "each point written once");
        int kn = -1, idx2 = -1;
        for (auto &o : p->obs) if (o.first != cur) { kn = (int)o.first->mnId - 1; idx2 = std::get<0>(o.second); }
        std::printf("N %d %d %d %d", kn, std::get<0>(p->obs[cur]), idx2, (int)(p->obs.begin()->first == cur));
        hex(p->pos(0)); hex(p->pos(1)); hex(p->pos(2));
        for (int b = 0; b < 32; b++) std::printf(" %02x", p->mDescriptor.ptr(0)[b]);
        hex(p->mNormalVector(0)); hex(p->mNormalVector(1)); hex(p->mNormalVector(2)); hex(p->mfMinDistance); hex(p->mfMaxDistance);
        std::printf("\n");
    }
    for (MapPointNP *p : created) delete p;
    if (fails) { std::printf("%d checks failed\n", fails); return 1; }
    return 0;
}

int main(int argc, char **argv) {
    if (argc < 2) { std::printf("usage: test_refresh_facade map.bin | newpoints scene.bin\n"); return 2; }
    if (argc >= 3 && std::strcmp(argv[1], "newpoints") == 0) return newpoints(argv[2]);
    World w;
    if (!load(argv[1], w)) { std::printf("cannot read %s\n", argv[1]); return 2; }
    std::vector<MapPointRF *> all;
    for (auto &p : w.mp) all.push_back(p.get());
    all.push_back(nullptr);                                        // skipped
    MapPointRF gone; gone.bad = true; gone.mpRefKF = w.kf[0].get(); gone.AddObservation(w.kf[0].get(), 0);
    all.push_back(&gone);                                          // isBad(): skipped, untouched
    const int n = rumi_facade::RefreshMapPoints(all);
    CHECK(n == (int)w.mp.size(), "every live point was refreshed");
    CHECK(gone.nSetDescriptor + gone.nSetNormal + gone.nSetRange == 0, "a bad point is left alone");
    for (size_t i = 0; i < w.mp.size(); i++) {
        MapPointRF *p = w.mp[i].get();
        const auto obs = p->GetObservations();
        std::printf("P %zu %zu", i, obs.size());
        for (auto &o : obs) std::printf(" %ld", o.first->mnId);
        for (int b = 0; b < 32; b++) std::printf(" %02x", p->mDescriptor.ptr(0)[b]);
        hex(p->mNormalVector(0)); hex(p->mNormalVector(1)); hex(p->mNormalVector(2)); hex(p->mfMinDistance); hex(p->mfMaxDistance);
        std::printf(" %d %d %d\n", p->nSetDescriptor, p->nSetNormal, p->nSetRange);
    }

    // one mode only
    {
        MapPointRF *p = w.mp[0].get();
        const int before = p->nSetDescriptor, beforeN = p->nSetNormal;
        CHECK(rumi_facade::RefreshMapPoints(std::vector<MapPointRF *>{p}, RUMI_REFRESH_NORMAL_DEPTH) == 1, "normal and depth alone");
        CHECK(p->nSetDescriptor == before && p->nSetNormal == beforeN + (p->obs.empty() ? 0 : 1), "only the members of the mode asked for are written");
    }
    // stereo observations are refused with a report, nothing written
    {
        MapPointRF *victim = nullptr;
        for (auto &p : w.mp) if (p->obs.size() >= 2) { victim = p.get(); break; }
        CHECK(victim != nullptr, "a point with two observations exists");
        if (victim) {
            std::vector<MapPointRF *> some{w.mp[0].get(), victim};
            const int c0 = some[0]->nSetNormal + some[0]->nSetDescriptor, c1 = victim->nSetNormal + victim->nSetDescriptor;
            auto first = victim->obs.begin();
            const auto keep = first->second;
            first->second = std::make_tuple(std::get<0>(keep), 3);
            rumi_facade::clear_status();
            CHECK(rumi_facade::RefreshMapPoints(some) == -1 && rumi_facade::last_status() == RUMI_E_INVALID, "a right index is refused and reported");
            first->second = keep;
            KeyFrameRF *k = static_cast<KeyFrameRF *>(first->first);
            k->NLeft = 100;
            rumi_facade::clear_status();
            CHECK(rumi_facade::RefreshMapPoints(some) == -1 && rumi_facade::last_status() == RUMI_E_INVALID, "a key-frame with NLeft != -1 is refused and reported");
            k->NLeft = -1;
            CHECK(some[0]->nSetNormal + some[0]->nSetDescriptor == c0 && victim->nSetNormal + victim->nSetDescriptor == c1, "a refused call writes nothing");
        }
    }
    // LocalMapping::ProcessNewKeyFrame :291-305 and SearchInNeighbors :730-739: a new key-frame whose slots hold the first points of the map
    {
        KeyFrameRF *src = w.kf[0].get();
        std::unique_ptr<KeyFrameRF> cur(new KeyFrameRF(*src));
        cur->mnId = (long)w.kf.size(); cur->bad = false; cur->NLeft = -1; cur->Ow = Eigen::Vector3f(0.25f, -0.5f, 0.75f);
        cur->mDescriptors = src->mDescriptors.clone();
        const int m = std::min<int>(cur->N, 40);
        int live = 0;
        for (int i = 0; i < m; i++) { cur->mvpMapPoints[i] = w.mp[i].get(); live += !w.mp[i]->bad; }
        cur->mvpMapPoints[0]->AddObservation(cur.get(), 0);     // already associated: goes to the recent list instead (:299-302)
        std::vector<int> before;
        for (int i = 0; i < m; i++) before.push_back(w.mp[i]->nSetNormal);
        std::list<MapPointRF *> recent;
        const int got = rumi_facade::AssociateAndRefresh(cur.get(), recent);
        CHECK(got == live - 1 && recent.size() == 1 && recent.front() == w.mp[0].get(), "AssociateAndRefresh adds the observations and refreshes those points once");
        for (int i = 1; i < m; i++)
            CHECK(w.mp[i]->IsInKeyFrame(cur.get()) && w.mp[i]->nSetNormal == before[i] + 1, "an associated point observes the key-frame and was refreshed");
        CHECK(rumi_facade::RefreshKeyFramePoints(cur.get()) == live, "RefreshKeyFramePoints refreshes every live point of the key-frame");
        for (int i = 0; i < m; i++) w.mp[i]->EraseObservation(cur.get());
    }
    if (fails) { std::printf("%d checks failed\n", fails); return 1; }
    return 0;
}
