// rumi_facade::RefreshMapPointsResident and the resident forms of the two LocalMapping loops (facade/MapPointRefresh.h) over a
// CovisibilityGraph and the mock data model of tests/cpp/mock_model_refresh_resident.h, against rumi_facade::RefreshMapPoints on a copy of the
// same map, on the GPU.  Reads a map written by tests/test_refresh_resident_facade_gpu.py (the format of test_refresh_facade.cc).
// Map A belongs to a graph (every key-frame with features and centre, every point with observers, attributes and reference) and takes the
// resident members; map B takes the block members.  The key-frames of a map lie in one array, so that both maps' std::map<KeyFrame*, ...>
// iterate a point's observations in the same order (by index) and the two sides must agree bit for bit.  Prints one line per check group:
//   E name n     n points compared equal (members read back from the mock points)
// and FAIL lines; the exit status is the number of failed checks.
#define RUMI_HAVE_SOPHUS 1
#include <cstdio>
#include <cstring>
#include <list>
#include <memory>
#include <vector>

#include "mock_sophus.h"

#include "CovisibilityGraph.h"
#include "MapPointRefresh.h"
#include "rumi_testhooks.h"

#include "mock_model_refresh_resident.h"

static int fails = 0;
#define CHECK(c, msg) do { if (!(c)) { std::printf("FAIL: %s (%s:%d)\n", msg, __FILE__, __LINE__); fails++; } } while (0)

template <class T> static bool rd(FILE *f, T *p, size_t n) { return n == 0 || std::fread(p, sizeof(T), n, f) == n; }

template <class KF, class MP> struct World {
    MapRR map;
    int nKf = 0;
    std::unique_ptr<KF[]> kf;                                      // nKf key-frames and one spare (the new key-frame of the loops), in address order
    std::vector<std::unique_ptr<MP>> mp;
};

template <class KF, class MP> static bool load(const char *path, World<KF, MP> &w) {
    FILE *f = std::fopen(path, "rb");
    if (!f) return false;
    int32_t h[2];
    if (!rd(f, h, 2)) return false;
    w.nKf = h[0];
    w.kf.reset(new KF[h[0] + 1]);
    for (int k = 0; k < h[0]; k++) {
        KF *kf = &w.kf[k];
        int32_t n, bad; float Ow[3], sf[8];
        if (!rd(f, &n, 1) || !rd(f, &bad, 1) || !rd(f, Ow, 3) || !rd(f, sf, 8)) return false;
        kf->N = n; kf->mnId = k; kf->bad = bad != 0; kf->Ow = Eigen::Vector3f(Ow[0], Ow[1], Ow[2]); kf->map = &w.map;
        kf->mvScaleFactors.assign(sf, sf + 8); kf->mnScaleLevels = 8;
        kf->mDescriptors.create(n > 0 ? n : 1, 32, CV_8U);
        std::vector<int32_t> oct(n);
        if (!rd(f, kf->mDescriptors.ptr(0), (size_t)n * 32) || !rd(f, oct.data(), n)) return false;
        kf->mvKeysUn.resize(n);
        for (int i = 0; i < n; i++) kf->mvKeysUn[i].octave = oct[i];
        kf->mvpMapPoints.assign(n, nullptr);
    }
    for (int i = 0; i < h[1]; i++) {
        std::unique_ptr<MP> p(new MP());
        float pos[3]; int32_t ref, nobs;
        if (!rd(f, pos, 3) || !rd(f, &ref, 1) || !rd(f, &nobs, 1)) return false;
        p->pos = Eigen::Vector3f(pos[0], pos[1], pos[2]); p->mpRefKF = &w.kf[ref]; p->nObs = 0; p->map = &w.map;
        std::vector<int32_t> o((size_t)nobs * 2);
        if (!rd(f, o.data(), o.size())) return false;
        for (int j = 0; j < nobs; j++) p->MapPoint::AddObservation(&w.kf[o[2 * j]], o[2 * j + 1]);
        p->mDescriptor.create(1, 32, CV_8U);
        std::memset(p->mDescriptor.ptr(0), 0xEE, 32);              // what a point keeps when the reference does not write
        p->mNormalVector = Eigen::Vector3f(7.f, 7.f, 7.f);
        w.mp.push_back(std::move(p));
    }
    std::fclose(f);
    return true;
}

static bool same_members(MapPointRF *a, MapPointRF *b) {
    return std::memcmp(a->mDescriptor.ptr(0), b->mDescriptor.ptr(0), 32) == 0 && std::memcmp(&a->mNormalVector, &b->mNormalVector, sizeof a->mNormalVector) == 0 &&
           std::memcmp(&a->mfMinDistance, &b->mfMinDistance, 4) == 0 && std::memcmp(&a->mfMaxDistance, &b->mfMaxDistance, 4) == 0 &&
           a->nSetDescriptor == b->nSetDescriptor && a->nSetNormal == b->nSetNormal && a->nSetRange == b->nSetRange;
}

using WorldA = World<KeyFrameRR, MapPointRR>;
using WorldB = World<KeyFrameRF, MapPointRF>;
using Graph = CovisibilityGraph<KeyFrameRR, MapPointRR>;

static int compare(const char *name, WorldA &A, WorldB &B) {
    int equal = 0;
    for (size_t i = 0; i < A.mp.size(); i++) equal += same_members(A.mp[i].get(), B.mp[i].get());
    std::printf("E %s %d\n", name, equal);
    return equal;
}

// The store's attribute records of every point of A, device copy and mirror, against the members of the mock points: what a SyncAttributes of
// these points would stage is what the store already holds.
static int records_current(Graph &graph, WorldA &A, int fromDevice) {
    std::vector<int32_t> ids;
    for (auto &p : A.mp) ids.push_back(graph.IdOf(p.get()));
    std::vector<uint8_t> rec(ids.size() * 64);
    if (rumi_hook_covis_read_attributes(graph.handle(), (int32_t)ids.size(), ids.data(), rec.data(), fromDevice) != RUMI_OK) return -1;
    int current = 0;
    for (size_t i = 0; i < A.mp.size(); i++) {
        MapPointRR *p = A.mp[i].get();
        float f[8] = {p->pos(0), p->pos(1), p->pos(2), p->mNormalVector(0), p->mNormalVector(1), p->mNormalVector(2), p->mfMinDistance, p->mfMaxDistance};
        current += std::memcmp(rec.data() + 64 * i, f, 32) == 0 && std::memcmp(rec.data() + 64 * i + 32, p->mDescriptor.ptr(0), 32) == 0;
    }
    return current;
}

int main(int argc, char **argv) {
    if (argc < 2) { std::printf("usage: test_refresh_resident_facade map.bin\n"); return 2; }
    WorldA A;
    WorldB B;
    if (!load(argv[1], A) || !load(argv[1], B)) { std::printf("cannot read %s\n", argv[1]); return 2; }
    const int nPts = (int)A.mp.size();

    Graph graph(A.nKf + 4, nPts + 4);
    if (!graph.ok()) return 3;
    std::vector<KeyFrameRR *> kfsA;
    std::vector<MapPointRR *> allA;
    std::vector<MapPointRF *> allB;
    for (int k = 0; k < A.nKf; k++) {
        kfsA.push_back(&A.kf[k]);
        if (graph.Sync(&A.kf[k]) != RUMI_OK || graph.SyncFeatures(&A.kf[k]) != RUMI_OK) return 3;
    }
    for (auto &p : A.mp) { allA.push_back(p.get()); if (graph.Sync(p.get()) != RUMI_OK) return 3; }
    for (auto &p : B.mp) allB.push_back(p.get());
    if (graph.SyncCentres(kfsA) != RUMI_OK || graph.SyncReferences(allA) != RUMI_OK || graph.SyncAttributes(allA) != RUMI_OK) return 3;

    // ---- every point, both modes, with a NULL and a bad point in the list
    MapPointRR goneA; goneA.bad = true; goneA.mpRefKF = &A.kf[0]; goneA.MapPoint::AddObservation(&A.kf[0], 0);
    MapPointRF goneB; goneB.bad = true; goneB.mpRefKF = &B.kf[0]; goneB.MapPoint::AddObservation(&B.kf[0], 0);
    std::vector<MapPointRR *> listA = allA; listA.push_back(nullptr); listA.push_back(&goneA); listA.push_back(allA[0]);     // a repeat: skipped
    std::vector<MapPointRF *> listB = allB; listB.push_back(nullptr); listB.push_back(&goneB);
    const int nA = rumi_facade::RefreshMapPointsResident(graph, listA), nB = rumi_facade::RefreshMapPoints(listB);
    CHECK(nA == nPts && nB == nPts, "every live point was refreshed on both sides");
    CHECK(goneA.nSetDescriptor + goneA.nSetNormal + goneA.nSetRange == 0, "a bad point is left alone");
    CHECK(compare("all", A, B) == nPts, "the members after the resident refresh equal those after the block refresh");
    int written = 0;
    for (auto &p : A.mp) written += p->nSetDescriptor;
    CHECK(written > nPts / 2, "most points got a descriptor");
    // a later TrackLocalMapResident reads these records: they are current without a SyncAttributes
    CHECK(graph.DirtyCount() == 0, "nothing is waiting for a SyncAttributes");
    CHECK(records_current(graph, A, 1) == nPts, "the device's attribute records hold the refreshed members");
    CHECK(records_current(graph, A, 0) == nPts, "the mirror's attribute records hold the refreshed members");

    // ---- one mode only
    {
        const int d0 = allA[1]->nSetDescriptor, n0 = allA[1]->nSetNormal;
        CHECK(rumi_facade::RefreshMapPointsResident(graph, std::vector<MapPointRR *>{allA[1]}, RUMI_REFRESH_NORMAL_DEPTH) == 1, "normal and depth alone");
        CHECK(allA[1]->nSetDescriptor == d0 && allA[1]->nSetNormal == n0 + (allA[1]->obs.empty() ? 0 : 1), "only the members of the mode asked for are written");
        rumi_facade::RefreshMapPoints(std::vector<MapPointRF *>{allB[1]}, RUMI_REFRESH_NORMAL_DEPTH);
    }
    // ---- stereo observations are refused with a report, nothing written
    {
        MapPointRR *victim = nullptr;
        for (auto &p : A.mp) if (p->obs.size() >= 2) { victim = p.get(); break; }
        CHECK(victim != nullptr, "a point with two observations exists");
        if (victim) {
            std::vector<MapPointRR *> some{allA[0], victim};
            const int c0 = some[0]->nSetNormal + some[0]->nSetDescriptor, c1 = victim->nSetNormal + victim->nSetDescriptor;
            const int before = records_current(graph, A, 1);
            auto first = victim->obs.begin();
            const auto keep = first->second;
            first->second = std::make_tuple(std::get<0>(keep), 3);
            rumi_facade::clear_status();
            CHECK(rumi_facade::RefreshMapPointsResident(graph, some) == -1 && rumi_facade::last_status() == RUMI_E_INVALID, "a right index is refused and reported");
            first->second = keep;
            KeyFrameRR *k = static_cast<KeyFrameRR *>(first->first);
            k->NLeft = 100;
            rumi_facade::clear_status();
            CHECK(rumi_facade::RefreshMapPointsResident(graph, some) == -1 && rumi_facade::last_status() == RUMI_E_INVALID, "a key-frame with NLeft != -1 is refused and reported");
            k->NLeft = -1;
            CHECK(some[0]->nSetNormal + some[0]->nSetDescriptor == c0 && victim->nSetNormal + victim->nSetDescriptor == c1, "a refused call writes nothing to the points");
            CHECK(records_current(graph, A, 1) == before, "a refused call writes nothing to the store");
        }
    }
    // ---- ProcessNewKeyFrame :291-305 and SearchInNeighbors :730-739: a new key-frame (the spare, last in address order on both sides)
    {
        auto make = [](auto &W, auto *cur) {
            auto *src = &W.kf[0];
            cur->N = src->N; cur->mnId = W.nKf; cur->bad = false; cur->NLeft = -1; cur->map = &W.map;
            cur->Ow = Eigen::Vector3f(0.25f, -0.5f, 0.75f);
            cur->mvScaleFactors = src->mvScaleFactors; cur->mnScaleLevels = 8; cur->mvKeysUn = src->mvKeysUn;
            cur->mDescriptors = src->mDescriptors.clone();
            cur->mvpMapPoints.assign(cur->N, nullptr);
        };
        KeyFrameRR *curA = &A.kf[A.nKf];
        KeyFrameRF *curB = &B.kf[B.nKf];
        make(A, curA); make(B, curB);
        const int m = std::min<int>(curA->N, 40);
        int live = 0;
        for (int i = 0; i < m; i++) { curA->mvpMapPoints[i] = allA[i]; curB->mvpMapPoints[i] = allB[i]; live += !allA[i]->bad; }
        allA[0]->AddObservation(curA, 0); allB[0]->AddObservation(curB, 0);      // already associated: goes to the recent list (:299-302)
        // what the mutators' hooks do: the new key-frame enters the graph, the point that changed is staged
        CHECK(graph.Sync(curA) == RUMI_OK && graph.SyncFeatures(curA) == RUMI_OK && graph.SyncCentres(std::vector<KeyFrameRR *>{curA}) == RUMI_OK &&
              graph.Sync(allA[0]) == RUMI_OK, "the new key-frame and the changed point are staged");
        std::list<MapPointRR *> recentA;
        std::list<MapPointRF *> recentB;
        const int gotA = rumi_facade::AssociateAndRefreshResident(graph, curA, recentA), gotB = rumi_facade::AssociateAndRefresh(curB, recentB);
        CHECK(gotA == live - 1 && gotA == gotB && recentA.size() == 1 && recentA.front() == allA[0], "AssociateAndRefreshResident adds the observations and refreshes those points once");
        for (int i = 1; i < m; i++) CHECK(allA[i]->IsInKeyFrame(curA), "an associated point observes the key-frame");
        CHECK(compare("associate", A, B) == nPts, "the association loop leaves the same members on both sides");
        const int kA = rumi_facade::RefreshKeyFramePointsResident(graph, curA), kB = rumi_facade::RefreshKeyFramePoints(curB);
        CHECK(kA == live && kA == kB, "RefreshKeyFramePointsResident refreshes every live point of the key-frame");
        CHECK(compare("keyframe", A, B) == nPts, "the update loop leaves the same members on both sides");
        CHECK(records_current(graph, A, 1) == nPts && records_current(graph, A, 0) == nPts, "the store's records are current after both loops");
    }
    if (fails) std::printf("%d checks failed\n", fails);
    return fails;
}
