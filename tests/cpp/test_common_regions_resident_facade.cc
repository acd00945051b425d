// rumi_facade::CommonRegionsBoWStageResident (facade/LoopClosingStep.h) on the GPU, two modes.
//
//   lc scene.bin unsynced   the mock key-frames of tests/cpp/mock_model_loopclosing.h (the scene file of tests/cpp/test_common_regions_facade.cc)
//                           in a synced graph.  KeyFrameLC has no GetMap / GetParent / GetObservations, so the graph is GraphLC below: the members
//                           the stage reads of CovisibilityGraph (ok, SlotOf, HasFeatures, FlushDirty, handle, PointAt) over the same C entries
//                           CovisibilityGraph::Sync and SyncFeatures call.  Runs CommonRegionsBoWStage by host pointers and the by-slot stage with
//                           and without member matches, compares field by field of BowStageResult and prints
//                             E with equal|DIFFERENT <what>      E without equal|DIFFERENT <what>
//                           then the by-slot result (with member matches) in test_common_regions_facade.cc's format: R C V M P K.
//                           unsynced >= 0: that key-frame gets no SyncFeatures; only "R ret status n_results" of the by-slot stage is printed.
//   lc scene.bin -1 repeats rounds
//                           for tools/common_regions_probe.py: after the comparison, the two stages (by slot without member matches) alternate
//                           call by call; "T pointer|slot <the median wall time in ms of each round>"; nothing else is printed.
//   pr map.bin nBoWMatches nBoWInliers nSim3Inliers nProjMatches nProjOptMatches unsynced
//                           the map of tests/test_place_recognition_facade_gpu.py twice (sim3_projection_world.h).  Graph B lacks the features
//                           of key-frame `unsynced`, graph A holds all: LoopClosingStep::DetectCommonRegionsFromBoWResident on both.  Prints
//                             S side rc      rumi_common_regions_bow_resident_stage_ms after the side's call (B runs first, on a fresh arena:
//                                            -1 there says no by-slot call was made, 0 after A that one was)
//                             D side ...     the outputs, as test_place_recognition_facade.cc prints them
//                           then, over graph A (the real CovisibilityGraph, two points marked dirty), CommonRegionsBoWStage against the by-slot
//                           stage with and without member matches: the two E lines of mode lc, and
//                             N ret n_results matched_points dirty_left
#define RUMI_HAVE_SOPHUS 1
#include <algorithm>
#include <chrono>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <set>
#include <string>
#include <vector>

#include "mock_sophus.h"

#include "CovisibilityGraph.h"
#include "LoopClosingStep.h"
#include "Optimizer.h"

#include "sim3_projection_world.h"
#include "mock_model_loopclosing.h"

// ---- lc ---------------------------------------------------------------------------------------------------------------------------------
struct GraphLC {
    RumiCovis *h = nullptr;
    std::map<KeyFrameLC *, int> slot;
    std::map<MapPointLC *, int> id;
    std::vector<MapPointLC *> pts;
    std::set<KeyFrameLC *> featured;
    GraphLC(int max_kf, int max_points) { if (rumi_covis_create(max_kf, max_points, 0, -1, &h) != RUMI_OK) h = nullptr; }
    ~GraphLC() { if (h) rumi_covis_destroy(h); }
    bool ok() const { return h != nullptr; }
    RumiCovis *handle() const { return h; }
    int SlotOf(KeyFrameLC *k) const { auto it = slot.find(k); return it == slot.end() ? -1 : it->second; }
    bool HasFeatures(KeyFrameLC *k) const { return featured.count(k) > 0; }
    int FlushDirty() { return RUMI_OK; }
    MapPointLC *PointAt(int i) const { return pts[i]; }
    // rows, bad bits and points of every key-frame, as CovisibilityGraph::Sync stages them
    int SyncAll(const std::vector<std::unique_ptr<KeyFrameLC>> &kfs) {
        std::vector<int32_t> slots, maps, mpOff{0}, mp, best, parent, chOff{0};
        std::vector<uint64_t> keys;
        std::vector<uint8_t> bad;
        for (const auto &k : kfs) {
            const int s = (int)slot.size();
            slot[k.get()] = s;
            slots.push_back(s); keys.push_back((uint64_t)(uintptr_t)k.get()); maps.push_back(0); bad.push_back(k->isBad() ? 1 : 0);
            for (MapPointLC *p : k->GetMapPointMatches()) {
                if (!p) { mp.push_back(-1); continue; }
                auto it = id.find(p);
                if (it == id.end()) { it = id.emplace(p, (int)pts.size()).first; pts.push_back(p); }
                mp.push_back(it->second);
            }
            mpOff.push_back((int32_t)mp.size());
            for (int j = 0; j < RUMI_COVIS_NBEST; j++) best.push_back(-1);
            parent.push_back(-1); chOff.push_back(0);
        }
        int32_t none = 0;
        int rc = rumi_covis_set_keyframes(h, (int32_t)slots.size(), slots.data(), keys.data(), maps.data(), bad.data(), mpOff.data(), mp.empty() ? &none : mp.data(),
                                          best.data(), parent.data(), chOff.data(), &none);
        if (rc != RUMI_OK || pts.empty()) return rc;
        std::vector<int32_t> ids, off(pts.size() + 1, 0);
        std::vector<uint8_t> pbad;
        for (size_t i = 0; i < pts.size(); i++) { ids.push_back((int32_t)i); pbad.push_back(pts[i]->isBad() ? 1 : 0); }
        return rumi_covis_set_points(h, (int32_t)ids.size(), ids.data(), pbad.data(), off.data(), &none);
    }
    int SyncFeatures(KeyFrameLC *k) {
        RumiFrameFeatures f;
        f.n = k->N;
        f.keys_un = reinterpret_cast<const RumiKeyPoint *>(k->mvKeysUn.data());
        f.desc = k->mDescriptors.ptr(0);
        f.min_x = k->mnMinX; f.min_y = k->mnMinY; f.max_x = k->mnMaxX; f.max_y = k->mnMaxY;
        f.scale_factors = k->mvScaleFactors.data();
        f.nlevels = (int32_t)k->mvScaleFactors.size();
        std::vector<uint32_t> nodes, idx;
        std::vector<int32_t> off{0};
        for (const auto &kv : k->mFeatVec) {
            nodes.push_back((uint32_t)kv.first);
            for (unsigned i : kv.second) idx.push_back(i);
            off.push_back((int32_t)idx.size());
        }
        const RumiFeatureVector fv{(int32_t)nodes.size(), nodes.data(), off.data(), idx.data()};
        const float K4[4] = {500.f, 500.f, 320.f, 240.f};
        const int rc = rumi_covis_set_keyframe_features(h, slot[k], &f, &fv, K4);
        if (rc == RUMI_OK) featured.insert(k);
        return rc;
    }
};

using ResultLC = rumi_facade::BowStageResult<KeyFrameLC, MapPointLC>;

template <class R> static std::string differ(const std::vector<R> &a, const std::vector<R> &b, bool members) {
    if (a.size() != b.size()) return "size";
    for (size_t g = 0; g < a.size(); g++) {
        const R &x = a[g], &y = b[g];
        if (x.pKFi != y.pKFi) return "pKFi";
        if (x.vpCovKFi != y.vpCovKFi) return "vpCovKFi";
        if (x.vpMatchedPoints != y.vpMatchedPoints) return "vpMatchedPoints";
        if (x.vpKeyFrameMatchedMP != y.vpKeyFrameMatchedMP) return "vpKeyFrameMatchedMP";
        if (x.numBoWMatches != y.numBoWMatches) return "numBoWMatches";
        if (x.nIndexMostBoWMatchesKF != y.nIndexMostBoWMatchesKF) return "nIndexMostBoWMatchesKF";
        if (x.nMostBoWNumMatches != y.nMostBoWNumMatches) return "nMostBoWNumMatches";
        if (x.vvpMatchedMPs.size() != y.vvpMatchedMPs.size()) return "vvpMatchedMPs.size";
        if (members) { if (x.vvpMatchedMPs != y.vvpMatchedMPs) return "vvpMatchedMPs"; }
        else for (const auto &v : y.vvpMatchedMPs) if (!v.empty()) return "vvpMatchedMPs filled without being asked for";
    }
    return "";
}

static int run_lc(int argc, char **argv) {
    if (argc < 4) return 2;
    FILE *f = std::fopen(argv[2], "rb");
    if (!f) { std::printf("cannot read %s\n", argv[2]); return 2; }
    const int unsynced = std::atoi(argv[3]);
    int32_t h[4], ori;
    float nnratio;
    if (!rd(f, h, 4) || !rd(f, &nnratio, 1) || !rd(f, &ori, 1)) return 2;
    std::vector<std::unique_ptr<MapPointLC>> mps;
    std::vector<uint8_t> bad(h[1]);
    if (!rd(f, bad.data(), bad.size())) return 2;
    for (int i = 0; i < h[1]; i++) { mps.emplace_back(new MapPointLC()); mps.back()->id = i; mps.back()->bad = bad[i] != 0; }
    std::vector<std::unique_ptr<KeyFrameLC>> kfs;
    std::vector<std::vector<int32_t>> cov(h[0]), conn(h[0]);
    for (int k = 0; k < h[0]; k++) {
        std::unique_ptr<KeyFrameLC> kf(new KeyFrameLC());
        int32_t v[6];
        if (!rd(f, v, 6)) return 2;
        kf->id = k; kf->N = v[0]; kf->bad = v[1] != 0; kf->NLeft = v[2];
        std::vector<float> angle(v[0]);
        std::vector<int32_t> mp(v[0]);
        kf->mDescriptors.create(v[0] > 0 ? v[0] : 1, 32, CV_8U);
        if (!rd(f, angle.data(), angle.size()) || !rd(f, kf->mDescriptors.ptr(0), (size_t)v[0] * 32) || !rd(f, mp.data(), mp.size())) return 2;
        kf->mvKeysUn.resize(v[0]); kf->mvpMapPoints.assign(v[0], nullptr);
        for (int i = 0; i < v[0]; i++) { kf->mvKeysUn[i].angle = angle[i]; if (mp[i] >= 0) kf->mvpMapPoints[i] = mps[mp[i]].get(); }
        for (int a = 0; a < v[3]; a++) {
            int32_t node[2];
            if (!rd(f, node, 2)) return 2;
            std::vector<int32_t> idx(node[1]);
            if (!rd(f, idx.data(), idx.size())) return 2;
            std::vector<unsigned> &list = kf->mFeatVec[(unsigned)node[0]];
            for (int32_t i : idx) list.push_back((unsigned)i);
        }
        cov[k].resize(v[4]); conn[k].resize(v[5]);
        if (!rd(f, cov[k].data(), cov[k].size()) || !rd(f, conn[k].data(), conn[k].size())) return 2;
        kfs.push_back(std::move(kf));
    }
    for (int k = 0; k < h[0]; k++) {
        for (int32_t c : cov[k]) kfs[k]->covisibles.push_back(c < 0 ? nullptr : kfs[c].get());
        for (int32_t c : conn[k]) kfs[k]->connected.insert(kfs[c].get());
    }
    std::vector<int32_t> cand(h[2]);
    if (!rd(f, cand.data(), cand.size())) return 2;
    std::fclose(f);
    std::vector<KeyFrameLC *> vpBowCand;
    for (int32_t c : cand) vpBowCand.push_back(c < 0 ? nullptr : kfs[c].get());

    GraphLC graph(h[0] + 1, h[1] + 1);
    if (!graph.ok() || graph.SyncAll(kfs) != RUMI_OK) return 3;
    for (int k = 0; k < h[0]; k++)
        if (k != unsynced && graph.SyncFeatures(kfs[k].get()) != RUMI_OK) return 3;

    ORB_SLAM3::ORBmatcher matcherBoW(nnratio, ori != 0);
    const std::set<KeyFrameLC *> spConnectedKeyFrames = kfs[0]->GetConnectedKeyFrames();
    std::vector<ResultLC> byPointer, with, without;
    rumi_facade::clear_status();
    const int ret = rumi_facade::CommonRegionsBoWStageResident(graph, kfs[0].get(), vpBowCand, spConnectedKeyFrames, h[3], matcherBoW, with, true);
    const int status = rumi_facade::last_status();
    if (unsynced >= 0) { std::printf("R %d %d %zu\n", ret, status, with.size()); return 0; }
    const int retP = rumi_facade::CommonRegionsBoWStage(kfs[0].get(), vpBowCand, spConnectedKeyFrames, h[3], matcherBoW, byPointer);
    const int ret0 = rumi_facade::CommonRegionsBoWStageResident(graph, kfs[0].get(), vpBowCand, spConnectedKeyFrames, h[3], matcherBoW, without, false);
    std::string d = ret != retP ? "return value" : differ(byPointer, with, true);
    std::printf("E with %s %s\n", d.empty() ? "equal" : "DIFFERENT", d.c_str());
    d = ret0 != retP ? "return value" : differ(byPointer, without, false);
    std::printf("E without %s %s\n", d.empty() ? "equal" : "DIFFERENT", d.c_str());
    if (argc >= 6) {
        const int repeats = std::atoi(argv[4]), rounds = std::atoi(argv[5]);
        std::vector<double> medP, medS;
        auto ms = [](std::chrono::steady_clock::time_point a) { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - a).count(); };
        for (int r = 0; r < rounds; r++) {
            std::vector<double> tp, ts;
            for (int i = 0; i < repeats; i++) {
                auto t0 = std::chrono::steady_clock::now();
                rumi_facade::CommonRegionsBoWStage(kfs[0].get(), vpBowCand, spConnectedKeyFrames, h[3], matcherBoW, byPointer);
                tp.push_back(ms(t0));
                t0 = std::chrono::steady_clock::now();
                rumi_facade::CommonRegionsBoWStageResident(graph, kfs[0].get(), vpBowCand, spConnectedKeyFrames, h[3], matcherBoW, without, false);
                ts.push_back(ms(t0));
            }
            std::sort(tp.begin(), tp.end()); std::sort(ts.begin(), ts.end());
            medP.push_back(tp[tp.size() / 2]); medS.push_back(ts[ts.size() / 2]);
        }
        std::printf("T pointer"); for (double v : medP) std::printf(" %.4f", v);
        std::printf("\nT slot"); for (double v : medS) std::printf(" %.4f", v);
        std::printf("\n");
        return differ(byPointer, without, false).empty() ? 0 : 4;
    }
    std::printf("R %d %d %zu\n", ret, status, with.size());
    for (const auto &r : with) {
        const int c = r.pKFi->id;
        std::printf("C %d %d %d %d\nV %d", c, r.numBoWMatches, r.nIndexMostBoWMatchesKF, r.nMostBoWNumMatches, c);
        for (KeyFrameLC *k : r.vpCovKFi) std::printf(" %d", k ? k->id : -1);
        std::printf("\n");
        for (size_t j = 0; j < r.vvpMatchedMPs.size(); j++) {
            std::printf("M %d %zu", c, j);
            if (r.vvpMatchedMPs[j].empty()) std::printf(" empty");
            for (MapPointLC *p : r.vvpMatchedMPs[j]) std::printf(" %d", p ? p->id : -1);
            std::printf("\n");
        }
        std::printf("P %d", c);
        for (MapPointLC *p : r.vpMatchedPoints) std::printf(" %d", p ? p->id : -1);
        std::printf("\nK %d", c);
        for (KeyFrameLC *k : r.vpKeyFrameMatchedMP) std::printf(" %d", k ? k->id : -1);
        std::printf("\n");
    }
    return 0;
}

// ---- pr ---------------------------------------------------------------------------------------------------------------------------------
struct Outputs {
    KeyFrameSN *pMatchedKF2 = nullptr, *pLastCurrentKF = nullptr;
    g2o::Sim3 g2oScw;
    int nNumCoincidences = -7;
    std::vector<MapPointSN *> vpMPs, vpMatchedMPs;
};
static void show(const char *tag, World &w, int ret, Outputs &o, int next) {
    double S[8];
    ORB_SLAM3::Optimizer::sim3_to8(o.g2oScw, S);
    std::printf("D %s %d %d %d %d %d %d |", tag, ret, o.pMatchedKF2 ? w.ki[o.pMatchedKF2] : -1, o.nNumCoincidences, o.pMatchedKF2 ? (int)o.pMatchedKF2->mbNotErase : -1,
                o.pLastCurrentKF ? w.ki[o.pLastCurrentKF] : -1, next);
    for (double d : S) { uint64_t u; std::memcpy(&u, &d, 8); std::printf(" %016llx", (unsigned long long)u); }
    std::printf(" |");
    for (MapPointSN *p : o.vpMPs) std::printf(" %d", p ? w.pi[p] : -1);
    std::printf(" |");
    for (MapPointSN *p : o.vpMatchedMPs) std::printf(" %d", p ? w.pi[p] : -1);
    std::printf("\n");
}

static int run_pr(int argc, char **argv) {
    if (argc < 9) return 2;
    int32_t h[8];
    World A, B;
    if (!load(argv[2], h, A) || !load(argv[2], h, B)) { std::printf("cannot read %s\n", argv[2]); return 2; }
    rumi::LoopClosingStep::PlaceRecognitionThresholds th;
    th.nBoWMatches = std::atoi(argv[3]); th.nBoWInliers = std::atoi(argv[4]); th.nSim3Inliers = std::atoi(argv[5]); th.nProjMatches = std::atoi(argv[6]);
    th.nProjOptMatches = std::atoi(argv[7]);
    const int unsynced = std::atoi(argv[8]);
    using Graph = CovisibilityGraph<KeyFrameSN, MapPointSN>;
    Graph graphA(h[0] + 4, h[1] + 64), graphB(h[0] + 4, h[1] + 64);
    if (!graphA.ok() || !graphB.ok()) return 3;
    auto fill = [&](Graph &graph, World &W, int skip) {
        for (int k = 0; k < h[0]; k++)
            if (graph.Sync(W.kfs[k].get()) != RUMI_OK || (k != skip && graph.SyncFeatures(W.kfs[k].get()) != RUMI_OK)) return false;
        std::vector<MapPointSN *> all;
        for (int i = 0; i < h[1]; i++) {
            if (graph.Sync(W.mps[i].get()) != RUMI_OK) return false;
            all.push_back(W.mps[i].get());
        }
        return graph.SyncAttributes(all) == RUMI_OK;
    };
    if (!fill(graphA, A, -1) || !fill(graphB, B, unsynced)) return 3;
    if (!ORB_SLAM3::Optimizer::arena()) return 3;                        // the first device calls of the process, before either side seeds rand()
    { std::vector<MapPointSN *> v; ORB_SLAM3::ORBmatcher warm(0.9, true); warm.SearchByBoW(B.cur, B.cand.back(), v); }
    auto side = [&](const char *tag, Graph &graph, World &W) {
        rumi::LoopClosingStep step;
        ORB_SLAM3::ORBmatcher matcherBoW(0.9, true);
        std::set<KeyFrameSN *> spConnectedKeyFrames;
        for (auto &e : W.cur->mConnectedKeyFrameWeights) spConnectedKeyFrames.insert(e.first);
        Outputs o;
        srand(4321);
        rumi_facade::clear_status();
        const int ret = step.DetectCommonRegionsFromBoWResident(graph, W.cur, W.cand, spConnectedKeyFrames, matcherBoW, false, false, th, o.pMatchedKF2, o.pLastCurrentKF, o.g2oScw,
                                                               o.nNumCoincidences, o.vpMPs, o.vpMatchedMPs, toSophusMock);
        const int next = rand();
        float ms[3];
        std::printf("S %s %d\n", tag, rumi_common_regions_bow_resident_stage_ms(ORB_SLAM3::ORBmatcher::arena(), ms));
        show(tag, W, ret, o, next);
    };
    side("B", graphB, B);
    side("A", graphA, A);
    // the by-slot stage over the real CovisibilityGraph (its FlushDirty, SlotOf, PointAt), with and without member matches, against the
    // host-pointer stage, field by field; two points marked dirty first, so that FlushDirty has something to flush
    {
        using Result = rumi_facade::BowStageResult<KeyFrameSN, MapPointSN>;
        ORB_SLAM3::ORBmatcher matcherBoW(0.9, true);
        std::set<KeyFrameSN *> spConnectedKeyFrames;
        for (auto &e : A.cur->mConnectedKeyFrameWeights) spConnectedKeyFrames.insert(e.first);
        std::vector<Result> byPointer, with, without;
        graphA.MarkDirty(A.mps[0].get()); graphA.MarkDirty(A.mps[1].get());
        const int retP = rumi_facade::CommonRegionsBoWStage(A.cur, A.cand, spConnectedKeyFrames, th.nNumCovisibles, matcherBoW, byPointer);
        const int ret1 = rumi_facade::CommonRegionsBoWStageResident(graphA, A.cur, A.cand, spConnectedKeyFrames, th.nNumCovisibles, matcherBoW, with, true);
        const int ret0 = rumi_facade::CommonRegionsBoWStageResident(graphA, A.cur, A.cand, spConnectedKeyFrames, th.nNumCovisibles, matcherBoW, without, false);
        std::string d = ret1 != retP ? "return value" : differ(byPointer, with, true);
        std::printf("E with %s %s\n", d.empty() ? "equal" : "DIFFERENT", d.c_str());
        d = ret0 != retP ? "return value" : differ(byPointer, without, false);
        std::printf("E without %s %s\n", d.empty() ? "equal" : "DIFFERENT", d.c_str());
        int matched = 0;
        for (const Result &r : with) for (MapPointSN *p : r.vpMatchedPoints) matched += p != nullptr;
        std::printf("N %d %zu %d %zu\n", retP, with.size(), matched, graphA.DirtyCount());
    }
    return 0;
}

int main(int argc, char **argv) {
    if (argc >= 2 && !std::strcmp(argv[1], "lc")) return run_lc(argc, argv);
    if (argc >= 2 && !std::strcmp(argv[1], "pr")) return run_pr(argc, argv);
    std::printf("usage: test_common_regions_resident_facade lc scene.bin unsynced | pr map.bin nBoWMatches nBoWInliers nSim3Inliers nProjMatches nProjOptMatches unsynced\n");
    return 2;
}
