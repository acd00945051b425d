// rumi_facade::CommonRegionsBoWStage (facade/LoopClosingStep.h) over the mock key-frames of tests/cpp/mock_model_loopclosing.h, on the GPU.  Reads
// the scene written by tests/test_common_regions_facade_gpu.py (all int32 unless noted):
//   header     n_kfs n_points n_cand n_covisibles nnratio (float) check_orientation
//   points     bad [n_points] (uint8)
//   key-frame  n bad nleft n_nodes n_cov n_conn | angle [n] (float) | desc [n x 32] (uint8) | mp [n] (point number, -1 NULL) |
//              per node: id count idx[count] | covisibles [n_cov] | connected [n_conn]           (key-frame 0 is the current one)
//   candidates [n_cand]  key-frame numbers, -1 = NULL
// and prints what the stage leaves:
//   R ret status n_results
//   C cand num index most | V cand kf... (vpCovKFi) | M cand j point... (vvpMatchedMPs[j]; "M cand j empty" when it was never assigned)
//   P cand point... (vpMatchedPoints) | K cand kf... (vpKeyFrameMatchedMP)          -1 = NULL throughout
#include <cstdio>
#include <memory>
#include <vector>

#include "ORBmatcher.h"
#include "LoopClosingStep.h"

#include "mock_model_loopclosing.h"

template <class T> static bool rd(FILE *f, T *p, size_t n) { return n == 0 || std::fread(p, sizeof(T), n, f) == n; }

int main(int argc, char **argv) {
    if (argc < 2) { std::printf("usage: test_common_regions_facade scene.bin\n"); return 2; }
    FILE *f = std::fopen(argv[1], "rb");
    if (!f) { std::printf("cannot read %s\n", argv[1]); return 2; }
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

    ORB_SLAM3::ORBmatcher matcherBoW(nnratio, ori != 0);
    std::vector<rumi_facade::BowStageResult<KeyFrameLC, MapPointLC>> out;
    rumi_facade::clear_status();
    const int ret = rumi_facade::CommonRegionsBoWStage(kfs[0].get(), vpBowCand, h[3], matcherBoW, out);
    std::printf("R %d %d %zu\n", ret, rumi_facade::last_status(), out.size());
    for (const auto &r : out) {
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
