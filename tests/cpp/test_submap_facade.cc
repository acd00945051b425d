// rumi_facade::MatchSubmapKeyPoints (facade/CloudMergingStep.h) over the mock key-frames of tests/cpp/mock_model_submap.h, on the GPU.  Reads the
// two sub-maps written by tests/test_submap_facade_gpu.py:
//   header  n_frames n_map1 n_map2 n_pairs nleft_frame cols_frame      (the last two: the frame to give NLeft = 0 / 32 grid columns, or -1)
//   frame   n min_x min_y (int32)  w_inv h_inv (float)  keys n x 2  keys_un n x 2 (float)  has_mp n (uint8)
//   map1 [n_map1], map2 [n_map2]  frame numbers in the order of GetAllKeyFrames();  pairs n_pairs x 2: mKfMatch12 (index in map 1, index in map 2)
// and prints what the member leaves:
//   R ret status n1 n2 n3 n4         the return value, rumi_facade::last_status() and the sizes of the four maps
//   N frame matchNum                 mvpMatchedPointsNum12, in pair order
//   P frame slot...                  mvpMatchedPoints12 as (frame of key-frame 2) * 100000 + slot, -1 = NULL
//   K frame i1 i2 ...                mvpMatchedKeyPoints12         V frame i1 i2 ...   mvpValidMatchedKeyPoints12
#include <cstdio>
#include <map>
#include <memory>
#include <vector>

#include "CloudMergingStep.h"

#include "mock_model_submap.h"

template <class T> static bool rd(FILE *f, T *p, size_t n) { return n == 0 || std::fread(p, sizeof(T), n, f) == n; }

int main(int argc, char **argv) {
    if (argc < 2) { std::printf("usage: test_submap_facade maps.bin\n"); return 2; }
    FILE *f = std::fopen(argv[1], "rb");
    if (!f) { std::printf("cannot read %s\n", argv[1]); return 2; }
    int32_t h[6];
    if (!rd(f, h, 6)) return 2;
    std::vector<std::unique_ptr<KeyFrameSM>> kfs;
    std::vector<std::unique_ptr<MapPointSM>> mps;
    std::map<const MapPointSM *, int> code;
    std::map<const KeyFrameSM *, int> number;
    for (int k = 0; k < h[0]; k++) {
        std::unique_ptr<KeyFrameSM> kf(new KeyFrameSM());
        int32_t v[3];
        float inv[2];
        if (!rd(f, v, 3) || !rd(f, inv, 2)) return 2;
        std::vector<float> keys(2 * (size_t)v[0]), un(2 * (size_t)v[0]);
        std::vector<uint8_t> mp(v[0]);
        if (!rd(f, keys.data(), keys.size()) || !rd(f, un.data(), un.size()) || !rd(f, mp.data(), mp.size())) return 2;
        kf->mnMinX = v[1]; kf->mnMinY = v[2]; kf->mfGridElementWidthInv = inv[0]; kf->mfGridElementHeightInv = inv[1];
        kf->mvKeys.resize(v[0]); kf->mvKeysUn.resize(v[0]); kf->mvpMapPoints.assign(v[0], nullptr);
        for (int i = 0; i < v[0]; i++) {
            kf->mvKeys[i].pt.x = keys[2 * i]; kf->mvKeys[i].pt.y = keys[2 * i + 1];
            kf->mvKeysUn[i].pt.x = un[2 * i]; kf->mvKeysUn[i].pt.y = un[2 * i + 1];
            if (mp[i]) {
                mps.emplace_back(new MapPointSM());
                code[mps.back().get()] = k * 100000 + i;
                kf->mvpMapPoints[i] = mps.back().get();
            }
        }
        if (k == h[4]) kf->NLeft = 0;
        if (k == h[5]) kf->mnGridCols = 32;
        number[kf.get()] = k;
        kfs.push_back(std::move(kf));
    }
    std::vector<int32_t> m1(h[1]), m2(h[2]), pairs(2 * (size_t)h[3]);
    if (!rd(f, m1.data(), m1.size()) || !rd(f, m2.data(), m2.size()) || !rd(f, pairs.data(), pairs.size())) return 2;
    std::fclose(f);
    std::vector<KeyFrameSM *> map1, map2;
    for (int32_t k : m1) map1.push_back(kfs[k].get());
    for (int32_t k : m2) map2.push_back(kfs[k].get());
    std::map<int, int> mKfMatch12;
    for (int p = 0; p < h[3]; p++) mKfMatch12[pairs[2 * p]] = pairs[2 * p + 1];

    std::map<KeyFrameSM *, std::vector<MapPointSM *>> matchedPoints;
    std::map<KeyFrameSM *, std::vector<std::pair<int, int>>> matchedKP, validKP;
    std::map<KeyFrameSM *, int> matchedNum;
    rumi_facade::clear_status();
    const int ret = rumi_facade::MatchSubmapKeyPoints(map1, map2, mKfMatch12, 3.f, matchedPoints, matchedKP, validKP, matchedNum);
    std::printf("R %d %d %zu %zu %zu %zu\n", ret, rumi_facade::last_status(), matchedPoints.size(), matchedKP.size(), validKP.size(), matchedNum.size());
    for (const auto &m : mKfMatch12) {
        KeyFrameSM *kf = map1[m.first];
        if (!matchedNum.count(kf)) continue;
        std::printf("N %d %d\nP %d", number[kf], matchedNum[kf], number[kf]);
        for (MapPointSM *p : matchedPoints[kf]) std::printf(" %d", p ? code[p] : -1);
        std::printf("\nK %d", number[kf]);
        for (const auto &e : matchedKP[kf]) std::printf(" %d %d", e.first, e.second);
        std::printf("\nV %d", number[kf]);
        for (const auto &e : validKP[kf]) std::printf(" %d %d", e.first, e.second);
        std::printf("\n");
    }
    return 0;
}
