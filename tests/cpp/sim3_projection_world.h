// The map file of tests/test_sim3_projection_facade_gpu.py (write_map) read into the mock data model of mock_model_sim3_projection.h: the loader of
// tests/cpp/test_sim3_projection_facade.cc as a header, for the tests of the members that came after it.  TEST INFRASTRUCTURE.
#pragma once
#include <cmath>
#include <cstdio>
#include <cstring>
#include <map>
#include <memory>
#include <vector>

#include "mock_model_sim3_projection.h"

template <class T> static bool rd(FILE *f, T *p, size_t n) { return n == 0 || std::fread(p, sizeof(T), n, f) == n; }

struct World {
    MapKR map;
    std::vector<std::unique_ptr<KeyFrameSN>> kfs;
    std::vector<std::unique_ptr<MapPointSN>> mps;
    KeyFrameSN *cur = nullptr;
    std::vector<KeyFrameSN *> cand;
    float sim3[8];                                                 // of the current key-frame: q xyzw, t, s
    std::map<const void *, int> pi, ki;
};

// header: n_kf n_pts nleftKf unsyncedKf unseenPoint mode (0: as is, 2: 641 jobs) cur n_cand
static bool load(const char *path, int32_t *h, World &w) {
    FILE *f = std::fopen(path, "rb");
    if (!f) return false;
    if (!rd(f, h, 8)) return false;
    std::vector<std::vector<int32_t>> cov(h[0]);
    for (int k = 0; k < h[0]; k++) {
        std::unique_ptr<KeyFrameSN> kf(new KeyFrameSN());
        int32_t n, nc;
        float T7[7];
        if (!rd(f, &n, 1) || !rd(f, T7, 7)) return false;
        kf->N = n; kf->mnId = k + 1; kf->map = &w.map; kf->mTimeStamp = k;
        kf->mvKeysUn.resize(n);
        kf->mDescriptors.create(n > 0 ? n : 1, 32, CV_8U);
        std::vector<int32_t> row(n);
        static_assert(sizeof(cv::KeyPoint) == 28, "the file holds 28-byte key-points");
        if (!rd(f, kf->mvKeysUn.data(), n) || !rd(f, kf->mDescriptors.ptr(0), (size_t)n * 32) || !rd(f, row.data(), n)) return false;
        if (!rd(f, &nc, 1)) return false;
        cov[k].resize(nc);
        if (!rd(f, cov[k].data(), nc)) return false;
        kf->mvScaleFactors.assign(8, 1.f);
        for (int l = 1; l < 8; l++) kf->mvScaleFactors[l] = kf->mvScaleFactors[l - 1] * 1.2f;
        kf->mnScaleLevels = 8; kf->mfLogScaleFactor = std::log(1.2f);
        kf->fx = kf->fy = 500.f; kf->cx = 320.f; kf->cy = 240.f;
        kf->cam.fx = kf->cam.fy = 500.f; kf->cam.cx = 320.f; kf->cam.cy = 240.f;
        kf->pose = Sophus::SE3f(Eigen::Quaternionf(T7[3], T7[0], T7[1], T7[2]), Eigen::Vector3f(T7[4], T7[5], T7[6]));
        kf->mvuRight.assign(n, -1.f);
        kf->mvpMapPoints.assign(n, nullptr);
        if (k == h[2]) kf->NLeft = 0;
        w.kfs.push_back(std::move(kf));
        for (int i = 0; i < n; i++) w.kfs.back()->mvpMapPoints[i] = reinterpret_cast<MapPoint *>((intptr_t)(row[i] + 1));   // ids for now
    }
    for (int k = 0; k < h[0]; k++) {
        std::vector<KeyFrameSN *> ord;
        std::map<KeyFrameSN *, int> wts;
        std::vector<int> ws;
        for (size_t i = 0; i < cov[k].size(); i++) {
            if (cov[k][i] < 0 || cov[k][i] >= h[0]) return false;
            ord.push_back(w.kfs[cov[k][i]].get()); wts[ord.back()] = 100 - (int)i; ws.push_back(100 - (int)i);
        }
        w.kfs[k]->SetCovisibility(wts, ord, ws);
    }
    std::vector<int32_t> cand(h[7]);
    if (!rd(f, w.sim3, 8) || !rd(f, cand.data(), cand.size()) || h[6] < 0 || h[6] >= h[0]) return false;
    w.cur = w.kfs[h[6]].get();
    for (int32_t c : cand) { if (c < 0 || c >= h[0]) return false; w.cand.push_back(w.kfs[c].get()); }
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
    // optional tail (tests/test_place_recognition_facade_gpu.py): per key-frame the vocabulary node of every feature (-1: in no node) -> mFeatVec
    for (int k = 0; k < h[0]; k++) {
        std::vector<int32_t> node(w.kfs[k]->N);
        if (!rd(f, node.data(), node.size())) break;
        for (int i = 0; i < w.kfs[k]->N; i++) if (node[i] >= 0) w.kfs[k]->mFeatVec[(unsigned)node[i]].push_back((unsigned)i);
    }
    std::fclose(f);
    for (auto &kf : w.kfs) {                                       // sigma tables of the 8-level pyramid, as ORBextractor fills them
        kf->mvLevelSigma2.assign(8, 1.f); kf->mvInvLevelSigma2.assign(8, 1.f);
        for (int l = 1; l < 8; l++) { kf->mvLevelSigma2[l] = kf->mvScaleFactors[l] * kf->mvScaleFactors[l]; kf->mvInvLevelSigma2[l] = 1.f / kf->mvLevelSigma2[l]; }
    }
    for (auto &kf : w.kfs)
        for (int i = 0; i < kf->N; i++) {
            const intptr_t id = reinterpret_cast<intptr_t>(kf->mvpMapPoints[i]) - 1;
            MapPointSN *p = id >= 0 ? w.mps[id].get() : nullptr;
            kf->mvpMapPoints[i] = p;
            if (p && !p->bad) { p->obs[kf.get()] = std::make_tuple(i, -1); p->nObs++; if (!p->mpRefKF) p->mpRefKF = kf.get(); }
        }
    for (size_t i = 0; i < w.mps.size(); i++) w.pi[w.mps[i].get()] = (int)i;
    for (size_t k = 0; k < w.kfs.size(); k++) w.ki[w.kfs[k].get()] = (int)k;
    return true;
}
