// LocalMappingStep::KeyFrameCulling / CloudKeyFrameCulling (facade/LocalMappingStep.h) over the mock data model of
// tests/cpp/mock_model_culling.h, on the GPU.  Reads a map written by tests/test_culling_facade_gpu.py (key-frames: flags and octaves;
// points: bad flag, nObs, observations; the covisible list; cloud variant, mbAbortBA, mbInertial, mbMonocular), builds mock objects, runs the
// member once and prints the map it leaves:
//   R ret status                     the member's return value and rumi_facade::last_status()
//   K k bad toBeErased nUpdateBestCovisibles
//   M k slot...                      mvpMapPoints as point indices, -1 = NULL
//   P i bad nObs n (kf feature)...   the point's observation map
#define RUMI_HAVE_SOPHUS 1
#include <cstdio>
#include <cstring>
#include <map>
#include <memory>
#include <vector>

#include "mock_sophus.h"

#include "LocalMappingStep.h"

#include "mock_model_culling.h"

template <class T> static bool rd(FILE *f, T *p, size_t n) { return n == 0 || std::fread(p, sizeof(T), n, f) == n; }

int main(int argc, char **argv) {
    if (argc < 2) { std::printf("usage: test_culling_facade map.bin\n"); return 2; }
    FILE *f = std::fopen(argv[1], "rb");
    if (!f) { std::printf("cannot read %s\n", argv[1]); return 2; }
    int32_t h[8];                                                  // n_kf n_pts n_cand cloud abort inertial monocular stereoKf
    if (!rd(f, h, 8)) return 2;
    Map map;
    std::vector<std::unique_ptr<KeyFrameKC>> kfs;
    std::vector<std::unique_ptr<MapPointKC>> mps;
    for (int k = 0; k < h[0]; k++) {
        std::unique_ptr<KeyFrameKC> kf(new KeyFrameKC());
        int32_t v[5];                                              // n bad init not_erase cloud
        if (!rd(f, v, 5)) return 2;
        std::vector<int32_t> oct(v[0]);
        if (!rd(f, oct.data(), oct.size())) return 2;
        kf->N = v[0]; kf->bad = v[1] != 0; kf->mnId = v[2] ? 0 : k + 1;   // Map::GetInitKFid() of the mock is 0
        kf->mbNotErase = v[3] != 0; kf->mbCloud = v[4] != 0; kf->map = &map;
        kf->mvKeysUn.resize(v[0]);
        for (int i = 0; i < v[0]; i++) kf->mvKeysUn[i].octave = oct[i];
        kf->mvpMapPoints.assign(v[0], nullptr);
        kf->mvuRight.assign(v[0], -1.f);
        if (k == h[7]) kf->NLeft = 0;
        kfs.push_back(std::move(kf));
    }
    for (int i = 0; i < h[1]; i++) {
        std::unique_ptr<MapPointKC> p(new MapPointKC());
        int32_t v[3];                                              // bad nObs n
        if (!rd(f, v, 3)) return 2;
        std::vector<int32_t> o((size_t)v[2] * 2);
        if (!rd(f, o.data(), o.size())) return 2;
        for (int j = 0; j < v[2]; j++) {
            p->obs[kfs[o[2 * j]].get()] = std::make_tuple(o[2 * j + 1], -1);
            kfs[o[2 * j]]->mvpMapPoints[o[2 * j + 1]] = p.get();
        }
        p->bad = v[0] != 0; p->nObs = v[1]; p->map = &map;
        mps.push_back(std::move(p));
    }
    std::vector<int32_t> cand(h[2]);
    if (!rd(f, cand.data(), cand.size())) return 2;
    std::fclose(f);
    KeyFrameKC current;
    current.map = &map; current.mnId = 1000000;
    for (int32_t c : cand) current.covisKC.push_back(kfs[c].get());

    rumi::LocalMappingStep step;
    rumi_facade::clear_status();
    const int ret = h[3] ? step.CloudKeyFrameCulling(&current, h[5] != 0, h[6] != 0, h[4] != 0)
                         : step.KeyFrameCulling(&current, h[5] != 0, h[6] != 0, h[4] != 0);
    std::printf("R %d %d\n", ret, rumi_facade::last_status());
    std::map<const MapPoint *, int> index;
    for (size_t i = 0; i < mps.size(); i++) index[mps[i].get()] = (int)i;
    std::map<const KeyFrame *, int> kindex;
    for (size_t k = 0; k < kfs.size(); k++) kindex[kfs[k].get()] = (int)k;
    for (size_t k = 0; k < kfs.size(); k++) {
        std::printf("K %zu %d %d %d\nM %zu", k, (int)kfs[k]->bad, (int)kfs[k]->mbToBeErased, current.nUpdateBestCovisibles, k);
        for (MapPoint *p : kfs[k]->mvpMapPoints) std::printf(" %d", p ? index[p] : -1);
        std::printf("\n");
    }
    for (size_t i = 0; i < mps.size(); i++) {
        std::printf("P %zu %d %d %zu", i, (int)mps[i]->bad, mps[i]->nObs, mps[i]->obs.size());
        for (auto &o : mps[i]->obs) std::printf(" %d %d", kindex[o.first], std::get<0>(o.second));
        std::printf("\n");
    }
    return 0;
}
