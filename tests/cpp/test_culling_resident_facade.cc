// LocalMappingStep::KeyFrameCullingResident / CloudKeyFrameCullingResident (facade/LocalMappingStep.h) over a CovisibilityGraph and the mock
// data model of tests/cpp/mock_model_culling_resident.h, against the block members on a copy of the same map, on the GPU.  Reads a map
// written by tests/test_culling_resident_facade_gpu.py: the format of test_culling_facade.cc with two covisible lists, one per current
// key-frame, and `unseen`, a candidate the graph is not told about.  Map A belongs to a graph (every key-frame and point staged, every
// key-frame's features, the mutators' Sync hooks on) and takes the resident member twice; map B takes the block member twice.  Prints
//   R map call ret status                  the member's return value and rumi_facade::last_status()
//   U call key-frames points               what the graph holds after the call
//   K map k bad toBeErased nUpdateBestCovisibles
//   M map k slot...                        mvpMapPoints as point indices, -1 = NULL
//   P map i bad nObs n (kf feature)...     the point's observation map
#define RUMI_HAVE_SOPHUS 1
#include <cstdio>
#include <cstring>
#include <map>
#include <memory>
#include <vector>

#include "mock_sophus.h"

#include "CovisibilityGraph.h"
#include "LocalMappingStep.h"

#include "mock_model_culling_resident.h"

template <class T> static bool rd(FILE *f, T *p, size_t n) { return n == 0 || std::fread(p, sizeof(T), n, f) == n; }

struct World {
    MapKR map;
    std::vector<std::unique_ptr<KeyFrameKR>> kfs;
    std::vector<std::unique_ptr<MapPointKR>> mps;
    KeyFrameKR current[2];
};

static bool load(const char *path, int32_t *h, World &w) {
    FILE *f = std::fopen(path, "rb");
    if (!f) return false;
    if (!rd(f, h, 10)) return false;                               // n_kf n_pts n_cand1 n_cand2 cloud abort inertial monocular stereoKf unseen
    for (int k = 0; k < h[0]; k++) {
        std::unique_ptr<KeyFrameKR> kf(new KeyFrameKR());
        int32_t v[5];                                              // n bad init not_erase cloud
        if (!rd(f, v, 5)) return false;
        std::vector<int32_t> oct(v[0]);
        if (!rd(f, oct.data(), oct.size())) return false;
        kf->N = v[0]; kf->bad = v[1] != 0; kf->mnId = v[2] ? 0 : k + 1;   // Map::GetInitKFid() of the mock is 0
        kf->mbNotErase = v[3] != 0; kf->mbCloud = v[4] != 0; kf->map = &w.map;
        kf->mvKeysUn.resize(v[0]);
        for (int i = 0; i < v[0]; i++) kf->mvKeysUn[i].octave = oct[i];
        kf->mDescriptors.create(v[0] > 0 ? v[0] : 1, 32, CV_8U);
        std::memset(kf->mDescriptors.ptr(0), 0, (size_t)(v[0] > 0 ? v[0] : 1) * 32);
        kf->mvScaleFactors.assign(8, 1.f);
        kf->mvpMapPoints.assign(v[0], nullptr);
        kf->mvuRight.assign(v[0], -1.f);
        if (k == h[8]) kf->NLeft = 0;
        w.kfs.push_back(std::move(kf));
    }
    for (int i = 0; i < h[1]; i++) {
        std::unique_ptr<MapPointKR> p(new MapPointKR());
        int32_t v[3];                                              // bad nObs n
        if (!rd(f, v, 3)) return false;
        std::vector<int32_t> o((size_t)v[2] * 2);
        if (!rd(f, o.data(), o.size())) return false;
        for (int j = 0; j < v[2]; j++) {
            p->obs[w.kfs[o[2 * j]].get()] = std::make_tuple(o[2 * j + 1], -1);
            w.kfs[o[2 * j]]->mvpMapPoints[o[2 * j + 1]] = p.get();
        }
        p->bad = v[0] != 0; p->nObs = v[1]; p->map = &w.map;
        w.mps.push_back(std::move(p));
    }
    for (int c = 0; c < 2; c++) {
        std::vector<int32_t> cand(h[2 + c]);
        if (!rd(f, cand.data(), cand.size())) return false;
        w.current[c].map = &w.map; w.current[c].mnId = 1000000 + c;
        for (int32_t k : cand) w.current[c].covisKR.push_back(w.kfs[k].get());
    }
    std::fclose(f);
    return true;
}

static void print(const char *tag, World &w) {
    std::map<const MapPoint *, int> index;
    for (size_t i = 0; i < w.mps.size(); i++) index[w.mps[i].get()] = (int)i;
    std::map<const KeyFrame *, int> kindex;
    for (size_t k = 0; k < w.kfs.size(); k++) kindex[w.kfs[k].get()] = (int)k;
    for (size_t k = 0; k < w.kfs.size(); k++) {
        std::printf("K %s %zu %d %d %d\nM %s %zu", tag, k, (int)w.kfs[k]->bad, (int)w.kfs[k]->mbToBeErased,
                    w.current[0].nUpdateBestCovisibles + w.current[1].nUpdateBestCovisibles, tag, k);
        for (MapPoint *p : w.kfs[k]->mvpMapPoints) std::printf(" %d", p ? index[p] : -1);
        std::printf("\n");
    }
    for (size_t i = 0; i < w.mps.size(); i++) {
        std::printf("P %s %zu %d %d %zu", tag, i, (int)w.mps[i]->bad, w.mps[i]->nObs, w.mps[i]->obs.size());
        for (auto &o : w.mps[i]->obs) std::printf(" %d %d", kindex[o.first], std::get<0>(o.second));
        std::printf("\n");
    }
}

int main(int argc, char **argv) {
    if (argc < 2) { std::printf("usage: test_culling_resident_facade map.bin\n"); return 2; }
    int32_t h[10];
    World A, B;
    if (!load(argv[1], h, A) || !load(argv[1], h, B)) { std::printf("cannot read %s\n", argv[1]); return 2; }
    const bool cloud = h[4] != 0, abortBA = h[5] != 0, inertial = h[6] != 0, mono = h[7] != 0;

    using Graph = CovisibilityGraph<KeyFrameKR, MapPointKR>;
    Graph graph(h[0] + 4, h[1] + 4);
    if (!graph.ok()) return 3;
    for (int k = 0; k < h[0]; k++)
        if (k != h[9] && (graph.Sync(A.kfs[k].get()) != RUMI_OK || graph.SyncFeatures(A.kfs[k].get()) != RUMI_OK)) return 3;
    for (auto &p : A.mps)                                          // (`unseen` observes no point: nothing brings it in)
        if (graph.Sync(p.get()) != RUMI_OK) return 3;
    A.map.hooks.keyframe = [&](KeyFrameKR *k) { graph.Sync(k); };
    A.map.hooks.point = [&](MapPointKR *p) { graph.Sync(p); };
    A.map.hooks.drop = [&](KeyFrameKR *k) { graph.DropFeatures(k); };

    rumi::LocalMappingStep step;
    for (int call = 0; call < 2; call++) {
        rumi_facade::clear_status();
        int ret = cloud ? step.CloudKeyFrameCullingResident(graph, &A.current[call], inertial, mono, abortBA)
                        : step.KeyFrameCullingResident(graph, &A.current[call], inertial, mono, abortBA);
        std::printf("R A %d %d %d\n", call, ret, rumi_facade::last_status());
        std::printf("U %d %d %d\n", call, graph.KeyFrameCount(), graph.PointCount());
        rumi_facade::clear_status();
        ret = cloud ? step.CloudKeyFrameCulling(&B.current[call], inertial, mono, abortBA) : step.KeyFrameCulling(&B.current[call], inertial, mono, abortBA);
        std::printf("R B %d %d %d\n", call, ret, rumi_facade::last_status());
    }
    print("A", A);
    print("B", B);
    return 0;
}
