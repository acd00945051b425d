// Runs CovisibilityGraph (facade/CovisibilityGraph.h) over the mock model of mock_model_covis.h on a map read from a text file, and prints the
// state it leaves on the mock objects (tests/test_covis_facade_gpu.py compares it with the oracle's).  TEST INFRASTRUCTURE.
//   file: max_kf max_points n_kf n_pt | per key-frame: slot key map bad timestamp first  n mp..  n best..  parent  n children.. |
//         per point: id bad  n observers.. | cloud  B batch.. | refuse | n_frames, per frame: n points..
// Key-frames are laid out in one array by the rank of their key, so that their addresses order as the keys do.
#include <cstdio>
#include <fstream>
#include <iostream>
#include <memory>

#include "CovisibilityGraph.h"
#include "mock_model_covis.h"

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    std::ifstream in(argv[1]);
    int maxKf, maxPts, nKf, nPt;
    in >> maxKf >> maxPts >> nKf >> nPt;
    struct Rec { int slot; unsigned long long key; int map, bad, first; double ts; std::vector<int> mp, best, ch; int parent; };
    std::vector<Rec> recs(nKf);
    for (Rec &r : recs) {
        int n;
        in >> r.slot >> r.key >> r.map >> r.bad >> r.ts >> r.first;
        in >> n; r.mp.resize(n); for (int &v : r.mp) in >> v;
        in >> n; r.best.resize(n); for (int &v : r.best) in >> v;
        in >> r.parent;
        in >> n; r.ch.resize(n); for (int &v : r.ch) in >> v;
    }
    std::vector<int> rank(nKf);
    for (int i = 0; i < nKf; i++) rank[i] = i;
    std::sort(rank.begin(), rank.end(), [&](int a, int b) { return recs[a].key < recs[b].key; });
    std::vector<KeyFrame> pool(nKf);
    std::vector<KeyFrame *> bySlot(maxKf, nullptr);
    for (int r = 0; r < nKf; r++) bySlot[recs[rank[r]].slot] = &pool[r];
    std::vector<MapPoint> pts(maxPts);
    for (int p = 0; p < maxPts; p++) pts[p].mnId = p;
    Map maps[2];
    maps[0].mnId = 0; maps[1].mnId = 1;
    maps[0].mnInitKFid = maps[1].mnInitKFid = recs.empty() ? 0 : recs[0].slot;
    for (const Rec &r : recs) {
        KeyFrame *k = bySlot[r.slot];
        k->mnId = r.slot; k->bad = r.bad; k->mTimeStamp = r.ts; k->mpMap = &maps[r.map]; k->mbFirstConnection = r.first;
        maps[0].kfs.push_back(k);
        for (int p : r.mp) k->mvpMapPoints.push_back(p < 0 ? nullptr : &pts[p]);
        for (size_t j = 0; j < r.best.size(); j++) {
            k->mvpOrderedConnectedKeyFrames.push_back(bySlot[r.best[j]]);
            k->mvOrderedWeights.push_back(1000 - (int)j);
            k->mConnectedKeyFrameWeights[bySlot[r.best[j]]] = 1000 - (int)j;
        }
        k->mpParent = r.parent < 0 ? nullptr : bySlot[r.parent];
        for (int c : r.ch) k->mspChildrens.insert(bySlot[c]);
    }
    for (int i = 0; i < nPt; i++) {
        int id, bad, n;
        in >> id >> bad >> n;
        pts[id].bad = bad;
        for (int j = 0; j < n; j++) { int k; in >> k; pts[id].mObservations[bySlot[k]] = std::make_tuple(0, -1); }
        maps[0].mps.push_back(&pts[id]);
    }
    int cloud, B, refuse, nFrames;
    in >> cloud >> B;
    std::vector<KeyFrame *> batch(B);
    for (auto &k : batch) { int s; in >> s; k = bySlot[s]; }
    in >> refuse >> nFrames;

    CovisibilityGraph<KeyFrame, MapPoint> graph(maxKf, maxPts);
    if (!graph.ok()) return 3;
    int rc = graph.SyncAll(&maps[0]);
    std::printf("S %d\n", rc);
    rc = graph.UpdateConnections(batch, cloud != 0);
    std::printf("U %d\n", rc);
    if (B > 0) std::printf("Y %d %d\n", graph.Sync(batch[0]), graph.Sync(&pts[0]));   // one object again, as a mutator of the reference would
    for (const Rec &r : recs) {
        KeyFrame *k = bySlot[r.slot];
        std::printf("K %d %d %d %zu", r.slot, k->mpParent ? (int)k->mpParent->mnId : -1, (int)k->mbFirstConnection, k->mspChildrens.size());
        for (KeyFrame *c : k->mspChildrens) std::printf(" %d", (int)c->mnId);
        std::printf("\nC %d %zu", r.slot, k->mConnectedKeyFrameWeights.size());
        for (auto &e : k->mConnectedKeyFrameWeights) std::printf(" %d %d", (int)e.first->mnId, e.second);
        std::printf("\nO %d %zu", r.slot, k->mvpOrderedConnectedKeyFrames.size());
        for (size_t i = 0; i < k->mvpOrderedConnectedKeyFrames.size(); i++) std::printf(" %d %d", (int)k->mvpOrderedConnectedKeyFrames[i]->mnId, k->mvOrderedWeights[i]);
        std::printf("\n");
    }
    std::vector<KeyFrame *> localKfs;
    std::vector<MapPoint *> localPts;
    KeyFrame *ref = nullptr;
    for (int f = 0; f < nFrames; f++) {
        Frame F;
        F.mnId = 100 + f;
        in >> F.N;
        for (int i = 0; i < F.N; i++) { int p; in >> p; F.mvpMapPoints.push_back(p < 0 ? nullptr : &pts[p]); }
        rc = graph.UpdateLocalMap(F, localKfs, localPts, ref, refuse != 1, refuse == 2);
        std::printf("F %d %d %d %d\nL %d", f, rc, ref ? (int)ref->mnId : -1, F.mpReferenceKF ? (int)F.mpReferenceKF->mnId : -1, f);
        for (KeyFrame *k : localKfs) std::printf(" %d", (int)k->mnId);
        std::printf("\nP %d", f);
        for (MapPoint *p : localPts) std::printf(" %d", (int)p->mnId);
        std::printf("\nN %d", f);
        for (MapPoint *p : F.mvpMapPoints) std::printf(" %d", p ? (int)p->mnId : -1);
        std::printf("\nT %d", f);                                    // the stamps of this frame: key-frames, then -2, then points
        for (const Rec &r : recs) if (bySlot[r.slot]->mnTrackReferenceForFrame == F.mnId) std::printf(" %d", r.slot);
        std::printf(" -2");
        for (int p = 0; p < maxPts; p++) if (pts[p].mnTrackReferenceForFrame == F.mnId) std::printf(" %d", p);
        std::printf("\n");
    }
    return 0;
}
