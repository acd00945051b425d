// CovisibilityGraph::SyncPoses / SyncPointMaps (facade/CovisibilityGraph.h) over the mock data model of tests/cpp/mock_model_lba_resident.h.
// Host only: the two members validate and stage, so what they left in the store is read back from its mirror (rumi_hook_covis_read_poses)
// without a device.  Built and run by tests/test_lba_resident_facade_cpu.py.  Prints FAIL lines; the exit status is the number of failed checks.
#define RUMI_HAVE_SOPHUS 1
#include <cmath>
#include <cstdio>
#include <memory>
#include <vector>

#include "mock_sophus.h"

#include "CovisibilityGraph.h"
#include "rumi_testhooks.h"

#include "mock_model_lba_resident.h"

static int fails = 0;
#define CHECK(c, msg) do { if (!(c)) { std::printf("FAIL: %s (%s:%d)\n", msg, __FILE__, __LINE__); fails++; } } while (0)

int main() {
    MapLR mapA, mapB;
    mapA.id = 3; mapB.id = 8;
    const int nKf = 3, nPt = 5;
    std::unique_ptr<KeyFrameLR[]> kf(new KeyFrameLR[nKf]);
    std::vector<std::unique_ptr<MapPointLR>> mp;
    for (int p = 0; p < nPt; p++) { mp.emplace_back(new MapPointLR()); mp[p]->map = p == 4 ? &mapB : &mapA; }
    for (int k = 0; k < nKf; k++) {
        kf[k].mnId = k; kf[k].map = &mapA; kf[k].N = nPt;
        kf[k].mvpMapPoints.assign(nPt, nullptr);
        const float a = 0.1f * (k + 1);
        // a quaternion that is not of unit length and has w < 0 for k = 2: the store keeps what the solver's staging makes of it
        kf[k].SetPose(Sophus::SE3f(Eigen::Quaternionf(k == 2 ? -std::cos(a) : std::cos(a), 0.f, std::sin(a), 0.f), Eigen::Vector3f(0.5f * k, -1.f, 2.f + k)));
    }
    for (int p = 0; p < nPt; p++)
        for (int k = 0; k < nKf; k++)
            if ((p + k) % 2 == 0) { kf[k].mvpMapPoints[p] = mp[p].get(); mp[p]->obs[&kf[k]] = std::make_tuple(p, -1); }

    CovisibilityGraph<KeyFrameLR, MapPointLR> graph(8, 16);
    CHECK(graph.ok(), "the store");
    CHECK(graph.SyncPoses({&kf[2], &kf[0], &kf[2]}) == RUMI_OK, "SyncPoses stages key-frames the store has not seen, each once");
    std::vector<MapPointLR *> pts;
    for (auto &p : mp) pts.push_back(p.get());
    pts.push_back(mp[1].get());
    CHECK(graph.SyncPointMaps(pts) == RUMI_OK, "SyncPointMaps");

    int32_t slots[3], has[3], ids[5], maps[5], hasMap[5];
    double T[3][8];
    for (int k = 0; k < nKf; k++) slots[k] = graph.SlotOf(&kf[k]);
    for (int p = 0; p < nPt; p++) ids[p] = graph.IdOf(mp[p].get());
    CHECK(slots[0] >= 0 && slots[2] >= 0, "slots of the synced key-frames");
    if (slots[1] < 0) slots[1] = 7;                                     // not seen by the store: any slot without a pose
    CHECK(rumi_hook_covis_read_poses(graph.handle(), nKf, slots, &T[0][0], has, nPt, ids, maps, hasMap, 0) == RUMI_OK, "read back");
    CHECK(has[0] == 1 && has[2] == 1, "has pose");
    for (int k : {0, 2}) {
        const auto P = kf[k].GetPose(); const auto q = P.unit_quaternion(); const auto t = P.translation();
        double w[4] = {q.x(), q.y(), q.z(), q.w()};
        if (w[3] < 0) for (double &v : w) v = -v;
        const double rn = 1.0 / std::sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2] + w[3] * w[3]);
        bool same = T[k][7] == 0;
        for (int c = 0; c < 4; c++) same = same && T[k][c] == w[c] * rn;
        for (int c = 0; c < 3; c++) same = same && T[k][4 + c] == (double)t(c);
        CHECK(same, "the staged pose is the solver's: w >= 0, normalised in double");
    }
    for (int p = 0; p < nPt; p++) CHECK(hasMap[p] == 1 && maps[p] == (p == 4 ? 8 : 3), "the point's map in the key-frames' numbering");
    mp[0]->map = &mapB;                                                  // a merge moves the point
    CHECK(graph.SyncPointMaps({mp[0].get()}) == RUMI_OK, "SyncPointMaps again");
    CHECK(rumi_hook_covis_read_poses(graph.handle(), 0, nullptr, nullptr, nullptr, 1, ids, maps, hasMap, 0) == RUMI_OK && maps[0] == 8, "the new map");
    std::printf("done %d\n", fails);
    return fails;
}
