// rumi_facade::TrackLocalMapResident (facade/TrackingStep.h) on the mock model of mock_model_localmap.h: it must leave the same member state as
// CovisibilityGraph::UpdateLocalMap followed by the existing rumi_facade::TrackLocalMap, and after a SetWorldPos on one point only that point
// travels to the device again.  usage: test_localmap_facade frame0.bin frame1.bin (640 x 480, 8-bit grey)
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "mock_model_localmap.h"

#include "CovisibilityGraph.h"
#include "ORBextractor.h"
#include "TrackingStep.h"
#include "rumi_status.h"

static int fails = 0;
#define CHECK(c, msg) do { if (!(c)) { std::printf("FAIL: %s (%s:%d)\n", msg, __FILE__, __LINE__); fails++; } } while (0)

struct PointState {
    bool inView; float x, y, vc, depth; int level, vis, found; long unsigned int seen, ref;
    bool operator==(const PointState &o) const {
        return inView == o.inView && x == o.x && y == o.y && vc == o.vc && depth == o.depth && level == o.level && vis == o.vis && found == o.found && seen == o.seen && ref == o.ref;
    }
};
struct State {
    std::vector<MapPoint *> mp; std::vector<bool> outl; float T[7]; KeyFrame *frameRef, *ref;
    std::vector<KeyFrame *> lk; std::vector<MapPoint *> lp; std::vector<PointState> pts; std::vector<long unsigned int> kfRef; int inliers;
};
static State snapshot(Frame &F, std::vector<MapPoint> &mps, std::vector<KeyFrame> &kfs, const std::vector<KeyFrame *> &lk, const std::vector<MapPoint *> &lp,
                      KeyFrame *ref, int inliers) {
    State s;
    s.mp = F.mvpMapPoints; s.outl = F.mvbOutlier; std::memcpy(s.T, F.pose.T, 28); s.frameRef = F.mpReferenceKF; s.ref = ref; s.lk = lk; s.lp = lp; s.inliers = inliers;
    for (auto &m : mps) s.pts.push_back(PointState{m.mbTrackInView, m.mTrackProjX, m.mTrackProjY, m.mTrackViewCos, m.mTrackDepth, m.mnTrackScaleLevel, m.nVisible, m.nFound, m.mnLastFrameSeen, m.mnTrackReferenceForFrame});
    for (auto &k : kfs) s.kfRef.push_back(k.mnTrackReferenceForFrame);
    return s;
}
static void reset(std::vector<MapPoint> &mps, std::vector<KeyFrame> &kfs) {
    for (auto &m : mps) { m.mbTrackInView = false; m.mbTrackInViewR = false; m.mTrackProjX = m.mTrackProjY = 0; m.mTrackViewCos = 1; m.mTrackDepth = 1; m.mnTrackScaleLevel = 0; m.nVisible = m.nFound = 0; m.mnLastFrameSeen = 0; m.mnTrackReferenceForFrame = 0; }
    for (auto &k : kfs) k.mnTrackReferenceForFrame = 0;
}

int main(int argc, char **argv) {
    if (argc < 3) { std::printf("usage: test_localmap_facade frame0.bin frame1.bin (640x480 u8)\n"); return 2; }
    std::vector<uint8_t> im[2];
    for (int k = 0; k < 2; k++) {
        im[k].resize(640 * 480);
        FILE *f = std::fopen(argv[1 + k], "rb");
        if (!f || std::fread(im[k].data(), 1, im[k].size(), f) != im[k].size()) { std::printf("cannot read %s\n", argv[1 + k]); return 2; }
        std::fclose(f);
    }
    ORB_SLAM3::ORBextractor ext(1000, 1.2f, 8, 20, 7);
    const std::vector<float> sf = ext.GetScaleFactors();
    cv::Mat image0(480, 640, CV_8U, im[0].data(), 640), image1(480, 640, CV_8U, im[1].data(), 640);
    // ---- the map: one point per feature of frame 0 on the plane z = 2, four key-frames over overlapping windows of the points
    Frame F0; F0.mnId = 10;
    CHECK(rumi_facade::ExtractFrame(F0, image0, ext, 4096) >= -1 && F0.N > 500, "frame 0");
    const int n0 = F0.N;
    std::vector<MapPoint> mps(n0);
    std::vector<KeyFrame> kfs(4);
    Map map;
    for (int i = 0; i < n0; i++) {
        MapPoint &m = mps[i];
        const cv::KeyPoint &kp = F0.mvKeysUn[i];
        m.mnId = i;
        m.pos = V3f{{(kp.pt.x - F0.cx) / F0.fx * 2.f, (kp.pt.y - F0.cy) / F0.fy * 2.f, 2.f}};
        const float d = std::sqrt(m.pos.v[0] * m.pos.v[0] + m.pos.v[1] * m.pos.v[1] + m.pos.v[2] * m.pos.v[2]);
        m.normal = V3f{{m.pos.v[0] / d, m.pos.v[1] / d, m.pos.v[2] / d}};
        m.maxD = d * sf[kp.octave]; m.minD = m.maxD / sf[7];
        m.desc = cv::Mat(1, 32, CV_8U); std::memcpy(m.desc.ptr(0), F0.mDescriptors.ptr(i), 32);
        m.bad = i % 53 == 7;
        F0.mvpMapPoints[i] = i % 3 ? &m : nullptr;               // the last frame knows two thirds of the points
    }
    for (int k = 0; k < 4; k++) {
        KeyFrame &K = kfs[k];
        K.mnId = k; K.mpMap = &map;
        const int a = k * n0 / 6, b = a + n0 / 2;
        for (int i = a; i < b && i < n0; i++) {
            if (i % 29 == 3) { K.mvpMapPoints.push_back(nullptr); continue; }     // (and points 3, 32, ... have fewer observers)
            K.mvpMapPoints.push_back(&mps[i]);
            mps[i].mObservations[&K] = std::make_tuple((int)K.mvpMapPoints.size() - 1, -1);
        }
        if (k > 0) { K.mpParent = &kfs[k - 1]; kfs[k - 1].mspChildrens.insert(&K); K.mvpOrderedConnectedKeyFrames.push_back(&kfs[k - 1]); }
        if (k + 1 < 4) K.mvpOrderedConnectedKeyFrames.push_back(&kfs[k + 1]);
    }
    CovisibilityGraph<KeyFrame, MapPoint> graph(16, 8192);
    CHECK(graph.ok(), "store");
    std::vector<KeyFrame *> allKfs;
    std::vector<MapPoint *> allPts;
    for (auto &k : kfs) allKfs.push_back(&k);
    for (auto &m : mps) allPts.push_back(&m);
    for (KeyFrame *k : allKfs) CHECK(graph.Sync(k) == RUMI_OK, "Sync(KeyFrame)");
    for (MapPoint *p : allPts) CHECK(graph.Sync(p) == RUMI_OK, "Sync(MapPoint)");
    CHECK(graph.SyncAttributes(allPts) == RUMI_OK, "SyncAttributes");
    const float T7[7] = {0, 0, 0, 1, 0, 0, 0};

    auto motion = [&](Frame &F, rumi_facade::TrackStep &st, std::vector<MapPoint *> &discarded) {
        rumi_facade::ExtractFrame(F, image1, ext, 4096);
        const bool ok = rumi_facade::TrackWithMotionModel(F, F0, T7, 15.f, &st);
        for (auto &m : mps) if (m.mnLastFrameSeen == F.mnId) discarded.push_back(&m);
        return ok;
    };
    // ---- (a) the two-step path: UpdateLocalMap() + TrackLocalMap
    reset(mps, kfs);
    Frame F1; F1.mnId = 31;
    rumi_facade::TrackStep s1;
    std::vector<MapPoint *> d1, lp1;
    std::vector<KeyFrame *> lk1;
    KeyFrame *ref1 = nullptr;
    CHECK(motion(F1, s1, d1), "TrackWithMotionModel succeeds on the scene");
    CHECK(graph.UpdateLocalMap(F1, lk1, lp1, ref1) == RUMI_OK, "UpdateLocalMap");
    const int in1 = rumi_facade::TrackLocalMap(F1, lp1, 1.f, false, 50.f, &s1);
    const State A = snapshot(F1, mps, kfs, lk1, lp1, ref1, in1);
    // ---- (b) the resident path on the same inputs
    reset(mps, kfs);
    Frame F2; F2.mnId = 31;
    rumi_facade::TrackStep s2;
    std::vector<MapPoint *> d2, lp2;
    std::vector<KeyFrame *> lk2;
    KeyFrame *ref2 = nullptr;
    CHECK(motion(F2, s2, d2) && d2 == d1, "the same motion step");
    const int in2 = rumi_facade::TrackLocalMapResident(F2, graph, d2, lk2, lp2, ref2, 1.f, false, 50.f, &s2);
    const State B = snapshot(F2, mps, kfs, lk2, lp2, ref2, in2);
    CHECK(in1 > 100 && in2 == in1 && s2.nToMatch == s1.nToMatch && s2.nmatchesLocal == s1.nmatchesLocal && s2.ngoodLocal == s1.ngoodLocal && s1.nmatchesLocal > 20, "the numbers TrackLocalMap decides on");
    CHECK(A.lk == B.lk && A.lk.size() >= 2 && A.lp == B.lp && A.lp.size() > 300 && A.ref == B.ref && A.ref && A.frameRef == B.frameRef, "mvpLocalKeyFrames, mvpLocalMapPoints, mpReferenceKF");
    CHECK(A.mp == B.mp && A.outl == B.outl && std::memcmp(A.T, B.T, 28) == 0, "the frame: mvpMapPoints, mvbOutlier, pose");
    CHECK(A.kfRef == B.kfRef, "mnTrackReferenceForFrame of the key-frames");
    int diff = 0, inView = 0, bads = 0;
    for (size_t i = 0; i < A.pts.size(); i++) { diff += !(A.pts[i] == B.pts[i]); inView += B.pts[i].inView; }
    for (int i = 0; i < F1.N; i++) bads += F1.mvpMapPoints[i] && F1.mvpMapPoints[i]->bad;
    CHECK(diff == 0 && inView > 50 && bads == 0, "every MapPoint: mbTrackInView, mTrack*, visible / found counts, stamps");
    std::printf("resident == two-step: %zu local key-frames, %zu local points, %d in view, %d inliers, %zu discarded\n", B.lk.size(), B.lp.size(), inView, in2, d2.size());
    // ---- (c) SetWorldPos on one point: only that point is uploaded again, and it is the point the device then reads
    MapPoint *moved = nullptr;
    for (int i = 0; i < F2.N && !moved; i++) if (F2.mvpMapPoints[i] && !F2.mvbOutlier[i]) moved = F2.mvpMapPoints[i];
    CHECK(moved != nullptr, "a tracked point");
    auto again = [&](State *s) {
        reset(mps, kfs);
        Frame F; F.mnId = 32;
        rumi_facade::TrackStep st;
        std::vector<MapPoint *> d, lp; std::vector<KeyFrame *> lk; KeyFrame *ref = nullptr;
        motion(F, st, d);
        const int in = rumi_facade::TrackLocalMapResident(F, graph, d, lk, lp, ref, 1.f, false, 50.f, &st);
        *s = snapshot(F, mps, kfs, lk, lp, ref, in);
        return graph.LastUploadBytes();
    };
    State C0, C1, C2;
    const int64_t quiet = again(&C0);                                  // nothing dirty: the query's input alone
    moved->SetWorldPosXYZ(moved->pos.v[0] + 0.004f, moved->pos.v[1], moved->pos.v[2]);      // about a pixel: it stays an inlier
    graph.MarkDirty(moved);
    CHECK(graph.DirtyCount() == 1, "one dirty point");
    const int64_t one = again(&C1);
    // one edit record (16 bytes) and its 64-byte attribute record; the input block may grow by one discarded outlier (id, flag, projection: at
    // most 64 bytes with their alignment).  A second attribute record would add another 80.
    CHECK(graph.DirtyCount() == 0 && one >= quiet + 80 && one <= quiet + 80 + 64, "one attribute record travels, nothing else");
    // the two-step path reads the moved point from the MapPoint object: the same result
    reset(mps, kfs);
    Frame F3; F3.mnId = 32;
    rumi_facade::TrackStep s3;
    std::vector<MapPoint *> d3, lp3; std::vector<KeyFrame *> lk3; KeyFrame *ref3 = nullptr;
    motion(F3, s3, d3);
    graph.UpdateLocalMap(F3, lk3, lp3, ref3);
    const int in3 = rumi_facade::TrackLocalMap(F3, lp3, 1.f, false, 50.f, &s3);
    C2 = snapshot(F3, mps, kfs, lk3, lp3, ref3, in3);
    CHECK(C1.mp == C2.mp && C1.outl == C2.outl && std::memcmp(C1.T, C2.T, 28) == 0 && C1.inliers == C2.inliers, "after SetWorldPos: resident == two-step");
    CHECK(std::memcmp(C0.T, C1.T, 28) != 0, "the moved point changes the pose");
    std::printf("uploads: %lld bytes with nothing dirty, %lld with one point\n", (long long)quiet, (long long)one);
    CHECK(rumi_facade::last_status() == RUMI_OK, "no reported error");
    if (fails) { std::printf("%d FAILED\n", fails); return 1; }
    std::printf("localmap facade OK\n");
    return 0;
}
