// rumi_facade::FrameStream over the mock cv types (facade/cv_shim.h): three frames of argv[1..3] (320 x 240, 8-bit), Push against the C entries
// (rumi_orb_stream_push on a second handle) and against ORBextractor::operator() between the pushes; an empty image; Reset.
#include <cstdio>
#include <cstring>
#include <vector>

#include "FrameStream.h"

static int failures = 0;
#define CHECK(c, what) do { if (!(c)) { std::printf("FAIL %s (line %d)\n", what, __LINE__); failures++; } else std::printf("ok   %s\n", what); } while (0)

int main(int argc, char **argv) {
    const int W = 320, H = 240;
    if (argc < 4) { std::printf("usage: test_stream_facade f0.bin f1.bin f2.bin\n"); return 2; }
    std::vector<std::vector<uint8_t>> im(3, std::vector<uint8_t>((size_t)W * H));
    for (int k = 0; k < 3; k++) {
        FILE *f = std::fopen(argv[1 + k], "rb");
        if (!f || std::fread(im[k].data(), 1, im[k].size(), f) != im[k].size()) { std::printf("cannot read %s\n", argv[1 + k]); return 2; }
        std::fclose(f);
    }
    std::vector<int> lap = {0, 1000};
    ORB_SLAM3::ORBextractor ext(500, 1.2f, 8, 20, 7), plain(500, 1.2f, 8, 20, 7);
    rumi_facade::FrameStream fs(ext);

    // the C entries on a handle of their own
    RumiOrb *h = nullptr;
    RumiOrbConfig cfg = plain.rumiConfig(W, H);
    if (rumi_orb_create(&cfg, &h) != RUMI_OK) { std::printf("rumi_orb_create: %s\n", rumi_last_error()); return 2; }
    RumiOrbStream *cs = nullptr;
    if (rumi_orb_stream_create(h, &cs) != RUMI_OK) { std::printf("rumi_orb_stream_create: %s\n", rumi_last_error()); return 2; }

    int prevN = 0;
    for (int k = 0; k < 3; k++) {
        cv::Mat image(H, W, CV_8UC1, im[k].data(), (size_t)W), desc, desc2;
        std::vector<cv::KeyPoint> kps, kps2;
        std::vector<int> bi, bd, sd;
        const int mono = fs.Push(image, kps, desc, lap, bi, bd, sd);
        RumiStreamFrame f;
        const int rc = rumi_orb_stream_push(cs, im[k].data(), W, H, W, 0, 1000, &f);
        CHECK(rc == RUMI_OK && mono == f.mono && (int)kps.size() == f.n && f.n > 100, "Push: return value and count = the C entry's");
        CHECK(fs.PreviousCount() == prevN && f.n_prev == prevN, "Push: matched against the previous frame's count");
        bool same = desc.rows == f.n && desc.cols == 32 && (int)bi.size() == f.n && (int)bd.size() == f.n && (int)sd.size() == f.n;
        for (int i = 0; same && i < f.n; i++)
            same = std::memcmp(&kps[i], &f.kp[i], sizeof(RumiKeyPoint)) == 0 && std::memcmp(desc.ptr(i), f.desc + (size_t)i * 32, 32) == 0 && bi[i] == f.best_idx[i] &&
                   bd[i] == f.best_dist[i] && sd[i] == f.second_dist[i];
        CHECK(same, "Push: key-points, descriptors and the three match rows = the C entry's");
        int matched = 0;
        for (int i = 0; i < f.n; i++) matched += bi[i] >= 0 && bi[i] < prevN;
        CHECK(k == 0 ? matched == 0 : matched == f.n, "Push: every index points into the previous frame (none on the first)");
        // operator() on the stream's own extractor between two pushes: same features, and the next push is not disturbed (checked by the next round)
        const int mono2 = ext(image, cv::Mat(), kps2, desc2, lap);
        bool same2 = mono2 == mono && kps2.size() == kps.size() && desc2.rows == desc.rows;
        for (size_t i = 0; same2 && i < kps.size(); i++) same2 = std::memcmp(&kps[i], &kps2[i], sizeof(cv::KeyPoint)) == 0 && std::memcmp(desc.ptr((int)i), desc2.ptr((int)i), 32) == 0;
        CHECK(same2, "operator() between two pushes = Push's features");
        prevN = f.n;
    }
    {   // an empty image: -1, nothing written, the previous frame stays
        cv::Mat none, desc;
        std::vector<cv::KeyPoint> kps;
        std::vector<int> bi, bd, sd;
        CHECK(fs.Push(none, kps, desc, lap, bi, bd, sd) == -1 && kps.empty() && bi.empty(), "Push: empty image returns -1");
        cv::Mat image(H, W, CV_8UC1, im[0].data(), (size_t)W);
        fs.Push(image, kps, desc, lap, bi, bd, sd);
        CHECK(fs.PreviousCount() == prevN, "Push after an empty image: still matched against the last good frame");
        fs.Reset();
        fs.Push(image, kps, desc, lap, bi, bd, sd);
        bool none256 = !bi.empty();
        for (size_t i = 0; i < bi.size(); i++) none256 = none256 && bi[i] == -1 && bd[i] == 256 && sd[i] == 256;
        CHECK(fs.PreviousCount() == 0 && none256, "Reset: the next frame is a first frame");
        void *a = nullptr, *b = nullptr, *c = nullptr;
        CHECK(fs.Resident(&a, &b, &c) && a && b && c, "Resident: device pointers of the current frame");
    }
    CHECK(rumi_facade::last_status() == RUMI_OK, "no status reported");
    rumi_orb_stream_destroy(cs);
    rumi_orb_destroy(h);
    std::printf(failures ? "%d FAILURES\n" : "all facade stream checks passed\n", failures);
    return failures ? 1 : 0;
}
