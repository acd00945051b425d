// The facade KFDSample (facade/KFDSample.h) over the mock cv types (facade/cv_shim.h):
//   test_kfd_facade W H decisions f0.bin t0 f1.bin t1 ...
// drives Step over the frames (W x H, 8-bit grey) with their timestamps; `decisions` is the oracle's string of 0 / 1, one per frame.  Checked: every
// decision, GetAllKF().size() and GetKF() after each step, the C entry (rumi_kfd_step on a handle of its own) step by step, Reset, an empty image.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "KFDSample.h"

static int failures = 0;
#define CHECK(c, what) do { if (!(c)) { std::printf("FAIL %s (line %d)\n", what, __LINE__); failures++; } else std::printf("ok   %s\n", what); } while (0)

int main(int argc, char **argv) {
    if (argc < 6 || (argc - 4) % 2) { std::printf("usage: test_kfd_facade W H decisions f0.bin t0 ...\n"); return 2; }
    const int W = std::atoi(argv[1]), H = std::atoi(argv[2]);
    const std::string want = argv[3];
    const int nf = (argc - 4) / 2;
    if ((int)want.size() != nf) { std::printf("one decision per frame\n"); return 2; }
    std::vector<std::vector<uint8_t>> im(nf, std::vector<uint8_t>((size_t)W * H));
    std::vector<double> t(nf);
    for (int k = 0; k < nf; k++) {
        FILE *f = std::fopen(argv[4 + 2 * k], "rb");
        if (!f || std::fread(im[k].data(), 1, im[k].size(), f) != im[k].size()) { std::printf("cannot read %s\n", argv[4 + 2 * k]); return 2; }
        std::fclose(f);
        t[k] = std::atof(argv[5 + 2 * k]);
    }
    const float Kp = 0.8f, Kd = 0.005f, th = 1.5f;
    cv::Mat none;
    KFDSample sampler(300, 4, 20, 7, 1.2f, none, 0.f);
    sampler.SetPDKFselectorParams(Kp, Kd, th);

    // the C entries on a handle of their own
    ORB_SLAM3::ORBextractor plain(300, 1.2f, 4, 20, 7);
    RumiOrb *h = nullptr;
    RumiOrbConfig cfg = plain.rumiConfig(W, H);
    if (rumi_orb_create(&cfg, &h) != RUMI_OK) { std::printf("rumi_orb_create: %s\n", rumi_last_error()); return 2; }
    RumiKfd *cs = nullptr;
    if (rumi_kfd_create(h, &cs) != RUMI_OK) { std::printf("rumi_kfd_create: %s\n", rumi_last_error()); return 2; }
    rumi_kfd_set_pd(cs, Kp, Kd, th);

    bool decisions = true, sizes = true, same = true, lastKF = true;
    size_t selected = 0;
    for (int k = 0; k < nf; k++) {
        cv::Mat image(H, W, CV_8UC1, im[k].data(), (size_t)W);
        const bool sel = sampler.Step(image, t[k]);
        RumiKfdStep r;
        const int rc = rumi_kfd_step(cs, im[k].data(), W, H, W, 1, t[k], &r);
        decisions = decisions && sel == (want[k] == '1');
        selected += sel;
        sizes = sizes && sampler.GetAllKF().size() == selected;
        const float flow = sampler.rumiLastFlow();
        same = same && rc == RUMI_OK && sel == (r.selected != 0) && (int)sampler.rumiLastNext().size() == r.n_tracked && std::memcmp(&r.moptf, &flow, 4) == 0;
        for (int i = 0; same && i < r.n_tracked; i++)
            same = sampler.rumiLastNext()[i].x == r.next[2 * i] && sampler.rumiLastNext()[i].y == r.next[2 * i + 1] && sampler.rumiLastStatus()[i] == r.status[i];
        if (sel) {
            cv::Mat kf = sampler.GetKF();
            lastKF = lastKF && kf.rows == H && kf.cols == W && kf.data != im[k].data();
            for (int y = 0; lastKF && y < H; y++) lastKF = std::memcmp(kf.ptr(y), im[k].data() + (size_t)y * W, (size_t)W) == 0;
        }
    }
    CHECK(decisions, "Step: every decision is the oracle's");
    CHECK(selected >= 2 && selected < (size_t)nf, "the sequence has selecting and non-selecting steps");
    CHECK(sizes, "GetAllKF().size() counts the selected frames");
    CHECK(lastKF, "GetKF() is a host copy of the last selected frame");
    CHECK(same, "Step: decision, tracked points, status and mean flow = the C entry's");
    {
        const size_t before = sampler.GetAllKF().size();
        CHECK(!sampler.Step(none, 99.0) && sampler.GetAllKF().size() == before && rumi_facade::last_status() == RUMI_E_EMPTY, "Step: an empty image selects nothing and is reported");
        rumi_facade::clear_status();
        sampler.Reset();
        cv::Mat image(H, W, CV_8UC1, im[1].data(), (size_t)W);
        CHECK(sampler.Step(image, 100.0) && sampler.GetAllKF().size() == before + 1 && sampler.rumiLastNext().empty(), "Reset: the next frame is a first frame");
    }
    CHECK(rumi_facade::last_status() == RUMI_OK, "no status reported");
    rumi_kfd_destroy(cs);
    rumi_orb_destroy(h);
    std::printf(failures ? "%d FAILURES\n" : "all facade KFDSample checks passed\n", failures);
    return failures ? 1 : 0;
}
