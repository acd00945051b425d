// Drop-in KFDSample over the MI355X C ABI (include/rumi_kfd.h): the PD frame selector of the rumination path.
// Same public members as R/include/cloud_edge_slam_lib/KFDSample.h:55-84; CloudImageSampler.cc (new KFDSample(), SetPDKFselectorParams, Step,
// Reset) compiles against it unchanged.  Step does on the device what the reference does with cv::calcOpticalFlowPyrLK, the PD controller and
// ORBextractor::operator() on the CPU; the frame is uploaded once.  No CPU fallback: a failing device call is reported (rumi_status.h) and Step
// returns false.
#pragma once
#include <iostream>
#include <vector>

#include "ORBextractor.h"
#include "rumi_kfd.h"
#include "rumi_status.h"

// (the reference's header opens both namespaces for everything that includes it, CloudImageSampler.h among them)
using namespace cv;
using namespace std;

inline void Printinfo(float Kp, float Kd, float setpoint) {
    cout << endl << "KeyFrame PD Selector Parameters: " << endl;
    cout << "- Kp: " << Kp << endl;
    cout << "- Kd: " << Kd << endl;
    cout << "- Setpoint" << setpoint << endl;
}

class KFDSample {
private:
    // Tracking points of the last step (old: before it, next / status: its result)
    vector<Point2f> old, next, good_old, good_next;
    ORB_SLAM3::ORBextractor *mpORBextractor = nullptr;
    // ORBextractor parameters, default for the TUM1 dataset
    float scaleFactor = 1.2f;
    int nfeatures = 2000, nlevels = 8, iniThFAST = 20, minThFAST = 7;
    // PD controller parameters
    float Kp = 0.8f, Kd = 0.005f;
    vector<KeyPoint> mvKeys;
    Mat mDescriptors;
    Mat frame2, imnext;
    double ltframe = 0;
    float moptf = 0, th = 10;
    vector<unsigned char> status;
    bool show = false;
    vector<Mat> KFset;
    vector<int> vLapping = {0, 0};
    RumiKfd *kfd_ = nullptr;

    // the sampler hangs on the extractor's handle: a frame larger than any before re-creates that handle, and the sampler with it (as a first step)
    RumiKfd *sampler(int cols, int rows) {
        if (kfd_ && !mpORBextractor->rumiHandleFits(cols, rows)) { rumi_kfd_destroy(kfd_); kfd_ = nullptr; }
        RumiOrb *h = mpORBextractor->rumiHandle(cols, rows);
        if (!h) return nullptr;
        if (!kfd_) {
            const int rc = rumi_kfd_create(h, &kfd_);
            if (rc != RUMI_OK) { rumi_facade::report("KFDSample: rumi_kfd_create", rc); kfd_ = nullptr; return nullptr; }
            rumi_kfd_set_pd(kfd_, Kp, Kd, th);
        }
        return kfd_;
    }

    // the grey frame a selected frame leaves in KFset (KFDSample.cc:115,155)
    static Mat greyCopy(const Mat &im, int channels) {
        if (channels == 1) return im.clone();
        Mat g(im.rows, im.cols, CV_8UC1);
        for (int y = 0; y < im.rows; y++) {
            const uint8_t *q = im.ptr(y);
            uint8_t *o = g.ptr(y);
            for (int x = 0; x < im.cols; x++, q += 3) o[x] = (uint8_t)((1868 * q[0] + 9617 * q[1] + 4899 * q[2] + 8192) >> 14);
        }
        return g;
    }

public:
    KFDSample(int nfeatures_, int nlevels_, int iniThFAST_, int minThFAST_, float scaleFactor_, Mat & /*Frame*/, float TimeStamp) {
        nfeatures = nfeatures_; minThFAST = minThFAST_; nlevels = nlevels_; iniThFAST = iniThFAST_; scaleFactor = scaleFactor_;
        InitORBextractor(nfeatures, scaleFactor, nlevels, iniThFAST, minThFAST);
        ltframe = TimeStamp;
    }
    KFDSample() {
        InitORBextractor(nfeatures, scaleFactor, nlevels, iniThFAST, minThFAST);
        InitPDKFselector();
    }
    ~KFDSample() { rumi_kfd_destroy(kfd_); delete mpORBextractor; }
    KFDSample(const KFDSample &) = delete;
    KFDSample &operator=(const KFDSample &) = delete;

    void InitORBextractor(const int nfeatures_, const float scaleFactor_, const int nlevels_, const int iniThFAST_, const int minThFAST_) {
        rumi_kfd_destroy(kfd_); kfd_ = nullptr;
        delete mpORBextractor;
        mpORBextractor = new ORB_SLAM3::ORBextractor(nfeatures_, scaleFactor_, nlevels_, iniThFAST_, minThFAST_);
    }
    void InitPDKFselector(float Kp_, float Kd_, float th_) { SetPDKFselectorParams(Kp_, Kd_, th_); Printinfo(Kp_, Kd_, th_); }
    void InitPDKFselector() { SetPDKFselectorParams(Kp, Kd, th); }
    void SetPDKFselectorParams(float Kp_, float Kd_, float th_) {
        Kp = Kp_; Kd = Kd_; th = th_;
        if (kfd_) rumi_kfd_set_pd(kfd_, Kp, Kd, th);
    }

    Mat GetKF() { return KFset.back(); }
    vector<Mat> GetAllKF() { return KFset; }
    void SetThreshold(const float TH) { th = TH; }          // (as in the reference: the controller's setpoint changes with the next SetPDKFselectorParams)
    void SetDisplay() { show = true; }                       // (no display on the device path)
    void SetNextFrame(const Mat &InputArray) { frame2 = InputArray.clone(); imnext = frame2; }
    void SelectGoodPts() {
        for (size_t i = 0; i < old.size() && i < status.size(); i++)
            if (status[i] == 1) { good_next.push_back(next[i]); good_old.push_back(old[i]); }
    }
    void Reset() {
        old.clear();
        if (kfd_) rumi_kfd_reset(kfd_);
    }

    bool Step(const Mat &inputIm, double timeStamp) {
        if (inputIm.empty()) { rumi_facade::report("KFDSample::Step", RUMI_E_EMPTY, "empty image"); return false; }
        int channels = 1;
#ifdef RUMI_HAVE_OPENCV
        if (inputIm.type() == CV_8UC3) channels = 3;
        else if (inputIm.type() != CV_8UC1) { cerr << "error image type" << endl; return false; }
#endif
        RumiKfd *s = sampler(inputIm.cols, inputIm.rows);
        if (!s) return false;
        RumiKfdStep r;
        const int rc = rumi_kfd_step(s, inputIm.data, inputIm.cols, inputIm.rows, (int)inputIm.step, channels, timeStamp, &r);
        if (rc != RUMI_OK) { rumi_facade::report("KFDSample::Step", rc); return false; }
        static_assert(sizeof(KeyPoint) == sizeof(RumiKeyPoint), "cv::KeyPoint must be the 28-byte POD");
        next.resize(r.n_tracked); status.assign(r.status, r.status + r.n_tracked);
        for (int i = 0; i < r.n_tracked; i++) { next[i].x = r.next[2 * i]; next[i].y = r.next[2 * i + 1]; }
        moptf = r.moptf;
        if (r.selected) {
            mvKeys.resize(r.n);
            if (r.n > 0) std::memcpy(static_cast<void *>(mvKeys.data()), r.kp, (size_t)r.n * sizeof(RumiKeyPoint));
            if (r.n == 0) mDescriptors.release();
            else {
                mDescriptors.create(r.n, 32, CV_8U);
                for (int i = 0; i < r.n; i++) std::memcpy(mDescriptors.ptr(i), r.desc + (size_t)i * 32, 32);
            }
            old.resize(r.n);
            for (int i = 0; i < r.n; i++) old[i] = mvKeys[i].pt;                 // KeyPoint::convert
            KFset.push_back(greyCopy(inputIm, channels));
        } else old = next;
        ltframe = timeStamp;
        good_next.clear(); good_old.clear();
        return r.selected != 0;
    }

    // facade-only: the last step's mean flow magnitude, tracked points and status bytes
    float rumiLastFlow() const { return moptf; }
    const vector<Point2f> &rumiLastNext() const { return next; }
    const vector<unsigned char> &rumiLastStatus() const { return status; }
};
