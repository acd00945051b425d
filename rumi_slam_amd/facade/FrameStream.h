// Streaming front-end over a facade ORBextractor (include/rumi_orb.h, RumiOrbStream): one call per camera frame that does what
// ORBextractor::operator() does for it and brute-force matches it against the previous frame, which stays on the device.  What a Tracking-style
// caller writes as Frame::ExtractORB followed by a consecutive-frame match (INTEGRATION.md has the snippet).
#pragma once
#include <cassert>
#include <cstring>
#include <vector>

#include "ORBextractor.h"
#include "rumi_status.h"

namespace rumi_facade {

class FrameStream {
public:
    // The extractor must outlive the stream.  Between two pushes the extractor may be called as usual.
    explicit FrameStream(ORB_SLAM3::ORBextractor &extractor) : ext_(extractor) {}
    ~FrameStream() { rumi_orb_stream_destroy(stream_); }
    FrameStream(const FrameStream &) = delete;
    FrameStream &operator=(const FrameStream &) = delete;

    // Returns what operator() returns (monoIndex; -1 for an empty image or after a reported failure) and fills key-points and descriptors as it
    // does; bestIdx[i] = the previous frame's key-point nearest to key-point i in Hamming distance (first index wins ties), -1 without a
    // previous frame or at distance 256; bestDist / secondDist: its distance and the runner-up's.  A frame larger than any before re-creates the
    // extractor's handle: it is then matched as a first frame.
    int Push(cv::InputArray _image, std::vector<cv::KeyPoint> &_keypoints, cv::OutputArray _descriptors, std::vector<int> &vLappingArea,
             std::vector<int> &bestIdx, std::vector<int> &bestDist, std::vector<int> &secondDist) {
        bestIdx.clear(); bestDist.clear(); secondDist.clear();
        if (_image.empty()) return -1;
        cv::Mat image = _image.getMat();
        assert(image.type() == CV_8UC1);
        if (!ext_.rumiHandleFits(image.cols, image.rows)) { rumi_orb_stream_destroy(stream_); stream_ = nullptr; }    // (before the handle it hangs on goes)
        RumiOrb *h = ext_.rumiHandle(image.cols, image.rows);
        if (!h) { _keypoints.clear(); _descriptors.release(); return -1; }
        if (!stream_) {
            const int rc = rumi_orb_stream_create(h, &stream_);
            if (rc != RUMI_OK) { report("FrameStream: rumi_orb_stream_create", rc); stream_ = nullptr; _keypoints.clear(); _descriptors.release(); return -1; }
        }
        RumiStreamFrame f;
        const int rc = rumi_orb_stream_push(stream_, image.data, image.cols, image.rows, (int)image.step, vLappingArea[0], vLappingArea[1], &f);
        if (rc == RUMI_E_EMPTY) return -1;
        if (rc != RUMI_OK) {                                    // reported (rumi_status.h); the frame gets no key-points -- no CPU fallback
            report("FrameStream::Push", rc);
            _keypoints.clear(); _descriptors.release();
            return -1;
        }
        static_assert(sizeof(cv::KeyPoint) == sizeof(RumiKeyPoint), "cv::KeyPoint must be the 28-byte POD");
        nPrev_ = f.n_prev;
        _keypoints.resize(f.n);
        if (f.n > 0) std::memcpy(static_cast<void *>(_keypoints.data()), f.kp, (size_t)f.n * sizeof(RumiKeyPoint));
        if (f.n == 0) _descriptors.release();
        else {
            _descriptors.create(f.n, 32, CV_8U);
            cv::Mat d = _descriptors.getMat();
            for (int i = 0; i < f.n; i++) std::memcpy(d.ptr(i), f.desc + (size_t)i * 32, 32);
        }
        bestIdx.assign(f.best_idx, f.best_idx + f.n); bestDist.assign(f.best_dist, f.best_dist + f.n); secondDist.assign(f.second_dist, f.second_dist + f.n);
        return f.mono;
    }

    // Forget the previous frame: the next Push is matched as a first frame.
    void Reset() { if (stream_) rumi_orb_stream_reset(stream_); }
    // Key-points of the frame the last Push was matched against (0: none).
    int PreviousCount() const { return nPrev_; }
    // The current frame where it lies on the device (rumi_orb_stream_resident); false before the first Push.
    bool Resident(void **d_kp, void **d_desc, void **d_counts) { return stream_ && rumi_orb_stream_resident(stream_, d_kp, d_desc, d_counts) == RUMI_OK; }

private:
    ORB_SLAM3::ORBextractor &ext_;
    RumiOrbStream *stream_ = nullptr;
    int nPrev_ = 0;
};

}  // namespace rumi_facade
