/*
 * rumi_kfd.h — C ABI of the PD frame selector (librumi_hip.so): KFDSample::Step on the device.
 *
 * Drop-in boundary for the reference class KFDSample (R/ = the reference's src/rumi-slam/):
 *   R/include/cloud_edge_slam_lib/KFDSample.h:55-84      class surface
 *   R/lib_src/KFDSample.cc:87-175                         Step: calcOpticalFlowPyrLK (31 x 31, maxLevel 2, 20 iterations or eps 0.03) on the
 *                                                         previous selection's key-points, mean flow magnitude, PD threshold, re-extraction
 *   R/include/cloud_edge_slam_lib/pd.hpp:21-39            PD::update
 * While tracking is lost CloudImageSampler::TrackStep (R/lib_src/CloudImageSampler.cc:46-54) hands every camera frame to Step.
 *
 * The flow is the published pyramidal Lucas-Kanade as OpenCV implements it, with the window sums kept as exact integers; its definition is the scalar
 * oracle tests/cpp/kfd_oracle.cc, which the device matches bit for bit (DESIGN.md sections 4n and 7: parity with the OpenCV binary is unpinned).
 * Conventions (status codes, rumi_last_error, threading): rumi_orb.h.
 */
#ifndef RUMI_KFD_H
#define RUMI_KFD_H

#include "rumi_orb.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct RumiKfd RumiKfd;

/* What one step decided and tracked.  The pointers go into pinned host memory: next / status stay valid until the next step on this sampler, kp / desc
 * until the next call on the sampler's extractor. */
typedef struct RumiKfdStep {
    int32_t selected;                 /* Step's return value: the frame enters the queue */
    int32_t n_tracked, n_good;        /* points handed to the flow (0 on a first step), points with status 1 */
    float moptf, pd_out, th;          /* mean flow magnitude of the good points (NaN without one), PD::update's output, TH = moptf + pd_out (0 on a first step) */
    const float *next;                /* [n_tracked][2] */
    const uint8_t *status;            /* [n_tracked] */
    int32_t n, mono;                  /* selected frames only: what rumi_orb_extract(lap 0, 0) returns for this frame ... */
    const RumiKeyPoint *kp;           /* ... [n] */
    const uint8_t *desc;              /* ... [n][32] */
} RumiKfdStep;

/* A sampler on extractor `h` (KFDSample::InitORBextractor: ORBextractor(2000, 1.2, 8, 20, 7) in the reference), which re-extracts the selected frames
 * and bounds the frame size (cfg.max_width x max_height, at least 128 x 128).  PD gains start at the reference's Kp 0.8, Kd 0.005, th 10.  Two frame
 * slots (three LK levels each) and their Scharr derivatives stay on the device.  Not concurrent with other use of `h`; destroy the sampler first. */
int rumi_kfd_create(RumiOrb *h, RumiKfd **out);
void rumi_kfd_destroy(RumiKfd *s);
/* KFDSample::SetPDKFselectorParams */
int rumi_kfd_set_pd(RumiKfd *s, float kp, float kd, float th);
/* KFDSample::Reset: forgets the tracked points (the next step is a first step); the controller keeps its previous input. */
int rumi_kfd_reset(RumiKfd *s);

/* KFDSample::Step(image, timestamp).  `img`: 8-bit grey (channels 1) or BGR (channels 3, converted as cv::cvtColor does), `stride` bytes per row,
 * at least 128 x 128 and at most the extractor's size; the size may only change on a first step.  The frame crosses to the device once: the flow's
 * level 0 is what the extractor reads on a selected frame.
 *   first step (none yet, or after a reset, or after a selected frame without key-points): the frame is extracted with lap {0, 0}, its key-points become
 *     the tracked points, selected = 1, no PD update;
 *   otherwise: the tracked points are followed from the previous frame into this one; moptf = the float sum, in index order, of the good points' flow
 *     magnitudes over their count (0 / 0 = NaN without a good point: NaN never selects and stays in the controller as its previous input, as in the
 *     reference); TH = moptf + PD::update(moptf, timestamp - previous timestamp); moptf > TH selects: the frame is extracted and its key-points become
 *     the tracked points; otherwise ALL next points, failed ones included, become the tracked points.
 * RUMI_E_EMPTY for an empty image, RUMI_E_INVALID for a wrong size or channel count; a failing step leaves the sampler as it was. */
int rumi_kfd_step(RumiKfd *s, const uint8_t *img, int32_t w, int32_t hgt, int32_t stride, int32_t channels, double timestamp, RumiKfdStep *out);

/* The flow alone, without a sampler: n points `pts` [n][2] followed from host frame `prev` into host frame `cur` (both w x hgt, `channels` 1 or 3) on
 * device `device` (-1: the current one) -> next [n][2], status [n].  pyr_out / deriv_out (may be NULL): the three LK levels of `prev`, dense, one
 * behind the other (w x hgt, then ((w + 1) / 2) x ((hgt + 1) / 2), ...), and their interleaved int16 (dx, dy) Scharr derivatives.  For tests and
 * probes: device memory is taken and released inside the call. */
int rumi_kfd_track(int32_t device, const uint8_t *prev, const uint8_t *cur, int32_t w, int32_t hgt, int32_t stride, int32_t channels, const float *pts,
                   int32_t n, float *next, uint8_t *status, uint8_t *pyr_out, int16_t *deriv_out);

#ifdef __cplusplus
}
#endif
#endif /* RUMI_KFD_H */
