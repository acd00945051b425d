// Scalar oracle of KFDSample::Step (R/lib_src/KFDSample.cc:87-175): grey conversion, the three-level LK pyramid, Scharr derivatives, pyramidal
// Lucas-Kanade tracking (31 x 31 window, maxLevel 2, 20 iterations or eps 0.03) as OpenCV's calcOpticalFlowPyrLK implements it, the mean flow
// magnitude, the PD controller (R/include/cloud_edge_slam_lib/pd.hpp:21-39) and the step logic around them.  TEST INFRASTRUCTURE: no
// dependencies, built by the tests with g++ -O2 -ffp-contract=off.  This file is the DEFINITION the device path (rumi_slam_amd/csrc/flow.hip,
// orb_kfd.inc) is compared with bit for bit; OpenCV itself is not available, so parity with its binary is unpinned.
//
// Two deliberate differences from OpenCV, both so that host and device give the same bits: the five window sums (A11, A12, A22, b1, b2) are exact
// 64-bit integers converted to float once (OpenCV accumulates in float, which makes the result depend on the summation order), and a float that
// does not fit an int (or is NaN) floors to a value outside every image instead of being undefined.
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

namespace {

constexpr int kWin = 31, kHalf = 15, kLevels = 3, kMaxIter = 20;

inline int reflect101(int i, int n) {
    if (i < 0) i = -i;
    if (i >= n) i = 2 * n - 2 - i;
    return i;
}

// cvFloor with a defined result for what does not fit: far outside every image
inline int ifloor(float v) {
    const float f = std::floor(v);
    if (!(f >= -1073741824.f)) return -1073741824;          // (NaN lands here too)
    if (f > 1073741824.f) return 1073741824;
    return (int)f;
}

struct Image { const uint8_t *p; int w, h, pitch; };

void grey_bgr(const uint8_t *bgr, int w, int h, int stride, uint8_t *out) {
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++) {
            const uint8_t *q = bgr + (size_t)y * stride + 3 * x;
            out[(size_t)y * w + x] = (uint8_t)((1868 * q[0] + 9617 * q[1] + 4899 * q[2] + 8192) >> 14);
        }
}

void pyr_down(const uint8_t *src, int w, int h, uint8_t *dst) {
    static const int tap[5] = {1, 4, 6, 4, 1};
    const int w2 = (w + 1) / 2, h2 = (h + 1) / 2;
    for (int y = 0; y < h2; y++)
        for (int x = 0; x < w2; x++) {
            int sum = 0;
            for (int dy = -2; dy <= 2; dy++) {
                const uint8_t *row = src + (size_t)reflect101(2 * y + dy, h) * w;
                int rs = 0;
                for (int dx = -2; dx <= 2; dx++) rs += tap[dx + 2] * row[reflect101(2 * x + dx, w)];
                sum += tap[dy + 2] * rs;
            }
            dst[(size_t)y * w2 + x] = (uint8_t)((sum + 128) >> 8);
        }
}

// interleaved (dx, dy) int16
void scharr(const uint8_t *src, int w, int h, int16_t *out) {
    for (int y = 0; y < h; y++) {
        const uint8_t *r0 = src + (size_t)reflect101(y - 1, h) * w, *r1 = src + (size_t)y * w, *r2 = src + (size_t)reflect101(y + 1, h) * w;
        for (int x = 0; x < w; x++) {
            const int xl = reflect101(x - 1, w), xr = reflect101(x + 1, w);
            const int dx = 3 * (r0[xr] - r0[xl]) + 10 * (r1[xr] - r1[xl]) + 3 * (r2[xr] - r2[xl]);
            const int dy = 3 * (r2[xl] - r0[xl]) + 10 * (r2[x] - r0[x]) + 3 * (r2[xr] - r0[xr]);
            out[((size_t)y * w + x) * 2] = (int16_t)dx;
            out[((size_t)y * w + x) * 2 + 1] = (int16_t)dy;
        }
    }
}

struct Weights { int w00, w01, w10, w11; };
inline Weights weights(float a, float b) {
    Weights k;
    k.w00 = (int)std::rint((1.f - a) * (1.f - b) * 16384.f);
    k.w01 = (int)std::rint(a * (1.f - b) * 16384.f);
    k.w10 = (int)std::rint((1.f - a) * b * 16384.f);
    k.w11 = 16384 - k.w00 - k.w01 - k.w10;
    return k;
}

inline int img_at(const uint8_t *img, int w, int h, int x, int y) { return img[(size_t)reflect101(y, h) * w + reflect101(x, w)]; }
inline int der_at(const int16_t *d, int w, int h, int x, int y, int c) { return (x < 0 || x >= w || y < 0 || y >= h) ? 0 : d[((size_t)y * w + x) * 2 + c]; }

// I, Ix, Iy of the 31 x 31 window whose top-left pixel is (ix, iy), and the exact sums A11, A12, A22
void window_prev(const uint8_t *img, const int16_t *der, int w, int h, int ix, int iy, Weights k, int *I, int *Ix, int *Iy, int64_t A[3]) {
    A[0] = A[1] = A[2] = 0;
    for (int y = 0; y < kWin; y++)
        for (int x = 0; x < kWin; x++) {
            const int X = ix + x, Y = iy + y, i = y * kWin + x;
            I[i] = (img_at(img, w, h, X, Y) * k.w00 + img_at(img, w, h, X + 1, Y) * k.w01 + img_at(img, w, h, X, Y + 1) * k.w10 +
                    img_at(img, w, h, X + 1, Y + 1) * k.w11 + 256) >> 9;
            Ix[i] = (der_at(der, w, h, X, Y, 0) * k.w00 + der_at(der, w, h, X + 1, Y, 0) * k.w01 + der_at(der, w, h, X, Y + 1, 0) * k.w10 +
                     der_at(der, w, h, X + 1, Y + 1, 0) * k.w11 + 8192) >> 14;
            Iy[i] = (der_at(der, w, h, X, Y, 1) * k.w00 + der_at(der, w, h, X + 1, Y, 1) * k.w01 + der_at(der, w, h, X, Y + 1, 1) * k.w10 +
                     der_at(der, w, h, X + 1, Y + 1, 1) * k.w11 + 8192) >> 14;
            A[0] += (int64_t)Ix[i] * Ix[i];
            A[1] += (int64_t)Ix[i] * Iy[i];
            A[2] += (int64_t)Iy[i] * Iy[i];
        }
}

void window_next(const uint8_t *img, int w, int h, int ix, int iy, Weights k, const int *I, const int *Ix, const int *Iy, int64_t b[2]) {
    b[0] = b[1] = 0;
    for (int y = 0; y < kWin; y++)
        for (int x = 0; x < kWin; x++) {
            const int X = ix + x, Y = iy + y, i = y * kWin + x;
            const int diff = ((img_at(img, w, h, X, Y) * k.w00 + img_at(img, w, h, X + 1, Y) * k.w01 + img_at(img, w, h, X, Y + 1) * k.w10 +
                               img_at(img, w, h, X + 1, Y + 1) * k.w11 + 256) >> 9) - I[i];
            b[0] += (int64_t)diff * Ix[i];
            b[1] += (int64_t)diff * Iy[i];
        }
}

inline float sum_to_float(int64_t v) { return (float)(double)v * (1.f / (1 << 20)); }

struct Pyramid {
    int w[kLevels], h[kLevels];
    std::vector<uint8_t> img[kLevels];
    std::vector<int16_t> der[kLevels];
    void build(const uint8_t *grey, int w0, int h0, int stride) {
        w[0] = w0; h[0] = h0;
        img[0].resize((size_t)w0 * h0);
        for (int y = 0; y < h0; y++) std::memcpy(img[0].data() + (size_t)y * w0, grey + (size_t)y * stride, (size_t)w0);
        for (int l = 1; l < kLevels; l++) {
            w[l] = (w[l - 1] + 1) / 2; h[l] = (h[l - 1] + 1) / 2;
            img[l].resize((size_t)w[l] * h[l]);
            pyr_down(img[l - 1].data(), w[l - 1], h[l - 1], img[l].data());
        }
        for (int l = 0; l < kLevels; l++) { der[l].resize((size_t)w[l] * h[l] * 2); scharr(img[l].data(), w[l], h[l], der[l].data()); }
    }
};

// how a level ended (diag): code | iterations << 8
enum { kSkipBounds = 0, kGateMinEig = 1, kGateDet = 2, kLeftFrame = 3, kEpsBreak = 4, kOscillation = 5, kAllIterations = 6 };

void track(const Pyramid &P, const Pyramid &N, const float *pts, int n, float *next, uint8_t *status, int32_t *diag) {
    std::vector<int> I(kWin * kWin), Ix(kWin * kWin), Iy(kWin * kWin);
    for (int p = 0; p < n; p++) {
        float outx = 0, outy = 0;
        uint8_t st = 1;
        for (int level = kLevels - 1; level >= 0; level--) {
            const int W = P.w[level], H = P.h[level];
            const float s = 1.f / (float)(1 << level);
            float px = pts[2 * p] * s, py = pts[2 * p + 1] * s, nx, ny;
            if (level == kLevels - 1) { nx = px; ny = py; }
            else { nx = outx * 2.f; ny = outy * 2.f; }
            outx = nx; outy = ny;
            px -= (float)kHalf; py -= (float)kHalf;
            const int ipx = ifloor(px), ipy = ifloor(py);
            if (ipx < -kWin || ipx >= W || ipy < -kWin || ipy >= H) {
                if (level == 0) st = 0;
                if (diag) diag[3 * p + level] = kSkipBounds;
                continue;
            }
            int64_t A[3];
            window_prev(P.img[level].data(), P.der[level].data(), W, H, ipx, ipy, weights(px - (float)ipx, py - (float)ipy), I.data(), Ix.data(), Iy.data(), A);
            const float A11 = sum_to_float(A[0]), A12 = sum_to_float(A[1]), A22 = sum_to_float(A[2]);
            float D = A11 * A22 - A12 * A12;
            const float minEig = (A22 + A11 - std::sqrt((A11 - A22) * (A11 - A22) + 4.f * A12 * A12)) / (float)(2 * kWin * kWin);
            if (minEig < 1e-4f || D < FLT_EPSILON) {
                if (level == 0) st = 0;
                if (diag) diag[3 * p + level] = minEig < 1e-4f ? kGateMinEig : kGateDet;
                continue;
            }
            D = 1.f / D;
            nx -= (float)kHalf; ny -= (float)kHalf;
            float pdx = 0, pdy = 0;
            int code = kAllIterations, j = 0;
            for (; j < kMaxIter; j++) {
                const int inx = ifloor(nx), iny = ifloor(ny);
                if (inx < -kWin || inx >= W || iny < -kWin || iny >= H) {
                    if (level == 0) st = 0;
                    code = kLeftFrame;
                    break;
                }
                int64_t b[2];
                window_next(N.img[level].data(), W, H, inx, iny, weights(nx - (float)inx, ny - (float)iny), I.data(), Ix.data(), Iy.data(), b);
                const float b1 = sum_to_float(b[0]), b2 = sum_to_float(b[1]);
                const float dx = (A12 * b2 - A22 * b1) * D, dy = (A12 * b1 - A11 * b2) * D;
                nx += dx; ny += dy;
                outx = nx + (float)kHalf; outy = ny + (float)kHalf;
                if ((double)dx * (double)dx + (double)dy * (double)dy <= 0.03 * 0.03) { code = kEpsBreak; j++; break; }      // Point2f::ddot is double
                if (j > 0 && (double)std::fabs(dx + pdx) < 0.01 && (double)std::fabs(dy + pdy) < 0.01) {
                    outx -= dx * 0.5f; outy -= dy * 0.5f;
                    code = kOscillation; j++;
                    break;
                }
                pdx = dx; pdy = dy;
            }
            if (diag) diag[3 * p + level] = code | (j << 8);
        }
        next[2 * p] = outx; next[2 * p + 1] = outy;
        status[p] = st;
    }
}

// pd.hpp:21-39 with the constructor defaults PD(kp, kd): Alpha 1, maxOutput 255
struct PD {
    float maxOutput = 255, kp = 1, kd = 0, prevInput = 0, setpoint = 0, Alpha = 1;
    float update(float input, double Ts) {
        float error = setpoint - input;
        float diff = Alpha * (prevInput - input);
        prevInput -= diff;
        float output = kp * error + kd / Ts * diff;
        if (output > maxOutput) output = maxOutput;
        return output;
    }
};

struct Sampler {
    PD pd;
    std::vector<float> old, next;
    std::vector<uint8_t> status;
    Pyramid prev;
    double ltframe = 0;
};

}  // namespace

extern "C" {

struct KfoStep { int32_t selected, n_tracked, n_good; float moptf, pd_out, th; };

void kfo_grey_bgr(const uint8_t *bgr, int w, int h, int stride, uint8_t *out) { grey_bgr(bgr, w, h, stride, out); }
void kfo_pyr_down(const uint8_t *src, int w, int h, uint8_t *dst) { pyr_down(src, w, h, dst); }
void kfo_scharr(const uint8_t *src, int w, int h, int16_t *out) { scharr(src, w, h, out); }

// the window at float position (px, py) = top-left corner: I, Ix, Iy [961] and A [3]; then b [2] of the window of `next_img` at (nx, ny)
void kfo_window(const uint8_t *img, const int16_t *der, const uint8_t *next_img, int w, int h, float px, float py, float nx, float ny, int32_t *I, int32_t *Ix,
                int32_t *Iy, int32_t *wts, int64_t *A, int64_t *b) {
    const int ipx = ifloor(px), ipy = ifloor(py), inx = ifloor(nx), iny = ifloor(ny);
    const Weights k = weights(px - (float)ipx, py - (float)ipy);
    wts[0] = k.w00; wts[1] = k.w01; wts[2] = k.w10; wts[3] = k.w11;
    window_prev(img, der, w, h, ipx, ipy, k, I, Ix, Iy, A);
    const Weights kn = weights(nx - (float)inx, ny - (float)iny);
    wts[4] = kn.w00; wts[5] = kn.w01; wts[6] = kn.w10; wts[7] = kn.w11;
    window_next(next_img, w, h, inx, iny, kn, I, Ix, Iy, b);
}

// pyramids of both frames (dense grey, w x h), then the track; pyr_out / der_out (may be null): the three levels of `prev`, packed one behind the other
void kfo_track(const uint8_t *prev, const uint8_t *cur, int w, int h, const float *pts, int n, float *next, uint8_t *status, int32_t *diag, uint8_t *pyr_out,
               int16_t *der_out) {
    Pyramid P, N;
    P.build(prev, w, h, w);
    N.build(cur, w, h, w);
    track(P, N, pts, n, next, status, diag);
    for (int l = 0; l < kLevels; l++) {
        if (pyr_out) { std::memcpy(pyr_out, P.img[l].data(), P.img[l].size()); pyr_out += P.img[l].size(); }
        if (der_out) { std::memcpy(der_out, P.der[l].data(), P.der[l].size() * 2); der_out += P.der[l].size(); }
    }
}

float kfo_pd_update(float *state6, float input, double Ts) {      // state: maxOutput, kp, kd, prevInput, setpoint, Alpha
    PD pd;
    pd.maxOutput = state6[0]; pd.kp = state6[1]; pd.kd = state6[2]; pd.prevInput = state6[3]; pd.setpoint = state6[4]; pd.Alpha = state6[5];
    const float out = pd.update(input, Ts);
    state6[3] = pd.prevInput;
    return out;
}

void *kfo_create(float kp, float kd, float th) {
    Sampler *s = new Sampler();
    s->pd.kp = kp; s->pd.kd = kd; s->pd.setpoint = th;
    return s;
}
void kfo_destroy(void *h) { delete (Sampler *)h; }
void kfo_set_pd(void *h, float kp, float kd, float th) { Sampler *s = (Sampler *)h; s->pd.kp = kp; s->pd.kd = kd; s->pd.setpoint = th; }
void kfo_reset(void *h) { ((Sampler *)h)->old.clear(); }
int kfo_old(void *h, float *out) { Sampler *s = (Sampler *)h; if (out) std::memcpy(out, s->old.data(), s->old.size() * 4); return (int)s->old.size() / 2; }
float kfo_prev_input(void *h) { return ((Sampler *)h)->pd.prevInput; }

// One KFDSample::Step on a grey frame.  The ORB extraction is not part of this file: when out->selected is 1 the caller extracts the frame and hands
// the key-points' (x, y) over with kfo_set_keypoints before the next step.  next / status (may be null) receive n_tracked entries.
void kfo_step(void *h, const uint8_t *grey, int w, int hgt, int stride, double t, KfoStep *out, float *next, uint8_t *status) {
    Sampler *s = (Sampler *)h;
    std::memset(out, 0, sizeof *out);
    Pyramid cur;
    cur.build(grey, w, hgt, stride);
    if (s->old.empty()) {                                       // KFDSample.cc:109-124
        s->ltframe = t;
        s->prev = std::move(cur);
        out->selected = 1;
        return;
    }
    const int n = (int)s->old.size() / 2;
    s->next.assign((size_t)n * 2, 0.f);
    s->status.assign((size_t)n, 0);
    track(s->prev, cur, s->old.data(), n, s->next.data(), s->status.data(), nullptr);
    float sum = 0;
    int good = 0;
    for (int i = 0; i < n; i++)
        if (s->status[i] == 1) {                                // Calmoptflmag over the good points, in index order
            const float dx = s->next[2 * i] - s->old[2 * i], dy = s->next[2 * i + 1] - s->old[2 * i + 1];
            sum += std::sqrt(dx * dx + dy * dy);
            good++;
        }
    const float moptf = sum / good;                             // (0 / 0 = NaN without a good point, as the reference)
    const float pdOut = s->pd.update(moptf, t - s->ltframe);
    const float TH = moptf + pdOut;
    out->n_tracked = n; out->n_good = good; out->moptf = moptf; out->pd_out = pdOut; out->th = TH;
    if (next) std::memcpy(next, s->next.data(), (size_t)n * 8);
    if (status) std::memcpy(status, s->status.data(), (size_t)n);
    if (moptf > TH) out->selected = 1;                          // old: the caller's kfo_set_keypoints
    else s->old = s->next;                                      // every point, the failed ones included
    s->ltframe = t;
    s->prev = std::move(cur);
}
void kfo_set_keypoints(void *h, const float *xy, int n) { Sampler *s = (Sampler *)h; s->old.assign(xy, xy + (size_t)n * 2); }

}  // extern "C"
