// Pyramidal Lucas-Kanade flow for the PD frame selector (include/rumi_kfd.h): what KFDSample::Step (R/lib_src/KFDSample.cc:131) asks of
// cv::calcOpticalFlowPyrLK with a 31 x 31 window, maxLevel 2 and 20 iterations or eps 0.03, restated so that the device and the scalar oracle
// (tests/cpp/kfd_oracle.cc) give the same bits: the window sums are exact integers, every float expression is written out, no contraction.
//   k_flow_grey      BGR -> level 0 (grey input is uploaded straight into level 0)
//   k_flow_pyrdown   levels 1 and 2 in one launch: a block builds its 36 x 36 piece of level 1 in LDS, writes the 32 x 32 it owns and reduces it again
//   k_flow_scharr    interleaved (dx, dy) of the three levels in one launch
//   k_flow_track     one wave64 per point through levels 2, 1, 0
// and rumi_kfd_track, the stateless entry the tests reach the kernels through.  The sampler itself lives with the extractor it uses (orb_kfd.inc).
#include <cfloat>
#include <cstring>

#include "flow_device.h"
#include "rumi_common.h"
#include "rumi_kfd.h"

namespace rumi {

FlowGeom flow_geometry(int w, int h) {
    FlowGeom g{};
    int off = 0, doff = 0;
    for (int l = 0; l < kFlowLevels; l++) {
        g.w[l] = l ? (g.w[l - 1] + 1) / 2 : w;
        g.h[l] = l ? (g.h[l - 1] + 1) / 2 : h;
        g.pitch[l] = (g.w[l] + 3) & ~3;
        g.off[l] = off; g.doff[l] = doff;
        off += (g.pitch[l] * g.h[l] + 255) & ~255;
        doff += g.w[l] * g.h[l];
    }
    g.frameBytes = off; g.derivElems = doff;
    return g;
}

namespace {

__device__ __forceinline__ int reflect101(int i, int n) {
    if (i < 0) i = -i;
    if (i >= n) i = 2 * n - 2 - i;
    return i;
}

// cvFloor; what does not fit an int (or is NaN) lands far outside every image
__device__ __forceinline__ int ifloor(float v) {
    const float f = floorf(v);
    if (!(f >= -1073741824.f)) return -1073741824;
    if (f > 1073741824.f) return 1073741824;
    return (int)f;
}

__global__ void k_flow_grey(const uint8_t *__restrict__ bgr, int bstride, uint8_t *__restrict__ out, int w, int h, int pitch) {
    const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
    if (x >= w || y >= h) return;
    const uint8_t *q = bgr + (size_t)y * bstride + 3 * x;
    out[(size_t)y * pitch + x] = (uint8_t)((1868 * q[0] + 9617 * q[1] + 4899 * q[2] + 8192) >> 14);
}

__device__ __forceinline__ int tap5(int d) { return d == 0 ? 6 : (d == 1 || d == -1) ? 4 : 1; }

// One block: the 16 x 16 tile of level 2 at (16 bx, 16 by), the 32 x 32 tile of level 1 under it, and that tile's two-pixel halo recomputed.
__global__ __launch_bounds__(256) void k_flow_pyrdown(uint8_t *__restrict__ frame, FlowGeom g) {
    __shared__ uint8_t t1[36][36];
    const uint8_t *l0 = frame + g.off[0];
    uint8_t *l1 = frame + g.off[1], *l2 = frame + g.off[2];
    const int w0 = g.w[0], h0 = g.h[0], w1 = g.w[1], h1 = g.h[1], w2 = g.w[2], h2 = g.h[2];
    const int X1 = 32 * blockIdx.x - 2, Y1 = 32 * blockIdx.y - 2;      // level-1 position of t1[0][0]
    for (int e = threadIdx.x; e < 36 * 36; e += 256) {
        const int ty = e / 36, tx = e - 36 * ty;
        // the level-1 pixel this slot stands for: reflected (the halo of a border tile), then clamped (slots nobody reads)
        const int rx = min(max(reflect101(X1 + tx, w1), 0), w1 - 1), ry = min(max(reflect101(Y1 + ty, h1), 0), h1 - 1);
        int sum = 0;
#pragma unroll
        for (int dy = -2; dy <= 2; dy++) {
            const uint8_t *row = l0 + (size_t)reflect101(2 * ry + dy, h0) * g.pitch[0];
            int rs = 0;
#pragma unroll
            for (int dx = -2; dx <= 2; dx++) rs += tap5(dx) * row[reflect101(2 * rx + dx, w0)];
            sum += tap5(dy) * rs;
        }
        const uint8_t v = (uint8_t)((sum + 128) >> 8);
        t1[ty][tx] = v;
        const int x1 = X1 + tx, y1 = Y1 + ty;
        if (tx >= 2 && tx < 34 && ty >= 2 && ty < 34 && x1 < w1 && y1 < h1) l1[(size_t)y1 * g.pitch[1] + x1] = v;
    }
    __syncthreads();
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    const int x2 = 16 * blockIdx.x + tx, y2 = 16 * blockIdx.y + ty;
    if (x2 >= w2 || y2 >= h2) return;
    int sum = 0;
#pragma unroll
    for (int dy = -2; dy <= 2; dy++) {
        int rs = 0;
#pragma unroll
        for (int dx = -2; dx <= 2; dx++) rs += tap5(dx) * t1[2 * ty + dy + 2][2 * tx + dx + 2];
        sum += tap5(dy) * rs;
    }
    l2[(size_t)y2 * g.pitch[2] + x2] = (uint8_t)((sum + 128) >> 8);
}

// blockIdx.z = level; the grid is sized for level 0
__global__ __launch_bounds__(256) void k_flow_scharr(const uint8_t *__restrict__ frame, uint32_t *__restrict__ deriv, FlowGeom g) {
    const int l = blockIdx.z, w = g.w[l], h = g.h[l], pitch = g.pitch[l];
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= w || y >= h) return;
    const uint8_t *img = frame + g.off[l];
    const uint8_t *r0 = img + (size_t)reflect101(y - 1, h) * pitch, *r1 = img + (size_t)y * pitch, *r2 = img + (size_t)reflect101(y + 1, h) * pitch;
    const int xl = reflect101(x - 1, w), xr = reflect101(x + 1, w);
    const int dx = 3 * (r0[xr] - r0[xl]) + 10 * (r1[xr] - r1[xl]) + 3 * (r2[xr] - r2[xl]);
    const int dy = 3 * (r2[xl] - r0[xl]) + 10 * (r2[x] - r0[x]) + 3 * (r2[xr] - r0[xr]);
    deriv[g.doff[l] + y * w + x] = ((uint32_t)dx & 0xffffu) | ((uint32_t)dy << 16);
}

struct Weights { int w00, w01, w10, w11; };
__device__ __forceinline__ Weights weights(float a, float b) {
    Weights k;
    k.w00 = (int)rintf((1.f - a) * (1.f - b) * 16384.f);
    k.w01 = (int)rintf(a * (1.f - b) * 16384.f);
    k.w10 = (int)rintf((1.f - a) * b * 16384.f);
    k.w11 = 16384 - k.w00 - k.w01 - k.w10;
    return k;
}

// the sum of a lane's int32 over the wave as an exact 64-bit integer, in every lane
__device__ __forceinline__ long long wave_sum(int v) {
    long long s = v;
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const int lo = __shfl_xor((int)(unsigned)(unsigned long long)s, m), hi = __shfl_xor((int)(s >> 32), m);
        s += (long long)(((unsigned long long)(unsigned)hi << 32) | (unsigned)lo);
    }
    return s;
}
__device__ __forceinline__ float sum_to_float(long long v) { return (float)(double)v * (1.f / (1 << 20)); }

// One wave64 per point.  Lane L owns the window pixels k = L + 64 i (i < 16, k < 961; the others carry zeros): their I, Ix, Iy stay in registers
// over the iterations of a level.  An iteration stages the 32 x 32 footprint of J (reflected) in LDS, every lane forms its 16 differences, and two
// integer butterflies give b1, b2 to every lane; a lane's partial sums fit an int32 (|diff| <= 8162, |Ix| <= 4082, 16 products), the wave's do not.
// Every lane then does the same 2 x 2 solve on the same bits, so the breaks are uniform without a broadcast.
__global__ __launch_bounds__(64) void k_flow_track(const uint8_t *__restrict__ prevFrame, const uint32_t *__restrict__ prevDeriv, const uint8_t *__restrict__ curFrame,
                                                   FlowGeom g, const float *__restrict__ pts, int n, float *__restrict__ outNext, uint8_t *__restrict__ outStatus) {
    __shared__ uint32_t sJ[256];                              // 32 rows of 32 bytes
    const int p = blockIdx.x, lane = threadIdx.x;
    if (p >= n) return;
    const float ptx = pts[2 * p], pty = pts[2 * p + 1];
    int fo[16];                                               // the pixel's byte in the footprint
#pragma unroll
    for (int i = 0; i < 16; i++) {
        const int k = lane + 64 * i, y = k / kFlowWin, x = k - kFlowWin * y;
        fo[i] = k < kFlowWin * kFlowWin ? y * 32 + x : -1;
    }
    float outx = 0.f, outy = 0.f;
    int st = 1;
    for (int level = kFlowLevels - 1; level >= 0; level--) {
        const int W = g.w[level], H = g.h[level], pitch = g.pitch[level];
        const uint8_t *I0 = prevFrame + g.off[level], *J0 = curFrame + g.off[level];
        const uint32_t *Dv = prevDeriv + g.doff[level];
        const float s = 1.f / (float)(1 << level);
        float px = ptx * s, py = pty * s, nx, ny;
        if (level == kFlowLevels - 1) { nx = px; ny = py; }
        else { nx = outx * 2.f; ny = outy * 2.f; }
        outx = nx; outy = ny;
        px -= 15.f; py -= 15.f;
        const int ipx = ifloor(px), ipy = ifloor(py);
        if (ipx < -kFlowWin || ipx >= W || ipy < -kFlowWin || ipy >= H) {
            if (level == 0) st = 0;
            continue;
        }
        const Weights k = weights(px - (float)ipx, py - (float)ipy);
        int Iv[16], Ixv[16], Iyv[16];
        int s11 = 0, s12 = 0, s22 = 0;
#pragma unroll
        for (int i = 0; i < 16; i++) {
            Iv[i] = 0; Ixv[i] = 0; Iyv[i] = 0;
            if (fo[i] >= 0) {
                const int X = ipx + (fo[i] & 31), Y = ipy + (fo[i] >> 5);
                const int x0 = reflect101(X, W), x1 = reflect101(X + 1, W);
                const uint8_t *r0 = I0 + (size_t)reflect101(Y, H) * pitch, *r1 = I0 + (size_t)reflect101(Y + 1, H) * pitch;
                Iv[i] = (r0[x0] * k.w00 + r0[x1] * k.w01 + r1[x0] * k.w10 + r1[x1] * k.w11 + 256) >> 9;
                const bool xin0 = X >= 0 && X < W, xin1 = X + 1 >= 0 && X + 1 < W, yin0 = Y >= 0 && Y < H, yin1 = Y + 1 >= 0 && Y + 1 < H;
                const uint32_t d00 = xin0 && yin0 ? Dv[Y * W + X] : 0u, d01 = xin1 && yin0 ? Dv[Y * W + X + 1] : 0u;
                const uint32_t d10 = xin0 && yin1 ? Dv[(Y + 1) * W + X] : 0u, d11 = xin1 && yin1 ? Dv[(Y + 1) * W + X + 1] : 0u;
                Ixv[i] = ((int)(int16_t)(d00 & 0xffffu) * k.w00 + (int)(int16_t)(d01 & 0xffffu) * k.w01 + (int)(int16_t)(d10 & 0xffffu) * k.w10 +
                          (int)(int16_t)(d11 & 0xffffu) * k.w11 + 8192) >> 14;
                Iyv[i] = (((int)d00 >> 16) * k.w00 + ((int)d01 >> 16) * k.w01 + ((int)d10 >> 16) * k.w10 + ((int)d11 >> 16) * k.w11 + 8192) >> 14;
            }
            s11 += Ixv[i] * Ixv[i]; s12 += Ixv[i] * Iyv[i]; s22 += Iyv[i] * Iyv[i];
        }
        const float A11 = sum_to_float(wave_sum(s11)), A12 = sum_to_float(wave_sum(s12)), A22 = sum_to_float(wave_sum(s22));
        float D = A11 * A22 - A12 * A12;
        const float minEig = (A22 + A11 - sqrtf((A11 - A22) * (A11 - A22) + 4.f * A12 * A12)) / (float)(2 * kFlowWin * kFlowWin);
        if (minEig < 1e-4f || D < FLT_EPSILON) {
            if (level == 0) st = 0;
            continue;
        }
        D = 1.f / D;
        nx -= 15.f; ny -= 15.f;
        float pdx = 0.f, pdy = 0.f;
        for (int j = 0; j < 20; j++) {
            const int inx = ifloor(nx), iny = ifloor(ny);
            if (inx < -kFlowWin || inx >= W || iny < -kFlowWin || iny >= H) {
                if (level == 0) st = 0;
                break;
            }
            const Weights kn = weights(nx - (float)inx, ny - (float)iny);
            __syncthreads();                                  // (one wave: the last iteration's reads are done)
#pragma unroll
            for (int i = 0; i < 4; i++) {
                const int e = lane + 64 * i, fy = e >> 3, fx = (e & 7) * 4;
                const uint8_t *row = J0 + (size_t)reflect101(iny + fy, H) * pitch;
                sJ[e] = (uint32_t)row[reflect101(inx + fx, W)] | ((uint32_t)row[reflect101(inx + fx + 1, W)] << 8) |
                        ((uint32_t)row[reflect101(inx + fx + 2, W)] << 16) | ((uint32_t)row[reflect101(inx + fx + 3, W)] << 24);
            }
            __syncthreads();
            const uint8_t *jb = reinterpret_cast<const uint8_t *>(sJ);
            int sb1 = 0, sb2 = 0;
#pragma unroll
            for (int i = 0; i < 16; i++) {
                const int o = fo[i] >= 0 ? fo[i] : 0;          // (a lane's empty slots read pixel 0 and multiply it by Ix = Iy = 0)
                const int diff = ((jb[o] * kn.w00 + jb[o + 1] * kn.w01 + jb[o + 32] * kn.w10 + jb[o + 33] * kn.w11 + 256) >> 9) - Iv[i];
                sb1 += diff * Ixv[i]; sb2 += diff * Iyv[i];
            }
            const float b1 = sum_to_float(wave_sum(sb1)), b2 = sum_to_float(wave_sum(sb2));
            const float dx = (A12 * b2 - A22 * b1) * D, dy = (A12 * b1 - A11 * b2) * D;
            nx += dx; ny += dy;
            outx = nx + 15.f; outy = ny + 15.f;
            if ((double)dx * (double)dx + (double)dy * (double)dy <= 0.03 * 0.03) break;
            if (j > 0 && (double)fabsf(dx + pdx) < 0.01 && (double)fabsf(dy + pdy) < 0.01) {
                outx -= dx * 0.5f; outy -= dy * 0.5f;
                break;
            }
            pdx = dx; pdy = dy;
        }
    }
    if (lane == 0) { outNext[2 * p] = outx; outNext[2 * p + 1] = outy; outStatus[p] = (uint8_t)st; }
}

}  // namespace

void flow_launch_grey(const uint8_t *dBgr, int bstride, uint8_t *frame, const FlowGeom &g, hipStream_t st) {
    k_flow_grey<<<dim3((g.w[0] + 255) / 256, g.h[0]), 256, 0, st>>>(dBgr, bstride, frame + g.off[0], g.w[0], g.h[0], g.pitch[0]);
}

void flow_launch_prepare(uint8_t *frame, uint32_t *deriv, const FlowGeom &g, hipStream_t st) {
    k_flow_pyrdown<<<dim3((g.w[2] + 15) / 16, (g.h[2] + 15) / 16), 256, 0, st>>>(frame, g);
    k_flow_scharr<<<dim3((g.w[0] + 63) / 64, (g.h[0] + 3) / 4, kFlowLevels), 256, 0, st>>>(frame, deriv, g);
}

void flow_launch_track(const uint8_t *prevFrame, const uint32_t *prevDeriv, const uint8_t *curFrame, const FlowGeom &g, const float *pts, int n, float *outNext,
                       uint8_t *outStatus, hipStream_t st) {
    if (n > 0) k_flow_track<<<n, 64, 0, st>>>(prevFrame, prevDeriv, curFrame, g, pts, n, outNext, outStatus);
}

}  // namespace rumi

using namespace rumi;

// Stateless: both frames go up, both pyramids are built, the points are tracked, everything comes back.  Device memory is taken and released inside.
extern "C" int rumi_kfd_track(int32_t device, const uint8_t *prev, const uint8_t *cur, int32_t w, int32_t hgt, int32_t stride, int32_t channels, const float *pts,
                              int32_t n, float *next, uint8_t *status, uint8_t *pyr_out, int16_t *deriv_out) {
    if (!prev || !cur || w <= 0 || hgt <= 0) return RUMI_E_EMPTY;
    if (channels != 1 && channels != 3) { g_lastError = "rumi_kfd_track: 1 (grey) or 3 (BGR) channels"; return RUMI_E_INVALID; }
    if (w < kFlowMinSide || hgt < kFlowMinSide || w > 16384 || hgt > 16384 || stride < w * channels) { g_lastError = "rumi_kfd_track: frames of at least 128 x 128, rows of at least w * channels bytes"; return RUMI_E_INVALID; }
    if (n < 0 || (n > 0 && (!pts || !next || !status))) { g_lastError = "rumi_kfd_track: bad point list"; return RUMI_E_INVALID; }
    if (device >= 0) HIP_TRY(hipSetDevice(device));
    const FlowGeom g = flow_geometry(w, hgt);
    uint8_t *dFrames = nullptr, *dBgr = nullptr, *dOut = nullptr;
    uint32_t *dDeriv = nullptr;
    float *dPts = nullptr;
    auto release = [&]() { for (void *q : {(void *)dFrames, (void *)dBgr, (void *)dOut, (void *)dDeriv, (void *)dPts}) if (q) (void)hipFree(q); };
    const size_t nn = (size_t)std::max(n, 1);
#define TRY_T(x) do { const hipError_t e_ = (x); if (e_ != hipSuccess) { release(); rumi::set_error("HIP error: %s -> %s (line %d)", #x, hipGetErrorString(e_), __LINE__); return RUMI_E_NO_DEVICE; } } while (0)
    TRY_T(hipMalloc((void **)&dFrames, 2 * (size_t)g.frameBytes));
    TRY_T(hipMalloc((void **)&dDeriv, (size_t)g.derivElems * sizeof(uint32_t)));
    TRY_T(hipMalloc((void **)&dPts, nn * 2 * sizeof(float)));
    TRY_T(hipMalloc((void **)&dOut, nn * 9));
    const uint8_t *src[2] = {prev, cur};
    if (channels == 3) TRY_T(hipMalloc((void **)&dBgr, (size_t)w * 3 * hgt));
    for (int f = 0; f < 2; f++) {
        uint8_t *frame = dFrames + (size_t)f * g.frameBytes;
        if (channels == 3) {
            TRY_T(hipMemcpy2D(dBgr, (size_t)w * 3, src[f], (size_t)stride, (size_t)w * 3, (size_t)hgt, hipMemcpyHostToDevice));
            flow_launch_grey(dBgr, w * 3, frame, g, nullptr);
            TRY_T(hipDeviceSynchronize());                    // (dBgr is reused by the second frame)
        } else TRY_T(hipMemcpy2D(frame + g.off[0], (size_t)g.pitch[0], src[f], (size_t)stride, (size_t)w, (size_t)hgt, hipMemcpyHostToDevice));
    }
    flow_launch_prepare(dFrames, dDeriv, g, nullptr);                               // the previous frame: pyramid and derivative
    k_flow_pyrdown<<<dim3((g.w[2] + 15) / 16, (g.h[2] + 15) / 16), 256, 0, nullptr>>>(dFrames + g.frameBytes, g);   // the current one: pyramid only
    if (n > 0) {
        TRY_T(hipMemcpy(dPts, pts, (size_t)n * 2 * sizeof(float), hipMemcpyHostToDevice));
        flow_launch_track(dFrames, dDeriv, dFrames + g.frameBytes, g, dPts, n, reinterpret_cast<float *>(dOut), dOut + (size_t)n * 8, nullptr);
    }
    TRY_T(hipGetLastError());
    TRY_T(hipDeviceSynchronize());
    if (n > 0) {
        TRY_T(hipMemcpy(next, dOut, (size_t)n * 8, hipMemcpyDeviceToHost));
        TRY_T(hipMemcpy(status, dOut + (size_t)n * 8, (size_t)n, hipMemcpyDeviceToHost));
    }
    for (int l = 0; l < kFlowLevels; l++) {
        if (pyr_out) {
            TRY_T(hipMemcpy2D(pyr_out, (size_t)g.w[l], dFrames + g.off[l], (size_t)g.pitch[l], (size_t)g.w[l], (size_t)g.h[l], hipMemcpyDeviceToHost));
            pyr_out += (size_t)g.w[l] * g.h[l];
        }
        if (deriv_out) {
            TRY_T(hipMemcpy(deriv_out, dDeriv + g.doff[l], (size_t)g.w[l] * g.h[l] * sizeof(uint32_t), hipMemcpyDeviceToHost));
            deriv_out += (size_t)g.w[l] * g.h[l] * 2;
        }
    }
#undef TRY_T
    release();
    return RUMI_OK;
}
