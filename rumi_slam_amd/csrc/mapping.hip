// LocalMapping::CreateNewMapPoints (R/lib_src/LocalMapping.cc:354-647, monocular pinhole) behind include/rumi_mapping.h: the search of every
// neighbour, the triangulation and gates of every candidate pair and the scene median depths in wide launches, then the order-dependent part
// (a feature that received a point is gone for the later neighbours) by one workgroup.  One pinned block up, one result block back.
//
// Why the loop decomposes:
//   cand[k][i1]  SearchForTriangulation's pick for feature i1 in neighbour k depends on i1, k and on whether i1 held a point BEFORE the call
//                (vbMatched2 is never set, ORBmatcher.cc:893; a neighbour's own flags are read before its points are added).
//   gate[k][i1]  whether (i1, cand[k][i1]) triangulates and passes every test depends on the two key-frames alone.
//   replay       for k = 0, 1, ...: baseline skip; the pairs whose i1 is still free; the rotation histogram over exactly those; survivors
//                with gate == 0 create a point and take i1 out.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "rumi_mapping.h"
#include "rumi_testhooks.h"
#include "match_host.h"

namespace rumi {

// One key-frame inside the upload block: sizes, byte offsets of its arrays, the small matrices.  Entry 0 is the current key-frame.
struct KFDev {
    int32_t n, nn, ne, nlevels;
    uint32_t keys, desc, scale, nodes, off, idx, mp, pos;
    float K[4], T[12], Ow[3], F12[9], ep[2];
    int32_t pad[2];
};
static_assert(sizeof(KFDev) % 16 == 0, "arrays behind the table start 16-byte aligned");

constexpr int kMaxCur = RUMI_NEWPTS_MAX_FEATURES;     // features of the current key-frame: the replay keeps one free flag each in LDS
static_assert(kMaxCur <= 32768, "k_newpts_replay's free flags (one byte a feature) and its other LDS must stay within 64 KiB");

enum { GATE_OK = 0, GATE_PARALLAX, GATE_W0, GATE_Z1, GATE_Z2, GATE_REPROJ1, GATE_REPROJ2, GATE_DIST0, GATE_FAR, GATE_SCALE };

template <class T> __device__ __forceinline__ const T *at(const uint8_t *blk, uint32_t off) { return reinterpret_cast<const T *>(blk + off); }

// ---- 1. search --------------------------------------------------------------------------------------------------------------------------
// One wavefront per (neighbour, node of the current key-frame's FeatureVector).  Lanes hold the candidates of the neighbour's node (descriptor,
// key-point, epipole test: loaded once per 64 candidates); the node's current features go by one at a time, wave-uniform, and each is reduced
// over the lanes on the key ~((dist << 16) | (0xffff - position)): the maximum is the smallest distance, the LATER position on ties
// (`dist > bestDist` rejects, ORBmatcher.cc:905).  Lane j keeps the running key of the tile's feature j, so nodes of more than 64
// candidates need no memory between chunks.  A wave rather than half of one: a node at levelsup = 4 holds ~20 features a side, and the
// cost is the 20 uniform steps, not the idle lanes; two nodes a wave would double the steps' register state for no shorter chain.
__global__ __launch_bounds__(256) void k_newpts_match(const uint8_t *__restrict__ blk, int coarse, int32_t *__restrict__ cand) {
    const KFDev *kf = reinterpret_cast<const KFDev *>(blk);
    const int lane = threadIdx.x & 63;
    const int a = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6)), k = blockIdx.y;
    const KFDev &C = kf[0], &N = kf[1 + k];
    if (a >= C.nn) return;
    const uint32_t *nodes2 = at<uint32_t>(blk, N.nodes);
    const uint32_t id = at<uint32_t>(blk, C.nodes)[a];
    int lo = 0, hi = N.nn;
    while (lo < hi) { const int mid = (lo + hi) >> 1; if (nodes2[mid] < id) lo = mid + 1; else hi = mid; }
    if (lo >= N.nn || nodes2[lo] != id) return;
    const int32_t *off1 = at<int32_t>(blk, C.off), *off2 = at<int32_t>(blk, N.off), *mp1 = at<int32_t>(blk, C.mp), *mp2 = at<int32_t>(blk, N.mp);
    const uint32_t *idx1 = at<uint32_t>(blk, C.idx), *idx2 = at<uint32_t>(blk, N.idx);
    const RumiKeyPoint *keys1 = at<RumiKeyPoint>(blk, C.keys), *keys2 = at<RumiKeyPoint>(blk, N.keys);
    const uint8_t *desc1 = blk + C.desc, *desc2 = blk + N.desc;
    const float *scale2 = at<float>(blk, N.scale);
    const float *F = N.F12;
    const float epx = N.ep[0], epy = N.ep[1];
    const int p0 = off1[a], p1 = off1[a + 1], c0 = off2[lo], c1 = off2[lo + 1];
    for (int pt = p0; pt < p1; pt += 64) {
        uint32_t mine = 0;                                   // running key of feature pt + lane
        const int pe = min(pt + 64, p1);
        for (int cb = c0; cb < c1; cb += 64) {
            const int c = cb + lane;
            bool valid = c < c1;
            const int i2 = valid ? (int)idx2[c] : 0;
            valid = valid && mp2[i2] < 0;                    // pKF2->GetMapPoint(idx2), :893
            uint32_t d2[8];
#pragma unroll
            for (int w = 0; w < 8; w++) d2[w] = reinterpret_cast<const uint32_t *>(desc2 + (size_t)i2 * 32)[w];
            const RumiKeyPoint k2 = keys2[i2];
            const float sc = scale2[k2.octave];
            const float ex = epx - k2.x, ey = epy - k2.y;
            if (ex * ex + ey * ey < 100 * sc) valid = false; // :912-918
            const float s2 = sc * sc;                        // mvLevelSigma2
            for (int p = pt; p < pe; p++) {
                const int i1 = (int)idx1[p];
                if (mp1[i1] >= 0) continue;                  // pKF1->GetMapPoint(idx1), :865 (wave-uniform)
                uint32_t d1[8];
#pragma unroll
                for (int w = 0; w < 8; w++) d1[w] = reinterpret_cast<const uint32_t *>(desc1 + (size_t)i1 * 32)[w];
                const int dist = hamming256(d1, d2);
                bool ok = valid && dist <= RUMI_TH_LOW;
                if (!coarse) {                               // Pinhole::epipolarConstrain (Pinhole.cpp:107-129), the arithmetic of k_tri_match
                    const float x1 = keys1[i1].x, y1 = keys1[i1].y;
                    const float la = x1 * F[0] + y1 * F[3] + F[6];
                    const float lb = x1 * F[1] + y1 * F[4] + F[7];
                    const float lc = x1 * F[2] + y1 * F[5] + F[8];
                    const float den = la * la + lb * lb;
                    const float num = la * k2.x + lb * k2.y + lc;
                    const float dsqr = num * num / den;
                    ok = ok && den != 0 && (double)dsqr < 3.84 * (double)s2;
                }
                const uint32_t key = ok ? ~(((uint32_t)dist << 16) | (uint32_t)(0xffff - c)) : 0u;
                const uint32_t best = wave_max_u32(key);
                if (lane == p - pt) mine = max(mine, best);
            }
        }
        const int p = pt + lane;
        if (p < pe && mine != 0) cand[(size_t)k * C.n + idx1[p]] = (int32_t)idx2[0xffff - (~mine & 0xffff)];
    }
}

// ---- 2. triangulation and gates ---------------------------------------------------------------------------------------------------------
// Right null vector of Triangulate's A (GeometricTools.cc:55-57) as include/rumi_mapping.h defines it: eigenvector of the smallest eigenvalue
// of A^T A, cyclic Jacobi in double, 6 sweeps over (0,1) (0,2) (0,3) (1,2) (1,3) (2,3).  Everything is indexed by constants after unrolling,
// so M and V stay in registers.
#define RUMI_JACOBI_ROT(P, Q)                                                                                   \
    if (M[P][Q] != 0.0) {                                                                                       \
        const double theta = (M[Q][Q] - M[P][P]) / (2.0 * M[P][Q]);                                             \
        const double t = (theta >= 0.0 ? 1.0 : -1.0) / (__builtin_fabs(theta) + __builtin_sqrt(theta * theta + 1.0)); \
        const double c = 1.0 / __builtin_sqrt(t * t + 1.0), s = t * c;                                          \
        _Pragma("unroll") for (int r = 0; r < 4; r++) {                                                         \
            const double mp = M[r][P], mq = M[r][Q];                                                            \
            M[r][P] = c * mp - s * mq; M[r][Q] = s * mp + c * mq;                                               \
        }                                                                                                       \
        _Pragma("unroll") for (int r = 0; r < 4; r++) {                                                         \
            const double mp = M[P][r], mq = M[Q][r];                                                            \
            M[P][r] = c * mp - s * mq; M[Q][r] = s * mp + c * mq;                                               \
        }                                                                                                       \
        _Pragma("unroll") for (int r = 0; r < 4; r++) {                                                         \
            const double vp = V[r][P], vq = V[r][Q];                                                            \
            V[r][P] = c * vp - s * vq; V[r][Q] = s * vp + c * vq;                                               \
        }                                                                                                       \
    }

__device__ __forceinline__ void null_vector4(const float (&A)[4][4], double (&v)[4]) {
    double M[4][4], V[4][4];
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
        for (int j = 0; j < 4; j++) {
            double s = 0.0;
#pragma unroll
            for (int r = 0; r < 4; r++) s += (double)A[r][i] * (double)A[r][j];
            M[i][j] = s;
            V[i][j] = i == j ? 1.0 : 0.0;
        }
#pragma unroll 1
    for (int sweep = 0; sweep < 6; sweep++) {
        RUMI_JACOBI_ROT(0, 1) RUMI_JACOBI_ROT(0, 2) RUMI_JACOBI_ROT(0, 3) RUMI_JACOBI_ROT(1, 2) RUMI_JACOBI_ROT(1, 3) RUMI_JACOBI_ROT(2, 3)
    }
    double best = M[0][0];
#pragma unroll
    for (int r = 0; r < 4; r++) v[r] = V[r][0];
#pragma unroll
    for (int j = 1; j < 4; j++) {
        const bool less = M[j][j] < best;
        best = less ? M[j][j] : best;
#pragma unroll
        for (int r = 0; r < 4; r++) v[r] = less ? V[r][j] : v[r];
    }
}
#undef RUMI_JACOBI_ROT

__device__ __forceinline__ float dot3(float a0, float a1, float a2, float b0, float b1, float b2) { return (a0 * b0 + a1 * b1) + a2 * b2; }
__device__ __forceinline__ float norm3(float x, float y, float z) { return __builtin_sqrtf((x * x + y * y) + z * z); }

// One lane per (neighbour, feature of the current key-frame) that has a candidate: LocalMapping.cc:506-626 in float, in the reference's order.
__global__ __launch_bounds__(256) void k_newpts_triangulate(const uint8_t *__restrict__ blk, const int32_t *__restrict__ cand, int farPoints,
                                                            float thFar, float ratioFactor, uint8_t *__restrict__ gate, float *__restrict__ x3Dout) {
    const KFDev *kf = reinterpret_cast<const KFDev *>(blk);
    const KFDev &C = kf[0], &N = kf[1 + blockIdx.y];
    const int i1 = blockIdx.x * blockDim.x + threadIdx.x;
    if (i1 >= C.n) return;
    const size_t slot = (size_t)blockIdx.y * C.n + i1;
    const int i2 = cand[slot];
    if (i2 < 0) return;
    const RumiKeyPoint kp1 = at<RumiKeyPoint>(blk, C.keys)[i1], kp2 = at<RumiKeyPoint>(blk, N.keys)[i2];
    const float *T1 = C.T, *T2 = N.T;
    // :507-512  unprojectEig (Pinhole.cpp:61-64), rays, parallax
    const float xn1[3] = {(kp1.x - C.K[2]) / C.K[0], (kp1.y - C.K[3]) / C.K[1], 1.f};
    const float xn2[3] = {(kp2.x - N.K[2]) / N.K[0], (kp2.y - N.K[3]) / N.K[1], 1.f};
    float ray1[3], ray2[3];
#pragma unroll
    for (int i = 0; i < 3; i++) {                            // Rwc = Rcw^T
        ray1[i] = dot3(T1[i], T1[4 + i], T1[8 + i], xn1[0], xn1[1], xn1[2]);
        ray2[i] = dot3(T2[i], T2[4 + i], T2[8 + i], xn2[0], xn2[1], xn2[2]);
    }
    const float cosPar = dot3(ray1[0], ray1[1], ray1[2], ray2[0], ray2[1], ray2[2]) /
                         (norm3(ray1[0], ray1[1], ray1[2]) * norm3(ray2[0], ray2[1], ray2[2]));
    const float cosStereo = cosPar + 1;
    int g = GATE_OK;
    float x3D[3] = {0.f, 0.f, 0.f};
    if (!(cosPar < cosStereo && cosPar > 0 && (double)cosPar < 0.9998)) g = GATE_PARALLAX;      // :531, mono, not inertial
    if (g == GATE_OK) {
        float A[4][4];                                       // GeometricTools.cc:49-53
#pragma unroll
        for (int j = 0; j < 4; j++) {
            A[0][j] = xn1[0] * T1[8 + j] - T1[j];
            A[1][j] = xn1[1] * T1[8 + j] - T1[4 + j];
            A[2][j] = xn2[0] * T2[8 + j] - T2[j];
            A[3][j] = xn2[1] * T2[8 + j] - T2[4 + j];
        }
        double v[4];
        null_vector4(A, v);
        if ((float)v[3] == 0.f) g = GATE_W0;                 // :59
        else {
#pragma unroll
            for (int i = 0; i < 3; i++) x3D[i] = (float)(v[i] / v[3]);
        }
    }
    if (g == GATE_OK) {
        const float z1 = dot3(T1[8], T1[9], T1[10], x3D[0], x3D[1], x3D[2]) + T1[11];            // :554-560
        const float z2 = dot3(T2[8], T2[9], T2[10], x3D[0], x3D[1], x3D[2]) + T2[11];
        if (z1 <= 0) g = GATE_Z1;
        else if (z2 <= 0) g = GATE_Z2;
        else {
            const float sf1 = at<float>(blk, C.scale)[kp1.octave], sf2 = at<float>(blk, N.scale)[kp2.octave];
            const float sig1 = sf1 * sf1, sig2 = sf2 * sf2;
            const float x1 = dot3(T1[0], T1[1], T1[2], x3D[0], x3D[1], x3D[2]) + T1[3];          // :563-574
            const float y1 = dot3(T1[4], T1[5], T1[6], x3D[0], x3D[1], x3D[2]) + T1[7];
            const float eX1 = (C.K[0] * x1 / z1 + C.K[2]) - kp1.x, eY1 = (C.K[1] * y1 / z1 + C.K[3]) - kp1.y;
            const float x2 = dot3(T2[0], T2[1], T2[2], x3D[0], x3D[1], x3D[2]) + T2[3];          // :588-597
            const float y2 = dot3(T2[4], T2[5], T2[6], x3D[0], x3D[1], x3D[2]) + T2[7];
            const float eX2 = (N.K[0] * x2 / z2 + N.K[2]) - kp2.x, eY2 = (N.K[1] * y2 / z2 + N.K[3]) - kp2.y;
            const float dist1 = norm3(x3D[0] - C.Ow[0], x3D[1] - C.Ow[1], x3D[2] - C.Ow[2]);      // :610-626
            const float dist2 = norm3(x3D[0] - N.Ow[0], x3D[1] - N.Ow[1], x3D[2] - N.Ow[2]);
            const float ratioDist = dist2 / dist1, ratioOctave = sf1 / sf2;
            if ((double)(eX1 * eX1 + eY1 * eY1) > 5.991 * (double)sig1) g = GATE_REPROJ1;
            else if ((double)(eX2 * eX2 + eY2 * eY2) > 5.991 * (double)sig2) g = GATE_REPROJ2;
            else if (dist1 == 0 || dist2 == 0) g = GATE_DIST0;
            else if (farPoints && (dist1 >= thFar || dist2 >= thFar)) g = GATE_FAR;
            else if (ratioDist * ratioFactor < ratioOctave || ratioDist > ratioOctave * ratioFactor) g = GATE_SCALE;
        }
    }
    gate[slot] = (uint8_t)g;
    x3Dout[3 * slot] = x3D[0]; x3Dout[3 * slot + 1] = x3D[1]; x3Dout[3 * slot + 2] = x3D[2];
}

// ---- 3. scene median depth and the baseline test ----------------------------------------------------------------------------------------
// KeyFrame::ComputeSceneMedianDepth(2) (KeyFrame.cc:947-978), then LocalMapping.cc:406-418.  The element of rank (m - 1) / 2 by counting, ties
// broken by index: std::sort's permutation of equal keys is not observable, only the value is read.  Features without a map point carry NaN,
// which no comparison counts.  (+0.0 and -0.0 compare equal, so the element picked among them may carry the other sign than std::sort's, and
// baseline / median the other infinity: a median depth of exactly zero, not reachable with a scene in front of the camera.)  The counting is n^2 compares, vector-issue bound, so a neighbour is spread over n / 256 workgroups: each
// recomputes the depths tile by tile into LDS (cheaper than a pass through memory and a second launch), each thread ranks one feature, and
// the one thread that holds the median applies the baseline test.
constexpr int kDepthTile = 2048;
__global__ __launch_bounds__(256) void k_newpts_depth(const uint8_t *__restrict__ blk, int32_t *__restrict__ skipped) {
    __shared__ __attribute__((aligned(16))) float sZ[kDepthTile];
    __shared__ int sCount;
    const KFDev *kf = reinterpret_cast<const KFDev *>(blk);
    const KFDev &C = kf[0], &N = kf[1 + blockIdx.y];
    const int tid = threadIdx.x, n = N.n, i = blockIdx.x * 256 + tid;
    if (blockIdx.x > 0 && (int)blockIdx.x * 256 >= n) return;
    const int32_t *mp = at<int32_t>(blk, N.mp);
    const float *pos = at<float>(blk, N.pos);
    auto depth = [&](int j) {                                 // :964-971, NaN where the feature holds no point
        return j < n && mp[j] >= 0 ? dot3(N.T[8], N.T[9], N.T[10], pos[3 * j], pos[3 * j + 1], pos[3 * j + 2]) + N.T[11] : __builtin_nanf("");
    };
    if (tid == 0) sCount = 0;
    const float zi = depth(i);
    int rank = 0, mine = 0;
    for (int t0 = 0; t0 < n; t0 += kDepthTile) {
        __syncthreads();
        const int len4 = (min(kDepthTile, n - t0) + 3) & ~3;                // the padding is NaN: it counts for nobody
        for (int j = tid; j < len4; j += 256) { const float zj = depth(t0 + j); sZ[j] = zj; mine += zj == zj ? 1 : 0; }
        __syncthreads();
#pragma unroll 2
        for (int j = 0; j < len4; j += 4) {                  // one 16-byte broadcast read, four compares
            const float4 q = *reinterpret_cast<const float4 *>(&sZ[j]);
            rank += (q.x < zi || (q.x == zi && t0 + j < i)) ? 1 : 0;
            rank += (q.y < zi || (q.y == zi && t0 + j + 1 < i)) ? 1 : 0;
            rank += (q.z < zi || (q.z == zi && t0 + j + 2 < i)) ? 1 : 0;
            rank += (q.w < zi || (q.w == zi && t0 + j + 3 < i)) ? 1 : 0;
        }
    }
    if (mine) atomicAdd(&sCount, mine);
    __syncthreads();
    const int m = sCount;
    // no map point at all: the median is taken as -1.0, the value for N == 0 (KeyFrame.cc:948-949; rumi_mapping.h), which skips the neighbour
    const bool holder = m > 0 ? (zi == zi && rank == (m - 1) / 2) : (i == 0);
    if (holder) {
        const float median = m > 0 ? zi : -1.0f;
        const float baseline = norm3(N.Ow[0] - C.Ow[0], N.Ow[1] - C.Ow[1], N.Ow[2] - C.Ow[2]);
        const float ratio = baseline / median;
        skipped[blockIdx.y] = (double)ratio < 0.01 ? 1 : 0;
    }
}

// ---- 4. replay --------------------------------------------------------------------------------------------------------------------------
// Result block, device and pinned host alike.
struct NewPtsResult {
    int32_t nOut, pad[3];
    int32_t perNeigh[RUMI_NEWPTS_MAX_NEIGH];
    int32_t skipped[RUMI_NEWPTS_MAX_NEIGH];
    RumiNewPoint pts[1];                                     // [n1]
};

// One workgroup walks the neighbours in order.  Feature i belongs to thread i % 1024 in every pass, so a free flag is only ever touched by
// its own thread; the histogram uses integer LDS atomics (order-free), the emission is an ordered compaction (ballot, wave totals, running base).
// matched (may be null: only rumi_hook_newpts_matches passes it) receives stages 1 + 3 per neighbour.
__global__ __launch_bounds__(1024) void k_newpts_replay(const uint8_t *__restrict__ blk, int nNeigh, int checkOri, const int32_t *__restrict__ cand,
                                                        const uint8_t *__restrict__ gate, const float *__restrict__ x3D, NewPtsResult *__restrict__ res,
                                                        int32_t *__restrict__ matched) {
    __shared__ uint8_t sFree[kMaxCur];
    __shared__ int sHist[RUMI_HISTO_LENGTH], sKeep[RUMI_HISTO_LENGTH], sWave[16], sBase;
    const KFDev *kf = reinterpret_cast<const KFDev *>(blk);
    const KFDev &C = kf[0];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), n1 = C.n;
    const RumiKeyPoint *keys1 = at<RumiKeyPoint>(blk, C.keys);
    const int32_t *mp1 = at<int32_t>(blk, C.mp);
    for (int i = tid; i < n1; i += 1024) sFree[i] = mp1[i] < 0;
    if (tid == 0) sBase = 0;
    __syncthreads();
    for (int k = 0; k < nNeigh; k++) {
        const int32_t *candK = cand + (size_t)k * n1;
        int32_t *matchedK = matched ? matched + (size_t)k * n1 : nullptr;
        const int before = sBase;
        if (res->skipped[k]) {                               // LocalMapping.cc:417-418
            if (matched) for (int i = tid; i < n1; i += 1024) matchedK[i] = -1;
            if (tid == 0) res->perNeigh[k] = 0;
            continue;
        }
        const RumiKeyPoint *keys2 = at<RumiKeyPoint>(blk, kf[1 + k].keys);
        if (tid < RUMI_HISTO_LENGTH) { sHist[tid] = 0; sKeep[tid] = 1; }
        __syncthreads();
        if (checkOri) {                                      // ORBmatcher.cc:964-1001 over the pairs the sequential search finds
            for (int i = tid; i < n1; i += 1024) {
                const int f = sFree[i] ? candK[i] : -1;
                if (f >= 0) atomicAdd(&sHist[rot_bin(keys1[i].angle, keys2[f].angle)], 1);
            }
            __syncthreads();
            if (tid == 0) {                                  // ComputeThreeMaxima, as k_tri_filter has it
                int max1 = 0, max2 = 0, max3 = 0, ind1 = -1, ind2 = -1, ind3 = -1;
                for (int i = 0; i < RUMI_HISTO_LENGTH; i++) {
                    const int s = sHist[i];
                    if (s > max1) { max3 = max2; max2 = max1; max1 = s; ind3 = ind2; ind2 = ind1; ind1 = i; }
                    else if (s > max2) { max3 = max2; max2 = s; ind3 = ind2; ind2 = i; }
                    else if (s > max3) { max3 = s; ind3 = i; }
                }
                if ((float)max2 < 0.1f * (float)max1) { ind2 = -1; ind3 = -1; }
                else if ((float)max3 < 0.1f * (float)max1) ind3 = -1;
                for (int i = 0; i < RUMI_HISTO_LENGTH; i++) sKeep[i] = (i == ind1 || i == ind2 || i == ind3);
            }
            __syncthreads();
        }
        for (int c0 = 0; c0 < n1; c0 += 1024) {
            const int i = c0 + tid;
            int idx2 = -1;
            bool emit = false;
            if (i < n1) {
                const int f = sFree[i] ? candK[i] : -1;
                if (f >= 0 && (!checkOri || sKeep[rot_bin(keys1[i].angle, keys2[f].angle)])) { idx2 = f; emit = gate[(size_t)k * n1 + i] == GATE_OK; }
                if (matched) matchedK[i] = idx2;
            }
            const unsigned long long b = __ballot(emit);
            if (lane == 0) sWave[wave] = __popcll(b);
            __syncthreads();
            int off = sBase;
            for (int w = 0; w < wave; w++) off += sWave[w];
            if (emit) {
                const int c = off + __popcll(b & ((1ull << lane) - 1));
                const float *x = x3D + 3 * ((size_t)k * n1 + i);
                RumiNewPoint P;
                P.neigh = k; P.idx1 = i; P.idx2 = idx2; P.x3D[0] = x[0]; P.x3D[1] = x[1]; P.x3D[2] = x[2];
                res->pts[c] = P;
                sFree[i] = 0;                                // mpCurrentKeyFrame->AddMapPoint(pMP, idx1), :636
            }
            __syncthreads();
            if (tid == 0) { int t = sBase; for (int w = 0; w < 16; w++) t += sWave[w]; sBase = t; }
            __syncthreads();
        }
        if (tid == 0) res->perNeigh[k] = sBase - before;
    }
    __syncthreads();
    if (tid == 0) res->nOut = sBase;
}

// ---- host -------------------------------------------------------------------------------------------------------------------------------
struct NewPtsState {
    MirrorBuf<uint8_t> blk, res;                             // the upload block; the result block, a NewPtsResult and its points
    DevBuf<int32_t> cand, matched; DevBuf<uint8_t> gate; DevBuf<float> x3D;      // a candidate, a gate and a point (three floats) per (neighbour, feature) pair
    int lastNeigh = 0, lastN1 = 0, lastOri = 0;              // the last call, whose device state rumi_hook_newpts_matches replays
};

static void newpts_destroy(void *p) { delete static_cast<NewPtsState *>(p); }     // rumi_match_destroy has made the matcher's device current

static bool kf_valid(const RumiNewPointsKF &k, bool neighbour, const char **why) {
    const RumiFrameFeatures &f = k.feat;
    const RumiFeatureVector &v = k.fv;
    *why = "RumiNewPointsKF: bad sizes or missing arrays";
    if (f.n < 0 || f.nlevels < 1 || f.nlevels > 64 || !f.scale_factors || v.n_nodes < 0) return false;
    if (f.n > 0 && (!f.keys_un || !f.desc || !k.kf_mp)) return false;
    if (v.n_nodes > 0 && (!v.node_ids || !v.offsets || !v.indices)) return false;
    if (neighbour && f.n > 0 && !k.mp_pos) return false;
    *why = "RumiNewPointsKF: key-point octave outside mvScaleFactors";
    for (int i = 0; i < f.n; i++) if (f.keys_un[i].octave < 0 || f.keys_un[i].octave >= f.nlevels) return false;
    *why = "RumiNewPointsKF: FeatureVector offsets or indices out of range";
    if (v.n_nodes > 0) {
        if (v.offsets[0] != 0) return false;
        for (int a = 0; a < v.n_nodes; a++) if (v.offsets[a + 1] < v.offsets[a]) return false;
        for (int p = 0; p < v.offsets[v.n_nodes]; p++) if (v.indices[p] >= (uint32_t)f.n) return false;
        *why = "RumiNewPointsKF: FeatureVector node ids not strictly ascending, or a feature listed twice";
        for (int a = 1; a < v.n_nodes; a++) if (v.node_ids[a] <= v.node_ids[a - 1]) return false;      // the kernels search the ids by bisection
        std::vector<uint8_t> seen((size_t)f.n, 0);                                                      // one writer per cand[k][i1]
        for (int p = 0; p < v.offsets[v.n_nodes]; p++) { if (seen[v.indices[p]]) return false; seen[v.indices[p]] = 1; }
    }
    return true;
}

static size_t kf_bytes(const RumiNewPointsKF &k) {
    const size_t n = k.feat.n, nn = k.fv.n_nodes, ne = nn ? k.fv.offsets[nn] : 0;
    auto up = [](size_t b) { return (b + 15) & ~(size_t)15; };
    return up(n * sizeof(RumiKeyPoint)) + up(n * 32) + up(k.feat.nlevels * 4) + up(nn * 4) + up((nn + 1) * 4) + up(ne * 4) + up(n * 4) + up(n * 12);
}

static void kf_pack(const RumiNewPointsKF &k, bool neighbour, uint8_t *blk, size_t *used, KFDev *d) {
    const size_t n = k.feat.n, nn = k.fv.n_nodes, ne = nn ? k.fv.offsets[nn] : 0;
    auto put = [&](const void *src, size_t bytes) {
        const uint32_t off = (uint32_t)*used;
        if (src && bytes) std::memcpy(blk + off, src, bytes);
        *used = (*used + bytes + 15) & ~(size_t)15;
        return off;
    };
    static const int32_t kZero = 0;
    d->n = (int32_t)n; d->nn = (int32_t)nn; d->ne = (int32_t)ne; d->nlevels = k.feat.nlevels;
    d->keys = put(k.feat.keys_un, n * sizeof(RumiKeyPoint));
    d->desc = put(k.feat.desc, n * 32);
    d->scale = put(k.feat.scale_factors, (size_t)k.feat.nlevels * 4);
    d->nodes = put(k.fv.node_ids, nn * 4);
    d->off = put(nn ? (const void *)k.fv.offsets : (const void *)&kZero, (nn + 1) * 4);
    d->idx = put(k.fv.indices, ne * 4);
    d->mp = put(k.kf_mp, n * 4);
    d->pos = put(neighbour ? k.mp_pos : nullptr, n * 12);
    std::memcpy(d->K, k.K4, 16); std::memcpy(d->T, k.Tcw, 48); std::memcpy(d->Ow, k.Ow, 12);
    std::memcpy(d->F12, k.F12, 36); std::memcpy(d->ep, k.epipole2, 8);
    d->pad[0] = d->pad[1] = 0;
}

}  // namespace rumi

using namespace rumi;

extern "C" int rumi_create_new_map_points(RumiMatcher *m, const RumiNewPointsKF *cur, const RumiNewPointsKF *neigh, int32_t n_neigh,
                                          const RumiNewPointsParams *p, RumiNewPoint *out, int32_t cap, int32_t *n_out,
                                          int32_t *per_neigh_out, uint8_t *neigh_skipped_out) {
    if (!m || !cur || !p || !n_out || n_neigh < 0 || n_neigh > RUMI_NEWPTS_MAX_NEIGH || cap < 0 || (cap > 0 && !out) ||
        (n_neigh > 0 && (!neigh || !per_neigh_out || !neigh_skipped_out))) {
        g_lastError = "rumi_create_new_map_points: missing argument, or n_neigh outside 0..RUMI_NEWPTS_MAX_NEIGH";
        return RUMI_E_INVALID;
    }
    const char *why = "";
    if (!kf_valid(*cur, false, &why)) { g_lastError = why; return RUMI_E_INVALID; }
    for (int k = 0; k < n_neigh; k++) if (!kf_valid(neigh[k], true, &why)) { g_lastError = why; return RUMI_E_INVALID; }
    const int maxFeat = m->maxFeat, maxQ = m->maxQ;
    MatcherExt *ext = &m->ext;
    const int n1 = cur->feat.n;
    auto entries = [](const RumiNewPointsKF &k) { return k.fv.n_nodes ? k.fv.offsets[k.fv.n_nodes] : 0; };
    bool fits = n1 <= std::min(std::min(maxFeat, maxQ), kMaxCur) && entries(*cur) <= std::min(maxFeat, maxQ) && cur->fv.n_nodes <= std::min(maxFeat, maxQ);
    int maxN2 = 1;
    for (int k = 0; k < n_neigh; k++) {
        fits = fits && neigh[k].feat.n <= maxFeat && entries(neigh[k]) <= maxFeat && neigh[k].fv.n_nodes <= maxFeat;
        maxN2 = std::max(maxN2, neigh[k].feat.n);
    }
    if (!fits) {
        g_lastError = "CreateNewMapPoints: a key-frame exceeds the matcher's capacities (max_features / max_queries)";
        return RUMI_E_CAPACITY;
    }
    *n_out = 0;
    for (int k = 0; k < n_neigh; k++) { per_neigh_out[k] = 0; neigh_skipped_out[k] = 0; }
    if (n_neigh == 0) return RUMI_OK;
    HIP_TRY(hipSetDevice(m->device));
    if (!ext->state) { ext->state = new NewPtsState(); ext->destroy = newpts_destroy; }
    NewPtsState *s = static_cast<NewPtsState *>(ext->state);
    s->lastNeigh = 0; s->lastN1 = 0;

    // ---- arenas (grown on demand, like the BoW batch blocks of the matcher)
    size_t blkBytes = (size_t)(n_neigh + 1) * sizeof(KFDev) + kf_bytes(*cur);
    for (int k = 0; k < n_neigh; k++) blkBytes += kf_bytes(neigh[k]);
    int rc;
    const size_t pairs = (size_t)n_neigh * std::max(n1, 1);
    const size_t resBytes = sizeof(NewPtsResult) + (size_t)n1 * sizeof(RumiNewPoint);
    if ((rc = s->blk.reserve(blkBytes, blkBytes + blkBytes / 4)) != RUMI_OK || (rc = s->cand.reserve(pairs, pairs)) != RUMI_OK ||
        (rc = s->gate.reserve(pairs, pairs)) != RUMI_OK || (rc = s->x3D.reserve(pairs * 3, pairs * 3)) != RUMI_OK ||
        (rc = s->res.reserve(resBytes, resBytes)) != RUMI_OK)
        return rc;
    NewPtsResult *dRes = reinterpret_cast<NewPtsResult *>(s->res.d);

    // ---- one block up
    size_t used = (size_t)(n_neigh + 1) * sizeof(KFDev);
    KFDev *tab = reinterpret_cast<KFDev *>(s->blk.h);
    kf_pack(*cur, false, s->blk.h, &used, &tab[0]);
    for (int k = 0; k < n_neigh; k++) kf_pack(neigh[k], true, s->blk.h, &used, &tab[1 + k]);
    HIP_TRY(hipMemcpyAsync(s->blk.d, s->blk.h, used, hipMemcpyHostToDevice, nullptr));
    HIP_TRY(hipMemsetAsync(s->cand.p, 0xFF, pairs * 4, nullptr));
    HIP_TRY(hipMemsetAsync(dRes, 0, sizeof(NewPtsResult), nullptr));

    // ---- four launches
    hipLaunchKernelGGL(k_newpts_depth, dim3((maxN2 + 255) / 256, n_neigh), dim3(256), 0, nullptr, s->blk.d, dRes->skipped);
    if (n1 > 0) {
        if (cur->fv.n_nodes > 0)
            hipLaunchKernelGGL(k_newpts_match, dim3((cur->fv.n_nodes + 3) / 4, n_neigh), dim3(256), 0, nullptr, s->blk.d, p->coarse, s->cand.p);
        hipLaunchKernelGGL(k_newpts_triangulate, dim3((n1 + 255) / 256, n_neigh), dim3(256), 0, nullptr, s->blk.d, s->cand.p, p->far_points,
                           p->th_far_points, p->ratio_factor, s->gate.p, s->x3D.p);
    }
    hipLaunchKernelGGL(k_newpts_replay, dim3(1), dim3(1024), 0, nullptr, s->blk.d, n_neigh, p->check_orientation, s->cand.p, s->gate.p, s->x3D.p,
                       dRes, (int32_t *)nullptr);
    HIP_TRY(hipGetLastError());

    // ---- one block back
    HIP_TRY(hipMemcpy(s->res.h, dRes, resBytes, hipMemcpyDeviceToHost));
    s->lastNeigh = n_neigh; s->lastN1 = n1; s->lastOri = p->check_orientation;
    const NewPtsResult *r = reinterpret_cast<const NewPtsResult *>(s->res.h);
    *n_out = r->nOut;
    for (int k = 0; k < n_neigh; k++) { per_neigh_out[k] = r->perNeigh[k]; neigh_skipped_out[k] = (uint8_t)r->skipped[k]; }
    if (std::min(r->nOut, cap) > 0) std::memcpy(out, r->pts, (size_t)std::min(r->nOut, cap) * sizeof(RumiNewPoint));
    if (r->nOut > cap) {
        g_lastError = "CreateNewMapPoints: more points than the output list holds (cap)";
        return RUMI_E_CAPACITY;
    }
    return RUMI_OK;
}

extern "C" int rumi_hook_newpts_matches(RumiMatcher *m, int32_t n_neigh, int32_t n1, int32_t *matches) {
    if (!m || !matches) return RUMI_E_INVALID;
    NewPtsState *s = static_cast<NewPtsState *>(m->ext.state);
    if (!s || s->lastNeigh != n_neigh || s->lastN1 != n1 || (size_t)n_neigh * n1 == 0) {
        g_lastError = "rumi_hook_newpts_matches: no rumi_create_new_map_points call of that shape precedes";
        return RUMI_E_INVALID;
    }
    HIP_TRY(hipSetDevice(m->device));
    // the last call's block, candidates, gates and skip flags are still on the device: the replay runs once more, this time recording its matches
    // (it rewrites the result block with the same bytes)
    const size_t pairs = (size_t)n_neigh * n1;
    const int rc = s->matched.reserve(pairs, pairs);
    if (rc != RUMI_OK) return rc;
    hipLaunchKernelGGL(k_newpts_replay, dim3(1), dim3(1024), 0, nullptr, s->blk.d, n_neigh, s->lastOri, s->cand.p, s->gate.p, s->x3D.p, reinterpret_cast<NewPtsResult *>(s->res.d), s->matched.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(matches, s->matched.p, pairs * 4, hipMemcpyDeviceToHost));
    return RUMI_OK;
}
