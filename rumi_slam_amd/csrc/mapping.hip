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
//
// The searches of LocalMapping::SearchInNeighbors over the same store: search_in_neighbors.inc, included at the end of this file; those of
// LoopClosing::SearchAndFuse: search_and_fuse.inc, after it.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
#include <memory>
#include <string>
#include <type_traits>
#include <vector>

#include "rumi_mapping.h"
#include "rumi_testhooks.h"
#include "keyframe_features.h"
#include "match_host.h"
#include "match_grid.h"
#include "match_bow_stage.h"

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

// ---- views --------------------------------------------------------------------------------------------------------------------------------
// The four kernels below read a key-frame through a view: view.kf(i) is key-frame i of the call (0 = the current one), and what it returns
// names every array and small matrix.  The kernels hold the arithmetic once; the two entries differ only in where the bytes lie.
//   BlockView     rumi_create_new_map_points: everything inside the call's upload block, arrays at blk + offset.
//   ResidentView  rumi_create_new_map_points_resident: a CovisKeyFrame of the covisibility store (covis_view.h), positions in the scratch
//                 k_newpts_gather filled, poses in the call's table.
struct BlockView {
    const uint8_t *blk;
    struct KF {
        const uint8_t *blk; const KFDev *d;
        __device__ __forceinline__ int n() const { return d->n; }
        __device__ __forceinline__ int nn() const { return d->nn; }
        __device__ __forceinline__ const RumiKeyPoint *keys() const { return at<RumiKeyPoint>(blk, d->keys); }
        __device__ __forceinline__ const uint8_t *desc() const { return blk + d->desc; }
        __device__ __forceinline__ const float *scale() const { return at<float>(blk, d->scale); }
        __device__ __forceinline__ const uint32_t *nodes() const { return at<uint32_t>(blk, d->nodes); }
        __device__ __forceinline__ const int32_t *off() const { return at<int32_t>(blk, d->off); }
        __device__ __forceinline__ const uint32_t *idx() const { return at<uint32_t>(blk, d->idx); }
        __device__ __forceinline__ const int32_t *mp() const { return at<int32_t>(blk, d->mp); }
        __device__ __forceinline__ const float *pos() const { return at<float>(blk, d->pos); }
        __device__ __forceinline__ const float *K() const { return d->K; }
        __device__ __forceinline__ const float *T() const { return d->T; }
        __device__ __forceinline__ const float *Ow() const { return d->Ow; }
        __device__ __forceinline__ const float *F12() const { return d->F12; }
        __device__ __forceinline__ const float *ep() const { return d->ep; }
    };
    __device__ __forceinline__ KF kf(int i) const { return KF{blk, reinterpret_cast<const KFDev *>(blk) + i}; }
};

// One key-frame of a resident call: where its block, its row and its positions lie, and the pose by value.
struct ResKF : CovisSlotRef {
    uint32_t posOff;                   // first float of its positions in the gather scratch (neighbours)
    float T[12], Ow[3], F12[9], ep[2];
};
static_assert(sizeof(ResKF) == 128, "a pose record");

struct ResidentView {
    const ResKF *tab; CovisView s; const float *pos;
    struct KF : CovisKeyFrame {
        const ResKF *p; const float *xyz;
        __device__ __forceinline__ const float *pos() const { return xyz; }
        __device__ __forceinline__ const float *T() const { return p->T; }
        __device__ __forceinline__ const float *Ow() const { return p->Ow; }
        __device__ __forceinline__ const float *F12() const { return p->F12; }
        __device__ __forceinline__ const float *ep() const { return p->ep; }
    };
    __device__ __forceinline__ KF kf(int i) const {
        const ResKF *p = tab + i;
        return KF{s.key_frame(*p), p, pos + p->posOff};
    }
};

// ---- 1. search --------------------------------------------------------------------------------------------------------------------------
// One wavefront per (neighbour, node of the current key-frame's FeatureVector).  Lanes hold the candidates of the neighbour's node (descriptor,
// key-point, epipole test: loaded once per 64 candidates); the node's current features go by one at a time, wave-uniform, and each is reduced
// over the lanes on the key ~((dist << 16) | (0xffff - position)): the maximum is the smallest distance, the LATER position on ties
// (`dist > bestDist` rejects, ORBmatcher.cc:905).  Lane j keeps the running key of the tile's feature j, so nodes of more than 64
// candidates need no memory between chunks.  A wave rather than half of one: a node at levelsup = 4 holds ~20 features a side, and the
// cost is the 20 uniform steps, not the idle lanes; two nodes a wave would double the steps' register state for no shorter chain.
template <class View> __global__ __launch_bounds__(256) void k_newpts_match(const View view, int coarse, int32_t *__restrict__ cand) {
    const int lane = threadIdx.x & 63;
    const int a = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6)), k = blockIdx.y;
    const typename View::KF C = view.kf(0), N = view.kf(1 + k);
    const int nn1 = C.nn(), nn2 = N.nn(), n1 = C.n();
    if (a >= nn1) return;
    const int lo = fv_find_node(N.nodes(), nn2, C.nodes()[a]);
    if (lo < 0) return;
    const int32_t *off1 = C.off(), *off2 = N.off(), *mp1 = C.mp(), *mp2 = N.mp();
    const uint32_t *idx1 = C.idx(), *idx2 = N.idx();
    const RumiKeyPoint *keys1 = C.keys(), *keys2 = N.keys();
    const uint8_t *desc1 = C.desc(), *desc2 = N.desc();
    const float *scale2 = N.scale();
    const float *F = N.F12();
    const float epx = N.ep()[0], epy = N.ep()[1];
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
        if (p < pe && mine != 0) cand[(size_t)k * n1 + idx1[p]] = (int32_t)idx2[0xffff - (~mine & 0xffff)];
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
template <class View>
__global__ __launch_bounds__(256) void k_newpts_triangulate(const View view, const int32_t *__restrict__ cand, int farPoints,
                                                            float thFar, float ratioFactor, uint8_t *__restrict__ gate, float *__restrict__ x3Dout) {
    const typename View::KF C = view.kf(0), N = view.kf(1 + blockIdx.y);
    const int i1 = blockIdx.x * blockDim.x + threadIdx.x, n1 = C.n();
    if (i1 >= n1) return;
    const size_t slot = (size_t)blockIdx.y * n1 + i1;
    const int i2 = cand[slot];
    if (i2 < 0) return;
    const RumiKeyPoint kp1 = C.keys()[i1], kp2 = N.keys()[i2];
    const float *T1 = C.T(), *T2 = N.T(), *K1 = C.K(), *K2 = N.K(), *Ow1 = C.Ow(), *Ow2 = N.Ow();
    // :507-512  unprojectEig (Pinhole.cpp:61-64), rays, parallax
    const float xn1[3] = {(kp1.x - K1[2]) / K1[0], (kp1.y - K1[3]) / K1[1], 1.f};
    const float xn2[3] = {(kp2.x - K2[2]) / K2[0], (kp2.y - K2[3]) / K2[1], 1.f};
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
            const float sf1 = C.scale()[kp1.octave], sf2 = N.scale()[kp2.octave];
            const float sig1 = sf1 * sf1, sig2 = sf2 * sf2;
            const float x1 = dot3(T1[0], T1[1], T1[2], x3D[0], x3D[1], x3D[2]) + T1[3];          // :563-574
            const float y1 = dot3(T1[4], T1[5], T1[6], x3D[0], x3D[1], x3D[2]) + T1[7];
            const float eX1 = (K1[0] * x1 / z1 + K1[2]) - kp1.x, eY1 = (K1[1] * y1 / z1 + K1[3]) - kp1.y;
            const float x2 = dot3(T2[0], T2[1], T2[2], x3D[0], x3D[1], x3D[2]) + T2[3];          // :588-597
            const float y2 = dot3(T2[4], T2[5], T2[6], x3D[0], x3D[1], x3D[2]) + T2[7];
            const float eX2 = (K2[0] * x2 / z2 + K2[2]) - kp2.x, eY2 = (K2[1] * y2 / z2 + K2[3]) - kp2.y;
            const float dist1 = norm3(x3D[0] - Ow1[0], x3D[1] - Ow1[1], x3D[2] - Ow1[2]);          // :610-626
            const float dist2 = norm3(x3D[0] - Ow2[0], x3D[1] - Ow2[1], x3D[2] - Ow2[2]);
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
template <class View> __global__ __launch_bounds__(256) void k_newpts_depth(const View view, int32_t *__restrict__ skipped) {
    __shared__ __attribute__((aligned(16))) float sZ[kDepthTile];
    __shared__ int sCount;
    const typename View::KF C = view.kf(0), N = view.kf(1 + blockIdx.y);
    const int tid = threadIdx.x, n = N.n(), i = blockIdx.x * 256 + tid;
    if (blockIdx.x > 0 && (int)blockIdx.x * 256 >= n) return;
    const int32_t *mp = N.mp();
    const float *pos = N.pos(), *T2 = N.T();
    auto depth = [&](int j) {                                 // :964-971, NaN where the feature holds no point
        return j < n && mp[j] >= 0 ? dot3(T2[8], T2[9], T2[10], pos[3 * j], pos[3 * j + 1], pos[3 * j + 2]) + T2[11] : __builtin_nanf("");
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
        const float *Ow1 = C.Ow(), *Ow2 = N.Ow();
        const float baseline = norm3(Ow2[0] - Ow1[0], Ow2[1] - Ow1[1], Ow2[2] - Ow1[2]);
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
// its own thread; the histogram uses integer LDS atomics (order-free), the emission is an ordered compaction (block_ordered_slot).
// matched (may be null: only rumi_hook_newpts_matches passes it) receives stages 1 + 3 per neighbour.
template <class View>
__global__ __launch_bounds__(1024) void k_newpts_replay(const View view, int nNeigh, int checkOri, const int32_t *__restrict__ cand,
                                                        const uint8_t *__restrict__ gate, const float *__restrict__ x3D, NewPtsResult *__restrict__ res,
                                                        int32_t *__restrict__ matched) {
    __shared__ uint8_t sFree[kMaxCur];
    __shared__ int sHist[RUMI_HISTO_LENGTH], sKeep[RUMI_HISTO_LENGTH], sWave[16], sBase;
    const typename View::KF C = view.kf(0);
    const int tid = threadIdx.x, n1 = C.n();
    const RumiKeyPoint *keys1 = C.keys();
    const int32_t *mp1 = C.mp();
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
        const RumiKeyPoint *keys2 = view.kf(1 + k).keys();
        if (tid < RUMI_HISTO_LENGTH) { sHist[tid] = 0; sKeep[tid] = 1; }
        __syncthreads();
        if (checkOri) {                                      // ORBmatcher.cc:964-1001 over the pairs the sequential search finds
            for (int i = tid; i < n1; i += 1024) {
                const int f = sFree[i] ? candK[i] : -1;
                if (f >= 0) atomicAdd(&sHist[rot_bin(keys1[i].angle, keys2[f].angle)], 1);
            }
            __syncthreads();
            if (tid == 0) three_maxima_keep(sHist, sKeep);
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
            block_ordered_slot(emit, sWave, &sBase, [&](int c) {
                const float *x = x3D + 3 * ((size_t)k * n1 + i);
                RumiNewPoint P;
                P.neigh = k; P.idx1 = i; P.idx2 = idx2; P.x3D[0] = x[0]; P.x3D[1] = x[1]; P.x3D[2] = x[2];
                res->pts[c] = P;
                sFree[i] = 0;                                // mpCurrentKeyFrame->AddMapPoint(pMP, idx1), :636
            });
        }
        if (tid == 0) res->perNeigh[k] = sBase - before;
    }
    __syncthreads();
    if (tid == 0) res->nOut = sBase;
}

// ---- 0. the resident entry's gather -----------------------------------------------------------------------------------------------------
// One lane per (neighbour, feature): the feature's entry in the neighbour's mp row, and where it names a point, the 12 position bytes of the
// point's 64-byte attribute record (covis.hip) into pos[posOff + 3 i]: what the block entry gets as mp_pos.  An entry whose point has no
// attributes is counted (integer atomic; the order does not matter) and the host refuses the call.  The current key-frame's positions
// are not read, as with mp_pos == NULL.
__global__ __launch_bounds__(256) void k_newpts_gather(const ResKF *__restrict__ tab, CovisView s, int32_t *__restrict__ pos, int32_t *__restrict__ missing) {
    const ResKF &N = tab[1 + blockIdx.y];
    const int n = s.rec(N.block)->n, i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int p = s.mp_row(N)[i];
    if (p < 0) return;
    if (!s.has_attr(p)) { atomicAdd(missing, 1); return; }
    const int32_t *A = s.attr_rec(p);
    int32_t *o = pos + N.posOff + 3 * (size_t)i;
    o[0] = A[0]; o[1] = A[1]; o[2] = A[2];
}

// ---- host -------------------------------------------------------------------------------------------------------------------------------
// What the entries of this file keep on a RumiMatcher (MatcherExt, rumi_internal.h): one NewPtsState, made by the first call of any of them, so that
// the blocks live and die with the handle.  Each by-slot search owns a part of it that is made by ITS first call: that is how its *_stage_ms
// knows that no call precedes.
struct SinState {                                            // rumi_search_in_neighbors_resident (search_in_neighbors.inc)
    MirrorBuf<uint8_t> tab;                                  // the table of SinKF
    MirrorBuf<int32_t> res;                                  // [head SIN_HEAD][fwd nT * nCur][revPoint E][revBest E], E = the targets' row entries
    DevBuf<uint16_t> sorted; DevBuf<int32_t> cellStart, blocks;
    DevBuf<uint32_t> slotTag; DevBuf<unsigned long long> claim;      // the stamped tables, which SearchAndFuse and the Sim3 projection search share
    DevBuf<uint4> work;
    uint32_t epoch = 0;
    StageClock clock;
    float stageMs[3] = {0.f, 0.f, 0.f};
};
struct SafState {                                            // rumi_search_and_fuse_resident (search_and_fuse.inc)
    MirrorBuf<uint8_t> up;                                   // the table of SinKF, then the ids
    MirrorBuf<int32_t> res;                                  // [head SIN_HEAD][per_kf nK][hits: 4 words each]
    DevBuf<int32_t> dense, cellStart, blocks;                // [nK][nP] best index per pair; the grids; block counts and bases
    DevBuf<uint16_t> sorted;
    DevBuf<uint4> work;
    StageClock clock;
    float stageMs[3] = {0.f, 0.f, 0.f};
};
struct S3pState {                                            // rumi_search_by_projection_sim3_resident (sim3_projection_batch.inc)
    MirrorBuf<uint8_t> up;                                   // the grids' SinKF, the jobs' S3pJob, the ids
    MirrorBuf<int32_t> res;                                  // [head SIN_HEAD][nmatches nJ][rounds nJ][rows]
    DevBuf<int32_t> pair, cellStart;                         // [4][pairs] counts, cursors, list starts, held features; the grids
    DevBuf<uint16_t> sorted;
    DevBuf<uint4> work;
    DevBuf<uint2> lists;
    std::vector<int32_t> rounds;                             // of the last call, per job
    StageClock clock;
    float stageMs[3] = {0.f, 0.f, 0.f};
};
struct CrrState {                                            // rumi_common_regions_bow_resident (common_regions_resident.inc)
    MirrorBuf<uint8_t> up;                                   // [BowSlotKF nM | group starts nG + 1]
    MirrorBuf<int32_t> res;                                  // CrResultLayout
    DevBuf<int8_t> rotBin;                                   // [nM][n]
    DevBuf<unsigned long long> first;                        // [groups][max_points], stamped
    size_t firstGroups = 0, firstPoints = 0;                 // the shape `first` was allocated for
    uint32_t epoch = 0;
    StageClock clock;
    float stageMs[3] = {0.f, 0.f, 0.f};
};

struct NewPtsState {
    MirrorBuf<uint8_t> blk, res;                             // the upload block; the result block, a NewPtsResult and its points
    DevBuf<int32_t> cand, matched; DevBuf<uint8_t> gate; DevBuf<float> x3D;      // a candidate, a gate and a point (three floats) per (neighbour, feature) pair
    MirrorBuf<uint8_t> tab; DevBuf<int32_t> pos;             // the resident entry: its table of ResKF, the gathered positions
    int lastNeigh = 0, lastN1 = 0, lastOri = 0;              // the last block call, whose device state rumi_hook_newpts_matches replays
    StageClock clock;
    float stageMs[3] = {0.f, 0.f, 0.f};
    std::unique_ptr<SinState> sin;                           // with the first SearchInNeighbors, SearchAndFuse or Sim3 projection call (the stamped tables)
    std::unique_ptr<SafState> saf;
    std::unique_ptr<S3pState> s3p;
    std::unique_ptr<CrrState> crr;
};

static void newpts_destroy(void *p) { delete static_cast<NewPtsState *>(p); }       // rumi_match_destroy has made the matcher's device current

// This matcher's state, and a part of it, each made on first use.
static NewPtsState *newpts_state(RumiMatcher *m) {
    if (!m->ext.state) { m->ext.state = new NewPtsState(); m->ext.destroy = newpts_destroy; }
    return static_cast<NewPtsState *>(m->ext.state);
}
template <class T> static T *made(std::unique_ptr<T> &part) {
    if (!part) part.reset(new T());
    return part.get();
}
// What a *_stage_ms entry reads: the part if its entry has been called on this matcher, else null.
static const NewPtsState *newpts_peek(const RumiMatcher *m) { return m ? static_cast<const NewPtsState *>(m->ext.state) : nullptr; }

static bool kf_valid(const RumiNewPointsKF &k, bool neighbour, const char **why) {
    *why = "key-frame features: bad sizes or missing arrays";
    if (k.feat.n > 0 && (!k.kf_mp || (neighbour && !k.mp_pos))) return false;
    return keyframe_features_valid(k.feat, k.fv, why);
}

static size_t kf_bytes(const RumiNewPointsKF &k) {
    const size_t n = k.feat.n, nn = k.fv.n_nodes, ne = nn ? k.fv.offsets[nn] : 0;
    return up16(n * sizeof(RumiKeyPoint)) + up16(n * 32) + up16(k.feat.nlevels * 4) + up16(nn * 4) + up16((nn + 1) * 4) + up16(ne * 4) + up16(n * 4) + up16(n * 12);
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

// ---- what both entries share behind their uploads
static int newpts_reserve(NewPtsState *s, int n_neigh, int n1) {
    const size_t pairs = (size_t)n_neigh * std::max(n1, 1), resBytes = sizeof(NewPtsResult) + (size_t)n1 * sizeof(RumiNewPoint);
    int rc;
    if ((rc = s->cand.reserve(pairs, pairs)) != RUMI_OK || (rc = s->gate.reserve(pairs, pairs)) != RUMI_OK ||
        (rc = s->x3D.reserve(pairs * 3, pairs * 3)) != RUMI_OK || (rc = s->res.reserve(resBytes, resBytes)) != RUMI_OK)
        return rc;
    return RUMI_OK;
}

// The four launches over `view` and the result block back into s->res.h.  The block entry clears the result block's header here; the
// resident entry has cleared it before its gather, which counts into it.
template <class View> static int newpts_run(NewPtsState *s, const View &view, int n_neigh, int n1, int nNodes1, int maxN2, const RumiNewPointsParams *p) {
    const size_t pairs = (size_t)n_neigh * std::max(n1, 1), resBytes = sizeof(NewPtsResult) + (size_t)n1 * sizeof(RumiNewPoint);
    NewPtsResult *dRes = reinterpret_cast<NewPtsResult *>(s->res.d);
    HIP_TRY(hipMemsetAsync(s->cand.p, 0xFF, pairs * 4, nullptr));
    if (std::is_same<View, BlockView>::value) HIP_TRY(hipMemsetAsync(dRes, 0, sizeof(NewPtsResult), nullptr));
    hipLaunchKernelGGL(k_newpts_depth<View>, dim3((maxN2 + 255) / 256, n_neigh), dim3(256), 0, nullptr, view, dRes->skipped);
    if (n1 > 0) {
        if (nNodes1 > 0)
            hipLaunchKernelGGL(k_newpts_match<View>, dim3((nNodes1 + 3) / 4, n_neigh), dim3(256), 0, nullptr, view, p->coarse, s->cand.p);
        hipLaunchKernelGGL(k_newpts_triangulate<View>, dim3((n1 + 255) / 256, n_neigh), dim3(256), 0, nullptr, view, s->cand.p, p->far_points,
                           p->th_far_points, p->ratio_factor, s->gate.p, s->x3D.p);
    }
    hipLaunchKernelGGL(k_newpts_replay<View>, dim3(1), dim3(1024), 0, nullptr, view, n_neigh, p->check_orientation, s->cand.p, s->gate.p, s->x3D.p,
                       dRes, (int32_t *)nullptr);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(s->res.h, dRes, resBytes, hipMemcpyDeviceToHost));      // one block back
    s->clock.mark();
    return RUMI_OK;
}

static int newpts_write_out(NewPtsState *s, int n_neigh, RumiNewPoint *out, int32_t cap, int32_t *n_out, int32_t *per_neigh_out, uint8_t *neigh_skipped_out) {
    const NewPtsResult *r = reinterpret_cast<const NewPtsResult *>(s->res.h);
    *n_out = r->nOut;
    for (int k = 0; k < n_neigh; k++) { per_neigh_out[k] = r->perNeigh[k]; neigh_skipped_out[k] = (uint8_t)r->skipped[k]; }
    if (std::min(r->nOut, cap) > 0) std::memcpy(out, r->pts, (size_t)std::min(r->nOut, cap) * sizeof(RumiNewPoint));
    s->clock.finish(s->stageMs);
    if (r->nOut > cap) {
        g_lastError = "CreateNewMapPoints: more points than the output list holds (cap)";
        return RUMI_E_CAPACITY;
    }
    return RUMI_OK;
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
    const auto t0 = std::chrono::steady_clock::now();
    const char *why = "";
    if (!kf_valid(*cur, false, &why)) { g_lastError = why; return RUMI_E_INVALID; }
    for (int k = 0; k < n_neigh; k++) if (!kf_valid(neigh[k], true, &why)) { g_lastError = why; return RUMI_E_INVALID; }
    const int maxFeat = m->maxFeat, maxQ = m->maxQ;
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
    NewPtsState *s = newpts_state(m);
    s->lastNeigh = 0; s->lastN1 = 0;
    s->clock.start(); s->clock.t[0] = t0;                    // the validation above belongs to the host stage

    // ---- arenas (grown on demand, like the BoW batch blocks of the matcher)
    size_t blkBytes = (size_t)(n_neigh + 1) * sizeof(KFDev) + kf_bytes(*cur);
    for (int k = 0; k < n_neigh; k++) blkBytes += kf_bytes(neigh[k]);
    int rc;
    if ((rc = s->blk.reserve(blkBytes, blkBytes + blkBytes / 4)) != RUMI_OK || (rc = newpts_reserve(s, n_neigh, n1)) != RUMI_OK) return rc;

    // ---- one block up
    size_t used = (size_t)(n_neigh + 1) * sizeof(KFDev);
    KFDev *tab = reinterpret_cast<KFDev *>(s->blk.h);
    kf_pack(*cur, false, s->blk.h, &used, &tab[0]);
    for (int k = 0; k < n_neigh; k++) kf_pack(neigh[k], true, s->blk.h, &used, &tab[1 + k]);
    s->clock.mark();
    HIP_TRY(hipMemcpyAsync(s->blk.d, s->blk.h, used, hipMemcpyHostToDevice, nullptr));
    if ((rc = newpts_run(s, BlockView{s->blk.d}, n_neigh, n1, cur->fv.n_nodes, maxN2, p)) != RUMI_OK) return rc;
    s->lastNeigh = n_neigh; s->lastN1 = n1; s->lastOri = p->check_orientation;
    return newpts_write_out(s, n_neigh, out, cap, n_out, per_neigh_out, neigh_skipped_out);
}

extern "C" int rumi_create_new_map_points_resident(RumiMatcher *m, RumiCovis *c, int32_t cur_slot, const RumiNewPointsPose *cur_pose,
                                                   const int32_t *neigh_slots, const RumiNewPointsPose *neigh_pose, int32_t n_neigh,
                                                   const RumiNewPointsParams *p, RumiNewPoint *out, int32_t cap, int32_t *n_out,
                                                   int32_t *per_neigh_out, uint8_t *neigh_skipped_out) {
    static const char *entry = "rumi_create_new_map_points_resident";
    if (!m || !c || !cur_pose || !p || !n_out || n_neigh < 0 || n_neigh > RUMI_NEWPTS_MAX_NEIGH || cap < 0 || (cap > 0 && !out) ||
        (n_neigh > 0 && (!neigh_slots || !neigh_pose || !per_neigh_out || !neigh_skipped_out))) {
        g_lastError = std::string(entry) + ": missing argument, or n_neigh outside 0..RUMI_NEWPTS_MAX_NEIGH";
        return RUMI_E_INVALID;
    }
    const auto t0 = std::chrono::steady_clock::now();
    int32_t slots[RUMI_NEWPTS_MAX_NEIGH + 1];
    CovisSlotFeatures info[RUMI_NEWPTS_MAX_NEIGH + 1];
    slots[0] = cur_slot;
    for (int k = 0; k < n_neigh; k++) slots[1 + k] = neigh_slots[k];
    int rc;
    if ((rc = covis_features_check(c, n_neigh + 1, slots, entry, info)) != RUMI_OK || (n_neigh > 0 && (rc = covis_same_device(c, m->device, entry)) != RUMI_OK)) return rc;
    const int lim = std::min(m->maxFeat, m->maxQ), n1 = info[0].n;
    bool fits = n1 <= std::min(lim, kMaxCur) && info[0].ne <= lim && info[0].nn <= lim;
    int maxN2 = 1;
    size_t posFloats = 0;
    for (int k = 1; k <= n_neigh; k++) {
        fits = fits && info[k].n <= m->maxFeat && info[k].ne <= m->maxFeat && info[k].nn <= m->maxFeat;
        maxN2 = std::max(maxN2, info[k].n);
        posFloats += 3 * (size_t)info[k].n;
    }
    if (!fits) {
        g_lastError = "CreateNewMapPoints: a key-frame exceeds the matcher's capacities (max_features / max_queries)";
        return RUMI_E_CAPACITY;
    }
    if (n_neigh == 0) { *n_out = 0; return RUMI_OK; }
    HIP_TRY(hipSetDevice(m->device));
    NewPtsState *s = newpts_state(m);
    s->lastNeigh = 0; s->lastN1 = 0;                         // the hook replays the block path's state, which this call overwrites
    s->clock.start(); s->clock.t[0] = t0;

    const size_t tabBytes = (size_t)(n_neigh + 1) * sizeof(ResKF);
    if ((rc = s->tab.reserve(tabBytes, (RUMI_NEWPTS_MAX_NEIGH + 1) * sizeof(ResKF))) != RUMI_OK ||
        (rc = s->pos.reserve(posFloats, posFloats + posFloats / 4)) != RUMI_OK || (rc = newpts_reserve(s, n_neigh, n1)) != RUMI_OK)
        return rc;
    // ---- the table of poses: all that travels for this call, besides what the store had staged
    ResKF *tab = reinterpret_cast<ResKF *>(s->tab.h);
    uint32_t posOff = 0;
    for (int k = 0; k <= n_neigh; k++) {
        const RumiNewPointsPose &P = k ? neigh_pose[k - 1] : *cur_pose;
        ResKF &R = tab[k];
        static_cast<CovisSlotRef &>(R) = covis_slot_ref(info[k]); R.posOff = k ? posOff : 0;
        std::memcpy(R.T, P.Tcw, 48); std::memcpy(R.Ow, P.Ow, 12); std::memcpy(R.F12, P.F12, 36); std::memcpy(R.ep, P.epipole2, 8);
        if (k) posOff += 3u * (uint32_t)info[k].n;
    }
    s->clock.mark();
    CovisView fv;
    if ((rc = covis_view(c, 0, &fv)) != RUMI_OK) return rc;
    HIP_TRY(hipMemcpyAsync(s->tab.d, s->tab.h, tabBytes, hipMemcpyHostToDevice, nullptr));
    NewPtsResult *dRes = reinterpret_cast<NewPtsResult *>(s->res.d);
    HIP_TRY(hipMemsetAsync(dRes, 0, sizeof(NewPtsResult), nullptr));
    const ResKF *dTab = reinterpret_cast<const ResKF *>(s->tab.d);
    hipLaunchKernelGGL(k_newpts_gather, dim3((maxN2 + 255) / 256, n_neigh), dim3(256), 0, nullptr, dTab, fv, s->pos.p, &dRes->pad[0]);
    if ((rc = newpts_run(s, ResidentView{dTab, fv, reinterpret_cast<const float *>(s->pos.p)}, n_neigh, n1, info[0].nn, maxN2, p)) != RUMI_OK)
        return rc;
    const int missing = reinterpret_cast<const NewPtsResult *>(s->res.h)->pad[0];
    if (missing) {
        g_lastError = std::string(entry) + ": " + std::to_string(missing) + " neighbour map point(s) without attributes (rumi_covis_set_point_attributes)";
        return RUMI_E_INVALID;
    }
    return newpts_write_out(s, n_neigh, out, cap, n_out, per_neigh_out, neigh_skipped_out);
}

extern "C" int rumi_newpts_stage_ms(const RumiMatcher *m, float *out3) {
    if (!out3 || !newpts_peek(m)) { g_lastError = "rumi_newpts_stage_ms: no CreateNewMapPoints call precedes on this matcher"; return RUMI_E_INVALID; }
    std::memcpy(out3, newpts_peek(m)->stageMs, 12);
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
    hipLaunchKernelGGL(k_newpts_replay<BlockView>, dim3(1), dim3(1024), 0, nullptr, BlockView{s->blk.d}, n_neigh, s->lastOri, s->cand.p, s->gate.p, s->x3D.p, reinterpret_cast<NewPtsResult *>(s->res.d), s->matched.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(matches, s->matched.p, pairs * 4, hipMemcpyDeviceToHost));
    return RUMI_OK;
}

#include "search_in_neighbors.inc"
#include "search_and_fuse.inc"
#include "sim3_projection_batch.inc"
#include "common_regions_resident.inc"
