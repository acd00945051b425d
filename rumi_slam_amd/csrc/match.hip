// MI355X-native Hamming matchers behind include/rumi_match.h (kernels + host side).
//
// The reference walks map points / key-frame features one after another and lets each one see the
// assignments of the ones before it (ORBmatcher.cc:80-82, :248-249, :1556-1558).  GPU formulation, exact:
//   1. k_grid        Frame::AssignFeaturesToGrid as a key sort: (cell << 16 | feature) ascending, cell = ix*48+iy, so
//                    the cells GetFeaturesInArea visits for one ix are one contiguous range, already in its order.
//   2. k_queries_*   one query per map point / last-frame feature / key-frame feature (projection, window, levels).
//   3. k_candidates  one wave per query: enumerate candidates in the reference's order, 256-bit Hamming by
//                    xor + popcount, ballot-compacted into a per-query list (count pass, scan, fill pass).
//   4. k_resolve     one workgroup: every query picks its best candidate given "feature f is taken by an earlier
//                    query" (blockedFrom[f] = smallest blocking query index); iterate to the fix point.  After
//                    round k queries 0..k-1 hold their sequential result, and a fix point is the sequential result
//                    (induction on the query index), so the outcome equals the reference's loop bit for bit.
//                    Then the rotation histogram / ComputeThreeMaxima filter and the result arrays.
//   k_bruteforce_mfma  all-pairs best / second-best as an FP4 GEMM on the matrix cores.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "match_host.h"

namespace rumi {

constexpr int kMaxSortN = 16384;     // features per frame: the mono-initialisation extractor asks for 5 x nfeatures (Tracking.cc:581: 10 000 with TUM3.yaml)

// ---- 1. grid -----------------------------------------------------------------------------------------------
// Frame::AssignFeaturesToGrid as a counting sort by cell (cell = column-major ix*48+iy, the order GetFeaturesInArea walks),
// ascending key-point index inside a cell (= push_back order).  One workgroup; the per-cell segments (a handful of entries) are
// put in index order by an insertion sort after an unordered atomic placement.
// (nDev: the feature count where the extractor left it, when the host has not read it yet; n is then its upper bound)
__global__ __launch_bounds__(1024) void k_grid(int n, const RumiKeyPoint *__restrict__ keys, float minX, float minY, float wInv,
                                               float hInv, uint16_t *__restrict__ sortedIdx, int32_t *__restrict__ cellStart, const int32_t *__restrict__ nDev) {
    if (nDev) n = min(n, *nDev);
    __shared__ int32_t sCnt[kGridCells + 1];
    __shared__ uint16_t sCell[kMaxSortN], sOut[kMaxSortN];
    __shared__ int32_t sWave[16];
    const int tid = threadIdx.x;
    for (int c = tid; c <= kGridCells; c += 1024) sCnt[c] = 0;
    __syncthreads();
    for (int i = tid; i < n; i += 1024) {
        // Frame::PosInGrid: round() of the float expression, dropped when outside the grid
        const int px = (int)__builtin_roundf((keys[i].x - minX) * wInv);
        const int py = (int)__builtin_roundf((keys[i].y - minY) * hInv);
        uint16_t cell = 0xFFFF;
        if (px >= 0 && px < kGridCols && py >= 0 && py < kGridRows) { cell = (uint16_t)(px * kGridRows + py); atomicAdd(&sCnt[cell], 1); }
        sCell[i] = cell;
    }
    __syncthreads();
    // exclusive scan of the 3072 counts: 3 cells per thread, a DPP scan inside each wave, the 16 wave totals through LDS (one barrier)
    constexpr int kPer = (kGridCells + 1023) / 1024;
    int loc[kPer], sum = 0;
#pragma unroll
    for (int k = 0; k < kPer; k++) { const int c = tid * kPer + k; loc[k] = c < kGridCells ? sCnt[c] : 0; sum += loc[k]; }
    const int incl = wave_scan_incl_i32(sum);
    if ((tid & 63) == 63) sWave[tid >> 6] = incl;
    __syncthreads();
    int before = 0, total = 0;
#pragma unroll
    for (int w = 0; w < 16; w++) { const int t = sWave[w]; total += t; if (w < (tid >> 6)) before += t; }
    int run = before + incl - sum;
#pragma unroll
    for (int k = 0; k < kPer; k++) {
        const int c = tid * kPer + k;
        if (c < kGridCells) { cellStart[c] = run; sCnt[c] = run; run += loc[k]; }
    }
    if (tid == 1023) cellStart[kGridCells] = total;
    __syncthreads();
    for (int i = tid; i < n; i += 1024) {
        const uint16_t cell = sCell[i];
        if (cell != 0xFFFF) sOut[atomicAdd(&sCnt[cell], 1)] = (uint16_t)i;
    }
    __syncthreads();
    // sCnt[c] is now the END of cell c; its start is the end of cell c-1 (or 0)
#pragma unroll
    for (int k = 0; k < kPer; k++) {
        const int c = tid * kPer + k;
        if (c >= kGridCells) continue;
        const int e = sCnt[c], b0 = e - loc[k];
        for (int i = b0 + 1; i < e; i++) {
            const uint16_t v = sOut[i];
            int j = i - 1;
            while (j >= b0 && sOut[j] > v) { sOut[j + 1] = sOut[j]; j--; }
            sOut[j + 1] = v;
        }
    }
    __syncthreads();
    for (int i = tid; i < total; i += 1024) sortedIdx[i] = sOut[i];
}

// ---- 2. queries ----------------------------------------------------------------------------------------------
__global__ void k_queries_mappoints(int nmp, const uint8_t *trackInView, const float *projX, const float *projY,
                                    const int32_t *scaleLevel, const float *viewCos, const float *trackDepth,
                                    const uint8_t *isBad, const int32_t *mpObs, const float *scaleFactors, float th,
                                    int farPoints, float thFar, Query *q) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nmp) return;
    q[i] = mappoint_query(i, trackInView[i] != 0, projX[i], projY[i], scaleLevel[i], viewCos[i], trackDepth[i], isBad[i] != 0, mpObs[i], scaleFactors, th, farPoints, thFar);
}

// SearchByProjection(Cur, Last): ORBmatcher.cc:1516-1551 (mono: levels nLastOctave-1 .. nLastOctave+1)
__global__ void k_queries_frame(int nlast, const RumiKeyPoint *lastKeys, const int32_t *lastMp, const uint8_t *lastOutlier,
                                const float *mpPos, const int32_t *mpObs, const float *Tcw, const float *K,
                                const float *scaleFactors, float th, float minX, float minY, float maxX, float maxY,
                                Query *q) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nlast) return;
    Query o{};
    const int mp = lastMp[i];
    if (mp >= 0 && !lastOutlier[i]) {
        // Sophus::SE3f * p: p + w*uv + q.vec x uv, uv = 2 (q.vec x p); then + t   (so3.hpp:358-367)
        const float qx = Tcw[0], qy = Tcw[1], qz = Tcw[2], qw = Tcw[3];
        const float p0 = mpPos[mp * 3], p1 = mpPos[mp * 3 + 1], p2 = mpPos[mp * 3 + 2];
        float u0 = qy * p2 - qz * p1, u1 = qz * p0 - qx * p2, u2 = qx * p1 - qy * p0;
        u0 += u0; u1 += u1; u2 += u2;
        const float c0 = qy * u2 - qz * u1, c1 = qz * u0 - qx * u2, c2 = qx * u1 - qy * u0;
        const float xc = ((p0 + qw * u0) + c0) + Tcw[4], yc = ((p1 + qw * u1) + c1) + Tcw[5], zc = ((p2 + qw * u2) + c2) + Tcw[6];
        const float invzc = (float)(1.0 / (double)zc);
        if (!(invzc < 0)) {
            const float u = K[0] * xc / zc + K[2], v = K[1] * yc / zc + K[3];      // Pinhole::project
            if (!(u < minX || u > maxX) && !(v < minY || v > maxY)) {
                const int oct = lastKeys[i].octave;
                o.valid = 1; o.u = u; o.v = v; o.r = th * scaleFactors[oct];
                o.minLevel = oct - 1; o.maxLevel = oct + 1;
            }
        }
        o.descId = mp; o.mpId = mp; o.blocks = mpObs[mp] > 0;
    }
    o.angle = lastKeys[i].angle;
    q[i] = o;
}

// SearchByBoW: one query per entry of the key-frame's FeatureVector, in (node, entry) order (ORBmatcher.cc:217-232).  One THREAD per entry
// (it finds its node by bisection of the offsets, then the node's twin in the frame's vector by bisection of the ids): a vocabulary level with
// few nodes -- levelsup near L, small trees -- used to leave the work to a handful of threads walking a hundred entries each (84 us at 10 nodes).
__global__ void k_queries_bow(int nnKF, const uint32_t *kfNodes, const int32_t *kfOff, const uint32_t *kfIdx,
                              const int32_t *kfMp, const uint8_t *mpBad, const RumiKeyPoint *kfKeys, int nnF,
                              const uint32_t *fNodes, const int32_t *fOff, Query *q, const int32_t *nnFdev) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (nnKF <= 0 || p >= kfOff[nnKF]) return;
    if (nnFdev) nnF = *nnFdev;                              // the frame's FeatureVector was built on the device (k_fv_build)
    int a = 0, ahi = nnKF;                                  // the node that holds entry p: last a with kfOff[a] <= p
    while (ahi - a > 1) { const int mid = (a + ahi) >> 1; if (kfOff[mid] <= p) a = mid; else ahi = mid; }
    // the merge-walk of the two ordered maps visits exactly the node ids present in both
    int lo = 0, hi = nnF;
    const uint32_t id = kfNodes[a];
    while (lo < hi) { const int mid = (lo + hi) >> 1; if (fNodes[mid] < id) lo = mid + 1; else hi = mid; }
    const bool hit = lo < nnF && fNodes[lo] == id;
    Query o{};
    const int feat = (int)kfIdx[p];
    const int mp = kfMp[feat];
    o.valid = hit && mp >= 0 && !mpBad[mp];
    o.descId = feat; o.mpId = mp; o.blocks = 1;
    if (o.valid) { o.c0 = fOff[lo]; o.c1 = fOff[lo + 1]; }
    o.angle = kfKeys[feat].angle;
    q[p] = o;
}

__device__ __forceinline__ void se3f_mul(const float *T, const float *p, float *o) {   // Sophus::SE3f * p (so3.hpp:358-367)
    const float qx = T[0], qy = T[1], qz = T[2], qw = T[3];
    float u0 = qy * p[2] - qz * p[1], u1 = qz * p[0] - qx * p[2], u2 = qx * p[1] - qy * p[0];
    u0 += u0; u1 += u1; u2 += u2;
    const float c0 = qy * u2 - qz * u1, c1 = qz * u0 - qx * u2, c2 = qx * u1 - qy * u0;
    o[0] = ((p[0] + qw * u0) + c0) + T[4]; o[1] = ((p[1] + qw * u1) + c1) + T[5]; o[2] = ((p[2] + qw * u2) + c2) + T[6];
}

// SearchByProjection(KeyFrame*, Sim3f&, points, ...): ORBmatcher.cc:389-436 (variant 0) / :491-539 (variant 1)
__global__ void k_queries_sim3(int nmp, const uint8_t *skip, const float *mpPos, const float *mpNormal, const float *mpMinDist,
                               const float *mpMaxDist, const float *pose /*Tcw7, K4, Ow3*/, const float *scaleFactors, int nLevels,
                               float logScaleFactor, float th, int variant, int blocks, int checkReproj, float minX, float minY, float maxX, float maxY,
                               Query *q) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nmp) return;
    Query o{};
    o.descId = i; o.mpId = i; o.blocks = blocks; o.c0 = checkReproj;
    const float *Tcw = pose, *K = pose + 7, *Ow = pose + 11;
    if (!skip[i]) {
        const float *p3Dw = mpPos + (size_t)i * 3;
        float pc[3];
        se3f_mul(Tcw, p3Dw, pc);
        if (!(pc[2] < 0.0f)) {
            float u, v;
            if (variant == 0) { u = K[0] * pc[0] / pc[2] + K[2]; v = K[1] * pc[1] / pc[2] + K[3]; }
            else { const float invz = 1 / pc[2]; const float x = pc[0] * invz, y = pc[1] * invz; u = K[0] * x + K[2]; v = K[1] * y + K[3]; }
            if (u >= minX && u < maxX && v >= minY && v < maxY) {                       // KeyFrame::IsInImage
                const float maxD = 1.2f * mpMaxDist[i], minD = 0.8f * mpMinDist[i];
                const float P0 = p3Dw[0] - Ow[0], P1 = p3Dw[1] - Ow[1], P2 = p3Dw[2] - Ow[2];
                const float dist = sqrtf((P0 * P0 + P1 * P1) + P2 * P2);
                const float *Pn = mpNormal + (size_t)i * 3;
                if (!(dist < minD || dist > maxD) && !((double)((P0 * Pn[0] + P1 * Pn[1]) + P2 * Pn[2]) < 0.5 * (double)dist)) {
                    const int lvl = predict_scale(mpMaxDist[i], dist, logScaleFactor, nLevels);
                    o.valid = 1; o.u = u; o.v = v; o.r = th * scaleFactors[lvl];
                    o.minLevel = lvl - 1; o.maxLevel = lvl;                              // the level test of :445-448 / :553-556
                }
            }
        }
    }
    q[i] = o;
}

// SearchBySim3, one direction (ORBmatcher.cc:1329-1371 / :1405-1447): points already in the target camera frame
__global__ void k_queries_campoints(int n, const uint8_t *skip, const float *pc, const float *mpMinDist, const float *mpMaxDist, const float *K,
                                    const float *scaleFactors, int nLevels, float logScaleFactor, float th, float minX, float minY, float maxX,
                                    float maxY, Query *q) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    Query o{};
    o.descId = i; o.mpId = i;
    if (!skip[i]) {
        const float *p = pc + (size_t)i * 3;
        if (!((double)p[2] < 0.0)) {
            const float invz = (float)(1.0 / (double)p[2]);
            const float x = p[0] * invz, y = p[1] * invz;
            const float u = K[0] * x + K[2], v = K[1] * y + K[3];
            if (u >= minX && u < maxX && v >= minY && v < maxY) {                       // KeyFrame::IsInImage
                const float maxD = 1.2f * mpMaxDist[i], minD = 0.8f * mpMinDist[i];
                const float dist = sqrtf((p[0] * p[0] + p[1] * p[1]) + p[2] * p[2]);
                if (!(dist < minD || dist > maxD)) {
                    const int lvl = predict_scale(mpMaxDist[i], dist, logScaleFactor, nLevels);
                    o.valid = 1; o.u = u; o.v = v; o.r = th * scaleFactors[lvl];
                    o.minLevel = lvl - 1; o.maxLevel = lvl;
                }
            }
        }
    }
    q[i] = o;
}

// SearchByProjection(Frame&, KeyFrame*, sAlreadyFound, th, ORBdist): ORBmatcher.cc:1700-1733
__global__ void k_queries_reloc(int nkf, const RumiKeyPoint *kfKeys, const int32_t *kfMp, const uint8_t *skip, const float *mpPos,
                                const float *mpMinDist, const float *mpMaxDist, const float *pose, const float *scaleFactors, int nLevels,
                                float logScaleFactor, float th, float minX, float minY, float maxX, float maxY, Query *q) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nkf) return;
    Query o{};
    const int mp = kfMp[i];
    const float *Tcw = pose, *K = pose + 7, *Ow = pose + 11;
    if (mp >= 0 && !skip[mp]) {
        const float *xw = mpPos + (size_t)mp * 3;
        float pc[3];
        se3f_mul(Tcw, xw, pc);
        const float u = K[0] * pc[0] / pc[2] + K[2], v = K[1] * pc[1] / pc[2] + K[3];
        if (!(u < minX || u > maxX) && !(v < minY || v > maxY)) {
            const float P0 = xw[0] - Ow[0], P1 = xw[1] - Ow[1], P2 = xw[2] - Ow[2];
            const float dist3D = sqrtf((P0 * P0 + P1 * P1) + P2 * P2);
            const float maxD = 1.2f * mpMaxDist[mp], minD = 0.8f * mpMinDist[mp];
            if (!(dist3D < minD || dist3D > maxD)) {
                const int lvl = predict_scale(mpMaxDist[mp], dist3D, logScaleFactor, nLevels);
                o.valid = 1; o.u = u; o.v = v; o.r = th * scaleFactors[lvl];
                o.minLevel = lvl - 1; o.maxLevel = lvl + 1;
            }
        }
        o.descId = mp; o.mpId = mp; o.blocks = 1;
    }
    o.angle = kfKeys[i].angle;
    q[i] = o;
}

// SearchForInitialization: level-0 key-points of F1, window around vbPrevMatched (ORBmatcher.cc:593-602)
__global__ void k_queries_init(int n1, const RumiKeyPoint *keys1, const float *prevMatched, float windowSize, Query *q) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n1) return;
    Query o{};
    o.valid = !(keys1[i].octave > 0);
    o.u = prevMatched[2 * i]; o.v = prevMatched[2 * i + 1]; o.r = windowSize;
    o.minLevel = 0; o.maxLevel = 0;
    o.descId = i; o.mpId = i; o.angle = keys1[i].angle;
    q[i] = o;
}

// Frame::isInFrustum (Frame.cc:558-617, mono): one lane per map point
__global__ void k_is_in_frustum(int nmp, const float *pose /*Rcw9 tcw3 Ow3 K4*/, float minX, float minY, float maxX, float maxY,
                                float logScaleFactor, int nLevels, float viewingCosLimit, const float *mpPos, const float *mpNormal,
                                const float *mpMinDist, const float *mpMaxDist, uint8_t *inView, float *projX, float *projY,
                                int32_t *scaleLevel, float *viewCosOut, float *trackDepth, const uint8_t *skip = nullptr) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nmp) return;
    if (skip && skip[i]) {                                // SearchLocalPoints does not evaluate these (already matched in this frame / bad)
        inView[i] = 0; projX[i] = -1; projY[i] = -1; scaleLevel[i] = 0; viewCosOut[i] = 0; trackDepth[i] = 0;
        return;
    }
    const float *R = pose, *t = pose + 9, *Ow = pose + 12, *K = pose + 15;
    const float *P = mpPos + (size_t)i * 3;
    uint8_t in = 0;
    float px = -1, py = -1, vc = 0, depth = 0;
    int lvl = 0;
    float Pc[3];
#pragma unroll
    for (int r = 0; r < 3; r++) Pc[r] = ((R[r * 3] * P[0] + R[r * 3 + 1] * P[1]) + R[r * 3 + 2] * P[2]) + t[r];
    const float Pc_dist = sqrtf((Pc[0] * Pc[0] + Pc[1] * Pc[1]) + Pc[2] * Pc[2]);
    if (!(Pc[2] < 0.0f)) {
        const float u = K[0] * Pc[0] / Pc[2] + K[2], v = K[1] * Pc[1] / Pc[2] + K[3];
        if (!(u < minX || u > maxX) && !(v < minY || v > maxY)) {
            px = u; py = v;
            const float maxD = 1.2f * mpMaxDist[i], minD = 0.8f * mpMinDist[i];
            const float P0 = P[0] - Ow[0], P1 = P[1] - Ow[1], P2 = P[2] - Ow[2];
            const float dist = sqrtf((P0 * P0 + P1 * P1) + P2 * P2);
            if (!(dist < minD || dist > maxD)) {
                const float *Pn = mpNormal + (size_t)i * 3;
                const float viewCos = ((P0 * Pn[0] + P1 * Pn[1]) + P2 * Pn[2]) / dist;
                if (!(viewCos < viewingCosLimit)) {
                    lvl = predict_scale(mpMaxDist[i], dist, logScaleFactor, nLevels);
                    in = 1; depth = Pc_dist; vc = viewCos;
                }
            }
        }
    }
    inView[i] = in; projX[i] = px; projY[i] = py; scaleLevel[i] = lvl; viewCosOut[i] = vc; trackDepth[i] = depth;
}

// ---- uploads: one pinned block per call, scattered to the arrays on the device ---------------------------------------------
__global__ __launch_bounds__(256) void k_scatter(const uint8_t *__restrict__ mirror, int nseg) {
    const Segment sg = reinterpret_cast<const Segment *>(mirror)[blockIdx.y];
    if ((int)blockIdx.y >= nseg) return;
    const uint32_t words = sg.bytes >> 2;
    const uint32_t *src = reinterpret_cast<const uint32_t *>(mirror + sg.off);
    uint32_t *dst = reinterpret_cast<uint32_t *>(sg.dst);
    for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < words; i += gridDim.x * 256) dst[i] = src[i];
    if (blockIdx.x == 0 && threadIdx.x < (sg.bytes & 3)) {
        const uint32_t k = (words << 2) + threadIdx.x;
        reinterpret_cast<uint8_t *>(sg.dst)[k] = mirror[sg.off + k];
    }
}

// ---- 3. candidates: one wave per query -----------------------------------------------------------------------------
// list entry: feature (16 bit) | distance (9 bit) << 16 | octave (4 bit) << 25
// Lists of up to kSortMax entries are stored SORTED by (distance, position in the reference's candidate order): the
// reference's "best / second best among the candidates not yet taken" is then simply the first / second not-taken entry
// (strict `<` keeps the earliest of equal distances, and a displaced best becomes the second), so a resolve round reads a
// couple of entries per query instead of the whole list.  Longer lists stay in candidate order and are scanned in full.
constexpr int kSortMax = 1024;
__device__ __forceinline__ void wave_lds_fence() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

template <int PASS> __device__ __forceinline__ int offsets_of(const int32_t *offsets, int qi, int listCap) { return PASS == 2 ? qi * listCap : offsets[qi]; }

// The candidates of one query, walked by one wave: FILL = false counts them, FILL = true computes their Hamming distances and stores them (into the
// wave's LDS sort arrays when they fit, else straight to `out`).  Returns the count.
template <bool FILL>
__device__ __forceinline__ int candidates_walk(int mode, const Query &Q, const FrameDev &F, const uint32_t (&qd)[8], const uint32_t *__restrict__ fvIdx, bool sorted,
                                               uint32_t *out, uint32_t *key, uint32_t *val, int lane) {
    int count = 0;
    if (mode == MODE_BOW || mode == MODE_BOW_KF) {
        for (int p = Q.c0 + lane; p - lane < Q.c1; p += 64) {
            const bool ok = p < Q.c1;
            if (FILL && ok) {
                const int idx = (int)fvIdx[p];
                const int d = hamming256(qd, reinterpret_cast<const uint32_t *>(F.desc + (size_t)idx * 32));
                const uint32_t e = (uint32_t)idx | ((uint32_t)d << 16);
                if (sorted) { key[p - Q.c0] = ((uint32_t)d << 10) | (uint32_t)(p - Q.c0); val[p - Q.c0] = e; }
                else out[p - Q.c0] = e;
            }
        }
        return Q.c1 - Q.c0;
    }
    // Frame::GetFeaturesInArea (Frame.cc:695-750)
    const int nMinCellX = max(0, (int)floorf((Q.u - F.minX - Q.r) * F.wInv));
    const int nMaxCellX = min(kGridCols - 1, (int)ceilf((Q.u - F.minX + Q.r) * F.wInv));
    const int nMinCellY = max(0, (int)floorf((Q.v - F.minY - Q.r) * F.hInv));
    const int nMaxCellY = min(kGridRows - 1, (int)ceilf((Q.v - F.minY + Q.r) * F.hInv));
    if (nMinCellX < kGridCols && nMaxCellX >= 0 && nMinCellY < kGridRows && nMaxCellY >= 0) {
        const bool checkLevels = Q.minLevel > 0 || Q.maxLevel >= 0;
        for (int ix = nMinCellX; ix <= nMaxCellX; ix++) {
            const int p0 = F.cellStart[ix * kGridRows + nMinCellY], p1 = F.cellStart[ix * kGridRows + nMaxCellY + 1];
            for (int base = p0; base < p1; base += 64) {
                const int p = base + lane;
                bool pass = false;
                int idx = 0, oct = 0;
                if (p < p1) {
                    idx = F.sortedIdx[p];
                    const RumiKeyPoint kp = F.keys[idx];
                    oct = kp.octave;
                    pass = true;
                    if (checkLevels) {
                        if (oct < Q.minLevel) pass = false;
                        if (Q.maxLevel >= 0 && oct > Q.maxLevel) pass = false;
                    }
                    const float dx = kp.x - Q.u, dy = kp.y - Q.v;
                    if (!(fabsf(dx) < Q.r && fabsf(dy) < Q.r)) pass = false;
                    if (mode == MODE_FUSE && Q.c0 && pass) {                        // mono reprojection gate, ORBmatcher.cc:1138-1145
                        const float ex = Q.u - kp.x, ey = Q.v - kp.y;
                        const float e2 = ex * ex + ey * ey;
                        const float s2 = F.scale[oct] * F.scale[oct];              // mvLevelSigma2; mvInvLevelSigma2 = 1.0f / it
                        if ((double)(e2 * (1.0f / s2)) > 5.99) pass = false;
                    }
                }
                const unsigned long long b = __ballot(pass);
                if (FILL && pass) {
                    const int d = hamming256(qd, reinterpret_cast<const uint32_t *>(F.desc + (size_t)idx * 32));
                    const int pos = count + __popcll(b & ((1ull << lane) - 1ull));
                    const uint32_t e = (uint32_t)idx | ((uint32_t)d << 16) | ((uint32_t)(oct & 15) << 25);
                    if (sorted) { key[pos] = ((uint32_t)d << 10) | (uint32_t)pos; val[pos] = e; }
                    else out[pos] = e;
                }
                count += __popcll(b);
            }
        }
    }
    return count;
}

// bitonic sort of one wave's (key, val) pairs in LDS by key, then the values to `out`
__device__ __forceinline__ void wave_bitonic_store(uint32_t *key, uint32_t *val, int total, uint32_t *out, int lane) {
    int m = 1;
    while (m < total) m <<= 1;
    for (int i = total + lane; i < m; i += 64) key[i] = 0xFFFFFFFFu;
    wave_lds_fence();
    for (int k = 2; k <= m; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = lane; t < (m >> 1); t += 64) {
                const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i | j;
                const uint32_t a = key[i], b = key[l];
                if ((a > b) == ((i & k) == 0)) {
                    key[i] = b; key[l] = a;
                    const uint32_t va = val[i]; val[i] = val[l]; val[l] = va;
                }
            }
            wave_lds_fence();
        }
    for (int i = lane; i < total; i += 64) out[i] = val[i];
}

// PASS 0: count pass (counts[q]).  PASS 1: fill pass at the offsets a scan of the counts produced.  PASS 2: both in one launch, every query's list
// in a fixed slot of `listCap` entries (offsets[q] = q * listCap written here): two dispatches (~4.5 us each) less per search; a query with more
// candidates than a slot raises kFusedOverflow and the host repeats the search with passes 0 / scan / 1.
template <int PASS>
__global__ __launch_bounds__(256) void k_candidates(int mode, int nq, const Query *__restrict__ q, FrameDev F,
                                                    const uint8_t *__restrict__ qDesc, const uint32_t *__restrict__ fvIdx,
                                                    int32_t *__restrict__ counts, int32_t *__restrict__ offsets,
                                                    uint32_t *__restrict__ lists, int listCap, int32_t *__restrict__ overflow) {
    constexpr bool FILL = PASS != 0;
    __shared__ uint32_t sKey[FILL ? 4 * kSortMax : 1], sVal[FILL ? 4 * kSortMax : 1];
    const int lane = threadIdx.x & 63;
    const int qi = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (qi >= nq) return;
    if (PASS == 1 && offsets[nq] > listCap) {            // the arena cannot hold this call's lists: report the need, write nothing
        if (qi == 0 && lane == 0) *overflow = offsets[nq];
        return;
    }
    const Query Q = q[qi];
    if (PASS == 2 && lane == 0) offsets[qi] = qi * listCap;
    if (!Q.valid) {
        if (PASS != 1 && lane == 0) counts[qi] = 0;
        return;
    }
    uint32_t *key = sKey + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6) * kSortMax, *val = sVal + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6) * kSortMax;
    uint32_t qd[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    int total = 0;
    if (PASS == 2 && mode != MODE_BOW && mode != MODE_BOW_KF) {
        // The usual search of the Tracking thread (a window of a few grid columns, a handful of candidates) as ONE dependent chain
        // instead of two walks of four loads per column: the cell ranges of all columns at once (one lane each), the window's
        // feature slots flat over the lanes (slot -> column by the prefix of the range lengths: the reference's candidate order),
        // key-point and descriptor of every slot fetched together, and up to 64 candidates ranked in registers.
        const int nMinCellX = max(0, (int)floorf((Q.u - F.minX - Q.r) * F.wInv));
        const int nMaxCellX = min(kGridCols - 1, (int)ceilf((Q.u - F.minX + Q.r) * F.wInv));
        const int nMinCellY = max(0, (int)floorf((Q.v - F.minY - Q.r) * F.hInv));
        const int nMaxCellY = min(kGridRows - 1, (int)ceilf((Q.v - F.minY + Q.r) * F.hInv));
        int ncol = 0;
        if (nMinCellX < kGridCols && nMaxCellX >= 0 && nMinCellY < kGridRows && nMaxCellY >= 0 && nMaxCellY >= nMinCellY) ncol = max(0, nMaxCellX - nMinCellX + 1);
        int c0 = 0, len = 0;
        if (lane < ncol) {
            const int cell = (nMinCellX + lane) * kGridRows;
            c0 = F.cellStart[cell + nMinCellY];
            len = F.cellStart[cell + nMaxCellY + 1] - c0;
        }
        const uint32_t qmine = reinterpret_cast<const uint32_t *>(qDesc + (size_t)Q.descId * 32)[lane & 7];
        const int incl = wave_scan_incl_i32(len);
        const int T = __builtin_amdgcn_readlane(incl, 63);
        if (T <= kSortMax) {
#pragma unroll
            for (int k = 0; k < 8; k++) qd[k] = __shfl(qmine, k);
            const bool checkLevels = Q.minLevel > 0 || Q.maxLevel >= 0;
            uint32_t *out = lists + qi * listCap;
            int count = 0;
            uint32_t myKey = 0xFFFFFFFFu, myVal = 0;
            unsigned long long b = 0;
            for (int base = 0; base < T; base += 64) {
                const int sl = base + lane;
                const bool live = sl < T;
                int col = 0;
                for (int c = 0; c < ncol; c++) col += __builtin_amdgcn_readlane(incl, c) <= sl;
                const int cc = live ? col : 0;
                const int p = __shfl(c0, cc) + (sl - (__shfl(incl, cc) - __shfl(len, cc)));
                bool pass = false;
                int idx = 0, oct = 0, d = 0;
                if (live) {
                    idx = F.sortedIdx[p];
                    const RumiKeyPoint kp = F.keys[idx];
                    const uint4 *dp = reinterpret_cast<const uint4 *>(F.desc + (size_t)idx * 32);
                    const uint4 d0 = dp[0], d1 = dp[1];
                    oct = kp.octave;
                    pass = true;
                    if (checkLevels) {
                        if (oct < Q.minLevel) pass = false;
                        if (Q.maxLevel >= 0 && oct > Q.maxLevel) pass = false;
                    }
                    const float dx = kp.x - Q.u, dy = kp.y - Q.v;
                    if (!(fabsf(dx) < Q.r && fabsf(dy) < Q.r)) pass = false;
                    if (mode == MODE_FUSE && Q.c0 && pass) {                        // mono reprojection gate, ORBmatcher.cc:1138-1145
                        const float ex = Q.u - kp.x, ey = Q.v - kp.y;
                        const float e2 = ex * ex + ey * ey;
                        const float s2 = F.scale[oct] * F.scale[oct];              // mvLevelSigma2; mvInvLevelSigma2 = 1.0f / it
                        if ((double)(e2 * (1.0f / s2)) > 5.99) pass = false;
                    }
                    d = __popc(qd[0] ^ d0.x) + __popc(qd[1] ^ d0.y) + __popc(qd[2] ^ d0.z) + __popc(qd[3] ^ d0.w) +
                        __popc(qd[4] ^ d1.x) + __popc(qd[5] ^ d1.y) + __popc(qd[6] ^ d1.z) + __popc(qd[7] ^ d1.w);
                }
                b = __ballot(pass);
                if (pass) {
                    const int pos = count + __popcll(b & ((1ull << lane) - 1ull));
                    myKey = ((uint32_t)d << 10) | (uint32_t)pos;
                    myVal = (uint32_t)idx | ((uint32_t)d << 16) | ((uint32_t)(oct & 15) << 25);
                    if (T > 64) { key[pos] = myKey; val[pos] = myVal; }
                }
                count += __popcll(b);
            }
            if (lane == 0) counts[qi] = count;
            if (count > listCap) {
                if (lane == 0) atomicExch(overflow, kFusedOverflow);
                return;
            }
            if (T <= 64) {                                                  // one trip: rank among the passing lanes (keys are distinct)
                int rank = 0;
                for (unsigned long long bb = b; bb; bb &= bb - 1) {
                    const uint32_t kj = (uint32_t)__builtin_amdgcn_readlane((int)myKey, __builtin_ctzll(bb));
                    rank += kj < myKey;
                }
                if (myKey != 0xFFFFFFFFu) out[rank] = myVal;
            } else if (count > 0) {
                wave_bitonic_store(key, val, count, out, lane);
            }
            return;
        }
    }
    if (PASS == 0 || PASS == 2) {
        total = candidates_walk<false>(mode, Q, F, qd, fvIdx, false, nullptr, key, val, lane);
        if (lane == 0) counts[qi] = total;
        if (PASS == 0) return;
        if (total > listCap) {
            if (lane == 0) atomicExch(overflow, kFusedOverflow);
            return;
        }
    } else total = counts[qi];
    const bool sorted = total <= kSortMax;
    {
        const uint32_t *src = reinterpret_cast<const uint32_t *>(qDesc + (size_t)Q.descId * 32);
        const uint32_t mine = src[lane & 7];
#pragma unroll
        for (int k = 0; k < 8; k++) qd[k] = __shfl(mine, k);
    }
    uint32_t *out = lists + offsets_of<PASS>(offsets, qi, listCap);
    candidates_walk<true>(mode, Q, F, qd, fvIdx, sorted, out, key, val, lane);
    if (sorted && total > 0) wave_bitonic_store(key, val, total, out, lane);
}

// exclusive scan of counts -> offsets (single workgroup; nq is a few thousand)
__global__ __launch_bounds__(256) void k_scan(int n, const int32_t *__restrict__ counts, int32_t *__restrict__ offsets) {
    __shared__ int part[256];
    const int tid = threadIdx.x, chunk = (n + 255) / 256;
    int s = 0;
    for (int k = 0; k < chunk; k++) { const int i = tid * chunk + k; if (i < n) s += counts[i]; }
    part[tid] = s;
    __syncthreads();
    if (tid == 0) { int run = 0; for (int i = 0; i < 256; i++) { const int t = part[i]; part[i] = run; run += t; } offsets[n] = run; }
    __syncthreads();
    int run = part[tid];
    for (int k = 0; k < chunk; k++) { const int i = tid * chunk + k; if (i < n) { offsets[i] = run; run += counts[i]; } }
}

// ---- 4. resolve ------------------------------------------------------------------------------------------------
// One workgroup iterates "every query picks its best candidate among the features no EARLIER query holds" to its fixed point (the
// result of the reference's sequential loop).  A round is latency, not work: what a round needs of a query -- count, the head of its
// candidate list, the blocks flag, its current pick -- is read once into registers (the first kResQ queries of a thread, i.e. up to
// 2048 queries; the rest go through global memory as before), the initial occupancy of a thread's features is a bit mask, and a
// round is three barriers over LDS.
constexpr int kResQ = 2, kResK = 4;
__global__ __launch_bounds__(1024) void k_resolve(ResolveArgs A) {
    extern __shared__ int32_t blockedFrom[];      // [nfeat] smallest blocking query index; -1 = taken before the call
    __shared__ int sChanged[2], sHist[RUMI_HISTO_LENGTH], sKeep[RUMI_HISTO_LENGTH], sCount;
    const int tid = threadIdx.x, nt = blockDim.x;
    const int kFree = 0x7FFFFFFF;
    if (A.nq > 0 && *A.overflow != 0) return;
    // ---- read once ----
    int cCnt[kResQ], cAsg[kResQ], cBlocks[kResQ];
    const uint32_t *cList[kResQ];
    uint32_t cHead[kResQ][kResK];
#pragma unroll
    for (int j = 0; j < kResQ; j++) {
        const int i = tid + j * nt;
        cCnt[j] = 0; cAsg[j] = -1; cBlocks[j] = 0; cList[j] = A.lists;
        if (i < A.nq) { cCnt[j] = A.counts[i]; cList[j] = A.lists + A.offsets[i]; cBlocks[j] = A.q[i].blocks; }
#pragma unroll
        for (int k = 0; k < kResK; k++) cHead[j][k] = k < cCnt[j] ? cList[j][k] : 0u;
    }
    for (int i = tid + kResQ * nt; i < A.nq; i += nt) A.assign[i] = -1;
    uint64_t taken0 = 0;                                                    // bit k: feature tid + k nt is taken before the call (nfeat <= 65536: list entries carry 16 bits)
    {
        int k = 0;
        for (int f = tid; f < A.nfeat; f += nt, k++) {
            bool t = false;
            if (A.featBlocked0) t = A.featBlocked0[f] != 0;
            else if (A.mode != MODE_BOW) { const int id = A.featMp[f]; t = id >= 0 && A.mpObs[id] > 0; }
            taken0 |= (uint64_t)t << k;
            blockedFrom[f] = t ? -1 : kFree;
        }
    }
    if (tid < RUMI_HISTO_LENGTH) sHist[tid] = 0;
    if (tid < 2) sChanged[tid] = 0;
    if (tid == 0) sCount = 0;
    auto pick_of = [&](int i, int cnt, const uint32_t *L, const uint32_t *head /* kResK entries in registers, or null */) -> int {
        if (cnt <= 0) return -1;
        int bestDist = 256, bestDist2 = 256, bestLevel = -1, bestLevel2 = -1, bestIdx = -1;
        const bool sortedList = cnt <= kSortMax;                           // then entries come in (distance, candidate order)
        bool done = false;
        auto take = [&](uint32_t e) {
            const int f = (int)(e & 0xFFFF);
            if (blockedFrom[f] < i) return;                                 // taken by an earlier query (or before the call)
            const int d = (int)((e >> 16) & 0x1FF), lv = (int)((e >> 25) & 15);
            if (d < bestDist) { bestDist2 = bestDist; bestDist = d; bestLevel2 = bestLevel; bestLevel = lv; bestIdx = f; }
            else if (d < bestDist2) { bestLevel2 = lv; bestDist2 = d; done = sortedList; }
            else done = sortedList;                                         // equal to the second best: nothing later can change either
        };
        int k = 0;
        if (head) {
#pragma unroll
            for (int h = 0; h < kResK; h++) if (h < cnt && !done) take(head[h]);
            k = kResK;
        }
        for (; k < cnt && !done; k++) take(L[k]);
        int pick = -1;
        if (A.mode == MODE_MAPPOINTS) {                                     // ORBmatcher.cc:106-111
            if (bestDist <= RUMI_TH_HIGH && !(bestLevel == bestLevel2 && (float)bestDist > A.nnratio * (float)bestDist2)) pick = bestIdx;
        } else if (A.mode == MODE_FRAME) {                                  // :1577
            if (bestDist <= RUMI_TH_HIGH) pick = bestIdx;
        } else if (A.mode == MODE_BOW) {                                    // :283-285
            if (bestDist <= RUMI_TH_LOW && (float)bestDist < A.nnratio * (float)bestDist2) pick = bestIdx;
        } else if (A.mode == MODE_BOW_KF) {                                 // :753-754
            if (bestDist < RUMI_TH_LOW && (float)bestDist < A.nnratio * (float)bestDist2) pick = bestIdx;
        } else if (A.mode == MODE_SIM3) {                                   // :463 / :571
            if ((float)bestDist <= A.thrF) pick = bestIdx;
        } else if (A.mode == MODE_FUSE) {                                   // Fuse :1161 / :1277 (TH_LOW), SearchBySim3 :1399 / :1475 (TH_HIGH)
            if (bestDist <= A.thrI) pick = bestIdx;
        } else {                                                            // MODE_RELOC :1757
            if (bestDist <= A.thrI) pick = bestIdx;
        }
        return pick;
    };
    for (int round = 0; round <= A.nq + 1; round++) {
        __syncthreads();                                                    // occupancy reset (below, or the initial one above) visible
        // occupancy as the previous round's assignments imply it
#pragma unroll
        for (int j = 0; j < kResQ; j++)
            if (cAsg[j] >= 0 && cBlocks[j]) atomicMin(&blockedFrom[cAsg[j]], tid + j * nt);
        for (int i = tid + kResQ * nt; i < A.nq; i += nt) {
            const int f = A.assign[i];
            if (f >= 0 && A.q[i].blocks) atomicMin(&blockedFrom[f], i);
        }
        __syncthreads();
        int changed = 0;
#pragma unroll
        for (int j = 0; j < kResQ; j++) {
            const int i = tid + j * nt;
            if (i >= A.nq) continue;
            const int pick = pick_of(i, cCnt[j], cList[j], cHead[j]);
            if (pick != cAsg[j]) { changed = 1; cAsg[j] = pick; }
        }
        for (int i = tid + kResQ * nt; i < A.nq; i += nt) {
            const int pick = pick_of(i, A.counts[i], A.lists + A.offsets[i], nullptr);
            if (pick != A.assign[i]) { changed = 1; A.assign[i] = pick; }
        }
        if (changed) sChanged[round & 1] = 1;
        __syncthreads();
        const int any = sChanged[round & 1];
        if (tid == 0) sChanged[(round + 1) & 1] = 0;                        // last read before this round's barriers, next written after the next round's
        if (!any) break;
        int k = 0;
        for (int f = tid; f < A.nfeat; f += nt, k++) blockedFrom[f] = ((taken0 >> k) & 1) ? -1 : kFree;
    }
#pragma unroll
    for (int j = 0; j < kResQ; j++) { const int i = tid + j * nt; if (i < A.nq) A.assign[i] = cAsg[j]; }
    // results: a feature keeps the LAST query that assigned it (later assignments overwrite, as in the loop)
    int32_t *last = blockedFrom;                                        // reuse LDS: last assigning query per feature
    for (int f = tid; f < A.nfeat; f += nt) last[f] = -1;
    __syncthreads();
    const bool useHist = A.checkOri && A.mode != MODE_MAPPOINTS && A.mode != MODE_SIM3;
    int local = 0;
    auto assigned = [&](int i, int j) { return j == 0 ? cAsg[0] : j == 1 ? cAsg[1] : A.assign[i]; };
    static_assert(kResQ == 2, "assigned() spells the register copies out");
    for (int i = tid, j = 0; i < A.nq; i += nt, j++) {
        const int f = assigned(i, j);
        if (f < 0) continue;
        local++;
        atomicMax(&last[f], i);
        if (useHist) atomicAdd(&sHist[rot_bin(A.q[i].angle, A.featKeys[f].angle)], 1);
    }
    if (local) atomicAdd(&sCount, local);
    __syncthreads();
    if (tid < 64) {                                                      // ComputeThreeMaxima, ORBmatcher.cc:1795-1826, by the lanes of one wave:
        // the scan with its strict comparisons keeps the three largest counts ordered by (count descending, bin ascending); empty bins never enter
        const int s = tid < RUMI_HISTO_LENGTH ? sHist[tid] : 0;
        int keep = 1, removed = 0;
        if (useHist) {
            uint32_t key = s > 0 ? ((uint32_t)s << 6) | (uint32_t)(63 - tid) : 0u;
            const uint32_t k1 = wave_max_u32(key);
            if (key == k1) key = 0;
            const uint32_t k2 = wave_max_u32(key);
            if (key == k2) key = 0;
            const uint32_t k3 = wave_max_u32(key);
            const int max1 = (int)(k1 >> 6), max2 = (int)(k2 >> 6), max3 = (int)(k3 >> 6);
            int ind1 = k1 ? 63 - (int)(k1 & 63) : -1, ind2 = k2 ? 63 - (int)(k2 & 63) : -1, ind3 = k3 ? 63 - (int)(k3 & 63) : -1;
            if ((float)max2 < 0.1f * (float)max1) { ind2 = -1; ind3 = -1; }
            else if ((float)max3 < 0.1f * (float)max1) ind3 = -1;
            keep = (tid == ind1 || tid == ind2 || tid == ind3);
            removed = wave_sum_i32(keep ? 0 : s);
        }
        if (tid < RUMI_HISTO_LENGTH) sKeep[tid] = keep;
        if (tid == 0) *A.nmatches = sCount - removed;
    }
    __syncthreads();
    // MODE_BOW starts from an all-NULL vector (ORBmatcher.cc:201); the other modes update the frame's vector in place
    if (A.mode == MODE_BOW)
        for (int f = tid; f < A.nfeat; f += nt) A.featMp[f] = -1;
    __syncthreads();
    if (A.mode != MODE_BOW_KF)
        for (int f = tid; f < A.nfeat; f += nt)
            if (last[f] >= 0) A.featMp[f] = A.q[last[f]].mpId;
    __syncthreads();
    if (useHist)                                                        // entries of the rejected bins are set to NULL
        for (int i = tid, j = 0; i < A.nq; i += nt, j++) {
            const int f = assigned(i, j);
            if (f >= 0 && !sKeep[rot_bin(A.q[i].angle, A.featKeys[f].angle)]) {
                if (A.mode == MODE_BOW_KF) A.assign[i] = -1;           // SearchByBoW(KF,KF) reports per QUERY (vpMatches12[idx1])
                else A.featMp[f] = -1;
            }
        }
    if (A.gXw) {                                                        // (uniform) the Tracking step's next launch would be this gather
        __shared__ int sGatherWave[16], sGatherBase;
        __syncthreads();                                                // the vector is final
        gather_correspondences(A.nfeat, A.featKeys, A.featMp, A.gMpPos, A.gInvSigma2, A.gXw, A.gObs, A.gW, A.gIdx, A.gStart, A.gSnapshot, sGatherWave, &sGatherBase);
    }
}

// SearchForInitialization resolve (ORBmatcher.cc:593-679).  The skip rule `vMatchedDistance[i2] <= dist` makes every query depend
// on the best distance accepted so far for each candidate, so the queries are replayed IN ORDER by one wave; the lanes share the
// candidate list of the current query.  Called once per initialisation attempt (a few thousand queries): latency, not throughput.
struct InitArgs {
    int n1, n2;
    const Query *q;
    const int32_t *counts, *offsets;
    const uint32_t *lists;
    const RumiKeyPoint *keys2;
    int32_t *matches12;             // out [n1]
    float *prevMatched;             // in/out [n1][2]
    int32_t *nmatches;
    float nnratio;
    int checkOri;
    const int32_t *overflow;
};

__global__ __launch_bounds__(64) void k_resolve_init(InitArgs A) {
    extern __shared__ int32_t sInit[];          // matchedDist[n2] | matches21[n2]
    __shared__ int sHist[RUMI_HISTO_LENGTH], sKeep[RUMI_HISTO_LENGTH];
    int32_t *matchedDist = sInit, *matches21 = sInit + A.n2;
    const int lane = threadIdx.x;
    const int kInf = 0x7FFFFFFF;
    if (*A.overflow != 0) return;
    for (int f = lane; f < A.n2; f += 64) { matchedDist[f] = kInf; matches21[f] = -1; }
    for (int i = lane; i < A.n1; i += 64) A.matches12[i] = -1;
    if (lane < RUMI_HISTO_LENGTH) sHist[lane] = 0;
    __syncthreads();
    int nmatches = 0;
    for (int i1 = 0; i1 < A.n1; i1++) {
        const int cnt = A.counts[i1];
        if (cnt == 0) continue;
        const uint32_t *L = A.lists + A.offsets[i1];
        int b1 = kInf, b2 = kInf, bKey = kInf;            // best, second-best distance; best as dist<<16 | list position
        int bFeat = -1;
        for (int k = lane; k < cnt; k += 64) {
            const uint32_t e = L[k];
            const int f = (int)(e & 0xFFFF), d = (int)((e >> 16) & 0x1FF);
            if (matchedDist[f] <= d) continue;                            // :617
            if (d < b1) { b2 = b1; b1 = d; bKey = (d << 16) | k; bFeat = f; }
            else if (d < b2) b2 = d;
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const int c1 = __shfl_xor(b1, o), c2 = __shfl_xor(b2, o), cKey = __shfl_xor(bKey, o), cFeat = __shfl_xor(bFeat, o);
            b2 = min(max(b1, c1), min(b2, c2));
            b1 = min(b1, c1);
            if (cKey < bKey) { bKey = cKey; bFeat = cFeat; }
        }
        // :629-638 (uniform across the wave)
        if (b1 <= RUMI_TH_LOW && (float)b1 < (float)b2 * A.nnratio) {
            if (lane == 0) {
                const int prev = matches21[bFeat];
                if (prev >= 0) A.matches12[prev] = -1;
                A.matches12[i1] = bFeat;
                matches21[bFeat] = i1;
                matchedDist[bFeat] = b1;
                if (A.checkOri) sHist[rot_bin(A.q[i1].angle, A.keys2[bFeat].angle)]++;
            }
            __syncthreads();
        }
    }
    __syncthreads();
    if (lane == 0) {
        for (int i = 0; i < RUMI_HISTO_LENGTH; i++) sKeep[i] = 1;
        if (A.checkOri) {                                                   // ComputeThreeMaxima over ALL accepted (also stolen) entries
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
    }
    __syncthreads();
    // a surviving match keeps the bin it was accepted with (its feature never changes afterwards): :661-677
    for (int i = lane; i < A.n1; i += 64) {
        int f = A.matches12[i];
        if (f >= 0 && A.checkOri && !sKeep[rot_bin(A.q[i].angle, A.keys2[f].angle)]) { A.matches12[i] = -1; f = -1; }
        if (f >= 0) { nmatches++; A.prevMatched[2 * i] = A.keys2[f].x; A.prevMatched[2 * i + 1] = A.keys2[f].y; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) nmatches += __shfl_xor(nmatches, o);
    if (lane == 0) *A.nmatches = nmatches;
}

// SearchForTriangulation, monocular branch (ORBmatcher.cc:806-1013).  vbMatched2 is never set in the reference, so the queries
// are independent: per KF1 feature without a map point, the LAST candidate of minimal distance (<= TH_LOW, `dist > bestDist`
// rejects, so ties move to the later one) among those passing the epipole and epipolar tests.  One thread per node of KF1.
struct TriArgs {
    int nn1, nn2;
    const uint32_t *nodes1; const int32_t *off1; const uint32_t *idx1;
    const uint32_t *nodes2; const int32_t *off2; const uint32_t *idx2;
    const RumiKeyPoint *keys1, *keys2;
    const uint8_t *desc1, *desc2;
    const int32_t *mp1, *mp2;
    const float *scale2;            // KF2 mvScaleFactors
    const float *geom;              // F12 row-major [9], epipole [2]
    int coarse;
    int32_t *assign;                // [entries of fv1] chosen KF2 feature or -1
};

__global__ void k_tri_match(TriArgs A) {
    const int a = blockIdx.x * blockDim.x + threadIdx.x;
    if (a >= A.nn1) return;
    int lo = 0, hi = A.nn2;
    const uint32_t id = A.nodes1[a];
    while (lo < hi) { const int mid = (lo + hi) >> 1; if (A.nodes2[mid] < id) lo = mid + 1; else hi = mid; }
    const bool hit = lo < A.nn2 && A.nodes2[lo] == id;
    const float *F = A.geom;
    const float epx = A.geom[9], epy = A.geom[10];
    for (int p = A.off1[a]; p < A.off1[a + 1]; p++) {
        int best = -1;
        const int i1 = (int)A.idx1[p];
        if (hit && A.mp1[i1] < 0) {
            const RumiKeyPoint k1 = A.keys1[i1];
            uint32_t d1[8];
#pragma unroll
            for (int k = 0; k < 8; k++) d1[k] = reinterpret_cast<const uint32_t *>(A.desc1 + (size_t)i1 * 32)[k];
            // epipolar line l = x1' F12 (Pinhole.cpp:114-117)
            const float la = k1.x * F[0] + k1.y * F[3] + F[6];
            const float lb = k1.x * F[1] + k1.y * F[4] + F[7];
            const float lc = k1.x * F[2] + k1.y * F[5] + F[8];
            const float den = la * la + lb * lb;
            int bestDist = RUMI_TH_LOW;
            for (int c = A.off2[lo]; c < A.off2[lo + 1]; c++) {
                const int i2 = (int)A.idx2[c];
                if (A.mp2[i2] >= 0) continue;
                const int dist = hamming256(d1, reinterpret_cast<const uint32_t *>(A.desc2 + (size_t)i2 * 32));
                if (dist > RUMI_TH_LOW || dist > bestDist) continue;
                const RumiKeyPoint k2 = A.keys2[i2];
                const float ex = epx - k2.x, ey = epy - k2.y;
                if (ex * ex + ey * ey < 100 * A.scale2[k2.octave]) continue;                       // :912-918
                if (!A.coarse) {
                    const float num = la * k2.x + lb * k2.y + lc;
                    if (den == 0) continue;
                    const float dsqr = num * num / den;
                    const float s2 = A.scale2[k2.octave] * A.scale2[k2.octave];                    // mvLevelSigma2
                    if (!((double)dsqr < 3.84 * (double)s2)) continue;
                }
                best = i2; bestDist = dist;
            }
        }
        A.assign[p] = best;
    }
}

// rotation-histogram filter + match count for k_tri_match (ORBmatcher.cc:964-1001); single workgroup
__global__ __launch_bounds__(256) void k_tri_filter(int nq, const uint32_t *idx1, const RumiKeyPoint *keys1, const RumiKeyPoint *keys2,
                                                    int32_t *assign, int checkOri, int32_t *nmatches) {
    __shared__ int sHist[RUMI_HISTO_LENGTH], sKeep[RUMI_HISTO_LENGTH], sCount;
    const int tid = threadIdx.x;
    if (tid < RUMI_HISTO_LENGTH) { sHist[tid] = 0; sKeep[tid] = 1; }
    if (tid == 0) sCount = 0;
    __syncthreads();
    if (checkOri) {
        for (int p = tid; p < nq; p += 256) {
            const int f = assign[p];
            if (f >= 0) atomicAdd(&sHist[rot_bin(keys1[idx1[p]].angle, keys2[f].angle)], 1);
        }
        __syncthreads();
        if (tid == 0) {
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
    int local = 0;
    for (int p = tid; p < nq; p += 256) {
        const int f = assign[p];
        if (f < 0) continue;
        if (checkOri && !sKeep[rot_bin(keys1[idx1[p]].angle, keys2[f].angle)]) assign[p] = -1;
        else local++;
    }
    atomicAdd(&sCount, local);
    __syncthreads();
    if (tid == 0) *nmatches = sCount;
}

// ---- brute force on the FP4 matrix cores -----------------------------------------------------------------------------
// With train bits t and query bits q (popcount pq): Ham(t, q) = pq + X, X = sum_k t_k (1 - 2 q_k), a GEMM of trains (A, values 0 / 1)
// by queries (B, values +1 / -1) over K = 256.  0, +1 and -1 are the E2M1 nibbles 0x0, 0x2 and 0xA, so the product runs on
// v_mfma_f32_32x32x64_f8f6f4 with FP4 operands and no block scale (4 per 32 x 32 tile, 4 VGPRs per fragment); sums of at most 256
// such products are exact in f32.  For one query pq is a constant, so the running (best, second) are kept on X and pq is added once at
// the end.  The key is the f32 number X + index / 65536 and it comes out of the MFMA itself: the chain's C operand starts at
// index / 65536.  |X| <= 255 leaves 16 fraction bits, X = -256 still does ([-256, -255) has ulp 2^-16), so every key of a pair at
// Ham < 256 is exact, and so is every partial sum (a partial X reaches 256 only as the whole sum).  X = 256 happens only at pq = 0,
// Ham = 256: the index rounds to even there, the key stays in [256, 257) because cap <= 65535 keeps the index at or below 65534 (the
// entries reject a larger cap), and such a pair is never a reported index.  f32 min and med3
// then order the keys exactly as (Ham << 16 | index) would: "first minimum wins, a tie goes to the second place" is
// best = min(best, key), second = med3(best, second, key): two v_med3_f32 per key (the min is med3 with -inf, see bfm_neg_inf).  The index field is 16 bits wide: cap <= 65535 runs through this one kernel.
//
// Fragment maps.  C/D of 32x32: column = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 h, h = lane >> 5.  A and B: lane l
// holds row (A) / column (B) l & 31 and 32 k-values that depend only on (h, nibble); the Hamming sum does not depend on the order
// of k, so both operands take the same bit -> nibble expansion and the hardware's k order never matters: k-step s, lane half h,
// fragment dword i, nibble j holds bit 4 j + s of descriptor dword 4 h + i.
//
// Workgroup: 4 waves, 64 queries each as two B-fragment sets (2 x 16 VGPRs, expanded once) and two accumulators, so one A fragment
// read feeds two MFMAs; train rows staged 64 at a time (two tiles), expanded into LDS as ready A fragments [tile][s][lane] (16 B
// each: one conflict-free ds_read_b128 per MFMA pair), double-buffered (2 x 8 KiB), one barrier per stage.  Per lane the 16
// accumulator rows belong to ONE query, so the reduction needs no cross-lane traffic until the end, where the two lane halves
// (lanes l and l + 32: same query) merge.  While looping a key carries the row WITHOUT the half's + 4 (a constant per lane keeps
// the argmin, and the index term is then wave-uniform: 16 VGPRs advanced by one v_add_f32 each per tile, shared by both
// accumulators); the merge adds it.  Padded train rows of the last tile are zero in LDS (X = 0) and their keys are replaced by 1024 (never beats
// the initial distance 256); padded query columns are computed and not written.
// Registers: 32 (B) + 32 (two accumulators) + 16 (index term) + fragments and addresses = 108 VGPRs, four waves a SIMD.  Held to 96 (five waves)
// the compiler spills B fragments into the loop and the launch is slower (66 against 58 us per 256 pairs, profiles/r08_bruteforce_stamps.txt).
typedef int32_t bfm_v4i __attribute__((ext_vector_type(4)));
typedef int32_t bfm_v8i __attribute__((ext_vector_type(8)));
typedef float bfm_v16f __attribute__((ext_vector_type(16)));
constexpr int kBfmWaves = 4, kBfmWaveQueries = 64, kBfmQueries = kBfmWaveQueries * kBfmWaves, kBfmStage = 64;
constexpr float kBfmIdx = 1.0f / 65536.0f;

__device__ __forceinline__ uint32_t bfm_expand(uint32_t x, int s) { return (x >> s) & 0x11111111u; }
// min as v_med3_f32(a, b, -inf): fminf would first quiet a possible signalling NaN in each MFMA result (one v_max_f32 x, x per key; keys are
// never NaN), and so would a med3 whose -inf the optimiser can see, which it turns back into fminf: the constant comes out of an asm
__device__ __forceinline__ float bfm_neg_inf() {
    float r;
    asm("s_mov_b32 %0, 0xff800000" : "=s"(r));
    return r;
}

#ifdef RUMI_BFM_STAMP
// cycle stamps (tools/build_stamp_lib.sh): wave 0 of the first workgroup of pair 0 sums its phases and prints them once
#define BFM_T(x) const long long x = clock64()
#define BFM_VAR(x) long long x = 0
#define BFM_FIRST(g, x) if ((g) == 0) x = clock64()
#define BFM_ADD(acc, a, b) acc += (b) - (a)
#else
#define BFM_T(x)
#define BFM_VAR(x)
#define BFM_FIRST(g, x)
#define BFM_ADD(acc, a, b)
#endif

__global__ __launch_bounds__(64 * kBfmWaves) __attribute__((amdgpu_waves_per_eu(4))) void k_bruteforce_mfma(const uint8_t *__restrict__ qd, const int32_t *__restrict__ nqArr,
                                                         const uint8_t *__restrict__ td, const int32_t *__restrict__ ntArr,
                                                         int countStride, long long qStride, long long tStride, int cap, int32_t *__restrict__ bestIdx,
                                                         int32_t *__restrict__ bestDist, int32_t *__restrict__ secondDist, int ring) {
    __shared__ bfm_v4i frag[2][2 * 4 * 64];                           // [buffer][tile * 4 + s][lane]
    const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, h = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int tb = ring > 0 ? (b + 1 == ring ? 0 : b + 1) : b;       // ring: frame b against its successor in the same buffer, the last against the first
    const int nq = min(nqArr[(size_t)b * countStride], cap), nt = min(ntArr[(size_t)tb * countStride], cap);
    const int q0 = blockIdx.x * kBfmQueries;
    if (q0 >= nq) return;
    const int qw = q0 + wave * kBfmWaveQueries;
    const bool waveLive = qw < nq;
    const float ninf = bfm_neg_inf();
#ifdef RUMI_BFM_STAMP
    long long cLoad = 0, cMfma = 0, cWait = 0, cKeys = 0, cStore = 0, cBar = 0;
    const long long cStart = clock64();
#endif

    // the queries: nibbles 0x2 (+1) / 0xA (-1) of this lane's half, and each one's popcount over both halves
    bfm_v8i bq[2][4];
    float best[2], second[2];
    auto query = [&](int u, uint32_t (&qa)[4]) -> int {              // this lane's half of query u of the wave; returns the popcount over both halves
        const int qi = qw + u * 32 + (lane & 31);
#pragma unroll
        for (int i = 0; i < 4; i++) qa[i] = 0;
        if (qi < nq) {
            const uint32_t *src = reinterpret_cast<const uint32_t *>(qd + (size_t)b * qStride + (size_t)qi * 32) + 4 * h;   // 4-byte aligned only
#pragma unroll
            for (int i = 0; i < 4; i++) qa[i] = src[i];
        }
        const int p = __popc(qa[0]) + __popc(qa[1]) + __popc(qa[2]) + __popc(qa[3]);
        return p + __shfl_xor(p, 32);
    };
#pragma unroll
    for (int u = 0; u < 2; u++) {
        uint32_t qa[4];
        const int pq = query(u, qa);
#pragma unroll
        for (int s = 0; s < 4; s++) {
            bq[u][s] = bfm_v8i{};
#pragma unroll
            for (int i = 0; i < 4; i++) bq[u][s][i] = (int32_t)((bfm_expand(qa[i], s) << 3) | 0x22222222u);
        }
        // X = 256 - pq is Ham = 256: the initial best and second (index 0; only the second's distance is ever read)
        best[u] = second[u] = (float)(256 - pq);
    }
    // the index term of the keys: rows of the tile at hand without the half's + 4
    bfm_v16f idxf;
#pragma unroll
    for (int g = 0; g < 16; g++) idxf[g] = (float)((g & 3) + 8 * (g >> 2)) * kBfmIdx;

    // staging: thread -> (fragment lane sl, dword i) of both tiles of the stage; per tile one source dword, four expanded dwords
    const int si = tid & 3, sl = tid >> 2;
    const int srow = sl & 31, sdw = 4 * (sl >> 5) + si;
    const uint32_t *tsrc = reinterpret_cast<const uint32_t *>(td + (size_t)tb * tStride) + sdw;
    auto load = [&](int r0, int tt) -> uint32_t { const int r = r0 + tt * 32 + srow; return r < nt ? tsrc[(size_t)r * 8] : 0u; };
    auto store = [&](int buf, int tt, uint32_t x) {
        uint32_t *dst = reinterpret_cast<uint32_t *>(&frag[buf][tt * 4 * 64 + sl]) + si;
#pragma unroll
        for (int s = 0; s < 4; s++) dst[s * 64 * 4] = bfm_expand(x, s) << 1;
    };
    if (nt > 0) { store(0, 0, load(0, 0)); store(0, 1, load(0, 1)); }
    __syncthreads();
    for (int r0 = 0, buf = 0; r0 < nt; r0 += kBfmStage, buf ^= 1) {
        const bool more = r0 + kBfmStage < nt;
        BFM_T(c0);
        const uint32_t next0 = more ? load(r0 + kBfmStage, 0) : 0u;   // in flight under this stage's MFMAs
        const uint32_t next1 = more ? load(r0 + kBfmStage, 1) : 0u;
        BFM_T(c1); BFM_ADD(cLoad, c0, c1);
        if (waveLive) {
#pragma unroll
            for (int tt = 0; tt < 2; tt++) {
                const int t0 = r0 + tt * 32;
                if (t0 >= nt) break;
                const bool partial = t0 + 32 > nt;                   // the last tile: rows at or past nt are zero in LDS (X = 0) and must not win
                BFM_T(m0); BFM_VAR(mw);
                bfm_v16f acc0 = idxf, acc1 = idxf;
#pragma unroll
                for (int s = 0; s < 4; s++) {
                    const bfm_v4i a4 = frag[buf][(tt * 4 + s) * 64 + lane];
                    const bfm_v8i a = {a4[0], a4[1], a4[2], a4[3], 0, 0, 0, 0};
                    acc0 = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a, bq[0][s], acc0, 4, 4, 0, 0, 0, 0);
                    acc1 = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a, bq[1][s], acc1, 4, 4, 0, 0, 0, 0);
                }
                BFM_T(m1); BFM_ADD(cMfma, m0, m1);
                if (partial) {
#pragma unroll
                    for (int g = 0; g < 16; g++) {
                        const bool live = t0 + (g & 3) + 8 * (g >> 2) + 4 * h < nt;
                        acc0[g] = live ? acc0[g] : 1024.0f; acc1[g] = live ? acc1[g] : 1024.0f;
                    }
                }
                // (plain code, not asm: the compiler pads the MFMA -> VALU read hazard)
#pragma unroll
                for (int g = 0; g < 16; g++) {
#pragma unroll
                    for (int u = 0; u < 2; u++) {
                        const float key = u ? acc1[g] : acc0[g];
                        second[u] = __builtin_amdgcn_fmed3f(best[u], second[u], key);
                        best[u] = __builtin_amdgcn_fmed3f(best[u], key, ninf);
                    }
                    BFM_FIRST(g, mw);                                // the first keys have waited for the MFMA results
                }
                BFM_T(m2); BFM_ADD(cWait, m1, mw); BFM_ADD(cKeys, mw, m2);
#pragma unroll
                for (int g = 0; g < 16; g++) idxf[g] += 32.0f * kBfmIdx;
            }
        }
        BFM_T(c2);
        if (more) { store(buf ^ 1, 0, next0); store(buf ^ 1, 1, next1); }
        BFM_T(c3); BFM_ADD(cStore, c2, c3);
        __syncthreads();
        BFM_T(c4); BFM_ADD(cBar, c3, c4);
    }
#ifdef RUMI_BFM_STAMP
    if (blockIdx.x == 0 && blockIdx.y == 0 && tid == 0)
        printf("bfm_stamp nq %d nt %d total %lld load %lld mfma %lld wait %lld keys %lld store %lld barrier %lld\n", nq, nt, clock64() - cStart, cLoad, cMfma, cWait, cKeys,
               cStore, cBar);
#endif
    // merge the halves: lane l + 32 holds the same query over rows + 4 (the popcount is read again: two registers less across the loop)
#pragma unroll
    for (int u = 0; u < 2; u++) {
        uint32_t qa[4];
        const int pq = query(u, qa), qi = qw + u * 32 + (lane & 31);
        const float ob = __shfl_xor(best[u], 32) + 4.0f * kBfmIdx, os = __shfl_xor(second[u], 32);
        if (h == 0 && qi < nq) {
            const float b2 = fminf(best[u], ob), s2 = fminf(fminf(second[u], os), fmaxf(best[u], ob));
            const size_t o = (size_t)b * cap + qi;
            const float fl = floorf(b2);
            const int d1 = (int)fl + pq;
            bestIdx[o] = d1 < 256 ? (int)((b2 - fl) * 65536.0f) : -1;
            bestDist[o] = d1; secondDist[o] = (int)floorf(s2) + pq;
        }
    }
}

// the blocking of k_bruteforce_mfma, for tests that place cases on its edges: queries per wave, queries per workgroup, train rows per stage
extern "C" void rumi_match_bruteforce_shape(int32_t *out3) { out3[0] = kBfmWaveQueries; out3[1] = kBfmQueries; out3[2] = kBfmStage; }

static int launch_bruteforce(const void *qd, const void *nq, const void *td, const void *nt, int count_stride, long long q_stride, long long t_stride,
                             int cap, int nrows, void *best_idx, void *best_dist, void *second_dist, int ring, hipStream_t st) {
    const dim3 grid((cap + kBfmQueries - 1) / kBfmQueries, nrows);
    hipLaunchKernelGGL(k_bruteforce_mfma, grid, dim3(64 * kBfmWaves), 0, st, (const uint8_t *)qd, (const int32_t *)nq, (const uint8_t *)td, (const int32_t *)nt,
                       count_stride, q_stride, t_stride, cap, (int32_t *)best_idx, (int32_t *)best_dist, (int32_t *)second_dist, ring);
    HIP_TRY(hipGetLastError());
    return RUMI_OK;
}


// ------------------------------------------------------------------------------------------------
// SearchByBoW(KF_k, F) for K candidate key-frames against ONE frame in one launch (Tracking::Relocalization walks the candidates of
// KeyFrameDatabase::DetectRelocalizationCandidates one by one, Tracking.cc:3240-3260; every walk starts from an empty vpMapPointMatches, so the
// K searches are independent).  Within one search a frame feature is taken by the first query that wins it -- but a frame feature lies in
// exactly ONE FeatureVector node, so that dependency never leaves a node: nodes run in parallel, the (few) key-frame features of a node
// sequentially.  16 lanes per (key-frame, node): the lanes share out the frame's features of the node, compute their Hamming distances
// to the current key-frame feature in parallel and reduce (best, second) with the reference's tie rules (ORBmatcher.cc:252-289).
// ------------------------------------------------------------------------------------------------
struct BowKF { int32_t n, nn, angle, desc, mp, good, nodes, off, idx, pad; };      // sizes and dword offsets of one key-frame's arrays in the block
struct BowBatch {
    const uint32_t *blk;          // the uploaded block (dword view)
    int K, nf, nnF;
    int fAngle, fDesc, fNodes, fOff, fIdx, kfTable;     // dword offsets
    int32_t *matches;             // [K][nf]  map-point index (per key-frame numbering), -1 none
    int8_t *rotBin;               // [K][nf]
    int32_t *hist;                // [K][32]
    int32_t *nmatch;              // [K]
    int32_t *err;                 // bit 0: a node with more than 512 frame features
    float nnratio;
    int checkOri;
};

__global__ __launch_bounds__(256) void k_bow_batch_match(BowBatch B) {
    const int k = blockIdx.y, lane = threadIdx.x & 15, a = blockIdx.x * 16 + (threadIdx.x >> 4);
    const BowKF *T = reinterpret_cast<const BowKF *>(B.blk + B.kfTable) + k;
    if (a >= T->nn) return;
    const uint32_t *kfNodes = B.blk + T->nodes, *fNodes = B.blk + B.fNodes;
    const uint32_t node = kfNodes[a];
    int lo = 0, hi = B.nnF;                                  // first frame node >= node (std::map order: ascending ids)
    while (lo < hi) { const int mid = (lo + hi) >> 1; if (fNodes[mid] < node) lo = mid + 1; else hi = mid; }
    if (lo >= B.nnF || fNodes[lo] != node) return;
    const int32_t *fOff = reinterpret_cast<const int32_t *>(B.blk + B.fOff), *kOff = reinterpret_cast<const int32_t *>(B.blk + T->off);
    const int c0 = fOff[lo], nc = fOff[lo + 1] - c0;
    if (nc > 512) { if (lane == 0) atomicOr(B.err, 1); return; }
    const uint32_t *fIdx = B.blk + B.fIdx + c0, *kIdx = B.blk + T->idx;
    const uint32_t *fDesc = B.blk + B.fDesc, *kDesc = B.blk + T->desc;
    const float *fAngle = reinterpret_cast<const float *>(B.blk + B.fAngle), *kAngle = reinterpret_cast<const float *>(B.blk + T->angle);
    const int32_t *kMp = reinterpret_cast<const int32_t *>(B.blk + T->mp);
    const uint8_t *kGood = reinterpret_cast<const uint8_t *>(B.blk + T->good);
    uint32_t taken = 0;                                      // bit j: my candidate lane + 16 j already holds a map point
    for (int p = kOff[a]; p < kOff[a + 1]; p++) {
        const int iKF = (int)kIdx[p];
        if (!kGood[iKF]) continue;                           // no map point, or a bad one (:238-243)
        uint32_t q[8];
#pragma unroll
        for (int w = 0; w < 8; w++) q[w] = kDesc[(size_t)iKF * 8 + w];
        uint32_t best = (256u << 16) | 0xFFFFu, second = 256u;
        for (int j = 0, pos = lane; pos < nc; j++, pos += 16) {
            if ((taken >> j) & 1u) continue;
            const uint32_t *d = fDesc + (size_t)fIdx[pos] * 8;
            uint32_t dist = 0;
#pragma unroll
            for (int w = 0; w < 8; w++) dist += __popc(q[w] ^ d[w]);
            const uint32_t key = (dist << 16) | (uint32_t)pos;
            if (key < best) { second = best >> 16; best = key; }       // a strictly smaller distance, or the same at an earlier position
            else if (dist < second) second = dist;
        }
        // 16-lane reduction: best = smallest key; second = second smallest distance of the union
#pragma unroll
        for (int o = 8; o > 0; o >>= 1) {
            const uint32_t ob = __shfl_xor(best, o, 16), os = __shfl_xor(second, o, 16);
            const uint32_t loser = max(best, ob) >> 16;
            best = min(best, ob);
            second = min(min(second, os), loser);
        }
        const int bestDist1 = (int)(best >> 16), bestDist2 = (int)second;
        if (bestDist1 <= RUMI_TH_LOW && (float)bestDist1 < B.nnratio * (float)bestDist2) {
            const int pos = (int)(best & 0xFFFFu), f = (int)fIdx[pos];
            if (lane == (pos & 15)) taken |= 1u << (pos >> 4);
            if (lane == 0) {
                B.matches[(size_t)k * B.nf + f] = kMp[iKF];
                if (B.checkOri) {
                    const int bin = rot_bin(kAngle[iKF], fAngle[f]);
                    B.rotBin[(size_t)k * B.nf + f] = (int8_t)bin;
                    atomicAdd(&B.hist[k * 32 + bin], 1);
                }
            }
        }
    }
}

// rotation-histogram filter (ComputeThreeMaxima, ORBmatcher.cc:1795-1826) and the match count of every key-frame
__global__ __launch_bounds__(256) void k_bow_batch_finish(BowBatch B) {
    __shared__ int sKeep[RUMI_HISTO_LENGTH], sCount;
    const int k = blockIdx.x, tid = threadIdx.x;
    if (tid == 0) {
        sCount = 0;
        for (int i = 0; i < RUMI_HISTO_LENGTH; i++) sKeep[i] = 1;
        if (B.checkOri) {
            int max1 = 0, max2 = 0, max3 = 0, ind1 = -1, ind2 = -1, ind3 = -1;
            for (int i = 0; i < RUMI_HISTO_LENGTH; i++) {
                const int s = B.hist[k * 32 + i];
                if (s > max1) { max3 = max2; max2 = max1; max1 = s; ind3 = ind2; ind2 = ind1; ind1 = i; }
                else if (s > max2) { max3 = max2; max2 = s; ind3 = ind2; ind2 = i; }
                else if (s > max3) { max3 = s; ind3 = i; }
            }
            if (max2 < 0.1f * (float)max1) { ind2 = -1; ind3 = -1; }
            else if (max3 < 0.1f * (float)max1) ind3 = -1;
            for (int i = 0; i < RUMI_HISTO_LENGTH; i++) sKeep[i] = (i == ind1 || i == ind2 || i == ind3);
        }
    }
    __syncthreads();
    int local = 0;
    for (int f = tid; f < B.nf; f += 256) {
        int32_t &m = B.matches[(size_t)k * B.nf + f];
        if (m < 0) continue;
        if (B.checkOri && !sKeep[B.rotBin[(size_t)k * B.nf + f]]) m = -1; else local++;
    }
    atomicAdd(&sCount, local);
    __syncthreads();
    if (tid == 0) B.nmatch[k] = sCount;
}

}  // namespace rumi

using namespace rumi;

// ================================================ host side =======================================================
extern "C" int rumi_descriptor_distance(const uint8_t *a, const uint8_t *b) {
    uint64_t x[4], y[4];
    std::memcpy(x, a, 32); std::memcpy(y, b, 32);
    return __builtin_popcountll(x[0] ^ y[0]) + __builtin_popcountll(x[1] ^ y[1]) + __builtin_popcountll(x[2] ^ y[2]) +
           __builtin_popcountll(x[3] ^ y[3]);
}

extern "C" void rumi_match_destroy(RumiMatcher *m) {
    if (!m) return;
    (void)hipSetDevice(m->device);
    if (m->ext.state && m->ext.destroy) m->ext.destroy(m->ext.state);
    void *p[] = {m->dKeys, m->dDesc, m->dScale, m->dSorted, m->dCellStart, m->dFvIdx, m->dQ, m->dQDesc, m->dCounts,
                 m->dOffsets, m->dLists, m->dOut, m->dU8a, m->dU8b, m->dF[0], m->dF[1], m->dF[2], m->dF[3],
                 m->dF[4], m->dF[5], m->dI[0], m->dI[1], m->dI[2], m->dI[3], m->dQKeys, m->dNodesA, m->dNodesB, m->dIdxA,
                 m->dOffA, m->dOffB, m->dPose, m->dStage};
    for (void *q : p) if (q) (void)hipFree(q);
    if (m->hStage) (void)hipHostFree(m->hStage);
    if (m->hOut) (void)hipHostFree(m->hOut);
    if (m->hBow) (void)hipHostFree(m->hBow);
    if (m->hBowOut) (void)hipHostFree(m->hBowOut);
    if (m->dBow) (void)hipFree(m->dBow);
    if (m->dBowOut) (void)hipFree(m->dBowOut);
    delete m;
}

extern "C" int rumi_match_create(int32_t max_features, int32_t max_queries, int32_t device, RumiMatcher **out) {
    if (!out) return RUMI_E_INVALID;
    *out = nullptr;
    if (max_features < 1 || max_features > kMaxSortN || max_queries < 1) {
        g_lastError = "rumi_match_create: max_features must be in 1..16384, max_queries >= 1";
        return RUMI_E_INVALID;
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
        g_lastError = "no HIP device visible: librumi_hip has no CPU fallback";
        return RUMI_E_NO_DEVICE;
    }
    RumiMatcher *m = new RumiMatcher();
    if (device >= 0) m->device = device; else if (hipGetDevice(&m->device) != hipSuccess) m->device = 0;
    if (hipSetDevice(m->device) != hipSuccess) { delete m; return RUMI_E_NO_DEVICE; }
    m->maxFeat = max_features; m->maxQ = max_queries;
    m->listCap = (size_t)max_queries * 256 + 65536;     // grown on demand
    const size_t F = max_features, Q = max_queries;
    int rc;
#define TRYA(x) if ((rc = (x)) != RUMI_OK) { rumi_match_destroy(m); return rc; }
    TRYA(dalloc(&m->dKeys, F)); TRYA(dalloc(&m->dDesc, F * 32)); TRYA(dalloc(&m->dScale, 64));
    TRYA(dalloc(&m->dSorted, F)); TRYA(dalloc(&m->dCellStart, kGridCells + 2));
    TRYA(dalloc(&m->dFvIdx, F));
    TRYA(dalloc(&m->dQ, Q)); TRYA(dalloc(&m->dQDesc, Q * 32)); TRYA(dalloc(&m->dCounts, Q + 1)); TRYA(dalloc(&m->dOffsets, Q + 1));
    TRYA(dalloc(&m->dLists, m->listCap));
    TRYA(dalloc(&m->dOut, 4 + F + Q));
    m->dNmatches = m->dOut; m->dOverflow = m->dOut + 1; m->dFeatMp = m->dOut + 4; m->dAssign = m->dOut + 4 + F;
    TRYA(dalloc(&m->dU8a, Q)); TRYA(dalloc(&m->dU8b, std::max(Q, F)));
    for (auto &f : m->dF) TRYA(dalloc(&f, Q * 3));
    for (auto &i : m->dI) TRYA(dalloc(&i, Q + 1));
    TRYA(dalloc(&m->dQKeys, Q)); TRYA(dalloc(&m->dNodesA, Q)); TRYA(dalloc(&m->dNodesB, F)); TRYA(dalloc(&m->dIdxA, Q));
    TRYA(dalloc(&m->dOffA, Q + 1)); TRYA(dalloc(&m->dOffB, F + 1)); TRYA(dalloc(&m->dPose, 32));
    m->stageCap = kStageHeader + F * 112 + Q * 224 + 65536;
    TRYA(dalloc(&m->dStage, m->stageCap));
    if (hipHostMalloc((void **)&m->hStage, m->stageCap, hipHostMallocDefault) != hipSuccess ||
        hipHostMalloc((void **)&m->hOut, (4 + F + Q) * sizeof(int32_t), hipHostMallocDefault) != hipSuccess) {
        g_lastError = "rumi_match_create: pinned host allocation failed";
        rumi_match_destroy(m);
        return RUMI_E_NO_DEVICE;
    }
    m->stageUsed = kStageHeader;
#undef TRYA
    *out = m;
    return RUMI_OK;
}

namespace rumi {

int stage_add(RumiMatcher *m, void *dst, const void *src, size_t bytes) {
    if (bytes == 0) return RUMI_OK;
    const size_t off = (m->stageUsed + 15) & ~(size_t)15;
    if (m->nseg >= kMaxSegments || off + bytes > m->stageCap) {
        g_lastError = "matcher upload block exhausted (raise max_features / max_queries)";
        return RUMI_E_CAPACITY;
    }
    std::memcpy(m->hStage + off, src, bytes);
    reinterpret_cast<Segment *>(m->hStage)[m->nseg++] = Segment{dst, (uint32_t)off, (uint32_t)bytes};
    m->stageUsed = off + bytes;
    return RUMI_OK;
}

int flush_uploads(RumiMatcher *m) {
    if (m->nseg > 0) {
        HIP_TRY(hipMemcpyAsync(m->dStage, m->hStage, m->stageUsed, hipMemcpyHostToDevice, m->upStream));
        hipLaunchKernelGGL(k_scatter, dim3(8, m->nseg), dim3(256), 0, m->upStream, m->dStage, m->nseg);
        m->nseg = 0;
        m->stageUsed = kStageHeader;
    }
    if (m->gridPending) {
        hipLaunchKernelGGL(k_grid, dim3(1), dim3(1024), 0, nullptr, m->gridN, m->gridKeys ? m->gridKeys : m->dKeys, m->gridMinX, m->gridMinY, m->gridWInv, m->gridHInv,
                           m->dSorted, m->dCellStart, m->gridNDev);
        m->gridPending = false;
        m->gridNDev = nullptr;
    }
    return RUMI_OK;
}

void reset_uploads(RumiMatcher *m) { m->nseg = 0; m->stageUsed = kStageHeader; m->gridPending = false; }

int upload_frame(RumiMatcher *m, const RumiFrameFeatures *F, FrameDev *fd) {
    reset_uploads(m);
    if (!F || F->n < 0 || F->n > m->maxFeat || F->nlevels < 1 || F->nlevels > 64 || !(F->max_x > F->min_x) || !(F->max_y > F->min_y)) {
        g_lastError = "bad RumiFrameFeatures (n, nlevels or bounds)";
        return RUMI_E_INVALID;
    }
    if (F->n > 0) { H2D(m->dKeys, F->keys_un, F->n); H2D(m->dDesc, F->desc, (size_t)F->n * 32); }
    H2D(m->dScale, F->scale_factors, F->nlevels);
    static const int32_t kZeroHeader[4] = {0, 0, 0, 0};     // result header [nmatches | list overflow | - | -]: cleared by the same scatter
    H2D(m->dOut, kZeroHeader, 4);
    fd->n = F->n; fd->keys = m->dKeys; fd->desc = m->dDesc;
    fd->minX = F->min_x; fd->minY = F->min_y; fd->maxX = F->max_x; fd->maxY = F->max_y;
    fd->wInv = (float)kGridCols / (float)(F->max_x - F->min_x);     // Frame.cc:322-323
    fd->hInv = (float)kGridRows / (float)(F->max_y - F->min_y);
    fd->sortedIdx = m->dSorted; fd->cellStart = m->dCellStart; fd->scale = m->dScale;
    m->gridPending = true; m->gridKeys = nullptr; m->gridN = F->n; m->gridMinX = fd->minX; m->gridMinY = fd->minY; m->gridWInv = fd->wInv; m->gridHInv = fd->hInv;
    return RUMI_OK;
}

// count pass, scan, fill pass.  The fill pass refuses to write past the list arena and raises the overflow word instead; the
// caller sees it in the result block, grows the arena and repeats the call (run_search) — no mid-pipeline read-back.
int build_lists(RumiMatcher *m, int mode, int nq, const FrameDev &fd, const uint8_t *dQueryDesc, bool retry, bool fused) {
    FLUSH(m);
    if (retry) HIP_TRY(hipMemsetAsync(m->dOut, 0, 4 * sizeof(int32_t), nullptr));   // the first attempt's header was cleared with the frame upload
    if (nq > 0 && fused) {
        // one launch: every query's list in a fixed slot of the arena (k_candidates<2>)
        const int slot = (int)std::min<size_t>(m->listCap / (size_t)nq, 0x7FFFFFFF / (size_t)nq);
        hipLaunchKernelGGL(k_candidates<2>, dim3((nq + 3) / 4), dim3(256), 0, nullptr, mode, nq, m->dQ, fd, dQueryDesc, m->dFvIdx,
                           m->dCounts, m->dOffsets, m->dLists, slot, m->dOverflow);
    } else if (nq > 0) {
        hipLaunchKernelGGL(k_candidates<0>, dim3((nq + 3) / 4), dim3(256), 0, nullptr, mode, nq, m->dQ, fd, dQueryDesc, m->dFvIdx,
                           m->dCounts, m->dOffsets, m->dLists, 0, m->dOverflow);
        hipLaunchKernelGGL(k_scan, dim3(1), dim3(256), 0, nullptr, nq, m->dCounts, m->dOffsets);
        hipLaunchKernelGGL(k_candidates<1>, dim3((nq + 3) / 4), dim3(256), 0, nullptr, mode, nq, m->dQ, fd, dQueryDesc, m->dFvIdx,
                           m->dCounts, m->dOffsets, m->dLists, (int)std::min<size_t>(m->listCap, 0x7FFFFFFF), m->dOverflow);
    }
    return RUMI_OK;
}

// bring back [header | featMp | assign] with one copy; returns RUMI_E_CAPACITY-like signal through *overflowTotal
static int fetch_results(RumiMatcher *m, int nfeat, int nq, bool wantAssign) {
    const size_t ints = wantAssign ? (size_t)4 + m->maxFeat + std::max(nq, 0) : (size_t)4 + std::max(nfeat, 0);
    HIP_TRY(hipMemcpy(m->hOut, m->dOut, ints * sizeof(int32_t), hipMemcpyDeviceToHost));
    return RUMI_OK;
}

static int grow_lists(RumiMatcher *m, size_t need) {
    (void)hipFree(m->dLists);
    m->dLists = nullptr;
    m->listCap = need * 2;
    return dalloc(&m->dLists, m->listCap);
}

int run_search(RumiMatcher *m, int mode, int nq, const FrameDev &fd, const uint8_t *dQueryDesc, const int32_t *dMpObs, float nnratio, int checkOri,
               int32_t *hostFeatMp, int32_t *nmatchesOut, const uint8_t *dBlocked0, float thrF, int thrI, int32_t *hostAssign) {
    // first with every query's list in a fixed slot (one candidate launch); a query that does not fit falls back to count / scan / fill, which
    // sizes the lists exactly and grows the arena when needed
    bool fused = track_speculation().fused && nq > 0 && m->listCap / (size_t)nq >= 64;
    for (int attempt = 0, grown = 0; attempt < 4; attempt++) {
        const int rcl = build_lists(m, mode, nq, fd, dQueryDesc, attempt > 0, fused);
        if (rcl != RUMI_OK) return rcl;
        ResolveArgs A{mode, nq, fd.n, m->dQ, m->dCounts, m->dOffsets, m->dLists, fd.keys, dMpObs, m->dFeatMp, m->dAssign, m->dNmatches,
                      nnratio, checkOri, dBlocked0, thrF, thrI, m->dOverflow};
        launch_resolve(A, nullptr);
        HIP_TRY(hipGetLastError());
        const int rcf = fetch_results(m, fd.n, nq, hostAssign != nullptr);
        if (rcf != RUMI_OK) return rcf;
        if (m->hOut[1] == 0) break;
        if (m->hOut[1] == kFusedOverflow) { fused = false; continue; }      // the resolve did not run; repeat with exact list sizes
        // list arena too small: the resolve did not run and the frame's map-point vector is untouched
        if (grown) { g_lastError = "candidate list arena overflow after growing"; return RUMI_E_CAPACITY; }
        const int rcg = grow_lists(m, (size_t)m->hOut[1]);
        if (rcg != RUMI_OK) return rcg;
        grown = 1;
    }
    *nmatchesOut = m->hOut[0];
    if (fd.n > 0 && hostFeatMp) std::memcpy(hostFeatMp, m->hOut + 4, (size_t)fd.n * sizeof(int32_t));
    if (nq > 0 && hostAssign) std::memcpy(hostAssign, m->hOut + 4 + m->maxFeat, (size_t)nq * sizeof(int32_t));
    return RUMI_OK;
}

const SearchSwitches &track_speculation() {
    static const SearchSwitches sw = [] {
        const char *spec = std::getenv("RUMI_TRACK_SPECULATE");
        const bool fused = std::getenv("RUMI_MATCH_NO_FUSED") == nullptr;
        return SearchSwitches{fused, fused && (spec ? std::atoi(spec) : 1) != 0};
    }();
    return sw;
}

void launch_queries_frame(RumiMatcher *m, const FrameDev &fd, int nlast, float th, hipStream_t st) {
    hipLaunchKernelGGL(k_queries_frame, dim3((nlast + 255) / 256), dim3(256), 0, st, nlast, m->dQKeys, m->dI[0], m->dU8a, m->dF[0], m->dI[1], m->dPose,
                       m->dPose + 7, m->dScale, th, fd.minX, fd.minY, fd.maxX, fd.maxY, m->dQ);
}
void launch_queries_bow(RumiMatcher *m, int nEntries, int nnKF, int nnF, const int32_t *nnFdev, hipStream_t st) {
    hipLaunchKernelGGL(k_queries_bow, dim3((std::max(nEntries, 1) + 255) / 256), dim3(256), 0, st, nnKF, m->dNodesA, m->dOffA, m->dIdxA, m->dI[0], m->dU8a,
                       m->dQKeys, nnF, m->dNodesB, m->dOffB, m->dQ, nnFdev);
}
void launch_resolve(const ResolveArgs &A, hipStream_t st) {
    hipLaunchKernelGGL(k_resolve, dim3(1), dim3(1024), (size_t)std::max(A.nfeat, 1) * sizeof(int32_t), st, A);
}

}  // namespace rumi

extern "C" int rumi_search_by_projection_mappoints(RumiMatcher *m, const RumiFrameFeatures *F, int32_t nmp,
                                                   const uint8_t *track_in_view, const float *proj_x, const float *proj_y,
                                                   const int32_t *scale_level, const float *view_cos, const float *track_depth,
                                                   const uint8_t *is_bad, const uint8_t *mp_desc, const int32_t *mp_obs, float th,
                                                   int32_t far_points, float th_far_points, float nnratio, int32_t *frame_mp,
                                                   int32_t *nmatches_out) {
    if (!m || !nmatches_out || !frame_mp || nmp < 0) return RUMI_E_INVALID;
    if (nmp > m->maxQ) { g_lastError = "more map points than max_queries"; return RUMI_E_CAPACITY; }
    HIP_TRY(hipSetDevice(m->device));
    FrameDev fd;
    int rc = upload_frame(m, F, &fd);
    if (rc != RUMI_OK) return rc;
    if (F->n > 0) H2D(m->dFeatMp, frame_mp, F->n);
    if (nmp > 0) {
        H2D(m->dU8a, track_in_view, nmp); H2D(m->dU8b, is_bad, nmp);
        H2D(m->dF[0], proj_x, nmp); H2D(m->dF[1], proj_y, nmp); H2D(m->dF[2], view_cos, nmp); H2D(m->dF[3], track_depth, nmp);
        H2D(m->dI[0], scale_level, nmp); H2D(m->dI[1], mp_obs, nmp);
        H2D(m->dQDesc, mp_desc, (size_t)nmp * 32);
        FLUSH(m);
        hipLaunchKernelGGL(k_queries_mappoints, dim3((nmp + 255) / 256), dim3(256), 0, nullptr, nmp, m->dU8a, m->dF[0], m->dF[1],
                           m->dI[0], m->dF[2], m->dF[3], m->dU8b, m->dI[1], m->dScale, th, far_points, th_far_points, m->dQ);
    }
    return run_search(m, MODE_MAPPOINTS, nmp, fd, m->dQDesc, m->dI[1], nnratio, 0, frame_mp, nmatches_out);
}

extern "C" int rumi_search_by_projection_frame(RumiMatcher *m, const RumiFrameFeatures *Cur, const float *Tcw7, const float *K4,
                                               const RumiKeyPoint *last_keys, int32_t nlast, const int32_t *last_mp,
                                               const uint8_t *last_outlier, int32_t nmp, const float *mp_pos, const uint8_t *mp_desc,
                                               const int32_t *mp_obs, float th, int32_t check_orientation, int32_t *cur_mp,
                                               int32_t *nmatches_out) {
    if (!m || !nmatches_out || !cur_mp || nlast < 0 || nmp < 0 || !Tcw7 || !K4) return RUMI_E_INVALID;
    if (nlast > m->maxQ || nmp > m->maxQ) { g_lastError = "more last-frame features / map points than max_queries"; return RUMI_E_CAPACITY; }
    HIP_TRY(hipSetDevice(m->device));
    FrameDev fd;
    int rc = upload_frame(m, Cur, &fd);
    if (rc != RUMI_OK) return rc;
    if (Cur->n > 0) H2D(m->dFeatMp, cur_mp, Cur->n);
    float pose[11];
    std::memcpy(pose, Tcw7, 7 * sizeof(float)); std::memcpy(pose + 7, K4, 4 * sizeof(float));
    H2D(m->dPose, pose, 11);
    if (nmp > 0) { H2D(m->dF[0], mp_pos, (size_t)nmp * 3); H2D(m->dI[1], mp_obs, nmp); H2D(m->dQDesc, mp_desc, (size_t)nmp * 32); }
    if (nlast > 0) {
        H2D(m->dQKeys, last_keys, nlast); H2D(m->dI[0], last_mp, nlast); H2D(m->dU8a, last_outlier, nlast);
        FLUSH(m);
        launch_queries_frame(m, fd, nlast, th, nullptr);
    }
    return run_search(m, MODE_FRAME, nlast, fd, m->dQDesc, m->dI[1], 0.f, check_orientation, cur_mp, nmatches_out);
}

extern "C" int rumi_search_by_bow(RumiMatcher *m, const RumiFrameFeatures *KF, const RumiFeatureVector *kf_fv, const int32_t *kf_mp,
                                  int32_t nmp, const uint8_t *mp_bad, const RumiFrameFeatures *F, const RumiFeatureVector *f_fv,
                                  float nnratio, int32_t check_orientation, int32_t *matches, int32_t *nmatches_out) {
    if (!m || !KF || !kf_fv || !f_fv || !matches || !nmatches_out || nmp < 0 || !kf_mp) return RUMI_E_INVALID;
    const int nqe = kf_fv->n_nodes > 0 ? kf_fv->offsets[kf_fv->n_nodes] : 0;     // one query per FeatureVector entry
    const int nfe = f_fv->n_nodes > 0 ? f_fv->offsets[f_fv->n_nodes] : 0;
    if (KF->n > m->maxQ || nqe > m->maxQ || nmp > m->maxQ || kf_fv->n_nodes > m->maxQ || nfe > m->maxFeat || f_fv->n_nodes > m->maxFeat) {
        g_lastError = "SearchByBoW: sizes exceed the matcher's capacities";
        return RUMI_E_CAPACITY;
    }
    HIP_TRY(hipSetDevice(m->device));
    FrameDev fd;
    int rc = upload_frame(m, F, &fd);
    if (rc != RUMI_OK) return rc;
    if (KF->n > 0) { H2D(m->dQKeys, KF->keys_un, KF->n); H2D(m->dQDesc, KF->desc, (size_t)KF->n * 32); H2D(m->dI[0], kf_mp, KF->n); }
    if (nmp > 0) H2D(m->dU8a, mp_bad, nmp);
    if (kf_fv->n_nodes > 0) { H2D(m->dNodesA, kf_fv->node_ids, kf_fv->n_nodes); H2D(m->dOffA, kf_fv->offsets, kf_fv->n_nodes + 1); }
    if (nqe > 0) H2D(m->dIdxA, kf_fv->indices, nqe);
    if (f_fv->n_nodes > 0) { H2D(m->dNodesB, f_fv->node_ids, f_fv->n_nodes); H2D(m->dOffB, f_fv->offsets, f_fv->n_nodes + 1); }
    if (nfe > 0) H2D(m->dFvIdx, f_fv->indices, nfe);
    m->gridPending = false;                                 // candidates come from the FeatureVectors: the spatial grid is not read
    FLUSH(m);
    if (kf_fv->n_nodes > 0) launch_queries_bow(m, nqe, kf_fv->n_nodes, f_fv->n_nodes, nullptr, nullptr);
    return run_search(m, MODE_BOW, nqe, fd, m->dQDesc, nullptr, nnratio, check_orientation, matches, nmatches_out);
}

extern "C" int rumi_search_by_bow_batch(RumiMatcher *m, int32_t K, const RumiFrameFeatures *KFs, const RumiFeatureVector *kf_fvs,
                                        const int32_t *const *kf_mp, const int32_t *nmp, const uint8_t *const *mp_bad, const RumiFrameFeatures *F,
                                        const RumiFeatureVector *f_fv, float nnratio, int32_t check_orientation, int32_t *matches,
                                        int32_t *nmatches_out) {
    if (!m || K < 1 || !KFs || !kf_fvs || !kf_mp || !nmp || !mp_bad || !F || !f_fv || !matches || !nmatches_out || F->n < 0) return RUMI_E_INVALID;
    HIP_TRY(hipSetDevice(m->device));
    const int nf = F->n, nnF = f_fv->n_nodes, nfe = nnF > 0 ? f_fv->offsets[nnF] : 0;
    for (int k = 0; k < K; k++) {
        nmatches_out[k] = 0;
        if (KFs[k].n < 0 || kf_fvs[k].n_nodes < 0 || nmp[k] < 0 || (KFs[k].n > 0 && !kf_mp[k])) return RUMI_E_INVALID;
    }
    for (size_t i = 0; i < (size_t)K * std::max(nf, 0); i++) matches[i] = -1;
    if (nf == 0 || nnF == 0) return RUMI_OK;
    // ---- one block: [frame arrays | key-frame table | key-frame arrays], every array on a 16-byte boundary ----
    size_t used = 0;
    auto take = [&](size_t bytes) { const size_t o = used; used += (bytes + 15) & ~(size_t)15; return o; };
    const size_t oFA = take((size_t)nf * 4), oFD = take((size_t)nf * 32), oFN = take((size_t)nnF * 4), oFO = take((size_t)(nnF + 1) * 4), oFI = take((size_t)nfe * 4);
    const size_t oT = take((size_t)K * sizeof(BowKF));
    std::vector<BowKF> tab(K);
    int maxNodes = 0;
    for (int k = 0; k < K; k++) {
        const int n = KFs[k].n, nn = kf_fvs[k].n_nodes, ne = nn > 0 ? kf_fvs[k].offsets[nn] : 0;
        BowKF &t = tab[k];
        t.n = n; t.nn = nn; t.pad = 0;
        t.angle = (int32_t)(take((size_t)n * 4) / 4); t.desc = (int32_t)(take((size_t)n * 32) / 4); t.mp = (int32_t)(take((size_t)n * 4) / 4);
        t.good = (int32_t)(take((size_t)n) / 4); t.nodes = (int32_t)(take((size_t)nn * 4) / 4); t.off = (int32_t)(take((size_t)(nn + 1) * 4) / 4);
        t.idx = (int32_t)(take((size_t)ne * 4) / 4);
        maxNodes = std::max(maxNodes, nn);
    }
    if (used > m->bowCap) {
        if (m->hBow) HIP_TRY(hipHostFree(m->hBow));
        if (m->dBow) HIP_TRY(hipFree(m->dBow));
        m->hBow = nullptr; m->dBow = nullptr; m->bowCap = 0;
        HIP_TRY(hipHostMalloc((void **)&m->hBow, used * 2, hipHostMallocDefault));
        HIP_TRY(hipMalloc((void **)&m->dBow, used * 2));
        m->bowCap = used * 2;
    }
    // outputs: [matches K nf | nmatch K | err 1 | hist K 32 | rotBin K nf bytes]; the first part comes back
    const size_t outInts = (size_t)K * nf + K + 1, outBytes = (outInts + (size_t)K * 32) * 4 + (size_t)K * nf;
    if (outBytes > m->bowOutCap) {
        if (m->hBowOut) HIP_TRY(hipHostFree(m->hBowOut));
        if (m->dBowOut) HIP_TRY(hipFree(m->dBowOut));
        m->hBowOut = nullptr; m->dBowOut = nullptr; m->bowOutCap = 0;
        HIP_TRY(hipHostMalloc((void **)&m->hBowOut, outBytes * 2, hipHostMallocDefault));
        HIP_TRY(hipMalloc((void **)&m->dBowOut, outBytes * 2));
        m->bowOutCap = outBytes * 2;
    }
    uint8_t *h = m->hBow;
    float *fa = reinterpret_cast<float *>(h + oFA);
    for (int i = 0; i < nf; i++) fa[i] = F->keys_un[i].angle;
    std::memcpy(h + oFD, F->desc, (size_t)nf * 32);
    std::memcpy(h + oFN, f_fv->node_ids, (size_t)nnF * 4);
    std::memcpy(h + oFO, f_fv->offsets, (size_t)(nnF + 1) * 4);
    if (nfe > 0) std::memcpy(h + oFI, f_fv->indices, (size_t)nfe * 4);
    std::memcpy(h + oT, tab.data(), (size_t)K * sizeof(BowKF));
    for (int k = 0; k < K; k++) {
        const BowKF &t = tab[k];
        const int n = t.n, nn = t.nn, ne = nn > 0 ? kf_fvs[k].offsets[nn] : 0;
        float *ka = reinterpret_cast<float *>(h + (size_t)t.angle * 4);
        uint8_t *good = h + (size_t)t.good * 4;
        for (int i = 0; i < n; i++) {
            ka[i] = KFs[k].keys_un[i].angle;
            const int mp = kf_mp[k][i];
            good[i] = mp >= 0 && mp < nmp[k] && !(mp_bad[k] && mp_bad[k][mp]);
        }
        if (n > 0) { std::memcpy(h + (size_t)t.desc * 4, KFs[k].desc, (size_t)n * 32); std::memcpy(h + (size_t)t.mp * 4, kf_mp[k], (size_t)n * 4); }
        if (nn > 0) { std::memcpy(h + (size_t)t.nodes * 4, kf_fvs[k].node_ids, (size_t)nn * 4); std::memcpy(h + (size_t)t.off * 4, kf_fvs[k].offsets, (size_t)(nn + 1) * 4); }
        if (ne > 0) std::memcpy(h + (size_t)t.idx * 4, kf_fvs[k].indices, (size_t)ne * 4);
    }
    HIP_TRY(hipMemcpyAsync(m->dBow, m->hBow, used, hipMemcpyHostToDevice, nullptr));
    int32_t *dOut = reinterpret_cast<int32_t *>(m->dBowOut);
    HIP_TRY(hipMemsetAsync(dOut, 0xFF, (size_t)K * nf * 4, nullptr));                              // matches = -1
    HIP_TRY(hipMemsetAsync(dOut + (size_t)K * nf, 0, ((size_t)K + 1 + (size_t)K * 32) * 4, nullptr));   // counts, error word, histograms
    BowBatch B;
    B.blk = reinterpret_cast<const uint32_t *>(m->dBow);
    B.K = K; B.nf = nf; B.nnF = nnF;
    B.fAngle = (int)(oFA / 4); B.fDesc = (int)(oFD / 4); B.fNodes = (int)(oFN / 4); B.fOff = (int)(oFO / 4); B.fIdx = (int)(oFI / 4); B.kfTable = (int)(oT / 4);
    B.matches = dOut; B.nmatch = dOut + (size_t)K * nf; B.err = B.nmatch + K; B.hist = B.err + 1;
    B.rotBin = reinterpret_cast<int8_t *>(B.hist + (size_t)K * 32);
    B.nnratio = nnratio; B.checkOri = check_orientation;
    if (maxNodes > 0) hipLaunchKernelGGL(k_bow_batch_match, dim3((maxNodes + 15) / 16, K), dim3(256), 0, nullptr, B);
    hipLaunchKernelGGL(k_bow_batch_finish, dim3(K), dim3(256), 0, nullptr, B);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(m->hBowOut, dOut, outInts * 4, hipMemcpyDeviceToHost));
    const int32_t *ho = reinterpret_cast<const int32_t *>(m->hBowOut);
    if (ho[(size_t)K * nf + K] & 1) {
        // a FeatureVector node of the frame holds more than 512 features (k_bow_batch_match keeps a node's "taken" flags in one 32-bit mask per
        // lane of a 16-lane group): shallow vocabularies or levelsup near L.  The results must still be those of K single searches, so run them.
        for (int k = 0; k < K; k++) {
            const int rc1 = rumi_search_by_bow(m, &KFs[k], &kf_fvs[k], kf_mp[k], nmp[k], mp_bad[k], F, f_fv, nnratio, check_orientation,
                                               matches + (size_t)k * nf, &nmatches_out[k]);
            if (rc1 != RUMI_OK) return rc1;
        }
        return RUMI_OK;
    }
    std::memcpy(matches, ho, (size_t)K * nf * 4);
    std::memcpy(nmatches_out, ho + (size_t)K * nf, (size_t)K * 4);
    return RUMI_OK;
}

extern "C" int rumi_search_by_bow_kf(RumiMatcher *m, const RumiFrameFeatures *KF1, const RumiFeatureVector *fv1, const int32_t *kf1_mp,
                                     const RumiFrameFeatures *KF2, const RumiFeatureVector *fv2, const int32_t *kf2_mp, int32_t nmp,
                                     const uint8_t *mp_bad, float nnratio, int32_t check_orientation, int32_t *matches12,
                                     int32_t *nmatches_out) {
    if (!m || !KF1 || !KF2 || !fv1 || !fv2 || !kf1_mp || !kf2_mp || !matches12 || !nmatches_out || nmp < 0) return RUMI_E_INVALID;
    const int nqe = fv1->n_nodes > 0 ? fv1->offsets[fv1->n_nodes] : 0, nfe = fv2->n_nodes > 0 ? fv2->offsets[fv2->n_nodes] : 0;
    if (KF1->n > m->maxQ || nqe > m->maxQ || nmp > m->maxQ || fv1->n_nodes > m->maxQ || nfe > m->maxFeat || fv2->n_nodes > m->maxFeat) {
        g_lastError = "SearchByBoW(KF,KF): sizes exceed the matcher's capacities";
        return RUMI_E_CAPACITY;
    }
    HIP_TRY(hipSetDevice(m->device));
    FrameDev fd;
    int rc = upload_frame(m, KF2, &fd);
    if (rc != RUMI_OK) return rc;
    // a KF2 feature is a candidate only if it holds a good map point (:732-736): everything else starts blocked
    std::vector<uint8_t> blocked(std::max(KF2->n, 1)), kf1bad(std::max(nmp, 1), 0);
    for (int f = 0; f < KF2->n; f++) blocked[f] = kf2_mp[f] < 0 || kf2_mp[f] >= nmp || mp_bad[kf2_mp[f]];
    if (KF2->n > 0) H2D(m->dU8b, blocked.data(), KF2->n);
    if (KF1->n > 0) { H2D(m->dQKeys, KF1->keys_un, KF1->n); H2D(m->dQDesc, KF1->desc, (size_t)KF1->n * 32); H2D(m->dI[0], kf1_mp, KF1->n); }
    if (nmp > 0) H2D(m->dU8a, mp_bad, nmp);
    if (fv1->n_nodes > 0) { H2D(m->dNodesA, fv1->node_ids, fv1->n_nodes); H2D(m->dOffA, fv1->offsets, fv1->n_nodes + 1); }
    if (nqe > 0) H2D(m->dIdxA, fv1->indices, nqe);
    if (fv2->n_nodes > 0) { H2D(m->dNodesB, fv2->node_ids, fv2->n_nodes); H2D(m->dOffB, fv2->offsets, fv2->n_nodes + 1); }
    if (nfe > 0) H2D(m->dFvIdx, fv2->indices, nfe);
    m->gridPending = false;
    FLUSH(m);
    if (fv1->n_nodes > 0) launch_queries_bow(m, nqe, fv1->n_nodes, fv2->n_nodes, nullptr, nullptr);
    std::vector<int32_t> assign(std::max(nqe, 1), -1);
    rc = run_search(m, MODE_BOW_KF, nqe, fd, m->dQDesc, nullptr, nnratio, check_orientation, nullptr, nmatches_out, m->dU8b, 0.f, 0, assign.data());
    if (rc != RUMI_OK) return rc;
    for (int i = 0; i < KF1->n; i++) matches12[i] = -1;
    for (int p = 0; p < nqe; p++) if (assign[p] >= 0) matches12[fv1->indices[p]] = assign[p];
    return RUMI_OK;
}

extern "C" int rumi_search_for_triangulation(RumiMatcher *m, const RumiFrameFeatures *KF1, const RumiFeatureVector *fv1, const int32_t *kf1_mp,
                                             const RumiFrameFeatures *KF2, const RumiFeatureVector *fv2, const int32_t *kf2_mp,
                                             const float *F12, const float *epipole2, int32_t only_stereo, int32_t coarse,
                                             int32_t check_orientation, int32_t *matches12, int32_t *nmatches_out) {
    if (!m || !KF1 || !KF2 || !fv1 || !fv2 || !F12 || !epipole2 || !nmatches_out) return RUMI_E_INVALID;
    if ((KF1->n > 0 && (!kf1_mp || !matches12)) || (KF2->n > 0 && !kf2_mp)) return RUMI_E_INVALID;
    const int nqe = fv1->n_nodes > 0 ? fv1->offsets[fv1->n_nodes] : 0, nfe = fv2->n_nodes > 0 ? fv2->offsets[fv2->n_nodes] : 0;
    if (KF1->n > m->maxQ || nqe > m->maxQ || fv1->n_nodes > m->maxQ || nfe > m->maxFeat || fv2->n_nodes > m->maxFeat) {
        g_lastError = "SearchForTriangulation: sizes exceed the matcher's capacities";
        return RUMI_E_CAPACITY;
    }
    for (int i = 0; i < KF1->n; i++) matches12[i] = -1;
    *nmatches_out = 0;
    // monocular key-frames have no stereo key-points (mvuRight < 0): bOnlyStereo skips every pair (:874-876)
    if (only_stereo || nqe == 0 || nfe == 0 || KF2->n == 0) return RUMI_OK;
    HIP_TRY(hipSetDevice(m->device));
    FrameDev fd;
    int rc = upload_frame(m, KF2, &fd);
    if (rc != RUMI_OK) return rc;
    float geom[11];
    std::memcpy(geom, F12, 36); std::memcpy(geom + 9, epipole2, 8);
    H2D(m->dPose, geom, 11);
    H2D(m->dFeatMp, kf2_mp, KF2->n);
    H2D(m->dQKeys, KF1->keys_un, KF1->n); H2D(m->dQDesc, KF1->desc, (size_t)KF1->n * 32); H2D(m->dI[0], kf1_mp, KF1->n);
    H2D(m->dNodesA, fv1->node_ids, fv1->n_nodes); H2D(m->dOffA, fv1->offsets, fv1->n_nodes + 1); H2D(m->dIdxA, fv1->indices, nqe);
    H2D(m->dNodesB, fv2->node_ids, fv2->n_nodes); H2D(m->dOffB, fv2->offsets, fv2->n_nodes + 1); H2D(m->dFvIdx, fv2->indices, nfe);
    TriArgs A{fv1->n_nodes, fv2->n_nodes, m->dNodesA, m->dOffA, m->dIdxA, m->dNodesB, m->dOffB, m->dFvIdx, m->dQKeys, m->dKeys,
              m->dQDesc, m->dDesc, m->dI[0], m->dFeatMp, m->dScale, m->dPose, coarse, m->dAssign};
    FLUSH(m);
    hipLaunchKernelGGL(k_tri_match, dim3((fv1->n_nodes + 63) / 64), dim3(64), 0, nullptr, A);
    hipLaunchKernelGGL(k_tri_filter, dim3(1), dim3(256), 0, nullptr, nqe, m->dIdxA, m->dQKeys, m->dKeys, m->dAssign, check_orientation, m->dNmatches);
    HIP_TRY(hipGetLastError());
    rc = fetch_results(m, 0, nqe, true);
    if (rc != RUMI_OK) return rc;
    *nmatches_out = m->hOut[0];
    const int32_t *assign = m->hOut + 4 + m->maxFeat;
    for (int p = 0; p < nqe; p++) if (assign[p] >= 0) matches12[fv1->indices[p]] = assign[p];
    return RUMI_OK;
}

extern "C" int rumi_search_by_projection_sim3(RumiMatcher *m, const RumiFrameFeatures *KF, float log_scale_factor, const float *Tcw7,
                                              const float *Ow3, const float *K4, int32_t nmp, const uint8_t *skip, const float *mp_pos,
                                              const float *mp_normal, const float *mp_min_dist, const float *mp_max_dist,
                                              const uint8_t *mp_desc, int32_t th, float ratio_hamming, int32_t explicit_invz,
                                              int32_t *matched, int32_t *nmatches_out) {
    if (!m || !KF || !Tcw7 || !Ow3 || !K4 || !matched || !nmatches_out || nmp < 0) return RUMI_E_INVALID;
    if (nmp > m->maxQ) { g_lastError = "more candidate points than max_queries"; return RUMI_E_CAPACITY; }
    HIP_TRY(hipSetDevice(m->device));
    FrameDev fd;
    int rc = upload_frame(m, KF, &fd);
    if (rc != RUMI_OK) return rc;
    std::vector<uint8_t> blocked(std::max(KF->n, 1));
    for (int f = 0; f < KF->n; f++) blocked[f] = matched[f] != -1;                 // vpMatched[idx] != NULL (:442)
    if (KF->n > 0) { H2D(m->dU8b, blocked.data(), KF->n); H2D(m->dFeatMp, matched, KF->n); }
    float pose[14];
    std::memcpy(pose, Tcw7, 28); std::memcpy(pose + 7, K4, 16); std::memcpy(pose + 11, Ow3, 12);
    H2D(m->dPose, pose, 14);
    if (nmp > 0) {
        H2D(m->dU8a, skip, nmp); H2D(m->dF[0], mp_pos, (size_t)nmp * 3); H2D(m->dF[1], mp_normal, (size_t)nmp * 3);
        H2D(m->dF[2], mp_min_dist, nmp); H2D(m->dF[3], mp_max_dist, nmp); H2D(m->dQDesc, mp_desc, (size_t)nmp * 32);
        FLUSH(m);
        hipLaunchKernelGGL(k_queries_sim3, dim3((nmp + 255) / 256), dim3(256), 0, nullptr, nmp, m->dU8a, m->dF[0], m->dF[1], m->dF[2], m->dF[3],
                           m->dPose, m->dScale, KF->nlevels, log_scale_factor, (float)th, explicit_invz, 1, 0, fd.minX, fd.minY, fd.maxX, fd.maxY, m->dQ);
    }
    return run_search(m, MODE_SIM3, nmp, fd, m->dQDesc, nullptr, 0.f, 0, matched, nmatches_out, m->dU8b, (float)RUMI_TH_LOW * ratio_hamming, 0);
}

extern "C" int rumi_fuse_candidates(RumiMatcher *m, const RumiFrameFeatures *KF, float log_scale_factor, const float *Tcw7, const float *Ow3,
                                    const float *K4, int32_t nmp, const uint8_t *skip, const float *mp_pos, const float *mp_normal,
                                    const float *mp_min_dist, const float *mp_max_dist, const uint8_t *mp_desc, float th,
                                    int32_t check_reprojection, int32_t *best_idx) {
    if (!m || !KF || !Tcw7 || !Ow3 || !K4 || nmp < 0 || (nmp > 0 && !best_idx)) return RUMI_E_INVALID;
    if (nmp > m->maxQ) { g_lastError = "more candidate points than max_queries"; return RUMI_E_CAPACITY; }
    if (nmp == 0) return RUMI_OK;
    HIP_TRY(hipSetDevice(m->device));
    FrameDev fd;
    int rc = upload_frame(m, KF, &fd);
    if (rc != RUMI_OK) return rc;
    HIP_TRY(hipMemsetAsync(m->dU8b, 0, std::max(KF->n, 1), nullptr));              // nothing is blocked: the points do not compete
    float pose[14];
    std::memcpy(pose, Tcw7, 28); std::memcpy(pose + 7, K4, 16); std::memcpy(pose + 11, Ow3, 12);
    H2D(m->dPose, pose, 14);
    H2D(m->dU8a, skip, nmp); H2D(m->dF[0], mp_pos, (size_t)nmp * 3); H2D(m->dF[1], mp_normal, (size_t)nmp * 3);
    H2D(m->dF[2], mp_min_dist, nmp); H2D(m->dF[3], mp_max_dist, nmp); H2D(m->dQDesc, mp_desc, (size_t)nmp * 32);
    FLUSH(m);
    hipLaunchKernelGGL(k_queries_sim3, dim3((nmp + 255) / 256), dim3(256), 0, nullptr, nmp, m->dU8a, m->dF[0], m->dF[1], m->dF[2], m->dF[3],
                       m->dPose, m->dScale, KF->nlevels, log_scale_factor, th, 0, 0, check_reprojection, fd.minX, fd.minY, fd.maxX, fd.maxY, m->dQ);
    int32_t n = 0;
    return run_search(m, MODE_FUSE, nmp, fd, m->dQDesc, nullptr, 0.f, 0, nullptr, &n, m->dU8b, 0.f, RUMI_TH_LOW, best_idx);
}

static int sim3_direction(RumiMatcher *m, const RumiFrameFeatures *KF, float logSf, const float *K4, int n, const uint8_t *skip, const float *pc,
                          const float *mn, const float *mx, const uint8_t *desc, float th, int32_t *best) {
    for (int i = 0; i < n; i++) best[i] = -1;
    if (n == 0) return RUMI_OK;
    FrameDev fd;
    int rc = upload_frame(m, KF, &fd);
    if (rc != RUMI_OK) return rc;
    HIP_TRY(hipMemsetAsync(m->dU8b, 0, std::max(KF->n, 1), nullptr));
    H2D(m->dPose, K4, 4);
    H2D(m->dU8a, skip, n); H2D(m->dF[0], pc, (size_t)n * 3); H2D(m->dF[2], mn, n); H2D(m->dF[3], mx, n); H2D(m->dQDesc, desc, (size_t)n * 32);
    FLUSH(m);
    hipLaunchKernelGGL(k_queries_campoints, dim3((n + 255) / 256), dim3(256), 0, nullptr, n, m->dU8a, m->dF[0], m->dF[2], m->dF[3], m->dPose, m->dScale,
                       KF->nlevels, logSf, th, fd.minX, fd.minY, fd.maxX, fd.maxY, m->dQ);
    int32_t cnt = 0;
    return run_search(m, MODE_FUSE, n, fd, m->dQDesc, nullptr, 0.f, 0, nullptr, &cnt, m->dU8b, 0.f, RUMI_TH_HIGH, best);
}

extern "C" int rumi_search_by_sim3(RumiMatcher *m, const RumiFrameFeatures *KF1, const RumiFrameFeatures *KF2, const float *K4,
                                   float log_scale_factor, const uint8_t *skip1, const float *pc1_in2, const float *min_dist1,
                                   const float *max_dist1, const uint8_t *desc1, const uint8_t *skip2, const float *pc2_in1,
                                   const float *min_dist2, const float *max_dist2, const uint8_t *desc2, float th, int32_t *match12,
                                   int32_t *nfound_out) {
    if (!m || !KF1 || !KF2 || !K4 || !nfound_out) return RUMI_E_INVALID;
    const int n1 = KF1->n, n2 = KF2->n;
    if (n1 < 0 || n2 < 0 || (n1 > 0 && (!skip1 || !pc1_in2 || !min_dist1 || !max_dist1 || !desc1 || !match12)) ||
        (n2 > 0 && (!skip2 || !pc2_in1 || !min_dist2 || !max_dist2 || !desc2)))
        return RUMI_E_INVALID;
    if (n1 > m->maxQ || n2 > m->maxQ) { g_lastError = "SearchBySim3: key-frame larger than max_queries"; return RUMI_E_CAPACITY; }
    HIP_TRY(hipSetDevice(m->device));
    std::vector<int32_t> vnMatch1(std::max(n1, 1)), vnMatch2(std::max(n2, 1));
    int rc = sim3_direction(m, KF2, log_scale_factor, K4, n1, skip1, pc1_in2, min_dist1, max_dist1, desc1, th, vnMatch1.data());
    if (rc != RUMI_OK) return rc;
    rc = sim3_direction(m, KF1, log_scale_factor, K4, n2, skip2, pc2_in1, min_dist2, max_dist2, desc2, th, vnMatch2.data());
    if (rc != RUMI_OK) return rc;
    int nFound = 0;                                                                 // check agreement, :1480-1493
    for (int i1 = 0; i1 < n1; i1++) {
        match12[i1] = -1;
        const int idx2 = vnMatch1[i1];
        if (idx2 >= 0 && vnMatch2[idx2] == i1) { match12[i1] = idx2; nFound++; }
    }
    *nfound_out = nFound;
    return RUMI_OK;
}

extern "C" int rumi_search_by_projection_reloc(RumiMatcher *m, const RumiFrameFeatures *Cur, float log_scale_factor, const float *Tcw7,
                                               const float *Ow3, const float *K4, const RumiKeyPoint *kf_keys, int32_t nkf,
                                               const int32_t *kf_mp, int32_t nmp, const uint8_t *skip, const float *mp_pos,
                                               const float *mp_min_dist, const float *mp_max_dist, const uint8_t *mp_desc, float th,
                                               int32_t orb_dist, int32_t check_orientation, int32_t *cur_mp, int32_t *nmatches_out) {
    if (!m || !Cur || !Tcw7 || !Ow3 || !K4 || !cur_mp || !nmatches_out || nkf < 0 || nmp < 0) return RUMI_E_INVALID;
    if (nkf > m->maxQ || nmp > m->maxQ) { g_lastError = "more key-frame features / map points than max_queries"; return RUMI_E_CAPACITY; }
    HIP_TRY(hipSetDevice(m->device));
    FrameDev fd;
    int rc = upload_frame(m, Cur, &fd);
    if (rc != RUMI_OK) return rc;
    std::vector<uint8_t> blocked(std::max(Cur->n, 1));
    for (int f = 0; f < Cur->n; f++) blocked[f] = cur_mp[f] >= 0;                  // CurrentFrame.mvpMapPoints[i2] != NULL (:1746)
    if (Cur->n > 0) { H2D(m->dU8b, blocked.data(), Cur->n); H2D(m->dFeatMp, cur_mp, Cur->n); }
    float pose[14];
    std::memcpy(pose, Tcw7, 28); std::memcpy(pose + 7, K4, 16); std::memcpy(pose + 11, Ow3, 12);
    H2D(m->dPose, pose, 14);
    if (nmp > 0) {
        H2D(m->dU8a, skip, nmp); H2D(m->dF[0], mp_pos, (size_t)nmp * 3); H2D(m->dF[2], mp_min_dist, nmp); H2D(m->dF[3], mp_max_dist, nmp);
        H2D(m->dQDesc, mp_desc, (size_t)nmp * 32);
    }
    if (nkf > 0) {
        H2D(m->dQKeys, kf_keys, nkf); H2D(m->dI[0], kf_mp, nkf);
        FLUSH(m);
        hipLaunchKernelGGL(k_queries_reloc, dim3((nkf + 255) / 256), dim3(256), 0, nullptr, nkf, m->dQKeys, m->dI[0], m->dU8a, m->dF[0], m->dF[2],
                           m->dF[3], m->dPose, m->dScale, Cur->nlevels, log_scale_factor, th, fd.minX, fd.minY, fd.maxX, fd.maxY, m->dQ);
    }
    return run_search(m, MODE_RELOC, nkf, fd, m->dQDesc, nullptr, 0.f, check_orientation, cur_mp, nmatches_out, m->dU8b, 0.f, orb_dist);
}

extern "C" int rumi_search_for_initialization(RumiMatcher *m, const RumiFrameFeatures *F1, const RumiFrameFeatures *F2,
                                              float *prev_matched, int32_t window_size, float nnratio, int32_t check_orientation,
                                              int32_t *matches12, int32_t *nmatches_out) {
    if (!m || !F1 || !F2 || !nmatches_out || F1->n < 0) return RUMI_E_INVALID;
    if (F1->n > m->maxQ) { g_lastError = "more F1 key-points than max_queries"; return RUMI_E_CAPACITY; }
    if (F1->n > 0 && (!prev_matched || !matches12 || !F1->keys_un || !F1->desc)) return RUMI_E_INVALID;
    HIP_TRY(hipSetDevice(m->device));
    FrameDev fd;
    int rc = upload_frame(m, F2, &fd);
    if (rc != RUMI_OK) return rc;
    const int n1 = F1->n;
    *nmatches_out = 0;
    if (n1 == 0) return RUMI_OK;
    H2D(m->dQKeys, F1->keys_un, n1); H2D(m->dQDesc, F1->desc, (size_t)n1 * 32); H2D(m->dF[0], prev_matched, (size_t)n1 * 2);
    FLUSH(m);
    hipLaunchKernelGGL(k_queries_init, dim3((n1 + 255) / 256), dim3(256), 0, nullptr, n1, m->dQKeys, m->dF[0], (float)window_size, m->dQ);
    for (int attempt = 0; attempt < 2; attempt++) {
        rc = build_lists(m, MODE_INIT, n1, fd, m->dQDesc, attempt > 0, false);
        if (rc != RUMI_OK) return rc;
        InitArgs A{n1, fd.n, m->dQ, m->dCounts, m->dOffsets, m->dLists, fd.keys, m->dAssign, m->dF[0], m->dNmatches, nnratio, check_orientation,
                   m->dOverflow};
        hipLaunchKernelGGL(k_resolve_init, dim3(1), dim3(64), (size_t)std::max(fd.n, 1) * 2 * sizeof(int32_t), nullptr, A);
        HIP_TRY(hipGetLastError());
        rc = fetch_results(m, 0, n1, true);
        if (rc != RUMI_OK) return rc;
        if (m->hOut[1] == 0) break;
        if (attempt == 1) { g_lastError = "candidate list arena overflow after growing"; return RUMI_E_CAPACITY; }
        rc = grow_lists(m, (size_t)m->hOut[1]);
        if (rc != RUMI_OK) return rc;
    }
    *nmatches_out = m->hOut[0];
    std::memcpy(matches12, m->hOut + 4 + m->maxFeat, (size_t)n1 * sizeof(int32_t));
    HIP_TRY(hipMemcpy(prev_matched, m->dF[0], (size_t)n1 * 2 * sizeof(float), hipMemcpyDeviceToHost));
    return RUMI_OK;
}

extern "C" int rumi_frame_is_in_frustum(RumiMatcher *m, const float *Rcw9, const float *tcw3, const float *Ow3, const float *K4,
                                        float min_x, float min_y, float max_x, float max_y, float log_scale_factor, int32_t nlevels,
                                        float viewing_cos_limit, int32_t nmp, const float *mp_pos, const float *mp_normal,
                                        const float *mp_min_dist, const float *mp_max_dist, uint8_t *track_in_view, float *proj_x,
                                        float *proj_y, int32_t *scale_level, float *view_cos, float *track_depth) {
    if (!m || !Rcw9 || !tcw3 || !Ow3 || !K4 || nmp < 0) return RUMI_E_INVALID;
    if (nmp > m->maxQ) { g_lastError = "more map points than max_queries"; return RUMI_E_CAPACITY; }
    if (nmp == 0) return RUMI_OK;
    if (!mp_pos || !mp_normal || !mp_min_dist || !mp_max_dist || !track_in_view || !proj_x || !proj_y || !scale_level || !view_cos || !track_depth)
        return RUMI_E_INVALID;
    HIP_TRY(hipSetDevice(m->device));
    reset_uploads(m);
    float pose[19];
    std::memcpy(pose, Rcw9, 36); std::memcpy(pose + 9, tcw3, 12); std::memcpy(pose + 12, Ow3, 12); std::memcpy(pose + 15, K4, 16);
    H2D(m->dPose, pose, 19);
    H2D(m->dF[0], mp_pos, (size_t)nmp * 3); H2D(m->dF[1], mp_normal, (size_t)nmp * 3); H2D(m->dF[2], mp_min_dist, nmp); H2D(m->dF[3], mp_max_dist, nmp);
    // outputs are packed into the upload mirror (its contents have been scattered by then) and come back with one copy
    const size_t n16 = ((size_t)nmp + 15) & ~(size_t)15;
    if (n16 * 21 > m->stageCap) { g_lastError = "isInFrustum: result block exceeds the staging block"; return RUMI_E_CAPACITY; }
    uint8_t *dIn = m->dStage;
    float *dX = reinterpret_cast<float *>(m->dStage + n16), *dY = dX + n16, *dC = dY + n16, *dD = dC + n16;
    int32_t *dL = reinterpret_cast<int32_t *>(dD + n16);
    FLUSH(m);
    hipLaunchKernelGGL(k_is_in_frustum, dim3((nmp + 255) / 256), dim3(256), 0, nullptr, nmp, m->dPose, min_x, min_y, max_x, max_y, log_scale_factor,
                       nlevels, viewing_cos_limit, m->dF[0], m->dF[1], m->dF[2], m->dF[3], dIn, dX, dY, dL, dC, dD);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(m->hStage, m->dStage, n16 * 21, hipMemcpyDeviceToHost));
    const uint8_t *h = m->hStage;
    std::memcpy(track_in_view, h, (size_t)nmp);
    std::memcpy(proj_x, h + n16, (size_t)nmp * 4); std::memcpy(proj_y, h + n16 * 5, (size_t)nmp * 4);
    std::memcpy(view_cos, h + n16 * 9, (size_t)nmp * 4); std::memcpy(track_depth, h + n16 * 13, (size_t)nmp * 4);
    std::memcpy(scale_level, h + n16 * 17, (size_t)nmp * 4);
    return RUMI_OK;
}

extern "C" int rumi_search_local_points(RumiMatcher *m, const RumiFrameFeatures *F, const float *Rcw9, const float *tcw3, const float *Ow3,
                                        const float *K4, float log_scale_factor, int32_t nlevels, float viewing_cos_limit, int32_t nmp,
                                        const uint8_t *skip, const float *mp_pos, const float *mp_normal, const float *mp_min_dist,
                                        const float *mp_max_dist, const uint8_t *mp_desc, const int32_t *mp_obs, float th, int32_t far_points,
                                        float th_far_points, float nnratio, uint8_t *track_in_view, float *proj_x, float *proj_y,
                                        int32_t *scale_level, float *view_cos, float *track_depth, int32_t *n_to_match_out, int32_t *frame_mp,
                                        int32_t *nmatches_out) {
    if (!m || !F || !Rcw9 || !tcw3 || !Ow3 || !K4 || !nmatches_out || !n_to_match_out || !frame_mp || nmp < 0) return RUMI_E_INVALID;
    *nmatches_out = 0; *n_to_match_out = 0;
    if (nmp > m->maxQ) { g_lastError = "more map points than max_queries"; return RUMI_E_CAPACITY; }
    if (nmp == 0) return RUMI_OK;                          // nToMatch == 0: the reference does not search (Tracking.cc:3032)
    if (!skip || !mp_pos || !mp_normal || !mp_min_dist || !mp_max_dist || !mp_desc || !mp_obs || !track_in_view || !proj_x || !proj_y || !scale_level ||
        !view_cos || !track_depth)
        return RUMI_E_INVALID;
    HIP_TRY(hipSetDevice(m->device));
    FrameDev fd;
    int rc = upload_frame(m, F, &fd);
    if (rc != RUMI_OK) return rc;
    if (F->n > 0) H2D(m->dFeatMp, frame_mp, F->n);
    float pose[19];
    std::memcpy(pose, Rcw9, 36); std::memcpy(pose + 9, tcw3, 12); std::memcpy(pose + 12, Ow3, 12); std::memcpy(pose + 15, K4, 16);
    H2D(m->dPose, pose, 19);
    H2D(m->dF[0], mp_pos, (size_t)nmp * 3); H2D(m->dF[1], mp_normal, (size_t)nmp * 3); H2D(m->dF[2], mp_min_dist, nmp); H2D(m->dF[3], mp_max_dist, nmp);
    H2D(m->dU8b, skip, nmp); H2D(m->dI[1], mp_obs, nmp); H2D(m->dQDesc, mp_desc, (size_t)nmp * 32);
    // the frustum test writes the six per-point fields into the (by then scattered) upload mirror; the query kernel reads them there and the
    // same block travels back to the host for the facade's write-back: no host round trip between isInFrustum and SearchByProjection
    const size_t n16 = ((size_t)nmp + 15) & ~(size_t)15;
    if (n16 * 21 > m->stageCap) { g_lastError = "SearchLocalPoints: result block exceeds the staging block"; return RUMI_E_CAPACITY; }
    uint8_t *dIn = m->dStage;
    float *dX = reinterpret_cast<float *>(m->dStage + n16), *dY = dX + n16, *dC = dY + n16, *dD = dC + n16;
    int32_t *dL = reinterpret_cast<int32_t *>(dD + n16);
    FLUSH(m);
    hipLaunchKernelGGL(k_is_in_frustum, dim3((nmp + 255) / 256), dim3(256), 0, nullptr, nmp, m->dPose, fd.minX, fd.minY, fd.maxX, fd.maxY, log_scale_factor,
                       nlevels, viewing_cos_limit, m->dF[0], m->dF[1], m->dF[2], m->dF[3], dIn, dX, dY, dL, dC, dD, m->dU8b);
    HIP_TRY(hipMemcpyAsync(m->hStage, m->dStage, n16 * 21, hipMemcpyDeviceToHost, nullptr));
    // is_bad of SearchByProjection = skip: a skipped point is never in view, so the flag is only read for points that are not bad
    hipLaunchKernelGGL(k_queries_mappoints, dim3((nmp + 255) / 256), dim3(256), 0, nullptr, nmp, dIn, dX, dY, dL, dC, dD, m->dU8b, m->dI[1], m->dScale, th,
                       far_points, th_far_points, m->dQ);
    rc = run_search(m, MODE_MAPPOINTS, nmp, fd, m->dQDesc, m->dI[1], nnratio, 0, frame_mp, nmatches_out);
    if (rc != RUMI_OK) return rc;
    const uint8_t *h = m->hStage;                           // complete: run_search synchronised the stream
    std::memcpy(track_in_view, h, (size_t)nmp);
    std::memcpy(proj_x, h + n16, (size_t)nmp * 4); std::memcpy(proj_y, h + n16 * 5, (size_t)nmp * 4);
    std::memcpy(view_cos, h + n16 * 9, (size_t)nmp * 4); std::memcpy(track_depth, h + n16 * 13, (size_t)nmp * 4);
    std::memcpy(scale_level, h + n16 * 17, (size_t)nmp * 4);
    int nTo = 0;
    for (int i = 0; i < nmp; i++) nTo += track_in_view[i];
    *n_to_match_out = nTo;
    if (nTo == 0) *nmatches_out = 0;                       // (nothing in view: no query was live, the search found nothing)
    return RUMI_OK;
}

extern "C" int rumi_match_bruteforce_batch_device_strided(const void *d_query, const void *d_nq, const void *d_train, const void *d_nt,
                                                          int32_t count_stride, int64_t query_stride, int64_t train_stride, int32_t cap, int32_t nbatch,
                                                          void *d_best_idx, void *d_best_dist, void *d_second_dist, void *hip_stream) {
    if (!d_query || !d_nq || !d_train || !d_nt || !d_best_idx || !d_best_dist || !d_second_dist || cap < 1 || cap > 65535 || nbatch < 1 || count_stride < 1 ||
        query_stride < 32ll * cap || train_stride < 32ll * cap || (query_stride & 3) || (train_stride & 3) ||
        (reinterpret_cast<uintptr_t>(d_query) & 3) || (reinterpret_cast<uintptr_t>(d_train) & 3))
        return RUMI_E_INVALID;                                 // the kernel packs the train index into 16 bits next to the distance
    return launch_bruteforce(d_query, d_nq, d_train, d_nt, count_stride, (long long)query_stride, (long long)train_stride, cap, nbatch, d_best_idx, d_best_dist,
                             d_second_dist, 0, (hipStream_t)hip_stream);
}

extern "C" int rumi_match_bruteforce_ring_device(const void *d_desc, const void *d_n, int32_t count_stride, int64_t frame_stride, int32_t cap, int32_t nframes,
                                                 void *d_best_idx, void *d_best_dist, void *d_second_dist, void *hip_stream) {
    if (!d_desc || !d_n || !d_best_idx || !d_best_dist || !d_second_dist || cap < 1 || cap > 65535 || nframes < 1 || count_stride < 1 ||
        frame_stride < 32ll * cap || (frame_stride & 3) || (reinterpret_cast<uintptr_t>(d_desc) & 3))
        return RUMI_E_INVALID;
    return launch_bruteforce(d_desc, d_n, d_desc, d_n, count_stride, (long long)frame_stride, (long long)frame_stride, cap, nframes, d_best_idx, d_best_dist,
                             d_second_dist, nframes, (hipStream_t)hip_stream);
}

extern "C" int rumi_match_bruteforce_batch_device(const void *d_query, const void *d_nq, const void *d_train, const void *d_nt,
                                                  int32_t count_stride, int32_t cap, int32_t nbatch, void *d_best_idx,
                                                  void *d_best_dist, void *d_second_dist, void *hip_stream) {
    return rumi_match_bruteforce_batch_device_strided(d_query, d_nq, d_train, d_nt, count_stride, 32ll * cap, 32ll * cap, cap, nbatch, d_best_idx, d_best_dist,
                                                      d_second_dist, hip_stream);
}
