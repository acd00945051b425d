// Device helpers the matcher kernels (match.hip and its match_*.inc parts: queries, candidates, resolve, tri, bow_batch, reloc_batch), the Tracking
// step (track.hip) and the mapping kernels (mapping.hip) share, among them the one body of every projection gate that has more than one caller, of
// ComputeThreeMaxima in its serial and its one-wave form, of the finish of a batched SearchByBoW, and of the ordered compaction of a workgroup.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "rumi_match.h"

namespace rumi {

__device__ __forceinline__ int hamming256(const uint32_t q[8], const uint32_t *d) {
    int s = 0;
#pragma unroll
    for (int k = 0; k < 8; k++) s += __popc(q[k] ^ d[k]);
    return s;
}
__device__ __forceinline__ int hamming256(const uint4 &q0, const uint4 &q1, const uint4 &d0, const uint4 &d1) {   // two rows held as 16-byte halves
    return __popc(q0.x ^ d0.x) + __popc(q0.y ^ d0.y) + __popc(q0.z ^ d0.z) + __popc(q0.w ^ d0.w) +
           __popc(q1.x ^ d1.x) + __popc(q1.y ^ d1.y) + __popc(q1.z ^ d1.z) + __popc(q1.w ^ d1.w);
}

// inclusive prefix sum over the lanes of a wave by DPP (row prefix, row_bcast:15, row_bcast:31); lane 63 holds the total
__device__ __forceinline__ int wave_scan_incl_i32(int v) {
#define RUMI_DPP_ADD(ctl, rows) v += __builtin_amdgcn_update_dpp(0, v, ctl, rows, 0xf, false)
    RUMI_DPP_ADD(0x111, 0xf); RUMI_DPP_ADD(0x112, 0xf); RUMI_DPP_ADD(0x114, 0xf); RUMI_DPP_ADD(0x118, 0xf);
    RUMI_DPP_ADD(0x142, 0xa); RUMI_DPP_ADD(0x143, 0xc);
#undef RUMI_DPP_ADD
    return v;
}

__device__ __forceinline__ int rot_bin(float a, float b) {          // ORBmatcher.cc:1592-1599
    const float factor = 1.0f / RUMI_HISTO_LENGTH;
    float rot = a - b;
    if (rot < 0.0f) rot += 360.0f;
    int bin = (int)__builtin_roundf(rot * factor);
    if (bin == RUMI_HISTO_LENGTH) bin = 0;
    return bin;
}

// wave-wide maximum / sum of one 32-bit value by DPP (row prefix, row_bcast:15, row_bcast:31; the total sits in lane 63)
__device__ __forceinline__ uint32_t wave_max_u32(uint32_t v) {
#define RUMI_DPP_MAX(ctl, rows) v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, ctl, rows, 0xf, false))
    RUMI_DPP_MAX(0x111, 0xf); RUMI_DPP_MAX(0x112, 0xf); RUMI_DPP_MAX(0x114, 0xf); RUMI_DPP_MAX(0x118, 0xf);
    RUMI_DPP_MAX(0x142, 0xa); RUMI_DPP_MAX(0x143, 0xc);
#undef RUMI_DPP_MAX
    return (uint32_t)__builtin_amdgcn_readlane((int)v, 63);
}
__device__ __forceinline__ int wave_sum_i32(int v) { return __builtin_amdgcn_readlane(wave_scan_incl_i32(v), 63); }

// ORBmatcher::ComputeThreeMaxima (ORBmatcher.cc:1795-1826) and the filter around it, in its two forms.  Neither is converted into the other: one
// thread against one wave is a speed choice of the kernel that calls it.
// Serial form, called by ONE thread: the scan of the 30 bins with its strict comparisons, the two 0.1f cuts in float, keep[bin] = bin is one of the three.
__device__ __forceinline__ void three_maxima_keep(const int *hist, int *keep) {
    int max1 = 0, max2 = 0, max3 = 0, ind1 = -1, ind2 = -1, ind3 = -1;
    for (int i = 0; i < RUMI_HISTO_LENGTH; i++) {
        const int s = hist[i];
        if (s > max1) { max3 = max2; max2 = max1; max1 = s; ind3 = ind2; ind2 = ind1; ind1 = i; }
        else if (s > max2) { max3 = max2; max2 = s; ind3 = ind2; ind2 = i; }
        else if (s > max3) { max3 = s; ind3 = i; }
    }
    if ((float)max2 < 0.1f * (float)max1) { ind2 = -1; ind3 = -1; }
    else if ((float)max3 < 0.1f * (float)max1) ind3 = -1;
    for (int i = 0; i < RUMI_HISTO_LENGTH; i++) keep[i] = (i == ind1 || i == ind2 || i == ind3);
}
// One-wave form, called by the first wave of a workgroup with s = its lane's bin count (0 from lane 30 on): the scan keeps the three largest counts
// ordered by (count descending, bin ascending) and empty bins never enter, which is three maxima of (count << 6 | 63 - bin).  Returns the lane's
// keep flag; *removed: the entries of the bins that go.  Without useHist every bin stays.
__device__ __forceinline__ int three_maxima_wave(int s, bool useHist, int *removed) {
    const int lane = threadIdx.x;
    int keep = 1;
    *removed = 0;
    if (useHist) {
        uint32_t key = s > 0 ? ((uint32_t)s << 6) | (uint32_t)(63 - lane) : 0u;
        const uint32_t k1 = wave_max_u32(key);
        if (key == k1) key = 0;
        const uint32_t k2 = wave_max_u32(key);
        if (key == k2) key = 0;
        const uint32_t k3 = wave_max_u32(key);
        const int max1 = (int)(k1 >> 6), max2 = (int)(k2 >> 6), max3 = (int)(k3 >> 6);
        int ind1 = k1 ? 63 - (int)(k1 & 63) : -1, ind2 = k2 ? 63 - (int)(k2 & 63) : -1, ind3 = k3 ? 63 - (int)(k3 & 63) : -1;
        if ((float)max2 < 0.1f * (float)max1) { ind2 = -1; ind3 = -1; }
        else if ((float)max3 < 0.1f * (float)max1) ind3 = -1;
        keep = (lane == ind1 || lane == ind2 || lane == ind3);
        *removed = wave_sum_i32(keep ? 0 : s);
    }
    return keep;
}
// The end of a batched SearchByBoW, one workgroup of 256 per row of a [rows][n] match matrix: the matches whose rotBin the row's histogram rejects
// become -1, the others are counted.  (32 keep flags read with & 31: a bin is 0..29 for every finite angle, and no byte indexes past the array.)
__device__ __forceinline__ void bow_finish(int32_t *matches, const int8_t *rotBin, const int32_t *hist, int n, int checkOri, int32_t *count) {
    __shared__ int sKeep[32], sCount;
    const int tid = threadIdx.x;
    if (tid == 0) {
        sCount = 0;
        for (int i = 0; i < 32; i++) sKeep[i] = 1;
        if (checkOri) three_maxima_keep(hist, sKeep);
    }
    __syncthreads();
    int local = 0;
    for (int f = tid; f < n; f += 256) {
        if (matches[f] < 0) continue;
        if (checkOri && !sKeep[rotBin[f] & 31]) matches[f] = -1; else local++;
    }
    if (local) atomicAdd(&sCount, local);
    __syncthreads();
    if (tid == 0) *count = sCount;
}

// One chunk of an ordered compaction by a workgroup of 1024: every thread brings a flag, the flagged ones get consecutive slots in thread order behind
// *sBase and call emit(slot), then *sBase advances by their number.  Three barriers: the wave counts; every slot taken (the emits run between the
// first two, where the sites had their stores) before thread 0 moves the base; the new base.
template <class Emit>
__device__ __forceinline__ void block_ordered_slot(bool flag, int *sCnt /* [16] */, int *sBase, Emit emit) {
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const unsigned long long b = __ballot(flag);
    if (lane == 0) sCnt[wave] = __popcll(b);
    __syncthreads();
    if (flag) {
        int slot = *sBase;
        for (int k = 0; k < wave; k++) slot += sCnt[k];
        emit(slot + __popcll(b & ((1ull << lane) - 1ull)));
    }
    __syncthreads();
    if (tid == 0) { int t = *sBase; for (int k = 0; k < 16; k++) t += sCnt[k]; *sBase = t; }
    __syncthreads();
}

struct Query {           // 48 bytes
    float u, v, r;       // window centre / half-size (MODE_BOW: unused)
    int32_t minLevel, maxLevel;
    int32_t valid;
    int32_t descId;      // row of the query descriptor in qDesc
    int32_t mpId;        // map point id this query assigns
    int32_t blocks;      // Observations() > 0: an assignment hides the feature from later queries
    int32_t c0, c1;      // MODE_BOW: candidate range in the frame's FeatureVector indices
    float angle;         // key-point angle on the query side (rotation histogram)
};

// SearchByProjection(F, map points): ORBmatcher.cc:44-71
__device__ __forceinline__ Query mappoint_query(int i, bool inView, float px, float py, int lvl, float viewCos, float depth, bool isBad, int obs,
                                                const float *scaleFactors, float th, int farPoints, float thFar) {
    Query o{};
    o.valid = inView && !(farPoints && depth > thFar) && !isBad;
    if (o.valid) {
        float r = (double)viewCos > 0.998 ? 2.5f : 4.0f;      // RadiusByViewingCos (float vs double literal)
        if ((double)th != 1.0) r *= th;
        o.u = px; o.v = py;
        o.r = r * scaleFactors[lvl];
        o.minLevel = lvl - 1; o.maxLevel = lvl;
    }
    o.descId = i; o.mpId = i; o.blocks = obs > 0;
    return o;
}

// MapPoint::PredictScale (MapPoint.cc:538-570); log in double (oracle/match_oracle.cc explains the choice)
__device__ __forceinline__ int predict_scale(float maxDistance, float dist, float logScaleFactor, int nLevels) {
    const float ratio = maxDistance / dist;
    int nScale = (int)ceil(log((double)ratio) / (double)logScaleFactor);
    if (nScale < 0) nScale = 0;
    else if (nScale >= nLevels) nScale = nLevels - 1;
    return nScale;
}

__device__ __forceinline__ void se3f_mul(const float *T, const float *p, float *o) {   // Sophus::SE3f * p (so3.hpp:358-367)
    const float qx = T[0], qy = T[1], qz = T[2], qw = T[3];
    float u0 = qy * p[2] - qz * p[1], u1 = qz * p[0] - qx * p[2], u2 = qx * p[1] - qy * p[0];
    u0 += u0; u1 += u1; u2 += u2;
    const float c0 = qy * u2 - qz * u1, c1 = qz * u0 - qx * u2, c2 = qx * u1 - qy * u0;
    o[0] = ((p[0] + qw * u0) + c0) + T[4]; o[1] = ((p[1] + qw * u1) + c1) + T[5]; o[2] = ((p[2] + qw * u2) + c2) + T[6];
}

// The projection and gates of one point for SearchByProjection(KeyFrame*, Sim3f&, points, ...) (ORBmatcher.cc:389-436, variant 0; :491-539,
// variant 1) and Fuse (:1058-1112): depth, KeyFrame::IsInImage, the distance range, the viewing angle, the predicted level and the window.
// One body for k_queries_sim3 (match_queries.inc) and the SearchInNeighbors kernels (search_in_neighbors.inc): their results are compared
// byte for byte.  The caller fills descId, mpId, blocks and c0.
__device__ __forceinline__ Query sim3_query(const float *p3Dw, const float *Pn, float minDist, float maxDist, const float *Tcw, const float *K,
                                            const float *Ow, const float *scaleFactors, int nLevels, float logScaleFactor, float th, int variant,
                                            float minX, float minY, float maxX, float maxY) {
    Query o{};
    float pc[3];
    se3f_mul(Tcw, p3Dw, pc);
    if (!(pc[2] < 0.0f)) {
        float u, v;
        if (variant == 0) { u = K[0] * pc[0] / pc[2] + K[2]; v = K[1] * pc[1] / pc[2] + K[3]; }
        else { const float invz = 1 / pc[2]; const float x = pc[0] * invz, y = pc[1] * invz; u = K[0] * x + K[2]; v = K[1] * y + K[3]; }
        if (u >= minX && u < maxX && v >= minY && v < maxY) {                       // KeyFrame::IsInImage
            const float maxD = 1.2f * maxDist, minD = 0.8f * minDist;
            const float P0 = p3Dw[0] - Ow[0], P1 = p3Dw[1] - Ow[1], P2 = p3Dw[2] - Ow[2];
            const float dist = sqrtf((P0 * P0 + P1 * P1) + P2 * P2);
            if (!(dist < minD || dist > maxD) && !((double)((P0 * Pn[0] + P1 * Pn[1]) + P2 * Pn[2]) < 0.5 * (double)dist)) {
                const int lvl = predict_scale(maxDist, dist, logScaleFactor, nLevels);
                o.valid = 1; o.u = u; o.v = v; o.r = th * scaleFactors[lvl];
                o.minLevel = lvl - 1; o.maxLevel = lvl;                              // the level test of :445-448 / :553-556
            }
        }
    }
    return o;
}

// Sophus::SE3f::inverse().translation(): conj(q) * (-t) by the quaternion's _transformVector, for Frame::UpdatePoseMatrices (pose_matrices19) and
// for a pose hypothesis of the relocalisation walk (match_reloc_batch.inc), which the facade forms with the same expression.
__device__ __forceinline__ void se3f_camera_centre(const float *T7, float *Ow) {
    const float qx = -T7[0], qy = -T7[1], qz = -T7[2], qw = T7[3];
    const float v0 = T7[4] * -1.f, v1 = T7[5] * -1.f, v2 = T7[6] * -1.f;
    float u0 = qy * v2 - qz * v1, u1 = qz * v0 - qx * v2, u2 = qx * v1 - qy * v0;
    u0 += u0; u1 += u1; u2 += u2;
    const float c0 = qy * u2 - qz * u1, c1 = qz * u0 - qx * u2, c2 = qx * u1 - qy * u0;
    Ow[0] = (v0 + qw * u0) + c0; Ow[1] = (v1 + qw * u1) + c1; Ow[2] = (v2 + qw * u2) + c2;
}

// The query of one key-frame feature for SearchByProjection(Frame&, KeyFrame*, sAlreadyFound, th, ORBdist) (ORBmatcher.cc:1700-1733): no depth
// test, the closed rectangle that lets a NaN projection through, the distance on xw - Ow, levels [L - 1, L + 1].  One body for k_queries_reloc
// (match_queries.inc) and k_reloc_walk<false> (match_reloc_batch.inc).  mp: the feature's map point (< 0: none); skip: the caller's
// "bad or already found", read only where mp >= 0.  The angle is the key-frame feature's, kept whether or not the point is searched.
__device__ __forceinline__ Query reloc_query(int mp, bool skip, const float *mpPos, const float *mpMinDist, const float *mpMaxDist, const float *Tcw,
                                             const float *K, const float *Ow, const float *scaleFactors, int nLevels, float logScaleFactor, float th,
                                             float minX, float minY, float maxX, float maxY, float angle) {
    Query o{};
    if (mp >= 0 && !skip) {
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
    o.angle = angle;
    return o;
}

// Correspondences of Optimizer::PoseOptimization(Frame*) (Optimizer.cc:749-815, mono): the features with a map point, in feature order.
// One workgroup of 1024 threads, ordered compaction (block_ordered_slot, chunks of 1024 features).  correspondence_store: feature i with point mp
// as correspondence c, also for the relocalisation's gather (track_reloc.inc).
__device__ __forceinline__ void correspondence_store(int c, int i, int mp, const RumiKeyPoint *__restrict__ keys, const float *__restrict__ mpPos,
                                                     const float *__restrict__ invSigma2, float *Xw, float *obs, float *w, int32_t *idx) {
    Xw[3 * c] = mpPos[3 * mp]; Xw[3 * c + 1] = mpPos[3 * mp + 1]; Xw[3 * c + 2] = mpPos[3 * mp + 2];
    obs[2 * c] = keys[i].x; obs[2 * c + 1] = keys[i].y;
    w[c] = invSigma2[keys[i].octave];
    idx[c] = i;
}
__device__ __forceinline__ void gather_correspondences(int n, const RumiKeyPoint *__restrict__ keys, const int32_t *featMp, const float *__restrict__ mpPos,
                                                       const float *__restrict__ invSigma2, float *Xw, float *obs, float *w, int32_t *idx, int32_t *start,
                                                       int32_t *snapshot, int *sWave /* [16] */, int *sBase) {
    const int tid = threadIdx.x;
    if (tid == 0) *sBase = 0;
    __syncthreads();
    for (int c0 = 0; c0 < n; c0 += 1024) {
        const int i = c0 + tid;
        const int mp = i < n ? featMp[i] : -1;
        if (snapshot && i < n) snapshot[i] = mp;            // the frame's map-point vector as the search left it (the optimisation's outliers leave it next)
        block_ordered_slot(mp >= 0, sWave, sBase, [&](int c) { correspondence_store(c, i, mp, keys, mpPos, invSigma2, Xw, obs, w, idx); });
    }
    if (tid == 0) { start[0] = 0; start[1] = *sBase; }
}

// Frame::UpdatePoseMatrices (Frame.cc:522-528) in Sophus' / Eigen's float arithmetic: Rcw = q.toRotationMatrix(), tcw, Ow = conj(q) * (-tcw)
// (se3f_camera_centre), as [Rcw9 | tcw3 | Ow3 | K4] for the frustum test.
__device__ __forceinline__ void pose_matrices19(const float *Tcw7, const float *K4, float *pose19) {
    const float x = Tcw7[0], y = Tcw7[1], z = Tcw7[2], w = Tcw7[3];
    const float tx = 2.f * x, ty = 2.f * y, tz = 2.f * z;
    const float twx = tx * w, twy = ty * w, twz = tz * w, txx = tx * x, txy = ty * x, txz = tz * x, tyy = ty * y, tyz = tz * y, tzz = tz * z;
    pose19[0] = 1.f - (tyy + tzz); pose19[1] = txy - twz; pose19[2] = txz + twy;
    pose19[3] = txy + twz; pose19[4] = 1.f - (txx + tzz); pose19[5] = tyz - twx;
    pose19[6] = txz - twy; pose19[7] = tyz + twx; pose19[8] = 1.f - (txx + tyy);
    const float t0 = Tcw7[4], t1 = Tcw7[5], t2 = Tcw7[6];
    pose19[9] = t0; pose19[10] = t1; pose19[11] = t2;
    se3f_camera_centre(Tcw7, pose19 + 12);
    pose19[15] = K4[0]; pose19[16] = K4[1]; pose19[17] = K4[2]; pose19[18] = K4[3];
}

// Frame::isInFrustum (Frame.cc:558-617, mono) of one map point against [Rcw9 | tcw3 | Ow3 | K4]: depth sign, the closed image rectangle, the
// distance range, the viewing cosine, PredictScale.  One body for k_is_in_frustum (match_queries.inc) and the tracker's fused form (frustum_body,
// track.hip).  px, py stand once the rectangle passes; lvl, viewCos and depth (|Pc|) only for a point in view.  The distances and the normal are read
// where the chain reaches them, hence the pointers.
struct FrustumResult { uint8_t in; float px, py; int lvl; float viewCos, depth; };
__device__ __forceinline__ FrustumResult frustum_gate(const float *P, const float *Pn, const float *minDist, const float *maxDist, const float *pose19,
                                                      float minX, float minY, float maxX, float maxY, float logScaleFactor, int nLevels,
                                                      float viewingCosLimit) {
    const float *R = pose19, *t = pose19 + 9, *Ow = pose19 + 12, *K = pose19 + 15;
    FrustumResult o{0, -1, -1, 0, 0, 0};
    float Pc[3];
#pragma unroll
    for (int r = 0; r < 3; r++) Pc[r] = ((R[r * 3] * P[0] + R[r * 3 + 1] * P[1]) + R[r * 3 + 2] * P[2]) + t[r];
    const float Pc_dist = sqrtf((Pc[0] * Pc[0] + Pc[1] * Pc[1]) + Pc[2] * Pc[2]);
    if (!(Pc[2] < 0.0f)) {
        const float u = K[0] * Pc[0] / Pc[2] + K[2], v = K[1] * Pc[1] / Pc[2] + K[3];
        if (!(u < minX || u > maxX) && !(v < minY || v > maxY)) {
            o.px = u; o.py = v;
            const float maxD = 1.2f * *maxDist, minD = 0.8f * *minDist;
            const float P0 = P[0] - Ow[0], P1 = P[1] - Ow[1], P2 = P[2] - Ow[2];
            const float dist = sqrtf((P0 * P0 + P1 * P1) + P2 * P2);
            if (!(dist < minD || dist > maxD)) {
                const float viewCos = ((P0 * Pn[0] + P1 * Pn[1]) + P2 * Pn[2]) / dist;
                if (!(viewCos < viewingCosLimit)) {
                    o.lvl = predict_scale(*maxDist, dist, logScaleFactor, nLevels);
                    o.in = 1; o.depth = Pc_dist; o.viewCos = viewCos;
                }
            }
        }
    }
    return o;
}

}  // namespace rumi
