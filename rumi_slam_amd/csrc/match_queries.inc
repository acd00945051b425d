// Query builders of the matcher (one query per map point / last-frame feature / key-frame feature: projection, window, levels) and the frustum test.  (Included inside namespace rumi.)
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
    const int lo = fv_find_node(fNodes, nnF, kfNodes[a]);
    const bool hit = lo >= 0;
    Query o{};
    const int feat = (int)kfIdx[p];
    const int mp = kfMp[feat];
    o.valid = hit && mp >= 0 && !mpBad[mp];
    o.descId = feat; o.mpId = mp; o.blocks = 1;
    if (o.valid) { o.c0 = fOff[lo]; o.c1 = fOff[lo + 1]; }
    o.angle = kfKeys[feat].angle;
    q[p] = o;
}

// SearchByProjection(KeyFrame*, Sim3f&, points, ...): ORBmatcher.cc:389-436 (variant 0) / :491-539 (variant 1); the arithmetic is sim3_query's (match_device.h)
__global__ void k_queries_sim3(int nmp, const uint8_t *skip, const float *mpPos, const float *mpNormal, const float *mpMinDist,
                               const float *mpMaxDist, const float *pose /*Tcw7, K4, Ow3*/, const float *scaleFactors, int nLevels,
                               float logScaleFactor, float th, int variant, int blocks, int checkReproj, float minX, float minY, float maxX, float maxY,
                               Query *q) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nmp) return;
    Query o{};
    if (!skip[i])
        o = sim3_query(mpPos + (size_t)i * 3, mpNormal + (size_t)i * 3, mpMinDist[i], mpMaxDist[i], pose, pose + 7, pose + 11, scaleFactors, nLevels,
                       logScaleFactor, th, variant, minX, minY, maxX, maxY);
    o.descId = i; o.mpId = i; o.blocks = blocks; o.c0 = checkReproj;
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

// SearchByProjection(Frame&, KeyFrame*, sAlreadyFound, th, ORBdist): ORBmatcher.cc:1700-1733; the gate is reloc_query (match_device.h)
__global__ void k_queries_reloc(int nkf, const RumiKeyPoint *kfKeys, const int32_t *kfMp, const uint8_t *skip, const float *mpPos,
                                const float *mpMinDist, const float *mpMaxDist, const float *pose, const float *scaleFactors, int nLevels,
                                float logScaleFactor, float th, float minX, float minY, float maxX, float maxY, Query *q) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nkf) return;
    const int mp = kfMp[i];
    q[i] = reloc_query(mp, mp >= 0 && skip[mp], mpPos, mpMinDist, mpMaxDist, pose, pose + 7, pose + 11, scaleFactors, nLevels, logScaleFactor, th,
                       minX, minY, maxX, maxY, kfKeys[i].angle);
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

// Frame::isInFrustum (Frame.cc:558-617, mono): one lane per map point; the chain is frustum_gate (match_device.h)
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
    const FrustumResult f = frustum_gate(mpPos + (size_t)i * 3, mpNormal + (size_t)i * 3, mpMinDist + i, mpMaxDist + i, pose, minX, minY, maxX, maxY,
                                         logScaleFactor, nLevels, viewingCosLimit);
    inView[i] = f.in; projX[i] = f.px; projY[i] = f.py; scaleLevel[i] = f.lvl; viewCosOut[i] = f.viewCos; trackDepth[i] = f.depth;
}
