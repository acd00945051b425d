// SearchForTriangulation: its two kernels and its C entry.
namespace rumi {

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
    const int lo = fv_find_node(A.nodes2, A.nn2, A.nodes1[a]);
    const bool hit = lo >= 0;
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
        if (tid == 0) three_maxima_keep(sHist, sKeep);
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

}  // namespace rumi

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
    RC_TRY(upload_frame(m, KF2, &fd));
    float geom[11];
    std::memcpy(geom, F12, 36); std::memcpy(geom + 9, epipole2, 8);
    H2D(m->dPose, geom, 11);
    H2D(m->dFeatMp, kf2_mp, KF2->n);
    RC_TRY(stage_query_keyframe(m, KF1, kf1_mp));
    RC_TRY(stage_fv_query(m, fv1, nqe));
    RC_TRY(stage_fv_frame(m, fv2, nfe));
    TriArgs A{fv1->n_nodes, fv2->n_nodes, m->dNodesA, m->dOffA, m->dIdxA, m->dNodesB, m->dOffB, m->dFvIdx, m->dQKeys, m->dKeys,
              m->dQDesc, m->dDesc, m->dI[0], m->dFeatMp, m->dScale, m->dPose, coarse, m->dAssign};
    FLUSH(m);
    hipLaunchKernelGGL(k_tri_match, dim3((fv1->n_nodes + 63) / 64), dim3(64), 0, nullptr, A);
    hipLaunchKernelGGL(k_tri_filter, dim3(1), dim3(256), 0, nullptr, nqe, m->dIdxA, m->dQKeys, m->dKeys, m->dAssign, check_orientation, m->dNmatches);
    HIP_TRY(hipGetLastError());
    RC_TRY(fetch_results(m, 0, nqe, true));
    *nmatches_out = m->hOut[0];
    const int32_t *assign = m->hOut + 4 + m->maxFeat;
    for (int p = 0; p < nqe; p++) if (assign[p] >= 0) matches12[fv1->indices[p]] = assign[p];
    return RUMI_OK;
}
