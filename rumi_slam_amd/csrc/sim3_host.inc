// sim3_host.inc -- host side of the Sim3 entries (kernels: sim3.inc): rumi_sim3_inliers, rumi_sim3_ransac, rumi_optimize_sim3.
// Included by opt.hip.

extern "C" int rumi_sim3_inliers(RumiOptimizer *o, int32_t n_pairs, const int32_t *pair_start, const int32_t *pair_denominator,
                                 const double *S_c1w2, const double *S_c2w1, const float *K4_1, const float *K4_2, const float *X1, const float *X2,
                                 const float *kp1, const float *kp2, const float *sigma2_1, const float *sigma2_2, const uint8_t *edge1,
                                 const uint8_t *edge2, uint8_t *inlier_out, float *ratio_out, float *median_out) {
    if (!o || n_pairs < 0 || !pair_start || !pair_denominator || !K4_1 || !K4_2 || !median_out) return RUMI_E_INVALID;
    *median_out = 0.f;
    if (n_pairs == 0) return RUMI_OK;
    const int total = pair_start[n_pairs];
    if (total < 0 || (total > 0 && (!S_c1w2 || !S_c2w1 || !X1 || !X2 || !kp1 || !kp2 || !sigma2_1 || !sigma2_2 || !edge1 || !edge2 || !inlier_out)))
        return RUMI_E_INVALID;
    std::vector<float> ratio(n_pairs, 0.f);
    if (total > 0) {
        HIP_TRY(hipSetDevice(o->device));
        // one pinned block up (read in place), one flag array back
        const size_t oP = 0, oA = al16(oP + (size_t)total * 4), oB = al16(oA + (size_t)n_pairs * 64), oK = al16(oB + (size_t)n_pairs * 64), oX1 = al16(oK + 32),
                     oX2 = al16(oX1 + (size_t)total * 12), oK1 = al16(oX2 + (size_t)total * 12), oK2 = al16(oK1 + (size_t)total * 8), oS1 = al16(oK2 + (size_t)total * 8),
                     oS2 = al16(oS1 + (size_t)total * 4), oE1 = al16(oS2 + (size_t)total * 4), oE2 = al16(oE1 + (size_t)total), bytes = al16(oE2 + (size_t)total);
        if (bytes > o->ba.arena.stage.cap || (size_t)total > o->ba.arena.stage.cap) { g_lastError = "Sim3 inliers: more matches than the optimiser's arenas hold"; return RUMI_E_CAPACITY; }
        uint8_t *h = o->ba.arena.stage.h;
        int32_t *pairOf = reinterpret_cast<int32_t *>(h + oP);
        for (int p = 0; p < n_pairs; p++) for (int i = pair_start[p]; i < pair_start[p + 1]; i++) pairOf[i] = p;
        std::memcpy(h + oA, S_c1w2, (size_t)n_pairs * 64); std::memcpy(h + oB, S_c2w1, (size_t)n_pairs * 64);
        std::memcpy(h + oK, K4_1, 16); std::memcpy(h + oK + 16, K4_2, 16);
        std::memcpy(h + oX1, X1, (size_t)total * 12); std::memcpy(h + oX2, X2, (size_t)total * 12);
        std::memcpy(h + oK1, kp1, (size_t)total * 8); std::memcpy(h + oK2, kp2, (size_t)total * 8);
        std::memcpy(h + oS1, sigma2_1, (size_t)total * 4); std::memcpy(h + oS2, sigma2_2, (size_t)total * 4);
        std::memcpy(h + oE1, edge1, (size_t)total); std::memcpy(h + oE2, edge2, (size_t)total);
        HIP_TRY(hipMemcpyAsync(o->ba.arena.stage.d, h, bytes, hipMemcpyHostToDevice, nullptr));
        uint8_t *d = o->ba.arena.stage.d;
        hipLaunchKernelGGL(k_sim3_inliers, dim3((total + 255) / 256), dim3(256), 0, nullptr, total, (const int32_t *)(d + oP), (const double *)(d + oA),
                           (const double *)(d + oB), (const float *)(d + oK), (const float *)(d + oK + 16), (const float *)(d + oX1), (const float *)(d + oX2),
                           (const float *)(d + oK1), (const float *)(d + oK2), (const float *)(d + oS1), (const float *)(d + oS2), d + oE1, d + oE2, o->ba.arena.stageOut.p);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpy(inlier_out, o->ba.arena.stageOut.p, (size_t)total, hipMemcpyDeviceToHost));
    }
    for (int p = 0; p < n_pairs; p++) {                                       // :643-646
        int nIn = 0;
        for (int i = pair_start[p]; i < pair_start[p + 1]; i++) nIn += inlier_out[i];
        ratio[p] = pair_denominator[p] ? (float)nIn / (float)pair_denominator[p] : 0.f;
    }
    if (ratio_out) std::memcpy(ratio_out, ratio.data(), (size_t)n_pairs * sizeof(float));
    std::sort(ratio.begin(), ratio.end());                                    // :654-662
    *median_out = ratio[n_pairs / 2];
    return RUMI_OK;
}

extern "C" int rumi_sim3_ransac(RumiOptimizer *o, int32_t n, const float *X3Dc1, const float *X3Dc2, const float *sigma2_1, const float *sigma2_2,
                                const float *K4_1, const float *K4_2, int32_t fix_scale, int32_t n_hyp, const int32_t *triples,
                                const RumiSim3ScoreSet *score, float *T12_out, int32_t *n_inliers_out, uint8_t *inlier_out, float *ratio_out,
                                float *median_out) {
    if (!o || n < 3 || n_hyp < 0 || !X3Dc1 || !X3Dc2 || !sigma2_1 || !sigma2_2 || !K4_1 || !K4_2 || !T12_out || !n_inliers_out) return RUMI_E_INVALID;
    if (n_hyp == 0) return RUMI_OK;
    if (!triples) return RUMI_E_INVALID;
    for (int i = 0; i < 3 * n_hyp; i++) if (triples[i] < 0 || triples[i] >= n) { g_lastError = "rumi_sim3_ransac: correspondence index out of range"; return RUMI_E_INVALID; }
    int total = 0, np = 0;
    if (score) {
        np = score->n_pairs;
        if (np < 1 || !score->pair_start || !score->pair_denominator || !score->S_c1w1 || !score->S_c2w2 || !score->S_kf1w || !score->S_kf2w || !score->K4_1 ||
            !score->K4_2 || !median_out) return RUMI_E_INVALID;
        total = score->pair_start[np];
        if (total < 0 || (total > 0 && (!score->X1 || !score->X2 || !score->kp1 || !score->kp2 || !score->sigma2_1 || !score->sigma2_2 || !score->edge1 || !score->edge2)))
            return RUMI_E_INVALID;
    }
    HIP_TRY(hipSetDevice(o->device));
    const size_t N = (size_t)n, H = (size_t)n_hyp, T = (size_t)total, NP = (size_t)np;
    const size_t oX1 = 0, oX2 = al16(oX1 + N * 12), oT1 = al16(oX2 + N * 12), oT2 = al16(oT1 + N * 4), oK = al16(oT2 + N * 4), oTri = al16(oK + 64), oKf = al16(oTri + H * 12),
                 oA = al16(oKf + 128), oB = al16(oA + NP * 64), oP = al16(oB + NP * 64), sX1 = al16(oP + T * 4), sX2 = al16(sX1 + T * 12), sK1 = al16(sX2 + T * 12),
                 sK2 = al16(sK1 + T * 8), sS1 = al16(sK2 + T * 8), sS2 = al16(sS1 + T * 4), sE1 = al16(sS2 + T * 4), sE2 = al16(sE1 + T), inBytes = al16(sE2 + T);
    const size_t rT = 0, rN = al16(rT + H * 64), rC = al16(rN + H * 4), rI = al16(rC + H * NP * 4), outBytes = al16(rI + (inlier_out ? H * N : 0)),
                 rComp = outBytes, scratchEnd = al16(rComp + H * NP * 128);
    if (inBytes > o->ba.arena.stage.cap || scratchEnd > o->ba.arena.stage.cap) { g_lastError = "rumi_sim3_ransac: more correspondences / hypotheses than the optimiser's arenas hold"; return RUMI_E_CAPACITY; }
    uint8_t *h = o->ba.arena.stage.h;
    std::memcpy(h + oX1, X3Dc1, N * 12); std::memcpy(h + oX2, X3Dc2, N * 12);
    float *t1 = reinterpret_cast<float *>(h + oT1), *t2 = reinterpret_cast<float *>(h + oT2);
    for (int i = 0; i < n; i++) {        // mvnMaxError1/2 are vector<size_t> upstream (Sim3Solver.h:77-78): 9.210 * sigma2 truncated, compared as float
        t1[i] = (float)(size_t)(9.210 * (double)sigma2_1[i]);
        t2[i] = (float)(size_t)(9.210 * (double)sigma2_2[i]);
    }
    std::memcpy(h + oK, K4_1, 16); std::memcpy(h + oK + 16, K4_2, 16);
    std::memcpy(h + oTri, triples, H * 12);
    if (score) {
        std::memcpy(h + oK + 32, score->K4_1, 16); std::memcpy(h + oK + 48, score->K4_2, 16);
        std::memcpy(h + oKf, score->S_kf1w, 64); std::memcpy(h + oKf + 64, score->S_kf2w, 64);
        std::memcpy(h + oA, score->S_c1w1, NP * 64); std::memcpy(h + oB, score->S_c2w2, NP * 64);
        int32_t *pairOf = reinterpret_cast<int32_t *>(h + oP);
        for (int p = 0; p < np; p++) {
            if (score->pair_start[p] > score->pair_start[p + 1] || score->pair_start[p] < 0) { g_lastError = "rumi_sim3_ransac: pair_start is not ascending"; return RUMI_E_INVALID; }
            for (int i = score->pair_start[p]; i < score->pair_start[p + 1]; i++) pairOf[i] = p;
        }
        if (total) {
            std::memcpy(h + sX1, score->X1, T * 12); std::memcpy(h + sX2, score->X2, T * 12); std::memcpy(h + sK1, score->kp1, T * 8); std::memcpy(h + sK2, score->kp2, T * 8);
            std::memcpy(h + sS1, score->sigma2_1, T * 4); std::memcpy(h + sS2, score->sigma2_2, T * 4); std::memcpy(h + sE1, score->edge1, T); std::memcpy(h + sE2, score->edge2, T);
        }
    }
    HIP_TRY(hipMemcpyAsync(o->ba.arena.stage.d, h, inBytes, hipMemcpyHostToDevice, nullptr));
    uint8_t *d = o->ba.arena.stage.d, *r = o->ba.arena.stageOut.p;
    RansacArgs A;
    A.n = n; A.nHyp = n_hyp; A.fixScale = fix_scale != 0;
    A.X1 = (const float *)(d + oX1); A.X2 = (const float *)(d + oX2); A.thr1 = (const float *)(d + oT1); A.thr2 = (const float *)(d + oT2);
    A.K1 = (const float *)(d + oK); A.K2 = (const float *)(d + oK + 16); A.tri = (const int32_t *)(d + oTri);
    A.T12 = (float *)(r + rT); A.nIn = (int32_t *)(r + rN); A.inl = inlier_out ? r + rI : nullptr;
    A.nPairs = np; A.total = score ? (total > 0 ? total : 0) : 0;
    A.pairOf = (const int32_t *)(d + oP); A.Sc1w1 = (const double *)(d + oA); A.Sc2w2 = (const double *)(d + oB); A.Skf = (const double *)(d + oKf);
    A.sK1 = (const float *)(d + oK + 32); A.sK2 = (const float *)(d + oK + 48); A.sX1 = (const float *)(d + sX1); A.sX2 = (const float *)(d + sX2);
    A.kp1 = (const float *)(d + sK1); A.kp2 = (const float *)(d + sK2); A.sg1 = (const float *)(d + sS1); A.sg2 = (const float *)(d + sS2);
    A.e1 = d + sE1; A.e2 = d + sE2; A.pairCnt = (int32_t *)(r + rC); A.comp = (double *)(r + rComp);
    hipLaunchKernelGGL(k_sim3_ransac, dim3(n_hyp), dim3(256), 0, nullptr, A);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(h, r, outBytes, hipMemcpyDeviceToHost, nullptr));
    HIP_TRY(hipStreamSynchronize(nullptr));
    std::memcpy(T12_out, h + rT, H * 64);
    std::memcpy(n_inliers_out, h + rN, H * 4);
    if (inlier_out) std::memcpy(inlier_out, h + rI, H * N);
    if (score) {                                                              // :643-662 per hypothesis
        const int32_t *cnt = reinterpret_cast<const int32_t *>(h + rC);
        std::vector<float> ratio(np);
        for (int hh = 0; hh < n_hyp; hh++) {
            for (int p = 0; p < np; p++) ratio[p] = (total > 0 && score->pair_denominator[p]) ? (float)cnt[(size_t)hh * np + p] / (float)score->pair_denominator[p] : 0.f;
            if (ratio_out) std::memcpy(ratio_out + (size_t)hh * np, ratio.data(), NP * sizeof(float));
            std::sort(ratio.begin(), ratio.end());
            median_out[hh] = ratio[np / 2];
        }
    }
    return RUMI_OK;
}

extern "C" int rumi_optimize_sim3(RumiOptimizer *o, int32_t n, const int32_t *pair_of, int32_t n_pairs, const double *S_c1w, const double *S_c2w,
                                  const float *P1c, const float *P2c, const float *obs1, const float *obs2, const float *inv_sigma2_1,
                                  const float *inv_sigma2_2, const uint8_t *skip12, const uint8_t *skip21, const float *K4_1, const float *K4_2,
                                  float th2, int32_t fix_scale, int32_t robust_first_pass, double *S_io8, uint8_t *status_out, int32_t *result3) {
    if (!o || n < 0 || !K4_1 || !K4_2 || !S_io8 || !result3) return RUMI_E_INVALID;
    if (n > 0 && (!P1c || !P2c || !obs1 || !obs2 || !inv_sigma2_1 || !inv_sigma2_2 || !status_out)) return RUMI_E_INVALID;
    const bool world = S_c1w != nullptr;
    if (world && (!S_c2w || n_pairs < 1 || (n > 0 && !pair_of))) return RUMI_E_INVALID;
    if (!world) n_pairs = 1;
    if (world) for (int i = 0; i < n; i++) if (pair_of[i] < 0 || pair_of[i] >= n_pairs) { g_lastError = "rumi_optimize_sim3: pair index out of range"; return RUMI_E_INVALID; }
    HIP_TRY(hipSetDevice(o->device));
    const size_t N = (size_t)n, NP = (size_t)n_pairs;
    const size_t oS = 0, oA = al16(oS + 64), oB = al16(oA + NP * 64), oK = al16(oB + NP * 64), oP = al16(oK + 32), oX1 = al16(oP + N * 4), oX2 = al16(oX1 + N * 12),
                 oO1 = al16(oX2 + N * 12), oO2 = al16(oO1 + N * 8), oW1 = al16(oO2 + N * 8), oW2 = al16(oW1 + N * 4), oE1 = al16(oW2 + N * 4), oE2 = al16(oE1 + N),
                 inBytes = al16(oE2 + N);
    // result block: estimate, counters, status; scratch behind it
    const size_t rS = 0, rR = 64, rSt = 80, outBytes = al16(rSt + N), sC = outBytes, sX1 = al16(sC + NP * 30 * 64), sX2 = al16(sX1 + N * 8), sO1 = al16(sX2 + N * 8),
                 sO2 = al16(sO1 + N), scratchEnd = al16(sO2 + N);
    if (inBytes > o->ba.arena.stage.cap || scratchEnd > o->ba.arena.stage.cap) { g_lastError = "rumi_optimize_sim3: more correspondences than the optimiser's arenas hold"; return RUMI_E_CAPACITY; }
    uint8_t *h = o->ba.arena.stage.h;
    std::memcpy(h + oS, S_io8, 64);
    if (world) { std::memcpy(h + oA, S_c1w, NP * 64); std::memcpy(h + oB, S_c2w, NP * 64); if (n) std::memcpy(h + oP, pair_of, N * 4); }
    std::memcpy(h + oK, K4_1, 16); std::memcpy(h + oK + 16, K4_2, 16);
    if (n) {
        std::memcpy(h + oX1, P1c, N * 12); std::memcpy(h + oX2, P2c, N * 12); std::memcpy(h + oO1, obs1, N * 8); std::memcpy(h + oO2, obs2, N * 8);
        std::memcpy(h + oW1, inv_sigma2_1, N * 4); std::memcpy(h + oW2, inv_sigma2_2, N * 4);
        if (skip12) std::memcpy(h + oE1, skip12, N); else std::memset(h + oE1, 0, N);
        if (skip21) std::memcpy(h + oE2, skip21, N); else std::memset(h + oE2, 0, N);
    }
    HIP_TRY(hipMemcpyAsync(o->ba.arena.stage.d, h, inBytes, hipMemcpyHostToDevice, nullptr));
    uint8_t *d = o->ba.arena.stage.d, *r = o->ba.arena.stageOut.p;
    Sim3Args A;
    A.n = n; A.nPairs = n_pairs; A.world = world; A.fixScale = fix_scale != 0; A.robustFirst = robust_first_pass != 0; A.th2 = th2;
    A.pairOf = world ? (const int32_t *)(d + oP) : nullptr;
    A.Sc1w = (const double *)(d + oA); A.Sc2w = (const double *)(d + oB); A.Sin = (const double *)(d + oS);
    A.P1c = (const float *)(d + oX1); A.P2c = (const float *)(d + oX2); A.obs1 = (const float *)(d + oO1); A.obs2 = (const float *)(d + oO2);
    A.w1 = (const float *)(d + oW1); A.w2 = (const float *)(d + oW2); A.skip12 = d + oE1; A.skip21 = d + oE2;
    A.K1 = (const float *)(d + oK); A.K2 = (const float *)(d + oK + 16);
    A.Sout = (double *)(r + rS); A.res = (int32_t *)(r + rR); A.status = r + rSt;
    A.comp = (double *)(r + sC); A.chi12 = (double *)(r + sX1); A.chi21 = (double *)(r + sX2); A.on12 = r + sO1; A.on21 = r + sO2;
    hipLaunchKernelGGL(k_sim3_opt, dim3(1), dim3(256), 0, nullptr, A);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(h, r, outBytes, hipMemcpyDeviceToHost, nullptr));
    HIP_TRY(hipStreamSynchronize(nullptr));
    std::memcpy(S_io8, h + rS, 64);
    std::memcpy(result3, h + rR, 12);
    if (n) std::memcpy(status_out, h + rSt, N);
    return RUMI_OK;
}
