// sim3_batch_host.inc -- host side of the batched Sim3 entries (kernels: sim3_batch.inc): rumi_sim3_ransac_batch, rumi_optimize_sim3_batch.
// Included by opt.hip after sim3_host.inc.  Both are one round trip through the handle's staging arena: one upload, the launches on the null
// stream, one download, one synchronise.

// the ranges [first, first + n) of the records ascend inside [0, total) without overlap
template <class Rec> static bool ranges_in_order(const Rec *r, int count, int total, int minN) {
    long long end = 0;
    for (int j = 0; j < count; j++) {
        if (r[j].n < minN || r[j].first < end || (long long)r[j].first + r[j].n > total) return false;
        end = (long long)r[j].first + r[j].n;
    }
    return true;
}

extern "C" int rumi_sim3_ransac_batch(RumiOptimizer *o, int32_t n_solvers, const RumiSim3RansacSolver *solvers, int32_t n_total, const float *X3Dc1,
                                      const float *X3Dc2, const float *sigma2_1, const float *sigma2_2, int32_t window, const int32_t *triples,
                                      RumiSim3RansacResult *results, uint8_t *inlier_out, int32_t *n_inliers_all, float *T12_all) {
    if (!o || n_solvers < 0 || n_total < 0) return RUMI_E_INVALID;
    if (window < 1) { g_lastError = "rumi_sim3_ransac_batch: window must be >= 1"; return RUMI_E_INVALID; }
    if (n_solvers == 0) return RUMI_OK;
    if (!solvers || !X3Dc1 || !X3Dc2 || !sigma2_1 || !sigma2_2 || !triples || !results || !inlier_out) return RUMI_E_INVALID;
    int nMax = 0;
    for (int j = 0; j < n_solvers; j++) {
        if (solvers[j].n < 3) { g_lastError = "rumi_sim3_ransac_batch: a solver needs at least 3 correspondences"; return RUMI_E_INVALID; }
        if (solvers[j].its_left < 1) { g_lastError = "rumi_sim3_ransac_batch: its_left must be >= 1"; return RUMI_E_INVALID; }
        nMax = std::max(nMax, solvers[j].n);
    }
    if (!ranges_in_order(solvers, n_solvers, n_total, 3)) { g_lastError = "rumi_sim3_ransac_batch: the solvers' ranges must ascend inside n_total without overlap"; return RUMI_E_INVALID; }
    const size_t J = (size_t)n_solvers, R = (size_t)window, N = (size_t)n_total, H = J * R;
    for (size_t j = 0; j < J; j++)
        for (size_t i = 0; i < R * 3; i++) {
            const int32_t t = triples[j * R * 3 + i];
            if (t < 0 || t >= solvers[j].n) { g_lastError = "rumi_sim3_ransac_batch: correspondence index out of range"; return RUMI_E_INVALID; }
        }
    const size_t oSol = 0, oX1 = al16(oSol + J * sizeof(S3bSolver)), oX2 = al16(oX1 + N * 12), oT1 = al16(oX2 + N * 12), oT2 = al16(oT1 + N * 4), oTri = al16(oT2 + N * 4),
                 inBytes = al16(oTri + H * 12);
    // result block: records, masks of the converged, then what only a caller that asks for every hypothesis downloads; scratch behind it
    const bool all = n_inliers_all || T12_all;
    const size_t rRes = 0, rInl = al16(rRes + J * sizeof(S3bResult)), rN = al16(rInl + N), rT = al16(rN + H * 4), rEnd = al16(rT + H * 64), outBytes = all ? rEnd : rN,
                 s12 = rEnd, s21 = al16(s12 + H * 48), sMask = al16(s21 + H * 48), scratchEnd = al16(sMask + H * (size_t)nMax);
    if (inBytes > o->ba.arena.stage.cap || scratchEnd > o->ba.arena.stage.cap) { g_lastError = "rumi_sim3_ransac_batch: more correspondences / hypotheses than the optimiser's arenas hold"; return RUMI_E_CAPACITY; }
    HIP_TRY(hipSetDevice(o->device));
    uint8_t *h = o->ba.arena.stage.h;
    std::memcpy(h + oSol, solvers, J * sizeof(S3bSolver));
    std::memcpy(h + oX1, X3Dc1, N * 12); std::memcpy(h + oX2, X3Dc2, N * 12);
    float *t1 = reinterpret_cast<float *>(h + oT1), *t2 = reinterpret_cast<float *>(h + oT2);
    for (int i = 0; i < n_total; i++) {  // mvnMaxError1/2 as rumi_sim3_ransac forms them
        t1[i] = (float)(size_t)(9.210 * (double)sigma2_1[i]);
        t2[i] = (float)(size_t)(9.210 * (double)sigma2_2[i]);
    }
    std::memcpy(h + oTri, triples, H * 12);
    HIP_TRY(hipMemcpyAsync(o->ba.arena.stage.d, h, inBytes, hipMemcpyHostToDevice, nullptr));
    uint8_t *d = o->ba.arena.stage.d, *r = o->ba.arena.stageOut.p;
    S3bArgs A;
    A.J = n_solvers; A.R = window; A.nMax = nMax;
    A.sol = (const S3bSolver *)(d + oSol); A.X1 = (const float *)(d + oX1); A.X2 = (const float *)(d + oX2); A.thr1 = (const float *)(d + oT1);
    A.thr2 = (const float *)(d + oT2); A.tri = (const int32_t *)(d + oTri);
    A.rows12 = (float *)(r + s12); A.rows21 = (float *)(r + s21); A.Tall = (float *)(r + rT); A.nInAll = (int32_t *)(r + rN); A.mask = r + sMask;
    A.res = (S3bResult *)(r + rRes); A.inl = r + rInl;
    HIP_TRY(hipMemsetAsync(r + rInl, 0, N, nullptr));              // correspondences between the solvers' ranges belong to nobody
    hipLaunchKernelGGL(k_s3b_hyp, dim3((unsigned)((H + 255) / 256)), dim3(256), 0, nullptr, A);
    hipLaunchKernelGGL(k_s3b_check, dim3((unsigned)((H + 3) / 4)), dim3(256), 0, nullptr, A);
    hipLaunchKernelGGL(k_s3b_select, dim3(1), dim3(64), 0, nullptr, A);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(h, r, outBytes, hipMemcpyDeviceToHost, nullptr));
    HIP_TRY(hipStreamSynchronize(nullptr));
    std::memcpy(results, h + rRes, J * sizeof(S3bResult));
    std::memcpy(inlier_out, h + rInl, N);
    if (n_inliers_all) std::memcpy(n_inliers_all, h + rN, H * 4);
    if (T12_all) std::memcpy(T12_all, h + rT, H * 64);
    return RUMI_OK;
}

extern "C" int rumi_optimize_sim3_batch(RumiOptimizer *o, int32_t n_problems, const RumiSim3OptProblem *problems, int32_t n_total, const float *P1c,
                                        const float *P2c, const float *obs1, const float *obs2, const float *inv_sigma2_1, const float *inv_sigma2_2,
                                        double *S_io8, uint8_t *status_out, int32_t *result3) {
    if (!o || n_problems < 0 || n_total < 0) return RUMI_E_INVALID;
    if (n_problems == 0) return RUMI_OK;
    if (!problems || !S_io8 || !result3) return RUMI_E_INVALID;
    if (n_total > 0 && (!P1c || !P2c || !obs1 || !obs2 || !inv_sigma2_1 || !inv_sigma2_2 || !status_out)) return RUMI_E_INVALID;
    if (!ranges_in_order(problems, n_problems, n_total, 0)) { g_lastError = "rumi_optimize_sim3_batch: the problems' ranges must ascend inside n_total without overlap"; return RUMI_E_INVALID; }
    const size_t J = (size_t)n_problems, N = (size_t)n_total;
    const size_t oTab = 0, oS = al16(oTab + J * sizeof(Sim3Args)), oK = al16(oS + J * 64), oX1 = al16(oK + J * 32), oX2 = al16(oX1 + N * 12), oO1 = al16(oX2 + N * 12),
                 oO2 = al16(oO1 + N * 8), oW1 = al16(oO2 + N * 8), oW2 = al16(oW1 + N * 4), inBytes = al16(oW2 + N * 4);
    // result block: estimates, counters, status; per problem scratch behind it (30 composites, chi2 of both edge kinds, the two active flags)
    const size_t rS = 0, rR = al16(rS + J * 64), rSt = al16(rR + J * 16), outBytes = al16(rSt + N), sC = outBytes, sX1 = al16(sC + J * 30 * 64), sX2 = al16(sX1 + N * 8),
                 sO1 = al16(sX2 + N * 8), sO2 = al16(sO1 + N), scratchEnd = al16(sO2 + N);
    if (inBytes > o->ba.arena.stage.cap || scratchEnd > o->ba.arena.stage.cap) { g_lastError = "rumi_optimize_sim3_batch: more correspondences than the optimiser's arenas hold"; return RUMI_E_CAPACITY; }
    HIP_TRY(hipSetDevice(o->device));
    uint8_t *h = o->ba.arena.stage.h, *d = o->ba.arena.stage.d, *r = o->ba.arena.stageOut.p;
    Sim3Args *tab = reinterpret_cast<Sim3Args *>(h + oTab);
    for (size_t j = 0; j < J; j++) {
        const RumiSim3OptProblem &p = problems[j];
        const size_t f = (size_t)p.first;
        std::memcpy(h + oK + j * 32, p.K4_1, 16); std::memcpy(h + oK + j * 32 + 16, p.K4_2, 16);
        Sim3Args &A = tab[j];
        A.n = p.n; A.nPairs = 1; A.world = 0; A.fixScale = p.fix_scale != 0; A.robustFirst = p.robust_first_pass != 0; A.th2 = p.th2;
        // (the single entry uploads zeroed skip arrays where the caller gives none; the kernel's `!(skip && skip[i])` reads a null pointer the same way)
        A.pairOf = nullptr; A.Sc1w = nullptr; A.Sc2w = nullptr; A.skip12 = nullptr; A.skip21 = nullptr;
        A.Sin = (const double *)(d + oS + j * 64);
        A.P1c = (const float *)(d + oX1) + f * 3; A.P2c = (const float *)(d + oX2) + f * 3; A.obs1 = (const float *)(d + oO1) + f * 2; A.obs2 = (const float *)(d + oO2) + f * 2;
        A.w1 = (const float *)(d + oW1) + f; A.w2 = (const float *)(d + oW2) + f;
        A.K1 = (const float *)(d + oK + j * 32); A.K2 = (const float *)(d + oK + j * 32 + 16);
        A.Sout = (double *)(r + rS + j * 64); A.res = (int32_t *)(r + rR + j * 16); A.status = r + rSt + f;
        A.comp = (double *)(r + sC + j * 30 * 64); A.chi12 = (double *)(r + sX1) + f; A.chi21 = (double *)(r + sX2) + f; A.on12 = r + sO1 + f; A.on21 = r + sO2 + f;
    }
    std::memcpy(h + oS, S_io8, J * 64);
    if (n_total) {
        std::memcpy(h + oX1, P1c, N * 12); std::memcpy(h + oX2, P2c, N * 12); std::memcpy(h + oO1, obs1, N * 8); std::memcpy(h + oO2, obs2, N * 8);
        std::memcpy(h + oW1, inv_sigma2_1, N * 4); std::memcpy(h + oW2, inv_sigma2_2, N * 4);
    }
    HIP_TRY(hipMemcpyAsync(d, h, inBytes, hipMemcpyHostToDevice, nullptr));
    HIP_TRY(hipMemsetAsync(r + rSt, 0, N, nullptr));               // correspondences between the problems' ranges belong to nobody
    hipLaunchKernelGGL(k_sim3_opt_batch, dim3(n_problems), dim3(256), 0, nullptr, (const Sim3Args *)(d + oTab));
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(h, r, outBytes, hipMemcpyDeviceToHost, nullptr));
    HIP_TRY(hipStreamSynchronize(nullptr));
    std::memcpy(S_io8, h + rS, J * 64);
    for (size_t j = 0; j < J; j++) std::memcpy(result3 + j * 3, h + rR + j * 16, 12);
    if (n_total) std::memcpy(status_out, h + rSt, N);
    return RUMI_OK;
}
