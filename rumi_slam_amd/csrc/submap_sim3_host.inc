// submap_sim3_host.inc -- host side of the sub-map alignment session (kernels: submap_sim3.inc): rumi_submap_sim3_begin / _end / _score / _ransac and
// the test hook that sets the chunk length.  Included by opt.hip after sim3_batch_host.inc.  The session's blocks live in RumiOptimizer::sms
// (SubmapSim3Part) and grow on demand; nothing here touches the per-call staging arena of the other Sim3 entries.

// Iterations of the stream enqueued between two read-backs of the state (DESIGN.md 4ac): the first chunk is short, for the merge that converges in its
// first block of 20; every later one is twice as long up to the cap, for the merge that uses every iteration of every solver.
constexpr int kSmsFirstChunk = 64, kSmsChunkCap = 1024;
constexpr size_t kSmsMaxBytes = (size_t)1 << 30;  // of any one block of the session

static int sms_require_set(const RumiOptimizer *o, const char *entry) {
    if (!o) return RUMI_E_INVALID;
    if (!o->sms.have) { g_lastError = std::string(entry) + ": no score set (rumi_submap_sim3_begin)"; return RUMI_E_INVALID; }
    return RUMI_OK;
}

extern "C" int rumi_submap_sim3_end(RumiOptimizer *o) {
    const int rc = sms_require_set(o, "rumi_submap_sim3_end");
    if (rc != RUMI_OK) return rc;
    o->sms.have = false;
    return RUMI_OK;
}

extern "C" int rumi_hook_submap_sim3_set_chunk(RumiOptimizer *o, int32_t chunk) {
    if (!o || chunk < 0) return RUMI_E_INVALID;
    o->sms.chunk = chunk;
    return RUMI_OK;
}

extern "C" int rumi_submap_sim3_begin(RumiOptimizer *o, const RumiSim3ScoreSet *set) {
    if (!o || !set) return RUMI_E_INVALID;
    const int np = set->n_pairs;
    if (np < 1 || !set->pair_start || !set->pair_denominator || !set->S_c1w1 || !set->S_c2w2 || !set->K4_1 || !set->K4_2) return RUMI_E_INVALID;
    for (int p = 0; p < np; p++)
        if (set->pair_start[p] < 0 || set->pair_start[p] > set->pair_start[p + 1]) { g_lastError = "rumi_submap_sim3_begin: pair_start is not ascending"; return RUMI_E_INVALID; }
    const int total = set->pair_start[np];
    if (total > 0 && (!set->X1 || !set->X2 || !set->kp1 || !set->kp2 || !set->sigma2_1 || !set->sigma2_2 || !set->edge1 || !set->edge2)) return RUMI_E_INVALID;
    // what pairOf is to the other entries: every pair's matches cut into slabs of at most kSmsSlab, the unit a workgroup of k_sms_score takes
    size_t nSlabs = 0;
    for (int p = 0; p < np; p++) nSlabs += ((size_t)(set->pair_start[p + 1] - set->pair_start[p]) + kSmsSlab - 1) / kSmsSlab;
    const size_t NP = (size_t)np, T = (size_t)total;
    const size_t oDen = 0, oSlab = al16(oDen + NP * 4), oA = al16(oSlab + nSlabs * 12), oB = al16(oA + NP * 64), oK = al16(oB + NP * 64), oX1 = al16(oK + 32),
                 oX2 = al16(oX1 + T * 12), oK1 = al16(oX2 + T * 12), oK2 = al16(oK1 + T * 8), oS1 = al16(oK2 + T * 8), oS2 = al16(oS1 + T * 4), oE1 = al16(oS2 + T * 4),
                 oE2 = al16(oE1 + T), bytes = al16(oE2 + T);
    if (bytes > kSmsMaxBytes) { g_lastError = "rumi_submap_sim3_begin: the score set is larger than a session holds"; return RUMI_E_CAPACITY; }
    HIP_TRY(hipSetDevice(o->device));
    SubmapSim3Part &S = o->sms;
    S.have = false;                                                  // a failure below leaves no half-replaced set behind
    const int rc = S.set.reserve(bytes, bytes);
    if (rc != RUMI_OK) return rc;
    uint8_t *h = S.set.h, *d = S.set.d;
    std::memcpy(h + oDen, set->pair_denominator, NP * 4);
    int32_t *slab = reinterpret_cast<int32_t *>(h + oSlab);
    for (int p = 0; p < np; p++)
        for (int a = set->pair_start[p]; a < set->pair_start[p + 1]; a += kSmsSlab) { *slab++ = p; *slab++ = a; *slab++ = std::min(kSmsSlab, set->pair_start[p + 1] - a); }
    std::memcpy(h + oA, set->S_c1w1, NP * 64); std::memcpy(h + oB, set->S_c2w2, NP * 64);
    std::memcpy(h + oK, set->K4_1, 16); std::memcpy(h + oK + 16, set->K4_2, 16);
    if (total) {
        std::memcpy(h + oX1, set->X1, T * 12); std::memcpy(h + oX2, set->X2, T * 12); std::memcpy(h + oK1, set->kp1, T * 8); std::memcpy(h + oK2, set->kp2, T * 8);
        std::memcpy(h + oS1, set->sigma2_1, T * 4); std::memcpy(h + oS2, set->sigma2_2, T * 4); std::memcpy(h + oE1, set->edge1, T); std::memcpy(h + oE2, set->edge2, T);
    }
    HIP_TRY(hipMemcpyAsync(d, h, bytes, hipMemcpyHostToDevice, nullptr));
    HIP_TRY(hipStreamSynchronize(nullptr));
    SmsSet &V = S.view;
    V.nPairs = np; V.total = total; V.nSlabs = (int)nSlabs;
    V.denom = (const int32_t *)(d + oDen); V.slab = (const int32_t *)(d + oSlab); V.Sc1w1 = (const double *)(d + oA); V.Sc2w2 = (const double *)(d + oB);
    V.K = (const float *)(d + oK); V.X1 = (const float *)(d + oX1); V.X2 = (const float *)(d + oX2); V.kp1 = (const float *)(d + oK1); V.kp2 = (const float *)(d + oK2);
    V.sg1 = (const float *)(d + oS1); V.sg2 = (const float *)(d + oS2); V.e1 = d + oE1; V.e2 = d + oE2;
    S.have = true;
    return RUMI_OK;
}

// ComputeInliersNum's counts and the median of the hypotheses (or transforms) [A.g0, A.g1) on the null stream
template <bool FORM> static int sms_enqueue_score(const SmsArgs &A) {
    const int n = A.g1 - A.g0, np = A.set.nPairs;
    const size_t groups = (size_t)A.set.nSlabs * (size_t)((n + kSmsHT - 1) / kSmsHT);   // one-dimensional grid of k_sms_score
    if (groups > 0x7fffffffu) { g_lastError = "rumi_submap_sim3: more (slab, hypothesis tile) workgroups than a launch takes"; return RUMI_E_CAPACITY; }
    HIP_TRY(hipMemsetAsync(A.cnt + (size_t)A.g0 * np, 0, (size_t)n * np * 4, nullptr));
    if (groups > 0) hipLaunchKernelGGL(k_sms_score<FORM>, dim3((unsigned)groups), dim3(256), 0, nullptr, A);
    hipLaunchKernelGGL(k_sms_median, dim3((n + 3) / 4), dim3(256), 0, nullptr, A);
    return RUMI_OK;
}

extern "C" int rumi_submap_sim3_score(RumiOptimizer *o, int32_t n_S, const double *S_c1w2, const double *S_c2w1, uint8_t *inlier_out, float *ratio_out,
                                      float *median_out) {
    int rc = sms_require_set(o, "rumi_submap_sim3_score");
    if (rc != RUMI_OK) return rc;
    if (n_S < 0) return RUMI_E_INVALID;
    if (n_S == 0) return RUMI_OK;
    if (!S_c1w2 || !S_c2w1 || !median_out) return RUMI_E_INVALID;
    SubmapSim3Part &S = o->sms;
    const size_t NS = (size_t)n_S, NP = (size_t)S.view.nPairs, T = (size_t)S.view.total;
    const size_t oA = 0, oB = al16(oA + NS * NP * 64), inBytes = al16(oB + NS * NP * 64);
    const size_t rM = 0, rR = al16(rM + NS * 4), rI = al16(rR + NS * NP * 4), outBytes = al16(rI + (inlier_out ? NS * T : 0));
    const size_t wBytes = al16(NS * NP * 4);
    if (inBytes > kSmsMaxBytes || outBytes > kSmsMaxBytes) { g_lastError = "rumi_submap_sim3_score: more transforms than a session holds"; return RUMI_E_CAPACITY; }
    HIP_TRY(hipSetDevice(o->device));
    rc = S.io.reserve(inBytes, inBytes);
    if (rc == RUMI_OK) rc = S.out.reserve(outBytes, outBytes);
    if (rc == RUMI_OK) rc = S.work.reserve(wBytes, wBytes);
    if (rc != RUMI_OK) return rc;
    std::memcpy(S.io.h + oA, S_c1w2, NS * NP * 64); std::memcpy(S.io.h + oB, S_c2w1, NS * NP * 64);
    HIP_TRY(hipMemcpyAsync(S.io.d, S.io.h, inBytes, hipMemcpyHostToDevice, nullptr));
    SmsArgs A{};
    A.set = S.view; A.g0 = 0; A.g1 = n_S;
    A.Sgiven1 = (const double *)(S.io.d + oA); A.Sgiven2 = (const double *)(S.io.d + oB);
    A.cnt = (int32_t *)S.work.p; A.med = (float *)(S.out.d + rM); A.ratio = (float *)(S.out.d + rR); A.inl = inlier_out ? S.out.d + rI : nullptr;
    rc = sms_enqueue_score<false>(A);
    if (rc != RUMI_OK) return rc;
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(S.out.h, S.out.d, outBytes, hipMemcpyDeviceToHost, nullptr));
    HIP_TRY(hipStreamSynchronize(nullptr));
    std::memcpy(median_out, S.out.h + rM, NS * 4);
    if (ratio_out) std::memcpy(ratio_out, S.out.h + rR, NS * NP * 4);
    if (inlier_out) std::memcpy(inlier_out, S.out.h + rI, NS * T);
    return RUMI_OK;
}

extern "C" int rumi_submap_sim3_ransac(RumiOptimizer *o, int32_t n_solvers, const RumiSubmapSolver *solvers, int32_t n_total, const float *X3Dc1,
                                       const float *X3Dc2, const float *sigma2_1, const float *sigma2_2, const int32_t *triples, float best_ratio_in,
                                       RumiSubmapSolverResult *results, int32_t *its_consumed, int32_t *n_inliers_all, float *median_all, float *T12_all) {
    int rc = sms_require_set(o, "rumi_submap_sim3_ransac");
    if (rc != RUMI_OK) return rc;
    if (n_solvers < 0 || n_total < 0 || !its_consumed) return RUMI_E_INVALID;
    if (n_solvers == 0) { *its_consumed = 0; return RUMI_OK; }
    if (!solvers || !X3Dc1 || !X3Dc2 || !sigma2_1 || !sigma2_2 || !triples || !results) return RUMI_E_INVALID;
    long long sum = 0;
    for (int j = 0; j < n_solvers; j++) {
        if (solvers[j].its < 1) { g_lastError = "rumi_submap_sim3_ransac: its must be >= 1"; return RUMI_E_INVALID; }
        sum += solvers[j].its;
    }
    if (!ranges_in_order(solvers, n_solvers, n_total, 3)) { g_lastError = "rumi_submap_sim3_ransac: the solvers' ranges (n >= 3) must ascend inside n_total without overlap"; return RUMI_E_INVALID; }
    SubmapSim3Part &S = o->sms;
    const size_t J = (size_t)n_solvers, N = (size_t)n_total, H = (size_t)sum, NP = (size_t)S.view.nPairs;
    if (H > kSmsMaxBytes / (128 + NP * 8)) { g_lastError = "rumi_submap_sim3_ransac: more iterations than a session holds"; return RUMI_E_CAPACITY; }
    {
        const int32_t *t = triples;
        for (size_t j = 0; j < J; j++)
            for (int i = 0; i < 3 * solvers[j].its; i++, t++)
                if (*t < 0 || *t >= solvers[j].n) { g_lastError = "rumi_submap_sim3_ransac: correspondence index out of range"; return RUMI_E_INVALID; }
    }
    // up: the state and the result records (the select kernel writes them in place), solvers, correspondences, thresholds, minimal sets, solver of every iteration
    const size_t oSt = 0, oRes = al16(oSt + sizeof(SmsState)), oSol = al16(oRes + J * sizeof(SmsResult)), oX1 = al16(oSol + J * sizeof(SmsSolver)), oX2 = al16(oX1 + N * 12),
                 oT1 = al16(oX2 + N * 12), oT2 = al16(oT1 + N * 4), oTri = al16(oT2 + N * 4), oIt = al16(oTri + H * 12), inBytes = al16(oIt + H * 4);
    const size_t rN = 0, rM = al16(rN + H * 4), rT = al16(rM + H * 4), outBytes = al16(rT + H * 64);
    const size_t w12 = 0, w21 = al16(w12 + H * 48), wSw = al16(w21 + H * 48), wCnt = al16(wSw + H * 128), wRat = al16(wCnt + H * NP * 4), wBytes = al16(wRat + H * NP * 4);
    if (inBytes > kSmsMaxBytes) { g_lastError = "rumi_submap_sim3_ransac: more correspondences than a session holds"; return RUMI_E_CAPACITY; }
    HIP_TRY(hipSetDevice(o->device));
    rc = S.io.reserve(inBytes, inBytes);
    if (rc == RUMI_OK) rc = S.out.reserve(outBytes, outBytes);
    if (rc == RUMI_OK) rc = S.work.reserve(wBytes, wBytes);
    if (rc != RUMI_OK) return rc;
    uint8_t *h = S.io.h, *d = S.io.d;
    SmsState st0{};
    st0.bestHyp = -1; st0.bestRatio = best_ratio_in;
    std::memcpy(h + oSt, &st0, sizeof st0);
    SmsResult *res0 = reinterpret_cast<SmsResult *>(h + oRes);
    for (size_t j = 0; j < J; j++) { std::memset(&res0[j], 0, sizeof(SmsResult)); res0[j].state = RUMI_SIM3_NOT_REACHED; res0[j].bestHyp = -1; }
    std::memcpy(h + oSol, solvers, J * sizeof(SmsSolver));
    std::memcpy(h + oX1, X3Dc1, N * 12); std::memcpy(h + oX2, X3Dc2, N * 12);
    float *t1 = reinterpret_cast<float *>(h + oT1), *t2 = reinterpret_cast<float *>(h + oT2);
    for (int i = 0; i < n_total; i++) {  // mvnMaxError1/2 as rumi_sim3_ransac forms them
        t1[i] = (float)(size_t)(9.210 * (double)sigma2_1[i]);
        t2[i] = (float)(size_t)(9.210 * (double)sigma2_2[i]);
    }
    std::memcpy(h + oTri, triples, H * 12);
    int32_t *itSol = reinterpret_cast<int32_t *>(h + oIt);
    for (size_t j = 0; j < J; j++) for (int i = 0; i < solvers[j].its; i++) *itSol++ = (int32_t)j;
    HIP_TRY(hipMemcpyAsync(d, h, inBytes, hipMemcpyHostToDevice, nullptr));
    SmsArgs A{};
    A.set = S.view;
    A.sol = (const SmsSolver *)(d + oSol); A.itSol = (const int32_t *)(d + oIt); A.tri = (const int32_t *)(d + oTri);
    A.X1 = (const float *)(d + oX1); A.X2 = (const float *)(d + oX2); A.thr1 = (const float *)(d + oT1); A.thr2 = (const float *)(d + oT2);
    A.nIn = (int32_t *)(S.out.d + rN); A.med = (float *)(S.out.d + rM); A.Tall = (float *)(S.out.d + rT);
    A.rows12 = (float *)(S.work.p + w12); A.rows21 = (float *)(S.work.p + w21); A.Sw = (double *)(S.work.p + wSw); A.cnt = (int32_t *)(S.work.p + wCnt);
    A.ratio = (float *)(S.work.p + wRat);
    A.st = (SmsState *)(d + oSt); A.res = (SmsResult *)(d + oRes);
    size_t chunk = S.chunk > 0 ? (size_t)S.chunk : (size_t)kSmsFirstChunk;
    A.nIter = (int)H;
    volatile const int32_t *seen = reinterpret_cast<volatile const int32_t *>(h + oSt);
    for (size_t g0 = 0, g1; g0 < H; g0 = g1, chunk = S.chunk > 0 ? chunk : std::min<size_t>(2 * chunk, kSmsChunkCap)) {
        g1 = std::min(H, g0 + chunk);
        const unsigned n = (unsigned)(g1 - g0);
        A.g0 = (int)g0; A.g1 = (int)g1;
        hipLaunchKernelGGL(k_sms_hyp, dim3((n + 63) / 64), dim3(64), 0, nullptr, A);
        hipLaunchKernelGGL(k_sms_check, dim3((n + 3) / 4), dim3(256), 0, nullptr, A);
        rc = sms_enqueue_score<true>(A);
        if (rc != RUMI_OK) { (void)hipStreamSynchronize(nullptr); return rc; }      // nothing was copied out: every output is untouched
        hipLaunchKernelGGL(k_sms_select, dim3(1), dim3(64), 0, nullptr, A);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(h + oSt, d + oSt, 16, hipMemcpyDeviceToHost, nullptr));
        HIP_TRY(hipStreamSynchronize(nullptr));
        if (seen[0]) break;                                          // converged: the chunks after it are never enqueued
    }
    const size_t used = (size_t)seen[1];
    HIP_TRY(hipMemcpyAsync(h + oSt, d + oSt, oSol - oSt, hipMemcpyDeviceToHost, nullptr));
    if (n_inliers_all) HIP_TRY(hipMemcpyAsync(S.out.h + rN, S.out.d + rN, used * 4, hipMemcpyDeviceToHost, nullptr));
    if (median_all) HIP_TRY(hipMemcpyAsync(S.out.h + rM, S.out.d + rM, used * 4, hipMemcpyDeviceToHost, nullptr));
    if (T12_all) HIP_TRY(hipMemcpyAsync(S.out.h + rT, S.out.d + rT, used * 64, hipMemcpyDeviceToHost, nullptr));
    HIP_TRY(hipStreamSynchronize(nullptr));
    SmsState end;
    std::memcpy(&end, h + oSt, sizeof end);
    for (size_t j = 0; j < J; j++) if (res0[j].state == RUMI_SIM3_NOT_REACHED) res0[j].bestRatioAfter = end.bestRatio;   // the ratio the call ended with
    std::memcpy(results, res0, J * sizeof(SmsResult));
    *its_consumed = end.consumed;
    // the iterations consumed; the entries after them are not written (the chunks a convergence skipped were never computed)
    if (n_inliers_all) std::memcpy(n_inliers_all, S.out.h + rN, used * 4);
    if (median_all) std::memcpy(median_all, S.out.h + rM, used * 4);
    if (T12_all) std::memcpy(T12_all, S.out.h + rT, used * 64);
    return RUMI_OK;
}
