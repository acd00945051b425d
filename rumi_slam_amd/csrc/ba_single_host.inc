// ba_single_host.inc -- host side of the single-window bundle adjustment (kernels: ba_single.inc, ba_solve_tiles.inc, ba_big.inc, chol_blocked.inc):
// ba_run as named steps and the C entries built on it.  Included by opt.hip after ba_windows_host.inc, which takes the windows of the tile solver.

// Offsets of a window's arrays in the upload block (o->hBa and its device mirror o->dBa) and the two sizes derived from kf_fixed.
// Part A [0, partA) is the caller's data: edges, measurements, initial state.  Part B is the structure: column blocks, edges by landmark, rows by key-frame.
struct BaLayout {
    int nOpt = 0, n = 0;                  // n = 6 nOpt
    size_t oEM = 0, oEK = 0, oOb = 0, oIn = 0, oT = 0, oX = 0, partA = 0, oPC = 0, oPS = 0, oKR = 0, oPE = 0, oRS = 0, upBytes = 0;
};
// How one call solves its reduced system and the launch geometry that goes with it: fixed before the first trial.
struct BaPlan {
    int gE = 1, NP = 16, NT = 1, K3 = 0, nBlocks = 0;   // nBlocks: Schur blocks (segments) of the large-window path
    bool big = false, useTiles = false;
    size_t ldsTiles = 0;
};
// What the LM passes of one call carry from trial to trial.
struct BaLmState { int cur = 0, iters = 0, trials = 0; bool ranChi2 = false, hppFresh = false, gClean = false; };   // cur: index of the current state buffer

// One pinned block up, in two parts.  Part A is converted first and already on its way over PCIe while the host derives part B (g2o buildStructure),
// written straight into the pinned block: two passes over the edges, no temporaries.  The kernels read both parts from the device mirror; the
// initial state is copied on the device into the first of the two state buffers.  tm: host time stamps after part A, its upload, part B's upload.
static int ba_host_structure(RumiOptimizer *o, hipStream_t st, int32_t nKF, const float *kf_pose7, const uint8_t *kf_fixed, int32_t nMP, const float *mp_pos3,
                             int32_t nE, const int32_t *e_mp, const int32_t *e_kf, const float *e_obs, const float *e_inv_sigma2, BaLayout &L, double tm[3]) {
    int nOpt = 0;
    for (int k = 0; k < nKF; k++) nOpt += kf_fixed[k] ? 0 : 1;
    L.nOpt = nOpt; L.n = 6 * nOpt;
    L.oEM = 0; L.oEK = al16(L.oEM + (size_t)nE * 4); L.oOb = al16(L.oEK + (size_t)nE * 4); L.oIn = al16(L.oOb + (size_t)nE * 8);
    L.oT = al16(L.oIn + (size_t)nE * 4); L.oX = al16(L.oT + (size_t)nKF * 64); L.partA = al16(L.oX + (size_t)nMP * 24);
    L.oPC = L.partA; L.oPS = al16(L.oPC + (size_t)nKF * 4); L.oKR = al16(L.oPS + (size_t)(nMP + 1) * 4); L.oPE = al16(L.oKR + (size_t)(nOpt + 1) * 4);
    L.oRS = al16(L.oPE + (size_t)nE * 4); L.upBytes = al16(L.oRS + (size_t)nE * 4);
    if (L.upBytes > o->baStageCap) { g_lastError = "local BA: upload block larger than the optimiser's arenas"; return RUMI_E_CAPACITY; }
    uint8_t *hs = o->hBa;
    int32_t *poseCol = reinterpret_cast<int32_t *>(hs + L.oPC), *ptStart = reinterpret_cast<int32_t *>(hs + L.oPS),
            *kfRowStart = reinterpret_cast<int32_t *>(hs + L.oKR), *ptEdge = reinterpret_cast<int32_t *>(hs + L.oPE),
            *rowSlot = reinterpret_cast<int32_t *>(hs + L.oRS);
    { int c = 0; for (int k = 0; k < nKF; k++) poseCol[k] = kf_fixed[k] ? -1 : c++; }
    // pass 1: validate, count edges per landmark and rows per optimised key-frame
    std::memset(ptStart, 0, (size_t)(nMP + 1) * 4);
    std::memset(kfRowStart, 0, (size_t)(nOpt + 1) * 4);
    for (int e = 0; e < nE; e++) {
        const unsigned mp = (unsigned)e_mp[e], kf = (unsigned)e_kf[e];
        if (mp >= (unsigned)nMP || kf >= (unsigned)nKF) { g_lastError = "local BA: edge index out of range"; return RUMI_E_INVALID; }
        ptStart[mp + 1]++;
        const int c = poseCol[kf];
        if (c >= 0) kfRowStart[c + 1] += 2;
    }
    // part A
    if (nE > 0) {
        std::memcpy(hs + L.oEM, e_mp, (size_t)nE * 4); std::memcpy(hs + L.oEK, e_kf, (size_t)nE * 4);
        std::memcpy(hs + L.oOb, e_obs, (size_t)nE * 8); std::memcpy(hs + L.oIn, e_inv_sigma2, (size_t)nE * 4);
    }
    ba_stage_poses(nKF, kf_pose7, reinterpret_cast<double *>(hs + L.oT));
    double *X0 = reinterpret_cast<double *>(hs + L.oX);
    for (size_t i = 0; i < (size_t)nMP * 3; i++) X0[i] = mp_pos3[i];
    tm[0] = ba_now_us();
    HIP_TRY(hipMemcpyAsync(o->dBa, hs, L.partA, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(o->dT[0], o->dBa + L.oT, (size_t)nKF * 64, hipMemcpyDeviceToDevice, st));
    if (nMP > 0) HIP_TRY(hipMemcpyAsync(o->dX[0], o->dBa + L.oX, (size_t)nMP * 24, hipMemcpyDeviceToDevice, st));
    if (nE > 0) HIP_TRY(hipMemsetAsync(o->dEOff, 0, (size_t)nE, st));
    tm[1] = ba_now_us();
    // part B, pass 2: prefix sums, then every edge into its landmark's list and its key-frame's rows (stable: input order inside a group)
    for (int p2 = 0; p2 < nMP; p2++) ptStart[p2 + 1] += ptStart[p2];
    for (int c = 0; c < nOpt; c++) kfRowStart[c + 1] += kfRowStart[c];
    o->hFill.resize((size_t)nMP + nOpt + 2);
    {
        int32_t *fillP = o->hFill.data(), *fillK = fillP + nMP + 1;
        std::memcpy(fillP, ptStart, (size_t)nMP * 4);
        std::memcpy(fillK, kfRowStart, (size_t)nOpt * 4);
        for (int e = 0; e < nE; e++) {
            ptEdge[fillP[e_mp[e]]++] = e;
            const int c = poseCol[e_kf[e]];
            int slot = -1;
            if (c >= 0) { slot = fillK[c]; fillK[c] = slot + 2; }
            rowSlot[e] = slot;
        }
    }
    HIP_TRY(hipMemcpyAsync(o->dBa + L.partA, hs + L.partA, L.upBytes - L.partA, hipMemcpyHostToDevice, st));
    tm[2] = ba_now_us();
    return RUMI_OK;
}

// the window as the kernels see it: the graph in the device mirror of the upload block, the handle's arenas
static BADev ba_device_view(const RumiOptimizer *o, const BaLayout &L, int mode, int gbaRobust, int32_t nKF, int32_t nMP, int32_t nE, const float *K4) {
    BADev B{};
    B.nKF = nKF; B.nMP = nMP; B.nE = nE; B.nOpt = L.nOpt; B.n = L.n;
    B.eMP = (const int32_t *)(o->dBa + L.oEM); B.eKF = (const int32_t *)(o->dBa + L.oEK); B.poseCol = (const int32_t *)(o->dBa + L.oPC);
    B.ptStart = (const int32_t *)(o->dBa + L.oPS); B.ptEdge = (const int32_t *)(o->dBa + L.oPE); B.rowSlot = (const int32_t *)(o->dBa + L.oRS);
    B.kfRowStart = (const int32_t *)(o->dBa + L.oKR); B.obs = (const float *)(o->dBa + L.oOb); B.info = (const float *)(o->dBa + L.oIn);
    B.cam = DCam{K4[0], K4[1], K4[2], K4[3]};
    B.delta = ba_huber_delta(mode);
    B.dsqr = B.delta * B.delta;
    B.off = o->dEOff; B.robust = mode == 2 ? (gbaRobust ? 1 : 0) : 1;
    B.Hll = o->dHll; B.bl = o->dBl; B.Hpl = o->dHpl; B.panel = o->dPanel; B.Hpp = o->dHpp; B.bp = o->dBp; B.Dinv = o->dDinv;
    B.x = o->dXv; B.lastChi2 = o->dChi; B.scal = o->dScal;
    return B;
}

// Large-window path, once per call (the structure is the same for every trial): the observation pairs of every landmark grouped by Schur block
// (ca, cb <= ca) by a counting sort over the blocks, uploaded behind the block descriptors; the per-edge arrays of the path on first use.
static int ba_big_prepare(RumiOptimizer *o, hipStream_t st, const BaLayout &L, int32_t nMP, int32_t nE, const int32_t *e_kf, int *nBlocksOut) {
    const int nOpt = L.nOpt, n = L.n;
    const int32_t *poseCol = reinterpret_cast<const int32_t *>(o->hBa + L.oPC), *ptStart = reinterpret_cast<const int32_t *>(o->hBa + L.oPS),
                  *ptEdge = reinterpret_cast<const int32_t *>(o->hBa + L.oPE);
    if ((size_t)n * 8 > 120 * 1024) { g_lastError = "bundle adjustment: more than 2560 optimised key-frames"; return RUMI_E_CAPACITY; }
    std::vector<int32_t> colAt((size_t)std::max(nE, 1));             // column block of the t-th entry of ptEdge (-1 fixed)
    for (int t = 0; t < nE; t++) colAt[t] = poseCol[e_kf[ptEdge[t]]];
    std::vector<int64_t> cnt((size_t)nOpt * nOpt + 1, 0);
    auto for_pairs = [&](auto &&f) {
        for (int p = 0; p < nMP; p++) {
            const int t0 = ptStart[p], t1 = ptStart[p + 1];
            for (int ia = t0; ia < t1; ia++) {
                const int ca = colAt[ia];
                if (ca < 0) continue;
                const size_t rowKey = (size_t)ca * nOpt;
                for (int ib = t0; ib < t1; ib++) {
                    const int cb = colAt[ib];
                    if (cb < 0 || cb > ca || (cb == ca && ib != ia)) continue;
                    f(rowKey + cb, ia, ib);
                }
            }
        }
    };
    for_pairs([&](size_t key, int, int) { cnt[key + 1]++; });
    std::vector<int32_t> blk;
    for (size_t key = 0; key < (size_t)nOpt * nOpt; key++) {
        const int64_t c0 = cnt[key], c1 = cnt[key] + cnt[key + 1];
        for (int64_t a0 = c0; a0 < c1; a0 += kSchurSeg) {
            blk.push_back((int32_t)(key / nOpt)); blk.push_back((int32_t)(key % nOpt) | (c1 - c0 > kSchurSeg ? 1 << 30 : 0));
            blk.push_back((int32_t)a0); blk.push_back((int32_t)std::min<int64_t>(a0 + kSchurSeg, c1));
        }
        cnt[key + 1] += cnt[key];
    }
    const int64_t nPairs = cnt[(size_t)nOpt * nOpt];
    if (nPairs > (int64_t)1 << 30) { g_lastError = "bundle adjustment: more than 2^30 co-observation pairs"; return RUMI_E_CAPACITY; }
    std::vector<int32_t> pairs((size_t)std::max<int64_t>(nPairs, 1) * 2);
    for_pairs([&](size_t key, int ia, int ib) { const int64_t at = cnt[key]++; pairs[2 * at] = ptEdge[ia]; pairs[2 * at + 1] = ptEdge[ib]; });
    *nBlocksOut = (int)(blk.size() / 4);
    const size_t need = (blk.size() + pairs.size()) * sizeof(int32_t);
    { const int rcp = o->pairs.reserve(need, need + need / 4); if (rcp != RUMI_OK) return rcp; }
    int32_t *dPairs = reinterpret_cast<int32_t *>(o->pairs.p);
    o->pairOff = blk.size();
    if (!blk.empty()) HIP_TRY(hipMemcpyAsync(dPairs, blk.data(), blk.size() * sizeof(int32_t), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(dPairs + blk.size(), pairs.data(), pairs.size() * sizeof(int32_t), hipMemcpyHostToDevice, st));
    HIP_TRY(hipStreamSynchronize(st));                 // blk / pairs are temporaries
    if (!o->dW) { int rcw = dev_alloc(&o->dW, (size_t)o->maxE * 18); if (rcw == RUMI_OK) rcw = dev_alloc(&o->dColOf, (size_t)o->maxE); if (rcw != RUMI_OK) return rcw; }
    // more than 64 KiB of dynamic LDS needs the opt-in; the limit is process state and only grows (rumi_common.h: raise_lds_limit), so that the
    // worker threads of rumi_local_ba_batch and the facade's per-thread arenas cannot lower it under each other
    if ((size_t)n * 8 > 16 * 1024) HIP_TRY(raise_lds_limit(reinterpret_cast<const void *>(k_chol_backsub), (size_t)n * 8));
    return RUMI_OK;
}

// reduced system of one LM trial of a large window -> B.x, B.scal[3]
static int ba_solve_big(RumiOptimizer *o, hipStream_t st, const BADev &B, const BaPlan &P, double lambda) {
    const int n = B.n, nMP = B.nMP, nE = B.nE;
    double *A = o->dAglob, *rdg = A + (size_t)(n + 1) * n;
    const int ld = n;
    const size_t tot = (size_t)(n + 1) * n;
    hipLaunchKernelGGL(k_big_init, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, st, B, lambda, A, ld);
    if (nMP > 0) {
        BADev Bz = B;
        Bz.n = 0;                                                      // z = L^T b_l lands in dYt[3 p .. 3 p + 2]
        hipLaunchKernelGGL(k_ba_dinv, dim3((nMP + 255) / 256), dim3(256), 0, st, Bz, lambda, o->dYt, 1, o->dLp);
        if (nE > 0) {
            hipLaunchKernelGGL(k_big_w, dim3(P.gE), dim3(256), 0, st, B, o->dLp, o->dW, o->dColOf);
            const int32_t *dPairs = reinterpret_cast<const int32_t *>(o->pairs.p);
            if (P.nBlocks > 0) hipLaunchKernelGGL(k_big_schur, dim3((P.nBlocks + 3) / 4), dim3(256), 0, st, B, dPairs, P.nBlocks, dPairs + o->pairOff, o->dW, o->dYt, A, ld);
        }
    }
    for (int j0 = 0; j0 < n; j0 += kNB) {
        const int w = std::min(kNB, n - j0), rows = n + 1 - (j0 + w);
        hipLaunchKernelGGL(k_chol_diag, dim3(1), dim3(256), 0, st, A, ld, n, j0, rdg, o->dScal);
        if (rows > 0) {
            hipLaunchKernelGGL(k_chol_trsm, dim3((rows + 63) / 64), dim3(256), 0, st, A, ld, n, j0, rdg);
            const int T = (rows + 63) / 64;
            if (j0 + w < n) hipLaunchKernelGGL(k_chol_syrk, dim3(T, T), dim3(256), 0, st, A, ld, n, j0);
        }
    }
    hipLaunchKernelGGL(k_chol_backsub, dim3(1), dim3(1024), (size_t)n * sizeof(double), st, A, ld, n, rdg, o->dXv, o->dScal);
    HIP_TRY(hipGetLastError());
    return RUMI_OK;
}

// g2o optimize(maxIt) (optimization_algorithm_levenberg.cpp:61-169): the LM iterations of one pass, every trial decided on the host from the eight
// published scalars, the stop flag polled between trials.  Accept / reject swaps S.cur between the two state buffers.
static int ba_lm(RumiOptimizer *o, hipStream_t st, const BADev &B, const BaPlan &P, BaLmState &S, int maxIt, const volatile uint8_t *stop_flag) {
    const int nKF = B.nKF, nMP = B.nMP, nE = B.nE, nOpt = B.nOpt, n = B.n, NP = P.NP, NT = P.NT;
    const bool big = P.big, prof = o->profiling;
    const int nSlices = 64;
    int rc = RUMI_OK;
    double lambda = -1, ni = 2;
    int nBad = 0;
    double currentChi = 0;
    for (int it = 0; it < maxIt && !(stop_flag && *stop_flag); it++) {
        // g2o recomputes the active errors here; the value is already known after the first iteration (an accepted trial
        // left it in tempChi, a rejected one did not change the state), so only the first iteration launches the kernel.
        if (it == 0) {
            HIP_TRY(hipMemsetAsync(o->dScal, 0, sizeof(double), st));
            hipLaunchKernelGGL(k_ba_chi2, dim3(P.gE), dim3(256), 0, st, B, o->dT[S.cur], o->dX[S.cur]);
            if ((rc = fetch_published_scalars(o, st)) != RUMI_OK) return rc;
            currentChi = o->hScal[0];
        }
        S.ranChi2 = true;
        const double iniChi = currentChi;
        // buildSystem
        {
            const ZeroList Z{{o->dHll, o->dBl, o->dHpp, o->dBp}, {nMP * 9, nMP * 3, nOpt * 36, n}};
            const int zmax = std::max(std::max(nMP * 9, nOpt * 36), 1);
            hipLaunchKernelGGL(k_ba_zero, dim3((zmax + 255) / 256), dim3(256), 0, st, Z);
        }
        if (nE > 0) hipLaunchKernelGGL(k_ba_build, dim3(P.gE), dim3(256), 0, st, B, o->dT[S.cur], o->dX[S.cur]);
        if (prof) HIP_TRY(hipEventRecord(o->evK[0], st));
        if (nOpt > 0) hipLaunchKernelGGL(k_ba_hpp_mfma, dim3(nOpt, kHppSlices), dim3(256), 0, st, B);
        if (prof) { HIP_TRY(hipEventRecord(o->evK[1], st)); S.hppFresh = true; }
        if (it == 0) {
            HIP_TRY(hipMemsetAsync(o->dScal + 2, 0, sizeof(double), st));
            const int nd = nOpt * 6 + nMP * 3;
            hipLaunchKernelGGL(k_ba_maxdiag, dim3((nd + 255) / 256), dim3(256), 0, st, B);
            if ((rc = fetch_published_scalars(o, st)) != RUMI_OK) return rc;
            lambda = 1e-5 * o->hScal[2]; ni = 2; nBad = 0;
        }
        double rho = 0;
        int qmax = 0;
        do {
            const int trial = S.cur ^ 1;
            if (!P.useTiles || !S.gClean) {                    // k_ba_solve_tiles leaves G and the two accumulators of dScal zeroed itself
                const ZeroList Z{{o->dG, o->dScal, nullptr, nullptr}, {big ? 0 : NP * NP, 2, 0, 0}};
                hipLaunchKernelGGL(k_ba_zero, dim3(((big ? 2 : NP * NP) + 255) / 256), dim3(256), 0, st, Z);
                S.gClean = true;
            }
            if (big) { if ((rc = ba_solve_big(o, st, B, P, lambda)) != RUMI_OK) return rc; }
            else {
                if (nMP > 0) hipLaunchKernelGGL(k_ba_dinv_yfill, dim3((nMP + nE + 255) / 256), dim3(256), 0, st, B, lambda, o->dYt, NP, o->dLp);
                if (prof) HIP_TRY(hipEventRecord(o->evK[2], st));
                if (nMP > 0 && n > 0) hipLaunchKernelGGL(k_ba_syrk_mfma, dim3(NT * (NT + 1) / 2 * (nSlices / 4)), dim3(256), 0, st, o->dYt, P.K3, NP, nSlices, o->dG);
                if (prof) { HIP_TRY(hipEventRecord(o->evK[3], st)); HIP_TRY(hipEventRecord(o->evK[4], st)); }
                if (n > 0) {
                    if (P.useTiles) hipLaunchKernelGGL(k_ba_solve_tiles, dim3(1), dim3(kSolveThreads), P.ldsTiles, st, B, lambda, o->dG, NP);
                    else hipLaunchKernelGGL(k_ba_solve, dim3(1), dim3(1024), 0, st, B, lambda, o->dG, NP, o->dAglob);
                }
                else HIP_TRY(hipMemsetAsync(o->dScal + 3, 0, sizeof(double), st));
                if (prof) HIP_TRY(hipEventRecord(o->evK[5], st));
            }
            hipLaunchKernelGGL(k_ba_update, dim3(((nMP + nKF) * kLmLanes + 255) / 256), dim3(256), 0, st, B, lambda, o->dT[S.cur], o->dX[S.cur], o->dT[trial], o->dX[trial]);
            hipLaunchKernelGGL(k_ba_chi2, dim3(P.gE), dim3(256), 0, st, B, o->dT[trial], o->dX[trial]);
            HIP_TRY(hipGetLastError());
            if (prof) HIP_TRY(hipStreamSynchronize(st));              // the event pairs below must have completed
            if ((rc = fetch_published_scalars(o, st)) != RUMI_OK) return rc;
            if (prof && !big) {
                float ms;
                if (S.hppFresh) { HIP_TRY(hipEventElapsedTime(&ms, o->evK[0], o->evK[1])); o->kernelMs[0] += ms; S.hppFresh = false; }
                HIP_TRY(hipEventElapsedTime(&ms, o->evK[2], o->evK[3])); o->kernelMs[1] += ms;
                HIP_TRY(hipEventElapsedTime(&ms, o->evK[4], o->evK[5])); o->kernelMs[2] += ms;
                o->kernelMs[3] += 1.f;
            }
            const bool ok2 = n == 0 || o->hScal[3] != 0.0;
            double tempChi = o->hScal[0];
            if (!ok2) tempChi = std::numeric_limits<double>::max();
            rho = currentChi - tempChi;
            const double scale = o->hScal[1] + 1e-3;
            rho /= scale;
            if (rho > 0 && std::isfinite(tempChi)) {
                double alpha = 1. - std::pow((2 * rho - 1), 3);
                alpha = std::min(alpha, 2. / 3.);
                lambda *= std::max(1. / 3., alpha);
                ni = 2;
                currentChi = tempChi;
                S.cur = trial;                     // discardTop(): the trial state becomes the estimate
            } else {
                lambda *= ni;
                ni *= 2;                           // pop(): keep the current state
            }
            qmax++;
            S.trials++;
        } while (rho < 0 && qmax < 10 && !(stop_flag && *stop_flag));
        S.iters++;
        if (qmax == 10 || rho == 0) break;
        if ((iniChi - currentChi) * 1e3 < iniChi) nBad++; else nBad = 0;
        if (nBad >= 3) break;
    }
    return RUMI_OK;
}

// mode 0: Optimizer::LocalBundleAdjustment(KeyFrame*, bool*, Map*, ...) — one optimize(10) with Huber(sqrt(5.991)).
// mode 1: Optimizer::LocalBundleAdjustment(KeyFrame *pMainKF, vpAdjustKF, vpFixedKF, bool*) (merge window, Optimizer.cc:3768-4183) —
//         optimize(5) with Huber(sqrt(5.99)); unless stopped: outlier edges to level 1, kernels off, initializeOptimization(0) +
//         optimize(10); the erase test reads every edge's stored error (level-1 edges: the one they had when they left).
// mode 2: Optimizer::BundleAdjustment(vpKFs, vpMP, nIterations, pbStopFlag, nLoopKF, bRobust) (Optimizer.cc:54-351, monocular edges) —
//         one optimize(nIterations), Huber(sqrt(5.99)) only if bRobust.
static int ba_run(RumiOptimizer *o, int mode, int32_t nKF, float *kf_pose7, const uint8_t *kf_fixed, int32_t nMP, float *mp_pos3,
                  int32_t nE, const int32_t *e_mp, const int32_t *e_kf, const float *e_obs, const float *e_inv_sigma2,
                  const float *K4, const volatile uint8_t *stop_flag, uint8_t *erase_out, int32_t *stats, int gbaIterations = 0, int gbaRobust = 1) {
    if (!o || nKF < 1 || nMP < 0 || nE < 0 || !kf_pose7 || !kf_fixed || !K4 || (nMP > 0 && !mp_pos3) ||
        (nE > 0 && (!e_mp || !e_kf || !e_obs || !e_inv_sigma2 || !erase_out)))
        return RUMI_E_INVALID;
    if (nKF > o->maxKF || nMP > o->maxMP || nE > o->maxE) { g_lastError = "local BA: problem larger than the optimiser's arenas"; return RUMI_E_CAPACITY; }
    // windows the tile solver takes (up to 29 optimised key-frames): the window-batched kernels, as a batch of one
    if (baw_eligible(o, nKF, kf_fixed, nMP, nE) && !(mode == 2 && (gbaIterations < 1 || (stop_flag && *stop_flag)))) {
        const BawArgs a{nKF, kf_pose7, kf_fixed, nMP, mp_pos3, nE, e_mp, e_kf, e_obs, e_inv_sigma2, K4, stop_flag, erase_out, stats};
        RumiOptimizer *arena = o;
        int32_t status = RUMI_OK;
        const int rc = baw_run(o, mode, 1, &a, &arena, gbaIterations, gbaRobust, &status);
        return rc != RUMI_OK ? rc : status;
    }
    int rc;
    if (ba_early_exit(mode, nKF, kf_fixed, stop_flag, stats, &rc)) return rc;
    HIP_TRY(hipSetDevice(o->device));
    // everything of a bundle adjustment runs on the handle's own (non-blocking) stream: handles on different host threads overlap on the device
    // (rumi_local_ba_batch; Tracking / LocalMapping / LoopClosing threads with their thread-local arenas)
    hipStream_t st = o->stream;
    static const bool hostDbg = std::getenv("RUMI_HOSTDBG") != nullptr;
    const double tA = ba_now_us();
    BaLayout L;
    double tm[3] = {tA, tA, tA};   // tB, tC, tD of the line below
    if ((rc = ba_host_structure(o, st, nKF, kf_pose7, kf_fixed, nMP, mp_pos3, nE, e_mp, e_kf, e_obs, e_inv_sigma2, L, tm)) != RUMI_OK) return rc;
    BADev B = ba_device_view(o, L, mode, gbaRobust, nKF, nMP, nE, K4);
    const int nOpt = L.nOpt, n = L.n;
    // The reduced pose system of a trial.  Up to 175 unknowns (29 optimised key-frames; here only on a profiled handle or with more than 512 key-frames):
    // dense Schur panel on the matrix cores + k_ba_solve_tiles.  180..252 unknowns (30..42): the same panel + k_ba_solve (one workgroup, matrix in L2).
    // More than 255 (43 and more): block-sparse Schur accumulation + multi-workgroup blocked Cholesky (ba_solve_big).
    BaPlan P;
    P.gE = std::max(1, (nE + 255) / 256);
    P.big = n > 255;
    P.NP = P.big ? 16 : (n + 1 + 15) / 16 * 16; P.NT = P.NP / 16; P.K3 = 3 * nMP;
    if (!P.big && P.NP > o->npCap) { g_lastError = "local BA: reduced system larger than the optimiser's arenas"; return RUMI_E_CAPACITY; }
    if (P.big && (rc = ba_big_prepare(o, st, L, nMP, nE, e_kf, &P.nBlocks)) != RUMI_OK) return rc;
    P.ldsTiles = ((size_t)(P.NT * (P.NT + 1) / 2) * 256 + (size_t)P.NT * 16) * sizeof(double);
    P.useTiles = !P.big && n > 0 && P.NT <= kSolveTilesMax;
    if (P.useTiles && P.ldsTiles > 48 * 1024) HIP_TRY(raise_lds_limit(reinterpret_cast<const void *>(k_ba_solve_tiles), P.ldsTiles));
    if (nMP > 0 && !P.big) HIP_TRY(hipMemsetAsync(o->dYt, 0, (size_t)P.K3 * P.NP * sizeof(double), st));   // pattern of Y is fixed: zero once, live entries are rewritten per trial
    HIP_TRY(hipEventRecord(o->ev[0], st));
    for (auto &k : o->kernelMs) k = 0.f;
    BaLmState S;
    const double tE = ba_now_us();
    if ((rc = ba_lm(o, st, B, P, S, mode == 0 ? 10 : mode == 1 ? 5 : gbaIterations, stop_flag)) != RUMI_OK) return rc;
    const double tF = ba_now_us();
    const int itersFirst = S.iters;
    if (mode == 1 && !(stop_flag && *stop_flag)) {          // bDoMore
        if (nE > 0 && S.ranChi2) hipLaunchKernelGGL(k_ba_mark, dim3(P.gE), dim3(256), 0, st, B, o->dT[S.cur], o->dX[S.cur], o->dEOff);
        B.robust = 0;
        if ((rc = ba_lm(o, st, B, P, S, 10, stop_flag)) != RUMI_OK) return rc;
    }
    // results gathered by the last kernel into one block and read back with one copy: [T | X | erase]
    const size_t rT = 0, rX = al16(rT + (size_t)nKF * 64), rE = al16(rX + (size_t)nMP * 24), dnBytes = al16(rE + (size_t)nE);
    const int gF = std::max(P.gE, std::max((nKF * 8 + 255) / 256, (nMP * 3 + 255) / 256));
    hipLaunchKernelGGL(k_ba_finalize, dim3(gF), dim3(256), 0, st, B, o->dT[S.cur], o->dX[S.cur], S.ranChi2 ? 1 : 0, o->dBaOut + rE, reinterpret_cast<double *>(o->dBaOut + rT),
                       reinterpret_cast<double *>(o->dBaOut + rX));
    HIP_TRY(hipEventRecord(o->ev[1], st));
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(o->hBa, o->dBaOut, dnBytes, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    HIP_TRY(hipEventElapsedTime(&o->stageMs[5], o->ev[0], o->ev[1]));
    ba_unpack(nKF, kf_fixed, nMP, nE, reinterpret_cast<const double *>(o->hBa + rT), reinterpret_cast<const double *>(o->hBa + rX), o->hBa + rE,
              kf_pose7, mp_pos3, erase_out);
    ba_write_stats(mode, S.iters, itersFirst, S.trials, nOpt, stats);
    if (hostDbg) fprintf(stderr, "ba host us: pass1+partA %.1f h2d-A %.1f pass2+h2d-B %.1f setup %.1f lm %.1f tail %.1f\n", tm[0] - tA, tm[1] - tm[0], tm[2] - tm[1], tE - tm[2], tF - tE, ba_now_us() - tF);
    return RUMI_OK;
}

extern "C" int rumi_local_ba(RumiOptimizer *o, int32_t nKF, float *kf_pose7, const uint8_t *kf_fixed, int32_t nMP, float *mp_pos3,
                             int32_t nE, const int32_t *e_mp, const int32_t *e_kf, const float *e_obs, const float *e_inv_sigma2,
                             const float *K4, const volatile uint8_t *stop_flag, uint8_t *erase_out, int32_t *stats) {
    return ba_run(o, 0, nKF, kf_pose7, kf_fixed, nMP, mp_pos3, nE, e_mp, e_kf, e_obs, e_inv_sigma2, K4, stop_flag, erase_out, stats);
}

// R independent local windows (the only multi-window form local BA has: a window does not shard, SURVEY section 8e).  n_workers host threads, each
// with a child handle of its own (own stream, own arenas, created on first use and kept), take the windows from a shared counter: while one
// window's host thread waits for the eight scalars of an LM trial, the kernels of the others fill the device.
extern "C" int rumi_local_ba_batch(RumiOptimizer *o, int32_t n_windows, RumiBaWindow *win, int32_t n_workers) {
    if (!o || n_windows < 0 || (n_windows > 0 && !win) || n_workers < 1) return RUMI_E_INVALID;
    if (n_windows == 0) return RUMI_OK;
    auto need_children = [&](int cnt) -> int {
        while ((int)o->workers.size() < cnt) {
            RumiOptimizer *c = nullptr;
            const int rc = rumi_opt_create(o->maxPoseEdges, 1, o->maxKF, o->maxMP, o->maxE, o->device, &c);
            if (rc != RUMI_OK) return rc;
            o->workers.push_back(c);
        }
        return RUMI_OK;
    };
    // windows of up to 29 optimised key-frames: the window is a batch dimension of the kernels (ba_windows.inc), driven by THIS thread alone, in
    // groups of kBawMaxWindows; a child handle per window of a group lends its arenas
    std::vector<int> batched, others;
    for (int i = 0; i < n_windows; i++) {
        const RumiBaWindow &W = win[i];
        const bool ok = W.kf_pose7 && W.kf_fixed && W.K4 && W.mp_pos3 && W.e_mp && W.e_kf && W.e_obs && W.e_inv_sigma2 && W.erase_out &&
                        W.n_kf <= o->maxKF && W.n_mp <= o->maxMP && W.n_edges <= o->maxE && baw_eligible(o, W.n_kf, W.kf_fixed, W.n_mp, W.n_edges);
        (ok ? batched : others).push_back(i);
    }
    for (size_t g0 = 0; g0 < batched.size(); g0 += kBawMaxWindows) {
        const int cnt = (int)std::min<size_t>(kBawMaxWindows, batched.size() - g0);
        { const int rc = need_children(cnt); if (rc != RUMI_OK) return rc; }
        std::vector<BawArgs> args((size_t)cnt);
        std::vector<int32_t> status((size_t)cnt, RUMI_OK);
        for (int j = 0; j < cnt; j++) {
            RumiBaWindow &W = win[batched[g0 + j]];
            args[j] = BawArgs{W.n_kf, W.kf_pose7, W.kf_fixed, W.n_mp, W.mp_pos3, W.n_edges, W.e_mp, W.e_kf, W.e_obs, W.e_inv_sigma2, W.K4, W.stop_flag, W.erase_out, W.stats};
        }
        // launch groups (two from 8 windows on, three from 12: baw_run): the parent handle lends the first its stream and window table, further children the others
        { const int rc = need_children(cnt + 3); if (rc != RUMI_OK) return rc; }
        RumiOptimizer *runners[4] = {o, o->workers[cnt], o->workers[cnt + 1], o->workers[cnt + 2]};
        const int rc = baw_run(o, 0, cnt, args.data(), o->workers.data(), 0, 1, status.data(), runners, 4);
        for (int j = 0; j < cnt; j++) win[batched[g0 + j]].status = status[j];
        if (rc != RUMI_OK && rc != RUMI_E_INVALID && rc != RUMI_E_CAPACITY) return rc;      // a HIP failure: nothing more to run
    }
    // everything else (larger windows, windows of more than 512 key-frames, structure-only windows, the profiled path): one single-window run each, over worker threads as before
    if (!others.empty()) {
        n_workers = std::min(std::min(n_workers, (int)others.size()), 16);
        { const int rc = need_children(n_workers); if (rc != RUMI_OK) return rc; }
        std::atomic<int> next{0};
        auto work = [&](RumiOptimizer *c) {
            for (int q = next.fetch_add(1); q < (int)others.size(); q = next.fetch_add(1)) {
                RumiBaWindow &W = win[others[q]];
                W.status = ba_run(c, 0, W.n_kf, W.kf_pose7, W.kf_fixed, W.n_mp, W.mp_pos3, W.n_edges, W.e_mp, W.e_kf, W.e_obs, W.e_inv_sigma2, W.K4, W.stop_flag,
                                  W.erase_out, W.stats);
            }
        };
        std::vector<std::thread> th;
        for (int k = 1; k < n_workers; k++) th.emplace_back(work, o->workers[k]);
        work(o->workers[0]);
        for (auto &t : th) t.join();
    }
    int worst = RUMI_OK;
    for (int i = 0; i < n_windows; i++) if (win[i].status != RUMI_OK) worst = win[i].status;
    return worst;
}

extern "C" int rumi_bundle_adjustment(RumiOptimizer *o, int32_t nKF, float *kf_pose7, const uint8_t *kf_fixed, int32_t nMP, float *mp_pos3,
                                      int32_t nE, const int32_t *e_mp, const int32_t *e_kf, const float *e_obs, const float *e_inv_sigma2,
                                      const float *K4, const volatile uint8_t *stop_flag, int32_t n_iterations, int32_t robust, int32_t *stats) {
    if (n_iterations < 0) return RUMI_E_INVALID;
    std::vector<uint8_t> erase((size_t)std::max(nE, 1));
    return ba_run(o, 2, nKF, kf_pose7, kf_fixed, nMP, mp_pos3, nE, e_mp, e_kf, e_obs, e_inv_sigma2, K4, stop_flag, erase.data(), stats, n_iterations, robust);
}

extern "C" int rumi_merge_ba(RumiOptimizer *o, int32_t nKF, float *kf_pose7, const uint8_t *kf_fixed, int32_t nMP, float *mp_pos3,
                             int32_t nE, const int32_t *e_mp, const int32_t *e_kf, const float *e_obs, const float *e_inv_sigma2,
                             const float *K4, const volatile uint8_t *stop_flag, uint8_t *erase_out, int32_t *stats) {
    return ba_run(o, 1, nKF, kf_pose7, kf_fixed, nMP, mp_pos3, nE, e_mp, e_kf, e_obs, e_inv_sigma2, K4, stop_flag, erase_out, stats);
}
