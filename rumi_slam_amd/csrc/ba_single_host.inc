// ba_single_host.inc -- host side of the single-window bundle adjustment (kernels: ba_single.inc, ba_solve_tiles.inc, ba_big.inc, chol_blocked.inc):
// ba_run as named steps and the C entries built on it.  Included by opt.hip after ba_windows_host.inc, which takes the windows of the tile solver.

// Offsets of a window's arrays in the upload block (the arena's `stage`: pinned half and device half) and the two sizes derived from kf_fixed.
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
static int ba_host_structure(BaArena &a, hipStream_t st, int32_t nKF, const float *kf_pose7, const uint8_t *kf_fixed, int32_t nMP, const float *mp_pos3,
                             int32_t nE, const int32_t *e_mp, const int32_t *e_kf, const float *e_obs, const float *e_inv_sigma2, BaLayout &L, double tm[3]) {
    int nOpt = 0;
    for (int k = 0; k < nKF; k++) nOpt += kf_fixed[k] ? 0 : 1;
    L.nOpt = nOpt; L.n = 6 * nOpt;
    L.oEM = 0; L.oEK = al16(L.oEM + (size_t)nE * 4); L.oOb = al16(L.oEK + (size_t)nE * 4); L.oIn = al16(L.oOb + (size_t)nE * 8);
    L.oT = al16(L.oIn + (size_t)nE * 4); L.oX = al16(L.oT + (size_t)nKF * 64); L.partA = al16(L.oX + (size_t)nMP * 24);
    L.oPC = L.partA; L.oPS = al16(L.oPC + (size_t)nKF * 4); L.oKR = al16(L.oPS + (size_t)(nMP + 1) * 4); L.oPE = al16(L.oKR + (size_t)(nOpt + 1) * 4);
    L.oRS = al16(L.oPE + (size_t)nE * 4); L.upBytes = al16(L.oRS + (size_t)nE * 4);
    if (L.upBytes > a.stage.cap) { g_lastError = "local BA: upload block larger than the optimiser's arenas"; return RUMI_E_CAPACITY; }
    uint8_t *hs = a.stage.h;
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
    HIP_TRY(hipMemcpyAsync(a.stage.d, hs, L.partA, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(a.T[0].p, a.stage.d + L.oT, (size_t)nKF * 64, hipMemcpyDeviceToDevice, st));
    if (nMP > 0) HIP_TRY(hipMemcpyAsync(a.X[0].p, a.stage.d + L.oX, (size_t)nMP * 24, hipMemcpyDeviceToDevice, st));
    if (nE > 0) HIP_TRY(hipMemsetAsync(a.eOff.p, 0, (size_t)nE, st));
    tm[1] = ba_now_us();
    // part B, pass 2: prefix sums, then every edge into its landmark's list and its key-frame's rows (stable: input order inside a group)
    for (int p2 = 0; p2 < nMP; p2++) ptStart[p2 + 1] += ptStart[p2];
    for (int c = 0; c < nOpt; c++) kfRowStart[c + 1] += kfRowStart[c];
    a.solo.fill.resize((size_t)nMP + nOpt + 2);
    {
        int32_t *fillP = a.solo.fill.data(), *fillK = fillP + nMP + 1;
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
    HIP_TRY(hipMemcpyAsync(a.stage.d + L.partA, hs + L.partA, L.upBytes - L.partA, hipMemcpyHostToDevice, st));
    tm[2] = ba_now_us();
    return RUMI_OK;
}

// the window as the kernels see it: the graph in the device mirror of the upload block, the handle's arenas
static BADev ba_device_view(const BaArena &a, const BaLayout &L, int mode, int gbaRobust, int32_t nKF, int32_t nMP, int32_t nE, const float *K4) {
    BADev B{};
    B.nKF = nKF; B.nMP = nMP; B.nE = nE; B.nOpt = L.nOpt; B.n = L.n;
    B.eMP = (const int32_t *)(a.stage.d + L.oEM); B.eKF = (const int32_t *)(a.stage.d + L.oEK); B.poseCol = (const int32_t *)(a.stage.d + L.oPC);
    B.ptStart = (const int32_t *)(a.stage.d + L.oPS); B.ptEdge = (const int32_t *)(a.stage.d + L.oPE); B.rowSlot = (const int32_t *)(a.stage.d + L.oRS);
    B.kfRowStart = (const int32_t *)(a.stage.d + L.oKR); B.obs = (const float *)(a.stage.d + L.oOb); B.info = (const float *)(a.stage.d + L.oIn);
    B.cam = DCam{K4[0], K4[1], K4[2], K4[3]};
    B.delta = ba_huber_delta(mode);
    B.dsqr = B.delta * B.delta;
    B.off = a.eOff.p; B.robust = mode == 2 ? (gbaRobust ? 1 : 0) : 1;
    B.Hll = a.solo.Hll.p; B.bl = a.bl.p; B.Hpl = a.solo.Hpl.p; B.panel = a.panel.p; B.Hpp = a.Hpp.p; B.bp = a.bp.p; B.Dinv = a.Dinv.p;
    B.x = a.xv.p; B.lastChi2 = a.chi.p; B.scal = a.solo.scal.p;
    return B;
}

// Large-window path, once per call (the structure is the same for every trial): the observation pairs of every landmark grouped by Schur block
// (ca, cb <= ca) by a counting sort over the blocks, uploaded behind the block descriptors; the per-edge arrays of the path on first use.
static int ba_big_prepare(BaArena &a, hipStream_t st, const BaLayout &L, int32_t nMP, int32_t nE, const int32_t *e_kf, int *nBlocksOut) {
    const int nOpt = L.nOpt, n = L.n;
    const int32_t *poseCol = reinterpret_cast<const int32_t *>(a.stage.h + L.oPC), *ptStart = reinterpret_cast<const int32_t *>(a.stage.h + L.oPS),
                  *ptEdge = reinterpret_cast<const int32_t *>(a.stage.h + L.oPE);
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
    { const int rcp = a.solo.pairs.reserve(need, need + need / 4); if (rcp != RUMI_OK) return rcp; }
    int32_t *dPairs = reinterpret_cast<int32_t *>(a.solo.pairs.p);
    a.solo.pairOff = blk.size();
    if (!blk.empty()) HIP_TRY(hipMemcpyAsync(dPairs, blk.data(), blk.size() * sizeof(int32_t), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(dPairs + blk.size(), pairs.data(), pairs.size() * sizeof(int32_t), hipMemcpyHostToDevice, st));
    HIP_TRY(hipStreamSynchronize(st));                 // blk / pairs are temporaries
    { int rcw = RUMI_OK; take(rcw, a.solo.W, (size_t)a.maxE * 18); take(rcw, a.solo.colOf, (size_t)a.maxE); if (rcw != RUMI_OK) return rcw; }
    // more than 64 KiB of dynamic LDS needs the opt-in; the limit is process state and only grows (rumi_common.h: raise_lds_limit), so that the
    // worker threads of rumi_local_ba_batch and the facade's per-thread arenas cannot lower it under each other
    if ((size_t)n * 8 > 16 * 1024) HIP_TRY(raise_lds_limit(reinterpret_cast<const void *>(k_chol_backsub), (size_t)n * 8));
    return RUMI_OK;
}

// reduced system of one LM trial of a large window -> B.x, B.scal[3]
static int ba_solve_big(BaArena &a, hipStream_t st, const BADev &B, const BaPlan &P, double lambda) {
    const int n = B.n, nMP = B.nMP, nE = B.nE;
    double *A = a.solo.Aglob.p, *rdg = A + (size_t)(n + 1) * n;
    const int ld = n;
    const size_t tot = (size_t)(n + 1) * n;
    hipLaunchKernelGGL(k_big_init, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, st, B, lambda, A, ld);
    if (nMP > 0) {
        BADev Bz = B;
        Bz.n = 0;                                                      // z = L^T b_l lands in dYt[3 p .. 3 p + 2]
        hipLaunchKernelGGL(k_ba_dinv, dim3((nMP + 255) / 256), dim3(256), 0, st, Bz, lambda, a.solo.Yt.p, 1, a.solo.Lp.p);
        if (nE > 0) {
            hipLaunchKernelGGL(k_big_w, dim3(P.gE), dim3(256), 0, st, B, a.solo.Lp.p, a.solo.W.p, a.solo.colOf.p);
            const int32_t *dPairs = reinterpret_cast<const int32_t *>(a.solo.pairs.p);
            if (P.nBlocks > 0) hipLaunchKernelGGL(k_big_schur, dim3((P.nBlocks + 3) / 4), dim3(256), 0, st, B, dPairs, P.nBlocks, dPairs + a.solo.pairOff, a.solo.W.p, a.solo.Yt.p, A, ld);
        }
    }
    for (int j0 = 0; j0 < n; j0 += kNB) {
        const int w = std::min(kNB, n - j0), rows = n + 1 - (j0 + w);
        hipLaunchKernelGGL(k_chol_diag, dim3(1), dim3(256), 0, st, A, ld, n, j0, rdg, a.solo.scal.p);
        if (rows > 0) {
            hipLaunchKernelGGL(k_chol_trsm, dim3((rows + 63) / 64), dim3(256), 0, st, A, ld, n, j0, rdg);
            const int T = (rows + 63) / 64;
            if (j0 + w < n) hipLaunchKernelGGL(k_chol_syrk, dim3(T, T), dim3(256), 0, st, A, ld, n, j0);
        }
    }
    hipLaunchKernelGGL(k_chol_backsub, dim3(1), dim3(1024), (size_t)n * sizeof(double), st, A, ld, n, rdg, a.xv.p, a.solo.scal.p);
    HIP_TRY(hipGetLastError());
    return RUMI_OK;
}

// g2o optimize(maxIt) (optimization_algorithm_levenberg.cpp:61-169): the LM iterations of one pass, every trial decided on the host from the eight
// published scalars, the stop flag polled between trials.  Accept / reject swaps S.cur between the two state buffers.
static int ba_lm(BaArena &a, BaProfile *pf, hipStream_t st, const BADev &B, const BaPlan &P, BaLmState &S, int maxIt, const volatile uint8_t *stop_flag) {
    const int nKF = B.nKF, nMP = B.nMP, nE = B.nE, nOpt = B.nOpt, n = B.n, NP = P.NP, NT = P.NT;
    const bool big = P.big, prof = pf != nullptr;
    const int nSlices = 64;
    int rc = RUMI_OK;
    double lambda = -1, ni = 2;
    int nBad = 0;
    double currentChi = 0;
    for (int it = 0; it < maxIt && !(stop_flag && *stop_flag); it++) {
        // g2o recomputes the active errors here; the value is already known after the first iteration (an accepted trial
        // left it in tempChi, a rejected one did not change the state), so only the first iteration launches the kernel.
        if (it == 0) {
            HIP_TRY(hipMemsetAsync(a.solo.scal.p, 0, sizeof(double), st));
            hipLaunchKernelGGL(k_ba_chi2, dim3(P.gE), dim3(256), 0, st, B, a.T[S.cur].p, a.X[S.cur].p);
            if ((rc = fetch_published_scalars(a.solo, st)) != RUMI_OK) return rc;
            currentChi = a.solo.pub.h[0];
        }
        S.ranChi2 = true;
        const double iniChi = currentChi;
        // buildSystem
        {
            const ZeroList Z{{a.solo.Hll.p, a.bl.p, a.Hpp.p, a.bp.p}, {nMP * 9, nMP * 3, nOpt * 36, n}};
            const int zmax = std::max(std::max(nMP * 9, nOpt * 36), 1);
            hipLaunchKernelGGL(k_ba_zero, dim3((zmax + 255) / 256), dim3(256), 0, st, Z);
        }
        if (nE > 0) hipLaunchKernelGGL(k_ba_build, dim3(P.gE), dim3(256), 0, st, B, a.T[S.cur].p, a.X[S.cur].p);
        if (prof) HIP_TRY(hipEventRecord(pf->ev[0], st));
        if (nOpt > 0) hipLaunchKernelGGL(k_ba_hpp_mfma, dim3(nOpt, kHppSlices), dim3(256), 0, st, B);
        if (prof) { HIP_TRY(hipEventRecord(pf->ev[1], st)); S.hppFresh = true; }
        if (it == 0) {
            HIP_TRY(hipMemsetAsync(a.solo.scal.p + 2, 0, sizeof(double), st));
            const int nd = nOpt * 6 + nMP * 3;
            hipLaunchKernelGGL(k_ba_maxdiag, dim3((nd + 255) / 256), dim3(256), 0, st, B);
            if ((rc = fetch_published_scalars(a.solo, st)) != RUMI_OK) return rc;
            lambda = 1e-5 * a.solo.pub.h[2]; ni = 2; nBad = 0;
        }
        double rho = 0;
        int qmax = 0;
        do {
            const int trial = S.cur ^ 1;
            if (!P.useTiles || !S.gClean) {                    // k_ba_solve_tiles leaves G and the two accumulators of dScal zeroed itself
                const ZeroList Z{{a.solo.G.p, a.solo.scal.p, nullptr, nullptr}, {big ? 0 : NP * NP, 2, 0, 0}};
                hipLaunchKernelGGL(k_ba_zero, dim3(((big ? 2 : NP * NP) + 255) / 256), dim3(256), 0, st, Z);
                S.gClean = true;
            }
            if (big) { if ((rc = ba_solve_big(a, st, B, P, lambda)) != RUMI_OK) return rc; }
            else {
                if (nMP > 0) hipLaunchKernelGGL(k_ba_dinv_yfill, dim3((nMP + nE + 255) / 256), dim3(256), 0, st, B, lambda, a.solo.Yt.p, NP, a.solo.Lp.p);
                if (prof) HIP_TRY(hipEventRecord(pf->ev[2], st));
                if (nMP > 0 && n > 0) hipLaunchKernelGGL(k_ba_syrk_mfma, dim3(NT * (NT + 1) / 2 * (nSlices / 4)), dim3(256), 0, st, a.solo.Yt.p, P.K3, NP, nSlices, a.solo.G.p);
                if (prof) { HIP_TRY(hipEventRecord(pf->ev[3], st)); HIP_TRY(hipEventRecord(pf->ev[4], st)); }
                if (n > 0) {
                    if (P.useTiles) hipLaunchKernelGGL(k_ba_solve_tiles, dim3(1), dim3(kSolveThreads), P.ldsTiles, st, B, lambda, a.solo.G.p, NP);
                    else hipLaunchKernelGGL(k_ba_solve, dim3(1), dim3(1024), 0, st, B, lambda, a.solo.G.p, NP, a.solo.Aglob.p);
                }
                else HIP_TRY(hipMemsetAsync(a.solo.scal.p + 3, 0, sizeof(double), st));
                if (prof) HIP_TRY(hipEventRecord(pf->ev[5], st));
            }
            hipLaunchKernelGGL(k_ba_update, dim3(((nMP + nKF) * kLmLanes + 255) / 256), dim3(256), 0, st, B, lambda, a.T[S.cur].p, a.X[S.cur].p, a.T[trial].p, a.X[trial].p);
            hipLaunchKernelGGL(k_ba_chi2, dim3(P.gE), dim3(256), 0, st, B, a.T[trial].p, a.X[trial].p);
            HIP_TRY(hipGetLastError());
            if (prof) HIP_TRY(hipStreamSynchronize(st));              // the event pairs below must have completed
            if ((rc = fetch_published_scalars(a.solo, st)) != RUMI_OK) return rc;
            if (prof && !big) {
                float ms;
                if (S.hppFresh) { HIP_TRY(hipEventElapsedTime(&ms, pf->ev[0], pf->ev[1])); pf->kernelMs[0] += ms; S.hppFresh = false; }
                HIP_TRY(hipEventElapsedTime(&ms, pf->ev[2], pf->ev[3])); pf->kernelMs[1] += ms;
                HIP_TRY(hipEventElapsedTime(&ms, pf->ev[4], pf->ev[5])); pf->kernelMs[2] += ms;
                pf->kernelMs[3] += 1.f;
            }
            const bool ok2 = n == 0 || a.solo.pub.h[3] != 0.0;
            double tempChi = a.solo.pub.h[0];
            if (!ok2) tempChi = std::numeric_limits<double>::max();
            rho = currentChi - tempChi;
            const double scale = a.solo.pub.h[1] + 1e-3;
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
// `cp`: the context the window runs in; `prof`: the handle's profile, null in a worker context (never profiled).
static int ba_run(BaContext *cp, BaProfile *prof, int mode, int32_t nKF, float *kf_pose7, const uint8_t *kf_fixed, int32_t nMP, float *mp_pos3,
                  int32_t nE, const int32_t *e_mp, const int32_t *e_kf, const float *e_obs, const float *e_inv_sigma2,
                  const float *K4, const volatile uint8_t *stop_flag, uint8_t *erase_out, int32_t *stats, int gbaIterations = 0, int gbaRobust = 1) {
    if (!cp || nKF < 1 || nMP < 0 || nE < 0 || !kf_pose7 || !kf_fixed || !K4 || (nMP > 0 && !mp_pos3) ||
        (nE > 0 && (!e_mp || !e_kf || !e_obs || !e_inv_sigma2 || !erase_out)))
        return RUMI_E_INVALID;
    BaContext &c = *cp;
    BaArena &a = c.arena;
    if (nKF > a.maxKF || nMP > a.maxMP || nE > a.maxE) { g_lastError = "local BA: problem larger than the optimiser's arenas"; return RUMI_E_CAPACITY; }
    // windows the tile solver takes (up to 29 optimised key-frames): the window-batched kernels, as a batch of one
    if (baw_eligible(prof && prof->on, nKF, kf_fixed, nMP, nE) && !(mode == 2 && (gbaIterations < 1 || (stop_flag && *stop_flag)))) {
        const BawArgs w{nKF, kf_pose7, kf_fixed, nMP, mp_pos3, nE, e_mp, e_kf, e_obs, e_inv_sigma2, K4, stop_flag, erase_out, stats};
        BaRunner *runner = &c.run;
        int32_t status = RUMI_OK;
        const int rc = baw_run(mode, 1, &w, &a, gbaIterations, gbaRobust, &status, &runner, 1);
        return rc != RUMI_OK ? rc : status;
    }
    int rc;
    if (ba_early_exit(mode, nKF, kf_fixed, stop_flag, stats, &rc)) return rc;
    HIP_TRY(hipSetDevice(c.run.device));
    // everything of a bundle adjustment runs on the runner's own (non-blocking) stream: handles on different host threads overlap on the device
    // (rumi_local_ba_batch; Tracking / LocalMapping / LoopClosing threads with their thread-local arenas)
    hipStream_t st = c.run.stream;
    static const bool hostDbg = std::getenv("RUMI_HOSTDBG") != nullptr;
    const double tA = ba_now_us();
    BaLayout L;
    double tm[3] = {tA, tA, tA};   // tB, tC, tD of the line below
    if ((rc = ba_host_structure(a, st, nKF, kf_pose7, kf_fixed, nMP, mp_pos3, nE, e_mp, e_kf, e_obs, e_inv_sigma2, L, tm)) != RUMI_OK) return rc;
    BADev B = ba_device_view(a, L, mode, gbaRobust, nKF, nMP, nE, K4);
    const int nOpt = L.nOpt, n = L.n;
    // The reduced pose system of a trial.  Up to 175 unknowns (29 optimised key-frames; here only on a profiled handle or with more than 512 key-frames):
    // dense Schur panel on the matrix cores + k_ba_solve_tiles.  180..252 unknowns (30..42): the same panel + k_ba_solve (one workgroup, matrix in L2).
    // More than 255 (43 and more): block-sparse Schur accumulation + multi-workgroup blocked Cholesky (ba_solve_big).
    BaPlan P;
    P.gE = std::max(1, (nE + 255) / 256);
    P.big = n > 255;
    P.NP = P.big ? 16 : (n + 1 + 15) / 16 * 16; P.NT = P.NP / 16; P.K3 = 3 * nMP;
    if (!P.big && P.NP > a.solo.npCap) { g_lastError = "local BA: reduced system larger than the optimiser's arenas"; return RUMI_E_CAPACITY; }
    if (P.big && (rc = ba_big_prepare(a, st, L, nMP, nE, e_kf, &P.nBlocks)) != RUMI_OK) return rc;
    P.ldsTiles = ((size_t)(P.NT * (P.NT + 1) / 2) * 256 + (size_t)P.NT * 16) * sizeof(double);
    P.useTiles = !P.big && n > 0 && P.NT <= kSolveTilesMax;
    if (P.useTiles && P.ldsTiles > 48 * 1024) HIP_TRY(raise_lds_limit(reinterpret_cast<const void *>(k_ba_solve_tiles), P.ldsTiles));
    if (nMP > 0 && !P.big) HIP_TRY(hipMemsetAsync(a.solo.Yt.p, 0, (size_t)P.K3 * P.NP * sizeof(double), st));   // pattern of Y is fixed: zero once, live entries are rewritten per trial
    HIP_TRY(hipEventRecord(c.run.ev[0], st));
    if (prof) for (auto &k : prof->kernelMs) k = 0.f;
    BaProfile *pf = prof && prof->on ? prof : nullptr;
    BaLmState S;
    const double tE = ba_now_us();
    if ((rc = ba_lm(a, pf, st, B, P, S, mode == 0 ? 10 : mode == 1 ? 5 : gbaIterations, stop_flag)) != RUMI_OK) return rc;
    const double tF = ba_now_us();
    const int itersFirst = S.iters;
    if (mode == 1 && !(stop_flag && *stop_flag)) {          // bDoMore
        if (nE > 0 && S.ranChi2) hipLaunchKernelGGL(k_ba_mark, dim3(P.gE), dim3(256), 0, st, B, a.T[S.cur].p, a.X[S.cur].p, a.eOff.p);
        B.robust = 0;
        if ((rc = ba_lm(a, pf, st, B, P, S, 10, stop_flag)) != RUMI_OK) return rc;
    }
    // results gathered by the last kernel into one block and read back with one copy: [T | X | erase]
    const size_t rT = 0, rX = al16(rT + (size_t)nKF * 64), rE = al16(rX + (size_t)nMP * 24), dnBytes = al16(rE + (size_t)nE);
    const int gF = std::max(P.gE, std::max((nKF * 8 + 255) / 256, (nMP * 3 + 255) / 256));
    hipLaunchKernelGGL(k_ba_finalize, dim3(gF), dim3(256), 0, st, B, a.T[S.cur].p, a.X[S.cur].p, S.ranChi2 ? 1 : 0, a.stageOut.p + rE, reinterpret_cast<double *>(a.stageOut.p + rT),
                       reinterpret_cast<double *>(a.stageOut.p + rX));
    HIP_TRY(hipEventRecord(c.run.ev[1], st));
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(a.stage.h, a.stageOut.p, dnBytes, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    HIP_TRY(hipEventElapsedTime(&c.run.stageMs[5], c.run.ev[0], c.run.ev[1]));
    ba_unpack(nKF, kf_fixed, nMP, nE, reinterpret_cast<const double *>(a.stage.h + rT), reinterpret_cast<const double *>(a.stage.h + rX), a.stage.h + rE,
              kf_pose7, mp_pos3, erase_out);
    ba_write_stats(mode, S.iters, itersFirst, S.trials, nOpt, stats);
    if (hostDbg) fprintf(stderr, "ba host us: pass1+partA %.1f h2d-A %.1f pass2+h2d-B %.1f setup %.1f lm %.1f tail %.1f\n", tm[0] - tA, tm[1] - tm[0], tm[2] - tm[1], tE - tm[2], tF - tE, ba_now_us() - tF);
    return RUMI_OK;
}

extern "C" int rumi_local_ba(RumiOptimizer *o, int32_t nKF, float *kf_pose7, const uint8_t *kf_fixed, int32_t nMP, float *mp_pos3,
                             int32_t nE, const int32_t *e_mp, const int32_t *e_kf, const float *e_obs, const float *e_inv_sigma2,
                             const float *K4, const volatile uint8_t *stop_flag, uint8_t *erase_out, int32_t *stats) {
    return ba_run(o ? &o->ba : nullptr, o ? &o->prof : nullptr, 0, nKF, kf_pose7, kf_fixed, nMP, mp_pos3, nE, e_mp, e_kf, e_obs, e_inv_sigma2, K4, stop_flag, erase_out, stats);
}

// R independent local windows (the only multi-window form local BA has: a window does not shard, SURVEY section 8e).  The handle keeps what they
// need beyond its own window (include/rumi_opt.h: batch arenas, batch runners, worker contexts), made on first use.
extern "C" int rumi_local_ba_batch(RumiOptimizer *o, int32_t n_windows, RumiBaWindow *win, int32_t n_workers) {
    if (!o || n_windows < 0 || (n_windows > 0 && !win) || n_workers < 1) return RUMI_E_INVALID;
    if (n_windows == 0) return RUMI_OK;
    HIP_TRY(hipSetDevice(o->device));
    const BaArena &lim = o->ba.arena;
    const size_t K = (size_t)lim.maxKF, M = (size_t)lim.maxMP, E = (size_t)lim.maxE;
    // windows of up to 29 optimised key-frames: the window is a batch dimension of the kernels (ba_windows.inc), driven by THIS thread alone, in
    // groups of kBawMaxWindows; every window of a group has a batch arena
    std::vector<int> batched, others;
    for (int i = 0; i < n_windows; i++) {
        const RumiBaWindow &W = win[i];
        const bool ok = W.kf_pose7 && W.kf_fixed && W.K4 && W.mp_pos3 && W.e_mp && W.e_kf && W.e_obs && W.e_inv_sigma2 && W.erase_out &&
                        W.n_kf <= lim.maxKF && W.n_mp <= lim.maxMP && W.n_edges <= lim.maxE && baw_eligible(o->prof.on, W.n_kf, W.kf_fixed, W.n_mp, W.n_edges);
        (ok ? batched : others).push_back(i);
    }
    for (size_t g0 = 0; g0 < batched.size(); g0 += kBawMaxWindows) {
        const int cnt = (int)std::min<size_t>(kBawMaxWindows, batched.size() - g0);
        // launch groups (two from 8 windows on, three from 12: baw_groups): the handle's own runner drives the first, batch runners the others
        const int G = baw_groups(cnt, 4);
        BaRunner *runners[4] = {&o->ba.run, &o->batchRunners[0], &o->batchRunners[1], &o->batchRunners[2]};
        int rc = RUMI_OK;                                   // (init keeps what is there: nothing happens from the second batch of this size on)
        for (int j = 0; j < cnt && rc == RUMI_OK; j++) rc = o->batchArenas[j].init(K, M, E, false);
        for (int g = 1; g < G && rc == RUMI_OK; g++) rc = runners[g]->init(o->device, K, M, E);
        if (rc != RUMI_OK) return rc;
        std::vector<BawArgs> args((size_t)cnt);
        std::vector<int32_t> status((size_t)cnt, RUMI_OK);
        for (int j = 0; j < cnt; j++) {
            RumiBaWindow &W = win[batched[g0 + j]];
            args[j] = BawArgs{W.n_kf, W.kf_pose7, W.kf_fixed, W.n_mp, W.mp_pos3, W.n_edges, W.e_mp, W.e_kf, W.e_obs, W.e_inv_sigma2, W.K4, W.stop_flag, W.erase_out, W.stats};
        }
        rc = baw_run(0, cnt, args.data(), o->batchArenas, 0, 1, status.data(), runners, G);
        for (int j = 0; j < cnt; j++) win[batched[g0 + j]].status = status[j];
        if (rc != RUMI_OK && rc != RUMI_E_INVALID && rc != RUMI_E_CAPACITY) return rc;      // a HIP failure: nothing more to run
    }
    // everything else (larger windows, windows of more than 512 key-frames, structure-only windows, the profiled path): one single-window run each
    // in a worker context, n_workers host threads taking the windows from a shared counter: while one window's thread waits for the eight scalars
    // of an LM trial, the kernels of the others fill the device
    if (!others.empty()) {
        n_workers = std::min(std::min(n_workers, (int)others.size()), kBaMaxWorkers);
        for (int k = 0; k < n_workers; k++) { const int rc = o->workers[k].init(o->device, K, M, E); if (rc != RUMI_OK) return rc; }
        std::atomic<int> next{0};
        auto work = [&](BaContext *c) {
            for (int q = next.fetch_add(1); q < (int)others.size(); q = next.fetch_add(1)) {
                RumiBaWindow &W = win[others[q]];
                W.status = ba_run(c, nullptr, 0, W.n_kf, W.kf_pose7, W.kf_fixed, W.n_mp, W.mp_pos3, W.n_edges, W.e_mp, W.e_kf, W.e_obs, W.e_inv_sigma2, W.K4, W.stop_flag,
                                  W.erase_out, W.stats);
            }
        };
        std::vector<std::thread> th;
        for (int k = 1; k < n_workers; k++) th.emplace_back(work, &o->workers[k]);
        work(&o->workers[0]);
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
    return ba_run(o ? &o->ba : nullptr, o ? &o->prof : nullptr, 2, nKF, kf_pose7, kf_fixed, nMP, mp_pos3, nE, e_mp, e_kf, e_obs, e_inv_sigma2, K4, stop_flag, erase.data(), stats, n_iterations, robust);
}

extern "C" int rumi_merge_ba(RumiOptimizer *o, int32_t nKF, float *kf_pose7, const uint8_t *kf_fixed, int32_t nMP, float *mp_pos3,
                             int32_t nE, const int32_t *e_mp, const int32_t *e_kf, const float *e_obs, const float *e_inv_sigma2,
                             const float *K4, const volatile uint8_t *stop_flag, uint8_t *erase_out, int32_t *stats) {
    return ba_run(o ? &o->ba : nullptr, o ? &o->prof : nullptr, 1, nKF, kf_pose7, kf_fixed, nMP, mp_pos3, nE, e_mp, e_kf, e_obs, e_inv_sigma2, K4, stop_flag, erase_out, stats);
}
