// Host side of rumi_essential_graph / rumi_sim3_correct_points (kernels: essential.inc).  Included by opt.hip after RumiOptimizer.

static bool eg_sim3_ok(const double *S) {
    for (int k = 0; k < 8; k++) if (!std::isfinite(S[k])) return false;
    const double nq = std::sqrt(S[0] * S[0] + S[1] * S[1] + S[2] * S[2] + S[3] * S[3]);
    return std::fabs(nq - 1.0) <= 1e-3 && S[7] > 0;
}

extern "C" int rumi_essential_graph(RumiOptimizer *o, int32_t n_v, double *S_io8, const uint8_t *fixed, const uint8_t *fix_scale, int32_t n_e,
                                    const int32_t *e_v0, const int32_t *e_v1, const double *meas8, int32_t n_iterations,
                                    const volatile uint8_t *stop_flag, int32_t *stats, double *chi2_trace) {
    // ---- validation: nothing below this block sees an unchecked index or a non-finite number ----
    if (!o || !S_io8 || !fixed || !fix_scale || !stats || !chi2_trace || n_v < 1 || n_e < 0 || n_iterations < 0) { g_lastError = "rumi_essential_graph: null argument or negative size"; return RUMI_E_INVALID; }
    if (n_e > 0 && (!e_v0 || !e_v1 || !meas8)) { g_lastError = "rumi_essential_graph: edges without arrays"; return RUMI_E_INVALID; }
    if (n_v > o->ba.arena.maxKF || n_e > o->ba.arena.maxE) { g_lastError = "rumi_essential_graph: graph larger than the optimiser's arenas"; return RUMI_E_CAPACITY; }
    for (int v = 0; v < n_v; v++) if (!eg_sim3_ok(S_io8 + (size_t)v * 8)) { g_lastError = "rumi_essential_graph: vertex estimate not finite, not a unit quaternion or scale <= 0"; return RUMI_E_INVALID; }
    for (int e = 0; e < n_e; e++) {
        if (e_v0[e] < 0 || e_v0[e] >= n_v || e_v1[e] < 0 || e_v1[e] >= n_v) { g_lastError = "rumi_essential_graph: edge vertex index out of range"; return RUMI_E_INVALID; }
        if (e_v0[e] == e_v1[e]) { g_lastError = "rumi_essential_graph: edge joins a vertex to itself"; return RUMI_E_INVALID; }
        if (!eg_sim3_ok(meas8 + (size_t)e * 8)) { g_lastError = "rumi_essential_graph: measurement not finite, not a unit quaternion or scale <= 0"; return RUMI_E_INVALID; }
    }
    // ---- active sets (SparseOptimizer::initializeOptimization): an edge between two fixed vertices is not active; a vertex owns rows when it
    //      is free and has an edge; incidence lists of the rows by a counting sort, ascending edge index within a row ----
    std::vector<int32_t> act0, act1, col((size_t)n_v, -1), deg((size_t)n_v, 0);
    std::vector<double> actM;
    act0.reserve(n_e); act1.reserve(n_e); actM.reserve((size_t)n_e * 8);
    for (int e = 0; e < n_e; e++) {
        const int a = e_v0[e], b = e_v1[e];
        if (fixed[a] && fixed[b]) continue;
        act0.push_back(a); act1.push_back(b);
        actM.insert(actM.end(), meas8 + (size_t)e * 8, meas8 + (size_t)e * 8 + 8);
        if (!fixed[a]) deg[a]++;
        if (!fixed[b]) deg[b]++;
    }
    const int nE = (int)act0.size();
    int nR = 0;
    for (int v = 0; v < n_v; v++) if (!fixed[v] && deg[v] > 0) col[v] = nR++;
    const double kNaN = std::numeric_limits<double>::quiet_NaN();
    if (nE == 0) {                                         // g2o: "Attempt to initialize an empty graph", optimize() touches nothing
        for (int i = 0; i < 4; i++) stats[i] = 0;
        for (int i = 0; i <= n_iterations; i++) chi2_trace[i] = kNaN;
        return RUMI_OK;
    }
    const int n = 7 * nR;
    std::vector<int32_t> rowStart((size_t)nR + 1, 0), inc;
    for (int v = 0; v < n_v; v++) if (col[v] >= 0) rowStart[col[v] + 1] = deg[v];
    for (int r = 0; r < nR; r++) rowStart[r + 1] += rowStart[r];
    inc.resize((size_t)rowStart[nR]);
    {
        std::vector<int32_t> cur(rowStart.begin(), rowStart.end() - 1);
        for (int e = 0; e < nE; e++) {
            if (col[act0[e]] >= 0) inc[cur[col[act0[e]]]++] = 2 * e;
            if (col[act1[e]] >= 0) inc[cur[col[act1[e]]]++] = 2 * e + 1;
        }
    }
    HIP_TRY(hipSetDevice(o->device));
    BaRunner &run = o->ba.run;                       // the handle's own stream, events and stage times
    BaArena::HostLoop &sc = o->ba.arena.solo;        // ... and published scalars
    hipStream_t st = run.stream;
    // ---- device arenas: the dense matrix [(n + 1) x n | n reciprocal pivots] and one block for everything else, grown on demand ----
    const size_t aBytes = ((size_t)(n + 1) * n + n) * sizeof(double);
    { const int rcg = o->egA.reserve(aBytes, aBytes); if (rcg != RUMI_OK) return rcg; }
    auto al = [](size_t x) { return (x + 63) & ~(size_t)63; };
    const size_t oS = 0, oM = al(oS + (size_t)n_v * 8 * 8), oV0 = al(oM + (size_t)nE * 8 * 8), oV1 = al(oV0 + (size_t)nE * 4), oCol = al(oV1 + (size_t)nE * 4),
                 oRow = al(oCol + (size_t)n_v * 4), oInc = al(oRow + (size_t)(nR + 1) * 4), oFix = al(oInc + inc.size() * 4), oFs = al(oFix + (size_t)n_v),
                 upBytes = al(oFs + (size_t)n_v);
    const size_t oS1 = upBytes, oEB = al(oS1 + (size_t)n_v * 8 * 8), oChi = al(oEB + (size_t)nE * kEgStride * 8), oB = al(oChi + (size_t)nE * 8),
                 oX = al(oB + (size_t)n * 8), oPart = al(oX + (size_t)n * 8), total = al(oPart + (size_t)nR * 8);
    { const int rcg = o->eg.reserve(total, total); if (rcg != RUMI_OK) return rcg; }
    std::vector<uint8_t> up(upBytes, 0);
    std::memcpy(up.data() + oS, S_io8, (size_t)n_v * 64);
    std::memcpy(up.data() + oM, actM.data(), (size_t)nE * 64);
    std::memcpy(up.data() + oV0, act0.data(), (size_t)nE * 4);
    std::memcpy(up.data() + oV1, act1.data(), (size_t)nE * 4);
    std::memcpy(up.data() + oCol, col.data(), (size_t)n_v * 4);
    std::memcpy(up.data() + oRow, rowStart.data(), (size_t)(nR + 1) * 4);
    std::memcpy(up.data() + oInc, inc.data(), inc.size() * 4);
    for (int v = 0; v < n_v; v++) { up[oFix + v] = fixed[v] != 0; up[oFs + v] = fix_scale[v] != 0; }
    HIP_TRY(hipMemcpyAsync(o->eg.p, up.data(), upBytes, hipMemcpyHostToDevice, st));
    HIP_TRY(hipStreamSynchronize(st));
    uint8_t *d = o->eg.p;
    double *A = (double *)o->egA.p, *rdg = A + (size_t)(n + 1) * n, *dS[2] = {(double *)(d + oS), (double *)(d + oS1)};
    const EGDev G{n_v, nE, nR, n, (const int32_t *)(d + oV0), (const int32_t *)(d + oV1), (const double *)(d + oM), d + oFix, d + oFs,
                  (const int32_t *)(d + oCol), (const int32_t *)(d + oRow), (const int32_t *)(d + oInc), (double *)(d + oEB), (double *)(d + oChi), A,
                  (double *)(d + oB), (double *)(d + oX), (double *)(d + oPart), sc.scal.p};
    const unsigned gE = (unsigned)((nE + 255) / 256), gV = (unsigned)((n_v + 255) / 256);
    auto chi2_of = [&](const double *S, int withScale, double *chi, double *scale) -> int {
        hipLaunchKernelGGL(k_eg_chi2, dim3(gE), dim3(256), 0, st, G, S);
        hipLaunchKernelGGL(k_eg_reduce, dim3(1), dim3(256), 0, st, G, withScale);
        const int rcf = fetch_published_scalars(sc, st);
        if (rcf != RUMI_OK) return rcf;
        *chi = sc.pub.h[0];
        if (scale) *scale = sc.pub.h[1];
        return RUMI_OK;
    };
    for (int i = 0; i <= n_iterations; i++) chi2_trace[i] = kNaN;
    const auto t0 = std::chrono::steady_clock::now();
    // ---- g2o's Levenberg-Marquardt (G/core/optimization_algorithm_levenberg.cpp:61-169) with setUserLambdaInit(1e-16) ----
    int cur = 0, iters = 0, trials = 0, how = 0, nBad = 0, rc = RUMI_OK;
    double lambda = 1e-16, ni = 2, currentChi = 0;
    auto stopped = [&]() { return stop_flag && *stop_flag; };
    if ((rc = chi2_of(dS[cur], 0, &currentChi, nullptr)) != RUMI_OK) return rc;
    chi2_trace[0] = currentChi;
    int it = 0;
    for (; it < n_iterations && !stopped(); it++) {
        const double iniChi = currentChi;
        hipLaunchKernelGGL(k_eg_linearise, dim3((unsigned)((nE + kEgEdgesPerBlock - 1) / kEgEdgesPerBlock)), dim3(256), 0, st, G, dS[cur]);
        double rho = 0;
        int qmax = 0;
        do {
            const int trial = cur ^ 1;
            HIP_TRY(hipMemsetAsync(A, 0, (size_t)(n + 1) * n * sizeof(double), st));
            hipLaunchKernelGGL(k_eg_assemble, dim3((unsigned)((nR + 3) / 4)), dim3(256), 0, st, G, lambda);
            HIP_TRY(hipEventRecord(run.ev[0], st));
            for (int j0 = 0; j0 < n; j0 += kNB) {
                const int w = std::min(kNB, n - j0), rows = n + 1 - (j0 + w);
                hipLaunchKernelGGL(k_chol_diag, dim3(1), dim3(256), 0, st, A, n, n, j0, rdg, sc.scal.p);
                if (rows > 0) {
                    const int T = (rows + 63) / 64;
                    hipLaunchKernelGGL(k_chol_trsm, dim3(T), dim3(256), 0, st, A, n, n, j0, rdg);
                    if (j0 + w < n) hipLaunchKernelGGL(k_chol_syrk, dim3(T, T), dim3(256), 0, st, A, n, n, j0);
                }
            }
            hipLaunchKernelGGL(k_eg_backsub, dim3(1), dim3(1024), 0, st, A, n, n, rdg, G.x, sc.scal.p);
            HIP_TRY(hipEventRecord(run.ev[1], st));
            hipLaunchKernelGGL(k_eg_update, dim3(gV), dim3(256), 0, st, G, lambda, dS[cur], dS[trial]);
            HIP_TRY(hipGetLastError());
            double tempChi = 0, scale = 0;
            if ((rc = chi2_of(dS[trial], 1, &tempChi, &scale)) != RUMI_OK) return rc;
            if (sc.pub.h[3] == 0.0) tempChi = std::numeric_limits<double>::max();     // the factorisation failed: g2o's solve() returned false
            rho = (currentChi - tempChi) / (scale + 1e-3);
            if (rho > 0 && std::isfinite(tempChi)) {
                double alpha = 1. - std::pow((2 * rho - 1), 3);
                alpha = std::min(alpha, 2. / 3.);
                lambda *= std::max(1. / 3., alpha);
                ni = 2;
                currentChi = tempChi;
                cur = trial;
            } else {
                lambda *= ni;
                ni *= 2;
            }
            qmax++;
            trials++;
        } while (rho < 0 && qmax < 10 && !stopped());
        iters++;
        chi2_trace[iters] = currentChi;
        if (qmax == 10 || rho == 0) { how = 1; break; }
        if ((iniChi - currentChi) * 1e3 < iniChi) nBad++; else nBad = 0;
        if (nBad >= 3) { how = 2; break; }
    }
    if (how == 0 && (it < n_iterations || stopped())) how = 3;
    std::vector<double> out((size_t)n_v * 8);
    HIP_TRY(hipMemcpyAsync(out.data(), dS[cur], (size_t)n_v * 64, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    for (int v = 0; v < n_v; v++) if (col[v] >= 0) std::memcpy(S_io8 + (size_t)v * 8, out.data() + (size_t)v * 8, 64);
    stats[0] = iters; stats[1] = trials; stats[2] = nR; stats[3] = how;
    for (auto &m : run.stageMs) m = 0.f;
    if (trials > 0) HIP_TRY(hipEventElapsedTime(&run.stageMs[3], run.ev[0], run.ev[1]));      // factorisation + back-substitution of the last trial
    run.stageMs[5] = (float)std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return RUMI_OK;
}

extern "C" int rumi_sim3_correct_points(RumiOptimizer *o, int32_t mode, int32_t n, float *X, const int32_t *ref, int32_t n_v, const void *tab_a,
                                        const void *tab_b) {
    if (!o || (mode != 0 && mode != 1) || n < 0 || n_v < 1 || !tab_a || !tab_b || (n > 0 && (!X || !ref))) { g_lastError = "rumi_sim3_correct_points: null argument, negative size or unknown mode"; return RUMI_E_INVALID; }
    if (n_v > o->ba.arena.maxKF || n > o->ba.arena.maxMP) { g_lastError = "rumi_sim3_correct_points: more vertices or points than the optimiser's arenas"; return RUMI_E_CAPACITY; }
    for (int i = 0; i < n; i++) {
        if (ref[i] < -1 || ref[i] >= n_v) { g_lastError = "rumi_sim3_correct_points: reference vertex index out of range"; return RUMI_E_INVALID; }
        if (!std::isfinite(X[3 * i]) || !std::isfinite(X[3 * i + 1]) || !std::isfinite(X[3 * i + 2])) { g_lastError = "rumi_sim3_correct_points: point not finite"; return RUMI_E_INVALID; }
    }
    for (int v = 0; v < n_v; v++) {
        bool ok = true;
        if (mode == 0) ok = eg_sim3_ok((const double *)tab_a + (size_t)v * 8) && eg_sim3_ok((const double *)tab_b + (size_t)v * 8);
        else for (const float *T : {(const float *)tab_a + (size_t)v * 7, (const float *)tab_b + (size_t)v * 7}) {
            for (int k = 0; k < 7; k++) ok = ok && std::isfinite(T[k]);
            ok = ok && std::fabs(std::sqrt((double)T[0] * T[0] + (double)T[1] * T[1] + (double)T[2] * T[2] + (double)T[3] * T[3]) - 1.0) <= 1e-3;
        }
        if (!ok) { g_lastError = "rumi_sim3_correct_points: transform not finite or not a unit quaternion"; return RUMI_E_INVALID; }
    }
    if (n == 0) return RUMI_OK;
    HIP_TRY(hipSetDevice(o->device));
    hipStream_t st = o->ba.run.stream;
    auto al = [](size_t x) { return (x + 63) & ~(size_t)63; };
    const size_t tb = (size_t)n_v * (mode == 0 ? 64 : 28), oX = 0, oR = al(oX + (size_t)n * 12), oA = al(oR + (size_t)n * 4), oB = al(oA + tb), total = al(oB + tb);
    { const int rcg = o->eg.reserve(total, total); if (rcg != RUMI_OK) return rcg; }
    std::vector<uint8_t> up(total, 0);
    std::memcpy(up.data() + oX, X, (size_t)n * 12); std::memcpy(up.data() + oR, ref, (size_t)n * 4);
    std::memcpy(up.data() + oA, tab_a, tb); std::memcpy(up.data() + oB, tab_b, tb);
    HIP_TRY(hipMemcpyAsync(o->eg.p, up.data(), total, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_sim3_correct_points, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, mode, n, (float *)(o->eg.p + oX), (const int32_t *)(o->eg.p + oR),
                       (const void *)(o->eg.p + oA), (const void *)(o->eg.p + oB));
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(up.data(), o->eg.p + oX, (size_t)n * 12, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    std::memcpy(X, up.data(), (size_t)n * 12);
    return RUMI_OK;
}
