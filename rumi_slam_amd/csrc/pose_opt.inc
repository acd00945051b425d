// pose_opt.inc -- PoseOptimization: the argument block, the -DRUMI_POSE_STAMP cycle stamps and k_pose_opt (host side: pose_opt_host.inc).
// Included by opt.hip inside namespace rumi.

struct PoseArgs {
    const int32_t *start;
    const float *Xw, *obs, *w, *K4;
    const float *Tin;     // initial poses [nbatch][7]
    float *Tout;          // optimised poses [nbatch][7] (left as Tin where the reference returns early)
    uint8_t *outlier;
    int32_t *nGood;
    uint8_t *active;      // scratch, one per correspondence
    double *lastChi2;     // scratch, one per correspondence
    int skipSmall;        // the global-memory instantiation leaves the frames the LDS instantiation solves
};

// (compiled with floating-point contraction, on rumi::fused's copy of the math: opt_math.h says why)
#pragma clang fp contract(fast)
// LDS = true (frames of up to kPoseLdsEdges correspondences): the edge data, the active flags and the last chi2 of every edge
// live in LDS for the whole solve, so none of the ~60 passes over the edges waits for global memory.
// (-DRUMI_POSE_STAMP, tools/build_stamp_lib.sh: every wave of frame 0 prints where its cycles went)
#ifdef RUMI_POSE_STAMP
#define POSE_STAMP_DECL long long stT = clock64(), stSerial = 0, stPass = 0, stRed = 0, stChi = 0, stOther = 0; int stN = 0, stTr = 0
#define POSE_STAMP(acc) do { const long long now_ = clock64(); acc += now_ - stT; stT = now_; } while (0)
#define POSE_COUNT(c) c++
#else
#define POSE_STAMP_DECL
#define POSE_STAMP(acc)
#define POSE_COUNT(c)
#endif
// (kPoseLdsEdges: rumi_internal.h, shared with the tracker)
template <bool LDS, int NT>
__global__ __launch_bounds__(NT) void k_pose_opt(PoseArgs A) {
    constexpr int NW = NT / 64;
    __shared__ double redBuf[2 * (NW + 1) * 32];                            // two reduction buffers used in turn: a reduction then needs no barrier before its first store
    int redFlip = 0;
    auto next_red = [&]() { redFlip ^= 1; return redBuf + redFlip * (NW + 1) * 32; };
    __shared__ float sXw[LDS ? 3 * kPoseLdsEdges : 1], sObs[LDS ? 2 * kPoseLdsEdges : 1], sW[LDS ? kPoseLdsEdges : 1];
    __shared__ double sChi[LDS ? kPoseLdsEdges : 1];
    __shared__ uint8_t sAct[LDS ? kPoseLdsEdges : 1];
    const int tid = threadIdx.x, b = blockIdx.x;
    const int s0 = A.start[b], n = A.start[b + 1] - s0;
    if (LDS && n > kPoseLdsEdges) return;                                  // such frames are solved by the global-memory instantiation
    if (!LDS && n <= kPoseLdsEdges && A.skipSmall) return;
    const float *Xw = LDS ? sXw : A.Xw + (size_t)s0 * 3, *obs = LDS ? sObs : A.obs + (size_t)s0 * 2, *wgt = LDS ? sW : A.w + s0;
    uint8_t *outlier = A.outlier + s0, *active = LDS ? sAct : A.active + s0;
    double *lastChi2 = LDS ? sChi : A.lastChi2 + s0;
    if (LDS) {
        for (int i = tid; i < 3 * n; i += NT) sXw[i] = A.Xw[(size_t)s0 * 3 + i];
        for (int i = tid; i < 2 * n; i += NT) sObs[i] = A.obs[(size_t)s0 * 2 + i];
        for (int i = tid; i < n; i += NT) sW[i] = A.w[s0 + i];
    }
    for (int i = tid; i < n; i += NT) { outlier[i] = 0; active[i] = 1; }
    if (LDS) __syncthreads();
    if (n < 3) {                                                            // Optimizer.cc:899-900: returns 0, pose untouched
        if (tid == 0) A.nGood[b] = 0;
        if (tid < 7) A.Tout[(size_t)b * 7 + tid] = A.Tin[(size_t)b * 7 + tid];
        return;
    }
    const fused::DCam cam{A.K4[0], A.K4[1], A.K4[2], A.K4[3]};
    const double delta = (double)(float)sqrt(5.991), dsqr = delta * delta;  // const float deltaMono = sqrt(5.991)
    const fused::DSE3 T0 = fused::se3_from_float7(A.Tin + (size_t)b * 7);
    fused::DSE3 T = T0;
    bool robust = true;
    int nBadRound = 0;
    POSE_STAMP_DECL;

    // (the estimate maps a point by its rotation MATRIX, built once per pass -- 9 multiply-adds an edge instead of the quaternion form's two
    // cross products; the quaternion is normalised by every update)
    double Rm[3][3];
    auto set_pose = [&](const fused::DSE3 &P) { fused::quat_to_matrix(P.r, Rm); };
    // a thread's first kRegEdges edges (all of them up to 512 correspondences) stay in registers as doubles for the whole solve: no LDS read and
    // no float -> double conversion in the ~60 passes; further edges are read from the LDS (or global) arrays
    constexpr int kRegEdges = 2;
    double eX[kRegEdges], eY[kRegEdges], eZ[kRegEdges], eU[kRegEdges], eV[kRegEdges], eW[kRegEdges];
#pragma unroll
    for (int k = 0; k < kRegEdges; k++) {
        const int i = min(tid + k * NT, n - 1);                              // (n >= 3 here)
        eX[k] = (double)Xw[3 * i]; eY[k] = (double)Xw[3 * i + 1]; eZ[k] = (double)Xw[3 * i + 2];
        eU[k] = (double)obs[2 * i]; eV[k] = (double)obs[2 * i + 1]; eW[k] = (double)wgt[i];
    }
    uint8_t rAct[kRegEdges];                                                // ... and so do their active flag and last chi2 (only the owning thread reads them)
    double rChi[kRegEdges];
#pragma unroll
    for (int k = 0; k < kRegEdges; k++) { rAct[k] = 1; rChi[k] = 0; }
    auto for_edges = [&](auto &&body) {
#pragma unroll
        for (int k = 0; k < kRegEdges; k++) { const int i = tid + k * NT; if (i < n) body(i, eX[k], eY[k], eZ[k], eU[k], eV[k], eW[k], rAct[k], rChi[k]); }
        for (int i = tid + kRegEdges * NT; i < n; i += NT)
            body(i, (double)Xw[3 * i], (double)Xw[3 * i + 1], (double)Xw[3 * i + 2], (double)obs[2 * i], (double)obs[2 * i + 1], (double)wgt[i], active[i], lastChi2[i]);
    };
    auto edge_chi2 = [&](double X, double Y, double Z, double ou, double ov, double w, const fused::DSE3 &P, double &e0, double &e1, fused::D3 &pc) -> double {
        pc = fused::D3{Rm[0][0] * X + Rm[0][1] * Y + Rm[0][2] * Z + P.t.x, Rm[1][0] * X + Rm[1][1] * Y + Rm[1][2] * Z + P.t.y,
                       Rm[2][0] * X + Rm[2][1] * Y + Rm[2][2] * Z + P.t.z};
        double u, v;
        fused::cam_project(cam, pc, u, v);
        e0 = ou - u; e1 = ov - v;
        return e0 * w * e0 + e1 * w * e1;
    };
    auto robust_chi2 = [&](const fused::DSE3 &P) -> double {                      // computeActiveErrors + activeRobustChi2
        double acc[1] = {0};
        set_pose(P);
        for_edges([&](int i, double X, double Y, double Z, double ou, double ov, double w, uint8_t &act, double &last) {
            if (!act) return;
            double e0, e1; fused::D3 pc;
            const double c = edge_chi2(X, Y, Z, ou, ov, w, P, e0, e1, pc);
            last = c;
            double r0 = c, r1 = 1;
            if (robust) fused::huber(c, delta, dsqr, r0, r1);
            acc[0] += r0;
        });
        block_sum<1, NW, false>(acc, next_red());
        return acc[0];
    };

    for (int it = 0; it < 4; it++) {
        T = T0;                                                            // estimate reset every round (:910-911)
        // (the edges active in this round: all in the first, then those the last re-classification kept -- no pass to count them)
        if ((it == 0 ? n : n - nBadRound) > 0) {
            // ---- g2o optimize(10): optimization_algorithm_levenberg.cpp:61-169 ----
            double lambda = -1, ni = 2;
            int nBad = 0;
            for (int itl = 0; itl < 10; itl++) {
                // computeActiveErrors + activeRobustChi2 and buildSystem evaluate every edge at the same estimate: one pass, the
                // robust chi2 rides along as the 28th reduced value (same per-edge values, same reduction tree as robust_chi2)
#ifdef RUMI_POSE_STAMP
                asm volatile("" : "+v"(lambda), "+v"(T.r.x), "+v"(T.t.x), "+v"(nBad));      // the trial's decisions are taken before the stamp
#endif
                POSE_STAMP(stSerial);
                double hb[28];                                             // 21 upper entries of H, 6 of b, robust chi2
#pragma unroll
                for (int k = 0; k < 28; k++) hb[k] = 0;
                set_pose(T);
                for_edges([&](int i, double X, double Y, double Z, double ou, double ov, double w, uint8_t &act, double &last) {
                    if (!act) return;
                    double e0, e1; fused::D3 pc;
                    const double c = edge_chi2(X, Y, Z, ou, ov, w, T, e0, e1, pc);
                    last = c;
                    double r0 = c, r1 = 1;
                    if (robust) fused::huber(c, delta, dsqr, r0, r1);
                    hb[27] += r0;
                    double J0[6], J1[6];
                    fused::jac_pose(cam, pc, J0, J1);
                    const double rw = r1 * w;
                    // H += rw J^T J, b -= r1 w J^T e with the weights multiplied into one factor first (two multiply-adds an entry); J0[4] and
                    // J1[3] are zero by construction (jac_pose): their products are left out, H[3][4] stays 0
                    double A0[6], A1[6];
#pragma unroll
                    for (int a = 0; a < 6; a++) { A0[a] = rw * J0[a]; A1[a] = rw * J1[a]; }
                    const double we0 = rw * e0, we1 = rw * e1;
                    int p = 0;
#pragma unroll
                    for (int a = 0; a < 6; a++) {
#pragma unroll
                        for (int c2 = a; c2 < 6; c2++, p++) {
                            const bool z0 = a == 4 || c2 == 4, z1 = a == 3 || c2 == 3;
                            if (z0 && z1) continue;
                            hb[p] += z0 ? A1[a] * J1[c2] : z1 ? A0[a] * J0[c2] : A0[a] * J0[c2] + A1[a] * J1[c2];
                        }
                    }
#pragma unroll
                    for (int a = 0; a < 6; a++) hb[21 + a] -= a == 4 ? J1[a] * we1 : a == 3 ? J0[a] * we0 : J0[a] * we0 + J1[a] * we1;
                });
                POSE_STAMP(stPass);
                block_sum_butterfly<28, NW, false>(hb, next_red());
                POSE_STAMP(stRed); POSE_COUNT(stN);
                double currentChi = hb[27];
                const double iniChi = currentChi;
                if (itl == 0) {                                            // computeLambdaInit: tau * max |H_jj|
                    double m = 0;
                    int p = 0;
                    for (int a = 0; a < 6; a++) { m = fmax(fabs(hb[p]), m); p += 6 - a; }
                    lambda = 1e-5 * m; ni = 2; nBad = 0;
                }
                double rho = 0;
                int qmax = 0;
                do {
                    const fused::DSE3 saved = T;                                  // push()
                    double x[6];
                    const bool ok2 = fused::chol_solve_packed<6>(hb, lambda, hb + 21, x);   // setLambda + solve + restoreDiagonal
                    if (ok2) T = fused::se3_mul(fused::se3_exp_series(x), T);                    // oplusImpl: exp(update) * estimate
                    POSE_STAMP(stSerial); POSE_COUNT(stTr);
                    double tempChi = robust_chi2(T);
                    POSE_STAMP(stChi);
                    if (!ok2) tempChi = DBL_MAX;
                    rho = currentChi - tempChi;
                    double scale = 0;
                    if (ok2) for (int j = 0; j < 6; j++) scale += x[j] * (lambda * x[j] + hb[21 + j]);
                    scale += 1e-3;
                    rho *= fused::m_rcp(scale);                             // (v_rcp_f64 + two Newton steps instead of the IEEE divide sequence)
                    if (rho > 0 && isfinite(tempChi)) {
                        const double tr = 2 * rho - 1;
                        double alpha = 1. - tr * tr * tr;          // pow(2 rho - 1, 3) (levenberg.cpp:124): the generic pow is ~150 instructions of this serial section
                        alpha = fmin(alpha, 2. / 3.);
                        lambda *= fmax(1. / 3., alpha);
                        ni = 2;
                        currentChi = tempChi;
                    } else {
                        lambda *= ni;
                        ni *= 2;
                        T = saved;                                         // pop()
                    }
                    qmax++;
                } while (rho < 0 && qmax < 10);
                if (qmax == 10 || rho == 0) break;                         // Terminate
                if ((iniChi - currentChi) * 1e3 < iniChi) nBad++; else nBad = 0;
                if (nBad >= 3) break;
            }
        }
        // re-classification (:916-939): former outliers get a fresh error, active edges keep the last computed one
        double bad[1] = {0};
        set_pose(T);
        for_edges([&](int i, double X, double Y, double Z, double ou, double ov, double w, uint8_t &act, double &last) {
            double e0, e1; fused::D3 pc;
            const float chi2 = (float)(!act ? edge_chi2(X, Y, Z, ou, ov, w, T, e0, e1, pc) : last);       // (an edge is inactive exactly when it is an outlier)
            if (chi2 > 5.991f) { outlier[i] = 1; act = 0; bad[0] += 1; }
            else { outlier[i] = 0; act = 1; }
        });
        block_sum<1, NW, false>(bad, next_red());
        nBadRound = (int)bad[0];
        if (it == 2) robust = false;                                       // setRobustKernel(0)
        if (n < 10) break;                                                 // optimizer.edges().size() < 10
    }
#ifdef RUMI_POSE_STAMP
    POSE_STAMP(stOther);
    if (b == 0 && (tid & 63) == 0) printf("pose stamp wave %d n %d builds %d trials %d: serial %lld  build passes %lld  butterfly %lld  chi2 passes+reduce %lld  other %lld\n", tid >> 6, n, stN, stTr, stSerial, stPass, stRed, stChi, stOther);
#endif
    if (tid == 0) {
        fused::se3_to_float7(T, A.Tout + (size_t)b * 7);
        A.nGood[b] = n - nBadRound;
    }
}

#pragma clang fp contract(off)
