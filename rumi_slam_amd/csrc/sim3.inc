// sim3.inc -- the three Sim3 kernels with their argument blocks: ComputeInliersNum, the RANSAC hypotheses, OptimizeSim3 (host side: sim3_host.inc).
// Included by opt.hip inside namespace rumi.  sim3_batch.inc runs the same per-hypothesis and per-problem device functions over several candidates.

// Sim3Solver::ComputeInliersNum (R/lib_src/Sim3Solver.cc:564-664): one lane per matched key-point pair.
// g2o::Sim3::map = s * (r * xyz) + t in double (G/types/sim3.h:144-146), Pinhole::project(Vector3d) in double then .cast<float>()
// (Pinhole.cpp:35-41), squared reprojection errors in float, tests against 2 * 9.210 * mvLevelSigma2 in double.
// squared reprojection error (float, as upstream) of point X under the Sim3 S (8 doubles) in the camera K
__device__ __forceinline__ float reproj2(const double *S, const float *K, const float *X, const float *kp) {
    const DQuat q{S[0], S[1], S[2], S[3]};
    const D3 r = quat_rotate(q, D3{(double)X[0], (double)X[1], (double)X[2]});
    const double s = S[7];
    const double px = s * r.x + S[4], py = s * r.y + S[5], pz = s * r.z + S[6];
    const float u = (float)((double)K[0] * px / pz + (double)K[2]), v = (float)((double)K[1] * py / pz + (double)K[3]);
    const float dx = kp[0] - u, dy = kp[1] - v;
    return dx * dx + dy * dy;
}
// ComputeInliersNum's test of one matched key-point pair (:621-630) under the composites gSc1w2 / gSc2w1 of its key-frame pair
__device__ __forceinline__ bool sim3_score_inlier(const double *Sc1w2, const double *Sc2w1, const float *K1, const float *K2, const float *X1, const float *X2,
                                                  const float *kp1, const float *kp2, float sg1, float sg2, bool e1, bool e2) {
    const float err1 = reproj2(Sc1w2, K1, X2, kp1);   // map-2 point into key-frame 1
    const float err2 = reproj2(Sc2w1, K2, X1, kp2);   // map-1 point into key-frame 2
    const bool ok1 = (double)err1 < 2 * 9.210 * (double)sg1 || e2;
    const bool ok2 = (double)err2 < 2 * 9.210 * (double)sg2 || e1;
    return ok1 && ok2;
}
__global__ void k_sim3_inliers(int total, const int32_t *pairOf, const double *Sc1w2, const double *Sc2w1, const float *K1, const float *K2,
                               const float *X1, const float *X2, const float *kp1, const float *kp2, const float *sigma1, const float *sigma2,
                               const uint8_t *edge1, const uint8_t *edge2, uint8_t *inlier) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int pr = pairOf[i];
    inlier[i] = sim3_score_inlier(Sc1w2 + (size_t)pr * 8, Sc2w1 + (size_t)pr * 8, K1, K2, X1 + (size_t)i * 3, X2 + (size_t)i * 3, kp1 + (size_t)i * 2,
                                  kp2 + (size_t)i * 2, sigma1[i], sigma2[i], edge1[i] != 0, edge2[i] != 0);
}


// ==================================================================================================================
// Sim3Solver::iterate (R/lib_src/Sim3Solver.cc:159-404): the hypotheses of one block of RANSAC iterations, one workgroup each.
// Lane 0 forms the hypothesis from its three correspondences (ComputeSim3 :437-540: Horn's closed form; float arithmetic as upstream
// up to the 4x4 matrix N, whose dominant eigenvector comes from a cyclic Jacobi iteration in double — upstream calls Eigen's general
// EigenSolver<Matrix4f>, which is not in the tree: "parity unpinned", DESIGN.md §7), then the workgroup runs CheckInliers (:542-562)
// over all correspondences and, for the rumination overload (:292-404), ComputeInliersNum (:564-664) under
// gSw1w2 = gSc1w^-1 * gSc1c2 * gSc2w (:344-347) over every matched key-point pair of every key-frame pair.
// ==================================================================================================================
struct RansacArgs {
    int n, nHyp, fixScale;
    const float *X1, *X2, *thr1, *thr2, *K1, *K2;
    const int32_t *tri;
    float *T12; int32_t *nIn; uint8_t *inl;
    int nPairs, total;                                            // score set (total == 0: none)
    const int32_t *pairOf; const double *Sc1w1, *Sc2w2, *Skf;
    const float *sK1, *sK2, *sX1, *sX2, *kp1, *kp2, *sg1, *sg2; const uint8_t *e1, *e2;
    int32_t *pairCnt; double *comp;
};

// dominant eigenvector (largest eigenvalue) of a symmetric 4x4 matrix: cyclic Jacobi rotations
__device__ inline void sym4_dominant_eigenvector(double a[4][4], double q[4]) {
    double v[4][4] = {{1, 0, 0, 0}, {0, 1, 0, 0}, {0, 0, 1, 0}, {0, 0, 0, 1}};
    for (int sweep = 0; sweep < 30; sweep++) {
        double off = 0;
        for (int i = 0; i < 4; i++) for (int j = i + 1; j < 4; j++) off += a[i][j] * a[i][j];
        if (off < 1e-300) break;
        for (int p = 0; p < 3; p++)
            for (int r = p + 1; r < 4; r++) {
                if (a[p][r] == 0) continue;
                const double theta = (a[r][r] - a[p][p]) / (2 * a[p][r]);
                const double t = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1));
                const double c = 1 / sqrt(t * t + 1), sn = t * c;
                for (int k = 0; k < 4; k++) { const double x = a[k][p], y = a[k][r]; a[k][p] = c * x - sn * y; a[k][r] = sn * x + c * y; }
                for (int k = 0; k < 4; k++) { const double x = a[p][k], y = a[r][k]; a[p][k] = c * x - sn * y; a[r][k] = sn * x + c * y; }
                for (int k = 0; k < 4; k++) { const double x = v[k][p], y = v[k][r]; v[k][p] = c * x - sn * y; v[k][r] = sn * x + c * y; }
            }
    }
    int best = 0;
    for (int i = 1; i < 4; i++) if (a[i][i] > a[best][best]) best = i;
    for (int k = 0; k < 4; k++) q[k] = v[k][best];
}

// ComputeSim3 (:437-540) of one minimal set: the three correspondences tri[0..2] of X1 / X2.  Writes the rows of [sR | t] of T12 and T21 (what
// CheckInliers multiplies with), the 16-float record of rumi_sim3_ransac's T12_out, and hands R, t, s back for the rumination overload.
// One thread; k_sim3_ransac (lane 0 of a workgroup) and k_s3b_hyp (one lane per hypothesis) both call it, so both round alike.
__device__ __forceinline__ void sim3_minimal_solve(const float *X1, const float *X2, const int32_t *tri, int fixScale, float *sT12, float *sT21, float *Tout,
                                                   float (&R)[3][3], float (&t12)[3], float &s12) {
    float P1[3][3], P2[3][3];                                  // column i = correspondence i (:185-188)
    for (int i = 0; i < 3; i++) {
        const int idx = tri[i];
        for (int r = 0; r < 3; r++) { P1[r][i] = X1[idx * 3 + r]; P2[r][i] = X2[idx * 3 + r]; }
    }
    float O1[3], O2[3], Pr1[3][3], Pr2[3][3];                  // ComputeCentroid :430-435
    for (int r = 0; r < 3; r++) {
        O1[r] = ((P1[r][0] + P1[r][1]) + P1[r][2]) / 3.f;
        O2[r] = ((P2[r][0] + P2[r][1]) + P2[r][2]) / 3.f;
        for (int i = 0; i < 3; i++) { Pr1[r][i] = P1[r][i] - O1[r]; Pr2[r][i] = P2[r][i] - O2[r]; }
    }
    float M[3][3];                                             // Pr2 * Pr1^T :453
    for (int r = 0; r < 3; r++) for (int c = 0; c < 3; c++) M[r][c] = (Pr2[r][0] * Pr1[c][0] + Pr2[r][1] * Pr1[c][1]) + Pr2[r][2] * Pr1[c][2];
    const double N11 = M[0][0] + M[1][1] + M[2][2], N12 = M[1][2] - M[2][1], N13 = M[2][0] - M[0][2], N14 = M[0][1] - M[1][0],
                 N22 = M[0][0] - M[1][1] - M[2][2], N23 = M[0][1] + M[1][0], N24 = M[2][0] + M[0][2], N33 = -M[0][0] + M[1][1] - M[2][2],
                 N34 = M[1][2] + M[2][1], N44 = -M[0][0] - M[1][1] + M[2][2];
    // upstream stores N in a Matrix4f: the solver sees the float-rounded entries
    double Nm[4][4] = {{(float)N11, (float)N12, (float)N13, (float)N14}, {(float)N12, (float)N22, (float)N23, (float)N24},
                       {(float)N13, (float)N23, (float)N33, (float)N34}, {(float)N14, (float)N24, (float)N34, (float)N44}};
    double q[4];
    sym4_dominant_eigenvector(Nm, q);
    const float e0 = (float)q[0];
    float vec[3] = {(float)q[1], (float)q[2], (float)q[3]};
    const float nrm = sqrtf((vec[0] * vec[0] + vec[1] * vec[1]) + vec[2] * vec[2]);
    int valid = !(vec[0] == 0 && vec[1] == 0 && vec[2] == 0);   // :493-494 upstream keeps the previous iteration's transform
    for (int r = 0; r < 3; r++) { for (int c = 0; c < 3; c++) R[r][c] = r == c ? 1.f : 0.f; t12[r] = 0.f; }
    s12 = 1.f;
    if (valid) {
        const double ang = atan2((double)nrm, (double)e0);
        const float f = (float)(2 * ang);
        for (int k = 0; k < 3; k++) vec[k] = vec[k] * f / nrm;   // angle-axis; the quaternion angle is the half
        // Sophus::SO3f::exp(vec).matrix()
        const float th2 = (vec[0] * vec[0] + vec[1] * vec[1]) + vec[2] * vec[2], th = sqrtf(th2), half = 0.5f * th;
        float im, re;
        if (th < 1e-5f) { const float th4 = th2 * th2; im = 0.5f - (1.f / 48.f) * th2 + (1.f / 3840.f) * th4; re = 1.f - (1.f / 8.f) * th2 + (1.f / 384.f) * th4; }
        else { im = sinf(half) / th; re = cosf(half); }
        const float qx = im * vec[0], qy = im * vec[1], qz = im * vec[2], qw = re;
        const float tx = 2 * qx, ty = 2 * qy, tz = 2 * qz, twx = tx * qw, twy = ty * qw, twz = tz * qw, txx = tx * qx, txy = ty * qx, txz = tz * qx,
                    tyy = ty * qy, tyz = tz * qy, tzz = tz * qz;
        R[0][0] = 1 - (tyy + tzz); R[0][1] = txy - twz; R[0][2] = txz + twy;
        R[1][0] = txy + twz; R[1][1] = 1 - (txx + tzz); R[1][2] = tyz - twx;
        R[2][0] = txz - twy; R[2][1] = tyz + twx; R[2][2] = 1 - (txx + tyy);
        if (!fixScale) {                                      // :503-520
            double nom = 0, den = 0;
            float P3[3][3];
            for (int r = 0; r < 3; r++) for (int c = 0; c < 3; c++) P3[r][c] = (R[r][0] * Pr2[0][c] + R[r][1] * Pr2[1][c]) + R[r][2] * Pr2[2][c];
            float fn = 0, fd = 0;                               // Eigen's float array sums, column-major order
            for (int c = 0; c < 3; c++) for (int r = 0; r < 3; r++) { fn += Pr1[r][c] * P3[r][c]; fd += P3[r][c] * P3[r][c]; }
            nom = fn; den = fd;
            s12 = (float)(nom / den);
        }
        for (int r = 0; r < 3; r++) {                           // mt12i = O1 - ms12i * mR12i * O2
            const float ro = ((s12 * R[r][0]) * O2[0] + (s12 * R[r][1]) * O2[1]) + (s12 * R[r][2]) * O2[2];
            t12[r] = O1[r] - ro;
        }
    }
    const float sinv = (float)(1.0 / s12);
    for (int r = 0; r < 3; r++) {
        for (int c = 0; c < 3; c++) { sT12[r * 4 + c] = s12 * R[r][c]; sT21[r * 4 + c] = sinv * R[c][r]; }
        sT12[r * 4 + 3] = t12[r];
    }
    for (int r = 0; r < 3; r++) sT21[r * 4 + 3] = -((sT21[r * 4 + 0] * t12[0] + sT21[r * 4 + 1] * t12[1]) + sT21[r * 4 + 2] * t12[2]);
    for (int r = 0; r < 3; r++) for (int c = 0; c < 3; c++) Tout[r * 3 + c] = R[r][c];
    Tout[9] = t12[0]; Tout[10] = t12[1]; Tout[11] = t12[2]; Tout[12] = s12; Tout[13] = (float)valid; Tout[14] = 0; Tout[15] = 0;
}

// CheckInliers :542-562 of one correspondence (float, as upstream): a = point 1 in camera 1, b = point 2 in camera 2, K = {fx fy cx cy}
__device__ __forceinline__ bool sim3_check_inlier(const float *K1, const float *K2, const float *sT12, const float *sT21, const float *a, const float *b,
                                                  float thr1, float thr2) {
    const float fx1 = K1[0], fy1 = K1[1], cx1 = K1[2], cy1 = K1[3], fx2 = K2[0], fy2 = K2[1], cx2 = K2[2], cy2 = K2[3];
    const float u1 = fx1 * a[0] / a[2] + cx1, v1 = fy1 * a[1] / a[2] + cy1;            // mvP1im1
    const float u2 = fx2 * b[0] / b[2] + cx2, v2 = fy2 * b[1] / b[2] + cy2;            // mvP2im2
    float p[3], r[3];
    for (int k = 0; k < 3; k++) {
        p[k] = ((sT12[k * 4] * b[0] + sT12[k * 4 + 1] * b[1]) + sT12[k * 4 + 2] * b[2]) + sT12[k * 4 + 3];   // point 2 in camera 1
        r[k] = ((sT21[k * 4] * a[0] + sT21[k * 4 + 1] * a[1]) + sT21[k * 4 + 2] * a[2]) + sT21[k * 4 + 3];   // point 1 in camera 2
    }
    const float d1x = u1 - (fx1 * p[0] / p[2] + cx1), d1y = v1 - (fy1 * p[1] / p[2] + cy1);
    const float d2x = (fx2 * r[0] / r[2] + cx2) - u2, d2y = (fy2 * r[1] / r[2] + cy2) - v2;
    const float err1 = d1x * d1x + d1y * d1y, err2 = d2x * d2x + d2y * d2y;
    return err1 < thr1 && err2 < thr2;
}

// gSw1w2 = gSc1w^-1 * gSc1c2 * gSc2w (:338-347) of one hypothesis; Skf = g2o::Sim3(R, t, 1.0) of the solver's two key-frames, 2 x 8 doubles.
// k_sim3_ransac and k_sms_hyp (submap_sim3.inc) both call it, so both round alike.
__device__ __forceinline__ DSim3 sim3_hyp_world(const float (&R)[3][3], const float (&t12)[3], float s12, const double *Skf) {
    double Rd[3][3];
    for (int r = 0; r < 3; r++) for (int c = 0; c < 3; c++) Rd[r][c] = (double)R[r][c];
    const DSim3 Sc1c2{quat_from_matrix(Rd), {(double)t12[0], (double)t12[1], (double)t12[2]}, (double)s12};
    return sim3_mul(sim3_mul(sim3_inverse(sim3_from8(Skf)), Sc1c2), sim3_from8(Skf + 8));
}

__global__ __launch_bounds__(256) void k_sim3_ransac(RansacArgs A) {
    __shared__ float sT12[12], sT21[12];      // rows of [sR | t]
    __shared__ int sCnt;
    __shared__ DSim3 sSw1w2;
    const int h = blockIdx.x, tid = threadIdx.x;
    if (tid == 0) {
        sCnt = 0;
        float R[3][3], t12[3], s12;
        sim3_minimal_solve(A.X1, A.X2, A.tri + h * 3, A.fixScale, sT12, sT21, A.T12 + (size_t)h * 16, R, t12, s12);
        if (A.total > 0) sSw1w2 = sim3_hyp_world(R, t12, s12, A.Skf);
    }
    __syncthreads();
    int mine = 0;
    for (int i = tid; i < A.n; i += 256) {
        const bool in = sim3_check_inlier(A.K1, A.K2, sT12, sT21, A.X1 + (size_t)i * 3, A.X2 + (size_t)i * 3, A.thr1[i], A.thr2[i]);
        if (A.inl) A.inl[(size_t)h * A.n + i] = in;
        mine += in;
    }
    if (mine) atomicAdd(&sCnt, mine);
    __syncthreads();
    if (tid == 0) A.nIn[h] = sCnt;
    if (A.total <= 0) return;
    // ComputeInliersNum :564-664 under this hypothesis
    double *comp = A.comp + (size_t)h * A.nPairs * 16;
    int32_t *cnt = A.pairCnt + (size_t)h * A.nPairs;
    for (int p = tid; p < A.nPairs; p += 256) {
        sim3_to8(sim3_mul(sim3_from8(A.Sc1w1 + (size_t)p * 8), sSw1w2), comp + (size_t)p * 16);                       // gSc1w2 :621
        sim3_to8(sim3_mul(sim3_from8(A.Sc2w2 + (size_t)p * 8), sim3_inverse(sSw1w2)), comp + (size_t)p * 16 + 8);     // gSc2w1 :620
        cnt[p] = 0;
    }
    __threadfence_block();
    __syncthreads();
    for (int i = tid; i < A.total; i += 256) {
        const int pr = A.pairOf[i];
        if (sim3_score_inlier(comp + (size_t)pr * 16, comp + (size_t)pr * 16 + 8, A.sK1, A.sK2, A.sX1 + (size_t)i * 3, A.sX2 + (size_t)i * 3, A.kp1 + (size_t)i * 2,
                              A.kp2 + (size_t)i * 2, A.sg1[i], A.sg2[i], A.e1[i] != 0, A.e2[i] != 0))
            atomicAdd(&cnt[pr], 1);
    }
}


// ==================================================================================================================
// OptimizeSim3 / OptimizeCloudSim3 (R/lib_src/Optimizer.cc:1920-2167, :2169-2471): one Sim3 vertex, fixed points, two reprojection
// edges per correspondence, numeric Jacobians (G/core/base_binary_edge.hpp:131-203, delta 1e-9, through VertexSim3Expmap::oplusImpl).
// One 256-thread workgroup runs both optimize() calls.  The transform an edge applies depends only on its key-frame pair and on the
// perturbation (gSc1w * est' * gSc2w^-1 and gSc2w * est'^-1 * gSc1w^-1, OptimizableTypes.h:242,285): the 15 (base, +-delta per
// dimension) x 2 composites per pair are formed once per linearisation and every correspondence evaluates 30 map + project against them.
// ==================================================================================================================
struct Sim3Args {
    int n, nPairs, world, fixScale, robustFirst;
    float th2;
    const int32_t *pairOf;
    const double *Sc1w, *Sc2w, *Sin;
    const float *P1c, *P2c, *obs1, *obs2, *w1, *w2;
    const uint8_t *skip12, *skip21;
    const float *K1, *K2;
    double *Sout; int32_t *res; uint8_t *status;          // results
    double *comp, *chi12, *chi21; uint8_t *on12, *on21;   // scratch
};

// The whole optimisation of one problem by one 256-thread workgroup: k_sim3_opt hands it the kernel's own argument block, k_sim3_opt_batch
// (sim3_batch.inc) the entry of its problem table.  Same text, same order of every sum, same bytes.
__device__ __forceinline__ void sim3_opt_run(const Sim3Args &A) {
    __shared__ double red[5 * 64];
    const int tid = threadIdx.x, n = A.n, np = A.world ? A.nPairs : 1;
    const DCam cam1{A.K1[0], A.K1[1], A.K1[2], A.K1[3]}, cam2{A.K2[0], A.K2[1], A.K2[2], A.K2[3]};
    const double delta = (double)sqrtf(A.th2), dsqr = delta * delta, th2 = (double)A.th2;
    DSim3 est = sim3_from8(A.Sin);
    bool robust = A.robustFirst != 0;
    for (int i = tid; i < n; i += 256) { A.on12[i] = !(A.skip12 && A.skip12[i]); A.on21[i] = !(A.skip21 && A.skip21[i]); A.status[i] = 0; }

    auto oplus = [&](const DSim3 &S, const double *upd) -> DSim3 {          // VertexSim3Expmap::oplusImpl
        double u[7];
#pragma unroll
        for (int k = 0; k < 7; k++) u[k] = upd[k];
        if (A.fixScale) u[6] = 0;
        return sim3_mul(sim3_exp(u), S);
    };
    auto fill = [&](const DSim3 &S0, bool full) {                            // composites of every pair: slot 0 base, 1 + 2d / 2 + 2d = +-delta in dimension d
        const int cnt = full ? 15 : 1;
        for (int idx = tid; idx < np * cnt; idx += 256) {
            const int p = idx / cnt, k = idx - p * cnt;
            DSim3 S = S0;
            if (k) {
                double add[7] = {0, 0, 0, 0, 0, 0, 0};
                const int d = (k - 1) >> 1;
                const double v = (k & 1) ? 1e-9 : -1e-9;
#pragma unroll
                for (int q = 0; q < 7; q++) if (q == d) add[q] = v;
                S = oplus(S0, add);
            }
            DSim3 F = S, I = sim3_inverse(S);
            if (A.world) {
                const DSim3 a = sim3_from8(A.Sc1w + (size_t)p * 8), b = sim3_from8(A.Sc2w + (size_t)p * 8);
                F = sim3_mul(sim3_mul(a, S), sim3_inverse(b));
                I = sim3_mul(sim3_mul(b, sim3_inverse(S)), sim3_inverse(a));
            }
            sim3_to8(F, A.comp + ((size_t)p * 30 + k) * 8);
            sim3_to8(I, A.comp + ((size_t)p * 30 + 15 + k) * 8);
        }
        __threadfence_block();
        __syncthreads();
    };
    auto err12 = [&](int i, int p, int k, double &e0, double &e1) {
        const D3 pc = sim3_map(sim3_from8(A.comp + ((size_t)p * 30 + k) * 8), D3{(double)A.P2c[3 * i], (double)A.P2c[3 * i + 1], (double)A.P2c[3 * i + 2]});
        double u, v;
        cam_project(cam1, pc, u, v);
        e0 = (double)A.obs1[2 * i] - u; e1 = (double)A.obs1[2 * i + 1] - v;
    };
    auto err21 = [&](int i, int p, int k, double &e0, double &e1) {
        const D3 pc = sim3_map(sim3_from8(A.comp + ((size_t)p * 30 + 15 + k) * 8), D3{(double)A.P1c[3 * i], (double)A.P1c[3 * i + 1], (double)A.P1c[3 * i + 2]});
        double u, v;
        cam_project(cam2, pc, u, v);
        e0 = (double)A.obs2[2 * i] - u; e1 = (double)A.obs2[2 * i + 1] - v;
    };
    auto robust_chi2 = [&](const DSim3 &S) -> double {                       // computeActiveErrors + activeRobustChi2
        fill(S, false);
        double acc[1] = {0};
        for (int i = tid; i < n; i += 256) {
            const int p = A.pairOf ? A.pairOf[i] : 0;
            if (A.on12[i]) {
                double e0, e1; err12(i, p, 0, e0, e1);
                const double w = (double)A.w1[i], c = e0 * w * e0 + e1 * w * e1;
                A.chi12[i] = c;
                double r0 = c, r1 = 1;
                if (robust) huber(c, delta, dsqr, r0, r1);
                acc[0] += r0;
            }
            if (A.on21[i]) {
                double e0, e1; err21(i, p, 0, e0, e1);
                const double w = (double)A.w2[i], c = e0 * w * e0 + e1 * w * e1;
                A.chi21[i] = c;
                double r0 = c, r1 = 1;
                if (robust) huber(c, delta, dsqr, r0, r1);
                acc[0] += r0;
            }
        }
        block_sum<1>(acc, red);
        return acc[0];
    };
    auto lm = [&](int maxIt) {                                               // optimization_algorithm_levenberg.cpp:61-169
        double lambda = -1, ni = 2;
        int nBadIt = 0;
        for (int itl = 0; itl < maxIt; itl++) {
            double hb[36];                                                   // 28 upper entries of H, 7 of b, robust chi2
#pragma unroll
            for (int k = 0; k < 36; k++) hb[k] = 0;
            fill(est, true);
            for (int i = tid; i < n; i += 256) {
                const int p = A.pairOf ? A.pairOf[i] : 0;
#pragma unroll
                for (int side = 0; side < 2; side++) {
                    if (!(side ? A.on21[i] : A.on12[i])) continue;
                    double e0, e1, J0[7], J1[7];
                    if (side) err21(i, p, 0, e0, e1); else err12(i, p, 0, e0, e1);
#pragma unroll
                    for (int d = 0; d < 7; d++) {
                        double p0, p1, m0, m1;
                        if (side) { err21(i, p, 1 + 2 * d, p0, p1); err21(i, p, 2 + 2 * d, m0, m1); }
                        else { err12(i, p, 1 + 2 * d, p0, p1); err12(i, p, 2 + 2 * d, m0, m1); }
                        J0[d] = 5e8 * (p0 - m0); J1[d] = 5e8 * (p1 - m1);       // scalar = 1 / (2 delta)
                    }
                    const double w = (double)(side ? A.w2[i] : A.w1[i]), c = e0 * w * e0 + e1 * w * e1;
                    if (side) A.chi21[i] = c; else A.chi12[i] = c;
                    double r0 = c, r1 = 1;
                    if (robust) huber(c, delta, dsqr, r0, r1);
                    hb[35] += r0;
                    const double rw = r1 * w;
                    int q = 0;
#pragma unroll
                    for (int a = 0; a < 7; a++) {
#pragma unroll
                        for (int c2 = a; c2 < 7; c2++) hb[q++] += rw * (J0[a] * J0[c2] + J1[a] * J1[c2]);
                    }
#pragma unroll
                    for (int a = 0; a < 7; a++) hb[28 + a] -= r1 * (J0[a] * w * e0 + J1[a] * w * e1);
                }
            }
            block_sum_butterfly<36>(hb, red);
            double currentChi = hb[35];
            const double iniChi = currentChi;
            if (itl == 0) {
                double m = 0;
                int q = 0;
                for (int a = 0; a < 7; a++) { m = fmax(fabs(hb[q]), m); q += 7 - a; }
                lambda = 1e-5 * m; ni = 2; nBadIt = 0;
            }
            double rho = 0;
            int qmax = 0;
            do {
                const DSim3 saved = est;
                double x[7];
                const bool ok2 = chol_solve_packed<7>(hb, lambda, hb + 28, x);
                if (ok2) est = oplus(est, x);
                double tempChi = robust_chi2(est);
                if (!ok2) tempChi = DBL_MAX;
                rho = currentChi - tempChi;
                double scale = 0;
                if (ok2) for (int j = 0; j < 7; j++) scale += x[j] * (lambda * x[j] + hb[28 + j]);
                scale += 1e-3;
                rho /= scale;
                if (rho > 0 && isfinite(tempChi)) {
                    const double tr = 2 * rho - 1;
                    double alpha = 1. - tr * tr * tr;
                    alpha = fmin(alpha, 2. / 3.);
                    lambda *= fmax(1. / 3., alpha);
                    ni = 2;
                    currentChi = tempChi;
                } else {
                    lambda *= ni;
                    ni *= 2;
                    est = saved;
                }
                qmax++;
            } while (rho < 0 && qmax < 10);
            if (qmax == 10 || rho == 0) break;
            if ((iniChi - currentChi) * 1e3 < iniChi) nBadIt++; else nBadIt = 0;
            if (nBadIt >= 3) break;
        }
    };

    __syncthreads();
    if (n > 0) lm(5);                                                        // optimizer.optimize(5)
    if (tid == 0) sim3_to8(est, A.Sout);                                     // OptimizeCloudSim3 publishes this estimate already (:2397)
    double bad[1] = {0};
    for (int i = tid; i < n; i += 256) {                                     // :2110 / :2407: chi2() of the errors the last computeActiveErrors() left
        if ((A.on12[i] && A.chi12[i] > th2) || (A.on21[i] && A.chi21[i] > th2)) { A.status[i] = 1; A.on12[i] = 0; A.on21[i] = 0; bad[0] += 1; }
    }
    block_sum<1>(bad, red);
    const int nBad = (int)bad[0];
    robust = false;                                                          // setRobustKernel(0)
    if (n - nBad < 10) {
        if (tid == 0) { A.res[0] = 0; A.res[1] = nBad; A.res[2] = 1; }
        return;
    }
    lm(nBad > 0 ? 10 : 5);
    fill(est, false);
    double in[1] = {0};
    for (int i = tid; i < n; i += 256) {
        if (A.status[i] == 1) continue;
        if (!A.on12[i] || !A.on21[i]) { A.status[i] = 3; continue; }         // :2450-2451
        const int p = A.pairOf ? A.pairOf[i] : 0;
        double a0, a1, b0, b1;
        err12(i, p, 0, a0, a1); err21(i, p, 0, b0, b1);
        const double w1 = (double)A.w1[i], w2 = (double)A.w2[i];
        if (a0 * w1 * a0 + a1 * w1 * a1 > th2 || b0 * w2 * b0 + b1 * w2 * b1 > th2) A.status[i] = 2; else in[0] += 1;
    }
    block_sum<1>(in, red);
    if (tid == 0) { sim3_to8(est, A.Sout); A.res[0] = (int)in[0]; A.res[1] = nBad; A.res[2] = 0; }
}

__global__ __launch_bounds__(256) void k_sim3_opt(Sim3Args A) { sim3_opt_run(A); }
