// ba_single.inc -- kernels of the single-window bundle adjustment (LocalBundleAdjustment, merge window, global BA) that ba_run drives trial by trial
// from the host (ba_single_host.inc): the device view of a window (BADev), build / Schur / one-workgroup solve / update / chi2 / mark / finalize,
// and k_ba_publish.  Included by opt.hip inside namespace rumi; ba_solve_tiles.inc and ba_big.inc build on BADev.

struct BADev {
    int nKF, nMP, nE, nOpt, n;                 // n = 6 nOpt
    const int32_t *eMP, *eKF, *poseCol;        // poseCol[kf] = column block or -1 (fixed)
    const int32_t *ptStart, *ptEdge;           // edges grouped by landmark (CSR)
    const int32_t *rowSlot;                    // edge -> first of its two rows in the key-frame-ordered pose panel (-1 fixed)
    const int32_t *kfRowStart;                 // [nOpt + 1] row ranges of the panel
    const float *obs, *info;                   // the caller's single-precision measurements and weights as they came (widened where they are read)
    DCam cam;
    double delta, dsqr;
    double *Hll, *bl, *Hpl, *panel, *Hpp, *bp, *Dinv, *x, *lastChi2;
    double *scal;                              // [0] chi2, [1] scale, [2] max diag (as bits), [3] ok flag
    const uint8_t *off;                        // edge at level 1 (excluded from the optimisation), merge BA second pass
    int robust;                                // Huber kernel on the edges (off in the merge BA second pass)
};

__device__ __forceinline__ DSE3 load_pose(const double *T, int k) {
    const double *p = T + (size_t)k * 8;
    return DSE3{{p[0], p[1], p[2], p[3]}, {p[4], p[5], p[6]}};
}
__device__ __forceinline__ void store_pose(double *T, int k, const DSE3 &P) {
    double *p = T + (size_t)k * 8;
    p[0] = P.r.x; p[1] = P.r.y; p[2] = P.r.z; p[3] = P.r.w; p[4] = P.t.x; p[5] = P.t.y; p[6] = P.t.z; p[7] = 0;
}

__global__ __launch_bounds__(256) void k_ba_chi2(BADev B, const double *T, const double *X) {
    __shared__ double red[4];
    const int e = blockIdx.x * 256 + threadIdx.x;
    double acc[1] = {0};
    if (e < B.nE) {
        const int p = B.eMP[e];
        const D3 pc = se3_map(load_pose(T, B.eKF[e]), D3{X[3 * p], X[3 * p + 1], X[3 * p + 2]});
        double u, v;
        cam_project(B.cam, pc, u, v);
        const double e0 = (double)B.obs[2 * e] - u, e1 = (double)B.obs[2 * e + 1] - v, w = (double)B.info[e];
        const double c = e0 * w * e0 + e1 * w * e1;
        if (!B.off[e]) {                                                    // level-1 edges keep the error of their last active pass
            B.lastChi2[e] = c;
            double r0 = c, r1 = 1;
            if (B.robust) huber(c, B.delta, B.dsqr, r0, r1);
            acc[0] = r0;
        }
    }
    block_sum<1>(acc, red);
    if (threadIdx.x == 0) atomicAdd(&B.scal[0], acc[0]);
}

// Lanes walk the edges in landmark order (ptEdge): the contributions to H_ll and b_l of one landmark sit in consecutive lanes and are summed
// by a segmented wave reduction, so only the first lane of every run issues atomics (device-scope f64 atomics are served past the per-XCD
// L2s: 12 per edge cost 37 us per call at 44 k edges, a twelfth of that 12 us).
__device__ __forceinline__ void seg_reduce_atomic(double v, int p, bool head, double *dst) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const double vo = __shfl_down(v, d);
        const int po = __shfl_down(p, d);
        if (lane + d < 64 && po == p) v += vo;
    }
    if (head && p >= 0) atomicAdd(dst, v);
}

__global__ __launch_bounds__(256) void k_ba_build(BADev B, const double *T, const double *X) {
    const int t = blockIdx.x * 256 + threadIdx.x, lane = threadIdx.x & 63;
    const bool liveEdge = t < B.nE;
    const int e = liveEdge ? B.ptEdge[t] : 0;
    const int pKey = liveEdge ? B.eMP[e] : -1;
    const int pPrev = __shfl_up(pKey, 1);
    const bool head = lane == 0 || pPrev != pKey;            // first lane of a landmark's run inside this wave
    double hl[6] = {0, 0, 0, 0, 0, 0}, blv[3] = {0, 0, 0};  // this edge's A^T W A (upper triangle) and -A^T W e
    if (liveEdge) {
    const int p = pKey, kf = B.eKF[e];
    const DSE3 P = load_pose(T, kf);
    const D3 pc = se3_map(P, D3{X[3 * p], X[3 * p + 1], X[3 * p + 2]});
    double u, v;
    cam_project(B.cam, pc, u, v);
    const double e0 = (double)B.obs[2 * e] - u, e1 = (double)B.obs[2 * e + 1] - v, info = (double)B.info[e];
    const double c = e0 * info * e0 + e1 * info * e1;
    if (B.off[e]) {                                                         // inactive edge: contributes nothing to H, b, Y
        const int slot0 = B.rowSlot[e];
        if (slot0 >= 0) {
            double *hp = B.Hpl + (size_t)e * 18, *rp = B.panel + (size_t)slot0 * 8;
#pragma unroll
            for (int k = 0; k < 18; k++) hp[k] = 0;
#pragma unroll
            for (int k = 0; k < 16; k++) rp[k] = 0;
        }
    } else {
    double r0 = c, r1 = 1;
    if (B.robust) huber(c, B.delta, B.dsqr, r0, r1);
    const double w = r1 * info;
    double J0[6], J1[6], R[3][3], A0[3], A1[3];
    jac_pose(B.cam, pc, J0, J1);
    quat_to_matrix(P.r, R);
    const double iz = 1.0 / pc.z, iz2 = iz * iz;
    const double j00 = B.cam.fx * iz, j02 = -B.cam.fx * pc.x * iz2, j11 = B.cam.fy * iz, j12 = -B.cam.fy * pc.y * iz2;
#pragma unroll
    for (int k = 0; k < 3; k++) { A0[k] = -(j00 * R[0][k] + j02 * R[2][k]); A1[k] = -(j11 * R[1][k] + j12 * R[2][k]); }   // -projectJac * R
    // landmark block and right-hand side: summed over the landmark's run below
    {
        int q = 0;
#pragma unroll
        for (int a = 0; a < 3; a++) {
            blv[a] = -w * (A0[a] * e0 + A1[a] * e1);
#pragma unroll
            for (int c2 = a; c2 < 3; c2++) hl[q++] = w * (A0[a] * A0[c2] + A1[a] * A1[c2]);
        }
    }
    const int slot = B.rowSlot[e];
    if (slot >= 0) {
        double *hp = B.Hpl + (size_t)e * 18;
#pragma unroll
        for (int a = 0; a < 6; a++)
#pragma unroll
            for (int c2 = 0; c2 < 3; c2++) hp[a * 3 + c2] = w * (J0[a] * A0[c2] + J1[a] * A1[c2]);
        const double sw = sqrt(w);
        double *r0p = B.panel + (size_t)slot * 8, *r1p = r0p + 8;
#pragma unroll
        for (int a = 0; a < 6; a++) { r0p[a] = sw * J0[a]; r1p[a] = sw * J1[a]; }
        r0p[6] = sw * e0; r0p[7] = 0; r1p[6] = sw * e1; r1p[7] = 0;
    }
    }   // active edge
    }   // live edge
    double *Hl = B.Hll + (size_t)max(pKey, 0) * 9, *bL = B.bl + (size_t)max(pKey, 0) * 3;
    seg_reduce_atomic(blv[0], pKey, head, &bL[0]); seg_reduce_atomic(blv[1], pKey, head, &bL[1]); seg_reduce_atomic(blv[2], pKey, head, &bL[2]);
    // upper triangle 00 01 02 11 12 22; the mirrored entries get the same sums
    {
        const int at[6] = {0, 1, 2, 4, 5, 8}, mir[6] = {-1, 3, 6, -1, 7, -1};
#pragma unroll
        for (int q = 0; q < 6; q++) {
            double v = hl[q];
            const int lanei = lane;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const double vo = __shfl_down(v, d);
                const int po = __shfl_down(pKey, d);
                if (lanei + d < 64 && po == pKey) v += vo;
            }
            if (head && pKey >= 0) { atomicAdd(&Hl[at[q]], v); if (mir[q] >= 0) atomicAdd(&Hl[mir[q]], v); }
        }
    }
}

// H_pp(kf) = sum over the key-frame's rows of row^T row on the f64 matrix cores; [0:6,0:6] is the 6x6 block, -[0:6,6] is b_p.
// Lane l feeds element (row l>>4, column l&15) of a 4-row chunk as BOTH operands (A = chunk^T, B = chunk).
// grid (nOpt, kHppSlices): every wave owns an interleaved subset of the 4-row chunks (4 loads in flight per wave); the
// slices of one key-frame are combined with f64 atomics into the zeroed H_pp / b_p.
constexpr int kHppSlices = 16;
__global__ __launch_bounds__(256) void k_ba_hpp_mfma(BADev B) {
    const int kf = blockIdx.x, lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int r0 = B.kfRowStart[kf], r1 = B.kfRowStart[kf + 1];
    const int col = lane & 15, sub = lane >> 4;
    const int nw = kHppSlices * 4, w = blockIdx.y * 4 + wave;
    constexpr int U = 16;                                  // 4-row chunks in flight per wave: the loop is bound by memory latency, not by the 64-cycle MFMAs
    v4f64 acc = {0, 0, 0, 0};
    if (r1 > r0) {
        for (int r = r0 + w * 4; r < r1; r += nw * 4 * U) {
            double v[U];
#pragma unroll
            for (int u = 0; u < U; u++) {                  // clamped address, no branch around the load
                const int row = r + u * nw * 4 + sub;
                v[u] = B.panel[(size_t)min(row, r1 - 1) * 8 + (col & 7)];
            }
#pragma unroll
            for (int u = 0; u < U; u++) {
                const int row = r + u * nw * 4 + sub;
                const double x = (row < r1 && col < 8) ? v[u] : 0.0;
                acc = __builtin_amdgcn_mfma_f64_16x16x4f64(x, x, acc, 0, 0, 0);
            }
        }
    }
    // D[row = sub + 4*reg][col]: rows 0..7 live in reg 0 and reg 1
#pragma unroll
    for (int reg = 0; reg < 2; reg++) {
        const int a = sub + 4 * reg, c = col;
        const double g = acc[reg];
        if (g != 0.0) {
            if (a < 6 && c < 6) atomicAdd(&B.Hpp[(size_t)kf * 36 + a * 6 + c], g);
            if (a < 6 && c == 6) atomicAdd(&B.bp[(size_t)kf * 6 + a], -g);
        }
    }
}

// one launch instead of a memset per array
struct ZeroList { double *p[4]; int n[4]; };
__global__ void k_ba_zero(ZeroList Z) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
#pragma unroll
    for (int s = 0; s < 4; s++) if (i < Z.n[s]) Z.p[s][i] = 0.0;
}

__global__ void k_ba_maxdiag(BADev B) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    double m = 0;
    if (i < B.nOpt * 6) m = fabs(B.Hpp[(size_t)(i / 6) * 36 + (i % 6) * 7]);
    else if (i < B.nOpt * 6 + B.nMP * 3) { const int j = i - B.nOpt * 6; m = fabs(B.Hll[(size_t)(j / 3) * 9 + (j % 3) * 4]); }
    else return;
    atomicMax(reinterpret_cast<unsigned long long *>(&B.scal[2]), (unsigned long long)__double_as_longlong(m));   // m >= 0: bit order = value order
}

// Schur complement as a dense SYRK on the f64 matrix cores.  With D^-1 = L L^T (3x3 Cholesky per landmark) the update is
//   S = H_pp + lambda I - Y Y^T,   b_s = b_p - Y z,     Y(:, 3p..3p+2) = stack of H_pl(e) L over the landmark's edges,  z = L^T b_l,
// and Y is ~75 % dense for a covisibility window (every landmark is seen by most key-frames), so the block-sparse loops of
// g2o (block_solver.hpp:379-438) become one Gram product.  Yt is stored K-major: row k = 3p+c holds the NP-padded column
// of Y plus z in entry n, so the augmented Gram matrix G = Yt^T Yt carries Y Y^T in G[0:n,0:n] and Y z in G[0:n,n].
// D^-1 of a landmark's block by cofactors and its 3x3 Cholesky factor: the one copy of this arithmetic
__device__ __forceinline__ void dinv_factor(const double *Hll, double lambda, double (&I)[9], double (&L)[6]) {
    double D[9];
#pragma unroll
    for (int i = 0; i < 9; i++) D[i] = Hll[i];
    D[0] += lambda; D[4] += lambda; D[8] += lambda;
    const double c00 = D[4] * D[8] - D[5] * D[7], c01 = D[5] * D[6] - D[3] * D[8], c02 = D[3] * D[7] - D[4] * D[6];
    const double id = 1.0 / (D[0] * c00 + D[1] * c01 + D[2] * c02);        // Eigen Matrix3d::inverse (cofactors)
    I[0] = c00 * id; I[1] = (D[2] * D[7] - D[1] * D[8]) * id; I[2] = (D[1] * D[5] - D[2] * D[4]) * id;
    I[3] = c01 * id; I[4] = (D[0] * D[8] - D[2] * D[6]) * id; I[5] = (D[2] * D[3] - D[0] * D[5]) * id;
    I[6] = c02 * id; I[7] = (D[1] * D[6] - D[0] * D[7]) * id; I[8] = (D[0] * D[4] - D[1] * D[3]) * id;
    const double l00 = sqrt(I[0]), l10 = I[3] / l00, l20 = I[6] / l00;
    const double l11 = sqrt(I[4] - l10 * l10), l21 = (I[7] - l20 * l10) / l11, l22 = sqrt(I[8] - l20 * l20 - l21 * l21);
    L[0] = l00; L[1] = l10; L[2] = l20; L[3] = l11; L[4] = l21; L[5] = l22;
}
// the landmark's share of a trial: D^-1 -> B.Dinv, L -> Lp, z = L^T b_l -> entry B.n of the landmark's three rows of Yt
__device__ __forceinline__ void dinv_landmark(const BADev &B, int p, double lambda, double *Yt, int NP, double *Lp) {
    double I[9], L[6];
    dinv_factor(B.Hll + (size_t)p * 9, lambda, I, L);
#pragma unroll
    for (int i = 0; i < 9; i++) B.Dinv[(size_t)p * 9 + i] = I[i];
#pragma unroll
    for (int i = 0; i < 6; i++) Lp[(size_t)p * 6 + i] = L[i];
    const double b0 = B.bl[3 * p], b1 = B.bl[3 * p + 1], b2 = B.bl[3 * p + 2];
    double *y0 = Yt + (size_t)(3 * p) * NP;
    y0[B.n] = L[0] * b0 + L[1] * b1 + L[2] * b2; y0[NP + B.n] = L[3] * b1 + L[4] * b2; y0[2 * NP + B.n] = L[5] * b2;    // z = L^T b_l
}
// The landmark part alone, for the large-window path: ba_solve_big launches it with B.n = 0 and NP = 1, so that z lands in Yt[3 p .. 3 p + 2].
__global__ void k_ba_dinv(BADev B, double lambda, double *Yt, int NP, double *Lp) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p < B.nMP) dinv_landmark(B, p, lambda, Yt, NP, Lp);
}

// The landmark part and the panel fill in one launch (one round of kernel-launch and memory latency less per LM trial): threads [0, nMP) do the
// landmark part; threads [nMP, nMP + nE) fill the panel from the factor of their landmark's block, which each recomputes (45 flops) rather than read.
__global__ __launch_bounds__(256) void k_ba_dinv_yfill(BADev B, double lambda, double *Yt, int NP, double *Lp) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t < B.nMP) { dinv_landmark(B, t, lambda, Yt, NP, Lp); return; }
    const int e = t - B.nMP;
    if (e >= B.nE) return;
    const int col = B.poseCol[B.eKF[e]];
    if (col < 0) return;
    const int p = B.eMP[e];
    double I[9], L[6];
    dinv_factor(B.Hll + (size_t)p * 9, lambda, I, L);
    const double *h = B.Hpl + (size_t)e * 18;
    double *y0 = Yt + (size_t)(3 * p) * NP + col * 6, *y1 = y0 + NP, *y2 = y1 + NP;
#pragma unroll
    for (int a = 0; a < 6; a++) {
        const double h0 = h[a * 3], h1 = h[a * 3 + 1], h2 = h[a * 3 + 2];
        y0[a] = h0 * L[0] + h1 * L[1] + h2 * L[2];
        y1[a] = h1 * L[3] + h2 * L[4];
        y2[a] = h2 * L[5];
    }
}

// G += Yt^T Yt over a K-slice; one wave per (upper 16x16 tile, slice); grid tiles x slices/4, 256 threads.  A wave's 36-odd MFMAs take 2.3 k
// cycles, one round trip to L2 / HBM about as long: the slice is walked in chunks of 64 rows (16 operand pairs per lane) with the loads of two
// chunks in flight before the first MFMA, so the kernel pays the memory latency once per wave, not once per 16 rows.
__global__ __launch_bounds__(256) void k_ba_syrk_mfma(const double *__restrict__ Yt, int K, int NP, int nSlices, double *G) {
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int NT = NP / 16;
    // 1-D grid of tiles x slice groups.  Workgroups go round-robin over the 8 XCDs, each with its own L2: the mapping below gives every XCD
    // its own slice groups (all tiles of them), so that a row of Yt is fetched from memory by ONE L2 instead of by all eight
    const int nTiles = NT * (NT + 1) / 2, nGroups = nSlices / 4;
    int lin = blockIdx.x;
    if (nGroups % 8 == 0) { const int xcd = lin & 7, within = lin >> 3, gpx = nGroups / 8; lin = (xcd * gpx + within / nTiles) * nTiles + within % nTiles; }
    int t = lin % nTiles, tr = 0;                       // upper-triangle tile index -> (tr, tc)
    while (t >= NT - tr) { t -= NT - tr; tr++; }
    const int tc = tr + t;
    const int slice = (lin / nTiles) * 4 + wave;
    const int per = (((K + nSlices - 1) / nSlices) + 3) & ~3;
    const int k0 = slice * per, k1 = min(K, k0 + per);
    if (k0 >= k1) return;
    const int i = lane & 15, kk = lane >> 4;
    constexpr int C = 16;                               // 4-row steps per chunk
    const double *pa = Yt + tr * 16 + i, *pb = Yt + tc * 16 + i;
    double a0[C], b0[C], a1[C], b1[C];
    auto load = [&](double (&a)[C], double (&b)[C], int kb) {
#pragma unroll
        for (int u = 0; u < C; u++) {
            const size_t row = (size_t)min(kb + 4 * u + kk, k1 - 1);          // clamped: no branch around the loads
            a[u] = pa[row * NP]; b[u] = pb[row * NP];
        }
    };
    v4f64 acc = {0, 0, 0, 0};
    auto mma = [&](const double (&a)[C], const double (&b)[C], int kb) {
#pragma unroll
        for (int u = 0; u < C; u++) {
            const bool ok = kb + 4 * u + kk < k1;
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(ok ? a[u] : 0.0, ok ? b[u] : 0.0, acc, 0, 0, 0);
        }
    };
    load(a0, b0, k0);
    if (k0 + 4 * C < k1) load(a1, b1, k0 + 4 * C);
    for (int kb = k0; kb < k1; kb += 8 * C) {
        mma(a0, b0, kb);
        if (kb + 8 * C < k1) load(a0, b0, kb + 8 * C);
        if (kb + 4 * C < k1) {
            mma(a1, b1, kb + 4 * C);
            if (kb + 12 * C < k1) load(a1, b1, kb + 12 * C);
        }
    }
#pragma unroll
    for (int reg = 0; reg < 4; reg++) {
        const double g = acc[reg];
        if (g != 0.0) atomicAdd(&G[(size_t)(tr * 16 + kk + 4 * reg) * NP + tc * 16 + i], g);
    }
}

// The LM control flow lives on the host (it must poll the reference's stop flag between trials), and every trial ends with a decision on eight
// scalars.  Instead of a device-to-host copy plus hipStreamSynchronize (~30 us of runtime latency per trial) the scalars are PUBLISHED into
// fine-grained pinned host memory by a one-wave kernel, followed by a sequence number; the host spins on that number (a few us).
__global__ void k_ba_publish(const double *__restrict__ scal, volatile double *hostScal, unsigned long long seq) {
    if (threadIdx.x < 8) hostScal[threadIdx.x] = scal[threadIdx.x];
    __threadfence_system();
    __builtin_amdgcn_s_barrier();
    if (threadIdx.x == 0) __hip_atomic_store(reinterpret_cast<unsigned long long *>(const_cast<double *>(hostScal + 8)), seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

// Reduced system (H_pp + lambda I - Y Y^T) x_p = b_p - Y z of the windows too large for the tile solver (30..42 optimised key-frames, 180..252
// unknowns): blocked right-looking Cholesky (panel width 8) of the matrix augmented with the right-hand side as an extra ROW (its factor row is the
// forward substitution), in one workgroup.  Per panel: wave 0 factors the 8x8 diagonal block in registers and publishes it through LDS, one thread
// per row solves its 8 panel entries, then the trailing matrix takes the rank-8 update: three barriers per 8 columns.  The backward substitution
// keeps y in the registers of wave 0 and walks rows of L (contiguous), so its serial chain is a broadcast and one FMA per unknown.
// The matrix lives in `A` (global memory, served by L2): at 180 unknowns it is 263 KB, more than the LDS of a CU.
constexpr int kPW = 8;
__global__ __launch_bounds__(1024) void k_ba_solve(BADev B, double lambda, const double *G, int NP, double *A) {
    __shared__ double ldb[kPW * kPW], rdb[kPW];
    __shared__ int sFail;
    const int n = B.n, tid = threadIdx.x, nt = blockDim.x;
    const int ld = n + 1;
    double *rdg = A + (size_t)(n + 1) * ld;                  // reciprocals of the factor's diagonal
    auto g = [&](int r, int c) -> double { return (r / 16 <= c / 16) ? G[(size_t)r * NP + c] : G[(size_t)c * NP + r]; };
    if (tid == 0) sFail = 0;
    for (int idx = tid; idx < (n + 1) * n; idx += nt) {
        const int i = idx / n, j = idx - i * n;
        if (j > i) continue;
        double v;
        if (i == n) v = B.bp[j] - g(j, n);
        else {
            v = -g(i, j);
            if (i / 6 == j / 6) v += B.Hpp[(size_t)(i / 6) * 36 + (i % 6) * 6 + (j % 6)];
            if (i == j) v += lambda;
        }
        A[(size_t)i * ld + j] = v;
    }
    __syncthreads();
    for (int c0 = 0; c0 < n; c0 += kPW) {
        const int w = min(kPW, n - c0);
        if (tid < 64) {                                      // wave 0: 8x8 diagonal block in registers (all lanes alike)
            double Ld[kPW][kPW], rd[kPW];
#pragma unroll
            for (int a = 0; a < kPW; a++)
#pragma unroll
                for (int b = 0; b < kPW; b++) Ld[a][b] = (a < w && b <= a) ? A[(size_t)(c0 + a) * ld + c0 + b] : (a == b ? 1.0 : 0.0);
            bool bad = false;
#pragma unroll
            for (int j = 0; j < kPW; j++) {
                double d = Ld[j][j];
#pragma unroll
                for (int k = 0; k < kPW; k++) if (k < j) d -= Ld[j][k] * Ld[j][k];
                if (!(d > 0) || !isfinite(d)) bad = true;
                const double rs = fast_rsqrt(d);
                rd[j] = rs;
                Ld[j][j] = d * rs;
#pragma unroll
                for (int i = 0; i < kPW; i++) if (i > j) {
                    double t = Ld[i][j];
#pragma unroll
                    for (int k = 0; k < kPW; k++) if (k < j) t -= Ld[i][k] * Ld[j][k];
                    Ld[i][j] = t * rs;
                }
            }
            // publish: lane (a*8+b) stores one entry of the block (static register selection)
            double mine = 0, myrd = 0;
#pragma unroll
            for (int a = 0; a < kPW; a++)
#pragma unroll
                for (int b = 0; b < kPW; b++) if (tid == a * kPW + b) mine = Ld[a][b];
#pragma unroll
            for (int a = 0; a < kPW; a++) if (tid == a) myrd = rd[a];
            ldb[tid] = mine;
            if (tid < kPW) { rdb[tid] = myrd; if (tid < w) rdg[c0 + tid] = myrd; }
            const int a = tid / kPW, b = tid - a * kPW;
            if (a < w && b <= a) A[(size_t)(c0 + a) * ld + c0 + b] = mine;    // nobody else reads the diagonal block now
            if (tid == 0 && bad) sFail = 1;
        }
        __syncthreads();
        if (sFail) break;
        // rows below the block: L[r][c0..] = A[r][c0..] * Ld^-T  (one thread per row)
        if (c0 + w + tid <= n) {                              // the block's factor, once per thread, into registers
            double lb[kPW][kPW], rb[kPW];
#pragma unroll
            for (int b = 0; b < kPW; b++) {
                rb[b] = rdb[b];
#pragma unroll
                for (int k = 0; k < kPW; k++) lb[b][k] = k < b ? ldb[b * kPW + k] : 0.0;
            }
        for (int r = c0 + w + tid; r <= n; r += nt) {
            double x[kPW];
#pragma unroll
            for (int b = 0; b < kPW; b++) x[b] = b < w ? A[(size_t)r * ld + c0 + b] : 0.0;
#pragma unroll
            for (int b = 0; b < kPW; b++) {
                double t = x[b];
#pragma unroll
                for (int k = 0; k < kPW; k++) if (k < b) t -= x[k] * lb[b][k];
                x[b] = t * rb[b];
            }
#pragma unroll
            for (int b = 0; b < kPW; b++) if (b < w) A[(size_t)r * ld + c0 + b] = x[b];
        }
        }
        __syncthreads();
        // trailing update: A[i][k] -= sum_q L[i][c0+q] L[k][c0+q] for c0+w <= k <= i <= n, k < n
        // 32 x 32 thread grid over the lower triangle: thread (ty, tx) owns rows i = t0 + ty + 32 a, columns k = t0 + tx + 32 b, k <= i;
        // the panel entries of its rows / columns are read once per (a, b) tile row / column, no integer division
        const int t0 = c0 + w;
        const int ty = tid >> 5, tx = tid & 31;
        for (int i = t0 + ty; i <= n; i += 32) {
            double li[kPW];
#pragma unroll
            for (int q = 0; q < kPW; q++) li[q] = q < w ? A[(size_t)i * ld + c0 + q] : 0.0;
            for (int k = t0 + tx; k <= i && k < n; k += 32) {
                double acc = 0;
#pragma unroll
                for (int q = 0; q < kPW; q++) if (q < w) acc += li[q] * A[(size_t)k * ld + c0 + q];
                A[(size_t)i * ld + k] -= acc;
            }
        }
        __syncthreads();
    }
    if (sFail) {
        if (tid == 0) B.scal[3] = 0.0;
        for (int i = tid; i < n; i += nt) B.x[i] = 0;
        return;
    }
    // backward substitution L^T x = y on wave 0: lane owns unknowns lane, lane+64, lane+128, lane+192
    if (tid < 64) {
        double y[4], x[4] = {0, 0, 0, 0};
#pragma unroll
        for (int q = 0; q < 4; q++) { const int i = tid + 64 * q; y[q] = i < n ? A[(size_t)n * ld + i] : 0.0; }
        for (int j = n - 1; j >= 0; j--) {
            const int jq = j >> 6, jl = j & 63;
            double row[4];                                   // row j of L: independent of the chain, issued first
#pragma unroll
            for (int q = 0; q < 4; q++) { const int i = tid + 64 * q; row[q] = i < j ? A[(size_t)j * ld + i] : 0.0; }
            const double rdj = rdg[j];
            const double ysel = jq == 0 ? y[0] : jq == 1 ? y[1] : jq == 2 ? y[2] : y[3];
            const double xj = readlane_f64(ysel, jl) * rdj;        // jl is wave-uniform: a readlane, not an LDS-routed shuffle
#pragma unroll
            for (int q = 0; q < 4; q++) {
                y[q] -= row[q] * xj;
                if (q == jq && tid == jl) x[q] = xj;
            }
        }
#pragma unroll
        for (int q = 0; q < 4; q++) { const int i = tid + 64 * q; if (i < n) B.x[i] = x[q]; }
        if (tid == 0) B.scal[3] = 1.0;
    }
}

// x_l = D^-1 (b_l - H_pl^T x_p); trial state = oplus(current, x); scale += x^T (lambda x + b)
// Landmark back-substitution x_l = D^-1 (b_l - H_pl^T x_p) (block_solver.hpp:468-481), oplus of points and poses, and the
// gain-ratio denominator.  Eight lanes share a landmark (its ~15 edges are two rounds instead of fifteen dependent ones); the
// first nKF * 8 lanes past the landmarks carry the poses (one per group of eight).
constexpr int kLmLanes = 8;
__global__ __launch_bounds__(256) void k_ba_update(BADev B, double lambda, const double *T, const double *X, double *Tt, double *Xt) {
    __shared__ double red[4];
    const int gi = (blockIdx.x * 256 + threadIdx.x) / kLmLanes, sub = threadIdx.x & (kLmLanes - 1);
    double acc[1] = {0};
    if (gi < B.nMP) {
        const int p = gi;
        double c0 = 0, c1 = 0, c2 = 0;
        for (int s = B.ptStart[p] + sub; s < B.ptStart[p + 1]; s += kLmLanes) {
            const int e = B.ptEdge[s], col = B.poseCol[B.eKF[e]];
            if (col < 0) continue;
            const double *h = B.Hpl + (size_t)e * 18, *xp = B.x + col * 6;
#pragma unroll
            for (int a = 0; a < 6; a++) { c0 -= h[a * 3] * xp[a]; c1 -= h[a * 3 + 1] * xp[a]; c2 -= h[a * 3 + 2] * xp[a]; }
        }
#pragma unroll
        for (int o = kLmLanes / 2; o > 0; o >>= 1) { c0 += __shfl_xor(c0, o, kLmLanes); c1 += __shfl_xor(c1, o, kLmLanes); c2 += __shfl_xor(c2, o, kLmLanes); }
        if (sub == 0) {
            const double b0 = B.bl[3 * p], b1 = B.bl[3 * p + 1], b2 = B.bl[3 * p + 2];
            c0 += b0; c1 += b1; c2 += b2;
            const double *I = B.Dinv + (size_t)p * 9;
            const double x0 = I[0] * c0 + I[1] * c1 + I[2] * c2, x1 = I[3] * c0 + I[4] * c1 + I[5] * c2, x2 = I[6] * c0 + I[7] * c1 + I[8] * c2;
            B.x[B.n + 3 * p] = x0; B.x[B.n + 3 * p + 1] = x1; B.x[B.n + 3 * p + 2] = x2;
            Xt[3 * p] = X[3 * p] + x0; Xt[3 * p + 1] = X[3 * p + 1] + x1; Xt[3 * p + 2] = X[3 * p + 2] + x2;
            acc[0] = x0 * (lambda * x0 + b0) + x1 * (lambda * x1 + b1) + x2 * (lambda * x2 + b2);
        }
    } else if (gi < B.nMP + B.nKF && sub == 0) {
        const int k = gi - B.nMP, col = B.poseCol[k];
        DSE3 P = load_pose(T, k);
        if (col >= 0) {
            const double *xp = B.x + col * 6;
            double u[6];
            for (int a = 0; a < 6; a++) { u[a] = xp[a]; acc[0] += xp[a] * (lambda * xp[a] + B.bp[col * 6 + a]); }
            P = se3_mul(se3_exp(u), P);
        }
        store_pose(Tt, k, P);
    }
    block_sum<1>(acc, red);
    if (threadIdx.x == 0 && acc[0] != 0.0) atomicAdd(&B.scal[1], acc[0]);
}

// merge BA, between its two optimisations (Optimizer.cc:3996-4010): edges with chi2 > 5.991 or non-positive depth go to level 1
__global__ void k_ba_mark(BADev B, const double *T, const double *X, uint8_t *off) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= B.nE) return;
    const int p = B.eMP[e];
    const D3 pc = se3_map(load_pose(T, B.eKF[e]), D3{X[3 * p], X[3 * p + 1], X[3 * p + 2]});
    off[e] = (B.lastChi2[e] > 5.991 || !(pc.z > 0.0)) ? 1 : 0;
}

// erase flags of the edges (Optimizer.cc:1292) and, in the same launch, the final state gathered behind them: [T | X | erase] leaves in one copy
__global__ void k_ba_finalize(BADev B, const double *T, const double *X, int useLast, uint8_t *erase, double *outT, double *outX) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e < B.nKF * 8) outT[e] = T[e];
    if (e < B.nMP * 3) outX[e] = X[e];
    if (e >= B.nE) return;
    const int p = B.eMP[e];
    const D3 pc = se3_map(load_pose(T, B.eKF[e]), D3{X[3 * p], X[3 * p + 1], X[3 * p + 2]});
    double chi2 = B.lastChi2[e];
    if (!useLast) {
        double u, v;
        cam_project(B.cam, pc, u, v);
        const double e0 = (double)B.obs[2 * e] - u, e1 = (double)B.obs[2 * e + 1] - v, w = (double)B.info[e];
        chi2 = e0 * w * e0 + e1 * w * e1;
    }
    erase[e] = (chi2 > 5.991 || !(pc.z > 0.0)) ? 1 : 0;       // Optimizer.cc:1292
}
