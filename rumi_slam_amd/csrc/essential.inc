// Optimizer::OptimizeEssentialGraph (R/lib_src/Optimizer.cc:1357-1623 and its merge overload :1625-1918): the Sim3 pose graph.  Included by
// opt.hip inside namespace rumi, after the blocked Cholesky (k_chol_*), which factors the dense 7 nR x 7 nR system of every LM trial.
//
// Vertices are g2o::VertexSim3Expmap (estimate (qx qy qz qw tx ty tz s) in double), edges g2o::EdgeSim3 with error log(C * S_v0 * S_v1^-1)
// and identity information.  Only ACTIVE edges reach the device: the host drops an edge whose two ends are fixed, as
// SparseOptimizer::initializeOptimization does (G/core/sparse_optimizer.cpp:234, `!e->allVerticesFixed()`).  A free vertex with an edge
// owns block row col[v] (vertex order); every other vertex has col[v] = -1.
//
// Per-edge buffer (kEgStride doubles): [0,49) J0^T J0, [49,98) J1^T J0, [98,147) J1^T J1, [147,154) -J0^T e, [154,161) -J1^T e, row-major.
// No floating-point atomics: a block row of the matrix is written by one wave only, every sum runs in a fixed order.
constexpr int kEgStride = 168;
constexpr int kEgEdgesPerBlock = 16;             // 256 threads: 16 lanes an edge, four edges a wave

struct EGDev {
    int nV, nE, nR, n;
    const int32_t *ev0, *ev1;
    const double *meas;
    const uint8_t *fixed, *fixScale;
    const int32_t *col, *rowStart, *inc;         // inc[k] = 2 * edge + (the row's vertex is the edge's vertex 1)
    double *EB, *chiE, *A, *bvec, *x, *part, *scal;
};

__device__ inline void eg_error(const DSim3 &C, const DSim3 &S0, const DSim3 &S1, double e[7]) {
    sim3_log(sim3_mul(sim3_mul(C, S0), sim3_inverse(S1)), e);
}
// VertexSim3Expmap::oplusImpl on a copy of the estimate: Sim3(update) * estimate, update[6] = 0 under _fix_scale
__device__ inline DSim3 eg_oplus(const DSim3 &S, double u[7], bool fixScale) {
    if (fixScale) u[6] = 0;
    return sim3_mul(sim3_exp(u), S);
}

// BaseBinaryEdge::linearizeOplus (G/core/base_binary_edge.hpp: central differences, delta 1e-9) and the edge's part of the quadratic form.
// Lane l < 14 of an edge's 16 owns Jacobian column l (end l / 7, component l % 7): it applies +delta and -delta to its component of its
// end's estimate and evaluates the error twice; lane 14 evaluates the error itself; lanes of a fixed end idle on zero columns.  The 7 x 15
// panel [J0 | J1 | e] goes through LDS, then the 16 lanes share the 161 dot products of the products above.
__global__ __launch_bounds__(256) void k_eg_linearise(EGDev G, const double *S) {
    __shared__ double sJ[kEgEdgesPerBlock][7][16];
    const int slot = threadIdx.x >> 4, l = threadIdx.x & 15, e = blockIdx.x * kEgEdgesPerBlock + slot;
    const bool live = e < G.nE;
    if (live) {
        const int v0 = G.ev0[e], v1 = G.ev1[e];
        const DSim3 C = sim3_from8(G.meas + (size_t)e * 8), S0 = sim3_from8(S + (size_t)v0 * 8), S1 = sim3_from8(S + (size_t)v1 * 8);
        double c[7] = {0, 0, 0, 0, 0, 0, 0};
        if (l < 14) {
            const int end = l >= 7, comp = l - 7 * end, v = end ? v1 : v0;
            if (!G.fixed[v]) {
                const bool fs = G.fixScale[v] != 0;
                const double delta = 1e-9, scalar = 1.0 / (2 * delta);
                double u[7], ep[7], em[7];
                for (int i = 0; i < 7; i++) u[i] = i == comp ? delta : 0.0;
                { const DSim3 Sp = eg_oplus(end ? S1 : S0, u, fs); eg_error(C, end ? S0 : Sp, end ? Sp : S1, ep); }
                for (int i = 0; i < 7; i++) u[i] = i == comp ? -delta : 0.0;
                { const DSim3 Sm = eg_oplus(end ? S1 : S0, u, fs); eg_error(C, end ? S0 : Sm, end ? Sm : S1, em); }
                for (int i = 0; i < 7; i++) c[i] = scalar * (ep[i] - em[i]);
            }
        } else if (l == 14) eg_error(C, S0, S1, c);
        for (int i = 0; i < 7; i++) sJ[slot][i][l] = c[i];
    }
    __syncthreads();
    if (!live) return;
    double *eb = G.EB + (size_t)e * kEgStride;
    for (int idx = l; idx < 161; idx += 16) {
        int ca, cb;
        double sign = 1.0;
        if (idx < 147) {
            const int blk = idx / 49, rem = idx - blk * 49, i = rem / 7, j = rem - i * 7;
            ca = (blk == 0 ? 0 : 7) + i; cb = (blk == 2 ? 7 : 0) + j;
        } else { ca = idx - 147; cb = 14; sign = -1.0; }
        double acc = 0;
        for (int k = 0; k < 7; k++) acc += sJ[slot][k][ca] * sJ[slot][k][cb];
        eb[idx] = sign * acc;
    }
}

// active chi2 of a state: one lane an edge, e^T e (identity information) to chiE[e]; k_eg_reduce sums them in a fixed order
__global__ __launch_bounds__(256) void k_eg_chi2(EGDev G, const double *S) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= G.nE) return;
    double r[7];
    eg_error(sim3_from8(G.meas + (size_t)e * 8), sim3_from8(S + (size_t)G.ev0[e] * 8), sim3_from8(S + (size_t)G.ev1[e] * 8), r);
    double acc = 0;
    for (int i = 0; i < 7; i++) acc += r[i] * r[i];
    G.chiE[e] = acc;
}

// [H + lambda I ; b^T] into the zeroed dense lower triangle (ld = n, right-hand side as row n, as k_chol_* expect it) and b into bvec.
// One wave a block row: lanes 0..48 carry the entries of a 7 x 7 block, lanes 49..55 the row's part of b.  The row's incident edges come in
// ascending edge index (CSR built by the host's counting sort): diagonal block and b accumulate in registers, an off-diagonal block (only
// the ones left of the diagonal: the other end owns an earlier row) is added to the matrix by the lane that owns the entry, so several edges
// between the same pair of vertices are summed in edge order.
__global__ __launch_bounds__(256) void k_eg_assemble(EGDev G, double lambda) {
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (r == 0 && lane == 0) G.scal[3] = 1.0;               // "factorisation succeeded" until k_chol_diag says otherwise
    if (r >= G.nR || lane >= 56) return;
    const int n = G.n, i = lane / 7, j = lane - i * 7;
    const bool ent = lane < 49;
    double acc = 0;
    for (int k = G.rowStart[r]; k < G.rowStart[r + 1]; k++) {
        const int code = G.inc[k], e = code >> 1, side = code & 1;
        const double *eb = G.EB + (size_t)e * kEgStride;
        acc += ent ? eb[side ? 98 + lane : lane] : eb[147 + side * 7 + (lane - 49)];
        const int r2 = G.col[side ? G.ev0[e] : G.ev1[e]];
        if (ent && r2 >= 0 && r2 < r)                      // side 1: J1^T J0 as stored; side 0: J0^T J1, its transpose
            G.A[(size_t)(7 * r + i) * n + 7 * r2 + j] += side ? eb[49 + i * 7 + j] : eb[49 + j * 7 + i];
    }
    if (ent) { if (j <= i) G.A[(size_t)(7 * r + i) * n + 7 * r + j] = i == j ? acc + lambda : acc; }
    else { G.A[(size_t)n * n + 7 * r + (lane - 49)] = acc; G.bvec[7 * r + (lane - 49)] = acc; }
}

// trial state = oplus(current, x) for the vertices that own rows (a copy for the others) and the row's share of x^T (lambda x + b)
__global__ __launch_bounds__(256) void k_eg_update(EGDev G, double lambda, const double *S, double *St) {
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= G.nV) return;
    const int r = G.col[v];
    if (r < 0) { for (int i = 0; i < 8; i++) St[(size_t)v * 8 + i] = S[(size_t)v * 8 + i]; return; }
    double u[7], acc = 0;
    for (int i = 0; i < 7; i++) { u[i] = G.x[7 * r + i]; acc += u[i] * (lambda * u[i] + G.bvec[7 * r + i]); }
    G.part[r] = acc;
    sim3_to8(eg_oplus(sim3_from8(S + (size_t)v * 8), u, G.fixScale[v] != 0), St + (size_t)v * 8);
}

// scal[0] = sum of chiE, scal[1] = sum of part (withScale): one workgroup, every thread a strided partial sum, then a tree in LDS
__global__ __launch_bounds__(256) void k_eg_reduce(EGDev G, int withScale) {
    __shared__ double s[2][256];
    const int t = threadIdx.x;
    double a = 0, b = 0;
    for (int e = t; e < G.nE; e += 256) a += G.chiE[e];
    if (withScale) for (int r = t; r < G.nR; r += 256) b += G.part[r];
    s[0][t] = a; s[1][t] = b;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (t < w) { s[0][t] += s[0][t + w]; s[1][t] += s[1][t + w]; }
        __syncthreads();
    }
    if (t == 0) { G.scal[0] = s[0][0]; G.scal[1] = s[1][0]; }
}

// L^T x = y (y = the factor's row n) by blocks of 64 from the back, as k_chol_backsub does, but with the unknowns in global memory (x itself)
// and only the current block's 64 in LDS: 7 * 2560 unknowns do not fit the LDS next to the diagonal block.  One workgroup; x[i] is updated by
// the thread i % 1024 only, the block solve (wave 0) is fenced from the updates by the workgroup barriers.
__global__ __launch_bounds__(1024) void k_eg_backsub(const double *A, int ld, int n, const double *rdg, double *x, const double *scal) {
    __shared__ double sD[kNB * kNB], sy[kNB];
    const int tid = threadIdx.x;
    if (scal[3] == 0.0) {                               // not positive definite: g2o's solve() fails, the LM step is rejected
        for (int i = tid; i < n; i += 1024) x[i] = 0;
        return;
    }
    for (int i = tid; i < n; i += 1024) x[i] = A[(size_t)n * ld + i];
    __syncthreads();
    for (int jb = (n + kNB - 1) / kNB - 1; jb >= 0; jb--) {
        const int j0 = jb * kNB, w = min(kNB, n - j0);
        for (int idx = tid; idx < kNB * kNB; idx += 1024) {
            const int r = idx / kNB, c = idx - r * kNB;
            sD[idx] = (r < w && c < r) ? A[(size_t)(j0 + r) * ld + j0 + c] : 0.0;
        }
        __syncthreads();
        if (tid < 64) {                                       // lane t carries unknown j0 + t; the solved one is broadcast by readlane
            double y = tid < w ? x[j0 + tid] : 0.0;
            const double rd = tid < w ? rdg[j0 + tid] : 0.0;
            for (int jj = w - 1; jj >= 0; jj--) {
                const double l = sD[jj * kNB + tid];          // row jj of the block (zero from the diagonal on)
                const double xj = readlane_f64(y, jj) * readlane_f64(rd, jj);
                y = tid == jj ? xj : y - l * xj;
            }
            sy[tid] = tid < w ? y : 0.0;
            if (tid < w) x[j0 + tid] = y;
        }
        __syncthreads();
        for (int i = tid; i < j0; i += 1024) {
            double acc0 = 0, acc1 = 0;
            const double *colp = A + (size_t)j0 * ld + i;
            int q = 0;
            for (; q + 2 <= w; q += 2) { acc0 += colp[(size_t)q * ld] * sy[q]; acc1 += colp[(size_t)(q + 1) * ld] * sy[q + 1]; }
            if (q < w) acc0 += colp[(size_t)q * ld] * sy[q];
            x[i] -= acc0 + acc1;
        }
        __syncthreads();
    }
}

// The map-point correction that ends both overloads, one lane a point; ref[i] < 0 leaves the point alone.
// mode 0 (Optimizer.cc:1611-1616): tabA[v] = Srw, tabB[v] = correctedSwr as Sim3 in double; X <- float(correctedSwr.map(Srw.map(double(X)))).
// mode 1 (Optimizer.cc:1907-1911): tabA[v] = Twr, tabB[v] = TNonCorrectedwr as SE(3) in float (qx qy qz qw tx ty tz);
//         X <- (Twr * TNonCorrectedwr^-1) * X, all in float, the product of the two transforms formed first, as upstream associates it.
__device__ inline void f_rotate(const float q[4], const float v[3], float o[3]) {       // Eigen _transformVector in float
    float uv[3] = {q[1] * v[2] - q[2] * v[1], q[2] * v[0] - q[0] * v[2], q[0] * v[1] - q[1] * v[0]};
    for (int k = 0; k < 3; k++) uv[k] += uv[k];
    const float c[3] = {q[1] * uv[2] - q[2] * uv[1], q[2] * uv[0] - q[0] * uv[2], q[0] * uv[1] - q[1] * uv[0]};
    for (int k = 0; k < 3; k++) o[k] = v[k] + q[3] * uv[k] + c[k];
}
__global__ __launch_bounds__(256) void k_sim3_correct_points(int mode, int n, float *X, const int32_t *ref, const void *tabA, const void *tabB) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int v = ref[i];
    if (v < 0) return;
    float *x = X + (size_t)i * 3;
    if (mode == 0) {
        const DSim3 A = sim3_from8((const double *)tabA + (size_t)v * 8), B = sim3_from8((const double *)tabB + (size_t)v * 8);
        const D3 p = sim3_map(B, sim3_map(A, D3{(double)x[0], (double)x[1], (double)x[2]}));
        x[0] = (float)p.x; x[1] = (float)p.y; x[2] = (float)p.z;
    } else {
        const float *a = (const float *)tabA + (size_t)v * 7, *b = (const float *)tabB + (size_t)v * 7;
        const float bi[4] = {-b[0], -b[1], -b[2], b[3]};                       // TNonCorrectedwr^-1 = (q*, -(q* t))
        float bt[3], q[4], t[3], o[3];
        f_rotate(bi, b + 4, bt);
        for (int k = 0; k < 3; k++) bt[k] = -bt[k];
        q[0] = a[3] * bi[0] + a[0] * bi[3] + a[1] * bi[2] - a[2] * bi[1];      // Twr * TNonCorrectedwr^-1
        q[1] = a[3] * bi[1] + a[1] * bi[3] + a[2] * bi[0] - a[0] * bi[2];
        q[2] = a[3] * bi[2] + a[2] * bi[3] + a[0] * bi[1] - a[1] * bi[0];
        q[3] = a[3] * bi[3] - a[0] * bi[0] - a[1] * bi[1] - a[2] * bi[2];
        f_rotate(a, bt, t);
        for (int k = 0; k < 3; k++) t[k] += a[4 + k];
        f_rotate(q, x, o);
        for (int k = 0; k < 3; k++) x[k] = o[k] + t[k];
    }
}
