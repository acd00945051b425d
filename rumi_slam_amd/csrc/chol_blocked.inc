// chol_blocked.inc -- multi-workgroup blocked Cholesky (panel kNB) of a dense lower triangle with the right-hand side as the extra row, and its backward
// substitution: large-window bundle adjustment (ba_single_host.inc) and essential graph (essential_host.inc).  Included by opt.hip inside namespace rumi.
constexpr int kNB = 64;

// diagonal block [j0, j0 + w) in LDS, sub-panels of 8 columns: wave 0 factors the 8 x 8 sub-diagonal in registers (every lane the same
// values: a chain of 36 dependent steps instead of 8 LDS round trips), lane i solves row i against it and publishes the row's eight entries;
// then four waves (lane = row, 16 columns each) take the trailing update with 8-term dot products.  Rows past w carry an identity; the
// update also runs over the unused upper triangle, which keeps the loops uniform.
__global__ __launch_bounds__(256) void k_chol_diag(double *A, int ld, int n, int j0, double *rdg, double *scal) {
    constexpr int kS = kNB + 1, kP = 8;
    __shared__ double S[kNB * kS];
    __shared__ double P[kNB * kP];                         // the current sub-panel, row-major: P[i][q] = L[i][c0 + q]
    const int tid = threadIdx.x, lane = tid & 63, part = tid >> 6, w = min(kNB, n - j0);
    for (int idx = tid; idx < kNB * kNB; idx += 256) {
        const int r = idx / kNB, c = idx - r * kNB;
        S[r * kS + c] = (r < w && c <= r) ? A[(size_t)(j0 + r) * ld + j0 + c] : (r == c ? 1.0 : 0.0);
    }
    __syncthreads();
    bool bad = false;
    double myRs = 1.0;
    double *__restrict__ row = S + lane * kS;
    for (int c0 = 0; c0 < kNB; c0 += kP) {
        if (part == 0) {
            double Ld[kP][kP], rd[kP];
#pragma unroll
            for (int a = 0; a < kP; a++)
#pragma unroll
                for (int b = 0; b < kP; b++) Ld[a][b] = b <= a ? S[(c0 + a) * kS + c0 + b] : 0.0;
#pragma unroll
            for (int j = 0; j < kP; j++) {
                double d = Ld[j][j];
#pragma unroll
                for (int k = 0; k < j; k++) d -= Ld[j][k] * Ld[j][k];
                if (!(d > 0) || !isfinite(d)) bad = true;
                const double rs = fast_rsqrt(d);
                rd[j] = rs;
                Ld[j][j] = d * rs;
#pragma unroll
                for (int i = j + 1; i < kP; i++) {
                    double t = Ld[i][j];
#pragma unroll
                    for (int k = 0; k < j; k++) t -= Ld[i][k] * Ld[j][k];
                    Ld[i][j] = t * rs;
                }
            }
            // own row: rows of the sub-diagonal take their factor row, rows below solve x Ld^T = a, rows above keep zeros
            double x[kP];
#pragma unroll
            for (int b = 0; b < kP; b++) x[b] = row[c0 + b];
            const int a = lane - c0;
#pragma unroll
            for (int b = 0; b < kP; b++) {
                double t = x[b];
#pragma unroll
                for (int k = 0; k < b; k++) t -= x[k] * Ld[b][k];
                x[b] = t * rd[b];
            }
#pragma unroll
            for (int q = 0; q < kP; q++) {
#pragma unroll
                for (int b = 0; b < kP; b++) if (a == q) { x[b] = b <= q ? Ld[q][b] : 0.0; if (b == q) myRs = rd[q]; }
            }
            if (a < 0) {
#pragma unroll
                for (int b = 0; b < kP; b++) x[b] = 0.0;
            }
#pragma unroll
            for (int b = 0; b < kP; b++) { if (a >= 0) row[c0 + b] = x[b]; P[lane * kP + b] = x[b]; }
        }
        __syncthreads();
        if (part * 16 + 15 >= c0 + kP) {                  // this wave's 16 columns of the trailing block
            double li[kP];
#pragma unroll
            for (int q = 0; q < kP; q++) li[q] = P[lane * kP + q];
#pragma unroll 4
            for (int u = 0; u < 16; u++) {
                const int k = part * 16 + u;
                double acc = 0;
#pragma unroll
                for (int q = 0; q < kP; q++) acc += li[q] * P[k * kP + q];
                if (k >= c0 + kP) row[k] -= acc;
            }
        }
        __syncthreads();
    }
    for (int idx = tid; idx < kNB * kNB; idx += 256) {
        const int r = idx / kNB, c = idx - r * kNB;
        if (r < w && c <= r) A[(size_t)(j0 + r) * ld + j0 + c] = S[r * kS + c];
    }
    if (part == 0 && lane < w) rdg[j0 + lane] = myRs;
    if (bad && tid == 0) scal[3] = 0.0;
}

// rows below the block (the right-hand side row n included): L[r][j0..] = A[r][j0..] Ld^-T, one lane per row.  Eight columns at a time live
// in registers; the columns already solved are read back from LDS (column-major: conflict-free), the block's factor as LDS broadcasts
// (stored transposed, so the eight factors of one step are contiguous), the reciprocal pivots on its diagonal.
__global__ __launch_bounds__(256) void k_chol_trsm(double *A, int ld, int n, int j0, const double *rdg) {
    __shared__ double sLt[kNB * kNB], sX[kNB * 64];          // sLt[k][b] = L[b][k]
    const int tid = threadIdx.x, lane = tid & 63, w = min(kNB, n - j0), t0 = j0 + w;
    for (int k = tid >> 6; k < kNB; k += 4) {                 // lanes over b: conflict-free LDS rows (the 64 x 64 block is re-read from L1 / L2)
        const int b = lane;
        sLt[k * kNB + b] = (b < w && k < b) ? A[(size_t)(j0 + b) * ld + j0 + k] : (k == b) ? (b < w ? rdg[j0 + b] : 1.0) : 0.0;
    }
    const int r0 = t0 + blockIdx.x * 64;
    // the 64 rows of this workgroup, coalesced; element (row rr, column c) sits at sX[c][rr ^ c]: the fill (lanes over c) and the solve
    // (lanes over rr) are both conflict-free
    for (int idx = tid; idx < 64 * kNB; idx += 256) {
        const int rr = idx / kNB, c = idx - rr * kNB;
        sX[c * 64 + (rr ^ c)] = (r0 + rr <= n && c < w) ? A[(size_t)(r0 + rr) * ld + j0 + c] : 0.0;
    }
    __syncthreads();
    if (tid < 64)
    for (int sp = 0; sp < kNB / 8; sp++) {
        const int c0 = sp * 8;
        double x[8];
#pragma unroll
        for (int b = 0; b < 8; b++) x[b] = sX[(c0 + b) * 64 + (lane ^ (c0 + b))];
#pragma unroll 4
        for (int k = 0; k < c0; k++) {
            const double xk = sX[k * 64 + (lane ^ k)];
            const double *l = sLt + k * kNB + c0;
#pragma unroll
            for (int b = 0; b < 8; b++) x[b] -= xk * l[b];
        }
#pragma unroll
        for (int b = 0; b < 8; b++) {
            double t = x[b];
#pragma unroll
            for (int k = 0; k < b; k++) t -= x[k] * sLt[(c0 + k) * kNB + c0 + b];
            x[b] = t * sLt[(c0 + b) * kNB + c0 + b];
        }
#pragma unroll
        for (int b = 0; b < 8; b++) sX[(c0 + b) * 64 + (lane ^ (c0 + b))] = x[b];
    }
    __syncthreads();
    for (int idx = tid; idx < 64 * kNB; idx += 256) {
        const int rr = idx / kNB, c = idx - rr * kNB;
        if (r0 + rr <= n && c < w) A[(size_t)(r0 + rr) * ld + j0 + c] = sX[c * 64 + (rr ^ c)];
    }
}

// trailing update A[i][k] -= sum_q L[i][j0 + q] L[k][j0 + q] for t0 <= k <= i <= n, k < n: one 64 x 64 tile per workgroup, 4 x 4 per thread
__global__ __launch_bounds__(256) void k_chol_syrk(double *A, int ld, int n, int j0) {
    const int w = min(kNB, n - j0), t0 = j0 + w;
    const int ti = blockIdx.y, tk = blockIdx.x;
    if (tk > ti) return;
    const int i0 = t0 + ti * 64, k0 = t0 + tk * 64;
    if (k0 >= n) return;
    __shared__ double sI[64][33], sK[64][33];
    const int tid = threadIdx.x, ty = tid >> 4, tx = tid & 15;
    double acc[4][4];
#pragma unroll
    for (int a = 0; a < 4; a++)
#pragma unroll
        for (int b = 0; b < 4; b++) acc[a][b] = 0;
    for (int q0 = 0; q0 < w; q0 += 32) {
        for (int idx = tid; idx < 64 * 32; idx += 256) {
            const int r = idx >> 5, q = idx & 31;
            const bool qv = q0 + q < w;
            sI[r][q] = (qv && i0 + r <= n) ? A[(size_t)(i0 + r) * ld + j0 + q0 + q] : 0.0;
            sK[r][q] = (qv && k0 + r < n) ? A[(size_t)(k0 + r) * ld + j0 + q0 + q] : 0.0;
        }
        __syncthreads();
#pragma unroll 8
        for (int q = 0; q < 32; q++) {
            double li[4], lk[4];
#pragma unroll
            for (int a = 0; a < 4; a++) { li[a] = sI[ty + 16 * a][q]; lk[a] = sK[tx + 16 * a][q]; }
#pragma unroll
            for (int a = 0; a < 4; a++)
#pragma unroll
                for (int b = 0; b < 4; b++) acc[a][b] += li[a] * lk[b];
        }
        __syncthreads();
    }
#pragma unroll
    for (int a = 0; a < 4; a++)
#pragma unroll
        for (int b = 0; b < 4; b++) {
            const int i = i0 + ty + 16 * a, k = k0 + tx + 16 * b;
            if (i <= n && k < n && k <= i) A[(size_t)i * ld + k] -= acc[a][b];
        }
}

// L^T x = y (y = the factor's row n), blocks of 64 from the back: wave 0 solves the block, all threads update the unknowns before it
__global__ __launch_bounds__(1024) void k_chol_backsub(const double *A, int ld, int n, const double *rdg, double *x, const double *scal) {
    extern __shared__ double ys[];
    __shared__ double sD[kNB * kNB];
    const int tid = threadIdx.x;
    if (scal[3] == 0.0) {                               // not positive definite: g2o's solve() fails, the LM step is rejected
        for (int i = tid; i < n; i += 1024) x[i] = 0;
        return;
    }
    for (int i = tid; i < n; i += 1024) ys[i] = A[(size_t)n * ld + i];
    __syncthreads();
    for (int jb = (n + kNB - 1) / kNB - 1; jb >= 0; jb--) {
        const int j0 = jb * kNB, w = min(kNB, n - j0);
        for (int idx = tid; idx < kNB * kNB; idx += 1024) {   // the diagonal block, coalesced, for the sequential solve below
            const int r = idx / kNB, c = idx - r * kNB;
            sD[idx] = (r < w && c < r) ? A[(size_t)(j0 + r) * ld + j0 + c] : 0.0;
        }
        __syncthreads();
        if (tid < 64) {                                       // lane t carries unknown j0 + t; the solved one is broadcast by readlane
            double y = tid < w ? ys[j0 + tid] : 0.0;
            const double rd = tid < w ? rdg[j0 + tid] : 0.0;
            for (int jj = w - 1; jj >= 0; jj--) {
                const double l = sD[jj * kNB + tid];          // row jj of the block (zero from the diagonal on)
                const double xj = readlane_f64(y, jj) * readlane_f64(rd, jj);
                y = tid == jj ? xj : y - l * xj;
            }
            if (tid < w) ys[j0 + tid] = y;
        }
        __syncthreads();
        for (int i = tid; i < j0; i += 1024) {
            double acc0 = 0, acc1 = 0;
            const double *col = A + (size_t)j0 * ld + i;
            int q = 0;
#pragma unroll 1
            for (; q + 16 <= w; q += 16) {
                double v[16];
#pragma unroll
                for (int u = 0; u < 16; u++) v[u] = col[(size_t)(q + u) * ld];
#pragma unroll
                for (int u = 0; u < 16; u += 2) { acc0 += v[u] * ys[j0 + q + u]; acc1 += v[u + 1] * ys[j0 + q + u + 1]; }
            }
            for (; q < w; q++) acc0 += col[(size_t)q * ld] * ys[j0 + q];
            ys[i] -= acc0 + acc1;
        }
        __syncthreads();
    }
    for (int i = tid; i < n; i += 1024) x[i] = ys[i];
}
