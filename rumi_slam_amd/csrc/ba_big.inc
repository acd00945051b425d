// ba_big.inc -- launched by ba_solve_big (ba_single_host.inc); the Cholesky kernels are in chol_blocked.inc.  Included by opt.hip inside namespace rumi, after ba_single.inc.
// Reduced system of a LARGE window (more than 42 optimised key-frames: global bundle adjustment after a loop closure or a map merge,
// Optimizer.cc:48-351).  The dense panel Y of the small-window path would be 3 P x 6 K; here the Schur complement is accumulated block-sparsely
// (a landmark seen by k key-frames touches k (k + 1) / 2 blocks of 6 x 6) into the dense lower triangle of the augmented matrix
// [H_pp + lambda I - sum W W^T ; (b_p - sum W z)^T], which a multi-workgroup blocked Cholesky (panel 64) then factors in place: per panel
// one wave factors the diagonal block in registers (row per lane, pivots and columns by v_readlane), one lane per row solves the rows
// below, and 64 x 64 tiles take the trailing update; the right-hand side rides along as the extra row, a blocked backward substitution
// finishes.  No host round trip inside a trial.
__global__ void k_big_init(BADev B, double lambda, double *A, int ld) {
    const int n = B.n;
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (size_t)(n + 1) * n) return;
    const int i = (int)(idx / n), j = (int)(idx - (size_t)i * n);
    double v = 0;
    if (i == n) v = B.bp[j];
    else if (i / 6 == j / 6) { v = B.Hpp[(size_t)(i / 6) * 36 + (i % 6) * 6 + (j % 6)]; if (i == j) v += lambda; }
    A[(size_t)i * ld + j] = v;
    if (idx == 0) B.scal[3] = 1.0;
}

// W_e = H_pl(e) L_p (6 x 3), L_p L_p^T = (H_ll + lambda I)^-1
__global__ void k_big_w(BADev B, const double *Lp, double *W, int32_t *colOf) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= B.nE) return;
    const int col = B.poseCol[B.eKF[e]];
    colOf[e] = col;
    if (col < 0) return;
    const double *L = Lp + (size_t)B.eMP[e] * 6, *h = B.Hpl + (size_t)e * 18;
    const double l00 = L[0], l10 = L[1], l20 = L[2], l11 = L[3], l21 = L[4], l22 = L[5];
    double *w = W + (size_t)e * 18;
#pragma unroll
    for (int a = 0; a < 6; a++) {
        const double h0 = h[a * 3], h1 = h[a * 3 + 1], h2 = h[a * 3 + 2];
        w[a * 3] = h0 * l00 + h1 * l10 + h2 * l20; w[a * 3 + 1] = h1 * l11 + h2 * l21; w[a * 3 + 2] = h2 * l22;
    }
}

// One wave per non-empty 6 x 6 block (ca, cb <= ca) of the Schur complement: the host groups the observation pairs (a, b) of all landmarks by
// block once per call (the structure is the same for every trial), lane (r, c) accumulates sum_pairs W_a[r] . W_b[c] in a register and
// subtracts it from the matrix with a plain store; lanes 36..41 of the diagonal blocks do the same for W_a z.  No atomics: device-scope f64
// atomics are served past the per-XCD L2s (the per-landmark atomic formulation measured 0.69 ms at 130 key-frames, LDS f64 atomics on a
// row strip per key-frame 0.9 - 1.6 ms, this one 0.05 ms).
constexpr int kSchurSeg = 32;   // pairs per wave: long blocks (the diagonal ones: every observation of the key-frame) are cut into segments
__global__ __launch_bounds__(256) void k_big_schur(BADev B, const int32_t *blk, int nb, const int32_t *pairs, const double *W, const double *z, double *A, int ld) {
    const int wv = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (wv >= nb) return;
    const int ca = blk[4 * wv], cbm = blk[4 * wv + 1], s = blk[4 * wv + 2], len = blk[4 * wv + 3] - s;
    const int cb = cbm & 0x3fffffff;
    const bool multi = (cbm >> 30) != 0;                  // the block has more segments: combine with atomics
    // the segment's pairs, one per lane (coalesced), broadcast below: no dependent index loads inside the loop
    int myA = 0, myB = 0;
    if (lane < len) { myA = pairs[2 * (size_t)(s + lane)]; myB = pairs[2 * (size_t)(s + lane) + 1]; }
    const bool ent = lane < 36, rhs = lane >= 36 && lane < 42 && ca == cb;
    const int r = ent ? lane / 6 : rhs ? lane - 36 : 0, c = ent ? lane - (lane / 6) * 6 : 0;
    double acc = 0;
#pragma unroll 1
    for (int t = 0; t < len; t++) {
        const int ea = __builtin_amdgcn_readlane(myA, t), eb = __builtin_amdgcn_readlane(myB, t);
        const double *wa = W + (size_t)ea * 18 + r * 3, *wb = W + (size_t)eb * 18 + c * 3;
        acc += wa[0] * wb[0] + wa[1] * wb[1] + wa[2] * wb[2];
    }
    if (rhs) {                                            // diagonal block: pairs are (a, a); - W_a z on lanes 36..41
        acc = 0;
        for (int t = 0; t < len; t++) {
            const int ea = __builtin_amdgcn_readlane(myA, t);
            const double *wa = W + (size_t)ea * 18 + r * 3, *zp = z + 3 * (size_t)B.eMP[ea];
            acc += wa[0] * zp[0] + wa[1] * zp[1] + wa[2] * zp[2];
        }
    }
    if (!ent && !rhs) return;
    double *dst = ent ? &A[(size_t)(6 * ca + r) * ld + 6 * cb + c] : &A[(size_t)B.n * ld + 6 * ca + r];
    if (multi) atomicAdd(dst, -acc); else *dst -= acc;
}
