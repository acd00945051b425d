// ba_windows.inc -- included by opt.hip inside namespace rumi, after the single-window bundle-adjustment kernels it shares helpers with.
//
// ==================================================================================================================
// Local bundle adjustment with the WINDOW as a batch dimension (round 4).
//
// Optimizer::LocalBundleAdjustment (R/lib_src/Optimizer.cc:1003-1355) on g2o's BlockSolver<6,3> + Levenberg (G/core/block_solver.hpp:353-486,
// G/core/optimization_algorithm_levenberg.cpp:61-169), for windows whose reduced pose system fits the tile solver (up to 29 optimised
// key-frames).  W independent windows (LocalMapping.cc:149 calls one; the rumination merge, CloudMerging.cc:1677, has several sub-maps) share
// every launch: blockIdx.y = window, a device-side table of BAWin descriptors says where each window's arrays live, every window carries its
// own Levenberg-Marquardt control block and a window that has finished makes its workgroups return at once.
//
// One LM trial ("slot") is FOUR launches for all windows together (nine per window before):
//   k_baw_system   head: every workgroup takes the accept / reject decision of the previous trial from that trial's partial sums (same inputs,
//                  same instruction stream: same bits in every workgroup; workgroup 0 records it and tells the host).  Body: a workgroup owns
//                  a slice of the window's LANDMARKS with all their observations; 16 lanes per landmark linearise its edges, sum H_ll and b_l
//                  over the landmark (butterfly inside the 16 lanes: fixed order), invert and factor (H_ll + lambda I)^-1 = L L^T, and put the rows
//                  of Y = H_pl L (3 per landmark, and z = L^T b_l in column n) into LDS -- the dense panel never exists in memory -- where the
//                  f64 matrix cores contract it: G_slice = Y^T Y, upper tiles, one accumulator set per wave.  H_pl per edge and the
//                  sqrt(w)-scaled pose rows [J | r] go to memory for the two kernels below.
//   k_baw_reduce   G = sum of the slices' partial Gram matrices in slice order (one thread per entry), and, in other workgroups of the same
//                  launch, H_pp / b_p per key-frame as a Gram product of its pose rows on the matrix cores (8 rows per v_mfma_f64_16x16x4_f64:
//                  two 8-column row groups side by side, both diagonal blocks of the result are the key-frame's).
//   k_baw_solve    the tile Cholesky of k_ba_solve_tiles on  H_pp + lambda I - G  (one workgroup per window).
//   k_baw_updchi   landmark back-substitution, oplus into the trial state and the trial's robust chi2 in one pass (a workgroup computes the new
//                  poses into LDS itself), partial sums per workgroup.
// NOTHING is accumulated with floating-point atomics: every sum has a fixed order (lane butterflies, wave order, slice order), so a window's
// result -- and with it every accept / reject decision -- is bit-reproducible from run to run and independent of what else is in the batch.
// ==================================================================================================================

struct LmCtl {                           // one of two copies per window: slot s reads copy s & 1 and writes copy (s + 1) & 1
    double lambda, ni, currentChi, iniChi;
    int32_t cur, done, nBad, qmax, it, trials, iters, phase;    // phase 0: before computeLambdaInit, 1: trials running
};
struct WinMirror {                       // fine-grained pinned host memory, written by workgroup 0 of k_baw_system
    volatile int32_t cur, iters, trials, pad;
    volatile unsigned long long word;    // run << 32 | (slot + 1) << 1 | done, stored last (release): slots of an EARLIER run that are still queued
};                                       // report too (they exit at once), the host only trusts words that carry its run number
struct BAWin {
    int32_t nKF, nMP, nE, nOpt, n, NP, NT, nT, nSlices, lmPerSlice, nUpd, robust, maxIt, useLast, cur0;
    double delta, dsqr;
    DCam cam;
    // per-edge arrays are in LANDMARK order (position s of the landmark lists, ptStart): a landmark's lanes read consecutive memory.  They are
    // built on the device (k_baws_*) from the caller's arrays as they came: raw*
    int32_t *sMP, *sKF, *sEdge, *rowSlot, *ptStart, *kfRowStart;      // sEdge[s] = the caller's edge index
    float *obs, *info;
    uint8_t *off;
    const int32_t *poseCol, *rawMP, *rawKF;
    const float *rawObs, *rawInfo, *rawX;
    const double *rawT;
    int32_t *cursor, *tmpEdge, *blkCnt, *err;            // scratch of the structure kernels; err: bit 0 index out of range, bit 1 a landmark observed twice by a key-frame
    uint8_t *rank8;
    int32_t nBlk;
    double *T[2], *X[2];
    double *panel, *Dinv, *bl, *Hpp, *bp, *x, *lastChi2, *Gpart, *G, *chiPart, *sclPart, *solveOk;
    unsigned long long *maxDiag;
    LmCtl *lm;
    WinMirror *mirror;
    const volatile int32_t *stopWord;    // the reference's pbStopFlag, forwarded by the host into pinned memory
    int32_t *stopSeen;                   // ... sampled ONCE per slot (k_baw_updchi), so that every workgroup of the next head sees the same value
    double *outT, *outX;                 // results gathered for one copy back
    uint8_t *erase;
    int32_t *errOut;
};

constexpr int kBawMaxSlices = 192, kBawMaxWindows = 32;
constexpr int kBawLm = 16;               // landmarks per chunk (16 lanes each)
constexpr int kBawRows = 3 * kBawLm;     // rows of Y per chunk
constexpr int kBawTileStride = kBawRows * 16;

// sum of cnt doubles in a fixed order, the same bits in every thread of the 256-thread workgroup
__device__ __forceinline__ double baw_fixed_sum(const double *p, int cnt, double *red) {
    double v[1] = {0};
    for (int i = threadIdx.x; i < cnt; i += 256) v[0] += p[i];
    block_sum<1>(v, red);
    return v[0];
}

// The head of a slot: the state of the LM loop after the previous slot.  levenberg.cpp:102-166 as ba_run's host loop has it.
__device__ __forceinline__ LmCtl baw_head(const BAWin &W, int slot, double *red) {
    if (slot == 0) { LmCtl c0{}; c0.cur = W.cur0; c0.ni = 2; c0.lambda = -1; return c0; }      // a run starts from the table alone: nothing to upload
    LmCtl c = W.lm[slot & 1];
    if (c.done) return c;
    if (c.phase == 0) {                                   // after the init slot: chi2 of the estimate, computeLambdaInit = tau * max |H_jj|
        const double chi = baw_fixed_sum(W.chiPart, W.nSlices, red);
        c.currentChi = chi; c.iniChi = chi;
        c.lambda = 1e-5 * __longlong_as_double((long long)*W.maxDiag); c.ni = 2; c.nBad = 0; c.qmax = 0;
        c.phase = 1;
        return c;
    }
    double v2[2] = {0, 0};
    for (int i = threadIdx.x; i < W.nUpd; i += 256) { v2[0] += W.chiPart[i]; v2[1] += W.sclPart[i]; }
    block_sum<2>(v2, red);
    const double tempChi0 = v2[0], scale = v2[1];
    const bool ok2 = *W.solveOk != 0.0;
    const double tempChi = ok2 ? tempChi0 : DBL_MAX;
    double rho = c.currentChi - tempChi;
    rho /= scale + 1e-3;
    if (rho > 0 && isfinite(tempChi)) {
        const double tr = 2 * rho - 1;
        double alpha = 1. - tr * tr * tr;
        alpha = fmin(alpha, 2. / 3.);
        c.lambda *= fmax(1. / 3., alpha);
        c.ni = 2;
        c.currentChi = tempChi;
        c.cur ^= 1;                                       // discardTop(): the trial state becomes the estimate
    } else {
        c.lambda *= c.ni;
        c.ni *= 2;                                        // pop(): keep the current state
    }
    c.qmax++; c.trials++;
    const bool stop = *W.stopSeen != 0;
    if (!(rho < 0 && c.qmax < 10 && !stop)) {
        c.iters++;
        bool term = c.qmax == 10 || rho == 0;
        if (!term) {
            if ((c.iniChi - c.currentChi) * 1e3 < c.iniChi) c.nBad++; else c.nBad = 0;
            term = c.nBad >= 3;
        }
        c.it++;
        if (term || c.it >= W.maxIt || stop) c.done = 1;
        else { c.qmax = 0; c.iniChi = c.currentChi; }
    }
    return c;
}

struct BawEdge { double A0[3], A1[3], J0[6], J1[6], e0, e1, w, chi, rho; };
struct BawRaw { int kf, rowSlot; float ox, oy, info; int off; };                 // what an edge reads from memory (position s of the landmark order)

__device__ __forceinline__ BawRaw baw_raw(const BAWin &W, int s) {
    const float2 o = reinterpret_cast<const float2 *>(W.obs)[s];
    return BawRaw{W.sKF[s], W.rowSlot[s], o.x, o.y, W.info[s], (int)W.off[s]};
}

// residual, Huber weight and the two Jacobians of one observation (k_ba_build's arithmetic; OptimizableTypes.cpp:135-156)
__device__ __forceinline__ void baw_edge(const BAWin &W, const double *sPose, const BawRaw &r, const D3 &Xp, BawEdge &t) {
    const double *pp = sPose + r.kf * 8;
    const DSE3 P{{pp[0], pp[1], pp[2], pp[3]}, {pp[4], pp[5], pp[6]}};
    const D3 pc = se3_map(P, Xp);
    double u, v;
    cam_project(W.cam, pc, u, v);
    t.e0 = (double)r.ox - u; t.e1 = (double)r.oy - v;
    const double info = (double)r.info;
    t.chi = t.e0 * info * t.e0 + t.e1 * info * t.e1;
    double r0 = t.chi, r1 = 1;
    if (W.robust) huber(t.chi, W.delta, W.dsqr, r0, r1);
    t.rho = r0;
    t.w = r1 * info;
    double R[3][3];
    jac_pose(W.cam, pc, t.J0, t.J1);
    quat_to_matrix(P.r, R);
    const double iz = m_rcp(pc.z), iz2 = iz * iz;
    const double j00 = W.cam.fx * iz, j02 = -W.cam.fx * pc.x * iz2, j11 = W.cam.fy * iz, j12 = -W.cam.fy * pc.y * iz2;
#pragma unroll
    for (int k = 0; k < 3; k++) { t.A0[k] = -(j00 * R[0][k] + j02 * R[2][k]); t.A1[k] = -(j11 * R[1][k] + j12 * R[2][k]); }   // -projectJac * R
}

// (H_ll + lambda I)^-1 by cofactors (Eigen Matrix3d::inverse, block_solver.hpp:389) and its Cholesky factor, with the hardware reciprocal /
// reciprocal square root refined to double precision (opt_math.h: m_rcp, m_rsqrt) instead of the IEEE divide and square-root sequences
__device__ __forceinline__ void baw_dinv_factor(const double (&h)[6] /* 00 01 02 11 12 22 */, double lambda, double (&I)[9], double (&L)[6]) {
    const double d0 = h[0] + lambda, d4 = h[3] + lambda, d8 = h[5] + lambda, d1 = h[1], d2 = h[2], d5 = h[4];
    const double c00 = d4 * d8 - d5 * d5, c01 = d5 * d2 - d1 * d8, c02 = d1 * d5 - d4 * d2;
    const double id = m_rcp(d0 * c00 + d1 * c01 + d2 * c02);
    I[0] = c00 * id; I[1] = (d2 * d5 - d1 * d8) * id; I[2] = (d1 * d5 - d2 * d4) * id;
    I[3] = c01 * id; I[4] = (d0 * d8 - d2 * d2) * id; I[5] = (d2 * d1 - d0 * d5) * id;
    I[6] = c02 * id; I[7] = (d1 * d2 - d0 * d5) * id; I[8] = (d0 * d4 - d1 * d1) * id;
    const double r00 = m_rsqrt(I[0]), l00 = I[0] * r00, l10 = I[3] * r00, l20 = I[6] * r00;
    const double t11 = I[4] - l10 * l10, r11 = m_rsqrt(t11), l11 = t11 * r11, l21 = (I[7] - l20 * l10) * r11;
    const double t22 = I[8] - l20 * l20 - l21 * l21, l22 = t22 * m_rsqrt(t22);
    L[0] = l00; L[1] = l10; L[2] = l20; L[3] = l11; L[4] = l21; L[5] = l22;
}

// MAXSLOTS = upper tiles a wave accumulates (tile t of the lower-triangle enumeration I (I + 1) / 2 + J goes to wave t & 3, slot t >> 2), a template
// parameter so that the matrix-core loop is straight-line code: 2 / 4 / 6 / 9 / 12 / 17 slots cover 2 / 5 / 6 / 8 / 9 / 11 tile rows (the host
// takes the smallest that holds the largest window of the batch; 9 = 20 optimised key-frames).
#ifdef RUMI_BAW_STAMP
#define BAW_STAMP_DECL long long stT = clock64(), stA[14] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}
#define BAW_STAMP(i) do { const long long now_ = clock64(); stA[i] += now_ - stT; stT = now_; } while (0)
#else
#define BAW_STAMP_DECL
#define BAW_STAMP(i)
#endif
template <int MAXSLOTS>
__global__ __launch_bounds__(256, 2) void k_baw_system(const BAWin *__restrict__ wins, int slot, unsigned run) {
    extern __shared__ double sh[];                        // Y chunk [NT][48][16] | contributions [9][256] | sums [16][9] | factors [16][6] | poses [nKF][8] | column blocks [nKF]
    __shared__ double red[8];
    const BAWin &W = wins[blockIdx.y];
    if ((int)blockIdx.x >= W.nSlices) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    BAW_STAMP_DECL;
    const LmCtl c = baw_head(W, slot, red);
    BAW_STAMP(0);
    if (blockIdx.x == 0 && tid == 0) {
        W.lm[(slot + 1) & 1] = c;
        W.stopSeen[1] = c.cur;
        WinMirror *m = W.mirror;
        m->cur = c.cur; m->iters = c.iters; m->trials = c.trials;
        __threadfence_system();
        __hip_atomic_store(const_cast<unsigned long long *>(&m->word), ((unsigned long long)run << 32) | ((unsigned long long)(slot + 1) << 1) | (unsigned)c.done,
                           __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
    if (c.done) return;
    const bool init = slot == 0;
    const int NT = W.NT, n = W.n, nKF = W.nKF;
    double *Ych = sh, *sBuf9 = sh + (size_t)NT * kBawTileStride, *sSum = sBuf9 + 9 * 256, *sL = sSum + kBawLm * 9, *sXb = sL + kBawLm * 6, *sPose = sXb + 2 * kBawRows;
    int *sCol = reinterpret_cast<int *>(sPose + (size_t)nKF * 8);
    const double *Tcur = W.T[c.cur], *Xcur = W.X[c.cur];
    const int lm0 = blockIdx.x * W.lmPerSlice, lm1 = min(W.nMP, lm0 + W.lmPerSlice);
    const int g = tid >> 4, l16 = tid & 15;
    // What a chunk reads from memory is FETCHED ONE CHUNK AHEAD (a chunk is a chain of dependent round trips otherwise: list bounds -> edge
    // records -> landmark positions, with two waves a SIMD to hide them): the first 256 edge records of the next chunk (it starts where this one
    // ends), its list bounds and its 16 landmark positions are requested before the matrix-core loop of the current chunk and used after it;
    // the positions wait in LDS (two buffers), the edge records in registers, where they also serve the second pass (no re-read).
    int cKf = 0, cRow = -1, cOff = 1, cPe = 0, cS0 = 0, cS1 = 0, cSE = 0;        // the current chunk's: first-round edge record, list bounds
    float cOx = 0, cOy = 0, cInfo = 0;
    double cX = 0;
#define RUMI_BAW_PREFETCH(c0n, sBn)                                                                                                 \
    do {                                                                                                                            \
        const int nln = min(kBawLm, lm1 - (c0n)), pn = (c0n) + g;                                                                   \
        const bool vn = g < nln;                                                                                                    \
        cS0 = vn ? W.ptStart[pn] : 0; cS1 = vn ? W.ptStart[pn + 1] : 0;                                                             \
        cSE = W.ptStart[(c0n) + nln];                                                                                               \
        const int sn = (sBn) + tid;                                                                                                 \
        if (sn < W.nE) {                                                                                                            \
            const BawRaw rr = baw_raw(W, sn);                                                                                       \
            cKf = rr.kf; cRow = rr.rowSlot; cOx = rr.ox; cOy = rr.oy; cInfo = rr.info; cOff = rr.off; cPe = W.sMP[sn];              \
        }                                                                                                                           \
        cX = tid < 3 * nln ? Xcur[3 * (c0n) + tid] : 0.0;                                                                           \
    } while (0)
    int sB = W.ptStart[lm0];
    RUMI_BAW_PREFETCH(lm0, sB);
    for (int i = tid; i < nKF * 8; i += 256) sPose[i] = Tcur[i];
    for (int i = tid; i < nKF; i += 256) sCol[i] = W.poseCol[i];
    // this wave's tiles
    int trj[MAXSLOTS], tcj[MAXSLOTS], mySlots = 0;
#pragma unroll
    for (int j = 0; j < MAXSLOTS; j++) {
        const int t = wave + 4 * j;                       // (uniform: scalar arithmetic)
        int I = 0;
        while ((I + 1) * (I + 2) / 2 <= t) I++;
        trj[j] = t - I * (I + 1) / 2; tcj[j] = I;
        if (t < W.nT) mySlots = j + 1; else { trj[j] = 0; tcj[j] = 0; }      // a surplus slot works on tile (0, 0) and is not stored: no branch in the loop
    }
    v4f64 acc[MAXSLOTS];
#pragma unroll
    for (int j = 0; j < MAXSLOTS; j++) acc[j] = v4f64{0, 0, 0, 0};
    double chiAcc[1] = {0};
    double dmax = 0;
    if (tid < kBawRows) sXb[tid] = cX;
    __syncthreads();                                      // poses and the first chunk's landmarks staged
    BAW_STAMP(1);
    // A chunk = 16 consecutive landmarks = one contiguous range of edges (landmark order).  Edges are dealt DENSELY over the lanes (a landmark has 2
    // to ~30 edges: one lane per (landmark, edge slot) left half the lanes idle); a landmark's sums are then taken over its run of the
    // contribution buffer by 9 lanes of its group, in run order.
    // the first round's linearisation stays in registers for the second pass where the accumulators leave room (up to 12 tiles a wave: 42 registers)
    constexpr bool kKeep = MAXSLOTS <= 12;
    BawEdge keep{};
    int xb = 0;
    for (int c0 = lm0; c0 < lm1; c0 += kBawLm) {
        const int nl = min(kBawLm, lm1 - c0);
        const int p = c0 + g;
        const bool valid = g < nl;
        const int s0 = cS0, s1 = cS1, sE = cSE;                                   // (sB, sE: uniform)
        const double *Xc = sXb + xb * kBawRows - 3 * c0;                          // landmark pe of the chunk at Xc[3 pe]
        if (!init) for (int i = tid; i < NT * kBawTileStride; i += 256) Ych[i] = 0.0;
        double sum9[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};      // (H_ll upper 00 01 02 11 12 22 | b_l) of landmark g: this lane's share (edges l16, l16 + 16, ... of its list)
        for (int rb = sB; rb < sE; rb += 256) {           // rounds of 256 edges (one, unless the chunk's landmarks average more than 16 edges)
            const int s = rb + tid;
            double cb[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
            if (s < sE) {
                BawRaw r{cKf, cRow, cOx, cOy, cInfo, cOff};
                int pe = cPe;
                if (rb != sB) { r = baw_raw(W, s); pe = W.sMP[s]; }
                if (!r.off) {
                    BawEdge t;
                    baw_edge(W, sPose, r, D3{Xc[3 * pe], Xc[3 * pe + 1], Xc[3 * pe + 2]}, t);
                    if (kKeep && rb == sB) keep = t;
                    int q = 0;
#pragma unroll
                    for (int a = 0; a < 3; a++) {
                        cb[6 + a] = -t.w * (t.A0[a] * t.e0 + t.A1[a] * t.e1);
#pragma unroll
                        for (int c2 = a; c2 < 3; c2++) cb[q++] = t.w * (t.A0[a] * t.A0[c2] + t.A1[a] * t.A1[c2]);
                    }
                    if (init) { chiAcc[0] += t.rho; W.lastChi2[s] = t.chi; }
                }
            }
            BAW_STAMP(10);
            if (rb > sB) __syncthreads();                 // the previous round's buffer has been summed
#pragma unroll
            for (int q = 0; q < 9; q++) sBuf9[q * 256 + tid] = cb[q];
            __syncthreads();
            BAW_STAMP(11);
            {                                             // every lane of the group: the nine contributions of its edges (nine reads in flight)
                const int hi = min(s1, rb + 256);
                for (int e = max(s0, rb) + l16; e < hi; e += 16) {
#pragma unroll
                    for (int q = 0; q < 9; q++) sum9[q] += sBuf9[q * 256 + e - rb];
                }
            }
        }
        BAW_STAMP(2);
        // the sums over the group's 16 lanes by rotate-and-add (DPP): every step adds two values that are each other's mirror, so all 16 lanes end
        // with the same bits and no broadcast is needed
        double hl[6], blv[3], I9[9], L[6];
#pragma unroll
        for (int q = 0; q < 6; q++) hl[q] = row_allreduce(sum9[q]);
#pragma unroll
        for (int a = 0; a < 3; a++) blv[a] = row_allreduce(sum9[6 + a]);
        if (init) {
            if (valid) dmax = fmax(dmax, fmax(fabs(hl[0]), fmax(fabs(hl[3]), fabs(hl[5]))));
        } else {
            baw_dinv_factor(hl, c.lambda, I9, L);
            if (valid && l16 == 0) {
#pragma unroll
                for (int i = 0; i < 9; i++) W.Dinv[(size_t)p * 9 + i] = I9[i];
                W.bl[3 * p] = blv[0]; W.bl[3 * p + 1] = blv[1]; W.bl[3 * p + 2] = blv[2];
#pragma unroll
                for (int i = 0; i < 6; i++) sL[g * 6 + i] = L[i];
            }
            if (valid && l16 == 0) {                      // z = L^T b_l rides in column n (the chunk was zeroed before the first barrier above)
                double *y = Ych + (n >> 4) * kBawTileStride + (3 * g) * 16 + (n & 15);
                y[0] = L[0] * blv[0] + L[1] * blv[1] + L[2] * blv[2]; y[16] = L[3] * blv[1] + L[4] * blv[2]; y[32] = L[5] * blv[2];
            }
        }
        BAW_STAMP(3);
        __syncthreads();                                  // the factors of the chunk's landmarks are in LDS
        BAW_STAMP(4);
        // second pass, dense again (re-linearised where the registers are needed for accumulators): the sqrt(w)-scaled pose rows [J | r] to
        // memory (k_baw_reduce contracts them per key-frame), the rows of Y = H_pl L into LDS
        for (int rb = sB; rb < sE; rb += 256) {
            const int s = rb + tid;
            if (s >= sE) continue;
            BawRaw r{cKf, cRow, cOx, cOy, cInfo, cOff};
            int pe = cPe;
            if (rb != sB) { r = baw_raw(W, s); pe = W.sMP[s]; }
            if (r.rowSlot < 0) continue;                  // fixed key-frame: no pose block
            typedef double d2 __attribute__((ext_vector_type(2)));
            d2 *rp2 = reinterpret_cast<d2 *>(W.panel + (size_t)r.rowSlot * 8);       // 16-byte stores (a row is 64 bytes)
            if (r.off) {
#pragma unroll
                for (int k = 0; k < 8; k++) rp2[k] = d2{0, 0};
                continue;
            }
            const int ge = pe - c0;
            BawEdge t;
            if (kKeep && rb == sB) t = keep;
            else baw_edge(W, sPose, r, D3{Xc[3 * pe], Xc[3 * pe + 1], Xc[3 * pe + 2]}, t);
            const double sw = m_sqrt(t.w);
            rp2[0] = d2{sw * t.J0[0], sw * t.J0[1]}; rp2[1] = d2{sw * t.J0[2], sw * t.J0[3]}; rp2[2] = d2{sw * t.J0[4], sw * t.J0[5]}; rp2[3] = d2{sw * t.e0, 0};
            rp2[4] = d2{sw * t.J1[0], sw * t.J1[1]}; rp2[5] = d2{sw * t.J1[2], sw * t.J1[3]}; rp2[6] = d2{sw * t.J1[4], sw * t.J1[5]}; rp2[7] = d2{sw * t.e1, 0};
            if (init) continue;
            const int col6 = sCol[r.kf] * 6;
            const double *Lg = sL + ge * 6;
            const double L0 = Lg[0], L1 = Lg[1], L2 = Lg[2], L3 = Lg[3], L4 = Lg[4], L5 = Lg[5];
            // H_pl L = w J^T (A L): the 2 x 3 product first
            const double a00 = t.w * (t.A0[0] * L0 + t.A0[1] * L1 + t.A0[2] * L2), a01 = t.w * (t.A0[1] * L3 + t.A0[2] * L4), a02 = t.w * (t.A0[2] * L5);
            const double a10 = t.w * (t.A1[0] * L0 + t.A1[1] * L1 + t.A1[2] * L2), a11 = t.w * (t.A1[1] * L3 + t.A1[2] * L4), a12 = t.w * (t.A1[2] * L5);
#pragma unroll
            for (int a = 0; a < 6; a++) {
                const int cc = col6 + a;
                double *y = Ych + (cc >> 4) * kBawTileStride + (3 * ge) * 16 + (cc & 15);
                y[0] = t.J0[a] * a00 + t.J1[a] * a10;
                y[16] = t.J0[a] * a01 + t.J1[a] * a11;
                y[32] = t.J0[a] * a02 + t.J1[a] * a12;
            }
        }
        // the next chunk's requests go out here and are met after the matrix-core loop
        const int c0n = c0 + kBawLm;
        const bool more = c0n < lm1;                      // (uniform)
        if (more) RUMI_BAW_PREFETCH(c0n, sE);             // (the c* variables now belong to the next chunk)
        BAW_STAMP(5);
        if (!init) {
            __syncthreads();
            BAW_STAMP(6);
            const int ksN = (3 * nl + 3) >> 2;
            for (int ks = 0; ks < ksN; ks++) {
                double pa[MAXSLOTS], pb[MAXSLOTS];
#pragma unroll
                for (int j = 0; j < MAXSLOTS; j++) { pa[j] = Ych[trj[j] * kBawTileStride + ks * 64 + lane]; pb[j] = Ych[tcj[j] * kBawTileStride + ks * 64 + lane]; }
#pragma unroll
                for (int j = 0; j < MAXSLOTS; j++) acc[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(pa[j], pb[j], acc[j], 0, 0, 0);
            }
            BAW_STAMP(7);
        }
        xb ^= 1;
        if (more && tid < kBawRows) sXb[xb * kBawRows + tid] = cX;
        __syncthreads();                                  // everyone is done with the chunk (its Y rows, its contribution buffer); the next one's landmarks are in LDS
        BAW_STAMP(8);
        sB = sE;
    }
#undef RUMI_BAW_PREFETCH
    if (init) {
        block_sum<1>(chiAcc, red);
        if (tid == 0) W.chiPart[blockIdx.x] = chiAcc[0];
        dmax = wave_allreduce_max(dmax);
        if (lane == 0) atomicMax(W.maxDiag, (unsigned long long)__double_as_longlong(dmax));       // >= 0: bit order = value order; a maximum has no order
        return;
    }
    double *gp = W.Gpart + (size_t)blockIdx.x * W.nT * 256;
#pragma unroll
    for (int j = 0; j < MAXSLOTS; j++) {
        if (j < mySlots) {
            double *o = gp + (size_t)(wave + 4 * j) * 256 + lane;
#pragma unroll
            for (int r = 0; r < 4; r++) o[64 * r] = acc[j][r];
        }
    }
#ifdef RUMI_BAW_STAMP
    BAW_STAMP(9);
    if (slot == 3 && blockIdx.y == 0 && (blockIdx.x == 1 || blockIdx.x == 5) && (tid & 63) == 0)
        printf("baw_system wg %d wave %d chunks %d: head %lld stage %lld pass1 (zero + linearise %lld, buffer + barrier %lld, run sums %lld) reduce+dinv %lld bar %lld pass2 %lld bar %lld mfma %lld bar %lld store %lld\n", blockIdx.x, tid >> 6,
               (lm1 - lm0 + kBawLm - 1) / kBawLm, stA[0], stA[1], stA[10], stA[11], stA[2], stA[3], stA[4], stA[5], stA[6], stA[7], stA[8], stA[9]);
#endif
}

// G = sum over the slices (fixed order), and H_pp / b_p per key-frame on the matrix cores.  grid (tileBlocks + kfBlocks, windows), 16 waves: both
// halves are chains of loads that only more waves shorten.
template <int NW> __device__ __forceinline__ double baw_tree(const double (*part)[256], int i) {      // the waves' values in a fixed, balanced order
    double q[NW / 2];
#pragma unroll
    for (int w = 0; w < NW / 2; w++) q[w] = part[2 * w][i] + part[2 * w + 1][i];
    if constexpr (NW == 4) return q[0] + q[1];
    else return ((q[0] + q[1]) + (q[2] + q[3])) + ((q[4] + q[5]) + (q[6] + q[7]));
}
// kRedWaves = 16 for launches with many slices per window (a single window: 188), 4 for batches (32 slices per window: more waves would idle)
template <int kRedWaves>
__global__ __launch_bounds__(kRedWaves * 64) void k_baw_reduce(const BAWin *__restrict__ wins, int slot, int tileBlocks) {
    __shared__ double part[kRedWaves][256];
    const BAWin &W = wins[blockIdx.y];
    if (W.lm[(slot + 1) & 1].done) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    if ((int)blockIdx.x < tileBlocks) {
        // four workgroups per tile (64 entries each); wave g sums the slices g, g + 16, ...
        const int t = blockIdx.x >> 2, ent = (blockIdx.x & 3) * 64 + lane;
        if (slot == 0 || t >= W.nT) return;
        const size_t stride = (size_t)W.nT * 256;
        const double *src = W.Gpart + (size_t)t * 256 + ent;
        const int S = W.nSlices;
        double v[kBawMaxSlices / kRedWaves];
#pragma unroll
        for (int u = 0; u < kBawMaxSlices / kRedWaves; u++) { const int k = wave + kRedWaves * u; v[u] = k < S ? src[(size_t)k * stride] : 0.0; }
        double s = 0;
#pragma unroll
        for (int u = 0; u < kBawMaxSlices / kRedWaves; u++) s += v[u];
        part[wave][lane] = s;
        __syncthreads();
        if (wave == 0) W.G[(size_t)t * 256 + ent] = baw_tree<kRedWaves>(part, lane);
        return;
    }
    const int kf = blockIdx.x - tileBlocks;
    if (kf >= W.nOpt) return;
    // rows [r0, r1) of the key-frame, 8 doubles each ([J0..J5, r, 0]); lane l of a step reads element l of 8 consecutive rows: row = 2 k + g with
    // k = l >> 4 the MFMA's K index and g = (l >> 3) & 1 the half of its 16 rows / columns the lane feeds, column a = l & 7.  Both operands are
    // that value, so D[(g, a)][(h, b)] = sum_k row(2 k + g)[a] row(2 k + h)[b]: the two diagonal blocks g = h are Gram products over the rows of
    // their parity, their sum is the key-frame's [H_pp | -b_p] (8 x 8), the off-diagonal blocks are not used.
    const int r0 = W.kfRowStart[kf], r1 = W.kfRowStart[kf + 1];
    const double *P = W.panel;
    v4f64 acc = {0, 0, 0, 0};
    constexpr int U = 8;
    for (int r = r0 + wave * 8; r < r1; r += kRedWaves * 8 * U) {
        double v[U];
#pragma unroll
        for (int u = 0; u < U; u++) {
            const int row = r + u * kRedWaves * 8 + (lane >> 3);
            v[u] = P[(size_t)min(row, r1 - 1) * 8 + (lane & 7)];
        }
#pragma unroll
        for (int u = 0; u < U; u++) {
            const int row = r + u * kRedWaves * 8 + (lane >> 3);
            const double x = row < r1 ? v[u] : 0.0;
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(x, x, acc, 0, 0, 0);
        }
    }
#pragma unroll
    for (int r = 0; r < 4; r++) part[wave][r * 64 + lane] = acc[r];
    __syncthreads();
    if (tid < 42) {                                       // (a, b): a < 6, b < 7
        const int a = tid / 7, b = tid - a * 7;
        const int i0 = (a >> 2) * 64 + (a & 3) * 16 + b, i1 = (2 + (a >> 2)) * 64 + (a & 3) * 16 + 8 + b;
        const double s = baw_tree<kRedWaves>(part, i0) + baw_tree<kRedWaves>(part, i1);
        if (b < 6) {
            W.Hpp[(size_t)kf * 36 + a * 6 + b] = s;
            if (slot == 0 && a == b) atomicMax(W.maxDiag, (unsigned long long)__double_as_longlong(fabs(s)));
        } else W.bp[(size_t)kf * 6 + a] = -s;
    }
}

// One workgroup per window: k_ba_solve_tiles' factorisation on H_pp + lambda I - G.
__global__ __launch_bounds__(kSolveThreads) void k_baw_solve(const BAWin *__restrict__ wins, int slot) {
    const BAWin &W = wins[blockIdx.x];
    const LmCtl &c = W.lm[(slot + 1) & 1];
    if (c.done) return;
    const SolveIO io{W.n, W.NP, W.Hpp, W.bp, W.x, W.solveOk, nullptr};
    solve_tiles_core<true>(io, c.lambda, W.G);
}

// Landmark back-substitution x_l = D^-1 (b_l - H_pl^T x_p) (block_solver.hpp:468-481), oplus of points and poses into the TRIAL state, the gain
// denominator x^T (lambda x + b) and the trial's robustified chi2 (sparse_optimizer.cpp:100-114), 8 lanes per landmark; partial sums per
// workgroup.  H_pl is not read from memory: an edge is linearised again at the estimate (H_pl^T x_p = w A^T (J x_p), ~250 instructions against
// 144 bytes written and read per edge and trial).  Every workgroup computes the window's new poses into LDS itself (a few dozen SE(3) products);
// workgroup 0 stores them.
__global__ __launch_bounds__(256) void k_baw_updchi(const BAWin *__restrict__ wins, int slot) {
    extern __shared__ double shu[];                       // estimate poses [nKF][8] | trial poses [nKF][8] | x_p [n] | column blocks [nKF]
    __shared__ double red[8];
    const BAWin &W = wins[blockIdx.y];
    if ((int)blockIdx.x >= W.nUpd) return;
    const LmCtl c = W.lm[(slot + 1) & 1];
    if (c.done) return;
    const int tid = threadIdx.x, nKF = W.nKF, n = W.n;
    double *sCur = shu, *sTrial = shu + (size_t)nKF * 8, *sX = sTrial + (size_t)nKF * 8;
    int *sCol = reinterpret_cast<int *>(sX + n);
    const double lambda = c.lambda;
    const double *T = W.T[c.cur], *X = W.X[c.cur];
    double *Tt = W.T[c.cur ^ 1], *Xt = W.X[c.cur ^ 1];
    double acc[2] = {0, 0};                               // chi2, scale
    for (int i = tid; i < n; i += 256) sX[i] = W.x[i];
    for (int k = tid; k < nKF; k += 256) {
        const int col = W.poseCol[k];
        sCol[k] = col;
        DSE3 P = load_pose(T, k);
        store_pose(sCur, k, P);
        if (col >= 0) {
            const double *xp = W.x + col * 6;
            double u[6];
            for (int a = 0; a < 6; a++) { u[a] = xp[a]; if (blockIdx.x == 0) acc[1] += xp[a] * (lambda * xp[a] + W.bp[col * 6 + a]); }
            P = se3_mul(se3_exp(u), P);
        }
        store_pose(sTrial, k, P);
        if (blockIdx.x == 0) store_pose(Tt, k, P);
    }
    if (blockIdx.x == 0 && tid == 0) *W.stopSeen = __hip_atomic_load(const_cast<const int32_t *>(W.stopWord), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    __syncthreads();
    const int p = (blockIdx.x * 256 + tid) / kLmLanes, sub = tid & (kLmLanes - 1);
    if (p < W.nMP) {
        const int s0 = W.ptStart[p], s1 = W.ptStart[p + 1];
        const D3 Xp{X[3 * p], X[3 * p + 1], X[3 * p + 2]};
        const double b0 = W.bl[3 * p], b1 = W.bl[3 * p + 1], b2 = W.bl[3 * p + 2];
        double I[9];
#pragma unroll
        for (int i = 0; i < 9; i++) I[i] = W.Dinv[(size_t)p * 9 + i];
        const bool has0 = s0 + sub < s1, has1 = s0 + sub + kLmLanes < s1;      // the lane's first two edges: read once, used by both loops
        const BawRaw off{0, -1, 0.f, 0.f, 0.f, true};
        const BawRaw raw0 = has0 ? baw_raw(W, s0 + sub) : off, raw1 = has1 ? baw_raw(W, s0 + sub + kLmLanes) : off;
        double c0 = 0, c1 = 0, c2 = 0;
        for (int s = s0 + sub; s < s1; s += kLmLanes) {
            const BawRaw r = s < s0 + kLmLanes ? raw0 : s < s0 + 2 * kLmLanes ? raw1 : baw_raw(W, s);
            const int col = sCol[r.kf];
            if (col < 0 || r.off) continue;
            BawEdge t;
            baw_edge(W, sCur, r, Xp, t);
            const double *xp = sX + col * 6;
            double d0 = 0, d1 = 0;
#pragma unroll
            for (int a = 0; a < 6; a++) { d0 += t.J0[a] * xp[a]; d1 += t.J1[a] * xp[a]; }
            c0 -= t.w * (t.A0[0] * d0 + t.A1[0] * d1); c1 -= t.w * (t.A0[1] * d0 + t.A1[1] * d1); c2 -= t.w * (t.A0[2] * d0 + t.A1[2] * d1);
        }
#pragma unroll
        for (int o = kLmLanes / 2; o > 0; o >>= 1) { c0 += __shfl_xor(c0, o, kLmLanes); c1 += __shfl_xor(c1, o, kLmLanes); c2 += __shfl_xor(c2, o, kLmLanes); }
        c0 += b0; c1 += b1; c2 += b2;
        const double x0 = I[0] * c0 + I[1] * c1 + I[2] * c2, x1 = I[3] * c0 + I[4] * c1 + I[5] * c2, x2 = I[6] * c0 + I[7] * c1 + I[8] * c2;
        const D3 Xn{Xp.x + x0, Xp.y + x1, Xp.z + x2};
        if (sub == 0) {
            Xt[3 * p] = Xn.x; Xt[3 * p + 1] = Xn.y; Xt[3 * p + 2] = Xn.z;
            acc[1] += x0 * (lambda * x0 + b0) + x1 * (lambda * x1 + b1) + x2 * (lambda * x2 + b2);
        }
        for (int s = s0 + sub; s < s1; s += kLmLanes) {
            const BawRaw r = s < s0 + kLmLanes ? raw0 : s < s0 + 2 * kLmLanes ? raw1 : baw_raw(W, s);
            if (r.off) continue;                          // level-1 edges keep the error of their last active pass
            const D3 pc = se3_map(load_pose(sTrial, r.kf), Xn);
            double u, v;
            cam_project(W.cam, pc, u, v);
            const double e0 = (double)r.ox - u, e1 = (double)r.oy - v, w = (double)r.info;
            const double ch = e0 * w * e0 + e1 * w * e1;
            W.lastChi2[s] = ch;
            double r0 = ch, r1 = 1;
            if (W.robust) huber(ch, W.delta, W.dsqr, r0, r1);
            acc[0] += r0;
        }
    }
    block_sum<2>(acc, red);
    if (tid == 0) { W.chiPart[blockIdx.x] = acc[0]; W.sclPart[blockIdx.x] = acc[1]; }
}

// ------------------------------------------------------------------------------------------------------------------
// g2o's buildStructure on the device (block_solver.hpp:142-295: which column block a key-frame is, which edges a landmark has, which rows a
// key-frame has), from the caller's arrays as they came.  The ORDER of everything is a function of the input alone -- inside a landmark by edge
// index, inside a key-frame by landmark order -- so the sums of the kernels above, which follow these orders, are reproducible.
//   k_baws_count    per edge: index check, landmark histogram (integer atomics: counts have no order)
//   k_baws_scan     per window: exclusive scan -> ptStart; initial landmark positions widened to double
//   k_baws_scatter  per edge: a place in its landmark's segment (atomic cursor: any order)
//   k_baws_order    16 lanes per landmark: the segment sorted by edge index (rank by comparison), the per-edge arrays gathered into that order;
//                   per chunk of 16 landmarks the number of edges of every key-frame (a presence bit per landmark) and the edge's rank among them
//   k_baws_kfscan   per window: key-frame row ranges and the chunks' offsets inside them
//   k_baws_rowslot  per edge: its two rows in the key-frame-ordered pose panel
// ------------------------------------------------------------------------------------------------------------------
__global__ void k_baws_zero(const BAWin *__restrict__ wins) {       // cursors, level-1 flags, the window's small words
    const BAWin &W = wins[blockIdx.y];
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i <= W.nMP) W.cursor[i] = 0;
    if (i < W.nE) W.off[i] = 0;
    if (i < 16) reinterpret_cast<int32_t *>(W.solveOk)[i] = 0;          // solveOk, maxDiag, stopSeen / cur, err (64 bytes)
}
// Edges usually arrive grouped by landmark (the reference builds them landmark by landmark): a run of equal landmarks inside a wave issues ONE
// atomic (its first lane, with the run's length) instead of one per edge on the same address.  Any input order stays correct: runs are then short.
__device__ __forceinline__ void baws_run(int key, bool live, int *runLen, int *rankInRun, bool *head) {
    const int lane = threadIdx.x & 63;
    const int prev = __shfl_up(key, 1);
    const bool prevLive = __shfl_up((int)live, 1) != 0;
    *head = live && (lane == 0 || !prevLive || prev != key);
    const unsigned long long heads = __ballot(*head), lives = __ballot(live);
    // the run of this lane starts at the last head at or below it and ends before the next head or dead lane
    const unsigned long long below = heads & ((2ull << lane) - 1);
    const int start = 63 - __clzll(below | 1ull);          // (live lanes always have a head at or below them)
    unsigned long long stop = (heads | ~lives) & ~((2ull << lane) - 1);       // first lane above that starts another run or is not part of one
    const int end = stop ? __ffsll((long long)stop) - 1 : 64;
    *rankInRun = lane - start; *runLen = end - start;
}
__global__ void k_baws_count(const BAWin *__restrict__ wins) {
    const BAWin &W = wins[blockIdx.y];
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    unsigned mp = 0;
    bool live = false;
    if (e < W.nE) {
        mp = (unsigned)W.rawMP[e];
        const unsigned kf = (unsigned)W.rawKF[e];
        live = mp < (unsigned)W.nMP && kf < (unsigned)W.nKF;
        if (!live) atomicOr(W.err, 1);
    }
    int len, rank; bool head;
    baws_run((int)mp, live, &len, &rank, &head);
    if (head) atomicAdd(&W.cursor[mp], len);
}
__global__ __launch_bounds__(1024) void k_baws_scan(const BAWin *__restrict__ wins) {
    __shared__ int wsum[16];
    const BAWin &W = wins[blockIdx.x];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), nMP = W.nMP;
    for (int i = tid; i < nMP * 3; i += 1024) W.X[0][i] = (double)W.rawX[i];
    for (int i = tid; i < W.nKF * 8; i += 1024) W.T[0][i] = W.rawT[i];
    const int per = (nMP + 1023) / 1024, i0 = tid * per, i1 = min(nMP, i0 + per);
    int sum = 0;
    for (int i = i0; i < i1; i++) sum += W.cursor[i];
    int inc = sum;                                        // inclusive scan over the workgroup
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { const int o = __shfl_up(inc, d); if (lane >= d) inc += o; }
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    int base = 0;
    for (int w = 0; w < wave; w++) base += wsum[w];
    int run = base + inc - sum;
    for (int i = i0; i < i1; i++) { const int cnt = W.cursor[i]; W.ptStart[i] = run; W.cursor[i] = run; run += cnt; }
    if (tid == 1023) W.ptStart[nMP] = base + inc;
}
__global__ void k_baws_scatter(const BAWin *__restrict__ wins) {
    const BAWin &W = wins[blockIdx.y];
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    unsigned mp = 0;
    bool live = false;
    if (e < W.nE) {
        mp = (unsigned)W.rawMP[e];
        live = mp < (unsigned)W.nMP && (unsigned)W.rawKF[e] < (unsigned)W.nKF;
    }
    int len, rank; bool head;
    baws_run((int)mp, live, &len, &rank, &head);
    int base = 0;
    if (head) base = atomicAdd(&W.cursor[mp], len);
    base = __shfl(base, (threadIdx.x & 63) - rank);        // the run's first lane
    if (live) W.tmpEdge[base + rank] = e;
}
__global__ __launch_bounds__(256) void k_baws_order(const BAWin *__restrict__ wins) {
    __shared__ unsigned pres[32];                         // per column block: which of the chunk's 16 landmarks have an edge of that key-frame
    const BAWin &W = wins[blockIdx.y];
    if ((int)blockIdx.x >= W.nBlk) return;
    const int tid = threadIdx.x, g = tid >> 4, l16 = tid & 15;
    if (tid < 32) pres[tid] = 0;
    __syncthreads();
    const int p = blockIdx.x * 16 + g;
    const bool valid = p < W.nMP;
    const int s0 = valid ? W.ptStart[p] : 0, s1 = valid ? W.ptStart[p + 1] : 0, k = s1 - s0;
    // rank of every edge of the segment by edge index (distinct values): rounds of 16 candidates against the whole segment
    for (int r = l16; r < k; r += 16) {
        const int e = W.tmpEdge[s0 + r];
        int rank = 0;
        for (int q = 0; q < k; q++) rank += W.tmpEdge[s0 + q] < e ? 1 : 0;
        const int s = s0 + rank, kf = W.rawKF[e];
        W.sEdge[s] = e; W.sMP[s] = p; W.sKF[s] = kf;
        reinterpret_cast<float2 *>(W.obs)[s] = reinterpret_cast<const float2 *>(W.rawObs)[e];
        W.info[s] = W.rawInfo[e];
        const int col = W.poseCol[kf];
        if (col >= 0) { if (atomicOr(&pres[col], 1u << g) & (1u << g)) atomicOr(W.err, 2); }
    }
    __syncthreads();
    if (tid < 32) W.blkCnt[(size_t)blockIdx.x * 32 + tid] = __popc(pres[tid]);
    for (int s = s0 + l16; s < s1; s += 16) {
        const int col = W.poseCol[W.sKF[s]];
        W.rank8[s] = col >= 0 ? (uint8_t)__popc(pres[col] & ((1u << g) - 1)) : 0;
    }
}
__global__ __launch_bounds__(1024) void k_baws_kfscan(const BAWin *__restrict__ wins) {
    __shared__ int tot[32];
    const BAWin &W = wins[blockIdx.x];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);            // 16 waves, two column blocks each: exclusive scan over the chunks
    for (int c = 2 * wave; c < 2 * wave + 2; c++) {
        int run = 0;
        for (int b0 = 0; b0 < W.nBlk; b0 += 64) {
            const int b = b0 + lane, v = b < W.nBlk ? W.blkCnt[(size_t)b * 32 + c] : 0;
            int inc = v;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) { const int o = __shfl_up(inc, d); if (lane >= d) inc += o; }
            if (b < W.nBlk) W.blkCnt[(size_t)b * 32 + c] = run + inc - v;
            run += __shfl(inc, 63);
        }
        if (lane == 0) tot[c] = run;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int run = 0;
        for (int k = 0; k < W.nOpt; k++) { W.kfRowStart[k] = run; run += 2 * tot[k]; }
        W.kfRowStart[W.nOpt] = run;
    }
}
__global__ __launch_bounds__(256) void k_baws_rowslot(const BAWin *__restrict__ wins) {
    const BAWin &W = wins[blockIdx.y];
    if ((int)blockIdx.x >= W.nBlk) return;
    const int tid = threadIdx.x, g = tid >> 4, l16 = tid & 15;
    const int p = blockIdx.x * 16 + g;
    if (p >= W.nMP) return;
    const int s0 = W.ptStart[p], s1 = W.ptStart[p + 1];
    for (int s = s0 + l16; s < s1; s += 16) {
        const int col = W.poseCol[W.sKF[s]];
        W.rowSlot[s] = col >= 0 ? W.kfRowStart[col] + 2 * (W.blkCnt[(size_t)blockIdx.x * 32 + col] + W.rank8[s]) : -1;
    }
}

// erase flags of the edges (Optimizer.cc:1292) and the final state gathered behind them, per window (k_ba_finalize with the window as blockIdx.y)
__global__ void k_baw_finalize(const BAWin *__restrict__ wins) {
    const BAWin &W = wins[blockIdx.y];
    const int cur = W.cur0;                               // (the table is uploaded again before this launch: the host knows the final buffer)
    const double *T = W.T[cur], *X = W.X[cur];
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e == 0) *W.errOut = *W.err;
    if (e < W.nKF * 8) W.outT[e] = T[e];
    if (e < W.nMP * 3) W.outX[e] = X[e];
    if (e >= W.ptStart[W.nMP]) return;                    // (edges with an index out of range were left out and reported)
    const int p = W.sMP[e];
    const D3 pc = se3_map(load_pose(T, W.sKF[e]), D3{X[3 * p], X[3 * p + 1], X[3 * p + 2]});
    double chi2 = W.lastChi2[e];
    if (!W.useLast) {
        double u, v;
        cam_project(W.cam, pc, u, v);
        const double e0 = (double)W.obs[2 * e] - u, e1 = (double)W.obs[2 * e + 1] - v, w = (double)W.info[e];
        chi2 = e0 * w * e0 + e1 * w * e1;
    }
    W.erase[W.sEdge[e]] = (chi2 > 5.991 || !(pc.z > 0.0)) ? 1 : 0;
}

// merge BA, between its two optimisations (Optimizer.cc:3996-4010): edges with chi2 > 5.991 or non-positive depth go to level 1
__global__ void k_baw_mark(const BAWin *__restrict__ wins) {
    const BAWin &W = wins[blockIdx.y];
    const int cur = W.stopSeen[1];
    const double *T = W.T[cur], *X = W.X[cur];
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= W.ptStart[W.nMP]) return;
    const int p = W.sMP[e];
    const D3 pc = se3_map(load_pose(T, W.sKF[e]), D3{X[3 * p], X[3 * p + 1], X[3 * p + 2]});
    W.off[e] = (W.lastChi2[e] > 5.991 || !(pc.z > 0.0)) ? 1 : 0;
}
