// submap_sim3.inc -- the RANSAC of CloudMerging::ComputeSubmapSim3 (R/lib_src/CloudMerging.cc:643-741) over a resident score set, every solver in one
// call (host side: submap_sim3_host.inc).  Included by opt.hip inside namespace rumi, after sim3_batch.inc: the minimal solve, the world transform of a
// hypothesis, CheckInliers of a wave and ComputeInliersNum's test of one match are sim3.inc's / sim3_batch.inc's own device text, so every
// per-iteration number is the byte rumi_sim3_ransac returns for the same solver and triple.
//
// The iterations of all solvers form one stream (solver j runs [sum of the its before it, + its_j): a solver that does not converge uses all its
// iterations and the first that converges ends the loop).  A chunk [g0, g1) of the stream runs k_sms_hyp, k_sms_check, k_sms_score, k_sms_median
// and k_sms_select; the select kernel carries the sequential rule's state across chunks in device memory.

constexpr int kSmsHT = 16;            // hypotheses a workgroup of k_sms_score walks with its matches in registers
constexpr int kSmsSlab = 256;         // matches of one key-frame pair a workgroup takes: one a lane

struct SmsSolver {                    // RumiSubmapSolver as it is uploaded
    int32_t first, n, minInliers, its, fixScale;
    float K1[4], K2[4];
    double Skf[16];                   // S_kf1w, S_kf2w
};
static_assert(sizeof(SmsSolver) == sizeof(RumiSubmapSolver) && sizeof(SmsSolver) == 184, "the solver records are uploaded as they come");
struct SmsResult {                    // RumiSubmapSolverResult
    int32_t state, its, bestHyp, bestInliers;
    float bestRatioAfter, T12[16];
};
static_assert(sizeof(SmsResult) == sizeof(RumiSubmapSolverResult) && sizeof(SmsResult) == 84, "the result records are downloaded as they are");

// The sequential rule's state between chunks.  The host reads the first 16 bytes after every chunk.
struct SmsState {
    int32_t converged, consumed, solver, posInSolver;
    int32_t bestN, bestHyp, lastN, lastHyp;      // mnBestInliers and the iteration held as mBest*; the solver's last valid iteration (what a degenerate set repeats)
    float bestRatio, lastRatio;
    int32_t hasLast, pad;
};

// device view of the resident score set
struct SmsSet {
    int nPairs, total, nSlabs;
    const int32_t *denom, *slab;      // slab [nSlabs][3]: key-frame pair, first match, matches (<= kSmsSlab)
    const double *Sc1w1, *Sc2w2;
    const float *K;                   // K4_1, K4_2
    const float *X1, *X2, *kp1, *kp2, *sg1, *sg2;
    const uint8_t *e1, *e2;
};

struct SmsArgs {
    SmsSet set;
    int g0, g1, nIter;                // the chunk of the stream and its length in all (score entry: the transforms)
    const SmsSolver *sol;
    const int32_t *itSol, *tri;       // per iteration: its solver, its minimal set (relative to the solver's first correspondence)
    const float *X1, *X2, *thr1, *thr2;
    float *Tall, *rows12, *rows21;    // [H][16], [H][12] x 2
    double *Sw;                       // [H][16]: gSw1w2 and its inverse
    const double *Sgiven1, *Sgiven2;  // score entry: caller-formed gSc1w2 / gSc2w1 [n_S][nPairs][8]
    int32_t *nIn, *cnt;               // [H], [H][nPairs]
    float *ratio, *med;               // [H][nPairs], [H]
    uint8_t *inl;                     // score entry: [n_S][total], may be null
    SmsState *st; SmsResult *res;
};

// one lane per iteration: ComputeSim3 of its minimal set, then gSw1w2 and its inverse
__global__ __launch_bounds__(64) void k_sms_hyp(SmsArgs A) {
    const int g = A.g0 + blockIdx.x * 64 + threadIdx.x;
    if (g >= A.g1) return;
    const SmsSolver &s = A.sol[A.itSol[g]];
    float R[3][3], t12[3], s12;
    sim3_minimal_solve(A.X1 + (size_t)s.first * 3, A.X2 + (size_t)s.first * 3, A.tri + (size_t)g * 3, s.fixScale, A.rows12 + (size_t)g * 12, A.rows21 + (size_t)g * 12,
                       A.Tall + (size_t)g * 16, R, t12, s12);
    const DSim3 W = sim3_hyp_world(R, t12, s12, s.Skf);
    sim3_to8(W, A.Sw + (size_t)g * 16);
    sim3_to8(sim3_inverse(W), A.Sw + (size_t)g * 16 + 8);
}

// one wave per iteration, four to a workgroup: CheckInliers over the solver's correspondences (the rumination overload keeps no mask)
__global__ __launch_bounds__(256) void k_sms_check(SmsArgs A) {
    const int lane = threadIdx.x & 63, g = A.g0 + blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (g >= A.g1) return;
    const SmsSolver &s = A.sol[A.itSol[g]];
    const int cnt = sim3_check_wave(lane, s.n, s.K1, s.K2, A.rows12 + (size_t)g * 12, A.rows21 + (size_t)g * 12, A.X1 + (size_t)s.first * 3, A.X2 + (size_t)s.first * 3,
                                    A.thr1 + s.first, A.thr2 + s.first, nullptr);
    if (lane == 0) A.nIn[g] = cnt;
}

// ComputeInliersNum's counts: workgroup (slab, tile) holds one match a lane in registers and walks the tile's hypotheses, whose two composites of the
// slab's key-frame pair (gSc1w1 * gSw1w2, gSc2w2 * gSw1w2^-1; FORM = false: the caller's) sit in LDS and are read as broadcasts.  Counts by ballot and
// popcount: one LDS add a wave, one global integer add a workgroup into cnt [hypothesis][pair] (zeroed before the launch).
template <bool FORM> __global__ __launch_bounds__(256) void k_sms_score(SmsArgs A) {
    __shared__ double sComp[kSmsHT][16];
    __shared__ int sCnt[kSmsHT];
    const int tid = threadIdx.x, lane = tid & 63;
    const int tile = blockIdx.x / A.set.nSlabs;                      // the grid is one-dimensional: tiles x slabs may pass the 65 535 of grid.y
    const int32_t *sl = A.set.slab + (size_t)(blockIdx.x - tile * A.set.nSlabs) * 3;
    const int p = sl[0], first = sl[1], count = sl[2];
    const int h0 = A.g0 + tile * kSmsHT, nh = min(kSmsHT, A.g1 - h0), np = A.set.nPairs;
    if (tid < 2 * nh) {
        const int h = tid >> 1, side = tid & 1;
        double *dst = sComp[h] + side * 8;
        if (FORM) {
            const double *own = (side ? A.set.Sc2w2 : A.set.Sc1w1) + (size_t)p * 8;
            sim3_to8(sim3_mul(sim3_from8(own), sim3_from8(A.Sw + (size_t)(h0 + h) * 16 + side * 8)), dst);
        } else {
            const double *src = (side ? A.Sgiven2 : A.Sgiven1) + ((size_t)(h0 + h) * np + p) * 8;
            for (int k = 0; k < 8; k++) dst[k] = src[k];
        }
    }
    if (tid < kSmsHT) sCnt[tid] = 0;
    __syncthreads();
    const bool have = tid < count;
    const size_t i = (size_t)first + (have ? tid : 0);
    float K1[4], K2[4], x1[3], x2[3], k1[2], k2[2];
    for (int k = 0; k < 4; k++) { K1[k] = A.set.K[k]; K2[k] = A.set.K[4 + k]; }
    for (int k = 0; k < 3; k++) { x1[k] = A.set.X1[i * 3 + k]; x2[k] = A.set.X2[i * 3 + k]; }
    for (int k = 0; k < 2; k++) { k1[k] = A.set.kp1[i * 2 + k]; k2[k] = A.set.kp2[i * 2 + k]; }
    const float sg1 = A.set.sg1[i], sg2 = A.set.sg2[i];
    const bool e1 = A.set.e1[i] != 0, e2 = A.set.e2[i] != 0;
    for (int h = 0; h < nh; h++) {
        const bool in = have && sim3_score_inlier(sComp[h], sComp[h] + 8, K1, K2, x1, x2, k1, k2, sg1, sg2, e1, e2);
        if (A.inl && have) A.inl[(size_t)(h0 + h) * A.set.total + i] = in;
        const int c = __popcll(__ballot(in));
        if (lane == 0 && c) atomicAdd(&sCnt[h], c);
    }
    __syncthreads();
    if (tid < nh && sCnt[tid]) atomicAdd(&A.cnt[(size_t)(h0 + tid) * np + p], sCnt[tid]);
}

// one wave per hypothesis, four to a workgroup: ratio[p] = count / denominator in float (:643-647), then the value at sorted position nPairs / 2
// (:654-662) by rank counting: v sits there when fewer than or exactly nPairs / 2 ratios are below it and more than nPairs / 2 are not above it.
__global__ __launch_bounds__(256) void k_sms_median(SmsArgs A) {
    const int lane = threadIdx.x & 63, g = A.g0 + blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), np = A.set.nPairs;
    if (g >= A.g1) return;
    float *ratio = A.ratio + (size_t)g * np;
    for (int p = lane; p < np; p += 64) ratio[p] = A.set.denom[p] ? (float)A.cnt[(size_t)g * np + p] / (float)A.set.denom[p] : 0.f;
    __threadfence();                                                 // the wave reads back what its own lanes wrote: no other wave touches this row
    const int k = np / 2;
    float m = 0.f;
    bool found = false;
    for (int p = lane; p < np; p += 64) {
        const float v = ratio[p];
        int less = 0, leq = 0;
        for (int q = 0; q < np; q++) { const float r = ratio[q]; less += r < v; leq += r <= v; }
        if (less <= k && k < leq) { m = v; found = true; }
    }
    const unsigned long long who = __ballot(found);
    m = __shfl(m, __ffsll((long long)who) - 1);
    if (lane == 0) A.med[g] = m;
}

// one wave: the sequential rule (Sim3Solver.cc:352-375, CloudMerging.cc:663-741) over the chunk in stream order.  The lanes load 64 iterations'
// (valid, nIn, ratio) at a time; every lane then walks them through shuffles and keeps the same state, lane 0 (the T12 record: 16 lanes) writes.
__global__ __launch_bounds__(64) void k_sms_select(SmsArgs A) {
    const int lane = threadIdx.x;
    SmsState st = *A.st;
    if (st.converged) return;
    int minInliers = A.sol[st.solver].minInliers, its = A.sol[st.solver].its;      // of the current solver: read again only when it changes
    for (int base = A.g0; base < A.g1 && !st.converged; base += 64) {
        const int g = base + lane, cntBlock = min(64, A.g1 - base);
        int v = 0, n = 0;
        float r = 0.f;
        if (g < A.g1) { v = A.Tall[(size_t)g * 16 + 13] != 0.f; n = A.nIn[g]; r = A.med[g]; }
        for (int k = 0; k < cntBlock && !st.converged; k++) {
            const int vv = __shfl(v, k), nn = __shfl(n, k), gi = base + k;
            const float rr = __shfl(r, k);
            // a degenerate minimal set repeats the solver's last valid iteration; without one it counts nothing under the ratio of its identity record
            if (vv) { st.lastN = nn; st.lastRatio = rr; st.lastHyp = gi; st.hasLast = 1; }
            else if (!st.hasLast) { st.lastN = 0; st.lastRatio = rr; st.lastHyp = gi; st.hasLast = 1; }
            st.posInSolver++; st.consumed++;
            if (st.lastRatio >= st.bestRatio && st.lastN >= st.bestN) {
                st.bestN = st.lastN; st.bestRatio = st.lastRatio; st.bestHyp = st.lastHyp;
                if ((double)st.lastRatio > 0.10 && st.lastN > minInliers) st.converged = 1;
            }
            if (st.converged || st.posInSolver == its) {
                SmsResult &o = A.res[st.solver];
                if (lane < 16) o.T12[lane] = st.bestHyp >= 0 ? A.Tall[(size_t)st.bestHyp * 16 + lane] : 0.f;
                if (lane == 0) {
                    o.state = st.converged ? RUMI_SIM3_CONVERGED : RUMI_SIM3_EXHAUSTED;
                    o.its = st.posInSolver; o.bestHyp = st.bestHyp; o.bestInliers = st.bestN; o.bestRatioAfter = st.bestRatio;
                }
                if (!st.converged) {
                    st.solver++; st.posInSolver = 0; st.bestN = 0; st.bestHyp = -1; st.hasLast = 0;
                    if (gi + 1 < A.nIter) { minInliers = A.sol[st.solver].minInliers; its = A.sol[st.solver].its; }      // (after the last iteration there is no next solver)
                }
            }
        }
    }
    if (lane == 0) *A.st = st;
}
