// sim3_batch.inc -- place recognition's Sim3 RANSAC and OptimizeSim3 over every candidate in one call (host side: sim3_batch_host.inc).
// Included by opt.hip inside namespace rumi, after sim3.inc: the per-hypothesis and per-problem work is sim3.inc's own device text.
//
// RANSAC (Sim3Solver::iterate(nIterations, bNoMore, vbInliers, nInliers, bConverge), R/lib_src/Sim3Solver.cc:222-290): J solvers share the
// process-wide rand(), so solver j + 1 draws where solver j stopped.  Iterations are whole triples of that stream: iteration g of the window uses
// the same three numbers whichever solver runs it, only the mapping to indices depends on the solver's N.  Every solver therefore evaluates all R
// iterations of the window with its own N (k_s3b_hyp, k_s3b_check) and one wave then walks the solvers in order and picks where each stopped
// (k_s3b_select).  Convergence is local: the first valid iteration with more than min_inliers inliers returns (an earlier one with at least as
// many would itself have returned; a degenerate set repeats a count that did not return).

struct S3bSolver {                    // RumiSim3RansacSolver plus where the solver's correspondences start
    int32_t first, n, minInliers, itsLeft, fixScale;
    float K1[4], K2[4];
};
static_assert(sizeof(S3bSolver) == sizeof(RumiSim3RansacSolver), "the solver records are uploaded as they come");
struct S3bResult {                    // RumiSim3RansacResult
    int32_t state, its, hyp, nInliers;
    float T12[16];
};
static_assert(sizeof(S3bResult) == sizeof(RumiSim3RansacResult), "the result records are downloaded as they are");

struct S3bArgs {
    int J, R, nMax;
    const S3bSolver *sol;
    const float *X1, *X2, *thr1, *thr2;
    const int32_t *tri;               // [J][R][3], relative to the solver's first correspondence
    float *rows12, *rows21;           // [J*R][12] rows of [sR | t]
    float *Tall; int32_t *nInAll;     // [J*R][16], [J*R]
    uint8_t *mask;                    // [J*R][nMax]
    S3bResult *res; uint8_t *inl;     // [J], [total]
};

// one lane per (solver, hypothesis): ComputeSim3 of its minimal set
__global__ __launch_bounds__(256) void k_s3b_hyp(S3bArgs A) {
    const int g = blockIdx.x * 256 + threadIdx.x;
    if (g >= A.J * A.R) return;
    const S3bSolver &s = A.sol[g / A.R];
    float R[3][3], t12[3], s12;
    sim3_minimal_solve(A.X1 + (size_t)s.first * 3, A.X2 + (size_t)s.first * 3, A.tri + (size_t)g * 3, s.fixScale, A.rows12 + (size_t)g * 12, A.rows21 + (size_t)g * 12,
                       A.Tall + (size_t)g * 16, R, t12, s12);
}

// CheckInliers of one hypothesis over the n correspondences of its solver by one wave: the count by ballot + popcount (the same in every lane), the
// mask where the caller keeps one.  k_s3b_check and k_sms_check (submap_sim3.inc) both call it.
__device__ __forceinline__ int sim3_check_wave(int lane, int n, const float *K1, const float *K2, const float *rows12, const float *rows21, const float *X1,
                                               const float *X2, const float *thr1, const float *thr2, uint8_t *mask) {
    float T12[12], T21[12];
    for (int k = 0; k < 12; k++) { T12[k] = rows12[k]; T21[k] = rows21[k]; }
    int cnt = 0;
    for (int base = 0; base < n; base += 64) {
        const int i = base + lane;
        bool in = false;
        if (i < n) {
            in = sim3_check_inlier(K1, K2, T12, T21, X1 + (size_t)i * 3, X2 + (size_t)i * 3, thr1[i], thr2[i]);
            if (mask) mask[i] = in;
        }
        cnt += __popcll(__ballot(in));
    }
    return cnt;
}

// one wave per (solver, hypothesis), four to a workgroup: CheckInliers over the solver's correspondences
__global__ __launch_bounds__(256) void k_s3b_check(S3bArgs A) {
    const int lane = threadIdx.x & 63, g = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (g >= A.J * A.R) return;
    const S3bSolver &s = A.sol[g / A.R];
    const int cnt = sim3_check_wave(lane, s.n, s.K1, s.K2, A.rows12 + (size_t)g * 12, A.rows21 + (size_t)g * 12, A.X1 + (size_t)s.first * 3, A.X2 + (size_t)s.first * 3,
                                    A.thr1 + s.first, A.thr2 + s.first, A.mask + (size_t)g * A.nMax);
    if (lane == 0) A.nInAll[g] = cnt;
}

// one wave: the sequential rule over the window, solver by solver
__global__ __launch_bounds__(64) void k_s3b_select(S3bArgs A) {
    const int lane = threadIdx.x;
    int pos = 0;
    bool ended = false;                                           // the window ran out inside an earlier solver: the rest is not reached
    for (int j = 0; j < A.J; j++) {
        const S3bSolver &s = A.sol[j];
        int state = RUMI_SIM3_NOT_REACHED, its = 0, hyp = -1;
        if (!ended) {
            const long long last = (long long)pos + s.itsLeft;    // its_left may be anything up to INT32_MAX
            const int end = last < A.R ? (int)last : A.R;
            for (int base = pos; base < end && hyp < 0; base += 64) {
                const int h = base + lane;
                const bool ok = h < end && A.Tall[((size_t)j * A.R + h) * 16 + 13] != 0.f && A.nInAll[(size_t)j * A.R + h] > s.minInliers;
                const unsigned long long m = __ballot(ok);
                if (m) hyp = base + __ffsll((long long)m) - 1;
            }
            if (hyp >= 0) { state = RUMI_SIM3_CONVERGED; its = hyp - pos + 1; pos = hyp + 1; }
            else if (last <= A.R) { state = RUMI_SIM3_EXHAUSTED; its = s.itsLeft; pos += s.itsLeft; }
            else { state = RUMI_SIM3_WINDOW_ENDED; its = A.R - pos; ended = true; }
        }
        const size_t g = (size_t)j * A.R + (hyp >= 0 ? hyp : 0);
        const uint8_t *row = A.mask + g * A.nMax;
        for (int i = lane; i < s.n; i += 64) A.inl[s.first + i] = hyp >= 0 ? row[i] : (uint8_t)0;
        if (lane < 16) A.res[j].T12[lane] = hyp >= 0 ? A.Tall[g * 16 + lane] : 0.f;
        if (lane == 0) { A.res[j].state = state; A.res[j].its = its; A.res[j].hyp = hyp; A.res[j].nInliers = hyp >= 0 ? A.nInAll[g] : 0; }
    }
}


// Optimizer::OptimizeSim3 of J candidates (pair form): one 256-thread workgroup per problem runs sim3_opt_run over its entry of the table.
__global__ __launch_bounds__(256) void k_sim3_opt_batch(const Sim3Args *tab) { sim3_opt_run(tab[blockIdx.x]); }
