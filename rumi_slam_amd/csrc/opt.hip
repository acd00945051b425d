// MI355X-native pose optimisation and bundle adjustment behind include/rumi_opt.h.  One translation unit: this file holds the optimiser handle
// (RumiOptimizer, create / destroy, the profiling getters, fetch_published_scalars) and includes the kernels and the host entries by job.
//   opt_reduce.h        wave / workgroup sums (DPP, v_permlane*_swap), readlane_f64, fast_rsqrt
//   pose_opt.inc        k_pose_opt: the whole 4-round / 10-iteration LM loop of a frame in one workgroup; frames batch.  Host: pose_opt_host.inc
//   ba_single.inc       one window, LM trials driven from the host (ba_single_host.inc: ba_run) over device-resident double-precision state:
//                       k_ba_chi2, k_ba_build (residuals, Jacobians, H_ll, b_l, H_pl, pose panel), k_ba_hpp_mfma (H_pp, b_p on the f64 matrix cores),
//                       k_ba_zero, k_ba_maxdiag, k_ba_dinv_yfill / k_ba_dinv (D^-1 = L L^T per landmark, the dense panel Y = H_pl L),
//                       k_ba_syrk_mfma (Schur complement Y Y^T as a split-K SYRK), k_ba_solve (reduced system of 180..252 unknowns, one workgroup),
//                       k_ba_update (back-substitution, oplus into the TRIAL state), k_ba_mark, k_ba_finalize, k_ba_publish (a trial's scalars)
//   ba_solve_tiles.inc  k_ba_solve_tiles: reduced system up to 175 unknowns as 16 x 16 tiles in LDS (the core k_baw_solve shares)
//   ba_big.inc          k_big_init / w / schur: block-sparse Schur accumulation of a window of more than 255 unknowns
//   chol_blocked.inc    k_chol_diag / trsm / syrk / backsub: multi-workgroup blocked Cholesky (large windows, essential graph)
//   sim3.inc            k_sim3_inliers / ransac / opt.  Host: sim3_host.inc
//   ba_windows.inc      k_baw_* / k_baws_*: local BA with the window as a batch dimension.  Host: ba_windows_host.inc
//   essential.inc       k_eg_*: OptimizeEssentialGraph.  Host: essential_host.inc
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <atomic>
#include <chrono>
#include <thread>
#include <sys/prctl.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "opt_math.h"
#include "rumi_internal.h"
#include "rumi_common.h"
#include "rumi_opt.h"

namespace rumi {

typedef double v4f64 __attribute__((ext_vector_type(4)));

#include "opt_reduce.h"
#include "pose_opt.inc"
#include "ba_single.inc"
#include "ba_solve_tiles.inc"
#include "ba_big.inc"
#include "chol_blocked.inc"
#include "sim3.inc"
#include "ba_windows.inc"
#include "essential.inc"

}  // namespace rumi

using namespace rumi;

// ================================================ host side =======================================================
struct RumiOptimizer {
    int device = 0;
    int maxPoseEdges = 0, maxPoseBatch = 0, maxKF = 0, maxMP = 0, maxE = 0;
    // pose optimisation
    uint8_t *dActive = nullptr, *dEOff = nullptr;       // pose inputs / outputs live in the transfer blocks below
    double *dLastChi2 = nullptr;
    // BA
    double *dT[2] = {nullptr, nullptr}, *dX[2] = {nullptr, nullptr};   // graph arrays are read in place from the upload mirror (dBa)
    double *dHll = nullptr, *dBl = nullptr, *dHpl = nullptr, *dPanel = nullptr, *dHpp = nullptr, *dBp = nullptr, *dDinv = nullptr,
           *dXv = nullptr, *dChi = nullptr, *dScal = nullptr, *dAglob = nullptr, *dYt = nullptr, *dG = nullptr, *dLp = nullptr;
    int npCap = 0;
    double *dW = nullptr;            // H_pl L per edge, allocated by the first large-window call
    int32_t *dColOf = nullptr;       // column block of every edge's key-frame (-1 fixed), same
    DevBuf<uint8_t> pairs; size_t pairOff = 0;   // Schur block descriptors + observation pairs (int32) of the large-window path; pairOff: where the pairs begin
    double *hScal = nullptr;         // fine-grained pinned: [0..7] the trial's scalars, [8] sequence number of the last publication (k_ba_publish)
    double *dhScal = nullptr;        // the same memory as the device sees it
    unsigned long long pubSeq = 0;
    int32_t *hStop = nullptr, *dhStop = nullptr;   // fine-grained pinned: the reference's stop flag as the window-batched kernels read it
    // window-batched local BA (ba_windows.inc): per-arena extras, allocated on first use; the window table lives in the handle that runs the batch
    double *dGpart = nullptr, *dGw = nullptr, *dChiPart = nullptr, *dSclPart = nullptr;
    uint8_t *dWinSmall = nullptr, *dSorted = nullptr; size_t sortedBytes = 0;
    rumi::LmCtl *dLmCtl = nullptr, *hLmCtl = nullptr;
    rumi::WinMirror *hWm = nullptr, *dhWm = nullptr;
    rumi::BAWin *hWinTab = nullptr, *dWinTab = nullptr;
    unsigned bawRun = 0;
    MirrorBuf<uint8_t> groupOut;     // results of a launch group, gathered for one copy back
    hipStream_t stream = nullptr;    // bundle adjustments of this handle (created non-blocking)
    std::vector<RumiOptimizer *> workers;   // rumi_local_ba_batch: one child handle per worker thread, created on first use
    uint8_t *hPose = nullptr, *hPoseOut = nullptr, *dPoseIn = nullptr, *dPoseOut = nullptr;   // PoseOptimization transfer blocks
    uint8_t *hBa = nullptr, *dBa = nullptr, *dBaOut = nullptr; size_t baStageCap = 0;            // bundle-adjustment transfer blocks
    std::vector<int32_t> hFill;                                                                  // counting-sort cursors of ba_run
    float stageMs[8] = {0};
    hipEvent_t ev[2] = {nullptr, nullptr};
    // opt-in per-kernel timing of the bundle adjustment (rumi_opt_set_profiling): event pairs around the pose-block Gram product, the Schur
    // SYRK and the reduced solve of every trial, summed after the trial's own synchronisation
    bool profiling = false;
    hipEvent_t evK[6] = {nullptr};
    float kernelMs[4] = {0};          // hpp, syrk, solve (ms over the call), trials
    // essential graph (essential_host.inc): the dense matrix and one block for the rest, allocated by the first rumi_essential_graph call
    DevBuf<uint8_t> egA, eg;
};

static size_t al16(size_t x) { return (x + 15) & ~(size_t)15; }   // offsets inside the transfer blocks

extern "C" void rumi_opt_destroy(RumiOptimizer *o) {
    if (!o) return;
    (void)hipSetDevice(o->device);
    for (RumiOptimizer *w : o->workers) rumi_opt_destroy(w);
    o->workers.clear();
    if (o->stream) (void)hipStreamDestroy(o->stream);
    void *p[] = {o->dActive, o->dLastChi2, o->dT[0], o->dT[1], o->dX[0],
                 o->dX[1], o->dHll, o->dBl, o->dHpl, o->dPanel, o->dHpp, o->dBp, o->dDinv, o->dXv, o->dChi, o->dScal,
                 o->dAglob, o->dEOff, o->dYt, o->dG, o->dLp, o->dW, o->dColOf};
    for (void *q : p) if (q) (void)hipFree(q);
    { void *q[] = {o->dGpart, o->dGw, o->dChiPart, o->dSclPart, o->dWinSmall, o->dLmCtl, o->dWinTab, o->dSorted}; for (void *x : q) if (x) (void)hipFree(x); }
    if (o->hLmCtl) (void)hipHostFree(o->hLmCtl);
    if (o->hWm) (void)hipHostFree((void *)o->hWm);
    if (o->hWinTab) (void)hipHostFree(o->hWinTab);
    if (o->hScal) (void)hipHostFree(o->hScal);
    if (o->hStop) (void)hipHostFree(o->hStop);
    if (o->hPose) (void)hipHostFree(o->hPose);
    if (o->hBa) (void)hipHostFree(o->hBa);
    if (o->dBa) (void)hipFree(o->dBa);
    if (o->dBaOut) (void)hipFree(o->dBaOut);
    if (o->hPoseOut) (void)hipHostFree(o->hPoseOut);
    if (o->dPoseIn) (void)hipFree(o->dPoseIn);
    if (o->dPoseOut) (void)hipFree(o->dPoseOut);
    for (auto &e : o->ev) if (e) (void)hipEventDestroy(e);
    for (auto &e : o->evK) if (e) (void)hipEventDestroy(e);
    delete o;
}

extern "C" int rumi_opt_create(int32_t max_pose_edges, int32_t max_pose_batch, int32_t max_kf, int32_t max_mp, int32_t max_edges,
                               int32_t device, RumiOptimizer **out) {
    if (!out) return RUMI_E_INVALID;
    *out = nullptr;
    if (max_pose_edges < 1 || max_pose_batch < 1 || max_kf < 1 || max_mp < 1 || max_edges < 1) { g_lastError = "rumi_opt_create: sizes must be >= 1"; return RUMI_E_INVALID; }
    int rc = require_device();
    if (rc != RUMI_OK) return rc;
    RumiOptimizer *o = new RumiOptimizer();
    if (device >= 0) o->device = device; else if (hipGetDevice(&o->device) != hipSuccess) o->device = 0;
    if (hipSetDevice(o->device) != hipSuccess) { delete o; return RUMI_E_NO_DEVICE; }
    o->maxPoseEdges = max_pose_edges; o->maxPoseBatch = max_pose_batch; o->maxKF = max_kf; o->maxMP = max_mp; o->maxE = max_edges;
    if (hipStreamCreateWithFlags(&o->stream, hipStreamNonBlocking) != hipSuccess) { delete o; return RUMI_E_NO_DEVICE; }
    const size_t PE = max_pose_edges, PB = max_pose_batch, K = max_kf, M = max_mp, E = max_edges, N = 6 * K;
#define TRYA(x) if ((rc = (x)) != RUMI_OK) { rumi_opt_destroy(o); return rc; }
    TRYA(dev_alloc(&o->dActive, PE)); TRYA(dev_alloc(&o->dLastChi2, PE));
    for (int i = 0; i < 2; i++) { TRYA(dev_alloc(&o->dT[i], K * 8)); TRYA(dev_alloc(&o->dX[i], M * 3)); }
    TRYA(dev_alloc(&o->dHll, M * 9)); TRYA(dev_alloc(&o->dBl, M * 3)); TRYA(dev_alloc(&o->dHpl, E * 18)); TRYA(dev_alloc(&o->dPanel, E * 16 + 64));
    TRYA(dev_alloc(&o->dHpp, K * 36)); TRYA(dev_alloc(&o->dBp, N)); TRYA(dev_alloc(&o->dDinv, M * 9));
    TRYA(dev_alloc(&o->dXv, N + M * 3)); TRYA(dev_alloc(&o->dChi, E)); TRYA(dev_alloc(&o->dScal, 8));
    o->npCap = (int)std::min<size_t>((N + 1 + 15) / 16 * 16, 256);
    TRYA(dev_alloc(&o->dAglob, (N + 2) * (N + 2) + 2 * N)); TRYA(dev_alloc(&o->dEOff, E));
    TRYA(dev_alloc(&o->dYt, 3 * M * (size_t)o->npCap)); TRYA(dev_alloc(&o->dG, (size_t)o->npCap * o->npCap)); TRYA(dev_alloc(&o->dLp, M * 6));
#undef TRYA
    if (hipHostMalloc((void **)&o->hScal, 16 * sizeof(double), hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess ||
        hipHostGetDevicePointer((void **)&o->dhScal, o->hScal, 0) != hipSuccess) { rumi_opt_destroy(o); return RUMI_E_NO_DEVICE; }
    std::memset(o->hScal, 0, 16 * sizeof(double));
    if (hipHostMalloc((void **)&o->hStop, 64, hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess ||
        hipHostGetDevicePointer((void **)&o->dhStop, o->hStop, 0) != hipSuccess) { rumi_opt_destroy(o); return RUMI_E_NO_DEVICE; }
    *o->hStop = 0;
    o->baStageCap = E * 48 + M * 32 + K * 80 + 1024;
    if (hipHostMalloc((void **)&o->hBa, o->baStageCap, hipHostMallocDefault) != hipSuccess || hipMalloc((void **)&o->dBa, o->baStageCap) != hipSuccess ||
        hipMalloc((void **)&o->dBaOut, o->baStageCap) != hipSuccess) {
        rumi_opt_destroy(o);
        return RUMI_E_NO_DEVICE;
    }
    {
        const size_t inCap = (PB + 1) * 4 + 16 + PB * 28 + PE * 24 + 256, outCap = PB * 32 + PE + 256;
        if (hipHostMalloc((void **)&o->hPose, inCap, hipHostMallocDefault) != hipSuccess ||
            hipHostMalloc((void **)&o->hPoseOut, outCap, hipHostMallocDefault) != hipSuccess ||
            hipMalloc((void **)&o->dPoseIn, inCap) != hipSuccess || hipMalloc((void **)&o->dPoseOut, outCap) != hipSuccess) {
            rumi_opt_destroy(o);
            return RUMI_E_NO_DEVICE;
        }
    }
    for (auto &e : o->ev) if (hipEventCreate(&e) != hipSuccess) { rumi_opt_destroy(o); return RUMI_E_NO_DEVICE; }
    for (auto &e : o->evK) if (hipEventCreate(&e) != hipSuccess) { rumi_opt_destroy(o); return RUMI_E_NO_DEVICE; }
    *out = o;
    return RUMI_OK;
}

extern "C" int rumi_opt_set_profiling(RumiOptimizer *o, int32_t on) {
    if (!o) return RUMI_E_INVALID;
    o->profiling = on != 0;
    return RUMI_OK;
}
extern "C" int rumi_opt_kernel_ms(RumiOptimizer *o, float ms[4]) {
    if (!o || !ms) return RUMI_E_INVALID;
    for (int i = 0; i < 4; i++) ms[i] = o->kernelMs[i];
    return RUMI_OK;
}

extern "C" int rumi_opt_stage_ms(RumiOptimizer *o, float ms[8]) {
    if (!o || !ms) return RUMI_E_INVALID;
    for (int i = 0; i < 8; i++) ms[i] = o->stageMs[i];
    return RUMI_OK;
}

#include "pose_opt_host.inc"

// The eight scalars of o->dScal -> o->hScal without a runtime synchronisation (see k_ba_publish); falls back to one if the stream has drained
// without the sequence number arriving (a failed launch).  Shared by the bundle adjustments and the essential graph.
static int fetch_published_scalars(RumiOptimizer *o, hipStream_t st) {
    const unsigned long long seq = ++o->pubSeq;
    hipLaunchKernelGGL(k_ba_publish, dim3(1), dim3(64), 0, st, o->dScal, o->dhScal, seq);
    HIP_TRY(hipGetLastError());
    volatile unsigned long long *flag = reinterpret_cast<volatile unsigned long long *>(o->hScal + 8);
    for (unsigned spin = 0; *flag != seq; spin++) {
        if ((spin & 0xFFFF) == 0xFFFF && hipStreamQuery(st) != hipErrorNotReady) {
            HIP_TRY(hipStreamSynchronize(st));
            if (*flag != seq) { HIP_TRY(hipMemcpyAsync(o->hScal, o->dScal, 8 * sizeof(double), hipMemcpyDeviceToHost, st)); HIP_TRY(hipStreamSynchronize(st)); break; }
        }
    }
    __atomic_thread_fence(__ATOMIC_ACQUIRE);
    return RUMI_OK;
}

#include "ba_host_shared.inc"
#include "ba_windows_host.inc"
#include "essential_host.inc"

#include "ba_single_host.inc"
#include "sim3_host.inc"
