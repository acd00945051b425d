// MI355X-native pose optimisation and bundle adjustment behind include/rumi_opt.h.  One translation unit: this file holds the optimiser handle
// (RumiOptimizer and its parts, create / destroy, the footprint and profiling getters, fetch_published_scalars) and includes the kernels and the host entries by job.
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
//   submap_sim3.inc     k_sms_*: the RANSAC of ComputeSubmapSim3 over a resident score set, every solver in one call.  Host: submap_sim3_host.inc
//   ba_windows.inc      k_baw_* / k_baws_*: local BA with the window as a batch dimension.  Host: ba_windows_host.inc
//   essential.inc       k_eg_*: OptimizeEssentialGraph.  Host: essential_host.inc
//   ba_resident.inc     k_lba_*: the local window assembled from the covisibility store (rumi_local_ba_resident).  Host: ba_resident_host.inc
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
#include <memory>
#include <vector>

#include "opt_math.h"
#include "rumi_internal.h"
#include "rumi_common.h"
#include "rumi_opt.h"
#include "rumi_covis.h"
#include "covis_view.h"

namespace rumi {

typedef double v4f64 __attribute__((ext_vector_type(4)));

#include "opt_reduce.h"
#include "pose_opt.inc"
#include "ba_single.inc"
#include "ba_solve_tiles.inc"
#include "ba_big.inc"
#include "chol_blocked.inc"
#include "sim3.inc"
#include "sim3_batch.inc"
#include "submap_sim3.inc"
#include "ba_windows.inc"
#include "essential.inc"
#include "ba_resident.inc"

}  // namespace rumi

using namespace rumi;

// ================================================ host side =======================================================
// Every block below has ONE owner (rumi_common.h: DevBuf, MirrorBuf, MappedBuf); include/rumi_opt.h states the element counts.
static size_t al16(size_t x) { return (x + 15) & ~(size_t)15; }   // offsets inside the transfer blocks
template <class B> static void take(int &rc, B &b, size_t n) { if (rc == RUMI_OK) rc = b.reserve(n, n); }   // a chain of these stops at the first failure

// PoseOptimization: the transfer blocks of a batch and the kernel's per-correspondence scratch
struct PoseBlocks {
    int maxEdges = 0, maxBatch = 0;
    MirrorBuf<uint8_t> in, out;
    DevBuf<uint8_t> active;
    DevBuf<double> lastChi2;
    int init(size_t PE, size_t PB) {
        maxEdges = (int)PE; maxBatch = (int)PB;
        int rc = RUMI_OK;
        take(rc, active, PE); take(rc, lastChi2, PE);
        take(rc, in, (PB + 1) * 4 + 16 + PB * 28 + PE * 24 + 256); take(rc, out, PB * 32 + PE + 256);
        return rc;
    }
    void count(Footprint &f) const { f.add(in, out, active, lastChi2); }
};

// One bundle-adjustment window's device state.  The window-batched kernels (ba_windows.inc) use the first two parts; ba_run's host loop, Sim3 and
// the essential graph also the third, which only an arena made with `hostLoop` holds.
struct BaArena {
    int maxKF = 0, maxMP = 0, maxE = 0;
    MirrorBuf<uint8_t> stage;        // transfer blocks: the upload (graph arrays are read in place from its device half) ...
    DevBuf<uint8_t> stageOut;        // ... and the results
    DevBuf<double> T[2], X[2], panel, Dinv, bl, Hpp, bp, xv, chi;
    DevBuf<uint8_t> eOff;
    MappedBuf<int32_t> stop;         // the reference's stop flag as the window-batched kernels read it
    // extras of the window-batched kernels, taken by the first window staged here (extras())
    DevBuf<double> Gpart, Gw, chiPart, sclPart;
    DevBuf<uint8_t> winSmall, sorted;   // winSmall: [0] solveOk (f64), [1] maxDiag (u64), [2] stopSeen, cur (2 x i32), [3] err (i32); sorted: the graph in landmark order (k_baws_*)
    DevBuf<LmCtl> lmCtl;
    MappedBuf<WinMirror> wm;
    struct HostLoop {
        int npCap = 0;               // padded width of the dense Schur panel this arena holds
        DevBuf<double> Hll, Hpl, Yt, G, Lp, Aglob, scal;
        MappedBuf<double> pub;       // [0..7] the trial's scalars, [8] sequence number of the last publication (k_ba_publish)
        unsigned long long pubSeq = 0;
        DevBuf<double> W;            // H_pl L per edge, taken by the first large-window call
        DevBuf<int32_t> colOf;       // column block of every edge's key-frame (-1 fixed), same
        DevBuf<uint8_t> pairs; size_t pairOff = 0;   // Schur block descriptors + observation pairs (int32) of the large-window path; pairOff: where the pairs begin
        std::vector<int32_t> fill;   // counting-sort cursors of ba_run
    } solo;

    int init(size_t K, size_t M, size_t E, bool hostLoop) {
        maxKF = (int)K; maxMP = (int)M; maxE = (int)E;
        const size_t N = 6 * K;
        int rc = RUMI_OK;
        take(rc, stage, E * 48 + M * 32 + K * 80 + 1024); take(rc, stageOut, stage.cap);
        for (int i = 0; i < 2; i++) { take(rc, T[i], K * 8); take(rc, X[i], M * 3); }
        take(rc, panel, E * 16 + 64); take(rc, Dinv, M * 9); take(rc, bl, M * 3); take(rc, Hpp, K * 36); take(rc, bp, N);
        take(rc, xv, N + M * 3); take(rc, chi, E); take(rc, eOff, E); take(rc, stop, 16);
        if (!hostLoop) return rc;
        solo.npCap = (int)std::min<size_t>((N + 1 + 15) / 16 * 16, 256);
        const size_t NP = (size_t)solo.npCap;
        take(rc, solo.Hll, M * 9); take(rc, solo.Hpl, E * 18); take(rc, solo.Yt, 3 * M * NP); take(rc, solo.G, NP * NP); take(rc, solo.Lp, M * 6);
        take(rc, solo.Aglob, (N + 2) * (N + 2) + 2 * N); take(rc, solo.scal, 8); take(rc, solo.pub, 16);
        return rc;
    }
    // Any of these may fail and the call be repeated: what is already there is kept, the rest is taken then.
    int extras() {
        const size_t nTmax = (size_t)kSolveTilesMax * (kSolveTilesMax + 1) / 2, E = (size_t)maxE, M = (size_t)maxMP;
        const size_t parts = std::max<size_t>(kBawMaxSlices, (M + 31) / 32) + 8;
        auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
        int rc = RUMI_OK;
        take(rc, Gpart, (size_t)kBawMaxSlices * nTmax * 256); take(rc, Gw, nTmax * 256); take(rc, chiPart, parts); take(rc, sclPart, parts);
        take(rc, winSmall, 64); take(rc, sorted, al((M + 1) * 4) * 2 + al(64 * 4) + al(E * 4) * 6 + al(E * 8) + al(E) + al((M / 16 + 2) * 32 * 4));
        take(rc, lmCtl, 2); take(rc, wm, 1);
        return rc;
    }
    void count(Footprint &f) const {
        f.add(stage, stageOut, T[0], T[1], X[0], X[1], panel, Dinv, bl, Hpp, bp, xv, chi, eOff, stop, Gpart, Gw, chiPart, sclPart, winSmall, sorted, lmCtl, wm);
        f.add(solo.Hll, solo.Hpl, solo.Yt, solo.G, solo.Lp, solo.Aglob, solo.scal, solo.pub, solo.W, solo.colOf, solo.pairs);
    }
};

static_assert(sizeof(BAWin) == 488 && sizeof(LmCtl) == 64 && sizeof(WinMirror) == 24, "include/rumi_opt.h states these sizes in its allocation paragraph");
// What a chain of launches needs: stream, events, the window table of a launch group and the block its results come back in (sized for
// kBawMaxWindows windows of the handle's limits: it never grows).
struct BaRunner {
    int device = 0;
    StreamHold stream;               // bundle adjustments run on a stream of their own (non-blocking): handles on different host threads overlap on the device
    EventHold ev[2];
    MirrorBuf<BAWin> winTab;
    MirrorBuf<uint8_t> groupOut;     // results of a launch group, gathered for one copy back
    unsigned bawRun = 0;
    float stageMs[8] = {0};
    int init(int dev, size_t K, size_t M, size_t E) {
        device = dev;
        int rc = stream.create();
        for (auto &e : ev) if (rc == RUMI_OK) rc = e.create();
        const size_t perWindow = (al16(al16(al16(al16(K * 64) + M * 24) + E) + 16) + 255) & ~(size_t)255;   // [T | X | erase | err], as baw_stage lays it out
        take(rc, winTab, kBawMaxWindows); take(rc, groupOut, perWindow * kBawMaxWindows);
        return rc;
    }
    void count(Footprint &f) const { f.add(winTab, groupOut); }
};

// An arena with every part and a runner: what one single-window run (ba_run) needs
struct BaContext {
    BaArena arena;
    BaRunner run;
    int init(int dev, size_t K, size_t M, size_t E) { const int rc = arena.init(K, M, E, true); return rc != RUMI_OK ? rc : run.init(dev, K, M, E); }
    void count(Footprint &f) const { arena.count(f); run.count(f); }
};

// opt-in per-kernel timing of the bundle adjustment (rumi_opt_set_profiling): event pairs around the pose-block Gram product, the Schur
// SYRK and the reduced solve of every trial, summed after the trial's own synchronisation
struct BaProfile {
    bool on = false;
    EventHold ev[6];
    float kernelMs[4] = {0};          // hpp, syrk, solve (ms over the call), trials
};

// rumi_local_ba_resident (ba_resident_host.inc): what the assembly of a window needs beyond the handle's own arena, taken by the first call
struct LbaResident {
    MirrorBuf<uint8_t> in, out;      // locals and roles up; the head, the key-frame list, the point ids and the erase list back
    DevBuf<uint8_t> work, edge;      // lists, counts and stamps of one call; per edge the observer word and the erase list
    DevBuf<unsigned long long> ptTag;   // [max_points of the store] first-occurrence stamps, epoch << 32 | priority
    EventHold ev;                    // the assembly (null stream) before the runner's stream
    uint32_t epoch = 0;
    std::vector<int32_t> locals, role;
    void count(Footprint &f) const { f.add(in, out, work, edge, ptTag); }
};

// The sub-map alignment session (submap_sim3_host.inc): the resident score set of rumi_submap_sim3_begin and the blocks of a call, all grown on demand
struct SubmapSim3Part {
    bool have = false;               // between begin and end
    int chunk = 0;                   // iterations between two read-backs of the state; 0 = the growing default (rumi_hook_submap_sim3_set_chunk)
    SmsSet view{};                   // where the parts of `set` lie on the device
    MirrorBuf<uint8_t> set;          // the score set as begin laid it out
    MirrorBuf<uint8_t> io, out;      // a call's upload with the state and result records; its per-iteration results
    DevBuf<uint8_t> work;            // rows of [sR | t], gSw1w2 and its inverse, counts and ratios per (iteration, pair)
    void count(Footprint &f) const { f.add(set, io, out, work); }
};

constexpr int kBaMaxWorkers = 16;
struct RumiOptimizer {
    int device = 0;
    PoseBlocks pose;
    BaContext ba;                    // the handle's own window: rumi_local_ba / merge / global BA, Sim3 and the essential graph run here
    BaProfile prof;
    // rumi_local_ba_batch; each owns nothing until the first batch that needs it, then keeps it: an arena (without the host-loop part) per window
    // of a launch wave, a runner per launch group after the first, a full context per worker thread of the windows that take ba_run's host loop
    BaArena batchArenas[kBawMaxWindows];
    BaRunner batchRunners[3];
    BaContext workers[kBaMaxWorkers];
    // essential graph (essential_host.inc): the dense matrix and one block for the rest, taken by the first rumi_essential_graph call
    DevBuf<uint8_t> egA, eg;
    LbaResident lba;
    SubmapSim3Part sms;
};

extern "C" void rumi_opt_destroy(RumiOptimizer *o) {
    if (!o) return;
    (void)hipSetDevice(o->device);
    delete o;
}

extern "C" int rumi_opt_create(int32_t max_pose_edges, int32_t max_pose_batch, int32_t max_kf, int32_t max_mp, int32_t max_edges,
                               int32_t device, RumiOptimizer **out) {
    if (!out) return RUMI_E_INVALID;
    *out = nullptr;
    if (max_pose_edges < 1 || max_pose_batch < 1 || max_kf < 1 || max_mp < 1 || max_edges < 1) { g_lastError = "rumi_opt_create: sizes must be >= 1"; return RUMI_E_INVALID; }
    int rc = require_device();
    if (rc != RUMI_OK) return rc;
    std::unique_ptr<RumiOptimizer> o(new RumiOptimizer());
    if (device >= 0) o->device = device; else if (hipGetDevice(&o->device) != hipSuccess) o->device = 0;
    HIP_TRY(hipSetDevice(o->device));
    rc = o->pose.init(max_pose_edges, max_pose_batch);
    if (rc == RUMI_OK) rc = o->ba.init(o->device, max_kf, max_mp, max_edges);
    for (auto &e : o->prof.ev) if (rc == RUMI_OK) rc = e.create();
    if (rc != RUMI_OK) return rc;
    *out = o.release();
    return RUMI_OK;
}

extern "C" int rumi_opt_footprint(const RumiOptimizer *o, int64_t out2[2]) {
    if (!o || !out2) return RUMI_E_INVALID;
    Footprint f;
    o->pose.count(f); o->ba.count(f); f.add(o->egA, o->eg); o->lba.count(f); o->sms.count(f);
    for (const auto &a : o->batchArenas) a.count(f);
    for (const auto &r : o->batchRunners) r.count(f);
    for (const auto &w : o->workers) w.count(f);
    out2[0] = f.dev; out2[1] = f.pin;
    return RUMI_OK;
}

extern "C" int rumi_opt_set_profiling(RumiOptimizer *o, int32_t on) {
    if (!o) return RUMI_E_INVALID;
    o->prof.on = on != 0;
    return RUMI_OK;
}
extern "C" int rumi_opt_kernel_ms(RumiOptimizer *o, float ms[4]) {
    if (!o || !ms) return RUMI_E_INVALID;
    for (int i = 0; i < 4; i++) ms[i] = o->prof.kernelMs[i];
    return RUMI_OK;
}

extern "C" int rumi_opt_stage_ms(RumiOptimizer *o, float ms[8]) {
    if (!o || !ms) return RUMI_E_INVALID;
    for (int i = 0; i < 8; i++) ms[i] = o->ba.run.stageMs[i];
    return RUMI_OK;
}

#include "pose_opt_host.inc"

// The eight scalars of s.scal -> s.pub without a runtime synchronisation (see k_ba_publish); falls back to one if the stream has drained
// without the sequence number arriving (a failed launch).  Shared by the bundle adjustments and the essential graph.
static int fetch_published_scalars(BaArena::HostLoop &s, hipStream_t st) {
    const unsigned long long seq = ++s.pubSeq;
    hipLaunchKernelGGL(k_ba_publish, dim3(1), dim3(64), 0, st, s.scal.p, s.pub.d, seq);
    HIP_TRY(hipGetLastError());
    volatile unsigned long long *flag = reinterpret_cast<volatile unsigned long long *>(s.pub.h + 8);
    for (unsigned spin = 0; *flag != seq; spin++) {
        if ((spin & 0xFFFF) == 0xFFFF && hipStreamQuery(st) != hipErrorNotReady) {
            HIP_TRY(hipStreamSynchronize(st));
            if (*flag != seq) { HIP_TRY(hipMemcpyAsync(s.pub.h, s.scal.p, 8 * sizeof(double), hipMemcpyDeviceToHost, st)); HIP_TRY(hipStreamSynchronize(st)); break; }
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
#include "sim3_batch_host.inc"
#include "submap_sim3_host.inc"
#include "ba_resident_host.inc"
