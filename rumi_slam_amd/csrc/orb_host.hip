// Host side of the C ABI in include/rumi_orb.h: handle, HBM arenas, stage scheduling.
// Reference behaviour: ORBextractor::operator() R/lib_src/ORBextractor.cc:1014-1091.
//
// One translation unit.  This file holds the error plumbing, the handle (RumiOrb: state that spans calls), create / destroy / alloc_frame_arenas,
// the small setters and rumi_orb_sync, and includes the rest by job:
//   orb_geometry.inc    set_geometry (level and resize tables, the one-launch pyramid's tiles), rumi_orb_tables
//   orb_schedule.inc    OutLayout, CallOpts (what one call asks beyond its arguments), extract_async_impl with its three stream arrangements,
//                       the device-batch entries
//   orb_host_batch.inc  extract_batch_host_impl (the feeder of host-resident batches) and its two entries
//   orb_single.inc      rumi_orb_image_buffer, rumi_orb_extract, RumiOrbStream and the rumi_orb_stream_* entries
//   orb_taps.inc        rumi_orb_pyramid_level, fetch_taps, rumi_orb_stage_keypoints
//   orb_kfd.inc         RumiKfd and the rumi_kfd_* entries (include/rumi_kfd.h): the PD frame selector, whose selected frames go through this extractor
#include <hip/hip_runtime.h>

#include <cstdlib>

#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstring>
#include <functional>
#include <string>
#include <thread>
#include <vector>

#include "flow_device.h"
#include "orb_device.h"
#include "orb_octree.h"
#include "rumi_common.h"
#include "rumi_internal.h"
#include "rumi_kfd.h"
#include "rumi_match.h"

using namespace rumi;

namespace rumi {
thread_local std::string g_lastError;
void set_error(const char *fmt, const char *a, const char *b, int line) {
    char buf[512];
    snprintf(buf, sizeof buf, fmt, a, b, line);
    g_lastError = buf;
}
}  // namespace rumi

extern "C" const char *rumi_last_error(void) { return g_lastError.c_str(); }

extern "C" int rumi_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

namespace {
constexpr int kChunk = 256;  // frames per pass through the candidate / quadtree scratch arenas
// Frames per sub-chunk of the resident queue.  256 since the end of round 3 (64 before): with the latency-bound kernels of a sub-chunk's chain
// shortened (compaction, quadtree) larger launches win at every call size (1024-frame steps +3 %, 128-frame calls +5 %).
constexpr int kResidentSub = 256;
static int scratch_frames(int maxBatch) { return (std::min(kChunk, maxBatch) + 11) / 12 * 12; }
}  // namespace

struct RumiOrb {
    RumiOrbConfig cfg{};
    OrbTables tab;
    int device = 0;
    int hostThreads = 1;
    // capacities (from max_width x max_height)
    long long capArena = 0;
    int capCells = 0, capCand = 0, capCellCand = 0, capSel = 0, capCoef = 0;
    // geometry of the current image size
    int gw = 0, gh = 0;
    DevParams hP{};
    DevParams *dP = nullptr;
    int16_t *dCoef = nullptr;
    RowTap *dRowTab = nullptr; int capRowTab = 0;   // per level and output row: source rows and vertical taps of the resize
    PyrTile *dPyrTiles = nullptr; int nPyrTiles = 0, pyrBuf = 0, pyrTab = 0;   // the one-launch pyramid (k_pyramid_tiles) of calls of a few frames: 0 tiles = not available for this geometry
    // HBM arenas (sized for max_batch frames unless noted)
    uint8_t *dIn = nullptr;          // staging for the single-frame host API (1 frame, rows padded to a multiple of 4 bytes)
    uint8_t *dL0 = nullptr;          // staging for device frames whose base / pitch / frame stride is not 4-byte aligned (allocated on first use)
    uint8_t *hIn = nullptr, *hOut1 = nullptr, *dOut1 = nullptr;   // pinned image / pinned + device [counts | kp | desc] block of that API
    uint8_t *dhOut1 = nullptr;        // the pinned block as the device addresses it: a one-frame call's kernels write counts, key-points and descriptors
    int32_t *dhErr = nullptr;         // straight into host memory (and k_assemble the final error word): no copy back, the call ends with its last kernel
    uint8_t *dPyr = nullptr, *dBlur = nullptr;
    uint32_t *dCellBuf = nullptr;    // kChunk frames
    int32_t *dCellCnt = nullptr;
    uint32_t *dCand = nullptr;       // kChunk frames x capCand
    int32_t *dLevelStart = nullptr;
    uint32_t *dSelPacked = nullptr, *dSelMeta = nullptr;   // kChunk frames x capSel
    int32_t *dSelCount = nullptr;
    float4 *dSelTrig = nullptr;      // kChunk frames x capSel: {angle, cos, sin, 0} of k_disc_angle (batches)
    uint32_t *dDiscVec = nullptr;    // k_disc_angle's per-row weight and mask vectors (make_disc_vectors of tab.umax)
    uint16_t *dOwner = nullptr;      // kChunk frames x capCand: quadtree node id of every candidate
    uint32_t *dSelLevel = nullptr;   // kChunk frames x nlevels x selLevelCap: quadtree output per level
    int32_t *dSelLevelCnt = nullptr;
    int32_t *dErr = nullptr;         // device error word (bit 0/1/2/3: roots, node pool, level cap, selection cap; bit 4: FAST candidate capacity);
                                     // sticky over the asynchronous calls since the last rumi_orb_sync.  Words 1, 2: the batch quadtree's
                                     // cumulative {trees finished by k_octree_narrow, trees redone}; they travel to hErr with the error word
    // batch quadtree pipeline (orb_device.h: OctNarrow): coordinate tables of the current geometry; per scratch frame the cell histogram and the
    // cell -> rank table (capOctCells 16-bit entries each), per (frame, level) the list length, per slot range the redo list and its counters
    uint16_t *dOctBins = nullptr; int capOctBins = 0, capOctCells = 0;
    uint32_t *dOctHist = nullptr, *dOctRank = nullptr;
    int32_t *dOctM = nullptr, *dOctRedo = nullptr, *dOctCtl = nullptr;
    uint32_t octStatBase[2] = {0, 0};        // the (wrapping) counters when the handle was last idle
    int32_t octStat[2] = {0, 0};             // the calls since, as of the last rumi_orb_sync
    bool octDirty = false;                   // a call returned between launch_compact and launch_octree: histogram / counters are not zero
    // host-resident batches (rumi_orb_extract_batch_host): device landing arena, pinned staging slots, copy streams
    DevBuf<uint8_t> hostIn;
    static constexpr int kFeedSlots = 4, kFeedFrames = 64;
    uint8_t *hFeed[kFeedSlots] = {nullptr}; size_t hFeedBytes = 0;
    hipEvent_t evFeed[kFeedSlots] = {nullptr};
    hipStream_t copyStream = nullptr, copyStream2 = nullptr;     // host -> device transfers of rumi_orb_extract_batch_host, groups alternating (two DMA engines)
    bool pending = false;            // an asynchronous call has been enqueued and not yet waited for
    hipStream_t pendingStream = nullptr;
    int selLevelCap = 0;
    OctLdsSizes octLds{0, 0, 0};
    // pinned host words
    int32_t *hErr = nullptr;
    // host copies fetched lazily by the stage taps
    std::vector<uint32_t> tapCand, tapSelPacked, tapSelMeta;
    std::vector<int32_t> tapLevelStart, tapSelCount;
    bool tapValid = false;
    // last-call bookkeeping for the stage taps
    ImgSrc lastSrc{};
    int lastFrames = 0, lastChunkBase = 0, lastChunkFrames = 0, lastChunkSlot = 0;   // frames / scratch slot the stage taps can read
    RumiKeyPoint *lastKp = nullptr;  // device pointer the last call wrote key-points to
    long long lastKpStride = 0;      // bytes between the key-points of consecutive frames there
    int32_t *lastCounts = nullptr;
    int lastOutCap = 0;
    bool profiling = false;
    float stageMs[8] = {0};
    hipEvent_t ev[8] = {nullptr};
    // the blur only depends on the pyramid: it runs on a side stream next to FAST / quadtree and joins before rBRIEF
    hipStream_t sideStream = nullptr;                // (made at the first call that forks the blur: ensure_side)
    hipEvent_t evFork = nullptr, evJoin = nullptr;   // fork / join of the blur on sideStream
    // a chunk's frames are split over the caller's stream and slots 1.. (slot 0 is the caller's stream except in the resident queue); the caller's
    // stream waits for slot p's sub-chunks on slotJoin[p]
    static constexpr int kMaxParts = 8;
    // A slot's streams exist from the first arrangement that drives them (ensure_lanes): every stream a handle creates holds a reference on one
    // of the process's few hardware queues, and the runtime places the next stream on the least-referenced queue, so idle streams only push
    // the driven ones together.
    struct Lane { hipStream_t s, bs; hipEvent_t fork, join; };   // main stream, blur stream (bs == s: the blur in line, no fork / join), fork / join of the blur
    Lane slot[kMaxParts] = {};
    hipEvent_t slotJoin[kMaxParts] = {nullptr};
    // rumi_orb_set_resident_queue: the frames of a call do not depend on work pending on the caller's stream, so sub-chunk 0 gets a stream of
    // its own too (with its blur stream) and no sub-chunk waits for the caller's stream: back-to-back calls then overlap like the sub-chunks of
    // one large call, only the caller's stream waits for each call's results
    bool residentQueue = false;
    int residentSlots = 4;                    // slots the caller asked for (2 .. kMaxParts): calls in flight, and what the arenas are sized for
    StreamPlan plan{4, true};                 // ... and what of them is driven: plan.streams slot streams, the blur in line or on blur streams (orb_geom.h: stream_plan)
    int scratchFrames = 0, arenaFrames = 0;   // frames the scratch arrays / the pyramid and blur arenas hold
    int rot = 0;                     // slot of the next sub-chunk
    hipEvent_t userReady = nullptr;  // rumi_orb_wait_event: the sub-chunks of the next resident-queue call start behind it
    bool lastResident = false;       // the previous batched call ran in the resident-queue arrangement
    hipEvent_t evPartFork = nullptr, evB0 = nullptr, evB1 = nullptr;
};

#include "orb_geometry.inc"

// The per-frame device arrays (alloc_frame_arenas sizes them), named once: released and forgotten.
static void free_frame_arenas(RumiOrb *h) {
    auto drop = [](auto *&...p) { (((p ? (void)hipFree(p) : (void)0), p = nullptr), ...); };
    drop(h->dPyr, h->dBlur, h->dCellBuf, h->dCellCnt, h->dCand, h->dLevelStart, h->dSelPacked, h->dSelMeta, h->dSelTrig, h->dSelCount, h->dOwner, h->dSelLevel, h->dSelLevelCnt);
    drop(h->dOctHist, h->dOctRank, h->dOctM, h->dOctRedo, h->dOctCtl);
}

extern "C" void rumi_orb_destroy(RumiOrb *h) {
    if (!h) return;
    (void)hipSetDevice(h->device);
    if (h->pending) (void)hipStreamSynchronize(h->pendingStream);
    void *dev[] = {h->dP, h->dCoef, h->dRowTab, h->dOctBins, h->dPyrTiles, h->dIn, h->dL0, h->dErr, h->dDiscVec};
    for (void *p : dev) if (p) (void)hipFree(p);
    free_frame_arenas(h);
    void *pin[] = {h->hErr};
    for (void *p : pin) if (p) (void)hipHostFree(p);
    for (auto &e : h->ev) if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : {h->evFork, h->evJoin, h->evB0, h->evB1, h->evPartFork}) if (e) (void)hipEventDestroy(e);
    if (h->sideStream) (void)hipStreamDestroy(h->sideStream);
    for (const auto &L : h->slot)
        for (hipStream_t s : {L.s, L.bs}) if (s) (void)hipStreamDestroy(s);
    for (const auto &L : h->slot)
        for (hipEvent_t e : {L.fork, L.join}) if (e) (void)hipEventDestroy(e);
    for (auto &e : h->slotJoin) if (e) (void)hipEventDestroy(e);
    for (auto &p : h->hFeed) if (p) (void)hipHostFree(p);
    for (auto &e : h->evFeed) if (e) (void)hipEventDestroy(e);
    if (h->copyStream) (void)hipStreamDestroy(h->copyStream);
    if (h->copyStream2) (void)hipStreamDestroy(h->copyStream2);
    if (h->hIn) (void)hipHostFree(h->hIn);
    if (h->hOut1) (void)hipHostFree(h->hOut1);
    if (h->dOut1) (void)hipFree(h->dOut1);
    delete h;
}

// The state the batch quadtree pipeline keeps zero between launches: every frame's cell histogram and every slot range's redo counters.
static int zero_octree_state(RumiOrb *h) {
    const size_t C = (size_t)h->scratchFrames;
    HIP_TRY(hipMemset(h->dOctHist, 0, std::max<size_t>(C * (h->capOctCells / 2), 1) * sizeof(uint32_t)));
    HIP_TRY(hipMemset(h->dOctCtl, 0, std::max<size_t>(C * 4, 1) * sizeof(int32_t)));
    h->octDirty = false;
    return RUMI_OK;
}

// The per-frame device arrays: candidate / quadtree scratch for `scratch` frames, pyramid and blurred levels for `arena` frames.  Called by
// rumi_orb_create and again by rumi_orb_set_resident_queue when the slots of the resident queue need more than the handle was created with.
static int alloc_frame_arenas(RumiOrb *h, size_t scratch, size_t arena) {
    free_frame_arenas(h);
    const size_t C = scratch;
    int rc;
    h->scratchFrames = 0; h->arenaFrames = 0;          // until everything below has succeeded the handle has NO arenas (extract refuses to run: RUMI_E_CAPACITY)
#define TRY_A(x) if ((rc = (x)) != RUMI_OK) return rc;
    TRY_A(dev_alloc(&h->dPyr, (size_t)h->capArena * arena));
    TRY_A(dev_alloc(&h->dBlur, (size_t)h->capArena * arena));
    TRY_A(dev_alloc(&h->dCellBuf, C * h->capCells * h->capCellCand));
    TRY_A(dev_alloc(&h->dCellCnt, C * h->capCells));
    TRY_A(dev_alloc(&h->dCand, C * h->capCand));
    TRY_A(dev_alloc(&h->dLevelStart, C * (kMaxLevels + 1)));
    TRY_A(dev_alloc(&h->dSelPacked, C * h->capSel));
    TRY_A(dev_alloc(&h->dSelMeta, C * h->capSel));
    TRY_A(dev_alloc(&h->dSelTrig, C * h->capSel));
    TRY_A(dev_alloc(&h->dSelCount, C));
    TRY_A(dev_alloc(&h->dOwner, C * h->capCand));
    TRY_A(dev_alloc(&h->dSelLevel, C * h->cfg.nlevels * h->selLevelCap));
    TRY_A(dev_alloc(&h->dSelLevelCnt, C * h->cfg.nlevels));
    TRY_A(dev_alloc(&h->dOctHist, C * (h->capOctCells / 2)));
    TRY_A(dev_alloc(&h->dOctRank, C * (h->capOctCells / 2)));
    TRY_A(dev_alloc(&h->dOctM, C * h->cfg.nlevels));
    TRY_A(dev_alloc(&h->dOctRedo, C * h->cfg.nlevels));
    TRY_A(dev_alloc(&h->dOctCtl, C * 4));
#undef TRY_A
    h->scratchFrames = (int)scratch; h->arenaFrames = (int)arena;
    // zeroed once: k_octree_narrow clears what it reads of the histogram, k_octree_redo's last workgroup its counters
    if (const int rz = zero_octree_state(h); rz != RUMI_OK) { h->scratchFrames = 0; h->arenaFrames = 0; return rz; }
    return RUMI_OK;
}

extern "C" int rumi_orb_create(const RumiOrbConfig *cfg, RumiOrb **out) {
    if (!out) return RUMI_E_INVALID;
    *out = nullptr;
    if (!cfg || cfg->nlevels < 1 || cfg->nlevels > kMaxLevels || cfg->nfeatures < 1 || cfg->max_batch < 1 ||
        cfg->max_width < 1 || cfg->max_height < 1 || !(cfg->scale_factor > 1.0f) || cfg->blur_variant < 0 || cfg->blur_variant > 1) {
        g_lastError = "invalid RumiOrbConfig";
        return RUMI_E_INVALID;
    }
    if (const int rc = require_device(); rc != RUMI_OK) return rc;
    RumiOrb *h = new RumiOrb();
    h->cfg = *cfg;
    if (cfg->device >= 0) { h->device = cfg->device; }
    else if (hipGetDevice(&h->device) != hipSuccess) h->device = 0;
    if (hipSetDevice(h->device) != hipSuccess) { delete h; g_lastError = "hipSetDevice failed"; return RUMI_E_NO_DEVICE; }
    h->tab = make_tables(cfg->nfeatures, cfg->scale_factor, cfg->nlevels);
    h->hostThreads = cfg->host_threads > 0 ? cfg->host_threads
                                           : (int)std::min<unsigned>(16u, std::max(1u, std::thread::hardware_concurrency()));
    std::vector<LevelGeom> g;
    int cells, cand, cellCand;
    if (!make_geometry(h->tab, cfg->max_width, cfg->max_height, g, &h->capArena, &cells, &cand, &cellCand)) {
        delete h;
        g_lastError = "max_width x max_height too small for the FAST cell grid at some level";
        return RUMI_E_INVALID;
    }
    int coefN = 0;
    for (int l = 1; l < cfg->nlevels; l++) coefN += 3 * (g[l].w + g[l].h);
    h->capCells = cells + cells / 8 + 16;            // slack: smaller images can have slightly different grids
    h->capCellCand = cellCand + cellCand / 2 + 16;
    int candSum = 0;
    for (int l = 0; l < cfg->nlevels; l++) candSum += std::min(g[l].candCap, 65535);
    h->capCand = candSum + 64;
    h->capCoef = coefN + 64 * cfg->nlevels;
    h->capRowTab = 0;
    for (int l = 1; l < cfg->nlevels; l++) h->capRowTab += g[l].h + 8;
    h->capSel = cfg->nfeatures + 4 * cfg->nlevels + 64;   // the quadtree may return a few more than N per level
    int maxN = 0;
    for (int l = 0; l < cfg->nlevels; l++) maxN = std::max(maxN, h->tab.featuresPerLevel[l]);
    h->selLevelCap = maxN + 4 * 16 + 8;
    // batch quadtree tables: a level's coordinate tables are shorter than its width + height; twice the depth-D cells of the largest geometry
    // (another aspect ratio has other root counts), at most 4096 per level -- a geometry that wants more keeps the one-launch kernel
    for (int l = 0; l < cfg->nlevels; l++) {
        h->capOctBins += g[l].w + g[l].h;
        h->capOctCells += 2 * oct_level_tabs(g[l].maxBX - kBorder, g[l].maxBY - kBorder, h->tab.featuresPerLevel[l]).cells;
    }
    h->capOctCells = std::min(std::max(h->capOctCells, 512), 4096 * cfg->nlevels);
    // scratch arenas: frames of one pass, rounded up to a multiple of 12 so that 2, 3 or 4 equal slots hold ceil(frames / parts) each
    const size_t B = (size_t)cfg->max_batch, C = (size_t)scratch_frames(cfg->max_batch);
    int rc = RUMI_OK;
#define TRY_ALLOC(x) if ((rc = (x)) != RUMI_OK) { rumi_orb_destroy(h); return rc; }
    TRY_ALLOC(dev_alloc(&h->dP, 1));
    TRY_ALLOC(dev_alloc(&h->dCoef, (size_t)h->capCoef));
    TRY_ALLOC(dev_alloc(&h->dRowTab, (size_t)std::max(h->capRowTab, 1)));
    TRY_ALLOC(dev_alloc(&h->dOctBins, (size_t)h->capOctBins));
    TRY_ALLOC(dev_alloc(&h->dIn, (size_t)((cfg->max_width + 3) & ~3) * cfg->max_height));
    TRY_ALLOC(alloc_frame_arenas(h, C, B));
    TRY_ALLOC(dev_alloc(&h->dOut1, (size_t)16 + (size_t)h->capSel * 60));
    if (hipHostMalloc((void **)&h->hIn, (size_t)((cfg->max_width + 3) & ~3) * cfg->max_height, hipHostMallocDefault) != hipSuccess ||
        hipHostMalloc((void **)&h->hOut1, (size_t)16 + (size_t)h->capSel * 60, hipHostMallocDefault) != hipSuccess) {
        rumi_orb_destroy(h); g_lastError = "pinned staging"; return RUMI_E_NO_DEVICE;
    }
    TRY_ALLOC(dev_alloc(&h->dErr, 4));
    if (hipMemset(h->dErr, 0, 4 * sizeof(int32_t)) != hipSuccess) { rumi_orb_destroy(h); g_lastError = "error word"; return RUMI_E_NO_DEVICE; }
    {
        uint32_t vec[kDiscVecLanes * kDiscVecLaneDwords];
        make_disc_vectors(h->tab.umax.data(), vec);
        TRY_ALLOC(dev_alloc(&h->dDiscVec, sizeof vec / sizeof vec[0]));
        if (hipMemcpy(h->dDiscVec, vec, sizeof vec, hipMemcpyHostToDevice) != hipSuccess) { rumi_orb_destroy(h); g_lastError = "disc vectors"; return RUMI_E_NO_DEVICE; }
    }
    TRY_ALLOC(pin_alloc(&h->hErr, 4));
    std::memset(h->hErr, 0, 4 * sizeof(int32_t));
    if (hipHostGetDevicePointer((void **)&h->dhOut1, h->hOut1, 0) != hipSuccess || hipHostGetDevicePointer((void **)&h->dhErr, h->hErr, 0) != hipSuccess) {
        (void)hipGetLastError();
        h->dhOut1 = nullptr; h->dhErr = nullptr;            // (no device view of the pinned blocks: the copies stay)
    }
#undef TRY_ALLOC
    for (auto &e : h->ev)
        if (hipEventCreate(&e) != hipSuccess) { rumi_orb_destroy(h); g_lastError = "hipEventCreate"; return RUMI_E_NO_DEVICE; }
    if (hipEventCreateWithFlags(&h->evPartFork, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&h->evFork, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&h->evJoin, hipEventDisableTiming) != hipSuccess || hipEventCreate(&h->evB0) != hipSuccess ||
        hipEventCreate(&h->evB1) != hipSuccess) { rumi_orb_destroy(h); g_lastError = "hipEventCreate"; return RUMI_E_NO_DEVICE; }
    *out = h;
    return RUMI_OK;
}

// The streams and events of slots [p0, p1), made when an arrangement first drives them (rumi_orb_set_resident_queue, the first call of equal
// sub-chunks); blurStreams: with a blur stream and its fork / join events each.  rumi_orb_destroy frees what exists.
static int ensure_lanes(RumiOrb *h, int p0, int p1, bool blurStreams) {
    for (int p = p0; p < p1; ++p) {
        RumiOrb::Lane &L = h->slot[p];
        if (!L.s) HIP_TRY(hipStreamCreateWithFlags(&L.s, hipStreamNonBlocking));
        if (!h->slotJoin[p]) HIP_TRY(hipEventCreateWithFlags(&h->slotJoin[p], hipEventDisableTiming));
        if (!blurStreams) continue;
        if (!L.bs) HIP_TRY(hipStreamCreateWithFlags(&L.bs, hipStreamNonBlocking));
        if (!L.fork) HIP_TRY(hipEventCreateWithFlags(&L.fork, hipEventDisableTiming));
        if (!L.join) HIP_TRY(hipEventCreateWithFlags(&L.join, hipEventDisableTiming));
    }
    return RUMI_OK;
}
static int ensure_side(RumiOrb *h) {
    if (!h->sideStream) HIP_TRY(hipStreamCreateWithFlags(&h->sideStream, hipStreamNonBlocking));
    return RUMI_OK;
}
extern "C" int rumi_orb_set_profiling(RumiOrb *h, int32_t on) {
    if (!h) return RUMI_E_INVALID;
    h->profiling = on != 0;
    return RUMI_OK;
}
extern "C" int rumi_orb_set_resident_queue(RumiOrb *h, int32_t on) {
    if (!h) return RUMI_E_INVALID;
    if (h->pending) { const int rc = rumi_orb_sync(h); if (rc != RUMI_OK) return rc; }
    if (on) {
        // `on` slots (1: the default of four) of up to 256 frames each: their scratch ranges and their ranges of the pyramid / blur arenas
        const int slots = on == 1 ? 4 : std::min(std::max(on, 2), (int)RumiOrb::kMaxParts);
        h->residentSlots = slots;
        h->plan = stream_plan(slots, hw_queues_env());
        HIP_TRY(hipSetDevice(h->device));
        if (const int rc = ensure_lanes(h, 0, h->plan.streams, !h->plan.blurInline); rc != RUMI_OK) return rc;
        const int need = (slots * std::min(kResidentSub, h->cfg.max_batch) + 23) / 24 * 24;
        if (h->scratchFrames < need || h->arenaFrames < need) {
            HIP_TRY(hipSetDevice(h->device));
            HIP_TRY(hipDeviceSynchronize());
            const size_t oldS = (size_t)h->scratchFrames, oldA = (size_t)h->arenaFrames;
            int rc = alloc_frame_arenas(h, std::max(oldS, (size_t)need), std::max(oldA, (size_t)need));
            if (rc != RUMI_OK) {                             // back to the sizes the handle had (those fitted before); if even that fails the handle refuses to extract
                h->residentQueue = false;
                (void)alloc_frame_arenas(h, oldS, oldA);
                g_lastError = "resident queue: device arenas";
                return rc;
            }
            h->lastFrames = 0; h->tapValid = false;
        }
    }
    h->residentQueue = on != 0;
    return RUMI_OK;
}
extern "C" int rumi_orb_wait_event(RumiOrb *h, void *hip_event) {
    if (!h) return RUMI_E_INVALID;
    h->userReady = (hipEvent_t)hip_event;
    return RUMI_OK;
}
extern "C" int rumi_orb_stage_ms(RumiOrb *h, float ms[8]) {
    if (!h || !ms) return RUMI_E_INVALID;
    for (int i = 0; i < 8; i++) ms[i] = h->stageMs[i];
    return RUMI_OK;
}

extern "C" int rumi_orb_octree_stats(RumiOrb *h, int32_t trees[2]) {
    if (!h || !trees) return RUMI_E_INVALID;
    trees[0] = h->octStat[0]; trees[1] = h->octStat[1];
    return RUMI_OK;
}

extern "C" int rumi_orb_sync(RumiOrb *h) {
    if (!h) return RUMI_E_INVALID;
    if (!h->pending) return RUMI_OK;
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipStreamSynchronize(h->pendingStream));
    h->pending = false;
    for (int i = 0; i < 2; i++) h->octStat[i] = (int32_t)((uint32_t)h->hErr[1 + i] - h->octStatBase[i]);   // (unsigned: the device counters wrap)
    const int err = *h->hErr;
    if (err & 16) { g_lastError = "FAST candidate capacity exceeded (more than 65535 in one level)"; return RUMI_E_CAPACITY; }
    if (err & 1) { g_lastError = "aspect ratio gives 0 or more than 16 quadtree roots"; return RUMI_E_INVALID; }
    if (err & 2) { g_lastError = "quadtree node pool exhausted"; return RUMI_E_INVALID; }
    if (err & (4 | 8)) { g_lastError = "more key-points than the handle's selection capacity"; return RUMI_E_CAPACITY; }
    return RUMI_OK;
}

#include "orb_schedule.inc"
#include "orb_host_batch.inc"
#include "orb_single.inc"
#include "orb_taps.inc"
#include "orb_kfd.inc"
