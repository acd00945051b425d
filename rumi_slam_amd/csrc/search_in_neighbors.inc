// The search half of LocalMapping::SearchInNeighbors (R/lib_src/LocalMapping.cc:649-743) for every target key-frame in one call, behind
// rumi_search_in_neighbors_resident (include/rumi_mapping.h).  Included at the end of mapping.hip; everything is read where the covisibility
// store keeps it, through a CovisView (covis_view.h).
//
// What the device computes is the search of ORBmatcher::Fuse (ORBmatcher.cc:1037-1174) on the map as it stands at the call: bestIdx for a
// (key-frame, point) pair reads the point's position, normal, distance range and descriptor and the key-frame's pose, key-points,
// descriptors, scale table and bounds.  The host replays AddObservation / AddMapPoint / Replace in the reference's order.  One of those inputs
// can change during the replay: Replace ends with ComputeDistinctiveDescriptors() on the survivor (MapPoint.cc:321), so the caller searches a
// current key-frame point whose descriptor changed again for the targets that follow (include/rumi_mapping.h, DESIGN.md 4t).
//
//   k_sin_grid       one workgroup per key-frame (the current one and every target): its 64 x 48 grid from the key-points where they lie, and
//                    the key-frame's place in the call stamped on its slot (slotTag)
//   k_sin_mark       one lane per row entry.  Current key-frame: the point's observer row is walked ONCE and every target it lists gets its
//                    pair stamped "listed" in fwd, so the wide gate kernel reads one word per pair instead of scanning observers.  Targets: a
//                    point that is not bad and does not list the current key-frame claims its id with atomicMax of an integer key that
//                    orders (target, feature): the first occurrence wins whichever wave arrives first.
//   k_sin_rev_count  winners per workgroup;  k_sin_rev_scan  their exclusive scan (one workgroup);  k_sin_rev_emit  the winners in
//                    (target, feature) order by a ballot prefix, their projection into the current key-frame, survivors to the work list
//   k_sin_fwd_gate   one lane per (target, current point): the cheap gates (depth, image, distance, viewing angle: sim3_query, the arithmetic
//                    of k_queries_sim3), survivors to the work list
//   k_sin_search     16 lanes per surviving pair walk the grid window in GetFeaturesInArea order; a pair that failed a gate never gets here
// Seven launches and two memsets whatever the number of targets, all on the null stream (the store's), one blocking copy at the end.
// Integer atomics only.  The ORDER of the work list depends on arrival, the results do not: an item writes its own output word.

namespace rumi {

static_assert(sizeof(RumiKeyPoint) == 28, "k_sin_grid reads x, y seven floats apart");

struct SinKF : CovisSlotRef {          // one key-frame of a call; entry 0 is the current one
    int32_t sortedOff, slot;           // first entry of its sorted feature indices; its slot in the store
    float T[7], Ow[3], bounds[4], logSf, wInv, hInv;
    float pad[4];
};
static_assert(sizeof(SinKF) % 16 == 0, "a table entry");

enum { SIN_WORK = 0, SIN_NREV = 1, SIN_MISSING = 2, SIN_HEAD = 16 };       // the head words of the result block
constexpr int kSinListed = -2;         // fwd[t][i] while the call runs: the point lists the target (becomes -1)
constexpr int kSinLanes = 16;          // lanes per surviving pair in k_sin_search
constexpr uint32_t kSinRevBit = 0x80000000u;

struct SinArgs {
    const SinKF *tab; CovisView v;
    int nT, nCur, gx, curSlot;
    uint32_t epoch;
    float th;
    uint32_t *slotTag; unsigned long long *claim;
    const uint16_t *sorted; const int32_t *cellStart;
    int32_t *blockCount, *blockBase;
    uint4 *work;
    int32_t *head, *fwd, *revPoint, *revBest;
};

__device__ __forceinline__ unsigned long long sin_claim(const SinArgs &a, int t, int i) {
    return ((unsigned long long)a.epoch << 32) | (0x7FFFFFFFu - (((uint32_t)t << 16) | (uint32_t)i));
}

__global__ __launch_bounds__(1024) void k_sin_grid(SinArgs a, uint16_t *__restrict__ sorted, int32_t *__restrict__ cellStart) {
    const SinKF F = a.tab[blockIdx.x];
    if (threadIdx.x == 0) a.slotTag[F.slot] = (a.epoch << 10) | blockIdx.x;
    grid_build_xy<7>(F.n, reinterpret_cast<const float *>(a.v.key_frame(F).keys()), F.bounds[0], F.bounds[1], F.wInv, F.hInv,
                     sorted + F.sortedOff, cellStart + (size_t)blockIdx.x * (kGridCells + 1));
}

__global__ __launch_bounds__(256) void k_sin_mark(SinArgs a) {
    const int k = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    const SinKF &F = a.tab[k];
    if (i >= F.n) return;
    const int p = a.v.mp_row(F)[i];
    if (p < 0) return;
    const CovisPoint P = a.v.point(p);
    if (P.bad()) return;                                     // pMP->isBad()
    const int32_t *obs = a.v.rows + P.obs_off();
    if (k == 0) {
        int listed = 0;                                      // observers are distinct slots: each target counts once
        for (int j = 0; j < P.obs_len(); j++) {
            const uint32_t tag = a.slotTag[covis_obs_slot(obs[j])];
            if ((tag >> 10) != a.epoch || (tag & 1023u) == 0) continue;
            a.fwd[(size_t)((tag & 1023u) - 1) * a.nCur + i] = kSinListed;       // pMP->IsInKeyFrame(pKFi)
            listed++;
        }
        // A point that some target would search and that has no attributes is counted HERE for the forward pass (k_sin_fwd_gate passes such
        // pairs over in silence: keep the two in step), and the call is refused.  Its id is claimed above every reverse claim, so that a
        // store whose observer row does not (yet) list the current slot cannot have k_sin_rev_emit count the same point again.
        if (listed < a.nT && !a.v.has_attr(P)) {
            atomicAdd(&a.head[SIN_MISSING], 1);
            atomicMax(&a.claim[p], ((unsigned long long)a.epoch << 32) | 0xFFFFFFFFull);
        }
    } else {
        bool inCur = false;                                  // pMP->IsInKeyFrame(mpCurrentKeyFrame), ORBmatcher.cc:1054 in the reverse pass
        for (int j = 0; j < P.obs_len(); j++) inCur = inCur || covis_obs_slot(obs[j]) == a.curSlot;
        if (!inCur) atomicMax(&a.claim[p], sin_claim(a, k - 1, i));
    }
}

// Does entry i of target t's row hold the first occurrence of a reverse candidate?  (Only a claim of this call carries this epoch.)
__device__ __forceinline__ int sin_winner(const SinArgs &a, int t, int i) {
    const SinKF &F = a.tab[1 + t];
    if (i >= F.n) return -1;
    const int p = a.v.mp_row(F)[i];
    return p >= 0 && a.claim[p] == sin_claim(a, t, i) ? p : -1;
}

__global__ __launch_bounds__(256) void k_sin_rev_count(SinArgs a) {
    __shared__ int sWave[4];
    const int p = sin_winner(a, blockIdx.y, blockIdx.x * 256 + threadIdx.x);
    const unsigned long long b = __ballot(p >= 0);
    if ((threadIdx.x & 63) == 0) sWave[threadIdx.x >> 6] = __popcll(b);
    __syncthreads();
    if (threadIdx.x == 0) a.blockCount[blockIdx.y * a.gx + blockIdx.x] = (sWave[0] + sWave[1]) + (sWave[2] + sWave[3]);
}

__global__ __launch_bounds__(1024) void k_sin_rev_scan(SinArgs a, int nBlocks) {
    __shared__ int sWave[16];
    const int tid = threadIdx.x, chunk = (nBlocks + 1023) / 1024;
    int s = 0;
    for (int k = 0; k < chunk; k++) { const int i = tid * chunk + k; if (i < nBlocks) s += a.blockCount[i]; }
    const int incl = wave_scan_incl_i32(s);
    if ((tid & 63) == 63) sWave[tid >> 6] = incl;
    __syncthreads();
    int before = 0, total = 0;
#pragma unroll
    for (int w = 0; w < 16; w++) { const int t = sWave[w]; total += t; if (w < (tid >> 6)) before += t; }
    int run = before + incl - s;
    for (int k = 0; k < chunk; k++) { const int i = tid * chunk + k; if (i < nBlocks) { a.blockBase[i] = run; run += a.blockCount[i]; } }
    if (tid == 0) a.head[SIN_NREV] = total;
}

// One item of the work list: a pair that passed every gate.  u, v: the projection; z: where the result goes (fwd index, or kSinRevBit | place
// in the reverse list); w: the predicted level.  The radius is th * scale[level] again in the search, the expression sim3_query uses.
__device__ __forceinline__ void sin_push(const SinArgs &a, bool valid, const Query &q, uint32_t where) {
    const unsigned long long b = __ballot(valid);
    if (!b) return;
    const int lane = threadIdx.x & 63, leader = __builtin_ctzll(b);
    int base = 0;
    if (lane == leader) base = atomicAdd(&a.head[SIN_WORK], __popcll(b));
    base = __builtin_amdgcn_readlane(base, leader);
    if (valid) a.work[base + __popcll(b & ((1ull << lane) - 1ull))] = make_uint4(__float_as_uint(q.u), __float_as_uint(q.v), where, (uint32_t)q.maxLevel);
}

__device__ __forceinline__ Query sin_query(const SinArgs &a, int k, int p) {
    const SinKF &F = a.tab[k];
    const CovisKeyFrame K = a.v.key_frame(F);
    const CovisAttrGeom A = a.v.attr_geom(p);
    float pos[3], nrm[3];
    A.pos(pos); A.normal(nrm);
    return sim3_query(pos, nrm, A.min_dist(), A.max_dist(), F.T, K.K(), F.Ow, K.scale(), K.nlevels(), F.logSf, a.th, 0, F.bounds[0], F.bounds[1], F.bounds[2],
                      F.bounds[3]);
}

__global__ __launch_bounds__(256) void k_sin_rev_emit(SinArgs a) {
    __shared__ int sWave[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int p = sin_winner(a, blockIdx.y, blockIdx.x * 256 + threadIdx.x);
    const unsigned long long b = __ballot(p >= 0);
    if (lane == 0) sWave[wave] = __popcll(b);
    __syncthreads();
    int j = a.blockBase[blockIdx.y * a.gx + blockIdx.x] + __popcll(b & ((1ull << lane) - 1ull));
    for (int w = 0; w < wave; w++) j += sWave[w];
    Query q{};
    if (p >= 0) {
        a.revPoint[j] = p; a.revBest[j] = -1;
        if (a.v.has_attr(p)) q = sin_query(a, 0, p);
        else atomicAdd(&a.head[SIN_MISSING], 1);
    }
    sin_push(a, q.valid != 0, q, kSinRevBit | (uint32_t)j);
}

__global__ __launch_bounds__(256) void k_sin_fwd_gate(SinArgs a) {
    const int t = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    Query q{};
    size_t at = 0;
    if (i < a.nCur) {
        at = (size_t)t * a.nCur + i;
        const int p = a.v.mp_row(a.tab[0])[i];
        if (a.fwd[at] == kSinListed) a.fwd[at] = -1;
        else if (p >= 0) {
            const CovisPoint P = a.v.point(p);
            if (!P.bad() && a.v.has_attr(P)) q = sin_query(a, 1 + t, p);
        }
    }
    sin_push(a, q.valid != 0, q, (uint32_t)at);
}

// The window walk of one work item, kSinLanes lanes each (walk_window, match_grid.h): the candidates of Frame::GetFeaturesInArea (Frame.cc:695-750)
// in its order, the level window [level - 1, level] and the strict `dist < bestDist`: the key (distance << 16 | place in the walk) has one
// minimum, the earliest of the nearest.  REPROJ: the monocular reprojection gate (5.99) of ORBmatcher.cc:1138-1145 (reproj_gate, the one
// candidates_walk applies in MODE_FUSE), which Fuse(KF, MapPoints) has and Fuse(KF, Scw, MapPoints) (:1258-1274, search_and_fuse.inc) has not.
// One body for k_sin_search and k_saf_search.
template <bool REPROJ>
__device__ __forceinline__ void sin_walk(const SinArgs &a, int k, int p, const uint4 &item, int sub, uint32_t &bestKey, int &bestIdx) {
    const SinKF &F = a.tab[k];
    const CovisKeyFrame K = a.v.key_frame(F);
    const uint8_t *desc = K.desc();
    const float *scale = K.scale();
    const GridView G{K.keys(), a.sorted + F.sortedOff, a.cellStart + (size_t)k * (kGridCells + 1), F.bounds[0], F.bounds[1], F.wInv, F.hInv};
    uint4 q0, q1;
    a.v.attr_desc(p, q0, q1);
    const float u = __uint_as_float(item.x), v = __uint_as_float(item.y);
    const int maxLevel = (int)item.w;
    walk_window<kSinLanes>(G, u, v, a.th * scale[maxLevel], maxLevel - 1, maxLevel, sub, [&](int idx, const RumiKeyPoint &kp, int place) {
        if (REPROJ && !reproj_gate(kp, u, v, scale)) return;
        const int d = hamming256(q0, q1, ld16_dword(desc + (size_t)idx * 32), ld16_dword(desc + (size_t)idx * 32 + 16));
        const uint32_t key = ((uint32_t)d << 16) | (uint32_t)place;
        if (key < bestKey) { bestKey = key; bestIdx = idx; }
    });
}

// The minimum of a group's kSinLanes keys; all 64 lanes are here, a group's lanes exchange among themselves only.
__device__ __forceinline__ void sin_group_min(uint32_t &bestKey, int &bestIdx) {
#pragma unroll
    for (int m = 1; m < kSinLanes; m <<= 1) {
        const uint32_t ok = (uint32_t)__shfl_xor((int)bestKey, m);
        const int oi = __shfl_xor(bestIdx, m);
        if (ok < bestKey) { bestKey = ok; bestIdx = oi; }
    }
}

// ORBmatcher.cc:1114-1161 for the pairs of the work list: sin_walk with the reprojection gate.
__global__ __launch_bounds__(256) void k_sin_search(SinArgs a) {
    const int sub = threadIdx.x & (kSinLanes - 1), perBlock = 256 / kSinLanes;
    const int count = a.head[SIN_WORK];
    for (int w0 = blockIdx.x * perBlock; w0 < count; w0 += gridDim.x * perBlock) {
        const int w = w0 + (threadIdx.x / kSinLanes);
        uint32_t bestKey = 0xFFFFFFFFu;
        int bestIdx = -1;
        int32_t *out = nullptr;
        if (w < count) {
            const uint4 item = a.work[w];
            int k, p;
            if (item.z & kSinRevBit) { const int j = (int)(item.z & ~kSinRevBit); k = 0; p = a.revPoint[j]; out = a.revBest + j; }
            else { const int t = (int)(item.z / (uint32_t)a.nCur), i = (int)(item.z - (uint32_t)t * (uint32_t)a.nCur); k = 1 + t; p = a.v.mp_row(a.tab[0])[i]; out = a.fwd + item.z; }
            sin_walk<true>(a, k, p, item, sub, bestKey, bestIdx);
        }
        sin_group_min(bestKey, bestIdx);
        if (out && sub == 0) *out = (int)(bestKey >> 16) <= RUMI_TH_LOW ? bestIdx : -1;      // :1161; no candidate: 0xFFFF
    }
}

// ---- host -------------------------------------------------------------------------------------------------------------------------------
}  // namespace rumi

// The RumiFuseKF of a call, k = 0 .. n - 1 through at(k): every float finite, then image bounds that are not empty.  What is wrong, or nullptr.
template <class At> static const char *fuse_kfs_check(int n, At at) {
    for (int k = 0; k < n; k++) {
        const float *f = reinterpret_cast<const float *>(&at(k));
        for (size_t i = 0; i < sizeof(RumiFuseKF) / 4; i++) if (!std::isfinite(f[i])) return "a pose, camera centre, bound or scale factor that is not finite";
    }
    for (int k = 0; k < n; k++) {
        const RumiFuseKF &P = at(k);
        if (!(P.bounds[2] > P.bounds[0]) || !(P.bounds[3] > P.bounds[1])) return "empty image bounds";
    }
    return nullptr;
}

// The grid entry of a key-frame: its slot record, its bounds and the cell sizes as upload_frame forms them (Frame.cc:322-323); the rest zero.
static void sin_kf_grid(rumi::SinKF *R, const rumi::CovisSlotRef &ref, int32_t slot, const float *bounds, int32_t sortedOff) {
    std::memset(R, 0, sizeof *R);
    static_cast<rumi::CovisSlotRef &>(*R) = ref; R->sortedOff = sortedOff; R->slot = slot;
    std::memcpy(R->bounds, bounds, 16);
    R->wInv = (float)rumi::kGridCols / (float)(bounds[2] - bounds[0]);
    R->hInv = (float)rumi::kGridRows / (float)(bounds[3] - bounds[1]);
}
// ... and the pose it is searched under (SearchInNeighbors, SearchAndFuse; a Sim3 projection job carries its own).
static void sin_kf_pose(rumi::SinKF *R, const RumiFuseKF &P) {
    std::memcpy(R->T, P.Tcw7, 28); std::memcpy(R->Ow, P.Ow, 12);
    R->logSf = P.log_scale_factor;
}

// The two stamped tables: a value of another epoch reads as "not of this call"; a new or outgrown table, or a wrapped epoch, starts from zero.
// Shared with rumi_search_and_fuse_resident (search_and_fuse.inc), whose calls take their epochs from the same counter.
static int sin_next_epoch(rumi::SinState *s, const rumi::CovisView &fv) {
    int rc;
    const bool fresh = (size_t)fv.maxKf > s->slotTag.cap || (size_t)fv.maxPoints > s->claim.cap || s->epoch >= (1u << 22) - 1;
    if ((rc = s->slotTag.reserve((size_t)fv.maxKf, (size_t)fv.maxKf)) != RUMI_OK || (rc = s->claim.reserve((size_t)fv.maxPoints, (size_t)fv.maxPoints)) != RUMI_OK) return rc;
    if (fresh) {
        HIP_TRY(hipMemsetAsync(s->slotTag.p, 0, s->slotTag.cap * sizeof(uint32_t), nullptr));
        HIP_TRY(hipMemsetAsync(s->claim.p, 0, s->claim.cap * sizeof(unsigned long long), nullptr));
        s->epoch = 0;
    }
    s->epoch++;
    return RUMI_OK;
}

extern "C" int rumi_search_in_neighbors_resident(RumiMatcher *m, RumiCovis *c, int32_t cur_slot, const RumiFuseKF *cur, const int32_t *target_slots,
                                                 const RumiFuseKF *targets, int32_t n_targets, float th, int32_t *fwd_best, int32_t *rev_point,
                                                 int32_t *rev_best, int32_t rev_cap, int32_t *n_rev) {
    static const char *entry = "rumi_search_in_neighbors_resident";
    if (!m || !c || !cur || !n_rev || n_targets < 0 || rev_cap < 0 || (rev_cap > 0 && (!rev_point || !rev_best)) ||
        (n_targets > 0 && (!target_slots || !targets || !fwd_best))) {
        g_lastError = std::string(entry) + ": missing argument, or a negative count";
        return RUMI_E_INVALID;
    }
    if (n_targets > RUMI_FUSE_MAX_TARGETS) {
        g_lastError = std::string(entry) + ": more than RUMI_FUSE_MAX_TARGETS target key-frames";
        return RUMI_E_CAPACITY;
    }
    const auto t0 = std::chrono::steady_clock::now();
    if (!(th > 0.f) || !std::isfinite(th)) { g_lastError = std::string(entry) + ": th must be positive"; return RUMI_E_INVALID; }
    const auto kfAt = [&](int k) -> const RumiFuseKF & { return k ? targets[k - 1] : *cur; };
    if (const char *why = fuse_kfs_check(n_targets + 1, kfAt)) { g_lastError = std::string(entry) + ": " + why; return RUMI_E_INVALID; }
    std::vector<int32_t> slots((size_t)n_targets + 1);
    std::vector<CovisSlotFeatures> info((size_t)n_targets + 1);
    slots[0] = cur_slot;
    for (int k = 0; k < n_targets; k++) slots[1 + k] = target_slots[k];
    int rc;
    // everything the host alone can refuse is refused before the matcher handle is read: the slots first, then the device both live on
    if ((rc = covis_features_check(c, n_targets + 1, slots.data(), entry, info.data())) != RUMI_OK) return rc;
    if (n_targets > 0 && (rc = covis_same_device(c, m->device, entry)) != RUMI_OK) return rc;
    size_t E = 0, feats = 0;
    int maxN = 1;
    for (int k = 0; k <= n_targets; k++) {
        if (info[k].n > m->maxFeat) { g_lastError = "SearchInNeighbors: a key-frame exceeds the matcher's max_features"; return RUMI_E_CAPACITY; }
        feats += (size_t)info[k].n; maxN = std::max(maxN, info[k].n);
        if (k) E += (size_t)info[k].n;
    }
    if (n_targets == 0) { *n_rev = 0; return RUMI_OK; }
    const int nCur = info[0].n;
    const size_t pairs = (size_t)n_targets * nCur;
    if (pairs >= kSinRevBit || E >= kSinRevBit) { g_lastError = "SearchInNeighbors: more pairs than a work item addresses"; return RUMI_E_CAPACITY; }
    HIP_TRY(hipSetDevice(m->device));
    SinState *s = made(newpts_state(m)->sin);
    s->clock.start(); s->clock.t[0] = t0;

    const size_t tabBytes = (size_t)(n_targets + 1) * sizeof(SinKF), resWords = SIN_HEAD + pairs + 2 * E;
    const int gx = (maxN + 255) / 256, nBlocks = gx * n_targets;
    if ((rc = s->tab.reserve(tabBytes, tabBytes + tabBytes / 2)) != RUMI_OK || (rc = s->res.reserve(resWords, resWords + resWords / 4)) != RUMI_OK ||
        (rc = s->sorted.reserve(feats + 1, feats + feats / 4 + 1)) != RUMI_OK ||
        (rc = s->cellStart.reserve((size_t)(n_targets + 1) * (kGridCells + 1), (size_t)(n_targets + 1) * (kGridCells + 1))) != RUMI_OK ||
        (rc = s->blocks.reserve(2 * (size_t)nBlocks, 2 * (size_t)nBlocks)) != RUMI_OK || (rc = s->work.reserve(pairs + E + 1, pairs + E + (pairs + E) / 4 + 1)) != RUMI_OK)
        return rc;
    CovisView fv;
    s->clock.mark();
    if ((rc = covis_view(c, 0, &fv)) != RUMI_OK) return rc;
    if ((rc = sin_next_epoch(s, fv)) != RUMI_OK) return rc;

    SinKF *tab = reinterpret_cast<SinKF *>(s->tab.h);
    int32_t sortedOff = 0;
    for (int k = 0; k <= n_targets; k++) {
        sin_kf_grid(&tab[k], covis_slot_ref(info[k]), slots[k], kfAt(k).bounds, sortedOff);
        sin_kf_pose(&tab[k], kfAt(k));
        sortedOff += info[k].n;
    }
    HIP_TRY(hipMemcpyAsync(s->tab.d, s->tab.h, tabBytes, hipMemcpyHostToDevice, nullptr));
    int32_t *dRes = s->res.d;
    HIP_TRY(hipMemsetAsync(dRes, 0, SIN_HEAD * 4, nullptr));
    if (pairs) HIP_TRY(hipMemsetAsync(dRes + SIN_HEAD, 0xFF, pairs * 4, nullptr));
    SinArgs a{};
    a.tab = reinterpret_cast<const SinKF *>(s->tab.d); a.v = fv;
    a.nT = n_targets; a.nCur = nCur; a.gx = gx; a.curSlot = cur_slot; a.epoch = s->epoch; a.th = th;
    a.slotTag = s->slotTag.p; a.claim = s->claim.p; a.sorted = s->sorted.p; a.cellStart = s->cellStart.p;
    a.blockCount = s->blocks.p; a.blockBase = s->blocks.p + nBlocks; a.work = s->work.p;
    a.head = dRes; a.fwd = dRes + SIN_HEAD; a.revPoint = a.fwd + pairs; a.revBest = a.revPoint + E;
    hipLaunchKernelGGL(k_sin_grid, dim3(n_targets + 1), dim3(1024), 0, nullptr, a, s->sorted.p, s->cellStart.p);
    hipLaunchKernelGGL(k_sin_mark, dim3(gx, n_targets + 1), dim3(256), 0, nullptr, a);
    hipLaunchKernelGGL(k_sin_rev_count, dim3(gx, n_targets), dim3(256), 0, nullptr, a);
    hipLaunchKernelGGL(k_sin_rev_scan, dim3(1), dim3(1024), 0, nullptr, a, nBlocks);
    hipLaunchKernelGGL(k_sin_rev_emit, dim3(gx, n_targets), dim3(256), 0, nullptr, a);
    if (nCur > 0) hipLaunchKernelGGL(k_sin_fwd_gate, dim3((nCur + 255) / 256, n_targets), dim3(256), 0, nullptr, a);
    const int searchBlocks = (int)std::min<size_t>(2048, (pairs + E + 15) / 16 + 1);
    hipLaunchKernelGGL(k_sin_search, dim3(searchBlocks), dim3(256), 0, nullptr, a);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(s->res.h, dRes, resWords * 4, hipMemcpyDeviceToHost));      // one block back; the call's one synchronisation
    s->clock.mark();
    const int32_t *h = s->res.h;
    if (h[SIN_MISSING]) {
        s->clock.finish(s->stageMs);
        g_lastError = std::string(entry) + ": " + std::to_string(h[SIN_MISSING]) + " searched map point(s) without attributes (rumi_covis_set_point_attributes)";
        return RUMI_E_INVALID;
    }
    const int nRev = h[SIN_NREV], wr = std::min(nRev, rev_cap);
    *n_rev = nRev;
    if (pairs) std::memcpy(fwd_best, h + SIN_HEAD, pairs * 4);
    if (wr > 0) { std::memcpy(rev_point, h + SIN_HEAD + pairs, (size_t)wr * 4); std::memcpy(rev_best, h + SIN_HEAD + pairs + E, (size_t)wr * 4); }
    s->clock.finish(s->stageMs);
    if (nRev > rev_cap) {
        g_lastError = "SearchInNeighbors: more reverse candidates than the output lists hold (rev_cap)";
        return RUMI_E_CAPACITY;
    }
    return RUMI_OK;
}

extern "C" int rumi_search_in_neighbors_stage_ms(const RumiMatcher *m, float *out3) {
    if (!out3 || !newpts_peek(m) || !newpts_peek(m)->sin) {
        g_lastError = "rumi_search_in_neighbors_stage_ms: no SearchInNeighbors call precedes on this matcher";
        return RUMI_E_INVALID;
    }
    std::memcpy(out3, newpts_peek(m)->sin->stageMs, 12);
    return RUMI_OK;
}
