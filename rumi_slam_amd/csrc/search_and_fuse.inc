// The searches of LoopClosing::SearchAndFuse (R/lib_src/LoopClosing.cc:1996-2065) for every corrected key-frame in one call, behind
// rumi_search_and_fuse_resident (include/rumi_mapping.h).  Included at the end of mapping.hip after search_in_neighbors.inc, whose table entry
// (SinKF), arguments (SinArgs), grid kernel, query, work list, scan and window walk it uses as they are.
//
// What the device computes is the search of ORBmatcher::Fuse(pKF, Scw, vpPoints, th, vpReplacePoint) (ORBmatcher.cc:1182-1291) on the map as
// it stands at the call: bestIdx of every (key-frame, list entry) pair.  Against the SearchInNeighbors entry the queries are a list of point
// ids instead of a key-frame's row, every key-frame is searched under the pose the caller derived from its corrected Sim3, the walk has no
// reprojection gate (:1258-1274), and the answer is sparse: the pairs that found a feature, in (key-frame, entry) order.
//
//   k_sin_grid    (search_in_neighbors.inc) one workgroup per key-frame: its 64 x 48 grid, and its place in the call stamped on its slot
//   k_saf_mark    one lane per list entry: the point record is read once, the observer row is walked once, and every key-frame of the call it
//                 lists gets its pair stamped "listed" in the dense matrix; an entry with a live pair left and no attributes is counted
//   k_saf_gate    one lane per (key-frame, entry) pair, entries the fast index: a wave's lanes share the key-frame (its table entry and feature
//                 header are scalar loads) and read consecutive ids; the cheap gates (sim3_query), survivors to the work list
//   k_saf_search  16 lanes per surviving pair: sin_walk<false>; the winner lane writes the pair's word of the dense matrix
//   k_saf_count   hits per workgroup of the dense matrix;  k_sin_rev_scan  their exclusive scan;  k_saf_emit  the hits in (key-frame, entry)
//                 order by a ballot prefix, each with the occupant of its feature from the row arena, and the hits per key-frame from the
//                 block bases
// Seven launches and two memsets whatever the number of key-frames, all on the null stream (the store's).  Integer atomics only; the order of
// the work list depends on arrival, the results do not.  The dense matrix never leaves the device.

namespace rumi {

static_assert(sizeof(RumiFuseHit) == 16, "k_saf_emit writes a hit as one int4");

struct SafArgs {
    SinArgs s;                         // nT: key-frames of the call, nCur: list entries, fwd: the dense matrix [nT][nCur], tab[k]: key-frame k
    const int32_t *ids;                // [nCur] the list
    int4 *hits; int32_t *perKf;        // [hitCap], [nT]
    int hitCap;
};

__global__ __launch_bounds__(256) void k_saf_mark(SafArgs a) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= a.s.nCur) return;
    const int p = a.ids[i];
    if (p < 0) return;
    const CovisPoint P = a.s.v.point(p);
    if (P.bad()) return;                                     // pMP->isBad()
    const int32_t *obs = a.s.v.rows + P.obs_off();
    int listed = 0;                                          // observers are distinct slots: each key-frame counts once
    for (int j = 0; j < P.obs_len(); j++) {
        const uint32_t tag = a.s.slotTag[covis_obs_slot(obs[j])];
        if ((tag >> 10) != a.s.epoch) continue;
        a.s.fwd[(size_t)(tag & 1023u) * a.s.nCur + i] = kSinListed;            // spAlreadyFound.count(pMP), ORBmatcher.cc:1205
        listed++;
    }
    // counted HERE for the whole call; k_saf_gate passes such pairs over in silence: keep the two in step
    if (listed < a.s.nT && !a.s.v.has_attr(P)) atomicAdd(&a.s.head[SIN_MISSING], 1);
}

__global__ __launch_bounds__(256) void k_saf_gate(SafArgs a) {
    const int k = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    Query q{};
    size_t at = 0;
    if (i < a.s.nCur) {
        at = (size_t)k * a.s.nCur + i;
        const int p = a.ids[i];
        if (a.s.fwd[at] == kSinListed) a.s.fwd[at] = -1;
        else if (p >= 0) {
            const CovisPoint P = a.s.v.point(p);
            if (!P.bad() && a.s.v.has_attr(P)) q = sin_query(a.s, k, p);
        }
    }
    sin_push(a.s, q.valid != 0, q, (uint32_t)at);
}

// ORBmatcher.cc:1246-1277 for the pairs of the work list: sin_walk without the reprojection gate.
__global__ __launch_bounds__(256) void k_saf_search(SafArgs a) {
    const int sub = threadIdx.x & (kSinLanes - 1), perBlock = 256 / kSinLanes;
    const int count = a.s.head[SIN_WORK];
    for (int w0 = blockIdx.x * perBlock; w0 < count; w0 += gridDim.x * perBlock) {
        const int w = w0 + (threadIdx.x / kSinLanes);
        uint32_t bestKey = 0xFFFFFFFFu;
        int bestIdx = -1;
        int32_t *out = nullptr;
        if (w < count) {
            const uint4 item = a.s.work[w];
            const int k = (int)(item.z / (uint32_t)a.s.nCur), i = (int)(item.z - (uint32_t)k * (uint32_t)a.s.nCur);
            out = a.s.fwd + item.z;
            sin_walk<false>(a.s, k, a.ids[i], item, sub, bestKey, bestIdx);
        }
        sin_group_min(bestKey, bestIdx);
        if (out && sub == 0) *out = (int)(bestKey >> 16) <= RUMI_TH_LOW ? bestIdx : -1;      // :1277; no candidate: 0xFFFF
    }
}

__device__ __forceinline__ int saf_hit(const SafArgs &a, int k, int i) { return i < a.s.nCur ? a.s.fwd[(size_t)k * a.s.nCur + i] : -1; }

__global__ __launch_bounds__(256) void k_saf_count(SafArgs a) {
    __shared__ int sWave[4];
    const unsigned long long b = __ballot(saf_hit(a, blockIdx.y, blockIdx.x * 256 + threadIdx.x) >= 0);
    if ((threadIdx.x & 63) == 0) sWave[threadIdx.x >> 6] = __popcll(b);
    __syncthreads();
    if (threadIdx.x == 0) a.s.blockCount[blockIdx.y * a.s.gx + blockIdx.x] = (sWave[0] + sWave[1]) + (sWave[2] + sWave[3]);
}

__global__ __launch_bounds__(256) void k_saf_emit(SafArgs a) {
    __shared__ int sWave[4];
    const int k = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int f = saf_hit(a, k, i);
    const unsigned long long b = __ballot(f >= 0);
    if (lane == 0) sWave[wave] = __popcll(b);
    __syncthreads();
    const int first = a.s.blockBase[k * a.s.gx];             // the key-frame's blocks are consecutive in the scan
    int j = a.s.blockBase[k * a.s.gx + blockIdx.x] + __popcll(b & ((1ull << lane) - 1ull));
    for (int w = 0; w < wave; w++) j += sWave[w];
    if (f >= 0 && j < a.hitCap) a.hits[j] = make_int4(k, i, f, a.s.v.mp_row(a.s.tab[k])[f]);      // pKF->GetMapPoint(bestIdx) at the call
    if (blockIdx.x == 0 && threadIdx.x == 0) a.perKf[k] = (k + 1 < a.s.nT ? a.s.blockBase[(k + 1) * a.s.gx] : a.s.head[SIN_NREV]) - first;
}

// ---- host -------------------------------------------------------------------------------------------------------------------------------
constexpr int kSafFirstHits = 2048;                          // hits that travel with the head; more take a second copy

}  // namespace rumi

extern "C" int rumi_search_and_fuse_resident(RumiMatcher *m, RumiCovis *c, const int32_t *kf_slots, const RumiFuseKF *kfs, int32_t n_kfs,
                                             const int32_t *point_ids, int32_t n_points, float th, RumiFuseHit *hits, int32_t hit_cap,
                                             int32_t *n_hits, int32_t *per_kf) {
    static const char *entry = "rumi_search_and_fuse_resident";
    if (!m || !c || !n_hits || n_kfs < 0 || n_points < 0 || hit_cap < 0 || (hit_cap > 0 && !hits) || (n_kfs > 0 && (!kf_slots || !kfs || !per_kf)) ||
        (n_points > 0 && !point_ids)) {
        g_lastError = std::string(entry) + ": missing argument, or a negative count";
        return RUMI_E_INVALID;
    }
    if (n_kfs > RUMI_FUSE_MAX_TARGETS) {
        g_lastError = std::string(entry) + ": more than RUMI_FUSE_MAX_TARGETS key-frames";
        return RUMI_E_CAPACITY;
    }
    const size_t pairs = (size_t)n_kfs * (size_t)n_points;
    if (pairs >= kSinRevBit) { g_lastError = std::string(entry) + ": more pairs than a work item addresses"; return RUMI_E_CAPACITY; }
    const auto t0 = std::chrono::steady_clock::now();
    if (!(th > 0.f) || !std::isfinite(th)) { g_lastError = std::string(entry) + ": th must be positive"; return RUMI_E_INVALID; }
    if (const char *why = fuse_kfs_check(n_kfs, [&](int k) -> const RumiFuseKF & { return kfs[k]; })) { g_lastError = std::string(entry) + ": " + why; return RUMI_E_INVALID; }
    std::vector<CovisSlotFeatures> info((size_t)n_kfs);
    const bool work = n_kfs > 0 && n_points > 0;
    int rc;
    // everything the host alone can refuse is refused before the matcher handle is read: the slots first, then the device both live on
    if ((rc = covis_features_check(c, n_kfs, kf_slots, entry, info.data())) != RUMI_OK) return rc;
    if (work && (rc = covis_same_device(c, m->device, entry)) != RUMI_OK) return rc;
    size_t feats = 0;
    for (int k = 0; k < n_kfs; k++) {
        if (info[k].n > m->maxFeat) { g_lastError = std::string(entry) + ": a key-frame exceeds the matcher's max_features"; return RUMI_E_CAPACITY; }
        feats += (size_t)info[k].n;
    }
    if (!work) {
        *n_hits = 0;
        for (int k = 0; k < n_kfs; k++) per_kf[k] = 0;
        return RUMI_OK;
    }
    HIP_TRY(hipSetDevice(m->device));
    NewPtsState *np = newpts_state(m);
    SinState *sin = made(np->sin);                           // the stamped tables and their epoch
    SafState *s = made(np->saf);
    s->clock.start(); s->clock.t[0] = t0;

    const size_t tabBytes = (size_t)n_kfs * sizeof(SinKF), upBytes = tabBytes + (size_t)n_points * 4;
    const size_t headWords = SIN_HEAD + (((size_t)n_kfs + 3) & ~(size_t)3);             // the hits are written as int4: 16-byte aligned behind per_kf
    const size_t hitDev = std::min<size_t>((size_t)hit_cap, pairs), resWords = headWords + 4 * hitDev;
    const int gx = (n_points + 255) / 256, nBlocks = gx * n_kfs;
    if ((rc = s->up.reserve(upBytes, upBytes + upBytes / 2)) != RUMI_OK || (rc = s->res.reserve(resWords, resWords + resWords / 4)) != RUMI_OK ||
        (rc = s->dense.reserve(pairs, pairs + pairs / 4)) != RUMI_OK || (rc = s->sorted.reserve(feats + 1, feats + feats / 4 + 1)) != RUMI_OK ||
        (rc = s->cellStart.reserve((size_t)n_kfs * (kGridCells + 1), (size_t)n_kfs * (kGridCells + 1))) != RUMI_OK ||
        (rc = s->blocks.reserve(2 * (size_t)nBlocks, 2 * (size_t)nBlocks)) != RUMI_OK || (rc = s->work.reserve(pairs + 1, pairs + pairs / 4 + 1)) != RUMI_OK)
        return rc;
    CovisView fv;
    s->clock.mark();
    if ((rc = covis_view(c, 0, &fv)) != RUMI_OK) return rc;
    for (int i = 0; i < n_points; i++)
        if (point_ids[i] >= fv.maxPoints) { g_lastError = std::string(entry) + ": a point id at or above the store's point capacity"; return RUMI_E_INVALID; }
    if ((rc = sin_next_epoch(sin, fv)) != RUMI_OK) return rc;

    SinKF *tab = reinterpret_cast<SinKF *>(s->up.h);
    int32_t sortedOff = 0;
    for (int k = 0; k < n_kfs; k++) {
        sin_kf_grid(&tab[k], covis_slot_ref(info[k]), kf_slots[k], kfs[k].bounds, sortedOff);
        sin_kf_pose(&tab[k], kfs[k]);
        sortedOff += info[k].n;
    }
    std::memcpy(s->up.h + tabBytes, point_ids, (size_t)n_points * 4);
    HIP_TRY(hipMemcpyAsync(s->up.d, s->up.h, upBytes, hipMemcpyHostToDevice, nullptr));
    int32_t *dRes = s->res.d;
    HIP_TRY(hipMemsetAsync(dRes, 0, SIN_HEAD * 4, nullptr));
    HIP_TRY(hipMemsetAsync(s->dense.p, 0xFF, pairs * 4, nullptr));
    SafArgs a{};
    a.s.tab = reinterpret_cast<const SinKF *>(s->up.d); a.s.v = fv;
    a.s.nT = n_kfs; a.s.nCur = n_points; a.s.gx = gx; a.s.curSlot = -1; a.s.epoch = sin->epoch; a.s.th = th;
    a.s.slotTag = sin->slotTag.p; a.s.claim = sin->claim.p; a.s.sorted = s->sorted.p; a.s.cellStart = s->cellStart.p;
    a.s.blockCount = s->blocks.p; a.s.blockBase = s->blocks.p + nBlocks; a.s.work = s->work.p;
    a.s.head = dRes; a.s.fwd = s->dense.p;
    a.ids = reinterpret_cast<const int32_t *>(s->up.d + tabBytes);
    static_assert(SIN_HEAD % 4 == 0, "the hits follow the head and per_kf");
    a.perKf = dRes + SIN_HEAD; a.hits = reinterpret_cast<int4 *>(dRes + headWords); a.hitCap = (int)hitDev;
    hipLaunchKernelGGL(k_sin_grid, dim3(n_kfs), dim3(1024), 0, nullptr, a.s, s->sorted.p, s->cellStart.p);
    hipLaunchKernelGGL(k_saf_mark, dim3(gx), dim3(256), 0, nullptr, a);
    hipLaunchKernelGGL(k_saf_gate, dim3(gx, n_kfs), dim3(256), 0, nullptr, a);
    const int searchBlocks = (int)std::min<size_t>(2048, (pairs + 15) / 16 + 1);
    hipLaunchKernelGGL(k_saf_search, dim3(searchBlocks), dim3(256), 0, nullptr, a);
    hipLaunchKernelGGL(k_saf_count, dim3(gx, n_kfs), dim3(256), 0, nullptr, a);
    hipLaunchKernelGGL(k_sin_rev_scan, dim3(1), dim3(1024), 0, nullptr, a.s, nBlocks);
    hipLaunchKernelGGL(k_saf_emit, dim3(gx, n_kfs), dim3(256), 0, nullptr, a);
    HIP_TRY(hipGetLastError());
    // The head, per_kf and the first hits in one blocking copy, the call's one synchronisation unless more than kSafFirstHits hits are wanted.
    const size_t firstHits = std::min<size_t>(hitDev, kSafFirstHits);
    HIP_TRY(hipMemcpy(s->res.h, dRes, (headWords + 4 * firstHits) * 4, hipMemcpyDeviceToHost));
    const int32_t *h = s->res.h;
    const int total = h[SIN_NREV];
    const size_t wr = std::min<size_t>((size_t)total, hitDev);
    if (!h[SIN_MISSING] && wr > firstHits)
        HIP_TRY(hipMemcpy(s->res.h + headWords + 4 * firstHits, dRes + headWords + 4 * firstHits, (wr - firstHits) * 16, hipMemcpyDeviceToHost));
    s->clock.mark();
    if (h[SIN_MISSING]) {
        s->clock.finish(s->stageMs);
        g_lastError = std::string(entry) + ": " + std::to_string(h[SIN_MISSING]) + " searched list entries whose map point has no attributes (rumi_covis_set_point_attributes)";
        return RUMI_E_INVALID;
    }
    *n_hits = total;
    std::memcpy(per_kf, h + SIN_HEAD, (size_t)n_kfs * 4);
    if (wr > 0) std::memcpy(hits, h + headWords, wr * 16);
    s->clock.finish(s->stageMs);
    if (total > hit_cap) {
        g_lastError = std::string(entry) + ": more hits than the output list holds (hit_cap)";
        return RUMI_E_CAPACITY;
    }
    return RUMI_OK;
}

extern "C" int rumi_search_and_fuse_stage_ms(const RumiMatcher *m, float *out3) {
    if (!out3 || !newpts_peek(m) || !newpts_peek(m)->saf) {
        g_lastError = "rumi_search_and_fuse_stage_ms: no SearchAndFuse call precedes on this matcher";
        return RUMI_E_INVALID;
    }
    std::memcpy(out3, newpts_peek(m)->saf->stageMs, 12);
    return RUMI_OK;
}
