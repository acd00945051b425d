// ORBmatcher::SearchByProjection(KeyFrame*, Sim3f&, points, ...) (R/lib_src/ORBmatcher.cc:372-471, :473-579) for every job of a place-recognition
// stage in one call, behind rumi_search_by_projection_sim3_resident (include/rumi_mapping.h).  Included at the end of mapping.hip after
// search_and_fuse.inc; the grid kernel, the table entry it reads (SinKF), the work list (sin_push) and the stamped
// slot table are search_in_neighbors.inc's, the gate is sim3_query (match_device.h).
//
// A job is one call of the member: a key-frame (by slot), a pose, a list of point ids (a range of the call's id array), th, the Hamming ratio
// and which of the two overloads' projections to use.  Unlike Fuse the member is sequential inside a job: `vpMatched[bestIdx] = pMP` (:465, :573)
// takes the feature away from every later entry, so a job is answered by the ordered fix-point resolve of k_resolve (match_resolve.inc,
// MODE_SIM3), one workgroup per job.  Jobs are independent of one another, also on the same slot.  Every call site starts from an all-NULL
// vpMatched (DESIGN.md 4w), so no feature is blocked at entry and spAlreadyFound is empty.
//
//   k_sin_grid     (search_in_neighbors.inc) one workgroup per DISTINCT (slot, bounds) of the call: its 64 x 48 grid.  Jobs name their grid by
//                  index, so a slot that many jobs search is gridded once.
//   k_s3p_gate     one lane per (job, entry), entries the fast index: a wave's lanes share the job; id < 0, bad, then sim3_query with the job's
//                  th and projection; survivors to the work list with projection, level and job.  An entry that would be searched and whose
//                  point has no attributes is counted.
//   k_s3p_walk<0>  16 lanes per surviving pair walk the window in GetFeaturesInArea order over levels [level - 1, level] (walk_window,
//                  match_grid.h: sin_walk's traversal, here keeping every candidate instead of the nearest) and COUNT the
//                  candidates within the job's threshold; a wave then takes the list space of its four pairs with one atomicAdd on the total.
//                  (A scan of the counts over all pairs would give the same disjoint ranges in pair order; one workgroup took 215 us for it at
//                  120 000 pairs, two thirds of the call.  Where a list lies reaches no result.)
//   k_s3p_walk<1>  the same walk FILLS the lists: (distance << 16 | place in the walk, feature).  List layout: count / allocate / fill, exact for
//                  any list length.  The entries of a list stand in arrival order; the resolve takes the minimum key among the free ones, and
//                  keys are distinct, so the order inside a list never reaches a result.
//   k_s3p_resolve  one workgroup per job: every entry picks its nearest candidate that no EARLIER entry of the job holds, to the fixed point;
//                  then the job's matched row and count.
// Five launches and three memsets whatever the number of jobs, all on the null stream (the store's), one blocking copy at the end.  Integer
// atomics only; the order of the work list and the place of a list depend on arrival, the results do not.  When the lists outgrow their arena
// the fill and the resolve do nothing, the host reads the total, grows the arena and launches the same five again (never in steady state: the
// arena starts at four candidates a pair).

namespace rumi {

struct S3pJob : CovisSlotRef {         // one job of a call: its key-frame, then
    int32_t grid;                      // which grid of the call is its
    int32_t sortedOff;                 // first entry of that grid's sorted feature indices
    int32_t pointStart, pointCount;    // its list in the call's ids
    int32_t pairBase, rowStart;        // its first (job, entry) pair; its row in the matched block
    int32_t variant;                   // 0: mpCamera->project (:372-471), 1: explicit 1 / z (:473-579)
    float th, thrF;                    // window factor; TH_LOW * ratio, compared in float as :464 / :572 do
    float T[7], Ow[3], bounds[4], logSf, wInv, hInv;
    float pad[1];
};
static_assert(sizeof(S3pJob) % 16 == 0, "a table entry");

struct S3pArgs {
    SinArgs s;                         // tab: the grids; blockCount / blockBase: candidates per pair and where its list starts; head; work
    const S3pJob *jobs; const int32_t *ids;
    int32_t *cursor, *asg;             // [pairs] fill position; the feature the entry holds (-1: none)
    uint2 *lists; int listCap;
    int32_t *nmatches, *rounds, *rows; // [jobs], [jobs], the dense rows
};

__global__ __launch_bounds__(256) void k_s3p_gate(S3pArgs a) {
    const S3pJob &J = a.jobs[blockIdx.y];
    if ((int)(blockIdx.x * 256) >= J.pointCount) return;
    const int i = blockIdx.x * 256 + threadIdx.x;
    Query q{};
    if (i < J.pointCount) {
        const int p = a.ids[J.pointStart + i];
        if (p >= 0) {
            const CovisPoint P = a.s.v.point(p);
            if (!P.bad()) {                                  // pMP->isBad(), :396 / :498
                if (!a.s.v.has_attr(P)) atomicAdd(&a.s.head[SIN_MISSING], 1);
                else {
                    const CovisKeyFrame K = a.s.v.key_frame(J);
                    const CovisAttrGeom A = a.s.v.attr_geom(p);
                    float pos[3], nrm[3];
                    A.pos(pos); A.normal(nrm);
                    q = sim3_query(pos, nrm, A.min_dist(), A.max_dist(), J.T, K.K(), J.Ow, K.scale(), K.nlevels(), J.logSf, J.th, J.variant, J.bounds[0],
                                   J.bounds[1], J.bounds[2], J.bounds[3]);
                    q.maxLevel |= (int)blockIdx.y << 8;      // the item's last word: level (predict_scale's bits) | job << 8
                }
            }
        }
    }
    sin_push(a.s, q.valid != 0, q, (uint32_t)(J.pairBase + i));
}

// ORBmatcher.cc:438-461 / :546-569 for the pairs of the work list.  Only candidates with distance <= TH_LOW * ratio are kept: the member assigns
// bestIdx only when bestDist is within that bound, so a farther feature can never be assigned; and while any candidate within the bound is free
// the nearest free one is within it too, so dropping the farther ones changes no pick; a point that matches nothing blocks nothing.
template <bool FILL>
__global__ __launch_bounds__(256) void k_s3p_walk(S3pArgs a) {
    if (FILL && (uint32_t)a.s.head[SIN_NREV] > (uint32_t)a.listCap) return;      // the host grows the arena and launches again
    const int sub = threadIdx.x & (kSinLanes - 1), perBlock = 256 / kSinLanes;
    const int count = a.s.head[SIN_WORK];
    for (int w0 = blockIdx.x * perBlock; w0 < count; w0 += gridDim.x * perBlock) {
        const int w = w0 + (threadIdx.x / kSinLanes);
        int found = 0;
        uint32_t pair = 0;
        if (w < count) {
            const uint4 item = a.s.work[w];
            pair = item.z;
            const S3pJob &J = a.jobs[item.w >> 8];
            const int p = a.ids[J.pointStart + (int)(pair - (uint32_t)J.pairBase)];
            const CovisKeyFrame K = a.s.v.key_frame(J);
            const uint8_t *desc = K.desc();
            const GridView G{K.keys(), a.s.sorted + J.sortedOff, a.s.cellStart + (size_t)J.grid * (kGridCells + 1), J.bounds[0], J.bounds[1], J.wInv, J.hInv};
            uint4 q0, q1;
            a.s.v.attr_desc(p, q0, q1);
            const int maxLevel = (int)(item.w & 255u);
            const int listAt = FILL ? a.s.blockBase[pair] : 0, listLen = FILL ? a.s.blockCount[pair] : 0;
            walk_window<kSinLanes>(G, __uint_as_float(item.x), __uint_as_float(item.y), J.th * K.scale()[maxLevel],
                                   maxLevel - 1, maxLevel, sub, [&](int idx, const RumiKeyPoint &, int place) {
                const int d = hamming256(q0, q1, ld16_dword(desc + (size_t)idx * 32), ld16_dword(desc + (size_t)idx * 32 + 16));
                if (!((float)d <= J.thrF)) return;                                  // the cut (above)
                if (FILL) {
                    const int at = atomicAdd(&a.cursor[pair], 1);
                    if (at < listLen && (uint32_t)(listAt + at) < (uint32_t)a.listCap)
                        a.lists[listAt + at] = make_uint2(((uint32_t)d << 16) | (uint32_t)place, (uint32_t)idx);
                } else found++;
            });
        }
        if (!FILL) {                                         // all 64 lanes are here: a wave's four pairs take their list space with one atomic
            static_assert(kSinLanes == 16, "four pairs a wave");
#pragma unroll
            for (int m = 1; m < kSinLanes; m <<= 1) found += __shfl_xor(found, m);
            const int f0 = __shfl(found, 0), f1 = __shfl(found, 16), f2 = __shfl(found, 32), f3 = __shfl(found, 48);
            const int lane = threadIdx.x & 63, all = (f0 + f1) + (f2 + f3);
            int base = 0;
            if (lane == 0 && all) base = atomicAdd(&a.s.head[SIN_NREV], all);
            base = __shfl(base, 0) + (lane >= 16 ? f0 : 0) + (lane >= 32 ? f1 : 0) + (lane >= 48 ? f2 : 0);
            if (w < count && sub == 0) { a.s.blockCount[pair] = found; a.s.blockBase[pair] = base; }
        }
    }
}

// The loop of the member over one job's entries, as k_resolve runs MODE_SIM3: round after round every entry picks the nearest candidate (strict
// `<` on distance, the first in walk order on a tie: the minimum key) that no earlier entry of the job held after the round before, until a
// round changes nothing.  Entry i is final after round i + 1, so nq + 1 rounds always suffice; only an entry that matched blocks.  An entry's
// state lives in global memory and is read and written by one thread; the per-thread boundary is the workgroup size.
constexpr int kS3pResolveThreads = 1024;
__global__ __launch_bounds__(kS3pResolveThreads) void k_s3p_resolve(S3pArgs a) {
    extern __shared__ int32_t sBlockedFrom[];                // [n] the smallest entry that holds the feature
    __shared__ int sChanged[2], sCount;
    if ((uint32_t)a.s.head[SIN_NREV] > (uint32_t)a.listCap || a.s.head[SIN_MISSING]) return;
    const S3pJob &J = a.jobs[blockIdx.x];
    const int tid = threadIdx.x, nt = kS3pResolveThreads, nq = J.pointCount, nfeat = J.n;
    const int kFree = 0x7FFFFFFF;
    const int32_t *cnt = a.s.blockCount + J.pairBase, *off = a.s.blockBase + J.pairBase;
    int32_t *asg = a.asg + J.pairBase;
    for (int f = tid; f < nfeat; f += nt) sBlockedFrom[f] = kFree;
    if (tid < 2) sChanged[tid] = 0;
    if (tid == 0) sCount = 0;
    int rounds = 0;
    for (int round = 0; round <= nq + 1; round++) {
        __syncthreads();
        for (int i = tid; i < nq; i += nt) {
            const int f = asg[i];
            if (f >= 0) atomicMin(&sBlockedFrom[f], i);
        }
        __syncthreads();
        int changed = 0;
        for (int i = tid; i < nq; i += nt) {
            const int c = cnt[i];
            if (c == 0) continue;
            if ((uint32_t)(off[i] + c) > (uint32_t)a.listCap) continue;      // (cannot happen below the total that was checked above)
            const uint2 *L = a.lists + off[i];
            uint32_t bestKey = 0xFFFFFFFFu;
            int pick = -1;
            for (int k = 0; k < c; k++) {
                const uint2 e = L[k];
                if (sBlockedFrom[e.y] < i) continue;         // vpMatched[idx] set by an earlier entry (:442 / :550)
                if (e.x < bestKey) { bestKey = e.x; pick = (int)e.y; }
            }
            if (pick != asg[i]) { changed = 1; asg[i] = pick; }
        }
        if (changed) sChanged[round & 1] = 1;
        __syncthreads();
        const int any = sChanged[round & 1];
        if (tid == 0) sChanged[(round + 1) & 1] = 0;         // last read before this round's barriers, next written after the next round's
        rounds = round + 1;
        if (!any) break;
        for (int f = tid; f < nfeat; f += nt) sBlockedFrom[f] = kFree;
    }
    // the row: a feature is held by at most one entry at the fixed point (a feature once taken is never offered again)
    __syncthreads();
    int32_t *holder = sBlockedFrom;
    for (int f = tid; f < nfeat; f += nt) holder[f] = -1;
    __syncthreads();
    int local = 0;
    for (int i = tid; i < nq; i += nt) {
        const int f = asg[i];
        if (f >= 0) { holder[f] = i; local++; }
    }
    if (local) atomicAdd(&sCount, local);
    __syncthreads();
    int32_t *row = a.rows + J.rowStart;
    for (int f = tid; f < nfeat; f += nt) row[f] = holder[f];
    if (tid == 0) { a.nmatches[blockIdx.x] = sCount; a.rounds[blockIdx.x] = rounds; }
}

// ---- host -------------------------------------------------------------------------------------------------------------------------------

}  // namespace rumi

extern "C" int rumi_search_by_projection_sim3_resident(RumiMatcher *m, RumiCovis *c, const RumiSim3ProjJob *jobs, int32_t n_jobs,
                                                       const int32_t *point_ids, int32_t n_points, int32_t *matched, int32_t *matched_start,
                                                       int32_t matched_cap, int32_t *nmatches) {
    static const char *entry = "rumi_search_by_projection_sim3_resident";
    if (!m || !c || !matched_start || n_jobs < 0 || n_points < 0 || matched_cap < 0 || (matched_cap > 0 && !matched) ||
        (n_jobs > 0 && (!jobs || !nmatches)) || (n_points > 0 && !point_ids)) {
        g_lastError = std::string(entry) + ": missing argument, or a negative count";
        return RUMI_E_INVALID;
    }
    if (n_jobs > RUMI_FUSE_MAX_TARGETS) {
        g_lastError = std::string(entry) + ": more than RUMI_FUSE_MAX_TARGETS jobs";
        return RUMI_E_CAPACITY;
    }
    const auto t0 = std::chrono::steady_clock::now();
    size_t pairs = 0;
    for (int j = 0; j < n_jobs; j++) {
        const RumiSim3ProjJob &J = jobs[j];
        if (J.th <= 0 || !std::isfinite(J.ratio_hamming) || !(J.ratio_hamming > 0.f)) {
            g_lastError = std::string(entry) + ": th and ratio_hamming must be positive";
            return RUMI_E_INVALID;
        }
        if (const char *why = fuse_kfs_check(1, [&](int) -> const RumiFuseKF & { return J.kf; })) { g_lastError = std::string(entry) + ": " + why; return RUMI_E_INVALID; }
        if (J.point_start < 0 || J.point_count < 0 || (int64_t)J.point_start + J.point_count > n_points) {
            g_lastError = std::string(entry) + ": a list range outside [0, n_points]";
            return RUMI_E_INVALID;
        }
        pairs += (size_t)J.point_count;
    }
    if (pairs >= kSinRevBit) { g_lastError = std::string(entry) + ": more (job, entry) pairs than a work item addresses"; return RUMI_E_CAPACITY; }
    // one grid per distinct (slot, bounds); the store is asked about each slot once
    std::vector<int32_t> slots, gridOf((size_t)n_jobs), slotAt, firstJob;            // distinct slots; job -> grid; grid -> place in slots, first job
    for (int j = 0; j < n_jobs; j++) {
        int g = -1;
        for (size_t k = 0; k < firstJob.size() && g < 0; k++)
            if (jobs[firstJob[k]].kf_slot == jobs[j].kf_slot && !std::memcmp(jobs[firstJob[k]].kf.bounds, jobs[j].kf.bounds, 16)) g = (int)k;
        if (g < 0) {
            int at = -1;
            for (size_t k = 0; k < slots.size() && at < 0; k++) if (slots[k] == jobs[j].kf_slot) at = (int)k;
            if (at < 0) { at = (int)slots.size(); slots.push_back(jobs[j].kf_slot); }
            g = (int)firstJob.size(); firstJob.push_back(j); slotAt.push_back(at);
        }
        gridOf[j] = g;
    }
    const int nG = (int)firstJob.size(), nS = (int)slots.size();
    std::vector<CovisSlotFeatures> info((size_t)nS);
    const bool work = pairs > 0;
    int rc;
    // the slots first, then (with work to do) the device both handles live on
    if ((rc = covis_features_check(c, nS, slots.data(), entry, info.data())) != RUMI_OK || (work && (rc = covis_same_device(c, m->device, entry)) != RUMI_OK)) return rc;
    for (int k = 0; k < nS; k++)
        if (info[k].n > m->maxFeat) { g_lastError = std::string(entry) + ": a key-frame exceeds the matcher's max_features"; return RUMI_E_CAPACITY; }
    size_t rowWords = 0, feats = 0;
    std::vector<int32_t> rowStart((size_t)n_jobs + 1);
    for (int j = 0; j < n_jobs; j++) { rowStart[j] = (int32_t)rowWords; rowWords += (size_t)info[slotAt[gridOf[j]]].n; }
    rowStart[n_jobs] = (int32_t)rowWords;
    for (int g = 0; g < nG; g++) feats += (size_t)info[slotAt[g]].n;
    if (rowWords > (size_t)matched_cap) {
        std::memcpy(matched_start, rowStart.data(), ((size_t)n_jobs + 1) * 4);       // the one refusal that writes: the caller sizes `matched` from it
        g_lastError = std::string(entry) + ": matched_cap too small (matched_start is written)";
        return RUMI_E_CAPACITY;
    }
    if (!work) {                                             // also a call: its rounds (none) and stage times (none) replace the last call's
        S3pState *s0 = made(newpts_state(m)->s3p);
        s0->rounds.assign((size_t)n_jobs, 0);
        s0->stageMs[0] = s0->stageMs[1] = s0->stageMs[2] = 0.f;
        std::memcpy(matched_start, rowStart.data(), ((size_t)n_jobs + 1) * 4);
        for (int j = 0; j < n_jobs; j++) nmatches[j] = 0;
        for (size_t f = 0; f < rowWords; f++) matched[f] = -1;
        return RUMI_OK;
    }
    HIP_TRY(hipSetDevice(m->device));
    NewPtsState *np = newpts_state(m);
    SinState *sin = made(np->sin);                           // the stamped tables and their epoch
    S3pState *s = made(np->s3p);
    s->clock.start(); s->clock.t[0] = t0;

    const size_t gridBytes = (size_t)nG * sizeof(SinKF), jobBytes = (size_t)n_jobs * sizeof(S3pJob), upBytes = gridBytes + jobBytes + (size_t)n_points * 4;
    const size_t headWords = SIN_HEAD + 2 * (size_t)n_jobs, resWords = headWords + rowWords;
    const size_t listFirst = std::min<size_t>(4 * pairs + 4096, 0x7FFFFFFF);
    if ((rc = s->up.reserve(upBytes, upBytes + upBytes / 2)) != RUMI_OK || (rc = s->res.reserve(resWords, resWords + resWords / 4)) != RUMI_OK ||
        (rc = s->pair.reserve(4 * pairs, 4 * pairs + pairs)) != RUMI_OK || (rc = s->sorted.reserve(feats + 1, feats + feats / 4 + 1)) != RUMI_OK ||
        (rc = s->cellStart.reserve((size_t)nG * (kGridCells + 1), (size_t)nG * (kGridCells + 1))) != RUMI_OK ||
        (rc = s->work.reserve(pairs + 1, pairs + pairs / 4 + 1)) != RUMI_OK || (rc = s->lists.reserve(listFirst, listFirst)) != RUMI_OK)
        return rc;
    CovisView fv;
    s->clock.mark();
    if ((rc = covis_view(c, 0, &fv)) != RUMI_OK) return rc;
    for (int i = 0; i < n_points; i++)
        if (point_ids[i] >= fv.maxPoints) { g_lastError = std::string(entry) + ": a point id at or above the store's point capacity"; return RUMI_E_INVALID; }
    if ((rc = sin_next_epoch(sin, fv)) != RUMI_OK) return rc;

    SinKF *grids = reinterpret_cast<SinKF *>(s->up.h);
    S3pJob *tab = reinterpret_cast<S3pJob *>(s->up.h + gridBytes);
    int32_t sortedOff = 0;
    for (int g = 0; g < nG; g++) {
        sin_kf_grid(&grids[g], covis_slot_ref(info[slotAt[g]]), slots[slotAt[g]], jobs[firstJob[g]].kf.bounds, sortedOff);
        sortedOff += grids[g].n;
    }
    int32_t pairBase = 0, maxCount = 0, maxN = 1;
    for (int j = 0; j < n_jobs; j++) {
        const RumiSim3ProjJob &Q = jobs[j];
        const SinKF &G = grids[gridOf[j]];
        S3pJob &R = tab[j];
        std::memset(&R, 0, sizeof R);
        static_cast<CovisSlotRef &>(R) = G; R.grid = gridOf[j]; R.sortedOff = G.sortedOff;
        R.pointStart = Q.point_start; R.pointCount = Q.point_count; R.pairBase = pairBase; R.rowStart = rowStart[j];
        R.variant = Q.explicit_invz != 0;
        R.th = (float)Q.th; R.thrF = (float)RUMI_TH_LOW * Q.ratio_hamming;
        std::memcpy(R.T, Q.kf.Tcw7, 28); std::memcpy(R.Ow, Q.kf.Ow, 12); std::memcpy(R.bounds, Q.kf.bounds, 16);
        R.logSf = Q.kf.log_scale_factor; R.wInv = G.wInv; R.hInv = G.hInv;
        pairBase += Q.point_count; maxCount = std::max(maxCount, Q.point_count); maxN = std::max(maxN, G.n);
    }
    std::memcpy(s->up.h + gridBytes + jobBytes, point_ids, (size_t)n_points * 4);
    const size_t ldsBytes = (size_t)maxN * sizeof(int32_t);
    if (ldsBytes > 48 * 1024) HIP_TRY(raise_lds_limit(reinterpret_cast<const void *>(k_s3p_resolve), ldsBytes));
    HIP_TRY(hipMemcpyAsync(s->up.d, s->up.h, upBytes, hipMemcpyHostToDevice, nullptr));
    int32_t *dRes = s->res.d;
    const int32_t *h = s->res.h;
    const int gx = (maxCount + 255) / 256;
    const int walkBlocks = (int)std::min<size_t>(2048, (pairs + 15) / 16 + 1);
    for (int attempt = 0;; attempt++) {
        HIP_TRY(hipMemsetAsync(dRes, 0, SIN_HEAD * 4, nullptr));
        HIP_TRY(hipMemsetAsync(s->pair.p, 0, 2 * pairs * 4, nullptr));
        HIP_TRY(hipMemsetAsync(s->pair.p + 3 * pairs, 0xFF, pairs * 4, nullptr));
        S3pArgs a{};
        a.s.tab = reinterpret_cast<const SinKF *>(s->up.d); a.s.v = fv;
        a.s.nT = nG; a.s.curSlot = -1; a.s.epoch = sin->epoch;
        a.s.slotTag = sin->slotTag.p; a.s.claim = sin->claim.p; a.s.sorted = s->sorted.p; a.s.cellStart = s->cellStart.p;
        a.s.blockCount = s->pair.p; a.s.blockBase = s->pair.p + 2 * pairs; a.s.work = s->work.p; a.s.head = dRes;
        a.jobs = reinterpret_cast<const S3pJob *>(s->up.d + gridBytes); a.ids = reinterpret_cast<const int32_t *>(s->up.d + gridBytes + jobBytes);
        a.cursor = s->pair.p + pairs; a.asg = s->pair.p + 3 * pairs;
        a.lists = s->lists.p; a.listCap = (int)std::min<size_t>(s->lists.cap, 0x7FFFFFFF);
        a.nmatches = dRes + SIN_HEAD; a.rounds = a.nmatches + n_jobs; a.rows = dRes + headWords;
        hipLaunchKernelGGL(k_sin_grid, dim3(nG), dim3(1024), 0, nullptr, a.s, s->sorted.p, s->cellStart.p);
        hipLaunchKernelGGL(k_s3p_gate, dim3(gx, n_jobs), dim3(256), 0, nullptr, a);
        hipLaunchKernelGGL(k_s3p_walk<false>, dim3(walkBlocks), dim3(256), 0, nullptr, a);
        hipLaunchKernelGGL(k_s3p_walk<true>, dim3(walkBlocks), dim3(256), 0, nullptr, a);
        hipLaunchKernelGGL(k_s3p_resolve, dim3(n_jobs), dim3(kS3pResolveThreads), ldsBytes, nullptr, a);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpy(s->res.h, dRes, resWords * 4, hipMemcpyDeviceToHost));     // counts and dense rows; the call's one synchronisation
        if (h[SIN_MISSING] || (uint32_t)h[SIN_NREV] <= (uint32_t)a.listCap) break;
        if (attempt || h[SIN_NREV] < 0) { g_lastError = std::string(entry) + ": the candidate lists outgrow their arena"; return RUMI_E_CAPACITY; }
        if ((rc = s->lists.reserve((size_t)h[SIN_NREV], (size_t)h[SIN_NREV] + (size_t)h[SIN_NREV] / 4)) != RUMI_OK) return rc;
    }
    s->clock.mark();
    if (h[SIN_MISSING]) {
        s->clock.finish(s->stageMs);
        g_lastError = std::string(entry) + ": " + std::to_string(h[SIN_MISSING]) + " searched list entries whose map point has no attributes (rumi_covis_set_point_attributes)";
        return RUMI_E_INVALID;
    }
    std::memcpy(matched_start, rowStart.data(), ((size_t)n_jobs + 1) * 4);
    std::memcpy(nmatches, h + SIN_HEAD, (size_t)n_jobs * 4);
    s->rounds.assign(h + SIN_HEAD + n_jobs, h + SIN_HEAD + 2 * (size_t)n_jobs);
    if (rowWords) std::memcpy(matched, h + headWords, rowWords * 4);
    s->clock.finish(s->stageMs);
    return RUMI_OK;
}

extern "C" int rumi_search_by_projection_sim3_stage_ms(const RumiMatcher *m, float *out3) {
    if (!out3 || !newpts_peek(m) || !newpts_peek(m)->s3p) {
        g_lastError = "rumi_search_by_projection_sim3_stage_ms: no resident Sim3 projection search precedes on this matcher";
        return RUMI_E_INVALID;
    }
    std::memcpy(out3, newpts_peek(m)->s3p->stageMs, 12);
    return RUMI_OK;
}

extern "C" int rumi_search_by_projection_sim3_rounds(const RumiMatcher *m, int32_t *rounds, int32_t n_jobs) {
    const rumi::S3pState *s = newpts_peek(m) ? newpts_peek(m)->s3p.get() : nullptr;
    if (!s || !rounds || n_jobs != (int32_t)s->rounds.size()) {
        g_lastError = "rumi_search_by_projection_sim3_rounds: no resident Sim3 projection search of n_jobs jobs precedes on this matcher";
        return RUMI_E_INVALID;
    }
    if (n_jobs) std::memcpy(rounds, s->rounds.data(), (size_t)n_jobs * 4);
    return RUMI_OK;
}
