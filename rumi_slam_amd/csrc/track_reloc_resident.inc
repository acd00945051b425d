// Tracking::Relocalization by slot (R/lib_src/Tracking.cc:3212-3357), behind rumi_track_compute_bow / rumi_track_reloc_bow /
// rumi_track_reloc_begin_resident (include/rumi_track.h, DESIGN.md 4z).  Included at the end of track.hip, behind track_reloc.inc, whose
// session block (RelocState) and refine chain it feeds unchanged.  The key-frame side is read where the covisibility store keeps it: the
// CovisFeatRec block of a slot (key-points, descriptors, mFeatVec as CSR), its map-point row in the row arena, the bad bits and the 64-byte
// attribute records of the points.  A call sends slot numbers and a few words per candidate, nothing else.
//
//   k_bowf_match<SlotView, ResidentFrame, TakenLds>   (match_bow_stage.h) SearchByBoW of every (candidate, key-frame node) pair, 16 lanes each.  A
//                    lane's `taken` flags lie in LDS words of its own, as many as the frame's feature count asks for: no node size is refused.
//   k_bow_rows_finish<SlotView>   ComputeThreeMaxima and the count of every candidate; a bad slot's count is -1.
//   k_rtab_claim     a lane per (candidate, key-frame feature): atomicMax of its claim u = place in (candidate order, feature order) on the
//                    point's stamp: the lowest u wins (the stamps of track_local_map.inc: table_claim, table_row, table_row_of; the map and the
//                    epoch counter are the session's own).
//   k_rtab_order     ONE workgroup: the winners in order of u (block_ordered_slot), their rows, the ids of the rows, the rows without attributes.
//   k_rtab_gather    table_gather_rows without normal, obs and local: position, distances, bad and descriptor into the session block.
//   k_rsess_fill     key-points out of the feature arena, map-point rows and BoW matches rewritten from point ids to table rows, the
//                    RelocCand records and K4.
// Integer atomics only (atomicOr / atomicAdd / atomicMax on integers): no result depends on the order anything arrives in.

namespace rumi {

// ---- the session's point table and block ------------------------------------------------------------------------------------------------
// A CovisSlotRef without nn, which the session does not read: with its own two words the record stays at 24 bytes.
struct RsessCand { long long block; int32_t mpOff, nkf, keyOff, matchRow; };      // keyOff: features of the candidates before it; matchRow: its row of the BoW matches
static_assert(sizeof(RsessCand) == 24, "the candidate table as uploaded");

struct RsessArgs {
    const RsessCand *cands;
    int Kc, n, rowCap;
    uint32_t epoch;
    CovisView v;
    unsigned long long *rowOf;           // [max_points] (epoch << 32) | value, as track_local_map.inc
    int32_t *head;                       // {n_table, rows without attributes, -, -}
    int32_t *tableIds;                   // [rowCap]
    const int32_t *bowMatches;           // [K][n] point ids
    // the session block (RelocState::sess)
    RelocCand *outCands;
    RumiKeyPoint *outKeys;
    int32_t *outRows, *outMatch;
    float *pos, *minD, *maxD, *k4Out;
    uint8_t *bad;
    uint32_t *desc;
    float K4[4];
};

__global__ __launch_bounds__(256) void k_rtab_claim(RsessArgs a) {
    const RsessCand C = a.cands[blockIdx.y];
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= C.nkf) return;
    const int p = a.v.rows[C.mpOff + i];
    if (p >= 0) atomicMax(&a.rowOf[p], table_claim(a.epoch, C.keyOff + i));
}

__global__ __launch_bounds__(kTableThreads) void k_rtab_order(RsessArgs a) {
    __shared__ int sCnt[kTableThreads / 64], sBase, sMissing;
    const int tid = threadIdx.x;
    if (tid == 0) { sBase = 0; sMissing = 0; }
    __syncthreads();
    for (int k = 0; k < a.Kc; k++) {
        const RsessCand C = a.cands[k];
        for (int c0 = 0; c0 < C.nkf; c0 += kTableThreads) {
            const int i = c0 + tid;
            const int p = i < C.nkf ? a.v.rows[C.mpOff + i] : -1;
            const bool win = p >= 0 && a.rowOf[p] == table_claim(a.epoch, C.keyOff + i);
            block_ordered_slot(win, sCnt, &sBase, [&](int row) {
                a.rowOf[p] = table_row(a.epoch, row);
                if (row < a.rowCap) a.tableIds[row] = p;
                if (!a.v.has_attr(p)) atomicAdd(&sMissing, 1);
            });
        }
    }
    if (tid == 0) { a.head[0] = sBase; a.head[1] = sMissing; }
}

__global__ __launch_bounds__(256) void k_rtab_gather(RsessArgs a) {       // (the host refuses a call that has a row without attributes)
    table_gather_rows<false>(a.v, a.tableIds, min(a.head[0], a.rowCap), 0, TableRows{a.pos, nullptr, a.minD, a.maxD, nullptr, a.desc, a.bad, nullptr});
}

// grid (x, Kc): candidate blockIdx.y's key-points and row, then its matches; block (0, 0) also writes K4
__global__ __launch_bounds__(256) void k_rsess_fill(RsessArgs a) {
    const int k = blockIdx.y;
    const RsessCand C = a.cands[k];
    const int step = gridDim.x * 256, t0 = blockIdx.x * 256 + threadIdx.x;
    if (t0 == 0) a.outCands[k] = RelocCand{C.nkf, C.keyOff};
    if (k == 0 && t0 < 4) a.k4Out[t0] = a.K4[t0];
    const RumiKeyPoint *keys = a.v.keys_at(C.block + kCovisFeatKeysOffset);
    for (int i = t0; i < C.nkf; i += step) {
        a.outKeys[C.keyOff + i] = keys[i];
        const int p = a.v.rows[C.mpOff + i];
        int row = p >= 0 ? table_row_of(a.rowOf, a.epoch, p) : -1;
        if (row >= a.rowCap) row = -1;                       // (the host refuses such a call: nothing of it is read)
        a.outRows[C.keyOff + i] = row;
    }
    for (int f = t0; f < a.n; f += step) {
        const int p = a.bowMatches[(size_t)C.matchRow * a.n + f];
        int row = p >= 0 ? table_row_of(a.rowOf, a.epoch, p) : -1;
        if (row >= a.rowCap) row = -1;
        a.outMatch[(size_t)k * a.n + f] = row;
    }
}

// What rumi_track_compute_bow and rumi_track_reloc_bow leave on the device for the calls that follow on the same frame.
struct RelocResident {
    // the frame's FeatureVector, tracker-owned: valid while bowSerial == frameSerial
    DevBuf<uint32_t> fvNodes, fvIdx;
    DevBuf<int32_t> fvOff, fvNN;
    uint32_t bowSerial = 0;
    bool haveBow = false;
    // the BoW walk: valid while walkSerial == frameSerial
    bool haveWalk = false;
    uint32_t walkSerial = 0;
    const RumiCovis *store = nullptr;
    std::vector<int32_t> slots;
    std::vector<uint8_t> slotBad;
    MirrorBuf<uint8_t> tab;              // the candidate table of either entry
    MirrorBuf<uint8_t> out;              // [matches K n | nmatch K | hist K 32 | rotBin K n]
    // the session's id -> row map
    DevBuf<unsigned long long> rowOf;
    uint32_t epoch = 0;
    MirrorBuf<int32_t> ids;              // [head 4 | table ids rowCap]
};
void reloc_resident_release(RelocResident *r) { delete r; }

static RelocResident *resident_of(RumiTracker *t) {
    if (!t->rres) t->rres = new RelocResident();
    return t->rres;
}

}  // namespace rumi

extern "C" int rumi_track_compute_bow(RumiTracker *t, RumiVocabulary *voc, int32_t levelsup, uint32_t *word_id, double *word_weight, uint32_t *node_id) {
    static const char *entry = "rumi_track_compute_bow";
    if (!t || !voc || !word_id || !word_weight || !node_id) { g_lastError = std::string(entry) + ": missing argument"; return RUMI_E_INVALID; }
    if (t->curN < 0) { g_lastError = std::string(entry) + ": no frame is resident (rumi_track_extract first)"; return RUMI_E_INVALID; }
    HIP_TRY(hipSetDevice(t->device));
    RelocResident *r = resident_of(t);
    r->haveBow = false; r->haveWalk = false;
    const int n = t->curN;
    const size_t C = (size_t)t->cap;
    int rc;
    if ((rc = r->fvNodes.reserve(C + 1, C + 1)) != RUMI_OK || (rc = r->fvIdx.reserve(C + 1, C + 1)) != RUMI_OK || (rc = r->fvOff.reserve(C + 2, C + 2)) != RUMI_OK ||
        (rc = r->fvNN.reserve(4, 4)) != RUMI_OK)
        return rc;
    if (n == 0) {
        HIP_TRY(hipMemsetAsync(r->fvNN.p, 0, 16, nullptr));
        HIP_TRY(hipMemsetAsync(r->fvOff.p, 0, 8, nullptr));
        HIP_TRY(hipStreamSynchronize(nullptr));
        r->bowSerial = t->frameSerial; r->haveBow = true;
        return RUMI_OK;
    }
    // Frame::ComputeBoW (Frame.cc:763-768): the two steps of rumi_track_reference_keyframe, the FeatureVector into the tracker's own arrays
    if ((rc = rumi_voc_transform_batch_device(voc, t->d.record + t->oDesc, t->d.record, 1, t->cap, levelsup, t->dWord, t->dWeight, t->dNode, nullptr)) != RUMI_OK) return rc;
    int npad = 1;
    while (npad < n) npad <<= 1;
    const size_t fvLds = (size_t)npad * sizeof(unsigned long long);
    if (fvLds > 64 * 1024) HIP_TRY(raise_lds_limit(reinterpret_cast<const void *>(k_fv_build), fvLds));
    hipLaunchKernelGGL(k_fv_build, dim3(1), dim3(kFvThreads), fvLds, nullptr, n, npad, t->dNode, t->dWeight, r->fvNodes.p, r->fvOff.p, r->fvIdx.p, r->fvNN.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(t->hBow, t->dBow, C * 16, hipMemcpyDeviceToHost));
    std::memcpy(word_weight, t->hBow, (size_t)n * 8); std::memcpy(word_id, t->hBow + C * 8, (size_t)n * 4); std::memcpy(node_id, t->hBow + C * 12, (size_t)n * 4);
    r->bowSerial = t->frameSerial; r->haveBow = true;
    return RUMI_OK;
}

extern "C" int rumi_track_reloc_bow(RumiTracker *t, RumiCovis *c, int32_t K, const int32_t *slots, float nnratio, int32_t check_orientation, int32_t *matches,
                                    int32_t *nmatches_out) {
    static const char *entry = "rumi_track_reloc_bow";
    if (!t || !c || !slots || !nmatches_out) { g_lastError = std::string(entry) + ": missing argument"; return RUMI_E_INVALID; }
    if (t->curN < 0) { g_lastError = std::string(entry) + ": no frame is resident (rumi_track_extract first)"; return RUMI_E_INVALID; }
    RelocResident *r = t->rres;
    if (!r || !r->haveBow || r->bowSerial != t->frameSerial) { g_lastError = std::string(entry) + ": no rumi_track_compute_bow precedes on the resident frame"; return RUMI_E_INVALID; }
    const int n = t->curN;
    if (K < 1 || (n > 0 && !matches)) { g_lastError = std::string(entry) + ": K < 1 or a missing output"; return RUMI_E_INVALID; }
    // ---- the slots: a bad key-frame is named but not searched; every other one must hold features that fit its row
    std::vector<int32_t> live, sorted(slots, slots + K);
    std::vector<uint8_t> bad((size_t)K, 0);
    std::sort(sorted.begin(), sorted.end());
    if (std::adjacent_find(sorted.begin(), sorted.end()) != sorted.end()) { g_lastError = std::string(entry) + ": a slot named twice"; return RUMI_E_INVALID; }
    for (int k = 0; k < K; k++) {
        CovisCullSlot cs;
        covis_cull_slot(c, slots[k], &cs);
        if (!cs.live) { g_lastError = std::string(entry) + ": a slot outside the store or not live"; return RUMI_E_INVALID; }
        bad[(size_t)k] = cs.bad ? 1 : 0;
        if (!cs.bad) live.push_back(slots[k]);
    }
    std::vector<CovisSlotFeatures> info(live.size() + 1);
    int rc;
    if ((rc = covis_features_check(c, (int)live.size(), live.data(), entry, info.data())) != RUMI_OK || (rc = covis_same_device(c, t->device, entry)) != RUMI_OK) return rc;
    // ---- device work from here on
    HIP_TRY(hipSetDevice(t->device));
    r->haveWalk = false;
    const size_t Kn = (size_t)K * n;
    const size_t oCnt = Kn * 4, oHist = oCnt + (size_t)K * 4, oBin = oHist + (size_t)K * 128, outBytes = oBin + Kn;
    if ((rc = r->tab.reserve((size_t)K * sizeof(BowSlotKF), (size_t)K * sizeof(BowSlotKF) * 2)) != RUMI_OK || (rc = r->out.reserve(outBytes, outBytes + outBytes / 2)) != RUMI_OK)
        return rc;
    BowSlotKF *hc = reinterpret_cast<BowSlotKF *>(r->tab.h);
    int maxNodes = 0;
    for (int k = 0, l = 0; k < K; k++) {
        if (bad[(size_t)k]) { hc[k] = BowSlotKF{{}, 1}; continue; }
        hc[k] = BowSlotKF{covis_slot_ref(info[(size_t)l++]), 0};
        maxNodes = std::max(maxNodes, hc[k].nn);
    }
    CovisView fv;
    if ((rc = covis_view(c, 0, &fv)) != RUMI_OK) return rc;
    HIP_TRY(hipMemcpyAsync(r->tab.d, r->tab.h, (size_t)K * sizeof(BowSlotKF), hipMemcpyHostToDevice, nullptr));
    if (Kn) HIP_TRY(hipMemsetAsync(r->out.d, 0xFF, Kn * 4, nullptr));                       // matches = -1
    HIP_TRY(hipMemsetAsync(r->out.d + oCnt, 0, oBin - oCnt, nullptr));                      // counts and histograms
    SlotView V{reinterpret_cast<const BowSlotKF *>(r->tab.d), fv};
    ResidentFrame F{resident_keys(t), reinterpret_cast<const uint32_t *>(t->d.record + t->oDesc), r->fvNodes.p, r->fvIdx.p, r->fvOff.p, r->fvNN.p};
    BowRows R;
    R.matches = reinterpret_cast<int32_t *>(r->out.d); R.nmatch = reinterpret_cast<int32_t *>(r->out.d + oCnt);
    R.hist = reinterpret_cast<int32_t *>(r->out.d + oHist); R.rotBin = reinterpret_cast<int8_t *>(r->out.d + oBin);
    R.n = n; R.nnratio = nnratio; R.checkOri = check_orientation;
    const size_t lds = taken_lds_bytes(n);                   // (a node holds at most n features)
    if (lds > 64 * 1024) HIP_TRY(raise_lds_limit(reinterpret_cast<const void *>(k_bowf_match<SlotView, ResidentFrame, TakenLds>), lds));
    if (maxNodes > 0 && n > 0) hipLaunchKernelGGL((k_bowf_match<SlotView, ResidentFrame, TakenLds>), dim3((maxNodes + 15) / 16, K), dim3(256), lds, nullptr, V, F, R);
    hipLaunchKernelGGL(k_bow_rows_finish<SlotView>, dim3(K), dim3(256), 0, nullptr, V, R);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(r->out.h, r->out.d, oHist, hipMemcpyDeviceToHost));                    // matches and counts: the call's one synchronisation
    if (Kn) std::memcpy(matches, r->out.h, Kn * 4);
    std::memcpy(nmatches_out, r->out.h + oCnt, (size_t)K * 4);
    r->store = c; r->slots.assign(slots, slots + K); r->slotBad = bad;
    r->walkSerial = t->frameSerial; r->haveWalk = true;
    return RUMI_OK;
}

extern "C" int rumi_track_reloc_begin_resident(RumiTracker *t, RumiCovis *c, const float *K4, int32_t Kc, const int32_t *cand, int32_t *table_ids,
                                               int32_t table_cap, int32_t *n_table) {
    static const char *entry = "rumi_track_reloc_begin_resident";
    if (!t || !c || !K4 || Kc < 0 || (Kc > 0 && !cand) || table_cap < 0 || (table_cap > 0 && !table_ids) || !n_table) {
        g_lastError = std::string(entry) + ": missing argument or negative count";
        return RUMI_E_INVALID;
    }
    if (t->curN < 0) { g_lastError = std::string(entry) + ": no frame is resident (rumi_track_extract first)"; return RUMI_E_INVALID; }
    RelocResident *r = t->rres;
    if (!r || !r->haveWalk || r->walkSerial != t->frameSerial || r->store != c) {
        g_lastError = std::string(entry) + ": no rumi_track_reloc_bow on this store precedes on the resident frame";
        return RUMI_E_INVALID;
    }
    const int n = t->curN, K = (int)r->slots.size();
    std::vector<int32_t> sel((size_t)Kc);
    for (int k = 0; k < Kc; k++) {
        if (cand[k] < 0 || cand[k] >= K || r->slotBad[(size_t)cand[k]]) { g_lastError = std::string(entry) + ": a candidate outside [0, K) or naming a bad slot"; return RUMI_E_INVALID; }
        sel[(size_t)k] = r->slots[(size_t)cand[k]];
    }
    std::vector<CovisSlotFeatures> info((size_t)Kc + 1);
    int rc;
    if ((rc = covis_features_check(c, Kc, sel.data(), entry, info.data())) != RUMI_OK ||                         // (also: a candidate named twice)
        (rc = covis_same_device(c, t->device, entry)) != RUMI_OK)
        return rc;
    size_t keysAll = 0;
    int maxNkf = 0;
    for (int k = 0; k < Kc; k++) { keysAll += (size_t)info[(size_t)k].n; maxNkf = std::max(maxNkf, info[(size_t)k].n); }
    if (keysAll > 0x7FFFFFFF / sizeof(RumiKeyPoint)) { g_lastError = std::string(entry) + ": the candidates' key-points exceed a 31-bit offset"; return RUMI_E_CAPACITY; }
    // ---- device work from here on
    HIP_TRY(hipSetDevice(t->device));
    if (!t->reloc) t->reloc = new RelocState();
    RelocState *s = t->reloc;
    s->open = false;
    const int rowCap = (int)std::min<size_t>(std::min(t->maxPts, table_cap), keysAll);      // a table has at most one row per key-frame feature
    s->oKeys = up16((size_t)Kc * sizeof(RelocCand)); s->oRows = up16(s->oKeys + keysAll * sizeof(RumiKeyPoint)); s->oMatch = up16(s->oRows + keysAll * 4);
    s->oPos = up16(s->oMatch + (size_t)Kc * n * 4); s->oMin = up16(s->oPos + (size_t)rowCap * 12); s->oMax = up16(s->oMin + (size_t)rowCap * 4);
    s->oBad = up16(s->oMax + (size_t)rowCap * 4); s->oDesc = up16(s->oBad + (size_t)rowCap); s->oK4 = up16(s->oDesc + (size_t)rowCap * 32);
    const size_t bytes = s->oK4 + 16;
    if ((rc = s->sess.reserve(bytes, bytes + bytes / 4)) != RUMI_OK) return rc;
    if ((rc = r->tab.reserve((size_t)std::max(Kc, 1) * sizeof(RsessCand), (size_t)std::max(Kc, 1) * sizeof(RsessCand) * 2)) != RUMI_OK ||
        (rc = r->ids.reserve(4 + (size_t)rowCap, 4 + (size_t)rowCap + (size_t)rowCap / 2)) != RUMI_OK)
        return rc;
    CovisView fv;
    if ((rc = covis_view(c, 0, &fv)) != RUMI_OK) return rc;
    if (r->rowOf.cap < (size_t)fv.maxPoints || r->epoch == 0xFFFFFFFFu) {
        if ((rc = r->rowOf.reserve((size_t)fv.maxPoints, (size_t)fv.maxPoints)) != RUMI_OK) return rc;
        HIP_TRY(hipMemsetAsync(r->rowOf.p, 0, r->rowOf.cap * 8, nullptr));
        r->epoch = 0;
    }
    RsessCand *hc = reinterpret_cast<RsessCand *>(r->tab.h);
    s->nkf.resize((size_t)Kc);
    size_t at = 0;
    for (int k = 0; k < Kc; k++) {
        const CovisSlotFeatures &I = info[(size_t)k];
        hc[k] = RsessCand{(long long)I.block, I.mpOff, I.n, (int32_t)at, cand[k]};
        s->nkf[(size_t)k] = I.n;
        at += (size_t)I.n;
    }
    if (Kc > 0) HIP_TRY(hipMemcpyAsync(r->tab.d, r->tab.h, (size_t)Kc * sizeof(RsessCand), hipMemcpyHostToDevice, nullptr));
    uint8_t *ds = s->sess.d;
    RsessArgs A{};
    A.cands = reinterpret_cast<const RsessCand *>(r->tab.d);
    A.Kc = Kc; A.n = n; A.rowCap = rowCap; A.epoch = ++r->epoch;
    A.v = fv;
    A.rowOf = r->rowOf.p; A.head = r->ids.d; A.tableIds = r->ids.d + 4;
    A.bowMatches = reinterpret_cast<const int32_t *>(r->out.d);
    A.outCands = reinterpret_cast<RelocCand *>(ds); A.outKeys = reinterpret_cast<RumiKeyPoint *>(ds + s->oKeys);
    A.outRows = reinterpret_cast<int32_t *>(ds + s->oRows); A.outMatch = reinterpret_cast<int32_t *>(ds + s->oMatch);
    A.pos = reinterpret_cast<float *>(ds + s->oPos); A.minD = reinterpret_cast<float *>(ds + s->oMin); A.maxD = reinterpret_cast<float *>(ds + s->oMax);
    A.bad = ds + s->oBad; A.desc = reinterpret_cast<uint32_t *>(ds + s->oDesc); A.k4Out = reinterpret_cast<float *>(ds + s->oK4);
    std::memcpy(A.K4, K4, 16);
    HIP_TRY(hipMemsetAsync(r->ids.d, 0, 16, nullptr));
    if (Kc > 0) {
        const int gx = std::max(1, (maxNkf + 255) / 256);
        if (maxNkf > 0) hipLaunchKernelGGL(k_rtab_claim, dim3(gx, Kc), dim3(256), 0, nullptr, A);
        hipLaunchKernelGGL(k_rtab_order, dim3(1), dim3(kTableThreads), 0, nullptr, A);
        hipLaunchKernelGGL(k_rtab_gather, dim3(std::min(std::max((rowCap + 255) / 256, 1), 256)), dim3(256), 0, nullptr, A);
        hipLaunchKernelGGL(k_rsess_fill, dim3(std::max(1, (std::max(maxNkf, n) + 255) / 256), Kc), dim3(256), 0, nullptr, A);
        HIP_TRY(hipGetLastError());
    } else HIP_TRY(hipMemcpyAsync(ds + s->oK4, K4, 16, hipMemcpyHostToDevice, nullptr));
    HIP_TRY(hipMemcpy(r->ids.h, r->ids.d, 16, hipMemcpyDeviceToHost));
    const int nmp = r->ids.h[0], nMissing = r->ids.h[1];
    if (nMissing > 0) {
        g_lastError = std::string(entry) + ": " + std::to_string(nMissing) + " row point(s) without attributes (rumi_covis_set_point_attributes)";
        return RUMI_E_INVALID;
    }
    if (nmp > table_cap || nmp > t->maxPts) {
        g_lastError = std::string(entry) + ": table_cap or the tracker's max_points is too small for the point table";
        return RUMI_E_CAPACITY;
    }
    if (nmp > 0) HIP_TRY(hipMemcpyAsync(r->ids.h + 4, r->ids.d + 4, (size_t)nmp * 4, hipMemcpyDeviceToHost, nullptr));
    // the resident frame as the matcher's kernels address it, and its grid (one for all hypotheses): as rumi_track_reloc_begin
    t->projN = 0;
    FrameDev fd;
    if ((rc = track_frame_dev(t, &fd)) != RUMI_OK) return rc;
    RumiMatcher *m = t->m;
    FLUSH(m);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(nullptr));
    s->fd = fd; s->K = Kc; s->nmp = nmp; s->maxNkf = maxNkf; s->words = (nmp + 31) / 32 + 1; s->n = n;
    std::memcpy(s->K4, K4, 16);
    s->serial = t->frameSerial;
    s->open = true;
    if (nmp > 0) std::memcpy(table_ids, r->ids.h + 4, (size_t)nmp * 4);
    *n_table = nmp;
    return RUMI_OK;
}
