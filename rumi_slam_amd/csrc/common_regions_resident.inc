// The BoW stage of LoopClosing::DetectCommonRegionsFromBoW (R/lib_src/LoopClosing.cc:576-651; CloudMerging.cc:1019-1094 is the same text) by slot,
// behind rumi_common_regions_bow_resident (include/rumi_mapping.h, DESIGN.md 4aa).  Included at the end of mapping.hip after
// sim3_projection_batch.inc.  What rumi_common_regions_bow (match_bow_kf_batch.inc) packs and uploads per call -- angles, descriptors, rows,
// FeatureVectors and the good flags of about 40 key-frames -- is read where the covisibility store keeps it: the CovisFeatRec block of a slot,
// its map-point row in the row arena and the bad bit of the point records.  A call sends 24 bytes a member and the group starts.
//
//   k_cr_match<SlotCrView, TakenLds>   (match_bow_stage.h) a lane's `taken` flags in LDS words of its own, as many as the largest member of the call
//                  asks for: a node of any size is searched here.  Both gates (ORBmatcher.cc:717-721, :736-742) are read in the store: row entry
//                  >= 0 and the point's bad bit clear.
//   k_bow_rows_finish<SlotCrView>      a bad member's count is -1.
//   k_cr_union<SlotCrView, FirstStamped>   the `first` table stamped instead of cleared: [groups][max_points] 64-bit words, owned by the handle, grown
//                  when a call has more groups or the store more points than any call before, and never cleared between calls (only when it is
//                  grown or the epoch counter wraps).
// Integer atomics only (atomicAdd / atomicMax on integers): no result depends on the order anything arrives in.

namespace rumi {

// ---- host -------------------------------------------------------------------------------------------------------------------------------
constexpr size_t kCrrFirstMaxBytes = (size_t)1 << 31;        // the `first` table is refused above 2 GiB (groups x max_points x 8 bytes)

}  // namespace rumi

extern "C" int rumi_common_regions_bow_resident(RumiMatcher *m, RumiCovis *c, int32_t cur_slot, int32_t n_groups, const int32_t *group_start,
                                                const int32_t *member_slot, float nnratio, int32_t check_orientation, int32_t *matches12,
                                                int32_t *nmatches, int32_t *matched_point, int32_t *matched_member, int32_t *num_bow_matches,
                                                int32_t *most_matches) {
    static const char *entry = "rumi_common_regions_bow_resident";
#define CRR_REFUSE(msg) do { g_lastError = std::string(entry) + ": " msg; return RUMI_E_INVALID; } while (0)
    // ---- what is refused, before anything touches the device or the outputs ----
    if (!c) CRR_REFUSE("the store is NULL");
    if (!group_start || n_groups < 0) CRR_REFUSE("group_start is NULL, or a negative group count");
    if (!nmatches || !matched_point || !matched_member || !num_bow_matches || !most_matches) CRR_REFUSE("an output array is NULL (only matches12 may be)");
    const auto t0 = std::chrono::steady_clock::now();
    int maxGroup = 0, nM = 0;
    if (const char *why = cr_groups_check(n_groups, group_start, &maxGroup, &nM)) { g_lastError = std::string(entry) + ": " + why; return RUMI_E_INVALID; }
    if (nM > 0 && !member_slot) CRR_REFUSE("member_slot is NULL");
    // the slots: a bad member is named but not searched; the current key-frame and every other member must hold features that fit their rows.
    // A slot may be named many times in a call; the store is asked about each distinct one once.
    std::vector<uint8_t> bad((size_t)nM, 0);
    std::vector<int32_t> distinct(1, cur_slot), at((size_t)nM, -1);      // the distinct slots, ascending; at[i]: member i's place among them
    for (int i = 0; i < nM; i++) {
        CovisCullSlot cs;
        covis_cull_slot(c, member_slot[i], &cs);
        if (!cs.live) CRR_REFUSE("a member slot outside the store or not live");
        if (cs.bad) bad[(size_t)i] = 1; else distinct.push_back(member_slot[i]);
    }
    std::sort(distinct.begin(), distinct.end());
    distinct.erase(std::unique(distinct.begin(), distinct.end()), distinct.end());
    auto place = [&](int32_t slot) { return (size_t)(std::lower_bound(distinct.begin(), distinct.end(), slot) - distinct.begin()); };
    std::vector<CovisSlotFeatures> info(distinct.size());
    int rc;
    if ((rc = covis_features_check(c, (int)distinct.size(), distinct.data(), entry, info.data())) != RUMI_OK) return rc;
    const size_t curAt = place(cur_slot);
    const int n = info[curAt].n, nnC = info[curAt].nn;
    int maxN = 0;                                            // over the members that are searched, the current key-frame among them when it is named
    for (int i = 0; i < nM; i++) {
        if (bad[(size_t)i]) continue;
        at[(size_t)i] = (int32_t)place(member_slot[i]);
        maxN = std::max(maxN, info[(size_t)at[(size_t)i]].n);
    }
    if (maxN > 65535) { g_lastError = std::string(entry) + ": a member above 65535 features (a node position has 16 bits in the search key)"; return RUMI_E_CAPACITY; }
    if ((int64_t)maxGroup * std::max(n, 1) > (int64_t)0x7FFFFFFF) CRR_REFUSE("group size x features exceeds the union's key range");
    if (!m) CRR_REFUSE("the matcher handle is NULL");
    const size_t P = (size_t)std::max(covis_max_points(c), 1);
    if ((size_t)std::max(n_groups, 1) * P * 8 > kCrrFirstMaxBytes) { g_lastError = std::string(entry) + ": groups x max_points x 8 bytes exceeds the union table's 2 GiB bound"; return RUMI_E_CAPACITY; }
    const size_t G = (size_t)n_groups, Mn = (size_t)nM * n;
    const CrOutputs out{matches12, nmatches, matched_point, matched_member, num_bow_matches, most_matches};
    if (n == 0 || nM == 0) {                                 // nothing to search: the literal loop leaves every vector NULL.  No device call.
        CrrState *s0 = made(newpts_state(m)->crr);
        s0->stageMs[0] = s0->stageMs[1] = s0->stageMs[2] = 0.f;
        cr_fill_nothing(n, nM, n_groups, bad.data(), out);
        return RUMI_OK;
    }
    // with work to do: the device both handles live on (a store without a device takes the matcher's)
    if ((rc = covis_same_device(c, m->device, entry)) != RUMI_OK) return rc;
#undef CRR_REFUSE
    // ---- device work from here on
    HIP_TRY(hipSetDevice(m->device));
    CrrState *s = made(newpts_state(m)->crr);
    s->clock.start(); s->clock.t[0] = t0;
    const size_t memBytes = (size_t)nM * sizeof(BowSlotKF), upBytes = memBytes + (G + 1) * 4;
    const CrResultLayout L(nM, n_groups, n);
    if ((rc = s->up.reserve(upBytes, upBytes * 2)) != RUMI_OK || (rc = s->res.reserve(L.iEnd, L.iEnd + L.iEnd / 2)) != RUMI_OK ||
        (rc = s->rotBin.reserve(Mn, Mn + Mn / 2)) != RUMI_OK)
        return rc;
    BowSlotKF *hm = reinterpret_cast<BowSlotKF *>(s->up.h);
    for (int i = 0; i < nM; i++) {
        if (bad[(size_t)i]) hm[i] = BowSlotKF{{}, 1};
        else hm[i] = BowSlotKF{covis_slot_ref(info[(size_t)at[(size_t)i]]), 0};
    }
    std::memcpy(s->up.h + memBytes, group_start, (G + 1) * 4);
    s->clock.mark();
    CovisView fv;
    if ((rc = covis_view(c, 0, &fv)) != RUMI_OK) return rc;
    // the stamped table: one row of max_points words a group.  A new block, or a wrapped counter, starts from zeroed stamps and epoch 1.
    if (G > s->firstGroups || P > s->firstPoints || s->epoch == 0xFFFFFFFFu) {
        // (a handle that has served a larger store or more groups keeps the larger shape; capped so that the bound above stays the bound)
        size_t wantG = std::max(G, s->firstGroups), wantP = std::max(P, s->firstPoints);
        if (wantG * wantP * 8 > kCrrFirstMaxBytes) { wantG = G; wantP = P; }
        if ((rc = s->first.reserve(wantG * wantP, wantG * wantP)) != RUMI_OK) { s->firstGroups = s->firstPoints = 0; return rc; }
        HIP_TRY(hipMemsetAsync(s->first.p, 0, s->first.cap * 8, nullptr));
        s->firstGroups = wantG; s->firstPoints = wantP; s->epoch = 0;
    }
    HIP_TRY(hipMemcpyAsync(s->up.d, s->up.h, upBytes, hipMemcpyHostToDevice, nullptr));
    int32_t *dRes = s->res.d;
    HIP_TRY(L.clear(dRes));
    SlotCrView V;
    V.tab = reinterpret_cast<const BowSlotKF *>(s->up.d); V.groupStart = reinterpret_cast<const int32_t *>(s->up.d + memBytes);
    V.s = fv;
    V.curKf = BowSlotKF{covis_slot_ref(info[curAt]), 0};
    BowRows R;
    CrGroups U;
    L.bind(dRes, &R, &U);
    R.rotBin = s->rotBin.p; R.nnratio = nnratio; R.checkOri = check_orientation != 0;
    const FirstStamped first{s->first.p, s->firstPoints, ++s->epoch};
    const size_t lds = taken_lds_bytes(maxN);                // (a node holds at most the member's feature count)
    if (lds > 64 * 1024) HIP_TRY(raise_lds_limit(reinterpret_cast<const void *>(k_cr_match<SlotCrView, TakenLds>), lds));
    if (nnC > 0 && maxN > 0) hipLaunchKernelGGL((k_cr_match<SlotCrView, TakenLds>), dim3((nnC + 15) / 16, nM), dim3(256), lds, nullptr, V, R);
    hipLaunchKernelGGL(k_bow_rows_finish<SlotCrView>, dim3(nM), dim3(256), 0, nullptr, V, R);
    hipLaunchKernelGGL((k_cr_union<SlotCrView, FirstStamped>), dim3(n_groups), dim3(1024), 0, nullptr, V, R, U, first);
    HIP_TRY(hipGetLastError());
    // counts, the groups' rows and (when asked for) the members' rows: the call's one synchronisation
    HIP_TRY(hipMemcpy(s->res.h + L.iNm, dRes + L.iNm, (L.back_end(matches12 != nullptr) - L.iNm) * 4, hipMemcpyDeviceToHost));
    s->clock.mark();
    L.unpack(s->res.h, out);
    s->clock.finish(s->stageMs);
    return RUMI_OK;
}

extern "C" int rumi_common_regions_bow_resident_stage_ms(const RumiMatcher *m, float *out3) {
    if (!out3 || !newpts_peek(m) || !newpts_peek(m)->crr) {
        g_lastError = "rumi_common_regions_bow_resident_stage_ms: no resident common-regions call precedes on this matcher";
        return RUMI_E_INVALID;
    }
    std::memcpy(out3, newpts_peek(m)->crr->stageMs, 12);
    return RUMI_OK;
}
