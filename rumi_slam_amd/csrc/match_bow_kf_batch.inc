// SearchByBoW(current key-frame, member) for every member of every candidate group of DetectCommonRegionsFromBoW in one launch, and the per-group
// union of the matched map points: the C entry over k_cr_match, k_bow_rows_finish and k_cr_union (match_bow_stage.h) with the packed view and the
// `first` table cleared per call.  The `taken` flags lie in a register when no member node holds more than 512 features, in LDS otherwise.
namespace rumi {

// ---- host side: checks, layout, pack, launch, unpack ----
static inline size_t crb_take(size_t &used, size_t bytes) { const size_t o = used; used += (bytes + 15) & ~(size_t)15; return o; }

// maxNode (may be NULL): raised to the vector's largest node
static bool crb_fv_ok(const RumiFeatureVector &fv, int n, int *maxNode) {
    if (fv.n_nodes < 0) return false;
    if (fv.n_nodes == 0) return true;
    if (!fv.node_ids || !fv.offsets || fv.offsets[0] != 0) return false;
    for (int a = 0; a < fv.n_nodes; a++) {
        if (fv.offsets[a + 1] < fv.offsets[a]) return false;
        if (a > 0 && fv.node_ids[a] <= fv.node_ids[a - 1]) return false;
        if (maxNode) *maxNode = std::max(*maxNode, fv.offsets[a + 1] - fv.offsets[a]);
    }
    const int ne = fv.offsets[fv.n_nodes];
    if (ne > 0 && !fv.indices) return false;
    for (int p = 0; p < ne; p++) if (fv.indices[p] >= (uint32_t)n) return false;
    return true;
}

}  // namespace rumi

extern "C" int rumi_common_regions_bow_profile(RumiMatcher *m, int32_t enable, float *ms5) {
    if (!m) return RUMI_E_INVALID;
    m->crbProfile = enable != 0;
    if (ms5) std::memcpy(ms5, m->crbMs, sizeof(m->crbMs));
    return RUMI_OK;
}

extern "C" int rumi_common_regions_bow(RumiMatcher *m, const RumiFrameFeatures *Cur, const RumiFeatureVector *cur_fv, const uint8_t *cur_good, int32_t n_kfs,
                                       const RumiBowKeyFrame *kfs, int32_t nmp, const uint8_t *mp_bad, int32_t n_groups, const int32_t *group_start,
                                       const int32_t *member_kf, float nnratio, int32_t check_orientation, int32_t *matches12, int32_t *nmatches,
                                       int32_t *matched_point, int32_t *matched_member, int32_t *num_bow_matches, int32_t *most_matches) {
    // ---- what is refused, before anything touches the device or the outputs ----
#define CRB_REFUSE(msg) do { g_lastError = "rumi_common_regions_bow: " msg; return RUMI_E_INVALID; } while (0)
    if (!Cur || !cur_fv || !group_start) CRB_REFUSE("Cur, cur_fv or group_start is NULL");
    if (Cur->n < 0 || n_kfs < 0 || nmp < 0 || n_groups < 0) CRB_REFUSE("a negative count");
    if (Cur->n > 0 && (!cur_good || !Cur->keys_un || !Cur->desc)) CRB_REFUSE("cur_good or an array of Cur is NULL");
    if ((n_kfs > 0 && !kfs) || (nmp > 0 && !mp_bad)) CRB_REFUSE("kfs or mp_bad is NULL");
    if (!matches12 || !nmatches || !matched_point || !matched_member || !num_bow_matches || !most_matches) CRB_REFUSE("an output array is NULL");
    int maxGroup = 0, nM = 0, maxNode = 0;
    if (const char *why = cr_groups_check(n_groups, group_start, &maxGroup, &nM)) { g_lastError = std::string("rumi_common_regions_bow: ") + why; return RUMI_E_INVALID; }
    const int n = Cur->n;
    if (nM > 0 && !member_kf) CRB_REFUSE("member_kf is NULL");
    for (int i = 0; i < nM; i++)
        if (member_kf[i] < 0 || member_kf[i] >= n_kfs) CRB_REFUSE("a member index lies outside the key-frame table");
    if ((int64_t)maxGroup * std::max(n, 1) >= (int64_t)kCrNever) CRB_REFUSE("group size x features exceeds the union's key range");
    if (!crb_fv_ok(*cur_fv, n, nullptr)) CRB_REFUSE("cur_fv is malformed (offsets, node order, or a feature index outside Cur)");
    for (int k = 0; k < n_kfs; k++) {
        const RumiBowKeyFrame &K = kfs[k];
        if (K.feat.n < 0) CRB_REFUSE("a member key-frame has a negative feature count");
        if (K.feat.n > 0 && (!K.feat.keys_un || !K.feat.desc || !K.mp)) CRB_REFUSE("a member key-frame's keys_un, desc or mp is NULL");
        if (!crb_fv_ok(K.fv, K.feat.n, &maxNode)) CRB_REFUSE("a member's FeatureVector is malformed (offsets, node order, or a feature index outside the key-frame)");
        for (int i = 0; i < K.feat.n; i++)
            if (K.mp[i] >= nmp) CRB_REFUSE("a map-point id is not below nmp");
    }
    if (!m) CRB_REFUSE("the matcher handle is NULL");
#undef CRB_REFUSE
    if (maxNode > 65535) { g_lastError = "rumi_common_regions_bow: a member node above 65535 features (a node position has 16 bits in the search key)"; return RUMI_E_CAPACITY; }
    std::memset(m->crbMs, 0, sizeof(m->crbMs));
    const CrOutputs out{matches12, nmatches, matched_point, matched_member, num_bow_matches, most_matches};
    const int nnC = cur_fv->n_nodes, neC = nnC > 0 ? cur_fv->offsets[nnC] : 0, checkOri = check_orientation != 0;
    if (n == 0 || nM == 0) { cr_fill_nothing(n, nM, n_groups, nullptr, out); return RUMI_OK; }
    HIP_TRY(hipSetDevice(m->device));
    const auto tHost = std::chrono::steady_clock::now();

    // ---- layout.  Upload block: [current key-frame | key-frame table | member table | group starts | key-frame arrays], every array on 16 bytes.
    // Result block: CrResultLayout, then [first G nmp] = kCrNever, then rotBin nM n bytes.
    size_t used = 0;
    const size_t oCA = crb_take(used, (size_t)n * 4), oCD = crb_take(used, (size_t)n * 32), oCG = crb_take(used, (size_t)n), oCN = crb_take(used, (size_t)nnC * 4),
                 oCO = crb_take(used, (size_t)(nnC + 1) * 4), oCI = crb_take(used, (size_t)neC * 4), oT = crb_take(used, (size_t)n_kfs * sizeof(BowPackedKF)),
                 oMK = crb_take(used, (size_t)nM * 4), oGS = crb_take(used, (size_t)(n_groups + 1) * 4);
    std::vector<BowPackedKF> tab(n_kfs);
    for (int k = 0; k < n_kfs; k++) {
        const int kn = kfs[k].feat.n, nn = kfs[k].fv.n_nodes, ne = nn > 0 ? kfs[k].fv.offsets[nn] : 0;
        BowPackedKF &t = tab[k];
        t.n = kn; t.nn = nn; t.pad = 0;
        t.angle = (int32_t)(crb_take(used, (size_t)kn * 4) / 4); t.desc = (int32_t)(crb_take(used, (size_t)kn * 32) / 4); t.mp = (int32_t)(crb_take(used, (size_t)kn * 4) / 4);
        t.good = (int32_t)(crb_take(used, (size_t)kn) / 4); t.nodes = (int32_t)(crb_take(used, (size_t)nn * 4) / 4); t.off = (int32_t)(crb_take(used, (size_t)(nn + 1) * 4) / 4);
        t.idx = (int32_t)(crb_take(used, (size_t)ne * 4) / 4);
    }
    if (used / 4 > 0x7FFFFFFFull) { g_lastError = "rumi_common_regions_bow: the upload block exceeds the 32-bit dword offsets"; return RUMI_E_CAPACITY; }
    const CrResultLayout L(nM, n_groups, n);
    const size_t iFirst = L.iEnd, iEnd = iFirst + L.G * nmp, outBytes = iEnd * 4 + (size_t)nM * n;
    RC_TRY(m->crb.reserve(used, used * 2));
    RC_TRY(m->crbOut.reserve(outBytes, outBytes * 2));

    // ---- pack straight into the pinned mirror: the current key-frame and every distinct member key-frame once ----
    uint8_t *h = m->crb.h;
    {
        float *ca = reinterpret_cast<float *>(h + oCA);
        for (int i = 0; i < n; i++) ca[i] = Cur->keys_un[i].angle;
        std::memcpy(h + oCD, Cur->desc, (size_t)n * 32);
        for (int i = 0; i < n; i++) h[oCG + i] = cur_good[i] != 0;
        if (nnC > 0) { std::memcpy(h + oCN, cur_fv->node_ids, (size_t)nnC * 4); std::memcpy(h + oCO, cur_fv->offsets, (size_t)(nnC + 1) * 4); }
        else std::memset(h + oCO, 0, 4);
        if (neC > 0) std::memcpy(h + oCI, cur_fv->indices, (size_t)neC * 4);
        if (n_kfs > 0) std::memcpy(h + oT, tab.data(), (size_t)n_kfs * sizeof(BowPackedKF));
        std::memcpy(h + oMK, member_kf, (size_t)nM * 4);
        std::memcpy(h + oGS, group_start, (size_t)(n_groups + 1) * 4);
    }
    for (int k = 0; k < n_kfs; k++) {
        const BowPackedKF &t = tab[k];
        const RumiBowKeyFrame &K = kfs[k];
        const int ne = t.nn > 0 ? K.fv.offsets[t.nn] : 0;
        float *ka = reinterpret_cast<float *>(h + (size_t)t.angle * 4);
        uint8_t *good = h + (size_t)t.good * 4;
        for (int i = 0; i < t.n; i++) {
            ka[i] = K.feat.keys_un[i].angle;
            good[i] = K.mp[i] >= 0 && !mp_bad[K.mp[i]];
        }
        if (t.n > 0) { std::memcpy(h + (size_t)t.desc * 4, K.feat.desc, (size_t)t.n * 32); std::memcpy(h + (size_t)t.mp * 4, K.mp, (size_t)t.n * 4); }
        if (t.nn > 0) { std::memcpy(h + (size_t)t.nodes * 4, K.fv.node_ids, (size_t)t.nn * 4); std::memcpy(h + (size_t)t.off * 4, K.fv.offsets, (size_t)(t.nn + 1) * 4); }
        else std::memset(h + (size_t)t.off * 4, 0, 4);
        if (ne > 0) std::memcpy(h + (size_t)t.idx * 4, K.fv.indices, (size_t)ne * 4);
    }
    m->crbMs[0] = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - tHost).count();

    // ---- the block up, cleared tables, three kernels, the results back (the one synchronisation) ----
    hipEvent_t ev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    const bool prof = m->crbProfile;
    if (prof) for (auto &e : ev) HIP_TRY(hipEventCreate(&e));
    auto stamp = [&](int i) { if (prof) (void)hipEventRecord(ev[i], nullptr); };
    int32_t *dOut = reinterpret_cast<int32_t *>(m->crbOut.d);
    stamp(0);
    HIP_TRY(hipMemcpyAsync(m->crb.d, m->crb.h, used, hipMemcpyHostToDevice, nullptr));
    HIP_TRY(L.clear(dOut));
    if (iEnd > iFirst) HIP_TRY(hipMemsetAsync(dOut + iFirst, 0x7F, (iEnd - iFirst) * 4, nullptr));
    stamp(1);
    PackedCrView V;
    V.blk = reinterpret_cast<const uint32_t *>(m->crb.d); V.kfTable = (int)(oT / 4); V.memKf = (int)(oMK / 4); V.groupStart = (int)(oGS / 4);
    V.curKf = BowPackedKF{n, nnC, (int)(oCA / 4), (int)(oCD / 4), 0, (int)(oCG / 4), (int)(oCN / 4), (int)(oCO / 4), (int)(oCI / 4), 0};    // (no map-point row: cur_good is all the stage reads)
    BowRows R;
    CrGroups U;
    L.bind(dOut, &R, &U);
    R.rotBin = reinterpret_cast<int8_t *>(dOut + iEnd); R.nnratio = nnratio; R.checkOri = checkOri;
    const FirstCleared first{dOut + iFirst, (size_t)nmp};
    if (nnC > 0) HIP_TRY(launch_match_by_node(k_cr_match<PackedCrView, TakenMask>, k_cr_match<PackedCrView, TakenLds>, maxNode, dim3((nnC + 15) / 16, nM), V, R));
    stamp(2);
    hipLaunchKernelGGL(k_bow_rows_finish<PackedCrView>, dim3(nM), dim3(256), 0, nullptr, V, R);
    hipLaunchKernelGGL((k_cr_union<PackedCrView, FirstCleared>), dim3(n_groups), dim3(1024), 0, nullptr, V, R, U, first);
    stamp(3);
    HIP_TRY(hipGetLastError());
    int32_t *ho = reinterpret_cast<int32_t *>(m->crbOut.h);
    const size_t backInts = L.back_end(true) - L.iNm;
    if (prof) {
        HIP_TRY(hipMemcpyAsync(ho + L.iNm, dOut + L.iNm, backInts * 4, hipMemcpyDeviceToHost, nullptr));
        stamp(4);
        HIP_TRY(hipStreamSynchronize(nullptr));
        for (int i = 0; i < 4; i++) (void)hipEventElapsedTime(&m->crbMs[1 + i], ev[i], ev[i + 1]);
        for (auto &e : ev) (void)hipEventDestroy(e);
    } else {
        HIP_TRY(hipMemcpy(ho + L.iNm, dOut + L.iNm, backInts * 4, hipMemcpyDeviceToHost));
    }
    L.unpack(ho, out);
    return RUMI_OK;
}
