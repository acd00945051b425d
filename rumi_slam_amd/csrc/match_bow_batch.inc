// SearchByBoW of K key-frames against one frame in one launch: the C entry over k_bowf_match and k_bow_rows_finish (match_bow_stage.h) with the
// packed view.  The `taken` flags lie in a register when no node of the frame holds more than 512 features, in LDS otherwise.
namespace rumi {

// ---- host side: layout, pack, launch, unpack ----
// Byte offsets inside the upload block: [frame arrays | key-frame table | key-frame arrays], every array on a 16-byte boundary.  Results:
// [matches K nf | nmatch K | hist K 32 | rotBin K nf bytes]; the first part (outInts words) comes back.
struct BowLayout {
    size_t oFA, oFD, oFN, oFO, oFI, oT, used = 0;
    std::vector<BowPackedKF> tab;
    int maxNodes = 0;
    size_t outInts, outBytes;
};
static BowLayout bow_layout(int K, const RumiFrameFeatures *KFs, const RumiFeatureVector *kf_fvs, int nf, int nnF, int nfe) {
    BowLayout L;
    auto take = [&](size_t bytes) { const size_t o = L.used; L.used += (bytes + 15) & ~(size_t)15; return o; };
    L.oFA = take((size_t)nf * 4); L.oFD = take((size_t)nf * 32); L.oFN = take((size_t)nnF * 4); L.oFO = take((size_t)(nnF + 1) * 4); L.oFI = take((size_t)nfe * 4);
    L.oT = take((size_t)K * sizeof(BowPackedKF));
    L.tab.resize(K);
    for (int k = 0; k < K; k++) {
        const int n = KFs[k].n, nn = kf_fvs[k].n_nodes, ne = nn > 0 ? kf_fvs[k].offsets[nn] : 0;
        BowPackedKF &t = L.tab[k];
        t.n = n; t.nn = nn; t.pad = 0;
        t.angle = (int32_t)(take((size_t)n * 4) / 4); t.desc = (int32_t)(take((size_t)n * 32) / 4); t.mp = (int32_t)(take((size_t)n * 4) / 4);
        t.good = (int32_t)(take((size_t)n) / 4); t.nodes = (int32_t)(take((size_t)nn * 4) / 4); t.off = (int32_t)(take((size_t)(nn + 1) * 4) / 4);
        t.idx = (int32_t)(take((size_t)ne * 4) / 4);
        L.maxNodes = std::max(L.maxNodes, nn);
    }
    L.outInts = (size_t)K * nf + K; L.outBytes = (L.outInts + (size_t)K * 32) * 4 + (size_t)K * nf;
    return L;
}

static void bow_pack(uint8_t *h, const BowLayout &L, int K, const RumiFrameFeatures *KFs, const RumiFeatureVector *kf_fvs, const int32_t *const *kf_mp,
                     const int32_t *nmp, const uint8_t *const *mp_bad, const RumiFrameFeatures *F, const RumiFeatureVector *f_fv, int nfe) {
    const int nf = F->n, nnF = f_fv->n_nodes;
    float *fa = reinterpret_cast<float *>(h + L.oFA);
    for (int i = 0; i < nf; i++) fa[i] = F->keys_un[i].angle;
    std::memcpy(h + L.oFD, F->desc, (size_t)nf * 32);
    std::memcpy(h + L.oFN, f_fv->node_ids, (size_t)nnF * 4);
    std::memcpy(h + L.oFO, f_fv->offsets, (size_t)(nnF + 1) * 4);
    if (nfe > 0) std::memcpy(h + L.oFI, f_fv->indices, (size_t)nfe * 4);
    std::memcpy(h + L.oT, L.tab.data(), (size_t)K * sizeof(BowPackedKF));
    for (int k = 0; k < K; k++) {
        const BowPackedKF &t = L.tab[k];
        const int n = t.n, nn = t.nn, ne = nn > 0 ? kf_fvs[k].offsets[nn] : 0;
        float *ka = reinterpret_cast<float *>(h + (size_t)t.angle * 4);
        uint8_t *good = h + (size_t)t.good * 4;
        for (int i = 0; i < n; i++) {
            ka[i] = KFs[k].keys_un[i].angle;
            const int mp = kf_mp[k][i];
            good[i] = mp >= 0 && mp < nmp[k] && !(mp_bad[k] && mp_bad[k][mp]);
        }
        if (n > 0) { std::memcpy(h + (size_t)t.desc * 4, KFs[k].desc, (size_t)n * 32); std::memcpy(h + (size_t)t.mp * 4, kf_mp[k], (size_t)n * 4); }
        if (nn > 0) { std::memcpy(h + (size_t)t.nodes * 4, kf_fvs[k].node_ids, (size_t)nn * 4); std::memcpy(h + (size_t)t.off * 4, kf_fvs[k].offsets, (size_t)(nn + 1) * 4); }
        if (ne > 0) std::memcpy(h + (size_t)t.idx * 4, kf_fvs[k].indices, (size_t)ne * 4);
    }
}

// the block up, cleared results, both kernels, the first part of the results back (synchronises).  maxNode: the frame's largest node.
static int bow_launch(RumiMatcher *m, const BowLayout &L, int K, int nf, int nnF, int maxNode, float nnratio, int checkOri) {
    HIP_TRY(hipMemcpyAsync(m->bow.d, m->bow.h, L.used, hipMemcpyHostToDevice, nullptr));
    int32_t *dOut = reinterpret_cast<int32_t *>(m->bowOut.d);
    HIP_TRY(hipMemsetAsync(dOut, 0xFF, (size_t)K * nf * 4, nullptr));                              // matches = -1
    HIP_TRY(hipMemsetAsync(dOut + (size_t)K * nf, 0, ((size_t)K + (size_t)K * 32) * 4, nullptr));   // counts, histograms
    const uint32_t *blk = reinterpret_cast<const uint32_t *>(m->bow.d);
    PackedView V{blk, (int)(L.oT / 4)};
    PackedFrame F{blk, nnF, (int)(L.oFA / 4), (int)(L.oFD / 4), (int)(L.oFN / 4), (int)(L.oFO / 4), (int)(L.oFI / 4)};
    BowRows R;
    R.matches = dOut; R.nmatch = dOut + (size_t)K * nf; R.hist = R.nmatch + K;
    R.rotBin = reinterpret_cast<int8_t *>(R.hist + (size_t)K * 32);
    R.n = nf; R.nnratio = nnratio; R.checkOri = checkOri;
    if (L.maxNodes > 0)
        HIP_TRY(launch_match_by_node(k_bowf_match<PackedView, PackedFrame, TakenMask>, k_bowf_match<PackedView, PackedFrame, TakenLds>, maxNode,
                                     dim3((L.maxNodes + 15) / 16, K), V, F, R));
    hipLaunchKernelGGL(k_bow_rows_finish<PackedView>, dim3(K), dim3(256), 0, nullptr, V, R);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(m->bowOut.h, dOut, L.outInts * 4, hipMemcpyDeviceToHost));
    return RUMI_OK;
}

}  // namespace rumi

extern "C" int rumi_search_by_bow_batch(RumiMatcher *m, int32_t K, const RumiFrameFeatures *KFs, const RumiFeatureVector *kf_fvs,
                                        const int32_t *const *kf_mp, const int32_t *nmp, const uint8_t *const *mp_bad, const RumiFrameFeatures *F,
                                        const RumiFeatureVector *f_fv, float nnratio, int32_t check_orientation, int32_t *matches,
                                        int32_t *nmatches_out) {
    if (!m || K < 1 || !KFs || !kf_fvs || !kf_mp || !nmp || !mp_bad || !F || !f_fv || !matches || !nmatches_out || F->n < 0) return RUMI_E_INVALID;
    const int nf = F->n, nnF = f_fv->n_nodes, nfe = nnF > 0 ? f_fv->offsets[nnF] : 0;
    int maxNode = 0;                                         // the frame's largest node: where the `taken` flags of a lane lie
    for (int a = 0; a < nnF; a++) maxNode = std::max(maxNode, f_fv->offsets[a + 1] - f_fv->offsets[a]);
    if (maxNode > 65535) { g_lastError = "rumi_search_by_bow_batch: a node of the frame above 65535 features (a node position has 16 bits in the search key)"; return RUMI_E_CAPACITY; }
    HIP_TRY(hipSetDevice(m->device));
    for (int k = 0; k < K; k++) {
        nmatches_out[k] = 0;
        if (KFs[k].n < 0 || kf_fvs[k].n_nodes < 0 || nmp[k] < 0 || (KFs[k].n > 0 && !kf_mp[k])) return RUMI_E_INVALID;
    }
    for (size_t i = 0; i < (size_t)K * std::max(nf, 0); i++) matches[i] = -1;
    if (nf == 0 || nnF == 0) return RUMI_OK;
    const BowLayout L = bow_layout(K, KFs, kf_fvs, nf, nnF, nfe);
    RC_TRY(m->bow.reserve(L.used, L.used * 2));
    RC_TRY(m->bowOut.reserve(L.outBytes, L.outBytes * 2));
    bow_pack(m->bow.h, L, K, KFs, kf_fvs, kf_mp, nmp, mp_bad, F, f_fv, nfe);
    RC_TRY(bow_launch(m, L, K, nf, nnF, maxNode, nnratio, check_orientation));
    const int32_t *ho = reinterpret_cast<const int32_t *>(m->bowOut.h);
    std::memcpy(matches, ho, (size_t)K * nf * 4);
    std::memcpy(nmatches_out, ho + (size_t)K * nf, (size_t)K * 4);
    return RUMI_OK;
}
