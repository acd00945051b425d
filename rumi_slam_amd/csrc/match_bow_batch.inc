// SearchByBoW of K key-frames against one frame in one launch: kernels and C entry.
namespace rumi {

// ------------------------------------------------------------------------------------------------
// SearchByBoW(KF_k, F) for K candidate key-frames against ONE frame in one launch (Tracking::Relocalization walks the candidates of
// KeyFrameDatabase::DetectRelocalizationCandidates one by one, Tracking.cc:3240-3260; every walk starts from an empty vpMapPointMatches, so the
// K searches are independent).  Within one search a frame feature is taken by the first query that wins it -- but a frame feature lies in
// exactly ONE FeatureVector node, so that dependency never leaves a node: nodes run in parallel, the (few) key-frame features of a node
// sequentially.  16 lanes per (key-frame, node): the lanes share out the frame's features of the node, compute their Hamming distances
// to the current key-frame feature in parallel and reduce (best, second) with the reference's tie rules (ORBmatcher.cc:252-289).
// ------------------------------------------------------------------------------------------------
struct BowKF { int32_t n, nn, angle, desc, mp, good, nodes, off, idx, pad; };      // sizes and dword offsets of one key-frame's arrays in the block
struct BowBatch {
    const uint32_t *blk;          // the uploaded block (dword view)
    int K, nf, nnF;
    int fAngle, fDesc, fNodes, fOff, fIdx, kfTable;     // dword offsets
    int32_t *matches;             // [K][nf]  map-point index (per key-frame numbering), -1 none
    int8_t *rotBin;               // [K][nf]
    int32_t *hist;                // [K][32]
    int32_t *nmatch;              // [K]
    int32_t *err;                 // bit 0: a node with more than 512 frame features
    float nnratio;
    int checkOri;
};

__global__ __launch_bounds__(256) void k_bow_batch_match(BowBatch B) {
    const int k = blockIdx.y, lane = threadIdx.x & 15, a = blockIdx.x * 16 + (threadIdx.x >> 4);
    const BowKF *T = reinterpret_cast<const BowKF *>(B.blk + B.kfTable) + k;
    if (a >= T->nn) return;
    const uint32_t *kfNodes = B.blk + T->nodes, *fNodes = B.blk + B.fNodes;
    const int lo = fv_find_node(fNodes, B.nnF, kfNodes[a]);
    if (lo < 0) return;
    const int32_t *fOff = reinterpret_cast<const int32_t *>(B.blk + B.fOff), *kOff = reinterpret_cast<const int32_t *>(B.blk + T->off);
    const int c0 = fOff[lo], nc = fOff[lo + 1] - c0;
    if (nc > 512) { if (lane == 0) atomicOr(B.err, 1); return; }
    const uint32_t *fIdx = B.blk + B.fIdx + c0, *kIdx = B.blk + T->idx;
    const uint32_t *fDesc = B.blk + B.fDesc, *kDesc = B.blk + T->desc;
    const float *fAngle = reinterpret_cast<const float *>(B.blk + B.fAngle), *kAngle = reinterpret_cast<const float *>(B.blk + T->angle);
    const int32_t *kMp = reinterpret_cast<const int32_t *>(B.blk + T->mp);
    const uint8_t *kGood = reinterpret_cast<const uint8_t *>(B.blk + T->good);
    TakenMask taken;                                         // a frame feature that already holds a map point
    bow_node_walk<false>(lane, kIdx, kOff[a], kOff[a + 1], kDesc, fIdx, nc, fDesc, B.nnratio, taken,
                         [&](int iKF) { return kGood[iKF] != 0; },                          // no map point, or a bad one (:238-243)
                         [&](int iKF, int f) {
                             B.matches[(size_t)k * B.nf + f] = kMp[iKF];
                             if (B.checkOri) {
                                 const int bin = rot_bin(kAngle[iKF], fAngle[f]);
                                 B.rotBin[(size_t)k * B.nf + f] = (int8_t)bin;
                                 atomicAdd(&B.hist[k * 32 + bin], 1);
                             }
                         });
}

// rotation-histogram filter (ComputeThreeMaxima, ORBmatcher.cc:1795-1826) and the match count of every key-frame
__global__ __launch_bounds__(256) void k_bow_batch_finish(BowBatch B) {
    const int k = blockIdx.x;
    bow_finish(B.matches + (size_t)k * B.nf, B.rotBin + (size_t)k * B.nf, B.hist + k * 32, B.nf, B.checkOri, &B.nmatch[k]);
}

// ---- host side: layout, pack, launch, unpack or fallback ----
// Byte offsets inside the upload block: [frame arrays | key-frame table | key-frame arrays], every array on a 16-byte boundary.  Results:
// [matches K nf | nmatch K | err 1 | hist K 32 | rotBin K nf bytes]; the first part (outInts words) comes back.
struct BowLayout {
    size_t oFA, oFD, oFN, oFO, oFI, oT, used = 0;
    std::vector<BowKF> tab;
    int maxNodes = 0;
    size_t outInts, outBytes;
};
static BowLayout bow_layout(int K, const RumiFrameFeatures *KFs, const RumiFeatureVector *kf_fvs, int nf, int nnF, int nfe) {
    BowLayout L;
    auto take = [&](size_t bytes) { const size_t o = L.used; L.used += (bytes + 15) & ~(size_t)15; return o; };
    L.oFA = take((size_t)nf * 4); L.oFD = take((size_t)nf * 32); L.oFN = take((size_t)nnF * 4); L.oFO = take((size_t)(nnF + 1) * 4); L.oFI = take((size_t)nfe * 4);
    L.oT = take((size_t)K * sizeof(BowKF));
    L.tab.resize(K);
    for (int k = 0; k < K; k++) {
        const int n = KFs[k].n, nn = kf_fvs[k].n_nodes, ne = nn > 0 ? kf_fvs[k].offsets[nn] : 0;
        BowKF &t = L.tab[k];
        t.n = n; t.nn = nn; t.pad = 0;
        t.angle = (int32_t)(take((size_t)n * 4) / 4); t.desc = (int32_t)(take((size_t)n * 32) / 4); t.mp = (int32_t)(take((size_t)n * 4) / 4);
        t.good = (int32_t)(take((size_t)n) / 4); t.nodes = (int32_t)(take((size_t)nn * 4) / 4); t.off = (int32_t)(take((size_t)(nn + 1) * 4) / 4);
        t.idx = (int32_t)(take((size_t)ne * 4) / 4);
        L.maxNodes = std::max(L.maxNodes, nn);
    }
    L.outInts = (size_t)K * nf + K + 1; L.outBytes = (L.outInts + (size_t)K * 32) * 4 + (size_t)K * nf;
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
    std::memcpy(h + L.oT, L.tab.data(), (size_t)K * sizeof(BowKF));
    for (int k = 0; k < K; k++) {
        const BowKF &t = L.tab[k];
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

// the block up, cleared results, both kernels, the first part of the results back (synchronises)
static int bow_launch(RumiMatcher *m, const BowLayout &L, int K, int nf, int nnF, float nnratio, int checkOri) {
    HIP_TRY(hipMemcpyAsync(m->bow.d, m->bow.h, L.used, hipMemcpyHostToDevice, nullptr));
    int32_t *dOut = reinterpret_cast<int32_t *>(m->bowOut.d);
    HIP_TRY(hipMemsetAsync(dOut, 0xFF, (size_t)K * nf * 4, nullptr));                              // matches = -1
    HIP_TRY(hipMemsetAsync(dOut + (size_t)K * nf, 0, ((size_t)K + 1 + (size_t)K * 32) * 4, nullptr));   // counts, error word, histograms
    BowBatch B;
    B.blk = reinterpret_cast<const uint32_t *>(m->bow.d);
    B.K = K; B.nf = nf; B.nnF = nnF;
    B.fAngle = (int)(L.oFA / 4); B.fDesc = (int)(L.oFD / 4); B.fNodes = (int)(L.oFN / 4); B.fOff = (int)(L.oFO / 4); B.fIdx = (int)(L.oFI / 4); B.kfTable = (int)(L.oT / 4);
    B.matches = dOut; B.nmatch = dOut + (size_t)K * nf; B.err = B.nmatch + K; B.hist = B.err + 1;
    B.rotBin = reinterpret_cast<int8_t *>(B.hist + (size_t)K * 32);
    B.nnratio = nnratio; B.checkOri = checkOri;
    if (L.maxNodes > 0) hipLaunchKernelGGL(k_bow_batch_match, dim3((L.maxNodes + 15) / 16, K), dim3(256), 0, nullptr, B);
    hipLaunchKernelGGL(k_bow_batch_finish, dim3(K), dim3(256), 0, nullptr, B);
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
    HIP_TRY(hipSetDevice(m->device));
    const int nf = F->n, nnF = f_fv->n_nodes, nfe = nnF > 0 ? f_fv->offsets[nnF] : 0;
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
    RC_TRY(bow_launch(m, L, K, nf, nnF, nnratio, check_orientation));
    const int32_t *ho = reinterpret_cast<const int32_t *>(m->bowOut.h);
    if (ho[(size_t)K * nf + K] & 1) {
        // a FeatureVector node of the frame holds more than 512 features (k_bow_batch_match keeps a node's "taken" flags in one 32-bit mask per
        // lane of a 16-lane group): shallow vocabularies or levelsup near L.  The results must still be those of K single searches, so run them.
        for (int k = 0; k < K; k++)
            RC_TRY(rumi_search_by_bow(m, &KFs[k], &kf_fvs[k], kf_mp[k], nmp[k], mp_bad[k], F, f_fv, nnratio, check_orientation, matches + (size_t)k * nf, &nmatches_out[k]));
        return RUMI_OK;
    }
    std::memcpy(matches, ho, (size_t)K * nf * 4);
    std::memcpy(nmatches_out, ho + (size_t)K * nf, (size_t)K * 4);
    return RUMI_OK;
}
