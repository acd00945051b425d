// SearchByBoW(current key-frame, member) for every member of every candidate group of DetectCommonRegionsFromBoW in one launch, and the per-group
// union of the matched map points: kernels and C entry.
namespace rumi {

// ------------------------------------------------------------------------------------------------
// LoopClosing::DetectCommonRegionsFromBoW (LoopClosing.cc:542-853; the same text at CloudMerging.cc:985-1294) matches the current key-frame against a
// candidate and its best covisibles one SearchByBoW(KF, KF) at a time (:622-633) and folds the match vectors through a std::set (:635-651).  Every
// search starts from an empty vbMatched2, so the searches are independent; inside one search "a member feature is taken by the first query that wins it"
// never leaves a FeatureVector node (a feature lies in exactly one node).  So: grid over (node of the current key-frame, member), 16 lanes per pair;
// the current key-frame's features of the node run in list order, the lanes share out the member's features of the node and reduce (best, second)
// with the (dist << 16 | position) key: bow_node_walk (match_bow.h), which k_bow_batch_match calls with the roles swapped.  What this caller passes: the query side is the one
// current key-frame, BOTH sides carry a "holds a good map point" gate (ORBmatcher.cc:717-721, :736-742), acceptance is bestDist1 < TH_LOW (strict,
// :757) and the output is the member's FEATURE index.
// ------------------------------------------------------------------------------------------------
struct CrKF { int32_t n, nn, angle, desc, mp, good, nodes, off, idx, pad; };     // sizes and dword offsets of one member key-frame's arrays in the block
struct CrArgs {
    const uint32_t *blk;          // the uploaded block (dword view)
    int n, nnC, nM, nG, nmp;      // current key-frame's features and nodes, members, groups, map points
    int cAngle, cDesc, cGood, cNodes, cOff, cIdx, kfTable, memKf, groupStart;      // dword offsets
    int32_t *matches;             // [nM][n]  member feature index, -1 none
    int32_t *nmatch;              // [nM]
    int32_t *mpoint, *mmember;    // [nG][n]
    int32_t *numBow;              // [nG]
    int32_t *most;                // [nG][2]
    int32_t *err;                 // bit 0: a member node with more than 512 features
    int32_t *hist;                // [nM][32]
    int32_t *first;               // [nG][nmp]  smallest j * n + k that matched the point, kCrNever: none
    int32_t *winner;              // [nG][n]    largest j whose match at k was a first occurrence, -1 none
    int8_t *rotBin;               // [nM][n]
    float nnratio;
    int checkOri;
};
constexpr int32_t kCrNever = 0x7F7F7F7F;           // what a byte-wise memset of 0x7F leaves: above every j * n + k the entry admits

__global__ __launch_bounds__(256) void k_crb_match(CrArgs A) {
    const int mem = blockIdx.y, lane = threadIdx.x & 15, a = blockIdx.x * 16 + (threadIdx.x >> 4);
    if (a >= A.nnC) return;
    const CrKF *T = reinterpret_cast<const CrKF *>(A.blk + A.kfTable) + reinterpret_cast<const int32_t *>(A.blk + A.memKf)[mem];
    const uint32_t *kNodes = A.blk + T->nodes;
    const int lo = fv_find_node(kNodes, T->nn, (A.blk + A.cNodes)[a]);
    if (lo < 0) return;
    const int32_t *cOff = reinterpret_cast<const int32_t *>(A.blk + A.cOff), *kOff = reinterpret_cast<const int32_t *>(A.blk + T->off);
    const int c0 = kOff[lo], nc = kOff[lo + 1] - c0;
    if (nc > 512) { if (lane == 0) atomicOr(A.err, 1); return; }
    const uint32_t *kIdx = A.blk + T->idx + c0, *cIdx = A.blk + A.cIdx;
    const uint32_t *kDesc = A.blk + T->desc, *cDesc = A.blk + A.cDesc;
    const float *kAngle = reinterpret_cast<const float *>(A.blk + T->angle), *cAngle = reinterpret_cast<const float *>(A.blk + A.cAngle);
    const uint8_t *kGood = reinterpret_cast<const uint8_t *>(A.blk + T->good), *cGood = reinterpret_cast<const uint8_t *>(A.blk + A.cGood);
    TakenMask taken;                                         // a member feature that is matched already, or holds no good map point (:738-742)
    for (int j = 0, pos = lane; pos < nc; j++, pos += 16)
        if (!kGood[kIdx[pos]]) taken.set(j);
    bow_node_walk<true>(lane, cIdx, cOff[a], cOff[a + 1], cDesc, kIdx, nc, kDesc, A.nnratio, taken,            // strict: :757-758
                        [&](int iC) { return cGood[iC] != 0; },                             // no map point, or a bad one (:717-721)
                        [&](int iC, int f) {
                            A.matches[(size_t)mem * A.n + iC] = f;
                            if (A.checkOri) {
                                // (angles of real key-points give bins 0..12; the clamp keeps a malformed angle inside the histogram)
                                const int bin = min(max(rot_bin(cAngle[iC], kAngle[f]), 0), RUMI_HISTO_LENGTH - 1);
                                A.rotBin[(size_t)mem * A.n + iC] = (int8_t)bin;
                                atomicAdd(&A.hist[mem * 32 + bin], 1);
                            }
                        });
}

// rotation-histogram filter (ComputeThreeMaxima, ORBmatcher.cc:1795-1826) and the match count of every member.  A match the histogram removes has
// kept its member feature taken during the search, as in the reference, where the filter runs after the walk (:786-801).
__global__ __launch_bounds__(256) void k_crb_finish(CrArgs A) {
    const int mem = blockIdx.x;
    bow_finish(A.matches + (size_t)mem * A.n, A.rotBin + (size_t)mem * A.n, A.hist + mem * 32, A.n, A.checkOri, &A.nmatch[mem]);
}

// The union of one group (LoopClosing.cc:635-651 walks j ascending, then k ascending): one workgroup per group, integer atomics only, so the
// outcome does not depend on the order in which the lanes arrive.
//   A  first[point] = min over the surviving matches of j * n + k        = the (j, k) at which the literal loop inserts the point into its set
//   B  a match whose key equals first[point] is that insertion: it counts, and winner[k] = max j over the insertions at k (a later insertion at
//      the same k overwrites vpMatchedPoints[k]; the count keeps both)
//   C  every k writes the point and the member of its winner
// and the member with the most matches (:628-632, strictly greater: the first j wins a tie; 0, 0 when no member matched anything).
__global__ __launch_bounds__(1024) void k_crb_union(CrArgs A) {
    __shared__ int sCount;
    const int g = blockIdx.x, tid = threadIdx.x;
    const int32_t *groupStart = reinterpret_cast<const int32_t *>(A.blk + A.groupStart), *memKf = reinterpret_cast<const int32_t *>(A.blk + A.memKf);
    const CrKF *T = reinterpret_cast<const CrKF *>(A.blk + A.kfTable);
    const int m0 = groupStart[g], nmem = groupStart[g + 1] - m0;
    int32_t *first = A.first + (size_t)g * A.nmp, *winner = A.winner + (size_t)g * A.n;
    if (tid == 0) sCount = 0;
    // member j's match vector and the map points of its key-frame's features: the loops run j outside (uniform), k over the lanes, so that a
    // lane's loads of different members do not wait for one another
    auto row_of = [&](int j) { return A.matches + (size_t)(m0 + j) * A.n; };
    auto points_of = [&](int j) { return reinterpret_cast<const int32_t *>(A.blk + T[memKf[m0 + j]].mp); };
    for (int j = 0; j < nmem; j++) {
        const int32_t *row = row_of(j), *mp = points_of(j);
        for (int k = tid; k < A.n; k += 1024) {
            const int f = row[k];
            if (f >= 0) atomicMin(&first[mp[f]], j * A.n + k);
        }
    }
    __syncthreads();
    int local = 0;
    for (int j = 0; j < nmem; j++) {
        const int32_t *row = row_of(j), *mp = points_of(j);
        for (int k = tid; k < A.n; k += 1024) {
            const int f = row[k];
            if (f >= 0 && first[mp[f]] == j * A.n + k) { local++; atomicMax(&winner[k], j); }
        }
    }
    if (local) atomicAdd(&sCount, local);
    __syncthreads();
    for (int k = tid; k < A.n; k += 1024) {
        const int j = winner[k];
        A.mpoint[(size_t)g * A.n + k] = j < 0 ? -1 : points_of(j)[row_of(j)[k]];
        A.mmember[(size_t)g * A.n + k] = j;
    }
    if (tid == 0) {
        int most = 0, at = 0;
        for (int j = 0; j < nmem; j++) if (A.nmatch[m0 + j] > most) { most = A.nmatch[m0 + j]; at = j; }
        A.numBow[g] = sCount; A.most[2 * g] = at; A.most[2 * g + 1] = most;
    }
}

// ---- host side: checks, layout, pack, launch, unpack or fallback ----
static inline size_t crb_take(size_t &used, size_t bytes) { const size_t o = used; used += (bytes + 15) & ~(size_t)15; return o; }

static bool crb_fv_ok(const RumiFeatureVector &fv, int n) {
    if (fv.n_nodes < 0) return false;
    if (fv.n_nodes == 0) return true;
    if (!fv.node_ids || !fv.offsets || fv.offsets[0] != 0) return false;
    for (int a = 0; a < fv.n_nodes; a++) {
        if (fv.offsets[a + 1] < fv.offsets[a]) return false;
        if (a > 0 && fv.node_ids[a] <= fv.node_ids[a - 1]) return false;
    }
    const int ne = fv.offsets[fv.n_nodes];
    if (ne > 0 && !fv.indices) return false;
    for (int p = 0; p < ne; p++) if (fv.indices[p] >= (uint32_t)n) return false;
    return true;
}

// LoopClosing.cc:622-651 on the host, from the per-member match vectors: the fallback's second half
static void crb_host_union(int n, int nmp, const RumiBowKeyFrame *kfs, int nG, const int32_t *group_start, const int32_t *member_kf, const int32_t *matches12,
                           const int32_t *nmatches, int32_t *matched_point, int32_t *matched_member, int32_t *num_bow_matches, int32_t *most_matches) {
    std::vector<uint8_t> seen((size_t)std::max(nmp, 1));
    for (int g = 0; g < nG; g++) {
        std::fill(seen.begin(), seen.end(), 0);
        int count = 0, most = 0, at = 0;
        for (int k = 0; k < n; k++) { matched_point[(size_t)g * n + k] = -1; matched_member[(size_t)g * n + k] = -1; }
        for (int mem = group_start[g]; mem < group_start[g + 1]; mem++) {
            const int j = mem - group_start[g];
            if (nmatches[mem] > most) { most = nmatches[mem]; at = j; }
            for (int k = 0; k < n; k++) {
                const int f = matches12[(size_t)mem * n + k];
                if (f < 0) continue;
                const int mp = kfs[member_kf[mem]].mp[f];
                if (seen[mp]) continue;
                seen[mp] = 1; count++;
                matched_point[(size_t)g * n + k] = mp; matched_member[(size_t)g * n + k] = j;
            }
        }
        num_bow_matches[g] = count; most_matches[2 * g] = at; most_matches[2 * g + 1] = most;
    }
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
    if (group_start[0] != 0) CRB_REFUSE("group_start must begin at 0");
    int maxGroup = 0;
    for (int g = 0; g < n_groups; g++) {
        if (group_start[g + 1] < group_start[g]) CRB_REFUSE("group_start is not ascending");
        maxGroup = std::max(maxGroup, group_start[g + 1] - group_start[g]);
    }
    const int nM = group_start[n_groups], n = Cur->n;
    if (nM > 65535) CRB_REFUSE("more than 65535 members");
    if (nM > 0 && !member_kf) CRB_REFUSE("member_kf is NULL");
    for (int i = 0; i < nM; i++)
        if (member_kf[i] < 0 || member_kf[i] >= n_kfs) CRB_REFUSE("a member index lies outside the key-frame table");
    if ((int64_t)maxGroup * std::max(n, 1) >= (int64_t)kCrNever) CRB_REFUSE("group size x features exceeds the union's key range");
    if (!crb_fv_ok(*cur_fv, n)) CRB_REFUSE("cur_fv is malformed (offsets, node order, or a feature index outside Cur)");
    for (int k = 0; k < n_kfs; k++) {
        const RumiBowKeyFrame &K = kfs[k];
        if (K.feat.n < 0) CRB_REFUSE("a member key-frame has a negative feature count");
        if (K.feat.n > 0 && (!K.feat.keys_un || !K.feat.desc || !K.mp)) CRB_REFUSE("a member key-frame's keys_un, desc or mp is NULL");
        if (!crb_fv_ok(K.fv, K.feat.n)) CRB_REFUSE("a member's FeatureVector is malformed (offsets, node order, or a feature index outside the key-frame)");
        for (int i = 0; i < K.feat.n; i++)
            if (K.mp[i] >= nmp) CRB_REFUSE("a map-point id is not below nmp");
    }
    if (!m) CRB_REFUSE("the matcher handle is NULL");
#undef CRB_REFUSE
    std::memset(m->crbMs, 0, sizeof(m->crbMs));
    const int nnC = cur_fv->n_nodes, neC = nnC > 0 ? cur_fv->offsets[nnC] : 0, checkOri = check_orientation != 0;
    if (n == 0 || nM == 0) {                                 // nothing to search: the literal loop leaves every vector NULL
        for (size_t i = 0; i < (size_t)nM * n; i++) matches12[i] = -1;
        for (int i = 0; i < nM; i++) nmatches[i] = 0;
        for (size_t i = 0; i < (size_t)n_groups * n; i++) matched_point[i] = matched_member[i] = -1;
        for (int g = 0; g < n_groups; g++) num_bow_matches[g] = most_matches[2 * g] = most_matches[2 * g + 1] = 0;
        return RUMI_OK;
    }
    HIP_TRY(hipSetDevice(m->device));
    const auto tHost = std::chrono::steady_clock::now();

    // ---- layout.  Upload block: [current key-frame | key-frame table | member table | group starts | key-frame arrays], every array on 16 bytes.
    // Result block (ints): [hist nM 32 | err 1 | nmatch nM | numBow G | most 2 G] zeroed, [mpoint G n | mmember G n] written in full by the union,
    // [matches nM n | winner G n] = -1, [first G nmp] = kCrNever, then rotBin nM n bytes.  err .. matches comes back with one copy.
    size_t used = 0;
    const size_t oCA = crb_take(used, (size_t)n * 4), oCD = crb_take(used, (size_t)n * 32), oCG = crb_take(used, (size_t)n), oCN = crb_take(used, (size_t)nnC * 4),
                 oCO = crb_take(used, (size_t)(nnC + 1) * 4), oCI = crb_take(used, (size_t)neC * 4), oT = crb_take(used, (size_t)n_kfs * sizeof(CrKF)),
                 oMK = crb_take(used, (size_t)nM * 4), oGS = crb_take(used, (size_t)(n_groups + 1) * 4);
    std::vector<CrKF> tab(n_kfs);
    for (int k = 0; k < n_kfs; k++) {
        const int kn = kfs[k].feat.n, nn = kfs[k].fv.n_nodes, ne = nn > 0 ? kfs[k].fv.offsets[nn] : 0;
        CrKF &t = tab[k];
        t.n = kn; t.nn = nn; t.pad = 0;
        t.angle = (int32_t)(crb_take(used, (size_t)kn * 4) / 4); t.desc = (int32_t)(crb_take(used, (size_t)kn * 32) / 4); t.mp = (int32_t)(crb_take(used, (size_t)kn * 4) / 4);
        t.good = (int32_t)(crb_take(used, (size_t)kn) / 4); t.nodes = (int32_t)(crb_take(used, (size_t)nn * 4) / 4); t.off = (int32_t)(crb_take(used, (size_t)(nn + 1) * 4) / 4);
        t.idx = (int32_t)(crb_take(used, (size_t)ne * 4) / 4);
    }
    if (used / 4 > 0x7FFFFFFFull) { g_lastError = "rumi_common_regions_bow: the upload block exceeds the 32-bit dword offsets"; return RUMI_E_CAPACITY; }
    const size_t G = (size_t)n_groups, iHist = 0, iErr = iHist + (size_t)nM * 32, iNm = iErr + 1, iNum = iNm + nM, iMost = iNum + G, iPoint = iMost + 2 * G,
                 iMember = iPoint + G * n, iMatches = iMember + G * n, iWinner = iMatches + (size_t)nM * n, iFirst = iWinner + G * n, iEnd = iFirst + G * nmp;
    const size_t outBytes = iEnd * 4 + (size_t)nM * n, backInts = iWinner - iErr;
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
        if (n_kfs > 0) std::memcpy(h + oT, tab.data(), (size_t)n_kfs * sizeof(CrKF));
        std::memcpy(h + oMK, member_kf, (size_t)nM * 4);
        std::memcpy(h + oGS, group_start, (size_t)(n_groups + 1) * 4);
    }
    for (int k = 0; k < n_kfs; k++) {
        const CrKF &t = tab[k];
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
    HIP_TRY(hipMemsetAsync(dOut, 0, iPoint * 4, nullptr));
    HIP_TRY(hipMemsetAsync(dOut + iMatches, 0xFF, (iFirst - iMatches) * 4, nullptr));
    if (iEnd > iFirst) HIP_TRY(hipMemsetAsync(dOut + iFirst, 0x7F, (iEnd - iFirst) * 4, nullptr));
    stamp(1);
    CrArgs A;
    A.blk = reinterpret_cast<const uint32_t *>(m->crb.d);
    A.n = n; A.nnC = nnC; A.nM = nM; A.nG = n_groups; A.nmp = nmp;
    A.cAngle = (int)(oCA / 4); A.cDesc = (int)(oCD / 4); A.cGood = (int)(oCG / 4); A.cNodes = (int)(oCN / 4); A.cOff = (int)(oCO / 4); A.cIdx = (int)(oCI / 4);
    A.kfTable = (int)(oT / 4); A.memKf = (int)(oMK / 4); A.groupStart = (int)(oGS / 4);
    A.hist = dOut + iHist; A.err = dOut + iErr; A.nmatch = dOut + iNm; A.numBow = dOut + iNum; A.most = dOut + iMost; A.mpoint = dOut + iPoint;
    A.mmember = dOut + iMember; A.matches = dOut + iMatches; A.winner = dOut + iWinner; A.first = dOut + iFirst;
    A.rotBin = reinterpret_cast<int8_t *>(dOut + iEnd);
    A.nnratio = nnratio; A.checkOri = checkOri;
    if (nnC > 0) hipLaunchKernelGGL(k_crb_match, dim3((nnC + 15) / 16, nM), dim3(256), 0, nullptr, A);
    stamp(2);
    hipLaunchKernelGGL(k_crb_finish, dim3(nM), dim3(256), 0, nullptr, A);
    hipLaunchKernelGGL(k_crb_union, dim3(n_groups), dim3(1024), 0, nullptr, A);
    stamp(3);
    HIP_TRY(hipGetLastError());
    int32_t *ho = reinterpret_cast<int32_t *>(m->crbOut.h);
    if (prof) {
        HIP_TRY(hipMemcpyAsync(ho, dOut + iErr, backInts * 4, hipMemcpyDeviceToHost, nullptr));
        stamp(4);
        HIP_TRY(hipStreamSynchronize(nullptr));
        for (int i = 0; i < 4; i++) (void)hipEventElapsedTime(&m->crbMs[1 + i], ev[i], ev[i + 1]);
        for (auto &e : ev) (void)hipEventDestroy(e);
    } else {
        HIP_TRY(hipMemcpy(ho, dOut + iErr, backInts * 4, hipMemcpyDeviceToHost));
    }
    if (ho[0] & 1) {
        // A FeatureVector node of a member holds more than 512 features (k_crb_match keeps a node's "taken" flags in one 32-bit mask per lane of a
        // 16-lane group): shallow vocabularies or levelsup near L.  The results must still be those of the literal loop, so run it: one
        // rumi_search_by_bow_kf per member, then the union on the host.  A current feature with a good map point is given the id nmp, a point
        // that is not bad and that no member holds.
        std::vector<int32_t> curMp(n);
        std::vector<uint8_t> bad((size_t)nmp + 1, 0);
        if (nmp > 0) std::memcpy(bad.data(), mp_bad, (size_t)nmp);
        for (int i = 0; i < n; i++) curMp[i] = cur_good[i] ? nmp : -1;
        static const float kOneLevel[1] = {1.f};
        for (int mem = 0; mem < nM; mem++) {
            const RumiBowKeyFrame &K = kfs[member_kf[mem]];
            RumiFrameFeatures F2 = K.feat;                   // this entry reads n, angles and descriptors only; the single search also wants bounds and levels
            if (F2.nlevels < 1 || F2.nlevels > 64 || !F2.scale_factors || !(F2.max_x > F2.min_x) || !(F2.max_y > F2.min_y)) {
                F2.min_x = F2.min_y = 0.f; F2.max_x = F2.max_y = 1.f; F2.scale_factors = kOneLevel; F2.nlevels = 1;
            }
            RC_TRY(rumi_search_by_bow_kf(m, Cur, cur_fv, curMp.data(), &F2, &K.fv, K.mp, nmp + 1, bad.data(), nnratio, check_orientation,
                                         matches12 + (size_t)mem * n, &nmatches[mem]));
        }
        crb_host_union(n, nmp, kfs, n_groups, group_start, member_kf, matches12, nmatches, matched_point, matched_member, num_bow_matches, most_matches);
        return RUMI_OK;
    }
    auto back = [&](size_t i) { return ho + (i - iErr); };     // result-block index -> its place in the part that came back
    std::memcpy(nmatches, back(iNm), (size_t)nM * 4);
    std::memcpy(num_bow_matches, back(iNum), G * 4);
    std::memcpy(most_matches, back(iMost), 2 * G * 4);
    std::memcpy(matched_point, back(iPoint), G * n * 4);
    std::memcpy(matched_member, back(iMember), G * n * 4);
    std::memcpy(matches12, back(iMatches), (size_t)nM * n * 4);
    return RUMI_OK;
}
