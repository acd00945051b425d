// The BoW stage of LoopClosing::DetectCommonRegionsFromBoW (R/lib_src/LoopClosing.cc:576-651; CloudMerging.cc:1019-1094 is the same text) by slot,
// behind rumi_common_regions_bow_resident (include/rumi_mapping.h, DESIGN.md 4aa).  Included at the end of mapping.hip after
// sim3_projection_batch.inc.  What rumi_common_regions_bow (match_bow_kf_batch.inc) packs and uploads per call -- angles, descriptors, rows,
// FeatureVectors and the good flags of about 40 key-frames -- is read where the covisibility store keeps it: the CovisFeatRec block of a slot,
// its map-point row in the row arena and the bad bit of the point records.  A call sends 24 bytes a member and the group starts.
//
//   k_crr_match    SearchByBoW(current key-frame, member) of every (node of the current key-frame, member) pair, 16 lanes each: bow_node_walk<true>
//                  (match_bow.h) over TakenLds.  A lane's `taken` flags lie in LDS words of its own (word w of thread t at sTaken[w * 256 + t]),
//                  as many as the largest member of the call asks for: a node of any size is searched here, there is no error bit.  Both gates
//                  (ORBmatcher.cc:717-721, :736-742) are read in the store: row entry >= 0 and the point's bad bit clear.
//   k_crr_finish   ComputeThreeMaxima and the count of every member (bow_finish, match_device.h); a bad member's count is -1.
//   k_crr_union    one workgroup per group, LoopClosing.cc:635-651 as k_crb_union states it, with the `first` table stamped instead of cleared:
//                  first[g][point] takes atomicMax of (epoch << 32) | (0x7FFFFFFF - (j * n + k)), so the smallest (j, k) of THIS call wins and
//                  whatever an earlier call left (a smaller epoch) loses to any stamp of this one.  The table is [groups][max_points] 64-bit words,
//                  owned by the handle, grown when a call has more groups or the store more points than any call before, and never cleared
//                  between calls (only when it is grown or the epoch counter wraps).
// Integer atomics only (atomicAdd / atomicMax on integers): no result depends on the order anything arrives in.

namespace rumi {

struct CrrMem { long long block; int32_t mpOff, n, nn, bad; };        // one member: its CovisFeatRec (bytes into the feature arena), its row
static_assert(sizeof(CrrMem) == 24, "the member table as uploaded");

struct CrrArgs {
    const CrrMem *mem;                   // [nM]
    const int32_t *groupStart;           // [nG + 1]
    const uint8_t *feat;                 // the feature arena
    const int32_t *rows, *pt;            // the row arena, the point records
    long long curBlock;                  // the current key-frame
    int curMpOff, n, nnC, nM, nG;
    int words;                           // LDS words of `taken` flags a lane owns
    uint32_t epoch;
    size_t maxPoints;
    unsigned long long *first;           // [nG][maxPoints] (epoch << 32) | (0x7FFFFFFF - (j * n + k))
    int32_t *matches;                    // [nM][n]  member feature index, -1 none
    int32_t *nmatch;                     // [nM]
    int32_t *mpoint, *mmember;           // [nG][n]
    int32_t *numBow;                     // [nG]
    int32_t *most;                       // [nG][2]
    int32_t *hist;                       // [nM][32]
    int32_t *winner;                     // [nG][n]  largest j whose match at k was a first occurrence, -1 none
    int8_t *rotBin;                      // [nM][n]
    float nnratio;
    int checkOri;
};

template <class T> __device__ __forceinline__ const T *crr_arr(const CovisFeatRec *r, uint32_t o) {
    return reinterpret_cast<const T *>(reinterpret_cast<const uint8_t *>(r) + o);
}
// "holds a map point that is not bad" (ORBmatcher.cc:717-721, :738-742), read in the store
__device__ __forceinline__ bool crr_good(const int32_t *pt, int p) { return p >= 0 && !(pt[(size_t)p * kCovisPointWords + 2] & 1); }

__global__ __launch_bounds__(256) void k_crr_match(CrrArgs A) {
    extern __shared__ uint32_t sTaken[];                      // [words][256]
    const int mem = blockIdx.y, lane = threadIdx.x & 15, a = blockIdx.x * 16 + (threadIdx.x >> 4);
    const CrrMem K = A.mem[mem];
    if (K.bad || a >= A.nnC) return;
    const CovisFeatRec *RC = reinterpret_cast<const CovisFeatRec *>(A.feat + A.curBlock), *RK = reinterpret_cast<const CovisFeatRec *>(A.feat + K.block);
    const int lo = fv_find_node(crr_arr<uint32_t>(RK, RK->nodes), K.nn, crr_arr<uint32_t>(RC, RC->nodes)[a]);
    if (lo < 0) return;
    const int32_t *cOff = crr_arr<int32_t>(RC, RC->off), *kOff = crr_arr<int32_t>(RK, RK->off);
    const int c0 = kOff[lo], nc = kOff[lo + 1] - c0;
    const uint32_t *kIdx = crr_arr<uint32_t>(RK, RK->idx) + c0, *cIdx = crr_arr<uint32_t>(RC, RC->idx);
    const uint32_t *kDesc = crr_arr<uint32_t>(RK, RK->desc), *cDesc = crr_arr<uint32_t>(RC, RC->desc);
    const RumiKeyPoint *kKeys = crr_arr<RumiKeyPoint>(RK, RK->keys), *cKeys = crr_arr<RumiKeyPoint>(RC, RC->keys);
    const int32_t *kMp = A.rows + K.mpOff, *cMp = A.rows + A.curMpOff;
    TakenLds taken{sTaken + threadIdx.x};                    // a member feature that is matched already, or holds no good map point (:738-742)
    const int myWords = ((nc + 15) / 16 + 31) / 32;          // (<= A.words: a node holds at most the member's feature count)
    for (int w = 0; w < myWords; w++) taken.w[w * 256] = 0;
    for (int j = 0, pos = lane; pos < nc; j++, pos += 16)
        if (!crr_good(A.pt, kMp[kIdx[pos]])) taken.set(j);
    bow_node_walk<true>(lane, cIdx, cOff[a], cOff[a + 1], cDesc, kIdx, nc, kDesc, A.nnratio, taken,            // strict: :757-758
                        [&](int iC) { return crr_good(A.pt, cMp[iC]); },                     // no map point, or a bad one (:717-721)
                        [&](int iC, int f) {
                            A.matches[(size_t)mem * A.n + iC] = f;
                            if (A.checkOri) {
                                // (the clamp of k_crb_match: a malformed angle stays inside the histogram)
                                const int bin = min(max(rot_bin(cKeys[iC].angle, kKeys[f].angle), 0), RUMI_HISTO_LENGTH - 1);
                                A.rotBin[(size_t)mem * A.n + iC] = (int8_t)bin;
                                atomicAdd(&A.hist[mem * 32 + bin], 1);
                            }
                        });
}

// rotation-histogram filter (ComputeThreeMaxima, ORBmatcher.cc:1795-1826) and the match count of every member; -1 for a bad member, whose row
// the clear left at -1 (as rumi_track_reloc_bow answers a bad slot)
__global__ __launch_bounds__(256) void k_crr_finish(CrrArgs A) {
    const int mem = blockIdx.x;
    if (A.mem[mem].bad) { if (threadIdx.x == 0) A.nmatch[mem] = -1; return; }
    bow_finish(A.matches + (size_t)mem * A.n, A.rotBin + (size_t)mem * A.n, A.hist + mem * 32, A.n, A.checkOri, &A.nmatch[mem]);
}

// The union of one group (LoopClosing.cc:635-651 walks j ascending, then k ascending), steps A, B, C of k_crb_union.  A point's stamp is written by
// atomics only and read back through an atomic load behind the barrier, so the value read is the one every lane's atomicMax has settled on.
// A bad member's row is all -1 and its count -1: it adds nothing, wins nothing, and keeps its position j.
__device__ __forceinline__ unsigned long long crr_stamp(uint32_t epoch, int key) { return ((unsigned long long)epoch << 32) | (uint32_t)(0x7FFFFFFF - key); }

__global__ __launch_bounds__(1024) void k_crr_union(CrrArgs A) {
    __shared__ int sCount;
    const int g = blockIdx.x, tid = threadIdx.x;
    const int m0 = A.groupStart[g], nmem = A.groupStart[g + 1] - m0;
    unsigned long long *first = A.first + (size_t)g * A.maxPoints;
    int32_t *winner = A.winner + (size_t)g * A.n;
    if (tid == 0) sCount = 0;
    auto row_of = [&](int j) { return A.matches + (size_t)(m0 + j) * A.n; };
    auto points_of = [&](int j) { return A.rows + A.mem[m0 + j].mpOff; };
    for (int j = 0; j < nmem; j++) {
        const int32_t *row = row_of(j), *mp = points_of(j);
        for (int k = tid; k < A.n; k += 1024) {
            const int f = row[k];
            if (f >= 0) atomicMax(&first[mp[f]], crr_stamp(A.epoch, j * A.n + k));
        }
    }
    __syncthreads();
    int local = 0;
    for (int j = 0; j < nmem; j++) {
        const int32_t *row = row_of(j), *mp = points_of(j);
        for (int k = tid; k < A.n; k += 1024) {
            const int f = row[k];
            if (f >= 0 && __hip_atomic_load(&first[mp[f]], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == crr_stamp(A.epoch, j * A.n + k)) {
                local++;
                atomicMax(&winner[k], j);
            }
        }
    }
    if (local) atomicAdd(&sCount, local);
    __syncthreads();
    for (int k = tid; k < A.n; k += 1024) {
        const int j = __hip_atomic_load(&winner[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        A.mpoint[(size_t)g * A.n + k] = j < 0 ? -1 : points_of(j)[row_of(j)[k]];
        A.mmember[(size_t)g * A.n + k] = j;
    }
    if (tid == 0) {
        int most = 0, at = 0;
        for (int j = 0; j < nmem; j++) if (A.nmatch[m0 + j] > most) { most = A.nmatch[m0 + j]; at = j; }
        A.numBow[g] = sCount; A.most[2 * g] = at; A.most[2 * g + 1] = most;
    }
}

// ---- host -------------------------------------------------------------------------------------------------------------------------------
struct CrrState {
    MirrorBuf<uint8_t> up;                                   // [CrrMem nM | group starts nG + 1]
    MirrorBuf<int32_t> res;                                  // [hist nM 32 | nmatch nM | numBow G | most 2 G | mpoint G n | mmember G n | matches nM n | winner G n]
    DevBuf<int8_t> rotBin;                                   // [nM][n]
    DevBuf<unsigned long long> first;                        // [groups][max_points], stamped
    size_t firstGroups = 0, firstPoints = 0;                 // the shape `first` was allocated for
    uint32_t epoch = 0;
    StageClock clock;
    float stageMs[3] = {0.f, 0.f, 0.f};
};
constexpr size_t kCrrFirstMaxBytes = (size_t)1 << 31;        // the `first` table is refused above 2 GiB (groups x max_points x 8 bytes)

static void crr_destroy(CrrState *s) { delete s; }

static CrrState *crr_state(RumiMatcher *m) {
    MatcherExt *ext = &m->ext;
    if (!ext->state) { ext->state = new NewPtsState(); ext->destroy = newpts_destroy; }
    NewPtsState *np = static_cast<NewPtsState *>(ext->state);
    if (!np->crr) np->crr = new CrrState();
    return np->crr;
}

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
    if (group_start[0] != 0) CRR_REFUSE("group_start must begin at 0");
    int maxGroup = 0;
    for (int g = 0; g < n_groups; g++) {
        if (group_start[g + 1] < group_start[g]) CRR_REFUSE("group_start is not ascending");
        maxGroup = std::max(maxGroup, group_start[g + 1] - group_start[g]);
    }
    const int nM = group_start[n_groups];
    if (nM > 65535) CRR_REFUSE("more than 65535 members");
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
    if ((rc = covis_features_check(c, (int)distinct.size(), distinct.data(), -1, entry, info.data())) != RUMI_OK) return rc;
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
    const size_t G = (size_t)n_groups, Mn = (size_t)nM * n, Gn = G * n;
    if (n == 0 || nM == 0) {                                 // nothing to search: the literal loop leaves every vector NULL.  No device call.
        CrrState *s0 = crr_state(m);
        s0->stageMs[0] = s0->stageMs[1] = s0->stageMs[2] = 0.f;
        if (matches12) for (size_t i = 0; i < Mn; i++) matches12[i] = -1;
        for (int i = 0; i < nM; i++) nmatches[i] = bad[(size_t)i] ? -1 : 0;
        for (size_t i = 0; i < Gn; i++) matched_point[i] = matched_member[i] = -1;
        for (int g = 0; g < n_groups; g++) num_bow_matches[g] = most_matches[2 * g] = most_matches[2 * g + 1] = 0;
        return RUMI_OK;
    }
    // with work to do: the device both handles live on (a store without a device takes the matcher's)
    if ((rc = covis_features_check(c, (int)distinct.size(), distinct.data(), m->device, entry, info.data())) != RUMI_OK) return rc;
#undef CRR_REFUSE
    // ---- device work from here on
    HIP_TRY(hipSetDevice(m->device));
    CrrState *s = crr_state(m);
    s->clock.start(); s->clock.t[0] = t0;
    const size_t memBytes = (size_t)nM * sizeof(CrrMem), upBytes = memBytes + (G + 1) * 4;
    const size_t iHist = 0, iNm = iHist + (size_t)nM * 32, iNum = iNm + nM, iMost = iNum + G, iPoint = iMost + 2 * G, iMember = iPoint + Gn, iMatches = iMember + Gn,
                 iWinner = iMatches + Mn, iEnd = iWinner + Gn;
    if ((rc = s->up.reserve(upBytes, upBytes * 2)) != RUMI_OK || (rc = s->res.reserve(iEnd, iEnd + iEnd / 2)) != RUMI_OK ||
        (rc = s->rotBin.reserve(Mn, Mn + Mn / 2)) != RUMI_OK)
        return rc;
    CrrMem *hm = reinterpret_cast<CrrMem *>(s->up.h);
    for (int i = 0; i < nM; i++) {
        if (bad[(size_t)i]) { hm[i] = CrrMem{0, 0, 0, 0, 1}; continue; }
        const CovisSlotFeatures &I = info[(size_t)at[(size_t)i]];
        hm[i] = CrrMem{(long long)I.block, I.mpOff, I.n, I.nn, 0};
    }
    std::memcpy(s->up.h + memBytes, group_start, (G + 1) * 4);
    s->clock.mark();
    CovisFeatureView fv;
    if ((rc = covis_features_flush(c, &fv)) != RUMI_OK) return rc;
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
    HIP_TRY(hipMemsetAsync(dRes, 0, iNum * 4, nullptr));                                   // histograms and counts
    HIP_TRY(hipMemsetAsync(dRes + iMatches, 0xFF, (iEnd - iMatches) * 4, nullptr));        // matches and winners = -1
    CrrArgs A{};
    A.mem = reinterpret_cast<const CrrMem *>(s->up.d); A.groupStart = reinterpret_cast<const int32_t *>(s->up.d + memBytes);
    A.feat = fv.feat; A.rows = fv.rows; A.pt = fv.pt;
    A.curBlock = (long long)info[curAt].block; A.curMpOff = info[curAt].mpOff; A.n = n; A.nnC = nnC; A.nM = nM; A.nG = n_groups;
    A.words = std::max(1, ((maxN + 15) / 16 + 31) / 32);
    A.epoch = ++s->epoch; A.maxPoints = s->firstPoints; A.first = s->first.p;
    A.hist = dRes + iHist; A.nmatch = dRes + iNm; A.numBow = dRes + iNum; A.most = dRes + iMost; A.mpoint = dRes + iPoint; A.mmember = dRes + iMember;
    A.matches = dRes + iMatches; A.winner = dRes + iWinner; A.rotBin = s->rotBin.p;
    A.nnratio = nnratio; A.checkOri = check_orientation != 0;
    const size_t lds = (size_t)A.words * 256 * 4;
    if (lds > 64 * 1024) HIP_TRY(raise_lds_limit(reinterpret_cast<const void *>(k_crr_match), lds));
    if (nnC > 0 && maxN > 0) hipLaunchKernelGGL(k_crr_match, dim3((nnC + 15) / 16, nM), dim3(256), lds, nullptr, A);
    hipLaunchKernelGGL(k_crr_finish, dim3(nM), dim3(256), 0, nullptr, A);
    if (n_groups > 0) hipLaunchKernelGGL(k_crr_union, dim3(n_groups), dim3(1024), 0, nullptr, A);
    HIP_TRY(hipGetLastError());
    // counts, the groups' rows and (when asked for) the members' rows: the call's one synchronisation
    const size_t backEnd = matches12 ? iWinner : iMatches;
    HIP_TRY(hipMemcpy(s->res.h + iNm, dRes + iNm, (backEnd - iNm) * 4, hipMemcpyDeviceToHost));
    s->clock.mark();
    const int32_t *h = s->res.h;
    std::memcpy(nmatches, h + iNm, (size_t)nM * 4);
    std::memcpy(num_bow_matches, h + iNum, G * 4);
    std::memcpy(most_matches, h + iMost, 2 * G * 4);
    std::memcpy(matched_point, h + iPoint, Gn * 4);
    std::memcpy(matched_member, h + iMember, Gn * 4);
    if (matches12) std::memcpy(matches12, h + iMatches, Mn * 4);
    s->clock.finish(s->stageMs);
    return RUMI_OK;
}

extern "C" int rumi_common_regions_bow_resident_stage_ms(const RumiMatcher *m, float *out3) {
    if (!m || !out3 || !m->ext.state || !static_cast<const NewPtsState *>(m->ext.state)->crr) {
        g_lastError = "rumi_common_regions_bow_resident_stage_ms: no resident common-regions call precedes on this matcher";
        return RUMI_E_INVALID;
    }
    std::memcpy(out3, static_cast<const NewPtsState *>(m->ext.state)->crr->stageMs, 12);
    return RUMI_OK;
}
