// The two resolves of the matcher: the fix-point resolve of every search but one, and SearchForInitialization's in-order replay.  (Included inside namespace rumi.)
// ---- 4. resolve ------------------------------------------------------------------------------------------------
// One workgroup iterates "every query picks its best candidate among the features no EARLIER query holds" to its fixed point (the
// result of the reference's sequential loop).  A round is latency, not work: what a round needs of a query -- count, the head of its
// candidate list, the blocks flag, its current pick -- is read once into registers (the first kResQ queries of a thread, i.e. up to
// 2048 queries; the rest go through global memory as before), the initial occupancy of a thread's features is a bit mask, and a
// round is three barriers over LDS.
constexpr int kResQ = 2, kResK = 4;
__global__ __launch_bounds__(1024) void k_resolve(ResolveArgs A) {
    extern __shared__ int32_t blockedFrom[];      // [nfeat] smallest blocking query index; -1 = taken before the call
    __shared__ int sChanged[2], sHist[RUMI_HISTO_LENGTH], sKeep[RUMI_HISTO_LENGTH], sCount;
    const int tid = threadIdx.x, nt = blockDim.x;
    const int kFree = 0x7FFFFFFF;
    if (A.nq > 0 && *A.overflow != 0) return;
    // ---- read once ----
    int cCnt[kResQ], cAsg[kResQ], cBlocks[kResQ];
    const uint32_t *cList[kResQ];
    uint32_t cHead[kResQ][kResK];
#pragma unroll
    for (int j = 0; j < kResQ; j++) {
        const int i = tid + j * nt;
        cCnt[j] = 0; cAsg[j] = -1; cBlocks[j] = 0; cList[j] = A.lists;
        if (i < A.nq) { cCnt[j] = A.counts[i]; cList[j] = A.lists + A.offsets[i]; cBlocks[j] = A.q[i].blocks; }
#pragma unroll
        for (int k = 0; k < kResK; k++) cHead[j][k] = k < cCnt[j] ? cList[j][k] : 0u;
    }
    for (int i = tid + kResQ * nt; i < A.nq; i += nt) A.assign[i] = -1;
    uint64_t taken0 = 0;                                                    // bit k: feature tid + k nt is taken before the call (nfeat <= 65536: list entries carry 16 bits)
    {
        int k = 0;
        for (int f = tid; f < A.nfeat; f += nt, k++) {
            bool t = false;
            if (A.featBlocked0) t = A.featBlocked0[f] != 0;
            else if (A.mode != MODE_BOW) { const int id = A.featMp[f]; t = id >= 0 && A.mpObs[id] > 0; }
            taken0 |= (uint64_t)t << k;
            blockedFrom[f] = t ? -1 : kFree;
        }
    }
    if (tid < RUMI_HISTO_LENGTH) sHist[tid] = 0;
    if (tid < 2) sChanged[tid] = 0;
    if (tid == 0) sCount = 0;
    auto pick_of = [&](int i, int cnt, const uint32_t *L, const uint32_t *head /* kResK entries in registers, or null */) -> int {
        if (cnt <= 0) return -1;
        int bestDist = 256, bestDist2 = 256, bestLevel = -1, bestLevel2 = -1, bestIdx = -1;
        const bool sortedList = cnt <= kSortMax;                           // then entries come in (distance, candidate order)
        bool done = false;
        auto take = [&](uint32_t e) {
            const int f = (int)(e & 0xFFFF);
            if (blockedFrom[f] < i) return;                                 // taken by an earlier query (or before the call)
            const int d = (int)((e >> 16) & 0x1FF), lv = (int)((e >> 25) & 15);
            if (d < bestDist) { bestDist2 = bestDist; bestDist = d; bestLevel2 = bestLevel; bestLevel = lv; bestIdx = f; }
            else if (d < bestDist2) { bestLevel2 = lv; bestDist2 = d; done = sortedList; }
            else done = sortedList;                                         // equal to the second best: nothing later can change either
        };
        int k = 0;
        if (head) {
#pragma unroll
            for (int h = 0; h < kResK; h++) if (h < cnt && !done) take(head[h]);
            k = kResK;
        }
        for (; k < cnt && !done; k++) take(L[k]);
        int pick = -1;
        if (A.mode == MODE_MAPPOINTS) {                                     // ORBmatcher.cc:106-111
            if (bestDist <= RUMI_TH_HIGH && !(bestLevel == bestLevel2 && (float)bestDist > A.nnratio * (float)bestDist2)) pick = bestIdx;
        } else if (A.mode == MODE_FRAME) {                                  // :1577
            if (bestDist <= RUMI_TH_HIGH) pick = bestIdx;
        } else if (A.mode == MODE_BOW) {                                    // :283-285
            if (bestDist <= RUMI_TH_LOW && (float)bestDist < A.nnratio * (float)bestDist2) pick = bestIdx;
        } else if (A.mode == MODE_BOW_KF) {                                 // :753-754
            if (bestDist < RUMI_TH_LOW && (float)bestDist < A.nnratio * (float)bestDist2) pick = bestIdx;
        } else if (A.mode == MODE_SIM3) {                                   // :463 / :571
            if ((float)bestDist <= A.thrF) pick = bestIdx;
        } else if (A.mode == MODE_FUSE) {                                   // Fuse :1161 / :1277 (TH_LOW), SearchBySim3 :1399 / :1475 (TH_HIGH)
            if (bestDist <= A.thrI) pick = bestIdx;
        } else {                                                            // MODE_RELOC :1757
            if (bestDist <= A.thrI) pick = bestIdx;
        }
        return pick;
    };
    for (int round = 0; round <= A.nq + 1; round++) {
        __syncthreads();                                                    // occupancy reset (below, or the initial one above) visible
        // occupancy as the previous round's assignments imply it
#pragma unroll
        for (int j = 0; j < kResQ; j++)
            if (cAsg[j] >= 0 && cBlocks[j]) atomicMin(&blockedFrom[cAsg[j]], tid + j * nt);
        for (int i = tid + kResQ * nt; i < A.nq; i += nt) {
            const int f = A.assign[i];
            if (f >= 0 && A.q[i].blocks) atomicMin(&blockedFrom[f], i);
        }
        __syncthreads();
        int changed = 0;
#pragma unroll
        for (int j = 0; j < kResQ; j++) {
            const int i = tid + j * nt;
            if (i >= A.nq) continue;
            const int pick = pick_of(i, cCnt[j], cList[j], cHead[j]);
            if (pick != cAsg[j]) { changed = 1; cAsg[j] = pick; }
        }
        for (int i = tid + kResQ * nt; i < A.nq; i += nt) {
            const int pick = pick_of(i, A.counts[i], A.lists + A.offsets[i], nullptr);
            if (pick != A.assign[i]) { changed = 1; A.assign[i] = pick; }
        }
        if (changed) sChanged[round & 1] = 1;
        __syncthreads();
        const int any = sChanged[round & 1];
        if (tid == 0) sChanged[(round + 1) & 1] = 0;                        // last read before this round's barriers, next written after the next round's
        if (!any) break;
        int k = 0;
        for (int f = tid; f < A.nfeat; f += nt, k++) blockedFrom[f] = ((taken0 >> k) & 1) ? -1 : kFree;
    }
#pragma unroll
    for (int j = 0; j < kResQ; j++) { const int i = tid + j * nt; if (i < A.nq) A.assign[i] = cAsg[j]; }
    // results: a feature keeps the LAST query that assigned it (later assignments overwrite, as in the loop)
    int32_t *last = blockedFrom;                                        // reuse LDS: last assigning query per feature
    for (int f = tid; f < A.nfeat; f += nt) last[f] = -1;
    __syncthreads();
    const bool useHist = A.checkOri && A.mode != MODE_MAPPOINTS && A.mode != MODE_SIM3;
    int local = 0;
    auto assigned = [&](int i, int j) { return j == 0 ? cAsg[0] : j == 1 ? cAsg[1] : A.assign[i]; };
    static_assert(kResQ == 2, "assigned() spells the register copies out");
    for (int i = tid, j = 0; i < A.nq; i += nt, j++) {
        const int f = assigned(i, j);
        if (f < 0) continue;
        local++;
        atomicMax(&last[f], i);
        if (useHist) atomicAdd(&sHist[rot_bin(A.q[i].angle, A.featKeys[f].angle)], 1);
    }
    if (local) atomicAdd(&sCount, local);
    __syncthreads();
    if (tid < 64) {                                                      // ComputeThreeMaxima by the lanes of one wave
        int removed;
        const int keep = three_maxima_wave(tid < RUMI_HISTO_LENGTH ? sHist[tid] : 0, useHist, &removed);
        if (tid < RUMI_HISTO_LENGTH) sKeep[tid] = keep;
        if (tid == 0) *A.nmatches = sCount - removed;
    }
    __syncthreads();
    // MODE_BOW starts from an all-NULL vector (ORBmatcher.cc:201); the other modes update the frame's vector in place
    if (A.mode == MODE_BOW)
        for (int f = tid; f < A.nfeat; f += nt) A.featMp[f] = -1;
    __syncthreads();
    if (A.mode != MODE_BOW_KF)
        for (int f = tid; f < A.nfeat; f += nt)
            if (last[f] >= 0) A.featMp[f] = A.q[last[f]].mpId;
    __syncthreads();
    if (useHist)                                                        // entries of the rejected bins are set to NULL
        for (int i = tid, j = 0; i < A.nq; i += nt, j++) {
            const int f = assigned(i, j);
            if (f >= 0 && !sKeep[rot_bin(A.q[i].angle, A.featKeys[f].angle)]) {
                if (A.mode == MODE_BOW_KF) A.assign[i] = -1;           // SearchByBoW(KF,KF) reports per QUERY (vpMatches12[idx1])
                else A.featMp[f] = -1;
            }
        }
    if (A.gXw) {                                                        // (uniform) the Tracking step's next launch would be this gather
        __shared__ int sGatherWave[16], sGatherBase;
        __syncthreads();                                                // the vector is final
        gather_correspondences(A.nfeat, A.featKeys, A.featMp, A.gMpPos, A.gInvSigma2, A.gXw, A.gObs, A.gW, A.gIdx, A.gStart, A.gSnapshot, sGatherWave, &sGatherBase);
    }
}

// SearchForInitialization resolve (ORBmatcher.cc:593-679).  The skip rule `vMatchedDistance[i2] <= dist` makes every query depend
// on the best distance accepted so far for each candidate, so the queries are replayed IN ORDER by one wave; the lanes share the
// candidate list of the current query.  Called once per initialisation attempt (a few thousand queries): latency, not throughput.
struct InitArgs {
    int n1, n2;
    const Query *q;
    const int32_t *counts, *offsets;
    const uint32_t *lists;
    const RumiKeyPoint *keys2;
    int32_t *matches12;             // out [n1]
    float *prevMatched;             // in/out [n1][2]
    int32_t *nmatches;
    float nnratio;
    int checkOri;
    const int32_t *overflow;
};

__global__ __launch_bounds__(64) void k_resolve_init(InitArgs A) {
    extern __shared__ int32_t sInit[];          // matchedDist[n2] | matches21[n2]
    __shared__ int sHist[RUMI_HISTO_LENGTH], sKeep[RUMI_HISTO_LENGTH];
    int32_t *matchedDist = sInit, *matches21 = sInit + A.n2;
    const int lane = threadIdx.x;
    const int kInf = 0x7FFFFFFF;
    if (*A.overflow != 0) return;
    for (int f = lane; f < A.n2; f += 64) { matchedDist[f] = kInf; matches21[f] = -1; }
    for (int i = lane; i < A.n1; i += 64) A.matches12[i] = -1;
    if (lane < RUMI_HISTO_LENGTH) sHist[lane] = 0;
    __syncthreads();
    int nmatches = 0;
    for (int i1 = 0; i1 < A.n1; i1++) {
        const int cnt = A.counts[i1];
        if (cnt == 0) continue;
        const uint32_t *L = A.lists + A.offsets[i1];
        int b1 = kInf, b2 = kInf, bKey = kInf;            // best, second-best distance; best as dist<<16 | list position
        int bFeat = -1;
        for (int k = lane; k < cnt; k += 64) {
            const uint32_t e = L[k];
            const int f = (int)(e & 0xFFFF), d = (int)((e >> 16) & 0x1FF);
            if (matchedDist[f] <= d) continue;                            // :617
            if (d < b1) { b2 = b1; b1 = d; bKey = (d << 16) | k; bFeat = f; }
            else if (d < b2) b2 = d;
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const int c1 = __shfl_xor(b1, o), c2 = __shfl_xor(b2, o), cKey = __shfl_xor(bKey, o), cFeat = __shfl_xor(bFeat, o);
            b2 = min(max(b1, c1), min(b2, c2));
            b1 = min(b1, c1);
            if (cKey < bKey) { bKey = cKey; bFeat = cFeat; }
        }
        // :629-638 (uniform across the wave)
        if (b1 <= RUMI_TH_LOW && (float)b1 < (float)b2 * A.nnratio) {
            if (lane == 0) {
                const int prev = matches21[bFeat];
                if (prev >= 0) A.matches12[prev] = -1;
                A.matches12[i1] = bFeat;
                matches21[bFeat] = i1;
                matchedDist[bFeat] = b1;
                if (A.checkOri) sHist[rot_bin(A.q[i1].angle, A.keys2[bFeat].angle)]++;
            }
            __syncthreads();
        }
    }
    __syncthreads();
    if (lane == 0) {
        for (int i = 0; i < RUMI_HISTO_LENGTH; i++) sKeep[i] = 1;
        if (A.checkOri) three_maxima_keep(sHist, sKeep);                    // over ALL accepted (also stolen) entries
    }
    __syncthreads();
    // a surviving match keeps the bin it was accepted with (its feature never changes afterwards): :661-677
    for (int i = lane; i < A.n1; i += 64) {
        int f = A.matches12[i];
        if (f >= 0 && A.checkOri && !sKeep[rot_bin(A.q[i].angle, A.keys2[f].angle)]) { A.matches12[i] = -1; f = -1; }
        if (f >= 0) { nmatches++; A.prevMatched[2 * i] = A.keys2[f].x; A.prevMatched[2 * i + 1] = A.keys2[f].y; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) nmatches += __shfl_xor(nmatches, o);
    if (lane == 0) *A.nmatches = nmatches;
}
