// ORBmatcher::SearchByProjection(Frame&, KeyFrame*, sAlreadyFound, th, ORBdist) (R/lib_src/ORBmatcher.cc:1685-1793) for every live pose
// hypothesis of rumi_track_reloc_refine in one pass (DESIGN.md 4y).  Included by match.hip inside namespace rumi; launched through
// launch_reloc_search (match_host.h) from track.hip.  The shape is sim3_projection_batch.inc's: a wave per (hypothesis, key-frame feature), count /
// allocate / fill, one ordered fix-point resolve per hypothesis.
//
//   k_reloc_walk<false>  the gate of k_queries_reloc (reloc_query, match_device.h: one body for both; the single entry keeps its own kernel) with
//                        skip = bad | sFound bitmap and the hypothesis' own pose and camera centre (se3f_camera_centre), the query kept for the
//                        later passes; then the window walk of candidates_walk in GetFeaturesInArea order (cell_window, window_gate: match_grid.h),
//                        COUNTING the candidates within ORBdist; lane 0 takes the list space with one atomicAdd on the stage's total.
//   k_reloc_walk<true>   the same walk FILLS (distance << 20 | place among the kept, feature).  Exact for any list length.
//   k_reloc_resolve      k_resolve's MODE_RELOC body, one workgroup per hypothesis: blockedFrom[nfeat] in LDS seeded from featMp[h][f] >= 0,
//                        the fix point, the rotation histogram and ComputeThreeMaxima, the frame's vector; thread 0 then decides the next stage.
// Only candidates within ORBdist are kept: MODE_RELOC accepts the best free candidate iff its distance is within that bound and reads no second
// best, so a farther candidate can never be picked and, while a nearer one is free, never shadows it.  Ties: strict `<` in candidate order = the
// minimum key.  A hypothesis whose live bit is clear costs one wave-uniform load per workgroup.  Integer atomics only; where a list lies depends
// on arrival, no result does.  When the lists outgrow the arena the fill and the resolve do nothing and the host repeats the whole refine with
// a larger one.

template <bool FILL>
__global__ __launch_bounds__(256) void k_reloc_walk(RelocSearchArgs A) {
    const int h = blockIdx.y;
    const int live = __builtin_amdgcn_readfirstlane(A.hyp[h].live);
    if (!(live & (A.stage == 0 ? RELOC_LIVE_S1 : RELOC_LIVE_S2))) return;
    if (FILL && (uint32_t)A.head[A.stage] > (uint32_t)A.listCap) return;
    const RelocCand C = A.cands[__builtin_amdgcn_readfirstlane(A.hyp[h].cand)];
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (i >= C.nkf) return;
    const size_t pair = (size_t)h * A.maxNkf + i;
    const FrameDev &F = A.fd;
    Query Q{};
    if (!FILL) {                                            // ORBmatcher.cc:1700-1733
        const int mp = A.kfMp[C.keyOff + i];
        const float *Tcw = A.T + (size_t)h * 7;
        float Ow[3];
        se3f_camera_centre(Tcw, Ow);
        Q = reloc_query(mp, mp >= 0 && (A.bad[mp] | ((A.found[(size_t)h * A.words + (mp >> 5)] >> (mp & 31)) & 1u)), A.pos, A.minD, A.maxD, Tcw, A.K, Ow,
                        F.scale, A.nLevels, A.logSf, A.th, F.minX, F.minY, F.maxX, F.maxY, A.kfKeys[C.keyOff + i].angle);
        if (lane == 0) A.q[pair] = Q;
    } else Q = A.q[pair];
    if (!Q.valid) {
        if (!FILL && lane == 0) { A.pairCount[pair] = 0; A.pairBase[pair] = 0; }
        return;
    }
    uint32_t qd[8];
    {
        const uint32_t mine = reinterpret_cast<const uint32_t *>(A.desc + (size_t)Q.descId * 32)[lane & 7];
#pragma unroll
        for (int k = 0; k < 8; k++) qd[k] = __shfl(mine, k);
    }
    const int listAt = FILL ? A.pairBase[pair] : 0, listLen = FILL ? A.pairCount[pair] : 0;
    int count = 0;
    // Frame::GetFeaturesInArea (Frame.cc:695-750), as candidates_walk visits it
    const CellWindow W = cell_window(Q.u, Q.v, Q.r, F.minX, F.minY, F.wInv, F.hInv);
    if (W.any) {
        for (int ix = W.x0; ix <= W.x1; ix++) {
            const int p0 = F.cellStart[ix * kGridRows + W.y0], p1 = F.cellStart[ix * kGridRows + W.y1 + 1];
            for (int base = p0; base < p1; base += 64) {
                const int p = base + lane;
                bool pass = false;
                int idx = 0, d = 0;
                if (p < p1) {
                    idx = F.sortedIdx[p];
                    const RumiKeyPoint kp = F.keys[idx];
                    pass = window_gate(kp, Q.u, Q.v, Q.r, Q.minLevel, Q.maxLevel);    // (maxLevel >= 1 here: the level test always applies)
                    if (pass && (uint32_t)idx < (uint32_t)A.nfeat) {
                        d = hamming256(qd, reinterpret_cast<const uint32_t *>(F.desc + (size_t)idx * 32));
                        if (d > A.orbDist) pass = false;                        // the cut (above)
                    } else pass = false;
                }
                const unsigned long long b = __ballot(pass);
                if (FILL && pass) {
                    const int pos = count + __popcll(b & ((1ull << lane) - 1ull));
                    if (pos < listLen && (uint32_t)(listAt + pos) < (uint32_t)A.listCap)
                        A.lists[listAt + pos] = make_uint2(((uint32_t)d << 20) | (uint32_t)pos, (uint32_t)idx);
                }
                count += __popcll(b);
            }
        }
    }
    if (!FILL && lane == 0) {
        A.pairCount[pair] = count;
        A.pairBase[pair] = count ? atomicAdd(&A.head[A.stage], count) : 0;
    }
}

constexpr int kRelocResolveThreads = 1024;
__global__ __launch_bounds__(kRelocResolveThreads) void k_reloc_resolve(RelocSearchArgs A) {
    extern __shared__ int32_t sBlockedFrom[];                // [nfeat] the smallest entry that holds the feature; -1: held before the search
    __shared__ int sChanged[2], sHist[RUMI_HISTO_LENGTH], sKeep[RUMI_HISTO_LENGTH], sCount;
    const int h = blockIdx.x;
    RelocHyp &R = A.hyp[h];
    const int live = __builtin_amdgcn_readfirstlane(R.live);
    if (!(live & (A.stage == 0 ? RELOC_LIVE_S1 : RELOC_LIVE_S2))) return;
    if ((uint32_t)A.head[A.stage] > (uint32_t)A.listCap) return;            // the host repeats the call with a larger arena
    const int tid = threadIdx.x, nt = kRelocResolveThreads, nfeat = A.nfeat;
    const RelocCand C = A.cands[__builtin_amdgcn_readfirstlane(R.cand)];
    const int nq = C.nkf;
    const int kFree = 0x7FFFFFFF;
    const size_t pair0 = (size_t)h * A.maxNkf;
    const int32_t *cnt = A.pairCount + pair0, *off = A.pairBase + pair0;
    const Query *q = A.q + pair0;
    int32_t *asg = A.asg + pair0;
    int32_t *featMp = A.featMp + (size_t)h * nfeat;
    for (int i = tid; i < nq; i += nt) asg[i] = -1;
    for (int f = tid; f < nfeat; f += nt) sBlockedFrom[f] = featMp[f] >= 0 ? -1 : kFree;       // CurrentFrame.mvpMapPoints[i2] != NULL (:1746)
    if (tid < RUMI_HISTO_LENGTH) sHist[tid] = 0;
    if (tid < 2) sChanged[tid] = 0;
    if (tid == 0) sCount = 0;
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
            if ((uint32_t)(off[i] + c) > (uint32_t)A.listCap) continue;      // (cannot happen below the total that was checked above)
            const uint2 *L = A.lists + off[i];
            uint32_t bestKey = 0xFFFFFFFFu;
            int pick = -1;
            for (int k = 0; k < c; k++) {
                const uint2 e = L[k];
                if (sBlockedFrom[e.y] < i) continue;         // taken by an earlier key-frame feature, or before the search
                if (e.x < bestKey) { bestKey = e.x; pick = (int)e.y; }
            }
            if (pick != asg[i]) { changed = 1; asg[i] = pick; }
        }
        if (changed) sChanged[round & 1] = 1;
        __syncthreads();
        const int any = sChanged[round & 1];
        if (tid == 0) sChanged[(round + 1) & 1] = 0;         // last read before this round's barriers, next written after the next round's
        if (!any) break;
        for (int f = tid; f < nfeat; f += nt) sBlockedFrom[f] = featMp[f] >= 0 ? -1 : kFree;
    }
    // rotation histogram and ComputeThreeMaxima in the one-wave form (ORBmatcher.cc:1759-1790, :1795-1826)
    __syncthreads();
    const RumiKeyPoint *featKeys = A.fd.keys;
    int local = 0;
    for (int i = tid; i < nq; i += nt) {
        const int f = asg[i];
        if (f < 0) continue;
        local++;
        if (A.checkOri) atomicAdd(&sHist[rot_bin(q[i].angle, featKeys[f].angle)], 1);
    }
    if (local) atomicAdd(&sCount, local);
    __syncthreads();
    if (tid < 64) {
        int removed;
        const int keep = three_maxima_wave(tid < RUMI_HISTO_LENGTH ? sHist[tid] : 0, A.checkOri, &removed);
        if (tid < RUMI_HISTO_LENGTH) sKeep[tid] = keep;
        if (tid == 0) {
            // the stage's decision: Tracking.cc:3317 (S1, with P1's nGood) / :3330 (S2, with P2's)
            const int nadd = sCount - removed, nGood = R.ngood[A.stage];
            R.nadd[A.stage] = nadd;
            if (nGood + nadd >= A.enough) {
                R.ran |= A.stage == 0 ? 8 : 32;
                R.live = live | (A.stage == 0 ? RELOC_LIVE_P2 : RELOC_LIVE_P3);
            } else R.ngoodFinal = nGood;
        }
    }
    __syncthreads();
    for (int i = tid; i < nq; i += nt) {                    // a feature is held by at most one entry (every valid query blocks)
        const int f = asg[i];
        if (f >= 0 && (!A.checkOri || sKeep[rot_bin(q[i].angle, featKeys[f].angle)])) featMp[f] = q[i].mpId;
    }
}
