// Tracking::Relocalization's refine chain (R/lib_src/Tracking.cc:3287-3345) for every pose hypothesis of a round in one call, behind
// rumi_track_reloc_begin / rumi_track_reloc_refine (include/rumi_track.h, DESIGN.md 4y).  Included at the end of track.hip.  The searches are
// match_reloc_batch.inc's (launch_reloc_search), the optimisations k_pose_opt's batch form (pose_opt_device with a batch count); the kernels
// here seed a hypothesis, gather its correspondences, and run what follows an optimisation.  Every kernel is launched once for all hypotheses
// (hypothesis = blockIdx.x, one workgroup each); a hypothesis whose live bit for the stage is clear returns after one wave-uniform load.
// No host read between the seed and the one copy back.
//
//   k_reloc_seed    mvpMapPoints from matches[cand] and vbInliers, sFound as a bitmap by atomicOr, outlier_last = 255, the record; then P1's
//                   correspondences in feature order (block_ordered_slot, as gather_correspondences) at start[h].  start[h] is the number of
//                   correspondences of the hypotheses before h, which the workgroup counts itself: no scan launch.
//   k_reloc_gather  the same gather from featMp[h] for P2 / P3 (count 0 for a hypothesis that does not run it: k_pose_opt then leaves its pose).
//   k_reloc_after   outlier_last from the optimisation's flags, the nulling loops (:3309, :3333), the count compares (:3306, :3314, :3322), and
//                   before S2 the bitmap rebuilt from every non-NULL slot (:3323-3326); after P3 the pose into the record.

namespace rumi {

struct RelocArgs {
    int H, n, words;
    const RelocHyp *hypIn;               // as uploaded: cand
    RelocHyp *hyp;                       // the records of the result block
    const RelocCand *cands;
    const int32_t *matches;              // [K][n]
    const uint8_t *inl;                  // [H][n]
    const float *Tin;                    // [H][7]
    const RumiKeyPoint *keys;
    const float *pos, *invSigma2;
    int32_t *featMp;                     // [H][n]
    uint8_t *outLast;                    // [H][n]
    uint32_t *found;                     // [H][words]
    float *T;                            // [H][7]
    float *Xw, *obs, *w;
    int32_t *idx, *start;                // [H n], [H + 1]
    const uint8_t *outC;
    const int32_t *nGood;                // [3][H]
    int minGood, enough, retryAbove;
};

// The correspondences of hypothesis h (the features with mp(f) >= 0, in feature order) behind those of the hypotheses before it, whose number is
// counted with `before(hp, f)`.  One workgroup of 1024 threads.
template <class Before, class Mp>
__device__ __forceinline__ void reloc_gather(const RelocArgs &A, int h, Before before, Mp mpOf) {
    __shared__ int sWave[16], sBase;
    const int tid = threadIdx.x;
    if (tid == 0) sBase = 0;
    __syncthreads();
    int mine = 0;
    for (int hp = 0; hp < h; hp++)
        for (int f = tid; f < A.n; f += 1024) mine += before(hp, f) ? 1 : 0;
    if (mine) atomicAdd(&sBase, mine);
    __syncthreads();
    const int base = sBase;
    for (int c0 = 0; c0 < A.n; c0 += 1024) {
        const int i = c0 + tid;
        const int mp = i < A.n ? mpOf(i) : -1;
        block_ordered_slot(mp >= 0, sWave, &sBase, [&](int c) { correspondence_store(c, i, mp, A.keys, A.pos, A.invSigma2, A.Xw, A.obs, A.w, A.idx); });
    }
    if (tid == 0) { A.start[h] = base; if (h == A.H - 1) A.start[A.H] = sBase; }
}

__global__ __launch_bounds__(1024) void k_reloc_seed(RelocArgs A) {
    const int h = blockIdx.x, tid = threadIdx.x;
    const int32_t *match = A.matches + (size_t)A.hypIn[h].cand * A.n;
    const uint8_t *inl = A.inl + (size_t)h * A.n;
    uint32_t *found = A.found + (size_t)h * A.words;
    for (int k = tid; k < A.words; k += 1024) found[k] = 0;
    if (tid == 0) {
        RelocHyp R{};
        R.ran = 1; R.ngoodFinal = -1; R.cand = A.hypIn[h].cand;
        for (int k = 0; k < 7; k++) R.T[k] = A.Tin[(size_t)h * 7 + k];
        A.hyp[h] = R;
    }
    if (tid < 7) A.T[(size_t)h * 7 + tid] = A.Tin[(size_t)h * 7 + tid];
    __syncthreads();
    for (int f = tid; f < A.n; f += 1024) {                 // Tracking.cc:3296-3302
        const int mp = inl[f] ? match[f] : -1;
        A.featMp[(size_t)h * A.n + f] = mp;
        A.outLast[(size_t)h * A.n + f] = 255;
        if (mp >= 0) atomicOr(&found[mp >> 5], 1u << (mp & 31));
    }
    reloc_gather(A, h,
                 [&](int hp, int f) { return A.inl[(size_t)hp * A.n + f] && A.matches[(size_t)A.hypIn[hp].cand * A.n + f] >= 0; },
                 [&](int f) { return inl[f] ? match[f] : -1; });
}

__global__ __launch_bounds__(1024) void k_reloc_gather(RelocArgs A, int liveBit) {
    const int h = blockIdx.x;
    const bool live = (__builtin_amdgcn_readfirstlane(A.hyp[h].live) & liveBit) != 0;
    reloc_gather(A, h,
                 [&](int hp, int f) { return (A.hyp[hp].live & liveBit) && A.featMp[(size_t)hp * A.n + f] >= 0; },
                 [&](int f) { return live ? A.featMp[(size_t)h * A.n + f] : -1; });
}

// stage 0 / 1 / 2: behind P1 / P2 / P3
__global__ __launch_bounds__(1024) void k_reloc_after(RelocArgs A, int stage) {
    const int h = blockIdx.x, tid = threadIdx.x;
    RelocHyp &R = A.hyp[h];
    const int live = __builtin_amdgcn_readfirstlane(R.live);
    const bool ran = stage == 0 || (live & (stage == 1 ? RELOC_LIVE_P2 : RELOC_LIVE_P3));
    if (ran) {
        const int nG = A.nGood[(size_t)stage * A.H + h];
        const bool pass = stage != 0 || nG >= A.minGood;                               // :3306
        const bool null = stage == 2 || (stage == 0 && pass);                          // :3309 / :3333; none after P2
        const bool search = stage == 0 ? pass && nG < A.enough                         // :3314
                                       : stage == 1 && nG > A.retryAbove && nG < A.enough;   // :3322
        int32_t *featMp = A.featMp + (size_t)h * A.n;
        uint8_t *outLast = A.outLast + (size_t)h * A.n;
        for (int c = A.start[h] + tid; c < A.start[h + 1]; c += 1024) {
            const int f = A.idx[c];
            const uint8_t o = A.outC[c];
            outLast[f] = o;
            if (null && o) featMp[f] = -1;
        }
        if (stage == 1 && search) {                                                    // :3323-3326 (P2's outliers are still in the frame)
            uint32_t *found = A.found + (size_t)h * A.words;
            for (int k = tid; k < A.words; k += 1024) found[k] = 0;
            __syncthreads();
            for (int f = tid; f < A.n; f += 1024) {
                const int mp = featMp[f];
                if (mp >= 0) atomicOr(&found[mp >> 5], 1u << (mp & 31));
            }
        }
        if (tid == 0) {
            R.ngood[stage] = nG;
            if (stage == 0 && pass) R.ran |= 2;
            if (search) { R.ran |= stage == 0 ? 4 : 16; R.live = live | (stage == 0 ? RELOC_LIVE_S1 : RELOC_LIVE_S2); }
            else R.ngoodFinal = pass ? nG : -1;
        }
    }
    if (stage == 2 && tid < 7) R.T[tid] = A.T[(size_t)h * 7 + tid];
}

// What a Relocalization call keeps on the device between begin and its refine calls, and the blocks of a refine call (grown on demand).
struct RelocState {
    bool open = false;
    uint32_t serial = 0;                 // the resident frame the session was begun on
    int K = 0, nmp = 0, maxNkf = 0, words = 0, n = 0;
    std::vector<int32_t> nkf;
    float K4[4] = {0, 0, 0, 0};
    FrameDev fd{};
    MirrorBuf<uint8_t> sess;             // [cands | keys | rows | matches | pos | minD | maxD | bad | desc | K4]
    size_t oKeys = 0, oRows = 0, oMatch = 0, oPos = 0, oMin = 0, oMax = 0, oBad = 0, oDesc = 0, oK4 = 0;
    MirrorBuf<uint8_t> up, res;          // [RelocHyp H | Tin | inliers]; [head 4 | RelocHyp H | featMp H n | outLast H n]
    DevBuf<uint32_t> found;
    DevBuf<float> fl;                    // T, Xw, obs, w
    DevBuf<int32_t> in;                  // idx, start, nGood, pairCount, pairBase, asg
    DevBuf<uint8_t> by;                  // outC, active
    DevBuf<double> chi;
    DevBuf<Query> q;
    DevBuf<uint2> lists;
    int attempts = 0;                    // of the last refine (1: the lists fitted their arena)
};
void reloc_release(RelocState *s) { delete s; }

}  // namespace rumi

extern "C" void rumi_reloc_default_params(RumiRelocParams *p) {
    if (!p) return;
    p->min_good = 10; p->enough = 50; p->retry_above = 30;
    p->th_coarse = 10.f; p->dist_coarse = 100; p->th_fine = 3.f; p->dist_fine = 64; p->check_orientation = 1;
}

extern "C" int rumi_track_reloc_begin(RumiTracker *t, const float *K4, int32_t K, const RumiRelocCandidate *cands, const RumiTrackPoints *pts) {
    static const char *entry = "rumi_track_reloc_begin";
    if (!t || !K4 || K < 0 || (K > 0 && !cands) || !pts || pts->n < 0 ||
        (pts->n > 0 && (!pts->pos || !pts->min_dist || !pts->max_dist || !pts->desc || !pts->bad))) {
        g_lastError = std::string(entry) + ": missing argument or negative count";
        return RUMI_E_INVALID;
    }
    if (t->curN < 0) { g_lastError = std::string(entry) + ": no frame is resident (rumi_track_extract first)"; return RUMI_E_INVALID; }
    const int n = t->curN, nmp = pts->n;
    if (nmp > t->maxPts) { g_lastError = std::string(entry) + ": more points than the tracker was created for"; return RUMI_E_CAPACITY; }
    size_t keysAll = 0;
    int maxNkf = 0;
    for (int k = 0; k < K; k++) {
        const RumiRelocCandidate &C = cands[k];
        if (C.nkf < 0 || (C.nkf > 0 && (!C.kf_keys || !C.kf_mp)) || (n > 0 && !C.matches)) {
            g_lastError = std::string(entry) + ": a candidate with a missing array or a negative count";
            return RUMI_E_INVALID;
        }
        for (int i = 0; i < C.nkf; i++)
            if (C.kf_mp[i] < -1 || C.kf_mp[i] >= nmp) { g_lastError = std::string(entry) + ": a kf_mp id outside the point table"; return RUMI_E_INVALID; }
        for (int f = 0; f < n; f++)
            if (C.matches[f] < -1 || C.matches[f] >= nmp) { g_lastError = std::string(entry) + ": a matches id outside the point table"; return RUMI_E_INVALID; }
        keysAll += (size_t)C.nkf; maxNkf = std::max(maxNkf, C.nkf);
    }
    if (keysAll > 0x7FFFFFFF / sizeof(RumiKeyPoint)) { g_lastError = std::string(entry) + ": the candidates' key-points exceed a 31-bit offset"; return RUMI_E_CAPACITY; }
    HIP_TRY(hipSetDevice(t->device));
    if (!t->reloc) t->reloc = new RelocState();
    RelocState *s = t->reloc;
    s->open = false;
    s->oKeys = up16((size_t)K * sizeof(RelocCand)); s->oRows = up16(s->oKeys + keysAll * sizeof(RumiKeyPoint)); s->oMatch = up16(s->oRows + keysAll * 4);
    s->oPos = up16(s->oMatch + (size_t)K * n * 4); s->oMin = up16(s->oPos + (size_t)nmp * 12); s->oMax = up16(s->oMin + (size_t)nmp * 4);
    s->oBad = up16(s->oMax + (size_t)nmp * 4); s->oDesc = up16(s->oBad + (size_t)nmp); s->oK4 = up16(s->oDesc + (size_t)nmp * 32);
    const size_t bytes = s->oK4 + 16;
    int rc;
    if ((rc = s->sess.reserve(bytes, bytes + bytes / 4)) != RUMI_OK) return rc;
    uint8_t *hs = s->sess.h;
    RelocCand *hc = reinterpret_cast<RelocCand *>(hs);
    s->nkf.resize((size_t)K);
    size_t at = 0;
    for (int k = 0; k < K; k++) {
        const RumiRelocCandidate &C = cands[k];
        hc[k] = RelocCand{C.nkf, (int32_t)at};
        s->nkf[(size_t)k] = C.nkf;
        if (C.nkf > 0) {
            std::memcpy(hs + s->oKeys + at * sizeof(RumiKeyPoint), C.kf_keys, (size_t)C.nkf * sizeof(RumiKeyPoint));
            std::memcpy(hs + s->oRows + at * 4, C.kf_mp, (size_t)C.nkf * 4);
        }
        if (n > 0) std::memcpy(hs + s->oMatch + (size_t)k * n * 4, C.matches, (size_t)n * 4);
        at += (size_t)C.nkf;
    }
    if (nmp > 0) {
        std::memcpy(hs + s->oPos, pts->pos, (size_t)nmp * 12); std::memcpy(hs + s->oMin, pts->min_dist, (size_t)nmp * 4);
        std::memcpy(hs + s->oMax, pts->max_dist, (size_t)nmp * 4); std::memcpy(hs + s->oBad, pts->bad, (size_t)nmp);
        std::memcpy(hs + s->oDesc, pts->desc, (size_t)nmp * 32);
    }
    std::memcpy(hs + s->oK4, K4, 16);
    HIP_TRY(hipMemcpyAsync(s->sess.d, hs, bytes, hipMemcpyHostToDevice, nullptr));
    // the resident frame as the matcher's kernels address it, and its grid (one for all hypotheses)
    t->projN = 0;
    FrameDev fd;
    if ((rc = track_frame_dev(t, &fd)) != RUMI_OK) return rc;
    RumiMatcher *m = t->m;
    FLUSH(m);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(nullptr));                  // once per Relocalization: the pinned block is the caller's to refill afterwards
    s->fd = fd; s->K = K; s->nmp = nmp; s->maxNkf = maxNkf; s->words = (nmp + 31) / 32 + 1; s->n = n;
    std::memcpy(s->K4, K4, 16);
    s->serial = t->frameSerial;
    s->open = true;
    return RUMI_OK;
}

extern "C" int rumi_track_reloc_refine(RumiTracker *t, const RumiRelocParams *p, int32_t H, const RumiRelocHypothesis *hyp, int32_t *frame_mp,
                                       uint8_t *outlier_last, RumiRelocResult *res) {
    static const char *entry = "rumi_track_reloc_refine";
    if (!t || H < 0 || (H > 0 && (!hyp || !frame_mp || !outlier_last || !res))) { g_lastError = std::string(entry) + ": missing argument or negative count"; return RUMI_E_INVALID; }
    RelocState *s = t->reloc;
    if (!s || !s->open || t->curN < 0 || s->serial != t->frameSerial) {
        g_lastError = std::string(entry) + ": no rumi_track_reloc_begin precedes on the resident frame";
        return RUMI_E_INVALID;
    }
    if (H > RUMI_RELOC_MAX_HYPOTHESES) { g_lastError = std::string(entry) + ": more than RUMI_RELOC_MAX_HYPOTHESES hypotheses"; return RUMI_E_CAPACITY; }
    for (int h = 0; h < H; h++) {
        if (hyp[h].cand < 0 || hyp[h].cand >= s->K) { g_lastError = std::string(entry) + ": a hypothesis names a candidate outside [0, K)"; return RUMI_E_INVALID; }
        if (!hyp[h].inliers) { g_lastError = std::string(entry) + ": a hypothesis without inlier flags"; return RUMI_E_INVALID; }
        for (int k = 0; k < 7; k++) if (!std::isfinite(hyp[h].Tcw7[k])) { g_lastError = std::string(entry) + ": a pose that is not finite"; return RUMI_E_INVALID; }
    }
    if (H == 0) return RUMI_OK;
    RumiRelocParams P;
    if (p) P = *p; else rumi_reloc_default_params(&P);
    HIP_TRY(hipSetDevice(t->device));
    const size_t n = (size_t)s->n, Hn = (size_t)H * n, pairs = (size_t)H * (size_t)std::max(s->maxNkf, 1);
    const size_t uT = up16((size_t)H * sizeof(RelocHyp)), uInl = up16(uT + (size_t)H * 28), upBytes = up16(uInl + Hn);
    const size_t rHyp = 16, rMp = up16(rHyp + (size_t)H * sizeof(RelocHyp)), rOut = up16(rMp + Hn * 4), resBytes = up16(rOut + Hn);
    const size_t fT = 0, fX = fT + (size_t)H * 8, fO = fX + Hn * 3, fW = fO + Hn * 2, flN = fW + Hn;
    const size_t iIdx = 0, iStart = iIdx + Hn, iGood = iStart + (size_t)H + 1, iCnt = iGood + 3 * (size_t)H, iBase = iCnt + pairs, iAsg = iBase + pairs, inN = iAsg + pairs;
    const size_t listFirst = std::min<size_t>(4 * pairs + 4096, 0x7FFFFFFF);
    int rc;
    if ((rc = s->up.reserve(upBytes, upBytes + upBytes / 2)) != RUMI_OK || (rc = s->res.reserve(resBytes, resBytes + resBytes / 2)) != RUMI_OK ||
        (rc = s->found.reserve((size_t)H * s->words, (size_t)H * s->words * 2)) != RUMI_OK || (rc = s->fl.reserve(flN, flN + flN / 2)) != RUMI_OK ||
        (rc = s->in.reserve(inN, inN + inN / 2)) != RUMI_OK || (rc = s->by.reserve(2 * Hn + 16, 3 * Hn + 16)) != RUMI_OK ||
        (rc = s->chi.reserve(Hn + 1, Hn + Hn / 2 + 1)) != RUMI_OK || (rc = s->q.reserve(pairs, pairs + pairs / 2)) != RUMI_OK ||
        (rc = s->lists.reserve(listFirst, listFirst)) != RUMI_OK)
        return rc;
    RelocHyp *hIn = reinterpret_cast<RelocHyp *>(s->up.h);
    for (int h = 0; h < H; h++) {
        std::memset(&hIn[h], 0, sizeof(RelocHyp));
        hIn[h].cand = hyp[h].cand;
        std::memcpy(s->up.h + uT + (size_t)h * 28, hyp[h].Tcw7, 28);
        if (n > 0) std::memcpy(s->up.h + uInl + (size_t)h * n, hyp[h].inliers, n);
    }
    HIP_TRY(hipMemcpyAsync(s->up.d, s->up.h, upBytes, hipMemcpyHostToDevice, nullptr));
    const uint8_t *ds = s->sess.d;
    int32_t *dHead = reinterpret_cast<int32_t *>(s->res.d);
    RelocArgs A{};
    A.H = H; A.n = (int)n; A.words = s->words;
    A.hypIn = reinterpret_cast<const RelocHyp *>(s->up.d); A.hyp = reinterpret_cast<RelocHyp *>(s->res.d + rHyp);
    A.cands = reinterpret_cast<const RelocCand *>(ds); A.matches = reinterpret_cast<const int32_t *>(ds + s->oMatch);
    A.inl = s->up.d + uInl; A.Tin = reinterpret_cast<const float *>(s->up.d + uT);
    A.keys = s->fd.keys; A.pos = reinterpret_cast<const float *>(ds + s->oPos); A.invSigma2 = t->dInvSigma2;
    A.featMp = reinterpret_cast<int32_t *>(s->res.d + rMp); A.outLast = s->res.d + rOut; A.found = s->found.p;
    A.T = s->fl.p + fT; A.Xw = s->fl.p + fX; A.obs = s->fl.p + fO; A.w = s->fl.p + fW;
    A.idx = s->in.p + iIdx; A.start = s->in.p + iStart; A.outC = s->by.p; A.nGood = s->in.p + iGood;
    A.minGood = P.min_good; A.enough = P.enough; A.retryAbove = P.retry_above;
    RelocSearchArgs S{};
    S.H = H; S.nfeat = (int)n; S.words = s->words; S.maxNkf = std::max(s->maxNkf, 1);
    S.hyp = A.hyp; S.cands = A.cands; S.kfKeys = reinterpret_cast<const RumiKeyPoint *>(ds + s->oKeys); S.kfMp = reinterpret_cast<const int32_t *>(ds + s->oRows);
    S.pos = A.pos; S.minD = reinterpret_cast<const float *>(ds + s->oMin); S.maxD = reinterpret_cast<const float *>(ds + s->oMax);
    S.desc = ds + s->oDesc; S.bad = ds + s->oBad; S.found = s->found.p; S.T = A.T;
    std::memcpy(S.K, s->K4, 16);
    S.fd = s->fd; S.nLevels = t->nlevels; S.logSf = std::log(t->cfg.scale_factor);
    S.checkOri = P.check_orientation; S.enough = P.enough;
    S.q = s->q.p; S.pairCount = s->in.p + iCnt; S.pairBase = s->in.p + iBase; S.asg = s->in.p + iAsg; S.head = dHead; S.featMp = A.featMp;
    const float *dK4 = reinterpret_cast<const float *>(ds + s->oK4);
    const bool fitsLds = (int)n <= kPoseLdsEdges;
    const size_t ldsBytes = std::max<size_t>(n, 1) * sizeof(int32_t);
    (void)ldsBytes;                                          // (nfeat <= 16384: the resolve's LDS stays below the default limit)
    auto pose = [&](int stage) {
        return rumi::pose_opt_device(A.start, A.Xw, A.obs, A.w, dK4, A.T, A.T, s->by.p, s->in.p + iGood + (size_t)stage * H, s->by.p + Hn + 16, s->chi.p, fitsLds,
                                     nullptr, H);
    };
    auto search = [&](int stage) {
        S.stage = stage; S.th = stage == 0 ? P.th_coarse : P.th_fine; S.orbDist = stage == 0 ? P.dist_coarse : P.dist_fine;
        launch_reloc_search(S, nullptr);
    };
    const int32_t *hHead = reinterpret_cast<const int32_t *>(s->res.h);
    for (int attempt = 0;; attempt++) {
        S.lists = s->lists.p; S.listCap = (int)std::min<size_t>(s->lists.cap, 0x7FFFFFFF);
        HIP_TRY(hipMemsetAsync(dHead, 0, 16, nullptr));
        hipLaunchKernelGGL(k_reloc_seed, dim3(H), dim3(1024), 0, nullptr, A);
        if ((rc = pose(0)) != RUMI_OK) return rc;
        hipLaunchKernelGGL(k_reloc_after, dim3(H), dim3(1024), 0, nullptr, A, 0);
        search(0);
        hipLaunchKernelGGL(k_reloc_gather, dim3(H), dim3(1024), 0, nullptr, A, (int)RELOC_LIVE_P2);
        if ((rc = pose(1)) != RUMI_OK) return rc;
        hipLaunchKernelGGL(k_reloc_after, dim3(H), dim3(1024), 0, nullptr, A, 1);
        search(1);
        hipLaunchKernelGGL(k_reloc_gather, dim3(H), dim3(1024), 0, nullptr, A, (int)RELOC_LIVE_P3);
        if ((rc = pose(2)) != RUMI_OK) return rc;
        hipLaunchKernelGGL(k_reloc_after, dim3(H), dim3(1024), 0, nullptr, A, 2);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpy(s->res.h, s->res.d, resBytes, hipMemcpyDeviceToHost));          // the call's one synchronisation
        s->attempts = attempt + 1;
        const uint32_t need = std::max((uint32_t)hHead[0], (uint32_t)hHead[1]);
        if (need <= (uint32_t)S.listCap) break;
        // a stage's candidate lists outgrew the arena: its fill and resolve did nothing; the whole chain again from the seed with a larger one
        if (attempt >= 3 || need > 0x7FFFFFFFu) { g_lastError = std::string(entry) + ": the candidate lists outgrow their arena"; return RUMI_E_CAPACITY; }
        if ((rc = s->lists.reserve((size_t)need, (size_t)need + (size_t)need / 4)) != RUMI_OK) return rc;
    }
    const RelocHyp *hR = reinterpret_cast<const RelocHyp *>(s->res.h + rHyp);
    for (int h = 0; h < H; h++) {
        std::memcpy(&res[h], &hR[h], sizeof(RumiRelocResult));
        if (n > 0) {
            std::memcpy(frame_mp + (size_t)h * t->cap, s->res.h + rMp + (size_t)h * n * 4, n * 4);
            std::memcpy(outlier_last + (size_t)h * t->cap, s->res.h + rOut + (size_t)h * n, n);
        }
    }
    return RUMI_OK;
}

/* How many times the last rumi_track_reloc_refine ran its chain (1: every candidate list fitted the arena at once). */
extern "C" int rumi_track_reloc_attempts(const RumiTracker *t, int32_t *attempts) {
    if (!t || !attempts || !t->reloc) { g_lastError = "rumi_track_reloc_attempts: no relocalisation session on this tracker"; return RUMI_E_INVALID; }
    *attempts = t->reloc->attempts;
    return RUMI_OK;
}
