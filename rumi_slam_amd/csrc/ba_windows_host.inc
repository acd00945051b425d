// ba_windows_host.inc -- host side of the window-batched local bundle adjustment (kernels: ba_windows.inc).  Included by opt.hip.
//
// ONE host thread drives any number of windows: per window it stages the caller's arrays and g2o's structure (buildStructure: column blocks,
// edges by landmark, pose rows by key-frame) into the window's arena, then all windows share every launch.  A slot (one LM trial of every
// window that is still running) is four launches; the thread keeps one slot queued ahead of the one that runs and naps in between.

struct BawArgs {                         // one window as the C ABI hands it over
    int32_t nKF; float *kf_pose7; const uint8_t *kf_fixed; int32_t nMP; float *mp_pos3;
    int32_t nE; const int32_t *e_mp, *e_kf; const float *e_obs, *e_inv_sigma2; const float *K4;
    const volatile uint8_t *stop_flag; uint8_t *erase_out; int32_t *stats;
    bool resident = false;               // the raw block already lies in the arena's stage.d (ba_resident_host.inc): mp_pos3 and the e_* arrays are not read
};
// Where the raw arrays of a window lie in the arena's upload block: poses as doubles, positions, column blocks, then the edges as they came.
struct BawRawLayout { size_t oT, oX, oPC, oEM, oEK, oOb, oIn, upBytes; };
static BawRawLayout baw_raw_layout(int nKF, int nMP, int nE) {
    BawRawLayout r;
    r.oT = 0; r.oX = al16(r.oT + (size_t)nKF * 64); r.oPC = al16(r.oX + (size_t)nMP * 12); r.oEM = al16(r.oPC + (size_t)nKF * 4); r.oEK = al16(r.oEM + (size_t)nE * 4);
    r.oOb = al16(r.oEK + (size_t)nE * 4); r.oIn = al16(r.oOb + (size_t)nE * 8); r.upBytes = al16(r.oIn + (size_t)nE * 4);
    return r;
}
struct BawPrep {                         // what staging a window leaves behind
    int nOpt = 0, n = 0, NP = 0, NT = 0;
    size_t rT = 0, rX = 0, rE = 0, rErr = 0, dnBytes = 0, outOff = 0;
    int cur = 0, iters = 0, trials = 0, itersFirst = 0;
    bool ran = false;
};

// Whether a window runs on this path (ba_run and rumi_local_ba_batch both ask here): up to 29 optimised key-frames (the tile solver), at most 512
// key-frames (k_baw_system / k_baw_updchi cache every pose in LDS), and not on a profiled handle.  Everything else takes ba_run's host loop.
static bool baw_eligible(bool profiled, int32_t nKF, const uint8_t *kf_fixed, int32_t nMP, int32_t nE) {
    if (profiled || nKF < 1 || nKF > 512 || nE < 1 || nMP < 1 || !kf_fixed) return false;
    int nOpt = 0;
    for (int k = 0; k < nKF; k++) nOpt += kf_fixed[k] ? 0 : 1;
    const int n = 6 * nOpt, NT = (n + 1 + 15) / 16;
    return n > 0 && NT <= kSolveTilesMax;
}

// Stages window `a` into arena `c` on stream `st` and fills its descriptor (the structure is derived on the device: k_baws_*).
static int baw_stage(BaArena *c, hipStream_t st, int mode, const BawArgs &a, int gbaRobust, BAWin &Wd, BawPrep &P, int slicesWanted) {
    const int nKF = a.nKF, nMP = a.nMP, nE = a.nE;
    if (nKF > c->maxKF || nMP > c->maxMP || nE > c->maxE) { g_lastError = "local BA: problem larger than the optimiser's arenas"; return RUMI_E_CAPACITY; }
    { const int rc = c->extras(); if (rc != RUMI_OK) return rc; }
    int nOpt = 0;
    for (int k = 0; k < nKF; k++) nOpt += a.kf_fixed[k] ? 0 : 1;
    const int n = 6 * nOpt;
    // The raw block: the caller's arrays as they came (the structure -- g2o's buildStructure -- is derived on the device, k_baws_*), the initial
    // poses as doubles, the column blocks.  ONE pinned block up, or, for a resident window, what the fill kernels left there (ba_resident.inc).
    const BawRawLayout rl = baw_raw_layout(nKF, nMP, nE);
    const size_t oT = rl.oT, oX = rl.oX, oPC = rl.oPC, oEM = rl.oEM, oEK = rl.oEK, oOb = rl.oOb, oIn = rl.oIn, upBytes = rl.upBytes;
    if (upBytes > c->stage.cap) { g_lastError = "local BA: upload block larger than the optimiser's arenas"; return RUMI_E_CAPACITY; }
    if (!a.resident) {
        uint8_t *hs = c->stage.h;
        ba_stage_poses(nKF, a.kf_pose7, reinterpret_cast<double *>(hs + oT));
        {
            int32_t *poseCol = reinterpret_cast<int32_t *>(hs + oPC);
            int cc = 0;
            for (int k = 0; k < nKF; k++) poseCol[k] = a.kf_fixed[k] ? -1 : cc++;
        }
        std::memcpy(hs + oX, a.mp_pos3, (size_t)nMP * 12);
        std::memcpy(hs + oEM, a.e_mp, (size_t)nE * 4); std::memcpy(hs + oEK, a.e_kf, (size_t)nE * 4);
        std::memcpy(hs + oOb, a.e_obs, (size_t)nE * 8); std::memcpy(hs + oIn, a.e_inv_sigma2, (size_t)nE * 4);
        HIP_TRY(hipMemcpyAsync(c->stage.d, hs, upBytes, hipMemcpyHostToDevice, st));
    }
    const int NP = (n + 1 + 15) / 16 * 16, NT = NP / 16;
    Wd = BAWin{};
    Wd.nKF = nKF; Wd.nMP = nMP; Wd.nE = nE; Wd.nOpt = nOpt; Wd.n = n; Wd.NP = NP; Wd.NT = NT; Wd.nT = NT * (NT + 1) / 2;
    const int chunks = (nMP + kBawLm - 1) / kBawLm, S = std::max(1, std::min(std::min(slicesWanted, kBawMaxSlices), chunks));
    Wd.lmPerSlice = kBawLm * ((chunks + S - 1) / S);
    Wd.nSlices = (nMP + Wd.lmPerSlice - 1) / Wd.lmPerSlice;
    Wd.nUpd = (nMP * kLmLanes + 255) / 256;
    Wd.robust = mode == 2 ? (gbaRobust ? 1 : 0) : 1;
    Wd.useLast = 1;
    Wd.delta = ba_huber_delta(mode);
    Wd.dsqr = Wd.delta * Wd.delta;
    Wd.cam = DCam{a.K4[0], a.K4[1], a.K4[2], a.K4[3]};
    Wd.poseCol = (const int32_t *)(c->stage.d + oPC); Wd.rawMP = (const int32_t *)(c->stage.d + oEM); Wd.rawKF = (const int32_t *)(c->stage.d + oEK);
    Wd.rawObs = (const float *)(c->stage.d + oOb); Wd.rawInfo = (const float *)(c->stage.d + oIn); Wd.rawX = (const float *)(c->stage.d + oX);
    Wd.rawT = (const double *)(c->stage.d + oT);
    {
        auto alS = [](size_t x) { return (x + 255) & ~(size_t)255; };
        uint8_t *q = c->sorted.p;
        auto take = [&](size_t bytes) { uint8_t *r = q; q += alS(bytes); return r; };
        Wd.ptStart = (int32_t *)take((size_t)(nMP + 1) * 4); Wd.cursor = (int32_t *)take((size_t)(nMP + 1) * 4); Wd.kfRowStart = (int32_t *)take(64 * 4);
        Wd.sMP = (int32_t *)take((size_t)nE * 4); Wd.sKF = (int32_t *)take((size_t)nE * 4); Wd.sEdge = (int32_t *)take((size_t)nE * 4);
        Wd.rowSlot = (int32_t *)take((size_t)nE * 4); Wd.tmpEdge = (int32_t *)take((size_t)nE * 4); Wd.info = (float *)take((size_t)nE * 4);
        Wd.obs = (float *)take((size_t)nE * 8); Wd.rank8 = take((size_t)nE);
        Wd.nBlk = (nMP + 15) / 16;
        Wd.blkCnt = (int32_t *)take((size_t)Wd.nBlk * 32 * 4);
        if ((size_t)(q - c->sorted.p) > c->sorted.cap) { g_lastError = "local BA: structure arena too small"; return RUMI_E_CAPACITY; }
    }
    Wd.err = reinterpret_cast<int32_t *>(c->winSmall.p + 24);
    Wd.off = c->eOff.p;
    Wd.T[0] = c->T[0].p; Wd.T[1] = c->T[1].p; Wd.X[0] = c->X[0].p; Wd.X[1] = c->X[1].p;
    Wd.panel = c->panel.p; Wd.Dinv = c->Dinv.p; Wd.bl = c->bl.p; Wd.Hpp = c->Hpp.p; Wd.bp = c->bp.p; Wd.x = c->xv.p; Wd.lastChi2 = c->chi.p;
    Wd.Gpart = c->Gpart.p; Wd.G = c->Gw.p; Wd.chiPart = c->chiPart.p; Wd.sclPart = c->sclPart.p;
    Wd.solveOk = reinterpret_cast<double *>(c->winSmall.p); Wd.maxDiag = reinterpret_cast<unsigned long long *>(c->winSmall.p + 8);
    Wd.stopSeen = reinterpret_cast<int32_t *>(c->winSmall.p + 16);
    Wd.lm = c->lmCtl.p; Wd.mirror = c->wm.d; Wd.stopWord = c->stop.d;
    P.nOpt = nOpt; P.n = n; P.NP = NP; P.NT = NT;
    P.rT = 0; P.rX = al16(P.rT + (size_t)nKF * 64); P.rE = al16(P.rX + (size_t)nMP * 24); P.rErr = al16(P.rE + (size_t)nE); P.dnBytes = al16(P.rErr + 16);
    Wd.outT = reinterpret_cast<double *>(c->stageOut.p + P.rT); Wd.outX = reinterpret_cast<double *>(c->stageOut.p + P.rX); Wd.erase = c->stageOut.p + P.rE;
    Wd.errOut = reinterpret_cast<int32_t *>(c->stageOut.p + P.rErr);
    return RUMI_OK;
}

// A GROUP of windows that share every launch: its own stream, window table and mirror words.  One host thread drives any number of groups as
// small state machines (stage -> structure -> [pass: slots until every window reports done] -> (merge BA: mark, second pass) -> finalize ->
// copy back): a batch is cut into two groups, so that the transfers, the one-workgroup-per-window solve and the launch tails of one group run
// beside the wide kernels of the other.
struct BawGroup {
    BaRunner *run = nullptr;               // stream, events, window table, result block
    int mode = 0, nW = 0, gbaIterations = 0, gbaRobust = 1;
    const BawArgs *args = nullptr;
    BaArena *arenas = nullptr;             // window i of the group runs in arenas[i]
    int32_t *status = nullptr;
    std::vector<BawPrep> prep;
    std::vector<int> live;
    int L = 0, worst = RUMI_OK;
    int maxS = 1, maxT = 1, maxOpt = 1, maxUpd = 1, maxNT = 1, maxKFs = 1, maxF = 1;
    size_t ldsSys = 0, ldsTiles = 0, ldsUpd = 0;
    typedef void (*SysKernel)(const BAWin *, int, unsigned);
    SysKernel sysK = nullptr;
    // pass state
    enum Phase { kIdle, kPass, kFinalWait, kDone } phase = kIdle;
    int passNo = 0, passMaxIt = 0, maxSlots = 0, enq = 0, naps = 0;
    unsigned runId = 0;
    bool anyRun = false;
    double tStage = 0, tLm0 = 0, tLm1 = 0;

    hipStream_t st() const { return run->stream; }
    BAWin *tab() const { return run->winTab.h; }

    int begin() {                          // stage every window, derive the structure on the device, start the first pass
        if (nW > kBawMaxWindows) { g_lastError = "local BA batch: too many windows in one launch group"; return RUMI_E_CAPACITY; }
        const double tA = ba_now_us();
        prep.assign((size_t)nW, BawPrep{});
        static const int envSlices = std::getenv("RUMI_BAW_SLICES") ? std::atoi(std::getenv("RUMI_BAW_SLICES")) : 0;
        const int slicesWanted = envSlices > 0 ? envSlices : std::max(8, std::min(kBawMaxSlices, 512 / std::max(nW, 1)));
        for (int i = 0; i < nW; i++) {
            const BawArgs &a = args[i];
            status[i] = RUMI_OK;
            int rcExit;
            if (ba_early_exit(mode, a.nKF, a.kf_fixed, a.stop_flag, a.stats, &rcExit)) { if (rcExit != RUMI_OK) status[i] = worst = rcExit; continue; }
            const int rc = baw_stage(&arenas[i], st(), mode, a, gbaRobust, tab()[live.size()], prep[i], slicesWanted);
            if (rc != RUMI_OK) { status[i] = worst = rc; continue; }
            live.push_back(i);
        }
        L = (int)live.size();
        tStage = ba_now_us() - tA;
        if (L == 0) { phase = kDone; return RUMI_OK; }
        HIP_TRY(hipEventRecord(run->ev[0], st()));
        int maxE = 1, maxMP = 1, maxBlk = 1;
        for (int j = 0; j < L; j++) {                       // launch geometry: the maxima over the live windows
            const BAWin &Wd = tab()[j];
            maxS = std::max(maxS, Wd.nSlices); maxT = std::max(maxT, Wd.nT); maxOpt = std::max(maxOpt, Wd.nOpt); maxUpd = std::max(maxUpd, Wd.nUpd);
            maxNT = std::max(maxNT, Wd.NT); maxKFs = std::max(maxKFs, Wd.nKF);
            maxF = std::max(maxF, std::max((Wd.nE + 255) / 256, std::max((Wd.nKF * 8 + 255) / 256, (Wd.nMP * 3 + 255) / 256)));
            maxE = std::max(maxE, Wd.nE); maxMP = std::max(maxMP, Wd.nMP); maxBlk = std::max(maxBlk, Wd.nBlk);
        }
        ldsSys = ((size_t)maxNT * kBawTileStride + 9 * 256 + kBawLm * 15 + 2 * kBawRows + (size_t)maxKFs * 8) * sizeof(double) + (size_t)maxKFs * 4 + 16;
        ldsTiles = ((size_t)(maxNT * (maxNT + 1) / 2) * 256 + (size_t)maxNT * 16) * sizeof(double);
        ldsUpd = ((size_t)maxKFs * 16 + (size_t)maxNT * 16) * sizeof(double) + (size_t)maxKFs * 4 + 16;
        const int slotsNeeded = (maxT + 3) / 4;
        sysK = slotsNeeded <= 2 ? k_baw_system<2> : slotsNeeded <= 4 ? k_baw_system<4> : slotsNeeded <= 6 ? k_baw_system<6> :
               slotsNeeded <= 9 ? k_baw_system<9> : slotsNeeded <= 12 ? k_baw_system<12> : k_baw_system<17>;
        if (ldsSys > 48 * 1024) HIP_TRY(raise_lds_limit(reinterpret_cast<const void *>(sysK), ldsSys));
        if (ldsTiles > 48 * 1024) HIP_TRY(raise_lds_limit(reinterpret_cast<const void *>(k_baw_solve), ldsTiles));
        // the structure of every window: seven small launches for the whole group
        const BAWin *dTab = run->winTab.d;
        HIP_TRY(hipMemcpyAsync(run->winTab.d, tab(), sizeof(BAWin) * L, hipMemcpyHostToDevice, st()));
        const int gE2 = (maxE + 255) / 256;
        hipLaunchKernelGGL(k_baws_zero, dim3((std::max(maxE, maxMP + 1) + 255) / 256, L), dim3(256), 0, st(), dTab);
        hipLaunchKernelGGL(k_baws_count, dim3(gE2, L), dim3(256), 0, st(), dTab);
        hipLaunchKernelGGL(k_baws_scan, dim3(L), dim3(1024), 0, st(), dTab);
        hipLaunchKernelGGL(k_baws_scatter, dim3(gE2, L), dim3(256), 0, st(), dTab);
        hipLaunchKernelGGL(k_baws_order, dim3(maxBlk, L), dim3(256), 0, st(), dTab);
        hipLaunchKernelGGL(k_baws_kfscan, dim3(L), dim3(1024), 0, st(), dTab);
        hipLaunchKernelGGL(k_baws_rowslot, dim3(maxBlk, L), dim3(256), 0, st(), dTab);
        HIP_TRY(hipGetLastError());
        tLm0 = ba_now_us();
        const int firstIt = mode == 0 ? 10 : mode == 1 ? 5 : gbaIterations;     // (mode 2 with the stop flag already up or no iteration goes the single-window path, ba_run)
        return start_pass(firstIt);
    }
    int start_pass(int maxIt) {            // a pass starts from the table alone: the head of slot 0 makes the control block
        passMaxIt = maxIt;
        for (int j = 0; j < L; j++) {
            tab()[j].maxIt = maxIt;
            tab()[j].cur0 = prep[live[j]].cur;
            *arenas[live[j]].stop.h = 0;
        }
        HIP_TRY(hipMemcpyAsync(run->winTab.d, tab(), sizeof(BAWin) * L, hipMemcpyHostToDevice, st()));
        runId = ++run->bawRun;
        maxSlots = maxIt * 10 + 2;                          // init, the trials, and the head that takes the last decision
        enq = 0; naps = 0;
        phase = kPass;
        return RUMI_OK;
    }
    void report(const BaArena *c, int *slotSeen, bool *done) const {
        const unsigned long long w = __atomic_load_n(const_cast<const unsigned long long *>(&c->wm.h->word), __ATOMIC_ACQUIRE);
        if ((unsigned)(w >> 32) != runId) { *slotSeen = -1; *done = false; return; }
        *slotSeen = (int)((w & 0xFFFFFFFFull) >> 1) - 1; *done = (w & 1) != 0;
    }
    void enqueue_slot(int slot) {
        const BAWin *dTab = run->winTab.d;
        hipLaunchKernelGGL(sysK, dim3(maxS, L), dim3(256), ldsSys, st(), dTab, slot, runId);
        if (maxS > 64) hipLaunchKernelGGL((k_baw_reduce<16>), dim3(4 * maxT + maxOpt, L), dim3(1024), 0, st(), dTab, slot, 4 * maxT);
        else hipLaunchKernelGGL((k_baw_reduce<4>), dim3(4 * maxT + maxOpt, L), dim3(256), 0, st(), dTab, slot, 4 * maxT);
        if (slot > 0) {
            hipLaunchKernelGGL(k_baw_solve, dim3(L), dim3(kSolveThreads), ldsTiles, st(), dTab, slot);
            hipLaunchKernelGGL(k_baw_updchi, dim3(maxUpd, L), dim3(256), ldsUpd, st(), dTab, slot);
        }
    }
    // one step of the machine; *worked = something was enqueued or a phase ended (the caller naps only when no group worked)
    int pump(bool *worked) {
        *worked = false;
        if (phase == kPass) {
            int seen = 1 << 30;
            bool allDone = true;
            for (int j = 0; j < L; j++) {
                BaArena *c = &arenas[live[j]];
                int sl; bool dn;
                report(c, &sl, &dn);
                if (!dn) { allDone = false; seen = std::min(seen, sl); }
                const volatile uint8_t *sf = args[live[j]].stop_flag;
                if (sf && *sf) *c->stop.h = 1;
            }
            if (!allDone) {
                if (enq < maxSlots && (enq <= 1 || enq <= seen + 1)) {
                    enqueue_slot(enq);
                    HIP_TRY(hipGetLastError());
                    enq++; naps = 0; *worked = true;
                } else if ((++naps & 0x3FF) == 0 && hipStreamQuery(st()) != hipErrorNotReady) {
                    HIP_TRY(hipStreamSynchronize(st()));
                    bool ok = true;
                    for (int j = 0; j < L; j++) { int sl; bool dn; report(&arenas[live[j]], &sl, &dn); ok &= dn; }
                    if (!ok && enq >= maxSlots) { g_lastError = "local BA: the device-side LM loop stalled"; return RUMI_E_NO_DEVICE; }
                }
                return RUMI_OK;
            }
            __atomic_thread_fence(__ATOMIC_ACQUIRE);
            for (int j = 0; j < L; j++) {
                BaArena *c = &arenas[live[j]];
                BawPrep &P = prep[live[j]];
                P.cur = c->wm.h->cur; P.iters += c->wm.h->iters; P.trials += c->wm.h->trials; P.ran = true;
            }
            anyRun = true;
            *worked = true;
            if (passNo == 0) for (int j = 0; j < L; j++) prep[live[j]].itersFirst = prep[live[j]].iters;
            if (mode == 1 && passNo == 0) {                 // bDoMore (Optimizer.cc:3986-4031)
                bool stopped = false;
                for (int j = 0; j < L; j++) { const volatile uint8_t *sf = args[live[j]].stop_flag; stopped |= sf && *sf; }
                if (!stopped) {
                    int gM = 1;
                    for (int j = 0; j < L; j++) gM = std::max(gM, (tab()[j].nE + 255) / 256);
                    hipLaunchKernelGGL(k_baw_mark, dim3(gM, L), dim3(256), 0, st(), run->winTab.d);     // (reads the table of the first pass: same arrays)
                    for (int j = 0; j < L; j++) tab()[j].robust = 0;
                    passNo = 1;
                    return start_pass(10);
                }
            }
            return finish_enqueue();
        }
        if (phase == kFinalWait) {
            if (hipStreamQuery(st()) == hipErrorNotReady) return RUMI_OK;
            *worked = true;
            return finish();
        }
        return RUMI_OK;
    }
    int finish_enqueue() {                 // results: [T | X | erase | err] per window, gathered by one launch, one copy each
        tLm1 = ba_now_us();
        // every window's block [T | X | erase | err] into ONE buffer of the group: one copy back instead of one per window
        size_t total = 0;
        for (int j = 0; j < L; j++) { prep[live[j]].outOff = total; total += (prep[live[j]].dnBytes + 255) & ~(size_t)255; }
        if (total > run->groupOut.cap) { g_lastError = "local BA: result block larger than the runner's"; return RUMI_E_CAPACITY; }   // (cannot happen: every window passed baw_stage's limits)
        for (int j = 0; j < L; j++) {
            const BawPrep &P = prep[live[j]];
            BAWin &Wd = tab()[j];
            Wd.useLast = P.ran ? 1 : 0; Wd.cur0 = P.cur;
            uint8_t *base = run->groupOut.d + P.outOff;
            Wd.outT = reinterpret_cast<double *>(base + P.rT); Wd.outX = reinterpret_cast<double *>(base + P.rX); Wd.erase = base + P.rE;
            Wd.errOut = reinterpret_cast<int32_t *>(base + P.rErr);
        }
        HIP_TRY(hipMemcpyAsync(run->winTab.d, tab(), sizeof(BAWin) * L, hipMemcpyHostToDevice, st()));
        hipLaunchKernelGGL(k_baw_finalize, dim3(maxF, L), dim3(256), 0, st(), run->winTab.d);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipEventRecord(run->ev[1], st()));
        HIP_TRY(hipMemcpyAsync(run->groupOut.h, run->groupOut.d, total, hipMemcpyDeviceToHost, st()));
        phase = kFinalWait;
        return RUMI_OK;
    }
    int finish() {
        HIP_TRY(hipStreamSynchronize(st()));
        HIP_TRY(hipEventElapsedTime(&run->stageMs[5], run->ev[0], run->ev[1]));
        const double tD = ba_now_us();
        for (int j = 0; j < L; j++) {
            const int i = live[j];
            const BawArgs &a = args[i];
            const BawPrep &P = prep[i];
            const uint8_t *hb = run->groupOut.h + P.outOff;
            const int32_t err = *reinterpret_cast<const int32_t *>(hb + P.rErr);
            if (err) {                                      // nothing of this window is written back
                g_lastError = (err & 1) ? "local BA: edge index out of range" : "local BA: a map point is observed twice by one key-frame";
                status[i] = worst = RUMI_E_INVALID;
                continue;
            }
            ba_unpack(a.nKF, a.kf_fixed, a.nMP, a.nE, reinterpret_cast<const double *>(hb + P.rT), reinterpret_cast<const double *>(hb + P.rX), hb + P.rE,
                      a.kf_pose7, a.mp_pos3, a.erase_out);
            ba_write_stats(mode, P.iters, P.itersFirst, P.trials, P.nOpt, a.stats);
        }
        static const bool hostDbg = std::getenv("RUMI_HOSTDBG") != nullptr;
        if (hostDbg) fprintf(stderr, "baw host us (%d windows): staging %.1f lm %.1f finalize+copy %.1f unpack %.1f\n", L, tStage, tLm1 - tLm0, tD - tLm1, ba_now_us() - tD);
        phase = kDone;
        return RUMI_OK;
    }
};

// Launch groups of a batch of nW windows when nRunners runners can be had.  Every group is a chain of dependent launches (system -> reduce -> solve
// -> update per trial) that leaves most of the device idle; chains of different groups fill each other's gaps.  16 windows of BASELINE configs[3]:
// 0.147 ms per window as one group, 0.127-0.135 as two, 0.120-0.124 as three, 0.144-0.152 as four (the one host thread then is the limit); 12 windows
// 0.155 / 0.135-0.145 / 0.129-0.132; 8 windows 0.174 / 0.166 / 0.166
static int baw_groups(int nW, int nRunners) {
    static const int envGroups = std::getenv("RUMI_BAW_GROUPS") ? std::atoi(std::getenv("RUMI_BAW_GROUPS")) : 0;
    const int G = envGroups > 0 ? envGroups : (nW >= 12 ? 3 : nW >= 8 ? 2 : 1);
    return std::max(1, std::min(std::min(G, nRunners), nW));
}

// nW windows (each already known to be eligible) from ONE thread; window i runs in arenas[i]; runners[g] drives group g (baw_groups(nW, nRunners) of them).
static int baw_run(int mode, int nW, const BawArgs *args, BaArena *arenas, int gbaIterations, int gbaRobust, int32_t *status,
                   BaRunner *const *runners, int nRunners) {
    HIP_TRY(hipSetDevice(runners[0]->device));
    const int G = baw_groups(nW, nRunners);
    std::vector<BawGroup> grp((size_t)G);
    for (int g = 0, i0 = 0; g < G; g++) {
        const int cnt = (nW - i0 + (G - g) - 1) / (G - g);
        BawGroup &B = grp[g];
        B.run = runners[g]; B.mode = mode; B.nW = cnt; B.args = args + i0; B.arenas = arenas + i0; B.status = status + i0;
        B.gbaIterations = gbaIterations; B.gbaRobust = gbaRobust;
        i0 += cnt;
    }
    struct SlackGuard {                     // naps of 25 us are not rounded up to the default 50 us timer slack meanwhile (the caller's thread: put back)
        long old;
        SlackGuard() : old(prctl(PR_GET_TIMERSLACK, 0UL, 0UL, 0UL, 0UL)) { (void)prctl(PR_SET_TIMERSLACK, 1000UL, 0UL, 0UL, 0UL); }
        ~SlackGuard() { if (old > 0) (void)prctl(PR_SET_TIMERSLACK, (unsigned long)old, 0UL, 0UL, 0UL); }
    } slackGuard;
    int rcAll = RUMI_OK;
    for (int g = 0; g < G; g++) {           // group g's transfers and structure kernels run beside group g - 1's first slots
        const int rc = grp[g].begin();
        if (rc != RUMI_OK) { rcAll = rc; grp[g].phase = BawGroup::kDone; }
        bool w;
        // its first two slots go out at once (they wait for no report): the device then has the group's first trial to run while the host stages
        // the next group (0.2 ms for 8 windows of BASELINE configs[3], during which this group's queue stood empty)
        for (int k = 0; k < 2 && grp[g].phase == BawGroup::kPass; k++) { const int rc2 = grp[g].pump(&w); if (rc2 != RUMI_OK) { rcAll = rc2; grp[g].phase = BawGroup::kDone; } }
        for (int q = 0; q < g; q++) if (grp[q].phase != BawGroup::kDone) { const int rc2 = grp[q].pump(&w); if (rc2 != RUMI_OK) { rcAll = rc2; grp[q].phase = BawGroup::kDone; } }
    }
    for (;;) {
        bool any = false, worked = false;
        for (int g = 0; g < G; g++) {
            if (grp[g].phase == BawGroup::kDone) continue;
            any = true;
            bool w = false;
            const int rc = grp[g].pump(&w);
            if (rc != RUMI_OK) { rcAll = rc; grp[g].phase = BawGroup::kDone; (void)hipStreamSynchronize(grp[g].st()); }
            worked |= w;
        }
        if (!any) break;
        if (!worked) std::this_thread::sleep_for(std::chrono::microseconds(25));
    }
    if (rcAll != RUMI_OK) return rcAll;
    int worst = RUMI_OK;
    for (int g = 0; g < G; g++) if (grp[g].worst != RUMI_OK) worst = grp[g].worst;
    return worst;
}
