// ba_resident_host.inc -- host side of rumi_local_ba_resident (kernels: ba_resident.inc).  Included by opt.hip after ba_single_host.inc.
//
// The store's mirror decides lLocalKeyFrames; the kernels build the lists, the counts and the raw block of the window in the handle's own
// arena; ONE small block (head and key-frame list) comes back between assembly and solve, because the launch geometry of the solver needs
// the sizes on the host.  The assembly runs on the null stream, where covis_view enqueues the store's staged edits; the runner's stream is
// non-blocking, so an event orders the two.

extern "C" int rumi_local_ba_resident(RumiOptimizer *o, RumiCovis *c, int32_t cur_slot, const int32_t *neigh_slots, int32_t n_neigh, int32_t init_slot,
                                      const volatile uint8_t *stop_flag, RumiLbaResidentOut *out) {
    const char *const E = "rumi_local_ba_resident";
    if (!o || !c || !out || n_neigh < 0 || (n_neigh > 0 && !neigh_slots) || out->kf_cap < 0 || out->mp_cap < 0 || out->erase_cap < 0 ||
        (out->kf_cap > 0 && (!out->kf_slots || !out->kf_pose7)) || (out->mp_cap > 0 && (!out->mp_ids || !out->mp_pos3)) || (out->erase_cap > 0 && !out->erased)) {
        g_lastError = std::string(E) + ": missing argument, negative count, or a capacity without its array";
        return RUMI_E_INVALID;
    }
    LbaResident &R = o->lba;
    BaArena &a = o->ba.arena;
    // ---- lLocalKeyFrames from the mirror (Optimizer.cc:1007-1017)
    R.locals.resize((size_t)n_neigh + 1); R.role.resize(RUMI_COVIS_MAX_KEYFRAMES);
    CovisLbaWindow W;
    int rc = covis_lba_window(c, cur_slot, neigh_slots, n_neigh, init_slot, E, R.locals.data(), R.role.data(), &W);
    if (rc != RUMI_OK || (rc = covis_same_device(c, o->device, E)) != RUMI_OK) return rc;
    HIP_TRY(hipSetDevice(o->device));
    CovisView cv;
    if ((rc = covis_view(c, 0, &cv)) != RUMI_OK || (rc = R.ev.create()) != RUMI_OK) return rc;
    const int nLocal = W.nLocal, hiSlot = W.hiSlot, gy = std::max(1, (W.maxRow + 255) / 256);
    const int ptCap = (int)std::max<int64_t>(1, std::min<int64_t>(W.sumRows, a.maxMP));
    auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
    // ---- the call's blocks: [head | key-frame list] come back together; the rest stays on the device
    const size_t wHead = 0, wKfList = wHead + LBA_HEAD_WORDS * 4, wBack = wKfList + (size_t)(nLocal + hiSlot) * 4, wBlk = al(wBack), wPts = al(wBlk + (size_t)nLocal * gy * 4),
                 wCnt = al(wPts + (size_t)ptCap * 4), wStart = al(wCnt + (size_t)ptCap * 4), wTag = al(wStart + (size_t)(ptCap + 1) * 4), wIdx = al(wTag + (size_t)hiSlot * 8),
                 wBytes = al(wIdx + (size_t)hiSlot * 4);
    const size_t iRole = al16((size_t)nLocal * 4), inBytes = iRole + al16((size_t)hiSlot * 4);
    const size_t edgeBytes = 2 * al((size_t)a.maxE * 4) + (size_t)a.maxE * 12;          // observer word, point id, erase list
    if ((rc = R.work.reserve(wBytes, wBytes + wBytes / 4)) != RUMI_OK || (rc = R.in.reserve(inBytes, inBytes + inBytes / 4)) != RUMI_OK ||
        (rc = R.edge.reserve(edgeBytes, edgeBytes)) != RUMI_OK)
        return rc;
    if (R.ptTag.cap < (size_t)cv.maxPoints) {
        if ((rc = R.ptTag.reserve((size_t)cv.maxPoints, (size_t)cv.maxPoints)) != RUMI_OK) return rc;
        HIP_TRY(hipMemsetAsync(R.ptTag.p, 0, (size_t)cv.maxPoints * 8, nullptr));
    }
    if (++R.epoch == 0) { HIP_TRY(hipMemsetAsync(R.ptTag.p, 0, R.ptTag.cap * 8, nullptr)); R.epoch = 1; }   // once every 2^32 calls: stale stamps could meet a reused epoch
    std::memcpy(R.in.h, R.locals.data(), (size_t)nLocal * 4);
    std::memcpy(R.in.h + iRole, R.role.data(), (size_t)hiSlot * 4);
    HIP_TRY(hipMemcpyAsync(R.in.d, R.in.h, inBytes, hipMemcpyHostToDevice, nullptr));
    HIP_TRY(hipMemsetAsync(R.work.p + wHead, 0, LBA_HEAD_WORDS * 4, nullptr));
    HIP_TRY(hipMemsetAsync(R.work.p + wTag, 0xFF, (size_t)hiSlot * 8, nullptr));
    LbaArgs A{};
    A.v = cv;
    A.locals = reinterpret_cast<const int32_t *>(R.in.d); A.role = reinterpret_cast<const int32_t *>(R.in.d + iRole);
    A.nLocal = nLocal; A.hiSlot = hiSlot; A.curMap = W.curMap; A.initIdx = W.initIdx; A.ptCap = ptCap; A.epoch = R.epoch;
    A.ptTag = R.ptTag.p;
    A.head = reinterpret_cast<int32_t *>(R.work.p + wHead); A.kfList = reinterpret_cast<int32_t *>(R.work.p + wKfList);
    A.blkCnt = reinterpret_cast<int32_t *>(R.work.p + wBlk); A.ptList = reinterpret_cast<int32_t *>(R.work.p + wPts);
    A.edgeCnt = reinterpret_cast<int32_t *>(R.work.p + wCnt); A.ptStart = reinterpret_cast<int32_t *>(R.work.p + wStart);
    A.fixTag = reinterpret_cast<unsigned long long *>(R.work.p + wTag); A.kfIndex = reinterpret_cast<int32_t *>(R.work.p + wIdx);
    hipLaunchKernelGGL(k_lba_points<1>, dim3(nLocal, gy), dim3(256), 0, nullptr, A);
    hipLaunchKernelGGL(k_lba_points<2>, dim3(nLocal, gy), dim3(256), 0, nullptr, A);
    hipLaunchKernelGGL(k_lba_points<3>, dim3(nLocal, gy), dim3(256), 0, nullptr, A);
    hipLaunchKernelGGL(k_lba_observers, dim3((ptCap + 3) / 4), dim3(256), 0, nullptr, A);
    hipLaunchKernelGGL(k_lba_scan, dim3(1), dim3(1024), 0, nullptr, A);
    HIP_TRY(hipGetLastError());
    // ---- the one read-back between assembly and solve
    const size_t oErased = al16(wBack), oIds = oErased + al16((size_t)a.maxE * 12), outBytes = oIds + (size_t)ptCap * 4;
    if ((rc = R.out.reserve(outBytes, outBytes + outBytes / 4)) != RUMI_OK) return rc;
    HIP_TRY(hipMemcpy(R.out.h, R.work.p, wBack, hipMemcpyDeviceToHost));
    const int32_t *head = reinterpret_cast<const int32_t *>(R.out.h), *kfList = reinterpret_cast<const int32_t *>(R.out.h + wKfList);
    if (head[LBA_V_NO_MAP] || head[LBA_V_OBS_MISMATCH] || head[LBA_V_KF_NO_POSE] || head[LBA_V_KF_NO_FEATURES] || head[LBA_V_NO_ATTR] || head[LBA_V_NO_OBS_FEATURES]) {
        g_lastError = std::string(E) + ": the store is inconsistent among what the call reads: " + std::to_string(head[LBA_V_NO_MAP]) +
                      " points of local rows were never given a map (rumi_covis_set_point_maps), " + std::to_string(head[LBA_V_OBS_MISMATCH]) +
                      " observations disagree with their slot's map-point row, " + std::to_string(head[LBA_V_KF_NO_POSE]) +
                      " key-frames or observations of the window have no pose (rumi_covis_set_keyframe_poses), " + std::to_string(head[LBA_V_KF_NO_FEATURES]) +
                      " have no resident features, " + std::to_string(head[LBA_V_NO_ATTR]) + " listed points have no attributes, " +
                      std::to_string(head[LBA_V_NO_OBS_FEATURES]) + " have observers but no observation features";
        return RUMI_E_INVALID;
    }
    const int nMP = head[LBA_H_NMP], nFixed = head[LBA_H_NFIXED], nE = head[LBA_H_NE], nKF = nLocal + nFixed;
    const int numFixed = nFixed + (W.initIdx >= 0 ? 1 : 0);
    if (numFixed == 0) { g_lastError = "LM-LBA: There are 0 fixed KF in the optimizations, LBA aborted"; return RUMI_E_INVALID; }   // Optimizer.cc:1057-1060
    if (stop_flag && *stop_flag) { out->stats[0] = out->stats[1] = out->stats[2] = 0; out->stats[3] = 1; return RUMI_OK; }          // :1274-1276
    if (nMP > ptCap || nKF > a.maxKF || nE > a.maxE) { g_lastError = "local BA: problem larger than the optimiser's arenas"; return RUMI_E_CAPACITY; }
    if (nKF > out->kf_cap || nMP > out->mp_cap) { g_lastError = std::string(E) + ": kf_cap or mp_cap is too small for the lists"; return RUMI_E_CAPACITY; }
    const BawRawLayout rl = baw_raw_layout(nKF, nMP, nE);
    if (rl.upBytes > a.stage.cap) { g_lastError = "local BA: upload block larger than the optimiser's arenas"; return RUMI_E_CAPACITY; }

    // ---- the raw block of the window, where baw_stage expects it
    LbaRaw raw;
    raw.rawT = reinterpret_cast<double *>(a.stage.d + rl.oT); raw.rawX = reinterpret_cast<float *>(a.stage.d + rl.oX);
    raw.poseCol = reinterpret_cast<int32_t *>(a.stage.d + rl.oPC); raw.rawMP = reinterpret_cast<int32_t *>(a.stage.d + rl.oEM);
    raw.rawKF = reinterpret_cast<int32_t *>(a.stage.d + rl.oEK); raw.rawObs = reinterpret_cast<float *>(a.stage.d + rl.oOb);
    raw.rawInfo = reinterpret_cast<float *>(a.stage.d + rl.oIn);
    raw.edgeObs = reinterpret_cast<int32_t *>(R.edge.p); raw.edgePt = reinterpret_cast<int32_t *>(R.edge.p + al((size_t)a.maxE * 4));
    int32_t *dErased = reinterpret_cast<int32_t *>(R.edge.p + 2 * al((size_t)a.maxE * 4));
    hipLaunchKernelGGL(k_lba_fill_kf, dim3((nKF + 255) / 256), dim3(256), 0, nullptr, A, raw, nKF);
    if (nMP > 0) hipLaunchKernelGGL(k_lba_fill_edges, dim3((nMP + 3) / 4), dim3(256), 0, nullptr, A, raw, nMP);
    HIP_TRY(hipGetLastError());
    int32_t *hIds = reinterpret_cast<int32_t *>(R.out.h + oIds);
    if (nMP > 0) HIP_TRY(hipMemcpyAsync(hIds, A.ptList, (size_t)nMP * 4, hipMemcpyDeviceToHost, nullptr));     // the ids come back under the solve

    std::vector<uint8_t> fixed((size_t)nKF, 1), erase((size_t)std::max(nE, 1), 0);
    for (int k = 0; k < nLocal; k++) fixed[k] = k == W.initIdx;
    std::vector<float> pose7((size_t)nKF * 7, 0.f), pos((size_t)std::max(nMP, 1) * 3, 0.f);
    for (int k = 0; k < nKF; k++) covis_lba_pose7(c, kfList[k], pose7.data() + (size_t)k * 7);
    int32_t stats[4] = {0, 0, 0, 0};
    const uint8_t *dResult = nullptr;                  // [T | X | erase] as the run left it on the device
    if (baw_eligible(o->prof.on, nKF, fixed.data(), nMP, nE)) {
        HIP_TRY(hipEventRecord(R.ev, nullptr));
        HIP_TRY(hipStreamWaitEvent(o->ba.run.stream, R.ev, 0));
        BawArgs w{nKF, pose7.data(), fixed.data(), nMP, pos.data(), nE, nullptr, nullptr, nullptr, nullptr, W.K4, stop_flag, erase.data(), stats};
        w.resident = true;
        BaRunner *runner = &o->ba.run;
        int32_t status = RUMI_OK;
        rc = baw_run(0, 1, &w, &a, 0, 1, &status, &runner, 1);
        if (rc == RUMI_OK) rc = status;
        dResult = o->ba.run.groupOut.d;
    } else {
        // any other window: read back once and handed to the single-window host loop as rumi_local_ba hands it over
        HIP_TRY(hipMemcpy(a.stage.h, a.stage.d, rl.upBytes, hipMemcpyDeviceToHost));
        std::vector<int32_t> eMP((size_t)std::max(nE, 1)), eKF((size_t)std::max(nE, 1));
        std::vector<float> eObs((size_t)std::max(nE, 1) * 2), eInfo((size_t)std::max(nE, 1));
        if (nMP > 0) std::memcpy(pos.data(), a.stage.h + rl.oX, (size_t)nMP * 12);
        if (nE > 0) {
            std::memcpy(eMP.data(), a.stage.h + rl.oEM, (size_t)nE * 4); std::memcpy(eKF.data(), a.stage.h + rl.oEK, (size_t)nE * 4);
            std::memcpy(eObs.data(), a.stage.h + rl.oOb, (size_t)nE * 8); std::memcpy(eInfo.data(), a.stage.h + rl.oIn, (size_t)nE * 4);
        }
        rc = ba_run(&o->ba, &o->prof, 0, nKF, pose7.data(), fixed.data(), nMP, pos.data(), nE, eMP.data(), eKF.data(), eObs.data(), eInfo.data(), W.K4, stop_flag,
                    erase.data(), stats);
        dResult = a.stageOut.p;
    }
    {   // the copy of the ids may still be in flight: no return below leaves it writing into a block the next call may replace
        const hipError_t es = hipStreamSynchronize(nullptr);
        if (rc == RUMI_OK) HIP_TRY(es);
    }
    if (rc != RUMI_OK) return rc;
    if (stats[3]) { std::memcpy(out->stats, stats, sizeof stats); return RUMI_OK; }     // the flag went up between the two looks: nothing ran
    int nErased = 0;
    for (int e = 0; e < nE; e++) nErased += erase[e] != 0;
    if (nErased > out->erase_cap) { g_lastError = std::string(E) + ": erase_cap is too small for the erased observations"; return RUMI_E_CAPACITY; }

    // ---- write-back (the run's stream has been waited for): positions into the attribute records, the erase list compacted in edge order
    const size_t rX = al16((size_t)nKF * 64), rE = al16(rX + (size_t)nMP * 24);
    hipLaunchKernelGGL(k_lba_commit, dim3(1), dim3(1024), 0, nullptr, A, raw, reinterpret_cast<const double *>(dResult + rX), dResult + rE, nMP, nE, dErased, a.maxE);
    HIP_TRY(hipGetLastError());
    int32_t *hErased = reinterpret_cast<int32_t *>(R.out.h + oErased);
    if (nErased > 0) HIP_TRY(hipMemcpyAsync(hErased, dErased, (size_t)nErased * 12, hipMemcpyDeviceToHost, nullptr));
    HIP_TRY(hipStreamSynchronize(nullptr));
    covis_lba_write_positions(c, nMP, hIds, pos.data());
    if ((rc = rumi_covis_set_keyframe_poses(c, nLocal, kfList, pose7.data())) != RUMI_OK) return rc;

    std::memcpy(out->kf_slots, kfList, (size_t)nKF * 4);
    std::memcpy(out->kf_pose7, pose7.data(), (size_t)nLocal * 28);
    if (nMP > 0) { std::memcpy(out->mp_ids, hIds, (size_t)nMP * 4); std::memcpy(out->mp_pos3, pos.data(), (size_t)nMP * 12); }
    if (nErased > 0) std::memcpy(out->erased, hErased, (size_t)nErased * 12);
    out->n_kf = nKF; out->num_OptKF = nLocal; out->num_fixedKF = numFixed; out->num_MPs = nMP; out->num_edges = nE; out->n_erased = nErased;
    std::memcpy(out->stats, stats, sizeof stats);
    return RUMI_OK;
}
