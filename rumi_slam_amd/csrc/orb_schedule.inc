// The scheduler of every extraction: extract_async_impl enqueues the stages of a call in one of three stream arrangements (the resident queue,
// equal sub-chunks, one stream) and the device-batch entries that are nothing but a call of it.

// Output addressing of one call: frame f's key-points start at kp + f * kpStride (bytes), likewise descriptors and the {n, monoIndex} pair.
// The three-array form has strides cap * 28 / cap * 32 / 8; the record form (one all-gather payload) has the record size for all three.
struct OutLayout { void *kp; long long kpStride; void *desc; long long descStride; void *counts; long long countsStride; };

static OutLayout three_array_layout(void *d_kp, void *d_desc, void *d_counts, int32_t cap) {
    return OutLayout{d_kp, (long long)cap * (long long)sizeof(RumiKeyPoint), d_desc, (long long)cap * 32, d_counts, 8};
}
// One fixed-capacity record per frame, {int32 n; int32 monoIndex; RumiKeyPoint kp[cap]; uint8 desc[cap][32]} = 8 + 60 cap bytes: the payload of the
// rumination queue's single all-gather (SURVEY.md section 8e).  record_bytes >= that size and a multiple of 4.
static int record_layout(const char *entry, void *d_records, int64_t record_bytes, int32_t cap, OutLayout *out) {
    if (!d_records || cap < 1 || record_bytes < 8 + 60ll * cap || (record_bytes & 3)) { g_lastError = std::string(entry) + ": bad record size"; return RUMI_E_INVALID; }
    uint8_t *r = (uint8_t *)d_records;
    *out = OutLayout{r + 8, record_bytes, r + 8 + (size_t)cap * sizeof(RumiKeyPoint), record_bytes, r, record_bytes};
    return RUMI_OK;
}

// What ONE call asks of the scheduler beyond its arguments.  The entry that needs any of it builds it on its stack and passes it down: nothing of it
// lives in the handle, so no entry, refused or not, can leave it behind for the next one.
struct CallOpts {
    size_t out1Bytes = 0;             // > 0: rumi_orb_extract wants that much of its result block copied dOut1 -> hOut1 before the call's one synchronisation
    bool zeroCopyOut = false;         // a one-frame call whose results go straight to pinned host memory: k_assemble publishes the final error word to dhErr
    bool hostImagePending = false;    // the frame of this call still sits in hIn (w x hgt, pitch wp): it is copied to dIn on the call's stream
    std::function<int(int, hipStream_t)> feed;   // host-resident batches: makes the frames [0, upto) of the call resident and lets stream s wait for them
    // the record entry with a PINNED host destination: every sub-chunk's records [frame0, frame0 + n) follow its kernels to the host on the sub-chunk's
    // own stream, under the kernels of the sub-chunks behind it
    struct Mirror { uint8_t *host; const uint8_t *dev; long long row; } mirror = {nullptr, nullptr, 0};
};

static int extract_async_impl(RumiOrb *h, const void *d_imgs, int32_t nframes, int32_t w, int32_t hgt, int32_t stride, int64_t frame_stride,
                              int32_t lap0, int32_t lap1, const OutLayout &out, int32_t cap, void *hip_stream, const CallOpts &opts) {
    void *d_kp = out.kp, *d_desc = out.desc, *d_counts = out.counts;
    if (!h || !d_imgs || !d_kp || !d_desc || !d_counts || nframes < 1 || cap < 1 || stride < w) {
        g_lastError = "rumi_orb_extract_batch_device: bad argument";
        return RUMI_E_INVALID;
    }
    if (w <= 0 || hgt <= 0) return RUMI_E_EMPTY;
    if (nframes > h->cfg.max_batch) { g_lastError = "nframes > max_batch"; return RUMI_E_CAPACITY; }
    if (h->scratchFrames <= 0 || h->arenaFrames <= 0) { g_lastError = "the handle has no device arenas (an earlier rumi_orb_set_resident_queue failed to allocate them)"; return RUMI_E_CAPACITY; }
    HIP_TRY(hipSetDevice(h->device));
    int rc;
    if (h->pending && (h->gw != w || h->gh != hgt) && (rc = rumi_orb_sync(h)) != RUMI_OK) return rc;   // new tables must not overtake running kernels
    rc = set_geometry(h, w, hgt);
    if (rc != RUMI_OK) return rc;
    hipStream_t st = (hipStream_t)hip_stream;
    // calls not yet waited for share the scratch arenas in stream order: another stream (or the profiled path) waits for them first
    if (h->pending && (st != h->pendingStream || h->profiling)) { rc = rumi_orb_sync(h); if (rc != RUMI_OK) return rc; }
    const DevParams &P = h->hP;
    if (!h->pending) { h->octStatBase[0] = (uint32_t)h->hErr[1]; h->octStatBase[1] = (uint32_t)h->hErr[2]; }   // rumi_orb_octree_stats counts from an idle handle
    if (h->octDirty) {           // an earlier call failed between its compaction and its quadtree launch: the pipeline's zero state is restored first
        HIP_TRY(hipDeviceSynchronize());
        if (const int rz = zero_octree_state(h); rz != RUMI_OK) return rz;
        h->octDirty = false;
    }
    // Level 0 is read where the caller has it, as aligned dwords.  Frames whose base, pitch or frame stride is not a multiple of 4 are
    // first copied into an aligned staging arena (the only case that costs a copy).
    bool stagedL0 = false;       // the frames were copied on `st`: the slot streams of a resident call must then wait for `st` (below)
    if ((reinterpret_cast<uintptr_t>(d_imgs) & 3) || (stride & 3) || (frame_stride & 3)) {
        stagedL0 = true;
        const int wp = (w + 3) & ~3;
        if (!h->dL0) HIP_TRY(hipMalloc((void **)&h->dL0, (size_t)((h->cfg.max_width + 3) & ~3) * h->cfg.max_height * h->cfg.max_batch));
        for (int f = 0; f < nframes; f++)
            HIP_TRY(hipMemcpy2DAsync(h->dL0 + (size_t)f * wp * hgt, wp, (const uint8_t *)d_imgs + (long long)f * frame_stride, stride, w, hgt,
                                     hipMemcpyDeviceToDevice, st));
        d_imgs = h->dL0; stride = wp; frame_stride = (int64_t)wp * hgt;
    }
    ImgSrc src{(const uint8_t *)d_imgs, frame_stride, stride, h->dPyr, h->dBlur};
    const bool prof = h->profiling;
    float acc[8] = {0};
    h->tapValid = false;

    // Stage A: pyramid + blur.  Levels depend on each other, frames do not.  The blur runs on a side stream next to FAST / quadtree and
    // joins before rBRIEF (stage times are taken with the same overlap the timed path has).
    // RUMI_SERIAL=1 (profiling aid): everything on the caller's stream, so that every kernel's duration is its stand-alone duration.
    static const bool serial = std::getenv("RUMI_SERIAL") != nullptr;
    // Batches of 64 frames and more are pipelined: sub-chunks of frames run pyramid -> FAST -> ... -> rBRIEF on up to 4 streams (sub-chunk j
    // on stream j % parts, in scratch slot j % parts), so the narrow launches of one sub-chunk (upper pyramid levels, compaction, quadtree:
    // latency-bound, few waves) sit beside the wide VALU-bound ones of the others.  Profiling and RUMI_SERIAL keep one stream.
    const int parts = (!prof && !serial) ? std::min(4, std::max(nframes / 32, 1)) : 1;
    const bool resident = h->residentQueue && !prof && !serial && !opts.feed;
    // the call's error word starts at zero: a memset on the caller's stream, or -- a call that runs as one part on that stream (a handful of
    // frames: every dispatch counts) -- a store by the first pyramid kernel, which nothing that writes the word precedes
    bool clearInKernel = !h->pending && parts == 1 && !resident && P.nlevels > 1;
    if (!h->pending && !clearInKernel) HIP_TRY(hipMemsetAsync(h->dErr, 0, sizeof(int32_t), st));
    if (h->userReady && !resident) { HIP_TRY(hipStreamWaitEvent(st, h->userReady, 0)); h->userReady = nullptr; }
    using Lane = RumiOrb::Lane;
    auto lane_of = [&](int slot) -> Lane {
        if (resident && h->plan.blurInline) return {h->slot[slot].s, h->slot[slot].s, nullptr, nullptr};   // the blur in line: behind the pyramid on the slot's own stream
        if (slot || resident) return h->slot[slot];      // (in the resident queue no slot runs on the caller's stream)
        return {st, serial || prof ? st : h->sideStream, h->evFork, h->evJoin};        // profiling: the blur on the call's stream too, so that every stage time is a stand-alone duration
    };
    // A few frames (the Tracking thread's call): FAST and the blur go out as ONE launch on the main stream (k_fast_blur).  As two launches the
    // blur runs on the side stream, and the event that forks it stalls the main queue for ~20 us on this runtime: more than the blur takes.
    const bool fuseBlur = !prof && !serial && nframes < 16 && fast_blur_fusable(P);
    // Up to 4 frames: the pyramid in ONE launch (k_pyramid_tiles) instead of a launch per level.  (Batches keep the per-level launches: a
    // workgroup walks seven levels between barriers and its threads idle on the small ones, which costs more than the saved re-reads bring.)
    const bool tilePyramid = !prof && !serial && nframes <= 4 && h->nPyrTiles > 0;
    // the streams this call's arrangement drives (made at its first use: ensure_lanes)
    if (resident) rc = ensure_lanes(h, 0, h->plan.streams, !h->plan.blurInline);
    else if (parts > 1) rc = ensure_lanes(h, 1, parts, true);
    if (rc == RUMI_OK && !resident && !serial && !prof && !fuseBlur) rc = ensure_side(h);
    if (rc != RUMI_OK) return rc;
    auto stage_a = [&](const ImgSrc &ps, int n, const Lane &L) -> int {
        hipStream_t s = L.s;
        if (prof) HIP_TRY(hipEventRecord(h->ev[0], s));
        if (tilePyramid) {
            launch_pyramid_tiles(h->dP, ps, h->dCoef, h->dRowTab, h->dPyrTiles, h->nPyrTiles, h->pyrBuf, h->pyrTab, n, s, clearInKernel ? h->dErr : nullptr);
            clearInKernel = false;
        } else
        for (int l = 1; l < P.nlevels; l++) {
            launch_resize(h->dP, P, ps, h->dCoef, h->dRowTab, l, n, s, clearInKernel ? h->dErr : nullptr);
            clearInKernel = false;
        }
        if (prof) HIP_TRY(hipEventRecord(h->ev[1], s));
        if (fuseBlur) return RUMI_OK;
        const bool forked = L.bs != s;           // (in line -- the resident queue's plan, RUMI_SERIAL, profiling -- stream order is the fork and the join)
        if (forked) {
            HIP_TRY(hipEventRecord(L.fork, s));
            HIP_TRY(hipStreamWaitEvent(L.bs, L.fork, 0));
        }
        if (prof) HIP_TRY(hipEventRecord(h->evB0, L.bs));
        launch_blur(h->dP, P, ps, n, h->cfg.blur_variant, L.bs);
        if (prof) HIP_TRY(hipEventRecord(h->evB1, L.bs));
        if (forked) HIP_TRY(hipEventRecord(L.join, L.bs));
        HIP_TRY(hipGetLastError());
        return RUMI_OK;
    };
    // rumi_orb_extract's frame, still in pinned host memory: copied to dIn first.  (Reading it over PCIe in the one-launch pyramid instead was
    // measured slower: 124.8 against 99.8 us per call.)
    if (opts.hostImagePending)
        HIP_TRY(hipMemcpyAsync(h->dIn, h->hIn, (size_t)stride * hgt, hipMemcpyHostToDevice, st));
    if (parts == 1 && !resident) {
        if (opts.feed && (rc = opts.feed(nframes, st)) != RUMI_OK) return rc;
        if ((rc = stage_a(src, nframes, lane_of(0))) != RUMI_OK) return rc;
    }

    // FAST -> compaction -> quadtree -> orientation + descriptors for the frames [frame0, frame0 + n) of the batch on stream s, in the scratch
    // arenas from frame slot scr0 on (every scratch array is indexed by frame slot, so disjoint slot ranges can run on different streams)
    // (arena0 >= 0: the sub-chunk's pyramid / blurred levels live at frame position arena0 of the arenas instead of at frame0)
    auto run_part = [&](int frame0, int n, int scr0, const Lane &L, bool timed, bool withStageA, int arena0) -> int {
        hipStream_t s = L.s;
        ImgSrc ps = src;
        ps.l0 = src.l0 + (long long)frame0 * frame_stride;
        ps.pyr = src.pyr + (long long)(arena0 >= 0 ? arena0 : frame0) * P.arenaStride;
        ps.blur = src.blur + (long long)(arena0 >= 0 ? arena0 : frame0) * P.arenaStride;
        if (withStageA) { const int ra = stage_a(ps, n, L); if (ra != RUMI_OK) return ra; }
        uint32_t *cellBuf = h->dCellBuf + (size_t)scr0 * P.totalCells * P.maxCellCand;
        int32_t *cellCnt = h->dCellCnt + (size_t)scr0 * P.totalCells;
        uint32_t *candp = h->dCand + (size_t)scr0 * P.totalCand;
        int32_t *lvStart = h->dLevelStart + (size_t)scr0 * (kMaxLevels + 1);
        uint32_t *selLevel = h->dSelLevel + (size_t)scr0 * P.nlevels * h->selLevelCap;
        int32_t *selLevelCnt = h->dSelLevelCnt + (size_t)scr0 * P.nlevels;
        uint32_t *selPacked = h->dSelPacked + (size_t)scr0 * h->capSel, *selMeta = h->dSelMeta + (size_t)scr0 * h->capSel;
        if (timed) HIP_TRY(hipEventRecord(h->ev[3], s));
        if (fuseBlur) (void)launch_fast_blur(h->dP, P, ps, cellBuf, cellCnt, n, h->cfg.blur_variant, s);
        else launch_fast(h->dP, P, ps, cellBuf, cellCnt, n, s);
        if (timed) HIP_TRY(hipEventRecord(h->ev[4], s));
        // batches: the quadtree pipeline starts from the cell histogram the compaction counts (this slot range's blocks)
        const bool octPipe = octree_plan(P, n) > 1;
        const size_t octRow = (size_t)scr0 * (size_t)(h->capOctCells / 2);
        const OctNarrow Q{h->dOctHist + octRow, h->dOctRank + octRow, h->dOctM + (size_t)scr0 * P.nlevels, h->dOctRedo + (size_t)scr0 * P.nlevels,
                          h->dOctCtl + (size_t)scr0 * 4, h->dErr + 1, h->dOctBins};
        // INVARIANT of the pipeline: the histogram rows and the redo counters are zero between launches (k_octree_narrow clears what it reads).
        // A return between the compaction and the quadtree launch would leave counted cells behind and every later tree of the handle wrong,
        // so the handle is marked until the quadtree is queued; a marked handle zeroes both before its next call (below, octDirty).
        if (octPipe) h->octDirty = true;
        launch_compact(h->dP, P, cellBuf, cellCnt, candp, lvStart, h->dErr, n, s, octPipe ? Q.hist : nullptr, h->dOctBins);
        if (timed) HIP_TRY(hipEventRecord(h->ev[5], s));
        launch_octree(h->dP, P, candp, lvStart, h->dOwner + (size_t)scr0 * P.totalCand, selLevel, selLevelCnt, h->selLevelCap, h->dErr, n, h->octLds, Q, s);
        h->octDirty = false;
        // a few frames: the slot assignment (k_assemble) inside the descriptor kernel's prologue, one launch less on the dependent chain
        const bool fuseAssemble = !timed && !serial && n <= 4 && (long long)((h->capSel + 7) / 8) * n <= 2048;
        int32_t *countsOut = (int32_t *)((uint8_t *)d_counts + (size_t)frame0 * out.countsStride);
        if (!fuseAssemble)
            launch_assemble(h->dP, selLevel, selLevelCnt, h->selLevelCap, lap0, lap1, selPacked, selMeta, h->dSelCount + scr0, h->capSel,
                            countsOut, out.countsStride, h->dErr, n, s, opts.zeroCopyOut ? h->dhErr : nullptr);
        if (timed) HIP_TRY(hipEventRecord(h->ev[6], s));
        // batches: IC_Angle and the trigonometry in a kernel of their own, BEFORE the join (it reads the un-blurred levels only)
        float4 *trig = !fuseAssemble && orient_desc_split(h->capSel, n) ? h->dSelTrig + (size_t)scr0 * h->capSel : nullptr;
        if (trig) launch_disc_angle(h->dP, ps, selPacked, selMeta, h->dSelCount + scr0, h->capSel, h->capSel, h->dDiscVec, trig, n, s);
        if (!fuseBlur && L.bs != s) HIP_TRY(hipStreamWaitEvent(s, L.join, 0));   // join: rBRIEF reads the blurred levels
        if (fuseAssemble)
            launch_assemble_orient_desc(h->dP, ps, selLevel, selLevelCnt, h->selLevelCap, lap0, lap1, countsOut, out.countsStride, h->dErr,
                                        opts.zeroCopyOut ? h->dhErr : nullptr, selPacked, selMeta, h->dSelCount + scr0, h->capSel, h->capSel,
                                        (RumiKeyPoint *)((uint8_t *)d_kp + (size_t)frame0 * out.kpStride), out.kpStride,
                                        (uint8_t *)d_desc + (size_t)frame0 * out.descStride, out.descStride, cap, n, s);
        else
        launch_orient_desc(h->dP, ps, selPacked, selMeta, h->dSelCount + scr0, h->capSel, h->capSel,
                           (RumiKeyPoint *)((uint8_t *)d_kp + (size_t)frame0 * out.kpStride), out.kpStride,
                           (uint8_t *)d_desc + (size_t)frame0 * out.descStride, out.descStride, cap, n, s, trig);
        if (timed) HIP_TRY(hipEventRecord(h->ev[7], s));
        const CallOpts::Mirror &mr = opts.mirror;
        if (mr.host) HIP_TRY(hipMemcpyAsync(mr.host + (size_t)frame0 * mr.row, mr.dev + (size_t)frame0 * mr.row, (size_t)n * mr.row, hipMemcpyDeviceToHost, s));
        return RUMI_OK;
    };
    if (resident) {
        // Resident queue: the plan's fixed slots (stream, scratch range, pyramid / blur arena range; a blur stream only where the hardware
        // queues have room for it), sub-chunks of at most 256 frames dealt to the slots round-robin ACROSS calls (a 64-frame call takes one
        // slot, the next call the next one).  The plan may drive fewer slots than the caller asked for (orb_geom.h: stream_plan): a call
        // then puts consecutive sub-chunks on one stream, which stream order covers like consecutive calls.  Everything a sub-chunk
        // touches on the device belongs to its slot, so stream order alone keeps consecutive users of a slot apart: no sub-chunk waits for
        // the caller's stream or for another slot -- except after a rumi_orb_sync, whose reset of the error word is queued on `st`.
        // With the blur in line a slot has ONE stream and both arena hazards rest on its order, nothing else:
        //   - a sub-chunk's blur writes the slot's blurred arena, which the previous sub-chunk's k_orient_desc on that slot read: the blur
        //     is enqueued behind it on the same stream;
        //   - a sub-chunk's pyramid overwrites the levels the previous sub-chunk's k_disc_angle and k_fast_cells read (and its blur):
        //     all of them precede it on the same stream.
        // (With blur streams the second hazard has a gap the join closes: the blur stream's join is waited for before k_orient_desc, so
        // the previous blur has ended before the slot's next pyramid starts.)
        constexpr int kMaxSlots = RumiOrb::kMaxParts;
        const int kSlots = h->plan.streams;
        const int slotFrames = h->scratchFrames / kSlots;
        const int cap64 = std::min(kResidentSub, slotFrames);
        const int nsub = (nframes + cap64 - 1) / cap64, sub = (nframes + nsub - 1) / nsub;
        // (unaligned frames were staged into dL0 by copies queued on `st`: every slot stream this call touches waits for them.  The previous
        // call's readers of dL0 are behind `st` already: the caller's stream waited for that call's results at its end.)
        const bool fork = !h->pending || !h->lastResident || stagedL0;
        if (fork) HIP_TRY(hipEventRecord(h->evPartFork, st));
        bool touched[kMaxSlots] = {false, false, false, false, false, false, false, false};
        for (int j = 0, base = 0; base < nframes; j++, base += sub) {
            const int n = std::min(sub, nframes - base), slot = (h->rot + j) % kSlots;
            const Lane L = lane_of(slot);
            if (fork && !touched[slot]) HIP_TRY(hipStreamWaitEvent(L.s, h->evPartFork, 0));
            if (h->userReady && !touched[slot]) HIP_TRY(hipStreamWaitEvent(L.s, h->userReady, 0));
            touched[slot] = true;
            rc = run_part(base, n, slot * slotFrames, L, false, true, slot * slotFrames);
            if (rc != RUMI_OK) return rc;
            h->lastChunkBase = base; h->lastChunkFrames = n; h->lastChunkSlot = slot * slotFrames;
        }
        h->rot = (h->rot + nsub) % kSlots;
        h->userReady = nullptr;
        // Join: the caller's stream waits for the results of every sub-chunk (an event per slot, taken after the slot's last sub-chunk)
        for (int p = 0; p < kSlots; p++)
            if (touched[p]) {
                HIP_TRY(hipEventRecord(h->slotJoin[p], h->slot[p].s));
                HIP_TRY(hipStreamWaitEvent(st, h->slotJoin[p], 0));
            }
        HIP_TRY(hipGetLastError());
    } else if (parts > 1) {
        // equal sub-chunks: rounds of `parts` sub-chunks, as few rounds as the slots allow, no short tail
        const int slotFrames = h->scratchFrames / parts;
        const int subMax = std::max(1, std::min(slotFrames, 64));      // (64: the host path's transfer groups; the arenas may hold more since the resident queue grew them)
        const int rounds = (nframes + parts * subMax - 1) / (parts * subMax), sub = (nframes + parts * rounds - 1) / (parts * rounds);
        HIP_TRY(hipEventRecord(h->evPartFork, st));
        int used = 0;
        for (int j = 0, base = 0; base < nframes; j++, base += sub) {
            const int n = std::min(sub, nframes - base), slot = j % parts;
            const Lane L = lane_of(slot);
            if (j < parts && slot) HIP_TRY(hipStreamWaitEvent(L.s, h->evPartFork, 0));
            if (opts.feed && (rc = opts.feed(base + n, L.s)) != RUMI_OK) return rc;
            rc = run_part(base, n, slot * slotFrames, L, false, true, -1);
            if (rc != RUMI_OK) return rc;
            used = std::max(used, slot + 1);
            h->lastChunkBase = base; h->lastChunkFrames = n; h->lastChunkSlot = slot * slotFrames;
        }
        for (int p = 1; p < used; p++) {
            HIP_TRY(hipEventRecord(h->slotJoin[p], h->slot[p].s));
            HIP_TRY(hipStreamWaitEvent(st, h->slotJoin[p], 0));
        }
        HIP_TRY(hipGetLastError());
    } else {
        // one stream: chunks of kChunk frames reuse the scratch arenas in stream order
        for (int base = 0; base < nframes; base += kChunk) {
            const int nf = std::min(kChunk, nframes - base);
            rc = run_part(base, nf, 0, lane_of(0), prof, false, -1);
            if (rc != RUMI_OK) return rc;
            HIP_TRY(hipGetLastError());
            if (prof) {
                float ms;
                HIP_TRY(hipStreamSynchronize(st));
                HIP_TRY(hipEventElapsedTime(&ms, h->ev[3], h->ev[4])); acc[1] += ms;
                HIP_TRY(hipEventElapsedTime(&ms, h->ev[4], h->ev[5])); acc[2] += ms;
                HIP_TRY(hipEventElapsedTime(&ms, h->ev[5], h->ev[6])); acc[4] += ms;
                HIP_TRY(hipEventElapsedTime(&ms, h->ev[6], h->ev[7])); acc[5] += ms;
            }
            h->lastChunkBase = base; h->lastChunkFrames = nf; h->lastChunkSlot = 0;
        }
    }
    // The call's error word (and, for the single-frame host API, its result block) follow the kernels on the stream; rumi_orb_sync waits
    // for them.  Nothing here blocks, so a caller can queue the next batch while this one runs.
    if (opts.out1Bytes) HIP_TRY(hipMemcpyAsync(h->hOut1, h->dOut1, opts.out1Bytes, hipMemcpyDeviceToHost, st));
    if (!opts.zeroCopyOut) HIP_TRY(hipMemcpyAsync(h->hErr, h->dErr, 3 * sizeof(int32_t), hipMemcpyDeviceToHost, st));   // with the quadtree's counters (zero-copy: k_assemble has published the error word)
    h->pending = true; h->pendingStream = st;
    if (prof) {
        float ms;
        HIP_TRY(hipStreamSynchronize(st));
        HIP_TRY(hipEventElapsedTime(&ms, h->ev[0], h->ev[1])); acc[0] = ms;
        HIP_TRY(hipEventElapsedTime(&ms, h->evB0, h->evB1)); acc[3] = ms;
        HIP_TRY(hipEventElapsedTime(&ms, h->ev[0], h->ev[7])); acc[6] = ms;
        for (int i = 0; i < 8; i++) h->stageMs[i] = acc[i];
    }
    h->lastSrc = src; h->lastFrames = nframes;
    h->lastResident = resident;
    if (resident) {      // the arenas hold the pyramids of the last sub-chunk of each slot only; the taps serve the call's last sub-chunk
        h->lastSrc.pyr = src.pyr + ((long long)h->lastChunkSlot - h->lastChunkBase) * P.arenaStride;
        h->lastSrc.blur = src.blur + ((long long)h->lastChunkSlot - h->lastChunkBase) * P.arenaStride;
    }
    h->lastKp = (RumiKeyPoint *)d_kp; h->lastKpStride = out.kpStride; h->lastOutCap = cap;
    h->lastCounts = (int32_t *)d_counts;
    return RUMI_OK;
}

extern "C" int rumi_orb_extract_batch_device_async(RumiOrb *h, const void *d_imgs, int32_t nframes, int32_t w, int32_t hgt,
                                                   int32_t stride, int64_t frame_stride, int32_t lap0, int32_t lap1,
                                                   void *d_kp, void *d_desc, void *d_counts, int32_t cap, void *hip_stream) {
    return extract_async_impl(h, d_imgs, nframes, w, hgt, stride, frame_stride, lap0, lap1, three_array_layout(d_kp, d_desc, d_counts, cap), cap, hip_stream, CallOpts{});
}

// The end of a synchronous entry: the one synchronisation; a call that failed after it had queued work waits for that work before it returns.
static int end_call(RumiOrb *h, int rc) {
    if (rc != RUMI_OK) { if (h && h->pending) (void)rumi_orb_sync(h); return rc; }
    return rumi_orb_sync(h);
}

extern "C" int rumi_orb_extract_batch_device(RumiOrb *h, const void *d_imgs, int32_t nframes, int32_t w, int32_t hgt,
                                             int32_t stride, int64_t frame_stride, int32_t lap0, int32_t lap1,
                                             void *d_kp, void *d_desc, void *d_counts, int32_t cap, void *hip_stream) {
    return end_call(h, rumi_orb_extract_batch_device_async(h, d_imgs, nframes, w, hgt, stride, frame_stride, lap0, lap1, d_kp, d_desc, d_counts, cap, hip_stream));
}

// The record form (record_layout) of rumi_orb_extract_batch_device_async.
extern "C" int rumi_orb_extract_batch_records_async(RumiOrb *h, const void *d_imgs, int32_t nframes, int32_t w, int32_t hgt,
                                                    int32_t stride, int64_t frame_stride, int32_t lap0, int32_t lap1,
                                                    void *d_records, int64_t record_bytes, int32_t cap, void *hip_stream) {
    OutLayout out;
    if (const int rc = record_layout("rumi_orb_extract_batch_records", d_records, record_bytes, cap, &out); rc != RUMI_OK) return rc;
    return extract_async_impl(h, d_imgs, nframes, w, hgt, stride, frame_stride, lap0, lap1, out, cap, hip_stream, CallOpts{});
}
