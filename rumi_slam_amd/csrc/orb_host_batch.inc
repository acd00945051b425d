// Host-resident batch: the rumination queue holds its frames as host cv::Mats (CloudImageSampler.cc:148-170).  The frames travel to the device
// in groups of 64 on a copy stream of their own, each group's extraction waits only for its own group, so the transfers run under the kernels
// of the groups before it.  Pinned sources (hipHostMalloc / hipHostRegister) are copied from where they lie; pageable ones pass through four
// pinned staging slots filled by the handle's host threads.
// (opts: the entry's options, to which the feeder is added here; tail: copies the entry queues behind the kernels before the one synchronisation)
static int extract_batch_host_impl(RumiOrb *h, const uint8_t *const *imgs, int32_t nframes, int32_t w, int32_t hgt, int32_t stride,
                                   int32_t lap0, int32_t lap1, const OutLayout &out, int32_t cap, void *hip_stream, CallOpts &opts,
                                   const std::function<int(hipStream_t)> &tail) {
    if (!h || !imgs || !out.kp || !out.desc || !out.counts || nframes < 1 || cap < 1 || stride < w) {
        g_lastError = "rumi_orb_extract_batch_host: bad argument";
        return RUMI_E_INVALID;
    }
    if (w <= 0 || hgt <= 0) return RUMI_E_EMPTY;
    if (nframes > h->cfg.max_batch) { g_lastError = "nframes > max_batch"; return RUMI_E_CAPACITY; }
    for (int f = 0; f < nframes; f++) if (!imgs[f]) { g_lastError = "rumi_orb_extract_batch_host: null frame"; return RUMI_E_INVALID; }
    HIP_TRY(hipSetDevice(h->device));
    int rc;
    if (h->pending && (rc = rumi_orb_sync(h)) != RUMI_OK) return rc;
    const int wp = (w + 3) & ~3;
    const size_t frameBytes = (size_t)wp * hgt;
    if ((rc = h->hostIn.reserve(frameBytes * nframes, frameBytes * h->cfg.max_batch)) != RUMI_OK) return rc;
    if (!h->copyStream) {
        HIP_TRY(hipStreamCreateWithFlags(&h->copyStream, hipStreamNonBlocking));
        HIP_TRY(hipStreamCreateWithFlags(&h->copyStream2, hipStreamNonBlocking));
        for (auto &e : h->evFeed) HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    }
    // is the source pinned?  (one answer for the whole queue: the frames of a queue come from one allocator)
    hipPointerAttribute_t attr{};
    const bool pinned = hipPointerGetAttributes(&attr, imgs[0]) == hipSuccess && attr.type == hipMemoryTypeHost;
    (void)hipGetLastError();
    constexpr int G = RumiOrb::kFeedFrames, S = RumiOrb::kFeedSlots;
    if (!pinned && h->hFeedBytes < frameBytes * G) {
        for (auto &p : h->hFeed) { if (p) HIP_TRY(hipHostFree(p)); p = nullptr; }
        for (auto &p : h->hFeed) HIP_TRY(hipHostMalloc((void **)&p, (size_t)((h->cfg.max_width + 3) & ~3) * h->cfg.max_height * G, hipHostMallocDefault));
        h->hFeedBytes = (size_t)((h->cfg.max_width + 3) & ~3) * h->cfg.max_height * G;
    }
    hipStream_t st = (hipStream_t)hip_stream;
    int fed = 0, group = 0;                                    // frames already on their way, groups enqueued
    opts.feed = [&](int upto, hipStream_t s) -> int {
        while (fed < upto) {
            const int n = std::min(G, nframes - fed), slot = group % S;
            hipStream_t cs = (group & 1) ? h->copyStream2 : h->copyStream;
            if (group >= S) HIP_TRY(hipEventSynchronize(h->evFeed[slot]));       // the slot's previous group has left the pinned buffer / its event is free again
            bool dense = pinned && stride == wp;                               // one buffer, frames back to back: one transfer per group
            for (int f = 1; dense && f < n; f++) dense = imgs[fed + f] == imgs[fed] + (size_t)f * frameBytes;
            if (dense) {
                HIP_TRY(hipMemcpyAsync(h->hostIn.p + (size_t)fed * frameBytes, imgs[fed], frameBytes * n, hipMemcpyHostToDevice, cs));
            } else if (pinned) {
                for (int f = 0; f < n; f++)
                    HIP_TRY(hipMemcpy2DAsync(h->hostIn.p + (size_t)(fed + f) * frameBytes, wp, imgs[fed + f], stride, w, hgt, hipMemcpyHostToDevice, cs));
            } else {
                uint8_t *dst = h->hFeed[slot];
                const int nt = std::max(1, std::min(h->hostThreads, n));
                auto work = [&](int t) {
                    for (int f = t; f < n; f += nt)
                        for (int y = 0; y < hgt; y++) std::memcpy(dst + (size_t)f * frameBytes + (size_t)y * wp, imgs[fed + f] + (size_t)y * stride, (size_t)w);
                };
                std::vector<std::thread> th;
                for (int t = 1; t < nt; t++) th.emplace_back(work, t);
                work(0);
                for (auto &x : th) x.join();
                HIP_TRY(hipMemcpyAsync(h->hostIn.p + (size_t)fed * frameBytes, dst, frameBytes * n, hipMemcpyHostToDevice, cs));
            }
            HIP_TRY(hipEventRecord(h->evFeed[slot], cs));
            fed += n; group++;
        }
        // copies complete in order on each copy stream: waiting for the newest group of each covers every frame below `upto`
        HIP_TRY(hipStreamWaitEvent(s, h->evFeed[(group - 1) % S], 0));
        if (group >= 2) HIP_TRY(hipStreamWaitEvent(s, h->evFeed[(group - 2) % S], 0));
        return RUMI_OK;
    };
    rc = extract_async_impl(h, h->hostIn.p, nframes, w, hgt, wp, (int64_t)frameBytes, lap0, lap1, out, cap, hip_stream, opts);
    if (rc == RUMI_OK && tail) rc = tail(st);
    return end_call(h, rc);
}

extern "C" int rumi_orb_extract_batch_host(RumiOrb *h, const uint8_t *const *imgs, int32_t nframes, int32_t w, int32_t hgt, int32_t stride,
                                           int32_t lap0, int32_t lap1, void *d_kp, void *d_desc, void *d_counts, int32_t cap,
                                           RumiKeyPoint *h_kp, uint8_t *h_desc, int32_t *h_counts, void *hip_stream) {
    CallOpts opts;
    // host arrays: one copy each at the end.  (Copies behind every sub-chunk, as the record layout below has them, were measured slower for these
    // three arrays: they hold the sub-chunk streams while the uploads are the bottleneck.)
    return extract_batch_host_impl(h, imgs, nframes, w, hgt, stride, lap0, lap1, three_array_layout(d_kp, d_desc, d_counts, cap), cap, hip_stream, opts, [&](hipStream_t st) -> int {
        if (h_counts) HIP_TRY(hipMemcpyAsync(h_counts, d_counts, (size_t)nframes * 2 * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        if (h_kp) HIP_TRY(hipMemcpyAsync(h_kp, d_kp, (size_t)nframes * cap * sizeof(RumiKeyPoint), hipMemcpyDeviceToHost, st));
        if (h_desc) HIP_TRY(hipMemcpyAsync(h_desc, d_desc, (size_t)nframes * cap * 32, hipMemcpyDeviceToHost, st));
        return RUMI_OK;
    });
}

// The host-resident queue with ONE record per frame as output (the all-gather payload, rumi_orb_extract_batch_records_async's layout); h_records:
// optional host copy of the nframes records.
extern "C" int rumi_orb_extract_batch_host_records(RumiOrb *h, const uint8_t *const *imgs, int32_t nframes, int32_t w, int32_t hgt, int32_t stride,
                                                   int32_t lap0, int32_t lap1, void *d_records, int64_t record_bytes, int32_t cap, uint8_t *h_records,
                                                   void *hip_stream) {
    OutLayout out;
    if (const int rc = record_layout("rumi_orb_extract_batch_host_records", d_records, record_bytes, cap, &out); rc != RUMI_OK) return rc;
    // a pinned destination takes the records sub-chunk by sub-chunk behind the kernels (run_part); a pageable one (whose "asynchronous" copy would hold
    // the enqueuing thread) gets them in one copy at the end
    hipPointerAttribute_t attr{};
    const bool pinnedOut = h && h_records && hipPointerGetAttributes(&attr, h_records) == hipSuccess && attr.type == hipMemoryTypeHost;
    (void)hipGetLastError();
    CallOpts opts;
    if (pinnedOut) opts.mirror = {h_records, (const uint8_t *)d_records, record_bytes};
    return extract_batch_host_impl(h, imgs, nframes, w, hgt, stride, lap0, lap1, out, cap, hip_stream, opts, [&](hipStream_t st) -> int {
        if (h_records && !pinnedOut) HIP_TRY(hipMemcpyAsync(h_records, d_records, (size_t)nframes * record_bytes, hipMemcpyDeviceToHost, st));
        return RUMI_OK;
    });
}
