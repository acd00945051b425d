// One frame per call from host memory: rumi_orb_extract, and the streaming front-end that keeps the previous frame resident and matches against it.

// The handle's pinned staging buffer for a w x hgt frame, for a caller that lets its camera driver / decoder write the frame there (a cv::Mat
// constructed on this memory): rumi_orb_extract called with this pointer and stride skips its staging copy.
extern "C" int rumi_orb_image_buffer(RumiOrb *h, int32_t w, int32_t hgt, uint8_t **buf, int32_t *stride) {
    if (!h || !buf || !stride) return RUMI_E_INVALID;
    if (w <= 0 || hgt <= 0 || w > h->cfg.max_width || hgt > h->cfg.max_height) { g_lastError = "rumi_orb_image_buffer: frame larger than the handle was created for"; return RUMI_E_CAPACITY; }
    *buf = h->hIn; *stride = (w + 3) & ~3;
    return RUMI_OK;
}

// The frame of a one-frame call into the pinned staging buffer, rows padded to wp so that level 0 can be read as aligned dwords; extract_async_impl
// copies it to dIn on the call's stream (CallOpts::hostImagePending).  A caller that captured straight into rumi_orb_image_buffer's memory has
// nothing to stage.
static void stage_host_frame(RumiOrb *h, const uint8_t *img, int w, int hgt, int stride, int wp) {
    if (img == h->hIn && stride == wp) return;
    for (int y = 0; y < hgt; y++) std::memcpy(h->hIn + (size_t)y * wp, img + (size_t)y * stride, (size_t)w);
}

// One frame, already staged in hIn (fromStaging: it is copied to dIn on the call's stream) or already resident at `dImg` (rows wp bytes apart), through the
// extractor into the handle's pinned result block hOut1 = [counts {n, monoIndex} | key-points capSel x 28 at +16 | descriptors capSel x 32]: one
// synchronisation in all.
static int extract_one_to_pinned(RumiOrb *h, const uint8_t *dImg, int w, int hgt, int wp, int lap0, int lap1, bool fromStaging) {
    // Results straight into pinned host memory: the kernels' output pointers are the device's view of hOut1 (k_assemble writes the counts and the
    // final error word, k_orient_desc key-points and descriptors), so the call ends with its last kernel -- no copy back, no second copy for the
    // error word (two dependent transfers of ~6 + 2 us with ~9 us of queue latency each).  Profiling keeps the copies.
    const bool zero = h->dhOut1 && h->dhErr && !h->profiling;
    uint8_t *ob = zero ? h->dhOut1 : h->dOut1;
    int32_t *dC = reinterpret_cast<int32_t *>(ob);
    RumiKeyPoint *dK = reinterpret_cast<RumiKeyPoint *>(ob + 16);
    uint8_t *dD = ob + 16 + (size_t)h->capSel * sizeof(RumiKeyPoint);
    CallOpts opts;
    opts.hostImagePending = fromStaging; opts.zeroCopyOut = zero; opts.out1Bytes = zero ? 0 : (size_t)16 + (size_t)h->capSel * 60;
    if (zero) *h->hErr = 0;
    return end_call(h, extract_async_impl(h, dImg, 1, w, hgt, wp, (int64_t)wp * hgt, lap0, lap1, three_array_layout(dK, dD, dC, h->capSel), h->capSel, nullptr, opts));
}

extern "C" int rumi_orb_extract(RumiOrb *h, const uint8_t *img, int32_t w, int32_t hgt, int32_t stride, int32_t lap0,
                                int32_t lap1, RumiKeyPoint *kp_out, uint8_t *desc_out, int32_t cap, int32_t *n_out,
                                int32_t *mono_out) {
    if (n_out) *n_out = 0;
    if (mono_out) *mono_out = -1;
    if (!h || !n_out || !mono_out) return RUMI_E_INVALID;
    if (!img || w <= 0 || hgt <= 0) return RUMI_E_EMPTY;            // operator() returns -1 on an empty image
    if (stride < w || w > h->cfg.max_width || hgt > h->cfg.max_height) { g_lastError = "image size"; return RUMI_E_INVALID; }
    HIP_TRY(hipSetDevice(h->device));
    // image -> pinned -> device (async), kernels, [counts | key-points | descriptors] -> pinned
    const int wp = (w + 3) & ~3;
    stage_host_frame(h, img, w, hgt, stride, wp);
    const int rc = extract_one_to_pinned(h, h->dIn, w, hgt, wp, lap0, lap1, true);
    if (rc != RUMI_OK) return rc;
    const int32_t *counts = reinterpret_cast<const int32_t *>(h->hOut1);
    *n_out = counts[0];
    *mono_out = counts[1];
    if (counts[0] > cap) { g_lastError = "kp_out/desc_out capacity"; return RUMI_E_CAPACITY; }
    if (counts[0] > 0) {
        if (!kp_out || !desc_out) return RUMI_E_INVALID;
        std::memcpy(kp_out, h->hOut1 + 16, (size_t)counts[0] * sizeof(RumiKeyPoint));
        std::memcpy(desc_out, h->hOut1 + 16 + (size_t)h->capSel * sizeof(RumiKeyPoint), (size_t)counts[0] * 32);
    }
    return RUMI_OK;
}

// ---- the streaming front-end: the previous frame stays resident, one call per frame ------------------------------------------------------
// Two slots in HBM, each [counts {n, monoIndex, -, -} | key-points cap x 28, padded to 16 bytes | descriptors cap x 32]; frame t is extracted
// into slot t & 1 and matched (k_bruteforce_pair, match.hip) as query against the other slot as train, on the extraction's stream.  The pinned
// block has a slot's layout followed by the three result rows; the pair kernel writes all of it through the device's view of the block (its
// mirror: counts, key-points, descriptors, results), so a push is kernels only and ends with one synchronisation.  Without a device view of
// pinned memory, or with profiling on, the kernels write device memory and two copies follow them.
struct RumiOrbStream {
    RumiOrb *h = nullptr;
    int cap = 0;
    size_t kpOff = 16, descOff = 0, slotBytes = 0, resOff = 0, blockBytes = 0;
    uint8_t *dSlots = nullptr;       // two slots
    int32_t *dZero = nullptr;        // the train count of a first frame
    uint8_t *dScratch = nullptr;     // k_bruteforce_pair's partials and tickets, zeroed once
    int32_t *dRes = nullptr;         // three result rows of cap (the copy path reads them; the mirror path leaves the same values here)
    uint8_t *hBlock = nullptr, *dhBlock = nullptr;
    long long t = 0;                 // frames pushed successfully
    bool hasPrev = false;
    int nPrev = 0;
};

extern "C" void rumi_orb_stream_destroy(RumiOrbStream *s) {
    if (!s) return;
    if (s->h) { (void)hipSetDevice(s->h->device); if (s->h->pending) (void)hipStreamSynchronize(s->h->pendingStream); }
    for (void *p : {(void *)s->dSlots, (void *)s->dZero, (void *)s->dScratch, (void *)s->dRes}) if (p) (void)hipFree(p);
    if (s->hBlock) (void)hipHostFree(s->hBlock);
    delete s;
}

extern "C" int rumi_orb_stream_create(RumiOrb *h, RumiOrbStream **out) {
    if (!out) return RUMI_E_INVALID;
    *out = nullptr;
    if (!h) return RUMI_E_INVALID;
    HIP_TRY(hipSetDevice(h->device));
    RumiOrbStream *s = new RumiOrbStream();
    s->h = h; s->cap = h->capSel;
    const size_t cap = (size_t)s->cap;
    s->descOff = s->kpOff + ((cap * sizeof(RumiKeyPoint) + 15) & ~(size_t)15);
    s->slotBytes = s->descOff + cap * 32;                       // a multiple of 16
    s->resOff = s->slotBytes;
    s->blockBytes = s->resOff + 3 * cap * sizeof(int32_t);
    const size_t scratchBytes = (size_t)rumi_match_bruteforce_pair_scratch_bytes(s->cap);
    int rc = RUMI_OK;
    if ((rc = dev_alloc(&s->dSlots, 2 * s->slotBytes)) != RUMI_OK || (rc = dev_alloc(&s->dZero, 4)) != RUMI_OK ||
        (rc = dev_alloc(&s->dScratch, scratchBytes)) != RUMI_OK || (rc = dev_alloc(&s->dRes, 3 * cap)) != RUMI_OK ||
        (rc = pin_alloc(&s->hBlock, s->blockBytes)) != RUMI_OK) { rumi_orb_stream_destroy(s); return rc; }
    if (hipMemset(s->dSlots, 0, 2 * s->slotBytes) != hipSuccess || hipMemset(s->dZero, 0, 4 * sizeof(int32_t)) != hipSuccess ||
        hipMemset(s->dScratch, 0, scratchBytes) != hipSuccess || hipDeviceSynchronize() != hipSuccess) {
        rumi_orb_stream_destroy(s); g_lastError = "rumi_orb_stream_create: clearing the slots failed"; return RUMI_E_NO_DEVICE;
    }
    std::memset(s->hBlock, 0, s->blockBytes);
    if (hipHostGetDevicePointer((void **)&s->dhBlock, s->hBlock, 0) != hipSuccess) { (void)hipGetLastError(); s->dhBlock = nullptr; }
    *out = s;
    return RUMI_OK;
}

extern "C" int rumi_orb_stream_reset(RumiOrbStream *s) {
    if (!s) return RUMI_E_INVALID;
    s->hasPrev = false; s->nPrev = 0;
    return RUMI_OK;
}

extern "C" int rumi_orb_stream_resident(RumiOrbStream *s, void **d_kp, void **d_desc, void **d_counts) {
    if (!s || !d_kp || !d_desc || !d_counts) return RUMI_E_INVALID;
    if (s->t == 0) { g_lastError = "rumi_orb_stream_resident: no frame has been pushed"; return RUMI_E_INVALID; }
    uint8_t *slot = s->dSlots + (size_t)((s->t - 1) & 1) * s->slotBytes;
    *d_counts = slot; *d_kp = slot + s->kpOff; *d_desc = slot + s->descOff;
    return RUMI_OK;
}

extern "C" int rumi_orb_stream_push(RumiOrbStream *s, const uint8_t *img, int32_t w, int32_t hgt, int32_t stride, int32_t lap0, int32_t lap1,
                                    RumiStreamFrame *out) {
    if (out) { std::memset(out, 0, sizeof *out); out->mono = -1; }
    if (!s || !out) return RUMI_E_INVALID;
    RumiOrb *h = s->h;
    if (!img || w <= 0 || hgt <= 0) return RUMI_E_EMPTY;            // operator() returns -1 on an empty image
    if (stride < w || w > h->cfg.max_width || hgt > h->cfg.max_height) { g_lastError = "image size"; return RUMI_E_INVALID; }
    HIP_TRY(hipSetDevice(h->device));
    const int wp = (w + 3) & ~3;                                     // the staging rules of rumi_orb_extract
    stage_host_frame(h, img, w, hgt, stride, wp);
    const bool zero = s->dhBlock && h->dhErr && !h->profiling;
    uint8_t *cur = s->dSlots + (size_t)(s->t & 1) * s->slotBytes, *prev = s->dSlots + (size_t)((s->t + 1) & 1) * s->slotBytes;
    CallOpts opts;
    opts.hostImagePending = true; opts.zeroCopyOut = zero;           // (the error word goes straight to pinned memory; the frame goes to its slot)
    if (zero) *h->hErr = 0;
    int rc = extract_async_impl(h, h->dIn, 1, w, hgt, wp, (int64_t)wp * hgt, lap0, lap1, three_array_layout(cur + s->kpOff, cur + s->descOff, cur, s->cap), s->cap, nullptr, opts);
    if (rc == RUMI_OK) {
        const size_t cap = (size_t)s->cap;
        uint8_t *hb = s->dhBlock;
        const PairMirrorArgs mir{hb, cur + s->kpOff, hb + s->kpOff, hb + s->descOff, hb + s->resOff, hb + s->resOff + cap * 4, hb + s->resOff + cap * 8};
        rc = launch_bruteforce_pair(cur + s->descOff, cur, prev + s->descOff, s->hasPrev ? (const void *)prev : (const void *)s->dZero, s->cap,
                                    s->hasPrev ? s->nPrev : 0, 0, s->dScratch, s->dRes, s->dRes + cap, s->dRes + 2 * cap, zero ? &mir : nullptr, nullptr);
        if (rc == RUMI_OK && !zero) {
            if (hipMemcpyAsync(s->hBlock, cur, s->slotBytes, hipMemcpyDeviceToHost, nullptr) != hipSuccess ||
                hipMemcpyAsync(s->hBlock + s->resOff, s->dRes, 3 * cap * sizeof(int32_t), hipMemcpyDeviceToHost, nullptr) != hipSuccess) {
                g_lastError = "rumi_orb_stream_push: copy to the pinned block failed"; rc = RUMI_E_NO_DEVICE;
            }
        }
    }
    if ((rc = end_call(h, rc)) != RUMI_OK) return rc;               // the one synchronisation; a failing push leaves t, and so the previous frame, as it was
    int32_t *counts = reinterpret_cast<int32_t *>(s->hBlock);
    if (!zero) counts[2] = s->hasPrev ? s->nPrev : 0;
    const size_t cap = (size_t)s->cap;
    out->n = counts[0]; out->mono = counts[1]; out->n_prev = counts[2];
    out->kp = reinterpret_cast<const RumiKeyPoint *>(s->hBlock + s->kpOff);
    out->desc = s->hBlock + s->descOff;
    out->best_idx = reinterpret_cast<const int32_t *>(s->hBlock + s->resOff);
    out->best_dist = out->best_idx + cap; out->second_dist = out->best_idx + 2 * cap;
    s->t++; s->hasPrev = true; s->nPrev = counts[0];
    return RUMI_OK;
}
