// The PD frame selector (include/rumi_kfd.h): KFDSample::Step (R/lib_src/KFDSample.cc:87-175) as one sampler on an extractor handle.  The flow
// kernels are flow.hip's (flow_device.h); the sampler lives here because a selected frame goes through this handle's extractor from where the
// flow left it on the device.
//
// Two slots hold a frame's three LK levels and their Scharr derivatives; frame t is built in the slot frame t - 1 does not occupy (pyramid and
// derivative when it arrives: it is the next step's previous frame) and the tracked points are followed from the other slot into it.  A tracking
// step is upload, [grey,] pyramid, Scharr, track, one copy back, one synchronisation; the controller is scalar host code with the reference's
// types.  A selected frame then runs the extractor on level 0 where it lies and synchronises a second time.  Nothing of the sampler changes
// before the step's last device call has succeeded.
struct RumiKfd {
    RumiOrb *h = nullptr;
    int cap = 0;                                  // tracked points at most: the extractor's capSel
    FlowGeom g{};                                 // of the frames since the last first step
    int frameCap = 0, derivCap = 0;               // bytes / elements of a slot, for the extractor's largest frame
    uint8_t *dFrames[2] = {nullptr, nullptr};
    uint32_t *dDeriv[2] = {nullptr, nullptr};
    MirrorBuf<uint8_t> bgr;                       // a BGR frame on its way to level 0 (allocated with the first one)
    float *hOld = nullptr, *dOld = nullptr;       // the tracked points, pinned and on the device
    uint8_t *hOut = nullptr, *dOut = nullptr;     // [next n x 2 float | status n]
    int prevSlot = 0, nOld = 0;
    double ltframe = 0;
    // pd.hpp: PD(Kp, Kd) leaves Alpha 1 and maxOutput 255
    float kp = 0.8f, kd = 0.005f, setpoint = 10.f, prevInput = 0.f, maxOutput = 255.f, alpha = 1.f;
};

extern "C" void rumi_kfd_destroy(RumiKfd *s) {
    if (!s) return;
    if (s->h) { (void)hipSetDevice(s->h->device); (void)hipStreamSynchronize(nullptr); }
    for (void *p : {(void *)s->dFrames[0], (void *)s->dFrames[1], (void *)s->dDeriv[0], (void *)s->dDeriv[1], (void *)s->dOld, (void *)s->dOut}) if (p) (void)hipFree(p);
    for (void *p : {(void *)s->hOld, (void *)s->hOut}) if (p) (void)hipHostFree(p);
    delete s;
}

extern "C" int rumi_kfd_create(RumiOrb *h, RumiKfd **out) {
    if (!out) return RUMI_E_INVALID;
    *out = nullptr;
    if (!h) return RUMI_E_INVALID;
    if (h->cfg.max_width < kFlowMinSide || h->cfg.max_height < kFlowMinSide) { g_lastError = "rumi_kfd_create: the extractor's frames must be at least 128 x 128"; return RUMI_E_INVALID; }
    HIP_TRY(hipSetDevice(h->device));
    RumiKfd *s = new RumiKfd();
    s->h = h; s->cap = h->capSel;
    const FlowGeom g = flow_geometry(h->cfg.max_width, h->cfg.max_height);
    s->frameCap = g.frameBytes; s->derivCap = g.derivElems;           // (every term of flow_geometry grows with the frame: a smaller frame fits)
    int rc = RUMI_OK;
    const size_t cap = (size_t)s->cap;
    if ((rc = dev_alloc(&s->dFrames[0], (size_t)s->frameCap)) != RUMI_OK || (rc = dev_alloc(&s->dFrames[1], (size_t)s->frameCap)) != RUMI_OK ||
        (rc = dev_alloc(&s->dDeriv[0], (size_t)s->derivCap)) != RUMI_OK || (rc = dev_alloc(&s->dDeriv[1], (size_t)s->derivCap)) != RUMI_OK ||
        (rc = dev_alloc(&s->dOld, cap * 2)) != RUMI_OK || (rc = dev_alloc(&s->dOut, cap * 9)) != RUMI_OK ||
        (rc = pin_alloc(&s->hOld, cap * 2)) != RUMI_OK || (rc = pin_alloc(&s->hOut, cap * 9)) != RUMI_OK) { rumi_kfd_destroy(s); return rc; }
    *out = s;
    return RUMI_OK;
}

extern "C" int rumi_kfd_set_pd(RumiKfd *s, float kp, float kd, float th) {
    if (!s) return RUMI_E_INVALID;
    s->kp = kp; s->kd = kd; s->setpoint = th;
    return RUMI_OK;
}

extern "C" int rumi_kfd_reset(RumiKfd *s) {
    if (!s) return RUMI_E_INVALID;
    s->nOld = 0;
    return RUMI_OK;
}

extern "C" int rumi_kfd_step(RumiKfd *s, const uint8_t *img, int32_t w, int32_t hgt, int32_t stride, int32_t channels, double timestamp, RumiKfdStep *out) {
    if (out) { std::memset(out, 0, sizeof *out); out->mono = -1; }
    if (!s || !out) return RUMI_E_INVALID;
    RumiOrb *h = s->h;
    if (!img || w <= 0 || hgt <= 0) return RUMI_E_EMPTY;
    if (channels != 1 && channels != 3) { g_lastError = "rumi_kfd_step: 1 (grey) or 3 (BGR) channels"; return RUMI_E_INVALID; }
    if (w < kFlowMinSide || hgt < kFlowMinSide || w > h->cfg.max_width || hgt > h->cfg.max_height || stride < w * channels) {
        g_lastError = "rumi_kfd_step: frames of at least 128 x 128 and at most the extractor's size"; return RUMI_E_INVALID;
    }
    const bool first = s->nOld == 0;
    if (!first && (w != s->g.w[0] || hgt != s->g.h[0])) { g_lastError = "rumi_kfd_step: the frame size changed between two tracked frames (rumi_kfd_reset first)"; return RUMI_E_INVALID; }
    HIP_TRY(hipSetDevice(h->device));
    if (h->pending) { const int rc = rumi_orb_sync(h); if (rc != RUMI_OK) return rc; }
    const FlowGeom g = flow_geometry(w, hgt);
    if (g.frameBytes > s->frameCap || g.derivElems > s->derivCap) { g_lastError = "rumi_kfd_step: frame slot too small"; return RUMI_E_CAPACITY; }
    const int cur = s->prevSlot ^ 1, wp = g.pitch[0];
    uint8_t *frame = s->dFrames[cur];
    // the frame crosses once: grey straight into level 0, BGR beside it and through k_flow_grey
    if (channels == 1) {
        stage_host_frame(h, img, w, hgt, stride, wp);
        HIP_TRY(hipMemcpyAsync(frame + g.off[0], h->hIn, (size_t)wp * hgt, hipMemcpyHostToDevice, nullptr));
    } else {
        const size_t row = (size_t)w * 3, bytes = row * hgt;
        const size_t most = (size_t)h->cfg.max_width * 3 * h->cfg.max_height;
        if (int rc = s->bgr.reserve(most, most); rc != RUMI_OK) return rc;
        for (int y = 0; y < hgt; y++) std::memcpy(s->bgr.h + (size_t)y * row, img + (size_t)y * stride, row);
        HIP_TRY(hipMemcpyAsync(s->bgr.d, s->bgr.h, bytes, hipMemcpyHostToDevice, nullptr));
        flow_launch_grey(s->bgr.d, (int)row, frame, g, nullptr);
    }
    flow_launch_prepare(frame, s->dDeriv[cur], g, nullptr);

    const int n = s->nOld;
    float prevInput = s->prevInput;
    bool selected = true;
    if (!first) {
        HIP_TRY(hipMemcpyAsync(s->dOld, s->hOld, (size_t)n * 8, hipMemcpyHostToDevice, nullptr));
        flow_launch_track(s->dFrames[s->prevSlot], s->dDeriv[s->prevSlot], frame, s->g, s->dOld, n, reinterpret_cast<float *>(s->dOut), s->dOut + (size_t)n * 8, nullptr);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(s->hOut, s->dOut, (size_t)n * 9, hipMemcpyDeviceToHost, nullptr));
        HIP_TRY(hipStreamSynchronize(nullptr));
        const float *next = reinterpret_cast<const float *>(s->hOut);
        const uint8_t *status = s->hOut + (size_t)n * 8;
        // Calmoptflmag over SelectGoodPts' points, in index order
        float sum = 0;
        int good = 0;
        for (int i = 0; i < n; i++)
            if (status[i] == 1) {
                const float dx = next[2 * i] - s->hOld[2 * i], dy = next[2 * i + 1] - s->hOld[2 * i + 1];
                sum += std::sqrt(dx * dx + dy * dy);
                good++;
            }
        const float moptf = sum / good;                                   // 0 / 0 = NaN without a good point
        // PD::update(moptf, timestamp - ltframe), pd.hpp:21-39
        const double Ts = timestamp - s->ltframe;
        float error = s->setpoint - moptf;
        float diff = s->alpha * (prevInput - moptf);
        prevInput -= diff;
        float output = s->kp * error + s->kd / Ts * diff;
        if (output > s->maxOutput) output = s->maxOutput;
        const float TH = moptf + output;
        selected = moptf > TH;
        out->n_tracked = n; out->n_good = good; out->moptf = moptf; out->pd_out = output; out->th = TH;
        out->next = next; out->status = status;
    }
    int nNew = 0;
    if (selected) {
        const int rc = extract_one_to_pinned(h, frame + g.off[0], w, hgt, wp, 0, 0, false);        // (vLapping = {0, 0}, KFDSample.h:53)
        if (rc != RUMI_OK) { std::memset(out, 0, sizeof *out); out->mono = -1; return rc; }
        const int32_t *counts = reinterpret_cast<const int32_t *>(h->hOut1);
        nNew = counts[0];
        out->n = nNew; out->mono = counts[1];
        out->kp = reinterpret_cast<const RumiKeyPoint *>(h->hOut1 + 16);
        out->desc = h->hOut1 + 16 + (size_t)h->capSel * sizeof(RumiKeyPoint);
    }
    // the step has succeeded: commit
    if (selected) {
        for (int i = 0; i < nNew; i++) { s->hOld[2 * i] = out->kp[i].x; s->hOld[2 * i + 1] = out->kp[i].y; }     // KeyPoint::convert
        s->nOld = nNew;
    } else std::memcpy(s->hOld, s->hOut, (size_t)n * 8);                  // old = next: every point, the failed ones included
    out->selected = selected ? 1 : 0;
    s->prevInput = prevInput;
    s->ltframe = timestamp;
    s->prevSlot = cur;
    s->g = g;
    return RUMI_OK;
}
