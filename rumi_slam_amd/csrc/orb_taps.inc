// The parity taps: intermediate results of the last call for the tests that compare stage by stage (pyramid levels, candidates, selected key-points).
extern "C" int rumi_orb_pyramid_level(RumiOrb *h, int32_t frame, int32_t level, int32_t which, int32_t border,
                                      uint8_t *out, int32_t out_stride, int32_t *w_out, int32_t *h_out) {
    if (!h || h->lastFrames == 0 || frame < 0 || frame >= h->lastFrames || level < 0 || level >= h->hP.nlevels || border < 0)
        return RUMI_E_INVALID;
    if (h->lastResident && (frame < h->lastChunkBase || frame >= h->lastChunkBase + h->lastChunkFrames)) {
        g_lastError = "with a resident queue the arenas keep the pyramid of the call's last sub-chunk only";
        return RUMI_E_INVALID;
    }
    const DevLevel &L = h->hP.lv[level];
    if (w_out) *w_out = L.w;
    if (h_out) *h_out = L.h;
    if (!out) return RUMI_OK;
    if (out_stride < L.w + 2 * border) return RUMI_E_CAPACITY;
    HIP_TRY(hipSetDevice(h->device));
    if (h->pending) { const int rcs = rumi_orb_sync(h); if (rcs != RUMI_OK) return rcs; }
    // no border is stored; the 19-px border copyMakeBorder(..., BORDER_REFLECT_101) gives mvImagePyramid (ORBextractor.cc:1105-1108)
    // is synthesised here from the interior, which is the same pixels by definition
    if (border > (which ? 0 : kEdge)) { g_lastError = which ? "blurred levels carry no border" : "border larger than EDGE_THRESHOLD (19)"; return RUMI_E_INVALID; }
    // level 0 is the caller's frame itself (it must still be alive); the other levels and every blurred level come from the arenas
    const bool own = !which && level == 0;
    const uint8_t *srcp = own ? h->lastSrc.l0 + (long long)frame * h->lastSrc.l0FrameStride
                              : (which ? h->lastSrc.blur : h->lastSrc.pyr) + (long long)frame * h->hP.arenaStride + L.off;
    uint8_t *inner = out + (size_t)border * out_stride + border;
    HIP_TRY(hipMemcpy2D(inner, out_stride, srcp, own ? h->lastSrc.l0Pitch : L.pitch, L.w, L.h, hipMemcpyDeviceToHost));
    auto refl = [](int p, int n) { if (n == 1) return 0; while (p < 0 || p >= n) p = p < 0 ? -p : 2 * n - 2 - p; return p; };
    for (int y = 0; y < L.h; y++) {
        uint8_t *row = inner + (size_t)y * out_stride;
        for (int x = 1; x <= border; x++) { row[-x] = row[refl(-x, L.w)]; row[L.w - 1 + x] = row[refl(L.w - 1 + x, L.w)]; }
    }
    for (int y = 1; y <= border; y++) {
        std::memcpy(inner + (long long)(-y) * out_stride - border, inner + (size_t)refl(-y, L.h) * out_stride - border, (size_t)L.w + 2 * border);
        std::memcpy(inner + (size_t)(L.h - 1 + y) * out_stride - border, inner + (size_t)refl(L.h - 1 + y, L.h) * out_stride - border, (size_t)L.w + 2 * border);
    }
    return RUMI_OK;
}

// Stage taps read the scratch arenas of the LAST chunk (device -> host on first use after a call).
static int fetch_taps(RumiOrb *h) {
    if (h->pending) { const int rc = rumi_orb_sync(h); if (rc != RUMI_OK) return rc; }
    if (h->tapValid) return RUMI_OK;
    const size_t nf = (size_t)h->lastChunkFrames;
    h->tapLevelStart.resize(nf * (kMaxLevels + 1));
    h->tapSelCount.resize(nf);
    h->tapCand.resize(nf * h->capCand);
    h->tapSelPacked.resize(nf * h->capSel);
    h->tapSelMeta.resize(nf * h->capSel);
    const size_t s0 = (size_t)h->lastChunkSlot;
    HIP_TRY(hipMemcpy(h->tapLevelStart.data(), h->dLevelStart + s0 * (kMaxLevels + 1), h->tapLevelStart.size() * 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(h->tapSelCount.data(), h->dSelCount + s0, nf * 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(h->tapCand.data(), h->dCand + s0 * h->capCand, h->tapCand.size() * 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(h->tapSelPacked.data(), h->dSelPacked + s0 * h->capSel, h->tapSelPacked.size() * 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(h->tapSelMeta.data(), h->dSelMeta + s0 * h->capSel, h->tapSelMeta.size() * 4, hipMemcpyDeviceToHost));
    h->tapValid = true;
    return RUMI_OK;
}

extern "C" int rumi_orb_stage_keypoints(RumiOrb *h, int32_t frame, int32_t level, int32_t stage, RumiKeyPoint *out,
                                        int32_t cap, int32_t *n_out) {
    if (!h || !n_out || h->lastFrames == 0 || level < 0 || level >= h->hP.nlevels) return RUMI_E_INVALID;
    const int f = frame - h->lastChunkBase;
    if (f < 0 || f >= h->lastChunkFrames) { g_lastError = "stage taps cover the frames of the last sub-chunk only"; return RUMI_E_INVALID; }
    HIP_TRY(hipSetDevice(h->device));
    int rc = fetch_taps(h);
    if (rc != RUMI_OK) return rc;
    if (stage == 0) {
        const int32_t *ls = h->tapLevelStart.data() + (size_t)f * (kMaxLevels + 1);
        const int n = ls[level + 1] - ls[level];
        *n_out = n;
        if (!out) return RUMI_OK;
        if (n > cap) return RUMI_E_CAPACITY;
        const uint32_t *c = h->tapCand.data() + (size_t)f * h->capCand + ls[level];
        for (int k = 0; k < n; k++)
            out[k] = RumiKeyPoint{(float)cand_x(c[k]), (float)cand_y(c[k]), 7.f, -1.f, (float)cand_score(c[k]), 0, -1};
        return RUMI_OK;
    }
    if (stage == 1) {
        const int tot = h->tapSelCount[f];
        const int ocap = h->lastOutCap;
        int n = 0;
        for (int k = 0; k < tot; k++) {
            const uint32_t meta = h->tapSelMeta[(size_t)f * h->capSel + k], pk = h->tapSelPacked[(size_t)f * h->capSel + k];
            if ((int)(meta & 0xFF) != level) continue;
            const int slot = (int)(meta >> 8);
            RumiKeyPoint kp;
            if (slot >= ocap) return RUMI_E_CAPACITY;
            HIP_TRY(hipMemcpy(&kp, (const uint8_t *)h->lastKp + (size_t)frame * h->lastKpStride + (size_t)slot * sizeof kp, sizeof kp, hipMemcpyDeviceToHost));
            kp.x = (float)(cand_x(pk) + kBorder); kp.y = (float)(cand_y(pk) + kBorder);
            if (out && n < cap) out[n] = kp;
            n++;
        }
        *n_out = n;
        return (out && n > cap) ? RUMI_E_CAPACITY : RUMI_OK;
    }
    return RUMI_E_INVALID;
}
