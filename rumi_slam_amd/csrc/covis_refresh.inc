// What rumi_refresh_map_points_resident (refresh.hip, refresh_resident.inc) needs of the covisibility store beyond what the other members keep
// there (include/rumi_covis.h; part of covis.hip): the camera centre of a slot and the reference key-frame of a point, both tables of their
// own that exist from their first edit on; the store's side of that entry (the checks on the mirror, the flush, the mirror's half of the
// write-back); and the read-back hook of the write-back tests.

extern "C" int rumi_covis_set_keyframe_centres(RumiCovis *h, int32_t n, const int32_t *slots, const float *Ow) {
    if (!h || n < 0 || (n > 0 && (!slots || !Ow))) {
        g_lastError = "rumi_covis_set_keyframe_centres: missing argument or negative count";
        return RUMI_E_INVALID;
    }
    if (n == 0) return RUMI_OK;
    if (h->stampKf > INT32_MAX - 4) { std::fill(h->kfStamp.begin(), h->kfStamp.end(), 0); h->stampKf = 0; }
    const int32_t inCall = ++h->stampKf;
    for (int i = 0; i < n; i++) {
        if (!is_live(h, slots[i]) || h->kfStamp[slots[i]] == inCall) {
            g_lastError = "rumi_covis_set_keyframe_centres: a slot that is not live, or named twice";
            return RUMI_E_INVALID;
        }
        h->kfStamp[slots[i]] = inCall;
        for (int j = 0; j < 3; j++) {
            uint32_t bits;
            std::memcpy(&bits, Ow + (size_t)i * 3 + j, 4);
            if ((bits & 0x7F800000u) == 0x7F800000u) {               // infinity or NaN
                g_lastError = "rumi_covis_set_keyframe_centres: a camera centre that is not finite";
                return RUMI_E_INVALID;
            }
        }
    }
    if (h->centre.empty()) h->centre.assign((size_t)h->maxKf * CTW, 0);
    for (int i = 0; i < n; i++) {
        int32_t *Cw = h->centre.data() + (size_t)slots[i] * CTW;
        std::memcpy(Cw, Ow + (size_t)i * 3, 12);
        Cw[3] = 1;
        note(h, T_CENTRE, (int64_t)slots[i] * CTW, CTW);
    }
    return RUMI_OK;
}

extern "C" int rumi_covis_set_point_reference(RumiCovis *h, int32_t n, const int32_t *ids, const int32_t *ref_slots) {
    if (!h || n < 0 || (n > 0 && (!ids || !ref_slots))) {
        g_lastError = "rumi_covis_set_point_reference: missing argument or negative count";
        return RUMI_E_INVALID;
    }
    if (n == 0) return RUMI_OK;
    if (h->stampPt > INT32_MAX - 4) { std::fill(h->ptStamp.begin(), h->ptStamp.end(), 0); h->stampPt = 0; }
    const int32_t inCall = ++h->stampPt;
    for (int i = 0; i < n; i++) {
        if (ids[i] < 0 || ids[i] >= h->maxPts || h->ptStamp[ids[i]] == inCall) {
            g_lastError = "rumi_covis_set_point_reference: a point id outside 0..max_points-1, or named twice";
            return RUMI_E_INVALID;
        }
        h->ptStamp[ids[i]] = inCall;
        if (ref_slots[i] != -1 && !is_live(h, ref_slots[i])) {
            g_lastError = "rumi_covis_set_point_reference: a reference that is neither -1 nor a live slot";
            return RUMI_E_INVALID;
        }
    }
    if (h->ref.empty()) h->ref.assign((size_t)h->maxPts, 0);
    for (int i = 0; i < n; i++) {
        h->ref[ids[i]] = ref_slots[i] + 1;
        h->hiRef = std::max(h->hiRef, ids[i] + 1);
        note(h, T_REF, ids[i], 1);
    }
    return RUMI_OK;
}

int rumi::covis_refresh_check(RumiCovis *h, int n, const int32_t *ids, bool needAttr, const char *entry, int32_t *rowLen) {
    if (h->stampPt > INT32_MAX - 4) { std::fill(h->ptStamp.begin(), h->ptStamp.end(), 0); h->stampPt = 0; }
    const int32_t inCall = ++h->stampPt;
    for (int i = 0; i < n; i++) {
        if (ids[i] < 0 || ids[i] >= h->maxPts || h->ptStamp[ids[i]] == inCall) {
            g_lastError = std::string(entry) + ": a point id outside 0..max_points-1, or named twice";
            return RUMI_E_INVALID;
        }
        h->ptStamp[ids[i]] = inCall;
    }
    int without = 0, noAttr = 0;
    for (int i = 0; i < n; i++) {
        const int32_t *P = h->pt.data() + (size_t)ids[i] * PTW;
        rowLen[i] = P[1];
        without += P[1] > 0 && !(P[2] & kCovisPointHasObsFeatures);
        noAttr += needAttr && !P[3];
    }
    if (without > 0) {
        g_lastError = std::string(entry) + ": " + std::to_string(without) + " points have observers but no observation features (rumi_covis_set_point_observations)";
        return RUMI_E_INVALID;
    }
    if (noAttr > 0) {
        g_lastError = std::string(entry) + ": " + std::to_string(noAttr) + " points have no attributes (rumi_covis_set_point_attributes): the position is read there, and the write-back goes there";
        return RUMI_E_INVALID;
    }
    return RUMI_OK;
}

void rumi::covis_refresh_write_mirror(RumiCovis *h, int n, const int32_t *ids, const int32_t *rowLen, const CovisRefreshOut *out, bool desc, bool normal) {
    for (int i = 0; i < n; i++) {
        if (rowLen[i] == 0) continue;
        int32_t *A = h->attr.data() + (size_t)ids[i] * ATW;
        if (desc && out[i].bestObs >= 0) std::memcpy(A + 8, out[i].desc, 32);
        if (normal && out[i].updated) { std::memcpy(A + 3, out[i].normal, 12); std::memcpy(A + 6, &out[i].minD, 4); std::memcpy(A + 7, &out[i].maxD, 4); }
    }
}

extern "C" int rumi_hook_covis_read_attributes(RumiCovis *h, int32_t n, const int32_t *ids, uint8_t *out, int32_t from_device) {
    if (!h || n < 0 || (n > 0 && (!ids || !out))) { g_lastError = "rumi_hook_covis_read_attributes: missing argument or negative count"; return RUMI_E_INVALID; }
    for (int i = 0; i < n; i++)
        if (ids[i] < 0 || ids[i] >= h->maxPts) { g_lastError = "rumi_hook_covis_read_attributes: a point id outside 0..max_points-1"; return RUMI_E_INVALID; }
    if (from_device ? !h->dAttr.p : h->attr.empty()) {
        g_lastError = "rumi_hook_covis_read_attributes: the store holds no attribute table there yet";
        return RUMI_E_INVALID;
    }
    if (from_device) {
        HIP_TRY(hipSetDevice(h->dev.device));
        HIP_TRY(hipDeviceSynchronize());
    }
    for (int i = 0; i < n; i++) {
        if (from_device) HIP_TRY(hipMemcpy(out + (size_t)i * 64, h->dAttr.p + (size_t)ids[i] * ATW, 64, hipMemcpyDeviceToHost));
        else std::memcpy(out + (size_t)i * 64, h->attr.data() + (size_t)ids[i] * ATW, 64);
    }
    return RUMI_OK;
}

extern "C" int rumi_hook_covis_read_row(RumiCovis *h, int32_t slot, int32_t cap, int32_t *row, uint8_t *point_bad, int32_t *kf_bad) {
    if (!h || cap < 0 || !row || !point_bad || !kf_bad) { g_lastError = "rumi_hook_covis_read_row: missing argument or negative cap"; return RUMI_E_INVALID; }
    if (!is_live(h, slot)) { g_lastError = "rumi_hook_covis_read_row: a slot that is not live"; return RUMI_E_INVALID; }
    const int32_t *K = h->kf.data() + (size_t)slot * KFW;
    if (K[K_MPLEN] > cap) { g_lastError = "rumi_hook_covis_read_row: the row is longer than cap"; return RUMI_E_CAPACITY; }
    for (int i = 0; i < K[K_MPLEN]; i++) {
        const int32_t p = h->arena[(size_t)K[K_MPOFF] + i];
        row[i] = p;
        point_bad[i] = p >= 0 ? (uint8_t)(h->pt[(size_t)p * PTW + 2] & 1) : 0;
    }
    *kf_bad = K[K_FLAGS] & 1;
    return RUMI_OK;
}
