// What rumi_local_ba_resident (opt.hip, ba_resident.inc, ba_resident_host.inc) needs of the covisibility store beyond what the other members
// keep there (include/rumi_covis.h; part of covis.hip): the pose of a slot as the bundle adjustment reads it and the map of a point, both
// tables of their own that exist from their first edit on; and the store's side of that entry (the window from the mirror, the mirror's half
// of the position write-back).

extern "C" int rumi_covis_set_keyframe_poses(RumiCovis *h, int32_t n, const int32_t *slots, const float *pose7) {
    if (!h || n < 0 || (n > 0 && (!slots || !pose7))) {
        g_lastError = "rumi_covis_set_keyframe_poses: missing argument or negative count";
        return RUMI_E_INVALID;
    }
    if (n == 0) return RUMI_OK;
    if (h->stampKf > INT32_MAX - 4) { std::fill(h->kfStamp.begin(), h->kfStamp.end(), 0); h->stampKf = 0; }
    const int32_t inCall = ++h->stampKf;
    for (int i = 0; i < n; i++) {
        if (!is_live(h, slots[i]) || h->kfStamp[slots[i]] == inCall) {
            g_lastError = "rumi_covis_set_keyframe_poses: a slot that is not live, or named twice";
            return RUMI_E_INVALID;
        }
        h->kfStamp[slots[i]] = inCall;
        for (int j = 0; j < 7; j++) {
            uint32_t bits;
            std::memcpy(&bits, pose7 + (size_t)i * 7 + j, 4);
            if ((bits & 0x7F800000u) == 0x7F800000u) {               // infinity or NaN
                g_lastError = "rumi_covis_set_keyframe_poses: a pose that is not finite";
                return RUMI_E_INVALID;
            }
        }
    }
    if (h->pose.empty()) { h->pose.assign((size_t)h->maxKf * PSW, 0); h->pose7.assign((size_t)h->maxKf * 7, 0.f); }
    for (int i = 0; i < n; i++) {
        const int32_t s = slots[i];
        // what ba_stage_poses (ba_host_shared.inc) makes of the seven floats, by the same function
        const DSE3 P = se3_from_float7(pose7 + (size_t)i * 7);
        const double t[8] = {P.r.x, P.r.y, P.r.z, P.r.w, P.t.x, P.t.y, P.t.z, 0};
        std::memcpy(h->pose.data() + (size_t)s * PSW, t, sizeof t);
        std::memcpy(h->pose7.data() + (size_t)s * 7, pose7 + (size_t)i * 7, 28);
        note(h, T_POSE, (int64_t)s * PSW, PSW);
        int32_t &has = h->kf[(size_t)s * KFW + kCovisKfHasPose];
        if (!has) { has = 1; note(h, T_KF, (int64_t)s * KFW + kCovisKfHasPose, 1); }
    }
    return RUMI_OK;
}

extern "C" int rumi_covis_set_point_maps(RumiCovis *h, int32_t n, const int32_t *ids, const int32_t *map_ids) {
    if (!h || n < 0 || (n > 0 && (!ids || !map_ids))) {
        g_lastError = "rumi_covis_set_point_maps: missing argument or negative count";
        return RUMI_E_INVALID;
    }
    if (n == 0) return RUMI_OK;
    if (h->stampPt > INT32_MAX - 4) { std::fill(h->ptStamp.begin(), h->ptStamp.end(), 0); h->stampPt = 0; }
    const int32_t inCall = ++h->stampPt;
    for (int i = 0; i < n; i++) {
        if (ids[i] < 0 || ids[i] >= h->maxPts || h->ptStamp[ids[i]] == inCall) {
            g_lastError = "rumi_covis_set_point_maps: a point id outside 0..max_points-1, or named twice";
            return RUMI_E_INVALID;
        }
        h->ptStamp[ids[i]] = inCall;
    }
    if (h->ptMap.empty()) h->ptMap.assign((size_t)h->maxPts, 0);
    for (int i = 0; i < n; i++) {
        const int32_t p = ids[i];
        h->ptMap[p] = map_ids[i];
        h->hiMap = std::max(h->hiMap, p + 1);
        note(h, T_PTMAP, p, 1);
        int32_t &f = h->pt[(size_t)p * PTW + 2];
        if (!(f & kCovisPointHasMap)) { f |= kCovisPointHasMap; note(h, T_PT, (int64_t)p * PTW + 2, 1); }
    }
    return RUMI_OK;
}

int rumi::covis_lba_window(RumiCovis *h, int32_t cur, const int32_t *neigh, int32_t nNeigh, int32_t init, const char *entry, int32_t *locals,
                           int32_t *role, CovisLbaWindow *w) {
    const std::string E(entry);
    const FeatureStore &F = h->feat;
    if (!is_live(h, cur) || F.place.empty() || F.place[cur].off < 0) {
        g_lastError = E + ": the current slot is not live or holds no features (rumi_covis_set_keyframe_features)";
        return RUMI_E_INVALID;
    }
    if (init < -1 || init >= h->maxKf) { g_lastError = E + ": init_slot is neither -1 nor a slot"; return RUMI_E_INVALID; }
    if (h->stampKf > INT32_MAX - 4) { std::fill(h->kfStamp.begin(), h->kfStamp.end(), 0); h->stampKf = 0; }
    const int32_t inCall = ++h->stampKf;
    h->kfStamp[cur] = inCall;
    for (int i = 0; i < nNeigh; i++) {
        if (!is_live(h, neigh[i]) || h->kfStamp[neigh[i]] == inCall) {
            g_lastError = E + ": a neighbour that is not a live slot, is the current slot, or is named twice";
            return RUMI_E_INVALID;
        }
        h->kfStamp[neigh[i]] = inCall;
    }
    std::fill(role, role + h->hiSlot, -1);
    const int32_t *KC = h->kf.data() + (size_t)cur * KFW;
    *w = CovisLbaWindow{};
    w->hiSlot = h->hiSlot; w->curMap = KC[K_MAP]; w->initIdx = -1;
    std::memcpy(w->K4, F.place[cur].rec.K, 16);
    int nL = 0;
    auto take = [&](int32_t s) {
        const int32_t *K = h->kf.data() + (size_t)s * KFW;
        if (s == init) w->initIdx = nL;
        role[s] = nL; locals[nL++] = s;
        w->maxRow = std::max(w->maxRow, K[K_MPLEN]); w->sumRows += K[K_MPLEN];
    };
    take(cur);                                                          // Optimizer.cc:1007
    for (int i = 0; i < nNeigh; i++) {                                  // :1012-1017
        const int32_t *K = h->kf.data() + (size_t)neigh[i] * KFW;
        // a neighbour that is bad or of another map is stamped (:1014) but joins no list: the same two tests keep it from being a fixed camera
        if (!(K[K_FLAGS] & 1) && K[K_MAP] == w->curMap) take(neigh[i]);
    }
    w->nLocal = nL;
    return RUMI_OK;
}

void rumi::covis_lba_pose7(const RumiCovis *h, int32_t slot, float *pose7) {
    if (h->pose7.empty() || slot < 0 || slot >= h->maxKf) { std::memset(pose7, 0, 28); return; }
    std::memcpy(pose7, h->pose7.data() + (size_t)slot * 7, 28);
}

void rumi::covis_lba_write_positions(RumiCovis *h, int32_t n, const int32_t *ids, const float *pos3) {
    if (h->attr.empty()) return;
    for (int i = 0; i < n; i++) std::memcpy(h->attr.data() + (size_t)ids[i] * ATW, pos3 + (size_t)i * 3, 12);
}

extern "C" int rumi_hook_covis_read_poses(RumiCovis *h, int32_t n_kf, const int32_t *slots, double *pose8, int32_t *has_pose, int32_t n_pt, const int32_t *ids,
                                          int32_t *map_id, int32_t *has_map, int32_t from_device) {
    if (!h || n_kf < 0 || n_pt < 0 || (n_kf > 0 && (!slots || !pose8 || !has_pose)) || (n_pt > 0 && (!ids || !map_id || !has_map))) {
        g_lastError = "rumi_hook_covis_read_poses: missing argument or negative count";
        return RUMI_E_INVALID;
    }
    for (int i = 0; i < n_kf; i++)
        if (slots[i] < 0 || slots[i] >= h->maxKf) { g_lastError = "rumi_hook_covis_read_poses: a slot outside 0..max_kf-1"; return RUMI_E_INVALID; }
    for (int i = 0; i < n_pt; i++)
        if (ids[i] < 0 || ids[i] >= h->maxPts) { g_lastError = "rumi_hook_covis_read_poses: a point id outside 0..max_points-1"; return RUMI_E_INVALID; }
    if (from_device) {
        if (!h->dev.bound) { g_lastError = "rumi_hook_covis_read_poses: the store has no device yet"; return RUMI_E_INVALID; }
        HIP_TRY(hipSetDevice(h->dev.device));
        HIP_TRY(hipDeviceSynchronize());
    }
    for (int i = 0; i < n_kf; i++) {
        const int32_t s = slots[i];
        std::memset(pose8 + (size_t)i * 8, 0, 64);
        if (from_device) {
            HIP_TRY(hipMemcpy(has_pose + i, h->dKf.p + (size_t)s * KFW + kCovisKfHasPose, 4, hipMemcpyDeviceToHost));
            if (h->dPose.p) HIP_TRY(hipMemcpy(pose8 + (size_t)i * 8, h->dPose.p + (size_t)s * PSW, 64, hipMemcpyDeviceToHost));
        } else {
            has_pose[i] = h->kf[(size_t)s * KFW + kCovisKfHasPose];
            if (!h->pose.empty()) std::memcpy(pose8 + (size_t)i * 8, h->pose.data() + (size_t)s * PSW, 64);
        }
    }
    for (int i = 0; i < n_pt; i++) {
        const int32_t p = ids[i];
        int32_t flags = 0;
        map_id[i] = 0;
        if (from_device) {
            HIP_TRY(hipMemcpy(&flags, h->dPt.p + (size_t)p * PTW + 2, 4, hipMemcpyDeviceToHost));
            if (h->dPtMap.p) HIP_TRY(hipMemcpy(map_id + i, h->dPtMap.p + p, 4, hipMemcpyDeviceToHost));
        } else {
            flags = h->pt[(size_t)p * PTW + 2];
            if (!h->ptMap.empty()) map_id[i] = h->ptMap[p];
        }
        has_map[i] = (flags & kCovisPointHasMap) != 0;
    }
    return RUMI_OK;
}
