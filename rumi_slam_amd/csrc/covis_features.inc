// The key-frame features of the covisibility store (include/rumi_covis.h; part of covis.hip): mvKeysUn, mDescriptors, mvScaleFactors, mFeatVec
// and the intrinsics of every slot, uploaded once and read where they lie by rumi_create_new_map_points_resident (mapping.hip).
//
//   block   CovisFeatRec (64 bytes: sizes, K4, where each array lies behind the record), keys, desc, scale, node ids, offsets, indices; every
//           array 16-byte aligned, padding zeroed.  The record travels with its arrays, so a key-frame is one contiguous copy and a consumer
//           needs one 64-bit block offset per key-frame.
//   arena   one device allocation.  A block goes to the first free block that holds it (first fit; the rest of the free block stays free), else
//           to the tail; when the tail would pass the capacity, the capacity doubles until it fits.  Growth allocates the new arena, copies
//           the old one device to device and releases it: nothing is uploaded twice.  A dropped or replaced block joins the free list, merged
//           with free neighbours; a free block at the tail pulls the tail back.  Offsets are 64-bit.
//   octaves a device-only byte table [max_kf][stride] of keys[i].octave, for the consumer that reads one octave per observation it meets
//           (rumi_keyframe_culling_resident): the key-points of 140 key-frames of 2000 features are 7.8 MB, their octaves 280 KB, and that
//           consumer's walks are latency-bound.  Filled from the arena by k_covis_octaves when that consumer flushes, for the slots whose
//           features changed since; the stride is the power of two that holds the longest key-frame seen (a longer one rebuilds the table).
//   staging rumi_covis_set_keyframe_features validates, places the block (host arithmetic only) and writes it into the staging block; the next
//           consumer sends the staging block with one copy per run of blocks that are neighbours in both places (one key-frame, or any number
//           appended at the tail: one copy).  The staging block is empty afterwards.

namespace {

constexpr int64_t kFeatDefaultCap = 32ll << 20;
constexpr int64_t kFeatLimit = 1ll << 38;              // far above any device; keeps the doubling below 2^63

// Slot `slot0 + blockIdx.y` of the octave table, from its key-points where they lie.  One slot (slot0 = the slot, gridDim.y = 1) or every slot
// below gridDim.y; a slot without features is left alone.
__global__ __launch_bounds__(256) void k_covis_octaves(CovisView v, uint8_t *oct, int slot0) {
    const int s = slot0 + (int)blockIdx.y, i = (int)blockIdx.x * 256 + (int)threadIdx.x;
    const long long keys = v.feat_keys(s);
    if (keys < 0 || i >= v.feat_count(s) || i >= v.octStride) return;
    oct[(size_t)s * v.octStride + i] = (uint8_t)v.keys_at(keys)[i].octave;
}

// Brings the octave table up to date with the arena and featTab on the device (both flushed before): the pending slots one launch each,
// or every slot in one launch when there are many or the table is new.
int oct_flush(RumiCovis *h) {
    FeatureStore &F = h->feat;
    int stride = 256;
    while (stride < F.maxN) stride *= 2;
    bool all = F.octPending.size() > 8;
    if (!F.oct.p || stride > F.octStride) {
        const size_t bytes = (size_t)h->maxKf * stride;
        const int rc = F.oct.reserve(bytes, bytes);
        if (rc != RUMI_OK) return rc;
        F.octStride = stride;
        all = true;
    }
    if (F.arena.p && h->hiSlot > 0) {
        const int gx = (F.octStride + 255) / 256;
        CovisView v;
        fill_view(h, &v);
        if (all) hipLaunchKernelGGL(k_covis_octaves, dim3(gx, h->hiSlot), dim3(256), 0, nullptr, v, F.oct.p, 0);
        else
            for (int32_t s : F.octPending)
                hipLaunchKernelGGL(k_covis_octaves, dim3(gx, 1), dim3(256), 0, nullptr, v, F.oct.p, s);
        HIP_TRY(hipGetLastError());
    }
    F.octPending.clear();
    return RUMI_OK;
}

// The record of a validated key-frame; false when the block would pass 2 GiB (the record's 32-bit offsets), or if the key-points did not
// follow the record at once (kCovisFeatKeysOffset, covis_view.h).
bool feat_layout(const RumiFrameFeatures &f, const RumiFeatureVector &v, const float *K4, CovisFeatRec *r) {
    const uint64_t n = (uint64_t)f.n, nn = (uint64_t)v.n_nodes, ne = nn ? (uint64_t)v.offsets[nn] : 0;
    uint64_t at = sizeof(CovisFeatRec);                // the key-points follow the record at once: refresh_resident.inc finds the record from featTab's offset
    auto put = [&](uint64_t bytes) { const uint64_t o = at; at = up16(at + bytes); return o; };
    const uint64_t keys = put(n * sizeof(RumiKeyPoint)), desc = put(n * 32), scale = put((uint64_t)f.nlevels * 4), nodes = put(nn * 4),
                   off = put((nn + 1) * 4), idx = put(ne * 4);
    if (at >= (1ull << 31) || keys != kCovisFeatKeysOffset) return false;
    r->n = (int32_t)n; r->nn = (int32_t)nn; r->ne = (int32_t)ne; r->nlevels = f.nlevels;
    std::memcpy(r->K, K4, 16);
    r->keys = (uint32_t)keys; r->desc = (uint32_t)desc; r->scale = (uint32_t)scale; r->nodes = (uint32_t)nodes; r->off = (uint32_t)off; r->idx = (uint32_t)idx;
    r->bytes = (uint32_t)at; r->pad = 0;
    return true;
}

void feat_free(FeatureStore &F, int64_t off, int64_t bytes) {
    auto it = std::lower_bound(F.freeList.begin(), F.freeList.end(), std::make_pair(off, (int64_t)0));
    it = F.freeList.insert(it, {off, bytes});
    if (it + 1 != F.freeList.end() && it->first + it->second == (it + 1)->first) { it->second += (it + 1)->second; F.freeList.erase(it + 1); }
    if (it != F.freeList.begin() && (it - 1)->first + (it - 1)->second == it->first) { (it - 1)->second += it->second; it = F.freeList.erase(it) - 1; }
    if (it->first + it->second == F.tail) { F.tail = it->first; F.freeList.erase(it); }
}

int64_t feat_alloc(FeatureStore &F, int64_t bytes) {
    for (auto it = F.freeList.begin(); it != F.freeList.end(); ++it)
        if (it->second >= bytes) {
            const int64_t off = it->first;
            if (it->second == bytes) F.freeList.erase(it); else { it->first += bytes; it->second -= bytes; }
            return off;
        }
    if (F.cap == 0) F.cap = F.firstCap ? F.firstCap : kFeatDefaultCap;
    if (F.tail + bytes > F.cap) {
        while (F.tail + bytes > F.cap) F.cap *= 2;
        F.growths++;
    }
    const int64_t off = F.tail;
    F.tail += bytes;
    return off;
}

// Room for `need` bytes in the staging block, what it holds kept.  Pinned once the store has a device (a set_ call on a machine without one
// must still succeed, so that refusals can be tested there); feat_flush re-houses an unpinned block.
int feat_stage_reserve(RumiCovis *h, size_t need, bool pinned) {
    FeatureStore &F = h->feat;
    if (need <= F.stageCap && (F.stagePinned || !pinned)) return RUMI_OK;
    const size_t cap = std::max(need + need / 2, (size_t)1 << 20);
    uint8_t *p = nullptr;
    if (pinned) {
        HIP_TRY(hipSetDevice(h->dev.device));
        const int rc = pin_alloc(&p, cap);
        if (rc != RUMI_OK) return rc;
    } else if (!(p = static_cast<uint8_t *>(std::malloc(cap)))) {
        g_lastError = "rumi_covis_set_keyframe_features: out of host memory for the staging block";
        return RUMI_E_CAPACITY;
    }
    if (F.stageUsed) std::memcpy(p, F.stage, F.stageUsed);
    F.release_stage();
    F.stage = p; F.stageCap = cap; F.stagePinned = pinned;
    return RUMI_OK;
}

// The slot's record of featTab follows its place in the arena.
void feat_tab_set(RumiCovis *h, int32_t slot) {
    const FeatPlace &P = h->feat.place[slot];
    const int64_t keys = P.off < 0 ? -1 : P.off + (int64_t)P.rec.keys;
    int32_t *T = h->featTab.data() + (size_t)slot * FTW;
    std::memcpy(T, &keys, 8);
    T[2] = P.off < 0 ? 0 : P.rec.n;
    note(h, T_FEAT, (int64_t)slot * FTW, FTW);
}

void feat_remove(FeatureStore &F, int32_t slot) {
    FeatPlace &P = F.place[slot];
    if (P.off < 0) return;
    feat_free(F, P.off, P.rec.bytes);
    F.used -= P.rec.bytes; F.slots--;
    P = FeatPlace{};
}

// Grows the device arena to the capacity the placements assume (device to device), then sends what is staged.
int feat_flush(RumiCovis *h) {
    FeatureStore &F = h->feat;
    F.lastUpload = 0;
    if (F.cap > 0 && (int64_t)F.arena.cap < F.cap) {
        DevBuf<uint8_t> grown;
        const int rc = grown.reserve((size_t)F.cap, (size_t)F.cap);
        if (rc != RUMI_OK) return rc;
        if (F.arena.p && F.onDevice > 0) HIP_TRY(hipMemcpyAsync(grown.p, F.arena.p, (size_t)F.onDevice, hipMemcpyDeviceToDevice, nullptr));
        std::swap(grown.p, F.arena.p); std::swap(grown.cap, F.arena.cap);        // `grown` releases the old arena; hipFree waits for the copy
    }
    if (!F.staged.empty() && !F.stagePinned) {
        const int rc = feat_stage_reserve(h, F.stageUsed, true);
        if (rc != RUMI_OK) return rc;
    }
    int64_t src = -1, dst = -1, len = 0;                                         // the run being collected
    auto send = [&]() -> hipError_t {
        const hipError_t e = len ? hipMemcpyAsync(F.arena.p + dst, F.stage + src, (size_t)len, hipMemcpyHostToDevice, nullptr) : hipSuccess;
        F.lastUpload += len; len = 0;
        return e;
    };
    for (const auto &st : F.staged) {
        FeatPlace &P = F.place[st.first];
        if (P.off < 0 || P.stageOff != st.second) continue;                      // dropped or replaced since
        if (len && (src + len != P.stageOff || dst + len != P.off)) HIP_TRY(send());
        if (!len) { src = P.stageOff; dst = P.off; }
        len += P.rec.bytes;
        P.stageOff = -1;
    }
    HIP_TRY(send());
    F.staged.clear(); F.stageUsed = 0;
    F.onDevice = F.tail;
    return RUMI_OK;
}

}  // namespace

extern "C" int rumi_covis_reserve_features(RumiCovis *h, int64_t bytes) {
    if (!h || bytes < 0 || bytes > kFeatLimit) { g_lastError = "rumi_covis_reserve_features: missing handle, or a size outside 0..2^38"; return RUMI_E_INVALID; }
    if (h->feat.cap != 0) { g_lastError = "rumi_covis_reserve_features: the feature arena is in use; its first size is set before the first key-frame"; return RUMI_E_INVALID; }
    h->feat.firstCap = bytes ? (int64_t)up16((size_t)std::max<int64_t>(bytes, 4096)) : 0;
    return RUMI_OK;
}

extern "C" int rumi_covis_set_keyframe_features(RumiCovis *h, int32_t slot, const RumiFrameFeatures *feat, const RumiFeatureVector *fv, const float *K4) {
    if (!h || !feat || !fv || !K4) { g_lastError = "rumi_covis_set_keyframe_features: missing argument"; return RUMI_E_INVALID; }
    if (!is_live(h, slot)) { g_lastError = "rumi_covis_set_keyframe_features: a slot that is not live"; return RUMI_E_INVALID; }
    if (feat->n > RUMI_COVIS_MAX_FEATURES) {                                     // before any array is read
        g_lastError = "rumi_covis_set_keyframe_features: more than RUMI_COVIS_MAX_FEATURES features";
        return RUMI_E_CAPACITY;
    }
    const char *why = "";
    if (!keyframe_features_valid(*feat, *fv, &why)) { g_lastError = why; return RUMI_E_INVALID; }
    FeatureStore &F = h->feat;
    CovisFeatRec rec;
    if (!feat_layout(*feat, *fv, K4, &rec) || F.tail + (int64_t)rec.bytes > kFeatLimit) {
        g_lastError = "rumi_covis_set_keyframe_features: the key-frame's block or the feature arena would pass its size limit";
        return RUMI_E_CAPACITY;
    }
    const int rc = feat_stage_reserve(h, F.stageUsed + rec.bytes, h->dev.bound);
    if (rc != RUMI_OK) return rc;
    // ---- nothing refuses from here on
    if (F.place.empty()) F.place.resize((size_t)h->maxKf);
    feat_remove(F, slot);
    FeatPlace &P = F.place[slot];
    P.rec = rec;
    P.off = feat_alloc(F, rec.bytes);
    P.stageOff = (int64_t)F.stageUsed;
    F.used += rec.bytes; F.slots++;
    uint8_t *b = F.stage + F.stageUsed;
    std::memset(b, 0, rec.bytes);
    std::memcpy(b, &rec, sizeof rec);
    const size_t n = (size_t)rec.n, nn = (size_t)rec.nn;
    if (n) { std::memcpy(b + rec.keys, feat->keys_un, n * sizeof(RumiKeyPoint)); std::memcpy(b + rec.desc, feat->desc, n * 32); }
    std::memcpy(b + rec.scale, feat->scale_factors, (size_t)rec.nlevels * 4);
    if (nn) {
        std::memcpy(b + rec.nodes, fv->node_ids, nn * 4); std::memcpy(b + rec.off, fv->offsets, (nn + 1) * 4);
        if (rec.ne) std::memcpy(b + rec.idx, fv->indices, (size_t)rec.ne * 4);
    }
    F.staged.push_back({slot, P.stageOff});
    F.stageUsed += rec.bytes;
    F.maxN = std::max(F.maxN, rec.n);
    F.octPending.push_back(slot);
    feat_tab_set(h, slot);
    return RUMI_OK;
}

extern "C" int rumi_covis_drop_keyframe_features(RumiCovis *h, int32_t n, const int32_t *slots) {
    if (!h || n < 0 || (n > 0 && !slots)) { g_lastError = "rumi_covis_drop_keyframe_features: missing argument or negative count"; return RUMI_E_INVALID; }
    for (int i = 0; i < n; i++)
        if (slots[i] < 0 || slots[i] >= h->maxKf) { g_lastError = "rumi_covis_drop_keyframe_features: a slot outside 0..max_kf-1"; return RUMI_E_INVALID; }
    if (!h->feat.place.empty())
        for (int i = 0; i < n; i++) { feat_remove(h->feat, slots[i]); feat_tab_set(h, slots[i]); }
    return RUMI_OK;
}

extern "C" int32_t rumi_covis_row_length(const RumiCovis *h, int32_t slot) {
    return h && is_live(h, slot) ? h->kf[(size_t)slot * KFW + K_MPLEN] : -1;
}

extern "C" int rumi_covis_feature_stats(const RumiCovis *h, int64_t *out6) {
    if (!h || !out6) return RUMI_E_INVALID;
    const FeatureStore &F = h->feat;
    const int64_t v[6] = {F.cap, F.used, F.slots, F.growths, F.compactions, F.lastUpload};
    std::memcpy(out6, v, sizeof v);
    return RUMI_OK;
}

int rumi::covis_same_device(RumiCovis *h, int wantDevice, const char *entry) {
    if (wantDevice < 0) return RUMI_OK;
    if (!h->dev.bound && h->dev.device < 0) h->dev.device = wantDevice;
    if (h->dev.device != wantDevice) { g_lastError = std::string(entry) + ": the store and the handle that reads it are on different devices"; return RUMI_E_INVALID; }
    return RUMI_OK;
}

int rumi::covis_features_check(RumiCovis *h, int n, const int32_t *slots, const char *entry, CovisSlotFeatures *info) {
    const FeatureStore &F = h->feat;
    if (h->stampKf > INT32_MAX - 4) { std::fill(h->kfStamp.begin(), h->kfStamp.end(), 0); h->stampKf = 0; }
    const int32_t inCall = ++h->stampKf;
    for (int i = 0; i < n; i++) {
        const int32_t s = slots[i];
        if (!is_live(h, s) || F.place.empty() || F.place[s].off < 0) {
            g_lastError = std::string(entry) + ": a slot that is not live or holds no features (rumi_covis_set_keyframe_features)";
            return RUMI_E_INVALID;
        }
        if (h->kfStamp[s] == inCall) { g_lastError = std::string(entry) + ": a slot named twice (the current key-frame is not its own neighbour)"; return RUMI_E_INVALID; }
        h->kfStamp[s] = inCall;
        const int32_t *K = h->kf.data() + (size_t)s * KFW;
        if (F.place[s].rec.n != K[K_MPLEN]) {
            g_lastError = std::string(entry) + ": a slot whose feature count differs from the length of its map-point row";
            return RUMI_E_INVALID;
        }
    }
    for (int i = 0; i < n; i++) {                        // rows move when an edit is staged (set_row), never in a query
        const FeatPlace &P = F.place[slots[i]];
        const int32_t *K = h->kf.data() + (size_t)slots[i] * KFW;
        info[i] = CovisSlotFeatures{P.rec.n, P.rec.nn, P.rec.ne, K[K_MPOFF], K[K_MPLEN], P.off};
    }
    return RUMI_OK;
}

int rumi::covis_max_points(const RumiCovis *h) { return h->maxPts; }

int rumi::covis_view(RumiCovis *h, int want, CovisView *view) {
    int rc;
    uint8_t *unused = nullptr;
    if ((rc = flush(h, nullptr, 0, &unused)) != RUMI_OK || (rc = feat_flush(h)) != RUMI_OK) return rc;      // flush binds the store
    if ((want & kCovisWantOctaves) && (rc = oct_flush(h)) != RUMI_OK) return rc;
    fill_view(h, view);
    return RUMI_OK;
}

void rumi::covis_cull_slot(const RumiCovis *h, int32_t slot, CovisCullSlot *out) {
    *out = CovisCullSlot{0, 0, -1, 0, 0};
    if (!is_live(h, slot)) return;
    const int32_t *K = h->kf.data() + (size_t)slot * KFW;
    const FeatureStore &F = h->feat;
    *out = CovisCullSlot{1, K[K_FLAGS] & 1, F.place.empty() || F.place[slot].off < 0 ? -1 : F.place[slot].rec.n, K[K_MPOFF], K[K_MPLEN]};
}

void rumi::covis_cull_row_points(const RumiCovis *h, int32_t mpOff, int32_t mpLen, int32_t *without, int32_t *longest) {
    const int32_t *row = h->arena.data() + mpOff;
    int32_t w = 0, l = 0;
    for (int i = 0; i < mpLen; i++) {
        if (row[i] < 0) continue;
        const int32_t *P = h->pt.data() + (size_t)row[i] * PTW;
        w += !(P[2] & kCovisPointHasObsFeatures);
        l = std::max(l, P[1]);
    }
    *without = w; *longest = l;
}
