// rumi_refresh_map_points_resident (include/rumi_mapping.h; part of refresh.hip): the two members over the covisibility store.  Nothing of the
// map travels: the ids and the bin lists go up, a 64-byte record a point comes back.
//
// The host reads O(1) words a point from the store's mirror (the observer-row length L, the flags) and bins the points by L, an upper bound of
// the rows left once bad observers are dropped.  One kernel a bin does both members for its points:
//   L  1..16 / 17..32 / 33..64   k_refresh_res_group<G>   a group of G lanes a point, an observer a lane
//   L 65..                       k_refresh_res_block      a workgroup a point, the observers strided over its 256 lanes
// A lane reads its observer word (slot | feature << 13) from the row arena where the row lies.
//   reference   the lane whose slot is the point's reference slot gives ref_feature (0 when no lane is, MapPoint.cc:495); the point's lane
//               reads the octave of that feature and the two scale factors from the reference slot's resident features
//   normal      the lane forms (Pos - Ow) / |Pos - Ow| of its observer into LDS -- the square roots and divisions of a row run side by side --
//               and the point's lane adds the components in list order: per element the operations of k_refresh_normal, so the same bytes
//   descriptor  the lane tests the slot's bad bit and fetches its 32-byte row from the feature arena (slot -> feature table -> block -> desc
//               + 32 * feature); the good rows are compacted into LDS by a ballot prefix (a group) or by a ballot prefix per wave and a count
//               per wave in LDS (the workgroup), each with its position in the whole row; then the walks of the block entry
//               (desc_group_best, desc_block_best)
// What the store cannot promise between two staged edits is counted among what these kernels read (viol[]); a lane that meets such an entry
// reads nothing through it.  k_refresh_res_commit writes the attribute records where they lie and returns at once when a count is not zero:
// the host does not come between compute and commit.  Integer atomics only (the counts).

namespace {

enum { V_NO_FEATURES = 0, V_FEATURE_RANGE, V_NO_CENTRE, V_NO_REFERENCE, V_REF_NO_FEATURES, V_REF_OCTAVE, kViolations };
constexpr size_t kViolBytes = 64;                      // the counts lie before the records, which stay 64-byte aligned
static_assert(kViolations * 4 <= kViolBytes, "the counts fit their block");

struct ResArgs {
    CovisView v;
    const int32_t *ids;            // [n]
    CovisRefreshOut *out;          // [n]
    int32_t *viol;                 // [kViolations]
    int what;
};

// The descriptor row of (slot, feature) where it lies; zero, and counted, when the store does not hold it.
__device__ __forceinline__ void res_fetch_desc(const ResArgs &a, int slot, int feature, uint4 &r0, uint4 &r1) {
    r0 = r1 = make_uint4(0, 0, 0, 0);
    const long long keys = a.v.feat_keys(slot);
    if (keys < 0) { atomicAdd(&a.viol[V_NO_FEATURES], 1); return; }
    if (feature >= a.v.feat_count(slot)) { atomicAdd(&a.viol[V_FEATURE_RANGE], 1); return; }
    const CovisFeatRec *R = a.v.rec_of_keys(keys);
    const uint4 *d = rec_arr<uint4>(R, R->desc) + 2 * (size_t)feature;
    r0 = d[0]; r1 = d[1];
}

// mvScaleFactors[octave of ref_feature] and mvScaleFactors[nLevels - 1] of the reference slot (:499, :514-515); false, and counted, otherwise.
__device__ __forceinline__ bool res_reference(const ResArgs &a, int ref, int refFeature, float &scaleRef, float &scaleLast) {
    scaleRef = scaleLast = 1.f;
    if (ref < 0) { atomicAdd(&a.viol[V_NO_REFERENCE], 1); return false; }
    const long long keys = a.v.feat_keys(ref);
    if (keys < 0) { atomicAdd(&a.viol[V_REF_NO_FEATURES], 1); return false; }
    if (refFeature >= a.v.feat_count(ref)) { atomicAdd(&a.viol[V_FEATURE_RANGE], 1); return false; }
    const CovisFeatRec *R = a.v.rec_of_keys(keys);
    const int oct = a.v.keys_at(keys)[refFeature].octave;
    if (oct < 0 || oct >= R->nlevels) { atomicAdd(&a.viol[V_REF_OCTAVE], 1); return false; }
    const float *scale = rec_arr<float>(R, R->scale);
    scaleRef = scale[oct]; scaleLast = scale[R->nlevels - 1];
    return true;
}

// GetCameraCenter() of a slot; zero, and counted, when it was never set.
__device__ __forceinline__ float4 res_centre(const ResArgs &a, int slot) {
    if (a.v.centre) {
        const float4 c = a.v.centre_of(slot);
        if (__float_as_int(c.w) != 0) return c;
    }
    atomicAdd(&a.viol[V_NO_CENTRE], 1);
    return make_float4(0.f, 0.f, 0.f, 0.f);
}

// One term of :471-483 in the operation order of rumi_mapping.h (k_refresh_normal forms the same).
__device__ __forceinline__ void res_unit(const float *pos, const float4 &O, float &ux, float &uy, float &uz) {
    const float dx = pos[0] - O.x, dy = pos[1] - O.y, dz = pos[2] - O.z;
    const float nrm = __builtin_sqrtf((dx * dx + dy * dy) + dz * dz);
    ux = dx / nrm; uy = dy / nrm; uz = dz / nrm;
}

// :492-516 on the point's lane, (nx, ny, nz) the sum in list order.
__device__ __forceinline__ void res_finish_normal(const float *pos, const float4 &R, float nx, float ny, float nz, int nObs, float scaleRef, float scaleLast,
                                                  CovisRefreshOut &o) {
    const float cx = pos[0] - R.x, cy = pos[1] - R.y, cz = pos[2] - R.z;
    const float dist = __builtin_sqrtf((cx * cx + cy * cy) + cz * cz);
    const float maxD = dist * scaleRef;
    const float n = (float)nObs;
    o.maxD = maxD; o.minD = maxD / scaleLast;
    o.normal[0] = nx / n; o.normal[1] = ny / n; o.normal[2] = nz / n;
    o.updated = 1;
}

// Points whose observer row has 1..G entries.  list [nList]: positions in ids.
template <int G>
__global__ __launch_bounds__(256) void k_refresh_res_group(ResArgs a, const int32_t *__restrict__ list, int nList) {
    __shared__ uint4 sRow[256 * 2];
    __shared__ int sPos[256];
    const int tid = threadIdx.x, lane = tid & 63, sub = tid & (G - 1);
    const int g = blockIdx.x * (256 / G) + tid / G;
    const bool live = g < nList;
    const int i = live ? list[g] : 0;
    const int p = live ? a.ids[i] : 0;
    int off = 0, L = 0;
    if (live) { const int2 R = a.v.point_obs(p); off = R.x; L = min(R.y, G); }
    const bool has = sub < L, mine = live && sub == 0 && L > 0;  // mine: the point's lane
    const int word = has ? a.v.rows[off + sub] : 0;
    const int slot = covis_obs_slot(word), feature = covis_obs_feature(word);
    const int gbase = lane & ~(G - 1);
    const unsigned long long gmask = G == 64 ? ~0ull : (1ull << (G & 63)) - 1;

    // ---- the reference key-frame: `observations[pRefKF]` (:495)
    const int ref = live ? a.v.ref_slot(p) : -1;
    const unsigned long long isRef = (__ballot(has && slot == ref) >> gbase) & gmask;        // a row lists a slot at most once
    const int refLane = isRef ? __ffsll((long long)isRef) - 1 : 0;
    const int refLaneFeature = __shfl(feature, gbase + refLane);
    const int refFeature = isRef ? refLaneFeature : 0;
    float scaleRef = 1.f, scaleLast = 1.f;
    bool refOk = false;
    if (mine) refOk = res_reference(a, ref, refFeature, scaleRef, scaleLast);

    if (a.what & RUMI_REFRESH_NORMAL_DEPTH) {
        float *sU = reinterpret_cast<float *>(sRow);             // [3][256]
        float pos[3] = {0.f, 0.f, 0.f};
        if (live && L > 0) {
            const float *A = a.v.attr_pos(p);
            pos[0] = A[0]; pos[1] = A[1]; pos[2] = A[2];
        }
        if (has) {                                               // bad key-frames included (:471-490)
            float ux, uy, uz;
            res_unit(pos, res_centre(a, slot), ux, uy, uz);
            sU[tid] = ux; sU[256 + tid] = uy; sU[512 + tid] = uz;
        }
        __syncthreads();
        if (mine) {
            float nx = 0.f, ny = 0.f, nz = 0.f;
            for (int k = 0; k < L; k++) { nx = nx + sU[tid + k]; ny = ny + sU[256 + tid + k]; nz = nz + sU[512 + tid + k]; }
            const float4 R = refOk ? res_centre(a, ref) : make_float4(0.f, 0.f, 0.f, 0.f);
            res_finish_normal(pos, R, nx, ny, nz, L, scaleRef, scaleLast, a.out[i]);
        }
        __syncthreads();                                         // the rows below take the same LDS
    }

    if (a.what & RUMI_REFRESH_DESCRIPTOR) {
        const bool good = has && !a.v.kf_bad(slot);              // :376
        uint4 r0 = make_uint4(0, 0, 0, 0), r1 = r0;
        if (good) res_fetch_desc(a, slot, feature, r0, r1);
        const unsigned long long gm = (__ballot(good) >> gbase) & gmask;
        const int N = __popcll(gm);                              // the rows left
        if (good) {
            const int c = tid - sub + __popcll(gm & ((1ull << sub) - 1ull));
            sRow[2 * c] = r0; sRow[2 * c + 1] = r1; sPos[c] = sub;
        }
        __syncthreads();
        const uint4 *rows = sRow + 2 * (tid - sub);
        uint4 a0 = make_uint4(0, 0, 0, 0), a1 = a0;
        if (sub < N) { a0 = rows[2 * sub]; a1 = rows[2 * sub + 1]; }
        int best, bestIdx;
        desc_group_best<G>(a0, a1, rows, N, sub, lane, best, bestIdx);
        if (mine) {
            CovisRefreshOut &o = a.out[i];
            if (N > 0) {
                o.bestObs = sPos[tid + bestIdx]; o.bestMedian = best;    // the position in the whole row, dropped entries counted
                uint4 *D = reinterpret_cast<uint4 *>(o.desc);
                D[0] = rows[2 * bestIdx]; D[1] = rows[2 * bestIdx + 1];
            } else { o.bestObs = -1; o.bestMedian = -1; }        // :389: every observing key-frame bad
        }
    }
}

// Points of more than 64 observers.  Dynamic LDS: nAlloc rows of 32 bytes (nAlloc >= every L of the launch; the unit vectors lie there
// first), a 257-bin count per wave, nAlloc 16-bit positions.
__global__ __launch_bounds__(256) void k_refresh_res_block(ResArgs a, const int32_t *__restrict__ list, int nAlloc) {
    extern __shared__ uint4 smem[];
    __shared__ int sBest[4], sBestIdx[4], sCnt[4], sRefFeature;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int i = list[blockIdx.x];
    const int p = a.ids[i];
    const int2 P = a.v.point_obs(p);
    const int off = P.x, L = min(P.y, nAlloc);
    uint4 *sRow = smem;
    int *histAll = reinterpret_cast<int *>(smem + 2 * (size_t)nAlloc), *hist = histAll + wave * kHistStride;
    uint16_t *sPos = reinterpret_cast<uint16_t *>(histAll + 4 * kHistStride);
    const int32_t *row = a.v.rows + off;

    const int ref = a.v.ref_slot(p);
    if (tid == 0) sRefFeature = 0;
    __syncthreads();
    for (int k = tid; k < L; k += 256)
        if (covis_obs_slot(row[k]) == ref) sRefFeature = covis_obs_feature(row[k]);     // at most one writer
    __syncthreads();
    float scaleRef = 1.f, scaleLast = 1.f;
    bool refOk = false;
    if (tid == 0) refOk = res_reference(a, ref, sRefFeature, scaleRef, scaleLast);

    if (a.what & RUMI_REFRESH_NORMAL_DEPTH) {
        float *sU = reinterpret_cast<float *>(smem);             // [3][nAlloc]
        const float *A = a.v.attr_pos(p);
        const float pos[3] = {A[0], A[1], A[2]};
        for (int k = tid; k < L; k += 256) {
            float ux, uy, uz;
            res_unit(pos, res_centre(a, covis_obs_slot(row[k])), ux, uy, uz);
            sU[k] = ux; sU[nAlloc + k] = uy; sU[2 * nAlloc + k] = uz;
        }
        __syncthreads();
        if (tid == 0) {
            float nx = 0.f, ny = 0.f, nz = 0.f;
            for (int k = 0; k < L; k++) { nx = nx + sU[k]; ny = ny + sU[nAlloc + k]; nz = nz + sU[2 * nAlloc + k]; }
            const float4 R = refOk ? res_centre(a, ref) : make_float4(0.f, 0.f, 0.f, 0.f);
            res_finish_normal(pos, R, nx, ny, nz, L, scaleRef, scaleLast, a.out[i]);
        }
        __syncthreads();
    }

    if (a.what & RUMI_REFRESH_DESCRIPTOR) {
        int N = 0;                                               // the rows left so far
        for (int k0 = 0; k0 < L; k0 += 256) {
            const int k = k0 + tid;
            const int word = k < L ? row[k] : 0;
            const int slot = covis_obs_slot(word);
            const bool good = k < L && !a.v.kf_bad(slot);
            uint4 r0 = make_uint4(0, 0, 0, 0), r1 = r0;
            if (good) res_fetch_desc(a, slot, covis_obs_feature(word), r0, r1);
            const unsigned long long m = __ballot(good);
            if (lane == 0) sCnt[wave] = __popcll(m);
            __syncthreads();
            int before = 0, all = 0;
            for (int w = 0; w < 4; w++) { const int c = sCnt[w]; before += w < wave ? c : 0; all += c; }
            if (good) {
                const int c = N + before + __popcll(m & ((1ull << lane) - 1ull));
                sRow[2 * c] = r0; sRow[2 * c + 1] = r1; sPos[c] = (uint16_t)k;
            }
            N += all;
            __syncthreads();
        }
        for (int k = lane; k < kHistStride; k += 64) hist[k] = 0;
        __syncthreads();
        int best, bestIdx;
        desc_block_best(sRow, hist, N, tid, lane, wave, sBest, sBestIdx, best, bestIdx);
        if (tid == 0) {
            CovisRefreshOut &o = a.out[i];
            if (N > 0) {
                o.bestObs = sPos[bestIdx]; o.bestMedian = best;
                uint4 *D = reinterpret_cast<uint4 *>(o.desc);
                D[0] = sRow[2 * bestIdx]; D[1] = sRow[2 * bestIdx + 1];
            } else { o.bestObs = -1; o.bestMedian = -1; }
        }
    }
}

// RUMI_REFRESH_WRITE_BACK: the attribute records take the results where they lie, unless the call is being refused.
__global__ __launch_bounds__(256) void k_refresh_res_commit(ResArgs a, int n) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    for (int v = 0; v < kViolations; v++)
        if (a.viol[v]) return;
    const int p = a.ids[i];
    if (a.v.point_obs_len(p) == 0) return;                       // an empty row: both members return before they write
    const CovisRefreshOut &o = a.out[i];
    int32_t *A = a.v.attr_rec(p);
    if ((a.what & RUMI_REFRESH_DESCRIPTOR) && o.bestObs >= 0) {
        const uint4 *D = reinterpret_cast<const uint4 *>(o.desc);
        uint4 *dst = reinterpret_cast<uint4 *>(A + kCovisAttrDesc);
        dst[0] = D[0]; dst[1] = D[1];
    }
    if ((a.what & RUMI_REFRESH_NORMAL_DEPTH) && o.updated) {
        float *F = reinterpret_cast<float *>(A);
        F[3] = o.normal[0]; F[4] = o.normal[1]; F[5] = o.normal[2]; F[6] = o.minD; F[7] = o.maxD;
    }
}

}  // namespace

extern "C" int rumi_refresh_map_points_resident(RumiRefresh *r, RumiCovis *c, const int32_t *ids, int32_t n_pts, int32_t what, int32_t flags,
                                                int32_t *best_obs, int32_t *best_median, uint8_t *desc, float *normal, float *min_distance,
                                                float *max_distance, uint8_t *updated) {
    const char *const E = "rumi_refresh_map_points_resident";
    const bool wantDesc = (what & RUMI_REFRESH_DESCRIPTOR) != 0, wantNormal = (what & RUMI_REFRESH_NORMAL_DEPTH) != 0;
    const bool writeBack = (flags & RUMI_REFRESH_WRITE_BACK) != 0;
    if (!r || !c || n_pts < 0 || (what & ~(RUMI_REFRESH_DESCRIPTOR | RUMI_REFRESH_NORMAL_DEPTH)) || !(wantDesc || wantNormal) ||
        (flags & ~RUMI_REFRESH_WRITE_BACK) || (n_pts > 0 && !ids) || (n_pts > 0 && wantDesc && (!best_obs || !best_median || !desc)) ||
        (n_pts > 0 && wantNormal && (!normal || !min_distance || !max_distance || !updated))) {
        g_lastError = std::string(E) + ": missing argument, negative count, `what` without a known mode bit, or an unknown flag";
        return RUMI_E_INVALID;
    }
    r->clock.start();
    // ---- the mirror: O(1) words a point, nothing per observation
    r->rowLen.resize((size_t)n_pts);
    int rc = covis_refresh_check(c, n_pts, ids, wantNormal || writeBack, E, r->rowLen.data());
    const bool named = r->dev.device >= 0;                   // a handle created without a device learns it when it binds: the rule is asked again then
    if (rc != RUMI_OK || (rc = covis_same_device(c, r->dev.device, E)) != RUMI_OK) return rc;
    for (auto &b : r->bins) b.clear();
    int maxLen = 0;
    for (int i = 0; i < n_pts; i++) {
        const int L = r->rowLen[i];
        if (L > RUMI_REFRESH_MAX_OBS) {
            g_lastError = std::string(E) + ": a point has more than RUMI_REFRESH_MAX_OBS observers";
            return RUMI_E_CAPACITY;
        }
        maxLen = std::max(maxLen, L);
        if (L > 0) r->bins[L <= 16 ? 0 : L <= 32 ? 1 : L <= 64 ? 2 : 3].push_back(i);
    }
    if (n_pts == 0) return RUMI_OK;
    // the workgroup kernel's points longest first, as in the block entry
    std::stable_sort(r->bins[3].begin(), r->bins[3].end(), [&](int a, int b) { return r->rowLen[a] > r->rowLen[b]; });
    size_t nBinned = 0;
    for (auto &b : r->bins) nBinned += b.size();

    // ---- the store's staged edits, then one small block: ids | bin lists
    CovisView cv;
    if ((rc = r->dev.bind()) != RUMI_OK || (!named && (rc = covis_same_device(c, r->dev.device, E)) != RUMI_OK) || (rc = covis_view(c, 0, &cv)) != RUMI_OK) return rc;
    const size_t offList = up16((size_t)n_pts * 4), blkBytes = offList + up16(nBinned * 4);
    const size_t outBytes = kViolBytes + (size_t)n_pts * sizeof(CovisRefreshOut);
    if ((rc = r->blk.reserve(blkBytes, blkBytes + blkBytes / 4)) != RUMI_OK || (rc = r->out.reserve(outBytes, outBytes + outBytes / 4)) != RUMI_OK) return rc;
    std::memcpy(r->blk.h, ids, (size_t)n_pts * 4);
    int32_t *hList = reinterpret_cast<int32_t *>(r->blk.h + offList);
    size_t binOff[4], at = 0;
    for (int b = 0; b < 4; b++) {
        binOff[b] = at;
        if (!r->bins[b].empty()) std::memcpy(hList + at, r->bins[b].data(), r->bins[b].size() * 4);
        at += r->bins[b].size();
    }
    r->clock.mark();
    HIP_TRY(hipMemcpyAsync(r->blk.d, r->blk.h, blkBytes, hipMemcpyHostToDevice, nullptr));
    HIP_TRY(hipMemsetAsync(r->out.d, 0, kViolBytes, nullptr));

    // ---- the launches
    ResArgs a;
    a.v = cv;
    a.ids = reinterpret_cast<const int32_t *>(r->blk.d);
    a.out = reinterpret_cast<CovisRefreshOut *>(r->out.d + kViolBytes);
    a.viol = reinterpret_cast<int32_t *>(r->out.d);
    a.what = what;
    const int32_t *dList = reinterpret_cast<const int32_t *>(r->blk.d + offList);
    const int n0 = (int)r->bins[0].size(), n1 = (int)r->bins[1].size(), n2 = (int)r->bins[2].size(), n3 = (int)r->bins[3].size();
    int launches = 0;
    if (n0) { hipLaunchKernelGGL(k_refresh_res_group<16>, dim3((n0 + 15) / 16), dim3(256), 0, nullptr, a, dList + binOff[0], n0); launches++; }
    if (n1) { hipLaunchKernelGGL(k_refresh_res_group<32>, dim3((n1 + 7) / 8), dim3(256), 0, nullptr, a, dList + binOff[1], n1); launches++; }
    if (n2) { hipLaunchKernelGGL(k_refresh_res_group<64>, dim3((n2 + 3) / 4), dim3(256), 0, nullptr, a, dList + binOff[2], n2); launches++; }
    if (n3) {
        const size_t lds = (size_t)maxLen * 32 + 4 * kHistStride * sizeof(int) + up16((size_t)maxLen * 2);     // at most 64 KiB + 4224 + 4096 bytes
        if (lds > 64 * 1024) HIP_TRY(raise_lds_limit(reinterpret_cast<const void *>(k_refresh_res_block), lds));
        hipLaunchKernelGGL(k_refresh_res_block, dim3(n3), dim3(256), lds, nullptr, a, dList + binOff[3], maxLen);
        launches++;
    }
    if (writeBack && nBinned) { hipLaunchKernelGGL(k_refresh_res_commit, dim3((n_pts + 255) / 256), dim3(256), 0, nullptr, a, n_pts); launches++; }
    HIP_TRY(hipGetLastError());

    // ---- one block back: the counts and a record a point
    HIP_TRY(hipMemcpy(r->out.h, r->out.d, outBytes, hipMemcpyDeviceToHost));
    r->clock.mark();
    const int32_t *viol = reinterpret_cast<const int32_t *>(r->out.h);
    for (int v = 0; v < kViolations; v++)
        if (viol[v]) {
            g_lastError = std::string(E) + ": the store is inconsistent among what the call reads: " + std::to_string(viol[V_NO_FEATURES]) +
                          " observers name a slot without resident features, " + std::to_string(viol[V_FEATURE_RANGE]) +
                          " observations name a feature outside their slot's feature count, " + std::to_string(viol[V_NO_CENTRE]) +
                          " observer or reference slots have no centre, " + std::to_string(viol[V_NO_REFERENCE]) +
                          " points with observers have no reference slot, " + std::to_string(viol[V_REF_NO_FEATURES]) +
                          " reference slots hold no features, " + std::to_string(viol[V_REF_OCTAVE]) +
                          " reference octaves lie outside their scale table";
            return RUMI_E_INVALID;
        }
    const CovisRefreshOut *hOut = reinterpret_cast<const CovisRefreshOut *>(r->out.h + kViolBytes);
    for (int i = 0; i < n_pts; i++) {
        const bool any = r->rowLen[i] > 0;
        const CovisRefreshOut &o = hOut[i];
        if (wantDesc) {
            const bool has = any && o.bestObs >= 0;              // :367, :389
            best_obs[i] = has ? o.bestObs : -1;
            best_median[i] = has ? o.bestMedian : -1;
            if (has) std::memcpy(desc + 32 * (size_t)i, o.desc, 32);
        }
        if (wantNormal) {
            updated[i] = any;
            if (any) {
                std::memcpy(normal + 3 * (size_t)i, o.normal, 12);
                min_distance[i] = o.minD; max_distance[i] = o.maxD;
            }
        }
    }
    if (writeBack) covis_refresh_write_mirror(c, n_pts, ids, r->rowLen.data(), hOut, wantDesc, wantNormal);
    r->launches = launches;
    r->clock.finish(r->stageMs);
    return RUMI_OK;
}

extern "C" int32_t rumi_refresh_last_launches(const RumiRefresh *r) { return r ? r->launches : -1; }
