// LocalMapping::KeyFrameCulling (R/lib_src/LocalMapping.cc:953-1079) and CloudKeyFrameCulling (:820-951) for the whole covisible list
// (include/rumi_mapping.h, rumi_keyframe_culling).
//
// The host validates every index and the consistency of the map, then packs one pinned block: point records, a byte table of the octaves
// of every key-frame, the observation pairs as the caller gave them, and the map-point row of every candidate the loop can reach.
//   k_cull_first    a lane per (candidate, feature slot), all candidates at once, with no key-frame culled: is the slot's point counted in
//                   nMPs, is it redundant.  The lane walks the point's observations, reads the observer's octave from the byte table and
//                   stops at the fourth qualifying one (:1032).  Two bits a slot are kept; the counts per candidate are summed by ballot +
//                   popcount, one integer LDS atomic a wave and one integer global atomic a workgroup.
//   k_cull_replay   one workgroup takes the candidates in order with the set S of culled key-frames as a bit set in LDS.  A cull adds one
//                   to the culled-observer count kept in every point record of the culled key-frame.  A slot whose point has no culled
//                   observer keeps its two bits of the first pass; any other slot is evaluated again under S: nObs = n_obs_count - culled
//                   observers, bad when that is <= 2, observers in S ignored.  Emits status and counts per candidate, the culled list in
//                   order, and stops where the reference breaks (:1075).
// rumi_keyframe_culling_resident runs the same two kernels over the covisibility store (covis.hip) instead of a packed block: both are templates
// over a view of the map (BlockView, ResidentView).  The host decides the candidates' status from the store's mirror and checks their points'
// "has observation features" flags; the store's staged edits and 16 bytes a candidate travel.
//   k_cull_check    resident entry only, before the first pass: a lane per (evaluated candidate, feature slot) walks the point's whole observer
//                   row and counts what the block entry's host validation would refuse -- an observer without resident features, an
//                   observation whose feature lies outside the observer's row or whose slot there holds another point, a candidate slot whose
//                   point does not list it.  Any count makes the two kernels behind it return at once and the call RUMI_E_INVALID.
// No binning by observation length (refresh.hip bins because its work is quadratic in the length): here a walk is linear and ends at the
// fourth qualifying observer; DESIGN 4j gives the walk lengths counted on the probe workloads (about 7 entries of 26 where lists reach 40).
// Integer arithmetic only, but for the verdict (one float multiply, one compare; the library is built with -ffp-contract=off).
#include <algorithm>
#include <climits>
#include <cstring>
#include <vector>

#include "rumi_common.h"
#include "covis_view.h"
#include "rumi_mapping.h"

namespace rumi {
namespace {

constexpr int kFirstThreads = 256, kReplayThreads = 1024;
constexpr int kBitWords = RUMI_CULL_MAX_KEYFRAMES / 32;

// Candidate record: x = key-frame, y = first entry of its slice of `first`, z = its feature count, w = the status decided on the host
// (0 = evaluate) | not_erase << 8.
struct CullArgs {
    const int4 *cands;
    int2 *counts;                 // [nUp] nMPs, nRedundant of the first pass; zero when uploaded
    uint8_t *first;               // [the candidates' rows, one after the other] bit 0 counted in nMPs, bit 1 redundant
    const int32_t *defects;       // resident entry: what k_cull_check counted (zero when uploaded); null for the block entry
    int4 *out;                    // [nUp] status, nMPs, nRedundant | [nUp .. ] x = culled count (-1: defects in y z w), y = candidates reached | culled list
    int nUp, limit;
};

// What the loop reads of a point: its observations [first, first + len), Observations(), isBad() at the call, and how many of its
// observers this call has culled so far.
struct CullPoint { int first, len, nObs, bad, gone; };

// The two views of the map.  BlockView: the block rumi_keyframe_culling packs.  Point record: x = first observation, y = number of
// observations, z = n_obs_count, w = bit 0 bad at the call | culled observers << 8 (zero when uploaded; only k_cull_replay writes it).
struct BlockView {
    int4 *pts;
    const int32_t *rows;          // the candidates' map-point rows; a candidate's row starts at its cd.y
    const int32_t *obsKf, *obsFeature;
    const int32_t *octOff;        // [n_kf] first byte of the key-frame's octaves
    const uint8_t *oct;
    __device__ __forceinline__ CullPoint point(int p) const { const int4 P = pts[p]; return CullPoint{P.x, P.y, P.z, P.w & 1, P.w >> 8}; }
    __device__ __forceinline__ int gone(int p) const { return pts[p].w >> 8; }
    __device__ __forceinline__ void add_gone(int p) const { pts[p].w += 256; }
    __device__ __forceinline__ const int32_t *row(const int4 &cd) const { return rows + cd.y; }
    __device__ __forceinline__ int2 obs(int o) const { return make_int2(obsKf[o], obsFeature[o]); }
    __device__ __forceinline__ int octave(int k, int f) const { return (int)oct[octOff[k] + f]; }
};

// ResidentView: the covisibility store's own tables (covis.hip), read in place.  Observations() is the length of the observer row; the
// culled-observer count is a word per point owned by the RumiCull handle, (call epoch << 8) | count, never cleared between calls.
struct ResidentView {
    CovisView s;                                                    // read through: point, kf_row, the observer words, featTab, the octave table
    uint32_t *goneOf;
    uint32_t epoch;
    __device__ __forceinline__ int gone(int p) const { const uint32_t w = goneOf[p]; return (w >> 8) == epoch ? (int)(w & 255u) : 0; }
    __device__ __forceinline__ void add_gone(int p) const { const uint32_t w = goneOf[p]; goneOf[p] = (w >> 8) == epoch ? w + 1u : (epoch << 8) | 1u; }
    __device__ __forceinline__ CullPoint point(int p) const {
        const CovisPoint P = s.point(p);
        return CullPoint{P.obs_off(), P.obs_len(), P.obs_len(), P.bad(), gone(p)};
    }
    __device__ __forceinline__ const int32_t *row(const int4 &cd) const { return s.kf_row(cd.x); }
    __device__ __forceinline__ int2 obs(int o) const { const int w = s.rows[o]; return make_int2(covis_obs_slot(w), covis_obs_feature(w)); }
    __device__ __forceinline__ int octave(int k, int f) const { return s.octave(k, f); }
};

// One slot of key-frame `own` (octave ownOct) holding point p: bit 0 counted in nMPs (:1000-1006), bit 1 redundant (:1007-1038).
// culled: the bit set S, or NULL for the empty set.
template <class V> __device__ __forceinline__ int eval_slot(const V &v, int p, int own, int ownOct, const uint32_t *culled) {
    const CullPoint P = v.point(p);
    const int nObs = P.nObs - P.gone;                                // MapPoint.cc:206 for every culled observer
    if (P.bad || (P.gone > 0 && nObs <= 2)) return 0;                // isBad(): at the call, or MapPoint.cc:218
    if (nObs <= 3) return 1;                                         // :1007
    int n = 0;
    for (int o = P.first, e = P.first + P.len; o < e; o++) {         // :1011
        const int2 kfq = v.obs(o);
        const int k = kfq.x;
        if (k == own) continue;                                      // :1013
        if (culled && ((culled[k >> 5] >> (k & 31)) & 1)) continue;  // erased by that key-frame's SetBadFlag
        if (v.octave(k, kfq.y) <= ownOct + 1 && ++n > 3) return 3;   // :1030-1037
    }
    return 1;
}

__device__ __forceinline__ bool has_defects(const CullArgs &a) { return a.defects && (a.defects[0] | a.defects[1] | a.defects[2]) != 0; }

// The resident entry's consistency check, a lane per (evaluated candidate, feature slot): every observation (k, f) of the slot's point names
// a key-frame with resident features and a feature inside k's row that holds the point, and the point lists (candidate, slot).  Reads
// nothing it has not checked; the two kernels behind it return at once when it counted anything.
__global__ __launch_bounds__(kFirstThreads) void k_cull_check(ResidentView v, CullArgs a, int32_t *defects) {
    const int c = blockIdx.x, i = (int)blockIdx.y * kFirstThreads + (int)threadIdx.x;
    const int4 cd = a.cands[c];
    if ((cd.w & 0xff) != 0 || i >= cd.z) return;
    const int p = v.row(cd)[i];
    if (p < 0) return;
    const CovisPoint P = v.s.point(p);
    int noFeat = 0, dangling = 0;
    bool listed = false;
    for (int o = P.obs_off(), e = P.obs_off() + P.obs_len(); o < e; o++) {
        const int2 kfq = v.obs(o);
        const int k = kfq.x, f = kfq.y;
        if (v.s.feat_keys(k) < 0) { noFeat++; continue; }
        if (f >= v.s.feat_count(k) || f >= v.s.kf_row_len(k) || v.s.kf_row_entry(k, f) != p) dangling++;
        listed = listed || (k == cd.x && f == i);
    }
    if (noFeat) atomicAdd(&defects[0], noFeat);
    if (dangling) atomicAdd(&defects[1], dangling);
    if (!listed) atomicAdd(&defects[2], 1);
}

template <class V> __global__ __launch_bounds__(kFirstThreads) void k_cull_first(V v, CullArgs a) {
    __shared__ int sCount[2];
    const int c = blockIdx.x, tid = threadIdx.x, i = (int)blockIdx.y * kFirstThreads + tid;
    const int4 cd = a.cands[c];
    if ((cd.w & 0xff) != 0 || (int)blockIdx.y * kFirstThreads >= cd.z || has_defects(a)) return;    // uniform for the workgroup
    if (tid < 2) sCount[tid] = 0;
    __syncthreads();
    int r = 0;
    if (i < cd.z) {
        const int p = v.row(cd)[i];
        if (p >= 0) r = eval_slot(v, p, cd.x, v.octave(cd.x, i), nullptr);
        a.first[cd.y + i] = (uint8_t)r;
    }
    const int nm = __popcll(__ballot(r & 1)), nr = __popcll(__ballot(r & 2));
    if ((tid & 63) == 0) { atomicAdd(&sCount[0], nm); atomicAdd(&sCount[1], nr); }
    __syncthreads();
    if (tid == 0) { atomicAdd(&a.counts[c].x, sCount[0]); atomicAdd(&a.counts[c].y, sCount[1]); }
}

template <class V> __global__ __launch_bounds__(kReplayThreads) void k_cull_replay(V v, CullArgs a) {
    __shared__ uint32_t sCulled[kBitWords];
    __shared__ int sCount[2];
    const int tid = threadIdx.x;
    int4 *head = a.out + a.nUp;
    if (has_defects(a)) {                                            // uniform: the host refuses the call with these counts
        if (tid == 0) *head = make_int4(-1, a.defects[0], a.defects[1], a.defects[2]);
        return;
    }
    for (int w = tid; w < kBitWords; w += kReplayThreads) sCulled[w] = 0;
    __syncthreads();
    int32_t *list = reinterpret_cast<int32_t *>(head + 1);
    int nCulled = 0, reached = a.nUp;
    for (int c = 0; c < a.nUp; c++) {                                // count = c + 1 (:986); every value below is uniform
        const int4 cd = a.cands[c];
        int st = cd.w & 0xff;
        if (st == 0 && ((sCulled[cd.x >> 5] >> (cd.x & 31)) & 1)) st = RUMI_CULL_SKIPPED_BAD;   // culled earlier in this loop (:989)
        __syncthreads();                                             // every wave has read S before this candidate's verdict may add to it: a wave
                                                                     // that read the bit of its own candidate would skip the cull the others apply
        if (st != 0) {                                               // `continue`: no break test
            if (tid == 0) a.out[c] = make_int4(st, 0, 0, 0);
            continue;
        }
        const int32_t *row = v.row(cd);
        int nMPs, nRed;
        if (nCulled == 0) { const int2 f = a.counts[c]; nMPs = f.x; nRed = f.y; }
        else {
            if (tid < 2) sCount[tid] = 0;
            __syncthreads();
            int nm = 0, nr = 0;
            for (int i = tid; i < cd.z; i += kReplayThreads) {
                const int p = row[i];
                if (p < 0) continue;
                const int r = v.gone(p) == 0 ? a.first[cd.y + i] : eval_slot(v, p, cd.x, v.octave(cd.x, i), sCulled);
                nm += r & 1; nr += (r >> 1) & 1;
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) { nm += __shfl_xor(nm, o); nr += __shfl_xor(nr, o); }
            if ((tid & 63) == 0) { atomicAdd(&sCount[0], nm); atomicAdd(&sCount[1], nr); }
            __syncthreads();
            nMPs = sCount[0]; nRed = sCount[1];
            __syncthreads();
        }
        const bool redundant = (float)nRed > 0.9f * (float)nMPs;     // :1044
        const bool erase = redundant && !(cd.w >> 8);                // KeyFrame.cc:783
        if (tid == 0) {
            a.out[c] = make_int4(!redundant ? RUMI_CULL_KEPT : erase ? RUMI_CULL_CULLED : RUMI_CULL_TO_BE_ERASED, nMPs, nRed, 0);
            if (erase) { list[nCulled] = c; sCulled[cd.x >> 5] |= 1u << (cd.x & 31); }
        }
        if (erase) {                                                 // KeyFrame.cc:793-797: a slot holds a point once, so no two lanes meet
            for (int i = tid; i < cd.z; i += kReplayThreads) {
                const int p = row[i];
                if (p >= 0) v.add_gone(p);
            }
            nCulled++;
            __syncthreads();                                         // the bit and the point records, before the next candidate reads them
        }
        if (c + 1 > a.limit) { reached = c + 1; break; }             // :1075
    }
    if (tid == 0) *head = make_int4(nCulled, reached, 0, 0);
}

}  // namespace
}  // namespace rumi

using namespace rumi;

struct RumiCull {
    DeviceBinding dev;
    MirrorBuf<uint8_t> blk, out;
    std::vector<int32_t> stamp, slots, octOff;
    std::vector<int4> cands;
    DevBuf<uint32_t> gone;                // resident entry: (epoch << 8) | culled observers, a word per point of the largest store seen
    uint32_t epoch = 0;
    StageClock clock;
    float stageMs[3] = {0.f, 0.f, 0.f};   // the last call: validation + pack | upload, kernels, download | write-out
};

extern "C" int rumi_cull_create(int32_t device, RumiCull **out) {
    if (!out) return RUMI_E_INVALID;
    *out = new RumiCull();
    (*out)->dev.device = device;
    return RUMI_OK;
}

extern "C" void rumi_cull_destroy(RumiCull *c) {
    if (!c) return;
    if (c->dev.bound) (void)hipSetDevice(c->dev.device);
    delete c;
}

extern "C" int rumi_keyframe_culling(RumiCull *h, const RumiCullKF *kfs, int32_t n_kf, const int32_t *cand, int32_t n_cand,
                                     const RumiCullPoint *pts, int32_t n_pts, const int32_t *obs_kf, const int32_t *obs_feature, int32_t n_obs,
                                     int32_t flags, int32_t *status, int32_t *n_mps, int32_t *n_redundant, int32_t *culled, int32_t *n_culled) {
    if (!h || n_kf < 0 || n_cand < 0 || n_pts < 0 || n_obs < 0 || (flags & ~(RUMI_CULL_CLOUD | RUMI_CULL_ABORT_BA)) || !n_culled ||
        (n_kf > 0 && !kfs) || (n_pts > 0 && !pts) || (n_obs > 0 && (!obs_kf || !obs_feature)) ||
        (n_cand > 0 && (!cand || !status || !n_mps || !n_redundant || !culled))) {
        g_lastError = "rumi_keyframe_culling: missing argument, negative count or unknown flag";
        return RUMI_E_INVALID;
    }
    h->clock.start();
    // ---- validation, all of it before anything is written or uploaded
    h->octOff.resize((size_t)n_kf + 1);
    h->slots.assign(n_pts, 0);
    int64_t nOct = 0;
    for (int k = 0; k < n_kf; k++) {
        const RumiCullKF &K = kfs[k];
        if (K.n < 0 || (K.n > 0 && (!K.octave || !K.mp))) {
            g_lastError = "rumi_keyframe_culling: a key-frame with a negative feature count or without its tables";
            return RUMI_E_INVALID;
        }
        h->octOff[k] = (int32_t)nOct;
        nOct += K.n;
        if (nOct > INT32_MAX) { g_lastError = "rumi_keyframe_culling: more than 2^31 features"; return RUMI_E_INVALID; }
        for (int i = 0; i < K.n; i++) {
            const int32_t p = K.mp[i];
            if (p < -1 || p >= n_pts || (uint32_t)K.octave[i] > 127u) {
                g_lastError = "rumi_keyframe_culling: an mp entry outside the point table or an octave outside 0..127";
                return RUMI_E_INVALID;
            }
            if (p >= 0) h->slots[p]++;
        }
    }
    h->octOff[n_kf] = (int32_t)nOct;
    for (int c = 0; c < n_cand; c++)
        if (cand[c] < 0 || cand[c] >= n_kf) {
            g_lastError = "rumi_keyframe_culling: a candidate outside the key-frame table";
            return RUMI_E_INVALID;
        }
    h->stamp.assign(n_kf, -1);
    bool tooMany = false;
    auto slots_agree = [&](int p) -> int {                                // every observation of p names a slot that holds p, and no slot is left over
        const RumiCullPoint &P = pts[p];
        for (int o = P.obs_begin; o < P.obs_end; o++) {
            const int k = obs_kf[o];
            if (kfs[k].mp[obs_feature[o]] != p || h->stamp[k] == p) {
                g_lastError = "rumi_keyframe_culling: an observation whose key-frame slot does not hold the point, or a point that lists a key-frame twice";
                return RUMI_E_INVALID;
            }
            h->stamp[k] = p;
        }
        if (h->slots[p] != P.obs_end - P.obs_begin) {                // every listed pair is a distinct slot holding p: more slots = one not listed
            g_lastError = "rumi_keyframe_culling: an mp entry whose point does not list that (key-frame, feature) pair";
            return RUMI_E_INVALID;
        }
        return RUMI_OK;
    };
    int rc = check_observation_table("rumi_keyframe_culling", n_kf, [&](int k) { return kfs[k].n; }, pts, n_pts, obs_kf, obs_feature, n_obs,
                                     RUMI_REFRESH_MAX_OBS, &tooMany, slots_agree);
    if (rc != RUMI_OK) return rc;
    if (tooMany || n_kf > RUMI_CULL_MAX_KEYFRAMES) {
        g_lastError = "rumi_keyframe_culling: a point has more than RUMI_REFRESH_MAX_OBS observations, or more than RUMI_CULL_MAX_KEYFRAMES key-frames";
        return RUMI_E_CAPACITY;
    }
    if (n_cand == 0) { *n_culled = 0; return RUMI_OK; }

    // ---- the candidates the loop can reach: up to the first one past the limit that is certain to be evaluated (:1075 sits behind the `continue`s)
    const int limit = (flags & RUMI_CULL_ABORT_BA) ? 20 : 100;
    h->cands.clear();
    std::fill(h->stamp.begin(), h->stamp.end(), -1);
    size_t nRows = 0;
    int maxN = 0;
    for (int c = 0; c < n_cand; c++) {
        const RumiCullKF &K = kfs[cand[c]];
        const int st = ((flags & RUMI_CULL_CLOUD) && K.is_cloud) ? RUMI_CULL_SKIPPED_CLOUD : K.is_init ? RUMI_CULL_SKIPPED_INIT : K.is_bad ? RUMI_CULL_SKIPPED_BAD : 0;
        const bool again = h->stamp[cand[c]] == 0;                   // listed before: bad by now if it was culled there
        h->stamp[cand[c]] = 0;
        h->cands.push_back(make_int4(cand[c], (int)nRows, st == 0 ? K.n : 0, st | (K.not_erase ? 256 : 0)));
        if (st == 0) { nRows += K.n; maxN = std::max(maxN, K.n); }
        if (nRows > INT32_MAX) { g_lastError = "rumi_keyframe_culling: more than 2^31 candidate features"; return RUMI_E_INVALID; }
        if (st == 0 && !again && c + 1 > limit) break;
    }
    const int nUp = (int)h->cands.size();

    // ---- one block: points | candidates | first-pass counts | octave offsets | rows | observations | octaves || (device only) first-pass bits
    const size_t offPts = 0, offCand = up16((size_t)n_pts * 16), offCount = offCand + (size_t)nUp * 16, offOctOff = offCount + up16((size_t)nUp * 8),
                 offRows = offOctOff + up16(((size_t)n_kf + 1) * 4), offObsKf = offRows + up16(nRows * 4), offObsF = offObsKf + up16((size_t)n_obs * 4),
                 offOct = offObsF + up16((size_t)n_obs * 4), upBytes = offOct + up16((size_t)nOct), blkBytes = upBytes + up16(nRows);
    const size_t outBytes = ((size_t)nUp + 1) * 16 + up16((size_t)nUp * 4);
    if ((rc = h->dev.bind()) != RUMI_OK || (rc = h->blk.reserve(blkBytes, blkBytes + blkBytes / 4)) != RUMI_OK ||
        (rc = h->out.reserve(outBytes, outBytes + outBytes / 4)) != RUMI_OK)
        return rc;
    uint8_t *b = h->blk.h;
    int4 *hPts = reinterpret_cast<int4 *>(b + offPts);
    for (int p = 0; p < n_pts; p++) hPts[p] = make_int4(pts[p].obs_begin, pts[p].obs_end - pts[p].obs_begin, pts[p].n_obs_count, pts[p].is_bad ? 1 : 0);
    std::memcpy(b + offCand, h->cands.data(), (size_t)nUp * 16);
    std::memset(b + offCount, 0, (size_t)nUp * 8);
    std::memcpy(b + offOctOff, h->octOff.data(), ((size_t)n_kf + 1) * 4);
    int32_t *hRows = reinterpret_cast<int32_t *>(b + offRows);
    for (const int4 &cd : h->cands)
        if (cd.z > 0) std::memcpy(hRows + cd.y, kfs[cd.x].mp, (size_t)cd.z * 4);
    if (n_obs > 0) { std::memcpy(b + offObsKf, obs_kf, (size_t)n_obs * 4); std::memcpy(b + offObsF, obs_feature, (size_t)n_obs * 4); }
    uint8_t *hOct = b + offOct;
    for (int k = 0; k < n_kf; k++) {
        const int32_t *src = kfs[k].octave;
        uint8_t *dst = hOct + h->octOff[k];
        for (int i = 0; i < kfs[k].n; i++) dst[i] = (uint8_t)src[i];
    }
    h->clock.mark();
    HIP_TRY(hipMemcpyAsync(h->blk.d, h->blk.h, upBytes, hipMemcpyHostToDevice, nullptr));

    // ---- the two launches
    BlockView v;
    v.pts = reinterpret_cast<int4 *>(h->blk.d + offPts);
    v.rows = reinterpret_cast<const int32_t *>(h->blk.d + offRows);
    v.obsKf = reinterpret_cast<const int32_t *>(h->blk.d + offObsKf);
    v.obsFeature = reinterpret_cast<const int32_t *>(h->blk.d + offObsF);
    v.octOff = reinterpret_cast<const int32_t *>(h->blk.d + offOctOff);
    v.oct = h->blk.d + offOct;
    CullArgs a;
    a.cands = reinterpret_cast<const int4 *>(h->blk.d + offCand);
    a.counts = reinterpret_cast<int2 *>(h->blk.d + offCount);
    a.first = h->blk.d + upBytes;
    a.defects = nullptr;
    a.out = reinterpret_cast<int4 *>(h->out.d);
    a.nUp = nUp; a.limit = limit;
    if (maxN > 0) hipLaunchKernelGGL(k_cull_first<BlockView>, dim3(nUp, (maxN + kFirstThreads - 1) / kFirstThreads), dim3(kFirstThreads), 0, nullptr, v, a);
    hipLaunchKernelGGL(k_cull_replay<BlockView>, dim3(1), dim3(kReplayThreads), 0, nullptr, v, a);
    HIP_TRY(hipGetLastError());

    // ---- one block back
    HIP_TRY(hipMemcpy(h->out.h, h->out.d, outBytes, hipMemcpyDeviceToHost));
    h->clock.mark();
    const int4 *res = reinterpret_cast<const int4 *>(h->out.h);
    const int nCulled = res[nUp].x, reached = res[nUp].y;
    const int32_t *list = reinterpret_cast<const int32_t *>(res + nUp + 1);
    for (int c = 0; c < n_cand; c++) {
        const bool in = c < reached;
        status[c] = in ? res[c].x : RUMI_CULL_NOT_REACHED;
        n_mps[c] = in ? res[c].y : 0;
        n_redundant[c] = in ? res[c].z : 0;
    }
    for (int i = 0; i < nCulled; i++) culled[i] = list[i];
    *n_culled = nCulled;
    h->clock.finish(h->stageMs);
    return RUMI_OK;
}

extern "C" int rumi_keyframe_culling_resident(RumiCull *h, RumiCovis *c, const RumiCullCandidate *cand, int32_t n_cand, int32_t flags, int32_t *status,
                                              int32_t *n_mps, int32_t *n_redundant, int32_t *culled, int32_t *n_culled) {
    const char *const E = "rumi_keyframe_culling_resident";
    if (!c || n_cand < 0 || (flags & ~(RUMI_CULL_CLOUD | RUMI_CULL_ABORT_BA)) || !n_culled ||
        (n_cand > 0 && (!cand || !status || !n_mps || !n_redundant || !culled))) {
        g_lastError = std::string(E) + ": missing argument, negative count or unknown flag";
        return RUMI_E_INVALID;
    }
    StageClock clock;
    clock.start();
    // ---- the candidates the loop can reach and their status, as rumi_keyframe_culling decides them; the bad bit is the store's
    const int limit = (flags & RUMI_CULL_ABORT_BA) ? 20 : 100;
    std::vector<int4> cands;
    std::vector<int32_t> seen;
    size_t nRows = 0;
    int maxN = 0, without = 0, longest = 0;
    for (int i = 0; i < n_cand; i++) {
        CovisCullSlot S;
        covis_cull_slot(c, cand[i].slot, &S);
        if (!S.live) { g_lastError = std::string(E) + ": a candidate slot that is not live"; return RUMI_E_INVALID; }
    }
    for (int i = 0; i < n_cand; i++) {
        const RumiCullCandidate &K = cand[i];
        CovisCullSlot S;
        covis_cull_slot(c, K.slot, &S);
        const int st = ((flags & RUMI_CULL_CLOUD) && K.is_cloud) ? RUMI_CULL_SKIPPED_CLOUD : K.is_init ? RUMI_CULL_SKIPPED_INIT : S.bad ? RUMI_CULL_SKIPPED_BAD : 0;
        const bool again = std::find(seen.begin(), seen.end(), K.slot) != seen.end();     // at most limit + skipped entries
        if (!again) seen.push_back(K.slot);
        if (st == 0) {
            if (S.nFeat < 0 || S.nFeat != S.mpLen) {
                g_lastError = std::string(E) + ": a candidate that holds no features (rumi_covis_set_keyframe_features), or whose feature count differs from the length of its map-point row";
                return RUMI_E_INVALID;
            }
            int32_t w, l;
            covis_cull_row_points(c, S.mpOff, S.mpLen, &w, &l);
            without += w; longest = std::max(longest, l);
        }
        cands.push_back(make_int4(K.slot, (int)nRows, st == 0 ? S.mpLen : 0, st | (K.not_erase ? 256 : 0)));
        if (st == 0) { nRows += (size_t)S.mpLen; maxN = std::max(maxN, S.mpLen); }
        if (st == 0 && !again && i + 1 > limit) break;
    }
    if (without > 0) {
        g_lastError = std::string(E) + ": " + std::to_string(without) + " map-point slots of the candidates hold a point without observation features (rumi_covis_set_point_observations)";
        return RUMI_E_INVALID;
    }
    if (longest > RUMI_REFRESH_MAX_OBS) { g_lastError = std::string(E) + ": a point has more than RUMI_REFRESH_MAX_OBS observations"; return RUMI_E_CAPACITY; }
    if (!h) { g_lastError = std::string(E) + ": missing handle"; return RUMI_E_INVALID; }
    if (n_cand == 0) { *n_culled = 0; return RUMI_OK; }
    const int nUp = (int)cands.size();

    // ---- the staged edits of the store, then one small block: candidates | first-pass counts | defect counts || (device only) first-pass bits
    int rc;
    CovisView cv;
    const bool named = h->dev.device >= 0;                   // a handle created without a device learns it when it binds: the rule is asked again then
    if ((rc = covis_same_device(c, h->dev.device, E)) != RUMI_OK || (rc = h->dev.bind()) != RUMI_OK) return rc;
    if ((!named && (rc = covis_same_device(c, h->dev.device, E)) != RUMI_OK) || (rc = covis_view(c, kCovisWantOctaves, &cv)) != RUMI_OK) return rc;
    const size_t offCount = (size_t)nUp * 16, offDefect = offCount + up16((size_t)nUp * 8), upBytes = offDefect + 16, blkBytes = upBytes + up16(nRows);
    const size_t outBytes = ((size_t)nUp + 1) * 16 + up16((size_t)nUp * 4);
    if ((rc = h->blk.reserve(blkBytes, blkBytes + blkBytes / 4)) != RUMI_OK || (rc = h->out.reserve(outBytes, outBytes + outBytes / 4)) != RUMI_OK) return rc;
    if (h->gone.cap < (size_t)cv.maxPoints || h->epoch >= (1u << 24) - 1) {          // a new block, or the stamp's 24 bits are used up
        if ((rc = h->gone.reserve((size_t)cv.maxPoints, (size_t)cv.maxPoints)) != RUMI_OK) return rc;
        HIP_TRY(hipMemsetAsync(h->gone.p, 0, h->gone.cap * 4, nullptr));
        h->epoch = 0;
    }
    h->epoch++;
    std::memcpy(h->blk.h, cands.data(), (size_t)nUp * 16);
    std::memset(h->blk.h + offCount, 0, upBytes - offCount);
    clock.mark();
    HIP_TRY(hipMemcpyAsync(h->blk.d, h->blk.h, upBytes, hipMemcpyHostToDevice, nullptr));

    ResidentView v{cv, h->gone.p, h->epoch};
    CullArgs a;
    a.cands = reinterpret_cast<const int4 *>(h->blk.d);
    a.counts = reinterpret_cast<int2 *>(h->blk.d + offCount);
    a.first = h->blk.d + upBytes;
    a.defects = reinterpret_cast<const int32_t *>(h->blk.d + offDefect);
    a.out = reinterpret_cast<int4 *>(h->out.d);
    a.nUp = nUp; a.limit = limit;
    if (maxN > 0) {
        const dim3 grid(nUp, (maxN + kFirstThreads - 1) / kFirstThreads);
        hipLaunchKernelGGL(k_cull_check, grid, dim3(kFirstThreads), 0, nullptr, v, a, reinterpret_cast<int32_t *>(h->blk.d + offDefect));
        hipLaunchKernelGGL(k_cull_first<ResidentView>, grid, dim3(kFirstThreads), 0, nullptr, v, a);
    }
    hipLaunchKernelGGL(k_cull_replay<ResidentView>, dim3(1), dim3(kReplayThreads), 0, nullptr, v, a);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(h->out.h, h->out.d, outBytes, hipMemcpyDeviceToHost));
    clock.mark();
    const int4 *res = reinterpret_cast<const int4 *>(h->out.h);
    if (res[nUp].x < 0) {
        g_lastError = std::string(E) + ": the map is inconsistent among what the loop reads: " + std::to_string(res[nUp].y) +
                      " observations name a key-frame without resident features, " + std::to_string(res[nUp].z) +
                      " name a feature outside the key-frame's row or one that does not hold the point, " + std::to_string(res[nUp].w) +
                      " candidate slots hold a point that does not list that (key-frame, feature) pair";
        return RUMI_E_INVALID;
    }
    const int nCulled = res[nUp].x, reached = res[nUp].y;
    const int32_t *list = reinterpret_cast<const int32_t *>(res + nUp + 1);
    for (int i = 0; i < n_cand; i++) {
        const bool in = i < reached;
        status[i] = in ? res[i].x : RUMI_CULL_NOT_REACHED;
        n_mps[i] = in ? res[i].y : 0;
        n_redundant[i] = in ? res[i].z : 0;
    }
    for (int i = 0; i < nCulled; i++) culled[i] = list[i];
    *n_culled = nCulled;
    h->clock = clock;
    h->clock.finish(h->stageMs);
    return RUMI_OK;
}

extern "C" int rumi_cull_stage_ms(const RumiCull *c, float *out3) {
    if (!c || !out3) return RUMI_E_INVALID;
    std::memcpy(out3, c->stageMs, sizeof c->stageMs);
    return RUMI_OK;
}
