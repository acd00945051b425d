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
// No binning by observation length (refresh.hip bins because its work is quadratic in the length): here a walk is linear and ends at the
// fourth qualifying observer; DESIGN 4j gives the walk lengths counted on the probe workloads (about 7 entries of 26 where lists reach 40).
// Integer arithmetic only, but for the verdict (one float multiply, one compare; the library is built with -ffp-contract=off).
#include <algorithm>
#include <climits>
#include <cstring>
#include <vector>

#include "rumi_common.h"
#include "rumi_mapping.h"

namespace rumi {
namespace {

constexpr int kFirstThreads = 256, kReplayThreads = 1024;
constexpr int kBitWords = RUMI_CULL_MAX_KEYFRAMES / 32;

// Point record: x = first observation, y = number of observations, z = n_obs_count, w = bit 0 bad at the call | culled observers << 8
// (zero when uploaded; only k_cull_replay writes it).
// Candidate record: x = key-frame, y = first entry of its map-point row, z = its feature count, w = the status decided on the host
// (0 = evaluate) | not_erase << 8.
struct CullArgs {
    int4 *pts;
    const int4 *cands;
    int2 *counts;                 // [nUp] nMPs, nRedundant of the first pass; zero when uploaded
    const int32_t *rows;          // the candidates' map-point rows
    uint8_t *first;               // [as rows] bit 0 counted in nMPs, bit 1 redundant
    const int32_t *obsKf, *obsFeature;
    const int32_t *octOff;        // [n_kf] first byte of the key-frame's octaves
    const uint8_t *oct;
    int4 *out;                    // [nUp] status, nMPs, nRedundant | [nUp .. ] x = culled count, y = candidates reached | culled list
    int nUp, limit;
};

// One slot of key-frame `own` (octave ownOct) holding point p: bit 0 counted in nMPs (:1000-1006), bit 1 redundant (:1007-1038).
// culled: the bit set S, or NULL for the empty set.
__device__ __forceinline__ int eval_slot(const CullArgs &a, int p, int own, int ownOct, const uint32_t *culled) {
    const int4 P = a.pts[p];
    const int gone = P.w >> 8, nObs = P.z - gone;                    // MapPoint.cc:206 for every culled observer
    if ((P.w & 1) || (gone > 0 && nObs <= 2)) return 0;             // isBad(): at the call, or MapPoint.cc:218
    if (nObs <= 3) return 1;                                         // :1007
    int n = 0;
    for (int o = P.x, e = P.x + P.y; o < e; o++) {                   // :1011
        const int k = a.obsKf[o];
        if (k == own) continue;                                      // :1013
        if (culled && ((culled[k >> 5] >> (k & 31)) & 1)) continue;  // erased by that key-frame's SetBadFlag
        if ((int)a.oct[a.octOff[k] + a.obsFeature[o]] <= ownOct + 1 && ++n > 3) return 3;   // :1030-1037
    }
    return 1;
}

__global__ __launch_bounds__(kFirstThreads) void k_cull_first(CullArgs a) {
    __shared__ int sCount[2];
    const int c = blockIdx.x, tid = threadIdx.x, i = (int)blockIdx.y * kFirstThreads + tid;
    const int4 cd = a.cands[c];
    if ((cd.w & 0xff) != 0 || (int)blockIdx.y * kFirstThreads >= cd.z) return;    // uniform for the workgroup
    if (tid < 2) sCount[tid] = 0;
    __syncthreads();
    int r = 0;
    if (i < cd.z) {
        const int p = a.rows[cd.y + i];
        if (p >= 0) r = eval_slot(a, p, cd.x, a.oct[a.octOff[cd.x] + i], nullptr);
        a.first[cd.y + i] = (uint8_t)r;
    }
    const int nm = __popcll(__ballot(r & 1)), nr = __popcll(__ballot(r & 2));
    if ((tid & 63) == 0) { atomicAdd(&sCount[0], nm); atomicAdd(&sCount[1], nr); }
    __syncthreads();
    if (tid == 0) { atomicAdd(&a.counts[c].x, sCount[0]); atomicAdd(&a.counts[c].y, sCount[1]); }
}

__global__ __launch_bounds__(kReplayThreads) void k_cull_replay(CullArgs a) {
    __shared__ uint32_t sCulled[kBitWords];
    __shared__ int sCount[2];
    const int tid = threadIdx.x;
    for (int w = tid; w < kBitWords; w += kReplayThreads) sCulled[w] = 0;
    __syncthreads();
    int4 *head = a.out + a.nUp;
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
        int nMPs, nRed;
        if (nCulled == 0) { const int2 f = a.counts[c]; nMPs = f.x; nRed = f.y; }
        else {
            if (tid < 2) sCount[tid] = 0;
            __syncthreads();
            int nm = 0, nr = 0;
            const int base = a.octOff[cd.x];
            for (int i = tid; i < cd.z; i += kReplayThreads) {
                const int p = a.rows[cd.y + i];
                if (p < 0) continue;
                const int r = (a.pts[p].w >> 8) == 0 ? a.first[cd.y + i] : eval_slot(a, p, cd.x, a.oct[base + i], sCulled);
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
                const int p = a.rows[cd.y + i];
                if (p >= 0) a.pts[p].w += 256;
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
    auto up = [](size_t b) { return (b + 15) & ~(size_t)15; };
    const size_t offPts = 0, offCand = up((size_t)n_pts * 16), offCount = offCand + (size_t)nUp * 16, offOctOff = offCount + up((size_t)nUp * 8),
                 offRows = offOctOff + up(((size_t)n_kf + 1) * 4), offObsKf = offRows + up(nRows * 4), offObsF = offObsKf + up((size_t)n_obs * 4),
                 offOct = offObsF + up((size_t)n_obs * 4), upBytes = offOct + up((size_t)nOct), blkBytes = upBytes + up(nRows);
    const size_t outBytes = ((size_t)nUp + 1) * 16 + up((size_t)nUp * 4);
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
    CullArgs a;
    a.pts = reinterpret_cast<int4 *>(h->blk.d + offPts);
    a.cands = reinterpret_cast<const int4 *>(h->blk.d + offCand);
    a.counts = reinterpret_cast<int2 *>(h->blk.d + offCount);
    a.rows = reinterpret_cast<const int32_t *>(h->blk.d + offRows);
    a.first = h->blk.d + upBytes;
    a.obsKf = reinterpret_cast<const int32_t *>(h->blk.d + offObsKf);
    a.obsFeature = reinterpret_cast<const int32_t *>(h->blk.d + offObsF);
    a.octOff = reinterpret_cast<const int32_t *>(h->blk.d + offOctOff);
    a.oct = h->blk.d + offOct;
    a.out = reinterpret_cast<int4 *>(h->out.d);
    a.nUp = nUp; a.limit = limit;
    if (maxN > 0) hipLaunchKernelGGL(k_cull_first, dim3(nUp, (maxN + kFirstThreads - 1) / kFirstThreads), dim3(kFirstThreads), 0, nullptr, a);
    hipLaunchKernelGGL(k_cull_replay, dim3(1), dim3(kReplayThreads), 0, nullptr, a);
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

extern "C" int rumi_cull_stage_ms(const RumiCull *c, float *out3) {
    if (!c || !out3) return RUMI_E_INVALID;
    std::memcpy(out3, c->stageMs, sizeof c->stageMs);
    return RUMI_OK;
}
