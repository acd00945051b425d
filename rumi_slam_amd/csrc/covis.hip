// The covisibility store (include/rumi_covis.h): KeyFrame::UpdateConnections for a batch of key-frames (R/lib_src/KeyFrame.cc:487-574) and
// Tracking::UpdateLocalKeyFrames + UpdateLocalPoints for one frame (R/lib_src/Tracking.cc:3067-3210), over tables that stay on the device.
//
// Resident state, all of it 32-bit words so that one scatter kernel applies every staged edit.  The record layout of kf, pt, attr, the row
// arena, featTab, centre and ref is covis_view.h's; what that header does not say:
//   attr   allocated with the first rumi_covis_set_point_attributes; the tracker's table gather reads it (track_local_map.inc)
//   arena  a row that outgrows its place moves to the tail; a full arena is rebuilt on the host (compacted, and doubled when the live rows
//          fill more than three quarters of it) and sent whole.  An observer entry holds the feature index GetObservations() holds, 0 where
//          the point was set without them (rumi_covis_set_points)
//   tag    [max_points]  64-bit stamps of the local-point selection, (call epoch << 32) | priority
//   rowOf  [max_points]  64-bit stamps of the same epoch for rumi_track_local_map's id -> table row map (allocated with its first call)
//   feat   the key-frames' constant part, a byte arena of its own with no host mirror (covis_features.inc)
//   centre, ref  allocated with the first rumi_covis_set_keyframe_centres / rumi_covis_set_point_reference; read by
//          rumi_refresh_map_points_resident (refresh_resident.inc) and by nothing else
//   pose, ptMap  allocated with the first rumi_covis_set_keyframe_poses / rumi_covis_set_point_maps (covis_lba.inc); read by
//          rumi_local_ba_resident (ba_resident.inc) and by nothing else
// The host keeps a mirror of kf, pt, attr and the arena; an edit writes the mirror and notes (table, offset, words).  The next query packs the noted
// ranges and its own input into one pinned block, sends it with one copy, and k_covis_apply scatters it.
//
//   k_covis_count<false>  a workgroup per batch key-frame: a lane per feature slot walks its point's observer row and counts into a histogram
//                         over slots in LDS (32-bit atomics); the non-zero slots are compacted by ballot + popcount, sorted by order_key
//                         (bitonic, slots in LDS, keys read through the cache) and written as KFcounter; the entries under the threshold are
//                         then replaced by a sentinel and the same array sorted by (weight, key) descending.
//   k_covis_count<true>   the vote of UpdateLocalKeyFrames: the same kernel with one row (the frame's points) and the observer filters off;
//                         its first wave then walks the expansion loop (:3148-3188) over an included-bitset in LDS.
//   k_covis_local<1,2,3>  UpdateLocalPoints over (rank from the end, feature) candidates: a 64-bit atomicMax of the candidate's priority on
//                         tag[point], the count of the winners per workgroup, and their write at the prefix offsets.
// Integer arithmetic only; no float atomics, and every sum is independent of arrival order.
#include <climits>
#include <cstdlib>
#include <cstring>
#include <unordered_map>
#include <vector>

#include "rumi_common.h"
#include "rumi_covis.h"
#include "covis_view.h"
#include "keyframe_features.h"
#include "opt_math.h"

namespace rumi {
namespace {

constexpr int kThreads = 256;
// short names of covis_view.h's layout for the kernels and the mirror code of this file
constexpr int KFW = kCovisKfWords, PTW = kCovisPointWords, ATW = kCovisAttrWords, CTW = kCovisCentreWords, FTW = kCovisFeatTabWords, PSW = kCovisPoseWords;
constexpr int K_MPOFF = kCovisKfMpOff, K_MPLEN = kCovisKfMpLen, K_CHOFF = kCovisKfChOff, K_CHLEN = kCovisKfChLen, K_FLAGS = kCovisKfFlags,
              K_MAP = kCovisKfMap, K_PARENT = kCovisKfParent, K_KEY = kCovisKfKey, K_BEST = kCovisKfBest;
constexpr int T_KF = 0, T_PT = 1, T_ARENA = 2, T_ATTR = 3, T_FEAT = 4, T_CENTRE = 5, T_REF = 6, T_POSE = 7, T_PTMAP = 8, kTables = 9;
constexpr uint16_t kNone = 0xFFFF;                     // sorts last; slots stay below RUMI_COVIS_MAX_KEYFRAMES
constexpr int kPosBits = 13;
static_assert((1 << kPosBits) == RUMI_COVIS_MAX_KEYFRAMES, "position bits of the packed maximum");
static_assert((1 << kCovisObsSlotBits) == RUMI_COVIS_MAX_KEYFRAMES && ((int64_t)RUMI_COVIS_MAX_FEATURES << kCovisObsSlotBits) <= (1ll << 31),
              "slot | feature << 13 is a non-negative 32-bit word");
static_assert((int64_t)RUMI_COVIS_MAX_FEATURES << kPosBits < (1ll << 31), "count << 13 | position fits 32 bits");
static_assert((int64_t)RUMI_COVIS_MAX_KEYFRAMES * RUMI_COVIS_MAX_FEATURES <= (1ll << 32), "rank * features + feature fits 32 bits");

struct CovisTables {
    const int32_t *kf, *pt, *arena;
    int hiSlot;                    // highest live slot + 1
};

struct CountArgs {
    CovisTables t;
    const int32_t *rows;           // batch slots [B], or the frame's points [nFrame]
    int nFrame;
    // update_connections
    int4 *head;                    // [B] status, first pair, KFcounter entries, ordered entries
    int2 *pairs;
    uint32_t *cursor;
    uint32_t pairsCap;
    // local_map
    int4 *lmHead;                  // K1, local key-frames, reference key-frame, local points
    uint8_t *outBad;               // [nFrame]
    int32_t *outKf;                // [hiSlot]
};

struct LocalArgs {
    CovisTables t;
    unsigned long long *tag;
    int4 *lmHead;
    const int32_t *outKf;
    int32_t *counts;               // [gridDim.x * gridDim.y]
    int32_t *outPts;
    int ptsCap;
    uint32_t epoch;
};

struct ApplyArgs {
    int32_t *base[kTables];
    const int4 *recs;              // table, first word there, first word of the payload, words
    const int32_t *payload;
};

__global__ __launch_bounds__(64) void k_covis_apply(ApplyArgs a) {
    const int4 r = a.recs[blockIdx.x];
    int32_t *dst = a.base[r.x] + r.y;
    const int32_t *src = a.payload + r.z;
    for (int i = threadIdx.x; i < r.w; i += 64) dst[i] = src[i];
}

__device__ __forceinline__ uint64_t key_of(const int32_t *kf, int s) { return *reinterpret_cast<const uint64_t *>(kf + s * KFW + K_KEY); }

template <class Before> __device__ __forceinline__ void bitonic_sort(uint16_t *a, int npad, int tid, Before before) {
    for (int k = 2; k <= npad; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < npad; i += kThreads) {
                const int l = i ^ j;
                if (l > i) {
                    const uint16_t x = a[i], y = a[l];
                    if ((i & k) == 0 ? before(y, x) : before(x, y)) { a[i] = y; a[l] = x; }
                }
            }
            __syncthreads();
        }
}

template <bool VOTE> __global__ __launch_bounds__(kThreads) void k_covis_count(CountArgs a) {
    __shared__ uint32_t sHist[RUMI_COVIS_MAX_KEYFRAMES];
    __shared__ uint16_t sIdx[RUMI_COVIS_MAX_KEYFRAMES];
    __shared__ uint32_t sIncl[RUMI_COVIS_MAX_KEYFRAMES / 32];
    __shared__ int sN, sOrd;
    __shared__ uint32_t sMax, sStart;
    const int tid = threadIdx.x, b = blockIdx.x, hi = a.t.hiSlot;
    const int32_t *kf = a.t.kf, *arena = a.t.arena;
    for (int s = tid; s < hi; s += kThreads) sHist[s] = 0;
    if (VOTE) for (int w = tid; w < RUMI_COVIS_MAX_KEYFRAMES / 32; w += kThreads) sIncl[w] = 0;
    if (tid == 0) { sN = 0; sOrd = 0; sMax = 0; }
    __syncthreads();

    // ---- the histogram: KFcounter[observer]++ (KeyFrame.cc:500-514), keyframeCounter[observer]++ (Tracking.cc:3093-3105)
    int self = -1, myMap = 0, rowLen;
    const int32_t *row;
    if (VOTE) { row = a.rows; rowLen = a.nFrame; }
    else {
        self = a.rows[b];
        const int32_t *K = kf + self * KFW;
        row = arena + K[K_MPOFF]; rowLen = K[K_MPLEN]; myMap = K[K_MAP];
    }
    for (int i = tid; i < rowLen; i += kThreads) {
        const int p = row[i];
        int bad = 0;
        if (p >= 0) {
            const int4 P = *reinterpret_cast<const int4 *>(a.t.pt + p * PTW);
            if (P.z & 1) bad = 1;
            else
                for (int o = P.x, e = P.x + P.y; o < e; o++) {
                    const int k = covis_obs_slot(arena[o]);
                    if (!VOTE) {
                        if (k == self) continue;
                        const int32_t *O = kf + k * KFW;
                        if ((O[K_FLAGS] & 1) || O[K_MAP] != myMap) continue;
                    }
                    atomicAdd(&sHist[k], 1u);
                }
        }
        if (VOTE) a.outBad[i] = (uint8_t)bad;
    }
    __syncthreads();

    // ---- the counted slots, compacted (the vote drops bad key-frames here: :3135)
    for (int base = 0; base < hi; base += kThreads) {
        const int s = base + tid;
        bool nz = s < hi && sHist[s] > 0;
        if (VOTE && nz) nz = !(kf[s * KFW + K_FLAGS] & 1);
        const unsigned long long mask = __ballot(nz);
        int wbase = 0;
        if ((tid & 63) == 0 && mask) wbase = atomicAdd(&sN, __popcll(mask));
        wbase = __shfl(wbase, 0);
        if (nz) sIdx[wbase + __popcll(mask & ((1ull << (tid & 63)) - 1ull))] = (uint16_t)s;
    }
    __syncthreads();
    const int n = sN;
    if (n == 0) {                                                    // KeyFrame.cc:519; an empty keyframeCounter
        if (tid == 0) {
            if (VOTE) *a.lmHead = make_int4(0, 0, -1, 0);
            else a.head[b] = make_int4(RUMI_COVIS_EMPTY, 0, 0, 0);
        }
        return;
    }
    int npad = 1;
    while (npad < n) npad <<= 1;
    for (int i = n + tid; i < npad; i += kThreads) sIdx[i] = kNone;
    __syncthreads();
    bitonic_sort(sIdx, npad, tid, [&](uint16_t x, uint16_t y) { return x != kNone && (y == kNone || key_of(kf, x) < key_of(kf, y)); });

    // ---- the first entry in key order with a strictly greater count (:529-532, :3137-3140), and how many reach the threshold
    for (int i = tid; i < n; i += kThreads) {
        const uint32_t c = sHist[sIdx[i]];
        atomicMax(&sMax, (c << kPosBits) | (uint32_t)(RUMI_COVIS_MAX_KEYFRAMES - 1 - i));
        if (!VOTE && c >= RUMI_COVIS_TH) atomicAdd(&sOrd, 1);
    }
    __syncthreads();
    const int nmax = (int)(sMax >> kPosBits), slotMax = sIdx[RUMI_COVIS_MAX_KEYFRAMES - 1 - (int)(sMax & (RUMI_COVIS_MAX_KEYFRAMES - 1))];

    if (!VOTE) {
        const int nOrd = sOrd > 0 ? sOrd : 1;
        if (tid == 0) sStart = atomicAdd(a.cursor, (uint32_t)(n + nOrd));
        __syncthreads();
        const uint32_t start = sStart;
        if ((uint64_t)start + (uint32_t)(n + nOrd) > a.pairsCap) {   // the host sizes the buffer for the bound; never taken
            if (tid == 0) a.head[b] = make_int4(-1, 0, 0, 0);
            return;
        }
        for (int i = tid; i < n; i += kThreads) a.pairs[start + i] = make_int2(sIdx[i], (int)sHist[sIdx[i]]);
        if (sOrd == 0) {
            if (tid == 0) a.pairs[start + n] = make_int2(slotMax, nmax);                      // :543-547
        } else {
            __syncthreads();
            for (int i = tid; i < n; i += kThreads)
                if (sHist[sIdx[i]] < RUMI_COVIS_TH) sIdx[i] = kNone;
            __syncthreads();
            // sort ascending on (weight, key), then push_front: weight descending, key descending among equal weights (:549-555)
            bitonic_sort(sIdx, npad, tid, [&](uint16_t x, uint16_t y) {
                if (x == kNone) return false;
                if (y == kNone) return true;
                const uint32_t wx = sHist[x], wy = sHist[y];
                return wx > wy || (wx == wy && key_of(kf, x) > key_of(kf, y));
            });
            for (int i = tid; i < nOrd; i += kThreads) a.pairs[start + n + i] = make_int2(sIdx[i], (int)sHist[sIdx[i]]);
        }
        if (tid == 0) a.head[b] = make_int4(RUMI_COVIS_CONNECTED, (int)start, n, nOrd);
        return;
    }

    // ---- the expansion (Tracking.cc:3148-3188): one wave, the included set as bits in LDS, the list in sIdx behind K1
    for (int i = tid; i < n; i += kThreads) atomicOr(&sIncl[sIdx[i] >> 5], 1u << (sIdx[i] & 31));
    __syncthreads();
    if (tid >= 64) return;
    const int lane = tid;
    int size = n;
    auto included = [&](int s) { return (sIncl[s >> 5] >> (s & 31)) & 1u; };
    auto is_bad = [&](int s) { return kf[s * KFW + K_FLAGS] & 1; };
    auto add = [&](int s) {                                          // uniform over the wave
        if (lane == 0) { sIdx[size] = (uint16_t)s; sIncl[s >> 5] |= 1u << (s & 31); }
        size++;
        __threadfence_block();
    };
    for (int m = 0; m < n; m++) {                                    // the end iterator is K1's (:3148)
        if (size > RUMI_COVIS_LOCAL_LIMIT) break;                    // :3150
        const int32_t *K = kf + (int)sIdx[m] * KFW;
        const int bs = lane < RUMI_COVIS_NBEST ? K[K_BEST + lane] : -1;
        const unsigned long long okBest = __ballot(bs >= 0 && !is_bad(bs) && !included(bs));
        if (okBest) add(__shfl(bs, __ffsll((long long)okBest) - 1)); // :3157-3166: the first that is not bad and not included
        uint64_t bestKey = 0;
        int bestSlot = -1;
        for (int j = lane, e = K[K_CHLEN]; j < e; j += 64) {         // :3168-3178: the first child in key order
            const int c = arena[K[K_CHOFF] + j];
            if (is_bad(c) || included(c)) continue;
            const uint64_t key = key_of(kf, c);
            if (bestSlot < 0 || key < bestKey) { bestKey = key; bestSlot = c; }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const uint32_t lo = __shfl_xor((uint32_t)bestKey, o), hi32 = __shfl_xor((uint32_t)(bestKey >> 32), o);
            const int os = __shfl_xor(bestSlot, o);
            const uint64_t ok = ((uint64_t)hi32 << 32) | lo;
            if (os >= 0 && (bestSlot < 0 || ok < bestKey)) { bestKey = ok; bestSlot = os; }
        }
        if (bestSlot >= 0) add(bestSlot);
        const int par = K[K_PARENT];
        if (par >= 0 && !included(par)) { add(par); break; }        // :3180-3187: the break leaves the loop; isBad() is not asked
    }
    for (int i = lane; i < size; i += 64) a.outKf[i] = sIdx[i];
    if (lane == 0) *a.lmHead = make_int4(n, size, slotMax, 0);
}

// UpdateLocalPoints (:3067-3087).  Workgroup (r, y): features y * 256 .. of the key-frame r places from the end of the list.
template <int PASS> __global__ __launch_bounds__(kThreads) void k_covis_local(LocalArgs a) {
    __shared__ int sWave[kThreads / 64];
    __shared__ int sPrefix;
    const int tid = threadIdx.x, r = blockIdx.x, nLocal = a.lmHead->y;
    if (r >= nLocal) return;
    const int32_t *K = a.t.kf + a.outKf[nLocal - 1 - r] * KFW;
    const int i = (int)blockIdx.y * kThreads + tid;
    int p = -1;
    if (i < K[K_MPLEN]) {
        p = a.t.arena[K[K_MPOFF] + i];
        if (p >= 0 && (a.t.pt[p * PTW + 2] & 1)) p = -1;
    }
    const unsigned long long value = ((unsigned long long)a.epoch << 32) | (0xFFFFFFFFu - ((uint32_t)r * RUMI_COVIS_MAX_FEATURES + (uint32_t)i));
    if (PASS == 1) {
        if (p >= 0) atomicMax(&a.tag[p], value);
        return;
    }
    const bool win = p >= 0 && a.tag[p] == value;
    const unsigned long long mask = __ballot(win);
    if ((tid & 63) == 0) sWave[tid >> 6] = __popcll(mask);
    const int blk = r * (int)gridDim.y + (int)blockIdx.y;
    if (PASS == 3 && tid == 0) sPrefix = 0;
    __syncthreads();
    if (PASS == 2) {
        if (tid == 0) a.counts[blk] = sWave[0] + sWave[1] + sWave[2] + sWave[3];
        return;
    }
    int part = 0;
    for (int j = tid; j < blk; j += kThreads) part += a.counts[j];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) part += __shfl_xor(part, o);
    if ((tid & 63) == 0 && part) atomicAdd(&sPrefix, part);
    __syncthreads();
    int off = sPrefix;
    for (int w = 0; w < (tid >> 6); w++) off += sWave[w];
    off += __popcll(mask & ((1ull << (tid & 63)) - 1ull));
    if (win && off < a.ptsCap) a.outPts[off] = p;
    if (tid == 0 && r == nLocal - 1 && blockIdx.y == gridDim.y - 1) a.lmHead->w = sPrefix + sWave[0] + sWave[1] + sWave[2] + sWave[3];
}

}  // namespace
}  // namespace rumi

using namespace rumi;

// The key-frame features (covis_features.inc): where each slot's block lies, the free blocks, what is staged.  No feature byte stays on the
// host once it is on the device.
struct FeatPlace { int64_t off = -1, stageOff = -1; CovisFeatRec rec{}; };       // off: in the arena; stageOff >= 0: still in the staging block
struct FeatureStore {
    std::vector<FeatPlace> place;                                // [max_kf], with the first set
    std::vector<std::pair<int64_t, int64_t>> freeList;           // (offset, bytes) ascending, neighbours merged, none touching the tail
    int64_t cap = 0, firstCap = 0, tail = 0, used = 0, slots = 0, growths = 0, compactions = 0, lastUpload = 0;
    uint8_t *stage = nullptr;                                    // ordinary memory until the store has a device, pinned from then on
    size_t stageCap = 0, stageUsed = 0;
    bool stagePinned = false;
    std::vector<std::pair<int32_t, int64_t>> staged;             // (slot, stageOff) in staging order; stale when the slot's stageOff differs
    DevBuf<uint8_t> arena;
    int64_t onDevice = 0;                                        // the device arena holds what lies below
    DevBuf<uint8_t> oct;                                         // [max_kf][octStride] keys[i].octave, device only (covis_features.inc)
    int32_t octStride = 0, maxN = 0;                             // maxN: the longest key-frame ever set
    std::vector<int32_t> octPending;                             // slots whose features changed since the table was brought up to date
    FeatureStore() = default;
    FeatureStore(const FeatureStore &) = delete;
    FeatureStore &operator=(const FeatureStore &) = delete;
    ~FeatureStore() { release_stage(); }
    void release_stage() {
        if (stage) { if (stagePinned) (void)hipHostFree(stage); else std::free(stage); }
        stage = nullptr; stageCap = 0;
    }
};

struct RumiCovis {
    DeviceBinding dev;
    FeatureStore feat;
    int32_t maxKf = 0, maxPts = 0;
    // host mirrors of the device tables
    std::vector<int32_t> kf, pt, arena, attr;        // attr: empty until the first rumi_covis_set_point_attributes
    std::vector<int32_t> featTab;                    // [max_kf][FTW]
    std::vector<int32_t> centre, ref;                // [max_kf][CTW], [max_points]: empty until their first edit
    int32_t hiRef = 0;                               // highest point id whose reference was ever set + 1
    std::vector<int32_t> pose, ptMap;                // [max_kf][PSW] (eight doubles a slot), [max_points]: empty until their first edit
    std::vector<float> pose7;                        // [max_kf][7] the floats the poses were staged from (host only)
    int32_t hiMap = 0;                               // highest point id whose map was ever set + 1
    int32_t hiAttr = 0;                              // highest point id with attributes + 1
    std::vector<int32_t> capMp, capCh, capObs;       // places of the rows in the arena (entries); 0 = never placed
    int64_t tail = 0, live = 0;
    int64_t replaced = 0, compactions = 0, growths = 0, lastUpload = 0;
    std::unordered_map<uint64_t, int32_t> keyToSlot;
    int32_t nLive = 0, hiSlot = 0, maxRow = 0;
    std::vector<int32_t> kfStamp, ptStamp;           // validation marks
    int32_t stampKf = 0, stampPt = 0;
    // staged edits
    std::vector<int4> recs;                          // table, first word, -, words
    bool full[kTables] = {true, true, true, true, true, true, true, true, true};
    // device
    DevBuf<int32_t> dKf, dPt, dArena, dAttr, dFeatTab, dCentre, dRef, dPose, dPtMap;       // dKf, dPt, dTag: with the first bind; dAttr, dRowOf: with their first use; dArena follows the mirror
    DevBuf<unsigned long long> dTag, dRowOf;
    std::vector<uint8_t> extra;                      // the input block of rumi_track_local_map: frame points and the discarded outliers
    StageClock clock;                                // of the query in flight (the local-map query is launched and read in two calls)
    uint32_t epoch = 0;
    MirrorBuf<uint8_t> stage, out;
    float stageMs[3] = {0.f, 0.f, 0.f};
};

namespace {

inline int32_t row_cap(int32_t n) { return n + (n >> 2) + 2; }

void note(RumiCovis *h, int table, int64_t off, int64_t words) {
    if (words > 0 && !h->full[table]) h->recs.push_back(make_int4(table, (int)off, 0, (int)words));
}

// Rebuilds the arena with every row at cap(len): in place when the rows and `need` more entries fill at most three quarters, else doubled.
void rebuild_arena(RumiCovis *h, int64_t need) {
    int64_t total = 0;
    for (int s = 0; s < h->hiSlot; s++) {
        if (h->capMp[s]) total += row_cap(h->kf[(size_t)s * KFW + K_MPLEN]);
        if (h->capCh[s]) total += row_cap(h->kf[(size_t)s * KFW + K_CHLEN]);
    }
    for (int p = 0; p < h->maxPts; p++)
        if (h->capObs[p]) total += row_cap(h->pt[(size_t)p * PTW + 1]);
    size_t cap = h->arena.size();
    if ((total + need) * 4 > (int64_t)cap * 3) {
        while ((total + need) * 4 > (int64_t)cap * 3) cap *= 2;
        h->growths++;
    } else h->compactions++;
    std::vector<int32_t> nv(cap, 0);
    int64_t t = 0;
    auto move = [&](int32_t &off, int32_t len, int32_t &c) {
        if (!c) return;
        if (len > 0) std::memcpy(nv.data() + t, h->arena.data() + off, (size_t)len * 4);
        off = (int32_t)t; c = row_cap(len); t += c;
    };
    for (int s = 0; s < h->hiSlot; s++) {
        int32_t *K = h->kf.data() + (size_t)s * KFW;
        move(K[K_MPOFF], K[K_MPLEN], h->capMp[s]);
        move(K[K_CHOFF], K[K_CHLEN], h->capCh[s]);
    }
    for (int p = 0; p < h->maxPts; p++) move(h->pt[(size_t)p * PTW], h->pt[(size_t)p * PTW + 1], h->capObs[p]);
    h->arena.swap(nv);
    h->tail = h->live = t;
    h->full[T_KF] = h->full[T_PT] = h->full[T_ARENA] = true;
    h->recs.erase(std::remove_if(h->recs.begin(), h->recs.end(), [](const int4 &r) { return r.x == T_KF || r.x == T_PT || r.x == T_ARENA; }), h->recs.end());
}

// Row (off, len) of place c takes src[0 .. n): in place when it fits, else at the tail.
void set_row(RumiCovis *h, int32_t &off, int32_t &len, int32_t &c, const int32_t *src, int32_t n) {
    if (n > c) {
        const int32_t nc = row_cap(n);
        if (h->tail + nc > (int64_t)h->arena.size()) rebuild_arena(h, nc);     // moves this row too, with its old contents
        if (n > c) {
            if (c) h->replaced++;
            h->live += nc - c;
            off = (int32_t)h->tail; h->tail += nc; c = nc;
        }
    }
    len = n;
    if (n > 0) std::memcpy(h->arena.data() + off, src, (size_t)n * 4);
    note(h, T_ARENA, off, n);
}

// The store's device, and with the first bind its fixed tables; bound only once they are in place.
int bind_device(RumiCovis *h) {
    bool first;
    int rc = h->dev.bind(&first);
    if (rc != RUMI_OK || !first) return rc;
    const size_t nKf = (size_t)h->maxKf * KFW, nPt = (size_t)h->maxPts * PTW, nTag = (size_t)h->maxPts, nFt = (size_t)h->maxKf * FTW;
    if ((rc = h->dKf.reserve(nKf, nKf)) != RUMI_OK || (rc = h->dFeatTab.reserve(nFt, nFt)) != RUMI_OK || (rc = h->dPt.reserve(nPt, nPt)) != RUMI_OK || (rc = h->dTag.reserve(nTag, nTag)) != RUMI_OK)
        return rc;
    HIP_TRY(hipMemsetAsync(h->dTag.p, 0, (size_t)h->maxPts * 8, nullptr));
    h->dev.bound = true;
    return RUMI_OK;
}

// Sends the staged edits and `extra` (the query's input) in one block; *dExtra is where the input lies on the device.
int flush(RumiCovis *h, const void *extra, size_t extraBytes, uint8_t **dExtra) {
    int rc;
    if ((rc = bind_device(h)) != RUMI_OK) return rc;
    if (h->recs.size() > (1u << 16)) { std::fill(h->full, h->full + kTables, true); }
    if (h->arena.size() > h->dArena.cap) {
        if ((rc = h->dArena.reserve(h->arena.size(), h->arena.size())) != RUMI_OK) return rc;
        h->full[T_ARENA] = true;
    }
    if (h->hiAttr > 0 && !h->dAttr.p) {
        if ((rc = h->dAttr.reserve((size_t)h->maxPts * ATW, (size_t)h->maxPts * ATW)) != RUMI_OK) return rc;
        h->full[T_ATTR] = true;
    }
    if (!h->centre.empty() && !h->dCentre.p) {
        if ((rc = h->dCentre.reserve(h->centre.size(), h->centre.size())) != RUMI_OK) return rc;
        h->full[T_CENTRE] = true;
    }
    if (!h->ref.empty() && !h->dRef.p) {
        if ((rc = h->dRef.reserve(h->ref.size(), h->ref.size())) != RUMI_OK) return rc;
        HIP_TRY(hipMemsetAsync(h->dRef.p, 0, h->ref.size() * 4, nullptr));     // ids above hiRef: no reference
        h->full[T_REF] = true;
    }
    if (!h->pose.empty() && !h->dPose.p) {
        if ((rc = h->dPose.reserve(h->pose.size(), h->pose.size())) != RUMI_OK) return rc;
        h->full[T_POSE] = true;
    }
    if (!h->ptMap.empty() && !h->dPtMap.p) {
        if ((rc = h->dPtMap.reserve(h->ptMap.size(), h->ptMap.size())) != RUMI_OK) return rc;
        HIP_TRY(hipMemsetAsync(h->dPtMap.p, 0, h->ptMap.size() * 4, nullptr));     // ids above hiMap: never read (no "has map" bit)
        h->full[T_PTMAP] = true;
    }
    int32_t *dBase[kTables] = {h->dKf.p, h->dPt.p, h->dArena.p, h->dAttr.p, h->dFeatTab.p, h->dCentre.p, h->dRef.p, h->dPose.p, h->dPtMap.p};
    const std::vector<int32_t> *mirror[kTables] = {&h->kf, &h->pt, &h->arena, &h->attr, &h->featTab, &h->centre, &h->ref, &h->pose, &h->ptMap};
    size_t words = 0, nRec = 0;
    for (int4 &r : h->recs)
        if (!h->full[r.x]) { r.z = (int)words; words += (size_t)r.w; h->recs[nRec++] = r; }
    h->recs.resize(nRec);
    const size_t offPay = up16(nRec * 16), offExtra = offPay + up16(words * 4), bytes = offExtra + up16(extraBytes);
    if ((rc = h->stage.reserve(bytes, bytes + bytes / 4 + 4096)) != RUMI_OK) return rc;
    h->lastUpload = (int64_t)bytes;
    for (int t = 0; t < kTables; t++)
        if (h->full[t]) {
            const size_t n = t == T_ARENA ? (size_t)h->tail : t == T_ATTR ? (size_t)h->hiAttr * ATW : t == T_REF ? (size_t)h->hiRef : t == T_PTMAP ? (size_t)h->hiMap : mirror[t]->size();
            if (n) HIP_TRY(hipMemcpyAsync(dBase[t], mirror[t]->data(), n * 4, hipMemcpyHostToDevice, nullptr));
            h->lastUpload += (int64_t)n * 4;
        }
    if (nRec) std::memcpy(h->stage.h, h->recs.data(), nRec * 16);
    int32_t *pay = reinterpret_cast<int32_t *>(h->stage.h + offPay);
    for (const int4 &r : h->recs) std::memcpy(pay + r.z, mirror[r.x]->data() + r.y, (size_t)r.w * 4);
    if (extraBytes) std::memcpy(h->stage.h + offExtra, extra, extraBytes);
    if (bytes) HIP_TRY(hipMemcpyAsync(h->stage.d, h->stage.h, bytes, hipMemcpyHostToDevice, nullptr));
    if (nRec) {
        ApplyArgs a;
        for (int t = 0; t < kTables; t++) a.base[t] = dBase[t];
        a.recs = reinterpret_cast<const int4 *>(h->stage.d);
        a.payload = reinterpret_cast<const int32_t *>(h->stage.d + offPay);
        hipLaunchKernelGGL(k_covis_apply, dim3((unsigned)nRec), dim3(64), 0, nullptr, a);
    }
    h->recs.clear();
    std::fill(h->full, h->full + kTables, false);
    *dExtra = h->stage.d + offExtra;
    return RUMI_OK;
}

inline bool is_live(const RumiCovis *h, int32_t s) { return s >= 0 && s < h->maxKf && (h->kf[(size_t)s * KFW + K_FLAGS] & kCovisKfLive); }

// Where the tables lie right now (after flush and feat_flush).
void fill_view(const RumiCovis *h, CovisView *v) {
    *v = CovisView{h->dKf.p, h->dPt.p, h->dArena.p, h->dAttr.p, h->dFeatTab.p, h->feat.arena.p, h->dCentre.p, h->dRef.p,
                   h->feat.oct.p, h->feat.octStride, h->maxKf, h->maxPts, h->dev.device, reinterpret_cast<const double *>(h->dPose.p), h->dPtMap.p};
}

}  // namespace

extern "C" int rumi_covis_create(int32_t max_kf, int32_t max_points, int64_t arena_entries, int32_t device, RumiCovis **out) {
    if (!out || max_kf <= 0 || max_points <= 0 || arena_entries < 0 || arena_entries > (1ll << 30) || max_points > (1 << 28)) {
        g_lastError = "rumi_covis_create: missing handle pointer or a size outside its range";
        return RUMI_E_INVALID;
    }
    if (max_kf > RUMI_COVIS_MAX_KEYFRAMES) {
        g_lastError = "rumi_covis_create: more than RUMI_COVIS_MAX_KEYFRAMES slots (one LDS counter each)";
        return RUMI_E_CAPACITY;
    }
    RumiCovis *h = new RumiCovis();
    h->dev.device = device; h->maxKf = max_kf; h->maxPts = max_points;
    h->kf.assign((size_t)max_kf * KFW, 0);
    h->pt.assign((size_t)max_points * PTW, 0);
    h->featTab.assign((size_t)max_kf * FTW, 0);
    for (int s = 0; s < max_kf; s++) h->featTab[(size_t)s * FTW] = h->featTab[(size_t)s * FTW + 1] = -1;
    h->arena.assign(arena_entries ? (size_t)std::max<int64_t>(arena_entries, 16) : (size_t)1 << 20, 0);
    h->capMp.assign(max_kf, 0); h->capCh.assign(max_kf, 0); h->capObs.assign(max_points, 0);
    h->kfStamp.assign(max_kf, 0); h->ptStamp.assign(max_points, 0);
    for (int s = 0; s < max_kf; s++) {
        int32_t *K = h->kf.data() + (size_t)s * KFW;
        K[K_PARENT] = -1;
        for (int j = 0; j < RUMI_COVIS_NBEST; j++) K[K_BEST + j] = -1;
    }
    *out = h;
    return RUMI_OK;
}

extern "C" void rumi_covis_destroy(RumiCovis *h) {
    if (!h) return;
    if (h->dev.bound) (void)hipSetDevice(h->dev.device);
    delete h;
}

extern "C" int rumi_covis_set_keyframes(RumiCovis *h, int32_t n, const int32_t *slots, const uint64_t *order_keys, const int32_t *map_ids,
                                        const uint8_t *is_bad, const int32_t *mp_off, const int32_t *mp, const int32_t *best,
                                        const int32_t *parent, const int32_t *child_off, const int32_t *children) {
    if (!h || n < 0 || (n > 0 && (!slots || !order_keys || !map_ids || !is_bad || !mp_off || !best || !parent || !child_off))) {
        g_lastError = "rumi_covis_set_keyframes: missing argument or negative count";
        return RUMI_E_INVALID;
    }
    if (n == 0) return RUMI_OK;
    // ---- validation, all of it before anything is staged
    if (h->stampKf > INT32_MAX - 4) { std::fill(h->kfStamp.begin(), h->kfStamp.end(), 0); h->stampKf = 0; }
    const int32_t inCall = ++h->stampKf;
    for (int i = 0; i < n; i++) {
        if (slots[i] < 0 || slots[i] >= h->maxKf || h->kfStamp[slots[i]] == inCall) {
            g_lastError = "rumi_covis_set_keyframes: a slot outside 0..max_kf-1, or named twice";
            return RUMI_E_INVALID;
        }
        h->kfStamp[slots[i]] = inCall;
    }
    {
        std::unordered_map<uint64_t, int32_t> seen;
        for (int i = 0; i < n; i++) {
            const auto it = h->keyToSlot.find(order_keys[i]);
            if (!seen.emplace(order_keys[i], slots[i]).second || (it != h->keyToSlot.end() && h->kfStamp[it->second] != inCall)) {
                g_lastError = "rumi_covis_set_keyframes: an order_key that another live slot holds";
                return RUMI_E_INVALID;
            }
        }
    }
    auto known = [&](int32_t s) { return s >= 0 && s < h->maxKf && (h->kfStamp[s] == inCall || (h->kf[(size_t)s * KFW + K_FLAGS] & 2)); };
    if (mp_off[0] < 0 || child_off[0] < 0) { g_lastError = "rumi_covis_set_keyframes: a negative offset"; return RUMI_E_INVALID; }
    int64_t need = 0;
    for (int i = 0; i < n; i++) {
        const int64_t nm = (int64_t)mp_off[i + 1] - mp_off[i], nc = (int64_t)child_off[i + 1] - child_off[i];
        if (nm < 0 || nc < 0 || nm > RUMI_COVIS_MAX_FEATURES || nc > h->maxKf || (nm > 0 && !mp) || (nc > 0 && !children)) {
            g_lastError = "rumi_covis_set_keyframes: a row slice that runs backwards, is longer than its limit, or has no array";
            return RUMI_E_INVALID;
        }
        need += row_cap((int32_t)nm) + row_cap((int32_t)nc);
        for (int64_t j = mp_off[i]; j < mp_off[i + 1]; j++)
            if (mp[j] < -1 || mp[j] >= h->maxPts) { g_lastError = "rumi_covis_set_keyframes: an mp entry outside -1..max_points-1"; return RUMI_E_INVALID; }
        for (int j = 0; j < RUMI_COVIS_NBEST; j++) {
            const int32_t b = best[(size_t)i * RUMI_COVIS_NBEST + j];
            if (b != -1 && !known(b)) { g_lastError = "rumi_covis_set_keyframes: a best entry that is neither -1 nor a live slot"; return RUMI_E_INVALID; }
        }
        if (parent[i] != -1 && (!known(parent[i]) || parent[i] == slots[i])) {
            g_lastError = "rumi_covis_set_keyframes: a parent that is neither -1 nor another live slot";
            return RUMI_E_INVALID;
        }
    }
    {   // children: distinct live slots, never the key-frame itself
        std::vector<int32_t> mark(h->maxKf, -1);
        for (int i = 0; i < n; i++)
            for (int64_t j = child_off[i]; j < child_off[i + 1]; j++) {
                const int32_t c = children[j];
                if (!known(c) || c == slots[i] || mark[c] == i) {
                    g_lastError = "rumi_covis_set_keyframes: a child that is not a live slot, is the key-frame itself, or is listed twice";
                    return RUMI_E_INVALID;
                }
                mark[c] = i;
            }
    }
    if (h->live + need > (1ll << 29)) { g_lastError = "rumi_covis_set_keyframes: the row arena would pass 2^29 entries"; return RUMI_E_CAPACITY; }
    // ---- apply to the mirror, note what changed
    for (int i = 0; i < n; i++) {
        const int32_t *K = h->kf.data() + (size_t)slots[i] * KFW;
        if (K[K_FLAGS] & 2) { uint64_t old; std::memcpy(&old, K + K_KEY, 8); h->keyToSlot.erase(old); }
    }
    for (int i = 0; i < n; i++) {
        const int32_t s = slots[i];
        int32_t *K = h->kf.data() + (size_t)s * KFW;
        if (!(K[K_FLAGS] & 2)) { h->nLive++; h->hiSlot = std::max(h->hiSlot, s + 1); }
        K[K_FLAGS] = 2 | (is_bad[i] ? 1 : 0);
        const int32_t nm = mp_off[i + 1] - mp_off[i], nc = child_off[i + 1] - child_off[i];
        // set_row works on the mirror's own words: a rebuild of the arena rewrites the offsets there
        set_row(h, K[K_MPOFF], K[K_MPLEN], h->capMp[s], nm ? mp + mp_off[i] : nullptr, nm);
        set_row(h, K[K_CHOFF], K[K_CHLEN], h->capCh[s], nc ? children + child_off[i] : nullptr, nc);
        K[K_MAP] = map_ids[i];
        K[K_PARENT] = parent[i];
        std::memcpy(K + K_KEY, &order_keys[i], 8);
        std::memcpy(K + K_BEST, best + (size_t)i * RUMI_COVIS_NBEST, RUMI_COVIS_NBEST * 4);
        h->keyToSlot[order_keys[i]] = s;
        h->maxRow = std::max(h->maxRow, nm);
        note(h, T_KF, (int64_t)s * KFW, KFW);
    }
    return RUMI_OK;
}

// rumi_covis_set_points (obs_feature null) and rumi_covis_set_point_observations: one validation, one staging.
static int set_points_impl(RumiCovis *h, const char *entry, int32_t n, const int32_t *ids, const uint8_t *is_bad, const int32_t *obs_off, const int32_t *obs,
                           const int32_t *obs_feature, bool withFeatures) {
    const std::string E(entry);
    if (!h || n < 0 || (n > 0 && (!ids || !is_bad || !obs_off))) {
        g_lastError = E + ": missing argument or negative count";
        return RUMI_E_INVALID;
    }
    if (n == 0) return RUMI_OK;
    if (h->stampPt > INT32_MAX - 4) { std::fill(h->ptStamp.begin(), h->ptStamp.end(), 0); h->stampPt = 0; }
    const int32_t inCall = ++h->stampPt;
    for (int i = 0; i < n; i++) {
        if (ids[i] < 0 || ids[i] >= h->maxPts || h->ptStamp[ids[i]] == inCall) {
            g_lastError = E + ": a point id outside 0..max_points-1, or named twice";
            return RUMI_E_INVALID;
        }
        h->ptStamp[ids[i]] = inCall;
    }
    if (obs_off[0] < 0) { g_lastError = E + ": a negative offset"; return RUMI_E_INVALID; }
    int64_t need = 0;
    int32_t longest = 0;
    std::vector<int32_t> mark(h->maxKf, -1);
    for (int i = 0; i < n; i++) {
        const int64_t no = (int64_t)obs_off[i + 1] - obs_off[i];
        if (no < 0 || no > h->maxKf || (no > 0 && (!obs || (withFeatures && !obs_feature)))) {
            g_lastError = E + ": an observer slice that runs backwards, is longer than max_kf, or has no array";
            return RUMI_E_INVALID;
        }
        need += row_cap((int32_t)no);
        longest = std::max(longest, (int32_t)no);
        for (int64_t j = obs_off[i]; j < obs_off[i + 1]; j++) {
            if (!is_live(h, obs[j]) || mark[obs[j]] == i) {
                g_lastError = E + ": an observer that is not a live slot, or is listed twice";
                return RUMI_E_INVALID;
            }
            mark[obs[j]] = i;
            if (withFeatures && (obs_feature[j] < 0 || obs_feature[j] >= RUMI_COVIS_MAX_FEATURES)) {
                g_lastError = E + ": a feature index outside 0..RUMI_COVIS_MAX_FEATURES-1";
                return RUMI_E_INVALID;
            }
        }
    }
    if (h->live + need > (1ll << 29)) { g_lastError = E + ": the row arena would pass 2^29 entries"; return RUMI_E_CAPACITY; }
    std::vector<int32_t> packed;
    if (withFeatures) packed.resize((size_t)longest);
    for (int i = 0; i < n; i++) {
        const int32_t p = ids[i], no = obs_off[i + 1] - obs_off[i];
        const int32_t *src = no ? obs + obs_off[i] : nullptr;
        if (withFeatures && no) {
            for (int j = 0; j < no; j++) packed[j] = src[j] | (obs_feature[obs_off[i] + j] << kCovisObsSlotBits);
            src = packed.data();
        }
        set_row(h, h->pt[(size_t)p * PTW], h->pt[(size_t)p * PTW + 1], h->capObs[p], src, no);
        h->pt[(size_t)p * PTW + 2] = (is_bad[i] ? 1 : 0) | (withFeatures ? kCovisPointHasObsFeatures : 0) | (h->pt[(size_t)p * PTW + 2] & kCovisPointHasMap);
        note(h, T_PT, (int64_t)p * PTW, PTW);
    }
    return RUMI_OK;
}

extern "C" int rumi_covis_set_points(RumiCovis *h, int32_t n, const int32_t *ids, const uint8_t *is_bad, const int32_t *obs_off, const int32_t *obs) {
    return set_points_impl(h, "rumi_covis_set_points", n, ids, is_bad, obs_off, obs, nullptr, false);
}

extern "C" int rumi_covis_set_point_observations(RumiCovis *h, int32_t n, const int32_t *ids, const uint8_t *is_bad, const int32_t *obs_off,
                                                 const int32_t *obs_slot, const int32_t *obs_feature) {
    return set_points_impl(h, "rumi_covis_set_point_observations", n, ids, is_bad, obs_off, obs_slot, obs_feature, true);
}

extern "C" int rumi_covis_set_bad(RumiCovis *h, int32_t n_kf, const int32_t *slots, const uint8_t *kf_bad, int32_t n_pt, const int32_t *ids,
                                  const uint8_t *pt_bad) {
    if (!h || n_kf < 0 || n_pt < 0 || (n_kf > 0 && (!slots || !kf_bad)) || (n_pt > 0 && (!ids || !pt_bad))) {
        g_lastError = "rumi_covis_set_bad: missing argument or negative count";
        return RUMI_E_INVALID;
    }
    for (int i = 0; i < n_kf; i++)
        if (!is_live(h, slots[i])) { g_lastError = "rumi_covis_set_bad: a key-frame slot that is not live"; return RUMI_E_INVALID; }
    for (int i = 0; i < n_pt; i++)
        if (ids[i] < 0 || ids[i] >= h->maxPts) { g_lastError = "rumi_covis_set_bad: a point id outside 0..max_points-1"; return RUMI_E_INVALID; }
    for (int i = 0; i < n_kf; i++) {
        h->kf[(size_t)slots[i] * KFW + K_FLAGS] = 2 | (kf_bad[i] ? 1 : 0);
        note(h, T_KF, (int64_t)slots[i] * KFW + K_FLAGS, 1);
    }
    for (int i = 0; i < n_pt; i++) {
        int32_t &f = h->pt[(size_t)ids[i] * PTW + 2];
        f = (f & ~1) | (pt_bad[i] ? 1 : 0);
        note(h, T_PT, (int64_t)ids[i] * PTW + 2, 1);
    }
    return RUMI_OK;
}

extern "C" int rumi_covis_set_maps(RumiCovis *h, int32_t n, const int32_t *slots, const int32_t *map_ids) {
    if (!h || n < 0 || (n > 0 && (!slots || !map_ids))) {
        g_lastError = "rumi_covis_set_maps: missing argument or negative count";
        return RUMI_E_INVALID;
    }
    for (int i = 0; i < n; i++)
        if (!is_live(h, slots[i])) { g_lastError = "rumi_covis_set_maps: a key-frame slot that is not live"; return RUMI_E_INVALID; }
    for (int i = 0; i < n; i++) {
        h->kf[(size_t)slots[i] * KFW + K_MAP] = map_ids[i];
        note(h, T_KF, (int64_t)slots[i] * KFW + K_MAP, 1);
    }
    return RUMI_OK;
}

extern "C" int rumi_covis_set_point_attributes(RumiCovis *h, int32_t n, const int32_t *ids, const float *pos, const float *normal, const float *min_dist,
                                               const float *max_dist, const uint8_t *desc) {
    if (!h || n < 0 || (n > 0 && (!ids || !pos || !normal || !min_dist || !max_dist || !desc))) {
        g_lastError = "rumi_covis_set_point_attributes: missing argument or negative count";
        return RUMI_E_INVALID;
    }
    if (n == 0) return RUMI_OK;
    if (h->maxPts > (1 << 26)) {                                     // a staged edit addresses its table by a 32-bit word offset
        g_lastError = "rumi_covis_set_point_attributes: the attribute table holds at most 2^26 points";
        return RUMI_E_CAPACITY;
    }
    if (h->stampPt > INT32_MAX - 4) { std::fill(h->ptStamp.begin(), h->ptStamp.end(), 0); h->stampPt = 0; }
    const int32_t inCall = ++h->stampPt;
    for (int i = 0; i < n; i++) {
        if (ids[i] < 0 || ids[i] >= h->maxPts || h->ptStamp[ids[i]] == inCall) {
            g_lastError = "rumi_covis_set_point_attributes: a point id outside 0..max_points-1, or named twice";
            return RUMI_E_INVALID;
        }
        h->ptStamp[ids[i]] = inCall;
    }
    if (h->attr.empty()) h->attr.assign((size_t)h->maxPts * ATW, 0);
    for (int i = 0; i < n; i++) {
        const int32_t p = ids[i];
        int32_t *A = h->attr.data() + (size_t)p * ATW;
        std::memcpy(A, pos + (size_t)i * 3, 12); std::memcpy(A + 3, normal + (size_t)i * 3, 12);
        std::memcpy(A + 6, min_dist + i, 4); std::memcpy(A + 7, max_dist + i, 4);
        std::memcpy(A + 8, desc + (size_t)i * 32, 32);
        h->hiAttr = std::max(h->hiAttr, p + 1);
        note(h, T_ATTR, (int64_t)p * ATW, ATW);
        if (!h->pt[(size_t)p * PTW + 3]) { h->pt[(size_t)p * PTW + 3] = 1; note(h, T_PT, (int64_t)p * PTW + 3, 1); }
    }
    return RUMI_OK;
}

extern "C" int rumi_covis_update_connections(RumiCovis *h, int32_t B, const int32_t *batch, int32_t *status, int32_t *conn_off, int32_t *conn_slot,
                                             int32_t *conn_count, int64_t conn_cap, int32_t *ord_off, int32_t *ord_slot, int32_t *ord_weight,
                                             int64_t ord_cap) {
    if (!h || B < 0 || conn_cap < 0 || ord_cap < 0 || !conn_off || !ord_off || (B > 0 && (!batch || !status)) ||
        (conn_cap > 0 && (!conn_slot || !conn_count)) || (ord_cap > 0 && (!ord_slot || !ord_weight))) {
        g_lastError = "rumi_covis_update_connections: missing argument or negative count";
        return RUMI_E_INVALID;
    }
    h->clock.start();
    for (int b = 0; b < B; b++)
        if (!is_live(h, batch[b])) { g_lastError = "rumi_covis_update_connections: a batch entry that is not a live slot"; return RUMI_E_INVALID; }
    if (B == 0) { conn_off[0] = ord_off[0] = 0; return RUMI_OK; }
    const uint64_t pairsCap = (uint64_t)B * 2u * (uint64_t)h->nLive;            // KFcounter and the ordered list hold at most every live slot
    if (pairsCap * 8 > (1ull << 30)) {
        g_lastError = "rumi_covis_update_connections: the batch times the live key-frames passes the result buffer (1 GiB); split the batch";
        return RUMI_E_CAPACITY;
    }
    int rc;
    uint8_t *dBatch = nullptr;
    if ((rc = flush(h, batch, (size_t)B * 4, &dBatch)) != RUMI_OK) return rc;
    const size_t offHead = 16, offPairs = offHead + (size_t)B * 16, outBytes = offPairs + (size_t)pairsCap * 8;
    if ((rc = h->out.reserve(outBytes, outBytes + outBytes / 4)) != RUMI_OK) return rc;
    h->clock.mark();
    HIP_TRY(hipMemsetAsync(h->out.d, 0, 16, nullptr));
    CountArgs a{};
    a.t = CovisTables{h->dKf.p, h->dPt.p, h->dArena.p, h->hiSlot};
    a.rows = reinterpret_cast<const int32_t *>(dBatch);
    a.head = reinterpret_cast<int4 *>(h->out.d + offHead);
    a.pairs = reinterpret_cast<int2 *>(h->out.d + offPairs);
    a.cursor = reinterpret_cast<uint32_t *>(h->out.d);
    a.pairsCap = (uint32_t)pairsCap;
    hipLaunchKernelGGL(k_covis_count<false>, dim3(B), dim3(kThreads), 0, nullptr, a);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(h->out.h, h->out.d, offPairs, hipMemcpyDeviceToHost));
    const uint32_t used = *reinterpret_cast<const uint32_t *>(h->out.h);
    const int4 *head = reinterpret_cast<const int4 *>(h->out.h + offHead);
    int64_t nConn = 0, nOrd = 0;
    for (int b = 0; b < B; b++) {
        if (head[b].x < 0 || used > pairsCap) { g_lastError = "rumi_covis_update_connections: the result buffer overflowed (internal error)"; return RUMI_E_INVALID; }
        nConn += head[b].z; nOrd += head[b].w;
    }
    if (nConn > conn_cap || nOrd > ord_cap || nConn > INT32_MAX) {
        g_lastError = "rumi_covis_update_connections: conn_cap or ord_cap is too small for the lists";
        return RUMI_E_CAPACITY;
    }
    if (used) HIP_TRY(hipMemcpy(h->out.h + offPairs, h->out.d + offPairs, (size_t)used * 8, hipMemcpyDeviceToHost));
    h->clock.mark();
    const int2 *pairs = reinterpret_cast<const int2 *>(h->out.h + offPairs);
    int32_t co = 0, oo = 0;
    for (int b = 0; b < B; b++) {
        status[b] = head[b].x;
        conn_off[b] = co; ord_off[b] = oo;
        const int2 *src = pairs + head[b].y;
        for (int i = 0; i < head[b].z; i++) { conn_slot[co] = src[i].x; conn_count[co++] = src[i].y; }
        src += head[b].z;
        for (int i = 0; i < head[b].w; i++) { ord_slot[oo] = src[i].x; ord_weight[oo++] = src[i].y; }
    }
    conn_off[B] = co; ord_off[B] = oo;
    h->clock.finish(h->stageMs);
    return RUMI_OK;
}

// The launch sequence of Tracking::UpdateLocalMap, nothing read back: k_covis_count<true>, k_covis_local<1..3>.  With `d` (rumi_track_local_map)
// the discarded outliers travel in the same block behind the frame's points, and the second header is cleared for the table kernels.
int rumi::covis_local_map_launch(RumiCovis *h, int n, const int32_t *frame_points, const CovisDiscarded *d, int wantDevice, const char *entry,
                                 CovisLocalView *view) {
    h->clock.start();
    if (n < 0 || n > RUMI_COVIS_MAX_FEATURES || (n > 0 && !frame_points)) {
        g_lastError = std::string(entry) + ": missing argument, negative count, or more than RUMI_COVIS_MAX_FEATURES frame points";
        return RUMI_E_INVALID;
    }
    for (int i = 0; i < n; i++)
        if (frame_points[i] < -1 || frame_points[i] >= h->maxPts) {
            g_lastError = std::string(entry) + ": a frame point outside -1..max_points-1";
            return RUMI_E_INVALID;
        }
    const int nd = d ? d->n : 0;
    const bool stale = d && d->inView && d->proj5;
    if (d) {
        if (nd < 0 || nd > RUMI_COVIS_MAX_FEATURES || (nd > 0 && !d->ids)) {
            g_lastError = std::string(entry) + ": missing discarded ids, negative count, or more than RUMI_COVIS_MAX_FEATURES of them";
            return RUMI_E_INVALID;
        }
        if (h->stampPt > INT32_MAX - 4) { std::fill(h->ptStamp.begin(), h->ptStamp.end(), 0); h->stampPt = 0; }
        const int32_t inCall = ++h->stampPt;
        for (int k = 0; k < nd; k++) {
            if (d->ids[k] < 0 || d->ids[k] >= h->maxPts || h->ptStamp[d->ids[k]] == inCall) {
                g_lastError = std::string(entry) + ": a discarded id outside 0..max_points-1, or named twice";
                return RUMI_E_INVALID;
            }
            h->ptStamp[d->ids[k]] = inCall;
        }
    }
    int rc;
    if ((rc = covis_same_device(h, wantDevice, entry)) != RUMI_OK) return rc;
    // the input block: frame points | discarded ids | their mbTrackInView | their projections, each part 16-byte aligned
    const size_t offIds = up16((size_t)n * 4), offIn = offIds + up16((size_t)nd * 4), offProj = offIn + up16(stale ? (size_t)nd : 0),
                 inBytes = d ? offProj + (stale ? (size_t)nd * 20 : 0) : (size_t)n * 4;
    const void *in = frame_points;
    if (d) {
        h->extra.assign(inBytes, 0);
        if (n > 0) std::memcpy(h->extra.data(), frame_points, (size_t)n * 4);
        if (nd > 0) std::memcpy(h->extra.data() + offIds, d->ids, (size_t)nd * 4);
        if (stale && nd > 0) { std::memcpy(h->extra.data() + offIn, d->inView, (size_t)nd); std::memcpy(h->extra.data() + offProj, d->proj5, (size_t)nd * 20); }
        in = h->extra.data();
    }
    uint8_t *dFrame = nullptr;
    if ((rc = flush(h, in, inBytes, &dFrame)) != RUMI_OK) return rc;
    const int gx = h->nLive, gy = (h->maxRow + kThreads - 1) / kThreads;
    const size_t offBad = 2 * 16, offKf = offBad + up16((size_t)n), offCounts = offKf + up16((size_t)h->hiSlot * 4),
                 offPts = offCounts + up16((size_t)gx * gy * 4), outBytes = offPts + (size_t)h->maxPts * 4;
    if ((rc = h->out.reserve(outBytes, outBytes + outBytes / 4)) != RUMI_OK) return rc;
    bool clearStamps = ++h->epoch == 0;                              // once every 2^32 calls: stale tags could meet a reused epoch
    if (d && !h->dRowOf.p) {
        if ((rc = h->dRowOf.reserve((size_t)h->maxPts, (size_t)h->maxPts)) != RUMI_OK) return rc;
        clearStamps = true;
    }
    if (clearStamps) {
        if (h->epoch == 0) { HIP_TRY(hipMemsetAsync(h->dTag.p, 0, (size_t)h->maxPts * 8, nullptr)); h->epoch = 1; }
        if (h->dRowOf.p) HIP_TRY(hipMemsetAsync(h->dRowOf.p, 0, (size_t)h->maxPts * 8, nullptr));
    }
    if (d) HIP_TRY(hipMemsetAsync(h->out.d + 16, 0, 16, nullptr));
    h->clock.mark();
    CountArgs a{};
    a.t = CovisTables{h->dKf.p, h->dPt.p, h->dArena.p, h->hiSlot};
    a.rows = reinterpret_cast<const int32_t *>(dFrame);
    a.nFrame = n;
    a.lmHead = reinterpret_cast<int4 *>(h->out.d);
    a.outBad = h->out.d + offBad;
    a.outKf = reinterpret_cast<int32_t *>(h->out.d + offKf);
    hipLaunchKernelGGL(k_covis_count<true>, dim3(1), dim3(kThreads), 0, nullptr, a);
    if (gx > 0 && gy > 0) {
        LocalArgs l{};
        l.t = a.t;
        l.tag = h->dTag.p;
        l.lmHead = a.lmHead;
        l.outKf = a.outKf;
        l.counts = reinterpret_cast<int32_t *>(h->out.d + offCounts);
        l.outPts = reinterpret_cast<int32_t *>(h->out.d + offPts);
        l.ptsCap = h->maxPts;
        l.epoch = h->epoch;
        hipLaunchKernelGGL(k_covis_local<1>, dim3(gx, gy), dim3(kThreads), 0, nullptr, l);
        hipLaunchKernelGGL(k_covis_local<2>, dim3(gx, gy), dim3(kThreads), 0, nullptr, l);
        hipLaunchKernelGGL(k_covis_local<3>, dim3(gx, gy), dim3(kThreads), 0, nullptr, l);
    }
    HIP_TRY(hipGetLastError());
    CovisLocalView &v = *view;
    v = CovisLocalView{};
    fill_view(h, &v.t);
    v.nFrame = n; v.nDiscarded = nd; v.epoch = h->epoch;
    v.rowOf = h->dRowOf.p;
    v.head = reinterpret_cast<int32_t *>(h->out.d);
    v.localPts = reinterpret_cast<const int32_t *>(h->out.d + offPts);
    v.framePts = reinterpret_cast<const int32_t *>(dFrame);
    if (d) {
        v.discIds = reinterpret_cast<const int32_t *>(dFrame + offIds);
        if (stale) { v.discInView = dFrame + offIn; v.discProj = reinterpret_cast<const float *>(dFrame + offProj); }
    }
    v.offBad = offBad; v.offKf = offKf; v.offPts = offPts; v.headBytes = offCounts;
    return RUMI_OK;
}

// The one read in the middle of the query: both headers, the frame's bad flags and the local key-frames, into the pinned block.
int rumi::covis_local_map_read(RumiCovis *h, const CovisLocalView &v, const int32_t **head8, const uint8_t **frameBad, const int32_t **localKf) {
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(h->out.h, h->out.d, v.headBytes, hipMemcpyDeviceToHost));
    *head8 = reinterpret_cast<const int32_t *>(h->out.h);
    *frameBad = h->out.h + v.offBad;
    *localKf = reinterpret_cast<const int32_t *>(h->out.h + v.offKf);
    h->clock.mark();
    h->clock.finish(h->stageMs);
    return RUMI_OK;
}

extern "C" int rumi_covis_local_map(RumiCovis *h, int32_t n, const int32_t *frame_points, uint8_t *frame_point_bad, int32_t *local_kf, int32_t kf_cap,
                                    int32_t *n_k1, int32_t *n_local_kf, int32_t *ref_kf, int32_t *local_points, int32_t pt_cap,
                                    int32_t *n_local_points) {
    if (!h || n < 0 || n > RUMI_COVIS_MAX_FEATURES || kf_cap < 0 || pt_cap < 0 || !n_k1 || !n_local_kf || !ref_kf || !n_local_points ||
        (n > 0 && (!frame_points || !frame_point_bad)) || (kf_cap > 0 && !local_kf) || (pt_cap > 0 && !local_points)) {
        g_lastError = "rumi_covis_local_map: missing argument, negative count, or more than RUMI_COVIS_MAX_FEATURES frame points";
        return RUMI_E_INVALID;
    }
    int rc;
    CovisLocalView v;
    const int32_t *head, *kfs;
    const uint8_t *bad;
    if ((rc = covis_local_map_launch(h, n, frame_points, nullptr, -1, "rumi_covis_local_map", &v)) != RUMI_OK) return rc;
    if ((rc = covis_local_map_read(h, v, &head, &bad, &kfs)) != RUMI_OK) return rc;
    if (head[1] > kf_cap || head[3] > pt_cap) {
        g_lastError = "rumi_covis_local_map: kf_cap or pt_cap is too small for the lists";
        return RUMI_E_CAPACITY;
    }
    if (head[3] > 0) HIP_TRY(hipMemcpy(h->out.h + v.offPts, h->out.d + v.offPts, (size_t)head[3] * 4, hipMemcpyDeviceToHost));
    h->clock.mark();                                                 // the list is part of the device stage
    if (n > 0) std::memcpy(frame_point_bad, bad, (size_t)n);
    if (head[1] > 0) std::memcpy(local_kf, kfs, (size_t)head[1] * 4);
    if (head[3] > 0) std::memcpy(local_points, h->out.h + v.offPts, (size_t)head[3] * 4);
    *n_k1 = head[0]; *n_local_kf = head[1]; *ref_kf = head[2]; *n_local_points = head[3];
    h->clock.finish(h->stageMs);
    return RUMI_OK;
}

#include "covis_features.inc"
#include "covis_refresh.inc"
#include "covis_lba.inc"

extern "C" int rumi_covis_stage_ms(const RumiCovis *h, float *out3) {
    if (!h || !out3) return RUMI_E_INVALID;
    std::memcpy(out3, h->stageMs, sizeof h->stageMs);
    return RUMI_OK;
}

extern "C" int rumi_covis_stats(const RumiCovis *h, int64_t *out7) {
    if (!h || !out7) return RUMI_E_INVALID;
    const int64_t v[7] = {(int64_t)h->arena.size(), h->tail, h->live, h->replaced, h->compactions, h->growths, h->lastUpload};
    std::memcpy(out7, v, sizeof v);
    return RUMI_OK;
}
