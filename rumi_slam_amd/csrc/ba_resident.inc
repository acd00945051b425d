// ba_resident.inc -- the window of Optimizer::LocalBundleAdjustment (R/lib_src/Optimizer.cc:1003-1271, monocular branch) assembled on the device
// from the covisibility store (covis_view.h): the kernels of rumi_local_ba_resident.  Host: ba_resident_host.inc.  Included by opt.hip.
//
// The host decides lLocalKeyFrames from the store's mirror (covis_lba_window) and sends them with a role per slot; everything else is read where
// it lies.  All orders are the reference's, and every one of them is decided by integers:
//   k_lba_points<1..3>  lLocalMapPoints (:1023-1039): a workgroup per (local key-frame, 256 features).  <1> a 64-bit atomicMax of
//                       epoch << 32 | ~(rank * RUMI_COVIS_MAX_FEATURES + feature) on the point's stamp keeps the first occurrence, <2> counts the
//                       winners per workgroup, <3> writes them at the prefix of the counts: list order, feature order.  <1> also counts what the
//                       call refuses: a row point that was never given a map, a local key-frame without pose or features.
//   k_lba_observers     a wave per listed point over its observer row.  The rank of an observer is its place in ascending order_key (std::map
//                       order, whatever order the row was given in).  An observer that is neither bad nor of another map gives an edge; if it
//                       is not local either, a 64-bit atomicMin of (point position << 13 | rank) on its slot keeps its first appearance in the
//                       walk of :1042-1055.  Counts the edges of the point, and the observations that disagree with their slot's row.
//   k_lba_scan          one workgroup: the fixed cameras ordered by that word (the rank of a slot is the number of smaller words), the index
//                       of every slot in the key-frame list, and the exclusive prefix of the edge counts (ptStart).
//   k_lba_fill_kf, k_lba_fill_edges   the raw block of the window-batched solver (ba_windows_host.inc: rawT, poseCol, rawX, rawMP, rawKF, rawObs,
//                       rawInfo) at the offsets baw_stage computes: an edge lies at ptStart[point] + its rank among the point's edge-giving
//                       observers, so e_mp is grouped and ascending as the reference builds it.
//   k_lba_commit        after a run: the new positions into the store's attribute records, and the erased observations compacted in edge
//                       order (one workgroup, ballot prefixes) as {slot, point id, feature}.
// Nothing is accumulated in floating point; two runs on the same state leave the same bytes.

enum { LBA_H_NMP = 0, LBA_H_NFIXED = 1, LBA_H_NE = 2, LBA_H_NERASED = 3, LBA_V_NO_MAP = 4, LBA_V_OBS_MISMATCH = 5, LBA_V_KF_NO_POSE = 6, LBA_V_KF_NO_FEATURES = 7,
       LBA_V_NO_ATTR = 8, LBA_V_NO_OBS_FEATURES = 9, LBA_HEAD_WORDS = 16 };
constexpr int kLbaRankBits = 13;
static_assert((1 << kLbaRankBits) == RUMI_COVIS_MAX_KEYFRAMES, "an observer row holds at most every slot: its ranks fit 13 bits");
constexpr unsigned long long kLbaNever = ~0ull;

struct LbaArgs {
    CovisView v;
    const int32_t *locals;                 // [nLocal] lLocalKeyFrames as slots
    const int32_t *role;                   // [hiSlot] index in locals, -1 every other slot
    int nLocal, hiSlot, curMap, initIdx, ptCap;
    uint32_t epoch;
    unsigned long long *ptTag;             // [max_points] stamps of the first occurrence
    int32_t *blkCnt;                       // [nLocal * gridDim.y]
    int32_t *head;                         // [LBA_HEAD_WORDS]
    int32_t *kfList;                       // [nLocal + hiSlot]: lLocalKeyFrames, then lFixedCameras
    int32_t *ptList;                       // [ptCap] lLocalMapPoints as ids
    int32_t *edgeCnt, *ptStart;            // [ptCap], [ptCap + 1]
    unsigned long long *fixTag;            // [hiSlot]
    int32_t *kfIndex;                      // [hiSlot] index in kfList, -1 none
};

struct LbaRaw {                            // the raw block of one window (BAWin's raw* members) and what the erase list needs of every edge
    double *rawT; float *rawX; int32_t *poseCol, *rawMP, *rawKF; float *rawObs, *rawInfo;
    int32_t *edgeObs, *edgePt;             // [nE] the observer word (slot | feature << 13) the edge was made from, and its point's id: these
                                           // outlive the raw block, which the single-window host loop overwrites with its own upload
};

// :1028-1038: is row entry p a local map point?  *noMap: a live point of the row that was never given a map.
__device__ __forceinline__ bool lba_takes(const LbaArgs &a, int p, bool *noMap) {
    *noMap = false;
    if (p < 0) return false;
    const CovisPoint P = a.v.point(p);
    if (P.bad()) return false;
    if (!P.has_map()) { *noMap = true; return false; }
    return a.v.point_map(p) == a.curMap;
}

template <int PASS> __global__ __launch_bounds__(256) void k_lba_points(LbaArgs a) {
    __shared__ int sWave[4];
    __shared__ int sPrefix;
    const int tid = threadIdx.x, r = blockIdx.x;
    const int slot = a.locals[r];
    const int i = (int)blockIdx.y * 256 + tid;
    int p = -1;
    bool noMap = false;
    if (i < a.v.kf_row_len(slot)) {
        p = a.v.kf_row_entry(slot, i);
        if (!lba_takes(a, p, &noMap)) p = -1;
    }
    const unsigned long long value = ((unsigned long long)a.epoch << 32) | (0xFFFFFFFFu - ((uint32_t)r * RUMI_COVIS_MAX_FEATURES + (uint32_t)i));
    if (PASS == 1) {
        if (p >= 0) atomicMax(&a.ptTag[p], value);
        if (noMap) atomicAdd(&a.head[LBA_V_NO_MAP], 1);
        if (tid == 0 && blockIdx.y == 0) {
            if (!a.v.has_pose(slot)) atomicAdd(&a.head[LBA_V_KF_NO_POSE], 1);
            if (!a.v.featTab || a.v.feat_keys(slot) < 0 || a.v.feat_count(slot) != a.v.kf_row_len(slot)) atomicAdd(&a.head[LBA_V_KF_NO_FEATURES], 1);
        }
        return;
    }
    const bool win = p >= 0 && a.ptTag[p] == value;
    const unsigned long long mask = __ballot(win);
    if ((tid & 63) == 0) sWave[tid >> 6] = __popcll(mask);
    const int blk = r * (int)gridDim.y + (int)blockIdx.y;
    if (PASS == 3 && tid == 0) sPrefix = 0;
    __syncthreads();
    if (PASS == 2) {
        if (tid == 0) a.blkCnt[blk] = sWave[0] + sWave[1] + sWave[2] + sWave[3];
        return;
    }
    int part = 0;
    for (int j = tid; j < blk; j += 256) part += a.blkCnt[j];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) part += __shfl_xor(part, o);
    if ((tid & 63) == 0 && part) atomicAdd(&sPrefix, part);
    __syncthreads();
    int off = sPrefix;
    for (int w = 0; w < (tid >> 6); w++) off += sWave[w];
    off += __popcll(mask & ((1ull << (tid & 63)) - 1ull));
    if (win && off < a.ptCap) a.ptList[off] = p;
    if (tid == 0 && r == a.nLocal - 1 && blockIdx.y == gridDim.y - 1) a.head[LBA_H_NMP] = sPrefix + sWave[0] + sWave[1] + sWave[2] + sWave[3];
}

// :1050 / :1171: the observer gives an edge (and, where it is not local, a fixed camera)
__device__ __forceinline__ bool lba_observer_ok(const CovisView &v, int slot, int curMap) { return !v.kf_bad(slot) && v.kf_map(slot) == curMap; }

__global__ __launch_bounds__(256) void k_lba_observers(LbaArgs a) {
    const int lane = threadIdx.x & 63, i = (int)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int nMP = min(a.head[LBA_H_NMP], a.ptCap);
    if (i >= nMP) return;
    const int p = a.ptList[i];
    const CovisPoint P = a.v.point(p);
    const int L = P.obs_len();
    const int32_t *row = a.v.rows + P.obs_off();
    if (lane == 0) {
        if (L > 0 && !P.has_obs_features()) atomicAdd(&a.head[LBA_V_NO_OBS_FEATURES], 1);
        if (!a.v.has_attr(P)) atomicAdd(&a.head[LBA_V_NO_ATTR], 1);
    }
    int edges = 0;
    for (int k0 = 0; k0 < L; k0 += 64) {
        const int k = k0 + lane;
        bool ok = false;
        if (k < L) {
            const int word = row[k], s = covis_obs_slot(word), f = covis_obs_feature(word);
            ok = lba_observer_ok(a.v, s, a.curMap);
            if (ok) {
                if (f >= a.v.kf_row_len(s) || a.v.kf_row_entry(s, f) != p) atomicAdd(&a.head[LBA_V_OBS_MISMATCH], 1);
                if (a.role[s] < 0) {                              // not local: its pose and key-points are read through the observation alone
                    if (!a.v.has_pose(s)) atomicAdd(&a.head[LBA_V_KF_NO_POSE], 1);
                    if (!a.v.featTab || a.v.feat_keys(s) < 0 || f >= a.v.feat_count(s)) atomicAdd(&a.head[LBA_V_KF_NO_FEATURES], 1);
                    // ... and it is a fixed camera (a dropped neighbour never gets here: what dropped it fails lba_observer_ok)
                    const unsigned long long key = a.v.kf_key(s);
                    int rank = 0;
                    for (int j = 0; j < L; j++) rank += a.v.kf_key(covis_obs_slot(row[j])) < key;
                    atomicMin(&a.fixTag[s], ((unsigned long long)i << kLbaRankBits) | (unsigned long long)rank);
                }
            }
        }
        edges += __popcll(__ballot(ok));
    }
    if (lane == 0) a.edgeCnt[i] = edges;
}

__global__ __launch_bounds__(1024) void k_lba_scan(LbaArgs a) {
    __shared__ int sWave[16];
    __shared__ int sCarry, sFixed;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid == 0) { sCarry = 0; sFixed = 0; }
    __syncthreads();
    // ---- the key-frame list: the locals, then the stamped slots in order of their first appearance
    for (int k = tid; k < a.nLocal; k += 1024) { a.kfList[k] = a.locals[k]; a.kfIndex[a.locals[k]] = k; }
    for (int s = tid; s < a.hiSlot; s += 1024) {
        const unsigned long long t = a.fixTag[s];
        if (t == kLbaNever) { if (a.role[s] < 0) a.kfIndex[s] = -1; continue; }
        int rank = 0;
        for (int j = 0; j < a.hiSlot; j++) rank += a.fixTag[j] < t;
        a.kfList[a.nLocal + rank] = s;
        a.kfIndex[s] = a.nLocal + rank;
        atomicAdd(&sFixed, 1);
    }
    // ---- ptStart: the exclusive prefix of the edge counts, 1024 points a round
    const int nMP = min(a.head[LBA_H_NMP], a.ptCap);
    for (int base = 0; base < nMP; base += 1024) {
        const int i = base + tid;
        const int c = i < nMP ? a.edgeCnt[i] : 0;
        int incl = c;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) { const int t = __shfl_up(incl, o); if (lane >= o) incl += t; }
        if (lane == 63) sWave[wave] = incl;
        __syncthreads();
        int before = sCarry;
        for (int w = 0; w < wave; w++) before += sWave[w];
        if (i < nMP) a.ptStart[i] = before + incl - c;
        __syncthreads();
        if (tid == 1023) sCarry = before + incl;
        __syncthreads();
    }
    if (tid == 0) { a.ptStart[nMP] = sCarry; a.head[LBA_H_NE] = sCarry; a.head[LBA_H_NFIXED] = sFixed; }
}

// rawT and poseCol of the key-frame list: a local key-frame is a fixed vertex iff it is the map's initial key-frame (:1094), a fixed camera always.
__global__ __launch_bounds__(256) void k_lba_fill_kf(LbaArgs a, LbaRaw w, int nKF) {
    const int k = (int)blockIdx.x * 256 + threadIdx.x;
    if (k >= nKF) return;
    const double *T = a.v.pose_of(a.kfList[k]);
    for (int j = 0; j < 7; j++) w.rawT[(size_t)k * 8 + j] = T[j];
    w.rawT[(size_t)k * 8 + 7] = 0;
    w.poseCol[k] = (k >= a.nLocal || k == a.initIdx) ? -1 : k - (a.initIdx >= 0 && k > a.initIdx ? 1 : 0);
}

// A wave per point: its position, and its edges in order_key order (:1155-1199).
__global__ __launch_bounds__(256) void k_lba_fill_edges(LbaArgs a, LbaRaw w, int nMP) {
    const int lane = threadIdx.x & 63, i = (int)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= nMP) return;
    const int p = a.ptList[i];
    if (lane < 3) w.rawX[(size_t)i * 3 + lane] = a.v.attr_pos(p)[lane];
    const int2 O = a.v.point_obs(p);
    const int32_t *row = a.v.rows + O.x;
    const int L = O.y, e0 = a.ptStart[i];
    for (int k = lane; k < L; k += 64) {
        const int word = row[k], s = covis_obs_slot(word), f = covis_obs_feature(word);
        if (!lba_observer_ok(a.v, s, a.curMap)) continue;
        const unsigned long long key = a.v.kf_key(s);
        int rank = 0;
        for (int j = 0; j < L; j++) {
            const int sj = covis_obs_slot(row[j]);
            rank += a.v.kf_key(sj) < key && lba_observer_ok(a.v, sj, a.curMap);
        }
        const long long keys = a.v.feat_keys(s);
        const RumiKeyPoint kp = a.v.keys_at(keys)[f];
        const CovisFeatRec *R = a.v.rec_of_keys(keys);
        const float sc = rec_arr<float>(R, R->scale)[kp.octave];
        const int e = e0 + rank;
        w.rawMP[e] = i;
        w.rawKF[e] = a.kfIndex[s];
        w.rawObs[2 * (size_t)e] = kp.x; w.rawObs[2 * (size_t)e + 1] = kp.y;
        w.rawInfo[e] = __fdiv_rn(1.0f, sc * sc);                  // mvInvLevelSigma2[octave] = 1.0f / (s * s), correctly rounded
        w.edgeObs[e] = word; w.edgePt[e] = p;
    }
}

// One workgroup after a run that was not aborted.  X: the result block's positions [nMP][3] (doubles), erase [nE].
__global__ __launch_bounds__(1024) void k_lba_commit(LbaArgs a, LbaRaw w, const double *X, const uint8_t *erase, int nMP, int nE, int32_t *erased, int erasedCap) {
    __shared__ int sWave[16];
    __shared__ int sCarry;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int i = tid; i < nMP * 3; i += 1024) {
        float *A = reinterpret_cast<float *>(a.v.attr_rec(a.ptList[i / 3]));
        A[i % 3] = (float)X[i];
    }
    if (tid == 0) sCarry = 0;
    __syncthreads();
    for (int base = 0; base < nE; base += 1024) {
        const int e = base + tid;
        const bool hit = e < nE && erase[e] != 0;
        const unsigned long long m = __ballot(hit);
        if (lane == 0) sWave[wave] = __popcll(m);
        __syncthreads();
        int off = sCarry, all = 0;
        for (int q = 0; q < 16; q++) { const int c = sWave[q]; off += q < wave ? c : 0; all += c; }
        off += __popcll(m & ((1ull << lane) - 1ull));
        if (hit && off < erasedCap) {
            const int word = w.edgeObs[e];
            erased[3 * (size_t)off] = covis_obs_slot(word); erased[3 * (size_t)off + 1] = w.edgePt[e]; erased[3 * (size_t)off + 2] = covis_obs_feature(word);
        }
        __syncthreads();
        if (tid == 0) sCarry += all;
        __syncthreads();
    }
    if (tid == 0) a.head[LBA_H_NERASED] = sCarry;
}
