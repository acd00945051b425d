// Key-frame database on gfx950 (include/rumi_kfdb.h): the inverted file of KeyFrameDatabase and its two queries,
// DetectRelocalizationCandidates (R/lib_src/KeyFrameDatabase.cc:733-843) and DetectNBestCandidates (:604-708), batched over queries.
//
// Layout.  Key-frames live in slots (maxKf); a slot holds the add sequence, map, flags, the BowVector's range in the entry pool, the ten
// best covisibles (slots, -1 padded) and the reference's per-KeyFrame query state for both kinds (last query id, last score).  The inverted
// file is one CSR over words of (slot, word) postings, rebuilt by count / scan / scatter on every add batch and erase; a posting list's
// order is not kept, because a query does not need it: the reference's list order is (rank of the first shared query word, add sequence),
// which the query computes as a key.
//
// A batch of Q queries (one tile: Q x maxKf counters) runs as
//   score:  k_q_count (one wave per (query, query word) over its posting list: integer atomicAdd count, atomicMin first-word rank)
//           k_q_scan1 (one lane per slot, queries in order: marks against the slot's last query id -> listed / marked / none, max count)
//           k_q_gather + k_q_sort (the key-frames above the word threshold, in list order)
//           k_q_si    (one wave per scored key-frame: the common words' L1 terms in parallel, folded in word order)
//   select: k_q_scan2 (one lane per slot, queries in order: the score a marked key-frame has at each query, stale or fresh)
//           k_q_acc   (one lane per scored key-frame: covisibility accumulation in covisibility order)
//           k_q_reloc / k_q_nbest (one workgroup per query: the final walk; N-best after a stable descending rank sort)
// No float atomics: every float and double result is a fixed-order fold.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>
#include <set>
#include <unordered_map>
#include <unordered_set>
#include <vector>

#include "rumi_common.h"
#include "rumi_internal.h"
#include "rumi_kfdb.h"

namespace rumi {

constexpr int kNCov = RUMI_KFDB_NCOV;
constexpr int kConnected = INT_MIN / 2;      // count of a connected key-frame: stays negative whatever it shares
constexpr int kMarked = -1;                  // count after scan1 of a key-frame marked by an EARLIER call with the same query id
constexpr uint32_t kAdded = 0xFFFFFFFEu;     // rank cell reused as the "already added" flag of the final walks
constexpr int kSeqBits = 40;

struct NewKF {
    int32_t slot, map, bowOff, bowN;
    int64_t seq;
    uint64_t lastQ[2];
    float lastS[2];
};

__global__ void k_new_meta(const NewKF *__restrict__ nk, int n, int maxKf, int64_t *seq, int32_t *map, uint8_t *live, uint8_t *bad, int32_t *bowOff,
                           int32_t *bowN, int32_t *cov, uint64_t *lastQ, float *lastS) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const NewKF k = nk[i];
    seq[k.slot] = k.seq; map[k.slot] = k.map; live[k.slot] = 1; bad[k.slot] = 0; bowOff[k.slot] = k.bowOff; bowN[k.slot] = k.bowN;
    for (int c = 0; c < kNCov; c++) cov[(size_t)k.slot * kNCov + c] = -1;
    lastQ[k.slot] = k.lastQ[0]; lastQ[maxKf + k.slot] = k.lastQ[1];
    lastS[k.slot] = k.lastS[0]; lastS[maxKf + k.slot] = k.lastS[1];
}

template <class T> __global__ void k_set_at(const int32_t *__restrict__ slots, const T *__restrict__ vals, int n, int stride, T *dst) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) for (int c = 0; c < stride; c++) dst[(size_t)slots[i] * stride + c] = vals[(size_t)i * stride + c];
}

__global__ void k_cov_clean(int n, const uint8_t *__restrict__ live, int32_t *cov) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n && cov[i] >= 0 && !live[cov[i]]) cov[i] = -1;
}

// ---- inverted file: count / scan / scatter ----
__global__ void k_count_old(int T, const int32_t *__restrict__ pSlot, const uint32_t *__restrict__ pWord, const uint8_t *__restrict__ live, int32_t *cnt) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < T && live[pSlot[i]]) atomicAdd(&cnt[pWord[i]], 1);
}
__global__ void k_count_new(const int32_t *__restrict__ slots, const int32_t *__restrict__ bowOff, const int32_t *__restrict__ bowN,
                            const uint32_t *__restrict__ poolW, int32_t *cnt) {
    const int s = slots[blockIdx.x], o = bowOff[s], n = bowN[s];
    for (int j = threadIdx.x; j < n; j += blockDim.x) atomicAdd(&cnt[poolW[o + j]], 1);
}
__global__ void k_scatter_old(int T, const int32_t *__restrict__ pSlot, const uint32_t *__restrict__ pWord, const uint8_t *__restrict__ live,
                              int32_t *fill, int32_t *nSlot, uint32_t *nWord) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= T) return;
    const int s = pSlot[i];
    if (!live[s]) return;
    const uint32_t w = pWord[i];
    const int p = atomicAdd(&fill[w], 1);
    nSlot[p] = s; nWord[p] = w;
}
__global__ void k_scatter_new(const int32_t *__restrict__ slots, const int32_t *__restrict__ bowOff, const int32_t *__restrict__ bowN,
                              const uint32_t *__restrict__ poolW, int32_t *fill, int32_t *nSlot, uint32_t *nWord) {
    const int s = slots[blockIdx.x], o = bowOff[s], n = bowN[s];
    for (int j = threadIdx.x; j < n; j += blockDim.x) {
        const uint32_t w = poolW[o + j];
        const int p = atomicAdd(&fill[w], 1);
        nSlot[p] = s; nWord[p] = w;
    }
}

// exclusive scan of n int32 (n <= 1024 * 4 * 1024 per pass of the block sums, which loop)
constexpr int kScanBlock = 1024, kScanPer = 4, kScanTile = kScanBlock * kScanPer;
__device__ int block_excl_scan(int v, int *sh, int *total) {
    const int t = threadIdx.x;
    sh[t] = v;
    __syncthreads();
    for (int o = 1; o < kScanBlock; o <<= 1) {
        const int x = t >= o ? sh[t - o] : 0;
        __syncthreads();
        sh[t] += x;
        __syncthreads();
    }
    const int incl = sh[t];
    *total = sh[kScanBlock - 1];
    __syncthreads();
    return incl - v;
}
__global__ __launch_bounds__(1024) void k_scan_tiles(const int32_t *__restrict__ in, int n, int32_t *out, int32_t *tileSums) {
    __shared__ int sh[kScanBlock];
    const int base = blockIdx.x * kScanTile + threadIdx.x * kScanPer;
    int v[kScanPer], s = 0;
    for (int k = 0; k < kScanPer; k++) { v[k] = base + k < n ? in[base + k] : 0; s += v[k]; }
    int total;
    int run = block_excl_scan(s, sh, &total);
    for (int k = 0; k < kScanPer; k++) { if (base + k < n) out[base + k] = run; run += v[k]; }
    if (threadIdx.x == 0) tileSums[blockIdx.x] = total;
}
__global__ __launch_bounds__(1024) void k_scan_sums(int32_t *tileSums, int m, int32_t *grand) {
    __shared__ int sh[kScanBlock];
    int carry = 0;
    for (int b = 0; b < m; b += kScanBlock) {
        const int i = b + threadIdx.x;
        const int v = i < m ? tileSums[i] : 0;
        int total;
        const int ex = block_excl_scan(v, sh, &total);
        if (i < m) tileSums[i] = carry + ex;
        carry += total;
    }
    if (threadIdx.x == 0) *grand = carry;
}
__global__ __launch_bounds__(1024) void k_scan_add(int32_t *out, int n, const int32_t *__restrict__ tileSums) {
    const int base = blockIdx.x * kScanTile + threadIdx.x * kScanPer;
    const int add = tileSums[blockIdx.x];
    for (int k = 0; k < kScanPer; k++) if (base + k < n) out[base + k] += add;
}

__global__ void k_pool_gather(const int32_t *__restrict__ slots, const int32_t *__restrict__ newOff, const int32_t *__restrict__ bowOff,
                              const int32_t *__restrict__ bowN, const uint32_t *__restrict__ w, const double *__restrict__ v, uint32_t *w2, double *v2) {
    const int s = slots[blockIdx.x], o = bowOff[s], n = bowN[s], d = newOff[blockIdx.x];
    for (int j = threadIdx.x; j < n; j += blockDim.x) { w2[d + j] = w[o + j]; v2[d + j] = v[o + j]; }
}

// ---- BowVector assembly on the device (rumi_voc_assemble, voc.hip, for L1 scoring) ----
// One workgroup per frame.  Live features with weight > 0 are ranked by (word, feature index); thread 0 then walks the ranks: per-word sums in
// feature order (addWeight) or the first value (addIfNotExist), the L1 norm in word order; the division is parallel.
__global__ __launch_bounds__(256) void k_bow_assemble(const uint32_t *__restrict__ word, const double *__restrict__ weight, const int32_t *__restrict__ counts,
                                                      int cap, int tf, uint64_t *key, int32_t *order, uint32_t *outW, double *outV, int32_t *outN) {
    const int f = blockIdx.x;
    const int n = min(counts[2 * f], cap);
    const size_t b = (size_t)f * cap;
    for (int i = threadIdx.x; i < n; i += blockDim.x) key[b + i] = weight[b + i] > 0 ? ((uint64_t)word[b + i] << 32) | (uint32_t)i : ~0ull;
    __syncthreads();
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
        const uint64_t k = key[b + i];
        if (k == ~0ull) continue;
        int r = 0;
        for (int j = 0; j < n; j++) r += key[b + j] < k;
        order[b + r] = i;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int m = 0;
        for (int i = 0; i < n; i++) m += key[b + i] != ~0ull;
        int u = -1;
        uint32_t prev = 0;
        for (int r = 0; r < m; r++) {
            const int i = order[b + r];
            const uint32_t w = word[b + i];
            const double x = weight[b + i];
            if (u < 0 || w != prev) { ++u; outW[b + u] = w; outV[b + u] = x; prev = w; }
            else if (tf) outV[b + u] = outV[b + u] + x;
        }
        const int nu = u + 1;
        double norm = 0.0;
        for (int k = 0; k < nu; k++) norm += fabs(outV[b + k]);
        outN[f] = nu;
        key[b] = __double_as_longlong(norm);          // hand the norm to the division below (slot 0 of the scratch is no longer needed)
    }
    __syncthreads();
    const int nu = outN[f];
    const double norm = __longlong_as_double((long long)key[b]);
    if (norm > 0.0)
        for (int k = threadIdx.x; k < nu; k += blockDim.x) outV[b + k] = outV[b + k] / norm;
}
__global__ void k_bow_place(const int32_t *__restrict__ frameOf, const int32_t *__restrict__ dstOff, const int32_t *__restrict__ nU, int cap,
                            const uint32_t *__restrict__ w, const double *__restrict__ v, uint32_t *poolW, double *poolV) {
    const int f = frameOf[blockIdx.x], d = dstOff[blockIdx.x], n = nU[f];
    const size_t b = (size_t)f * cap;
    for (int j = threadIdx.x; j < n; j += blockDim.x) { poolW[d + j] = w[b + j]; poolV[d + j] = v[b + j]; }
}

// ---- queries ----
struct QDev {
    int nq, maxKf, kind;
    const uint64_t *qid; const int32_t *qmap; const int64_t *qvb; const int32_t *qBowOff; const uint32_t *qW; const double *qV;
    int32_t *count; uint32_t *rank; float *val;                       // [nq][maxKf]
    int32_t *list; uint64_t *key; float *si; float *acc; int32_t *best; int32_t *order;   // [nq][maxKf], list-indexed
    int32_t *maxc, *minc, *nsc, *scOff;                                // [nq] / [nq + 1]
};

__global__ void k_q_conn(int n, const int32_t *__restrict__ cq, const int32_t *__restrict__ cs, int maxKf, int32_t *count) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) count[(size_t)cq[i] * maxKf + cs[i]] = kConnected;
}

// One wave per (query, query word): every posting of the word, visible to the query, counts once (mnRelocWords++ / mnPlaceRecognitionWords++);
// the smallest rank of the query words a key-frame is met on is its first encounter.
__global__ __launch_bounds__(256) void k_q_count(QDev Q, int nWordsTotal, const int32_t *__restrict__ qOfWord, const int32_t *__restrict__ off,
                                                 const int32_t *__restrict__ pSlot, const int64_t *__restrict__ seq) {
    const int gw = (int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6), lane = threadIdx.x & 63;
    if (gw >= nWordsTotal) return;
    const int q = qOfWord[gw];
    const uint32_t r = (uint32_t)(gw - Q.qBowOff[q]);
    const uint32_t w = Q.qW[gw];
    const int64_t bound = Q.qvb[q];
    const size_t row = (size_t)q * Q.maxKf;
    for (int p = off[w] + lane; p < off[w + 1]; p += 64) {
        const int X = pSlot[p];
        if (seq[X] >= bound) continue;
        atomicAdd(&Q.count[row + X], 1);
        atomicMin(&Q.rank[row + X], r);
    }
}

// One lane per slot, the queries of the tile in order (the reference's per-KeyFrame mnXQuery): a key-frame that shares a word, is not connected and
// whose last query id is not this query's is listed and takes the id; one whose last query id already is this query's (an earlier call with the
// same id) is marked but not listed.  count afterwards: > 0 listed (its word count), kMarked, or 0.
__global__ void k_q_scan1(QDev Q, int hi, const uint8_t *__restrict__ live, const int64_t *__restrict__ seq, uint64_t *lastQ) {
    const int X = blockIdx.x * blockDim.x + threadIdx.x;
    if (X >= hi) return;
    uint64_t lq = lastQ[(size_t)Q.kind * Q.maxKf + X];
    const bool lv = live[X] != 0;
    const int64_t sx = seq[X];
    for (int q = 0; q < Q.nq; q++) {
        const size_t idx = (size_t)q * Q.maxKf + X;
        const int c = Q.count[idx];
        const bool pre = lv && sx < Q.qvb[q] && lq == Q.qid[q];
        if (c > 0 && !pre) { atomicMax(&Q.maxc[q], c); lq = Q.qid[q]; }
        else if (pre) Q.count[idx] = kMarked;
        else if (c != 0) Q.count[idx] = 0;
    }
    lastQ[(size_t)Q.kind * Q.maxKf + X] = lq;
}

__device__ __forceinline__ int min_common(int maxc) { return (int)((float)maxc * 0.8f); }   // int minCommonWords = maxCommonWords*0.8f;

__global__ void k_q_gather(QDev Q, int hi, const int64_t *__restrict__ seq) {
    const int X = blockIdx.x * blockDim.x + threadIdx.x, q = blockIdx.y;
    if (X >= hi) return;
    const size_t idx = (size_t)q * Q.maxKf + X;
    if (Q.count[idx] > min_common(Q.maxc[q])) {
        const int i = atomicAdd(&Q.nsc[q], 1);
        Q.order[(size_t)q * Q.maxKf + i] = X;
        Q.key[(size_t)q * Q.maxKf + i] = ((uint64_t)Q.rank[idx] << kSeqBits) | (uint64_t)seq[X];
    }
}

// list order = (rank of the first shared query word, add sequence): keys are distinct, so a rank is a position
__global__ __launch_bounds__(256) void k_q_sort(QDev Q) {
    const int q = blockIdx.x, n = Q.nsc[q];
    const size_t row = (size_t)q * Q.maxKf;
    if (threadIdx.x == 0) Q.minc[q] = min_common(Q.maxc[q]);
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
        const uint64_t k = Q.key[row + i];
        int r = 0;
        for (int j = 0; j < n; j++) r += Q.key[row + j] < k;
        Q.list[row + r] = Q.order[row + i];
    }
}

__device__ __forceinline__ int query_of(const int32_t *scOff, int nq, int g) {    // last q with scOff[q] <= g
    int lo = 0, hi = nq - 1;
    while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (scOff[mid] <= g) lo = mid; else hi = mid - 1; }
    return lo;
}

// L1Scoring::score(query, kf) (ScoringObject.cpp:23-68): over the common words in ascending id, score += fabs(v-w) - fabs(v) - fabs(w); -score/2.0.
// One wave per scored key-frame: 64 of the key-frame's words at a time are looked up in the query's words, the terms come in parallel, and
// every lane folds them in word order (the same fold in every lane).
__global__ __launch_bounds__(256) void k_q_si(QDev Q, int total, const int32_t *__restrict__ bowOff, const int32_t *__restrict__ bowN,
                                              const uint32_t *__restrict__ poolW, const double *__restrict__ poolV, int32_t *flatSlot, float *flatSi) {
    const int g = (int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6), lane = threadIdx.x & 63;
    if (g >= total) return;
    const int q = query_of(Q.scOff, Q.nq, g), i = g - Q.scOff[q];
    const size_t row = (size_t)q * Q.maxKf;
    const int X = Q.list[row + i];
    const int q0 = Q.qBowOff[q], nqw = Q.qBowOff[q + 1] - q0, o = bowOff[X], nk = bowN[X];
    double s = 0;
    for (int base = 0; base < nk; base += 64) {
        const int j = base + lane;
        bool found = false;
        double term = 0;
        if (j < nk) {
            const uint32_t w = poolW[o + j];
            int lo = 0, hi = nqw;
            while (lo < hi) { const int mid = (lo + hi) >> 1; if (Q.qW[q0 + mid] < w) lo = mid + 1; else hi = mid; }
            if (lo < nqw && Q.qW[q0 + lo] == w) {
                const double vi = Q.qV[q0 + lo], wi = poolV[o + j];
                term = fabs(vi - wi) - fabs(vi) - fabs(wi);
                found = true;
            }
        }
        unsigned long long m = __ballot(found);
        while (m) {
            const int b = __ffsll((long long)m) - 1;
            s += __shfl(term, b);
            m &= m - 1;
        }
    }
    if (lane == 0) {
        const float si = (float)(-s / 2.0);
        Q.val[row + X] = si;
        Q.si[row + i] = si;
        flatSlot[g] = X;
        flatSi[g] = si;
    }
}

// One lane per slot, queries in order: the score a key-frame carries at each query (mRelocScore / mPlaceRecognitionScore): this query's si where
// it was scored, else the value the last earlier scoring left.
__global__ void k_q_scan2(QDev Q, int hi, float *lastS) {
    const int X = blockIdx.x * blockDim.x + threadIdx.x;
    if (X >= hi) return;
    float ls = lastS[(size_t)Q.kind * Q.maxKf + X];
    for (int q = 0; q < Q.nq; q++) {
        const size_t idx = (size_t)q * Q.maxKf + X;
        if (Q.count[idx] > Q.minc[q]) ls = Q.val[idx];
        else Q.val[idx] = ls;
    }
    lastS[(size_t)Q.kind * Q.maxKf + X] = ls;
}

// "Lets now accumulate score by covisibility": float sums in covisibility order over the covisibles this query marked.
__global__ void k_q_acc(QDev Q, int total, const int32_t *__restrict__ cov) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= total) return;
    const int q = query_of(Q.scOff, Q.nq, g), i = g - Q.scOff[q];
    const size_t row = (size_t)q * Q.maxKf;
    const int P = Q.list[row + i];
    float bestScore = Q.si[row + i], accScore = bestScore;
    int bestKF = P;
    for (int k = 0; k < kNCov; k++) {
        const int X = cov[(size_t)P * kNCov + k];
        if (X < 0) continue;
        const int c = Q.count[row + X];
        if (c <= 0 && c != kMarked) continue;
        const float v = Q.val[row + X];
        accScore += v;
        if (v > bestScore) { bestKF = X; bestScore = v; }
    }
    Q.acc[row + i] = accScore;
    Q.best[row + i] = bestKF;
}

__device__ float block_max256(float v, float *sh) {
    sh[threadIdx.x] = v;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) sh[threadIdx.x] = fmaxf(sh[threadIdx.x], sh[threadIdx.x + o]);
        __syncthreads();
    }
    return sh[0];
}

// DetectRelocalizationCandidates' final walk (:823-840), list order, first occurrence of each best key-frame of the query's map
__global__ __launch_bounds__(256) void k_q_reloc(QDev Q, const int32_t *__restrict__ map, int32_t *outSlot, int32_t *outN) {
    __shared__ float sh[256];
    const int q = blockIdx.x, n = Q.nsc[q];
    const size_t row = (size_t)q * Q.maxKf;
    float m = 0.f;                                               // bestAccScore = 0; if(accScore>bestAccScore) ...
    for (int i = threadIdx.x; i < n; i += blockDim.x) { const float a = Q.acc[row + i]; if (a > m) m = a; }
    const float bestAcc = block_max256(m, sh);
    if (threadIdx.x != 0) return;
    const float minScoreToRetain = 0.75f * bestAcc;
    const int qmap = Q.qmap[q], o = Q.scOff[q];
    int k = 0;
    for (int i = 0; i < n; i++) {
        if (!(Q.acc[row + i] > minScoreToRetain)) continue;
        const int P = Q.best[row + i];
        if (map[P] != qmap) continue;
        if (Q.rank[row + P] == kAdded) continue;
        Q.rank[row + P] = kAdded;
        outSlot[o + k++] = P;
    }
    outN[q] = k;
}

// DetectNBestCandidates' final walk (:680-706) after lAccScoreAndMatch.sort(compFirst): std::list::sort is stable, so the position of entry i is the
// number of entries with a larger acc plus the earlier entries with an equal one.  isBad() key-frames are skipped and the walk advances.
__global__ __launch_bounds__(256) void k_q_nbest(QDev Q, const int32_t *__restrict__ map, const uint8_t *__restrict__ bad, const int32_t *__restrict__ badMaps,
                                                 int nBadMaps, const int32_t *__restrict__ nCand, int stride, int32_t *loop, int32_t *nLoop, int32_t *merge,
                                                 int32_t *nMerge) {
    const int q = blockIdx.x, n = Q.nsc[q];
    const size_t row = (size_t)q * Q.maxKf;
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
        const float a = Q.acc[row + i];
        int r = 0;
        for (int j = 0; j < n; j++) { const float b = Q.acc[row + j]; r += (b > a) || (b == a && j < i); }
        Q.order[row + r] = i;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    const int N = nCand[q], qmap = Q.qmap[q];
    int nl = 0, nm = 0;
    for (int i = 0; i < n && (nl < N || nm < N); i++) {
        const int P = Q.best[row + Q.order[row + i]];
        if (bad[P]) continue;
        if (Q.rank[row + P] == kAdded) continue;
        const int mp = map[P];
        if (mp == qmap && nl < N) loop[(size_t)q * stride + nl++] = P;
        else if (mp != qmap && nm < N) {
            bool mapBad = false;
            for (int b = 0; b < nBadMaps; b++) mapBad |= badMaps[b] == mp;
            if (!mapBad) merge[(size_t)q * stride + nm++] = P;
        }
        Q.rank[row + P] = kAdded;
    }
    nLoop[q] = nl;
    nMerge[q] = nm;
}

// The query arrays are DevBufs of at least 64 elements, so that the small ones stop growing early.
template <class T> int ensure(DevBuf<T> &b, size_t n) { return b.reserve(n, std::max<size_t>(n, 64)); }
template <class T> int put(DevBuf<T> &b, const T *h, size_t n) {
    const int rc = ensure(b, n);
    if (rc != RUMI_OK) return rc;
    if (n) HIP_TRY(hipMemcpy(b.p, h, n * sizeof(T), hipMemcpyHostToDevice));
    return RUMI_OK;
}

inline int blocks(size_t n, int t) { return (int)((n + t - 1) / t); }

}  // namespace rumi

using namespace rumi;

struct RumiKFDatabase {
    int device = 0, nWords = 0, weighting = 0, maxKf = 0, tileQ = 1;
    int64_t maxEntries = 0;
    // host mirrors
    std::unordered_map<uint64_t, int> slotOf;
    std::vector<uint64_t> idOf;
    std::vector<uint8_t> liveH;
    std::vector<int32_t> mapH, bowOffH, bowNH;
    std::vector<int> freeSlots;
    int hi = 0;                                   // slots [0, hi) have been used
    int64_t nextSeq = 0, liveEntries = 0, poolTop = 0;
    int nLive = 0;
    struct Saved { uint64_t q[2]; float s[2]; };
    std::unordered_map<uint64_t, Saved> saved;    // query state of key-frames that left the inverted file (the KeyFrame object keeps it)
    std::set<int32_t> badMaps;
    // staged adds
    std::vector<NewKF> staged;
    std::vector<uint32_t> stW;
    std::vector<double> stV;
    // device
    int64_t *dSeq = nullptr; int32_t *dMap = nullptr; uint8_t *dLive = nullptr, *dBad = nullptr; int32_t *dBowOff = nullptr, *dBowN = nullptr;
    int32_t *dCov = nullptr; uint64_t *dLastQ = nullptr; float *dLastS = nullptr;
    uint32_t *dPoolW = nullptr; double *dPoolV = nullptr;
    int32_t *dOff = nullptr, *dFill = nullptr, *dTileSums = nullptr, *dGrand = nullptr;
    int32_t *dPSlot[2] = {nullptr, nullptr}; uint32_t *dPWord[2] = {nullptr, nullptr};
    int cur = 0;
    int64_t T = 0;                                // postings in the inverted file
    // query workspace
    int32_t *wCount = nullptr; uint32_t *wRank = nullptr; float *wVal = nullptr; int32_t *wList = nullptr; uint64_t *wKey = nullptr; float *wSi = nullptr;
    float *wAcc = nullptr; int32_t *wBest = nullptr; int32_t *wOrder = nullptr;
    int32_t *qSmall = nullptr;                    // maxc, minc, nsc, scOff [tileQ + 1], outN, nLoop, nMerge, nCand
    DevBuf<uint64_t> qId; DevBuf<int32_t> qMap; DevBuf<int64_t> qVb; DevBuf<int32_t> qBowOff, qOfWord, connQ, connS, flatSlot, outSlot, loopS, mergeS, badM, tmpI;
    DevBuf<uint32_t> qW; DevBuf<double> qV; DevBuf<float> flatSi; DevBuf<NewKF> newKF;
    DevBuf<uint64_t> asmKey; DevBuf<int32_t> asmOrder, asmN; DevBuf<uint32_t> asmW; DevBuf<double> asmV;
    // pending query
    int pendKind = -1, pendNq = 0;
    std::vector<int32_t> pendScOff;
};

namespace {

void kfdb_free(RumiKFDatabase *d) {
    void *p[] = {d->dSeq, d->dMap, d->dLive, d->dBad, d->dBowOff, d->dBowN, d->dCov, d->dLastQ, d->dLastS, d->dPoolW, d->dPoolV, d->dOff, d->dFill,
                 d->dTileSums, d->dGrand, d->dPSlot[0], d->dPSlot[1], d->dPWord[0], d->dPWord[1], d->wCount, d->wRank, d->wVal, d->wList, d->wKey,
                 d->wSi, d->wAcc, d->wBest, d->wOrder, d->qSmall};
    for (void *q : p) if (q) (void)hipFree(q);
}

int fail(const char *msg, int code) { g_lastError = msg; return code; }

// the inverted file again from its live postings plus the entries of the new slots
int rebuild(RumiKFDatabase *d, const std::vector<int32_t> &newSlots) {
    const int nw1 = d->nWords + 1;
    HIP_TRY(hipMemset(d->dFill, 0, (size_t)nw1 * 4));
    int rc = put(d->tmpI, newSlots.data(), newSlots.size());
    if (rc != RUMI_OK) return rc;
    if (d->T > 0) hipLaunchKernelGGL(k_count_old, dim3(blocks(d->T, 256)), dim3(256), 0, nullptr, (int)d->T, d->dPSlot[d->cur], d->dPWord[d->cur], d->dLive, d->dFill);
    if (!newSlots.empty()) hipLaunchKernelGGL(k_count_new, dim3((unsigned)newSlots.size()), dim3(256), 0, nullptr, d->tmpI.p, d->dBowOff, d->dBowN, d->dPoolW, d->dFill);
    const int nt = blocks(nw1, kScanTile);
    hipLaunchKernelGGL(k_scan_tiles, dim3(nt), dim3(kScanBlock), 0, nullptr, d->dFill, nw1, d->dOff, d->dTileSums);
    hipLaunchKernelGGL(k_scan_sums, dim3(1), dim3(kScanBlock), 0, nullptr, d->dTileSums, nt, d->dGrand);
    hipLaunchKernelGGL(k_scan_add, dim3(nt), dim3(kScanBlock), 0, nullptr, d->dOff, nw1, d->dTileSums);
    HIP_TRY(hipMemcpy(d->dFill, d->dOff, (size_t)nw1 * 4, hipMemcpyDeviceToDevice));
    const int nx = d->cur ^ 1;
    if (d->T > 0) hipLaunchKernelGGL(k_scatter_old, dim3(blocks(d->T, 256)), dim3(256), 0, nullptr, (int)d->T, d->dPSlot[d->cur], d->dPWord[d->cur], d->dLive, d->dFill, d->dPSlot[nx], d->dPWord[nx]);
    if (!newSlots.empty()) hipLaunchKernelGGL(k_scatter_new, dim3((unsigned)newSlots.size()), dim3(256), 0, nullptr, d->tmpI.p, d->dBowOff, d->dBowN, d->dPoolW, d->dFill, d->dPSlot[nx], d->dPWord[nx]);
    HIP_TRY(hipGetLastError());
    d->cur = nx;
    d->T = d->liveEntries;
    HIP_TRY(hipDeviceSynchronize());
    return RUMI_OK;
}

// moves the live BowVectors to the front of the pool (slot order) so that `need` more entries fit at poolTop
int compact_pool(RumiKFDatabase *d) {
    std::vector<int32_t> slots, newOff;
    int64_t top = 0;
    for (int s = 0; s < d->hi; s++) if (d->liveH[s]) { slots.push_back(s); newOff.push_back((int32_t)top); top += d->bowNH[s]; }
    uint32_t *w2 = nullptr; double *v2 = nullptr;
    auto drop = [&](int rc) { if (w2) (void)hipFree(w2); if (v2) (void)hipFree(v2); return rc; };
    if (hipMalloc((void **)&w2, (size_t)std::max<int64_t>(d->maxEntries, 1) * 4) != hipSuccess ||
        hipMalloc((void **)&v2, (size_t)std::max<int64_t>(d->maxEntries, 1) * 8) != hipSuccess)
        return drop(fail("rumi_kfdb: entry pool compaction: device allocation failed", RUMI_E_NO_DEVICE));
    if (!slots.empty()) {
        int rc = put(d->tmpI, slots.data(), slots.size());
        if (rc == RUMI_OK) rc = put(d->flatSlot, newOff.data(), newOff.size());
        if (rc != RUMI_OK) return drop(rc);
        hipLaunchKernelGGL(k_pool_gather, dim3((unsigned)slots.size()), dim3(256), 0, nullptr, d->tmpI.p, d->flatSlot.p, d->dBowOff, d->dBowN, d->dPoolW, d->dPoolV, w2, v2);
        hipLaunchKernelGGL(k_set_at<int32_t>, dim3(blocks(slots.size(), 256)), dim3(256), 0, nullptr, d->tmpI.p, d->flatSlot.p, (int)slots.size(), 1, d->dBowOff);
    }
    if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess)
        return drop(fail("rumi_kfdb: entry pool compaction: kernel failed", RUMI_E_NO_DEVICE));
    (void)hipFree(d->dPoolW); (void)hipFree(d->dPoolV);
    d->dPoolW = w2; d->dPoolV = v2;
    for (size_t i = 0; i < slots.size(); i++) d->bowOffH[slots[i]] = newOff[i];
    d->poolTop = top;
    return RUMI_OK;
}

int take_slot(RumiKFDatabase *d) {
    if (!d->freeSlots.empty()) { const int s = d->freeSlots.back(); d->freeSlots.pop_back(); return s; }
    return d->hi++;
}

NewKF new_kf(RumiKFDatabase *d, int slot, uint64_t id, int32_t map, int32_t n) {
    NewKF k{};
    k.slot = slot; k.map = map; k.bowN = n; k.seq = d->nextSeq++;
    auto it = d->saved.find(id);
    if (it != d->saved.end()) { for (int j = 0; j < 2; j++) { k.lastQ[j] = it->second.q[j]; k.lastS[j] = it->second.s[j]; } d->saved.erase(it); }
    d->slotOf[id] = slot; d->idOf[slot] = id; d->liveH[slot] = 1; d->mapH[slot] = map; d->bowNH[slot] = n;
    d->nLive++;
    return k;
}

int upload_new(RumiKFDatabase *d, const std::vector<NewKF> &ks) {
    int rc = put(d->newKF, ks.data(), ks.size());
    if (rc != RUMI_OK) return rc;
    hipLaunchKernelGGL(k_new_meta, dim3(blocks(ks.size(), 256)), dim3(256), 0, nullptr, d->newKF.p, (int)ks.size(), d->maxKf, d->dSeq, d->dMap, d->dLive, d->dBad,
                       d->dBowOff, d->dBowN, d->dCov, d->dLastQ, d->dLastS);
    HIP_TRY(hipGetLastError());
    return RUMI_OK;
}

// applies the staged host adds: their BowVectors at the pool's top, their slots, one rebuild of the inverted file
int flush(RumiKFDatabase *d) {
    if (d->staged.empty()) return RUMI_OK;
    HIP_TRY(hipSetDevice(d->device));
    const int64_t need = (int64_t)d->stW.size();
    if (d->poolTop + need > d->maxEntries) {
        // the staged slots are marked live on the host but have no pool range yet: leave them out of the compaction
        for (auto &k : d->staged) d->liveH[k.slot] = 0;
        const int rc = compact_pool(d);
        for (auto &k : d->staged) d->liveH[k.slot] = 1;
        if (rc != RUMI_OK) return rc;
    }
    if (need) {
        HIP_TRY(hipMemcpy(d->dPoolW + d->poolTop, d->stW.data(), (size_t)need * 4, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(d->dPoolV + d->poolTop, d->stV.data(), (size_t)need * 8, hipMemcpyHostToDevice));
    }
    std::vector<int32_t> slots;
    for (auto &k : d->staged) {
        k.bowOff = (int32_t)(d->poolTop + k.bowOff);
        d->bowOffH[k.slot] = k.bowOff;
        slots.push_back(k.slot);
    }
    d->poolTop += need;
    int rc = upload_new(d, d->staged);
    if (rc != RUMI_OK) return rc;
    d->staged.clear(); d->stW.clear(); d->stV.clear();
    return rebuild(d, slots);
}

// takes slots out of the inverted file; their query state is kept by id
int remove_slots(RumiKFDatabase *d, const std::vector<int32_t> &slots) {
    if (slots.empty()) return RUMI_OK;
    const size_t mk = (size_t)d->maxKf;
    std::vector<uint64_t> lq(2 * mk);
    std::vector<float> ls(2 * mk);
    HIP_TRY(hipMemcpy(lq.data(), d->dLastQ, 2 * mk * 8, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(ls.data(), d->dLastS, 2 * mk * 4, hipMemcpyDeviceToHost));
    std::vector<uint8_t> zeros(slots.size(), 0);
    for (int s : slots) {
        RumiKFDatabase::Saved sv;
        for (int j = 0; j < 2; j++) { sv.q[j] = lq[j * mk + s]; sv.s[j] = ls[j * mk + s]; }
        d->saved[d->idOf[s]] = sv;
        d->slotOf.erase(d->idOf[s]);
        d->liveH[s] = 0;
        d->liveEntries -= d->bowNH[s];
        d->nLive--;
    }
    int rc = put(d->tmpI, slots.data(), slots.size());
    if (rc != RUMI_OK) return rc;
    rc = ensure(d->badM, slots.size());
    if (rc != RUMI_OK) return rc;
    HIP_TRY(hipMemcpy(d->badM.p, zeros.data(), zeros.size(), hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_set_at<uint8_t>, dim3(blocks(slots.size(), 256)), dim3(256), 0, nullptr, d->tmpI.p, (const uint8_t *)d->badM.p, (int)slots.size(), 1, d->dLive);
    hipLaunchKernelGGL(k_cov_clean, dim3(blocks((size_t)d->hi * kNCov, 256)), dim3(256), 0, nullptr, d->hi * kNCov, d->dLive, d->dCov);
    HIP_TRY(hipGetLastError());
    rc = rebuild(d, {});
    if (rc != RUMI_OK) return rc;
    for (int s : slots) d->freeSlots.push_back(s);
    return RUMI_OK;
}

bool bow_ok(const uint32_t *w, int n, int nWords) {
    for (int j = 0; j < n; j++) if (w[j] >= (uint32_t)nWords || (j > 0 && w[j] <= w[j - 1])) return false;
    return true;
}

}  // namespace

extern "C" void rumi_kfdb_destroy(RumiKFDatabase *d) {
    if (!d) return;
    (void)hipSetDevice(d->device);
    kfdb_free(d);
    delete d;
}

extern "C" int rumi_kfdb_create(const RumiVocabulary *voc, int32_t max_kf, int64_t max_entries, int32_t device, RumiKFDatabase **out) {
    if (!out) return RUMI_E_INVALID;
    *out = nullptr;
    if (!voc || max_kf < 1 || max_entries < 1 || max_entries >= INT_MAX) return fail("rumi_kfdb_create: bad argument", RUMI_E_INVALID);
    int vdev, nWords, weighting, scoring;
    voc_params(voc, &vdev, &nWords, &weighting, &scoring);
    if (scoring != 0) return fail("rumi_kfdb_create: only L1_NORM scoring is implemented (the vocabulary's ScoringType is another)", RUMI_E_INVALID);
    if (nWords < 1) return fail("rumi_kfdb_create: the vocabulary has no words", RUMI_E_INVALID);
    if (const int rc = require_device(); rc != RUMI_OK) return rc;
    RumiKFDatabase *d = new RumiKFDatabase();
    d->device = device >= 0 ? device : vdev;
    d->nWords = nWords; d->weighting = weighting; d->maxKf = max_kf; d->maxEntries = max_entries;
    d->tileQ = (int)std::max<int64_t>(1, std::min<int64_t>(1024, ((int64_t)1 << 23) / max_kf));
    d->idOf.assign(max_kf, 0); d->liveH.assign(max_kf, 0); d->mapH.assign(max_kf, 0); d->bowOffH.assign(max_kf, 0); d->bowNH.assign(max_kf, 0);
    if (hipSetDevice(d->device) != hipSuccess) { delete d; return RUMI_E_NO_DEVICE; }
    const size_t mk = (size_t)max_kf, me = (size_t)max_entries, nw1 = (size_t)nWords + 1, cells = (size_t)d->tileQ * mk;
    auto alloc = [&](void **p, size_t bytes) { return hipMalloc(p, std::max<size_t>(bytes, 8)); };
    hipError_t e = hipSuccess;
    auto A = [&](void **p, size_t bytes) { if (e == hipSuccess) e = alloc(p, bytes); };
    A((void **)&d->dSeq, mk * 8); A((void **)&d->dMap, mk * 4); A((void **)&d->dLive, mk); A((void **)&d->dBad, mk); A((void **)&d->dBowOff, mk * 4);
    A((void **)&d->dBowN, mk * 4); A((void **)&d->dCov, mk * kNCov * 4); A((void **)&d->dLastQ, 2 * mk * 8); A((void **)&d->dLastS, 2 * mk * 4);
    A((void **)&d->dPoolW, me * 4); A((void **)&d->dPoolV, me * 8); A((void **)&d->dOff, nw1 * 4); A((void **)&d->dFill, nw1 * 4);
    A((void **)&d->dTileSums, ((nw1 + kScanTile - 1) / kScanTile + 1) * 4); A((void **)&d->dGrand, 4);
    for (int j = 0; j < 2; j++) { A((void **)&d->dPSlot[j], me * 4); A((void **)&d->dPWord[j], me * 4); }
    A((void **)&d->wCount, cells * 4); A((void **)&d->wRank, cells * 4); A((void **)&d->wVal, cells * 4); A((void **)&d->wList, cells * 4);
    A((void **)&d->wKey, cells * 8); A((void **)&d->wSi, cells * 4); A((void **)&d->wAcc, cells * 4); A((void **)&d->wBest, cells * 4);
    A((void **)&d->wOrder, cells * 4); A((void **)&d->qSmall, ((size_t)d->tileQ * 8 + 8) * 4);
    if (e == hipSuccess) e = hipMemset(d->dLive, 0, mk);
    if (e == hipSuccess) e = hipMemset(d->dOff, 0, nw1 * 4);
    if (e != hipSuccess) { kfdb_free(d); delete d; return fail("rumi_kfdb_create: device allocation failed", RUMI_E_NO_DEVICE); }
    *out = d;
    return RUMI_OK;
}

extern "C" int32_t rumi_kfdb_size(const RumiKFDatabase *d) { return d ? d->nLive : 0; }
extern "C" int64_t rumi_kfdb_next_seq(const RumiKFDatabase *d) { return d ? d->nextSeq : 0; }
extern "C" int32_t rumi_kfdb_max_batch(const RumiKFDatabase *d) { return d ? d->tileQ : 0; }

extern "C" int rumi_kfdb_add(RumiKFDatabase *d, int32_t n, const uint64_t *ids, const int32_t *maps, const int32_t *off, const uint32_t *words,
                             const double *values) {
    if (!d || n < 0 || (n > 0 && (!ids || !maps || !off || (off[n] > 0 && (!words || !values))))) return fail("rumi_kfdb_add: bad argument", RUMI_E_INVALID);
    if (d->pendKind >= 0) return fail("rumi_kfdb_add: a scored batch waits for its select", RUMI_E_INVALID);
    std::unordered_set<uint64_t> seen;
    for (int i = 0; i < n; i++) {
        if (off[i + 1] < off[i] || d->slotOf.count(ids[i]) || !seen.insert(ids[i]).second) return fail("rumi_kfdb_add: bad offsets or an id already in the database", RUMI_E_INVALID);
        if (!bow_ok(words + off[i], off[i + 1] - off[i], d->nWords)) return fail("rumi_kfdb_add: BowVector words must be ascending vocabulary word ids", RUMI_E_INVALID);
    }
    const int64_t ne = n ? off[n] - off[0] : 0;
    if (d->nLive + n > d->maxKf) return fail("rumi_kfdb_add: max_kf exceeded", RUMI_E_CAPACITY);
    if (d->liveEntries + ne > d->maxEntries) return fail("rumi_kfdb_add: max_entries exceeded", RUMI_E_CAPACITY);
    for (int i = 0; i < n; i++) {
        const int nb = off[i + 1] - off[i];
        NewKF k = new_kf(d, take_slot(d), ids[i], maps[i], nb);
        k.bowOff = (int32_t)d->stW.size();              // relative to the staged block until the flush
        d->stW.insert(d->stW.end(), words + off[i], words + off[i + 1]);
        d->stV.insert(d->stV.end(), values + off[i], values + off[i + 1]);
        d->staged.push_back(k);
    }
    d->liveEntries += ne;
    return RUMI_OK;
}

extern "C" int rumi_kfdb_add_batch_device(RumiKFDatabase *d, int32_t nf, const uint64_t *ids, const int32_t *maps, const void *d_word, const void *d_weight,
                                          const void *d_counts, int32_t cap, void *stream) {
    if (!d || nf < 0 || cap < 1 || (nf > 0 && (!ids || !maps || !d_word || !d_weight || !d_counts))) return fail("rumi_kfdb_add_batch_device: bad argument", RUMI_E_INVALID);
    if (d->pendKind >= 0) return fail("rumi_kfdb_add_batch_device: a scored batch waits for its select", RUMI_E_INVALID);
    if (nf == 0) return RUMI_OK;
    std::unordered_set<uint64_t> seen;
    for (int i = 0; i < nf; i++)
        if (d->slotOf.count(ids[i]) || !seen.insert(ids[i]).second) return fail("rumi_kfdb_add_batch_device: an id already in the database", RUMI_E_INVALID);
    if (d->nLive + nf > d->maxKf) return fail("rumi_kfdb_add_batch_device: max_kf exceeded", RUMI_E_CAPACITY);
    int rc = flush(d);
    if (rc != RUMI_OK) return rc;
    HIP_TRY(hipSetDevice(d->device));
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    const size_t cells = (size_t)nf * cap;
    if ((rc = ensure(d->asmKey, cells)) || (rc = ensure(d->asmOrder, cells)) || (rc = ensure(d->asmW, cells)) || (rc = ensure(d->asmV, cells)) || (rc = ensure(d->asmN, nf)))
        return rc;
    const int tf = d->weighting == 0 || d->weighting == 1;
    hipLaunchKernelGGL(k_bow_assemble, dim3(nf), dim3(256), 0, nullptr, (const uint32_t *)d_word, (const double *)d_weight, (const int32_t *)d_counts, cap, tf,
                       d->asmKey.p, d->asmOrder.p, d->asmW.p, d->asmV.p, d->asmN.p);
    HIP_TRY(hipGetLastError());
    std::vector<int32_t> nu(nf);
    HIP_TRY(hipMemcpy(nu.data(), d->asmN.p, (size_t)nf * 4, hipMemcpyDeviceToHost));
    int64_t ne = 0;
    for (int v : nu) ne += v;
    if (d->liveEntries + ne > d->maxEntries) return fail("rumi_kfdb_add_batch_device: max_entries exceeded", RUMI_E_CAPACITY);
    if (d->poolTop + ne > d->maxEntries && (rc = compact_pool(d)) != RUMI_OK) return rc;
    std::vector<NewKF> ks;
    std::vector<int32_t> frameOf(nf), dst(nf), slots(nf);
    for (int f = 0; f < nf; f++) {
        NewKF k = new_kf(d, take_slot(d), ids[f], maps[f], nu[f]);
        k.bowOff = (int32_t)d->poolTop;
        d->bowOffH[k.slot] = k.bowOff;
        frameOf[f] = f; dst[f] = k.bowOff; slots[f] = k.slot;
        d->poolTop += nu[f];
        ks.push_back(k);
    }
    d->liveEntries += ne;
    if ((rc = put(d->tmpI, frameOf.data(), nf)) || (rc = put(d->flatSlot, dst.data(), nf))) return rc;
    hipLaunchKernelGGL(k_bow_place, dim3(nf), dim3(256), 0, nullptr, d->tmpI.p, d->flatSlot.p, d->asmN.p, cap, d->asmW.p, d->asmV.p, d->dPoolW, d->dPoolV);
    HIP_TRY(hipGetLastError());
    if ((rc = upload_new(d, ks)) != RUMI_OK) return rc;
    return rebuild(d, slots);
}

extern "C" int rumi_kfdb_bow(RumiKFDatabase *d, uint64_t id, uint32_t *words, double *values, int32_t cap, int32_t *n_out) {
    if (!d || !n_out) return RUMI_E_INVALID;
    *n_out = 0;
    int rc = flush(d);
    if (rc != RUMI_OK) return rc;
    auto it = d->slotOf.find(id);
    if (it == d->slotOf.end()) return fail("rumi_kfdb_bow: unknown key-frame id", RUMI_E_INVALID);
    const int s = it->second, n = d->bowNH[s];
    if (n > cap || (n > 0 && (!words || !values))) return fail("rumi_kfdb_bow: output capacity", RUMI_E_CAPACITY);
    HIP_TRY(hipSetDevice(d->device));
    if (n) {
        HIP_TRY(hipMemcpy(words, d->dPoolW + d->bowOffH[s], (size_t)n * 4, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(values, d->dPoolV + d->bowOffH[s], (size_t)n * 8, hipMemcpyDeviceToHost));
    }
    *n_out = n;
    return RUMI_OK;
}

extern "C" int rumi_kfdb_erase(RumiKFDatabase *d, int32_t n, const uint64_t *ids) {
    if (!d || n < 0 || (n > 0 && !ids)) return RUMI_E_INVALID;
    if (d->pendKind >= 0) return fail("rumi_kfdb_erase: a scored batch waits for its select", RUMI_E_INVALID);
    int rc = flush(d);
    if (rc != RUMI_OK) return rc;
    std::vector<int32_t> slots;
    for (int i = 0; i < n; i++) {
        auto it = d->slotOf.find(ids[i]);
        if (it != d->slotOf.end() && d->liveH[it->second]) { slots.push_back(it->second); d->liveH[it->second] = 2; }   // (2: taken once)
    }
    HIP_TRY(hipSetDevice(d->device));
    return remove_slots(d, slots);
}

extern "C" int rumi_kfdb_clear_map(RumiKFDatabase *d, int32_t map) {
    if (!d) return RUMI_E_INVALID;
    if (d->pendKind >= 0) return fail("rumi_kfdb_clear_map: a scored batch waits for its select", RUMI_E_INVALID);
    int rc = flush(d);
    if (rc != RUMI_OK) return rc;
    std::vector<int32_t> slots;
    for (int s = 0; s < d->hi; s++) if (d->liveH[s] && d->mapH[s] == map) slots.push_back(s);
    HIP_TRY(hipSetDevice(d->device));
    return remove_slots(d, slots);
}

extern "C" int rumi_kfdb_clear(RumiKFDatabase *d) {
    if (!d) return RUMI_E_INVALID;
    if (d->pendKind >= 0) return fail("rumi_kfdb_clear: a scored batch waits for its select", RUMI_E_INVALID);
    int rc = flush(d);
    if (rc != RUMI_OK) return rc;
    std::vector<int32_t> slots;
    for (int s = 0; s < d->hi; s++) if (d->liveH[s]) slots.push_back(s);
    HIP_TRY(hipSetDevice(d->device));
    rc = remove_slots(d, slots);
    if (rc == RUMI_OK) d->poolTop = 0;
    return rc;
}

extern "C" int rumi_kfdb_set_map_bad(RumiKFDatabase *d, int32_t map, int32_t bad) {
    if (!d) return RUMI_E_INVALID;
    if (bad) d->badMaps.insert(map); else d->badMaps.erase(map);
    return RUMI_OK;
}

namespace {
template <class T> int set_per_kf(RumiKFDatabase *d, int n, const uint64_t *ids, const T *vals, int stride, T *dst, std::vector<int32_t> *mirror) {
    if (n < 0 || (n > 0 && (!ids || !vals))) return RUMI_E_INVALID;
    // allowed between score and select (nothing is staged then: adds are refused while a batch is pending); select reads these arrays
    int rc = flush(d);
    if (rc != RUMI_OK) return rc;
    std::vector<int32_t> slots;
    std::vector<T> v;
    for (int i = 0; i < n; i++) {
        auto it = d->slotOf.find(ids[i]);
        if (it == d->slotOf.end()) continue;
        slots.push_back(it->second);
        v.insert(v.end(), vals + (size_t)i * stride, vals + (size_t)(i + 1) * stride);
        if (mirror) (*mirror)[it->second] = (int32_t)vals[i];
    }
    if (slots.empty()) return RUMI_OK;
    HIP_TRY(hipSetDevice(d->device));
    DevBuf<T> tmp;                                                   // released when the function returns, behind the synchronisation
    if ((rc = put(d->tmpI, slots.data(), slots.size())) != RUMI_OK || (rc = put(tmp, v.data(), v.size())) != RUMI_OK) return rc;
    hipLaunchKernelGGL(k_set_at<T>, dim3(blocks(slots.size(), 256)), dim3(256), 0, nullptr, d->tmpI.p, tmp.p, (int)slots.size(), stride, dst);
    HIP_TRY(hipDeviceSynchronize());
    return RUMI_OK;
}
}  // namespace

extern "C" int rumi_kfdb_set_maps(RumiKFDatabase *d, int32_t n, const uint64_t *ids, const int32_t *maps) {
    if (!d) return RUMI_E_INVALID;
    return set_per_kf<int32_t>(d, n, ids, maps, 1, d->dMap, &d->mapH);
}
extern "C" int rumi_kfdb_set_bad(RumiKFDatabase *d, int32_t n, const uint64_t *ids, const uint8_t *bad) {
    if (!d) return RUMI_E_INVALID;
    return set_per_kf<uint8_t>(d, n, ids, bad, 1, d->dBad, nullptr);
}
extern "C" int rumi_kfdb_set_covisibles(RumiKFDatabase *d, int32_t n, const uint64_t *ids, const int64_t *best) {
    if (!d || n < 0 || (n > 0 && (!ids || !best))) return RUMI_E_INVALID;
    int rc = flush(d);                           // (also between score and select: k_q_acc reads the rows in select)
    if (rc != RUMI_OK) return rc;
    std::vector<int32_t> rows((size_t)n * kNCov, -1);
    for (int i = 0; i < n; i++) {
        int k = 0;
        for (int c = 0; c < kNCov; c++) {
            const int64_t id = best[(size_t)i * kNCov + c];
            if (id < 0) continue;
            auto it = d->slotOf.find((uint64_t)id);
            if (it != d->slotOf.end()) rows[(size_t)i * kNCov + k++] = it->second;     // ids not in the database never contribute
        }
    }
    std::vector<uint64_t> ids2;
    std::vector<int32_t> rows2;
    for (int i = 0; i < n; i++)
        if (d->slotOf.count(ids[i])) { ids2.push_back(ids[i]); rows2.insert(rows2.end(), rows.begin() + (size_t)i * kNCov, rows.begin() + (size_t)(i + 1) * kNCov); }
    return set_per_kf<int32_t>(d, (int)ids2.size(), ids2.data(), rows2.data(), kNCov, d->dCov, nullptr);
}

namespace {
QDev qdev(RumiKFDatabase *d) {
    QDev Q;
    Q.nq = d->pendNq; Q.maxKf = d->maxKf; Q.kind = d->pendKind;
    Q.qid = d->qId.p; Q.qmap = d->qMap.p; Q.qvb = d->qVb.p; Q.qBowOff = d->qBowOff.p; Q.qW = d->qW.p; Q.qV = d->qV.p;
    Q.count = d->wCount; Q.rank = d->wRank; Q.val = d->wVal; Q.list = d->wList; Q.key = d->wKey; Q.si = d->wSi; Q.acc = d->wAcc; Q.best = d->wBest;
    Q.order = d->wOrder;
    const int t = d->tileQ;
    Q.maxc = d->qSmall; Q.minc = d->qSmall + t; Q.nsc = d->qSmall + 2 * t; Q.scOff = d->qSmall + 3 * t;   // scOff: t + 1
    return Q;
}
int32_t *q_outN(RumiKFDatabase *d) { return d->qSmall + 4 * d->tileQ + 1; }
int32_t *q_nLoop(RumiKFDatabase *d) { return d->qSmall + 5 * d->tileQ + 1; }
int32_t *q_nMerge(RumiKFDatabase *d) { return d->qSmall + 6 * d->tileQ + 1; }
int32_t *q_nCand(RumiKFDatabase *d) { return d->qSmall + 7 * d->tileQ + 1; }
}  // namespace

extern "C" int rumi_kfdb_score(RumiKFDatabase *d, int32_t kind, int32_t nq, const uint64_t *qid, const int32_t *qmap, const int64_t *vb, const int32_t *bow_off,
                               const uint32_t *bow_w, const double *bow_v, const int32_t *conn_off, const uint64_t *conn_ids, int32_t *scored_off) {
    if (!d || (kind != RUMI_KFDB_RELOC && kind != RUMI_KFDB_NBEST) || nq < 0 || !scored_off || (nq > 0 && (!qid || !qmap || !bow_off)))
        return fail("rumi_kfdb_score: bad argument", RUMI_E_INVALID);
    if (d->pendKind >= 0) return fail("rumi_kfdb_score: the previous scored batch waits for its select", RUMI_E_INVALID);
    if (nq > d->tileQ) return fail("rumi_kfdb_score: more queries than rumi_kfdb_max_batch", RUMI_E_CAPACITY);
    scored_off[0] = 0;
    const int nwt = nq ? bow_off[nq] - bow_off[0] : 0;
    if (nwt > 0 && (!bow_w || !bow_v)) return fail("rumi_kfdb_score: bad argument", RUMI_E_INVALID);
    std::unordered_set<uint64_t> seen;
    for (int q = 0; q < nq; q++) {
        if (bow_off[q + 1] < bow_off[q] || !seen.insert(qid[q]).second) return fail("rumi_kfdb_score: bad offsets or a repeated query id", RUMI_E_INVALID);
        if (!bow_ok(bow_w + bow_off[q], bow_off[q + 1] - bow_off[q], d->nWords)) return fail("rumi_kfdb_score: BowVector words must be ascending vocabulary word ids", RUMI_E_INVALID);
    }
    int rc = flush(d);
    if (rc != RUMI_OK) return rc;
    HIP_TRY(hipSetDevice(d->device));
    // query arrays
    std::vector<int32_t> boff(nq + 1), qow(std::max(nwt, 1));
    std::vector<int64_t> vbs(std::max(nq, 1), INT64_MAX);
    for (int q = 0; q <= nq; q++) boff[q] = bow_off[q] - bow_off[0];
    for (int q = 0; q < nq; q++) { for (int j = boff[q]; j < boff[q + 1]; j++) qow[j] = q; if (vb) vbs[q] = vb[q]; }
    std::vector<int32_t> cq, cs;
    if (kind == RUMI_KFDB_NBEST && conn_off && nq > 0) {
        for (int q = 0; q < nq; q++)
            for (int j = conn_off[q]; j < conn_off[q + 1]; j++) {
                auto it = d->slotOf.find(conn_ids[j]);
                if (it != d->slotOf.end()) { cq.push_back(q); cs.push_back(it->second); }
            }
    }
    if ((rc = put(d->qId, qid, nq)) || (rc = put(d->qMap, qmap, nq)) || (rc = put(d->qVb, vbs.data(), nq)) || (rc = put(d->qBowOff, boff.data(), nq + 1)) ||
        (rc = put(d->qOfWord, qow.data(), nwt)) || (rc = put(d->qW, bow_w ? bow_w + bow_off[0] : nullptr, nwt)) ||
        (rc = put(d->qV, bow_v ? bow_v + bow_off[0] : nullptr, nwt)) || (rc = put(d->connQ, cq.data(), cq.size())) || (rc = put(d->connS, cs.data(), cs.size())))
        return rc;
    d->pendKind = kind; d->pendNq = nq;
    QDev Q = qdev(d);
    const size_t cells = (size_t)nq * d->maxKf;
    if (nq == 0 || d->hi == 0) {
        d->pendScOff.assign(nq + 1, 0);
        for (int q = 0; q <= nq; q++) scored_off[q] = 0;
        HIP_TRY(hipMemset(d->qSmall, 0, ((size_t)d->tileQ * 8 + 8) * 4));
        return RUMI_OK;
    }
    HIP_TRY(hipMemset(d->wCount, 0, cells * 4));
    HIP_TRY(hipMemset(d->wRank, 0xFF, cells * 4));
    HIP_TRY(hipMemset(d->qSmall, 0, ((size_t)d->tileQ * 8 + 8) * 4));
    if (!cq.empty()) hipLaunchKernelGGL(k_q_conn, dim3(blocks(cq.size(), 256)), dim3(256), 0, nullptr, (int)cq.size(), d->connQ.p, d->connS.p, d->maxKf, d->wCount);
    if (nwt > 0) hipLaunchKernelGGL(k_q_count, dim3(blocks(nwt, 4)), dim3(256), 0, nullptr, Q, nwt, d->qOfWord.p, d->dOff, d->dPSlot[d->cur], d->dSeq);
    hipLaunchKernelGGL(k_q_scan1, dim3(blocks(d->hi, 256)), dim3(256), 0, nullptr, Q, d->hi, d->dLive, d->dSeq, d->dLastQ);
    hipLaunchKernelGGL(k_q_gather, dim3(blocks(d->hi, 256), nq), dim3(256), 0, nullptr, Q, d->hi, d->dSeq);
    hipLaunchKernelGGL(k_q_sort, dim3(nq), dim3(256), 0, nullptr, Q);
    HIP_TRY(hipGetLastError());
    std::vector<int32_t> nsc(nq);
    HIP_TRY(hipMemcpy(nsc.data(), Q.nsc, (size_t)nq * 4, hipMemcpyDeviceToHost));
    d->pendScOff.assign(nq + 1, 0);
    for (int q = 0; q < nq; q++) d->pendScOff[q + 1] = d->pendScOff[q] + nsc[q];
    const int total = d->pendScOff[nq];
    HIP_TRY(hipMemcpy(Q.scOff, d->pendScOff.data(), (size_t)(nq + 1) * 4, hipMemcpyHostToDevice));
    if ((rc = ensure(d->flatSlot, total)) || (rc = ensure(d->flatSi, total))) return rc;
    if (total > 0)
        hipLaunchKernelGGL(k_q_si, dim3(blocks(total, 4)), dim3(256), 0, nullptr, Q, total, d->dBowOff, d->dBowN, d->dPoolW, d->dPoolV, d->flatSlot.p, d->flatSi.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    for (int q = 0; q <= nq; q++) scored_off[q] = d->pendScOff[q];
    return RUMI_OK;
}

extern "C" int rumi_kfdb_scored(RumiKFDatabase *d, uint64_t *ids, float *si) {
    if (!d || d->pendKind < 0) return fail("rumi_kfdb_scored: no scored batch", RUMI_E_INVALID);
    const int total = d->pendScOff.empty() ? 0 : d->pendScOff.back();
    if (total == 0) return RUMI_OK;
    if (!ids || !si) return RUMI_E_INVALID;
    std::vector<int32_t> slots(total);
    HIP_TRY(hipSetDevice(d->device));
    HIP_TRY(hipMemcpy(slots.data(), d->flatSlot.p, (size_t)total * 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(si, d->flatSi.p, (size_t)total * 4, hipMemcpyDeviceToHost));
    for (int i = 0; i < total; i++) ids[i] = d->idOf[slots[i]];
    return RUMI_OK;
}

namespace {
int select_common(RumiKFDatabase *d, int kind, QDev *Q) {
    if (d->pendKind != kind) return fail("rumi_kfdb_select: no scored batch of this kind", RUMI_E_INVALID);
    *Q = qdev(d);
    const int total = d->pendScOff.back();
    if (Q->nq == 0 || d->hi == 0) return RUMI_OK;
    HIP_TRY(hipSetDevice(d->device));
    hipLaunchKernelGGL(k_q_scan2, dim3(blocks(d->hi, 256)), dim3(256), 0, nullptr, *Q, d->hi, d->dLastS);
    if (total > 0) hipLaunchKernelGGL(k_q_acc, dim3(blocks(total, 256)), dim3(256), 0, nullptr, *Q, total, d->dCov);
    HIP_TRY(hipGetLastError());
    return RUMI_OK;
}
}  // namespace

extern "C" int rumi_kfdb_select_reloc(RumiKFDatabase *d, int32_t *cand_off, uint64_t *cand_ids, int64_t cap) {
    if (!d || !cand_off) return RUMI_E_INVALID;
    QDev Q;
    int rc = select_common(d, RUMI_KFDB_RELOC, &Q);
    if (rc != RUMI_OK) return rc;
    const int nq = d->pendNq, total = d->pendScOff.back();
    d->pendKind = -1;
    cand_off[0] = 0;
    if (nq == 0) return RUMI_OK;
    if (total == 0 || d->hi == 0) { for (int q = 0; q <= nq; q++) cand_off[q] = 0; return RUMI_OK; }
    if ((rc = ensure(d->outSlot, total)) != RUMI_OK) return rc;
    hipLaunchKernelGGL(k_q_reloc, dim3(nq), dim3(256), 0, nullptr, Q, d->dMap, d->outSlot.p, q_outN(d));
    HIP_TRY(hipGetLastError());
    std::vector<int32_t> n(nq), slots(total);
    HIP_TRY(hipMemcpy(n.data(), q_outN(d), (size_t)nq * 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(slots.data(), d->outSlot.p, (size_t)total * 4, hipMemcpyDeviceToHost));
    int64_t k = 0;
    for (int q = 0; q < nq; q++) {
        if (k + n[q] > cap || (n[q] > 0 && !cand_ids)) return fail("rumi_kfdb_select_reloc: output capacity", RUMI_E_CAPACITY);
        for (int j = 0; j < n[q]; j++) cand_ids[k++] = d->idOf[slots[d->pendScOff[q] + j]];
        cand_off[q + 1] = (int32_t)k;
    }
    return RUMI_OK;
}

extern "C" int rumi_kfdb_select_nbest(RumiKFDatabase *d, const int32_t *n_cand, int32_t stride, int32_t *n_loop, uint64_t *loop_ids, int32_t *n_merge,
                                      uint64_t *merge_ids) {
    if (!d || (d->pendNq > 0 && (!n_cand || !n_loop || !n_merge || stride < 0 || (stride > 0 && (!loop_ids || !merge_ids))))) return RUMI_E_INVALID;
    for (int q = 0; q < d->pendNq; q++) if (n_cand[q] < 0 || n_cand[q] > stride) return fail("rumi_kfdb_select_nbest: n_cand must be in 0..stride", RUMI_E_INVALID);
    QDev Q;
    int rc = select_common(d, RUMI_KFDB_NBEST, &Q);
    if (rc != RUMI_OK) return rc;
    const int nq = d->pendNq, total = d->pendScOff.back();
    d->pendKind = -1;
    for (int q = 0; q < nq; q++) { n_loop[q] = 0; n_merge[q] = 0; }
    if (nq == 0 || total == 0 || d->hi == 0 || stride == 0) return RUMI_OK;
    std::vector<int32_t> bm(d->badMaps.begin(), d->badMaps.end());
    if ((rc = ensure(d->loopS, (size_t)nq * stride)) || (rc = ensure(d->mergeS, (size_t)nq * stride)) || (rc = put(d->badM, bm.data(), bm.size()))) return rc;
    HIP_TRY(hipMemcpy(q_nCand(d), n_cand, (size_t)nq * 4, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_q_nbest, dim3(nq), dim3(256), 0, nullptr, Q, d->dMap, d->dBad, d->badM.p, (int)bm.size(), q_nCand(d), stride, d->loopS.p, q_nLoop(d),
                       d->mergeS.p, q_nMerge(d));
    HIP_TRY(hipGetLastError());
    std::vector<int32_t> ls((size_t)nq * stride), ms((size_t)nq * stride);
    HIP_TRY(hipMemcpy(n_loop, q_nLoop(d), (size_t)nq * 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(n_merge, q_nMerge(d), (size_t)nq * 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(ls.data(), d->loopS.p, ls.size() * 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(ms.data(), d->mergeS.p, ms.size() * 4, hipMemcpyDeviceToHost));
    for (int q = 0; q < nq; q++) {
        for (int j = 0; j < n_loop[q]; j++) loop_ids[(size_t)q * stride + j] = d->idOf[ls[(size_t)q * stride + j]];
        for (int j = 0; j < n_merge[q]; j++) merge_ids[(size_t)q * stride + j] = d->idOf[ms[(size_t)q * stride + j]];
    }
    return RUMI_OK;
}
