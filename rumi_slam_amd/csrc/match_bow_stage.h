// The two BoW batch stages, each body stated once for the entry that packs host pointers into a block and for the entry that reads the
// covisibility store by slot (the idiom of mapping.hip's k_newpts_*<View>):
//   k_bowf_match       SearchByBoW(KF_k, F) of K key-frames against one frame      rumi_search_by_bow_batch (match.hip), rumi_track_reloc_bow (track.hip)
//   k_cr_match         SearchByBoW(current key-frame, member) of every member      rumi_common_regions_bow (match.hip),
//   k_cr_union         the union of every group's matched map points               rumi_common_regions_bow_resident (mapping.hip)
//   k_bow_rows_finish  ComputeThreeMaxima and the count of every row of either stage
// A kernel reads a key-frame through a view: view.kf(i) names the arrays of row i's key-frame, wherever the bytes lie.  The library is built without
// relocatable device code, so every instantiation belongs to ONE translation unit; the view types are what keeps them apart:
//   PackedView, PackedCrView   match.hip     arrays at blk + dword offset, one BowPackedKF a key-frame
//   SlotView                   track.hip     a CovisFeatRec in the feature arena and a row in the row arena, one BowSlotKF a row
//   SlotCrView                 mapping.hip   the same, with the current key-frame and the group starts
// Below the kernels: what the two common-regions entries share on the host.
#pragma once
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdint>
#include <cstring>

#include "match_bow.h"
#include "rumi_common.h"
#include "covis_view.h"

namespace rumi {

// ---- key-frame views ----------------------------------------------------------------------------------------------------------------------
struct BowPackedKF { int32_t n, nn, angle, desc, mp, good, nodes, off, idx, pad; };      // sizes and dword offsets of one key-frame's arrays in the block
struct BowSlotKF : CovisSlotRef { int32_t bad; };            // one row; bad: named, not searched
static_assert(sizeof(BowSlotKF) == 24, "the slot table as uploaded");

// angle of feature i / "feature i holds a map point that is not bad" (ORBmatcher.cc:238-243, :717-721, :738-742), as either side keeps them
struct PackedAngles { const float *p; __device__ __forceinline__ float operator[](int i) const { return p[i]; } };
struct PackedGood { const uint8_t *p; __device__ __forceinline__ bool operator[](int i) const { return p[i] != 0; } };
struct SlotAngles { const RumiKeyPoint *p; __device__ __forceinline__ float operator[](int i) const { return p[i].angle; } };
struct SlotGood {                                            // read in the store: row entry >= 0 and the point's bad bit clear
    const int32_t *row; CovisView s;
    __device__ __forceinline__ bool operator[](int i) const { const int p = row[i]; return p >= 0 && !s.point_bad(p); }
};

struct PackedKF {
    const uint32_t *blk; const BowPackedKF *t;
    __device__ __forceinline__ int n() const { return t->n; }
    __device__ __forceinline__ int nn() const { return t->nn; }
    __device__ __forceinline__ const uint32_t *nodes() const { return blk + t->nodes; }
    __device__ __forceinline__ const int32_t *off() const { return reinterpret_cast<const int32_t *>(blk + t->off); }
    __device__ __forceinline__ const uint32_t *idx() const { return blk + t->idx; }
    __device__ __forceinline__ const uint32_t *desc() const { return blk + t->desc; }
    __device__ __forceinline__ const int32_t *mp() const { return reinterpret_cast<const int32_t *>(blk + t->mp); }
    __device__ __forceinline__ PackedAngles angles() const { return PackedAngles{reinterpret_cast<const float *>(blk + t->angle)}; }
    __device__ __forceinline__ PackedGood good() const { return PackedGood{reinterpret_cast<const uint8_t *>(blk + t->good)}; }
    __device__ __forceinline__ bool bad() const { return false; }
};
struct SlotKF : CovisKeyFrame {                              // sizes from the table row: nothing behind r is read before bad() has said no
    CovisView s; int32_t n_, nn_, bad_;
    __device__ __forceinline__ int n() const { return n_; }
    __device__ __forceinline__ int nn() const { return nn_; }
    __device__ __forceinline__ const uint32_t *desc() const { return rec_arr<uint32_t>(r, r->desc); }
    __device__ __forceinline__ SlotAngles angles() const { return SlotAngles{keys()}; }
    __device__ __forceinline__ SlotGood good() const { return SlotGood{row, s}; }
    __device__ __forceinline__ bool bad() const { return bad_ != 0; }
};

struct PackedView {
    using KF = PackedKF;
    const uint32_t *blk;          // the uploaded block (dword view)
    int kfTable;                  // dword offset of the BowPackedKF table
    __device__ __forceinline__ KF kf(int k) const { return KF{blk, reinterpret_cast<const BowPackedKF *>(blk + kfTable) + k}; }
};
struct PackedCrView : PackedView {                           // row = member: the table entry its index names; the current key-frame by value
    BowPackedKF curKf;
    int memKf, groupStart;        // dword offsets
    __device__ __forceinline__ KF kf(int mem) const { return PackedView::kf(reinterpret_cast<const int32_t *>(blk + memKf)[mem]); }
    __device__ __forceinline__ KF cur() const { return KF{blk, &curKf}; }
    __device__ __forceinline__ const int32_t *group_start() const { return reinterpret_cast<const int32_t *>(blk + groupStart); }
};
struct SlotView {
    using KF = SlotKF;
    const BowSlotKF *tab;         // [rows]
    CovisView s;                  // read through: key_frame, point_bad
    __device__ __forceinline__ KF of(const BowSlotKF &T) const { return KF{s.key_frame(T), s, T.n, T.nn, T.bad}; }
    __device__ __forceinline__ KF kf(int k) const { return of(tab[k]); }
};
struct SlotCrView : SlotView {
    BowSlotKF curKf;
    const int32_t *groupStart;    // [nG + 1]
    __device__ __forceinline__ KF cur() const { return of(curKf); }
    __device__ __forceinline__ const int32_t *group_start() const { return groupStart; }
};

// The frame of SearchByBoW(KF, F): in the block for the host-pointer entry, in the tracker's buffers (its FeatureVector built on the device, the
// node count with it) for the by-slot entry.
struct PackedFrame {
    const uint32_t *blk;
    int nnF, fAngle, fDesc, fNodes, fOff, fIdx;              // node count; dword offsets
    __device__ __forceinline__ int nn() const { return nnF; }
    __device__ __forceinline__ const uint32_t *nodes() const { return blk + fNodes; }
    __device__ __forceinline__ const int32_t *off() const { return reinterpret_cast<const int32_t *>(blk + fOff); }
    __device__ __forceinline__ const uint32_t *idx() const { return blk + fIdx; }
    __device__ __forceinline__ const uint32_t *desc() const { return blk + fDesc; }
    __device__ __forceinline__ PackedAngles angles() const { return PackedAngles{reinterpret_cast<const float *>(blk + fAngle)}; }
};
struct ResidentFrame {
    const RumiKeyPoint *keys;
    const uint32_t *fDesc, *fNodes, *fIdx;
    const int32_t *fOff, *fNN;
    __device__ __forceinline__ int nn() const { return fNN[0]; }
    __device__ __forceinline__ const uint32_t *nodes() const { return fNodes; }
    __device__ __forceinline__ const int32_t *off() const { return fOff; }
    __device__ __forceinline__ const uint32_t *idx() const { return fIdx; }
    __device__ __forceinline__ const uint32_t *desc() const { return fDesc; }
    __device__ __forceinline__ SlotAngles angles() const { return SlotAngles{keys}; }
};

// ---- the rows of a stage: one per key-frame (k_bowf_match) or member (k_cr_match) -----------------------------------------------------------
struct BowRows {
    int32_t *matches;             // [rows][n]  -1 none
    int8_t *rotBin;               // [rows][n]
    int32_t *hist;                // [rows][32]
    int32_t *nmatch;              // [rows]
    int n;                        // features of the side the rows are indexed by: the frame, the current key-frame
    float nnratio;
    int checkOri;
};

// A lane's `taken` flags for a node of nc candidates.  TakenMask: one register, nodes of up to 512.  TakenLds: word w of thread t at
// sTaken[w * 256 + t], as many words as the node asks for (the launch sizes the dynamic LDS for the largest node of the call); a lane clears and
// reads its own words only.
constexpr int kTakenMaskNode = 512;
static inline size_t taken_lds_bytes(int maxNode) { return (size_t)std::max(1, ((maxNode + 15) / 16 + 31) / 32) * 256 * 4; }
// A match kernel of a host-pointer entry, whose host knows the largest candidate-side node of the call: the TakenMask instantiation without
// dynamic LDS up to 512 features, the TakenLds one above.  (The by-slot entries size TakenLds by feature counts: their node sizes lie on the device.)
template <class... Args>
static inline hipError_t launch_match_by_node(void (*mask)(Args...), void (*inLds)(Args...), int maxNode, dim3 grid, Args... args) {
    if (maxNode <= kTakenMaskNode) { hipLaunchKernelGGL(mask, grid, dim3(256), 0, nullptr, args...); return hipSuccess; }
    const size_t lds = taken_lds_bytes(maxNode);
    if (lds > 64 * 1024) { const hipError_t e = raise_lds_limit(reinterpret_cast<const void *>(inLds), lds); if (e != hipSuccess) return e; }
    hipLaunchKernelGGL(inLds, grid, dim3(256), lds, nullptr, args...);
    return hipSuccess;
}
template <class Taken> __device__ __forceinline__ Taken taken_for_node(int nc);
template <> __device__ __forceinline__ TakenMask taken_for_node<TakenMask>(int) { return TakenMask{}; }
template <> __device__ __forceinline__ TakenLds taken_for_node<TakenLds>(int nc) {
    extern __shared__ uint32_t sTaken[];                      // [words][256]
    TakenLds taken{sTaken + threadIdx.x};
    const int words = ((nc + 15) / 16 + 31) / 32;
    for (int w = 0; w < words; w++) taken.w[w * 256] = 0;
    return taken;
}

// ---- SearchByBoW(KF_k, F) -----------------------------------------------------------------------------------------------------------------
// K candidate key-frames against ONE frame in one launch (Tracking::Relocalization walks the candidates of
// KeyFrameDatabase::DetectRelocalizationCandidates one by one, Tracking.cc:3240-3260; every walk starts from an empty vpMapPointMatches, so the
// K searches are independent).  Within one search a frame feature is taken by the first query that wins it -- but a frame feature lies in
// exactly ONE FeatureVector node, so that dependency never leaves a node: nodes run in parallel, the (few) key-frame features of a node
// sequentially.  16 lanes per (key-frame, node): the lanes share out the frame's features of the node, compute their Hamming distances
// to the current key-frame feature in parallel and reduce (best, second) with the reference's tie rules (ORBmatcher.cc:252-289): bow_node_walk.
// The output is the key-frame feature's map point at the frame feature's place.
template <class View, class Frame, class Taken> __global__ __launch_bounds__(256) void k_bowf_match(View V, Frame F, BowRows R) {
    const int k = blockIdx.y, lane = threadIdx.x & 15, a = blockIdx.x * 16 + (threadIdx.x >> 4);
    const typename View::KF K = V.kf(k);
    if (K.bad() || a >= K.nn()) return;
    const int lo = fv_find_node(F.nodes(), F.nn(), K.nodes()[a]);
    if (lo < 0) return;
    const int32_t *fOff = F.off(), *kOff = K.off();
    const int c0 = fOff[lo], nc = fOff[lo + 1] - c0;
    const uint32_t *fIdx = F.idx() + c0;
    const int32_t *kMp = K.mp();
    const auto kGood = K.good();
    const auto kAngle = K.angles();
    const auto fAngle = F.angles();
    Taken taken = taken_for_node<Taken>(nc);                 // a frame feature that already holds a map point
    bow_node_walk<false>(lane, K.idx(), kOff[a], kOff[a + 1], K.desc(), fIdx, nc, F.desc(), R.nnratio, taken,
                         [&](int iKF) { return kGood[iKF]; },                                // no map point, or a bad one (:238-243)
                         [&](int iKF, int f) {
                             R.matches[(size_t)k * R.n + f] = kMp[iKF];
                             if (R.checkOri) {
                                 const int bin = rot_bin(kAngle[iKF], fAngle[f]);
                                 R.rotBin[(size_t)k * R.n + f] = (int8_t)bin;
                                 atomicAdd(&R.hist[k * 32 + bin], 1);
                             }
                         });
}

// ---- SearchByBoW(current key-frame, member) -----------------------------------------------------------------------------------------------
// LoopClosing::DetectCommonRegionsFromBoW (LoopClosing.cc:542-853; the same text at CloudMerging.cc:985-1294) matches the current key-frame against a
// candidate and its best covisibles one SearchByBoW(KF, KF) at a time (:622-633) and folds the match vectors through a std::set (:635-651).  Every
// search starts from an empty vbMatched2, so the searches are independent; inside one search "a member feature is taken by the first query that wins it"
// never leaves a FeatureVector node (a feature lies in exactly one node).  So: grid over (node of the current key-frame, member), 16 lanes per pair;
// the current key-frame's features of the node run in list order, the lanes share out the member's features of the node and reduce (best, second)
// with the (dist << 16 | position) key: bow_node_walk, which k_bowf_match calls with the roles swapped.  What this caller passes: the query side is the
// one current key-frame, BOTH sides carry a "holds a good map point" gate (ORBmatcher.cc:717-721, :736-742), acceptance is bestDist1 < TH_LOW (strict,
// :757) and the output is the member's FEATURE index.  A bad member (by slot only) is named but not searched: its row stays -1.
template <class View, class Taken> __global__ __launch_bounds__(256) void k_cr_match(View V, BowRows R) {
    const int mem = blockIdx.y, lane = threadIdx.x & 15, a = blockIdx.x * 16 + (threadIdx.x >> 4);
    const typename View::KF C = V.cur(), K = V.kf(mem);
    if (K.bad() || a >= C.nn()) return;
    const int lo = fv_find_node(K.nodes(), K.nn(), C.nodes()[a]);
    if (lo < 0) return;
    const int32_t *cOff = C.off(), *kOff = K.off();
    const int c0 = kOff[lo], nc = kOff[lo + 1] - c0;
    const uint32_t *kIdx = K.idx() + c0;
    const auto kGood = K.good(), cGood = C.good();
    const auto kAngle = K.angles(), cAngle = C.angles();
    Taken taken = taken_for_node<Taken>(nc);                 // a member feature that is matched already, or holds no good map point (:738-742)
    for (int j = 0, pos = lane; pos < nc; j++, pos += 16)
        if (!kGood[kIdx[pos]]) taken.set(j);
    bow_node_walk<true>(lane, C.idx(), cOff[a], cOff[a + 1], C.desc(), kIdx, nc, K.desc(), R.nnratio, taken,           // strict: :757-758
                        [&](int iC) { return cGood[iC]; },                                  // no map point, or a bad one (:717-721)
                        [&](int iC, int f) {
                            R.matches[(size_t)mem * R.n + iC] = f;
                            if (R.checkOri) {
                                // (angles of real key-points give bins 0..12; the clamp keeps a malformed angle inside the histogram)
                                const int bin = min(max(rot_bin(cAngle[iC], kAngle[f]), 0), RUMI_HISTO_LENGTH - 1);
                                R.rotBin[(size_t)mem * R.n + iC] = (int8_t)bin;
                                atomicAdd(&R.hist[mem * 32 + bin], 1);
                            }
                        });
}

// rotation-histogram filter (ComputeThreeMaxima, ORBmatcher.cc:1795-1826) and the match count of every row.  A match the histogram removes has
// kept its candidate taken during the search, as in the reference, where the filter runs after the walk (:786-801).  The count of a bad
// key-frame (Tracking.cc:3245), whose row the clear left at -1, is -1; the packed view has no such row.
template <class View> __global__ __launch_bounds__(256) void k_bow_rows_finish(View V, BowRows R) {
    const int row = blockIdx.x;
    if (V.kf(row).bad()) { if (threadIdx.x == 0) R.nmatch[row] = -1; return; }
    bow_finish(R.matches + (size_t)row * R.n, R.rotBin + (size_t)row * R.n, R.hist + row * 32, R.n, R.checkOri, &R.nmatch[row]);
}

// ---- the union of a group -----------------------------------------------------------------------------------------------------------------
// first[g][point]: the smallest key j * n + k among the surviving matches of group g that hold the point.  Two forms of the table:
//   FirstCleared  int32 words the call has set to kCrNever; atomicMin, and a plain read behind the barrier
//   FirstStamped  64-bit words that are never cleared between calls: atomicMax of (epoch << 32) | (0x7FFFFFFF - key), so the smallest key of THIS
//                 call wins and whatever an earlier call left (a smaller epoch) loses to any stamp of this one; read back through an atomic load
//                 behind the barrier, so the value read is the one every lane's atomicMax has settled on
constexpr int32_t kCrNever = 0x7F7F7F7F;                     // what a byte-wise memset of 0x7F leaves: above every j * n + k the entry admits
struct FirstCleared {
    int32_t *tab; size_t stride;                             // [nG][stride]
    __device__ __forceinline__ void claim(int g, int p, int key) const { atomicMin(&tab[(size_t)g * stride + p], key); }
    __device__ __forceinline__ bool won(int g, int p, int key) const { return tab[(size_t)g * stride + p] == key; }
};
struct FirstStamped {
    unsigned long long *tab; size_t stride; uint32_t epoch;
    __device__ __forceinline__ unsigned long long stamp(int key) const { return ((unsigned long long)epoch << 32) | (uint32_t)(0x7FFFFFFF - key); }
    __device__ __forceinline__ void claim(int g, int p, int key) const { atomicMax(&tab[(size_t)g * stride + p], stamp(key)); }
    __device__ __forceinline__ bool won(int g, int p, int key) const {
        return __hip_atomic_load(&tab[(size_t)g * stride + p], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == stamp(key);
    }
};
struct CrGroups {
    int32_t *mpoint, *mmember;    // [nG][n]
    int32_t *numBow;              // [nG]
    int32_t *most;                // [nG][2]
    int32_t *winner;              // [nG][n]  largest j whose match at k was a first occurrence, -1 none
};

// The union of one group (LoopClosing.cc:635-651 walks j ascending, then k ascending): one workgroup per group, integer atomics only, so the
// outcome does not depend on the order in which the lanes arrive.
//   A  first[point] = min over the surviving matches of j * n + k        = the (j, k) at which the literal loop inserts the point into its set
//   B  a match whose key equals first[point] is that insertion: it counts, and winner[k] = max j over the insertions at k (a later insertion at
//      the same k overwrites vpMatchedPoints[k]; the count keeps both)
//   C  every k writes the point and the member of its winner
// and the member with the most matches (:628-632, strictly greater: the first j wins a tie; 0, 0 when no member matched anything).
// A bad member's row is all -1 and its count -1: it adds nothing, wins nothing, and keeps its position j.
template <class View, class First> __global__ __launch_bounds__(1024) void k_cr_union(View V, BowRows R, CrGroups U, First first) {
    __shared__ int sCount;
    const int g = blockIdx.x, tid = threadIdx.x;
    const int32_t *groupStart = V.group_start();
    const int m0 = groupStart[g], nmem = groupStart[g + 1] - m0;
    int32_t *winner = U.winner + (size_t)g * R.n;
    if (tid == 0) sCount = 0;
    // member j's match vector and the map points of its key-frame's features: the loops run j outside (uniform), k over the lanes, so that a
    // lane's loads of different members do not wait for one another
    auto row_of = [&](int j) { return R.matches + (size_t)(m0 + j) * R.n; };
    auto points_of = [&](int j) { return V.kf(m0 + j).mp(); };
    for (int j = 0; j < nmem; j++) {
        const int32_t *row = row_of(j), *mp = points_of(j);
        for (int k = tid; k < R.n; k += 1024) {
            const int f = row[k];
            if (f >= 0) first.claim(g, mp[f], j * R.n + k);
        }
    }
    __syncthreads();
    int local = 0;
    for (int j = 0; j < nmem; j++) {
        const int32_t *row = row_of(j), *mp = points_of(j);
        for (int k = tid; k < R.n; k += 1024) {
            const int f = row[k];
            if (f >= 0 && first.won(g, mp[f], j * R.n + k)) { local++; atomicMax(&winner[k], j); }
        }
    }
    if (local) atomicAdd(&sCount, local);
    __syncthreads();
    for (int k = tid; k < R.n; k += 1024) {
        const int j = __hip_atomic_load(&winner[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        U.mpoint[(size_t)g * R.n + k] = j < 0 ? -1 : points_of(j)[row_of(j)[k]];
        U.mmember[(size_t)g * R.n + k] = j;
    }
    if (tid == 0) {
        int most = 0, at = 0;
        for (int j = 0; j < nmem; j++) if (R.nmatch[m0 + j] > most) { most = R.nmatch[m0 + j]; at = j; }
        U.numBow[g] = sCount; U.most[2 * g] = at; U.most[2 * g + 1] = most;
    }
}

// ---- host: what rumi_common_regions_bow and rumi_common_regions_bow_resident share --------------------------------------------------------
// The groups: ascending starts from 0, at most 65535 members.  Returns what is wrong, or nullptr with the largest group and the member count.
static inline const char *cr_groups_check(int nG, const int32_t *group_start, int *maxGroup, int *nM) {
    if (group_start[0] != 0) return "group_start must begin at 0";
    *maxGroup = 0;
    for (int g = 0; g < nG; g++) {
        if (group_start[g + 1] < group_start[g]) return "group_start is not ascending";
        *maxGroup = std::max(*maxGroup, group_start[g + 1] - group_start[g]);
    }
    *nM = group_start[nG];
    return *nM > 65535 ? "more than 65535 members" : nullptr;
}

// The six result arrays of either entry (matches12 may be NULL for the by-slot entry only).
struct CrOutputs { int32_t *matches12, *nmatches, *matched_point, *matched_member, *num_bow_matches, *most_matches; };

// Nothing to search (no member, or a current key-frame without features): the literal loop leaves every vector NULL.  bad: the by-slot entry's
// members that are named but bad (count -1), or NULL.
static inline void cr_fill_nothing(int n, int nM, int nG, const uint8_t *bad, const CrOutputs &o) {
    if (o.matches12) for (size_t i = 0; i < (size_t)nM * n; i++) o.matches12[i] = -1;
    for (int i = 0; i < nM; i++) o.nmatches[i] = bad && bad[i] ? -1 : 0;
    for (size_t i = 0; i < (size_t)nG * n; i++) o.matched_point[i] = o.matched_member[i] = -1;
    for (int g = 0; g < nG; g++) o.num_bow_matches[g] = o.most_matches[2 * g] = o.most_matches[2 * g + 1] = 0;
}

// The result block (ints): [hist nM 32 | nmatch nM] zeroed, [numBow G | most 2 G | mpoint G n | mmember G n] written in full by the union,
// [matches nM n | winner G n] = -1.  nmatch .. matches comes back with one copy (.. mmember when the members' rows are not asked for).
struct CrResultLayout {
    size_t nM, G, n, iHist, iNm, iNum, iMost, iPoint, iMember, iMatches, iWinner, iEnd;
    CrResultLayout(int nM_, int nG, int n_)
        : nM((size_t)nM_), G((size_t)nG), n((size_t)n_), iHist(0), iNm(iHist + nM * 32), iNum(iNm + nM), iMost(iNum + G), iPoint(iMost + 2 * G),
          iMember(iPoint + G * n), iMatches(iMember + G * n), iWinner(iMatches + nM * n), iEnd(iWinner + G * n) {}
    hipError_t clear(int32_t *d) const {
        const hipError_t e = hipMemsetAsync(d + iHist, 0, (iNum - iHist) * 4, nullptr);
        return e != hipSuccess ? e : hipMemsetAsync(d + iMatches, 0xFF, (iEnd - iMatches) * 4, nullptr);
    }
    void bind(int32_t *d, BowRows *R, CrGroups *U) const {
        R->hist = d + iHist; R->nmatch = d + iNm; R->matches = d + iMatches; R->n = (int)n;
        U->numBow = d + iNum; U->most = d + iMost; U->mpoint = d + iPoint; U->mmember = d + iMember; U->winner = d + iWinner;
    }
    size_t back_end(bool withMatches) const { return withMatches ? iWinner : iMatches; }     // the copy back runs from iNm to here
    void unpack(const int32_t *h, const CrOutputs &o) const {                                 // h: the block's host mirror, from index 0
        std::memcpy(o.nmatches, h + iNm, nM * 4);
        std::memcpy(o.num_bow_matches, h + iNum, G * 4);
        std::memcpy(o.most_matches, h + iMost, 2 * G * 4);
        std::memcpy(o.matched_point, h + iPoint, G * n * 4);
        std::memcpy(o.matched_member, h + iMember, G * n * 4);
        if (o.matches12) std::memcpy(o.matches12, h + iMatches, nM * n * 4);
    }
};

}  // namespace rumi
