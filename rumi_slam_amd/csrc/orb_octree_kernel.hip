// On-device quadtree key-point distribution + output slot assignment (gfx950).
//
//   k_octree    one workgroup per (frame, level): DistributeOctTree, R/lib_src/ORBextractor.cc:538-724.
//               Keys stay where the FAST kernel left them (cand[], HBM/L2; in registers for a handful of frames).  The node pool, the list
//               (an array in list order), the open/sort arrays live in LDS.  The quadrant counts of the first 4-6 subdivision levels come
//               from ONE histogram pass over the keys (count tables); only a tree that outgrows them relabels keys and counts round by
//               round (a 16-bit owner id per key then, owner[]).  The list passes (divide, push children to the front, erase parents) are
//               prefix sums + scatters -- on one wave without barriers while the list is short -- and std::sort is replayed exactly
//               (wave_sort_like_libstdcxx up to 64 entries, wg_sort_like_libstdcxx beyond), so the result ORDER equals the reference's.
//   k_octree_narrow, k_octree_redo, k_oct_select   batches: the same trees with ONE wave each, from the cell histogram k_compact counts; the keys
//               are read once, by k_oct_select; a tree that outgrows the count tables is redone by k_octree's keys-in-memory form (below,
//               "the batch pipeline")
//   k_assemble  one workgroup per frame: concatenates the levels and assigns the output slot of every key-point
//               by the lapping-area rule of operator() (:1067-1088) with a block scan (the reference walks them
//               serially with monoIndex++ / stereoIndex--).
//
// One translation unit.  This file holds the quadtree (k_octree, launch_octree, octree_lds_for) and what the parts share, and includes:
//   orb_sort_replay.inc  wg_sort_like_libstdcxx, wave_sort_like_libstdcxx: the replays of std::sort; k_sort_hook, launch_sort_hook (the test hook)
//   orb_assemble.inc     k_assemble, launch_assemble
#include <hip/hip_runtime.h>

#include "orb_device.h"
#include "rumi_common.h"
#include "orb_octree.h"

namespace rumi {

constexpr int kOctThreads = 512;

// (pool size, count tables and the per-coordinate path rule: orb_octree.h, shared with set_geometry)
// LDS bytes of one k_octree workgroup for a pool of `cap` nodes: nodes, open + sort arrays, free stack, split stack, two list arrays,
// two SortSeg work lists, the count tables and the cell -> leaf table
// (W, H: the level's key-point area; the two per-coordinate path tables have W + 1 and H + 1 entries; the narrow kernel has none: -1, -1)
__host__ __device__ inline size_t octree_lds_bytes(int cap, int nIni, int D, int W, int H) {
    return (size_t)cap * (sizeof(OctNode) + 2 * sizeof(OctEntry) + 4 * sizeof(uint16_t)) + 2 * (size_t)(cap / 16 + 2) * 8 + 64 +
           ((size_t)(oct_tab_entries(nIni, D) + oct_leaf_entries(nIni, D) + W + H + 4) * sizeof(uint16_t) + 16);
}

// A value every lane holds (read from LDS, or the total of a scan) moves to a scalar register: the control state of the rounds would
// otherwise sit in VGPRs for the whole kernel.
__device__ __forceinline__ int uni(int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ unsigned long long uni64(unsigned long long v) {
    return ((unsigned long long)(unsigned int)__builtin_amdgcn_readfirstlane((int)(v >> 32)) << 32) | (unsigned int)__builtin_amdgcn_readfirstlane((int)v);
}

// exclusive scan of one 64-bit value per thread over the workgroup (three packed 20-bit counters); *total = sum over all threads
template <int NT>
__device__ __forceinline__ unsigned long long block_scan64(unsigned long long v, unsigned long long *sWave, unsigned long long *total) {
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    unsigned long long inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned long long t = __shfl_up(inc, o);
        if (lane >= o) inc += t;
    }
    if (lane == 63) sWave[wave] = inc;
    __syncthreads();
    unsigned long long base = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < NT / 64; w++) {
        const unsigned long long t = sWave[w];
        if (w < wave) base += t;
        tot += t;
    }
    __syncthreads();
    *total = uni64(tot);
    return base + inc - v;
}

}  // namespace rumi

#include "orb_sort_replay.inc"

namespace rumi {

struct OctLds {
    OctNode *nodes;
    OctEntry *open, *prev;
    uint16_t *freeIds, *splitIds, *listA, *listB;
    SortSeg *segA, *segB;
    uint16_t *tab, *leaf;      // count tables T_0 .. T_D; cell of depth D -> id of the list node that covers it
    uint16_t *xbin, *ybin;     // the x half (with the root) and the y half of the depth-D path of a key, by coordinate
    int D, nIni;
};
// The kernel keeps the list as arrays, so the link fields of a node are free: they hold its place in the subdivision.
__device__ __forceinline__ uint16_t &node_path(OctNode &nd) { return nd.next; }
__device__ __forceinline__ uint16_t &node_depth(OctNode &nd) { return nd.prev; }

// DivideNode + the push_front block after it (ORBextractor.cc:471-522, :603-637) for ONE parent, given where its children land:
// g0 = creation index of its first child in this round (the list receives children in REVERSE creation order, because every
// child is pushed to the front), o0 = index of its first child with more than one key in vSizeAndPointerToNode.
// table: children of depth < D take their quadrant counts from the count tables; the return value says that a child of depth D with more
// than one key was created (its counts need a pass over the keys).  SOLO: the caller returns the parent to the free stack itself.
// Everything that is read is read first, in a handful of wide LDS loads that are in flight together: the stores may alias any of it as far
// as the compiler knows, and one dependent LDS round trip (~130 cycles) per quadrant is what the list passes used to spend their time on.
template <bool SOLO>
__device__ __forceinline__ bool emit_children(const OctLds &S, int id, int g0, int o0, int K, int freeTop, uint16_t *newList,
                                              int *sNSplit, bool table) {
    OctNode &p = S.nodes[id];
    const uint4 plo = reinterpret_cast<const uint4 *>(&p)[0];               // x0 y0 | x1 y1 | path depth | n noMore split
    const uint2 pcn = *reinterpret_cast<const uint2 *>(&p.cnt[0]);
    const int x0 = (int)(plo.x & 0xFFFFu), y0 = (int)(plo.x >> 16), x1 = (int)(plo.y & 0xFFFFu), y1 = (int)(plo.y >> 16);
    const int dc = (int)(plo.z >> 16) + 1, pc0 = (int)(plo.z & 0xFFFFu) * 4;
    const int hx = (x1 - x0 + 1) >> 1, hy = (y1 - y0 + 1) >> 1;            // ceil(float(d)/2)
    const int xs[3] = {x0, x0 + hx, x1}, ys[3] = {y0, y0 + hy, y1};
    const int cnt[4] = {(int)(pcn.x & 0xFFFFu), (int)(pcn.x >> 16), (int)(pcn.y & 0xFFFFu), (int)(pcn.y >> 16)};
    const bool born = table && dc < S.D;                                   // children come with their counts
    uint16_t fid[4];
    uint2 cc[4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
        fid[j] = S.freeIds[max(freeTop - 1 - g0 - j, 0)];
        cc[j] = born ? *reinterpret_cast<const uint2 *>(S.tab + oct_tab_off(dc + 1, S.nIni) + 4 * (pc0 + j)) : make_uint2(0u, 0u);
    }
    bool deep = false;
    int made = 0;
    uint32_t kids[2] = {0xFFFFFFFFu, 0xFFFFFFFFu};
#pragma unroll
    for (int q = 0; q < 4; q++) {
        const int c = cnt[q];
        if (c != 0) {
            const uint16_t cid = made == 0 ? fid[0] : made == 1 ? fid[1] : made == 2 ? fid[2] : fid[3];
            const uint32_t cx0 = (uint32_t)xs[q & 1], cx1 = (uint32_t)xs[(q & 1) + 1], cy0 = (uint32_t)ys[q >> 1], cy1 = (uint32_t)ys[(q >> 1) + 1];
            uint4 *ch = reinterpret_cast<uint4 *>(&S.nodes[cid]);
            ch[0] = make_uint4(cx0 | (cy0 << 16), cx1 | (cy1 << 16), (uint32_t)(pc0 + q) | ((uint32_t)dc << 16), (uint32_t)c | (c == 1 ? 0x10000u : 0u));
            ch[1] = make_uint4(c > 1 ? cc[q].x : 0u, c > 1 ? cc[q].y : 0u, 0xFFFFFFFFu, 0xFFFFFFFFu);
            deep |= table && c > 1 && dc >= S.D;
            newList[K - 1 - g0 - made] = cid;
            if (c > 1) S.open[o0++] = OctEntry{((uint32_t)c << 16) | cx0, cid, 0};
            kids[q >> 1] = (kids[q >> 1] & ~(0xFFFFu << (16 * (q & 1)))) | ((uint32_t)cid << (16 * (q & 1)));
            made++;
        }
    }
    *reinterpret_cast<uint2 *>(&p.child[0]) = make_uint2(kids[0], kids[1]);
    if constexpr (!SOLO) {
        p.split = 1;
        S.splitIds[atomicAdd(sNSplit, 1)] = (uint16_t)id;
    }
    return deep;
}

__device__ __forceinline__ int quadrants_nonempty(const OctNode &nd) { return (nd.cnt[0] != 0) + (nd.cnt[1] != 0) + (nd.cnt[2] != 0) + (nd.cnt[3] != 0); }
__device__ __forceinline__ int quadrants_open(const OctNode &nd) { return (nd.cnt[0] > 1) + (nd.cnt[1] > 1) + (nd.cnt[2] > 1) + (nd.cnt[3] > 1); }

// The std::list of the reference is kept as an ARRAY in list order (front = element 0).  A pass over the list that divides
// nodes and pushes their children to the front then becomes: children (in reverse creation order) ++ surviving old nodes (in
// their old order) — two prefix sums and a scatter.
// One LDS atomic per DISTINCT key of the wave instead of one per lane: the key-points of a level arrive in cell order, so the 64 of a wave
// fall into a handful of nodes / quadrants, and in the first rounds ALL of them hit the same two or three counters (64 serialised
// updates per instruction otherwise).
// key < 0: the lane has nothing to add; lanes with equal keys must pass the same word and the same increment.
__device__ __forceinline__ void wave_agg_add(int key, unsigned int *word, unsigned int one) {
    const int lane = threadIdx.x & 63;
    unsigned long long todo = __ballot(key >= 0);
    while (todo) {
        const int leader = __ffsll((long long)todo) - 1;
        const int k0 = __builtin_amdgcn_readlane(key, leader);
        const unsigned long long mk = __ballot(key == k0);
        if (lane == leader) atomicAdd(word, one * (unsigned int)__popcll(mk));
        todo &= ~mk;
    }
}

// (wave_run_add, the same for keys that arrive in RUNS: orb_octree.h -- k_compact counts with it too)

// inclusive prefix sum over the wave in six DPP steps (no LDS round trips: __shfl_up is a ds_bpermute each)
__device__ __forceinline__ unsigned int wave_scan_incl(unsigned int v) {
    v += (unsigned int)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xF, 0xF, false);      // row_shr:1
    v += (unsigned int)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xF, 0xF, false);      // row_shr:2
    v += (unsigned int)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xF, 0xF, false);      // row_shr:4
    v += (unsigned int)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xF, 0xF, false);      // row_shr:8
    v += (unsigned int)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xA, 0xF, false);      // row_bcast:15 -> rows 1, 3
    v += (unsigned int)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xC, 0xF, false);      // row_bcast:31 -> rows 2, 3
    return v;
}

// atomicMax(best[owner], v) for the lanes of a wave, one atomic per run of equal owners inside a row of 16 lanes (row-wide DPP shifts: the
// last lane of a run ends up with the run's maximum and is the only one that goes to LDS; 64 lanes on two or three counters serialise otherwise).
#define RUMI_RUN_MAX_STEP(S_)                                                              \
    {                                                                                      \
        const int o2 = __builtin_amdgcn_update_dpp(-2, oo, 0x110 + S_, 0xF, 0xF, false);   \
        const int v2 = __builtin_amdgcn_update_dpp(0, (int)v, 0x110 + S_, 0xF, 0xF, false); \
        if (o2 == oo) v = max(v, (uint32_t)v2);                                            \
    }
// best0 + owner * strideWords: the owner's word (the nodes' `best` fields in k_octree, a plain array by list rank in k_oct_select)
__device__ __forceinline__ void wave_run_max(uint32_t *best0, int strideWords, int owner, bool valid, uint32_t v) {
    const int oo = valid ? owner : -1;
    RUMI_RUN_MAX_STEP(1) RUMI_RUN_MAX_STEP(2) RUMI_RUN_MAX_STEP(4) RUMI_RUN_MAX_STEP(8)
    const int after = __builtin_amdgcn_update_dpp(-2, oo, 0x101, 0xF, 0xF, false);          // row_shl:1 = the next lane's owner
    if (valid && after != oo) atomicMax(best0 + owner * strideWords, v);
}
__device__ __forceinline__ void wave_run_max(OctNode *nodes, int owner, bool valid, uint32_t v) {
    wave_run_max(&nodes[0].best, (int)(sizeof(OctNode) / sizeof(uint32_t)), owner, valid, v);
}
#undef RUMI_RUN_MAX_STEP

constexpr int kKeysPerLane = 24;   // levels with at most kKeysPerLane * kOctThreads (12288) keys keep keys and owners in registers

// The keys of one level, walked by the whole workgroup with a UNIFORM trip count (wave_agg_add ballots inside the visitor).
// REG: every lane holds keys i = k * NT + tid and their owners in registers — the level is read from HBM/L2 once, with all loads
// in flight together, and the passes of the rounds below cost LDS + VALU only (a pass over keys in memory paid one dependent L2
// round trip per 512 keys: 6-10 us per pass at level 0 of a 640 x 480 frame, seven passes).  !REG: keys stay in memory, owners in owner[].
template <bool REG, int NT>
struct OctKeys {
    uint32_t ck[REG ? kKeysPerLane : 1];
    uint32_t ow[REG ? kKeysPerLane : 1];
    const uint32_t *c;
    uint16_t *own;
    int n;
    __device__ __forceinline__ void load() {
        if constexpr (REG) {
#pragma unroll
            for (int k = 0; k < kKeysPerLane; k++) {
                const int i = k * NT + (int)threadIdx.x;
                ck[k] = i < n ? c[i] : 0u;
                ow[k] = 0;
            }
        }
    }
    // f(i, valid, key, owner&): owner may be rewritten.  OWN (keys in memory only): 0 = owners are read and written back when they change,
    // 1 = no owner traffic at all (the visitor gets 0 and what it leaves is dropped), 2 = written, not read.
    template <int OWN = 0, class F>
    __device__ __forceinline__ void for_each(F f) {
        if constexpr (REG) {
#pragma unroll
            for (int k = 0; k < kKeysPerLane; k++) {
                if (k * NT >= n) break;
                const int i = k * NT + (int)threadIdx.x;
                int o = (int)ow[k];
                f(i, i < n, ck[k], o);
                ow[k] = (uint32_t)o;
            }
        } else {
            for (int i0 = 0; i0 < n; i0 += 4 * NT) {            // four trips' loads in flight together
                uint32_t k4[4];
                int o4[4];
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    const int i = i0 + u * NT + (int)threadIdx.x;
                    k4[u] = i < n ? c[i] : 0u;
                    o4[u] = OWN == 0 && i < n ? (int)own[i] : 0;
                }
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    if (i0 + u * NT >= n) break;
                    const int i = i0 + u * NT + (int)threadIdx.x;
                    int o = o4[u];
                    f(i, i < n, k4[u], o);
                    if (OWN != 1 && i < n && (OWN == 2 || o != o4[u])) own[i] = (uint16_t)o;
                }
            }
        }
    }
};

// Where the tree of one (frame, level) gets its keys' cells from.  kKeysMem / kKeysReg: two passes over the keys (in memory / in registers), the
// kernel selects the best key of every node itself.  kKeysHist (k_octree_narrow): the keys are never touched -- T_D arrives counted (k_compact's
// histogram, cleared as it is read) and the result is the list length and the cell -> list rank table k_oct_select picks the keys by; a tree
// that outgrows the count tables is handed to k_octree_redo.
enum { kKeysMem = 0, kKeysReg = 1, kKeysHist = 2 };

template <int MODE, int NT>
__device__ __forceinline__ void octree_level(const DevParams *__restrict__ P, const uint32_t *__restrict__ cand,
                                             const int32_t *__restrict__ levelStart, uint16_t *__restrict__ owner,
                                             uint32_t *__restrict__ selLevel, int32_t *__restrict__ selLevelCnt,
                                             int selLevelCap, int32_t *__restrict__ errFlag, unsigned char *lds, int level, int frame,
                                             const OctNarrow &Q) {
    constexpr bool REG = MODE == kKeysReg, HIST = MODE == kKeysHist;
    __shared__ int sPhase, sM, sNOpen, sNFree, sNSplit, sOverflow, sDeep, sSolo;
    __shared__ unsigned long long sWave[NT / 64];
    __shared__ int sSortCount[2];

    const int tid = threadIdx.x;
    const DevLevel &L = P->lv[level];
    const int32_t *ls = levelStart + (long long)frame * (kMaxLevels + 1);
    // kKeysHist: this tree is k_octree_redo's (its list entry is the only thing written)
    [[maybe_unused]] auto redo = [&]() {
        if (tid == 0) {
            Q.m[frame * P->nlevels + level] = kOctRedo;
            Q.redoList[atomicAdd(&Q.ctl[0], 1)] = frame * kMaxLevels + level;
        }
    };
    OctKeys<REG, NT> keys;
    keys.n = ls[level + 1] - ls[level];
    keys.c = cand + (long long)frame * P->totalCand + ls[level];
    keys.own = owner + (long long)frame * P->totalCand + ls[level];
    const int n = keys.n;
    const uint32_t *c = keys.c;
    uint32_t *out = selLevel + ((long long)frame * P->nlevels + level) * selLevelCap;
    int32_t *outCnt = selLevelCnt + (long long)frame * P->nlevels + level;
    if (n <= 0) {
        if (tid == 0) {
            *outCnt = 0;
            if constexpr (HIST) Q.m[frame * P->nlevels + level] = 0;
        }
        return;
    }
    const int N = L.nfeat;
    const int W = L.maxBX - kBorder, Hh = L.maxBY - kBorder;
    const int nIni = uni(oct_roots(W, Hh));        // (float arithmetic is per-lane: everything derived from it would be too)
    if (nIni <= 0 || nIni > kMaxRoots) {           // the reference divides by zero / we do not stage that many roots
        if constexpr (HIST) { redo(); return; }    // (such a level has no histogram: nothing to clear)
        if (tid == 0) { *outCnt = 0; atomicOr(errFlag, 1); }
        return;
    }
#ifdef RUMI_OCT_STAMP
    long long stAcc[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, stLast = clock64(); int stRounds[2] = {0, 0};
#define OCT_STAMP(k) do { if (tid == 0) { const long long t_ = clock64(); stAcc[k] += t_ - stLast; stLast = t_; } } while (0)
#else
#define OCT_STAMP(k) do { } while (0)
#endif
    keys.load();
    const float hX = __int_as_float(uni(__float_as_int(oct_root_width(W, nIni))));
    const int cap = octree_pool_cap(N, nIni);

    OctLds S;
    S.nodes = reinterpret_cast<OctNode *>(lds);
    S.open = reinterpret_cast<OctEntry *>(S.nodes + cap);
    S.prev = S.open + cap;
    S.freeIds = reinterpret_cast<uint16_t *>(S.prev + cap);
    S.splitIds = S.freeIds + cap;
    S.listA = S.splitIds + cap;
    S.listB = S.listA + cap;
    S.segA = reinterpret_cast<SortSeg *>(lds + (((size_t)cap * (sizeof(OctNode) + 2 * sizeof(OctEntry) + 4 * sizeof(uint16_t)) + 7) & ~(size_t)7));
    S.segB = S.segA + (cap / 16 + 2);
    S.D = oct_tab_depth(nIni, N); S.nIni = nIni;
    S.tab = reinterpret_cast<uint16_t *>((reinterpret_cast<uintptr_t>(S.segB + (cap / 16 + 2)) + 7) & ~(uintptr_t)7);
    S.leaf = S.tab + oct_tab_entries(nIni, S.D);
    S.xbin = S.leaf + oct_leaf_entries(nIni, S.D);
    S.ybin = S.xbin + W + 1;
    OctNode *nodes = S.nodes;
    uint16_t *A = S.listA, *B = S.listB;
    const int D = S.D, offD = oct_tab_off(D, nIni);

    // free stack: ids cap-1 .. nIni (top of the stack = smallest id); roots take ids 0 .. nIni-1
    for (int i = tid; i < cap - nIni; i += NT) S.freeIds[i] = (uint16_t)(cap - 1 - i);
    if (tid == 0) { sNFree = cap - nIni; sNSplit = 0; sOverflow = 0; sPhase = 0; sNOpen = 0; sDeep = 0; }
    if constexpr (HIST) {
        // T_D as k_compact counted it; what is read is cleared, so the next call's k_compact finds zeros without a memset launch
        uint32_t *hg = Q.hist + (size_t)frame * (size_t)(P->octCellStride / 2) + L.octCell / 2;
        for (int i = tid; i < (nIni << (2 * D)) / 2; i += NT) {
            const uint32_t w = hg[i];
            reinterpret_cast<uint32_t *>(S.tab + offD)[i] = w;
            if (w) hg[i] = 0u;
        }
    } else {
        for (int i = tid; i < (nIni << (2 * D)) / 2; i += NT) reinterpret_cast<uint32_t *>(S.tab + offD)[i] = 0u;
        for (int i = tid; i <= W + Hh + 1; i += NT) {  // per-coordinate halves of the path, this workgroup's own copy of the tables of set_geometry
            const bool isX = i <= W;
            const int v = isX ? i : i - (W + 1);
            const uint16_t b = oct_coord_bin(isX, v, hX, Hh, nIni, D);
            if (isX) S.xbin[v] = b;
            else S.ybin[v] = b;
        }
    }
    __syncthreads();
    OCT_STAMP(7);
    // :564-567  keys -> roots, and with the same comparisons DivideNode would make (:471-511) on down to depth D: the key's cell there.
    // The x comparisons of a path depend on x alone (the root is a function of x) and the y comparisons on y alone, so the two halves of
    // the path come from two small tables by coordinate.  A key keeps the path of its cell (its "owner" until the tree outgrows the
    // tables); T_D counts the keys of every cell.
    [[maybe_unused]] auto cell_of = [&](uint32_t ck) { return (int)S.xbin[min(cand_x(ck), W)] | (int)S.ybin[min(cand_y(ck), Hh)]; };
    if constexpr (!HIST) {
        keys.template for_each<1>([&](int, bool valid, uint32_t ck, int &o) {      // (keys in memory: the cell is looked up again when it is needed)
            int P = -1;
            if (valid) {
                P = cell_of(ck);
                o = P;
            }
            wave_run_add(P, reinterpret_cast<unsigned int *>(S.tab + offD) + ((P < 0 ? 0 : P) >> 1), 1u << (16 * (P & 1)));
        });
        __syncthreads();
    }
    OCT_STAMP(8);
    for (int d = D - 1; d >= 0; d--) {             // sum pyramid
        const uint16_t *src = S.tab + oct_tab_off(d + 1, nIni);
        uint16_t *dst = S.tab + oct_tab_off(d, nIni);
        for (int e = tid; e < (nIni << (2 * d)); e += NT) {
            const uint2 c4 = *reinterpret_cast<const uint2 *>(src + 4 * e);
            dst[e] = (uint16_t)((c4.x & 0xFFFFu) + (c4.x >> 16) + (c4.y & 0xFFFFu) + (c4.y >> 16));
        }
        __syncthreads();
    }
    if (tid < nIni) {                              // :548-561  roots in push_back order
        OctNode &r = nodes[tid];
        r.x0 = (uint16_t)(int)(hX * (float)tid); r.x1 = (uint16_t)(int)(hX * (float)(tid + 1));
        r.y0 = 0; r.y1 = (uint16_t)Hh;
        node_depth(r) = 0; node_path(r) = (uint16_t)tid;
        r.n = S.tab[tid]; r.noMore = r.n == 1; r.split = 0;
        *reinterpret_cast<uint2 *>(&r.cnt[0]) = *reinterpret_cast<const uint2 *>(S.tab + oct_tab_off(1, nIni) + 4 * tid);
        r.child[0] = r.child[1] = r.child[2] = r.child[3] = kNil;
    }
    __syncthreads();
    if (tid == 0) {                                // :570-578: empty roots leave the list (their ids are simply not reused)
        int m = 0;
        for (int i = 0; i < nIni; i++)
            if (nodes[i].n != 0) A[m++] = (uint16_t)i;
        sM = m;
    }
    __syncthreads();
    bool table = true;                             // uniform: the count tables still cover every open node
    // leaf[cell of depth D] = the node of `list` that covers it; the cells of a node are consecutive paths.  One thread per node writes up
    // to 16 cells itself; the few shallower nodes (64, 256 cells: sparse levels) are filled by their wave, lane per cell.
    // kKeysHist: the table holds the node's RANK in the list instead (k_oct_select has no node pool).
    auto fill_leaf = [&](const uint16_t *list, int len) {
        for (int r0 = 0; r0 < len; r0 += NT) {
            const int r = r0 + tid;
            int id = 0, span = 0, base = 0;
            if (r < len) {
                id = list[r];
                OctNode &nd = nodes[id];
                span = 1 << (2 * (D - (int)node_depth(nd)));
                base = (int)node_path(nd) * span;
                if constexpr (HIST) id = r;
                if (span <= 16)
                    for (int cI = 0; cI < span; cI++) S.leaf[base + cI] = (uint16_t)id;
            }
            unsigned long long big = __ballot(span > 16);
            while (big) {
                const int src = __ffsll((long long)big) - 1;
                big &= big - 1;
                const int bId = __builtin_amdgcn_readlane(id, src), bSpan = __builtin_amdgcn_readlane(span, src), bBase = __builtin_amdgcn_readlane(base, src);
                for (int cI = tid & 63; cI < bSpan; cI += 64) S.leaf[bBase + cI] = (uint16_t)bId;
            }
        }
    };
    OCT_STAMP(0);
    // while (!bFinish)  :587-702
    while (true) {
        const int m = uni(sM), phase = uni(sPhase), nFree = uni(sNFree);
#ifdef RUMI_OCT_STAMP
        stRounds[phase != 0]++;
#endif
        bool freed = false;
        if (table && phase == 0 && m <= 64) {
            // ---- the first coarse passes, while the list fits one wave and children are born with their counts: wave 0 runs them back to
            // back (divide, push to the front, free the parents) on wave-level scans, without a workgroup barrier; the others wait below
            if (tid < 64) {
                int mm = m, nf = nFree, ph = 0, rounds = 0, E = 0;
                bool anyDeep = false;
                uint16_t *La = A, *Lb = B;
                while (true) {
                    const bool has = tid < mm;
                    int id = 0;
                    unsigned int loc = 0;                                   // children | kept << 10 | open children << 20
                    bool div = false;
                    if (has) {
                        id = La[tid];
                        const OctNode &nd = nodes[id];
                        div = !nd.noMore;
                        loc = div ? (unsigned int)quadrants_nonempty(nd) | ((unsigned int)quadrants_open(nd) << 20) : 1u << 10;
                    }
                    const unsigned int inc = wave_scan_incl(loc);
                    const unsigned int tot = (unsigned int)__builtin_amdgcn_readlane((int)inc, 63);
                    const int K = (int)(tot & 0x3FF), kept = (int)((tot >> 10) & 0x3FF);
                    if (K > nf) {                                           // cannot happen with cap >= 2N+16 (reported, not hidden)
                        if (tid == 0) sOverflow = 1;
                        ph = 2;
                        break;
                    }
                    E = (int)(tot >> 20);
                    const unsigned int base = inc - loc;
                    bool deep = false;
                    if (has) {
                        if (div) deep = emit_children<true>(S, id, (int)(base & 0x3FF), (int)(base >> 20), K, nf, Lb, nullptr, true);
                        else Lb[K + (int)((base >> 10) & 0x3FF)] = (uint16_t)id;
                    }
                    // divided nodes return to the free stack (the slots their children came from: every read of those is already issued)
                    const unsigned long long dv = __ballot(div);
                    nf -= K;
                    if (div) S.freeIds[nf + __popcll(dv & ((1ull << tid) - 1ull))] = (uint16_t)id;
                    nf += __popcll(dv);
                    if (__ballot(deep)) anyDeep = true;
                    wave_fence_lds();
                    const int size = K + kept;
                    ph = (size >= N || size == mm) ? 2 : (size + E * 3 > N ? 1 : 0);
                    { uint16_t *t = La; La = Lb; Lb = t; }
                    rounds++;
                    mm = size;
                    if (ph != 0 || mm > 64 || anyDeep) break;
                }
                if (tid == 0 && anyDeep) sDeep = 1;
                if (tid == 0) { sM = mm; sNFree = nf; sNOpen = E; sPhase = ph; sSolo = rounds; }
            }
            __syncthreads();
            if (uni(sSolo) & 1) { uint16_t *t = A; A = B; B = t; }
            freed = true;
        } else {
        if (phase == 0) {
            // ---- coarse pass: every node that can be divided is divided (:590-640)
            const int chunk = (m + NT - 1) / NT, p0 = min(m, tid * chunk), p1 = min(m, p0 + chunk);
            unsigned long long loc = 0;                                     // children | kept << 20 | open children << 40
            for (int p = p0; p < p1; p++) {
                const OctNode &nd = nodes[A[p]];
                if (!nd.noMore) loc += (unsigned long long)quadrants_nonempty(nd) | ((unsigned long long)quadrants_open(nd) << 40);
                else loc += 1ull << 20;
            }
            unsigned long long tot;
            const unsigned long long base = block_scan64<NT>(loc, sWave, &tot);
            const int K = (int)(tot & 0xFFFFF), kept = (int)((tot >> 20) & 0xFFFFF), E = (int)(tot >> 40);
            if (K > nFree) {                                                 // cannot happen with cap >= 2N+16 (reported, not hidden)
                if (tid == 0) { sOverflow = 1; sPhase = 2; }
            } else {
                int g = (int)(base & 0xFFFFF), kb = (int)((base >> 20) & 0xFFFFF), o = (int)(base >> 40);
                for (int p = p0; p < p1; p++) {
                    const int id = A[p];
                    const OctNode &nd = nodes[id];
                    if (!nd.noMore) {
                        const int kc = quadrants_nonempty(nd), ko = quadrants_open(nd);
                        if (emit_children<false>(S, id, g, o, K, nFree, B, &sNSplit, table)) sDeep = 1;
                        g += kc; o += ko;
                    } else {
                        B[K + kb++] = (uint16_t)id;
                    }
                }
                if (tid == 0) {
                    const int size = K + kept;
                    sM = size; sNFree = nFree - K; sNOpen = E;
                    if (size >= N || size == m) sPhase = 2;
                    else if (size + E * 3 > N) sPhase = 1;
                }
            }
        } else {
            // ---- fine round: largest nodes first, stop as soon as there are N nodes (:646-699)
            const int nPrev = uni(sNOpen);
            if (nPrev <= 64) {                      // one wave, entries in registers
                if (tid < 64) {
                    OctEntry e = OctEntry{0u, 0, 0};
                    if (tid < nPrev) e = S.open[tid];
                    wave_fence_lds();
                    wave_sort_like_libstdcxx(e.key, e.id, nPrev, S.prev, S.open);
                }
                __syncthreads();
            } else {
                for (int i = tid; i < nPrev; i += NT) S.prev[i] = S.open[i];
                __syncthreads();
                wg_sort_like_libstdcxx(S.prev, nPrev, S.open, B, S.splitIds, S.segA, S.segB, sSortCount);   // open/B/splitIds are idle here
            }
            OCT_STAMP(2);
            // processing order t = 0.. is the sorted array walked from the back
            const int chunk = (nPrev + NT - 1) / NT, t0 = min(nPrev, tid * chunk), t1 = min(nPrev, t0 + chunk);
            unsigned long long loc = 0;                                     // children | open children << 40
            for (int t = t0; t < t1; t++) {
                const OctNode &nd = nodes[S.prev[nPrev - 1 - t].id];
                loc += (unsigned long long)quadrants_nonempty(nd) | ((unsigned long long)quadrants_open(nd) << 40);
            }
            unsigned long long tot;
            const unsigned long long base = block_scan64<NT>(loc, sWave, &tot);
            // node t is divided iff the list was still short of N before it: m + sum_{u<t}(children_u - 1) < N
            unsigned long long mine = 0;                                    // children | divided << 20 | open << 40, over MY divided nodes
            {
                int g = (int)(base & 0xFFFFF);
                for (int t = t0; t < t1; t++) {
                    const OctNode &nd = nodes[S.prev[nPrev - 1 - t].id];
                    const int kc = quadrants_nonempty(nd);
                    if (t == 0 || m + g - t < N) mine += (unsigned long long)kc | (1ull << 20) | ((unsigned long long)quadrants_open(nd) << 40);
                    g += kc;
                }
            }
            unsigned long long tot2;
            (void)block_scan64<NT>(mine, sWave, &tot2);
            const int K = (int)(tot2 & 0xFFFFF), J = (int)((tot2 >> 20) & 0xFFFFF), E = (int)(tot2 >> 40);
            if (K > nFree) {
                if (tid == 0) { sOverflow = 1; sPhase = 2; }
            } else {
                int g = (int)(base & 0xFFFFF), o = (int)(base >> 40);
                for (int t = t0; t < t1; t++) {
                    const int id = S.prev[nPrev - 1 - t].id;
                    const OctNode &nd = nodes[id];
                    const int kc = quadrants_nonempty(nd), ko = quadrants_open(nd);
                    if (t < J) if (emit_children<false>(S, id, g, o, K, nFree, B, &sNSplit, table)) sDeep = 1;
                    g += kc; o += ko;
                }
                __syncthreads();
                // the rest of the list keeps its order behind the new children
                const int chunkL = (m + NT - 1) / NT, p0 = min(m, tid * chunkL), p1 = min(m, p0 + chunkL);
                unsigned long long keep = 0;
                for (int p = p0; p < p1; p++) keep += nodes[A[p]].split ? 0 : 1;
                unsigned long long totK;
                int kb = (int)block_scan64<NT>(keep, sWave, &totK);
                for (int p = p0; p < p1; p++) {
                    const int id = A[p];
                    if (!nodes[id].split) B[K + kb++] = (uint16_t)id;
                }
                if (tid == 0) {
                    const int size = K + (int)totK;
                    sM = size; sNFree = nFree - K; sNOpen = E;
                    if (size >= N || size == m) sPhase = 2;
                }
            }
        }
        __syncthreads();
        { uint16_t *t = A; A = B; B = t; }
        }
        OCT_STAMP(phase == 0 ? 1 : 3);
        if (uni(sPhase) == 2) break;                // the last relabelling is folded into the selection pass below
        const int m2 = uni(sM);
        if (table) {
            // Nothing to do while the children were born with their counts.  Once a cell of depth D has been opened the tables end:
            // every key moves from its cell to the node that covers the cell now, the keys of those deepest nodes are counted, and the
            // rounds after this one relabel and count as they go (below).
            if (uni(sDeep)) {
                if constexpr (HIST) { redo(); return; }     // the tree outgrows the count tables: the rest needs the keys
                fill_leaf(A, m2);
                __syncthreads();
                keys.template for_each<2>([&](int, bool valid, uint32_t ck, int &o) {
                    int key = -1, q = 0, id = 0;
                    if (valid) {
                        id = S.leaf[REG ? o : cell_of(ck)];
                        o = id;
                        OctNode &nd = nodes[id];
                        if (!nd.noMore && node_depth(nd) == D) { q = oct_quadrant(nd, cand_x(ck), cand_y(ck)); key = id * 4 + q; }
                    }
                    wave_agg_add(key, reinterpret_cast<unsigned int *>(&nodes[id].cnt[q & 2]), 1u << (16 * (q & 1)));
                });
                table = false;
            }
        } else {
            // relabel keys of divided nodes, count inside the new owners (one LDS atomic per distinct (node, quadrant) of the wave)
            keys.for_each([&](int, bool valid, uint32_t ck, int &o) {
                int key = -1, q = 0, id = 0;
                if (valid && nodes[o].split) {
                    const int x = cand_x(ck), y = cand_y(ck);
                    id = nodes[o].child[oct_quadrant(nodes[o], x, y)];
                    o = id;
                    const OctNode &nd = nodes[id];
                    if (!nd.noMore) { q = oct_quadrant(nd, x, y); key = id * 4 + q; }
                }
                wave_agg_add(key, reinterpret_cast<unsigned int *>(&nodes[id].cnt[q & 2]), 1u << (16 * (q & 1)));
            });
        }
        __syncthreads();
        OCT_STAMP(4);
        if (!freed) {                               // divided nodes return to the free stack
            const int ns = uni(sNSplit), nf = uni(sNFree);
            for (int i = tid; i < ns; i += NT) { const int id = S.splitIds[i]; nodes[id].split = 0; S.freeIds[nf + i] = (uint16_t)id; }
            __syncthreads();
            if (tid == 0) { sNFree = nf + ns; sNSplit = 0; }
        }
        __syncthreads();
        OCT_STAMP(5);
    }
    // :705-721  best key of every node, nodes in list order; the keys of the nodes divided in the last round move to their
    // children on the way (best shares its word with the quadrant counts of the surviving nodes, hence the clearing first)
    const int m = uni(sM);
    if constexpr (HIST) {
        // the errors of the old kernel are the old kernel's to report; otherwise: the list length and, by cell, the rank of the node that covers it
        if (uni(sOverflow) || m > selLevelCap) { redo(); return; }
        fill_leaf(A, m);                           // (the count tables covered every round: every node is at most D deep)
        __syncthreads();
        uint32_t *rg = Q.rank + (size_t)frame * (size_t)(P->octCellStride / 2) + L.octCell / 2;
        for (int i = tid; i < (nIni << (2 * D)) / 2; i += NT) rg[i] = reinterpret_cast<const uint32_t *>(S.leaf)[i];
        if (tid == 0) Q.m[frame * P->nlevels + level] = m;
        return;
    }
    if (tid == 0 && sOverflow) atomicOr(errFlag, 2);
    if (table) fill_leaf(A, m);                    // every node of the final list is at most D deep here
    for (int r = tid; r < m; r += NT) nodes[A[r]].best = 0;
    __syncthreads();
    OCT_STAMP(9);
    if (table) {
        keys.template for_each<1>([&](int i, bool valid, uint32_t ck, int &o) {
            wave_run_max(nodes, valid ? (int)S.leaf[REG ? o : cell_of(ck)] : 0, valid, ((uint32_t)cand_score(ck) << 16) | (uint32_t)(0xFFFF - i));
        });
    } else {
        keys.for_each([&](int i, bool valid, uint32_t ck, int &o) {
            if (valid && nodes[o].split) o = nodes[o].child[oct_quadrant(nodes[o], cand_x(ck), cand_y(ck))];
            wave_run_max(nodes, o, valid, ((uint32_t)cand_score(ck) << 16) | (uint32_t)(0xFFFF - i));
        });
    }
    __syncthreads();
    OCT_STAMP(10);
    if (m > selLevelCap) {
        if (tid == 0) { *outCnt = 0; atomicOr(errFlag, 4); }
        return;
    }
    for (int r = tid; r < m; r += NT) out[r] = c[0xFFFF - (int)(nodes[A[r]].best & 0xFFFF)];
    if (tid == 0) *outCnt = m;
    OCT_STAMP(6);
#ifdef RUMI_OCT_STAMP
    if (tid == 0 && frame == 0) printf("oct L%d n=%d N=%d m=%d D=%d %s rounds %d+%d  setup %lld coarse %lld sort %lld fine %lld relabel %lld free %lld select %lld | init %lld pass1 %lld leaf %lld pass2 %lld\n", level, n, N, m, D, table ? "tables" : "relabel", stRounds[0], stRounds[1], stAcc[0], stAcc[1], stAcc[2], stAcc[3], stAcc[4], stAcc[5], stAcc[6], stAcc[7], stAcc[8], stAcc[9], stAcc[10]);
#endif
}

// REGS: levels of up to kKeysPerLane * kOctThreads keys run with their keys in registers (one workgroup per CU, the latency of one
// (frame, level) is what counts -- small batches); !REGS: 120 VGPRs, two workgroups per CU hide each other's LDS and L2 round trips (large
// batches; at 64 VGPRs the loads-first emit_children spills and the launch is 20-60 % slower).  launch_octree picks by the number of workgroups.
// Large batches: NT = 256 up to ~1200 features per frame (four workgroups per CU overlap their serial phases), 512 beyond (the passes over
// the keys weigh more).
template <bool REGS, int NT>
__global__ __launch_bounds__(NT, REGS ? 1 : 4) void k_octree(const DevParams *__restrict__ P, const uint32_t *__restrict__ cand,
                                                        const int32_t *__restrict__ levelStart, uint16_t *__restrict__ owner,
                                                        uint32_t *__restrict__ selLevel, int32_t *__restrict__ selLevelCnt,
                                                        int selLevelCap, int32_t *__restrict__ errFlag) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    const OctNarrow none{};
    if constexpr (REGS) {
        const int32_t *ls = levelStart + (long long)blockIdx.y * (kMaxLevels + 1);
        if (ls[blockIdx.x + 1] - ls[blockIdx.x] <= kKeysPerLane * NT) {
            octree_level<kKeysReg, NT>(P, cand, levelStart, owner, selLevel, selLevelCnt, selLevelCap, errFlag, lds, blockIdx.x, blockIdx.y, none);
            return;
        }
    }
    octree_level<kKeysMem, NT>(P, cand, levelStart, owner, selLevel, selLevelCnt, selLevelCap, errFlag, lds, blockIdx.x, blockIdx.y, none);
}

// ---- the batch pipeline: k_compact's histogram -> k_octree_narrow -> k_octree_redo -> k_oct_select ------------------------------------
// A k_octree<false, 256> workgroup wants a 128-register slot on all four SIMDs of a CU at once plus 29 KB of LDS, and beside the other slot
// streams' kernels (small waves that fill the SIMDs) it waits for that: 330 us in the overlapped step against 80 us alone.  Most of the
// footprint idles -- the list phases run on wave 0 while three waves sit at barriers.  So a tree gets ONE wave (NT = 64: every barrier of
// the rounds is gone) and the two data-parallel passes over the keys move into wide, light kernels: the count of every depth-D cell into
// k_compact (it has each key in a register anyway), the choice of the best key of every node into k_oct_select.
template <int NT>
__global__ __launch_bounds__(NT, 4) void k_octree_narrow(const DevParams *__restrict__ P, const int32_t *__restrict__ levelStart,
                                                         int32_t *__restrict__ selLevelCnt, int selLevelCap, OctNarrow Q) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    octree_level<kKeysHist, NT>(P, nullptr, levelStart, nullptr, nullptr, selLevelCnt, selLevelCap, nullptr, lds, blockIdx.x, blockIdx.y, Q);
}

// The trees k_octree_narrow handed on (the count tables ended before the tree did, or one of the reported errors), by the keys-in-memory
// kernel as it is: it counts from the keys again, so its results are k_octree<false, NT>'s by construction.  A fixed grid strides over the
// list and is gone at once when the list is empty; the last workgroup to finish adds the launch to the handle's statistic and clears the
// list's counter for the slot range's next launch.  No workgroup waits for another.
// (32 workgroups: each of them, empty list or not, waits for the 128-register, 29 KB slot the pipeline exists to avoid -- 256 of them
// took 45 us beside the other streams' kernels with nothing to do)
constexpr int kRedoGrid = 32;
template <int NT>
__global__ __launch_bounds__(NT, 4) void k_octree_redo(const DevParams *__restrict__ P, const uint32_t *__restrict__ cand,
                                                       const int32_t *__restrict__ levelStart, uint16_t *__restrict__ owner,
                                                       uint32_t *__restrict__ selLevel, int32_t *__restrict__ selLevelCnt,
                                                       int selLevelCap, int32_t *__restrict__ errFlag, OctNarrow Q, int ntrees) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    __shared__ int sCnt;
    if (threadIdx.x == 0) sCnt = Q.ctl[0];
    __syncthreads();
    const int cnt = uni(sCnt);
    for (int t = blockIdx.x; t < cnt; t += gridDim.x) {
        const int e = uni(Q.redoList[t]);
        octree_level<kKeysMem, NT>(P, cand, levelStart, owner, selLevel, selLevelCnt, selLevelCap, errFlag, lds, e % kMaxLevels, e / kMaxLevels, Q);
        __syncthreads();                            // (the next tree's set-up overwrites what this one's last pass reads)
    }
    if (threadIdx.x == 0 && atomicAdd(&Q.ctl[1], 1) == (int)gridDim.x - 1) {   // every workgroup has read the counter before its ticket
        atomicAdd(&Q.stat[0], ntrees - cnt);
        atomicAdd(&Q.stat[1], cnt);
        Q.ctl[0] = 0; Q.ctl[1] = 0;
    }
}

// The best key of every node of the final list (:705-721: largest response, first in candidate order on ties) for the trees
// k_octree_narrow finished: a key's node is rank[cell of the key], its cell comes from the host-built coordinate tables.
constexpr int kSelectThreads = 256;
__global__ __launch_bounds__(kSelectThreads) void k_oct_select(const DevParams *__restrict__ P, const uint32_t *__restrict__ cand,
                                                               const int32_t *__restrict__ levelStart, uint32_t *__restrict__ selLevel,
                                                               int32_t *__restrict__ selLevelCnt, int selLevelCap, OctNarrow Q) {
    extern __shared__ __attribute__((aligned(16))) uint32_t sel[];     // cell -> rank (16 bit each) | best [m]
    const int tid = threadIdx.x, level = blockIdx.x, frame = blockIdx.y;
    const int m = uni(Q.m[frame * P->nlevels + level]);
    if (m <= 0) return;                            // no keys (the count is written), or the tree is k_octree_redo's (kOctRedo)
    const DevLevel &L = P->lv[level];
    const int32_t *ls = levelStart + (long long)frame * (kMaxLevels + 1);
    const int n = ls[level + 1] - ls[level];
    const uint32_t *c = cand + (long long)frame * P->totalCand + ls[level];
    const int W = L.maxBX - kBorder, Hh = L.maxBY - kBorder;
    const uint16_t *xbin = Q.bins + L.octBin, *ybin = xbin + W + 1;
    const uint16_t *rank = reinterpret_cast<const uint16_t *>(sel);
    uint32_t *best = sel + L.octCells / 2;
    const uint32_t *rg = Q.rank + (size_t)frame * (size_t)(P->octCellStride / 2) + L.octCell / 2;
    for (int i = tid; i < L.octCells / 2; i += kSelectThreads) sel[i] = rg[i];
    for (int r = tid; r < m; r += kSelectThreads) best[r] = 0u;
    __syncthreads();
    for (int i0 = 0; i0 < n; i0 += kSelectThreads) {
        const int i = i0 + tid;
        const bool valid = i < n;
        const uint32_t ck = valid ? c[i] : 0u;
        const int r = valid ? (int)rank[(int)xbin[min(cand_x(ck), W)] | (int)ybin[min(cand_y(ck), Hh)]] : 0;
        wave_run_max(best, 1, r, valid, ((uint32_t)cand_score(ck) << 16) | (uint32_t)(0xFFFF - i));
    }
    __syncthreads();
    uint32_t *out = selLevel + ((long long)frame * P->nlevels + level) * selLevelCap;
    for (int r = tid; r < m; r += kSelectThreads) out[r] = c[min(0xFFFF - (int)(best[r] & 0xFFFF), n - 1)];   // (every node of the list has a key)
    if (tid == 0) selLevelCnt[(long long)frame * P->nlevels + level] = m;
}

// 0: the keys-in-registers kernel (at most one workgroup per CU); 1: the keys-in-memory kernel in one launch; 2: the batch pipeline.
// RUMI_OCT_REGS and RUMI_OCT_NARROW are read once per process.
int octree_plan(const DevParams &hP, int nframes) {
    static const int forced = [] { const char *e = getenv("RUMI_OCT_REGS"); return e ? atoi(e) : -1; }();
    static const bool narrow = [] { const char *e = getenv("RUMI_OCT_NARROW"); return !e || atoi(e) != 0; }();
    const bool regs = forced >= 0 ? forced != 0 : hP.nlevels * nframes <= 256;   // at most one workgroup per CU
    if (regs) return 0;
    return narrow && hP.octCellStride > 0 ? 2 : 1;
}

// One wave per tree: 256 threads per tree were measured too (93 us against 61 us per 256-frame launch in the overlapped step)
constexpr int kNarrowThreads = 64;
void launch_octree(const DevParams *dP, const DevParams &hP, const uint32_t *cand, const int32_t *levelStart,
                   uint16_t *owner, uint32_t *selLevel, int32_t *selLevelCnt, int selLevelCap, int32_t *errFlag,
                   int nframes, const OctLdsSizes &lds, const OctNarrow &Q, hipStream_t st) {
    const int plan = octree_plan(hP, nframes);
    auto go = [&](auto kern, int threads) {
        // > 64 KiB of dynamic LDS needs the opt-in (process state that only grows: rumi_common.h)
        (void)raise_lds_limit(reinterpret_cast<const void *>(kern), lds.wide);
        hipLaunchKernelGGL(kern, dim3(hP.nlevels, nframes), dim3(threads), lds.wide, st, dP, cand, levelStart, owner, selLevel, selLevelCnt, selLevelCap,
                           errFlag);
    };
    const bool small = hP.lv[0].nfeat <= 260;                                   // level 0 of 1200 features at scale 1.2, 8 levels
    if (plan == 0) { go(k_octree<true, kOctThreads>, kOctThreads); return; }
    if (plan == 1) {
        if (small) go(k_octree<false, 256>, 256);
        else go(k_octree<false, kOctThreads>, kOctThreads);
        return;
    }
    const dim3 grid(hP.nlevels, nframes);
    (void)raise_lds_limit(reinterpret_cast<const void *>(k_octree_narrow<kNarrowThreads>), lds.narrow);
    hipLaunchKernelGGL(k_octree_narrow<kNarrowThreads>, grid, dim3(kNarrowThreads), lds.narrow, st, dP, levelStart, selLevelCnt, selLevelCap, Q);
    auto redo = [&](auto kern, int threads) {
        (void)raise_lds_limit(reinterpret_cast<const void *>(kern), lds.wide);
        hipLaunchKernelGGL(kern, dim3(kRedoGrid), dim3(threads), lds.wide, st, dP, cand, levelStart, owner, selLevel, selLevelCnt, selLevelCap, errFlag,
                           Q, hP.nlevels * nframes);
    };
    if (small) redo(k_octree_redo<256>, 256);
    else redo(k_octree_redo<kOctThreads>, kOctThreads);
    hipLaunchKernelGGL(k_oct_select, grid, dim3(kSelectThreads), lds.select, st, dP, cand, levelStart, selLevel, selLevelCnt, selLevelCap, Q);
}
OctLdsSizes octree_lds_for(const DevParams &hP, int selLevelCap) {
    OctLdsSizes s{0, 0, 0};
    for (int l = 0; l < hP.nlevels; l++) {
        const int W = hP.lv[l].maxBX - kBorder, Hh = hP.lv[l].maxBY - kBorder;
        int nIni = oct_roots(W, Hh);
        if (nIni < 1) nIni = 1;
        const int nr = nIni > kMaxRoots ? kMaxRoots : nIni;
        const int cap = octree_pool_cap(hP.lv[l].nfeat, nIni), D = oct_tab_depth(nr, hP.lv[l].nfeat);
        s.wide = std::max(s.wide, octree_lds_bytes(cap, nr, D, W, Hh));
        s.narrow = std::max(s.narrow, octree_lds_bytes(cap, nr, D, -1, -1));
        s.select = std::max(s.select, (size_t)hP.lv[l].octCells * sizeof(uint16_t) + (size_t)selLevelCap * sizeof(uint32_t));
    }
    return s;
}

}  // namespace rumi

#include "orb_assemble.inc"
