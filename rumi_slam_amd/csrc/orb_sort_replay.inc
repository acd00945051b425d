// libstdc++'s std::sort replayed on the device, by a workgroup and by one wave (the quadtree's fine rounds sort with them), and the test hook
// that runs them on an arbitrary array.
namespace rumi {

// ---- workgroup-parallel replay of libstdc++'s std::sort on (key, id) entries -------------------------------------------------
// std::sort = introsort loop (median-of-3 pivot moved to the front, Hoare "unguarded" partition, recursion on the right part,
// depth limit 2*floor(log2 n) with a heap-sort fallback) down to segments of <= 16, then one insertion sort over everything.
// The segments of one recursion level are disjoint, so they are partitioned concurrently, one WAVE per segment; inside a
// segment the Hoare partition is data-parallel: the k-th stop of the left pointer (element not < pivot) is swapped with the
// k-th stop of the right pointer (element not > pivot) while the former lies left of the latter, which only needs the ranks
// of the stop positions.  The final insertion sort is stable and never moves an element out of its <= 16-element leaf, so it
// equals a stable rank over a +-15 window.  Tie order of equal keys therefore matches libstdc++ exactly (tests compare with
// the real std::sort).
struct SortSeg { uint16_t first, last; int16_t depth; uint16_t pad; };

__device__ __forceinline__ void wave_fence_lds() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// a[0..n) sorted in place; tmp[n] entries, sf/sr[n] uint16, segA/segB[n/16+2] are scratch; every thread of the workgroup calls it
__device__ void wg_sort_like_libstdcxx(OctEntry *a, int n, OctEntry *tmp, uint16_t *sf, uint16_t *sr, SortSeg *segA, SortSeg *segB,
                                       int *sCount /* [2] in LDS */) {
    using namespace sortimpl;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), nWaves = blockDim.x >> 6;
    if (n <= 1) return;
    if (tid == 0) {
        int lg = 0;
        for (int t = n; t > 1; t >>= 1) lg++;
        sCount[0] = 0; sCount[1] = 0;
        if (n > 16) { segA[0] = SortSeg{0, (uint16_t)n, (int16_t)(lg * 2), 0}; sCount[0] = 1; }
    }
    __syncthreads();
    int cur = 0;
    while (true) {
        const int nSeg = uni(sCount[cur]);
        if (nSeg == 0) break;
        SortSeg *in = cur ? segB : segA, *outS = cur ? segA : segB;
        for (int si = wave; si < nSeg; si += nWaves) {
            const SortSeg sg = in[si];
            const int first = uni(sg.first), last = uni(sg.last);
            if (sg.depth == 0) {                                        // std::__partial_sort(first, last, last)
                if (lane == 0) heap_sort(a + first, a + last);
                continue;
            }
            if (lane == 0) move_median_to_first(a + first, a + first + 1, a + first + (last - first) / 2, a + last - 1);
            wave_fence_lds();
            const uint32_t piv = (uint32_t)uni((int)a[first].key);
            // stops of the left pointer, in ascending order: sf[first + k]
            int nF = 0, nR = 0;
            for (int base = first + 1; base < last; base += 64) {
                const int i = base + lane;
                const bool stop = i < last && !(a[i].key < piv);
                const unsigned long long b = __ballot(stop);
                if (stop) sf[first + nF + __popcll(b & ((1ull << lane) - 1ull))] = (uint16_t)i;
                nF += __popcll(b);
            }
            // stops of the right pointer, in descending order: sr[first + k]
            for (int base = last - 1; base > first; base -= 64) {
                const int i = base - lane;
                const bool stop = i > first && !(piv < a[i].key);
                const unsigned long long b = __ballot(stop);
                if (stop) sr[first + nR + __popcll(b & ((1ull << lane) - 1ull))] = (uint16_t)i;
                nR += __popcll(b);
            }
            wave_fence_lds();
            int swaps = 0;
            const int nPair = min(nF, nR);
            for (int base = 0; base < nPair; base += 64) {
                const int k = base + lane;
                bool sw = false;
                if (k < nPair) {
                    const int f = sf[first + k], r = sr[first + k];
                    if (f < r) { sw = true; const OctEntry t = a[f]; a[f] = a[r]; a[r] = t; }
                }
                swaps += __popcll(__ballot(sw));
            }
            wave_fence_lds();
            if (lane == 0) {
                int cut;
                if (swaps >= 1) {
                    const int nextF = swaps < nF ? (int)sf[first + swaps] : 0x7FFFFFFF;
                    cut = min(nextF, (int)sr[first + swaps - 1]);
                } else {
                    cut = sf[first];
                }
                const int16_t d = (int16_t)(sg.depth - 1);
                if (last - cut > 16) outS[atomicAdd(&sCount[cur ^ 1], 1)] = SortSeg{(uint16_t)cut, (uint16_t)last, d, 0};
                if (cut - first > 16) outS[atomicAdd(&sCount[cur ^ 1], 1)] = SortSeg{(uint16_t)first, (uint16_t)cut, d, 0};
            }
        }
        __syncthreads();
        if (tid == 0) sCount[cur] = 0;
        cur ^= 1;
        __syncthreads();
    }
    // __final_insertion_sort == stable sort inside each leaf == stable rank over a +-15 window
    for (int i = tid; i < n; i += blockDim.x) {
        const OctEntry e = a[i];
        int pos = i;
        for (int j = max(0, i - 15); j < i; j++) pos -= a[j].key > e.key;
        for (int j = i + 1; j < min(n, i + 16); j++) pos += a[j].key < e.key;
        tmp[pos] = e;
    }
    __syncthreads();
    for (int i = tid; i < n; i += blockDim.x) a[i] = tmp[i];
    __syncthreads();
}

// ---- the same replay for up to 64 entries, by ONE wave with the entries in registers (lane i = element i) ------------------------
// The fine rounds of a 1000-feature frame sort ~60 entries: the workgroup version spends its time in barriers and dependent LDS round
// trips (median, pivot, stop lists, swaps, segment lists: ~15 k cycles); here the stops of the two pointers are two ballots, the k-th stop
// of one pointer meets the k-th stop of the other through two ds_permute rank tables, the swap is one ds_bpermute pair, and nothing is stored in LDS.
// key / id: the lane's entry (lanes >= n: anything); sorted entries are written to out[0..n) (LDS); heapScratch: n entries of LDS
__device__ __forceinline__ void wave_sort_like_libstdcxx(uint32_t key, uint32_t id, int n, OctEntry *out, OctEntry *heapScratch) {
    using namespace sortimpl;
    const int lane = threadIdx.x & 63;
    if (n > 16) {
        int stack = 0, sp = 0;                       // a VGPR as a 64-entry array of first | last << 8 | depth << 16 (uniform)
        {
            int lg = 0;
            for (int t = n; t > 1; t >>= 1) lg++;
            if (lane == 0) stack = n << 8 | (lg * 2) << 16;
            sp = 1;
        }
        while (sp > 0) {
            const int top = __builtin_amdgcn_readlane(stack, --sp);
            int first = top & 0xFF, last = (top >> 8) & 0xFF, depth = top >> 16;
            while (last - first > 16) {
                if (depth == 0) {                    // std::__partial_sort(first, last, last): serial, through LDS (adversarial inputs only)
                    if (lane < n) heapScratch[lane] = OctEntry{key, (uint16_t)id, 0};
                    wave_fence_lds();
                    if (lane == 0) heap_sort(heapScratch + first, heapScratch + last);
                    wave_fence_lds();
                    if (lane < n) { const OctEntry e = heapScratch[lane]; key = e.key; id = e.id; }
                    wave_fence_lds();
                    break;
                }
                depth--;
                // std::__move_median_to_first(first, first + 1, mid, last - 1)
                const int ia = first + 1, ib = first + (last - first) / 2, ic = last - 1;
                const uint32_t ka = (uint32_t)__builtin_amdgcn_readlane((int)key, ia), kb = (uint32_t)__builtin_amdgcn_readlane((int)key, ib),
                               kc = (uint32_t)__builtin_amdgcn_readlane((int)key, ic);
                const int sIdx = ka < kb ? (kb < kc ? ib : (ka < kc ? ic : ia)) : (ka < kc ? ia : (kb < kc ? ic : ib));
                {
                    const uint32_t kf = (uint32_t)__builtin_amdgcn_readlane((int)key, first), idf = (uint32_t)__builtin_amdgcn_readlane((int)id, first);
                    const uint32_t ks = (uint32_t)__builtin_amdgcn_readlane((int)key, sIdx), ids = (uint32_t)__builtin_amdgcn_readlane((int)id, sIdx);
                    if (lane == first) { key = ks; id = ids; }
                    else if (lane == sIdx) { key = kf; id = idf; }
                }
                const uint32_t piv = (uint32_t)__builtin_amdgcn_readlane((int)key, first);
                // std::__unguarded_partition(first + 1, last, first): stops of the left pointer (ascending) and of the right one (descending)
                const bool inSeg = lane > first && lane < last;
                const unsigned long long MF = __ballot(inSeg && !(key < piv)), MR = __ballot(inSeg && !(piv < key));
                const int nF = __popcll(MF), nR = __popcll(MR);
                const unsigned long long below = (1ull << lane) - 1ull, above = lane == 63 ? 0ull : ~0ull << (lane + 1);
                const bool isF = (MF >> lane) & 1, isR = (MR >> lane) & 1;
                const int fBelow = __popcll(MF & below), rBelow = __popcll(MR & below);
                const int kF = fBelow, kR = __popcll(MR & above);
                // tabF[k] / tabR[k] (in lane k) = position of the k-th stop of the left / right pointer: every lane sends its index to a slot
                // of its own (stops first, by rank; the other lanes behind them), one ds_permute each
                const int tabF = __builtin_amdgcn_ds_permute((isF ? kF : nF + lane - fBelow) << 2, lane);
                const int tabR = __builtin_amdgcn_ds_permute((isR ? kR : nR + lane - rBelow) << 2, lane);
                const int rpos = __builtin_amdgcn_ds_bpermute(kF << 2, tabR), fpos = __builtin_amdgcn_ds_bpermute(kR << 2, tabF);
                const bool swF = isF && kF < nR && lane < rpos, swR = isR && kR < nF && fpos < lane;
                const int swaps = __popcll(__ballot(swF));
                {
                    const int partner = swF ? rpos : fpos;
                    const uint32_t pk = (uint32_t)__builtin_amdgcn_ds_bpermute(partner << 2, (int)key), pid = (uint32_t)__builtin_amdgcn_ds_bpermute(partner << 2, (int)id);
                    if (swF || swR) { key = pk; id = pid; }
                }
                int cut;
                if (swaps >= 1) {
                    const int nextF = swaps < nF ? __builtin_amdgcn_readlane(tabF, swaps) : 0x7FFFFFFF;
                    cut = min(nextF, __builtin_amdgcn_readlane(tabR, swaps - 1));
                } else {
                    cut = __builtin_amdgcn_readlane(tabF, 0);
                }
                if (last - cut > 16) {
                    if (lane == sp) stack = cut | last << 8 | depth << 16;
                    sp++;
                }
                last = cut;
            }
        }
    }
    // __final_insertion_sort == stable sort inside each leaf of <= 16 == stable rank over a +-15 window (elements of other leaves never
    // count: left ones are <=, right ones >=).  The neighbours come by whole-wave DPP shifts, one lane further per step.
    int pos = lane;
    {
        const uint32_t kk = lane < n ? key : 0xFFFFFFFFu;
        int l = (int)kk, r = (int)kk;
#pragma unroll
        for (int d = 1; d <= 15; d++) {
            l = __builtin_amdgcn_update_dpp(0, l, 0x138, 0xF, 0xF, false);             // wave_shr:1 -> key of lane - d (0 beyond lane 0)
            r = __builtin_amdgcn_update_dpp(-1, r, 0x130, 0xF, 0xF, false);            // wave_shl:1 -> key of lane + d (max beyond lane 63)
            pos -= (uint32_t)l > kk ? 1 : 0;
            pos += (uint32_t)r < kk ? 1 : 0;
        }
    }
    if (lane < n) out[pos] = OctEntry{key, (uint16_t)id, 0};
}

// test hook: the workgroup sort on an arbitrary array (tests/test_extractor_gpu.py compares it with the real std::sort)
__global__ __launch_bounds__(kOctThreads) void k_sort_hook(OctEntry *data, int n) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    __shared__ int sCnt[2];
    OctEntry *a = reinterpret_cast<OctEntry *>(lds), *tmp = a + n;
    uint16_t *sf = reinterpret_cast<uint16_t *>(tmp + n), *sr = sf + n;
    SortSeg *segA = reinterpret_cast<SortSeg *>(lds + (((size_t)n * 20 + 7) & ~(size_t)7)), *segB = segA + (n / 16 + 2);
    for (int i = threadIdx.x; i < n; i += blockDim.x) a[i] = data[i];
    __syncthreads();
    if (n <= 64) {                                  // as the fine rounds of octree_level choose
        if (threadIdx.x < 64) {
            OctEntry e = OctEntry{0u, 0, 0};
            if ((int)threadIdx.x < n) e = a[threadIdx.x];
            wave_fence_lds();
            wave_sort_like_libstdcxx(e.key, e.id, n, tmp, a);
        }
        __syncthreads();
        for (int i = threadIdx.x; i < n; i += blockDim.x) a[i] = tmp[i];
        __syncthreads();
    } else {
        wg_sort_like_libstdcxx(a, n, tmp, sf, sr, segA, segB, sCnt);
    }
    for (int i = threadIdx.x; i < n; i += blockDim.x) data[i] = a[i];
}
int launch_sort_hook(uint32_t *keys, uint16_t *ids, int n) {
    if (n < 0 || n > 4096) return -1;
    if (n == 0) return 0;
    std::vector<OctEntry> h(n);
    for (int i = 0; i < n; i++) h[i] = OctEntry{keys[i], ids[i], 0};
    OctEntry *d = nullptr;
    if (hipMalloc((void **)&d, n * sizeof(OctEntry)) != hipSuccess) return -2;
    const size_t ldsBytes = (size_t)n * 20 + 8 + 2 * (size_t)(n / 16 + 2) * sizeof(SortSeg) + 64;
    (void)raise_lds_limit(reinterpret_cast<const void *>(k_sort_hook), ldsBytes);
    bool ok = hipMemcpy(d, h.data(), n * sizeof(OctEntry), hipMemcpyHostToDevice) == hipSuccess;
    if (ok) {
        hipLaunchKernelGGL(k_sort_hook, dim3(1), dim3(kOctThreads), ldsBytes, nullptr, d, n);
        ok = hipMemcpy(h.data(), d, n * sizeof(OctEntry), hipMemcpyDeviceToHost) == hipSuccess;
    }
    (void)hipFree(d);
    if (!ok) return -2;
    for (int i = 0; i < n; i++) { keys[i] = h[i].key; ids[i] = h[i].id; }
    return 0;
}

}  // namespace rumi
