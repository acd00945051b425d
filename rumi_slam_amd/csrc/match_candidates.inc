// Candidate lists of the matcher: count pass, scan, fill pass (or all three in one launch), one wave per query.  (Included inside namespace rumi.)
// ---- 3. candidates: one wave per query -----------------------------------------------------------------------------
// list entry: feature (16 bit) | distance (9 bit) << 16 | octave (4 bit) << 25
// Lists of up to kSortMax entries are stored SORTED by (distance, position in the reference's candidate order): the
// reference's "best / second best among the candidates not yet taken" is then simply the first / second not-taken entry
// (strict `<` keeps the earliest of equal distances, and a displaced best becomes the second), so a resolve round reads a
// couple of entries per query instead of the whole list.  Longer lists stay in candidate order and are scanned in full.
constexpr int kSortMax = 1024;
__device__ __forceinline__ void wave_lds_fence() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

template <int PASS> __device__ __forceinline__ int offsets_of(const int32_t *offsets, int qi, int listCap) { return PASS == 2 ? qi * listCap : offsets[qi]; }

// The candidates of one query, walked by one wave: FILL = false counts them, FILL = true computes their Hamming distances and stores them (into the
// wave's LDS sort arrays when they fit, else straight to `out`).  Returns the count.
template <bool FILL>
__device__ __forceinline__ int candidates_walk(int mode, const Query &Q, const FrameDev &F, const uint32_t (&qd)[8], const uint32_t *__restrict__ fvIdx, bool sorted,
                                               uint32_t *out, uint32_t *key, uint32_t *val, int lane) {
    int count = 0;
    if (mode == MODE_BOW || mode == MODE_BOW_KF) {
        for (int p = Q.c0 + lane; p - lane < Q.c1; p += 64) {
            const bool ok = p < Q.c1;
            if (FILL && ok) {
                const int idx = (int)fvIdx[p];
                const int d = hamming256(qd, reinterpret_cast<const uint32_t *>(F.desc + (size_t)idx * 32));
                const uint32_t e = (uint32_t)idx | ((uint32_t)d << 16);
                if (sorted) { key[p - Q.c0] = ((uint32_t)d << 10) | (uint32_t)(p - Q.c0); val[p - Q.c0] = e; }
                else out[p - Q.c0] = e;
            }
        }
        return Q.c1 - Q.c0;
    }
    const CellWindow W = cell_window(Q.u, Q.v, Q.r, F.minX, F.minY, F.wInv, F.hInv);       // Frame::GetFeaturesInArea (Frame.cc:695-750)
    if (W.any) {
        const bool checkLevels = Q.minLevel > 0 || Q.maxLevel >= 0;
        for (int ix = W.x0; ix <= W.x1; ix++) {
            const int p0 = F.cellStart[ix * kGridRows + W.y0], p1 = F.cellStart[ix * kGridRows + W.y1 + 1];
            for (int base = p0; base < p1; base += 64) {
                const int p = base + lane;
                bool pass = false;
                int idx = 0, oct = 0;
                if (p < p1) {
                    idx = F.sortedIdx[p];
                    const RumiKeyPoint kp = F.keys[idx];
                    oct = kp.octave;
                    pass = true;
                    if (checkLevels) {
                        if (oct < Q.minLevel) pass = false;
                        if (Q.maxLevel >= 0 && oct > Q.maxLevel) pass = false;
                    }
                    if (!window_gate(kp.x, kp.y, Q.u, Q.v, Q.r)) pass = false;
                    if (mode == MODE_FUSE && Q.c0 && pass && !reproj_gate(kp, Q.u, Q.v, F.scale)) pass = false;
                }
                const unsigned long long b = __ballot(pass);
                if (FILL && pass) {
                    const int d = hamming256(qd, reinterpret_cast<const uint32_t *>(F.desc + (size_t)idx * 32));
                    const int pos = count + __popcll(b & ((1ull << lane) - 1ull));
                    const uint32_t e = (uint32_t)idx | ((uint32_t)d << 16) | ((uint32_t)(oct & 15) << 25);
                    if (sorted) { key[pos] = ((uint32_t)d << 10) | (uint32_t)pos; val[pos] = e; }
                    else out[pos] = e;
                }
                count += __popcll(b);
            }
        }
    }
    return count;
}

// bitonic sort of one wave's (key, val) pairs in LDS by key, then the values to `out`
__device__ __forceinline__ void wave_bitonic_store(uint32_t *key, uint32_t *val, int total, uint32_t *out, int lane) {
    int m = 1;
    while (m < total) m <<= 1;
    for (int i = total + lane; i < m; i += 64) key[i] = 0xFFFFFFFFu;
    wave_lds_fence();
    for (int k = 2; k <= m; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = lane; t < (m >> 1); t += 64) {
                const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i | j;
                const uint32_t a = key[i], b = key[l];
                if ((a > b) == ((i & k) == 0)) {
                    key[i] = b; key[l] = a;
                    const uint32_t va = val[i]; val[i] = val[l]; val[l] = va;
                }
            }
            wave_lds_fence();
        }
    for (int i = lane; i < total; i += 64) out[i] = val[i];
}

// PASS 0: count pass (counts[q]).  PASS 1: fill pass at the offsets a scan of the counts produced.  PASS 2: both in one launch, every query's list
// in a fixed slot of `listCap` entries (offsets[q] = q * listCap written here): two dispatches (~4.5 us each) less per search; a query with more
// candidates than a slot raises kFusedOverflow and the host repeats the search with passes 0 / scan / 1.
template <int PASS>
__global__ __launch_bounds__(256) void k_candidates(int mode, int nq, const Query *__restrict__ q, FrameDev F,
                                                    const uint8_t *__restrict__ qDesc, const uint32_t *__restrict__ fvIdx,
                                                    int32_t *__restrict__ counts, int32_t *__restrict__ offsets,
                                                    uint32_t *__restrict__ lists, int listCap, int32_t *__restrict__ overflow) {
    constexpr bool FILL = PASS != 0;
    __shared__ uint32_t sKey[FILL ? 4 * kSortMax : 1], sVal[FILL ? 4 * kSortMax : 1];
    const int lane = threadIdx.x & 63;
    const int qi = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (qi >= nq) return;
    if (PASS == 1 && offsets[nq] > listCap) {            // the arena cannot hold this call's lists: report the need, write nothing
        if (qi == 0 && lane == 0) *overflow = offsets[nq];
        return;
    }
    const Query Q = q[qi];
    if (PASS == 2 && lane == 0) offsets[qi] = qi * listCap;
    if (!Q.valid) {
        if (PASS != 1 && lane == 0) counts[qi] = 0;
        return;
    }
    uint32_t *key = sKey + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6) * kSortMax, *val = sVal + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6) * kSortMax;
    uint32_t qd[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    int total = 0;
    if (PASS == 2 && mode != MODE_BOW && mode != MODE_BOW_KF) {
        // The usual search of the Tracking thread (a window of a few grid columns, a handful of candidates) as ONE dependent chain
        // instead of two walks of four loads per column: the cell ranges of all columns at once (one lane each), the window's
        // feature slots flat over the lanes (slot -> column by the prefix of the range lengths: the reference's candidate order),
        // key-point and descriptor of every slot fetched together, and up to 64 candidates ranked in registers.
        const CellWindow W = cell_window(Q.u, Q.v, Q.r, F.minX, F.minY, F.wInv, F.hInv);
        const int ncol = W.any ? max(0, W.x1 - W.x0 + 1) : 0;
        int c0 = 0, len = 0;
        if (lane < ncol) {
            const int cell = (W.x0 + lane) * kGridRows;
            c0 = F.cellStart[cell + W.y0];
            len = F.cellStart[cell + W.y1 + 1] - c0;
        }
        const uint32_t qmine = reinterpret_cast<const uint32_t *>(qDesc + (size_t)Q.descId * 32)[lane & 7];
        const int incl = wave_scan_incl_i32(len);
        const int T = __builtin_amdgcn_readlane(incl, 63);
        if (T <= kSortMax) {
#pragma unroll
            for (int k = 0; k < 8; k++) qd[k] = __shfl(qmine, k);
            const bool checkLevels = Q.minLevel > 0 || Q.maxLevel >= 0;
            uint32_t *out = lists + qi * listCap;
            int count = 0;
            uint32_t myKey = 0xFFFFFFFFu, myVal = 0;
            unsigned long long b = 0;
            for (int base = 0; base < T; base += 64) {
                const int sl = base + lane;
                const bool live = sl < T;
                int col = 0;
                for (int c = 0; c < ncol; c++) col += __builtin_amdgcn_readlane(incl, c) <= sl;
                const int cc = live ? col : 0;
                const int p = __shfl(c0, cc) + (sl - (__shfl(incl, cc) - __shfl(len, cc)));
                bool pass = false;
                int idx = 0, oct = 0, d = 0;
                if (live) {
                    idx = F.sortedIdx[p];
                    const RumiKeyPoint kp = F.keys[idx];
                    const uint4 *dp = reinterpret_cast<const uint4 *>(F.desc + (size_t)idx * 32);
                    const uint4 d0 = dp[0], d1 = dp[1];
                    oct = kp.octave;
                    pass = true;
                    if (checkLevels) {
                        if (oct < Q.minLevel) pass = false;
                        if (Q.maxLevel >= 0 && oct > Q.maxLevel) pass = false;
                    }
                    if (!window_gate(kp.x, kp.y, Q.u, Q.v, Q.r)) pass = false;
                    if (mode == MODE_FUSE && Q.c0 && pass && !reproj_gate(kp, Q.u, Q.v, F.scale)) pass = false;
                    d = hamming256(make_uint4(qd[0], qd[1], qd[2], qd[3]), make_uint4(qd[4], qd[5], qd[6], qd[7]), d0, d1);
                }
                b = __ballot(pass);
                if (pass) {
                    const int pos = count + __popcll(b & ((1ull << lane) - 1ull));
                    myKey = ((uint32_t)d << 10) | (uint32_t)pos;
                    myVal = (uint32_t)idx | ((uint32_t)d << 16) | ((uint32_t)(oct & 15) << 25);
                    if (T > 64) { key[pos] = myKey; val[pos] = myVal; }
                }
                count += __popcll(b);
            }
            if (lane == 0) counts[qi] = count;
            if (count > listCap) {
                if (lane == 0) atomicExch(overflow, kFusedOverflow);
                return;
            }
            if (T <= 64) {                                                  // one trip: rank among the passing lanes (keys are distinct)
                int rank = 0;
                for (unsigned long long bb = b; bb; bb &= bb - 1) {
                    const uint32_t kj = (uint32_t)__builtin_amdgcn_readlane((int)myKey, __builtin_ctzll(bb));
                    rank += kj < myKey;
                }
                if (myKey != 0xFFFFFFFFu) out[rank] = myVal;
            } else if (count > 0) {
                wave_bitonic_store(key, val, count, out, lane);
            }
            return;
        }
    }
    if (PASS == 0 || PASS == 2) {
        total = candidates_walk<false>(mode, Q, F, qd, fvIdx, false, nullptr, key, val, lane);
        if (lane == 0) counts[qi] = total;
        if (PASS == 0) return;
        if (total > listCap) {
            if (lane == 0) atomicExch(overflow, kFusedOverflow);
            return;
        }
    } else total = counts[qi];
    const bool sorted = total <= kSortMax;
    {
        const uint32_t *src = reinterpret_cast<const uint32_t *>(qDesc + (size_t)Q.descId * 32);
        const uint32_t mine = src[lane & 7];
#pragma unroll
        for (int k = 0; k < 8; k++) qd[k] = __shfl(mine, k);
    }
    uint32_t *out = lists + offsets_of<PASS>(offsets, qi, listCap);
    candidates_walk<true>(mode, Q, F, qd, fvIdx, sorted, out, key, val, lane);
    if (sorted && total > 0) wave_bitonic_store(key, val, total, out, lane);
}

// exclusive scan of counts -> offsets (single workgroup; nq is a few thousand)
__global__ __launch_bounds__(256) void k_scan(int n, const int32_t *__restrict__ counts, int32_t *__restrict__ offsets) {
    __shared__ int part[256];
    const int tid = threadIdx.x, chunk = (n + 255) / 256;
    int s = 0;
    for (int k = 0; k < chunk; k++) { const int i = tid * chunk + k; if (i < n) s += counts[i]; }
    part[tid] = s;
    __syncthreads();
    if (tid == 0) { int run = 0; for (int i = 0; i < 256; i++) { const int t = part[i]; part[i] = run; run += t; } offsets[n] = run; }
    __syncthreads();
    int run = part[tid];
    for (int k = 0; k < chunk; k++) { const int i = tid * chunk + k; if (i < n) { offsets[i] = run; run += counts[i]; } }
}
