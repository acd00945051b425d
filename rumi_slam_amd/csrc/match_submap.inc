// The key-point match of CloudMerging::ComputeSubmapSim3 (CloudMerging.cc:503-551) for every matched key-frame pair in one call: rumi_submap_match.
//
// The reference: for every key-point i1 of key-frame 1, KeyFrame::GetFeaturesInArea(mvKeys1[i1], 3) in key-frame 2 (KeyFrame.cc:887-925, mono),
// then the nearest candidate by the pixel distance of the two mvKeys, among the candidates whose slot and the query's slot both hold a map point.
// The frames carry no descriptors, so there is nothing for a wave to share: a query sees a handful of candidates and spends a few flops on each.
// One lane per query, all pairs in one launch:
//   k_grid_batch      the 64x48 grid of every frame that stands on side 2, one workgroup per frame (k_grid's sort, restated over x, y pairs)
//   k_submap_match    grid (ceil(max n1 / 256), pairs): best2 per query, and the number of matches of every block
//   k_submap_compact  same grid: (i1, i2) in ascending i1 per pair, packed pair after pair, and pair_start (the block counts are the scan's input)
// Three launches whatever the number of pairs; the uploads travel as one pinned block through k_scatter.
namespace rumi {

struct SubFrame {
    const float *keys;          // mvKeys[i].pt, n x 2
    const float *keysUn;        // mvKeysUn[i].pt, n x 2
    const uint8_t *hasMp;       // n
    int32_t n;
    float minX, minY, wInv, hInv;
    int32_t grid;               // which grid of the call is this frame's (-1: the frame stands on side 1 only)
    int32_t sortedOff;          // where its sorted indices start
};
struct SubPair { int32_t f1, f2, qStart, pad; };

__global__ __launch_bounds__(1024) void k_grid_batch(const SubFrame *__restrict__ frames, const int32_t *__restrict__ gridFrames, uint16_t *__restrict__ sorted,
                                                     int32_t *__restrict__ cellStart) {
    const SubFrame F = frames[gridFrames[blockIdx.x]];
    grid_build_xy<2>(F.n, F.keysUn, F.minX, F.minY, F.wInv, F.hInv, sorted + F.sortedOff, cellStart + (size_t)blockIdx.x * (kGridCells + 1));
}

// The number of set predicates in the workgroup (256 threads) in front of this thread, and the workgroup's total.
__device__ __forceinline__ int block_rank_256(bool pred, int *sWave /* [4] */, int *total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long b = __ballot(pred);
    if (lane == 0) sWave[wave] = __popcll(b);
    __syncthreads();
    int before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < 4; w++) { const int t = sWave[w]; all += t; if (w < wave) before += t; }
    *total = all;
    return before + __popcll(b & ((1ull << lane) - 1ull));
}

__global__ __launch_bounds__(256) void k_submap_match(const SubFrame *__restrict__ frames, const SubPair *__restrict__ pairs, const uint16_t *__restrict__ sorted,
                                                      const int32_t *__restrict__ cellStart, float r, int32_t *__restrict__ best2, int32_t *__restrict__ blockCount) {
    __shared__ int sWave[4];
    const SubPair P = pairs[blockIdx.y];
    const SubFrame A = frames[P.f1], B = frames[P.f2];
    const int i1 = blockIdx.x * 256 + threadIdx.x;
    int best = -1;
    if (i1 < A.n && A.hasMp[i1]) {            // a query without a map point keeps nothing, whatever its candidates are (:532)
        const float u = A.keys[2 * i1], v = A.keys[2 * i1 + 1];
        // KeyFrame::GetFeaturesInArea(u, v, r), KeyFrame.cc:894-908, with its four early returns
        const CellWindow W = cell_window(u, v, r, B.minX, B.minY, B.wInv, B.hInv);
        if (W.any) {
            const uint16_t *S = sorted + B.sortedOff;
            const int32_t *CS = cellStart + (size_t)B.grid * (kGridCells + 1);
            float bestDist = r;
            for (int ix = W.x0; ix <= W.x1; ix++) {
                // the cells of one column lie one behind the other, each in ascending key-point index: the reference's candidate order
                const int p0 = CS[ix * kGridRows + W.y0], p1 = CS[ix * kGridRows + W.y1 + 1];
                for (int p = p0; p < p1; p++) {
                    const int i2 = S[p];
                    if (!window_gate(B.keysUn[2 * i2], B.keysUn[2 * i2 + 1], u, v, r)) continue;     // the gate: mvKeysUn of key-frame 2 against mvKeys of 1
                    // (float)sqrt(pow(u1 - u2, 2) + pow(v1 - v2, 2)), :531: float differences of the two mvKeys, the rest in double
                    const double ex = (double)(u - B.keys[2 * i2]), ey = (double)(v - B.keys[2 * i2 + 1]);
                    const float d = (float)sqrt(ex * ex + ey * ey);
                    if (d < bestDist && B.hasMp[i2]) { best = i2; bestDist = d; }
                }
            }
        }
    }
    if (i1 < A.n) best2[P.qStart + i1] = best;
    int total;
    block_rank_256(best >= 0, sWave, &total);
    if (threadIdx.x == 0) blockCount[blockIdx.y * gridDim.x + blockIdx.x] = total;
}

__global__ __launch_bounds__(256) void k_submap_compact(const SubFrame *__restrict__ frames, const SubPair *__restrict__ pairs, const int32_t *__restrict__ best2,
                                                        const int32_t *__restrict__ blockCount, int32_t *__restrict__ pairStart, int32_t *__restrict__ matches) {
    __shared__ int sWave[4], sSum[4];
    const SubPair P = pairs[blockIdx.y];
    const int n1 = frames[P.f1].n;
    // matches of every block in front of this one: the earlier pairs, then the earlier blocks of this pair
    const int mine = blockIdx.y * gridDim.x + blockIdx.x;
    int part = 0;
    for (int k = threadIdx.x; k < mine; k += 256) part += blockCount[k];
    part = wave_sum_i32(part);
    if ((threadIdx.x & 63) == 0) sSum[threadIdx.x >> 6] = part;
    __syncthreads();
    const int base = sSum[0] + sSum[1] + sSum[2] + sSum[3];
    const int i1 = blockIdx.x * 256 + threadIdx.x;
    const int i2 = i1 < n1 ? best2[P.qStart + i1] : -1;
    int total;
    const int rank = block_rank_256(i2 >= 0, sWave, &total);
    if (i2 >= 0) { matches[2 * (size_t)(base + rank)] = i1; matches[2 * (size_t)(base + rank) + 1] = i2; }
    if (threadIdx.x == 0) {
        if (blockIdx.x == 0) pairStart[blockIdx.y] = base;
        if (blockIdx.x == gridDim.x - 1 && blockIdx.y == gridDim.y - 1) pairStart[gridDim.y] = base + total;
    }
}

static size_t sub_align(size_t v) { return (v + 15) & ~(size_t)15; }

}  // namespace rumi

extern "C" int rumi_submap_match(RumiMatcher *m, int32_t n_frames, const RumiSubmapFrame *frames, int32_t n_pairs, const int32_t *pair_f1, const int32_t *pair_f2,
                                 float tolerance, int32_t *best2, int32_t *pair_start, int32_t *matches) {
    // ---- what is refused, before anything touches the device or the outputs ----
#define SUB_REFUSE(msg) do { g_lastError = "rumi_submap_match: " msg; return RUMI_E_INVALID; } while (0)
    if (n_frames < 0 || n_pairs < 0 || (n_frames > 0 && !frames) || (n_pairs > 0 && (!pair_f1 || !pair_f2))) SUB_REFUSE("bad frame table or pair list");
    if (!pair_start || !best2 || !matches) SUB_REFUSE("an output array is NULL");
    if (!(tolerance > 0.f) || !std::isfinite(tolerance)) SUB_REFUSE("tolerance must be a positive finite number");
    for (int f = 0; f < n_frames; f++) {
        const RumiSubmapFrame &F = frames[f];
        if (F.n < 0 || F.n > kMaxSortN) SUB_REFUSE("a frame has more key-points than the grid kernel sorts (16384), or a negative count");
        if (F.n > 0 && (!F.keys_xy || !F.has_mp)) SUB_REFUSE("a frame's keys_xy or has_mp is NULL");
        if (!std::isfinite(F.min_x) || !std::isfinite(F.min_y) || !std::isfinite(F.grid_w_inv) || !std::isfinite(F.grid_h_inv))
            SUB_REFUSE("a frame's bounds (min_x, min_y, grid_w_inv, grid_h_inv) are not finite");
    }
    for (int p = 0; p < n_pairs; p++)
        if (pair_f1[p] < 0 || pair_f1[p] >= n_frames || pair_f2[p] < 0 || pair_f2[p] >= n_frames) SUB_REFUSE("a pair names a frame outside the frame table");
    if (!m) SUB_REFUSE("the matcher handle is NULL");
#undef SUB_REFUSE
    if (n_pairs == 0) { pair_start[0] = 0; return RUMI_OK; }
    HIP_TRY(hipSetDevice(m->device));

    // ---- layout.  dSub: [SubFrame F | SubPair P | grid list G | key-points of the host frames] (the upload), then [cellStart | sorted | block counts] ----
    std::vector<int8_t> side(n_frames, 0);                  // bit 0: stands on side 1 of some pair, bit 1: on side 2
    int maxN1 = 0;
    size_t sumQ = 0;
    for (int p = 0; p < n_pairs; p++) {
        side[pair_f1[p]] |= 1; side[pair_f2[p]] |= 2;
        maxN1 = std::max(maxN1, frames[pair_f1[p]].n);
        sumQ += (size_t)frames[pair_f1[p]].n;
    }
    std::vector<SubFrame> hf(n_frames);
    std::vector<int32_t> gridList;
    std::vector<size_t> oKeys(n_frames, 0), oUn(n_frames, 0), oMp(n_frames, 0);
    size_t sumGridN = 0;
    const size_t oPairs = sub_align((size_t)n_frames * sizeof(SubFrame)), oGridList = sub_align(oPairs + (size_t)n_pairs * sizeof(SubPair));
    for (int f = 0; f < n_frames; f++)
        if (side[f] & 2) { hf[f].grid = (int32_t)gridList.size(); hf[f].sortedOff = (int32_t)sumGridN; gridList.push_back(f); sumGridN += (size_t)frames[f].n; }
        else { hf[f].grid = -1; hf[f].sortedOff = 0; }
    size_t up = sub_align(oGridList + gridList.size() * sizeof(int32_t));
    for (int f = 0; f < n_frames; f++) {
        const RumiSubmapFrame &F = frames[f];
        if (!side[f] || F.on_device || F.n == 0) continue;
        oKeys[f] = up; up = sub_align(up + (size_t)F.n * 8);
        if ((side[f] & 2) && F.keys_un_xy) { oUn[f] = up; up = sub_align(up + (size_t)F.n * 8); }
        oMp[f] = up; up = sub_align(up + (size_t)F.n);
    }
    const int gx = std::max(1, (maxN1 + 255) / 256);
    const size_t oCell = up, oSorted = sub_align(oCell + gridList.size() * (kGridCells + 1) * sizeof(int32_t));
    const size_t oBlocks = sub_align(oSorted + sumGridN * sizeof(uint16_t)), total = oBlocks + (size_t)n_pairs * gx * sizeof(int32_t);
    const size_t outInts = (size_t)n_pairs + 1 + 3 * sumQ;              // [pair_start P + 1 | best2 sumQ | matches 2 sumQ]
    RC_TRY(m->sub.reserve(total, total * 2));
    RC_TRY(m->subOut.reserve(outInts * sizeof(int32_t), outInts * sizeof(int32_t) * 2));
    reset_uploads(m);
    constexpr int kChunks = 24;                                          // segments of the one block: k_scatter gives each eight workgroups
    { const size_t stageBytes = kStageHeader + up + 16 * (kChunks + 1); RC_TRY(m->stage.reserve(stageBytes, stageBytes * 2)); }

    // ---- pack the upload straight into the pinned mirror, in chunks that k_scatter copies side by side ----
    const size_t chunk = sub_align((up + kChunks - 1) / kChunks);
    uint8_t *h0 = nullptr;
    for (size_t o = 0; o < up; o += chunk) {
        uint8_t *h = stage_reserve(m, m->sub.p + o, std::min(chunk, up - o));
        if (!h) { reset_uploads(m); return RUMI_E_CAPACITY; }
        if (!h0) h0 = h;                                                 // every chunk is a multiple of 16 bytes: the chunks are contiguous in the mirror
    }
    for (int f = 0; f < n_frames; f++) {
        const RumiSubmapFrame &F = frames[f];
        SubFrame &D = hf[f];
        D.n = F.n; D.minX = F.min_x; D.minY = F.min_y; D.wInv = F.grid_w_inv; D.hInv = F.grid_h_inv;
        D.keys = D.keysUn = nullptr; D.hasMp = nullptr;
        if (!side[f] || F.n == 0) continue;
        if (F.on_device) { D.keys = F.keys_xy; D.keysUn = F.keys_un_xy ? F.keys_un_xy : F.keys_xy; D.hasMp = F.has_mp; continue; }
        D.keys = reinterpret_cast<const float *>(m->sub.p + oKeys[f]);
        D.keysUn = oUn[f] ? reinterpret_cast<const float *>(m->sub.p + oUn[f]) : D.keys;
        D.hasMp = m->sub.p + oMp[f];
        std::memcpy(h0 + oKeys[f], F.keys_xy, (size_t)F.n * 8);
        if (oUn[f]) std::memcpy(h0 + oUn[f], F.keys_un_xy, (size_t)F.n * 8);
        std::memcpy(h0 + oMp[f], F.has_mp, (size_t)F.n);
    }
    std::memcpy(h0, hf.data(), (size_t)n_frames * sizeof(SubFrame));
    SubPair *hp = reinterpret_cast<SubPair *>(h0 + oPairs);
    size_t q = 0;
    for (int p = 0; p < n_pairs; p++) { hp[p] = SubPair{pair_f1[p], pair_f2[p], (int32_t)q, 0}; q += (size_t)frames[pair_f1[p]].n; }
    std::memcpy(h0 + oGridList, gridList.data(), gridList.size() * sizeof(int32_t));
    FLUSH(m);

    // ---- the three launches, one copy back ----
    const SubFrame *dFrames = reinterpret_cast<const SubFrame *>(m->sub.p);
    const SubPair *dPairs = reinterpret_cast<const SubPair *>(m->sub.p + oPairs);
    int32_t *dCell = reinterpret_cast<int32_t *>(m->sub.p + oCell), *dBlocks = reinterpret_cast<int32_t *>(m->sub.p + oBlocks);
    uint16_t *dSorted = reinterpret_cast<uint16_t *>(m->sub.p + oSorted);
    int32_t *dPairStart = reinterpret_cast<int32_t *>(m->subOut.d), *dBest = dPairStart + n_pairs + 1, *dMatches = dBest + sumQ;
    hipLaunchKernelGGL(k_grid_batch, dim3((unsigned)gridList.size()), dim3(1024), 0, nullptr, dFrames, reinterpret_cast<const int32_t *>(m->sub.p + oGridList), dSorted, dCell);
    hipLaunchKernelGGL(k_submap_match, dim3(gx, n_pairs), dim3(256), 0, nullptr, dFrames, dPairs, dSorted, dCell, tolerance, dBest, dBlocks);
    hipLaunchKernelGGL(k_submap_compact, dim3(gx, n_pairs), dim3(256), 0, nullptr, dFrames, dPairs, dBest, dBlocks, dPairStart, dMatches);
    HIP_TRY(hipGetLastError());
    // pair_start and best2 first; the list is as long as pair_start says
    HIP_TRY(hipMemcpy(m->subOut.h, m->subOut.d, ((size_t)n_pairs + 1 + sumQ) * sizeof(int32_t), hipMemcpyDeviceToHost));
    const int32_t *ho = reinterpret_cast<const int32_t *>(m->subOut.h);
    const size_t nm = (size_t)ho[n_pairs];
    if (nm > sumQ) { g_lastError = "rumi_submap_match: the device reports more matches than queries"; return RUMI_E_NO_DEVICE; }
    int32_t *hm = reinterpret_cast<int32_t *>(m->subOut.h) + n_pairs + 1 + sumQ;
    if (nm > 0) HIP_TRY(hipMemcpy(hm, dMatches, nm * 2 * sizeof(int32_t), hipMemcpyDeviceToHost));
    std::memcpy(matches, hm, nm * 2 * sizeof(int32_t));
    std::memcpy(pair_start, ho, ((size_t)n_pairs + 1) * sizeof(int32_t));
    std::memcpy(best2, ho + n_pairs + 1, sumQ * sizeof(int32_t));
    return RUMI_OK;
}
