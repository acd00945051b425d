// The Gaussian blur of the pyramid: k_blur (a few frames), k_blur_packed (batches), k_fast_blur (FAST and blur of a few frames in one launch),
// the grid builders and the launch wrappers.
namespace rumi {

// ------------------------------------------------------------------------------------------------
// Gaussian blur 7x7, sigma 2, fixed point: taps {18,34,48,56,48,34,18}/256, row pass to u16, column
// pass to u32, (v + 32768) >> 16, BORDER_REFLECT_101 at the level's own edges.
// ------------------------------------------------------------------------------------------------
// Register formulation: a lane owns a 4-pixel column strip, a wave walks kBlurRows output rows top to bottom.
// Per source row: ONE aligned dword load per lane; the left / right neighbours' dwords arrive by DPP shuffles (the two
// outer lanes load their halo dwords); the 7-tap row pass runs on the 10 unpacked bytes, the column pass on a 7-deep
// register ring of row results; 4 output pixels leave as one dword store.  No LDS, no barriers.
// Edges (no border is stored around a level): rows above / below the level are the mirrored rows (a row index, wave-uniform); the three
// columns left of column 0 are bytes 3, 2, 1 of the first dword (one v_perm_b32 in the first strip block); columns from w on are mirrored
// bytes fetched by the few lanes whose dword touches them (byte loads of the same cache lines, only in waves that hold the right edge).
// output rows a wave walks: 64 for batches (6 halo rows per 64: +1.3 % on the pipelined step over 32, which was +1.7 % over 16), 16 for a few
// frames (a wave's walk is a chain of dependent row loads and one frame fills few waves: the device chain of a one-frame call takes 107-110 us
// with 16 rows, 116-126 with 32, 103-117 with 8 or 4 on the same box)
constexpr int kBlurRowsSmall = 16, kBlurRowsBatch = 64;

// all levels in one launch: workgroup `lin` of a frame belongs to the level whose [base, base + gx * gy) range holds it
struct BlurGrid { int base[kMaxLevels + 1]; int gx[kMaxLevels]; int bw[kMaxLevels]; };   // bw: pixels a wave's strips cover (256, or less: see launch_blur)
// Batches (kPacked): the rows of G[l] consecutive frames side by side (LanePack, orb_geom.h) in a ONE-dimensional grid, level after level:
// level l owns the workgroups [base[l], base[l + 1]), group-major, then row block, then the gx[l] waves along the group's row.  The strips
// and the outer lanes' halo loads above are gone: a wave's lanes 0 and 63 only hold the dwords lanes 1 and 62 need, every seam and edge
// is a per-lane predicate, and nothing but the lane's address offset knows its frame.
struct BlurPack { int base[kMaxLevels + 1]; int gx[kMaxLevels], gy[kMaxLevels], G[kMaxLevels]; unsigned M[kMaxLevels]; int nframes; };
// a * b + c on 24-bit operands as ONE v_mad_u32_u24 (the compiler splits the C expression into a multiply and a 3-input add)
__device__ __forceinline__ uint32_t mad_u24(uint32_t a, uint32_t b, uint32_t c) {
    uint32_t r;
    asm("v_mad_u32_u24 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
}
// VARIANT: RumiOrbConfig.blur_variant -- 0: taps {18,34,48,56,..}/256 of the fixed-point GaussianBlur of OpenCV >= 3.4.2; 1: the integer-scaled float
// kernel {18,34,49,55,..}/256 of 3.4.0 / 3.4.1 (sum 257: the result is saturated)
template <int VARIANT, int kBlurRows, bool kPacked, typename Grid>
__device__ __forceinline__ void blur_body(const DevParams *__restrict__ P, const ImgSrc &src, const Grid &G, unsigned bxg, unsigned gxg) {
    constexpr uint32_t kT2 = VARIANT ? 49u : 48u, kT3 = VARIANT ? 55u : 56u;      // taps at distance 1 and 0 (18 and 34 are common)
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);      // (scalar: the row walk is scalar arithmetic)
    const unsigned wg = kPacked ? xcd_swizzle(bxg, gxg) : xcd_swizzle(blockIdx.y * gxg + bxg, gxg * gridDim.y);
    const int lin = kPacked ? wg : wg % gxg;
    int frame = kPacked ? 0 : wg / gxg;                          // (packed: the first frame of the wave's group)
    int level = 0;
    for (int l = 1; l < P->nlevels; l++)
        if (lin >= G.base[l]) level = l;
    const DevLevel &L = P->lv[level];
    int bx, by, bw, xa;
    uint32_t fsrc = 0, fdst = 0;                                 // packed: my frame's byte offset from the group's first frame, source and blurred arena
    bool produce, first = false;
    if constexpr (kPacked) {
        const int per = G.gx[level] * G.gy[level], idx = lin - G.base[level], group = idx / per;
        bx = (idx - group * per) % G.gx[level]; by = (idx - group * per) / G.gx[level];
        frame = group * G.G[level];
        const LanePack K{blur_lanes_per_row(L.w), 1, G.G[level], 62, 1, G.gx[level], G.M[level]};
        const LaneSlot slot = lane_slot(K, bx, lane);
        // lanes beyond the group's last frame (or, in the launch's last group, beyond the last frame) walk along on frame 0 of the group and store nothing
        const bool mine = lane_frame(K, slot, group, G.nframes) >= 0;
        const uint32_t f = mine ? (uint32_t)slot.frame : 0u;
        fsrc = f * (uint32_t)(level == 0 ? src.l0FrameStride : P->arenaStride); fdst = f * (uint32_t)P->arenaStride;
        bw = 256; xa = slot.col * 4;
        produce = mine && slot.produce; first = slot.first;
    } else {
        bx = (lin - G.base[level]) % G.gx[level]; by = (lin - G.base[level]) / G.gx[level];
        bw = G.bw[level];
        xa = bx * bw + lane * 4;                                 // first pixel of my strip (lanes from bw / 4 on only feed their left neighbour's halo)
    }
    const int y0 = (by * 4 + wave) * kBlurRows;
    if (y0 >= L.h) return;                                       // whole wave (wave-uniform)
    int pitch;
    const uint8_t *img = level_base(src, P, level, frame, &pitch);
    uint8_t *out = src.blur + (long long)frame * P->arenaStride + L.off + fdst;
    const int w = L.w, h = L.h;
    // Right edge.  The dword that holds column w - 1 may be partial and the one after it lies wholly beyond the row, yet both feed the
    // halos of the last strips: their missing bytes are the mirrored columns 2 (w - 1) - x, which sit in the same lane or one / two lanes to
    // the left.  In the wave that holds the edge every lane rebuilds its dword from {own, left, left-left} with two v_perm_b32 whose
    // selectors are fixed per lane (identity away from the edge).  The host picks the strip width of a level (G.bw) so that the partial dword
    // is never lane 0 or 1 of a wave and a wave's last producing lane never needs a halo dword from beyond the row edge out of memory.
    const int xLast = (w - 1) & ~3;                              // last dword that holds a pixel of the row
    const int xl = min(xa, xLast);
    const bool firstBlock = bx == 0;
    // a dword of this wave (its right halo included) reaches column w or beyond (wave-uniform); packed: a frame's right edge may lie anywhere
    // in the wave, and so may a frame's first dword
    const bool edgeWave = kPacked ? __builtin_amdgcn_ballot_w64(xa + 3 >= w) != 0 : bx * bw + bw + 4 > w;
    const bool seamWave = kPacked && __builtin_amdgcn_ballot_w64(first) != 0;
    if constexpr (!kPacked) produce = lane * 4 < bw && xa < w;
    uint32_t selA = 0x03020100u, selB = 0x07060504u;             // identity: keep my own four bytes
    if (edgeWave && xa + 3 >= w && xa <= xLast + 4) {
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const int x = xa + i;
            if (x < w) continue;
            const int sx = 2 * (w - 1) - x, d = (xa - (sx & ~3)) >> 2;                 // mirrored column, lanes to the left (0, 1 or 2 for every byte that is used)
            const uint32_t a = (d == 1 ? 4u : 0u) + (uint32_t)(sx & 3);                 // byte of {left-left (0-3), left (4-7)}
            const uint32_t b = d == 0 ? 4u + (uint32_t)(sx & 3) : (uint32_t)i;          // byte of {gathered (0-3), own (4-7)}
            selA = (selA & ~(0xFFu << (8 * i))) | (a << (8 * i));
            selB = (selB & ~(0xFFu << (8 * i))) | (b << (8 * i));
        }
    }
    int ring[7][4];                                              // row results of the last seven source rows; slot = source row mod 7 of this walk
#pragma unroll
    for (int k = 0; k < 7; k++)
#pragma unroll
        for (int i = 0; i < 4; i++) ring[k][i] = 0;
    const int yEnd = min(y0 + kBlurRows, h), rEnd = yEnd + 3;
    // the walk is unrolled by seven so that the ring never moves: source row r0 + j lands in slot j, and the taps of the output row it
    // completes sit at compile-time slots (a runtime ring costs 24 register moves per row)
    uint8_t *orow = out + (long long)(y0 - 6) * L.pitch + xa - L.pitch;
    // the halo dword of the wave's outer lanes: lane 0 reads the dword left of its own (but in the first strip block, where it is the mirrored
    // bytes of its own), lane 63 of a 256-pixel wave the one to the right
    const int haloOff = kPacked ? 0 : lane == 0 ? (firstBlock ? 0 : -4) : (lane == 63 && !edgeWave && bw == 256 ? 4 : 0);
    // the source rows of the NEXT seven are fetched while the current seven are filtered (a wave's walk is otherwise a chain of
    // load -> filter -> load; rows past the walk's end re-read its last row).  256 frames alone on the device: 260 -> 192 us at 83 registers
    // (5 waves a SIMD); forced to 80 registers / 6 waves (one spill) 217 us, held at 4 waves 207 us, two register sets taking turns 88 registers
    uint32_t Cn[7], Hn[7];
    auto fetch = [&](int r, uint32_t &C, uint32_t &H) {
        const int rc = min(r, rEnd - 1);
        const int rr = rc < 0 ? -rc : (rc >= h ? 2 * (h - 1) - rc : rc);        // rows -3..-1 and h..h+2 mirror into the level
        const uint8_t *row = img + (long long)rr * pitch;           // (scalar)
        if constexpr (kPacked) row += fsrc + (uint32_t)xl; else row += xl;
        C = *reinterpret_cast<const uint32_t *>(row);
        H = 0;
        if (!kPacked && haloOff) H = *reinterpret_cast<const uint32_t *>(row + haloOff);
    };
#pragma unroll
    for (int j = 0; j < 7; j++) fetch(y0 - 3 + j, Cn[j], Hn[j]);
    uint32_t Cm[7], Hm[7];                                       // the seven being filtered
    auto walk7 = [&](const uint32_t (&Cc)[7], const uint32_t (&Hc)[7], int r0) {
#pragma unroll
        for (int j = 0; j < 7; j++) {
            const int r = r0 + j;
            if (r >= rEnd) break;                                // wave-uniform
            orow += L.pitch;
            uint32_t C = Cc[j];
            if (edgeWave) {
                const uint32_t c1 = __shfl_up(C, 1), c2 = __shfl_up(c1, 1);
                C = __builtin_amdgcn_perm(C, __builtin_amdgcn_perm(c1, c2, selA), selB);
            }
            uint32_t Lw = __shfl_up(C, 1), Rw = __shfl_down(C, 1);
            if constexpr (kPacked) {
                // no shuffled dword crosses a seam into a producing lane: a frame's first dword mirrors its own bytes, its last producing
                // dword has the frame's rebuilt halo dword to its right
                if (seamWave && first) Lw = __builtin_amdgcn_perm(C, C, 0x01020300u);
            } else {
                if (lane == 0) Lw = firstBlock ? __builtin_amdgcn_perm(C, C, 0x01020300u) : Hc[j];
                if (lane == 63 && !edgeWave && bw == 256) Rw = Hc[j];   // (only a 256-pixel wave has a producing lane 63)
            }
            // row pass on packed bytes: output i needs the 7 bytes S[i+1 .. i+7] of the 12-byte run {Lw, C, Rw}; two byte-dot-products
            // (v_dot4_u32_u8) against the taps {18,34,48,56} and {48,34,18,0} give the exact integer sum (<= 65 280)
            constexpr uint32_t tA = 18u | (34u << 8) | (kT2 << 16) | (kT3 << 24), tB = kT2 | (34u << 8) | (18u << 16);
            const uint32_t A0 = __builtin_amdgcn_alignbyte(C, Lw, 1), A1 = __builtin_amdgcn_alignbyte(C, Lw, 2), A2 = __builtin_amdgcn_alignbyte(C, Lw, 3);
            const uint32_t B0 = __builtin_amdgcn_alignbyte(Rw, C, 1), B1 = __builtin_amdgcn_alignbyte(Rw, C, 2), B2 = __builtin_amdgcn_alignbyte(Rw, C, 3);
            ring[j][0] = (int)__builtin_amdgcn_udot4(B0, tB, __builtin_amdgcn_udot4(A0, tA, 0u, false), false);
            ring[j][1] = (int)__builtin_amdgcn_udot4(B1, tB, __builtin_amdgcn_udot4(A1, tA, 0u, false), false);
            ring[j][2] = (int)__builtin_amdgcn_udot4(B2, tB, __builtin_amdgcn_udot4(A2, tA, 0u, false), false);
            ring[j][3] = (int)__builtin_amdgcn_udot4(Rw, tB, __builtin_amdgcn_udot4(C, tA, 0u, false), false);
            const int y = r - 3;                                 // slots (j+1)%7 .. j now hold rows y-3 .. y+3
            if (y >= y0 && produce) {
                uint32_t o[4];
#pragma unroll
                for (int i = 0; i < 4; i++) {
                    // rounding constant folded into the first multiply-add; the result's byte 2 is the output pixel (sum <= 255 * 65536 + 32768)
                    // row sums are <= 65 280 and their pairs <= 130 560: 24-bit multiply-adds (v_mad_u32_u24: tap and accumulation in one instruction)
                    uint32_t acc = mad_u24(kT3, (uint32_t)ring[(j + 4) % 7][i], 32768u);
                    acc = mad_u24(kT2, (uint32_t)(ring[(j + 3) % 7][i] + ring[(j + 5) % 7][i]), acc);
                    acc = mad_u24(34u, (uint32_t)(ring[(j + 2) % 7][i] + ring[(j + 6) % 7][i]), acc);
                    acc = mad_u24(18u, (uint32_t)(ring[(j + 1) % 7][i] + ring[j][i]), acc);
                    if (VARIANT) acc = min(acc, 0x00FFFFFFu);            // taps sum to 257: saturate_cast<uchar>
                    o[i] = acc;
                }
                // byte 2 of the four sums -> one dword (v_perm_b32: selectors 0-3 take from the second operand, 4-7 from the first, 0x0c = zero);
                // the blurred arena's rows are padded to 64 B, so a whole dword always fits in the row
                const uint32_t p01 = __builtin_amdgcn_perm(o[1], o[0], 0x0c0c0602u), p23 = __builtin_amdgcn_perm(o[3], o[2], 0x06020c0cu);
                *reinterpret_cast<uint32_t *>(orow) = p01 | p23;         // orow = out + y * pitch + xa
            }
        }
    };
    for (int r0 = y0 - 3; r0 < rEnd; r0 += 7) {
#pragma unroll
        for (int j = 0; j < 7; j++) Cm[j] = Cn[j], Hm[j] = Hn[j];
        if (r0 + 7 < rEnd) {
#pragma unroll
            for (int j = 0; j < 7; j++) fetch(r0 + 7 + j, Cn[j], Hn[j]);
        }
        walk7(Cm, Hm, r0);
    }
}
template <int VARIANT, int kBlurRows>
__global__ __launch_bounds__(256) void k_blur(const DevParams *__restrict__ P, ImgSrc src, BlurGrid G) {
    blur_body<VARIANT, kBlurRows, false>(P, src, G, blockIdx.x, gridDim.x);
}
template <int VARIANT>
__global__ __launch_bounds__(256) void k_blur_packed(const DevParams *__restrict__ P, ImgSrc src, BlurPack G) {
    blur_body<VARIANT, kBlurRowsBatch, true>(P, src, G, blockIdx.x, gridDim.x);
}
// A few frames (the Tracking thread's call): FAST and the blur in ONE launch, the first gxFast workgroup columns FAST cells, the rest blur strips.
// Both only read the pyramid; as two launches the blur goes to a side stream, and the event that forks it stalls the main queue for ~20 us on
// this runtime (and the join for ~5): more than the blur takes.
template <int TPC, int VARIANT>
__global__ __launch_bounds__(256) void k_fast_blur(const DevParams *__restrict__ P, ImgSrc src, FastLds F, uint32_t *__restrict__ cellBuf,
                                                   int32_t *__restrict__ cellCnt, BlurGrid G, unsigned gxFast) {
    if (blockIdx.x < gxFast) fast_cells_body<TPC>(P, src, F, cellBuf, cellCnt, blockIdx.x, gxFast);
    else blur_body<VARIANT, kBlurRowsSmall, false>(P, src, G, blockIdx.x - gxFast, gridDim.x - gxFast);
}
// ---- launch wrappers (called from orb_schedule.inc) ----
// strip width of a level's waves: 256 pixels unless that would put the row's partial dword into lane 0 or 1 of a wave (its mirrored bytes
// then lie in the previous wave) or make a wave's lane 63 need a halo dword that reaches beyond the row edge; narrower waves leave their
// last lanes as pure halo providers
static int blur_strip_width(int w) {
    for (int bw : {256, 240, 224, 208}) {
        const int r = w % bw;
        const bool partialInFirstLanes = r >= 1 && r <= 8;
        const bool lane63Halo = bw == 256 && (r >= 253 || r <= 3);
        if (!partialInFirstLanes && !lane63Halo) return bw;
    }
    return 192;
}
static BlurGrid blur_grid_of(const DevParams &hP, int rows, int *total) {
    BlurGrid G{};
    int run = 0;
    for (int l = 0; l < hP.nlevels; l++) {
        G.bw[l] = blur_strip_width(hP.lv[l].w);
        G.gx[l] = (hP.lv[l].w + G.bw[l] - 1) / G.bw[l];
        G.base[l] = run;
        run += G.gx[l] * ((hP.lv[l].h + 4 * rows - 1) / (4 * rows));
    }
    G.base[hP.nlevels] = run;
    *total = run;
    return G;
}
bool fast_blur_fusable(const DevParams &hP) { return fast_lds_of(hP).tp == 48; }
// FAST + blur of a few frames as one launch (k_fast_blur); false: this geometry has no fused instantiation, launch them separately
bool launch_fast_blur(const DevParams *dP, const DevParams &hP, ImgSrc src, uint32_t *cellBuf, int32_t *cellCnt, int nframes, int variant, hipStream_t st) {
    const FastLds F = fast_lds_of(hP);
    if (F.tp != 48) return false;                                  // (640 x 480 and its neighbours; other pitches keep the two launches)
    int run = 0;
    const BlurGrid G = blur_grid_of(hP, kBlurRowsSmall, &run);
    const int wpg = 4;
    const unsigned gxFast = (unsigned)((hP.totalCells + wpg - 1) / wpg);
    const dim3 grid(gxFast + (unsigned)run, nframes);
    const size_t lds = (size_t)wpg * F.perWave;
    if (variant) hipLaunchKernelGGL((k_fast_blur<48, 1>), grid, dim3(256), lds, st, dP, src, F, cellBuf, cellCnt, G, gxFast);
    else hipLaunchKernelGGL((k_fast_blur<48, 0>), grid, dim3(256), lds, st, dP, src, F, cellBuf, cellCnt, G, gxFast);
    return true;
}
// the packed grid of a batch (k_blur_packed); the same G for every level would tie the levels' group counts together for no gain
static BlurPack blur_pack_grid(const DevParams &hP, int nframes, long long span, int *total) {
    BlurPack G{};
    int run = 0;
    for (int l = 0; l < hP.nlevels; l++) {
        const LanePack K = blur_pack_of(hP.lv[l].w, nframes, span);
        G.gx[l] = K.waves; G.gy[l] = (hP.lv[l].h + 4 * kBlurRowsBatch - 1) / (4 * kBlurRowsBatch); G.G[l] = K.G; G.M[l] = K.M;
        G.base[l] = run;
        run += G.gx[l] * G.gy[l] * ((nframes + K.G - 1) / K.G);
    }
    G.base[hP.nlevels] = run;
    G.nframes = nframes;
    *total = run;
    return G;
}
void launch_blur(const DevParams *dP, const DevParams &hP, ImgSrc src, int nframes, int variant, hipStream_t st) {
    if (nframes >= kPackMinFrames) {
        int run = 0;
        const BlurPack G = blur_pack_grid(hP, nframes, pack_span(hP, src, true), &run);
        if (variant) hipLaunchKernelGGL((k_blur_packed<1>), dim3(run), dim3(256), 0, st, dP, src, G);
        else hipLaunchKernelGGL((k_blur_packed<0>), dim3(run), dim3(256), 0, st, dP, src, G);
        return;
    }
    int run = 0;
    const BlurGrid G = blur_grid_of(hP, kBlurRowsSmall, &run);
    if (variant) hipLaunchKernelGGL((k_blur<1, kBlurRowsSmall>), dim3(run, nframes), dim3(256), 0, st, dP, src, G);
    else hipLaunchKernelGGL((k_blur<0, kBlurRowsSmall>), dim3(run, nframes), dim3(256), 0, st, dP, src, G);
}

}  // namespace rumi
