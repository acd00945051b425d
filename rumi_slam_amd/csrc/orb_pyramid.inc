// The image pyramid: k_resize (a launch per level), k_pyramid_tiles (all levels of a few frames in one launch) and their launch wrappers.
namespace rumi {

// ------------------------------------------------------------------------------------------------
// Pyramid: level l from level l-1 (cv::resize INTER_LINEAR 8U; taps from host tables that follow cv's coefficient rule, orb_geom.h),
// level 1 straight from the caller's frame.  A lane produces 4 horizontally adjacent pixels of kResizeRows consecutive rows and stores
// one dword per row: the column tables are loaded once and the 2 x kResizeRows source-row loads are issued back to back.
// No border pixels are written: the blur mirrors at the edges itself.
// Frames: blockIdx.z counts GROUPS of K.G consecutive frames whose rows lie side by side along x (LanePack, orb_geom.h); the row state below
// is the same for every frame, so it stays scalar, and the lane's frame only enters its 32-bit address offsets (the host checks the span).
// ------------------------------------------------------------------------------------------------
// (kResizeRows: 4 for the small levels, 8 for levels of 200 rows and more -- launch_resize)
template <int kResizeRows>
__global__ __launch_bounds__(256) void k_resize(const DevParams *__restrict__ P, ImgSrc src,
                                                const int16_t *__restrict__ coef, const RowTap *__restrict__ rowTab, int level, int32_t *__restrict__ clearWord,
                                                LanePack K, int nframes) {
    if (clearWord && (blockIdx.x | blockIdx.y | blockIdx.z | threadIdx.x) == 0) *clearWord = 0;    // the call's error word (orb_schedule.inc)
    const DevLevel &D = P->lv[level];
    const DevLevel &S = P->lv[level - 1];
    const unsigned wg = xcd_swizzle((blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x, gridDim.x * gridDim.y * gridDim.z);
    const int bx = wg % gridDim.x, by = (wg / gridDim.x) % gridDim.y, group = wg / (gridDim.x * gridDim.y), frame0 = group * K.G;
    const LaneSlot slot = lane_slot(K, bx, threadIdx.x & 63);
    const int ox = slot.col * 4;
    // (the wave index as a scalar: the row table entries, the source-row pointers and the vertical taps then live in scalar registers)
    const int oyBase = (by * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6)) * kResizeRows;
    if (lane_frame(K, slot, group, nframes) < 0 || oyBase >= D.h) return;
    int sp;
    const uint8_t *sb = level_base(src, P, level - 1, frame0, &sp);
    const uint32_t fo = (uint32_t)slot.frame * (uint32_t)(level == 1 ? src.l0FrameStride : P->arenaStride);      // my frame's source, from the group's first
    uint8_t *dbase = src.pyr + (long long)frame0 * P->arenaStride + D.off + ((uint32_t)slot.frame * (uint32_t)P->arenaStride + (uint32_t)ox);
    const int16_t *xofs = coef + D.coefX, *xa = coef + D.coefXT;
    // per output row: the two source rows and the vertical taps come ready from a host-built table (the clamps are the same for every
    // lane of every frame)
    const uint8_t *r0p[kResizeRows], *r1p[kResizeRows];
    uint32_t bh0[kResizeRows], bh1[kResizeRows];
    bool live[kResizeRows], shared[kResizeRows];                  // shared: the row's first source row is the previous output row's second (scalar)
#pragma unroll
    for (int r = 0; r < kResizeRows; r++) {
        const int oy = oyBase + r;
        live[r] = oy < D.h;
        const RowTap t = rowTab[D.rowTab + (live[r] ? oy : 0)];
        r0p[r] = sb + (long long)t.r0 * sp; r1p[r] = sb + (long long)t.r1 * sp;
        bh0[r] = t.bh0; bh1[r] = t.bh1;
        shared[r] = kResizeRows == 4 && r > 0 && r0p[r] == r1p[r - 1];       // (eight rows a lane: the branches cost 47 registers and the gain, measured)
    }
    const int sx0 = xofs[ox];
    // (the row's last dword may be partial: its surplus outputs come from the padded table entries and land in the row's padding)
    if (ox + 3 < D.xmaxFast && xofs[ox + 3] + 1 - sx0 <= 7) {
        // the 4 outputs read source bytes sx0 .. sx0+7 of two rows -> two (unaligned) 8-byte loads per row; offsets and taps
        // come as one 8-byte and one 16-byte table load.  The window never leaves the source row (the last lanes slide it left).
        const int wx0 = min(sx0, S.w - 8);
        const uint32_t wo = fo + (uint32_t)wx0;
        const uint64_t ofs = reinterpret_cast<const U64 *>(xofs + ox)->v;
        const U64 *t8 = reinterpret_cast<const U64 *>(xa + 2 * ox);
        const uint64_t ta = t8[0].v, tb = t8[1].v;
        // (at the usual scale factors five output rows in six start on the source row the row above ended on: that row is neither loaded
        // nor filtered horizontally again -- the test is scalar, the branch is a real one)
        uint64_t s0[kResizeRows], s1[kResizeRows];
#pragma unroll
        for (int r = 0; r < kResizeRows; r++) {
            s0[r] = 0;
            if (!shared[r]) s0[r] = reinterpret_cast<const U64 *>(r0p[r] + wo)->v;
            s1[r] = reinterpret_cast<const U64 *>(r1p[r] + wo)->v;
        }
        // horizontal pass as a 2-element dot product: the two source bytes of an output are adjacent, v_perm_b32 spreads them into
        // 16-bit halves and v_dot2_u32_u16 multiplies by the (non-negative, <= 2048) tap pair as it lies in the table
        typedef unsigned short v2u16 __attribute__((ext_vector_type(2)));
        // output i reads the source bytes k_i, k_i + 1 of the 8-byte window: ONE v_perm_b32 over the window's two dwords puts them into the
        // 16-bit halves [b0, 0, b1, 0] (selector built once per column, used for 2 source rows x kResizeRows outputs)
        uint32_t sel[4], tap[4];
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const uint32_t k = (uint32_t)((int)(int16_t)(ofs >> (16 * i)) - wx0);          // 0 .. 6
            sel[i] = k | 0x0c000c00u | ((k + 1u) << 16);
            const uint64_t tt = i < 2 ? ta : tb;
            tap[i] = (uint32_t)(tt >> (32 * (i & 1)));
        }
        uint32_t hPrev[4] = {0, 0, 0, 0};                              // horizontal results (>> 4) of the previous output row's second source row
#pragma unroll
        for (int r = 0; r < kResizeRows; r++) {
            // vertical taps come pre-shifted: (b * x) >> 16 == mulhi(b << 16, x) for the non-negative operands here (b <= 2048, x <= 32 640)
            uint32_t h0[4], h1[4];
            if (shared[r]) {
#pragma unroll
                for (int i = 0; i < 4; i++) h0[i] = hPrev[i];
            } else {
#pragma unroll
                for (int i = 0; i < 4; i++) {
                    const uint32_t p0 = __builtin_amdgcn_perm((uint32_t)(s0[r] >> 32), (uint32_t)s0[r], sel[i]);
                    h0[i] = __builtin_amdgcn_udot2(__builtin_bit_cast(v2u16, p0), __builtin_bit_cast(v2u16, tap[i]), 0u, false) >> 4;
                }
            }
            uint32_t packed = 0;
#pragma unroll
            for (int i = 0; i < 4; i++) {
                const uint32_t p1 = __builtin_amdgcn_perm((uint32_t)(s1[r] >> 32), (uint32_t)s1[r], sel[i]);
                h1[i] = __builtin_amdgcn_udot2(__builtin_bit_cast(v2u16, p1), __builtin_bit_cast(v2u16, tap[i]), 0u, false) >> 4;
                packed |= ((__umulhi(bh0[r], h0[i]) + __umulhi(bh1[r], h1[i]) + 2u) >> 2) << (8 * i);
                hPrev[i] = h1[i];
            }
            if (live[r]) *reinterpret_cast<uint32_t *>(dbase + (long long)(oyBase + r) * D.pitch) = packed;
        }
    } else {
        for (int r = 0; r < kResizeRows; r++) {
            if (!live[r]) continue;
            uint32_t packed = 0;
            for (int i = 0; i < 4 && ox + i < D.w; i++) {
                const int dx = ox + i;
                const uint32_t sx = fo + (uint32_t)xofs[dx];
                int q0, q1;
                if (dx < D.xmax) {
                    const int a0 = xa[dx * 2], a1 = xa[dx * 2 + 1];
                    q0 = r0p[r][sx] * a0 + r0p[r][sx + 1] * a1;
                    q1 = r1p[r][sx] * a0 + r1p[r][sx + 1] * a1;
                } else {
                    q0 = r0p[r][sx] * 2048;
                    q1 = r1p[r][sx] * 2048;
                }
                packed |= (uint32_t)(((((int)(bh0[r] >> 16) * (q0 >> 4)) >> 16) + (((int)(bh1[r] >> 16) * (q1 >> 4)) >> 16) + 2) >> 2) << (8 * i);
            }
            *reinterpret_cast<uint32_t *>(dbase + (long long)(oyBase + r) * D.pitch) = packed;
        }
    }
}

// ------------------------------------------------------------------------------------------------
// The pyramid of a call of a few frames in ONE launch.  Seven dependent launches of ~4.4 us are most of such a call's pyramid time, and each
// level is read back from HBM by the next.  Here a workgroup owns a tile of the top level and computes, level by level in LDS, the region of
// every level that tile descends from (plus its share of a partition of the level, so that every pixel of every level is produced): level l - 1's
// region is the source of level l's, the regions (PyrTile, from the host's resize tables) overlap by the taps' reach, and every workgroup
// stores all it computed -- overlapping stores carry the same bytes.  The arithmetic per pixel is k_resize's general path, tap for tap.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_pyramid_tiles(const DevParams *__restrict__ P, ImgSrc src, const int16_t *__restrict__ coef,
                                                       const RowTap *__restrict__ rowTab, const PyrTile *__restrict__ tiles, int bufBytes,
                                                       int32_t *__restrict__ clearWord) {
    // LDS: two image buffers of bufBytes (a level's region and the one computed from it), then the tile's slices of the resize tables
    // (per level and row: source rows relative to the buffer | vertical taps; per level and column: source column relative to the buffer, tap pair)
    extern __shared__ __attribute__((aligned(16))) uint8_t pyrLds[];
    if (clearWord && (blockIdx.x | blockIdx.y | threadIdx.x) == 0) *clearWord = 0;    // the call's error word (orb_schedule.inc)
    const int frame = blockIdx.y, tid = threadIdx.x, nlevels = P->nlevels;
    uint8_t *A = pyrLds, *B = pyrLds + bufBytes;
    uint2 *tab = reinterpret_cast<uint2 *>(pyrLds + 2 * bufBytes);
    // ---- the per-level parameters first, one lane per level, into LDS: read where they are needed they are a chain of scalar loads from
    // global memory, two or three per level, ~1 us each
    struct Lv { int x0, x1, y0, y1, coefX, coefXT, xmax, rowTab, pitch, pad; long long off; };
    __shared__ Lv sLv[kMaxLevels];
    if (tid < nlevels) {
        const PyrTile &T = tiles[blockIdx.x];
        const DevLevel &D = P->lv[tid];
        sLv[tid] = Lv{T.x0[tid], T.x1[tid], T.y0[tid], T.y1[tid], D.coefX, D.coefXT, D.xmax, D.rowTab, D.pitch, 0, D.off};
    }
    __syncthreads();
    // ---- everything else this workgroup reads from global memory: the table slices of all levels (one row entry and one column entry per
    // thread and level) and the window of level 0 (dwords: 64 columns x 4 rows per pass).  ALL loads are issued before the first value is
    // stored to LDS: as loops of load-then-store they were some fifty dependent round trips, 28 of the kernel's 34 us.
    // (the host offers this kernel for up to kPyrLevels levels, regions of up to 256 rows / columns and windows of up to 80 rows x 256 columns)
    int apitch;
    {
        RowTap rt[kPyrLevels];
        int cofs[kPyrLevels];
        uint32_t ctap[kPyrLevels];
#pragma unroll
        for (int level = 1; level < kPyrLevels; level++) {
            rt[level] = RowTap{0, 0, 0u, 0u}; cofs[level] = 0; ctap[level] = 0;
            if (level < nlevels) {
                const Lv D = sLv[level];
                if (tid < D.y1 - D.y0) rt[level] = rowTab[D.rowTab + D.y0 + tid];
                if (tid < D.x1 - D.x0) {
                    const int dx = D.x0 + tid;
                    cofs[level] = (coef + D.coefX)[dx];
                    // the tap pair as one dword (a0 in the low half); a single-tap column multiplies its one source byte by 2048
                    ctap[level] = dx < D.xmax ? reinterpret_cast<const U32 *>(coef + D.coefXT + dx * 2)->v : 2048u;
                }
            }
        }
        int sp;
        const uint8_t *sb = level_base(src, P, 0, frame, &sp);
        const int ax0 = sLv[0].x0, ay0 = sLv[0].y0, aw = sLv[0].x1 - ax0, ah = sLv[0].y1 - ay0, W0 = P->lv[0].w;
        apitch = (aw + 3) & ~3;
        uint32_t win[kPyrWinPasses];
        const int wx = (tid & 63) * 4, wy = tid >> 6;
#pragma unroll
        for (int k = 0; k < kPyrWinPasses; k++) {
            const int y = wy + 4 * k;
            win[k] = 0;
            if (y < ah && wx < aw) {
                const uint8_t *p = sb + (long long)(ay0 + y) * sp + ax0 + wx;
                if (ax0 + wx + 4 <= W0) win[k] = reinterpret_cast<const U32 *>(p)->v;
                else for (int i = 0; ax0 + wx + i < W0; i++) win[k] |= (uint32_t)p[i] << (8 * i);      // the frame's last columns: no read past the row
            }
        }
        // ---- now the stores
        int tb = 0;
#pragma unroll
        for (int level = 1; level < kPyrLevels; level++) {
            if (level < nlevels) {
                const Lv D = sLv[level];
                const int cols = D.x1 - D.x0, rows = D.y1 - D.y0, sx0 = sLv[level - 1].x0, sy0 = sLv[level - 1].y0;
                if (tid < rows) tab[tb + tid] = make_uint2((uint32_t)(rt[level].r0 - sy0) | ((uint32_t)(rt[level].r1 - sy0) << 16), (rt[level].bh0 >> 16) | (rt[level].bh1 & 0xFFFF0000u));
                if (tid < cols) tab[tb + rows + tid] = make_uint2((uint32_t)(cofs[level] - sx0), ctap[level]);
                tb += rows + cols;
            }
        }
#pragma unroll
        for (int k = 0; k < kPyrWinPasses; k++) {
            const int y = wy + 4 * k;
            if (y < ah && wx < aw) *reinterpret_cast<uint32_t *>(A + y * apitch + wx) = win[k];
        }
    }
    __syncthreads();
    int base = 0;
    for (int level = 1; level < nlevels; level++) {
        const Lv D = sLv[level];
        const int X0 = D.x0, Y0 = D.y0, bw = D.x1 - X0, rows = D.y1 - Y0, gpr = bw >> 2;
        const uint2 *rowT = tab + base, *colT = rowT + rows;
        base += rows + bw;
        uint8_t *dbase = src.pyr + (long long)frame * P->arenaStride + D.off + (long long)Y0 * D.pitch + X0;
        // threads per row of 4-pixel groups: the power of two that holds them (the top levels have eight groups a row)
        const int tprLog = gpr <= 8 ? 3 : gpr <= 16 ? 4 : gpr <= 32 ? 5 : 6, tpr = 1 << tprLog, rstep = 256 >> tprLog;
        for (int gx = tid & (tpr - 1); gx < gpr; gx += tpr) {
            uint32_t sx[4], tap[4], sel[4];
#pragma unroll
            for (int i = 0; i < 4; i++) { const uint2 c = colT[4 * gx + i]; sx[i] = c.x; tap[i] = c.y; }
            // k_resize's dword form on the LDS tile: the 4 outputs read source bytes sx[0] .. sx[0] + 7 of two rows (one 8-byte read each), v_perm_b32
            // spreads an output's two bytes into 16-bit halves, v_dot2_u32_u16 multiplies by the tap pair; wider spans take the byte form
            const bool span8 = sx[3] + 1u - sx[0] <= 7u;
#pragma unroll
            for (int i = 0; i < 4; i++) { const uint32_t k = sx[i] - sx[0]; sel[i] = k | 0x0c000c00u | ((k + 1u) << 16); }
            typedef unsigned short v2u16 __attribute__((ext_vector_type(2)));
            for (int gy = tid >> tprLog; gy < rows; gy += rstep) {
                const uint2 t = rowT[gy];
                const uint8_t *r0 = A + (t.x & 0xFFFFu) * apitch, *r1 = A + (t.x >> 16) * apitch;
                const uint32_t bh0 = t.y << 16, bh1 = t.y & 0xFFFF0000u;       // vertical taps << 16: (b * x) >> 16 == mulhi(b << 16, x)
                uint32_t packed = 0;
                if (span8) {
                    const uint64_t s0 = reinterpret_cast<const U64 *>(r0 + sx[0])->v, s1 = reinterpret_cast<const U64 *>(r1 + sx[0])->v;
#pragma unroll
                    for (int i = 0; i < 4; i++) {
                        const uint32_t p0 = __builtin_amdgcn_perm((uint32_t)(s0 >> 32), (uint32_t)s0, sel[i]);
                        const uint32_t p1 = __builtin_amdgcn_perm((uint32_t)(s1 >> 32), (uint32_t)s1, sel[i]);
                        const uint32_t q0 = __builtin_amdgcn_udot2(__builtin_bit_cast(v2u16, p0), __builtin_bit_cast(v2u16, tap[i]), 0u, false);
                        const uint32_t q1 = __builtin_amdgcn_udot2(__builtin_bit_cast(v2u16, p1), __builtin_bit_cast(v2u16, tap[i]), 0u, false);
                        packed |= ((__umulhi(bh0, q0 >> 4) + __umulhi(bh1, q1 >> 4) + 2u) >> 2) << (8 * i);
                    }
                } else {
#pragma unroll
                    for (int i = 0; i < 4; i++) {
                        const uint32_t a0 = tap[i] & 0xFFFFu, a1 = tap[i] >> 16;
                        const uint32_t q0 = r0[sx[i]] * a0 + (a1 ? r0[sx[i] + 1] * a1 : 0u), q1 = r1[sx[i]] * a0 + (a1 ? r1[sx[i] + 1] * a1 : 0u);
                        packed |= ((__umulhi(bh0, q0 >> 4) + __umulhi(bh1, q1 >> 4) + 2u) >> 2) << (8 * i);
                    }
                }
                *reinterpret_cast<uint32_t *>(B + gy * bw + 4 * gx) = packed;
                *reinterpret_cast<uint32_t *>(dbase + (long long)gy * D.pitch + 4 * gx) = packed;
            }
        }
        __syncthreads();
        uint8_t *t2 = A; A = B; B = t2;
        apitch = bw;
    }
}
// ---- launch wrappers (called from orb_schedule.inc) ----
void launch_resize(const DevParams *dP, const DevParams &hP, ImgSrc src, const int16_t *coef, const RowTap *rowTab, int level, int nframes,
                   hipStream_t st, int32_t *clearWord) {
    const int rows = hP.lv[level].h >= 200 ? 8 : 4;
    const LanePack K = resize_pack_of(hP.lv[level].w, nframes, pack_span(hP, src, level == 1));
    dim3 g(K.waves, (hP.lv[level].h + 4 * rows - 1) / (4 * rows), (nframes + K.G - 1) / K.G);
    if (rows == 8) hipLaunchKernelGGL(k_resize<8>, g, dim3(256), 0, st, dP, src, coef, rowTab, level, clearWord, K, nframes);
    else hipLaunchKernelGGL(k_resize<4>, g, dim3(256), 0, st, dP, src, coef, rowTab, level, clearWord, K, nframes);
}
void launch_pyramid_tiles(const DevParams *dP, ImgSrc src, const int16_t *coef, const RowTap *rowTab, const PyrTile *tiles, int ntiles, int bufBytes,
                          int tabEntries, int nframes, hipStream_t st, int32_t *clearWord) {
    hipLaunchKernelGGL(k_pyramid_tiles, dim3(ntiles, nframes), dim3(256), (size_t)2 * bufBytes + (size_t)tabEntries * 8, st, dP, src, coef, rowTab, tiles, bufBytes, clearWord);
}

}  // namespace rumi
