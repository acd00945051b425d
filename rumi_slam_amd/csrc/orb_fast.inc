// FAST per cell and the candidate compaction: k_fast_cells (fast_cells_body, which k_fast_blur of orb_blur.inc runs too), k_compact and their
// launch wrappers.
namespace rumi {

// ------------------------------------------------------------------------------------------------
// FAST 9/16 + per-cell NMS + threshold fallback, one wave per (frame, cell).
//
// score(p) = max over the 16 arcs of 9 of min |v - I_k| on the bright or dark side, minus 1  (cv's
// cornerScore with the start threshold folded out); p is a corner at T  <=>  score(p) >= T, so ONE
// score tile serves both thresholds.  NMS neighbours outside the cell's detection region count as 0,
// exactly as cv::FAST's zero-initialised score rows make them (SURVEY.md B.1).
// The sub-image is staged in LDS; scores never touch HBM.  A cheap necessary test on every pixel selects the (pixel, polarity)
// pairs that get the exact score (fast_quick_pair / fast_score_polar).
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ int min3i(int a, int b, int c) { return min(min(a, b), c); }
__device__ __forceinline__ int max3i(int a, int b, int c) { return max(max(a, b), c); }

// One WAVE per (frame, cell), four cells per 256-thread workgroup, no workgroup barrier anywhere: the wave stages its
// sub-image as dwords, tests 256 pixels per step, and emits in index order with a running offset.  LDS per wave is
// sized by the host from the largest cell of the current geometry (FastLds), so occupancy is not limited by LDS.
struct FastLds { int tp, sp, tileBytes, scBytes, maxIters, perWave; };

__device__ __forceinline__ void wave_lds_fence() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// ---- quick test and exact score ---------------------------------------------------------------------------------------------------
// Instruction classes on gfx950 (tools/valu_rate.hip, profiles/r02_valu_issue_rates.txt): plain add / sub / and / or / xor / right shift /
// mov issue in ~2.4 cycles per wave once two waves share a SIMD; every min / max, three-operand, packed, SDWA and DPP form takes ~4.2.
//
// Tile.  Column c of the LDS tile is image column iniX - 1 + c: the detection region (cv::FAST's 3-px margin inside the sub-image)
// ALWAYS starts at tile column 4, i.e. on a dword, whatever iniX is (the staging loads are unaligned 4-byte global loads).  A row of the
// region then is made of aligned 4-pixel groups with no partial first group (round 2 staged aligned dwords and lost up to one
// group per row to the shift).
//
// Quick test (necessary condition, per polarity): every arc of 9 contains 4 consecutive of the 8 EVEN circle positions, so a pixel can
// reach contrast T on the darker-ring side only if 4 consecutive even positions all have v - p_k >= T (brighter ring: p_k - v >= T).
// Ring entries = tile offset of the pixel | polarity << 15; a pixel's darker entry always precedes its brighter one.
constexpr int kRingCap = 640;        // linear: < 128 entries wait between steps, a step appends up to 1024 (64 lanes x 8 pixels x 2 polarities)
                                     // in two halves when they do not fit
constexpr int kScoredCap = 640;
// (ring pixels q in [0, 255] travel as 0x4100 + q: positive normal f16 bit patterns of one exponent, ordered like the integers)

__device__ __forceinline__ uint32_t pk_min3_f16(uint32_t a, uint32_t b, uint32_t c) {
    uint32_t r;
    asm("v_pk_minimum3_f16 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
}
__device__ __forceinline__ uint32_t pk_max3_f16(uint32_t a, uint32_t b, uint32_t c) {
    uint32_t r;
    asm("v_pk_maximum3_f16 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
}
// inclusive prefix sum over the wave's 64 lanes: four row shifts and two row broadcasts (v_add_u32 with a DPP operand each)
__device__ __forceinline__ int wave_incl_scan(int v) {
    v += __builtin_amdgcn_update_dpp(0, v, 0x111, 0xf, 0xf, false);    // row_shr:1
    v += __builtin_amdgcn_update_dpp(0, v, 0x112, 0xf, 0xf, false);    // row_shr:2
    v += __builtin_amdgcn_update_dpp(0, v, 0x114, 0xf, 0xf, false);    // row_shr:4
    v += __builtin_amdgcn_update_dpp(0, v, 0x118, 0xf, 0xf, false);    // row_shr:8
    v += __builtin_amdgcn_update_dpp(0, v, 0x142, 0xa, 0xf, false);    // row_bcast:15 into rows 1 and 3
    v += __builtin_amdgcn_update_dpp(0, v, 0x143, 0xc, 0xf, false);    // row_bcast:31 into rows 2 and 3
    return v;
}


typedef __attribute__((address_space(3))) const uint8_t lds_cu8;
__device__ __forceinline__ uint32_t lds_addr(const uint8_t *p) { return (uint32_t)(uintptr_t)(lds_cu8 *)p; }

// The 16 circle pixels and the centre of ring entry 0 (7 x 7 neighbourhood with top-left corner t0) in the LOW halves of 17 registers, and
// those of entry 1 (t1) in the HIGH halves of 17 others: ds_read_u8 and ds_read_u8_d16_hi with immediate offsets (compile-time tile
// pitch).  The d16_hi form puts the byte where the packed arithmetic wants it, so that no shift is spent on packing -- but on a part
// with SRAM ECC (gfx950) a d16 load ZEROES the other half of its destination instead of keeping it, so the two entries cannot share a
// register at load time; one three-input bit operation per circle position merges them (and applies the polarity mask, see below).
// Each asm block carries its own s_waitcnt: the compiler does not track the LDS counter of inline asm, so no result may leave a block
// before it has arrived.
template <int CTP>
__device__ __forceinline__ void fast_ring_load(const uint8_t *t0g, const uint8_t *t1, int tp, uint32_t (&lo)[17], uint32_t (&hi)[17]) {
    if constexpr (CTP != 0) {
        lds_cu8 *t0 = (lds_cu8 *)t0g;
        const uint32_t A1 = lds_addr(t1);
#define RUMI_LD(reg, dx, dy) " %" #reg ", %17 offset:%18*(3+(" #dy "))+3+(" #dx ")\n\t"
#define RUMI_LD17(op)                                                                                              \
        op RUMI_LD(0, 0, 3)    op RUMI_LD(1, 1, 3)    op RUMI_LD(2, 2, 2)     op RUMI_LD(3, 3, 1)                      \
        op RUMI_LD(4, 3, 0)    op RUMI_LD(5, 3, -1)   op RUMI_LD(6, 2, -2)    op RUMI_LD(7, 1, -3)                     \
        op RUMI_LD(8, 0, -3)   op RUMI_LD(9, -1, -3)  op RUMI_LD(10, -2, -2)  op RUMI_LD(11, -3, -1)                   \
        op RUMI_LD(12, -3, 0)  op RUMI_LD(13, -3, 1)  op RUMI_LD(14, -2, 2)   op RUMI_LD(15, -1, 3)                    \
        op RUMI_LD(16, 0, 0)   "s_waitcnt lgkmcnt(0)"
        // entry 0: plain byte loads the compiler issues and tracks itself; they are queued BEFORE the asm block below (a volatile asm with a
        // memory clobber is not crossed), whose single s_waitcnt lgkmcnt(0) therefore covers all 34 loads in one LDS round trip
        asm("" : "+v"(t0));            // the base as one opaque register: all 17 offsets then are non-negative immediates of the load instruction
#define RUMI_LO(k, dx, dy) lo[k] = t0[(3 + (dy)) * CTP + 3 + (dx)];
        RUMI_LO(0, 0, 3)    RUMI_LO(1, 1, 3)    RUMI_LO(2, 2, 2)     RUMI_LO(3, 3, 1)
        RUMI_LO(4, 3, 0)    RUMI_LO(5, 3, -1)   RUMI_LO(6, 2, -2)    RUMI_LO(7, 1, -3)
        RUMI_LO(8, 0, -3)   RUMI_LO(9, -1, -3)  RUMI_LO(10, -2, -2)  RUMI_LO(11, -3, -1)
        RUMI_LO(12, -3, 0)  RUMI_LO(13, -3, 1)  RUMI_LO(14, -2, 2)   RUMI_LO(15, -1, 3)
        RUMI_LO(16, 0, 0)
#undef RUMI_LO
        asm volatile(RUMI_LD17("ds_read_u8_d16_hi")
                     : "=&v"(hi[0]), "=&v"(hi[1]), "=&v"(hi[2]), "=&v"(hi[3]), "=&v"(hi[4]), "=&v"(hi[5]), "=&v"(hi[6]), "=&v"(hi[7]), "=&v"(hi[8]),
                       "=&v"(hi[9]), "=&v"(hi[10]), "=&v"(hi[11]), "=&v"(hi[12]), "=&v"(hi[13]), "=&v"(hi[14]), "=&v"(hi[15]), "=&v"(hi[16])
                     : "v"(A1), "n"(CTP)
                     : "memory");
#undef RUMI_LD17
#undef RUMI_LD
    } else {
#define RUMI_RING(k, dx, dy) lo[k] = t0g[(3 + (dy)) * tp + 3 + (dx)]; hi[k] = (uint32_t)t1[(3 + (dy)) * tp + 3 + (dx)] << 16;
        RUMI_RING(0, 0, 3)    RUMI_RING(1, 1, 3)    RUMI_RING(2, 2, 2)     RUMI_RING(3, 3, 1)
        RUMI_RING(4, 3, 0)    RUMI_RING(5, 3, -1)   RUMI_RING(6, 2, -2)    RUMI_RING(7, 1, -3)
        RUMI_RING(8, 0, -3)   RUMI_RING(9, -1, -3)  RUMI_RING(10, -2, -2)  RUMI_RING(11, -3, -1)
        RUMI_RING(12, -3, 0)  RUMI_RING(13, -3, 1)  RUMI_RING(14, -2, 2)   RUMI_RING(15, -1, 3)
        RUMI_RING(16, 0, 0)
#undef RUMI_RING
    }
}

// exact scores of up to 128 ring entries, two per lane (entries `lane` and `lane + 64` of the batch: one LDS instruction then serves 64
// CONSECUTIVE entries, which lie within a few tile rows).
// A darker-ring entry is scored on COMPLEMENTED pixels (255 - p, 255 - v): its contrasts v - p_k are then the brighter-ring contrasts
// q_k - vq of the complemented data, so one network serves both polarities and the two entries of a lane may differ in polarity.  Per
// entry, with q_k = p_k ^ x (x = 0xFF darker, 0 brighter) and vq = v ^ x:  score = max over the 16 arcs of 9 of min q_k  -  vq  -  1.
// The XOR also sets the f16 exponent (0x4100) and rides on the instruction that merges the two entries' bytes; then 16 + 16 packed
// three-input minima and 8 maxima for both entries.
// A pixel cannot reach a positive score in both polarities (two arcs of 9 on a circle of 16 share two positions), so a hit stores its
// score byte unconditionally and is appended to the cell's SCORED LIST sl (tile offsets, ascending because the ring is filled in pixel
// order): NMS and emission then walk a few hundred listed pixels instead of the whole score map.  nScored counts all appends; once it
// passes kScoredCap the list is abandoned and the caller scans the map.
template <int CTP>
__device__ __forceinline__ void fast_score_batch(const uint8_t *tile, uint8_t *sc, uint16_t *sl, int &nScored, const uint16_t *ring, int n, int tp, int scDelta,
                                                 int tlow, int lane) {
    const int TP = CTP ? CTP : tp;
    const bool act0 = lane < n, act1 = lane + 64 < n;
    const uint32_t e0 = ring[lane], e1 = ring[lane + 64];
    const int a0 = act0 ? (int)(e0 & 0x7FFFu) : 3 * TP + 4, a1 = act1 ? (int)(e1 & 0x7FFFu) : 3 * TP + 4;
    // per half: 0x41FF for a darker-ring entry, 0x4100 for a brighter-ring one
    const uint32_t X = 0x41FF41FFu - ((e0 >> 15) | ((e1 >> 15) << 16)) * 0xFFu;
    uint32_t lo[17], hi[17], q[16];
    fast_ring_load<CTP>(tile + a0 - 3 * TP - 3, tile + a1 - 3 * TP - 3, TP, lo, hi);     // top-left corners of the 7 x 7 neighbourhoods: every offset is >= 0
#pragma unroll
    for (int k = 0; k < 16; k++) q[k] = (lo[k] | hi[k]) ^ X;                              // one v_bitop3_b32 each
    const uint32_t vc = lo[16] | hi[16];
    uint32_t lo3[16];
#pragma unroll
    for (int k = 0; k < 16; k++) lo3[k] = pk_min3_f16(q[k], q[(k + 1) & 15], q[(k + 2) & 15]);
    uint32_t arc[16];
#pragma unroll
    for (int k = 0; k < 16; k++) arc[k] = pk_min3_f16(lo3[k], lo3[(k + 3) & 15], lo3[(k + 6) & 15]);
    uint32_t A = pk_max3_f16(arc[0], arc[1], arc[2]);
#pragma unroll
    for (int k = 3; k < 15; k += 2) A = pk_max3_f16(A, arc[k], arc[k + 1]);
    A = pk_max3_f16(A, arc[15], arc[15]);
    // per half: A = 0x4100 + max-min q, vq' = 0x4100 + vq; hit <=> A - vq' - 1 >= tlow.  D = (A | 0x8000) - (vq' + tlow + 1) stays within
    // 0x7E01 .. 0x80FE per half (no borrow between the halves) and carries the decision in bits 15 / 31; for a hit the low byte of
    // D + tlow is the score.
    const uint32_t D = (A | 0x80008000u) - ((vc ^ X) + (uint32_t)(tlow + 1) * 0x10001u);
    const uint32_t Sb = D + (uint32_t)tlow * 0x10001u;
    const bool hit0 = act0 && (D & 0x8000u) != 0, hit1 = act1 && (int32_t)D < 0;
    if (hit0) sc[a0 + scDelta] = (uint8_t)Sb;
    if (hit1) sc[a1 + scDelta] = (uint8_t)(Sb >> 16);
    const unsigned long long h0 = __ballot(hit0), h1 = __ballot(hit1);
    const int c0 = __popcll(h0), total = nScored + c0 + __popcll(h1);
    if (total <= kScoredCap) {                                       // wave-uniform: once the list has overflowed its content is never read
        const int pos0 = __builtin_amdgcn_mbcnt_hi((uint32_t)(h0 >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)h0, nScored));
        const int pos1 = __builtin_amdgcn_mbcnt_hi((uint32_t)(h1 >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)h1, nScored + c0));   // ring order: entries 0..63, then 64..127
        if (hit0) sl[pos0] = (uint16_t)a0;
        if (hit1) sl[pos1] = (uint16_t)a1;
    }
    nScored = total;
}

// ---- quick test on bytes, eight pixels a lane ---------------------------------------------------------------------------------------
// The necessary condition above (4 consecutive of the 8 even circle positions reach contrast T), computed on the pixel bytes as
// they lie in LDS, four pixels per dword, two adjacent dwords (eight pixels) per lane.
//   Circle dwords: the ring bytes of a 4-pixel group at (0, +-3) are the aligned dword of that row; the others are ONE v_alignbyte_b32 of
//   two loaded dwords, and the two groups of a lane share the middle one of rows +-2 (10 alignbytes for 16 circle dwords).
//   Compares: v_lerp_u8 computes (a + b + r) >> 1 per byte, so bit 7 of lerp(p, ~x, 0) is [p > x] and bit 7 of lerp(p, ~y, 1) is [p >= y]:
//   four compares per instruction.  With x = sat(v + T) and y = sat(v - T) they are cv::FAST's strict tests: brighter = p > x, darker =
//   NOT [p >= y] (saturation is exact: v + T > 255 admits no brighter pixel, v - T < 0 no darker one).  ~x and ~y come once per group
//   from packed saturating 16-bit arithmetic on the centre bytes held in the HIGH byte of each half (the low byte never carries into it).
//   Rule: per dword and polarity the "4 consecutive of 8" network of ten two- / three-input operations on the raw lerp words (only
//   bit 7 of each byte is read); the not-darker words take its De Morgan dual.  Four networks cost less than merging the flag words first
//   (a shift and a bit-field insert per word and position).
//   Ring append: the four bit-7 words become ONE 16-bit mask in ring order (bit 2 i darker, 2 i + 1 brighter, pixel i = 0..7) by a mask
//   and a multiplication per dword; a lane then writes its set bits lowest first.
// Ring contract unchanged: entries in pixel order, darker before brighter within a pixel.
__device__ __forceinline__ uint32_t pk_add_sat_u16(uint32_t a, uint32_t b) {
    typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
    return __builtin_bit_cast(uint32_t, __builtin_elementwise_add_sat(__builtin_bit_cast(u16x2, a), __builtin_bit_cast(u16x2, b)));      // v_pk_add_u16 clamp
}
__device__ __forceinline__ uint32_t pk_sub_sat_u16(uint32_t a, uint32_t b) {
    typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
    return __builtin_bit_cast(uint32_t, __builtin_elementwise_sub_sat(__builtin_bit_cast(u16x2, a), __builtin_bit_cast(u16x2, b)));      // v_pk_sub_u16 clamp
}
// per byte of the centre dword c: nb = ~sat(v + T), nd = ~sat(v - T) = sat(~v + T).  TT = T << 8 in both halves.
__device__ __forceinline__ void fast_bytes_thresholds(uint32_t c, uint32_t TT, uint32_t &nb, uint32_t &nd) {
    const uint32_t n = ~c, ne = n << 8;       // bytes 1, 3 (odd pixels) high in the halves of n, bytes 0, 2 (even pixels) in those of ne
    nb = __builtin_amdgcn_perm(pk_sub_sat_u16(n, TT), pk_sub_sat_u16(ne, TT), 0x07030501u);
    nd = __builtin_amdgcn_perm(pk_add_sat_u16(n, TT), pk_add_sat_u16(ne, TT), 0x07030501u);
}
// 4 consecutive of the 8 words set (circular), every bit on its own: the runs starting at even positions are p0 p2 | p2 p4 | p4 p6 | p6 p0
// = (p0 | p4) & (p2 | p6) with p_k = f_k & f_k+1, the odd ones likewise -- ten operations instead of 16 (compiled to v_bitop3_b32, v_and_b32, v_or_b32 and a few v_and_or_b32)
__device__ __forceinline__ uint32_t four_of_eight(const uint32_t (&f)[8]) {
    const uint32_t te = (f[0] & f[1]) | (f[4] & f[5]), ue = (f[2] & f[3]) | (f[6] & f[7]);
    const uint32_t to = (f[1] & f[2]) | (f[5] & f[6]), uo = (f[3] & f[4]) | (f[7] & f[0]);
    return (te & ue) | (to & uo);
}
// the same rule for the complements: returns ~four_of_eight(~g)
__device__ __forceinline__ uint32_t four_of_eight_dual(const uint32_t (&g)[8]) {
    const uint32_t te = (g[0] | g[1]) & (g[4] | g[5]), ue = (g[2] | g[3]) & (g[6] | g[7]);
    const uint32_t to = (g[1] | g[2]) & (g[5] | g[6]), uo = (g[3] | g[4]) & (g[7] | g[0]);
    return (te | ue) & (to | uo);
}
// ring-order mask of one dword's four pixels in bits 24-31 (bit 24 + 2 q darker, 25 + 2 q brighter for byte q): brighter in bit 7 of
// each byte of y, NOT darker in bit 7 of each byte of z.  The two flags of byte q sit at bits 8 q + 6, 7; the multiplier 2^18 + 2^12 +
// 2^6 + 1 moves them to 24 + 2 q (every other product lands below bit 24 or above bit 31, and no two products overlap: no carries).
__device__ __forceinline__ uint32_t fast_bytes_ringmask(uint32_t y, uint32_t z) {
    const uint32_t f = ((y & 0x80808080u) | (~(z >> 1) & 0x40404040u));
    return f * 0x41041u;
}

template <int CTP>
__device__ __forceinline__ int fast_score_cell_bytes(const uint8_t *tile, uint8_t *sc, uint16_t *cl, uint16_t *sl, int tp, int dw, int dh, int tlow, int lane) {
    const int TP = CTP ? CTP : tp;
    const int ng = (dw + 7) >> 3;                         // 8-pixel items per row; the first starts at tile column 4
    const int nItems = ng * dh;
    const unsigned Mng = magic_of(ng);
    const int scDelta = -2 * TP - 3;
    const uint32_t mLast = 0xFFFFu >> (2 * (8 * ng - dw));   // ring mask of a row's last item: pixels from column dw on lie outside the region
    const uint32_t TT = (uint32_t)tlow * 0x01000100u;
    uint32_t *cl32 = reinterpret_cast<uint32_t *>(cl);
    int pending = 0, nScored = 0;
    // full batches of 128 leave the front of the ring; the entries still waiting move to the front (fewer than 128, from beyond them)
    auto drain = [&]() {
        int head = 0;
        while (pending >= 128) {
            wave_lds_fence();
            fast_score_batch<CTP>(tile, sc, sl, nScored, cl + head, 128, tp, scDelta, tlow, lane);
            head += 128;
            pending -= 128;
        }
        if (head) {
            wave_lds_fence();
            const uint32_t q = cl32[(head >> 1) + lane];
            wave_lds_fence();
            if (2 * lane < pending) cl32[lane] = q;
        }
    };
    for (int base = 0; base < nItems; base += 64) {
        const int ip = base + lane;
        const bool live = ip < nItems;
        const int row = live ? magic_div(ip, Mng) : 0, gi = live ? ip - mul24(row, ng) : 0;
        const int A = mul24(row + 3, TP) + 8 * gi + 4;                        // tile offset of the item's first pixel (a dword)
        const uint8_t *t = tile + A;
#define RUMI_DW(off) (*reinterpret_cast<const uint32_t *>(t + (off)))
        // every read is an aligned dword inside the tile: columns 0 .. 8 ng + 7 of rows row .. row + 6 (a read past the row's last dword
        // lands at the start of the next row, inside the tile; such bytes only reach pixels outside the region, which the mask drops)
        const uint32_t M3a = RUMI_DW(-3 * TP), M3b = RUMI_DW(-3 * TP + 4), P3a = RUMI_DW(3 * TP), P3b = RUMI_DW(3 * TP + 4);
        const uint32_t M2l = RUMI_DW(-2 * TP - 4), M2a = RUMI_DW(-2 * TP), M2b = RUMI_DW(-2 * TP + 4), M2r = RUMI_DW(-2 * TP + 8);
        const uint32_t P2l = RUMI_DW(2 * TP - 4), P2a = RUMI_DW(2 * TP), P2b = RUMI_DW(2 * TP + 4), P2r = RUMI_DW(2 * TP + 8);
        const uint32_t Cl = RUMI_DW(-4), Ca = RUMI_DW(0), Cb = RUMI_DW(4), Cr = RUMI_DW(8);
#undef RUMI_DW
        // rows -2 / +2 at column offsets -2, +2, +6 of the item
        const uint32_t m0 = __builtin_amdgcn_alignbyte(M2a, M2l, 2), m1 = __builtin_amdgcn_alignbyte(M2b, M2a, 2), m2 = __builtin_amdgcn_alignbyte(M2r, M2b, 2);
        const uint32_t p0 = __builtin_amdgcn_alignbyte(P2a, P2l, 2), p1 = __builtin_amdgcn_alignbyte(P2b, P2a, 2), p2 = __builtin_amdgcn_alignbyte(P2r, P2b, 2);
        // even circle positions in circular order (0,+3) (+2,+2) (+3,0) (+2,-2) (0,-3) (-2,-2) (-3,0) (-2,+2), dword a then dword b
        const uint32_t ra[8] = {P3a, p1, __builtin_amdgcn_alignbyte(Cb, Ca, 3), m1, M3a, m0, __builtin_amdgcn_alignbyte(Ca, Cl, 1), p0};
        const uint32_t rb[8] = {P3b, p2, __builtin_amdgcn_alignbyte(Cr, Cb, 3), m2, M3b, m1, __builtin_amdgcn_alignbyte(Cb, Ca, 1), p1};
        uint32_t nba, nda, nbb, ndb;
        fast_bytes_thresholds(Ca, TT, nba, nda);
        fast_bytes_thresholds(Cb, TT, nbb, ndb);
        uint32_t ba[8], ga[8], bb[8], gb[8];
#pragma unroll
        for (int k = 0; k < 8; k++) {
            ba[k] = __builtin_amdgcn_lerp(ra[k], nba, 0u);              // bit 7: brighter
            ga[k] = __builtin_amdgcn_lerp(ra[k], nda, 0x01010101u);     // bit 7: NOT darker
            bb[k] = __builtin_amdgcn_lerp(rb[k], nbb, 0u);
            gb[k] = __builtin_amdgcn_lerp(rb[k], ndb, 0x01010101u);
        }
        // ring mask: bits 0-7 pixels 0-3 (dword a), bits 8-15 pixels 4-7 (dword b)
        uint32_t m = __builtin_amdgcn_perm(fast_bytes_ringmask(four_of_eight(bb), four_of_eight_dual(gb)),
                                           fast_bytes_ringmask(four_of_eight(ba), four_of_eight_dual(ga)), 0x0c0c0703u);
        if (gi == ng - 1) m &= mLast;
        if (!live) m = 0;
        if (__ballot(m != 0) != 0) {
            // ring positions: entries of lower lanes first; within a lane lowest bit first (pixel by pixel, darker before brighter)
            const int cnt = __popc(m);
            const int incl = wave_incl_scan(cnt);
            const int total = __builtin_amdgcn_readlane(incl, 63);
            auto append = [&](uint16_t *w) {
                for (uint32_t r = m; r; r &= r - 1) {
                    const uint32_t b = __builtin_ctz(r);
                    *w++ = (uint16_t)(((uint32_t)A + (b >> 1)) | ((b & 1u) << 15));
                }
            };
            // (pending is wave-uniform; readfirstlane keeps it, and the branches on it, on the scalar unit)
            if (pending + total <= kRingCap) {
                append(cl + pending + incl - cnt);
                pending = __builtin_amdgcn_readfirstlane(pending + total);
                drain();
            } else {                                       // a step appends up to 1024 entries: then lanes 0-31 first, 32-63 after (at most 512 each)
                const int half = __builtin_amdgcn_readlane(incl, 31);
                if (lane < 32) append(cl + pending + incl - cnt);
                pending = __builtin_amdgcn_readfirstlane(pending + half);
                drain();
                if (lane >= 32) append(cl + pending + incl - half - cnt);
                pending = __builtin_amdgcn_readfirstlane(pending + total - half);
                drain();
            }
        }
    }
    wave_lds_fence();
    if (pending) fast_score_batch<CTP>(tile, sc, sl, nScored, cl, pending, tp, scDelta, tlow, lane);
    return nScored;
}

// One cell's place in its frame.
struct FastCell {
    const uint8_t *img;              // first staged byte: row iniY, column iniX - 1 (any alignment)
    long long cellIdx;
    int pitch, rows, cols, nd;       // image pitch; sub-image size; dwords per staged row
    int ox, oy;                      // cell origin relative to (16, 16): ci_j * wCell, ci_i * hCell
    bool live;
};
__device__ __forceinline__ FastCell fast_cell_geom(const DevParams *__restrict__ P, const ImgSrc &src, int cell, int frame, int32_t *__restrict__ cellCnt, int lane) {
    FastCell g;
    g.live = false;
    if (cell >= P->totalCells) return g;
    int level = 0;
    for (int l = 1; l < P->nlevels; l++)
        if (cell >= P->lv[l].cellBase) level = l;
    const DevLevel &L = P->lv[level];
    const int ci = cell - L.cellBase;
    const int ci_i = ci / L.nCols, ci_j = ci - ci_i * L.nCols;
    g.cellIdx = (long long)frame * P->totalCells + cell;
    const int iniY = kBorder + ci_i * L.hCell, iniX = kBorder + ci_j * L.wCell;
    const int maxY = min(iniY + L.hCell + 6, L.maxBY), maxX = min(iniX + L.wCell + 6, L.maxBX);
    g.cols = maxX - iniX; g.rows = maxY - iniY;
    // skip rules of ORBextractor.cc:752,760 and cv::FAST's 3-px margins
    if (iniY >= L.maxBY - 3 || iniX >= L.maxBX - 6 || g.cols < 7 || g.rows < 7) {
        if (lane == 0) cellCnt[g.cellIdx] = 0;
        return g;
    }
    // tile column c = image column iniX - 1 + c (iniX >= 16): the detection region starts at tile column 4.  A staged row is
    // ceil((cols - 6) / 4) + 2 dwords; its last byte is at most image column maxX + 3 <= width - 13, inside the row.
    g.img = level_base(src, P, level, frame, &g.pitch) + (long long)iniY * g.pitch + (iniX - 1);
    g.nd = ((g.cols - 6 + 3) >> 2) + 2;
    g.ox = ci_j * L.wCell; g.oy = ci_i * L.hCell;
    g.live = true;
    return g;
}
// Staging.  A lane owns ONE dword column c of the tile and one row r0 of every block of rps rows (rps = 64 / dword columns of the tile
// pitch): its offset into the sub-image and its LDS address are computed once, a block adds a wave-uniform row offset to both.  The
// last block is moved up so that it ends with the sub-image's last row (it re-loads a few rows of its predecessor): every lane of a
// block then is in range and no per-lane row test is needed.  The first kStageDepth blocks are in flight together (one memory round
// trip per cell for sub-images of up to kStageDepth x rps rows); lanes of columns beyond the cell's own width idle.  The loads are
// unaligned 4-byte GLOBAL accesses (the tile's column 0 is image column iniX - 1; buffer loads would drop the two low address bits).
constexpr int kStageDepth = 10;
template <int TPC>
__device__ __forceinline__ void fast_cell_stage(const FastCell &g, uint8_t *tile, int tp, int lane) {
    const int TP = TPC ? TPC : tp;
    const int ndT = TP >> 2, rps = min(64 / ndT, 7);           // a sub-image has at least 7 rows
    const int r0 = lane / ndT, c = lane - r0 * ndT;
    if (r0 < rps && c < g.nd) {
        const uint8_t *src = g.img + r0 * g.pitch + 4 * c;
        uint8_t *dst = tile + r0 * TP + 4 * c;
        const int nb = (g.rows + rps - 1) / rps, lastRow = g.rows - rps;
        uint32_t v[kStageDepth];
#pragma unroll
        for (int j = 0; j < kStageDepth; j++)
            if (j < nb) v[j] = reinterpret_cast<const U32 *>(src + (long long)min(j * rps, lastRow) * g.pitch)->v;
#pragma unroll
        for (int j = 0; j < kStageDepth; j++)
            if (j < nb) *reinterpret_cast<uint32_t *>(dst + min(j * rps, lastRow) * TP) = v[j];
        for (int j = kStageDepth; j < nb; j++)                    // taller sub-images: the rest, one round trip per block of rows
            *reinterpret_cast<uint32_t *>(dst + min(j * rps, lastRow) * TP) = reinterpret_cast<const U32 *>(src + (long long)min(j * rps, lastRow) * g.pitch)->v;
    }
}

// everything after the staging of one cell: score map, NMS, ordered emission
template <int TPC>
__device__ __forceinline__ void fast_cell_process(const DevParams *__restrict__ P, const FastLds &F, const FastCell &g, uint8_t *tile, uint8_t *sc,
                                                  uint32_t *__restrict__ cellBuf, int32_t *__restrict__ cellCnt, int lane) {
    const int TP = TPC ? TPC : F.tp;
    const int dw = g.cols - 6, dh = g.rows - 6;
    const unsigned Mdw = magic_of(dw), Mtp = magic_of(TP);
    for (int idx = lane * 16; idx < (dh + 2) * TP; idx += 1024) *reinterpret_cast<uint4 *>(&sc[idx]) = make_uint4(0, 0, 0, 0);   // (scBytes is a multiple of 16)
    wave_lds_fence();
    const int npx = dw * dh;
    const int scDelta = -2 * TP - 3;                                 // tile offset of a detection pixel -> its byte in the score map
    uint16_t *cl = reinterpret_cast<uint16_t *>(sc + F.scBytes);
    uint16_t *sl = cl + kRingCap;
    // Two passes, as upstream calls cv::FAST (:771-785): threshold iniThFAST first, and minThFAST only when the cell yields no key-point (after
    // NMS) at iniThFAST.  A pixel below the pass's threshold can neither be emitted nor suppress a neighbour (cv::FAST's score rows hold 0
    // for it, and NMS needs a strictly larger neighbour), so each pass scores only what reaches ITS threshold: at iniThFAST the quick test
    // passes a fraction of the pixels it passes at minThFAST, and textured cells never run the second pass.
    int thr = max(1, P->iniTh);
    uint32_t *out = cellBuf + g.cellIdx * P->maxCellCand;
    int found;
#pragma nounroll
    for (int pass = 0;; pass++) {
        const int nScored = fast_score_cell_bytes<TPC>(tile, sc, cl, sl, TP, dw, dh, thr, lane);
        wave_lds_fence();
        // NMS + emission in one sweep over the scored list (ascending pixel order = the row-major order cv::FAST emits in; every pixel at
        // most once); a cell with more than kScoredCap scored pixels scans its whole score map instead.  Two items per lane and sweep, all
        // their LDS reads issued together and the eight comparisons evaluated without short-circuit: a sweep costs two LDS round trips, not
        // ten.  Survivors go straight to the cell's output slots (a pass that finds nothing has written nothing).
        const bool listed = nScored <= kScoredCap;
        const int nItems = listed ? nScored : npx;
        found = 0;
        for (int base = 0; base < nItems; base += 128) {
            int si[2];
            bool in[2];
#pragma unroll
            for (int h = 0; h < 2; h++) {
                const int k = base + 64 * h + lane;
                in[h] = k < nItems;
                if (listed) {
                    si[h] = (int)sl[in[h] ? k : 0] + scDelta;                     // score-map offset of the pixel
                } else {
                    const int kk = in[h] ? k : 0, py = magic_div(kk, Mdw);
                    si[h] = mul24(py + 1, TP) + (kk - mul24(py, dw)) + 1;
                }
            }
            int v[2];
            bool isMax[2];
#pragma unroll
            for (int h = 0; h < 2; h++) {
                const uint8_t *s = &sc[si[h]];
                v[h] = s[0];
                const int n0 = s[-TP - 1], n1 = s[-TP], n2 = s[-TP + 1], n3 = s[-1], n4 = s[1], n5 = s[TP - 1], n6 = s[TP], n7 = s[TP + 1];
                isMax[h] = in[h] & (v[h] > 0) & (v[h] > n0) & (v[h] > n1) & (v[h] > n2) & (v[h] > n3) & (v[h] > n4) & (v[h] > n5) & (v[h] > n6) & (v[h] > n7);
            }
            const unsigned long long b0 = __ballot(isMax[0]), b1 = __ballot(isMax[1]);
            const int c0 = __popcll(b0);
#pragma unroll
            for (int h = 0; h < 2; h++) {
                if (isMax[h]) {
                    const unsigned long long b = h ? b1 : b0;
                    const int slot = __builtin_amdgcn_mbcnt_hi((uint32_t)(b >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)b, found + (h ? c0 : 0)));
                    const int py1 = magic_div(si[h], Mtp), px1 = si[h] - mul24(py1, TP);     // score-map row / column = detection row / column + 1
                    const uint32_t x = (uint32_t)(px1 + 2 + g.ox), y = (uint32_t)(py1 + 2 + g.oy);
                    out[slot] = x | (y << 12) | ((uint32_t)v[h] << 24);
                }
            }
            found += c0 + __popcll(b1);
        }
        if (found > 0 || pass == 1) break;               // retry with minThFAST only if the first call found nothing (:783)
        thr = max(1, P->minTh);                                      // scores of the first pass that are still in the map are rewritten with the same values
    }
    if (lane == 0) cellCnt[g.cellIdx] = found;
}

// TPC: tile pitch (= score-map pitch) as a compile-time constant: the circle offsets and the NMS neighbours then are immediate LDS
// offsets instead of one address add each; 0 = run-time
// (bx, gx): the workgroup's column and the columns of the FAST part of the launch (the whole grid, or its first gx columns in the fused launch)
template <int TPC>
__device__ __forceinline__ void fast_cells_body(const DevParams *__restrict__ P, const ImgSrc &src, const FastLds &F, uint32_t *__restrict__ cellBuf,
                                                int32_t *__restrict__ cellCnt, unsigned bx, unsigned gx) {
    extern __shared__ __attribute__((aligned(16))) uint8_t fl[];
    // the wave index as a scalar: everything that depends only on the cell (geometry, magic numbers, LDS bases) then runs on the scalar unit
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const unsigned wg = xcd_swizzle(blockIdx.y * gx + bx, gx * gridDim.y);
    const int wpg = blockDim.x >> 6;
    const int cell = (wg % gx) * wpg + wave, frame = wg / gx;
    uint8_t *tile = fl + (size_t)wave * F.perWave;
    uint8_t *sc = tile + F.tileBytes;
    const int TP = TPC ? TPC : F.tp;
    const FastCell gA = fast_cell_geom(P, src, cell, frame, cellCnt, lane);
    if (!gA.live) return;
    fast_cell_stage<TPC>(gA, tile, TP, lane);
    fast_cell_process<TPC>(P, F, gA, tile, sc, cellBuf, cellCnt, lane);
}
template <int TPC>
__global__ __launch_bounds__(256) void k_fast_cells(const DevParams *__restrict__ P, ImgSrc src, FastLds F,
                                                    uint32_t *__restrict__ cellBuf, int32_t *__restrict__ cellCnt) {
    fast_cells_body<TPC>(P, src, F, cellBuf, cellCnt, blockIdx.x, gridDim.x);
}

// ------------------------------------------------------------------------------------------------
// Candidate compaction: one workgroup per frame concatenates the cell lists in cell order (levels
// ascending, cells row-major) into cand[frame][...] and writes levelStart[frame][0..nlevels].
// A level that would exceed its capacity is truncated and flagged (bit 4 of the call's error word); the host turns that into
// RUMI_E_CAPACITY.
// ------------------------------------------------------------------------------------------------
// 256 threads (a 1024-thread workgroup waits for a CU with sixteen free wave slots beside the other streams' kernels: 0.42 ms per 256-frame launch
// in the pipelined step against 0.03 ms alone -- without costing the step anything measurable; one frame: 6.7 -> ~3 us)
// hist != null (batches: the quadtree pipeline of orb_octree_kernel.hip): every candidate is also counted in the depth-D quadtree cell of its
// level, hist[frame][level's cells], 16-bit counts two to a dword -- the table the quadtree kernel used to fill by a pass of its own over the
// keys.  The cell comes from the host-built coordinate tables (bins).
constexpr int kCompactThreads = 256;
__global__ __launch_bounds__(kCompactThreads) void k_compact(const DevParams *__restrict__ P, const uint32_t *__restrict__ cellBuf,
                                                 const int32_t *__restrict__ cellCnt, uint32_t *__restrict__ cand,
                                                 int32_t *__restrict__ levelStart, int32_t *__restrict__ errFlag,
                                                 uint32_t *__restrict__ hist, const uint16_t *__restrict__ bins) {
    extern __shared__ int sStart[];          // totalCells + 1 exclusive prefix
    __shared__ int part[kCompactThreads];
    const int tid = threadIdx.x, frame = blockIdx.x;
    const int nc = P->totalCells;
    const int32_t *cnt = cellCnt + (long long)frame * nc;
    const int chunk = (nc + kCompactThreads - 1) / kCompactThreads;
    int sum = 0;
    for (int k = 0; k < chunk; k++) {
        const int c = tid * chunk + k;
        if (c < nc) sum += cnt[c];
    }
    // exclusive scan of the per-thread sums: shuffles inside a wave, the 16 wave totals through LDS
    const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    int inc = sum;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(inc, o);
        if (lane >= o) inc += t;
    }
    if (lane == 63) part[wave] = inc;
    __syncthreads();
    int base = 0, total = 0;
#pragma unroll
    for (int w = 0; w < kCompactThreads / 64; w++) {
        const int t = part[w];
        if (w < wave) base += t;
        total += t;
    }
    if (tid == 0) sStart[nc] = total;
    int run = base + inc - sum;
    for (int k = 0; k < chunk; k++) {
        const int c = tid * chunk + k;
        if (c < nc) { sStart[c] = run; run += cnt[c]; }
    }
    __syncthreads();
    // few frames per launch: gridDim.y workgroups share a frame's outputs (each repeats the cheap scan), which cuts the latency of a
    // single-frame call; slice 0 publishes the level starts
    int32_t *ls = levelStart + (long long)frame * (kMaxLevels + 1);
    if (blockIdx.y == 0 && tid <= P->nlevels) {
        const int c = tid < P->nlevels ? P->lv[tid].cellBase : nc;
        ls[tid] = sStart[c];
    }
    if (blockIdx.y == 0 && tid < P->nlevels) {
        const int c0 = P->lv[tid].cellBase, c1 = c0 + P->lv[tid].nCells;
        if (sStart[c1] - sStart[c0] > P->lv[tid].candCap) atomicOr(errFlag, 16);
    }
    uint32_t *out = cand + (long long)frame * P->totalCand;
    // one lane per output element: its cell is the last one whose start is <= j (binary search in the LDS prefix), so every
    // lane has an independent load in flight instead of a wave walking its cells one round trip at a time
    const int nOut = min(sStart[nc], P->totalCand);
    const uint32_t *inBase = cellBuf + (long long)frame * nc * P->maxCellCand;
    if (!hist) {
        for (int j = blockIdx.y * kCompactThreads + tid; j < nOut; j += kCompactThreads * gridDim.y) {
            int lo = 0, hi = nc;                       // invariant: sStart[lo] <= j < sStart[hi]
            while (hi - lo > 1) {
                const int mid = (lo + hi) >> 1;
                if (sStart[mid] <= j) lo = mid; else hi = mid;
            }
            out[j] = inBase[(long long)lo * P->maxCellCand + (j - sStart[lo])];
        }
        return;
    }
    // ... and the count of the candidate's quadtree cell; whole waves walk the loop (wave_run_add looks at the neighbour lanes)
    __shared__ int sLevCell[kMaxLevels];           // first FAST cell of the level
    __shared__ int4 sLev[kMaxLevels];              // {its coordinate tables, its first entry in the frame's row (-1: none), W, H}
    if (tid < P->nlevels) {
        const DevLevel &L = P->lv[tid];
        sLevCell[tid] = L.cellBase;
        sLev[tid] = make_int4(L.octBin, L.octCells > 0 ? L.octCell : -1, L.maxBX - kBorder, L.maxBY - kBorder);
    }
    static_assert(sizeof(part) + sizeof(sLevCell) + sizeof(sLev) + 64 <= kCompactStaticLds, "oct_hist_lds_bytes sizes the launch with this bound");
    // The workgroup counts into a table of its own in LDS (behind the cell prefix; oct_hist_lds_bytes: a geometry whose table does not fit has
    // no pipeline) and adds what is not zero to the frame's row at the end -- the candidates of a FAST cell's row rarely fill a run, so
    // counting straight into HBM / L2 was one atomic per candidate or two (measured: 106 us alone against 48).  A workgroup takes a
    // CONTIGUOUS share of the candidates, so its counts fall into a share of the cells
    const int nl = P->nlevels, hw = P->octCellStride / 2;
    uint32_t *hf = hist + (size_t)frame * (size_t)hw;
    uint32_t *sh = reinterpret_cast<uint32_t *>(sStart + nc + 1);
    for (int i = tid; i < hw; i += kCompactThreads) sh[i] = 0u;
    __syncthreads();
    const int per = ((nOut + (int)gridDim.y - 1) / (int)gridDim.y + kCompactThreads - 1) / kCompactThreads * kCompactThreads;
    const int jBeg = min(nOut, (int)blockIdx.y * per), jEnd = min(nOut, jBeg + per);
    for (int j0 = jBeg; j0 < jEnd; j0 += kCompactThreads) {
        const int j = j0 + tid;
        int entry = -1;                            // the cell's entry in the frame's row: equal for equal (level, cell)
        if (j < jEnd) {
            int lo = 0, hi = nc;
            while (hi - lo > 1) {
                const int mid = (lo + hi) >> 1;
                if (sStart[mid] <= j) lo = mid; else hi = mid;
            }
            const uint32_t ck = inBase[(long long)lo * P->maxCellCand + (j - sStart[lo])];
            out[j] = ck;
            int l = 0;
            for (int k = 1; k < nl; k++) l += sLevCell[k] <= lo;
            const int4 L = sLev[l];
            if (L.y >= 0) {
                const uint16_t *xbin = bins + L.x, *ybin = xbin + L.z + 1;
                entry = L.y + ((int)xbin[min((int)(ck & 0xFFFu), L.z)] | (int)ybin[min((int)((ck >> 12) & 0xFFFu), L.w)]);
            }
        }
        wave_run_add(entry, sh + ((entry < 0 ? 0 : entry) >> 1), 1u << (16 * (entry & 1)));
    }
    __syncthreads();
    for (int i = tid; i < hw; i += kCompactThreads) {
        const uint32_t w = sh[i];
        if (w) atomicAdd(hf + i, w);
    }
}
// ---- launch wrappers (called from orb_schedule.inc) ----
static FastLds fast_lds_of(const DevParams &hP) {
    // LDS per wave from the largest cell of this geometry
    int wMax = 0, hMax = 0;
    for (int l = 0; l < hP.nlevels; l++) { wMax = std::max(wMax, hP.lv[l].wCell); hMax = std::max(hMax, hP.lv[l].hCell); }
    FastLds F;
    F.tp = 4 * (((wMax + 3) >> 2) + 2);                   // the detection region's 4-pixel groups + one dword of margin on either side (tile column 4 = first detection column)
    F.sp = F.tp;                                          // the score map shares the tile's pitch (a pixel's score byte sits at its tile offset + a constant)
    F.tileBytes = (hMax + 6) * F.tp;
    F.scBytes = ((hMax + 2) * F.sp + 15) & ~15;
    F.maxIters = (wMax * hMax + 63) / 64 + 1;
    F.tileBytes = (F.tileBytes + 15) & ~15;
    // tile | score map | ring of (pixel, polarity) entries that passed the quick test (linear, kRingCap x uint16; the NMS ballots reuse it) |
    // list of scored pixels (kScoredCap x uint16)
    F.perWave = (F.tileBytes + F.scBytes + std::max(kRingCap * 2, F.maxIters * 8) + kScoredCap * 2 + 15) & ~15;
    return F;
}
void launch_fast(const DevParams *dP, const DevParams &hP, ImgSrc src, uint32_t *cellBuf, int32_t *cellCnt, int nframes,
                 hipStream_t st) {
    const FastLds F = fast_lds_of(hP);
    // tile pitches of the common image sizes as compile-time constants (cells up to 36 / 40 / 44 / 48 pixels wide: 44 / 48 / 52 / 56);
    // anything else takes the run-time instantiation
    const int wpg = 4;                                    // cells (= waves) per workgroup
    const dim3 grid((hP.totalCells + wpg - 1) / wpg, nframes);
    const size_t lds = (size_t)wpg * F.perWave;
#define RUMI_FAST_CASE(T)                                                                                      \
    if (F.tp == T) {                                                                                           \
        hipLaunchKernelGGL((k_fast_cells<T>), grid, dim3(64 * wpg), lds, st, dP, src, F, cellBuf, cellCnt);    \
        return;                                                                                                \
    }
    RUMI_FAST_CASE(48) RUMI_FAST_CASE(44) RUMI_FAST_CASE(52) RUMI_FAST_CASE(56)
#undef RUMI_FAST_CASE
    hipLaunchKernelGGL((k_fast_cells<0>), grid, dim3(64 * wpg), lds, st, dP, src, F, cellBuf, cellCnt);
}
// workgroups per frame (each repeats the cheap scan and copies its share of the outputs: the copy is a chain of dependent LDS reads per
// element, so one workgroup per frame is ~40 us of latency whatever the batch)
static int compactSlices(int nframes) { return nframes < 32 ? 32 : 8; }
void launch_compact(const DevParams *dP, const DevParams &hP, const uint32_t *cellBuf, const int32_t *cellCnt,
                    uint32_t *cand, int32_t *levelStart, int32_t *errFlag, int nframes, hipStream_t st, uint32_t *hist, const uint16_t *bins) {
    // with a histogram: the workgroup's own count table behind the prefix (640 x 480, 8 levels: 4 KB); set_geometry has checked that it fits
    const size_t histBytes = hist ? (size_t)oct_hist_lds_bytes(hP.totalCells, hP.octCellStride) : 0;
    hipLaunchKernelGGL(k_compact, dim3(nframes, compactSlices(nframes)), dim3(kCompactThreads), (hP.totalCells + 1) * sizeof(int) + histBytes, st, dP, cellBuf,
                       cellCnt, cand, levelStart, errFlag, hist, bins);
}

}  // namespace rumi
