// Orientation, rBRIEF and output assembly: k_orient_desc (with k_assemble's work in its prologue for calls of a few frames), the two kernels batches
// take instead (k_disc_angle: IC_Angle and the trigonometry, a key-point per lane; k_orient_desc<2, false, true>: rBRIEF and the output) and the
// launch wrappers.
namespace rumi {

// ------------------------------------------------------------------------------------------------
// Orientation + descriptor + output assembly: one HALF wave (32 lanes) per selected key-point, eight key-points per workgroup.
//   The arithmetic that is the same for every lane of a key-point (fastAtan2, the libm sinf / cosf restatement in double precision, the
//   record) is a third of the fused kernel: with two key-points per wave an instruction serves both.  Batches (orient_desc_split) leave it and
//   IC_Angle to k_disc_angle, where a lane IS a key-point for it, and run the descriptor part alone (kSplit).
//   IC_Angle: integer moments over the radius-15 disc of the UN-blurred level, lane = disc column;
//   rBRIEF:   lane l evaluates test pairs l, l+32, ... l+224; __ballot packs 32 bits per key-point at a time, which
//             is exactly the descriptor's little-endian bit order (bit k of byte i = pair 8i+k).
// ------------------------------------------------------------------------------------------------
// sum over the 32 lanes of a half wave, returned in every lane of that half: DPP adds inside the rows of 16 (the row's total lands in its
// lane 15), row_bcast:15 carries it into the next row, lanes 31 / 63 then hold the two totals (five ds_bpermute round trips otherwise)
__device__ __forceinline__ int half_wave_sum(int v) {
    v += __builtin_amdgcn_update_dpp(0, v, 0x111, 0xF, 0xF, false);          // row_shr:1
    v += __builtin_amdgcn_update_dpp(0, v, 0x112, 0xF, 0xF, false);          // row_shr:2
    v += __builtin_amdgcn_update_dpp(0, v, 0x114, 0xF, 0xF, false);          // row_shr:4
    v += __builtin_amdgcn_update_dpp(0, v, 0x118, 0xF, 0xF, false);          // row_shr:8
    v += __builtin_amdgcn_update_dpp(0, v, 0x142, 0xA, 0xF, false);          // row_bcast:15 -> rows 1 and 3
    const int lo = __builtin_amdgcn_readlane(v, 31), hi = __builtin_amdgcn_readlane(v, 63);
    return (threadIdx.x & 32) ? hi : lo;
}
__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

constexpr int kDiscP = 48, kPatchP = 48;       // LDS row pitches: 36 and 40 staged bytes per row (31 / 37 + alignment slack), rows 16-byte aligned for b128 stores
constexpr int kKpPerWg = 8;                    // half waves of a workgroup
constexpr int kPatchRows = 37, kPatchRowPieces = 5, kPatchTrips = (kPatchRows * kPatchRowPieces + 31) / 32;   // the patch as 8-byte pieces: 185 in six trips of a half wave
// kKpGroups: key-points a half wave handles one after the other (the next one's pixels are in flight meanwhile).  Two for batches (kSplit): with four,
// the workgroups resident on an XCD span five frames instead of two and a half, their pyramids no longer fit its L2 and the kernel fetches
// 1.7x the bytes (FETCH_SIZE).  One for a handful of frames: there are not enough workgroups to fill the chip otherwise.

// kAssemble (calls of a few frames): k_assemble's work -- concatenate the levels, the lapping rule's slots (ORBextractor.cc:1077-1085), the frame's
// {n, monoIndex} -- is done by every workgroup for its own key-points in its prologue (a count over the frame's <= ~1100 selected key-points: four
// loads a thread), so that launch and its ~7 us on the dependent chain of a one-frame call disappear; workgroup 0 of a frame writes the counts and,
// for calls whose results go straight to pinned host memory, the call's final error word.
struct AssembleArgs {
    const uint32_t *selLevel; const int32_t *selLevelCnt; int selLevelCap, lap0, lap1;
    int32_t *counts; long long countsStride; int32_t *errFlag, *errMirror;
    uint32_t *selPackedOut, *selMetaOut; int32_t *selCountOut;      // k_assemble's arrays are still written (the parity taps read them)
};
// kSplit (batches): the angle and its cosine / sine come from k_disc_angle's array (indexed like selMeta); no disc is fetched or staged here.
template <int kKpGroups, bool kAssemble, bool kSplit>
__global__ __launch_bounds__(256, kSplit ? 8 : 7) void k_orient_desc(const DevParams *__restrict__ P, ImgSrc src,
                                                     const uint32_t *__restrict__ selPacked,
                                                     const uint32_t *__restrict__ selMeta,
                                                     const int32_t *__restrict__ selCount, int selCap,
                                                     RumiKeyPoint *__restrict__ kpOut, long long kpStride, uint8_t *__restrict__ descOut,
                                                     long long descStride, int outCap, AssembleArgs A, const float4 *__restrict__ trig) {
    static_assert(!(kSplit && kAssemble), "the split form reads k_assemble's arrays");
    // per key-point: the 31-row disc neighbourhood of the un-blurred level, THEN (in the same LDS: the moments are done with the disc before the
    // descriptor wants the patch) the 37-row patch of the blurred level, staged by the half wave that owns the key-point and read by nobody else:
    // no workgroup barrier anywhere past the pattern table's.  18 KB per workgroup: seven workgroups per CU (30 KB with both resident: five)
    static_assert(kDiscP == kPatchP, "the disc and the patch share their rows");
    __shared__ __attribute__((aligned(16))) uint8_t sWin[kKpPerWg][37 * kPatchP];
    __shared__ __attribute__((aligned(16))) float sPat[256 * 4];
    __shared__ int4 sLv[kMaxLevels];              // per level: offset and pitch of the un-blurred image (level 0 = the caller's frame), of the blurred one
    __shared__ float2 sLvF[kMaxLevels];           // scale, patch size
    reinterpret_cast<float4 *>(sPat)[threadIdx.x] = reinterpret_cast<const float4 *>(c_patternF.v)[threadIdx.x];
    if (threadIdx.x < (unsigned)P->nlevels) {
        const DevLevel &Lv = P->lv[threadIdx.x];
        sLv[threadIdx.x] = threadIdx.x == 0 ? make_int4(0, src.l0Pitch, (int)Lv.off, Lv.pitch) : make_int4((int)Lv.off, Lv.pitch, (int)Lv.off, Lv.pitch);
        sLvF[threadIdx.x] = make_float2(Lv.scale, Lv.patchSize);
    }
    const int lane = threadIdx.x & 31, hw = threadIdx.x >> 5;             // lane within the half wave, half-wave index 0..7
    const unsigned wg = xcd_swizzle(blockIdx.y * gridDim.x + blockIdx.x, gridDim.x * gridDim.y);   // a frame's key-points share one L2
    const int kb = (wg % gridDim.x) * (kKpPerWg * kKpGroups) + hw, frame = wg / gridDim.x;
    int cnt;
    __shared__ uint32_t sOwnPk[kAssemble ? kKpPerWg * kKpGroups : 1], sOwnMt[kAssemble ? kKpPerWg * kKpGroups : 1];
    if constexpr (!kAssemble) {
        cnt = selCount[frame];
        __syncthreads();
    } else {
        __shared__ int sLvStart[kMaxLevels + 1], sRed[2], sOwnF[kKpPerWg * kKpGroups];
        const int nl = P->nlevels, tid = threadIdx.x;
        if (tid == 0) {
            int run = 0;
            for (int l = 0; l < nl; l++) { sLvStart[l] = run; run += A.selLevelCnt[(long long)frame * nl + l]; }
            sLvStart[nl] = run; sRed[0] = 0; sRed[1] = 0;
        }
        __syncthreads();
        const int total = sLvStart[nl], kbase = (wg % gridDim.x) * (kKpPerWg * kKpGroups);
        const bool first = wg % gridDim.x == 0, over = total > selCap;
        int32_t *counts = reinterpret_cast<int32_t *>(reinterpret_cast<uint8_t *>(A.counts) + frame * A.countsStride);
        if (over) {                                           // k_assemble's refusal: more key-points than the selection arrays hold
            if (first && tid == 0) { A.selCountOut[frame] = 0; counts[0] = total; counts[1] = 0; const int old = atomicOr(A.errFlag, 8); if (A.errMirror) *A.errMirror = old | 8; }
            return;
        }
        cnt = total;
        auto key_at = [&](int k, int *levelOut) -> uint32_t {
            int level = 0;
            while (k >= sLvStart[level + 1]) level++;
            *levelOut = level;
            return A.selLevel[((long long)frame * nl + level) * A.selLevelCap + (k - sLvStart[level])];
        };
        auto lapped = [&](uint32_t pk, int level) -> bool {
            float x = (float)((int)(pk & 0xFFF) + kBorder);
            if (level != 0) x = x * P->lv[level].scale;
            return x >= (float)A.lap0 && x <= (float)A.lap1;
        };
        int before = 0, all = 0;
        for (int k = tid; k < total; k += 256) {
            int level;
            const uint32_t pk = key_at(k, &level);
            const int f = lapped(pk, level) ? 1 : 0;
            all += f; before += k < kbase ? f : 0;
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) { before += __shfl_xor(before, o); all += __shfl_xor(all, o); }
        if ((tid & 63) == 0) { atomicAdd(&sRed[0], before); atomicAdd(&sRed[1], all); }
        if (tid < kKpPerWg * kKpGroups) {
            const int k = kbase + tid;
            int level = 0;
            uint32_t pk = 0;
            int f = 0;
            if (k < total) { pk = key_at(k, &level); f = lapped(pk, level) ? 1 : 0; }
            sOwnPk[tid] = pk; sOwnMt[tid] = (uint32_t)level; sOwnF[tid] = f;
        }
        __syncthreads();
        if (tid == 0) {
            int b = sRed[0];
            for (int j = 0; j < kKpPerWg * kKpGroups; j++) {
                const int k = kbase + j;
                if (k >= total) break;
                const int f = sOwnF[j], slot = f ? (total - 1 - b) : (k - b);
                b += f;
                sOwnMt[j] |= (uint32_t)slot << 8;
            }
            if (first) {
                counts[0] = total; counts[1] = total - sRed[1];      // {n, monoIndex}
                A.selCountOut[frame] = total;
                if (A.errMirror) *A.errMirror = *A.errFlag;
            }
        }
        __syncthreads();
        if (tid < kKpPerWg * kKpGroups && kbase + tid < total) {
            A.selPackedOut[(long long)frame * selCap + kbase + tid] = sOwnPk[tid];
            A.selMetaOut[(long long)frame * selCap + kbase + tid] = sOwnMt[tid];
        }
    }
#ifdef RUMI_OD_STAMP
    long long st[8] = {0, 0, 0, 0, 0, 0, 0, 0}, stLast = clock64();
#define OD_STAMP(k) do { const long long t_ = clock64(); st[k] += t_ - stLast; stLast = t_; } while (0)
#else
#define OD_STAMP(k) do { } while (0)
#endif

    struct __attribute__((packed, aligned(4))) Q16 { uint32_t x, y, z, w; };      // (dword-aligned wide loads)
    struct __attribute__((packed, aligned(4))) Q8 { uint32_t x, y; };
    auto ld16 = [](const uint8_t *q) { const Q16 t = *reinterpret_cast<const Q16 *>(q); return make_uint4(t.x, t.y, t.z, t.w); };
    auto ld8 = [](const uint8_t *q) { const Q8 t = *reinterpret_cast<const Q8 *>(q); return make_uint2(t.x, t.y); };
    struct Staged { uint4 d0, d1, p0, p1, q0, q1; uint2 p2, q2; uint32_t d2; uint2 c[kPatchTrips]; };
    // kSplit: the patch by 8-byte pieces, five a row, piece q = lane + 32 t of the half wave in trip t: the pieces of a row sit in neighbouring
    // lanes of ONE load instruction, which then asks for six or seven cache lines instead of a line per lane (0.105 -> 0.096 ms per 256 frames
    // against the row form in this kernel).  The same bytes as the row form's, to the same LDS addresses.
    int pcRow[kPatchTrips], pcCol[kPatchTrips];
    if constexpr (kSplit) {
#pragma unroll
        for (int t = 0; t < kPatchTrips; t++) { const int q = lane + 32 * t; pcRow[t] = q / kPatchRowPieces; pcCol[t] = (q % kPatchRowPieces) * 8; }
    }
    const bool dRow = lane < 31, qRow = lane < 5;
    const uint8_t *frame0 = src.l0 + (long long)frame * src.l0FrameStride, *framePyr = src.pyr + (long long)frame * P->arenaStride,
                  *frameBlur = src.blur + (long long)frame * P->arenaStride;
    // lane = row: a row's 36 / 40 bytes are two 16-byte loads and a 4- / 8-byte one (dword-aligned addresses; the 37 rows of the patch take a
    // second, five-lane trip); no index arithmetic
    auto fetch_disc = [&](uint32_t pk, uint32_t meta, bool live, Staged &S) {
        if (!live || !dRow) return;
        const int level = meta & 0xFF, x = (int)(pk & 0xFFF) + kBorder, y = (int)((pk >> 12) & 0xFFF) + kBorder;
        const int4 lv = sLv[level];                                       // (a frame's arena is far below 2 GB: 32-bit offsets)
        const uint8_t *cr = (level == 0 ? frame0 : framePyr) + (lv.x + (y - kHalfPatch + lane) * lv.y + ((x - kHalfPatch) & ~3));
        S.d0 = ld16(cr); S.d1 = ld16(cr + 16); S.d2 = *reinterpret_cast<const uint32_t *>(cr + 32);
    };
    auto fetch_patch = [&](uint32_t pk, uint32_t meta, bool live, Staged &S) {
        if (!live) return;
        const int level = meta & 0xFF, x = (int)(pk & 0xFFF) + kBorder, y = (int)((pk >> 12) & 0xFFF) + kBorder;
        const int4 lv = sLv[level];
        if constexpr (kSplit) {
            const uint8_t *b0 = frameBlur + (lv.z + (y - 18) * lv.w + ((x - 18) & ~3));
#pragma unroll
            for (int t = 0; t < kPatchTrips; t++)
                if (pcRow[t] < kPatchRows) S.c[t] = ld8(b0 + (pcRow[t] * lv.w + pcCol[t]));
            return;
        }
        const uint8_t *br = frameBlur + (lv.z + (y - 18 + lane) * lv.w + ((x - 18) & ~3)), *br2 = br + 32 * lv.w;
        S.p0 = ld16(br); S.p1 = ld16(br + 16); S.p2 = ld8(br + 32);
        if (qRow) { S.q0 = ld16(br2); S.q1 = ld16(br2 + 16); S.q2 = ld8(br2 + 32); }
    };
    auto stage_disc = [&](bool live, const Staged &S) {
        if (!live || !dRow) return;
        uint8_t *dst = &sWin[hw][lane * kDiscP];
        *reinterpret_cast<uint4 *>(dst) = S.d0; *reinterpret_cast<uint4 *>(dst + 16) = S.d1; *reinterpret_cast<uint32_t *>(dst + 32) = S.d2;
    };
    auto stage_patch = [&](bool live, const Staged &S) {
        if (!live) return;
        if constexpr (kSplit) {
#pragma unroll
            for (int t = 0; t < kPatchTrips; t++)
                if (pcRow[t] < kPatchRows) *reinterpret_cast<uint2 *>(&sWin[hw][pcRow[t] * kPatchP + pcCol[t]]) = S.c[t];
            return;
        }
        {
            uint8_t *dst = &sWin[hw][lane * kPatchP];
            *reinterpret_cast<uint4 *>(dst) = S.p0; *reinterpret_cast<uint4 *>(dst + 16) = S.p1; *reinterpret_cast<uint2 *>(dst + 32) = S.p2;
        }
        if (qRow) {
            uint8_t *dst = &sWin[hw][(lane + 32) * kPatchP];
            *reinterpret_cast<uint4 *>(dst) = S.q0; *reinterpret_cast<uint4 *>(dst + 16) = S.q1; *reinterpret_cast<uint2 *>(dst + 32) = S.q2;
        }
    };
    auto orientation = [&](uint32_t pk) -> float {
        const int x = (int)(pk & 0xFFF) + kBorder;
        const int xd = (x - kHalfPatch) & ~3;
        // IC_Angle (ORBextractor.cc:73-97): lane = column u of the disc; the disc is symmetric (|u| <= umax[|v|]  <=>  |v| <= umax[|u|]), so a
        // lane's rows are |v| <= umax[|u|], known before the loop; m10 = u * (sum of the column), m01 = sum of v * pixel
        const uint8_t *dc = &sWin[hw][kHalfPatch * kDiscP + (x - xd)];
        const int u = lane - kHalfPatch;
        const int vmaxU = lane < 31 ? P->umax[u < 0 ? -u : u] : -1;
        // rows +v and -v share their bound: one compare masks both; every row of the staged disc exists, so the reads are unconditional
        const int mid = dc[u];
        int colSum = vmaxU >= 0 ? mid : 0, m01 = 0;
#pragma unroll
        for (int v = 1; v <= kHalfPatch; v++) {
            const int lo = dc[-v * kDiscP + u], hi = dc[v * kDiscP + u];
            const bool in = v <= vmaxU;
            colSum += in ? lo + hi : 0;
            m01 += in ? v * (hi - lo) : 0;
        }
        int m10 = u * colSum;
        m10 = half_wave_sum(m10);
        m01 = half_wave_sum(m01);
        OD_STAMP(4);
        return fast_atan2_deg((float)m01, (float)m10);
    };
    auto describe = [&](uint32_t pk, uint32_t meta, float angle, float cosA, float sinA) {
        const int level = meta & 0xFF, slot = (int)(meta >> 8);
        const int x = (int)(pk & 0xFFF) + kBorder, y = (int)((pk >> 12) & 0xFFF) + kBorder, score = (int)(pk >> 24);
        const int xp = (x - 18) & ~3;
        // computeOrbDescriptor (ORBextractor.cc:99-143) on the blurred level
        float a = cosA, b = sinA;
        if constexpr (!kSplit) {
            const float factorPI = (float)(3.1415926535897932384626433832795 / 180.f);
            const float ang = angle * factorPI;
            a = cosf_glibc(ang); b = sinf_glibc(ang);
        }
        const uint8_t *bc = &sWin[hw][18 * kPatchP + (x - xp)];
        uint32_t w = 0;                                                   // lane j of the half wave ends up with descriptor word j
        OD_STAMP(5);
#pragma unroll
        for (int j = 0; j < 8; j++) {
            const float4 pt = reinterpret_cast<const float4 *>(sPat)[j * 32 + lane];
            const float x0 = pt.x, y0 = pt.y, x1 = pt.z, y1 = pt.w;
            const int r0 = cv_round_f(x0 * b + y0 * a), c0 = cv_round_f(x0 * a - y0 * b);
            const int r1 = cv_round_f(x1 * b + y1 * a), c1 = cv_round_f(x1 * a - y1 * b);
            const int t0 = bc[r0 * kPatchP + c0], t1 = bc[r1 * kPatchP + c1];
            const unsigned long long bal = __ballot(t0 < t1);             // both key-points of the wave; lanes j and 32 + j keep their halves
            const uint32_t lo = (uint32_t)bal, hi = (uint32_t)(bal >> 32);
            // (v_writelane reads its scalar operand early: the compare that wrote it needs wait states the assembler does not add inside asm
            //  blocks; without them lanes 32.. received the PREVIOUS ballot)
            asm("s_nop 4\n\tv_writelane_b32 %0, %1, %3\n\tv_writelane_b32 %0, %2, %4" : "+v"(w) : "s"(lo), "s"(hi), "n"(j), "n"(32 + j));
        }
        OD_STAMP(6);
        if (slot < outCap) {
            if (lane < 8) reinterpret_cast<uint32_t *>(descOut + frame * descStride + (long long)slot * 32)[lane] = w;
            if (lane == 0) {
                RumiKeyPoint kp;
                kp.x = (float)x; kp.y = (float)y;
                const float2 lf = sLvF[level];
                if (level != 0) { kp.x = kp.x * lf.x; kp.y = kp.y * lf.x; }   // keypoint->pt *= scale (:1073-1075)
                kp.size = lf.y;
                kp.angle = angle;
                kp.response = (float)score;
                kp.octave = level;
                kp.class_id = -1;
                reinterpret_cast<RumiKeyPoint *>(reinterpret_cast<uint8_t *>(kpOut) + frame * kpStride)[slot] = kp;
            }
        }
    };

    const uint32_t *selP = selPacked + (long long)frame * selCap, *selM = selMeta + (long long)frame * selCap;
    const float4 *selT = kSplit ? trig + (long long)frame * selCap : nullptr;
    auto key_rec = [&](int k, uint32_t &pk, uint32_t &mt, float4 &tg) {     // key-point k of the frame: from k_assemble's arrays, or from this workgroup's own prologue
        if constexpr (kAssemble) { const int j = k - (kb - hw); pk = sOwnPk[j]; mt = sOwnMt[j]; }
        else { pk = selP[k]; mt = selM[k]; }
        if constexpr (kSplit) tg = selT[k];                                 // {angle, cos, sin, 0} of k_disc_angle
    };
    bool liveC = kb < cnt, liveN = kb + kKpPerWg < cnt;
    uint32_t pkC = 0, mtC = 0, pkN = 0, mtN = 0;
    float4 tgC = make_float4(0.f, 0.f, 0.f, 0.f), tgN = tgC;
    if (liveC) key_rec(kb, pkC, mtC, tgC);
    if (liveN && kKpGroups > 1) key_rec(kb + kKpPerWg, pkN, mtN, tgN);
    if (kKpGroups == 1) liveN = false;
    Staged S;
    if constexpr (!kSplit) fetch_disc(pkC, mtC, liveC, S);
    fetch_patch(pkC, mtC, liveC, S);
#pragma unroll
    for (int g = 0; g < kKpGroups; g++) {
        if (!__any(liveC)) break;                                         // (key-points of a half wave come in ascending k: nothing further)
        OD_STAMP(0);
        if constexpr (!kSplit) stage_disc(liveC, S);
        OD_STAMP(1);
        // the key-point after this one: its pixels travel while this one is computed (the disc behind this one's disc store, the patch behind
        // this one's patch store: the registers are free then); the one after that: its record
        const int k2 = kb + (g + 2) * kKpPerWg;
        const bool liveNN = g + 2 < kKpGroups && k2 < cnt;
        uint32_t pkNN = 0, mtNN = 0;
        float4 tgNN = make_float4(0.f, 0.f, 0.f, 0.f);
        if (liveNN) key_rec(k2, pkNN, mtNN, tgNN);
        if constexpr (!kSplit) if (g + 1 < kKpGroups) fetch_disc(pkN, mtN, liveN, S);
        OD_STAMP(2);
        float angle = tgC.x;
        if constexpr (!kSplit) if (liveC) angle = orientation(pkC);
        stage_patch(liveC, S);                                            // (the same LDS rows: the moments above have read the disc)
        if (g + 1 < kKpGroups) fetch_patch(pkN, mtN, liveN, S);
        if (liveC) describe(pkC, mtC, angle, tgC.y, tgC.z);
        OD_STAMP(3);
        pkC = pkN; mtC = mtN; tgC = tgN; liveC = liveN;
        pkN = pkNN; mtN = mtNN; tgN = tgNN; liveN = liveNN;
    }
#ifdef RUMI_OD_STAMP
    if (threadIdx.x == 0 && (blockIdx.x % 8) == 0 && blockIdx.y == 0) printf("od wg %d: loop-head %lld stage(wait loads) %lld issue-next %lld | IC_Angle %lld trig %lld rBRIEF %lld store %lld\n", (int)blockIdx.x, st[0], st[1], st[2], st[4], st[5], st[6], st[3]);
#endif
}
// ------------------------------------------------------------------------------------------------
// IC_Angle and the trigonometry of a batch (orient_desc_split): one WAVE per key-point and round, 16 key-points per workgroup in four rounds,
// then ONE wave with a key-point per lane for fastAtan2 and the sinf / cosf restatement -- the same functions on the same moments as the fused
// kernel's, so the same bits.
//   Lanes 2r and 2r + 1 own row v = r - 15 of the disc: ONE 16-byte load each, of columns u = -15..0 and 1..16, straight from x - 15 (no
//   alignment: bytes inside the fused kernel's 36-byte row from (x - 15) & ~3), a load instruction per key-point and no byte shifts.  The
//   kernel is bound by what it fetches (a frame's whole un-blurred pyramid, 117 MB per 256 frames), not by its vector instructions (15.6 M):
//   78 us per 256 frames; with a row per lane and the fused kernel's three loads a row, one round in flight and 64 key-points a workgroup it
//   took 87 us (profiles/orient_split_*).
//   The bytes stay in registers: disc_chunk_moments (orb_math.h) takes the masked sum and the column-weighted one with v_dot4_u32_u8 against
//   the lane's two constant vectors.  The disc is symmetric (|u| <= umax[|v|]  <=>  |v| <= umax[|u|]), so the row formulation sums the same
//   pixels as the fused kernel's column one.  The bytes of the next three rounds are requested before this round's arithmetic.  Reads only the
//   un-blurred levels: it runs before the blur joins.
// ------------------------------------------------------------------------------------------------
// sum over the 64 lanes of a wave: half_wave_sum's DPP adds, then row_bcast:31 carries the lower half's total into the upper one
__device__ __forceinline__ int wave_sum_dpp(int v) {
    v += __builtin_amdgcn_update_dpp(0, v, 0x111, 0xF, 0xF, false);          // row_shr:1
    v += __builtin_amdgcn_update_dpp(0, v, 0x112, 0xF, 0xF, false);          // row_shr:2
    v += __builtin_amdgcn_update_dpp(0, v, 0x114, 0xF, 0xF, false);          // row_shr:4
    v += __builtin_amdgcn_update_dpp(0, v, 0x118, 0xF, 0xF, false);          // row_shr:8
    v += __builtin_amdgcn_update_dpp(0, v, 0x142, 0xA, 0xF, false);          // row_bcast:15 -> rows 1 and 3
    v += __builtin_amdgcn_update_dpp(0, v, 0x143, 0xC, 0xF, false);          // row_bcast:31 -> rows 2 and 3
    return __builtin_amdgcn_readlane(v, 63);
}
// 16 key-points a workgroup, as in the descriptor kernel: with 64 the workgroups resident on an XCD span fifteen frames instead of four, their
// pyramids no longer fit its L2 and the kernel fetches 194 MB per 256 frames (FETCH_SIZE) where the descriptor kernel fetches 122 MB
constexpr int kAngleKpPerWg = 16, kAngleWaves = 4, kAngleRounds = kAngleKpPerWg / kAngleWaves, kAngleAhead = 3;
__global__ __launch_bounds__(256) void k_disc_angle(const DevParams *__restrict__ P, ImgSrc src, const uint32_t *__restrict__ selPacked,
                                                    const uint32_t *__restrict__ selMeta, const int32_t *__restrict__ selCount, int selCap,
                                                    const uint4 *__restrict__ discVec, float4 *__restrict__ trig) {
    __shared__ int2 sLv[kMaxLevels];              // per level: offset and pitch of the un-blurred image (level 0 = the caller's frame)
    __shared__ int2 sMom[kAngleKpPerWg];          // {m01, m10} of the workgroup's key-points
    if (threadIdx.x < (unsigned)P->nlevels) {
        const DevLevel &Lv = P->lv[threadIdx.x];
        sLv[threadIdx.x] = threadIdx.x == 0 ? make_int2(0, src.l0Pitch) : make_int2((int)Lv.off, Lv.pitch);
    }
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const unsigned wg = xcd_swizzle(blockIdx.y * gridDim.x + blockIdx.x, gridDim.x * gridDim.y);   // a frame's key-points share one L2
    const int kbase = (wg % gridDim.x) * kAngleKpPerWg, frame = wg / gridDim.x;
    const int cnt = selCount[frame];
    if (kbase >= cnt) return;                                             // (the whole workgroup)
    __syncthreads();
    // lanes 62 and 63 are left over: they repeat row 15's loads with the zero vectors of table row 31
    const int r = lane >> 1, chunk = lane & 1, row = r < kPatchSize ? r : kPatchSize - 1;
    const uint4 w = discVec[r * 4 + chunk], m = discVec[r * 4 + kDiscRowChunks + chunk];
    const uint32_t W[kDiscChunkDwords] = {w.x, w.y, w.z, w.w}, M[kDiscChunkDwords] = {m.x, m.y, m.z, m.w};   // column weights u + 15 and the 0 / 1 mask, both inside the disc only
    struct __attribute__((packed)) Q16 { uint32_t x, y, z, w; };          // (a 16-byte load at any byte address)
    struct Chunk { uint32_t d[kDiscChunkDwords]; };
    const uint8_t *frame0 = src.l0 + (long long)frame * src.l0FrameStride, *framePyr = src.pyr + (long long)frame * P->arenaStride;
    const uint32_t *selP = selPacked + (long long)frame * selCap, *selM = selMeta + (long long)frame * selCap;
    // the records of the wave's four key-points in one load (lane j: round j's), so that no round's pixel load waits for a record load
    uint32_t pkL = 0, mtL = 0;
    if (lane < kAngleRounds && kbase + lane * kAngleWaves + wv < cnt) { pkL = selP[kbase + lane * kAngleWaves + wv]; mtL = selM[kbase + lane * kAngleWaves + wv]; }
    auto fetch = [&](int rd, Chunk &R) {                                  // (rd: a constant after unrolling; the record is wave-uniform)
        if (kbase + rd * kAngleWaves + wv >= cnt) return;
        const uint32_t pk = (uint32_t)__builtin_amdgcn_readlane((int)pkL, rd), meta = (uint32_t)__builtin_amdgcn_readlane((int)mtL, rd);
        const int level = meta & 0xFF, x = (int)(pk & 0xFFF) + kBorder, y = (int)((pk >> 12) & 0xFFF) + kBorder;
        const int2 lv = sLv[level];                                       // (a frame's arena is far below 2 GB: 32-bit offsets)
        const uint8_t *cr = (level == 0 ? frame0 : framePyr) + (lv.x + (y - kHalfPatch + row) * lv.y + (x - kHalfPatch) + 16 * chunk);
        const Q16 t = *reinterpret_cast<const Q16 *>(cr);
        R.d[0] = t.x; R.d[1] = t.y; R.d[2] = t.z; R.d[3] = t.w;
    };
    Chunk B[kAngleAhead + 1] = {};                                        // kAngleAhead rounds' bytes in flight behind the one being summed
#pragma unroll
    for (int rd = 0; rd < kAngleAhead; rd++) fetch(rd, B[rd]);
#pragma unroll
    for (int rd = 0; rd < kAngleRounds; rd++) {
        if (kbase + rd * kAngleWaves >= cnt) break;                       // (key-points come in ascending k: nothing further for the workgroup)
        if (rd + kAngleAhead < kAngleRounds) fetch(rd + kAngleAhead, B[(rd + kAngleAhead) % (kAngleAhead + 1)]);
        int m01, m10;
        disc_chunk_moments(B[rd % (kAngleAhead + 1)].d, W, M, r - kHalfPatch, m01, m10);
        m10 = wave_sum_dpp(m10);
        m01 = wave_sum_dpp(m01);
        if (lane == 0) sMom[rd * kAngleWaves + wv] = make_int2(m01, m10);
    }
    __syncthreads();
    const int k = kbase + (int)threadIdx.x;
    if (threadIdx.x < kAngleKpPerWg && k < cnt) {                         // wave 0: a key-point per lane
        const int2 mo = sMom[threadIdx.x];
        const float angle = fast_atan2_deg((float)mo.x, (float)mo.y);
        const float factorPI = (float)(3.1415926535897932384626433832795 / 180.f);
        const float ang = angle * factorPI;
        trig[(long long)frame * selCap + k] = make_float4(angle, cosf_glibc(ang), sinf_glibc(ang), 0.f);
    }
}
// ---- launch wrappers (called from orb_schedule.inc) ----
// trig: null = the fused kernel (the caller guarantees ceil(maxSel / 8) * nframes <= 2048 workgroups: !orient_desc_split), else the array
// launch_disc_angle has filled on the same stream
void launch_orient_desc(const DevParams *dP, ImgSrc src, const uint32_t *selPacked, const uint32_t *selMeta,
                        const int32_t *selCount, int selCap, int maxSel, RumiKeyPoint *kpOut, long long kpStride, uint8_t *descOut,
                        long long descStride, int outCap, int nframes, hipStream_t st, const float4 *trig) {
    if (maxSel <= 0) return;
    const int wg1 = (maxSel + kKpPerWg - 1) / kKpPerWg;
    const AssembleArgs none{};
    if (!trig)
        hipLaunchKernelGGL((k_orient_desc<1, false, false>), dim3(wg1, nframes), dim3(256), 0, st, dP, src, selPacked, selMeta, selCount, selCap, kpOut, kpStride, descOut,
                           descStride, outCap, none, trig);
    else
        hipLaunchKernelGGL((k_orient_desc<2, false, true>), dim3((wg1 + 1) / 2, nframes), dim3(256), 0, st, dP, src, selPacked, selMeta, selCount, selCap, kpOut, kpStride,
                           descOut, descStride, outCap, none, trig);
}
void launch_disc_angle(const DevParams *dP, ImgSrc src, const uint32_t *selPacked, const uint32_t *selMeta, const int32_t *selCount, int selCap,
                       int maxSel, const uint32_t *discVec, float4 *trig, int nframes, hipStream_t st) {
    if (maxSel <= 0) return;
    hipLaunchKernelGGL(k_disc_angle, dim3((maxSel + kAngleKpPerWg - 1) / kAngleKpPerWg, nframes), dim3(256), 0, st, dP, src, selPacked, selMeta, selCount, selCap,
                       reinterpret_cast<const uint4 *>(discVec), trig);
}
// k_assemble + k_orient_desc in ONE launch, for calls of a few frames (the caller guarantees (maxSel / 8) * nframes <= 2048 workgroups)
void launch_assemble_orient_desc(const DevParams *dP, ImgSrc src, const uint32_t *selLevel, const int32_t *selLevelCnt, int selLevelCap, int lap0, int lap1,
                                 int32_t *counts, long long countsStride, int32_t *errFlag, int32_t *errMirror, uint32_t *selPacked, uint32_t *selMeta,
                                 int32_t *selCount, int selCap, int maxSel, RumiKeyPoint *kpOut,
                                 long long kpStride, uint8_t *descOut, long long descStride, int outCap, int nframes, hipStream_t st) {
    if (maxSel <= 0) return;
    const int wg1 = (maxSel + kKpPerWg - 1) / kKpPerWg;
    const AssembleArgs A{selLevel, selLevelCnt, selLevelCap, lap0, lap1, counts, countsStride, errFlag, nframes == 1 ? errMirror : nullptr, selPacked, selMeta, selCount};
    hipLaunchKernelGGL((k_orient_desc<1, true, false>), dim3(wg1, nframes), dim3(256), 0, st, dP, src, (const uint32_t *)nullptr, (const uint32_t *)nullptr,
                       (const int32_t *)nullptr, selCap, kpOut, kpStride, descOut, descStride, outCap, A, (const float4 *)nullptr);
}

}  // namespace rumi
