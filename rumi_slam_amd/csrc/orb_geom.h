// Host-side geometry and constant tables of the ORB extractor (no device code here).
// Reference: R/lib_src/ORBextractor.cc:405-461 (constructor), :729-763 (cell grid), :1093-1112
// (level sizes); OpenCV 3.4 resize coefficient rule.
#pragma once
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <vector>

namespace rumi {

constexpr int kPatchSize = 31;
constexpr int kHalfPatch = 15;
constexpr int kEdge = 19;          // EDGE_THRESHOLD
constexpr int kBorder = kEdge - 3; // minBorderX/Y = 16
constexpr int kMaxLevels = 16;
constexpr int kCellTileMax = 96;   // largest FAST sub-image side the cell kernel stages in LDS
// No border is materialised around a level: the only reader outside a level is the 7x7 blur, which mirrors (BORDER_REFLECT_101) at the
// edges itself; the 19-px border of mvImagePyramid is synthesised on export (rumi_orb_pyramid_level).

inline int cv_round_host(double v) { return (int)std::lrint(v); }

// idx / d without an integer divide, for an index into a tile of at most 98 rows of d <= 98 elements (idx < 99 d):
// M = floor(2^20 / d) + 1, q = (idx * M) >> 20.  With M d = 2^20 + f, 0 < f <= d, and idx = q d + r:
// idx M = q 2^20 + (q f + r M) with q f + r M < 2^20 because q <= 98 and f <= d <= 98; idx M < 99 * 2^20 * 1.0001 < 2^32.
// Checked exhaustively by tests/test_hostcode_cpu.py through rumi_hook_magic_div.
#if defined(__HIPCC__)
#define RUMI_GEOM_HD __host__ __device__ inline
#else
#define RUMI_GEOM_HD inline
#endif
RUMI_GEOM_HD unsigned magic_of(unsigned d) { return (1u << 20) / d + 1u; }
RUMI_GEOM_HD int magic_div(int idx, unsigned M) { return (int)(((unsigned)idx * M) >> 20); }
// plain 32-bit products: v_mul_lo_u32 issues at the rate of v_mul_u32_u24 on gfx950 (both ~4.2 cycles per wave64 instruction, the slow class:
// profiles/r02_valu_issue_rates.txt, r06_valu_issue_rates_bytes.txt), and the 24-bit intrinsics cost an extra mask per operand where the
// compiler cannot prove the range (measured: +0.8 % instructions in k_fast_cells)
RUMI_GEOM_HD int mul24(int a, int b) { return a * b; }

struct LevelGeom {
    int w, h, pitch;            // level size, row pitch in bytes (64-B aligned)
    long long off;              // byte offset of the level's pixel (0,0) inside one frame's arena
    int nCols, nRows, wCell, hCell;
    int cellBase, nCells;       // first cell id of this level in the frame's cell list
    int maxBX, maxBY;           // w-16, h-16
    int nfeat;                  // mnFeaturesPerLevel
    float scale;                // mvScaleFactor
    int candBase;               // first slot of this level in the frame's worst-case candidate arena
    int candCap;
    int coefOff;                // offset (in int16 units) of this level's resize tables
};

struct OrbTables {
    int nlevels = 0;
    std::vector<float> scale, invScale, sigma2, invSigma2;
    std::vector<int> featuresPerLevel, umax;
};

// ORBextractor::ORBextractor, R/lib_src/ORBextractor.cc:405-461
inline OrbTables make_tables(int nfeatures, float scaleFactorArg, int nlevels) {
    OrbTables t;
    t.nlevels = nlevels;
    const double scaleFactor = scaleFactorArg;   // the member is a double initialised from the float arg
    t.scale.assign(nlevels, 1.f); t.sigma2.assign(nlevels, 1.f);
    t.invScale.resize(nlevels); t.invSigma2.resize(nlevels);
    for (int i = 1; i < nlevels; i++) {
        t.scale[i] = (float)(t.scale[i - 1] * scaleFactor);
        t.sigma2[i] = t.scale[i] * t.scale[i];
    }
    for (int i = 0; i < nlevels; i++) { t.invScale[i] = 1.0f / t.scale[i]; t.invSigma2[i] = 1.0f / t.sigma2[i]; }
    t.featuresPerLevel.assign(nlevels, 0);
    float factor = (float)(1.0f / scaleFactor);
    float want = (float)(nfeatures * (1 - factor) / (1 - (float)std::pow((double)factor, (double)nlevels)));
    int sum = 0;
    for (int l = 0; l < nlevels - 1; l++) {
        t.featuresPerLevel[l] = cv_round_host(want);
        sum += t.featuresPerLevel[l];
        want *= factor;
    }
    t.featuresPerLevel[nlevels - 1] = std::max(nfeatures - sum, 0);
    t.umax.assign(kHalfPatch + 1, 0);
    int vmax = (int)std::floor(kHalfPatch * std::sqrt(2.f) / 2 + 1);
    int vmin = (int)std::ceil(kHalfPatch * std::sqrt(2.f) / 2);
    const double hp2 = kHalfPatch * kHalfPatch;
    for (int v = 0; v <= vmax; ++v) t.umax[v] = cv_round_host(std::sqrt(hp2 - v * v));
    for (int v = kHalfPatch, v0 = 0; v >= vmin; --v) {
        while (t.umax[v0] == t.umax[v0 + 1]) ++v0;
        t.umax[v] = v0;
        ++v0;
    }
    return t;
}

// k_disc_angle's constant vectors (disc_chunk_moments, orb_math.h), from the umax table: row v = r - 15 of the disc, r = 0..30, gets 16 dwords
// at out[16 r]: eight of column weights (byte j = j where |j - 15| <= umax[|v|], else 0), eight of the mask (1 in the same bytes); a row's two lanes
// take a half of each.  Byte 31 and the whole of row 31 (the lanes left over) are zero.
constexpr int kDiscVecLanes = 32, kDiscVecLaneDwords = 16;
inline void make_disc_vectors(const int *umax, uint32_t *out) {
    std::fill(out, out + kDiscVecLanes * kDiscVecLaneDwords, 0u);
    for (int r = 0; r < kPatchSize; r++) {
        const int v = r - kHalfPatch, um = umax[v < 0 ? -v : v];
        for (int j = 0; j < kPatchSize; j++) {
            if (std::abs(j - kHalfPatch) > um) continue;
            out[r * kDiscVecLaneDwords + j / 4] |= (uint32_t)j << (8 * (j % 4));
            out[r * kDiscVecLaneDwords + 8 + j / 4] |= 1u << (8 * (j % 4));
        }
    }
}

// Level sizes (ComputePyramid :1095-1096) and FAST cell grids (:729-746) for a w x h frame.
// Returns false when a level is too small for the FAST cell loop or a cell exceeds the LDS tile.
inline bool make_geometry(const OrbTables &t, int w, int h, std::vector<LevelGeom> &g,
                          long long *arenaBytes, int *totalCells, int *totalCand, int *maxCellCand) {
    g.assign(t.nlevels, LevelGeom{});
    long long off = 0;
    int cells = 0, cand = 0, cellCand = 1;
    for (int l = 0; l < t.nlevels; l++) {
        LevelGeom &L = g[l];
        L.w = cv_round_host((float)w * t.invScale[l]);
        L.h = cv_round_host((float)h * t.invScale[l]);
        L.pitch = (L.w + 63) & ~63;
        L.off = off;
        off += (long long)L.pitch * L.h + 64;             // + slack: the resize reads 8-byte windows that may end a few bytes past a row
        L.maxBX = L.w - kBorder; L.maxBY = L.h - kBorder;
        const float width = (float)(L.maxBX - kBorder), height = (float)(L.maxBY - kBorder);
        L.nCols = (int)(width / 35.f); L.nRows = (int)(height / 35.f);
        if (L.nCols <= 0 || L.nRows <= 0) return false;      // the reference divides by zero here
        L.wCell = (int)std::ceil(width / L.nCols); L.hCell = (int)std::ceil(height / L.nRows);
        if (L.wCell + 6 > kCellTileMax || L.hCell + 6 > kCellTileMax) return false;
        L.cellBase = cells; L.nCells = L.nCols * L.nRows; cells += L.nCells;
        L.nfeat = t.featuresPerLevel[l];
        L.scale = t.scale[l];
        // NMS keeps at most one of any 2x2 block: worst case per level / per cell
        const int dw = L.maxBX - kBorder - 6, dh = L.maxBY - kBorder - 6;   // detection region
        L.candBase = cand;
        L.candCap = std::min(65535, std::max(1, ((dw + 1) / 2) * ((dh + 1) / 2)));   // u16 key ids in the quadtree
        cand += L.candCap;
        cellCand = std::max(cellCand, ((L.wCell + 1) / 2) * ((L.hCell + 1) / 2));
        L.coefOff = 0;
    }
    *arenaBytes = (off + 255) & ~255LL;
    *totalCells = cells; *totalCand = cand; *maxCellCand = cellCand;
    return true;
}

// ---- Lane packing of the batch launches of k_resize and k_blur ----
// Both kernels give a lane one dword (4 pixels) of a row and a wave one stretch of a row; a wave that hangs over the row's end issues its
// instructions for lanes that own nothing.  The row state (row index, source rows, vertical taps, mirrored rows) is the same for every frame
// of a launch, so the launch lays the same rows of G consecutive frames side by side: a group's row is G * lpr virtual lanes long, a wave
// takes 64 consecutive ones, and a lane derives (frame in group, dword column) once in its prologue.  Only a lane's ADDRESS depends on its
// frame.  k_resize: lpr = ceil(w / 4), a wave advances by 64 lanes (G = 1 is the mapping of a launch per frame).  k_blur: a frame's row gets
// one more column, the dword beyond the row's last one (all mirrored bytes: the right halo of the last producing lane), and a wave advances
// by 62: its lanes 0 and 63 repeat the neighbour waves' lanes and only hand their dword to lanes 1 and 62, so no lane fetches a halo dword
// from memory and a frame's seam may fall anywhere in a wave.
struct LanePack {
    int lpr;        // virtual lanes per frame row
    int halo;       // of these, the last `halo` (0 or 1) produce nothing
    int G;          // frames per group
    int step, lead; // a wave advances by `step` virtual lanes and starts `lead` lanes before its first producing one (64, 0 or 62, 1)
    int waves;      // waves along a group's row
    unsigned M;     // floor(2^32 / lpr) + 1: v / lpr == (v * M) >> 32 while v * lpr < 2^32
};
struct LaneSlot {
    int frame, col; // frame inside the group, dword column inside the frame's row (col == lpr - 1 with halo: the mirrored dword)
    bool live;      // the lane maps into the group (frame < G)
    bool produce;   // ... and stores its column
    bool first;     // col == 0: the left neighbour lane belongs to another frame
    bool last;      // col == lpr - 1: the right neighbour lane belongs to another frame
};
RUMI_GEOM_HD int lane_pack_waves(int lpr, int G, int step) { return (G * lpr + step - 1) / step; }
RUMI_GEOM_HD LaneSlot lane_slot(const LanePack &K, int wave, int lane) {
    const int v = wave * K.step - K.lead + lane;
    const unsigned vv = v < 0 ? 0u : (unsigned)v;
    LaneSlot s;
    s.frame = (int)(((unsigned long long)vv * K.M) >> 32);
    s.col = (int)vv - s.frame * K.lpr;
    s.live = v >= 0 && s.frame < K.G;
    s.produce = s.live && lane >= K.lead && lane < K.lead + K.step && s.col < K.lpr - K.halo;
    s.first = s.col == 0;
    s.last = s.col == K.lpr - 1;
    return s;
}
// the lane's frame in a launch of `nframes` frames (group `group` of the launch), -1: beyond the group or the launch's last frame
RUMI_GEOM_HD int lane_frame(const LanePack &K, const LaneSlot &s, int group, int nframes) {
    const int f = group * K.G + s.frame;
    return s.live && f < nframes ? f : -1;
}
constexpr int kLanePackMaxG = 8;   // a handful of frames: neighbouring workgroups still share a frame's cache lines
// Frames per group for a launch of `nframes` frames: the G <= kLanePackMaxG with the fewest issued waves (the partial last group counted; ties
// go to the smaller G).  `spanBytes`: bytes from a frame to the next (the larger of source and destination, 0: not packable): the kernels add
// the frame to a 32-bit per-lane offset against the base of the group's first frame, so a group's span must fit.
inline LanePack lane_pack_choose(int lpr, int halo, int step, int lead, int nframes, int maxG, long long spanBytes) {
    LanePack K{lpr, halo, 1, step, lead, lane_pack_waves(lpr, 1, step), (unsigned)((1ull << 32) / (unsigned)lpr) + 1u};
    long long best = (long long)nframes * K.waves;
    for (int G = 2; G <= std::min(std::min(maxG, kLanePackMaxG), nframes); G++) {
        if (spanBytes <= 0 || (long long)G * spanBytes >= (1ll << 31)) break;
        if (((long long)G * lpr + 64) * lpr >= (1ll << 32)) break;
        const int waves = lane_pack_waves(lpr, G, step);
        const long long issued = (long long)((nframes + G - 1) / G) * waves;
        if (issued < best) { best = issued; K.G = G; K.waves = waves; }
    }
    return K;
}
RUMI_GEOM_HD int resize_lanes_per_row(int w) { return (w + 3) >> 2; }
RUMI_GEOM_HD int blur_lanes_per_row(int w) { return ((w + 3) >> 2) + 1; }
constexpr int kPackMinFrames = 16;   // launches of fewer frames keep a launch per frame (G = 1) and the strip blur: they do not fill the device
inline LanePack resize_pack_of(int w, int nframes, long long spanBytes) {
    return lane_pack_choose(resize_lanes_per_row(w), 0, 64, 0, nframes, nframes >= kPackMinFrames ? kLanePackMaxG : 1, spanBytes);
}
inline LanePack blur_pack_of(int w, int nframes, long long spanBytes) {
    return lane_pack_choose(blur_lanes_per_row(w), 1, 62, 1, nframes, kLanePackMaxG, spanBytes);
}

// Stream plan of the resident queue.  A process has `hwQueues` hardware queues (GPU_MAX_HW_QUEUES, 4 unless set) and a hardware queue runs its
// packets in order whichever stream they came from, so streams beyond the queues do not add concurrency: they couple unrelated slots (a slot's
// blur stream lands on the queue of ANOTHER slot's main stream and waits behind its kernels).  The plan drives
//   streams = min(requestedSlots, max(2, hwQueues - reserve))
// slot streams, and runs a slot's blur on the slot's own stream (`blurInline`) whenever slot + blur streams + reserve would not fit the queues.
// reserve: queues left to the caller's stream (the matcher); kStreamReserve is the measured choice.
constexpr int kStreamReserve = 1;
constexpr int kDefaultHwQueues = 4;
struct StreamPlan { int streams; bool blurInline; };
inline StreamPlan stream_plan(int requestedSlots, int hwQueues, int reserve = kStreamReserve) {
    const int streams = std::min(requestedSlots, std::max(2, hwQueues - reserve));
    return StreamPlan{streams, 2 * streams + reserve > hwQueues};
}
// GPU_MAX_HW_QUEUES as the runtime reads it: a positive decimal integer; unset (null) or anything else = the default of 4
inline int parse_hw_queues(const char *v) {
    if (!v || !*v) return kDefaultHwQueues;
    char *end = nullptr;
    const long q = std::strtol(v, &end, 10);
    return (*end || q < 1 || q > 4096) ? kDefaultHwQueues : (int)q;
}
// ... read once per process; the library only reads the variable
inline int hw_queues_env() {
    static const int q = parse_hw_queues(std::getenv("GPU_MAX_HW_QUEUES"));
    return q;
}

// cv::resize INTER_LINEAR 8UC1 coefficient tables for one axis: ofs[d] and the two 11-bit taps.
// Horizontal axis (clampX = true): the source index is clamped and the tap zeroed as cv does, and
// `maxOut` receives xmax (first destination index whose second tap would fall outside the source:
// from there on the row pass emits S[sx]*2048).  Vertical axis (clampX = false): cv keeps the raw
// index and fractional tap and clips the two ROW indices when it fetches them, so we do the same.
inline void make_resize_axis(int srcN, int dstN, bool clampX, std::vector<int16_t> &ofs,
                             std::vector<int16_t> &taps, int *maxOut) {
    const double inv = (double)dstN / srcN, scale = 1. / inv;
    ofs.resize(dstN); taps.resize(dstN * 2);
    int dmax = dstN;
    for (int d = 0; d < dstN; d++) {
        float f = (float)((d + 0.5) * scale - 0.5);
        int s = (int)std::floor(f);
        f -= s;
        if (clampX) {
            if (s < 0) { f = 0; s = 0; }
            if (s + 1 >= srcN) {
                dmax = std::min(dmax, d);
                if (s >= srcN - 1) { f = 0; s = srcN - 1; }
            }
        }
        ofs[d] = (int16_t)s;
        taps[d * 2] = (int16_t)cv_round_host((1.f - f) * 2048.f);
        taps[d * 2 + 1] = (int16_t)cv_round_host(f * 2048.f);
    }
    *maxOut = dmax;
}

}  // namespace rumi
