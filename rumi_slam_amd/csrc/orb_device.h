// Device-visible parameter blocks of the ORB extractor and the kernel launch wrappers.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "orb_geom.h"
#include "rumi_orb.h"

namespace rumi {

struct DevLevel {
    int w, h, pitch;
    long long off;                 // byte offset of the level in a frame's arena (pyramid and blur arenas alike)
    int nCols, nRows, wCell, hCell;
    int cellBase, nCells;
    int maxBX, maxBY;
    int nfeat;
    float scale;                   // mvScaleFactor[level]
    float patchSize;               // (float)(int)(31 * scale)  (ORBextractor.cc:816)
    int candCap;
    int coefX, coefXT, coefY, xmax; // resize tables (int16 units into the coefficient buffer): column offsets, column tap pairs, row tables;
                                   // the column tables carry 4 more entries than the level has columns (copies of the last one), so that the
                                   // lane holding the row's last, partial dword computes 4 outputs like every other lane
    int xmaxFast;                  // xmax, or w + 3 when no column clamps its second tap (then every lane's 4 outputs may take the fast path)
    int rowTab;                    // first entry of the level's output-row table (RowTap units, row 0 first)
    // batch quadtree (orb_octree.h: oct_level_tabs): the level's coordinate tables in the handle's table array (x half: W + 1 entries, then
    // the y half: H + 1), its cells of depth D in a frame's histogram / rank row (first entry: even; 0 cells: the level has no tables)
    int octBin, octCell, octCells;
};

struct DevParams {
    int nlevels, totalCells, maxCellCand, totalCand;
    int iniTh, minTh;
    long long arenaStride;         // bytes per frame in the pyramid / blur arenas
    int umax[16];
    int octCellStride;             // 16-bit entries per frame in OctNarrow::hist / rank (even); 0: this geometry has no batch pipeline -- the handle's arrays or k_compact's LDS have no room for its tables
    DevLevel lv[kMaxLevels];
};

// Where the kernels find pixels: level 0 IS the caller's frame (4-byte aligned base / pitch / frame stride; the host stages a frame
// that is not), levels 1.. live in `pyr`, the blurred levels (0 included) in `blur` with the same per-level offsets.  No borders anywhere.
struct ImgSrc {
    const uint8_t *l0;             // caller's frames = level 0
    long long l0FrameStride;
    int l0Pitch;
    uint8_t *pyr;
    uint8_t *blur;
};

struct RowTap { int32_t r0, r1; uint32_t bh0, bh1; };   // the two (clamped) source rows, vertical taps << 16
// The whole pyramid in ONE launch for calls of a few frames (k_pyramid_tiles): per workgroup and level the region it computes (multiples of 4 in x;
// level 0: the window of the caller's frame it reads), derived on the host from the resize tables
struct PyrTile { int16_t x0[kMaxLevels], x1[kMaxLevels], y0[kMaxLevels], y1[kMaxLevels]; };
void launch_pyramid_tiles(const DevParams *dP, ImgSrc src, const int16_t *coef, const RowTap *rowTab, const PyrTile *tiles, int ntiles, int bufBytes,
                          int tabEntries, int nframes, hipStream_t st, int32_t *clearWord = nullptr);
void launch_resize(const DevParams *dP, const DevParams &hP, ImgSrc src, const int16_t *coef, const RowTap *rowTab, int level, int nframes,
                   hipStream_t st, int32_t *clearWord = nullptr);
void launch_fast(const DevParams *dP, const DevParams &hP, ImgSrc src, uint32_t *cellBuf, int32_t *cellCnt, int nframes,
                 hipStream_t st);
bool fast_blur_fusable(const DevParams &hP);
bool launch_fast_blur(const DevParams *dP, const DevParams &hP, ImgSrc src, uint32_t *cellBuf, int32_t *cellCnt, int nframes, int variant, hipStream_t st);
// hist: the candidates are also counted by depth-D quadtree cell (OctNarrow::hist, through the coordinate tables `bins`); null: not
void launch_compact(const DevParams *dP, const DevParams &hP, const uint32_t *cellBuf, const int32_t *cellCnt,
                    uint32_t *cand, int32_t *levelStart, int32_t *errFlag, int nframes, hipStream_t st, uint32_t *hist, const uint16_t *bins);
void launch_blur(const DevParams *dP, const DevParams &hP, ImgSrc src, int nframes, int variant, hipStream_t st);
// Batches take IC_Angle and the trigonometry in a kernel of their own (launch_disc_angle) and the descriptor kernel without them; every call the
// fused kernel fills the device with keeps it.  THE rule, asked once per sub-chunk by the scheduler.
inline bool orient_desc_split(int maxSel, int nframes) { return (long long)((maxSel + 7) / 8) * nframes > 2048; }
// trig: null = the fused kernel; else the {angle, cos, sin, 0} array (indexed like selMeta) launch_disc_angle has filled on the same stream
void launch_orient_desc(const DevParams *dP, ImgSrc src, const uint32_t *selPacked, const uint32_t *selMeta,
                        const int32_t *selCount, int selCap, int maxSel, RumiKeyPoint *kpOut, long long kpStride, uint8_t *descOut,
                        long long descStride, int outCap, int nframes, hipStream_t st, const float4 *trig);   // strides: bytes from one frame's outputs to the next
// discVec: make_disc_vectors' table on the device.  Reads the un-blurred levels only.
void launch_disc_angle(const DevParams *dP, ImgSrc src, const uint32_t *selPacked, const uint32_t *selMeta, const int32_t *selCount, int selCap,
                       int maxSel, const uint32_t *discVec, float4 *trig, int nframes, hipStream_t st);

void launch_assemble_orient_desc(const DevParams *dP, ImgSrc src, const uint32_t *selLevel, const int32_t *selLevelCnt, int selLevelCap, int lap0, int lap1,
                                 int32_t *counts, long long countsStride, int32_t *errFlag, int32_t *errMirror, uint32_t *selPacked, uint32_t *selMeta,
                                 int32_t *selCount, int selCap, int maxSel, RumiKeyPoint *kpOut,
                                 long long kpStride, uint8_t *descOut, long long descStride, int outCap, int nframes, hipStream_t st);
// What the batch quadtree pipeline (orb_octree_kernel.hip) keeps for ONE scratch slot range, beside the tables of the geometry.  Per frame
// the depth-D cells of all levels lie side by side (DevLevel::octCell, DevParams::octCellStride), 16 bits a cell, two to a dword.
constexpr int kOctRedo = -1;       // in m: the tree went to k_octree_redo
struct OctNarrow {
    uint32_t *hist;                // [frames][octCellStride / 2] keys per cell: k_compact adds, k_octree_narrow reads and clears (zero between calls)
    uint32_t *rank;                // [frames][octCellStride / 2] cell -> rank of its node in the level's final list
    int32_t *m;                    // [frames][nlevels] length of that list, 0: the level has no keys, kOctRedo
    int32_t *redoList;             // [frames * nlevels] frame * kMaxLevels + level of the trees handed on
    int32_t *ctl;                  // {entries of redoList, workgroups of k_octree_redo that are done, -, -}: zero between launches
    int32_t *stat;                 // the handle's {trees k_octree_narrow finished, trees redone}, cumulative
    const uint16_t *bins;          // the geometry's coordinate tables (DevLevel::octBin)
};
struct OctLdsSizes { size_t wide, narrow, select; };   // dynamic LDS of k_octree / k_octree_redo, k_octree_narrow, k_oct_select
// which kernels a launch of nframes frames takes: 0 keys in registers, 1 keys in memory (one launch), 2 the batch pipeline -- launch_compact
// then counts the histogram it starts from
int octree_plan(const DevParams &hP, int nframes);
// Q: the slot range's blocks (used when octree_plan says pipeline)
void launch_octree(const DevParams *dP, const DevParams &hP, const uint32_t *cand, const int32_t *levelStart,
                   uint16_t *owner, uint32_t *selLevel, int32_t *selLevelCnt, int selLevelCap, int32_t *errFlag,
                   int nframes, const OctLdsSizes &lds, const OctNarrow &Q, hipStream_t st);
void launch_assemble(const DevParams *dP, const uint32_t *selLevel, const int32_t *selLevelCnt, int selLevelCap, int lap0,
                     int lap1, uint32_t *selPacked, uint32_t *selMeta, int32_t *selCount, int selCap, int32_t *counts, long long countsStride,
                     int32_t *errFlag, int nframes, hipStream_t st, int32_t *errMirror = nullptr);
OctLdsSizes octree_lds_for(const DevParams &hP, int selLevelCap);

}  // namespace rumi
