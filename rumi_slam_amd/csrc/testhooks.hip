// Host-only test hooks (include/rumi_testhooks.h): the host compilation of code the kernels share.
#include <hip/hip_runtime.h>

#include <vector>

#include "orb_geom.h"
#include "orb_math.h"
#include "orb_octree.h"
#include "rumi_orb.h"
#include <algorithm>
#include <utility>
#include <vector>

#include "rumi_testhooks.h"

using namespace rumi;

extern "C" int rumi_hook_sort_like_std(uint32_t *keys, uint16_t *ids, int32_t n) {
    if (n < 0 || (n > 0 && (!keys || !ids))) return RUMI_E_INVALID;
    std::vector<OctEntry> e((size_t)n);
    for (int i = 0; i < n; i++) e[i] = OctEntry{keys[i], ids[i], 0};
    sort_like_libstdcxx(e.data(), n);
    for (int i = 0; i < n; i++) { keys[i] = e[i].key; ids[i] = e[i].id; }
    return RUMI_OK;
}

namespace rumi { int launch_sort_hook(uint32_t *keys, uint16_t *ids, int n); }
// the same entries through the workgroup-parallel replay on the GPU (orb_octree_kernel.hip)
extern "C" int rumi_hook_sort_device(uint32_t *keys, uint16_t *ids, int32_t n) { return rumi::launch_sort_hook(keys, ids, n); }
// ... and through the real std::sort of the libstdc++ this library is built against (what the reference's compareNodes sort does)
extern "C" int rumi_hook_std_sort(uint32_t *keys, uint16_t *ids, int32_t n) {
    if (n < 0) return -1;
    std::vector<std::pair<uint32_t, uint16_t>> v(n);
    for (int i = 0; i < n; i++) v[i] = {keys[i], ids[i]};
    std::sort(v.begin(), v.end(), [](const std::pair<uint32_t, uint16_t> &a, const std::pair<uint32_t, uint16_t> &b) { return a.first < b.first; });
    for (int i = 0; i < n; i++) { keys[i] = v[i].first; ids[i] = v[i].second; }
    return 0;
}

extern "C" int rumi_hook_quadtree(const uint32_t *cand, int32_t n, int32_t minX, int32_t maxX, int32_t minY,
                                  int32_t maxY, int32_t N, int32_t *out_idx, int32_t cap, int32_t *n_out) {
    if (!n_out || n < 0 || n > 65535 || maxX <= minX || maxY <= minY) return RUMI_E_INVALID;
    std::vector<int> out;
    int m = octree_host(cand, n, minX, maxX, minY, maxY, N, out);
    if (m < 0) return RUMI_E_INVALID;
    *n_out = m;
    if (m > cap) return RUMI_E_CAPACITY;
    for (int i = 0; i < m; i++) out_idx[i] = out[i];
    return RUMI_OK;
}

// the batch quadtree's coordinate tables of one level, by the functions set_geometry builds them with (oct_level_tabs, oct_make_bins)
extern "C" int rumi_hook_octree_bins(int32_t w, int32_t h, int32_t nfeatures, float scale, int32_t nlevels, int32_t level, int32_t *info,
                                     uint16_t *bins, int32_t cap, int32_t *n_out) {
    if (!info || !n_out || nfeatures < 1 || nlevels < 1 || nlevels > kMaxLevels || level < 0 || level >= nlevels) return RUMI_E_INVALID;
    const OrbTables t = make_tables(nfeatures, scale, nlevels);
    std::vector<LevelGeom> g;
    long long arena = 0;
    int cells, cand, cellCand;
    if (!make_geometry(t, w, h, g, &arena, &cells, &cand, &cellCand)) return RUMI_E_INVALID;
    const int W = g[level].maxBX - kBorder, Hh = g[level].maxBY - kBorder;
    const OctLevelTabs T = oct_level_tabs(W, Hh, g[level].nfeat);
    const int32_t inf[6] = {W, Hh, T.nIni, T.D, T.cells, g[level].nfeat};
    std::copy(inf, inf + 6, info);
    *n_out = T.cells ? W + 1 + Hh + 1 : 0;
    if (*n_out > cap || (*n_out && !bins)) return RUMI_E_CAPACITY;
    if (T.cells) oct_make_bins(W, Hh, T, bins);
    return RUMI_OK;
}

// k_compact's LDS sizing for the batch quadtree of a geometry, by the functions set_geometry and launch_compact use (oct_row_entries, oct_hist_lds_bytes)
extern "C" int rumi_hook_compact_hist_lds(int32_t w, int32_t h, int32_t nfeatures, float scale, int32_t nlevels, int32_t *info) {
    if (!info || nfeatures < 1 || nlevels < 1 || nlevels > kMaxLevels) return RUMI_E_INVALID;
    const OrbTables t = make_tables(nfeatures, scale, nlevels);
    std::vector<LevelGeom> g;
    long long arena = 0;
    int cells, cand, cellCand;
    if (!make_geometry(t, w, h, g, &arena, &cells, &cand, &cellCand)) return RUMI_E_INVALID;
    int row = 0;
    for (int l = 0; l < nlevels; l++) row += oct_row_entries(oct_level_tabs(g[l].maxBX - kBorder, g[l].maxBY - kBorder, g[l].nfeat).cells);
    info[0] = cells; info[1] = row; info[2] = oct_hist_lds_bytes(cells, row); info[3] = kCompactStaticLds;
    return RUMI_OK;
}

extern "C" float rumi_hook_sinf(float x) { return sinf_glibc(x); }
extern "C" float rumi_hook_cosf(float x) { return cosf_glibc(x); }
extern "C" float rumi_hook_fast_atan2(float y, float x) { return fast_atan2_deg(y, x); }
extern "C" int rumi_hook_cv_round(float v) { return cv_round_f(v); }
extern "C" int rumi_hook_magic_div(int32_t idx, int32_t d) { return magic_div(idx, magic_of((unsigned)d)); }

// IC_Angle by rows: the vectors the launch code builds from umax and the kernel's own chunk function (disc_chunk_moments) on the 2 x 16 bytes a
// row's two lanes load from byte s of the staged row on, summed over the 31 rows
extern "C" int rumi_hook_disc_moments(const uint8_t *rows, int32_t s, const int32_t *umax16, int32_t *m01, int32_t *m10, uint32_t *W, uint32_t *M) {
    if (!rows || !umax16 || !m01 || !m10 || s < 0 || s > 3) return RUMI_E_INVALID;
    for (int i = 0; i <= kHalfPatch; i++) if (umax16[i] < 0 || umax16[i] > kHalfPatch) return RUMI_E_INVALID;
    uint32_t vec[kDiscVecLanes * kDiscVecLaneDwords];
    make_disc_vectors(umax16, vec);
    int s01 = 0, s10 = 0;
    for (int r = 0; r < kPatchSize; r++) {
        const uint32_t *w = vec + r * kDiscVecLaneDwords, *m = w + kDiscRowChunks * kDiscChunkDwords;
        for (int c = 0; c < kDiscRowChunks; c++) {
            uint32_t d[kDiscChunkDwords];
            std::memcpy(d, rows + r * 36 + s + 16 * c, sizeof d);
            int a, b;
            disc_chunk_moments(d, w + c * kDiscChunkDwords, m + c * kDiscChunkDwords, r - kHalfPatch, a, b);
            s01 += a; s10 += b;
        }
        if (W) std::copy(w, w + 8, W + r * 8);
        if (M) std::copy(m, m + 8, M + r * 8);
    }
    *m01 = s01; *m10 = s10;
    return RUMI_OK;
}

// the lane packing of the batch resize / blur launches: the launch code's choice of G and the kernels' lane_slot, evaluated on the host
extern "C" int rumi_hook_lane_packing(int32_t w, int32_t h, float scale, int32_t nlevels, int32_t nframes, int32_t kernel, int32_t level,
                                      int32_t force_g, int32_t *info, int32_t *slots, int32_t cap, int32_t *n_out) {
    if (!info || !n_out || nframes < 1 || nlevels < 1 || nlevels > kMaxLevels || kernel < 0 || kernel > 1 || level < (kernel ? 0 : 1) || level >= nlevels ||
        force_g < 0 || force_g > nframes)
        return RUMI_E_INVALID;
    const OrbTables t = make_tables(1000, scale, nlevels);
    std::vector<LevelGeom> g;
    long long arena = 0;
    int cells, cand, cellCand;
    if (!make_geometry(t, w, h, g, &arena, &cells, &cand, &cellCand)) return RUMI_E_INVALID;
    const long long span = std::max(arena, (long long)w * h);
    LanePack K = kernel ? blur_pack_of(g[level].w, nframes, span) : resize_pack_of(g[level].w, nframes, span);
    if (force_g) { K.G = force_g; K.waves = lane_pack_waves(K.lpr, K.G, K.step); }
    const int groups = (nframes + K.G - 1) / K.G;
    const int32_t inf[8] = {g[level].w, K.lpr, K.G, K.waves, groups, K.step, K.halo, g[level].h};
    std::copy(inf, inf + 8, info);
    const long long n = (long long)groups * K.waves * 64;
    *n_out = (int32_t)std::min<long long>(n, INT32_MAX);
    if (n > cap || !slots) return RUMI_E_CAPACITY;
    int32_t *o = slots;
    for (int grp = 0; grp < groups; grp++)
        for (int wv = 0; wv < K.waves; wv++)
            for (int lane = 0; lane < 64; lane++, o += 3) {
                const LaneSlot s = lane_slot(K, wv, lane);
                const int f = lane_frame(K, s, grp, nframes);
                o[0] = f; o[1] = s.col; o[2] = (f >= 0 && s.produce ? 1 : 0) | (s.first ? 2 : 0) | (s.last ? 4 : 0);
            }
    return RUMI_OK;
}

// the stream plan of the resident queue (orb_geom.h: stream_plan, the function rumi_orb_set_resident_queue asks)
extern "C" int rumi_hook_stream_plan(int32_t requested_slots, int32_t hw_queues, int32_t *streams, int32_t *blur_inline, int32_t *reserve) {
    if (!streams || !blur_inline || requested_slots < 1) return RUMI_E_INVALID;
    const StreamPlan p = stream_plan(requested_slots, hw_queues > 0 ? hw_queues : hw_queues_env());
    *streams = p.streams; *blur_inline = p.blurInline ? 1 : 0;
    if (reserve) *reserve = kStreamReserve;
    return RUMI_OK;
}
extern "C" int rumi_hook_parse_hw_queues(const char *value) { return parse_hw_queues(value); }
