/*
 * rumi_testhooks.h — host-only entry points of librumi_hip.so that expose, for CPU tests, the pieces of
 * product code that are shared between host and device builds (the same source compiles both ways):
 * the replay of libstdc++'s std::sort used by the quadtree, the array quadtree itself, and the scalar
 * math of orb_math.h.  None of these touch a GPU; none is used by the reference-facing API.
 */
#ifndef RUMI_TESTHOOKS_H
#define RUMI_TESTHOOKS_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* Sort (key, id) pairs exactly as std::sort(first,last,compareNodes) of libstdc++ would
 * (ORBextractor.cc:524-536,658); ids are permuted in place alongside keys. */
int rumi_hook_sort_like_std(uint32_t *keys, uint16_t *ids, int32_t n);
/* The same through the workgroup-parallel replay on the GPU (n <= 4096; needs a device) and through the real std::sort. */
int rumi_hook_sort_device(uint32_t *keys, uint16_t *ids, int32_t n);
int rumi_hook_std_sort(uint32_t *keys, uint16_t *ids, int32_t n);

/* DistributeOctTree (ORBextractor.cc:538-724) on packed candidates x | y<<12 | score<<24 (coordinates
 * relative to (minX,minY)); writes indices into `cand` in the reference's result order. */
int rumi_hook_quadtree(const uint32_t *cand, int32_t n, int32_t minX, int32_t maxX, int32_t minY, int32_t maxY,
                       int32_t N, int32_t *out_idx, int32_t cap, int32_t *n_out);

/* The coordinate tables of the batch quadtree (orb_octree.h: the per-coordinate halves of a key's depth-D path, built on the host by the rule the
 * kernels share) for `level` of a w x h frame: info[6] = {W, H of the level's key-point area, roots, table depth D, cells of depth D (0: the
 * level has no tables), features wanted on the level}; bins = the x half (W + 1 entries: root << 2 D | bit 2 (D - 1 - d) = right side taken
 * at depth d), then the y half (H + 1 entries: bit 2 (D - 1 - d) + 1 = lower side); n_out = entries (RUMI_E_CAPACITY if > cap). */
int rumi_hook_octree_bins(int32_t w, int32_t h, int32_t nfeatures, float scale, int32_t nlevels, int32_t level, int32_t *info, uint16_t *bins,
                          int32_t cap, int32_t *n_out);

/* k_compact's LDS for the batch quadtree of a w x h geometry: info[4] = {FAST cells of a frame (the kernel's prefix has one dword more),
 * depth-D cells of a frame's histogram row (every level's count rounded up to even), bytes of the kernel's count table in LDS -- 0 when
 * prefix + table + static LDS would pass the 64 KiB a launch gets without an opt-in: such a geometry keeps the one-launch quadtree --, the
 * bound on the kernel's static LDS the rule uses}. */
int rumi_hook_compact_hist_lds(int32_t w, int32_t h, int32_t nfeatures, float scale, int32_t nlevels, int32_t *info);

float rumi_hook_sinf(float x);           /* restated glibc sinf  (orb_math.h) */
float rumi_hook_cosf(float x);           /* restated glibc cosf  (orb_math.h) */
float rumi_hook_fast_atan2(float y, float x);   /* cv::fastAtan2, degrees */
int rumi_hook_cv_round(float v);         /* cvRound */
int rumi_hook_magic_div(int32_t idx, int32_t d);   /* divide-free idx / d used by the FAST cell kernel (orb_geom.h) */

/* IC_Angle (ORBextractor.cc:73-97) as k_disc_angle computes it: rows = 31 rows of 36 bytes of the level from (x - 15) & ~3 on, so column u = -15 of
 * the disc sits in byte s = (x - 15) & 3 = 0..3 of a row; the kernel's two lanes of a row load the 2 x 16 bytes from there.  umax16 = the
 * extractor's umax table.  m01 / m10: the moments, by the kernel's own chunk function (orb_math.h) summed over the rows.  W / M (31 x 8 dwords
 * each, may be null): the per-row weight and mask vectors the launch code builds from umax16 (orb_geom.h). */
int rumi_hook_disc_moments(const uint8_t *rows, int32_t s, const int32_t *umax16, int32_t *m01, int32_t *m10, uint32_t *W, uint32_t *M);

/* Lane packing of the batch launches (orb_geom.h: LanePack / lane_slot, the code the kernels and the launch wrappers use): for a w x h frame,
 * the pyramid rule (scale, nlevels) and a launch of nframes frames, the mapping of every lane of kernel 0 = the resize launch that writes `level`
 * (1 .. nlevels - 1) or kernel 1 = the batch blur's part for `level` (0 .. nlevels - 1).  force_g = 0: the frames per group the launch code
 * picks; > 0: that many.  info[8] = {level width, lanes per frame row, G, waves per group row, groups, lanes a wave advances by, non-producing
 * columns at the row's end, level height}.  slots: groups x waves x 64 entries of {frame (-1: the lane maps to no frame), dword column, flags}
 * with flags 1 = produces, 2 = first dword of its frame's row, 4 = last column of its frame's row; n_out = entries (RUMI_E_CAPACITY if > cap). */
int rumi_hook_lane_packing(int32_t w, int32_t h, float scale, int32_t nlevels, int32_t nframes, int32_t kernel, int32_t level, int32_t force_g,
                           int32_t *info, int32_t *slots, int32_t cap, int32_t *n_out);

/* Stream plan of the resident queue (orb_geom.h: stream_plan, what rumi_orb_set_resident_queue asks): for requested_slots slots and hw_queues
 * hardware queues (<= 0: GPU_MAX_HW_QUEUES as the library read it, 4 when unset or unparsable), the slot streams it drives and whether a
 * slot's blur runs on the slot's own stream; reserve (may be null) = the queues the rule leaves to the caller's stream.
 * rumi_hook_parse_hw_queues: the library's reading of a GPU_MAX_HW_QUEUES value (null = unset). */
int rumi_hook_stream_plan(int32_t requested_slots, int32_t hw_queues, int32_t *streams, int32_t *blur_inline, int32_t *reserve);
int rumi_hook_parse_hw_queues(const char *value);

/* Stages 1 + 3 of the last rumi_create_new_map_points call on this matcher (rumi_mapping.h; needs a device): per neighbour k and feature i1 of
 * the current key-frame, matches[k * n1 + i1] = the neighbour's feature SearchForTriangulation pairs it with when the loop reaches neighbour k
 * (after the rotation histogram, before the triangulation gates), -1 = none.  n_neigh and n1 must be those of that call.  The call itself does
 * not record this: the hook runs the replay kernel once more on the state the call left on the device. */
struct RumiMatcher;
int rumi_hook_newpts_matches(struct RumiMatcher *m, int32_t n_neigh, int32_t n1, int32_t *matches);

/* The 64-byte attribute records of n points of a covisibility store (rumi_covis.h: position, normal, min and max distance, descriptor), from
 * the device copy (from_device != 0; waits for the device) or from the host mirror.  Uploads nothing: staged edits stay staged.
 * RUMI_E_INVALID for an id outside the store or when that side holds no attribute table yet.  For the write-back tests of
 * rumi_refresh_map_points_resident. */
struct RumiCovis;
int rumi_hook_covis_read_attributes(struct RumiCovis *c, int32_t n, const int32_t *ids, uint8_t *out, int32_t from_device);

/* What the host mirror of a covisibility store holds for a live slot, staged edits included: its map-point row (row_length entries, cap at least
 * that), per entry the bad bit of its point (0 for a NULL entry) and the key-frame's bad bit.  Uploads nothing.  For the tests that fill a store
 * from a scene (rumi_common_regions_bow_resident). */
int rumi_hook_covis_read_row(struct RumiCovis *c, int32_t slot, int32_t cap, int32_t *row, uint8_t *point_bad, int32_t *kf_bad);

/* What a covisibility store holds of rumi_covis_set_keyframe_poses and rumi_covis_set_point_maps, from the device copy (from_device != 0; waits
 * for the device) or from the host mirror, staged edits included there.  Uploads nothing.  pose8 [n_kf][8] doubles and has_pose [n_kf] of the
 * slots (zeros where the table does not exist yet); map_id [n_pt] and has_map [n_pt] of the points.  For the tests of rumi_local_ba_resident. */
int rumi_hook_covis_read_poses(struct RumiCovis *c, int32_t n_kf, const int32_t *slots, double *pose8, int32_t *has_pose, int32_t n_pt,
                               const int32_t *ids, int32_t *map_id, int32_t *has_map, int32_t from_device);

/* The chunk length of rumi_submap_sim3_ransac on this optimiser (rumi_opt.h): iterations of the stream enqueued between two read-backs of the
 * rule's state.  0 = the library's default; a length at or above the sum of the solvers' iterations runs the call as one chunk.  Results do not
 * depend on it; the tests put chunk edges on solver boundaries and on the converging iteration. */
struct RumiOptimizer;
int rumi_hook_submap_sim3_set_chunk(struct RumiOptimizer *o, int32_t chunk);

#ifdef __cplusplus
}
#endif
#endif
