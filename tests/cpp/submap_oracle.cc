// Scalar oracle for rumi_submap_match (include/rumi_match.h): the key-point match of CloudMerging::ComputeSubmapSim3 (R/lib_src/CloudMerging.cc:503-551)
// over key-frames that keep their grid the way the reference does, as one vector of key-point indices per cell.  TEST INFRASTRUCTURE, compiled by
// tests/submap_scene.py with -ffp-contract=off.
//
//   grid        Frame::AssignFeaturesToGrid / PosInGrid (Frame.cc:441-466, :752-761): key-points in index order, cell = round((un - min) * inv),
//               dropped when the cell lies outside 64 x 48
//   in_area     KeyFrame::GetFeaturesInArea (KeyFrame.cc:887-925), mono: cell bounds by floor / ceil, four early returns, columns outside rows
//               inside, the gate |dx| < r && |dy| < r on the undistorted point
//   match       :517-544: running best that starts at the tolerance, strict <, both slots must hold a map point
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <utility>
#include <vector>

namespace {

constexpr int kCols = 64, kRows = 48;

struct KeyFrameS {
    int n = 0;
    const float *keys = nullptr, *un = nullptr;     // mvKeys, mvKeysUn: n x 2
    const uint8_t *hasMp = nullptr;
    float minX = 0, minY = 0, wInv = 0, hInv = 0;
    std::vector<std::vector<std::vector<size_t>>> grid;

    void assign_to_grid() {
        grid.assign(kCols, std::vector<std::vector<size_t>>(kRows));
        for (int i = 0; i < n; i++) {
            const int px = (int)std::round((un[2 * i] - minX) * wInv);
            const int py = (int)std::round((un[2 * i + 1] - minY) * hInv);
            if (px < 0 || px >= kCols || py < 0 || py >= kRows) continue;
            grid[px][py].push_back((size_t)i);
        }
    }

    std::vector<size_t> in_area(float x, float y, float r) const {
        std::vector<size_t> found;
        const int cx0 = std::max(0, (int)std::floor((x - minX - r) * wInv));
        if (cx0 >= kCols) return found;
        const int cx1 = std::min(kCols - 1, (int)std::ceil((x - minX + r) * wInv));
        if (cx1 < 0) return found;
        const int cy0 = std::max(0, (int)std::floor((y - minY - r) * hInv));
        if (cy0 >= kRows) return found;
        const int cy1 = std::min(kRows - 1, (int)std::ceil((y - minY + r) * hInv));
        if (cy1 < 0) return found;
        for (int cx = cx0; cx <= cx1; cx++)
            for (int cy = cy0; cy <= cy1; cy++)
                for (size_t j : grid[cx][cy]) {
                    const float dx = un[2 * j] - x, dy = un[2 * j + 1] - y;
                    if (std::fabs(dx) < r && std::fabs(dy) < r) found.push_back(j);
                }
        return found;
    }
};

}  // namespace

// frame f: key-points frame_start[f] .. frame_start[f + 1] of keys / keys_un / has_mp, bounds[4 f] = min_x, min_y, grid_w_inv, grid_h_inv.
// Outputs as rumi_submap_match's.  Returns the total number of matches.
extern "C" int smo_submap_match(int32_t n_frames, const int32_t *frame_start, const float *keys, const float *keys_un, const uint8_t *has_mp,
                                const float *bounds, int32_t n_pairs, const int32_t *pair_f1, const int32_t *pair_f2, float tolerance,
                                int32_t *best2, int32_t *pair_start, int32_t *matches) {
    std::vector<KeyFrameS> kf(n_frames);
    for (int f = 0; f < n_frames; f++) {
        KeyFrameS &K = kf[f];
        const size_t o = (size_t)frame_start[f];
        K.n = frame_start[f + 1] - frame_start[f];
        K.keys = keys + 2 * o; K.un = keys_un + 2 * o; K.hasMp = has_mp + o;
        K.minX = bounds[4 * f]; K.minY = bounds[4 * f + 1]; K.wInv = bounds[4 * f + 2]; K.hInv = bounds[4 * f + 3];
        K.assign_to_grid();
    }
    int total = 0;
    size_t q = 0;
    for (int p = 0; p < n_pairs; p++) {
        const KeyFrameS &A = kf[pair_f1[p]], &B = kf[pair_f2[p]];
        pair_start[p] = total;
        for (int i1 = 0; i1 < A.n; i1++) {
            best2[q + i1] = -1;
            const float u1 = A.keys[2 * i1], v1 = A.keys[2 * i1 + 1];
            const std::vector<size_t> cand = B.in_area(u1, v1, tolerance);
            float nearest = tolerance;
            int kept = -1;
            for (size_t i2 : cand) {
                const float u2 = B.keys[2 * i2], v2 = B.keys[2 * i2 + 1];
                const float dist = (float)std::sqrt(std::pow(u1 - u2, 2) + std::pow(v1 - v2, 2));     // float differences, the rest in double
                if (dist < nearest && A.hasMp[i1] && B.hasMp[i2]) { kept = (int)i2; nearest = dist; }
            }
            if (kept < 0) continue;
            best2[q + i1] = kept;
            matches[2 * total] = i1; matches[2 * total + 1] = kept;
            total++;
        }
        q += (size_t)A.n;
    }
    pair_start[n_pairs] = total;
    return total;
}
