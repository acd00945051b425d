// The FeatureVector side of SearchByBoW (ORBmatcher.cc:203-300, :700-800), once for every kernel that walks two vectors node by node (match.hip,
// track.hip, mapping.hip): the twin of a node in the other vector, and the walk of one node pair by 16 lanes with the reference's tie rules.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "match_device.h"

namespace rumi {

// The place of node `id` among `nn` ascending node ids (std::map order: the merge-walk of two vectors visits exactly the ids present in both), -1: absent.
__device__ __forceinline__ int fv_find_node(const uint32_t *nodes, int nn, uint32_t id) {
    int lo = 0, hi = nn;
    while (lo < hi) { const int mid = (lo + hi) >> 1; if (nodes[mid] < id) lo = mid + 1; else hi = mid; }
    return lo < nn && nodes[lo] == id ? lo : -1;
}

// (best, second) over the 16 lanes of a group: best = the smallest (dist << 16 | position) key, so equal distances go to the earlier position;
// second = the second smallest DISTANCE of the union, the losing best of every exchange included.  Every lane ends with both.
__device__ __forceinline__ void bow_reduce16(uint32_t &best, uint32_t &second) {
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) {
        const uint32_t ob = __shfl_xor(best, o, 16), os = __shfl_xor(second, o, 16);
        const uint32_t loser = max(best, ob) >> 16;
        best = min(best, ob);
        second = min(min(second, os), loser);
    }
}

// Where a lane keeps "my candidate at position lane + 16 j is taken".  One register: nodes of up to 512 candidates.  LDS words of the thread's own
// (word w at w[w * 256]): any size, and no lane reads another's word, so nothing to synchronise.
struct TakenMask {
    uint32_t m = 0;
    __device__ __forceinline__ bool test(int j) const { return (m >> j) & 1u; }
    __device__ __forceinline__ void set(int j) { m |= 1u << j; }
};
struct TakenLds {
    uint32_t *w;
    __device__ __forceinline__ bool test(int j) const { return (w[(j >> 5) * 256] >> (j & 31)) & 1u; }
    __device__ __forceinline__ void set(int j) { w[(j >> 5) * 256] |= 1u << (j & 31); }
};

// One node pair by the 16 lanes of a group (lane: this one's place).  The queries qIdx[p0 .. p1) go by in list order, uniform over the group; gate(i)
// says whether query feature i searches at all.  The lanes share out the nc candidates cIdx[0 .. nc) of the other side's node, skip the taken ones,
// and reduce their Hamming distances to (bestDist1, bestDist2) (:252-276).  A query that passes TH_LOW (STRICT: `<`, :757; else `<=`, :283) and the
// ratio test takes its candidate: the owner lane sets the taken bit, lane 0 calls accept(query feature, candidate feature).
template <bool STRICT, class Taken, class Gate, class Accept>
__device__ __forceinline__ void bow_node_walk(int lane, const uint32_t *qIdx, int p0, int p1, const uint32_t *qDesc, const uint32_t *cIdx, int nc,
                                              const uint32_t *cDesc, float nnratio, Taken &taken, Gate gate, Accept accept) {
    for (int p = p0; p < p1; p++) {
        const int iq = (int)qIdx[p];
        if (!gate(iq)) continue;
        uint32_t q[8];
#pragma unroll
        for (int w = 0; w < 8; w++) q[w] = qDesc[(size_t)iq * 8 + w];
        uint32_t best = (256u << 16) | 0xFFFFu, second = 256u;
        for (int j = 0, pos = lane; pos < nc; j++, pos += 16) {
            if (taken.test(j)) continue;
            const uint32_t dist = (uint32_t)hamming256(q, cDesc + (size_t)cIdx[pos] * 8);
            const uint32_t key = (dist << 16) | (uint32_t)pos;
            if (key < best) { second = best >> 16; best = key; }       // a strictly smaller distance (positions ascend inside a lane)
            else if (dist < second) second = dist;
        }
        bow_reduce16(best, second);
        const int bestDist1 = (int)(best >> 16), bestDist2 = (int)second;
        if ((STRICT ? bestDist1 < RUMI_TH_LOW : bestDist1 <= RUMI_TH_LOW) && (float)bestDist1 < nnratio * (float)bestDist2) {
            const int pos = (int)(best & 0xFFFFu);
            if (lane == (pos & 15)) taken.set(pos >> 4);
            if (lane == 0) accept(iq, (int)cIdx[pos]);
        }
    }
}

}  // namespace rumi
