// Scalar oracle of the covisibility store (include/rumi_covis.h), on flat arrays.  TEST INFRASTRUCTURE.
//
// Written from KeyFrame::UpdateConnections (R/lib_src/KeyFrame.cc:487-574) and Tracking::UpdateLocalKeyFrames / UpdateLocalPoints
// (R/lib_src/Tracking.cc:3067-3210, the first branch at :3093-3105, no inertial tail).  A key-frame is a slot, a point an id; "pointer
// order" is ascending key[slot].  The counters are std::map keyed by the order key, as the reference's are keyed by the pointer; nothing
// else of the reference's shape is kept (no copies of the observation maps).
#include <algorithm>
#include <cstdint>
#include <map>
#include <utility>
#include <vector>

extern "C" {

// B times UpdateConnections, none of them writing anything the others read.  Returns 0.
int cvo_update_connections(const uint64_t *key, const int32_t *map_id, const uint8_t *kf_bad, const int32_t *mp_off, const int32_t *mp,
                           const uint8_t *pt_bad, const int32_t *obs_off, const int32_t *obs, int32_t B, const int32_t *batch, int32_t *status,
                           int32_t *conn_off, int32_t *conn_slot, int32_t *conn_count, int32_t *ord_off, int32_t *ord_slot, int32_t *ord_weight) {
    int32_t co = 0, oo = 0;
    for (int b = 0; b < B; b++) {
        const int self = batch[b];
        conn_off[b] = co; ord_off[b] = oo;
        std::map<uint64_t, std::pair<int, int>> counter;             // key -> (slot, count)
        for (int i = mp_off[self]; i < mp_off[self + 1]; i++) {
            const int p = mp[i];
            if (p < 0 || pt_bad[p]) continue;
            for (int o = obs_off[p]; o < obs_off[p + 1]; o++) {
                const int k = obs[o];
                if (k == self || kf_bad[k] || map_id[k] != map_id[self]) continue;
                auto &e = counter[key[k]];
                e.first = k; e.second++;
            }
        }
        if (counter.empty()) { status[b] = 1; continue; }
        status[b] = 0;
        int nmax = 0, kmax = -1;
        std::vector<std::pair<int, uint64_t>> pairs;                 // (weight, key): sort() orders them as pair<int, KeyFrame*>
        for (const auto &e : counter) {
            conn_slot[co] = e.second.first; conn_count[co++] = e.second.second;
            if (e.second.second > nmax) { nmax = e.second.second; kmax = e.second.first; }
            if (e.second.second >= 15) pairs.push_back({e.second.second, e.first});
        }
        if (pairs.empty()) pairs.push_back({nmax, key[kmax]});
        std::sort(pairs.begin(), pairs.end());
        for (size_t i = pairs.size(); i-- > 0;) {                    // push_front of each = the reverse
            ord_slot[oo] = counter[pairs[i].second].first; ord_weight[oo++] = pairs[i].first;
        }
    }
    conn_off[B] = co; ord_off[B] = oo;
    return 0;
}

// One frame.  best [n_kf][10] (-1 padded), parent [n_kf] (-1 = none), children rows.  Returns 0.
int cvo_local_map(int32_t n_kf, const uint64_t *key, const uint8_t *kf_bad, const int32_t *mp_off, const int32_t *mp, const int32_t *best,
                  const int32_t *parent, const int32_t *child_off, const int32_t *children, int32_t n_pts, const uint8_t *pt_bad,
                  const int32_t *obs_off, const int32_t *obs, int32_t n, const int32_t *frame_points, uint8_t *frame_point_bad, int32_t *local_kf,
                  int32_t *n_k1, int32_t *n_local_kf, int32_t *ref_kf, int32_t *local_points, int32_t *n_local_points) {
    std::map<uint64_t, std::pair<int, int>> counter;
    for (int i = 0; i < n; i++) {
        frame_point_bad[i] = 0;
        const int p = frame_points[i];
        if (p < 0) continue;
        if (pt_bad[p]) { frame_point_bad[i] = 1; continue; }        // :3102, the caller NULLs it
        for (int o = obs_off[p]; o < obs_off[p + 1]; o++) {
            auto &e = counter[key[obs[o]]];
            e.first = obs[o]; e.second++;
        }
    }
    std::vector<uint8_t> stamped(n_kf > 0 ? n_kf : 1, 0);            // mnTrackReferenceForFrame == this frame
    std::vector<int> list;
    int max = 0, kmax = -1;
    for (const auto &e : counter) {
        const int k = e.second.first;
        if (kf_bad[k]) continue;
        if (e.second.second > max) { max = e.second.second; kmax = k; }
        list.push_back(k);
        stamped[k] = 1;
    }
    const size_t k1 = list.size();
    for (size_t m = 0; m < k1; m++) {
        if (list.size() > 80) break;
        const int k = list[m];
        for (int j = 0; j < 10; j++) {
            const int nb = best[k * 10 + j];
            if (nb < 0) continue;                                    // padding
            if (!kf_bad[nb] && !stamped[nb]) { list.push_back(nb); stamped[nb] = 1; break; }
        }
        std::vector<std::pair<uint64_t, int>> kids;                  // a std::set<KeyFrame*> walks in pointer order
        for (int j = child_off[k]; j < child_off[k + 1]; j++) kids.push_back({key[children[j]], children[j]});
        std::sort(kids.begin(), kids.end());
        for (const auto &c : kids)
            if (!kf_bad[c.second] && !stamped[c.second]) { list.push_back(c.second); stamped[c.second] = 1; break; }
        const int par = parent[k];
        if (par >= 0 && !stamped[par]) { list.push_back(par); stamped[par] = 1; break; }
    }
    for (size_t i = 0; i < list.size(); i++) local_kf[i] = list[i];
    *n_k1 = (int32_t)k1; *n_local_kf = (int32_t)list.size(); *ref_kf = kmax;

    std::vector<uint8_t> taken(n_pts > 0 ? n_pts : 1, 0);
    int32_t np = 0;
    for (size_t r = list.size(); r-- > 0;) {
        const int k = list[r];
        for (int i = mp_off[k]; i < mp_off[k + 1]; i++) {
            const int p = mp[i];
            if (p < 0 || taken[p] || pt_bad[p]) continue;
            local_points[np++] = p;
            taken[p] = 1;
        }
    }
    *n_local_points = np;
    return 0;
}
}
