// The scalar loop of Optimizer::LocalBundleAdjustment's graph construction (R/lib_src/Optimizer.cc:1003-1271, monocular branch) on flat host
// arrays: what tools/lba_probe.py --resident times on one core beside rumi_local_ba.  Stamps instead of the mnBALocalForKF members, a sort
// by order_key per point instead of the std::map walk; the live object graph of the reference (hash lookups, map nodes) is slower than this.
//   g++ -O2 -shared -fPIC tools/lba_flatten.cc -o tools/bin/liblba_flatten.so
#include <algorithm>
#include <cstdint>
#include <vector>

extern "C" int lba_flatten(int32_t n_kf, const uint64_t *key, const int32_t *kf_map, const uint8_t *kf_bad, const int32_t *row_off, const int32_t *row,
                           const float *kp_x, const float *kp_y, const int32_t *kp_oct, const float *sf, int32_t nlevels, const float *pose7,
                           int32_t n_pt, const uint8_t *pt_bad, const int32_t *pt_map, const float *pos, const int32_t *obs_off, const int32_t *obs_slot,
                           const int32_t *obs_feat, int32_t cur, const int32_t *neigh, int32_t n_neigh, int32_t init,
                           int32_t *kf_slots, float *kf_pose, uint8_t *kf_fixed, int32_t *mp_ids, float *mp_pos, int32_t *e_mp, int32_t *e_kf, float *e_obs,
                           float *e_w, int32_t *counts /* nKF, nOpt, nFixed, nMP, nE */) {
    std::vector<int32_t> local(n_kf, -1), index(n_kf, -1);
    std::vector<uint8_t> stampL(n_kf, 0), stampF(n_kf, 0), seen(n_pt, 0);
    const int32_t curMap = kf_map[cur];
    int nKF = 0, nFixed = 0, nMP = 0, nE = 0;
    auto add_kf = [&](int32_t s, bool fixed) {
        index[s] = nKF; kf_slots[nKF] = s; kf_fixed[nKF] = fixed;
        for (int c = 0; c < 7; c++) kf_pose[nKF * 7 + c] = pose7[s * 7 + c];
        nKF++;
    };
    stampL[cur] = 1; add_kf(cur, cur == init);
    for (int i = 0; i < n_neigh; i++) {
        const int32_t s = neigh[i];
        stampL[s] = 1;
        if (!kf_bad[s] && kf_map[s] == curMap) add_kf(s, s == init);
    }
    const int nOpt = nKF;
    for (int k = 0; k < nOpt; k++) {
        const int32_t s = kf_slots[k];
        if (s == init) nFixed = 1;
        for (int32_t j = row_off[s]; j < row_off[s + 1]; j++) {
            const int32_t p = row[j];
            if (p < 0 || pt_bad[p] || pt_map[p] != curMap || seen[p]) continue;
            seen[p] = 1; mp_ids[nMP++] = p;
        }
    }
    std::vector<std::pair<uint64_t, int32_t>> ord;
    auto by_key = [&](int32_t p) {
        ord.clear();
        for (int32_t j = obs_off[p]; j < obs_off[p + 1]; j++) ord.emplace_back(key[obs_slot[j]], j);
        std::sort(ord.begin(), ord.end());
    };
    for (int i = 0; i < nMP; i++) {
        by_key(mp_ids[i]);
        for (const auto &o : ord) {
            const int32_t s = obs_slot[o.second];
            if (stampL[s] || stampF[s]) continue;
            stampF[s] = 1;
            if (!kf_bad[s] && kf_map[s] == curMap) { add_kf(s, true); nFixed++; }
        }
    }
    counts[0] = nKF; counts[1] = nOpt; counts[2] = nFixed; counts[3] = nMP; counts[4] = 0;
    if (nFixed == 0) return 1;
    for (int i = 0; i < nMP; i++) {
        const int32_t p = mp_ids[i];
        for (int c = 0; c < 3; c++) mp_pos[i * 3 + c] = pos[p * 3 + c];
        by_key(p);
        for (const auto &o : ord) {
            const int32_t s = obs_slot[o.second], f = obs_feat[o.second];
            if (kf_bad[s] || kf_map[s] != curMap || index[s] < 0) continue;
            const int32_t g = row_off[s] + f;
            const float sc = sf[s * nlevels + kp_oct[g]];
            e_mp[nE] = i; e_kf[nE] = index[s]; e_obs[2 * nE] = kp_x[g]; e_obs[2 * nE + 1] = kp_y[g]; e_w[nE] = 1.0f / (sc * sc);
            nE++;
        }
    }
    counts[4] = nE;
    return 0;
}
