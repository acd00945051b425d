// ORB_SLAM3::KeyFrameDatabase (R/include/cloud_edge_slam_lib/KeyFrameDatabase.h, R/lib_src/KeyFrameDatabase.cc) over the device key-frame
// database of include/rumi_kfdb.h, templated over the caller's KeyFrame / Frame / Map so that it drops into the reference's data model:
//
//   namespace ORB_SLAM3 { using KeyFrameDatabase = rumi_facade::KeyFrameDatabaseT<KeyFrame, Frame, Map>; }
//
// What it reads from the model, and when:
//   KeyFrame: mnId, mBowVec (add), GetMap(), isBad(), GetBestCovisibilityKeyFrames(10), GetConnectedKeyFrames() (queries);
//   Frame:    mnId, mBowVec;
//   Map:      IsBad().
// A query runs in two stages.  The score stage returns the key-frames it scored; before the select stage the facade reads, for each of them
// and for each of their ten best covisibles, the current covisibility list, map, isBad() and the map's IsBad(), so the device sees the model as
// the reference's query would (the accumulation reads exactly those key-frames).  clearMap reads every key-frame's GetMap() first.
// Maps are given int32 ids in the order the facade first meets them.
//
// One deviation, as in the C ABI: DetectNBestCandidates skips an isBad() key-frame and advances (the reference's `continue` there does not
// advance and would not terminate).  Errors are reported through rumi_facade::report (rumi_status.h); the query then returns no candidates.
#pragma once
#include <cstdint>
#include <map>
#include <set>
#include <unordered_map>
#include <vector>

#include "rumi_kfdb.h"
#include "rumi_status.h"

namespace rumi_facade {

template <class KeyFrame, class Frame, class Map>
class KeyFrameDatabaseT {
public:
    // voc: any vocabulary object with handle() -> RumiVocabulary* (rumi_facade::ORBVocabulary); it must outlive the database
    template <class Voc>
    explicit KeyFrameDatabaseT(const Voc &voc, int32_t max_kf = 1 << 16, int64_t max_entries = (int64_t)1 << 25, int32_t device = -1)
        : maxKf_(max_kf), maxEntries_(max_entries), device_(device) {
        create(voc.handle());
    }
    ~KeyFrameDatabaseT() { if (db_) rumi_kfdb_destroy(db_); }
    KeyFrameDatabaseT(const KeyFrameDatabaseT &) = delete;
    KeyFrameDatabaseT &operator=(const KeyFrameDatabaseT &) = delete;

    void add(KeyFrame *pKF) {                                                   // KeyFrameDatabase.cc:38-44
        if (!db_ || !pKF) return;
        std::vector<uint32_t> w;
        std::vector<double> v;
        for (auto it = pKF->mBowVec.begin(); it != pKF->mBowVec.end(); ++it) { w.push_back((uint32_t)it->first); v.push_back((double)it->second); }
        const uint64_t id = (uint64_t)pKF->mnId;
        const int32_t map = mapId(pKF->GetMap());
        const int32_t off[2] = {0, (int32_t)w.size()};
        const int rc = rumi_kfdb_add(db_, 1, &id, &map, off, w.data(), v.data());
        if (rc != RUMI_OK) { report("KeyFrameDatabase::add", rc); return; }
        kfs_[id] = pKF;
    }

    void erase(KeyFrame *pKF) {                                                 // :46-64
        if (!db_ || !pKF) return;
        const uint64_t id = (uint64_t)pKF->mnId;
        const int rc = rumi_kfdb_erase(db_, 1, &id);
        if (rc != RUMI_OK) report("KeyFrameDatabase::erase", rc);
        kfs_.erase(id);
    }

    void clear() {                                                              // :66-70
        if (!db_) return;
        const int rc = rumi_kfdb_clear(db_);
        if (rc != RUMI_OK) report("KeyFrameDatabase::clear", rc);
        kfs_.clear();
    }

    void clearMap(Map *pMap) {                                                  // :72-94, by each key-frame's current map
        if (!db_) return;
        std::vector<KeyFrame *> all;
        for (auto &p : kfs_) all.push_back(p.second);
        refreshMaps(all);
        const int rc = rumi_kfdb_clear_map(db_, mapId(pMap));
        if (rc != RUMI_OK) report("KeyFrameDatabase::clearMap", rc);
        for (KeyFrame *k : all) if (k->GetMap() == pMap) kfs_.erase((uint64_t)k->mnId);
    }

    // The reference only swaps its vocabulary pointer (a loaded atlas).  Word ids are the vocabulary's, so the inverted file stays; an empty
    // database is re-created on the new vocabulary.
    template <class Voc> void SetORBVocabulary(Voc *pORBVoc) {
        if (pORBVoc && kfs_.empty()) { if (db_) rumi_kfdb_destroy(db_); db_ = nullptr; create(pORBVoc->handle()); }
    }

    // :604-708
    void DetectNBestCandidates(KeyFrame *pKF, std::vector<KeyFrame *> &vpLoopCand, std::vector<KeyFrame *> &vpMergeCand, int nNumCandidates) {
        if (!db_ || !pKF || nNumCandidates < 0) return;
        std::vector<uint32_t> w;
        std::vector<double> v;
        bow(pKF->mBowVec, w, v);
        const uint64_t qid = (uint64_t)pKF->mnId;
        const int32_t qmap = mapId(pKF->GetMap());
        std::vector<uint64_t> conn;
        for (KeyFrame *k : pKF->GetConnectedKeyFrames()) if (k) conn.push_back((uint64_t)k->mnId);
        const int32_t off[2] = {0, (int32_t)w.size()}, coff[2] = {0, (int32_t)conn.size()};
        int32_t so[2] = {0, 0};
        int rc = rumi_kfdb_score(db_, RUMI_KFDB_NBEST, 1, &qid, &qmap, nullptr, off, w.data(), v.data(), coff, conn.data(), so);
        if (rc != RUMI_OK) { report("KeyFrameDatabase::DetectNBestCandidates", rc); return; }
        if ((rc = refreshScored(so[1])) != RUMI_OK) report("KeyFrameDatabase::DetectNBestCandidates", rc);
        const int32_t n = nNumCandidates, stride = nNumCandidates > 0 ? nNumCandidates : 1;
        int32_t nl = 0, nm = 0;
        std::vector<uint64_t> li(stride), mi(stride);
        rc = rumi_kfdb_select_nbest(db_, &n, stride, &nl, li.data(), &nm, mi.data());
        if (rc != RUMI_OK) { report("KeyFrameDatabase::DetectNBestCandidates", rc); return; }
        vpLoopCand.reserve(nNumCandidates);
        vpMergeCand.reserve(nNumCandidates);
        for (int i = 0; i < nl; i++) vpLoopCand.push_back(kfs_.at(li[i]));
        for (int i = 0; i < nm; i++) vpMergeCand.push_back(kfs_.at(mi[i]));
    }

    // :733-843
    std::vector<KeyFrame *> DetectRelocalizationCandidates(Frame *F, Map *pMap) {
        std::vector<KeyFrame *> out;
        if (!db_ || !F) return out;
        std::vector<uint32_t> w;
        std::vector<double> v;
        bow(F->mBowVec, w, v);
        const uint64_t qid = (uint64_t)F->mnId;
        const int32_t qmap = mapId(pMap);
        const int32_t off[2] = {0, (int32_t)w.size()};
        int32_t so[2] = {0, 0};
        int rc = rumi_kfdb_score(db_, RUMI_KFDB_RELOC, 1, &qid, &qmap, nullptr, off, w.data(), v.data(), nullptr, nullptr, so);
        if (rc != RUMI_OK) { report("KeyFrameDatabase::DetectRelocalizationCandidates", rc); return out; }
        if ((rc = refreshScored(so[1])) != RUMI_OK) report("KeyFrameDatabase::DetectRelocalizationCandidates", rc);
        int32_t co[2] = {0, 0};
        std::vector<uint64_t> ids((size_t)so[1] + 1);
        rc = rumi_kfdb_select_reloc(db_, co, ids.data(), (int64_t)ids.size());
        if (rc != RUMI_OK) { report("KeyFrameDatabase::DetectRelocalizationCandidates", rc); return out; }
        for (int i = 0; i < co[1]; i++) out.push_back(kfs_.at(ids[i]));
        return out;
    }

    RumiKFDatabase *handle() const { return db_; }

private:
    void create(const RumiVocabulary *voc) {
        const int rc = rumi_kfdb_create(voc, maxKf_, maxEntries_, device_, &db_);
        if (rc != RUMI_OK) { db_ = nullptr; report("KeyFrameDatabase::KeyFrameDatabase", rc); }
    }

    template <class BowVectorT> static void bow(const BowVectorT &b, std::vector<uint32_t> &w, std::vector<double> &v) {
        for (auto it = b.begin(); it != b.end(); ++it) { w.push_back((uint32_t)it->first); v.push_back((double)it->second); }
    }

    int32_t mapId(Map *m) {
        auto it = mapIds_.find(m);
        if (it != mapIds_.end()) return it->second;
        const int32_t id = (int32_t)mapIds_.size() + 1;
        mapIds_[m] = id;
        maps_[id] = m;
        return id;
    }

    int refreshMaps(const std::vector<KeyFrame *> &ks) {
        if (ks.empty()) return RUMI_OK;
        std::vector<uint64_t> ids;
        std::vector<int32_t> maps;
        std::vector<uint8_t> bad;
        for (KeyFrame *k : ks) { ids.push_back((uint64_t)k->mnId); maps.push_back(mapId(k->GetMap())); bad.push_back(k->isBad() ? 1 : 0); }
        int rc = rumi_kfdb_set_maps(db_, (int32_t)ids.size(), ids.data(), maps.data());
        if (rc == RUMI_OK) rc = rumi_kfdb_set_bad(db_, (int32_t)ids.size(), ids.data(), bad.data());
        return rc;
    }

    // between score and select: covisibility, map, isBad() of the scored key-frames and their covisibles, and IsBad() of every known map
    int refreshScored(int32_t n) {
        if (n <= 0) return RUMI_OK;
        std::vector<uint64_t> ids((size_t)n);
        std::vector<float> si((size_t)n);
        int rc = rumi_kfdb_scored(db_, ids.data(), si.data());
        if (rc != RUMI_OK) return rc;
        std::vector<KeyFrame *> touched;
        std::set<KeyFrame *> seen;
        std::vector<int64_t> rows((size_t)n * RUMI_KFDB_NCOV, -1);
        for (int i = 0; i < n; i++) {
            KeyFrame *p = kfs_.at(ids[i]);
            if (seen.insert(p).second) touched.push_back(p);
            int k = 0;
            for (KeyFrame *c : p->GetBestCovisibilityKeyFrames(RUMI_KFDB_NCOV)) {
                if (!c || k >= RUMI_KFDB_NCOV) continue;
                rows[(size_t)i * RUMI_KFDB_NCOV + k++] = (int64_t)c->mnId;
                if (kfs_.count((uint64_t)c->mnId) && seen.insert(c).second) touched.push_back(c);
            }
        }
        if ((rc = rumi_kfdb_set_covisibles(db_, n, ids.data(), rows.data())) != RUMI_OK) return rc;
        if ((rc = refreshMaps(touched)) != RUMI_OK) return rc;
        for (KeyFrame *k : touched) mapId(k->GetMap());
        for (auto &m : maps_)
            if (m.second && (rc = rumi_kfdb_set_map_bad(db_, m.first, m.second->IsBad() ? 1 : 0)) != RUMI_OK) return rc;
        return RUMI_OK;
    }

    RumiKFDatabase *db_ = nullptr;
    int32_t maxKf_;
    int64_t maxEntries_;
    int32_t device_;
    std::unordered_map<uint64_t, KeyFrame *> kfs_;
    std::map<Map *, int32_t> mapIds_;
    std::map<int32_t, Map *> maps_;
};

}  // namespace rumi_facade
