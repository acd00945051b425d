// CovisibilityGraph — KeyFrame::UpdateConnections / UpdateCloudConnections for a list of key-frames and Tracking::UpdateLocalMap for a frame,
// over the device-resident store of include/rumi_covis.h.
// A class template over the data-model types, like the rest of facade/: it compiles against the reference's KeyFrame / MapPoint / Map /
// Frame (the members INTEGRATION.md lists) and against the mock model of tests/cpp/mock_model_covis.h.
//
// The store holds what the two members read.  Sync(KeyFrame*) / Sync(MapPoint*) stage one object as it is now (and every key-frame it names
// that the store has not seen); SyncAll(Map*) stages a whole map.  INTEGRATION.md names the mutators of the reference that must call Sync.
// A key-frame's order key is its address: the walks of std::map<KeyFrame*, ..> and std::set<KeyFrame*> and the ties of sort(vPairs) come out
// as the reference's do in the same process.
//
//   UpdateConnections(list)   one device call counts for every key-frame of the list; the host then replays, in list order, what the member
//                             writes: AddConnection(this, w) on every listed key-frame, the three member writes, and the first parent.
//   UpdateLocalMap(frame, ..) one device call; writes the frame's NULLed points, mvpLocalKeyFrames, mvpLocalMapPoints, mpReferenceKF and the
//                             mnTrackReferenceForFrame stamps.  The inertial branches (Tracking.cc:3106-3123, :3190-3204) are refused with
//                             a report: the ABI does not express them.
//   SyncAttributes(points)    stages position, normal, distances and descriptor of the listed points (rumi_covis_set_point_attributes): what
//                             rumi_facade::TrackLocalMapResident (TrackingStep.h) builds its point table from on the device.  MarkDirty(p)
//                             notes a point whose SetWorldPos / UpdateNormalAndDepth / ComputeDistinctiveDescriptors has run (any thread's
//                             caller serialises, as for Sync); FlushDirty() stages the noted points, once each, before the frame's query.
//   Sync(MapPoint*)           stages the feature index of every observation with its observer (rumi_covis_set_point_observations), which is
//                             what rumi::LocalMappingStep::KeyFrameCullingResident reads an observer's octave through.
//   SyncCentres(kfs)          stages GetCameraCenter() of the listed key-frames, SyncReferences(points) GetReferenceKeyFrame() of the listed
//                             points: with those, rumi_facade::RefreshMapPointsResident (MapPointRefresh.h) refreshes points by id, and its
//                             write-back leaves their attributes current in the store without a SyncAttributes.
// Errors follow rumi_status.h: reported, never thrown; the member returns without having written anything.
#pragma once
#include <cstdint>
#include <map>
#include <set>
#include <tuple>
#include <unordered_map>
#include <vector>

#include "rumi_covis.h"
#include "rumi_status.h"

template <class KeyFrameT, class MapPointT> class CovisibilityGraph {
  public:
    CovisibilityGraph(int max_kf, int max_points, int device = -1) {
        const int rc = rumi_covis_create(max_kf, max_points, 0, device, &h_);
        if (rc != RUMI_OK) { rumi_facade::report("CovisibilityGraph", rc); h_ = nullptr; }
    }
    ~CovisibilityGraph() { if (h_) rumi_covis_destroy(h_); }
    CovisibilityGraph(const CovisibilityGraph &) = delete;
    CovisibilityGraph &operator=(const CovisibilityGraph &) = delete;
    bool ok() const { return h_ != nullptr; }

    // ---- keeping the store current ----
    int Sync(KeyFrameT *pKF) { return sync_keyframes(std::vector<KeyFrameT *>{pKF}); }
    int Sync(MapPointT *pMP) { return sync_points(std::vector<MapPointT *>{pMP}); }
    template <class MapT> int SyncAll(MapT *pMap) {
        const int rc = sync_keyframes(pMap->GetAllKeyFrames());
        return rc != RUMI_OK ? rc : sync_points(pMap->GetAllMapPoints());
    }

    // ---- the attributes TrackLocalMap reads (GetWorldPos, GetNormal, GetMinDistance, GetMaxDistance, GetDescriptor)
    int SyncAttributes(const std::vector<MapPointT *> &vpMPs) {
        if (!h_) return RUMI_E_INVALID;
        std::vector<MapPointT *> unseen;
        std::set<MapPointT *> in;
        std::vector<int32_t> ids;
        std::vector<float> pos, nrm, mn, mx;
        std::vector<uint8_t> desc;
        for (MapPointT *p : vpMPs)
            if (p && in.insert(p).second && !id_.count(p)) unseen.push_back(p);
        int rc;
        if (!unseen.empty() && (rc = sync_points(unseen)) != RUMI_OK) return rc;
        for (MapPointT *p : in) {
            ids.push_back(id_[p]);
            const auto P = p->GetWorldPos(), N = p->GetNormal();
            for (int c = 0; c < 3; c++) { pos.push_back(P(c)); nrm.push_back(N(c)); }
            mn.push_back(p->GetMinDistance()); mx.push_back(p->GetMaxDistance());
            const auto d = p->GetDescriptor();
            desc.insert(desc.end(), d.ptr(0), d.ptr(0) + 32);
            dirty_.erase(p);
        }
        if (ids.empty()) return RUMI_OK;
        rc = rumi_covis_set_point_attributes(h_, (int32_t)ids.size(), ids.data(), pos.data(), nrm.data(), mn.data(), mx.data(), desc.data());
        if (rc != RUMI_OK) rumi_facade::report("CovisibilityGraph::SyncAttributes", rc);
        return rc;
    }
    void MarkDirty(MapPointT *pMP) { if (pMP) dirty_.insert(pMP); }
    size_t DirtyCount() const { return dirty_.size(); }
    int FlushDirty() {
        if (dirty_.empty()) return RUMI_OK;
        return SyncAttributes(std::vector<MapPointT *>(dirty_.begin(), dirty_.end()));
    }

    // ---- what rumi_facade::RefreshMapPointsResident (MapPointRefresh.h) reads beside features, observers and attributes: GetCameraCenter()
    // of the key-frames (rumi_covis_set_keyframe_centres; after SetPose) and GetReferenceKeyFrame() of the points
    // (rumi_covis_set_point_reference; wherever mpRefKF changes).  Objects the store has not seen are staged first.
    int SyncCentres(const std::vector<KeyFrameT *> &vpKFs) {
        if (!h_) return RUMI_E_INVALID;
        std::vector<KeyFrameT *> unseen;
        std::set<KeyFrameT *> in;
        for (KeyFrameT *k : vpKFs)
            if (k && in.insert(k).second && !slot_.count(k)) unseen.push_back(k);
        int rc;
        if (!unseen.empty() && (rc = sync_keyframes(unseen)) != RUMI_OK) return rc;
        std::vector<int32_t> slots;
        std::vector<float> Ow;
        for (KeyFrameT *k : in) {
            slots.push_back(slot_[k]);
            const auto C = k->GetCameraCenter();
            for (int c = 0; c < 3; c++) Ow.push_back(C(c));
        }
        if (slots.empty()) return RUMI_OK;
        rc = rumi_covis_set_keyframe_centres(h_, (int32_t)slots.size(), slots.data(), Ow.data());
        if (rc != RUMI_OK) rumi_facade::report("CovisibilityGraph::SyncCentres", rc);
        return rc;
    }
    int SyncReferences(const std::vector<MapPointT *> &vpMPs) {
        if (!h_) return RUMI_E_INVALID;
        std::vector<MapPointT *> unseen;
        std::vector<KeyFrameT *> unseenKfs;
        std::set<MapPointT *> in;
        for (MapPointT *p : vpMPs) {
            if (!p || !in.insert(p).second) continue;
            if (!id_.count(p)) unseen.push_back(p);
            KeyFrameT *ref = p->GetReferenceKeyFrame();
            if (ref && !slot_.count(ref)) unseenKfs.push_back(ref);
        }
        int rc;
        if (!unseenKfs.empty() && (rc = sync_keyframes(unseenKfs)) != RUMI_OK) return rc;
        if (!unseen.empty() && (rc = sync_points(unseen)) != RUMI_OK) return rc;
        std::vector<int32_t> ids, refs;
        for (MapPointT *p : in) {
            KeyFrameT *ref = p->GetReferenceKeyFrame();
            ids.push_back(id_[p]);
            refs.push_back(ref ? slot_[ref] : -1);
        }
        if (ids.empty()) return RUMI_OK;
        rc = rumi_covis_set_point_reference(h_, (int32_t)ids.size(), ids.data(), refs.data());
        if (rc != RUMI_OK) rumi_facade::report("CovisibilityGraph::SyncReferences", rc);
        return rc;
    }

    // ---- what Optimizer::LocalBundleAdjustmentResident (Optimizer.h) reads beside rows, observers, features and attributes: GetPose() of the
    // key-frames (rumi_covis_set_keyframe_poses; after SetPose, beside SyncCentres) and GetMap() of the points (rumi_covis_set_point_maps; where
    // a point is created, and where a merge moves it to another map).  Objects the store has not seen are staged first.
    int SyncPoses(const std::vector<KeyFrameT *> &vpKFs) {
        if (!h_) return RUMI_E_INVALID;
        std::vector<KeyFrameT *> unseen;
        std::set<KeyFrameT *> in;
        for (KeyFrameT *k : vpKFs)
            if (k && in.insert(k).second && !slot_.count(k)) unseen.push_back(k);
        int rc;
        if (!unseen.empty() && (rc = sync_keyframes(unseen)) != RUMI_OK) return rc;
        std::vector<int32_t> slots;
        std::vector<float> T7;
        for (KeyFrameT *k : in) {
            slots.push_back(slot_[k]);
            const auto T = k->GetPose(); const auto q = T.unit_quaternion(); const auto t = T.translation();
            const float p[7] = {q.x(), q.y(), q.z(), q.w(), t(0), t(1), t(2)};
            T7.insert(T7.end(), p, p + 7);
        }
        if (slots.empty()) return RUMI_OK;
        rc = rumi_covis_set_keyframe_poses(h_, (int32_t)slots.size(), slots.data(), T7.data());
        if (rc != RUMI_OK) rumi_facade::report("CovisibilityGraph::SyncPoses", rc);
        return rc;
    }
    int SyncPointMaps(const std::vector<MapPointT *> &vpMPs) {
        if (!h_) return RUMI_E_INVALID;
        std::vector<MapPointT *> unseen;
        std::set<MapPointT *> in;
        for (MapPointT *p : vpMPs)
            if (p && in.insert(p).second && !id_.count(p)) unseen.push_back(p);
        int rc;
        if (!unseen.empty() && (rc = sync_points(unseen)) != RUMI_OK) return rc;
        std::vector<int32_t> ids, maps;
        for (MapPointT *p : in) { ids.push_back(id_[p]); maps.push_back((int32_t)p->GetMap()->GetId()); }
        if (ids.empty()) return RUMI_OK;
        rc = rumi_covis_set_point_maps(h_, (int32_t)ids.size(), ids.data(), maps.data());
        if (rc != RUMI_OK) rumi_facade::report("CovisibilityGraph::SyncPointMaps", rc);
        return rc;
    }

    // ---- the key-frame's constant part (mvKeysUn, mDescriptors, mvScaleFactors, mFeatVec, fx fy cx cy): rumi_covis_set_keyframe_features.
    // SyncFeatures is called once, where the key-frame enters the graph (after ComputeBoW: mFeatVec must be final); DropFeatures from
    // KeyFrame::SetBadFlag.  rumi::LocalMappingStep::CreateNewMapPointsResident then names slots instead of uploading key-frames.
    int SyncFeatures(KeyFrameT *pKF) {
        if (!h_ || !pKF) return RUMI_E_INVALID;
        int rc;
        if (!slot_.count(pKF) && (rc = sync_keyframes(std::vector<KeyFrameT *>{pKF})) != RUMI_OK) return rc;
        RumiFrameFeatures f;
        f.n = pKF->N;
        f.keys_un = reinterpret_cast<const RumiKeyPoint *>(pKF->mvKeysUn.data());
        f.desc = pKF->mDescriptors.ptr(0);
        f.min_x = pKF->mnMinX; f.min_y = pKF->mnMinY; f.max_x = pKF->mnMaxX; f.max_y = pKF->mnMaxY;
        f.scale_factors = pKF->mvScaleFactors.data();
        f.nlevels = (int32_t)pKF->mvScaleFactors.size();
        std::vector<uint32_t> nodes, idx;
        std::vector<int32_t> off{0};
        for (const auto &kv : pKF->mFeatVec) {                                           // std::map order: node ids ascending
            nodes.push_back((uint32_t)kv.first);
            for (unsigned i : kv.second) idx.push_back(i);
            off.push_back((int32_t)idx.size());
        }
        const RumiFeatureVector fv{(int32_t)nodes.size(), nodes.data(), off.data(), idx.data()};
        const float K4[4] = {pKF->fx, pKF->fy, pKF->cx, pKF->cy};
        rc = rumi_covis_set_keyframe_features(h_, slot_[pKF], &f, &fv, K4);
        if (rc != RUMI_OK) { rumi_facade::report("CovisibilityGraph::SyncFeatures", rc); return rc; }
        featured_.insert(pKF);
        return RUMI_OK;
    }
    int DropFeatures(KeyFrameT *pKF) {
        auto it = slot_.find(pKF);
        if (!h_ || it == slot_.end()) return RUMI_OK;                                    // never seen: nothing to drop
        const int32_t s = it->second;
        const int rc = rumi_covis_drop_keyframe_features(h_, 1, &s);
        if (rc != RUMI_OK) rumi_facade::report("CovisibilityGraph::DropFeatures", rc);
        featured_.erase(pKF);
        return rc;
    }
    bool HasFeatures(KeyFrameT *pKF) const { return featured_.count(pKF) > 0; }
    // the slot of a key-frame the store has seen, else -1
    int SlotOf(KeyFrameT *pKF) const { auto it = slot_.find(pKF); return it == slot_.end() ? -1 : it->second; }

    // ---- for the callers that drive the store themselves (TrackingStep.h): the handle, and objects <-> slots and ids
    RumiCovis *handle() const { return h_; }
    int KeyFrameCount() const { return (int)kfs_.size(); }
    int PointCount() const { return (int)pts_.size(); }
    KeyFrameT *KeyFrameAt(int slot) const { return kfs_[slot]; }
    MapPointT *PointAt(int id) const { return pts_[id]; }
    // has the store seen the point?  (IdOf below stages a point it has not)
    bool HasPoint(MapPointT *pMP) const { return id_.count(pMP) > 0; }
    // the id of a point, staging it first when the store has not seen it (-1 on failure)
    int IdOf(MapPointT *pMP) {
        auto it = id_.find(pMP);
        if (it != id_.end()) return it->second;
        if (sync_points(std::vector<MapPointT *>{pMP}) != RUMI_OK) return -1;
        return id_[pMP];
    }
    int64_t LastUploadBytes() const {
        int64_t v[7] = {0, 0, 0, 0, 0, 0, 0};
        return h_ && rumi_covis_stats(h_, v) == RUMI_OK ? v[6] : -1;
    }

    // KeyFrame::UpdateConnections for every key-frame of the list, in this order.  cloud: UpdateCloudConnections (the parent is the first of
    // the ordered list with an earlier time stamp, KeyFrame.cc:656-668).
    int UpdateConnections(const std::vector<KeyFrameT *> &vpKFs, bool cloud = false) {
        if (!h_) { rumi_facade::report("CovisibilityGraph::UpdateConnections", RUMI_E_INVALID, "no store"); return RUMI_E_INVALID; }
        if (vpKFs.empty()) return RUMI_OK;
        int rc;
        std::vector<KeyFrameT *> unseen;
        for (KeyFrameT *k : vpKFs)
            if (!slot_.count(k)) unseen.push_back(k);
        if (!unseen.empty() && (rc = sync_keyframes(unseen)) != RUMI_OK) return rc;
        const int B = (int)vpKFs.size();
        std::vector<int32_t> batch(B), status(B), co(B + 1), oo(B + 1);
        for (int b = 0; b < B; b++) batch[b] = slot_[vpKFs[b]];
        const int64_t cap = (int64_t)B * (int64_t)kfs_.size();
        std::vector<int32_t> cs(cap), cc(cap), os(cap), ow(cap);
        rc = rumi_covis_update_connections(h_, B, batch.data(), status.data(), co.data(), cs.data(), cc.data(), cap, oo.data(), os.data(), ow.data(), cap);
        if (rc != RUMI_OK) { rumi_facade::report("CovisibilityGraph::UpdateConnections", rc); return rc; }
        // ---- the host replay, in list order (KeyFrame.cc:519-572)
        std::set<KeyFrameT *> touched;
        for (int b = 0; b < B; b++) {
            KeyFrameT *pKF = vpKFs[b];
            if (status[b] == RUMI_COVIS_EMPTY) continue;                                 // :519
            std::map<KeyFrameT *, int> counter;
            for (int i = co[b]; i < co[b + 1]; i++) counter[kfs_[cs[i]]] = cc[i];
            std::vector<KeyFrameT *> ordered;
            std::vector<int> weights;
            for (int i = oo[b]; i < oo[b + 1]; i++) {
                kfs_[os[i]]->AddConnection(pKF, ow[i]);                                  // :536, :546
                touched.insert(kfs_[os[i]]);
                ordered.push_back(kfs_[os[i]]);
                weights.push_back(ow[i]);
            }
            pKF->SetCovisibility(counter, ordered, weights);                             // :563-565
            if (pKF->FirstConnection() && pKF->mnId != pKF->GetMap()->GetInitKFid()) {
                KeyFrameT *parent = nullptr;
                if (!cloud) parent = ordered.front();                                    // :567-571
                else
                    for (KeyFrameT *c : ordered)
                        if (c->mTimeStamp < pKF->mTimeStamp) { parent = c; break; }      // :656-668
                if (parent) { pKF->SetFirstParent(parent); touched.insert(parent); }
            }
            touched.insert(pKF);
        }
        return touched.empty() ? RUMI_OK : sync_keyframes(std::vector<KeyFrameT *>(touched.begin(), touched.end()));
    }

    // Tracking::UpdateLocalMap without the visualisation call.  voteFromCurrentFrame: the condition of Tracking.cc:3093; inertialSensor: the
    // condition of :3191.  Returns RUMI_OK, or the status reported.
    template <class FrameT>
    int UpdateLocalMap(FrameT &F, std::vector<KeyFrameT *> &vpLocalKeyFrames, std::vector<MapPointT *> &vpLocalMapPoints, KeyFrameT *&pReferenceKF,
                       bool voteFromCurrentFrame = true, bool inertialSensor = false) {
        const char *where = "CovisibilityGraph::UpdateLocalMap";
        if (!h_) { rumi_facade::report(where, RUMI_E_INVALID, "no store"); return RUMI_E_INVALID; }
        if (!voteFromCurrentFrame || inertialSensor) {
            rumi_facade::report(where, RUMI_E_INVALID, "the inertial branches (vote from the last frame, the temporal key-frames) are not built");
            return RUMI_E_INVALID;
        }
        int rc;
        std::vector<MapPointT *> unseen;
        std::vector<int32_t> fp(F.N, -1);
        for (int i = 0; i < F.N; i++) {
            MapPointT *p = F.mvpMapPoints[i];
            if (!p) continue;
            auto it = id_.find(p);
            if (it == id_.end()) unseen.push_back(p);
            else fp[i] = it->second;
        }
        if (!unseen.empty()) {
            if ((rc = sync_points(unseen)) != RUMI_OK) return rc;
            for (int i = 0; i < F.N; i++)
                if (F.mvpMapPoints[i]) fp[i] = id_[F.mvpMapPoints[i]];
        }
        std::vector<uint8_t> bad(F.N > 0 ? F.N : 1);
        std::vector<int32_t> lk(kfs_.size() + 1), lp(pts_.size() + 1);
        int32_t nK1 = 0, nK = 0, ref = -1, nP = 0;
        rc = rumi_covis_local_map(h_, F.N, fp.data(), bad.data(), lk.data(), (int32_t)kfs_.size(), &nK1, &nK, &ref, lp.data(), (int32_t)pts_.size(), &nP);
        if (rc != RUMI_OK) { rumi_facade::report(where, rc); return rc; }
        for (int i = 0; i < F.N; i++)
            if (bad[i]) F.mvpMapPoints[i] = nullptr;                                     // :3102
        vpLocalKeyFrames.clear();
        for (int i = 0; i < nK; i++) {
            vpLocalKeyFrames.push_back(kfs_[lk[i]]);
            kfs_[lk[i]]->mnTrackReferenceForFrame = F.mnId;
        }
        vpLocalMapPoints.clear();
        for (int i = 0; i < nP; i++) {
            vpLocalMapPoints.push_back(pts_[lp[i]]);
            pts_[lp[i]]->mnTrackReferenceForFrame = F.mnId;
        }
        if (ref >= 0) { pReferenceKF = kfs_[ref]; F.mpReferenceKF = pReferenceKF; }      // :3206-3209
        return RUMI_OK;
    }

  private:
    RumiCovis *h_ = nullptr;
    std::unordered_map<KeyFrameT *, int32_t> slot_;
    std::unordered_map<MapPointT *, int32_t> id_;
    std::vector<KeyFrameT *> kfs_;
    std::vector<MapPointT *> pts_;
    std::set<MapPointT *> dirty_;
    std::set<KeyFrameT *> featured_;                                                     // key-frames whose features the store holds

    int32_t slot_of(KeyFrameT *k, std::vector<KeyFrameT *> &work) {                      // a key-frame the store has not seen joins the call
        auto it = slot_.find(k);
        if (it != slot_.end()) return it->second;
        const int32_t s = (int32_t)kfs_.size();
        slot_[k] = s; kfs_.push_back(k); work.push_back(k);
        return s;
    }

    template <class List> int sync_keyframes(const List &list) {
        if (!h_) return RUMI_E_INVALID;
        std::vector<KeyFrameT *> work;
        std::set<KeyFrameT *> in;
        for (KeyFrameT *k : list)
            if (k && in.insert(k).second) { if (!slot_.count(k)) slot_of(k, work); else work.push_back(k); }
        std::vector<int32_t> slots, maps, mpOff{0}, mp, best, parent, chOff{0}, ch;
        std::vector<uint64_t> keys;
        std::vector<uint8_t> bad;
        std::vector<MapPointT *> newPts;
        for (size_t w = 0; w < work.size(); w++) {                                       // grows while relatives join
            KeyFrameT *k = work[w];
            in.insert(k);
            slots.push_back(slot_[k]);
            keys.push_back((uint64_t)(uintptr_t)k);
            maps.push_back((int32_t)k->GetMap()->GetId());
            bad.push_back(k->isBad() ? 1 : 0);
            for (MapPointT *p : k->GetMapPointMatches()) {
                if (!p) { mp.push_back(-1); continue; }
                auto it = id_.find(p);
                if (it == id_.end()) { it = id_.emplace(p, (int32_t)pts_.size()).first; pts_.push_back(p); newPts.push_back(p); }
                mp.push_back(it->second);
            }
            mpOff.push_back((int32_t)mp.size());
            const std::vector<KeyFrameT *> nb = k->GetBestCovisibilityKeyFrames(RUMI_COVIS_NBEST);
            for (int j = 0; j < RUMI_COVIS_NBEST; j++) best.push_back(j < (int)nb.size() ? slot_of(nb[j], work) : -1);
            KeyFrameT *par = k->GetParent();
            parent.push_back(par ? slot_of(par, work) : -1);
            for (KeyFrameT *c : k->GetChilds()) ch.push_back(slot_of(c, work));
            chOff.push_back((int32_t)ch.size());
        }
        if (slots.empty()) return RUMI_OK;
        int rc = rumi_covis_set_keyframes(h_, (int32_t)slots.size(), slots.data(), keys.data(), maps.data(), bad.data(), mpOff.data(), mp.data(), best.data(),
                                          parent.data(), chOff.data(), ch.data());
        if (rc != RUMI_OK) { rumi_facade::report("CovisibilityGraph::Sync(KeyFrame)", rc); return rc; }
        return newPts.empty() ? RUMI_OK : sync_points(newPts);                           // points first seen in a row: their observers go along
    }

    template <class List> int sync_points(const List &list) {
        if (!h_) return RUMI_E_INVALID;
        std::vector<KeyFrameT *> newKfs;
        std::vector<int32_t> ids, off{0}, obs, feat;
        std::vector<uint8_t> bad;
        std::set<MapPointT *> in;
        bool leftOnly = true;                                                            // every observation has a left index the store can keep
        for (MapPointT *p : list) {
            if (!p || !in.insert(p).second) continue;
            auto it = id_.find(p);
            if (it == id_.end()) { it = id_.emplace(p, (int32_t)pts_.size()).first; pts_.push_back(p); }
            ids.push_back(it->second);
            bad.push_back(p->isBad() ? 1 : 0);
            for (const auto &o : p->GetObservations()) {
                obs.push_back(slot_of(o.first, newKfs));
                const int left = std::get<0>(o.second);                                  // the feature index KeyFrameCullingResident reads the octave through
                feat.push_back(left);
                leftOnly = leftOnly && left >= 0 && left < RUMI_COVIS_MAX_FEATURES;
            }
            off.push_back((int32_t)obs.size());
        }
        if (ids.empty()) return RUMI_OK;
        int rc;
        if (!newKfs.empty()) {                                                           // observers the store has not seen: staged first
            for (KeyFrameT *k : newKfs) { kfs_.pop_back(); slot_.erase(k); }             // sync_keyframes assigns the same slots again
            if ((rc = sync_keyframes(newKfs)) != RUMI_OK) return rc;
        }
        // a right-only (stereo) observation has no left index: those points go without observation features, and the resident culling,
        // which is monocular, refuses a call that reads one of them
        rc = leftOnly ? rumi_covis_set_point_observations(h_, (int32_t)ids.size(), ids.data(), bad.data(), off.data(), obs.data(), feat.data())
                      : rumi_covis_set_points(h_, (int32_t)ids.size(), ids.data(), bad.data(), off.data(), obs.data());
        if (rc != RUMI_OK) rumi_facade::report("CovisibilityGraph::Sync(MapPoint)", rc);
        return rc;
    }
};
