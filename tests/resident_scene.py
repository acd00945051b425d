"""A covisibility store filled from a NewPointsScene (tests/newpoints_scene.py), for the tests of rumi_create_new_map_points_resident and of
the store's key-frame features.  TEST INFRASTRUCTURE.

Every feature with kf_mp >= 0 gets a point id of its own; its key-frame is the point's one observer; mp_pos is the point's attribute position
(normal, distances and descriptor are arbitrary: CreateNewMapPoints does not read them).  Slot numbers are not list positions, and the
key-frames enter in another order than the call lists them, so that nothing can lean on either."""
import numpy as np

from newpoints_scene import RATIO_FACTOR, TH_FAR
from rumi_slam_amd.covis import Covisibility
from rumi_slam_amd.mapping import CreateNewMapPointsResident, KeyFrameView, pose


def slot_of(k):
    """Slot of the scene's view k (0 = the current key-frame)."""
    return 5 + 3 * k


def view_pose(v):
    return pose(v.Tcw, v.Ow, v.F12, v.epipole2)


class ResidentScene:
    def __init__(self, scene, reserve=None, sync=True, max_points=None):
        self.views = [scene.cur] + list(scene.neigh)
        total = sum(v.frame.n for v in self.views)
        self.store = Covisibility(slot_of(len(self.views)) + 8, (total + 4096) if max_points is None else max_points)
        if reserve is not None:
            self.store.reserve_features(reserve)
        self.rows = [None] * len(self.views)
        self.next_id = 0
        order = list(range(len(self.views)))[::-1]
        for k in order:
            self.set_row(k, self.views[k])
            if sync:
                self.sync(k)

    # ---- edits ----
    def set_row(self, k, view, first_id=None):
        """The map-point row and the points of view k from a KeyFrameView: fresh ids for its features with kf_mp >= 0."""
        have = np.nonzero(view.kf_mp >= 0)[0]
        ids = np.arange(self.next_id, self.next_id + len(have), dtype=np.int32)
        self.next_id += len(have)
        row = np.full(view.frame.n, -1, np.int32)
        row[have] = ids
        self.rows[k] = row
        s = slot_of(k)
        self.store.set_keyframes([s], [1000 + 7 * s], [0], [0], [row], [[]], [-1], [[]])
        if len(ids):
            self.store.set_points(ids, np.zeros(len(ids), np.uint8), [[s]] * len(ids))
            p = view.mp_pos[have] if view.mp_pos is not None else np.zeros((len(have), 3), np.float32)
            self.set_positions(ids, p)

    def set_positions(self, ids, pos):
        n = len(ids)
        self.store.set_point_attributes(ids, pos, np.tile(np.float32([0, 0, 1]), (n, 1)), np.full(n, 0.5, np.float32), np.full(n, 50.0, np.float32),
                                        np.full((n, 32), 0x5A, np.uint8))

    def sync(self, k, view=None, check=True):
        v = self.views[k] if view is None else view
        return self.store.set_keyframe_features(slot_of(k), v.frame, v.fv, v.K4, check=check)

    # ---- the call ----
    def call(self, matcher, coarse=0, far=0, n=None, neigh=None, **kw):
        """neigh: view indices (1-based) of the neighbours, default all (or the first n)."""
        if neigh is None:
            neigh = list(range(1, len(self.views) if n is None else n + 1))
        return CreateNewMapPointsResident(matcher, self.store, slot_of(0), view_pose(self.views[0]), [slot_of(k) for k in neigh],
                                          [view_pose(self.views[k]) for k in neigh], RATIO_FACTOR, bool(coarse), bool(far), TH_FAR, **kw)

    def edited_view(self, k, kf_mp=None, mp_pos=None):
        """View k with another kf_mp / mp_pos (for the oracle on an edited scene)."""
        v = self.views[k]
        return KeyFrameView(v.frame, v.fv, v.kf_mp if kf_mp is None else kf_mp, v.K4, v.Tcw, v.Ow, v.mp_pos if mp_pos is None else mp_pos,
                            v.F12 if k else None, v.epipole2 if k else None)
