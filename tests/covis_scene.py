"""Maps for the tests of the covisibility store (include/rumi_covis.h), and the binding of their C++ oracle (tests/cpp/covis_oracle.cc).
TEST INFRASTRUCTURE.

A World is the state the store holds, as Python lists: key-frames by slot (order key, map, bad, mp row, best, parent, children) and points
by id (bad, observers).  The ABI does not ask that rows and observers agree (the reference's do not while a point is being added or
erased), so the constructed scenes set each side directly.  uc_scenes() and lm_scenes() are the smallest shapes at which the kernels can
still go wrong, one per line of the list in their docstrings; random_world() is a trajectory with consistent rows and observers."""
import ctypes as C
import os
import subprocess

import numpy as np

from rumi_slam_amd.covis import MAX_KEYFRAMES, NBEST

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class World:
    def __init__(self, max_kf, max_points):
        self.max_kf, self.max_points = max_kf, max_points
        self.kf, self.pt = {}, {}

    def add_kf(self, slot, key, map_id=0, bad=False, mp=(), best=(), parent=-1, children=()):
        self.kf[slot] = dict(key=int(key), map=int(map_id), bad=bool(bad), mp=[int(p) for p in mp], best=[int(b) for b in best], parent=int(parent),
                             children=[int(c) for c in children])

    def add_pt(self, pid, obs=(), bad=False):
        self.pt[pid] = dict(bad=bool(bad), obs=[int(k) for k in obs])

    def copy_kf(self, s):
        return {k: (list(v) if isinstance(v, list) else v) for k, v in self.kf[s].items()}

    def copy(self):
        w = World(self.max_kf, self.max_points)
        w.kf = {s: self.copy_kf(s) for s in self.kf}
        w.pt = {p: dict(bad=d["bad"], obs=list(d["obs"])) for p, d in self.pt.items()}
        return w

    # ---- the flat arrays of the oracle: dense over every slot and id ----
    def flat(self):
        nk, npts = self.max_kf, self.max_points
        key, mapid, kbad = np.zeros(nk, np.uint64), np.zeros(nk, np.int32), np.zeros(nk, np.uint8)
        best, parent = np.full((nk, NBEST), -1, np.int32), np.full(nk, -1, np.int32)
        mp_off, ch_off = np.zeros(nk + 1, np.int32), np.zeros(nk + 1, np.int32)
        mp, ch = [], []
        for s in range(nk):
            d = self.kf.get(s)
            if d is not None:
                key[s], mapid[s], kbad[s], parent[s] = d["key"], d["map"], d["bad"], d["parent"]
                best[s, :len(d["best"])] = d["best"]
                mp += d["mp"]; ch += d["children"]
            mp_off[s + 1], ch_off[s + 1] = len(mp), len(ch)
        pbad, obs_off, obs = np.zeros(npts, np.uint8), np.zeros(npts + 1, np.int32), []
        for p in range(npts):
            d = self.pt.get(p)
            if d is not None:
                pbad[p] = d["bad"]
                obs += d["obs"]
            obs_off[p + 1] = len(obs)
        a = lambda v: np.ascontiguousarray(np.asarray(v, np.int32).reshape(-1), np.int32)
        return dict(key=key, map=mapid, kf_bad=kbad, mp_off=mp_off, mp=a(mp), best=np.ascontiguousarray(best), parent=parent, child_off=ch_off,
                    children=a(ch), pt_bad=pbad, obs_off=obs_off, obs=a(obs))

    # ---- into a handle ----
    def put_keyframes(self, h, slots, check=True):
        slots = list(slots)
        d = [self.kf[s] for s in slots]
        return h.set_keyframes(slots, [x["key"] for x in d], [x["map"] for x in d], [x["bad"] for x in d], [x["mp"] for x in d], [x["best"] for x in d],
                               [x["parent"] for x in d], [x["children"] for x in d], check=check)

    def put_points(self, h, ids, check=True):
        ids = list(ids)
        return h.set_points(ids, [self.pt[p]["bad"] for p in ids], [self.pt[p]["obs"] for p in ids], check=check)

    def load(self, h):
        """The whole state in one go: every key-frame in one call, every point in one call."""
        if self.kf:
            self.put_keyframes(h, sorted(self.kf))
        if self.pt:
            self.put_points(h, sorted(self.pt))
        return h

    def handle(self, arena_entries=0):
        from rumi_slam_amd.covis import Covisibility
        return self.load(Covisibility(self.max_kf, self.max_points, arena_entries))

    def n_live(self):
        return len(self.kf)

    def relabelled(self, seed):
        """The same map with the point ids permuted and every observer row shuffled; returns (world, new id of old id)."""
        rng = np.random.default_rng(seed)
        new_of = rng.permutation(self.max_points)
        w = World(self.max_kf, self.max_points)
        for s, d in self.kf.items():
            w.add_kf(s, d["key"], d["map"], d["bad"], [-1 if p < 0 else new_of[p] for p in d["mp"]], d["best"], d["parent"],
                     [d["children"][j] for j in rng.permutation(len(d["children"]))])
        for p, d in self.pt.items():
            w.add_pt(int(new_of[p]), [d["obs"][j] for j in rng.permutation(len(d["obs"]))], d["bad"])
        return w, new_of


def _keys(rng, n):
    """n distinct order keys, a third of them above 2^63 (an unsigned comparison, not a signed one)."""
    k = set()
    while len(k) < n:
        k.add(int(rng.integers(1, 1 << 62)) | (int(rng.integers(0, 3) == 0) << 63))
    return list(k)


# ---- update_connections: (name, world, batch) ----
def uc_scenes():
    """empty (no countable observer; a row of length 0) | counts 14 and 15 | no count >= 15, a tie at the maximum | three equal weights >= 15 |
    keys anti-monotone in slot | self, bad and other-map observers | a bad point in the row | a point observed by 300 key-frames | rows of
    1, 63, 64, 65, 255, 256, 257 features | observers in slot 0 and slot RUMI_COVIS_MAX_KEYFRAMES - 1 | one slot twice | B = 1 and B = 70"""
    out = []

    def world(n_kf, n_pts, key=lambda s: 1000 - s, max_kf=None):          # keys anti-monotone in the slot unless said otherwise
        w = World(max_kf or n_kf, n_pts)
        for s in range(n_kf):
            w.add_kf(s, key(s))
        return w

    w = world(3, 4)
    w.kf[0]["mp"] = [0, 1, -1]
    w.add_pt(0, [0]); w.add_pt(1, [0])
    out.append(("empty", w, [0, 1]))

    w = world(4, 40)
    w.kf[0]["mp"] = list(range(15))
    for p in range(15):
        w.add_pt(p, [0, 1] + ([2] if p < 14 else []) + ([3] if p < 2 else []))
    out.append(("14_and_15", w, [0]))

    w = world(5, 10, key=lambda s: (50, 40, 10, 30, 20)[s])               # slot 2 is first in key order, slot 3 and 4 tie with it
    w.kf[0]["mp"] = list(range(6))
    for p in range(6):
        w.add_pt(p, [0] + ([1] if p < 3 else []) + ([3, 2, 4] if p < 5 else []))
    out.append(("tie_at_max_below_th", w, [0]))

    w = world(6, 30, key=lambda s: (7, 3, 9, 1, 5, 8)[s])
    w.kf[0]["mp"] = list(range(20))
    for p in range(20):
        w.add_pt(p, [0, 4] + ([1, 2, 3] if p < 16 else []) + ([5] if p < 15 else []))
    out.append(("three_equal_weights", w, [0]))

    w = world(6, 40)
    w.kf[2]["bad"] = True
    w.kf[3]["map"] = 1
    w.kf[0]["mp"] = list(range(16)) + [30]
    w.kf[3]["mp"] = list(range(16))
    for p in range(16):
        w.add_pt(p, [0, 1, 2, 3, 4])                                      # self, good, bad, other map, good
    w.add_pt(30, [5, 0], bad=True)                                        # a bad point: slot 5 gets nothing from it
    w.add_pt(31, [5])
    out.append(("filters_and_bad_point", w, [0, 3]))                      # 3 lives in map 1: every observer of its points is in map 0

    w = world(301, 30)
    w.kf[0]["mp"] = list(range(21))
    for p in range(20):
        w.add_pt(p, list(range(300, -1, -1)))                             # 300 others at weight 20: one long run of equal weights
    w.add_pt(20, [7, 0, 9])
    w.kf[300]["mp"] = [20]                                                # from 300: nobody reaches 15, counts 1, 1, 1
    out.append(("300_observers", w, [0, 300]))

    lens = (1, 63, 64, 65, 255, 256, 257)
    w = world(len(lens) + 3, 300)
    for p in range(300):
        w.add_pt(p, [p % len(lens), 7] + ([8] if p % 3 else []) + ([9] if p >= 240 else []))
    for s, n in enumerate(lens):
        w.kf[s]["mp"] = [(-1 if (i % 17 == 5 and n > 1) else (i + s) % 300) for i in range(n)]
    w.kf[s]["mp"][-1] = 299                                               # the last lane of the 257 row counts
    out.append(("row_seams", w, list(range(len(lens)))))

    w = World(MAX_KEYFRAMES, 40)
    for s, k in ((0, 5), (1, 9), (MAX_KEYFRAMES - 1, 2), (4000, 7)):
        w.add_kf(s, k)
    w.kf[1]["mp"] = list(range(18))
    for p in range(18):
        w.add_pt(p, [MAX_KEYFRAMES - 1, 1, 0] + ([4000] if p < 15 else []))
    out.append(("first_and_last_slot", w, [1, MAX_KEYFRAMES - 1]))

    w, _ = random_world(5, 12, nfeat=(40, 60))
    out.append(("slot_twice", w, [3, 7, 3]))
    w, _ = random_world(6, 75, nfeat=(50, 80))
    out.append(("B1", w, [11]))
    out.append(("B70", w, [int(s) for s in np.random.default_rng(1).permutation(75)[:70]]))
    return out


# ---- local_map: (name, world, [frame points of consecutive calls], expected local_kf of the first call or None) ----
def lm_scenes():
    """no votes | a bad frame point | a tie for the reference | K1 of 80 and 81 | the list passes 80 mid-loop | a first neighbour already
    included and one bad | children out of key order and a bad child | the parent at the second member ends the loop | a bad parent is
    added | a point held by three local key-frames | the frame's own points among the rows | two calls with different frames"""
    out = []

    def world(n_kf, n_pts, key=lambda s: 1000 - s):
        w = World(n_kf, n_pts)
        for s in range(n_kf):
            w.add_kf(s, key(s))
        return w

    w = world(3, 6)
    w.add_pt(0, []); w.add_pt(1, [], bad=True)
    w.kf[0]["mp"] = [0, 1]
    out.append(("no_votes", w, [[-1, 0, -1], [], [1]], []))

    w = world(4, 8, key=lambda s: (4, 3, 2, 1)[s])
    w.add_pt(0, [0, 1]); w.add_pt(1, [2], bad=True); w.add_pt(2, [1, 0]); w.add_pt(3, [3])
    w.kf[0]["mp"] = [0, 1, 2]; w.kf[1]["mp"] = [2, -1, 0]; w.kf[3]["mp"] = [3, 1]
    # slot 2 is voted by the bad point alone: no vote.  0 and 1 tie at 2 votes: 1 is first in key order.  Order: 3 (key 1), 1, 0.
    out.append(("bad_frame_point_and_tie", w, [[0, 1, 2, 3, -1]], [3, 1, 0]))

    for k1 in (80, 81, 78):
        w = world(200, 4, key=lambda s: s + 1)
        w.add_pt(0, list(range(k1)))
        for s in range(k1):
            w.kf[s]["best"] = [100 + s]                                   # every member has a neighbour of its own
            w.kf[s]["mp"] = [0]
        exp = list(range(k1)) + {80: [100], 81: [], 78: [100, 101, 102]}[k1]   # 80 still expands once; 78 stops when the list holds 81
        out.append((f"k1_{k1}", w, [[0]], exp))

    w = world(12, 4, key=lambda s: 100 - s)                               # key order: 11, 10, ..., 0
    w.add_pt(0, [0, 1, 2])
    w.kf[5]["bad"] = True; w.kf[8]["bad"] = True
    w.kf[2]["best"] = [1, 5, 6, 7]                                        # included, bad, taken
    w.kf[2]["children"] = [9, 8, 10]                                      # keys 91, 92 (bad), 90: 10 is first in key order
    w.kf[1]["best"] = [6, 7]                                              # 6 went to member 2: 7
    w.kf[0]["children"] = [10, 9]                                         # 10 is included by now: 9
    out.append(("neighbours_and_children", w, [[0]], [2, 1, 0, 6, 10, 7, 9]))

    w = world(12, 4, key=lambda s: s + 1)                                 # key order = slot order
    w.add_pt(0, [0, 1, 2, 3])
    w.kf[0]["parent"] = 1                                                 # included: the loop goes on
    w.kf[1]["best"] = [5]; w.kf[1]["parent"] = 6; w.kf[6]["bad"] = True  # a bad parent is added all the same, and ends the loop
    w.kf[2]["best"] = [7]; w.kf[2]["children"] = [8]; w.kf[3]["parent"] = 9   # members 3.. add nothing
    out.append(("parent_ends_the_loop", w, [[0]], [0, 1, 2, 3, 5, 6]))

    w = world(4, 12, key=lambda s: s + 1)
    w.add_pt(0, [0, 1, 2]); w.add_pt(1, [0]); w.add_pt(2, [1]); w.add_pt(3, [2]); w.add_pt(4, [2], bad=True); w.add_pt(5, [0])
    w.kf[0]["mp"] = [1, 0, 5]; w.kf[1]["mp"] = [0, 2, 0]; w.kf[2]["mp"] = [3, -1, 4, 0]
    # reverse walk: 2 gives 3, 0 (the shared point, at its place in the LAST key-frame); 1 gives 2; 0 gives 1, 5
    out.append(("shared_point_and_own_points", w, [[0, 5, -1], [1], [0, 3]], [0, 1, 2]))

    w, frames = random_world(9, 40, nfeat=(30, 50), n_frames=3)
    out.append(("consecutive_frames", w, frames, None))
    return out


LM_EXPECTED_POINTS = {"shared_point_and_own_points": [3, 0, 2, 1, 5]}


def random_world(seed, n_kf, nfeat=(40, 70), n_frames=2, max_kf=None, spare_points=0, obs=(2, 9), frame_points=None):
    """A trajectory: point j is observed by the key-frames of a window, one free feature each, so rows and observers agree.  A few
    key-frames are bad or live in a second map, a few points are bad; best, parent and children are a random forest with extra children.
    Returns (world, frames)."""
    rng = np.random.default_rng(9000 + seed)
    n = rng.integers(nfeat[0], nfeat[1] + 1, n_kf)
    keys = _keys(rng, n_kf)
    rows = [np.full(int(n[k]), -1, np.int64) for k in range(n_kf)]
    free = [list(rng.permutation(int(n[k]))) for k in range(n_kf)]
    pts = []
    for _ in range(int(n.sum()) // 4):
        m = int(rng.integers(obs[0], obs[1] + 1))
        t0 = int(rng.integers(0, n_kf))
        pool = [k for k in range(max(0, t0 - m), min(n_kf, t0 + m + 1)) if len(free[k]) > 2]
        if len(pool) < 2:
            continue
        ks = [int(k) for k in rng.choice(pool, min(m, len(pool)), replace=False)]
        for k in ks:
            rows[k][free[k].pop()] = len(pts)
        pts.append(ks)
    w = World(max_kf or n_kf, len(pts) + spare_points)
    bad = rng.random(n_kf) < 0.08
    maps = (rng.random(n_kf) < 0.1).astype(int)
    parent = [-1] + [int(rng.integers(0, k)) for k in range(1, n_kf)]
    for k in range(n_kf):
        kids = [c for c in range(n_kf) if parent[c] == k]
        kids += [int(c) for c in rng.choice(n_kf, 2, replace=False) if c != k and c not in kids and rng.random() < 0.3]
        others = [int(c) for c in rng.permutation(n_kf) if c != k][:int(rng.integers(0, NBEST + 1))]
        w.add_kf(k, keys[k], maps[k], bad[k], rows[k], others, parent[k] if rng.random() < 0.8 else -1, [kids[j] for j in rng.permutation(len(kids))])
    for p, ks in enumerate(pts):
        w.add_pt(p, ks, rng.random() < 0.04)
    frames = []
    for _ in range(n_frames):
        t0 = int(rng.integers(0, n_kf))
        near = [p for p, ks in enumerate(pts) if any(abs(k - t0) <= 2 for k in ks)]
        m = frame_points or int(rng.integers(20, 60))
        f = [int(p) for p in rng.choice(near, min(m, len(near)), replace=False)] if near else []
        f += [-1] * int(rng.integers(0, 10))
        frames.append([f[j] for j in rng.permutation(len(f))])
    return w, frames


def edit_sequence(seed, n_edits=200):
    """(start world, [(kind, payload), ...], final world): about n_edits edits that grow rows, shrink rows, flip bad flags, move key-frames
    between maps and add key-frames and points.  kinds: kf (slots), pt (ids), bad (kf slots, pt ids), maps (slots)."""
    rng = np.random.default_rng(500 + seed)
    w0, _ = random_world(40 + seed, 24, nfeat=(20, 30), max_kf=40, spare_points=60)
    w = w0.copy()
    edits = []
    for e in range(n_edits):
        kind = ("pt", "pt", "pt", "kf", "bad", "maps", "newkf", "grow")[int(rng.integers(0, 8))]
        live = sorted(w.kf)
        if kind == "pt":                                                  # new observers: longer or shorter
            ids = [int(p) for p in rng.choice(w.max_points, int(rng.integers(1, 4)), replace=False)]
            for p in ids:
                m = int(rng.integers(0, min(len(live), 12) + 1))
                w.add_pt(p, [int(k) for k in rng.choice(live, m, replace=False)], rng.random() < 0.1)
            edits.append(("pt", ids))
        elif kind == "grow":                                              # one observer more on a few points: rows leave their places
            ids = [int(p) for p in rng.choice(sorted(w.pt), 3, replace=False)]
            for p in ids:
                rest = [k for k in live if k not in w.pt[p]["obs"]]
                if rest:
                    w.pt[p]["obs"] += [int(k) for k in rng.choice(rest, min(len(rest), 3), replace=False)]
            edits.append(("pt", ids))
        elif kind == "kf":                                                # a row rewritten: other points, another length, new relatives
            s = int(rng.choice(live))
            d = w.kf[s]
            d["mp"] = [int(p) if rng.random() < 0.8 else -1 for p in rng.integers(0, w.max_points, int(rng.integers(0, 45)))]
            d["best"] = [int(k) for k in rng.permutation(live) if k != s][:int(rng.integers(0, NBEST + 1))]
            d["children"] = [int(k) for k in rng.permutation(live) if k != s][:int(rng.integers(0, 5))]
            d["parent"] = int(rng.choice([k for k in live if k != s])) if rng.random() < 0.7 else -1
            edits.append(("kf", [s]))
        elif kind == "newkf" and len(live) < w.max_kf:
            s = int(rng.choice([k for k in range(w.max_kf) if k not in w.kf]))
            w.add_kf(s, _keys(rng, 1)[0] ^ (e << 20), 0, False, [int(p) for p in rng.integers(0, w.max_points, 25)], live[:3], live[0], [])
            edits.append(("kf", [s]))
        elif kind == "bad":
            ks = [int(k) for k in rng.choice(live, 2, replace=False)]
            ps = [int(p) for p in rng.choice(w.max_points, 3, replace=False)]
            for k in ks:
                w.kf[k]["bad"] = bool(rng.random() < 0.3)
            for p in ps:
                if p not in w.pt:
                    w.add_pt(p, [])
                w.pt[p]["bad"] = bool(rng.random() < 0.3)
            edits.append(("bad", (ks, ps)))
        else:
            ks = [int(k) for k in rng.choice(live, 3, replace=False)]
            for k in ks:
                w.kf[k]["map"] = int(rng.integers(0, 2))
            edits.append(("maps", ks))
        kind, what = edits[-1]                                            # the values as they are right after this edit
        ks, ps = what if kind == "bad" else (what, []) if kind in ("kf", "maps") else ([], what)
        snap = World(w.max_kf, w.max_points)
        snap.kf = {k: w.copy_kf(k) for k in ks}
        snap.pt = {p: dict(bad=w.pt[p]["bad"], obs=list(w.pt[p]["obs"])) for p in ps}
        edits[-1] = (kind, what, snap)
    return w0, edits, w


def apply_edit(h, edit):
    """Sends one edit of edit_sequence to the handle."""
    kind, what, w = edit
    if kind == "kf":
        w.put_keyframes(h, what)
    elif kind == "pt":
        w.put_points(h, what)
    elif kind == "bad":
        ks, ps = what
        h.set_bad(ks, [w.kf[k]["bad"] for k in ks], ps, [w.pt[p]["bad"] for p in ps])
    else:
        h.set_maps(what, [w.kf[k]["map"] for k in what])


# ---- the C++ oracle ----
def build_oracle(out_dir):
    so = os.path.join(str(out_dir), "libcovis_oracle.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", os.path.join(ROOT, "tests", "cpp", "covis_oracle.cc"), "-o", so])
    L = C.CDLL(so)
    vp, i32 = C.c_void_p, C.c_int32
    L.cvo_update_connections.argtypes = [vp] * 8 + [i32] + [vp] * 8
    L.cvo_local_map.argtypes = [i32] + [vp] * 8 + [i32] + [vp] * 3 + [i32] + [vp] * 8
    return L


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def oracle_connections(L, w, batch, flat=None):
    """The oracle's update_connections, in the form Covisibility.update_connections returns."""
    f = flat or w.flat()
    B = len(batch)
    cap = max(B * w.n_live(), 1)
    batch = np.ascontiguousarray(batch, np.int32)
    o = dict(status=np.zeros(max(B, 1), np.int32), conn_off=np.zeros(B + 1, np.int32), conn_slot=np.zeros(cap, np.int32), conn_count=np.zeros(cap, np.int32),
             ord_off=np.zeros(B + 1, np.int32), ord_slot=np.zeros(cap, np.int32), ord_weight=np.zeros(cap, np.int32))
    assert L.cvo_update_connections(_ptr(f["key"]), _ptr(f["map"]), _ptr(f["kf_bad"]), _ptr(f["mp_off"]), _ptr(f["mp"]), _ptr(f["pt_bad"]),
                                    _ptr(f["obs_off"]), _ptr(f["obs"]), B, _ptr(batch), *[_ptr(o[k]) for k in
                                                                                           ("status", "conn_off", "conn_slot", "conn_count", "ord_off", "ord_slot", "ord_weight")]) == 0
    nc, no = int(o["conn_off"][B]), int(o["ord_off"][B])
    return dict(status=o["status"][:B], conn_off=o["conn_off"], conn_slot=o["conn_slot"][:nc], conn_count=o["conn_count"][:nc], ord_off=o["ord_off"],
                ord_slot=o["ord_slot"][:no], ord_weight=o["ord_weight"][:no])


def oracle_local_map(L, w, frame, flat=None):
    """The oracle's local_map, in the form Covisibility.local_map returns."""
    f = flat or w.flat()
    fp = np.ascontiguousarray(frame, np.int32)
    n = len(fp)
    bad, lkf, lpt = np.zeros(max(n, 1), np.uint8), np.zeros(max(w.max_kf, 1), np.int32), np.zeros(max(w.max_points, 1), np.int32)
    s = [np.zeros(1, np.int32) for _ in range(4)]                      # n_k1, n_local_kf, ref_kf, n_local_points
    assert L.cvo_local_map(w.max_kf, _ptr(f["key"]), _ptr(f["kf_bad"]), _ptr(f["mp_off"]), _ptr(f["mp"]), _ptr(f["best"]), _ptr(f["parent"]),
                           _ptr(f["child_off"]), _ptr(f["children"]), w.max_points, _ptr(f["pt_bad"]), _ptr(f["obs_off"]), _ptr(f["obs"]), n, _ptr(fp),
                           _ptr(bad), _ptr(lkf), _ptr(s[0]), _ptr(s[1]), _ptr(s[2]), _ptr(lpt), _ptr(s[3])) == 0
    return dict(frame_point_bad=bad[:n], local_kf=lkf[:int(s[1][0])], n_k1=int(s[0][0]), ref_kf=int(s[2][0]), local_points=lpt[:int(s[3][0])])


def differing(a, b):
    """The keys under which two result dicts differ (arrays by their bytes and dtypes, scalars by value)."""
    bad = []
    for k in a:
        x, y = a[k], b[k]
        if isinstance(x, np.ndarray):
            if x.dtype != y.dtype or x.tobytes() != y.tobytes():
                bad.append(k)
        elif x != y:
            bad.append(k)
    return bad


def probe_world(n_kf=300, n_feat=1000, obs=(4, 15), frame_points=400, seed=0):
    """The workload of tools/covis_probe.py: n_kf key-frames of n_feat features, obs observers a point, one frame of frame_points matches."""
    w, frames = random_world(seed, n_kf, nfeat=(n_feat, n_feat), n_frames=1, obs=obs, frame_points=frame_points)
    return w, frames[0]
