#!/usr/bin/env python3
"""Measurements behind the PD frame selector, one JSON record per line on standard output and, with --out FILE, appended to
that file (the quoted copy lives in profiles/).  640 x 480 frames, ORBextractor(2000, 1.2, 8, 20, 7): the reference's configuration.

  step     rumi_kfd_step through the C entry on the extractor's pinned capture buffer, results read where they lie in pinned memory: a
           NON-selecting step (setpoint far above every flow) and a SELECTING step (setpoint far below), --frames steps a round, --rounds rounds
           alternated, the run-to-run spread of the first variant first; rumi_orb_extract alone on the same frames (what a selecting step adds);
           the oracle's step (tests/cpp/kfd_oracle.cc, g++ -O2) on one host core of the same machine: the yardstick.
  --trace  only runs the two kinds of step (for a separate rocprofv3 --kernel-trace --stats pass; nothing is timed or written).

The camera moves two pixels right and one down and back again, so the tracked points stay inside the frame over a round.  Needs a GPU: there is no fallback."""
import argparse
import ctypes as C
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

W, H, ORB = 640, 480, (2000, 1.2, 8, 20, 7)
NEVER, ALWAYS = 1e9, -1e9                                     # setpoints: TH = moptf + 0.8 (th - moptf) + ... lies far above / below moptf


def stats(xs):
    xs = sorted(xs)
    return {"min": round(xs[0], 2), "median": round(xs[len(xs) // 2], 2), "max": round(xs[-1], 2)}


def make_frames():
    from rumi_slam_amd.synth import synth_frame
    a = synth_frame(4711)
    assert a.shape == (H, W)
    return [a, np.ascontiguousarray(np.roll(a, (1, 2), (0, 1)))]


class Device:
    def __init__(self):
        from rumi_slam_amd import capi
        from rumi_slam_amd.extractor import ORBextractor
        from rumi_slam_amd.kfd import KFDSampler
        self.capi, self.L = capi, capi.kfd_lib()
        self.ext = ORBextractor(*ORB)
        self.kfd = KFDSampler(self.ext)
        self.buf = self.ext.image_buffer(W, H)
        self.bufp, self.stride = C.c_void_p(self.buf.ctypes.data), self.buf.strides[0]
        self.out = capi.RumiKfdStep()
        self.frames = make_frames()
        self.t = 0.0

    def steps(self, n, setpoint):
        """n timed steps (seconds each) after a first step; returns (times, tracked points of the last step, good ones, selected steps)."""
        self.kfd.set_pd(0.8, 0.005, setpoint)
        self.kfd.reset()
        ts, sel = [], 0
        for i in range(n + 1):
            self.buf[:] = self.frames[i & 1]                   # the camera's write, not timed
            self.t += 0.033
            t0 = time.perf_counter()
            rc = self.L.rumi_kfd_step(self.kfd._s, self.bufp, W, H, self.stride, 1, self.t, C.byref(self.out))
            dt = time.perf_counter() - t0
            assert rc == 0, self.capi.lib().rumi_last_error()
            if i:
                ts.append(dt)
                sel += self.out.selected
        return ts, self.out.n_tracked, self.out.n_good, sel

    def extracts(self, n):
        cap = ORB[0] + 4 * ORB[2] + 64
        kps, desc = np.zeros(cap, self.capi.KP_DTYPE), np.zeros((cap, 32), np.uint8)
        cnt, mono = C.c_int32(), C.c_int32()
        ts = []
        for i in range(n):
            self.buf[:] = self.frames[i & 1]
            t0 = time.perf_counter()
            rc = self.capi.lib().rumi_orb_extract(self.ext._h, self.bufp, W, H, self.stride, 0, 0, self.capi.ptr(kps), self.capi.ptr(desc), cap, C.byref(cnt), C.byref(mono))
            ts.append(time.perf_counter() - t0)
            assert rc == 0
        return ts, cnt.value


def oracle_steps(points, n):
    """The oracle's non-selecting step on one core: the same frames, the device's tracked points."""
    import kfd_scene as ks
    with tempfile.TemporaryDirectory() as d:
        L = ks.build_oracle(d)
        frames = make_frames()
        h = L.kfo_create(0.8, 0.005, NEVER)
        out = ks.KfoStep()
        L.kfo_step(h, frames[0].ctypes.data, W, H, W, 0.0, C.byref(out), None, None)
        pts = np.ascontiguousarray(points, np.float32)
        L.kfo_set_keypoints(h, pts.ctypes.data, len(pts))
        ts = []
        for i in range(1, n + 1):
            t0 = time.perf_counter()
            L.kfo_step(h, frames[i & 1].ctypes.data, W, H, W, 0.033 * i, C.byref(out), None, None)
            ts.append(time.perf_counter() - t0)
            assert not out.selected and out.n_tracked == len(pts)
        L.kfo_destroy(h)
        return ts, out.n_good


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=300)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--oracle-steps", type=int, default=5)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args()
    dev = Device()
    if a.trace:
        dev.steps(60, NEVER)
        dev.steps(60, ALWAYS)
        return
    import torch
    name = torch.cuda.get_device_name(0)

    def emit(rec):
        line = json.dumps({"device": name, **rec})
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")

    variants = [("rumi_kfd_step, non-selecting", lambda: dev.steps(a.frames, NEVER)), ("rumi_kfd_step, selecting", lambda: dev.steps(a.frames, ALWAYS)),
                ("rumi_orb_extract alone", lambda: dev.extracts(a.frames))]
    for _, fn in variants:
        fn()                                                   # warm-up of every path
    spread = [float(np.median(variants[0][1]()[0])) * 1e6 for _ in range(a.rounds)]
    emit({"probe": "step_spread", "variant": variants[0][0], "median_us": [round(x, 2) for x in spread], "relative_range": round((max(spread) - min(spread)) / min(spread), 4)})
    acc, info = {n: [] for n, _ in variants}, {}
    for _ in range(a.rounds):
        for n, fn in variants:
            r = fn()
            acc[n].append(r[0])
            info[n] = r[1:]
    for n, _ in variants:
        med = [float(np.median(r)) * 1e6 for r in acc[n]]
        mean = [float(np.mean(r)) * 1e6 for r in acc[n]]
        extra = {"n_tracked": info[n][0], "n_good": info[n][1], "selected_steps": info[n][2]} if len(info[n]) == 3 else {"n_keypoints": info[n][0]}
        emit({"probe": "step", "variant": n, "frames": a.frames, "rounds": a.rounds, "median_us": stats(med), "mean_us": stats(mean), "w": W, "h": H, "orb": list(ORB), **extra})
    # the yardstick: the oracle on one core, tracking what the device tracked after a first step
    dev.kfd.set_pd(0.8, 0.005, NEVER)
    dev.kfd.reset()
    first = dev.kfd.step(dev.frames[0], 0.0)
    pts = np.stack([first.keypoints["x"], first.keypoints["y"]], 1)
    ts, good = oracle_steps(pts, a.oracle_steps)
    emit({"probe": "oracle_step", "variant": "kfo_step on one host core, non-selecting", "steps": a.oracle_steps, "n_tracked": len(pts), "n_good": good,
          "ms": stats([t * 1e3 for t in ts])})


if __name__ == "__main__":
    main()
