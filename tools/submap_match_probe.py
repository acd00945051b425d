"""rumi_submap_match at the shape of a rumination merge: 40 key-frame pairs of 2000 key-points (CloudMerging.cc:100, TUM3.yaml).  One JSON line:
device time by HIP events (two events on the null stream around the call on device-resident key-points: the table upload, the scatter, the three
kernels and the copies back, as the GPU sees them), the whole call from host arrays and from device-resident key-points by the host clock, and
the oracle (tests/cpp/submap_oracle.cc) on one core.  Both forms are checked against the oracle before anything is timed.

    python tools/submap_match_probe.py [--pairs 40] [--n 2000] [--reps 30]
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def median_ms(fn, reps, warmup=3):
    for _ in range(warmup):
        fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t)), float(np.min(t))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=40)
    ap.add_argument("--n", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=30)
    a = ap.parse_args()
    import torch
    from submap_scene import TOL, build_oracle, device_frames, probe_scene, run_oracle
    from rumi_slam_amd.submap import SubmapMatcher
    s = probe_scene(a.pairs, a.n)
    m = SubmapMatcher()
    host, dev = device_frames(s), device_frames(s, on_device=True)
    want = run_oracle(build_oracle(tempfile.mkdtemp()), s)
    L = build_oracle(tempfile.mkdtemp())
    for frames in (host, dev):
        r = m.match(frames, s.pairs, TOL)
        assert np.array_equal(np.concatenate(r.best2), want[0]) and np.array_equal(np.concatenate(r.matches), want[2])
    host_ms = median_ms(lambda: m.match(host, s.pairs, TOL), a.reps)
    dev_ms = median_ms(lambda: m.match(dev, s.pairs, TOL), a.reps)
    ev = []
    for _ in range(a.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record(torch.cuda.default_stream())
        m.match(dev, s.pairs, TOL)
        e1.record(torch.cuda.default_stream())
        torch.cuda.synchronize()
        ev.append(e0.elapsed_time(e1))
    oracle_ms = median_ms(lambda: run_oracle(L, s), max(3, a.reps // 5), warmup=1)
    print(json.dumps(dict(probe="submap_match", pairs=a.pairs, n=a.n, matches=int(want[1][-1]), reps=a.reps,
                          device_events_ms_median=round(float(np.median(ev)), 4), device_events_ms_min=round(float(np.min(ev)), 4),
                          call_host_arrays_ms_median=round(host_ms[0], 4), call_host_arrays_ms_min=round(host_ms[1], 4),
                          call_device_resident_ms_median=round(dev_ms[0], 4), call_device_resident_ms_min=round(dev_ms[1], 4),
                          oracle_one_core_ms_median=round(oracle_ms[0], 4), oracle_one_core_ms_min=round(oracle_ms[1], 4),
                          device=torch.cuda.get_device_name(0))))
    m.close()


if __name__ == "__main__":
    main()
