#!/usr/bin/env python3
"""Measurements behind the streaming front-end, one JSON record per line on standard output and, with
--out FILE, appended to that file (the quoted copy lives in profiles/):

  kernel   k_bruteforce_pair (automatic slice count, then every forced count) against k_bruteforce_mfma at nbatch = 1, for 1000 x 1000 and
           500 x 500 descriptors: HIP-event time per launch over --launches back-to-back launches, variants alternated --rounds times, the
           run-to-run spread of one variant first.
  call     rumi_orb_stream_push on the pinned capture buffer (640 x 480, 1000 features, --frames frames) against the best a caller could do
           without it -- upload, rumi_orb_extract_batch_device_async with one frame, rumi_match_bruteforce_batch_device with one pair, six copies to
           pinned memory, one synchronisation -- through the same ctypes layer, alternated; the Python mirror (FrameStream.push) next to them;
           the extractor's per-stage times with profiling on.
  --trace  only launches the two kernels (for a separate rocprofv3 --kernel-trace --stats pass; nothing is timed or written).

Needs a GPU: there is no fallback."""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def event_us(fn, launches):
    import torch
    for _ in range(20):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(launches):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1000.0 / launches


def stats(xs):
    xs = sorted(xs)
    return {"min": round(xs[0], 2), "median": round(xs[len(xs) // 2], 2), "max": round(xs[-1], 2)}


def kernel_variants(n):
    import numpy as np
    import torch
    from rumi_slam_amd import matcher as M
    cap = n + 96                                              # the extractor's capacity for n features on 8 levels
    rng = np.random.default_rng(n)
    q = torch.from_numpy(rng.integers(0, 256, (1, cap, 32), dtype=np.uint8)).cuda()
    t = torch.from_numpy(rng.integers(0, 256, (1, cap, 32), dtype=np.uint8)).cuda()
    cnt = torch.tensor([[n, 0]], dtype=torch.int32, device="cuda")
    out = [torch.empty((1, cap), dtype=torch.int32, device="cuda") for _ in range(3)]
    out1 = [o[0] for o in out]
    scratch = M.bruteforce_pair_scratch(cap, "cuda")
    L, st = M._lib(), torch.cuda.current_stream().cuda_stream
    mx = min((cap + 63) // 64, 64)

    def batch():
        L.rumi_match_bruteforce_batch_device(q.data_ptr(), cnt.data_ptr(), t.data_ptr(), cnt.data_ptr(), 2, cap, 1, out[0].data_ptr(), out[1].data_ptr(),
                                             out[2].data_ptr(), st)

    def pair(s):
        return lambda: L.rumi_match_bruteforce_pair_device(q.data_ptr(), cnt.data_ptr(), t.data_ptr(), cnt.data_ptr(), cap, s, scratch.data_ptr(),
                                                           out1[0].data_ptr(), out1[1].data_ptr(), out1[2].data_ptr(), st)
    variants = [("k_bruteforce_mfma nbatch=1", batch), ("k_bruteforce_pair auto", pair(0))] + [(f"k_bruteforce_pair slices={s}", pair(s)) for s in range(1, mx + 1)]
    # the results agree before anything is timed
    batch(); torch.cuda.synchronize()
    ref = [o[0, :n].clone() for o in out]
    for name, fn in variants[1:]:
        for o in out1:
            o.fill_(-9)
        fn(); torch.cuda.synchronize()
        assert all(torch.equal(o[:n], r) for o, r in zip(out1, ref)), name
    return cap, variants, M.bruteforce_pair_shape(cap, cap, 0)


def probe_kernels(emit, launches, rounds):
    for n in (1000, 500):
        cap, variants, auto = kernel_variants(n)
        spread = [event_us(variants[0][1], launches) for _ in range(rounds)]
        emit({"probe": "kernel_spread", "n": n, "cap": cap, "variant": variants[0][0], "us_per_launch": [round(x, 2) for x in spread],
              "relative_range": round((max(spread) - min(spread)) / min(spread), 4)})
        times = {name: [] for name, _ in variants}
        for _ in range(rounds):                               # alternate the variants
            for name, fn in variants:
                times[name].append(event_us(fn, launches))
        for name, _ in variants:
            emit({"probe": "kernel", "n": n, "cap": cap, "variant": name, "launches": launches, "us_per_launch": stats(times[name]),
                  **({"auto_shape": {"slices": auto[0], "rows_per_slice": auto[1]}} if name.endswith("auto") else {})})


def trace_kernels(launches):
    import torch
    cap, variants, _ = kernel_variants(1000)
    for name, fn in variants[:2]:
        for _ in range(launches):
            fn()
        torch.cuda.synchronize()


def probe_calls(emit, frames, rounds):
    import numpy as np
    import torch
    from rumi_slam_amd import capi
    from rumi_slam_amd import matcher as M
    from rumi_slam_amd.extractor import ORBextractor
    from rumi_slam_amd.stream import FrameStream
    from rumi_slam_amd.synth import synth_frame, warp_frame
    W, H, NF = 640, 480, 1000
    imgs = [synth_frame(777)]
    for i in range(7):
        imgs.append(warp_frame(imgs[-1], 900 + i)[0])
    L = capi.lib()
    Lm = M._lib()

    # the stream, through the C entry, on the pinned capture buffer
    ext = ORBextractor(NF, 1.2, 8, 20, 7)
    fs = FrameStream(ext)
    buf = ext.image_buffer(W, H)
    bufp, stride = C.c_void_p(buf.ctypes.data), buf.strides[0]
    frame = capi.RumiStreamFrame()

    def run_push():
        ts = []
        for i in range(frames):
            buf[:] = imgs[i % len(imgs)]                       # the camera's write, not timed
            t0 = time.perf_counter()
            rc = L.rumi_orb_stream_push(fs._s, bufp, W, H, stride, 0, 1000, C.byref(frame))
            ts.append(time.perf_counter() - t0)
            assert rc == 0 and frame.n > 0, rc
        return ts

    def run_mirror():
        ts = []
        for i in range(frames):
            buf[:] = imgs[i % len(imgs)]
            t0 = time.perf_counter()
            fs.push(buf)
            ts.append(time.perf_counter() - t0)
        return ts

    # what a caller could do before: upload, batched extraction of one frame, batch matcher with one pair, six copies to pinned memory
    ext_b = ORBextractor(NF, 1.2, 8, 20, 7)
    cap = NF + 4 * 8 + 64
    dev = torch.device("cuda", 0)
    pinned_img = torch.zeros((1, H, W), dtype=torch.uint8).pin_memory()
    d_img = torch.zeros((1, H, W), dtype=torch.uint8, device=dev)
    slots = [(torch.zeros((1, cap, 7), dtype=torch.float32, device=dev), torch.zeros((1, cap, 32), dtype=torch.uint8, device=dev),
              torch.zeros((1, 2), dtype=torch.int32, device=dev)) for _ in range(2)]
    res = [torch.zeros((1, cap), dtype=torch.int32, device=dev) for _ in range(3)]
    host = [torch.zeros((1, cap, 7), dtype=torch.float32).pin_memory(), torch.zeros((1, cap, 32), dtype=torch.uint8).pin_memory(),
            torch.zeros((1, 2), dtype=torch.int32).pin_memory()] + [torch.zeros((1, cap), dtype=torch.int32).pin_memory() for _ in range(3)]
    st = torch.cuda.current_stream(dev).cuda_stream
    pin_np = pinned_img.numpy()

    def run_baseline(upload):
        ts = []
        for i in range(frames):
            pin_np[0] = imgs[i % len(imgs)]
            if not upload:
                d_img.copy_(pinned_img); torch.cuda.synchronize()
            kp, desc, cnt = slots[i & 1]
            pk, pd, pc = slots[(i + 1) & 1]
            t0 = time.perf_counter()
            if upload:
                d_img.copy_(pinned_img, non_blocking=True)
            rc = L.rumi_orb_extract_batch_device_async(ext_b._h, d_img.data_ptr(), 1, W, H, W, W * H, 0, 1000, kp.data_ptr(), desc.data_ptr(), cnt.data_ptr(), cap, st)
            rc |= Lm.rumi_match_bruteforce_batch_device(desc.data_ptr(), cnt.data_ptr(), pd.data_ptr(), pc.data_ptr(), 2, cap, 1, res[0].data_ptr(),
                                                        res[1].data_ptr(), res[2].data_ptr(), st)
            for hdst, src in zip(host, (kp, desc, cnt, *res)):
                hdst.copy_(src, non_blocking=True)
            torch.cuda.synchronize()
            rc |= L.rumi_orb_sync(ext_b._h)
            ts.append(time.perf_counter() - t0)
            assert rc == 0
        return ts

    variants = [("rumi_orb_stream_push (C entry, pinned capture buffer)", run_push),
                ("baseline: upload + extract_batch_device(1) + bruteforce_batch_device(1) + 6 copies", lambda: run_baseline(True)),
                ("baseline without the upload (device-resident frame)", lambda: run_baseline(False)),
                ("FrameStream.push (Python mirror, with its copies)", run_mirror)]
    for _, fn in variants:
        fn()                                                  # warm-up of every path
    spread = [float(np.median(run_push())) * 1e6 for _ in range(rounds)]
    emit({"probe": "call_spread", "variant": variants[0][0], "median_us": [round(x, 2) for x in spread], "relative_range": round((max(spread) - min(spread)) / min(spread), 4)})
    acc = {name: [] for name, _ in variants}
    for _ in range(rounds):
        for name, fn in variants:
            acc[name].append(fn())
    for name, _ in variants:
        med = [float(np.median(r)) * 1e6 for r in acc[name]]
        mean = [float(np.mean(r)) * 1e6 for r in acc[name]]
        m = sorted(med)[len(med) // 2]
        emit({"probe": "call", "variant": name, "frames": frames, "rounds": rounds, "median_us_per_frame": stats(med), "mean_us_per_frame": stats(mean),
              "fps_at_median": round(1e6 / m, 1), "w": W, "h": H, "nfeatures": NF})
    # where a push spends its device time: the extractor's stages with profiling on (the push then takes its copy path), and the pair kernel above
    ext.set_profiling(True)
    for i in range(5):
        buf[:] = imgs[i % len(imgs)]
        fs.push(buf)
    emit({"probe": "push_stage_ms_profiled", "stages": {k: round(float(v), 4) for k, v in ext.stage_ms().items()},
          "note": "HIP events around the extraction's stages inside a profiled push (one stream, copies instead of the mirror); the match is the kernel probe's figure"})
    ext.set_profiling(False)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--frames", type=int, default=500)
    ap.add_argument("--only", choices=["kernel", "call"], default=None)
    ap.add_argument("--trace", action="store_true")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("stream_probe.py needs a GPU")
    if args.trace:
        trace_kernels(args.launches)
        return
    f = open(args.out, "a") if args.out else None

    def emit(rec):
        line = json.dumps({"device": torch.cuda.get_device_name(0), **rec})
        if f:
            f.write(line + "\n"); f.flush()
        print(line, flush=True)
    if args.only in (None, "kernel"):
        probe_kernels(emit, args.launches, args.rounds)
    if args.only in (None, "call"):
        probe_calls(emit, args.frames, args.rounds)
    if f:
        f.close()


if __name__ == "__main__":
    main()
