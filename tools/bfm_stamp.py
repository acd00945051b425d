#!/usr/bin/env python3
"""Phase breakdown of k_bruteforce_mfma from its in-kernel cycle stamps (-DRUMI_BFM_STAMP, tools/build_stamp_lib.sh): one ring launch over
B random frames of 1096 descriptors; wave 0 of the first workgroup of pair 0 prints the cycles it spent issuing the stage loads, in the MFMA
chains, in the key loops, in the staging stores and at the barrier.
    python tools/with_lib.py tools/bin/librumi_hip_bfm_stamp.so tools/bfm_stamp.py [B]"""
import sys

import numpy as np
import torch

from rumi_slam_amd.matcher import bruteforce_ring

B = int(sys.argv[1]) if len(sys.argv) > 1 else 256
cap = 1096
rng = np.random.default_rng(1)
desc = torch.from_numpy(rng.integers(0, 256, (B, cap, 32), dtype=np.uint8)).cuda()
counts = torch.from_numpy(np.stack([np.full(B, cap, np.int32), np.zeros(B, np.int32)], 1)).cuda()
out = None
for _ in range(3):
    out = bruteforce_ring(desc, counts, out=out)
    torch.cuda.synchronize()
ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
ev[0].record()
for _ in range(20):
    bruteforce_ring(desc, counts, out=out)
ev[1].record()
torch.cuda.synchronize()
print(f"bfm_probe B {B} cap {cap} ms_per_launch {ev[0].elapsed_time(ev[1]) / 20:.4f} (stamped builds print once per launch and run slower)")
