"""us per AR step (HIP graph replay on a side stream) for B streams by start position and call length, under
option sets in one process: does a variant's gain hold over the position range, or only where the history is
short? Each (P0, n) is the median and minimum of five calls of n steps from position P0.
usage: python tools/step_positions.py B 'opt=v,...' ['opt=v,...' ...]   (LVX_SWEEP_KV=fp8: fp8 KV cache)"""
import os
import statistics
import sys
import time

import torch
from llmvox_amd.engine import build_engine

B = int(sys.argv[1])
e = build_engine(0, "bf16", os.environ.get("LVX_SWEEP_KV", "bf16"), max_streams=B, max_positions=1024, max_codec_frames=256)
dev = e.device
torch.cuda.set_stream(torch.cuda.Stream(device=dev))
plan = torch.full((B, 1024), 100, dtype=torch.int32, device=dev)
slots = torch.arange(B, dtype=torch.int32, device=dev)
tok = torch.zeros(B, 1024, dtype=torch.int32, device=dev)


def run(P0, n, reps=5):
    ts = []
    for _ in range(reps):
        for s in range(B):
            e.set_slot(s, P0, 5)
        rowstep = torch.zeros(B, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e.ar_steps(n, slots, plan, rowstep, tok)
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) / n * 1e6)
    return statistics.median(ts), min(ts)


for rnd in range(2):
    for spec in sys.argv[2:] or [""]:
        for kv in spec.split(","):
            if kv:
                k, v = kv.split("=")
                e.set_option(k, int(v))
        run(384, 16, 2)  # capture
        for P0, n in ((0, 16), (128, 16), (384, 16), (624, 16), (384, 64), (384, 256)):
            med, mn = run(P0, n)
            print(f"B={B} [{spec}] P0={P0} n={n}: median {med:.1f} min {mn:.1f} us/step", flush=True)
