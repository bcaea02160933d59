"""us per AR step (HIP graph replay, all kernels) at positions [P0, P0+256) for B streams under
option sets; each config measured 3 times (median).
usage: python tools/step_sweep.py B P0 'opt=v,...' ['opt=v' ...]
LVX_SWEEP_STREAM=1: run on a torch side stream (the library then replays 16-step HIP graphs; on the
default (null) stream it launches every kernel). LVX_SWEEP_KV=fp8: fp8 KV cache (configs[4]).
LVX_SWEEP_W=fp32: the fp32 parity mode (fp32 weights and KV).
LVX_SWEEP_SAMPLE=T,k: every option set is measured twice in the same process, greedy as given and
then with seeded sampling (temperature T, top-k k) enabled on all B slots (the step then runs the
defer_select 0 plan with ar_sample_kernel after lm_head: compare with the set 'defer_select=0').
T,k,top_p[,R[,W]] adds a nucleus and a repetition penalty R over the last W tokens (1 and 64 when left
out); several sets separated by ';' are measured one after the other."""
import os, statistics, sys, time
import torch
from llmvox_amd.engine import build_engine

B, P0 = int(sys.argv[1]), int(sys.argv[2])
WD = os.environ.get("LVX_SWEEP_W", "bf16")
e = build_engine(0, WD, "fp32" if WD == "fp32" else os.environ.get("LVX_SWEEP_KV", "bf16"), max_streams=B, max_positions=P0 + 512, max_codec_frames=256)
dev = e.device
plan = torch.full((B, P0 + 256), 100, dtype=torch.int32, device=dev)
slots = torch.arange(B, dtype=torch.int32, device=dev)
tok = torch.zeros(B, P0 + 256, dtype=torch.int32, device=dev)
side = torch.cuda.Stream(device=dev) if os.environ.get("LVX_SWEEP_STREAM") == "1" else None
if side is not None:
    torch.cuda.set_stream(side)
SAMPLE = os.environ.get("LVX_SWEEP_SAMPLE")
runs = [(spec, smp) for spec in (sys.argv[3:] or [""]) for smp in ([None] + SAMPLE.split(";") if SAMPLE else [None])]
for spec, smp in runs:
    opts = [kv.split("=") for kv in spec.split(",") if kv]
    for k, v in opts:
        e.set_option(k, int(v))
    if smp:
        f = smp.split(",")
        T, topk = f[0], f[1]
        extra = {}
        if len(f) > 2:  # only then does the call name the extended parameters
            extra = {"top_p": float(f[2]), "repetition_penalty": float(f[3]) if len(f) > 3 else 1.0,
                     "repetition_window": int(f[4]) if len(f) > 4 else 64}
        for s in range(B):
            e.set_sampling(s, float(T), int(topk), 1000 + s, **extra)
    ts = []
    for rep in range(3):
        for s in range(B):
            e.set_slot(s, P0, 5)
        rowstep = torch.zeros(B, dtype=torch.int32, device=dev)
        e.ar_steps(16, slots, plan, rowstep, tok)  # warm / capture
        torch.cuda.synchronize()
        for s in range(B):
            e.set_slot(s, P0, 5)
        rowstep.zero_()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e.ar_steps(256, slots, plan, rowstep, tok)
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) / 256 * 1e6)
    us = statistics.median(ts)
    print(f"B={B} P={P0}.. [{spec}]{' +sample ' + smp if smp else ''}: {us:7.1f} us/step  {B / us * 1e6:9.0f} tok/s", flush=True)
    if smp:
        for s in range(B):
            e.set_sampling(s, 0.0, 0, 0)
    for k, v in opts:
        e.set_option(k, {"bt": 1, "defer_select": 1, "fuse_mlp": 1, "codec_g2": 1, "codec_g3": 1, "codec_skinny": 1, "f32b": 1, "ln_max": 8, "l0q": 1, "l0a": 1, "laf": 1, "xfold": 1, "lmf": 1}.get(k, 0))
