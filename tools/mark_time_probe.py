"""Development probe: the watermark stage's device time beside the formant and the level stages' on the same rows in the
same run, HIP events round back-to-back calls on one stream: lvx_pcm_mark at strength 2, lvx_pcm_formant at 5 / 4 and
lvx_pcm_level at volume 250, each on 32 rows (non-final calls of open segments: every row reads its history, emits its
hop blocks and keeps a history), at a dump of 10 frames (3,200 samples a row), of 30 (9,600) and at the largest codec
call there is (1,280 frames: 409,600 samples, 1,600 hops a row). The timed calls are queued behind a few large matmuls,
so the kernels run back to back and the host's launch pace stays out of the window. The three stages are timed in
alternation, five windows each, with the launch's own choice of the hop blocks a workgroup writes (option fmt_group 0).
usage: python tools/mark_time_probe.py"""
import sys
import numpy as np
import torch
sys.path.insert(0, ".")
from llmvox_amd import _lib
from llmvox_amd.engine import build_engine

B, BLOCKS = 32, 5
KEY = 0x5EEDC0DEF00DFACE
e = build_engine(0, "fp32", "fp32", max_streams=B, max_positions=64, max_codec_frames=64)
rng = np.random.default_rng(7)
slots, finals = list(range(B)), [False] * B
big = torch.randn(8192, 8192, device=e.device)


def timed(fn, reps):
    for slot in slots:
        e.pcm_reset(slot)
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(6):
        big @ big  # (tens of ms: every call below is queued before they end)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / reps


print(f"library {_lib.LIB_PATH}", flush=True)
for n_in, reps in ((3200, 100), (9600, 100), (409600, 5)):
    x = torch.from_numpy((rng.standard_normal((B, n_in)) * rng.uniform(0.05, 0.5, (B, 1))).astype(np.float32)).to(e.device)
    stages = {"pcm_mark_kernel": lambda: e.pcm_mark(x, slots, finals, KEY, 0xA5, 2),
              "pcm_formant_kernel": lambda: e.pcm_formant(x, slots, finals, 5, 4),
              "pcm_level_kernel": lambda: e.pcm_level(x, slots, finals, 250)}
    times = {name: [] for name in stages}
    for _ in range(BLOCKS):  # alternated
        for name, fn in stages.items():
            times[name].append(timed(fn, reps))
    print(f"{B} rows of {n_in} samples, median us per call over {BLOCKS} windows of {reps} calls: "
          + "; ".join(f"{name} {np.median(v):.1f} ({min(v):.1f} .. {max(v):.1f})" for name, v in times.items()), flush=True)
for slot in slots:
    e.pcm_reset(slot)
e.check_errors()
