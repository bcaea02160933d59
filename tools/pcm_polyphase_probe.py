"""Development probe: the device time of the two kernels that share the polyphase loop (pcm_kernels.hip: polyphase),
HIP events round back-to-back calls on one stream: lvx_pcm_convert at 16 kHz s16le and lvx_pcm_ratio at 133 / 120, each
on 32 rows of 3,200 samples (non-final calls of open segments: every row reads its history, emits its outputs and keeps
a history). The timed calls are queued behind a few large matmuls, so the kernels run back to back and the host's launch
pace stays out of the window. Run from the tree to measure (LVX_LIB_PATH: another build of the library).
usage: python tools/pcm_polyphase_probe.py"""
import sys
import numpy as np
import torch
sys.path.insert(0, ".")
from llmvox_amd import audio as A
from llmvox_amd.engine import build_engine

B, N_IN, REPS, BLOCKS = 32, 3200, 100, 5
e = build_engine(0, "fp32", "fp32", max_streams=B, max_positions=64, max_codec_frames=64)
rng = np.random.default_rng(7)
x = torch.from_numpy((rng.standard_normal((B, N_IN)) * rng.uniform(0.05, 0.5, (B, 1))).astype(np.float32)).to(e.device)
slots, finals = list(range(B)), [False] * B
big = torch.randn(8192, 8192, device=e.device)
fmt = A.AudioFormat(16000, "s16le")


def timed(fn):
    for slot in slots:
        e.pcm_reset(slot)
    for _ in range(10):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(6):
        big @ big  # (tens of ms: every call below is queued before they end)
    a.record()
    for _ in range(REPS):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / REPS


convert, ratio = [], []
for _ in range(BLOCKS):  # alternated
    convert.append(timed(lambda: e.pcm_convert(x, slots, finals, fmt)))
    ratio.append(timed(lambda: e.pcm_ratio(x, slots, finals, 133, 120)))
for slot in slots:
    e.pcm_reset(slot)
e.check_errors()
print(f"{B} rows of {N_IN} samples, us per call over {BLOCKS} windows of {REPS} calls: "
      f"pcm_convert_kernel<2, 3, 72, s16> {' '.join(f'{v:.2f}' for v in convert)} (median {np.median(convert):.2f}); "
      f"pcm_ratio_kernel {' '.join(f'{v:.2f}' for v in ratio)} (median {np.median(ratio):.2f})", flush=True)
