"""Development probe: the device time of one lvx_pcm_convert call at 8 kHz per encoding, HIP events round back-to-back
calls on one stream: 32 rows of 3,200 samples (non-final calls of open segments: every row reads its history, emits
its outputs and keeps a history), `pcm_convert_kernel<1, 3, 72, ENC>`. The timed calls are queued behind a few large
matmuls, so the kernels run back to back and the host's launch pace stays out of the window. The encodings named on the
command line are timed in alternation, five windows each; a build of another commit is timed by running this file
from that commit's tree (only the encodings it has).
usage: python tools/g711_time_probe.py [s16le ulaw alaw]"""
import sys
import numpy as np
import torch
sys.path.insert(0, ".")
from llmvox_amd.audio import AudioFormat
from llmvox_amd.engine import build_engine

B, N_IN, REPS, BLOCKS = 32, 3200, 100, 5
encodings = sys.argv[1:] or ["s16le", "ulaw", "alaw"]
e = build_engine(0, "fp32", "fp32", max_streams=B, max_positions=64, max_codec_frames=64)
rng = np.random.default_rng(7)
x = torch.from_numpy((rng.standard_normal((B, N_IN)) * rng.uniform(0.05, 0.5, (B, 1))).astype(np.float32)).to(e.device)
slots, finals = list(range(B)), [False] * B
big = torch.randn(8192, 8192, device=e.device)


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


us = {enc: [] for enc in encodings}
for _ in range(BLOCKS):  # alternated
    for enc in encodings:
        fmt = AudioFormat(8000, enc)
        us[enc].append(timed(lambda: e.pcm_convert(x, slots, finals, fmt)))
for slot in slots:
    e.pcm_reset(slot)
e.check_errors()
print(f"{B} rows of {N_IN} samples at 8 kHz, us per call over {BLOCKS} windows of {REPS} calls: "
      + "; ".join(f"{enc} {' '.join(f'{v:.2f}' for v in us[enc])} (median {np.median(us[enc]):.2f})" for enc in encodings),
      flush=True)
