"""Development probe: the pause stage's device time beside the level and the formant stage's on the same dumps, HIP
events round back-to-back calls on one stream: lvx_pcm_pause on the s16le rows of a 16 kHz format and on the f32le rows
of a 24 kHz one, lvx_pcm_level at volume 250 and lvx_pcm_formant at 5 / 4 on the dump's 24 kHz rows, each on 32 rows
(non-final calls of open segments: every row reads what its slot kept, emits its blocks and keeps its last samples), at
a dump of 10 frames (3,200 samples a row at 24 kHz), of 30 (9,600) and at the largest codec call there is (1,280 frames:
409,600 samples). The pause stage's rows start 3 samples into their tensor's rows, as a segment's count leaves them: no
16-byte alignment. The timed calls are queued behind a few large matmuls, so the kernels run back to back and the
host's launch pace stays out of the window. usage: python tools/pause_time_probe.py"""
import sys
import numpy as np
import torch
sys.path.insert(0, ".")
from llmvox_amd import _lib
from llmvox_amd.audio import AudioFormat
from llmvox_amd.engine import build_engine

B, BLOCKS = 32, 5
e = build_engine(0, "fp32", "fp32", max_streams=B, max_positions=64, max_codec_frames=64)
rng = np.random.default_rng(7)
slots, finals = list(range(B)), [False] * B
big = torch.randn(8192, 8192, device=e.device)
S16, F32 = AudioFormat(16000, "s16le", pause_ms=0), AudioFormat(24000, "f32le", pause_ms=0)


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
    host = (rng.standard_normal((B, n_in + 3)) * rng.uniform(0.001, 0.5, (B, 1))).astype(np.float32)
    x = torch.from_numpy(host[:, 3:].copy()).to(e.device)
    f32 = torch.from_numpy(host).to(e.device)[:, 3:]
    n16 = n_in * 2 // 3
    s16 = torch.from_numpy(np.clip(np.rint(host[:, :n16 + 3] * 32768), -32768, 32767).astype(np.int16)).to(e.device)[:, 3:]
    times = {"pcm_pause_kernel s16le 16 kHz": [], "pcm_pause_kernel f32le 24 kHz": [], "pcm_level_kernel": [],
             "pcm_formant_kernel": []}
    for _ in range(BLOCKS):  # alternated
        times["pcm_pause_kernel s16le 16 kHz"].append(timed(lambda: e.pcm_pause(s16, slots, finals, S16), reps))
        times["pcm_pause_kernel f32le 24 kHz"].append(timed(lambda: e.pcm_pause(f32, slots, finals, F32), reps))
        times["pcm_level_kernel"].append(timed(lambda: e.pcm_level(x, slots, finals, 250), reps))
        times["pcm_formant_kernel"].append(timed(lambda: e.pcm_formant(x, slots, finals, 5, 4), reps))
    print(f"{B} rows of a dump of {n_in} samples at 24 kHz, median us per call over {BLOCKS} windows of {reps} calls: "
          + "; ".join(f"{k} {np.median(v):.1f} ({min(v):.1f} .. {max(v):.1f})" for k, v in times.items()), flush=True)
for slot in slots:
    e.pcm_reset(slot)
e.check_errors()
