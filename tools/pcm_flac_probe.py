"""Development probe: the device time of pcm_flac_kernel next to pcm_convert_kernel's s16le call on the same rows, and
the host time of lvx_flac_finish per frame. HIP events round back-to-back calls on one stream (non-final calls of open
segments: every row reads what its slot kept, emits its frames and keeps the rest), queued behind a few large matmuls so
that the host's launch pace stays out of the window; the two calls alternate in windows. Shapes: 32 rows of one 32-step
chunk (10,240 samples at 24 kHz) delivered at 24 kHz and at 8 kHz, and 8,192 codec frames as 32 rows of 256 at 24 kHz.
The signal is a voiced one (harmonics of a wobbling 110 Hz under a syllable envelope, a little noise), which takes the
FIXED path. Run from the tree to measure (LVX_LIB_PATH: another build of the library).
usage: python tools/pcm_flac_probe.py"""
import sys
import time

import numpy as np
import torch

sys.path.insert(0, ".")
from llmvox_amd import audio as A
from llmvox_amd.engine import build_engine

B, REPS, BLOCKS = 32, 50, 5
e = build_engine(0, "fp32", "fp32", max_streams=B, max_positions=64, max_codec_frames=64)
big = torch.randn(8192, 8192, device=e.device)
slots, finals = list(range(B)), [False] * B


def voiced(n, seed):
    rng = np.random.default_rng(seed)
    t = np.arange(n) / 24000.0
    phase = 2 * np.pi * np.cumsum(110.0 * (1.0 + 0.04 * np.sin(2 * np.pi * 3.1 * t))) / 24000.0
    x = sum(np.sin(h * phase + 0.7 * h) / h for h in range(1, 12))
    env = 0.15 + 0.85 * np.sin(np.pi * np.minimum(1.0, (t * 4.0) % 1.0 / 0.8)) ** 2
    return (0.14 * env * x + rng.normal(0.0, 4e-4, n)).astype(np.float32)


def timed(fn):
    for slot in slots:
        e.pcm_reset(slot)
    for _ in range(5):
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


for n_in, rate in ((10240, 24000), (10240, 8000), (81920, 24000)):
    x = torch.from_numpy(np.stack([voiced(n_in, b) for b in range(B)])).to(e.device)
    fmt = A.AudioFormat(rate, "s16le")
    s16, cnt = e.pcm_convert(x, slots, [True] * B, fmt)
    s16 = s16[:, :cnt[0]].contiguous()
    conv, flac = [], []
    for _ in range(BLOCKS):  # alternated
        conv.append(timed(lambda: e.pcm_convert(x, slots, finals, fmt)))
        flac.append(timed(lambda: e.pcm_flac(s16, slots, finals, rate)))
    for slot in slots:
        e.pcm_reset(slot)
    out, frames = e.pcm_flac(s16, slots, [True] * B, rate)
    host = out.cpu().numpy()
    size = A.flac_slot_bytes(rate)
    blobs = [host[b, :frames[b] * size].tobytes() for b in range(B)]
    best = []
    for _ in range(BLOCKS):
        mux, n_bytes = A.FlacMux(rate), 0
        t0 = time.perf_counter()
        for blob in blobs:
            n_bytes += len(mux.push(blob))
        best.append((time.perf_counter() - t0) * 1e6 / sum(frames))
    print(f"{B} rows of {n_in} samples at 24 kHz delivered at {rate} Hz ({s16.shape[1]} s16 a row, {sum(frames)} frames, "
          f"{n_bytes / (2 * B * s16.shape[1]):.3f} of the s16le bytes), us per call over {BLOCKS} windows of {REPS} calls: "
          f"pcm_convert_kernel s16le {' '.join(f'{v:.2f}' for v in conv)} (median {np.median(conv):.2f}); "
          f"pcm_flac_kernel {' '.join(f'{v:.2f}' for v in flac)} (median {np.median(flac):.2f}); "
          f"lvx_flac_finish on the host, us per frame: {' '.join(f'{v:.2f}' for v in best)} (median {np.median(best):.2f})",
          flush=True)
e.check_errors()
