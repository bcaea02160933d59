"""Development probe: the dump join's own time beside the codec call that feeds it, HIP events round back-to-back
calls on one stream. The shape is a joined stream's third dump, 16 context frames and 90 new ones, for 32
streams: lvx_pcm_join on 32 rows of 106 frames (non-final, every slot open with context, so every row crossfades,
copies its body and keeps a tail) and lvx_codec_decode_codes of [32, 106]. usage: python tools/join_time_probe.py"""
import sys
import torch
sys.path.insert(0, ".")
from llmvox_amd.engine import build_engine

B, FRAMES, CTX, REPS = 32, 106, 16, 50
e = build_engine(0, "bf16", "bf16", max_streams=B, max_positions=64, max_codec_frames=B * FRAMES)
s = torch.cuda.Stream()
torch.cuda.set_stream(s)
codes = torch.randint(0, 4096, (B, FRAMES), dtype=torch.int32).to(e.device)
pcm = torch.empty(B, 320 * FRAMES, device=e.device)
slots = list(range(B))


def timed(fn):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(s)
    for _ in range(REPS):
        fn()
    b.record(s)
    b.synchronize()
    return a.elapsed_time(b) / REPS


codec_ms = timed(lambda: e.decode_codes(codes, 0, out=pcm))
e.pcm_join(pcm, slots, [0] * B, [False] * B)  # (opens every slot: the timed calls carry context)
join_ms = timed(lambda: e.pcm_join(pcm, slots, [CTX] * B, [False] * B))
for slot in slots:
    e.pcm_reset(slot)
e.check_errors()
moved = B * (2 * 320 * (FRAMES - CTX) + 2 * 320 + 2 * 320) * 4  # body in and out, the crossfade's two inputs, the tail in and out
print(f"{B} rows of {FRAMES} frames: codec decode {codec_ms:.3f} ms, dump join {join_ms * 1e3:.1f} us "
      f"({moved / 1e6:.2f} MB moved, {moved / join_ms / 1e6:.1f} GB/s with the call's host side and its output allocation; "
      f"{100 * join_ms / codec_ms:.2f} % of the codec call)", flush=True)
