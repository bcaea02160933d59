"""The watermark's detector on the command line:

    python -m llmvox_amd.watermark detect FILE.wav --key K [--window-s 3.0]

prints the verdict of ``audio.mark_detect`` for a mono WAV of any of the service's rates (8, 16, 24 or 48 kHz) with
float32, 16-bit PCM or G.711 (mu-law, A-law) samples: what the service delivers with ``"container": "wav"``, whose
header leaves the sizes open (0xFFFFFFFF), and what a tool that rewrote it with real sizes made of it. Host numpy only:
it works on audio that has left the service. The exit status is 0 where a mark was found, 1 where none was, 2 for a
file it cannot read. The key is read, never printed."""
from __future__ import annotations

import argparse
import struct
import sys
from typing import Tuple

import numpy as np

from . import audio as A

_TAGS = {(1, 16): "s16le", (3, 32): "f32le", (7, 8): "ulaw", (6, 8): "alaw"}


def read_wav(data: bytes) -> Tuple[np.ndarray, int, str]:
    """(float32 samples, sample rate, encoding) of a mono RIFF / WAVE file; ValueError for anything else. A chunk size
    of 0xFFFFFFFF (a stream of unknown length) reaches to the end of the file."""
    if len(data) < 12 or data[:4] != b"RIFF" or data[8:12] != b"WAVE":
        raise ValueError("not a RIFF / WAVE file")
    at, fmt, body = 12, None, None
    while at + 8 <= len(data):
        name, size = data[at:at + 4], struct.unpack("<I", data[at + 4:at + 8])[0]
        end = len(data) if size == 0xFFFFFFFF else min(at + 8 + size, len(data))
        if name == b"fmt ":
            if end - (at + 8) < 16:
                raise ValueError("a fmt chunk shorter than 16 bytes")
            fmt = struct.unpack("<HHIIHH", data[at + 8:at + 24])
        elif name == b"data":
            body = data[at + 8:end]
            break
        at = end + ((end - at) & 1)  # (chunks are padded to even sizes)
    if fmt is None or body is None:
        raise ValueError("no fmt chunk in front of a data chunk")
    tag, channels, rate, _, _, bits = fmt
    encoding = _TAGS.get((tag, bits))
    if channels != 1 or encoding is None:
        raise ValueError(f"format tag {tag} with {bits} bits and {channels} channel(s): not mono f32le, s16le, mu-law or A-law")
    if rate not in A.RATES:
        raise ValueError(f"sample rate {rate}: not one of {sorted(A.RATES)}")
    dtype = A.AudioFormat(rate, encoding).dtype
    raw = np.frombuffer(body[:len(body) // dtype.itemsize * dtype.itemsize], dtype=dtype)
    if encoding in A.G711_LAWS:
        raw = A.g711_decode(raw, encoding)
    x = raw.astype(np.float32) if encoding == "f32le" else raw.astype(np.float32) / np.float32(32768.0)
    return x, rate, encoding


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(prog="python -m llmvox_amd.watermark")
    sub = ap.add_subparsers(dest="command", required=True)
    det = sub.add_parser("detect", help="look for the service's mark in a WAV file")
    det.add_argument("file")
    det.add_argument("--key", type=lambda v: int(v, 0), required=True, help="the service's watermark key (an integer; 0x... for hexadecimal)")
    det.add_argument("--window-s", type=float, default=None,
                     help="search windows of this many seconds and report the best (a request of several sentences: every "
                          "sentence restarts the pattern; default: the whole file as one)")
    a = ap.parse_args(argv)
    try:
        with open(a.file, "rb") as f:
            x, rate, encoding = read_wav(f.read())
        S, found, mark_id, offset = A.mark_detect(x, rate, a.key, a.window_s)
    except (OSError, ValueError) as e:
        print(f"error: {e}", file=sys.stderr)
        return 2
    print(f"file: {a.file}: {x.size} samples, {rate} Hz, {encoding}")
    print(f"score: S = {S:.2f} (a mark is reported at S >= {A.MARK_DETECT_MIN:.0f})")
    if found:
        print(f"watermark: found, id {mark_id} (0x{mark_id:02x}), blocks start at sample {offset} of the 24 kHz signal")
    else:
        print("watermark: not found")
    return 0 if found else 1


if __name__ == "__main__":
    sys.exit(main())
