"""A decoder of the FLAC subset the service emits (mono, 16 bits, variable blocksize, CONSTANT / VERBATIM / FIXED
subframes with Rice partitions), written from the format: its own bit reader and its own bitwise CRCs; nothing of
llmvox_amd is imported. ``decode(data)`` checks, and raises FlacError where it fails: the stream header, every frame's
sync and codes, the CRC-8 and the CRC-16, that sample numbers are contiguous from ``first_sample``, and that every block
size is within STREAMINFO's bounds but for a last frame shorter than the minimum. Returns (int16 samples, frames), a
frame being (sample number, block size, subframe kind, bytes of the frame); kind: "constant", "verbatim", "fixed0" ..
"fixed4"."""
import numpy as np

RATE_CODES = {4: 8000, 5: 16000, 7: 24000, 10: 48000}


class FlacError(ValueError):
    pass


def _need(cond, what):
    if not cond:
        raise FlacError(what)


def crc8(data) -> int:
    c = 0
    for b in data:
        c ^= b
        for _ in range(8):
            c = ((c << 1) ^ 0x07) & 0xFF if c & 0x80 else (c << 1) & 0xFF
    return c


def crc16(data) -> int:
    c = 0
    for b in data:
        c ^= b << 8
        for _ in range(8):
            c = ((c << 1) ^ 0x8005) & 0xFFFF if c & 0x8000 else (c << 1) & 0xFFFF
    return c


class Bits:
    """MSB-first reader over the unpacked bits of ``data`` from byte ``at``."""

    def __init__(self, data: bytes, at: int):
        self.bits = np.unpackbits(np.frombuffer(data, dtype=np.uint8))
        self.ones = np.flatnonzero(self.bits)
        self.pos = 8 * at

    def read(self, n: int) -> int:
        _need(self.pos + n <= self.bits.size, "the stream ends inside a field")
        v = 0
        for b in self.bits[self.pos:self.pos + n]:
            v = (v << 1) | int(b)
        self.pos += n
        return v

    def signed(self, n: int) -> int:
        v = self.read(n)
        return v - (1 << n) if v >> (n - 1) else v

    def unary(self) -> int:
        """Zeros in front of the next one (which is consumed)."""
        i = int(np.searchsorted(self.ones, self.pos))
        _need(i < self.ones.size, "the stream ends inside a unary run")
        zeros = int(self.ones[i]) - self.pos
        self.pos += zeros + 1
        return zeros

    def align(self):
        pad = -self.pos % 8
        _need(self.read(pad) == 0 if pad else True, "the padding of a frame is not zero")

    @property
    def byte(self) -> int:
        return self.pos // 8


def _stream_info(data: bytes):
    _need(len(data) >= 42 and data[:4] == b"fLaC", "no fLaC marker")
    _need(data[4] == 0x80 and data[5:8] == bytes([0, 0, 34]), "the first block is not a last STREAMINFO block of 34 bytes")
    b = Bits(data, 8)
    info = {"min_bs": b.read(16), "max_bs": b.read(16), "min_frame": b.read(24), "max_frame": b.read(24),
            "rate": b.read(20), "channels": b.read(3) + 1, "bps": b.read(5) + 1, "total": b.read(36)}
    info["md5"] = data[26:42]
    _need(info["channels"] == 1 and info["bps"] == 16, "not mono 16 bit")
    _need(info["rate"] in RATE_CODES.values(), "not a rate of the service")
    _need(16 <= info["min_bs"] <= info["max_bs"], "block size bounds out of order")
    return info


def _utf8(data: bytes, at: int):
    first = data[at]
    if first < 0x80:
        return first, 1
    n = 0
    while n < 8 and first & (0x80 >> n):
        n += 1
    _need(2 <= n <= 7, "a bad first byte of the coded sample number")
    v = first & (0x7F >> n)
    for i in range(1, n):
        _need(data[at + i] & 0xC0 == 0x80, "a bad continuation byte of the coded sample number")
        v = (v << 6) | (data[at + i] & 0x3F)
    _need(n == 1 or v >= (1 << (5 * (n - 1) + 1 if n > 2 else 7)), "the sample number is coded longer than needed")
    return v, n


def _subframe(b: Bits, n: int):
    _need(b.read(1) == 0, "the subframe's padding bit is set")
    kind = b.read(6)
    _need(b.read(1) == 0, "wasted bits are not used")
    if kind == 0:
        return np.full(n, b.signed(16), dtype=np.int64), "constant"
    if kind == 1:
        return np.array([b.signed(16) for _ in range(n)], dtype=np.int64), "verbatim"
    _need(8 <= kind <= 12, f"subframe type {kind} is none of constant, verbatim, fixed 0 .. 4")
    order = kind - 8
    _need(order <= n, "more warm-up samples than the block has")
    x = [b.signed(16) for _ in range(order)]
    _need(b.read(2) == 0, "not the 4-bit Rice coding method")
    P = b.read(4)
    _need(n % (1 << P) == 0 and (n >> P) >= order, "the partition order does not fit the block")
    res = []
    for j in range(1 << P):
        k = b.read(4)
        _need(k != 15, "the escape code is never used")
        for _ in range((n >> P) - (order if j == 0 else 0)):
            u = (b.unary() << k) | (b.read(k) if k else 0)
            res.append((u >> 1) ^ -(u & 1))
    coef = [[], [1], [2, -1], [3, -3, 1], [4, -6, 4, -1]][order]
    for r in res:
        x.append(r + sum(c * x[-1 - t] for t, c in enumerate(coef)))
    return np.array(x, dtype=np.int64), f"fixed{order}"


def decode(data: bytes, first_sample: int = 0, header: bool = True, rate=None):
    """(samples int16, [(sample number, block size, kind, frame bytes)]) of a whole stream; ``header`` False: bare
    frames of ``rate`` (no STREAMINFO to hold the block sizes to)."""
    data = bytes(data)
    info = _stream_info(data) if header else None
    at = 42 if header else 0
    rate = info["rate"] if header else rate
    out, frames, expect = [], [], first_sample
    while at < len(data):
        _need(len(data) - at >= 10, "a truncated frame")
        _need(data[at] == 0xFF and data[at + 1] == 0xF9, "no sync code of a variable-blocksize frame")
        _need(data[at + 2] >> 4 == 0b0111, "the block size is not in 16 bits behind the header")
        _need(RATE_CODES.get(data[at + 2] & 15) == rate, "the frame's rate code is not the stream's")
        _need(data[at + 3] == 0x08, "not mono, 16 bits")
        no, ln = _utf8(data, at + 4)
        h = at + 4 + ln
        n = ((data[h] << 8) | data[h + 1]) + 1
        _need(crc8(data[at:h + 2]) == data[h + 2], "the header's CRC-8 fails")
        _need(no == expect, f"sample number {no}, expected {expect}")
        b = Bits(data, h + 3)
        x, kind = _subframe(b, n)
        b.align()
        end = b.byte
        _need(end + 2 <= len(data), "the stream ends before a frame's CRC-16")
        _need(crc16(data[at:end]) == ((data[end] << 8) | data[end + 1]), "the frame's CRC-16 fails")
        _need(x.min() >= -32768 and x.max() <= 32767, "a sample outside 16 bits")
        frames.append((no, n, kind, end + 2 - at))
        out.append(x)
        expect += n
        at = end + 2
    if header:
        for i, (_, n, _, _) in enumerate(frames):
            _need(n <= info["max_bs"], "a block larger than STREAMINFO's maximum")
            _need(n >= info["min_bs"] or i == len(frames) - 1, "a block smaller than STREAMINFO's minimum that is not the last")
    samples = np.concatenate(out).astype(np.int16) if out else np.zeros(0, dtype=np.int16)
    return samples, frames
