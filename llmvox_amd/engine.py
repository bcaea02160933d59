"""Thin Python owner of one ``lvx_ctx`` (one device): weights, KV slots, entry points.

Every compute method is asynchronous on the device's current torch stream and takes /
returns torch device tensors (torch is only the allocator and the stream provider here).
"""
from __future__ import annotations

import ctypes
from typing import Dict, Optional

import numpy as np
import torch
import torch.distributed as dist

from . import _lib
from .weights import CODEBOOK_KEY, TEXT_EMBED_KEY


def _ptr(t: Optional[torch.Tensor]):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _mark_key(key) -> int:
    # (ctypes would wrap a key outside 64 bits silently; the message does not repeat the key)
    if isinstance(key, bool) or not isinstance(key, int) or not 0 <= key < 1 << 64:
        raise ValueError("the watermark key must be an integer in 0 .. 2^64 - 1")
    return key


class Engine:
    def __init__(self, device_index: int = 0, weight_dtype: str = "fp32", kv_dtype: str = "fp32",
                 max_streams: int = 8, max_positions: int = 8192, max_codec_frames: int = 1280,
                 codec_dtype: Optional[str] = None):
        self.lib = _lib.load()
        if not torch.cuda.is_available():
            raise RuntimeError("llmvox_amd needs a ROCm GPU (MI355X); there is no CPU path")
        self.device = torch.device(f"cuda:{device_index}")
        self.device_index = device_index
        cfg = _lib.LvxConfig(device_index, _lib.DTYPES[weight_dtype], _lib.DTYPES[kv_dtype], max_streams,
                             max_positions, max_codec_frames, _lib.DTYPES[codec_dtype] if codec_dtype else 0)
        h = ctypes.c_void_p()
        with torch.cuda.device(self.device):
            _lib.check(self.lib.lvx_create(ctypes.byref(cfg), ctypes.byref(h)))
        self.h = h
        self._capture_stream = None
        self.weight_dtype = weight_dtype
        self.kv_dtype = kv_dtype
        self.codec_dtype = codec_dtype or weight_dtype
        self.max_streams = max_streams
        self.max_positions = max_positions
        self.max_codec_frames = max_codec_frames
        self.finalized = False

    # ---- weights ----------------------------------------------------------------
    def set_weight(self, name: str, arr):
        a = np.ascontiguousarray(np.asarray(arr, dtype=np.float32))
        _lib.check(self.lib.lvx_set_weight(self.h, name.encode(), a.ctypes.data_as(ctypes.c_void_p), a.size))

    def load_weights(self, gpt: Dict[str, np.ndarray], codec: Dict[str, np.ndarray], text_table: np.ndarray):
        for k, v in gpt.items():
            if k.endswith("attn.bias"):  # causal-mask buffer of the no-flash path, not a weight
                continue
            self.set_weight(k, v)
        for k, v in codec.items():
            if k == "head.istft.window":
                continue
            self.set_weight(k, v)
        self.set_weight(TEXT_EMBED_KEY, text_table)
        # exactly torch's periodic Hann window (decoder/spectral_ops.py:30-31)
        self.set_weight("head.istft.window", torch.hann_window(1280).numpy())
        with torch.cuda.device(self.device):
            _lib.check(self.lib.lvx_finalize(self.h))
        self.finalized = True

    # ---- helpers ----------------------------------------------------------------
    def stream_handle(self):
        return ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    # ---- drop-in members -------------------------------------------------------------
    def text_embed(self, ids: torch.Tensor) -> torch.Tensor:
        ids = ids.to(self.device, torch.int64).contiguous()
        out = torch.empty(*ids.shape, 256, device=self.device, dtype=torch.float32)
        _lib.check(self.lib.lvx_text_embed(self.h, _ptr(ids), ids.numel(), _ptr(out), self.stream_handle()))
        return out

    def codes_to_features(self, codes: torch.Tensor) -> torch.Tensor:
        """codes int [B, L] -> [B, 512, L]."""
        codes = codes.to(self.device, torch.int64).contiguous()
        B, L = codes.shape
        out = torch.empty(B, 512, L, device=self.device, dtype=torch.float32)
        _lib.check(self.lib.lvx_codes_to_features(self.h, _ptr(codes), B, L, _ptr(out), self.stream_handle()))
        return out

    def forward_row(self, slot: int, pos: int, row: torch.Tensor, logits: torch.Tensor):
        _lib.check(self.lib.lvx_ar_forward_row(self.h, slot, pos, _ptr(row), _ptr(logits), self.stream_handle()))

    def reset_slot(self, slot: int):
        _lib.check(self.lib.lvx_stream_reset(self.h, slot, self.stream_handle()))

    def set_slot(self, slot: int, pos: int, prev_token: int = 0):
        _lib.check(self.lib.lvx_stream_set(self.h, slot, pos, prev_token, self.stream_handle()))

    def set_sampling(self, slot: int, temperature: float = 0.0, top_k: int = 0, seed: int = 0, top_p: float = 1.0,
                     min_p: float = 0.0, repetition_penalty: float = 1.0, repetition_window: int = 64):
        """Seeded sampling of the slot's decode steps (lvx_stream_sampling_ex; temperature 0: greedy): top-k,
        nucleus and min-p crops and a repetition penalty over the slot's last ``repetition_window`` tokens.
        Stream-ordered on the current stream, like ``set_slot``."""
        p = _lib.LvxSampling(float(temperature), int(top_k), float(top_p), float(min_p), float(repetition_penalty),
                             int(repetition_window), int(seed) & 0xFFFFFFFFFFFFFFFF)
        _lib.check(self.lib.lvx_stream_sampling_ex(self.h, slot, ctypes.byref(p), self.stream_handle()))

    def stream_history(self, slot: int, pos0: int, n: int) -> torch.Tensor:
        """Test hook: entries ``pos0 .. pos0 + n - 1`` of the slot's token history, a device int32 tensor [n]
        (lvx_stream_history)."""
        out = torch.empty(max(int(n), 0), device=self.device, dtype=torch.int32)
        _lib.check(self.lib.lvx_stream_history(self.h, int(slot), int(pos0), int(n), _ptr(out), 0, self.stream_handle()))
        return out

    def write_history(self, slot: int, pos0: int, tokens):
        """Test hook: store ``tokens`` as the slot's history entries from ``pos0`` on (hist_from drops to pos0)."""
        t = torch.as_tensor(tokens, dtype=torch.int32).to(self.device).contiguous()
        _lib.check(self.lib.lvx_stream_history(self.h, int(slot), int(pos0), int(t.numel()), _ptr(t), 1,
                                               self.stream_handle()))

    def sample_kept(self, B: int) -> torch.Tensor:
        """Test hook: per batch row of the last sampled select, int32 [B, 4] = (kept tokens, fp32 bits of the
        lowest kept z, distinct penalised tokens, 0) (lvx_sample_kept)."""
        out = torch.empty(int(B), 4, device=self.device, dtype=torch.int32)
        _lib.check(self.lib.lvx_sample_kept(self.h, int(B), _ptr(out), self.stream_handle()))
        return out

    def slot_position(self, slot: int) -> int:
        v = ctypes.c_int()
        _lib.check(self.lib.lvx_stream_position(self.h, slot, ctypes.byref(v), self.stream_handle()))
        return v.value

    def ar_steps(self, n_steps: int, slots: torch.Tensor, text_plan: torch.Tensor, rowstep: torch.Tensor,
                 tok_plan: torch.Tensor, margin_plan: Optional[torch.Tensor] = None):
        B, stride = text_plan.shape
        self._capture_guard()
        _lib.check(self.lib.lvx_ar_steps(self.h, n_steps, B, _ptr(slots), _ptr(text_plan), stride, _ptr(rowstep),
                                         _ptr(tok_plan), _ptr(margin_plan), self.stream_handle()))

    def probe_kernel(self, which: int, slots: torch.Tensor, iters: int):
        self._capture_guard()
        _lib.check(self.lib.lvx_probe_kernel(self.h, which, slots.numel(), _ptr(slots), iters, self.stream_handle()))

    def select_probe(self, path: int, slots: torch.Tensor, logits: torch.Tensor, text_plan: torch.Tensor,
                     rowstep: torch.Tensor, tok_plan: torch.Tensor, margin_plan: Optional[torch.Tensor] = None):
        """Test hook: one production select path (0 argmax kernel, 1 deferred lm_head granules,
        2 batched deferred select, 3 the 4 <= B <= 8 prologue granules, 4 the sampled select with the
        slots' current set_sampling parameters) over the given logits [B, 4096], committed as a step commits."""
        B, stride = text_plan.shape
        logits = logits.to(self.device, torch.float32).contiguous()
        _lib.check(self.lib.lvx_select_probe(self.h, path, B, _ptr(slots), _ptr(logits), _ptr(text_plan), stride,
                                             _ptr(rowstep), _ptr(tok_plan), _ptr(margin_plan), self.stream_handle()))

    def kv_write(self, slot: int, layer: int, pos0: int, k: Optional[torch.Tensor], v: Optional[torch.Tensor],
                 raw: bool = False):
        """Test hook: store rows ``pos0 ..`` of one (slot, layer) of the KV cache from device tensors [n, 768]
        (head-major). float32 values are converted as a step's append converts them; ``raw``: int32 tensors
        whose low 32 / 16 / 8 bits are the stored elements (lvx_kv_write / lvx_kv_write_raw)."""
        want = torch.int32 if raw else torch.float32
        n = None
        for t in (k, v):
            if t is not None:
                if t.dtype != want or t.device != self.device or t.dim() != 2 or t.shape[1] != 768 or not t.is_contiguous():
                    raise ValueError(f"k / v must be contiguous {want} [n, 768] tensors on {self.device}")
                if n is not None and t.shape[0] != n:
                    raise ValueError("k and v must hold the same number of rows")
                n = int(t.shape[0])
        fn = self.lib.lvx_kv_write_raw if raw else self.lib.lvx_kv_write
        _lib.check(fn(self.h, int(slot), int(layer), int(pos0), n or 0, _ptr(k), _ptr(v), self.stream_handle()))

    def kv_read(self, slot: int, layer: int, pos0: int, n: int):
        """Test hook: rows ``pos0 .. pos0 + n - 1`` of one (slot, layer) of the KV cache, widened exactly to
        float32: (k, v) device tensors [n, 768] (lvx_kv_read)."""
        k = torch.empty(n, 768, device=self.device, dtype=torch.float32)
        v = torch.empty(n, 768, device=self.device, dtype=torch.float32)
        _lib.check(self.lib.lvx_kv_read(self.h, int(slot), int(layer), int(pos0), int(n), _ptr(k), _ptr(v),
                                        self.stream_handle()))
        return k, v

    def attn_probe(self, slots: torch.Tensor, layer: int, q: torch.Tensor, out: Optional[torch.Tensor] = None):
        """Test hook: the plan's production decode attention (and its merge kernel, if it has one) at
        B = len(slots) over ``q`` float32 [B, 768] and the slots' KV rows up to their current positions
        (lvx_attn_probe). Returns (form, out, part_o, part_ml, (nsplit, attn_direct, attn8)): form 0: the
        normalised rows in ``out`` [B, 768] (``out`` given: written in place, so an untouched row keeps
        the caller's values only where no kernel wrote the scratch row); form 1: the split partials
        part_o [B, 8, 16, 96] and part_ml [B, 8, 16, 2] for the caller to merge. Synchronises the stream."""
        B = int(slots.numel())
        q = q.to(self.device, torch.float32).contiguous()
        if q.shape != (B, 768):
            raise ValueError(f"q must be [{B}, 768]")
        if out is None:
            out = torch.zeros(B, 768, device=self.device, dtype=torch.float32)
        po = torch.zeros(B, 8, 16, 96, device=self.device, dtype=torch.float32)
        pml = torch.zeros(B, 8, 16, 2, device=self.device, dtype=torch.float32)
        info = (ctypes.c_int * 4)()
        _lib.check(self.lib.lvx_attn_probe(self.h, B, _ptr(slots), int(layer), _ptr(q), _ptr(out), _ptr(po), _ptr(pml),
                                           info, self.stream_handle()))
        torch.cuda.current_stream(self.device).synchronize()
        return info[0], out, po, pml, (info[1], info[2], info[3])

    def ar_ops(self, slots: torch.Tensor, first: int, last: int, x_in: Optional[torch.Tensor] = None,
               q_in: Optional[torch.Tensor] = None, text_ids: Optional[torch.Tensor] = None, poison: bool = False):
        """Test hook: ops ``first .. last`` of one decode step (5 * layer + {0 c_attn, 1 attention, 2 c_proj,
        3 c_fc, 4 mlp c_proj}, 20 lm_head) as the plan at B = len(slots) launches them, on given input
        (lvx_ar_ops in llmvox.h): ``x_in`` float32 [B, 768] for every entry but op 0, ``q_in`` for an entry at
        an attention, ``text_ids`` int32 [B] for op 0. Returns a dict: ``form`` (``_lib.AR_OUT_*``), ``out``
        (the rows of that form; the K-split partials as [4, B, 2304]), ``copies`` (the pending copies at the
        exit, float32 or int64 [B, n, 768], n may be 0), ``part_o`` / ``part_ml`` (attention partials) and
        ``plan``: (path, fused_mlp, nsplit, attn_direct, attn8, xpk, ksplit, qsplit, copies, fixed point).
        Synchronises the stream."""
        B = int(slots.numel())

        def rows(t, dtype, shape):
            if t is None:
                return None
            t = t.to(self.device, dtype).contiguous()
            if tuple(t.shape) != shape:
                raise ValueError(f"expected a tensor of shape {shape}, got {tuple(t.shape)}")
            return t

        x_in, q_in = rows(x_in, torch.float32, (B, 768)), rows(q_in, torch.float32, (B, 768))
        text_ids = rows(text_ids, torch.int32, (B,))
        out = torch.zeros(4 * B * 2304, device=self.device, dtype=torch.float32)
        cp = torch.zeros(B, 4, 768, device=self.device, dtype=torch.float32)
        cfx = torch.zeros(B, 4, 768, device=self.device, dtype=torch.int64)
        po = torch.zeros(B, 8, 16, 96, device=self.device, dtype=torch.float32)
        pml = torch.zeros(B, 8, 16, 2, device=self.device, dtype=torch.float32)
        info = (ctypes.c_int * _lib.AR_INFO)()
        _lib.check(self.lib.lvx_ar_ops(self.h, B, _ptr(slots), int(first), int(last), _ptr(x_in), _ptr(q_in),
                                       _ptr(text_ids), int(bool(poison)), _ptr(out), _ptr(cp), _ptr(cfx), _ptr(po),
                                       _ptr(pml), info, self.stream_handle()))
        torch.cuda.current_stream(self.device).synchronize()
        form, n = info[0], info[11]
        width = {_lib.AR_OUT_H: 3072, _lib.AR_OUT_LOGITS: 4096}.get(form, 768)
        o = out[:4 * B * 2304].view(4, B, 2304) if form == _lib.AR_OUT_QKV_PARTS else out[:B * width].view(B, width)
        copies = (cfx if info[10] else cp).view(-1)[:B * n * 768].view(B, n, 768)
        return dict(form=form, out=o, copies=copies, part_o=po, part_ml=pml, plan=tuple(info[1:11]))

    def last_logits(self, B: int) -> torch.Tensor:
        out = torch.empty(B, 4096, device=self.device, dtype=torch.float32)
        _lib.check(self.lib.lvx_ar_logits(self.h, B, _ptr(out), self.stream_handle()))
        return out

    def check_errors(self):
        """Synchronise the current stream and raise for the device error bits of both words (AR and
        codec); every set condition is named in the message."""
        code = self.lib.lvx_check_errors(self.h, self.stream_handle())
        if code:
            raise _lib.error_for(code)

    def take_errors(self, which: int, out: torch.Tensor):
        """Enqueue (no synchronisation) the atomic take of the AR (``_lib.ERRW_AR``) and / or codec
        (``_lib.ERRW_CODEC``) error bits into the device int32 ``out[0]``; ``_lib.check_bits`` on the
        host copy raises for them."""
        _lib.check(self.lib.lvx_error_take(self.h, int(which), _ptr(out), self.stream_handle()))

    def set_option(self, name: str, value: int):
        _lib.check(self.lib.lvx_set_option(self.h, name.encode(), int(value)))

    def set_capture_stream(self, stream: Optional["torch.cuda.Stream"]):
        """Capture the decode graphs on `stream` (None: on the caller's stream), lvx_set_capture_stream."""
        self._capture_stream = stream
        _lib.check(self.lib.lvx_set_capture_stream(self.h, ctypes.c_void_p(stream.cuda_stream if stream else None)))

    def _capture_guard(self):
        # Once an RCCL process group exists, its watchdog thread queries the events that synchronous
        # collectives record on the current stream, and HIP refuses that query while the stream is
        # capturing (lvx_api.cpp cached_graph): capture on a pooled stream of torch's that nothing else
        # records on. Not before: one more stream per process cost two ranks sharing a GPU 6.5x.
        # (a pooled stream may come round again as the caller's: never capture on the stream called on)
        if self._capture_stream is None:
            if not (dist.is_available() and dist.is_initialized() and "nccl" in str(dist.get_backend()).lower()):
                return
        elif self._capture_stream.cuda_stream != torch.cuda.current_stream(self.device).cuda_stream:
            return
        cur = torch.cuda.current_stream(self.device).cuda_stream
        s = torch.cuda.Stream(device=self.device)
        while s.cuda_stream == cur:
            s = torch.cuda.Stream(device=self.device)
        self.set_capture_stream(s)

    def set_graphs(self, enable: bool):
        _lib.check(self.lib.lvx_set_graphs(self.h, int(enable)))

    def decode_features(self, feats: torch.Tensor, bandwidth_id: int = 0) -> torch.Tensor:
        feats = feats.to(self.device, torch.float32).contiguous()
        B, C, L = feats.shape
        if C != 512:
            raise ValueError(f"features must be [B, 512, L], got {tuple(feats.shape)}")
        pcm = torch.empty(B, 320 * L, device=self.device, dtype=torch.float32)
        _lib.check(self.lib.lvx_codec_decode_features(self.h, _ptr(feats), B, L, int(bandwidth_id), _ptr(pcm),
                                                      self.stream_handle()))
        return pcm

    def decode_codes(self, codes: torch.Tensor, bandwidth_id: int = 0, out: Optional[torch.Tensor] = None):
        codes = codes.to(self.device, torch.int32).contiguous()
        B, L = codes.shape
        pcm = out if out is not None else torch.empty(B, 320 * L, device=self.device, dtype=torch.float32)
        _lib.check(self.lib.lvx_codec_decode_codes(self.h, _ptr(codes), B, L, int(bandwidth_id), _ptr(pcm),
                                                   self.stream_handle()))
        return pcm

    def codec_stages(self, first: int, last: int, inp: torch.Tensor, B: int, L: int, bandwidth_id: int = 0):
        """Test hook: stages ``first .. last`` of the codec decode (the table at lvx_codec_stages in llmvox.h)
        on ``inp``: int32 codes [B, L] for stage 0, the float32 residual stream [B * L, 768] for 1 .. 19, the
        spectrum [B * L, 1282] for 20. Returns (out, routes): the state after ``last`` (x, the spectrum after
        19, PCM [B, 320 L] after 20) and one tuple (family, ksplit, inlaunch, v0, v1, v2, N, K) per GEMM the
        window launched, in launch order (family: _lib.ROUTE_*)."""
        B, L, M = int(B), int(L), int(B) * int(L)
        want = (B, L) if first == 0 else (M, 1282) if first == 20 else (M, 768)
        inp = inp.to(self.device, torch.int32 if first == 0 else torch.float32).contiguous()
        if tuple(inp.shape) != want:
            raise ValueError(f"stage {first} takes an input of shape {want}, got {tuple(inp.shape)}")
        shape = (B, 320 * L) if last == 20 else (M, 1282) if last == 19 else (M, 768)
        out = torch.empty(*shape, device=self.device, dtype=torch.float32)
        cap = 64
        rec = (ctypes.c_int32 * (8 * cap))()
        n = ctypes.c_int()
        _lib.check(self.lib.lvx_codec_stages(self.h, int(first), int(last), _ptr(inp), B, L, int(bandwidth_id),
                                             _ptr(out), rec, cap, ctypes.byref(n), self.stream_handle()))
        if n.value > cap:
            raise RuntimeError(f"{n.value} GEMMs in the window, more than the {cap} route records asked for")
        return out, [tuple(rec[8 * i:8 * i + 8]) for i in range(n.value)]

    # ---- PCM output stage ------------------------------------------------------------
    def pcm_filter(self, sample_rate: int):
        """(L, M, N, taps float32 [2 N + 1]) of an output rate, as the library designs them (lvx_pcm_filter)."""
        L, M, N = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        _lib.check(self.lib.lvx_pcm_filter(int(sample_rate), ctypes.byref(L), ctypes.byref(M), ctypes.byref(N), None, 0))
        taps = np.zeros(2 * N.value + 1, dtype=np.float32)
        _lib.check(self.lib.lvx_pcm_filter(int(sample_rate), None, None, None, taps.ctypes.data_as(ctypes.c_void_p),
                                           taps.size))
        return L.value, M.value, N.value, taps

    def pcm_reset(self, slot: int):
        """Forget the slot's output-stage history and position: its next ``pcm_convert`` starts a segment."""
        _lib.check(self.lib.lvx_pcm_reset(self.h, int(slot), self.stream_handle()))

    def pcm_stretch_window(self):
        """(wr, wf) float32 [240]: the time stretch's window tables as the library builds them
        (lvx_pcm_stretch_window)."""
        wr, wf = np.zeros(240, dtype=np.float32), np.zeros(240, dtype=np.float32)
        _lib.check(self.lib.lvx_pcm_stretch_window(wr.ctypes.data_as(ctypes.c_void_p),
                                                   wf.ctypes.data_as(ctypes.c_void_p), 240))
        return wr, wf

    def _pcm_rows(self, pcm: Optional[torch.Tensor], B: int):
        """(rows, n_in) of a stage's input, checked; None: no rows, a flush."""
        if pcm is None:
            return None, 0
        if pcm.shape[0] != B or pcm.dtype != torch.float32 or pcm.device != self.device:
            raise ValueError(f"pcm must be a float32 [{B}, n_in] tensor on {self.device}")
        return pcm.contiguous(), int(pcm.shape[1])

    def _pcm_args(self, pcm: Optional[torch.Tensor], slots, finals):
        """What every stage's library call takes: (rows, n_in, B, slots as c_int32, finals as c_uint8, the counts array
        to fill) and the output of a stage with nothing to do, the rows themselves."""
        slots = [int(s) for s in slots]
        B = len(slots)
        pcm, n_in = self._pcm_rows(pcm, B)
        same = pcm if pcm is not None else torch.empty(B, 0, device=self.device, dtype=torch.float32)
        return (pcm, n_in, B, (ctypes.c_int32 * B)(*slots), (ctypes.c_uint8 * B)(*[1 if f else 0 for f in finals]),
                (ctypes.c_int32 * B)(), same)

    def pcm_stretch(self, pcm: Optional[torch.Tensor], slots, finals, speed_pct: int, want_d: bool = False):
        """The time stretch alone (lvx_pcm_stretch): rows of ``pcm`` (device float32 [B, n_in] at 24 kHz; None
        or n_in 0: flush only) continue the stretch segments of ``slots`` at ``speed_pct``; a true
        ``finals[b]`` emits the rest of row b's segment and ends it. Returns (out, counts, d): a device
        float32 tensor [B, width] whose row b holds counts[b] samples, and (``want_d``) a device int32 tensor
        whose row b holds the chosen d_j of the hops the call emitted (else None). speed_pct 100: the rows
        themselves. Asynchronous on the current stream; a slot's calls must be issued in order on one stream."""
        pcm, n_in, B, sl, fl, cnt, same = self._pcm_args(pcm, slots, finals)
        speed_pct = int(speed_pct)
        out = d = None
        width = dw = 0
        if speed_pct == 100:
            out = same
        elif 50 <= speed_pct <= 200:
            # a call emits at most the hops that waited for their right-hand inputs (<= 960 inputs' worth)
            # and its own inputs' worth, cut to whole hops; rows start on 16-byte boundaries
            width = ((n_in * 100 + 96000) // speed_pct + 2 * 240 + 7) // 8 * 8
            out = torch.empty(B, width, device=self.device, dtype=torch.float32)
            if want_d:
                dw = width // 240 + 1
                d = torch.zeros(B, dw, device=self.device, dtype=torch.int32)
        _lib.check(self.lib.lvx_pcm_stretch(self.h, _ptr(pcm) if n_in else None, B, n_in, sl, fl, speed_pct, _ptr(out),
                                            width * 4, cnt, _ptr(d), dw, self.stream_handle()))
        return out, list(cnt), d

    def pcm_pitch_plan(self, speed_pct: int, pitch_pct: int):
        """(stretch_pct, L, M) of a speed and a pitch as the library plans them (lvx_pcm_pitch_plan)."""
        st, L, M = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        _lib.check(self.lib.lvx_pcm_pitch_plan(int(speed_pct), int(pitch_pct), ctypes.byref(st), ctypes.byref(L),
                                               ctypes.byref(M)))
        return st.value, L.value, M.value

    def pcm_ratio_filter(self, L: int, M: int):
        """(N, taps float32 [2 N + 1]) of the ratio L / M, as the library designs them (lvx_pcm_ratio_filter)."""
        N = ctypes.c_int()
        _lib.check(self.lib.lvx_pcm_ratio_filter(int(L), int(M), ctypes.byref(N), None, 0))
        taps = np.zeros(2 * N.value + 1, dtype=np.float32)
        _lib.check(self.lib.lvx_pcm_ratio_filter(int(L), int(M), None, taps.ctypes.data_as(ctypes.c_void_p), taps.size))
        return N.value, taps

    def pcm_ratio(self, pcm: Optional[torch.Tensor], slots, finals, L: int, M: int):
        """The pitch control's resampler alone (lvx_pcm_ratio): rows of ``pcm`` (device float32 [B, n_in]; None or
        n_in 0: flush only) continue the ratio segments of ``slots`` at L / M (output count over input count); a
        true ``finals[b]`` emits the rest of row b's segment and ends it. Returns (out, counts): a device
        float32 tensor [B, width] whose row b holds counts[b] samples. 1 / 1: the rows themselves. Asynchronous
        on the current stream; a slot's calls must be issued in order on one stream."""
        pcm, n_in, B, sl, fl, cnt, same = self._pcm_args(pcm, slots, finals)
        L, M = int(L), int(M)
        out, width = None, 0
        if L == M == 1:
            out = same
        elif 1 <= L <= 200 and 1 <= M <= 200:
            # a call emits at most (n_in L + L + N) / M + 2 samples, N = 24 max(L, M) (a final call of a segment
            # whose earlier outputs waited for their right-hand inputs); rows start on 16-byte boundaries
            width = ((n_in * L + L + 24 * max(L, M)) // M + 3 + 7) // 8 * 8
            out = torch.empty(B, width, device=self.device, dtype=torch.float32)
        _lib.check(self.lib.lvx_pcm_ratio(self.h, _ptr(pcm) if n_in else None, B, n_in, sl, fl, L, M, _ptr(out), width * 4,
                                          cnt, self.stream_handle()))
        return out, list(cnt)

    def pcm_join_window(self):
        """(wr, wf) float32 [320]: the dump join's crossfade tables as the library builds them
        (lvx_pcm_join_window)."""
        wr, wf = np.zeros(320, dtype=np.float32), np.zeros(320, dtype=np.float32)
        _lib.check(self.lib.lvx_pcm_join_window(wr.ctypes.data_as(ctypes.c_void_p),
                                                wf.ctypes.data_as(ctypes.c_void_p), 320))
        return wr, wf

    def pcm_join(self, pcm: Optional[torch.Tensor], slots, ctx_frames, finals):
        """The dump join alone (lvx_pcm_join): rows of ``pcm`` (device float32 [B, n_in] at 24 kHz, n_in a
        multiple of 320; None or n_in 0: flush only) continue the join segments of ``slots``; the first
        ``ctx_frames[b]`` frames of row b re-render what its segment has already delivered; a true
        ``finals[b]`` emits the row to its end and closes the segment. Returns (out, counts): a device float32
        tensor [B, width] whose row b holds counts[b] samples. Asynchronous on the current stream; a slot's
        calls must be issued in order on one stream."""
        pcm, n_in, B, sl, fl, cnt, _ = self._pcm_args(pcm, slots, finals)
        width = n_in + 320  # (the most a call emits: its row and the held-back frame; rows on 16-byte boundaries)
        out = torch.empty(B, width, device=self.device, dtype=torch.float32)
        cf = (ctypes.c_int32 * B)(*[int(c) for c in ctx_frames])
        _lib.check(self.lib.lvx_pcm_join(self.h, _ptr(pcm) if n_in else None, B, n_in, sl, cf, fl, _ptr(out), width * 4,
                                         cnt, self.stream_handle()))
        return out, list(cnt)

    def pcm_level_window(self):
        """w float32 [241]: the level stage's smoothing window as the library builds it (lvx_pcm_level_window)."""
        w = np.zeros(241, dtype=np.float32)
        _lib.check(self.lib.lvx_pcm_level_window(w.ctypes.data_as(ctypes.c_void_p), w.size))
        return w

    def pcm_level(self, pcm: Optional[torch.Tensor], slots, finals, volume_pct: int, want_g: bool = False):
        """The volume control alone (lvx_pcm_level): rows of ``pcm`` (device float32 [B, n_in] at 24 kHz; None or
        n_in 0: flush only) continue the level segments of ``slots`` at ``volume_pct`` (a gain of volume_pct / 100
        and the peak limiter); a true ``finals[b]`` emits the held-back 240 samples too and ends row b's segment.
        Returns (out, counts, g): a device float32 tensor [B, width] whose row b holds counts[b] samples, and
        (``want_g``) a device float32 tensor whose row b holds the limiter's gain of each (else None). volume_pct
        100: the rows themselves. Asynchronous on the current stream; a slot's calls must be issued in order on
        one stream."""
        pcm, n_in, B, sl, fl, cnt, same = self._pcm_args(pcm, slots, finals)
        volume_pct = int(volume_pct)
        out = g = None
        width = 0
        if volume_pct == 100:
            out = same
        elif 0 <= volume_pct <= 400:
            width = (n_in + 240 + 7) // 8 * 8  # (the call's inputs and the held-back 240; rows on 16-byte boundaries)
            out = torch.empty(B, width, device=self.device, dtype=torch.float32)
            if want_g:
                g = torch.zeros(B, width, device=self.device, dtype=torch.float32)
        _lib.check(self.lib.lvx_pcm_level(self.h, _ptr(pcm) if n_in else None, B, n_in, sl, fl, volume_pct, _ptr(out),
                                          width * 4, cnt, _ptr(g), width * 4, self.stream_handle()))
        return out, list(cnt), g

    def pcm_formant_plan(self, speed_pct: int, pitch_pct: int, formant_pct: int):
        """(Fn, Fd) of a speed, a pitch and a formant as the library plans them (lvx_pcm_formant_plan)."""
        Fn, Fd = ctypes.c_int(), ctypes.c_int()
        _lib.check(self.lib.lvx_pcm_formant_plan(int(speed_pct), int(pitch_pct), int(formant_pct), ctypes.byref(Fn),
                                                 ctypes.byref(Fd)))
        return Fn.value, Fd.value

    def pcm_formant_tables(self):
        """(w float32 [1024], c float32 [25], tw float32 [1024]): the formant stage's window, smoothing taps and
        twiddles as the library builds them (lvx_pcm_formant_tables)."""
        w, c, tw = np.zeros(1024, dtype=np.float32), np.zeros(25, dtype=np.float32), np.zeros(1024, dtype=np.float32)
        ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)
        _lib.check(self.lib.lvx_pcm_formant_tables(ptr(w), w.size, ptr(c), c.size, ptr(tw), tw.size))
        return w, c, tw

    def pcm_formant(self, pcm: Optional[torch.Tensor], slots, finals, Fn: int, Fd: int):
        """The formant control's envelope correction alone (lvx_pcm_formant): rows of ``pcm`` (device float32 [B, n_in]
        at 24 kHz; None or n_in 0: flush only) continue the formant segments of ``slots`` at the ratio Fn / Fd (the
        envelope of the output at a frequency is that of the input at Fn / Fd times it); a true ``finals[b]`` emits the
        held-back 768 .. 1023 samples too and ends row b's segment. Returns (out, counts): a device float32 tensor
        [B, width] whose row b holds counts[b] samples. 1 / 1: the rows themselves. Asynchronous on the current stream;
        a slot's calls must be issued in order on one stream."""
        pcm, n_in, B, sl, fl, cnt, same = self._pcm_args(pcm, slots, finals)
        Fn, Fd = int(Fn), int(Fd)
        out, width = None, 0
        if Fn == Fd == 1:
            out = same
        elif 1 <= Fn <= 40000 and 1 <= Fd <= 40000:
            # (the call's inputs and the held-back <= 1023; rows on 16-byte boundaries)
            width = (n_in + 1023 + 7) // 8 * 8
            out = torch.empty(B, width, device=self.device, dtype=torch.float32)
        _lib.check(self.lib.lvx_pcm_formant(self.h, _ptr(pcm) if n_in else None, B, n_in, sl, fl, Fn, Fd, _ptr(out),
                                            width * 4, cnt, self.stream_handle()))
        return out, list(cnt)

    def pcm_mark_table(self, key: int, mark_id: int = 0):
        """uint16 [64]: the watermark's sign table of (key, id) as the library builds it (lvx_pcm_mark_table)."""
        words = np.zeros(64, dtype=np.uint16)
        _lib.check(self.lib.lvx_pcm_mark_table(_mark_key(key), int(mark_id), words.ctypes.data_as(ctypes.c_void_p),
                                               words.size))
        return words

    def pcm_mark(self, pcm: Optional[torch.Tensor], slots, finals, key: int, mark_id: int = 0, strength: int = 2):
        """The watermark alone (lvx_pcm_mark): rows of ``pcm`` (device float32 [B, n_in] at 24 kHz; None or n_in 0:
        flush only) continue the mark segments of ``slots`` under the 64-bit ``key``, the payload ``mark_id``
        (0 .. 255) and ``strength`` (1 .. 3); a true ``finals[b]`` emits the held-back 768 .. 1023 samples too and
        ends row b's segment. Returns (out, counts): a device float32 tensor [B, width] whose row b holds counts[b]
        samples. Asynchronous on the current stream; a slot's calls must be issued in order on one stream."""
        pcm, n_in, B, sl, fl, cnt, _ = self._pcm_args(pcm, slots, finals)
        width = (n_in + 1023 + 7) // 8 * 8  # (the call's inputs and the held-back <= 1023; rows on 16-byte boundaries)
        out = torch.empty(B, width, device=self.device, dtype=torch.float32)
        _lib.check(self.lib.lvx_pcm_mark(self.h, _ptr(pcm) if n_in else None, B, n_in, sl, fl, _mark_key(key),
                                         int(mark_id), int(strength), _ptr(out), width * 4, cnt, self.stream_handle()))
        return out, list(cnt)

    def pcm_convert(self, pcm: Optional[torch.Tensor], slots, finals, fmt, ctx_frames=None):
        """Rows of ``pcm`` (device float32 [B, n_in] at 24 kHz; None or n_in 0: flush only) continue the
        segments of ``slots``; a true ``finals[b]`` flushes row b's filter and ends its segment. ``fmt``: an
        ``audio.AudioFormat`` (its speed, pitch, formant, volume, rate and encoding). Returns (out, counts): a device
        tensor [B, width] of float32, int16 or (G.711) uint8 whose row b holds counts[b] samples. Six stages in this
        order, each only where the format needs it, so that a format makes exactly the calls of the stages it uses: the
        dump join (lvx_pcm_join, a format with ``join``: row b with ``ctx_frames[b]`` frames of context in front, None:
        none anywhere), the time stretch at the plan's stretch_pct (lvx_pcm_stretch), the resampling by the plan's
        L / M (lvx_pcm_ratio), the envelope correction by the plan's Fn / Fd (lvx_pcm_formant), the watermark of a
        format with a ``mark_key`` (lvx_pcm_mark), the gain and limiter at
        volume_pct (lvx_pcm_level), the rate and the encoding (lvx_pcm_convert). A "flac" format runs that last stage as
        s16le and one more behind it (lvx_pcm_flac): its rows are uint8, whole slots of LVX_FLAC_SLOT bytes (a record
        and a subframe each; ``audio.FlacMux`` makes them frames), and counts[b] is their bytes. A format that
        ``pauses`` (``pause_ms`` / ``max_pause_ms``) runs one more stage behind the format's encoded rows (lvx_pcm_pause):
        its rows are uint8 too, whole slots of LVX_PAUSE_SLOT bytes (a record and a block of 10 ms each;
        ``audio.PauseMux`` trims and spaces by them), and counts[b] is their bytes. Rows may leave a stage with different counts: they pass the next one grouped by count.
        Asynchronous on the current stream; a slot's calls must be issued in order on one stream."""
        stretch_pct, (L, M), vol, (Fn, Fd) = fmt.stretch_pct, fmt.ratio, fmt.volume_pct, fmt.formant
        slots, finals = [int(s) for s in slots], [bool(f) for f in finals]
        if not fmt.join and ctx_frames is not None and any(ctx_frames):
            raise ValueError("ctx_frames without a joined format")
        ctx = ctx_frames if ctx_frames is not None else [0] * len(slots)
        stages = []  # the stages this format needs, in the order the rows pass them (the join sees every row at once)
        if fmt.join:
            stages.append(lambda sub, sl, fl: self.pcm_join(sub, sl, ctx, fl))
        if stretch_pct != 100:
            stages.append(lambda sub, sl, fl: self.pcm_stretch(sub, sl, fl, stretch_pct)[:2])
        if L != M:
            stages.append(lambda sub, sl, fl: self.pcm_ratio(sub, sl, fl, L, M))
        if Fn != Fd:
            stages.append(lambda sub, sl, fl: self.pcm_formant(sub, sl, fl, Fn, Fd))
        if fmt.mark_key is not None:  # the watermark: behind the formant, in front of the limiter
            stages.append(lambda sub, sl, fl: self.pcm_mark(sub, sl, fl, fmt.mark_key, fmt.mark_id, fmt.mark_strength))
        if vol != 100:
            stages.append(lambda sub, sl, fl: self.pcm_level(sub, sl, fl, vol)[:2])
        # The rate and the encoding come last. At 24 kHz f32le they have nothing to do and the output of the stage
        # before them is the result: they are skipped, unless no other stage runs (the library's mirror of the
        # segment still has to advance).
        if not stages or not (fmt.sample_rate == 24000 and fmt.encoding == "f32le"):
            stages.append(lambda sub, sl, fl: self._pcm_resample(sub, sl, fl, fmt))
        if fmt.encoding == "flac":  # the sixth stage, behind the s16le rows of the rate: whole slots, counted in bytes
            rate, slot = fmt.sample_rate, ((8 + 1 + 2 * (fmt.sample_rate // 25 + 15) + 15) // 16) * 16

            def flac(sub, sl, fl):
                out, frames = self.pcm_flac(sub, sl, fl, rate)
                return out, [n * slot for n in frames]
            stages.append(flac)
        dtype = _PCM_ENCODINGS[fmt.encoding][1]
        if fmt.pauses:  # the last stage, behind the format's encoded rows: whole slots, counted in bytes
            slot = 8 + fmt.sample_rate // 100 * fmt.sample_bytes

            def pause(sub, sl, fl):
                out, blocks = self.pcm_pause(sub, sl, fl, fmt)
                return out, [n * slot for n in blocks]
            stages.append(pause)
            dtype = torch.uint8

        def run(i, sub, sl, fl):  # stage i and, grouped by what it hands on, the stages behind it
            out, cnt = stages[i](sub, sl, fl)
            if i + 1 == len(stages):
                return out, cnt
            return self._pcm_grouped(out, cnt, sl, fl, lambda *rows: run(i + 1, *rows), dtype)

        return run(0, pcm, slots, finals)

    def _pcm_grouped(self, st, cnt, slots, finals, stage, dtype):
        """The hand-over between two stages: row b of ``st`` holds cnt[b] samples; the rows pass
        ``stage(rows, slots, finals)`` grouped by count (a row with nothing to hand on and no end is left
        out). Returns (out, counts) over all rows."""
        slots, finals = [int(s) for s in slots], [bool(f) for f in finals]
        groups: Dict[int, list] = {}
        for b, n in enumerate(cnt):
            if n or finals[b]:  # (nothing came out of the stage before and no end: nothing to hand on)
                groups.setdefault(n, []).append(b)
        parts = []
        for n, rows in groups.items():
            sub = None if n == 0 else st[:, :n] if len(rows) == len(slots) else st[rows, :n]
            o, c = stage(sub, [slots[b] for b in rows], [finals[b] for b in rows])
            parts.append((rows, o, c))
        if len(parts) == 1 and len(parts[0][0]) == len(slots):
            return parts[0][1], parts[0][2]
        width = max([o.shape[1] for _, o, _ in parts], default=0)
        out = torch.zeros(len(slots), width, device=self.device, dtype=dtype)
        counts = [0] * len(slots)
        for rows, o, c in parts:
            out[rows, :o.shape[1]] = o
            for b, n in zip(rows, c):
                counts[b] = n
        return out, counts

    def pcm_flac(self, s16: Optional[torch.Tensor], slots, finals, sample_rate: int):
        """The FLAC stage alone (lvx_pcm_flac): rows of ``s16`` (device int16 [B, n_in] at ``sample_rate``, what
        ``pcm_convert`` writes as s16le; rows may be strided; None or n_in 0: flush only) continue the FLAC segments of
        ``slots``; a true ``finals[b]`` emits the sentence's last frame and ends the segment. Returns (out, frames): a
        device uint8 tensor [B, width] whose row b holds frames[b] slots of LVX_FLAC_SLOT(sample_rate) bytes, each the
        record {u16 n, u16 body_bytes, u32 0} and the frame's subframe. Asynchronous on the current stream; a slot's
        calls must be issued in order on one stream."""
        slots = [int(s) for s in slots]
        B, n_in, stride = len(slots), 0, 0
        if s16 is not None and s16.shape[1]:
            if s16.shape[0] != B or s16.dtype != torch.int16 or s16.device != self.device:
                raise ValueError(f"s16 must be an int16 [{B}, n_in] tensor on {self.device}")
            if s16.stride(1) != 1 or (B > 1 and s16.stride(0) < s16.shape[1]):
                s16 = s16.contiguous()
            n_in, stride = int(s16.shape[1]), 2 * int(s16.stride(0) if B > 1 else s16.shape[1])
        sl, fl = (ctypes.c_int32 * B)(*slots), (ctypes.c_uint8 * B)(*[1 if f else 0 for f in finals])
        cnt = (ctypes.c_int32 * B)()
        bs = int(sample_rate) // 25
        slot = ((8 + 1 + 2 * (bs + 15) + 15) // 16) * 16
        # (a call emits at most the frames of its own samples and the kept BS + 15, and the last one)
        width = ((n_in + bs + 15) // max(bs, 1) + 1) * slot
        out = torch.empty(B, width, device=self.device, dtype=torch.uint8)
        _lib.check(self.lib.lvx_pcm_flac(self.h, _ptr(s16) if n_in else None, stride, B, n_in, sl, fl, int(sample_rate),
                                         _ptr(out), width, cnt, self.stream_handle()))
        return out, list(cnt)

    def pcm_pause(self, rows: Optional[torch.Tensor], slots, finals, fmt):
        """The pause stage alone (lvx_pcm_pause): ``rows`` (a device tensor [B, n_in] of the samples ``fmt`` encodes to,
        what ``pcm_convert`` writes for it: float32, int16 or uint8; rows may be strided; None or n_in 0: flush only)
        continue the pause segments of ``slots``; a true ``finals[b]`` emits the sentence's last block and ends the
        segment. Returns (out, blocks): a device uint8 tensor [B, width] whose row b holds blocks[b] slots of
        LVX_PAUSE_SLOT bytes, each the record {u16 n, u8 active, u8 last, u32 0} and the block's samples. The stage
        holds back 1 .. bl samples until the final call. Asynchronous on the current stream; a slot's calls must be
        issued in order on one stream."""
        slots = [int(s) for s in slots]
        enc, dtype = _PCM_ENCODINGS[fmt.encoding]
        if enc is None:
            raise ValueError(f"the pause stage takes no {fmt.encoding!r} rows")
        B, n_in, stride, bps = len(slots), 0, 0, fmt.sample_bytes
        if rows is not None and rows.shape[1]:
            if rows.shape[0] != B or rows.dtype != dtype or rows.device != self.device:
                raise ValueError(f"rows must be a {dtype} [{B}, n_in] tensor on {self.device}")
            if rows.stride(1) != 1 or (B > 1 and rows.stride(0) < rows.shape[1]):
                rows = rows.contiguous()
            n_in, stride = int(rows.shape[1]), bps * int(rows.stride(0) if B > 1 else rows.shape[1])
        sl, fl = (ctypes.c_int32 * B)(*slots), (ctypes.c_uint8 * B)(*[1 if f else 0 for f in finals])
        cnt = (ctypes.c_int32 * B)()
        bl = fmt.sample_rate // 100
        # (a call emits at most the blocks of its own samples and the kept bl; a slot is a multiple of 8 bytes)
        width = ((n_in + bl - 1) // bl + 1) * (8 + bl * bps)
        out = torch.empty(B, width, device=self.device, dtype=torch.uint8)
        _lib.check(self.lib.lvx_pcm_pause(self.h, _ptr(rows) if n_in else None, stride, B, n_in, sl, fl, fmt.sample_rate, enc,
                                          _ptr(out), width, cnt, self.stream_handle()))
        return out, list(cnt)

    def _pcm_resample(self, pcm: Optional[torch.Tensor], slots, finals, fmt):
        """pcm_convert without the speed and the pitch: the rate and the encoding (lvx_pcm_convert; a "flac" format: as
        s16le, the FLAC stage's input)."""
        pcm, n_in, B, sl, fl, cnt, same = self._pcm_args(pcm, slots, finals)
        enc, dtype = _PCM_ENCODINGS["s16le" if fmt.encoding == "flac" else fmt.encoding]
        if fmt.sample_rate == 24000 and fmt.encoding == "f32le":  # the rows are the output (nothing is launched)
            out, width = same, n_in
        else:
            L, M, N = (ctypes.c_int() for _ in range(3))
            _lib.check(self.lib.lvx_pcm_filter(fmt.sample_rate, ctypes.byref(L), ctypes.byref(M), ctypes.byref(N), None, 0))
            # a call emits at most (n_in L + L + N) / M + 2 samples (a final call of a segment whose earlier
            # outputs waited for their right-hand inputs); rows start on 16-byte boundaries at any sample size, one
            # byte included (a multiple of 16 elements)
            width = ((n_in * L.value + L.value + N.value) // M.value + 3 + 15) // 16 * 16
            out = torch.empty(B, width, device=self.device, dtype=dtype)
        _lib.check(self.lib.lvx_pcm_convert(self.h, _ptr(pcm) if n_in else None, B, n_in, sl, fl, fmt.sample_rate, enc,
                                            _ptr(out), width * out.element_size(), cnt, self.stream_handle()))
        return out, list(cnt)

    def _g711(self, fn, src, law: str, src_dtype, dst_dtype):
        if law not in ("ulaw", "alaw"):
            raise ValueError(f"law must be 'ulaw' or 'alaw', got {law!r}")
        src = np.ascontiguousarray(src, dtype=src_dtype)
        dst = np.empty(src.shape, dtype=dst_dtype)
        _lib.check(fn(_PCM_ENCODINGS[law][0], src.ctypes.data_as(ctypes.c_void_p), src.size,
                      dst.ctypes.data_as(ctypes.c_void_p)))
        return dst

    def g711_encode(self, q, law: str):
        """The G.711 codes (uint8) of the int16 samples ``q`` at ``law`` ("ulaw" / "alaw"), on the host
        (lvx_pcm_g711_encode): the companding the device applies behind its s16 quantisation."""
        return self._g711(self.lib.lvx_pcm_g711_encode, q, law, np.int16, np.uint8)

    def g711_decode(self, codes, law: str):
        """The int16 samples of the G.711 ``codes`` (uint8) at ``law``, on the host (lvx_pcm_g711_decode)."""
        return self._g711(self.lib.lvx_pcm_g711_decode, codes, law, np.uint8, np.int16)

    def close(self):
        if getattr(self, "h", None):
            self.lib.lvx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# an audio.AudioFormat's encoding: (the LVX_PCM_* value, the dtype of the rows lvx_pcm_convert writes)
_PCM_ENCODINGS = {"f32le": (_lib.LVX_PCM_F32LE, torch.float32), "s16le": (_lib.LVX_PCM_S16LE, torch.int16),
                  "ulaw": (_lib.LVX_PCM_ULAW, torch.uint8), "alaw": (_lib.LVX_PCM_ALAW, torch.uint8),
                  "flac": (None, torch.uint8)}  # (no encoding of lvx_pcm_convert: lvx_pcm_flac behind its s16le rows)


def build_engine(device_index=0, weight_dtype="fp32", kv_dtype="fp32", seed=1234, max_streams=8,
                 max_positions=8192, max_codec_frames=1280, weights=None, codec_dtype=None) -> Engine:
    """Engine loaded with ``weights`` = (gpt, codec, text_table) or the seeded synthetic set.
    codec_dtype "fp8": codec GEMM weights stored as e4m3fn with per-row scales (configs[4])."""
    from .weights import synthetic_all
    gw, cw, tt = weights if weights is not None else synthetic_all(seed)
    # a checkpoint trained with a smaller block_size has zero-padded wpe rows past it: positions
    # there must raise (the reference asserts t <= block_size, src/model.py:205), so the KV
    # capacity never exceeds it
    max_positions = min(int(max_positions), int(getattr(gw, "block_size", max_positions)))
    e = Engine(device_index, weight_dtype, kv_dtype, max_streams, max_positions, max_codec_frames, codec_dtype)
    e.load_weights(gw, cw, tt)
    return e


__all__ = ["Engine", "build_engine", "CODEBOOK_KEY"]
