"""Multi-queue streaming scheduler of the LLMVoX TTS hot path.

Two layers:

1. ``audio_generator_sync`` / ``route_text`` / ``audio_generator_async`` / ``clean_text`` —
   the reference's scheduler (streaming_server.py:106-149,184-469) with the same signature
   and behaviour, driving any ModelHandler-like object one token at a time (our
   ``llmvox_amd.ModelHandler``, the CPU oracle, or a scripted fake in tests).

2. ``SegmentMachine`` + ``FusedScheduler`` — the same per-stream semantics (dump schedule,
   EOA flush, reset, control signals) restated as a state machine that consumes greedy
   tokens produced in chunks by the fused HIP decode step (``lvx_ar_steps``) for many
   streams at once (continuous batching), with the codec decode of every dump batched
   across streams. Run-ahead past an end-of-audio token is rolled back exactly.
"""
from __future__ import annotations

import asyncio
import atexit
import contextlib
import copy
import re
import threading
import weakref
from collections import deque
from dataclasses import dataclass, field
from queue import Empty, Queue
from typing import Callable, Deque, Dict, List, Optional

import numpy as np

from . import config as C
from .audio import JOIN_CONTEXT
from .streams import side_stream


def _cfg(config, key, default):
    if config is None:
        return default
    if hasattr(config, "get"):
        v = config.get(key, default)
    else:
        v = getattr(config, key, default)
    return default if v is None else v


# ---------------------------------------------------------------------------------------
# text cleaning / routing (streaming_server.py:106-149, 224-244)
# ---------------------------------------------------------------------------------------

def clean_text(text: str, eos_token: str = C.EOS_TOKEN) -> str:
    """Same substitutions, same order as the reference's clean_text."""
    text = text.strip().replace("**", "").replace("-", " ")
    text = re.sub(r"(\d)\.(?=\s|$)", r"\1", text)
    text = re.sub(r"\*", "", text)
    text = re.sub(r"#", " number ", text)
    text = re.sub(r"&", " and ", text)
    text = re.sub(r"@", " at ", text)
    text = re.sub(r"\s+", " ", text)
    text = re.sub(r"\.{3,}", " pause ", text)
    text = re.sub(r"(\d),(\d)", r"\1\2", text)
    text = re.sub(r"\/+", " slash ", text)
    text = re.sub(r"\\+", " backslash ", text)
    return text


def route_text(outputs, queues, eos: str = C.EOS_TOKEN):
    """text_streamer_producer's routing: skip '' / '-', strip, clean (unless it is the EOS
    token), put on the active queue, switch queue after a word that ends with '.'."""
    active = 0
    routed = []
    for out in outputs:
        if out in ("", "-"):
            continue
        out = out.strip()
        if out != eos:
            out = clean_text(out, eos)
        routed.append(out)
        if out:
            queues[active].put(out)
            if out.endswith("."):
                active = 1 - active
    return routed


# ---------------------------------------------------------------------------------------
# 1. the reference-shaped consumer (one token per model call)
# ---------------------------------------------------------------------------------------

def audio_generator_sync(index: int, dump_size: int, model_handler, text_token_queue: Queue,
                         audio_byte_queue: Queue, config=None):
    """Consumer thread of the multi-queue design (streaming_server.py:250-426).

    Extension: a ``None`` text token ends the loop (the reference loops forever); the
    generator then puts ``None`` on the audio queue, as the reference's unreachable tail does.
    """
    import torch
    import torch.nn.functional as F

    max_audio_len = _cfg(config, "max_audio_length", C.MAX_AUDIO_LENGTH)
    max_dump = _cfg(config, "max_dump_size", C.MAX_DUMP_SIZE)
    eos = _cfg(config, "eos_token", C.EOS_TOKEN)
    pad_token_id = _cfg(config, "pad_token_id", C.PAD_TOKEN_ID)
    eoa_token_id = _cfg(config, "eoa_token_id", C.EOA_TOKEN_ID)
    dev = model_handler.device
    bandwidth_id = torch.tensor([0]).to(dev)

    gen_index, cur_tok, kvcache = 0, None, None
    end_of_speech, end_generation = False, False
    speech_outputs: List[int] = []
    hist = None

    def grow(ds):
        return min(ds * 3, max_dump) if ds < max_dump else ds

    def emit(tokens):
        codes = torch.tensor([tokens]).to(dev)
        feats = model_handler.wavtokenizer.codes_to_features(codes)
        audio = model_handler.wavtokenizer.decode(feats, bandwidth_id=bandwidth_id).squeeze(0)
        audio_byte_queue.put(audio.detach().cpu().numpy().astype("float32").tobytes())

    with torch.inference_mode():
        while True:
            if not end_of_speech:
                word = text_token_queue.get()
                if word is None:
                    break
                if (eos in word) or (word[-1] == "."):
                    if eos in word:
                        end_generation = True
                    word = word.rstrip(eos)  # a character-set strip, as in the reference
                    end_of_speech = True
                else:
                    end_of_speech = False
                ids = model_handler.tokenizer(word.strip())["input_ids"]
                if end_of_speech:
                    ids = ids + [C.EOS_TEXT_ID]
                text_emb = model_handler.llm_model(torch.tensor(ids).unsqueeze(0).to(dev))
            else:
                text_emb = model_handler.llm_model(torch.tensor([pad_token_id]).unsqueeze(0).to(dev))

            for i in range(text_emb.shape[1]):
                if gen_index == 0:
                    speech = torch.zeros((1, 1, 512), device=dev)
                else:
                    tok_t = torch.tensor([[cur_tok]]).to(dev)
                    speech = model_handler.wavtokenizer.codes_to_features(tok_t).permute(0, 2, 1).to(dev)
                x = torch.cat([text_emb[:, i, :].unsqueeze(1), speech], dim=2)
                x = F.normalize(x, p=2, dim=2, eps=1e-8)
                if gen_index > 0:
                    x = torch.cat([hist, x], dim=1)
                logits, _, kvcache = model_handler.model(x, kvcache=kvcache)
                cur_tok = int(F.softmax(logits[:, -1, :], dim=-1).argmax(dim=-1).item())
                speech_outputs.append(cur_tok)
                hist = x
                gen_index += 1

                if len(speech_outputs) >= dump_size:
                    batch, speech_outputs = speech_outputs[:dump_size], speech_outputs[dump_size:]
                    emit(batch)
                    dump_size = grow(dump_size)
                elif eoa_token_id in speech_outputs:
                    emit(speech_outputs)
                    speech_outputs = []
                    dump_size = grow(dump_size)

                if cur_tok == eoa_token_id or len(speech_outputs) > max_audio_len:
                    if end_generation:
                        audio_byte_queue.put("end")
                    else:
                        audio_byte_queue.put(1 if index == 0 else 0)
                    gen_index, cur_tok, kvcache, hist = 0, None, None, None
                    end_of_speech, end_generation = False, False
                    speech_outputs = []
                    dump_size = grow(dump_size)
    audio_byte_queue.put(None)


def audio_chunks(queue_1: Queue, queue_2: Queue, timeout: float = 1.0, stop: Optional[Callable[[], bool]] = None):
    """Synchronous form of audio_generator_async (streaming_server.py:428-469): yields PCM
    byte chunks in speaking order, switching queues on the 0/1 signals; 'end' closes the
    stream (the reference yields None there, which ends the HTTP response by exception)."""
    qs = [queue_1, queue_2]
    cur = qs[0]
    while True:
        if stop is not None and stop():
            return
        try:
            item = cur.get(True, timeout)
        except Empty:
            continue
        if isinstance(item, str) and item == "end":
            return
        if isinstance(item, int) and not isinstance(item, bool) and item in (0, 1):
            cur = qs[item]
            continue
        if item is None:
            continue
        yield item


async def audio_generator_async(queue_1: Queue, queue_2: Queue):
    loop = asyncio.get_event_loop()
    qs = [queue_1, queue_2]
    cur = qs[0]
    while True:
        try:
            item = await loop.run_in_executor(None, cur.get, True, 1)
        except Empty:
            continue
        if isinstance(item, str) and item == "end":
            return
        if isinstance(item, int) and item in (0, 1):
            cur = qs[item]
            continue
        if item is None:
            continue
        yield item


# ---------------------------------------------------------------------------------------
# 2. token-level state machine of one replica stream (same semantics as above)
# ---------------------------------------------------------------------------------------

@dataclass
class Event:
    kind: str            # "audio" (tokens to decode) or "signal" (0 / 1 / "end")
    tokens: Optional[List[int]] = None
    signal: object = None


@dataclass
class SegmentMachine:
    """The per-token semantics of audio_generator_sync, with the model call factored out:
    ``next_text_id()`` says what the next decode step is fed, ``consume(token)`` applies the
    dump / EOA / reset rules and returns the events, exactly in the reference's order."""
    index: int = 0
    dump_size: int = C.INITIAL_DUMP_SIZE_1
    tokenizer: object = None
    max_audio_len: int = C.MAX_AUDIO_LENGTH
    max_dump: int = C.MAX_DUMP_SIZE
    eos: str = C.EOS_TOKEN
    pad_id: int = C.PAD_TOKEN_ID
    eoa_id: int = C.EOA_TOKEN_ID
    words: Deque[str] = field(default_factory=deque)
    pending: Deque[int] = field(default_factory=deque)
    gen_index: int = 0
    end_of_speech: bool = False
    end_generation: bool = False
    speech_outputs: List[int] = field(default_factory=list)
    closed: bool = False

    def __post_init__(self):
        if self.tokenizer is None:
            from .tokenizer import ByteTokenizer
            self.tokenizer = ByteTokenizer()

    # -- text side --
    def feed(self, word: Optional[str]):
        self.words.append(word)

    def _word_ids(self, word: str):
        """(ids, end of speech, end of generation) of a word; memoised (plan() re-reads the words ahead
        every chunk, and the regex tokenizer costs ~10 us a word)."""
        cache = self.__dict__.setdefault("_ids_cache", {})
        got = cache.get(word)
        if got is None:
            got = cache[word] = self._word_ids_uncached(word)
            if len(cache) > 4096:
                cache.clear()
        ids, eos_flag, end_gen = got
        return list(ids), eos_flag, end_gen

    def _word_ids_uncached(self, word: str):
        eos = self.eos
        if (eos in word) or (word[-1] == "."):
            end_gen = eos in word
            word = word.rstrip(eos)
            eos_flag = True
        else:
            end_gen, eos_flag = False, False
        ids = self.tokenizer(word.strip())["input_ids"]
        if eos_flag:
            ids = ids + [C.EOS_TEXT_ID]
        return ids, eos_flag, end_gen

    def _refill(self) -> bool:
        """Make ``pending`` non-empty; False when the next word has not arrived yet."""
        if self.pending:
            return True
        if self.end_of_speech:
            self.pending.append(self.pad_id)
            return True
        if not self.words:
            return False
        word = self.words.popleft()
        if word is None:
            self.closed = True
            return False
        ids, self.end_of_speech, eg = self._word_ids(word)
        if eg:
            self.end_generation = True
        self.pending.extend(ids)
        return True

    def plan(self, n: int) -> List[int]:
        """The text ids of the next n steps if no end-of-audio occurs (no state change);
        shorter when text is not available yet."""
        out = list(self.pending)[:n]
        eos_flag, words = self.end_of_speech, list(self.words)
        wi = 0
        while len(out) < n:
            if eos_flag:
                out.extend([self.pad_id] * (n - len(out)))
                break
            if wi >= len(words) or words[wi] is None:
                break
            ids, eos_flag, _ = self._word_ids(words[wi])
            wi += 1
            out.extend(ids[: n - len(out)])
        return out

    def next_text_id(self) -> Optional[int]:
        if not self._refill():
            return None
        return self.pending[0]

    # -- token side --
    def _grow(self):
        if self.dump_size < self.max_dump:
            self.dump_size = min(self.dump_size * 3, self.max_dump)

    def consume(self, token: int) -> List[Event]:
        """Apply one greedy token of the step fed ``next_text_id()``."""
        if not self._refill():
            raise RuntimeError("consume() without an available text id")
        self.pending.popleft()
        ev: List[Event] = []
        self.speech_outputs.append(int(token))
        self.gen_index += 1
        if len(self.speech_outputs) >= self.dump_size:
            batch = self.speech_outputs[: self.dump_size]
            self.speech_outputs = self.speech_outputs[self.dump_size:]
            ev.append(Event("audio", tokens=batch))
            self._grow()
        elif self.eoa_id in self.speech_outputs:
            ev.append(Event("audio", tokens=self.speech_outputs))
            self.speech_outputs = []
            self._grow()
        if token == self.eoa_id or len(self.speech_outputs) > self.max_audio_len:
            sig = "end" if self.end_generation else (1 if self.index == 0 else 0)
            ev.append(Event("signal", signal=sig))
            self.gen_index = 0
            self.end_of_speech = False
            self.end_generation = False
            self.speech_outputs = []
            self._grow()
        return ev

    def consume_many(self, tokens) -> tuple:
        """``consume`` over a run of tokens, stopping after a segment end: (events, tokens consumed).
        A run without end-of-audio that stays within max_audio_length takes a batched path (the text
        ids popped at once, the dumps cut as consecutive dump-size slices: exactly what consume does one
        token at a time, since a dump empties the outputs whenever they reach the dump size)."""
        n = len(tokens)
        if self.eoa_id in tokens or len(self.speech_outputs) + n > self.max_audio_len:
            ev: List[Event] = []
            for j, t in enumerate(tokens):
                e = self.consume(int(t))
                ev += e
                if any(x.kind == "signal" for x in e):
                    return ev, j + 1
            return ev, n
        k = n
        while k:
            if not self.pending and self.end_of_speech:
                break  # the rest are PAD steps: _refill would push one PAD id per step and pop it
            if not self._refill():
                raise RuntimeError("consume() without an available text id")
            take = min(k, len(self.pending))
            for _ in range(take):
                self.pending.popleft()
            k -= take
        self.gen_index += n
        buf = self.speech_outputs + [int(t) for t in tokens]  # (ints: tokens may be numpy scalars)
        ev = []
        pos = 0
        while len(buf) - pos >= self.dump_size:
            ev.append(Event("audio", tokens=buf[pos:pos + self.dump_size]))
            pos += self.dump_size
            self._grow()
        self.speech_outputs = buf[pos:]
        return ev, n

    @property
    def position(self):
        return self.gen_index


# ---------------------------------------------------------------------------------------
# fused multi-stream scheduler on the HIP step
# ---------------------------------------------------------------------------------------

class FusedStream:
    def __init__(self, sched, slot, machine: SegmentMachine, sink: Optional[Queue] = None):
        self.sched = sched
        self.slot = slot
        self.m = machine
        self.sink = sink if sink is not None else Queue()
        self.events: List[object] = []   # decoded items in order: bytes or signals
        self.tokens: List[int] = []      # every greedy token consumed (diagnostics / tests)
        self.fed = False                 # a word has been fed (the service caps only fed streams)
        self.sampling = None             # a sampling.Sampling: the slot draws its tokens (open_stream)
        self.index = 0                   # replica index of the request (enters the segment seeds)
        self.segment = 0                 # sentences ended so far: each one draws from a seed of its own
        self.audio = None                # an audio.AudioFormat that converts: the dumps pass the PCM output stage
        self.pcm_open = False            # the sentence has dumps behind it that its filter has not been flushed after
        self.joined: List[int] = []      # a joined stream: the last tokens of its sentence dumped so far (<= 16)

    def feed(self, word):
        self.fed = True
        self.m.feed(word)

    def _out(self, item):
        self.events.append(item)
        self.sink.put(item)


class _JoinedRow(list):
    """The codec row of a joined stream's dump: ``ctx`` context tokens (the last ones its sentence dumped
    before), then the dump's own."""
    ctx = 0


def _dump_ctx(toks) -> int:
    return getattr(toks, "ctx", 0)


def _copy_machine(m: SegmentMachine) -> SegmentMachine:
    """A speculative copy of a machine (its own word / id queues and speech outputs; the tokenizer
    is shared)."""
    c = copy.copy(m)
    c.words = deque(m.words)
    c.pending = deque(m.pending)
    c.speech_outputs = list(m.speech_outputs)
    return c


class _Chunk:
    """One launched AR chunk: its rows, steps, buffer set and completion event; ``bad`` holds the
    streams whose rows it must not consume (rolled back by an end-of-audio of an older chunk)."""

    def __init__(self, ready, n, buf, event, near=None):
        self.ready, self.n, self.buf, self.event, self.near = ready, n, buf, event, near
        self.bad = set()


_LIVE_DELIVERERS: "weakref.WeakSet" = weakref.WeakSet()


@atexit.register
def _close_deliverers():
    """Stop every delivery thread before the interpreter finalises: a daemon thread still inside a
    GIL-releasing torch call (Event.synchronize) when finalisation reclaims it unwinds through a C++
    destructor and the process aborts ("terminate called without an active exception")."""
    for d in list(_LIVE_DELIVERERS):
        d.close()


class _Deliverer:
    """The overlapped scheduler's delivery thread: jobs run in submission order; each waits for its
    codec event (if any), then hands its items to the streams, so a dump reaches its stream as soon
    as its codec call has finished, in the reference's per-stream order."""

    def __init__(self):
        self.q: Queue = Queue()
        self.cv = threading.Condition()
        self.pending = 0
        self.error: Optional[BaseException] = None
        self.thread = threading.Thread(target=self._run, name="lvx-deliver", daemon=True)
        self.thread.start()
        _LIVE_DELIVERERS.add(self)

    def put(self, event, fn):
        with self.cv:
            self.pending += 1
        self.q.put((event, fn))

    def _run(self):
        while True:
            ev, fn = self.q.get()
            if fn is None:
                return
            try:
                if ev is not None:
                    ev.synchronize()
                fn()
            except BaseException as e:  # surfaced on the scheduler thread (take_error)
                from ._lib import LvxStreamError
                if self.error is None:
                    self.error = e
                elif isinstance(self.error, LvxStreamError) and isinstance(e, LvxStreamError):
                    # two groups' codec errors before the scheduler took the first: one error naming both
                    self.error.streams = sorted(set(self.error.streams) | set(e.streams), key=lambda st: st.slot)
            with self.cv:
                self.pending -= 1
                self.cv.notify_all()

    def wait(self):
        with self.cv:
            while self.pending:
                self.cv.wait()

    def take_error(self):
        e, self.error = self.error, None
        if e is not None:
            raise e

    def close(self):
        if self.thread.is_alive():
            self.q.put((None, None))
            self.thread.join(timeout=30)
        _LIVE_DELIVERERS.discard(self)


class _PcmPass:
    """The PCM output-stage calls of one chunk's dumps (streams opened with ``audio``). A slot's calls
    must reach the engine in dump order, whatever order the codec groups are decoded in, and no call may
    name a slot twice: ``run()`` converts, in rounds, every dump that is the next one of its stream and
    whose codec call has been queued, one ``pcm_convert`` per (codec call, rate, encoding, speed, pitch, join, volume,
    formant, pauses or not, the mark), and leaves the others for the ``run()`` after a later group. A dump without tokens is a flush (no codec call)."""

    def __init__(self, sched, dumps, finals):
        self.sched, self.dumps, self.finals = sched, dumps, finals
        self.seq: Dict[FusedStream, Deque[int]] = {}  # stream -> its dumps still to convert, in dump order
        self.where: Dict[int, tuple] = {}             # dump -> (its codec call's PCM rows or None, its row)
        for i, (st, toks) in enumerate(dumps):
            if st is not None and st.audio is not None:
                self.seq.setdefault(st, deque()).append(i)
                if not toks:
                    self.where[i] = (None, 0)

    def converts(self, i) -> bool:
        st = self.dumps[i][0]
        return st is not None and st.audio is not None

    def decoded(self, grp, out):
        for k, i in enumerate(grp):
            self.where[i] = (out, k)

    def run(self):
        """Queue (on the current stream) the calls whose turn has come: [(dump indices, out, counts)]."""
        eng, calls = self.sched.engine, []
        while True:
            buckets: Dict[tuple, List[int]] = {}
            for st, q in self.seq.items():
                if not q or q[0] not in self.where:
                    continue
                i = q.popleft()
                if st in self.sched.failed:  # a codec error ended it: nothing more is delivered to it
                    eng.pcm_reset(st.slot)
                    continue
                buckets.setdefault((id(self.where[i][0]), st.audio.sample_rate, st.audio.encoding,
                                    st.audio.speed_pct, st.audio.pitch_pct, st.audio.join, st.audio.volume_pct,
                                    st.audio.formant_pct, st.audio.pauses, st.audio.mark_key, st.audio.mark_id,
                                    st.audio.mark_strength),
                                   []).append(i)
            if not buckets:
                return calls
            for idx in buckets.values():
                out = self.where[idx[0]][0]
                rows = [self.where[i][1] for i in idx]
                if out is None:
                    pcm = None
                elif rows == list(range(rows[0], rows[0] + len(rows))):
                    pcm = out[rows[0]:rows[0] + len(rows)]
                else:
                    pcm = out[rows]
                audio = self.dumps[idx[0]][0].audio
                kw = {"ctx_frames": [_dump_ctx(self.dumps[i][1]) for i in idx]} if audio.join else {}
                o, counts = eng.pcm_convert(pcm, [self.dumps[i][0].slot for i in idx],
                                            [i in self.finals for i in idx], audio, **kw)
                calls.append((idx, o, counts))


class FusedScheduler:
    """Continuous batching of many replica streams on one Engine.

    A chunk: each stream with text available contributes its planned text ids for the next n steps
    (n ends at the earliest pending dump boundary, so the first chunk of a stream is decoded as soon
    as its tokens exist); the fused step runs n times for all rows (one HIP-graph replay per 16
    steps, no host traffic); tokens are read back once; every stream's SegmentMachine consumes them
    in order; a stream that hits end-of-audio drops its run-ahead tokens and its slot is rewound to
    position 0; all dumps of the chunk are decoded (batched by length) and delivered in order.

    ``overlap=True`` runs the schedule of the reference's two replicas and of the bench
    (streaming_server.py:357-376): chunk c + 1's decode steps are queued on the main
    stream BEFORE chunk c's tokens are read back (planned from the streams' speculative state after
    chunk c without an end-of-audio; a stream whose chunk c does end its segment has its chunk c + 1
    row discarded, and its slot rewound behind it); chunk c's codec runs on a second HIP stream, queued
    only once the host holds its tokens (host-paced: no queue ever waits on the other's event, which
    costs every dispatch of the AR chain ~1 us); each chunk's items are delivered by a
    delivery thread as soon as its codec event completes. Streams see the same items, in the same
    order, as without overlap (tests/test_gpu_streaming.py). Run-ahead is skipped for a chunk whose
    rows would cross max_positions (the capacity edge then behaves as without overlap). On a CPU
    stand-in engine the same run-ahead / rollback / ordering runs with synchronous decodes.

    ``stop_rule(stream, tokens, position)`` (optional): True when a stream must not be planned once it
    has consumed ``tokens`` tokens and stands at ``position`` (the service's max_tokens / capacity
    stop), applied to the speculative state too, so run-ahead never decodes past a stop.

    Joining streams: a chunk longer than ``tail`` steps is queued as two calls with an event between
    them, ``tail`` steps before its end; the next chunk is planned once that event has passed, so a
    stream opened while a chunk runs joins the very next chunk (with run-ahead planned at the chunk's
    start it would wait a whole extra chunk), and the tail steps cover the host's planning.
    ``waiter(event)`` (optional) replaces every host wait on a device event: the service passes one that
    releases its lock meanwhile, so requests are admitted while the scheduler waits for the device.
    ``stream`` (optional): the HIP stream of the decode steps and slot updates, whatever thread calls
    (default: the calling thread's current stream). Decode steps on the legacy null stream run
    without graphs and serialise with every other stream, so the service gives each device one.
    """

    def __init__(self, engine, max_chunk: int = 32, max_rows: Optional[int] = None, to_bytes: bool = True,
                 overlap: bool = False, stop_rule=None, waiter=None, tail: int = 8, stream=None,
                 codec_stream: bool = True):
        import torch
        self.engine = engine
        self.torch = torch
        self.max_chunk = max_chunk
        self.max_rows = max_rows or engine.max_streams
        self.streams: List[FusedStream] = []
        self.free_slots = list(range(engine.max_streams - 1, -1, -1))
        self.to_bytes = to_bytes
        self.stop_rule = stop_rule
        self.waiter = waiter
        self.tail = max(1, int(tail))
        self.ar_stream = stream
        dev = engine.device
        self.cuda = torch.device(dev).type == "cuda"
        self.overlap = bool(overlap)
        # the codec's stream is checked to run beside the decode stream (streams.side_stream: two streams
        # on one hardware queue run in order, and the overlap would be silently lost)
        self.codec_stream = (side_stream(dev, [stream]) if codec_stream else (stream or torch.cuda.current_stream(dev))) \
            if (self.overlap and self.cuda) else None
        self.take = self.cuda and hasattr(engine, "take_errors")
        self.codec_take = hasattr(engine, "take_errors")  # (host-synchronous decodes: any engine with the words)
        self.bufs = [self._alloc() for _ in range(2 if self.overlap else 1)]
        self._bi = 0
        self.inflight: Deque[_Chunk] = deque()
        self.deliverer = _Deliverer() if self.overlap else None
        # streams whose dump failed in the codec (its error word): nothing more is delivered to them,
        # so a client never receives audio after a hole (the error names them; the caller closes them;
        # weak: kept past close_stream, for the jobs of chunks still queued behind the failure)
        self.failed = weakref.WeakSet()

    def _alloc(self):
        torch, dev = self.torch, self.engine.device
        R, n = self.max_rows, self.max_chunk
        pin = self.cuda
        return {"slots_d": torch.full((R,), -1, dtype=torch.int32, device=dev),
                "plan_d": torch.zeros((R, n), dtype=torch.int32, device=dev),
                "rowstep_d": torch.zeros((R,), dtype=torch.int32, device=dev),
                "tok_d": torch.zeros((R, n), dtype=torch.int32, device=dev),
                "err_d": torch.zeros((1,), dtype=torch.int32, device=dev),
                "plan_h": torch.zeros((R, n), dtype=torch.int32, pin_memory=pin),
                "slots_h": torch.full((R,), -1, dtype=torch.int32, pin_memory=pin),
                "tok_h": torch.zeros((R, n), dtype=torch.int32, pin_memory=pin),
                "err_h": torch.zeros((1,), dtype=torch.int32, pin_memory=pin)}

    def open_stream(self, index=0, dump_size=C.INITIAL_DUMP_SIZE_1, sink=None, sampling=None, audio=None,
                    **kw) -> FusedStream:
        """sampling: a ``sampling.Sampling`` (temperature > 0) makes the stream draw its tokens, every
        sentence from ``segment_seed(seed, index, sentence)``; None (or temperature 0): greedy, and the
        engine's ``set_sampling`` is never called.
        audio: an ``audio.AudioFormat`` with another speed, pitch, formant, volume, rate or encoding than f32le at 24 kHz as
        spoken: every dump of the stream is converted on the device (``Engine.pcm_convert``), behind its codec call on the same
        stream, each sentence as a signal of its own, and the stream's items are those samples (float32,
        int16 or, G.711, uint8 arrays with ``to_bytes=False``). None (or 24 kHz f32le): today's items, and the engine's
        ``pcm_*`` are never called. A format with ``join``: every dump of a sentence after its first is decoded
        with context in front, the last min(16, frames of the sentence dumped so far, max_codec_frames - the
        dump's length) tokens dumped before it (``_join_row``), and the output stage crossfades the seam. A format
        that ``pauses``: the items are uint8, whole slots of the pause stage (``audio.pause_slots_ref``), which
        ``audio.PauseMux`` turns into the paced samples where the speaking order is known."""
        if sampling is not None and not sampling.temperature > 0:
            sampling = None
        if sampling is not None and not hasattr(self.engine, "set_sampling"):
            raise RuntimeError("this engine cannot sample (it has no set_sampling): open the stream without `sampling`")
        if audio is not None and not audio.converts:
            audio = None
        if audio is not None and not hasattr(self.engine, "pcm_convert"):
            raise RuntimeError("this engine has no PCM output stage (no pcm_convert): open the stream without `audio`")
        if not self.free_slots:
            raise RuntimeError("no free KV slot")
        slot = self.free_slots.pop()
        st = FusedStream(self, slot, SegmentMachine(index=index, dump_size=dump_size, **kw), sink)
        st.sampling, st.index, st.audio = sampling, index, audio
        with self._on_ar():
            self.engine.reset_slot(slot)  # (stream-ordered behind any chunk in flight on the slot)
            if audio is not None:
                self.engine.pcm_reset(slot)
            self._seed_segment(st)
        self.streams.append(st)
        return st

    def _seed_segment(self, st: FusedStream):
        """Queue (on the AR stream: the caller holds _on_ar) the parameters of the stream's current sentence."""
        if st.sampling is not None:
            from .sampling import segment_seed
            sp = st.sampling
            self.engine.set_sampling(st.slot, sp.temperature, sp.top_k, segment_seed(sp.seed, st.index, st.segment),
                                     **sp.extra())

    def close_stream(self, st: FusedStream):
        self.streams.remove(st)
        self.free_slots.append(st.slot)
        if st.sampling is not None:  # the slot's next stream starts greedy (behind this one's chunks in flight)
            with self._on_ar():
                self.engine.set_sampling(st.slot, 0.0, 0, 0)
        if st.audio is not None:  # (an unfinished sentence's filter state goes with it)
            self.engine.pcm_reset(st.slot)

    def close(self):
        """Stop the delivery thread (after delivering what is queued)."""
        if self.deliverer is not None:
            self.deliverer.wait()
            self.deliverer.close()
            self.deliverer = None

    def _on_ar(self):
        return self.torch.cuda.stream(self.ar_stream) if self.ar_stream is not None else contextlib.nullcontext()

    def _join_row(self, st: FusedStream, tokens: List[int]):
        """The codec row of a dump of committed tokens: for a joined stream its context tokens in front (none
        where the engine has no room for them: that seam is then a plain one), and the record of the
        sentence's dumped tokens moved on; any other stream: the tokens themselves."""
        if st is None or st.audio is None or not st.audio.join or not tokens:
            return tokens
        c = max(0, min(JOIN_CONTEXT, len(st.joined), self.engine.max_codec_frames - len(tokens)))
        row = _JoinedRow(st.joined[len(st.joined) - c:] + list(tokens))
        row.ctx = c
        st.joined = (st.joined + list(tokens))[-JOIN_CONTEXT:]
        return row

    def _steps_to_dump(self, m: SegmentMachine):
        return max(1, m.dump_size - len(m.speech_outputs))

    # -- planning ---------------------------------------------------------------------------
    def _speculative(self):
        """Each stream of the chunk in flight, advanced over that chunk as if it ended no segment:
        {stream: (machine copy or None when the chunk ends its segment anyway, tokens consumed)}."""
        spec = {}
        for ch in self.inflight:
            for st in ch.ready:
                if st in ch.bad or st not in self.streams:
                    continue
                m0, ntok = spec.get(st, (st.m, len(st.tokens)))
                if m0 is None:
                    continue
                m = _copy_machine(m0)
                dummy = 0 if m.eoa_id != 0 else 1
                try:
                    ev, used = m.consume_many([dummy] * ch.n)
                    ends = used < ch.n or any(e.kind == "signal" for e in ev)  # (a max_audio_length reset)
                except RuntimeError:
                    ends = True
                spec[st] = (None if ends else m, ntok + ch.n)
        return spec

    def _launch_next(self) -> int:
        """Plan and queue the next chunk (from the speculative state of the chunk in flight, if any);
        returns its steps, 0 when nothing is ready or run-ahead would cross the capacity edge."""
        torch = self.torch
        if self.inflight and self.inflight[-1].near is not None:
            self._wait(self.inflight[-1].near)  # `tail` steps before the chunk in flight ends
            self.inflight[-1].near = None
        spec = self._speculative() if self.inflight else {}
        ready = []
        for st in self.streams:
            m, ntok = spec.get(st, (st.m, len(st.tokens)))
            if m is None or m.closed or m.next_text_id() is None:
                continue
            if self.stop_rule is not None and self.stop_rule(st, ntok, m.position):
                continue
            ready.append((st, m))
        ready = ready[: self.max_rows]
        if not ready:
            return 0
        n = min(self.max_chunk, min(self._steps_to_dump(m) for _, m in ready))
        plans = []
        for st, m in ready:
            p = m.plan(n)
            plans.append(p)
            n = min(n, len(p))
        if self.inflight and any(m.position + n > self.engine.max_positions for _, m in ready):
            return 0  # the capacity edge: complete the chunk in flight first (no run-ahead)
        with self._on_ar():
            return self._launch(ready, plans, n)

    def _launch(self, ready, plans, n) -> int:
        torch = self.torch
        buf = self.bufs[self._bi]
        self._bi = (self._bi + 1) % len(self.bufs)
        B = len(ready)
        sl = buf["slots_h"].numpy()
        sl[:] = -1
        sl[:B] = [st.slot for st, _ in ready]
        buf["plan_h"].numpy()[:B, :n] = np.array([p[:n] for p in plans], dtype=np.int32)
        buf["slots_d"].copy_(buf["slots_h"], non_blocking=True)
        buf["plan_d"].copy_(buf["plan_h"], non_blocking=True)
        buf["rowstep_d"].zero_()
        args = (buf["slots_d"][:B], buf["plan_d"][:B], buf["rowstep_d"][:B], buf["tok_d"][:B])
        near = None
        if self.overlap and self.cuda and n >= 2 * self.tail:  # (a short chunk is planned behind at once)
            # (round 5, measured worse: the head rounded down to whole 16-step graph replays moved the
            # planning point up to 16 steps before the chunk's end, and a request arriving in that window
            # waits for the whole next chunk: loaded first chunk p50 11.2 / 13.8 vs 9.0 / 10.2 ms,
            # tools/latency_ab.py 32)
            head = n - self.tail
            self.engine.ar_steps(head, *args)
            near = torch.cuda.Event()
            near.record(torch.cuda.current_stream(self.engine.device))
            self.engine.ar_steps(n - head, *args)
        else:
            self.engine.ar_steps(n, *args)
        ev = None
        if self.cuda:
            buf["tok_h"].copy_(buf["tok_d"], non_blocking=True)
            if self.take:
                from . import _lib
                self.engine.take_errors(_lib.ERRW_AR, buf["err_d"])
                buf["err_h"].copy_(buf["err_d"], non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(torch.cuda.current_stream(self.engine.device))
        self.inflight.append(_Chunk([st for st, _ in ready], n, buf, ev, near))
        return n

    def _wait(self, ev):
        if self.waiter is not None:
            self.waiter(ev)
        else:
            ev.synchronize()

    # -- completion --------------------------------------------------------------------------
    def _chunk_error(self, ch):
        if not self.take:  # a stand-in engine: its own (synchronous) check
            try:
                self.engine.check_errors()
            except Exception as e:
                return e
            return None
        bits = int(ch.buf["err_h"][0])
        if not bits:
            return None
        from . import _lib
        return _lib.error_for(self.engine.lib.lvx_error_status(bits), bits)

    def _complete(self, ch: _Chunk) -> int:
        """Read back the chunk's tokens (waits for its event only), consume them, queue its decodes."""
        if ch.event is not None:
            self._wait(ch.event)
        B, n = len(ch.ready), ch.n
        toks = (ch.buf["tok_h"] if self.cuda else ch.buf["tok_d"])[:B, :n].numpy()
        err = self._chunk_error(ch)
        # a KV-capacity error concerns only the rows that reached max_positions in this chunk (their
        # last positions were clamped); every other row's tokens are valid and are consumed, decoded
        # and delivered below before the error is raised, naming the streams at the edge. A fused-MLP
        # range error (B <= 2) invalidates the logits of this chunk's rows: they are named the same way
        from ._lib import LvxCapacityError, LvxNumericError
        edge, at_cap = set(), set()
        live = [st for st in ch.ready if st in self.streams and st not in ch.bad]  # (rows still consumed)
        if err is not None:
            if isinstance(err, LvxCapacityError):
                # a row that ran past max_positions had its last positions clamped: those tokens are
                # invalid. A row that ends exactly AT max_positions set the flag with the commit of
                # its last step, but all n of its tokens came from positions <= max_positions - 1:
                # they are consumed below, then the row is reported at capacity
                P = self.engine.max_positions
                bits = getattr(err, "bits", 0) or 0  # (device bits: 1 KV capacity, 2 a plan overrun)
                if bits & 2:
                    raise err
                # the rows at the edge among the live ones (a discarded row's machine was rewound by its
                # end of audio: its host position no longer says where its device row ran)
                if not any(st.m.position + n >= P for st in live):
                    if len(live) == len(ch.ready):
                        raise err  # no row can have reached the edge: not a capacity condition of ours
                    err = None  # only discarded rows can have run into it: their tokens are dropped anyway
                else:
                    edge = {st for st in live if st.m.position + n > P}
                    at_cap = {st for st in live if st.m.position + n == P}
            elif isinstance(err, LvxNumericError):
                edge = set(live)
            else:
                raise err
            # the named streams' rows in newer chunks (planned assuming this chunk was consumed) are not
            # consumed either: the caller ends those streams
            for st in edge | at_cap:
                for newer in self.inflight:
                    newer.bad.add(st)
            # (an error of rows already discarded -- a closed stream, a run-ahead row rolled back --
            # concerns no live stream: nothing is raised for it below)
        dumps = []  # (stream, tokens)
        order: Dict[FusedStream, List[tuple]] = {st: [] for st in ch.ready}
        ended = set()
        for r, st in enumerate(ch.ready):
            if st in edge or st in ch.bad or st not in self.streams:
                continue
            row = toks[r].tolist()
            evs, used = st.m.consume_many(row)
            st.tokens.extend(row[:used])
            reset = False
            for e in evs:
                if e.kind == "audio":
                    dumps.append((st, self._join_row(st, e.tokens)))
                    order[st].append(("audio", len(dumps) - 1))
                else:
                    order[st].append(("signal", e.signal))
                    st.joined = []  # (the sentence ends: an end of audio or the max_audio_length reset)
                    reset = True
            if reset:
                # run-ahead past end-of-audio: drop the rest, restart the slot at position 0
                # (queued behind any newer chunk in flight, whose row of this stream is discarded)
                # (a sampling stream: the next sentence's seed in the same place in stream order, so the
                # discarded run-ahead rows and the serial schedule see the same parameters)
                st.segment += 1
                with self._on_ar():
                    self.engine.set_slot(st.slot, 0, 0)
                    self._seed_segment(st)
                for newer in self.inflight:
                    newer.bad.add(st)
                ended.add(st)
        # a row that reached the capacity exactly AND ended its segment in this chunk was rewound to
        # position 0 by the end of audio: it continues, as the reference would
        at_cap -= ended
        codec_err = None
        finals = self._mark_finals(dumps, order)  # (None: no stream of the chunk converts its audio)
        if self.overlap:
            self._launch_decode(dumps, order, ch.ready, finals)
        else:
            pcm, codec_err = self._decode(dumps, finals)
            self._deliver(pcm, order, ch.ready)
        if err is not None:
            if self.deliverer is not None:
                self.deliverer.wait()
            err.streams = sorted(edge | at_cap | set(codec_err.streams if codec_err else ()), key=lambda st: st.slot)
            if err.streams:
                raise err
        if codec_err is not None:
            raise codec_err
        return n

    def run_chunk(self) -> int:
        """Serial: one chunk for all ready streams, its items delivered on return. Overlap: queue the
        next chunk, then complete the one in flight before it (its items are delivered when its codec
        call ends). Returns the steps queued or completed (0 = idle: everything delivered)."""
        if self.deliverer is not None:
            self.deliverer.take_error()
        launched = self._launch_next()
        if self.inflight and (len(self.inflight) > 1 or not launched or not self.overlap):
            done = self._complete(self.inflight.popleft())
            return launched or done
        if not launched:
            self.flush()
        return launched

    def _deliver(self, pcm, order, ready):
        for st in ready:
            if st in self.failed:
                continue
            for kind, v in order[st]:
                st._out(pcm[v] if kind == "audio" else v)

    def _codec_failure(self, exc, streams):
        """A codec call's error word was set: the streams of its dumps get nothing more (``failed``) and
        the error is re-raised as an LvxStreamError naming them (the service ends only their requests);
        an error of a call that carries no stream's dump (decode_now) is returned as it was."""
        from ._lib import LvxStreamError
        streams = [st for st in streams if st is not None]
        if not streams:
            return exc
        for st in streams:
            self.failed.add(st)
        se = LvxStreamError(getattr(exc, "code", -2), f"codec error word: {exc}")
        se.bits = getattr(exc, "bits", 0)
        se.streams = sorted(set(streams), key=lambda st: st.slot)
        return se

    def _groups(self, dumps):
        """Dump indices batched by decoded length, a joined dump's context included (one codec call per group,
        within max_codec_frames)."""
        by_len: Dict[int, List[int]] = {}
        for i, (_, toks) in enumerate(dumps):
            if toks:  # (no tokens: a flush of the PCM output stage, _mark_finals)
                by_len.setdefault(len(toks), []).append(i)
        for L, idx in by_len.items():
            cap = max(1, self.engine.max_codec_frames // L)
            for s in range(0, len(idx), cap):
                yield L, idx[s:s + cap]

    def _mark_finals(self, dumps, order):
        """The PCM output stage's view of a chunk's (or a tail's) items: the dumps that end a sentence, for
        the streams that convert their audio. A dump is final when the stream's next item is a signal; a
        sentence that ends with no dump behind its last audio (the max_audio_length reset drops its
        outputs) gets a flush appended to ``dumps`` (no tokens) and queued in front of its signal, so every
        sentence delivers exactly ceil(T L / M) samples. Returns the set of final dump indices, or None
        when no stream with items converts (the caller then takes today's path, call for call)."""
        finals = None
        for st, items in order.items():
            if st.audio is None or not items:
                continue
            finals = set() if finals is None else finals
            k = 0
            while k < len(items):
                kind, v = items[k]
                if kind == "audio":
                    st.pcm_open = not (k + 1 < len(items) and items[k + 1][0] == "signal")
                    if not st.pcm_open:
                        finals.add(v)
                elif st.pcm_open:
                    dumps.append((st, []))
                    items.insert(k, ("audio", len(dumps) - 1))
                    finals.add(len(dumps) - 1)
                    st.pcm_open = False
                    k += 1
                k += 1
        return finals

    def _host_item(self, a):
        return a.tobytes() if self.to_bytes else a.copy()

    def _decode(self, dumps, finals=None):
        """Every dump decoded now (one call per length group), host-synchronous. Returns (PCM per dump,
        None or the LvxStreamError naming the streams of the groups whose codec error word was set:
        the other groups' PCM is valid and delivered). ``finals`` (_mark_finals; None: no dump is
        converted): the dumps of streams with an audio format go through the PCM output stage behind their
        codec call, and only their converted rows are copied to the host."""
        torch = self.torch
        res: List[object] = [None] * len(dumps)
        first, bad = None, []
        pp = _PcmPass(self, dumps, finals) if finals is not None else None

        def converted():
            for idx, o, counts in pp.run():
                host = o.cpu().numpy()
                for r, i in enumerate(idx):
                    res[i] = self._host_item(host[r, :counts[r]])

        for L, grp in self._groups(dumps):
            codes = torch.tensor([dumps[i][1] for i in grp], dtype=torch.int32, device=self.engine.device)
            dev_out = self.engine.decode_codes(codes)
            plain = [k for k, i in enumerate(grp) if pp is None or not pp.converts(i)]
            if plain:  # (the rows delivered as the codec wrote them; all of them without an audio format)
                out = (dev_out if len(plain) == len(grp) else dev_out[plain]).cpu().numpy()
                for r, k in enumerate(plain):
                    res[grp[k]] = out[r].astype("float32").tobytes() if self.to_bytes else out[r]
            if pp is not None:
                pp.decoded(grp, dev_out)
                converted()
            if self.codec_take:  # the codec's own error word, per group
                from . import _lib
                e = torch.zeros((1,), dtype=torch.int32, device=self.engine.device)
                self.engine.take_errors(_lib.ERRW_CODEC, e)
                try:
                    _lib.check_bits(int(e.item()))
                except _lib.LvxError as exc:
                    first = first or exc
                    bad += [dumps[i][0] for i in grp]
        if pp is not None:
            converted()  # (flushes of streams without a dump in the chunk)
        return res, (self._codec_failure(first, bad) if first is not None else None)

    def decode_now(self, tokens: List[int]):
        """One dump decoded and returned at once, on the codec stream when overlapping, so it does not
        queue behind the decode chunk in flight (raises for the codec's error word)."""
        torch = self.torch
        with (torch.cuda.stream(self.codec_stream) if self.codec_stream is not None else contextlib.nullcontext()):
            res, err = self._decode([(None, tokens)])
        if err is not None:
            raise err
        return res[0]

    def queue_tail(self, st: FusedStream, tokens: List[int]):
        """The stream's undumped tail decoded as one last dump and delivered AFTER every item already
        queued for it (the service's end of a request). Overlap: queued on the codec stream, delivered by
        the delivery thread behind its event (the caller never waits for the device); serial: now.
        A stream with an audio format: the tail ends its sentence (a final dump of the PCM output stage);
        no tokens: only the flush of the dumps already delivered."""
        dumps, order = [(st, tokens)], {st: [("audio", 0)]}
        if st.audio is not None:
            if not tokens and not st.pcm_open:
                return
            st.pcm_open = False
            dumps[0] = (st, self._join_row(st, tokens))  # (a joined stream: the tail gets its context too)
            st.joined = []
            if self.deliverer is None:
                with (self.torch.cuda.stream(self.codec_stream) if self.codec_stream is not None
                      else contextlib.nullcontext()):
                    res, err = self._decode(dumps, {0})
                if err is not None:
                    raise err
                st._out(res[0])
            else:
                self._launch_decode(dumps, order, [st], {0})
            return
        if self.deliverer is None:
            st._out(self.decode_now(tokens))
            return
        self._launch_decode(dumps, order, [st])

    def after_delivered(self, fn):
        """fn() once every item queued so far has been delivered (in the delivery order)."""
        if self.deliverer is None:
            fn()
        else:
            self.deliverer.put(None, fn)

    def _launch_decode(self, dumps, order, ready, finals=None):
        """Queue the chunk's decodes on the codec stream (codes from the host: no wait on the AR
        stream), one call per dump length, shortest first, each with its PCM copied into pinned host
        memory and a delivery job behind its own event: a stream's items go out with the job of its
        (last) dump as soon as that call ends; a 10-frame first dump does not wait for a 1,280-frame one
        of the same chunk. Streams without a dump in the chunk are served by the first job.
        ``finals`` (_mark_finals): some stream converts its audio, see _launch_decode_audio."""
        torch = self.torch
        if not self.cuda:  # a stand-in engine: decode now, deliver in order through the same thread
            pcm, err = self._decode(dumps, finals)

            def job():
                self._deliver(pcm, order, ready)
                if err is not None:
                    raise err
            self.deliverer.put(None, job)
            return
        if finals is not None:
            self._launch_decode_audio(dumps, order, ready, finals)
            return
        groups = sorted(self._groups(dumps), key=lambda g: g[0])
        if not groups:
            self.deliverer.put(None, lambda: self._deliver([], order, ready))
            return
        from . import _lib
        dev = self.engine.device
        gi = {i: g for g, (_, grp) in enumerate(groups) for i in grp}
        last = {}  # stream -> the group whose job delivers its items
        for st in ready:
            idx = [gi[v] for kind, v in order[st] if kind == "audio"]
            last[st] = max(idx) if idx else 0
        to_bytes, nd = self.to_bytes, len(dumps)
        pcm: List[object] = [None] * nd  # filled by the jobs, in order
        for g, (L, grp) in enumerate(groups):
            host = torch.empty(len(grp) * 320 * L, dtype=torch.float32, pin_memory=True)
            err_h = torch.zeros((1,), dtype=torch.int32, pin_memory=True)
            codes = torch.tensor([dumps[i][1] for i in grp], dtype=torch.int32).pin_memory()
            with torch.cuda.stream(self.codec_stream):
                out = self.engine.decode_codes(codes.to(dev, non_blocking=True))
                host.view(out.shape).copy_(out, non_blocking=True)
                err_d = torch.zeros((1,), dtype=torch.int32, device=dev)
                self.engine.take_errors(_lib.ERRW_CODEC, err_d)
                err_h.copy_(err_d, non_blocking=True)
                ev = torch.cuda.Event()
                ev.record(self.codec_stream)
            sts = [st for st in ready if last[st] == g]

            def deliver(host=host, err_h=err_h, grp=grp, L=L, sts=sts, codes=codes):  # (codes: kept alive)
                # a set codec error word fails this group's streams only: the
                # other streams of the job, and the other groups' jobs, are still delivered
                exc = None
                try:
                    _lib.check_bits(int(err_h[0]))
                except _lib.LvxError as e:
                    exc = self._codec_failure(e, [dumps[i][0] for i in grp])
                if exc is None:
                    for k, i in enumerate(grp):
                        a = host[k * 320 * L:(k + 1) * 320 * L].numpy()
                        pcm[i] = a.tobytes() if to_bytes else a.copy()
                self._deliver(pcm, order, sts)
                if exc is not None:
                    raise exc

            self.deliverer.put(ev, deliver)

    def _launch_decode_audio(self, dumps, order, ready, finals):
        """_launch_decode for a chunk in which some stream converts its audio: the same codec calls in the
        same order; behind each, on the codec stream, the PCM output-stage calls whose turn has come
        (_PcmPass), and the copies to pinned host memory of exactly what is delivered: the f32 rows of the
        streams without a format, the converted rows of the others. The job behind a call's event hands out
        the rows that are on the host by then and serves every stream all of whose dumps are."""
        torch = self.torch
        from . import _lib
        dev = self.engine.device
        groups = sorted(self._groups(dumps), key=lambda g: g[0])
        pp = _PcmPass(self, dumps, finals)
        nd = len(dumps)
        pcm: List[object] = [None] * nd  # filled by the jobs, in order
        on_host = set()                  # dumps whose rows' copies are queued (known when a job is put)
        served = set()

        def convert(fills, keep):
            for idx, o, counts in pp.run():
                h = torch.empty(o.shape, dtype=o.dtype, pin_memory=True)
                h.copy_(o, non_blocking=True)
                keep.append(o)
                for r, i in enumerate(idx):
                    fills.append((i, h, r, counts[r]))
                    on_host.add(i)

        def put(ev, fills, err_h, grp, keep):
            sts = [st for st in ready if st not in served
                   and all(v in on_host for kind, v in order[st] if kind == "audio")]
            served.update(sts)

            def deliver():  # (keep: the device rows and the codes, alive until their copies have run)
                exc = None
                if err_h is not None:
                    try:
                        _lib.check_bits(int(err_h[0]))
                    except _lib.LvxError as e:
                        exc = self._codec_failure(e, [dumps[i][0] for i in grp])
                for i, h, r, n in fills:
                    if dumps[i][0] not in self.failed:
                        pcm[i] = self._host_item(h[r, :n].numpy())
                self._deliver(pcm, order, sts)
                keep.clear()
                if exc is not None:
                    raise exc

            self.deliverer.put(ev, deliver)

        for L, grp in groups:
            fills, keep = [], []
            err_h = torch.zeros((1,), dtype=torch.int32, pin_memory=True)
            codes = torch.tensor([dumps[i][1] for i in grp], dtype=torch.int32).pin_memory()
            keep.append(codes)
            with torch.cuda.stream(self.codec_stream):
                out = self.engine.decode_codes(codes.to(dev, non_blocking=True))
                plain = [k for k, i in enumerate(grp) if not pp.converts(i)]
                if plain:
                    sub = out if len(plain) == len(grp) else out[plain]
                    h = torch.empty(sub.shape, dtype=torch.float32, pin_memory=True)
                    h.copy_(sub, non_blocking=True)
                    keep.append(sub)
                    for r, k in enumerate(plain):
                        fills.append((grp[k], h, r, 320 * L))
                        on_host.add(grp[k])
                err_d = torch.zeros((1,), dtype=torch.int32, device=dev)
                self.engine.take_errors(_lib.ERRW_CODEC, err_d)
                err_h.copy_(err_d, non_blocking=True)
                pp.decoded(grp, out)
                convert(fills, keep)
                ev = torch.cuda.Event()
                ev.record(self.codec_stream)
            put(ev, fills, err_h, grp, keep)
        if not groups or len(served) < len(ready):  # flushes (and signals) of streams without a dump in the chunk
            fills, keep = [], []
            with torch.cuda.stream(self.codec_stream):
                convert(fills, keep)
                ev = torch.cuda.Event()
                ev.record(self.codec_stream)
            put(ev, fills, None, [], keep)

    def flush(self):
        """Complete every chunk in flight and deliver everything queued."""
        while self.inflight:
            self._complete(self.inflight.popleft())
        if self.deliverer is not None:
            self.deliverer.wait()
            self.deliverer.take_error()

    def run_until_idle(self, max_chunks: int = 1 << 30) -> int:
        total = 0
        for _ in range(max_chunks):
            n = self.run_chunk()
            if n == 0:
                break
            total += n
        self.flush()
        return total
