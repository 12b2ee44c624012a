"""Voice cache: the codec-decoder state of a voice's reference frames, kept across requests.

A voice-clone (ICL) request's audio is the decode of cat(ref_code, codes) cut at the reference / generated boundary,
so the serving routes need a codec row in the state "after R reference frames" before the request's first frame.
That state depends on the reference codes alone.  `VoiceCache` keeps it per voice: built once on a one-row
`codec.RowCodecStream` of its own (never through the serving stream's feeds), exported with qt_codec_row_state, and
adopted into the request's row -- one launch for all rows that adopt in a report.

`joint_walk` is the chunk walk both the serving loop and the warm-up follow, `plan_feed` and `feed_span` the loop's
choice of a feed's frames and of the samples a row hands out from it.  The bookkeeping and the walk touch no
device API, so this module imports (and is tested) without a GPU; only building an entry needs one.
"""
from __future__ import annotations

import threading
import weakref
from collections import OrderedDict
from dataclasses import dataclass
from typing import List, Optional, Tuple

import numpy as np

REF_CHUNK, REF_CTX = 300, 25  # Qwen3TTSTokenizerV2Decoder.chunked_decode (K:885-895)
TAIL = 555                    # samples of a chunk's decode that need the frame after it (dropped at a chunk's end)
WARM_CAPS = (8, 32)           # feed capacities of the warm-up stream (one captured codec graph each)


def joint_walk(R: int, lo: int, f: int, chunk: int = REF_CHUNK, ctx: int = REF_CTX) -> Tuple[List[int], dict]:
    """The codec feed list of a request's generated frames [lo, f), R reference frames in front of them: generated
    frame t sits at joint position R + t of cat(ref, codes), and a position that is a multiple of `chunk` opens a
    reference chunk -- the row restarts there, after position 0 on the chunk's `ctx` context frames, whose output is
    discarded.  Returns (todo, marks): the joint positions to feed in order, and {index in todo at which the row
    (re)starts: context frames fed from there}."""
    todo, marks = [], {}
    for t in range(lo, f):
        j = R + t
        if j % chunk == 0:
            c = ctx if j else 0
            marks[len(todo)] = c
            todo += range(j - c, j)
        todo.append(j)
    return todo, marks


def plan_feed(todo, marks, at: int, cap: int) -> Tuple[int, int]:
    """The next feed of a row that stands at index `at` of its feed list: (frames it takes, does it begin).  A restart
    opens a feed of its own, so the frames stop in front of the next mark."""
    hi = min(len(todo), at + cap)
    nxt = [m for m in marks if at < m < hi]
    n = (min(nxt) if nxt else hi) - at
    return n, int(n > 0 and at in marks)


def boundary_skip(R: int, chunk: int = REF_CHUNK, tail: int = TAIL) -> Tuple[bool, int]:
    """How a request with R reference frames starts: (adopt, samples to drop before its output).  The decode of
    cat(ref, codes) loses `tail` samples at every chunk end, so joint frame j of chunk k starts at sample
    1920 j - tail k of it, and a chunk that has been fed m >= 1 frames has produced 1920 m - tail samples.  With
    R % chunk != 0 the row adopts the state after R - chunk k frames of chunk k = R // chunk, and the request's output
    (from sample 1920 R of the decode) starts tail (k + 1) samples into the next feed.  With R % chunk == 0 the first
    generated frame opens chunk k itself: nothing to adopt, and tail k samples go after the context's."""
    k = R // chunk
    return (True, tail * (k + 1)) if R % chunk else (False, tail * k)


def feed_span(begin, nrow: int, ctx_s: int, ended, final, nz: int, discard: int, extra: int, cum: int, up: int,
              tail: int = TAIL) -> Tuple[int, int, bool, int, int, int]:
    """The samples a row hands out from one feed of nrow frames, whose decode is [0, up * nrow) of the feed's PCM row
    (a feed that begins has nothing in its first `tail` samples).  begin: the row (re)starts with this feed, on ctx_s
    samples of context (the feed's mark, in samples) whose output is dropped, and `extra` more at the request's first
    begin (boundary_skip without adoption); discard: samples still to drop from earlier feeds; ended: the request's
    frames are all known, nz nonzero cb0 among reference and generated ones, so the 1920 x #nonzero-cb0 length rule
    cuts at up * nz; final: this is the last feed of the row's list; cum: the sample of the request's whole decode the
    row has reached.  Returns (lo, hi, last, discard, extra, cum): the span [lo, hi) to hand out, whether it is the
    request's last, and the new state."""
    if begin:
        discard, extra = ctx_s + extra, 0
    lo, hi = tail if begin else 0, up * nrow
    d = min(discard, hi - lo)
    lo += d
    if ended:
        hi = min(hi, lo + max(up * nz - cum, 0))
    return lo, hi, bool(ended and final), discard - d, extra, cum + hi - lo


@dataclass
class VoiceEntry:
    R: int                 # reference frames
    nz: int                # nonzero cb0 among them (the reference's share of the 1920 x #nonzero-cb0 length rule)
    snapshot: object       # codec.CodecRowSnapshot at joint position R, or None: R % 300 == 0, nothing to adopt
    ref: object            # device int32 [R][Q]: the reference codes, for qt_codec_feed_codes
    nbytes: int
    event: object = None   # recorded behind the export that filled the snapshot
    stream: object = None  # the stream it was recorded on

    @property
    def adopts(self) -> bool:
        return self.snapshot is not None


class VoiceCache:
    """Reference-voice entries keyed by the reference codes (R and the int32 [R, Q] contents), LRU by bytes.

    A cache binds to the first codec decoder that uses it (weights, dtype, geometry); passing it to another raises
    ValueError.  The bookkeeping takes a lock; adopted state is a copy, so evicting an entry never touches a running
    request.  An entry that does not fit max_bytes serves the request that built it and is not kept, so
    VoiceCache(max_bytes=0) serves correctly and always misses."""

    def __init__(self, max_bytes: int = 256 << 20):
        self.max_bytes = int(max_bytes)
        self._lock = threading.Lock()
        self._entries: "OrderedDict[tuple, VoiceEntry]" = OrderedDict()
        self._bytes = 0
        self._owner = None  # weakref to the decoder
        self._sig = None
        self._n = dict(hits=0, misses=0, stores=0, evictions=0)

    # ------------------------------------------------------------------ keys
    @staticmethod
    def codes_array(codes) -> np.ndarray:
        """Reference codes (list / tensor / array [R, Q]) as a contiguous int32 array."""
        if hasattr(codes, "detach"):
            codes = codes.detach().cpu().numpy()
        a = np.ascontiguousarray(np.asarray(codes), dtype=np.int32)
        if a.ndim != 2:
            raise ValueError(f"reference codes are [R, Q] integers, got shape {a.shape}")
        return a

    @classmethod
    def key(cls, codes) -> tuple:
        a = cls.codes_array(codes)
        return (int(a.shape[0]), int(a.shape[1]), a.tobytes())

    # ------------------------------------------------------------------ bookkeeping
    def bind(self, decoder):
        """Bind to `decoder` (first use), or check that it is the decoder this cache is bound to."""
        sig = decoder.signature()
        with self._lock:
            if self._owner is None:
                self._owner, self._sig = weakref.ref(decoder), sig
                return
            if self._owner() is not decoder or self._sig != sig:
                raise ValueError("this VoiceCache is bound to another codec decoder (its entries are that decoder's "
                                 "row state: weights, dtype and geometry); use one cache per speech tokenizer")

    def fits(self, nbytes: int) -> bool:
        return int(nbytes) <= self.max_bytes

    def lookup(self, key: tuple) -> Optional[VoiceEntry]:
        """The entry of `key`, now the most recently used (a hit), or None (a miss)."""
        with self._lock:
            e = self._entries.get(key)
            if e is None:
                self._n["misses"] += 1
                return None
            self._entries.move_to_end(key)
            self._n["hits"] += 1
            return e

    def store(self, key: tuple, entry: VoiceEntry) -> bool:
        """Keep `entry`, evicting least recently used entries until it fits.  An entry larger than max_bytes is not
        stored; a key that is present already keeps its entry.  True when stored."""
        nbytes = int(entry.nbytes)
        with self._lock:
            if nbytes > self.max_bytes or key in self._entries:
                return False
            while self._entries and self._bytes + nbytes > self.max_bytes:
                _, old = self._entries.popitem(last=False)
                self._bytes -= old.nbytes
                self._n["evictions"] += 1
            self._entries[key] = entry
            self._bytes += nbytes
            self._n["stores"] += 1
            return True

    def clear(self):
        """Drop every entry (the counters stay)."""
        with self._lock:
            self._entries.clear()
            self._bytes = 0

    def keys(self) -> List[tuple]:
        """The keys held, least recently used first."""
        with self._lock:
            return list(self._entries)

    @property
    def stats(self) -> dict:
        with self._lock:
            return dict(self._n, entries=len(self._entries), bytes=self._bytes)

    # ------------------------------------------------------------------ entries (GPU)
    def get(self, decoder, codes) -> VoiceEntry:
        """The entry of a request's reference codes: looked up (a hit) or built now (a miss) and stored if it fits.
        Runs on the current stream; the caller waits on entry.event before it adopts."""
        a = self.codes_array(codes)
        key = (int(a.shape[0]), int(a.shape[1]), a.tobytes())
        e = self.lookup(key)
        if e is None:
            e = build_entry(decoder, a)
            self.store(key, e)
        return e

    def warm(self, model_or_tokenizer, voice_clone_prompt) -> int:
        """Fill the entries of a prompt's ICL items ahead of any request (call it next to create_voice_clone_prompt):
        voice_clone_prompt is the wrapper's list of VoiceClonePromptItem or the model's dict.  Counts neither hits nor
        misses.  Returns the number of entries built."""
        dec = decoder_of(model_or_tokenizer)
        self.bind(dec)
        if isinstance(voice_clone_prompt, dict):
            refs = voice_clone_prompt.get("ref_code") or []
            icl = voice_clone_prompt.get("icl_mode") or [True] * len(refs)
        else:
            refs = [it.ref_code for it in voice_clone_prompt]
            icl = [it.icl_mode for it in voice_clone_prompt]
        built = 0
        for ref, on in zip(refs, icl):
            if ref is None or not on:
                continue
            a = self.codes_array(ref)
            key = (int(a.shape[0]), int(a.shape[1]), a.tobytes())
            with self._lock:
                have = key in self._entries
            if have or a.shape[0] == 0:
                continue
            if self.store(key, build_entry(dec, a)):
                built += 1
        return built


def decoder_of(x):
    """The codec.CodecDecoder behind a Qwen3TTSModel, a TTSModel, a Qwen3TTSTokenizer or itself."""
    from .codec import CodecDecoder
    o = x
    for _ in range(5):
        if isinstance(o, CodecDecoder):
            return o
        nxt = getattr(o, "speech_tokenizer", None)
        o = nxt if nxt is not None else getattr(o, "model", None)
        if o is None:
            break
    raise ValueError(f"no codec decoder behind a {type(x).__name__}: pass the model (with its speech tokenizer "
                     "loaded) or the Qwen3TTSTokenizer")


def check_codes(decoder, a: np.ndarray):
    """Reference codes the decoder cannot look up are refused (the codebook gather does not check its ids)."""
    Q, cb = int(decoder.tables.shape[0]), int(decoder.tables.shape[1])
    if int(a.shape[1]) != Q:
        raise ValueError(f"reference codes have {int(a.shape[1])} codebooks, the decoder {Q}")
    if a.size and (int(a.min()) < 0 or int(a.max()) >= cb):
        raise ValueError(f"reference codes must lie in [0, {cb}); got [{int(a.min())}, {int(a.max())}]")


def build_entry(decoder, a: np.ndarray) -> VoiceEntry:
    """Decode the reference frames the state at joint position R depends on -- chunk k = R // 300 of the reference,
    begun on its 25 context frames when k > 0 -- on a one-row RowCodecStream of its own, on the current stream, and
    export the row.  The walk is the serving loop's (joint_walk)."""
    import torch
    dec = decoder
    check_codes(dec, a)
    R, Q = int(a.shape[0]), int(a.shape[1])
    dev = dec.dev
    ref = torch.from_numpy(a).to(dev)
    nz = int((a[:, 0] != 0).sum())
    snap = None
    if R % REF_CHUNK:
        todo, marks = joint_walk(0, (R // REF_CHUNK) * REF_CHUNK, R)
        assert list(marks) == [0]
        plan, at = [], 0
        while at < len(todo):  # (take, capacity) of every feed
            take, _ = plan_feed(todo, marks, at, WARM_CAPS[-1])
            plan.append((take, next(c for c in WARM_CAPS if c >= take)))
            at += take
        host = np.zeros((sum(c for _, c in plan), Q), dtype=np.int32)  # the feeds' windows back to back, zero filler
        at = o = 0
        for take, c in plan:
            host[o:o + take] = a[todo[at:at + take]]
            at, o = at + take, o + c
        seq = torch.from_numpy(host).to(dev)
        rs = dec.row_stream(1, REF_CTX + REF_CHUNK, WARM_CAPS[-1])
        try:
            o = 0
            for i, (take, c) in enumerate(plan):
                rs.feed(seq[None, o:o + c], [take], [int(i == 0)])
                o += c
            snap = rs.export_row(0)
        finally:
            rs.close()
    ev = torch.cuda.Event()
    st = torch.cuda.current_stream(dev)
    ev.record(st)
    nbytes = int(ref.numel() * ref.element_size()) + (0 if snap is None else int(snap.nbytes))
    return VoiceEntry(R, nz, snap, ref, nbytes, ev, st)
