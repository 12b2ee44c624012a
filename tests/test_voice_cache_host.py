"""CPU-only: the voice cache's host side (qwen_tts/voice.py) -- VoiceCache bookkeeping with stub entries,
and the joint-position chunk walk of the serving loop against a plain restatement of the reference's chunked decode of
cat(ref, codes), down to the samples a row hands out from every feed (feed_span)."""
import numpy as np
import pytest
import torch

from qwen_tts.voice import VoiceCache, VoiceEntry, boundary_skip, feed_span, joint_walk, plan_feed

UP, TAIL, RC, RX = 1920, 555, 300, 25


class _Decoder:
    def __init__(self, sig=("dec", "torch.float32", 8, 16, 64, 72)):
        self.sig = sig

    def signature(self):
        return self.sig


def _entry(n, tag="x"):
    return VoiceEntry(R=7, nz=7, snapshot=tag, ref=None, nbytes=n)


def _stats(c):
    s = c.stats
    return s["hits"], s["misses"], s["stores"], s["evictions"], s["entries"], s["bytes"]


def test_lru_by_bytes_and_counts():
    c = VoiceCache(max_bytes=100)
    assert c.stats == dict(hits=0, misses=0, stores=0, evictions=0, entries=0, bytes=0)
    a, b, d = VoiceCache.key([[1] * 16]), VoiceCache.key([[2] * 16]), VoiceCache.key([[3] * 16] * 2)
    assert c.lookup(a) is None
    assert c.store(a, _entry(40, "A")) and c.store(b, _entry(40, "B"))
    assert _stats(c) == (0, 1, 2, 0, 2, 80)
    assert c.lookup(a).snapshot == "A"        # a is now the most recently used: b goes first
    assert c.store(d, _entry(50, "D"))
    assert c.keys() == [a, d] and c.lookup(b) is None
    assert _stats(c) == (1, 2, 3, 1, 2, 90)
    assert c.store(b, _entry(100, "B2"))      # needs the whole cache: both others go
    assert c.keys() == [b] and _stats(c) == (1, 2, 4, 3, 1, 100)
    assert not c.store(b, _entry(10, "B3"))   # a key that is present keeps its entry
    assert c.lookup(b).snapshot == "B2" and c.stats["stores"] == 4
    c.clear()
    assert c.keys() == [] and c.lookup(b) is None and _stats(c) == (2, 3, 4, 3, 0, 0)


def test_max_bytes_zero_never_stores():
    c = VoiceCache(max_bytes=0)
    k = VoiceCache.key([[5] * 16])
    assert not c.fits(1) and not c.store(k, _entry(1))
    assert c.lookup(k) is None and c.lookup(k) is None
    assert _stats(c) == (0, 2, 0, 0, 0, 0)
    big = VoiceCache(max_bytes=64)
    assert big.store(k, _entry(64)) and not big.store(VoiceCache.key([[6] * 16]), _entry(65))
    assert big.keys() == [k] and _stats(big) == (0, 0, 1, 0, 1, 64)  # and the refused one evicted nothing


def test_key_equality_on_codes():
    g = np.random.default_rng(3)
    codes = g.integers(0, 2048, (7, 16))
    k = VoiceCache.key(codes.tolist())
    assert k[0] == 7 and k[1] == 16
    assert VoiceCache.key(codes) == k                                     # int64 array
    assert VoiceCache.key(codes.astype(np.int32)) == k
    assert VoiceCache.key(torch.tensor(codes, dtype=torch.long)) == k     # the wrapper's ref_code tensors
    assert VoiceCache.key(torch.tensor(codes, dtype=torch.int32)) == k
    other = codes.copy()
    other[6, 15] ^= 1
    assert VoiceCache.key(other) != k and VoiceCache.key(codes[:6]) != k
    assert VoiceCache.key(codes.reshape(14, 8)) != k                      # same bytes, other frame layout
    with pytest.raises(ValueError):
        VoiceCache.key(codes.reshape(-1))


def test_bind_refusal():
    c = VoiceCache()
    d = _Decoder()
    c.bind(d)
    c.bind(d)
    with pytest.raises(ValueError, match="another codec decoder"):
        c.bind(_Decoder())
    d.sig = d.sig[:-1] + (96,)
    with pytest.raises(ValueError, match="another codec decoder"):
        c.bind(d)


def _chunks(T):
    """The reference's chunked decode of T frames (K:885-895): [(start, end, context frames, first wav sample)]; a
    chunk contributes 1920 (end - start) - 555 samples."""
    out, start, w = [], 0, 0
    while start < T:
        end = min(start + RC, T)
        ctx = RX if start - RX > 0 else start
        out.append((start, end, ctx, w))
        w += UP * (end - start) - TAIL
        start = end
    return out, w


def _plain(R, F):
    """What serving a request of F generated frames behind R reference frames must do: the positions fed, the
    positions at which the row begins with their context lengths, and the samples dropped at the start and at each
    begin so that the output is wav[1920 R:] of the chunked decode of all R + F frames."""
    chunks, total = _chunks(R + F)
    fed, begins, drops = [], [], []
    for start, end, ctx, w in chunks:
        if end <= R:
            continue  # a chunk of reference frames alone: the voice entry's business
        if start < R:  # the chunk the boundary falls into: adopted after R - start frames
            fed += range(R, end)
            drops.append(("adopt", UP * R - (w + UP * (R - start) - TAIL)))
        else:
            fed += range(start - ctx, end)
            begins.append((start - ctx, ctx))
            drops.append(("begin", UP * ctx + max(UP * R - w, 0)))
    return fed, begins, drops, total - UP * R


@pytest.mark.parametrize("cut", [1, 8])
@pytest.mark.parametrize("R,F", [(0, 331), (7, 12), (290, 14), (300, 3), (301, 5), (310, 300)])
def test_joint_walk_matches_chunked_decode(R, F, cut):
    fed_x, begins_x, drops_x, out_len = _plain(R, F)
    adopt, skip = boundary_skip(R)
    assert adopt == bool(R % RC)
    fed, begins, drops = [], [], ([("adopt", skip)] if adopt else [])
    extra = 0 if adopt else skip
    valid = 0
    for lo in range(0, F, cut):
        todo, marks = joint_walk(R, lo, min(lo + cut, F))
        at = 0
        while at < len(todo):
            n, begin = plan_feed(todo, marks, at, 8)
            assert 1 <= n <= 8
            assert not any(at < m < at + n for m in marks)  # a restart opens a feed of its own
            if begin:
                begins.append((todo[at], marks[at]))
                drops.append(("begin", UP * marks[at] + extra))
                extra = 0
            fed += todo[at:at + n]
            valid += UP * n - (TAIL if begin else 0)
            at += n
    assert fed == fed_x
    assert begins == begins_x
    assert drops == drops_x
    assert valid - sum(d for _, d in drops) == out_len  # what is left is exactly wav[1920 R:]


def test_boundary_skip_values():
    assert boundary_skip(0) == (False, 0)
    assert boundary_skip(7) == (True, 555) and boundary_skip(299) == (True, 555)
    assert boundary_skip(300) == (False, 555) and boundary_skip(301) == (True, 1110)
    assert boundary_skip(600) == (False, 1110)


CH, CX = 5, 2  # a small geometry for the sample accounting: chunks of 5 frames, 2 frames of context


def _one_shot_labels(T):
    """The chunked decode of joint frames [0, T) at chunk CH / context CX, every sample labelled 1920 * (the frame it
    is decoded from) + its offset: chunk [start, end) decodes its context frames and its own, loses the last 555
    samples and drops the context's."""
    out = []
    for start in range(0, T, CH):
        end = min(start + CH, T)
        c = CX if start - CX > 0 else start
        frames = np.arange(start - c, end)
        q = np.arange(UP * c, UP * len(frames) - TAIL)
        out.append(frames[q // UP] * UP + q % UP)
    return np.concatenate(out) if out else np.zeros(0, np.int64)


class _FakeRow:
    """One row of the incremental decoder, as the serving loop sees it: after m frames since its begin it has produced
    1920 m - 555 samples of their decode, and a feed of n frames returns [1920 n] with what those frames added at its
    end -- so nothing in the first 555 of a feed that begins (-1 here)."""

    def __init__(self, fed=()):
        self.fed = list(fed)

    def feed(self, positions, begin):
        if begin:
            self.fed = []
        assert begin or self.fed, "a row that has no state must begin"
        q = UP * len(self.fed) - TAIL + np.arange(UP * len(positions))
        self.fed += positions
        return np.where(q >= 0, np.asarray(self.fed)[np.maximum(q, 0) // UP] * UP + q % UP, -1)


def _serve(R, F, caps, step, cb0):
    """One slot's walk through a request of F generated frames behind R reference ones, reported `step` frames at a
    time, as TTSModel._serve_codec runs it; returns (the chunks handed out, their last flags)."""
    adopt, skip = boundary_skip(R, CH, TAIL)
    row = _FakeRow()
    if adopt:  # the voice entry's state: chunk R // CH of the reference, fed from its context up to frame R
        start = R // CH * CH
        row = _FakeRow(range(start - (CX if start - CX > 0 else start), R))
    discard, extra = (skip, 0) if adopt else (0, skip)
    cum, nz = UP * R, sum(cb0[:R])
    chunks, lasts = [], []
    for lo in range(0, F, step):
        f = min(lo + step, F)
        ended = f == F
        nz += sum(cb0[R + lo:R + f])
        todo, mk = joint_walk(R, lo, f, CH, CX)
        marks = {k: c * UP for k, c in mk.items()}
        at = 0
        while at < len(todo):
            n, begin = plan_feed(todo, marks, at, caps[-1])
            assert 1 <= n and any(c >= n for c in caps)
            pcm = row.feed(todo[at:at + n], begin)
            ctx_s = marks[at] if begin else 0
            at += n
            lo_s, hi_s, last, discard, extra, cum = feed_span(begin, n, ctx_s, ended, at == len(todo), nz, discard,
                                                              extra, cum, UP, TAIL)
            assert (TAIL if begin else 0) <= lo_s <= hi_s <= UP * n
            if hi_s > lo_s or last:
                chunks.append(pcm[lo_s:hi_s])
                lasts.append(last)
    return chunks, lasts


@pytest.mark.parametrize("F", [1, 4, 11])
@pytest.mark.parametrize("R", [0, 3, 5, 7])
def test_feed_span_hands_out_the_one_shot_samples(R, F):
    """joint_walk + plan_feed + boundary_skip + feed_span against a decoder that labels its samples: whatever the
    feed capacities and the reports' sizes, a request gets wav[1920 R : 1920 nz] of the chunked decode of its R + F
    joint frames, in order, and exactly one last, on its final chunk.

    The length rule 1920 x #nonzero-cb0 is known with the request's last report only, and what a stream has handed
    out stays handed out: where zero cb0 make 1920 nz fall below the samples that existed before the last report
    (all of the decode of the T' joint frames known until then, 1920 T' - 555 ceil(T' / chunk)), the audio ends
    there instead.  With every cb0 nonzero, and with the request in one report, that is the rule itself."""
    T = R + F
    wav = _one_shot_labels(T)
    whole = UP * T - TAIL * -(-T // CH)
    assert len(wav) == whole
    for zeros in ((), {0, T - 1}):  # every cb0 nonzero; two zero ones (one, where there is one frame)
        cb0 = [int(j not in zeros) for j in range(T)]
        nz = sum(cb0)
        for caps in ((1, 8), (2, 3)):
            for step in (1, 3, F):
                before = R + (F - 1) // step * step  # joint frames known before the last report
                end = max(UP * nz, UP * before - TAIL * -(-before // CH))
                want = wav[:end][UP * R:]
                if not zeros or step == F:
                    assert len(want) == max(0, min(whole, UP * nz) - UP * R)
                chunks, lasts = _serve(R, F, caps, step, cb0)
                assert lasts.count(True) == 1 and lasts[-1] is True, (caps, step, lasts)
                got = np.concatenate(chunks)
                assert got.shape == want.shape and (got == want).all(), (caps, step, len(zeros))


def test_feed_span_plain_request_is_the_no_reference_case():
    """R = 0 without a voice cache: no adoption, nothing extra, and the first feed drops its 555 alone"""
    assert boundary_skip(0, CH, TAIL) == (False, 0)
    assert feed_span(1, 1, 0, False, True, 1, 0, 0, 0, UP) == (TAIL, UP, False, 0, 0, UP - TAIL)
    assert feed_span(0, 2, 0, True, True, 3, 0, 0, UP - TAIL, UP) == (0, 2 * UP, True, 0, 0, 3 * UP - TAIL)
    assert feed_span(0, 2, 0, True, False, 2, 0, 0, UP - TAIL, UP) == (0, UP + TAIL, False, 0, 0, 2 * UP)
