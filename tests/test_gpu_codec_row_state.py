"""qt_codec_row_state / qt_codec_feed_codes and RowCodecStream.export_row / adopt_rows, tiny decoder.

A row's state exported at clocks below and above the 72-position attention window (1, 5 and 80 frames) and adopted
into other rows of other streams: the re-exported block is the same bytes, the neighbours keep theirs, a row
continued on the same row index of a stream of the same shape gives the same PCM bit for bit, and one continued on
another row index of another shape agrees within the project's PCM bound (atol 2e-4 in fp32; bf16 rel-L2 2e-2, the
bound of test_row_codec_stream_matches_forward) -- with the exporting stream and with CodecDecoder.forward of the whole
request."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

UP, TAIL = 1920, 555
FRAMES = [1, 5, 80]      # frames on the three rows of X when they are exported
CONT = [1, 3, 8]         # the feeds X and the adopting streams continue with

_DEC = {}


def _dec(dtype):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    if dtype not in _DEC:
        from oracle import codec_param_specs, load_preset, synth_state_dict
        from qwen_tts.codec import CodecDecoder
        _, ccfg = load_preset("tiny-customvoice")
        W = {k: torch.from_numpy(v) for k, v in synth_state_dict(codec_param_specs(ccfg)).items()}
        _DEC[dtype] = (CodecDecoder(ccfg, W, dtype=dtype, device="cuda:0"), ccfg, W)
    return _DEC[dtype][0]


def _codes(dec, g, *shape):
    return torch.randint(1, dec.tables.shape[1], (*shape, dec.tables.shape[0]), generator=g).to(dec.dev, torch.int32)


def _busy(rs, g, nrow):
    """begin every row of a stream on random codes, so that its slot holds other state"""
    n = max(nrow)
    rs.feed(_codes(rs.dec, g, rs.B, n), nrow, [1] * rs.B)


def _close(got, exp, dtype, what):
    assert got.shape == exp.shape, (what, got.shape, exp.shape)
    if dtype == "fp32":
        print(f"{what}: max |diff| {float((got - exp).abs().max()):.3g}")
        torch.testing.assert_close(got, exp, atol=2e-4, rtol=0)
    else:
        rel = float((got - exp).norm() / exp.norm())
        print(f"{what}: rel-L2 {rel:.3g}")
        assert rel < 2e-2, (what, rel)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_export_adopt_round_trip(dtype):
    dec = _dec(dtype)
    g = torch.Generator().manual_seed(5)
    total = [f + sum(CONT) for f in FRAMES]
    seq = [_codes(dec, g, t) for t in total]          # each row's whole request
    X = dec.row_stream(3, 96, 8)
    streams = [X]
    try:
        # rows begin with 1, 5 and 8 frames; row 2 goes on to 80 while the others ride along
        cc = _codes(dec, g, 3, 8)
        for a in range(3):
            cc[a, :min(FRAMES[a], 8)] = seq[a][:min(FRAMES[a], 8)]
        X.feed(cc, [1, 5, 8], [1, 1, 1])
        for k in range(1, 10):
            cc = _codes(dec, g, 3, 8)
            cc[2] = seq[2][8 * k:8 * k + 8]
            X.feed(cc, [0, 0, 8], [0, 0, 0])
        assert X.nf == FRAMES
        snaps = [X.export_row(a) for a in range(3)]
        assert [s.p for s in snaps] == FRAMES and len({s.nbytes for s in snaps}) == 1
        assert X.slot.nf_dev.tolist() == FRAMES          # exporting leaves the row as it was

        # the same shape, the same row indices: all three rows adopt in one launch, then both streams continue
        Y1 = dec.row_stream(3, 96, 8)
        streams.append(Y1)
        assert Y1.slot is not X.slot
        _busy(Y1, g, [2, 7, 4])
        Y1.adopt_rows(list(enumerate(snaps)))
        assert Y1.nf == FRAMES and Y1.slot.nf_dev.tolist() == FRAMES and all(Y1.live)
        cont = [[] for _ in range(3)]
        at = list(FRAMES)
        for n in CONT:
            cc = torch.stack([seq[a][at[a]:at[a] + n] for a in range(3)])
            px = X.feed(cc, [n] * 3, [0] * 3).clone()
            py = Y1.feed(cc, [n] * 3, [0] * 3)
            assert torch.equal(px, py), f"{n}-frame feed after adoption differs from the exporting stream's"
            for a in range(3):
                cont[a].append(px[a, :UP * n])
                at[a] += n
        cont = [torch.cat(c) for c in cont]
        for a in range(3):  # and both are the one-shot decode of the whole request (a continuing row's sample j of
            # the feed behind p frames is sample 1920 p - 555 + j of it)
            ref = dec.forward(seq[a][None])[0]
            lo = UP * FRAMES[a] - TAIL
            _close(cont[a][:ref.shape[0] - lo], ref[lo:], dtype, f"row {a} continued vs forward")

        # another B, capacity and n_max, another row index
        for a in range(3):
            Y = dec.row_stream(4, 120, 4)
            streams.append(Y)
            _busy(Y, g, [3, 2, 4, 1])
            before = Y.export_row(0)
            Y.adopt_row(2, snaps[a])
            again = Y.export_row(2)
            assert again.p == FRAMES[a] and torch.equal(again.block, snaps[a].block), f"row {a}: re-export differs"
            assert torch.equal(Y.export_row(0).block, before.block), "adoption touched a neighbour row"
            assert Y.slot.nf_dev.tolist() == [3, 2, FRAMES[a], 1] and Y.nf == [3, 2, FRAMES[a], 1]
            got, p = [], FRAMES[a]
            for n in (1, 3, 4, 4):
                cc = _codes(dec, g, 4, 4)[:, :n].contiguous()
                cc[2] = seq[a][p:p + n]
                got.append(Y.feed(cc, [0, 0, n, 0], [0] * 4)[2, :UP * n].clone())
                p += n
            _close(torch.cat(got), cont[a], dtype, f"row {a} adopted into row 2 of 4")
            Y.close()
        Z = dec.row_stream(2, 96, 8)  # B = 2: a fresh slot whose histories do not exist yet
        streams.append(Z)
        Z.adopt_row(1, snaps[2])
        assert torch.equal(Z.export_row(1).block, snaps[2].block) and Z.slot.nf_dev.tolist() == [0, 80]
    finally:
        for s in streams:
            s.close()
    assert not any(sl.busy for pool in dec._row_slots.values() for sl in pool)


def test_argument_checks_launch_nothing():
    from qwen_tts import _hip
    from qwen_tts.codec import CodecDecoder
    dec = _dec("fp32")
    g = torch.Generator().manual_seed(6)
    rs = dec.row_stream(3, 96, 8)
    try:
        _busy(rs, g, [2, 5, 8])
        snap = rs.export_row(1)
        tab = rs._state_table()
        state = [rs.export_row(b).block.clone() for b in range(3)]
        guard = torch.full((tab.block_bytes + 32,), 0xA5, dtype=torch.uint8, device=dec.dev)
        L = _hip.lib()

        def call(block_ptr, row, p, d):
            job = (_hip.CodecRowJob * 1)(_hip.CodecRowJob(block_ptr, row, p, d, 0))
            return L.qt_codec_row_state(ctypes.byref(tab.args), job, 1, _hip.stream())
        ok = guard.data_ptr() + 16
        assert ok % 16 == 0
        for d in (_hip.CODEC_ROW_ADOPT, _hip.CODEC_ROW_EXPORT):
            assert call(ok, 3, 5, d) == -2 and call(ok, -1, 5, d) == -2          # a row outside [0, B): QT_ERR_SHAPE
            assert call(ok, 1, tab.args.Lm + 1, d) == -2 and call(ok, 1, -1, d) == -2   # p outside [0, Lm]
            assert call(ok + 4, 1, 5, d) == -1 and call(None, 1, 5, d) == -1      # misaligned / null block: QT_ERR_ARG
        assert call(ok, 1, 5, 2) == -1                                           # another direction
        two = (_hip.CodecRowJob * 2)(_hip.CodecRowJob(ok, 1, 5, 0, 0), _hip.CodecRowJob(snap.block.data_ptr(), 1, 5, 0, 0))
        assert L.qt_codec_row_state(ctypes.byref(tab.args), two, 2, _hip.stream()) == -1   # two jobs adopt into one row
        assert L.qt_codec_row_state(ctypes.byref(tab.args), two, 65, _hip.stream()) == -2  # too many jobs
        assert L.qt_codec_row_state(None, two, 1, _hip.stream()) == -1
        assert L.qt_codec_row_state(ctypes.byref(tab.args), None, 0, _hip.stream()) == 0   # no jobs: nothing to do
        torch.cuda.synchronize()
        assert bool((guard == 0xA5).all()), "a refused call wrote to its block"
        for b in range(3):
            assert torch.equal(rs.export_row(b).block, state[b]), "a refused call wrote to the stream"
        # an accepted export writes its block and nothing around it (positions past the clock are not written: the
        # block is zeroed first, as export_row's is)
        guard[16:16 + tab.block_bytes] = 0
        assert call(ok, 1, rs.nf[1], _hip.CODEC_ROW_EXPORT) == 0
        torch.cuda.synchronize()
        assert torch.equal(guard[16:16 + tab.block_bytes], snap.block)
        assert bool((guard[:16] == 0xA5).all()) and bool((guard[16 + tab.block_bytes:] == 0xA5).all())

        # a snapshot of another decoder (same weights, another object) is refused before anything is launched
        _, ccfg, W = _DEC["fp32"]
        other = CodecDecoder(ccfg, W, dtype="fp32", device="cuda:0")
        rs2 = other.row_stream(3, 96, 8)
        try:
            with pytest.raises(ValueError, match="another decoder"):
                rs2.adopt_row(1, snap)
            assert not rs2.live[1]
        finally:
            rs2.close()
        with pytest.raises(ValueError):
            rs.export_row(3)
        short = dec.row_stream(1, 4, 4)  # 5 frames do not fit a stream of 4 per row
        try:
            with pytest.raises(ValueError, match="does not fit"):
                short.adopt_row(0, snap)
        finally:
            short.close()
    finally:
        rs.close()


def test_feed_codes_matches_indexing():
    from qwen_tts import kernels as K
    dec = _dec("fp32")
    dev = dec.dev
    g = torch.Generator().manual_seed(7)
    B, n, F, Q = 4, 8, 12, 16
    codes = torch.randint(0, 2048, (B, F, Q), generator=g, dtype=torch.int32)
    R = [0, 4, 7, 0]
    refs = [None, torch.randint(0, 2048, (4, Q), generator=g, dtype=torch.int32),
            torch.randint(0, 2048, (7, Q), generator=g, dtype=torch.int32), None]
    refs_dev = [None if r is None else r.to(dev) for r in refs]
    # windows that straddle the boundary, with fillers; row 0 has a null reference whatever its length entry says
    pos = torch.tensor([[0, 1, 2, -1, 5, 11, -1, -1],
                        [2, 3, 4, 5, -1, 0, 15, -1],
                        [-1, 5, 6, 7, 8, 9, 18, 0],
                        [11, 10, -1, 0, 1, 2, 3, 4]], dtype=torch.int32)
    ref_ptr = torch.tensor([0 if r is None else r.data_ptr() for r in refs_dev], dtype=torch.int64, device=dev)
    ref_len = torch.tensor([5, 4, 7, 0], dtype=torch.int32, device=dev)
    out = torch.full((B, n, Q), -7, dtype=torch.int32, device=dev)
    K.codec_feed_codes(pos.to(dev), ref_ptr, ref_len, codes.to(dev), out)
    exp = torch.zeros(B, n, Q, dtype=torch.int32)
    for b in range(B):
        joint = codes[b] if refs[b] is None else torch.cat([refs[b], codes[b]])
        assert joint.shape[0] == R[b] + F
        for j in range(n):
            if pos[b, j] >= 0:
                exp[b, j] = joint[pos[b, j]]
    assert torch.equal(out.cpu(), exp)
    L = K._hip.lib()
    assert L.qt_codec_feed_codes(None, ref_ptr.data_ptr(), ref_len.data_ptr(), codes.to(dev).data_ptr(), B, n, F, Q,
                                 out.data_ptr(), K._hip.stream()) == -1
    assert L.qt_codec_feed_codes(pos.to(dev).data_ptr(), ref_ptr.data_ptr(), ref_len.data_ptr(),
                                 codes.to(dev).data_ptr(), B, 0, F, Q, out.data_ptr(), K._hip.stream()) == -2
