"""codec.RowCodecStream (the incremental codec decode with a clock per batch row) against CodecDecoder.forward of each
request alone, on a fixed script of feeds in which the three batch rows begin, idle, end and are refilled
independently, with ragged frame counts and random filler frames.  Bounds are those of
test_codec_stream_matches_forward (fp32 atol 2e-5, bf16 rel-L2 < 2e-2): the per-row stream runs the same per-row
math as CodecStream, so a miss here that CodecStream does not show is a leaking spurious or filler row."""
import pytest
import torch

pytestmark = pytest.mark.gpu

B, N = 3, 8
# frames each row consumes in each of the 14 feeds (capacity 8), and the feeds in which it begins a request
NROW = [[8, 8, 3, 8, 1, 8, 0, 8, 8, 8, 8, 8, 8, 8],    # one request of 92 frames: past the 72-frame attention window
        [0, 0, 8, 1, 3, 8, 0, 8, 8, 3, 0, 0, 0, 0],    # idles for two feeds, then a request of 39
        [8, 3, 1, 0, 8, 8, 3, 1, 8, 0, 3, 0, 0, 0]]    # 12 frames, idle, then a refill: 31 frames of other codes
BEGIN = [[0], [2], [0, 4]]


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _requests():
    """[(row, first feed, frames)] of the script"""
    out = []
    for b in range(B):
        for k, f0 in enumerate(BEGIN[b]):
            f1 = BEGIN[b][k + 1] if k + 1 < len(BEGIN[b]) else len(NROW[b])
            out.append((b, f0, sum(NROW[b][f0:f1])))
    return out


def _close(got, exp, dtype, what):
    assert got.shape == exp.shape, (what, got.shape, exp.shape)
    if dtype == "fp32":
        print(f"{what}: max |diff| {float((got - exp).abs().max()):.3g}")
        torch.testing.assert_close(got, exp, atol=2e-5, rtol=0)
    else:
        rel = float((got - exp).norm() / exp.norm())
        print(f"{what}: rel-L2 {rel:.3g}")
        assert rel < 2e-2, (what, rel)


@pytest.mark.parametrize("preset,dtype", [("tiny-customvoice", "fp32"), ("1.7b-customvoice", "fp32"),
                                          ("1.7b-customvoice", "bf16")])
def test_row_codec_stream_matches_forward(preset, dtype):
    from oracle import codec_param_specs, load_preset, synth_state_dict
    from qwen_tts.codec import CodecDecoder
    dev = _dev()
    _, ccfg = load_preset(preset)
    W = {k: torch.from_numpy(v) for k, v in synth_state_dict(codec_param_specs(ccfg)).items()}
    dec = CodecDecoder(ccfg, W, dtype=dtype, device=str(dev))
    cb, Q, up = dec.tables.shape[1], dec.tables.shape[0], dec.total_upsample
    g = torch.Generator().manual_seed(11)
    reqs = _requests()
    assert [r[2] for r in reqs] == [92, 39, 12, 31]
    codes = [torch.randint(1, cb, (F, Q), generator=g).to(dev, torch.int32) for _, _, F in reqs]
    refs = [dec.forward(c[None])[0] for c in codes]  # computed once, shared by the three runs and the last case
    for c, r in zip(codes, refs):
        assert r.shape[0] == up * c.shape[0] - 555
    filler = torch.randint(0, cb, (len(NROW[0]), B, N, Q), generator=g).to(dev, torch.int32)

    runs, slot = [], None
    for rep in range(3):  # on the pooled slot: the first run feeds eagerly and captures, the others replay
        rs = dec.row_stream(B, 96, N)
        assert slot is None or rs.slot is slot
        slot = rs.slot
        got = [[] for _ in reqs]
        cur, fed = [None] * B, [0] * B
        for f in range(len(NROW[0])):
            cc = filler[f].clone()  # filler frames are random codes, not zeros
            nrow, begin = [NROW[b][f] for b in range(B)], [int(f in BEGIN[b]) for b in range(B)]
            for b in range(B):
                if begin[b]:
                    cur[b], fed[b] = next(i for i, r in enumerate(reqs) if r[0] == b and r[1] == f), 0
                if nrow[b]:
                    cc[b, :nrow[b]] = codes[cur[b]][fed[b]:fed[b] + nrow[b]]
            pcm = rs.feed(cc, nrow, begin)
            assert pcm.shape == (B, up * N)
            for b in range(B):
                if nrow[b]:
                    got[cur[b]].append(pcm[b, 555 if begin[b] else 0:up * nrow[b]].clone())
                    fed[b] += nrow[b]
        for i, (b, f0, F) in enumerate(reqs):
            _close(torch.cat(got[i]), refs[i], dtype, f"run {rep}, row {b}, request of {F} frames")
        runs.append([torch.cat(x) for x in got])
        with pytest.raises(ValueError):  # row 0 sits at 92 of 96 frames
            rs.feed(filler[0], [8, 0, 0], [0, 0, 0])
        rs.close()
    assert len(slot.graphs) == 1 and list(slot.graphs) == [N]  # one graph for every mix of row states
    for a, b_ in zip(runs[1], runs[2]):
        assert torch.equal(a, b_)  # a replay equals the replay before it, bit for bit

    # a row that reaches exactly max_frames while its feed's filler rows write K/V past it
    rs = dec.row_stream(B, 12, N)
    try:
        c12, c39 = codes[2], codes[1]
        cc = filler[1].clone()
        cc[0, :8], cc[1, :3] = c12[:8], c39[:3]
        p0 = rs.feed(cc, [8, 3, 0], [1, 1, 0])
        out0, out1 = [p0[0, 555:up * 8].clone()], [p0[1, 555:up * 3].clone()]
        cc = filler[2].clone()
        cc[0, :4], cc[1, :8], cc[2, :1] = c12[8:], c39[3:11], codes[3][:1]
        p1 = rs.feed(cc, [4, 8, 1], [0, 0, 1])
        out0.append(p1[0, :up * 4].clone())
        out1.append(p1[1, :up * 8].clone())
        assert rs.nf == [12, 11, 1]
        _close(torch.cat(out0), refs[2], dtype, "row at max_frames")
        _close(torch.cat(out1), dec.forward(c39[None, :11])[0], dtype, "its neighbour")
        with pytest.raises(ValueError):
            rs.feed(cc, [1, 0, 0], [0, 0, 0])
    finally:
        rs.close()
