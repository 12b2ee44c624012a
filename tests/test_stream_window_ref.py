"""CPU: the per-row stream kernels' restatement (tests/stream_window_ref.py) and the scheme built on it.

The toy stack has every stage kind of the codec's decoder (causal conv, transposed conv trimmed on both sides,
dilated residual units with biases, a last conv).  Its per-row incremental decode -- fixed shapes, ragged nrow, filler
rows of noise, idle feeds, a begin over a polluted state -- must reproduce the one-shot decode of each request alone.
Both sides are fp64 and sum the same products, so the expected difference is 0 up to summation order: bound 1e-12."""
import pytest
import torch

import stream_window_ref as R

F64 = torch.float64


def test_window_semantics():
    g = torch.Generator().manual_seed(0)
    B, H, n, C = 4, 3, 4, 2
    hist, x = torch.randn(B, H, C, generator=g, dtype=F64), torch.randn(B, n, C, generator=g, dtype=F64)
    xin, new = R.stream_window(hist, x, [0, 1, 2, 1], [0, 0, 0, 1], 2, 3)
    assert torch.equal(new[0], hist[0])                       # idle row: the history stays
    assert torch.equal(xin[0], torch.cat([hist[0], x[0]]))
    assert torch.equal(new[1], torch.cat([hist[1, 2:], x[1, :2]]))  # m = 2 < H: old and new rows
    assert torch.equal(new[2], x[2, 1:4])                     # m = 4 > H: the last H consumed rows
    assert torch.equal(xin[3, :H + 3], torch.zeros(H + 3, C, dtype=F64))  # begin: zero history, zero head
    assert torch.equal(xin[3, H + 3:], x[3, 3:])
    assert torch.equal(new[3], xin[3, 2:5])
    # filler rows (j >= m) are copied but never enter the history
    x2 = x.clone()
    x2[1, 2:] = 99.0
    assert torch.equal(R.stream_window(hist, x2, [0, 1, 2, 1], [0, 0, 0, 1], 2, 3)[1][1], new[1])


def test_rows_semantics():
    nf = torch.tensor([5, 9, 0, 7], dtype=torch.int32)
    pos, row_len, new = R.stream_rows(nf, [2, 0, 3, 1], [0, 0, 0, 1], 3)
    assert pos.tolist() == [[5, 6, 7], [9, 10, 11], [0, 1, 2], [0, 1, 2]]
    assert torch.equal(row_len, pos + 1)
    assert new.tolist() == [7, 9, 3, 1]


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_toy_stack_rowwise_incremental_equals_one_shot(seed):
    g = torch.Generator().manual_seed(100 + seed)
    st = R.ToyStack(seed)
    assert st.up == 12 and st.heads == [0, 2, 9]
    B, n, c_in = 3, 4, 3
    rs = R.ToyRowStream(st, B, pollute=g)
    # each batch row serves two requests in turn; the second begins over the first one's state
    lens = [[int(torch.randint(1, 14, (1,), generator=g)) for _ in range(2)] for _ in range(B)]
    reqs = [[torch.randn(L, c_in, generator=g, dtype=F64) for L in row] for row in lens]
    cur, fed = [0] * B, [0] * B
    delay = [0, 2, 1]  # feeds a row idles before its first begin (its polluted state is then still there)
    got = [[[] for _ in range(2)] for _ in range(B)]
    feeds = 0
    while any(cur[b] < 2 for b in range(B)):
        x = torch.randn(B, n, c_in, generator=g, dtype=F64) * 3  # filler: noise, not zeros
        nrow, begin = [0] * B, [0] * B
        for b in range(B):
            if cur[b] >= 2 or feeds < delay[b]:
                continue
            left = lens[b][cur[b]] - fed[b]
            nrow[b] = min(left, int(torch.randint(0, n + 1, (1,), generator=g)))  # ragged, 0 included
            begin[b] = int(fed[b] == 0 and nrow[b] > 0)
            x[b, :nrow[b]] = reqs[b][cur[b]][fed[b]:fed[b] + nrow[b]]
        out = rs.feed(x, nrow, begin)
        assert out.shape == (B, st.up * n)
        for b in range(B):
            if nrow[b]:
                got[b][cur[b]].append(out[b, st.look if begin[b] else 0:st.up * nrow[b]])
                fed[b] += nrow[b]
                if fed[b] == lens[b][cur[b]]:
                    cur[b], fed[b] = cur[b] + 1, 0
        feeds += 1
    worst = 0.0
    for b in range(B):
        for k in range(2):
            ref = st.forward(reqs[b][k][None])[0]
            assert ref.shape[0] == max(st.up * lens[b][k] - st.look, 0)
            inc = torch.cat(got[b][k])[:ref.shape[0]]
            assert inc.shape == ref.shape
            if ref.numel():
                worst = max(worst, float((inc - ref).abs().max()))
    print(f"toy stack, seed {seed}: {feeds} feeds, max |incremental - one-shot| = {worst:.3g}")
    assert worst <= 1e-12
