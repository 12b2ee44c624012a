"""qt_trail_append through the C ABI: rows [n][H] scattered to trailing[row][pos] by a {row, pos} table,
bit-exact against a torch restatement.  H = 64 (one partial block per entry) and 2048 (two blocks per entry); n = 1
and 16; B = 1 and 3; tables mixing valid entries with row = -1, row = B and pos = T - 1 (written) and pos = T
(skipped).  `trailing` sits between guard rows inside one allocation, filled with a sentinel like every position no
entry names: all of that must come back untouched.  Shape and alignment errors return their code and launch
nothing."""
import pytest
import torch

pytestmark = pytest.mark.gpu

SENT = 7.0
GUARD = 2  # guard rows of H floats in front of and behind trailing


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _call(rows, slots, trailing_ptr, B, T, H, n):
    from qwen_tts import _hip
    return _hip.lib().qt_trail_append(rows.data_ptr(), slots.data_ptr(), trailing_ptr, B, T, H, n, _hip.stream())


def _table(kind, n, B, T):
    """n entries {row, pos}; distinct targets among the valid ones"""
    if kind == "valid":       # every entry lands, the last position of a row among them
        order = [T - 1] + list(range(T - 1))
        return [(j % B, order[j // B]) for j in range(n)]
    if kind == "mixed":       # valid entries between padding (row = -1), a row past the batch and a position past T
        pat = [(0, T - 1), (-1, 0), (B, 1), (B - 1, T), (B - 1, 1), (-1, -1), (0, 0), (B + 5, T + 5)]
        cells = [pat[j % len(pat)] if j < len(pat) else (-1, -1) for j in range(n)]
        return cells
    if kind == "pos_T":       # nothing lands
        return [(j % B, T) for j in range(n)]
    raise AssertionError(kind)


def _restate(rows, cells, trailing):
    out = trailing.clone()
    B, T, _ = out.shape
    for j, (r, p) in enumerate(cells):
        if 0 <= r < B and 0 <= p < T:
            out[r, p] = rows[j]
    return out


@pytest.mark.parametrize("kind", ["valid", "mixed", "pos_T"])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("n", [1, 16])
@pytest.mark.parametrize("H", [64, 2048])
def test_trail_append(H, n, B, kind):
    dev = _dev()
    T, n_use = 19, n
    g = torch.Generator().manual_seed(1000 * H + 100 * n + 10 * B + len(kind))
    rows = torch.randn(n_use, H, generator=g).to(dev)
    cells = _table(kind, n_use, B, T)
    slots = torch.tensor(cells, dtype=torch.int32).to(dev)
    buf = torch.full(((B * T + 2 * GUARD) * H,), SENT, dtype=torch.float32, device=dev)
    trailing = buf[GUARD * H:(GUARD + B * T) * H].view(B, T, H)
    before = trailing.clone()
    want = _restate(rows, cells, before)
    assert _call(rows, slots, trailing.data_ptr(), B, T, H, n_use) == 0
    torch.cuda.synchronize()
    assert torch.equal(trailing.view(torch.int32), want.view(torch.int32))     # bit-exact, untouched rows included
    assert bool((buf[:GUARD * H] == SENT).all()) and bool((buf[(GUARD + B * T) * H:] == SENT).all())
    named = {(r, p) for r, p in cells if 0 <= r < B and 0 <= p < T}
    if kind == "pos_T":
        assert not named and torch.equal(trailing, before)
    if kind == "mixed":
        assert (0, T - 1) in named                                              # pos = T - 1 is written
    for b in range(B):
        for t in range(T):
            if (b, t) not in named:
                assert bool((trailing[b, t] == SENT).all()), (b, t)


def test_trail_append_rejects_without_launching():
    dev = _dev()
    B, T, H = 2, 4, 64
    rows = torch.ones(4, H + 4, device=dev)
    slots = torch.tensor([[0, 0], [1, 1], [0, 2], [1, 3]], dtype=torch.int32, device=dev)
    trailing = torch.full((B, T, H + 4), SENT, device=dev)
    sh, arg = -2, -1  # QT_ERR_SHAPE, QT_ERR_ARG
    assert _call(rows, slots, trailing.data_ptr(), B, T, 62, 4) == sh           # H % 4 != 0
    assert _call(rows, slots, trailing.data_ptr(), B, T, H, 0) == sh
    assert _call(rows, slots, trailing.data_ptr(), 0, T, H, 4) == sh
    assert _call(rows, slots, trailing.data_ptr() + 4, B, T, H, 4) == arg       # trailing not 16-byte aligned
    assert _call(rows.view(-1)[1:], slots, trailing.data_ptr(), B, T, H, 4) == arg  # rows not 16-byte aligned
    assert _call(rows, slots, 0, B, T, H, 4) == arg                             # null pointer
    torch.cuda.synchronize()
    assert bool((trailing == SENT).all())
