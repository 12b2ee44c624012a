"""GPU unit of qt_row_state (csrc/row_state.hip) through the C ABI, against torch indexing.  The kernel only moves
data, so every result is compared bit for bit.

The live side is one uint8 arena holding nine regions with 64 guard bytes in front of, between and behind them; the
stash has 256 guard bytes on either side.  Regions: a 1-byte flag at stride 1 (`finished`), five 4-byte counters at
stride 4 (the field-major `ctr`), 37 bytes at stride 41 from an odd address (byte path), 4096 aligned bytes (vector
path, one block), and 512 bytes at stride 1024 starting half a row in (the odd rows of `cp_x`).  A 40000-byte region
in a test of its own takes three blocks per row, the last one partial."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

GUARD, SGUARD = 64, 256
# (bytes per row, stride, misalignment of the base)
SHAPES = [(1, 1, 0)] + [(4, 4, 0)] * 5 + [(37, 41, 3), (4096, 4096, 0), (512, 1024, 0)]
CASES = [(3, 0b000), (3, 0b010), (3, 0b101), (3, 0b111), (64, 1 << 63)]


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


class Arena:
    """The live buffer, its regions' offsets, the stash with its guards, and the kernels.RowState over both."""

    def __init__(self, B, dev, shapes=SHAPES, seed=0):
        from qwen_tts import kernels as Kn
        self.B, self.shapes = B, shapes
        self.offs, o = [], GUARD
        for nbytes, stride, mis in shapes:
            o = (o + 255) // 256 * 256 + mis
            self.offs.append(o)
            o += stride * (B - 1) + nbytes + GUARD
        g = torch.Generator().manual_seed(seed)
        self.live = torch.randint(0, 256, (o,), dtype=torch.uint8, generator=g).to(dev)
        self.soffs, so = [], 0
        for nbytes, _, _ in shapes:
            self.soffs.append(so)
            so += (nbytes + 15) // 16 * 16
        self.row_bytes = so
        self.sbuf = torch.full((2 * SGUARD + B * so,), 0xAB, dtype=torch.uint8, device=dev)
        stash = self.sbuf[SGUARD:SGUARD + B * so].view(B, so)
        self.rs = Kn.RowState([(self.live[off:], st, nb) for off, (nb, st, _) in zip(self.offs, shapes)], B, dev,
                              stash=stash)
        assert self.rs.row_bytes == so

    def rows(self, mask):
        return [b for b in range(self.B) if mask >> b & 1]

    def stash_after_save(self, live, before, mask):
        want = before.clone()
        v = want[SGUARD:SGUARD + self.B * self.row_bytes].view(self.B, self.row_bytes)
        for off, soff, (nb, st, _) in zip(self.offs, self.soffs, self.shapes):
            for b in self.rows(mask):
                v[b, soff:soff + nb] = live[off + b * st:off + b * st + nb]
        return want

    def live_after_restore(self, live, sbuf, mask):
        want = live.clone()
        v = sbuf[SGUARD:SGUARD + self.B * self.row_bytes].view(self.B, self.row_bytes)
        for off, soff, (nb, st, _) in zip(self.offs, self.soffs, self.shapes):
            for b in self.rows(mask):
                want[off + b * st:off + b * st + nb] = v[b, soff:soff + nb]
        return want


def _run(a, mask, direction):
    from qwen_tts import kernels as Kn
    Kn.row_state(a.rs, mask, direction)
    torch.cuda.synchronize()


@pytest.mark.parametrize("B,mask", CASES)
def test_save_fills_the_selected_rows_of_the_stash_and_nothing_else(B, mask):
    from qwen_tts import _hip
    a = Arena(B, _dev())
    live0, s0 = a.live.clone(), a.sbuf.clone()
    _run(a, mask, _hip.ROW_SAVE)
    assert torch.equal(a.live, live0)
    assert torch.equal(a.sbuf, a.stash_after_save(live0, s0, mask))
    if mask == 0:
        assert torch.equal(a.sbuf, s0)


@pytest.mark.parametrize("B,mask", CASES)
def test_save_scramble_restore_gives_back_the_selected_rows_only(B, mask):
    from qwen_tts import _hip
    dev = _dev()
    a = Arena(B, dev)
    live0 = a.live.clone()
    _run(a, mask, _hip.ROW_SAVE)
    s1 = a.sbuf.clone()
    g = torch.Generator().manual_seed(7)
    scr = torch.randint(0, 256, a.live.shape, dtype=torch.uint8, generator=g).to(dev)
    a.live.copy_(scr)
    _run(a, mask, _hip.ROW_RESTORE)
    assert torch.equal(a.sbuf, s1)
    want = a.live_after_restore(scr, s1, mask)
    assert torch.equal(a.live, want)
    for off, (nb, st, _) in zip(a.offs, a.shapes):  # the restored rows are the original ones, the others the scramble
        for b in range(B):
            src = live0 if mask >> b & 1 else scr
            assert torch.equal(a.live[off + b * st:off + b * st + nb], src[off + b * st:off + b * st + nb])


def test_a_region_of_several_blocks_with_a_partial_last_one():
    from qwen_tts import _hip
    dev = _dev()
    a = Arena(3, dev, shapes=[(40000, 40000 + 16, 0), (40003, 40003, 1)])
    live0, s0 = a.live.clone(), a.sbuf.clone()
    _run(a, 0b110, _hip.ROW_SAVE)
    s1 = a.stash_after_save(live0, s0, 0b110)
    assert torch.equal(a.sbuf, s1) and torch.equal(a.live, live0)
    a.live.fill_(0x5C)
    scr = a.live.clone()
    _run(a, 0b100, _hip.ROW_RESTORE)
    assert torch.equal(a.live, a.live_after_restore(scr, s1, 0b100))


def test_every_error_code_is_returned_and_nothing_is_written():
    from qwen_tts import _hip
    from qwen_tts import kernels as Kn
    dev = _dev()
    a = Arena(3, dev)
    live0, s0 = a.live.clone(), a.sbuf.clone()
    L = _hip.lib()

    def call(**over):
        args = _hip.RowStateArgs()
        ctypes.memmove(ctypes.byref(args), ctypes.byref(a.rs.args), ctypes.sizeof(args))
        args.mask, args.dir = 0b111, _hip.ROW_SAVE
        for k, v in over.items():
            if k.startswith("r0_"):
                setattr(args.regions[0], k[3:], v)
            elif k.startswith("r8_"):
                setattr(args.regions[8], k[3:], v)
            else:
                setattr(args, k, v)
        rc = L.qt_row_state(ctypes.byref(args), _hip.stream())
        torch.cuda.synchronize()
        return rc

    ARG, SHAPE = -1, -2
    assert _hip.ERRORS[ARG] == "bad argument" and _hip.ERRORS[SHAPE] == "bad shape"
    assert L.qt_row_state(None, _hip.stream()) == ARG
    assert call(r0_base=None) == ARG and call(r8_base=None) == ARG
    assert call(stash=None) == ARG
    assert call(stash=a.rs.args.stash + 8) == ARG          # the stash is not 16-byte aligned
    assert call(dir=2) == ARG
    assert call(r0_bytes=0) == SHAPE and call(r8_bytes=-16) == SHAPE
    assert call(r8_stride=256) == SHAPE                    # rows would overlap
    assert call(n_regions=17) == SHAPE and call(n_regions=0) == SHAPE
    assert call(B=0) == SHAPE and call(B=65) == SHAPE
    assert call(mask=0b1000) == SHAPE                      # row 3 of 3
    assert call(stash_row_bytes=a.row_bytes - 16) == SHAPE and call(stash_row_bytes=a.row_bytes + 8) == SHAPE
    assert call(mask=0, r0_base=None) == ARG               # the table is checked before the empty mask returns
    assert L.qt_row_state_row_bytes(None) == ARG
    assert torch.equal(a.live, live0) and torch.equal(a.sbuf, s0)
    assert call(mask=0) == 0
    assert torch.equal(a.live, live0) and torch.equal(a.sbuf, s0)
    with pytest.raises(RuntimeError, match="bad shape"):   # the Python wrapper raises, it does not fall back
        Kn.row_state(a.rs, 0b1000, _hip.ROW_SAVE)
    with pytest.raises(RuntimeError, match="bad shape"):
        Kn.RowState([(a.live, 4, 4)] * 17, 3, dev)
    assert call() == 0                                     # and the unmodified call is a good one
    assert torch.equal(a.sbuf, a.stash_after_save(live0, s0, 0b111))
