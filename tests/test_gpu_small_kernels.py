"""GPU units of the small memory-bound kernels (csrc/misc.hip) through qwen_tts.kernels, each against the plain
reference of tests/small_kernel_refs.py on seeded inputs, at the shapes where such kernels go wrong: below / at /
off the thread stride, ragged last waves, more than one block per row, non-default leading dimensions, the pad and
causal edges, the 65,536-block grid cap.

* Pure moves (gather_rows, advance, clamp_pcm) and the two ordered-fp32 sums (frame_embed, rvq_gather): bit-exact.
* fp32 arithmetic (rmsnorm, snake, dwconv_ln): every element within max(2 x the error of plain torch fp32 against
  fp64 on the same input, 4 fp32 ulp of the magnitude) -- small_kernel_refs.fp32_tolerance; the factor 2 allows for
  the device sinf / rsqrtf and another summation tree.
* bf16 outputs (snake, dwconv_ln): within one bf16 step of the fp64 result rounded to bf16 everywhere and equal on
  >= 99.9 % of the elements (tests/test_small_kernel_refs.py shows plain fp32 compute meets that on these inputs).
* Every output buffer and every padding column starts at a sentinel (7.0), which must survive wherever the kernel
  has no business writing.

measured on the MI355X (kernel vs fp64 / torch-fp32 vs fp64, worst case over the shapes, scaled as
small_kernel_refs.py describes):
  rmsnorm (and _rec)  9.6e-8 .. 1.8e-7 / 9.6e-8 .. 1.5e-7 of |ref|, per row (worst kernel / torch ratio 1.25)
  snake fp32          1.3e-7 .. 1.5e-7 / 1.3e-7 .. 1.5e-7 of |x| + inv_beta (worst ratio 1.07)
  dwconv_ln fp32      2.9e-8 .. 1.9e-7 / 6.8e-8 .. 2.3e-7 of the row's largest |ref| (worst ratio 0.98)
  bf16 cap            snake >= 99.9937 % equal (grid-cap case, 134 M elements: 99.9905 %), dwconv_ln >= 99.986 %;
                      never more than one step (plain fp32 on CPU: 99.9937 % / 99.993 %)
"""
import pytest
import torch

import small_kernel_refs as R

pytestmark = pytest.mark.gpu

F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16
S = R.SENTINEL


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _kn():
    from qwen_tts import kernels
    return kernels


def _sent(shape, dtype, dev):
    return torch.full(shape, S, dtype=dtype, device=dev)


def _is_sent(t):
    return bool((t == S).all())


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == F32 else torch.int16)


def _same_bits(a, b):
    return a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


def _fp32_ok(what, got, plain32, ref64, scale, per_row=False):
    ok, ek, et = R.judge_fp32(got, plain32, ref64, scale, per_row)
    print(f"{what}: kernel vs fp64 {ek:.3g}, torch-fp32 vs fp64 {et:.3g}")
    assert ok, (what, ek, et)


# ------------------------------------------------------------------------------------------ rmsnorm / rmsnorm_rec
@pytest.mark.parametrize("M,N", R.RMSNORM_SHAPES)
def test_rmsnorm(M, N):
    Kn, dev = _kn(), _dev()
    x, g = R.rmsnorm_inputs(M, N)
    out = _sent((M + 1, N), F32, dev)
    Kn.rmsnorm(x.to(dev), g.to(dev), R.RMSNORM_EPS, out, M, N)
    ref = R.rmsnorm(x, g, R.RMSNORM_EPS)
    _fp32_ok(f"rmsnorm {M}x{N}", out[:M].cpu(), R.rmsnorm(x, g, R.RMSNORM_EPS, F32), ref, ref.abs(), per_row=True)
    assert _is_sent(out[M:])


@pytest.mark.parametrize("step_stride", [1, 0])
@pytest.mark.parametrize("wide", [False, True])
@pytest.mark.parametrize("M,N", R.RMSNORM_SHAPES)
def test_rmsnorm_rec(M, N, wide, step_stride):
    """rec [M][F][N] (wide: a slice of a wider buffer, rec.stride(0) > F*N): the slot step[m * stride] + step_off of
    row m equals out bit for bit, everything else keeps its sentinel.  Per-row steps run through the F slots (all
    different for M <= F); step_stride 0 reads one shared counter."""
    Kn, dev = _kn(), _dev()
    Fr, off = 5, 1
    x, g = R.rmsnorm_inputs(M, N)
    out = _sent((M + 1, N), F32, dev)
    base = _sent((M, Fr * N + (7 if wide else 0)), F32, dev)
    rec = base[:, :Fr * N].unflatten(1, (Fr, N))
    assert (M == 1 or rec.stride(0) == base.stride(0)) and rec.data_ptr() == base.data_ptr()  # one row: no stride
    steps = [(m + 2) % Fr - off for m in range(M)] if step_stride else [2] + [0] * (M - 1)  # stride 0: only [0] is read
    slots = [(steps[m] if step_stride else steps[0]) + off for m in range(M)]
    step = torch.tensor(steps, dtype=torch.int32, device=dev)
    Kn.rmsnorm(x.to(dev), g.to(dev), R.RMSNORM_EPS, out, M, N, rec=rec, step=step, step_off=off, step_stride=step_stride)
    plain = _sent((M + 1, N), F32, dev)
    Kn.rmsnorm(x.to(dev), g.to(dev), R.RMSNORM_EPS, plain, M, N)
    assert _same_bits(out, plain) and _is_sent(out[M:])  # recording changes nothing in out
    want = _sent(tuple(base.shape), F32, dev)
    wrec = want[:, :Fr * N].unflatten(1, (Fr, N))
    for m in range(M):
        wrec[m, slots[m]] = out[m]
    assert _same_bits(base, want)
    ref = R.rmsnorm(x, g, R.RMSNORM_EPS)
    _fp32_ok(f"rmsnorm_rec {M}x{N}", out[:M].cpu(), R.rmsnorm(x, g, R.RMSNORM_EPS, F32), ref, ref.abs(), per_row=True)


# ------------------------------------------------------------------------------------------ gather_rows
@pytest.mark.parametrize("pad", [0, 5])
@pytest.mark.parametrize("M", [1, 37])
@pytest.mark.parametrize("H", [1, 7, 256, 2048])
@pytest.mark.parametrize("dtype", [F32, BF16])
def test_gather_rows(dtype, H, M, pad):
    Kn, dev = _kn(), _dev()
    V = 9
    g = torch.Generator().manual_seed(100 * H + M)
    tab = torch.randn(V, H, generator=g).to(dtype)
    idx = torch.randint(0, V, (M,), generator=g, dtype=torch.int32)
    idx[-1] = V - 1
    if M > 3:
        idx[0], idx[1], idx[2] = 0, 4, 4  # first row, a repeat, (above) the last row
    ldo = H + pad
    out = _sent((M + 1, ldo), F32, dev)
    Kn.gather_rows(tab.to(dev), idx.to(dev), M, H, out, ldo)
    assert _same_bits(out[:M, :H].cpu(), tab[idx.long()].float())
    assert _is_sent(out[:M, H:]) and _is_sent(out[M:])


# ------------------------------------------------------------------------------------------ frame_embed
T_BAD = R.FRAME_T_CODES - 1  # fills the counters a step_stride-0 launch must not read: a valid frame, another sum


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("G", [1, 16, 32])
@pytest.mark.parametrize("H", [8, 512, 520, 1024, 2048])  # grid.y 1, 1, 2, 2, 4; 520: a ragged last wave
@pytest.mark.parametrize("dtype", [F32, BF16])
def test_frame_embed(dtype, H, G, B):
    """x bit-exact against the ordered fp32 sum, x16 against its bf16 rounding.  Per-row frame indices straddle T
    (t = T-1: the row's trailing text, t = T and t > T: the pad row); step_stride 0 shares one counter."""
    Kn, dev = _kn(), _dev()
    T = R.FRAME_T
    e0, ecp, codes, ld, trailing, pad = R.frame_embed_inputs(H, G, B, dtype)
    tr = trailing[:B * T].view(B, T, H)
    d = [t.to(dev) for t in (e0, ecp, codes, trailing, pad)]
    straddle = [T - 1, T, T + 2]
    runs = [(1, straddle)] if B == 3 else [(1, [t]) for t in straddle]
    runs += [(0, [T - 1] * B), (0, [T] * B)]
    for stride, steps in runs:
        ref = R.frame_embed_ordered(e0, ecp, G, codes, ld, steps, tr, T, pad)
        step = torch.tensor(steps if stride else steps[:1] + [T_BAD] * (B - 1), dtype=torch.int32, device=dev)
        for with16 in (False, True):
            x = _sent((B + 1, H), F32, dev)
            x16 = _sent((B + 1, H), BF16, dev) if with16 else None
            Kn.frame_embed(d[0], d[1], G, H, d[2], ld, step, d[3], T, d[4], x, B, x16=x16, step_stride=stride)
            assert _same_bits(x[:B].cpu(), ref), (stride, steps, with16)
            assert _is_sent(x[B:])
            if with16:
                assert _same_bits(x16[:B].cpu(), ref.to(BF16)) and _is_sent(x16[B:])


@pytest.mark.parametrize("G,H", [(33, 512), (0, 512), (16, 12)])
def test_frame_embed_rejects(G, H):
    Kn, dev = _kn(), _dev()
    Hb = 512
    e0, ecp, codes, ld, trailing, pad = R.frame_embed_inputs(Hb, 33, 1, F32)  # valid buffers, large enough for any G here
    x = _sent((1, Hb), F32, dev)
    step = torch.zeros(1, dtype=torch.int32, device=dev)
    with pytest.raises(RuntimeError):
        Kn.frame_embed(e0.to(dev), ecp.to(dev), G, H, codes.to(dev), ld, step, trailing.to(dev), R.FRAME_T, pad.to(dev),
                       x, 1, step_stride=1)
    torch.cuda.synchronize()
    assert _is_sent(x)


# ------------------------------------------------------------------------------------------ advance
@pytest.mark.parametrize("n", [1, 5, 1024])
def test_advance(n):
    Kn, dev = _kn(), _dev()
    g = torch.Generator().manual_seed(n)
    c0 = torch.randint(-50, 50, (1030,), generator=g, dtype=torch.int32)
    c = c0.clone().to(dev)
    Kn.advance(c, n)
    want = c0.clone()
    want[:n] += 1
    assert torch.equal(c.cpu(), want)


def test_advance_rejects():
    Kn, dev = _kn(), _dev()
    c = torch.zeros(1030, dtype=torch.int32, device=dev)
    with pytest.raises(RuntimeError):
        Kn.advance(c, 1025)
    torch.cuda.synchronize()
    assert not c.any()


# ------------------------------------------------------------------------------------------ rvq_gather
@pytest.mark.parametrize("BT", [1, 45])
@pytest.mark.parametrize("cb", [320, 2048])
@pytest.mark.parametrize("dim", [7, 256, 300])
@pytest.mark.parametrize("Q,n_first", [(16, 1), (16, 0), (16, 16), (1, 1)])
def test_rvq_gather(Q, n_first, dim, cb, BT):
    Kn, dev = _kn(), _dev()
    tabs, codes = R.rvq_inputs(Q, cb, dim, BT)
    o1, o2 = _sent((BT + 1, dim), F32, dev), _sent((BT + 1, dim), F32, dev)
    B, T = (1, 1) if BT == 1 else (5, 9)
    Kn.rvq_gather(tabs.to(dev), Q, n_first, cb, dim, codes.to(dev), B, T, o1, o2)
    r1, r2 = R.rvq_gather_ordered(tabs, codes, n_first)
    assert _same_bits(o1[:BT].cpu(), r1) and _same_bits(o2[:BT].cpu(), r2)
    assert _is_sent(o1[BT:]) and _is_sent(o2[BT:])


# ------------------------------------------------------------------------------------------ snake
@pytest.mark.parametrize("C,rows", R.SNAKE_SHAPES)  # C = 24: c0 = (i*8) % C wraps inside a block
@pytest.mark.parametrize("dtype", [F32, BF16])
def test_snake(dtype, C, rows):
    Kn, dev = _kn(), _dev()
    x, al, ib = R.snake_inputs(C, rows, dtype)
    buf = _sent((rows + 1, C), dtype, dev)
    Kn.snake(x.to(dev), buf, rows, C, al.to(dev), ib.to(dev))
    inpl = _sent((rows + 1, C), dtype, dev)
    inpl[:rows] = x.to(dev)
    Kn.snake(inpl, inpl, rows, C, al.to(dev), ib.to(dev))
    assert _same_bits(buf, inpl) and _is_sent(buf[rows:])  # in place == out of place, nothing past the rows
    got, ref = buf[:rows].cpu(), R.snake(x, al, ib)
    if dtype == F32:
        _fp32_ok(f"snake C={C}", got, R.snake(x, al, ib, F32), ref, x.abs().double() + ib.double())
    else:
        worst, same = R.assert_bf16_cap(got, ref, f"snake C={C}")
        print(f"snake bf16 C={C}: worst {worst} step, equal {100 * same:.4f} %")


def test_snake_rejects():
    Kn, dev = _kn(), _dev()
    x, al, ib = R.snake_inputs(24, 10, F32)
    y = _sent((10, 24), F32, dev)
    with pytest.raises(RuntimeError):
        Kn.snake(x.to(dev), y, 20, 12, al.to(dev), ib.to(dev))
    torch.cuda.synchronize()
    assert _is_sent(y)


def test_snake_grid_cap():
    """bf16, C = 8, one row past 65,536 blocks x 256 threads: the grid-stride loop takes a second trip.  The whole
    tensor is judged (fp64 reference on the GPU in chunks), and the elements of the second trip on their own."""
    Kn, dev = _kn(), _dev()
    C, rows = R.SNAKE_GRID_CAP
    _, al, ib = R.snake_inputs(C, 1, BF16)
    al, ib = al.to(dev), ib.to(dev)
    step = 1000003  # rows of one seeded host block, tiled: its period divides neither the grid nor a power of two
    base = (2 * torch.randn(step, C, generator=torch.Generator().manual_seed(8))).to(BF16).to(dev)
    x = _sent((rows + 1, C), BF16, dev)
    for r0 in range(0, rows, step):
        n = min(step, rows - r0)
        x[r0:r0 + n] = base[:n]
    y = _sent((rows + 1, C), BF16, dev)
    Kn.snake(x, y, rows, C, al, ib)
    assert _is_sent(y[rows:])
    worst, differ = 0, 0
    for r0 in range(0, rows, step):
        n = min(step, rows - r0)
        d = R.bf16_ulp_diff(y[r0:r0 + n], R.to_bf16(R.snake(x[r0:r0 + n], al, ib)))
        worst, differ = max(worst, int(d.max())), differ + int((d != 0).sum())
    same = 1 - differ / (rows * C)
    print(f"snake grid cap: worst {worst} step, equal {100 * same:.4f} %")
    assert worst <= 1 and same >= 0.999
    tail = slice(65536 * 256, rows)  # the second trip's rows
    assert int(R.bf16_ulp_diff(y[tail], R.to_bf16(R.snake(x[tail], al, ib))).max()) <= 1
    assert not _same_bits(y[tail], x[tail])


# ------------------------------------------------------------------------------------------ dwconv_ln
@pytest.mark.parametrize("B,T", R.DWCONV_BT)
@pytest.mark.parametrize("C", R.DWCONV_CS)
@pytest.mark.parametrize("dtype", [F32, BF16])
def test_dwconv_ln(dtype, C, B, T):
    Kn, dev = _kn(), _dev()
    a = R.dwconv_inputs(B, T, C, dtype)
    out = _sent((B * T + 1, C), dtype, dev)
    d = [t.to(dev) for t in a]
    Kn.dwconv_ln(d[0], B, T, C, *d[1:], R.DWCONV_EPS, out)
    got = out[:B * T].view(B, T, C).cpu()
    ref = R.dwconv_ln(*a, R.DWCONV_EPS)
    assert _is_sent(out[B * T:])
    if dtype == F32:
        _fp32_ok(f"dwconv_ln C={C} B={B} T={T}", got, R.dwconv_ln(*a, R.DWCONV_EPS, F32), ref, R.row_scale(ref),
                 per_row=True)
    else:
        worst, same = R.assert_bf16_cap(got, ref, f"dwconv_ln C={C} B={B} T={T}")
        print(f"dwconv_ln bf16 C={C} B={B} T={T}: worst {worst} step, equal {100 * same:.4f} %")


def test_dwconv_ln_rejects():
    Kn, dev = _kn(), _dev()
    C = 8200
    x, w, bias, lw, lb = [t.to(dev) for t in R.dwconv_inputs(1, 1, C, F32)]
    out = _sent((1, C), F32, dev)
    with pytest.raises(RuntimeError):
        Kn.dwconv_ln(x, 1, 1, C, w, bias, lw, lb, R.DWCONV_EPS, out)
    torch.cuda.synchronize()
    assert _is_sent(out)


# ------------------------------------------------------------------------------------------ clamp_pcm
def _clamp_input(n, dtype):
    g = torch.Generator().manual_seed(n)
    x = 1.5 * torch.randn(n, generator=g)
    up, dn = (2.0 ** -23, 2.0 ** -24) if dtype == F32 else (2.0 ** -7, 2.0 ** -8)  # one step above / below 1
    edge = torch.tensor([1 + up, 1.0, -1.0, 1 - dn, -1 - up, -1 + dn, float("inf"), float("-inf"), -0.0],
                        dtype=F64).float()
    k = min(n, len(edge))
    x[:k] = edge[:k]
    x = x.to(dtype)
    assert _same_bits(x[:k].float(), edge[:k])  # the edge values exist in dtype
    return x


@pytest.mark.parametrize("n", [1, 257, 4099])
@pytest.mark.parametrize("dtype", [F32, BF16])
def test_clamp_pcm(dtype, n):
    """fp32 in place (as the codec calls it), bf16 into a separate fp32 buffer; exact, the sign of -0.0 included."""
    Kn, dev = _kn(), _dev()
    x = _clamp_input(n, dtype)
    want = torch.clamp(x.float(), -1.0, 1.0)
    if dtype == F32:
        out = _sent((n + 5,), F32, dev)
        out[:n] = x.to(dev)
        Kn.clamp_pcm(out, n, out)
    else:
        out = _sent((n + 5,), F32, dev)
        Kn.clamp_pcm(x.to(dev), n, out)
    assert _same_bits(out[:n].cpu(), want) and _is_sent(out[n:])


def test_clamp_pcm_grid_cap():
    """fp32 in place, 257 elements past 65,536 blocks x 256 threads."""
    Kn, dev = _kn(), _dev()
    n = 65536 * 256 + 257
    per = 1000003  # one seeded host block, tiled
    base = (1.5 * torch.randn(per, generator=torch.Generator().manual_seed(9))).to(dev)
    x = _sent((n + 5,), F32, dev)
    for i0 in range(0, n, per):
        k = min(per, n - i0)
        x[i0:i0 + k] = base[:k]
    want = torch.clamp(x[:n], -1.0, 1.0)
    Kn.clamp_pcm(x, n, x)
    assert _same_bits(x[:n], want) and _is_sent(x[n:])
    assert float(want[65536 * 256:].abs().max()) == 1.0  # the second trip had something to clamp
