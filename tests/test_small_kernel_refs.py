"""CPU checks of tests/small_kernel_refs.py: the references that tests/test_gpu_small_kernels.py and the kernel
units of tests/test_gpu_frontend.py judge the HIP kernels by.

* The two ordered-fp32 emulations are the right operation, not merely self-consistent: they agree with the same sum
  formed in fp64 to within n * 2^-24 of the summands' total magnitude (n = G adds for frame_embed, Q for
  rvq_gather: each fp32 add errs by at most 2^-24 of its partial sum, which never exceeds sum |x_i|).
* The bf16 cap (<= 1 bf16 step from the fp64 result rounded to bf16, equal on >= 99.9 %) is attainable: plain
  torch fp32 rounded to bf16 meets it on the very inputs the GPU tests use.
* The error of plain torch fp32 against fp64 on those inputs, which the GPU tests double for their bounds, is
  recorded (printed with -s) and sane (fp32 has not lost half its bits: < 2^-12 of the scale).

measured here (torch-fp32 vs fp64, scaled as small_kernel_refs.py describes):
  rmsnorm 9.6e-8 .. 1.5e-7, snake 1.3e-7 .. 1.5e-7, dwconv_ln 6.8e-8 .. 2.3e-7, layernorm 0 .. 2.1e-7
  (1.1e-5 on the mean-1e3 row), time_stats mean 0 .. 2.4e-7, std 5e-10 .. 1.2e-7, scale_add 5.3e-8 .. 8.0e-8.
  bf16 cap of plain fp32: snake >= 99.9937 % equal, dwconv_ln >= 99.993 %, layernorm and scale_add 100 %; never
  more than one step.
"""
import pytest
import torch

import small_kernel_refs as R

F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16
U = 2.0 ** -24


def test_judging_helpers():
    x = torch.tensor([1.0, 1.5, 0.99, 3.0, 1e3], dtype=F64)
    want = torch.tensor([2.0 ** -23, 2.0 ** -23, 2.0 ** -24, 2.0 ** -22, 2.0 ** -14], dtype=F64)
    assert torch.equal(R.ulp32(x), want)
    a = torch.tensor([1.0, 1.0, -0.0, 2.0 ** -126], dtype=BF16)
    b = torch.tensor([1.0 + 2.0 ** -7, 1.0 - 2.0 ** -8, 0.0, -(2.0 ** -126)], dtype=BF16)
    assert R.bf16_ulp_diff(a, b).tolist() == [1, 1, 0, 2 * 0x0080]
    # one rounding step from fp64: 1 + 2^-8 + 2^-40 lies above the tie, through fp32 it would land on the tie -> even
    t = torch.tensor([1 + 2.0 ** -8 + 2.0 ** -40, 1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -3.0], dtype=F64)
    assert R.to_bf16(t).double().tolist() == [1 + 2.0 ** -7, 1.0, 1 + 2.0 ** -6, -3.0]
    ref = torch.tensor([[1.0, -2.0]], dtype=F64)
    tol, e = R.fp32_tolerance(ref.float(), ref, ref.abs())
    assert float(e) == 0 and torch.equal(tol, 4 * R.ulp32(ref))  # the 4-ulp floor
    tol, e = R.fp32_tolerance((ref * (1 + 1e-5)).float(), ref, ref.abs())
    assert abs(float(e) - 1e-5) < 1e-7 and torch.allclose(tol, 2e-5 * ref.abs(), rtol=1e-2)


@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("G", [1, 16, 32])
def test_frame_embed_ordered_is_the_fp64_sum(G, dtype):
    H, B = 520, 3
    e0, ecp, codes, ld, trailing, pad = R.frame_embed_inputs(H, G, B, dtype)
    T = R.FRAME_T
    tr = trailing[:B * T].view(B, T, H)
    steps = [T - 1, T, T + 2]
    got = R.frame_embed_ordered(e0, ecp, G, codes, ld, steps, tr, T, pad)
    ref = R.frame_embed_f64(e0, ecp, G, codes, ld, steps, tr, T, pad)
    mag = R.frame_embed_f64(e0.float().abs().to(dtype), ecp.float().abs().to(dtype), G, codes, ld, steps, tr.abs(), T,
                            pad.abs())
    assert got.dtype == F32 and ((got.double() - ref).abs() <= G * U * mag).all()
    # the branch: row 0 (t = T-1) ends with its trailing row, rows 1 and 2 (t >= T) with pad
    base = R.frame_embed_ordered(e0, ecp, G, codes, ld, steps, torch.zeros_like(tr), T, torch.zeros_like(pad))
    assert torch.equal(got[0], base[0] + tr[0, T - 1]) and torch.equal(got[1], base[1] + pad)
    assert torch.equal(got[2], base[2] + pad)


@pytest.mark.parametrize("Q,n_first", [(16, 1), (16, 0), (16, 16), (1, 1)])
def test_rvq_gather_ordered_is_the_fp64_sum(Q, n_first):
    tabs, codes = R.rvq_inputs(Q, 320, 300, 45)
    o1, o2 = R.rvq_gather_ordered(tabs, codes, n_first)
    r1, r2 = R.rvq_gather_f64(tabs, codes, n_first)
    m1, m2 = R.rvq_gather_f64(tabs.abs(), codes, n_first)
    assert ((o1.double() - r1).abs() <= Q * U * m1).all() and ((o2.double() - r2).abs() <= Q * U * m2).all()
    assert codes.min() < 0 and codes.max() >= 320  # the planted codes are there and were clamped, not wrapped
    assert torch.equal(R.rvq_gather_ordered(tabs, codes.clamp(0, 319), n_first)[1], o2)
    if n_first == 0:
        assert not o1.any()
    if n_first == Q:
        assert not o2.any()


def test_dwconv_ln_reference_is_causal():
    """The fp64 reference against torch's own conv1d + layer_norm, and its causal edge: frame t sees t-6 .. t only."""
    import torch.nn.functional as Fn
    x, w, bias, lw, lb = R.dwconv_inputs(2, 9, 40, F32)
    ref = R.dwconv_ln(x, w, bias, lw, lb, R.DWCONV_EPS)
    y = Fn.conv1d(Fn.pad(x.double().transpose(1, 2), (6, 0)), w.double()[:, None, :], bias.double(), groups=40)
    want = Fn.layer_norm(y.transpose(1, 2), (40,), lw.double(), lb.double(), float(torch.tensor(R.DWCONV_EPS, dtype=F32)))
    torch.testing.assert_close(ref, want, atol=1e-12, rtol=1e-12)
    x2 = x.clone()
    x2[1, 5:] += 1.0  # later frames of batch 1 change nothing before them, and nothing in batch 0
    ref2 = R.dwconv_ln(x2, w, bias, lw, lb, R.DWCONV_EPS)
    assert torch.equal(ref2[0], ref[0]) and torch.equal(ref2[1, :5], ref[1, :5]) and not torch.equal(ref2[1, 5], ref[1, 5])


def _cap(plain32, ref64, what):
    worst, same = R.assert_bf16_cap(plain32.to(BF16), ref64, what)
    print(f"bf16 cap {what}: worst {worst} step, equal {100 * same:.4f} %")


@pytest.mark.parametrize("C,rows", R.SNAKE_SHAPES)
def test_bf16_cap_snake(C, rows):
    x, al, ib = R.snake_inputs(C, rows, BF16)
    _cap(R.snake(x, al, ib, F32), R.snake(x, al, ib), f"snake C={C}")


@pytest.mark.parametrize("B,T", R.DWCONV_BT)
@pytest.mark.parametrize("C", R.DWCONV_CS)
def test_bf16_cap_dwconv_ln(C, B, T):
    a = R.dwconv_inputs(B, T, C, BF16)
    _cap(R.dwconv_ln(*a, R.DWCONV_EPS, F32), R.dwconv_ln(*a, R.DWCONV_EPS), f"dwconv_ln C={C} B={B} T={T}")


@pytest.mark.parametrize("M,N", R.LAYERNORM_SHAPES)
def test_bf16_cap_layernorm(M, N):
    a = R.layernorm_inputs(M, N, False)
    _cap(R.layernorm(*a, R.LAYERNORM_EPS, F32), R.layernorm(*a, R.LAYERNORM_EPS), f"layernorm {M}x{N}")


@pytest.mark.parametrize("B,T,C", R.SCALE_ADD_SHAPES)
def test_bf16_cap_scale_add(B, T, C):
    a = R.scale_add_inputs(B, T, C, BF16)
    _cap(R.scale_add(*a, F32), R.scale_add(*a), f"scale_add {B}x{T}x{C}")


def _record(what, plain32, ref64, scale, per_row=False):
    tol, e = R.fp32_tolerance(plain32, ref64, scale, per_row)
    e = float(e.max())
    print(f"torch-fp32 vs fp64 {what}: {e:.3g}")
    assert e < 2.0 ** -12 and bool((tol >= 4 * R.ulp32(scale.double().expand_as(ref64))).all())
    return e


@pytest.mark.parametrize("M,N", R.RMSNORM_SHAPES)
def test_fp32_error_rmsnorm(M, N):
    x, g = R.rmsnorm_inputs(M, N)
    ref = R.rmsnorm(x, g, R.RMSNORM_EPS)
    _record(f"rmsnorm {M}x{N}", R.rmsnorm(x, g, R.RMSNORM_EPS, F32), ref, ref.abs(), per_row=True)
    ms = (x.double() ** 2).mean(-1)  # eps decides the scale of row 0 and is nothing in the last row
    assert ms[0] < 0.1 * R.RMSNORM_EPS and (M == 1 or ms[-1] > 1e9 * R.RMSNORM_EPS)


@pytest.mark.parametrize("C,rows", R.SNAKE_SHAPES)
def test_fp32_error_snake(C, rows):
    x, al, ib = R.snake_inputs(C, rows, F32)
    _record(f"snake C={C}", R.snake(x, al, ib, F32), R.snake(x, al, ib), x.abs().double() + ib.double())


@pytest.mark.parametrize("B,T", R.DWCONV_BT)
@pytest.mark.parametrize("C", R.DWCONV_CS)
def test_fp32_error_dwconv_ln(C, B, T):
    a = R.dwconv_inputs(B, T, C, F32)
    ref = R.dwconv_ln(*a, R.DWCONV_EPS)
    _record(f"dwconv_ln C={C} B={B} T={T}", R.dwconv_ln(*a, R.DWCONV_EPS, F32), ref, R.row_scale(ref), per_row=True)


@pytest.mark.parametrize("M,N", R.LAYERNORM_SHAPES)
def test_fp32_error_layernorm(M, N):
    a = R.layernorm_inputs(M, N, True)
    ref = R.layernorm(*a, R.LAYERNORM_EPS)
    plain = R.layernorm(*a, R.LAYERNORM_EPS, F32)
    _record(f"layernorm {M}x{N}", plain, ref, R.row_scale(ref), per_row=True)
    if N > 1:  # the mean-1e3 row: a one-pass E[x^2] - E[x]^2 in fp32 is nowhere near the two-pass bound
        x = a[0][-1]
        var1 = (x * x).mean() - x.mean() ** 2
        one = (x - x.mean()) * torch.rsqrt(var1 + R.LAYERNORM_EPS) * a[1] + a[2]
        tol, _ = R.fp32_tolerance(plain, ref, R.row_scale(ref), per_row=True)
        assert not bool(((one.double() - ref[-1]).abs() <= tol[-1]).all())


@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("C", R.TIME_STATS_CS)
@pytest.mark.parametrize("T", R.TIME_STATS_TS)
def test_fp32_error_time_stats(T, C, dtype):
    x, lg = R.time_stats_inputs(2, T, C, dtype)
    for logits in (None, lg):
        ref = R.time_stats(x, logits)
        plain = R.time_stats(x, logits, dtype=F32)
        for name, p, r in zip(("mean", "std"), plain, ref):
            _record(f"time_stats {name} T={T} C={C} logits={logits is not None}", p, r, r.abs().max())
        assert torch.equal(ref[1][:, 1], torch.full((2,), R.f32_scalar(1e-12) ** 0.5, dtype=F64))  # the eps floor
        assert torch.equal(plain[1][:, 1].double(), torch.tensor(R.f32_scalar(1e-12)).sqrt().double().expand(2))


@pytest.mark.parametrize("B,T,C", R.SCALE_ADD_SHAPES)
def test_fp32_error_scale_add(B, T, C):
    x, s, res = R.scale_add_inputs(B, T, C, F32)
    scale = (x.double() * s.double()[:, None]).abs() + res.double().abs()
    _record(f"scale_add {B}x{T}x{C}", R.scale_add(x, s, res, F32), R.scale_add(x, s, res), scale)
