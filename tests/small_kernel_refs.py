"""Plain references for the small memory-bound kernels (csrc/misc.hip) and the voice-clone glue kernels
(csrc/frontend.hip), plus the seeded input builders that the CPU and the GPU tests share.

torch only, no project imports; every function runs on CPU or GPU tensors.  Two kinds of reference:

* ordered-fp32 emulation (`frame_embed_ordered`, `rvq_gather_ordered`): the kernel's sum is a fixed sequence of
  fp32 adds (no multiply, so no fused multiply-add can enter) -- the emulation repeats that sequence and the kernel
  must match it bit for bit.
* fp64 reference (`rmsnorm`, `snake`, `dwconv_ln`, `layernorm`, `time_stats`, `scale_add`): the stored operands
  widened to `dtype` (float64 by default).  The same function with `dtype=torch.float32` is the "plain torch fp32"
  computation whose own error against fp64 the fp32 tolerances are scaled from (`fp32_tolerance`).

bf16 outputs are judged by `bf16_cap`: within one bf16 ulp of the fp64 result rounded to bf16 everywhere, and equal
on >= 99.9 % of the elements.
"""
import torch

F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16
SENTINEL = 7.0


# ------------------------------------------------------------------------------------------ judging helpers
def f32_scalar(v):
    """A Python float as the kernel receives it (a C float argument)."""
    return float(torch.tensor(v, dtype=F32))


def ulp32(x):
    """Spacing of fp32 numbers at magnitude |x| (normal range)."""
    _, e = torch.frexp(x.abs().to(F64).clamp_min(2.0 ** -126))  # |x| = m * 2^e, m in [0.5, 1)
    return torch.ldexp(torch.ones_like(x, dtype=F64), e - 24)


def rowmax(t):
    """max over the last dim, kept (per-row error / magnitude)."""
    return t.amax(-1, keepdim=True)


def fp32_tolerance(plain32, ref64, scale, per_row=False, margin=2.0):
    """Elementwise bound for an fp32 kernel against ref64: margin (2) x the error of plain torch fp32 (measured
    relative to `scale`, its maximum over the case or over each row), never below 4 fp32 ulp of `scale`.  Returns
    (tol, e_torch) with e_torch the scaled torch-fp32 error the bound was derived from."""
    scale = scale.to(F64).expand_as(ref64)
    rel = (plain32.to(F64) - ref64).abs() / scale.clamp_min(2.0 ** -126)
    e = rowmax(rel) if per_row else rel.max()
    return torch.maximum(margin * e * scale, 4.0 * ulp32(scale)), e


def scaled_error(got, ref64, scale, per_row=False):
    scale = scale.to(F64).expand_as(ref64)
    rel = (got.to(F64) - ref64).abs() / scale.clamp_min(2.0 ** -126)
    return rowmax(rel) if per_row else rel.max()


def judge_fp32(got, plain32, ref64, scale, per_row=False, margin=2.0):
    """(every element within fp32_tolerance, kernel's scaled error, torch-fp32's scaled error)."""
    tol, e_torch = fp32_tolerance(plain32, ref64, scale, per_row, margin)
    ok = bool(((got.to(F64) - ref64).abs() <= tol).all())
    return ok, float(scaled_error(got, ref64, scale, per_row).max()), float(e_torch.max())


# The magnitude each kernel's error is measured against:
#   rmsnorm             |ref| per element (a pure product: no cancellation), error maximum per row
#   snake               |x| + inv_beta[c] per element (the two summands' magnitudes), maximum over the case
#   layernorm/dwconv_ln the row's largest |ref| (the centring cancels, so the error is absolute per row), per row
#   time_stats          the case's largest |ref| (weighted sums that cancel), maximum over the case
#   scale_add           |x * s| + |res| per element, maximum over the case
def row_scale(ref64):
    return rowmax(ref64.abs())


def _bf16_ord(t):
    i = t.contiguous().view(torch.int16).to(torch.int32)
    return torch.where(i < 0, -(i & 0x7FFF), i)  # monotonic in the value; -0 and +0 coincide


def bf16_ulp_diff(a, b):
    """Distance between two bf16 tensors in bf16 steps."""
    return (_bf16_ord(a) - _bf16_ord(b)).abs()


def to_bf16(x64):
    """fp64 -> bf16 in one round-to-nearest-even step (through fp32 it would round twice); normal range."""
    m, e = torch.frexp(x64.to(F64))
    return torch.ldexp(torch.round(m * 256.0) / 256.0, e).to(F32).to(BF16)  # torch.round: half to even


def bf16_cap(got_bf16, ref64):
    """(largest bf16-step distance to ref64 rounded to bf16, fraction of equal elements)."""
    d = bf16_ulp_diff(got_bf16, to_bf16(ref64))
    return int(d.max()), float((d == 0).double().mean())


def assert_bf16_cap(got_bf16, ref64, what=""):
    worst, same = bf16_cap(got_bf16, ref64)
    assert worst <= 1 and same >= 0.999, (what, worst, same)
    return worst, same


# ------------------------------------------------------------------------------------------ ordered-fp32 emulations
def _frame_rows(codes, codes_ld, steps, G):
    c = codes.reshape(-1).long()
    return [c[b * codes_ld + t * G: b * codes_ld + (t + 1) * G] for b, t in enumerate(steps)]


def frame_embed_ordered(e0, ecp, G, codes, codes_ld, steps, trailing, T, pad):
    """x[b] = ((e0[c0] + ecp[0][c1]) + ... + ecp[G-2][c_{G-1}]) + (trailing[b, t] if t < T else pad), fp32 adds in
    that order after widening the table rows.  e0 [V0][H], ecp [>= G-1][Vcp][H] (fp32 or bf16), codes int
    [B][codes_ld] holding frames of G codes, steps: the B frame indices, trailing fp32 [B][T][H], pad fp32 [H]."""
    out = []
    for b, c in enumerate(_frame_rows(codes, codes_ld, steps, G)):
        acc = e0[c[0]].to(F32)
        for g in range(1, G):
            acc = acc + ecp[g - 1, c[g]].to(F32)
        t = steps[b]
        out.append(acc + (trailing[b, t] if t < T else pad))
    return torch.stack(out)


def frame_embed_f64(e0, ecp, G, codes, codes_ld, steps, trailing, T, pad):
    """The same sum formed at once in fp64 (one torch.sum over the stacked summands)."""
    out = []
    for b, c in enumerate(_frame_rows(codes, codes_ld, steps, G)):
        t = steps[b]
        rows = [e0[c[0]]] + [ecp[g - 1, c[g]] for g in range(1, G)] + [trailing[b, t] if t < T else pad]
        out.append(torch.stack([r.to(F64) for r in rows]).sum(0))
    return torch.stack(out)


def _rvq_rows(tabs, codes):
    Q, cb, _ = tabs.shape
    c = codes.reshape(-1, Q).long().clamp(0, cb - 1)
    return [tabs[q][c[:, q]] for q in range(Q)]  # Q x [BT][dim]


def rvq_gather_ordered(tabs, codes, n_first):
    """o1 = sum over q < n_first, o2 = sum over the rest, each a sequence of fp32 adds in q order starting from 0;
    codes clamped to the table.  tabs fp32 [Q][cb][dim], codes int [BT][Q]."""
    rows = _rvq_rows(tabs, codes)
    s1, s2 = torch.zeros_like(rows[0]), torch.zeros_like(rows[0])
    for q, r in enumerate(rows):
        if q < n_first:
            s1 = s1 + r
        else:
            s2 = s2 + r
    return s1, s2


def rvq_gather_f64(tabs, codes, n_first):
    r = torch.stack(_rvq_rows(tabs, codes)).to(F64)
    return r[:n_first].sum(0), r[n_first:].sum(0)


# ------------------------------------------------------------------------------------------ fp64 / plain-fp32 references
def rmsnorm(x, g, eps, dtype=F64):
    x, g = x.to(dtype), g.to(dtype)
    return g * (x * torch.rsqrt((x * x).mean(-1, keepdim=True) + f32_scalar(eps)))


def snake(x, alpha, inv_beta, dtype=F64):
    """x [rows][C] (any float dtype, widened): x + inv_beta[c] * sin(x * alpha[c])**2."""
    x = x.to(dtype)
    return x + inv_beta.to(dtype) * torch.sin(x * alpha.to(dtype)) ** 2


def layernorm(x, w, b, eps, dtype=F64):
    x = x.to(dtype)
    d = x - x.mean(-1, keepdim=True)
    return d * torch.rsqrt((d * d).mean(-1, keepdim=True) + f32_scalar(eps)) * w.to(dtype) + b.to(dtype)


def dwconv_ln(x, w, bias, lw, lb, eps, dtype=F64):
    """x [B][T][C]: y[b,t,c] = bias[c] + sum_j w[c,j] * x[b,t-6+j,c] (zeros before t = 0), then LayerNorm over C."""
    B, T, C = x.shape
    xp = torch.cat([torch.zeros(B, 6, C, dtype=dtype, device=x.device), x.to(dtype)], 1)
    y = bias.to(dtype).expand(B, T, C).clone()
    for j in range(7):
        y = y + w.to(dtype)[:, j] * xp[:, j:j + T]
    return layernorm(y, lw, lb, eps, dtype)


def time_stats(x, logits=None, eps=1e-12, dtype=F64):
    """x [B][T][C], logits [B][T][C] or None -> (mean, std) [B][C]: weights softmax(logits) over time (uniform when
    None), mean = sum a x, std = sqrt(max(sum a (x - mean)^2, eps))."""
    x = x.to(dtype)
    a = torch.softmax(logits.to(dtype), 1) if logits is not None else torch.full_like(x, 1.0 / x.shape[1])
    m = (a * x).sum(1)
    v = (a * (x - m[:, None]) ** 2).sum(1)
    return m, torch.sqrt(v.clamp_min(f32_scalar(eps)))


def scale_add(x, s, res, dtype=F64):
    """x, res [B][T][C], s [B][C]: x * s[b] + res."""
    return x.to(dtype) * s.to(dtype)[:, None, :] + res.to(dtype)


# ------------------------------------------------------------------------------------------ seeded inputs
RMSNORM_SHAPES = [(1, 7), (3, 256), (5, 1000), (8, 1024), (2, 2048)]
RMSNORM_EPS = 1e-6


def rmsnorm_inputs(M, N):
    """Row 0 at magnitude ~1e-4 (eps decides the scale), the last row at ~1e3 (eps is nothing), the rest ~1."""
    g = torch.Generator().manual_seed(1000 * M + N)
    x = torch.randn(M, N, generator=g)
    x[0] *= 1e-4
    if M > 1:
        x[-1] *= 1e3
    return x, 1 + 0.1 * torch.randn(N, generator=g)


SNAKE_SHAPES = [(8, 4001), (24, 4001), (96, 333), (1536, 37)]  # (C, rows): rows * C / 8 is no multiple of 256
SNAKE_GRID_CAP = (8, 65536 * 256 + 3)  # one row past the 65,536-block cap of 256-thread blocks


def snake_inputs(C, rows, dtype):
    g = torch.Generator().manual_seed(7 * C + rows % 1000)
    x = (2 * torch.randn(rows, C, generator=g)).to(dtype)
    alpha = torch.exp(0.3 * torch.randn(C, generator=g))
    inv_beta = 1 / (torch.exp(0.3 * torch.randn(C, generator=g)) + 1e-9)
    return x, alpha, inv_beta


DWCONV_CS = [40, 256, 1000, 1024]
DWCONV_BT = [(1, 1), (2, 7), (2, 9)]
DWCONV_EPS = 1e-6


def dwconv_inputs(B, T, C, dtype):
    """Batch 0's last six frames at ~1e3, everything else ~1: a read of batch b-1's tail for t < 6 cannot hide."""
    g = torch.Generator().manual_seed(100 * C + 10 * B + T)
    x = torch.randn(B, T, C, generator=g)
    x[0, max(0, T - 6):] *= 1e3
    w = 0.3 * torch.randn(C, 7, generator=g)
    bias = 0.1 * torch.randn(C, generator=g)
    lw, lb = 1 + 0.1 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g)
    return x.to(dtype), w, bias, lw, lb


LAYERNORM_SHAPES = [(1, 1), (2, 257), (37, 64), (5, 512)]
LAYERNORM_EPS = 1e-5


def layernorm_inputs(M, N, offset_row):
    """offset_row: the last row is 1000 + k/8 with small integers k (mean 1e3, spread ~1).  Every partial sum of
    such a row is an exact fp32 number in any order, so the two-pass kernel and plain torch fp32 see the same mean
    and the 2x rule compares like with like; a one-pass E[x^2] - E[x]^2 form loses the variance outright."""
    g = torch.Generator().manual_seed(31 * M + N)
    x = torch.randn(M, N, generator=g) * 3 + 1
    if offset_row:
        x[-1] = 1000 + torch.randint(-16, 17, (N,), generator=g).float() / 8
    return x, 1 + 0.1 * torch.randn(N, generator=g), 0.1 * torch.randn(N, generator=g)


TIME_STATS_TS = [1, 3, 8, 9, 37]
TIME_STATS_CS = [5, 64, 70, 128]


def time_stats_inputs(B, T, C, dtype):
    """Channel 1 is constant in time (the eps floor decides its std); logits span +-30."""
    g = torch.Generator().manual_seed(1000 * T + C)
    x = torch.randn(B, T, C, generator=g)
    x[:, :, 1] = 0.5
    lg = (torch.rand(B, T, C, generator=g) * 2 - 1) * 30
    return x.to(dtype), lg


SCALE_ADD_SHAPES = [(2, 5, 1), (3, 10, 6), (2, 9, 70)]  # B*T*C = 10, 180, 1260: none a multiple of 256


def scale_add_inputs(B, T, C, dtype):
    g = torch.Generator().manual_seed(100 * T + C)
    x = torch.randn(B, T, C, generator=g).to(dtype)
    s = torch.rand(B, C, generator=g)
    res = torch.randn(B, T, C, generator=g).to(dtype)
    return x, s, res


FRAME_T, FRAME_T_CODES, FRAME_V0, FRAME_VCP = 3, 6, 11, 13


def frame_embed_inputs(H, G, B, dtype):
    """Tables e0 [V0][H] / ecp [max(G-1, 1)][Vcp][H] in dtype, codes int32 [B][T_codes * G + 3] (the three padding
    columns hold valid codes too, so a wrong read shows as a wrong sum, never as a wild index), trailing fp32 with
    T_codes spare rows after its B * T (a kernel that took the trailing branch at t >= T would still read inside
    the buffer), pad fp32 [H]."""
    g = torch.Generator().manual_seed(10000 * B + 100 * G + H)
    e0 = torch.randn(FRAME_V0, H, generator=g).to(dtype)
    ecp = torch.randn(max(G - 1, 1), FRAME_VCP, H, generator=g).to(dtype)
    codes_ld = FRAME_T_CODES * G + 3
    codes = torch.randint(0, min(FRAME_V0, FRAME_VCP), (B, codes_ld), generator=g, dtype=torch.int32)
    trailing = torch.randn(B * FRAME_T + FRAME_T_CODES, H, generator=g)
    pad = torch.randn(H, generator=g)
    return e0, ecp, codes, codes_ld, trailing, pad


def rvq_inputs(Q, cb, dim, BT):
    """tabs fp32 [Q][cb][dim]; codes int32 [BT][Q] with -3 and cb + 2 planted (they must clamp)."""
    g = torch.Generator().manual_seed(1000 * Q + cb + dim + BT)
    tabs = torch.randn(Q, cb, dim, generator=g)
    codes = torch.randint(0, cb, (BT, Q), generator=g, dtype=torch.int32)
    codes[0, 0] = -3
    codes[-1, -1] = cb + 2
    if BT > 2 and Q > 2:
        codes[1, 1], codes[2, Q // 2] = cb + 2, -3
    return tabs, codes
