"""qt_gemm's argument block against fp64: the reference, the case table, the judges and the mutants that the CPU
file (tests/test_gemm_refs.py) and the GPU file (tests/test_gpu_gemm_fp64.py) share.

torch only; every function runs on CPU or GPU tensors.  The header's contract,

    out (=|+=) epi( rs[m] * sum_k W[n][k] * gamma[k] * A[m][k] + bias[n] ) * colscale[n]

is restated once by `gemm_ref(case, inp, dtype)` from the stored operands.  The operand roundings are single IEEE
operations and are repeated exactly: with bf16 weights the A operand is rounded to bf16 (an unfolded gamma: A * gamma
in fp32, then bf16), with fp32 weights nothing is rounded.  The RMS sum of squares is taken from A as stored, over the
logical K.  Everything after the roundings runs in `dtype`: float64 is the reference, float32 is plain torch fp32,
whose own error the tolerances are scaled from (small_kernel_refs.fp32_tolerance).

The case table is cut along the argument block: `PATHS` lists the kernels and the plan fields that select a code path
in them, each at the smallest shape at which the planner (csrc/gemm_route.h) still picks it plus one more row fragment /
column tile / k stage; `VARIANTS` lists option sets; a case is a (path, variant) pair.  `OPTIONS` are the cells: a cell
(path, option) is covered by a case when taking the option out of the case changes what is stored (`covers`), or it is
in `UNREACHABLE` with the reason and a probe that the planner reroutes or rejects.

Judges (none taken from what the kernels give):
* fp32 out: |got - ref64| <= max(margin x e32 x scale, 4 ulp32(scale)), scale = (|A'| |W|^T rs + |bias|) |colscale|
  + |residual| per element (SwiGLU: the product of the two halves' scales), e32 the largest scaled error of plain
  torch fp32 over the case.  margin 2; margin 4 where the arithmetic differs by construction: the split-K merges
  (plan field ws_split) and silu_fast in gemm_pf2_k's SwiGLU form.
* bf16 out: |got - ref64| <= tol_fp32 + half a bf16 step at |ref64| + tol_fp32: one correct rounding of a value that
  passes the fp32 judge.
* out2 == bf16(out) bit for bit; every padding element keeps its sentinel bit for bit.
"""
import zlib
from types import SimpleNamespace

import torch

from small_kernel_refs import fp32_tolerance, scaled_error, to_bf16

F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16
DT = {"f32": F32, "bf16": BF16}
SENTINEL = 12288.0  # exact in bf16; three orders above every operand
EPS = 1e-6
MIB = 1 << 20
ACTS = {"none": 0, "silu": 1, "gelu": 2, "relu": 3, "sigmoid": 4, "relu_tanh": 5}
EPIS = {"store": 0, "add": 1, "swiglu": 2}
PLAN_FIELDS = ("route", "inner", "mr", "ks", "fold", "ws_split", "sk_mi", "pf2_cfg", "pf2_ks", "ntb", "mi")

OPTIONS = ("bias", "act_silu", "act_gelu", "act_relu", "act_sigmoid", "act_relu_tanh", "colscale", "add", "swiglu",
           "bf16_out", "bf16_out_add", "out2", "ldo", "lda", "rms", "gamma", "a_index", "n_tail", "m_tail", "k_tail_rms")


# ------------------------------------------------------------------------------------------ code paths
def _p(route, M, N, K, a, w, N16=None, splitk=0, ws=True, row_tile=16, full=None, **plan):
    """One code path: the shape (N with a ragged last column tile, N16 its SwiGLU stand-in), the A dtypes it takes
    (the variants alternate), the weight dtype, and the plan fields that select it."""
    return SimpleNamespace(route=route, M=M, N=N, N16=N16 or (N + 15) // 16 * 16, K=K, a=a.split("|"), w=w,
                           splitk=splitk, ws=ws, row_tile=row_tile, full=full, plan=dict(route=route, **plan))


# Smallest shapes found by walking the planner on the CPU (tests/test_gemm_refs.py repeats every query).
PATHS = {
    # decode GEMV, ungrouped (M <= 4): fold 4; 3 column tiles, 5 k tiles over 4 waves
    "gemv_m3": _p("GEMV", 3, 40, 160, "f32|bf16", "bf16", mr=3, ks=1, fold=4, ws_split=0),
    # two row groups (65..128 column tiles): 13 rows -> 7 + 6, fold 2
    "gemv_rg2": _p("GEMV", 13, 1035, 96, "bf16|f32", "bf16", mr=7, ks=1, fold=2, ws_split=0),
    # four row groups (<= 64 column tiles): 13 rows -> 4 + 4 + 4 + 1, fold 4
    "gemv_rg4": _p("GEMV", 13, 40, 96, "f32|bf16", "bf16", mr=4, ks=1, fold=4, ws_split=0),
    # > 128 column tiles: 9..16 rows in one block, fold 1 with bf16 weights
    "gemv_m11": _p("GEMV", 11, 2072, 64, "bf16|f32", "bf16", mr=11, ks=1, fold=1, ws_split=0),
    # fp32 weights: fold 1, k tiles of 16
    "gemv_f32w": _p("GEMV", 6, 40, 80, "f32", "f32", mr=6, ks=1, fold=1, ws_split=0),
    # split-K forced to 3: 7 k tiles -> 3 + 3 + 1 (ragged last split)
    "gemv_split3": _p("GEMV", 3, 40, 224, "bf16|f32", "bf16", splitk=3, mr=3, ks=3, fold=4, ws_split=1),
    # the automatic split of 2: > 4 k tiles per wave on < 256 column tiles (33 k tiles over 8 waves)
    "gemv_auto2": _p("GEMV", 4, 40, 1056, "f32|bf16", "bf16", mr=4, ks=2, fold=4, ws_split=1),
    # 16-row groups of 17..256 rows: 37 rows -> 16 + 16 + 5
    "gemv_rows16": _p("GEMV", 37, 40, 96, "f32|bf16", "bf16", mr=16, ks=1, fold=1, ws_split=0),
    # gemm_sk_k: >= 4096 columns, 17..48 rows; 18 k tiles over 8 waves (3 each, the last waves short)
    "sk_mi2": _p("SK", 21, 4100, 576, "bf16", "bf16", N16=4128, sk_mi=2),
    "sk_mi3": _p("SK", 37, 4100, 576, "bf16", "bf16", N16=4128, sk_mi=3),
    # gemm_wt: fp32 weights (or an unfolded gamma) keep a call off the other kernels
    "wt_1x8": _p("WT_1x8", 7, 40, 72, "f32", "f32|bf16", ),
    "wt_2x8": _p("WT_2x8", 21, 40, 72, "f32", "f32|bf16", row_tile=32),
    "wt_4x4": _p("WT_4x4", 70, 40, 72, "f32", "f32|bf16", row_tile=64),
    # gemm_pf2_k (past the 17..256-row rules: > 256 rows), 4 waves, 64 x 96 tiles, unsplit (no workspace): a ragged
    # launch and an interior-tile one
    "pf2_4w": _p("PF2", 300, 200, 192, "bf16", "bf16", ws=False, row_tile=64, full=(320, 192), pf2_cfg=11, pf2_ks=1),
    # the same tiles with K split in two (>= 32 stages of 64, <= 2048 columns, a workspace): the record merge
    "pf2_4w_split": _p("PF2", 300, 200, 2048, "bf16", "bf16", row_tile=64, full=(320, 192), pf2_cfg=11, pf2_ks=2,
                       ws_split=1),
    # ping-pong configuration 21 (128 x 128 tiles, >= 256 rows): residual chunks of 32 registers
    "pf2_pp": _p("PF2", 400, 4100, 192, "bf16", "bf16", N16=4112, ws=False, row_tile=128, full=(384, 4096), pf2_cfg=21,
                 pf2_ks=1),
    # configuration 22: the ping-pong tiles with K split over two blocks
    "pf2_pp_split": _p("PF2", 710, 2024, 2048, "bf16", "bf16", N16=2032, row_tile=128, full=(768, 2048), pf2_cfg=22,
                       pf2_ks=2, ws_split=1),
    # gemm_pf_k: K % 64 != 0 (K tail with RMSNorm), 128 x 64 tiles
    "pf_ntb4": _p("PF", 150, 72, 200, "bf16", "bf16", row_tile=128, ntb=4),
    # igemm_k as a linear: fp32 A, >= 128 rows; 64-row tiles / 128-row tiles (>= 256 blocks)
    "igemm_mi1": _p("IGEMM", 150, 72, 200, "f32", "bf16", row_tile=64, mi=1, ntb=4),
    "igemm_mi2": _p("IGEMM", 300, 11000, 72, "f32", "bf16", N16=11008, row_tile=128, mi=2, ntb=8),
}

# what a path's kernel takes beyond the common options (UNREACHABLE holds the reasons for the rest)
TAKES_OUT2 = ("GEMV", "SK", "PF2", "PF")
TAKES_A_INDEX = ("GEMV", "WT_1x8", "WT_2x8", "WT_4x4")

# conv_n1_k (one output channel) and the single IM2COL case have their own case lists below
CONV_PATHS = ("conv_n1", "im2col")
ALL_PATHS = tuple(PATHS) + CONV_PATHS

# ------------------------------------------------------------------------------------------ option sets
# pad: ldo / lda / ldo2 beyond the logical widths (multiples of 8 elements)
VARIANTS = {
    # everything at once: RMSNorm (folded gamma), bias, SiLU, colscale, residual add, padded strides, out2
    "sink_silu": dict(rms=1, bias=1, act="silu", colscale=1, epi="add", ldo_pad=8, lda_pad=16, out2=24, ai=0),
    # the codec's pw1: bias, GELU, bf16 out
    "pw1_gelu": dict(bias=1, act="gelu", o="bf16", ai=1),
    # the codec's pw2: bias, colscale, add, bf16 out
    "pw2": dict(bias=1, colscale=1, epi="add", o="bf16", ldo_pad=8, ai=0),
    # the codec transformer's o / down: fp32 A, colscale (LayerScale), add
    "codec_o": dict(a="f32", colscale=1, epi="add", ai=0),
    # gathered rows, ReLU, colscale, out2 beside a padded out
    "gather_relu": dict(a_index=1, bias=1, act="relu", colscale=1, out2=8, ldo_pad=16, lda_pad=8, ai=1),
    # RMSNorm + sigmoid + add into a bf16 out
    "rms_sigmoid": dict(rms=1, bias=1, act="sigmoid", epi="add", o="bf16", lda_pad=8, ai=0),
    # GELU and sigmoid into an fp32 out (fp32 weights write nothing else); the second with RMSNorm on the other A dtype
    "gelu_f32": dict(bias=1, act="gelu", lda_pad=8, ai=0),
    "sigmoid_f32": dict(rms=1, bias=1, act="sigmoid", epi="add", ai=1),
    # tanh(relu) with bias and colscale
    "relu_tanh": dict(bias=1, act="relu_tanh", colscale=1, ai=1),
    # gate / up pairing after RMSNorm, bf16 out as the product issues it, and fp32 out
    "swiglu": dict(rms=1, epi="swiglu", o="bf16", ldo_pad=8, ai=0),
    "swiglu_f32": dict(epi="swiglu", ai=1),
    # an unfolded gamma (gemm_wt only)
    "gamma": dict(gamma=1, bias=1, act="gelu", epi="add", w="bf16", ai=0),
    "gamma_f32w": dict(gamma=1, colscale=1, w="f32", ai=0),
}
FULL_VARIANTS = ("sink_silu", "pw1_gelu", "pw2", "swiglu")  # gemm_pf2_k: repeated as interior-tile launches


def _case(path, variant):
    P, V = PATHS[path], VARIANTS[variant]
    a = V.get("a", P.a[V["ai"] % len(P.a)])
    if a not in P.a:
        return None
    ws = P.w.split("|")
    w = V.get("w", "bf16" if V.get("o") == "bf16" and "bf16" in ws else ws[0])
    if w not in ws or (V.get("gamma") and not P.route.startswith("WT")):
        return None
    if w == "f32" and (a != "f32" or V.get("o", "f32") != "f32"):
        return None  # fp32 weights: fp32 A and fp32 out (QT_ERR_DTYPE otherwise; see UNREACHABLE)
    swiglu = V.get("epi") == "swiglu"
    N = P.N16 if swiglu else P.N
    out2 = V.get("out2", 0) if P.route in TAKES_OUT2 else 0
    a_index = V.get("a_index", 0) if P.route in TAKES_A_INDEX else 0
    return SimpleNamespace(
        id=f"{path}/{variant}", path=path, variant=variant, M=P.M, N=N, K=P.K, a=a, w=w, o=V.get("o", "f32"),
        rms=V.get("rms", 0), gamma=V.get("gamma", 0), bias=V.get("bias", 0), colscale=V.get("colscale", 0),
        act=V.get("act", "none"), epi=V.get("epi", "store"), a_index=a_index,
        lda=P.K + V.get("lda_pad", 0), ldo=(N // 2 if swiglu else N + 7) // 8 * 8 + V.get("ldo_pad", 0),
        out2=int(bool(out2)), ldo2=(N + 7) // 8 * 8 + out2 if out2 else 0, splitk=P.splitk, ws=P.ws, conv=None,
        full=False, plan=dict(P.plan))


def _full_case(path, variant):
    """The interior-tile (FULL) form of a gemm_pf2_k case: M and N whole tiles of every configuration it can run."""
    c = _case(path, variant)
    M, N = PATHS[path].full
    c.id, c.M, c.N = f"{path}/{variant}/full", M, N
    c.ldo = (c.N // 2 if c.epi == "swiglu" else c.N) + VARIANTS[variant].get("ldo_pad", 0)
    c.ldo2 = c.N + VARIANTS[variant].get("out2", 0) if c.out2 else 0
    c.full = True
    return c


def _conv_case(name, taps, dil, cin, B, t_out, w, a="bf16", o="f32", N=1, epi="store", bias=1, act="none", lda_pad=8,
               ldo_pad=7, ws=False, plan=None):
    kt = 32 if w == "bf16" else 16
    cin_pad = (cin + kt - 1) // kt * kt
    path = "conv_n1" if N == 1 else "im2col"
    return SimpleNamespace(
        id=f"{path}/{name}", path=path, variant=name, M=B * t_out, N=N, K=taps * cin_pad, a=a, w=w, o=o, rms=0, gamma=0,
        bias=bias, colscale=0, act=act, epi=epi, a_index=0, lda=(cin + 7) // 8 * 8 + lda_pad, ldo=N + ldo_pad, out2=0, ldo2=0,
        splitk=0, ws=ws, full=False, conv=SimpleNamespace(taps=taps, dil=dil, cin=cin, cin_pad=cin_pad, B=B, t=t_out,
                                              t_off=-(taps - 1) * dil),
        plan=plan or dict(route="CONV_N1"))


def _conv_cases():
    return [
        # bf16 weights round the A operand; fp32 A goes the scalar staging path, bf16 A the vector one
        _conv_case("bf16w_f32a", 7, 1, 40, 2, 37, "bf16", a="f32"),
        _conv_case("bf16w_add", 3, 2, 40, 1, 300, "bf16", epi="add"),                 # a second 256-step window
        _conv_case("bf16w_bf16out_add", 7, 3, 24, 2, 37, "bf16", o="bf16", epi="add", ldo_pad=15),
        _conv_case("f32w_add", 5, 1, 20, 2, 37, "f32", a="f32", epi="add", bias=0),
        _conv_case("span240", 7, 40, 24, 1, 300, "bf16"),                            # (taps - 1) * dil = 240
        _conv_case("span240_f32w", 7, 40, 20, 1, 270, "f32", a="f32", epi="add"),
        # im2col_k + the decode GEMV on the image: the rewrite hands bias + act + add through
        _conv_case("bias_silu_add", 2, 1, 64, 4, 3, "bf16", a="f32", N=40, epi="add", act="silu", ldo_pad=8, ws=True,
                   plan=dict(route="IM2COL", inner="GEMV", mr=3, fold=4)),
    ]


def _all_cases():
    out = []
    for path, P in PATHS.items():
        out += [c for c in (_case(path, v) for v in VARIANTS) if c is not None]
        if P.full:
            out += [_full_case(path, v) for v in FULL_VARIANTS]
    out += _conv_cases()
    ids = [c.id for c in out]
    assert len(set(ids)) == len(ids)
    return out


_CASES = None


def cases():
    """The case table (built once)."""
    global _CASES
    if _CASES is None:
        _CASES = _all_cases()
    return _CASES


def case_by_id(cid):
    return next(c for c in cases() if c.id == cid)


def margin_of(case):
    """2, or 4 for the two named differences: a split-K merge, silu_fast in gemm_pf2_k's SwiGLU form."""
    pf2 = "PF2" in (case.plan.get("route"), case.plan.get("inner"))
    return 4.0 if case.plan.get("ws_split") or (pf2 and case.epi == "swiglu") else 2.0


# ------------------------------------------------------------------------------------------ unreachable cells
# (path, option) -> reason.  tests/test_gemm_refs.py probes each one: the path's base call with the option
# added must be rejected by qt_gemm_route or planned onto another path.
def unreachable():
    U = {}
    lin = tuple(PATHS)
    for p in lin:
        if not p.startswith("wt"):
            U[(p, "gamma")] = "an unfolded gamma keeps a call off every kernel but gemm_wt"
    for p in (p for p in lin if PATHS[p].route not in TAKES_A_INDEX):
        U[(p, "a_index")] = "gathered rows go to the row-group GEMV / gemm_wt"
    for p in (p for p in lin if PATHS[p].route not in TAKES_OUT2):
        U[(p, "out2")] = "out2 is written by gemv_wt, gemm_sk_k, gemm_pf2_k and gemm_pf_k only (QT_ERR_ARG)"
    for p in ("gemv_f32w",):
        for o in ("bf16_out", "bf16_out_add"):
            U[(p, o)] = "fp32 weights write fp32 only (QT_ERR_DTYPE)"
    for p in lin:
        P = PATHS[p]
        if P.route in ("GEMV", "SK", "PF2"):
            U[(p, "k_tail_rms")] = "needs K % KT == 0 (GEMV) / K % 64 == 0 (SK, PF2): a K tail goes to gemm_wt / gemm_pf_k / igemm_k"
    U[("gemv_m3", "m_tail")] = U[("gemv_split3", "m_tail")] = U[("gemv_auto2", "m_tail")] = \
        "ungrouped decode rows: one block holds all M <= 4 rows, there is no row tile to be off"
    U[("gemv_m11", "m_tail")] = U[("gemv_f32w", "m_tail")] = "one block holds all M <= 16 rows"
    for o in OPTIONS:
        if o.startswith("act_") or o in ("colscale", "rms", "gamma", "a_index"):
            U[("conv_n1", o)] = "conv_n1_k takes none of act / colscale / rmsnorm / gamma / a_index: such a call goes to gemm_wt"
    U[("conv_n1", "swiglu")] = "N = 1 is no SwiGLU width (QT_ERR_SHAPE)"
    U[("conv_n1", "out2")] = "out2 is for linear calls (QT_ERR_ARG)"
    U[("conv_n1", "k_tail_rms")] = "no rmsnorm on conv_n1_k"
    U[("sk_mi4", "*")] = "gemm_sk_k's 4-fragment form needs 49..64 rows; the planner's row bound is 48 (GemmKnobs::sk_max_m)"
    return U


# One IM2COL case shows that the rewritten call keeps its epilogue; the inner routes are pinned directly, so the other
# cells of that row are not claimed.
IM2COL_CELLS = ("bias", "act_silu", "add", "ldo", "lda", "n_tail")


# ------------------------------------------------------------------------------------------ inputs
def _gen(case):
    return torch.Generator().manual_seed(zlib.crc32(case.id.encode()))


def _nout(case):
    return case.N // 2 if case.epi == "swiglu" else case.N


def make_inputs(case):
    """Seeded CPU tensors of a case.  A: rows of differing magnitude (so the RMS scale matters); W sized for
    pre-activation values of about +-3; bias and residual of the product's order; colscale +-[0.25, 2]; every padding
    element (A's columns K..lda, the gather table's unused rows, out's and out2's columns past the width, a row past
    M in each buffer) holds SENTINEL."""
    g = _gen(case)
    M, N, K = case.M, case.N, case.K
    ad, wd, od = DT[case.a], DT[case.w], DT[case.o]
    r = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    inp = SimpleNamespace()
    if case.conv:
        cv = case.conv
        A = torch.full((cv.B * cv.t + 1, case.lda), SENTINEL)
        A[:cv.B * cv.t, :cv.cin] = r(cv.B * cv.t, cv.cin)
        W = torch.zeros(N, cv.taps, cv.cin_pad)
        W[:, :, :cv.cin] = r(N, cv.taps, cv.cin) * (1.5 / (cv.taps * cv.cin) ** 0.5)
        inp.W = W.reshape(N, K).to(wd)
        inp.idx = None
    else:
        rows = M + 5 if case.a_index else M
        A = torch.full((rows + 1, case.lda), SENTINEL)
        mag = 0.5 + 1.5 * torch.rand(rows, generator=g)
        A[:rows, :K] = r(rows, K) * mag[:, None]
        inp.idx = None
        if case.a_index:  # no identity, repeats, some table rows unused
            idx = torch.randint(0, rows, (M,), generator=g)
            idx[0], idx[1] = rows - 1, rows - 1
            idx[-1] = 0
            unused = torch.ones(rows, dtype=torch.bool)
            unused[idx] = False
            A[:rows][unused] = SENTINEL
            inp.idx = idx.to(torch.int32)
        wstd = 1.5 / K ** 0.5 / (1.0 if case.rms or case.gamma else 1.25)
        inp.W = (r(N, K) * wstd).to(wd)
    inp.A = A.to(ad)
    inp.gamma = (1 + 0.3 * r(K)) if case.gamma else None
    inp.bias = r(N) if case.bias else None
    inp.colscale = None
    if case.colscale:
        sign = torch.where(torch.rand(N, generator=g) < 0.5, -1.0, 1.0)
        inp.colscale = sign * (0.25 + 1.75 * torch.rand(N, generator=g))
    No = _nout(case)
    out = torch.full((M + 1, case.ldo), SENTINEL)
    if case.epi == "add":
        out[:M, :No] = r(M, No)
    inp.out = out.to(od)
    inp.out2 = torch.full((M + 1, case.ldo2), SENTINEL, dtype=BF16) if case.out2 else None
    return inp


def to_device(inp, dev):
    return SimpleNamespace(**{k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in vars(inp).items()})


# ------------------------------------------------------------------------------------------ the reference
def act_ref(x, act):
    if act == "silu":
        return x * torch.sigmoid(x)
    if act == "gelu":  # the erf form (common.h gelu_f)
        return 0.5 * x * (1.0 + torch.erf(x * 0.7071067811865476))
    if act == "relu":
        return torch.relu(x)
    if act == "sigmoid":
        return torch.sigmoid(x)
    if act == "relu_tanh":
        return torch.tanh(torch.relu(x))
    if act == "gelu_tanh":  # mutant only
        return 0.5 * x * (1.0 + torch.tanh(0.7978845608028654 * (x + 0.044715 * x ** 3)))
    return x


def _kt(case):
    return 32 if case.w == "bf16" else 16


def _a_rows(case, inp, mut):
    """A's logical rows [M][K] as stored."""
    M, K = case.M, case.K
    if mut == "lda_as_K":
        flat = inp.A.reshape(-1)
        rows = inp.idx.long() if case.a_index else torch.arange(M, device=flat.device)
        return flat[(rows[:, None] * K + torch.arange(K, device=flat.device)[None, :])]
    if case.a_index and mut not in ("a_index_ignored", "a_index_on_out"):
        return inp.A[inp.idx.long(), :K]
    return inp.A[:M, :K]


def _operand(case, a, gamma, dtype):
    """The A operand after the kernel's rounding, in dtype."""
    if gamma is not None:
        x = a.to(F32) * gamma.to(F32)
        return x.to(BF16).to(dtype) if case.w == "bf16" else a.to(dtype) * gamma.to(dtype)
    return a.to(BF16).to(dtype) if case.w == "bf16" else a.to(dtype)


def _conv_product(case, inp, dtype, absolute=False, mut=None):
    """sum over taps and channels of W[n][j][c] x[b][t + t_off + j dil][c] (zero outside [0, t_in)), as tap-wise
    matrix products: conv1d on the rounded operand."""
    cv = case.conv
    a = inp.A[:cv.B * cv.t, :cv.cin]
    if mut == "lda_as_K":  # rows taken at a stride of cin
        a = inp.A.reshape(-1)[:cv.B * cv.t * cv.cin].reshape(cv.B * cv.t, cv.cin)
    x = _operand(case, a, None, dtype).reshape(cv.B, cv.t, cv.cin)
    if mut == "drop_last_ktile":  # the last 32-channel chunk
        x = x.clone()
        x[:, :, (cv.cin - 1) // 32 * 32:] = 0
    W = inp.W.to(dtype).reshape(case.N, cv.taps, cv.cin_pad)[:, :, :cv.cin]
    if absolute:
        x, W = x.abs(), W.abs()
    xp = torch.cat([torch.zeros(cv.B, -cv.t_off, cv.cin, dtype=dtype, device=x.device), x], 1)
    y = torch.zeros(cv.B, cv.t, case.N, dtype=dtype, device=x.device)
    for j in range(cv.taps):
        y = y + xp[:, j * cv.dil: j * cv.dil + cv.t] @ W[:, j].T
    return y.reshape(cv.B * cv.t, case.N)


def _swiglu_split(y):
    """[M][N] with 8 gate / 8 up columns per 16 -> (gate, up), each [M][N / 2]."""
    M, N = y.shape
    t = y.reshape(M, N // 16, 2, 8)
    return t[:, :, 0].reshape(M, N // 2), t[:, :, 1].reshape(M, N // 2)


OPERAND_MUTANTS = ("lda_as_K", "a_index_ignored", "a_index_on_out", "drop_last_ktile")


def gemm_ref(case, inp, dtype=F64, mut=None, parts=False, memo=None):
    """What the call leaves in out[:M, :width], in dtype (before the rounding to o_dtype).  mut: a wrong variant
    (MUTANTS).  parts: also the value before the residual add (out2's mutant).  memo: a dict that keeps the operand
    product between calls on one case (the mutants mostly share it)."""
    key = (dtype, mut if mut in OPERAND_MUTANTS else None)
    M, N, K = case.M, case.N, case.K
    dev = inp.A.device
    rs = None
    if case.conv:
        y = memo[key] if memo is not None and key in memo else _conv_product(case, inp, dtype, mut=mut)
    else:
        a = _a_rows(case, inp, mut)
        if case.rms or case.gamma:
            src = a.to(BF16) if mut == "rs_from_bf16" else a
            ss = (src.to(dtype) ** 2).sum(-1, keepdim=True)
            kden = (K + _kt(case) - 1) // _kt(case) * _kt(case) if mut == "mean_over_kp" else K
            rs = torch.rsqrt(ss / kden + float(torch.tensor(EPS, dtype=F32)))
        x = _operand(case, a, inp.gamma if case.gamma else None, dtype)
        if mut == "drop_last_ktile":
            x = x.clone()
            x[:, (K - 1) // _kt(case) * _kt(case):] = 0
        y = memo[key] if memo is not None and key in memo else x @ inp.W.to(dtype).T
    if memo is not None:
        memo[key] = y
    bias = inp.bias.to(dtype) if case.bias else None  # (the case's flags decide: `covers` takes options out)
    cs = inp.colscale.to(dtype) if case.colscale else None
    if mut == "bias_scaled_rs" and bias is not None:
        y = y + bias
        bias = None
    if rs is not None:
        y = y * rs
    act = case.act
    if mut == "silu_for_gelu" and act == "gelu":
        act = "silu"
    if mut == "gelu_tanh" and act == "gelu":
        act = "gelu_tanh"
    if mut == "cs_before_act" and cs is not None:
        y = act_ref((y + bias if bias is not None else y) * cs, act)
    elif mut == "bias_after_act" and bias is not None:
        y = act_ref(y, act) + bias
        y = y * cs if cs is not None else y
    else:
        y = act_ref(y + bias if bias is not None else y, act)
        y = y * cs if cs is not None else y
    if case.epi == "swiglu":
        gate, up = _swiglu_split(y)
        if mut == "swiglu_swapped":
            gate, up = up, gate
        y = gate * torch.sigmoid(gate) * up
    pre = y
    if case.epi == "add":
        No = y.shape[1]
        if mut == "res_f32_from_bf16" and case.o == "bf16":
            flat = inp.out.contiguous().reshape(-1)
            raw = flat[:flat.numel() // 2 * 2].view(F32)  # pairs of bf16 read as one fp32
            at = torch.arange(M, device=dev)[:, None] * case.ldo + torch.arange(No, device=dev)[None, :]
            res = raw[at % raw.numel()].to(dtype)
        else:
            res = inp.out[:M, :No].to(dtype)
        y = res + y
        if mut == "cs_on_residual" and cs is not None:
            y = (res + pre / cs) * cs
    if mut == "a_index_on_out" and case.a_index:  # row m's result lands in row idx[m] (folded into [0, M))
        z = (inp.out[:M, :y.shape[1]].to(dtype)).clone()
        z[inp.idx.long() % M] = y
        y = z
    return (y, pre) if parts else y


def err_scale(case, inp):
    """The magnitude fp32 rounding in the call is proportional to, per stored element (fp64)."""
    M, K = case.M, case.K
    if case.conv:
        s = _conv_product(case, inp, F64, absolute=True)
    else:
        a = _a_rows(case, inp, None)
        s = _operand(case, a, inp.gamma if case.gamma else None, F64).abs() @ inp.W.to(F64).abs().T
        if case.rms or case.gamma:
            s = s * torch.rsqrt((a.to(F64) ** 2).sum(-1, keepdim=True) / K + EPS)
    if case.bias:
        s = s + inp.bias.to(F64).abs()
    if case.colscale:
        s = s * inp.colscale.to(F64).abs()
    if case.epi == "swiglu":
        g, u = _swiglu_split(s)
        s = g * u
    if case.epi == "add":
        s = s + inp.out[:M, :s.shape[1]].to(F64).abs()
    return s


def stored(case, y):
    """y (fp64 or fp32) as the o_dtype buffer holds it."""
    if case.o == "bf16":
        return to_bf16(y) if y.dtype == F64 else y.to(BF16)
    return y.to(F32)


# ------------------------------------------------------------------------------------------ judges
def half_bf16_step(x):
    """Half the spacing of bf16 numbers at magnitude |x|."""
    _, e = torch.frexp(x.abs().to(F64).clamp_min(2.0 ** -126))
    return torch.ldexp(torch.ones_like(x, dtype=F64), e - 9)


def tolerance(case, plain32, ref64, scale):
    """(elementwise bound on |got - ref64|, torch-fp32's scaled error)"""
    tol, e32 = fp32_tolerance(plain32, ref64, scale, margin=margin_of(case))
    if case.o == "bf16":
        tol = tol + half_bf16_step(ref64.abs() + tol)
    return tol, float(e32)


def judge(case, got, plain32, ref64, scale):
    """got: the stored out[:M, :width] (o_dtype).  -> dict(ok, e_kernel, e_torch, ratio, worst = largest
    |got - ref64| / bound, flips = share of bf16 elements that differ from to_bf16(ref64))."""
    tol, e32 = tolerance(case, plain32, ref64, scale)
    err = (got.to(F64) - ref64).abs()
    rec = dict(ok=bool((err <= tol).all()), e_torch=e32, e_kernel=float(scaled_error(got, ref64, scale)),
               worst=float((err / tol).max()), flips=None)
    rec["ratio"] = rec["e_kernel"] / max(e32, 2.0 ** -30)
    if case.o == "bf16":
        rec["flips"] = float((got != to_bf16(ref64)).double().mean())
    return rec


def out2_ok(out, out2, M, N):
    """out2 == bf16(out), bit for bit (one round-to-nearest-even)."""
    return torch.equal(out2[:M, :N].view(torch.int16), out[:M, :N].to(BF16).view(torch.int16))


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF16 else torch.int32)


def padding_ok(buf, init, M, width):
    """Everything outside [:M, :width] still holds what it held (the sentinel), bit for bit."""
    a, b = _bits(buf), _bits(init)
    return torch.equal(a[M:], b[M:]) and torch.equal(a[:M, width:], b[:M, width:])


ROUTE_FIELDS = {"GEMV": ("mr", "ks", "fold", "ws_split"), "SK": ("sk_mi",), "PF2": ("pf2_cfg", "pf2_ks", "ws_split"),
                "PF": ("ntb",), "IGEMM": ("ntb", "mi")}


def format_record(case, plan, rec):
    """One line of profiles/gemm_fp64_errors.txt.  plan: plan_dict of the launch."""
    kernel = plan["inner"] if plan["route"] == "IM2COL" else plan["route"]
    fields = " ".join(f"{k} {plan[k]}" for k in ROUTE_FIELDS.get(kernel, ()))
    route = plan["route"] + (f" inner {kernel}" if plan["route"] == "IM2COL" else "")
    head = f"gemmpin | {case.id} | {route} {fields}".rstrip()
    if case.o == "bf16":
        body = f"bf16 |got-ref64|/bound {rec['worst']:.2f} | differs from bf16(ref64) on {100 * rec['flips']:.2f} %"
    else:
        body = f"kernel {rec['e_kernel']:.3g} | torch-fp32 {rec['e_torch']:.3g} | ratio {rec['ratio']:5.2f}"
    return f"{head} | {body} | margin {margin_of(case):g} | {'ok' if rec['ok'] else 'FAIL'}"


# ------------------------------------------------------------------------------------------ mutants
# name -> can it differ at a case: True (it must fail the judge there), False (it must be bit-equal there), None (it
# differs by less than the output format resolves: rs from the bf16-rounded A moves a row by about 2^-9 / sqrt(K)
# of itself, far inside half a bf16 step, so only fp32 outputs are asked to show it)
MUTANTS = {
    "cs_before_act": lambda c: c.colscale and c.act != "none",
    "cs_on_residual": lambda c: c.colscale and c.epi == "add",
    "bias_after_act": lambda c: c.bias and c.act != "none",
    "bias_scaled_rs": lambda c: c.bias and (c.rms or c.gamma),
    "rs_from_bf16": lambda c: (None if c.o == "bf16" else True) if (c.rms or c.gamma) and c.a == "f32" else False,
    "mean_over_kp": lambda c: (c.rms or c.gamma) and c.K % _kt(c) != 0,
    "drop_last_ktile": lambda c: True,
    "a_index_ignored": lambda c: c.a_index,
    "a_index_on_out": lambda c: c.a_index,
    "lda_as_K": lambda c: c.lda != (c.conv.cin if c.conv else c.K),
    "ldo_as_N": lambda c: c.ldo != _nout(c),
    "out2_before_add": lambda c: c.out2 and c.epi == "add",
    "res_f32_from_bf16": lambda c: c.o == "bf16" and c.epi == "add",
    "swiglu_swapped": lambda c: c.epi == "swiglu",
    "silu_for_gelu": lambda c: c.act == "gelu",
    "gelu_tanh": lambda c: c.act == "gelu",
}


def mutant_image(case, inp, mut, memo=None):
    """(out, out2) buffers as the wrong computation `mut` would leave them (fp64 arithmetic, one rounding)."""
    y, pre = gemm_ref(case, inp, F64, mut=mut, parts=True, memo=memo)
    M, No = y.shape
    out = inp.out.clone()
    if mut == "ldo_as_N":
        flat = out.reshape(-1)
        at = torch.arange(M)[:, None] * No + torch.arange(No)[None, :]
        flat[at] = stored(case, y)
    else:
        out[:M, :No] = stored(case, y)
    out2 = None
    if case.out2:
        out2 = inp.out2.clone()
        out2[:M, :No] = (stored(case, pre) if mut == "out2_before_add" else out[:M, :No]).to(BF16)
    return out, out2


# ------------------------------------------------------------------------------------------ coverage
def _without(case, opt):
    """The case with one option taken out (None: the option is not in the case)."""
    c = SimpleNamespace(**vars(case))
    if opt == "bias" and case.bias:
        c.bias = 0
    elif opt.startswith("act_") and case.act == opt[4:]:
        c.act = "none"
    elif opt == "colscale" and case.colscale:
        c.colscale = 0
    elif opt == "add" and case.epi == "add":
        c.epi = "store"
    elif opt in ("rms", "k_tail_rms") and case.rms:
        c.rms = 0
    elif opt == "gamma" and case.gamma:
        c.gamma = 0
    elif opt == "a_index" and case.a_index:
        c.a_index = 0
    else:
        return None
    return c


def covers(case, inp, opt, ref64=None):
    """Does this case pin the cell `opt`: is the option there, and would what is stored change without it."""
    No = _nout(case)
    if opt == "swiglu":
        return case.epi == "swiglu"  # another output width altogether
    if opt == "bf16_out":
        return case.o == "bf16"
    if opt == "bf16_out_add":  # the residual read back from a bf16 out
        return case.o == "bf16" and case.epi == "add" and bool(inp.out[:case.M, :No].float().abs().max() > 0)
    if opt == "out2":
        return bool(case.out2) and case.ldo2 != case.ldo
    if opt == "ldo":
        return case.ldo > No
    if opt == "lda":
        return case.lda > (case.conv.cin if case.conv else case.K)
    if opt == "n_tail":
        return case.N % 16 != 0
    if opt == "m_tail":  # rows per block: the GEMV's row group, the kernel's row tile, conv_n1_k's 256 steps
        if case.conv:
            return case.path == "conv_n1" and case.conv.t % 256 != 0
        P = PATHS[case.path]
        return case.M % (P.plan.get("mr") or P.row_tile) != 0
    if opt == "k_tail_rms" and (case.conv or case.K % _kt(case) == 0 or not case.rms):
        return False
    c = _without(case, opt)
    if c is None:
        return False
    ref64 = gemm_ref(case, inp, F64) if ref64 is None else ref64
    if opt == "a_index":
        other = gemm_ref(case, inp, F64, mut="a_index_ignored")
    else:
        other = gemm_ref(c, inp, F64)
    return not torch.equal(other, ref64)


# ------------------------------------------------------------------------------------------ the argument block
def gemm_args(hip, case, ptrs):
    """qt_gemm_args of a case.  hip: the qwen_tts._hip module; ptrs: addresses of A, W, out, and of the optional
    operands the case uses (idx, gamma, bias, colscale, out2, ws)."""
    a = hip.GemmArgs()
    a.M, a.N, a.K = case.M, case.N, case.K
    code = {"f32": 0, "bf16": 1}
    a.a_dtype, a.w_dtype, a.o_dtype = code[case.a], code[case.w], code[case.o]
    a.A, a.W, a.out = ptrs["A"], ptrs["W"], ptrs["out"]
    a.lda, a.ldo = case.lda, case.ldo
    a.a_index = ptrs["idx"] if case.a_index else None
    a.gamma = ptrs["gamma"] if case.gamma else None
    a.rmsnorm, a.eps = int(bool(case.rms or case.gamma)), EPS
    a.bias = ptrs["bias"] if case.bias else None
    a.colscale = ptrs["colscale"] if case.colscale else None
    a.act, a.epi, a.splitk = ACTS[case.act], EPIS[case.epi], case.splitk
    if case.conv:
        cv = case.conv
        a.taps, a.dil, a.cin, a.cin_pad, a.t_in, a.t_out, a.t_off = cv.taps, cv.dil, cv.cin, cv.cin_pad, cv.t, cv.t, cv.t_off
    if case.ws:
        a.ws, a.ws_bytes = ptrs["ws"], 16 * MIB
    if case.out2:
        a.out2, a.ldo2 = ptrs["out2"], case.ldo2
    return a


FAKE_PTRS = dict(A=0x100000, W=0x200000, out=0x300000, idx=0x400000, gamma=0x500000, bias=0x600000, colscale=0x700000,
                 out2=0xA00000, ws=0x10000000)


def plan_dict(hip, info, rc=0):
    d = {"rc": rc}
    for f in PLAN_FIELDS:
        v = getattr(info, f)
        d[f] = hip.ROUTE_NAMES[v] if f in ("route", "inner") else v
    return d


def plan_matches(case, got):
    """The planner's answer carries the route and every plan field the table claims."""
    return got["rc"] == 0 and all(got[k] == v for k, v in case.plan.items())
