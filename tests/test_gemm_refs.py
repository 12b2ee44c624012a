"""CPU-only: the fp64 pin of qt_gemm's argument block (tests/gemm_refs.py) checked against itself and the planner.

* every case of the table is planned by qt_gemm_route onto the kernel and plan fields it claims (made-up aligned
  pointers as in tests/test_gemm_plan_host.py, a 16 MiB workspace where the case has one), and every "unreachable"
  cell is shown to be rerouted or rejected;
* the coverage matrix has no empty (code path, option) cell, and the product's own combinations are on every route
  their operands can reach;
* plain torch fp32 is inside every judge, and so is its rounding to bf16 (the share of bf16 elements that differ
  from to_bf16(ref64) is printed: fp32 error alone flips far more than 0.1 % of a K-deep sum's roundings);
* every mutant of the computation fails the judge wherever it can differ, is bit-equal to the reference elsewhere,
  and is caught on every code path whose kernel implements what it mutates.
"""
import ctypes
from types import SimpleNamespace

import pytest
import torch
import torch.nn.functional as F

import gemm_refs as G

F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16
CASES = G.cases()
BY_PATH = {p: [c for c in CASES if c.path == p] for p in G.ALL_PATHS}
UNREACHABLE = G.unreachable()


def _hip():
    from qwen_tts import _hip
    return _hip


def _plan(case):
    hip = _hip()
    info = hip.GemmRouteInfo()
    rc = hip.load_library().qt_gemm_route(ctypes.byref(G.gemm_args(hip, case, G.FAKE_PTRS)), ctypes.byref(info))
    return G.plan_dict(hip, info, rc)


class _Memo:
    """inputs, references and the tolerance of a case, formed once for the module"""

    def __init__(self):
        self.d = {}

    def __call__(self, case):
        if case.id not in self.d:
            inp = G.make_inputs(case)
            memo = {}
            ref64 = G.gemm_ref(case, inp, F64, memo=memo)
            plain32 = G.gemm_ref(case, inp, F32)
            self.d[case.id] = SimpleNamespace(inp=inp, memo=memo, ref64=ref64, plain32=plain32,
                                              scale=G.err_scale(case, inp))
        return self.d[case.id]


REFS = _Memo()


def _reachable(path, opt):
    if path == "im2col":
        return opt in G.IM2COL_CELLS
    return (path, opt) not in UNREACHABLE


# ------------------------------------------------------------------------------------------ the planner
def test_every_case_reaches_its_kernel():
    wrong = [(c.id, c.plan, got) for c in CASES for got in [_plan(c)] if not G.plan_matches(c, got)]
    assert not wrong, wrong[:5]
    # the two workspace states: split cases have one, the unsplit gemm_pf2_k cases run without
    assert all(c.ws for c in CASES if c.plan.get("ws_split"))
    assert {c.ws for c in CASES if c.plan.get("route") == "PF2"} == {True, False}


def test_paths_are_distinct_code_paths():
    keys = [tuple(sorted(G.PATHS[p].plan.items())) for p in G.PATHS if not p.startswith(("gemv_m", "gemv_rg4"))]
    assert len(set(keys)) == len(keys)
    plans = [G.PATHS[p].plan for p in G.PATHS]
    gemv = [p for p in plans if p["route"] == "GEMV"]
    assert {p["fold"] for p in gemv} == {1, 2, 4} and {p["ks"] for p in gemv} == {1, 2, 3}
    assert {p["mr"] for p in gemv} >= {3, 4, 6, 7, 11, 16}
    assert {p["sk_mi"] for p in plans if p["route"] == "SK"} == {2, 3}
    assert {(p["pf2_cfg"], p["pf2_ks"]) for p in plans if p["route"] == "PF2"} == {(11, 1), (11, 2), (21, 1), (22, 2)}
    assert {p["mi"] for p in plans if p["route"] == "IGEMM"} == {1, 2}
    assert {p["route"] for p in plans} >= {"WT_1x8", "WT_2x8", "WT_4x4", "PF"}
    assert any(c.w == "f32" for c in BY_PATH["gemv_f32w"]) and any(c.gamma for c in BY_PATH["wt_4x4"])
    # gemm_pf2_k: every path in an interior-tile launch and in a ragged one
    for p in G.PATHS:
        if G.PATHS[p].route == "PF2":
            assert {c.full for c in BY_PATH[p]} == {True, False}, p


def _probe(path, opt):
    """The path's call with the option added: the argument blocks whose plans show the cell cannot be reached."""
    if path == "sk_mi4":
        base = SimpleNamespace(**vars(BY_PATH["sk_mi3"][0]))
        base.M = 64
        return [(base, dict(route="SK"))]
    base = next(c for c in BY_PATH[path] if c.o == "f32" and c.epi != "swiglu" and not c.full)
    c = SimpleNamespace(**vars(base))
    plan = dict(base.plan)
    if opt == "gamma":
        c.gamma = 1
    elif opt == "a_index":
        c.a_index = 1
    elif opt == "out2":
        c.out2, c.ldo2 = 1, c.ldo
    elif opt in ("bf16_out", "bf16_out_add"):
        c.o = "bf16"
    elif opt == "k_tail_rms":
        c.rms, c.K, c.lda = 1, c.K + 8, c.lda + 8
    elif opt.startswith("act_"):
        c.act = opt[4:]
    elif opt == "colscale":
        c.colscale = 1
    elif opt == "rms":
        c.rms = 1
    elif opt == "swiglu":
        c.epi = "swiglu"
    elif opt == "m_tail":  # one block holds every row: at any other row count of the route the block still does
        out = []
        for M in range(1, 17):
            d = SimpleNamespace(**vars(c))
            d.M = M
            out.append((d, dict(plan, mr=M + 1)))  # i.e. never a plan with rows beyond the block's
        return out
    else:
        raise AssertionError(opt)
    return [(c, plan)]


@pytest.mark.parametrize("path,opt", sorted(UNREACHABLE))
def test_unreachable_cells_are_rerouted_or_rejected(path, opt):
    for c, claimed in _probe(path, opt):
        got = _plan(c)
        assert got["rc"] != 0 or any(got[k] != v for k, v in claimed.items()), (path, opt, got)
    if opt == "m_tail":  # and the rows of one block are all of M
        for c, _ in _probe(path, opt):
            got = _plan(c)
            assert got["route"] != "GEMV" or got["mr"] == c.M or got["mr"] < c.M  # grouped: another path
        assert G.PATHS[path].plan["mr"] == G.PATHS[path].M


# ------------------------------------------------------------------------------------------ coverage
def test_coverage_matrix_has_no_empty_cell():
    empty, both = [], []
    for path in G.ALL_PATHS:
        for opt in G.OPTIONS:
            covered = any(G.covers(c, REFS(c).inp, opt, REFS(c).ref64) for c in BY_PATH[path])
            if path == "im2col" and opt not in G.IM2COL_CELLS:
                continue
            if not covered and (path, opt) not in UNREACHABLE:
                empty.append((path, opt))
            if covered and (path, opt) in UNREACHABLE:
                both.append((path, opt))
    assert not empty, empty
    assert not both, both
    assert all(p in G.ALL_PATHS or p == "sk_mi4" for p, _ in UNREACHABLE)


def test_the_products_combinations_are_on_every_route():
    """codec o / down: fp32 A + colscale + add; pw1: bias + GELU + bf16 out; pw2: bias + colscale + add + bf16 out."""
    for path, P in G.PATHS.items():
        cs = BY_PATH[path]
        if "f32" in P.a:
            assert any(c.a == "f32" and c.colscale and c.epi == "add" and not c.bias and c.act == "none" and not c.rms
                       for c in cs), path
        if path == "gemv_f32w":  # fp32 weights write fp32 only
            continue
        assert any(c.bias and c.act == "gelu" and c.o == "bf16" and not c.colscale and c.epi == "store" for c in cs), path
        assert any(c.bias and c.colscale and c.epi == "add" and c.o == "bf16" and c.act == "none" for c in cs), path
    inner = BY_PATH["im2col"][0]
    assert inner.bias and inner.act != "none" and inner.epi == "add"


def test_inputs_keep_to_the_contract():
    for c in CASES:
        inp = REFS(c).inp
        assert c.lda % 8 == 0 and c.ldo % 8 == 0 and c.ldo2 % 8 == 0, c.id
        pre = REFS(c).ref64
        assert torch.isfinite(pre).all() and float(pre.abs().max()) < 64, c.id
        if c.colscale:
            cs = inp.colscale
            assert (cs.abs() >= 0.25).all() and (cs.abs() <= 2).all() and (cs > 0).any() and (cs < 0).any()
        if c.a_index:
            idx = inp.idx.long()
            assert len(set(idx.tolist())) < c.M and not torch.equal(idx, torch.arange(c.M)) and int(idx.max()) >= c.M
            assert bool((inp.A[idx].float()[:, :c.K] != G.SENTINEL).all())


def test_conv_reference_is_conv1d():
    for c in BY_PATH["conv_n1"] + BY_PATH["im2col"]:
        cv, inp = c.conv, REFS(c).inp
        x = G._operand(c, inp.A[:cv.B * cv.t, :cv.cin], None, F64).reshape(cv.B, cv.t, cv.cin).permute(0, 2, 1)
        w = inp.W.to(F64).reshape(c.N, cv.taps, cv.cin_pad)[:, :, :cv.cin].permute(0, 2, 1)
        y = F.conv1d(F.pad(x, (-cv.t_off, 0)), w, dilation=cv.dil).permute(0, 2, 1).reshape(c.M, c.N)
        got = G._conv_product(c, inp, F64)
        assert (got - y).abs().max() <= 1e-13 * y.abs().max(), c.id


# ------------------------------------------------------------------------------------------ plain torch fp32
def test_plain_torch_fp32_passes_every_judge(capsys):
    lines = []
    for c in CASES:
        r = REFS(c)
        got = G.stored(c, r.plain32)
        rec = G.judge(c, got, r.plain32, r.ref64, r.scale)
        assert rec["ok"], (c.id, rec)
        if c.o == "bf16":
            assert rec["flips"] < 0.25, (c.id, rec)  # (a sanity bound: most roundings do agree)
            lines.append(f"{c.id}: torch fp32 rounded to bf16 differs from to_bf16(ref64) on {100 * rec['flips']:.2f} %")
    with capsys.disabled():
        print("\n" + "\n".join(lines))
    assert max(float(line.rsplit(" ", 2)[1]) for line in lines) > 0.1  # the 99.9 % cap of the small kernels cannot hold


def test_out2_and_padding_judges():
    c = G.case_by_id("gemv_rg2/sink_silu")
    r = REFS(c)
    out, out2 = G.mutant_image(c, r.inp, None)
    assert G.out2_ok(out, out2, c.M, c.N) and G.padding_ok(out, r.inp.out, c.M, c.N)
    assert G.padding_ok(out2, r.inp.out2, c.M, c.N)
    out[c.M, 0] = 0
    assert not G.padding_ok(out, r.inp.out, c.M, c.N)
    out2[0, 0] = out2[0, 0] * 1.0078125
    assert not G.out2_ok(out, out2, c.M, c.N)


# ------------------------------------------------------------------------------------------ mutants
MUTANT_NEEDS = {  # the cells a mutant's code exists in ("act": any activation)
    "cs_before_act": ("colscale", "act"), "cs_on_residual": ("colscale", "add"), "bias_after_act": ("bias", "act"),
    "bias_scaled_rs": ("bias", "rms"), "rs_from_bf16": ("rms", "f32a"), "mean_over_kp": ("k_tail_rms",),
    "drop_last_ktile": (), "a_index_ignored": ("a_index",), "a_index_on_out": ("a_index",), "lda_as_K": ("lda",),
    "ldo_as_N": ("ldo",), "out2_before_add": ("out2", "add"), "res_f32_from_bf16": ("bf16_out_add",),
    "swiglu_swapped": ("swiglu",), "silu_for_gelu": ("act_gelu",), "gelu_tanh": ("act_gelu",),
}


def _implements(path, need):
    if need == "act":
        return any(_reachable(path, o) for o in G.OPTIONS if o.startswith("act_"))
    if need == "f32a":
        return any(c.a == "f32" for c in BY_PATH[path])
    return _reachable(path, need)


def _mutant_passes(c, r, mut):
    """(the mutant's buffers pass every judge of the case, they equal the reference's buffers bit for bit)"""
    out, out2 = G.mutant_image(c, r.inp, mut, memo=r.memo)
    good, good2 = G.mutant_image(c, r.inp, None, memo=r.memo)
    No = r.ref64.shape[1]
    ok = G.judge(c, out[:c.M, :No], r.plain32, r.ref64, r.scale)["ok"] and G.padding_ok(out, r.inp.out, c.M, No)
    if c.out2:
        ok = ok and G.out2_ok(out, out2, c.M, No) and G.padding_ok(out2, r.inp.out2, c.M, No)
    same = torch.equal(G._bits(out), G._bits(good)) and (out2 is None or torch.equal(G._bits(out2), G._bits(good2)))
    return ok, same


def test_mutant_table_is_complete():
    assert set(G.MUTANTS) == set(MUTANT_NEEDS)


@pytest.mark.parametrize("mut", sorted(G.MUTANTS))
def test_every_mutant_is_caught(mut):
    caught = {p: 0 for p in G.ALL_PATHS}
    for c in CASES:
        r = REFS(c)
        ok, same = _mutant_passes(c, r, mut)
        can = G.MUTANTS[mut](c)
        if can:
            assert not ok, (mut, c.id, "passes the judge")
            caught[c.path] += 1
        elif can is not None:
            assert same, (mut, c.id, "differs where it cannot")
    for path in G.ALL_PATHS:
        if all(_implements(path, n) for n in MUTANT_NEEDS[mut]):
            assert caught[path], (mut, path, "no case of the path can show it")
