"""qt_gemm's argument block on the MI355X against the fp64 reference of tests/gemm_refs.py, one launch per case of that
file's table (code path x option set; tests/test_gemm_refs.py shows on a CPU that the table has no empty cell, that
plain torch fp32 meets every bound and that sixteen wrong epilogues / prologues do not).

Per case: the planner is asked again with the real argument block (the route and the plan fields that select the code
path must be the ones the table claims), the call is launched once (twice where it merges split-K partials: the two
results must be bit-equal and the arrival counters back at zero), the stored output is judged against the reference
formed in fp64 on the device, out2 must be bf16(out) bit for bit, and every padding element (out's columns past the
width and its row past M, the same of out2) must still hold its sentinel.

Bounds (gemm_refs.tolerance; none of them taken from what the kernels give): fp32 outputs within max(margin x the
scaled error of plain torch fp32 over the case, 4 ulp32) of the per-element scale (|A'| |W|^T rs + |bias|) |colscale|
+ |residual|; margin 2, and 4 for the split-K merges and for silu_fast in gemm_pf2_k's SwiGLU form.  bf16 outputs
within that plus half a bf16 step: one correct rounding of a value that passes the fp32 judge.

measured on one MI355X run (profiles/gemm_fp64_errors.txt: per case the plan, kernel vs fp64, torch fp32 vs fp64, their
ratio, the margin): see DESIGN.md section 3 for the worst ratio per kernel.
"""
import ctypes

import pytest
import torch

import gemm_refs as G

pytestmark = pytest.mark.gpu

F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16
_WS = {}


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _workspace(dev):
    """One zeroed 16 MiB workspace for the module (the counters must start at zero: a case may not inherit another's)."""
    if dev not in _WS:
        _WS[dev] = torch.zeros(16 * G.MIB, dtype=torch.uint8, device=dev)
    else:
        _WS[dev].zero_()
    return _WS[dev]


def _padded(v, n, dev):
    """A per-column operand in a buffer whose tail (the padded columns of the last weight tile) holds the sentinel."""
    t = torch.full(((n + 15) // 16 * 16 + 16,), G.SENTINEL, dtype=F32, device=dev)
    t[:n] = v
    return t


@pytest.mark.parametrize("cid", [c.id for c in G.cases()])
def test_gemm_against_fp64(cid):
    from qwen_tts import _hip, kernels as Kn
    dev = _dev()
    c = G.case_by_id(cid)
    inp = G.to_device(G.make_inputs(c), dev)
    wt = Kn.tile(inp.W, G.DT[c.w])  # inp.W is already in the weight dtype: the tiles hold exactly these values
    ws = _workspace(dev) if c.ws else None
    keep = dict(bias=_padded(inp.bias, c.N, dev) if c.bias else None,
                colscale=_padded(inp.colscale, c.N, dev) if c.colscale else None)
    A0 = inp.A.clone()
    width = c.N // 2 if c.epi == "swiglu" else c.N

    def launch():
        out = inp.out.clone()
        out2 = inp.out2.clone() if c.out2 else None
        ptrs = dict(A=inp.A.data_ptr(), W=wt.w.data_ptr(), out=out.data_ptr(), idx=_hip.ptr(inp.idx),
                    gamma=_hip.ptr(inp.gamma), bias=_hip.ptr(keep["bias"]), colscale=_hip.ptr(keep["colscale"]),
                    out2=_hip.ptr(out2), ws=_hip.ptr(ws))
        args = G.gemm_args(_hip, c, ptrs)
        info = _hip.GemmRouteInfo()
        rc = _hip.lib().qt_gemm_route(ctypes.byref(args), ctypes.byref(info))
        plan = G.plan_dict(_hip, info, rc)
        assert G.plan_matches(c, plan), (c.plan, plan)
        assert _hip.lib().qt_gemm(ctypes.byref(args), _hip.stream()) == 0
        torch.cuda.synchronize()
        return out, out2, plan

    out, out2, plan = launch()
    bad = []
    if c.plan.get("ws_split"):
        if ws[:16384].any():
            bad.append("arrival counters not back at zero")
        again, again2, _ = launch()
        if not torch.equal(G._bits(out), G._bits(again)) or (c.out2 and not torch.equal(G._bits(out2), G._bits(again2))):
            bad.append("two launches of a split-K call differ")
    ref64 = G.gemm_ref(c, inp, F64)
    plain32 = G.gemm_ref(c, inp, F32)
    rec = G.judge(c, out[:c.M, :width], plain32, ref64, G.err_scale(c, inp))
    print(G.format_record(c, plan, rec))
    if not rec["ok"]:
        bad.append(("outside the bound", rec))
    if not G.padding_ok(out, inp.out, c.M, width):
        bad.append("out: a padding element changed")
    if c.out2:
        if not G.out2_ok(out, out2, c.M, width):
            bad.append("out2 != bf16(out)")
        if not G.padding_ok(out2, inp.out2, c.M, width):
            bad.append("out2: a padding element changed")
    if not torch.equal(G._bits(inp.A), G._bits(A0)):
        bad.append("A changed")
    assert not bad, bad
