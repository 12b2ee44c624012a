"""CPU-only: qt_gemm's planner (csrc/gemm_route.h) through qt_gemm_route, against tests/golden/gemm_routes.json.

The fixture lists argument descriptions and the plan expected for each: both sides of every threshold of the planner,
every argument error, and the shapes the product issues (talker / code-predictor linears, the codec's conv stages).
qt_gemm_route makes no HIP call and never dereferences a pointer, so the arguments carry made-up addresses.

Regenerate (after a deliberate routing change only):  python tests/test_gemm_plan_host.py --write
(--dump prints the argument blocks for tools/gemm_plan_sweep.cpp, the planner's sanitizer sweep.)
"""
import ctypes
import json
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "gemm_routes.json")
MIB = 1 << 20
DT = {"f32": 0, "bf16": 1, "bad": 2}
FIELDS = ("route", "inner", "ks", "mr", "wpb", "u", "fold", "nt_loads", "pf2_cfg", "pf2_ks", "ntb", "mi", "sk_mi",
          "ws_split")
# description defaults: a linear call of bf16 A x bf16 W -> fp32 with a 16 MiB workspace
DEFAULTS = dict(a="bf16", w="bf16", o="f32", epi=0, act=0, a_act=0, rms=0, gamma=0, bias=0, colscale=0, a_index=0,
                snake=0, out2=0, conv=None, splitk=0, ws_bytes=16 * MIB, a_misalign=0, lda=None, null=None)


def _hip():
    from qwen_tts import _hip
    return _hip


def gemm_args(d):
    """qt_gemm_args of a description; pointers are distinct made-up 16-byte-aligned addresses (A + a_misalign)."""
    _hip_ = _hip()
    d = {**DEFAULTS, **d}
    a = _hip_.GemmArgs()
    a.M, a.N, a.K = d["M"], d["N"], d["K"]
    a.a_dtype, a.w_dtype, a.o_dtype = DT[d["a"]], DT[d["w"]], DT[d["o"]]
    a.A, a.W, a.out = 0x100000 + d["a_misalign"], 0x200000, 0x300000
    a.lda, a.ldo = (d["K"] if d["lda"] is None else d["lda"]), d["N"]
    a.a_index = 0x400000 if d["a_index"] else None
    a.gamma = 0x500000 if d["gamma"] else None
    a.rmsnorm, a.eps = d["rms"], 1e-6
    a.bias = 0x600000 if d["bias"] else None
    a.colscale = 0x700000 if d["colscale"] else None
    a.act, a.epi, a.a_act, a.splitk = d["act"], d["epi"], d["a_act"], d["splitk"]
    if d["conv"]:
        a.taps, a.dil, a.cin, a.cin_pad, a.t_in, a.t_out, a.t_off = d["conv"]
        if d["lda"] is None:
            a.lda = a.cin
    if d["ws_bytes"]:
        a.ws, a.ws_bytes = 0x10000000, d["ws_bytes"]
    if d["snake"]:  # 1: both tables, 2: alpha alone (an argument error)
        a.snake_alpha = 0x800000
        a.snake_inv_beta = 0x900000 if d["snake"] == 1 else None
    if d["out2"]:
        a.out2, a.ldo2 = 0xA00000, d["N"]
    if d["null"]:
        setattr(a, d["null"], None)
    return a


def plan_of(lib, d):
    """{"rc": qt_gemm_route's return, every qt_gemm_route_info field} with the routes by name"""
    _hip_ = _hip()
    info = _hip_.GemmRouteInfo()
    rc = lib.qt_gemm_route(ctypes.byref(gemm_args(d)), ctypes.byref(info))
    out = {"rc": rc}
    for f in FIELDS:
        v = getattr(info, f)
        out[f] = _hip_.ROUTE_NAMES[v] if f in ("route", "inner") else v
    return out


# ---- the argument descriptions -------------------------------------------------------------------------------------
def _conv(taps, dil, cin, B, t_out, cin_pad=None):
    """causal conv group [taps, dil, cin, cin_pad, t_in, t_out, t_off] over B windows of t_out steps"""
    return [taps, dil, cin, (cin + 31) // 32 * 32 if cin_pad is None else cin_pad, t_out, t_out, -(taps - 1) * dil]


def descriptions():
    out = []

    def add(name, M, N, K, **kw):
        out.append(dict(id=name, M=M, N=N, K=K, **kw))

    # decode GEMV: row groups (M 4/5, column tiles 64/65 and 128/129), split-K (column tiles 255/256, k tiles per wave),
    # waves per block (k tiles 15/16, 47/48, 95/96; column tiles 256/257 and 512/513), 16 / 17 rows
    for M in (1, 4, 5, 8, 16, 17):
        for N in (1024, 1040, 2048, 2064, 4080, 4096, 4112, 8192, 8208):
            add(f"gemv_M{M}_N{N}", M, N, 2048)
        for K in (480, 512, 1504, 1536, 3040, 3072, 6144):
            add(f"gemv_M{M}_K{K}", M, 1024, K)
    for N in (16 * 4096, 16 * 4097):  # split-K needs <= 4096 column tiles
        add(f"gemv_splitk4_N{N}", 1, N, 256, splitk=4)
    add("gemv_nt_16MiB", 1, 4096, 2048)      # weight bytes at 16 MiB: non-temporal loads from there
    add("gemv_nt_below", 1, 4080, 2048)
    add("gemv_f32w_nt_16MiB", 1, 2048, 2048, a="f32", w="f32")
    for sk in (0, 1, 4):
        for ws in (0, 4 * MIB - 16, 4 * MIB, 16 * MIB):
            add(f"gemv_splitk{sk}_ws{ws}", 1, 1024, 6144, splitk=sk, ws_bytes=ws)
            add(f"pf2_narrow_splitk{sk}_ws{ws}", 112, 2048, 6144, splitk=sk, ws_bytes=ws)
            add(f"pf2_long_splitk{sk}_ws{ws}", 300, 1024, 3072, splitk=sk, ws_bytes=ws)
    add("gemv_rms_f32a", 8, 4096, 2048, a="f32", rms=1)
    add("gemv_gamma_is_wt", 8, 1024, 2048, a="f32", gamma=1)
    add("gemv_snake", 8, 1024, 2048, snake=1)
    add("gemv_out2", 8, 2048, 2048, epi=1, out2=1)
    add("gemv_a_index", 8, 2048, 2048, a="f32", a_index=1)
    # 17..256 rows of bf16 x bf16: gemm_sk_k (48/49, 64/65 rows; N 4095/4096; N x K at 8 Mi), row-group GEMV while
    # M x N x K <= 400 Mi (N = K = 2048: 100/101 rows), gemm_pf2_k; 255/256/257 rows; N 31/32
    for M in (17, 24, 32, 33, 48, 49, 64, 65, 80, 96, 97, 100, 101, 112, 127, 128, 200, 255, 256, 257):
        add(f"skinny_M{M}_N4096", M, 4096, 2048)
        add(f"skinny_M{M}_N2048", M, 2048, 2048)
        add(f"skinny_M{M}_N1024", M, 1024, 1024)
        if M in (17, 48, 49, 96, 97, 256, 257):
            add(f"skinny_M{M}_N4095", M, 4095, 2048)
            add(f"skinny_M{M}_N4112", M, 4112, 2048)   # N x K just above 8 Mi
            add(f"skinny_M{M}_N2049", M, 2049, 2048)
            add(f"f32a_M{M}_N2049", M, 2049, 2048, a="f32")
        add(f"skinny_M{M}_down", M, 2048, 6144, epi=1)
        # not the skinny rule (fp32 A): row-group GEMV to 96 rows, to 256 rows of <= 2048 columns, then igemm_k / gemm_wt
        add(f"f32a_M{M}_N4096", M, 4096, 2048, a="f32")
        add(f"f32a_M{M}_N2048", M, 2048, 2048, a="f32")
    for N in (16, 31, 32):
        for M in (24, 300):
            add(f"narrow_M{M}_N{N}", M, N, 1024)
            add(f"narrow_f32a_M{M}_N{N}", M, N, 1024, a="f32")
    add("skinny_misaligned_A", 80, 4096, 2048, a_misalign=8)
    add("skinny_lda_odd", 80, 4096, 2048, lda=2052)
    add("skinny_out2_sk", 24, 4096, 2048, out2=1)
    add("skinny_out2_pf2", 112, 4096, 2048, epi=1, out2=1)
    add("skinny_elu", 80, 4096, 2048, a_act=1)
    # gemm_wt fallbacks (K % 32 != 0 keeps bf16 weights off the GEMV; 16/17, 32/33, 64/65 rows) and 127/128 to igemm_k
    for M in (1, 16, 17, 32, 33, 64, 65, 127, 128):
        add(f"wt_M{M}_K40", M, 256, 40, a="f32")
        add(f"wt_f32w_M{M}", M, 256, 64, a="f32", w="f32")
        add(f"wt_f32w_M{M}_K20", M, 256, 20, a="f32", w="f32")
    add("wt_elu_M8", 8, 256, 64, a_act=1)
    # prefill: gemm_pf2_k against gemm_pf_k (K % 64, K % 32, A alignment, lda), igemm_k for fp32 A / gathered rows
    for M in (128, 300, 680, 1024, 4096):
        add(f"pf_M{M}_K2080", M, 2048, 2080)
        add(f"pf_M{M}_K2056", M, 2048, 2056)
        add(f"pf_M{M}_K2052", M, 2048, 2052)
        add(f"pf_M{M}_misaligned_A", M, 2048, 2048, a_misalign=8)
        add(f"pf_M{M}_lda_odd", M, 2048, 2048, lda=2052)
        add(f"pf_M{M}_narrow_N288_K400", M, 288, 400)
        add(f"igemm_M{M}_a_index", M, 2048, 2048, a_index=1)
        add(f"igemm_M{M}_f32a", M, 2048, 2048, a="f32")
        add(f"igemm_M{M}_N96", M, 96, 1024, a="f32")
        add(f"igemm_M{M}_N192", M, 192, 1024, a="f32")
        add(f"wt_M{M}_gamma", M, 2048, 2048, a="f32", gamma=1)
        add(f"wt_M{M}_f32w", M, 2048, 2048, a="f32", w="f32")
    add("pf_out2", 300, 2048, 2080, epi=1, out2=1)
    add("pf2_out2", 300, 2048, 2048, epi=1, out2=1)
    # the product's linears: 1.7B / 0.6B talker and the code predictor (qwen_tts/configs/*/config.json: hidden,
    # intermediate, 16 + 2 x 8 heads of 128, vocab); the code predictor has the 0.6B talker's sizes but for its head
    for model, H, I, V in (("talker17", 2048, 6144, 3072), ("talker06_cp", 1024, 3072, 3072)):
        for M in (1, 8, 16, 24, 80, 112, 200, 680, 4096):
            if H == 1024:
                add(f"cp_head_M{M}", M, 2048, H, rms=1)
            add(f"{model}_qkv_M{M}", M, 4096, H, rms=1)
            add(f"{model}_o_M{M}", M, H, 2048, epi=1, out2=int(M <= 16))
            add(f"{model}_gateup_M{M}", M, 2 * I, H, rms=1, epi=2, o="bf16")
            add(f"{model}_down_M{M}", M, H, I, epi=1, out2=int(M <= 16))
            add(f"{model}_head_M{M}", M, V, H, rms=1)
            if M in (1, 8, 680):
                add(f"{model}_qkv_f32a_M{M}", M, 4096, H, a="f32", rms=1)
                add(f"{model}_gateup_f32a_M{M}", M, 2 * I, H, a="f32", rms=1, epi=2, o="bf16")
    # the codec decoder (qwen_tts/codec.py; speech_tokenizer/config.json: latent 1024, decoder_dim 1536, upsampling
    # 2 x 2, rates 8 5 4 3): one streamed window of B = 8 x 1 frame, and T = 300 of one item
    for tag, B, T in (("win", 8, 1), ("t300", 1, 300)):
        cv = dict(a="bf16", o="bf16", bias=1)
        add(f"codec_{tag}_proj", B * T, 512, 256, a="f32", o="bf16")
        add(f"codec_{tag}_pre_conv", B * T, 1024, 3 * 512, conv=_conv(3, 1, 512, B, T), **cv)
        for nm, N, K, kw in (("inp", 1024, 1024, dict(bias=1)), ("qkv", 3072, 1024, dict(a="f32", rms=1)),
                             ("o", 1024, 1024, dict(a="f32", colscale=1, epi=1)),
                             ("gateup", 6144, 1024, dict(a="f32", rms=1, epi=2)),
                             ("down", 1024, 3072, dict(a="f32", colscale=1, epi=1)),
                             ("outp", 1024, 1024, dict(a="f32", rms=1, bias=1, o="bf16"))):
            add(f"codec_{tag}_tf_{nm}", B * T, N, K, **kw)
        L = T
        for i in range(2):
            add(f"codec_{tag}_up{i}_tconv", B * L, 2048, 1024, conv=[1, 1, 1024, 1024, L, L, 0], **cv)
            L *= 2
            add(f"codec_{tag}_up{i}_pw1", B * L, 4096, 1024, o="bf16", bias=1, act=2)
            add(f"codec_{tag}_up{i}_pw2", B * L, 1024, 4096, o="bf16", bias=1, colscale=1, epi=1)
        add(f"codec_{tag}_conv0", B * L, 1536, 7 * 1024, conv=_conv(7, 1, 1024, B, L), **cv)
        C = 1536
        for r in (8, 5, 4, 3):
            Lw = L if tag == "win" else L - 1   # a streamed window keeps the tap history: every step is produced
            add(f"codec_{tag}_r{r}_tconv", B * Lw, r * (C // 2), 2 * C, conv=[2, 1, C, C, Lw + 1, Lw, 0], snake=1, **cv)
            L, C = Lw * r, C // 2
            for dil in (1, 3, 9):
                add(f"codec_{tag}_r{r}_c1_d{dil}", B * L, C, 7 * C, conv=_conv(7, dil, C, B, L), snake=1, **cv)
            add(f"codec_{tag}_r{r}_c2", B * L, C, C, conv=_conv(1, 1, C, B, L), snake=1, epi=1, **cv)
        add(f"codec_{tag}_conv_last", B * L, 1, 7 * C, conv=_conv(7, 1, C, B, L), snake=1, a="bf16", bias=1)
    # conv routes: im2col to 1024 rows (1024/1025), its workspace (absent / 8 MiB / 16 MiB, splitk 1), igemm_k's staged
    # window (dilation 9 / 10 at 7 taps... 64 rows of reach), conv_n1_k (K <= 2048, window reach 240), ELU, fp32 weights
    for M in (16, 17, 512, 1024, 1025):
        add(f"conv_M{M}_c512_k7", M, 512, 7 * 512, conv=_conv(7, 1, 512, 1, M), o="bf16")
        add(f"conv_M{M}_c512_k7_f32a", M, 512, 7 * 512, conv=_conv(7, 1, 512, 1, M), a="f32", o="bf16")
        add(f"conv_M{M}_c512_k7_nows", M, 512, 7 * 512, conv=_conv(7, 1, 512, 1, M), ws_bytes=0)
        add(f"conv_M{M}_c512_k7_ws8", M, 512, 7 * 512, conv=_conv(7, 1, 512, 1, M), ws_bytes=8 * MIB)
        add(f"conv_M{M}_c512_k7_splitk1", M, 512, 7 * 512, conv=_conv(7, 1, 512, 1, M), splitk=1)
        add(f"conv_M{M}_c96_cinpad", M, 96, 7 * 96, conv=_conv(7, 1, 96, 1, M), ws_bytes=0)
        add(f"conv_M{M}_rms", M, 512, 512, conv=_conv(1, 1, 512, 1, M), rms=1)
        add(f"conv_M{M}_elu", M, 512, 7 * 512, conv=_conv(7, 1, 512, 1, M), a="f32", a_act=1)
        add(f"conv_M{M}_f32w", M, 512, 7 * 512, conv=_conv(7, 1, 512, 1, M, 512), a="f32", w="f32")
        add(f"conv_M{M}_n1", M, 1, 7 * 96, conv=_conv(7, 1, 96, 1, M), ws_bytes=0)
    add("conv_image_8MiB", 1024, 512, 4096, conv=_conv(8, 1, 512, 1, 1024))       # the image fills its half exactly
    add("conv_image_over", 1024, 512, 4608, conv=_conv(9, 1, 512, 1, 1024))
    add("conv_image_sk", 32, 4096, 2048, conv=_conv(2, 1, 1024, 8, 4))             # the image on gemm_sk_k
    add("conv_batch_rows", 96, 512, 7 * 512, conv=_conv(7, 1, 512, 8, 12))
    add("conv_batch_ragged", 100, 512, 7 * 512, conv=_conv(7, 1, 512, 8, 12))     # M % t_out != 0: no im2col
    for dil in (10, 11):   # (taps - 1) * dil at 64: igemm_k's staged window
        add(f"conv_window_d{dil}", 2048, 512, 7 * 512, conv=_conv(7, dil, 512, 1, 2048))
    for dil in (40, 41):   # (taps - 1) * dil at 240: conv_n1_k's window
        add(f"conv_n1_window_d{dil}", 2048, 1, 7 * 96, conv=_conv(7, dil, 96, 1, 2048))
    add("conv_n1_K2048", 2048, 1, 2048, conv=_conv(8, 1, 256, 1, 2048))
    add("conv_n1_K2080", 2048, 1, 2080, conv=_conv(65, 1, 32, 1, 2048))
    add("conv_n1_act", 2048, 1, 7 * 96, conv=_conv(7, 1, 96, 1, 2048), act=1)
    add("conv_n1_short", 8, 1, 7 * 96, conv=_conv(7, 1, 96, 1, 8), ws_bytes=0)
    # every argument error qt_gemm returns, in its precedence
    err = dict(M=8, N=1024, K=2048)
    for nul in ("A", "W", "out"):
        out.append(dict(id=f"err_null_{nul}", **err, null=nul))
    add("err_conv_cin_pad", 64, 512, 0, conv=[7, 1, 512, 520, 64, 64, -6], ws_bytes=0)
    add("err_conv_cin", 64, 512, 0, conv=[7, 1, 500, 512, 64, 64, -6], ws_bytes=0)
    add("err_conv_t_out", 64, 512, 0, conv=[7, 1, 512, 512, 64, 0, -6])
    add("err_K_mod_8", 8, 1024, 2052)
    add("err_K_mod_4_f32w", 8, 1024, 2050, a="f32", w="f32")
    add("err_M_zero", 0, 1024, 2048)
    add("err_M_negative", -4, 1024, 2048)
    add("err_N_zero", 8, 0, 2048)
    add("err_swiglu_N", 8, 1032, 2048, epi=2)
    add("err_swiglu_bias", 8, 1024, 2048, epi=2, bias=1)
    add("err_swiglu_colscale", 8, 1024, 2048, epi=2, colscale=1)
    add("err_out2_conv", 2048, 512, 0, conv=_conv(7, 1, 512, 1, 2048), out2=1)
    add("err_out2_swiglu", 8, 1024, 2048, epi=2, out2=1)
    add("err_out2_bf16_out", 8, 1024, 2048, o="bf16", out2=1)
    add("err_snake_half", 8, 1024, 2048, snake=2)
    add("err_a_act", 8, 1024, 2048, a_act=2)
    add("err_act_low", 8, 1024, 2048, act=-1)
    add("err_act_high", 8, 1024, 2048, act=6)
    add("err_out2_igemm", 300, 2048, 2048, a="f32", out2=1)
    add("err_out2_wt", 8, 1024, 2048, a="f32", gamma=1, out2=1)
    add("err_out2_K_mod_32", 8, 1024, 2056, out2=1)
    add("err_out2_elu", 8, 1024, 2048, a_act=1, out2=1)
    add("err_dtype_f32w_bf16a", 8, 1024, 2048, w="f32")
    add("err_dtype_f32w_bf16o", 8, 1024, 2048, a="f32", w="f32", o="bf16")
    add("err_dtype_a", 8, 1024, 2048, a="bad")
    add("err_dtype_w", 8, 1024, 2048, w="bad", a="f32")
    add("err_dtype_o", 300, 1024, 2048, o="bad")
    add("err_dtype_im2col_a", 64, 512, 0, conv=_conv(7, 1, 512, 1, 64), a="bad")
    add("err_shape_before_arg", 0, 1024, 2048, act=9, a="bad")      # precedence: shape, then argument, then dtype
    add("err_arg_before_dtype", 8, 1024, 2048, act=9, a="bad")
    ids = [d["id"] for d in out]
    assert len(set(ids)) == len(ids)
    return out


def _library():
    return _hip().load_library()


def write_fixture():
    lib = _library()
    rows = [json.dumps({"args": d, "plan": list(plan_of(lib, d).values())}, separators=(",", ":")) for d in descriptions()]
    with open(FIXTURE, "w") as f:
        f.write("[\n" + ",\n".join(rows) + "\n]\n")


def load_fixture(path=FIXTURE):
    """[{"args": description, "plan": {"rc", *FIELDS}}]; the file keeps each plan as the list of those values"""
    with open(path) as f:
        return [{"args": c["args"], "plan": dict(zip(("rc",) + FIELDS, c["plan"]))} for c in json.load(f)]


@pytest.fixture(scope="module")
def cases():
    return load_fixture()


def test_fixture_lists_the_current_descriptions(cases):
    assert [c["args"] for c in cases] == descriptions()


def test_every_plan_matches(cases):
    lib = _library()
    wrong = [(c["args"]["id"], c["plan"], got) for c in cases for got in [plan_of(lib, c["args"])] if got != c["plan"]]
    assert not wrong, wrong[:5]


def test_fixture_covers_every_route_and_configuration(cases):
    names = _hip().ROUTE_NAMES
    plans = [c["plan"] for c in cases]
    assert {p["route"] for p in plans} == set(names)  # NONE: the rejected arguments
    assert {p["inner"] for p in plans if p["route"] == "IM2COL"} >= {"GEMV", "SK", "PF2"}
    assert {p["pf2_cfg"] for p in plans if "PF2" in (p["route"], p["inner"])} == {3, 4, 9, 11, 21, 22, 23}
    assert {p["pf2_ks"] for p in plans if p["pf2_cfg"] in (3, 11)} >= {1, 2, 4}
    assert {(p["ntb"], p["mi"]) for p in plans if "IGEMM" in (p["route"], p["inner"])} == {(8, 2), (6, 2), (4, 1), (6, 1)}
    assert {p["ntb"] for p in plans if p["route"] == "PF"} == {4, 8}
    assert {p["sk_mi"] for p in plans if p["route"] == "SK"} == {2, 3}
    gemv = [p for p in plans if "GEMV" in (p["route"], p["inner"])]
    assert {p["wpb"] for p in gemv} == {4, 8, 16} and {p["u"] for p in gemv} == {4, 8}
    assert {p["fold"] for p in gemv} == {1, 2, 4} and {p["nt_loads"] for p in gemv} == {0, 1}
    assert {p["ks"] for p in gemv} >= {1, 2, 4} and {p["mr"] for p in gemv} >= {1, 2, 4, 8, 16}
    assert {p["rc"] for p in plans} == {0, -1, -2, -3}
    assert all((p["rc"] == 0) == (p["route"] != "NONE") for p in plans)


def test_route_needs_both_pointers():
    lib, _hip_ = _library(), _hip()
    a = gemm_args(dict(M=8, N=1024, K=2048))
    assert lib.qt_gemm_route(ctypes.byref(a), None) == -1
    assert lib.qt_gemm_route(None, ctypes.byref(_hip_.GemmRouteInfo())) == -1


if __name__ == "__main__":
    if sys.argv[1:] not in (["--write"], ["--dump"]):
        sys.exit("usage: python tests/test_gemm_plan_host.py --write | --dump")
    sys.path.insert(0, os.path.join(os.path.dirname(HERE), "qwen3-tts_amd"))
    if sys.argv[1] == "--dump":  # qt_gemm_args' fields as integers (eps as 0), for tools/gemm_plan_sweep.cpp
        for d in descriptions():
            a = gemm_args(d)
            print(*[0 if n == "eps" else int(getattr(a, n) or 0) for n, _ in type(a)._fields_])
    else:
        write_fixture()
        print(f"wrote {FIXTURE}")
