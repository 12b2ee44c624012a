"""One qt_gemm call per entry of tests/golden/gemm_routes.json that is not an argument error, on real tensors.

    python tools/gemm_route_trace.py run <fixture.json> <digests.json>
        seeded A / tiled W / bias / scales, a zeroed workspace of the entry's size, K.gemm once; writes the sha256
        of every output (and of out2).  Run it under `rocprofv3 --kernel-trace --output-format csv -- python ...`
    python tools/gemm_route_trace.py kernels <kernel_trace.csv> <launches.json>
        the ordered qt_gemm launches of that trace: [kernel with template arguments, grid, workgroup, LDS bytes]
    python tools/gemm_route_trace.py diff <a.json> <b.json>
        one line: identical, or the first entries that differ
    python tools/gemm_route_trace.py summary <launches.json> <digests.json>
        the record kept under profiles/: sha256 of the ordered launch list and of the digest list, launches per kernel

Two trees (before / after a routing change) must give identical launches and digests: same kernels, same bits.
Uses only qwen_tts.kernels' long-standing API (tile, gemm, use_workspace) so it runs on older trees as it is.
"""
import csv
import hashlib
import json
import os
import re
import sys

GEMM_KERNELS = ("gemv_wt", "gemm_wt", "gemm_sk_k", "gemm_pf2_k", "gemm_pf_k", "igemm_k", "conv_n1_k", "im2col_k")
DEFAULTS = dict(a="bf16", w="bf16", o="f32", epi=0, act=0, a_act=0, rms=0, gamma=0, bias=0, colscale=0, a_index=0,
                snake=0, out2=0, conv=None, splitk=0, ws_bytes=16 << 20, a_misalign=0, lda=None, null=None)


def digest(t):
    import torch
    return hashlib.sha256(t.contiguous().view(torch.uint8).cpu().numpy().tobytes()).hexdigest()


def run_entry(K, torch, i, d):
    dev = "cuda"
    dt = {"f32": torch.float32, "bf16": torch.bfloat16}
    d = {**DEFAULTS, **d}
    torch.manual_seed(i)
    M, N, Kd = d["M"], d["N"], d["K"]
    adt, wdt, odt = dt[d["a"]], dt[d["w"]], dt[d["o"]]
    kw = dict(a_dtype=adt, o_dtype=odt, epi=d["epi"], act=d["act"], a_act=d["a_act"], rms=bool(d["rms"]),
              eps=1e-6, splitk=d["splitk"])
    bias = torch.randn(N, device=dev) * 0.1 if d["bias"] else None
    if d["conv"]:
        taps, dil, cin, cin_pad, t_in, t_out, t_off = d["conv"]
        w = torch.zeros(N, taps, cin_pad, device=dev)
        w[:, :, :cin] = torch.randn(N, taps, cin, device=dev) / (taps * cin) ** 0.5
        W = K.tile(w.reshape(N, taps * cin_pad), wdt, bias, taps=taps, cin=cin, cin_pad=cin_pad, K=Kd)
        rows, lda, nch = -(-M // t_out) * t_in, cin, cin
        kw["conv"] = (t_in, t_out, t_off, dil)
    else:
        W = K.tile(torch.randn(N, Kd, device=dev) / Kd ** 0.5, wdt, bias, K=Kd)
        rows, lda, nch = M, (Kd if d["lda"] is None else d["lda"]), Kd
    off = d["a_misalign"] // adt.itemsize
    A = (torch.randn(rows * lda + off, device=dev) * 0.5).to(adt)[off:]
    if d["a_index"]:
        kw["a_index"] = torch.randperm(M, device=dev).to(torch.int32)
    if d["gamma"]:
        kw["gamma"] = 1.0 + 0.1 * torch.randn(nch, device=dev)
    if d["colscale"]:
        kw["colscale"] = 0.5 + torch.rand(N, device=dev)
    if d["snake"]:
        kw["snake"] = (0.5 + torch.rand(nch, device=dev), 0.5 + torch.rand(nch, device=dev))
    ldo = N // 2 if d["epi"] == 2 else N
    out = (torch.randn(M, ldo, device=dev) * 0.5).to(odt)  # the residual of an accumulating epilogue
    if d["out2"]:
        kw["out2"] = torch.zeros(M, N, dtype=torch.bfloat16, device=dev)
    ws = torch.zeros(d["ws_bytes"], dtype=torch.uint8, device=dev) if d["ws_bytes"] else None
    with K.use_workspace(ws):
        K.gemm(A, W, out, M, lda, ldo, **kw)
    torch.cuda.synchronize()
    res = {"id": d["id"], "out": digest(out)}
    if d["out2"]:
        res["out2"] = digest(kw["out2"])
    return res


def run(fixture, dst):
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "qwen3-tts_amd"))
    import torch
    from qwen_tts import kernels as K
    with open(fixture) as f:
        cases = [c["args"] for c in json.load(f) if c["plan"][0] == 0]  # plan[0]: qt_gemm's return code
    res = [run_entry(K, torch, i, d) for i, d in enumerate(cases)]
    with open(dst, "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(r) for r in res) + "\n]\n")
    print(f"{len(res)} calls -> {dst}")


def kernels(trace, dst):
    rows = sorted(csv.DictReader(open(trace)), key=lambda r: int(r["Start_Timestamp"]))  # one stream, synchronised
    out = []
    for r in rows:
        name = r["Kernel_Name"].replace("void ", "").replace("(anonymous namespace)::", "")
        name = re.sub(r"\(qt_gemm_impl::GemmP.*$", "", name)
        if not name.startswith(GEMM_KERNELS):
            continue
        name = re.sub(r"^(igemm_k<.*), true>$", r"\1>", name)  # trees that still carry igemm_k's wave-grid flag
        out.append([name, [int(r[f"Grid_Size_{a}"]) for a in "XYZ"], [int(r[f"Workgroup_Size_{a}"]) for a in "XYZ"],
                    int(r["LDS_Block_Size"])])
    with open(dst, "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(r) for r in out) + "\n]\n")
    print(f"{len(out)} qt_gemm launches -> {dst}")


def diff(a, b):
    x, y = json.load(open(a)), json.load(open(b))
    bad = [i for i in range(max(len(x), len(y))) if i >= len(x) or i >= len(y) or x[i] != y[i]]
    if not bad:
        print(f"identical: {len(x)} entries ({a} vs {b})")
        return 0
    print(f"{len(bad)} of {max(len(x), len(y))} entries differ ({a} vs {b}); first: " +
          "; ".join(f"#{i} {x[i] if i < len(x) else None} != {y[i] if i < len(y) else None}" for i in bad[:3]))
    return 1


def summary(launches, digests):
    import collections
    x, y = json.load(open(launches)), json.load(open(digests))
    sha = lambda v: hashlib.sha256(json.dumps(v, sort_keys=True).encode()).hexdigest()  # noqa: E731
    print(f"{len(x)} qt_gemm launches in order [kernel, grid, workgroup, LDS bytes]: sha256 {sha(x)}")
    print(f"{len(y)} calls' output digests in order [id, out, out2]: sha256 {sha(y)}")
    for name, n in sorted(collections.Counter(r[0] for r in x).items()):
        print(f"{n:4d} {name}")


if __name__ == "__main__":
    mode = {"run": run, "kernels": kernels, "diff": diff, "summary": summary}.get(sys.argv[1] if len(sys.argv) == 4 else "")
    if mode is None:
        sys.exit(__doc__)
    sys.exit(mode(sys.argv[2], sys.argv[3]) or 0)
