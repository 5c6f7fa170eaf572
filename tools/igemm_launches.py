"""Every entry point of csrc/conv_igemm.hip once over the case tables of tests/igemm_ref.py, at automatic tile selection: the sha256 of each
output goes to a JSON file.  Two builds of the library that make the same launches give the same file, and under
`rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/igemm_launches.py ...` the same kernel sequence.

    python tools/igemm_launches.py --lib path/to/librunet_hip.so --out hashes.json
    python tools/igemm_launches.py --diff-traces DIR_A DIR_B          # (kernel, grid, workgroup, LDS bytes) sequences of two traces, the HIP runtime's copy kernels aside

Used to check a host-side restructuring of the launchers against the build before it."""
import argparse
import csv
import glob
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = "eusipco-2026-robust-unet_amd"


def trace_rows(d):
    files = sorted(glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True))
    assert len(files) == 1, (d, files)
    rows = sorted(csv.DictReader(open(files[0])), key=lambda r: int(r["Start_Timestamp"]))
    dims = lambda r, k: tuple(int(r[f"{k}_{a}"]) for a in "XYZ")
    return [(r["Kernel_Name"].replace("(anonymous namespace)::", ""), dims(r, "Grid_Size"), dims(r, "Workgroup_Size"), int(r["LDS_Block_Size"])) for r in rows]


def diff_traces(a, b):
    """The HIP runtime's own copy kernels (__amd_rocclr_*) are left out: whether a host <-> device copy goes through one is the runtime's
    choice, copy by copy, and differs between two runs of the same library."""
    ra, rb = trace_rows(a), trace_rows(b)
    print(f"left out: {sum(r[0].startswith('__amd_rocclr_') for r in ra)} / {sum(r[0].startswith('__amd_rocclr_') for r in rb)} copy kernels of the HIP runtime")
    ra, rb = ([r for r in rows if not r[0].startswith("__amd_rocclr_")] for rows in (ra, rb))
    ours = lambda rows: sum(1 for r in rows if any(k in r[0] for k in ("igemm_kernel", "wgrad", "slab_reduce", "transpose_taps", "gemm_nn", "gemm_tn")))
    print(f"{a}: {len(ra)} launches ({ours(ra)} of the library's GEMM kernels)\n{b}: {len(rb)} launches ({ours(rb)})")
    bad = [(i, x, y) for i, (x, y) in enumerate(zip(ra, rb)) if x != y]
    for i, x, y in bad[:20]:
        print(f"launch {i} differs:\n  {x}\n  {y}")
    same = len(ra) == len(rb) and not bad
    print("same sequence of (kernel, grid, workgroup, LDS bytes)" if same else f"DIFFERENT: {len(bad)} launches differ, lengths {len(ra)} / {len(rb)}")
    return 0 if same else 1


def run(lib_path, out_path):
    os.environ["RUNET_HIP_LIB"] = os.path.abspath(lib_path)
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
    import importlib
    import torch
    import igemm_ref as R
    m = importlib.import_module(PKG + "._lib")
    lib, check = m.lib, m.check
    dev = torch.device("cuda:0")
    st = lambda: torch.cuda.current_stream().cuda_stream
    hashes = {}

    def put(key, t):
        assert key not in hashes, key
        torch.cuda.synchronize()
        hashes[key] = hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()

    def ptr(t):
        return t.data_ptr() if t is not None else None

    mode = {"conv": R.FWD, "conv_dgrad": R.DGRAD, "convt2": R.CONVT_FWD, "convt2_dgrad": R.CONVT_DGRAD, "gconv": R.FWD, "gconv_dgrad": R.DGRAD,
            "convt4": R.CONVT_FWD, "convt4_dgrad": R.CONVT_DGRAD}

    # ---- forward and data gradient: without bias into NaN, with bias on top of `old`
    for c in R.igemm_cases() + R.general_cases():
        p = R.op_problem(c)
        x, w, b = p.x.to(dev), p.w.to(dev), p.bias.to(dev)
        wt = None
        if c.kind in ("conv_dgrad", "convt2_dgrad"):      # the _T modes read the per-tap transposed weight
            wt = torch.empty(c.k * c.k, c.cin, c.cout, device=dev)
            check(lib.runet_transpose_taps(ptr(w), ptr(wt), c.k * c.k, c.cout, c.cin, st()))
            put(f"transpose_taps/{c.id}", wt)
        for bias, acc in ((None, 0), (b, 1)):
            tag = f"{c.id}/b{int(bias is not None)}a{acc}"
            new = lambda: p.old.to(dev).clone() if acc else torch.full((c.n,) + p.dst_hw + (c.cout,), float("nan"), device=dev)
            if c.kind in ("conv", "conv_dgrad", "convt2", "convt2_dgrad"):
                y = new()
                check(lib.runet_conv_igemm(ptr(x), c.cin, ptr(w), ptr(bias), ptr(y), c.cout, c.n, c.h, c.w, c.cin, c.cin_w, c.cout, c.k, c.k, c.dil, mode[c.kind],
                                           acc, st()))
                put("conv_igemm/" + tag, y)
                if wt is not None:
                    y = new()
                    mt = R.DGRAD_T if c.kind == "conv_dgrad" else R.CONVT_DGRAD_T
                    check(lib.runet_conv_igemm(ptr(x), c.cin, ptr(wt), ptr(bias), ptr(y), c.cout, c.n, c.h, c.w, c.cin, c.cin_w, c.cout, c.k, c.k, c.dil, mt, acc, st()))
                    put("conv_igemm_T/" + tag, y)
            elif c.kind in ("gconv", "gconv_dgrad"):
                y = new()
                check(lib.runet_conv2d_general(ptr(x), c.cin, ptr(w), ptr(bias), ptr(y), c.cout, c.n, c.h, c.w, c.cin, c.cin_w, c.cout, c.k, c.k, c.stride, c.pad,
                                               c.dil, mode[c.kind], acc, st()))
                put("conv2d_general/" + tag, y)
                y = new()
                check(lib.runet_conv2d_rect(ptr(x), c.cin, ptr(w), ptr(bias), ptr(y), c.cout, c.n, c.h, c.w, c.cin, c.cin_w, c.cout, c.k, c.k, c.stride, c.pad, c.pad,
                                            c.dil, c.dil, mode[c.kind], acc, st()))
                put("conv2d_rect/" + tag, y)
            else:
                y = new()
                check(lib.runet_convt4_igemm(ptr(x), c.cin, ptr(w), ptr(bias), ptr(y), c.cout, c.n, c.h, c.w, c.cin, c.cout, mode[c.kind], acc, st()))
                put("convt4_igemm/" + tag, y)
        if c.kind == "convt4":
            y = torch.full((c.n,) + p.dst_hw + (c.cout,), float("nan"), device=dev)
            stats = torch.full((lib.runet_convt4_igemm_stats_parts(c.n, c.h, c.w, c.cout), c.cout, 3), float("nan"), device=dev)
            check(lib.runet_convt4_igemm_stats(ptr(x), c.cin, ptr(w), ptr(b), ptr(y), c.cout, c.n, c.h, c.w, c.cin, c.cout, ptr(stats), st()))
            put(f"convt4_igemm_stats/{c.id}/y", y)
            put(f"convt4_igemm_stats/{c.id}/stats", stats)
            wq, y = torch.empty(9, c.cin, c.cout, device=dev), torch.full((c.n,) + p.dst_hw + (c.cout,), float("nan"), device=dev)
            w9 = R.randn((9, c.cin, c.cout), 77 + c.cin, 0.1).to(dev)
            check(lib.runet_convt3_pack(ptr(w9), ptr(wq), c.cin, c.cout, st()))
            check(lib.runet_convt3_fwd(ptr(x), c.cin, ptr(wq), ptr(b), ptr(y), c.cout, c.n, c.h, c.w, c.cin, c.cout, st()))
            put(f"convt3_fwd/{c.id}", y)

    # ---- rectangular kernels (ENet's asymmetric bottleneck) and the weight gradients of the general geometries
    for kh, kw, ph, pw in ((5, 1, 2, 0), (1, 5, 0, 2)):
        n, h, wd, cin, cout = 3, 9, 11, 20, 36
        x, dy = R.randn((n, h, wd, cin), 501).to(dev), R.randn((n, h, wd, cout), 502).to(dev)
        w = R.randn((kh, kw, cin, cout), 503, 0.1).to(dev)
        y, dx = torch.empty(n, h, wd, cout, device=dev), torch.empty(n, h, wd, cin, device=dev)
        check(lib.runet_conv2d_rect(ptr(x), cin, ptr(w), None, ptr(y), cout, n, h, wd, cin, cin, cout, kh, kw, 1, ph, pw, 1, 1, R.FWD, 0, st()))
        put(f"conv2d_rect/{kh}x{kw}/fwd", y)
        check(lib.runet_conv2d_rect(ptr(dy), cout, ptr(w), None, ptr(dx), cin, n, h, wd, cout, cout, cin, kh, kw, 1, ph, pw, 1, 1, R.DGRAD, 0, st()))
        put(f"conv2d_rect/{kh}x{kw}/dgrad", dx)
        floats = lib.runet_conv_wgrad_rect_workspace_floats(n * h * wd, cin, cout, kh, kw)
        ws, dw = torch.empty(max(floats, 4), device=dev), torch.empty(kh * kw, cin, cout, device=dev)
        check(lib.runet_conv_wgrad_rect(ptr(x), cin, ptr(dy), cout, ptr(dw), ptr(ws), floats, n, h, wd, cin, cin, cout, kh, kw, 1, ph, pw, 1, 1, st()))
        put(f"conv_wgrad_rect/{kh}x{kw}", dw)
    for c in R.general_cases():
        if c.kind not in ("gconv", "convt4"):
            continue
        p = R.op_problem(c)
        x, dy = p.x.to(dev), p.old.to(dev)      # `old` has the output's shape: it stands in for dy
        tr4 = int(c.kind == "convt4")
        pixels = c.n * (c.h * c.w if tr4 else p.dst_hw[0] * p.dst_hw[1])
        for name, fn_ws in (("general", lib.runet_conv_wgrad_general_workspace_floats), ("rect", lib.runet_conv_wgrad_rect_workspace_floats)):
            if tr4 and name == "rect":
                continue
            floats = fn_ws(pixels, c.cin_w, c.cout, c.k, c.k)
            ws, dw = torch.empty(max(floats, 4), device=dev), torch.empty(c.k * c.k, c.cin_w, c.cout, device=dev)
            if name == "general":
                check(lib.runet_conv_wgrad_general(ptr(x), c.cin, ptr(dy), c.cout, ptr(dw), ptr(ws), floats, c.n, c.h, c.w, c.cin, c.cin_w, c.cout, c.k, c.k, c.stride,
                                                   c.pad, c.dil, tr4, st()))
            else:
                check(lib.runet_conv_wgrad_rect(ptr(x), c.cin, ptr(dy), c.cout, ptr(dw), ptr(ws), floats, c.n, c.h, c.w, c.cin, c.cin_w, c.cout, c.k, c.k, c.stride,
                                                c.pad, c.pad, c.dil, c.dil, st()))
            put(f"conv_wgrad_{name}/{c.id}", dw)
        dw = torch.empty(c.k * c.k, c.cin_w, c.cout, device=dev)      # no workspace: one split
        check(lib.runet_conv_wgrad_general(ptr(x), c.cin, ptr(dy), c.cout, ptr(dw), None, 0, c.n, c.h, c.w, c.cin, c.cin_w, c.cout, c.k, c.k, c.stride, c.pad, c.dil,
                                           tr4, st()))
        put(f"conv_wgrad_general/{c.id}/no-workspace", dw)

    # ---- runet_conv_wgrad: every route, with the workspace it asks for and with none (one slab) where the route allows
    for c in R.wgrad_cases():
        p = R.wgrad_problem(c)
        x, dy = p.x.to(dev), p.dy.to(dev)
        floats = lib.runet_conv_wgrad_workspace_floats(c.n, c.h, c.w, c.cin_w, c.cout, c.k, c.k)
        for tag, fl in (("ws", floats), ("ws-one-slab", c.k * c.k * c.cin_w * c.cout)):
            ws, dw = torch.empty(max(fl, 4), device=dev), torch.full((c.k * c.k, c.cin_w, c.cout), float("nan"), device=dev)
            check(lib.runet_conv_wgrad(ptr(x), c.cin, ptr(dy), c.cout, ptr(dw), ptr(ws), fl, c.n, c.h, c.w, c.cin, c.cin_w, c.cout, c.k, c.k, c.dil, c.tr, st()))
            put(f"conv_wgrad/{c.id}/{tag}", dw)

    # ---- the batched GEMMs
    for c in R.gemm_cases():
        a, b = R.randn((c.batch, c.rows, c.k), 600 + c.n).to(dev), R.randn((c.batch, c.k, c.n), 601 + c.k, 0.1).to(dev)
        out = torch.full((c.batch, c.rows, c.n), float("nan"), device=dev)
        check(lib.runet_gemm_batched(ptr(a), c.k, c.rows * c.k, ptr(b), c.k * c.n, ptr(out), c.n, c.rows * c.n, c.batch, c.rows, c.k, c.n, st()))
        put(f"gemm_batched/{c.id}/{lib.runet_gemm_batched_kernel_name(c.batch, c.rows, c.k, c.n).decode()}", out)
    for rows in R.TN_ROWS:
        for k in R.TN_KN:
            for n in R.TN_KN:
                a, b = R.randn((R.TN_BATCH, rows, k), 700 + k).to(dev), R.randn((R.TN_BATCH, rows, n), 701 + n).to(dev)
                out = torch.full(((rows + R.TN_RPS - 1) // R.TN_RPS, R.TN_BATCH, k, n), float("nan"), device=dev)
                check(lib.runet_gemm_tn_batched(ptr(a), k, rows * k, ptr(b), n, rows * n, ptr(out), R.TN_BATCH, rows, k, n, R.TN_RPS, st()))
                put(f"gemm_tn_batched/{rows}x{k}x{n}", out)

    torch.cuda.synchronize()
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(hashes, f, indent=1, sort_keys=True)
    print(f"{len(hashes)} outputs hashed -> {out_path} (library {m.LIB_PATH})")
    return 0


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--lib", help="librunet_hip.so to run")
    ap.add_argument("--out", help="JSON file of the output hashes")
    ap.add_argument("--diff-traces", nargs=2, metavar="DIR")
    a = ap.parse_args()
    if a.diff_traces:
        return diff_traces(*a.diff_traces)
    assert a.lib and a.out, "--lib and --out"
    return run(a.lib, a.out)


if __name__ == "__main__":
    sys.exit(main())
