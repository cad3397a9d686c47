"""Stand-alone times of the node-level GEMMs of a training step (fc0, the distance bank, their backward) through the C ABI:
pn_linear_forward / pn_gemm_f32 / pn_linear_backward at the headline (Cora) and Pubmed shapes, HIP events around blocks of
launches.  Used for the A/Bs of gemm_kernel variants in round 6 (the 32 x 32-tile bf16 x 3 kernel, the split-K target, two K
tiles in flight: profiles/r06_node_gemm.txt, r06_glue.txt sections 16-17), run against two builds of the library
(PN_LIB_PATH).   python tools/bench_node_gemm.py [reps]

    python tools/bench_node_gemm.py sparse [steps]
fc0 over prepared sparse features against the dense kernels (profiles/sparse_fc0.txt: the density threshold): the fc0 and
fc0_bwd stages of a training step, bracketed one by one (pn_profile_configure mode 1: stages back to back on one stream), with
module.sparse_features "never" and "always" at F = 1433 (N = 2708) and F = 500 (N = 19717) over a range of densities."""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pathnet_amd import _lib  # noqa: E402


def timed(fn, reps):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    best = []
    for _ in range(5):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        best.append(a.elapsed_time(b) * 1000.0 / reps)
    best.sort()
    return round(best[len(best) // 2], 2)


def stage_ms(lib, ctx, fn, steps):
    """{stage name: ms per call} of `steps` calls of fn with every stage bracketed"""
    import ctypes
    n = lib.pn_profile_stage_count()
    names = [lib.pn_profile_stage_name(i).decode() for i in range(n)]
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    _lib.check(lib.pn_profile_configure(ctx, 1, 0))
    for _ in range(steps):
        fn()
    ms, cnt = (ctypes.c_double * n)(), (ctypes.c_int64 * n)()
    _lib.check(lib.pn_profile_read(ctx, ms, cnt))
    _lib.check(lib.pn_profile_configure(ctx, 0, 0))
    return {names[i]: ms[i] / cnt[i] for i in range(n) if cnt[i]}


def sparse_table(steps):
    import pathnet_amd
    lib = _lib.load()
    ctx = _lib.context("cuda")
    H, C, L, S, W = 128, 7, 4, 256, 8
    out = {}
    for F, N in ((1433, 2708), (500, 19717)):
        torch.manual_seed(F)
        m = pathnet_amd.PathNet_homo(F, H, C, L, dropout=0.5).cuda().train()
        m.range_guard = False
        ids = torch.randint(0, N, (S, W * L), dtype=torch.int32, device="cuda")
        sel = torch.arange(S, dtype=torch.int32, device="cuda")
        ids[:, 0::L] = sel[:, None]
        codes = torch.randint(0, L, (S, W, L), dtype=torch.uint8, device="cuda")
        y = torch.randint(0, C, (S,), device="cuda")
        for density in (0.005, 0.013, 0.02, 0.03, 0.06, 0.12):
            X = ((torch.rand(N, F, device="cuda") < density).float() * torch.rand(N, F, device="cuda")).contiguous()
            row = {}
            for mode in ("never", "always"):
                m.sparse_features = mode

                def step():
                    m.zero_grad(set_to_none=True)
                    loss, _ = m.forward_loss(X, ids, W, L, sel, codes, y, fused=True)
                    loss.backward()
                st = stage_ms(lib, ctx, step, steps)
                row[mode] = {"fc0_us": round(st["fc0"] * 1e3, 2), "fc0_bwd_us": round(st["fc0_bwd"] * 1e3, 2)}
            row["ratio_fwd"] = round(row["always"]["fc0_us"] / row["never"]["fc0_us"], 3)
            row["ratio_bwd"] = round(row["always"]["fc0_bwd_us"] / row["never"]["fc0_bwd_us"], 3)
            out["F%d_d%g" % (F, density)] = row
            print("F=%d N=%d density %.3f  %s" % (F, N, density, json.dumps(row)), flush=True)
    print("RESULT " + json.dumps(out))


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "sparse":
        return sparse_table(int(sys.argv[2]) if len(sys.argv) > 2 else 20)
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 200
    lib = _lib.load()
    ctx = _lib.context("cuda")
    out = {}
    for name, (N, F, H, L) in {"cora": (2708, 1433, 128, 4), "pubmed": (19717, 500, 128, 4)}.items():
        torch.manual_seed(0)
        X = torch.randn(N, F, device="cuda")
        W0 = torch.randn(H, F, device="cuda") / F ** 0.5
        b0 = torch.randn(H, device="cuda")
        Wb = torch.randn(L * H, H, device="cuda") / H ** 0.5
        bb = torch.randn(L * H, device="cuda")
        Xh = torch.empty(N, H, device="cuda")
        Z = torch.empty(N, L * H, device="cuda")
        dZ = torch.randn(N, L * H, device="cuda")
        dXh = torch.empty(N, H, device="cuda")
        gW0, gb0 = torch.empty_like(W0), torch.empty_like(b0)
        gWb, gbb = torch.empty_like(Wb), torch.empty_like(bb)
        ws = torch.empty(_lib.LINEAR_SPLIT_MAX * N * max(H, 1), device="cuda")
        s = torch.cuda.current_stream().cuda_stream
        r = {}
        r["fc0_fwd"] = timed(lambda: _lib.check(lib.pn_linear_forward(ctx, X.data_ptr(), W0.data_ptr(), b0.data_ptr(), N, F, H, 1,
                                                                       Xh.data_ptr(), ws.data_ptr(), ws.numel() * 4, s)), reps)
        r["bank_fwd"] = timed(lambda: _lib.check(lib.pn_gemm_f32(Xh.data_ptr(), H, 1, Wb.data_ptr(), H, 1, Z.data_ptr(), L * H,
                                                                  bb.data_ptr(), N, L * H, H, 1, s)), reps)
        # bank backward as a linear layer in = H, out = L H: g_X = dZ' . Wb, g_W = dZ'^T . Xh, g_b
        r["bank_bwd_dx"] = timed(lambda: _lib.check(lib.pn_linear_backward(ctx, dZ.data_ptr(), Z.data_ptr(), None, Wb.data_ptr(), N, H, L * H,
                                                                            None, None, dXh.data_ptr(), None, 0, s)), reps)
        r["bank_bwd_dw"] = timed(lambda: _lib.check(lib.pn_linear_backward(ctx, dZ.data_ptr(), Z.data_ptr(), Xh.data_ptr(), None, N, H, L * H,
                                                                            gWb.data_ptr(), gbb.data_ptr(), None, None, 0, s)), reps)
        r["fc0_bwd_dw"] = timed(lambda: _lib.check(lib.pn_linear_backward(ctx, dXh.data_ptr(), Xh.data_ptr(), X.data_ptr(), None, N, F, H,
                                                                           gW0.data_ptr(), gb0.data_ptr(), None, None, 0, s)), reps)
        # values, against float64
        ref = torch.relu(X.double() @ W0.double().t() + b0.double())
        r["fc0_fwd_err"] = float((Xh.double() - ref).abs().max())
        d = dXh.double() * (Xh > 0)
        r["fc0_bwd_dw_relerr"] = float((gW0.double() - d.t() @ X.double()).abs().max() / (d.t() @ X.double()).abs().max())
        out[name] = r
    print("RESULT " + json.dumps(out))


if __name__ == "__main__":
    main()
