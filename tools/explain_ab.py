"""What an explanation costs: the headline shape (bench.workload: 2708 nodes, 1299 masked, 40 paths of 4, H = 128, C = 7),
PathNet_homo in eval mode, groups="path", three legs in ONE process, alternating blocks, device events around each block:
  (a) encode(path_state=True) alone
  (b) model.explain(...)                         = (a) with PN_EVAL_ZW off + pn_explain_groups + pn_explain_totals
  (c) the same answers through the existing interface: the plain forward and a weighted forward per drop_g
      (W + 1 forwards; the keep_g half would double it and is not run)
and pn_explain_groups by itself on (a)'s tensors (launched back to back through the C entry point), with its achieved
bytes/s over S * W * H * 4.  In the same alternation, explanations by node and by edge:
  (d) model.explain(groups="node")  (e) model.explain(groups="edge")
and their kernels by themselves, ten launches a call: pn_explain_units and pn_explain_overlap for each kind (G = W * L = 160
and W * (L - 1) = 120 columns against the 40 of groups="path"), and pn_explain_node_totals.  Prints medians and spread
(half the range between the 10th and 90th percentile of the blocks) and one JSON line.  Needs a GPU: there is no fallback.
   python tools/explain_ab.py [--blocks 8] [--steps 10] [--warmup 3] [--out FILE]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=8)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None, help="append the report to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("explain_ab: needs a GPU")
    import bench
    import pathnet_amd
    import ctypes
    from pathnet_amd import _lib
    dev = torch.device("cuda:0")
    wl = bench.workload(0, 1)
    n, F, C, H, W, L = wl["n"], wl["F"], wl["C"], wl["H"], wl["W"], wl["L"]
    gn, u, v, p = wl["graph"]
    smp = pathnet_amd.MerwSampler(gn, u, v, p, L, device=dev)
    torch.manual_seed(0)
    model = pathnet_amd.PathNet_homo(F, H, C, L).to(dev).eval()
    X = torch.from_numpy(wl["X"]).to(dev)
    sel = torch.from_numpy(np.flatnonzero(wl["mask"]).astype(np.int32)).to(dev)
    S = int(sel.numel())
    ids, codes = smp.sample(W, 1234, epoch_count=1, nodes=sel, draw_source=pathnet_amd.DRAW_PHILOX, check=False)
    ids, codes = ids[0], codes[0]
    drop = [torch.ones(S, W, device=dev) for _ in range(W)]
    for g in range(W):
        drop[g][:, g] = 0.0
    group = torch.arange(W, dtype=torch.int32, device=dev).repeat(S, 1)
    with torch.no_grad():
        enc = model.encode(X, ids, W, L, sel, codes, path_state=True)

    def leg_encode():
        return model.encode(X, ids, W, L, sel, codes, path_state=True).logits

    def leg_explain():
        return model.explain(X, ids, W, L, sel, codes, groups="path").drop_delta

    def leg_forwards():
        out = model(X, ids, W, L, sel, codes)
        for g in range(W):
            out = model(X, ids, W, L, sel, codes, reuse_tables=True, path_weights=drop[g])
        return out

    # the kernel by itself: outputs allocated once, the C entry point called directly (a host call of a few microseconds)
    f = torch.empty((2, S, W), dtype=torch.float32, device=dev)
    flip = torch.empty((S, W), dtype=torch.uint8, device=dev)
    present = torch.empty((S, W), dtype=torch.int32, device=dev)
    tused = torch.empty(S, dtype=torch.int64, device=dev)
    desc = _lib.ExplainOut(drop_delta=f[0].data_ptr(), keep_gain=f[1].data_ptr(), flip=flip.data_ptr(),
                           present=present.data_ptr(), target_used=tused.data_ptr())
    lib, ctx, stream = _lib.load(), _lib.context(dev), _lib.stream_ptr(dev)
    state, coef, emb = enc.path_state.contiguous(), enc.path_weight.contiguous(), enc.embedding.contiguous()
    fw, fb = model.fc2.weight.detach().contiguous(), model.fc2.bias.detach().contiguous()

    def leg_kernel():
        for _ in range(10):
            _lib.check(lib.pn_explain_groups(ctx, S, W, H, C, W, _lib.ptr(state), H, _lib.ptr(coef), _lib.ptr(emb), 2 * H,
                                             _lib.ptr(fw), 2 * H, _lib.ptr(fb), None, _lib.ptr(group), _lib.PATH_NORM_SUM, 0, None,
                                             ctypes.byref(desc), None, stream))
        return f[0]

    # ---- by node and by edge: the public call, and each new kernel by itself on tensors made once --------------------------
    ex = sys.modules["pathnet_amd.explain"]
    node = pathnet_amd.member_nodes("homo", ids, S, W, L)
    unit_legs = {}
    for kind in ("node", "edge"):
        unit, count, label = pathnet_amd.explain_units(node, kind, sel if kind == "node" else None)
        M, G = int(label.shape[2]), int(unit.shape[1])
        fk = torch.empty((2, S, G), dtype=torch.float32, device=dev)
        flk = torch.empty((S, G), dtype=torch.uint8, device=dev)
        prk = torch.empty((S, G), dtype=torch.int32, device=dev)
        dk = _lib.ExplainOut(drop_delta=fk[0].data_ptr(), keep_gain=fk[1].data_ptr(), flip=flk.data_ptr(),
                             present=prk.data_ptr(), target_used=tused.data_ptr())
        keep = (unit, count, label, fk, flk, prk, dk)          # (alive for the closures)

        def leg_units(kind=kind, keep=keep):
            unit, count, label = keep[:3]
            for _ in range(10):
                _lib.check(lib.pn_explain_units(ctx, S, W, L, ex.UNIT_KINDS[kind], _lib.ptr(node),
                                                _lib.ptr(sel) if kind == "node" else None, _lib.ptr(unit), _lib.ptr(count),
                                                _lib.ptr(label), stream))
            return count.float()

        def leg_overlap(keep=keep, M=M, G=G):
            label, fk, dk = keep[2], keep[3], keep[6]
            for _ in range(10):
                _lib.check(lib.pn_explain_overlap(ctx, S, W, H, C, G, M, _lib.ptr(state), H, _lib.ptr(coef), _lib.ptr(emb), 2 * H,
                                                  _lib.ptr(fw), 2 * H, _lib.ptr(fb), None, _lib.ptr(label), _lib.PATH_NORM_SUM, 0,
                                                  None, ctypes.byref(dk), None, stream))
            return fk[0]

        def leg_public(kind=kind):
            return model.explain(X, ids, W, L, sel, codes, groups=kind).drop_delta
        unit_legs["explain_" + kind] = (leg_public, args.steps)
        unit_legs["units_" + kind] = (leg_units, args.steps)
        unit_legs["overlap_" + kind] = (leg_overlap, args.steps)
        if kind == "node":
            table = torch.zeros((4, n), dtype=torch.int64, device=dev)

            def leg_node_totals(keep=keep, G=G):
                unit, fk, flk, prk = keep[0], keep[3], keep[4], keep[5]
                for _ in range(10):
                    _lib.check(lib.pn_explain_node_totals(ctx, S, G, n, _lib.ptr(unit), _lib.ptr(fk[0]), _lib.ptr(fk[1]),
                                                          _lib.ptr(flk), _lib.ptr(prk), None, 0, _lib.ptr(table), stream))
                return table[0].float()
            unit_legs["node_totals"] = (leg_node_totals, args.steps)
    ten = {"kernel", "units_node", "units_edge", "overlap_node", "overlap_edge", "node_totals"}      # ten launches per call

    legs = {"encode": (leg_encode, args.steps), "explain": (leg_explain, args.steps),
            "forwards": (leg_forwards, max(1, args.steps // 5)), "kernel": (leg_kernel, args.steps)}
    legs.update(unit_legs)
    times = {k: [] for k in legs}
    with torch.no_grad():
        for name, (fn, _) in legs.items():
            for _ in range(args.warmup):
                last = fn()
            torch.cuda.synchronize()
            assert torch.isfinite(last).all().item(), name
        for _ in range(args.blocks):
            for name, (fn, steps) in legs.items():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(steps):
                    fn()
                b.record()
                b.synchronize()
                times[name].append(a.elapsed_time(b) / steps)
    rec = {"shape": dict(n=n, S=S, F=F, H=H, C=C, W=W, L=L, groups="path"), "blocks": args.blocks}
    lines = []
    for name, t in times.items():
        t = np.asarray(t)
        if name in ten:
            t = t / 10          # ten launches per call
        rec[name] = {"median_ms": float(np.median(t)), "spread_ms": float((np.percentile(t, 90) - np.percentile(t, 10)) / 2),
                     "min_ms": float(t.min()), "max_ms": float(t.max())}
        lines.append("%-14s median %.4f ms  spread +-%.4f  (min %.4f max %.4f) over %d blocks of %d calls"
                     % (name, rec[name]["median_ms"], rec[name]["spread_ms"], t.min(), t.max(), args.blocks, legs[name][1]))
    state_bytes = S * W * H * 4
    rec["state_bytes"] = state_bytes
    rec["kernel_gb_per_s"] = state_bytes / (rec["kernel"]["median_ms"] * 1e-3) / 1e9
    rec["explain_over_encode"] = rec["explain"]["median_ms"] / rec["encode"]["median_ms"]
    rec["forwards_over_explain"] = rec["forwards"]["median_ms"] / rec["explain"]["median_ms"]
    lines.append("kernel leg (pn_explain_groups alone, back to back): %.1f GB/s over S*W*H*4 = %.1f MB"
                 % (rec["kernel_gb_per_s"], state_bytes / 1e6))
    lines.append("explain / encode = %.3f   (W + 1 forwards) / explain = %.1f" % (rec["explain_over_encode"],
                                                                                 rec["forwards_over_explain"]))
    for kind, G in (("node", W * L), ("edge", W * (L - 1))):
        rec["overlap_%s_over_kernel" % kind] = rec["overlap_" + kind]["median_ms"] / rec["kernel"]["median_ms"]
        rec["explain_%s_over_explain" % kind] = rec["explain_" + kind]["median_ms"] / rec["explain"]["median_ms"]
        lines.append("groups=%r: pn_explain_overlap / pn_explain_groups = %.2f at (2 G + 2) = %d against %d vectors;  "
                     "explain(%s) / explain(path) = %.2f" % (kind, rec["overlap_%s_over_kernel" % kind], 2 * G + 2, 2 * W + 2,
                                                             kind, rec["explain_%s_over_explain" % kind]))
    lines.append(json.dumps(rec))
    print("\n".join(lines))
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
