"""What the gradients at the per-path interface cost: the headline shape (bench.workload: 2708 nodes, 1299 masked, 40 paths of
4, H = 128, C = 7), PathNet_homo in training mode without dropout, five legs in ONE process, alternating blocks, device events
around each block:
  (a) weighted forward + cross entropy + backward, the weights as data                  (pn_pagg_backward_weighted)
  (b) the same with path_grad=True and weights that require grad                        (pn_pagg_backward_paths: + d_omega)
  (c) the fused step forward_loss(fused=True), the weights as data                      (pn_pagg_train_step_weighted)
  (d) the same with path_grad=True and weights that require grad                        (pn_pagg_train_step_paths)
  (e) encode(path_state=True, path_grad=True) with a loss on all four outputs           (+ g_state [S, W, H], g_coef loads)
Prints medians and spread (half the range between the 10th and 90th percentile of the blocks) and one JSON line.  Needs a GPU:
there is no fallback.
   python tools/path_grads_ab.py [--blocks 8] [--steps 10] [--warmup 3] [--out FILE]"""
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
        raise SystemExit("path_grads_ab: needs a GPU")
    import bench
    import pathnet_amd
    dev = torch.device("cuda:0")
    wl = bench.workload(0, 1)
    n, F, C, H, W, L = wl["n"], wl["F"], wl["C"], wl["H"], wl["W"], wl["L"]
    gn, u, v, p = wl["graph"]
    smp = pathnet_amd.MerwSampler(gn, u, v, p, L, device=dev)
    torch.manual_seed(0)
    model = pathnet_amd.PathNet_homo(F, H, C, L, dropout=0.0).to(dev).train()
    X = torch.from_numpy(wl["X"]).to(dev)
    sel = torch.from_numpy(np.flatnonzero(wl["mask"]).astype(np.int32)).to(dev)
    S = int(sel.numel())
    ids, codes = smp.sample(W, 1234, epoch_count=1, nodes=sel, draw_source=pathnet_amd.DRAW_PHILOX, check=False)
    ids, codes = ids[0], codes[0]
    Y = torch.randint(0, C, (S,), device=dev)
    w_data = torch.rand(S, W, device=dev) + 0.5
    w_leaf = w_data.clone().requires_grad_(True)
    A, B, Cst = torch.randn(S, 2 * H, device=dev), torch.randn(S, W, device=dev), torch.randn(S, W, H, device=dev)
    ce = torch.nn.functional.cross_entropy

    def done(loss):
        model.zero_grad(set_to_none=True)
        w_leaf.grad = None
        loss.backward()
        return loss.detach()

    def leg_data():
        return done(ce(model(X, ids, W, L, sel, codes, path_weights=w_data), Y))

    def leg_grad():
        return done(ce(model(X, ids, W, L, sel, codes, path_weights=w_leaf, path_grad=True), Y))

    def leg_fused_data():
        return done(model.forward_loss(X, ids, W, L, sel, codes, Y, fused=True, path_weights=w_data)[0])

    def leg_fused_grad():
        return done(model.forward_loss(X, ids, W, L, sel, codes, Y, fused=True, path_weights=w_leaf, path_grad=True)[0])

    def leg_encode():
        enc = model.encode(X, ids, W, L, sel, codes, path_state=True, path_weights=w_leaf, path_grad=True)
        return done(ce(enc.logits, Y) + (A * enc.embedding).sum() + (B * enc.path_weight).sum() + (Cst * enc.path_state).sum())

    legs = {"data": leg_data, "path_grad": leg_grad, "fused_data": leg_fused_data, "fused_path_grad": leg_fused_grad,
            "encode_all_four": leg_encode}
    times = {k: [] for k in legs}
    for name, fn in legs.items():
        for _ in range(args.warmup):
            last = fn()
        torch.cuda.synchronize()
        assert torch.isfinite(last).all().item(), name
    for _ in range(args.blocks):
        for name, fn in legs.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(args.steps):
                fn()
            b.record()
            b.synchronize()
            times[name].append(a.elapsed_time(b) / args.steps)
    rec = {"shape": dict(n=n, S=S, F=F, H=H, C=C, W=W, L=L), "blocks": args.blocks, "steps": args.steps}
    lines = []
    for name, t in times.items():
        t = np.asarray(t)
        rec[name] = {"median_ms": float(np.median(t)), "spread_ms": float((np.percentile(t, 90) - np.percentile(t, 10)) / 2),
                     "min_ms": float(t.min()), "max_ms": float(t.max())}
        lines.append("%-16s median %.4f ms  spread +-%.4f  (min %.4f max %.4f) over %d blocks of %d calls"
                     % (name, rec[name]["median_ms"], rec[name]["spread_ms"], t.min(), t.max(), args.blocks, args.steps))
    rec["path_grad_over_data"] = rec["path_grad"]["median_ms"] / rec["data"]["median_ms"]
    rec["fused_path_grad_over_fused_data"] = rec["fused_path_grad"]["median_ms"] / rec["fused_data"]["median_ms"]
    rec["encode_all_four_over_data"] = rec["encode_all_four"]["median_ms"] / rec["data"]["median_ms"]
    lines.append("path_grad / data = %.3f   fused: %.3f   encode with all four upstreams / data = %.3f"
                 % (rec["path_grad_over_data"], rec["fused_path_grad_over_fused_data"], rec["encode_all_four_over_data"]))
    lines.append(json.dumps(rec))
    print("\n".join(lines))
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
