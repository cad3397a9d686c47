"""What per-path weights cost: the headline-shape fused training step (bench.workload: 2708 nodes, 1299 masked, 40 paths of
4, H = 128) through module.forward_loss(fused=True) + backward, without weights (the register-resident pooling step,
pool_step2_kernel) and with path_weights = the paths' multiplicities (the three pooling bodies in one launch,
pool_step_kernel<4>), in ONE process, alternating blocks, device events around each block.  Prints medians and spread (half
the range between the 10th and 90th percentile of the blocks) and one JSON line.  The difference says whether
pool_step2_kernel should carry the weights in registers.  Needs a GPU: there is no fallback.
   python tools/path_weights_ab.py [--blocks 12] [--steps 20] [--warmup 10]"""
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
    ap.add_argument("--blocks", type=int, default=12)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=10)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("path_weights_ab: needs a GPU")
    import bench
    import pathnet_amd
    dev = torch.device("cuda:0")
    wl = bench.workload(0, 1)
    n, F, C, H, W, L = wl["n"], wl["F"], wl["C"], wl["H"], wl["W"], wl["L"]
    gn, u, v, p = wl["graph"]
    smp = pathnet_amd.MerwSampler(gn, u, v, p, L, device=dev)
    torch.manual_seed(0)
    model = pathnet_amd.PathNet_homo(F, H, C, L, dropout=0.7).to(dev).train()
    X = torch.from_numpy(wl["X"]).to(dev)
    sel = torch.from_numpy(np.flatnonzero(wl["mask"]).astype(np.int32)).to(dev)
    S = int(sel.numel())
    Y = torch.from_numpy(wl["Y"]).to(dev)[sel.long()]
    ids, codes = smp.sample(W, 1234, epoch_count=1, nodes=sel, draw_source=pathnet_amd.DRAW_PHILOX, check=False)
    ids, codes = ids[0], codes[0]
    mult = pathnet_amd.path_multiplicity(ids, codes)

    def step(weights):
        model.zero_grad(set_to_none=True)
        loss, _ = model.forward_loss(X, ids, W, L, sel, codes, Y, fused=True, path_weights=weights)
        pathnet_amd.backward(loss)
        return loss

    variants = {"plain": None, "weighted": mult}
    for name, w in variants.items():
        for _ in range(args.warmup):
            last = step(w)
        torch.cuda.synchronize()
        assert torch.isfinite(last).item(), name
    times = {k: [] for k in variants}
    for _ in range(args.blocks):
        for name, w in variants.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(args.steps):
                step(w)
            b.record()
            b.synchronize()
            times[name].append(a.elapsed_time(b) / args.steps)
    rec = {"shape": dict(n=n, S=S, F=F, H=H, C=C, W=W, L=L), "blocks": args.blocks, "steps_per_block": args.steps,
           "dead_paths_share": float((mult == 0).float().mean())}
    for name, t in times.items():
        t = np.asarray(t)
        rec[name] = {"median_ms": float(np.median(t)), "spread_ms": float((np.percentile(t, 90) - np.percentile(t, 10)) / 2),
                     "min_ms": float(t.min()), "max_ms": float(t.max())}
        print("%-8s median %.4f ms  spread +-%.4f  (min %.4f max %.4f) over %d blocks of %d steps"
              % (name, rec[name]["median_ms"], rec[name]["spread_ms"], t.min(), t.max(), args.blocks, args.steps))
    rec["weighted_minus_plain_ms"] = rec["weighted"]["median_ms"] - rec["plain"]["median_ms"]
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
