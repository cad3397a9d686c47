"""What the loss options cost: the headline-shape fused training step (bench.workload: 2708 nodes, 1299 masked, 40 paths of
4, H = 128) through module.forward_loss(fused=True) + backward, with loss=None and with class weights + ignore_index +
label smoothing, in ONE process, alternating blocks, device events around each block.  Prints medians and spread (half the
range between the 10th and 90th percentile of the blocks) and one JSON line.  Needs a GPU: there is no fallback.
   python tools/loss_options_ab.py [--blocks 12] [--steps 20] [--warmup 10]"""
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
        raise SystemExit("loss_options_ab: needs a GPU")
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
    Yi = Y.clone()
    Yi[torch.arange(0, S, 5, device=dev)] = -1          # a fifth of the rows unlabelled
    weight = pathnet_amd.balanced_class_weight(Yi, C, ignore_index=-1)
    opts = pathnet_amd.CrossEntropyLoss(weight=weight, ignore_index=-1, label_smoothing=0.1)

    def step(loss_fn, target):
        model.zero_grad(set_to_none=True)
        loss, _ = model.forward_loss(X, ids, W, L, sel, codes, target, fused=True, loss=loss_fn)
        pathnet_amd.backward(loss)
        return loss

    variants = {"plain": (None, Y), "options": (opts, Yi)}
    for name, (fn, tgt) in variants.items():
        for _ in range(args.warmup):
            last = step(fn, tgt)
        torch.cuda.synchronize()
        assert torch.isfinite(last).item(), name
    times = {k: [] for k in variants}
    for _ in range(args.blocks):
        for name, (fn, tgt) in variants.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(args.steps):
                step(fn, tgt)
            b.record()
            b.synchronize()
            times[name].append(a.elapsed_time(b) / args.steps)
    rec = {"shape": dict(n=n, S=S, F=F, H=H, C=C, W=W, L=L), "blocks": args.blocks, "steps_per_block": args.steps}
    for name, t in times.items():
        t = np.asarray(t)
        rec[name] = {"median_ms": float(np.median(t)), "spread_ms": float((np.percentile(t, 90) - np.percentile(t, 10)) / 2),
                     "min_ms": float(t.min()), "max_ms": float(t.max())}
        print("%-8s median %.4f ms  spread +-%.4f  (min %.4f max %.4f) over %d blocks of %d steps"
              % (name, rec[name]["median_ms"], rec[name]["spread_ms"], t.min(), t.max(), args.blocks, args.steps))
    rec["options_minus_plain_ms"] = rec["options"]["median_ms"] - rec["plain"]["median_ms"]
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
