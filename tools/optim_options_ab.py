"""What the optimizer's options cost on the step's tail: `StepState.advance(); opt.step()` captured into a graph at the
parameter set of the headline workload (bench.workload: PathNet_homo, F = 1433, H = 128, C = 7, L = 4), static gradient
buffers, with no option (pn_adam_step), with clipping, and with clipping + warm-up/cosine schedule + amsgrad -- in ONE
process, alternating blocks of replays, device events around each block.  Beside them, eagerly (not captured) and on the
same tensors: torch.nn.utils.clip_grad_norm_ + torch.optim.AdamW, and this library's clip + AdamW.  Prints medians and
spread (half the range between the 10th and 90th percentile of the blocks), writes them to --out, and ends with one JSON
line.  No pass/fail threshold.  Needs a GPU: there is no fallback.
   python tools/optim_options_ab.py [--blocks 12] [--steps 500] [--warmup 50] [--out profiles/optim_options.txt]"""
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
    ap.add_argument("--steps", type=int, default=500)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "optim_options.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("optim_options_ab: needs a GPU")
    import bench
    import pathnet_amd
    dev = torch.device("cuda:0")
    wl = bench.workload(0, 1)
    F, C, H, L = wl["F"], wl["C"], wl["H"], wl["L"]
    torch.manual_seed(0)
    model = pathnet_amd.PathNet_homo(F, H, C, L, dropout=0.7).to(dev)
    shapes = [tuple(p.shape) for p in model.parameters()]
    init = [p.detach().clone() for p in model.parameters()]
    gen = torch.Generator(device=dev).manual_seed(1)
    grads = [torch.randn(*s, generator=gen, device=dev) * 0.1 for s in shapes]
    sched = pathnet_amd.LRSchedule("cosine", warmup_steps=10, t_max=1000, lr_min=1e-5)

    def fresh():
        ps = [torch.nn.Parameter(p.clone()) for p in init]
        for p, g in zip(ps, grads):
            p.grad = g.clone()
        return ps

    captured = {"off": dict(), "clip": dict(max_grad_norm=1.0),
                "clip+schedule+amsgrad": dict(max_grad_norm=1.0, schedule=sched, amsgrad=True)}
    runs = {}
    for name, kw in captured.items():
        ps = fresh()
        st = pathnet_amd.StepState(dev, seed=1)
        opt = pathnet_amd.Adam(ps, lr=0.005, weight_decay=0.0005, step_state=st, **kw)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):       # step 1: creates the optimizer's state and its device buffer
            st.advance()
            opt.step()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            st.advance()
            opt.step()
        runs[name] = (graph.replay, (ps, st, opt, graph))

    tps = fresh()
    topt = torch.optim.AdamW(tps, lr=0.005, weight_decay=0.0005)

    def torch_eager():
        torch.nn.utils.clip_grad_norm_(tps, 1.0)
        topt.step()
    ops = fresh()
    oopt = pathnet_amd.AdamW(ops, lr=0.005, weight_decay=0.0005, max_grad_norm=1.0)
    runs["eager torch clip_grad_norm_ + AdamW"] = (torch_eager, None)
    runs["eager pathnet_amd.AdamW(max_grad_norm)"] = (oopt.step, None)

    for name, (fn, _) in runs.items():
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
    times = {k: [] for k in runs}
    for _ in range(args.blocks):
        for name, (fn, _) in runs.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(args.steps):
                fn()
            b.record()
            b.synchronize()
            times[name].append(1e3 * a.elapsed_time(b) / args.steps)
    for name in captured:       # the replays did what they claim
        ps, st, opt, _ = runs[name][1]
        assert all(bool(torch.isfinite(p).all()) for p in ps), name
        assert st.values()["adam_step"] == 1 + args.warmup + args.blocks * args.steps, name
    rec = {"parameters": int(sum(p.numel() for p in init)), "tensors": len(init), "blocks": args.blocks,
           "steps_per_block": args.steps, "device": torch.cuda.get_device_name(0)}
    lines = ["optimizer options on the step's tail: %d parameters in %d tensors, %s" % (rec["parameters"], rec["tensors"], rec["device"]),
             "%d alternating blocks of %d steps, device events; us per step (captured: advance + step() replayed)"
             % (args.blocks, args.steps)]
    for name, t in times.items():
        t = np.asarray(t)
        rec[name] = {"median_us": float(np.median(t)), "spread_us": float((np.percentile(t, 90) - np.percentile(t, 10)) / 2),
                     "min_us": float(t.min()), "max_us": float(t.max())}
        lines.append("%-40s median %8.2f us  spread +-%.2f  (min %.2f max %.2f)"
                     % (name, rec[name]["median_us"], rec[name]["spread_us"], t.min(), t.max()))
    for name in ("clip", "clip+schedule+amsgrad"):
        rec[name + " minus off_us"] = rec[name]["median_us"] - rec["off"]["median_us"]
        lines.append("%-40s %+8.2f us over `off`" % (name, rec[name + " minus off_us"]))
    print("\n".join(lines))
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
