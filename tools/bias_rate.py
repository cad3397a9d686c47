#!/usr/bin/env python
"""Rate of the biased walker (pn_bias.hip) beside the plain Philox walker, in paths/s.

    python tools/bias_rate.py [--repeats 20] [--big-n 1000000] [--out FILE]

Two shapes, W = 40, L = 4:
    step   the training step: 1 300 listed source nodes over the Cora tables (tests/golden/sampler_cora_40_4.npz), dense hops
    large  --big-n nodes, degree ~16 (tools/bench_sampler_large.er_graph), every node, hop codes on the fly
Each call is timed between device events on one stream into preallocated outputs (check=False: nothing is read back) after
three warm-up calls, median of --repeats (min and max beside it).  The biased walk runs at (p, q) = (1, 1) -- every
proposal accepted: the cost of the second-order machinery alone -- and (4, 1/4).  Mean trials per step come from the CPU
restatement tests/biased_ref.py over the same tables and seed (the large shape: the first 2 000 source nodes).
On the fly the biased call is two launches (walk, then pn_path_codes over its ids); the plain walker finds the codes
while it walks.  Needs a GPU; there is no fallback.
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import biased_ref  # noqa: E402
from bench_sampler_large import er_graph  # noqa: E402
from pathnet_amd import MerwSampler  # noqa: E402

SETTINGS = ((1.0, 1.0), (4.0, 0.25))
SEED = 1


def median_ms(fn, repeats):
    for _ in range(3):
        fn()
    ts = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    ts.sort()
    return ts[len(ts) // 2], ts[0], ts[-1]


def measure(name, smp, tb, W, nodes, ref_nodes, repeats, lines):
    count = smp.n if nodes is None else int(nodes.numel())
    out = (torch.empty((1, count, W, smp.L), dtype=torch.int32, device="cuda"),
           torch.empty((1, count, W, smp.L), dtype=torch.uint8, device="cuda"))
    paths = count * W
    rows = []

    def row(label, fn, trials):
        med, lo, hi = median_ms(fn, repeats)
        r = dict(shape=name, walk=label, paths=paths, ms=round(med, 4), ms_min=round(lo, 4), ms_max=round(hi, 4),
                 paths_per_s=round(paths / (med * 1e-3)), trials_per_step=trials)
        rows.append(r)
        lines.append(json.dumps(r))
        print(lines[-1], flush=True)

    row("plain philox", lambda: smp.sample(W, SEED, check=False, out=out, nodes=nodes), 1.0)
    for p, q in SETTINGS:
        view = smp.biased(p, q)
        ref = biased_ref.walk(tb, W, smp.L, SEED, p, q, sources=ref_nodes, codes=False)
        row("biased (%g, %g)" % (p, q), lambda: view.sample(W, SEED, check=False, out=out, nodes=nodes),
            round(ref.trials / ref.steps, 3))
        rows[-1]["exhausted"] = view.exhausted_steps()
    return rows


def main():
    argv = list(sys.argv[1:])
    repeats, out, big_n = 20, None, 1_000_000
    for flag in ("--repeats", "--out", "--big-n"):
        if flag in argv:
            i = argv.index(flag)
            if flag == "--repeats":
                repeats = int(argv[i + 1])
            elif flag == "--big-n":
                big_n = int(argv[i + 1])
            else:
                out = argv[i + 1]
            del argv[i:i + 2]
    if not torch.cuda.is_available():
        raise SystemExit("bias_rate: needs a GPU (a CPU run says nothing about the device)")
    W, L = 40, 4
    lines = ["# %s, W = %d, L = %d, median of %d calls after 3 warm-ups, device events" % (torch.cuda.get_device_name(0), W, L, repeats)]
    g = dict(np.load(os.path.join(ROOT, "tests", "golden", "sampler_cora_40_4.npz")))
    n = int(g["n"])
    listed = np.sort(np.random.default_rng(0).permutation(n)[:1300]).astype(np.int32)
    smp = MerwSampler(n, g["u"], g["v"], g["p"], L, hops="dense")
    measure("step: 1300 listed nodes, Cora tables, dense", smp, biased_ref.merw_tables(n, g["u"], g["v"], g["p"]), W,
            torch.as_tensor(listed).cuda(), listed, repeats, lines)
    del smp
    n, u, v, p = er_graph(big_n, 16, 0)
    smp = MerwSampler(n, u, v, p, L, hops="otf", build="device")
    measure("large: %d nodes, degree ~16, on the fly" % n, smp, biased_ref.merw_tables(n, u, v, p), W, None,
            np.arange(min(n, 2000)), repeats, lines)
    if out:
        with open(out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
