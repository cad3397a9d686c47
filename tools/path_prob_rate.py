#!/usr/bin/env python
"""Rate of the path likelihoods (pn_prob.hip) beside the Philox walker that produced the paths, in transitions per second.

    python tools/path_prob_rate.py [--repeats 20] [--epochs 16] [--out FILE]

The bench graph and shape (bench.synthetic_graph(2708, 0), W = 40, L = 4, dense hops), --epochs epochs per call, so one call
sees epochs * 2708 * 40 * 3 transitions.  Each call is timed between device events on one stream after three warm-up calls,
median of --repeats (min and max beside it):
    walker              smp.sample(..., check=False) into preallocated outputs: what produces the paths
    path_prob           smp.path_prob(ids): the kernel in first order, then num / 2^62 and the log-likelihoods (torch ops)
    path_prob realised  smp.biased(4, .25).path_prob(ids): the kernel in second order (class masses and classes), then the
                        realised probabilities and the log-likelihoods (torch ops)
    kernel 1st / 2nd    pn_path_prob alone into preallocated outputs, first and second order
Before anything is timed the numerators of every source row are checked to be possible (> 0) and the masses to sum to 2^62.
Needs a GPU; there is no fallback.
"""
import ctypes
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from pathnet_amd import MerwSampler, _lib  # noqa: E402

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


def main():
    argv = list(sys.argv[1:])
    repeats, epochs, out = 20, 16, None
    for flag in ("--repeats", "--epochs", "--out"):
        if flag in argv:
            k = argv.index(flag)
            if flag == "--repeats":
                repeats = int(argv[k + 1])
            elif flag == "--epochs":
                epochs = int(argv[k + 1])
            else:
                out = argv[k + 1]
            del argv[k:k + 2]
    if not torch.cuda.is_available():
        raise SystemExit("path_prob_rate: needs a GPU (a CPU run says nothing about the device)")
    W, L = 40, 4
    n, u, v, p = bench.synthetic_graph(2708, 0)
    smp = MerwSampler(n, u, v, p, L, hops="dense")
    view = smp.biased(4, .25)
    buf = (torch.empty((epochs, n, W, L), dtype=torch.int32, device="cuda"),
           torch.empty((epochs, n, W, L), dtype=torch.uint8, device="cuda"))
    ids, _ = smp.sample(W, SEED, epoch_count=epochs, out=buf)
    steps = ids.numel() // L * (L - 1)
    first, second = smp.path_prob(ids), view.path_prob(ids)
    assert (first.num > 0).all() and torch.equal(first.num, second.num) and first.counters.tolist() == [0, 0, 0, 0]
    assert (second.mass[..., 1:, :].sum(-1) == 2 ** 62).all() and torch.isfinite(second.logp).all()

    lib, dev = _lib.load(), ids.device
    tb = smp._tables()
    desc1 = _lib.PathProbOut(second.num.data_ptr(), None, None, second.counters.data_ptr())
    desc2 = _lib.PathProbOut(second.num.data_ptr(), second.mass.data_ptr(), second.cls.data_ptr(), second.counters.data_ptr())

    def kernel(desc, order):
        _lib.check(lib.pn_path_prob(_lib.context(dev), ctypes.byref(tb), W, L, epochs * n, _lib.ptr(ids), order,
                                    ctypes.byref(desc), None, 0, _lib.stream_ptr(dev)))

    lines = ["# %s, bench graph n = %d, W = %d, L = %d, %d epochs a call = %d transitions, median of %d calls after 3 warm-ups, "
             "device events" % (torch.cuda.get_device_name(0), n, W, L, epochs, steps, repeats)]
    rows = {}

    def row(label, fn):
        med, lo, hi = median_ms(fn, repeats)
        rows[label] = r = dict(what=label, ms=round(med, 4), ms_min=round(lo, 4), ms_max=round(hi, 4),
                               transitions_per_s=round(steps / (med * 1e-3)))
        if "walker" in rows:
            r["of_walker_rate"] = round(r["transitions_per_s"] / rows["walker"]["transitions_per_s"], 3)
        lines.append(json.dumps(r))
        print(lines[-1], flush=True)

    row("walker", lambda: smp.sample(W, SEED, epoch_count=epochs, out=buf, check=False))
    row("path_prob", lambda: smp.path_prob(ids))
    row("path_prob realised", lambda: view.path_prob(ids))
    row("kernel 1st", lambda: kernel(desc1, 0))
    row("kernel 2nd", lambda: kernel(desc2, 1))
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
