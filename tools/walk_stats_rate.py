#!/usr/bin/env python
"""Rate of the walk statistics (pn_stats.hip) beside the Philox walker and beside the same statistics written with stock
torch ops on the device, in path nodes per second.

    python tools/walk_stats_rate.py [--repeats 20] [--epochs 16] [--out FILE]

The bench graph and shape (bench.synthetic_graph(2708, 0), W = 40, L = 4, 7 classes), --epochs epochs per call, so one call
sees epochs * 2708 * 160 path nodes.  Each call is timed between device events on one stream into preallocated outputs
after three warm-up calls, median of --repeats (min and max beside it):
    walker            smp.sample(..., check=False): what produces the paths
    walk_stats        every output but visits (the default of walk_stats), labels given
    walk_stats -rows  the same without unique_paths and cover: the call without its two sorts
    walk_stats +vis   every output, visits included
    torch             step_code / label_pairs / unlabeled by bincount, stay / back by comparison, distinct ids per path, unique
                      paths and cover by sort + neighbour comparison (a path packed into one int64 key: ids < 2^15 and
                      L <= 4 only) -- what a user can write on the device without this kernel; its results are compared
                      with the kernel's before anything is timed
Needs a GPU; there is no fallback.
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from pathnet_amd import MerwSampler, walk_stats  # noqa: E402

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


def torch_stats(ids, codes, n, labels, C):
    """The statistics of walk_stats (without visits and the two counters) from stock torch ops; ids [E, n, W, L] in range."""
    W, L = ids.shape[-2:]
    i = ids.reshape(-1, W, L).long()
    c = codes.reshape(-1, W, L).long()
    t = torch.arange(L, device=ids.device).expand_as(i)
    step_code = torch.bincount((t * L + c).reshape(-1), minlength=L * L).view(L, L)
    la = labels.long()[i[:, :1, :1]].expand_as(i)
    lb = labels.long()[i]
    ok = (la >= 0) & (lb >= 0)
    label_pairs = torch.bincount(((c * C + la) * C + lb)[ok], minlength=L * C * C).view(L, C, C)
    unlabeled = torch.bincount(c[~ok], minlength=L)
    stay = torch.zeros(L, dtype=torch.int64, device=ids.device)
    back = torch.zeros(L, dtype=torch.int64, device=ids.device)
    eq1 = i[..., 1:] == i[..., :-1]
    stay[1:] = eq1.sum((0, 1))
    back[2:] = ((i[..., 2:] == i[..., :-2]) & ~eq1[..., 1:]).sum((0, 1))
    s = i.sort(-1).values
    distinct = 1 + (s[..., 1:] != s[..., :-1]).sum(-1)
    distinct_hist = torch.bincount(distinct.reshape(-1), minlength=L + 1)
    key = torch.zeros(i.shape[:-1], dtype=torch.int64, device=ids.device)
    for k in range(L):
        key = key * 32768 + i[..., k]
    ks = key.sort(-1).values
    unique_paths = 1 + (ks[:, 1:] != ks[:, :-1]).sum(-1)
    fs = i.reshape(i.shape[0], -1).sort(-1).values
    cover = 1 + (fs[:, 1:] != fs[:, :-1]).sum(-1)
    return dict(step_code=step_code, label_pairs=label_pairs, unlabeled=unlabeled, stay=stay, back=back,
                distinct_hist=distinct_hist, unique_paths=unique_paths, cover=cover)


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
        raise SystemExit("walk_stats_rate: needs a GPU (a CPU run says nothing about the device)")
    W, L, C = 40, 4, 7
    n, u, v, p = bench.synthetic_graph(2708, 0)
    labels = torch.as_tensor(np.random.default_rng(1).integers(0, C, n).astype(np.int32)).cuda()
    smp = MerwSampler(n, u, v, p, L, hops="dense")
    buf = (torch.empty((epochs, n, W, L), dtype=torch.int32, device="cuda"),
           torch.empty((epochs, n, W, L), dtype=torch.uint8, device="cuda"))
    ids, codes = smp.sample(W, SEED, epoch_count=epochs, out=buf)
    nodes = ids.numel()
    full = walk_stats(ids, codes, n, labels=labels, num_classes=C, visits=True)
    want = torch_stats(ids, codes, n, labels, C)
    for f, x in want.items():
        assert torch.equal(getattr(full, f).reshape(-1).long(), x.reshape(-1)), "torch formulation disagrees on " + f
    lines = ["# %s, bench graph n = %d, W = %d, L = %d, C = %d, %d epochs a call = %d path nodes, median of %d calls after "
             "3 warm-ups, device events" % (torch.cuda.get_device_name(0), n, W, L, C, epochs, nodes, repeats)]
    rows = {}

    def row(label, fn):
        med, lo, hi = median_ms(fn, repeats)
        rows[label] = r = dict(what=label, ms=round(med, 4), ms_min=round(lo, 4), ms_max=round(hi, 4),
                               path_nodes_per_s=round(nodes / (med * 1e-3)))
        if "walker" in rows:
            r["of_walker_rate"] = round(r["path_nodes_per_s"] / rows["walker"]["path_nodes_per_s"], 3)
        lines.append(json.dumps(r))
        print(lines[-1], flush=True)

    row("walker", lambda: smp.sample(W, SEED, epoch_count=epochs, out=buf, check=False))
    row("walk_stats", lambda: walk_stats(ids, codes, n, labels=labels, num_classes=C, out=full._replace(visits=None)))
    row("walk_stats -rows", lambda: walk_stats(ids, codes, n, labels=labels, num_classes=C,
                                               out=full._replace(visits=None, unique_paths=None, cover=None)))
    row("walk_stats +vis", lambda: walk_stats(ids, codes, n, labels=labels, num_classes=C, out=full))
    row("torch", lambda: torch_stats(ids, codes, n, labels, C))
    r = dict(what="walk_stats over torch", speedup=round(rows["torch"]["ms"] / rows["walk_stats"]["ms"], 2))
    lines.append(json.dumps(r))
    print(lines[-1], flush=True)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
