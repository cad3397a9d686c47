"""Walk statistics: what sampled paths look like, counted on the GPU without a read-back (pn_walk_stats, pn_stats.hip).

``walk_stats(ids, codes, n, ...)`` makes one pass over the paths a sampler returned (or any ``[..., W, L]`` ids with their
distance codes) and returns a ``WalkStats`` of device tensors; ``.summary()`` makes the one host read.  The samplers carry
it as ``smp.walk_stats(ids, codes, ...)`` with their own n.

``python -m pathnet_amd.walkstats <edge file> <W> <L> [--uniform] [--bias P,Q] [--epochs E] [--labels FILE] [--seed S]``
samples with Philox draws and prints one JSON object: the code-by-step table, stay and back shares, mean unique paths, mean
cover and, with a label file (one integer per node, -1 = unlabelled), the label agreement by distance.
"""
import collections
import ctypes
import json
import sys

import numpy as np
import torch

from . import _lib

FIELDS = _lib.WalkStatsOut.FIELDS
PER_ROW = ("unique_paths", "cover")
GLOBAL = tuple(f for f in FIELDS if f not in PER_ROW)       # the int64 tables a call zeroes, or adds to


class WalkStats(collections.namedtuple("WalkStats", FIELDS)):
    """Device tensors; a field that was not asked for is None.
    step_code int64 [L, L]      [t][d]: path nodes at step t with distance code d
    label_pairs int64 [L, C, C] [d][a][b]: path nodes with code d, source label a, own label b
    unlabeled int64 [L]         [d]: path nodes with code d where either label is missing
    stay, back int64 [L]        [t]: ids[t] == ids[t-1]; ids[t] == ids[t-2] != ids[t-1]
    distinct_hist int64 [L+1]   [k]: paths that visit exactly k distinct ids
    unique_paths, cover int32 [rows...]   distinct id sequences / distinct ids of a row's W paths
    visits int64 [n]            times a node occurs at a step >= 1
    counters int64 [2]          {ids outside [0, n), codes >= L}"""
    __slots__ = ()

    def summary(self):
        """A small dict of Python numbers (one host read; visits and the per-row tensors are reduced on the device)."""
        parts, names = [], []
        for f in GLOBAL:
            t = getattr(self, f)
            if t is not None and f != "visits":
                names.append((f, tuple(t.shape)))
                parts.append(t.reshape(-1))
        for f in PER_ROW:
            t = getattr(self, f)
            if t is not None:
                names.append((f, (2,)))
                parts.append(torch.stack((t.sum(dtype=torch.int64), torch.tensor(t.numel(), device=t.device))))
        if self.visits is not None:
            names.append(("visits", (2,)))
            parts.append(torch.stack((self.visits.sum(), (self.visits > 0).sum())))
        flat = torch.cat(parts).cpu().numpy() if parts else np.zeros(0, np.int64)
        got, at = {}, 0
        for f, shape in names:
            k = int(np.prod(shape))
            got[f] = flat[at:at + k].reshape(shape)
            at += k
        share = lambda a, b: float(a) / float(b) if b else None      # noqa: E731
        out = {}
        if "step_code" in got:
            sc = got["step_code"]
            out["path_nodes"] = int(sc.sum())
            out["step_code"] = sc.tolist()
            paths = int(sc[0].sum())
            for f in ("stay", "back"):
                if f in got:
                    out[f + "_share"] = [share(v, paths) for v in got[f].tolist()]
        if "distinct_hist" in got:
            dh = got["distinct_hist"]
            out["paths"] = int(dh.sum())
            out["mean_distinct_nodes"] = share((dh * np.arange(len(dh))).sum(), dh.sum())
        if "unique_paths" in got:
            out["mean_unique_paths"] = share(*got["unique_paths"])
        if "cover" in got:
            out["mean_cover"] = share(*got["cover"])
        if "label_pairs" in got:
            lp = got["label_pairs"]
            out["label_agreement"] = [share(np.trace(m), m.sum()) for m in lp]
            out["labelled_pairs"] = lp.sum(axis=(1, 2)).tolist()
        if "unlabeled" in got:
            out["unlabeled"] = got["unlabeled"].tolist()
        if "visits" in got:
            out["visits"] = int(got["visits"][0])
            out["visited_nodes"] = int(got["visits"][1])
        if "counters" in got:
            out["out_of_range"], out["bad_codes"] = (int(x) for x in got["counters"])
        return out


def _int32(t, name, dev):
    t = t if isinstance(t, torch.Tensor) else torch.as_tensor(t)
    if t.dtype.is_floating_point or t.dtype.is_complex or t.dtype == torch.bool:
        raise TypeError("walk_stats: integer %s expected, got %s" % (name, t.dtype))
    if t.dtype != torch.int32:
        t = t.clamp(-1, 2 ** 31 - 1).to(torch.int32)
    return t.to(dev).contiguous()


def _shapes(n, L, C, lead, rows):
    return dict(step_code=(L, L), label_pairs=(L, C, C), unlabeled=(L,), stay=(L,), back=(L,), distinct_hist=(L + 1,),
                unique_paths=lead, cover=lead, visits=(n,), counters=(2,))


def walk_stats(ids, codes, n, *, labels=None, num_classes=None, sources=None, visits=False, per_row=True,
               accumulate_into=None, out=None):
    """Statistics of the paths ids / codes ``[..., W, L]`` (int32 / uint8 device tensors as sample() returns them; anything
    else is converted and uploaded) over a graph of n nodes -> WalkStats.  A row is one ``[W, L]`` block; its source is
    sources[row] when given (shape ``ids.shape[:-2]``), else its first node.
    labels (int [n], with num_classes = C <= 64): also label_pairs and unlabeled; -1 or anything outside [0, C) is "no
    label".  visits=True: also the per-node visit counts [n].  per_row=False: skip unique_paths and cover (the two sorts).
    accumulate_into=WalkStats: add to its tables instead of zeroing new ones -- a loop over epochs profiles a run without
    keeping its paths; its None fields stay None, and unique_paths / cover are this call's own.
    out=WalkStats: write into these tensors (zeroed by the call); its None fields are not computed.
    Limits: L <= 16, W * L <= 8192.  Enqueued on the current stream; nothing is read back."""
    if accumulate_into is not None and out is not None:
        raise ValueError("walk_stats: accumulate_into and out exclude each other")
    t = ids if isinstance(ids, torch.Tensor) else torch.as_tensor(ids)
    if t.dim() < 2:
        raise ValueError("walk_stats: ids of shape [..., W, L] expected, got %s" % (tuple(t.shape),))
    dev = t.device if t.is_cuda else torch.device("cuda", torch.cuda.current_device())
    t = _int32(t, "ids", dev)
    c = codes if isinstance(codes, torch.Tensor) else torch.as_tensor(codes)
    if tuple(c.shape) != tuple(t.shape):
        raise ValueError("walk_stats: codes of shape %s for ids of shape %s" % (tuple(c.shape), tuple(t.shape)))
    if c.dtype != torch.uint8:
        c = c.clamp(0, 255).to(torch.uint8)
    c = c.to(dev).contiguous()
    W, L = int(t.shape[-2]), int(t.shape[-1])
    lead = tuple(t.shape[:-2])
    rows = t.numel() // max(W * L, 1)
    C = 0
    if labels is not None:
        if num_classes is None:
            raise ValueError("walk_stats: labels need num_classes")
        C = int(num_classes)
        labels = _int32(labels, "labels", dev)
        if labels.numel() != n:
            raise ValueError("walk_stats: %d labels for %d nodes" % (labels.numel(), n))
    if sources is not None:
        sources = _int32(sources, "sources", dev)
        if sources.numel() != rows:
            raise ValueError("walk_stats: %d sources for %d rows" % (sources.numel(), rows))
    need = ctypes.c_int64(0)
    lib = _lib.load()
    _lib.check(lib.pn_walk_stats_workspace_bytes(int(n), W, L, rows, C, ctypes.byref(need)))   # refuses a bad shape here
    shapes = _shapes(int(n), L, C, lead, rows)
    given = accumulate_into if accumulate_into is not None else out
    with torch.cuda.device(dev):
        if given is None:
            want = [f for f in GLOBAL if (labels is not None or f not in ("label_pairs", "unlabeled")) and
                    (visits or f != "visits")]
            sizes = [int(np.prod(shapes[f])) for f in want]
            block = torch.empty(sum(sizes), dtype=torch.int64, device=dev)      # one allocation; the call zeroes it
            got = dict(zip(want, (p.view(shapes[f]) for f, p in zip(want, block.split(sizes)))))
        else:
            got = {f: getattr(given, f) for f in GLOBAL}
            if accumulate_into is None:
                got.update({f: getattr(given, f) for f in PER_ROW})
            for f, x in got.items():
                if x is None:
                    continue
                dt = torch.int32 if f in PER_ROW else torch.int64
                if labels is None and f in ("label_pairs", "unlabeled"):
                    raise ValueError("walk_stats: %s asked for without labels" % f)
                if tuple(x.shape) != tuple(shapes[f]) or x.dtype != dt or not x.is_contiguous() or x.device != dev:
                    raise ValueError("walk_stats: %s must be a contiguous %s tensor of shape %s on %s, got %s %s on %s"
                                     % (f, dt, tuple(shapes[f]), dev, x.dtype, tuple(x.shape), x.device))
        if given is None or accumulate_into is not None:
            for f in PER_ROW:
                got[f] = torch.empty(lead, dtype=torch.int32, device=dev) if per_row else None
        ws = torch.empty(need.value, dtype=torch.uint8, device=dev) if need.value else None
        desc = _lib.WalkStatsOut(*(got[f].data_ptr() if got.get(f) is not None else None for f in FIELDS))
        _lib.check(lib.pn_walk_stats(_lib.context(dev), int(n), W, L, rows, _lib.ptr(t), _lib.ptr(c), _lib.ptr(sources),
                                     _lib.ptr(labels), C, 1 if accumulate_into is not None else 0, ctypes.byref(desc),
                                     _lib.ptr(ws), need.value, _lib.stream_ptr(dev)))
    return WalkStats(*(got.get(f) for f in FIELDS))


def path_multiplicity(ids, codes=None):
    """How often each path of a row occurs in it (pn_path_multiplicity): ids ``[..., W, L]`` (codes alike, or None) ->
    float32 ``[..., W]`` on the device.  Entry j of a row counts the paths whose id sequence -- and code sequence, with
    codes -- equals path j's when j is the first of them, and is 0 otherwise, so every row sums to W.  Passed as
    ``path_weights=`` to PathNet_homo / PAGG it pools every distinct path of a node once, weighted by how often it was drawn:
    the same value as the unweighted call.  (Not for PathNet, whose pooling slots are not its rows' paths.)
    Limits: L <= 16, W * L <= 8192.  Enqueued on the current stream; nothing is read back."""
    t = ids if isinstance(ids, torch.Tensor) else torch.as_tensor(ids)
    if t.dim() < 2:
        raise ValueError("path_multiplicity: ids of shape [..., W, L] expected, got %s" % (tuple(t.shape),))
    dev = t.device if t.is_cuda else torch.device("cuda", torch.cuda.current_device())
    t = _int32(t, "ids", dev)
    c = None
    if codes is not None:
        c = codes if isinstance(codes, torch.Tensor) else torch.as_tensor(codes)
        if tuple(c.shape) != tuple(t.shape):
            raise ValueError("path_multiplicity: codes of shape %s for ids of shape %s" % (tuple(c.shape), tuple(t.shape)))
        if c.dtype != torch.uint8:
            c = c.clamp(0, 255).to(torch.uint8)
        c = c.to(dev).contiguous()
    W, L = int(t.shape[-2]), int(t.shape[-1])
    rows = t.numel() // max(W * L, 1)
    with torch.cuda.device(dev):
        mult = torch.empty(tuple(t.shape[:-1]), dtype=torch.float32, device=dev)
        _lib.check(_lib.load().pn_path_multiplicity(_lib.context(dev), W, L, rows, _lib.ptr(t), _lib.ptr(c), _lib.ptr(mult),
                                                    _lib.stream_ptr(dev)))
    return mult


def main(argv=None):
    argv = list(sys.argv[1:] if argv is None else argv)
    from . import sampler
    uniform = "--uniform" in argv
    opts = {"--bias": None, "--epochs": "1", "--labels": None, "--seed": "0"}
    pos, i = [], 0
    while i < len(argv):
        a = argv[i]
        if a == "--uniform":
            i += 1
        elif a in opts:
            if i + 1 >= len(argv):
                print("ERROR: %s needs a value" % a, file=sys.stderr)
                return 2
            opts[a] = argv[i + 1]
            i += 2
        else:
            pos.append(a)
            i += 1
    if len(pos) != 3:
        print("usage: python -m pathnet_amd.walkstats <edge file> <W> <L> [--uniform] [--bias P,Q] [--epochs E] "
              "[--labels FILE] [--seed S]", file=sys.stderr)
        return 2
    edge, W, L = pos[0], int(pos[1]), int(pos[2])
    epochs, seed = int(opts["--epochs"]), int(opts["--seed"])
    smp = sampler.UniformSampler.from_pair_file(edge, L) if uniform else sampler.MerwSampler.from_edge_file(edge, L)
    if opts["--bias"] is not None:
        bias = tuple(float(x) for x in opts["--bias"].split(","))
        if len(bias) != 2:
            print("ERROR: --bias P,Q expected", file=sys.stderr)
            return 2
        smp = smp.biased(*bias)
    labels = C = None
    if opts["--labels"] is not None:
        labels = np.loadtxt(opts["--labels"], dtype=np.int64, ndmin=1).reshape(-1)
        if labels.size != smp.n:
            print("ERROR: %d labels for %d nodes" % (labels.size, smp.n), file=sys.stderr)
            return 2
        C = max(int(labels.max()) + 1, 1)
        labels = torch.as_tensor(labels.astype(np.int32)).to(smp.device)
    chunk = max(1, min(epochs, (256 << 20) // max(1, smp.n * W * L * 5)))
    total = None
    per_row = torch.zeros(2, dtype=torch.int64, device=smp.device)       # sums of unique_paths and cover
    for e0 in range(0, epochs, chunk):
        ids, codes = smp.sample(W, seed, epoch_begin=e0, epoch_count=min(chunk, epochs - e0))
        st = walk_stats(ids, codes, smp.n, labels=labels, num_classes=C, accumulate_into=total)
        per_row += torch.stack((st.unique_paths.sum(dtype=torch.int64), st.cover.sum(dtype=torch.int64)))
        total = st
    res = dict(edge_file=edge, n=smp.n, W=W, L=L, epochs=epochs, seed=seed,
               sampler="uniform" if uniform else "merw", bias=opts["--bias"])
    res.update(total._replace(unique_paths=None, cover=None).summary())
    rows = max(epochs * smp.n, 1)
    res["mean_unique_paths"], res["mean_cover"] = (float(x) / rows for x in per_row.tolist())
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
