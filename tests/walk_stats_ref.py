"""Plain NumPy restatement of pn_walk_stats (include/pathnet_hip.h, pn_stats.hip): the reference of every comparison in
test_walk_stats_host.py and test_gpu_walk_stats.py.  Written from the definitions, with Python sets where the kernel sorts."""
import collections

import numpy as np

FIELDS = ("step_code", "label_pairs", "unlabeled", "stay", "back", "distinct_hist", "unique_paths", "cover", "visits",
          "counters")
GLOBAL = tuple(f for f in FIELDS if f not in ("unique_paths", "cover"))      # the tables `accumulate` adds to
Stats = collections.namedtuple("Stats", FIELDS)


def walk_stats(ids, codes, n, labels=None, num_classes=None, sources=None):
    """ids, codes: [..., W, L] -> Stats of int64 arrays (unique_paths / cover: int32 [rows]; label_pairs and unlabeled: None
    without labels)."""
    ids = np.asarray(ids)
    W, L = ids.shape[-2:]
    ids = ids.reshape(-1, W, L).astype(np.int64)
    codes = np.asarray(codes).reshape(-1, W, L).astype(np.int64)
    rows = ids.shape[0]
    src = ids[:, 0, 0] if sources is None else np.asarray(sources).reshape(-1).astype(np.int64)
    assert src.shape[0] == rows
    inside = (ids >= 0) & (ids < n)
    good = codes < L
    t = np.broadcast_to(np.arange(L), ids.shape)
    counters = np.array([(~inside).sum(), (~good).sum()], np.int64)
    step_code = np.zeros((L, L), np.int64)
    np.add.at(step_code, (t[good], codes[good]), 1)

    label_pairs = unlabeled = None
    if labels is not None:
        C = int(num_classes)
        labels = np.asarray(labels).astype(np.int64)

        def label_of(x, ok):        # -1: none
            lab = np.full(x.shape, -1, np.int64)
            lab[ok] = labels[x[ok]]
            lab[(lab < 0) | (lab >= C)] = -1
            return lab
        la = np.broadcast_to(label_of(src, (src >= 0) & (src < n))[:, None, None], ids.shape)
        lb = label_of(ids, inside)
        both = good & (la >= 0) & (lb >= 0)
        label_pairs = np.zeros((L, C, C), np.int64)
        np.add.at(label_pairs, (codes[both], la[both], lb[both]), 1)
        unlabeled = np.zeros(L, np.int64)
        np.add.at(unlabeled, codes[good & ~both], 1)

    stay = np.zeros(L, np.int64)
    back = np.zeros(L, np.int64)
    for k in range(1, L):
        stay[k] = (ids[..., k] == ids[..., k - 1]).sum()
    for k in range(2, L):
        back[k] = ((ids[..., k] == ids[..., k - 2]) & (ids[..., k] != ids[..., k - 1])).sum()

    distinct_hist = np.zeros(L + 1, np.int64)
    unique_paths = np.zeros(rows, np.int32)
    cover = np.zeros(rows, np.int32)
    for s in range(rows):
        for w in range(W):
            distinct_hist[len(set(ids[s, w].tolist()))] += 1
        unique_paths[s] = len({tuple(p) for p in ids[s].tolist()})
        cover[s] = len(set(ids[s].reshape(-1).tolist()))

    later = ids[..., 1:][inside[..., 1:]]
    visits = np.bincount(later, minlength=n).astype(np.int64)
    return Stats(step_code, label_pairs, unlabeled, stay, back, distinct_hist, unique_paths, cover, visits, counters)
