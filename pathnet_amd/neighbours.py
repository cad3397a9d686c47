"""Exact k nearest neighbours of embeddings and the weighted k-NN classifier (pn_knn_search / pn_knn_vote, pn_knn.hip).

``knn(query, bank, k)`` finds, for every row of ``query``, the k rows of ``bank`` with the largest cosine (or dot product):
tiled HIP kernels with exact fp32 products, a total order on (score, bank index) and no ``[Sq, N]`` array in memory; the same
inputs give the same bits for every work split.  ``knn_classify`` is the weighted vote over the neighbours' labels, the
label-free monitor of contrastive pretraining (``model.knn_probe`` drives both from node ids).
"""
import collections
import ctypes
import math

import torch

from . import _lib

METRICS = {"cosine": _lib.KNN_COSINE, "dot": _lib.KNN_DOT}
MAX_K = _lib.KNN_MAX_K
MAX_D, MAX_SPLITS, MAX_CLASSES = 8192, 1024, 4096


class Neighbours(collections.namedtuple("Neighbours", ("index", "score", "count", "counts"))):
    """index int64 [Sq, k]    slot j: the bank row of the j-th neighbour (higher score first, lower index on equal bits); -1
                             past ``count``
    score float32 [Sq, k]    its score; -inf past ``count``
    count int32 [Sq]         min(k, candidates); 0 for a dead query (an entry not finite; cosine: a zero norm)
    counts int64 [2]         {dead queries, bank rows left out for their data's sake}
    All device tensors."""
    __slots__ = ()

    def summary(self):
        """A dict of Python numbers (the one host read)"""
        Sq, k = (int(v) for v in self.index.shape)
        flat = torch.cat((self.counts.double(), self.count.double().sum().reshape(1),
                          (self.count < k).double().sum().reshape(1))).cpu().numpy()
        return dict(queries=Sq, k=k, dead_queries=int(flat[0]), dead_bank_rows=int(flat[1]), neighbours=int(flat[2]),
                    short_rows=int(flat[3]))


class KnnVote(collections.namedtuple("KnnVote", ("prob", "label", "confusion", "skipped"))):
    """prob float64 [Sq, C]      normalised votes; all 0 for a query nothing voted for
    label int64 [Sq]            argmax of the votes, the lowest class on ties; -1 when nothing voted
    confusion int64 [C, C]      [true, predicted], with ``labels`` (else None): ``trainer.metrics_from_confusion`` reads it
    skipped int64 [1]           queries left out of the confusion matrix: a label outside [0, C) or nothing voted (else None)
    All device tensors."""
    __slots__ = ()


def _rows(x, name):
    if x.dim() != 2:
        raise ValueError("knn: %s [rows, D] expected, got %s" % (name, tuple(x.shape)))
    if not x.dtype.is_floating_point:
        raise TypeError("knn: %s must be a float tensor, got %s" % (name, x.dtype))
    x = x.detach().float()
    if x.shape[0] > 1 and (x.stride(1) != 1 or x.stride(0) < x.shape[1]) or x.shape[0] <= 1 and not x.is_contiguous():
        x = x.contiguous()
    return x


def plan(Sq, N, D, k, splits=None):
    """-> dict(splits, workgroups, row_tile, column_tile) a call of these shapes runs with (pn_knn_plan; needs no GPU)"""
    out = (ctypes.c_int64 * 4)()
    _lib.check(_lib.load().pn_knn_plan(int(Sq), int(N), int(D), int(k), int(splits or 0), out))
    return dict(splits=int(out[0]), workgroups=int(out[1]), row_tile=int(out[2]), column_tile=int(out[3]))


def knn(query, bank, k, metric="cosine", bank_valid=None, exclude=None, splits=None):
    """The k nearest rows of ``bank`` [N, D] for every row of ``query`` [Sq, D] (both on the GPU) -> ``Neighbours``.

    metric "cosine": rows scaled to unit length (norms in fp64); "dot": the rows as they are.  A row with an entry that is
    not finite (cosine: or with a zero norm) is dead: a dead bank row is nobody's neighbour, a dead query has no neighbours.
    bank_valid (bool / integer [N], optional): only bank rows with a non-zero flag are candidates.  exclude (integer [Sq],
    optional): one bank row per query that is no candidate of it (-1: none) -- ``exclude=torch.arange(N)`` with query is bank
    is leave-one-out.  splits (1 .. 1024, default: the library chooses) cuts the bank over workgroups; it changes no bit.
    Limits: k in 1 .. 64, D in 1 .. 8192, Sq and N below 2^31.  fp32 inputs; other float dtypes are converted.  Row-strided
    inputs (a column slice) are read in place.  Nothing is read back."""
    if query.device.type != "cuda" or bank.device != query.device:
        raise RuntimeError("pathnet_amd.knn runs on the GPU only (query on %s, bank on %s); no CPU fallback"
                           % (query.device, bank.device))
    q, x = _rows(query, "query"), _rows(bank, "bank")
    dev = q.device
    (Sq, D), N = (int(v) for v in q.shape), int(x.shape[0])
    if int(x.shape[1]) != D:
        raise ValueError("knn: query has %d columns, bank %d" % (D, int(x.shape[1])))
    k = int(k)
    if not 1 <= k <= MAX_K:
        raise ValueError("knn: k=%d, 1 .. %d" % (k, MAX_K))
    if not 1 <= D <= MAX_D:
        raise ValueError("knn: %d columns, 1 .. %d" % (D, MAX_D))
    if metric not in METRICS:
        raise ValueError("knn: metric %r, one of %s" % (metric, sorted(METRICS)))
    if splits is not None and not 1 <= int(splits) <= MAX_SPLITS:
        raise ValueError("knn: splits=%d, 1 .. %d (None: the library chooses)" % (int(splits), MAX_SPLITS))
    splits = 0 if splits is None else int(splits)
    if bank_valid is not None:
        bank_valid = torch.as_tensor(bank_valid).reshape(-1)
        if bank_valid.numel() != N:
            raise ValueError("knn: %d bank_valid flags for %d bank rows" % (bank_valid.numel(), N))
        bank_valid = (bank_valid != 0).to(device=dev, dtype=torch.uint8).contiguous()
    if exclude is not None:
        exclude = torch.as_tensor(exclude).reshape(-1)
        if exclude.numel() != Sq or exclude.dtype.is_floating_point:
            raise ValueError("knn: exclude must hold one integer bank index per query (%d), got %d of %s"
                             % (Sq, exclude.numel(), exclude.dtype))
        exclude = exclude.to(device=dev, dtype=torch.int64).contiguous()
    lib = _lib.load()
    need = ctypes.c_int64(0)
    _lib.check(lib.pn_knn_workspace_bytes(Sq, N, D, k, splits, ctypes.byref(need)))
    with torch.cuda.device(dev):
        ws = torch.empty(max(need.value, 8), dtype=torch.uint8, device=dev)
        index = torch.empty((Sq, k), dtype=torch.int64, device=dev)
        score = torch.empty((Sq, k), dtype=torch.float32, device=dev)
        count = torch.empty(Sq, dtype=torch.int32, device=dev)
        counts = torch.empty(2, dtype=torch.int64, device=dev)
        out = _lib.KnnOut(index.data_ptr(), score.data_ptr(), count.data_ptr(), counts.data_ptr())
        _lib.check(lib.pn_knn_search(_lib.context(dev), _lib.ptr(q), q.stride(0) if Sq > 1 else D, Sq, _lib.ptr(x),
                                     x.stride(0) if N > 1 else D, N, D, k, METRICS[metric], _lib.ptr(bank_valid),
                                     _lib.ptr(exclude), splits, _lib.ptr(ws), ws.numel(), ctypes.byref(out),
                                     _lib.stream_ptr(dev)))
    return Neighbours(index, score, count, counts)


def exclude_of(query_nodes, bank_nodes, num_nodes):
    """``knn(exclude=)`` for queries and bank rows that are nodes of one graph (integer ids below num_nodes, on the GPU):
    int64 [Sq], the bank position of every query's own node, -1 where it is not in the bank (a node listed twice in the bank:
    its last position).  Formed on the device, nothing is read back."""
    q, b = query_nodes.reshape(-1).long(), bank_nodes.reshape(-1).long()
    pos = torch.full((int(num_nodes),), -1, dtype=torch.int64, device=b.device)
    # (an integer maximum: "the last position" whatever order the scatter writes in)
    order = torch.arange(b.numel(), dtype=torch.int64, device=b.device)
    pos.scatter_reduce_(0, b, order, "amax", include_self=True)
    return pos.index_select(0, q.to(b.device))


def knn_classify(neighbours, bank_labels, num_classes, temperature=0.07, labels=None):
    """The weighted k-NN classifier over ``knn``'s result -> ``KnnVote``.

    bank_labels (integer [N]): slot j of a query votes for its bank row's label with weight exp((s_j - s_0) / temperature),
    s_0 the query's best score (the shift changes neither the argmax nor the normalised votes); a label outside
    [0, num_classes) does not vote.  temperature=math.inf is the plain majority vote.  The weights and sums are fp64, added in
    ascending slot order: the same bits every run.  labels (integer [Sq], optional): the queries' own labels, for the
    confusion matrix [true, predicted] and the skipped count.  Limits: num_classes in 1 .. 4096.  Nothing is read back."""
    index, score, count = neighbours.index, neighbours.score, neighbours.count
    dev = index.device
    if dev.type != "cuda":
        raise RuntimeError("pathnet_amd.knn_classify runs on the GPU only (neighbours on %s); no CPU fallback" % dev)
    Sq, k = (int(v) for v in index.shape)
    C = int(num_classes)
    if not 1 <= C <= MAX_CLASSES:
        raise ValueError("knn_classify: num_classes=%d, 1 .. %d" % (C, MAX_CLASSES))
    T = float(temperature)
    if not T > 0.0:
        raise ValueError("knn_classify: temperature %r, > 0 (math.inf: the majority vote)" % (temperature,))
    bank_labels = torch.as_tensor(bank_labels).reshape(-1)
    if bank_labels.dtype.is_floating_point:
        raise TypeError("knn_classify: bank_labels must be integers, got %s" % bank_labels.dtype)
    bank_labels = bank_labels.to(device=dev, dtype=torch.int64).contiguous()
    N = int(bank_labels.numel())
    if labels is not None:
        labels = torch.as_tensor(labels).reshape(-1)
        if labels.numel() != Sq or labels.dtype.is_floating_point:
            raise ValueError("knn_classify: one integer label per query (%d) expected, got %d of %s"
                             % (Sq, labels.numel(), labels.dtype))
        labels = labels.to(device=dev, dtype=torch.int64).contiguous()
    with torch.cuda.device(dev):
        prob = torch.empty((Sq, C), dtype=torch.float64, device=dev)
        label = torch.empty(Sq, dtype=torch.int64, device=dev)
        confusion = torch.zeros((C, C), dtype=torch.int64, device=dev) if labels is not None else None
        skipped = torch.zeros(1, dtype=torch.int64, device=dev) if labels is not None else None
        _lib.check(_lib.load().pn_knn_vote(_lib.context(dev), _lib.ptr(index.contiguous()), _lib.ptr(score.contiguous()),
                                           _lib.ptr(count.contiguous()), Sq, k, _lib.ptr(bank_labels), N, C, T, _lib.ptr(labels),
                                           _lib.ptr(prob), _lib.ptr(label), _lib.ptr(confusion), _lib.ptr(skipped),
                                           _lib.stream_ptr(dev)))
    return KnnVote(prob, label, confusion, skipped)
