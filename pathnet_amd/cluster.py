"""k-means clustering of embeddings and the scores of a grouping against labels (pn_kmeans_run / pn_cluster_scores,
pn_kmeans.hip).

``kmeans(x, clusters)`` groups the rows of ``x`` by cosine or squared euclidean distance: k-means++ seeding and Lloyd's
iterations in HIP kernels with exact fp32 products, defined ties (the lowest cluster), fp64 means added in ascending row
order and no ``[N, K]`` array in memory; the same inputs give the same bits in every run.  ``cluster_scores`` holds a grouping
against labels: the contingency table, NMI, ARI and purity on the device (``model.cluster_probe`` drives both from node ids).
"""
import collections
import ctypes

import torch

from . import _lib

METRICS = {"cosine": _lib.KMEANS_COSINE, "euclidean": _lib.KMEANS_EUCLIDEAN}
MAX_K = _lib.KMEANS_MAX_K
MAX_D, MAX_ITERS, MAX_CLASSES = 8192, 65536, 4096


class Clusters(collections.namedtuple("Clusters", ("label", "centroid", "count", "inertia", "iterations", "moved", "counts"))):
    """label int64 [N]          the cluster of every row, the nearest of ``centroid``; -1 for a dead row (an entry not finite;
                              cosine: a zero norm; ``valid`` 0)
    centroid float32 [K, D]  cosine: unit rows
    count int64 [K]          members
    inertia float64 [1]      the sum of the live rows' costs (cosine: 1 - cos; euclidean: the squared distance)
    iterations int32 [1]     assignments run before none moved (at most ``iters``)
    moved int64 [iters]      rows that changed cluster in every assignment; -1 past ``iterations``
    counts int64 [1]         {dead rows}
    All device tensors, of the best restart."""
    __slots__ = ()

    def summary(self):
        """A dict of Python numbers (the one host read)"""
        flat = torch.cat((self.inertia.double(), self.iterations.double(), self.counts.double(),
                          (self.count == 0).double().sum().reshape(1), self.count.double().max().reshape(1),
                          self.moved.double())).cpu().numpy()
        its = int(flat[1])
        return dict(rows=int(self.label.shape[0]), clusters=int(self.centroid.shape[0]), inertia=float(flat[0]), iterations=its,
                    converged=bool(its > 0 and flat[5 + its - 1] == 0), dead_rows=int(flat[2]), empty_clusters=int(flat[3]),
                    largest=int(flat[4]), moved=[int(v) for v in flat[5:5 + its]])


class ClusterScores(collections.namedtuple("ClusterScores", ("table", "nmi", "ari", "purity", "n", "skipped"))):
    """table int64 [K, C]       [cluster, class] counts
    nmi, ari, purity float64 [1]   normalised mutual information (arithmetic mean of the entropies, natural logs), adjusted
                              Rand index, purity; NaN when n == 0
    n float64 [1]            pairs in the table
    skipped int64 [1]        pairs left out: a cluster or a class outside its range (a dead row's -1, an unlabelled node)
    All device tensors."""
    __slots__ = ()

    def summary(self):
        """A dict of Python numbers; reads the table once.  ``accuracy`` is computed ON THE HOST from that table: the best
        one-to-one match of clusters to classes (scipy.optimize.linear_sum_assignment), matched pairs / n."""
        from scipy.optimize import linear_sum_assignment
        K, C = (int(v) for v in self.table.shape)
        flat = torch.cat((self.table.reshape(-1).double(), self.nmi, self.ari, self.purity, self.n,
                          self.skipped.double())).cpu().numpy()
        table = flat[:K * C].reshape(K, C).astype("int64")
        n = int(flat[K * C + 3])
        rows, cols = linear_sum_assignment(table, maximize=True)
        return dict(n=n, skipped=int(flat[K * C + 4]), nmi=float(flat[K * C]), ari=float(flat[K * C + 1]),
                    purity=float(flat[K * C + 2]), accuracy=float(table[rows, cols].sum()) / n if n else float("nan"),
                    accuracy_computed_on="host", match={int(r): int(c) for r, c in zip(rows, cols)})


def _rows(x, name):
    if x.dim() != 2:
        raise ValueError("kmeans: %s [rows, D] expected, got %s" % (name, tuple(x.shape)))
    if not x.dtype.is_floating_point:
        raise TypeError("kmeans: %s must be a float tensor, got %s" % (name, x.dtype))
    x = x.detach().float()
    if x.shape[0] > 1 and (x.stride(1) != 1 or x.stride(0) < x.shape[1]) or x.shape[0] <= 1 and not x.is_contiguous():
        x = x.contiguous()
    return x


def plan(N, D, K):
    """-> dict(workgroups, row_tile, column_tile, k_chunk, update_chunk, inertia_block) (pn_kmeans_plan; needs no GPU)"""
    out = (ctypes.c_int64 * 6)()
    _lib.check(_lib.load().pn_kmeans_plan(int(N), int(D), int(K), out))
    return dict(zip(("workgroups", "row_tile", "column_tile", "k_chunk", "update_chunk", "inertia_block"), (int(v) for v in out)))


def kmeans(x, clusters, metric="cosine", iters=50, restarts=1, seed=0, init="k-means++", valid=None):
    """k-means of the rows of ``x`` [N, D] (on the GPU) into ``clusters`` groups -> ``Clusters``.

    metric "cosine": rows scaled to unit length (norms in fp64), centroids renormalised means (spherical k-means);
    "euclidean": the rows as they are.  init "k-means++" (seeded by ``seed`` and the restart index, drawn on the device) or
    a [K, D] tensor of starting centroids, used as they are (cosine: pass unit rows), with which restarts must be 1.  Every
    restart runs at most ``iters`` assignments and stops when none moves a row; the restart with the lowest inertia is
    returned (the earliest on equal values).  valid (bool / integer [N], optional): rows with a zero flag are left out, as
    are rows with an entry that is not finite (cosine: or a zero norm): label -1, no cost, in no mean.  A cluster that loses
    all its members keeps its centroid.  Limits: clusters in 1 .. 1024, D in 1 .. 8192, N below 2^31, iters in 1 .. 65536.
    fp32 inputs; other float dtypes are converted.  Row-strided inputs (a column slice) are read in place.  Nothing is read
    back."""
    if x.device.type != "cuda":
        raise RuntimeError("pathnet_amd.kmeans runs on the GPU only (x on %s); no CPU fallback" % x.device)
    z = _rows(x, "x")
    dev = z.device
    N, D = (int(v) for v in z.shape)
    K, iters, restarts = int(clusters), int(iters), int(restarts)
    if not 1 <= K <= MAX_K:
        raise ValueError("kmeans: clusters=%d, 1 .. %d" % (K, MAX_K))
    if not 1 <= D <= MAX_D:
        raise ValueError("kmeans: %d columns, 1 .. %d" % (D, MAX_D))
    if metric not in METRICS:
        raise ValueError("kmeans: metric %r, one of %s" % (metric, sorted(METRICS)))
    if not 1 <= iters <= MAX_ITERS:
        raise ValueError("kmeans: iters=%d, 1 .. %d" % (iters, MAX_ITERS))
    if restarts < 1:
        raise ValueError("kmeans: restarts=%d, at least 1" % restarts)
    start = None
    if isinstance(init, torch.Tensor):
        if init.device != dev:
            raise RuntimeError("kmeans: init on %s, x on %s" % (init.device, dev))
        start = _rows(init, "init")
        if tuple(start.shape) != (K, D):
            raise ValueError("kmeans: init %s, [%d, %d] expected" % (tuple(start.shape), K, D))
        if restarts != 1:
            raise ValueError("kmeans: restarts=%d with an init tensor, 1 expected" % restarts)
    elif init != "k-means++":
        raise ValueError("kmeans: init %r, \"k-means++\" or a [K, D] tensor" % (init,))
    if valid is not None:
        valid = torch.as_tensor(valid).reshape(-1)
        if valid.numel() != N:
            raise ValueError("kmeans: %d valid flags for %d rows" % (valid.numel(), N))
        valid = (valid != 0).to(device=dev, dtype=torch.uint8).contiguous()
    lib = _lib.load()
    need = ctypes.c_int64(0)
    _lib.check(lib.pn_kmeans_workspace_bytes(N, D, K, iters, ctypes.byref(need)))
    with torch.cuda.device(dev):
        ws = torch.empty(need.value, dtype=torch.uint8, device=dev)
        label = torch.empty(N, dtype=torch.int64, device=dev)
        centroid = torch.empty((K, D), dtype=torch.float32, device=dev)
        count = torch.empty(K, dtype=torch.int64, device=dev)
        inertia = torch.empty(1, dtype=torch.float64, device=dev)
        iterations = torch.empty(1, dtype=torch.int32, device=dev)
        moved = torch.empty(iters, dtype=torch.int64, device=dev)
        counts = torch.empty(1, dtype=torch.int64, device=dev)
        out = _lib.KmeansOut(label.data_ptr(), centroid.data_ptr(), count.data_ptr(), inertia.data_ptr(), iterations.data_ptr(),
                             moved.data_ptr(), counts.data_ptr(), None)
        _lib.check(lib.pn_kmeans_run(_lib.context(dev), _lib.ptr(z), z.stride(0) if N > 1 else D, N, D, K, METRICS[metric],
                                     _lib.ptr(valid), _lib.ptr(start), (start.stride(0) if K > 1 else D) if start is not None else 0,
                                     iters, restarts, int(seed) & 0xFFFFFFFFFFFFFFFF, _lib.ptr(ws), ws.numel(), 64,
                                     ctypes.byref(out), _lib.stream_ptr(dev)))
    return Clusters(label, centroid, count, inertia, iterations, moved, counts)


def cluster_scores(pred, truth, num_clusters, num_classes, table=None):
    """A grouping ``pred`` (integer [S], clusters in [0, num_clusters)) against labels ``truth`` (integer [S], classes in
    [0, num_classes)) -> ``ClusterScores``.

    The pairs are added to the contingency table [cluster, class] by integer atomics; a pair with either side outside its
    range (a dead row's -1, an unlabelled node) is counted in ``skipped`` instead.  table (int64 [K, C] on the GPU, optional):
    a table kept from earlier calls, added to in place, so that batches accumulate; the scores are always those of the whole
    table.  NMI, ARI and purity are formed in fp64 by one workgroup in a fixed order.  Limits: num_clusters in 1 .. 1024,
    num_classes in 1 .. 4096.  Nothing is read back."""
    pred = torch.as_tensor(pred).reshape(-1)
    dev = pred.device
    if dev.type != "cuda":
        raise RuntimeError("pathnet_amd.cluster_scores runs on the GPU only (pred on %s); no CPU fallback" % dev)
    truth = torch.as_tensor(truth).reshape(-1)
    if pred.dtype.is_floating_point or truth.dtype.is_floating_point:
        raise TypeError("cluster_scores: pred and truth must be integers, got %s and %s" % (pred.dtype, truth.dtype))
    S = int(pred.numel())
    if int(truth.numel()) != S:
        raise ValueError("cluster_scores: %d labels for %d rows" % (truth.numel(), S))
    K, C = int(num_clusters), int(num_classes)
    if not 1 <= K <= MAX_K:
        raise ValueError("cluster_scores: num_clusters=%d, 1 .. %d" % (K, MAX_K))
    if not 1 <= C <= MAX_CLASSES:
        raise ValueError("cluster_scores: num_classes=%d, 1 .. %d" % (C, MAX_CLASSES))
    pred = pred.to(dtype=torch.int64).contiguous()
    truth = truth.to(device=dev, dtype=torch.int64).contiguous()
    with torch.cuda.device(dev):
        if table is None:
            table = torch.zeros((K, C), dtype=torch.int64, device=dev)
        elif (tuple(table.shape) != (K, C) or table.dtype != torch.int64 or table.device != dev or not table.is_contiguous()):
            raise ValueError("cluster_scores: table must be a contiguous int64 [%d, %d] tensor on %s" % (K, C, dev))
        skipped = torch.zeros(1, dtype=torch.int64, device=dev)
        scores = torch.empty(4, dtype=torch.float64, device=dev)
        _lib.check(_lib.load().pn_cluster_scores(_lib.context(dev), _lib.ptr(pred), K, _lib.ptr(truth), C, S, _lib.ptr(table),
                                                 _lib.ptr(skipped), _lib.ptr(scores), _lib.stream_ptr(dev)))
    return ClusterScores(table, scores[0:1], scores[1:2], scores[2:3], scores[3:4], skipped)
