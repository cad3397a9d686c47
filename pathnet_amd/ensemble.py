"""Ensemble prediction over resampled paths (pn_ensemble_add / pn_ensemble_finish, pn_ensemble.hip).

The logits of a node depend on the W paths the sampler drew for it.  An ``Ensemble`` keeps, per node, the sum of the class
probabilities of every draw it was given (fp64, on the device), the votes and the per-draw entropies; ``result()`` turns
them into a ``Prediction`` of device tensors and ``summary()`` makes the one host read.  ``model.predict(...)`` of the
aggregator classes drives it; ``predict_with`` below is that method's body.
"""
import collections
import ctypes

import numpy as np
import torch

from . import _lib

STACK_NODES = 1 << 15       # predict's default stacking: samples of a chunk share a forward up to this many rows

FIELDS = ("prob", "label", "vote_label", "confidence", "entropy", "mutual_info", "agreement", "count", "bad", "confusion",
          "skipped")


class Prediction(collections.namedtuple("Prediction", FIELDS)):
    """Device tensors, one row per node of the ensemble (or of ``rows=``):
    prob float32 [S, C]       mean class probabilities over the samples
    label int64 [S]           argmax of prob (lowest class on ties); -1 for a node without a valid sample
    vote_label int64 [S]      the class most samples voted for
    confidence float32 [S]    prob[label]
    entropy float32 [S]       entropy of the mean distribution (nats)
    mutual_info float32 [S]   entropy minus the mean entropy of the samples: the uncertainty that comes from the path draw
    agreement float32 [S]     share of the samples whose own argmax is `label`
    count, bad int32 [S]      samples averaged / samples refused because a logit was not finite
    confusion int64 [C, C]    [true, predicted], with labels= only (else None)
    skipped int64 [2]         {labels outside [0, C), nodes with label -1}, with labels= only (else None)"""
    __slots__ = ()

    def summary(self):
        """A dict of Python numbers (one host read): rows, bad_share, mean_agreement and, with a confusion matrix, accuracy,
        macro_f1, micro_f1, macro_recall, macro_precision and the two skipped counts."""
        from .trainer import metrics_from_confusion
        C = self.prob.shape[1]
        rows = self.label.numel()
        valid = self.label >= 0
        head = torch.stack((valid.sum().double(), (self.bad > 0).sum().double(),
                            (self.agreement.double() * valid).sum()))
        parts = [head]
        if self.confusion is not None:
            parts += [self.confusion.reshape(-1).double(), self.skipped.double()]
        flat = torch.cat(parts).cpu().numpy()
        out = dict(rows=rows, valid_rows=int(flat[0]), bad_share=float(flat[1]) / rows if rows else 0.0,
                   mean_agreement=float(flat[2] / flat[0]) if flat[0] else 0.0)
        if self.confusion is not None:
            conf = torch.from_numpy(flat[3:3 + C * C].reshape(C, C).copy())
            f1, micro, rec, prec, acc = metrics_from_confusion(conf)
            out.update(accuracy=acc, macro_f1=f1, micro_f1=micro, macro_recall=rec, macro_precision=prec,
                       labels_out_of_range=int(flat[3 + C * C]), unlabelled_rows=int(flat[4 + C * C]))
        return out

    def calibration(self, labels, bins=15, curve=True):
        """How far the confidences can be trusted, against ``labels`` (int [rows of this Prediction]) -> a
        ``pathnet_amd.Calibration`` of device tensors: reliability bins (``bins`` of them, 1 .. 1024), ece, mce, nll, brier
        and, with curve=True, the risk-coverage order, err_prefix and aurc (pn_calib_stats; nothing read back)."""
        from .calibration import calibration_of
        return calibration_of(self, labels, bins=bins, curve=curve)


class Ensemble:
    """Running ensemble of `rows` nodes over `num_classes` classes on `device` (1 <= num_classes <= 4096).

    add(logits, index=None)   one sample ``[S, C]`` or R samples ``[R, S, C]`` of the same S nodes (fp32); index (int [S])
                              names the ensemble row of logits row s, default row s.
    result(labels=None, rows=None) -> Prediction
    reset()                   an empty ensemble again
    temperature: None, or a float or 1-element fp64 device tensor (a ``Temperature.tau``): every add divides the logits'
    distance to their maximum by it before the softmax (pn_ensemble_add_scaled; the tensor is read on the device).  A
    temperature that is not finite and positive adds nothing and counts the refused logits rows in ``status``.
    Everything is enqueued on the current stream; nothing is read back except by check=True and Prediction.summary()."""

    def __init__(self, rows, num_classes, device="cuda", temperature=None):
        self.rows, self.num_classes = int(rows), int(num_classes)
        dev = torch.device(device)
        if dev.type != "cuda":
            raise RuntimeError("pathnet_amd.Ensemble runs on the GPU only (device %s); no CPU fallback" % dev)
        self.device = dev if dev.index is not None else torch.device("cuda", torch.cuda.current_device())
        need = ctypes.c_int64(0)
        _lib.check(_lib.load().pn_ensemble_state_bytes(self.rows, self.num_classes, ctypes.byref(need)))   # refuses a bad shape
        self.state = torch.zeros(max(need.value, 8), dtype=torch.uint8, device=self.device)    # (the allocator aligns it)
        self.status = torch.zeros(1, dtype=torch.int32, device=self.device)     # logits rows whose index was out of range
        self.temperature = None
        if temperature is not None:
            if torch.is_tensor(temperature):
                if temperature.numel() != 1:
                    raise ValueError("Ensemble: temperature must hold one value, got %s" % (tuple(temperature.shape),))
                tau = temperature.detach().reshape(1).to(device=self.device, dtype=torch.float64)
            else:
                tau = torch.tensor([float(temperature)], dtype=torch.float64, device=self.device)
            self.temperature = tau.contiguous()

    # ---- views of the state (include/pathnet_hip.h: psum, hsum, votes, count, bad) ---------------------------------------
    def _views(self):
        n, C = self.rows, self.num_classes
        f = self.state[:8 * (n * C + n)].view(torch.float64)
        i = self.state[8 * (n * C + n):8 * (n * C + n) + 4 * (n * C + 2 * n)].view(torch.int32)
        return (f[:n * C].view(n, C), f[n * C:], i[:n * C].view(n, C), i[n * C:n * C + n], i[n * C + n:n * C + 2 * n])

    psum = property(lambda self: self._views()[0])
    hsum = property(lambda self: self._views()[1])
    votes = property(lambda self: self._views()[2])
    count = property(lambda self: self._views()[3])
    bad = property(lambda self: self._views()[4])

    def reset(self):
        self.state.zero_()
        self.status.zero_()
        return self

    def add(self, logits, index=None, check=False):
        """check=True: raise on an index entry outside [0, rows) or named twice (one host read)."""
        x = logits.detach()
        if x.dim() == 2:
            x = x.unsqueeze(0)
        if x.dim() != 3 or x.shape[2] != self.num_classes:
            raise ValueError("Ensemble.add: logits [S, %d] or [R, S, %d] expected, got %s"
                             % (self.num_classes, self.num_classes, tuple(logits.shape)))
        if x.device != self.device:
            raise ValueError("Ensemble.add: logits on %s, the ensemble is on %s" % (x.device, self.device))
        x = x.float().contiguous()
        R, S, C = (int(v) for v in x.shape)
        if R < 1:
            raise ValueError("Ensemble.add: no samples")
        if index is not None:
            index = torch.as_tensor(index)
            if index.dtype.is_floating_point or index.dtype == torch.bool or index.numel() != S:
                raise ValueError("Ensemble.add: index must hold %d integers" % S)
            index = index.reshape(-1).to(device=self.device, dtype=torch.int32).contiguous()
            if check and S:
                inside = (index >= 0) & (index < self.rows)
                seen = torch.bincount(index[inside].long(), minlength=max(self.rows, 1))
                if not bool(inside.all()) or int(seen.max()) > 1:
                    raise ValueError("Ensemble.add: index entries outside [0, %d) or named twice" % self.rows)
        elif S > self.rows:
            raise ValueError("Ensemble.add: %d logits rows for an ensemble of %d and no index" % (S, self.rows))
        with torch.cuda.device(self.device):
            if self.temperature is None:
                _lib.check(_lib.load().pn_ensemble_add(_lib.context(self.device), _lib.ptr(x), R, S, C, _lib.ptr(index),
                                                       self.rows, _lib.ptr(self.state), _lib.ptr(self.status),
                                                       _lib.stream_ptr(self.device)))
            else:
                _lib.check(_lib.load().pn_ensemble_add_scaled(_lib.context(self.device), _lib.ptr(x), R, S, C, _lib.ptr(index),
                                                              self.rows, _lib.ptr(self.state), _lib.ptr(self.status),
                                                              _lib.ptr(self.temperature), _lib.stream_ptr(self.device)))
        return self

    def result(self, labels=None, rows=None):
        """labels (int [rows of the ensemble]): also the confusion matrix [true, predicted] and the skipped counts.
        rows (int [n] ensemble rows, or a bool mask over them): the Prediction of those rows only, in that order."""
        dev, C = self.device, self.num_classes
        subset = None
        if rows is not None:
            subset = torch.as_tensor(rows)
            if subset.dtype == torch.bool:
                subset = torch.nonzero(subset.reshape(-1), as_tuple=False).flatten()
            subset = subset.reshape(-1).to(device=dev, dtype=torch.int32).contiguous()
        n = self.rows if subset is None else int(subset.numel())
        target = None
        if labels is not None:
            target = torch.as_tensor(labels).reshape(-1).to(device=dev, dtype=torch.int64).contiguous()
            if target.numel() != self.rows:
                raise ValueError("Ensemble.result: %d labels for %d rows" % (target.numel(), self.rows))
        with torch.cuda.device(dev):
            f = torch.empty((4, n), dtype=torch.float32, device=dev)
            lab = torch.empty((2, n), dtype=torch.int64, device=dev)
            prob = torch.empty((n, C), dtype=torch.float32, device=dev)
            confusion = torch.zeros((C, C), dtype=torch.int64, device=dev) if target is not None else None
            skipped = torch.zeros(2, dtype=torch.int64, device=dev) if target is not None else None
            out = _lib.EnsembleOut(prob.data_ptr(), lab[0].data_ptr(), lab[1].data_ptr(), f[0].data_ptr(), f[1].data_ptr(),
                                   f[2].data_ptr(), f[3].data_ptr(), _lib.ptr(confusion), _lib.ptr(skipped))
            _lib.check(_lib.load().pn_ensemble_finish(_lib.context(dev), self.rows, C, _lib.ptr(self.state), _lib.ptr(subset),
                                                      n if subset is not None else 0, _lib.ptr(target), ctypes.byref(out),
                                                      _lib.stream_ptr(dev)))
            count, bad = self.count, self.bad
            if subset is not None:
                at = subset.long().clamp(0, max(self.rows - 1, 0))
                inside = (subset >= 0) & (subset < self.rows)
                count = torch.where(inside, count[at], 0) if self.rows else torch.zeros_like(subset)
                bad = torch.where(inside, bad[at], 0) if self.rows else torch.zeros_like(subset)
            else:
                count, bad = count.clone(), bad.clone()
        return Prediction(prob, lab[0], lab[1], f[0], f[1], f[2], f[3], count, bad, confusion, skipped)

    def summary(self, labels=None, rows=None):
        """result(labels, rows).summary(): the one host read"""
        return self.result(labels, rows).summary()


def _node_list(nodes, N, dev):
    """nodes= of predict (a mask or node ids, the rules of modules._as_index_tensors) -> int32 ids on dev"""
    if nodes is None:
        return torch.arange(N, dtype=torch.int32, device=dev)
    if isinstance(nodes, np.ndarray):
        nodes = torch.from_numpy(np.flatnonzero(nodes) if nodes.dtype == np.bool_ else np.ascontiguousarray(nodes))
    t = torch.as_tensor(nodes)
    if t.dtype == torch.bool:
        t = torch.nonzero(t.reshape(-1), as_tuple=False).flatten()
    elif t.dtype.is_floating_point or t.dtype.is_complex:
        raise TypeError("predict: nodes must be a bool mask or integer node ids, got %s" % t.dtype)
    return t.reshape(-1).to(device=dev, dtype=torch.int32).contiguous()


def predict_with(model, X, paths, num_w, walk_len, nodes=None, *, samples=8, seed=0, first_epoch=0, batch_nodes=None,
                 samples_per_call=None, labels=None, path_weights=None, path_weight_norm="sum", ensemble=None, reuse_tables=False,
                 temperature=None, collect=None, embedding=False):
    """The body of ``model.predict`` (modules._Aggregator.predict carries the documentation).
    collect (``model.calibrate``): a callable ``collect(logits [R, cnt, C], k0, b0)`` that is handed every forward's logits --
    samples k0 .. k0 + R - 1 of nodes b0 .. b0 + cnt - 1 of the node list -- in place of an ensemble; nothing is returned.
    embedding (``model.embed``; needs collect): the forwards are ``model.encode`` calls and collect is handed their
    embeddings [R, cnt, 2H] in place of the logits."""
    from . import modules
    from .sampler import DRAW_PHILOX
    dev = X.device
    if dev.type != "cuda":
        raise RuntimeError("pathnet_amd aggregators run on the GPU only (X is on %s); no CPU fallback" % dev)
    K, W, L = int(samples), int(num_w), int(walk_len)
    if K < 1:
        raise ValueError("predict: samples=%d, at least 1" % K)
    N, C = int(X.shape[0]), int(model.out_size)
    nodes32 = _node_list(nodes, N, dev)
    S = int(nodes32.numel())
    from_sampler = hasattr(paths, "sample")
    if from_sampler:
        def paths_of(sel32, k):
            i, c = paths.sample(W, seed, epoch_begin=int(first_epoch) + k, epoch_count=1, draw_source=DRAW_PHILOX, nodes=sel32)
            return i[0], c[0]
    else:
        ids_all, codes_all = (torch.as_tensor(t).to(dev) for t in paths)
        E = int(ids_all.shape[0])
        if E < 1 or tuple(ids_all.shape[1:]) != (N, W, L) or tuple(codes_all.shape) != tuple(ids_all.shape):
            raise ValueError("predict: paths (ids, codes) of shape [E, %d, %d, %d] expected, got %s / %s"
                             % (N, W, L, tuple(ids_all.shape), tuple(codes_all.shape)))

        def paths_of(sel32, k):
            e, idx = (int(first_epoch) + k) % E, sel32.long()
            return ids_all[e].index_select(0, idx), codes_all[e].index_select(0, idx)

    def weights_of(ids, codes, sel32, k):
        if path_weights is None:
            return None
        w = path_weights(ids, codes, sel32, k)
        return None if w is None else modules.as_path_weights(w, int(sel32.numel()), W).to(dev)

    if embedding and collect is None:
        raise ValueError("predict: embedding= hands the embeddings to collect=")

    def forward(ids, sel, codes, **kw):
        if embedding:
            return model.encode(X, ids, W, L, sel, codes, None, **kw).embedding
        return model(X, ids, W, L, sel, codes, None, **kw)

    if collect is not None:
        if ensemble is not None or temperature is not None or labels is not None:
            raise ValueError("predict: collect= takes the logits as they are; no ensemble, temperature or labels")
    elif ensemble is None:
        ensemble = Ensemble(S, C, dev, temperature=temperature)
    elif temperature is not None:
        raise ValueError("predict: temperature= belongs to the ensemble that is passed in (Ensemble(temperature=))")
    elif ensemble.rows != S or ensemble.num_classes != C or ensemble.device != nodes32.device:
        raise ValueError("predict: ensemble of %d rows x %d classes on %s, the call has %d nodes x %d classes on %s"
                         % (ensemble.rows, ensemble.num_classes, ensemble.device, S, C, nodes32.device))
    hetero = model.variant == "hetero"
    if batch_nodes is None:
        # what one call's workspace allows: the library's own micro-batches take care of a large batch, so the default is
        # the whole node list (pick_batch_groups / default_budget inside forward)
        batch_nodes = max(S, 1)
    batch_nodes = max(1, min(int(batch_nodes), max(S, 1)))
    if samples_per_call is None:
        # stack until a call carries about as many nodes as a mid-sized batch (a small graph then fills the GPU)
        per_call = max(1, min(K, STACK_NODES // batch_nodes))
    else:
        per_call = max(1, min(int(samples_per_call), K))
    # (a hetero row reads paths of the batch's other nodes: a sample is one whole-batch forward, samples_per_call is ignored)
    was_training = model.training
    model.eval()
    try:
        with torch.no_grad():
            fresh = not reuse_tables    # the first forward computes fc0 and the bank; every later one of this predict reuses them
            if hetero:
                for k in range(K):
                    ids, codes = paths_of(nodes32, k)
                    w = weights_of(ids, codes, nodes32, k)
                    for b0 in range(0, S, batch_nodes):
                        cnt = min(batch_nodes, S - b0)
                        out = forward(ids, nodes32, codes, reuse_tables=not fresh, group_slice=(b0, cnt), path_weights=w,
                                      path_weight_norm=path_weight_norm)
                        fresh = False
                        if collect is not None:
                            collect(out.reshape(1, cnt, -1) if embedding else out.view(1, cnt, C), k, b0)
                        else:
                            ensemble.add(out, index=torch.arange(b0, b0 + cnt, dtype=torch.int32, device=dev))
            else:
                for b0 in range(0, S, batch_nodes):
                    sel = nodes32[b0:b0 + batch_nodes]
                    cnt = int(sel.numel())
                    index = torch.arange(b0, b0 + cnt, dtype=torch.int32, device=dev)
                    for k0 in range(0, K, per_call):
                        R = min(per_call, K - k0)
                        drawn = [paths_of(sel, k) for k in range(k0, k0 + R)]
                        ws = [weights_of(i, c, sel, k0 + j) for j, (i, c) in enumerate(drawn)]
                        if any(w is None for w in ws) and not all(w is None for w in ws):
                            raise ValueError("predict: path_weights returned None for some samples of a stacked call and "
                                             "weights for others; use samples_per_call=1")
                        ids = torch.cat([i for i, _ in drawn]) if R > 1 else drawn[0][0]
                        codes = torch.cat([c for _, c in drawn]) if R > 1 else drawn[0][1]
                        w = None if ws[0] is None else (torch.cat(ws) if R > 1 else ws[0])
                        out = forward(ids, sel.repeat(R) if R > 1 else sel, codes, reuse_tables=not fresh, path_weights=w,
                                      path_weight_norm=path_weight_norm)
                        fresh = False
                        if collect is not None:
                            collect(out.reshape(R, cnt, -1) if embedding else out.view(R, cnt, C), k0, b0)
                        else:
                            ensemble.add(out.view(R, cnt, C), index=index)
    finally:
        model.train(was_training)
    if collect is not None:
        return None
    if labels is not None:
        labels = torch.as_tensor(labels).reshape(-1).to(dev)
        if labels.numel() == N:
            labels = labels.index_select(0, nodes32.long())       # labels of all N nodes: the node list's are picked
        elif labels.numel() != S:
            raise ValueError("predict: %d labels for %d nodes (of %d)" % (labels.numel(), S, N))
    return ensemble.result(labels=labels)
