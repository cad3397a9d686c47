"""Training-loop glue: the reference's ``train_fixed_indices``
(/root/reference/PathNet_run.py:281-403) with everything resident on the GPU.

Same recipe: model by dataset name (:286-291), Adam(lr, weight_decay) + CrossEntropyLoss (:295-297), one training
step per epoch on that epoch's paths (:336-352), validation every epoch (:355-366), test + checkpoint whenever
the validation accuracy improves (:368-389), checkpoint renamed with time stamp and round at the end (:398-401),
returns (macro-F1, micro-F1, macro recall, macro precision, accuracy) of the selected epoch (:403).

What changes is only where the data lives: paths are int32/uint8 device tensors -- either pre-sampled
[epochs, N, W, L] tensors or a MerwSampler that walks each epoch's paths on the GPU just before the step (no
text file, no per-epoch Python parse, PathNet_run.py:317-334) -- masks are index tensors on the device, and the
metrics (sklearn in the reference, :384-389) are computed on the device as well.
"""
import collections
import os
import time

import numpy as np
import torch

from . import modules, optim
from .sampler import DRAW_PHILOX

HOMO_DATASETS = ("cora", "citeseer", "pubmed")          # PathNet_run.py:286


def classification_metrics(y_true, y_pred, num_classes):
    """-> (macro F1, micro F1, macro recall, macro precision, accuracy) with scikit-learn's conventions
    (labels = classes present in y_true or y_pred; 0/0 counts as 0)."""
    y_true, y_pred = y_true.reshape(-1).long(), y_pred.reshape(-1).long()
    conf = torch.bincount(y_true * num_classes + y_pred, minlength=num_classes * num_classes).view(
        num_classes, num_classes).double()
    return metrics_from_confusion(conf)


def metrics_from_confusion(conf):
    """classification_metrics' tuple from a confusion matrix [true, predicted] (any real dtype, any device): the matrix an
    Ensemble counts on the device (Prediction.confusion) needs no per-sample read-back."""
    conf = torch.as_tensor(conf).double()
    tp = conf.diag()
    support, predicted = conf.sum(1), conf.sum(0)
    present = (support + predicted) > 0
    prec = torch.where(predicted > 0, tp / predicted.clamp(min=1), torch.zeros_like(tp))
    rec = torch.where(support > 0, tp / support.clamp(min=1), torch.zeros_like(tp))
    f1 = torch.where(prec + rec > 0, 2 * prec * rec / (prec + rec).clamp(min=1e-300), torch.zeros_like(tp))
    k = present.sum().clamp(min=1)
    acc = tp.sum() / conf.sum().clamp(min=1)
    return (float((f1 * present).sum() / k), float(acc), float((rec * present).sum() / k),
            float((prec * present).sum() / k), float(acc))


def _index_tensor(mask_or_index, device):
    if isinstance(mask_or_index, np.ndarray):
        t = torch.from_numpy(np.flatnonzero(mask_or_index) if mask_or_index.dtype == np.bool_ else mask_or_index)
    else:
        t = torch.as_tensor(mask_or_index)
        if t.dtype == torch.bool:
            t = torch.nonzero(t, as_tuple=False).flatten()
    return t.to(device=device, dtype=torch.int64)


class _EvalDraws:
    """The sampler as train_fixed_indices(eval_samples=K) hands it to model.predict: sample 0 of epoch e is the epoch's own
    draw, samples 1 .. K-1 come from epochs behind the training run's, epochs + e (K-1) + (k-1), which no step uses."""

    def __init__(self, sampler, epoch, epochs, K):
        self.sampler, self.epoch, self.epochs, self.K = sampler, int(epoch), int(epochs), int(K)

    def epoch_of(self, k):
        return self.epoch if k == 0 else self.epochs + self.epoch * (self.K - 1) + (k - 1)

    def sample(self, num_w, seed, epoch_begin=0, epoch_count=1, **kw):
        if epoch_count != 1:
            raise ValueError("one epoch per call")
        return self.sampler.sample(num_w, seed, epoch_begin=self.epoch_of(int(epoch_begin)), epoch_count=1, **kw)


def train_fixed_indices(X, Y, num_classes, data_name, train_indices, val_indices, test_indices, num_w, hid_size,
                        walk_len, paths, round_i=0, *, epochs=1000, lr=0.005, weight_decay=0.0005, dropout=0.7,
                        device="cuda:0", save_dir="./saved_models", sampler_seed=0, model=None, verbose=False,
                        fused_step=None, loss=None, path_weights=None, optimizer=None, eval_samples=1):
    """paths: (ids, codes) tensors [epochs, N, W, L] (int32 / uint8, any device) or a MerwSampler.
    fused_step: True = forward, loss and backward of the training step in one library call (module.forward_loss ->
    pn_pagg_train_step), False = three calls, None = fused exactly when the batch needs micro-batches (then it saves every
    micro-batch's second forward).  Same values.
    loss: a pathnet_amd.CrossEntropyLoss (class weights, ignore_index, label smoothing) handed to forward_loss; None = the
    plain mean.  With ignore_index the training rows may hold unlabelled nodes (Y = the ignore value).
    path_weights: a callable (ids, codes, nodes32, epoch) -> weights [S, W] of the S nodes' paths (or None for that call),
    handed as path_weights= to the training step and to the validation and test forwards: importance weights of a biased
    sampler, pathnet_amd.path_multiplicity, zeros for paths a check found broken.  None: the loop as it is without them.
    optimizer: a callable (parameters) -> optimizer that replaces the built-in Adam(lr, weight_decay) -- pathnet_amd.AdamW
    with max_grad_norm= and schedule=, say; called once, with the model's parameters.  None: the loop as it is.
    eval_samples: K > 1 scores validation and test of an epoch with a K-sample ensemble (model.predict with labels=Y: fp64
    mean of the class probabilities, confusion matrix counted on the device) instead of one draw.  Sample 0 of epoch e is
    today's draw (sampler and tensors: epoch e); samples k = 1 .. K-1 draw from epochs no training step uses -- sampler:
    epochs + e (K-1) + (k-1); tensors: (e + k) % E, which REUSES other epochs' paths.  path_weights then sees that epoch
    number.  The validation accuracy is the trace of the confusion matrix over its sum: one host read per epoch, as now.
    1: the loop exactly as it is without the keyword.
    Returns (test macro-F1, micro-F1, macro recall, macro precision, accuracy) at the best-validation epoch."""
    dev = torch.device(device)
    loss_fn = loss          # (`loss` is the step's value below)
    X = torch.as_tensor(X).to(dev).float()
    Y = torch.as_tensor(Y).to(dev).long()
    tr, va, te = (_index_tensor(m, dev) for m in (train_indices, val_indices, test_indices))
    if model is None:
        cls = modules.PathNet_homo if data_name in HOMO_DATASETS else modules.PathNet
        model = cls(X.shape[-1], hid_size, num_classes, walk_len, dropout=dropout).to(dev)
    if optimizer is None:
        opt = optim.Adam(model.parameters(), lr=lr, weight_decay=weight_decay)     # = torch.optim.Adam, one launch
    else:
        opt = optimizer(model.parameters())
    from_sampler = hasattr(paths, "sample")
    if not from_sampler:
        ids_all, codes_all = (torch.as_tensor(t).to(dev) for t in paths)
    os.makedirs(save_dir, exist_ok=True)
    ckpt = os.path.join(save_dir, data_name + ".pth")
    best_val, result = 0.0, (0.0, 0.0, 0.0, 0.0, 0.0)
    tr32, va32, te32 = tr.to(torch.int32), va.to(torch.int32), te.to(torch.int32)
    if from_sampler:
        # an epoch needs the paths of its train and validation nodes, and the test nodes' only when the validation
        # accuracy improves: three node-list windows of the sampler instead of all N nodes (a walk's draws depend on
        # (epoch, source node, walk) alone: the rows are those of a whole-epoch sample -- tests/test_gpu_sampler.py)
        def paths_of(nodes32, epoch, check=False):
            i, c = paths.sample(num_w, sampler_seed, epoch_begin=epoch, epoch_count=1, draw_source=DRAW_PHILOX,
                                check=check, nodes=nodes32)
            return i[0], c[0]
    else:
        def paths_of(nodes32, epoch, check=False):
            idx = nodes32.long()
            return ids_all[epoch].index_select(0, idx), codes_all[epoch].index_select(0, idx)
    def weights_of(ids, codes, nodes32, epoch):       # the extra keyword of a call, only when the caller weights paths
        return {} if path_weights is None else {"path_weights": path_weights(ids, codes, nodes32, epoch)}
    K = int(eval_samples)
    if K < 1:
        raise ValueError("eval_samples=%d, at least 1" % K)

    def ensemble_eval(epoch, best_val):
        """eval_samples > 1: -> (validation accuracy, test metrics when it beats best_val, else None)"""
        if from_sampler:
            draws, first = _EvalDraws(paths, epoch, epochs, K), 0
            epoch_of = draws.epoch_of
        else:
            draws, first = (ids_all, codes_all), epoch
            epoch_of = lambda k: (epoch + k) % int(ids_all.shape[0])        # noqa: E731
        weigh = None if path_weights is None else (lambda ids, codes, nodes32, k: path_weights(ids, codes, nodes32, epoch_of(k)))
        kw = dict(samples=K, seed=sampler_seed, first_epoch=first, labels=Y, path_weights=weigh)
        conf = model.predict(X, draws, num_w, walk_len, va32, **kw).confusion.double()
        val_acc = float(conf.diag().sum() / conf.sum().clamp(min=1))      # the one host round trip of an epoch
        if not best_val < val_acc:
            return val_acc, None
        torch.save(model.state_dict(), ckpt)
        # (same X, same weights as the validation forwards just above: the test forwards reuse their tables)
        return val_acc, metrics_from_confusion(model.predict(X, draws, num_w, walk_len, te32, reuse_tables=True, **kw).confusion)

    for epoch in range(epochs):
        model.train()
        ids_tr, codes_tr = paths_of(tr32, epoch, check=(epoch == 0))
        loss, out = model.forward_loss(X, ids_tr, num_w, walk_len, tr32, codes_tr, Y[tr], fused=fused_step, loss=loss_fn,
                                       **weights_of(ids_tr, codes_tr, tr32, epoch))
        opt.zero_grad(set_to_none=True)
        optim.backward(loss)        # = loss.backward(), minus the seed gradient's fill and multiply
        opt.step()
        with torch.no_grad():
            model.eval()
            if K > 1:
                val_acc, improved = ensemble_eval(epoch, best_val)
                if improved is not None:
                    best_val, result = val_acc, improved
            else:
                ids_va, codes_va = paths_of(va32, epoch)
                pred = model(X, ids_va, num_w, walk_len, va32, codes_va, None,
                             **weights_of(ids_va, codes_va, va32, epoch)).argmax(1)
                val_acc = float((pred == Y[va]).double().mean())      # the one host round trip of an epoch
                if best_val < val_acc:
                    best_val = val_acc
                    torch.save(model.state_dict(), ckpt)
                    # same X, same weights as the validation forward just above: its projected features and distance
                    # bank are still in the module's workspace (PathNet_run.py:362 and :378 recompute them)
                    ids_te, codes_te = paths_of(te32, epoch)
                    pred = model(X, ids_te, num_w, walk_len, te32, codes_te, None, reuse_tables=True,
                                 **weights_of(ids_te, codes_te, te32, epoch)).argmax(1)
                    result = classification_metrics(Y[te], pred, num_classes)
        if verbose and (epoch % 50 == 0 or epoch == epochs - 1):
            print("epoch %d loss %.4f val_acc %.4f test_acc %.4f" % (epoch, float(loss), val_acc, result[4]))
    if os.path.exists(ckpt):
        os.rename(ckpt, os.path.join(save_dir, data_name + time.strftime("%Y-%m-%d_%H:%M:%S", time.localtime())
                                     + str(round_i) + ".pth"))
    return result


Pretrained = collections.namedtuple("Pretrained", ("loss", "hits", "pairs"))
Pretrained.__doc__ = """Device tensors of a pretrain() run, one entry per step: loss float32 [steps], hits int64 [steps] (rows whose
partner had the largest logit, of 2 * pairs), pairs int64 [steps] (live pairs of the step)."""


def pretrain_seed(seed, step, view):
    """the dropout seed of view `view` (0 / 1) of step `step` of a pretrain(seed=) run"""
    return (int(seed) * 1000003 + 2 * int(step) + int(view)) & ((1 << 62) - 1)


def pretrain(model, X, paths, num_w, walk_len, nodes=None, *, epochs, batch_nodes=None, temperature=0.5, intra=True,
             head=None, optimizer=None, lr=1e-3, seed=0, first_epoch=0):
    """Self-supervised pretraining of an aggregator on unlabelled nodes -> ``Pretrained(loss, hits, pairs)``.

    Two independent path draws of a node are two views of it.  Every epoch takes `nodes` (a bool mask or node ids, default all
    N) in batches of batch_nodes (default: all of them); step t over a batch
      - draws view 1 as path draw first_epoch + 2t and view 2 as draw first_epoch + 2t + 1 -- `paths` follows predict()'s
        convention: a sampler (``smp.biased(p, q)`` included; sampled with `seed` and ``nodes=``) or pre-sampled
        ``(ids, codes)`` tensors [E, N, W, L], where draw k is epoch k % E;
      - runs two ``model.encode(...)`` calls in training mode, so dropout differs between the views as well
        (``seed=pretrain_seed(seed, t, view)``), both in one autograd graph;
      - takes z = head(embedding) when a ``torch.nn.Module`` head is given (a 2-layer MLP, say), else the embedding itself;
      - ``pathnet_amd.contrastive_loss(z1, z2, temperature, intra)``, ``pathnet_amd.backward``, the optimizer's step.
    optimizer: a callable (parameters) -> optimizer; None: ``pathnet_amd.Adam(lr)`` over the model's and the head's parameters.
    After the first step (whose sampler calls run the sampler's own check) the loop reads nothing back: loss, hits and
    pairs are written into device tensors by index.
    PathNet (the hetero class): a row pools sequences made of OTHER masked nodes' paths of its batch (encode()'s doc string),
    so its embedding, and with it what is being pretrained, is a property of (node, batch).
    Not supported: the aggregators of pathnet_amd.dist (no negatives across ranks), path_grad, and capturing the loop into a
    hipGraph (the sampler and the workspaces allocate)."""
    from . import contrast
    from . import ensemble as ens
    dev = X.device
    if dev.type != "cuda":
        raise RuntimeError("pathnet_amd aggregators run on the GPU only (X is on %s); no CPU fallback" % dev)
    W, L, N = int(num_w), int(walk_len), int(X.shape[0])
    nodes32 = ens._node_list(nodes, N, dev)
    S = int(nodes32.numel())
    if S < 1 or int(epochs) < 0:
        raise ValueError("pretrain: %d nodes, %d epochs" % (S, int(epochs)))
    batch = S if batch_nodes is None else max(1, min(int(batch_nodes), S))
    from_sampler = hasattr(paths, "sample")
    if from_sampler:
        def paths_of(sel32, k, check):       # (the sampler's own check reads one word back: the first step alone asks for it)
            i, c = paths.sample(W, seed, epoch_begin=k, epoch_count=1, draw_source=DRAW_PHILOX, check=check, nodes=sel32)
            return i[0], c[0]
    else:
        ids_all, codes_all = (torch.as_tensor(t).to(dev) for t in paths)
        E = int(ids_all.shape[0])
        if E < 1 or tuple(ids_all.shape[1:]) != (N, W, L) or tuple(codes_all.shape) != tuple(ids_all.shape):
            raise ValueError("pretrain: paths (ids, codes) of shape [E, %d, %d, %d] expected, got %s / %s"
                             % (N, W, L, tuple(ids_all.shape), tuple(codes_all.shape)))

        def paths_of(sel32, k, check):
            idx = sel32.long()
            return ids_all[k % E].index_select(0, idx), codes_all[k % E].index_select(0, idx)

    params = list(model.parameters()) + (list(head.parameters()) if head is not None else [])
    opt = optim.Adam(params, lr=lr) if optimizer is None else optimizer(params)
    chunks = [nodes32[b0:b0 + batch] for b0 in range(0, S, batch)]
    steps = int(epochs) * len(chunks)
    loss_t = torch.zeros(steps, dtype=torch.float32, device=dev)
    hits_t = torch.zeros(steps, dtype=torch.int64, device=dev)
    pairs_t = torch.zeros(steps, dtype=torch.int64, device=dev)
    was_training = model.training
    head_training = head.training if head is not None else None
    model.train()
    if head is not None:
        head.train()
    try:
        for t in range(steps):
            sel = chunks[t % len(chunks)]
            z = []
            for view in (0, 1):
                ids, codes = paths_of(sel, int(first_epoch) + 2 * t + view, t == 0)
                emb = model.encode(X, ids, W, L, sel, codes, None, seed=pretrain_seed(seed, t, view)).embedding
                z.append(head(emb) if head is not None else emb)
            c = contrast.contrastive_loss(z[0], z[1], temperature=temperature, intra=intra)
            opt.zero_grad(set_to_none=True)
            optim.backward(c.loss)
            opt.step()
            loss_t[t:t + 1].copy_(c.loss.detach().reshape(1))
            hits_t[t:t + 1].copy_(c.hits)
            pairs_t[t:t + 1].copy_(c.counts[:1])
    finally:
        model.train(was_training)
        if head is not None:
            head.train(head_training)
    return Pretrained(loss_t, hits_t, pairs_t)
