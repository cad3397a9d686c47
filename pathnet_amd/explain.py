"""Explanations: which paths a prediction rests on (pn_explain_groups / pn_explain_totals, pn_explain.hip).

The aggregators classify a node from the W paths around it.  ``model.explain(...)`` says what the model would answer without
a group of a node's paths (``drop_delta``, ``flip``) and with that group alone (``keep_gain``), for every group of every
node, from ONE ``encode(path_state=True)`` forward: the recurrence never sees the pooling, and the classifier is linear after
it, so every leave-out and keep-only answer is a closed form over the paths' final hidden states, which one kernel evaluates
in fp64 on the device (include/pathnet_hip.h has the definition).  By construction ``drop_logits[:, g]`` is the model's own
``forward(path_weights=...)`` with the members of group g given weight 0, and ``keep_logits[:, g]`` the forward with every
other member given weight 0 -- at the cost of one forward instead of 2 G + 1.

Not covered: the attribution of single steps or nodes inside a path (the recurrence is not linear), the node-sharded and
replicated aggregators of pathnet_amd.dist, and training mode (explain runs the model in eval mode under no_grad).
"""
import collections
import ctypes

import torch

from . import _lib

FIELDS = ("logits", "drop_delta", "keep_gain", "flip", "present", "target", "drop_logits", "keep_logits", "contribution",
          "totals")


class Totals:
    """Per-group running totals over every row the explain calls have added (views of ONE device buffer, ``state``: 40 G
    bytes, the layout of pn_explain_totals); pass it as ``totals=`` to continue it:
    rows_present int64 [G]      rows in which the group had a live member (and finite scores)
    members int64 [G]           live members of the group over those rows
    flips int64 [G]             rows whose argmax changes without the group
    drop_delta_sum, keep_gain_sum float64 [G]   sums of the scores over those rows"""

    def __init__(self, num_groups, device="cuda", state=None):
        self.num_groups = G = int(num_groups)
        self.state = torch.zeros(40 * G, dtype=torch.uint8, device=device) if state is None else state
        if self.state.numel() != 40 * G or self.state.dtype != torch.uint8:
            raise ValueError("Totals: a uint8 buffer of %d bytes expected" % (40 * G))

    def _i(self, k):
        G = self.num_groups
        return self.state[8 * G * k:8 * G * (k + 1)].view(torch.int64)

    def _f(self, k):
        G = self.num_groups
        return self.state[8 * G * (3 + k):8 * G * (4 + k)].view(torch.float64)

    rows_present = property(lambda self: self._i(0))
    members = property(lambda self: self._i(1))
    flips = property(lambda self: self._i(2))
    drop_delta_sum = property(lambda self: self._f(0))
    keep_gain_sum = property(lambda self: self._f(1))


class Explanation(collections.namedtuple("Explanation", FIELDS)):
    """Device tensors, one row per explained node, G groups:
    logits float32 [S, C]           encode()'s logits of the unchanged row, on the plain inference path (PN_EVAL_ZW off: bits that
                                    do not depend on batch_nodes; within the forward's 1e-5 of forward()'s)
    drop_delta float32 [S, G]       log p(target) of the row minus log p(target) without group g: positive = the group supports it
    keep_gain float32 [S, G]        log p(target) with group g alone minus log p(target) with no path at all
    flip uint8 [S, G]               the argmax changes without group g (and the group has a live member)
    present int32 [S, G]            live members of group g in the row
    target int64 [S]                the class the scores refer to: target=, or the argmax of the row's logits
    drop_logits, keep_logits float32 [S, G, C]   with logits=True, else None
    contribution float32 [S, W, C]  with contribution=True: member j's share of the logits, logits = e + sum_j contribution
    totals                          the Totals over every row of this call and of the totals= it continued"""
    __slots__ = ()

    def top(self, k):
        """torch.topk of drop_delta over the groups -> (values [S, k], group ids [S, k]); groups without a live member in the
        row rank last"""
        score = torch.where(self.present > 0, self.drop_delta, torch.full_like(self.drop_delta, float("-inf")))
        return torch.topk(score, min(int(k), score.shape[1]), dim=1)

    def summary(self):
        """The one host read -> a list of G dicts: group, rows_present, members, mean_drop_delta, mean_keep_gain, flip_rate
        (means over the rows in which the group is present)"""
        t = self.totals
        G = t.num_groups
        raw = t.state.cpu().numpy()
        rows, mem, flips = raw[:24 * G].view("int64").reshape(3, G)
        dd, kg = raw[24 * G:].view("float64").reshape(2, G)
        out = []
        for g in range(G):
            n = rows[g]
            out.append(dict(group=g, rows_present=int(n), members=int(mem[g]), mean_drop_delta=float(dd[g] / n) if n else 0.0,
                            mean_keep_gain=float(kg[g] / n) if n else 0.0, flip_rate=float(flips[g] / n) if n else 0.0))
        return out


def reach_groups(layer_type, S, W, L, device):
    """groups="reach": the largest distance code along each path, int32 [S, W]"""
    codes = torch.as_tensor(layer_type).to(device).reshape(S, W, L)
    return codes.to(torch.int32).amax(dim=2).contiguous()


def explain_groups(state, coef, ego, fc2_w, fc2_b, group, G, *, weight=None, norm=_lib.PATH_NORM_SUM, renorm=False, target=None,
                   logits=False, contribution=False, totals=None):
    """One pn_explain_groups call (and its pn_explain_totals) on tensors in encode()'s member order:
    state [S, W, H], coef [S, W], ego [S, >= H] (a view of the embedding will do), fc2_w [C, 2H], fc2_b [C], group int32 [S, W],
    weight [S, W] or None, totals a Totals or None -> (dict of the kernel's outputs, Totals)."""
    dev = state.device
    S, W, H = (int(v) for v in state.shape)
    C = int(fc2_w.shape[0])
    state = state.contiguous()
    if ego.stride(-1) != 1:
        ego = ego.contiguous()
    ld_state, ld_ego = H, max(int(ego.stride(0)), H)
    fc2_w, fc2_b = fc2_w.detach().float().contiguous(), fc2_b.detach().float().contiguous()
    coef, group = coef.float().contiguous(), group.to(device=dev, dtype=torch.int32).contiguous()
    if tuple(group.shape) != (S, W):
        raise ValueError("explain: groups of shape %s, [%d, %d] expected" % (tuple(group.shape), S, W))
    if weight is not None:
        weight = weight.to(device=dev, dtype=torch.float32).contiguous()
    if target is not None:
        target = target.to(device=dev, dtype=torch.int64).contiguous()
    with torch.cuda.device(dev):
        f = torch.empty((2, S, G), dtype=torch.float32, device=dev)
        out = dict(full=None, drop_delta=f[0], keep_gain=f[1],        # (full: encode's logits are the caller's)
                   flip=torch.empty((S, G), dtype=torch.uint8, device=dev),
                   present=torch.empty((S, G), dtype=torch.int32, device=dev),
                   target_used=torch.empty(S, dtype=torch.int64, device=dev),
                   drop_logits=torch.empty((S, G, C), dtype=torch.float32, device=dev) if logits else None,
                   keep_logits=torch.empty((S, G, C), dtype=torch.float32, device=dev) if logits else None,
                   contribution=torch.empty((S, W, C), dtype=torch.float32, device=dev) if contribution else None)
        if totals is None:
            totals = Totals(G, dev)
        desc = _lib.ExplainOut(*(_lib.ptr(out[k]) for k in _lib.ExplainOut.FIELDS))
        lib, ctx, stream = _lib.load(), _lib.context(dev), _lib.stream_ptr(dev)
        _lib.check(lib.pn_explain_groups(ctx, S, W, H, C, G, _lib.ptr(state), ld_state, _lib.ptr(coef), _lib.ptr(ego), ld_ego,
                                         _lib.ptr(fc2_w), 2 * H, _lib.ptr(fc2_b), _lib.ptr(weight), _lib.ptr(group), int(norm),
                                         int(bool(renorm)), _lib.ptr(target), ctypes.byref(desc), None, stream))
        _lib.check(lib.pn_explain_totals(ctx, S, G, _lib.ptr(out["drop_delta"]), _lib.ptr(out["keep_gain"]),
                                         _lib.ptr(out["flip"]), _lib.ptr(out["present"]), None, 0, _lib.ptr(totals.state), stream))
    return out, totals


def explain(model, X, neis, num_w, walk_len, indices, layer_type, *, groups="path", num_groups=None, target=None,
            path_weights=None, path_weight_norm="sum", batch_nodes=None, logits=False, contribution=False, totals=None):
    """The body of ``model.explain`` (modules._Aggregator.explain carries the documentation)."""
    from . import modules
    dev = X.device
    if dev.type != "cuda":
        raise RuntimeError("pathnet_amd aggregators run on the GPU only (X is on %s); no CPU fallback" % dev)
    if path_weight_norm not in modules._PATH_NORM:
        raise ValueError("path_weight_norm=%r: 'sum' or 'count'" % (path_weight_norm,))
    W, L, H = int(num_w), int(walk_len), int(model.hidden_size)
    hetero = model.variant == "hetero"
    ids, codes, sel, S = modules._as_index_tensors(neis, layer_type, indices, W, L, dev, n_nodes=X.shape[0])
    # ---- the groups, [S, W] int32 in member order ----------------------------------------------------------------------------
    if isinstance(groups, str):
        if groups == "path":
            group, G = torch.arange(W, dtype=torch.int32, device=dev).repeat(S, 1), W
        elif groups == "reach":
            if hetero:
                raise ValueError('groups="reach": PathNet_homo / PAGG only -- a PathNet member is a slot of the scrambled batch '
                                 "whose steps come from other nodes' paths; pass an explicit [S, W] tensor in member order")
            group, G = reach_groups(codes, S, W, L, dev), L
        else:
            raise ValueError("groups=%r: 'path', 'reach' or an int tensor [S, W]" % (groups,))
        if num_groups is not None and int(num_groups) != G:
            raise ValueError("groups=%r has %d groups, num_groups=%d" % (groups, G, int(num_groups)))
    else:
        group = torch.as_tensor(groups)
        if group.dtype.is_floating_point or group.dtype == torch.bool or tuple(group.shape) != (S, W):
            raise ValueError("groups: 'path', 'reach' or an int tensor [%d, %d] in member order" % (S, W))
        group = group.to(device=dev, dtype=torch.int32).contiguous()
        G = int(num_groups) if num_groups is not None else (int(group.max()) + 1 if S else 1)      # (inferred: one host read)
        G = max(G, 1)
    w_slots = modules.as_path_weights(path_weights, S, W)
    w_member = None
    if w_slots is not None:
        w_slots = w_slots.to(dev)
        w_member = w_slots.reshape(W, S).t().contiguous() if hetero else w_slots       # PathNet: slot q = j * S + s
    if target is not None:
        target = torch.as_tensor(target).reshape(-1).to(device=dev, dtype=torch.int64)
        if target.numel() != S:
            raise ValueError("explain: %d targets for %d masked nodes" % (target.numel(), S))
    if totals is not None and (not isinstance(totals, Totals) or totals.num_groups != G or totals.state.device != group.device):
        raise ValueError("explain: totals= takes an Explanation.totals of the same %d groups and device" % G)
    step = max(1, min(int(batch_nodes), max(S, 1))) if batch_nodes is not None else max(S, 1)
    norm, parts = modules._PATH_NORM[path_weight_norm], []
    was_training = model.training
    model.eval()
    # The forwards run on the plain inference path (PN_EVAL_ZW off).  The library's shortcut that applies W_ih to the bank rows
    # before the gather is taken only when its table fits the slice's workspace slot, so with it a group_slice of 4 rows can
    # round differently from the same rows of the whole batch (1e-7); without it every slice leaves the whole batch's bits,
    # and batch_nodes changes nothing but the memory.  The knob is the context's: it is put back before explain returns.
    zw_was = _lib.set_knob("PN_EVAL_ZW", 0, dev)
    try:
        with torch.no_grad():
            fresh = True
            for b0 in range(0, S, step):
                cnt = min(step, S - b0)
                rows = slice(b0, b0 + cnt)
                # a group_slice of the one batch description: the rows' bits are those of the unchunked call (the library's
                # promise for every class), and PathNet's rows read paths of the batch's other nodes anyway
                enc = model.encode(X, ids, W, L, sel, codes, path_state=True, group_slice=(b0, cnt) if cnt < S else None,
                                   reuse_tables=not fresh, path_weights=w_slots, path_weight_norm=path_weight_norm)
                fresh = False
                out, totals = explain_groups(enc.path_state, enc.path_weight, enc.embedding, model.fc2.weight, model.fc2.bias,
                                            group[rows], G, weight=None if w_member is None else w_member[rows], norm=norm,
                                            renorm=hetero, target=None if target is None else target[rows], logits=logits,
                                            contribution=contribution, totals=totals)
                out["logits"] = enc.logits
                parts.append(out)
    finally:
        _lib.set_knob("PN_EVAL_ZW", zw_was, dev)
        model.train(was_training)
    if totals is None:
        totals = Totals(G, dev)

    def whole(k):
        vals = [p[k] for p in parts]
        if not vals:
            shape = dict(logits=(0, int(model.out_size)), drop_delta=(0, G), keep_gain=(0, G), flip=(0, G), present=(0, G),
                         target_used=(0,))
            dt = dict(flip=torch.uint8, present=torch.int32, target_used=torch.int64).get(k, torch.float32)
            return torch.empty(shape[k], dtype=dt, device=dev) if k in shape else None
        if vals[0] is None:
            return None
        return vals[0] if len(vals) == 1 else torch.cat(vals)
    return Explanation(whole("logits"), whole("drop_delta"), whole("keep_gain"), whole("flip"), whole("present"),
                       whole("target_used"), whole("drop_logits"), whole("keep_logits"), whole("contribution"),
                       totals)
