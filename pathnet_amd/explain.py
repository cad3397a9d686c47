"""Explanations: which paths, nodes or edges a prediction rests on (pn_explain_groups / pn_explain_overlap /
pn_explain_totals, pn_explain.hip; pn_explain_units / pn_explain_node_totals, pn_explain_units.hip).

The aggregators classify a node from the W paths around it.  ``model.explain(...)`` says what the model would answer without
a group of a node's paths (``drop_delta``, ``flip``) and with that group alone (``keep_gain``), for every group of every
node, from ONE ``encode(path_state=True)`` forward: the recurrence never sees the pooling, and the classifier is linear after
it, so every leave-out and keep-only answer is a closed form over the paths' final hidden states, which one kernel evaluates
in fp64 on the device (include/pathnet_hip.h has the definition).  By construction ``drop_logits[:, g]`` is the model's own
``forward(path_weights=...)`` with the members of group g given weight 0, and ``keep_logits[:, g]`` the forward with every
other member given weight 0 -- at the cost of one forward instead of 2 G + 1.

Paths are redrawn every epoch; the graph stays.  ``groups="node"`` and ``groups="edge"`` make a row's distinct nodes (edges)
its groups: removing node u removes every member that passed through u, so the groups overlap -- the closed form does not
mind (pn_explain_overlap).  ``Explanation.unit`` names the node (edge) behind every column, ``NodeTotals`` counts per node
over the whole graph.

Not covered: the attribution of single steps inside a path -- what a member's state would be had it skipped a node (the
recurrence is not linear; node and edge groups remove whole members); per-node sums of scores and per-edge totals; the
aggregation over several path draws; the node-sharded and replicated aggregators of pathnet_amd.dist; and training mode
(explain runs the model in eval mode under no_grad).
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


class NodeTotals:
    """Per-node running counts over every row the ``groups="node"`` explain calls have added (four int64 views of ONE device
    buffer, ``state`` int64 [4, n_nodes]: the table of pn_explain_node_totals); pass it as ``totals=`` to continue it:
    rows_present [N]    rows in which the node was a unit with a live member (and finite scores)
    members [N]         live members that passed through the node, over those rows
    flips [N]           rows whose argmax changes without the node
    top [N]             rows in which the node had the largest drop_delta of the row's units"""

    def __init__(self, n_nodes, device="cuda", state=None):
        self.n_nodes = N = int(n_nodes)
        if N < 1:
            raise ValueError("NodeTotals: %d nodes, at least 1" % N)
        self.state = torch.zeros((4, N), dtype=torch.int64, device=device) if state is None else state
        if tuple(self.state.shape) != (4, N) or self.state.dtype != torch.int64 or not self.state.is_contiguous():
            raise ValueError("NodeTotals: a contiguous int64 tensor [4, %d] expected" % N)

    rows_present = property(lambda self: self.state[0])
    members = property(lambda self: self.state[1])
    flips = property(lambda self: self.state[2])
    top = property(lambda self: self.state[3])

    def summary(self, k=20):
        """The one host read -> a list of at most k dicts, the nodes with the most flips first (then the lower id): node,
        rows_present, members, flips, top, flip_rate (flips / rows_present); nodes never present are left out"""
        t = self.state.cpu().numpy()
        order = sorted((i for i in range(self.n_nodes) if t[0, i] > 0), key=lambda i: (-int(t[2, i]), i))[:max(int(k), 0)]
        return [dict(node=i, rows_present=int(t[0, i]), members=int(t[1, i]), flips=int(t[2, i]), top=int(t[3, i]),
                     flip_rate=float(t[2, i] / t[0, i])) for i in order]


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
    totals                          the Totals over every row of this call and of the totals= it continued (groups="node": the
                                    NodeTotals; groups="edge": None)
    Two trailing fields, given after ``totals`` (or by name) and None unless groups="node" / "edge"; attributes, not tuple items:
    unit int64 [S, G]               the key behind column g of row s: the node id, or (min << 32) | max of an edge's ends; the
                                    row's distinct keys in ascending order, then -1
    unit_count int32 [S]            how many columns of the row are units"""

    def __new__(cls, *args, unit=None, unit_count=None, **kw):
        n = len(FIELDS)
        extra = args[n:]
        if len(extra) > 2 or (len(extra) > 0 and unit is not None) or (len(extra) > 1 and unit_count is not None):
            raise TypeError("Explanation: %d positional fields at most, unit and unit_count once" % (n + 2))
        self = super().__new__(cls, *args[:n], **kw)
        self.unit = extra[0] if len(extra) > 0 else unit
        self.unit_count = extra[1] if len(extra) > 1 else unit_count
        return self

    def _replace(self, **kw):
        unit, unit_count = kw.pop("unit", self.unit), kw.pop("unit_count", self.unit_count)
        return type(self)(*super()._replace(**kw), unit, unit_count)

    def units(self):
        """unit for nodes; for edges the two ends, int32 [S, G, 2] (-1, -1 where the column is no unit)"""
        if self.unit is None:
            raise ValueError('units(): an explanation by groups="node" or groups="edge" has them')
        if self.totals is not None:         # (an edge explanation has no totals: an edge has no dense index)
            return self.unit
        return edge_ends(self.unit)

    def top_units(self, k):
        """top(k) with the group positions replaced by their keys -> (values [S, k], keys int64 [S, k]; -1 where the row has
        fewer units)"""
        if self.unit is None:
            raise ValueError('top_units(): an explanation by groups="node" or groups="edge" has them')
        vals, idx = self.top(k)
        return vals, torch.gather(self.unit, 1, idx)

    def top(self, k):
        """torch.topk of drop_delta over the groups -> (values [S, k], group ids [S, k]); groups without a live member in the
        row rank last"""
        score = torch.where(self.present > 0, self.drop_delta, torch.full_like(self.drop_delta, float("-inf")))
        return torch.topk(score, min(int(k), score.shape[1]), dim=1)

    def summary(self):
        """The one host read -> a list of G dicts: group, rows_present, members, mean_drop_delta, mean_keep_gain, flip_rate
        (means over the rows in which the group is present).  groups="node": NodeTotals.summary(); groups="edge" has none"""
        t = self.totals
        if isinstance(t, NodeTotals):
            return t.summary()
        if t is None:
            raise ValueError('summary(): groups="edge" keeps no totals (an edge has no dense index)')
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


MAX_UNIT_STEPS, MAX_UNIT_KEYS = 16, 1024        # pn_explain_units / pn_explain_overlap: L, and W * M
UNIT_KINDS = {"node": _lib.UNIT_NODE, "edge": _lib.UNIT_EDGE}


def edge_keys(a, b):
    """the key of the undirected edge {a, b}: (min << 32) | max, int64 (pn_explain_units, PN_UNIT_EDGE)"""
    a, b = torch.as_tensor(a).to(torch.int64), torch.as_tensor(b).to(torch.int64)
    return (torch.minimum(a, b) << 32) | torch.maximum(a, b)


def edge_ends(unit):
    """edge keys int64 [...] -> their two ends int32 [..., 2], lower id first; (-1, -1) for a key of -1"""
    u = torch.as_tensor(unit).to(torch.int64)
    ends = torch.stack([u >> 32, u & 0xFFFFFFFF], dim=-1)
    return torch.where((u >= 0)[..., None], ends, torch.full_like(ends, -1)).to(torch.int32)


def units_per_member(kind, W, L):
    """M of a node / edge explanation, after the limits of pn_explain_units (named in the ValueError)"""
    if kind not in UNIT_KINDS:
        raise ValueError("kind=%r: 'node' or 'edge'" % (kind,))
    W, L = int(W), int(L)
    lo = 2 if kind == "edge" else 1
    if W < 1:
        raise ValueError("explain units: W = %d members, at least 1" % W)
    if L < lo or L > MAX_UNIT_STEPS:
        raise ValueError("explain units: L = %d steps, %d <= L <= %d for groups=%r" % (L, lo, MAX_UNIT_STEPS, kind))
    M = L - 1 if kind == "edge" else L
    if W * M > MAX_UNIT_KEYS:
        raise ValueError("explain units: W * M = %d * %d = %d keys per row, W * M <= %d" % (W, M, W * M, MAX_UNIT_KEYS))
    return M


def member_nodes(variant, ids, S, W, L):
    """The node whose table row member j of row s consumed at step t -> int32 [S, W, L], encode()'s member order.
    PathNet_homo / PAGG ("homo", "pagg"): the path array itself.  PathNet ("hetero"): slot q = j * S + s of the reference's
    scrambled batch reads ids_flat[(q L + t) % P, L - 1 - (q L + t) // P] with P = S * W of the WHOLE batch (pn_plan.hip's
    plan_kernel).  Plain indexing on the tensor's device (CPU tensors too)."""
    S, W, L = int(S), int(W), int(L)
    ids = torch.as_tensor(ids)
    if ids.numel() != S * W * L:
        raise ValueError("member_nodes: %d ids, %d x %d x %d expected" % (ids.numel(), S, W, L))
    ids = ids.reshape(S * W, L)
    if variant in ("homo", "pagg"):
        return ids.reshape(S, W, L).to(torch.int32).contiguous()
    if variant != "hetero":
        raise ValueError("member_nodes: variant %r" % (variant,))
    P = S * W
    dev = ids.device
    s = torch.arange(S, device=dev)[:, None, None]
    j = torch.arange(W, device=dev)[None, :, None]
    t = torch.arange(L, device=dev)[None, None, :]
    r = (j * S + s) * L + t
    if P == 0:
        return torch.empty((S, W, L), dtype=torch.int32, device=dev)
    return ids[r % P, L - 1 - torch.div(r, P, rounding_mode="floor")].to(torch.int32).contiguous()


def explain_units(node, kind, exclude=None):
    """One pn_explain_units call: node int32 [S, W, L] in member order (member_nodes), kind "node" or "edge", exclude int32 [S]
    or None ("node" only) -> (unit int64 [S, W * M], count int32 [S], label int32 [S, W, M]) on node's device"""
    node = torch.as_tensor(node)
    if node.dim() != 3:
        raise ValueError("explain_units: node of shape %s, [S, W, L] expected" % (tuple(node.shape),))
    dev = node.device
    S, W, L = (int(v) for v in node.shape)
    M = units_per_member(kind, W, L)
    if exclude is not None and kind == "edge":
        raise ValueError('explain_units: exclude= goes with kind="node" only')
    if dev.type != "cuda":
        raise RuntimeError("pathnet_amd explanations run on the GPU only (node is on %s); no CPU fallback" % dev)
    node = node.to(torch.int32).contiguous()
    if exclude is not None:
        exclude = torch.as_tensor(exclude).reshape(-1).to(device=dev, dtype=torch.int32).contiguous()
        if exclude.numel() != S:
            raise ValueError("explain_units: %d excluded nodes for %d rows" % (exclude.numel(), S))
    with torch.cuda.device(dev):
        unit = torch.empty((S, W * M), dtype=torch.int64, device=dev)
        count = torch.empty(S, dtype=torch.int32, device=dev)
        label = torch.empty((S, W, M), dtype=torch.int32, device=dev)
        _lib.check(_lib.load().pn_explain_units(_lib.context(dev), S, W, L, UNIT_KINDS[kind], _lib.ptr(node), _lib.ptr(exclude),
                                                _lib.ptr(unit), _lib.ptr(count), _lib.ptr(label), _lib.stream_ptr(dev)))
    return unit, count, label


def explain_overlap(state, coef, ego, fc2_w, fc2_b, label, G, *, unit=None, weight=None, norm=_lib.PATH_NORM_SUM, renorm=False,
                    target=None, logits=False, contribution=False, totals=None):
    """One pn_explain_overlap call on tensors in encode()'s member order: explain_groups' arguments with label int32 [S, W, M]
    (explain_units) in the place of group.  totals: a NodeTotals, added to by one pn_explain_node_totals over `unit` [S, G], or
    None -> (dict of the kernel's outputs, totals)."""
    if label.dim() != 3:
        raise ValueError("explain_overlap: label of shape %s, [S, W, M] expected" % (tuple(label.shape),))
    return _explain_call(state, coef, ego, fc2_w, fc2_b, label, G, int(label.shape[2]), unit, weight, norm, renorm, target,
                         logits, contribution, totals)


def explain_groups(state, coef, ego, fc2_w, fc2_b, group, G, *, weight=None, norm=_lib.PATH_NORM_SUM, renorm=False, target=None,
                   logits=False, contribution=False, totals=None):
    """One pn_explain_groups call (and its pn_explain_totals) on tensors in encode()'s member order:
    state [S, W, H], coef [S, W], ego [S, >= H] (a view of the embedding will do), fc2_w [C, 2H], fc2_b [C], group int32 [S, W],
    weight [S, W] or None, totals a Totals or None -> (dict of the kernel's outputs, Totals)."""
    return _explain_call(state, coef, ego, fc2_w, fc2_b, group, G, 0, None, weight, norm, renorm, target, logits, contribution,
                         totals)


def _explain_call(state, coef, ego, fc2_w, fc2_b, group, G, M, unit, weight, norm, renorm, target, logits, contribution, totals):
    """M == 0: pn_explain_groups on group [S, W] and pn_explain_totals (a Totals is made when none is given).  M >= 1:
    pn_explain_overlap on labels [S, W, M], and pn_explain_node_totals when totals is a NodeTotals."""
    dev = state.device
    S, W, H = (int(v) for v in state.shape)
    C, G = int(fc2_w.shape[0]), int(G)
    if M:
        if M > MAX_UNIT_STEPS or W * M > MAX_UNIT_KEYS:
            raise ValueError("explain_overlap: M = %d labels per member and W * M = %d, M <= %d and W * M <= %d"
                             % (M, W * M, MAX_UNIT_STEPS, MAX_UNIT_KEYS))
        if totals is not None and (not isinstance(totals, NodeTotals) or unit is None or tuple(unit.shape) != (S, G)
                                   or totals.state.device != dev):
            raise ValueError("explain_overlap: totals= takes a NodeTotals on the same device, with unit= int64 [%d, %d]" % (S, G))
    if dev.type != "cuda":
        raise RuntimeError("pathnet_amd explanations run on the GPU only (state is on %s); no CPU fallback" % dev)
    state = state.contiguous()
    if ego.stride(-1) != 1:
        ego = ego.contiguous()
    ld_state, ld_ego = H, max(int(ego.stride(0)), H)
    fc2_w, fc2_b = fc2_w.detach().float().contiguous(), fc2_b.detach().float().contiguous()
    coef, group = coef.float().contiguous(), group.to(device=dev, dtype=torch.int32).contiguous()
    if tuple(group.shape) != ((S, W, M) if M else (S, W)):
        raise ValueError("explain: groups of shape %s, %s expected" % (tuple(group.shape), [S, W, M] if M else [S, W]))
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
        if totals is None and not M:
            totals = Totals(G, dev)
        desc = _lib.ExplainOut(*(_lib.ptr(out[k]) for k in _lib.ExplainOut.FIELDS))
        lib, ctx, stream = _lib.load(), _lib.context(dev), _lib.stream_ptr(dev)
        head = (ctx, S, W, H, C, G) + ((M,) if M else ())
        _lib.check((lib.pn_explain_overlap if M else lib.pn_explain_groups)(
            *head, _lib.ptr(state), ld_state, _lib.ptr(coef), _lib.ptr(ego), ld_ego, _lib.ptr(fc2_w), 2 * H, _lib.ptr(fc2_b),
            _lib.ptr(weight), _lib.ptr(group), int(norm), int(bool(renorm)), _lib.ptr(target), ctypes.byref(desc), None, stream))
        scores = (_lib.ptr(out["drop_delta"]), _lib.ptr(out["keep_gain"]), _lib.ptr(out["flip"]), _lib.ptr(out["present"]))
        if not M:
            _lib.check(lib.pn_explain_totals(ctx, S, G, *scores, None, 0, _lib.ptr(totals.state), stream))
        elif totals is not None:
            unit = unit.contiguous()
            _lib.check(lib.pn_explain_node_totals(ctx, S, G, totals.n_nodes, _lib.ptr(unit), *scores, None, 0,
                                                  _lib.ptr(totals.state), stream))
    return out, totals


def explain(model, X, neis, num_w, walk_len, indices, layer_type, *, groups="path", num_groups=None, target=None,
            path_weights=None, path_weight_norm="sum", batch_nodes=None, logits=False, contribution=False, totals=None,
            exclude_self=True):
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
    kind, M, node = None, 0, None
    if isinstance(groups, str) and groups in UNIT_KINDS:
        kind = groups
        if kind == "edge" and hetero:
            raise ValueError('groups="edge": PathNet_homo / PAGG only -- a PathNet member is a slot of the scrambled batch '
                             "whose steps come from other nodes' paths: consecutive consumed nodes are not edges there; "
                             'groups="node" names the nodes a slot consumed')
        M = units_per_member(kind, W, L)
        G = W * M
        if num_groups is not None and int(num_groups) != G:
            raise ValueError("groups=%r has W * M = %d columns, num_groups=%d" % (groups, G, int(num_groups)))
        node = member_nodes(model.variant, ids, S, W, L)       # [S, W, L] in member order, of the whole batch
        group = None
    elif isinstance(groups, str):
        if groups == "path":
            group, G = torch.arange(W, dtype=torch.int32, device=dev).repeat(S, 1), W
        elif groups == "reach":
            if hetero:
                raise ValueError('groups="reach": PathNet_homo / PAGG only -- a PathNet member is a slot of the scrambled batch '
                                 "whose steps come from other nodes' paths; pass an explicit [S, W] tensor in member order")
            group, G = reach_groups(codes, S, W, L, dev), L
        else:
            raise ValueError("groups=%r: 'path', 'reach', 'node', 'edge' or an int tensor [S, W]" % (groups,))
        if num_groups is not None and int(num_groups) != G:
            raise ValueError("groups=%r has %d groups, num_groups=%d" % (groups, G, int(num_groups)))
    else:
        group = torch.as_tensor(groups)
        if group.dtype.is_floating_point or group.dtype == torch.bool or tuple(group.shape) != (S, W):
            raise ValueError("groups: 'path', 'reach', 'node', 'edge' or an int tensor [%d, %d] in member order" % (S, W))
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
    if kind == "node":
        if totals is not None and (not isinstance(totals, NodeTotals) or totals.n_nodes != int(X.shape[0])
                                   or totals.state.device != dev):
            raise ValueError('explain: groups="node" takes a NodeTotals of the same %d nodes and device as totals=' % X.shape[0])
        if totals is None:
            totals = NodeTotals(int(X.shape[0]), dev)
    elif kind == "edge":
        if totals is not None:
            raise ValueError('explain: groups="edge" keeps no totals (an edge has no dense index); totals= must be None')
    elif totals is not None and (not isinstance(totals, Totals) or totals.num_groups != G or totals.state.device != dev):
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
                kw = dict(weight=None if w_member is None else w_member[rows], norm=norm, renorm=hetero,
                          target=None if target is None else target[rows], logits=logits, contribution=contribution,
                          totals=totals)
                if kind is None:
                    out, totals = explain_groups(enc.path_state, enc.path_weight, enc.embedding, model.fc2.weight,
                                                 model.fc2.bias, group[rows], G, **kw)
                else:
                    unit, count, label = explain_units(node[rows], kind, sel[rows] if kind == "node" and exclude_self else None)
                    out, totals = explain_overlap(enc.path_state, enc.path_weight, enc.embedding, model.fc2.weight,
                                                  model.fc2.bias, label, G, unit=unit, **kw)
                    out["unit"], out["unit_count"] = unit, count
                out["logits"] = enc.logits
                parts.append(out)
    finally:
        _lib.set_knob("PN_EVAL_ZW", zw_was, dev)
        model.train(was_training)
    if totals is None and kind is None:
        totals = Totals(G, dev)

    def whole(k):
        vals = [p[k] for p in parts]
        if not vals:
            shape = dict(logits=(0, int(model.out_size)), drop_delta=(0, G), keep_gain=(0, G), flip=(0, G), present=(0, G),
                         target_used=(0,), unit=(0, G), unit_count=(0,))
            dt = dict(flip=torch.uint8, present=torch.int32, target_used=torch.int64, unit=torch.int64,
                      unit_count=torch.int32).get(k, torch.float32)
            return torch.empty(shape[k], dtype=dt, device=dev) if k in shape else None
        if vals[0] is None:
            return None
        return vals[0] if len(vals) == 1 else torch.cat(vals)
    return Explanation(whole("logits"), whole("drop_delta"), whole("keep_gain"), whole("flip"), whole("present"),
                       whole("target_used"), whole("drop_logits"), whole("keep_logits"), whole("contribution"),
                       totals, whole("unit") if kind else None, whole("unit_count") if kind else None)
