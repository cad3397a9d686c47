"""Drop-in aggregator modules with the reference's constructor / forward surface and state_dict keys.

  PathNet       <- /root/reference/PathNet_run.py:150-211   (heterophilous datasets)
  PathNet_homo  <- /root/reference/PathNet_run.py:214-278   (cora / citeseer / pubmed)
  PAGG          <- /root/reference/baseline/GPRGNN/src/copy.py:299-359

``forward(X, neis, num_w, walk_len, indices, layer_type, indxx)`` keeps the reference's argument
meaning (PathNet_run.py:172): X fp32 [N, F] on the GPU, neis [S, W*L] node ids, indices a bool mask
[N] (numpy or torch), layer_type [S, W, L] distance codes, indxx ignored (it is arange(S*W*L)).
All arithmetic runs in hand-written HIP kernels through libpathnet_hip.so; there is no PyTorch
fallback -- if the library is missing, construction fails.
"""
import collections
import ctypes
import os
import weakref

import numpy as np
import torch
import torch.nn as nn

from . import _lib

# The reference reads the module-level global `dropout` inside forward (PathNet_run.py:71, :194).
# A training script can set pathnet_amd.modules.dropout the same way, or pass dropout= to the ctor.
dropout = 0.7

_VARIANT = {"hetero": _lib.VARIANT_HETERO, "homo": _lib.VARIANT_HOMO, "pagg": _lib.VARIANT_PAGG}
# path encoders: the classes' own (lstm / rnn) and the ablation rows of the paper's table (gru / mean / sum, README.md:118)
_CELL = {None: _lib.CELL_DEFAULT, "lstm": _lib.CELL_LSTM, "rnn": _lib.CELL_RNN, "gru": _lib.CELL_GRU,
         "mean": _lib.CELL_MEAN, "sum": _lib.CELL_SUM}
_HEAD_PARAMS = ("fc0_w", "fc0_b", "w_ih", "w_hh", "b_ih", "b_hh", "att_w", "att_b", "fc2_w", "fc2_b")


# Per-path tensors of one aggregator call (saved gates, [x|h] rows, gate gradients: ~6 KB per path step) are kept
# below this many bytes: a batch with more paths is walked in micro-batches inside the library (pn_pagg_shape
# .batch_groups), the backward re-running each micro-batch's recurrence.  Cora / Pubmed-size batches fit in one.
WORKSPACE_BUDGET_BYTES = 48 << 30
MIN_BATCH_BYTES = 8 << 30           # floor of the per-micro-batch part (pick_batch_groups)


def default_budget(device=None):
    """Workspace budget when the module has none of its own: WORKSPACE_BUDGET_BYTES, but never more than 60 % of the
    HBM that is free on `device` right now (a smaller GPU, or one shared with other tensors, then gets micro-batches
    instead of an out-of-memory error)."""
    try:
        free, _ = torch.cuda.mem_get_info(device)
        return int(min(WORKSPACE_BUDGET_BYTES, max(0.6 * free, MIN_BATCH_BYTES)))
    except Exception:       # noqa: BLE001  (no CUDA context yet / CPU-only import)
        return WORKSPACE_BUDGET_BYTES


_SEQ_MATH = {None: _lib.SEQ_MATH_DEFAULT, "": _lib.SEQ_MATH_DEFAULT, "f16x2": _lib.SEQ_MATH_F16X2, "bf16x3": _lib.SEQ_MATH_BF16X3}


_PATH_NORM = {"sum": _lib.PATH_NORM_SUM, "count": _lib.PATH_NORM_COUNT}


def as_path_weights(path_weights, rows, W, check=False, path_grad=False):
    """path_weights= of the aggregators -> a float32 tensor [rows, W] (still on its own device), or None.  Any float (or
    integer) dtype, shape [rows, W] or [rows * W]; rows: the rows of the call's neis.  A wrong shape, or without path_grad a
    tensor that requires grad, raises ValueError -- by default the weights are data, no gradient is returned for them.  With
    path_grad=True (the aggregators' keyword) the result is a differentiable function of the caller's tensor.  check: also
    raise on a negative or non-finite entry (one host read); unchecked, the kernels count such an entry as 0."""
    if path_weights is None:
        return None
    w = torch.as_tensor(path_weights)
    if w.requires_grad and not path_grad:
        raise ValueError("path_weights requires grad: by default the weights are data and no gradient is returned for them "
                         "(detach them, or pass path_grad=True)")
    if w.dtype == torch.bool or w.dtype.is_complex:
        raise TypeError("path_weights: a real dtype expected, got %s" % w.dtype)
    if tuple(w.shape) not in ((rows, W), (rows * W,)):
        raise ValueError("path_weights of shape %s: [%d, %d] (masked nodes of neis x paths) or [%d] expected"
                         % (tuple(w.shape), rows, W, rows * W))
    w = w.reshape(rows, W)
    if check and bool((~torch.isfinite(w) | (w < 0)).any()):
        raise ValueError("path_weights hold negative or non-finite entries")
    return w.to(torch.float32)


def compact_default():
    """pn_pagg_shape.compact when a call does not say: PN_COMPACT=1 / 0 in the environment forces the touched-row
    compaction of the distance bank on / off (tests, A/B runs); otherwise the library decides from the shape.  Read when a
    call is set up -- the value then travels with the call's shape through workspace size, forward and backward."""
    e = os.environ.get("PN_COMPACT")
    if e is None or e == "":
        return _lib.COMPACT_AUTO
    return _lib.COMPACT_ON if int(e) != 0 else _lib.COMPACT_OFF


RANGE_WINDOW_BITS = 18      # spread (bits) of the gathered rows' magnitudes the fp16 x 2 kernels carry at full precision
RANGE_POLL_EVERY = 16       # calls between two asynchronous read-backs of the range record


def seq_math_default():
    """pn_pagg_shape.seq_math when a module does not say: PN_SEQ_MATH=bf16x3 selects rounds 1-3's six-MFMA bf16 products
    for the recurrent GEMMs, the default (f16x2) is three fp16 MFMAs over scaled two-plane splits (include/pathnet_hip.h)."""
    e = os.environ.get("PN_SEQ_MATH", "").strip().lower()
    if e not in _SEQ_MATH:
        raise ValueError("PN_SEQ_MATH=%r: f16x2 or bf16x3" % e)
    return _SEQ_MATH[e]


class PaggCall:
    """One aggregator call as the library is to see it, described once: the fields of pn_pagg_shape by name (SHAPE_FIELDS: the
    struct's order and defaults; variant and cell by their Python names) and what the call carries besides.  Everything
    that fills a pn_pagg_shape / pn_pagg_args -- the modules here, dist.HipOps -- goes through shape() / args().  What is
    decided after construction (batch_groups, workspace, reuse_tables) is assigned to attributes that exist from the start;
    a name that is not listed below raises."""
    SHAPE_FIELDS = ("variant", "N", "F", "H", "C", "S", "W", "L", "S_total", "group_begin", "batch_groups", "cell",
                    "deterministic", "compact", "seq_math")
    __slots__ = SHAPE_FIELDS + ("p_seq", "p_cls", "seed", "mask_seq", "mask_cls", "step_state", "index_rows_local", "bank_w",
                                "bank_b", "grad", "reuse_tables", "grad_scale", "path_state", "sparse_plan", "workspace",
                                "features", "loss", "path_weights", "path_weight_norm", "_shape", "_ws_bytes")

    def __init__(self, variant, N, F, H, C, S, W, L, S_total=0, group_begin=0, batch_groups=0, cell=None, deterministic=False,
                 compact=None, seq_math=None, *, p_seq=0.0, p_cls=0.0, seed=0, mask_seq=None, mask_cls=None, step_state=None,
                 index_rows_local=False, bank_w=None, bank_b=None, grad=True, reuse_tables=0, grad_scale=1.0,
                 path_state=False, sparse_plan=None, workspace=None, features=None, loss=None, path_weights=None,
                 path_weight_norm="sum"):
        self.variant, self.N, self.F, self.H, self.C, self.S, self.W, self.L = variant, N, F, H, C, S, W, L
        self.S_total, self.group_begin, self.batch_groups, self.cell = S_total, group_begin, batch_groups, cell
        # decisions that shape the workspace are taken once per call and travel with its shape
        self.deterministic = bool(deterministic)
        self.compact = compact_default() if compact is None else int(compact)
        self.seq_math = seq_math_default() if seq_math is None else int(seq_math)
        self.p_seq, self.p_cls, self.seed, self.mask_seq, self.mask_cls = p_seq, p_cls, seed, mask_seq, mask_cls
        self.step_state, self.index_rows_local, self.bank_w, self.bank_b = step_state, index_rows_local, bank_w, bank_b
        # grad False: a torch.no_grad() forward, which skips the saved tensors.  reuse_tables 1: Xh and the dense bank in the
        # workspace are valid, 2: Xh only
        self.grad, self.reuse_tables, self.grad_scale, self.path_state = grad, reuse_tables, grad_scale, path_state
        self.sparse_plan, self.workspace = sparse_plan, workspace
        self.features = features        # PreparedFeatures of the call's X (fc0 over its non-zeros), or None: the dense kernels
        # (optim.CrossEntropyLoss with options, grad_scale of the reduced loss) of forward_loss(loss=...), or None: the plain loss
        self.loss = loss
        # per-path weights of the pooling: a contiguous fp32 device tensor [rows of ids, W] (as_path_weights) or None, and
        # "sum" / "count".  The call keeps the tensor alive until its backward has read it.
        self.path_weights, self.path_weight_norm = path_weights, path_weight_norm
        self._shape = self._ws_bytes = None

    def get(self, name, default=None):
        """call.get("S_total") / call["W"]: read access by name for ShardedAggregator(ops=...) backends written against the
        earlier dict description.  Every name exists, so no default applies: an unknown one raises here too."""
        return getattr(self, name)
    __getitem__ = get

    def shape(self):
        """the call's _lib.PaggShape, built at the first use"""
        if self._shape is None:
            self._shape = _lib.PaggShape(_VARIANT[self.variant], self.N, self.F, self.H, self.C, self.S, self.W, self.L,
                                         self.S_total, self.group_begin, self.batch_groups, _CELL[self.cell],
                                         1 if self.deterministic else 0, self.compact, self.seq_math)
        return self._shape

    def set_batch_groups(self, bg):
        """the one shape field that is decided after the others: what was derived from the shape is derived again"""
        self.batch_groups = bg
        self._shape = self._ws_bytes = None
        return self

    def pick_batch_groups(self, budget, device=None):
        # (the module's function, looked up at the call: tools/ab_chunks.py replaces it)
        return self.set_batch_groups(pick_batch_groups(
            self.variant, self.N, self.F, self.H, self.C, self.S, self.W, self.L, budget, cell=self.cell, device=device,
            deterministic=self.deterministic, S_total=self.S_total, group_begin=self.group_begin, compact=self.compact,
            seq_math=self.seq_math))

    def workspace_bytes(self):
        if self._ws_bytes is None:
            n = ctypes.c_int64(0)
            _lib.check(_lib.load().pn_pagg_workspace_bytes(ctypes.byref(self.shape()), ctypes.byref(n)))
            self._ws_bytes = n.value
        return self._ws_bytes

    def take_workspace(self, dev, have=None):
        """`have` when it sits on `dev` and is large enough for this call, else a new tensor"""
        need = self.workspace_bytes()
        if have is not None and have.numel() >= need and have.device == dev:
            return have
        return torch.empty(max(need, 1), dtype=torch.uint8, device=dev)

    def features_ref(self):
        """the call's pn_sparse_features for the pn_pagg_*_sparse entry points (None = NULL: the plain calls)"""
        return ctypes.byref(self.features.c) if self.features is not None else None

    def args(self, ids, codes, sel, p, X=None, Xh=None):
        """A _lib.PaggArgs with the call's inputs: shape, index arrays, parameters (p: _split_params), dropout, flags.
        X: the feature matrix, which the library projects itself (the modules here).  Xh: the caller has projected already --
        the node-sharded runner applies fc0 to its own rows before the exchange -- so the library gets the projected table
        and no fc0; that runner has no captured steps either, its calls carry no step_state.
        Outputs, workspace and gradient pointers are the caller's to add (grad_buffers)."""
        a = _lib.PaggArgs()
        a.shape = self.shape()
        if Xh is None:
            a.X, names = X.data_ptr(), _HEAD_PARAMS
        else:
            a.Xh_in, names = Xh.data_ptr(), _HEAD_PARAMS[2:]
        a.ids, a.codes, a.sel = ids.data_ptr(), codes.data_ptr(), sel.data_ptr()
        for k in names:
            if p[k] is not None:
                setattr(a, k, p[k].data_ptr())
        a.bank_w, a.bank_b = self.bank_w.data_ptr(), self.bank_b.data_ptr()
        a.p_seq, a.p_cls, a.seed = self.p_seq, self.p_cls, self.seed
        a.mask_seq = self.mask_seq.data_ptr() if self.mask_seq is not None else None
        a.mask_cls = self.mask_cls.data_ptr() if self.mask_cls is not None else None
        a.step_state = self.step_state.ptr() if self.step_state is not None else None
        a.index_rows_local = 1 if self.index_rows_local else 0
        return a

    def weights_ref(self):
        """the call's pn_path_weights for the pn_pagg_*_weighted entry points (None = NULL: the unweighted pooling)"""
        if self.path_weights is None:
            return None
        return ctypes.byref(_lib.PathWeights(self.path_weights.data_ptr(), _PATH_NORM[self.path_weight_norm]))

    def weight_grad_buffer(self):
        """the tensor for pn_path_grads.g_weight, laid out like the call's path_weights.  The library stores the entries of the
        call's own groups and touches no other: a call that computes a part of the batch its weights describe (group_slice),
        or nothing, starts from zeros."""
        whole = self.S > 0 and (self.index_rows_local or self.S_total in (0, self.S))
        return (torch.empty_like if whole else torch.zeros_like)(self.path_weights)

    def grad_buffers(self, a, p, X=None, flat=False):
        """Gradient tensors for every parameter `a` names (and for X, when given), their addresses set in a.g_*.
        -> ({head parameter name / "bank_w" / "bank_b": tensor}, g_X or None, flat buffer or None).  flat: the parameter
        gradients are views of ONE buffer, in 16-byte aligned pieces, that a single launch can scale."""
        keys = [k for k in _HEAD_PARAMS if getattr(a, k)]
        like = [p[k] for k in keys] + [self.bank_w, self.bank_b]
        buf = None
        if flat:
            sizes = [-(-t.numel() // 4) * 4 for t in like]
            buf = torch.empty(sum(sizes), dtype=torch.float32, device=self.bank_w.device)
            pieces = [v[:t.numel()].view(t.shape) for v, t in zip(buf.split(sizes), like)]
        else:
            pieces = [torch.empty_like(t) for t in like]
        grads = dict(zip(keys + ["bank_w", "bank_b"], pieces))
        for k, g in grads.items():
            setattr(a, "g_" + k, g.data_ptr())
        gX = torch.empty_like(X) if X is not None else None
        a.g_X = gX.data_ptr() if gX is not None else None
        return grads, gX, buf


SPARSE_MAX_ELEMS = 1 << 28      # pn_sparse_count's limit: positions of the non-zeros stay in int32
SPARSE_CACHE_ENTRIES = 4        # prepared feature matrices a module keeps (train / validation / test splits share one X)
SPARSE_DENSE_KEYS = 16          # keys remembered as dense (no tensor is kept for them)
SPARSE_SEEN_KEYS = 8            # keys seen once and not looked at yet (after SPARSE_MISS_LIMIT misses)
SPARSE_MISS_LIMIT = 2           # scanned matrices in a row that never came back before first sights stop being scanned


class PreparedFeatures:
    """The non-zeros of a feature matrix X [N, F] (fp32, contiguous, on the GPU) as the library's pn_sparse_features: CSR
    (row_off, col, val: features ascending in a row) and CSC (col_off, row, valc: nodes ascending in a column), built by
    pn_sparse_count / pn_sparse_fill.  count() costs one launch chain and ONE host read (nnz); fill() allocates exactly.
    The object keeps X alive: while it exists no other tensor can take X's address."""
    __slots__ = ("X", "nnz", "row_off", "col_off", "col", "val", "row", "valc", "c", "pinned")

    def __init__(self, X):
        N, F = X.shape
        dev = X.device
        self.X = X
        with torch.cuda.device(dev):
            self.row_off = torch.empty(N + 1, dtype=torch.int32, device=dev)
            self.col_off = torch.empty(F + 1, dtype=torch.int32, device=dev)
            _lib.check(_lib.load().pn_sparse_count(_lib.context(dev), X.data_ptr(), N, F, self.row_off.data_ptr(),
                                                   self.col_off.data_ptr(), _lib.stream_ptr(dev)))
            self.nnz = int(self.row_off[N].item())
        self.col = self.val = self.row = self.valc = self.c = None
        self.pinned = False         # handed to a call while its stream was being captured

    def density(self):
        return self.nnz / float(self.X.shape[0] * self.X.shape[1])

    def fill(self):
        N, F = self.X.shape
        dev = self.X.device
        with torch.cuda.device(dev):
            # (zeros: an entry the fill does not reach -- X written to between count and fill -- is feature / node 0 with value 0)
            self.col, self.row = (torch.zeros(self.nnz, dtype=torch.int32, device=dev) for _ in range(2))
            self.val, self.valc = (torch.zeros(self.nnz, dtype=torch.float32, device=dev) for _ in range(2))
            self.c = _lib.SparseFeatures(self.nnz, self.row_off.data_ptr(), self.col.data_ptr(), self.val.data_ptr(),
                                         self.col_off.data_ptr(), self.row.data_ptr(), self.valc.data_ptr())
            _lib.check(_lib.load().pn_sparse_fill(_lib.context(dev), self.X.data_ptr(), N, F, ctypes.byref(self.c),
                                                  _lib.stream_ptr(dev)))
        return self


def _shape(variant, N, F, H, C, S, W, L, S_total=0, group_begin=0, batch_groups=0, cell=None, deterministic=False,
           compact=None, seq_math=None):
    return PaggCall(variant, N, F, H, C, S, W, L, S_total, group_begin, batch_groups, cell, deterministic, compact, seq_math).shape()


def shape_info(sh):
    """(compact, rows of Z, micro-batches, seq_math) the library derives from a pn_pagg_shape"""
    out = (ctypes.c_int64 * 4)()
    _lib.check(_lib.load().pn_pagg_shape_info(ctypes.byref(sh), out))
    return bool(out[0]), int(out[1]), int(out[2]), int(out[3])


def deterministic_default():
    """The backward's mode when a module does not say: torch.use_deterministic_algorithms(True) or PN_DETERMINISTIC=1
    select the fixed-order backward (pn_pagg_shape.deterministic: bitwise reproducible gradients, no fp32 atomics)."""
    return torch.are_deterministic_algorithms_enabled() or os.environ.get("PN_DETERMINISTIC", "0") not in ("", "0")


def workspace_bytes(variant, N, F, H, C, S, W, L, S_total=0, group_begin=0, batch_groups=0, cell=None, deterministic=False,
                    compact=None, seq_math=None):
    return PaggCall(variant, N, F, H, C, S, W, L, S_total, group_begin, batch_groups, cell, deterministic, compact, seq_math).workspace_bytes()


def pick_batch_groups(variant, N, F, H, C, S, W, L, budget=None, cell=None, device=None, deterministic=False,
                      S_total=0, group_begin=0, compact=None, seq_math=None):
    """0 when the whole batch fits the workspace budget, else the largest micro-batch (in masked nodes) that does.
    budget=None: default_budget(device) -- queried only when the batch needs more than MIN_BATCH_BYTES, so that ordinary
    steps make no runtime call.
    The workspace of a call that runs b masked nodes at a time is fixed(S) + b * per_group: the node tables -- whose rows
    depend on the WHOLE call's S (and S_total for a slice of a hetero batch) when the bank runs over compact rows -- plus
    the per-path tensors of one micro-batch.  Both terms are measured on this call's own shape (batch_groups = 1 and
    1 + step), and the pick is checked against the budget afterwards."""
    call = PaggCall(variant, N, F, H, C, S, W, L, S_total, group_begin, 0, cell, deterministic, compact, seq_math)

    def ws(bg):
        return call.set_batch_groups(bg).workspace_bytes()
    need = ws(0) if S > 1 else 0
    floor = MIN_BATCH_BYTES if budget is None else 0       # an explicit budget is kept to the byte
    if budget is None:
        if need <= MIN_BATCH_BYTES:
            return 0
        budget = default_budget(device)
    budget = int(budget)
    if S <= 1 or need <= budget:
        return 0
    step = min(1024, S - 1)
    w1 = ws(1)
    per_group = max((ws(1 + step) - w1) // step, 1) if step > 0 else max(need, 1)
    fixed = w1 - per_group                  # the node tables (and the compact-row arrays): needed whatever the micro-batch
    avail = max(budget - fixed, floor)      # default budget: graphs whose tables alone exceed it still get real batches
    bg = int(max(1, min(S, avail // per_group if avail > 0 else 1)))
    if floor == 0:                          # an explicit budget is kept to the byte: settle on the real layout (alignment,
        while bg > 1 and ws(bg) > budget:   # terms that are not linear in the micro-batch such as the sort's scratch)
            bg = max(1, min(bg - 1, int(bg * 0.98)))
        for _ in range(16):
            if bg >= S or ws(bg + 1) > budget:
                break
            bg += 1
    return bg


def _split_params(params, L):
    """Function inputs -> dict of the tensors the C ABI wants.  `params` is
    (the ten _HEAD_PARAMS, bank_w_0..L-1, bank_b_0..L-1);
    the bank entries are views of one contiguous [L,H,H] / [L,H] buffer (see _Aggregator._bank)."""
    p = dict(zip(_HEAD_PARAMS, params[:10]))
    p["bank_ws"], p["bank_bs"] = params[10:10 + L], params[10 + L:10 + 2 * L]
    return p


def _grad_tuple(grads, L):
    """PaggCall.grad_buffers' dict -> the gradients in the order of the Function inputs `params` (None: no such parameter)"""
    return tuple(grads.get(k) for k in _HEAD_PARAMS) + tuple(grads["bank_w"][d] for d in range(L)) + tuple(
        grads["bank_b"][d] for d in range(L))


def _begin(call, ids, codes, sel, p, X=None, Xh=None):
    """what every forward starts with (X / Xh: PaggCall.args): -> (args with inputs, logits and workspace set; logits; workspace)"""
    dev = ids.device
    out = torch.empty((call.S, call.C), dtype=torch.float32, device=dev)
    ws = call.take_workspace(dev, call.workspace)
    a = call.args(ids, codes, sel, p, X=X, Xh=Xh)
    a.out = out.data_ptr()
    a.workspace, a.workspace_bytes = ws.data_ptr(), ws.numel()
    return a, out, ws


class _PaggFunction(torch.autograd.Function):
    """forward/backward through pn_pagg_forward / pn_pagg_backward."""

    @staticmethod
    def _forward(ctx, call, X, ids, codes, sel, params, encode_out=None):
        """encode_out (_PaggEncodeFunction): (embedding, path weights, path states or None) for the library to fill"""
        p = _split_params(params, call.L)
        dev = X.device
        with torch.cuda.device(dev):        # the library launches on the current device
            a, out, ws = _begin(call, ids, codes, sel, p, X=X)
            a.no_save = 0 if call.grad else 1
            a.reuse_tables = int(call.reuse_tables or 0)
            if encode_out is not None:
                a.out_embed, a.out_path_weight = encode_out[0].data_ptr(), encode_out[1].data_ptr()
                a.out_path_state = encode_out[2].data_ptr() if encode_out[2] is not None else None
            if call.S > 0:
                _lib.check(_lib.load().pn_pagg_forward_weighted(_lib.context(dev), ctypes.byref(a), call.features_ref(),
                                                                call.weights_ref(), _lib.stream_ptr(dev)))
        ctx.call, ctx.ws = call, ws
        ctx.present = [t is not None for t in params]
        ctx.save_for_backward(X, ids, codes, sel, *[t for t in params if t is not None])
        return out

    @staticmethod
    def forward(ctx, call, X, ids, codes, sel, *params):
        return _PaggFunction._forward(ctx, call, X, ids, codes, sel, params)

    @staticmethod
    def backward(ctx, g_out):
        return _PaggFunction._backward(ctx, g_out, None)

    @staticmethod
    def _backward(ctx, g_out, g_embed, g_pw=None, g_ps=None, g_weight=None, want_gX=None):
        """one pn_pagg_backward for d loss / d logits (g_out) and / or d loss / d embedding (g_embed); either may be None.
        _PaggPathFunction: also the upstream gradients of encode()'s path_weight / path_state (g_pw / g_ps) and the tensor
        d loss / d path weights goes to (g_weight: PaggCall.weight_grad_buffer) -- then one pn_pagg_backward_paths"""
        call = ctx.call
        saved = list(ctx.saved_tensors)
        X, ids, codes, sel = saved[:4]
        it = iter(saved[4:])
        params = [next(it) if pres else None for pres in ctx.present]
        p = _split_params(params, call.L)
        dev = X.device
        with torch.cuda.device(dev):
            g_out = g_out.contiguous().float() if g_out is not None else None
            g_embed = g_embed.contiguous().float() if g_embed is not None else None
            a = call.args(ids, codes, sel, p, X=X)
            grads, gX, _ = call.grad_buffers(a, p, X if (ctx.needs_input_grad[1] if want_gX is None else want_gX) else None)
            a.workspace, a.workspace_bytes = ctx.ws.data_ptr(), ctx.ws.numel()
            a.g_out = g_out.data_ptr() if g_out is not None else None
            a.g_embed = g_embed.data_ptr() if g_embed is not None else None
            if call.S > 0 and (g_pw is not None or g_ps is not None or g_weight is not None):
                g_pw = g_pw.contiguous().float() if g_pw is not None else None
                g_ps = g_ps.contiguous().float() if g_ps is not None else None
                pg = _lib.PathGrads(g_ps.data_ptr() if g_ps is not None else None, g_pw.data_ptr() if g_pw is not None else None,
                                    g_weight.data_ptr() if g_weight is not None else None)
                _lib.check(_lib.load().pn_pagg_backward_paths(_lib.context(dev), ctypes.byref(a), call.features_ref(),
                                                              call.weights_ref(), ctypes.byref(pg), _lib.stream_ptr(dev)))
            elif call.S > 0:
                _lib.check(_lib.load().pn_pagg_backward_weighted(_lib.context(dev), ctypes.byref(a), call.features_ref(),
                                                                 call.weights_ref(), _lib.stream_ptr(dev)))
            else:
                for g in list(grads.values()) + [gX] * (gX is not None):
                    g.zero_()
        return (None, gX, None, None, None) + _grad_tuple(grads, call.L)


class _PaggEncodeFunction(torch.autograd.Function):
    """logits, embedding [S, 2H], path weights [S, W] (and final hidden states [S, W, H]) of ONE pn_pagg_forward; the
    library's optional outputs (pn_pagg_args.out_*).  Logits and embedding are differentiable: one pn_pagg_backward takes
    the upstream gradients of both (g_out / g_embed, an unused output's being NULL)."""

    @staticmethod
    def forward(ctx, call, X, ids, codes, sel, *params):
        S, W, H, dev = call.S, call.W, call.H, X.device
        with torch.cuda.device(dev):
            emb = torch.empty((S, 2 * H), dtype=torch.float32, device=dev)
            pw = torch.empty((S, W), dtype=torch.float32, device=dev)
            ps = torch.empty((S, W, H), dtype=torch.float32, device=dev) if call.path_state else None
        # (the outputs travel as an argument: ctx keeps `call`, and it must not hold the outputs)
        out = _PaggFunction._forward(ctx, call, X, ids, codes, sel, params, encode_out=(emb, pw, ps))
        ctx.mark_non_differentiable(*[t for t in (pw, ps) if t is not None])
        # (an output the loss does not use gets no zero-filled gradient: pn_pagg_backward is given NULL for it)
        ctx.set_materialize_grads(False)
        return (out, emb, pw) if ps is None else (out, emb, pw, ps)

    @staticmethod
    def backward(ctx, g_out, g_embed, *_unused):
        if g_out is None and g_embed is None:
            return (None,) * (5 + len(ctx.present))
        return _PaggFunction._backward(ctx, g_out, g_embed)


class _PaggPathFunction(torch.autograd.Function):
    """path_grad=True: _PaggFunction (encode False: logits) or _PaggEncodeFunction (encode True) with the gradients at the
    per-path interface.  `weights` -- the tensor call.path_weights was detached from, or None -- is a differentiable input,
    and encode()'s path_weight / path_state are differentiable outputs; one pn_pagg_backward_paths takes whichever upstream
    gradients the loss produced and returns d loss / d weights with the parameters' gradients."""

    @staticmethod
    def forward(ctx, call, encode, weights, X, ids, codes, sel, *params):
        S, W, H, dev = call.S, call.W, call.H, X.device
        enc = None
        if encode:
            with torch.cuda.device(dev):
                enc = (torch.empty((S, 2 * H), dtype=torch.float32, device=dev), torch.empty((S, W), dtype=torch.float32, device=dev),
                       torch.empty((S, W, H), dtype=torch.float32, device=dev) if call.path_state else None)
        out = _PaggFunction._forward(ctx, call, X, ids, codes, sel, params, encode_out=enc)
        ctx.want_weight = weights is not None
        ctx.set_materialize_grads(False)
        if not encode:
            return out
        return (out,) + tuple(t for t in enc if t is not None)

    @staticmethod
    def backward(ctx, g_out=None, g_embed=None, g_pw=None, g_ps=None):
        n_in = 7 + len(ctx.present)
        if g_out is None and g_embed is None and g_pw is None and g_ps is None:
            return (None,) * n_in
        call = ctx.call
        gw = call.weight_grad_buffer() if (ctx.want_weight and ctx.needs_input_grad[2]) else None
        # (_backward sees X's flag where _PaggFunction has it: the inputs here are shifted by two)
        res = _PaggFunction._backward(ctx, g_out, g_embed, g_pw, g_ps, gw, want_gX=ctx.needs_input_grad[3])
        if gw is not None and call.S == 0:
            gw.zero_()
        return (None, None, gw) + res[1:]


class _PaggLossFunction(torch.autograd.Function):
    """loss, logits = one pn_pagg_train_step: forward, softmax cross entropy and backward in one library call (what it
    saves: the second forward of every micro-batch, include/pathnet_hip.h).  The gradients are computed here and handed
    out by backward(), scaled by the upstream gradient of the loss."""

    @staticmethod
    def forward(ctx, call, X, ids, codes, sel, target, *params):
        return _PaggLossFunction._forward(ctx, call, X, ids, codes, sel, target, params, ctx.needs_input_grad[1], False)

    @staticmethod
    def _forward(ctx, call, X, ids, codes, sel, target, params, want_gX, want_gw):
        """want_gw (_PaggPathLossFunction): the same library call also leaves d loss / d path weights in ctx.g_weight"""
        p = _split_params(params, call.L)
        dev = X.device
        with torch.cuda.device(dev):
            a, out, _ = _begin(call, ids, codes, sel, p, X=X)
            # (pn_pagg_train_step stores the loss -- or clears it itself before accumulating over micro-batches: no fill here)
            loss = (torch.empty if call.S > 0 else torch.zeros)((), dtype=torch.float32, device=dev)
            # every parameter gradient is a view of one flat buffer: backward() scales them by the upstream gradient of
            # the loss with one launch instead of one per tensor
            grads, gX, flat = call.grad_buffers(a, p, X if want_gX else None, flat=True)
            target = target.to(device=dev, dtype=torch.int64).contiguous()
            ctx.g_weight = call.weight_grad_buffer() if want_gw else None
            if call.S > 0 and want_gw:
                spec = None
                if call.loss is not None:
                    loss_fn, scale = call.loss
                    spec, ctx.loss_keep = loss_fn.spec(dev, call.C, scale)
                pg = _lib.PathGrads(None, None, ctx.g_weight.data_ptr())
                _lib.check(_lib.load().pn_pagg_train_step_paths(
                    _lib.context(dev), ctypes.byref(a), call.features_ref(), ctypes.byref(spec) if spec is not None else None,
                    call.weights_ref(), ctypes.byref(pg), target.data_ptr(), float(call.grad_scale), loss.data_ptr(),
                    _lib.stream_ptr(dev)))
            elif call.S > 0 and call.loss is not None:
                # (the spec's weight and denominator tensors live on the context until backward(); under capture they are the
                #  graph's pool's, like every other tensor of the step)
                loss_fn, scale = call.loss
                spec, ctx.loss_keep = loss_fn.spec(dev, call.C, scale)
                _lib.check(_lib.load().pn_pagg_train_step_loss_weighted(
                    _lib.context(dev), ctypes.byref(a), call.features_ref(), ctypes.byref(spec), call.weights_ref(),
                    target.data_ptr(), loss.data_ptr(), _lib.stream_ptr(dev)))
            elif call.S > 0:
                _lib.check(_lib.load().pn_pagg_train_step_weighted(
                    _lib.context(dev), ctypes.byref(a), call.features_ref(), call.weights_ref(), target.data_ptr(),
                    float(call.grad_scale), loss.data_ptr(), _lib.stream_ptr(dev)))
            else:
                flat.zero_()
                if gX is not None:
                    gX.zero_()
        ctx.grads = (gX,) + _grad_tuple(grads, call.L)
        ctx.flat = flat
        ctx.mark_non_differentiable(out)
        # (without this autograd materialises a zero gradient for `out` -- an [S, C] fill launch in front of the optimizer,
        #  on the step's critical path: profiles/r06_glue.txt)
        ctx.set_materialize_grads(False)
        return loss, out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_loss, _g_out):
        return _PaggLossFunction._backward(ctx, g_loss)

    @staticmethod
    def _backward(ctx, g_loss, g_weight=None):
        """g_weight (_PaggPathLossFunction): d loss / d path weights of the same step, scaled with the others"""
        # (the context lets go of the tensors: with a second owner alive autograd's AccumulateGrad would copy every
        #  gradient into a fresh tensor instead of adopting it -- 18 copy launches per step)
        grads, flat = ctx.grads, ctx.flat
        ctx.grads = ctx.flat = None
        if grads is None:
            raise RuntimeError("forward_loss: the gradients were handed out already (backward twice)")
        # (d loss' / d loss: 1 for loss.backward().  The gradients were computed once, in forward(): a single backward, no
        #  double backward -- once_differentiable says so to autograd; a second backward raises above)
        from . import optim
        if g_loss is None:      # (set_materialize_grads(False): the loss took no part in what is being differentiated)
            return (None,) * (6 + len(grads) - 1)
        one = optim._UNIT.get(g_loss.device)
        if one is None or g_loss.data_ptr() != one.data_ptr():       # (optim.backward(loss) seeds with the cached 1.0: nothing to scale)
            flat.mul_(g_loss)
            if grads[0] is not None:
                grads[0].mul_(g_loss)
            if g_weight is not None:
                g_weight.mul_(g_loss)
        return (None, grads[0], None, None, None, None) + tuple(grads[1:])


class _PaggPathLossFunction(torch.autograd.Function):
    """_PaggLossFunction with path_grad=True: `weights` (the tensor call.path_weights was detached from) is a differentiable
    input, its gradient comes out of the same pn_pagg_train_step_paths call as every other gradient of the step."""

    @staticmethod
    def forward(ctx, call, weights, X, ids, codes, sel, target, *params):
        return _PaggLossFunction._forward(ctx, call, X, ids, codes, sel, target, params, ctx.needs_input_grad[2], True)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_loss, _g_out):
        gw, ctx.g_weight = ctx.g_weight, None
        res = _PaggLossFunction._backward(ctx, g_loss, gw)
        return (None, gw if g_loss is not None else None) + res[1:]


def _as_index_tensors(neis, layer_type, indices, num_w, walk_len, device, n_nodes=None):
    """Reference argument conventions -> device int32 ids [S,W,L], uint8 codes, int32 sel [S].
    `indices`: a bool mask over the nodes (numpy or torch: the reference's two conventions) or the node ids
    themselves (any integer dtype, numpy or torch)."""
    if isinstance(indices, np.ndarray):
        if indices.dtype == np.bool_:
            sel = torch.from_numpy(np.flatnonzero(indices).astype(np.int32))
        elif np.issubdtype(indices.dtype, np.integer):
            sel = torch.from_numpy(np.ascontiguousarray(indices).reshape(-1).astype(np.int32))
        else:
            raise TypeError("indices: bool mask or integer node ids expected, got numpy %s" % indices.dtype)
    else:
        idx = torch.as_tensor(indices)
        if idx.dtype == torch.bool:
            sel = torch.nonzero(idx, as_tuple=False).flatten().to(torch.int32)
        elif not idx.dtype.is_floating_point and not idx.dtype.is_complex:
            sel = idx.flatten().to(torch.int32)
        else:
            raise TypeError("indices: bool mask or integer node ids expected, got %s" % idx.dtype)
    S = int(sel.numel())
    ids = torch.as_tensor(neis)
    codes = torch.as_tensor(layer_type)
    if ids.numel() != S * num_w * walk_len or codes.numel() != S * num_w * walk_len:
        raise ValueError("neis / layer_type hold %d / %d entries, %d masked nodes x %d paths x %d steps = %d expected"
                         % (ids.numel(), codes.numel(), S, num_w, walk_len, S * num_w * walk_len))
    if n_nodes is not None and S and sel.device.type == "cpu":      # (device-resident indices are not read back: the
                                                                    #  kernels clamp ids, codes and sel to the tables)
        lo, hi = int(sel.min()), int(sel.max())
        if lo < 0 or hi >= n_nodes:
            raise IndexError("indices name node %d, the feature matrix has %d rows" % (lo if lo < 0 else hi, n_nodes))
    if ids.dtype != torch.int32:
        ids = ids.to(torch.int32)
    if codes.dtype != torch.uint8:
        codes = codes.to(torch.uint8)
    ids = ids.reshape(S, num_w, walk_len).to(device, non_blocking=True).contiguous()
    codes = codes.reshape(S, num_w, walk_len).to(device, non_blocking=True).contiguous()
    return ids, codes, sel.to(device, non_blocking=True).contiguous(), S


Encoded = collections.namedtuple("Encoded", ("logits", "embedding", "path_weight", "path_state"))


def _explicit_masks(ms, mc, H, Hk, seq_math, check_range=True):
    """Explicit dropout masks (test hook; given for the module's own hidden size H) as the kernels at hidden size Hk read
    them.  The caller zeroes the call's dropout probabilities.  check_range: the library's kernels will read them."""
    if ms is None and mc is None:
        return None, None
    if Hk != H:
        P = torch.nn.functional.pad
        ms = P(ms, (0, Hk - H)).contiguous() if ms is not None else None
        mc = P(mc.view(mc.shape[0], 2, H), (0, Hk - H)).reshape(mc.shape[0], 2 * Hk).contiguous() if mc is not None else None
    if ms is not None and check_range and seq_math != _lib.SEQ_MATH_BF16X3 and float(ms.abs().max()) > 16.0:
        # (one device round trip) the fp16 kernels scale the gathered rows for masks up to 16 = 1 / (1 - 0.9375)
        raise ValueError("explicit sequence masks must satisfy |m| <= 16 with seq_math f16x2 (include/pathnet_hip.h); "
                         "use seq_math='bf16x3' for others")
    return ms, mc


class _Aggregator(nn.Module):
    variant = None

    def _common_init(self, feature_length, hidden_size, out_size, dropout_p, cell=None):
        _lib.load()     # fail at construction if the HIP library is missing
        if cell not in _CELL:
            raise ValueError("cell must be one of %s" % sorted(k for k in _CELL if k))
        # None: the class's own path encoder (its state_dict is the reference's); "gru" / "mean" / "sum" / "lstm" / "rnn":
        # the ablation rows of the paper's table ("Changing the PAGG class can deliver other variants", README.md:118)
        self.cell = cell
        self.feature_length, self.hidden_size, self.out_size = feature_length, hidden_size, out_size
        self._dropout = dropout_p
        self._ws_eval = None
        self._ws_tables = None            # (X address, shape, L) whose tables sit in _ws_eval
        self.step_state = None            # pathnet_amd.StepState: dropout seed read from device memory (hipGraph replay)
        self.workspace_budget = None      # bytes; None = modules.WORKSPACE_BUDGET_BYTES (see pick_batch_groups)
        self.deterministic = None         # True / False: fixed-order backward or not; None: deterministic_default()
        self.seq_math = None              # "f16x2" / "bf16x3": arithmetic of the recurrent GEMMs; None: seq_math_default()
        # Range guard of the default arithmetic (seq_math None -> f16x2).  Its two fp16 planes keep 22 bits of a gathered row
        # within ~2^18 of the largest one; a single spike row 2^20 times the typical row -- bag-of-words features after fc0
        # can do that -- costs the typical rows bits (include/pathnet_hip.h: pn_seq_range).  The forward's kernels leave the
        # maximum and the spread of the rows' magnitudes in device memory; the module reads them back -- synchronously after
        # its FIRST call (which is run again in bf16x3 when the spread is beyond the window), asynchronously every
        # RANGE_POLL_EVERY-th call afterwards -- and switches itself to bf16x3 for good once it has seen such an input.
        self.range_guard = True
        self._range_wide = False          # sticky: an input beyond the window was seen
        self._range_calls = 0
        self._range_pending = None        # (pinned int32[6], event) of a read-back in flight
        self.range_spread_bits = None     # last evaluated spread: exponent(max |Z|) - mean exponent of the sampled tiles
        # fc0 over the non-zeros of X (pn_sparse.hip), for the resident dataset matrix.  A matrix is looked at ONCE, when its
        # key (address, shape, in-place version, device) is first seen and it has at least sparse_min_nodes rows and at most 2^28
        # elements: a count launch and one host read.  It is prepared when its density is at most sparse_max_density, else
        # remembered as dense and not scanned again.  A caller whose X is a new tensor, or a new version, in every call would pay
        # that scan per call: when SPARSE_MISS_LIMIT scanned matrices in a row have not come back, scanning at first sight stops
        # (two scans at the most), and a matrix is then looked at only when the same tensor object comes back unchanged.
        # "never": always the dense kernels; "always": prepared at first sight, no size / density gate (small tests).
        # While the stream is being captured an unprepared X is not prepared: that call runs dense.  Calls that compute a part
        # of a batch (group_slice, batch_position: the runners of pathnet_amd.dist) always run dense.  Same convention as
        # _tables_key: a write to X that bypasses its version counter (X.data, a raw kernel) is not seen.
        # At most SPARSE_CACHE_ENTRIES prepared matrices are kept, each with its X; the oldest makes room for a new one, except
        # that an entry a captured graph was given stays for as long as the module lives (with four of those, a fifth matrix
        # runs dense).
        self.sparse_features = "auto"
        self.sparse_min_nodes = 2048      # the floor of the row-reduction kernel the dense weight gradient uses (rgrad_pays)
        self.sparse_max_density = 1.0 / 64  # (profiles/sparse_fc0.txt: Cora's 1.3 % is inside, Pubmed's 10 % TF-IDF rows are not)
        self._sparse_cache = collections.OrderedDict()     # key -> PreparedFeatures
        self._sparse_dense = collections.OrderedDict()     # keys looked at and found too dense
        self._sparse_seen = collections.OrderedDict()      # key -> weak reference to the tensor seen once under it
        self.sparse_scans = 0             # matrices counted so far (each is a launch chain and a host read)
        self._sparse_misses = 0           # scanned matrices in a row that did not come back
        self._sparse_scan_open = False    # the matrix scanned last has not been seen again yet
        self.fc0_route = None             # "sparse" / "dense": what the last call handed to the library
        self.fc0_route_calls = {"sparse": 0, "dense": 0}
        self._mask_seq = None     # test hook: explicit dropout masks (reference order)
        self._mask_cls = None
        self._bank_flat = (None, None)

    # ---- dropout probability: ctor argument, else the module-level global like the reference -------
    def dropout_p(self):
        return float(dropout if self._dropout is None else self._dropout)

    def set_dropout(self, p):
        self._dropout = p

    def _bank_layers(self):
        raise NotImplementedError

    def _tables_key(self, X, L):
        """what the projected feature matrix and the distance bank in the eval workspace were computed from: X (address,
        shape, in-place version) and the versions of the fc0 / bank parameters (an optimizer step bumps them)"""
        lins = [self.fc0] + list(self._bank_layers())
        return (X.data_ptr(), tuple(X.shape), int(X._version), int(L),
                tuple(int(t._version) for l in lins for t in (l.weight, l.bias)))

    def _features_for(self, X, Hk):
        """PreparedFeatures for this call's X, or None for the dense route (see _common_init)"""
        mode = self.sparse_features
        if mode not in ("auto", "never", "always"):
            raise ValueError("sparse_features: auto, never or always")
        N, F = X.shape
        if mode == "never" or Hk > 256 or N * F == 0 or N * F > SPARSE_MAX_ELEMS:
            return None
        key = (X.data_ptr(), (N, F), int(X._version), X.device)
        cache, capturing = self._sparse_cache, torch.cuda.is_current_stream_capturing()
        feat = cache.get(key)
        if feat is not None:
            cache.move_to_end(key)
            feat.pinned = feat.pinned or capturing      # a captured graph holds its pointers: never evicted from here on
            self._sparse_misses, self._sparse_scan_open = 0, False
            return feat
        if mode == "auto" and key in self._sparse_dense:
            self._sparse_misses, self._sparse_scan_open = 0, False
            return None
        if capturing or (mode == "auto" and N < self.sparse_min_nodes):
            return None             # (a capture remembers nothing: the next eager call looks at X)
        if mode == "auto" and self._sparse_scan_open:   # the matrix scanned last never came back: a miss
            self._sparse_misses += 1
            self._sparse_scan_open = False
        if mode == "auto" and self._sparse_misses >= SPARSE_MISS_LIMIT:
            # X is not a resident matrix here -- a fresh tensor per step (feature dropout, a gathered sub-matrix) or one that
            # changes in place every step: the scans stop.  From now on the first sight of a key costs nothing, it is only noted,
            # with a weak reference to the tensor, and a matrix is scanned when the same tensor object comes back unchanged
            seen = self._sparse_seen.pop(key, None)
            if seen is None or seen() is not X:
                self._sparse_seen[key] = weakref.ref(X)
                while len(self._sparse_seen) > SPARSE_SEEN_KEYS:
                    self._sparse_seen.popitem(last=False)
                return None
        if len(cache) >= SPARSE_CACHE_ENTRIES:          # room: the oldest entry no captured graph has been given, if there is one
            old = next((k for k, f in cache.items() if not f.pinned), None)
            if old is None:
                return self._remember_dense(key)
        feat = PreparedFeatures(X)
        self.sparse_scans += 1
        self._sparse_scan_open = mode == "auto"
        if mode == "auto" and feat.density() > self.sparse_max_density:
            return self._remember_dense(key)
        if len(cache) >= SPARSE_CACHE_ENTRIES:
            del cache[old]
        cache[key] = feat.fill()
        return feat

    def _remember_dense(self, key):
        """a verdict costs no slot of the prepared matrices: keys only, the oldest forgotten first"""
        self._sparse_dense[key] = True
        while len(self._sparse_dense) > SPARSE_DENSE_KEYS:
            self._sparse_dense.popitem(last=False)
        return None

    def _make_cell(self, default):
        """the recurrent sub-module, under the attribute name torch users expect (LSTM / RNN / GRU); none for mean / sum"""
        kind = self.cell or default
        H = self.hidden_size
        if kind == "lstm":
            self.LSTM = nn.LSTM(H, H)
        elif kind == "rnn":
            self.RNN = nn.RNN(H, H)
        elif kind == "gru":
            self.GRU = nn.GRU(H, H)
        self._cell_kind = kind

    def _cell(self):
        return {"lstm": getattr(self, "LSTM", None), "rnn": getattr(self, "RNN", None),
                "gru": getattr(self, "GRU", None)}.get(self._cell_kind)

    def _bank(self):
        """The L distance layers as ONE contiguous [L,H,H] / [L,H] pair (what the kernels read), without a
        per-step torch.stack: the layers' weight/bias Parameters are re-pointed to be views of two flat
        buffers.  Anything that re-creates the parameters (.to(), .cuda()) is detected by address and the
        buffers are rebuilt.  state_dict keys and Parameter identities are unchanged."""
        lins = self._bank_layers()
        H = self.hidden_size
        fw, fb = self._bank_flat
        ok = (fw is not None and fw.device == lins[0].weight.device and
              all(l.weight.data_ptr() == fw.data_ptr() + d * H * H * 4 and l.bias.data_ptr() == fb.data_ptr() + d * H * 4
                  for d, l in enumerate(lins)))
        if not ok:
            with torch.no_grad():
                fw = torch.stack([l.weight.detach() for l in lins]).contiguous()
                fb = torch.stack([l.bias.detach() for l in lins]).contiguous()
                for d, l in enumerate(lins):
                    l.weight.data = fw[d]
                    l.bias.data = fb[d]
            self._bank_flat = (fw, fb)
        return fw, fb, [l.weight for l in lins], [l.bias for l in lins]

    def _padded_param_inputs(self, Hk):
        """The same inputs for a hidden size that is not a multiple of 32 (`-hid` is any integer, PathNet_run.py:52), zero-padded
        to Hk units as differentiable functions of the parameters.  Exact: a padded unit's projected feature, bank row,
        gates' inputs and attention / classifier weights are 0, so its cell and hidden state stay 0 (sigmoid(0) * tanh(0))
        and it feeds nothing into the real units; autograd drops the padded gradient entries on the way back."""
        H, G = self.hidden_size, {"lstm": 4, "rnn": 1, "gru": 3}.get(self._cell_kind, 0)
        pad = Hk - H
        P = torch.nn.functional.pad

        def rows(w):            # [H, *] -> [Hk, *]
            return P(w, (0, 0) * (w.dim() - 1) + (0, pad))

        def gates(w):           # [G*H, H] -> [G*Hk, Hk]  /  [G*H] -> [G*Hk]
            if w.dim() == 2:
                return P(w.view(G, H, H), (0, pad, 0, pad)).reshape(G * Hk, Hk)
            return P(w.view(G, H), (0, pad)).reshape(G * Hk)

        def halves(w):          # [C, 2H] -> [C, 2Hk]  ([ego | pooled paths])
            return P(w.view(w.shape[0], 2, H), (0, pad)).reshape(w.shape[0], 2 * Hk)
        lins = self._bank_layers()
        ws = [P(l.weight, (0, pad, 0, pad)) for l in lins]
        bs = [P(l.bias, (0, pad)) for l in lins]
        cell = self._cell()
        att = getattr(self, "attw", None)
        rec = tuple(gates(t) for t in (cell.weight_ih_l0, cell.weight_hh_l0, cell.bias_ih_l0, cell.bias_hh_l0)) \
            if cell is not None else (None,) * 4
        head = (rows(self.fc0.weight), P(self.fc0.bias, (0, pad))) + rec + (
            halves(att.weight) if att is not None else None, att.bias if att is not None else None,
            halves(self.fc2.weight), self.fc2.bias)
        with torch.no_grad():
            fw, fb = torch.stack([w.detach() for w in ws]).contiguous(), torch.stack([b.detach() for b in bs]).contiguous()
        return fw, fb, head + tuple(ws) + tuple(bs)

    def _param_inputs(self):
        fw, fb, ws, bs = self._bank()
        cell = self._cell()
        att = getattr(self, "attw", None)
        rec = (cell.weight_ih_l0, cell.weight_hh_l0, cell.bias_ih_l0, cell.bias_hh_l0) if cell is not None else (None,) * 4
        head = (self.fc0.weight, self.fc0.bias) + rec + (
                att.weight if att is not None else None, att.bias if att is not None else None,
                self.fc2.weight, self.fc2.bias)
        return fw, fb, head + tuple(ws) + tuple(bs)

    def forward_loss(self, X, neis, num_w, walk_len, indices, layer_type, target, indxx=None, grad_scale=None, fused=None,
                     loss=None, *, path_weights=None, path_weight_norm="sum", check_weights=False, path_grad=False):
        """(loss, logits) of a training step's forward + torch.nn.CrossEntropyLoss() (PathNet_run.py:343-346); loss.backward()
        yields the parameter gradients.  target: class index of every masked node, in the order of the logits' rows.
        grad_scale: weight of a row's loss (default 1 / rows = the mean).
        fused=True: forward, loss and backward in ONE library call (pn_pagg_train_step; backward() hands out the gradients that
        call already computed) -- for a batch that runs in micro-batches this saves every micro-batch's second forward (the
        10 M-node configuration: 0.250 -> 0.222 s per step).  fused=False: the three calls, which is what a batch that fits
        the workspace is quicker with (measured 1.26 vs 1.29 ms per step at the headline shape).  None: fused exactly when
        the batch needs micro-batches.  Same values either way.
        loss: a pathnet_amd.CrossEntropyLoss with class weights, ignore_index, label smoothing or reduction="sum" (None, or one
        with every option at its default: the plain mean, today's call and bits).  Every route above takes it -- fused or
        not, micro-batches, sparse features, the deterministic mode -- and the weighted mean's denominator is formed on the
        device over the whole batch, so a captured step follows targets whose ignored count changes.  With a loss, grad_scale
        (default 1 / rows) times rows multiplies the reduced loss: the default is torch's value.
        path_weights / path_weight_norm / check_weights: forward()'s.  A weighted fused step runs the pooling as three kernel
        bodies in one launch; the register-resident pooling step is the unweighted call's.
        path_grad=True: path_weights may require grad (forward()'s keyword); the fused step computes their gradient inside its
        one library call, and backward() scales it by the loss's upstream gradient with the others."""
        return self._run(X, neis, num_w, walk_len, indices, layer_type, target=target, grad_scale=grad_scale, fused=fused,
                         loss=loss, path_weights=path_weights, path_weight_norm=path_weight_norm, check_weights=check_weights,
                         path_grad=path_grad)

    def forward(self, X, neis, num_w, walk_len, indices, layer_type, indxx=None, reuse_tables=False, group_slice=None, *,
                path_weights=None, path_weight_norm="sum", check_weights=False, path_grad=False):
        """path_weights (extension; None: the reference's pooling, bit for bit): a weight per path, float [S, W] or [S * W] on
        any device, S the masked nodes of neis (the whole batch also with group_slice).  PathNet_homo / PAGG: entry [s, w]
        weighs path w of masked node s.  PathNet: entry [s, w] weighs sequence slot q = s * W + w of the reference's scrambled
        LSTM batch, which the pooling reads as member q // S of node q % S (encode()'s member order) -- not path w of node s.
        An entry that is no finite positive number counts as 0: the path is left out of the row.  path_weight_norm="sum"
        scales a row's weights to sum to W, so integer weights are repeated paths and pathnet_amd.importance_weights are a
        self-normalised estimate; "count" applies them as given.  A row without a live path pools zeros and passes no
        gradient to its paths.  By default the weights are data: no gradient is returned for them, a tensor that requires grad
        is refused.  check_weights=True raises on a negative or non-finite entry (one host read).
        path_grad=True (extension; with grad enabled): path_weights may require grad and gets its gradient in its own shape,
        dtype and device -- 0 at every entry that counts as 0, in a row without a live path and, with group_slice, in the rows
        outside the slice (pn_pagg_backward_paths; the closed form: INTEGRATION.md section 1).  Under torch.no_grad() the
        keyword changes nothing.  Not covered: the aggregators of pathnet_amd.dist, predict() / explain() / the trainer's
        fixed-index steps (their weights stay data), and a step that is being captured into a hipGraph, which raises."""
        return self._run(X, neis, num_w, walk_len, indices, layer_type, reuse_tables=reuse_tables, group_slice=group_slice,
                         path_weights=path_weights, path_weight_norm=path_weight_norm, check_weights=check_weights,
                         path_grad=path_grad)

    def encode(self, X, neis, num_w, walk_len, indices, layer_type, indxx=None, *, path_state=False, group_slice=None,
               reuse_tables=False, seed=None, path_weights=None, path_weight_norm="sum", check_weights=False, path_grad=False):
        """The model's internals next to its logits, from the same single forward: ``Encoded(logits, embedding, path_weight,
        path_state)``, every tensor fp32 on X's device, one row per masked node (of the group_slice, when given).

          logits      [S, C]     bit-identical to forward() on the same inputs, weights and dropout seed.
          embedding   [S, 2H]    cat(Xh[sel[s]], pooled[s]): the classifier input BEFORE the classifier's dropout
                                 (layer1 = torch.cat((ego, h_n), dim=1), PathNet_run.py:207 / :275, copy.py:355); in training
                                 it holds the sequence dropout of the same call.  Differentiable w.r.t. every parameter and X.
          path_weight [S, W]     the coefficient that multiplies member j's final hidden state in row s's mean: the softmax
                                 weight (PathNet), 1 + att (PathNet_homo), 1 (PAGG); with path_weights (forward()'s) the
                                 coefficient actually applied, kappa * weight * that.  Differentiable with path_grad=True.
          path_state  [S, W, H]  member j's final hidden state h_n; only with path_state=True (it is large), else None.
                                 Differentiable with path_grad=True.

        Member order is the reference's: for PathNet_homo / PAGG member j of row s is path j of masked node s.  For PathNet
        it is sequence slot q = j * S + s of the reference's scrambled LSTM batch (S: masked nodes of the whole batch; the
        [W, S] re-view of PathNet_run.py:196-197): its steps come from other masked nodes' paths, and that is what the
        reference pools for node s (oracle/pagg_oracle.py, plan()).

        A loss over any mix of logits and embedding runs ONE backward of the library.  group_slice, reuse_tables and the
        dropout handling are forward()'s; seed (training only) fixes the dropout seed instead of drawing it from torch's
        generator.  path_grad=True (with grad enabled): path_weight and path_state are differentiable too, and path_weights
        may require grad (forward()'s keyword) -- a loss over any mix of the four outputs still runs ONE backward of the
        library (pn_pagg_backward_paths), an output the loss does not use costs nothing.  Not covered: the node-sharded and
        replicated aggregators of pathnet_amd.dist, and the fused training step (forward_loss(fused=True))."""
        res = self._run(X, neis, num_w, walk_len, indices, layer_type, reuse_tables=reuse_tables, group_slice=group_slice,
                        seed=seed, _encode=bool(path_state), path_weights=path_weights, path_weight_norm=path_weight_norm,
                        check_weights=check_weights, path_grad=path_grad)
        logits, emb, pw = res[:3]
        ps = res[3] if path_state else None
        H = self.hidden_size
        Hk = emb.shape[1] // 2
        if Hk != H:         # the kernels ran at a hidden size padded to a multiple of 32: the padded units are zeros
            S = emb.shape[0]
            emb = emb.view(S, 2, Hk)[:, :, :H].reshape(S, 2 * H)      # (its backward zero-pads the gradient going in)
            ps = ps[:, :, :H].contiguous() if ps is not None else None
        return Encoded(logits, emb, pw, ps)

    def predict(self, X, paths, num_w, walk_len, nodes=None, *, samples=8, seed=0, first_epoch=0, batch_nodes=None,
                samples_per_call=None, labels=None, path_weights=None, path_weight_norm="sum", ensemble=None,
                reuse_tables=False, temperature=None):
        """Ensemble prediction: ``samples`` independent path draws per node, their class probabilities averaged on the
        device (pathnet_amd.Ensemble: fp64 softmax and sums, no read-back) -> ``pathnet_amd.Prediction`` of device tensors
        (prob, label, vote_label, confidence, entropy, mutual_info, agreement, count, bad, confusion, skipped), one row per
        node of `nodes` in their order.

        paths: a sampler (anything with ``.sample``, ``smp.biased(p, q)`` included) -- sample k draws epoch_begin =
        first_epoch + k with ``nodes=`` and `seed` -- or pre-sampled ``(ids, codes)`` tensors ``[E, N, W, L]``, where sample k
        is epoch ``(first_epoch + k) % E``.  nodes: a bool mask or node ids (forward()'s rules); default all N nodes.
        labels (int, per node of X or per node of `nodes`): also the confusion matrix [true, predicted] and the skipped counts.
        path_weights: a callable ``(ids, codes, nodes32, k) -> [S, W]`` or None, as the trainer's.
        ensemble: an Ensemble of len(nodes) rows to continue -- more samples later (a new first_epoch), or several checkpoints
        averaged; the returned Prediction describes everything it holds.
        reuse_tables (extension, forward()'s): X and the weights are those of this module's previous no-grad forward, so
        the first forward of this call reuses the tables too (a test predict right after the validation predict).
        temperature: a float or a 1-element fp64 device tensor (``model.calibrate(...).tau``) the new Ensemble divides the
        logits by, on the device; None: the plain softmax, as before.  With ensemble= the ensemble's own temperature holds.

        The forwards run under no_grad in eval mode (no dropout, torch's generator untouched); the module's training flag is
        restored afterwards.  PathNet_homo / PAGG, where a row depends on its own paths only: the nodes are taken in chunks of
        batch_nodes (default: all of them; a batch beyond the workspace budget runs in the library's own micro-batches), and
        up to samples_per_call samples of a chunk share ONE forward, the chunk's node list tiled R times (default: as many
        as keep a call at about 32 K rows).  Every forward after the first reuses the projected features and the distance bank
        (reuse_tables): fc0 and the bank run once per predict.  Stacked and single calls may take different GEMM routes, so
        their probabilities agree to rounding, not to the bit.
        PathNet (the hetero class): a row reads paths of other masked nodes of its batch, so its
        prediction is a property of (node, batch), as in the reference.  Every sample is the reference's single whole-batch
        forward over `nodes`; batch_nodes only cuts it into group_slice pieces with the same values, and samples_per_call is
        ignored -- samples are never stacked."""
        from . import ensemble as ens
        return ens.predict_with(self, X, paths, num_w, walk_len, nodes, samples=samples, seed=seed, first_epoch=first_epoch,
                                batch_nodes=batch_nodes, samples_per_call=samples_per_call, labels=labels,
                                path_weights=path_weights, path_weight_norm=path_weight_norm, ensemble=ensemble,
                                reuse_tables=reuse_tables, temperature=temperature)

    def calibrate(self, X, paths, num_w, walk_len, nodes, labels, *, samples=8, seed=0, first_epoch=0, max_bytes=1 << 30,
                  **fit_kw):
        """Fit one temperature on `nodes` (the validation nodes) -> ``pathnet_amd.Temperature`` of device tensors; pass its
        ``tau`` to ``predict(temperature=)``.  Runs the forwards predict() would run with the same samples, seed and
        first_epoch (same draws, same stacking), keeps the samples x nodes x classes fp32 logits on the device and hands them
        to ``pathnet_amd.fit_temperature`` with fit_kw (grid=, rounds=).  labels: per node of X or per node of `nodes`.
        Logits beyond max_bytes raise ValueError: use fewer nodes -- one scalar does not need the whole validation set."""
        from . import calibration
        return calibration.calibrate_with(self, X, paths, num_w, walk_len, nodes, labels, samples=samples, seed=seed,
                                          first_epoch=first_epoch, max_bytes=max_bytes, **fit_kw)

    def pretrain(self, X, paths, num_w, walk_len, nodes=None, **kw):
        """Self-supervised pretraining on unlabelled nodes: the contrastive loss (``pathnet_amd.contrastive_loss``) between
        two path draws of every node of a batch -> ``pathnet_amd.trainer.Pretrained(loss, hits, pairs)`` of device tensors.
        ``pathnet_amd.trainer.pretrain`` carries the keywords (epochs=, batch_nodes=, temperature=, intra=, head=,
        optimizer=, lr=, seed=, first_epoch=) and the documentation."""
        from . import trainer
        return trainer.pretrain(self, X, paths, num_w, walk_len, nodes, **kw)

    def embed(self, X, paths, num_w, walk_len, nodes=None, *, samples=1, seed=0, first_epoch=0, batch_nodes=None, head=None):
        """The embeddings of `nodes` (a bool mask or node ids, default all N) -> fp32 [S, 2H] on X's device, one row per node
        in their order: ``encode(...).embedding`` in eval mode under no_grad (no dropout, torch's generator untouched; the
        training flags are restored), averaged over ``samples`` path draws.

        paths follows predict()'s convention: a sampler (``smp.biased(p, q)`` included; sampled with `seed` and ``nodes=``)
        or pre-sampled ``(ids, codes)`` tensors [E, N, W, L].  Draw j is path draw ``first_epoch + j`` (tensors: epoch
        ``(first_epoch + j) % E``); the draws of a node are added in ascending j, starting from draw 0's embedding, and the
        sum is divided by ``samples`` once, in fp32.  The nodes are taken in chunks of batch_nodes (default: all of them),
        one encode() per chunk and draw -- predict()'s loop with samples_per_call=1, so a chunk's rows have the bits of that
        encode() call.  head (a ``torch.nn.Module``, as pretrain()'s): every draw's embedding passes through it, in eval
        mode, before the average, and the result has the head's width.
        PathNet (the hetero class): a row pools sequences made of OTHER masked nodes' paths of its batch (encode()'s doc
        string), so an embedding belongs to (node, batch): the batch is the whole of `nodes`, and batch_nodes only cuts it
        into group_slice pieces with the same values."""
        from . import ensemble as ens
        dev = X.device
        if dev.type != "cuda":
            raise RuntimeError("pathnet_amd aggregators run on the GPU only (X is on %s); no CPU fallback" % dev)
        K = int(samples)
        if K < 1:
            raise ValueError("embed: samples=%d, at least 1" % K)
        nodes32 = ens._node_list(nodes, int(X.shape[0]), dev)
        S = int(nodes32.numel())
        got = []

        def collect(emb, k0, b0):           # (samples_per_call=1: emb is [1, cnt, 2H], draw k0 of rows b0 ..)
            z = emb[0] if head is None else head(emb[0])
            if not got:
                got.append(torch.empty((S, int(z.shape[1])), dtype=torch.float32, device=dev))
            rows = got[0][b0:b0 + int(z.shape[0])]
            if k0 == 0:
                rows.copy_(z)
            else:
                rows.add_(z.to(rows.dtype))

        head_training = head.training if head is not None else None
        if head is not None:
            head.eval()
        try:
            ens.predict_with(self, X, paths, num_w, walk_len, nodes32, samples=K, seed=seed, first_epoch=first_epoch,
                             batch_nodes=batch_nodes, samples_per_call=1, collect=collect, embedding=True)
            if not got:                     # no node: the width is still the head's
                with torch.no_grad():
                    z = torch.empty((0, 2 * self.hidden_size), dtype=torch.float32, device=dev)
                    got.append(z if head is None else head(z).float())
        finally:
            if head is not None:
                head.train(head_training)
        return got[0] / K if K > 1 else got[0]

    def knn_probe(self, X, paths, num_w, walk_len, bank_nodes, bank_labels, query_nodes, query_labels=None, num_classes=None,
                  *, k=20, temperature=0.07, metric="cosine", samples=1, seed=0, first_epoch=0, batch_nodes=None, head=None):
        """The weighted k-NN classifier over this model's embeddings, the label-free monitor of contrastive pretraining ->
        ``pathnet_amd.KnnVote(prob, label, confusion, skipped)`` of device tensors, one row per query node.

        The bank is ``embed(bank_nodes)``, the queries ``embed(query_nodes)`` (one call when query_nodes IS bank_nodes, the
        same object: the lists are not compared, which would be a host read; samples, seed, first_epoch, batch_nodes and head
        are embed()'s), and the result is
        ``knn_classify(knn(queries, bank, k, metric, bank_valid, exclude), bank_labels, num_classes, temperature,
        labels=query_labels)``.  bank_labels / query_labels: per node of X or per node of the list; N labels are always read
        as per node of X and picked by node id (predict()'s rule), also where the list itself has N entries.  num_classes
        defaults to the model's out_size.  Nothing is read back.  bank_valid is formed on the device from the bank labels inside [0, num_classes): an
        unlabelled bank node (label -1) is nobody's neighbour.  exclude is formed on the device from the node ids, so a
        query node that is also a bank node never votes for itself (a node listed twice in the bank: its last position).
        ``trainer.metrics_from_confusion(vote.confusion)`` gives accuracy and F1 when query_labels is given.  A caller
        alternates ``pretrain(first_epoch=...)`` and ``knn_probe()``.  For PathNet (the hetero class) an embedding belongs to
        (node, batch) -- embed()'s doc string -- so bank and queries are embedded within their own node lists."""
        from . import ensemble as ens
        from . import neighbours as nb
        dev, N = X.device, int(X.shape[0])
        bank32, query32 = ens._node_list(bank_nodes, N, dev), ens._node_list(query_nodes, N, dev)
        C = int(self.out_size if num_classes is None else num_classes)

        def labels_of(labels, nodes32, name):
            labels = torch.as_tensor(labels).reshape(-1).to(dev)
            if labels.numel() == N:
                return labels.index_select(0, nodes32.long())
            if labels.numel() != nodes32.numel():
                raise ValueError("knn_probe: %d %s for %d nodes (of %d)" % (labels.numel(), name, nodes32.numel(), N))
            return labels

        bl = labels_of(bank_labels, bank32, "bank_labels").long()
        ql = labels_of(query_labels, query32, "query_labels").long() if query_labels is not None else None
        kw = dict(samples=samples, seed=seed, first_epoch=first_epoch, batch_nodes=batch_nodes, head=head)
        zb = self.embed(X, paths, num_w, walk_len, bank32, **kw)
        zq = zb if query_nodes is bank_nodes else self.embed(X, paths, num_w, walk_len, query32, **kw)
        found = nb.knn(zq, zb, k, metric=metric, bank_valid=(bl >= 0) & (bl < C), exclude=nb.exclude_of(query32, bank32, N))
        return nb.knn_classify(found, bl, C, temperature=temperature, labels=ql)

    def cluster_probe(self, X, paths, num_w, walk_len, nodes=None, labels=None, clusters=None, *, metric="cosine", iters=50,
                      restarts=4, seed=0, samples=1, first_epoch=0, batch_nodes=None, head=None):
        """k-means of this model's embeddings, the judgement of contrastive pretraining that needs no labels at all ->
        ``(pathnet_amd.Clusters, pathnet_amd.ClusterScores or None)`` of device tensors, one label per node of `nodes`.

        It is ``kmeans(embed(nodes), clusters, metric, iters, restarts, seed)`` and, with labels,
        ``cluster_scores(found.label, labels, clusters, out_size)``: samples, seed, first_epoch, batch_nodes and head are
        embed()'s (seed also seeds k-means++).  clusters defaults to the model's out_size.  labels: per node of X or per
        node of the list; N labels are always read as per node of X and picked by node id (knn_probe()'s rule).  A label
        outside [0, out_size) -- an unlabelled node's -1 -- is counted in ``skipped``, as is a dead row.  Nothing is read
        back; ``scores.summary()`` adds the matched accuracy on the host.  For PathNet (the hetero class) an embedding belongs
        to (node, batch) -- embed()'s doc string."""
        from . import cluster as cl
        from . import ensemble as ens
        dev, N = X.device, int(X.shape[0])
        nodes32 = ens._node_list(nodes, N, dev)
        K = int(self.out_size if clusters is None else clusters)
        if labels is not None:
            labels = torch.as_tensor(labels).reshape(-1).to(dev)
            if labels.numel() == N:
                labels = labels.index_select(0, nodes32.long())
            elif labels.numel() != nodes32.numel():
                raise ValueError("cluster_probe: %d labels for %d nodes (of %d)" % (labels.numel(), nodes32.numel(), N))
        z = self.embed(X, paths, num_w, walk_len, nodes32, samples=samples, seed=seed, first_epoch=first_epoch,
                       batch_nodes=batch_nodes, head=head)
        found = cl.kmeans(z, K, metric=metric, iters=iters, restarts=restarts, seed=seed)
        if labels is None:
            return found, None
        return found, cl.cluster_scores(found.label, labels.long(), K, int(self.out_size))

    def explain(self, X, neis, num_w, walk_len, indices, layer_type, *, groups="path", num_groups=None, target=None,
                path_weights=None, path_weight_norm="sum", batch_nodes=None, logits=False, contribution=False, totals=None,
                exclude_self=True):
        """Which paths, nodes or edges the prediction of every masked node rests on -> ``pathnet_amd.Explanation`` of device tensors (logits,
        drop_delta, keep_gain, flip, present, target, drop_logits / keep_logits with logits=True, contribution with
        contribution=True, totals), one row per masked node, one column per group.

        drop_delta[s, g] = log p(target) of row s minus log p(target) of the row WITHOUT the members of group g (positive: the
        group supports the class); keep_gain[s, g] = log p(target) with group g ALONE minus log p(target) with no path at all;
        flip[s, g]: the argmax changes without the group.  drop_logits[:, g] are the logits of this module's own
        forward(path_weights=...) with the group's members given weight 0, keep_logits[:, g] those with every other member
        given weight 0 -- but all of them come from ONE encode(path_state=True) forward and one kernel over the paths' final
        hidden states (pn_explain_groups, fp64 on the device): the recurrence never sees the pooling, and the classifier is
        linear after it.  Every cell= works, and any hidden size.

        groups: "path" -- group = member index, G = W.  For PathNet_homo / PAGG member j is path j of the node; for PathNet it
                is SLOT q = j * S + s of the reference's scrambled LSTM batch (encode()'s member order), whose steps come from
                other masked nodes' paths: what the reference pools for node s, not a path of node s.
                "reach" -- group = the largest distance code along the path, G = walk_len; computed from layer_type on the
                device.  PathNet_homo / PAGG only; PathNet raises.
                an int tensor [S, W] in member order, G = num_groups or max + 1 (inferred: one host read); an entry outside
                [0, G) belongs to no group and is never removed.
                "node" -- a group per distinct node the row's members consumed (pathnet_amd.member_nodes): removing node u
                removes every member that passed through u, so the groups overlap (pn_explain_units, pn_explain_overlap).
                G = W * walk_len columns, no host read: Explanation.unit [S, G] holds the row's node ids in ascending order,
                then -1, unit_count [S] how many; units() / top_units(k) read them.  exclude_self (default True) leaves out
                the row's own node, which sits on every path of a PathNet_homo / PAGG row and also enters through the ego
                half of the embedding.  totals is a pathnet_amd.NodeTotals over the graph's nodes (rows_present, members,
                flips, top; summary(k) reads it).  For PathNet this is the readable unit: which nodes' rows a slot's
                recurrence consumed.  walk_len <= 16 and W * walk_len <= 1024, else ValueError.
                "edge" -- a group per distinct undirected edge between consecutive steps (a stay step (u, u) included),
                G = W * (walk_len - 1); unit holds (min << 32) | max, units() the two ends [S, G, 2]; totals is None (an edge
                has no dense index).  PathNet_homo / PAGG only: consecutive consumed nodes are not edges in PathNet's
                scrambled batch, which raises as "reach" does.
        target (int [S]): the class the scores refer to; default the argmax of the row's logits.
        path_weights / path_weight_norm: forward()'s, by sequence slot; a member of weight 0 is in no group's count, and
                "sum" renormalises what remains.  (PathNet: re-ordered to member order for the kernel, w.reshape(W, S).t().)
        batch_nodes: the node list is taken in chunks of that many nodes -- path_state is S * W * H * 4 bytes -- each a
                group_slice of the same batch (PathNet's rows read paths of the batch's other nodes, which a group_slice
                keeps).  The chunks leave the bits of the unchunked call: explain runs its forwards with PN_EVAL_ZW off (and
                puts the knob back), because that shortcut is taken or not by the size of the slice and rounds differently;
                `logits` are therefore within the forward's 1e-5 of forward()'s, not its bits.
        totals: an earlier Explanation.totals to continue (added into, e.g. over epochs of resampled paths); summary() reads it.

        Runs under no_grad in eval mode (no dropout, torch's generator untouched) and restores the training flag.  Not
        covered: the attribution of single steps inside a path (the recurrence is not linear; node and edge groups remove
        whole members), per-node sums of scores, the aggregators of pathnet_amd.dist, and training mode."""
        from .explain import explain as explain_with       # (the package attribute `explain` is this function, not the module)
        return explain_with(self, X, neis, num_w, walk_len, indices, layer_type, groups=groups, num_groups=num_groups,
                            target=target, path_weights=path_weights, path_weight_norm=path_weight_norm,
                            batch_nodes=batch_nodes, logits=logits, contribution=contribution, totals=totals,
                            exclude_self=exclude_self)

    def paths_stream(self):
        """The torch stream on which this module's NEXT call will read its path arrays (neis / layer_type), judged by the
        shape of its last call on the current stream (pn_pagg_paths_stream): the library's second stream when the call forks
        the index plan off, else the current stream.  A training loop that enqueues its sampler there
        (``with torch.cuda.stream(model.paths_stream()): sampler.sample(..., out=bufs)``) takes the walk off the step's
        critical path -- it runs under the tail of the previous step -- without an event on the main stream.  The path
        buffers must then be written by that stream only.  With ``step_state`` set the walk stays on the current stream:
        a sampler driven by the step state reads its epoch and seed from device memory, advanced on this stream."""
        cur = torch.cuda.current_stream()
        last = getattr(self, "_last_shape", None)
        if last is None or self.step_state is not None:
            prev = getattr(self, "_paths_stream_prev", None)
            if prev is not None and prev.cuda_stream != cur.cuda_stream:
                cur.wait_stream(prev)           # (behind the walk handed out last time)
            self._paths_stream_prev = cur
            return cur
        shape, dev = last
        out = ctypes.c_void_p()
        with torch.cuda.device(dev):
            cur = torch.cuda.current_stream(dev)
            _lib.check(_lib.load().pn_pagg_paths_stream(_lib.context(dev), ctypes.byref(shape), _lib.stream_ptr(dev), ctypes.byref(out)))
        new = cur if (not out.value or out.value == cur.cuda_stream) else torch.cuda.ExternalStream(out.value, device=dev)
        # the readers of the previous batch's paths ran on the stream handed out last time: when the answer changes (first
        # steps, pn_profile_configure, another batch shape) the new producer is ordered behind them once, with an event
        prev = getattr(self, "_paths_stream_prev", None)
        if prev is not None and prev.cuda_stream != new.cuda_stream:
            new.wait_stream(prev)
            new.wait_stream(cur)
        self._paths_stream_prev = new
        return new

    # ---- range guard (see _common_init) ---------------------------------------------------------------------------------
    def _range_eval(self, rec):
        x_bits, esum, cnt = int(rec[0]) & 0xFFFFFFFF, int(rec[1]), int(rec[2]) & 0xFFFFFFFF
        if cnt > 0 and x_bits:
            self.range_spread_bits = ((x_bits >> 23) & 255) - esum / cnt
            if self.range_spread_bits > RANGE_WINDOW_BITS and not self._range_wide:
                self._range_wide = True
                import warnings
                warnings.warn("pathnet_amd: the distance-bank rows span %.1f bits between their largest value and the typical row "
                              "(window of the fp16 x 2 recurrent kernels: %d); this module now runs seq_math='bf16x3'"
                              % (self.range_spread_bits, RANGE_WINDOW_BITS))

    def _range_poll(self):
        if self._range_pending is not None and self._range_pending[1].query():
            rec, _ = self._range_pending
            self._range_pending = None
            self._range_eval(rec)

    def _range_read(self, call, ws, sync):
        """start (sync: finish) the read-back of the range record that `call` left in its workspace `ws`"""
        off = ctypes.c_int64(-1)
        _lib.check(_lib.load().pn_pagg_range_offset(ctypes.byref(call.shape()), ctypes.byref(off)))
        if ws is None or off.value < 0:
            return
        rec = torch.empty(6, dtype=torch.int32, pin_memory=True)
        rec.copy_(ws[off.value:off.value + 24].view(torch.int32), non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        if sync:
            ev.synchronize()
            self._range_eval(rec)
        else:
            self._range_pending = (rec, ev)

    def _call_modes(self):
        """(deterministic, compact, seq_math) of a call of this module, as PaggCall takes them"""
        return (deterministic_default() if self.deterministic is None else bool(self.deterministic), compact_default(),
                seq_math_default() if self.seq_math is None else _SEQ_MATH[self.seq_math])

    def _run(self, X, neis, num_w, walk_len, indices, layer_type, reuse_tables=False, group_slice=None, target=None,
             grad_scale=None, fused=None, batch_position=None, seed=None, _math=None, _encode=None, loss=None,
             path_weights=None, path_weight_norm="sum", check_weights=False, path_grad=False):
        """reuse_tables (extension, inference only): X and the weights are those of the previous no-grad forward of this
        module -- the validation and the test forward of an epoch (PathNet_run.py:362, :378) -- so the projected
        feature matrix and the distance bank still sitting in the module's workspace are used again.
        group_slice=(begin, count) (extension): neis / indices / layer_type describe the whole batch as always, but only
        the logits of its masked nodes [begin, begin + count) are computed and returned -- exactly those rows of the
        whole-batch result, also for the hetero class whose rows read paths of other masked nodes of the batch."""
        dev = X.device
        # (the weights are judged first: what is wrong with them does not depend on where the call runs)
        if path_weight_norm not in _PATH_NORM:
            raise ValueError("path_weight_norm=%r: 'sum' or 'count'" % (path_weight_norm,))
        if path_weights is not None:
            rows = int(torch.as_tensor(neis).numel()) // max(int(num_w) * int(walk_len), 1)       # the masked nodes neis describes
            path_weights = as_path_weights(path_weights, rows, int(num_w), check=check_weights, path_grad=bool(path_grad))
        # path_grad counts with grad enabled only (under no_grad the call is the one without it); wgrad: the weights as the
        # differentiable input of the path Functions, or None when they ask for no gradient
        path_grad = bool(path_grad) and torch.is_grad_enabled()
        if path_grad and dev.type == "cuda" and torch.cuda.is_current_stream_capturing():
            raise RuntimeError("path_grad=True is not available while a hipGraph is being captured: the captured training "
                               "steps treat the path weights as data")
        wgrad = None
        if path_weights is not None and path_weights.requires_grad:
            wgrad = path_weights.to(dev).contiguous() if path_grad else None
            path_weights = (wgrad if wgrad is not None else path_weights).detach()
        if dev.type != "cuda":
            raise RuntimeError("pathnet_amd aggregators run on the GPU only (X is on %s); no CPU fallback" % dev)
        X_given = X
        X = X.contiguous().float()
        ids, codes, sel, S = _as_index_tensors(neis, layer_type, indices, num_w, walk_len, dev, n_nodes=X.shape[0])
        H, L = self.hidden_size, int(walk_len)
        Hk = -(-H // 32) * 32           # the kernels' hidden size: H, or H zero-padded to the next multiple of 32
        fw, fb, params = self._param_inputs() if Hk == H else self._padded_param_inputs(Hk)
        training = self.training
        p = self.dropout_p() if training else 0.0
        det, compact, math = self._call_modes()
        if _math is not None:
            math = _math
        guard = (_math is None and self.seq_math is None and self.range_guard and math != _lib.SEQ_MATH_BF16X3 and
                 self.step_state is None)
        if guard:
            self._range_poll()
            if self._range_wide:
                math, guard = _lib.SEQ_MATH_BF16X3, False
        draws = p > 0 and self.step_state is None       # (else the seed is unused, or read from the step state)
        seed = (int(seed) if seed is not None else int(torch.randint(0, 2 ** 62, (1,)).item())) if draws else 0
        S_total = begin = 0
        if batch_position is not None:
            # (data-parallel ranks, dist.ReplicatedAggregator) the S masked nodes of this call are the rows [begin, begin + S)
            # of a batch of S_total whose other rows are computed elsewhere; neis / indices / layer_type hold this call's
            # rows only.  Dropout counters and explicit masks are positions in the whole batch.  Not for the hetero class,
            # whose rows read paths of other masked nodes: give it the whole batch and a group_slice.
            if self.variant == "hetero" or group_slice is not None:
                raise ValueError("batch_position: homo / PAGG classes, without group_slice")
            S_total, begin = int(batch_position[0]), int(batch_position[1])
            if begin < 0 or begin + S > S_total:
                raise ValueError("batch_position (%d, %d): %d rows do not fit" % (S_total, begin, S))
        if group_slice is not None:
            begin, count = int(group_slice[0]), int(group_slice[1])
            if begin < 0 or count < 0 or begin + count > S:
                raise ValueError("group_slice (%d, %d) outside the batch of %d masked nodes" % (begin, count, S))
            S_total, S = S, count
        if len(params) != 10 + 2 * L:
            raise ValueError("walk_len=%d but the module has %d distance layers" % (L, (len(params) - 10) // 2))
        ms, mc = _explicit_masks(self._mask_seq, self._mask_cls, H, Hk, math) if training else (None, None)
        p_drop = p if ms is None and mc is None else 0.0       # explicit masks stand in for the drawn ones
        grad = torch.is_grad_enabled()
        call = PaggCall(self.variant, X.shape[0], X.shape[1], Hk, self.out_size, S, int(num_w), L, S_total, begin, 0,
                        self._cell_kind, det, compact, math, p_seq=p_drop, p_cls=p_drop, seed=seed, mask_seq=ms, mask_cls=mc,
                        step_state=self.step_state, index_rows_local=batch_position is not None, bank_w=fw, bank_b=fb,
                        grad=grad, path_state=bool(_encode), path_weight_norm=path_weight_norm,
                        path_weights=path_weights.to(dev).contiguous() if path_weights is not None else None)
        # (a converted copy of X is a new tensor in every call: nothing to remember it by)
        whole = batch_position is None and group_slice is None
        call.features = self._features_for(X, Hk) if (X is X_given and S > 0 and whole) else None
        self.fc0_route = "sparse" if call.features is not None else "dense"
        self.fc0_route_calls[self.fc0_route] += 1
        call.pick_batch_groups(self.workspace_budget, dev)
        self._last_shape = (call.shape(), dev)       # (paths_stream: where the NEXT call of this shape reads its paths)
        if not grad:
            ws = call.take_workspace(dev, self._ws_eval)
            fits = ws is self._ws_eval
            key = self._tables_key(X, L)
            compact_now = shape_info(call.shape())[0]
            # what the workspace holds: (key, dense) -- Xh for `key`, and with dense also the distance bank over all N * L
            # rows.  A compact call leaves only ITS batch's rows of the bank behind (a later dense call must not
            # read them as the full table), so it hands on Xh alone.
            have_key, have_dense = self._ws_tables if self._ws_tables is not None else (None, False)
            if reuse_tables and fits and have_key == key:
                call.reuse_tables = 1 if (have_dense and not compact_now) else 2
            call.workspace = self._ws_eval = ws
            # the tables are in the workspace after this call only if it computes (or keeps) them: S = 0 returns early
            self._ws_tables = (key, not compact_now) if S > 0 else None
        elif reuse_tables:
            raise RuntimeError("reuse_tables is for no-grad (inference) forwards")
        else:
            call.workspace = call.take_workspace(dev)
            self._ws_tables = None          # a training forward: the weights are about to change
        if target is not None:
            if not grad:
                raise RuntimeError("forward_loss computes gradients: call it with grad enabled")
            target = torch.as_tensor(target)
            if target.numel() != S:
                raise ValueError("target holds %d classes, the batch has %d masked nodes" % (target.numel(), S))
            call.grad_scale = (1.0 / max(S, 1)) if grad_scale is None else float(grad_scale)
            target = target.reshape(-1)
            from . import optim
            if loss is not None and not isinstance(loss, optim.CrossEntropyLoss):
                raise TypeError("forward_loss: loss must be a pathnet_amd.CrossEntropyLoss")
            loss_fn = loss if loss is not None and loss.has_options else None       # (no option set: today's call)
            if loss_fn is not None:     # the options' grad_scale multiplies the reduced loss
                call.loss = (loss_fn, 1.0 if grad_scale is None else float(grad_scale) * max(S, 1))
            if fused is None:
                fused = call.batch_groups > 0
            if fused and wgrad is not None:
                res = _PaggPathLossFunction.apply(call, wgrad, X, ids, codes, sel, target, *params)
            elif fused:
                res = _PaggLossFunction.apply(call, X, ids, codes, sel, target, *params)
            else:
                if wgrad is not None:
                    out = _PaggPathFunction.apply(call, False, wgrad, X, ids, codes, sel, *params)
                else:
                    out = _PaggFunction.apply(call, X, ids, codes, sel, *params)
                value = (loss_fn or optim.CrossEntropyLoss())(out, target.to(device=dev, dtype=torch.int64))
                if grad_scale is not None:      # (the plain loss: the mean over the S rows)
                    value = value * (float(grad_scale) * max(S, 1))
                res = (value, out)
        elif _encode is not None and path_grad:     # (the per-path outputs are differentiable, whatever the weights ask for)
            res = _PaggPathFunction.apply(call, True, wgrad, X, ids, codes, sel, *params)
        elif _encode is not None:       # (encode(): _encode = whether the paths' final hidden states are wanted)
            res = _PaggEncodeFunction.apply(call, X, ids, codes, sel, *params)
        elif wgrad is not None:
            res = _PaggPathFunction.apply(call, False, wgrad, X, ids, codes, sel, *params)
        else:
            res = _PaggFunction.apply(call, X, ids, codes, sel, *params)
        if guard and S > 0:
            first = self._range_calls == 0
            self._range_calls += 1
            if first or (self._range_calls % RANGE_POLL_EVERY == 0 and self._range_pending is None):
                self._range_read(call, call.workspace, sync=first)
                if first and self._range_wide:      # the very first result is not handed out on a range it cannot carry
                    return self._run(X, neis, num_w, walk_len, indices, layer_type, reuse_tables=False, group_slice=group_slice,
                                     target=target, grad_scale=grad_scale, fused=fused, batch_position=batch_position,
                                     seed=seed, _math=_lib.SEQ_MATH_BF16X3, _encode=_encode, loss=loss,
                                     path_weights=wgrad if wgrad is not None else path_weights,
                                     path_weight_norm=path_weight_norm, path_grad=path_grad)
        return res


class PathNet(_Aggregator):
    """PathNet_run.py:150-211.  state_dict: fc0, LSTM, fc2, nets.<d>, attw."""
    variant = "hetero"

    def __init__(self, feature_length, hidden_size, out_size, wl, dropout=None, cell=None, **kwargs):
        super().__init__()
        self._common_init(feature_length, hidden_size, out_size, dropout, cell)
        self.fc0 = nn.Linear(feature_length, hidden_size)
        self._make_cell("lstm")
        self.fc2 = nn.Linear(2 * hidden_size, out_size)
        self.nets = nn.ModuleList([nn.Linear(hidden_size, hidden_size) for _ in range(wl)])
        self.attw = nn.Linear(2 * hidden_size, 1)
        self.Lrelu = nn.LeakyReLU()

    def _bank_layers(self):
        return list(self.nets)


class PathNet_homo(PathNet):
    """PathNet_run.py:214-278 (xavier_uniform on fc0/fc2, :236-237)."""
    variant = "homo"

    def __init__(self, feature_length, hidden_size, out_size, wl, dropout=None, cell=None, **kwargs):
        super().__init__(feature_length, hidden_size, out_size, wl, dropout=dropout, cell=cell, **kwargs)
        nn.init.xavier_uniform_(self.fc0.weight)
        nn.init.xavier_uniform_(self.fc2.weight)


class PAGG(_Aggregator):
    """baseline/GPRGNN/src/copy.py:299-359.  state_dict: fc0, RNN, fc2, nei0..nei3.  dropout is 0.9 there."""
    variant = "pagg"

    def __init__(self, feature_length, hidden_size, out_size, node_num, dropout=0.9, cell=None, **kwargs):
        super().__init__()
        self._common_init(feature_length, hidden_size, out_size, dropout, cell)
        self.node_num = node_num
        self.fc0 = nn.Linear(feature_length, hidden_size)
        self._make_cell("rnn")
        self.fc2 = nn.Linear(2 * hidden_size, out_size)
        self.nei0 = nn.Linear(hidden_size, hidden_size)
        self.nei1 = nn.Linear(hidden_size, hidden_size)
        self.nei2 = nn.Linear(hidden_size, hidden_size)
        self.nei3 = nn.Linear(hidden_size, hidden_size)
        for lin in (self.fc0, self.fc2, self.nei0, self.nei1, self.nei2, self.nei3):
            nn.init.xavier_uniform_(lin.weight)

    def _bank_layers(self):
        return [self.nei0, self.nei1, self.nei2, self.nei3]
