"""Probe parameters that turn the aggregator into a read-out of its dropout masks, and the decoders of that read-out.
Shared by tests/test_dropout_host.py, which proves every construction on the CPU oracle alone (oracle/pagg_oracle.py with
the reference masks of tests/dropout_ref.py: every bit of both masks is read back), and tests/test_gpu_dropout_masks.py,
which decodes the library's outputs with the same functions.

The construction.  F = H, X = 0, fc0 = (I, 1): every projected row is 1, also after the homo class's ReLU.  The distance
layer of code t is (0.5 amp[t] I, 0.5 amp[t]), so y = amp[t] at step t of every path (codes[q, t] = t) and 0 where amp[t] = 0.
amp is 1 - p at an active step: the recurrent input is 1 (up to rounding) where the bit is kept and exactly 0 where it is
dropped, at every p, so no activation saturates and no derivative vanishes.  The attention weights are 0.  The cells pass
a positive input on as a positive state and an exact zero as an exact zero:

    rnn   W_ih = 0.5 I, W_hh = I, bias b       h = tanh(0.5 x + h + b)
    lstm  g block of W_ih = I, the rest 0, W_hh = 0, biases i, f, o = +10, g = b
                                               c = s c + s tanh(x + b), h = s tanh(c), s = sigmoid(10)
    gru   W_in = I, the rest 0, b_in = b       h = 0.5 tanh(x + b) + 0.5 h
    mean / sum                                 amp[t] = 2^t: at p = 0.5 the state is the exact integer sum of the kept steps' 2^(t+1)

With b = 0 and ONE active step t the final state of slot q is > 0 exactly where bit (t, q, h) is kept.  With b = 1 and every
step active the embedding is > 0 everywhere, so fc2.weight.grad under a one-hot upstream gradient is non-zero exactly where
the classifier's bit is kept.  With every step active, all path nodes distinct and a loss over the pooled half of the
embedding, X.grad[node(q, t), h] is non-zero exactly where the backward's bit (t, q, h) is kept."""
import numpy as np
import torch

from oracle import pagg_oracle as po

N = 300
_GATES = {"lstm": 4, "gru": 3, "rnn": 1}
_NAME = {"lstm": "LSTM", "gru": "GRU", "rnn": "RNN"}


def cell_kind(variant, cell):
    return cell or ("rnn" if variant == "pagg" else "lstm")


def amp_one_step(p, L, t):
    a = np.zeros(L, np.float32)
    a[t] = np.float32(1) - np.float32(p)
    return a


def amp_every_step(p, L):
    return np.full(L, np.float32(1) - np.float32(p), np.float32)


def amp_powers(L):
    return (2.0 ** np.arange(L)).astype(np.float32)


def params(variant, cell, H, L, C, amp, cell_bias=0.0):
    """reference state_dict keys -> fp32 tensors of the probe"""
    kind = cell_kind(variant, cell)
    eye = torch.eye(H)
    sd = {"fc0.weight": eye.clone(), "fc0.bias": torch.ones(H)}
    for t in range(L):
        name = ("nei%d" % t) if variant == "pagg" else ("nets.%d" % t)
        sd[name + ".weight"] = eye * (0.5 * float(amp[t]))
        sd[name + ".bias"] = torch.full((H,), 0.5 * float(amp[t]))
    if kind in _GATES:
        G, nm = _GATES[kind], _NAME[kind]
        w_ih, b_ih = torch.zeros(G, H, H), torch.zeros(G, H)
        w_hh = torch.zeros(G, H, H)
        if kind == "rnn":
            w_ih[0], w_hh[0], b_ih[0] = 0.5 * eye, eye, cell_bias
        elif kind == "lstm":                                # torch gate order i, f, g, o
            w_ih[2] = eye
            b_ih[0], b_ih[1], b_ih[2], b_ih[3] = 10.0, 10.0, cell_bias, 10.0
        else:                                               # torch gate order r, z, n
            w_ih[2], b_ih[2] = eye, cell_bias
        sd[nm + ".weight_ih_l0"], sd[nm + ".weight_hh_l0"] = w_ih.reshape(G * H, H), w_hh.reshape(G * H, H)
        sd[nm + ".bias_ih_l0"], sd[nm + ".bias_hh_l0"] = b_ih.reshape(G * H), torch.zeros(G * H)
    if variant != "pagg":
        sd["attw.weight"], sd["attw.bias"] = torch.zeros(1, 2 * H), torch.zeros(1)
    sd["fc2.weight"], sd["fc2.bias"] = torch.full((C, 2 * H), 1.0 / C), torch.zeros(C)
    return sd


def paths(S, W, L, seed=0, ego_first=False):
    """(sel [S], ids [S, W, L], codes [S, W, L]): codes[.., t] = t; the S W L path nodes all distinct and none of them a
    masked node -- or, with ego_first, column 0 the masked node itself (the homo plan then merges every node's W step-0 rows)"""
    rng = np.random.default_rng(seed)
    perm = rng.permutation(N)
    need = S + S * W * L
    assert need <= N
    sel = np.sort(perm[:S])
    ids = perm[S:need].reshape(S, W, L).astype(np.int32)
    if ego_first:
        ids[:, :, 0] = sel[:, None]
    codes = np.broadcast_to(np.arange(L, dtype=np.uint8), (S, W, L)).copy()
    return sel, ids, codes


def slots(variant, S_total, W, begin=0, count=None):
    """[count, W] sequence slot of member j of row begin + s (the member order of encode()'s path_state)"""
    count = S_total - begin if count is None else count
    s = np.arange(begin, begin + count)[:, None]
    j = np.arange(W)[None, :]
    return j * S_total + s if variant == "hetero" else s * W + j


def oracle_run(variant, cell, sd, X, sel, ids, codes, W, L, drop_seq, drop_cls, loss=None, dtype=torch.float32):
    """The module surface on the CPU oracle: -> dict(logits, embedding [S, 2H], path_state [S, W, H]) and, with
    loss(logits, embedding) given, the gradients {"X": ..., parameter names: ...} of that scalar."""
    S = len(sel)
    want_grad = loss is not None
    p = {k: v.clone().to(dtype).requires_grad_(want_grad) for k, v in sd.items()}
    Xr = X.clone().to(dtype).requires_grad_(want_grad)
    out, mid = po.forward(variant, p, Xr, ids, codes, sel, W, L, drop_seq=drop_seq, drop_cls=drop_cls, dtype=dtype,
                          return_intermediates=True, cell=cell)
    _, _, group, member, _ = po.plan(variant, ids, codes, S, W, L)
    order = torch.from_numpy(np.argsort(group * W + member, kind="stable"))
    emb = torch.cat([mid["Xh"][torch.as_tensor(np.asarray(sel), dtype=torch.long)], mid["pooled"]], dim=1)
    res = {"logits": out.detach(), "embedding": emb.detach(), "path_state": mid["h"][order].view(S, W, -1).detach()}
    if want_grad:
        loss(out, emb).backward()
        res["grads"] = {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in p.items()}
        res["grads"]["X"] = Xr.grad if Xr.grad is not None else torch.zeros_like(Xr)
    return res


# ---- decoders: the same code reads the oracle's outputs and the library's ------------------------------------------------
def put_forward_bits(bits, t, path_state, slot):
    """bits [L, P_total, H] (bool, filled in place): step t's bits of the slots `slot` [rows, W] from the final states
    [rows, W, H] of the run whose only active step is t"""
    bits[t, torch.as_tensor(slot).reshape(-1)] = path_state.reshape(-1, path_state.shape[-1]).cpu() > 0


def put_sum_bits(bits, path_state, slot, L, mean):
    """mean / sum encoders at p = 0.5 with amp = 2^t: the state is sum_t bit_t 2^(t+1) (/ L) exactly"""
    v = path_state.reshape(-1, path_state.shape[-1]).cpu().double() * (L if mean else 1) / 2.0
    n = v.round().long()
    assert torch.equal(n.double(), v) and int(n.min()) >= 0 and int(n.max()) < 2 ** L, "not the exact sum of kept steps"
    idx = torch.as_tensor(slot).reshape(-1)
    for t in range(L):
        bits[t, idx] = ((n >> t) & 1).bool()


def classifier_bits(fc2_grads, S, C):
    """fc2.weight.grad [C, 2H] of pass k under the upstream gradient one_hot_pass(S, C, k) -> bits [S, 2H]"""
    rows = [fc2_grads[s // C][s % C].cpu() != 0 for s in range(S)]
    return torch.stack(rows)


def one_hot_pass(S, C, k):
    G = torch.zeros(S, C)
    for s in range(k * C, min(S, (k + 1) * C)):
        G[s, s % C] = 1.0
    return G


def backward_bits(x_grad, node):
    """X.grad [N, H] and the plan's node [P, L] (all distinct) -> bits [L, P, H]"""
    g = x_grad.cpu()
    return (g[torch.as_tensor(node).t().reshape(-1)] != 0).view(node.shape[1], node.shape[0], -1)


def group_of(variant, S, W):
    """pooling group of every sequence slot (oracle/pagg_oracle.py: plan)"""
    q = np.arange(S * W)
    return q % S if variant == "hetero" else q // W


def joint_bits(x_grads, sel, node, S, W, C, variant):
    """What X.grad of the classifier read-out's passes shows (x_grads[k]: pass k, a loss over the logits): the classifier's
    ego half alone on the masked nodes' rows [S, H], and on the row of (slot q, step t) the sequence bit AND the pooled
    half's bit of q's pooling group [L, P, H]"""
    ego = torch.stack([x_grads[s // C][sel[s]] != 0 for s in range(S)])
    group = group_of(variant, S, W)
    rows = [x_grads[group[q] // C][torch.as_tensor(node[q])] != 0 for q in range(S * W)]
    return ego, torch.stack(rows, dim=1)


def pooled_loss(H):
    """a loss over the pooled half of the embedding, which the classifier's mask does not touch"""
    return lambda logits, emb: emb[:, H:].sum()


def merged_counts(x_grad_rows, unit):
    """homo plan with column 0 = the masked node and step 0 the only active step: X.grad on node s's row is `unit` times
    the number of kept step-0 bits among its W paths -> the counts [S, H] (exact integers or the assertion fails)"""
    v = x_grad_rows.cpu().double() / unit
    n = v.round()
    assert float((v - n).abs().max()) < 1e-3, "not a whole number of equal contributions"
    return n.long()


# (variant, cell, H, S, W, L, p): P = S W in {1, 33, 65}, L in {1, 4} (PAGG has its four distance layers), every p, the fused
# sizes 32 / 96 / 128 / 256, H = 100 (the kernels run at 128), H = 288 (the step-by-step recurrence), mean / sum at p = 0.5
PROBE_CASES = [
    ("homo", None, 128, 13, 5, 4, 0.5),
    ("homo", None, 128, 1, 1, 1, 0.1),
    ("homo", None, 32, 11, 3, 4, 0.9),
    ("homo", "gru", 96, 13, 5, 4, 0.5),
    ("homo", "rnn", 256, 11, 3, 1, 0.1),
    ("homo", None, 256, 13, 5, 4, 0.9),
    ("hetero", None, 128, 11, 3, 4, 0.9),
    ("hetero", "gru", 32, 13, 5, 1, 0.5),
    ("hetero", None, 96, 1, 1, 4, 0.1),
    ("hetero", None, 256, 11, 3, 4, 0.5),
    ("pagg", None, 128, 13, 5, 4, 0.9),
    ("pagg", None, 32, 11, 3, 4, 0.5),
    ("pagg", "lstm", 256, 1, 1, 4, 0.1),
    ("pagg", "gru", 96, 11, 3, 4, 0.1),
    ("homo", None, 100, 11, 3, 4, 0.5),
    ("hetero", None, 100, 13, 5, 4, 0.9),
    ("homo", None, 288, 11, 3, 4, 0.5),
    ("pagg", None, 288, 13, 5, 4, 0.1),
    ("hetero", "gru", 288, 1, 1, 1, 0.9),
    ("homo", "mean", 128, 13, 5, 4, 0.5),
    ("homo", "sum", 96, 11, 3, 4, 0.5),
    ("hetero", "sum", 32, 13, 5, 1, 0.5),
    ("pagg", "mean", 128, 1, 1, 4, 0.5),
    ("hetero", "mean", 288, 11, 3, 4, 0.5),
]
REDUCING = ("mean", "sum")


def case_id(case):
    v, cell, H, S, W, L, p = case
    return "%s-%s-H%d-S%dW%dL%d-p%g" % (v, cell or "own", H, S, W, L, p)
