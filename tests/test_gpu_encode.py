"""encode(): node embeddings, path weights and final path states next to the logits (pn_pagg_args.out_* / g_embed), against
the CPU oracle -- values, member order, gradients of losses over logits and embedding, micro-batches, slices, the
deterministic backward and a captured step."""
import numpy as np
import pytest
import torch

from oracle import pagg_oracle as po
from gradcheck import assert_grads_close, named_grads
from test_gpu_pagg import TOL_OUT, zero_ok

pytestmark = pytest.mark.gpu


def make(variant, F, H, C, L, N, cell=None, seed=0):
    import pathnet_amd
    torch.manual_seed(seed)
    cls = {"hetero": pathnet_amd.PathNet, "homo": pathnet_amd.PathNet_homo, "pagg": pathnet_amd.PAGG}[variant]
    m = cls(F, H, C, L if variant != "pagg" else N, cell=cell).cuda()
    with torch.no_grad():
        for k, v in m.named_parameters():
            if k.endswith("bias") or "bias_" in k:
                v.uniform_(-0.3, 0.3)
    return m


def case(rng, N, S, W, L):
    mask = np.zeros(N, bool)
    mask[rng.permutation(N)[:S]] = True
    sel = np.flatnonzero(mask)
    ids = rng.integers(0, N, (S, W, L))
    ids[:, :, 0] = sel[:, None]
    codes = np.minimum(rng.integers(0, L, (S, W, L)), np.arange(L)[None, None, :])
    return mask, sel, ids, codes


def args(ids, codes, mask, W, L):
    S = int(mask.sum())
    return (torch.as_tensor(ids.reshape(S, W * L).astype(np.int64)), W, L, mask, torch.as_tensor(codes.astype(np.int64)))


def oracle(variant, m, X, ids, codes, sel, W, L, cell=None, drop_seq=None, drop_cls=None):
    """(logits, embedding, path weights [S, W], path states [S, W, H]) of the oracle; parameters / X differentiable"""
    pr = {k: v.detach().cpu().clone().requires_grad_(True) for k, v in m.state_dict().items()}
    Xo = X.detach().cpu().clone().requires_grad_(True)
    out, it = po.forward(variant, pr, Xo, ids, codes, sel, W, L, drop_seq=drop_seq, drop_cls=drop_cls, cell=cell,
                         return_intermediates=True)
    S = len(sel)
    emb = torch.cat([it["Xh"][torch.as_tensor(sel, dtype=torch.long)], it["pooled"]], dim=1)
    att = it["att"]
    if variant == "hetero":
        pw = att.detach().view(S, W)
    elif variant == "homo":
        pw = 1.0 + att.detach().view(S, W)
    else:
        pw = torch.ones(S, W)
    s, j = np.meshgrid(np.arange(S), np.arange(W), indexing="ij")
    q = j * S + s if variant == "hetero" else s * W + j
    ps = it["h"].detach()[torch.as_tensor(q.reshape(-1))].view(S, W, -1)
    return out, emb, pw, ps, pr, Xo


CELLS = [None, "gru", "mean"]


@pytest.mark.parametrize("variant", ["hetero", "homo", "pagg"])
@pytest.mark.parametrize("cell", CELLS)
@pytest.mark.parametrize("H", [32, 128, 100])
def test_encode_outputs_match_the_oracle(variant, cell, H):
    rng = np.random.default_rng(81)
    N, F, C, W, L, S = 60, 16, 4, 9, 4, 23
    m = make(variant, F, H, C, L, N, cell, seed=81).eval()
    mask, sel, ids, codes = case(rng, N, S, W, L)
    X = torch.rand(N, F)
    Xd = X.cuda()
    with torch.no_grad():
        want_logits = m(Xd, *args(ids, codes, mask, W, L))
        enc = m.encode(Xd, *args(ids, codes, mask, W, L), path_state=True)
    assert torch.equal(enc.logits, want_logits)
    assert enc.embedding.shape == (S, 2 * H) and enc.path_weight.shape == (S, W) and enc.path_state.shape == (S, W, H)
    out, emb, pw, ps, _, _ = oracle(variant, m, X, ids, codes, sel, W, L, cell)
    assert (enc.logits.cpu() - out.detach()).abs().max().item() < TOL_OUT
    assert (enc.embedding.cpu() - emb.detach()).abs().max().item() < TOL_OUT
    assert (enc.path_weight.cpu() - pw).abs().max().item() < TOL_OUT
    assert (enc.path_state.cpu() - ps).abs().max().item() < TOL_OUT
    if variant == "hetero":
        assert (enc.path_weight.sum(1).cpu() - 1.0).abs().max().item() < 1e-5
    with torch.no_grad():
        assert m.encode(Xd, *args(ids, codes, mask, W, L)).path_state is None


def _grad_case(variant, train, embed_only, H=64, cell=None):
    rng = np.random.default_rng(82)
    N, F, C, W, L, S = 64, 18, 5, 10, 4, 27
    m = make(variant, F, H, C, L, N, cell, seed=82)
    mask, sel, ids, codes = case(rng, N, S, W, L)
    X = torch.rand(N, F)
    R = torch.randn(S, 2 * H)
    Y = torch.as_tensor(rng.integers(0, C, S))
    drop_seq = drop_cls = None
    if train:
        drop_seq = (torch.rand(L, S * W, H) >= 0.5).float() / 0.5
        drop_cls = (torch.rand(S, 2 * H) >= 0.5).float() / 0.5
        m.train()
        m._mask_seq, m._mask_cls = drop_seq.cuda(), drop_cls.cuda()
    else:
        m.eval()
    Xd = X.cuda().requires_grad_(True)
    enc = m.encode(Xd, *args(ids, codes, mask, W, L))
    loss = (enc.embedding * R.cuda()).sum()
    if not embed_only:
        loss = loss + torch.nn.functional.cross_entropy(enc.logits, Y.cuda())
    loss.backward()
    out, emb, _, _, pr, Xo = oracle(variant, m, X, ids, codes, sel, W, L, cell, drop_seq, drop_cls)
    assert (enc.embedding.detach().cpu() - emb.detach()).abs().max().item() < TOL_OUT
    lo = (emb * R).sum()
    if not embed_only:
        lo = lo + torch.nn.functional.cross_entropy(out, Y)
    lo.backward()
    ref = {k: pr[k].grad for k, _ in m.named_parameters()}
    ref["X"] = Xo.grad
    got = named_grads(m, {"X": Xd.grad})
    if embed_only:
        for k in ("fc2.weight", "fc2.bias"):
            assert torch.count_nonzero(got.pop(k)).item() == 0, k
            ref.pop(k)
    assert_grads_close(got, ref, zero_ok=zero_ok(variant))


@pytest.mark.parametrize("variant", ["hetero", "homo", "pagg"])
@pytest.mark.parametrize("train", [False, True])
def test_gradients_of_logits_and_embedding_match_the_oracle(variant, train):
    _grad_case(variant, train, embed_only=False)


@pytest.mark.parametrize("variant", ["hetero", "homo", "pagg"])
@pytest.mark.parametrize("train", [False, True])
def test_embedding_only_loss_matches_the_oracle_and_leaves_fc2_at_zero(variant, train):
    _grad_case(variant, train, embed_only=True)


@pytest.mark.parametrize("variant,cell,H", [("hetero", None, 100), ("homo", "gru", 288), ("pagg", "mean", 320)])
def test_gradients_at_padded_and_generic_hidden_sizes(variant, cell, H):
    _grad_case(variant, True, embed_only=False, H=H, cell=cell)


def _loss_grads(m, X, a, R, G):
    m.zero_grad()
    Xd = X.clone().requires_grad_(True)
    enc = m.encode(Xd, *a, path_state=True)
    ((enc.logits * G).sum() + (enc.embedding * R).sum()).backward()
    return enc, {k: v.clone() for k, v in named_grads(m, {"X": Xd.grad}).items()}


@pytest.mark.parametrize("variant", ["hetero", "homo", "pagg"])
@pytest.mark.parametrize("train", [False, True])
def test_micro_batches_equal_one_batch(variant, train):
    from pathnet_amd import modules
    rng = np.random.default_rng(83)
    N, F, H, C, W, L, S = 80, 20, 64, 4, 11, 4, 47
    m = make(variant, F, H, C, L, N, seed=83)
    mask, sel, ids, codes = case(rng, N, S, W, L)
    X = torch.rand(N, F).cuda()
    R, G = torch.randn(S, 2 * H).cuda(), torch.randn(S, C).cuda()
    if train:
        m.train()
        m._mask_seq = ((torch.rand(L, S * W, H) >= 0.5).float() / 0.5).cuda()
        m._mask_cls = ((torch.rand(S, 2 * H) >= 0.5).float() / 0.5).cuda()
    else:
        m.eval()
    a = args(ids, codes, mask, W, L)
    one, g1 = _loss_grads(m, X, a, R, G)
    kw = dict(cell=m._cell_kind, deterministic=modules.deterministic_default(), compact=modules.compact_default())
    m.workspace_budget = modules.workspace_bytes(variant, N, F, H, C, S, W, L, batch_groups=10, **kw)
    bg = modules.pick_batch_groups(variant, N, F, H, C, S, W, L, m.workspace_budget, **kw)
    assert 0 < bg < S, bg
    many, gb = _loss_grads(m, X, a, R, G)
    for k in ("logits", "embedding", "path_weight", "path_state"):
        assert (getattr(many, k) - getattr(one, k)).abs().max().item() < 2e-6, k
    assert_grads_close(gb, g1, rel=2e-5, zero_ok=zero_ok(variant))


@pytest.mark.parametrize("variant", ["hetero", "homo", "pagg"])
def test_slice_rows_are_rows_of_the_whole_batch(variant):
    rng = np.random.default_rng(84)
    N, F, H, C, W, L, S = 70, 20, 64, 3, 9, 4, 41
    m = make(variant, F, H, C, L, N, seed=84).eval()
    mask, sel, ids, codes = case(rng, N, S, W, L)
    X = torch.rand(N, F).cuda()
    a = args(ids, codes, mask, W, L)
    with torch.no_grad():
        whole = m.encode(X, *a, path_state=True)
        for begin, count in ((0, 13), (13, 20), (33, 8)):
            part = m.encode(X, *a, path_state=True, group_slice=(begin, count))
            for k in ("logits", "embedding", "path_weight", "path_state"):
                assert torch.equal(getattr(part, k), getattr(whole, k)[begin:begin + count]), (k, begin, count)


@pytest.mark.parametrize("variant", ["hetero", "homo"])
def test_deterministic_backward_with_g_embed_is_bitwise_reproducible(variant):
    rng = np.random.default_rng(85)
    N, F, H, C, W, L, S = 60, 16, 64, 4, 10, 4, 33
    m = make(variant, F, H, C, L, N, seed=85).eval()
    m.deterministic = True
    mask, sel, ids, codes = case(rng, N, S, W, L)
    X = torch.rand(N, F).cuda()
    R, G = torch.randn(S, 2 * H).cuda(), torch.randn(S, C).cuda()
    a = args(ids, codes, mask, W, L)
    _, g1 = _loss_grads(m, X, a, R, G)
    _, g2 = _loss_grads(m, X, a, R, G)
    for k in g1:
        assert torch.equal(g1[k], g2[k]), k
    m.zero_grad()
    Xd = X.clone().requires_grad_(True)
    (m.encode(Xd, *a).embedding * R).sum().backward()            # g_out NULL
    e1 = {k: v.clone() for k, v in named_grads(m, {"X": Xd.grad}).items()}
    m.zero_grad()
    Xd = X.clone().requires_grad_(True)
    (m.encode(Xd, *a).embedding * R).sum().backward()
    for k, v in dict(named_grads(m), X=Xd.grad).items():
        assert torch.equal(v, e1[k]), k


@pytest.mark.parametrize("variant", ["hetero", "pagg"])
def test_forward_and_forward_loss_unchanged_by_encode(variant):
    rng = np.random.default_rng(86)
    N, F, H, C, W, L, S = 60, 16, 64, 4, 10, 4, 29
    m = make(variant, F, H, C, L, N, seed=86).eval()
    m.deterministic = True
    mask, sel, ids, codes = case(rng, N, S, W, L)
    X = torch.rand(N, F).cuda()
    Y = torch.as_tensor(rng.integers(0, C, S)).cuda()
    a = args(ids, codes, mask, W, L)

    def run():
        with torch.no_grad():
            out = m(X, *a)
        m.zero_grad()
        loss, logits = m.forward_loss(X, *a, Y)
        loss.backward()
        return [out, loss.detach(), logits.detach()] + [v.grad.clone() for _, v in m.named_parameters()]

    before = run()
    enc = m.encode(X, *a, path_state=True)
    (enc.embedding.sum() + enc.logits.sum()).backward()
    after = run()
    for x, y in zip(before, after):
        assert torch.equal(x, y)


def test_encode_step_captured_in_a_hip_graph_replays_equal_to_eager():
    """encode + a loss over logits and embedding + the gradients, captured as one hipGraph (device-resident index arrays,
    no dropout: nothing the host decides per step) -- the replay computes what the eager step computes."""
    rng = np.random.default_rng(87)
    N, F, H, C, W, L, S = 120, 24, 64, 4, 10, 4, 50
    m = make("homo", F, H, C, L, N, seed=87).eval()
    m.range_guard = False           # (its read-backs are host round trips; the capture has none)
    mask, sel, ids, codes = case(rng, N, S, W, L)
    X = torch.rand(N, F).cuda()
    neis = torch.as_tensor(ids.reshape(S, W * L), dtype=torch.int32).cuda()
    lt = torch.as_tensor(codes, dtype=torch.uint8).cuda()
    sel32 = torch.as_tensor(sel, dtype=torch.int32).cuda()
    Y = torch.as_tensor(rng.integers(0, C, S)).cuda()
    R = torch.randn(S, 2 * H).cuda()
    params = [v for _, v in m.named_parameters()]
    outs = [torch.zeros_like(p) for p in params] + [torch.zeros((), device="cuda"), torch.zeros(S, 2 * H, device="cuda")]

    def step():
        enc = m.encode(X, neis, W, L, sel32, lt)
        loss = torch.nn.functional.cross_entropy(enc.logits, Y) + (enc.embedding * R).sum()
        grads = torch.autograd.grad(loss, params)
        for o, g in zip(outs, list(grads) + [loss.detach(), enc.embedding.detach()]):
            o.copy_(g)

    step()
    torch.cuda.synchronize()
    eager = [o.clone() for o in outs]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()                      # warm-up on the capture's stream
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        step()
    for _ in range(2):
        for o in outs:
            o.zero_()
        g.replay()
        torch.cuda.synchronize()
        for k, (x, y) in enumerate(zip(outs, eager)):
            assert (x - y).abs().max().item() <= 1e-5 * max(1.0, y.abs().max().item()), k
