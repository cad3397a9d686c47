"""contrastive_loss through autograd, two encode() calls in one graph, and pretrain() end to end, on a small planted-partition
graph built here (96 nodes in 2 blocks; W = 4, L = 3, H = 32, F = 16).  PAGG has four distance layers, one per path
position, so its cases walk L = 4 on the same graph.

Wherever two runs are compared bit for bit the models run the fixed-order backward (``model.deterministic = True``): the
aggregators' default backward adds some gradients with fp32 atomics, whose order differs from run to run."""
import copy
import functools

import numpy as np
import pytest
import torch

import contrast_ref as ref
from gradcheck import assert_grads_close, named_grads

pytestmark = pytest.mark.gpu

N, F, W, L, H, C = 96, 16, 4, 3, 32, 2
NOISE = 1.0
CLASSES = ("PathNet_homo", "PAGG")


def length_of(name):
    return 4 if name == "PAGG" else L


@functools.lru_cache(None)
def graph(L=L, noise=NOISE):
    """-> (sampler, X on the GPU, block of every node): edges inside a block with probability 0.2, across with 0.01; the
    features are the block's signal in 4 of the 16 columns plus noise of scale `noise`"""
    import pathnet_amd
    rng = np.random.default_rng(4)
    block = (np.arange(N) >= N // 2).astype(np.int64)
    prob = np.where(block[:, None] == block[None, :], 0.2, 0.01)
    adj = np.triu(rng.random((N, N)) < prob, 1)
    adj = adj | adj.T | np.eye(N, dtype=bool)
    src, dst = np.nonzero(adj)                      # sorted by (src, dst); both directions and the self loops
    deg = adj.sum(axis=1)
    p = 1.0 / deg[src]
    smp = pathnet_amd.MerwSampler(N, src.astype(np.int32), dst.astype(np.int32), p, L)
    X = torch.from_numpy((noise * rng.standard_normal((N, F)) + 1.5 * (2 * block[:, None] - 1) * (np.arange(F) < 4)).astype(np.float32))
    return smp, X.cuda(), block


def model_of(name, seed=3):
    import pathnet_amd
    torch.manual_seed(seed)
    m = getattr(pathnet_amd, name)(F, H, C, length_of(name)).cuda()
    m.deterministic = True
    return m


def head_of(seed=8):
    torch.manual_seed(seed)
    return torch.nn.Sequential(torch.nn.Linear(2 * H, 32), torch.nn.ReLU(), torch.nn.Linear(32, 16)).cuda()


def all_nodes():
    return torch.arange(N, dtype=torch.int32, device="cuda")


@pytest.mark.parametrize("intra", (True, False))
def test_contrastive_loss_through_autograd(intra):
    import pathnet_amd
    A, B, valid = ref.make_inputs("valid", 70, 19)
    a, b = (torch.tensor(x, device="cuda", requires_grad=True) for x in (A, B))
    got = pathnet_amd.contrastive_loss(a, b, temperature=0.5, intra=intra, valid=valid)
    pathnet_amd.backward(got.loss * 1.0)
    a64, b64 = (torch.tensor(x, dtype=torch.float64, requires_grad=True) for x in (A, B))
    live = torch.from_numpy(valid != 0)
    z = torch.nn.functional.normalize(torch.cat((a64, b64)), dim=1, eps=0.0)
    s = z @ z.t() / 0.5
    r = torch.arange(140)
    live2 = torch.cat((live, live))
    mask = live2[:, None] & live2[None, :] & (r[:, None] != r[None, :])
    if not intra:
        mask &= (r[:, None] >= 70) != (r[None, :] >= 70)
    rows = torch.logsumexp(s.masked_fill(~mask, float("-inf")), dim=1) - s[r, (r + 70) % 140]
    want = torch.where(live2, rows, torch.zeros_like(rows)).sum() / (2 * live.sum())
    want.backward()
    assert got.loss.dtype == torch.float32 and got.loss.dim() == 0
    assert abs(float(got.loss.detach()) - float(want.detach())) <= 3e-5 * abs(float(want.detach()))
    assert_grads_close({"a": a.grad, "b": b.grad}, {"a": a64.grad, "b": b64.grad})
    summ = got.summary()
    assert summ["pairs"] == int(live.sum()) and summ["bad_pairs"] == 0 and 0 <= summ["hits"] <= 2 * summ["pairs"]
    assert got.row_loss.shape == (140,) and not got.row_loss.requires_grad
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pathnet_amd.contrastive_loss(a.detach().cpu(), b.detach().cpu())
    half = pathnet_amd.contrastive_loss(a.detach().half(), b.detach().double(), intra=intra, valid=valid)      # converted
    assert abs(float(half.loss) - float(want.detach())) <= 5e-3 * abs(float(want.detach()))


@pytest.mark.parametrize("name", CLASSES)
def test_two_encodes_in_one_graph(name):
    """parameter gradients of contrastive_loss(enc1.embedding, enc2.embedding) against the sum of two single-view backwards
    fed the reference's dA and dB: the second forward does not disturb what the first saved"""
    import pathnet_amd
    Ln = length_of(name)
    smp, X, _ = graph(Ln)
    nodes = all_nodes()[5:75].contiguous()
    m = model_of(name).train()
    views = []
    for v in (0, 1):
        i, c = smp.sample(W, 7, epoch_begin=v, epoch_count=1, nodes=nodes)
        views.append((i[0], c[0], 100 + v))
    enc = [m.encode(X, i, W, Ln, nodes, c, None, seed=s) for i, c, s in views]
    loss = pathnet_amd.contrastive_loss(enc[0].embedding, enc[1].embedding, temperature=0.5).loss
    m.zero_grad(set_to_none=True)
    pathnet_amd.backward(loss)
    got = {k: v.clone() for k, v in named_grads(m).items()}
    want_ref = ref.reference(enc[0].embedding.detach().cpu().numpy(), enc[1].embedding.detach().cpu().numpy(), 0.5, 1)
    want = None
    for (i, c, s), d in zip(views, (want_ref.dA, want_ref.dB)):
        m.zero_grad(set_to_none=True)
        e = m.encode(X, i, W, Ln, nodes, c, None, seed=s)
        e.embedding.backward(torch.from_numpy(d).float().cuda())
        g = {k: (v.grad.clone() if v.grad is not None else torch.zeros_like(v)) for k, v in m.named_parameters()}
        want = g if want is None else {k: want[k] + g[k] for k in g}
    unused = tuple(k for k, v in want.items() if not v.any())        # the classifier: the loss does not use the logits
    assert all(k.startswith("fc2") for k in unused), unused
    assert_grads_close(got, want, zero_ok=unused)


def hand_loop(m, head, smp, X, nodes, steps, seed, first, tau, intra, lr, L=L):
    import pathnet_amd
    from pathnet_amd.trainer import pretrain_seed
    params = list(m.parameters()) + (list(head.parameters()) if head is not None else [])
    opt = pathnet_amd.Adam(params, lr=lr)
    m.train()
    losses = []
    for t in range(steps):
        z = []
        for v in (0, 1):
            i, c = smp.sample(W, seed, epoch_begin=first + 2 * t + v, epoch_count=1, nodes=nodes)
            e = m.encode(X, i[0], W, L, nodes, c[0], None, seed=pretrain_seed(seed, t, v)).embedding
            z.append(head(e) if head is not None else e)
        c = pathnet_amd.contrastive_loss(z[0], z[1], temperature=tau, intra=intra)
        opt.zero_grad(set_to_none=True)
        pathnet_amd.backward(c.loss)
        opt.step()
        losses.append(c.loss.detach())
    return torch.stack(losses)


@pytest.mark.parametrize("name,with_head", (("PathNet_homo", False), ("PathNet_homo", True), ("PAGG", False)))
def test_pretrain_is_the_hand_written_loop(name, with_head):
    Ln = length_of(name)
    smp, X, _ = graph(Ln)
    nodes = all_nodes()
    a, b = model_of(name), model_of(name)
    ha, hb = (head_of(), head_of()) if with_head else (None, None)
    out = a.pretrain(X, smp, W, Ln, nodes, epochs=6, temperature=0.3, intra=True, head=ha, lr=1e-2, seed=5, first_epoch=3)
    want = hand_loop(b, hb, smp, X, nodes, 6, 5, 3, 0.3, True, 1e-2, L=Ln)
    assert out.loss.shape == (6,) and out.hits.dtype == torch.int64 and out.pairs.tolist() == [N] * 6
    assert torch.equal(out.loss, want)
    for (k, p), (_, q) in zip(a.named_parameters(), b.named_parameters()):
        assert torch.equal(p, q), k
    if with_head:
        for p, q in zip(ha.parameters(), hb.parameters()):
            assert torch.equal(p, q)
    assert a.training        # the mode it was in


def test_pretrain_hetero_biased_sampler_presampled_tensors_and_batches():
    smp, X, _ = graph()
    nodes = all_nodes()
    m = model_of("PathNet")
    before = copy.deepcopy(m.state_dict())
    out = m.pretrain(X, smp, W, L, nodes, epochs=2, lr=1e-2)
    assert torch.isfinite(out.loss).all() and out.loss.numel() == 2
    assert any(not torch.equal(v, before[k]) for k, v in m.state_dict().items())
    # a biased view of the sampler
    out = model_of("PathNet_homo").pretrain(X, smp.biased(2, 0.5), W, L, nodes, epochs=2)
    assert torch.isfinite(out.loss).all() and (out.pairs == N).all()
    # pre-sampled tensors hold the sampler's own draws: the same run
    ids, codes = smp.sample(W, 9, epoch_begin=0, epoch_count=4)
    a, b = model_of("PathNet_homo"), model_of("PathNet_homo")
    x = a.pretrain(X, (ids, codes), W, L, nodes, epochs=2, seed=9, intra=False)
    y = b.pretrain(X, smp, W, L, nodes, epochs=2, seed=9, intra=False)
    assert torch.equal(x.loss, y.loss) and torch.equal(x.hits, y.hits)
    # node batches: 96 nodes in batches of 40 are 3 steps an epoch
    out = model_of("PAGG").pretrain(X, graph(4)[0], W, 4, None, epochs=2, batch_nodes=40)
    assert out.loss.numel() == 6 and out.pairs.tolist() == [40, 40, 16] * 2


@pytest.mark.parametrize("seed", (0, 1, 2))
def test_pretraining_learns_on_the_planted_graph(seed):
    """40 steps at lr = 1e-2: the loss falls and the partner is found more often.
    With feature noise of scale 1 every node is told from every other before the first step (hit rate 1.0 at step 0 at all
    three seeds), so the rate has nowhere to go; the features here are the block signal plus noise of scale 0.05, where an
    untrained model finds 47 .. 66 % of the partners and 40 steps bring that to 94 .. 98 % (loss 4.68 -> 3.53 .. 3.59).  lr
    and steps are the ones first tried."""
    smp, X, _ = graph(L, 0.05)
    m = model_of("PathNet_homo", seed=20 + seed)
    out = m.pretrain(X, smp, W, L, all_nodes(), epochs=40, lr=1e-2, seed=seed, temperature=0.5)
    loss = out.loss.double().cpu()
    rate = (out.hits.double() / (2 * out.pairs.double())).cpu()
    print("seed %d: loss %.4f -> %.4f, hit rate %.3f -> %.3f" % (seed, loss[:5].mean(), loss[-5:].mean(), rate[0], rate[-1]))
    assert loss[-5:].mean() < loss[:5].mean()
    assert rate[-1] > rate[0]


def test_no_host_sync_inside_the_loop():
    """the steps after the first (whose sampler calls check their status word) run with synchronising calls forbidden"""
    smp, X, _ = graph()
    m, nodes = model_of("PathNet_homo"), all_nodes()
    real = smp.sample
    calls = []

    def sample(*a, **kw):
        if not kw.get("check", True) and not calls:      # the first sampler call of step 1
            calls.append(1)
            torch.cuda.set_sync_debug_mode("error")
        return real(*a, **kw)

    smp.sample = sample
    try:
        out = m.pretrain(X, smp, W, L, nodes, epochs=4, lr=1e-2)
    finally:
        torch.cuda.set_sync_debug_mode("default")
        del smp.sample
    assert calls and torch.isfinite(out.loss).all()
