"""model.embed() and model.knn_probe() on a small planted-partition graph built here (300 nodes in 2 blocks; W = 8, L = 4,
H = 32, F = 16): embed() against explicit eval-mode encode() calls, knn_probe() against knn_classify(knn(...)) on those
embeddings, both bit for bit; no query is its own neighbour; planted feature clusters are classified without an error."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

N, F, W, L, H, C = 300, 16, 8, 4, 32, 2
SEED = 11


@functools.lru_cache(None)
def graph():
    """-> (sampler, X on the GPU, block of every node): edges inside a block with probability 0.06, across with 0.004; the
    features are the block's signal in 4 of the 16 columns plus unit noise: two clusters far apart"""
    import pathnet_amd
    rng = np.random.default_rng(4)
    block = (np.arange(N) >= N // 2).astype(np.int64)
    prob = np.where(block[:, None] == block[None, :], 0.06, 0.004)
    adj = np.triu(rng.random((N, N)) < prob, 1)
    adj = adj | adj.T | np.eye(N, dtype=bool)
    src, dst = np.nonzero(adj)
    p = 1.0 / adj.sum(axis=1)[src]
    smp = pathnet_amd.MerwSampler(N, src.astype(np.int32), dst.astype(np.int32), p, L)
    X = torch.from_numpy((rng.standard_normal((N, F)) + 4.0 * (2 * block[:, None] - 1) * (np.arange(F) < 4)).astype(np.float32))
    return smp, X.cuda(), block


def model_of(name, seed=3):
    import pathnet_amd
    torch.manual_seed(seed)
    return getattr(pathnet_amd, name)(F, H, C, L).cuda()


def explicit(m, nodes32, samples, first_epoch, batch_nodes, head=None):
    """embed(), spelled out: one eval-mode encode() per chunk and draw, added in ascending draw order, divided once"""
    from pathnet_amd import DRAW_PHILOX
    smp, X, _ = graph()
    S = int(nodes32.numel())
    step = S if batch_nodes is None else batch_nodes
    m.eval()
    out = None
    with torch.no_grad():
        for j in range(samples):
            if m.variant == "hetero":       # one whole-batch draw, cut into group_slice pieces
                i, c = smp.sample(W, SEED, epoch_begin=first_epoch + j, epoch_count=1, draw_source=DRAW_PHILOX, nodes=nodes32)
                rows = torch.cat([m.encode(X, i[0], W, L, nodes32, c[0], None, group_slice=(b0, min(step, S - b0))).embedding
                                  for b0 in range(0, S, step)])
            else:
                rows = []
                for b0 in range(0, S, step):
                    sel = nodes32[b0:b0 + step]
                    i, c = smp.sample(W, SEED, epoch_begin=first_epoch + j, epoch_count=1, draw_source=DRAW_PHILOX, nodes=sel)
                    rows.append(m.encode(X, i[0], W, L, sel, c[0], None).embedding)
                rows = torch.cat(rows)
            if head is not None:
                rows = torch.cat([head(rows[b0:b0 + step]) for b0 in range(0, S, step)])
            out = rows.clone() if out is None else out + rows
    m.train()
    return out / samples if samples > 1 else out


@pytest.mark.parametrize("name,batch_nodes", [("PathNet_homo", None), ("PathNet_homo", 37), ("PAGG", None), ("PAGG", 37),
                                              ("PathNet", None)])
def test_embed_equals_explicit_encode_calls(name, batch_nodes):
    smp, X, _ = graph()
    m = model_of(name).train()
    nodes = torch.arange(N, dtype=torch.int32, device="cuda")[7:290:2].contiguous()
    got = m.embed(X, smp, W, L, nodes, samples=3, seed=SEED, first_epoch=5, batch_nodes=batch_nodes)
    assert m.training and got.shape == (len(nodes), 2 * H) and got.dtype == torch.float32 and not got.requires_grad
    want = explicit(m, nodes, 3, 5, batch_nodes)
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    one = m.embed(X, smp, W, L, nodes, seed=SEED, first_epoch=5, batch_nodes=batch_nodes)
    assert torch.equal(one.view(torch.int32), explicit(m, nodes, 1, 5, batch_nodes).view(torch.int32))
    if name == "PathNet_homo" and batch_nodes == 37:        # a head, a bool mask, and no node at all
        torch.manual_seed(8)
        head = torch.nn.Sequential(torch.nn.Linear(2 * H, 24), torch.nn.Dropout(0.5)).cuda().train()
        mask = torch.zeros(N, dtype=torch.bool)
        mask[nodes.long().cpu()] = True
        z = m.embed(X, smp, W, L, mask, samples=2, seed=SEED, batch_nodes=37, head=head)
        assert head.training and z.shape == (len(nodes), 24)
        head.eval()
        assert torch.equal(z, explicit(m, nodes, 2, 0, 37, head=head))
        assert m.embed(X, smp, W, L, nodes[:0], seed=SEED).shape == (0, 2 * H)


@pytest.mark.parametrize("name", ("PathNet_homo", "PAGG"))
def test_knn_probe_equals_the_composition(name):
    import pathnet_amd
    from pathnet_amd import neighbours as nb
    smp, X, block = graph()
    m = model_of(name)
    ids = torch.arange(N, dtype=torch.int32, device="cuda")
    bank, query = ids[:220].contiguous(), ids[180:].contiguous()          # 40 query nodes sit in the bank
    y = torch.from_numpy(block).cuda()
    y_bank = y.clone()
    y_bank[::9] = -1                                                       # unlabelled bank nodes
    kw = dict(samples=2, seed=SEED, first_epoch=3, batch_nodes=64)
    got = m.knn_probe(X, smp, W, L, bank, y_bank, query, y, k=10, temperature=0.07, **kw)
    zb, zq = m.embed(X, smp, W, L, bank, **kw), m.embed(X, smp, W, L, query, **kw)
    yb = y_bank[bank.long()]
    exclude = nb.exclude_of(query, bank, N)
    found = pathnet_amd.knn(zq, zb, 10, bank_valid=yb >= 0, exclude=exclude)
    want = pathnet_amd.knn_classify(found, yb, C, temperature=0.07, labels=y[query.long()])
    for a, b in zip(got, want):
        assert torch.equal(a, b)
    # a query node present in the bank never appears in its own list, and an unlabelled bank node in nobody's
    assert exclude[:40].tolist() == list(range(180, 220)) and (exclude[40:] == -1).all()
    assert not (found.index == exclude[:, None]).any() and (found.count == 10).all()
    assert (yb[found.index.reshape(-1)] >= 0).all()
    s = found.summary()
    assert s["dead_queries"] == 0 and s["dead_bank_rows"] == 0 and s["neighbours"] == 10 * len(query)
    # one embed() when the node lists coincide; labels per node of the list; the dot metric
    same = m.knn_probe(X, smp, W, L, bank, yb, bank, k=5, metric="dot", **kw)
    f2 = pathnet_amd.knn(zb, zb, 5, metric="dot", bank_valid=yb >= 0, exclude=torch.arange(220))
    assert same.confusion is None and torch.equal(same.prob, pathnet_amd.knn_classify(f2, yb, C).prob)


@pytest.mark.parametrize("name", ("PathNet_homo", "PAGG", "PathNet"))
def test_planted_clusters_are_classified_without_an_error(name):
    from pathnet_amd import trainer
    smp, X, block = graph()
    m = model_of(name)
    ids = torch.arange(N, dtype=torch.int32, device="cuda")
    train, test = ids[::2].contiguous(), ids[1::2].contiguous()
    vote = m.knn_probe(X, smp, W, L, train, block, test, block, k=20, seed=SEED)
    assert int(vote.confusion.sum()) == len(test) and int(vote.skipped) == 0
    assert trainer.metrics_from_confusion(vote.confusion)[1] == 1.0
    assert vote.prob.dtype == torch.float64 and torch.allclose(vote.prob.sum(1), torch.ones(len(test), dtype=torch.float64, device="cuda"))


def test_python_limits_are_named():
    import pathnet_amd
    q, x = torch.zeros((3, 4), device="cuda"), torch.ones((5, 4), device="cuda")
    for kw, word in ((dict(k=0), "k=0"), (dict(k=65), "k=65"), (dict(k=2, metric="l2"), "metric"), (dict(k=2, splits=0), "splits"),
                     (dict(k=2, splits=1025), "splits"), (dict(k=2, bank_valid=torch.ones(4)), "bank_valid"),
                     (dict(k=2, exclude=torch.zeros(2, dtype=torch.long)), "exclude")):
        with pytest.raises(ValueError, match=word):
            pathnet_amd.knn(q, x, **kw)
    with pytest.raises(ValueError, match="columns"):
        pathnet_amd.knn(q, torch.ones((5, 3), device="cuda"), 2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pathnet_amd.knn(q.cpu(), x.cpu(), 2)
    dead = pathnet_amd.knn(q, x, 2)             # zero rows: dead queries for the cosine
    assert dead.summary() == dict(queries=3, k=2, dead_queries=3, dead_bank_rows=0, neighbours=0, short_rows=3)
    found = pathnet_amd.knn(x[:2], x, 2, metric="dot")
    with pytest.raises(ValueError, match="num_classes"):
        pathnet_amd.knn_classify(found, torch.zeros(5, dtype=torch.long), 0)
    with pytest.raises(ValueError, match="temperature"):
        pathnet_amd.knn_classify(found, torch.zeros(5, dtype=torch.long), 2, temperature=0.0)
    vote = pathnet_amd.knn_classify(found, torch.tensor([0, 1, 1, 1, 1]), 2, temperature=float("inf"))
    assert vote.label.tolist() == [0, 0] and vote.prob.tolist() == [[0.5, 0.5], [0.5, 0.5]] and vote.confusion is None
