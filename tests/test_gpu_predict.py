"""model.predict(): K path draws per node averaged on the device, against explicit forward() calls on the same draws fed
to the NumPy restatement of the ensemble (tests/ensemble_ref.py); the trainer's eval_samples.  The comparison rule and its
tolerance are tests/predict_cases.py's; the seed is checked on the CPU by tests/test_predict_seed_host.py."""
import functools

import numpy as np
import pytest
import torch

import ensemble_ref as ref
import predict_cases as pc

pytestmark = pytest.mark.gpu

W, L, C, K = pc.W, pc.L, pc.C, pc.K


@functools.lru_cache(None)
def sampler():
    import pathnet_amd
    n, u, v, p = pc.graph()
    return pathnet_amd.MerwSampler(n, u, v, p, L)


@functools.lru_cache(None)
def setup(variant, H):
    """-> (model on the GPU in eval mode, X, node ids int32 on the GPU); shared, never written to"""
    return pc.model(variant, H).cuda(), pc.features().cuda(), torch.from_numpy(pc.node_list()).cuda()


def draw(smp, nodes, k, seed=pc.SEED, first=pc.FIRST):
    i, c = smp.sample(W, seed, epoch_begin=first + k, epoch_count=1, nodes=nodes)
    return i[0], c[0]


def forwards(m, X, nodes, draws, **kw):
    """logits [K, S, C] (numpy) of explicit whole-list forward() calls, one per draw"""
    with torch.no_grad():
        return np.stack([m(X, i, W, L, nodes, c, None, **kw).cpu().numpy() for i, c in draws])


@functools.lru_cache(None)
def reference(variant, H):
    """the restatement's ensemble over K explicit forwards on draws FIRST + k: computed once per (class, hidden size)"""
    m, X, nodes = setup(variant, H)
    logits = forwards(m, X, nodes, [draw(sampler(), nodes, k) for k in range(K)])
    logits.setflags(write=False)
    return pc.ensemble_of(logits)[0], logits


@pytest.mark.parametrize("variant", ["hetero", "homo", "pagg"])
@pytest.mark.parametrize("H", [32, 100])
def test_one_sample_is_the_softmax_of_forward(variant, H):
    m, X, nodes = setup(variant, H)
    _, logits = reference(variant, H)
    pred = m.predict(X, sampler(), W, L, nodes, samples=1, seed=pc.SEED, first_epoch=pc.FIRST)
    x = logits[0].astype(np.float64)
    e = np.exp(x - x.max(axis=1, keepdims=True))
    want = (e / e.sum(axis=1, keepdims=True)).astype(np.float32)
    got = pred.prob.cpu().numpy()
    assert (np.abs(got.astype(np.float64) - want) <= ref.ulp32(want)).all()
    assert (pred.label.cpu().numpy() == logits[0].argmax(axis=1)).all()
    assert (pred.vote_label == pred.label).all() and (pred.count == 1).all() and (pred.bad == 0).all()
    assert (pred.agreement == 1).all() and (pred.mutual_info == 0).all()
    assert pred.confusion is None and pred.skipped is None
    # the paths the CPU restatement of the sampler walks for these nodes are the ones predict drew
    i, c = draw(sampler(), nodes, 0)
    ci, cc = pc.cpu_draw(0)
    assert (i.cpu().numpy() == ci).all() and (c.cpu().numpy() == cc).all()


@pytest.mark.parametrize("variant", ["homo", "pagg"])
@pytest.mark.parametrize("H", [32, 100])
@pytest.mark.parametrize("batch_nodes,per_call", [(None, None), (None, 1), (None, 2), (None, K), (17, 1), (17, 2), (17, K)])
def test_k_samples_chunked_and_stacked(variant, H, batch_nodes, per_call):
    m, X, nodes = setup(variant, H)
    want, _ = reference(variant, H)
    pred = m.predict(X, sampler(), W, L, nodes, samples=K, seed=pc.SEED, first_epoch=pc.FIRST, batch_nodes=batch_nodes,
                     samples_per_call=per_call)
    pc.same_prediction(pred, want, "%s H=%d batch_nodes=%s samples_per_call=%s" % (variant, H, batch_nodes, per_call))
    assert (pred.count == K).all() and (pred.bad == 0).all()


@pytest.mark.parametrize("H", [32, 100])
def test_hetero_is_the_whole_batch_forward_averaged(H):
    m, X, nodes = setup("hetero", H)
    want, _ = reference("hetero", H)
    whole = m.predict(X, sampler(), W, L, nodes, samples=K, seed=pc.SEED, first_epoch=pc.FIRST)
    pc.same_prediction(whole, want, "hetero H=%d" % H)
    # chunks are group_slice pieces of the same whole-batch forward; samples_per_call is ignored (never stacked)
    for kw in (dict(batch_nodes=17), dict(batch_nodes=17, samples_per_call=K), dict(samples_per_call=2)):
        part = m.predict(X, sampler(), W, L, nodes, samples=K, seed=pc.SEED, first_epoch=pc.FIRST, **kw)
        pc.same_prediction(part, want, "hetero H=%d %s" % (H, kw))
        assert (part.label == whole.label).all() or pc.inside_margin(want.prob).any()
        assert (part.count == K).all()
    # a row of the hetero class depends on its batch: another node list gives other probabilities for the same node
    other = m.predict(X, sampler(), W, L, nodes[:30], samples=K, seed=pc.SEED, first_epoch=pc.FIRST)
    assert (other.prob - whole.prob[:30]).abs().max().item() > 10 * pc.TOL_P


def test_presampled_tensors_masks_and_defaults():
    """(ids, codes) [E, N, W, L]: sample k is epoch (first_epoch + k) % E; nodes as a bool mask; nodes=None is every node"""
    m, X, _ = setup("homo", 32)
    rng = np.random.default_rng(12)
    N, E = pc.N, 3
    ids = rng.integers(0, N, (E, N, W, L))
    ids[:, :, :, 0] = np.arange(N)[None, :, None]
    codes = np.minimum(rng.integers(0, L, (E, N, W, L)), np.arange(L))
    paths = (torch.as_tensor(ids, dtype=torch.int32), torch.as_tensor(codes, dtype=torch.uint8))
    mask = np.zeros(N, bool)
    mask[rng.permutation(N)[:50]] = True
    sel = torch.from_numpy(np.flatnonzero(mask).astype(np.int32)).cuda()
    epochs = [(2 + k) % E for k in range(K)]
    draws = [(paths[0][e].cuda()[sel.long()], paths[1][e].cuda()[sel.long()]) for e in epochs]
    want, _ = pc.ensemble_of(forwards(m, X, sel, draws))
    for nodes in (mask, torch.from_numpy(mask), sel):
        pred = m.predict(X, paths, W, L, nodes, samples=K, first_epoch=2)
        pc.same_prediction(pred, want, "tensors")
    everyone = m.predict(X, paths, W, L, samples=2, first_epoch=1)
    assert everyone.prob.shape == (N, C) and (everyone.count == 2).all()
    picked = m.predict(X, paths, W, L, sel, samples=2, first_epoch=1)
    assert (everyone.prob[sel.long()] - picked.prob).abs().max().item() <= 2 * pc.TOL_P
    with pytest.raises(ValueError):
        m.predict(X, (paths[0][:, :5], paths[1][:, :5]), W, L, samples=2)
    with pytest.raises(ValueError):
        m.predict(X, paths, W, L, samples=0)


def test_continuing_an_ensemble():
    import pathnet_amd
    m, X, nodes = setup("homo", 32)
    smp = sampler()
    both = m.predict(X, smp, W, L, nodes, samples=2 * K, seed=pc.SEED, samples_per_call=1)
    ens = pathnet_amd.Ensemble(nodes.numel(), C, "cuda")
    first = m.predict(X, smp, W, L, nodes, samples=K, seed=pc.SEED, samples_per_call=1, ensemble=ens)
    assert (first.count == K).all()
    more = m.predict(X, smp, W, L, nodes, samples=K, seed=pc.SEED, first_epoch=K, samples_per_call=1, ensemble=ens)
    assert (more.count == 2 * K).all()
    # the same forwards in the same order: the same bits
    for f in ("prob", "label", "vote_label", "confidence", "entropy", "mutual_info", "agreement"):
        assert torch.equal(getattr(more, f), getattr(both, f)), f
    # ... and against 2K explicit forwards
    want, _ = pc.ensemble_of(forwards(m, X, nodes, [draw(smp, nodes, k, first=0) for k in range(2 * K)]))
    pc.same_prediction(more, want, "K then K more")
    with pytest.raises(ValueError):
        m.predict(X, smp, W, L, nodes[:10], samples=1, ensemble=ens)


def test_labels_give_the_confusion_matrix_and_summary():
    from pathnet_amd import trainer
    m, X, nodes = setup("pagg", 32)
    Y = torch.from_numpy(np.random.default_rng(3).integers(0, C, pc.N)).cuda()
    Y[nodes[:4].long()] = -1                                    # unlabelled nodes: skipped, not counted
    pred = m.predict(X, sampler(), W, L, nodes, samples=K, seed=pc.SEED, first_epoch=pc.FIRST, labels=Y)
    y = Y[nodes.long()]
    keep = y >= 0
    conf = torch.bincount(y[keep] * C + pred.label[keep], minlength=C * C).view(C, C)
    assert torch.equal(pred.confusion, conf) and pred.skipped.tolist() == [4, 0]
    want = trainer.classification_metrics(y[keep], pred.label[keep], C)
    assert trainer.metrics_from_confusion(pred.confusion) == want
    s = pred.summary()
    assert (s["macro_f1"], s["micro_f1"], s["macro_recall"], s["macro_precision"], s["accuracy"]) == pytest.approx(want, abs=1e-12)
    assert s["rows"] == pc.S and s["labels_out_of_range"] == 4 and s["unlabelled_rows"] == 0 and s["bad_share"] == 0.0
    assert s["mean_agreement"] == pytest.approx(float(pred.agreement.double().mean()))
    per_row = m.predict(X, sampler(), W, L, nodes, samples=K, seed=pc.SEED, first_epoch=pc.FIRST, labels=y)     # labels per row
    assert torch.equal(per_row.confusion, conf)


def test_path_weights_are_passed_through():
    m, X, nodes = setup("homo", 32)
    smp = sampler()
    seen = []

    def drop_first(ids, codes, nodes32, k):
        seen.append((tuple(ids.shape), tuple(codes.shape), int(nodes32.numel()), k))
        w = torch.ones(ids.shape[:2], device=ids.device)
        w[:, 0] = 0.0
        return w
    draws = [draw(smp, nodes, k) for k in range(K)]
    w = torch.ones(nodes.numel(), W, device="cuda")
    w[:, 0] = 0.0
    want, _ = pc.ensemble_of(forwards(m, X, nodes, draws, path_weights=w))
    plain, _ = reference("homo", 32)
    assert np.abs(want.prob - plain.prob).max() > 10 * pc.TOL_P           # the weights matter
    for per_call in (1, 2):
        seen.clear()
        pred = m.predict(X, smp, W, L, nodes, samples=K, seed=pc.SEED, first_epoch=pc.FIRST, samples_per_call=per_call,
                         path_weights=drop_first)
        pc.same_prediction(pred, want, "path_weights, samples_per_call=%d" % per_call)
        assert sorted(s[3] for s in seen) == list(range(K)) and all(s[0] == (pc.S, W, L) == s[1] for s in seen)
    none = m.predict(X, smp, W, L, nodes, samples=K, seed=pc.SEED, first_epoch=pc.FIRST, path_weights=lambda *a: None)
    pc.same_prediction(none, plain, "path_weights -> None")


def test_biased_sampler_and_module_state():
    m, X, nodes = setup("homo", 100)
    view = sampler().biased(2.0, 0.5)
    want, _ = pc.ensemble_of(forwards(m, X, nodes, [draw(view, nodes, k) for k in range(K)]))
    pred = m.predict(X, view, W, L, nodes, samples=K, seed=pc.SEED, first_epoch=pc.FIRST)
    pc.same_prediction(pred, want, "biased sampler")
    # a module in training mode: predict runs it in eval (no dropout: the values are the eval forward's), restores the flag
    # and draws nothing from torch's generators
    import pathnet_amd
    torch.manual_seed(pc.MODEL_SEED)
    t = pathnet_amd.PathNet_homo(pc.F, 100, C, L, dropout=0.5).cuda()
    t.load_state_dict(m.state_dict())
    t.train()
    cpu_state, gpu_state = torch.get_rng_state(), torch.cuda.get_rng_state()
    again = t.predict(X, view, W, L, nodes, samples=K, seed=pc.SEED, first_epoch=pc.FIRST)
    assert t.training and t.dropout_p() == 0.5
    assert torch.equal(torch.get_rng_state(), cpu_state) and torch.equal(torch.cuda.get_rng_state(), gpu_state)
    pc.same_prediction(again, want, "module in training mode")
    assert not m.training
    with torch.enable_grad():
        t.predict(X, view, W, L, nodes, samples=1)
    assert all(p.grad is None for p in t.parameters())


def _toy(rng, n=90):
    Y = rng.integers(0, C, n)
    X = rng.random((n, pc.F)).astype(np.float32) * 0.5
    X[np.arange(n), Y] += 1.5                              # learnable from the ego features
    return torch.as_tensor(X), torch.as_tensor(Y), np.arange(0, 40), np.arange(40, 62), np.arange(62, n)


@pytest.mark.parametrize("source", ["sampler", "tensors"])
def test_trainer_eval_samples_one_is_the_loop_as_it_is(tmp_path, source):
    import pathnet_amd
    from pathnet_amd import trainer
    X, Y, tr, va, te = _toy(np.random.default_rng(31))
    if source == "sampler":
        from test_gpu_sampler import synthetic_graph
        paths = pathnet_amd.MerwSampler(*synthetic_graph(90, 4, 3), L)
    else:
        i, c = sampler().sample(W, 1, epoch_count=3)
        paths = (i[:, :90] % 90, c[:, :90])

    def run(tag, **kw):
        torch.manual_seed(19)
        m = pathnet_amd.PathNet_homo(pc.F, 32, C, L, dropout=0.4).cuda()
        m.deterministic = True
        res = trainer.train_fixed_indices(X, Y, C, "cora", tr, va, te, W, 32, L, paths, epochs=3, save_dir=str(tmp_path / tag),
                                          model=m, **kw)
        return res, {k: v.detach().clone() for k, v in m.state_dict().items()}
    base, sd0 = run("base")
    res, sd = run("one", eval_samples=1)
    assert res == base
    for k in sd0:
        assert torch.equal(sd[k], sd0[k]), k
    with pytest.raises(ValueError):
        run("zero", eval_samples=0)


@pytest.mark.parametrize("source", ["sampler", "tensors"])
def test_trainer_eval_samples_four(tmp_path, monkeypatch, source):
    import pathnet_amd
    from pathnet_amd import trainer
    X, Y, tr, va, te = _toy(np.random.default_rng(32))
    epochs, KS = 3, 4
    calls = []
    if source == "sampler":
        from test_gpu_sampler import synthetic_graph
        smp = pathnet_amd.MerwSampler(*synthetic_graph(90, 4, 3), L)

        class Spy:      # the sampler, noting which epochs are drawn for how many nodes
            def sample(self, *a, **kw):
                calls.append((int(kw["epoch_begin"]), int(kw["nodes"].numel())))
                return smp.sample(*a, **kw)
        paths = Spy()
    else:
        i, c = sampler().sample(W, 1, epoch_count=3)
        paths = (i[:, :90] % 90, c[:, :90])
    seen = []
    real = trainer.metrics_from_confusion
    monkeypatch.setattr(trainer, "metrics_from_confusion", lambda conf: seen.append(conf.clone()) or real(conf))
    torch.manual_seed(23)
    res = trainer.train_fixed_indices(X, Y, C, "cora", tr, va, te, W, 32, L, paths, epochs=epochs, dropout=0.2,
                                      save_dir=str(tmp_path), eval_samples=KS)
    assert len(res) == 5 and all(np.isfinite(r) and 0.0 <= r <= 1.0 for r in res)
    assert seen, "no epoch was selected"
    conf = seen[-1].double()                        # the test confusion matrix of the last selected epoch
    assert int(conf.sum()) == len(te)
    assert res[4] == float(conf.diag().sum() / conf.sum()) and res[1] == res[4]
    if source == "sampler":
        train_epochs = [e for e, n in calls if n == len(tr)]
        assert train_epochs == list(range(epochs))
        val = [e for e, n in calls if n == len(va)]
        want = [e if k == 0 else epochs + e * (KS - 1) + (k - 1) for e in range(epochs) for k in range(KS)]
        assert val == want
        assert not set(x for x in val if x >= epochs) & set(train_epochs)
