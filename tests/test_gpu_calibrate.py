"""model.calibrate(), predict(temperature=) and Prediction.calibration() end to end on a small graph, for the class whose rows
stand alone (PathNet_homo) and the one whose rows read their batch (PathNet).

Tolerance of a probability: two evaluations of the same forward agree within predict_cases.TOL_LOGIT on the logits; divided
by tau that is a perturbation of TOL_LOGIT / tau of the softmax's argument, which moves a probability by at most
expm1(2 TOL_LOGIT / tau) (predict_cases' derivation), plus half an fp32 ulp of a number below 1.
"""
import copy
import functools

import numpy as np
import pytest
import torch

import calib_ref as ref
import predict_cases as pc

pytestmark = pytest.mark.gpu

N, F, W, L, H, C, K, S = 60, 16, 4, 3, 32, 5, 3, 37
SEED, FIRST = 11, 2
CLASSES = {"homo": "PathNet_homo", "hetero": "PathNet"}
VARIANTS = tuple(CLASSES)


@functools.lru_cache(None)
def sampler():
    import pathnet_amd
    from test_gpu_sampler import synthetic_graph
    n, u, v, p = synthetic_graph(N, 4, 2)
    return pathnet_amd.MerwSampler(n, u, v, p, L)


@functools.lru_cache(None)
def setup(variant):
    """-> (model in eval mode, X, node ids, labels of those nodes), all on the GPU; shared, never written to"""
    import pathnet_amd
    torch.manual_seed(17)
    m = getattr(pathnet_amd, CLASSES[variant])(F, H, C, L)
    with torch.no_grad():
        for k, v in m.named_parameters():
            if k.startswith("fc2.weight"):
                v.mul_(3.0)
    m = m.cuda().eval()
    X = torch.rand(N, F, generator=torch.Generator().manual_seed(5)).cuda()
    nodes = torch.from_numpy(np.random.default_rng(6).permutation(N)[:S].astype(np.int32)).cuda()
    logits = explicit_logits(m, X, nodes)
    y = logits.mean(dim=0).argmax(dim=1)
    y[::3] = (y[::3] + 1) % C               # a third of the labels are wrong: the fitted temperature is finite
    return m, X, nodes, y


def explicit_logits(m, X, nodes):
    """[K, S, C] on the device: one whole-list forward per draw FIRST + k"""
    out = []
    with torch.no_grad():
        for k in range(K):
            i, c = sampler().sample(W, SEED, epoch_begin=FIRST + k, epoch_count=1, nodes=nodes)
            out.append(m(X, i[0], W, L, nodes, c[0], None).float())
    return torch.stack(out)


def tripled(m):
    m3 = copy.deepcopy(m)
    with torch.no_grad():
        for k, v in m3.named_parameters():
            if k.startswith("fc2."):
                v.mul_(3.0)
    return m3


@pytest.mark.parametrize("variant", VARIANTS)
def test_calibrate_is_fit_temperature_on_the_same_draws(variant):
    import pathnet_amd
    m, X, nodes, y = setup(variant)
    got = m.calibrate(X, sampler(), W, L, nodes, y, samples=K, seed=SEED, first_epoch=FIRST)
    want = pathnet_amd.fit_temperature(explicit_logits(m, X, nodes), y)
    assert torch.equal(got.temps, want.temps) and got.temps.numel() == 17
    assert int(got.best) == int(want.best) >= 0 and float(got.tau) == float(want.tau) == float(got.temps[int(got.best)])
    assert got.counts.tolist() == [S, 0, 0]
    s = got.summary()
    assert s["tau"] == float(got.tau) and s["rows_used"] == S and 0 < s["mean_nll"] < np.log(C) + 1
    # labels of all N nodes are picked by the node list
    full = torch.full((N,), -1, dtype=torch.int64, device="cuda")
    full[nodes.long()] = y
    again = m.calibrate(X, sampler(), W, L, nodes, full, samples=K, seed=SEED, first_epoch=FIRST)
    assert torch.equal(again.nll, got.nll) and torch.equal(again.tau, got.tau)
    with pytest.raises(ValueError, match="fewer nodes"):
        m.calibrate(X, sampler(), W, L, nodes, y, samples=K, seed=SEED, max_bytes=4 * K * S * C - 1)


@pytest.mark.parametrize("variant", VARIANTS)
def test_predict_with_a_temperature_is_the_scaled_ensemble(variant):
    import pathnet_amd
    m, X, nodes, y = setup(variant)
    fit = m.calibrate(X, sampler(), W, L, nodes, y, samples=K, seed=SEED, first_epoch=FIRST)
    before = m.predict(X, sampler(), W, L, nodes, samples=K, seed=SEED, first_epoch=FIRST)
    pred = m.predict(X, sampler(), W, L, nodes, samples=K, seed=SEED, first_epoch=FIRST, temperature=fit.tau, labels=y)
    ens = pathnet_amd.Ensemble(S, C, "cuda", temperature=fit.tau).add(explicit_logits(m, X, nodes))
    want = ens.result(labels=y)
    tau = float(fit.tau)
    tol = float(np.expm1(2 * pc.TOL_LOGIT / tau)) + 2.0 ** -24
    err = (pred.prob.double() - want.prob.double()).abs().max().item()
    assert err <= tol, "probabilities differ by %g (bound %g)" % (err, tol)
    assert (pred.count == K).all() and (pred.vote_label == want.vote_label).all()
    assert tau != 1.0 and (pred.prob - before.prob).abs().max().item() > 100 * tol       # the temperature did something
    assert (pred.vote_label == before.vote_label).all()                                   # ... but not to the votes
    # a float temperature is the same call
    same = m.predict(X, sampler(), W, L, nodes, samples=K, seed=SEED, first_epoch=FIRST, temperature=tau)
    assert torch.equal(same.prob, pred.prob)
    with pytest.raises(ValueError):
        m.predict(X, sampler(), W, L, nodes, samples=K, temperature=tau, ensemble=pathnet_amd.Ensemble(S, C, "cuda"))


@pytest.mark.parametrize("variant", VARIANTS)
def test_predict_without_the_keyword_does_not_change(variant):
    m, X, nodes, y = setup(variant)
    kw = dict(samples=K, seed=SEED, first_epoch=FIRST)
    before = m.predict(X, sampler(), W, L, nodes, labels=y, **kw)
    m.calibrate(X, sampler(), W, L, nodes, y, **kw)
    after = m.predict(X, sampler(), W, L, nodes, labels=y, **kw)
    for f in before._fields:
        assert torch.equal(getattr(before, f), getattr(after, f)), f
    assert not m.training


@pytest.mark.parametrize("variant", VARIANTS)
def test_logits_three_times_as_large_fit_three_times_the_temperature(variant):
    m, X, nodes, y = setup(variant)
    grid = ref.DEFAULT_GRID
    kw = dict(samples=K, seed=SEED, first_epoch=FIRST, rounds=1)
    one = m.calibrate(X, sampler(), W, L, nodes, y, grid=grid, **kw)
    three = tripled(m).calibrate(X, sampler(), W, L, nodes, y, grid=3.0 * grid, **kw)
    b = int(one.best)
    assert 0 < b < len(grid) - 1, "the fitted temperature sits at the end of the grid"
    assert int(three.best) == b and float(one.tau) == grid[b] and float(three.tau) == 3.0 * grid[b]
    unit = list(grid).index(1.0)
    assert float(one.nll[b]) <= float(one.nll[unit])
    assert np.allclose(three.nll.cpu().numpy(), one.nll.cpu().numpy(), rtol=1e-4)


@pytest.mark.parametrize("variant", VARIANTS)
def test_calibration_summary_agrees_with_the_restatement(variant):
    m, X, nodes, y = setup(variant)
    pred = m.predict(X, sampler(), W, L, nodes, samples=K, seed=SEED, first_epoch=FIRST)
    labels = y.clone()
    labels[5] = -1                          # out of range: counted, not used
    cal = pred.calibration(labels)
    s = cal.summary()
    conf, label, prob = (t.cpu().numpy() for t in (pred.confidence, pred.label, pred.prob))
    hi = ref.stats(conf, label, labels.cpu().numpy(), prob, C, 15, np.longdouble)
    m_used = int(hi.counts[0])
    assert s["used"] == m_used == S - 1 and s["labels_out_of_range"] == 1 and s["rows"] == S
    assert s["bin_count"] == hi.bin_count.tolist()
    assert (cal.bin_correct.cpu().numpy() == hi.bin_correct).all() and (cal.bin_conf.cpu().numpy() == hi.bin_conf).all()
    assert (cal.order.cpu().numpy() == hi.order).all() and (cal.err_prefix.cpu().numpy() == hi.err_prefix).all()
    ece, mce = ref.ece_mce(hi.bin_count, hi.bin_correct, hi.bin_conf)
    # (a handful of fp64 operations on exact integers, in torch and in NumPy)
    assert s["ece"] == pytest.approx(ece, rel=1e-12, abs=1e-15) and s["mce"] == pytest.approx(mce, rel=1e-12, abs=1e-15)
    rows = m_used - int(hi.counts[4])
    assert abs(s["nll"] * rows - float(hi.sums[0])) <= 2 * ref.tol_stats_nll(hi.sums[0], S)
    assert abs(s["brier"] * m_used - float(hi.sums[1])) <= 2 * ref.tol_stats_brier(hi.sums[1], S, C)
    assert abs(s["aurc"] - float(hi.aurc)) <= ref.tol_aurc(hi.aurc, m_used)
    assert float(cal.threshold(1.0)) == conf[hi.order[m_used - 1]] and float(cal.threshold(0.25)) >= float(cal.threshold(0.5))
