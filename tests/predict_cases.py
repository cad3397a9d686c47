"""The small problem tests/test_gpu_predict.py runs model.predict() on, shared with the CPU check of its seed
(tests/test_predict_seed_host.py): a random graph, a model per (class, hidden size), the Philox draws of the sampler as the
CPU restatement walks them, and the rule by which two ensembles are compared.

Tolerance.  Two evaluations of the same forward agree within TOL_OUT = 1e-5 on the logits (the suite's bound, tests/
test_gpu_pagg.py).  A perturbation d of the logits with |d_c| <= delta moves a softmax by p'_c / p_c = exp(d_c) / sum_j p_j
exp(d_j), which lies in [exp(-2 delta), exp(2 delta)]: |p'_c - p_c| <= (exp(2 delta) - 1) p_c <= 2.0001e-5.  The mean over the
samples obeys the same bound, and the fp32 rounding of the result adds half an ulp of a number below 1: TOL_P below.
A label is held equal where the top-two margin of the reference's mean probabilities exceeds 2 TOL_P (either side may move
by TOL_P); rows inside that margin are counted, and must be under 5 % of the rows on the seed chosen here.
"""
import numpy as np
import torch

import ensemble_ref as ref

TOL_LOGIT = 1e-5                                    # = TOL_OUT of tests/test_gpu_pagg.py
TOL_P = float(np.expm1(2 * TOL_LOGIT)) + 2.0 ** -24
N, F, C, W, L, S, K = 120, 16, 5, 9, 4, 61, 5
SEED, FIRST = 7, 3                                  # the sampler's seed and predict's first_epoch
MODEL_SEED = 90
CLASSES = {"hetero": "PathNet", "homo": "PathNet_homo", "pagg": "PAGG"}


def graph():
    from test_gpu_sampler import synthetic_graph
    return synthetic_graph(N, 4, 2)


def model(variant, H, cell=None):
    """on the CPU; the caller moves it"""
    import pathnet_amd
    torch.manual_seed(MODEL_SEED)
    cls = getattr(pathnet_amd, CLASSES[variant])
    m = cls(F, H, C, L if variant != "pagg" else N, cell=cell)
    with torch.no_grad():
        for k, v in m.named_parameters():
            if k.endswith("bias") or "bias_" in k:
                v.uniform_(-0.3, 0.3)
            if k.startswith("fc2.weight"):
                v.mul_(3.0)                          # logits of order one: margins far above the tolerance
    return m.eval()


def features():
    return torch.rand(N, F, generator=torch.Generator().manual_seed(5))


def node_list():
    """S node ids, not sorted: predict keeps the caller's order"""
    return np.random.default_rng(6).permutation(N)[:S].astype(np.int32)


def cpu_draw(k, seed=SEED, first=FIRST):
    """(ids, codes) [S, W, L] of sample k for node_list(), walked by the CPU restatement of the sampler"""
    from oracle import merw
    n, u, v, p = graph()
    ids, codes = merw.sample_full(n, u, v, p, W, L, merw.DRAW_PHILOX, seed, epoch_begin=first + k, epoch_count=1)
    sel = node_list().astype(np.int64)
    return ids[0][sel], codes[0][sel]


def oracle_logits(variant, m, X, ids, codes, sel, cell=None):
    from oracle import pagg_oracle as po
    params = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    with torch.no_grad():
        return po.forward(variant, params, X.cpu(), ids, codes, np.asarray(sel), W, L, cell=cell).numpy()


def ensemble_of(logits):
    """[K, S, C] logits -> (restatement's Result, its state)"""
    x = np.asarray(logits, np.float32)
    st = ref.new_state(x.shape[1], x.shape[2])
    ref.add(st, x)
    return ref.finish(st), st


def inside_margin(prob):
    top = np.sort(np.asarray(prob, np.float64), axis=1)[:, -2:]
    return (top[:, 1] - top[:, 0]) <= 2 * TOL_P


def same_prediction(got, want, what=""):
    """got: a Prediction (device tensors) or a Result; want: a Result.  -> rows inside the margin"""
    g = (lambda t: t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t))       # noqa: E731
    err = np.abs(g(got.prob).astype(np.float64) - want.prob.astype(np.float64)).max()
    assert err <= TOL_P, "%s: probabilities differ by %g (bound %g)" % (what, err, TOL_P)
    close = inside_margin(want.prob)
    print("%s: max |dp| = %.3g, %d of %d rows inside the label margin" % (what, err, close.sum(), len(close)))
    assert close.mean() < 0.05, "%s: %d of %d rows inside the margin" % (what, close.sum(), len(close))
    assert (g(got.label)[~close] == want.label[~close]).all(), what
    for k, tol in (("confidence", TOL_P), ("entropy", None), ("mutual_info", None)):
        a, b = g(getattr(got, k)).astype(np.float64), getattr(want, k).astype(np.float64)
        if tol is None:
            # |d (p log p)| <= |log p + 1| |dp|; with |dp| <= TOL_P p (the bound above is relative) the C terms sum to at
            # most TOL_P (H + 1), for the entropy and for each sample's entropy alike
            tol = 2 * TOL_P * (np.log(C) + 1)
        assert np.abs(a - b).max() <= tol, (what, k, np.abs(a - b).max())
    return close
