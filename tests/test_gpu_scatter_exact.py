"""The backward's scatter-adds held to EXACT counts at the chunk and run edges of det_scatter_kernel (pn_det.hip), on every
route a gradient can take to its row: the fp32 atomics of seq_reduce_kernel<true> and the pooling backward, the sorted
two-pass fixed-order scatter (det_keys3_kernel, the one rocPRIM sort, DET_ROW / DET_SEL / DET_EGO), either over compact rows
(mark_rows / scan_*, pn_plan.hip) and either per micro-batch.

The cases, their probe parameters and the reference are tests/scatter_probe.py's: sum / mean encoders over X = 0 whose every
backward quantity is a dyadic rational with a few significant bits, so that every fp32 sum is exact in any order
(tests/test_scatter_probe_host.py proves that, and that the reference is the fp64 oracle, per case on the CPU).  Each case
is a plain forward + backward in training mode, dropout 0, under G[s] = (C g_s, 0, ...); every compared tensor -- X.grad,
the distance layers' weights and biases, fc0.bias and, with attention, attw.weight / attw.bias -- must be torch.equal to the
integer reference, and the rows of X.grad nothing touches +0 bit for bit.  No tolerance: a dropped or doubled piece of a
crossing run, a middle chunk taken for a head, one lane group, a contribution on the neighbouring row all show, and the
failure names the row with the runs and chunks of its keys."""
import functools

import pytest
import torch

import scatter_probe as sp

pytestmark = pytest.mark.gpu

# route -> (deterministic, compact rows, micro-batches)
ROUTES = {
    "atomic": (False, False, False),
    "fixed-order": (True, False, False),
    "compact-atomic": (False, True, False),
    "compact-fixed-order": (True, True, False),
    "micro-atomic": (False, False, True),
    "micro-fixed-order": (True, False, True),
}
PARAMS = [pytest.param(c.id, r, id="%s-%s" % (c.id, r)) for c in sp.CASES for r, (_, _, micro) in ROUTES.items()
          if not micro or c.data["micro"]]        # (a batch of fewer than five masked nodes has no three unequal micro-batches)


@functools.lru_cache(maxsize=None)
def _reference(cid):
    """computed once per case, shared by its routes, never written to"""
    return sp.reference(sp.CASES[sp.CASE_IDS.index(cid)])


def _module(case):
    import pathnet_amd
    N = case.data["N"]
    if case.variant == "pagg":
        m = pathnet_amd.PAGG(case.H, case.H, case.C, N, dropout=0.0, cell=case.cell)
    else:
        cls = {"homo": pathnet_amd.PathNet_homo, "hetero": pathnet_amd.PathNet}[case.variant]
        m = cls(case.H, case.H, case.C, case.L, dropout=0.0, cell=case.cell)
    m = m.cuda().train()
    res = m.load_state_dict(sp.probe_params(case), strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    return m


def _budget(case, m, det):
    """the workspace budget at which the library cuts the batch into the case's micro-batches"""
    from pathnet_amd import modules as M
    d = case.data
    args = (case.variant, d["N"], case.H, case.H, case.C, d["S"], case.W, case.L)
    kw = dict(cell=m._cell_kind, deterministic=det)
    b = M.workspace_bytes(*args, batch_groups=d["micro"], **kw)
    assert M.pick_batch_groups(*args, b, **kw) == d["micro"]
    return b


@pytest.mark.parametrize("cid,route", PARAMS)
def test_scatter_adds_are_exact(cid, route, monkeypatch):
    from pathnet_amd import modules as M
    case = sp.CASES[sp.CASE_IDS.index(cid)]
    det, compact, micro = ROUTES[route]
    d = case.data
    want, _, touched = _reference(cid)
    monkeypatch.setenv("PN_COMPACT", "1" if compact else "0")
    m = _module(case)
    m.deterministic = det
    nb = 1
    if micro:
        assert d["micro"], "no micro-batches for this case"
        m.workspace_budget = _budget(case, m, det)
        nb = len(sp.micro_groups(d["S"], d["micro"]))
        assert nb >= 3 and d["S"] % d["micro"] != 0
    X = torch.zeros(d["N"], case.H, device="cuda", requires_grad=True)
    ids = torch.as_tensor(d["ids"], dtype=torch.int32).cuda()
    codes = torch.as_tensor(d["codes"], dtype=torch.uint8).cuda()
    sel = torch.as_tensor(d["sel"], dtype=torch.int32).cuda()
    out = m(X, ids, case.W, case.L, sel, codes, None)
    out.backward(d["G"].cuda())
    torch.cuda.synchronize()
    info = M.shape_info(m._last_shape[0])
    assert info[0] == compact, "route %s: the call ran %s rows" % (route, "compact" if info[0] else "dense")
    assert info[2] == nb, "route %s: %d micro-batches, %d expected" % (route, info[2], nb)
    got = {k: v.grad for k, v in m.named_parameters() if k in want}
    got["X"] = X.grad
    assert set(got) == set(want)
    msgs = sp.compare(case, got, want, touched)
    assert not msgs, "%s, %s (%s): %s" % (cid, route, case.why, " | ".join(msgs))
