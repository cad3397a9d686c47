"""The row-reduction weight-gradient kernel of the node-level stage (g_bank_w = dZ'^T . Xh, g_fc0_w = dXh'^T . X with their
column sums: rgrad_kernel, rgrad_pays and launch_rgrad of pn_rgrad.hip, pad_rows_kernel of pn_plan.hip, run_bank_bwd /
run_fc0_bwd / xpad_floats of pn_pagg.hip) against the fp64 CPU oracle at its tile, split, tail and dispatch edges.

The rows, the edge classes they contain and the probes are those of tests/rgrad_cases.py (proven on the CPU by
tests/test_rgrad_cases_host.py: every class is in the table for the GATE and the no-GATE instantiation, the fp32 oracle passes
this file's own assertion at under 3 % of the bound, and one dropped, doubled or clamped edge row fails it thousands of times
over).  Every row runs in train mode with explicit dropout masks at keep 0.5, one forward and backward per probe through
the module, dense bank (PN_COMPACT=0), dense features (sparse_features "never"), deterministic off, default seq_math;
PN_NODE_RGRAD is what the row says: 2 forces the kernel below 2 048 rows, the default leaves the dispatch to rgrad_pays.

Upstream gradients: the dense random one -- every tensor is compared -- and, for the homo and PAGG plans, two one-group
probes whose paths are pinned to the reduction rows on an edge (node 0, 31 / 32, N - 1, the ragged tile's first and last
row, one node in a tile of every split).  The backward is linear in the upstream gradient: under a probe every other row of
dXh / dZ is exactly zero, so a row that is dropped, doubled, taken from the clamp or wrongly gated moves the result by the
order of 1 / (rows visited) of its maximum.  A probe compares the logits and the node-level tensors.

Bounds: logits within 1e-5, gradients by tests/gradcheck.py at its default 3e-5 of each tensor's largest element."""
import numpy as np
import pytest
import torch

import rgrad_cases as rc

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _restore_knobs():
    from pathnet_amd import _lib
    knobs = {k: _lib.get_knob(k) for k in ("PN_NODE_RGRAD",)}
    yield
    for k, v in knobs.items():
        _lib.set_knob(k, v)


def _module(c, params):
    import pathnet_amd
    if c.variant == "pagg":
        m = pathnet_amd.PAGG(c.F, c.H, rc.C, c.N, dropout=0.5, cell=c.cell)
    else:
        cls = {"homo": pathnet_amd.PathNet_homo, "hetero": pathnet_amd.PathNet}[c.variant]
        m = cls(c.F, c.H, rc.C, c.L, dropout=0.5, cell=c.cell)
    assert set(m.state_dict()) == set(params)
    m.load_state_dict(params)
    m = m.cuda().train()
    m.deterministic = False
    m.sparse_features = "never"
    return m


def _hip(m, c, d, dev, G):
    m._mask_seq, m._mask_cls = dev["mask_seq"], dev["mask_cls"]
    node_mask = np.zeros(c.N, bool)
    node_mask[d["sel"]] = True
    torch.manual_seed(7)
    m.zero_grad(set_to_none=True)
    out = m(dev["X"], dev["neis"], c.W, c.L, node_mask, dev["codes"], None)
    out.backward(G.cuda())
    torch.cuda.synchronize()
    return out.detach().cpu(), {k: v.grad.detach().cpu() for k, v in m.named_parameters()}


@pytest.mark.parametrize("cid", rc.CASE_IDS)
def test_node_level_weight_gradient_edges_match_the_fp64_oracle(cid, monkeypatch):
    from pathnet_amd import _lib, modules
    c = rc.CASES[rc.CASE_IDS.index(cid)]
    # the row is about the route the table says: the kernel for both tensors, but for the one row below the dispatch floor
    rt = rc.route(c.variant, c.N, c.F, c.H, c.L, c.knob, deterministic=False, compact=0)
    if c.N == 2047:
        assert rt == {"g_bank_w": "gemm", "g_fc0_w": "gemm"}
    else:
        assert rt["g_bank_w"] == "rgrad" and rt["g_fc0_w"] in ("rgrad", "rgrad+xpad"), rt
    want = rc.reference(cid)
    d = rc.make_inputs(c)
    monkeypatch.setenv("PN_COMPACT", "0")
    m = _module(c, rc.make_params(c))
    _lib.set_knob("PN_NODE_RGRAD", c.knob)
    monkeypatch.setattr(modules, "pick_batch_groups", lambda *a, **k: c.batch_groups)
    dev = dict(X=d["X"].cuda(), mask_seq=d["mask_seq"].cuda(), mask_cls=d["mask_cls"].cuda(),
               neis=torch.as_tensor(d["ids"].reshape(c.S, c.W * c.L).astype(np.int64)),
               codes=torch.as_tensor(d["codes"].astype(np.int64)))
    msgs = []
    for kind, group in rc.probes(c):
        out, g = _hip(m, c, d, dev, rc.upstream(c, d["G"], group))
        msgs += rc.check(c, kind, group, out, g, want[kind], "rgrad")
        # the call ran the dense bank over dense features in as many micro-batches as the row says
        compact, _, nb, _ = modules.shape_info(m._last_shape[0])
        assert not compact and nb == len(rc.micro_batches(c)) and m.fc0_route == "dense"
    assert _lib.get_knob("PN_NODE_RGRAD") == c.knob and not m._range_wide
    assert not msgs, "\n".join(msgs)
