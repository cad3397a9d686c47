"""The recurrent weight-gradient GEMMs ([g_W_ih | g_W_hh] = dG^T . [x | h], g_b = colsum(dG): wgradh_kernel of pn_seqh.hip,
wgrad4_kernel of pn_seq4.hip, wgrad3_kernel and wgrad_reduce_kernel of pn_seq3.hip, the split arithmetic of ws_layout /
run_wgrad in pn_pagg.hip) against the fp64 CPU oracle at their tile, split and tail edges.

The rows, the edge classes they contain and the probes are those of tests/wgrad_cases.py (proven on the CPU by
tests/test_wgrad_cases_host.py: every class is in the table for every kernel, and the fp32 oracle passes this file's own
assertion at about 1 % of the bound).  Every row runs in train mode with explicit dropout masks at keep 0.5, one forward and
backward through the module, under each arithmetic that reaches another kernel:

  seq_math "f16x2"                 wgradh_kernel (H <= 256)
  seq_math "bf16x3"                wgrad4_kernel at H = 128 with four gate slots, wgrad3_kernel elsewhere
  seq_math "bf16x3", PN_SEQ4 = 0   wgrad3_kernel at H = 128 as well
  H = 288                          the generic route: wgrad3_kernel whatever the arithmetic (run once)

Upstream gradients: the dense random one -- every tensor is compared -- and, for the homo and PAGG plans, one-group probes:
group 0, the last group, the last group of the first micro-batch, and the group that straddles the boundary between the last
whole K tile and the ragged one.  The backward is linear in the upstream gradient: under a probe every row of dG outside the
group's W L rows is exactly zero, the recurrent gradients are sums over W L rows that sit on the chosen edge, and a dropped,
doubled or misplaced row moves them by the order of 1 / (W L) of their maximum.  A probe compares the logits and the four
recurrent tensors.  (It also lowers the launch-wide max |dG| that wgradh scales by: the scale must follow the data.)

Bounds: logits within 1e-5, gradients by tests/gradcheck.py at its default 3e-5 of each tensor's largest element."""
import pytest
import torch

import wgrad_cases as wc

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _restore_knobs():
    from pathnet_amd import _lib
    knobs = {k: _lib.get_knob(k) for k in ("PN_SEQ4",)}
    yield
    for k, v in knobs.items():
        _lib.set_knob(k, v)


def _module(c, params, seq_math):
    import pathnet_amd
    if c.variant == "pagg":
        m = pathnet_amd.PAGG(wc.F, c.H, wc.C, wc.N, dropout=0.5, cell=c.cell)
    else:
        cls = {"homo": pathnet_amd.PathNet_homo, "hetero": pathnet_amd.PathNet}[c.variant]
        m = cls(wc.F, c.H, wc.C, c.L, dropout=0.5, cell=c.cell)
    assert set(m.state_dict()) == set(params)
    m.load_state_dict(params)
    m = m.cuda().train()
    m.seq_math = seq_math
    return m


def _hip(m, c, d, dev, G):
    import numpy as np
    m._mask_seq, m._mask_cls = dev["mask_seq"], dev["mask_cls"]
    node_mask = np.zeros(wc.N, bool)
    node_mask[d["sel"]] = True
    torch.manual_seed(7)
    m.zero_grad(set_to_none=True)
    out = m(dev["X"], dev["neis"], c.W, c.L, node_mask, dev["codes"], None)
    out.backward(G.cuda())
    torch.cuda.synchronize()
    return out.detach().cpu(), {k: v.grad.detach().cpu() for k, v in m.named_parameters()}


RUNS = [(cid, kernel, sm, knob) for cid, c in zip(wc.CASE_IDS, wc.CASES) for kernel, sm, knob in wc.runs(c)]


@pytest.mark.parametrize("cid,kernel,seq_math,seq4", RUNS, ids=["%s-%s%s" % (k, r, "" if q is None else "-seq4=%d" % q) for r, k, _, q in RUNS])
def test_weight_gradient_edges_match_the_fp64_oracle(cid, kernel, seq_math, seq4, monkeypatch):
    import numpy as np
    from pathnet_amd import _lib, modules
    c = wc.CASES[wc.CASE_IDS.index(cid)]
    want = wc.reference(cid)
    d = wc.make_inputs(c)
    m = _module(c, wc.make_params(c), seq_math)
    if seq4 is not None:
        _lib.set_knob("PN_SEQ4", seq4)
    monkeypatch.setattr(modules, "pick_batch_groups", lambda *a, **k: c.batch_groups)
    dev = dict(X=d["X"].cuda(), mask_seq=d["mask_seq"].cuda(), mask_cls=d["mask_cls"].cuda(),
               neis=torch.as_tensor(d["ids"].reshape(c.S, c.W * c.L).astype(np.int64)),
               codes=torch.as_tensor(d["codes"].astype(np.int64)))
    msgs = []
    for kind, group in wc.probes(c):
        out, g = _hip(m, c, d, dev, wc.upstream(c, d["G"], group))
        msgs += wc.check(c, kind, group, out, g, want[kind], kernel)
    # the arithmetic asked for is the one that ran: an explicit seq_math switches the module's range guard off, and nothing
    # has moved the module to bf16 x 3 behind the test's back
    assert m.seq_math == seq_math and not m._range_wide
    assert not msgs, "\n".join(msgs)
