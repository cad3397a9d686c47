"""module.paths_stream() (pn_pagg_paths_stream): a training loop enqueues each step's walk where the aggregator reads the path
arrays -- the library's second stream -- so that it runs under the tail of the previous step.  Every reader of ids / codes
must then be ordered after that walk, and the walk after every reader of the previous step's paths, whatever shape the
calls have: a compact call reads them on the caller's stream ahead of its fork (run_compact_rows), the batch shape can
change between steps, and a sampler driven by a StepState reads epoch and seed advanced on the main stream.

In a normal loop the walk finishes before its readers start, so these tests hold one stream back on purpose
(torch.cuda._sleep, checked to last >= 20 ms) and compare, bit for bit (deterministic backward), eight steps of
sample -> step -> Adam against the same loop with the walk on the main stream; the last step's logits are also held to
the fp64 oracle on the paths read back from the buffers."""
import numpy as np
import pytest
import torch

from oracle import pagg_oracle as po

pytestmark = pytest.mark.gpu

F, H, C, W, L = 24, 64, 5, 8, 4
HOLD_MS, HOLD_MIN_MS = 30.0, 20.0
STEPS = 8
TOL = 1e-5


@pytest.fixture(scope="module")
def hold_cycles():
    """torch.cuda._sleep cycles for HOLD_MS, measured once"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda._sleep(1000)
    a.record()
    torch.cuda._sleep(1_000_000)
    b.record()
    b.synchronize()
    ms = a.elapsed_time(b)
    assert ms > 0.01, ms
    return int(1_000_000 * HOLD_MS / ms)


def _graph(n, seed=3):
    import bench
    return bench.synthetic_graph(n, seed)


class Holds:
    """sleeps put on a stream, each between two timing events"""

    def __init__(self, cycles):
        self.cycles, self.ev = cycles, []

    def __call__(self, stream):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(stream):
            a.record()
            torch.cuda._sleep(self.cycles)
            b.record()
        self.ev.append((a, b))

    def check(self):
        assert self.ev
        for a, b in self.ev:
            assert a.elapsed_time(b) >= HOLD_MIN_MS, "a hold lasted %.1f ms only" % a.elapsed_time(b)


def train(variant, n, batches, beside, cycles, fused=True, hold="producer", step_state=None, seed=1):
    """STEPS steps of sample -> fused step (or forward + backward) -> Adam; step e trains batches[e % len(batches)] (an
    int32 tensor of masked nodes).  beside: the walk on model.paths_stream(), else on the current stream.  hold: the stream
    held back -- "producer" (the walk's, ahead of it), "consumer" (the main stream between forward and backward) or
    "advance" (the main stream ahead of the step state's advance: StepState.advance(), or Adam with advance_in_adam).
    step_state: None, or advance_in_adam for a StepState that drives the sampler and the step.
    Returns losses, parameters, every step's paths, the last step's logits / parameters before it / batch index."""
    import pathnet_amd
    nn_, u, v, p = _graph(n)
    smp = pathnet_amd.MerwSampler(nn_, u, v, p, L, device="cuda")
    X = torch.rand(n, F, generator=torch.Generator().manual_seed(seed)).cuda()
    y_all = torch.as_tensor(np.random.default_rng(seed).integers(0, C, n)).cuda()
    torch.manual_seed(seed)
    cls = {"homo": pathnet_amd.PathNet_homo, "hetero": pathnet_amd.PathNet, "pagg": pathnet_amd.PAGG}[variant]
    m = cls(F, H, C, L, dropout=0.5).cuda().train()
    m.deterministic = True
    st = None
    if step_state is not None:
        st = pathnet_amd.StepState("cuda", seed=1234, first_epoch=0, advance_in_adam=step_state)
        m.step_state = st
    opt = pathnet_amd.Adam(m.parameters(), lr=0.01, step_state=st)
    g = torch.Generator().manual_seed(seed + 1)
    masks = [((torch.rand(L, len(s) * W, H, generator=g) < 0.5).float().cuda() / 0.5,
              (torch.rand(len(s), 2 * H, generator=g) < 0.5).float().cuda() / 0.5) for s in batches]
    bufs = [(torch.empty((1, len(s), W, L), dtype=torch.int32, device="cuda"),
             torch.empty((1, len(s), W, L), dtype=torch.uint8, device="cuda")) for s in batches]
    for s, out in zip(batches, bufs):       # valid paths in every buffer from step 0 on: a stale read stays in bounds
        smp.sample(W, 5, epoch_begin=0, nodes=s, draw_source=pathnet_amd.DRAW_PHILOX, check=False, out=out)
    holds = Holds(cycles)
    main = torch.cuda.current_stream()
    losses, paths = [], []
    for e in range(STEPS):
        k = e % len(batches)
        sel, (ids, codes) = batches[k], bufs[k]
        if st is not None:
            if hold == "advance" and not st.advance_in_adam:
                holds(main)
            st.advance()
        ps = m.paths_stream() if beside else main
        with torch.cuda.stream(ps):
            if hold == "producer":
                holds(ps)
            smp.sample(W, 77, epoch_begin=e, epoch_count=1, nodes=sel, draw_source=pathnet_amd.DRAW_PHILOX, check=False,
                       out=(ids, codes), step_state=st)
            paths.append((ids.clone(), codes.clone()))      # (on the walk's stream: what it wrote)
        opt.zero_grad(set_to_none=True)
        m._mask_seq, m._mask_cls = masks[k]
        before = {name: t.detach().clone() for name, t in m.state_dict().items()}
        y = y_all[sel.long()]
        loss, out = m.forward_loss(X, ids[0], W, L, sel, codes[0], y, fused=fused)
        if hold == "consumer":
            holds(main)
        pathnet_amd.backward(loss)
        if st is not None and hold == "advance" and st.advance_in_adam:
            holds(main)
        opt.step()
        losses.append(loss.detach())
    torch.cuda.synchronize()
    holds.check()
    return dict(losses=torch.stack(losses).cpu(), params=[q.detach().cpu() for q in m.parameters()],
                paths=[(i.cpu(), c.cpu()) for i, c in paths], out=out.detach().cpu(), before=before, k=k, X=X.cpu(),
                masks=masks, batches=batches)


def assert_same_steps(ref, got, variant):
    for e, ((ia, ca), (ib, cb)) in enumerate(zip(ref["paths"], got["paths"])):
        assert torch.equal(ia, ib) and torch.equal(ca, cb), "step %d: other paths" % e
    assert torch.equal(ref["losses"], got["losses"]), (ref["losses"], got["losses"])
    for a, b in zip(ref["params"], got["params"]):
        assert torch.equal(a, b)
    # the last step's logits against fp64, on the paths it read
    k = got["k"]
    ids, codes = got["paths"][-1]
    sel = got["batches"][k].cpu().numpy()
    ms, mc = got["masks"][k]
    params = {name: t.cpu().double() for name, t in got["before"].items()}
    want = po.forward(variant, params, got["X"].double(), ids[0].numpy(), codes[0].numpy(), sel, W, L, dtype=torch.float64,
                      drop_seq=ms.cpu(), drop_cls=mc.cpu())
    err = (got["out"].double() - want).abs().max().item()
    assert err <= TOL * max(1.0, want.abs().max().item()), err


def _sel(n, S, seed=0):
    return torch.as_tensor(np.sort(np.random.default_rng(seed).choice(n, S, replace=False)), dtype=torch.int32).cuda()


def _compact(variant, n, S):
    from pathnet_amd import modules as M
    return M.shape_info(M._shape(variant, n, F, H, C, S, W, L))[0]


# (variant, n, S, PN_COMPACT, fused): compact by the library's own choice (n = 20 000: 8 192 path steps, 80 000 rows),
# compact forced at a shape that is dense by default, and the dense control
@pytest.mark.parametrize("variant,n,S,compact,fused", [
    ("homo", 20000, 256, None, True),
    ("homo", 600, 200, "1", False),
    ("hetero", 20000, 256, None, False),
    ("hetero", 600, 200, "1", True),
    ("pagg", 20000, 256, None, True),
    ("pagg", 600, 200, "1", False),
    ("homo", 600, 200, "0", True),          # dense: the call reads the paths on the second stream only
])
def test_compact_reader_waits_for_a_delayed_walk(variant, n, S, compact, fused, hold_cycles, monkeypatch):
    """The walk on paths_stream() held back: the touched-row marks of a compact call (caller's stream, ahead of the fork)
    must still read this step's paths."""
    if compact is None:
        monkeypatch.delenv("PN_COMPACT", raising=False)
    else:
        monkeypatch.setenv("PN_COMPACT", compact)
    assert _compact(variant, n, S) == (compact != "0")
    batches = [_sel(n, S)]
    ref = train(variant, n, batches, False, hold_cycles, fused=fused)
    got = train(variant, n, batches, True, hold_cycles, fused=fused)
    assert_same_steps(ref, got, variant)


@pytest.mark.parametrize("variant,fused", [("homo", True), ("hetero", False)])
def test_batch_shape_changes_between_steps(variant, fused, hold_cycles, monkeypatch):
    """A dense-sized and a compact-sized batch in turn on one module: paths_stream() is judged by the OTHER shape (after a
    dense call it answers the second stream, and the compact call that follows reads on the main stream)."""
    monkeypatch.delenv("PN_COMPACT", raising=False)
    n = 3000
    batches = [_sel(n, 300, 1), _sel(n, 100, 2)]
    assert not _compact(variant, n, 300) and _compact(variant, n, 100)
    ref = train(variant, n, batches, False, hold_cycles, fused=fused)
    got = train(variant, n, batches, True, hold_cycles, fused=fused)
    assert_same_steps(ref, got, variant)


@pytest.mark.parametrize("n,S,compact", [(20000, 256, None), (600, 200, "0")])
def test_walk_waits_for_the_readers_of_the_previous_paths(n, S, compact, hold_cycles, monkeypatch):
    """Write-after-read: the main stream held between the forward and the backward of a non-fused step; the next step's walk
    on paths_stream() must not overwrite ids / codes before the current step's readers have run."""
    if compact is None:
        monkeypatch.delenv("PN_COMPACT", raising=False)
    else:
        monkeypatch.setenv("PN_COMPACT", compact)
    batches = [_sel(n, S)]
    ref = train("homo", n, batches, False, hold_cycles, fused=False, hold="consumer")
    got = train("homo", n, batches, True, hold_cycles, fused=False, hold="consumer")
    assert_same_steps(ref, got, "homo")


@pytest.mark.parametrize("advance_in_adam", [False, True])
def test_step_state_walk_sees_the_advanced_epoch(advance_in_adam, hold_cycles, monkeypatch):
    """A sampler driven by model.step_state reads epoch and seed from device memory, advanced on the main stream (advance()
    or Adam's last launch): the main stream held ahead of the advance, the walk placed by paths_stream() must still see the
    new epoch -- every step's paths equal the main-stream run's."""
    monkeypatch.delenv("PN_COMPACT", raising=False)
    n, S = 600, 200
    batches = [_sel(n, S)]
    ref = train("homo", n, batches, False, hold_cycles, hold="advance", step_state=advance_in_adam)
    got = train("homo", n, batches, True, hold_cycles, hold="advance", step_state=advance_in_adam)
    assert len({tuple(i.flatten()[:64].tolist()) for i, _ in ref["paths"]}) == STEPS     # a new epoch's walks every step
    assert_same_steps(ref, got, "homo")
