"""Round-2 surface of the aggregator (through the C ABI): micro-batches, slices of a batch, hidden sizes that are any
multiple of 32, shapes beyond 2^32 elements (BASELINE.json configs[4]), the shared projected tables of the
validation / test forwards, contexts, and an end-to-end training trajectory against the CPU oracle."""
import threading

import numpy as np
import pytest
import torch

from oracle import pagg_oracle as po
from gradcheck import assert_grads_close, named_grads
from test_gpu_pagg import TOL_OUT, build_module, run_module, zero_ok

pytestmark = pytest.mark.gpu


def no_relu_ties(m):
    """Large-shape tests of the homo class: with millions of ReLU pre-activations one of them lands within rounding error
    of zero, where two correct fp32 evaluations (another summation order, the bf16 x 3 products) disagree about the gate --
    and ONE flipped gate shows up as |dZ element| in that bias gradient, far above the parity tolerance (seen: 5e-4 on
    nets.3.bias after fc0 moved to another kernel).  The gates are covered with ties-free-by-luck small shapes elsewhere;
    here every pre-activation is pushed away from zero, half of the columns to each side, so both gate outcomes occur."""
    with torch.no_grad():
        for k, v in m.named_parameters():
            if k.endswith("bias") and (k.startswith("fc0") or k.startswith("nets")):
                v.copy_(torch.where(torch.arange(v.numel(), device=v.device) % 2 == 0, 4.0, -4.0))
    return m


def random_case(rng, N, S, W, L):
    mask = np.zeros(N, bool)
    mask[rng.permutation(N)[:S]] = True
    sel = np.flatnonzero(mask)
    ids = rng.integers(0, N, (S, W, L))
    ids[:, :, 0] = sel[:, None]
    codes = np.minimum(rng.integers(0, L, (S, W, L)), np.arange(L)[None, None, :])
    return mask, sel, ids, codes


@pytest.mark.parametrize("variant", ["hetero", "homo", "pagg"])
@pytest.mark.parametrize("mode", ["eval", "masks", "philox"])
def test_micro_batches_equal_one_batch(variant, mode, monkeypatch):
    """pn_pagg_shape.batch_groups: the library walks the masked nodes in micro-batches (forward keeps nothing, backward
    re-runs each micro-batch's recurrence).  Logits and every gradient must equal the one-batch run -- with explicit
    masks, and with the built-in Philox masks, whose counters are positions in the whole batch."""
    from pathnet_amd import modules
    torch.manual_seed(61)
    rng = np.random.default_rng(61)
    N, F, H, C, W, L, S = 90, 24, 64, 4, 12, 4, 53
    m = build_module(variant, F, H, C, L, N, None)
    mask, sel, ids, codes = random_case(rng, N, S, W, L)
    X = torch.rand(N, F).cuda()
    G = torch.randn(S, C).cuda()
    if mode == "eval":
        m.eval()
    else:
        m.train()
        m.set_dropout(0.5)
        if mode == "masks":
            m._mask_seq = ((torch.rand(L, S * W, H) >= 0.5).float() / 0.5).cuda()
            m._mask_cls = ((torch.rand(S, 2 * H) >= 0.5).float() / 0.5).cuda()

    def run(batch_groups):
        monkeypatch.setattr(modules, "pick_batch_groups", lambda *a, **k: batch_groups)
        m.zero_grad()
        Xd = X.clone().requires_grad_(True)
        torch.manual_seed(5)                    # same dropout seed
        out = run_module(m, Xd, ids, codes, mask, W, L)
        (out * G).sum().backward()
        return out.detach().clone(), {k: v.grad.clone() for k, v in m.named_parameters()}, Xd.grad.clone()

    out1, g1, gx1 = run(0)
    for bg in (7, 20, 52):                      # 8, 3 and 2 micro-batches, ragged tails
        outb, gb, gxb = run(bg)
        assert (outb - out1).abs().max().item() < 2e-6, (bg, "out")
        assert_grads_close(dict(gb, X=gxb), dict(g1, X=gx1), rel=2e-5, zero_ok=zero_ok(variant))


@pytest.mark.parametrize("variant", ["hetero", "homo", "pagg"])
def test_slice_of_a_batch_is_rows_of_the_whole_batch(variant):
    """pn_pagg_shape.S_total / group_begin (modules: group_slice): for the hetero class a row reads paths of OTHER
    masked nodes of the batch (PathNet_run.py:196-197); computed from the whole batch's index arrays a slice is still
    bit-for-bit the rows of the whole-batch result -- what node sharding across GPUs relies on."""
    torch.manual_seed(62)
    rng = np.random.default_rng(62)
    N, F, H, C, W, L, S = 70, 20, 64, 3, 9, 4, 41
    m = build_module(variant, F, H, C, L, N, None).eval()
    mask, sel, ids, codes = random_case(rng, N, S, W, L)
    X = torch.rand(N, F).cuda()
    neis = torch.as_tensor(ids.reshape(S, W * L).astype(np.int64))
    lt = torch.as_tensor(codes.astype(np.int64))
    with torch.no_grad():
        whole = m(X, neis, W, L, mask, lt, None)
        for begin, count in ((0, 13), (13, 20), (33, 8), (5, 0)):
            part = m(X, neis, W, L, mask, lt, None, group_slice=(begin, count))
            assert part.shape == (count, C)
            assert torch.equal(part, whole[begin:begin + count]), (begin, count)
    # gradients of the slices add up to the gradient of the whole batch
    G = torch.randn(S, C).cuda()
    m.zero_grad()
    (m(X, neis, W, L, mask, lt, None) * G).sum().backward()
    want = {k: v.grad.clone() for k, v in m.named_parameters()}
    m.zero_grad()
    for begin, count in ((0, 17), (17, 24)):
        (m(X, neis, W, L, mask, lt, None, group_slice=(begin, count)) * G[begin:begin + count]).sum().backward()
    assert_grads_close(named_grads(m), want, rel=2e-5, zero_ok=zero_ok(variant))
    with pytest.raises(ValueError):
        m(X, neis, W, L, mask, lt, None, group_slice=(30, 20))


@pytest.mark.parametrize("variant", ["hetero", "homo", "pagg"])
@pytest.mark.parametrize("H", [96, 160, 192, 224])
def test_hidden_sizes_that_are_multiples_of_32(variant, H):
    """The reference's -hid is any integer (PathNet_run.py:52); the recurrent kernels are instantiated for every
    multiple of 32 up to 256 (3, 5, 6, 7 waves per workgroup besides the powers of two)."""
    torch.manual_seed(63)
    rng = np.random.default_rng(63)
    N, F, C, W, L, S = 60, 18, 4, 11, 4, 27
    m = build_module(variant, F, H, C, L, N, None).eval()
    with torch.no_grad():
        for k, v in m.named_parameters():
            if k.endswith("bias"):
                v.uniform_(-0.3, 0.3)
    mask, sel, ids, codes = random_case(rng, N, S, W, L)
    X = torch.rand(N, F)
    G = torch.randn(S, C)
    Xd = X.cuda().requires_grad_(True)
    out = run_module(m, Xd, ids, codes, mask, W, L)
    (out * G.cuda()).sum().backward()
    pr = {k: v.detach().cpu().clone().requires_grad_(True) for k, v in m.state_dict().items()}
    Xo = X.clone().requires_grad_(True)
    want = po.forward(variant, pr, Xo, ids, codes, sel, W, L)
    (want * G).sum().backward()
    assert (out.detach().cpu() - want.detach()).abs().max().item() < TOL_OUT
    ref = {k: pr[k].grad for k, _ in m.named_parameters()}
    ref["X"] = Xo.grad
    assert_grads_close(named_grads(m, {"X": Xd.grad}), ref, zero_ok=zero_ok(variant))


def test_unsupported_hidden_sizes_fail_loudly():
    """The C ABI takes hidden sizes that are multiples of 32 up to 1024 and refuses the rest; the modules zero-pad any
    other size up to the next multiple (tests/test_gpu_pagg.py::test_hidden_size_that_is_not_a_multiple_of_32) and refuse
    what lies beyond 1024 -- with the library's error, not a fallback."""
    import ctypes
    from pathnet_amd import _lib, modules
    lib = _lib.load()
    for H in (48, 272, 1056):
        n = ctypes.c_int64(0)
        sh = modules._shape("homo", 20, 8, H, 3, 2, 3, 4)
        assert lib.pn_pagg_workspace_bytes(ctypes.byref(sh), ctypes.byref(n)) == _lib.PN_ERR_ARG
    m = build_module("homo", 8, 1056, 3, 4, 20, None).eval()
    with pytest.raises(_lib.PnError):
        run_module(m, torch.rand(20, 8).cuda(), np.zeros((2, 3, 4), np.int64), np.zeros((2, 3, 4), np.int64),
                   np.arange(20) < 2, 3, 4)


@pytest.mark.parametrize("variant", ["homo", "hetero"])
def test_configs4_shape_beyond_2_pow_32_elements(variant):
    """BASELINE.json configs[4] on one GPU, scaled to what a test can afford: N = 6 M nodes, hid = F = 128, L = 6, so
    that the node tables Z / dZ [N, L, H] hold 4.6e9 elements (> 2^32: round 1 refused the shape), the masked nodes
    walked in micro-batches.  Checked against the CPU oracle on the COMPACTED graph (only the visited nodes, renumbered:
    a node's logits depend on nothing else), including table rows beyond the 2^32-element offset."""
    from pathnet_amd import modules
    torch.manual_seed(64)
    rng = np.random.default_rng(64)
    N, F, H, C, W, L, S = 6_000_000, 128, 128, 4, 40, 6, 600
    assert N * L * H > 2 ** 32
    m = build_module(variant, F, H, C, L, N, None).eval()
    if variant == "homo":
        no_relu_ties(m)
    m.workspace_budget = modules.workspace_bytes(variant, N, F, H, C, 128, W, L) + 1       # -> micro-batches of <= 128 nodes
    sel = np.sort(rng.choice(N, S, replace=False))
    sel[-50:] = np.sort(rng.choice(np.arange(N - 100_000, N), 50, replace=False))    # high rows: offsets > 2^32 elements
    sel = np.unique(sel)
    S = len(sel)
    near = rng.integers(0, N, 5000)                     # paths revisit a pool of nodes (and the top of the table)
    near[:500] = rng.integers(N - 1000, N, 500)
    ids = near[rng.integers(0, len(near), (S, W, L))]
    ids[:, :, 0] = sel[:, None]
    codes = np.minimum(rng.integers(0, L, (S, W, L)), np.arange(L)[None, None, :])
    used = np.unique(np.concatenate([ids.reshape(-1), sel]))
    Xs = torch.rand(len(used), F)                       # features of the visited nodes; everything else is zero
    X = torch.zeros(N, F, device="cuda")
    X[torch.as_tensor(used).cuda()] = Xs.cuda()
    assert 0 < modules.pick_batch_groups(variant, N, F, H, C, S, W, L, m.workspace_budget) < S / 2     # several micro-batches
    G = torch.randn(S, C)
    d_ids, d_codes = torch.as_tensor(ids.astype(np.int32)).cuda(), torch.as_tensor(codes.astype(np.uint8)).cuda()
    out = m(X, d_ids, W, L, torch.as_tensor(sel.astype(np.int32)).cuda(), d_codes, None)
    (out * G.cuda()).sum().backward()
    # oracle on the compacted graph
    remap = np.full(N, -1, np.int64)
    remap[used] = np.arange(len(used))
    pr = {k: v.detach().cpu().clone().requires_grad_(True) for k, v in m.state_dict().items()}
    want = po.forward(variant, pr, Xs, remap[ids], codes, remap[sel], W, L)
    (want * G).sum().backward()
    assert (out.detach().cpu() - want.detach()).abs().max().item() < TOL_OUT
    # (the bias gradients of fc0 / the bank sum over all N rows on the GPU and over the visited rows in the
    #  oracle: rows nobody visits have zero upstream gradient, so they are the same numbers)
    assert_grads_close(named_grads(m), {k: pr[k].grad for k, _ in m.named_parameters()}, zero_ok=zero_ok(variant))


def test_validation_and_test_forwards_share_the_projected_tables():
    """pn_pagg_args.reuse_tables: the test forward of an epoch reuses Xh / Z of the validation forward
    (PathNet_run.py:362, :378 recompute fc0 and the bank) -- same logits, bit for bit."""
    torch.manual_seed(65)
    rng = np.random.default_rng(65)
    N, F, H, C, W, L = 200, 64, 128, 5, 40, 4
    m = build_module("homo", F, H, C, L, N, None).eval()
    X = torch.rand(N, F).cuda()
    mv, sv, iv, cv = random_case(rng, N, 50, W, L)
    mt, st, it, ct = random_case(rng, N, 90, W, L)          # larger batch: the workspace is re-allocated
    mt2, st2, it2, ct2 = random_case(rng, N, 30, W, L)
    with torch.no_grad():
        want_t = run_module(m, X, it, ct, mt, W, L).clone()
        want_t2 = run_module(m, X, it2, ct2, mt2, W, L).clone()
        run_module(m, X, iv, cv, mv, W, L)                  # "validation"
        S = 30
        got_t2 = m(X, torch.as_tensor(it2.reshape(S, -1)), W, L, mt2, torch.as_tensor(ct2), None, reuse_tables=True)
        assert torch.equal(got_t2, want_t2)
        # a forward whose workspace does not hold the tables falls back to computing them
        S = 90
        got_t = m(X, torch.as_tensor(it.reshape(S, -1)), W, L, mt, torch.as_tensor(ct), None, reuse_tables=True)
        assert torch.equal(got_t, want_t)
        # and the flag really skips the work: with the tables poisoned the result changes
        run_module(m, X, iv, cv, mv, W, L)
        m._ws_eval[:N * H * 4].zero_()
        S = 30
        poisoned = m(X, torch.as_tensor(it2.reshape(S, -1)), W, L, mt2, torch.as_tensor(ct2), None, reuse_tables=True)
        assert not torch.equal(poisoned, want_t2)
    with pytest.raises(RuntimeError):
        m(X, torch.as_tensor(it2.reshape(30, -1)), W, L, mt2, torch.as_tensor(ct2), None, reuse_tables=True)


def test_reused_tables_after_a_compact_forward():
    """a validation forward small enough to run over compact rows of the distance bank leaves only ITS
    rows of Z in the workspace; the test forward of the same epoch (PathNet_run.py:362, :378), large enough to run dense,
    must not read them as the full table.  The module hands on Xh alone after a compact call (reuse_tables = 2)."""
    from pathnet_amd import modules
    torch.manual_seed(67)
    rng = np.random.default_rng(67)
    N, F, H, C, W, L = 2000, 32, 128, 5, 4, 4
    m = build_module("homo", F, H, C, L, N, None).eval()
    X = torch.rand(N, F).cuda()
    mv, sv, iv, cv = random_case(rng, N, 100, W, L)         # 2 * 100 * 4 * 4 path steps < 2000 * 4 rows: compact
    mt, st, it, ct = random_case(rng, N, 600, W, L)         # 2 * 600 * 4 * 4 >= 8000: dense
    assert modules.shape_info(modules._shape("homo", N, F, H, C, 100, W, L))[0]
    assert not modules.shape_info(modules._shape("homo", N, F, H, C, 600, W, L))[0]
    with torch.no_grad():
        want_t = run_module(m, X, it, ct, mt, W, L).clone()
        want_v = run_module(m, X, iv, cv, mv, W, L).clone()
        # dense first (the workspace is large enough for both afterwards), then compact, then dense with reuse
        run_module(m, X, it, ct, mt, W, L)
        got_v = m(X, torch.as_tensor(iv.reshape(100, -1)), W, L, mv, torch.as_tensor(cv), None, reuse_tables=True)
        assert torch.equal(got_v, want_v)
        assert m._ws_tables is not None and m._ws_tables[1] is False        # Xh only from here on
        got_t = m(X, torch.as_tensor(it.reshape(600, -1)), W, L, mt, torch.as_tensor(ct), None, reuse_tables=True)
        assert torch.equal(got_t, want_t)
        assert m._ws_tables[1] is True
        # and once a dense forward has run, the next dense one reuses the bank as well
        got_t = m(X, torch.as_tensor(it.reshape(600, -1)), W, L, mt, torch.as_tensor(ct), None, reuse_tables=True)
        assert torch.equal(got_t, want_t)


def test_two_contexts_two_host_threads_one_device():
    """No process-global state: two host threads drive the same GPU through two pn_context handles on
    two streams at the same time; a NULL context works too (single stream); a context of another device is refused."""
    import ctypes
    from pathnet_amd import _lib, modules
    lib = _lib.load()
    torch.manual_seed(66)
    rng = np.random.default_rng(66)
    N, F, H, C, W, L, S = 120, 32, 128, 4, 40, 4, 60
    m = build_module("homo", F, H, C, L, N, None).eval()
    mask, sel, ids, codes = random_case(rng, N, S, W, L)
    X = torch.rand(N, F).cuda()
    with torch.no_grad():
        want = run_module(m, X, ids, codes, mask, W, L).clone()
    d_ids, d_codes = torch.as_tensor(ids.astype(np.int32)).cuda(), torch.as_tensor(codes.astype(np.uint8)).cuda()
    d_sel = torch.as_tensor(sel.astype(np.int32)).cuda()
    fw, fb, params = m._param_inputs()
    p = modules._split_params(params, L)
    nbytes = modules.workspace_bytes("homo", N, F, H, C, S, W, L)
    results, errors = {}, []

    def worker(tag, use_ctx):
        try:
            torch.cuda.set_device(0)
            ctx = ctypes.c_void_p()
            if use_ctx:
                _lib.check(lib.pn_context_create(ctypes.byref(ctx)))
            stream = torch.cuda.Stream()
            out = torch.empty(S, C, device="cuda")
            ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
            call = modules.PaggCall("homo", N, F, H, C, S, W, L, p_seq=0.0, p_cls=0.0, seed=0, bank_w=fw, bank_b=fb)
            a = call.args(d_ids, d_codes, d_sel, p, X=X)
            a.out, a.workspace, a.workspace_bytes, a.no_save = out.data_ptr(), ws.data_ptr(), ws.numel(), 1
            stream.wait_stream(torch.cuda.default_stream())
            for _ in range(20):
                _lib.check(lib.pn_pagg_forward(ctx if use_ctx else None, ctypes.byref(a),
                                               ctypes.c_void_p(stream.cuda_stream)))
            stream.synchronize()
            results[tag] = out.clone()
            if use_ctx:
                _lib.check(lib.pn_context_destroy(ctx))
        except Exception as e:      # noqa: BLE001
            errors.append((tag, repr(e)))

    threads = [threading.Thread(target=worker, args=("a", True)), threading.Thread(target=worker, args=("b", True)),
               threading.Thread(target=worker, args=("null", False))]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    for tag in ("a", "b", "null"):
        assert torch.equal(results[tag], want), tag
    assert lib.pn_context_destroy(None) == 0
    assert lib.pn_profile_configure(None, 1, -1) != 0           # profiling state lives in a context


def test_module_on_a_non_current_device_index():
    """launches must go to the device of the tensors, not to whatever device is current.  With one GPU this
    can only check that an explicit cuda:0 works while the calls are wrapped in torch.cuda.device()."""
    torch.manual_seed(67)
    rng = np.random.default_rng(67)
    N, F, H, C, W, L, S = 50, 16, 64, 3, 8, 4, 20
    m = build_module("homo", F, H, C, L, N, None).eval().to("cuda:0")
    mask, sel, ids, codes = random_case(rng, N, S, W, L)
    X = torch.rand(N, F)
    with torch.no_grad():
        out = run_module(m, X.to("cuda:0"), ids, codes, mask, W, L).cpu()
    want = po.forward("homo", {k: v.cpu() for k, v in m.state_dict().items()}, X, ids, codes, sel, W, L)
    assert (out - want).abs().max().item() < TOL_OUT


def test_sampler_rejects_wrong_output_tensors():
    """sample(out=...) validates shape / dtype / device before handing raw pointers to the kernel."""
    import pathnet_amd
    import bench
    n, u, v, p = bench.synthetic_graph(300, 1)
    smp = pathnet_amd.MerwSampler(n, u, v, p, 4, device="cuda")
    good = (torch.empty((1, n, 5, 4), dtype=torch.int32, device="cuda"),
            torch.empty((1, n, 5, 4), dtype=torch.uint8, device="cuda"))
    smp.sample(5, 1, out=good)
    for bad in ((torch.empty((1, n, 5, 3), dtype=torch.int32, device="cuda"), good[1]),
                (good[0].to(torch.int64), good[1]),
                (good[0], torch.empty((1, n, 5, 4), dtype=torch.uint8)),
                (good[0].transpose(2, 3), good[1])):
        with pytest.raises(ValueError):
            smp.sample(5, 1, out=bad)


@pytest.mark.parametrize("variant", ["hetero", "homo"])
def test_training_trajectory_matches_the_oracle(variant):
    """End-to-end substitute for the Cornell accuracy check (splits.zip is absent from the reference mount): the
    reference recipe -- Adam(lr 0.005, wd 5e-4) + CrossEntropyLoss, dropout 0.7, fresh paths every epoch
    (PathNet_run.py:336-352) -- run for 25 epochs with the SAME dropout masks on the HIP path (fused loss / Adam
    launches included) and on the CPU oracle (torch autograd + torch.optim.Adam): the loss trajectories agree to 1e-4
    and the predictions of all masked nodes are identical at the end."""
    import pathnet_amd
    torch.manual_seed(68)
    rng = np.random.default_rng(68)
    N, F, H, C, W, L, S, E = 120, 32, 64, 4, 20, 4, 60, 25
    pdrop = 0.7
    m = build_module(variant, F, H, C, L, N, None)
    m.set_dropout(pdrop)
    Y = torch.as_tensor(rng.integers(0, C, N))
    X = torch.rand(N, F) + torch.nn.functional.one_hot(Y, F).float() * 1.5
    mask = np.zeros(N, bool)
    mask[rng.permutation(N)[:S]] = True
    sel = np.flatnonzero(mask)
    pr = {k: v.detach().cpu().clone().requires_grad_(True) for k, v in m.state_dict().items()}
    opt_o = torch.optim.Adam(list(pr.values()), lr=0.005, weight_decay=0.0005)
    opt_h = pathnet_amd.Adam(m.parameters(), lr=0.005, weight_decay=0.0005)
    lossf_h = pathnet_amd.CrossEntropyLoss()
    Xd, Yd = X.cuda(), Y[mask].cuda()
    worst = 0.0
    for epoch in range(E):
        ids = rng.integers(0, N, (S, W, L))
        ids[:, :, 0] = sel[:, None]
        codes = np.minimum(rng.integers(0, L, (S, W, L)), np.arange(L)[None, None, :])
        mseq = (torch.rand(L, S * W, H) >= pdrop).float() / (1 - pdrop)
        mcls = (torch.rand(S, 2 * H) >= pdrop).float() / (1 - pdrop)
        m.train()
        m._mask_seq, m._mask_cls = mseq.cuda(), mcls.cuda()
        loss_h = lossf_h(run_module(m, Xd, ids, codes, mask, W, L), Yd)
        opt_h.zero_grad(set_to_none=True)
        loss_h.backward()
        opt_h.step()
        loss_o = torch.nn.functional.cross_entropy(po.forward(variant, pr, X, ids, codes, sel, W, L, drop_seq=mseq,
                                                              drop_cls=mcls), Y[mask])
        opt_o.zero_grad()
        loss_o.backward()
        opt_o.step()
        worst = max(worst, abs(loss_h.item() - loss_o.item()))
        assert worst < 1e-4, (epoch, loss_h.item(), loss_o.item())
    m.eval()
    with torch.no_grad():
        pred_h = run_module(m, Xd, ids, codes, mask, W, L).argmax(1).cpu()
        out_o = po.forward(variant, pr, X, ids, codes, sel, W, L)
    top2 = out_o.topk(2, dim=1).values
    clear = (top2[:, 0] - top2[:, 1]) > 1e-3            # (ties within rounding are not predictions)
    assert torch.equal(pred_h[clear], out_o.argmax(1)[clear]) and clear.float().mean() > 0.9
    for k, v in m.state_dict().items():
        assert (v.cpu() - pr[k].detach()).abs().max().item() < 1e-3, k


def test_step_captured_in_a_hip_graph_replays_with_fresh_epoch_seed_and_adam_step():
    """pn_step_state: the sampler's epoch, the dropout seed and Adam's step count live in device memory and are read when
    the kernels run, so one training step captured into a hipGraph replays as the NEXT step each time (the library's
    second stream joins the capture through its fork / join events; no runtime call besides launches after warm-up)."""
    import pathnet_amd
    import bench
    n, u, v, p = bench.synthetic_graph(400, 2)
    rng = np.random.default_rng(70)
    F, H, C, W, L = 24, 64, 4, 10, 4
    X = torch.rand(n, F, device="cuda")
    Y = torch.as_tensor(rng.integers(0, C, n)).cuda()
    sel = torch.as_tensor(np.sort(rng.permutation(n)[:150])).cuda()
    sel32 = sel.to(torch.int32)

    def make():
        torch.manual_seed(7)
        smp = pathnet_amd.MerwSampler(n, u, v, p, L, device="cuda")
        m = pathnet_amd.PathNet_homo(F, H, C, L, dropout=0.5).cuda().train()
        st = pathnet_amd.StepState("cuda", seed=1234, first_epoch=0)
        m.step_state = st
        opt = pathnet_amd.Adam(m.parameters(), lr=0.005, weight_decay=0.0005, step_state=st)
        lossf = pathnet_amd.CrossEntropyLoss()
        ids_buf = torch.empty((1, n, W, L), dtype=torch.int32, device="cuda")
        codes_buf = torch.empty((1, n, W, L), dtype=torch.uint8, device="cuda")
        loss_out = torch.zeros((), device="cuda")

        def step():
            st.advance()
            smp.sample(W, 0, check=False, out=(ids_buf, codes_buf), step_state=st)
            out = m(X, ids_buf[0].index_select(0, sel), W, L, sel32, codes_buf[0].index_select(0, sel), None)
            loss = lossf(out, Y[sel])
            opt.zero_grad(set_to_none=True)
            loss.backward()
            opt.step()
            loss_out.copy_(loss.detach())
        return m, st, step, ids_buf, loss_out

    K = 6
    ma, sta, step_a, ids_a, loss_a = make()
    losses_a, first_ids = [], []
    for _ in range(K):
        step_a()
        losses_a.append(loss_a.item())
        first_ids.append(ids_a[0, :, :, 1].clone())
    assert sta.values()["epoch"] == K - 1 and sta.values()["adam_step"] == K
    assert not torch.equal(first_ids[0], first_ids[1])                      # a new epoch's walks every step

    mb, stb, step_b, ids_b, loss_b = make()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step_b()                                                            # warm-up = step 1
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    losses_b = [loss_b.item()]
    assert torch.equal(ids_b[0, :, :, 1], first_ids[0])
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        step_b()                                                            # captured, not run
    assert stb.values()["adam_step"] == 1
    for k in range(1, K):
        g.replay()
        torch.cuda.synchronize()
        losses_b.append(loss_b.item())
        assert torch.equal(ids_b[0, :, :, 1], first_ids[k]), k             # the replay sampled epoch k
    assert stb.values() == sta.values()
    assert max(abs(a - b) for a, b in zip(losses_a, losses_b)) < 1e-4, (losses_a, losses_b)
    for (k, va), (_, vb) in zip(ma.state_dict().items(), mb.state_dict().items()):
        assert (va - vb).abs().max().item() < 5e-4, k


@pytest.mark.parametrize("variant,cell", [("hetero", "gru"), ("homo", "gru"), ("pagg", "gru"), ("hetero", "mean"),
                                          ("homo", "sum"), ("pagg", "mean"), ("pagg", "lstm"), ("hetero", "rnn")])
@pytest.mark.parametrize("H,train", [(64, False), (128, True)])
def test_ablation_cells_match_the_oracle(variant, cell, H, train):
    """the path encoders of the paper's ablation rows (GRU / mean / sum, README.md:118 -- no code in the
    reference; pinned to torch.nn.GRU and the definitions in tests/test_oracle_pagg.py) and the classes' own cells
    swapped (LSTM in PAGG, RNN in PathNet): logits and every gradient against the CPU oracle, eval and with injected
    dropout masks; the GRU rides on the LSTM kernels' four gate slots."""
    import pathnet_amd
    torch.manual_seed(71)
    rng = np.random.default_rng(71)
    N, F, C, W, L, S = 70, 20, 4, 13, 4, 29
    cls = {"hetero": pathnet_amd.PathNet, "homo": pathnet_amd.PathNet_homo, "pagg": pathnet_amd.PAGG}[variant]
    m = cls(F, H, C, L if variant != "pagg" else N, cell=cell).cuda()
    with torch.no_grad():
        for k, v in m.named_parameters():
            if k.endswith("bias") or "bias_" in k:
                v.uniform_(-0.3, 0.3)
    assert not (cell in ("mean", "sum") and any("weight_ih" in k for k in m.state_dict()))
    mask, sel, ids, codes = random_case(rng, N, S, W, L)
    X = torch.rand(N, F)
    G = torch.randn(S, C)
    drop_seq = drop_cls = None
    if train:
        drop_seq = (torch.rand(L, S * W, H) >= 0.5).float() / 0.5
        drop_cls = (torch.rand(S, 2 * H) >= 0.5).float() / 0.5
        m.train()
        m._mask_seq, m._mask_cls = drop_seq.cuda(), drop_cls.cuda()
    else:
        m.eval()
    Xd = X.cuda().requires_grad_(True)
    out = run_module(m, Xd, ids, codes, mask, W, L)
    (out * G.cuda()).sum().backward()
    pr = {k: v.detach().cpu().clone().requires_grad_(True) for k, v in m.state_dict().items()}
    Xo = X.clone().requires_grad_(True)
    want = po.forward(variant, pr, Xo, ids, codes, sel, W, L, drop_seq=drop_seq, drop_cls=drop_cls, cell=cell)
    (want * G).sum().backward()
    assert (out.detach().cpu() - want.detach()).abs().max().item() < TOL_OUT
    ref = {k: pr[k].grad for k, _ in m.named_parameters()}
    ref["X"] = Xo.grad
    assert_grads_close(named_grads(m, {"X": Xd.grad}), ref, zero_ok=zero_ok(variant))


@pytest.mark.parametrize("variant,cell,H,train", [("hetero", None, 288, True), ("homo", None, 512, True),
                                                  ("pagg", None, 320, False), ("hetero", "gru", 384, True),
                                                  ("homo", "rnn", 1024, False), ("pagg", "lstm", 512, True),
                                                  ("homo", "mean", 512, True)])
def test_hidden_sizes_beyond_the_fused_kernels(variant, cell, H, train):
    """-hid is any integer in the reference (PathNet_run.py:52).  Past 256 the recurrence runs step by step -- one fp32
    (3 x bf16 MFMA) GEMM per step on [x_t | h_{t-1}], element-wise cell kernels around it, the BPTT the same way in
    reverse, the weight gradient one split-K GEMM -- for every multiple of 32 up to 1024: logits and every gradient
    against the CPU oracle."""
    import pathnet_amd
    torch.manual_seed(73)
    rng = np.random.default_rng(73)
    N, F, C, W, L, S = 50, 20, 4, 7, 4, 19
    cls = {"hetero": pathnet_amd.PathNet, "homo": pathnet_amd.PathNet_homo, "pagg": pathnet_amd.PAGG}[variant]
    kw = {"cell": cell} if cell else {}
    m = cls(F, H, C, L if variant != "pagg" else N, **kw).cuda()
    with torch.no_grad():
        for k, v in m.named_parameters():
            if k.endswith("bias") or "bias_" in k:
                v.uniform_(-0.3, 0.3)
    mask, sel, ids, codes = random_case(rng, N, S, W, L)
    X = torch.rand(N, F)
    G = torch.randn(S, C)
    drop_seq = drop_cls = None
    if train:
        drop_seq = (torch.rand(L, S * W, H) >= 0.5).float() / 0.5
        drop_cls = (torch.rand(S, 2 * H) >= 0.5).float() / 0.5
        m.train()
        m._mask_seq, m._mask_cls = drop_seq.cuda(), drop_cls.cuda()
    else:
        m.eval()
    Xd = X.cuda().requires_grad_(True)
    out = run_module(m, Xd, ids, codes, mask, W, L)
    (out * G.cuda()).sum().backward()
    pr = {k: v.detach().cpu().clone().requires_grad_(True) for k, v in m.state_dict().items()}
    Xo = X.clone().requires_grad_(True)
    want = po.forward(variant, pr, Xo, ids, codes, sel, W, L, drop_seq=drop_seq, drop_cls=drop_cls, cell=cell)
    (want * G).sum().backward()
    scale = max(1.0, want.detach().abs().max().item())
    assert (out.detach().cpu() - want.detach()).abs().max().item() < TOL_OUT * scale
    ref = {k: pr[k].grad for k, _ in m.named_parameters()}
    ref["X"] = Xo.grad
    assert_grads_close(named_grads(m, {"X": Xd.grad}), ref, zero_ok=zero_ok(variant))


def test_generic_recurrence_in_micro_batches_with_builtin_dropout(monkeypatch):
    """hid = 512 walked in micro-batches with the Philox masks: same logits and gradients as one batch"""
    from pathnet_amd import modules
    import pathnet_amd
    torch.manual_seed(74)
    rng = np.random.default_rng(74)
    N, F, H, C, W, L, S = 60, 16, 512, 3, 6, 4, 23
    m = pathnet_amd.PathNet(F, H, C, L, dropout=0.4).cuda().train()
    mask, sel, ids, codes = random_case(rng, N, S, W, L)
    X = torch.rand(N, F).cuda()
    G = torch.randn(S, C).cuda()

    def run(bg):
        monkeypatch.setattr(modules, "pick_batch_groups", lambda *a, **k: bg)
        m.zero_grad()
        torch.manual_seed(9)
        out = run_module(m, X, ids, codes, mask, W, L)
        (out * G).sum().backward()
        return out.detach().clone(), {k: v.grad.clone() for k, v in m.named_parameters()}

    o1, g1 = run(0)
    o2, g2 = run(9)
    assert (o1 - o2).abs().max().item() < 2e-6 * max(1.0, o1.abs().max().item())
    assert_grads_close(g2, g1, zero_ok=zero_ok("hetero"))


@pytest.mark.parametrize("cell", ["gru", "sum"])
def test_ablation_cells_in_micro_batches_with_builtin_dropout(cell, monkeypatch):
    from pathnet_amd import modules
    import pathnet_amd
    torch.manual_seed(72)
    rng = np.random.default_rng(72)
    N, F, H, C, W, L, S = 80, 16, 64, 3, 10, 4, 37
    m = pathnet_amd.PathNet(F, H, C, L, dropout=0.4, cell=cell).cuda().train()
    mask, sel, ids, codes = random_case(rng, N, S, W, L)
    X = torch.rand(N, F).cuda()
    G = torch.randn(S, C).cuda()

    def run(bg):
        monkeypatch.setattr(modules, "pick_batch_groups", lambda *a, **k: bg)
        m.zero_grad()
        torch.manual_seed(9)
        out = run_module(m, X, ids, codes, mask, W, L)
        (out * G).sum().backward()
        return out.detach().clone(), {k: v.grad.clone() for k, v in m.named_parameters()}

    o1, g1 = run(0)
    o2, g2 = run(11)
    assert (o1 - o2).abs().max().item() < 2e-6
    assert_grads_close(g2, g1, rel=2e-5, zero_ok=zero_ok("hetero"))


def test_empty_batch_gives_empty_logits_and_zero_gradients():
    """an epoch whose mask selects no node (a rank of the sharded path whose block holds no masked node)"""
    torch.manual_seed(73)
    for variant in ("hetero", "homo", "pagg"):
        N, F, H, C, W, L = 30, 12, 64, 3, 7, 4
        m = build_module(variant, F, H, C, L, N, None).train()
        X = torch.rand(N, F).cuda().requires_grad_(True)
        mask = np.zeros(N, bool)
        out = m(X, torch.zeros((0, W * L), dtype=torch.int64), W, L, mask, torch.zeros((0, W, L), dtype=torch.int64), None)
        assert out.shape == (0, C)
        out.sum().backward()
        assert all(v.grad is not None and float(v.grad.abs().max()) == 0.0 for v in m.parameters())
        assert float(X.grad.abs().max()) == 0.0


@pytest.mark.parametrize("variant", ["hetero", "homo", "pagg"])
@pytest.mark.parametrize("S,W,L,N", [(1, 1, 1, 5), (1, 40, 4, 3), (7, 33, 4, 20), (5, 100, 4, 16), (3, 1, 6, 9),
                                     (24, 3, 2, 24), (2, 65, 3, 40)])
def test_ragged_and_degenerate_shapes_match_the_oracle(variant, S, W, L, N):
    """one masked node, one path, one step; path counts that are not multiples of the 32-row tile or exceed a
    wavefront's 64 lanes; every node masked; L = 1 .. 6 -- forward and all gradients against the oracle."""
    if variant == "pagg" and L != 4:
        pytest.skip("PAGG has exactly four distance layers nei0..nei3 (copy.py:310-313)")
    torch.manual_seed(74)
    rng = np.random.default_rng(74)
    F, H, C = 9, 64, 3
    m = build_module(variant, F, H, C, L, N, None).eval()
    with torch.no_grad():
        for k, v in m.named_parameters():
            if "bias" in k:
                v.uniform_(-0.3, 0.3)
    mask, sel, ids, codes = random_case(rng, N, S, W, L)
    X = torch.rand(N, F)
    G = torch.randn(S, C)
    Xd = X.cuda().requires_grad_(True)
    out = run_module(m, Xd, ids, codes, mask, W, L)
    (out * G.cuda()).sum().backward()
    pr = {k: v.detach().cpu().clone().requires_grad_(True) for k, v in m.state_dict().items()}
    Xo = X.clone().requires_grad_(True)
    want = po.forward(variant, pr, Xo, ids, codes, sel, W, L)
    (want * G).sum().backward()
    assert (out.detach().cpu() - want.detach()).abs().max().item() < TOL_OUT
    ref = {k: pr[k].grad if pr[k].grad is not None else torch.zeros_like(v) for k, v in m.named_parameters()}
    ref["X"] = Xo.grad
    # (L = 1: h_{-1} = 0, the recurrent weights get an exactly-zero gradient on both sides)
    # (S = 5, W = 100: the homo class's attention-bias gradient is a sum of 500 score gradients that cancel to a thousandth
    #  of their size -- 1.6e-4 of ITS norm, 1e-7 of the case's scale: fp32 summation order; every other case runs the default)
    assert_grads_close(named_grads(m, {"X": Xd.grad}), ref, zero_ok=zero_ok(variant), noise=2e-7 if W == 100 else 1e-9)


def test_indices_outside_the_graph_are_refused_or_clamped():
    """the reference indexes X / the Linear list with whatever the path file holds and dies with an IndexError; here
    host-side index lists are validated and device-resident ids / codes are clamped by the kernels (no out-of-bounds
    access whatever the file contained)"""
    torch.manual_seed(75)
    N, F, H, C, W, L, S = 12, 8, 64, 3, 5, 4, 4
    m = build_module("homo", F, H, C, L, N, None).eval()
    X = torch.rand(N, F).cuda()
    ids = torch.randint(0, N, (S, W, L))
    codes = torch.randint(0, L, (S, W, L))
    with pytest.raises(IndexError):
        m(X, ids.reshape(S, -1), W, L, np.array([0, 1, 2, N]), codes, None)
    bad_ids = ids.clone()
    bad_ids[0, 0, 1] = 10 ** 6
    bad_ids[1, 2, 3] = -5
    bad_codes = codes.clone()
    bad_codes[2, 1, 2] = 200
    with torch.no_grad():
        out = m(X, bad_ids.reshape(S, -1), W, L, np.array([0, 1, 2, 3]), bad_codes, None)
        fixed_ids = bad_ids.clamp(0, N - 1)
        fixed_codes = bad_codes.clamp(0, L - 1)
        want = m(X, fixed_ids.reshape(S, -1), W, L, np.array([0, 1, 2, 3]), fixed_codes, None)
    assert torch.isfinite(out).all() and torch.equal(out, want)


# ------------------------------------------------------------------------------------------------
# touched-row compaction of the distance bank (pn_pagg.hip: run_compact_rows; the kernels: pn_plan.hip)
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant,cell", [("homo", None), ("hetero", None), ("pagg", None), ("homo", "gru"), ("hetero", "mean")])
def test_compact_rows_forced_on_small_shapes_match_the_dense_bank(variant, cell, monkeypatch):
    """PN_COMPACT=1 forces the compact path where it would not pay: same logits (the bank's dot products run in the same
    order), gradients within the usual tolerance of the dense path and of the oracle; micro-batches and slices included."""
    import pathnet_amd
    from pathnet_amd import modules
    torch.manual_seed(81)
    rng = np.random.default_rng(81)
    N, F, H, C, W, L, S = 150, 20, 64, 4, 9, 4, 41
    cls = {"hetero": pathnet_amd.PathNet, "homo": pathnet_amd.PathNet_homo, "pagg": pathnet_amd.PAGG}[variant]
    m = cls(F, H, C, L if variant != "pagg" else N, cell=cell).cuda().train()
    mask, sel, ids, codes = random_case(rng, N, S, W, L)
    pdrop = 0.5
    ms = (torch.rand(L, S * W, H) >= pdrop).float() / (1 - pdrop)
    mc = (torch.rand(S, 2 * H) >= pdrop).float() / (1 - pdrop)
    m._mask_seq, m._mask_cls = ms.cuda(), mc.cuda()
    X = torch.rand(N, F)
    G = torch.randn(S, C).cuda()
    neis, lt = torch.as_tensor(ids.reshape(S, -1).astype(np.int64)), torch.as_tensor(codes.astype(np.int64))

    def run(compact, bg=None):
        monkeypatch.setenv("PN_COMPACT", "1" if compact else "0")
        if bg is not None:
            monkeypatch.setattr(modules, "pick_batch_groups", lambda *a, **k: bg)
        m.zero_grad(set_to_none=True)
        out = m(X.cuda(), neis, W, L, mask, lt, None)
        out.backward(G)
        return out.detach().clone(), {k: v.grad.detach().clone() for k, v in m.named_parameters()}
    dense_out, dense_g = run(False, 0)
    for bg in (0, 7):
        out, g = run(True, bg)
        assert (out - dense_out).abs().max().item() <= 1e-6, bg
        assert_grads_close(g, dense_g, zero_ok=zero_ok(variant))
    with torch.no_grad():       # a slice of the batch, compact
        part = m(X.cuda(), neis, W, L, mask, lt, None, group_slice=(5, 20))
    assert (part - dense_out[5:25]).abs().max().item() <= 1e-6
    pr = {k: v.detach().cpu().clone().requires_grad_(True) for k, v in m.state_dict().items()}
    want = po.forward(variant, pr, X, ids, codes, sel, W, L, drop_seq=ms, drop_cls=mc, cell=cell)
    assert (out.cpu() - want.detach()).abs().max().item() < 1e-5
    (want * G.cpu()).sum().backward()
    assert_grads_close(g, {k: pr[k].grad for k in g}, zero_ok=zero_ok(variant))


def test_compact_rows_on_a_million_node_graph_match_the_oracle():
    """N = 1 200 000 nodes, path_len 6: 7.2 M (node, code) rows, of which the 300 masked nodes x 12 paths x 6 steps can
    touch 21 600 (0.3 %): the library switches to compact rows by itself, the workspace shrinks with the tables, and
    logits and every gradient match the CPU oracle."""
    import pathnet_amd
    from pathnet_amd import modules
    torch.manual_seed(82)
    rng = np.random.default_rng(82)
    N, F, H, C, W, L, S = 1_200_000, 16, 128, 5, 12, 6, 300
    m = pathnet_amd.PathNet_homo(F, H, C, L).cuda().eval()
    X = torch.rand(N, F)
    sel = np.sort(rng.permutation(N)[:S])
    mask = np.zeros(N, bool)
    mask[sel] = True
    ids = rng.integers(0, N, (S, W, L))
    ids[:, :, 0] = sel[:, None]
    ids[:, :, 2] = ids[:, :, 1]                                  # repeated (node, code) pairs inside and across paths
    codes = np.minimum(rng.integers(0, L, (S, W, L)), np.arange(L)[None, None, :])
    dense_bytes = N * L * H * 4
    assert modules.workspace_bytes("homo", N, F, H, C, S, W, L) < 0.6 * 2 * dense_bytes       # Z and dZ are compact
    Xd = X.cuda().requires_grad_(True)
    out = run_module(m, Xd, ids, codes, mask, W, L)
    G = torch.randn(S, C)
    out.backward(G.cuda())
    pr = {k: v.detach().cpu().clone().requires_grad_(True) for k, v in m.state_dict().items()}
    Xr = X.clone().requires_grad_(True)
    want = po.forward("homo", pr, Xr, ids, codes, sel, W, L)
    assert (out.detach().cpu() - want.detach()).abs().max().item() < 1e-5
    want.backward(G)
    ref = {k: pr[k].grad for k, _ in m.named_parameters()}
    ref["X"] = Xr.grad
    assert_grads_close(named_grads(m, {"X": Xd.grad}), ref)


@pytest.mark.parametrize("variant,compact", [("homo", 0), ("homo", 1), ("hetero", 0), ("hetero", 1)])
def test_node_level_gemms_on_the_bf16_pipe_match_the_oracle(variant, compact, monkeypatch):
    """Graphs of >= ~50 000 rows run fc0 (feature width a multiple of 32), the distance bank and the bank's dX backward on
    gemm3_kernel (fp32 results from six bf16 MFMAs per product, 128 x 128 tiles) instead of the fp32-input MFMA kernel: the
    dense bank, and the bank over the touched rows (row lists, ReLU gate of the homo class; its dX stays on the fp32-input
    kernel, C += over the row list)."""
    import pathnet_amd
    monkeypatch.setenv("PN_COMPACT", str(compact))
    torch.manual_seed(91)
    rng = np.random.default_rng(91)
    N, F, H, C, W, L, S = 70_000, 32, 128, 5, 40, 4, 500          # 80 000 path steps: the compact bank is 80 000 rows at most
    cls = {"hetero": pathnet_amd.PathNet, "homo": pathnet_amd.PathNet_homo}[variant]
    m = cls(F, H, C, L).cuda().eval()
    if variant == "homo":
        no_relu_ties(m)
    X = torch.rand(N, F)
    sel = np.sort(rng.permutation(N)[:S])
    mask = np.zeros(N, bool)
    mask[sel] = True
    ids = rng.integers(0, N, (S, W, L))
    ids[:, :, 0] = sel[:, None]
    codes = np.minimum(rng.integers(0, L, (S, W, L)), np.arange(L)[None, None, :])
    Xd = X.cuda().requires_grad_(True)
    out = run_module(m, Xd, ids, codes, mask, W, L)
    G = torch.randn(S, C)
    out.backward(G.cuda())
    pr = {k: v.detach().cpu().clone().requires_grad_(True) for k, v in m.state_dict().items()}
    Xr = X.clone().requires_grad_(True)
    want = po.forward(variant, pr, Xr, ids, codes, sel, W, L)
    assert (out.detach().cpu() - want.detach()).abs().max().item() < 1e-5
    want.backward(G)
    ref = {k: pr[k].grad for k, _ in m.named_parameters()}
    ref["X"] = Xr.grad
    assert_grads_close(named_grads(m, {"X": Xd.grad}), ref, zero_ok=zero_ok(variant))
