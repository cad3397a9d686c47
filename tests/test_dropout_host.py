"""The dropout reference (tests/dropout_ref.py) and the probe constructions (tests/dropout_probes.py), on the CPU alone.

The chain that decides what the right mask is: Random123's known answers for Philox4x32-10 -> the numpy restatement ->
oracle.merw.philox_draw (oracle/merw_oracle.c), which the GPU sampler tests pin bit-exact to rocRAND.  The probes are proved
on oracle/pagg_oracle.py with the reference masks: the decoders of tests/test_gpu_dropout_masks.py must read back every
bit of both masks from the oracle's outputs, for every probe case -- a coverage of 100 %, nothing left out."""
import numpy as np
import pytest
import torch

import dropout_probes as dp
import dropout_ref as dr
from optim_ref import splitmix_advance
from oracle import merw

SEEDS = (0, 1, 2 ** 62 - 1, 0x1234ABCD9876FEDC)
COUNTERS = (0, 1, 2 ** 32 - 1, 2 ** 32, 2 ** 33 + 5)


def test_known_answers_of_philox4x32_10():
    f = 0xFFFFFFFF
    kat = [((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
           ((f, f, f, f), (f, f), (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
           ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0),
            (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1))]
    for ctr, key, want in kat:
        assert tuple(int(w) for w in dr.philox4x32_10(ctr, key)) == want
    # the same three through the vectorised path, in one call
    got = dr.philox4x32_10(tuple(np.array([k[0][i] for k in kat]) for i in range(4)),
                           tuple(np.array([k[1][i] for k in kat]) for i in range(2)))
    assert got.dtype == np.uint32 and [tuple(int(w) for w in r) for r in got] == [k[2] for k in kat]


@pytest.mark.parametrize("seed", SEEDS)
def test_hash_equals_the_c_oracle(seed):
    """counter words (ctr lo, ctr hi, stream, tag), key (seed lo, seed hi): mo_philox_draw with sub = tag << 32 | stream"""
    for stream in (dr.STREAM_SEQ, dr.STREAM_CLS):
        words = dr.philox4(seed, np.array(COUNTERS, dtype=np.uint64), stream)
        for i, ctr in enumerate(COUNTERS):
            want = [merw.philox_draw(seed, (dr.TAG << 32) | stream, 4 * ctr + k) for k in range(4)]
            assert [int(w) for w in words[i]] == want, (seed, stream, ctr)
            assert [int(w) for w in dr.philox4(seed, ctr, stream)] == want
    assert not np.array_equal(dr.philox4(seed, 7, 1), dr.philox4(seed, 7, 2))


@pytest.mark.parametrize("p", [0.1, 0.4, 0.5, 0.7, 0.9])
def test_keep_share(p):
    n = 1 << 20
    words = dr.philox4(0x5EED0001CAFE, np.arange(n // 4, dtype=np.uint64), dr.STREAM_SEQ).reshape(-1)
    q = 1.0 - float(np.float32(p))
    share = float(dr.keep(words, p).mean())
    assert abs(share - q) <= 4.0 * (q * (1.0 - q) / n) ** 0.5, (p, share)
    assert int(dr.cut(p)) == int(float(np.float32(p)) * 2 ** 32)
    assert int(dr.cut(1.0)) == 4294967040


def test_mask_layouts():
    """element [t, slot, 4 c4 + k] of stream 1 and element e of stream 2, spelt out one word at a time"""
    seed, p, L, P, Hk, S = 0x0123456789ABCDEF, 0.4, 3, 5, 32, 4
    ms, mc = dr.seq_mask(seed, p, L, P, Hk), dr.cls_mask(seed, p, S, Hk)
    assert ms.shape == (L, P, Hk) and mc.shape == (S, 2 * Hk) and ms.dtype == mc.dtype == np.float32
    sc, cut = np.float32(1) / (np.float32(1) - np.float32(p)), int(dr.cut(p))
    for t, slot, h in ((0, 0, 0), (1, 3, 17), (2, 4, 31), (2, 0, 6)):
        w = merw.philox_draw(seed, (dr.TAG << 32) | 1, 4 * ((t * P + slot) * (Hk // 4) + h // 4) + h % 4)
        assert ms[t, slot, h] == (sc if w >= cut else 0)
    for s, e in ((0, 0), (1, 63), (3, 33), (2, 5)):
        w = merw.philox_draw(seed, (dr.TAG << 32) | 2, s * 2 * Hk + e)
        assert mc[s, e] == (sc if w >= cut else 0)
    assert set(np.unique(ms)) == {np.float32(0), sc}
    # a hidden size that the kernels pad: drawn at Hk = 128, cut to the module's 100
    a, b = dr.module_masks(seed, p, L, S, 2, 100)
    full, fullc = dr.seq_mask(seed, p, L, S * 2, 128), dr.cls_mask(seed, p, S, 128)
    assert a.shape == (L, S * 2, 100) and np.array_equal(a.numpy(), full[:, :, :100])
    assert np.array_equal(b.numpy()[:, 100:], fullc[:, 128:228])


def test_module_seed_and_step_state_seeds():
    s = dr.module_seed(7)
    torch.manual_seed(7)
    assert s == int(torch.randint(0, 2 ** 62, (1,)).item()) and 0 <= s < 2 ** 62
    st = {"epoch": -1, "seed": 1234, "adam_step": 0}
    seeds = []
    for _ in range(3):
        st = splitmix_advance(st)
        seeds.append(st["seed"])
    assert len(set(seeds)) == 3 and all(0 <= x < 2 ** 64 for x in seeds)


# ---- the probes, proved on the oracle ---------------------------------------------------------------------------------------
C = 16


def _setup(case, ego_first=False):
    variant, cell, H, S, W, L, p = case
    sel, ids, codes = dp.paths(S, W, L, seed=3, ego_first=ego_first)
    ms, mc = dr.module_masks(0x0BADC0DE12345678, p, L, S, W, H)
    return sel, ids, codes, torch.zeros(dp.N, H), ms, mc


@pytest.mark.parametrize("case", dp.PROBE_CASES, ids=dp.case_id)
def test_forward_probe_reads_every_bit_of_the_sequence_mask(case):
    variant, cell, H, S, W, L, p = case
    sel, ids, codes, X, ms, mc = _setup(case)
    bits = torch.zeros(L, S * W, H, dtype=torch.bool)
    seen = torch.zeros_like(bits)
    slot = dp.slots(variant, S, W)
    if cell in dp.REDUCING:
        sd = dp.params(variant, cell, H, L, C, dp.amp_powers(L))
        r = dp.oracle_run(variant, cell, sd, X, sel, ids, codes, W, L, ms, mc)
        dp.put_sum_bits(bits, r["path_state"], slot, L, cell == "mean")
        seen[:, torch.as_tensor(slot).reshape(-1)] = True
    else:
        for t in range(L):
            sd = dp.params(variant, cell, H, L, C, dp.amp_one_step(p, L, t))
            r = dp.oracle_run(variant, cell, sd, X, sel, ids, codes, W, L, ms, mc)
            dp.put_forward_bits(bits, t, r["path_state"], slot)
            seen[t, torch.as_tensor(slot).reshape(-1)] = True
    assert bool(seen.all())                     # no position left out
    assert torch.equal(bits, ms != 0)


@pytest.mark.parametrize("case", dp.PROBE_CASES, ids=dp.case_id)
def test_backward_probe_reads_every_bit_of_the_sequence_mask(case):
    variant, cell, H, S, W, L, p = case
    sel, ids, codes, X, ms, mc = _setup(case)
    amp = dp.amp_powers(L) if cell in dp.REDUCING else dp.amp_every_step(p, L)
    sd = dp.params(variant, cell, H, L, C, amp)
    r = dp.oracle_run(variant, cell, sd, X, sel, ids, codes, W, L, ms, mc, loss=dp.pooled_loss(H))
    node = dp.po.plan(variant, ids, codes, S, W, L)[0]
    assert len(np.unique(node)) == node.size        # every (slot, step) has a row of X.grad of its own
    assert torch.equal(dp.backward_bits(r["grads"]["X"], node), ms != 0)
    others = np.setdiff1d(np.arange(dp.N), node.reshape(-1))
    assert float(r["grads"]["X"][others].abs().max()) == 0.0


@pytest.mark.parametrize("case", [c for c in dp.PROBE_CASES if c[1] not in dp.REDUCING], ids=dp.case_id)
def test_classifier_probe_reads_every_bit_of_the_classifier_mask(case):
    variant, cell, H, S, W, L, p = case
    sel, ids, codes, X, ms, mc = _setup(case)
    sd = dp.params(variant, cell, H, L, C, dp.amp_every_step(p, L), cell_bias=1.0)
    grads, xg = [], []
    for k in range(-(-S // C)):
        G = dp.one_hot_pass(S, C, k)
        r = dp.oracle_run(variant, cell, sd, X, sel, ids, codes, W, L, ms, mc, loss=lambda out, emb: (out * G).sum())
        assert float(r["embedding"].min()) > 0.0
        grads.append(r["grads"]["fc2.weight"])
        xg.append(r["grads"]["X"])
    assert torch.equal(dp.classifier_bits(grads, S, C), mc != 0)
    # the mask as the BACKWARD applies it to the embedding's gradient: the ego half arrives alone on the masked nodes' rows
    ego, joint = dp.joint_bits(xg, sel, dp.po.plan(variant, ids, codes, S, W, L)[0], S, W, C, variant)
    assert torch.equal(ego, mc[:, :H] != 0)
    assert torch.equal(joint, (ms != 0) & (mc[:, H:] != 0)[torch.as_tensor(dp.group_of(variant, S, W))][None])


@pytest.mark.parametrize("case", [c for c in dp.PROBE_CASES if c[0] == "homo" and c[1] not in dp.REDUCING], ids=dp.case_id)
def test_merged_step0_rows_count_the_kept_bits(case):
    variant, cell, H, S, W, L, p = case
    sel, ids, codes, X, ms, mc = _setup(case, ego_first=True)
    sd = dp.params(variant, cell, H, L, C, dp.amp_one_step(p, L, 0))
    r = dp.oracle_run(variant, cell, sd, X, sel, ids, codes, W, L, ms, mc, loss=dp.pooled_loss(H), dtype=torch.float64)
    want = (ms[0] != 0).view(S, W, H).sum(dim=1)
    g = r["grads"]["X"][sel]
    unit = float((g[want > 0] / want[want > 0]).median()) if bool((want > 0).any()) else 1.0
    assert unit > 0 and torch.equal(dp.merged_counts(g, unit), want)
