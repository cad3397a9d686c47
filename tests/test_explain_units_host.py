"""Node and edge explanations without a GPU: pathnet_amd.member_nodes against the oracle's plan, the NumPy restatement
tests/explain_units_ref.py against explain_ref and its edge rules, the edge keys, the ValueErrors that name a limit, and the
header's new declarations against the bindings."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

import explain_ref as ref
import explain_units_ref as uref
import pathnet_amd
from conftest import ROOT
from oracle import pagg_oracle as po
from pathnet_amd import _lib

ex = sys.modules["pathnet_amd.explain"]       # (the package attribute `explain` is the function, not the module)


@pytest.mark.parametrize("shape", [(1, 1, 2), (6, 5, 4), (7, 3, 6)])
@pytest.mark.parametrize("variant", po.VARIANTS)
def test_member_nodes_is_the_oracles_plan_in_member_order(variant, shape):
    S, W, L = shape
    rng = np.random.default_rng(S * 100 + W * 10 + L)
    ids = rng.integers(0, 1000, (S, W, L)).astype(np.int32)
    node, _, group, member, _ = po.plan(variant, ids, np.zeros_like(ids), S, W, L)
    want = np.zeros((S, W, L), np.int64)
    want[group, member] = node                      # slot q -> (pooling group, member)
    got = pathnet_amd.member_nodes(variant, torch.as_tensor(ids), S, W, L)
    assert got.dtype == torch.int32 and tuple(got.shape) == (S, W, L) and (got.numpy() == want).all()
    flat = pathnet_amd.member_nodes(variant, torch.as_tensor(ids.reshape(S, W * L).astype(np.int64)), S, W, L)
    assert (flat.numpy() == want).all()
    with pytest.raises(ValueError):
        pathnet_amd.member_nodes(variant, torch.as_tensor(ids), S + 1, W, L)


def tiny(seed=0, S=4, W=6, H=5, C=3):
    rng = np.random.default_rng(seed)
    return dict(state=rng.standard_normal((S, W, H)).astype(np.float32), coef=(rng.random((S, W)) + 0.5).astype(np.float32),
                ego=rng.standard_normal((S, H)).astype(np.float32), fc2_w=rng.standard_normal((C, 2 * H)).astype(np.float32),
                fc2_b=rng.standard_normal(C).astype(np.float32))


@pytest.mark.parametrize("norm", (ref.NORM_SUM, ref.NORM_COUNT))
@pytest.mark.parametrize("renorm", (0, 1))
def test_one_label_per_member_is_explain_ref_bit_for_bit(norm, renorm):
    case = ref.make_case(S=5, W=7, H=9, C=4, G=3, seed=3, norm=norm, renorm=renorm)
    a = ref.run(case)
    b = uref.overlap(*case[:6], case.group[:, :, None], case.G, norm, renorm, case.target)
    for k in ("full", "contribution", "drop_logits", "keep_logits", "drop_delta", "keep_gain", "flip", "present", "target_used",
              "status", "rho_d", "rho_k"):
        assert np.asarray(getattr(a, k)).tobytes() == np.asarray(getattr(b, k)).tobytes(), k
    for k in a.tol:
        assert (a.tol[k] == b.tol[k]).all(), k


def test_overlap_edge_rules():
    d = tiny()
    S, W, C, G = 4, 6, 3, 4
    label = np.full((S, W, 3), -1, np.int32)
    label[:, :, 0] = 0                                  # unit 0 sits on every member
    label[:, :2, 1] = 1                                 # unit 1: members 0 and 1 ...
    label[:, 1, 2] = 1                                  # ... member 1 twice: counted once
    label[:, 5, 1] = G                                  # outside [0, G): no membership;  units 2 and 3 are empty
    weight = np.ones((S, W), np.float32)
    weight[1, 0] = 0.0                                  # row 1: member 0 is dead
    for renorm in (0, 1):
        r = uref.overlap(d["state"], d["coef"], d["ego"], d["fc2_w"], d["fc2_b"], weight, label, G, ref.NORM_SUM, renorm)
        assert (r.present == np.array([[6, 2, 0, 0], [5, 1, 0, 0], [6, 2, 0, 0], [6, 2, 0, 0]])).all()
        assert r.drop_logits[:, 0].tobytes() == r.e.tobytes()               # a unit on every path: the logits are e
        live_rows = [0, 2, 3]           # (row 1's full still sums its dead member's coefficient: the inputs' business)
        assert np.abs(r.keep_logits[live_rows, 0] - r.full[live_rows]).max() < 1e-12     # kept alone: every member, rho = 1
        for g in (2, 3):                                                    # empty: drop = full bit for bit, keep = e
            assert r.drop_logits[:, g].tobytes() == r.full.tobytes() and r.keep_logits[:, g].tobytes() == r.e.tobytes()
            assert (r.drop_delta[:, g] == 0).all() and (r.flip[:, g] == 0).all()
    t = uref.touches(label, G)
    assert t[0, 1].tolist() == [True, True, False, False, False, False] and not t[:, 2:].any() and t[:, 0].all()


def test_unit_labels_of_excluded_and_negative_ids():
    node = np.array([[[4, 7, 4], [9, -1, 7], [4, 4, 4]],
                     [[5, 5, 5], [5, 5, 5], [5, 5, 5]]], np.int32)
    unit, count, label = uref.units(node, uref.UNIT_NODE, exclude=np.array([4, 5], np.int32))
    assert count.tolist() == [2, 0] and unit[0].tolist() == [7, 9] + [-1] * 7 and (unit[1] == -1).all()
    assert label[0].tolist() == [[-1, 0, -1], [1, -1, 0], [-1, -1, -1]] and (label[1] == -1).all()
    unit, count, label = uref.units(node, uref.UNIT_NODE)
    assert count.tolist() == [3, 1] and unit[0, :3].tolist() == [4, 7, 9] and label[0, 1].tolist() == [2, -1, 1]
    unit, count, label = uref.units(node, uref.UNIT_EDGE)
    k = lambda a, b: int(uref.edge_key(a, b))                               # noqa: E731
    assert count.tolist() == [2, 1] and unit[0].tolist() == [k(4, 4), k(7, 4)] + [-1] * 4 and label.shape == (2, 3, 2)
    assert label[0].tolist() == [[1, 1], [-1, -1], [0, 0]] and unit[1, 0] == k(5, 5) and (label[1] == 0).all()


def test_edge_keys_are_symmetric_and_round_trip():
    big = 2 ** 31 - 1
    for a, b in ((0, 0), (0, big), (big, big), (3, 2), (big, 0), (17, 17)):
        k = uref.edge_key(a, b)
        assert k == uref.edge_key(b, a) and 0 <= k < 2 ** 63
        assert uref.edge_ends(k).tolist() == [min(a, b), max(a, b)]
        kt = ex.edge_keys(torch.tensor(a), torch.tensor(b))
        assert int(kt) == int(k) == int(ex.edge_keys(torch.tensor(b, dtype=torch.int32), torch.tensor(a, dtype=torch.int32)))
        assert ex.edge_ends(kt).tolist() == [min(a, b), max(a, b)] and ex.edge_ends(kt).dtype == torch.int32
    assert ex.edge_ends(torch.tensor([-1])).tolist() == [[-1, -1]]
    # ascending keys order the edges by (lower end, higher end)
    assert uref.edge_key(1, big) < uref.edge_key(2, 2)


def test_node_totals_reference():
    unit = np.array([[3, 5, 9, -1], [0, 5, 40, -1]], np.int64)
    dd = np.array([[0.5, 0.5, 2.0, 9.0], [np.nan, 1.0, 7.0, 0.0]], np.float32)
    kg = np.zeros((2, 4), np.float32)
    flip = np.array([[1, 0, 1, 1], [1, 1, 1, 0]], np.uint8)
    present = np.array([[2, 1, 0, 3], [1, 4, 1, 0]], np.int32)
    t = uref.node_totals_add(uref.new_table(10), unit, dd, kg, flip, present, rows=[0, 1, 1, -1, 2])
    assert t.rows_present.tolist() == [0, 0, 0, 1, 0, 3, 0, 0, 0, 0] and t.members[[3, 5]].tolist() == [2, 9]
    assert t.flips[[3, 5]].tolist() == [1, 2] and t.top[[3, 5]].tolist() == [1, 2] and t.top.sum() == 3      # (key 40 is outside)


def test_value_errors_name_the_limit():
    with pytest.raises(ValueError, match="W \\* M <= 1024"):
        ex.units_per_member("node", 65, 16)
    with pytest.raises(ValueError, match="W \\* M <= 1024"):
        pathnet_amd.explain_units(torch.zeros((2, 257, 4), dtype=torch.int32), "node")
    assert ex.units_per_member("node", 64, 16) == 16 and ex.units_per_member("edge", 1024, 2) == 1
    with pytest.raises(ValueError, match="L <= 16"):
        pathnet_amd.explain_units(torch.zeros((2, 3, 17), dtype=torch.int32), "node")
    with pytest.raises(ValueError, match="2 <= L"):
        pathnet_amd.explain_units(torch.zeros((2, 3, 1), dtype=torch.int32), "edge")
    with pytest.raises(ValueError, match="exclude"):
        pathnet_amd.explain_units(torch.zeros((2, 3, 4), dtype=torch.int32), "edge", exclude=torch.zeros(2))
    with pytest.raises(ValueError, match="'node' or 'edge'"):
        pathnet_amd.explain_units(torch.zeros((2, 3, 4), dtype=torch.int32), "path")
    d = {k: torch.as_tensor(v) for k, v in tiny().items()}
    args = (d["state"], d["coef"], d["ego"], d["fc2_w"], d["fc2_b"])
    with pytest.raises(ValueError, match="M <= 16"):
        pathnet_amd.explain_overlap(*args, torch.zeros((4, 6, 17), dtype=torch.int32), 4)
    wrong = ex.Totals(4, device="cpu")
    with pytest.raises(ValueError, match="NodeTotals"):
        pathnet_amd.explain_overlap(*args, torch.zeros((4, 6, 2), dtype=torch.int32), 4, totals=wrong,
                                    unit=torch.zeros((4, 4), dtype=torch.int64))
    with pytest.raises(ValueError, match="NodeTotals"):
        pathnet_amd.explain_overlap(*args, torch.zeros((4, 6, 2), dtype=torch.int32), 4, totals=pathnet_amd.NodeTotals(9, "cpu"))
    with pytest.raises(ValueError):
        pathnet_amd.NodeTotals(9, "cpu", state=torch.zeros((3, 9), dtype=torch.int64))
    with pytest.raises(RuntimeError, match="GPU only"):           # the limits hold: then the device is looked at
        pathnet_amd.explain_units(torch.zeros((2, 3, 4), dtype=torch.int32), "node")


def test_explanation_keeps_its_ten_fields():
    e = pathnet_amd.Explanation(*range(10))
    assert len(e) == 10 and e.unit is None and e.unit_count is None and e.totals == 9
    a, b, c, d, f, g, h, i, j, k = e
    e2 = pathnet_amd.Explanation(*range(10), "u", "n")
    assert len(e2) == 10 and e2.unit == "u" and e2.unit_count == "n"
    e3 = pathnet_amd.Explanation(*range(10), unit="u")._replace(logits=5)
    assert e3.logits == 5 and e3.unit == "u" and e3.unit_count is None
    with pytest.raises(ValueError):
        e.units()


C_TYPES = {"int64_t": ctypes.c_int64, "int32_t": ctypes.c_int32}


def declared(name):
    txt = open(os.path.join(ROOT, "include", "pathnet_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    m = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % name, txt, flags=re.S)
    assert m, name
    out = []
    for arg in m.group(1).split(","):
        arg = " ".join(arg.split())
        if "*" in arg:
            out.append(ctypes.POINTER(_lib.ExplainOut) if "pn_explain_out" in arg else ctypes.c_void_p)
        else:
            out.append(C_TYPES[arg.replace("const ", "").split()[0]])
    return out


@pytest.mark.parametrize("name", ["pn_explain_units", "pn_explain_overlap", "pn_explain_node_totals", "pn_explain_groups"])
def test_header_declarations_match_the_bindings(name):
    res, args = _lib.SIGNATURES[name]
    assert res is ctypes.c_int and args == declared(name), name
    assert hasattr(_lib.load(), name)
    txt = open(os.path.join(ROOT, "include", "pathnet_hip.h")).read()
    assert re.search(r"#define PN_UNIT_NODE 0\b", txt) and re.search(r"#define PN_UNIT_EDGE 1\b", txt)
    assert (_lib.UNIT_NODE, _lib.UNIT_EDGE) == (0, 1) and _lib.load().pn_abi_version() == 12
