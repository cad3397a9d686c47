"""The seed tests/test_gpu_predict.py compares K-sample ensembles on, checked on the CPU with the oracle: under 5 % of the
rows may sit inside the label margin (tests/predict_cases.py), else "labels equal outside the margin" would say little."""
import numpy as np
import pytest

import predict_cases as pc


@pytest.mark.parametrize("variant", ["homo", "pagg", "hetero"])
@pytest.mark.parametrize("H", [32, 100])
def test_chosen_seed_leaves_few_rows_inside_the_margin(variant, H):
    m, X, sel = pc.model(variant, H), pc.features(), pc.node_list()
    logits = np.stack([pc.oracle_logits(variant, m, X, *pc.cpu_draw(k), sel) for k in range(pc.K)])
    assert logits.shape == (pc.K, pc.S, pc.C) and np.isfinite(logits).all()
    res, st = pc.ensemble_of(logits)
    close = pc.inside_margin(res.prob)
    assert close.mean() < 0.05, "%d of %d rows inside the margin" % (close.sum(), len(close))
    # the draws differ: the ensemble has something to average (and for the classes whose rows pool their own paths the
    # samples' votes differ on some row)
    assert (res.mutual_info > 0).any()
    assert variant == "hetero" or (st.votes.max(axis=1) < pc.K).any()
    assert variant == "hetero" or len(set(res.label.tolist())) > 1
