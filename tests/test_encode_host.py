"""encode(): the C ABI and module surface that carry the aggregators' embeddings and path weights (no GPU needed)."""
import ctypes
import os
import re

from pathnet_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_pagg_args_end_with_the_encode_fields():
    names = [f[0] for f in _lib.PaggArgs._fields_]
    assert _lib.ABI_VERSION == 12
    assert names[names.index("step_state") + 1:] == ["out_embed", "out_path_weight", "out_path_state", "g_embed"]
    assert all(t is ctypes.c_void_p for n, t in _lib.PaggArgs._fields_[-4:])


def test_header_declares_the_same_fields_in_the_same_order():
    txt = open(os.path.join(ROOT, "include", "pathnet_hip.h")).read()
    body = txt[txt.index("typedef struct pn_pagg_args"):txt.index("} pn_pagg_args;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    tail = body[body.index("*step_state;"):]
    assert re.findall(r"\*\s*(\w+);", tail) == ["step_state", "out_embed", "out_path_weight", "out_path_state", "g_embed"]


def test_every_module_class_has_encode():
    import inspect

    import pathnet_amd
    from pathnet_amd import modules
    for cls in (pathnet_amd.PathNet, pathnet_amd.PathNet_homo, pathnet_amd.PAGG):
        assert callable(getattr(cls, "encode", None)), cls
        sig = inspect.signature(cls.encode)
        for k in ("path_state", "group_slice", "reuse_tables", "seed"):
            assert sig.parameters[k].kind is inspect.Parameter.KEYWORD_ONLY, k
    assert modules.Encoded._fields == ("logits", "embedding", "path_weight", "path_state")


def test_fused_step_refuses_the_encode_fields():
    """pn_pagg_train_step returns PN_ERR_ARG for out_* / g_embed before it looks at the device"""
    lib = _lib.load()
    for k in ("out_embed", "out_path_weight", "out_path_state", "g_embed"):
        a = _lib.PaggArgs()
        setattr(a, k, 256)
        assert lib.pn_pagg_train_step(None, ctypes.byref(a), None, 1.0, None, None) == _lib.PN_ERR_ARG, k
        assert k in lib.pn_last_error().decode()
