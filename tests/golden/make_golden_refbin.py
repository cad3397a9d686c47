"""Generate tests/golden/refbin_*.npz and tests/golden/refclass_*.npz: what the reference itself produced for the cases
the tests used to recompute live (the unmodified programs under oracle/_ref, the reference classes ast-loaded by
tests/ref_extract.py, the shipped edge files and saved_models/cornell.pth), so that the suite needs neither.
Run in the build container only, after `make -C oracle`:  python tests/golden/make_golden_refbin.py

refbin_<tag>.npz    : W, L, seed, epochs and the reference program's output bytes ("text", uint8) -- or, where that
                      is megabytes, its md5 and length -- plus the raw bytes of a shipped edge file ("edge_file")
refclass_<v>.npz    : test_oracle_matches_reference_classes' inputs, every state_dict tensor ("param/<key>"), the
                      reference classes' eval() output ("out")
refmodel_cornell_pth.npz : the state_dict key -> shape map of saved_models/cornell.pth ("shape/<key>")
"""
import hashlib
import os
import sys
import tempfile
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import merw  # noqa: E402
from ref_extract import REF_ROOT, reference_classes  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
TMP = tempfile.mkdtemp(prefix="pn_golden_")


def golden(name):
    return dict(np.load(os.path.join(OUT, name)))


def text(b):
    return np.frombuffer(b, dtype=np.uint8)


def merw_case(tag, n, u, v, p, W, L, seed, epochs):
    """gen_merw on an edge list, the first `epochs` epochs of its output"""
    edge = os.path.join(TMP, tag + ".in")
    merw.write_edge_file(edge, n, u, v, p)
    nbytes = len(merw.format_text(*merw.sample_full(n, u, v, p, W, L, merw.DRAW_GLIBC, seed, epoch_count=epochs)))
    txt = merw.run_ref(edge, W, L, seed, max_bytes=nbytes)
    assert len(txt) == nbytes
    np.savez_compressed(os.path.join(OUT, "refbin_%s.npz" % tag), W=W, L=L, seed=seed, epochs=epochs, text=text(txt))
    print(tag, len(txt), "bytes")


def uniform_case(tag, n, u, v, W, L, seed, epochs):
    """gen (uniform walks) on a pair list, the first `epochs` epochs of its output"""
    pair = os.path.join(TMP, tag + "_nsl.in")
    merw.write_pair_file(pair, n, u, v)
    nbytes = len(merw.format_text(*merw.sample_uniform(n, u, v, W, L, merw.DRAW_GLIBC, seed, epoch_count=epochs)))
    txt = merw.run_ref_uniform(pair, W, L, seed, max_bytes=nbytes)
    assert len(txt) == nbytes
    np.savez_compressed(os.path.join(OUT, "refbin_%s.npz" % tag), W=W, L=L, seed=seed, epochs=epochs, text=text(txt))
    print(tag, len(txt), "bytes")


def shipped_case(name, W, L, seed, epochs):
    """gen_merw on a shipped edge file: the file itself and the md5 of the output's first `epochs` epochs"""
    f = os.path.join(REF_ROOT, "edge_input", name + ".in")
    n, u, v, p = merw.read_edge_file(f)
    nbytes = len(merw.format_text(*merw.sample_full(n, u, v, p, W, L, merw.DRAW_GLIBC, seed, epoch_count=epochs)))
    txt = merw.run_ref(f, W, L, seed, max_bytes=nbytes)
    assert len(txt) == nbytes
    with open(f, "rb") as fh:
        raw = fh.read()
    np.savez_compressed(os.path.join(OUT, "refbin_shipped_%s.npz" % name), W=W, L=L, seed=seed, epochs=epochs,
                        edge_file=text(raw), md5=hashlib.md5(txt).hexdigest(), nbytes=len(txt))
    print(name, len(txt), "bytes", hashlib.md5(txt).hexdigest())


def class_case(variant, cname):
    """the case of tests/test_oracle_pagg.py::test_oracle_matches_reference_classes, as it was run live"""
    cls = reference_classes(0.0)
    torch.manual_seed(3)
    rng = np.random.default_rng(3)
    N, F, H, C, W, L, S = 64, 21, 128, 6, 40, 4, 29
    model = cls[cname](F, H, C, L if variant != "pagg" else N)
    X = torch.rand(N, F)
    mask = np.zeros(N, bool)
    mask[rng.permutation(N)[:S]] = True
    ids = rng.integers(0, N, size=(S, W, L))
    ids[:, :, 0] = np.nonzero(mask)[0][:, None]
    codes = rng.integers(0, L, size=(S, W, L))
    model.eval()
    with torch.no_grad():
        out = model(X, torch.tensor(ids.reshape(S, W * L)), W, L, torch.tensor(mask), torch.tensor(codes),
                    torch.arange(S * W * L))
    d = dict(variant=variant, N=N, F=F, H=H, C=C, W=W, L=L, S=S, X=X.numpy(), ids=ids.astype(np.int32),
             codes=codes.astype(np.uint8), mask=mask, out=out.numpy())
    for k, v in model.state_dict().items():
        d["param/" + k] = v.numpy()
    np.savez_compressed(os.path.join(OUT, "refclass_%s.npz" % variant), **d)
    print(variant, "out absmax %.3f" % out.abs().max().item())


def cornell_pth():
    sd = torch.load(os.path.join(REF_ROOT, "saved_models", "cornell.pth"), map_location="cpu")
    np.savez_compressed(os.path.join(OUT, "refmodel_cornell_pth.npz"),
                        **{"shape/" + k: np.array(v.shape, dtype=np.int64) for k, v in sd.items()})
    print("cornell.pth", len(sd), "tensors")


if __name__ == "__main__":
    assert merw.have_ref() and os.path.exists(merw.REF_GEN), "build oracle/_ref first (make -C oracle)"
    warnings.filterwarnings("ignore")
    g = golden("sampler_synthetic97_12_5.npz")
    n, u, v, p = int(g["n"]), g["u"], g["v"], g["p"]
    merw_case("synthetic97_9_3", n, u, v, p, 9, 3, 77, 6)             # tests/test_oracle_sampler.py
    merw_case("synthetic97_6_4", n, u, v, p, 6, 4, 31337, 5)          # tests/test_gpu_sampler.py (the CLI)
    g = golden("uniform_ring37_5_4.npz")
    uniform_case("uniform_ring37_6_5", int(g["n"]), g["u"], g["v"], 6, 5, 4242, 4)   # tests/test_gpu_sampler.py
    rng = np.random.default_rng(77)                                    # tests/test_oracle_sampler.py's fresh graph
    n = 41
    u = np.concatenate([np.arange(n), rng.integers(0, n, 60)]).astype(np.int32)
    v = np.concatenate([(np.arange(n) + 1) % n, rng.integers(0, n, 60)]).astype(np.int32)
    uniform_case("uniform_fresh41_6_5", n, u, v, 6, 5, 31337, 2)
    for name in ("cora", "citeseer", "cora_nsl"):
        shipped_case(name, 40, 4, 5, 2)
    for variant, cname in (("hetero", "PathNet"), ("homo", "PathNet_homo"), ("pagg", "PAGG")):
        class_case(variant, cname)
    cornell_pth()
