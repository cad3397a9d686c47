"""Generate tests/golden/census_*.npz by running the UNMODIFIED synthetic-label programs
(/root/reference/synthetic_data/gen_cora_syn.cpp, gen_citeseer_syn.cpp), compiled into a temporary directory.
Run in the build container only:  python tests/golden/make_golden_census.py

The programs read ../preprocess/<name>.in (a header "n m" and m pairs) and write <name>_label.out.  The reference ships
no such file; its pairs are the first two columns of the shipped edge_input/cora_nsl.in and edge_input/citeseer.in.  The
third golden is a small graph with what the list build treats specially -- rows u == u (two entries), repeated rows (kept),
isolated nodes, an odd n -- written under the name the Cora program expects.
Every file carries its own input rows: n, u, v (int32) and the labels exactly as printed.
"""
import os
import subprocess
import tempfile
import time

import numpy as np

REF = "/root/reference"
OUT = os.path.dirname(os.path.abspath(__file__))


def pairs_of(edge_file):
    with open(edge_file) as f:
        n, m = map(int, f.readline().split()[:2])
        rows = np.array([ln.split()[:2] for ln in f.read().strip().split("\n")], dtype=np.int64)
    assert rows.shape == (m, 2), (rows.shape, m)
    return n, rows[:, 0].astype(np.int32), rows[:, 1].astype(np.int32)


def small_graph(n=101, m=260, seed=7):
    rng = np.random.default_rng(seed)
    live = n - 6                                                     # the last six nodes stay isolated
    u, v = rng.integers(0, live, m), rng.integers(0, live, m)
    u[:8] = v[:8] = rng.integers(0, live, 8)                         # rows u == u
    u, v = np.concatenate([u, u[20:50], v[60:70]]), np.concatenate([v, v[20:50], u[60:70]])     # repeats, both ways round
    return n, u.astype(np.int32), v.astype(np.int32)


def run(tmp, program, name, n, u, v):
    with open(os.path.join(tmp, "preprocess", name + ".in"), "w") as f:
        f.write("%d %d\n" % (n, len(u)))
        f.write("".join("%d %d\n" % (a, b) for a, b in zip(u, v)))
    t0 = time.perf_counter()
    subprocess.run([os.path.join(tmp, program)], cwd=os.path.join(tmp, "synthetic_data"), check=True)
    dt = time.perf_counter() - t0
    with open(os.path.join(tmp, "synthetic_data", name + "_label.out")) as f:
        labels = np.array(f.read().split(), dtype=np.int64)
    assert labels.shape == (n,)
    return labels, dt


def save(tag, n, u, v, labels):
    np.savez_compressed(os.path.join(OUT, "census_%s.npz" % tag), n=np.int32(n), u=u, v=v, labels=labels)
    print(tag, "n", n, "rows", len(u), "labels", np.bincount(labels, minlength=8).tolist())


if __name__ == "__main__":
    with tempfile.TemporaryDirectory() as tmp:
        os.makedirs(os.path.join(tmp, "preprocess"))
        os.makedirs(os.path.join(tmp, "synthetic_data"))
        for prog in ("gen_cora_syn", "gen_citeseer_syn"):
            subprocess.run(["g++", "-O2", "-w", "-o", os.path.join(tmp, prog),
                            os.path.join(REF, "synthetic_data", prog + ".cpp")], check=True)
        n, u, v = small_graph()
        save("small", n, u, v, run(tmp, "gen_cora_syn", "cora", n, u, v)[0])
        n, u, v = pairs_of(os.path.join(REF, "edge_input", "cora_nsl.in"))
        labels, dt = run(tmp, "gen_cora_syn", "cora", n, u, v)
        save("cora", n, u, v, labels)
        print("gen_cora_syn wall time %.3f s (file IO included)" % dt)
        n, u, v = pairs_of(os.path.join(REF, "edge_input", "citeseer.in"))
        save("citeseer", n, u, v, run(tmp, "gen_citeseer_syn", "citeseer", n, u, v)[0])
