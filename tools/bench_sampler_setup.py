#!/usr/bin/env python
"""Set-up of the sampler (gen_merw.cpp:162-179: edge file -> per-node lists -> alias tables -> bfs/dis).

    python tools/bench_sampler_setup.py [n_nodes=19717] [L=4] [dense|otf]
        the host builders timed stage by stage on the CPU (no GPU needed)
    python tools/bench_sampler_setup.py [n_nodes] [L] [dense|otf] --build host|device|both [--repeats 3]
        MerwSampler(..., build=...) on the GPU from the Erdos-Renyi rows in memory: wall clock of the whole set-up
        (tables + upload, or upload + device build) ending in torch.cuda.synchronize(), after one warm-up build of each
        kind on a small graph (code-object load excluded); prints one JSON line with host_sampler_tables_s and / or
        device_sampler_tables_s (median) and their spread
"""
import json
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import merw  # noqa: E402  (edge-file writer only)
from pathnet_amd import sampler  # noqa: E402
from tools.bench_sampler_large import er_graph  # noqa: E402


def host_stages(n, L, mode):
    g = er_graph(n, 16, 0)
    d = tempfile.mkdtemp(prefix="pn_setup_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    f = os.path.join(d, "g.in")
    try:
        merw.write_edge_file(f, *g)
        t = [time.perf_counter()]
        n2, u, v, p = sampler.read_edge_file(f)
        t.append(time.perf_counter())
        sampler.build_alias(n2, u, v, p)
        t.append(time.perf_counter())
        if mode == "dense":
            sampler.hops_dense(n2, u, v, L)
        else:
            sampler.csr_build(n2, u, v)
            sampler.csr_build(n2, u, v, reverse=True)
        t.append(time.perf_counter())
        print("n=%d rows=%d L=%d file %.1f MB, PN_HOST_THREADS=%s" % (n2, len(u), L, os.path.getsize(f) / 1e6,
                                                                   os.environ.get("PN_HOST_THREADS", "(auto)")))
        print("edge file read  %.3f s (%.1f M rows/s)" % (t[1] - t[0], len(u) / (t[1] - t[0]) / 1e6))
        print("alias tables    %.3f s" % (t[2] - t[1]))
        print("%-15s %.3f s" % ("hop table" if mode == "dense" else "CSR fwd + rev", t[3] - t[2]))
    finally:
        if os.path.exists(f):
            os.remove(f)
        os.rmdir(d)


def timed_builds(n, L, mode, builds, repeats):
    import torch
    small = er_graph(1000, 16, 1)
    for b in builds:                                # warm-up: code objects, allocator, host thread pool
        sampler.MerwSampler(*small, L, hops=mode, build=b)
    torch.cuda.synchronize()
    g = er_graph(n, 16, 0)
    rec = {"n": n, "rows": len(g[1]), "L": L, "hops": mode, "repeats": repeats}
    for b in builds:
        ts = []
        for _ in range(repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            smp = sampler.MerwSampler(*g, L, hops=mode, build=b)
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
            del smp
        ts.sort()
        rec["%s_sampler_tables_s" % b] = round(ts[len(ts) // 2], 4)
        rec["%s_sampler_tables_s_all" % b] = [round(t, 4) for t in ts]
    return rec


def main():
    argv = list(sys.argv[1:])
    builds, repeats = None, 3
    if "--build" in argv:
        i = argv.index("--build")
        builds = ["host", "device"] if argv[i + 1] == "both" else [argv[i + 1]]
        del argv[i:i + 2]
    if "--repeats" in argv:
        i = argv.index("--repeats")
        repeats = int(argv[i + 1])
        del argv[i:i + 2]
    n = int(argv[0]) if len(argv) > 0 else 19717
    L = int(argv[1]) if len(argv) > 1 else 4
    mode = argv[2] if len(argv) > 2 else ("dense" if n <= 50000 else "otf")
    if builds is None:
        host_stages(n, L, mode)
    else:
        print(json.dumps(timed_builds(n, L, mode, builds, repeats)))


if __name__ == "__main__":
    main()
