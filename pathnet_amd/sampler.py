"""MERW path sampler: host set-up + GPU walker, and the gen_merw / gen_epoch_merw command line.

Mirrors /root/reference/preprocess/gen_merw.cpp: ``main`` (:125-213) becomes
``MerwSampler.from_edge_file(...)`` (parse :162-172, alias tables :174-176, hop table :178-179) and
``MerwSampler.sample(...)`` (walk loop :182-209) which runs on the GPU through libpathnet_hip.so.
``python -m pathnet_amd.sampler <data_name> <path_num> <path_length>`` keeps the reference CLI: reads
``../edge_input/<name>.in`` and writes ``./<name>_<W>_<L>_merw.txt`` (or one file per epoch with
``--per-epoch``, gen_epoch_merw.cpp:166-178), 1000 epochs.
"""
import collections
import ctypes
import sys
import time

import numpy as np
import torch

from . import _lib, pathfile

DRAW_GLIBC_REPLAY = _lib.DRAW_GLIBC_REPLAY
DRAW_PHILOX = _lib.DRAW_PHILOX


def read_edge_file(path):
    """-> (n, u int32[m], v int32[m], p float64[m]) in file order (gen_merw.cpp:162-172)."""
    lib = _lib.load()
    n, m = ctypes.c_int32(0), ctypes.c_int64(0)
    _lib.check(lib.pn_edges_read_text(str(path).encode(), ctypes.byref(n), ctypes.byref(m), None, None, None, 0))
    u = np.empty(m.value, np.int32)
    v = np.empty(m.value, np.int32)
    p = np.empty(m.value, np.float64)
    if m.value:
        _lib.check(lib.pn_edges_read_text(str(path).encode(), ctypes.byref(n), ctypes.byref(m),
                                          _lib.np_ptr(u, ctypes.c_int32), _lib.np_ptr(v, ctypes.c_int32),
                                          _lib.np_ptr(p, ctypes.c_double), m.value))
    return n.value, u, v, p


def read_pair_file(path):
    """-> (n, u int32[m], v int32[m]) in file order: the uniform sampler's 2-column input (gen.cpp:80-92)."""
    lib = _lib.load()
    n, m = ctypes.c_int32(0), ctypes.c_int64(0)
    _lib.check(lib.pn_pairs_read_text(str(path).encode(), ctypes.byref(n), ctypes.byref(m), None, None, 0))
    u = np.empty(m.value, np.int32)
    v = np.empty(m.value, np.int32)
    if m.value:
        _lib.check(lib.pn_pairs_read_text(str(path).encode(), ctypes.byref(n), ctypes.byref(m),
                                          _lib.np_ptr(u, ctypes.c_int32), _lib.np_ptr(v, ctypes.c_int32), m.value))
    return n.value, u, v


def build_uniform(n, u, v):
    """The graph gen.cpp:83-94 walks on -> off[int64 n+1], packed int32 [total*4] walker table, and the same graph as
    a directed edge list (src, nbr) for the hop table / CSR builders."""
    lib = _lib.load()
    u = np.ascontiguousarray(u, np.int32)
    v = np.ascontiguousarray(v, np.int32)
    total = ctypes.c_int64(0)
    args = (n, len(u), _lib.np_ptr(u, ctypes.c_int32), _lib.np_ptr(v, ctypes.c_int32))
    _lib.check(lib.pn_uniform_build(*args, None, None, None, None, 0, ctypes.byref(total)))
    t = max(total.value, 1)
    off = np.zeros(n + 1, np.int64)
    packed = np.zeros(t * 4, np.int32)
    src, nbr = np.zeros(t, np.int32), np.zeros(t, np.int32)
    _lib.check(lib.pn_uniform_build(*args, _lib.np_ptr(off, ctypes.c_int64), _lib.np_ptr(packed, ctypes.c_int32),
                                    _lib.np_ptr(src, ctypes.c_int32), _lib.np_ptr(nbr, ctypes.c_int32), total.value,
                                    ctypes.byref(total)))
    k = total.value
    return off, packed, src[:k], nbr[:k]


def build_alias(n, u, v, p):
    """AliasTable::init for every node (gen_merw.cpp:23-79) -> off[int64 n+1], A, B, S(float64), thr(uint32)."""
    lib = _lib.load()
    u = np.ascontiguousarray(u, np.int32)
    v = np.ascontiguousarray(v, np.int32)
    p = np.ascontiguousarray(p, np.float64)
    off = np.zeros(n + 1, np.int64)
    total = ctypes.c_int64(0)
    args = (n, len(u), _lib.np_ptr(u, ctypes.c_int32), _lib.np_ptr(v, ctypes.c_int32), _lib.np_ptr(p, ctypes.c_double),
            _lib.np_ptr(off, ctypes.c_int64))
    _lib.check(lib.pn_alias_build(*args, None, None, None, None, 0, ctypes.byref(total)))
    t = max(total.value, 1)
    A, B = np.empty(t, np.int32), np.empty(t, np.int32)
    S, thr = np.empty(t, np.float64), np.empty(t, np.uint32)
    _lib.check(lib.pn_alias_build(*args, _lib.np_ptr(A, ctypes.c_int32), _lib.np_ptr(B, ctypes.c_int32),
                                  _lib.np_ptr(S, ctypes.c_double), _lib.np_ptr(thr, ctypes.c_uint32), total.value,
                                  ctypes.byref(total)))
    k = total.value
    return off, A[:k], B[:k], S[:k], thr[:k]


def hops_dense(n, u, v, seq_len):
    """dis[n, n] uint8 = 1 + hops for nodes within seq_len-1 hops (bfs, gen_merw.cpp:101-123)."""
    u = np.ascontiguousarray(u, np.int32)
    v = np.ascontiguousarray(v, np.int32)
    dis = np.empty((n, n), np.uint8)
    _lib.check(_lib.load().pn_hops_dense(n, len(u), _lib.np_ptr(u, ctypes.c_int32), _lib.np_ptr(v, ctypes.c_int32),
                                         seq_len, _lib.np_ptr(dis, ctypes.c_uint8)))
    return dis


def csr_build(n, u, v, reverse=False):
    """Sorted duplicate-free neighbour lists: off int64 [n+1], adj int32 (out-neighbours, or in-neighbours)."""
    lib = _lib.load()
    u = np.ascontiguousarray(u, np.int32)
    v = np.ascontiguousarray(v, np.int32)
    off = np.zeros(n + 1, np.int64)
    cnt = ctypes.c_int64(0)
    args = (n, len(u), _lib.np_ptr(u, ctypes.c_int32), _lib.np_ptr(v, ctypes.c_int32), 1 if reverse else 0,
            _lib.np_ptr(off, ctypes.c_int64))
    _lib.check(lib.pn_csr_build(*args, None, 0, ctypes.byref(cnt)))
    adj = np.empty(max(cnt.value, 1), np.int32)
    _lib.check(lib.pn_csr_build(*args, _lib.np_ptr(adj, ctypes.c_int32), cnt.value, ctypes.byref(cnt)))
    return off, adj[:cnt.value]


def _cuda_device(device):
    dev = torch.device(device)
    if dev.type == "cuda" and dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    return dev


def _on_device(x, dtype, device):
    """x (NumPy array or tensor) as a contiguous `dtype` tensor on `device`; a dtype conversion runs there."""
    t = x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x))
    return t.to(device=device).to(dtype).contiguous()


def tables_workspace(n, m, device="cuda"):
    """A workspace for the device table builders (pn_tables_workspace_bytes(n, m) bytes, uint8 on `device`)."""
    need = ctypes.c_int64(0)
    _lib.check(_lib.load().pn_tables_workspace_bytes(int(n), int(m), ctypes.byref(need)))
    return torch.empty(need.value, dtype=torch.uint8, device=device)


def build_alias_device(n, u, v, p, device="cuda", split=False, workspace=None):
    """build_alias + pn_alias_pack + pn_node_ref_pack on the GPU (pn_alias_build_device), bit-identical.
    u / v / p: NumPy arrays or tensors (int32 / int32 / float64 on `device`; anything else is uploaded and converted).
    -> device tensors off int64 [n+1], packed int32 [max(total, 1) * 4] {A, B, thr, 0}, node_ref int32 [max(n, 1) * 2]
    (uint32 bits) and, with split=True, S float64 [total] (else None).  total = the number of rows."""
    dev = _cuda_device(device)
    with torch.cuda.device(dev):
        u, v, p = _on_device(u, torch.int32, dev), _on_device(v, torch.int32, dev), _on_device(p, torch.float64, dev)
        m = int(u.numel())
        if int(v.numel()) != m or int(p.numel()) != m:
            raise ValueError("build_alias_device: u, v and p must have the same length")
        ws = workspace if workspace is not None else tables_workspace(n, m, dev)
        off = torch.empty(int(n) + 1, dtype=torch.int64, device=dev)
        packed = torch.empty(max(m, 1) * 4, dtype=torch.int32, device=dev)
        node_ref = torch.empty(2 * max(int(n), 1), dtype=torch.int32, device=dev)
        S = torch.empty(max(m, 1), dtype=torch.float64, device=dev) if split else None
        total = ctypes.c_int64(0)
        _lib.check(_lib.load().pn_alias_build_device(int(n), m, _lib.ptr(u), _lib.ptr(v), _lib.ptr(p), _lib.ptr(off),
                                                     _lib.ptr(packed), _lib.ptr(node_ref), _lib.ptr(S), max(m, 1),
                                                     ctypes.byref(total), _lib.ptr(ws), ws.numel(), _lib.stream_ptr(dev)))
    return off, packed, node_ref, (S[:total.value] if split else None)


def csr_build_device(n, u, v, reverse=False, device="cuda", workspace=None):
    """csr_build on the GPU (pn_csr_build_device), bit-identical: device tensors off int64 [n+1], adj int32 [count].
    u / v as for build_alias_device."""
    dev = _cuda_device(device)
    with torch.cuda.device(dev):
        u, v = _on_device(u, torch.int32, dev), _on_device(v, torch.int32, dev)
        m = int(u.numel())
        if int(v.numel()) != m:
            raise ValueError("csr_build_device: u and v must have the same length")
        ws = workspace if workspace is not None else tables_workspace(n, m, dev)
        off = torch.empty(int(n) + 1, dtype=torch.int64, device=dev)
        adj = torch.empty(max(m, 1), dtype=torch.int32, device=dev)     # m bounds the count: one call, no sizing pass
        cnt = ctypes.c_int64(0)
        _lib.check(_lib.load().pn_csr_build_device(int(n), m, _lib.ptr(u), _lib.ptr(v), 1 if reverse else 0,
                                                   _lib.ptr(off), _lib.ptr(adj), max(m, 1), ctypes.byref(cnt),
                                                   _lib.ptr(ws), ws.numel(), _lib.stream_ptr(dev)))
    return off, adj[:cnt.value]


def hops_dense_device(n, off, adj, seq_len):
    """hops_dense on the GPU (pn_hops_dense_device) from the out-lists of csr_build_device: dis [n, n] uint8 on their
    device, the same values."""
    dev = off.device
    dis = torch.empty((int(n), int(n)), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().pn_hops_dense_device(int(n), _lib.ptr(off), _lib.ptr(adj), int(seq_len), _lib.ptr(dis),
                                                    _lib.stream_ptr(dev)))
    return dis


def glibc_draws(seed, first, count):
    out = np.empty(count, np.int32)
    _lib.check(_lib.load().pn_glibc_draws(seed & 0xFFFFFFFF, first, count, _lib.np_ptr(out, ctypes.c_int32)))
    return out


PathReport = collections.namedtuple("PathReport", ("out_of_range", "non_edges", "far", "first_bad"))


class _HopSource:
    """What the walker reads hop counts from -- the dense dis[n][n] table or the two CSR lists, on self.device -- and
    annotate(), which reads nothing else.  Needs self.n, self.L, self.device and the five d_* tensors (None when unused)."""

    DENSE_LIMIT_BYTES = 8 << 30     # hops="auto": dense n*n table up to 8 GB (n <= 92681), else on the fly
    # pn_path_codes' workspace.  A call without a report writes its counters there and nobody reads them, so calls on
    # several streams may share it; whoever starts reading counters from it needs one per stream.
    _codes_ws = None

    def annotate(self, ids, sources=None, *, report=False, check=False, out=None):
        """Distance codes for paths that did not come from sample() (pn_path_codes): another sampler's, an ids-only
        file's, or paths sampled before edges were hidden or added.
        ids: [S, W, L] or [E, S, W, L]; an int32 tensor on the device is read in place, anything else torch.as_tensor
        takes is narrowed to int32 and uploaded.  L <= the seq_len the tables were built for.
        sources: the node every row's hops are counted from, one per [W, L] block (shape ids.shape[:-2]); default: the
        row's first node ids[..., 0, 0].
        -> codes, a uint8 device tensor shaped like ids: min(hops(source -> node), L-1) over the directed edges of the
        graph; nodes further away, unreachable or outside [0, n) get L-1.
        report=True: -> (codes, PathReport(out_of_range, non_edges, far, first_bad)) -- ids outside the graph, steps that
        are no edge (staying in place is accepted), nodes beyond L-1 hops, flat index of the first id outside the graph
        or -1; costs one read-back.  check=True: IndexError naming first_bad when an id lies outside the graph.
        Without either flag nothing is read back: the call is enqueued on the current stream like sample().
        On the fly (hops="otf") a node that is not within two hops of its source is searched for over chains of
        in-neighbours up to L-1 long, without a visited set: many far or random targets in a graph with in-degrees of 16
        and more, at L near 8, make one launch long.  The dense table has no such case."""
        dev = self.device
        t = ids if isinstance(ids, torch.Tensor) else torch.as_tensor(ids)
        if t.dim() not in (3, 4):
            raise ValueError("annotate: ids of shape [S, W, L] or [E, S, W, L] expected, got %s" % (tuple(t.shape),))
        if t.dtype.is_floating_point or t.dtype.is_complex or t.dtype == torch.bool:
            raise TypeError("annotate: integer node ids expected, got %s" % t.dtype)
        if t.dtype != torch.int32:       # (a wider id cannot be a node: it stays out of range after the narrowing)
            t = t.clamp(-1, 2 ** 31 - 1).to(torch.int32)
        t = t.to(dev).contiguous()
        W, L = int(t.shape[-2]), int(t.shape[-1])
        rows = t.numel() // max(W * L, 1)
        if L < 1 or W < 1 or L > self.L:
            raise ValueError("annotate: paths of %d x %d nodes; the hop source was built for path lengths up to %d"
                             % (W, L, self.L))
        src = None
        if sources is not None:
            src = sources if isinstance(sources, torch.Tensor) else torch.as_tensor(sources)
            if src.numel() != rows:
                raise ValueError("annotate: %d sources for %d rows" % (src.numel(), rows))
            if src.dtype != torch.int32:
                src = src.clamp(-1, 2 ** 31 - 1).to(torch.int32)
            src = src.to(dev).contiguous()
        if out is None:
            codes = torch.empty(t.shape, dtype=torch.uint8, device=t.device)
        else:
            codes = out
            if (tuple(codes.shape) != tuple(t.shape) or codes.dtype != torch.uint8 or not codes.is_contiguous() or
                    codes.device != t.device):
                raise ValueError("annotate(out=...): contiguous uint8 tensor of shape %s on %s expected, got %s %s on %s"
                                 % (tuple(t.shape), t.device, codes.dtype, tuple(codes.shape), codes.device))
        lib = _lib.load()
        dp = lambda x: x.data_ptr() if x is not None else None      # noqa: E731
        tb = _lib.SamplerTables(self.n, 0, None, None, dp(self.d_dis), dp(self.d_adj_off), dp(self.d_adj),
                                dp(self.d_radj_off), dp(self.d_radj), 0, None)
        need = ctypes.c_int64(0)
        _lib.check(lib.pn_path_codes_workspace_bytes(ctypes.byref(tb), W, L, rows, ctypes.byref(need)))
        with torch.cuda.device(t.device):
            if self._codes_ws is None or self._codes_ws.numel() < need.value:
                self._codes_ws = torch.empty(max(need.value, 1), dtype=torch.uint8, device=t.device)
            rep = torch.empty(4, dtype=torch.int64, device=t.device) if (report or check) else None
            _lib.check(lib.pn_path_codes(_lib.context(t.device), ctypes.byref(tb), W, L, rows, _lib.ptr(t), _lib.ptr(src),
                                         _lib.ptr(codes), _lib.ptr(rep), _lib.ptr(self._codes_ws),
                                         self._codes_ws.numel(), _lib.stream_ptr(t.device)))
        if rep is None:
            return codes
        rep = PathReport(*rep.tolist())
        if check and rep.out_of_range > 0:
            raise IndexError("annotate: %d ids lie outside [0, %d); the first is element %d of the flattened ids"
                             % (rep.out_of_range, self.n, rep.first_bad))
        return (codes, rep) if report else codes

    def walk_stats(self, ids, codes, **kw):
        """walkstats.walk_stats(ids, codes, n=self.n, ...): statistics of sampled (or annotated) paths, counted on the
        device -> WalkStats."""
        from . import walkstats
        return walkstats.walk_stats(ids, codes, self.n, **kw)


class PathAnnotator(_HopSource):
    """The hop source of a graph without a sampler around it: annotate() for callers that bring their own paths and
    have no transition probabilities.  (u[i] -> v[i]) are the directed edges; hops / build as for MerwSampler."""

    def __init__(self, n, u, v, seq_len, device="cuda", hops="auto", build="host"):
        if build not in ("host", "device"):
            raise ValueError("build must be 'host' or 'device'")
        if hops not in ("dense", "otf", "auto"):
            raise ValueError("hops must be 'dense', 'otf' or 'auto'")
        self.n, self.L = int(n), int(seq_len)
        self.device = dev = _cuda_device(device)
        if hops == "auto":
            hops = "dense" if self.n * self.n <= self.DENSE_LIMIT_BYTES else "otf"
        self.hops = hops
        if hops == "otf" and seq_len > 8:
            raise ValueError("on-the-fly hop codes support path lengths up to 8")
        self.d_dis = self.d_adj_off = self.d_adj = self.d_radj_off = self.d_radj = None
        if build == "device":
            with torch.cuda.device(dev):
                u, v = _on_device(u, torch.int32, dev), _on_device(v, torch.int32, dev)
                ws = tables_workspace(n, u.numel(), dev)
                self.d_adj_off, self.d_adj = csr_build_device(n, u, v, False, dev, workspace=ws)
                if hops == "dense":
                    self.d_dis = hops_dense_device(n, self.d_adj_off, self.d_adj, seq_len)
                    self.d_adj_off = self.d_adj = None
                else:
                    self.d_radj_off, self.d_radj = csr_build_device(n, u, v, True, dev, workspace=ws)
        elif hops == "dense":
            self.d_dis = torch.from_numpy(hops_dense(n, u, v, seq_len)).to(dev)
        else:
            ao, aa = csr_build(n, u, v, reverse=False)
            ro, ra = csr_build(n, u, v, reverse=True)
            self.d_adj_off, self.d_adj = torch.from_numpy(ao).to(dev), torch.from_numpy(aa).to(dev)
            self.d_radj_off, self.d_radj = torch.from_numpy(ro).to(dev), torch.from_numpy(ra).to(dev)


class MerwSampler(_HopSource):
    """Device-resident sampler tables for one graph and one path length."""

    draws_per_step = 2              # the alias roll: slot draw + probability draw (gen_merw.cpp:81-91)

    def __init__(self, n, u, v, p, seq_len, device="cuda", hops="auto", build="host"):
        """hops: "dense" = the reference's dis[n][n] byte table in HBM; "otf" = exact hop codes derived on the
        fly from CSR lists (any n); "auto" picks dense while n*n <= DENSE_LIMIT_BYTES.
        build: "host" = the host builders, then one upload (self.host keeps their arrays); "device" = the same tables,
        bit-identical, built on `device` (pn_tables.hip) from the rows -- NumPy arrays (uploaded once) or device
        tensors -- and self.host is None."""
        if build not in ("host", "device"):
            raise ValueError("build must be 'host' or 'device'")
        if hops not in ("dense", "otf", "auto"):
            raise ValueError("hops must be 'dense', 'otf' or 'auto'")
        if build == "device":
            self._build_on_device(n, u, v, p, seq_len, device, hops)
            return
        off, A, B, S, thr = build_alias(n, u, v, p)
        self.host = dict(off=off, A=A, B=B, S=S, thr=thr)
        packed = np.empty(max(len(A), 1) * 4, np.int32)
        _lib.check(_lib.load().pn_alias_pack(len(A), _lib.np_ptr(A, ctypes.c_int32), _lib.np_ptr(B, ctypes.c_int32),
                                             _lib.np_ptr(thr, ctypes.c_uint32), _lib.np_ptr(packed, ctypes.c_int32)))
        self._upload(n, seq_len, device, hops, off, packed, len(A), u, v)

    def _place(self, n, seq_len, device, hops):
        self.n, self.L = int(n), int(seq_len)
        self.device = _cuda_device(device)
        if hops == "auto":
            hops = "dense" if self.n * self.n <= self.DENSE_LIMIT_BYTES else "otf"
        if hops not in ("dense", "otf"):
            raise ValueError("hops must be 'dense', 'otf' or 'auto'")
        self.hops = hops

    def _build_on_device(self, n, u, v, p, seq_len, device, hops):
        """build="device": the walker table, node_ref and the hop-code source, all built on self.device."""
        self._place(n, seq_len, device, hops)
        if self.hops == "otf" and seq_len > 8:
            raise ValueError("on-the-fly hop codes support path lengths up to 8")
        dev = self.device
        with torch.cuda.device(dev):
            u, v, p = _on_device(u, torch.int32, dev), _on_device(v, torch.int32, dev), _on_device(p, torch.float64, dev)
            ws = tables_workspace(n, u.numel(), dev)
            self.d_off, self.d_triples, self.d_node_ref, _ = build_alias_device(n, u, v, p, dev, workspace=ws)
            self.d_dis = self.d_adj_off = self.d_adj = self.d_radj_off = self.d_radj = None
            if self.hops == "dense":
                self.d_dis = hops_dense_device(n, *csr_build_device(n, u, v, False, dev, workspace=ws), seq_len)
            else:
                self.d_adj_off, self.d_adj = csr_build_device(n, u, v, False, dev, workspace=ws)
                self.d_radj_off, self.d_radj = csr_build_device(n, u, v, True, dev, workspace=ws)
            self._status = torch.zeros(1, dtype=torch.int32, device=dev)
        self.host = None
        self.total = int(u.numel())
        self._ws = None

    def _upload(self, n, seq_len, device, hops, off, packed, total, eu, ev):
        """Device copies of the walker table (off, packed) and of the hop-code source built from the directed edge
        list (eu -> ev): the dense table or the two CSR lists."""
        self._place(n, seq_len, device, hops)
        hops = self.hops
        self.d_off = torch.from_numpy(off).to(self.device)
        self.d_triples = torch.from_numpy(packed).to(self.device)
        self.d_node_ref = None
        if int(off[-1]) < 2 ** 32:          # {first triple, count} per node: one 8-byte load per roll
            ref = np.empty(2 * max(int(n), 1), np.uint32)
            _lib.check(_lib.load().pn_node_ref_pack(int(n), _lib.np_ptr(np.ascontiguousarray(off), ctypes.c_int64),
                                                    _lib.np_ptr(ref, ctypes.c_uint32)))
            self.d_node_ref = torch.from_numpy(ref.view(np.int32)).to(self.device)
        self.d_dis = self.d_adj_off = self.d_adj = self.d_radj_off = self.d_radj = None
        if hops == "dense":
            self.d_dis = torch.from_numpy(hops_dense(n, eu, ev, seq_len)).to(self.device)
        else:
            if seq_len > 8:
                raise ValueError("on-the-fly hop codes support path lengths up to 8")
            ao, aa = csr_build(n, eu, ev, reverse=False)
            ro, ra = csr_build(n, eu, ev, reverse=True)
            self.d_adj_off, self.d_adj = torch.from_numpy(ao).to(self.device), torch.from_numpy(aa).to(self.device)
            self.d_radj_off, self.d_radj = torch.from_numpy(ro).to(self.device), torch.from_numpy(ra).to(self.device)
        self.total = int(total)
        self._status = torch.zeros(1, dtype=torch.int32, device=self.device)
        self._ws = None

    @classmethod
    def from_edge_file(cls, path, seq_len, device="cuda", hops="auto", build="host"):
        n, u, v, p = read_edge_file(path)
        return cls(n, u, v, p, seq_len, device=device, hops=hops, build=build)

    def _window(self, W, epoch_count, node_begin, node_count, out, nodes):
        """-> node_begin, node_count and the two output tensors of a sample() call (checked `out`, or new ones)."""
        if nodes is not None:
            if nodes.dtype != torch.int32 or not nodes.is_cuda or not nodes.is_contiguous() or nodes.dim() != 1:
                raise ValueError("sample(nodes=...): contiguous 1-D int32 device tensor of node ids expected")
            node_begin, node_count = 0, int(nodes.numel())
        elif node_count is None:
            node_count = self.n - node_begin
        shape = (epoch_count, node_count, W, self.L)
        if out is None:
            ids = torch.empty(shape, dtype=torch.int32, device=self.device)
            codes = torch.empty(shape, dtype=torch.uint8, device=self.device)
        else:
            ids, codes = out
            for t, dt in ((ids, torch.int32), (codes, torch.uint8)):
                if (tuple(t.shape) != shape or t.dtype != dt or not t.is_contiguous() or t.device.type != "cuda" or
                        (self.device.index is not None and t.device != self.device)):
                    raise ValueError("sample(out=...): contiguous %s tensor of shape %s on %s expected, got %s %s on %s"
                                     % (dt, shape, self.device, t.dtype, tuple(t.shape), t.device))
        return node_begin, node_count, ids, codes

    def _tables(self):
        dp = lambda t: t.data_ptr() if t is not None else None      # noqa: E731
        return _lib.SamplerTables(self.n, self.total, self.d_off.data_ptr(), self.d_triples.data_ptr(), dp(self.d_dis),
                                  dp(self.d_adj_off), dp(self.d_adj), dp(self.d_radj_off), dp(self.d_radj),
                                  self.draws_per_step, dp(self.d_node_ref))

    def biased(self, p, q):
        """A view of this sampler that walks with node2vec's return parameter p and in-out parameter q (BiasedSampler):
        same device tables, same sample() signature; p = inf is a non-backtracking walk."""
        return BiasedSampler(self, p, q)

    def path_prob(self, ids):
        """pathprob.path_prob(self, ids): the likelihood of the paths ids [..., W, L] under this sampler's own tables --
        exact transition numerators over 2^62, their fp64 probabilities and every path's log-likelihood -> PathProb."""
        from . import pathprob
        return pathprob.path_prob(self, ids)

    def sample(self, W, seed, epoch_begin=0, epoch_count=1, node_begin=0, node_count=None,
               draw_source=DRAW_PHILOX, check=True, out=None, step_state=None, nodes=None):
        """-> ids int32 [epoch_count, node_count, W, L], codes uint8 [...] on the GPU.
        nodes (int32 device tensor, Philox only): sample the paths of these source nodes (in this order) instead of the
        range [node_begin, node_begin + node_count) -- e.g. the step's masked nodes; a walk's draws depend on (epoch,
        source node, walk index) only, so the paths are the ones a full-epoch sample holds for those nodes.
        step_state (pathnet_amd.StepState, Philox only): seed and epoch_begin are read from device memory when the
        kernel runs, so the call can be captured in a hipGraph and replayed."""
        lib = _lib.load()
        node_begin, node_count, ids, codes = self._window(W, epoch_count, node_begin, node_count, out, nodes)
        L = self.L
        need = ctypes.c_int64(0)
        _lib.check(lib.pn_sample_workspace_bytes(W, L, draw_source, epoch_count, node_count, ctypes.byref(need)))
        tb = self._tables()
        dev = ids.device
        with torch.cuda.device(dev):        # the library launches on the current device
            if need.value and (self._ws is None or self._ws.numel() < need.value):
                self._ws = torch.empty(need.value, dtype=torch.uint8, device=dev)
            if check:
                self._status.zero_()
            _lib.check(lib.pn_sample_paths(_lib.context(dev), ctypes.byref(tb), W, L, draw_source,
                                           seed & 0xFFFFFFFFFFFFFFFF, epoch_begin, epoch_count, node_begin, node_count,
                                           _lib.ptr(ids), _lib.ptr(codes), _lib.ptr(self._ws) if need.value else None,
                                           need.value, _lib.ptr(self._status),
                                           step_state.ptr() if step_state is not None else None,
                                           _lib.ptr(nodes) if nodes is not None else None, _lib.stream_ptr(dev)))
        if check and int(self._status.item()) != 0:
            # the reference prints this and exits (gen_merw.cpp:84-87)
            raise _lib.PnError(int(self._status.item()), "ERROR:: A.size() == 0 in Alias Table")
        return ids, codes


class UniformSampler(MerwSampler):
    """The uniform random-walk sampler of the "RW-PathNet" ablation (preprocess/gen.cpp, gen_epoch.cpp): same walker
    and hop codes, but the graph is the symmetrised pair list with self loops (gen.cpp:83-94) and a step is ONE draw,
    ``E[u][rand() % deg]`` (gen.cpp:113-114).  ``sample()`` is MerwSampler's; glibc-replay draws are bit-exact to the
    reference binary."""

    draws_per_step = 1

    def __init__(self, n, u, v, seq_len, device="cuda", hops="auto"):
        off, packed, src, nbr = build_uniform(n, u, v)
        self.host = dict(off=off, nbr=nbr)
        self._upload(n, seq_len, device, hops, off, packed, len(nbr), src, nbr)

    @classmethod
    def from_pair_file(cls, path, seq_len, device="cuda", hops="auto"):
        n, u, v = read_pair_file(path)
        return cls(n, u, v, seq_len, device=device, hops=hops)


def bias_thresholds(p, q):
    """pn_bias_thresholds: the accept thresholds (T_return, T_near, T_far), integers in [0, 2^32], of a walk with return
    parameter p and in-out parameter q -- floor(2^32 * w / max(w)) for w = (1/p, 1, 1/q) in fp64.  No device needed."""
    thr = (ctypes.c_uint64 * 3)()
    rc = _lib.load().pn_bias_thresholds(float(p), float(q), thr)
    if rc == _lib.PN_ERR_ARG:
        raise ValueError("p and q must be > 0 (inf allowed), got p=%r q=%r" % (p, q))
    _lib.check(rc)
    return tuple(int(t) for t in thr)


class BiasedSampler:
    """sampler.biased(p, q): second-order walks over the tables of a MerwSampler / UniformSampler (pn_sample_paths_biased).
    Step t >= 1 at node cur, having come from prev, goes to x with probability ~ P_table(cur -> x) * a, a = 1/p for
    x == prev, 1 when prev -> x is an edge, 1/q otherwise; realised by rejection from the table with at most 64 trials a
    step (the 64th proposal is taken as it is and the step counted in exhausted_steps()), so the realised distribution
    differs from the target on at most that share of the steps, and p = inf at a leaf returns.
    A light view: it owns no tables, only the device counter.  Takes the place of the sampler wherever one is taken."""

    def __init__(self, base, p, q):
        self.base, self.p, self.q = base, float(p), float(q)
        self.thresholds = bias_thresholds(p, q)     # refuses bad p / q here, not at the first sample()
        self._exhausted = self._ws = None

    n = property(lambda self: self.base.n)
    L = property(lambda self: self.base.L)
    device = property(lambda self: self.base.device)

    def annotate(self, *args, **kw):
        return self.base.annotate(*args, **kw)

    def walk_stats(self, ids, codes, **kw):
        return self.base.walk_stats(ids, codes, **kw)

    def path_prob(self, ids, kind="realised"):
        """pathprob.biased_path_prob(self, ids, kind): the likelihood of the paths under this second-order walk --
        kind="realised": what sample() does, trial cap included; kind="target": the distribution it aims at -> PathProb
        with the class masses and classes beside the numerators."""
        from . import pathprob
        return pathprob.biased_path_prob(self, ids, kind)

    def exhausted_steps(self):
        """Steps of the latest sample() that came to their 64th trial (one read-back); 0 before the first call."""
        return 0 if self._exhausted is None else int(self._exhausted.item())

    def sample(self, W, seed, epoch_begin=0, epoch_count=1, node_begin=0, node_count=None,
               draw_source=DRAW_PHILOX, check=True, out=None, step_state=None, nodes=None):
        """MerwSampler.sample's signature and results; Philox draws only (trial j of a walk reads Philox block j)."""
        if draw_source != DRAW_PHILOX:
            raise ValueError("biased walks draw from Philox only (draw_source=DRAW_PHILOX)")
        base, lib = self.base, _lib.load()
        node_begin, node_count, ids, codes = base._window(W, epoch_count, node_begin, node_count, out, nodes)
        tb = base._tables()
        need = ctypes.c_int64(0)
        _lib.check(lib.pn_sample_paths_biased_workspace_bytes(ctypes.byref(tb), W, base.L, epoch_count, node_count,
                                                              ctypes.byref(need)))
        dev = ids.device
        with torch.cuda.device(dev):        # the library launches on the current device
            if need.value and (self._ws is None or self._ws.numel() < need.value):
                self._ws = torch.empty(need.value, dtype=torch.uint8, device=dev)
            if self._exhausted is None:
                self._exhausted = torch.zeros(1, dtype=torch.int64, device=dev)
            if check:
                base._status.zero_()
            _lib.check(lib.pn_sample_paths_biased(_lib.context(dev), ctypes.byref(tb), W, base.L,
                                                  seed & 0xFFFFFFFFFFFFFFFF, epoch_begin, epoch_count, node_begin,
                                                  node_count, self.p, self.q, _lib.ptr(ids), _lib.ptr(codes),
                                                  _lib.ptr(self._exhausted), _lib.ptr(self._ws) if need.value else None,
                                                  need.value, _lib.ptr(base._status),
                                                  step_state.ptr() if step_state is not None else None,
                                                  _lib.ptr(nodes) if nodes is not None else None, _lib.stream_ptr(dev)))
        if check and int(base._status.item()) != 0:
            raise _lib.PnError(int(base._status.item()), "ERROR:: A.size() == 0 in Alias Table")
        return ids, codes


def main(argv=None):
    """Drop-in for ./gen_merw and ./gen_epoch_merw (argv: <data_name> <path_num> <path_length>); with --uniform for
    ./gen and ./gen_epoch (the uniform random-walk sampler)."""
    argv = list(sys.argv[1:] if argv is None else argv)
    per_epoch = "--per-epoch" in argv
    uniform = "--uniform" in argv        # gen.cpp / gen_epoch.cpp instead of gen_merw.cpp / gen_epoch_merw.cpp
    binary = "--binary" in argv          # also write the PNPATHS1 sidecar(s) next to the text file(s)
    opts = {"--seed": None, "--epochs": "1000", "--draw": "glibc", "--in": None, "--out-root": "./", "--bias": None,
            "--marker": None}
    pos = []
    i = 0
    while i < len(argv):
        a = argv[i]
        if a in ("--per-epoch", "--binary", "--uniform"):
            i += 1
        elif a in opts:
            opts[a] = argv[i + 1]
            i += 2
        else:
            pos.append(a)
            i += 1
    if len(pos) != 3:
        print("ERROR: Incorrect number of parameters. ", file=sys.stderr)   # gen_merw.cpp:128-132
        return 0
    name, W, L = pos[0], int(pos[1]), int(pos[2])
    seed = int(opts["--seed"]) if opts["--seed"] is not None else int(time.time())  # srand(time(0)), :161
    epochs = int(opts["--epochs"])
    draw = DRAW_GLIBC_REPLAY if opts["--draw"] == "glibc" else DRAW_PHILOX
    root = opts["--out-root"]
    bias = None
    if opts["--bias"] is not None:      # --bias P,Q: second-order walks (BiasedSampler); inf is accepted
        if draw != DRAW_PHILOX:
            print("ERROR: --bias needs --draw philox (a biased walk has no glibc draw stream to replay)", file=sys.stderr)
            return 2
        bias = tuple(float(x) for x in opts["--bias"].split(","))
        if len(bias) != 2:
            print("ERROR: --bias P,Q expected", file=sys.stderr)
            return 2
    if uniform:
        # gen.cpp:50-68 reads <name>_nsl.in and writes <name>_<W>_<L>_nsl.txt; gen_epoch.cpp:50-56,:84-95 reads <name>.in
        # and writes <name>_<W>_<L>_<epoch>.txt
        edge = opts["--in"] or ("../edge_input/%s.in" % name if per_epoch else "../edge_input/%s_nsl.in" % name)
        whole = pathfile.whole_run_name(root, name, W, L, marker=opts["--marker"] or "nsl")
        if not per_epoch:
            print("File input: " + edge)                                     # gen.cpp:73-74
            print("File output: " + whole)
        n_, u_, v_ = read_pair_file(edge)
        smp = UniformSampler(n_, u_, v_, L)
        if per_epoch:
            print("%d %d" % (smp.n, len(u_)))                                # gen_epoch.cpp:64
        else:
            print(smp.n, file=sys.stderr)                                    # gen.cpp:81
    else:
        edge = opts["--in"] or "../edge_input/%s.in" % name
        smp = MerwSampler.from_edge_file(edge, L)
        print(name + ": " + str(smp.n), file=sys.stderr)                    # :164
        whole = pathfile.whole_run_name(root, name, W, L, marker=opts["--marker"] or "merw")
    if bias is not None:
        smp = smp.biased(*bias)
    chunk = max(1, min(epochs, (64 << 20) // max(1, smp.n * W * L * 5)))
    for e0 in range(0, epochs, chunk):
        ec = min(chunk, epochs - e0)
        try:
            ids, codes = smp.sample(W, seed, epoch_begin=e0, epoch_count=ec, draw_source=draw)
        except _lib.PnError as ex:
            if ex.code != _lib.PN_ERR_EMPTY_TABLE:
                raise
            print("ERROR:: A.size() == 0 in Alias Table", file=sys.stderr)      # gen_merw.cpp:84-87: message + exit(0)
            return 0
        ids, codes = ids.cpu().numpy(), codes.cpu().numpy()
        for k in range(ec):
            if per_epoch:
                fn = ("%s%s_%d_%d_%d.txt" % (root, name, W, L, e0 + k) if uniform       # gen_epoch.cpp:84-95: no marker
                      else pathfile.per_epoch_name(root, name, W, L, e0 + k, marker=opts["--marker"] or "merw"))
                pathfile.write_paths(fn, ids[k], codes[k])
                if binary:
                    pathfile.write_paths_binary(fn[:-4] + ".bin", ids[k], codes[k])
            else:
                pathfile.write_paths(whole, ids[k], codes[k], append=(e0 + k) > 0)
        if binary and not per_epoch:
            if epochs > chunk:
                raise SystemExit("--binary without --per-epoch needs the whole run in one chunk; use --per-epoch")
            pathfile.write_paths_binary(whole[:-4] + ".bin", ids, codes)
    return 0


if __name__ == "__main__":
    sys.exit(main())
