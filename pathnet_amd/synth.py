"""Path-pattern census: the labels of the paper's synthetic experiment, on the GPU.

Mirrors the reference's synthetic_data/gen_cora_syn.cpp and gen_citeseer_syn.cpp: the pair file becomes undirected
multiset neighbour lists (:25-30), every walk of ``walk_len`` steps from a node is binned by the symbols of the nodes it
visits (:9-18, symbol = node id & 1) and the node's label is its most frequent bin, the lowest on ties (:36-43).  The
reference enumerates the walks one by one; ``PatternCensus`` runs the equivalent level-by-level recurrence through
libpathnet_hip.so (pn_census.hip) with exact int64 counts.

``python -m pathnet_amd.synth <name> [--walk-len 3]``, run from a directory beside ``preprocess/`` as the reference
programs are, reads ``../preprocess/<name>.in`` and writes ``./<name>_label.out``.
"""
import ctypes
import sys

import torch

from . import _lib
from .sampler import _cuda_device, _on_device, read_pair_file

USAGE = "usage: python -m pathnet_amd.synth <data_name> [--walk-len K]"


def check_limits(walk_len, num_symbols, max_list=0):
    """ValueError unless 1 <= walk_len, 2 <= num_symbols <= 16, num_symbols ** walk_len <= 1024 (the kernel's limits) and
    max_list ** walk_len < 2**63 (no count can leave int64)."""
    k, B = int(walk_len), int(num_symbols)
    if k < 1:
        raise ValueError("walk_len = %d, need at least 1" % k)
    if not 2 <= B <= 16:
        raise ValueError("num_symbols = %d, need 2..16" % B)
    if B ** k > 1024:
        raise ValueError("%d symbols over %d steps are %d patterns, more than 1024" % (B, k, B ** k))
    if int(max_list) ** k >= 2 ** 63:
        raise ValueError("a list of %d entries walked %d steps can exceed the int64 counts" % (max_list, k))


class PatternCensus:
    """The graph of a pair file as the reference walks it, resident on the GPU: every row (u, v) puts v into u's list and
    u into v's, duplicated rows stay (a multigraph) and a row u == v adds two entries to that node's list."""

    def __init__(self, n, u, v, device="cuda"):
        """u / v: the rows, NumPy arrays (uploaded once) or tensors on `device`.  ValueError for ids outside [0, n)."""
        self.n = int(n)
        self.device = dev = _cuda_device(device)
        if dev.type != "cuda":
            raise RuntimeError("pathnet_amd.synth: GPU only (device %s); there is no CPU fallback" % dev)
        if self.n < 0:
            raise ValueError("PatternCensus: n = %d" % self.n)
        lib = _lib.load()
        with torch.cuda.device(dev):
            u, v = _on_device(u, torch.int32, dev), _on_device(v, torch.int32, dev)
            m = int(u.numel())
            if int(v.numel()) != m:
                raise ValueError("PatternCensus: u and v must have the same length")
            need = ctypes.c_int64(0)
            _lib.check(lib.pn_census_lists_workspace_bytes(self.n, m, ctypes.byref(need)))
            ws = torch.empty(need.value, dtype=torch.uint8, device=dev)
            self.d_off = torch.empty(self.n + 1, dtype=torch.int64, device=dev)
            self.d_adj = torch.empty(max(2 * m, 1), dtype=torch.int32, device=dev)
            try:
                _lib.check(lib.pn_census_lists(_lib.context(dev), self.n, m, _lib.ptr(u), _lib.ptr(v), _lib.ptr(self.d_off),
                                               _lib.ptr(self.d_adj), _lib.ptr(ws), ws.numel(), _lib.stream_ptr(dev)))
            except _lib.PnError as ex:
                if ex.code != _lib.PN_ERR_ARG:
                    raise
                raise ValueError(str(ex)) from None
            self.entries = 2 * m
            self.max_list = int((self.d_off[1:] - self.d_off[:-1]).max().item()) if self.n > 0 else 0

    @classmethod
    def from_pair_file(cls, path, device="cuda"):
        n, u, v = read_pair_file(path)
        return cls(n, u, v, device=device)

    def fits_int32(self, walk_len=3):
        """max_list ** walk_len < 2**31: no count can reach 2**31, so the reference's int counters do not wrap."""
        return self.max_list ** int(walk_len) < 2 ** 31

    def _run(self, walk_len, symbols, num_symbols, want_counts, want_labels):
        k, B, dev = int(walk_len), int(num_symbols), self.device
        check_limits(k, B, self.max_list)
        if self.n == 0:
            return (torch.empty((0, B ** k), dtype=torch.int64, device=dev) if want_counts else None,
                    torch.empty(0, dtype=torch.int64, device=dev) if want_labels else None)
        with torch.cuda.device(dev):
            sym = None
            if symbols is not None:
                t = symbols if isinstance(symbols, torch.Tensor) else torch.as_tensor(symbols)
                if t.dtype.is_floating_point or t.dtype.is_complex or t.dtype == torch.bool:
                    raise TypeError("symbols: an integer tensor expected, got %s" % t.dtype)
                if t.dim() != 1 or t.numel() != self.n:
                    raise ValueError("symbols: %d values expected, got shape %s" % (self.n, tuple(t.shape)))
                t = t.to(dev)
                if self.n > 0 and (int(t.min()) < 0 or int(t.max()) >= B):
                    raise ValueError("symbols must lie in [0, %d)" % B)
                sym = t.to(torch.uint8).contiguous()
            need = ctypes.c_int64(0)
            lib = _lib.load()
            _lib.check(lib.pn_pattern_census_workspace_bytes(self.n, B, k, ctypes.byref(need)))
            # (a fresh workspace per call: the allocator hands a block back in the order of the stream that used it, so
            # calls on different streams never share level tables)
            ws = torch.empty(need.value, dtype=torch.uint8, device=dev)
            counts = torch.empty((self.n, B ** k), dtype=torch.int64, device=dev) if want_counts else None
            labels = torch.empty(self.n, dtype=torch.int64, device=dev) if want_labels else None
            _lib.check(lib.pn_pattern_census(_lib.context(dev), self.n, _lib.ptr(self.d_off), _lib.ptr(self.d_adj),
                                             _lib.ptr(sym), B, k, _lib.ptr(counts), _lib.ptr(labels), _lib.ptr(ws),
                                             ws.numel(), _lib.stream_ptr(dev)))
        return counts, labels

    def counts(self, walk_len=3, symbols=None, num_symbols=2):
        """-> int64 [n, B**k] on the GPU: counts[i, p] = the walks of `walk_len` steps from i, along list entries and with
        their multiplicity, whose pattern sum_j s[v_j] * B**(k-j) is p (first step most significant).  symbols: uint8 or
        int tensor / array [n] with values in [0, num_symbols); None = node id & 1, the reference's features.
        Enqueued on the current stream; nothing is read back (a given `symbols` is range-checked, which reads back)."""
        return self._run(walk_len, symbols, num_symbols, True, False)[0]

    def labels(self, walk_len=3, symbols=None, num_symbols=2):
        """-> int64 [n]: the smallest pattern among those with the largest count (an isolated node gets 0).  The count
        table of the last level is not materialised."""
        return self._run(walk_len, symbols, num_symbols, False, True)[1]


def main(argv=None):
    """Drop-in for ./gen_cora_syn and ./gen_citeseer_syn: <name> selects ../preprocess/<name>.in -> ./<name>_label.out."""
    argv = list(sys.argv[1:] if argv is None else argv)
    walk_len, pos, i = 3, [], 0
    while i < len(argv):
        if argv[i] == "--walk-len" and i + 1 < len(argv):
            walk_len = int(argv[i + 1])
            i += 2
        else:
            pos.append(argv[i])
            i += 1
    if len(pos) != 1 or pos[0].startswith("-"):
        print(USAGE, file=sys.stderr)
        return 2
    name = pos[0]
    cen = PatternCensus.from_pair_file("../preprocess/%s.in" % name)
    labels = cen.labels(walk_len=walk_len).cpu().numpy()
    with open("%s_label.out" % name, "w") as f:                      # printf("%d\n", o), :42
        f.write("".join("%d\n" % x for x in labels))
    return 0


if __name__ == "__main__":
    sys.exit(main())
