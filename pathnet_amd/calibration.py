"""Calibrated ensemble predictions (pn_calib_sweep / pn_calib_stats, pn_calib.hip; pn_ensemble_add_scaled).

``fit_temperature`` fits one temperature on validation logits by a grid sweep on the device, ``model.calibrate`` collects
those logits with the forwards ``model.predict`` would run, ``Ensemble(temperature=)`` / ``predict(temperature=)`` apply the
fitted value without reading it back, and ``Prediction.calibration(labels)`` measures the result: reliability bins, ECE,
MCE, NLL, Brier score and the risk-coverage curve.  Everything is a device tensor until ``summary()``.
"""
import collections
import ctypes

import numpy as np
import torch

from . import _lib

DEFAULT_GRID = tuple(2.0 ** (k / 4.0) for k in range(-12, 13))      # 25 points, 1/8 .. 8
REFINE_POINTS = 17
MAX_GRID = 256


class Temperature(collections.namedtuple("Temperature", ("tau", "best", "temps", "nll", "counts"))):
    """Device tensors of the last sweep:
    tau float64 [1]      the grid member with the lowest summed NLL (1.0 when nothing could be fitted)
    best int32 [1]       its position in temps, -1 when no row was used or no NLL is finite
    temps float64 [T]    the grid swept
    nll float64 [T]      summed NLL of the used rows at every grid point (+inf at a refused temperature)
    counts int64 [3]     {rows used, labels outside [0, C), rows without a finite sample}"""
    __slots__ = ()

    def summary(self):
        """A dict of Python numbers (the one host read)"""
        flat = torch.cat((self.tau, self.best.double(), self.counts.double(), self.temps, self.nll)).cpu().numpy()
        T = self.temps.numel()
        best, used = int(flat[1]), int(flat[2])
        nll = flat[5 + T:5 + 2 * T]
        return dict(tau=float(flat[0]), best=best, rows_used=used, labels_out_of_range=int(flat[3]),
                    rows_without_sample=int(flat[4]), grid=flat[5:5 + T].tolist(), nll=nll.tolist(),
                    mean_nll=float(nll[best] / used) if best >= 0 and used else float("nan"))


def _sweep(x, target, temps):
    dev = x.device
    R, S, C = (int(v) for v in x.shape)
    T = int(temps.numel())
    lib = _lib.load()
    need = ctypes.c_int64(0)
    _lib.check(lib.pn_calib_sweep_workspace_bytes(S, T, ctypes.byref(need)))
    ws = torch.empty(max(need.value, 8), dtype=torch.uint8, device=dev)
    nll = torch.empty(T, dtype=torch.float64, device=dev)
    tau = torch.empty(1, dtype=torch.float64, device=dev)
    best = torch.empty(1, dtype=torch.int32, device=dev)
    counts = torch.empty(3, dtype=torch.int64, device=dev)
    out = _lib.CalibSweepOut(nll.data_ptr(), best.data_ptr(), tau.data_ptr(), counts.data_ptr())
    _lib.check(lib.pn_calib_sweep(_lib.context(dev), _lib.ptr(x), R, S, C, _lib.ptr(target), _lib.ptr(temps), T, _lib.ptr(ws),
                                  ws.numel(), ctypes.byref(out), _lib.stream_ptr(dev)))
    return Temperature(tau, best, temps, nll, counts)


def fit_temperature(logits, labels, grid=None, rounds=2):
    """Fit one temperature to ``logits`` [K, S, C] (or [S, C]; fp32, on the GPU) and ``labels`` [S] by minimising the NLL of the
    K-sample mean probability of the label over a grid -> ``Temperature``.

    grid: the temperatures of the first sweep (at most 256; default 25 points 2^(k/4), k = -12 .. 12).
    rounds: 2 sweeps a second grid of 17 geometric points between the best point's two neighbours (clamped at the ends of
    the grid), built on the device, so nothing is read back.  ``tau`` is always a member of the last grid swept."""
    x = logits.detach()
    if x.dim() == 2:
        x = x.unsqueeze(0)
    if x.dim() != 3:
        raise ValueError("fit_temperature: logits [S, C] or [K, S, C] expected, got %s" % (tuple(logits.shape),))
    if x.device.type != "cuda":
        raise RuntimeError("pathnet_amd.fit_temperature runs on the GPU only (logits on %s); no CPU fallback" % x.device)
    if int(rounds) not in (1, 2):
        raise ValueError("fit_temperature: rounds=%r, 1 or 2" % (rounds,))
    x = x.float().contiguous()
    dev, S = x.device, int(x.shape[1])
    target = torch.as_tensor(labels).reshape(-1).to(device=dev, dtype=torch.int64).contiguous()
    if target.numel() != S:
        raise ValueError("fit_temperature: %d labels for %d rows" % (target.numel(), S))
    if grid is None:
        grid = DEFAULT_GRID
    temps = torch.as_tensor(grid, dtype=torch.float64).reshape(-1).to(dev).contiguous()
    if not 1 <= temps.numel() <= MAX_GRID:
        raise ValueError("fit_temperature: a grid of %d temperatures, 1 .. %d" % (temps.numel(), MAX_GRID))
    with torch.cuda.device(dev):
        fit = _sweep(x, target, temps)
        if int(rounds) == 2 and temps.numel() > 1:
            T = temps.numel()
            at = fit.best.long().clamp(min=0)           # (nothing fitted: the neighbours of the first point, harmless)
            lo = temps[(at - 1).clamp(min=0)]
            hi = temps[(at + 1).clamp(max=T - 1)]
            step = torch.arange(REFINE_POINTS, dtype=torch.float64, device=dev) / (REFINE_POINTS - 1)
            fine = lo * (hi / lo) ** step
            fit = _sweep(x, target, fine.contiguous())
    return fit


def calibrate_with(model, X, paths, num_w, walk_len, nodes, labels, *, samples=8, seed=0, first_epoch=0, max_bytes=1 << 30,
                   **fit_kw):
    """The body of ``model.calibrate`` (modules._Aggregator.calibrate carries the documentation)."""
    from . import ensemble as ens
    dev = X.device
    if dev.type != "cuda":
        raise RuntimeError("pathnet_amd aggregators run on the GPU only (X is on %s); no CPU fallback" % dev)
    K, C, N = int(samples), int(model.out_size), int(X.shape[0])
    nodes32 = ens._node_list(nodes, N, dev)
    S = int(nodes32.numel())
    if 4 * K * S * C > int(max_bytes):
        raise ValueError("calibrate: %d samples x %d nodes x %d classes of fp32 logits exceed max_bytes=%d; use fewer nodes "
                         "(one scalar does not need the whole validation set)" % (K, S, C, int(max_bytes)))
    target = torch.as_tensor(labels).reshape(-1).to(dev)
    if target.numel() == N and N != S:
        target = target.index_select(0, nodes32.long())
    elif target.numel() != S:
        raise ValueError("calibrate: %d labels for %d nodes (of %d)" % (target.numel(), S, N))
    store = torch.empty((max(K, 1), S, C), dtype=torch.float32, device=dev)

    def collect(out, k0, b0):       # out [R, cnt, C]: samples k0 .. k0 + R - 1 of nodes b0 .. b0 + cnt - 1
        store[k0:k0 + out.shape[0], b0:b0 + out.shape[1]].copy_(out)

    ens.predict_with(model, X, paths, num_w, walk_len, nodes32, samples=K, seed=seed, first_epoch=first_epoch, collect=collect)
    return fit_temperature(store, target, **fit_kw)


FIELDS = ("bin_count", "bin_correct", "bin_conf", "ece", "mce", "nll", "brier", "aurc", "order", "err_prefix", "counts",
          "confidence")


class Calibration(collections.namedtuple("Calibration", FIELDS)):
    """Device tensors:
    bin_count, bin_correct int64 [B]   used rows / correct rows whose confidence falls into bin b = min(B-1, floor(conf B))
    bin_conf int64 [B]                 the bin's summed confidence in units of 2^-32 (exact)
    ece, mce float64 []                sum_b count_b / m |acc_b - conf_b| and max_b |acc_b - conf_b| over the non-empty bins
    nll, brier float64 []              mean -log prob[label] (over the rows where it is > 0) and mean sum_c (p_c - [c == y])^2
    aurc float64 []                    area under the risk-coverage curve (None with curve=False)
    order int32 [n]                    used rows by descending confidence, ties by row, unused rows last (None with curve=False)
    err_prefix int32 [n]               errors among the first k + 1 rows of order (None with curve=False)
    counts int64 [5]                   {used, unlabelled by the ensemble, label outside [0, C), confidence refused,
                                       prob[label] == 0}
    confidence float32 [n]             the Prediction's confidence (what threshold() reads)"""
    __slots__ = ()

    def summary(self):
        """A dict of Python numbers and lists (the one host read)"""
        B = self.bin_count.numel()
        parts = [self.bin_count.double(), self.bin_correct.double(), self.bin_conf.double() / 2.0 ** 32,
                 self.counts.double(), torch.stack((self.ece, self.mce, self.nll, self.brier))]
        if self.aurc is not None:
            parts.append(self.aurc.reshape(1))
        flat = torch.cat(parts).cpu().numpy()
        cnt = flat[:B]
        live = np.maximum(cnt, 1.0)
        c = flat[3 * B:3 * B + 5]
        tail = flat[3 * B + 5:]
        out = dict(rows=int(self.confidence.numel()), used=int(c[0]), unlabelled_rows=int(c[1]), labels_out_of_range=int(c[2]),
                   confidence_refused=int(c[3]), zero_prob_rows=int(c[4]), bin_count=cnt.astype(np.int64).tolist(),
                   bin_accuracy=(flat[B:2 * B] / live).tolist(), bin_confidence=(flat[2 * B:3 * B] / live).tolist(),
                   accuracy=float(flat[B:2 * B].sum() / c[0]) if c[0] else 0.0,
                   ece=float(tail[0]), mce=float(tail[1]), nll=float(tail[2]), brier=float(tail[3]))
        if self.aurc is not None:
            out["aurc"] = float(tail[4])
        return out

    def threshold(self, coverage):
        """The confidence above which (inclusive) the share ``coverage`` of the used rows lies -> float32 device scalar (NaN
        when no row is used).  Needs curve=True."""
        if self.order is None:
            raise ValueError("Calibration.threshold needs the risk-coverage order (curve=True)")
        if not 0.0 < float(coverage) <= 1.0:
            raise ValueError("Calibration.threshold: coverage %r, in (0, 1]" % (coverage,))
        m = self.counts[0]
        if self.order.numel() == 0:
            return torch.full((), float("nan"), dtype=torch.float32, device=self.counts.device)
        k = torch.ceil(m.double() * float(coverage)).long().clamp(min=1, max=self.order.numel())
        value = self.confidence[self.order[k - 1].long()]
        return torch.where(m > 0, value, torch.full_like(value, float("nan")))


def calibration_of(pred, labels, bins=15, curve=True):
    """The body of ``Prediction.calibration``"""
    conf = pred.confidence.contiguous()
    dev = conf.device
    if dev.type != "cuda":
        raise RuntimeError("Prediction.calibration runs on the GPU only (the prediction is on %s); no CPU fallback" % dev)
    n, C, B = int(conf.numel()), int(pred.prob.shape[1]), int(bins)
    target = torch.as_tensor(labels).reshape(-1).to(device=dev, dtype=torch.int64).contiguous()
    if target.numel() != n:
        raise ValueError("Prediction.calibration: %d labels for %d rows" % (target.numel(), n))
    lib = _lib.load()
    need = ctypes.c_int64(0)
    _lib.check(lib.pn_calib_stats_workspace_bytes(n, B, ctypes.byref(need)))      # refuses a bad bin count
    with torch.cuda.device(dev):
        ws = torch.empty(max(need.value, 8), dtype=torch.uint8, device=dev)
        ints = torch.zeros((3, B), dtype=torch.int64, device=dev)
        counts = torch.zeros(5, dtype=torch.int64, device=dev)
        sums = torch.zeros(2, dtype=torch.float64, device=dev)
        order = torch.empty(n, dtype=torch.int32, device=dev) if curve else None
        err_prefix = torch.empty(n, dtype=torch.int32, device=dev) if curve else None
        aurc = torch.zeros(1, dtype=torch.float64, device=dev) if curve else None
        label, prob = pred.label.contiguous(), pred.prob.float().contiguous()
        out = _lib.CalibStatsOut(ints[0].data_ptr(), ints[1].data_ptr(), ints[2].data_ptr(), counts.data_ptr(), sums.data_ptr(),
                                 order.data_ptr() if curve else None, err_prefix.data_ptr() if curve else None,
                                 aurc.data_ptr() if curve else None)
        _lib.check(lib.pn_calib_stats(_lib.context(dev), _lib.ptr(conf), _lib.ptr(label), _lib.ptr(target), _lib.ptr(prob), n, C,
                                      B, _lib.ptr(ws), ws.numel(), ctypes.byref(out), _lib.stream_ptr(dev)))
        cnt = ints[0].double()
        m = counts[0].double()
        live = cnt > 0
        safe = torch.where(live, cnt, torch.ones_like(cnt))
        gap = torch.where(live, (ints[1].double() / safe - ints[2].double() / 2.0 ** 32 / safe).abs(), torch.zeros_like(cnt))
        m_safe = torch.clamp(m, min=1.0)
        ece = (cnt / m_safe * gap).sum()
        mce = gap.max()
        nll_rows = torch.clamp(m - counts[4].double(), min=1.0)
        nll = sums[0] / nll_rows
        brier = sums[1] / m_safe
    return Calibration(ints[0], ints[1], ints[2], ece, mce, nll, brier, aurc[0] if curve else None, order, err_prefix, counts,
                       conf)
