"""What calibration costs at the headline shape (S = 1299 validation rows, C = 7 classes, K = 8 samples), on logits made here
(base ~ N(0, 4), 0.3 noise per sample, labels drawn from softmax(base)).  Legs in ONE process, alternating blocks, device
events around each block, every leg ten calls of the C entry point back to back:
  sweep_25     pn_calib_sweep over the default grid of 25 temperatures        (round 1 of fit_temperature)
  sweep_17     pn_calib_sweep over the 17 points of the refinement            (round 2)
  stats        pn_calib_stats, 15 bins, with prob and the risk-coverage curve (the radix sort included)
  stats_bins   pn_calib_stats, 15 bins, with prob, without the curve
  add          pn_ensemble_add of the [8, 1299, 7] logits
  add_scaled   pn_ensemble_add_scaled of the same logits at the fitted tau
and fit_temperature() end to end (both rounds, the grid of round 2 built with torch on the device).  Prints medians and spread
(half the range between the 10th and 90th percentile of the blocks) and one JSON line.  Needs a GPU: there is no fallback.
   python tools/calibrate_ab.py [--blocks 8] [--steps 10] [--warmup 3] [--out FILE]"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

S, C, K, BINS = 1299, 7, 8, 15


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=8)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None, help="append the report to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("calibrate_ab: needs a GPU")
    import pathnet_amd
    from pathnet_amd import _lib, calibration
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    base = 2.0 * torch.randn(S, C, generator=g, dtype=torch.float64)
    logits = (1.7 * (base[None] + 0.3 * torch.randn(K, S, C, generator=g, dtype=torch.float64))).float().to(dev).contiguous()
    target = torch.multinomial(torch.softmax(base, dim=1), 1, generator=g).flatten().to(dev)
    lib, ctx, stream = _lib.load(), _lib.context(dev), _lib.stream_ptr(dev)

    fit = pathnet_amd.fit_temperature(logits, target)
    coarse = torch.tensor(calibration.DEFAULT_GRID, dtype=torch.float64, device=dev)
    fine = fit.temps.contiguous()
    sweeps = {}
    for name, temps in (("sweep_25", coarse), ("sweep_17", fine)):
        T = int(temps.numel())
        need = ctypes.c_int64(0)
        _lib.check(lib.pn_calib_sweep_workspace_bytes(S, T, ctypes.byref(need)))
        ws = torch.empty(need.value, dtype=torch.uint8, device=dev)
        nll = torch.empty(T, dtype=torch.float64, device=dev)
        tau, best = torch.empty(1, dtype=torch.float64, device=dev), torch.empty(1, dtype=torch.int32, device=dev)
        counts = torch.empty(3, dtype=torch.int64, device=dev)
        out = _lib.CalibSweepOut(nll.data_ptr(), best.data_ptr(), tau.data_ptr(), counts.data_ptr())

        def leg(temps=temps, T=T, ws=ws, out=out, nll=nll, keep=(tau, best, counts)):
            for _ in range(10):
                _lib.check(lib.pn_calib_sweep(ctx, _lib.ptr(logits), K, S, C, _lib.ptr(target), _lib.ptr(temps), T, _lib.ptr(ws),
                                              ws.numel(), ctypes.byref(out), stream))
            return nll
        sweeps[name] = leg

    pred = pathnet_amd.Ensemble(S, C, dev, temperature=fit.tau).add(logits).result()
    conf, label, prob = pred.confidence.contiguous(), pred.label.contiguous(), pred.prob.contiguous()
    need = ctypes.c_int64(0)
    _lib.check(lib.pn_calib_stats_workspace_bytes(S, BINS, ctypes.byref(need)))
    sws = torch.empty(need.value, dtype=torch.uint8, device=dev)
    ints = torch.zeros((3, BINS), dtype=torch.int64, device=dev)
    cnt, sums = torch.zeros(5, dtype=torch.int64, device=dev), torch.zeros(2, dtype=torch.float64, device=dev)
    order, prefix = torch.empty(S, dtype=torch.int32, device=dev), torch.empty(S, dtype=torch.int32, device=dev)
    aurc = torch.zeros(1, dtype=torch.float64, device=dev)
    with_curve = _lib.CalibStatsOut(ints[0].data_ptr(), ints[1].data_ptr(), ints[2].data_ptr(), cnt.data_ptr(), sums.data_ptr(),
                                    order.data_ptr(), prefix.data_ptr(), aurc.data_ptr())
    bins_only = _lib.CalibStatsOut(ints[0].data_ptr(), ints[1].data_ptr(), ints[2].data_ptr(), cnt.data_ptr(), sums.data_ptr(),
                                   None, None, None)

    def leg_stats(out=with_curve):
        for _ in range(10):
            _lib.check(lib.pn_calib_stats(ctx, _lib.ptr(conf), _lib.ptr(label), _lib.ptr(target), _lib.ptr(prob), S, C, BINS,
                                          _lib.ptr(sws), sws.numel(), ctypes.byref(out), stream))
        return sums

    plain, scaled = pathnet_amd.Ensemble(S, C, dev), pathnet_amd.Ensemble(S, C, dev, temperature=fit.tau)

    def leg_add():
        for _ in range(10):
            _lib.check(lib.pn_ensemble_add(ctx, _lib.ptr(logits), K, S, C, None, S, _lib.ptr(plain.state), None, stream))
        return plain.hsum

    def leg_add_scaled():
        for _ in range(10):
            _lib.check(lib.pn_ensemble_add_scaled(ctx, _lib.ptr(logits), K, S, C, None, S, _lib.ptr(scaled.state), None,
                                                  _lib.ptr(scaled.temperature), stream))
        return scaled.hsum

    def leg_fit():
        return pathnet_amd.fit_temperature(logits, target).nll

    legs = dict(sweeps)
    legs.update(stats=leg_stats, stats_bins=lambda: leg_stats(bins_only), add=leg_add, add_scaled=leg_add_scaled,
                fit_temperature=leg_fit)
    ten = set(legs) - {"fit_temperature"}
    times = {k: [] for k in legs}
    for name, fn in legs.items():
        for _ in range(args.warmup):
            last = fn()
        torch.cuda.synchronize()
        assert torch.isfinite(last).all().item(), name
    for _ in range(args.blocks):
        for name, fn in legs.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(args.steps):
                fn()
            b.record()
            b.synchronize()
            times[name].append(a.elapsed_time(b) / args.steps)
    rec = {"shape": dict(S=S, C=C, K=K, bins=BINS), "blocks": args.blocks, "steps": args.steps,
           "fitted": fit.summary()["tau"]}
    lines = ["calibrate_ab: S = %d, C = %d, K = %d, %d bins; fitted tau %.6f" % (S, C, K, BINS, rec["fitted"])]
    for name, t in times.items():
        t = np.asarray(t) / (10 if name in ten else 1)
        rec[name] = {"median_ms": float(np.median(t)), "spread_ms": float((np.percentile(t, 90) - np.percentile(t, 10)) / 2),
                     "min_ms": float(t.min()), "max_ms": float(t.max())}
        lines.append("%-16s median %.4f ms  spread +-%.4f  (min %.4f max %.4f) over %d blocks of %d calls%s"
                     % (name, rec[name]["median_ms"], rec[name]["spread_ms"], t.min(), t.max(), args.blocks, args.steps,
                        ", ten launches each" if name in ten else ""))
    rec["add_scaled_over_add"] = rec["add_scaled"]["median_ms"] / rec["add"]["median_ms"]
    lines.append("pn_ensemble_add_scaled / pn_ensemble_add = %.3f" % rec["add_scaled_over_add"])
    lines.append(json.dumps(rec))
    print("\n".join(lines))
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
