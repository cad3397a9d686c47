"""What the fused contrastive loss costs against the torch composition of the same formula, forward + backward, at D = 256
for S = 1299, 2708 and 8192 pairs and both `intra` settings, on random embeddings made here.  The two legs:
  fused   pathnet_amd.contrastive_loss(a, b).loss.backward()          (pn_contrast_forward / pn_contrast_backward)
  torch   F.normalize, cat, mm, masked logsumexp, autograd            (what a user writes without it: [2S, 2S] arrays)
alternate in ONE process, every call between two device events; per leg 3 warm-up calls, then the median of 20.  Peak memory is
torch.cuda.max_memory_allocated over one call of the leg, above what is allocated before it.  Prints one line per shape and
one JSON line.  Needs a GPU: there is no fallback.
   python tools/contrast_ab.py [--calls 20] [--warmup 3] [--out FILE]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

D, TAU = 256, 0.5
SHAPES = (1299, 2708, 8192)


def torch_loss(a, b, tau, intra):
    S = a.shape[0]
    z = torch.nn.functional.normalize(torch.cat((a, b)), dim=1)
    s = z @ z.t() / tau
    r = torch.arange(2 * S, device=a.device)
    mask = r[:, None] != r[None, :]
    if not intra:
        mask = mask & ((r[:, None] >= S) != (r[None, :] >= S))
    lse = torch.logsumexp(s.masked_fill(~mask, float("-inf")), dim=1)
    return (lse - s[r, (r + S) % (2 * S)]).mean()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None, help="append the report to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("contrast_ab: needs a GPU")
    import pathnet_amd
    dev = torch.device("cuda:0")
    lines = ["contrast_ab: D = %d, tau = %g, forward + backward, median of %d calls after %d warm-ups, legs alternating"
             % (D, TAU, args.calls, args.warmup)]
    recs = []
    for S in SHAPES:
        for intra in (True, False):
            g = torch.Generator().manual_seed(S)
            a = (torch.randn(D, generator=g) + torch.randn(S, D, generator=g)).to(dev).requires_grad_()
            b = (a.detach().cpu() + 0.5 * torch.randn(S, D, generator=g)).to(dev).requires_grad_()

            def fused():
                a.grad = b.grad = None
                loss = pathnet_amd.contrastive_loss(a, b, temperature=TAU, intra=intra).loss
                pathnet_amd.backward(loss)
                return loss

            def composed():
                a.grad = b.grad = None
                loss = torch_loss(a, b, TAU, intra)
                loss.backward()
                return loss

            legs = {"fused": fused, "torch": composed}
            vals, peak, times = {}, {}, {k: [] for k in legs}
            for name, fn in legs.items():
                for _ in range(args.warmup):
                    vals[name] = float(fn().detach())
                torch.cuda.synchronize()
                base = torch.cuda.memory_allocated()
                torch.cuda.reset_peak_memory_stats()
                fn()
                torch.cuda.synchronize()
                peak[name] = torch.cuda.max_memory_allocated() - base
            for _ in range(args.calls):
                for name, fn in legs.items():
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    fn()
                    e1.record()
                    e1.synchronize()
                    times[name].append(e0.elapsed_time(e1))
            rec = dict(S=S, D=D, intra=int(intra), loss_fused=vals["fused"], loss_torch=vals["torch"])
            for name in legs:
                t = np.asarray(times[name])
                rec[name] = dict(median_ms=float(np.median(t)), min_ms=float(t.min()), max_ms=float(t.max()),
                                 peak_mib=peak[name] / 2.0 ** 20)
            rec["fused_over_torch"] = rec["fused"]["median_ms"] / rec["torch"]["median_ms"]
            recs.append(rec)
            lines.append("S %5d intra %d: fused %8.3f ms (min %.3f max %.3f) peak %9.1f MiB | torch %8.3f ms (min %.3f max %.3f) "
                         "peak %9.1f MiB | fused / torch time %.2f, loss %.6f vs %.6f"
                         % (S, intra, rec["fused"]["median_ms"], rec["fused"]["min_ms"], rec["fused"]["max_ms"],
                            rec["fused"]["peak_mib"], rec["torch"]["median_ms"], rec["torch"]["min_ms"], rec["torch"]["max_ms"],
                            rec["torch"]["peak_mib"], rec["fused_over_torch"], vals["fused"], vals["torch"]))
            del a, b
            torch.cuda.empty_cache()
    lines.append(json.dumps(recs))
    print("\n".join(lines))
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
