"""Self-supervised contrastive loss between two path draws (pn_contrast_forward / pn_contrast_backward, pn_contrast.hip).

Two independent path draws of the same nodes are two views of them; ``contrastive_loss(a, b)`` is the NT-Xent / InfoNCE loss
between the two ``[S, D]`` embeddings: the rows are normalised, every row's partner in the other view is its positive, every
other live row (``intra=True``; only the other view's with ``intra=False``) a negative.  Forward and backward are tiled HIP
kernels with exact fp32 products and fixed summation orders: no ``[2S, 2S]`` array is ever in memory and the same inputs give
the same bits.  ``pathnet_amd.trainer.pretrain`` / ``model.pretrain`` drive it.
"""
import collections
import ctypes
import math

import torch

from . import _lib


class Contrast(collections.namedtuple("Contrast", ("loss", "row_loss", "hits", "counts", "loss64"))):
    """loss float32 []        (1 / 2M) sum of the live rows' losses; differentiable w.r.t. both inputs (0 when M == 0)
    row_loss float32 [2S]    log sum_{c in N(r)} exp(s_rc) - s_{r, partner}; view 1's rows first; 0 for a row that is not live
    hits int64 [1]           rows whose partner has the largest logit of the row
    counts int64 [2]         {M: live pairs, pairs left out because an entry is not finite or a norm is 0}
    loss64 float64 [1]       the loss as the kernel summed it
    All device tensors; only ``loss`` carries a gradient."""
    __slots__ = ()

    def summary(self):
        """A dict of Python numbers (the one host read)"""
        flat = torch.cat((self.loss64, self.hits.double(), self.counts.double())).cpu().numpy()
        M = int(flat[2])
        return dict(loss=float(flat[0]), hits=int(flat[1]), pairs=M, bad_pairs=int(flat[3]),
                    hit_rate=float(flat[1]) / (2 * M) if M else 0.0)


class _ContrastFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, b, tau, intra, valid):
        dev = a.device
        S, D = (int(v) for v in a.shape)
        lib = _lib.load()
        need = ctypes.c_int64(0)
        _lib.check(lib.pn_contrast_workspace_bytes(S, D, ctypes.byref(need)))
        with torch.cuda.device(dev):
            ws = torch.empty(max(need.value, 8), dtype=torch.uint8, device=dev)
            loss64 = torch.empty(1, dtype=torch.float64, device=dev)
            row_loss = torch.empty(2 * S, dtype=torch.float32, device=dev)
            hits = torch.empty(1, dtype=torch.int64, device=dev)
            counts = torch.empty(2, dtype=torch.int64, device=dev)
            out = _lib.ContrastOut(loss64.data_ptr(), row_loss.data_ptr(), hits.data_ptr(), counts.data_ptr())
            _lib.check(lib.pn_contrast_forward(_lib.context(dev), _lib.ptr(a), a.stride(0), _lib.ptr(b), b.stride(0), S, D, tau,
                                               intra, _lib.ptr(valid), _lib.ptr(ws), ws.numel(), ctypes.byref(out),
                                               _lib.stream_ptr(dev)))
        ctx.save_for_backward(a, b, ws)
        ctx.args = (S, D, tau, intra)
        ctx.mark_non_differentiable(row_loss, hits, counts, loss64)
        return loss64[0].float(), row_loss, hits, counts, loss64

    @staticmethod
    def backward(ctx, g_loss, *unused):
        a, b, ws = ctx.saved_tensors
        S, D, tau, intra = ctx.args
        dev = a.device
        with torch.cuda.device(dev):
            g = g_loss.detach().reshape(1).to(device=dev, dtype=torch.float32).contiguous()
            da, db = torch.empty((S, D), dtype=torch.float32, device=dev), torch.empty((S, D), dtype=torch.float32, device=dev)
            _lib.check(_lib.load().pn_contrast_backward(_lib.context(dev), _lib.ptr(a), a.stride(0), _lib.ptr(b), b.stride(0), S,
                                                        D, tau, intra, _lib.ptr(ws), ws.numel(), _lib.ptr(g), _lib.ptr(da),
                                                        _lib.ptr(db), _lib.stream_ptr(dev)))
        return da, db, None, None, None


def _rows(x, name):
    if x.dim() != 2:
        raise ValueError("contrastive_loss: %s [S, D] expected, got %s" % (name, tuple(x.shape)))
    if not x.dtype.is_floating_point:
        raise TypeError("contrastive_loss: %s must be a float tensor, got %s" % (name, x.dtype))
    x = x.float()
    if x.shape[0] > 1 and (x.stride(1) != 1 or x.stride(0) < x.shape[1]) or x.shape[0] <= 1 and not x.is_contiguous():
        x = x.contiguous()
    return x


def contrastive_loss(a, b, temperature=0.5, intra=True, valid=None):
    """NT-Xent / InfoNCE between ``a`` and ``b`` ([S, D], on the GPU; row s of both is the same node) -> ``Contrast``.

    With z the rows of a and b scaled to unit length (norms in fp64), s_rc = <z_r, z_c> / temperature and N(r) the live rows
    c != r (intra=True: SimCLR / GRACE NT-Xent; intra=False: only the rows of the other view, the symmetric cross-view form),
    a row's loss is log sum_{c in N(r)} exp(s_rc) - s_{r, partner} and ``loss`` their mean over the 2M live rows.  A pair is
    live when ``valid`` (bool / integer [S], optional) is non-zero for it, all its entries are finite and neither norm is 0;
    the other pairs take no part, as positives or as negatives, and get a zero gradient.
    fp32 inputs; other float dtypes are converted.  Row-strided inputs (a column slice) are read in place.  Nothing is read
    back: M divides on the device, so a step that uses the loss stays capturable."""
    if a.device.type != "cuda" or b.device != a.device:
        raise RuntimeError("pathnet_amd.contrastive_loss runs on the GPU only (a on %s, b on %s); no CPU fallback"
                           % (a.device, b.device))
    a, b = _rows(a, "a"), _rows(b, "b")
    if a.shape != b.shape:
        raise ValueError("contrastive_loss: a %s and b %s differ in shape" % (tuple(a.shape), tuple(b.shape)))
    tau = float(temperature)
    if not (tau > 0.0 and math.isfinite(tau)):
        raise ValueError("contrastive_loss: temperature %r, finite and > 0" % (temperature,))
    if valid is not None:
        valid = torch.as_tensor(valid).reshape(-1)
        if valid.numel() != a.shape[0]:
            raise ValueError("contrastive_loss: %d valid flags for %d rows" % (valid.numel(), a.shape[0]))
        valid = (valid != 0).to(device=a.device, dtype=torch.uint8).contiguous()
    return Contrast(*_ContrastFunction.apply(a, b, tau, 1 if intra else 0, valid))
