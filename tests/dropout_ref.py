"""Plain numpy restatement of the built-in dropout masks (pathnet_amd/csrc/pn_kernels.h: philox4 / dropout4 / dropout1).
No library code, no GPU.  tests/test_dropout_host.py holds it to Random123's known answers for Philox4x32-10 and to
oracle.merw.philox_draw, the C restatement that the GPU sampler tests pin bit-exact to rocRAND.

The contract (include/pathnet_hip.h: mask_seq / mask_cls; pn_kernels.h: dropout4):

    words    philox4x32-10 of counter (ctr lo, ctr hi, stream, 0x50415448) under key (seed lo, seed hi)
    keep     word >= (uint32)(p * 2^32), the product formed in fp32 and clamped at 4294967040
    value    1.0f / (1.0f - p) where kept, else 0
    stream 1 the recurrent input [L, P_total, Hk]: element [t, slot, 4 c4 + k] is word k of counter
             (t * P_total + slot) * (Hk / 4) + c4;  slot is the sequence slot q of oracle/pagg_oracle.py: plan()
    stream 2 the classifier input [S_total, 2 Hk]: element e (row-major) is word e & 3 of counter e >> 2

Hk is the kernels' hidden size, H rounded up to a multiple of 32; P_total and S_total are those of the whole batch."""
import numpy as np
import torch

TAG = 0x50415448
STREAM_SEQ, STREAM_CLS = 1, 2
_M0, _M1, _W0, _W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
_LO = np.uint64(0xFFFFFFFF)
_32 = np.uint64(32)


def philox4x32_10(ctr, key):
    """ctr: four, key: two arrays (or integers) of 32-bit values, broadcast together -> uint32 [..., 4]"""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) for c in ctr)
    k0, k1 = (np.asarray(k, dtype=np.uint64) for k in key)
    for _ in range(10):
        m0, m1 = np.uint64(_M0) * c0, np.uint64(_M1) * c2
        c0, c1, c2, c3 = (m1 >> _32) ^ c1 ^ k0, m1 & _LO, (m0 >> _32) ^ c3 ^ k1, m0 & _LO
        k0, k1 = (k0 + np.uint64(_W0)) & _LO, (k1 + np.uint64(_W1)) & _LO
    return np.stack(np.broadcast_arrays(c0, c1, c2, c3), axis=-1).astype(np.uint32)


def philox4(seed, ctr, stream):
    """the kernels' hash: four uint32 words per 64-bit counter (array or integer) -> [..., 4]"""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    ctr = np.asarray(ctr, dtype=np.uint64)
    return philox4x32_10((ctr & _LO, ctr >> _32, np.uint64(stream), np.uint64(TAG)), (seed & 0xFFFFFFFF, seed >> 32))


def cut(p):
    p32 = np.float32(p)
    return np.uint32(min(np.float32(p32 * np.float32(4294967296.0)), np.float32(4294967040.0)))


def scale(p):
    return np.float32(1) / (np.float32(1) - np.float32(p))


def keep(words, p):
    return words >= cut(p)


def kernel_hidden(H):
    return -(-int(H) // 32) * 32


def seq_mask(seed, p, L, P_total, Hk):
    """fp32 [L, P_total, Hk]"""
    assert Hk % 4 == 0
    ctr = np.arange(L * P_total * (Hk // 4), dtype=np.uint64)
    k = keep(philox4(seed, ctr, STREAM_SEQ), p).reshape(L, P_total, Hk)
    return np.where(k, scale(p), np.float32(0)).astype(np.float32)


def cls_mask(seed, p, S_total, Hk):
    """fp32 [S_total, 2 Hk]"""
    ctr = np.arange(S_total * 2 * Hk // 4, dtype=np.uint64)
    k = keep(philox4(seed, ctr, STREAM_CLS), p).reshape(S_total, 2 * Hk)
    return np.where(k, scale(p), np.float32(0)).astype(np.float32)


def module_masks(seed, p, L, S_total, W, H):
    """(mask_seq [L, S_total W, H], mask_cls [S_total, 2 H]) as torch fp32 tensors for a module of hidden size H: drawn at
    the kernels' Hk and cut as modules._explicit_masks pads -- what oracle/pagg_oracle.py takes as drop_seq / drop_cls"""
    Hk = kernel_hidden(H)
    ms = seq_mask(seed, p, L, S_total * W, Hk)[:, :, :H]
    mc = cls_mask(seed, p, S_total, Hk).reshape(S_total, 2, Hk)[:, :, :H].reshape(S_total, 2 * H)
    return torch.from_numpy(np.ascontiguousarray(ms)), torch.from_numpy(np.ascontiguousarray(mc))


def module_seed(torch_seed):
    """the seed modules._run draws from torch's generator after torch.manual_seed(torch_seed)"""
    torch.manual_seed(torch_seed)
    return int(torch.randint(0, 2 ** 62, (1,)).item())
