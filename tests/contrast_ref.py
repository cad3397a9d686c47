"""NumPy fp64 restatement of pn_contrast_forward / pn_contrast_backward (pathnet_amd/csrc/pn_contrast.hip), over explicit
[2S, 2S] arrays, with the analytic gradient, the derived error bounds and the input builders of the GPU tests.  Not a test.

The definition (include/pathnet_hip.h).  A, B [S, D]; pair i is live when valid[i] != 0 (or valid is None), all entries of a_i
and b_i are finite and both fp64 norms are finite and > 0; M live pairs, `bad` pairs dead for the data's sake alone.  z stacks
the unit rows (view 1 first, n = 2S), p(r) = r +- S, s_rc = <z_r, z_c> / tau, N(r) = live c != r (intra == 0: other view only).
    lse_r = log sum_{N(r)} exp(s_rc);  row_loss_r = lse_r - s_{r,p(r)};  loss = sum_{live r} row_loss_r / (2M)
    P_rc = exp(s_rc - lse_r);  dz_r = g / (2 M tau) [sum_{N(r)} (P_rc + P_cr) z_c - 2 z_{p(r)}];  dx_r = (dz_r - z_r <z_r, dz_r>) / |x_r|

The bounds.  u = 2^-24 is the fp32 unit round-off; everything the kernels do in fp64 (norms, log, the loss sum, the
projection) contributes O(2^-53) and is covered by the +1e-12 terms.  First order in u throughout, times SAFETY = 1.5.

 1. unit rows.  z^ = fl32(x / norm): |z^_d - z_d| <= u |z_d|.
 2. logit.  The MFMA is one k-ordered fma chain of D products: |fl(<z^_r, z^_c>) - <z^_r, z^_c>| <= D u sum_d |z_rd z_cd| <= D u
    (Cauchy-Schwarz, unit rows); the two operand errors of (1) add 2u, the factor fl32(1 / tau) and the product with it 2u:
        E_s = (D + 4) u / tau                                                       tol_logit
 3. lse.  d lse / d s is a probability vector, so the logit errors move lse by at most E_s.  The online softmax adds relative
    errors to the SUM: an exponent v - m (|v - m| <= 2 / tau) is rounded (2u / tau) and expf is good to 2u, an fp32 product and
    an fp32 add are u each -- c = 2u / tau + 5u per step -- and a term passes through at most one rescale per column tile, one
    add per logit of its lane (2 per tile), 5 butterfly merges and the merge of the two column halves: steps = 3 T + 8 with
    T = ceil(2S / column tile).  A relative error of the sum is an absolute error of its log.
        E_lse = E_s + (3T + 8) (2u / tau + 5u)
 4. row_loss = lse - pos, rounded to fp32:  E_row = E_lse + E_s + u |row_loss|      tol_row_loss
    loss (from the fp64 row losses, fp64 sums):  E_loss = max_r (E_lse + E_s) + 1e-12    tol_loss
 5. weights.  P^_rc = expf(s^ - lse^_r), lse^ stored in fp32 (u (1 / tau + log 2S)), the subtraction rounded (u |s - lse| <=
    u (2 / tau + log 2S)), expf 2u:  relative error  d_P = E_s + E_lse + u (3 / tau + 2 log 2S) + 2u.  W_rc = P_rc + P_cr
    (- 2 for the partner): one or two more roundings, of terms bounded by P_rc + P_cr + 2.
 6. G_rd = sum_c W_rc z_cd, a chain of n_c <= 2S products (|z_cd| <= 1, operand error u):
        |G^_rd - G_rd| <= A_r (d_P + (2S + 4) u),   A_r = sum_{N(r)} (P_rc + P_cr) + 2
 7. dx_rd = k_r (G_rd - z_rd <z_r, G_r>), k_r = g / (2 M tau |x_r|), in fp64 from G^ and z^, rounded to fp32.  With e_G the
    bound of (6) for every element of the row, sum_d |z_rd| <= sqrt(D), |<z_r, G_r>| <= sqrt(D) max_d |G_rd| <= sqrt(D) A_r:
        |dx^_rd - dx_rd| <= |k_r| [ e_G (1 + sqrt(D) |z_rd|) + 3 u sqrt(D) A_r |z_rd| ] + u |dx_rd|      tol_grad
"""
import ctypes
import functools

import numpy as np

U = 2.0 ** -24
SAFETY = 1.5
TAUS = (0.07, 0.5, 2.0)

VARIANTS = ("diag", "nopartner", "intra", "1/M", "notranspose", "noproj", "deadneg")


@functools.lru_cache(maxsize=None)
def tiles():
    """(row tile, column tile, K chunk) of the kernels, from the library (needs no GPU)"""
    from pathnet_amd import _lib
    out = (ctypes.c_int32 * 3)()
    _lib.check(_lib.load().pn_contrast_tiles(out))
    return tuple(int(v) for v in out)


class Result:
    """everything of one evaluation; arrays fp64"""

    def __init__(self, **kw):
        self.__dict__.update(kw)


def liveness(A, B, valid=None):
    """-> (live [S] bool, M, bad, norms [2S], X [2S, D] with the rows of dead pairs zeroed)"""
    A, B = np.asarray(A, np.float64), np.asarray(B, np.float64)
    S = A.shape[0]
    X = np.concatenate((A, B))
    with np.errstate(invalid="ignore", over="ignore"):
        fin = np.isfinite(X).all(axis=1)
        norm = np.sqrt((np.where(fin[:, None], X, 0.0) ** 2).sum(axis=1))
    ok = fin & np.isfinite(norm) & (norm > 0)
    ok = ok[:S] & ok[S:]
    wanted = np.ones(S, bool) if valid is None else (np.asarray(valid).reshape(-1) != 0)
    live = wanted & ok
    return live, int(live.sum()), int((wanted & ~ok).sum()), norm, X


def reference(A, B, tau, intra, valid=None, g=1.0, variant=None):
    """The definition in fp64 over explicit [2S, 2S] arrays.  variant: one of VARIANTS, a named WRONG implementation."""
    live, M, bad, norm, X = liveness(A, B, valid)
    S, D = np.asarray(A).shape
    n = 2 * S
    live2 = np.concatenate((live, live))
    with np.errstate(invalid="ignore", divide="ignore"):
        Zall = np.where(np.isfinite(X).all(axis=1, keepdims=True) & (norm > 0)[:, None], np.where(np.isfinite(X), X, 0.0)
                        / np.where(norm > 0, norm, 1.0)[:, None], 0.0)
    Z = np.where(live2[:, None], Zall, 0.0)
    Zc = Zall if variant == "deadneg" else Z          # what serves as a column
    col_ok = np.ones(n, bool) if variant == "deadneg" else live2
    if variant == "intra":
        intra = not intra
    r = np.arange(n)
    partner = np.where(r < S, r + S, r - S)
    view = r >= S
    mask = live2[:, None] & col_ok[None, :]
    if variant != "diag":
        mask &= r[:, None] != r[None, :]
    if not intra:
        mask &= view[:, None] != view[None, :]
    if variant == "nopartner":
        mask &= partner[:, None] != r[None, :]
    s = Z @ Zc.T / tau
    sm = np.where(mask, s, -np.inf)
    top = sm.max(axis=1, initial=-np.inf)
    top = np.where(np.isfinite(top), top, 0.0)
    with np.errstate(divide="ignore"):
        lse = top + np.log(np.exp(sm - top[:, None]).sum(axis=1))
    pos = s[r, partner]
    has = mask.any(axis=1)
    row_loss = np.where(live2 & has, lse - pos, 0.0)
    denom = (M if variant == "1/M" else 2 * M)
    loss = row_loss.sum() / denom if M else 0.0
    P = np.where(mask, np.exp(np.where(mask, s - np.where(has, lse, 0.0)[:, None], -np.inf)), 0.0)
    if variant == "deadneg":        # the transposed term of a dead column does not exist: it has no row of its own
        W = P + np.where(live2[None, :], P.T, 0.0)
    elif variant == "notranspose":
        W = P
    else:
        W = P + P.T
    absW = W.sum(axis=1) + 2.0
    coef = g / (denom * tau) if M else 0.0
    Gm = W @ Zc - 2.0 * Z[partner]
    dz = coef * Gm
    if variant == "noproj":
        dx = dz / norm_safe(norm)[:, None]
    else:
        dx = (dz - Z * (Z * dz).sum(axis=1, keepdims=True)) / norm_safe(norm)[:, None]
    dx = np.where(live2[:, None], dx, 0.0)
    others = mask & (partner[:, None] != r[None, :])
    best_neg = np.where(others, s, -np.inf).max(axis=1, initial=-np.inf)
    margin = np.where(live2, pos - best_neg, np.inf)
    hits = int((live2 & (margin >= 0)).sum())
    return Result(S=S, D=D, n=n, M=M, bad=bad, live=live2, Z=Z, norm=norm, s=s, lse=lse, pos=pos, row_loss=row_loss, loss=loss,
                  dA=dx[:S], dB=dx[S:], absW=absW, margin=margin, hits=hits, coef=coef, tau=tau)


def norm_safe(norm):
    return np.where(np.isfinite(norm) & (norm > 0), norm, 1.0)


# ---- the bounds (derivation: module docstring) ----------------------------------------------------------------------------------
def tol_logit(D, tau):
    return SAFETY * (D + 4) * U / tau


def _e_lse(ref):
    T = -(-ref.n // tiles()[1])
    return tol_logit(ref.D, ref.tau) + SAFETY * (3 * T + 8) * (2 * U / ref.tau + 5 * U)


def tol_row_loss(ref):
    return _e_lse(ref) + tol_logit(ref.D, ref.tau) + SAFETY * U * np.abs(ref.row_loss) + 1e-12


def tol_loss(ref):
    return _e_lse(ref) + tol_logit(ref.D, ref.tau) + 1e-12


def tol_grad(ref, g=1.0):
    """-> (tol dA [S, D], tol dB [S, D]) around reference(..., g=g)"""
    n, D, tau = ref.n, ref.D, ref.tau
    logn = np.log(max(n, 2))
    d_p = tol_logit(D, tau) + _e_lse(ref) + SAFETY * U * (3 / tau + 2 * logn + 2)
    e_g = ref.absW * (d_p + SAFETY * (n + 4) * U)
    k = abs(g) / (2 * max(ref.M, 1) * tau) / norm_safe(ref.norm)
    absz = np.abs(ref.Z)
    dx = np.concatenate((ref.dA, ref.dB))
    tol = k[:, None] * (e_g[:, None] * (1 + np.sqrt(D) * absz) + SAFETY * 3 * U * np.sqrt(D) * ref.absW[:, None] * absz)
    tol = tol + SAFETY * U * np.abs(dx) + 1e-30
    tol = np.where(ref.live[:, None], tol, 0.0)
    return tol[:ref.S], tol[ref.S:]


def hits_decidable(ref):
    """every live row's fp64 margin between the positive and the best negative exceeds twice the logit bound"""
    m = np.abs(ref.margin[ref.live])
    return bool((m > 2 * tol_logit(ref.D, ref.tau)).all()), float(m.min() / (2 * tol_logit(ref.D, ref.tau))) if m.size else np.inf


# ---- inputs ---------------------------------------------------------------------------------------------------------------------
KINDS = ("random", "dup", "scaled", "nonfinite", "zero", "valid", "mix")


def make_inputs(kind, S, D, seed=0):
    """-> (A, B fp32 [S, D], valid uint8 [S] or None).  Every row holds a shared component (embeddings do; it keeps the
    negatives' cosines near 0.8, so that no term of a row's sum vanishes below the bound at tau = 0.07); B is A plus noise, so
    most positives win clearly; a tenth of the pairs are unrelated, so some lose clearly."""
    rng = np.random.default_rng(1000 * S + 10 * D + seed)
    A = 2.0 * rng.standard_normal(D) + rng.standard_normal((S, D))
    B = A + 0.5 * rng.standard_normal((S, D))
    swap = rng.random(S) < 0.1
    B[swap] = rng.standard_normal((int(swap.sum()), D))
    A, B = A.astype(np.float32), B.astype(np.float32)
    valid = None
    pick = lambda k, m: rng.permutation(S)[:max(1, S // m)] if S >= k else np.zeros(0, np.int64)        # noqa: E731
    if kind == "dup" and S >= 2:
        src = pick(2, 4)
        A[(src + 1) % S] = A[src]           # duplicated rows inside a view: logits of exactly 1 / tau that are not the partner
    if kind in ("scaled", "mix"):
        A[pick(1, 5)] *= np.float32(1e-20)      # squares underflow / overflow in fp32: the norms need fp64
        B[pick(1, 5)] *= np.float32(1e20)
    if kind in ("nonfinite", "mix"):
        for X, v in ((A, np.nan), (B, np.inf), (A, -np.inf)):
            rows = pick(2, 9)
            X[rows, rng.integers(0, D, len(rows))] = v
    if kind in ("zero", "mix"):
        A[pick(2, 8)] = 0.0
        B[pick(2, 11)] = 0.0
    if kind in ("valid", "mix"):
        valid = (rng.random(S) < 0.7).astype(np.uint8)
        if S >= 2:
            valid[0], valid[S - 1] = 0, 1
    return A, B, valid


@functools.lru_cache(maxsize=None)
def case_table():
    """(kind, S, D, hits_exact) of the GPU tests, built from the kernels' tiles.  2S is even, so "2S at t - 1, t, t + 1" is held
    twice: 2S at t - 2, t, t + 2 and S itself at t - 1, t, t + 1 (the view boundary against the tile edge).
    hits_exact: hits is compared exactly.  Not where rows tie BY CONSTRUCTION -- D == 1 (every logit is +- 1 / tau) and
    duplicated rows (a duplicate's logit equals the original's in every row) -- there the margin is 0 in fp64 too."""
    rt, ct, kc = tiles()
    sizes = {1, 2}
    for t in (rt, ct):
        sizes |= {t // 2 - 1, t // 2, t // 2 + 1, t - 1, t, t + 1}
    sizes |= {ct + 1, (3 * ct) // 2}                  # 2S = 2 ct + 2: three column tiles, the last partial; 2S = 3 ct
    d0 = kc + 1
    rows = [("random", S, d0, True) for S in sorted(sizes)]
    s0 = rt // 2 + 1
    rows += [("random", s0, D, D > 1) for D in (1, 2, kc - 1, kc, 2 * kc + 1)]
    rows += [(kind, rt + 1, d0, kind not in ("dup",)) for kind in KINDS[1:]]
    rows += [("mix", (3 * ct) // 2, 2 * kc + 1, True)]
    assert max(2 * r[1] for r in rows) <= 3 * ct + 1 and max(r[2] for r in rows) <= 2 * kc + 1
    return tuple(rows)


@functools.lru_cache(maxsize=None)
def case(kind, S, D, tau, intra):
    """-> (A, B, valid, reference at g = 1); computed once and shared -- leave the arrays unchanged"""
    A, B, valid = make_inputs(kind, S, D)
    for x in (A, B) + ((valid,) if valid is not None else ()):
        x.setflags(write=False)
    return A, B, valid, reference(A, B, tau, intra, valid)


def without_dead_rows(A, B, valid):
    """the live pairs alone, and their positions"""
    live = liveness(A, B, valid)[0]
    keep = np.flatnonzero(live)
    return A[keep], B[keep], keep
