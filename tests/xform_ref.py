"""Float64 restatement of the splice + affine stage (mfx_batch_set_transform, k_splice_affine) with its float32 bound.

Plain numpy: no GPU, no oracle.  The rows y the stage reads come from a twin handle without a transform (same PCM, same
plan), so nothing but the new kernel enters the comparison; the twin's rows are held to the reference by the other suites.

    z[t]   = [ y[clamp(t - left, 0, T - 1)] | ... | y[clamp(t + right, 0, T - 1)] ]          per utterance
    o[t][r] = b[r] + sum_i A[r][i] z[t][i]

The kernel computes o as a chain of n = in_dim float32 FMAs started at b, one rounding each.  For such a chain
(Higham, Accuracy and Stability of Numerical Algorithms, recursive summation / inner products)

    |o^ - o| <= gamma(n) (|b| + sum_i |A_i| |z_i|),   gamma(n) = n u / (1 - n u),   u = 2^-24.

The bound is derived, not measured: every output value is checked against its own bound, no factor on top.
"""
import numpy as np

U = 2.0 ** -24


def gamma(n):
    return n * U / (1.0 - n * U)


def splice(y, left, right):
    """y [T][Wd] of ONE utterance -> z [T][(left + right + 1) Wd], first and last frame replicated."""
    y = np.asarray(y)
    T = y.shape[0]
    if T == 0:
        return np.zeros((0, (left + right + 1) * y.shape[1]), y.dtype)
    t = np.arange(T)
    return np.concatenate([y[np.clip(t + c, 0, T - 1)] for c in range(-left, right + 1)], axis=1)


def xform_ref(y, A, b, left, right):
    """(o, bound), float64 [T][out_dim], from the float32 rows y of one utterance and the float32 A [out_dim][in_dim], b."""
    z = splice(np.asarray(y, np.float32), left, right).astype(np.float64)
    A = np.asarray(A, np.float32).astype(np.float64)
    b = np.zeros(A.shape[0]) if b is None else np.asarray(b, np.float32).astype(np.float64)
    assert A.shape[1] == z.shape[1]
    with np.errstate(invalid="ignore", over="ignore"):
        o = b[None, :] + z @ A.T
        bound = gamma(A.shape[1]) * (np.abs(b)[None, :] + np.abs(z) @ np.abs(A).T)
    return o, bound


def assert_xform_consistent(got, y, rows, frames, A, b, left, right, utt_xf=None, what=""):
    """Every value of `got` [total][out_dim] within its own bound of the float64 map of the twin's rows y [total][Wd];
    utterance u holds rows [rows[u], rows[u] + frames[u]) and maps with A[utt_xf[u]] (A 3-D) or A (2-D).  Rows whose
    float64 result is not finite (a one-frame utterance under CVN is 0 x inf in the twin already) must be non-finite in
    `got` too.  Prints and returns the worst err / bound."""
    A = np.asarray(A, np.float32)
    if A.ndim == 2:
        A = A[None]
    bb = None if b is None else np.asarray(b, np.float32).reshape(A.shape[0], A.shape[1])
    worst, checked = 0.0, 0
    for u, (r0, T) in enumerate(zip(rows, frames)):
        x = 0 if utt_xf is None else int(utt_xf[u])
        o, bound = xform_ref(y[r0:r0 + T], A[x], None if bb is None else bb[x], left, right)
        g = np.asarray(got[r0:r0 + T], np.float64)
        assert g.shape == o.shape, "%s: utterance %d has shape %s, expected %s" % (what, u, g.shape, o.shape)
        fin = np.isfinite(o)
        assert np.array_equal(np.isfinite(g), fin), "%s: utterance %d: non-finite values differ" % (what, u)
        err = np.abs(np.where(fin, g - np.where(fin, o, 0.0), 0.0))
        lim = np.where(fin, bound, 0.0)
        bad = err > lim
        with np.errstate(invalid="ignore", divide="ignore"):
            ratio = np.where(lim > 0, err / np.where(lim > 0, lim, 1.0), 0.0)
        worst = max(worst, float(ratio.max()) if ratio.size else 0.0)
        checked += int(fin.sum())
        assert not bad.any(), "%s: utterance %d: %d values exceed their bound (worst err / bound %.3g)" % (
            what, u, int(bad.sum()), float((err[bad] / np.maximum(lim[bad], 1e-300)).max()))
    print("%s: %d values, worst err / bound = %.3g" % (what, checked, worst))
    return worst


# ---- the kernel's tile rule, restated (mfx_xform.hip: xform_ksteps, xform_lds_bytes, xform_tile_rows) ----------------

def lds_bytes(R, width, left, right, out_dim):
    in_dim = (left + right + 1) * width
    tiles, steps = (out_dim + 15) // 16, (in_dim + 3) // 4
    ksteps = min(32 // tiles, steps)
    return 4 * (((R * out_dim + 3) & ~3) + 2 * ksteps * tiles * 64 + (R + left + right) * width + 4)


def tile_rows(width, left, right, out_dim):
    """Rows per block the launcher takes: the largest of 64 / 32 / 16 inside the 40 KB target, else inside 160 KB, else 0."""
    for cap in (40 * 1024, 160 * 1024):
        for R in (64, 32, 16):
            if lds_bytes(R, width, left, right, out_dim) <= cap:
                return R
    return 0
