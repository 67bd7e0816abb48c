"""Energy VAD and voiced-frame selection of mfx_batch_set_vad restated in plain numpy (no GPU): the float64 threshold with
its error bound, the decision rule with float32 comparisons, and the SELECT / PACK layouts.

thr_ref's bound is derived, not tuned.  The kernel's threshold is (float)(et + ms * (S / T)) with S summed in double in an
order of its own choice:
  - any order of a double sum of T terms is within gamma_T(2^-53) * sum|e| of the exact sum (Higham, Accuracy and Stability,
    section 4.2), so ms * S / T moves by at most |ms| * gamma_T * sum|e| / T;
  - the three double operations behind it (the division, the product, the addition) each round once, and the reference's own
    three: together at most 4 * 2^-53 * (|et| + |ms * mean|) to first order with the second-order terms rounded up;
  - one rounding to float32: 2^-24 * |thr|.
As tail_ref.norm_stats_ref derives its bounds; no factor on top."""
import numpy as np

U32 = 2.0 ** -24
U64 = 2.0 ** -53


def gamma(n, u=U64):
    return n * u / (1.0 - n * u)


def thr_ref(e, et, ms):
    """(threshold in float64, bound) for the float32 column e [T] of one utterance; T = 0 gives (et, 0)."""
    e = np.asarray(e, np.float32).astype(np.float64)
    T = e.size
    et, ms = float(np.float32(et)), float(np.float32(ms))
    if T == 0:
        return et, 0.0
    with np.errstate(invalid="ignore"):
        mean = e.sum() / T
        thr = et + ms * mean
        bound = abs(ms) * gamma(T) * np.abs(e).sum() / T + 4 * U64 * (abs(et) + abs(ms * mean)) + U32 * abs(thr)
    return float(thr), float(bound)


def flags_ref(e32, thr32, ctx, p):
    """flag[t] = (float32(num) >= float32(den) * float32(p)); the window [t - ctx, t + ctx] is cut at the utterance ends; num
    counts e > thr in float32, a NaN on either side being "not greater"."""
    e32 = np.asarray(e32, np.float32)
    thr32 = np.float32(thr32)
    T = e32.size
    with np.errstate(invalid="ignore"):
        loud = (e32 > thr32).astype(np.int64)
    cum = np.concatenate([[0], np.cumsum(loud)])
    t = np.arange(T)
    lo, hi = np.maximum(t - int(ctx), 0), np.minimum(t + int(ctx), T - 1)
    num = (cum[hi + 1] - cum[lo]) if T else np.zeros(0, np.int64)
    den = hi - lo + 1
    return (num.astype(np.float32) >= den.astype(np.float32) * np.float32(p)).astype(np.uint8)


def select_ref(y, rows, frames, flags):
    """SELECT: every utterance's voiced rows at the front of its own row range, +0.0 behind them."""
    y = np.asarray(y, np.float32)
    out = np.zeros_like(y)
    for r0, T in zip(rows, frames):
        r0, T = int(r0), int(T)
        keep = y[r0:r0 + T][np.asarray(flags[r0:r0 + T], bool)]
        out[r0:r0 + keep.shape[0]] = keep
    return out


def pack_ref(y, rows, frames, flags):
    """PACK: (rows, packed_row0 [n_utt + 1]) -- the batch's voiced rows back to back, +0.0 behind them."""
    y = np.asarray(y, np.float32)
    out = np.zeros_like(y)
    keep = y[np.asarray(flags, bool)]
    out[:keep.shape[0]] = keep
    voiced = [int(np.asarray(flags[int(r0):int(r0) + int(T)], np.int64).sum()) for r0, T in zip(rows, frames)]
    return out, np.concatenate([[0], np.cumsum(voiced)]).astype(np.int64)
