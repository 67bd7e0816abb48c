"""Float64 restatement of Kaldi's pitch features as include/mfx.h defines them (mfx_batch_set_pitch_feats, k_pitch_feats),
with the bound a float32 output is held to.

Plain numpy: it calls nothing from the library.  Per utterance of T rows (lag_t, rho_t), float32 as k_pitch_track wrote them:

    n = min(1, max(-1, rho_t)),  a = |n|
    r = -5.2 + 5.4 exp(7.5 (a - 1)) + 4.8 a - 2 exp(-10 a) + 4.2 exp(20 (a - 1)),   w_t = 1 / (1 + exp(-r))
    p_t = ln(sample_rate / lag_t)
    POV    pov_scale (pow(1.0001 - n, 0.15) - 1) + pov_offset
    NORM   pitch_scale (p_t - sum_i w_i p_i / sum_i w_i),  i = max(0, t - left) .. min(T - 1, t + right) ascending
    DELTA  delta_scale sum_{l = 1 .. D} l (p[min(T - 1, t + l)] - p[max(0, t - l)]) / (2 sum l^2)
    RAW    p_t

The bound.  The definition is in double, and an output is (float) of the double: B = 2^-24 |ref| + A.  The first term is the
one rounding to float32.  A is the absolute error by which two CORRECT double evaluations of the formulas can differ: each one
rounds every operation to within e / 2 relative (e = 2^-52) and calls an exp, ln and pow that are not correctly rounded.  The
ulp errors taken for them are the largest that any of the libraries involved states: OpenCL's double-precision limits, which
the device library is built to and which glibc's and numpy's stated errors (below 1 ulp) lie inside:

    exp  3 ulp        ln  3 ulp        pow  16 ulp          (1 ulp <= e relative)

One evaluation, to first order in e (a factor 1 + 2^-10 on the total pays for the higher orders: every relative error below
is under 2^-40).  P is the largest |p| of the utterance, N = left + right + 1 the longest window.
    p     the quotient is within e / 2 relative, which moves its ln by e / 2 absolute; the ln adds 3 e |p|:
              dp = e (1/2 + 3 P)
    w     a is exact (a float32 clamped).  7.5 (a - 1): two roundings of a value of at most 7.5, 7.5 e absolute, so
          exp(.) is within (7.5 + 3) e relative and 5.4 exp(.) <= 5.4 within 5.4 * 11 e = 59.4 e absolute; 4.8 a within
          2.4 e; 2 exp(-10 a) <= 2 within 2 (5 + 3 + 1/2) e = 17 e; 4.2 exp(20 (a - 1)) <= 4.2 within 4.2 (20 + 3 + 1/2) e
          = 98.7 e; the four additions round partial sums of at most 21.6: 4 * 10.8 e.  Together dr <= 221 e.  exp(-r) is
          within dr + 3 e relative; 1 + . and 1 / . add e / 2 each, and d ln w / d ln exp(-r) = 1 - w < 1:
              w is within EW = 225 e relative
    NORM  sw = sum w_i (1 + th_i)(1 + g_i) with |th| <= EW and |g| <= (N - 1) e / 2 (recursive summation of positive terms);
          sp = sum w_i p_i (1 + th_i)(1 + g'_i) + sum w_i dp_i with |g'| <= N e / 2 (one product more).  The quotient of
          two such sums with the same positive weights differs from the mean m by at most
              dm = P (2 EW + N e) + dp + e / 2 P          (the last: the division's own rounding)
          and the value pitch_scale (p_t - m) by |pitch_scale| (dp + dm) + e |v| (subtraction and product round once each):
              one evaluation of NORM: |pitch_scale| (2 dp + P (2 EW + (N + 1/2) e)) + e |v|
    DELTA every difference of at most 2 P is within 2 dp + e P, its product with l rounds by another l e P at most, and
          the D additions round partial sums of at most 2 P sum l: the numerator is within sum l (2 dp + (D + 2) e P).
          Scaling and dividing by den = 2 sum l^2 round once each, and sum l / den = 3 / (2 (2 D + 1)):
              one evaluation of DELTA: |delta_scale| 3 / (2 (2 D + 1)) (2 dp + (D + 2) e P) + e |v|
    POV   1.0001 - n in [0.0001, 2.0001] is within e / 2 relative, its power 0.15 within (0.075 + 16) e relative of a value
          y in [0.25, 1.11]: 17.9 e absolute; y - 1 rounds by at most e / 2 * 0.75; scale and offset round once each:
              one evaluation of POV: |pov_scale| 18.3 e + e (|pov_scale| 0.75 + |v|) <= e (19.1 |pov_scale| + |v|)
    RAW   dp
A is twice one evaluation's error (two evaluations, one on either side of the exact value), times 1 + 2^-10.  Nothing in it
is measured."""
import numpy as np

U = 2.0 ** -24
E = 2.0 ** -52
EW = 225.0 * E
POV, NORM, DELTA, RAW = 1, 2, 4, 8
KALDI = dict(columns=0, left=75, right=75, D=2, pov_scale=2.0, pov_offset=0.0, pitch_scale=2.0, delta_scale=10.0)


def n_columns(columns):
    return bin(columns if columns else 7).count("1")


def weights(rho):
    n = np.clip(np.asarray(rho, np.float32).astype(np.float64), -1.0, 1.0)
    a = np.abs(n)
    r = -5.2 + 5.4 * np.exp(7.5 * (a - 1.0)) + 4.8 * a - 2.0 * np.exp(-10.0 * a) + 4.2 * np.exp(20.0 * (a - 1.0))
    return n, 1.0 / (1.0 + np.exp(-r))


def feats_ref(lag, rho, sample_rate, columns=0, left=75, right=75, D=2, pov_scale=2.0, pov_offset=0.0, pitch_scale=2.0,
              delta_scale=10.0):
    """(ref, A), float64 [T][F] each, from the float32 track (lag [T], rho [T]) of ONE utterance.  B = U |ref| + A."""
    columns = columns if columns else 7
    lag = np.asarray(lag, np.float32).astype(np.float64).reshape(-1)
    T = lag.size
    F = n_columns(columns)
    if T == 0:
        return np.zeros((0, F)), np.zeros((0, F))
    n, w = weights(np.asarray(rho).reshape(-1))
    p = np.log(float(np.float32(sample_rate)) / lag)
    P = float(np.abs(p).max())
    dp = E * (0.5 + 3.0 * P)
    ps, po, ts, ds = (float(np.float32(v)) for v in (pov_scale, pov_offset, pitch_scale, delta_scale))
    t = np.arange(T)
    cols, errs = [], []
    if columns & POV:
        v = ps * (np.power(1.0001 - n, 0.15) - 1.0) + po
        cols.append(v)
        errs.append(E * (19.1 * abs(ps) + np.abs(v)))
    if columns & NORM:
        # the window of every row as one line of a [T][N] table, zero weight outside the utterance: the sums go ascending
        # (cumsum adds in sequence; a leading 0 + x is exact)
        N = left + right + 1
        idx = t[:, None] + np.arange(-left, right + 1)[None, :]
        ok = (idx >= 0) & (idx < T)
        idx = np.clip(idx, 0, T - 1)
        ww = np.where(ok, w[idx], 0.0)
        sw = np.cumsum(ww, axis=1)[:, -1]
        sp = np.cumsum(ww * p[idx], axis=1)[:, -1]
        v = ts * (p - sp / sw)
        cols.append(v)
        errs.append(abs(ts) * (2.0 * dp + P * (2.0 * EW + (N + 0.5) * E)) + E * np.abs(v))
    if columns & DELTA:
        num = np.zeros(T)
        for l in range(1, D + 1):
            num = num + l * (p[np.minimum(T - 1, t + l)] - p[np.maximum(0, t - l)])
        den = 2.0 * sum(l * l for l in range(1, D + 1))
        v = ds * num / den
        cols.append(v)
        errs.append(abs(ds) * 3.0 / (2.0 * (2 * D + 1)) * (2.0 * dp + (D + 2) * E * P) + E * np.abs(v))
    if columns & RAW:
        cols.append(p)
        errs.append(np.full(T, dp))
    ref = np.stack(cols, axis=1)
    A = 2.0 * (1.0 + 2.0 ** -10) * np.stack(errs, axis=1)
    return ref, A


def bound(ref, A):
    return U * np.abs(ref) + A


def check(got, lag, rho, sample_rate, scale=1.0, what="", **kw):
    """Every value of got [T][F] within scale * B of the float64 reference of the track; returns (worst err / (scale B),
    share of values that are the float32 rounding of the reference bit for bit)."""
    ref, A = feats_ref(lag, rho, sample_rate, **kw)
    got = np.asarray(got, np.float32)
    assert got.shape == ref.shape, "%s: shape %s, expected %s" % (what, got.shape, ref.shape)
    if ref.size == 0:
        return 0.0, 1.0
    assert np.isfinite(got).all(), "%s: non-finite values" % what
    B = scale * bound(ref, A)
    err = np.abs(got.astype(np.float64) - ref)
    ratio = err / B
    assert (err <= B).all(), "%s: %d values exceed the bound, worst err / B %.3g at %s" % (
        what, int((err > B).sum()), float(ratio.max()), np.unravel_index(ratio.argmax(), ratio.shape))
    same = float((got.view(np.int32) == ref.astype(np.float32).view(np.int32)).mean())
    return float(ratio.max()), same


# ---- the batch the host and GPU tests share: 16 kHz, window_size 400, shift 160; the track is cheap: window 400, lags 40 .. 76
TRACK = dict(window=400, shift=160, lag_min=40, lag_max=76, lag_cost=0.1, penalty=1.0, max_jump=16)
FRAMES = (0, 1, 2, 4, 5, 75, 76, 151, 152, 255, 256, 257, 513)
# (left, right), D and columns the ragged batch runs at
SETTINGS = ([dict(left=l, right=r, D=2, columns=15) for l, r in ((75, 75), (0, 0), (3, 0), (0, 7), (1024, 1024))] +
            [dict(left=75, right=75, D=d, columns=15) for d in (1, 16)] +
            [dict(left=75, right=75, D=2, columns=c) for c in (POV, NORM, DELTA, RAW)])
_BATCH = []


def ragged():
    """(pcm, offsets, lengths, utterances) with FRAMES frames each, at odd offsets, a full-scale neighbour behind each."""
    if not _BATCH:
        import pitch_ref as PR
        lens = [399 if f == 0 else 400 + 160 * (f - 1) + (7 * i) % 160 for i, f in enumerate(FRAMES)]
        b = PR.ragged_batch(lens, seed=4100)
        for a in (b[0], *b[3]):
            a.setflags(write=False)
        _BATCH.append(b)
    return _BATCH[0]
