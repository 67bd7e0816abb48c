"""The sliding-window CMN / CVN of mfx_batch_set_sliding_norm restated in numpy, exactly as include/mfx.h defines it: the
window rule as the loop of Kaldi's SlidingWindowCmn, the window sums as differences of the online normaliser's chunked
float64 prefix chains (onorm_ref.prefix), every operation rounded on its own (numpy's float64 operators are single IEEE
operations).  Beside the definition's bits it returns the same quantities from a direct np.longdouble sum over every window
with nothing rounded, and the bound on the difference.  Plain numpy: no GPU, no library."""
import numpy as np

import onorm_ref

same_bits = onorm_ref.same_bits
VAR_FLOOR = 1e-10


def window(T, N, min_window, center, t):
    """[ws, we) of row t of an utterance of T rows: feature-functions.cc, SlidingWindowCmnInternal, line by line."""
    if center:
        window_start = t - (N // 2)
        window_end = window_start + N
    else:
        window_start = t - N
        window_end = t + 1
    if window_start < 0:
        window_end -= window_start
        window_start = 0
    if not center:
        if window_end > t:
            window_end = max(t + 1, min_window)
    if window_end > T:
        window_start -= (window_end - T)
        window_end = T
        if window_start < 0:
            window_start = 0
    return window_start, window_end


def sliding_norm(rows, N, min_window=0, center=True, norm_vars=False, exact=True):
    """rows [T][W] float32 -> (y float32, y64, mean64, mult64, B).  y is the definition's result bit for bit.  With `exact`,
    y64 = (v - m) * mult with m, the variance (of the EXACT squares) and mult from np.longdouble sums of each window and
    nothing rounded to float32, and B the bound on |y - y64| (bound()); without it the last four are None."""
    x = np.ascontiguousarray(rows, dtype=np.float32)
    T, W = x.shape
    v = x.astype(np.float64)
    q = (x * x).astype(np.float32).astype(np.float64)
    Pv, Pq = onorm_ref.prefix(v), onorm_ref.prefix(q)
    zero = np.zeros(W)
    y = np.empty((T, W), np.float32)
    y64 = mean64 = mult64 = B = None
    if exact:
        y64, mean64, mult64, B = np.empty((T, W)), np.empty((T, W)), np.ones((T, W)), np.empty((T, W))
        vl = x.astype(np.longdouble)
    for t in range(T):
        ws, we = window(T, N, min_window, center, t)
        assert 0 <= ws <= t < we <= T
        n = we - ws
        Sw = Pv[we - 1] - (Pv[ws - 1] if ws > 0 else zero)
        Qw = Pq[we - 1] - (Pq[ws - 1] if ws > 0 else zero)
        nn = np.float64(n)
        m = Sw / nn
        mean = m.astype(np.float32)
        c = (x[t] - mean).astype(np.float32)
        if not norm_vars:
            y[t] = c
        elif n == 1:
            y[t] = np.float32(0.0)
        else:
            var = Qw / nn - m * m
            var = np.where(var < VAR_FLOOR, VAR_FLOOR, var)
            mult = (1.0 / np.sqrt(var)).astype(np.float32)
            y[t] = (c * mult).astype(np.float32)
        if exact:
            seg = vl[ws:we]
            ml = seg.sum(0) / n
            mean64[t] = ml
            if not norm_vars:
                y64[t] = vl[t] - ml
                B[t] = bound(v[t], mean64[t], 1.0)
            elif n == 1:
                y64[t], mult64[t], B[t] = 0.0, 0.0, 0.0
            else:
                e2 = (seg * seg).sum(0) / n
                varl = e2 - ml * ml
                varl = np.where(varl < VAR_FLOOR, np.longdouble(VAR_FLOOR), varl)
                mul = 1.0 / np.sqrt(varl)
                mult64[t] = mul
                y64[t] = (vl[t] - ml) * mul
                B[t] = bound(v[t], mean64[t], mult64[t], y64[t], np.asarray(e2 / varl, np.float64))
    return y, y64, mean64, mult64, B


def bound(v, mean64, mult64, y64=None, e2_over_var=None):
    """CMN: B = 2^-22 (|v| + |mean|), onorm_ref.bound with mult 1.  CVN: B = 2^-22 mult (|v| + |mean|) + |y64| 2^-25 (Q / n) /
    var: the first term is the four float32 roundings (mean, difference, multiplier, product); the second the float32
    rounding of the squares (2^-24 relative on Q / n, hence 2^-24 (Q / n) / var relative on var and half that on
    var^-1/2) passing through Q / n - m^2."""
    b = onorm_ref.bound(v, mean64, mult64)
    if y64 is not None:
        b = b + np.abs(y64) * 2.0 ** -25 * e2_over_var
    return b
