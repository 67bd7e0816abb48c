"""The online (causal, sliding-window) CMN / CVN of mfx_batch_set_online_norm / mfx_sessions_set_online_norm restated in numpy,
exactly as include/mfx.h defines it: sequential float64 chains in chunks of 32 rows, every operation rounded on its own
(numpy's float64 operators are single IEEE operations).  Plain numpy: no GPU, no library."""
import numpy as np

CHUNK = 32
CMN, CVN = 1, 2


def prefix(a):
    """P[t] = O[t div 32] + I[t] of the [T][W] float64 array `a`: I restarts from 0 in every chunk and adds the chunk's rows in
    ascending order, O[c + 1] = O[c] + Tot[c] from O[0] = 0."""
    T, W = a.shape
    P = np.empty((T, W))
    O = np.zeros(W)
    I = np.zeros(W)
    for t in range(T):
        I = I + a[t]
        P[t] = O + I
        if t % CHUNK == CHUNK - 1:
            O = O + I
            I = np.zeros(W)
    return P


def online_norm(rows, kind, window=0, prior_frames=0, prior_count=0, prior_acc=None):
    """rows [T][W] float32 -> (y float32, y64, mean64, mult64): y is the definition's result bit for bit, y64 = (v - m) *
    mult the same value with nothing rounded to float32, mean64 = m and mult64 the unrounded multiplier (1 for CMN)."""
    x = np.ascontiguousarray(rows, dtype=np.float32)
    T, W = x.shape
    v = x.astype(np.float64)
    q = (x * x).astype(np.float32).astype(np.float64)
    Pv, Pq = prefix(v), prefix(q)
    N, F, p = int(window), int(prior_frames), int(prior_count)
    if p > 0:
        PS, PQ = np.asarray(prior_acc, np.float64).reshape(2, W)
    y = np.empty((T, W), np.float32)
    y64, mean64, mult64 = np.empty((T, W)), np.empty((T, W)), np.ones((T, W))
    for t in range(T):
        if N > 0 and t >= N:
            Sw, Qw, n = Pv[t] - Pv[t - N], Pq[t] - Pq[t - N], N
        else:
            Sw, Qw, n = Pv[t], Pq[t], t + 1
        k = min(p, F - n) if (p > 0 and F > n) else 0
        if k > 0:
            r = np.float64(k) / np.float64(p)
            Sw = Sw + PS * r
            Qw = Qw + PQ * r
        nn = np.float64(n + k)
        m = Sw / nn
        mean = m.astype(np.float32)
        c = (x[t] - mean).astype(np.float32)
        mean64[t] = m
        if kind == CVN:
            d = Qw - Sw * m
            with np.errstate(all="ignore"):
                mu = np.where((nn >= 2) & (d > 0), np.sqrt((nn - 1) / d), 1.0)
            mult64[t] = mu
            y[t] = (c * mu.astype(np.float32)).astype(np.float32)
        else:
            y[t] = c
        y64[t] = (v[t] - m) * mult64[t]
    return y, y64, mean64, mult64


def bound(rows, mean64, mult64):
    """B = 2^-22 mult (|v| + |mean|): four float32 roundings (mean, difference, multiplier, product), each at most 2^-24
    relative to a quantity no larger than mult (|v| + |mean|)."""
    return 2.0 ** -22 * mult64 * (np.abs(np.asarray(rows, np.float64)) + np.abs(mean64))


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))
