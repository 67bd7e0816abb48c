"""Sample-rate conversion in numpy float64 (include/mfx.h, "sample-rate conversion"): the filter formula, the output sums
from the float32 table the library reports, and the per-sample bound.  No code of the library or of any other project is
involved; the only library input is the table itself, which test_resample_host.py checks against `taps` below."""
from math import gcd

import numpy as np

U = 2.0 ** -24  # unit roundoff of float32


def ratio(in_hz, out_hz):
    g = gcd(int(in_hz), int(out_hz))
    return out_hz // g, in_hz // g      # L, M


def shape(in_hz, out_hz, zeros=0, rolloff=0.0):
    """(L, M, P, Wh, c) with the defaults of the interface: zeros 0 -> 6, rolloff 0 -> 0.99."""
    L, M = ratio(in_hz, out_hz)
    zeros = 6 if zeros == 0 else zeros
    ro = 0.99 if rolloff == 0 else float(np.float32(rolloff))
    c = ro * min(1.0, L / M)
    Wh = int(np.ceil(zeros / c))
    return L, M, 2 * Wh, Wh, c


def taps(in_hz, out_hz, zeros=0, rolloff=0.0):
    """h [L][P] in float64: c sinc(c t) (1 + cos(pi t / Wh)) / 2 for |t| < Wh, t = (k - Wh + 1) - phi / L."""
    L, M, P, Wh, c = shape(in_hz, out_hz, zeros, rolloff)
    t = (np.arange(P, dtype=np.float64)[None, :] - Wh + 1) - np.arange(L, dtype=np.float64)[:, None] / L
    h = c * np.sinc(c * t) * 0.5 * (1.0 + np.cos(np.pi * t / Wh))     # np.sinc(x) = sin(pi x) / (pi x), 1 at 0
    h[np.abs(t) >= Wh] = 0.0
    return h


def out_length(n_in, in_hz, out_hz):
    L, M = ratio(in_hz, out_hz)
    return (int(n_in) * L + M - 1) // M     # Python integers: exact at any size


def layout(lengths, rates, out_hz):
    offs, outs, pos = [], [], 0
    for n, r in zip(lengths, rates):
        m = out_length(n, r, out_hz)
        offs.append(pos)
        outs.append(m)
        pos += m + (m & 1)
    return offs, outs, pos


def convert(x, h32, L, M):
    """One channel of one utterance: (o, B) for every output sample.  o[j] = sum_k h32[phi][k] x[n - Wh + 1 + k] in
    float64 (x zero outside the utterance), B[j] = 0.5 + gamma_P sum_k |h32 x|, gamma_P = P u / (1 - P u): half a unit
    for the rounding to an integer plus Higham's bound for a recursive float32 sum of P products (an FMA chain rounds once
    per step, so the bound for separate products and sums covers it)."""
    x = np.asarray(x, np.float64)
    L_, P = h32.shape
    assert L_ == L
    Wh = P // 2
    n_out = (x.size * L + M - 1) // M
    j = np.arange(n_out, dtype=np.int64)
    n, phi = (j * M) // L, (j * M) % L
    xp = np.concatenate([np.zeros(Wh + 1), x, np.zeros(Wh + 1)])
    idx = (n - Wh + 1)[:, None] + np.arange(P)[None, :] + (Wh + 1)    # into xp; n <= N_in - 1 keeps it inside
    prod = h32.astype(np.float64)[phi] * xp[idx]
    gam = P * U / (1.0 - P * U)
    return prod.sum(1), 0.5 + gam * np.abs(prod).sum(1)


def to_pcm(o):
    return np.clip(np.rint(o), -32768, 32767).astype(np.int16)
