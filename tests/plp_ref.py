"""Float64 oracle of the PLP cepstra (PLP; TEST INFRASTRUCTURE ONLY).

Steps 1-8 of the definition, per frame:
  P[j] = v[j]^2, v = |rfft(frame)| / W2                       the stored magnitude of the MFCC path
  E_m  = max(sum_j T[m%2][j] P[j], 1e-30)                     np_restatement.mel_tables (alpha in force), on power
  A_m  = (e_m E_m)^(1/3), e_m at f_m = warped centres[m+1]   equal loudness, cube root
  A_0 = A_1, A_{M+1} = A_M; r_i = inverse DFT of the real even spectrum A, i = 0 .. p
  Levinson-Durbin -> a, E^p; c_0 = ln E^p; c_n = -a_n - sum_{k<n} (k/n) c_k a_{n-k}
  row = [w_1 c_1 .. w_C c_C (, c_0)], w_i = 1 + L/2 sin(pi i / L) (float32, as the MFCC lifter)
Framing, mel tables and the delta regression come from oracle/np_restatement.py (imported, not copied).
"""
import os
import sys

import numpy as np

_ORACLE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle")
if _ORACLE not in sys.path:
    sys.path.insert(0, _ORACLE)
import np_restatement as npr  # noqa: E402


def centres(nb, sr, low, high, alpha=1.0):
    """Warped filter centres in Hz, [nb + 2] (the `centers` of np_restatement.mel_tables)."""
    hz2mel = lambda f: 1127.0 * np.log(f / 700.0 + 1.0)
    mel2hz = lambda m: 700.0 * (np.exp(m / 1127.0) - 1.0)
    lo, hi = hz2mel(low), hz2mel(high)
    f = mel2hz(np.arange(nb + 2) / float(nb + 1) * (hi - lo) + lo)
    o = 2 * np.pi * f / sr
    o = o + 2 * np.arctan(((1 - alpha) * np.sin(o)) / (1 - (1 - alpha) * np.cos(o)))
    return sr * o / (2 * np.pi)


def equal_loudness(nb, sr, low, high, alpha=1.0):
    q = centres(nb, sr, low, high, alpha)[1:nb + 1] ** 2
    return (q / (q + 1.6e5)) ** 2 * (q + 1.44e6) / (q + 9.61e6)


def idft_basis(nb, p):
    """[p + 1][nb + 2]: r_i = sum_m basis[i][m] A_m."""
    N = nb + 2
    m = np.arange(N)
    w = np.where((m == 0) | (m == N - 1), 1.0, 2.0)
    i = np.arange(p + 1)[:, None]
    return w[None, :] * np.cos(np.pi * i * m[None, :] / (N - 1)) / (2.0 * (N - 1))


def lifter(C, lift):
    c = np.arange(1, C + 1, dtype=np.float32)
    L = np.float32(lift)
    pi = np.float32(np.pi)
    return (np.float32(1) + L / np.float32(2) * np.sin(pi * c / L).astype(np.float32)).astype(np.float64)


def levinson(r, p):
    """Levinson-Durbin on r[..., 0..p]: returns a [..., p + 1] (a_0 = 1) and the final error E^p."""
    r = np.asarray(r, np.float64)
    a = np.zeros(r.shape[:-1] + (p + 1,))
    a[..., 0] = 1.0
    E = r[..., 0].copy()
    for i in range(1, p + 1):
        acc = r[..., i] + np.sum(a[..., 1:i] * r[..., i - 1:0:-1], axis=-1)
        k = -acc / E
        prev = a.copy()
        for j in range(1, i):
            a[..., j] = prev[..., j] + k * prev[..., i - j]
        a[..., i] = k
        E = (1 - k * k) * E
    return a, E


def lpc_cepstrum(a, E, C):
    """c[..., 0..C] of the all-pole model E / |A(e^iw)|^2, A(z) = sum a_j z^-j (a_0 = 1)."""
    p = a.shape[-1] - 1
    c = np.zeros(a.shape[:-1] + (C + 1,))
    c[..., 0] = np.log(E)
    for n in range(1, C + 1):
        s = np.zeros(a.shape[:-1])
        for k in range(max(1, n - p), n):
            s += (k / n) * c[..., k] * a[..., n - k]
        c[..., n] = -(a[..., n] if n <= p else 0.0) - s
    return c


def spectrum(pcm, window, W, S, W2):
    """|rfft(frame)| / W2 of every frame (whole-utterance framing of np_restatement.mfcc_batch)."""
    pcm = np.asarray(pcm, dtype=np.float64)
    T = npr.ewc(pcm.size, W, S)
    idx = np.arange(T)[:, None] * S + np.arange(W)[None, :]
    x = np.zeros((T, W2))
    x[:, :W] = pcm[idx] * np.asarray(window, dtype=np.float64)[None, :]
    return np.abs(np.fft.rfft(x, axis=1)) / W2


def plp_frames(v, nb, W2, sr, low, high, p, C, want_c0, lift, alpha=1.0, want_r=False):
    """PLP statics of magnitude rows v [T][W2/2 + 1] (and the autocorrelations r [T][p + 1] with want_r)."""
    Tm, beg = npr.mel_tables(nb, W2, sr, low, high, alpha)
    P = np.asarray(v, np.float64) ** 2
    E = np.empty((P.shape[0], nb))
    for m in range(nb):
        E[:, m] = P[:, beg[m]:beg[m + 2]] @ Tm[m % 2, beg[m]:beg[m + 2]]
    E = np.maximum(E, 1e-30)
    At = np.cbrt(equal_loudness(nb, sr, low, high, alpha)[None, :] * E)
    A = np.concatenate([At[:, :1], At, At[:, -1:]], 1)
    r = A @ idft_basis(nb, p).T
    a, Ep = levinson(r, p)
    c = lpc_cepstrum(a, Ep, C)
    rows = c[:, 1:] * lifter(C, lift)[None, :]
    if want_c0:
        rows = np.concatenate([rows, c[:, :1]], 1)
    return (rows, r) if want_r else rows


def with_deltas(c, dyn, l1, l2):
    """Whole-utterance delta / delta-delta of statics c (np_restatement.mfcc_batch's tail)."""
    if dyn == 0:
        return c
    if dyn == 1:
        l2 = 0
    D = l1 + l2
    cp = np.concatenate([np.repeat(c[:1], D, 0), c, np.repeat(c[-1:], D, 0)], 0)
    T = c.shape[0]
    d_ext = npr.regress(cp, l1)
    out = [c, d_ext[l2:l2 + T]]
    if dyn == 2:
        out.append(npr.regress(d_ext, l2))
    return np.concatenate(out, 1)


def downmix(pcm):
    """Interleaved stereo int16 -> (L + R) >> 1, as the batch entry reads it."""
    x = np.asarray(pcm, np.int32).reshape(-1, 2)
    return ((x[:, 0] + x[:, 1]) >> 1).astype(np.int16)


def plp_batch(pcm, window, W, S, nb, sr, low, high, C, want_c0, lift, dyn, l1, l2, p, alpha=1.0, fft_size=0):
    """Whole-utterance PLP rows with delta / delta-delta (what a multi-block streaming run delivers)."""
    W2 = fft_size or (1 << int(np.ceil(np.log2(W))))
    v = spectrum(pcm, window, W, S, W2)
    return with_deltas(plp_frames(v, nb, W2, sr, low, high, p, C, want_c0, lift, alpha), dyn, l1, l2)
