"""Float64 oracle of the Kaldi front end (MFX_METHOD_KALDI), written from the formula in include/mfx.h -- not from Kaldi's or
torchaudio's code, neither of which is available here: agreement with a Kaldi binary is unmeasured.

What the definition rounds to float32 is rounded here in the same place: the frame mean (one conversion, one float32 division),
the pre-emphasis coefficient, the window and the two tables.  Everything else is double; numpy.fft.rfft computes the DFT.  The
tables use math.log / math.cos / math.sin (the C library's, as the host builders do), so that they can be compared bit for
bit after rounding.  Test infrastructure only."""
import math

import numpy as np

FLOOR = float(np.float32(2.0 ** -23))        # Kaldi's FLT_EPSILON
SILENCE = math.log(FLOOR)                    # -15.9424


def fft_size(W):
    return 128 if W <= 128 else 256 if W <= 256 else 512


def frame_count(n, W, S):
    return (n - W) // S + 1 if n >= W else 0


def povey_window(W):
    i = np.arange(W, dtype=np.float64)
    return np.power(0.5 - 0.5 * np.cos(2.0 * np.pi * i / (W - 1)), 0.85).astype(np.float32)


def hamming_window(W):
    """Kaldi's window_type=hamming."""
    i = np.arange(W, dtype=np.float64)
    return (0.54 - 0.46 * np.cos(2.0 * np.pi * i / (W - 1))).astype(np.float32)


def rect_window(W):
    return np.ones(W, np.float32)


def ramp_window(W):
    """Asymmetric, every tap distinct, both ends non-zero: 0.2 + 0.8 / W at tap 0, 1 at tap W - 1."""
    i = np.arange(W, dtype=np.float64)
    return (0.2 + 0.8 * (i + 1.0) / W).astype(np.float32)


WINDOWS = {"povey": povey_window, "hamming": hamming_window, "rect": rect_window, "ramp": ramp_window}

# the frame-start predecessor: the definition's d[0]; the two seeded faults of tests/test_kaldi_windows_host.py
PRED_FIRST, PRED_ZERO, PRED_BEFORE = "d0", "zero", "before"


def high_abs(sample_rate, high):
    """high > 0 is absolute, else Kaldi's offset from Nyquist -- from the float32 values the configuration holds."""
    sr, hi = float(np.float32(sample_rate)), float(np.float32(high))
    return hi if hi > 0.0 else sr / 2.0 + hi


def mel(f):
    return 1127.0 * math.log(1.0 + f / 700.0)


def mel_table(M, N, sample_rate, low, high):
    """(weights [M][N / 2] float32, beg [M], len [M]): the table in double, rounded once."""
    sr, lo = float(np.float32(sample_rate)), float(np.float32(low))
    K = N // 2
    ml, mh = mel(lo), mel(high_abs(sample_rate, high))
    delta = (mh - ml) / float(M + 1)
    mk = [mel(float(k) * sr / float(N)) for k in range(K)]
    w = np.zeros((M, K), np.float64)
    for m in range(M):
        l = ml + float(m) * delta
        c = l + delta
        r = l + 2.0 * delta
        for k in range(K):
            if l < mk[k] < r:
                w[m, k] = (mk[k] - l) / (c - l) if mk[k] <= c else (r - mk[k]) / (r - c)
    w32 = w.astype(np.float32)
    beg, ln = np.zeros(M, np.int32), np.zeros(M, np.int32)
    for m in range(M):
        nz = np.nonzero(w32[m])[0]
        if nz.size:
            beg[m], ln[m] = nz[0], nz[-1] - nz[0] + 1
    return w32, beg, ln


def dct(M, C, Q):
    """G [C][M] float32 = (float)(l[i] D[i][m]), in double, rounded once."""
    q = float(np.float32(Q))
    g = np.zeros((C, M), np.float64)
    for i in range(C):
        lift = 1.0 + q / 2.0 * math.sin(math.pi * float(i) / q) if q > 0.0 else 1.0
        for m in range(M):
            d = math.sqrt(1.0 / float(M)) if i == 0 else math.sqrt(2.0 / float(M)) * math.cos(math.pi / float(M) * (float(m) + 0.5) * float(i))
            g[i, m] = lift * d
    return g.astype(np.float32)


def features(pcm, window, S, M, sample_rate, low, high, C=0, Q=22.0, preemph=0.97, remove_dc=True, use_power=True, energies=False,
             predecessor=PRED_FIRST):
    """Rows [T][C or M] in float64.  energies: the mel energies before the floor and the log, [T][M].
    predecessor (tests only; the default is the definition): what e[0] takes for d[-1] -- PRED_FIRST d[0], PRED_ZERO 0,
    PRED_BEFORE the sample in front of the frame less the frame's mean (d[0] at sample 0 of the utterance)."""
    pcm = np.asarray(pcm, np.int16)
    w = np.asarray(window, np.float32).astype(np.float64)
    W = w.size
    N = fft_size(W)
    T = frame_count(pcm.size, W, S)
    cols = M if (C == 0 or energies) else C
    if T == 0:
        return np.zeros((0, cols))
    idx = np.arange(T)[:, None] * S + np.arange(W)[None, :]
    xi = pcm[idx].astype(np.int64)
    x = xi.astype(np.float64)
    if remove_dc:
        s = xi.sum(axis=1)
        assert np.abs(s).max() <= (1 << 24)        # (512 samples of 16 bits: the conversion to float32 is exact)
        mean = (s.astype(np.float32) / np.float32(W)).astype(np.float64)
        d = x - mean[:, None]
    else:
        d = x
    c = float(np.float32(preemph))
    if predecessor == PRED_FIRST:
        first = d[:, :1]
    elif predecessor == PRED_ZERO:
        first = np.zeros((T, 1))
    else:
        assert predecessor == PRED_BEFORE
        at = np.arange(T) * S - 1
        before = pcm[np.maximum(at, 0)].astype(np.float64) - (mean if remove_dc else 0.0)
        first = np.where(at >= 0, before, d[:, 0])[:, None]
    prev = np.concatenate([first, d[:, :-1]], axis=1)
    e = d - c * prev
    z = np.zeros((T, N))
    z[:, :W] = e * w[None, :]
    X = np.fft.rfft(z, axis=1)[:, :N // 2]
    P = X.real ** 2 + X.imag ** 2
    if not use_power:
        P = np.sqrt(P)
    Wm = mel_table(M, N, sample_rate, low, high)[0].astype(np.float64)
    E = P @ Wm.T
    if energies:
        return E
    L = np.log(np.maximum(E, FLOOR))
    if C == 0:
        return L
    return L @ dct(M, C, Q).astype(np.float64).T
