"""Float64 oracle of the Kaldi front end's options (kaldi_flags of mfx_create_kaldi, kaldi_energy_floor), written from the formula in
include/mfx.h, method 7, "Options": the centred frame gather through Kaldi's mirror -- written with Kaldi's `while` loop, not with
the closed form the kernel uses --, the two frame energies, the energy floor and the column orders.  The mel / cepstra part of a
frame is tests/kaldi_ref.py's arithmetic, applied to the gathered frames; it rounds only where the definition rounds.  Test
infrastructure only."""
import math

import numpy as np

import kaldi_ref as KR

NO_SNIP_EDGES, USE_ENERGY, ENERGY_WINDOWED, HTK_COMPAT = 1, 2, 4, 8
SQRT2 = 1.4142135623730951


def frame_count(n, W, S, flags=0):
    if not (flags & NO_SNIP_EDGES):
        return KR.frame_count(n, W, S)
    return (n + S // 2) // S if n > 0 else 0


def mirror(s, n):
    """Kaldi's loop (feature-window.cc)."""
    while s < 0 or s >= n:
        s = -s - 1 if s < 0 else 2 * n - 1 - s
    return s


def frame_samples(n, W, S, flags, t):
    """The utterance sample index of every tap of frame t."""
    if not (flags & NO_SNIP_EDGES):
        return np.arange(t * S, t * S + W, dtype=np.int64)
    s0 = t * S + S // 2 - W // 2
    return np.array([mirror(s0 + i, n) for i in range(W)], np.int64)


def frame_index(n, W, S, flags):
    """[T][W] sample indices of every frame (the loop runs only where a tap leaves the utterance)."""
    T = frame_count(n, W, S, flags)
    if T == 0:
        return np.zeros((0, W), np.int64)
    start = np.arange(T, dtype=np.int64) * S + ((S // 2 - W // 2) if (flags & NO_SNIP_EDGES) else 0)
    idx = start[:, None] + np.arange(W, dtype=np.int64)[None, :]
    for t, i in zip(*np.nonzero((idx < 0) | (idx >= n))):
        idx[t, i] = mirror(int(idx[t, i]), n)
    return idx


def padded_twin(pcm, W, S):
    """y of exactly (T - 1) S + W samples: x gathered through the mirror from S div 2 - W div 2 on.  features(y) under snip_edges =
    true are features(x) under snip_edges = false: the same arithmetic on the same samples."""
    pcm = np.asarray(pcm, np.int16)
    T = frame_count(pcm.size, W, S, NO_SNIP_EDGES)
    if T == 0:
        return np.zeros(0, np.int16)
    s0 = S // 2 - W // 2
    return np.array([pcm[mirror(s0 + j, pcm.size)] for j in range((T - 1) * S + W)], np.int16)


def features(pcm, window, S, M, sample_rate, low, high, C=0, Q=22.0, preemph=0.97, remove_dc=True, use_power=True, flags=0,
             energy_floor=0.0):
    """Rows [T][width] in float64 under `flags`."""
    pcm = np.asarray(pcm, np.int16)
    w = np.asarray(window, np.float32).astype(np.float64)
    W = w.size
    N = KR.fft_size(W)
    idx = frame_index(pcm.size, W, S, flags)
    T = idx.shape[0]
    energy, htk = bool(flags & USE_ENERGY), bool(flags & HTK_COMPAT)
    cols = C if C > 0 else M + (1 if energy else 0)
    if T == 0:
        return np.zeros((0, cols))
    xi = pcm[idx].astype(np.int64)
    x = xi.astype(np.float64)
    if remove_dc:
        mean = (xi.sum(axis=1).astype(np.float32) / np.float32(W)).astype(np.float64)
        d = x - mean[:, None]
    else:
        d = x
    c = float(np.float32(preemph))
    e = d - c * np.concatenate([d[:, :1], d[:, :-1]], axis=1)
    zw = e * w[None, :]
    z = np.zeros((T, N))
    z[:, :W] = zw
    X = np.fft.rfft(z, axis=1)[:, :N // 2]
    P = X.real ** 2 + X.imag ** 2
    if not use_power:
        P = np.sqrt(P)
    L = np.log(np.maximum(P @ KR.mel_table(M, N, sample_rate, low, high)[0].astype(np.float64).T, KR.FLOOR))
    logE = None
    if energy:
        E = ((zw if (flags & ENERGY_WINDOWED) else d) ** 2).sum(axis=1)
        logE = np.log(np.maximum(E, KR.FLOOR))
        if energy_floor > 0.0:
            logE = np.maximum(logE, float(np.float32(math.log(float(np.float32(energy_floor))))))
    if C == 0:
        if not energy:
            return L
        return np.concatenate([L, logE[:, None]] if htk else [logE[:, None], L], axis=1)
    cep = L @ KR.dct(M, C, Q).astype(np.float64).T
    if energy:
        cep[:, 0] = logE
    if htk:
        last = cep[:, :1] if energy else cep[:, :1] * SQRT2
        cep = np.concatenate([cep[:, 1:], last], axis=1)
    return cep
