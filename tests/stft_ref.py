"""float64 oracle of the STFT log-mel front end (MFX_METHOD_STFT_LOGMEL, include/mfx.h).  It does not call the library.

Per utterance of n samples (N = DFT length, S = hop, M = bands, K1 = N / 2 + 1):
  frames   T = 0 when n <= N / 2, else n // S; frame t, tap j reads sample t S + j - N / 2, i < 0 -> -i, i >= n -> 2 (n - 1) - i
  samples  x = pcm / 32768
  basis    the DOUBLE values of the float32 basis: float32(w[j] cos(2 pi ((k j) mod N) / N)), float32(-w[j] sin(...))
  DFT      re, im = direct sums over the taps, in double
  power    P = re^2 + im^2
  mel      the Slaney table (librosa filters.mel(htk=False, norm="slaney")), its float32 values, applied in double
  log      log10(max(mel, float32(1e-10)))  (LN: the natural log)
  WHISPER  L = max(L, max over the utterance - 8), out = (L + 4) / 4
"""
import numpy as np

WHISPER, LOG10, LN = 0, 1, 2
FLOOR = float(np.float32(1e-10))


def frame_count(n, N, S):
    return 0 if n <= N // 2 else n // S


def frame_index(n, N, S):
    """[T][N] sample index of every tap of every frame, reflected at the utterance's ends."""
    T = frame_count(n, N, S)
    i = np.arange(T, dtype=np.int64)[:, None] * S + np.arange(N, dtype=np.int64)[None, :] - N // 2
    i = np.where(i < 0, -i, i)
    i = np.where(i >= n, 2 * (n - 1) - i, i)
    assert T == 0 or (i.min() >= 0 and i.max() < n)
    return i


def frames(pcm, N, S):
    x = np.asarray(pcm, dtype=np.float64) / 32768.0
    return x[frame_index(x.size, N, S)] if frame_count(x.size, N, S) else np.zeros((0, N))


def basis(window):
    """[2][K1][N] float32: windowed cosine rows, negated windowed sine rows, evaluated in double and rounded once."""
    w = np.asarray(window, dtype=np.float32).astype(np.float64)
    N = w.size
    k = np.arange(N // 2 + 1, dtype=np.int64)[:, None]
    j = np.arange(N, dtype=np.int64)[None, :]
    a = 2.0 * np.pi * ((k * j) % N).astype(np.float64) / N
    return np.stack([(w * np.cos(a)).astype(np.float32), (-w * np.sin(a)).astype(np.float32)])


def dft(pcm, window, S):
    """(re, im) [T][K1] in double from the float32 basis."""
    b = basis(window).astype(np.float64)
    f = frames(pcm, b.shape[2], S)
    return f @ b[0].T, f @ b[1].T


def hz_to_mel(f):
    f = np.asarray(f, dtype=np.float64)
    return np.where(f < 1000.0, f / (200.0 / 3.0), 15.0 + np.log(np.maximum(f, 1e-300) / 1000.0) / (np.log(6.4) / 27.0))


def mel_to_hz(m):
    m = np.asarray(m, dtype=np.float64)
    return np.where(m < 15.0, m * (200.0 / 3.0), 1000.0 * np.exp((np.log(6.4) / 27.0) * (m - 15.0)))


def mel_table64(M, N, sr, low, high):
    """[M][K1] in double."""
    sr, low, high = float(np.float32(sr)), float(np.float32(low)), float(np.float32(high))
    m_lo, m_hi = float(hz_to_mel(low)), float(hz_to_mel(high))
    p = mel_to_hz(m_lo + (m_hi - m_lo) * np.arange(M + 2, dtype=np.float64) / (M + 1))
    f = np.arange(N // 2 + 1, dtype=np.float64) * sr / N
    up = (f[None, :] - p[:-2, None]) / (p[1:-1] - p[:-2])[:, None]
    down = (p[2:, None] - f[None, :]) / (p[2:] - p[1:-1])[:, None]
    return np.maximum(0.0, np.minimum(up, down)) * (2.0 / (p[2:] - p[:-2]))[:, None]


def mel_table(M, N, sr, low, high):
    """(weights [M][K1] float32, beg [M], len [M]): the table rounded once, the non-zero span of every row (len 0: none)."""
    w = mel_table64(M, N, sr, low, high).astype(np.float32)
    beg, ln = np.zeros(M, np.int32), np.zeros(M, np.int32)
    for m in range(M):
        nz = np.nonzero(w[m])[0]
        if nz.size:
            beg[m], ln[m] = nz[0], nz[-1] - nz[0] + 1
    return w, beg, ln


def logmel(pcm, window, S, M, sr, low, high, post=WHISPER):
    """Rows [T][M] in double."""
    window = np.asarray(window, dtype=np.float32)
    re, im = dft(pcm, window, S)
    P = re * re + im * im
    w, _, _ = mel_table(M, window.size, sr, low, high)
    mel = P @ w.astype(np.float64).T
    v = np.maximum(mel, FLOOR)
    if post == LN:
        return np.log(v)
    L = np.log10(v)
    if post == WHISPER and L.size:
        L = (np.maximum(L, L.max() - 8.0) + 4.0) / 4.0
    return L
