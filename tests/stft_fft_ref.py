"""float64 oracle of the FFT form of the STFT log-mel front end (MFX_METHOD_STFT_LOGMEL at N = 1024 / 2048, include/mfx.h).  It
does not call the library.  TEST INFRASTRUCTURE ONLY.

Frames, samples, mel table, floor, log and post are those of tests/stft_ref.py (generic in N); the DFT is not a sum over a
rounded basis but the exact transform of the windowed frame:
  z[j]     = x[j] w[j]           (in double, w the float32 window)
  X        = np.fft.rfft(z)      (in double)
  P        = |X|^2
"""
import numpy as np

import stft_edge
import stft_ref

WHISPER, LOG10, LN = stft_ref.WHISPER, stft_ref.LOG10, stft_ref.LN

# (N, S, M, sr): the shapes the issue's margin was checked on
SHAPES = [(1024, 256, 80, 22050.0), (2048, 512, 128, 44100.0), (1024, 1024, 128, 16000.0), (2048, 2048, 1, 16000.0),
          (1024, 160, 80, 16000.0), (2048, 441, 64, 44100.0), (1024, 1, 8, 16000.0)]
# the probe shapes: (2048, 441) is none (a reflected index lands a multiple of 193 away: its separation is 0), (1024, 1) neither
PROBE_SHAPES = SHAPES[:5]
TILES = (16, 8, 4)          # frames per block of k_stft_fft_mel, descending
LDS = 160 * 1024


def shape_id(s):
    return "%d_%d_%d_%gk" % (s[0], s[1], s[2], s[3] / 1000.0)


def padded_hann(L, N):
    """The periodic Hann of L taps centred in N, zeros around it: torch.stft's placement, left pad (N - L) // 2."""
    w = np.zeros(N, np.float32)
    left = (N - L) // 2
    w[left:left + L] = stft_edge.periodic_hann(L)
    return w


def windows(N):
    """name -> float32 window of N taps: Hann, stft_edge's rect / ramp / ends, and the short Hann (800 in 1024, 1200 in 2048)."""
    w = dict(stft_edge.windows(N))
    w["short"] = padded_hann({1024: 800, 2048: 1200}[N], N)
    return w


def power(pcm, window, S):
    """[T][K1] in double."""
    w = np.asarray(window, np.float32).astype(np.float64)
    f = stft_ref.frames(pcm, w.size, S) * w[None, :]
    X = np.fft.rfft(f, axis=1)
    return X.real * X.real + X.imag * X.imag


def logmel(pcm, window, S, M, sr, low, high, post=WHISPER):
    """Rows [T][M] in double."""
    window = np.asarray(window, np.float32)
    P = power(pcm, window, S)
    w, _, _ = stft_ref.mel_table(M, window.size, sr, low, high)
    v = np.maximum(P @ w.astype(np.float64).T, stft_ref.FLOOR)
    if post == LN:
        return np.log(v)
    L = np.log10(v)
    if post == WHISPER and L.size:
        L = (np.maximum(L, L.max() - 8.0) + 4.0) / 4.0
    return L


def lds_bytes(N, S, M, R):
    """ALL the LDS of a block of k_stft_fft_mel at R frames per block, restated from the layout in mfx_stft_fft.hip: the span (or
    the finished rows) | the window | W_M^k | four FFT buffers of N / 2 complex points | the power rows | four reduction words."""
    xo = (max((R - 1) * S + N, R * M) + 3) & ~3
    return 4 * (xo + N + N + 4 * N + R * ((N // 2 + 1) | 1) + 4)


def tile_rows(N, S, M):
    return next(R for R in TILES if lds_bytes(N, S, M, R) <= LDS)
