"""Float64 oracle of the TRAPS temporal patterns (TRAPS; TEST INFRASTRUCTURE ONLY).

Per utterance of T frames (M = num_banks, L = traps_len, H = (L - 1) / 2, K = traps_dct_len):
  x[t][m]    = log(max(sum_j T[m%2][j] v[j], 1e-30))          the log mel energies of the MFCC path (ceps_len = 0)
  u[j]       = x[clamp(t - H + j, 0, T - 1)][m], j < L        first / last frame replicated
  y[t][m][k] = sum_j B[k][j] u[j]
  B[k][j]    = (0.54 - 0.46 cos(2 pi j / (L - 1))) sqrt(2 / L) cos(pi k (j + 1/2) / L)
  row t      = y[t] band-major (column m K + k), then delta / delta-delta as for every other method
Spectrum and delta regression come from tests/plp_ref.py, the mel tables from oracle/np_restatement.py (imported, not
copied).
"""
import numpy as np

import plp_ref
from plp_ref import npr


def basis(L, K, hamming=True):
    """[K][L]: window times DCT-II in the reference's DCT convention (mfcccpu.cpp:124-135)."""
    j = np.arange(L, dtype=np.float64)
    w = 0.54 - 0.46 * np.cos(2 * np.pi * j / (L - 1)) if hamming else np.ones(L)
    k = np.arange(K, dtype=np.float64)[:, None]
    return w[None, :] * np.sqrt(2.0 / L) * np.cos(np.pi * k * (j[None, :] + 0.5) / L)


def log_mel(v, nb, W2, sr, low, high, alpha=1.0):
    """Log mel energies [T][nb] of magnitude rows v [T][W2/2 + 1]."""
    Tm, beg = npr.mel_tables(nb, W2, sr, low, high, alpha)
    v = np.asarray(v, np.float64)
    E = np.empty((v.shape[0], nb))
    for m in range(nb):
        E[:, m] = v[:, beg[m]:beg[m + 2]] @ Tm[m % 2, beg[m]:beg[m + 2]]
    return np.log(np.maximum(E, 1e-30))


def traps_statics(x, L, K, B=None):
    """Statics [T][M K] of log mel rows x [T][M]."""
    x = np.asarray(x, np.float64)
    T, M = x.shape
    if T == 0:
        return np.zeros((0, M * K))
    B = basis(L, K) if B is None else B
    H = (L - 1) // 2
    idx = np.clip(np.arange(T)[:, None] - H + np.arange(L)[None, :], 0, T - 1)  # [T][L]
    u = x[idx]                                                                  # [T][L][M]
    y = np.einsum("kj,tjm->tmk", B, u)
    return y.reshape(T, M * K)


def traps_batch(pcm, window, W, S, nb, sr, low, high, L, K, dyn, l1, l2, alpha=1.0, fft_size=0):
    """Whole-utterance TRAPS rows with delta / delta-delta."""
    W2 = fft_size or (1 << int(np.ceil(np.log2(W))))
    L, K = L or 31, K or 10
    groups = {0: 1, 1: 2, 2: 3}[dyn]
    if npr.ewc(np.asarray(pcm).size, W, S) <= 0:
        return np.zeros((0, nb * K * groups))
    v = plp_ref.spectrum(pcm, window, W, S, W2)
    c = traps_statics(log_mel(v, nb, W2, sr, low, high, alpha), L, K)
    return plp_ref.with_deltas(c, dyn, l1, l2)
