"""Reference side of the pitch track (include/mfx.h, mfx_batch_set_pitch).  Nothing here calls the library:
  nccf_ref    the NCCF rows in float64, with a bound B on |rho - rho64| for a float32 evaluation that follows the definition;
  track_ref   the track (local costs, DP, backtrace, refinement) in float32 numpy.  Every operation of it in the definition is
              a singly-rounded float32 operation, so numpy reproduces it bit for bit from the same rho rows;
  the test signals the host and GPU tests share.

The bound.  u = 2^-24, n = window, z the exact (float64) centred samples of the frame, hats the float32 values.
  m       three roundings (the conversion of the sum, c1, the product): |m^ - m| <= 3 u |m|.
  z       one subtraction: |z^ - z| <= dz = u (3 |m| + max|z|), all to first order and blown up by 1 % once.
  c       an FMA chain of n links: |c^ - sum z^ z^| <= g_n sum |z^ z^|, g_n = n u / (1 - n u) -- the "chain length times unit
          roundoff" term, at most g_n of the normaliser by Cauchy-Schwarz -- and the products' inputs moved by dz:
          dc = g_n A + dz (sum |z_j| + sum |z_{j+l}|) + n dz^2,  A = sum |z_j z_{j+l}|.
  e       float32 squares (u each), a double chain (2 Ls 2^-53 of the span's total per difference), one rounding to float32,
          inputs moved by dz:  de = 2 dz sum |z| + n dz^2 + 2 Ls 2^-53 P_total + 2 u e.
  s       two roundings on top: ds = e0 del + el de0 + de0 del + 3 u s.
  rho     |rho^ - rho| <= dc / sqrt(s - ds) + |c| (1 / sqrt(s - ds) - 1 / sqrt(s)) + 3 u |rho| (square root and division).
Where s - ds <= 0 (a frame that is silent but for rounding residue) nothing better holds than |rho^| <= 1.001 and |rho| <= 1:
B is capped at 2.01 there, and the tests say how often that happens on their inputs."""
import math

import numpy as np

U = 2.0 ** -24
DEFAULT = dict(window=400, shift=160, lag_min=40, lag_max=320)


def downmix(pcm, channels):
    """int32 mono samples as the front ends form them: (L + R) >> 1 for stereo."""
    x = np.asarray(pcm, np.int16).astype(np.int32).reshape(-1)
    if channels == 2:
        return (x[0::2] + x[1::2]) >> 1
    return x


def frame_count(n, window, shift):
    """mfx_batch_frames of the framed methods, clamped at 0."""
    return max(0, (n - (window - shift)) // shift) if n >= window else 0


def nccf_ref(p, T, shift, window, lag_min, lag_max, ballast):
    """rho64 [T][K] and the bound B [T][K] for mono int samples p of one utterance."""
    K, Ls, n = lag_max - lag_min + 1, window + lag_max, window
    x = np.zeros(max((T - 1) * shift + Ls, 0) if T > 0 else 0, np.float64)
    m = min(x.size, len(p))
    x[:m] = np.asarray(p[:m], np.float64)
    lags = np.arange(lag_min, lag_max + 1)
    rho, B = np.zeros((T, K)), np.zeros((T, K))
    gam = n * U / (1 - n * U)
    ballast = float(np.float32(ballast))
    for t in range(T):
        seg = x[t * shift:t * shift + Ls]
        mean = seg.sum() / (32768.0 * Ls)
        z = seg / 32768.0 - mean
        az = np.abs(z)
        P = np.concatenate(([0.0], np.cumsum(z * z)))
        S = np.concatenate(([0.0], np.cumsum(az)))
        e0, el = P[window], P[lags + window] - P[lags]
        s1_0, s1_l = S[window], S[lags + window] - S[lags]
        c = np.correlate(z[lag_min:lag_max + window], z[:window], "valid")
        A = np.correlate(az[lag_min:lag_max + window], az[:window], "valid")
        dz = 1.01 * U * (3 * abs(mean) + az.max())
        dc = 1.01 * (gam * A + dz * (s1_0 + s1_l) + n * dz * dz)
        de_abs = 2 * Ls * 2.0 ** -53 * P[-1]
        de0 = 1.01 * (2 * dz * s1_0 + n * dz * dz + de_abs + 2 * U * e0)
        del_ = 1.01 * (2 * dz * s1_l + n * dz * dz + de_abs + 2 * U * el)
        s = e0 * el + ballast
        ds = 1.01 * (e0 * del_ + el * de0 + de0 * del_ + 3 * U * s)
        s_lo = s - ds
        ok = s_lo > 0
        r = np.where(s > 0, c / np.sqrt(np.where(s > 0, s, 1.0)), 0.0)
        inv_lo = 1.0 / np.sqrt(np.where(ok, s_lo, 1.0))
        inv = 1.0 / np.sqrt(np.where(ok, s, 1.0))
        b = 1.01 * (dc * inv_lo + np.abs(c) * (inv_lo - inv) + 3 * U * np.abs(r))
        rho[t], B[t] = r, np.minimum(np.where(ok, b, np.inf), 2.01)
    return rho, B


def tables(lag_min, lag_max, lag_cost):
    """wt, lg: double, rounded once."""
    l = np.arange(lag_min, lag_max + 1, dtype=np.float64)
    wt = (1.0 - float(np.float32(lag_cost)) * l / float(lag_max)).astype(np.float32)
    lg = np.array([math.log(v) for v in l], np.float64).astype(np.float32)
    return wt, lg


def resolve_jump(K, max_jump):
    top = max(K - 1, 1)
    return top if max_jump == 0 else min(max_jump, top)


def track_ref(rho, lag_min, lag_max, lag_cost, penalty, max_jump):
    """(lag [T] float32, rho [T] float32, index [T] int32) from rho rows [T][K] float32, in float32 throughout."""
    rho = np.asarray(rho, np.float32)
    T, K = rho.shape
    assert K == lag_max - lag_min + 1
    J = resolve_jump(K, max_jump)
    wt, lg = tables(lag_min, lag_max, lag_cost)
    pen = np.float32(penalty)
    one = np.float32(1.0)
    ks = np.arange(K)
    bp = np.zeros((T, K), np.int32)
    fwd = np.zeros(K, np.float32)
    inf = np.float32(np.inf)
    # tr[o + J][k] for k' = k + o (inf where k' is outside the states)
    tr = np.full((2 * J + 1, K), inf, np.float32)
    for o in range(-J, J + 1):
        kk = ks + o
        v = (kk >= 0) & (kk < K)
        d = lg[ks[v]] - lg[kk[v]]
        tr[o + J, v] = (pen * d) * d
    for t in range(T):
        loc = one - rho[t] * wt
        if t == 0:
            a = loc
        else:
            best = np.full(K, inf, np.float32)
            bk = np.zeros(K, np.int32)
            padded = np.concatenate((np.full(J, inf, np.float32), fwd, np.full(J, inf, np.float32)))
            for o in range(-J, J + 1):
                cand = padded[J + o:J + o + K] + tr[o + J]
                take = cand < best
                best = np.where(take, cand, best)
                bk = np.where(take, ks + o, bk)
            a = loc + best
            bp[t] = bk
        fwd = a - a[int(np.argmin(a))]
    lag, r, idx = np.zeros(T, np.float32), np.zeros(T, np.float32), np.zeros(T, np.int32)
    if T == 0:
        return lag, r, idx
    k = int(np.argmin(fwd))
    half, lim = np.float32(0.5), np.float32(0.5)
    for t in range(T - 1, -1, -1):
        delta = np.float32(0.0)
        if 0 < k < K - 1:
            a_, b_, c_ = rho[t, k - 1], rho[t, k], rho[t, k + 1]
            den = (a_ - b_) + (c_ - b_)
            if den < 0:
                delta = (half * (a_ - c_)) / den
                delta = min(max(delta, -lim), lim)
        idx[t], r[t] = k, rho[t, k]
        lag[t] = np.float32(lag_min + k) + np.float32(delta)
        if t > 0:
            k = int(bp[t, k])
    return lag, r, idx


# ---- signals ------------------------------------------------------------------------------------------------------------------

def glide(n=16000, rate=16000.0, f_start=120.0, f_end=180.0, dc=0.05, noise=0.02, seed=7):
    """Five harmonics of a linear f0 glide, a DC offset and noise.  Returns (pcm int16, f0 [n])."""
    rng = np.random.default_rng(seed)
    f0 = np.linspace(f_start, f_end, n)
    phase = 2 * np.pi * np.cumsum(f0) / rate
    amps = (0.5, 1.0, 0.7, 0.5, 0.3)
    x = sum(a * np.sin((h + 1) * phase + 0.7 * h) for h, a in enumerate(amps))
    x = 0.18 * x / max(amps) + dc + noise * rng.standard_normal(n)
    return np.clip(np.round(32768.0 * x), -32768, 32767).astype(np.int16), f0


def voiced(n, seed, f0=140.0, level=0.2, rate=16000.0):
    """A harmonic signal with some noise: an ordinary utterance of n samples."""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / rate
    f = f0 * (1.0 + 0.1 * np.sin(2 * np.pi * 1.3 * t + seed))
    ph = 2 * np.pi * np.cumsum(f) / rate
    x = level * (np.sin(ph) + 0.6 * np.sin(2 * ph + 1.0) + 0.3 * np.sin(3 * ph + 2.0)) / 1.9 + 0.01 * rng.standard_normal(n) + 0.01
    return np.clip(np.round(32768.0 * x), -32768, 32767).astype(np.int16)


def loud(n, seed):
    """Full-scale noise: the neighbour a zero fill must never read."""
    rng = np.random.default_rng(seed)
    return rng.integers(-32768, 32768, n).astype(np.int16)


def ragged_batch(lengths, first_offset=1, channels=1, seed=100):
    """Utterances of the given lengths (samples per channel) at odd sample offsets, each followed directly by a loud neighbour
    that belongs to no utterance.  Returns (pcm int16 [total * channels], offsets, lengths, utterances)."""
    parts, offs, utts = [loud(first_offset * channels, seed)], [], []
    pos = first_offset
    for i, n in enumerate(lengths):
        u = voiced(n * channels, seed + 1 + i) if n else np.zeros(0, np.int16)
        if channels == 2 and n:   # two different channels
            u = u.copy()
            u[1::2] = voiced(n, seed + 50 + i, f0=140.0, level=0.1)
        gap = 2 * (5 + i) + (1 if (pos + n) % 2 == 0 else 0)   # the next offset is odd again
        offs.append(pos)
        utts.append(u)
        parts += [u, loud(gap * channels, seed + 200 + i)]
        pos += n + gap
    pcm = np.concatenate(parts)
    if (pcm.size // channels) % 2:
        pcm = np.concatenate((pcm, loud(channels, seed + 999)))
    return pcm, np.array(offs, np.int64), np.array(lengths, np.int64), utts


def square(n):
    """Full-scale square wave, period 100 samples."""
    return np.where((np.arange(n) // 50) % 2 == 0, 32767, -32768).astype(np.int16)


# ---- the batches the host and GPU tests share: 16 kHz, handles of window_size 400 ------------------------------------------------
# lengths in samples per channel.  "ragged": no frame (0, 399), one frame, a few, 63 / 64 / 65 frames (k_pitch_nccf takes 64
# frames per tile at this shape), a second of signal.  The others: one shape each, two utterances (a tail of a few frames).
SHAPES = {
    "ragged": dict(DEFAULT, lengths=[0, 399, 400, 1000, 10479, 10480, 10640, 16001]),
    "k1": dict(window=400, shift=160, lag_min=100, lag_max=100, lengths=[2000, 700]),
    "k37": dict(window=400, shift=160, lag_min=40, lag_max=76, lengths=[3001, 401]),
    "k281": dict(DEFAULT, lengths=[2500]),
    "k512": dict(window=1024, shift=160, lag_min=513, lag_max=1024, lengths=[4000, 1024]),
    "w32": dict(window=32, shift=160, lag_min=2, lag_max=40, lengths=[1500, 450]),
    "stereo": dict(DEFAULT, channels=2, lengths=[3000, 1001]),
    "shift1": dict(DEFAULT, shift=1, lengths=[431, 400]),
    "signals": dict(DEFAULT, lengths=[2000, 2000, 2000], signals=("square", "silence", "dc")),
    "signals_ballast": dict(DEFAULT, ballast=1e-3, lengths=[2000, 2000, 2000], signals=("square", "silence", "dc")),
}
_BATCHES = {}


def shape_batch(name):
    """(pcm, offsets, lengths, utterances) of SHAPES[name]: built once, read-only."""
    if name not in _BATCHES:
        c = SHAPES[name]
        b = ragged_batch(c["lengths"], channels=c.get("channels", 1), seed=100 + 7 * list(SHAPES).index(name))
        if "signals" in c:
            pcm, offs, lens, utts = b
            pcm = pcm.copy()
            for i, kind in enumerate(c["signals"]):
                u = {"square": square(lens[i]), "silence": np.zeros(lens[i], np.int16), "dc": np.full(lens[i], 1638, np.int16)}[kind]
                pcm[offs[i]:offs[i] + lens[i]] = u
                utts[i] = u
            b = (pcm, offs, lens, utts)
        for a in (b[0], *b[3]):
            a.setflags(write=False)
        _BATCHES[name] = b
    return _BATCHES[name]
