"""Edge signals for the MFCC front ends, their float64 reference and the bars they are held to (TEST INFRASTRUCTURE ONLY).

Signals: what Gaussian noise at sigma = 3000 never produces -- exact zeros, the two ends of the int16 range on every sample,
+-1 LSB, an impulse on every window tap, silence around a burst, frames that are all alike ("Edge signals").
Reference: the whole-utterance formulas in float64, assembled from plp_ref.downmix / plp_ref.spectrum (framing with an explicit
transform length) and np_restatement.mel_tables / dct_matrix; no table is restated here.
Yardstick: an absolute bar on the log mel energies that a float32 transform can resolve (see "conditioning" below); the cepstra
of nearly constant log energies are cancelled sums of -69.08, so their errors are measured against max |log mel energy| of the
utterance, the scale of the DCT's input (conftest.assert_close, scale_floor).
"""
import functools
import os
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (_HERE, os.path.join(os.path.dirname(_HERE), "oracle")):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import np_restatement as npr  # noqa: E402
import plp_ref  # noqa: E402
from conftest import TOL_MAX, TOL_L2, assert_close  # noqa: E402

# The two constants are derived from the checker's own distance to float64 (liboracle.so, bug_compat off, against
# reference() below), measured by tests/test_edge_signals_host.py over the 31 rows of mfcc.KERNEL_TABLE and every signal, on
# the well-conditioned entries (COND_TOL below):
#   worst |d log E| of the checker              1.285e-4  (square on the 2048-point 1102 / 441 rows; 7.2e-5 and less elsewhere)
#   worst floored relative L2 of the checker    7.835e-6  (min / max on the C3 shapes)
#   worst floored max error of the checker      2.131e-5 = 0.21 of TOL_MAX: under TOL_MAX / 4 on every row and signal
# The kernels differ from the checker by another FFT factorisation, v_log_f32 times ln 2 and a k-ordered or matrix-pipe DCT:
# three roundings of the same order and count as the checker's own, not a systematic term; hence 4 x the checker's error:
#   EDGE_TOL_LOGMEL = 4 x 1.285e-4 = 5.14e-4, rounded up to one significant digit
#   EDGE_TOL_L2     = max(TOL_L2, 4 x 7.835e-6 = 3.134e-5)
# (tests/test_edge_signals_host.py asserts both derivations.)  A half-LSB input error or a lost sign moves the log energies
# of the LSB and full-scale signals by tenths, three orders of magnitude more.
EDGE_TOL_LOGMEL = 6e-4
EDGE_TOL_L2 = 3.14e-5
assert EDGE_TOL_L2 >= TOL_L2
LOG_FLOOR = float(np.log(1e-30))            # -69.0776: the log of the mel floor
FLOOR_TOL = 2e-7 * 69.08                    # the fast log's one ulp of log2, at the floor

FRAMES = 40                                 # 2.5 chunks of 16 frames: crosses the 4-frame tail pieces
FILLER = 0x5A5A

MONO = ("zero", "min", "max", "one", "nyquist", "square", "tone_grid", "tone_off", "chirp", "lsb1", "lsb3", "impulses",
        "one_impulse", "burst", "clipped", "uniform")
STEREO = ("lr_extremes", "lr_lsb", "l_only")


def tone_grid_period(shift, sr):
    """Period in samples of `tone_grid`: the divisor of the shift (>= 4 samples, >= 100 Hz) nearest 1 kHz on a log scale;
    None where the shift has none (the tone is then 1 kHz and its frames differ)."""
    div = [d for d in range(4, shift + 1) if shift % d == 0 and sr / d >= 100.0]
    if not div:
        return None
    return min(div, key=lambda d: abs(np.log(sr / d / 1000.0)))


def _clip16(x):
    return np.clip(np.rint(x), -32768, 32767).astype(np.int16)


def signals(n, sr, channels=1, seed=0, shift=None):
    """name -> int16 array of n samples per channel (interleaved for stereo).  Deterministic in (n, sr, channels, seed, shift).
    Stereo: the deterministic signals are the same on both channels (their downmix is the mono signal), the random ones are
    drawn independently per channel; lr_extremes, lr_lsb and l_only exist for stereo only."""
    rng = np.random.default_rng(0xED6E0000 + seed)
    t = np.arange(n)
    ch = channels

    def both(x):                 # the same samples on every channel
        return np.repeat(np.asarray(x, np.int16), ch)

    def draw(f):                 # independent samples per channel
        return np.asarray(f(n * ch), np.int16)

    out = {}
    out["zero"] = both(np.zeros(n))
    out["min"] = both(np.full(n, -32768))
    out["max"] = both(np.full(n, 32767))
    out["one"] = both(np.ones(n))
    out["nyquist"] = both(np.where(t % 2 == 0, 32767, -32768))
    out["square"] = both(np.where((t // 23) % 2 == 0, 32767, -32768))
    period = tone_grid_period(shift, sr) if shift else None
    if period:                   # from the phase within the period: exactly periodic (32767 sin 30 deg is 16383.5)
        out["tone_grid"] = both(_clip16(32767.0 * np.sin(2 * np.pi * (t % period) / period)))
    else:
        out["tone_grid"] = both(_clip16(32767.0 * np.sin(2 * np.pi * 1000.0 * t / sr)))
    out["tone_off"] = both(_clip16(32767.0 * np.sin(2 * np.pi * (1234.5 * sr / 16000.0) * t / sr)))
    f0, f1 = 50.0, 0.99 * sr / 2
    out["chirp"] = both(_clip16(30000.0 * np.sin(2 * np.pi * (f0 * t + (f1 - f0) * t * t / (2.0 * n)) / sr)))
    out["lsb1"] = draw(lambda k: rng.integers(-1, 2, k))
    out["lsb3"] = draw(lambda k: rng.integers(-3, 4, k))
    imp = np.zeros(n, np.int32)
    imp[0::997] = 32767
    imp[500::1994] = -32768
    out["impulses"] = both(imp)
    one = np.zeros(n, np.int32)
    one[n // 2 + 3] = 32767
    out["one_impulse"] = both(one)
    burst = np.zeros(n * ch, np.float64)
    b0 = (n // 2 - 400) * ch
    burst[b0:b0 + 800 * ch] = 3000.0 * rng.standard_normal(800 * ch)
    out["burst"] = _clip16(burst)
    out["clipped"] = draw(lambda k: _clip16(40000.0 * rng.standard_normal(k)))
    out["uniform"] = draw(lambda k: rng.integers(-32768, 32768, k))
    if ch == 2:
        cyc = np.array([[-32768, -32768], [32767, 32767], [32767, -32768], [-32768, 32767]], np.int16)
        out["lr_extremes"] = cyc[t % 4].reshape(-1)
        out["lr_lsb"] = rng.integers(-1, 2, 2 * n).astype(np.int16)
        lo = rng.integers(-32768, 32768, 2 * n).astype(np.int16)
        lo[1::2] = 0
        out["l_only"] = lo
    assert list(out) == list(MONO) + (list(STEREO) if ch == 2 else [])
    assert all(v.dtype == np.int16 and v.size == n * ch for v in out.values())
    return out


def identical_frame_signals(shift, sr, channels=1):
    """The signals whose frames all hold the same samples (nyquist at an odd shift: see identical_stride)."""
    names = ["zero", "min", "max", "one", "nyquist"]
    if tone_grid_period(shift, sr) is not None:
        names.append("tone_grid")
    if channels == 2 and shift % 4 == 0:
        names.append("lr_extremes")
    return names


def identical_stride(name, shift):
    """Frames t and t + stride of an identical-frame signal hold the same samples.  2 for nyquist at an odd shift: a frame
    that starts on an odd sample reads -32768, 32767, ..., which is not the negation of 32767, -32768, ..."""
    return 2 if name == "nyquist" and shift % 2 else 1


def utterance_length(W, S, index):
    """W + 39 S + r samples, r < S fixed per signal: FRAMES frames and a ragged end."""
    return W + (FRAMES - 1) * S + (7 * index + 3) % S


_mel_tables = functools.lru_cache(maxsize=8)(npr.mel_tables)       # (a reference() per signal: the same tables)


def reference(pcm, window, W, S, fft_size, nb, sr, low, high, nc, c0, lift, alpha=1.0, channels=1):
    """(cepstra -- the log mel energies where nc == 0 --, log mel energies) of every frame, float64.  `pcm` may hold
    integers outside int16 (mono): the mutants of tests/test_edge_signals_host.py feed such samples."""
    x = plp_ref.downmix(pcm) if channels == 2 else np.asarray(pcm)
    W2 = fft_size or (1 << int(np.ceil(np.log2(W))))
    v = plp_ref.spectrum(x, window, W, S, W2)
    Tm, beg = _mel_tables(nb, W2, sr, low, high, alpha)
    E = np.empty((v.shape[0], nb))
    for m in range(nb):
        E[:, m] = v[:, beg[m]:beg[m + 2]] @ Tm[m % 2, beg[m]:beg[m + 2]]
    mel = np.log(np.maximum(E, 1e-30))
    return (mel @ npr.dct_matrix(nb, nc, c0, lift) if nc > 0 else mel), mel


# ---- conditioning ------------------------------------------------------------------------------------------------------------
# Not every log mel energy of these signals is a property of the signal.  A constant, a Nyquist alternation or a tone put all
# their energy into a few bins; what the far filters collect is window leakage 80 dB and more below the peak -- where the
# window fills the transform (W = W2: its periodic raised cosine has three non-zero bins) or a filter spans a single bin in a
# spectral null, exactly nothing.  A float32 transform is backward stable, not exact: its result is the exact transform of
# samples moved by about u log2(W2) of their size (u = 2^-24; Higham, Accuracy and Stability, thm 24.2), and that white
# perturbation lies level across all bins.  The checker does not show this: its transform runs in double precision.
# sensitivity() applies two such perturbations (relative, uniform in +-u log2 W2, on samples and window taps) to the float64
# reference and records how far each log mel energy moves.  Entries that move by more than COND_TOL are rounding noise of ANY
# float32 front end and are not held to the float64 value (they must be finite); rows holding such an entry are not held to
# the float64 cepstra (tests/test_edge_signals_gpu.py checks their DCT against the kernel's own log mel energies instead).
# The bit-for-bit checks do not depend on any of this.  COND_TOL is fixed, not derived from the bars it guards.
COND_TOL = 2.5e-5


def sensitivity(mono, window, **shape):
    """[T][nb]: the largest move of each float64 log mel energy under two float32-transform-sized perturbations."""
    W2 = shape["fft_size"] or (1 << int(np.ceil(np.log2(shape["W"]))))
    eps = 2.0 ** -24 * np.log2(W2)
    mel = reference(mono, window, **shape)[1]
    x, w = np.asarray(mono, np.float64), np.asarray(window, np.float64)
    sens = np.zeros_like(mel)
    for k in range(2):
        rng = np.random.default_rng(0xC09D + k)
        xp = x * (1.0 + eps * rng.uniform(-1.0, 1.0, x.size))
        wp = w * (1.0 + eps * rng.uniform(-1.0, 1.0, w.size))
        sens = np.maximum(sens, np.abs(reference(xp, wp, **shape)[1] - mel))
    return sens


def logmel_errors(got, want, ok=None):
    """(max |got - want| off the floor, max |got - want| on entries where want is the floor), over the entries `ok`."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, "shape %s vs %s" % (got.shape, want.shape)
    ok = np.ones(want.shape, bool) if ok is None else np.asarray(ok, bool)
    d = np.abs(got - want)
    floor = want == LOG_FLOOR
    a, b = ok & ~floor, ok & floor
    return (float(d[a].max()) if a.any() else 0.0), (float(d[b].max()) if b.any() else 0.0)


def assert_logmel_close(got, want, what="", tol=None, ok=None):
    """max |got - want| <= EDGE_TOL_LOGMEL over the well-conditioned entries `ok` (None: all); entries whose reference is the
    1e-30 floor to FLOOR_TOL; every entry finite."""
    tol = EDGE_TOL_LOGMEL if tol is None else tol
    assert np.isfinite(np.asarray(got)).all(), "%s: non-finite log mel energies" % what
    e, ef = logmel_errors(got, want, ok)
    assert e <= tol, "%s: max |d log E| = %.3g > %.3g" % (what, e, tol)
    assert ef <= FLOOR_TOL, "%s: entries on the 1e-30 floor differ by %.3g > %.3g" % (what, ef, FLOOR_TOL)
    return e


def rows_errors(got, want, logmel, groups=None):
    """(max err / scale, rel L2) of conftest.assert_close with scale_floor = max |logmel|, worst over the column groups."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    if got.size == 0:
        return 0.0, 0.0
    floor = float(np.abs(logmel).max())
    g = groups or 1
    w = want.shape[1] // g
    emax = el2 = 0.0
    for i in range(g):
        a, b = got[:, i * w:(i + 1) * w], want[:, i * w:(i + 1) * w]
        emax = max(emax, np.abs(a - b).max() / max(np.abs(b).max(), 1e-30, floor))
        el2 = max(el2, np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30, floor * np.sqrt(b.size)))
    return float(emax), float(el2)


def assert_rows_close(got, want, logmel, what="", groups=None, tol_max=TOL_MAX, tol_l2=None):
    """conftest.assert_close with scale_floor = max |logmel|, tol_max = TOL_MAX (the project's) and tol_l2 = EDGE_TOL_L2."""
    assert_close(got, want, what, tol_max=tol_max, tol_l2=EDGE_TOL_L2 if tol_l2 is None else tol_l2, groups=groups,
                 scale_floor=float(np.abs(logmel).max()))
    return rows_errors(got, want, logmel, groups)


# ---- rows of mfcc.KERNEL_TABLE ---------------------------------------------------------------------------------------------

def row_shape(kw):
    """The keywords of a KERNEL_TABLE row as the arguments of reference() and of the handles (low 64 Hz, high sr / 2,
    lifter 22: plan_kernel's defaults)."""
    sr = float(kw["sample_rate"])
    return dict(W=kw["window_size"], S=kw["shift"], fft_size=kw.get("fft_size", 0), nb=kw["num_banks"], sr=sr, low=64.0,
                high=sr / 2, nc=kw["ceps_len"], c0=bool(kw.get("want_c0", False)), lift=22.0, channels=kw.get("channels", 1))


def row_id(what):
    return "-".join(what.replace(",", " ").replace(":", " ").replace("/", " ").replace("(", " ").replace(")", " ").split()[:6])


def row_signals(shape, seed=0):
    """The utterances of a row: name -> int16 array of utterance_length() samples per channel."""
    W, S, ch = shape["W"], shape["S"], shape["channels"]
    names = list(MONO) + (list(STEREO) if ch == 2 else [])
    out = {}
    for i, name in enumerate(names):
        n = utterance_length(W, S, i)
        out[name] = signals(n, shape["sr"], ch, seed, shift=S)[name]
    return out


def mono_of(pcm, channels):
    return plp_ref.downmix(pcm) if channels == 2 else np.asarray(pcm)


_ROWS = {}


def row_reference(kw, window):
    """Per signal of a row: dict(pcm, mono, c, mel, ok) -- the float64 cepstra and log mel energies of every frame and the
    mask of well-conditioned entries.  Computed once per row, shared by the tests of a run, never changed."""
    key = tuple(sorted(kw.items()))
    if key in _ROWS:
        return _ROWS[key]
    shape = row_shape(kw)
    args = {k: v for k, v in shape.items() if k != "channels"}
    out = {}
    for name, pcm in row_signals(shape).items():
        mono = mono_of(pcm, shape["channels"])
        c, mel = reference(mono, window, **args)
        ok = sensitivity(mono, window, **args) <= COND_TOL
        for a in (pcm, mono, c, mel, ok):
            a.setflags(write=False)
        out[name] = dict(pcm=pcm, mono=mono, c=c, mel=mel, ok=ok)
    _ROWS[key] = out
    return out
