"""Windows beyond Hann, edge and probe signals, a float32 checker and the bars for the STFT log-mel front end (k_stft_mel,
k_stft_post, k_sess_stft_mel).  TEST INFRASTRUCTURE ONLY; no GPU, no call into the library.

Why: periodic_hann(N) has w[0] == 0.0 exactly and weighs taps 1..3 and N-3..N-1 with 6e-5 to 5.5e-4, so the first and the
last matrix step of stft_dft_power (4 taps each) add about 4e-6 of a frame's amplitude; at conftest.assert_close's bar a
kernel that drops, zeroes or misreads them passes (tests/test_stft_edge_host.py lists the mutants that do).  The windows here
give those taps weight:
  hann   the library's periodic Hann
  rect   all ones
  ramp   w[j] = (j + 1) / N: asymmetric, a reversed or shifted tap order shows
  ends   ones on taps 0..3 and N-4..N-1, zero elsewhere: the result comes from the two outer matrix steps alone
  onehot(N, j): with probe_signal() every row is 2 log10|x[i]| + log10(row sum) of ONE sample, so the row names the sample
Reference: tests/stft_ref.py (float64).  Yardstick: absolute bars in log10 units on the entries a float32 DFT can resolve
(sensitivity(), the construction of edge_signals.sensitivity), exact -10.0f where the reference is the 1e-10 floor.
"""
import functools

import numpy as np

import edge_signals as ES
import stft_ref

LOG10, LN, WHISPER = stft_ref.LOG10, stft_ref.LN, stft_ref.WHISPER

# (N, S, M, sr, low, high).  Blocks of k_stft_mel: 64 frames but 512/512 and 396/336 (32) -- and 16 nowhere in the method's
# range of shapes with these M: see test_stft_edge_host.test_block_rows_of_the_shapes, which asserts what occurs.
SHAPES = [(400, 160, 80, 16000.0, 0.0, 8000.0),       # the default
          (34, 5, 6, 16000.0, 0.0, 8000.0),           # the smallest N % 4 == 2 shape
          (414, 138, 40, 16000.0, 0.0, 8000.0),       # the last single-pass DFT (N % 4 == 2)
          (416, 104, 40, 16000.0, 0.0, 8000.0),       # the first two-pass DFT: the second pass holds the Nyquist bin alone
          (510, 170, 40, 16000.0, 0.0, 8000.0),
          (512, 512, 128, 16000.0, 0.0, 8000.0),
          (396, 336, 8, 16000.0, 0.0, 8000.0),        # 32-frame blocks
          (200, 80, 40, 8000.0, 300.0, 3400.0)]       # low > 0, high < sr / 2
WINDOWS = ("hann", "rect", "ramp", "ends")
FLOOR_L10 = np.float32(-10.0)                         # the kernel's exact value at the 1e-10 floor (LOG10)
FLOOR_WANT = float(np.log10(stft_ref.FLOOR))          # the oracle's: log10 of the float32 nearest 1e-10, -10 + 5.8e-9
FLOOR_LN = np.float32(np.log(np.float64(np.float32(1e-10))))


def shape_id(shape):
    return "%d_%d_%d_%gk" % (shape[0], shape[1], shape[2], shape[3] / 1000.0)


# ---- windows ---------------------------------------------------------------------------------------------------------

def periodic_hann(N):
    """mfcc.periodic_hann restated (tests/test_stft_edge_host.py holds the two equal)."""
    return (0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(N, dtype=np.float64) / N)).astype(np.float32)


def onehot(N, j):
    w = np.zeros(N, np.float32)
    w[j] = 1.0
    return w


def windows(N):
    ends = np.zeros(N, np.float32)
    ends[:4] = ends[N - 4:] = 1.0
    return {"hann": periodic_hann(N), "rect": np.ones(N, np.float32),
            "ramp": ((np.arange(N, dtype=np.float64) + 1.0) / N).astype(np.float32), "ends": ends}


# ---- signals ---------------------------------------------------------------------------------------------------------

def utterance_length(N, S, index):
    """max(N + 39 S, 800) + r samples, r < S fixed per signal (800: edge_signals' burst needs them)."""
    return max(N + (ES.FRAMES - 1) * S, 800) + (7 * index + 3) % S


def edge_utterances(shape, seed=0):
    """name -> int16 utterance: edge_signals.signals unchanged, every signal at its own ragged length."""
    N, S, sr = shape[0], shape[1], shape[3]
    return {name: ES.signals(utterance_length(N, S, i), sr, 1, seed, shift=S)[name] for i, name in enumerate(ES.MONO)}


PROBE_PERIOD = 193
PROBE_SEPARATION = 0.01          # least distance, in 2 log10|x|, between the probed sample and every sample a wrong index reads


def probe_value(i):
    """Sample i of the probe signal for ANY integer i: sign(i) rint(600 x 1.02^(i mod 193)), 600 .. 26877; neighbours differ
    by 2 log10(1.02) = 0.0172 in 2 log10|x| (the wrap 26877 -> 600 by 3.3), so a row under a one-hot window names its sample
    up to the period.  The signs (a fixed pattern of period 7) do not reach the power; they keep a sum of taps from being one."""
    i = np.asarray(i, np.int64)
    sign = np.where((i % 7) % 3 == 1, -1.0, 1.0)
    return (sign * np.rint(600.0 * 1.02 ** (i % PROBE_PERIOD).astype(np.float64))).astype(np.int16)


def probe_signal(n, start=0):
    """n samples of the probe from its sample `start` on (streams that share a session slot start at different samples)."""
    return probe_value(np.arange(n) + start)


def probe_taps(N):
    return [0, 1, 3, 4, N // 2 - 1, N // 2, N - 5, N - 4, N - 2, N - 1]


def probe_lengths(N, S, R):
    """Samples of the probe utterances of a shape whose blocks hold R frames."""
    return [N // 2 + 1, N // 2 + 2, 15 * S + 1, 16 * S, 17 * S + 3, (R + 1) * S + 1]


def probe_decode(row_value, rowsum_log10):
    """The residue i mod 193 of the sample a one-hot row of value L = 2 log10(|x| / 32768) + log10(row sum) was read from."""
    a = 10.0 ** ((row_value - rowsum_log10) / 2.0) * 32768.0
    return int(np.clip(np.rint(np.log(max(a, 1.0) / 600.0) / np.log(1.02)), 0, PROBE_PERIOD - 1))


def probe_separation(n, N, S, taps, start=0):
    """Least |2 log10|x[i]| - 2 log10|x[i']|| over the probed (frame, tap) of probe_signal(n, start), i the sample the
    frame rule reads and i' every index a wrong kernel could read in its place: i +- 1..4, the unreflected index r = t S + j -
    N / 2 where r != i (the probe is defined for every integer, so this also covers an r outside the utterance), and the other
    reflection rule's index (-r - 1 at the left end, 2 n - 1 - r at the right)."""
    T = stft_ref.frame_count(n, N, S)
    if T == 0:
        return np.inf
    idx = stft_ref.frame_index(n, N, S)[:, taps]
    raw = np.arange(T, dtype=np.int64)[:, None] * S + np.asarray(taps, np.int64)[None, :] - N // 2

    def lv(i):
        return 2.0 * np.log10(np.abs(probe_value(i + start).astype(np.float64)))

    here = lv(idx)
    least = np.inf
    for d in (1, 2, 3, 4):
        least = min(least, np.abs(lv(idx + d) - here).min(), np.abs(lv(idx - d) - here).min())
    refl = raw != idx
    if refl.any():
        least = min(least, np.abs(lv(raw) - here)[refl].min())
        other = np.where(raw < 0, -raw - 1, 2 * n - 1 - raw)
        least = min(least, np.abs(lv(other) - here)[refl].min())
    return float(least)


# ---- the float32 checker -----------------------------------------------------------------------------------------------

MUTATIONS = ("drop tap 0", "drop taps >= N & ~3", "reflect with -j - 1", "reflect with 2n - 1 - j", "read the sample one behind",
             "zero the last bin", "zero the last weighted bin")


def _fma32(a, b, c):
    """float32 fmaf through double: the product of two float32 is exact in double, the sum rounds once to double and once
    more to float32 -- a double rounding that can differ from fmaf by one float32 ulp on rare near-ties, far below every bar."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def checker_frame_index(n, N, S, mutation=None):
    T = stft_ref.frame_count(n, N, S)
    i = np.arange(T, dtype=np.int64)[:, None] * S + np.arange(N, dtype=np.int64)[None, :] - N // 2
    i = np.where(i < 0, -i - 1 if mutation == "reflect with -j - 1" else -i, i)
    i = np.where(i >= n, (2 * n - 1 if mutation == "reflect with 2n - 1 - j" else 2 * (n - 1)) - i, i)
    if mutation == "read the sample one behind":
        i = np.maximum(i - 1, 0)
    return np.clip(i, 0, n - 1)


def checker_logmel(pcm, window, S, M, sr, low, high, post=LOG10, mutation=None):
    """The pipeline of mfx_stft.hip restated in float32 numpy (rows [T][M], float32): x = float(pcm) 2^-15; re / im one
    tap-ascending fmaf chain each over the float32 basis of stft_ref.basis; P = fmaf(im, im, re re); the mel chain over each
    row's non-zero span, ascending; max(., 1e-10f); the log.  `mutation`: one of MUTATIONS, a deliberately wrong front end."""
    assert mutation is None or mutation in MUTATIONS
    pcm = np.asarray(pcm)
    window = np.asarray(window, np.float32)
    N, n = window.size, pcm.size
    T = stft_ref.frame_count(n, N, S)
    if T == 0:
        return np.zeros((0, M), np.float32)
    x = (pcm.astype(np.float32) * np.float32(1.0 / 32768.0))[checker_frame_index(n, N, S, mutation)]     # [T][N]
    b = stft_ref.basis(window).copy()
    if mutation == "drop tap 0":
        b[:, :, 0] = 0.0
    if mutation == "drop taps >= N & ~3":
        b[:, :, N & ~3:] = 0.0
    K1 = N // 2 + 1
    re, im = np.zeros((T, K1), np.float32), np.zeros((T, K1), np.float32)
    for j in range(N):
        if not b[:, :, j].any():
            continue                       # (fmaf(x, 0, acc) == acc)
        xj = x[:, j, None]
        re, im = _fma32(xj, b[0, None, :, j], re), _fma32(xj, b[1, None, :, j], im)
    P = _fma32(im, im, re * re)
    w, beg, ln = stft_ref.mel_table(M, N, sr, low, high)
    if mutation == "zero the last bin":
        P[:, K1 - 1] = 0.0
    if mutation == "zero the last weighted bin":
        P[:, int((beg + ln).max()) - 1] = 0.0
    mel = np.zeros((T, M), np.float32)
    for m in range(M):
        acc = np.zeros(T, np.float32)
        for k in range(beg[m], beg[m] + ln[m]):
            acc = _fma32(np.broadcast_to(w[m, k], (T,)), P[:, k], acc)
        mel[:, m] = acc
    v = np.maximum(mel, np.float32(1e-10))
    if post == LN:
        return np.log(v.astype(np.float64)).astype(np.float32)
    L = np.where(v == np.float32(1e-10), FLOOR_L10, np.log10(v.astype(np.float64)).astype(np.float32))
    if post == WHISPER:
        L = (np.maximum(L, L.max() - np.float32(8.0)) + np.float32(4.0)) * np.float32(0.25)
    return L


# ---- conditioning ----------------------------------------------------------------------------------------------------
# edge_signals.py, "conditioning", for this front end: a float32 DFT returns the exact transform of samples and window moved
# by about u log2 N of their size (u = 2^-24).  sensitivity() applies two such perturbations to the float64 oracle (with an
# unrounded basis, so that the perturbed window is not rounded back) and records how far each log10 mel value moves; entries
# that move by more than COND_TOL / ln 10 -- edge_signals' COND_TOL is in natural-log units -- are rounding noise of any
# float32 front end: they must be finite and take part in every bit comparison, and are not held to the float64 value.
COND_TOL10 = ES.COND_TOL / np.log(10.0)


def _oracle_unrounded(x, w, S, M, sr, low, high):
    f = stft_ref.frames(x, w.size, S) * w[None, :]
    P = np.abs(np.fft.rfft(f, axis=1)) ** 2
    mel = P @ stft_ref.mel_table(M, w.size, sr, low, high)[0].astype(np.float64).T
    return np.log10(np.maximum(mel, stft_ref.FLOOR))


def sensitivity(pcm, window, S, M, sr, low, high):
    x, w = np.asarray(pcm, np.float64), np.asarray(window, np.float32).astype(np.float64)
    eps = 2.0 ** -24 * np.log2(w.size)
    L = _oracle_unrounded(x, w, S, M, sr, low, high)
    sens = np.zeros_like(L)
    for k in range(2):
        rng = np.random.default_rng(0xC09D + k)
        xp = x * (1.0 + eps * rng.uniform(-1.0, 1.0, x.size))
        wp = w * (1.0 + eps * rng.uniform(-1.0, 1.0, w.size))
        sens = np.maximum(sens, np.abs(_oracle_unrounded(xp, wp, S, M, sr, low, high) - L))
    return sens


# ---- bars ------------------------------------------------------------------------------------------------------------
# Absolute, in log10 units, one per window class: 4 x the checker's own worst distance to stft_ref.logmel over all SHAPES and
# all edge signals on held (unmasked), off-floor entries, rounded up to one significant digit.  4 x is the margin of
# edge_signals.py, for the same three extra roundings between checker and kernel: the matrix instruction's inner order, the
# device's log, FMA contraction.  Measured by tests/test_stft_edge_host.py, which asserts every derivation below:
#   window   checker's worst |d L|   at                                  4 x         bar
#   hann     1.411e-4                414/138/40 (1.37e-4 at 416/104/40)  5.64e-4     6e-4
#   rect     9.25e-6                 512/512/128                         3.70e-5     4e-5
#   ramp     6.02e-6                 512/512/128                         2.41e-5     3e-5
#   ends     1.23e-6                 512/512/128                         4.92e-6     5e-6
#   onehot   5.17e-7                 396/336/8 (probe utterances)        2.07e-6     3e-6 + 2 ulp of the largest |L|
# (The checker rounds its log to float32 as the kernel does: half an ulp of |L| in [4, 8) is 2.4e-7 of the one-hot figure.)
# The one-hot bar adds two float32 ulp of the largest |L| of the probe rows (6.17, below ONEHOT_LMAX) for the device's log10f;
# it stays below 1 / 100 of PROBE_SEPARATION, asserted here.  Under LN the bars are the same figures times ln 10; after
# WHISPER's map, a quarter.
CHECKER_WORST = {"hann": 1.411e-4, "rect": 9.25e-6, "ramp": 6.02e-6, "ends": 1.23e-6, "onehot": 5.17e-7}
BARS = {"hann": 6e-4, "rect": 4e-5, "ramp": 3e-5, "ends": 5e-6}
ONEHOT_LMAX = 8.0
ONEHOT_BAR = 3e-6 + 2 * 2.0 ** -21      # (an ulp of a float32 in [4, 8) is 2^-21)
assert ONEHOT_BAR <= PROBE_SEPARATION / 100.0
LN_FLOOR_ULPS = 2


def round_up_one_digit(v):
    digit = 10.0 ** np.floor(np.log10(v))
    return float(np.ceil(v / digit * (1 - 1e-12)) * digit)


def errors(got, want, ok=None):
    """(max |got - want| on held off-floor entries, count of floor entries that are not exactly -10.0f), LOG10 rows."""
    got, want = np.asarray(got), np.asarray(want, np.float64)
    assert got.shape == want.shape, "shape %s vs %s" % (got.shape, want.shape)
    ok = np.ones(want.shape, bool) if ok is None else np.asarray(ok, bool)
    floor = want == FLOOR_WANT
    d = np.abs(got.astype(np.float64) - want)
    held = ok & ~floor
    return (float(d[held].max()) if held.any() else 0.0), int((got[floor] != FLOOR_L10).sum())


def assert_rows(got, want, bar, what="", ok=None):
    """Every entry finite; held off-floor entries within `bar`; entries on the reference's floor exactly -10.0f."""
    assert np.isfinite(np.asarray(got)).all(), "%s: non-finite rows" % what
    e, off_floor = errors(got, want, ok)
    assert off_floor == 0, "%s: %d entries on the 1e-10 floor are not -10.0f" % (what, off_floor)
    assert e <= bar, "%s: max |d L| = %.3g > %.3g" % (what, e, bar)
    return e


# ---- references, computed once and shared --------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def shape_reference(shape, window_name):
    """Per edge signal of (shape, window): dict(pcm, want -- stft_ref.logmel under LOG10 --, ok -- the held entries).
    Computed once per process, read-only."""
    N, S, M, sr, low, high = shape
    w = windows(N)[window_name]
    out = {}
    for name, pcm in edge_utterances(shape).items():
        want = stft_ref.logmel(pcm, w, S, M, sr, low, high, LOG10)
        ok = sensitivity(pcm, w, S, M, sr, low, high) <= COND_TOL10
        for a in (pcm, want, ok):
            a.setflags(write=False)
        out[name] = dict(pcm=pcm, want=want, ok=ok)
    return out


def identical_rows(name, n, N, S):
    """(first, last + 1, stride) of the frames of an identical-frame signal that read no reflected sample: from ceil(N / 2S)
    on, up to the last frame whose right half ends inside the utterance."""
    first = -(-(N // 2) // S)
    last = min((n - N // 2) // S, stft_ref.frame_count(n, N, S) - 1)      # (t S + N / 2 - 1 <= n - 1; N is even)
    return first, last + 1, ES.identical_stride(name, S)
