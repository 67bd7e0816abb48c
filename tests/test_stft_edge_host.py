"""tests/stft_edge.py on the CPU: the float32 checker against the float64 oracle on every shape, window and signal -- the proof
that the bars of tests/test_stft_edge_gpu.py and tests/test_sess_stft_gpu.py are what stft_edge.py says they are --, the
conditions the GPU tests rest on (which entries are held, how far apart the probe's samples lie), deliberately wrong front
ends that the bars must refuse, the record of those that pass under Hann at the project bar, and the host-built basis for the
new windows.  No GPU.  Run with -s for the figures."""
import ctypes as C
import functools

import numpy as np
import pytest

import edge_signals as ES
import stft_edge as SE
import stft_ref
from conftest import assert_close, synth_utterance

IDS = [SE.shape_id(s) for s in SE.SHAPES]
# signals that hold no structure a window can null: none of their entries may be masked, under any window
NEVER_MASKED = ("zero", "lsb1", "lsb3", "impulses", "one_impulse", "burst")
# clipped and uniform noise: a band of a single bin now and then holds a bin whose taps nearly cancel, three to four decades
# below the row's largest value (at most 8 of a signal's 1720 entries over all shapes and windows): held to two digits
NOISE = ("clipped", "uniform")
# rect, ramp, ends hold at least 80 % of every signal's entries but where the window spans whole periods of a signal, whose
# leakage is then exactly nothing: tone_grid's period is 23 at S = 138 (N = 414 = 18 x 23) and 17 at S = 170 (N = 510 =
# 30 x 17); the chirp at 512 / 512 with 128 bands of one bin each.  Those are held to two thirds.
WHOLE_PERIODS = {((414, 138), "rect", "tone_grid"), ((510, 170), "rect", "tone_grid"), ((512, 512), "rect", "chirp")}


def block_rows(pkg, shape):
    r = C.c_int32(0)
    assert pkg.load_library().mfx_host_stft_lds_bytes(shape[0], shape[1], shape[2], C.byref(r)) > 0
    return r.value


@functools.lru_cache(maxsize=None)
def measured(shape, window):
    """(the checker's worst |d L| on held off-floor entries, name -> held share) of one shape and window."""
    N, S, M, sr, low, high = shape
    w = SE.windows(N)[window]
    worst, shares = 0.0, {}
    for name, r in SE.shape_reference(shape, window).items():
        got = SE.checker_logmel(r["pcm"], w, S, M, sr, low, high)
        assert got.dtype == np.float32 and np.isfinite(got).all()
        e, off_floor = SE.errors(got, r["want"], r["ok"])
        assert off_floor == 0, "%s %s %s: the checker leaves the floor" % (SE.shape_id(shape), window, name)
        worst = max(worst, e)
        shares[name] = float(r["ok"].mean())
    return worst, shares


@functools.lru_cache(maxsize=None)
def measured_onehot(shape, R):
    """(the checker's worst |d L| over the probe utterances and taps, the largest |L|, the least separation)."""
    N, S, M, sr, low, high = shape
    worst, lmax, sep = 0.0, 0.0, np.inf
    for n in SE.probe_lengths(N, S, R):
        x = SE.probe_signal(n)
        sep = min(sep, SE.probe_separation(n, N, S, SE.probe_taps(N)))
        for j in SE.probe_taps(N):
            w = SE.onehot(N, j)
            want = stft_ref.logmel(x, w, S, M, sr, low, high, SE.LOG10)
            e, off_floor = SE.errors(SE.checker_logmel(x, w, S, M, sr, low, high), want)
            assert off_floor == 0
            worst, lmax = max(worst, e), max(lmax, float(np.abs(want[want != SE.FLOOR_WANT]).max(initial=0.0)))
    return worst, lmax, sep


# ---- windows, signals ----------------------------------------------------------------------------------------------------

def test_windows(pkg):
    for N in (34, 400, 416, 512):
        w = SE.windows(N)
        assert list(w) == list(SE.WINDOWS) and all(v.dtype == np.float32 and v.shape == (N,) for v in w.values())
        assert np.array_equal(w["hann"], pkg.periodic_hann(N)) and w["hann"][0] == 0.0
        assert (w["rect"] == 1.0).all() and w["ramp"][0] == np.float32(1.0 / N) and w["ramp"][-1] == 1.0
        assert (np.diff(w["ramp"]) > 0).all()
        assert np.nonzero(w["ends"])[0].tolist() == [0, 1, 2, 3, N - 4, N - 3, N - 2, N - 1]
        for j in (0, N - 1):
            assert np.nonzero(SE.onehot(N, j))[0].tolist() == [j] and SE.onehot(N, j)[j] == 1.0
    # what Hann gives the outer matrix steps: at most 5.5e-4 on taps 1..3 and N-3..N-1 of the default shape
    h = SE.windows(400)["hann"]
    assert 6e-5 < h[1] < 6.3e-5 and h[3] < 5.6e-4 and h[397] < 5.6e-4 and h[399] == h[1]


def test_signals_and_lengths():
    for shape in SE.SHAPES:
        N, S = shape[:2]
        u = SE.edge_utterances(shape)
        assert list(u) == list(ES.MONO)
        for i, (name, x) in enumerate(u.items()):
            n = SE.utterance_length(N, S, i)
            assert x.size == n >= 800 and 0 <= n - max(N + 39 * S, 800) < S
            assert x.tobytes() == ES.signals(n, shape[3], 1, 0, shift=S)[name].tobytes()      # edge_signals' own, unchanged
            assert stft_ref.frame_count(n, N, S) >= ES.FRAMES
    x = SE.probe_signal(400)
    assert x.dtype == np.int16 and x[0] == 600 and abs(int(x[192])) == 26877 and abs(int(x[193])) == 600
    assert (x < 0).any() and (x > 0).any() and np.array_equal(x, SE.probe_value(np.arange(400)))
    assert SE.probe_decode(2 * np.log10(abs(int(x[77])) / 32768.0) - 1.25, -1.25) == 77


def test_block_rows_of_the_shapes(pkg):
    """Blocks of 64 and of 32 frames occur among the shapes.  A block of 16 frames occurs for NO shape the method accepts:
    the LDS of a block grows with N, S and M, and 32 frames fit at the top of all three (512 / 512 / 128), so no shape can be
    swapped in for it -- tests/test_stft_host.py walks the whole range and agrees."""
    assert sorted({block_rows(pkg, s) for s in SE.SHAPES}) == [32, 64]
    assert block_rows(pkg, (512, 512, 128)) == 32 and block_rows(pkg, (512, 1, 128)) == 64
    assert block_rows(pkg, SE.SHAPES[6]) == 32 and block_rows(pkg, SE.SHAPES[5]) == 32


# ---- the checker against the oracle: bars and conditions ---------------------------------------------------------------------

@pytest.mark.parametrize("window", SE.WINDOWS)
@pytest.mark.parametrize("shape", SE.SHAPES, ids=IDS)
def test_checker_is_within_a_quarter_of_the_bar(shape, window):
    worst, shares = measured(shape, window)
    least = min(shares, key=shares.get)
    print("\n%-16s %-5s checker vs float64: |d L| %.3g = %.2f of the bar; least held share %.2f (%s)" % (
        SE.shape_id(shape), window, worst, worst / SE.BARS[window], shares[least], least))
    assert worst <= SE.BARS[window] / 4
    for name in NEVER_MASKED:
        assert shares[name] == 1.0, "%s %s: entries of %s are masked" % (SE.shape_id(shape), window, name)
    for name in NOISE:
        assert shares[name] >= 0.995, "%s %s: %s held %.4f" % (SE.shape_id(shape), window, name, shares[name])
    if window == "hann":
        print("    held under Hann: " + ", ".join("%s %.2f" % (k, v) for k, v in shares.items() if v < 1.0))
        assert min(shares.values()) >= 0.1          # (tones, chirp and square are mostly masked; something of each is held)
    else:
        for name, v in shares.items():
            low = 2.0 / 3.0 if (shape[:2], window, name) in WHOLE_PERIODS else 0.8
            assert v >= low, "%s %s: %s held %.2f" % (SE.shape_id(shape), window, name, v)


def test_bars_are_four_times_the_checkers_worst(pkg):
    """BARS[w] = 4 x the checker's worst |d L| over all shapes and signals, rounded up to one significant digit; the figures
    quoted in stft_edge.py are the measured ones (to their four digits)."""
    for window in SE.WINDOWS:
        worst = max(measured(s, window)[0] for s in SE.SHAPES)
        print("\n%-5s worst over the shapes %.4g, 4 x = %.4g, bar %.3g" % (window, worst, 4 * worst, SE.BARS[window]))
        assert SE.BARS[window] == pytest.approx(SE.round_up_one_digit(4 * worst), rel=1e-12)
        assert worst == pytest.approx(SE.CHECKER_WORST[window], rel=2e-3)
    figs = [measured_onehot(s, block_rows(pkg, s)) for s in SE.SHAPES]
    worst, lmax, sep = max(f[0] for f in figs), max(f[1] for f in figs), min(f[2] for f in figs)
    print("\none-hot probes: worst %.4g, largest |L| %.3g, least separation of the probed samples %.4f" % (worst, lmax, sep))
    assert worst == pytest.approx(SE.CHECKER_WORST["onehot"], rel=2e-3)
    assert 4.0 <= lmax <= SE.ONEHOT_LMAX
    assert SE.ONEHOT_BAR == pytest.approx(SE.round_up_one_digit(4 * worst) + 2 * 2.0 ** -21, rel=1e-12)
    assert worst <= SE.ONEHOT_BAR / 4
    assert sep >= SE.PROBE_SEPARATION and SE.ONEHOT_BAR <= SE.PROBE_SEPARATION / 100


def test_probe_separation_of_the_session_streams():
    """The streams of test_sess_stft_gpu.test_tap_probes_through_sessions: stream k starts at sample 31 k of the probe."""
    for N, S, M in [(400, 160, 80), (34, 5, 6)]:
        for k, n in enumerate(SE.probe_lengths(N, S, 16)):
            assert SE.probe_separation(n, N, S, [0, 1, N // 2, N - 1], start=31 * k) >= SE.PROBE_SEPARATION


# ---- mutants ---------------------------------------------------------------------------------------------------------------

MUTANT_SIGNALS = ("uniform", "impulses", "lsb3")


def refused(got, want, bar, ok=None):
    try:
        SE.assert_rows(got, want, bar, ok=ok)
    except AssertionError:
        return True
    return False


@functools.lru_cache(maxsize=None)
def mutant_table(R_of):
    """mutation -> (where a non-Hann window or a one-hot probe refuses it, the shapes on which it passes under Hann at
    conftest.assert_close's bar, whether its rows under Hann ARE the checker's)."""
    R_of = dict(R_of)
    table = {}
    for mu in SE.MUTATIONS:
        caught, blind, exact = [], [], True
        for shape in SE.SHAPES:
            N, S, M, sr, low, high = shape
            for window in ("rect", "ramp", "ends"):
                ref = SE.shape_reference(shape, window)
                w = SE.windows(N)[window]
                if any(refused(SE.checker_logmel(ref[n]["pcm"], w, S, M, sr, low, high, mutation=mu), ref[n]["want"], SE.BARS[window],
                               ref[n]["ok"]) for n in MUTANT_SIGNALS):
                    caught.append((SE.shape_id(shape), window))
            x = SE.probe_signal(SE.probe_lengths(N, S, R_of[shape])[4])
            for j in (0, N // 2, N - 1):
                w = SE.onehot(N, j)
                if refused(SE.checker_logmel(x, w, S, M, sr, low, high, mutation=mu), stft_ref.logmel(x, w, S, M, sr, low, high, SE.LOG10),
                           SE.ONEHOT_BAR):
                    caught.append((SE.shape_id(shape), "onehot %d" % j))
            # under Hann, at the project bar, on the kind of input tests/test_stft_gpu.py uses
            w = SE.windows(N)["hann"]
            passes = True
            for x in (synth_utterance(SE.utterance_length(N, S, 0), 11, sr=sr), SE.shape_reference(shape, "hann")["uniform"]["pcm"]):
                want = stft_ref.logmel(x, w, S, M, sr, low, high, SE.LOG10)
                got = SE.checker_logmel(x, w, S, M, sr, low, high, mutation=mu)
                exact = exact and np.array_equal(got.view(np.uint32), SE.checker_logmel(x, w, S, M, sr, low, high).view(np.uint32))
                try:
                    assert_close(got, want, mu)
                except AssertionError:
                    passes = False
            if passes:
                blind.append(SE.shape_id(shape))
        table[mu] = (caught, blind, exact)
    return table


def test_mutants(pkg):
    """Every wrong front end is refused by a non-Hann window or a one-hot probe.  Under Hann at the project bar (the suite
    before these tests) `drop tap 0` passes on EVERY shape, with the checker's very bits -- tap 0 meets an exact zero --, and
    `drop taps >= N & ~3` (the padded last matrix step) passes at N = 510, the one N % 4 == 2 shape that ran before.
    `zero the last bin` is seen by nothing: the Slaney table ends on high_freq <= sr / 2, so the Nyquist bin weighs exactly 0
    in every row of every shape; its observable form, `zero the last weighted bin`, is refused."""
    table = mutant_table(tuple((s, block_rows(pkg, s)) for s in SE.SHAPES))
    for mu, (caught, blind, exact) in table.items():
        print("\n%-28s refused at %2d (shape, window) pairs, e.g. %s; passes under Hann on %d shapes: %s%s" % (
            mu, len(caught), caught[:3], len(blind), blind, " (bit-identical)" if exact else ""))
    for shape in SE.SHAPES:
        N, S, M, sr, low, high = shape
        assert not stft_ref.mel_table(M, N, sr, low, high)[0][:, N // 2].any()
    for mu, (caught, blind, exact) in table.items():
        if mu == "zero the last bin":
            assert not caught and exact and len(blind) == len(SE.SHAPES)
        else:
            assert caught, "%s: no window refuses it" % mu
    assert table["drop tap 0"][2] and len(table["drop tap 0"][1]) == len(SE.SHAPES)
    mod2 = {SE.shape_id(s) for s in SE.SHAPES if s[0] % 4 == 2}
    padded = table["drop taps >= N & ~3"]
    assert {c[0] for c in padded[0]} == mod2                  # (on N % 4 == 0 shapes it is no mutation at all)
    assert set(padded[1]) >= {SE.shape_id(s) for s in SE.SHAPES if s[0] % 4 == 0}
    assert "510_170_40_16k" in padded[1]                      # the one N % 4 == 2 shape the suite ran before: Hann lets it pass
    for mu in ("reflect with -j - 1", "reflect with 2n - 1 - j", "read the sample one behind"):
        assert any(w.startswith("onehot") for _, w in table[mu][0]), mu
    # tap 0 is what only the new windows see: every shape refuses its loss under rect, ramp, ends and the tap-0 probe
    for shape in SE.SHAPES:
        seen = {w for s, w in table["drop tap 0"][0] if s == SE.shape_id(shape)}
        assert seen >= {"rect", "ramp", "ends", "onehot 0"}, (SE.shape_id(shape), seen)


# ---- the host-built basis ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N", [34, 414, 416])
def test_stft_basis_for_the_new_windows(pkg, N):
    wins = dict(SE.windows(N))
    wins.update({"onehot %d" % j: SE.onehot(N, j) for j in (0, N // 2, N - 1)})
    for name, w in wins.items():
        b = pkg.host_stft_basis(w)
        r = stft_ref.basis(w)
        assert b.shape == r.shape == (2, N // 2 + 1, N)
        ulp = np.abs(b.view(np.int32).astype(np.int64) - r.view(np.int32).astype(np.int64))
        assert ulp.max() <= 1, (N, name, ulp.max())
        assert not b[:, :, w == 0].any()                      # a zero tap is an exact zero column (+0 or -0)
