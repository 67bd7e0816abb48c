"""The edge signals of tests/edge_signals.py on the CPU: the float32 checker (liboracle.so) against the float64 reference on
every row of mfcc.KERNEL_TABLE -- the proof that the bars of tests/test_edge_signals_gpu.py are what edge_signals.py says they
are --, three deliberately wrong references that the bars must refuse, and the premises of the GPU test (reproducible
signals, identical frames).  Run with -s to see the checker's worst errors per row."""
import numpy as np
import pytest

import __graft_entry__ as G
import edge_signals as ES
from conftest import TOL_MAX

KERNEL_TABLE = G.load_package().mfcc.KERNEL_TABLE
IDS = [ES.row_id(what) for what, _, _ in KERNEL_TABLE]
_WORST = {}


def _window(pkg, shape):
    return pkg.reference_window(shape["W"])


def _checker(orc, shape, mono, window, nc, c0):
    """The checker's static rows (bug_compat off).  A transform longer than the window: the checker ties the two, so it is
    given a window of fft_size taps whose tail is zero (make_pair of test_parity_gpu.py) and loses the last few frames."""
    Wo = shape["fft_size"] or shape["W"]
    w_o = np.zeros(Wo, np.float32)
    w_o[:shape["W"]] = window
    cfg = orc.make_config(mono.size + 1000, window_size=Wo, shift=shape["S"], num_banks=shape["nb"], sample_rate=shape["sr"],
                          low_freq=shape["low"], high_freq=shape["high"], ceps_len=nc, want_c0=c0, lift_coef=shape["lift"],
                          norm=0, dyn=0)
    return orc.run_utterance(cfg, mono, w_o, bug_compat=False)


@pytest.mark.parametrize("row", range(len(KERNEL_TABLE)), ids=IDS)
def test_checker_is_within_a_quarter_of_the_bars(pkg, orc, row):
    what, kw, _ = KERNEL_TABLE[row]
    shape = ES.row_shape(kw)
    window = _window(pkg, shape)
    ref = ES.row_reference(kw, window)
    assert len(ref) == (19 if shape["channels"] == 2 else 16)
    worst = dict(logmel=0.0, emax=0.0, el2=0.0, left_out=0, entries=0)
    for name, r in ref.items():
        assert r["mel"].shape == (ES.FRAMES, shape["nb"])
        mel = _checker(orc, shape, r["mono"], window, 0, False)
        rows = _checker(orc, shape, r["mono"], window, shape["nc"], shape["c0"])
        n = mel.shape[0]
        assert ES.FRAMES - 5 <= n <= ES.FRAMES and rows.shape[0] == n     # (common prefix)
        ok = r["ok"][:n]
        tag = "%s, %s" % (what, name)
        e = ES.assert_logmel_close(mel, r["mel"][:n], tag, tol=ES.EDGE_TOL_LOGMEL / 4, ok=ok)
        good = ok.all(axis=1)
        emax, el2 = ES.assert_rows_close(rows[good], r["c"][:n][good], r["mel"][:n], tag, tol_max=TOL_MAX / 4,
                                         tol_l2=ES.EDGE_TOL_L2 / 4)
        worst = dict(logmel=max(worst["logmel"], e), emax=max(worst["emax"], emax), el2=max(worst["el2"], el2),
                     left_out=worst["left_out"] + int((~ok).sum()), entries=worst["entries"] + ok.size)
    _WORST[row] = worst
    print("\n%-68s checker vs float64: |d log E| %.3g  floored max %.3g  floored L2 %.3g  (ill-conditioned entries: %d of %d)" % (
        what[:68], worst["logmel"], worst["emax"], worst["el2"], worst["left_out"], worst["entries"]))


def test_zz_constants_are_the_measured_values_times_four():
    """EDGE_TOL_LOGMEL = 4 x the checker's worst |d log E|, rounded up to one significant digit; EDGE_TOL_L2 = max(TOL_L2,
    4 x its worst floored L2) (rounded up to three digits).  Needs every row above to have run."""
    if len(_WORST) != len(KERNEL_TABLE):
        pytest.skip("runs with the whole module")
    logmel = max(w["logmel"] for w in _WORST.values())
    el2 = max(w["el2"] for w in _WORST.values())
    emax = max(w["emax"] for w in _WORST.values())
    print("\nworst over the table: |d log E| %.4g  floored max %.4g (%.2f of TOL_MAX)  floored L2 %.4g" % (
        logmel, emax, emax / TOL_MAX, el2))
    digit = 10.0 ** np.floor(np.log10(4 * logmel))
    assert ES.EDGE_TOL_LOGMEL == pytest.approx(np.ceil(4 * logmel / digit) * digit, rel=1e-12)
    assert 4 * el2 <= ES.EDGE_TOL_L2 <= 4 * el2 * 1.005
    assert emax <= TOL_MAX / 4


# ---- the bars tell wrong front ends apart ----------------------------------------------------------------------------------

def _trunc_downmix(pcm):
    """(L + R) / 2 rounded towards zero instead of floored."""
    x = np.asarray(pcm, np.int32).reshape(-1, 2)
    return np.trunc((x[:, 0] + x[:, 1]) / 2.0).astype(np.int32)


def _one_sample_late(mono):
    return np.concatenate([mono[1:], mono[-1:]])


def _low_half_unsigned(mono):
    """A packed 32-bit load whose low int16 is widened without its sign."""
    x = np.asarray(mono, np.int32).copy()
    x[0::2] &= 0xFFFF
    return x


MUTANTS = [("downmix by truncating division", _trunc_downmix, "lr_lsb"),
           ("frames started one sample late", _one_sample_late, "impulses"),
           ("low int16 of each pair read unsigned", _low_half_unsigned, "min"),
           ("low int16 of each pair read unsigned", _low_half_unsigned, "square")]


@pytest.mark.parametrize("row", range(len(KERNEL_TABLE)), ids=IDS)
def test_mutants_of_the_reference_fail_the_bars(pkg, row):
    """Each mutant against the unmutated reference, on the signals named for it: both checks must refuse it.  A signal none of
    whose entries is well conditioned on the row (min where the window fills the transform) cannot show anything; every
    mutant keeps at least one signal that can.  The cepstra are asked where the signal has a row free of such entries."""
    what, kw, _ = KERNEL_TABLE[row]
    shape = ES.row_shape(kw)
    window = _window(pkg, shape)
    ref = ES.row_reference(kw, window)
    args = {k: v for k, v in shape.items() if k != "channels"}
    caught = {}
    for mutant, fn, name in MUTANTS:
        if name not in ref:
            continue                                         # (lr_lsb: stereo rows)
        caught.setdefault(mutant, 0)
        r = ref[name]
        good = r["ok"].all(axis=1)
        if not r["ok"].any():
            continue
        c, mel = ES.reference(fn(r["pcm"] if fn is _trunc_downmix else r["mono"]), window, **args)
        tag = "%s, %s on %s" % (what, mutant, name)
        with pytest.raises(AssertionError):
            ES.assert_logmel_close(mel, r["mel"], tag, ok=r["ok"])
        if good.any():                                       # (rows without an ill-conditioned entry)
            with pytest.raises(AssertionError):
                ES.assert_rows_close(c[good], r["c"][good], r["mel"], tag)
        caught[mutant] += 1
    assert caught and all(caught.values()), caught


# ---- premises of the GPU test --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("channels", [1, 2])
def test_signals_are_reproducible(channels):
    a = ES.signals(6643, 16000.0, channels, seed=3, shift=160)
    b = ES.signals(6643, 16000.0, channels, seed=3, shift=160)
    c = ES.signals(6643, 16000.0, channels, seed=4, shift=160)
    assert list(a) == list(b) == list(ES.MONO) + (list(ES.STEREO) if channels == 2 else [])
    for name in a:
        assert a[name].tobytes() == b[name].tobytes(), name
    assert a["lsb1"].tobytes() != c["lsb1"].tobytes()
    assert set(np.unique(a["lsb1"])) == {-1, 0, 1} and set(np.unique(a["lsb3"])) == set(range(-3, 4))
    assert a["min"].min() == a["min"].max() == -32768 and a["max"].min() == 32767
    assert a["clipped"].min() == -32768 and a["clipped"].max() == 32767
    imp = a["impulses"].reshape(-1, channels)[:, 0]
    assert list(np.nonzero(imp)[0][:4]) == [0, 500, 997, 1994] and imp[500] == -32768 and imp[997] == 32767
    assert np.count_nonzero(a["one_impulse"]) == channels
    if channels == 2:
        s = a["lr_lsb"].astype(np.int32).reshape(-1, 2).sum(1)
        assert ((s < 0) & (s % 2 != 0)).sum() > 0.3 * (s < 0).sum()        # the sums where flooring and truncating differ
        assert not a["l_only"][1::2].any() and a["l_only"][0::2].any()
        assert a["lr_extremes"][:8].tolist() == [-32768, -32768, 32767, 32767, 32767, -32768, -32768, 32767]


@pytest.mark.parametrize("row", range(len(KERNEL_TABLE)), ids=IDS)
def test_frames_of_the_stationary_signals_are_identical(pkg, row):
    """zero, min, max, one, nyquist, tone_grid (period | S) and lr_extremes (4 | S): every frame holds the samples of frame 0,
    so every row of the float64 reference equals row 0.  nyquist at an odd shift: 32767, -32768, ... read from an odd sample
    is -32768, 32767, ..., the negation of frame 0 moved by one count -- its magnitudes differ from frame 0's by 3e-5 --, so
    there the frames are alike in two classes, the even and the odd ones (edge_signals.identical_stride)."""
    what, kw, _ = KERNEL_TABLE[row]
    shape = ES.row_shape(kw)
    W, S = shape["W"], shape["S"]
    ref = ES.row_reference(kw, _window(pkg, shape))
    names = ES.identical_frame_signals(S, shape["sr"], shape["channels"])
    assert names[:5] == ["zero", "min", "max", "one", "nyquist"] and "tone_grid" in names    # every shift of the table allows it
    for name in names:
        r = ref[name]
        x = r["mono"].astype(np.int64)
        frames = x[np.arange(ES.FRAMES)[:, None] * S + np.arange(W)[None, :]]
        step = ES.identical_stride(name, S)
        assert step == (2 if name == "nyquist" and S % 2 else 1)
        ok = r["ok"].all(axis=0)
        for k in range(step):
            f, mel, c = frames[k::step], r["mel"][k::step], r["c"][k::step]
            assert ((f == f[:1]).all(axis=1) | (f == -f[:1]).all(axis=1)).all(), "%s, %s" % (what, name)
            assert np.abs(mel[:, ok] - mel[:1, ok]).max(initial=0.0) <= 1e-9, "%s, %s" % (what, name)
            assert not ok.all() or np.abs(c - c[:1]).max() <= 1e-6, "%s, %s" % (what, name)
