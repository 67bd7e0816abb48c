"""The Kaldi front end (k_kaldi_front) on the MI355X under windows other than Povey -- Kaldi's Hamming, the rectangular window
and an asymmetric ramp whose taps are all distinct and non-zero (tests/kaldi_ref.py) -- at the shapes where the kernel's layout
or its guards change (kaldi_windows_cases.MATRIX: W = 128, 129, 256, 257; log-mel rows that outgrow the staged span; S = 1),
against the float64 oracle at the unchanged project bar, and the method's bit contract and its session path away from W = 400.

Under Povey taps 0 and W - 1 are exactly zero, so the frame-start rule e[0] = fmaf(-c, d[0], d[0]), the two end taps and the
i1 < W guard of an odd W cannot move a row; tests/test_kaldi_windows_host.py shows on the CPU that each of these, seeded as a
fault, moves the rows of every shape here by at least 10 x the bar under the windows below (and a mirrored window by more than a
tenth of the scale under the ramp), and that a float32 restatement stays 39 x under the bar (2.6e-6 of scale, 7.9e-7 relative
L2 at worst).  Every case runs two utterances, of 45 and 3 frames.  The sessions are the only place where a frame-start fault
of the session path -- the sample in front of the frame is at hand there -- could show.

The kernel's own figures on the MI355X: over the 27 shape / window pairs at most 1.5e-6 of scale (400 / 160 / 80 / 0 under
Hamming) and 6.3e-7 relative L2 (256 / 64 / 40 / 13 under Hamming); the energy-domain edge signals at most 2.6e-6 of the frame's
largest energy (the tone under rect) against their bar of 1e-4; no signal / window pair is left not held.  DESIGN.md section 5,
"Kaldi front end", has the table per shape and window.

Agreement with a Kaldi or torchaudio binary remains unmeasured."""
import numpy as np
import pytest

import kaldi_ref as KR
import kaldi_windows_cases as KC
import onorm_drive as OD
from conftest import synth_utterance
from kaldi_drive import Shape, check, make
from stft_drive import layout, run_batch, same_bits
from kaldi_windows_cases import ENERGY_BAR, shape_utterances
from test_kaldi_gpu import OPTIONS
from test_kaldi_sessions_gpu import CUTS

pytestmark = pytest.mark.gpu

IDS = [s.id() for s in KC.MATRIX]


def floor_of(x):
    """logf of the floor as the device has it: one value, -15.9424."""
    assert abs(float(x) + 15.9424) < 1e-4
    return x


# ---- 1. window matrix ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("sh", KC.MATRIX, ids=IDS)
def test_window_matrix(pkg, sh):
    worst = (0.0, 0.0)
    for window in KC.NEW_WINDOWS:
        s = KC.under(sh, window)
        utts = shape_utterances(s)
        m = make(pkg, s)
        assert m.dominant_kernel_name() == "k_kaldi_front" and m.fft_size() == KR.fft_size(s.W)
        got = run_batch(m, utts)
        m.close()
        assert [g.shape for g in got] == [(45, s.cols), (4 if s.S == 1 else 3, s.cols)]      # (S = 1: the remainder is a hop)
        w = (0.0, 0.0)
        for i, u in enumerate(utts):
            e = check(got[i], s.oracle(u), "%s %s utt %d" % (s.id(), window, i))
            w = (max(w[0], e[0]), max(w[1], e[1]))
        print("%s under %s: worst max err / scale %.3g, rel L2 %.3g" % ((s.id(), window) + w))
        worst = (max(worst[0], w[0]), max(worst[1], w[1]))
    print("%s: worst max err / scale %.3g, rel L2 %.3g over %s" % ((sh.id(),) + worst + (", ".join(KC.NEW_WINDOWS),)))


@pytest.mark.parametrize("window", KC.NEW_WINDOWS)
def test_empty_bands_sit_on_the_floor(pkg, window):
    """128 / 4 / 64 / 20 feeds seven empty bands to its DCT; its fbank twin shows them: the floor value, in every frame."""
    s = Shape(128, 4, 64, 0, window=window)
    empty = np.nonzero(KR.mel_table(64, 128, s.sr, s.low, s.high)[2] == 0)[0]
    assert empty.size == 7
    utts = shape_utterances(s)
    m = make(pkg, s)
    got = run_batch(m, utts)
    m.close()
    floor = floor_of(got[0][0, empty[0]])
    for i, u in enumerate(utts):
        check(got[i], s.oracle(u), "128-4-64-0 %s utt %d" % (window, i))
        assert (got[i][:, empty] == floor).all()
        assert (np.delete(got[i], empty, axis=1) > floor).all()


# ---- 2. options under a window without a taper --------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(OPTIONS))
def test_options_under_the_rectangular_window(pkg, name):
    base = KC.under(KC.MATRIX[0], "rect")
    sh = base.options(**OPTIONS[name])
    utts = shape_utterances(sh)
    utts[0] = (utts[0].astype(np.int32) // 2 + 900).astype(np.int16)      # (a DC offset for the DC removal to take out)
    m = make(pkg, base)
    default = run_batch(m, utts)
    m.kaldi_set_options(sh.preemph, sh.remove_dc, sh.use_power)
    got = run_batch(m, utts)
    m.kaldi_set_options()
    back = run_batch(m, utts)
    m.close()
    for i, u in enumerate(utts):
        assert np.abs(got[i].astype(np.float64) - default[i]).max() > 1e-2, name
        assert same_bits(back[i], default[i]), "%s: the defaults' bits did not come back (utt %d)" % (name, i)
        check(got[i], sh.oracle(u), "rect, %s utt %d" % (name, i))
        check(default[i], base.oracle(u), "rect, defaults utt %d" % i)


# ---- 3. the window replaced on a live handle ----------------------------------------------------------------------------------

def test_window_replaced_on_a_live_handle(pkg):
    povey, ramp = KC.MATRIX[2], KC.under(KC.MATRIX[2], "ramp")          # 257 / 100 / 40 / 0
    utts = shape_utterances(povey)
    m = make(pkg, povey)
    first = run_batch(m, utts)
    m.set_window(ramp.taps())
    second = run_batch(m, utts)
    m.set_window(pkg.povey_window(povey.W))
    third = run_batch(m, utts)
    m.close()
    for i, u in enumerate(utts):
        assert same_bits(third[i], first[i]), "Povey again: not the first run's bits (utt %d)" % i
        assert not same_bits(second[i], first[i]) and np.abs(second[i].astype(np.float64) - first[i]).max() > 1e-2
        check(first[i], povey.oracle(u), "Povey utt %d" % i)
        check(second[i], ramp.oracle(u), "ramp on the live handle utt %d" % i)


# ---- 4. the bit contract away from W = 400 ------------------------------------------------------------------------------------

BITS_SHAPES = (KC.under(KC.MATRIX[2], "ramp"), KC.under(KC.MATRIX[5], "ramp"))      # 257 / 100 / 40 / 0, 128 / 32 / 23 / 0
BITS_FRAMES = [0, 0, 1, 2, 15, 16, 17, 33]


def bits_lengths(sh):
    """No sample, one short of a frame, then 1, 2, 15, 16, 17 and 33 frames and a remainder; the one-frame utterance has an odd
    length, so that in a sub-batch that starts with it every later utterance starts at an odd sample."""
    W, S = sh.W, sh.S
    lens = [0, W - 1, W + (1 - W % 2)] + [W + (T - 1) * S + r for T, r in ((2, 0), (15, 3), (16, S - 1), (17, 1), (33, S // 2))]
    assert [sh.frames(n) for n in lens] == BITS_FRAMES and lens[2] % 2 == 1
    return lens


@pytest.mark.parametrize("sh", BITS_SHAPES, ids=[s.id() for s in BITS_SHAPES])
def test_bits_do_not_depend_on_batch_offset_run_entry_or_placement(pkg, sh):
    import torch
    utts = [synth_utterance(n, 600 + i, sr=sh.sr) for i, n in enumerate(bits_lengths(sh))]
    m = make(pkg, sh)
    got = run_batch(m, utts)
    assert [g.shape for g in got] == [(T, sh.cols) for T in BITS_FRAMES]
    for i, u in enumerate(utts):
        check(got[i], sh.oracle(u), "%s utt %d (%d frames)" % (sh.id(), i, BITS_FRAMES[i]))
        alone = run_batch(m, [u])[0]
        assert same_bits(alone, got[i]), "utt %d alone differs from its rows in the batch" % i
    sub = run_batch(m, utts[2:])                     # an odd length first: 3 .. 7 start at odd samples behind it
    shifted = run_batch(m, utts[2:], first=1)        # ... and the whole sub-batch one sample on
    for i in range(2, len(utts)):
        assert same_bits(sub[i - 2], got[i]), "utt %d in a sub-batch" % i
        assert same_bits(shifted[i - 2], got[i]), "utt %d at another offset" % i
    again = run_batch(m, utts)
    for i in range(len(utts)):
        assert same_bits(again[i], got[i]), "second run differs, utt %d" % i
    # the device entry, the output at an even and at an odd word of its allocation, NaN guards around it
    offs, lens, pcm_h = layout(utts)
    rows, total = m.batch_plan(offs, lens)
    dev = torch.device("cuda", 0)
    pcm = torch.from_numpy(pcm_h).to(dev)
    for lead in (32, 33):
        big = torch.full((lead + total * sh.cols + 64,), float("nan"), dtype=torch.float32, device=dev)
        torch.cuda.synchronize()
        m.batch_run_device(pcm.data_ptr(), pcm_h.size, big.data_ptr() + 4 * lead)
        m.synchronize()
        b = big.cpu().numpy()
        assert np.isnan(b[:lead]).all() and np.isnan(b[lead + total * sh.cols:]).all(), "guard words written (lead %d)" % lead
        out = b[lead:lead + total * sh.cols].reshape(total, sh.cols)
        for i in range(len(utts)):
            assert same_bits(out[rows[i]:rows[i] + got[i].shape[0]], got[i]), (lead, i)
    m.close()


# ---- 5. edge signals under rect and ramp --------------------------------------------------------------------------------------

@pytest.mark.parametrize("window", KC.EDGE_WINDOWS)
def test_edge_signals(pkg, window):
    """Each signal in the domain kaldi_windows_cases.edge_plan assigns it from the float32 restatement's room (printed by the host
    module): the floor value in every element, the project bar in the log domain, or ENERGY_BAR of the frame's largest energy."""
    plan = KC.edge_plan()
    cases = KC.edge_cases()
    sh = KC.under(KC.EDGE_SHAPE, window)
    got = {}
    for dc in (True, False):                         # one batch per setting of the DC removal
        names = [k for k, (_, d) in cases.items() if d == dc]
        m = make(pkg, sh.options(remove_dc=dc))
        got.update(zip(names, run_batch(m, [cases[k][0] for k in names])))
        m.close()
    floor = floor_of(got["silence"][0, 0])
    not_held, worst = [], 0.0
    for name, (pcm, dc) in cases.items():
        s = sh.options(remove_dc=dc)
        how, fig = plan[(name, window)]
        g = got[name]
        assert g.shape == (20, s.M) and np.isfinite(g).all()
        if how == "floor":
            assert (g == floor).all(), name
        elif how == "log":
            check(g, s.oracle(pcm), "%s under %s" % (name, window))
        elif how == "energy":
            err = KC.energy_err(g, s.oracle(pcm, energies=True))
            print("%s under %s: worst energy err / frame maximum = %.3g (bar %.3g, float32 restatement %.3g)" % (name, window, err, ENERGY_BAR, fig))
            assert err <= ENERGY_BAR, (name, window, err)
            worst = max(worst, err)
        else:
            not_held.append((name, fig))
    assert got["impulse"].max() > 10.0 and (got["impulse"][:7] == floor).all()      # (the impulse is in frame 7 at the earliest)
    assert not same_bits(got["constant, DC kept"], got["constant"])
    print("edge signals under %s: worst energy err / frame maximum %.3g; not held: %s" % (window, worst, not_held or "none"))


# ---- 6. sessions --------------------------------------------------------------------------------------------------------------

SESSION_CONFIGS = {
    "fbank40_w257_ramp": (KC.under(KC.MATRIX[2], "ramp"), dict()),
    "mfcc13_d_dd_w129_hamming_8k": (KC.under(KC.MATRIX[4], "hamming"), dict(dyn=2, l1=2, l2=2)),
}
SESSION_FRAMES = [0, 1, 7, 18, 33]


def session_streams(sh):
    W, S = sh.W, sh.S
    lens = [W - 1, W, W + 6 * S + S // 2 + 1, W + 17 * S + S - 1, W + 32 * S + 1]
    assert [sh.frames(n) for n in lens] == SESSION_FRAMES
    return [synth_utterance(n, 520 + i, sr=sh.sr) for i, n in enumerate(lens)]


@pytest.fixture(scope="module")
def session_twins(pkg):
    out = {}
    for name, (sh, kw) in SESSION_CONFIGS.items():
        m = make(pkg, sh, **kw)
        rows = run_batch(m, session_streams(sh))
        m.close()
        assert [r.shape[0] for r in rows] == SESSION_FRAMES
        for r in rows:
            r.setflags(write=False)
        out[name] = rows
    return out


@pytest.mark.parametrize("cut", sorted(CUTS))
@pytest.mark.parametrize("name", sorted(SESSION_CONFIGS))
def test_session_rows_are_the_batch_twins_bits(pkg, session_twins, name, cut):
    sh, kw = SESSION_CONFIGS[name]
    streams = session_streams(sh)
    want = session_twins[name]
    for u, x in enumerate(streams):                  # (the twin is the kernel's own output: its statics against the oracle)
        check(want[u][:, :sh.cols], sh.oracle(x), "%s stream %d" % (name, u))
    utts = [u.reshape(-1, 1) for u in streams]
    m = make(pkg, sh, **kw)
    m.sessions_create(3, max(u.size for u in streams))
    for odd in (False, True):
        got = OD.drive(m, utts, 3, CUTS[cut], seed=7 + odd, odd_offsets=odd)
        for u, w in enumerate(want):
            assert same_bits(got[u], w), "%s, %s, odd offsets %d: stream %d differs from its batch rows" % (name, cut, odd, u)
    got = OD.drive(m, utts, 3, CUTS[cut], seed=9, host=True)
    for u, w in enumerate(want):
        assert same_bits(got[u], w), (name, cut, "host entry", u)
    m.close()
    print("%s, %s: %d rows per pass, the batch twin's bits" % (name, cut, sum(w.shape[0] for w in want)))
