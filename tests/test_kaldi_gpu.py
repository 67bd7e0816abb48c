"""The Kaldi front end (MFX_METHOD_KALDI: k_kaldi_front) on the MI355X, under the Povey window, against the float64 oracle of
tests/kaldi_ref.py at the project bar (conftest.assert_close: 1e-4 of scale, 1e-5 rel-L2), the bit contract of the method at W =
400 -- rows do not depend on the batch, the offset, the run, the entry or the placement --, and its composition with the stages
behind it, each against the restatement the project already has for that stage.  Shapes are W / S / M / C.

Every test here runs under the Povey window, whose taps 0 and W - 1 are exactly zero: the frame-start rule, the end taps and the
i1 < W guard of an odd W cannot move a row of this module.  Windows other than Povey, the shapes where the kernel's layout or
its guards change, and the bit contract and the sessions away from W = 400 are held in tests/test_kaldi_windows_gpu.py (its
inputs' power is shown on the CPU in tests/test_kaldi_windows_host.py); the other batch attachments and the session transform
and rates on a Kaldi handle in tests/test_kaldi_compose_gpu.py.

Room under the bar.  A float32 restatement of the pipeline on the CPU (float32 mean, pre-emphasis and window product, torch's
float32 rfft, float32 tables, mel product and log) against the float64 oracle, on the utterances used here:
  fbank shapes   on synth_utterance at most 2.1e-5 of scale and 3.1e-7 relative L2 (the worst: 512 / 512 / 128 / 0; 400 / 160 /
                 80 / 0 stays at 8.1e-6, 100 / 50 / 10 / 0 at 1.2e-7); a0001 at 400 / 160 / 80 / 0: 2.7e-5 and 5.4e-7 (its quiet
                 frames: a log energy moves by the energy's RELATIVE error),
  MFCC shapes    on synth_utterance at most 6.0e-7 of scale and 4.9e-7 relative L2,
  the option matrix at most 1.3e-6 of scale and 9.5e-8 relative L2,
  the four energy-domain edge signals at most 2.0e-7 of the frame's largest energy (in the log domain they miss: up to 5.6e-4
  of scale)
-- the bars leave about 3.7x (a0001) and 5x (synth_utterance) of room on the fbank shapes, more than 20x elsewhere.  Every
test prints its worst figure.  The kernel's own on the MI355X: a0001 at 400 / 160 / 80 / 0 4.1e-5 of scale and 6.1e-7 relative
L2, 512 / 512 / 128 / 0 1.5e-5, the MFCC shapes at most 4.7e-7 and 5.6e-7, the energy-domain edge signals at most 1.1e-6.

Agreement with a Kaldi or torchaudio binary is not measured here: neither exists on the build machines; the oracle is the
formula of include/mfx.h.
"""
import numpy as np
import pytest

import kaldi_ref as KR
import tensor_ref as TR
import xform_ref
from conftest import synth_utterance
from kaldi_drive import FBANK80, MFCC13, Shape, check, make
from stft_drive import layout, run_batch, same_bits
from tail_ref import assert_norm_consistent, assert_tail_consistent

pytestmark = pytest.mark.gpu

W0, S0, M0 = FBANK80.W, FBANK80.S, FBANK80.M


# ---- 1. ragged batch ------------------------------------------------------------------------------------------------

def ragged_lengths():
    """No sample, one short of a frame, one frame, one short of two, two; 15, 16, 17 and 33 frames and a remainder: a chunk
    short of full, a full one, one frame into the second, one into the third."""
    return [0, 399, 400, 559, 560] + [W0 + (T - 1) * S0 + r for T, r in ((15, 3), (16, 159), (17, 1), (33, 80))]


RAGGED_FRAMES = [0, 0, 1, 1, 2, 15, 16, 17, 33]


@pytest.fixture(scope="module")
def ragged(pkg, a0001):
    utts = [synth_utterance(n, 300 + i) for i, n in enumerate(ragged_lengths())] + [a0001.copy()]
    m = make(pkg, FBANK80)
    got = run_batch(m, utts)        # (utterance 1 has 399 samples: every later one starts at an odd sample)
    m.close()
    for g in got:
        g.setflags(write=False)
    return utts, got


def test_ragged_batch_against_oracle(pkg, ragged):
    utts, got = ragged
    assert [g.shape[0] for g in got[:9]] == RAGGED_FRAMES
    worst = (0.0, 0.0)
    for i, (u, g) in enumerate(zip(utts, got)):
        want = FBANK80.oracle(u)
        assert want.shape == (KR.frame_count(u.size, W0, S0), M0) and g.shape == want.shape
        e = check(g, want, "utt %d (%d samples, %d frames)" % (i, u.size, want.shape[0]))
        worst = (max(worst[0], e[0]), max(worst[1], e[1]))
    print("ragged batch: worst max err / scale %.3g, rel L2 %.3g" % worst)


# ---- 2. bits ----------------------------------------------------------------------------------------------------------

def test_rows_do_not_depend_on_the_batch(pkg, ragged):
    utts, got = ragged
    m = make(pkg, FBANK80)
    for i, u in enumerate(utts):
        alone = run_batch(m, [u])[0]                 # (at sample 0: the other parity for all but the first two)
        assert same_bits(alone, got[i]), "utt %d alone differs from its rows in the batch" % i
    sub = run_batch(m, utts[3:9])                    # 559 samples first: 4 .. 8 start at odd samples behind it
    for i in range(3, 9):
        assert same_bits(sub[i - 3], got[i]), "utt %d in a sub-batch" % i
    shifted = run_batch(m, utts[3:9], first=1)       # ... and the whole sub-batch one sample on
    for i in range(3, 9):
        assert same_bits(shifted[i - 3], got[i]), "utt %d at another offset" % i
    again = run_batch(m, utts)
    for i in range(len(utts)):
        assert same_bits(again[i], got[i]), "second run differs, utt %d" % i
    m.close()


def test_device_entry_equals_host_entry_at_any_placement(pkg, ragged):
    import torch
    utts, got = ragged
    offs, lens, pcm_h = layout(utts)
    m = make(pkg, FBANK80)
    rows, total = m.batch_plan(offs, lens)
    dev = torch.device("cuda", 0)
    pcm = torch.from_numpy(pcm_h).to(dev)
    for lead in (32, 33):      # (33: the output at an odd word of the allocation)
        big = torch.full((lead + total * M0 + 64,), float("nan"), dtype=torch.float32, device=dev)
        torch.cuda.synchronize()
        m.batch_run_device(pcm.data_ptr(), pcm_h.size, big.data_ptr() + 4 * lead)
        m.synchronize()
        b = big.cpu().numpy()
        assert np.isnan(b[:lead]).all() and np.isnan(b[lead + total * M0:]).all(), "guard words written (lead %d)" % lead
        out = b[lead:lead + total * M0].reshape(total, M0)
        assert np.isfinite(out).all()
        for i in range(len(utts)):
            assert same_bits(out[rows[i]:rows[i] + got[i].shape[0]], got[i]), (lead, i)
    m.close()


# ---- 3. shape matrix, option matrix -------------------------------------------------------------------------------------

SHAPES = (
    Shape(400, 160, 23, 13, Q=22.0),
    Shape(400, 160, 40, 40, high=-400.0),
    Shape(200, 80, 23, 13, sr=8000.0),                 # N = 256
    Shape(100, 50, 10, 0, sr=4000.0),                  # N = 128
    Shape(65, 7, 3, 3, Q=0.0),
    Shape(512, 512, 128, 0, low=0.0),                  # band 0 is empty
)


def shape_utterances(sh):
    """45 frames and a remainder -- two full chunks and a cut one --, and 3 frames: an utterance that ends inside its first chunk."""
    return [synth_utterance(sh.W + 44 * sh.S + sh.S // 2, 11, sr=sh.sr), synth_utterance(sh.W + 2 * sh.S + 1, 12, sr=sh.sr)]


@pytest.mark.parametrize("sh", SHAPES, ids=[s.id() for s in SHAPES])
def test_shape_matrix(pkg, sh):
    utts = shape_utterances(sh)
    m = make(pkg, sh)
    assert m.dominant_kernel_name() == "k_kaldi_front" and m.fft_size() == KR.fft_size(sh.W)
    got = run_batch(m, utts)
    m.close()
    assert [g.shape for g in got] == [(45, sh.cols), (3, sh.cols)]
    worst = (0.0, 0.0)
    for i, u in enumerate(utts):
        e = check(got[i], sh.oracle(u), "%s utt %d" % (sh.id(), i))
        worst = (max(worst[0], e[0]), max(worst[1], e[1]))
    if sh.low == 0.0 and sh.C == 0:
        assert (got[0][:, 0] == got[0][0, 0]).all() and abs(float(got[0][0, 0]) + 15.9424) < 1e-4    # the empty band sits on the floor
    print("%s: worst max err / scale %.3g, rel L2 %.3g" % ((sh.id(),) + worst))


OPTIONS = {
    "preemph 0": dict(preemph=0.0),
    "DC removal off": dict(remove_dc=False),
    "magnitude": dict(use_power=False),
    "all three": dict(preemph=0.0, remove_dc=False, use_power=False),
}


@pytest.mark.parametrize("name", sorted(OPTIONS))
def test_option_matrix(pkg, name):
    sh = FBANK80.options(**OPTIONS[name])
    utts = shape_utterances(sh)
    utts[0] = (utts[0].astype(np.int32) // 2 + 900).astype(np.int16)      # (a DC offset for the DC removal to take out)
    m = make(pkg, FBANK80)
    default = run_batch(m, utts)
    m.kaldi_set_options(sh.preemph, sh.remove_dc, sh.use_power)
    got = run_batch(m, utts)
    m.kaldi_set_options()                                                   # back on Kaldi's defaults: the same bits as before
    back = run_batch(m, utts)
    m.close()
    for i, u in enumerate(utts):
        assert not same_bits(got[i], default[i]), "%s: the rows did not move (utt %d)" % (name, i)
        assert np.abs(got[i].astype(np.float64) - default[i]).max() > 1e-2, name
        assert same_bits(back[i], default[i])
        check(got[i], sh.oracle(u), "%s utt %d" % (name, i))
        check(default[i], FBANK80.oracle(u), "defaults utt %d" % i)


# ---- 4. edge signals ----------------------------------------------------------------------------------------------------

def edge_signals():
    n = W0 + 19 * S0 + 77
    t = np.arange(n)
    imp = np.zeros(n, np.int16)
    imp[n // 2] = 32767
    return {
        "tone": np.round(32767.0 * np.sin(2 * np.pi * 1000.0 * t / 16000.0)).astype(np.int16),
        "lsb": np.where(t % 2 == 0, 1, -1).astype(np.int16),
        "ramp": (t * 3 - 4000).astype(np.int16),
        "square": np.where((t // 8) % 2 == 0, 32767, -32768).astype(np.int16),
        "impulse": imp,
        "constant": np.full(n, 12345, np.int16),
        "silence": np.zeros(n, np.int16),
    }


ENERGY_BAR = 1e-4       # of the frame's largest mel energy


def test_edge_signals(pkg):
    sig = edge_signals()
    names = list(sig)
    m = make(pkg, FBANK80)
    got = dict(zip(names, run_batch(m, [sig[k] for k in names])))
    m.close()
    for k in ("impulse", "constant", "silence"):
        check(got[k], FBANK80.oracle(sig[k]), k)
    floor = got["silence"][0, 0]            # logf of the floor: one value, -15.9424 (its last bit is the device logf's)
    assert abs(float(floor) + 15.9424) < 1e-4
    for k in ("constant", "silence"):      # (a constant frame is its own mean: d = 0 exactly)
        assert got[k].shape == (20, M0) and (got[k] == floor).all(), k
    assert got["impulse"].max() > 10.0 and (got["impulse"][:7] == floor).all()
    worst = 0.0
    for k in ("tone", "lsb", "ramp", "square"):
        # in the log domain the leakage bands of these signals are rounding noise (a float32 restatement on the CPU misses the
        # log bar there); the energies are held to the frame's largest one
        want = np.maximum(FBANK80.oracle(sig[k], energies=True), KR.FLOOR)
        e = np.exp(got[k].astype(np.float64))
        assert np.isfinite(got[k]).all() and e.shape == want.shape == (20, M0)
        err = (np.abs(e - want) / want.max(axis=1, keepdims=True)).max()
        print("%s: worst energy err / frame maximum = %.3g (bar %.3g)" % (k, err, ENERGY_BAR))
        assert err <= ENERGY_BAR, (k, err)
        worst = max(worst, err)
    print("edge signals: worst energy err / frame maximum %.3g" % worst)


# ---- 5. composition ---------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def comp_utts():
    return [synth_utterance(W0 + 70 * S0 + 9, 401), synth_utterance(W0 + 16 * S0, 402), synth_utterance(W0 + 2 * S0 + 5, 403),
            synth_utterance(300, 404)]


COMP_FRAMES = [71, 17, 3, 0]


def test_deltas_and_cvn_against_their_own_statics(pkg, comp_utts):
    """dyn = ACC + CVN after the deltas on 400 / 160 / 23 / 13 (13 columns: the compact statics rows): the statics against the
    oracle, the deltas and the normalised rows against their own statics through tests/tail_ref.py."""
    l1 = l2 = 2
    m0 = make(pkg, MFCC13, norm=0, dyn=2, l1=l1, l2=l2)
    xs = run_batch(m0, comp_utts)
    m0.close()
    plain = make(pkg, MFCC13)
    ps = run_batch(plain, comp_utts)
    plain.close()
    m = pkg.MfccHip(200000, 400, 160, 23, 16000.0, 20.0, 0.0, 13, False, 22.0, 2, 2, l1, l2, True, device=0, bug_compat=False,
                    batch_norm_stats=1, method=pkg.METHOD_KALDI)
    m.set_window(pkg.povey_window(400))
    ys = run_batch(m, comp_utts)
    st = m.debug_read(6).reshape(3, len(comp_utts), 2, 13)
    m.close()
    for u, (x, y, p) in enumerate(zip(xs, ys, ps)):
        assert x.shape == y.shape == (COMP_FRAMES[u], 39)
        assert same_bits(x[:, :13], p), "the statics of a dyn = ACC handle are the plain handle's rows (utt %d)" % u
        if x.shape[0] == 0:
            continue
        check(x[:, :13], MFCC13.oracle(comp_utts[u]), "statics utt %d" % u)
        w = assert_tail_consistent(x, 13, 2, l1, l2, "deltas utt %d" % u)
        wm, wk, keep = assert_norm_consistent(y, x, st[:, u], 2, True, 13, x.shape[0], "CVN utt %d" % u)
        assert keep.all()
        print("utt %d: deltas err / bound %s, CVN mean %.3g multiplier %.3g of their bounds" % (u, w, wm, wk))


def test_transform_tensor_pitch(pkg, comp_utts):
    offs, lens, pcm = layout(comp_utts)
    m = make(pkg, Shape(400, 160, 8, 0))
    rows, total = m.batch_plan(offs, lens)
    y = m.batch_run_host(pcm)
    frames = [m.batch_frames(int(n)) for n in lens]
    assert frames == COMP_FRAMES and total == sum(frames)
    # splice +-2 -> 24
    rng = np.random.default_rng(9)
    A = rng.standard_normal((24, 40)).astype(np.float32)
    b = rng.standard_normal(24).astype(np.float32)
    m.batch_set_transform(A, b, left=2, right=2)
    assert m.batch_output_width() == 24
    got = m.batch_run_host(pcm)
    xform_ref.assert_xform_consistent(got, y, rows, frames, A, b, 2, 2, what="kaldi transform")
    m.batch_set_transform(None)
    # channel-major half tensor of the plain rows
    m.batch_set_tensor(TR.CHANNEL_MAJOR, TR.F16, 0, -1.0)
    t = m.batch_run_host(pcm)
    assert t.shape == (len(comp_utts), 8, max(frames))
    assert TR.same_bits(t, TR.tensor_ref(y, rows, frames, max(frames), TR.CHANNEL_MAJOR, TR.F16, -1.0), TR.F16)
    m.batch_clear_tensor()
    # the pitch track runs beside the rows and leaves their bits alone
    m.batch_set_pitch(40, 200)
    assert same_bits(m.batch_run_host(pcm), y)
    lag, rho = m.batch_pitch_read()[:2]
    assert lag.shape[0] == total and np.isfinite(rho).all() and np.isfinite(lag).all()
    m.batch_clear_pitch()
    # the VAD's default column is the last static column; c0 of an MFCC handle is column 0
    m.batch_set_vad(mode=pkg.VAD_FLAGS)
    assert same_bits(m.batch_run_host(pcm), y)
    flags, voiced, thr, tv = m.batch_vad_read()
    assert flags.size == total and voiced.sum() == tv
    m.close()


# ---- 6. driver --------------------------------------------------------------------------------------------------------

def test_driver(pkg, orc, tmp_path):
    import os
    import subprocess
    from conftest import GOLDEN, ROOT
    exe = os.path.join(ROOT, "asr-featext-opencl_amd", "host", "afet_hip")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", os.path.dirname(exe)])
    wav = os.path.join(GOLDEN, "a0001.wav")
    pcm, sr = orc.read_wav_pcm16(wav)
    assert sr == 16000 and pcm.shape[1] == 1
    pcm = pcm[:, 0].copy()

    def rows_of(path):
        return np.array([[float(v) for v in line.strip().strip("|").split("|")] for line in open(path)])

    t = tmp_path / "r.txt"
    base = [exe, "--method", "KALDI", "--norm", "0", "--dyn", "0"]
    subprocess.check_call(base + ["--banks", "80", "--ceps", "0", wav, str(t)])                  # fbank-80, Kaldi's defaults
    rows = rows_of(t)
    want = FBANK80.oracle(pcm)
    assert rows.shape == (want.shape[0], 1 + 80)
    check(rows[:, 1:], want, "afet_hip --method KALDI fbank-80")
    sh = MFCC13.options(preemph=0.5, remove_dc=False, use_power=False, high=-400.0)
    subprocess.check_call(base + ["--banks", "23", "--ceps", "13", "--high-freq", "-400", "--preemph", "0.5", "--no-dc-removal", "--magnitude",
                                  wav, str(t)])
    rows = rows_of(t)
    want = sh.oracle(pcm)
    assert rows.shape == (want.shape[0], 1 + 13)
    check(rows[:, 1:], want, "afet_hip --method KALDI MFCC 13, options")
    for bad in (["--method", "KALDI", "--preemph", "1.5"], ["--preemph", "0.5"], ["--magnitude"], ["--method", "KALDI", "--alpha-min", "1.0", "--alpha-max", "1.3", "--alpha-step", "0.1"],
                ["--method", "KALDI", "--batch-mb", "0"]):
        r = subprocess.run([exe] + bad + [wav, str(t)], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        assert r.returncode == 2, bad


# ---- 7. refusals ------------------------------------------------------------------------------------------------------

def test_refusals_on_real_handles(pkg, comp_utts):
    offs, lens, pcm = layout(comp_utts)
    m = make(pkg, FBANK80)
    m.batch_plan(offs, lens)
    want = m.batch_run_host(pcm)
    with pytest.raises(pkg.MfxError) as e:
        m.batch_set_alphas(np.ones(len(comp_utts), np.float32))
    assert e.value.status == -5 and "Kaldi" in str(e.value)
    m.set_alpha(1.2)                # accepted, no effect
    u = comp_utts[0]
    for call in (lambda: m.set_input(u[:4000]), m.flush, m.apply, lambda: m.get_output_data(1), lambda: m.apply_alphas([1.0]),
                 lambda: m.get_output_data_alpha(0, 1)):
        with pytest.raises(pkg.MfxError) as e:
            call()
        assert e.value.status == -8 and "batch" in str(e.value)
    for bad in ((-0.5, 1, 1), (1.5, 1, 1), (float("nan"), 1, 1), (0.97, 2, 1), (0.97, 1, -1)):
        with pytest.raises(pkg.MfxError) as e:
            m.kaldi_set_options(*bad)
        assert e.value.status == -7, bad
    assert same_bits(m.batch_run_host(pcm), want)       # every refusal left the handle as it was
    m.sessions_create(2, 1600)
    with pytest.raises(pkg.MfxError) as e:              # an open stream's bits must not change under it
        m.kaldi_set_options(0.5, 1, 1)
    assert e.value.status == -8
    m.sessions_create(0, 0)
    m.kaldi_set_options(0.5, 1, 1)
    assert not same_bits(m.batch_run_host(pcm), want)
    m.close()
    other = pkg.MfccHip(200000, 400, 160, 23, 16000.0, 64.0, 8000.0, 13, False, 22.0, device=0, bug_compat=False)
    with pytest.raises(pkg.MfxError) as e:
        other.kaldi_set_options()
    assert e.value.status == -5
    other.close()
    for kw in (dict(W=64, S=32), dict(W=513), dict(M=129), dict(C=24, M=23)):
        sh = Shape(kw.get("W", 400), kw.get("S", 160), kw.get("M", 80), kw.get("C", 0))
        with pytest.raises(pkg.MfxError) as e:
            make(pkg, sh)
        assert e.value.status == -5, kw
    with pytest.raises(pkg.MfxError) as e:
        pkg.MfccHip(200000, 400, 160, 23, 16000.0, 20.0, 0.0, 13, True, 22.0, device=0, method=pkg.METHOD_KALDI)     # want_c0
    assert e.value.status == -5
