"""The Kaldi front end's options (kaldi_flags of mfx_create_kaldi: k_kaldi_front_opts) on the MI355X.

Twin bits.  Every row of a NO_SNIP_EDGES batch is the bit pattern a flags-0 handle writes for the utterance's padded twin y, built
on the host through Kaldi's loop (tests/kaldi_opts_ref.padded_twin; tests/test_kaldi_opts_host.py shows on the oracle that the
two are the same arithmetic on the same samples).  The utterances lie in one PCM array between full-scale fillers of 3 samples
that belong to no utterance, so most start at odd samples and a mirror that crossed into a neighbour would read +-32767.
Accuracy.  The same rows, the two energies, the floor and the column orders against the float64 oracle of
tests/kaldi_opts_ref.py at the project bar as tests/test_kaldi_gpu.py applies it (conftest.assert_close: 1e-4 of scale, 1e-5
relative L2).  Column bits, the stages behind the front end, the two entries, placement, and the two refusals follow.
Agreement with a Kaldi / kaldifeat / torchaudio binary is not measured: none exists on the build machines."""
import numpy as np
import pytest

import kaldi_opts_ref as KO
import kaldi_ref as KR
import tensor_ref as TR
import xform_ref
from conftest import synth_utterance
from kaldi_drive import Shape, check
from stft_drive import same_bits
from tail_ref import assert_norm_consistent, assert_tail_consistent

pytestmark = pytest.mark.gpu

NSE, EN, WIN, HTK = KO.NO_SNIP_EDGES, KO.USE_ENERGY, KO.ENERGY_WINDOWED, KO.HTK_COMPAT
FULL = np.array([32767, -32767, 32767], np.int16)       # between the utterances, part of none


def make(pkg, sh, flags=0, floor=0.0, norm=0, dyn=0, l1=2, l2=2, **kw):
    m = pkg.MfccHip(200000, sh.W, sh.S, sh.M, sh.sr, sh.low, sh.high, sh.C, False, sh.Q, norm, dyn, l1, l2, True, device=0,
                    bug_compat=False, method=pkg.METHOD_KALDI, kaldi_flags=flags, kaldi_energy_floor=floor, **kw)
    m.set_window(sh.taps())
    m.kaldi_set_options(sh.preemph, sh.remove_dc, sh.use_power)
    return m


def oracle(sh, pcm, flags=0, floor=0.0):
    return KO.features(pcm, sh.taps(), sh.S, sh.M, sh.sr, sh.low, sh.high, sh.C, sh.Q, sh.preemph, sh.remove_dc, sh.use_power, flags, floor)


def packed(utts):
    """offsets, lengths, pcm: the utterances with full-scale fillers in front of, between and behind them."""
    parts, offs, at = [FULL], [], FULL.size
    for u in utts:
        offs.append(at)
        parts += [u, FULL]
        at += u.size + FULL.size
    return np.array(offs, np.int64), np.array([u.size for u in utts], np.int64), np.concatenate(parts + [np.zeros(2, np.int16)])


def run(m, utts):
    offs, lens, pcm = packed(utts)
    rows, total = m.batch_plan(offs, lens)
    out = m.batch_run_host(pcm)
    assert out.shape == (total, m.get_output_data_width())
    return [out[rows[i]:rows[i] + m.batch_frames(int(lens[i]))] for i in range(len(utts))]


# ---- 1. snip_edges = false: the padded twin's bits, and the oracle --------------------------------------------------------------

WS = ((400, 160), (401, 161), (512, 512), (65, 1), (200, 80))
TWIN_SHAPES = [Shape(W, S, 23, C, sr=8000.0 if W == 200 else 16000.0) for W, S in WS for C in (0, 13)]


def twin_lengths(S):
    """Reflections that repeat (1 .. 199 samples under windows of up to 512); chunk and tail-piece boundaries; 3 s."""
    return [1, 79, 80, 81, 199, 16 * S, 17 * S, 33 * S + 7, 48000]


@pytest.fixture(scope="module")
def centred(pkg):
    """shape id -> (utterances, rows of the NO_SNIP_EDGES batch), computed once"""
    cache = {}

    def get(sh):
        if sh.id() not in cache:
            utts = [synth_utterance(n, 900 + i) for i, n in enumerate(twin_lengths(sh.S))]
            m = make(pkg, sh, NSE)
            got = run(m, utts)
            m.close()
            for g in got:
                g.setflags(write=False)
            cache[sh.id()] = (utts, got)
        return cache[sh.id()]
    return get


@pytest.mark.parametrize("sh", TWIN_SHAPES, ids=[s.id() for s in TWIN_SHAPES])
def test_centred_rows_are_the_padded_twins_bits(pkg, centred, sh):
    utts, got = centred(sh)
    assert [g.shape[0] for g in got] == [KO.frame_count(u.size, sh.W, sh.S, NSE) for u in utts]
    twins = [KO.padded_twin(u, sh.W, sh.S) for u in utts]
    m = make(pkg, sh, 0)
    want = run(m, twins)
    m.close()
    rows = 0
    for i, (g, w) in enumerate(zip(got, want)):
        assert same_bits(g, w), "utt %d (%d samples, %d frames) differs from its padded twin" % (i, utts[i].size, w.shape[0])
        rows += g.shape[0]
    assert rows > 0
    print("%s: %d rows, the padded twins' bits" % (sh.id(), rows))


@pytest.mark.parametrize("sh", TWIN_SHAPES, ids=[s.id() for s in TWIN_SHAPES])
def test_centred_rows_against_the_oracle(pkg, centred, sh):
    utts, got = centred(sh)
    worst = (0.0, 0.0)
    for i, (u, g) in enumerate(zip(utts, got)):
        e = check(g, oracle(sh, u, NSE), "%s utt %d (%d samples)" % (sh.id(), i, u.size))
        worst = (max(worst[0], e[0]), max(worst[1], e[1]))
    print("%s centred: worst max err / scale %.3g, rel L2 %.3g" % ((sh.id(),) + worst))


def test_centred_rows_do_not_depend_on_the_batch_or_the_offset(pkg, centred):
    sh = TWIN_SHAPES[0]
    utts, got = centred(sh)
    m = make(pkg, sh, NSE)
    for i in (0, 3, 4, 7):
        offs, lens, pcm = np.array([0], np.int64), np.array([utts[i].size], np.int64), np.concatenate([utts[i], np.zeros(2, np.int16)])
        rows, total = m.batch_plan(offs, lens)
        assert same_bits(m.batch_run_host(pcm), got[i]), "utt %d alone at sample 0" % i
    again = run(m, utts)
    assert all(same_bits(a, g) for a, g in zip(again, got))
    m.close()


# ---- 2. energy ------------------------------------------------------------------------------------------------------------

ENERGY_UTTS = [400, 560, 400 + 16 * 160 + 3, 400 + 40 * 160 + 159]


@pytest.mark.parametrize("remove_dc", (True, False), ids=("dc", "nodc"))
@pytest.mark.parametrize("flags", (EN, EN | WIN), ids=("raw", "windowed"))
@pytest.mark.parametrize("C", (0, 13), ids=("fbank23", "mfcc13"))
def test_energy_against_the_oracle(pkg, C, flags, remove_dc):
    sh = Shape(400, 160, 23, C, remove_dc=remove_dc)
    utts = [(synth_utterance(n, 40 + i).astype(np.int32) + (1500 if i & 1 else 0)).clip(-32768, 32767).astype(np.int16)
            for i, n in enumerate(ENERGY_UTTS)]
    m = make(pkg, sh, flags, floor=3.0)
    got = run(m, utts)
    m.close()
    worst = (0.0, 0.0)
    for i, (u, g) in enumerate(zip(utts, got)):
        want = oracle(sh, u, flags, 3.0)
        e = check(g, want, "utt %d" % i)
        ee = check(g[:, :1], want[:, :1], "utt %d, the energy column alone" % i)
        worst = (max(worst[0], e[0], ee[0]), max(worst[1], e[1], ee[1]))
    print("energy C %d flags %d dc %d: worst max err / scale %.3g, rel L2 %.3g" % (C, flags, remove_dc, worst[0], worst[1]))


def test_energy_edge_signals(pkg):
    """Silence: exactly logf(0x1p-23f) -- the DEVICE's logf, whose result at this argument (-15.942386 on gfx950) lies one ulp
    from the correctly rounded -15.942385, inside the 1 ulp the device library states for logf: the column is held to the bits
    the same kernel's logf writes into the mel columns of silence (the floor of the existing definition, the same function at the
    same argument), and to within one ulp of the correctly rounded value -- and exactly 0 under energy_floor = 1.  A constant with DC removal: d = 0, the floor.
    Full-scale alternation at W = 512, the largest energy a frame can have (512 x 32767^2 = 5.5e11): finite; the energy column
    within the bar (the mel columns of that signal are leakage of a line at the Nyquist bin, which carries no band: they are
    held finite here, and to the oracle on ordinary signals above)."""
    silence = np.float32(np.log(np.float64(np.float32(2.0 ** -23))))
    sh = Shape(400, 160, 23, 0)
    zero, const = np.zeros(2000, np.int16), np.full(2000, 12345, np.int16)
    for flags in (EN, EN | WIN):
        m = make(pkg, sh, flags)
        z, c = run(m, [zero, const])
        m.close()
        assert z.shape == (11, 24) and same_bits(z[:, 0], z[:, 1]) and same_bits(z[:, 0], np.full(11, z[0, 23], np.float32)), z[:, 0]
        assert (np.abs(z[:, 0] - silence) <= np.spacing(np.abs(silence))).all(), z[:, 0]
        assert same_bits(c[:, 0], z[:, 0]), c[:, 0]          # (mean = 12345 exactly: d = 0)
        m = make(pkg, sh, flags, floor=1.0)
        z, c = run(m, [zero, const])
        m.close()
        assert same_bits(z[:, 0], np.zeros(11, np.float32)) and same_bits(c[:, 0], np.zeros(11, np.float32))
    alt = (32767 * (1 - 2 * (np.arange(4096) & 1))).astype(np.int16)
    for dc in (True, False):
        big = Shape(512, 160, 23, 0, remove_dc=dc)
        for flags in (EN, EN | WIN):
            m = make(pkg, big, flags)
            g = run(m, [alt])[0]
            m.close()
            assert np.isfinite(g).all()
            want = oracle(big, alt, flags)
            check(g[:, :1], want[:, :1], "full-scale alternation, flags %d, dc %d (logE = %.4f)" % (flags, dc, want[0, 0]))
    assert abs(oracle(Shape(512, 160, 23, 0, remove_dc=False), alt, EN)[0, 0] - np.log(512 * 32767.0 ** 2)) < 1e-9


# ---- 3. column bits ---------------------------------------------------------------------------------------------------------

COL_SHAPES = [Shape(400, 160, 23, 13), Shape(400, 160, 23, 0), Shape(400, 160, 128, 0), Shape(400, 160, 23, 1), Shape(200, 80, 23, 13, sr=8000.0)]


@pytest.mark.parametrize("sh", COL_SHAPES, ids=[s.id() for s in COL_SHAPES])
def test_columns_are_the_plain_handles_bits_in_the_stated_order(pkg, sh):
    utts = [synth_utterance(n, 70 + i) for i, n in enumerate((sh.W, sh.W + 16 * sh.S + 5, sh.W + 20 * sh.S))]
    out = {}
    for flags in (0, EN, HTK, EN | HTK, EN | WIN | HTK):
        m = make(pkg, sh, flags)
        out[flags] = np.concatenate(run(m, utts))
        m.close()
    p, e, h, eh, ewh = (out[f] for f in (0, EN, HTK, EN | HTK, EN | WIN | HTK))
    M, C = sh.M, sh.C
    if C == 0:
        assert p.shape[1] == M and e.shape[1] == M + 1 == eh.shape[1]
        assert same_bits(e[:, 1:], p), "fbank + energy: columns 1 .. M are the plain handle's"
        assert same_bits(h, p), "HTK_COMPAT without energy changes nothing on fbank"
        assert same_bits(eh[:, :M], p) and same_bits(eh[:, M], e[:, 0]), "HTK: the bands, then the energy"
        assert same_bits(ewh[:, :M], p) and not same_bits(ewh[:, M], e[:, 0])
    else:
        assert p.shape[1] == e.shape[1] == h.shape[1] == eh.shape[1] == C
        assert same_bits(e[:, 1:], p[:, 1:]), "MFCC + energy: columns 1 .. C - 1 are the plain handle's"
        assert not same_bits(e[:, 0], p[:, 0])
        c0s = (p[:, 0].astype(np.float64) * KO.SQRT2).astype(np.float32)
        assert same_bits(h[:, :C - 1], p[:, 1:]) and same_bits(h[:, C - 1], c0s), "HTK: c1 .. first, then c0 sqrt 2"
        assert same_bits(eh[:, :C - 1], p[:, 1:]) and same_bits(eh[:, C - 1], e[:, 0]), "HTK + energy"
    check(ewh, np.concatenate([oracle(sh, u, EN | WIN | HTK) for u in utts]), "%s, windowed energy, HTK order" % sh.id())


# ---- 4. behind the front end ---------------------------------------------------------------------------------------------------

COMP = Shape(400, 160, 23, 0)
COMP_FLAGS = NSE | EN


def comp_utts():
    return [synth_utterance(n, 80 + i) for i, n in enumerate((11283, 2801, 81, 79))]          # 71, 18, 1, 0 frames


def test_deltas_and_cmn_behind_centred_fbank_with_energy(pkg):
    utts, l1, l2 = comp_utts(), 2, 2
    plain = make(pkg, COMP, COMP_FLAGS)
    ps = run(plain, utts)
    plain.close()
    m0 = make(pkg, COMP, COMP_FLAGS, dyn=2, l1=l1, l2=l2)
    xs = run(m0, utts)
    m0.close()
    m = make(pkg, COMP, COMP_FLAGS, norm=1, dyn=2, l1=l1, l2=l2, batch_norm_stats=1)
    ys = run(m, utts)
    st = m.debug_read(6).reshape(3, len(utts), 2, 24)
    m.close()
    assert [x.shape[0] for x in xs] == [71, 18, 1, 0]
    for u, (x, y, p) in enumerate(zip(xs, ys, ps)):
        assert x.shape == y.shape == (p.shape[0], 72) and p.shape[1] == 24
        assert same_bits(x[:, :24], p), "statics of the dyn = ACC handle (utt %d)" % u
        if x.shape[0] == 0:
            continue
        check(p, oracle(COMP, utts[u], COMP_FLAGS), "statics utt %d" % u)
        w = assert_tail_consistent(x, 24, 2, l1, l2, "deltas utt %d" % u)
        wm, wk, keep = assert_norm_consistent(y, x, st[:, u], 1, True, 24, x.shape[0], "CMN utt %d" % u)
        assert keep.all()
        print("utt %d: deltas err / bound %s, CMN mean %.3g of its bound" % (u, w, wm))


def test_transform_and_tensor_behind_the_options(pkg):
    utts = comp_utts()
    sh = Shape(400, 160, 8, 0)
    offs, lens, pcm = packed(utts)
    m = make(pkg, sh, COMP_FLAGS | HTK)
    rows, total = m.batch_plan(offs, lens)
    y = m.batch_run_host(pcm)
    frames = [m.batch_frames(int(n)) for n in lens]
    assert frames == [71, 18, 1, 0] and total == sum(frames) and y.shape == (total, 9)
    rng = np.random.default_rng(9)
    A, b = rng.standard_normal((24, 45)).astype(np.float32), rng.standard_normal(24).astype(np.float32)
    m.batch_set_transform(A, b, left=2, right=2)
    assert m.batch_output_width() == 24
    xform_ref.assert_xform_consistent(m.batch_run_host(pcm), y, rows, frames, A, b, 2, 2, what="transform behind the options")
    m.batch_set_transform(None)
    m.batch_set_tensor(TR.CHANNEL_MAJOR, TR.F16, 0, -1.0)
    t = m.batch_run_host(pcm)
    assert t.shape == (len(utts), 9, max(frames))
    assert TR.same_bits(t, TR.tensor_ref(y, rows, frames, max(frames), TR.CHANNEL_MAJOR, TR.F16, -1.0), TR.F16)
    m.batch_clear_tensor()
    # the VAD's default column is the last static one: the energy under HTK_COMPAT
    m.batch_set_vad(mode=pkg.VAD_FLAGS)
    assert same_bits(m.batch_run_host(pcm), y)
    flags, voiced, thr, tv = m.batch_vad_read()
    assert flags.size == total and voiced.sum() == tv
    m.close()


@pytest.mark.parametrize("C", (0, 13), ids=("fbank23", "mfcc13"))
def test_device_entry_equals_host_entry_at_an_odd_placement(pkg, C):
    import torch
    sh = Shape(400, 160, 23, C)
    flags = NSE | EN | HTK
    utts = comp_utts()
    offs, lens, pcm_h = packed(utts)
    m = make(pkg, sh, flags)
    rows, total = m.batch_plan(offs, lens)
    host = m.batch_run_host(pcm_h)
    width = m.get_output_data_width()
    assert width == (24 if C == 0 else 13)
    dev = torch.device("cuda", 0)
    pcm = torch.from_numpy(pcm_h).to(dev)
    for lead in (32, 33):
        big = torch.full((lead + total * width + 64,), float("nan"), dtype=torch.float32, device=dev)
        torch.cuda.synchronize()
        m.batch_run_device(pcm.data_ptr(), pcm_h.size, big.data_ptr() + 4 * lead)
        m.synchronize()
        b = big.cpu().numpy()
        assert np.isnan(b[:lead]).all() and np.isnan(b[lead + total * width:]).all(), "guard words written (lead %d)" % lead
        assert same_bits(b[lead:lead + total * width].reshape(total, width), host), lead
    m.close()


# ---- 5. refusals ---------------------------------------------------------------------------------------------------------

def test_sessions_and_pitch_are_refused_on_a_centred_handle_which_stays_usable(pkg):
    sh = Shape(400, 160, 23, 13)
    utts = comp_utts()
    m = make(pkg, sh, NSE | EN)
    before = run(m, utts)
    with pytest.raises(pkg.MfxError) as e:
        m.sessions_create(2, 4000)
    assert e.value.status == -8 and "batch entries" in str(e.value)
    with pytest.raises(pkg.MfxError) as e:
        m.batch_set_pitch(40, 200)
    assert e.value.status == -5 and "NO_SNIP_EDGES" in str(e.value)
    after = run(m, utts)
    assert all(same_bits(a, b) for a, b in zip(after, before))
    m.close()
    # the energy and HTK options alone keep both
    m = make(pkg, sh, EN | HTK)
    m.sessions_create(2, 4000)
    m.sessions_create(0, 0)
    offs, lens, pcm = packed(utts)
    m.batch_plan(offs, lens)
    m.batch_set_pitch(40, 200)
    m.batch_clear_pitch()
    m.close()
