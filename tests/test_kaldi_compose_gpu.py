"""The "Entries" paragraph of MFX_METHOD_KALDI in include/mfx.h on the MI355X: "all batch attachments work", and the session
entries serve the method with mfx_sessions_set_transform and mfx_sessions_set_rates "unchanged".  Each claim once, on Kaldi
handles under the asymmetric ramp window (tests/kaldi_ref.py), at utterances of 71, 17, 3 and 0 frames, each stage held to the
restatement the project already has for it and fed with the Kaldi handle's own rows from before the setter: the rates plan
(a twin planned plainly on the converted samples; the float64 oracle of those samples), the speaker list (tests/spk_ref.py), the
VAD on c0 and on the default column (tests/vad_ref.py), the pitch track and the pasted pitch features (mfx_host_pitch; the
feats array), the overlap mode, the session transform (tests/xform_ref.py) and the session rates (the rates plan's bits).

Agreement with a Kaldi or torchaudio binary remains unmeasured."""
import numpy as np
import pytest

import kaldi_windows_cases as KC
import sess_resample_drive as RD
import sess_xform_drive as XD
import spk_ref
import vad_ref as VR
import xform_ref as XR
from conftest import synth_utterance
from kaldi_drive import Shape, check, make
from stft_drive import layout, same_bits

pytestmark = pytest.mark.gpu

W, S = 400, 160
MFCC = KC.COMP_SHAPE
SMALL = Shape(W, S, 8, 0, window="ramp")
FRAMES, LENGTHS, VAD = KC.COMP_FRAMES, KC.COMP_LENGTHS, KC.VAD
comp_utts, enveloped = KC.comp_utts, KC.enveloped


def plain_run(pkg, sh, utts, **kw):
    """(handle, offsets, lengths, pcm, rows, total, y): planned and run once, nothing attached."""
    offs, lens, pcm = layout(utts)
    m = make(pkg, sh, **kw)
    rows, total = m.batch_plan(offs, lens)
    y = m.batch_run_host(pcm)
    assert [m.batch_frames(int(n)) for n in lens] == FRAMES and total == sum(FRAMES)
    return m, offs, lens, pcm, rows, total, y


# ---- mfx_batch_plan_rates --------------------------------------------------------------------------------------------------------

def test_rates_plan_rows_are_a_plain_twins_bits_and_the_oracle_of_the_converted_samples(pkg):
    rates = [48000, 8000, 16000, 48000]
    utts = [synth_utterance(3 * LENGTHS[0], 411, sr=48000.0), synth_utterance(LENGTHS[1] // 2, 412, sr=8000.0),
            synth_utterance(LENGTHS[2], 413), synth_utterance(3 * LENGTHS[3], 414, sr=48000.0)]
    offs, lens, pcm = layout(utts)
    m, t = make(pkg, MFCC), make(pkg, MFCC)
    rows, total = m.batch_plan_rates(offs, lens, rates)
    got = m.batch_run_host(pcm)
    y = m.debug_read(8)
    off, ln, tot = m.batch_resample_layout()
    assert ln.tolist() == [LENGTHS[0], LENGTHS[1], LENGTHS[2], LENGTHS[3]] and [m.batch_frames(int(n)) for n in ln] == FRAMES
    assert np.array_equal(y[off[2]:off[2] + ln[2]], utts[2])                       # the 16 kHz utterance passes through
    trows, ttotal = t.batch_plan(off, ln)
    assert trows.tolist() == rows.tolist() and ttotal == total == sum(FRAMES)
    want = t.batch_run_host(np.concatenate([y, np.zeros(8, np.int16)]))
    m.close(), t.close()
    assert got.shape == (total, 13) and same_bits(got, want)
    for u in range(4):
        check(got[rows[u]:rows[u] + FRAMES[u]], MFCC.oracle(y[off[u]:off[u] + ln[u]]), "rates plan, utt %d at %d Hz" % (u, rates[u]))


# ---- mfx_batch_set_speakers ------------------------------------------------------------------------------------------------------

def test_speaker_list_pools_cmn_over_kaldi_rows(pkg):
    utts = comp_utts()
    t, offs, lens, pcm, rows, total, x = plain_run(pkg, MFCC, utts)
    t.close()
    xs = [x[rows[u]:rows[u] + FRAMES[u]] for u in range(4)]
    ids = [0, 1, 1, 0]                               # speaker 0: 71 + 0 frames, speaker 1: 17 + 3
    m = make(pkg, MFCC, norm=1)
    m.batch_plan(offs, lens)
    m.batch_set_speakers(ids, 2)
    y = m.batch_run_host(pcm)
    count, acc, stats = m.batch_speaker_stats()
    m.close()
    ys = [y[rows[u]:rows[u] + FRAMES[u]] for u in range(4)]
    assert count.tolist() == [71, 20] and stats.shape == (2, 2, 13)
    for s in range(2):
        mine = [u for u in range(4) if ids[u] == s]
        wm, wk, keep = spk_ref.assert_speaker_consistent([ys[u] for u in mine], [xs[u] for u in mine], stats[s], 1, 13,
                                                         what="Kaldi MFCC 13 under CMN, speaker %d" % s)
        assert keep.all()
        print("speaker %d: mean err / bound %.3g" % (s, wm))
    assert not same_bits(ys[1], xs[1])


# ---- mfx_batch_set_vad -----------------------------------------------------------------------------------------------------------

def test_vad_decides_on_c0_and_on_the_default_column(pkg):
    KC.vad_input_condition()
    utts = enveloped()
    m, offs, lens, pcm, rows, total, y = plain_run(pkg, MFCC, utts)
    seen = {}
    for column in (0, -1):
        col = 12 if column < 0 else column
        m.batch_set_vad(column, *VAD, pkg.VAD_FLAGS)
        assert same_bits(m.batch_run_host(pcm), y), "FLAGS moved the rows"
        flags, voiced, thr, tv = m.batch_vad_read()
        assert flags.shape == (total,) and tv == int(flags.sum())
        for u, (r0, T) in enumerate(zip(rows, FRAMES)):
            e = y[r0:r0 + T, col]
            want, bound = VR.thr_ref(e, VAD[0], VAD[1])
            if T == 0:
                assert thr[u] == np.float32(VAD[0]) and voiced[u] == 0
                continue
            assert abs(float(thr[u]) - want) <= bound, (column, u, float(thr[u]), want, bound)
            assert np.array_equal(flags[r0:r0 + T], VR.flags_ref(e, thr[u], VAD[2], VAD[3])), (column, u)
            assert voiced[u] == int(flags[r0:r0 + T].sum())
        assert 0.2 * FRAMES[0] <= voiced[0] <= 0.8 * FRAMES[0]
        m.batch_set_vad(column, *VAD, pkg.VAD_SELECT)
        got = m.batch_run_host(pcm)
        dec = m.batch_vad_read()
        assert np.array_equal(dec[0], flags) and same_bits(dec[2], thr)
        assert same_bits(got, VR.select_ref(y, rows, FRAMES, flags)), "SELECT on column %d" % column
        seen[column] = flags
    m.close()
    assert not np.array_equal(seen[0], seen[-1]), "c0 and the default column decide alike: the column is not read where the header says"


# ---- mfx_batch_set_pitch, mfx_batch_set_pitch_feats --------------------------------------------------------------------------------

def test_pitch_track_and_pasted_pitch_features(pkg):
    utts = comp_utts()
    m, offs, lens, pcm, rows, total, y = plain_run(pkg, SMALL, utts)
    m.batch_set_pitch(40, 200)
    assert same_bits(m.batch_run_host(pcm), y)
    lag, rho, idx = m.batch_pitch_read()
    for u, (r0, T) in enumerate(zip(rows, FRAMES)):            # the Kaldi front end does not change what the pitch kernels read
        h = pkg.host_pitch(utts[u], T, S, W, 40, 200)
        assert same_bits(lag[r0:r0 + T], h[0]) and same_bits(rho[r0:r0 + T], h[1]) and np.array_equal(idx[r0:r0 + T], h[2]), "utt %d" % u
    assert lag.shape == (total,) and (lag >= 40).all() and (lag <= 200).all()
    m.batch_set_pitch_feats(paste=True)
    assert m.batch_output_width() == 8 + 3
    wide = m.batch_run_host(pcm)
    feats = m.batch_pitch_feats_read()
    assert wide.shape == (total, 11) and feats.shape == (total, 3) and np.isfinite(feats).all()
    assert same_bits(wide[:, 8:], feats) and same_bits(wide[:, :8], y)
    lag2, rho2, idx2 = m.batch_pitch_read()
    assert same_bits(lag2, lag) and same_bits(rho2, rho)
    m.batch_clear_pitch()
    assert m.batch_output_width() == 8 and same_bits(m.batch_run_host(pcm), y)
    m.close()


# ---- mfx_batch_overlap -----------------------------------------------------------------------------------------------------------

def test_overlap_mode_three_runs_in_flight_deliver_the_plain_bytes(pkg):
    import torch
    utts = comp_utts()
    m, offs, lens, pcm, rows, total, y = plain_run(pkg, MFCC, utts, dyn=2, l1=2, l2=2)
    assert y.shape == (total, 39)
    m.batch_overlap(True)
    dev = torch.device("cuda:0")
    d_pcm = torch.from_numpy(pcm.copy()).to(dev)
    outs = [torch.full((total, 39), float("nan"), dtype=torch.float32, device=dev) for _ in range(3)]
    torch.cuda.synchronize()
    for o in outs:
        m.batch_run_device(d_pcm.data_ptr(), d_pcm.numel(), o.data_ptr())
    m.synchronize()
    for i, o in enumerate(outs):
        assert same_bits(o.cpu().numpy(), y), "overlapped batch %d" % i
    m.batch_overlap(False)
    assert same_bits(m.batch_run_host(pcm), y)
    m.close()


# ---- mfx_sessions_set_transform ----------------------------------------------------------------------------------------------------

def test_session_transform_on_kaldi_streams(pkg):
    utts = comp_utts()
    t, offs, lens, pcm, rows, total, y = plain_run(pkg, MFCC, utts)
    rng = np.random.default_rng(21)
    left, right, od = 2, 1, 24
    A = (rng.standard_normal((od, (left + right + 1) * 13)) / np.sqrt(4 * 13)).astype(np.float32)
    b = rng.standard_normal(od).astype(np.float32)
    t.batch_set_transform(A, b, left=left, right=right)
    twin = t.batch_run_host(pcm)                     # the batch attachment: existing, separately tested code
    t.close()
    m = make(pkg, MFCC)
    m.sessions_set_transform(A, b, left=left, right=right)
    assert m.sessions_output_width() == od and m.get_output_data_width() == 13
    m.sessions_create(3, 3000)
    got = XD.drive(m, [u.reshape(-1, 1) for u in utts], 3, XD.OD.cut_random_with_empty, 31, right)    # (asserts the delivery rule)
    m.close()
    cat = np.concatenate([got[u] for u in range(4)])
    assert [got[u].shape[0] for u in range(4)] == FRAMES and cat.shape == (total, od)
    XR.assert_xform_consistent(cat, y, [int(r) for r in rows], FRAMES, A, b, left, right, what="session transform on Kaldi rows")
    assert same_bits(cat, twin), "the session transform's rows are not the batch attachment's bits"


# ---- mfx_sessions_set_rates --------------------------------------------------------------------------------------------------------

def test_session_rates_deliver_the_rates_plans_bits(pkg):
    kaldi = lambda pkg, channels=1, norm=0: make(pkg, SMALL, ibs=400000)
    rates = [48000, 8000]
    xs = [synth_utterance(3 * LENGTHS[0] + 1, 421, sr=48000.0).reshape(-1, 1), synth_utterance(LENGTHS[1] // 2 + 7, 422, sr=8000.0).reshape(-1, 1)]
    wants = RD.twins(pkg, xs, rates, make_handle=kaldi)
    assert [w[1].shape for w in wants] == [(71, 8), (17, 8)]
    for u, (conv, rows) in enumerate(wants):
        check(rows, SMALL.oracle(conv[:, 0]), "rates twin, stream %d at %d Hz" % (u, rates[u]))
    m = kaldi(pkg)
    m.sessions_set_rates(rates)
    m.sessions_create(2, 4800)
    fleet = RD.Fleet(pkg, m, seed=5)
    for sid, (x, rate) in enumerate(zip(xs, rates)):
        m.sessions_select_rate(sid, sid)
        Wh = RD.shape(pkg, rate)[2]
        RD.feed(fleet, sid, sid, rate, x, RD.cut_random(len(x), Wh, rate // 10, 40 + sid), D=0)
        conv, rows = wants[sid]
        assert np.array_equal(fleet.converted(sid), conv), "stream %d: converted samples differ" % sid
        assert same_bits(fleet.delivered(sid), rows), "stream %d: rows differ" % sid
    m.close()
