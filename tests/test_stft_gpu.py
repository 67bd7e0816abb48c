"""STFT log-mel front end (MFX_METHOD_STFT_LOGMEL: k_stft_mel + k_stft_post) on the MI355X against the float64 oracle of
tests/stft_ref.py at the project bar (conftest.assert_close: 1e-4 of scale, 1e-5 rel-L2).

A float32 restatement of the pipeline on the CPU stays below 2e-6 of scale in WHISPER mode on the inputs used here, so the bar
leaves about 50x room for the chain order and the device's log; every test prints its worst figure.
"""
import os
import struct
import subprocess

import numpy as np
import pytest

import stft_ref
import xform_ref
from conftest import GOLDEN, synth_utterance
from stft_drive import MATRIX, check, hard_inputs, layout, run_batch, same_bits

pytestmark = pytest.mark.gpu

R = 64   # frames per block of k_stft_mel at N = 400, S = 160 (mfx_stft.hip: the largest tile whose LDS fits)
make, oracle = MATRIX.make, MATRIX.oracle       # (N, S, M, sr default to (400, 160, 80, 16 kHz))


# ---- 1. ragged batch ------------------------------------------------------------------------------------------------

# 0 frames: 0, 200 samples; then 201 (1 frame), 319 (1), 320 (2), 2559 (15), 2719 (16); 15 / 16 / 17 frames: a 16-row group
# edge; R - 1 / R / R + 1 frames: a block edge; 145 frames: three blocks
RAGGED = [201, 0, 200, 319, 320, 2559, 2560 + 159, 2400 + 7, 2560, 2720 + 1, (R - 1) * 160 + 3, R * 160, (R + 1) * 160 + 80, 145 * 160 + 77]


@pytest.fixture(scope="module")
def ragged(pkg, a0001):
    utts = [synth_utterance(n, 70 + i) for i, n in enumerate(RAGGED)] + [a0001.copy()]
    m = make(pkg)
    got = run_batch(m, utts)       # (utterance 0 has 201 samples: 1, 2 and 3 start at an odd sample)
    m.close()
    return utts, got


@pytest.fixture(scope="module")
def ragged_want(pkg, ragged):
    return [oracle(pkg, u) for u in ragged[0]]


def test_ragged_batch_against_oracle(pkg, ragged, ragged_want):
    utts, got = ragged
    worst = 0.0
    for i, (u, g, want) in enumerate(zip(utts, got, ragged_want)):
        assert want.shape == (stft_ref.frame_count(u.size, 400, 160), 80)
        worst = max(worst, check(g, want, "utt %d (%d samples, %d frames)" % (i, u.size, want.shape[0])))
    print("ragged batch: worst max err / scale %.3g" % worst)


def test_ragged_batch_rows_do_not_depend_on_the_batch(pkg, ragged):
    utts, got = ragged
    m = make(pkg)
    for i, u in enumerate(utts):
        alone = run_batch(m, [u])[0]
        assert same_bits(alone, got[i]), "utt %d alone differs from its rows in the batch" % i
    shifted = run_batch(m, utts[3:8], first=1)
    for i in range(3, 8):
        assert same_bits(shifted[i - 3], got[i]), "utt %d at another offset" % i
    again = run_batch(m, utts)
    for i in range(len(utts)):
        assert same_bits(again[i], got[i]), "second run differs, utt %d" % i
    m.close()


def test_ragged_batch_device_entry_equals_host_entry(pkg, ragged):
    import torch
    utts, got = ragged
    offs, lens, pcm_h = layout(utts)
    m = make(pkg)
    rows, total = m.batch_plan(offs, lens)
    dev = torch.device("cuda", 0)
    pcm = torch.from_numpy(pcm_h).to(dev)
    for lead in (32, 33):      # (33: the output at an odd word of the allocation)
        big = torch.full((lead + total * 80 + 64,), float("nan"), dtype=torch.float32, device=dev)
        torch.cuda.synchronize()
        m.batch_run_device(pcm.data_ptr(), pcm_h.size, big.data_ptr() + 4 * lead)
        m.synchronize()
        b = big.cpu().numpy()
        assert np.isnan(b[:lead]).all() and np.isnan(b[lead + total * 80:]).all(), "guard words written (lead %d)" % lead
        out = b[lead:lead + total * 80].reshape(total, 80)
        assert np.isfinite(out).all()
        for i in range(len(utts)):
            assert same_bits(out[rows[i]:rows[i] + got[i].shape[0]], got[i]), (lead, i)
    m.close()


# ---- 2. shape matrix ------------------------------------------------------------------------------------------------

SHAPES = [(400, 160, 128, 16000.0), (64, 16, 8, 16000.0), (64, 48, 20, 16000.0), (512, 128, 80, 16000.0), (510, 170, 40, 16000.0),
          (32, 32, 1, 16000.0), (200, 80, 40, 8000.0),
          # 64 frames per block would overshoot the LDS by 16 bytes: 32-frame blocks, the second one with a second pass over the taps
          (396, 336, 8, 16000.0), (480, 292, 20, 16000.0), (512, 512, 128, 16000.0)]


@pytest.mark.parametrize("N,S,M,sr", SHAPES)
def test_shape_matrix(pkg, N, S, M, sr):
    utts = [synth_utterance(int(1.3 * sr), 11, sr=sr), synth_utterance(int(1.3 * sr) // 3 + 1, 12, sr=sr)]
    m = make(pkg, N, S, M, sr)
    got = run_batch(m, utts)
    m.close()
    for i, u in enumerate(utts):
        check(got[i], oracle(pkg, u, N, S, M, sr), "N %d S %d M %d sr %g utt %d" % (N, S, M, sr, i))


# ---- 3. post modes --------------------------------------------------------------------------------------------------

def test_post_modes(pkg):
    utts = [synth_utterance(20800, 21), synth_utterance(4000, 22)]
    rows = {}
    for post in (pkg.LOGMEL_WHISPER, pkg.LOGMEL_LOG10, pkg.LOGMEL_LN):
        m = make(pkg, post=post)
        rows[post] = run_batch(m, utts)
        m.close()
        for i, u in enumerate(utts):
            check(rows[post][i], oracle(pkg, u, post=post), "post %d utt %d" % (post, i))
    eps = 2.0 ** -23
    for i in range(len(utts)):
        l10, ln, wh = rows[1][i], rows[2][i], rows[0][i]
        # two logs of the same float32 value, each good to 2 ulp, and the rounding of the comparison's own product
        d = np.abs(l10.astype(np.float64) * np.log(10.0) - ln.astype(np.float64))
        assert (d <= 4.5 * eps * np.abs(ln.astype(np.float64)) + 1e-7).all(), d.max()
        mx = l10.max()
        want = (np.maximum(l10, mx - np.float32(8.0)) + np.float32(4.0)) * np.float32(0.25)
        ulp = np.abs(want.view(np.int32).astype(np.int64) - wh.view(np.int32).astype(np.int64))
        assert ulp.max() <= 2, ulp.max()


# ---- 4. hard inputs -------------------------------------------------------------------------------------------------

def test_hard_inputs(pkg):
    sig = hard_inputs()
    names = list(sig)
    m = make(pkg)
    got = run_batch(m, [sig[k] for k in names])
    m.close()
    for k, g in zip(names, got):
        check(g, oracle(pkg, sig[k]), k)
    assert (got[names.index("silence")] == np.float32(-1.5)).all()
    ends = got[names.index("impulses at both ends")]
    assert ends[0].max() > ends[5].max() and ends[-1].max() > ends[5].max()   # both reflections carry energy


def test_clamp_scope(pkg):
    loud = synth_utterance(8000, 41)
    quiet = (synth_utterance(8000, 42).astype(np.int32) // 256).astype(np.int16)
    m = make(pkg)
    both = run_batch(m, [loud, quiet])
    alone = run_batch(m, [quiet])[0]
    m.close()
    assert same_bits(both[1], alone)
    check(both[0], oracle(pkg, loud), "loud")
    check(both[1], oracle(pkg, quiet), "quiet")
    assert both[1].max() < both[0].max() - 0.3


# ---- 5. composition -------------------------------------------------------------------------------------------------

def test_rates_plan(pkg):
    a = synth_utterance(30011, 51, sr=44100.0)
    b = synth_utterance(9001, 52)
    offs, lens, pcm = layout([a, b])
    m = make(pkg)
    rows, total = m.batch_plan_rates(offs, lens, [44100, 16000])
    out = m.batch_run_host(pcm)
    y = m.debug_read(8)
    off2, len2, tot2 = m.batch_resample_layout()
    assert [int(v) for v in len2] == [pkg.MfccHip.host_resampled_length(30011, 44100, 16000), 9001]
    assert total == sum(stft_ref.frame_count(int(n), 400, 160) for n in len2)
    m2 = make(pkg)
    rows2, total2 = m2.batch_plan(off2, len2)
    out2 = m2.batch_run_host(np.concatenate([y, np.zeros(2, np.int16)]))
    assert total2 == total and np.array_equal(rows, rows2) and same_bits(out, out2)
    check(out[rows[1]:], oracle(pkg, b), "pass-through utterance")
    m.close()
    m2.close()


def test_transform_vad_alphas(pkg):
    utts = [synth_utterance(5000, 61), synth_utterance(321, 62), synth_utterance(100, 63)]
    offs, lens, pcm = layout(utts)
    m = make(pkg, M=8)
    rows, total = m.batch_plan(offs, lens)
    y = m.batch_run_host(pcm)
    frames = [m.batch_frames(int(n)) for n in lens]
    rng = np.random.default_rng(9)
    A = rng.standard_normal((4, 24)).astype(np.float32)
    b = rng.standard_normal(4).astype(np.float32)
    m.batch_set_transform(A, b, left=1, right=1)
    assert m.batch_output_width() == 4
    got = m.batch_run_host(pcm)
    xform_ref.assert_xform_consistent(got, y, rows, frames, A, b, 1, 1, what="stft transform")
    m.batch_set_transform(None)
    m.batch_set_vad(mode=pkg.VAD_FLAGS)
    assert same_bits(m.batch_run_host(pcm), y)
    flags, voiced, thr, tv = m.batch_vad_read()
    assert flags.size == total and voiced.sum() == tv
    m.batch_clear_vad()
    with pytest.raises(pkg.MfxError) as e:
        m.batch_set_alphas(np.ones(3, np.float32))
    assert e.value.status == -5
    m.set_alpha(1.2)        # accepted, no effect
    assert same_bits(m.batch_run_host(pcm), y)
    m.close()


def test_overlap(pkg):
    import torch
    dev = torch.device("cuda", 0)
    batches = [[synth_utterance(3000 + 500 * k + 7 * i, 80 + 3 * k + i) for i in range(3)] for k in range(3)]
    outs = {}
    for ov in (False, True):
        m = make(pkg)
        m.batch_overlap(ov)
        res = []
        for utts in batches:
            offs, lens, pcm_h = layout(utts)
            rows, total = m.batch_plan(offs, lens)
            pcm = torch.from_numpy(pcm_h).to(dev)
            out = torch.full((total, 80), float("nan"), dtype=torch.float32, device=dev)
            torch.cuda.synchronize()
            m.batch_run_device(pcm.data_ptr(), pcm_h.size, out.data_ptr())
            res.append((pcm, out))
        m.synchronize()
        outs[ov] = [o.cpu().numpy() for _, o in res]
        m.close()
    for a, b in zip(outs[False], outs[True]):
        assert np.isfinite(a).all() and same_bits(a, b)


def test_streaming_and_session_entries_refused(pkg):
    m = make(pkg)
    u = synth_utterance(4000, 91)
    for call in (lambda: m.set_input(u), m.flush, m.apply, lambda: m.get_output_data(1), lambda: m.apply_alphas([1.0]),
                 lambda: m.get_output_data_alpha(0, 1), lambda: m.sessions_create(2, 1600)):
        with pytest.raises(pkg.MfxError) as e:
            call()
        assert e.value.status == -8 and "batch" in str(e.value)
    check(run_batch(m, [u])[0], oracle(pkg, u), "after the refusals")
    m.close()


def test_mixed_handles(pkg):
    utts = [synth_utterance(6000, 95), synth_utterance(2001, 96)]
    kinds = {"mfcc": dict(ceps=13, method=pkg.METHOD_MFCC), "plp": dict(ceps=12, method=pkg.METHOD_PLP),
             "traps": dict(ceps=0, method=pkg.METHOD_TRAPS)}

    def other(kind):
        k = kinds[kind]
        h = pkg.MfccHip(200000, 400, 160, 15, 16000.0, 64.0, 8000.0, k["ceps"], False, 22.0, device=0, bug_compat=False, method=k["method"])
        h.set_window(pkg.reference_window(400))
        return h

    alone = {}
    for kind in kinds:
        h = other(kind)
        alone[kind] = run_batch(h, utts)
        h.close()
    s = make(pkg)
    want = run_batch(s, utts)
    s.close()
    before = {k: other(k) for k in kinds}
    s = make(pkg)
    after = {k: other(k) for k in kinds}
    for rnd in range(2):
        got = run_batch(s, utts)
        for i in range(len(utts)):
            assert same_bits(got[i], want[i]), ("stft", rnd, i)
        for hs in (before, after):
            for kind, h in hs.items():
                g = run_batch(h, utts)
                for i in range(len(utts)):
                    assert same_bits(g[i], alone[kind][i]), (kind, rnd, i)
    for h in list(before.values()) + list(after.values()) + [s]:
        h.close()


# ---- 6. driver ------------------------------------------------------------------------------------------------------

def test_driver(pkg, orc, tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "asr-featext-opencl_amd", "host", "afet_hip")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", os.path.dirname(exe)])
    riff = os.path.join(GOLDEN, "sample1_riff.wav")
    pcm, sr = orc.read_wav_pcm16(riff)
    pcm = pcm[:, 0].copy()
    N, S = int(sr * 25e-3), int(sr * 10e-3)
    t, h = tmp_path / "r.txt", tmp_path / "r.htk"
    opts = ["--method", "LOGMEL", "--banks", "80"]
    want = oracle(pkg, pcm, N, S, 80, float(sr))
    subprocess.check_call([exe] + opts + [riff, str(t)])
    subprocess.check_call([exe] + opts + ["--htk", riff, str(h)])
    rows = np.array([[float(v) for v in line.strip().strip("|").split("|")] for line in open(t)])
    assert rows.shape == (want.shape[0], 1 + 80)
    check(rows[:, 1:], want, "afet_hip --method LOGMEL (text)")

    def read_htk(path):
        raw = open(path, "rb").read()
        n, period, size, kind = struct.unpack(">iihh", raw[:12])
        assert (n, size) == (want.shape[0], 4 * 80)
        return np.frombuffer(raw[12:], dtype=">f4").reshape(n, 80).astype(np.float32)

    htk = read_htk(h)
    check(htk, want, "afet_hip --method LOGMEL (htk)")
    # --logmel-post log10: the rows ahead of the clamp and the map (the clamp is what makes a real recording's silent bands
    # comparable to a float64 reference, so these are held against the default mode's rows, not the oracle)
    subprocess.check_call([exe] + opts + ["--logmel-post", "log10", "--htk", riff, str(h)])
    l10 = read_htk(h)
    mapped = (np.maximum(l10, l10.max() - np.float32(8.0)) + np.float32(4.0)) * np.float32(0.25)
    assert np.abs(mapped.view(np.int32).astype(np.int64) - htk.view(np.int32).astype(np.int64)).max() <= 2
    r = subprocess.run([exe, "--method", "LOGMEL", "--banks", "80", "--batch-mb", "0", riff, str(t)], stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE)
    assert r.returncode == 2
