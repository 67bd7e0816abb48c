"""The FFT form of the STFT log-mel front end (MFX_METHOD_STFT_LOGMEL at N = 1024 / 2048: k_stft_fft_mel + k_stft_post) on the
MI355X against the float64 oracle of tests/stft_fft_ref.py at the project bar (conftest.assert_close: 1e-4 of scale, 1e-5
rel-L2), and the bit contract of the method: rows do not depend on the batch, the offset, the run, the entry or the placement.

A float32 restatement of the pipeline on the CPU (torch.fft.rfft in float32, float32 mel product and log) stays below 5.6e-7 of
scale and 1.8e-7 relative L2 on the shapes, windows and modes used here, so the bar leaves more than 50x room; every test prints
its worst figure.
"""
import os
import struct
import subprocess

import numpy as np
import pytest

import stft_edge as SE
import stft_fft_ref as FR
import stft_ref
import xform_ref
from conftest import GOLDEN, synth_utterance
from stft_drive import FFT, check, hard_inputs, layout, run_batch, same_bits

pytestmark = pytest.mark.gpu

N0, S0, M0, SR0 = FFT.shape             # (1024, 256, 80, 22050 Hz): the shape most tests run at
make, oracle, block_rows = FFT.make, FFT.oracle, FFT.block_rows


# ---- 1. ragged batch ------------------------------------------------------------------------------------------------

def ragged_lengths(R):
    """0 and 512 samples: no frame; 513: two; 767 / 768: two / three; k 256 + r around the block edges; 2 R + 1: three blocks."""
    return [513, 0, 512, 767, 768, (R - 1) * 256 + 3, R * 256, (R + 1) * 256 + 80, (2 * R + 1) * 256 + 77]


@pytest.fixture(scope="module")
def ragged(pkg, a0001):
    R = block_rows(pkg, N0, S0, M0)
    utts = [synth_utterance(n, 170 + i, sr=SR0) for i, n in enumerate(ragged_lengths(R))] + [a0001.copy()]
    m = make(pkg)
    got = run_batch(m, utts)       # (utterance 0 has 513 samples: 1, 2 and 3 start at an odd sample)
    m.close()
    return utts, got


@pytest.fixture(scope="module")
def ragged_want(pkg, ragged):
    return [oracle(pkg, u) for u in ragged[0]]


def test_ragged_batch_against_oracle(pkg, ragged, ragged_want):
    utts, got = ragged
    worst = 0.0
    assert [g.shape[0] for g in got[:5]] == [2, 0, 0, 2, 3]
    for i, (u, g, want) in enumerate(zip(utts, got, ragged_want)):
        assert want.shape == (stft_ref.frame_count(u.size, N0, S0), M0)
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


# ---- 2. shape matrix, post modes ------------------------------------------------------------------------------------------

def shape_utterances(N, S, sr):
    """Two utterances of a shape: 45 frames and a remainder -- every tile of the list sees a full and a cut block --, and a short
    one that ends inside its first block."""
    return [synth_utterance(N + 44 * S + S // 2, 11, sr=sr), synth_utterance(N // 2 + 2 * S + 1, 12, sr=sr)]


@pytest.mark.parametrize("shape", FR.SHAPES, ids=[FR.shape_id(s) for s in FR.SHAPES])
def test_shape_matrix(pkg, shape):
    N, S, M, sr = shape
    utts = shape_utterances(N, S, sr)
    m = make(pkg, N, S, M, sr)
    got = run_batch(m, utts)
    m.close()
    for i, u in enumerate(utts):
        check(got[i], oracle(pkg, u, N, S, M, sr), "N %d S %d M %d sr %g utt %d" % (N, S, M, sr, i))


def test_post_modes(pkg):
    utts = [synth_utterance(20800, 21, sr=SR0), synth_utterance(4000, 22, sr=SR0)]
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


# ---- 3. windows -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", FR.SHAPES[:3], ids=[FR.shape_id(s) for s in FR.SHAPES[:3]])
def test_windows(pkg, shape):
    """rect, ramp (what a reversed or conjugated tap order cannot pass), ends, and the short Hann centred in N."""
    N, S, M, sr = shape
    utts = shape_utterances(N, S, sr)
    m = make(pkg, N, S, M, sr)
    for name, w in FR.windows(N).items():
        if name == "hann":
            continue
        m.set_window(w)
        got = run_batch(m, utts)
        for i, u in enumerate(utts):
            check(got[i], oracle(pkg, u, N, S, M, sr, window=w), "%s window %s utt %d" % (FR.shape_id(shape), name, i))
    m.close()


# ---- 4. one-hot probes ------------------------------------------------------------------------------------------------

PROBE_BAR = 1e-3        # a tenth of stft_edge.PROBE_SEPARATION; 30 x the worst-case float32 bound (26 eps on P, 1025 eps on the
                        # longest mel chain: 3e-5 in log10)


@pytest.mark.parametrize("shape", FR.PROBE_SHAPES, ids=[FR.shape_id(s) for s in FR.PROBE_SHAPES])
def test_tap_probes(pkg, shape):
    """Under a one-hot window at tap j every bin's power is x[i]^2 of the ONE sample the frame rule names, so every row is
    2 log10(|x[i]| / 32768) + log10(sum_k Wm[m][k]); neighbouring samples of the probe signal differ by 0.0162 there."""
    N, S, M, sr = shape
    R = block_rows(pkg, N, S, M)
    lengths = SE.probe_lengths(N, S, R)
    utts = [SE.probe_signal(n) for n in lengths]
    taps = SE.probe_taps(N)
    for n in lengths:
        assert SE.probe_separation(n, N, S, taps) >= SE.PROBE_SEPARATION, n
    table = stft_ref.mel_table(M, N, sr, 0.0, sr / 2)[0].astype(np.float64)
    rowsum = np.log10(table.sum(axis=1))
    # No entry reaches the 1e-10 floor: |x| >= 600, and a unit-area Slaney row sums to about N / sr (10^-0.89 at 2048 / 16 kHz,
    # 10^-1.2 at 1024 / 16 kHz, 10^-1.33 at 1024 / 22.05 kHz and 2048 / 44.1 kHz; the least row of these shapes: 10^-1.376)
    assert np.isfinite(rowsum).all() and rowsum.min() >= -1.4
    assert 2.0 * np.log10(600.0 / 32768.0) + rowsum.min() > -5.0
    m = make(pkg, N, S, M, sr, window=SE.onehot(N, 0), post=pkg.LOGMEL_LOG10)
    worst, misses = 0.0, []
    for j in taps:
        m.set_window(SE.onehot(N, j))
        got = run_batch(m, utts)
        for u, g in zip(utts, got):
            T = stft_ref.frame_count(u.size, N, S)
            assert g.shape == (T, M)
            if T == 0:
                continue
            idx = stft_ref.frame_index(u.size, N, S)[:, j]
            want = 2.0 * np.log10(np.abs(u[idx].astype(np.float64)) / 32768.0)[:, None] + rowsum[None, :]
            d = np.abs(g.astype(np.float64) - want)
            worst = max(worst, d.max())
            for t in np.nonzero(d.max(axis=1) > PROBE_BAR)[0]:
                misses.append("tap %d, %d samples, frame %d: |d L| %.3g; the row reads sample = %d (mod 193), the frame rule sample %d "
                              "= %d (mod 193)" % (j, u.size, t, d[t].max(), SE.probe_decode(float(g[t, 0]), rowsum[0]), idx[t],
                                                  idx[t] % SE.PROBE_PERIOD))
    m.close()
    if S == N:      # (the two shortest lengths, N / 2 + 1 and N / 2 + 2 samples, have no frame: n div S == 0)
        assert stft_ref.frame_count(lengths[0], N, S) == stft_ref.frame_count(lengths[1], N, S) == 0
    print("\n%s one-hot probes: worst |d L| %.3g / bar %.3g" % (FR.shape_id(shape), worst, PROBE_BAR))
    assert not misses, "%d rows miss the one-hot bar:\n%s" % (len(misses), "\n".join(misses[:20]))


# ---- 5. hard inputs ---------------------------------------------------------------------------------------------------

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
    loud = synth_utterance(8000, 41, sr=SR0)
    quiet = (synth_utterance(8000, 42, sr=SR0).astype(np.int32) // 256).astype(np.int16)
    m = make(pkg)
    both = run_batch(m, [loud, quiet])
    alone = run_batch(m, [quiet])[0]
    m.close()
    assert same_bits(both[1], alone)
    check(both[0], oracle(pkg, loud), "loud")
    check(both[1], oracle(pkg, quiet), "quiet")
    assert both[1].max() < both[0].max() - 0.3


# ---- 6. the maximum of k_stft_post over more than 256 blocks ----------------------------------------------------------------

def test_whisper_maximum_beyond_256_blocks(pkg):
    """256 R + R + 1 frames: 258 blocks, the second trip of k_stft_post's stride of 256 slots; the loudest second lies in the
    last block, and everything in front of it sits on the clamp it sets."""
    R = block_rows(pkg, N0, S0, M0)
    T = 256 * R + R + 1
    n = T * S0 + 5
    long = (synth_utterance(n, 61, sr=SR0).astype(np.int32) // 4096).astype(np.int16)       # about +-3 LSB
    tail = synth_utterance(2 * S0, 62, sr=SR0)
    long[n - tail.size:] = tail                                                            # inside the last block
    short = synth_utterance(5 * S0 + 7, 63, sr=SR0)
    m = make(pkg)
    both = run_batch(m, [long, short])
    alone = run_batch(m, [short])[0]
    m.close()
    assert both[0].shape[0] == T and -(-T // R) == 258
    l10 = oracle(pkg, long, post=stft_ref.LOG10)
    assert l10.max() == l10[257 * R:].max() and l10[:256 * R].max() < l10.max() - 1.0     # the level comes from the last block
    check(both[0], oracle(pkg, long), "%d frames in %d blocks" % (T, -(-T // R)))
    check(both[1], oracle(pkg, short), "the short neighbour")
    assert same_bits(both[1], alone), "the short utterance's rows depend on its neighbour"


# ---- 7. composition -------------------------------------------------------------------------------------------------

def test_rates_plan(pkg):
    a = synth_utterance(30011, 51, sr=44100.0)
    b = synth_utterance(9001, 52, sr=SR0)
    offs, lens, pcm = layout([a, b])
    m = make(pkg)
    rows, total = m.batch_plan_rates(offs, lens, [44100, 22050])
    out = m.batch_run_host(pcm)
    y = m.debug_read(8)
    off2, len2, tot2 = m.batch_resample_layout()
    assert [int(v) for v in len2] == [pkg.MfccHip.host_resampled_length(30011, 44100, 22050), 9001]
    assert total == sum(stft_ref.frame_count(int(n), N0, S0) for n in len2)
    m2 = make(pkg)
    rows2, total2 = m2.batch_plan(off2, len2)
    out2 = m2.batch_run_host(np.concatenate([y, np.zeros(2, np.int16)]))
    assert total2 == total and np.array_equal(rows, rows2) and same_bits(out, out2)
    check(out[rows[1]:], oracle(pkg, b), "pass-through utterance")
    m.close()
    m2.close()


def test_transform_vad_alphas(pkg):
    utts = [synth_utterance(9000, 61, sr=SR0), synth_utterance(769, 62, sr=SR0), synth_utterance(300, 63, sr=SR0)]
    offs, lens, pcm = layout(utts)
    m = make(pkg, M=8)
    rows, total = m.batch_plan(offs, lens)
    y = m.batch_run_host(pcm)
    frames = [m.batch_frames(int(n)) for n in lens]
    assert frames == [35, 3, 0]
    rng = np.random.default_rng(9)
    A = rng.standard_normal((4, 24)).astype(np.float32)
    b = rng.standard_normal(4).astype(np.float32)
    m.batch_set_transform(A, b, left=1, right=1)
    assert m.batch_output_width() == 4
    got = m.batch_run_host(pcm)
    xform_ref.assert_xform_consistent(got, y, rows, frames, A, b, 1, 1, what="stft fft transform")
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
    batches = [[synth_utterance(5000 + 900 * k + 7 * i, 80 + 3 * k + i, sr=SR0) for i in range(3)] for k in range(3)]
    outs = {}
    for ov in (False, True):
        m = make(pkg)
        m.batch_overlap(ov)
        res = []
        for utts in batches:
            offs, lens, pcm_h = layout(utts)
            rows, total = m.batch_plan(offs, lens)
            pcm = torch.from_numpy(pcm_h).to(dev)
            out = torch.full((total, M0), float("nan"), dtype=torch.float32, device=dev)
            torch.cuda.synchronize()
            m.batch_run_device(pcm.data_ptr(), pcm_h.size, out.data_ptr())
            res.append((pcm, out))
        m.synchronize()
        outs[ov] = [o.cpu().numpy() for _, o in res]
        m.close()
    for a, b in zip(outs[False], outs[True]):
        assert np.isfinite(a).all() and same_bits(a, b)


def test_host_entry_slices_equal_one_device_run(pkg):
    """The smallest batch that takes the sliced path of mfx_batch_run_host -- 8 utterances (two slices), 32 MB of PCM, pinned
    buffers: every slice runs the front end over its own range of chunks.  Against one device run over the whole batch."""
    import ctypes as C
    import torch
    L = pkg.load_library()
    L.mfx_alloc_pinned.restype, L.mfx_alloc_pinned.argtypes = C.c_void_p, [C.c_size_t]
    L.mfx_free_pinned.restype, L.mfx_free_pinned.argtypes = None, [C.c_void_p]
    rng = np.random.default_rng(23)
    lens = [int(v) for v in rng.integers(2100000, 2110000, size=8)]
    offs, pos = [], 0
    for n in lens:
        offs.append(pos)
        pos += n + (n & 1)
    base = synth_utterance(1 << 16, 77, sr=SR0)
    pcm_h = np.tile(base, pos // base.size + 1)[:pos].copy()
    assert pcm_h.nbytes >= 32 << 20
    m = make(pkg, ibs=4000000)
    rows, total = m.batch_plan(offs, lens)
    dev = torch.device("cuda", 0)
    pcm = torch.from_numpy(pcm_h).to(dev)
    out = torch.full((total, M0), float("nan"), dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    m.batch_run_device(pcm.data_ptr(), pcm_h.size, out.data_ptr())
    m.synchronize()
    want = out.cpu().numpy()
    del pcm, out
    p_in, p_out = L.mfx_alloc_pinned(pcm_h.nbytes), L.mfx_alloc_pinned(want.nbytes)
    assert p_in and p_out
    try:
        C.memmove(p_in, pcm_h.ctypes.data, pcm_h.nbytes)
        rc = L.mfx_batch_run_host(m._h, C.cast(p_in, C.POINTER(C.c_int16)), pcm_h.size, C.cast(p_out, C.POINTER(C.c_float)))
        assert rc == 0
        got = np.ctypeslib.as_array(C.cast(p_out, C.POINTER(C.c_float)), shape=(total, M0)).copy()
    finally:
        m.synchronize()
        L.mfx_free_pinned(p_in), L.mfx_free_pinned(p_out)
    m.close()
    assert np.isfinite(want).all() and same_bits(got, want)
    T = 40      # the first frames of the last utterance (the last slice's range) against the oracle, in LOG10 terms of the clamp:
    u = pcm_h[offs[7]:offs[7] + lens[7]]
    whole = oracle(pkg, u[:(T + 8) * S0], post=stft_ref.LOG10)[:T]          # (frames that read no sample beyond the cut)
    r0 = int(rows[7])
    mx = (float(want[r0:r0 + lens[7] // S0].max()) * 4.0 - 4.0)             # the utterance's largest log10 value, from its rows
    check(want[r0:r0 + T], (np.maximum(whole, mx - 8.0) + 4.0) / 4.0, "first %d frames of utterance 7" % T)


# ---- 8. refusals and neighbours -----------------------------------------------------------------------------------------

def test_streaming_and_session_entries_refused(pkg):
    for post in (pkg.LOGMEL_WHISPER, pkg.LOGMEL_LOG10):      # (LOG10: what the session entries serve up to N = 512)
        m = make(pkg, post=post)
        u = synth_utterance(4000, 91, sr=SR0)
        for call in (lambda: m.set_input(u), m.flush, m.apply, lambda: m.get_output_data(1), lambda: m.apply_alphas([1.0]),
                     lambda: m.get_output_data_alpha(0, 1), lambda: m.sessions_create(2, 1600)):
            with pytest.raises(pkg.MfxError) as e:
                call()
            assert e.value.status == -8 and "batch" in str(e.value)
        check(run_batch(m, [u])[0], oracle(pkg, u, post=post), "after the refusals (post %d)" % post)
        m.close()


def test_mixed_handles(pkg):
    utts = [synth_utterance(6000, 95), synth_utterance(2001, 96)]

    def other(kind):
        if kind == "stft400":
            h = pkg.MfccHip(200000, 400, 160, 80, 16000.0, 0.0, 8000.0, 0, False, 22.0, device=0, bug_compat=False,
                            method=pkg.METHOD_STFT_LOGMEL)
            h.set_window(pkg.periodic_hann(400))
        else:
            h = pkg.MfccHip(200000, 400, 160, 15, 16000.0, 64.0, 8000.0, 13, False, 22.0, device=0, bug_compat=False, method=pkg.METHOD_MFCC)
            h.set_window(pkg.reference_window(400))
        return h

    kinds = ("stft400", "mfcc")
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
            assert same_bits(got[i], want[i]), ("stft fft", rnd, i)
        for hs in (before, after):
            for kind, h in hs.items():
                g = run_batch(h, utts)
                for i in range(len(utts)):
                    assert same_bits(g[i], alone[kind][i]), (kind, rnd, i)
    for h in list(before.values()) + list(after.values()) + [s]:
        h.close()


# ---- 9. driver ------------------------------------------------------------------------------------------------------

def test_driver(pkg, orc, tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "asr-featext-opencl_amd", "host", "afet_hip")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", os.path.dirname(exe)])
    riff = os.path.join(GOLDEN, "sample1_riff.wav")
    pcm, sr = orc.read_wav_pcm16(riff)
    pcm = pcm[:, 0].copy()
    L, S = int(sr * 25e-3), int(sr * 10e-3)
    assert L <= 1024
    t, h = tmp_path / "r.txt", tmp_path / "r.htk"
    opts = ["--method", "LOGMEL", "--logmel-nfft", "1024", "--banks", "80"]
    want = oracle(pkg, pcm, 1024, S, 80, float(sr), window=FR.padded_hann(L, 1024))
    subprocess.check_call([exe] + opts + [riff, str(t)])
    subprocess.check_call([exe] + opts + ["--htk", riff, str(h)])
    rows = np.array([[float(v) for v in line.strip().strip("|").split("|")] for line in open(t)])
    assert rows.shape == (want.shape[0], 1 + 80)
    check(rows[:, 1:], want, "afet_hip --method LOGMEL --logmel-nfft 1024 (text)")
    raw = open(h, "rb").read()
    n, period, size, kind = struct.unpack(">iihh", raw[:12])
    assert (n, size) == (want.shape[0], 4 * 80)
    check(np.frombuffer(raw[12:], dtype=">f4").reshape(n, 80).astype(np.float32), want, "afet_hip --method LOGMEL --logmel-nfft 1024 (htk)")
    for bad in (["--logmel-nfft", "1000"], ["--logmel-nfft", "512"], ["--logmel-nfft", "1024", "--window-size", "200"]):
        r = subprocess.run([exe, "--method", "LOGMEL", "--banks", "80"] + bad + [riff, str(t)], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        assert r.returncode == 2, bad
    r = subprocess.run([exe, "--logmel-nfft", "1024", riff, str(t)], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 2        # (the option goes with --method LOGMEL)
