"""Per-utterance sample-rate conversion in front of the batch entries (mfx_batch_plan_rates; k_resample) on the MI355X.

Four kinds of check, all through the C ABI:
  - exact: an impulse of 16384 returns the one tap it meets, rint(16384 h32[phi][k]), bit for bit (every product is exact
    and every other FMA adds zero);
  - bound: every converted sample of a ragged, mixed-rate batch within B = 0.5 + gamma_P sum |h32 x| of the float64 sum
    from the float32 table the library reports (resample_ref.py: derived, not tuned);
  - bits: each utterance alone, even and odd input offsets, a second run and the device entry deliver the same samples;
  - rows: a twin handle planned plainly on the converted PCM (mfx_debug_read kind 8) and its layout delivers bit-identical
    rows, whatever else is in force (normaliser, warp-factor list, transform, overlap, TRAPS, 2048-point stereo).
Reference window, C2 feature configuration (16 kHz, W = 400, S = 160, 40 mel, 13 cepstra + d + dd) unless stated."""
import numpy as np
import pytest

import resample_ref as RR

pytestmark = pytest.mark.gpu

W, S, SR = 400, 160, 16000
PAIRS = [(48000, 16000), (8000, 16000), (44100, 16000), (11025, 16000), (17600, 16000), (16000, 44100)]
ERR_STATE = -8


def make(pkg, sr=SR, channels=1, norm=0, dyn=2, method=None, W_=W, S_=S, fft=0, nb=40, nc=13, **kw):
    m = pkg.MfccHip(400000, W_, S_, nb, float(sr), 64.0, sr / 2.0, nc, False, 22.0, norm, dyn, 3, 3, True, device=0,
                    bug_compat=False, channels=channels, fft_size=fft,
                    method=pkg.METHOD_MFCC if method is None else method, **kw)
    m.set_window(pkg.reference_window(W_))
    return m


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ---- 1. impulse, exact ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("channels", [1, 2])
@pytest.mark.parametrize("pair", PAIRS)
def test_impulse_returns_the_taps_bit_for_bit(pkg, pair, channels):
    r_in, r_out = pair
    h, L, M, P = pkg.mfcc.host_resample_taps(r_in, r_out)
    Wh = P // 2
    n_in = 4 * P + 3 * M
    n_out = RR.out_length(n_in, r_in, r_out)
    m = make(pkg, sr=r_out, channels=channels)
    j = np.arange(n_out, dtype=np.int64)
    n, phi = (j * M) // L, (j * M) % L
    for pos in (0, Wh, n_in // 2, n_in - 1):
        x = np.zeros((n_in + 1, channels), np.int16)      # one spare sample: an odd mono length stays inside the array
        x[pos, channels - 1] = 16384
        m.batch_plan_rates([0], [n_in], [r_in])
        m.batch_run_host(x.reshape(-1))
        y = m.debug_read(8).reshape(-1, channels)
        off, ln, total = m.batch_resample_layout()
        assert ln.tolist() == [n_out] and off.tolist() == [0] and y.shape[0] == total == n_out + (n_out & 1)
        k = pos - (n - Wh + 1)
        hit = (k >= 0) & (k < P)
        want = np.zeros(n_out, np.float64)
        want[hit] = np.rint(16384.0 * h[phi[hit], k[hit]].astype(np.float64))
        assert np.array_equal(y[:n_out, channels - 1], want.astype(np.int16)), (pair, channels, pos)
        assert np.count_nonzero(want) > 0
        if channels == 2:
            assert not y[:, 0].any()                       # the silent channel stays silent
        assert not y[n_out:].any()
    m.close()


# ---- 2. float64 oracle on a ragged, mixed-rate batch ---------------------------------------------------------------------

RATES3 = (48000, 8000, 44100)
_BATCH = {}


def signal(kind, n, rate, seed):
    t = np.arange(n)
    if kind == 0:                                           # full-scale noise
        return np.random.default_rng(900 + seed).integers(-32768, 32768, n).astype(np.int16)
    if kind == 1:                                           # a 997 Hz sine
        return np.rint(30000.0 * np.sin(2 * np.pi * 997.0 * t / rate)).astype(np.int16)
    return np.where((t // 23) % 2 == 0, 32767, -32768).astype(np.int16)   # full-scale square wave: the overshoot saturates


def ragged(pkg, in_rates, out_hz, channels=1, kinds=3):
    """A ragged batch to convert to out_hz (host arithmetic only): per input rate lengths 0, 1, 2, Wh - 1, Wh, 2 Wh + 1, around
    one tile of the kernel, two tiles + 3; three pass-through utterances; every other utterance on an odd input offset; gaps
    between utterances filled with +-32767.  Utterance i carries signal kind i % kinds (kinds = 1: full-scale noise throughout);
    a second channel carries the same kind at another seed.  Returns dict(lens, rates, offs, utts [n][channels] (mono: [n]),
    pcm (flat, interleaved))."""
    lens, rates = [], []
    for r in in_rates:
        h, L, M, P = pkg.mfcc.host_resample_taps(r, out_hz)
        Wh, tile = P // 2, pkg.mfcc.host_resample_tile(r, out_hz, channels=channels)
        edge = -(-tile * M // L)                            # the shortest input that fills one tile
        for n in (0, 1, 2, Wh - 1, Wh, 2 * Wh + 1, edge - 1, edge, edge + 1, 2 * edge + 3):
            lens.append(n), rates.append(r)
    for n in (0, 401, 4096 + 5):                            # pass-through: empty, short, more than one copy tile
        lens.append(n), rates.append(out_hz)
    order = np.random.default_rng(5).permutation(len(lens))
    lens, rates = [lens[i] for i in order], [rates[i] for i in order]
    offs, pos = [], 2
    for i, n in enumerate(lens):
        pos += 1 + (i % 3)
        if (pos & 1) != (i & 1):
            pos += 1                                        # odd utterances on odd offsets
        offs.append(pos)
        pos += n
    pcm = np.repeat(np.where(np.arange(pos + 8) % 2 == 0, 32767, -32767).astype(np.int16)[:, None], channels, 1)
    utts = []
    for i, (o, n, r) in enumerate(zip(offs, lens, rates)):
        x = np.stack([signal(i % kinds, n, r, i + 1000 * c) for c in range(channels)], 1)
        pcm[o:o + n] = x
        utts.append(x[:, 0].copy() if channels == 1 else x)
    return dict(lens=lens, rates=rates, offs=offs, utts=utts, pcm=pcm.reshape(-1))


def batch(pkg):
    """ragged() of RATES3 -> SR, mono, the three signal kinds, and what the library gives for it (computed once, never
    modified)."""
    if _BATCH:
        return _BATCH
    d = ragged(pkg, RATES3, SR)
    lens, rates, offs, pcm, utts = d["lens"], d["rates"], d["offs"], d["pcm"], d["utts"]
    m = make(pkg)
    rows, total = m.batch_plan_rates(offs, lens, rates)
    feats = m.batch_run_host(pcm)
    y = m.debug_read(8)
    lay = m.batch_resample_layout()
    m.close()
    for a in (pcm, y, feats, *utts):
        a.setflags(write=False)
    _BATCH.update(lens=lens, rates=rates, offs=offs, pcm=pcm, utts=utts, rows=rows, total=total, feats=feats, y=y, lay=lay)
    return _BATCH


def test_layout_and_lengths_equal_the_host_builders(pkg):
    d = batch(pkg)
    off, ln, total = d["lay"]
    hoff, hln, htotal = pkg.mfcc.host_resample_layout(d["lens"], d["rates"], SR)
    assert off.tolist() == hoff.tolist() and ln.tolist() == hln.tolist() and total == htotal == d["y"].size
    woff, wln, wtotal = RR.layout(d["lens"], d["rates"], SR)
    assert off.tolist() == woff and ln.tolist() == wln and total == wtotal
    one = make(pkg)
    frames = [one.batch_frames(int(n)) for n in ln]
    one.close()
    assert d["total"] == sum(frames) and d["rows"].tolist() == np.concatenate([[0], np.cumsum(frames)[:-1]]).tolist()


def test_every_sample_is_within_the_bound_of_the_float64_sum(pkg):
    d = batch(pkg)
    off, ln, _ = d["lay"]
    worst, saturated = 0.0, 0
    for u, (x, r) in enumerate(zip(d["utts"], d["rates"])):
        y = d["y"][off[u]:off[u] + ln[u]].astype(np.float64)
        if r == SR:
            assert np.array_equal(d["y"][off[u]:off[u] + ln[u]], x), "pass-through utterance %d" % u
            continue
        h, L, M, P = pkg.mfcc.host_resample_taps(r, SR)
        o, B = RR.convert(x, h, L, M)
        assert o.size == ln[u]
        if o.size == 0:
            continue
        oc = np.clip(o, -32768.0, 32767.0)                  # the clamp is monotone: it cannot increase a distance
        ratio = np.abs(y - oc) / B
        print("utterance %2d  rate %5d  n_in %6d  n_out %6d  worst |y - o| / B = %.4f" % (u, r, x.size, o.size, ratio.max()))
        worst = max(worst, float(ratio.max()))
        saturated += int((np.abs(o) > 32768.0).sum())
        assert (np.abs(y - oc) <= B).all(), "utterance %d (rate %d, %d samples)" % (u, r, x.size)
    print("worst |y - o| / B over the batch: %.4f; samples whose float64 sum is beyond full scale: %d" % (worst, saturated))
    assert saturated > 0                                     # the square wave's overshoot is in the batch


# ---- 3. same bits --------------------------------------------------------------------------------------------------------

def test_each_utterance_alone_even_and_odd_offset(pkg):
    d = batch(pkg)
    off, ln, _ = d["lay"]
    m = make(pkg)
    for u, (x, r) in enumerate(zip(d["utts"], d["rates"])):
        want = d["y"][off[u]:off[u] + ln[u]]
        for o in (0, 1, 7):
            pcm = np.full(o + x.size + 8, -32767, np.int16)
            pcm[o:o + x.size] = x
            m.batch_plan_rates([o], [x.size], [r])
            m.batch_run_host(pcm)
            assert np.array_equal(m.debug_read(8)[:ln[u]], want), "utterance %d at offset %d" % (u, o)
    m.close()


def test_second_run_and_device_entry_give_the_same_bits(pkg):
    import torch
    d = batch(pkg)
    m = make(pkg)
    m.batch_plan_rates(d["offs"], d["lens"], d["rates"])
    for _ in range(2):
        assert same_bits(m.batch_run_host(d["pcm"]), d["feats"])
        assert np.array_equal(m.debug_read(8), d["y"])
    dev = torch.device("cuda:0")
    pcm = torch.from_numpy(d["pcm"].copy()).to(dev)
    out = torch.full((d["total"], 39), float("nan"), dtype=torch.float32, device=dev)
    m.batch_run_device(pcm.data_ptr(), pcm.numel(), out.data_ptr())
    m.synchronize()
    assert same_bits(out.cpu().numpy(), d["feats"]) and np.array_equal(m.debug_read(8), d["y"])
    with pytest.raises(pkg.MfxError):                        # the bounds check refers to the input array
        m.batch_run_device(pcm.data_ptr(), pcm.numel() - 64, out.data_ptr())
    m.close()


# ---- 4. rows: a twin planned plainly on the converted PCM ------------------------------------------------------------------

def rows_pair(pkg, d, setup=None, **kw):
    """(rows of the rates plan, rows of a twin planned plainly on the converted PCM and its layout)"""
    m, t = make(pkg, **kw), make(pkg, **kw)
    rows, total = m.batch_plan_rates(d["offs"], d["lens"], d["rates"])
    if setup:
        setup(m)
    got = m.batch_run_host(d["pcm"])
    y = m.debug_read(8)
    off, ln, tot = m.batch_resample_layout()
    trows, ttotal = t.batch_plan(off, ln)
    assert trows.tolist() == rows.tolist() and ttotal == total
    assert [m.batch_frames(int(n)) for n in ln] == np.diff(np.append(rows, total)).tolist()
    if setup:
        setup(t)
    want = t.batch_run_host(np.concatenate([y, np.zeros(8, np.int16)]))
    m.close(), t.close()
    return got, want


def test_rows_equal_a_twin_on_the_converted_pcm(pkg):
    d = batch(pkg)
    got, want = rows_pair(pkg, d)
    assert got.shape == (d["total"], 39) and same_bits(got, want) and same_bits(got, d["feats"])


def test_rows_with_normaliser(pkg):
    got, want = rows_pair(pkg, batch(pkg), norm=2, dyn=2)
    keep = np.isfinite(want)                                 # (one-frame utterances under CVN are 0 x inf in both)
    assert keep.any() and same_bits(np.where(keep, got, 0), np.where(keep, want, 0)) and np.array_equal(np.isnan(got), np.isnan(want))


def test_rows_with_alpha_list(pkg):
    d = batch(pkg)
    alphas = (0.9 + 0.02 * (np.arange(len(d["lens"])) % 7)).astype(np.float32)
    got, want = rows_pair(pkg, d, setup=lambda h: h.batch_set_alphas(alphas))
    assert same_bits(got, want)


def test_rows_with_transform(pkg):
    d = batch(pkg)
    A = (np.random.default_rng(3).standard_normal((24, 5 * 39)) / 14).astype(np.float32)
    got, want = rows_pair(pkg, d, setup=lambda h: h.batch_set_transform(A, None, left=2, right=2))
    assert got.shape[1] == 24 and same_bits(got, want)


def test_rows_with_overlap(pkg):
    d = batch(pkg)
    got, want = rows_pair(pkg, d, setup=lambda h: h.batch_overlap(True))
    assert same_bits(got, want) and same_bits(got, d["feats"])


def test_rows_traps(pkg):
    d = batch(pkg)
    got, want = rows_pair(pkg, d, method=pkg.METHOD_TRAPS, nb=15, nc=0, dyn=0, traps_len=31, traps_dct_len=10)
    assert got.shape[1] == 150 and same_bits(got, want)


def test_rows_2048_point_stereo_44k1_to_48k(pkg):
    rng = np.random.default_rng(8)
    lens = [0, 3, 2500, 9001, 1764, 1765]
    offs, pos = [], 0
    for n in lens:
        pos += 1
        offs.append(pos)
        pos += n
    pcm = rng.integers(-32768, 32768, (pos + 4, 2)).astype(np.int16)
    d = dict(offs=offs, lens=lens, rates=[44100, 44100, 48000, 44100, 44100, 44100], pcm=pcm.reshape(-1))
    got, want = rows_pair(pkg, d, sr=48000, channels=2, W_=1102, S_=480, fft=2048)
    assert got.shape[0] > 0 and same_bits(got, want)
    # the stereo samples against the float64 sums, channel by channel
    m = make(pkg, sr=48000, channels=2, W_=1102, S_=480, fft=2048)
    m.batch_plan_rates(offs, lens, d["rates"])
    m.batch_run_host(d["pcm"])
    y = m.debug_read(8).reshape(-1, 2)
    off, ln, _ = m.batch_resample_layout()
    m.close()
    h, L, M, P = pkg.mfcc.host_resample_taps(44100, 48000)
    for u in (1, 3, 5):
        for c in (0, 1):
            o, B = RR.convert(pcm[offs[u]:offs[u] + lens[u], c], h, L, M)
            assert (np.abs(y[off[u]:off[u] + ln[u], c] - np.clip(o, -32768, 32767)) <= B).all(), (u, c)
    assert np.array_equal(y[off[2]:off[2] + ln[2]], pcm[offs[2]:offs[2] + lens[2]])


# ---- 5. plan lifecycle -----------------------------------------------------------------------------------------------------

def test_a_plain_plan_after_a_rates_plan_drops_the_converter(pkg):
    d = batch(pkg)
    off, ln, _ = d["lay"]
    padded = np.concatenate([d["y"], np.zeros(8, np.int16)])
    fresh = make(pkg)
    fresh.batch_plan(off, ln)
    want = fresh.batch_run_host(padded)
    fresh.close()
    m = make(pkg)
    with pytest.raises(pkg.MfxError) as e:
        m.batch_resample_layout()
    assert e.value.status == ERR_STATE
    m.batch_plan_rates(d["offs"], d["lens"], d["rates"])
    m.batch_run_host(d["pcm"])
    m.batch_plan(off, ln)
    assert same_bits(m.batch_run_host(padded), want)
    with pytest.raises(pkg.MfxError) as e:
        m.batch_resample_layout()
    assert e.value.status == ERR_STATE and m.debug_read(8).size == 0
    m.close()


def test_limits_and_config_errors_on_the_handle(pkg):
    m = make(pkg)
    for rates in ([999], [768001], [16001]):
        with pytest.raises(pkg.MfxError) as e:
            m.batch_plan_rates([0], [100], rates)
        assert e.value.status == -7
    with pytest.raises(pkg.MfxError) as e:
        m.batch_plan_rates([0] * 17, [10] * 17, [8000 + 100 * i for i in range(17)])
    assert e.value.status == -7
    with pytest.raises(pkg.MfxError) as e:
        m.batch_plan_rates([0], [100], [44100], zeros=65)
    assert e.value.status == -7
    # utterances at the output rate have no filter: zeros and rolloff are not judged for them (the sessions do judge them:
    # tests/test_sess_resample_gpu.py)
    x = signal(0, 500, SR, 1)
    m.batch_plan_rates([0], [500], [SR], zeros=65)
    m.batch_run_host(np.concatenate([x, np.zeros(8, np.int16)]))
    assert np.array_equal(m.debug_read(8), x)
    m.close()
    f = make(pkg, sr=16000.5)
    with pytest.raises(pkg.MfxError) as e:
        f.batch_plan_rates([0], [100], [8000])
    assert e.value.status == -5
    f.close()


def test_streaming_and_sessions_ignore_a_rates_plan(pkg):
    from conftest import synth_utterance
    x = synth_utterance(6000, 41)
    m = make(pkg)
    before = m.process_stream(x)
    m.sessions_create(2, 4000)

    def push(h):
        out = []
        for a, fin in ((0, 0), (3000, 1)):
            h.sessions_plan([1], [a], [3000], [fin])
            out.append(h.sessions_run_host(x))
        return np.concatenate(out, 0)
    sess_before = push(m)
    d = batch(pkg)
    m.batch_plan_rates(d["offs"], d["lens"], d["rates"])
    assert same_bits(m.batch_run_host(d["pcm"]), d["feats"])
    assert same_bits(m.process_stream(x), before)
    assert same_bits(push(m), sess_before) and sess_before.shape[0] > 0
    assert same_bits(m.batch_run_host(d["pcm"]), d["feats"])
    m.close()


# ---- 6. driver ---------------------------------------------------------------------------------------------------------------

def test_driver_resample_to(pkg, a0001, tmp_path):
    """afet_hip --resample-to 16000 on an 8 kHz file, a 44.1 kHz file and a 16 kHz golden file writes the rows the Python
    binding gives for the same three files (text rows, %f); without the option the mixed list fails with the reference's
    message, unchanged.  Batch mode (one mfx_batch_plan_rates per batch, extractor on MFX_ENGINE_STREAM_KERNELS) and the
    per-file loop (--batch-mb 0: a converted file is a batch of one)."""
    import os
    import subprocess
    import wave
    from conftest import GOLDEN, synth_utterance
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "asr-featext-opencl_amd", "host", "afet_hip")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", os.path.dirname(exe)])
    files = {}
    for rate, seed in ((8000, 61), (44100, 62)):
        x = synth_utterance(rate + 37, seed, sr=float(rate))        # about 1 s, an odd length
        path = str(tmp_path / ("u%d.wav" % rate))
        with wave.open(path, "wb") as f:
            f.setnchannels(1), f.setsampwidth(2), f.setframerate(rate)
            f.writeframes(x.astype("<i2").tobytes())
        files[rate] = (path, x)
    files[SR] = (os.path.join(GOLDEN, "a0001.wav"), a0001)
    order = [SR, 8000, 44100]
    opts = ["--bug-compat", "0", "--banks", "40", "--ceps", "13", "--c0", "0", "--norm", "0", "--dyn", "2", "--l1", "3", "--l2", "3",
            "--sample-limit", "200000"]

    def run(extra):
        args = []
        for r in order:
            args += [files[r][0], str(tmp_path / ("o%d.txt" % r))]
        return subprocess.run([exe] + opts + extra + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)

    def rows_of(r):
        return np.array([[float(v) for v in line.strip().strip("|").split("|")][1:] for line in open(tmp_path / ("o%d.txt" % r))])

    def printed(a):
        return np.array([[float("%f" % float(v)) for v in row] for row in a])

    # without the option: the reference's refusal, for both files at another rate
    r = run([])
    assert r.returncode == 1
    for rate in (8000, 44100):
        assert 'File "%s" has incorrect sample rate' % files[rate][0] in r.stderr
    r = run(["--batch-mb", "0"])
    assert r.returncode == 1 and r.stderr.count("has incorrect sample rate") == 2

    # batch mode against the binding: one rates plan over the three files
    r = run(["--resample-to", str(SR)])
    assert r.returncode == 0, r.stderr
    m = pkg.MfccHip(200000, W, S, 40, float(SR), 64.0, SR / 2.0, 13, False, 22.0, 0, 2, 3, 3, True, device=0, bug_compat=False,
                    engine=pkg.mfcc.ENGINE_STREAM_KERNELS)
    m.set_window(pkg.reference_window(W))
    lens = [files[k][1].size for k in order]
    offs = np.concatenate([[0], np.cumsum([n + (n & 1) for n in lens])[:-1]])
    pcm = np.zeros(int(offs[-1]) + lens[-1] + 8, np.int16)
    for o, k in zip(offs, order):
        pcm[o:o + files[k][1].size] = files[k][1]
    rows, total = m.batch_plan_rates(offs, lens, order)
    want = m.batch_run_host(pcm)
    m.close()
    bounds = np.append(rows, total)
    for i, k in enumerate(order):
        got = rows_of(k)
        assert got.shape == (bounds[i + 1] - bounds[i], 39) and got.shape[0] > 90, k
        assert np.array_equal(got, printed(want[bounds[i]:bounds[i + 1]])), "file at %d Hz" % k

    # per-file loop: the two converted files as batches of one (the 16 kHz file takes the streaming interface as always)
    for k in order:
        os.remove(tmp_path / ("o%d.txt" % k))
    r = run(["--resample-to", str(SR), "--batch-mb", "0"])
    assert r.returncode == 0, r.stderr
    m = pkg.MfccHip(200000, W, S, 40, float(SR), 64.0, SR / 2.0, 13, False, 22.0, 0, 2, 3, 3, True, device=0, bug_compat=False)
    m.set_window(pkg.reference_window(W))
    for k in (8000, 44100):
        x = files[k][1]
        m.batch_plan_rates([0], [x.size], [k])
        assert np.array_equal(rows_of(k), printed(m.batch_run_host(np.concatenate([x, np.zeros(2, np.int16)])))), k
    m.close()
    assert rows_of(SR).shape == (711, 39)
