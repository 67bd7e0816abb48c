"""PLP cepstra on the MI355X (k_plp) against the float64 oracle of tests/plp_ref.py, at the north-star bar
(conftest.assert_close: 1e-4 of scale, 1e-5 rel-L2, per column group)."""
import os
import struct
import subprocess
import threading

import numpy as np
import pytest

import plp_ref
from conftest import GOLDEN, assert_close, synth_utterance

pytestmark = pytest.mark.gpu


def groups_of(dyn):
    return {0: 1, 1: 2, 2: 3}[dyn]


def make(pkg, ibs, W=400, S=160, nb=40, sr=16000.0, low=64.0, high=None, nc=13, c0=True, lift=22.0, norm=0, dyn=2,
         l1=3, l2=3, nad=True, p=12, fft_size=0, channels=1, bug_compat=False, batch_norm_stats=0, method=None, engine=0):
    m = pkg.MfccHip(ibs, W, S, nb, sr, low, sr / 2 if high is None else high, nc, c0, lift, norm, dyn, l1, l2, nad, device=0,
                    fft_size=fft_size, channels=channels, bug_compat=bug_compat, batch_norm_stats=batch_norm_stats,
                    method=pkg.METHOD_PLP if method is None else method, lpc_order=p, engine=engine)
    m.set_window(pkg.reference_window(W))
    return m


def oracle(pkg, pcm, W=400, S=160, nb=40, sr=16000.0, low=64.0, high=None, nc=13, c0=True, lift=22.0, dyn=2, l1=3, l2=3,
           p=12, fft_size=0, alpha=1.0):
    return plp_ref.plp_batch(pcm, pkg.reference_window(W), W, S, nb, sr, low, sr / 2 if high is None else high, nc, c0, lift,
                             dyn, l1, l2, p, alpha=alpha, fft_size=fft_size)


def run_batch(m, utts):
    lens = [u.size for u in utts]
    offs = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
    rows, total = m.batch_plan(offs, lens)
    out = m.batch_run_host(np.concatenate(utts))
    return [out[rows[i]:rows[i] + m.batch_frames(lens[i])] for i in range(len(utts))]


# ---- batch entry ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nb", [26, 40])
def test_plp_batch_ragged(pkg, a0001, nb):
    utts = [synth_utterance(n, s) for s, n in enumerate([16000, 4000, 23456, 401, 9999])] + [a0001]
    m = make(pkg, 200000, nb=nb)
    got = run_batch(m, utts)
    for i, (u, g) in enumerate(zip(utts, got)):
        assert_close(g, oracle(pkg, u, nb=nb), "utt %d nb %d" % (i, nb), groups=3)
    m.close()


SHAPES = [
    ("8k 256 stuffed", dict(W=200, S=80, nb=23, sr=8000.0)),
    ("16k 512", dict()),
    ("16k fft 1024", dict(nb=80, fft_size=1024)),
    ("44.1k stereo 2048", dict(W=1102, S=441, nb=128, sr=44100.0, nc=40, channels=2)),
    ("48k 4096", dict(W=2400, S=480, nb=64, sr=48000.0, nc=20)),
]


@pytest.mark.parametrize("name,shape", SHAPES, ids=[s[0] for s in SHAPES])
@pytest.mark.parametrize("p,nc,dyn", [(1, 13, 0), (8, 13, 1), (12, 13, 2), (12, 8, 2), (24, 13, 1), (24, 30, 2)])
def test_plp_shape_matrix(pkg, name, shape, p, nc, dyn):
    shape = dict(shape)
    nb = shape.get("nb", 40)
    p = min(p, nb)
    base_nc = shape.pop("nc", 13)
    nc = base_nc if nc == 13 else nc
    ch = shape.pop("channels", 1)
    sr = shape.get("sr", 16000.0)
    n = int(1.3 * sr)
    pcm = synth_utterance(n * ch, 3, sr=sr)
    m = make(pkg, 4 * n, nc=nc, dyn=dyn, p=p, channels=ch, **shape)
    got = run_batch(m, [pcm])[0] if ch == 1 else None
    if ch == 2:
        m.batch_plan([0], [n])
        got = m.batch_run_host(pcm)
        pcm = plp_ref.downmix(pcm)
    kw = {k: v for k, v in shape.items()}
    want = oracle(pkg, pcm, nc=nc, dyn=dyn, p=p, **kw)
    assert_close(got, want, "%s p %d C %d dyn %d" % (name, p, nc, dyn), groups=groups_of(dyn))
    m.close()


# ---- streaming ------------------------------------------------------------------------------------------------------

def stream(m, pcm, block):
    rows, pos = [], 0
    while pos < pcm.size:
        n = m.set_input(pcm[pos:pos + block])
        pos += block
        if n > 0:
            m.apply()
            rows.append(m.get_output_data(n))
    n = m.flush()
    if n > 0:
        m.apply()
        rows.append(m.get_output_data(n))
    return rows


def frame_map(orc, pcm, block, bug_compat, T):
    """Frame index of every static row a streaming run delivers, read off the MFCC oracle (same state machine): its
    streamed statics matched to its whole-utterance statics."""
    cfg = orc.make_config(block, num_banks=40, ceps_len=13, want_c0=True, dyn=2)
    got = orc.run_utterance(cfg, pcm, bug_compat=bug_compat, block_samples=block)[:, :14]
    whole = orc.run_utterance(orc.make_config(pcm.size + 1000, num_banks=40, ceps_len=13, want_c0=True, dyn=0), pcm,
                              bug_compat=False)
    d = ((got[:, None, :] - whole[None, :T, :]) ** 2).sum(-1)
    return d.argmin(1)


@pytest.mark.parametrize("bug_compat", [0, 1])
@pytest.mark.parametrize("block", [4000, 40000])
def test_plp_streaming_statics(pkg, orc, bug_compat, block):
    pcm = synth_utterance(30000, 11)
    m = make(pkg, block, bug_compat=bool(bug_compat))
    rows = np.concatenate(stream(m, pcm, min(block, m.get_input_buffer_size())))
    statics = oracle(pkg, pcm, dyn=0)
    idx = frame_map(orc, pcm, min(block, m.get_input_buffer_size()), bool(bug_compat), statics.shape[0])
    assert rows.shape[0] == idx.size
    assert_close(rows[:, :14], statics[idx], "statics block %d bug_compat %d" % (block, bug_compat))
    if not bug_compat:
        assert_close(rows, oracle(pkg, pcm), "whole utterance, block %d" % block, groups=3)
    m.close()


def test_plp_batch_one_block_equals_streaming(pkg):
    pcm = synth_utterance(20000, 5)
    m = make(pkg, 40000)
    s = np.concatenate(stream(m, pcm, m.get_input_buffer_size()))
    m.close()
    b = make(pkg, 40000, engine=8)  # MFX_ENGINE_STREAM_KERNELS: the streaming interface's kernels (PLP has no other)
    got = run_batch(b, [pcm])[0]
    b2 = make(pkg, 40000)
    got2 = run_batch(b2, [pcm])[0]
    assert np.array_equal(got, s) and np.array_equal(got2, s)
    b.close()
    b2.close()


# ---- VTLN -----------------------------------------------------------------------------------------------------------

def test_plp_vtln(pkg):
    pcm = synth_utterance(24000, 7)
    alphas = [0.88, 1.0, 1.12]
    m = make(pkg, 40000)
    n = m.set_input(pcm)
    per = []
    for a in alphas:
        m.set_alpha(a)
        m.apply()
        per.append(m.get_output_data(n))
        want = oracle(pkg, pcm, alpha=a)[:n]
        assert_close(per[-1][:, :14], want[:, :14], "alpha %g statics" % a)
    m.apply_alphas(np.array(alphas, np.float32))
    for i in range(len(alphas)):
        assert np.array_equal(m.get_output_data_alpha(i, n), per[i]), "sweep alpha %g" % alphas[i]
    m.close()


# ---- normalisation --------------------------------------------------------------------------------------------------

def np_norm(x, kind, stats=None):
    """normalizercpu.cpp:22-89 on rows x [n][dim]: returns (normalised rows, mean, multiplier)."""
    x = np.asarray(x, np.float64)
    if stats is None:
        n = x.shape[0]
        s, s2 = x.sum(0), (x * x).sum(0)
        mean = s / n
        if kind == 1:
            mult = np.ones_like(mean)
        elif kind == 2:
            mult = np.sqrt((n - 1) / (s2 - s * (s / n)))
        else:
            mult = 1.0 / np.maximum(np.abs(x.min(0) - mean), np.abs(x.max(0) - mean))
    else:
        mean, mult = stats
    return (x - mean) * mult, mean, mult


def restate_block(x, st, kind, nad, cols):
    """Normalise a NONE twin's rows with statistics st [G][2][cols] (mfx_debug_read 5 / 6)."""
    if nad:
        mean, mult = st[:, 0].reshape(-1), st[:, 1].reshape(-1)
        return np_norm(x, kind, (mean, mult))[0]
    mean, mult = st[0, 0], st[0, 1]
    y = np.asarray(x, np.float64) * np.tile(mult, x.shape[1] // cols)
    y[:, :cols] -= mean * mult
    return y


@pytest.mark.parametrize("kind", [1, 2, 3])
@pytest.mark.parametrize("nad", [0, 1])
def test_plp_streaming_norm(pkg, kind, nad):
    pcm = synth_utterance(30000, 9)  # blocks of 11 920, 11 920, 6 160 samples: none of one row (degenerate statistics)
    block = 12000
    m = make(pkg, block, norm=kind, nad=bool(nad))
    m0 = make(pkg, block, norm=0, nad=bool(nad))
    twin = np.concatenate(stream(m0, pcm, m0.get_input_buffer_size()))
    assert_close(twin, oracle(pkg, pcm), "NONE twin", groups=3)
    pos, r0, last_stats = 0, 0, None
    limit = m.get_input_buffer_size()
    while True:
        flush = pos >= pcm.size
        n = m.flush() if flush else m.set_input(pcm[pos:pos + limit])
        pos += limit
        if n > 0:
            m.apply()
            y = m.get_output_data(n)
            st = m.debug_read(5).reshape(-1, 2, 13 + 1)
            x = twin[r0:r0 + n]
            if nad:  # statistics of the block's own rows (a flush block re-uses the previous block's)
                want_y, mean, mult = np_norm(x, kind, last_stats if flush else None)
                if not flush:
                    last_stats = (mean, mult)
                np.testing.assert_allclose(st[:, 0].reshape(-1), mean, rtol=1e-4, atol=1e-4 * np.abs(x).max())
                np.testing.assert_allclose(st[:, 1].reshape(-1), mult, rtol=1e-3)
            else:
                want_y = restate_block(x, st, kind, nad, 14)
            assert_close(y, want_y, "norm %d nad %d rows %d" % (kind, nad, r0), groups=3)
            r0 += n
        if flush:
            break
    assert r0 == twin.shape[0]
    m.close()
    m0.close()


@pytest.mark.parametrize("kind", [1, 2, 3])
@pytest.mark.parametrize("nad", [0, 1])
@pytest.mark.parametrize("bns", [0, 1])
def test_plp_batch_norm(pkg, kind, nad, bns):
    utts = [synth_utterance(n, 20 + n % 7) for n in (16000, 9000, 30000)]
    m = make(pkg, 100000, norm=kind, nad=bool(nad), batch_norm_stats=bns)
    m0 = make(pkg, 100000, norm=0, nad=bool(nad))
    ys, xs = run_batch(m, utts), run_batch(m0, utts)
    G = 3 if nad else 1
    st = m.debug_read(6).reshape(G, len(utts), 2, 14)
    for u, (y, x) in enumerate(zip(ys, xs)):
        assert_close(x, oracle(pkg, utts[u]), "twin utt %d" % u, groups=3)
        if nad:
            rows = x if bns else x[:x.shape[0] - 6]  # D = l1 + l2 = 6 flush rows re-use the block's statistics
            _, mean, mult = np_norm(rows, kind)
            np.testing.assert_allclose(st[:, u, 0].reshape(-1), mean, rtol=1e-4, atol=1e-4 * np.abs(x).max())
            np.testing.assert_allclose(st[:, u, 1].reshape(-1), mult, rtol=1e-3)
        want = restate_block(x, st[:, u], kind, nad, 14)
        assert_close(y, want, "norm %d nad %d bns %d utt %d" % (kind, nad, bns, u), groups=3)
    m.close()
    m0.close()


# ---- stage tap ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("p", [8, 12, 20])
def test_plp_autocorrelation_tap(pkg, p):
    pcm = synth_utterance(16000, 4)
    m = make(pkg, 40000, p=p, dyn=0)
    n = m.set_input(pcm)
    m.apply()
    r = m.debug_read(7).reshape(-1, p + 1)
    v = plp_ref.spectrum(pcm, pkg.reference_window(400), 400, 160, 512)
    _, want = plp_ref.plp_frames(v, 40, 512, 16000.0, 64.0, 8000.0, p, 13, True, 22.0, want_r=True)
    assert r.shape[0] >= n
    k = min(r.shape[0], want.shape[0])
    err = np.abs(r[:k] - want[:k]) / want[:k, :1]
    assert err.max() <= 1e-5, err.max()
    m.close()


# ---- hard inputs ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("what", ["silence", "tone", "clipped"])
def test_plp_hard_inputs(pkg, what):
    n = 16000
    t = np.arange(n)
    if what == "silence":
        pcm = np.zeros(n, np.int16)
    elif what == "tone":
        pcm = np.round(32767 * np.sin(2 * np.pi * 1000.0 * t / 16000.0)).astype(np.int16)
    else:
        pcm = np.clip(np.round(40000 * np.random.default_rng(3).standard_normal(n)), -32768, 32767).astype(np.int16)
    m = make(pkg, 40000)
    got = run_batch(m, [pcm])[0]
    assert np.isfinite(got).all()
    want = oracle(pkg, pcm)
    # silence: every row is rounding noise around the 1e-30 floor; tone: 160 samples are 10 whole periods, so the frames are
    # identical and the deltas are rounding noise of the statics -- measured against the statics' scale
    floor = {"silence": 1.0, "tone": np.abs(want[:, :14]).max(), "clipped": 0.0}[what]
    assert_close(got, want, what, groups=3, scale_floor=floor)
    m.close()


# ---- mixed handles --------------------------------------------------------------------------------------------------

def test_plp_mfcc_handles_interleaved(pkg):
    pcm = [synth_utterance(20000, s) for s in range(4)]
    alone = {}
    for meth in (0, 1):
        m = make(pkg, 8000, method=meth)
        alone[meth] = [np.concatenate(stream(m, x, m.get_input_buffer_size())) for x in pcm]
        m.close()
    hs = {meth: make(pkg, 8000, method=meth) for meth in (0, 1)}
    for i, x in enumerate(pcm):  # one thread, blocks of the two handles interleaved
        outs = {0: [], 1: []}
        lim = hs[0].get_input_buffer_size()
        for pos in range(0, x.size, lim):
            for meth in (1, 0):
                n = hs[meth].set_input(x[pos:pos + lim])
                if n > 0:
                    hs[meth].apply()
                    outs[meth].append(hs[meth].get_output_data(n))
        for meth in (0, 1):
            n = hs[meth].flush()
            if n > 0:
                hs[meth].apply()
                outs[meth].append(hs[meth].get_output_data(n))
            assert np.array_equal(np.concatenate(outs[meth]), alone[meth][i]), (i, meth)
    res, errs = {}, []

    def work(meth):
        try:
            res[meth] = [np.concatenate(stream(hs[meth], x, hs[meth].get_input_buffer_size())) for x in pcm * 3]
        except Exception as e:  # pragma: no cover
            errs.append(e)
    th = [threading.Thread(target=work, args=(meth,)) for meth in (0, 1)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errs, errs
    for meth in (0, 1):
        for i, r in enumerate(res[meth]):
            assert np.array_equal(r, alone[meth][i % 4]), ("two threads", meth, i)
        hs[meth].close()


# ---- driver ---------------------------------------------------------------------------------------------------------

def test_plp_driver_htk(pkg, orc, tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "asr-featext-opencl_amd", "host", "afet_hip")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", os.path.dirname(exe)])
    opts = ["--method", "PLP", "--model-order", "12", "--banks", "26", "--ceps", "13", "--c0", "1", "--norm", "0",
            "--dyn", "2", "--l1", "3", "--l2", "3", "--sample-limit", "20000", "--bug-compat", "0"]
    riff = os.path.join(GOLDEN, "sample1_riff.wav")
    t, h = tmp_path / "r.txt", tmp_path / "r.htk"
    subprocess.check_call([exe] + opts + [riff, str(t)])
    subprocess.check_call([exe] + opts + ["--htk", riff, str(h)])
    rows = np.array([[float(v) for v in line.strip().strip("|").split("|")] for line in open(t)])
    pcm, sr = orc.read_wav_pcm16(riff)
    pcm = pcm[:, 0].copy()
    want = oracle(pkg, pcm, nb=26)
    assert rows.shape == (want.shape[0], 1 + 42)
    assert_close(rows[:, 1:], want, "afet_hip --method PLP", groups=3)
    raw = open(h, "rb").read()
    n, period, size, kind = struct.unpack(">iihh", raw[:12])
    assert (n, period, size) == (want.shape[0], 100000, 4 * 42)
    assert kind & 0xFFFF == 11 | 0x2000 | 0x0100 | 0x0200          # PLP_0_D_A
    htk = np.frombuffer(raw[12:], dtype=">f4").reshape(n, 42)
    assert np.abs(htk - rows[:, 1:]).max() <= 5.1e-7 * max(1.0, np.abs(htk).max()) + 5e-7
