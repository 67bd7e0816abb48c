"""TRAPS temporal patterns on the MI355X (fused front end -> k_traps -> delta / normaliser) against the float64 oracle of
tests/traps_ref.py.

Bars (conftest.assert_close): the statics at the project bar as it stands, 1e-4 of scale and 1e-5 rel-L2.  The delta and
delta-delta groups are checked one group at a time at the same two figures with scale_floor = max |oracle statics|: a
delta of a TRAPS row is a small difference of large, slowly varying numbers (scale ~0.2 against statics of ~19), the
regression moves an error of the statics by at most sum(2 l) / (2 sum(l^2)) = 0.43 at l = 3, so the bar on the statics
implies 1e-4 max|statics| on the deltas, not 1e-4 max|delta|; a wrong clamp or tap still shows at ~1e-2 of that scale.

That bar alone lets a delta column be wrong by 1 % of its own range.  check() therefore also holds every delta and
delta-delta value against the float64 restatement of the rows' OWN statics within float32 rounding bounds
(tail_ref.assert_tail_consistent: about 1e-7 relative, no oracle noise in it).
"""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

import plp_ref
import tail_ref
import traps_ref
from conftest import GOLDEN, assert_close, assert_normalised_close, synth_utterance  # noqa: F401

pytestmark = pytest.mark.gpu


def make(pkg, ibs=200000, W=400, S=160, nb=15, sr=16000.0, low=64.0, high=None, L=31, K=10, norm=0, dyn=2, l1=3, l2=3,
         nad=True, fft_size=0, channels=1, batch_norm_stats=0, engine=0, lift=22.0):
    m = pkg.MfccHip(ibs, W, S, nb, sr, low, sr / 2 if high is None else high, 0, False, lift, norm, dyn, l1, l2, nad,
                    device=0, fft_size=fft_size, channels=channels, bug_compat=False, batch_norm_stats=batch_norm_stats,
                    method=pkg.METHOD_TRAPS, traps_len=L, traps_dct_len=K, engine=engine)
    m.set_window(pkg.reference_window(W))
    return m


def oracle(pkg, pcm, W=400, S=160, nb=15, sr=16000.0, low=64.0, high=None, L=31, K=10, dyn=2, l1=3, l2=3, fft_size=0,
           alpha=1.0):
    return traps_ref.traps_batch(pcm, pkg.reference_window(W), W, S, nb, sr, low, sr / 2 if high is None else high, L, K,
                                 dyn, l1, l2, alpha=alpha, fft_size=fft_size)


def run_batch(m, utts):
    lens = [u.size for u in utts]
    offs = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
    rows, total = m.batch_plan(offs, lens)
    out = m.batch_run_host(np.concatenate(utts))
    return [out[rows[i]:rows[i] + m.batch_frames(lens[i])] for i in range(len(utts))]


def check(got, want, dyn, what, floor=0.0, worst=None, l1=3, l2=3, tail=True):
    """Statics at the bar; every delta group at the bar with the statics' scale as the floor (module docstring); and the
    delta groups of `got` against its own statics.  tail=False only for rows that are not [static | d | dd] in float32:
    rows normalised AFTER the deltas (every group has its own mean and multiplier) and rows read back from decimal text."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, "%s: shape %s vs %s" % (what, got.shape, want.shape)
    if want.shape[0] == 0:
        return
    g = 1 + dyn
    c = want.shape[1] // g
    if dyn > 0 and tail:
        w = tail_ref.assert_tail_consistent(got, c, dyn, l1, l2 if dyn == 2 else 0, what)
        print("%s: deltas against their own statics, worst err / bound %s" % (what, w))
    s_scale = float(np.abs(want[:, :c]).max())
    for i in range(g):
        a, b = got[:, i * c:(i + 1) * c], want[:, i * c:(i + 1) * c]
        fl = floor if i == 0 else max(floor, s_scale)
        scale = max(np.abs(b).max(), 1e-30, fl)
        emax = np.abs(a.astype(np.float64) - b).max() / scale
        el2 = np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30, fl * np.sqrt(b.size))
        print("%s group %d: max err / scale = %.3g, rel L2 = %.3g (scale %.3g)" % (what, i, emax, el2, scale))
        if worst is not None:
            worst[i] = max(worst.get(i, 0.0), emax)
        assert_close(a, b, "%s group %d" % (what, i), scale_floor=fl)


def samples_for(frames, W=400, S=160, extra=36):
    """An even sample count that gives exactly `frames` frames (0: shorter than one window)."""
    return W - S + frames * S + extra if frames > 0 else W - 100


# ---- 1. ragged batch ------------------------------------------------------------------------------------------------

RAGGED_FRAMES = [1, 2, 15, 16, 0, 31, 32, 98, 145]  # H = 15, L = 31; 145 rows cross two 64-row tile boundaries


@pytest.fixture(scope="module")
def ragged(pkg, a0001):
    utts = [synth_utterance(samples_for(t), 40 + i) for i, t in enumerate(RAGGED_FRAMES)] + [a0001[:a0001.size & ~1]]
    m = make(pkg, dyn=0)
    got = run_batch(m, utts)
    m.close()
    return utts, got


def test_ragged_batch_against_oracle(pkg, ragged):
    utts, got = ragged
    for i, (u, g) in enumerate(zip(utts, got)):
        want = oracle(pkg, u, dyn=0)
        if i < len(RAGGED_FRAMES):
            assert want.shape[0] == RAGGED_FRAMES[i]
        check(g, want, 0, "utt %d (%d frames)" % (i, want.shape[0]))


@pytest.fixture(scope="module")
def ragged_dyn2(pkg, ragged):
    """The same batch with deltas on: the 1-, 2-, 15- and 16-frame utterances through the delta stage."""
    m = make(pkg, dyn=2)
    got = run_batch(m, ragged[0])
    m.close()
    return got


def test_ragged_batch_with_deltas(pkg, ragged, ragged_dyn2):
    utts, statics = ragged
    for i, (u, g, s) in enumerate(zip(utts, ragged_dyn2, statics)):
        assert g.shape == (s.shape[0], 450)
        assert np.array_equal(g[:, :150], s), "utt %d: statics differ from the dyn = NONE handle's" % i
        if i < len(RAGGED_FRAMES):
            check(g, oracle(pkg, u), 2, "dyn 2, utt %d (%d frames)" % (i, RAGGED_FRAMES[i]))
        elif g.shape[0]:   # (the long utterance's oracle is computed once, for the dyn = NONE rows)
            w = tail_ref.assert_tail_consistent(g, 150, 2, 3, 3, "dyn 2, utt %d" % i)
            print("dyn 2, utt %d (%d frames): worst err / bound %s" % (i, g.shape[0], w))


def test_ragged_batch_rows_do_not_depend_on_the_batch(pkg, ragged):
    utts, got = ragged
    m = make(pkg, dyn=0)
    for i, u in enumerate(utts):
        alone = run_batch(m, [u])[0]
        assert np.array_equal(alone, got[i]), "utt %d alone differs from its rows in the batch" % i
    again = run_batch(m, utts)
    for i in range(len(utts)):
        assert np.array_equal(again[i], got[i]), "second run differs, utt %d" % i
    m.close()


def test_ragged_batch_device_entry_equals_host_entry(pkg, ragged):
    import torch
    utts, got = ragged
    m = make(pkg, dyn=0)
    lens = [u.size for u in utts]
    offs = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
    rows, total = m.batch_plan(offs, lens)
    dev = torch.device("cuda", 0)
    pcm = torch.from_numpy(np.concatenate(utts)).to(dev)
    out = torch.full((total, 150), float("nan"), dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    m.batch_run_device(pcm.data_ptr(), pcm.numel(), out.data_ptr())
    m.synchronize()
    host = out.cpu().numpy()
    for i in range(len(utts)):
        assert np.array_equal(host[rows[i]:rows[i] + got[i].shape[0]], got[i]), "utt %d" % i
    m.close()


# ---- 2. shape matrix ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("M,L,K,dyn", [(15, 31, 10, 2), (23, 31, 10, 1), (40, 11, 6, 2), (26, 3, 1, 0), (16, 51, 16, 0),
                                       (8, 101, 32, 0)])
@pytest.mark.parametrize("engine", [0, 512], ids=["mfma", "valu"])
def test_shape_matrix(pkg, M, L, K, dyn, engine):
    pcm = synth_utterance(int(1.3 * 16000), 3)
    m = make(pkg, nb=M, L=L, K=K, dyn=dyn, engine=engine)
    got = run_batch(m, [pcm])[0]
    m.close()
    check(got, oracle(pkg, pcm, nb=M, L=L, K=K, dyn=dyn), dyn, "M %d L %d K %d dyn %d" % (M, L, K, dyn))


def test_matrix_and_vector_forms_give_the_same_bits(pkg):
    pcm = synth_utterance(int(1.3 * 16000), 3)
    outs = []
    for engine in (0, 512):
        m = make(pkg, engine=engine)
        outs.append(run_batch(m, [pcm])[0])
        m.close()
    assert np.array_equal(outs[0], outs[1])


FRONT_ENDS = [
    ("8k 256 stuffed", dict(W=200, S=80, sr=8000.0), "k_front512"),
    ("16k fft 1024", dict(fft_size=1024), "k_front1024"),
    ("44.1k stereo 2048", dict(W=1102, S=441, nb=25, sr=44100.0, channels=2), "k_front2048"),
    ("48k 4096 slab", dict(W=2400, S=480, sr=48000.0), "k_front_reg"),
    ("stream kernels", dict(engine=8), "k_front512"),
]


@pytest.mark.parametrize("name,shape,kernel", FRONT_ENDS, ids=[s[0] for s in FRONT_ENDS])
def test_front_ends(pkg, name, shape, kernel):
    shape = dict(shape)
    ch = shape.pop("channels", 1)
    engine = shape.pop("engine", 0)
    sr = shape.get("sr", 16000.0)
    n = int(1.3 * sr) & ~1
    pcm = synth_utterance(n * ch, 3, sr=sr)
    m = make(pkg, ibs=4 * n, channels=ch, engine=engine, **shape)
    assert m.dominant_kernel_name() == kernel
    if ch == 2:
        m.batch_plan([0], [n])
        got = m.batch_run_host(pcm)
        pcm = plp_ref.downmix(pcm)
    else:
        got = run_batch(m, [pcm])[0]
    m.close()
    check(got, oracle(pkg, pcm, **shape), 2, name)


def test_odd_utterance_offset(pkg):
    utts = [synth_utterance(16001, 8), synth_utterance(20000, 9)]  # the second utterance starts on an odd sample
    m = make(pkg)
    got = run_batch(m, utts)
    m.close()
    for i, (u, g) in enumerate(zip(utts, got)):
        check(g, oracle(pkg, u), 2, "unaligned build, utt %d" % i)


# ---- 3. VTLN --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("alpha", [0.88, 1.12])
def test_vtln(pkg, alpha):
    pcm = synth_utterance(24000, 7)
    m = make(pkg)
    m.set_alpha(alpha)
    got = run_batch(m, [pcm])[0]
    m.close()
    check(got, oracle(pkg, pcm, alpha=alpha), 2, "alpha %g" % alpha)


# ---- 4. normalisation -----------------------------------------------------------------------------------------------

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
    """Normalise a NONE twin's rows with statistics st [G][2][cols] (mfx_debug_read 6)."""
    if nad:
        mean, mult = st[:, 0].reshape(-1), st[:, 1].reshape(-1)
        return np_norm(x, kind, (mean, mult))[0]
    mean, mult = st[0, 0], st[0, 1]
    y = np.asarray(x, np.float64) * np.tile(mult, x.shape[1] // cols)
    y[:, :cols] -= mean * mult
    return y


@pytest.fixture(scope="module")
def norm_utts():
    return [synth_utterance(n, 20 + n % 7) for n in (16000, 9000, 30000)]


@pytest.fixture(scope="module")
def norm_twins(pkg, norm_utts):
    """The norm = NONE rows of both orders and their oracle, computed once."""
    out = {}
    for nad in (0, 1):
        m0 = make(pkg, norm=0, nad=bool(nad))
        out[nad] = run_batch(m0, norm_utts)
        m0.close()
    want = [oracle(pkg, u) for u in norm_utts]
    return out, want


@pytest.mark.parametrize("kind", [1, 2, 3])
@pytest.mark.parametrize("nad", [0, 1])
@pytest.mark.parametrize("bns", [0, 1])
def test_batch_norm(pkg, norm_utts, norm_twins, kind, nad, bns):
    cols = 150
    m = make(pkg, norm=kind, nad=bool(nad), batch_norm_stats=bns)
    ys = run_batch(m, norm_utts)
    xs, wants = norm_twins[0][nad], norm_twins[1]
    G = 3 if nad else 1
    st = m.debug_read(6).reshape(G, len(norm_utts), 2, cols)
    for u, (y, x) in enumerate(zip(ys, xs)):
        check(x, wants[u], 2, "twin utt %d" % u)
        if nad:
            rows = x if bns else x[:x.shape[0] - 6]  # D = l1 + l2 = 6 flush rows re-use the block's statistics
            _, mean, mult = np_norm(rows, kind)
            np.testing.assert_allclose(st[:, u, 0].reshape(-1), mean, rtol=1e-4, atol=1e-4 * np.abs(x).max())
            np.testing.assert_allclose(st[:, u, 1].reshape(-1), mult, rtol=1e-3)
        want = restate_block(x, st[:, u], kind, nad, cols)
        check(y, want, 2, "norm %d nad %d bns %d utt %d" % (kind, nad, bns, u), tail=not nad)
    m.close()


# ---- 5. overlap -----------------------------------------------------------------------------------------------------

def test_batch_overlap(pkg):
    import torch
    dev = torch.device("cuda", 0)
    lens = [samples_for(t) for t in (98, 145, 31, 200)]
    offs = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
    batches = [np.concatenate([synth_utterance(n, 60 + 10 * b + i) for i, n in enumerate(lens)]) for b in range(3)]
    res = {}
    for overlap in (0, 1):
        m = make(pkg)
        rows, total = m.batch_plan(offs, lens)
        if overlap:
            m.batch_overlap(True)
        pcms = [torch.from_numpy(b).to(dev) for b in batches]
        outs = [torch.full((total, 450), float("nan"), dtype=torch.float32, device=dev) for _ in batches]
        torch.cuda.synchronize()
        for p, o in zip(pcms, outs):
            m.batch_run_device(p.data_ptr(), p.numel(), o.data_ptr())
        m.synchronize()
        res[overlap] = [o.cpu().numpy() for o in outs]
        m.close()
    for b in range(3):
        assert np.isfinite(res[0][b]).all()
        assert np.array_equal(res[0][b], res[1][b]), "batch %d" % b
    assert not np.array_equal(res[0][0], res[0][1])


# ---- 6. hard inputs -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("what", ["silence", "tone", "clipped"])
def test_hard_inputs(pkg, what):
    n = 16000
    t = np.arange(n)
    if what == "silence":
        pcm = np.zeros(n, np.int16)
    elif what == "tone":
        pcm = np.round(32767 * np.sin(2 * np.pi * 1000.0 * t / 16000.0)).astype(np.int16)
    else:
        pcm = np.clip(np.round(40000 * np.random.default_rng(3).standard_normal(n)), -32768, 32767).astype(np.int16)
    m = make(pkg)
    got = run_batch(m, [pcm])[0]
    m.close()
    assert np.isfinite(got).all()
    want = oracle(pkg, pcm)
    # silence: every log energy is log(1e-30) = -69.08, the coefficients k > 0 of a constant trajectory cancel to rounding
    # noise of that input: its scale is the yardstick.  tone: 160 samples are 10 whole periods, the frames are identical
    # and the oracle's deltas exactly zero: check() measures them against the statics' scale, as it does for every input
    check(got, want, 2, what, floor=69.08 if what == "silence" else 0.0)
    if what == "tone":
        assert np.abs(want[:, 150:]).max() <= 1e-9


# ---- 7. streaming refusal -------------------------------------------------------------------------------------------

def test_streaming_entries_are_refused(pkg):
    m = make(pkg)
    L, h = m._L, m._h
    pcm = synth_utterance(16000, 2)
    n = C.c_int32(0)
    buf = np.zeros(450 * 4, np.float32)
    fp = buf.ctypes.data_as(C.POINTER(C.c_float))
    a = np.array([0.9, 1.1], np.float32)
    calls = {
        "mfx_set_input": lambda: L.mfx_set_input(h, pcm.ctypes.data_as(C.POINTER(C.c_int16)), pcm.size, C.byref(n)),
        "mfx_flush": lambda: L.mfx_flush(h, C.byref(n)),
        "mfx_apply": lambda: L.mfx_apply(h),
        "mfx_apply_alphas": lambda: L.mfx_apply_alphas(h, a.ctypes.data_as(C.POINTER(C.c_float)), 2),
        "mfx_get_output_data": lambda: L.mfx_get_output_data(h, fp, 4),
        "mfx_get_output_data_alpha": lambda: L.mfx_get_output_data_alpha(h, 0, fp, 4),
    }
    for name, call in calls.items():
        assert call() == -8, name
        assert b"batch" in L.mfx_last_error(h), name
    with pytest.raises(pkg.MfxError) as e:
        m.process_stream(pcm)
    assert e.value.status == -8
    # geometry accessors, set_alpha and the batch entries still work
    assert m.get_output_data_width() == 450 and m.fft_size() == 512 and m.get_input_buffer_size() > 0
    m.set_alpha(1.0)
    got = run_batch(m, [pcm])[0]
    m.close()
    check(got, oracle(pkg, pcm), 2, "batch after refused streaming calls")


# ---- 8. mixed handles -----------------------------------------------------------------------------------------------

def test_mixed_handles(pkg):
    utts = [synth_utterance(n, 70 + i) for i, n in enumerate((16000, 4000, 23456))]

    def other(meth):
        m = pkg.MfccHip(200000, 400, 160, 26, 16000.0, 64.0, 8000.0, 13, True, 22.0, 0, 2, 3, 3, True, device=0,
                        bug_compat=False, method=meth, lpc_order=12)
        m.set_window(pkg.reference_window(400))
        return m

    alone = {}
    for meth in (pkg.METHOD_MFCC, pkg.METHOD_PLP):
        m = other(meth)
        alone[meth] = run_batch(m, utts)
        m.close()
    t = make(pkg)
    alone[pkg.METHOD_TRAPS] = run_batch(t, utts)
    t.close()

    before = {meth: other(meth) for meth in (pkg.METHOD_MFCC, pkg.METHOD_PLP)}
    t = make(pkg)
    after = {meth: other(meth) for meth in (pkg.METHOD_MFCC, pkg.METHOD_PLP)}
    for rnd in range(2):
        got_t = run_batch(t, utts)
        for i in range(len(utts)):
            assert np.array_equal(got_t[i], alone[pkg.METHOD_TRAPS][i]), ("traps", rnd, i)
        for which, hs in (("before", before), ("after", after)):
            for meth, m in hs.items():
                got = run_batch(m, utts)
                for i in range(len(utts)):
                    assert np.array_equal(got[i], alone[meth][i]), (which, meth, rnd, i)
    for m in list(before.values()) + list(after.values()) + [t]:
        m.close()


# ---- 9. driver ------------------------------------------------------------------------------------------------------

def test_driver(pkg, orc, tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "asr-featext-opencl_amd", "host", "afet_hip")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", os.path.dirname(exe)])
    # (--norm 0: the driver's default is the reference's CVN; the oracle states the un-normalised rows)
    opts = ["--method", "TRAPS", "--traps-length", "31", "--traps-dct", "10", "--banks", "15", "--dyn", "2", "--norm", "0"]
    riff = os.path.join(GOLDEN, "sample1_riff.wav")
    t, h = tmp_path / "r.txt", tmp_path / "r.htk"
    subprocess.check_call([exe] + opts + [riff, str(t)])
    subprocess.check_call([exe] + opts + ["--htk", riff, str(h)])
    rows = np.array([[float(v) for v in line.strip().strip("|").split("|")] for line in open(t)])
    pcm, sr = orc.read_wav_pcm16(riff)
    pcm = pcm[:, 0].copy()
    want = oracle(pkg, pcm, W=int(sr * 25e-3), S=int(sr * 10e-3), sr=float(sr))
    assert rows.shape == (want.shape[0], 1 + 450)
    check(rows[:, 1:], want, 2, "afet_hip --method TRAPS (text)", tail=False)   # (six decimals, not float32)
    raw = open(h, "rb").read()
    n, period, size, kind = struct.unpack(">iihh", raw[:12])
    assert (n, period, size) == (want.shape[0], 100000, 4 * 450)
    assert kind & 0xFFFF == 9 | 0x0100 | 0x0200          # USER_D_A
    htk = np.frombuffer(raw[12:], dtype=">f4").reshape(n, 450)
    check(htk, want, 2, "afet_hip --method TRAPS (htk)")
    assert np.abs(htk - rows[:, 1:]).max() <= 5.1e-7 * max(1.0, np.abs(htk).max()) + 5e-7
    r = subprocess.run([exe] + opts + ["--batch-mb", "0", riff, str(t)], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 2
