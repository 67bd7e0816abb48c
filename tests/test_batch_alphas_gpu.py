"""Per-utterance VTLN warp factors of the batch entries (mfx_batch_set_alphas; k_melcep_runs / k_plp_runs) on the MI355X.

The main oracle needs no tolerance: rows of utterance u of a run with a per-utterance list must be BIT-IDENTICAL to the
rows of utterance u of a second handle with the same configuration plus MFX_ENGINE_STREAM_KERNELS, mfx_set_alpha(alpha_u)
and the same plan -- one reference run per distinct factor, all columns (deltas and normalised rows included).  Both sides
run the same per-row code on the same spectrum; a difference means a row's result depends on which rows share its wave
step.  Against the float64 / numpy oracles and against the default fused kernels the bar is conftest.assert_close, the one
the existing batch checks use."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import plp_ref
from conftest import GOLDEN, assert_close, synth_utterance

pytestmark = pytest.mark.gpu

STREAM_KERNELS = 8
W, S, SR = 400, 160, 16000.0
# run edges off the 4-row grid of k_melcep and the 64-row grid of k_plp; utterance 0 is shorter than one window
FRAMES = [0, 1, 3, 4, 5, 63, 64, 65, 130]
ALPHAS = np.array([1.0, 0.88, 0.88, 1.12, 1.0, 1.0, 0.88, 1.12, 1.12], np.float32)

CONFIGS = {
    # 16 kHz, 400 / 160, CVN after the deltas everywhere
    "mfcc": dict(nb=40, nc=13, dyn=2, l1=3, l2=3),
    "fbank": dict(nb=80, nc=0, dyn=2, l1=3, l2=3),
    "plp": dict(nb=40, nc=13, dyn=2, l1=3, l2=3, method="plp", lpc_order=12),
    "traps": dict(nb=15, nc=0, dyn=2, l1=3, l2=3, method="traps", traps_len=31, traps_dct_len=10),
    "mfcc1024": dict(nb=80, nc=13, dyn=2, l1=3, l2=3, fft_size=1024),      # not a 512-point shape: kSpecGen feeds it
}


def make(pkg, name, engine=0, norm=2, ibs=200000):
    kw = dict(CONFIGS[name])
    method = {"plp": pkg.METHOD_PLP, "traps": pkg.METHOD_TRAPS}.get(kw.pop("method", None), pkg.METHOD_MFCC)
    m = pkg.MfccHip(ibs, W, S, kw["nb"], SR, 64.0, SR / 2, kw["nc"], False, 22.0, norm, kw["dyn"], kw["l1"], kw["l2"], True,
                    device=0, fft_size=kw.get("fft_size", 0), bug_compat=False, engine=engine, method=method,
                    lpc_order=kw.get("lpc_order", 0), traps_len=kw.get("traps_len", 0), traps_dct_len=kw.get("traps_dct_len", 0))
    m.set_window(pkg.reference_window(W))
    return m


_RAGGED = {}


def ragged():
    """The ragged batch (computed once, never modified): utterances, even offsets, lengths, PCM."""
    if not _RAGGED:
        lens = [300 if T == 0 else (T - 1) * S + W + 7 * (i % 3) for i, T in enumerate(FRAMES)]
        utts = [synth_utterance(n, 40 + i) for i, n in enumerate(lens)]
        offs, pos = [], 0
        for n in lens:
            offs.append(pos)
            pos += n + (n & 1) + 2 * (len(offs) % 2)
        pcm = np.zeros(pos + 8, np.int16)
        for o_, u in zip(offs, utts):
            pcm[o_:o_ + u.size] = u
        for a in (pcm, *utts):
            a.setflags(write=False)
        _RAGGED.update(lens=lens, utts=utts, offs=offs, pcm=pcm)
    return _RAGGED


def reference_rows(pkg, name, offs, lens, pcm, alphas, engine=STREAM_KERNELS, norm=2, ibs=200000):
    """{factor: whole batch at that factor} from single-factor handles: one run per distinct factor."""
    out = {}
    for a in np.unique(alphas):
        r = make(pkg, name, engine=engine, norm=norm, ibs=ibs)
        r.set_alpha(float(a))
        r.batch_plan(offs, lens)
        out[np.float32(a)] = r.batch_run_host(pcm)
        r.close()
    return out


def same_bits(a, b):
    """Equality of the bit patterns (a one-frame utterance under CVN is NaN on both sides: 0 x inf)."""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def assert_rows_identical(got, ref, rows, frames, alphas, what):
    for u, (r0, T, a) in enumerate(zip(rows, frames, alphas)):
        want = ref[np.float32(a)][r0:r0 + T]
        assert got[r0:r0 + T].shape == want.shape
        assert same_bits(got[r0:r0 + T], want), "%s: utterance %d (%d frames, alpha %g) differs in %d values" % (
            what, u, T, a, int((got[r0:r0 + T].view(np.uint32) != want.view(np.uint32)).sum()))


# ---- 1. ragged batch, every method -----------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(CONFIGS))
def test_ragged_batch_bit_identical_to_single_factor_handles(pkg, name):
    d = ragged()
    m = make(pkg, name)
    rows, total = m.batch_plan(d["offs"], d["lens"])
    assert [m.batch_frames(n) for n in d["lens"]] == FRAMES and total == sum(FRAMES)
    m.batch_set_alphas(ALPHAS)
    got = m.batch_run_host(d["pcm"])
    ref = reference_rows(pkg, name, d["offs"], d["lens"], d["pcm"], ALPHAS)
    assert_rows_identical(got, ref, rows, FRAMES, ALPHAS, name)
    # the factors matter: an utterance's rows differ from the same rows at another factor
    assert not same_bits(got[rows[8]:rows[8] + 130], ref[np.float32(1.0)][rows[8]:rows[8] + 130])
    # a second run gives the same bits (nothing of the run depends on timing)
    assert same_bits(m.batch_run_host(d["pcm"]), got)
    m.close()


# ---- 2. against the float64 / numpy oracles --------------------------------------------------------------------------

def test_ragged_mfcc_against_the_oracle_at_each_utterances_factor(pkg, orc):
    """Un-normalised twin of the ragged MFCC batch against oracle_py (utterances of fewer than 2 D frames: the numpy
    restatement of the whole-utterance formulas, as tests/test_parity_gpu.py::test_c2_ragged_batch); the normalised rows
    are covered by the bit identity with handles whose normaliser the existing tests check."""
    import np_restatement as NP
    d = ragged()
    m = make(pkg, "mfcc", norm=0)
    rows, _ = m.batch_plan(d["offs"], d["lens"])
    m.batch_set_alphas(ALPHAS)
    got = m.batch_run_host(d["pcm"])
    cfg = orc.make_config(200000, window_size=W, shift=S, num_banks=40, sample_rate=SR, low_freq=64.0, high_freq=SR / 2,
                          ceps_len=13, want_c0=False, lift_coef=22.0, norm=0, dyn=2, delta_l1=3, delta_l2=3, norm_after_dyn=True)
    w = pkg.reference_window(W)
    for u, (T, a) in enumerate(zip(FRAMES, ALPHAS)):
        if T == 0:
            continue
        if T >= 12:
            want = orc.run_utterance(cfg, d["utts"][u], w, alpha=float(a), bug_compat=False)
        else:
            want = NP.mfcc_batch(d["utts"][u], w, W, S, 40, SR, 64.0, SR / 2, 13, False, 22.0, 2, 3, 3, alpha=float(a))
        assert_close(got[rows[u]:rows[u] + T], want, "utterance %d alpha %g" % (u, a), groups=3)
    m.close()


def test_ragged_plp_against_the_float64_oracle_at_each_utterances_factor(pkg):
    d = ragged()
    m = make(pkg, "plp", norm=0)
    rows, _ = m.batch_plan(d["offs"], d["lens"])
    m.batch_set_alphas(ALPHAS)
    got = m.batch_run_host(d["pcm"])
    w = pkg.reference_window(W)
    for u, (T, a) in enumerate(zip(FRAMES, ALPHAS)):
        if T == 0:
            continue
        want = plp_ref.plp_batch(d["utts"][u], w, W, S, 40, SR, 64.0, SR / 2, 13, False, 22.0, 2, 3, 3, 12, alpha=float(a))
        assert_close(got[rows[u]:rows[u] + T], want, "utterance %d alpha %g" % (u, a), groups=3)
    m.close()


# ---- 3. agreement with the default fused kernels ---------------------------------------------------------------------

@pytest.mark.parametrize("name", ["mfcc", "mfcc1024"])
def test_agrees_with_the_default_fused_kernels(pkg, name):
    d = ragged()
    m = make(pkg, name, norm=0)
    fused_name = m.dominant_kernel_name()
    rows, _ = m.batch_plan(d["offs"], d["lens"])
    m.batch_set_alphas(ALPHAS)
    got = m.batch_run_host(d["pcm"])
    ref = reference_rows(pkg, name, d["offs"], d["lens"], d["pcm"], ALPHAS, engine=0, norm=0)
    assert fused_name == {"mfcc": "k_front512", "mfcc1024": "k_front1024"}[name]
    for u, (T, a) in enumerate(zip(FRAMES, ALPHAS)):
        if T:
            assert_close(got[rows[u]:rows[u] + T], ref[np.float32(a)][rows[u]:rows[u] + T], "%s utterance %d" % (name, u), groups=3)
    m.close()


# ---- 4. slab boundary ------------------------------------------------------------------------------------------------

def test_rows_on_both_sides_of_the_slab_boundary(pkg):
    """140 utterances of 1000 frames over the same samples: 140 000 rows, the spectrum slab holds at most 2^17 = 131 072.
    The run of utterance 131 (rows 131 000 .. 131 999) is cut by the slab boundary: its rows come from two launches."""
    n = 999 * S + W
    pcm = synth_utterance(n, 3)
    n_utt = 140
    offs, lens = [0] * n_utt, [n] * n_utt
    alphas = np.array([0.9, 1.0, 1.1], np.float32)[np.arange(n_utt) % 3]
    m = make(pkg, "mfcc")
    rows, total = m.batch_plan(offs, lens)
    assert total == 140000 > 1 << 17 and rows[131] < 1 << 17 < rows[132]
    m.batch_set_alphas(alphas)
    got = m.batch_run_host(pcm)
    # (every utterance of a single-factor handle is the same utterance: one utterance per factor is the reference)
    for a in np.unique(alphas):
        r = make(pkg, "mfcc", engine=STREAM_KERNELS)
        r.set_alpha(float(a))
        r.batch_plan([0], [n])
        want = r.batch_run_host(pcm)
        r.close()
        for u in np.nonzero(alphas == a)[0]:
            assert same_bits(got[rows[u]:rows[u] + 1000], want), "utterance %d alpha %g" % (u, a)
    m.close()


# ---- 5. host slicing -------------------------------------------------------------------------------------------------

def test_sliced_host_run_with_pinned_buffers(pkg):
    """mfx_batch_run_host with buffers from mfx_alloc_pinned, ascending offsets and more than 32 MB of PCM: the 8-slice
    path, every slice after the first a range with u0 > 0 whose rows the slab window selects from the run lists."""
    L = pkg.load_library()
    L.mfx_alloc_pinned.restype, L.mfx_alloc_pinned.argtypes = C.c_void_p, [C.c_size_t]
    L.mfx_free_pinned.restype, L.mfx_free_pinned.argtypes = None, [C.c_void_p]
    rng = np.random.default_rng(11)
    n_utt = 96
    lens = [int(v) for v in rng.integers(170000, 190000, size=n_utt)]
    offs, pos = [], 0
    for n in lens:
        offs.append(pos)
        pos += n + int(rng.integers(0, 5))
    assert pos * 2 >= 32 << 20
    pcm = (3000.0 * rng.standard_normal(pos)).astype(np.int16)
    alphas = np.where(np.arange(n_utt) % 2 == 0, np.float32(0.92), np.float32(1.08)).astype(np.float32)
    m = make(pkg, "mfcc")
    rows, total = m.batch_plan(offs, lens)
    frames = [m.batch_frames(n) for n in lens]
    m.batch_set_alphas(alphas)
    width = m.get_output_data_width()
    p_in, p_out = L.mfx_alloc_pinned(pos * 2), L.mfx_alloc_pinned(total * width * 4)
    assert p_in and p_out
    try:
        C.memmove(p_in, pcm.ctypes.data, pos * 2)
        rc = L.mfx_batch_run_host(m._h, C.cast(p_in, C.POINTER(C.c_int16)), pos, C.cast(p_out, C.POINTER(C.c_float)))
        assert rc == 0, L.mfx_last_error(m._h)
        got = np.ctypeslib.as_array(C.cast(p_out, C.POINTER(C.c_float)), shape=(total, width)).copy()
    finally:
        L.mfx_free_pinned(p_in)
        L.mfx_free_pinned(p_out)
    ref = reference_rows(pkg, "mfcc", offs, lens, pcm, alphas)
    assert_rows_identical(got, ref, rows, frames, alphas, "sliced")
    assert same_bits(m.batch_run_host(pcm), got)              # pageable buffers: the whole batch in one piece, same bits
    m.close()


# ---- 6. state rules --------------------------------------------------------------------------------------------------

def status_of(fn, *args):
    try:
        fn(*args)
    except Exception as e:      # MfxError
        return e.status
    return 0


def test_state_rules(pkg):
    d = ragged()
    m = make(pkg, "mfcc1024")
    plain = make(pkg, "mfcc1024")
    rows, total = m.batch_plan(d["offs"], d["lens"])
    plain.batch_plan(d["offs"], d["lens"])
    never = plain.batch_run_host(d["pcm"])                     # a handle that never had a list
    old_name = m.dominant_kernel_name()
    assert old_name == "k_front1024"
    # arguments
    assert status_of(m.batch_set_alphas, ALPHAS[:-1]) == -7
    assert status_of(m.batch_set_alphas, np.concatenate([ALPHAS, ALPHAS[:1]])) == -7
    for bad in (0.0, -1.0, np.nan):
        a = ALPHAS.copy()
        a[4] = bad
        assert status_of(m.batch_set_alphas, a) == -7
        assert "alpha must be positive" in m._L.mfx_last_error(m._h).decode()
    assert m.dominant_kernel_name() == old_name                # a refused list changes nothing
    assert same_bits(m.batch_run_host(d["pcm"]), never)
    # in force: the spectrum kernel runs and is named; profiling times it
    m.batch_set_alphas(ALPHAS)
    assert m.dominant_kernel_name() == "k_front_reg"
    m.profile_enable(True)
    with_list = m.batch_run_host(d["pcm"])
    launches, ms = m.profile_read()
    m.profile_enable(False)
    assert launches == 1 and ms > 0
    assert not same_bits(with_list, never)
    # mfx_set_alpha + a streaming block on the same handle: unaffected by the list, and the list by them
    pcm = synth_utterance(30000, 9)
    fresh = make(pkg, "mfcc1024")
    streamed = []
    for e in (m, fresh):
        n = e.set_input(pcm)
        e.set_alpha(0.93)
        e.apply()
        streamed.append(e.get_output_data(n))
    assert same_bits(streamed[0], streamed[1])
    assert same_bits(m.batch_run_host(d["pcm"]), with_list)
    m.set_alpha(1.0)
    # clearing: bit for bit the rows and the kernel of a handle that never had a list
    m.batch_set_alphas(None)
    assert m.dominant_kernel_name() == old_name
    assert same_bits(m.batch_run_host(d["pcm"]), never)
    # a new plan clears the list too
    m.batch_set_alphas(ALPHAS)
    assert m.dominant_kernel_name() == "k_front_reg"
    m.batch_plan(d["offs"], d["lens"])
    assert m.dominant_kernel_name() == old_name
    assert same_bits(m.batch_run_host(d["pcm"]), never)
    for e in (m, plain, fresh):
        e.close()


def test_more_than_4096_distinct_factors_are_refused(pkg):
    m = make(pkg, "mfcc", norm=0)
    n_utt = 4097
    pcm = synth_utterance(W, 1)
    m.batch_plan([0] * n_utt, [W] * n_utt)
    a = (np.float32(0.8) + np.arange(n_utt, dtype=np.float32) * np.float32(1e-5)).astype(np.float32)
    assert np.unique(a).size == n_utt
    assert status_of(m.batch_set_alphas, a) == -7
    m.batch_set_alphas(a[:-1].tolist() + [a[0]])               # 4096 distinct values: accepted
    got = m.batch_run_host(pcm)
    assert got.shape[0] == n_utt and np.isfinite(got[:, :13]).all()
    assert np.array_equal(got[0], got[-1]) and not np.array_equal(got[0, :13], got[4095, :13])
    m.close()


# ---- 7. the driver ---------------------------------------------------------------------------------------------------

def exe_path():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "asr-featext-opencl_amd", "host", "afet_hip")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", os.path.dirname(exe)])
    return exe


@pytest.mark.parametrize("opts", [
    ["--banks", "40", "--ceps", "13", "--c0", "0", "--norm", "2", "--dyn", "2"],                           # MFCC, text rows
    ["--method", "TRAPS", "--htk"],
], ids=["mfcc-text", "traps-htk"])
def test_driver_alpha_file_equals_one_run_per_factor(tmp_path, opts):
    exe = exe_path()
    srcs = ["a0001.wav", "a1.wav", "a0001.wav", "a1.wav", "a1.wav", "a0001.wav"]
    factors = ["0.9", "1.0", "1.1", "0.9", "1.1", "1.0"]
    alpha_file = tmp_path / "alphas.txt"
    alpha_file.write_text("\n".join(factors) + "\n")

    def run(tag, extra, which):
        args = []
        for i in which:
            args += [os.path.join(GOLDEN, srcs[i]), str(tmp_path / ("%s_%d.out" % (tag, i)))]
        subprocess.check_call([exe] + opts + extra + args, stdout=subprocess.DEVNULL)
        return {i: open(tmp_path / ("%s_%d.out" % (tag, i)), "rb").read() for i in which}

    listed = run("list", ["--alpha-file", str(alpha_file)], range(len(srcs)))
    assert all(len(v) > 1000 for v in listed.values())
    for a in sorted(set(factors)):
        which = [i for i, f in enumerate(factors) if f == a]
        single = run("single" + a, ["--alpha", a], which)
        for i in which:
            assert listed[i] == single[i], "file %d (%s) at alpha %s" % (i, srcs[i], a)
    assert listed[0] != listed[5]                              # the same file at 0.9 and at 1.0


def test_driver_alpha_file_usage_errors(tmp_path):
    exe = exe_path()
    wav = os.path.join(GOLDEN, "a0001.wav")
    two = tmp_path / "two.txt"
    two.write_text("0.9\n1.1\n")
    files = [wav, str(tmp_path / "a.out")]
    run = lambda extra: subprocess.run([exe] + extra + files, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL).returncode
    assert run(["--alpha-file", str(two)]) == 2                                    # two factors, one file
    one = tmp_path / "one.txt"
    one.write_text("0.9\n")
    assert run(["--alpha-file", str(one), "--alpha", "1.0"]) == 2
    assert run(["--alpha-file", str(one), "--alpha-min", "0.9", "--alpha-max", "1.1", "--alpha-step", "0.1"]) == 2
    assert run(["--alpha-step", "0.1", "--alpha-file", str(one)]) == 2
    assert run(["--alpha-file", str(tmp_path / "missing.txt")]) == 2
    assert run(["--alpha-file", str(one)]) == 0
