"""CPU tests of the Kaldi front end's options (kaldi_flags and kaldi_energy_floor of mfx_create_kaldi): the frame rule of snip_edges = false
and the closed-form mirror against Kaldi's loop (tests/kaldi_opts_ref.py), widths and refusals through planning handles, the
options-aware LDS query, the padded-twin identity the GPU module relies on, shown on the float64 oracle, and the stand-alone
sanitizer program.

LDS over the cap: inside the method's limits (W <= 512, M <= 128) no flag word brings a block over 160 KB -- the worst shape
stays near 70 KB, test_lds_query below walks the limits --, so that refusal cannot be provoked through a configuration; what is
checked instead is that the query mfx_create consults is the flags-aware one and stays under the cap everywhere."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import kaldi_opts_ref as KO
import kaldi_ref as KR
from conftest import synth_utterance

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "asr-featext-opencl_amd", "csrc")
LDS = 160 * 1024
ERR_CONFIG, ERR_ARG = -5, -7
SHAPES_WS = ((400, 160), (401, 161), (512, 512), (65, 1), (200, 80))


def plan(pkg, W=400, S=160, M=23, Cc=0, flags=0, floor=0.0, dyn=0, method=7):
    L = pkg.load_library()
    cfg = pkg.MfxConfig(200000, W, S, M, 16000.0, 20.0, 0.0, Cc, 0, 22.0, 0, dyn, 2, 2, 1, 0, 1, 0, 0, 0, 0)
    cfg.method = method
    h = C.c_void_p()
    rc = L.mfx_plan_create_kaldi(C.byref(cfg), flags, floor, C.byref(h))
    return rc, (h if rc == 0 else None)


def test_symbols_and_constants(pkg):
    L = pkg.load_library()
    header = open(os.path.join(ROOT, "include", "mfx.h")).read()
    for s in ("mfx_create_kaldi", "mfx_plan_create_kaldi", "mfx_kaldi_flags_supported", "mfx_host_kaldi_lds_bytes_flags", "mfx_host_kaldi_frame_count", "mfx_host_kaldi_frame_samples"):
        assert hasattr(L, s) and s in pkg.mfcc.EXPORTED_SYMBOLS and s in header, s
    assert L.mfx_kaldi_flags_supported() == 15 == pkg.kaldi_flags_supported()
    assert (pkg.KALDI_NO_SNIP_EDGES, pkg.KALDI_USE_ENERGY, pkg.KALDI_ENERGY_WINDOWED, pkg.KALDI_HTK_COMPAT) == (1, 2, 4, 8)
    for name, v in (("NO_SNIP_EDGES", 1), ("USE_ENERGY", 2), ("ENERGY_WINDOWED", 4), ("HTK_COMPAT", 8)):
        assert "#define MFX_KALDI_%s %d" % (name, v) in header
    assert [f[0] for f in pkg.MfxConfig._fields_][-1] == "logmel_post"      # (the options are arguments: mfx_config is what it was)


@pytest.mark.parametrize("W,S", SHAPES_WS)
def test_frame_count_against_the_oracle(pkg, W, S):
    f = pkg.load_library().mfx_host_kaldi_frame_count
    for n in range(0, 2001):
        assert f(n, W, S, 1) == KO.frame_count(n, W, S, 1) == ((n + S // 2) // S if n else 0), n
        assert f(n, W, S, 0) == KR.frame_count(n, W, S), n
    assert f(-1, W, S, 1) == ERR_ARG and f(10, 64, 1, 1) == ERR_ARG and f(10, W, S, 16) == ERR_ARG


@pytest.mark.parametrize("W,S", SHAPES_WS)
def test_frame_samples_equal_kaldis_loop(pkg, W, S):
    for n in (1, 2, 79, 80, 81, 199, 200, 201, 400, 1000):
        T = KO.frame_count(n, W, S, 1)
        assert T == pkg.host_kaldi_frame_count(n, W, S, 1)
        for t in range(T):
            got = pkg.host_kaldi_frame_samples(n, W, S, 1, t)
            want = KO.frame_samples(n, W, S, 1, t)
            assert np.array_equal(got, want), (n, t)
            assert got.min() >= 0 and got.max() < n
        with pytest.raises(pkg.MfxError):
            pkg.host_kaldi_frame_samples(n, W, S, 1, T)
    # snip_edges = true: the plain run of taps
    assert np.array_equal(pkg.host_kaldi_frame_samples(2000, W, S, 0, 1), np.arange(S, S + W))


def test_mirror_far_outside_the_utterance(pkg):
    """One sample: every tap of every frame reads it (Kaldi's loop runs hundreds of times; the closed form does not)."""
    assert np.array_equal(pkg.host_kaldi_frame_samples(1, 512, 1, 1, 0), np.zeros(512, np.int64))
    assert np.array_equal(pkg.host_kaldi_frame_samples(3, 400, 2, 1, 1), KO.frame_samples(3, 400, 2, 1, 1))


def test_widths_on_planning_handles(pkg):
    L = pkg.load_library()
    for (M, Cc, flags, dyn, width) in ((23, 0, 0, 0, 23), (23, 0, 2, 0, 24), (23, 0, 2 | 8, 0, 24), (23, 0, 8, 0, 23), (23, 0, 1, 0, 23),
                                       (23, 0, 6, 2, 72), (128, 0, 2, 0, 129), (23, 13, 2, 0, 13), (23, 13, 15, 2, 39), (23, 1, 10, 0, 1)):
        rc, h = plan(pkg, M=M, Cc=Cc, flags=flags, dyn=dyn)
        assert rc == 0, (M, Cc, flags)
        try:
            assert L.mfx_get_output_data_width(h) == width, (M, Cc, flags, dyn)
            assert L.mfx_batch_frames(h, 1000) == KO.frame_count(1000, 400, 160, flags)
            assert L.mfx_dominant_kernel_name(h).decode() == ("k_kaldi_front_opts" if flags else "k_kaldi_front")
        finally:
            L.mfx_destroy(h)


def test_refusals(pkg):
    assert plan(pkg, flags=16)[0] == ERR_CONFIG                  # unknown bit
    assert plan(pkg, flags=-1)[0] == ERR_CONFIG
    assert plan(pkg, flags=4)[0] == ERR_CONFIG                   # ENERGY_WINDOWED without USE_ENERGY
    assert plan(pkg, flags=4 | 8 | 1)[0] == ERR_CONFIG
    for floor in (-1.0, -1e-30, float("inf"), float("nan")):
        assert plan(pkg, flags=2, floor=floor)[0] == ERR_CONFIG, floor
    L = pkg.load_library()
    rc, h = plan(pkg, flags=6, floor=1.0)
    assert rc == 0
    L.mfx_destroy(h)
    # the entry is a Kaldi handle's: another method is refused, and (0, 0) is mfx_plan_create itself
    assert plan(pkg, Cc=13, flags=0, method=0)[0] == ERR_CONFIG and plan(pkg, Cc=13, flags=2, method=0)[0] == ERR_CONFIG
    rc, h = plan(pkg, Cc=13)
    assert rc == 0 and L.mfx_get_output_data_width(h) == 13 and L.mfx_batch_frames(h, 1000) == KR.frame_count(1000, 400, 160)
    assert L.mfx_dominant_kernel_name(h).decode() == "k_kaldi_front"
    L.mfx_destroy(h)


def test_lds_query(pkg):
    L = pkg.load_library()
    f, g = L.mfx_host_kaldi_lds_bytes, L.mfx_host_kaldi_lds_bytes_flags
    # the pinned values of the plain query (tests/test_kaldi_host.py holds them too) and flags 0 of the new one
    assert f(400, 160, 80, 0) < 48 * 1024
    worst = 0
    for W in (65, 128, 129, 200, 256, 257, 400, 512):
        for S in (1, W // 2, W):
            for M, Cc in ((1, 0), (23, 0), (23, 13), (80, 0), (128, 0), (128, 128)):
                assert g(W, S, M, Cc, 0) == f(W, S, M, Cc) == pkg.host_kaldi_lds_bytes(W, S, M, Cc)
                for flags in (1, 2, 3, 6, 8, 10, 15):
                    b = g(W, S, M, Cc, flags)
                    assert b == pkg.host_kaldi_lds_bytes(W, S, M, Cc, flags) and f(W, S, M, Cc) <= b <= LDS
                    worst = max(worst, b)
                    grows = Cc == 0 and (flags & 2) and 16 * (M + 1) > 15 * S + W
                    assert (b > f(W, S, M, Cc)) == bool(grows and ((16 * (M + 1) + 3) & ~3) > ((max(15 * S + W, 16 * M) + 3) & ~3))
    assert g(400, 160, 80, 0, 3) == f(400, 160, 80, 0)               # fbank-80 + energy: still three blocks per CU
    assert g(400, 160, 80, 0, 4) == ERR_ARG and g(400, 160, 80, 0, 16) == ERR_ARG and g(64, 160, 80, 0, 0) == ERR_ARG
    print("k_kaldi_front_opts: at most %d bytes of LDS" % worst)


@pytest.mark.parametrize("W,S", SHAPES_WS)
def test_padded_twin_identity_on_the_oracle(W, S):
    """features(y) under snip_edges = true == features(x) under snip_edges = false, exactly: the same arithmetic on the same
    samples.  tests/test_kaldi_opts_gpu.py holds the kernel's rows of x to the flags-0 handle's rows of y, bit for bit."""
    win = KR.povey_window(W)
    for n in (1, 79, 80, 81, 199, 16 * S, 17 * S, 33 * S + 7):
        x = synth_utterance(n, 7 + n)
        y = KO.padded_twin(x, W, S)
        T = KO.frame_count(n, W, S, 1)
        assert y.size == ((T - 1) * S + W if T else 0) and KR.frame_count(y.size, W, S) == T
        for M, Cc in ((23, 0), (23, 13)):
            a = KO.features(x, win, S, M, 16000.0, 20.0, 0.0, Cc, flags=1)
            b = KR.features(y, win, S, M, 16000.0, 20.0, 0.0, Cc)
            assert a.shape == b.shape == (T, Cc or M) and np.array_equal(a, b), (n, M, Cc)
            c = KO.features(y, win, S, M, 16000.0, 20.0, 0.0, Cc, flags=14, energy_floor=2.0)
            d = KO.features(x, win, S, M, 16000.0, 20.0, 0.0, Cc, flags=15, energy_floor=2.0)
            assert np.array_equal(c, d)


def test_oracle_columns():
    """The column orders of the oracle against one another (what the GPU module checks on the kernel's bits)."""
    x = synth_utterance(3000, 5)
    win = KR.povey_window(400)
    args = (x, win, 160, 23, 16000.0, 20.0, 0.0)
    fb, fe, fh = KO.features(*args), KO.features(*args, flags=2), KO.features(*args, flags=10)
    assert np.array_equal(fb, KR.features(*args)) and np.array_equal(fe[:, 1:], fb) and np.array_equal(fh[:, :23], fb)
    assert np.array_equal(fh[:, 23], fe[:, 0]) and np.array_equal(KO.features(*args, flags=8), fb)
    mf = KO.features(*args, C=13)
    me, mh, meh = KO.features(*args, C=13, flags=2), KO.features(*args, C=13, flags=8), KO.features(*args, C=13, flags=10)
    assert np.array_equal(me[:, 1:], mf[:, 1:]) and np.array_equal(me[:, 0], fe[:, 0])
    assert np.array_equal(mh[:, :12], mf[:, 1:]) and np.array_equal(mh[:, 12], mf[:, 0] * KO.SQRT2)
    assert np.array_equal(meh[:, :12], mf[:, 1:]) and np.array_equal(meh[:, 12], fe[:, 0])
    # raw energy of a frame by hand; the floor
    d = x[:400].astype(np.float64) - float(np.float32(x[:400].astype(np.int64).sum()) / np.float32(400))
    assert abs(fe[0, 0] - np.log((d ** 2).sum())) <= 1e-12 * abs(fe[0, 0])
    assert KO.features(np.zeros(400, np.int16), win, 160, 23, 16000.0, 20.0, 0.0, flags=2)[0, 0] == KR.SILENCE
    assert KO.features(np.zeros(400, np.int16), win, 160, 23, 16000.0, 20.0, 0.0, flags=2, energy_floor=1.0)[0, 0] == 0.0


def test_sanitizer_program(tmp_path):
    """tools/asan/kaldi_opts_asan.cpp as `make asan` builds and runs it: mfx_host_kaldi_frame_samples' worker into exactly sized
    buffers for n in 0 .. 3 W, the closed form against Kaldi's loop, every index in [0, n); a stand-alone CPU program under
    AddressSanitizer + UBSan, linked against mfx_tables.cpp alone."""
    gxx = shutil.which("g++")
    assert gxx, "g++ was not found"
    exe = str(tmp_path / "kaldi_opts_asan")
    r = subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-ffp-contract=off", "-o", exe,
                        os.path.join(ROOT, "tools", "asan", "kaldi_opts_asan.cpp"), os.path.join(CSRC, "mfx_tables.cpp")],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-2000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env)
    assert r.returncode == 0 and "frame rule clean" in r.stdout, r.stdout[-2000:]
    assert "kaldi_opts_asan" in open(os.path.join(CSRC, "Makefile")).read()
