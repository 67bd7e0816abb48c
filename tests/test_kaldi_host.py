"""CPU tests of the Kaldi front end (MFX_METHOD_KALDI = 7): the symbols, the configuration rules and the setter's answers through
planning handles (no device), the two host-built tables against the float64 oracle of tests/kaldi_ref.py bit for bit after
rounding -- with anchors computed in double for M = 23, N = 512, 16 kHz, 20 Hz .. Nyquist --, the kernel's LDS over the limits
of the method, and the stand-alone sanitizer program."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import kaldi_ref as KR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "asr-featext-opencl_amd", "csrc")
LDS = 160 * 1024

SYMBOLS = ("mfx_kaldi_set_options", "mfx_host_kaldi_mel_table", "mfx_host_kaldi_dct", "mfx_host_kaldi_lds_bytes")

# the shapes of tests/test_kaldi_gpu.py: W, S, M, C, sample rate, low, high, Q
SHAPES = (
    (400, 160, 80, 0, 16000.0, 20.0, 0.0, 22.0),
    (400, 160, 23, 13, 16000.0, 20.0, 0.0, 22.0),
    (400, 160, 40, 40, 16000.0, 20.0, -400.0, 22.0),
    (200, 80, 23, 13, 8000.0, 20.0, 0.0, 22.0),
    (100, 50, 10, 0, 4000.0, 20.0, 0.0, 22.0),
    (65, 7, 3, 3, 16000.0, 20.0, 0.0, 0.0),
    (512, 512, 128, 0, 16000.0, 0.0, 0.0, 22.0),
)


def config(pkg, W=400, S=160, M=80, C_=0, sr=16000.0, low=20.0, high=0.0, Q=22.0, want_c0=0, norm=0, dyn=0, l1=2, l2=2, fft_size=0,
           channels=1, method=7):
    cfg = pkg.MfxConfig(200000, W, S, M, sr, low, high, C_, want_c0, Q, norm, dyn, l1, l2, 1, fft_size, channels, 0, 0, 0, 0)
    cfg.method = method
    return cfg


def plan(pkg, **kw):
    """(status, planning handle or None)"""
    L = pkg.load_library()
    h = C.c_void_p()
    rc = L.mfx_plan_create(C.byref(config(pkg, **kw)), C.byref(h))
    return rc, (h if rc == 0 else None)


def test_symbols_are_declared_and_exported(pkg):
    L = pkg.load_library()
    header = open(os.path.join(ROOT, "include", "mfx.h")).read()
    for s in SYMBOLS:
        assert hasattr(L, s), s
        assert s in pkg.mfcc.EXPORTED_SYMBOLS
        assert re.search(r"\b%s\s*\(" % s, re.sub(r"/\*.*?\*/", "", header, flags=re.S)), s
    assert "MFX_METHOD_KALDI = 7" in header
    assert pkg.METHOD_KALDI == 7
    assert L.mfx_method_supported(7) == 1 and L.mfx_method_supported(6) == 0
    assert L.mfx_abi_version() == 2


@pytest.mark.parametrize("shape", SHAPES, ids=["%d-%d-%d-%d" % s[:4] for s in SHAPES])
def test_planning_handle_shapes(pkg, shape):
    W, S, M, Cc, sr, low, high, Q = shape
    L = pkg.load_library()
    for dyn in (0, 2):
        rc, h = plan(pkg, W=W, S=S, M=M, C_=Cc, sr=sr, low=low, high=high, Q=Q, dyn=dyn)
        assert rc == 0
        try:
            assert L.mfx_dominant_kernel_name(h).decode() == "k_kaldi_front"
            for aligned in (0, 1):      # (whatever the alignment)
                L.mfx_plan_set_aligned(h, aligned)
                assert L.mfx_dominant_kernel_name(h).decode() == "k_kaldi_front"
            assert L.mfx_get_output_data_width(h) == (Cc or M) * (1 + dyn)
            assert L.mfx_fft_size(h) == KR.fft_size(W)
            assert L.mfx_batch_frames(h, W - 1) == 0 and L.mfx_batch_frames(h, W) == 1
            assert L.mfx_batch_frames(h, W + S - 1) == 1 and L.mfx_batch_frames(h, W + S) == 2
            assert L.mfx_batch_frames(h, 0) == 0
        finally:
            L.mfx_destroy(h)
    assert pkg.plan_kernel(W, S, M, sr, Cc, method=pkg.METHOD_KALDI, low_freq=low, high_freq=high) == "k_kaldi_front"


def test_engine_bits_do_not_move_the_kernel(pkg):
    for engine in (0, 8, 128, 1 | 4):
        assert pkg.plan_kernel(400, 160, 80, 16000.0, 0, method=pkg.METHOD_KALDI, low_freq=20.0, high_freq=0.0, engine=engine) == "k_kaldi_front"


REFUSED = {
    "window 64": dict(W=64, S=32),
    "window 513": dict(W=513),
    "shift 0": dict(S=0),
    "shift W + 1": dict(S=401),
    "no band": dict(M=0),
    "129 bands": dict(M=129),
    "fft_size 1024": dict(fft_size=1024),
    "fft_size 256 under a 400-tap window": dict(fft_size=256),
    "stereo": dict(channels=2),
    "negative low": dict(low=-1.0),
    "low at high": dict(low=4000.0, high=4000.0),
    "low above the offset high": dict(low=7700.0, high=-400.0),
    "high above Nyquist": dict(high=8000.5),
    "offset high at zero": dict(high=-8000.0),
    "more cepstra than bands": dict(M=23, C_=24),
    "negative cepstra": dict(C_=-1),
    "want_c0": dict(M=23, C_=13, want_c0=1),
    "want_c0 on fbank": dict(want_c0=1),
    "negative lifter": dict(M=23, C_=13, Q=-1.0),
    "NaN lifter": dict(M=23, C_=13, Q=float("nan")),
    "delta order 0": dict(dyn=2, l1=0),
    "norm 4": dict(norm=4),
}


@pytest.mark.parametrize("what", sorted(REFUSED))
def test_configuration_refusals(pkg, what):
    rc, h = plan(pkg, **REFUSED[what])
    assert h is None and rc == -5, (what, rc)


def test_configuration_limits_accepted(pkg):
    L = pkg.load_library()
    ok = (dict(W=65, S=1, M=1), dict(W=512, S=512, M=128, C_=128, Q=0.0), dict(fft_size=512), dict(W=128, S=64, M=10, fft_size=128, sr=4000.0),
          dict(channels=0), dict(high=8000.0), dict(high=-0.0), dict(M=23, C_=13, Q=0.0), dict(M=23, C_=23), dict(norm=2, dyn=2),
          dict(low=0.0), dict(M=23, C_=1))
    for kw in ok:
        rc, h = plan(pkg, **kw)
        assert rc == 0, kw
        L.mfx_destroy(h)
    # the general rule "lift_coef == 0 is refused" still holds for the other cepstral methods
    rc, h = plan(pkg, M=23, C_=13, Q=0.0, high=8000.0, method=0)
    assert rc == -5 and h is None
    rc, h = plan(pkg, method=6, high=8000.0)
    assert rc == -5 and h is None


def test_setter_answers(pkg):
    L = pkg.load_library()
    f = L.mfx_kaldi_set_options
    rc, h = plan(pkg)
    assert rc == 0
    try:
        assert f(h, 0.97, 1, 1) == 0 and f(h, 0.0, 0, 0) == 0 and f(h, 1.0, 1, 0) == 0     # works on a planning handle
        for c in (-0.01, 1.01, float("nan"), float("inf"), -float("inf")):
            assert f(h, c, 1, 1) == -7, c
        for dc, pw in ((2, 1), (-1, 1), (1, 2), (1, -1)):
            assert f(h, 0.97, dc, pw) == -7, (dc, pw)
        assert "mfx_kaldi_set_options" in L.mfx_last_error(h).decode()
    finally:
        L.mfx_destroy(h)
    rc, h = plan(pkg, M=23, C_=13, high=8000.0, method=0)         # not a Kaldi handle
    assert rc == 0
    try:
        assert f(h, 0.97, 1, 1) == -5
    finally:
        L.mfx_destroy(h)
    assert f(None, 0.97, 1, 1) == -7


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def test_mel_table_anchors(pkg):
    w, beg, ln = pkg.host_kaldi_mel_table(23, 512, 16000.0, 20.0, 0.0)
    assert w.shape == (23, 256)
    assert (beg[0], ln[0]) == (1, 5)
    want = np.array([0.14932837, 0.55237826, 0.93923697, 0.68884475, 0.33075566])
    assert np.abs(w[0, 1:6].astype(np.float64) - want).max() <= 6e-8 * 1.0      # half an ulp of 1 around the printed digits
    assert (w[0, :1] == 0).all() and (w[0, 6:] == 0).all()
    assert (beg[22], beg[22] + ln[22] - 1) == (204, 255)
    # Kaldi's offset rule: high_freq = -400 is Nyquist - 400, and Nyquist itself is 0
    a = pkg.host_kaldi_mel_table(40, 512, 16000.0, 20.0, -400.0)
    b = pkg.host_kaldi_mel_table(40, 512, 16000.0, 20.0, 7600.0)
    c = pkg.host_kaldi_mel_table(40, 512, 16000.0, 20.0, 8000.0)
    d = pkg.host_kaldi_mel_table(40, 512, 16000.0, 20.0, 0.0)
    assert all(np.array_equal(bits(x), bits(y)) for x, y in zip(a, b)) and all(np.array_equal(bits(x), bits(y)) for x, y in zip(c, d))
    assert not np.array_equal(bits(a[0]), bits(c[0]))
    # 512 points, 128 bands from 0 Hz: band 0 ends below bin 1 and bin 0 sits on its left edge -- empty; no other band is
    w, beg, ln = pkg.host_kaldi_mel_table(128, 512, 16000.0, 0.0, 0.0)
    assert list(np.nonzero(ln == 0)[0]) == [0] and not w[0].any()
    with pytest.raises(pkg.MfxError):
        pkg.host_kaldi_mel_table(23, 1024, 16000.0, 20.0, 0.0)
    with pytest.raises(pkg.MfxError):
        pkg.host_kaldi_mel_table(23, 512, 16000.0, 20.0, 8001.0)
    with pytest.raises(pkg.MfxError):
        pkg.host_kaldi_mel_table(129, 512, 16000.0, 20.0, 0.0)


def test_dct_anchors(pkg):
    g = pkg.host_kaldi_dct(23, 13, 22.0)
    assert g.shape == (13, 23)
    for (i, m), v in {(0, 0): 0.20851441, (1, 0): 0.75475022, (12, 22): 2.39275183}.items():
        assert abs(float(g[i, m]) - v) <= 1.3e-7 * max(1.0, abs(v)), (i, m, float(g[i, m]))
    assert (g[0] == g[0, 0]).all()                                        # c0: the plain sum, no lifter at i = 0
    plain = pkg.host_kaldi_dct(23, 13, 0.0)
    assert np.array_equal(bits(plain[0]), bits(g[0])) and not np.array_equal(bits(plain[1]), bits(g[1]))
    for bad in ((23, 0, 22.0), (23, 24, 22.0), (23, 13, -1.0), (0, 1, 22.0)):
        with pytest.raises(pkg.MfxError):
            pkg.host_kaldi_dct(*bad)


@pytest.mark.parametrize("shape", SHAPES, ids=["%d-%d-%d-%d" % s[:4] for s in SHAPES])
def test_tables_equal_the_oracle_bit_for_bit(pkg, shape):
    W, S, M, Cc, sr, low, high, Q = shape
    N = KR.fft_size(W)
    got = pkg.host_kaldi_mel_table(M, N, sr, low, high)
    want = KR.mel_table(M, N, sr, low, high)
    assert np.array_equal(bits(got[0]), bits(want[0])) and np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2])
    assert (got[1] + got[2] <= N // 2).all()
    if Cc:
        assert np.array_equal(bits(pkg.host_kaldi_dct(M, Cc, Q)), bits(KR.dct(M, Cc, Q)))
    assert np.array_equal(bits(pkg.povey_window(W)), bits(KR.povey_window(W)))


def test_lds_stays_inside_a_block_over_the_limits(pkg):
    f = pkg.load_library().mfx_host_kaldi_lds_bytes
    worst = 0
    for W in range(65, 513):
        for M in (1, 80, 128):
            for Cc in (0, M):
                # (monotone in S: the staged span is 15 S + W samples -- the ends and the power-of-two steps of the hop)
                for S in sorted({1, 2, 7, W // 4, W // 2, W - 1, W}):
                    if S < 1:
                        continue
                    b = f(W, S, M, Cc)
                    assert 0 < b <= LDS, (W, S, M, Cc, b)
                    worst = max(worst, b)
    for W in (65, 128, 129, 256, 257, 400, 512):      # every hop at the windows where the DFT length steps
        for S in range(1, W + 1):
            assert 0 < f(W, S, 128, 128) <= LDS
    assert worst == f(512, 512, 128, 128) == pkg.host_kaldi_lds_bytes(512, 512, 128, 128)
    assert pkg.host_kaldi_lds_bytes(400, 160, 80, 0) < 48 * 1024           # three blocks per CU at fbank-80
    for bad in ((64, 32, 10, 0), (513, 160, 80, 0), (400, 0, 80, 0), (400, 401, 80, 0), (400, 160, 0, 0), (400, 160, 129, 0), (400, 160, 23, 24)):
        assert f(*bad) == -7, bad
    print("k_kaldi_front: at most %d bytes of LDS (512 / 512 / 128 / 128), %d at 400 / 160 / 80 / 0" % (worst, f(400, 160, 80, 0)))


def test_oracle_silence_and_frames():
    z = KR.features(np.zeros(1000, np.int16), KR.povey_window(400), 160, 80, 16000.0, 20.0, 0.0)
    assert z.shape == (4, 80) and np.allclose(z, -15.9424, atol=1e-4)
    assert KR.features(np.zeros(399, np.int16), KR.povey_window(400), 160, 80, 16000.0, 20.0, 0.0).shape == (0, 80)
    assert KR.features(np.full(1000, 12345, np.int16), KR.povey_window(400), 160, 23, 16000.0, 20.0, 0.0, C=13).shape == (4, 13)


def test_host_driver_runs_clean_under_the_sanitizers(tmp_path):
    """tools/asan/kaldi_asan.cpp (the two table builders and a restatement of the kernel's FFT stages) as `make asan` builds and
    runs it: a stand-alone CPU program under AddressSanitizer + UBSan, linked against mfx_tables.cpp alone."""
    gxx = shutil.which("g++")
    assert gxx, "g++ was not found"
    exe = str(tmp_path / "kaldi_asan")
    r = subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-ffp-contract=off", "-o", exe,
                        os.path.join(ROOT, "tools", "asan", "kaldi_asan.cpp"), os.path.join(CSRC, "mfx_tables.cpp")],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-2000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env)
    assert r.returncode == 0 and "tables clean" in r.stdout, r.stdout[-2000:]
    assert "kaldi_asan" in open(os.path.join(CSRC, "Makefile")).read()


def test_kernel_builds_for_gfx950_without_private_memory():
    """mfx_kaldi.hip compiled for gfx950 as the Makefile compiles it: k_kaldi_front uses no scratch and no static LDS."""
    hipcc = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    assert os.path.exists(hipcc), "hipcc (the compiler build() uses) was not found"
    r = subprocess.run([hipcc, "-O3", "-fPIC", "-std=c++17", "--offload-arch=gfx950", "-fno-slp-vectorize",
                        "-Rpass-analysis=kernel-resource-usage", "-c", "mfx_kaldi.hip", "-o", os.devnull],
                       cwd=CSRC, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-2000:]
    names = re.findall(r"Function Name: (\S+)", r.stdout)
    assert len(names) == 1 and "k_kaldi_front" in names[0], names
    assert [int(v) for v in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stdout)] == [0]
    assert [int(v) for v in re.findall(r"LDS Size \[bytes/block\]: (\d+)", r.stdout)] == [0]
    assert "mfx_kaldi" in open(os.path.join(CSRC, "Makefile")).read()
