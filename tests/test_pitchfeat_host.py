"""Pitch features of the batch entries (mfx_batch_set_pitch_feats) on the CPU: the declared and exported symbols, what a
planning handle answers, every limit through mfx_host_pitch_feats, the host restatement against the float64 reference and
its bound (pitchfeat_ref.py) on every input the GPU tests use, a constant track, a linear ramp, POV at and beyond rho = +-1,
three rows worked by hand, the new translation unit's resource usage when compiled for gfx950, and the sanitizer run of the
host code (no GPU)."""
import ctypes as C
import math
import os
import re
import shutil
import subprocess

import numpy as np

import pitch_ref as PR
import pitchfeat_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "asr-featext-opencl_amd", "csrc")
NAMES = ("mfx_batch_set_pitch_feats", "mfx_batch_clear_pitch_feats", "mfx_batch_pitch_feats_read", "mfx_batch_pitch_feats_device",
         "mfx_host_pitch_feats")


def test_symbols_are_declared_and_exported(pkg):
    L = pkg.load_library()
    header = open(os.path.join(ROOT, "include", "mfx.h")).read()
    for name in NAMES:
        assert name in pkg.mfcc.EXPORTED_SYMBOLS and hasattr(L, name)
        assert re.search(r"^int %s\(" % name, header, re.M), name
    assert L.mfx_abi_version() == 2
    assert re.search(r"enum \{ MFX_PF_POV = 1, MFX_PF_NORM_LOG_PITCH = 2, MFX_PF_DELTA = 4, MFX_PF_RAW_LOG_PITCH = 8 \};", header)
    assert (pkg.PF_POV, pkg.PF_NORM_LOG_PITCH, pkg.PF_DELTA, pkg.PF_RAW_LOG_PITCH) == (1, 2, 4, 8)
    assert len(L.mfx_batch_set_pitch_feats.argtypes) == 10 and len(L.mfx_host_pitch_feats.argtypes) == 12
    for name in ("batch_set_pitch_feats", "batch_clear_pitch_feats", "batch_pitch_feats_read", "batch_pitch_feats_device",
                 "host_pitch_feats"):
        assert callable(getattr(pkg.MfccHip, name))
    assert callable(pkg.host_pitch_feats)
    assert "delta-pitch-noise-stddev" in header                     # what is not served is said where the entry is declared


def test_a_planning_handle_answers_err_device(pkg):
    L = pkg.load_library()
    cfg = pkg.MfxConfig()
    for k, v in dict(input_buffer_size=16000, window_size=400, shift=160, num_banks=40, sample_rate=16000.0, low_freq=64.0,
                     high_freq=8000.0, ceps_len=12, want_c0=1, lift_coef=22.0, norm=0, dyn=2, delta_l1=3, delta_l2=3,
                     norm_after_dyn=1).items():
        setattr(cfg, k, v)
    h = C.c_void_p()
    assert L.mfx_plan_create(C.byref(cfg), C.byref(h)) == 0
    try:
        assert L.mfx_batch_set_pitch_feats(h, 0, 75, 75, 2, 2.0, 0.0, 2.0, 10.0, 1) == -6
        assert L.mfx_batch_set_pitch_feats(h, 99, -1, 5000, 0, float("nan"), 0.0, 2.0, 10.0, 7) == -6   # (before any argument is looked at)
        assert L.mfx_batch_clear_pitch_feats(h) == -6
        assert L.mfx_batch_pitch_feats_read(h, None) == -6
        assert L.mfx_batch_pitch_feats_device(h, None, None) == -6
        assert L.mfx_batch_set_pitch_feats(None, 0, 75, 75, 2, 2.0, 0.0, 2.0, 10.0, 0) == -7
        assert L.mfx_batch_clear_pitch_feats(None) == -7 and L.mfx_batch_pitch_feats_read(None, None) == -7
        assert L.mfx_batch_pitch_feats_device(None, None, None) == -7
    finally:
        L.mfx_destroy(h)


def test_every_limit_is_refused_through_the_host_entry(pkg):
    L = pkg.load_library()
    track = np.tile(np.array([[57.5, 0.5]], np.float32), (10, 1))
    canary = np.full(64, 5.0, np.float32)
    fp = C.POINTER(C.c_float)

    def call(T=10, rate=16000.0, columns=0, left=75, right=75, D=2, ps=2.0, po=0.0, ts=2.0, ds=10.0):
        return L.mfx_host_pitch_feats(track.ctypes.data_as(fp), T, rate, columns, left, right, D, ps, po, ts, ds, canary.ctypes.data_as(fp))

    bad = [dict(columns=16), dict(columns=-1), dict(columns=32), dict(left=-1), dict(left=1025), dict(right=-1), dict(right=1025),
           dict(D=0), dict(D=17), dict(D=-1), dict(ps=np.inf), dict(ps=np.nan), dict(po=-np.inf), dict(po=np.nan), dict(ts=np.inf),
           dict(ts=np.nan), dict(ds=np.inf), dict(ds=np.nan), dict(T=-1), dict(rate=0.0), dict(rate=-16000.0), dict(rate=np.nan),
           dict(rate=np.inf)]
    for k in bad:
        assert call(**k) == -7, k
        assert (canary == 5.0).all(), k
    ok = [dict(), dict(columns=15), dict(columns=8), dict(left=0, right=0), dict(left=1024, right=1024), dict(D=1), dict(D=16),
          dict(ps=-3.0, po=1e30, ts=0.0, ds=-1.0), dict(T=0), dict(T=1)]
    for k in ok:
        canary[:] = 5.0
        assert call(**k) == 0, k
        n = k.get("T", 10) * R.n_columns(k.get("columns", 0))
        assert (canary[:n] != 5.0).all() and (canary[n:] == 5.0).all(), k      # T * F floats, and nothing behind them
    assert L.mfx_host_pitch_feats(None, 3, 16000.0, 0, 75, 75, 2, 2.0, 0.0, 2.0, 10.0, canary.ctypes.data_as(fp)) == -7
    assert L.mfx_host_pitch_feats(track.ctypes.data_as(fp), 3, 16000.0, 0, 75, 75, 2, 2.0, 0.0, 2.0, 10.0, None) == -7


def test_host_stays_within_the_bound_on_every_input_of_the_gpu_tests(pkg):
    """The tracks are mfx_host_pitch's (the device's are the same bits: tests/test_pitch_gpu.py), the settings
    pitchfeat_ref.SETTINGS."""
    pcm, offs, lens, utts = R.ragged()
    worst, same, n = 0.0, 0.0, 0
    k = R.TRACK
    for u, f in zip(utts, R.FRAMES):
        T = PR.frame_count(u.size, 400, 160)
        assert T == f
        lag, rho, idx, nccf = pkg.host_pitch(u, T, k["shift"], k["window"], k["lag_min"], k["lag_max"], 0.0, k["lag_cost"], k["penalty"],
                                             k["max_jump"])
        for s in R.SETTINGS:
            got = pkg.host_pitch_feats(lag, rho, 16000.0, columns=s["columns"], left=s["left"], right=s["right"], delta_window=s["D"])
            w, sm = R.check(got, lag, rho, 16000.0, what="%d frames, %s" % (f, s), **s)
            worst, same, n = max(worst, w), same + sm * got.size, n + got.size
    print("worst err / B over the GPU inputs: %.4f; %.2f %% of %d values are the reference's bits" % (worst, 100.0 * same / n, n))
    assert n > 20000


def test_a_constant_track_has_no_delta_and_no_normalised_pitch(pkg):
    T = 400
    lag = np.full(T, 61.75, np.float32)
    rho = (0.05 + 0.9 * np.random.default_rng(5).random(T)).astype(np.float32)      # any weights: the mean of a constant
    got = pkg.host_pitch_feats(lag, rho, 16000.0, columns=15)
    ref, A = R.feats_ref(lag, rho, 16000.0, columns=15)
    assert (got[:, 2] == 0.0).all()
    assert (np.abs(got[:, 1].astype(np.float64)) <= A[:, 1]).all() and A[:, 1].max() < 1e-11
    assert (got[:, 3] == np.float32(math.log(16000.0 / 61.75))).all()


def test_a_linear_ramp_of_log_pitch_gives_delta_scale_times_the_slope(pkg):
    T, D, slope, ds = 120, 3, -0.004, 10.0
    lag = (16000.0 / np.exp(5.0 + slope * np.arange(T))).astype(np.float32)
    p = np.log(16000.0 / lag.astype(np.float64))                       # (the ramp as the float32 lags hold it)
    got = pkg.host_pitch_feats(lag, np.full(T, 0.7, np.float32), 16000.0, columns=R.DELTA, delta_window=D, delta_scale=ds)[:, 0]
    inner = slice(D, T - D)
    # the regression of an exact ramp is its slope; a float32 lag moves its p by at most 2^-24, a difference by 2^-23, and
    # sum l 2^-23 / (2 sum l^2) <= 2^-24; then the one rounding of the output
    assert np.abs(got[inner] - ds * slope).max() <= ds * 2.0 ** -24 + 2.0 ** -24 * abs(ds * slope) + 1e-12
    assert np.abs(np.diff(p) - slope).max() < 2.0 ** -22
    assert abs(got[0]) < abs(ds * slope) and abs(got[-1]) < abs(ds * slope)      # edges replicated: a smaller numerator


def test_pov_is_finite_at_and_beyond_the_ends_of_rho(pkg):
    rho = np.array([1.0, -1.0, 0.0, np.nextafter(np.float32(1), np.float32(2)), 1.5, -1.5, -np.nextafter(np.float32(1), np.float32(2)),
                    1e30, -1e30], np.float32)
    lag = np.full(rho.size, 80.0, np.float32)
    got = pkg.host_pitch_feats(lag, rho, 16000.0, columns=15)
    assert np.isfinite(got).all()
    pov = got[:, 0].astype(np.float64)
    hi, lo, mid = 2.0 * (0.0001 ** 0.15 - 1.0), 2.0 * (2.0001 ** 0.15 - 1.0), 2.0 * (1.0001 ** 0.15 - 1.0)
    want = np.array([hi, lo, mid, hi, hi, lo, lo, hi, lo])
    assert np.abs(pov - want).max() <= 2.0 ** -23                   # beyond +-1 is +-1
    R.check(got, lag, rho, 16000.0, what="rho at the ends", columns=15)


def test_three_rows_worked_by_hand(pkg):
    """rate 16000, lags 80, 100, 125: p = ln 200, ln 160, ln 128.  left = 1, right = 0, D = 1, scales 1, 0, 1, 1.
    rho = 0 for every row: a = 0, r = -5.2 + 5.4 e^-7.5 + 0 - 2 + 4.2 e^-20, one w for all, which cancels in the mean.
    POV = 1.0001^0.15 - 1.   NORM: row 0 alone -> 0; row 1 -> p1 - (p0 + p1) / 2 = ln(160 / 200) / 2; row 2 -> ln(128 / 160) / 2.
    DELTA, den = 2: row 0 (p1 - p0) / 2, row 1 (p2 - p0) / 2, row 2 (p2 - p1) / 2.  RAW = p."""
    lag, rho = np.array([80.0, 100.0, 125.0], np.float32), np.zeros(3, np.float32)
    got = pkg.host_pitch_feats(lag, rho, 16000.0, columns=15, left=1, right=0, delta_window=1, pov_scale=1.0, pov_offset=0.0,
                               pitch_scale=1.0, delta_scale=1.0).astype(np.float64)
    p = [math.log(200.0), math.log(160.0), math.log(128.0)]
    want = np.array([[1.0001 ** 0.15 - 1.0, 0.0, (p[1] - p[0]) / 2, p[0]],
                     [1.0001 ** 0.15 - 1.0, math.log(0.8) / 2, (p[2] - p[0]) / 2, p[1]],
                     [1.0001 ** 0.15 - 1.0, math.log(0.8) / 2, (p[2] - p[1]) / 2, p[2]]])
    assert np.abs(got - want).max() <= 2.0 ** -24 * 5.3 + 1e-14
    r = -5.2 + 5.4 * math.exp(-7.5) - 2.0 + 4.2 * math.exp(-20.0)
    assert abs(R.weights(rho)[1][0] - 1.0 / (1.0 + math.exp(-r))) < 1e-15      # (the reference's w is NccfToPov(0))


def test_kernels_build_for_gfx950_without_private_memory():
    hipcc = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    assert os.path.exists(hipcc), "hipcc (the compiler build() uses) was not found"
    r = subprocess.run([hipcc, "-O3", "-fPIC", "-std=c++17", "--offload-arch=gfx950", "-fno-slp-vectorize",
                        "-Rpass-analysis=kernel-resource-usage", "-c", "mfx_pitchfeat.hip", "-o", os.devnull],
                       cwd=CSRC, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-2000:]
    names = re.findall(r"Function Name: (\S+)", r.stdout)
    scratch = [int(v) for v in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stdout)]
    lds = [int(v) for v in re.findall(r"LDS Size \[bytes/block\]: (\d+)", r.stdout)]
    assert len(scratch) == len(names) == 2, names
    for k in ("k_pitch_feats", "k_pitch_paste"):
        assert sum(k in n for n in names) == 1, (k, names)
    assert all(v == 0 for v in scratch), dict(zip(names, scratch))
    assert sorted(lds) == [0, (256 + 2048) * 16], dict(zip(names, lds))
    assert "mfx_pitchfeat" in open(os.path.join(CSRC, "Makefile")).read().split("KERNEL_TUS :=")[1].split("\n")[0]


def test_host_driver_runs_clean_under_the_sanitizers(tmp_path):
    """tools/asan/pitchfeat_asan.cpp (the tile layout, the limits and host_pitch_feats of mfx_tables.cpp) as `make asan` builds
    and runs it: a stand-alone CPU program under AddressSanitizer + UBSan, linked against mfx_tables.cpp alone."""
    gxx = shutil.which("g++")
    assert gxx, "g++ was not found"
    exe = str(tmp_path / "pitchfeat_asan")
    r = subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-ffp-contract=off", "-o", exe,
                        os.path.join(ROOT, "tools", "asan", "pitchfeat_asan.cpp"), os.path.join(CSRC, "mfx_tables.cpp")],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-2000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env)
    assert r.returncode == 0 and "pitch features clean" in r.stdout, r.stdout[-2000:]
    assert "pitchfeat_asan" in open(os.path.join(CSRC, "Makefile")).read()


def test_driver_refuses_pitch_without_batches_and_on_logmel(tmp_path):
    exe = os.path.join(ROOT, "asr-featext-opencl_amd", "host", "afet_hip")
    assert os.path.exists(exe), "afet_hip is built by build()"
    wav = os.path.join(ROOT, "tests", "golden", "a0001.wav")
    for extra, word in ((["--batch-mb", "0"], "--batch-mb"), (["--method", "LOGMEL"], "LOGMEL"), (["--pitch-range", "400:100"], "LO:HI")):
        r = subprocess.run([exe, "--pitch", *extra, wav, str(tmp_path / "o.txt")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                           text=True, timeout=60)
        assert r.returncode == 2 and "--pitch" in r.stdout and word in r.stdout, r.stdout[-500:]
        assert not (tmp_path / "o.txt").exists()
