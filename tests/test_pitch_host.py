"""Pitch track of the batch entries (mfx_batch_set_pitch) on the CPU: the declared and exported symbols, what a planning
handle answers, the host restatement mfx_host_pitch against the float64 NCCF oracle and its bound (pitch_ref.py) on the inputs
the GPU tests use, its track against the float32 numpy restatement bit for bit, a track worked out by hand, the synthetic
glide on which the per-frame argmax makes octave errors and the path does not, every refusal, the new translation unit's
resource usage when compiled for gfx950, and the sanitizer run of the host code (no GPU)."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np

import pitch_ref as PR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "asr-featext-opencl_amd", "csrc")
NAMES = ("mfx_batch_set_pitch", "mfx_batch_clear_pitch", "mfx_batch_pitch_read", "mfx_batch_pitch_device", "mfx_host_pitch")
D = PR.DEFAULT


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def test_symbols_are_declared_and_exported(pkg):
    L = pkg.load_library()
    header = open(os.path.join(ROOT, "include", "mfx.h")).read()
    for name in NAMES:
        assert name in pkg.mfcc.EXPORTED_SYMBOLS and hasattr(L, name)
        assert re.search(r"^int %s\(" % name, header, re.M), name
    assert L.mfx_abi_version() == 2
    assert len(L.mfx_batch_set_pitch.argtypes) == 8 and len(L.mfx_batch_pitch_read.argtypes) == 4
    assert len(L.mfx_host_pitch.argtypes) == 15
    for name in ("batch_set_pitch", "batch_clear_pitch", "batch_pitch_read", "batch_pitch_device", "host_pitch"):
        assert callable(getattr(pkg.MfccHip, name))
    assert callable(pkg.host_pitch)


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
        assert L.mfx_batch_set_pitch(h, 400, 40, 320, 0.0, 0.1, 1.0, 16) == -6
        assert L.mfx_batch_set_pitch(h, 7, 0, 9999, -1.0, 5.0, -1.0, -3) == -6       # (before any argument is looked at)
        assert L.mfx_batch_clear_pitch(h) == -6
        assert L.mfx_batch_pitch_read(h, None, None, None) == -6
        assert L.mfx_batch_pitch_device(h, None, None) == -6
        assert L.mfx_batch_set_pitch(None, 400, 40, 320, 0.0, 0.1, 1.0, 16) == -7
        assert L.mfx_batch_clear_pitch(None) == -7 and L.mfx_batch_pitch_read(None, None, None, None) == -7
        assert L.mfx_batch_pitch_device(None, None, None) == -7
    finally:
        L.mfx_destroy(h)


# ---- the inputs of the GPU tests: rho within the bound, the track bit for bit ------------------------------------------------

def gpu_inputs():
    """(name, pcm of one utterance, channels, shift, window, lag_min, lag_max, ballast): what tests/test_pitch_gpu.py runs
    (pitch_ref.SHAPES)."""
    out = []
    for name, c in PR.SHAPES.items():
        for i, u in enumerate(PR.shape_batch(name)[3]):
            out.append(("%s[%d]" % (name, i), u, c.get("channels", 1), c["shift"], c["window"], c["lag_min"], c["lag_max"],
                        c.get("ballast", 0.0)))
    return out


def test_host_rho_stays_within_the_bound_of_float64_and_the_bound_says_something(pkg):
    worst, ordinary = 0.0, []
    for name, u, ch, S, W, l0, l1, bal in gpu_inputs():
        n = u.size // ch
        T = PR.frame_count(n, 400, S)                                # (the handles' window_size, whatever the track's window)
        if T == 0:
            continue
        nccf = pkg.host_pitch(u, T, S, W, l0, l1, bal, 0.1, 1.0, 16, channels=ch)[3]
        r64, B = PR.nccf_ref(PR.downmix(u, ch), T, S, W, l0, l1, bal)
        assert np.isfinite(nccf).all() and np.abs(nccf).max() <= 1.001, name
        err = np.abs(nccf - r64)
        assert (err <= B).all(), "%s: |rho - rho64| exceeds the bound by %.3g" % (name, (err - B).max())
        ratio = np.where(B > 0, err / np.where(B > 0, B, 1.0), 0.0)   # (B = 0: an exact frame, silence over a ballast)
        print("%-16s T %4d  worst err %.3g  worst err / B %.4f  median B %.3g  capped %d of %d" % (
            name, T, err.max(), ratio.max(), np.median(B), int((B >= 2.01).sum()), B.size))
        worst = max(worst, float(ratio.max()))
        if name.startswith("ragged") and n >= 10000:
            # frames whose span lies inside the utterance: ordinary signal, nothing zero-filled
            full = [t for t in range(T) if t * S + W + l1 <= n]
            ordinary.append(B[full])
    print("worst err / B over the GPU inputs: %.4f" % worst)
    # B against 1, the size of rho: on ordinary frames the bound is five decimal orders below it, and never the cap
    allb = np.concatenate([b.reshape(-1) for b in ordinary])
    assert allb.size > 10000 and allb.max() < 1e-3 and np.median(allb) < 5e-5


def test_host_track_equals_the_numpy_restatement_on_its_own_rho(pkg):
    for name, u, ch, S, W, l0, l1, bal in gpu_inputs():
        T = PR.frame_count(u.size // ch, 400, S)
        K = l1 - l0 + 1
        for lc, pen, mj in ((0.1, 1.0, 16), (0.0, 0.25, 1), (0.3, 4.0, 0)):
            if name.startswith("k512") and mj != 16:
                continue
            lag, rho, idx, nccf = pkg.host_pitch(u, T, S, W, l0, l1, bal, lc, pen, mj, channels=ch)
            l2, r2, i2 = PR.track_ref(nccf.reshape(T, K), l0, l1, lc, pen, mj)
            assert np.array_equal(i2, idx) and np.array_equal(bits(l2), bits(lag)) and np.array_equal(bits(r2), bits(rho)), (name, lc, pen, mj)


def test_track_on_a_hand_worked_case():
    """K = 3 (lags 2, 3, 4), 4 frames, lag_cost 0 (wt = 1), penalty 0 (every transition free), J = 2.
    loc = 1 - rho:  t0 (.5, .5, 1)  t1 (1, .25, .25)  t2 (1, 1, .5)  t3 (.5, .75, .5): all exact in float32.
    t0: a = loc, min .5 (state 0 before state 1) -> fwd (0, 0, .5).
    t1: every state takes fwd 0 from state 0, the smaller of the tied predecessors 0 and 1 -> a (1, .25, .25), fwd (.75, 0, 0).
    t2: best is fwd 0 from state 1 (tied with 2) -> a (1, 1, .5), fwd (.5, .5, 0).   t3: from state 2 -> a (.5, .75, .5).
    End state: states 0 and 2 tie at the minimum, the smaller wins: 0.  Back: bp_3[0] = 2, bp_2[2] = 1, bp_1[1] = 0.
    Path 0, 1, 2, 0.  Refinement only at interior states: t1 is state 1 with rho (0, .75, .75): den = -.75 < 0,
    delta = (.5 * (0 - .75)) / -.75 = .5 -> lag 3.5."""
    rho = np.array([[.5, .5, 0], [0, .75, .75], [0, 0, .5], [.5, .25, .5]], np.float32)
    lag, r, idx = PR.track_ref(rho, 2, 4, 0.0, 0.0, 0)
    assert idx.tolist() == [0, 1, 2, 0]
    assert r.tolist() == [.5, .75, .5, .5]
    assert lag.tolist() == [2.0, 3.5, 4.0, 2.0]
    # with J = 1 state 2 cannot be reached from state 0 at t1, nor state 0 from state 2 at t3
    lag1, r1, idx1 = PR.track_ref(rho, 2, 4, 0.0, 0.0, 1)
    assert idx1.tolist() == [0, 1, 2, 2] and lag1.tolist() == [2.0, 3.5, 4.0, 4.0]
    # a transition cost keeps the path where it is: penalty 100 on (ln l - ln l')^2 >= 100 * ln(4/3)^2 = 8.3 per step
    assert len(set(PR.track_ref(rho, 2, 4, 0.0, 100.0, 0)[2].tolist())) == 1
    # T = 0 and K = 1
    assert PR.track_ref(np.zeros((0, 3), np.float32), 2, 4, 0.1, 1.0, 0)[2].size == 0
    one = PR.track_ref(np.array([[.25], [.5]], np.float32), 7, 7, 0.1, 1.0, 0)
    assert one[2].tolist() == [0, 0] and one[0].tolist() == [7.0, 7.0] and one[1].tolist() == [.25, .5]


def test_the_path_follows_a_glide_on_which_the_per_frame_argmax_makes_octave_errors(pkg):
    pcm, f0 = PR.glide()
    W, S, l0, l1 = D["window"], D["shift"], D["lag_min"], D["lag_max"]
    T = PR.frame_count(pcm.size, W, S)
    for mj in (16, 0):
        lag, rho, idx, nccf = pkg.host_pitch(pcm, T, S, W, l0, l1, 0.0, 0.1, 1.0, mj)
        # the frame compares samples j and j + lag, j < W: it is centred (W + lag) / 2 behind its first sample
        at = np.clip((np.arange(T) * S + (W + lag) / 2).astype(int), 0, pcm.size - 1)
        err = np.abs(16000.0 / lag - f0[at]) / f0[at]
        assert err.max() <= 0.02, "path: worst relative f0 error %.4f at frame %d" % (err.max(), err.argmax())
        arg = nccf.argmax(axis=1) + l0
        worst = (np.abs(16000.0 / arg - f0[at]) / f0[at]).max()
        assert worst > 0.3, "the per-frame argmax never leaves the track (worst %.3f): the case shows nothing" % worst


def test_every_limit_is_refused_through_the_host_entry(pkg):
    L = pkg.load_library()
    pcm = PR.voiced(3000, 3)
    canary = np.full(32, 5.0, np.float32)                            # pitch [T][2] of the calls below, T <= 10, and room behind it
    fp = C.POINTER(C.c_float)

    def call(n=3000, ch=1, T=10, S=160, W=400, l0=40, l1=320, bal=0.0, lc=0.1, pen=1.0, mj=16):
        return L.mfx_host_pitch(pcm.ctypes.data_as(C.POINTER(C.c_int16)), n, ch, T, S, W, l0, l1, bal, lc, pen, mj,
                                canary.ctypes.data_as(fp), None, None)

    bad = [dict(W=31), dict(W=1025), dict(W=0), dict(l0=1), dict(l0=0), dict(l1=1025), dict(l0=41, l1=40), dict(l0=2, l1=514),
           dict(bal=-1e-9), dict(bal=np.inf), dict(bal=np.nan), dict(lc=-0.01), dict(lc=1.01), dict(lc=np.nan), dict(lc=np.inf),
           dict(pen=-1.0), dict(pen=np.inf), dict(pen=np.nan), dict(mj=-1), dict(mj=512), dict(ch=0), dict(ch=3), dict(T=-1),
           dict(S=0), dict(n=-1)]
    for k in bad:
        assert call(**k) == -7, k
        assert (canary == 5.0).all(), k
    # on the limits it runs: window 32 and 1024, lags 2 and 1024, K = 1 and 512, lag_cost 0 and 1, max_jump 0 and 511
    ok = [dict(W=32, T=2), dict(W=1024, T=2, l0=513, l1=1024), dict(l0=2, l1=2), dict(l0=2, l1=513, T=2), dict(l0=1024, l1=1024, T=1),
          dict(lc=0.0, pen=0.0), dict(lc=1.0), dict(mj=0), dict(mj=511), dict(T=0)]
    for k in ok:
        canary[:] = 5.0
        assert call(**k) == 0, k
        T = k.get("T", 10)
        assert (canary[:2] != 5.0).any() or T == 0, k
        assert (canary[2 * T:] == 5.0).all(), k                      # nothing behind the T rows is written
    assert L.mfx_host_pitch(None, 10, 1, 1, 160, 400, 40, 320, 0.0, 0.1, 1.0, 16, None, None, None) == -7   # samples without an array


def test_clamped_jump_is_the_full_jump(pkg):
    """max_jump above K - 1 is clamped to it, 0 means it: the same track."""
    u = PR.voiced(4000, 11)
    T = PR.frame_count(u.size, 400, 160)
    a = pkg.host_pitch(u, T, 160, 400, 40, 76, 0.0, 0.1, 1.0, 0)
    for mj in (36, 100, 511):
        b = pkg.host_pitch(u, T, 160, 400, 40, 76, 0.0, 0.1, 1.0, mj)
        assert np.array_equal(a[2], b[2]) and np.array_equal(bits(a[0]), bits(b[0]))


def test_kernels_build_for_gfx950_without_private_memory():
    hipcc = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    assert os.path.exists(hipcc), "hipcc (the compiler build() uses) was not found"
    r = subprocess.run([hipcc, "-O3", "-fPIC", "-std=c++17", "--offload-arch=gfx950", "-fno-slp-vectorize",
                        "-Rpass-analysis=kernel-resource-usage", "-c", "mfx_pitch.hip", "-o", os.devnull],
                       cwd=CSRC, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-2000:]
    names = re.findall(r"Function Name: (\S+)", r.stdout)
    scratch = [int(v) for v in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stdout)]
    assert len(scratch) == len(names) == 2, names
    for k in ("k_pitch_nccf", "k_pitch_track"):
        assert sum(k in n for n in names) == 1, (k, names)
    assert all(v == 0 for v in scratch), dict(zip(names, scratch))


def test_host_driver_runs_clean_under_the_sanitizers(tmp_path):
    """tools/asan/pitch_asan.cpp (the tile layout, the padded span and host_pitch of mfx_tables.cpp) as `make asan` builds and
    runs it: a stand-alone CPU program under AddressSanitizer + UBSan."""
    gxx = shutil.which("g++")
    assert gxx, "g++ was not found"
    exe = str(tmp_path / "pitch_asan")
    r = subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-ffp-contract=off", "-o", exe,
                        os.path.join(ROOT, "tools", "asan", "pitch_asan.cpp"), os.path.join(CSRC, "mfx_tables.cpp")],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-2000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env)
    assert r.returncode == 0 and "tracks clean" in r.stdout, r.stdout[-2000:]
