"""Energy VAD and voiced-frame selection (mfx_batch_set_vad) on the CPU: the declared and exported symbols, the numpy
restatement (vad_ref.py) against a case worked out by hand, what a planning handle answers, the new translation unit's
resource usage when compiled for gfx950, and the sanitizer run of the host layout (no GPU)."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np

import vad_ref as VR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "asr-featext-opencl_amd", "csrc")
NAMES = ("mfx_batch_set_vad", "mfx_batch_clear_vad", "mfx_batch_vad_read", "mfx_batch_vad_device")


def test_symbols_are_declared_and_exported(pkg):
    L = pkg.load_library()
    header = open(os.path.join(ROOT, "include", "mfx.h")).read()
    for name in NAMES:
        assert name in pkg.mfcc.EXPORTED_SYMBOLS and hasattr(L, name)
        assert re.search(r"^int %s\(" % name, header, re.M), name
    assert re.search(r"enum \{ MFX_VAD_FLAGS = 0, MFX_VAD_SELECT = 1, MFX_VAD_PACK = 2 \};", header)
    assert (pkg.VAD_FLAGS, pkg.VAD_SELECT, pkg.VAD_PACK) == (0, 1, 2)
    assert L.mfx_abi_version() == 2
    for name in ("batch_set_vad", "batch_clear_vad", "batch_vad_read"):
        assert callable(getattr(pkg.MfccHip, name))


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
        assert L.mfx_batch_set_vad(h, -1, 0.0, 1.0, 2, 0.6, 0) == -6
        assert L.mfx_batch_set_vad(h, 99, 0.0, 1.0, 2, 0.6, 7) == -6          # (before any argument is looked at)
        assert L.mfx_batch_clear_vad(h) == -6
        assert L.mfx_batch_vad_read(h, None, None, None, None) == -6
        assert L.mfx_batch_vad_device(h, None, None, None) == -6
        assert L.mfx_batch_set_vad(None, -1, 0.0, 1.0, 2, 0.6, 0) == -7
    finally:
        L.mfx_destroy(h)


def test_reference_on_a_hand_written_case():
    # six frames; the mean is 3, so with et = 0, ms = 1 frames 3 and 5 (values 7 and 6) are loud, frame 4 (a NaN later) not
    e = np.array([1, 2, 0, 7, 2, 6], np.float32)
    thr, bound = VR.thr_ref(e, 0.0, 1.0)
    assert thr == 3.0 and 0 < bound < 1e-6
    assert VR.flags_ref(e, thr, 0, 0.5).tolist() == [0, 0, 0, 1, 0, 1]
    # ctx 1, p = 0.5: windows cut at the ends -- t = 0: {0, 1} 0 of 2; t = 2: {1, 2, 3} 1 of 3 (1 >= 1.5 fails);
    # t = 3: 1 of 3; t = 4: {3, 4, 5} 2 of 3; t = 5: {4, 5} 1 of 2 (1 >= 1.0 holds)
    assert VR.flags_ref(e, thr, 1, 0.5).tolist() == [0, 0, 0, 0, 1, 1]
    # p = 1: every frame of the window must be loud -- with ctx 0 that is the frame itself; with ctx 1 no window qualifies
    assert VR.flags_ref(e, thr, 0, 1.0).tolist() == [0, 0, 0, 1, 0, 1]
    assert VR.flags_ref(e, thr, 1, 1.0).tolist() == [0, 0, 0, 0, 0, 0]
    # a context wider than the utterance: every window is the whole utterance, 2 loud of 6 for every frame
    assert VR.flags_ref(e, thr, 64, 2 / 6).tolist() == [1] * 6
    assert VR.flags_ref(e, thr, 64, 0.34).tolist() == [0] * 6
    # a NaN frame is not loud, whichever side it is on; a NaN threshold makes no frame loud
    n = e.copy()
    n[5] = np.nan
    assert VR.flags_ref(n, 3.0, 0, 0.5).tolist() == [0, 0, 0, 1, 0, 0]
    assert VR.flags_ref(n, 3.0, 1, 0.5).tolist() == [0, 0, 0, 0, 0, 0]   # t = 4: 1 of 3; t = 5: 0 of 2
    assert VR.flags_ref(e, np.nan, 2, 0.1).tolist() == [0] * 6
    assert np.isnan(VR.thr_ref(n, 0.0, 1.0)[0])
    # T = 1: the frame equals its own mean and is not above it; an offset below it makes it voiced at any context
    one = np.array([4.0], np.float32)
    assert VR.thr_ref(one, 0.0, 1.0)[0] == 4.0 and VR.flags_ref(one, 4.0, 64, 1.0).tolist() == [0]
    thr1, _ = VR.thr_ref(one, -1.0, 0.5)
    assert thr1 == 1.0 and VR.flags_ref(one, thr1, 64, 1.0).tolist() == [1]
    # T = 0
    assert VR.thr_ref(np.zeros(0, np.float32), 2.5, 9.0) == (2.5, 0.0) and VR.flags_ref(np.zeros(0, np.float32), 2.5, 3, 0.5).size == 0


def test_reference_layouts():
    y = np.arange(1, 13, dtype=np.float32).reshape(6, 2)
    rows, frames = [0, 2, 2], [2, 0, 4]
    flags = np.array([0, 1, 1, 0, 0, 1], np.uint8)
    s = VR.select_ref(y, rows, frames, flags)
    assert s.tolist() == [[3, 4], [0, 0], [5, 6], [11, 12], [0, 0], [0, 0]]
    p, row0 = VR.pack_ref(y, rows, frames, flags)
    assert p.tolist() == [[3, 4], [5, 6], [11, 12], [0, 0], [0, 0], [0, 0]] and row0.tolist() == [0, 1, 1, 3]
    assert not np.signbit(s).any() and not np.signbit(p).any()


def test_threshold_bound_covers_other_summation_orders():
    """Any order of the double sum stays inside the bound, and the bound is not vacuous: far below one float32 step of a
    threshold of ordinary size plus that step itself."""
    rng = np.random.default_rng(5)
    e = (40.0 * rng.standard_normal(5000) - 60.0).astype(np.float32)
    thr, bound = VR.thr_ref(e, -31.0, 0.5)
    v = e.astype(np.float64)
    for order in (v[::-1], np.sort(v), v[rng.permutation(v.size)]):
        s = 0.0
        for x in order:
            s += x
        assert abs(np.float64(np.float32(-31.0 + 0.5 * (s / v.size))) - thr) <= bound
    assert bound < 1.01 * 2.0 ** -24 * abs(thr)


def test_kernels_build_for_gfx950_without_private_memory():
    hipcc = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    assert os.path.exists(hipcc), "hipcc (the compiler build() uses) was not found"
    r = subprocess.run([hipcc, "-O3", "-fPIC", "-std=c++17", "--offload-arch=gfx950", "-fno-slp-vectorize",
                        "-Rpass-analysis=kernel-resource-usage", "-c", "mfx_vad.hip", "-o", os.devnull],
                       cwd=CSRC, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-2000:]
    names = re.findall(r"Function Name: (\S+)", r.stdout)
    scratch = [int(v) for v in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stdout)]
    assert len(scratch) == len(names)
    for k in ("k_vad_sums", "k_vad_thresh", "k_vad_flags", "k_vad_scan", "k_vad_pack"):
        assert sum(k in n for n in names) == 1, (k, names)
    assert sum("k_vad_select" in n for n in names) == 2          # 16-byte and word form
    assert all(v == 0 for v in scratch), dict(zip(names, scratch))


def test_layout_driver_runs_clean_under_the_sanitizers(tmp_path):
    """tools/asan/vad_asan.cpp (build_utt_tiling of mfx_tables.cpp at the VAD's two sizes) as `make asan` builds and runs it: a stand-alone CPU
    program under AddressSanitizer + UBSan."""
    gxx = shutil.which("g++")
    assert gxx, "g++ was not found"
    exe = str(tmp_path / "vad_asan")
    r = subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-ffp-contract=off", "-o", exe,
                        os.path.join(ROOT, "tools", "asan", "vad_asan.cpp"), os.path.join(CSRC, "mfx_tables.cpp")],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-2000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env)
    assert r.returncode == 0 and "layouts clean" in r.stdout, r.stdout[-2000:]
