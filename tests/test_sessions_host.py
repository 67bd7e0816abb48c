"""Session entries on the CPU: the planner's per-push arithmetic (mfx_host_session_step) against a restatement of the
contract of include/mfx.h, what a planning handle answers, and the new translation unit's resource usage when compiled for
gfx950 (no GPU)."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "asr-featext-opencl_amd", "csrc")

SHAPES = [(400, 160, 0), (400, 160, 2), (400, 160, 6), (200, 80, 4), (1102, 441, 4), (2048, 512, 20)]
MAX_PUSH = 3000


def frames(n, W, S):
    return max(0, (n - W + S) // S)


def contract_step(W, S, D, n, E, length, final):
    """The contract, restated: what one push must deliver and what the planner must derive for it."""
    T_old, f0 = frames(n, W, S), max(0, E - D)
    n_new = n + length
    T_new = frames(n_new, W, S)
    E_new = T_new if final else max(0, T_new - D)
    return dict(rows=E_new - E, n=n_new, E=E_new, carry_samples=n - T_old * S, carry_rows=T_old - f0, new_frames=T_new - T_old,
                n_out=E_new - E, static_off=E - f0, shift=E - f0 - D, lo=0, hi=T_new - 1 - f0)


def push_lengths(rng, W, S, count):
    must = [0, 1, S - 1, S, W - 1, W, MAX_PUSH]
    extra = [int(rng.integers(0, MAX_PUSH + 1)) for _ in range(count)]
    ls = must + extra
    rng.shuffle(ls)
    return ls


@pytest.mark.parametrize("W,S,D", SHAPES)
def test_step_follows_the_contract_over_random_push_sequences(pkg, W, S, D):
    rng = np.random.default_rng(1000 * W + D)
    for trial in range(20):
        ls = push_lengths(rng, W, S, int(rng.integers(0, 12)))
        if trial % 4 == 0:
            ls = ls + [0]                                  # the flush: a final push without samples
        n = E = 0
        delivered = 0
        for k, length in enumerate(ls):
            final = k == len(ls) - 1
            want = contract_step(W, S, D, n, E, length, final)
            got = pkg.host_session_step(W, S, D, (n, E), length, final)
            for key in ("rows", "carry_samples", "carry_rows", "new_frames", "n_out", "static_off", "shift", "lo", "hi"):
                assert got[key] == want[key], (key, trial, k, length, got, want)
            assert 0 <= got["carry_samples"] < W + S
            assert 0 <= got["carry_rows"] <= 2 * D
            assert got["static_off"] - got["shift"] == D
            assert got["rows"] >= 0
            # every row the delta stage reads for the delivered rows lies inside the slot: carried rows + new frames
            if got["n_out"] > 0:
                top = got["n_out"] - 1 + got["static_off"] + D
                assert min(top, got["hi"]) < got["carry_rows"] + got["new_frames"]
                if not final:
                    assert top <= got["hi"]                # the right edge clamps only at the true end
            delivered += got["rows"]
            n, E = want["n"], want["E"]
            assert E == (frames(n, W, S) if final else max(0, frames(n, W, S) - D))
            assert got["state"] == ((0, 0) if final else (n, E))
        assert delivered == frames(sum(ls), W, S)


@pytest.mark.parametrize("W,S,D", [s for s in SHAPES if s[2] > 0])
def test_short_streams_deliver_everything_at_the_final_push(pkg, W, S, D):
    for T in range(0, D + 1):
        total = 0 if T == 0 else W + (T - 1) * S + S // 2
        assert frames(total, W, S) == T
        n = E = 0
        pieces = [total // 3, total - total // 3]
        for length in pieces:
            got = pkg.host_session_step(W, S, D, (n, E), length, False)
            assert got["rows"] == 0
            n, E = got["state"]
        assert (n, E) == (total, 0)
        got = pkg.host_session_step(W, S, D, (n, E), 0, True)
        assert got["rows"] == T and got["state"] == (0, 0)
        if T > 0:
            assert got["hi"] == T - 1 and got["carry_rows"] == T and got["new_frames"] == 0 and got["static_off"] == 0


def test_a_stream_without_a_frame_delivers_nothing(pkg):
    for W, S, D in SHAPES:
        for total in (0, 1, W - 1):
            got = pkg.host_session_step(W, S, D, (0, 0), total, True)
            assert got["rows"] == 0 and got["new_frames"] == 0 and got["state"] == (0, 0)


def test_bad_arguments_are_refused(pkg):
    L = pkg.load_library()
    st = (C.c_int64 * 2)(0, 0)
    assert L.mfx_host_session_step(0, 160, 2, st, 10, 0, None, None, None, None) == -7
    assert L.mfx_host_session_step(400, 0, 2, st, 10, 0, None, None, None, None) == -7
    assert L.mfx_host_session_step(400, 160, -1, st, 10, 0, None, None, None, None) == -7
    assert L.mfx_host_session_step(400, 160, 2, st, -1, 0, None, None, None, None) == -7
    assert L.mfx_host_session_step(400, 160, 2, None, 1, 0, None, None, None, None) == -7
    assert L.mfx_host_session_step(400, 160, 2, st, 560, 1, None, None, None, None) == 2   # every output may be NULL


def test_a_planning_handle_answers_err_device(pkg):
    L = pkg.load_library()
    cfg = pkg.MfxConfig()
    for k, v in dict(input_buffer_size=16000, window_size=400, shift=160, num_banks=26, sample_rate=16000.0, low_freq=64.0,
                     high_freq=8000.0, ceps_len=13, want_c0=0, lift_coef=22.0, norm=0, dyn=2, delta_l1=3, delta_l2=3,
                     norm_after_dyn=1).items():
        setattr(cfg, k, v)
    h = C.c_void_p()
    assert L.mfx_plan_create(C.byref(cfg), C.byref(h)) == 0
    try:
        assert L.mfx_sessions_create(h, 8, 1600) == -6
        assert len(L.mfx_last_error(h)) > 0
        assert L.mfx_sessions_reset(h, -1) == -6
        assert L.mfx_sessions_plan(h, 0, None, None, None, None, None, None, None) == -6
        assert L.mfx_sessions_run_device(h, None, 0, None) == -6
        assert L.mfx_sessions_run_host(h, None, 0, None) == -6
    finally:
        L.mfx_destroy(h)
    assert L.mfx_sessions_create(None, 8, 1600) == -7
    assert L.mfx_sessions_delivered(None, 0) == -7


def test_symbols_are_declared_and_exported(pkg):
    L = pkg.load_library()
    for name in ("mfx_sessions_create", "mfx_sessions_reset", "mfx_sessions_plan", "mfx_sessions_run_device",
                 "mfx_sessions_run_host", "mfx_sessions_delivered", "mfx_host_session_step"):
        assert name in pkg.mfcc.EXPORTED_SYMBOLS and hasattr(L, name)
    assert L.mfx_abi_version() == 2
    for name in ("sessions_create", "sessions_reset", "sessions_plan", "sessions_run_device", "sessions_run_host",
                 "sessions_delivered", "host_session_step"):
        assert hasattr(pkg.MfccHip, name)
    assert callable(pkg.host_session_step)


def test_kernel_builds_for_gfx950_without_private_memory():
    """k_sess_gather compiled for gfx950 as the Makefile compiles it: present in the code object, no scratch, no LDS."""
    hipcc = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    assert os.path.exists(hipcc), "hipcc (the compiler build() uses) was not found"
    r = subprocess.run([hipcc, "-O3", "-fPIC", "-std=c++17", "--offload-arch=gfx950", "-fno-slp-vectorize",
                        "-Rpass-analysis=kernel-resource-usage", "-c", "mfx_sessions.hip", "-o", os.devnull],
                       cwd=CSRC, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-2000:]
    names = re.findall(r"Function Name: (\S+)", r.stdout)
    scratch = [int(v) for v in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stdout)]
    lds = [int(v) for v in re.findall(r"LDS Size \[bytes/block\]: (\d+)", r.stdout)]
    kernels = [n for n in names if "k_sess_gather" in n]
    assert len(kernels) == 1 and len(scratch) == len(names) == len(lds)
    assert all(v == 0 for v in scratch), dict(zip(names, scratch))
    assert all(v == 0 for v in lds), dict(zip(names, lds))
