"""Session sample-rate conversion (mfx_sessions_set_rates) on the CPU: the new symbols, the planner's step
(mfx_host_session_resample_step) against a brute-force count from the definition, its argument checks, what a planning handle
answers, and the new translation unit's resource usage when compiled for gfx950 (no GPU)."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "asr-featext-opencl_amd", "csrc")
SR = 16000
RATES = (48000, 8000, 44100, 11025, 17600, 12345)

NEW = ("mfx_sessions_set_rates", "mfx_sessions_clear_rates", "mfx_sessions_select_rate", "mfx_sessions_converted_read",
       "mfx_host_session_resample_step")


def test_symbols_are_declared_exported_and_bound(pkg):
    L = pkg.load_library()
    header = open(os.path.join(ROOT, "include", "mfx.h")).read()
    for name in NEW:
        assert name in pkg.mfcc.EXPORTED_SYMBOLS and hasattr(L, name)
        assert re.search(r"\b%s\(" % name, header), name
    assert L.mfx_abi_version() == 2
    for name in ("sessions_set_rates", "sessions_clear_rates", "sessions_select_rate", "sessions_converted_read",
                 "host_session_resample_step"):
        assert hasattr(pkg.MfccHip, name)


def _shape(pkg, r):
    h, L, M, P = pkg.mfcc.host_resample_taps(r, SR)
    return L, M, P // 2, P


@pytest.mark.parametrize("r", RATES)
def test_open_stream_rule_equals_the_brute_force_count(pkg, r):
    """The check the delivery rule rests on, restated: the outputs j whose last tap (j M) div L + Wh has arrived number
    max(0, ceil((N - Wh) L / M)), and the input samples still needed afterwards, [max(0, (J M) div L - Wh + 1), N), number at
    most 2 Wh + M div L + 1 -- for every N up to 3 P + 5 (M div L) + 40."""
    L, M, Wh, P = _shape(pkg, r)
    top = 3 * P + 5 * (M // L) + 40
    j = np.arange((top * L) // M + 4, dtype=np.int64)
    last = (j * M) // L + Wh
    for N in range(top + 1):
        count = int(np.count_nonzero(last <= N - 1))
        J = max(0, -(-(N - Wh) * L // M))
        assert count == J, (r, N)
        need = N - max(0, (J * M) // L - Wh + 1)
        assert 0 <= need <= 2 * Wh + M // L + 1, (r, N, need)


def _cuts(n, Wh, rng, flush):
    """Piece lengths of a stream of n input samples: empty pushes, single samples, Wh - 1 and Wh samples, short and long
    pieces; the end either as a zero-sample final push (the flush) or inside the last piece."""
    out, left = [], n
    special = [0, 1, Wh - 1, Wh]
    while left > 0:
        k = int(rng.integers(0, 8))
        c = special[k] if k < 4 else int(rng.integers(1, 3 * Wh + 50))
        c = min(c, left)
        out.append(c)
        left -= c
    fins = [False] * len(out)
    if flush or not out:
        out.append(0), fins.append(True)
    else:
        fins[-1] = True
    return list(zip(out, fins))


@pytest.mark.parametrize("r", RATES + (SR,))
def test_step_follows_the_rule_however_the_stream_is_cut(pkg, r):
    rng = np.random.default_rng(r)
    passthrough = r == SR
    L, M, Wh, P = (1, 1, 0, 0) if passthrough else _shape(pkg, r)
    bound = 0 if passthrough else 2 * Wh + M // L + 1
    for trial in range(40):
        n = int(rng.integers(0, 6 * max(Wh, 4) + 300)) if trial else 0
        state, N, J, carry = (0, 0), 0, 0, 0
        total = 0
        for length, fin in _cuts(n, max(Wh, 2), rng, flush=trial % 2 == 0):
            d = pkg.mfcc.host_session_resample_step(r, SR, state, length, fin)
            N += length
            if passthrough:
                J_new = N
            elif fin:
                J_new = -(-N * L // M)
            else:
                J_new = max(0, -(-(N - Wh) * L // M))
            assert d["n_out"] == J_new - J, (r, n, N, fin)
            assert d["carry_in"] == carry and 0 <= d["carry_out"] <= bound
            if not passthrough and not fin:
                assert d["carry_out"] == N - max(0, (J_new * M) // L - Wh + 1)
            if fin:
                assert d["carry_out"] == 0 and d["state"] == (0, 0)
            else:
                assert d["state"] == (N, J_new)
            total += d["n_out"]
            J, carry, state = J_new, d["carry_out"], d["state"]
        assert N == n and total == (n if passthrough else -(-n * L // M))


def test_bad_arguments_are_refused_and_nothing_is_written(pkg):
    L = pkg.load_library()
    ERR_ARG = -7

    def call(in_hz, out_hz, zeros, rolloff, st, length, with_state=True):
        state = (C.c_int64 * 2)(*st)
        ci, co = C.c_int32(77), C.c_int32(78)
        rc = L.mfx_host_session_resample_step(in_hz, out_hz, zeros, rolloff, state if with_state else None, length, 0,
                                              C.byref(ci), C.byref(co))
        return rc, tuple(state), ci.value, co.value

    for args in ((999, SR, 0, 0.0, (0, 0), 10), (48000, 768001, 0, 0.0, (0, 0), 10), (48000, SR, 65, 0.0, (0, 0), 10),
                 (48000, SR, -1, 0.0, (0, 0), 10), (48000, SR, 0, 1.5, (0, 0), 10), (48000, SR, 0, -0.1, (0, 0), 10),
                 (48000, SR, 0, 0.0, (0, 0), -1), (48000, SR, 0, 0.0, (-1, 0), 1), (48000, SR, 0, 0.0, (0, -1), 1),
                 (48000, SR, 0, 0.0, (30, 11), 1),            # J beyond ceil(N L / M)
                 (1001, 768000, 0, 0.0, (0, 0), 1)):          # L > 4096
        rc, st, ci, co = call(*args)
        assert rc == ERR_ARG, args
        assert st == tuple(args[4]) and (ci, co) == (77, 78), args
    assert call(48000, SR, 0, 0.0, (0, 0), 1, with_state=False)[0] == ERR_ARG
    rc, st, ci, co = call(48000, SR, 0, 0.0, (0, 0), 300)
    assert rc >= 0 and st[0] == 300


def test_a_planning_handle_answers_err_device(pkg):
    L = pkg.load_library()
    cfg = pkg.MfxConfig()
    for k, v in dict(input_buffer_size=16000, window_size=400, shift=160, num_banks=40, sample_rate=16000.0, low_freq=64.0,
                     high_freq=8000.0, ceps_len=13, want_c0=0, lift_coef=22.0, norm=0, dyn=2, delta_l1=3, delta_l2=3,
                     norm_after_dyn=1).items():
        setattr(cfg, k, v)
    h = C.c_void_p()
    assert L.mfx_plan_create(C.byref(cfg), C.byref(h)) == 0
    try:
        rates = (C.c_int32 * 2)(48000, 8000)
        assert L.mfx_sessions_set_rates(h, 2, rates, 0, 0.0) == -6
        assert L.mfx_sessions_set_rates(h, 99, None, -5, 7.0) == -6           # before any argument is looked at
        assert L.mfx_sessions_clear_rates(h) == -6
        assert L.mfx_sessions_select_rate(h, -3, 99) == -6
        assert L.mfx_sessions_converted_read(h, None, -1, None, None) == -6
    finally:
        L.mfx_destroy(h)


def test_kernel_builds_for_gfx950_without_private_memory():
    """Both instantiations of k_sess_resample compiled for gfx950 as the Makefile compiles them: no scratch."""
    hipcc = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    assert os.path.exists(hipcc), "hipcc (the compiler build() uses) was not found"
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"^KERNEL_TUS :=.*\bmfx_sess_resample\b", mk, re.M)
    r = subprocess.run([hipcc, "-O3", "-fPIC", "-std=c++17", "--offload-arch=gfx950", "-fno-slp-vectorize",
                        "-Rpass-analysis=kernel-resource-usage", "-c", "mfx_sess_resample.hip", "-o", os.devnull],
                       cwd=CSRC, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-2000:]
    names = re.findall(r"Function Name: (\S+)", r.stdout)
    scratch = [int(v) for v in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stdout)]
    kernels = [n for n in names if "k_sess_resample" in n]
    assert len(kernels) == 2 and len(scratch) == len(names)
    assert all(s == 0 for s in scratch), list(zip(names, scratch))
