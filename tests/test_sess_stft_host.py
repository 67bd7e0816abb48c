"""Session entries on an STFT log-mel handle, on the CPU: the new symbols, the planner's step against a brute-force Python
restatement of the delivery rule, the LDS sum that decides how many frame groups share a block of k_sess_stft_mel, the
stand-alone sanitizer program, and the kernels' resource usage when compiled for gfx950 (no GPU)."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "asr-featext-opencl_amd", "csrc")
LDS = 160 * 1024
SHAPES = [(400, 160), (512, 512), (32, 1), (512, 1), (400, 400), (400, 199), (400, 201), (64, 24), (32, 17), (34, 33)]

NEW = ("mfx_host_session_stft_step", "mfx_host_sess_stft_lds_bytes")


def test_symbols_are_declared_and_exported(pkg):
    L = pkg.load_library()
    header = open(os.path.join(ROOT, "include", "mfx.h")).read()
    for name in NEW:
        assert name in pkg.mfcc.EXPORTED_SYMBOLS and hasattr(L, name)
        assert re.search(r"\b%s\(" % name, header), name
    assert pkg.mfcc.ENGINE_SESS_STFT_PLAIN == 8192
    assert re.search(r"#define MFX_ENGINE_SESS_STFT_PLAIN 8192\b", header)
    assert L.mfx_abi_version() == 2
    assert hasattr(pkg.MfccHip, "host_session_stft_step") and hasattr(pkg.mfcc, "host_sess_stft_lds_bytes")


def frames(n, N, S):
    return 0 if n <= N // 2 else n // S


def open_rows(n, N, S):
    """Rows an open stream of n samples has delivered, from the definition: frame t counts once its last tap t S + N / 2 - 1
    and sample N / 2 (frame 0's left reflection) have arrived, and no longer stream has fewer frames than t + 1."""
    if n <= N // 2:
        return 0
    E = 0
    while E * S + N // 2 - 1 <= n - 1 and E < n // S:
        E += 1
    return E


def _cuts(n, S, rng, flush):
    out, left = [], n
    while left > 0:
        r = rng.random()
        k = 0 if r < 0.2 else 1 if r < 0.35 else int(rng.integers(1, 2 * S + 3))
        k = min(k, left)
        left -= k
        out.append([k, False])
    if flush or not out:
        out.append([0, True])
    else:
        out[-1][1] = True
    return out


@pytest.mark.parametrize("N,S", SHAPES)
def test_step_against_a_brute_force_rule(pkg, N, S):
    step = pkg.mfcc.host_session_stft_step
    rng = np.random.default_rng(100 * N + S)
    top = 3 * N + 5 * S
    lengths = sorted({0, 1, N // 2, N // 2 + 1, N // 2 + 2, N - 1, N, N + 1, S, S + 1, top} | set(int(v) for v in rng.integers(0, top, 12)))
    for n in lengths:
        for trial in range(3):
            cuts = [[n, True]] if trial == 0 else _cuts(n, S, rng, flush=trial == 1)
            state, got, fed = (0, 0), 0, 0
            for length, fin in cuts:
                E_old = state[1]
                st = step(N, S, state, length, fin)
                fed += length
                E_new = frames(fed, N, S) if fin else open_rows(fed, N, S)
                assert st["rows"] == E_new - E_old >= 0, (n, cuts, fed)           # the rule; E never decreases
                assert E_new <= frames(fed, N, S)
                assert st["state"] == ((0, 0) if fin else (fed, E_new))
                c0 = max(0, E_old * S - N // 2)
                assert st["carry_in"] == fed - length - c0 and 0 <= st["carry_in"] < N + S
                assert st["carry_out"] == (0 if fin else fed - max(0, E_new * S - N // 2)) and st["carry_out"] < N + S
                if length == 0:
                    assert st["rows"] <= N // (2 * S) + 1                          # the flush bound
                for t in range(E_old, E_new):
                    first, last = t * S - N // 2, t * S + N // 2 - 1
                    assert fed > N // 2 and -first < fed                           # the left reflection stays inside the stream
                    if not fin:
                        assert last <= fed - 1                                     # every sample of the frame has arrived
                    lowest = max(first, 0)                                         # (a frame that spans sample 0 reads it)
                    if last >= fed:
                        lowest = min(lowest, 2 * (fed - 1) - last)                 # the right reflection reaches back to here
                    assert c0 <= lowest, (n, cuts, t)                              # ... and lies in the carried range [c0, fed)
                got += st["rows"]
                state = st["state"]
            assert got == frames(n, N, S) and state == (0, 0)


def test_step_refuses_bad_arguments(pkg):
    L = pkg.load_library()
    st = (C.c_int64 * 2)(1000, 6)
    for N, S in ((30, 10), (514, 10), (401, 10), (400, 0), (400, 401)):
        assert L.mfx_host_session_stft_step(N, S, st, 1, 0, None, None) == -7
    assert L.mfx_host_session_stft_step(400, 160, None, 1, 0, None, None) == -7
    assert L.mfx_host_session_stft_step(400, 160, st, -1, 0, None, None) == -7
    bad = (C.c_int64 * 2)(1000, 7)                                 # more rows than the stream has frames
    assert L.mfx_host_session_stft_step(400, 160, bad, 1, 0, None, None) == -7
    low = (C.c_int64 * 2)(1000, 2)                                 # fewer rows than an open stream of 1000 samples has delivered
    assert L.mfx_host_session_stft_step(400, 160, low, 1, 0, None, None) == -7
    assert tuple(st) == (1000, 6) and tuple(bad) == (1000, 7) and tuple(low) == (1000, 2)      # nothing was written
    assert L.mfx_host_session_stft_step(400, 160, st, 600, 0, None, None) == 3 and tuple(st) == (1600, 9)
    g = C.c_int32(3)
    assert L.mfx_host_sess_stft_lds_bytes(400, 160, 80, C.byref(g)) == -7
    assert L.mfx_host_sess_stft_lds_bytes(400, 160, 129, None) == -7


def test_lds_helper_over_the_methods_limits(pkg):
    """Every (N, S) of the method's limits at M in {1, 80, 128}: the packing taken fits 160 KB, twice as many groups would
    not (or it is the full block of four), and one group always fits."""
    L = pkg.load_library()
    f = L.mfx_host_sess_stft_lds_bytes
    seen = set()
    for M in (1, 80, 128):
        for N in range(32, 513, 2):
            for S in range(1, N + 1):
                g = C.c_int32(0)
                b = f(N, S, M, C.byref(g))
                G = g.value
                assert G in (1, 2, 4) and 0 < b <= LDS, (N, S, M, G, b)
                if G < 4:
                    g2 = C.c_int32(2 * G)
                    assert f(N, S, M, C.byref(g2)) > LDS, (N, S, M, G)
                if G > 1:
                    g1 = C.c_int32(1)
                    assert 0 < f(N, S, M, C.byref(g1)) < b
                seen.add(G)
    assert seen == {2, 4}      # (two groups fit every shape of the limits: the largest, 512 / 512 / 128, takes 125 KB)
    assert pkg.mfcc.host_sess_stft_lds_bytes(400, 160, 80) == (26624 + 4 * 11216 + 51456, 4)   # 122 944 bytes
    assert pkg.mfcc.host_sess_stft_lds_bytes(512, 512, 80)[1] == 2
    assert pkg.mfcc.host_sess_stft_lds_bytes(400, 160, 80, 1) == (26624 + 11216 + 51456 // 4, 1)


def test_host_driver_runs_clean_under_the_sanitizers(tmp_path):
    """tools/asan/sess_stft_asan.cpp (session_stft_step and cut_sess_stft_groups of mfx_tables.cpp) as `make asan` builds and
    runs it: a stand-alone CPU program under AddressSanitizer + UBSan, linked against mfx_tables.cpp alone."""
    gxx = shutil.which("g++")
    assert gxx, "g++ was not found"
    exe = str(tmp_path / "sess_stft_asan")
    r = subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-ffp-contract=off", "-o", exe,
                        os.path.join(ROOT, "tools", "asan", "sess_stft_asan.cpp"), os.path.join(CSRC, "mfx_tables.cpp")],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-2000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env)
    assert r.returncode == 0 and "work lists clean" in r.stdout, r.stdout[-2000:]
    assert "sess_stft_asan" in open(os.path.join(CSRC, "Makefile")).read()


def test_kernels_build_for_gfx950_without_private_memory():
    """mfx_stft.hip compiled for gfx950 as the Makefile compiles it: k_sess_stft_mel and k_stft_mel, which share the DFT loop,
    use no scratch and keep two waves per SIMD."""
    hipcc = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    assert os.path.exists(hipcc), "hipcc (the compiler build() uses) was not found"
    r = subprocess.run([hipcc, "-O3", "-fPIC", "-std=c++17", "--offload-arch=gfx950", "-fno-slp-vectorize",
                        "-Rpass-analysis=kernel-resource-usage", "-c", "mfx_stft.hip", "-o", os.devnull],
                       cwd=CSRC, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-2000:]
    names = re.findall(r"Function Name: (\S+)", r.stdout)
    scratch = [int(v) for v in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stdout)]
    occ = [int(v) for v in re.findall(r"Occupancy \[waves/SIMD\]: (\d+)", r.stdout)]
    assert len(scratch) == len(names) == len(occ)
    for kernel in ("k_sess_stft_mel", "k_stft_mel"):
        i = [k for k, n in enumerate(names) if kernel in n]
        assert len(i) == 1, (kernel, names)
        assert scratch[i[0]] == 0 and occ[i[0]] >= 2, (kernel, scratch[i[0]], occ[i[0]])
