"""Sample-rate conversion on the CPU: the host builders (tap table, lengths, layout) against the numpy formula of
resample_ref.py, the limits, what a planning handle answers, and the new translation unit's resource usage when compiled
for gfx950 (no GPU)."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import resample_ref as RR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "asr-featext-opencl_amd", "csrc")

PAIRS = [(48000, 16000), (8000, 16000), (44100, 16000), (11025, 16000), (17600, 16000), (16000, 44100)]
ERR_ARG, ERR_DEVICE = -7, -6


def ulp_distance(a, b):
    """distance in float32 ulps between two float32 arrays (sign-magnitude order mapped to a line)"""
    def key(v):
        i = np.ascontiguousarray(v, np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7fffffff), i)
    return np.abs(key(a) - key(b))


def test_symbols_are_exported(pkg):
    L = pkg.load_library()
    for name in ("mfx_batch_plan_rates", "mfx_batch_resample_layout", "mfx_host_resample_taps", "mfx_host_resampled_length",
                 "mfx_host_resample_layout", "mfx_host_resample_tile"):
        assert name in pkg.mfcc.EXPORTED_SYMBOLS and hasattr(L, name)
    assert L.mfx_abi_version() == 2


@pytest.mark.parametrize("zeros", [1, 6, 64])
@pytest.mark.parametrize("pair", PAIRS)
def test_taps_match_the_formula_to_one_ulp(pkg, pair, zeros):
    h, L, M, P = pkg.mfcc.host_resample_taps(pair[0], pair[1], zeros)
    wl, wm, wp, wh, _ = RR.shape(pair[0], pair[1], zeros)
    assert (L, M, P) == (wl, wm, wp) and h.shape == (L, P)
    want = RR.taps(pair[0], pair[1], zeros)
    assert ulp_distance(h, want.astype(np.float32)).max() <= 1
    # every phase sums to what the float64 formula itself sums to (1 within the window's ripple: up to 18 % at one zero crossing), to float32 rounding of
    # P taps of magnitude <= 1: P u
    assert np.abs(h.astype(np.float64).sum(1) - want.sum(1)).max() <= P * RR.U


def test_default_quality_shapes(pkg):
    assert pkg.mfcc.host_resample_taps(44100, 16000)[1:] == (160, 441, 34)
    assert pkg.mfcc.host_resample_taps(11025, 16000)[1:] == (640, 441, 14)
    assert pkg.mfcc.host_resample_taps(48000, 16000)[1:] == (1, 3, 38)
    h, L, M, P = pkg.mfcc.host_resample_taps(48000, 16000, 6, 0.0)
    assert np.array_equal(h, pkg.mfcc.host_resample_taps(48000, 16000)[0])      # zeros = 0 means 6


@pytest.mark.parametrize("pair", PAIRS)
def test_lengths_are_exact_at_any_size(pkg, pair):
    L, M = RR.ratio(*pair)
    for n in sorted({0, 1, 2, max(M - 1, 0), M, M + 1, 2 ** 31 + 5, 2 ** 40 + 1}):
        assert pkg.mfcc.host_resampled_length(n, *pair) == (n * L + M - 1) // M, n
    assert pkg.mfcc.host_resampled_length(12345, 16000, 16000) == 12345


def test_layout_even_ascending_disjoint(pkg):
    lengths = [0, 1, 2, 4411, 16000, 7, 48001, 3, 0, 8000]
    rates = [8000, 44100, 16000, 44100, 16000, 16000, 48000, 11025, 16000, 8000]
    off, out, total = pkg.mfcc.host_resample_layout(lengths, rates, 16000)
    woff, wout, wtotal = RR.layout(lengths, rates, 16000)
    assert off.tolist() == woff and out.tolist() == wout and total == wtotal
    assert all(o % 2 == 0 for o in off) and total % 2 == 0
    for u in range(1, len(lengths)):
        assert off[u] >= off[u - 1] + out[u - 1]                    # ascending, no overlap
    for u, r in enumerate(rates):
        if r == 16000:
            assert out[u] == lengths[u]                                 # pass-through lengths unchanged
    assert total >= off[-1] + out[-1]


def test_limits_return_err_arg(pkg):
    L = pkg.load_library()
    q = lambda i, o, z=0, r=0.0: L.mfx_host_resample_taps(i, o, z, r, None, 0, None, None, None)
    assert q(999, 16000) == ERR_ARG and q(16000, 768001) == ERR_ARG and q(768000, 1000) == ERR_ARG  # (P = 9310 > 4096)
    assert q(1000, 768000) > 0 and q(768000, 1000, 1, 1.0) == 1536
    assert q(16000, 16001) == ERR_ARG                                   # L = 16001 > 4096
    assert q(44100, 16000, 65) == ERR_ARG and q(44100, 16000, -1) == ERR_ARG
    assert q(44100, 16000, 6, 1.5) == ERR_ARG and q(44100, 16000, 6, -0.1) == ERR_ARG
    assert q(4096, 4095, 64, 0.25) == ERR_ARG                           # L = 4095, P = 514: L P > 2^20
    assert q(4096, 4095, 6) == 4095 * 14
    assert q(768000, 16000, 64) == ERR_ARG                              # P = 2 ceil(64 * 48 / 0.99) > 4096
    out = np.zeros(10, np.float32)
    assert L.mfx_host_resample_taps(48000, 16000, 0, 0.0, out.ctypes.data_as(C.POINTER(C.c_float)), 10, None, None, None) == ERR_ARG
    assert L.mfx_host_resampled_length(-1, 8000, 16000) == ERR_ARG and L.mfx_host_resampled_length(5, 10, 16000) == ERR_ARG
    p64 = C.POINTER(C.c_int64)
    ln, rt = np.array([5], np.int64), np.array([500], np.int32)
    assert L.mfx_host_resample_layout(1, ln.ctypes.data_as(p64), rt.ctypes.data_as(C.POINTER(C.c_int32)), 16000, None, None) == ERR_ARG


def test_tile_rule_stays_inside_the_lds(pkg):
    """every corner of the limits has a tile of at least two outputs, an even count"""
    for i, o, z, r in [(768000, 1000, 1, 1.0), (768000, 1000, 2, 0.75), (1000, 768000, 64, 0.01 * 64), (44100, 16000, 64, 0.99),
                       (16000, 44100, 0, 0.0), (48000, 16000, 0, 0.0), (4096, 4095, 6, 0.0), (11025, 16000, 0, 0.0)]:
        for ch in (1, 2):
            t = pkg.mfcc.host_resample_tile(i, o, z, r, ch)
            assert t >= 2 and t % 2 == 0 and t <= 2048, (i, o, z, r, ch, t)
    assert pkg.mfcc.host_resample_tile(48000, 16000) == 2048 and pkg.mfcc.host_resample_tile(44100, 16000) == 1920
    assert pkg.mfcc.host_resample_tile(16000, 16000) == 4096


def test_the_tile_of_the_output_rate_itself_judges_zeros_and_rolloff(pkg):
    """mfx_host_resample_tile goes through the planners' rate builder with the check the sessions ask for: a pair of equal
    rates is a copy tile, and its zeros and rolloff are still judged (mfx_batch_plan_rates alone does not judge them:
    tests/test_resample_gpu.py, tools/asan/tables_asan.cpp)."""
    L = pkg.load_library()
    assert L.mfx_host_resample_tile(16000, 16000, 0, 0.0, 1) == 4096 and L.mfx_host_resample_tile(16000, 16000, 64, 1.0, 2) == 4096
    assert L.mfx_host_resample_tile(16000, 16000, 65, 0.0, 1) == ERR_ARG and L.mfx_host_resample_tile(16000, 16000, 0, 1.5, 1) == ERR_ARG
    assert L.mfx_host_resample_tile(44100, 16000, 65, 0.0, 1) == ERR_ARG and L.mfx_host_resample_tile(16000, 16001, 0, 0.0, 1) == ERR_ARG
    assert L.mfx_host_resample_tile(44100, 16000, 0, 0.0, 3) == ERR_ARG


def test_the_recorded_cases_name_their_geometry_and_their_paths(pkg):
    """tests/resample_bits_cases.py on the CPU: every case's geometry is the library's, every session cut takes the paths of the
    group loader it is there for, and the one case over 64 KB of LDS is over it."""
    import resample_bits_cases as BC
    for name, c in BC.CASES.items():
        assert BC.geometry(pkg, c) == c["want"], name
        if c["kind"] == "session":
            assert BC.needed(c) <= BC.paths(pkg, c), (name, BC.paths(pkg, c))
    assert BC.lds_bytes(BC.CASES["batch_44142_44100_ch1"]) == 75424
    assert [n for n, c in BC.CASES.items() if c["kind"] == "batch" and BC.lds_bytes(c) > 65536] == ["batch_44142_44100_ch1"]
    assert any("carry5" in BC.needed(c) for c in BC.CASES.values() if c["kind"] == "session")


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
        p64 = C.POINTER(C.c_int64)
        off, ln, rt = np.array([0], np.int64), np.array([8000], np.int64), np.array([8000], np.int32)
        total = C.c_int64(0)
        assert L.mfx_batch_plan_rates(h, 1, off.ctypes.data_as(p64), ln.ctypes.data_as(p64), rt.ctypes.data_as(C.POINTER(C.c_int32)),
                                      0, 0.0, None, C.byref(total)) == ERR_DEVICE
        assert L.mfx_batch_resample_layout(h, None, None, None) == ERR_DEVICE
        assert L.mfx_batch_resample_layout(None, None, None, None) == ERR_ARG
    finally:
        L.mfx_destroy(h)


def test_oracle_bound_holds_for_a_float32_fma_chain(pkg):
    """The chain the kernel is specified as, restated with numpy float32 (an FMA emulated in float64), stays inside the
    bound of resample_ref.convert, and the bound is not vacuous (well under one unit beyond the rounding half)."""
    rng = np.random.default_rng(11)
    x = rng.integers(-32768, 32768, 700).astype(np.int16)
    h, L, M, P = pkg.mfcc.host_resample_taps(44100, 16000)
    o, B = RR.convert(x, h, L, M)
    Wh = P // 2
    xp = np.concatenate([np.zeros(Wh + 1), x.astype(np.float64), np.zeros(Wh + 1)])
    j = np.arange(o.size)
    n, phi = (j * M) // L, (j * M) % L
    acc = np.zeros(o.size, np.float32)
    for k in range(P):
        acc = (h[phi, k].astype(np.float64) * xp[n - Wh + 1 + k + Wh + 1] + acc.astype(np.float64)).astype(np.float32)
    assert (np.abs(acc.astype(np.float64) - o) <= B - 0.5).all()
    assert (B < 0.75).all()
    assert np.abs(RR.to_pcm(acc.astype(np.float64)).astype(np.int64) - RR.to_pcm(o)).max() <= 1


def test_kernel_builds_for_gfx950_without_private_memory():
    """Both instantiations of k_resample (mono, stereo) compiled for gfx950 as the Makefile compiles them: no scratch."""
    hipcc = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    assert os.path.exists(hipcc), "hipcc (the compiler build() uses) was not found"
    r = subprocess.run([hipcc, "-O3", "-fPIC", "-std=c++17", "--offload-arch=gfx950", "-fno-slp-vectorize",
                        "-Rpass-analysis=kernel-resource-usage", "-c", "mfx_resample.hip", "-o", os.devnull],
                       cwd=CSRC, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-2000:]
    names = re.findall(r"Function Name: (\S+)", r.stdout)
    scratch = [int(v) for v in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stdout)]
    kernels = [n for n in names if "k_resample" in n]
    assert len(kernels) == 2 and len(scratch) == len(names)
    assert all(v == 0 for v in scratch), dict(zip(names, scratch))
