"""Dense padded tensor output (mfx_batch_set_tensor) on the CPU: the declared and exported symbols, what a planning handle
answers, the byte count over the shape limits, the host restatement (integer conversions) against tensor_ref.py (torch's CPU
conversions) bit for bit, the new translation unit's resource usage when compiled for gfx950, and the sanitizer run of the
restatement (no GPU)."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import tensor_ref as TR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "asr-featext-opencl_amd", "csrc")
INT_NAMES = ("mfx_batch_set_tensor", "mfx_batch_clear_tensor", "mfx_batch_tensor_shape", "mfx_batch_tensor_lengths",
             "mfx_batch_tensor_from_rows", "mfx_host_tensor_pack")
I64_NAMES = ("mfx_batch_output_bytes", "mfx_host_tensor_bytes", "mfx_host_tensor_lds_bytes")
WRAPPERS = ("batch_set_tensor", "batch_clear_tensor", "batch_output_bytes", "batch_tensor_shape", "batch_tensor_lengths",
            "batch_tensor_from_rows")
LAYOUTS = (TR.TIME_MAJOR, TR.CHANNEL_MAJOR)
DTYPES = (TR.F32, TR.F16, TR.BF16)


def test_symbols_are_declared_and_exported(pkg):
    L = pkg.load_library()
    header = open(os.path.join(ROOT, "include", "mfx.h")).read()
    for name in INT_NAMES:
        assert name in pkg.mfcc.EXPORTED_SYMBOLS and hasattr(L, name)
        assert re.search(r"^int %s\(" % name, header, re.M), name
    for name in I64_NAMES:
        assert name in pkg.mfcc.EXPORTED_SYMBOLS and hasattr(L, name)
        assert re.search(r"^int64_t %s\(" % name, header, re.M), name
    assert re.search(r"enum \{ MFX_TENSOR_TIME_MAJOR = 0 [^}]*, MFX_TENSOR_CHANNEL_MAJOR = 1 [^}]*\};", header)
    assert re.search(r"enum \{ MFX_DTYPE_F32 = 0, MFX_DTYPE_F16 = 1, MFX_DTYPE_BF16 = 2 \};", header)
    assert (pkg.TENSOR_TIME_MAJOR, pkg.TENSOR_CHANNEL_MAJOR) == (0, 1)
    assert (pkg.DTYPE_F32, pkg.DTYPE_F16, pkg.DTYPE_BF16) == (0, 1, 2)
    assert L.mfx_abi_version() == 2
    for name in WRAPPERS:
        assert callable(getattr(pkg.MfccHip, name)), name
    for name in ("host_tensor_pack", "host_tensor_bytes"):
        assert callable(getattr(pkg, name)), name


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
        assert L.mfx_batch_set_tensor(h, 0, 0, 0, 0.0) == -6
        assert L.mfx_batch_set_tensor(h, 9, 9, -5, 0.0) == -6                  # (before any argument is looked at)
        assert L.mfx_batch_clear_tensor(h) == -6
        assert L.mfx_batch_output_bytes(h) == -6
        assert L.mfx_batch_tensor_shape(h, None, None) == -6
        assert L.mfx_batch_tensor_lengths(h, None, None) == -6
        assert L.mfx_batch_tensor_from_rows(h, None, None) == -6
        assert L.mfx_batch_set_tensor(None, 0, 0, 0, 0.0) == -7
        assert L.mfx_batch_output_bytes(None) == -7
    finally:
        L.mfx_destroy(h)


def test_tensor_bytes_over_the_shape_limits(pkg):
    hb = pkg.host_tensor_bytes
    assert hb(3, 5, 7, TR.F32) == 3 * 5 * 7 * 4 and hb(3, 5, 7, TR.F16) == hb(3, 5, 7, TR.BF16) == 3 * 5 * 7 * 2
    assert hb(0, 5, 7, TR.F32) == hb(3, 5, 0, TR.F16) == hb(3, 0, 7, TR.F16) == 0
    # the largest t_pad, and one beyond it
    assert hb(1, 1, 1 << 24, TR.F32) == 4 << 24
    # 64-bit counts: a batch the 32-bit product of which wraps
    assert hb(100000, 256, 1 << 24, TR.F32) == 100000 * 256 * (1 << 24) * 4
    L = pkg.load_library()
    for bad in ((1, 1, (1 << 24) + 1, 0), (-1, 1, 1, 0), (1, -1, 1, 0), (1, 1, -1, 0), (1, 1, 1, 3), (1, 1, 1, -1),
                ((1 << 40), 1023, 1 << 24, 0),                      # beyond int64
                ((1 << 62) // (1 << 24), 1, 1 << 24, 1)):           # 2^62 elements of 2 bytes: exactly 2^63
        assert L.mfx_host_tensor_bytes(*bad) == -7, bad
    assert hb((1 << 61) // (1 << 24), 1, 1 << 24, TR.F16) == 1 << 62
    r, lds = pkg.host_tensor_tile()
    assert r in (64, 128)
    assert lds(256) == r * 257 * 4 <= 160 * 1024 and lds(39) == r * 39 * 4 and lds(1) == r * 4


@pytest.fixture(scope="module")
def edges():
    return TR.edge_values()


@pytest.mark.parametrize("dtype", DTYPES)
def test_host_conversion_of_the_edge_values_equals_torch(pkg, edges, dtype):
    """(a) .. (e) of tensor_ref.edge_values through mfx_host_tensor_pack as one long utterance of width 1 -- and once more as
    the pad value of an empty one -- against torch's CPU conversion."""
    x = edges.view(np.float32).reshape(-1, 1)
    got = pkg.host_tensor_pack(x, [0], [x.shape[0]], x.shape[0], TR.TIME_MAJOR, dtype)
    want = TR.convert(x.reshape(1, -1, 1), dtype)
    assert TR.same_bits(got, want, dtype)
    if dtype != TR.F32:                                   # the check is not vacuous: ties, subnormals, inf and NaN are all there
        w = want.view(np.uint16).reshape(-1)
        exp, man = (0x7c00, 0x03ff) if dtype == TR.F16 else (0x7f80, 0x007f)
        assert ((w & exp) == exp).any() and (((w & exp) == 0) & ((w & man) != 0)).any() and (w == 0x8000).any()
    # the pad value goes through the same conversion (no NaN here: a Python float does not carry a float32 NaN's payload)
    for bits in edges[:: max(1, edges.size // 257)]:
        pad = np.array([bits], np.uint32).view(np.float32)[0]
        if np.isnan(pad):
            continue
        got = pkg.host_tensor_pack(np.zeros((1, 1), np.float32), [0], [0], 1, TR.CHANNEL_MAJOR, dtype, pad=pad)
        assert TR.same_bits(got, TR.convert(np.array([[[pad]]], np.float32), dtype), dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("shape", ((3, 5, 1), (2, 7, 39), (1, 0, 4)))
def test_host_pack_equals_the_reference(pkg, edges, shape, layout, dtype):
    """Both layouts, lengths 0, below Tp and above Tp."""
    B, Tp, Wo = shape
    rng = np.random.default_rng(B * 100 + Tp)
    lengths = {3: [0, Tp - 2, Tp + 3], 2: [Tp + 3, Tp - 2], 1: [Tp + 3]}[B]
    out_rows = np.concatenate([[0], np.cumsum(lengths)[:-1]]).astype(np.int64)
    total = int(np.sum(lengths))
    rows = (100.0 * rng.standard_normal((total, Wo))).astype(np.float32)
    flat = rows.reshape(-1)
    flat[::5] = edges[rng.integers(0, edges.size, flat[::5].size)].view(np.float32)     # every fifth value an edge value
    got = pkg.host_tensor_pack(rows, out_rows, lengths, Tp, layout, dtype, pad=-1.5)
    want = TR.tensor_ref(rows, out_rows, lengths, Tp, layout, dtype, -1.5)
    assert got.shape == want.shape == ((B, Tp, Wo) if layout == TR.TIME_MAJOR else (B, Wo, Tp))
    assert got.dtype == want.dtype == TR.NP_DTYPE[dtype]
    assert TR.same_bits(got, want, dtype)


def test_host_pack_refuses_what_is_outside_the_limits(pkg):
    L = pkg.load_library()
    rows = np.zeros((4, 2), np.float32)
    r0, ln = np.zeros(1, np.int64), np.array([4], np.int32)
    out = np.zeros(64, np.float32)
    fp, p64, p32 = C.POINTER(C.c_float), C.POINTER(C.c_int64), C.POINTER(C.c_int32)
    call = lambda B, Wo, Tp, layout, dtype: L.mfx_host_tensor_pack(rows.ctypes.data_as(fp), r0.ctypes.data_as(p64), ln.ctypes.data_as(p32),
                                                                  B, Wo, Tp, layout, dtype, 0.0, C.c_void_p(out.ctypes.data))
    assert call(1, 2, 4, 0, 0) == 0
    for bad in ((1, 0, 4, 0, 0), (1, 2, 4, 2, 0), (1, 2, 4, 0, 3), (1, 2, -1, 0, 0), (-1, 2, 4, 0, 0), (1, 2, (1 << 24) + 1, 0, 0)):
        assert call(*bad) == -7, bad


def test_kernels_build_for_gfx950_without_private_memory():
    hipcc = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    assert os.path.exists(hipcc), "hipcc (the compiler build() uses) was not found"
    r = subprocess.run([hipcc, "-O3", "-fPIC", "-std=c++17", "--offload-arch=gfx950", "-fno-slp-vectorize",
                        "-Rpass-analysis=kernel-resource-usage", "-c", "mfx_tensor.hip", "-o", os.devnull],
                       cwd=CSRC, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-2000:]
    names = re.findall(r"Function Name: (\S+)", r.stdout)
    scratch = [int(v) for v in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stdout)]
    assert len(scratch) == len(names)
    assert sum("k_tensor_pack_tm" in n for n in names) == 3 and sum("k_tensor_pack_cm" in n for n in names) == 3   # per element type
    assert all(v == 0 for v in scratch), dict(zip(names, scratch))


def test_restatement_runs_clean_under_the_sanitizers(tmp_path):
    """tools/asan/tensor_asan.cpp (tensor_pack_host of mfx_tables.cpp into exactly sized buffers) as `make asan` builds and runs
    it: a stand-alone CPU program under AddressSanitizer + UBSan."""
    gxx = shutil.which("g++")
    assert gxx, "g++ was not found"
    exe = str(tmp_path / "tensor_asan")
    r = subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-ffp-contract=off", "-o", exe,
                        os.path.join(ROOT, "tools", "asan", "tensor_asan.cpp"), os.path.join(CSRC, "mfx_tables.cpp")],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-2000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env)
    assert r.returncode == 0 and "tensor clean" in r.stdout, r.stdout[-2000:]
