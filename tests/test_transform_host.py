"""Splice + affine transform on the CPU: what a planning handle answers, the operand builder against the matrix element
by element, the float64 oracle against its own defining properties, and the new translation unit's resource usage when
compiled for gfx950 (no GPU)."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import xform_ref as XR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "asr-featext-opencl_amd", "csrc")


def _plan_handle(pkg):
    L = pkg.load_library()
    cfg = pkg.MfxConfig()
    for k, v in dict(input_buffer_size=16000, window_size=400, shift=160, num_banks=40, sample_rate=16000.0, low_freq=64.0,
                     high_freq=8000.0, ceps_len=13, want_c0=0, lift_coef=22.0, norm=0, dyn=2, delta_l1=3, delta_l2=3,
                     norm_after_dyn=1).items():
        setattr(cfg, k, v)
    h = C.c_void_p()
    assert L.mfx_plan_create(C.byref(cfg), C.byref(h)) == 0
    return L, h


def test_a_planning_handle_answers_err_device(pkg):
    L, h = _plan_handle(pkg)
    try:
        A = np.zeros((8, 39), np.float32)
        fpt = C.POINTER(C.c_float)
        assert L.mfx_batch_set_transform(h, 0, 0, 8, 1, A.ctypes.data_as(fpt), None, None, 0) == -6
        assert L.mfx_batch_set_transform(h, 0, 0, 0, 0, None, None, None, 0) == -6
        assert L.mfx_batch_output_width(h) == L.mfx_get_output_data_width(h) == 39      # a geometry accessor: answered
        assert L.mfx_batch_output_width(None) == -7
    finally:
        L.mfx_destroy(h)


def test_symbols_are_exported(pkg):
    L = pkg.load_library()
    for name in ("mfx_batch_set_transform", "mfx_batch_output_width", "mfx_host_xform_operands"):
        assert name in pkg.mfcc.EXPORTED_SYMBOLS and hasattr(L, name)
    assert pkg.mfcc.ENGINE_XFORM_VALU == 1024
    assert L.mfx_abi_version() == 2


@pytest.mark.parametrize("out_dim,in_dim", [(1, 1), (13, 52), (40, 351), (17, 39), (16, 8), (256, 39), (33, 450)])
def test_operands_hold_the_matrix_element_by_element(pkg, out_dim, in_dim):
    rng = np.random.default_rng(out_dim * 10007 + in_dim)
    A = rng.standard_normal((out_dim, in_dim)).astype(np.float32)
    ops = pkg.mfcc.host_xform_operands(A)
    tiles, steps = (out_dim + 15) // 16, (in_dim + 3) // 4
    assert ops.shape == (steps, tiles, 64)
    pad = np.zeros((tiles * 16, steps * 4), np.float32)
    pad[:out_dim, :in_dim] = A
    lane = np.arange(64)
    for s in range(steps):
        for t in range(tiles):
            want = pad[16 * t + (lane & 15), 4 * s + (lane >> 4)]
            assert np.array_equal(ops[s, t].view(np.uint32), want.view(np.uint32)), (s, t)
    # every element of A appears exactly once, everything else is zero
    assert np.count_nonzero(ops) == np.count_nonzero(A)


def test_operand_builder_refuses_shapes_outside_the_limits(pkg):
    L = pkg.load_library()
    A = np.zeros(16, np.float32)
    fpt = C.POINTER(C.c_float)
    for od, ind in [(0, 4), (257, 4), (4, 0), (4, 8193)]:
        assert L.mfx_host_xform_operands(od, ind, A.ctypes.data_as(fpt), None, 0, None, None) == -7
    assert L.mfx_host_xform_operands(4, 4, None, None, 0, None, None) == -7
    out = np.zeros(10, np.float32)
    assert L.mfx_host_xform_operands(4, 4, A.ctypes.data_as(fpt), out.ctypes.data_as(fpt), out.size, None, None) == -7  # too small
    assert L.mfx_host_xform_operands(4, 4, A.ctypes.data_as(fpt), None, 0, None, None) == 64


def test_oracle_splice_clamps_at_the_utterance_ends():
    y = np.arange(5 * 2, dtype=np.float32).reshape(5, 2)
    z = XR.splice(y, 2, 1)
    assert z.shape == (5, 8)
    for t in range(5):
        for c, dt in enumerate((-2, -1, 0, 1)):
            assert np.array_equal(z[t, 2 * c:2 * c + 2], y[min(max(t + dt, 0), 4)])
    assert XR.splice(y[:1], 3, 3).tolist() == [list(y[0]) * 7]
    assert XR.splice(y[:0], 1, 1).shape == (0, 6)


def test_oracle_bound_holds_for_a_float32_fma_chain():
    """The chain the kernel is specified as, restated with numpy float32 (an FMA emulated in float64: the product of two
    float32 is exact there, the sum rounds once to float64 and once to float32 -- double rounding moves a result by at
    most one part in 2^29 of an ulp-sized step, far inside gamma), stays inside the bound; the bound is not vacuous."""
    rng = np.random.default_rng(3)
    y = rng.standard_normal((9, 39)).astype(np.float32)
    A = (rng.standard_normal((5, 3 * 39)) / 10).astype(np.float32)
    b = rng.standard_normal(5).astype(np.float32)
    o, bound = XR.xform_ref(y, A, b, 1, 1)
    z = XR.splice(y, 1, 1)
    acc = np.repeat(b[None, :], 9, 0).astype(np.float32)
    for i in range(z.shape[1]):
        acc = (A[None, :, i].astype(np.float64) * z[:, i, None].astype(np.float64) + acc.astype(np.float64)).astype(np.float32)
    err = np.abs(acc.astype(np.float64) - o)
    assert (err <= bound).all() and err.max() > 0
    assert (bound < 1e-3 * np.abs(o).max()).all()


def test_tile_rule_always_finds_a_tile_inside_the_limits():
    """The limits of mfx_batch_set_transform leave a tile at every row width a handle can have (at most 256 static columns
    x 3): the rule restated in xform_ref.py never returns 0 on the corners."""
    for width in (1, 13, 39, 150, 256, 768):
        for left, right in ((0, 0), (32, 32), (32, 0), (0, 32), (4, 4)):
            if (left + right + 1) * width > 8192:
                continue
            for out_dim in (1, 16, 17, 40, 255, 256):
                R = XR.tile_rows(width, left, right, out_dim)
                assert R in (64, 32, 16), (width, left, right, out_dim)
                assert XR.lds_bytes(R, width, left, right, out_dim) <= 160 * 1024
    assert XR.tile_rows(768, 5, 4, 256) == 16 and XR.tile_rows(39, 4, 4, 40) == 64


def test_kernel_builds_for_gfx950_without_private_memory():
    """Every instantiation of k_splice_affine compiled for gfx950 as the Makefile compiles it: no scratch (a spilled or
    dynamically indexed accumulator would show here before any GPU run)."""
    hipcc = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    assert os.path.exists(hipcc), "hipcc (the compiler build() uses) was not found"
    r = subprocess.run([hipcc, "-O3", "-fPIC", "-std=c++17", "--offload-arch=gfx950", "-fno-slp-vectorize",
                        "-Rpass-analysis=kernel-resource-usage", "-c", "mfx_xform.hip", "-o", os.devnull],
                       cwd=CSRC, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-2000:]
    names = re.findall(r"Function Name: (\S+)", r.stdout)
    scratch = [int(v) for v in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stdout)]
    kernels = [n for n in names if "k_splice_affine" in n]
    assert len(kernels) == 12 and len(scratch) == len(names)     # matrix and vector form x 1, 2, 3, 4, 8, 16 tiles per wave
    assert all(v == 0 for v in scratch), dict(zip(names, scratch))
