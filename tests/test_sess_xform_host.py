"""The session transform (mfx_sessions_set_transform) on the CPU: the new symbols, the planner's step against a brute-force
model of the whole stream, the packer of k_sess_xform's work list, what a planning handle answers, and the new translation
unit's resource usage when compiled for gfx950 (no GPU)."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import sess_xform_drive as SD

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "asr-featext-opencl_amd", "csrc")
W, S = 400, 160

NEW = ("mfx_sessions_set_transform", "mfx_sessions_clear_transform", "mfx_sessions_select_transform", "mfx_sessions_output_width",
       "mfx_host_session_xform_step", "mfx_host_sess_xform_groups")


def test_symbols_are_declared_and_exported(pkg):
    L = pkg.load_library()
    header = open(os.path.join(ROOT, "include", "mfx.h")).read()
    for name in NEW:
        assert name in pkg.mfcc.EXPORTED_SYMBOLS and hasattr(L, name)
        assert re.search(r"\b%s\(" % name, header), name
    assert pkg.mfcc.ENGINE_SESS_XFORM_PLAIN == 4096
    assert re.search(r"#define MFX_ENGINE_SESS_XFORM_PLAIN 4096\b", header)
    assert L.mfx_abi_version() == 2
    for name in ("sessions_set_transform", "sessions_clear_transform", "sessions_select_transform", "sessions_output_width",
                 "host_session_xform_step"):
        assert hasattr(pkg.MfccHip, name)


def _cuts(n, rng, flush):
    """Piece lengths of a stream of n samples: empty pushes, single samples, short and long pieces; the end either as a
    zero-sample final push (the flush) or inside the last piece."""
    out, left = [], n
    while left > 0:
        r = rng.random()
        k = 0 if r < 0.2 else 1 if r < 0.3 else int(rng.integers(1, 3000))
        k = min(k, left)
        left -= k
        out.append([k, False])
    if flush or not out:
        out.append([0, True])
    else:
        out[-1][1] = True
    return out


@pytest.mark.parametrize("D", (0, 2, 6))
@pytest.mark.parametrize("right", (0, 1, 4, 32))
@pytest.mark.parametrize("left", (0, 1, 4, 32))
def test_step_against_a_brute_force_model_of_the_stream(pkg, left, right, D):
    """Whole stream first (the definition: output t reads rows clamp(t - left + c, 0, T - 1) of the stream), then cut: every
    push's slot holds the rows its outputs read, at the rows the step says."""
    step, xstep = pkg.mfcc.host_session_step, pkg.mfcc.host_session_xform_step
    rng = np.random.default_rng(1000 * left + 10 * right + D)
    for T in sorted({0, 1, 2, right, right + 1, 100}):
        n = int(rng.integers(0, W)) if T == 0 else W + (T - 1) * S + int(rng.integers(0, S))
        for trial in range(4):
            cuts = [[n, True]] if trial == 0 else _cuts(n, rng, flush=trial % 2 == 1)
            state, xstate = (0, 0), (0, 0)
            slot0, delivered = 0, 0                             # stream row that is row 0 of the previous slot; rows so far
            for length, fin in cuts:
                st = step(W, S, D, state, length, fin)
                Ey, Ex = xstate
                xs = xstep(left, right, xstate, st["rows"], fin)
                Ey_new = Ey + st["rows"]
                Ex_new = Ey_new if fin else max(0, Ey_new - right)
                assert xs["rows"] == Ex_new - Ex
                assert xs["state"] == ((0, 0) if fin else (Ey_new, Ex_new))
                y0 = max(0, Ex - left)                          # rows [y0, Ey) are carried in: at most left + right
                assert xs["carry_rows"] == Ey - y0 and 0 <= xs["carry_rows"] <= left + right
                assert y0 >= slot0                              # ... and the previous slot holds them
                slot_rows = xs["carry_rows"] + st["rows"]
                assert slot_rows <= left + right + st["new_frames"] + D
                assert xs["src_row0"] == Ex - y0 and xs["lo"] == -xs["src_row0"]
                for r in range(xs["rows"]):
                    for c in range(left + right + 1):
                        row = xs["src_row0"] + min(max(r - left + c, xs["lo"]), xs["hi"])
                        assert 0 <= row < slot_rows, (T, cuts, r, c, row, slot_rows)
                        assert y0 + row == min(max(Ex + r - left + c, 0), T - 1)     # the whole stream's clamp
                delivered += xs["rows"]
                slot0 = y0
                state, xstate = st["state"], xs["state"]
            assert delivered == T and state == (0, 0) and xstate == (0, 0)


def test_step_refuses_bad_arguments(pkg):
    L = pkg.load_library()
    st = (C.c_int64 * 2)(5, 3)
    assert L.mfx_host_session_xform_step(33, 0, st, 1, 0, None, None) == -7
    assert L.mfx_host_session_xform_step(0, -1, st, 1, 0, None, None) == -7
    assert L.mfx_host_session_xform_step(1, 1, st, -1, 0, None, None) == -7
    assert L.mfx_host_session_xform_step(1, 1, None, 1, 0, None, None) == -7
    bad = (C.c_int64 * 2)(3, 5)                                  # more delivered than finished
    assert L.mfx_host_session_xform_step(1, 1, bad, 1, 0, None, None) == -7
    assert L.mfx_host_session_xform_step(1, 1, st, 4, 0, None, None) == 5 and tuple(st) == (9, 8)


@pytest.mark.parametrize("G", (1, 2, 4))
def test_packer_covers_every_row_once_and_mixes_no_transforms(pkg, G):
    rng = np.random.default_rng(G)
    for trial in range(30):
        n = int(rng.integers(0, 40))
        n_out = rng.choice([0, 0, 1, 9, 10, 11, 15, 16, 17, 32, 33, 100], n).astype(np.int32)
        xf = rng.integers(0, 5, n).astype(np.int32)
        groups, blocks = pkg.mfcc.host_sess_xform_groups(n_out, xf, G)
        seen = [np.zeros(k, np.int32) for k in n_out]
        for piece, r0, rows in groups:
            assert 1 <= rows <= 16 and r0 % 16 == 0
            seen[piece][r0:r0 + rows] += 1
        assert all((s == 1).all() for s in seen)                # every delivered row is in exactly one group
        assert len(groups) == int(((n_out + 15) // 16).sum())
        gx = [int(xf[p]) for p, _, _ in groups]
        assert gx == sorted(gx)                                 # sorted by transform
        nxt = 0
        for g0, ng, x in blocks:
            assert g0 == nxt and 1 <= ng <= G
            assert all(v == x for v in gx[g0:g0 + ng])          # no block mixes transforms
            nxt = g0 + ng
        assert nxt == len(groups)
        # a block is closed early only where the transform changes
        for k, (g0, ng, x) in enumerate(blocks[:-1]):
            assert ng == G or blocks[k + 1][2] != x
    groups, blocks = pkg.mfcc.host_sess_xform_groups([0, 0, 0], [1, 0, 2], G)
    assert len(groups) == 0 and len(blocks) == 0               # an empty push gives no groups
    groups, blocks = pkg.mfcc.host_sess_xform_groups([], [], G)
    assert len(groups) == 0 and len(blocks) == 0
    L = pkg.load_library()
    one = (C.c_int32 * 1)(5)
    assert L.mfx_host_sess_xform_groups(1, one, one, 3, None, 0, None, 0, None) == -7


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
        A = np.zeros((8, 39), np.float32)
        fpt = C.POINTER(C.c_float)
        assert L.mfx_sessions_set_transform(h, 0, 0, 8, 1, A.ctypes.data_as(fpt), None) == -6
        assert L.mfx_sessions_set_transform(h, 99, -1, 0, 0, None, None) == -6       # before any argument is looked at
        assert L.mfx_sessions_clear_transform(h) == -6
        assert L.mfx_sessions_select_transform(h, 0, 0) == -6
        assert L.mfx_sessions_output_width(h) == -6
        assert L.mfx_sessions_output_width(None) == -7
    finally:
        L.mfx_destroy(h)


def test_kernel_builds_for_gfx950_without_private_memory():
    """Every instantiation of k_sess_xform compiled for gfx950 as the Makefile compiles it: no scratch."""
    hipcc = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    assert os.path.exists(hipcc), "hipcc (the compiler build() uses) was not found"
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"^KERNEL_TUS :=.*\bmfx_sess_xform\b", mk, re.M)
    r = subprocess.run([hipcc, "-O3", "-fPIC", "-std=c++17", "--offload-arch=gfx950", "-fno-slp-vectorize",
                        "-Rpass-analysis=kernel-resource-usage", "-c", "mfx_sess_xform.hip", "-o", os.devnull],
                       cwd=CSRC, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-2000:]
    names = re.findall(r"Function Name: (\S+)", r.stdout)
    scratch = [int(v) for v in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stdout)]
    kernels = [n for n in names if "k_sess_xform" in n]
    assert len(kernels) == 12 and len(scratch) == len(names)     # matrix and vector form x 1, 2, 3, 4, 8, 16 tiles per wave
    assert all(v == 0 for v in scratch), dict(zip(names, scratch))
