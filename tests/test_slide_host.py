"""The sliding-window normaliser's host entries (mfx_host_sliding_window, mfx_host_sliding_norm) against tests/slide_ref.py,
and the argument checks that need no device.  No GPU."""
import ctypes as C
import os

import numpy as np
import pytest

import slide_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARG, DEVICE = -7, -6
SYMBOLS = ("mfx_batch_set_sliding_norm", "mfx_batch_clear_sliding_norm", "mfx_host_sliding_window", "mfx_host_sliding_norm")


def test_symbols_are_declared_and_exported(pkg):
    header = open(os.path.join(ROOT, "include", "mfx.h")).read()
    L = pkg.load_library()
    for s in SYMBOLS:
        assert s + "(" in header, s
        assert s in pkg.mfcc.EXPORTED_SYMBOLS, s
        assert getattr(L, s) is not None
    assert "HAS NOT BEEN MEASURED" in header                  # agreement with a Kaldi binary: said where it is defined
    assert pkg.host_sliding_norm is pkg.mfcc.host_sliding_norm and pkg.host_sliding_window is pkg.mfcc.host_sliding_window
    assert hasattr(pkg.MfccHip, "batch_set_sliding_norm") and hasattr(pkg.MfccHip, "batch_clear_sliding_norm")


def test_window_against_kaldis_loop(pkg):
    """Every t of T = 1 .. 70, N in {1, 2, 3, 32, 33, 64}, both centres, min_window in {0, 1, N div 2, N}: the loop's window, the
    invariant 0 <= ws <= t < we <= T, and what k_slide_apply's chains rest on -- we - 1 and ws - 1 never decrease from a row
    to the next and advance by at most one."""
    n = 0
    for T in range(1, 71):
        for N in (1, 2, 3, 32, 33, 64):
            for center in (0, 1):
                for mw in sorted({0, 1, N // 2, N}):
                    prev = None
                    for t in range(T):
                        ws, we = pkg.host_sliding_window(T, N, mw, center, t)
                        assert (ws, we) == R.window(T, N, mw, center, t), (T, N, center, mw, t)
                        assert 0 <= ws <= t < we <= T, (T, N, center, mw, t, ws, we)
                        if prev is not None:
                            assert 0 <= ws - prev[0] <= 1 and 0 <= we - prev[1] <= 1, (T, N, center, mw, t, prev, ws, we)
                        prev = (ws, we)
                        n += 1
    assert n == 2 * (2 + 3 + 3 + 4 + 4 + 4) * sum(range(1, 71))   # (the distinct min_window values of N = 1, 2, 3, 32, 33, 64)
    # the steady window without a centre holds N + 1 rows, with one N
    assert pkg.host_sliding_window(1000, 300, 100, 0, 500) == (200, 501)
    assert pkg.host_sliding_window(1000, 300, 100, 1, 500) == (350, 650)


def rows_of(T, W, seed):
    """Rows that look like features, with a constant column and a column of +-3e4."""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((T, W)) * rng.uniform(0.5, 8.0, W) + rng.standard_normal(W) * 20.0).astype(np.float32)
    x[:, 0] = np.float32(-7.25)
    if W > 1:
        x[:, W - 1] = (3e4 * np.where(rng.random(T) < 0.5, -1.0, 1.0)).astype(np.float32)
    return x


@pytest.mark.parametrize("W", (1, 13, 39, 256))
def test_rows_are_the_restatement_bit_for_bit(pkg, W):
    worst = {False: 0.0, True: 0.0}
    for T, N, mw, center in ((1, 300, 0, 1), (2, 2, 0, 1), (33, 32, 0, 1), (70, 33, 0, 1), (161, 64, 0, 1), (161, 4096, 0, 1),
                             (70, 1, 1, 0), (97, 64, 64, 0), (97, 64, 1, 0), (161, 100, 0, 0), (161, 33, 16, 0)):
        x = rows_of(T, W, 1000 * W + T + N)
        for nv in (False, True):
            want, y64, _, _, B = R.sliding_norm(x, N, mw, center, nv)
            got = pkg.host_sliding_norm(x, N, mw, center, nv)
            assert R.same_bits(got, want), (W, T, N, mw, center, nv, int((got.view(np.uint32) != want.view(np.uint32)).sum()))
            if N >= 32 and T >= 32 and (center or mw >= 32):  # every window holds >= 32 rows: the float64 bar applies
                err = np.abs(want.astype(np.float64) - y64)
                assert (err <= B).all(), (W, T, N, mw, center, nv)
                with np.errstate(invalid="ignore", divide="ignore"):
                    worst[nv] = max(worst[nv], float(np.nanmax(np.where(B > 0, err / B, 0.0))))
            if nv:
                assert np.isfinite(got).all()
                assert (got[:, 0] == 0).all()                 # the constant column: c = 0 times the floored multiplier
    print("width %d: worst err / B of the restatement: CMN %.3g, CVN %.3g" % (W, worst[False], worst[True]))
    # a pitch wider than the row on both sides
    x = rows_of(50, W + 3, 7)
    out = np.full((50, W + 2), np.float32(np.nan))
    fp = C.POINTER(C.c_float)
    L = pkg.load_library()
    assert L.mfx_host_sliding_norm(x.ctypes.data_as(fp), 50, W, W + 3, 32, 0, 1, 1, out.ctypes.data_as(fp), W + 2) == 0
    assert R.same_bits(out[:, :W], R.sliding_norm(x[:, :W], 32, 0, True, True, exact=False)[0]) and np.isnan(out[:, W:]).all()


def test_argument_checks_without_a_device(pkg):
    L = pkg.load_library()
    cfg = pkg.MfxConfig(8000, 400, 160, 40, 16000.0, 64.0, 8000.0, 13, 0, 22.0, 0, 2, 3, 3, 1, 0, 1, 1, 0, 0, 0)
    h = C.c_void_p()
    assert L.mfx_plan_create(C.byref(cfg), C.byref(h)) == 0
    try:
        assert L.mfx_batch_set_sliding_norm(h, 300, 100, 1, 0) == DEVICE
        assert L.mfx_batch_clear_sliding_norm(h) == DEVICE
        assert DEVICE == L.mfx_create(C.byref(cfg), 9999, C.byref(C.c_void_p()))   # (= MFX_ERR_DEVICE)
    finally:
        L.mfx_destroy(h)
    ws, we = C.c_int64(-5), C.c_int64(-5)
    for T, N, mw, center, t in ((10, 0, 0, 1, 0), (10, 4097, 0, 1, 0), (10, 32, -1, 0, 0), (10, 32, 33, 0, 0), (10, 32, 0, 2, 0),
                                (10, 32, 0, -1, 0), (10, 32, 0, 1, 10), (10, 32, 0, 1, -1), (0, 32, 0, 1, 0)):
        assert L.mfx_host_sliding_window(T, N, mw, center, t, C.byref(ws), C.byref(we)) == ARG, (T, N, mw, center, t)
    assert L.mfx_host_sliding_window(10, 32, 0, 1, 0, None, C.byref(we)) == ARG
    assert (ws.value, we.value) == (-5, -5)
    x = np.ones((4, 3), np.float32)
    out = np.full((4, 3), np.float32(7.0))
    fp = C.POINTER(C.c_float)
    xp, op = x.ctypes.data_as(fp), out.ctypes.data_as(fp)
    for T, W, pitch, N, mw, center, nv, opitch in ((4, 3, 3, 0, 0, 1, 0, 3), (4, 3, 3, 4097, 0, 1, 0, 3), (4, 3, 3, 32, -1, 0, 0, 3),
                                                   (4, 3, 3, 32, 33, 0, 0, 3), (4, 3, 3, 32, 0, 2, 0, 3), (4, 3, 3, 32, 0, 1, 2, 3),
                                                   (4, 0, 3, 32, 0, 1, 0, 3), (4, 257, 257, 32, 0, 1, 0, 257), (4, 3, 2, 32, 0, 1, 0, 3),
                                                   (4, 3, 3, 32, 0, 1, 0, 2), (-1, 3, 3, 32, 0, 1, 0, 3)):
        assert L.mfx_host_sliding_norm(xp, T, W, pitch, N, mw, center, nv, op, opitch) == ARG, (T, W, pitch, N, mw, center, nv, opitch)
    assert L.mfx_host_sliding_norm(None, 4, 3, 3, 32, 0, 1, 0, op, 3) == ARG
    assert (out == 7.0).all()
    assert L.mfx_host_sliding_norm(None, 0, 3, 3, 32, 0, 1, 0, None, 3) == 0   # no row: nothing to read or write
