"""The online normaliser (mfx_batch_set_online_norm / mfx_sessions_set_online_norm), the parts that need no GPU: the host
restatement mfx_host_online_norm against tests/onorm_ref.py bit for bit, its refusals, the entries on a planning handle."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import onorm_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("mfx_batch_set_online_norm", "mfx_batch_clear_online_norm", "mfx_sessions_set_online_norm",
         "mfx_sessions_clear_online_norm", "mfx_host_online_norm")
LENGTHS = (0, 1, 31, 32, 33, 95, 96, 97, 133, 199)
W = 6


def signal(T, seed=3):
    """[T][6]: four ordinary columns, one constant column, one with mean 1e3 against a deviation of 3"""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((T, W)) * np.array([20, 5, 1, 0.1, 0, 3]) + np.array([60, -3, 0, 0.5, 7.25, 1e3])
    return x.astype(np.float32)


def prior_of(seed=11):
    x = signal(100, seed)
    return np.stack([x.astype(np.float64).sum(0), (x * x).astype(np.float64).sum(0)])


def test_header_exports_and_prototypes_name_the_entries(pkg):
    header = open(os.path.join(ROOT, "include", "mfx.h")).read()
    L = pkg.load_library()
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, header)
        assert name in pkg.mfcc.EXPORTED_SYMBOLS
        assert getattr(L, name).argtypes is not None
    assert L.mfx_abi_version() == 2                          # functions are added, no struct changes
    assert len(L.mfx_batch_set_online_norm.argtypes) == 5 and len(L.mfx_host_online_norm.argtypes) == 10


@pytest.mark.parametrize("kind", (onorm_ref.CMN, onorm_ref.CVN))
@pytest.mark.parametrize("N", (0, 32, 96))
def test_host_entry_is_the_restatement_bit_for_bit(pkg, kind, N):
    pa = prior_of()
    for T in LENGTHS:
        x = signal(T)
        for F, p in ((0, 0), (0, 100), (64, 100), (200, 100)):
            acc = pa if p else None
            got = pkg.mfcc.host_online_norm(x, kind, N, F, p, acc)
            want = onorm_ref.online_norm(x, kind, N, F, p, acc)[0]
            assert got.shape == (T, W) and got.dtype == np.float32
            assert onorm_ref.same_bits(got, want), (kind, N, T, F, p)
            if T:
                assert np.isfinite(got).all()


def test_constant_column_and_large_mean_column():
    """what the definition gives at the two awkward columns: a constant column is exactly 0 (CVN: d = 0, the multiplier is
    1), and the mean-1e3 column stays within the derived bound of its float64 value"""
    x = signal(199)
    for N in (0, 32, 96):
        y, y64, m, mu = onorm_ref.online_norm(x, onorm_ref.CVN, N)
        assert not y[:, 4].any() and (mu[:, 4] == 1.0).all()
        B = onorm_ref.bound(x, m, mu)
        assert (np.abs(y.astype(np.float64) - y64) <= B).all()
        assert np.abs(y[40:, 5]).max() < 6.0                 # (a deviation of 3 scaled to unit variance)


def test_a_pitch_wider_than_the_columns(pkg):
    x = signal(97)
    wide = np.full((97, 11), np.nan, np.float32)
    wide[:, :W] = x
    got = pkg.mfcc.host_online_norm(wide, onorm_ref.CVN, 32, wn=W)
    assert onorm_ref.same_bits(got, onorm_ref.online_norm(x, onorm_ref.CVN, 32)[0])


def test_argument_refusals(pkg):
    L = pkg.load_library()
    x = signal(40)
    out = np.zeros((40, W), np.float32)
    pa = prior_of()
    fp, dp = C.POINTER(C.c_float), C.POINTER(C.c_double)

    def call(T=40, pitch=W, wn=W, kind=1, N=32, F=0, p=0, acc=None, rows=x, dst=out):
        return L.mfx_host_online_norm(None if rows is None else rows.ctypes.data_as(fp), T, pitch, wn, kind, N, F, p,
                                      None if acc is None else acc.ctypes.data_as(dp), None if dst is None else dst.ctypes.data_as(fp))

    assert call() == 0
    assert call(p=100, F=64, acc=pa) == 0
    for bad in (dict(T=-1), dict(wn=0), dict(wn=257, pitch=257), dict(pitch=W - 1), dict(kind=0), dict(kind=3), dict(N=-32), dict(N=16),
                dict(N=33), dict(N=4128), dict(F=-1), dict(F=(1 << 20) + 1), dict(p=-1), dict(p=5), dict(acc=pa), dict(rows=None),
                dict(dst=None)):
        out[:] = 7.0
        assert call(**bad) == -7, bad                        # MFX_ERR_ARG
        assert (out == 7.0).all()                            # and nothing is written
    assert call(T=0, rows=None, dst=None) == 0               # no row: nothing to read or write
    assert call(N=4096) == 0 and call(F=1 << 20) == 0


def test_the_entries_on_a_planning_handle_are_device_errors(pkg):
    L = pkg.load_library()
    cfg = pkg.mfcc.MfxConfig(100 * 160 + 400, 400, 160, 40, 16000.0, 64.0, 8000.0, 13, 0, 22.0, 2, 2, 3, 3, 1, 0, 1, 1, 0, 0, 0)
    h = C.c_void_p()
    assert L.mfx_plan_create(C.byref(cfg), C.byref(h)) == 0
    try:
        for f in (L.mfx_batch_set_online_norm, L.mfx_sessions_set_online_norm):
            assert f(h, 32, 0, 0, None) == -6                # MFX_ERR_DEVICE
            assert b"planning handle" in L.mfx_last_error(h)
        assert L.mfx_batch_clear_online_norm(h) == -6 and L.mfx_sessions_clear_online_norm(h) == -6
    finally:
        L.mfx_destroy(h)
