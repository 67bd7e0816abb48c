"""TRAPS on the CPU: the library's configuration checks, kernel choice and host basis against the float64 oracle of
tests/traps_ref.py, and the oracle against its own defining properties (no GPU)."""
import ctypes as C

import numpy as np
import pytest

import traps_ref


def _cfg(pkg, **kw):
    base = dict(input_buffer_size=16000, window_size=400, shift=160, num_banks=15, sample_rate=16000.0, low_freq=64.0,
                high_freq=8000.0, ceps_len=0, want_c0=0, lift_coef=22.0, norm=0, dyn=2, delta_l1=3, delta_l2=3,
                norm_after_dyn=1, method=pkg.METHOD_TRAPS, traps_len=0, traps_dct_len=0)
    base.update(kw)
    cfg = pkg.MfxConfig()
    for k, v in base.items():
        setattr(cfg, k, v)
    return cfg


def _plan(pkg, cfg):
    L = pkg.load_library()
    h = C.c_void_p()
    rc = L.mfx_plan_create(C.byref(cfg), C.byref(h))
    if rc != 0:
        return rc, None
    try:
        return rc, L.mfx_get_output_data_width(h)
    finally:
        L.mfx_destroy(h)


def test_method_supported(pkg):
    L = pkg.load_library()
    assert pkg.METHOD_TRAPS == 3
    assert L.mfx_method_supported(3) == 1
    assert L.mfx_method_supported(2) == 0  # unassigned, stays refused
    assert L.mfx_method_supported(4) == 0
    assert pkg.method_supported(pkg.METHOD_TRAPS)


def test_plan_defaults(pkg):
    rc, w = _plan(pkg, _cfg(pkg))
    assert rc == 0 and w == 15 * 10 * 3


@pytest.mark.parametrize("M,L,K", [(26, 3, 1), (16, 51, 16), (8, 101, 32), (40, 11, 6)])
@pytest.mark.parametrize("dyn", [0, 1, 2])
def test_plan_accepts(pkg, M, L, K, dyn):
    rc, w = _plan(pkg, _cfg(pkg, num_banks=M, traps_len=L, traps_dct_len=K, dyn=dyn))
    assert rc == 0 and w == M * K * (1 + dyn)


@pytest.mark.parametrize("kw", [
    dict(ceps_len=13),
    dict(want_c0=1),
    dict(traps_len=30),
    dict(traps_len=1),
    dict(traps_len=103),
    dict(traps_len=-31),
    dict(traps_dct_len=33, traps_len=51),
    dict(traps_dct_len=-1),
    dict(traps_len=5, traps_dct_len=6),   # K > L
    dict(traps_len=9),                    # K > L after the default K = 10 is applied
    dict(num_banks=26, traps_dct_len=10),  # M K = 260
], ids=lambda kw: ",".join("%s=%s" % kv for kv in kw.items()))
def test_plan_refuses(pkg, kw):
    rc, _ = _plan(pkg, _cfg(pkg, **kw))
    assert rc == -5


def test_plan_accepts_zero_lifter(pkg):
    rc, w = _plan(pkg, _cfg(pkg, lift_coef=0.0))  # ignored for TRAPS (the MFCC path refuses it only with a DCT)
    assert rc == 0 and w == 450


def test_other_methods_ignore_the_traps_fields(pkg):
    for meth, nc in ((pkg.METHOD_MFCC, 13), (pkg.METHOD_PLP, 13)):
        rc, w = _plan(pkg, _cfg(pkg, method=meth, ceps_len=nc, num_banks=26, traps_len=30, traps_dct_len=77))
        assert rc == 0 and w == 13 * 3


def test_traps_runs_the_fbank_front_end(pkg):
    """One row of KERNEL_TABLE per front-end kernel, in its log-energy form: TRAPS plans the same kernel."""
    seen = {}
    for what, kw, kernel in pkg.mfcc.KERNEL_TABLE:
        kw = dict(kw, ceps_len=0, want_c0=False)
        try:
            fbank = pkg.plan_kernel(**kw)
        except pkg.MfxError:
            continue
        if fbank in seen:
            continue
        K = max(1, min(10, 256 // kw["num_banks"]))
        seen[fbank] = what
        assert pkg.plan_kernel(method=pkg.METHOD_TRAPS, traps_dct_len=K, **kw) == fbank, what
    assert set(seen) == {"k_front512", "k_front1024", "k_front2048", "k_front_reg", "k_front_wave"}, seen


@pytest.mark.parametrize("L,K", [(31, 10), (3, 1), (3, 3), (51, 16), (101, 32), (11, 6)])
def test_host_basis_equals_oracle(pkg, L, K):
    got = pkg.host_traps_basis(L, K)
    want = traps_ref.basis(L, K)
    assert got.shape == (K, L) and got.dtype == np.float32
    np.testing.assert_allclose(got, want, rtol=1e-6, atol=1e-6 * np.abs(want).max())


@pytest.mark.parametrize("L", [3, 11, 31, 101])
def test_oracle_basis_is_orthonormal_without_the_window(L):
    B = traps_ref.basis(L, L, hamming=False)
    G = B @ B.T
    want = np.eye(L)
    want[0, 0] = 2.0  # the k = 0 row carries the c0 column's scale, sqrt(2 / L) instead of sqrt(1 / L)
    np.testing.assert_allclose(G, want, rtol=0, atol=1e-12)


def test_oracle_constant_trajectory():
    L, K, M, T, c = 31, 10, 4, 50, -7.25
    y = traps_ref.traps_statics(np.full((T, M), c), L, K).reshape(T, M, K)
    want = c * traps_ref.basis(L, K).sum(1)
    np.testing.assert_allclose(y, np.broadcast_to(want, y.shape), rtol=1e-12, atol=1e-12)


def test_oracle_clamps_like_the_delta_stage():
    """Frame t of a short utterance sees the first / last frame replicated: against a direct loop."""
    rng = np.random.default_rng(5)
    L, K, M, T = 11, 4, 3, 7
    x = rng.standard_normal((T, M))
    B = traps_ref.basis(L, K)
    y = traps_ref.traps_statics(x, L, K).reshape(T, M, K)
    for t in range(T):
        for m in range(M):
            u = np.array([x[min(max(t - 5 + j, 0), T - 1), m] for j in range(L)])
            np.testing.assert_allclose(y[t, m], B @ u, rtol=1e-12, atol=1e-12)
