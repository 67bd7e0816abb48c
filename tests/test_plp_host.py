"""PLP on the CPU: the float64 oracle against independent formulations, and the library's configuration checks and
host tables (no GPU)."""
import ctypes as C

import numpy as np
import pytest

import plp_ref


def _cfg(pkg, **kw):
    base = dict(input_buffer_size=16000, window_size=400, shift=160, num_banks=40, sample_rate=16000.0, low_freq=64.0,
                high_freq=8000.0, ceps_len=13, want_c0=1, lift_coef=22.0, norm=0, dyn=2, delta_l1=3, delta_l2=3,
                norm_after_dyn=1, method=pkg.METHOD_PLP, lpc_order=12)
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


@pytest.mark.parametrize("p", [1, 2, 8, 12, 20])
def test_levinson_matches_solve_toeplitz(p):
    from scipy.linalg import solve_toeplitz
    rng = np.random.default_rng(p)
    for _ in range(5):
        A = np.cbrt(rng.uniform(1e-3, 1.0, 42))
        r = (A[None, :] @ plp_ref.idft_basis(40, p).T)[0]
        a, E = plp_ref.levinson(r, p)
        want = solve_toeplitz(r[:p], -r[1:p + 1])
        np.testing.assert_allclose(a[1:], want, rtol=1e-9, atol=1e-12)
        assert a[0] == 1.0
        np.testing.assert_allclose(E, r[0] + np.dot(a[1:], r[1:p + 1]), rtol=1e-9)


@pytest.mark.parametrize("p,C", [(8, 13), (12, 13), (12, 20), (20, 13), (1, 5)])
def test_cepstrum_of_model_spectrum(p, C):
    rng = np.random.default_rng(100 + p)
    A = np.cbrt(rng.uniform(1e-3, 1.0, 42))
    r = (A[None, :] @ plp_ref.idft_basis(40, p).T)[0]
    a, E = plp_ref.levinson(r, p)
    c = plp_ref.lpc_cepstrum(a, E, C)
    n = 4096
    model = E / np.abs(np.fft.rfft(a, n)) ** 2
    want = np.fft.irfft(np.log(model), n)[:C + 1]
    np.testing.assert_allclose(c, want, rtol=0, atol=1e-9 * max(1.0, np.abs(want).max()))


def test_autocorrelation_is_inverse_dft_of_even_spectrum():
    rng = np.random.default_rng(7)
    A = rng.uniform(0.1, 1.0, 27)
    r = plp_ref.idft_basis(25, 10) @ A
    full = np.concatenate([A, A[-2:0:-1]])  # real even sequence of length 2 (N - 1)
    want = np.fft.ifft(full).real[:11]
    np.testing.assert_allclose(r, want, rtol=1e-12, atol=1e-14)


def test_method_supported(pkg):
    L = pkg.load_library()
    assert L.mfx_method_supported(0) == 1
    assert L.mfx_method_supported(1) == 1
    assert L.mfx_method_supported(2) == 0
    assert L.mfx_method_supported(-1) == 0
    assert pkg.method_supported(pkg.METHOD_PLP)


@pytest.mark.parametrize("kw", [
    dict(),
    dict(want_c0=0, ceps_len=12, dyn=0),
    dict(lpc_order=0),
    dict(lpc_order=1, ceps_len=20),
    dict(lpc_order=32, num_banks=40),
    dict(lpc_order=26, num_banks=26, dyn=1),
    dict(window_size=200, shift=80, sample_rate=8000.0, high_freq=4000.0, num_banks=23, lpc_order=23),
    dict(window_size=2400, shift=480, sample_rate=48000.0, high_freq=24000.0, num_banks=64, lpc_order=24),
    dict(window_size=1102, shift=441, sample_rate=44100.0, high_freq=22050.0, num_banks=128, ceps_len=40, channels=2),
])
def test_plp_plan_accepts_and_matches_mfcc_width(pkg, kw):
    rc, w = _plan(pkg, _cfg(pkg, **kw))
    assert rc == 0
    rc0, w0 = _plan(pkg, _cfg(pkg, method=pkg.METHOD_MFCC, lpc_order=0, **{k: v for k, v in kw.items() if k != "lpc_order"}))
    assert rc0 == 0 and w == w0


def test_plp_plan_runs_spectrum_kernels(pkg):
    # PLP never takes a fused MFCC front end: the spectrum forms (k_front512 / the generic spectrum kernel) serve it
    assert pkg.plan_kernel(400, 160, 40, 16000.0, 13, dyn=2, method=pkg.METHOD_PLP, lpc_order=12) == "k_front512"
    assert pkg.plan_kernel(400, 160, 40, 16000.0, 13, fft_size=1024, method=pkg.METHOD_PLP) == "k_front_reg"
    assert pkg.plan_kernel(1102, 441, 128, 44100.0, 40, channels=2, method=pkg.METHOD_PLP) == "k_front_reg"


@pytest.mark.parametrize("kw", [
    dict(ceps_len=0),
    dict(lpc_order=-1),
    dict(lpc_order=33, num_banks=40),
    dict(lpc_order=27, num_banks=26),
    dict(lift_coef=0.0),
    dict(method=2),
    dict(method=-1),
])
def test_plp_plan_refuses(pkg, kw):
    rc, _ = _plan(pkg, _cfg(pkg, **kw))
    assert rc == -5


def test_zeroed_method_is_mfcc(pkg):
    cfg = _cfg(pkg, method=0, lpc_order=0, ceps_len=0)  # log mel energies: MFCC only
    rc, w = _plan(pkg, cfg)
    assert rc == 0 and w == 40 * 3


@pytest.mark.parametrize("nb,sr,low,high,p", [(40, 16000.0, 64.0, 8000.0, 12), (26, 16000.0, 0.0, 8000.0, 8),
                                              (23, 8000.0, 64.0, 4000.0, 1), (128, 44100.0, 64.0, 22050.0, 32),
                                              (64, 48000.0, 20.0, 20000.0, 24)])
@pytest.mark.parametrize("alpha", [0.88, 1.0, 1.12])
def test_host_plp_tables(pkg, nb, sr, low, high, p, alpha):
    eql, idft = pkg.host_plp_tables(nb, 512, sr, low, high, alpha, p)
    assert eql.shape == (nb,) and idft.shape == (p + 1, nb + 2)
    want_e = plp_ref.equal_loudness(nb, sr, low, high, alpha)
    np.testing.assert_allclose(eql, want_e, rtol=1e-6, atol=0)
    want_b = plp_ref.idft_basis(nb, p)
    np.testing.assert_allclose(idft, want_b, rtol=1e-6, atol=1e-6 * np.abs(want_b).max())
