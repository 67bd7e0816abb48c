"""Host side of the STFT log-mel front end (MFX_METHOD_STFT_LOGMEL): the oracle of tests/stft_ref.py against torch.stft, the
library's host-built tables and frame rule against the oracle, the configuration rules, the planning handle.  No GPU."""
import ctypes as C

import numpy as np
import pytest
import torch

import stft_ref


# ---- the oracle's framing + DFT against torch.stft -------------------------------------------------------------------

STFT_SHAPES = [(400, 160), (64, 48), (510, 1)]


@pytest.mark.parametrize("N,S", STFT_SHAPES)
def test_oracle_matches_torch_stft(pkg, N, S):
    win = pkg.periodic_hann(N)
    lengths = sorted({N // 2 + 1, N // 2 + 2, N, max(S, N // 2 + 1), 3 * S - 1 + N, 3 * S + N, 3 * S + 1 + N, 7 * S + N // 2 + 1}
                     | ({S * (N // (2 * S) + 1)} if S > 1 else set()))
    rng = np.random.default_rng(N + S)
    for n in lengths:
        pcm = rng.integers(-32768, 32768, n).astype(np.int16)
        re, im = stft_ref.dft(pcm, win, S)
        x = torch.from_numpy(pcm.astype(np.float64) / 32768.0)
        X = torch.stft(x, N, hop_length=S, window=torch.from_numpy(win.astype(np.float64)), center=True, pad_mode="reflect",
                       return_complex=True)[..., :-1].numpy().T
        assert X.shape[0] == 1 + n // S - 1 == stft_ref.frame_count(n, N, S) == re.shape[0], (n, X.shape)
        # (the oracle's basis is the float32 one: 2^-24 relative per tap, N taps of at most 1)
        if re.size:
            assert np.abs(re - X.real).max() <= 1e-6 * N and np.abs(im - X.imag).max() <= 1e-6 * N, n
    assert stft_ref.frame_count(N // 2, N, S) == 0 and stft_ref.frame_count(0, N, S) == 0


# ---- host tables -----------------------------------------------------------------------------------------------------

def ulp_diff(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


MEL_SHAPES = [(80, 400, 16000.0, 0.0, 8000.0), (128, 400, 16000.0, 0.0, 8000.0), (8, 64, 16000.0, 0.0, 8000.0),
              (20, 64, 16000.0, 100.0, 7000.0), (80, 512, 16000.0, 0.0, 8000.0), (40, 510, 16000.0, 50.0, 7600.0),
              (1, 32, 16000.0, 0.0, 8000.0), (40, 200, 8000.0, 0.0, 4000.0), (128, 64, 16000.0, 0.0, 8000.0)]


@pytest.mark.parametrize("M,N,sr,lo,hi", MEL_SHAPES)
def test_slaney_table_against_oracle(pkg, M, N, sr, lo, hi):
    w, beg, ln = pkg.host_slaney_mel_table(M, N, sr, lo, hi)
    rw, rbeg, rln = stft_ref.mel_table(M, N, sr, lo, hi)
    assert w.shape == rw.shape == (M, N // 2 + 1)
    assert ulp_diff(w, rw).max() <= 1
    assert np.array_equal(ln, rln) and np.array_equal(beg[ln > 0], rbeg[rln > 0])
    for m in range(M):   # nothing outside the span, nothing zero inside it
        assert not w[m, :beg[m]].any() and not w[m, beg[m] + ln[m]:].any() and (w[m, beg[m]:beg[m] + ln[m]] > 0).all()
    # area of EVERY row with a non-empty span: a unit-area triangle sampled every df = sr / N Hz.  The sum of the samples times
    # df is the trapezoid rule (the function is 0 at both ends of the grid), which is linear in the function and exact on
    # straight pieces: a kink of slope jump J at the fraction th of a grid cell costs J df^2 th (1 - th) / 2 <= J df^2 / 8,
    # wherever it lies and however many share a cell.  The triangle of flanks a, b and height h = 2 / (a + b) has three kinks
    # of total |J| = 2 h (1 / a + 1 / b): the bound is df^2 / (2 a b), i.e. (df / width)^2 -- tight for wide bands, and still
    # a statement (0.58 at 37-Hz flanks on a 40-Hz grid) for bands narrower than a bin.  1e-6: the table's float32 rounding
    p = stft_ref.mel_to_hz(float(stft_ref.hz_to_mel(lo)) + (float(stft_ref.hz_to_mel(hi)) - float(stft_ref.hz_to_mel(lo))) *
                           np.arange(M + 2) / (M + 1))
    df = sr / N
    checked = 0
    for m in range(M):
        a, b = p[m + 1] - p[m], p[m + 2] - p[m + 1]
        if ln[m] == 0:
            assert df * df / (2.0 * a * b) >= 1.0 - 1e-6, m     # (no sample inside the triangle: only where the bound allows it)
            continue
        area = float(w[m].astype(np.float64).sum()) * df
        bound = df * df / (2.0 * a * b) + 1e-6
        assert abs(area - 1.0) <= bound, (m, area, bound)
        checked += 1
    assert checked == int((ln > 0).sum())
    if (M, N) == (80, 400):
        assert checked == 80


def test_slaney_table_pins(pkg):
    w, beg, ln = pkg.host_slaney_mel_table(80, 400, 16000.0, 0.0, 8000.0)
    assert abs(float(w.max()) - 0.025880684545) < 2e-9
    assert beg[0] == 1 and ln[0] == 1 and np.count_nonzero(w[0]) == 1


@pytest.mark.parametrize("N", [32, 64, 400, 510, 512])
def test_stft_basis_against_oracle(pkg, N):
    rng = np.random.default_rng(N)
    for win in (pkg.periodic_hann(N), rng.standard_normal(N).astype(np.float32)):
        b = pkg.host_stft_basis(win)
        assert b.shape == (2, N // 2 + 1, N)
        assert ulp_diff(b, stft_ref.basis(win)).max() <= 1   # cos / sin of the exactly reduced argument, one rounding


def test_periodic_hann(pkg):
    for n in (32, 400, 510):
        assert np.abs(pkg.periodic_hann(n).astype(np.float64) - torch.hann_window(n, dtype=torch.float64).numpy()).max() < 1e-7
    assert pkg.periodic_hann(400)[0] == 0.0 and pkg.periodic_hann(400)[200] == 1.0


@pytest.mark.parametrize("N,S", [(400, 160), (64, 48), (510, 1), (32, 32), (512, 128)])
def test_stft_frame_count(pkg, N, S):
    k = 7
    for n in (0, N // 2, N // 2 + 1, S - 1, S, k * S - 1, k * S, (1 << 31) + 5, (1 << 40) + 3):
        assert pkg.stft_frame_count(n, N, S) == stft_ref.frame_count(n, N, S), n
    L = pkg.load_library()
    for bad in ((-1, N, S), (10, N + 1, S), (10, 30, 10), (10, 514, 10), (10, N, 0), (10, N, N + 1)):
        assert L.mfx_host_stft_frame_count(*bad) == -7


# ---- LDS of k_stft_mel over the whole of the method's limits --------------------------------------------------------------

def test_lds_fits_for_every_shape(pkg):
    """For every (N, S) inside the limits and M at its ends: the tile mfx_create takes is the largest of 64 / 32 / 16 whose
    block -- operand buffers, span or finished rows, power rows and the four reduction words, ALL the LDS the kernel uses --
    stays within the 160 KB a gfx950 block may ask for, and one always does (restated here from the layout in mfx_stft.hip)."""
    L = pkg.load_library()
    cap = 160 * 1024

    def need(N, S, M, R):
        K1 = N // 2 + 1
        tb = min((K1 + 15) // 16, 13)
        bufs = 2 * (2 * 2 * tb * 64)
        xo = (max((R - 1) * S + N + 4, R * M) + 3) & ~3
        return 4 * (bufs + xo + R * (K1 | 1) + 4)

    r = C.c_int32(0)
    at_cap = 0
    for N in range(32, 513, 2):
        for S in range(1, N + 1):
            for M in (1, 128):
                got = L.mfx_host_stft_lds_bytes(N, S, M, C.byref(r))
                want_r = next(R for R in (64, 32, 16) if need(N, S, M, R) <= cap)
                assert (r.value, got) == (want_r, need(N, S, M, want_r)) and got <= cap, (N, S, M, r.value, got)
                at_cap += got > cap - 64
    assert at_cap > 0      # (the walk does reach shapes within a few words of the cap)
    for N, S in ((394, 336), (396, 336), (436, 315), (478, 292), (480, 292)):   # 64 rows would need cap + 16 bytes
        assert L.mfx_host_stft_lds_bytes(N, S, 80, C.byref(r)) <= cap and r.value == 32
    assert L.mfx_host_stft_lds_bytes(400, 160, 80, C.byref(r)) == 120032 and r.value == 64
    assert L.mfx_host_stft_lds_bytes(512, 512, 128, C.byref(r)) == 125088 and r.value == 32
    for bad in ((30, 10, 8), (401, 10, 8), (400, 0, 8), (400, 401, 8), (400, 160, 0), (400, 160, 129)):
        assert L.mfx_host_stft_lds_bytes(*bad, None) == -7


# ---- the struct mirror, configuration rules, planning handle ---------------------------------------------------------

def test_struct_mirror_and_constants(pkg):
    fields = [f[0] for f in pkg.MfxConfig._fields_]
    assert fields[-1] == "logmel_post" and fields[-2] == "traps_dct_len"
    assert pkg.MfxConfig.logmel_post.offset == C.sizeof(pkg.MfxConfig) - 4
    assert pkg.METHOD_STFT_LOGMEL == 5 and (pkg.LOGMEL_WHISPER, pkg.LOGMEL_LOG10, pkg.LOGMEL_LN) == (0, 1, 2)


def test_method_supported(pkg):
    L = pkg.load_library()
    assert L.mfx_method_supported(5) == 1
    assert L.mfx_method_supported(4) == 0 and L.mfx_method_supported(2) == 0 and L.mfx_method_supported(6) == 0
    assert pkg.method_supported(pkg.METHOD_STFT_LOGMEL)


def cfg(pkg, **kw):
    c = pkg.MfxConfig()
    c.input_buffer_size, c.window_size, c.shift, c.num_banks = 200000, 400, 160, 80
    c.sample_rate, c.low_freq, c.high_freq = 16000.0, 0.0, 8000.0
    c.lift_coef, c.delta_l1, c.delta_l2, c.norm_after_dyn, c.channels = 22.0, 3, 3, 1, 1
    c.method = pkg.METHOD_STFT_LOGMEL
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def plan(pkg, c):
    L = pkg.load_library()
    h = C.c_void_p()
    rc = L.mfx_plan_create(C.byref(c), C.byref(h))
    return rc, h


BAD = [dict(window_size=401), dict(window_size=30), dict(window_size=514), dict(fft_size=512), dict(shift=0), dict(shift=401),
       dict(num_banks=0), dict(num_banks=129), dict(low_freq=-1.0), dict(low_freq=8000.0), dict(high_freq=8000.5),
       dict(ceps_len=13), dict(want_c0=1), dict(dyn=1), dict(dyn=2), dict(norm=1), dict(norm=2), dict(norm=3), dict(channels=2),
       dict(logmel_post=3), dict(logmel_post=-1)]


@pytest.mark.parametrize("kw", BAD, ids=[repr(b) for b in BAD])
def test_configuration_errors(pkg, kw):
    rc, h = plan(pkg, cfg(pkg, **kw))
    assert rc == -5 and not h.value


GOOD = [dict(), dict(fft_size=400), dict(channels=0), dict(window_size=32, shift=32, num_banks=1), dict(window_size=512, shift=512, num_banks=128),
        dict(window_size=512, shift=1, num_banks=128), dict(window_size=510, shift=170, num_banks=40), dict(shift=400),
        dict(lift_coef=0.0, delta_l1=0, delta_l2=-4, bug_compat=1), dict(logmel_post=1), dict(logmel_post=2),
        dict(sample_rate=8000.0, high_freq=4000.0, window_size=200, shift=80, num_banks=40)]


@pytest.mark.parametrize("kw", GOOD, ids=[repr(g) for g in GOOD])
def test_planning_handle_answers(pkg, kw):
    L = pkg.load_library()
    c = cfg(pkg, **kw)
    rc, h = plan(pkg, c)
    assert rc == 0
    try:
        assert L.mfx_get_output_data_width(h) == c.num_banks
        assert L.mfx_fft_size(h) == c.window_size
        assert L.mfx_dominant_kernel_name(h) == b"k_stft_mel"
        for n in (0, c.window_size // 2, c.window_size // 2 + 1, 16000):
            assert L.mfx_batch_frames(h, n) == stft_ref.frame_count(n, c.window_size, c.shift)
        # every entry that needs the device, the streaming ones included, answers as on any planning handle
        n = C.c_int32(0)
        pcm = np.zeros(16, np.int16)
        assert L.mfx_set_input(h, pcm.ctypes.data_as(C.POINTER(C.c_int16)), 16, C.byref(n)) == -6
        assert L.mfx_flush(h, C.byref(n)) == -6
        assert L.mfx_apply(h) == -6
        assert L.mfx_sessions_create(h, 1, 160) == -6
        assert L.mfx_set_window(h, pkg.periodic_hann(c.window_size).ctypes.data_as(C.POINTER(C.c_float))) == -6
    finally:
        L.mfx_destroy(h)


def test_other_methods_ignore_logmel_post(pkg):
    """logmel_post is read by method 5 only: a value outside its range does not disturb an MFCC configuration."""
    L = pkg.load_library()
    c = cfg(pkg, method=pkg.METHOD_MFCC, num_banks=26, ceps_len=13, low_freq=64.0, logmel_post=77)
    rc, h = plan(pkg, c)
    assert rc == 0
    assert L.mfx_dominant_kernel_name(h) == b"k_front512" and L.mfx_fft_size(h) == 512
    L.mfx_destroy(h)
