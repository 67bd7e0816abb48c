"""Host side of the FFT form of the STFT log-mel front end (MFX_METHOD_STFT_LOGMEL at N = 1024 / 2048): the oracle of
tests/stft_fft_ref.py against torch.stft, planning handles and what stays refused, the Slaney and FFT tables, the LDS sum that
picks the tile of k_stft_fft_mel, the kernel's resource usage when compiled for gfx950, the stand-alone sanitizer program.
No GPU."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import stft_fft_ref as FR
import stft_ref
from conftest import synth_utterance

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "asr-featext-opencl_amd", "csrc")


# ---- the oracle against torch.stft -------------------------------------------------------------------------------------

@pytest.mark.parametrize("N,S,win", [(1024, 256, "hann"), (2048, 512, "short"), (1024, 160, "short"), (2048, 441, "ramp")])
def test_oracle_matches_torch_stft(N, S, win):
    """Framing, window and DFT of the oracle are torch.stft(center=True, pad_mode="reflect") in float64 with the last frame
    dropped; the short window is the one torch.stft builds from win_length < n_fft."""
    w = FR.windows(N)[win]
    rng = np.random.default_rng(N + S)
    for n in (N // 2 + 1, N, 3 * S + N + 1, 7 * S + N // 2 + 1):
        pcm = rng.integers(-32768, 32768, n).astype(np.int16)
        x = torch.from_numpy(pcm.astype(np.float64) / 32768.0)
        if win == "short":
            L = {1024: 800, 2048: 1200}[N]
            X = torch.stft(x, N, hop_length=S, win_length=L, window=torch.hann_window(L, dtype=torch.float64), center=True,
                           pad_mode="reflect", return_complex=True)
            tol = 1e-6 * N      # (the oracle's window is the float32 one: 2^-24 relative per tap, N taps of at most 1)
        else:
            X = torch.stft(x, N, hop_length=S, window=torch.from_numpy(w.astype(np.float64)), center=True, pad_mode="reflect",
                           return_complex=True)
            tol = 1e-9 * N
        P = (X.abs() ** 2)[..., :-1].numpy().T
        got = FR.power(pcm, w, S)
        assert got.shape == P.shape == (stft_ref.frame_count(n, N, S), N // 2 + 1), (n, got.shape, P.shape)
        if P.size:
            assert np.abs(np.sqrt(got) - np.sqrt(P)).max() <= tol, (n, np.abs(np.sqrt(got) - np.sqrt(P)).max())


def test_oracle_agrees_with_the_basis_rounded_one():
    """Below N = 512 both oracles exist: the exact transform and the sum over the float32 basis differ by the basis rounding."""
    pcm = synth_utterance(6000, 3)
    w = FR.stft_edge.periodic_hann(400)
    a = FR.logmel(pcm, w, 160, 80, 16000.0, 0.0, 8000.0)
    b = stft_ref.logmel(pcm, w, 160, 80, 16000.0, 0.0, 8000.0)
    assert np.abs(a - b).max() <= 1e-6 * np.abs(b).max()


# ---- planning handles and refusals ---------------------------------------------------------------------------------------

def cfg(pkg, **kw):
    c = pkg.MfxConfig()
    c.input_buffer_size, c.window_size, c.shift, c.num_banks = 400000, 1024, 256, 80
    c.sample_rate, c.low_freq, c.high_freq = 22050.0, 0.0, 11025.0
    c.lift_coef, c.delta_l1, c.delta_l2, c.norm_after_dyn, c.channels = 22.0, 3, 3, 1, 1
    c.method = pkg.METHOD_STFT_LOGMEL
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def plan(pkg, c):
    h = C.c_void_p()
    return pkg.load_library().mfx_plan_create(C.byref(c), C.byref(h)), h


GOOD = [dict(), dict(fft_size=1024), dict(window_size=2048, shift=512, num_banks=128, sample_rate=44100.0, high_freq=22050.0),
        dict(window_size=2048, fft_size=2048, shift=2048, num_banks=1), dict(shift=1024, num_banks=128), dict(shift=1, num_banks=8),
        dict(window_size=2048, shift=441, num_banks=64), dict(logmel_post=1), dict(logmel_post=2)]


@pytest.mark.parametrize("kw", GOOD, ids=[repr(g) for g in GOOD])
def test_planning_handle_answers(pkg, kw):
    L = pkg.load_library()
    c = cfg(pkg, **kw)
    rc, h = plan(pkg, c)
    assert rc == 0
    try:
        assert L.mfx_get_output_data_width(h) == c.num_banks
        assert L.mfx_fft_size(h) == c.window_size
        assert L.mfx_dominant_kernel_name(h) == b"k_stft_fft_mel"
        for n in (0, c.window_size // 2, c.window_size // 2 + 1, c.window_size, 50000):
            assert L.mfx_batch_frames(h, n) == stft_ref.frame_count(n, c.window_size, c.shift)
        assert L.mfx_sessions_create(h, 1, 160) == -6
    finally:
        L.mfx_destroy(h)


BAD = [dict(window_size=n) for n in (514, 768, 1022, 1026, 1536, 2046, 2050, 4096, 1023, 1025)] + \
      [dict(fft_size=2048), dict(fft_size=512), dict(window_size=2048, fft_size=1024), dict(shift=1025), dict(window_size=2048, shift=2049),
       dict(shift=0), dict(num_banks=129), dict(num_banks=0), dict(ceps_len=13), dict(dyn=1), dict(norm=1), dict(channels=2),
       dict(logmel_post=3), dict(high_freq=11025.5)]


@pytest.mark.parametrize("kw", BAD, ids=[repr(b) for b in BAD])
def test_configuration_errors(pkg, kw):
    rc, h = plan(pkg, cfg(pkg, **kw))
    assert rc == -5 and not h.value


def test_symbols_are_declared_and_exported(pkg):
    L = pkg.load_library()
    header = open(os.path.join(ROOT, "include", "mfx.h")).read()
    for name in ("mfx_host_stft_fft_tables", "mfx_host_stft_fft_lds_bytes"):
        assert name in pkg.mfcc.EXPORTED_SYMBOLS and hasattr(L, name)
        assert re.search(r"\b%s\(" % name, header), name
    assert L.mfx_abi_version() == 2
    assert hasattr(pkg, "host_stft_fft_tables") and hasattr(pkg, "host_stft_fft_lds_bytes")


def test_matrix_form_helpers_still_refuse(pkg):
    """mfx_host_stft_basis, mfx_host_stft_lds_bytes, mfx_host_session_stft_step and mfx_host_sess_stft_lds_bytes describe the
    matrix kernels; the frame rule and the Slaney table serve both forms, and nothing else."""
    L = pkg.load_library()
    fpt = C.POINTER(C.c_float)
    for N in (1024, 2048):
        w, out = np.ones(N, np.float32), np.zeros(8, np.float32)      # (refused before anything is written)
        assert L.mfx_host_stft_basis(N, w.ctypes.data_as(fpt), out.ctypes.data_as(fpt)) == -7 and not out.any()
        assert L.mfx_host_stft_lds_bytes(N, 256, 80, None) == -7
        st = (C.c_int64 * 2)(0, 0)
        assert L.mfx_host_session_stft_step(N, 256, st, 100, 0, None, None) == -7
        assert L.mfx_host_sess_stft_lds_bytes(N, 256, 80, None) == -7
        assert L.mfx_host_stft_frame_count(10 * N + 3, N, N // 4) == (10 * N + 3) // (N // 4)
        assert L.mfx_host_stft_frame_count(N // 2, N, 1) == 0 and L.mfx_host_stft_frame_count(N // 2 + 1, N, 1) == N // 2 + 1
    for bad in ((10, 514, 10), (10, 1026, 10), (10, 1536, 10), (10, 4096, 10), (10, 1024, 1025), (10, 1024, 0), (-1, 1024, 256)):
        assert L.mfx_host_stft_frame_count(*bad) == -7
    for N in (514, 1536, 4096):
        assert L.mfx_host_stft_fft_lds_bytes(N, 1, 8, None) == -7
        with pytest.raises(pkg.MfxError):
            pkg.host_stft_fft_tables(N)
        with pytest.raises(pkg.MfxError):
            pkg.host_slaney_mel_table(8, N, 16000.0, 0.0, 8000.0)
    for bad in ((1024, 0, 8), (1024, 1025, 8), (1024, 256, 0), (1024, 256, 129)):
        assert L.mfx_host_stft_fft_lds_bytes(*bad, None) == -7


# ---- tables ----------------------------------------------------------------------------------------------------------------

def ulp_diff(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


@pytest.mark.parametrize("M,N,sr,lo,hi", [(80, 1024, 22050.0, 0.0, 11025.0), (128, 2048, 44100.0, 0.0, 22050.0), (128, 1024, 16000.0, 0.0, 8000.0),
                                          (1, 2048, 16000.0, 0.0, 8000.0), (64, 2048, 44100.0, 50.0, 20000.0), (8, 1024, 16000.0, 0.0, 8000.0)])
def test_slaney_table_bits(pkg, M, N, sr, lo, hi):
    w, beg, ln = pkg.host_slaney_mel_table(M, N, sr, lo, hi)
    rw, rbeg, rln = stft_ref.mel_table(M, N, sr, lo, hi)
    assert w.shape == rw.shape == (M, N // 2 + 1)
    assert ulp_diff(w, rw).max() == 0
    assert np.array_equal(ln, rln) and np.array_equal(beg[ln > 0], rbeg[rln > 0]) and (ln > 0).all()


@pytest.mark.parametrize("N", [1024, 2048])
def test_fft_tables_against_the_double_formula(pkg, N):
    twid, split = pkg.host_stft_fft_tables(N)
    M = N // 2
    assert twid.shape == (M,) and split.shape == (M + 1,) and twid.dtype == split.dtype == np.complex64
    a = -2.0 * np.pi * np.arange(M, dtype=np.float64) / M
    b = -2.0 * np.pi * np.arange(M + 1, dtype=np.float64) / N
    want_t = (np.cos(a) + 1j * np.sin(a)).astype(np.complex64)                 # W_M^k
    want_s = (np.sin(b) - 1j * np.cos(b)).astype(np.complex64)                 # -i W_N^k
    for got, want in ((twid, want_t), (split, want_s)):
        big = np.abs(want.view(np.float32)) > 1e-12      # (cos / sin at their zeros: 6e-17 either way, no ulp to count)
        assert ulp_diff(got.view(np.float32), want.view(np.float32))[big].max() <= 1
        assert np.abs(got.view(np.float32) - want.view(np.float32))[~big].max() <= 1e-15
    # the real split with these tables, in double on an exact half-length FFT, is the DFT of the real frame
    rng = np.random.default_rng(N)
    z = rng.standard_normal(N)
    Z = np.fft.fft(z[0::2] + 1j * z[1::2])
    k = np.arange(M + 1)
    zk, zm = Z[k % M], np.conj(Z[(M - k) % M])
    X = 0.5 * ((zk + zm) + split.astype(np.complex128) * (zk - zm))
    assert np.abs(X - np.fft.rfft(z)).max() <= 1e-6 * np.abs(np.fft.rfft(z)).max()


def test_lds_fits_for_every_shape(pkg):
    """For both N, every S in 1 .. N and M at its ends: the tile mfx_create takes is the largest of 16 / 8 / 4 whose block --
    span or finished rows, window, twiddles, four FFT buffers, power rows and the four reduction words, ALL the LDS the kernel
    uses (restated in stft_fft_ref.lds_bytes from the layout in mfx_stft_fft.hip) -- stays within the 160 KB a gfx950 block may
    ask for, and 4 frames always do."""
    L = pkg.load_library()
    r = C.c_int32(0)
    seen = set()
    for N in (1024, 2048):
        for S in range(1, N + 1):
            for M in (1, 128):
                got = L.mfx_host_stft_fft_lds_bytes(N, S, M, C.byref(r))
                want_r = FR.tile_rows(N, S, M)
                assert 0 < got <= FR.LDS and (r.value, got) == (want_r, FR.lds_bytes(N, S, M, want_r)), (N, S, M, r.value, got)
                seen.add((N, r.value))
    assert seen == {(1024, 16), (2048, 16), (2048, 8)}    # (2048: 16 frames up to S = 681, 8 beyond; 4 is the list's reserve)
    assert pkg.host_stft_fft_lds_bytes(1024, 256, 80) == (76880, 16)          # under 80 KB: two blocks per CU
    assert pkg.host_stft_fft_lds_bytes(2048, 512, 128) == (153680, 16)
    assert pkg.host_stft_fft_lds_bytes(2048, 681, 1)[1] == 16 and pkg.host_stft_fft_lds_bytes(2048, 682, 1)[1] == 8
    assert pkg.host_stft_fft_lds_bytes(2048, 2048, 128) == (147504, 8)
    assert FR.lds_bytes(2048, 2048, 128, 4) == 98336


# ---- the kernel's build, the sanitizer program ---------------------------------------------------------------------------

def test_kernel_builds_for_gfx950_without_private_memory():
    """mfx_stft_fft.hip compiled for gfx950 as the Makefile compiles it: k_stft_fft_mel uses no scratch, keeps the two waves per
    SIMD its LDS allows at (1024, 256, 80), and the unit is one of KERNEL_TUS with an object rule."""
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"^KERNEL_TUS :=.*\bmfx_stft_fft\b", mk, re.M) and re.search(r"\bmfx_stft_fft\.o\b.*: %\.o: %\.hip", mk)
    hipcc = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    assert os.path.exists(hipcc), "hipcc (the compiler build() uses) was not found"
    r = subprocess.run([hipcc, "-O3", "-fPIC", "-std=c++17", "--offload-arch=gfx950", "-fno-slp-vectorize",
                        "-Rpass-analysis=kernel-resource-usage", "-c", "mfx_stft_fft.hip", "-o", os.devnull],
                       cwd=CSRC, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-2000:]
    names = re.findall(r"Function Name: (\S+)", r.stdout)
    scratch = [int(v) for v in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stdout)]
    occ = [int(v) for v in re.findall(r"Occupancy \[waves/SIMD\]: (\d+)", r.stdout)]
    lds = [int(v) for v in re.findall(r"LDS Size \[bytes/block\]: (\d+)", r.stdout)]
    assert len(scratch) == len(names) == len(occ) == len(lds)
    i = [k for k, n in enumerate(names) if "k_stft_fft_mel" in n]
    assert len(i) == 1, names
    assert scratch[i[0]] == 0 and occ[i[0]] >= 2 and lds[i[0]] == 0, (scratch[i[0]], occ[i[0]], lds[i[0]])   # (no static LDS)


def test_host_driver_runs_clean_under_the_sanitizers(tmp_path):
    """tools/asan/stft_fft_asan.cpp (the FFT tables, the Slaney table and the frame rule of mfx_tables.cpp at 1024 / 2048, and a
    restatement of the kernel's transform on them) as `make asan` builds and runs it: a stand-alone CPU program under
    AddressSanitizer + UBSan, linked against mfx_tables.cpp alone."""
    gxx = shutil.which("g++")
    assert gxx, "g++ was not found"
    exe = str(tmp_path / "stft_fft_asan")
    r = subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-ffp-contract=off", "-o", exe,
                        os.path.join(ROOT, "tools", "asan", "stft_fft_asan.cpp"), os.path.join(CSRC, "mfx_tables.cpp")],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-2000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env)
    assert r.returncode == 0 and "tables clean" in r.stdout, r.stdout[-2000:]
    assert "stft_fft_asan" in open(os.path.join(CSRC, "Makefile")).read()
