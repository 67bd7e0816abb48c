"""Helpers the GPU suites of the STFT log-mel front end share (tests/test_stft_gpu.py, test_stft_fft_gpu.py,
test_stft_edge_gpu.py, stft_bits_cases.py): handles, the float64 oracle, the batch layout, one run through the host entry, the
comparison at the project bar, bit comparisons and the hard inputs -- and one record per form of the front end (MATRIX:
k_stft_mel, N <= 512; FFT: k_stft_fft_mel, N = 1024 / 2048) with its default shape, its oracle module and its tile helper.
Test infrastructure only."""
import ctypes as C

import numpy as np

import stft_fft_ref
import stft_ref
from conftest import assert_close, synth_utterance


def make(pkg, N, S, M, sr, low=0.0, high=None, window=None, post=0, ibs=200000, engine=0):
    """An STFT log-mel handle under `window` (None: the periodic Hann)."""
    m = pkg.MfccHip(ibs, N, S, M, sr, low, sr / 2 if high is None else high, 0, False, 22.0, device=0, bug_compat=False,
                    method=pkg.METHOD_STFT_LOGMEL, logmel_post=post, engine=engine)
    m.set_window(pkg.periodic_hann(N) if window is None else window)
    return m


class Form:
    """One form of the front end: `shape` (N, S, M, sr) is where most of its tests run, `ref` its float64 oracle module,
    `tiles` the frames per block its kernel can take, `lds_entry` the library's inspection entry that names the tile."""

    def __init__(self, name, shape, ref, tiles, lds_entry, ibs):
        self.name, self.shape, self.ref, self.tiles, self.lds_entry, self.ibs = name, shape, ref, tiles, lds_entry, ibs

    def _shape(self, N, S, M, sr):
        d = self.shape
        return d[0] if N is None else N, d[1] if S is None else S, d[2] if M is None else M, d[3] if sr is None else sr

    def make(self, pkg, N=None, S=None, M=None, sr=None, low=0.0, high=None, window=None, post=0, ibs=None, engine=0):
        N, S, M, sr = self._shape(N, S, M, sr)
        return make(pkg, N, S, M, sr, low, high, window, post, self.ibs if ibs is None else ibs, engine)

    def oracle(self, pkg, pcm, N=None, S=None, M=None, sr=None, low=0.0, high=None, window=None, post=0):
        N, S, M, sr = self._shape(N, S, M, sr)
        return self.ref.logmel(pcm, pkg.periodic_hann(N) if window is None else window, S, M, sr, low, sr / 2 if high is None else high,
                               post)

    def block_rows(self, pkg, N, S, M):
        """Frames per block of the form's kernel at the shape, as the library answers."""
        r = C.c_int32(0)
        assert getattr(pkg.load_library(), self.lds_entry)(int(N), int(S), int(M), C.byref(r)) > 0
        assert r.value in self.tiles
        return r.value


MATRIX = Form("matrix", (400, 160, 80, 16000.0), stft_ref, (64, 32, 16), "mfx_host_stft_lds_bytes", 200000)
FFT = Form("fft", stft_fft_ref.SHAPES[0], stft_fft_ref, stft_fft_ref.TILES, "mfx_host_stft_fft_lds_bytes", 400000)


def form_of(N):
    return FFT if N in (1024, 2048) else MATRIX


def layout(utts, first=0):
    lens = np.array([u.size for u in utts], np.int64)
    offs = first + np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
    pcm = np.concatenate([np.zeros(first, np.int16)] + list(utts) + [np.zeros(2, np.int16)])
    return offs, lens, pcm


def run_batch(m, utts, first=0):
    offs, lens, pcm = layout(utts, first)
    rows, total = m.batch_plan(offs, lens)
    out = m.batch_run_host(pcm)
    return [out[rows[i]:rows[i] + m.batch_frames(int(lens[i]))] for i in range(len(utts))]


def check(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, "%s: shape %s vs %s" % (what, got.shape, want.shape)
    if want.size == 0:
        return 0.0
    scale = max(np.abs(want).max(), 1e-30)
    emax = np.abs(got.astype(np.float64) - want).max() / scale
    el2 = np.linalg.norm(got - want) / max(np.linalg.norm(want), 1e-30)
    print("%s: max err / scale = %.3g, rel L2 = %.3g (scale %.3g)" % (what, emax, el2, scale))
    assert_close(got, want, what)
    return emax


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def same_bits(a, b):
    a, b = bits(a), bits(b)
    return a.shape == b.shape and np.array_equal(a, b)


def hard_inputs():
    n = 20800
    t = np.arange(n)
    rng = np.random.default_rng(5)
    imp_mid = np.zeros(n, np.int16)
    imp_mid[n // 2] = 32767
    imp_ends = np.zeros(n, np.int16)
    imp_ends[0], imp_ends[-1] = 32767, -32768
    return {
        "silence": np.zeros(n, np.int16),
        "full-scale tone": np.round(32767.0 * np.sin(2 * np.pi * 1000.0 * t / 16000.0)).astype(np.int16),
        "clipped noise": np.clip(np.round(40000.0 * rng.standard_normal(n)), -32768, 32767).astype(np.int16),
        "quiet": (synth_utterance(n, 31).astype(np.int32) // 512).astype(np.int16),
        "impulse at the centre": imp_mid,
        "impulses at both ends": imp_ends,
    }
