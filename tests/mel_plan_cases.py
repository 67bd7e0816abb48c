"""Cases of the mel lane plan that tests/golden/mel_plan_parent.json pins (tests/golden/make_mel_plan_parent.py records them
from the parent commit's library, tests/test_host.py::test_mel_lane_plan_equals_parent compares the tree's): the corners where
the two builders that build_mel_plan replaced differed, or where a plan can break.

    lanes      16 / 32 / 64
    num_banks  1, lanes - 1, lanes, lanes + 1, 8 lanes (the last plan that fits), 8 lanes + 1 (refused: 9 rounds), and the
               project's 13, 23, 26, 40, 80, 128
    fft_size   64, 256, 512, 1024, 2048, 4096; max_read_bin as the kernels pass it: 479 (16 lanes, 512 points), 527 (16 lanes,
               1024 points: starts at multiples of 4 bins), 1039 (32 lanes, 2048 points), else fft_size - 1
    rate       8 / 16 / 44.1 / 48 kHz, filters from 64 Hz to half of it
    alpha      0.8 / 1.0 / 1.2
and, per lane count, one plan whose max_read_bin is too small for its last round (refused).

How they combine.  What the builders differed in -- lanes, the start alignment, the matching group, the number of candidates
-- and what bounds a plan -- the rounds, max_read_bin -- are functions of (lanes, num_banks, fft_size): that product is taken
whole (210 shapes, at 16 kHz and alpha 1).  Rate and alpha do one thing, they move the filter edges of the table the builder
is handed; all twelve (rate, alpha) pairs are taken at every (lanes, fft_size) with the project's 40 filters (a first round of
wide filters and, on 16 and 32 lanes, short later rounds).  411 cases (the full product of the five lists
would be 2520, a fixture of 280 KB of digests)."""
import ctypes as C
import hashlib

import numpy as np

LANES = (16, 32, 64)
FFTS = (64, 256, 512, 1024, 2048, 4096)
RATES = (8000.0, 16000.0, 44100.0, 48000.0)
ALPHAS = (0.8, 1.0, 1.2)


def max_read_bin(lanes, fft):
    return {(16, 512): 479, (16, 1024): 527, (32, 2048): 1039}.get((lanes, fft), fft - 1)


def cases():
    """(lanes, num_banks, fft_size, rate, alpha, max_read_bin), in a fixed order"""
    out = []
    for lanes in LANES:
        banks = sorted({1, lanes - 1, lanes, lanes + 1, 8 * lanes, 8 * lanes + 1, 13, 23, 26, 40, 80, 128})
        for fft in FFTS:
            for nb in banks:
                out.append((lanes, nb, fft, 16000.0, 1.0, max_read_bin(lanes, fft)))
            for sr in RATES:
                for alpha in ALPHAS:
                    if (sr, alpha) != (16000.0, 1.0):
                        out.append((lanes, 40, fft, sr, alpha, max_read_bin(lanes, fft)))
        out.append((lanes, 40, 512, 16000.0, 1.0, 100))  # the filters reach bin 256
    return out


def key(case):
    return "lanes%d_nb%d_fft%d_sr%g_a%g_max%d" % case


def plan_digest(lib, case):
    """(return code of mfx_host_mel_lane_plan, SHA-256 over L[8], row_stride, start, fid, w -- None where it refuses)"""
    lanes, nb, fft, sr, alpha, max_read = case
    ip, fpt = C.POINTER(C.c_int32), C.POINTER(C.c_float)
    wt, beg = np.zeros((2, fft), np.float32), np.zeros(nb + 2, np.int32)
    lib.mfx_host_mel_table.argtypes = [C.c_int32, C.c_int32, C.c_float, C.c_float, C.c_float, C.c_float, fpt, ip]
    lib.mfx_host_mel_table.restype = C.c_int
    rc = lib.mfx_host_mel_table(nb, fft, sr, 64.0, sr / 2, alpha, wt.ctypes.data_as(fpt), beg.ctypes.data_as(ip))
    assert rc == 0, (case, rc)
    fn = lib.mfx_host_mel_lane_plan
    fn.argtypes = [C.c_int32, C.c_int32, C.c_int32, fpt, ip, C.c_int32, ip, ip, ip, ip, fpt, C.c_int64]
    fn.restype = C.c_int
    L, rs = np.zeros(8, np.int32), C.c_int32(0)
    head = (lanes, nb, fft, wt.ctypes.data_as(fpt), beg.ctypes.data_as(ip), max_read, L.ctypes.data_as(ip), C.byref(rs))
    rounds = fn(*head, None, None, None, 0)
    if rounds < 0:
        return rounds, None
    start, fid = np.zeros((rounds, lanes), np.int32), np.zeros((rounds, lanes), np.int32)
    w = np.zeros((lanes, rs.value), np.float32)
    rc = fn(*head, start.ctypes.data_as(ip), fid.ctypes.data_as(ip), w.ctypes.data_as(fpt), w.size)
    assert rc == rounds, (case, rc, rounds)
    h = hashlib.sha256()
    for part in (L, np.int32(rs.value), start, fid, w):
        h.update(np.ascontiguousarray(part).tobytes())
    return rounds, h.hexdigest()
