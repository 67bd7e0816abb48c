"""Cases of tests/test_kaldi_bits_gpu.py, shared with tests/golden/make_kaldi_bits_parent.py (which recorded the rows of commit
b6732e9, the last one before the Kaldi kernels took their FFT stages, real split and mel-span chain from the pieces they share
with the STFT FFT form): one case per branch of k_kaldi_front and k_kaldi_front_opts -- the three DFT lengths (N = 128: 16 of 64
lanes hold a butterfly; N = 256: the radix-2 last stage; N = 512 with W < N and W = N), fbank and MFCC, the three frame options,
every flag of kaldi_flags with the energy floor off and at 1.0 -- under Povey's window and under the ramp of tests/kaldi_ref.py,
which is asymmetric: a changed tap order shows.

A case is one ragged batch of utterances with 0, 1, 15, 16, 17 and 33 frames (a chunk of 16 short by one, full, spilling into
the next, two chunks and one frame); the longest ends half a hop into the frame that would follow.  The utterances lie in one
PCM array between fillers of 3 full-scale samples that belong to none, so they start at odd and at even samples.  Under
NO_SNIP_EDGES the utterance of one frame is shorter than a window: its mirror wraps more than once.  Batch only: the session
rows are held to the batch twin's bits by tests/test_kaldi_sessions_gpu.py and tests/test_kaldi_opts_sessions_gpu.py."""
import numpy as np

from conftest import synth_utterance
from kaldi_drive import Shape, make
from stft_bits_cases import digests, shortest, shortest_bits  # noqa: F401  (what the fixture holds per case)

NSE, EN, WIN, HTK = 1, 2, 4, 8                          # kaldi_flags of mfx_create_kaldi (include/mfx.h)
FRAMES = (0, 1, 15, 16, 17, 33)
FILL = np.array([32767, -32767, 32767], np.int16)       # between the utterances, part of none


def _c(sh, flags=0, floor=0.0):
    return dict(shape=sh, flags=flags, floor=floor)


CASES = {}
# ---- k_kaldi_front: the three DFT lengths, fbank and MFCC, both windows
for W, S, M, C in ((65, 17, 5, 0), (128, 128, 23, 13),                              # N = 128
                   (200, 80, 40, 0), (256, 100, 23, 13),                            # N = 256
                   (400, 160, 80, 0), (400, 160, 23, 13), (512, 512, 128, 0)):      # N = 512, W < N and W = N
    for w in ("povey", "ramp"):
        CASES["%d_%d_%d_%d_%s" % (W, S, M, C, w)] = _c(Shape(W, S, M, C, window=w))
# ---- the three frame options
for tag, kw in (("preemph0", dict(preemph=0.0)), ("dc_kept", dict(remove_dc=False)), ("magnitude", dict(use_power=False))):
    CASES["400_160_80_0_ramp_" + tag] = _c(Shape(400, 160, 80, 0, window="ramp", **kw))
# ---- k_kaldi_front_opts: every flag; the energy floor where a flag reads it
for W, S, M, C in ((400, 160, 80, 0), (400, 160, 23, 13), (200, 80, 40, 0)):
    for flags in (NSE, EN, EN | WIN, EN | HTK, HTK, NSE | EN | WIN | HTK):
        if flags == HTK and C == 0:
            continue                # (without the energy column HTK_COMPAT moves nothing in an fbank row)
        for floor in (0.0, 1.0) if flags in (EN, NSE | EN | WIN | HTK) else (0.0,):
            CASES["%d_%d_%d_%d_ramp_f%d%s" % (W, S, M, C, flags, "_floor1" if floor else "")] = _c(Shape(W, S, M, C, window="ramp"), flags, floor)


def fft_size(W):
    return 128 if W <= 128 else 256 if W <= 256 else 512


def cols(c):
    """Floats of a row: the cepstra, or the bands and -- fbank under USE_ENERGY -- the energy column."""
    sh = c["shape"]
    return sh.C if sh.C else sh.M + (1 if c["flags"] & EN else 0)


def lengths(pkg, c):
    """Samples of the case's utterances, one per entry of FRAMES: the shortest length with T frames under the case's flags
    plus r < S samples (the longest: half a hop); T = 0: the longest length without a frame."""
    sh, snip = c["shape"], not c["flags"] & NSE
    W, S = sh.W, sh.S
    count = lambda n: pkg.host_kaldi_frame_count(n, W, S, c["flags"] & NSE)
    out = []
    for i, T in enumerate(FRAMES):
        first = (W + (T - 1) * S) if snip else (T * S - S // 2)       # the first length with T frames
        n = first + (S // 2 if T == max(FRAMES) else (3 * i + 1) % S) if T else (W - 1 if snip else S - S // 2 - 1)
        assert count(n) == T and (T == 0 or count(first) == T and count(first - 1) == T - 1), (W, S, c["flags"], T, n)
        out.append(n)
    assert snip or out[1] < W
    return out


def utterances(pkg, c):
    return [synth_utterance(n, 500 + 7 * i, sr=c["shape"].sr) for i, n in enumerate(lengths(pkg, c))]


def packed(utts):
    """offsets, lengths, pcm: the utterances with the fillers in front of, between and behind them."""
    parts, offs, at = [FILL], [], FILL.size
    for u in utts:
        offs.append(at)
        parts += [u, FILL]
        at += u.size + FILL.size
    return np.array(offs, np.int64), np.array([u.size for u in utts], np.int64), np.concatenate(parts)


def run_case(pkg, name):
    """The case's rows, one float32 array [frames][cols] per utterance."""
    c = CASES[name]
    offs, lens, pcm = packed(utterances(pkg, c))
    assert {int(o) & 1 for o in offs} == {0, 1}, (name, offs)
    m = make(pkg, c["shape"], flags=c["flags"], floor=c["floor"])
    try:
        rows, total = m.batch_plan(offs, lens)
        out = m.batch_run_host(pcm)
        assert out.shape == (total, cols(c)) and total == sum(FRAMES), (name, out.shape, total)
        got = [out[rows[i]:rows[i] + T] for i, T in enumerate(FRAMES)]
    finally:
        m.close()
    for g, T in zip(got, FRAMES):
        assert g.shape == (T, cols(c)), (name, g.shape, T)
        assert np.isfinite(g).all(), "%s: utterance of %d frames has non-finite values" % (name, T)
    return [np.ascontiguousarray(g, np.float32) for g in got]


def branches():
    """What the cases cover, for the module-level test: (DFT length, MFCC?, kernel with options?, window) of every case, the
    flag sets, the frame options that leave their defaults, the floors."""
    seen = {(fft_size(c["shape"].W), c["shape"].C > 0, c["flags"] != 0, c["shape"].window) for c in CASES.values()}
    opts = {k for c in CASES.values() for k, d in (("preemph", 0.97), ("remove_dc", True), ("use_power", True)) if getattr(c["shape"], k) != d}
    return seen, {c["flags"] for c in CASES.values()}, opts, {c["floor"] for c in CASES.values()}
