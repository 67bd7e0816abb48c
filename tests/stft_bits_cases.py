"""Cases of tests/test_stft_bits_gpu.py, shared with tests/golden/make_stft_bits_parent.py (which recorded the rows of commit
51f5b97, the last one before the STFT log-mel kernels got their one form rule, one argument core and shared block tail): one
case per branch of k_stft_mel, k_stft_fft_mel, k_stft_post and k_sess_stft_mel that this code walks -- the tile, the number of
passes over the taps, padded taps, the post mode, the packing of the session kernel and its plain twin -- each under the
periodic Hann and under the ramp of tests/stft_edge.py, which is asymmetric: a changed tap order shows.

A batch case is one ragged batch; with R the frames per block of the case: no frame (N / 2 samples), the first length with
frames, R - 1, R and R + 1 frames, 2 R + 1 frames and a remainder.  A session case is eight streams through six sessions,
pushes cut by sess_stft_drive.cut_random at a fixed seed, final pushes included.  Every case names its tile (its packing), and
`tile(pkg, case)` asks the library for it on the CPU."""
import hashlib

import numpy as np

import sess_stft_drive as SD
import stft_drive as D
import stft_edge as SE
from conftest import synth_utterance

WHISPER, LOG10, LN = 0, 1, 2
SESS_STFT_PLAIN = 8192          # mfx_config.engine bit (include/mfx.h): the session entries through k_stft_mel itself
SR = 16000.0
SEED = 0x57F7


def _b(N, S, M, R, window, post=WHISPER, why=""):
    return dict(kind="batch", N=N, S=S, M=M, want=R, window=window, post=post, engine=0, why=why)


def _s(N, S, M, G, engine):
    return dict(kind="sessions", N=N, S=S, M=M, want=G, window="ramp", post=LOG10, engine=engine)


POSTS = {WHISPER: "whisper", LOG10: "log10", LN: "ln"}
CASES = {}
# ---- matrix form, batch: (N, S, M) and the tile mfx_create takes
for N, S, M, R, why in ((32, 8, 4, 64, "one bin tile pair, the smallest N"), (400, 160, 80, 64, "one pass of 13 tiles"),
                        (394, 336, 80, 32, "32-frame blocks"), (510, 170, 40, 64, "N % 4 == 2: padded taps, two passes"),
                        (512, 512, 128, 32, "32-frame blocks, two passes")):
    for w in ("hann", "ramp"):
        for post in (WHISPER, LOG10, LN) if N == 400 else (WHISPER,):
            CASES["matrix_%d_%d_%d_%s_%s" % (N, S, M, w, POSTS[post])] = _b(N, S, M, R, w, post, why)
# ---- FFT form, batch
for N, S, M, R in ((1024, 256, 80, 16), (2048, 512, 128, 16), (2048, 2048, 128, 8)):
    for w in ("hann", "ramp"):
        for post in (WHISPER, LN):
            CASES["fft_%d_%d_%d_%s_%s" % (N, S, M, w, POSTS[post])] = _b(N, S, M, R, w, post)
# ---- session entries: the packed kernel and its plain twin.  4 groups per block at the default shape, 2 at the other two.  NO
# accepted shape answers 1: the block of (512, 512, 128), the largest group the method has (15 S + N + 4 staged words, 257
# bins), takes 125 088 bytes at 2 groups; test_no_shape_packs_one_group holds that.
for N, S, M, G in ((400, 160, 80, 4), (512, 512, 128, 2), (480, 292, 20, 2)):
    for engine, tag in ((0, "packed"), (SESS_STFT_PLAIN, "plain")):
        CASES["sess_%d_%d_%d_%s" % (N, S, M, tag)] = _s(N, S, M, G, engine)
SESSION_FRAMES = (15, 16, 17, 37, 33, 5)             # frames of the streams behind the first two (no frame, the first length with frames)


def tile(pkg, c):
    """What the library answers for the case's shape: frames per block (batch), groups per block (sessions)."""
    if c["kind"] == "sessions":
        return pkg.mfcc.host_sess_stft_lds_bytes(c["N"], c["S"], c["M"])[1]
    return D.form_of(c["N"]).block_rows(pkg, c["N"], c["S"], c["M"])


def lengths(c):
    """Samples of the case's utterances: N / 2 (no frame), the first length with frames, then T S + r, r < S, for each T of the
    case (n div S frames beyond N / 2 samples); the longest ends half a hop into its last frame."""
    N, S, R = c["N"], c["S"], c["want"]
    Ts = SESSION_FRAMES if c["kind"] == "sessions" else (R - 1, R, R + 1, 2 * R + 1)
    out = [N // 2, max(N // 2 + 1, S)]
    assert SD.frames(out[0], N, S) == 0 and SD.frames(out[1] - 1, N, S) == 0 and SD.frames(out[1], N, S) > 0
    for i, T in enumerate(Ts):
        n = T * S + (S // 2 if T == max(Ts) else (3 * i + 1) % S)
        assert n > N // 2 and SD.frames(n, N, S) == T, (c, T, n)
        out.append(n)
    return out


def frames(c):
    """Frames of the case's utterances, in order."""
    return tuple(SD.frames(n, c["N"], c["S"]) for n in lengths(c))


def utterances(c):
    return [synth_utterance(n, 300 + 7 * i, sr=SR) for i, n in enumerate(lengths(c))]


def run_case(pkg, name):
    """The case's rows, one float32 array [frames][M] per utterance (stream)."""
    c = CASES[name]
    N, S, M = c["N"], c["S"], c["M"]
    utts = utterances(c)
    m = D.form_of(N).make(pkg, N, S, M, SR, window=SE.windows(N)[c["window"]], post=c["post"], engine=c["engine"])
    try:
        if c["kind"] == "sessions":
            m.sessions_create(6, 8000)
            got = SD.drive(m, utts, 6, SD.cut_random, N, S, seed=SEED)
        else:
            got = D.run_batch(m, utts)
    finally:
        m.close()
    for g, T in zip(got, frames(c)):
        assert g.shape == (T, M), (name, g.shape, T)
        assert np.isfinite(g).all(), "%s: utterance of %d frames has non-finite values" % (name, T)
    return [np.ascontiguousarray(g, np.float32) for g in got]


# ---- what the fixture holds per case ----------------------------------------------------------------------------------

def digests(rows_list):
    """An 8-byte BLAKE2b digest of every row's bytes, utterance after utterance: uint64 [sum of frames]."""
    return np.array([int.from_bytes(hashlib.blake2b(r.tobytes(), digest_size=8).digest(), "little") for g in rows_list for r in g],
                    np.uint64)


def shortest(rows_list):
    """Indices of the three shortest utterances that have rows."""
    return sorted((i for i in range(len(rows_list)) if len(rows_list[i])), key=lambda i: (len(rows_list[i]), i))[:3]


def shortest_bits(rows_list):
    """The int32 bit patterns of the rows of the three shortest non-empty utterances, in full."""
    return np.concatenate([rows_list[i] for i in shortest(rows_list)]).view(np.int32)
