"""Cases of tests/test_front_bits_gpu.py, shared with tests/golden/make_front_bits_parent.py (which recorded the rows of commit
64dcbfe, the last one before the register front ends' shared pieces moved into csrc/mfx_front_dev.h): one case per family of
instantiations of k_front512, k_front1024 and k_front2048 that tests/test_mel_rounds_gpu.py (six aligned mono k_front512
shapes) does not reach.  Every case is one batch of three utterances of 5, 18 and 37 frames with filler in between: dead slots
in the last 4-frame and 2-frame iteration, a whole 16-frame chunk plus a remainder and, in the 37-frame utterance, two chunk
boundaries, so that the chunk rotation and the prefetch across chunks both run.  No delta stage unless the case says so."""
import numpy as np

from conftest import synth_utterance

FRAMES = (5, 18, 37)
FRAMES_DELTA = (18, 37, 70)      # the fused delta wave's case: utterances long enough for the (3, 3) regressions
FILLER = 0x5A5A
ENGINE_FUSE_DELTA, ENGINE_STREAM_KERNELS, ENGINE_FRONT1024_12_WAVES = 2, 8, 256      # mfx_config.engine bits (include/mfx.h)
DYN_NONE, DYN_ACC = 0, 2


def _sh(W, S, nb, sr, nc, fft=0, ch=1, odd=False, engine=0, dyn=DYN_NONE, frames=FRAMES):
    return dict(W=W, S=S, nb=nb, sr=float(sr), nc=nc, c0=False, fft=fft, ch=ch, odd=odd, engine=engine, dyn=dyn, frames=frames)


# name -> (shape, kernel the run reports, the family of instantiations the case is here for)
CASES = {
    # k_front512
    "f512_c2_odd161": (_sh(400, 161, 40, 16000, 13, odd=True), "k_front512", "C2 at odd shift 161, utterances on odd offsets: the unaligned build"),
    "f512_win512": (_sh(512, 160, 40, 16000, 13), "k_front512", "a 512-tap window: NM = 16"),
    "f512_stereo16k": (_sh(400, 160, 40, 16000, 13, ch=2), "k_front512", "16 kHz stereo"),
    "f512_stereo8k": (_sh(200, 80, 23, 8000, 13, ch=2), "k_front512", "8 kHz stereo: stuffed + stereo"),
    "f512_128pt": (_sh(128, 64, 20, 8000, 12), "k_front512", "128 points: zero-stuffed twice over"),
    "f512_64pt": (_sh(64, 32, 12, 8000, 8), "k_front512", "64 points: zero-stuffed three times over"),
    "f512_c2_stream_kernels": (_sh(400, 160, 40, 16000, 13, engine=ENGINE_STREAM_KERNELS), "k_front512",
                               "C2 under MFX_ENGINE_STREAM_KERNELS: the TO_SPEC build, then k_melcep"),
    "f512_c2_fuse_delta": (_sh(400, 160, 40, 16000, 13, engine=ENGINE_FUSE_DELTA, dyn=DYN_ACC, frames=FRAMES_DELTA), "k_front512",
                           "C2 with the deltas (3, 3) under MFX_ENGINE_FUSE_DELTA: the FUSE build and its delta wave"),
    # k_front1024
    "f1024_c3": (_sh(400, 160, 80, 16000, 13, fft=1024), "k_front1024", "C3: 16 waves"),
    "f1024_c3_12waves": (_sh(400, 160, 80, 16000, 13, fft=1024, engine=ENGINE_FRONT1024_12_WAVES), "k_front1024",
                         "C3 under MFX_ENGINE_FRONT1024_12_WAVES"),
    "f1024_c3_odd161": (_sh(400, 161, 80, 16000, 13, fft=1024, odd=True), "k_front1024", "C3 at odd shift 161: unaligned, 12 waves"),
    "f1024_22k_552": (_sh(552, 220, 80, 22050, 13), "k_front1024", "22.05 kHz, 552 taps: NM = 24"),
    "f1024_32k_800": (_sh(800, 320, 80, 32000, 13), "k_front1024", "32 kHz, 800 taps: NM = 32"),
    "f1024_22k_fbank80": (_sh(552, 220, 80, 22050, 0), "k_front1024", "22.05 kHz fbank-80: no DCT"),
    # k_front2048
    "f2048_c5_stereo": (_sh(1102, 441, 128, 44100, 40, ch=2), "k_front2048", "C5 stereo: split DCT"),
    "f2048_mono_aligned": (_sh(1102, 440, 128, 44100, 40), "k_front2048", "44.1 kHz mono on aligned sample pairs"),
    "f2048_mono_odd441": (_sh(1102, 441, 128, 44100, 40, odd=True), "k_front2048", "mono at odd shift 441: the any-alignment build"),
    "f2048_48k_1200": (_sh(1200, 480, 128, 48000, 40), "k_front2048", "48 kHz, 1200 taps: the 20-row build"),
    "f2048_full_window": (_sh(2048, 512, 128, 44100, 40), "k_front2048", "n_fft = win_length = 2048, hop 512: the 32-row build"),
}


def cols(sh):
    return (sh["nc"] if sh["nc"] > 0 else sh["nb"]) * (1 + sh["dyn"])


def utterances(sh):
    """[n][ch] int16 each: BASELINE noise + tone, frames[i] frames exactly."""
    ch = sh["ch"]
    return [synth_utterance((sh["W"] + (f - 1) * sh["S"]) * ch, 800 + i, sr=sh["sr"]).reshape(-1, ch) for i, f in enumerate(sh["frames"])]


def place(utts, ch, odd):
    """The utterances at even offsets (odd: at odd ones) with 2, 4, 6 samples of filler in between: (flat PCM, offsets,
    lengths), offsets and lengths in samples per channel."""
    offs, pos = [], 1 if odd else 0
    for i, u in enumerate(utts):
        offs.append(pos)
        pos += len(u)
        pos += (pos + (1 if odd else 0)) & 1
        pos += 2 * (1 + i)
    pcm = np.full((pos + 8, ch), np.int16(FILLER), np.int16)
    for o, u in zip(offs, utts):
        pcm[o:o + len(u)] = u
    return pcm.reshape(-1), offs, [len(u) for u in utts]


def handle(pkg, sh):
    m = pkg.MfccHip(200 * sh["S"] + sh["W"], sh["W"], sh["S"], sh["nb"], sh["sr"], 64.0, sh["sr"] / 2, sh["nc"], sh["c0"], 22.0,
                    pkg.NORM_NONE, sh["dyn"], 3, 3, True, device=0, fft_size=sh["fft"], channels=sh["ch"], bug_compat=False,
                    engine=sh["engine"])
    m.set_window(pkg.reference_window(sh["W"]))
    return m


def run_batch(pkg, sh):
    """The batch through the batch entry: (rows [sum of frames][cols], first row of each utterance, kernel name)."""
    pcm, offs, lens = place(utterances(sh), sh["ch"], sh["odd"])
    m = handle(pkg, sh)
    try:
        rows, total = m.batch_plan(offs, lens)
        assert total == sum(sh["frames"])
        kernel = m.dominant_kernel_name()
        out = m.batch_run_host(pcm)
        return out, [int(r) for r in rows], kernel
    finally:
        m.close()


def fused_wave_runs(sh):
    """Whether a batch_run_host of the case takes k_front512's fused delta wave -- plan_fused_delta (mfx_batch_plan.cpp) and
    decide_mode (mfx_batch.cpp), restated: the engine bit, a mono 512-point shape that is not zero-stuffed, a delta stage of
    at most 16 rows of context on at most 16 cepstra with the DCT on the matrix pipe (at most 40 bands), no normaliser, a
    whole-batch run into a 16-byte aligned d_out (batch_run_host's own allocation is)."""
    W2 = sh["fft"] or (1 << int(np.ceil(np.log2(sh["W"]))))
    return bool(sh["engine"] & ENGINE_FUSE_DELTA) and W2 == 512 and sh["ch"] == 1 and sh["dyn"] == DYN_ACC and \
        0 < sh["nc"] <= 16 and 3 + 3 <= 16 and sh["nb"] <= 40
