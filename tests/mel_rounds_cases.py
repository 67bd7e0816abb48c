"""Cases of tests/test_mel_rounds_gpu.py, shared with tests/golden/make_mel_rounds_parent.py (which recorded the rows of
commit cb8bf57, k_front512's mel walk in 8-bin trips, before the 16-bin batches).  One batch of three utterances of 5, 18 and 37 frames: 16-frame
chunks of 4-frame iterations with 3, 2 and 3 dead slots in their last iteration and, in the 37-frame utterance, two chunk
boundaries.  No delta stage (5 frames are fewer than the reference accepts with one), so the rows are the front end's own."""
import numpy as np

from conftest import synth_utterance

FRAMES = (5, 18, 37)

# name -> (MfccHip / oracle shape, round lengths of its 16-lane plan, what the plan is here for)
CASES = {
    "c2_40mel_13cep": (dict(W=400, S=160, nb=40, sr=16000.0, nc=13, c0=False), (32, 16, 8),
                       "C2's plan: a 32-bin, a 16-bin and an 8-bin round, DCT on the matrix pipe"),
    "r_15mel_12cep_c0": (dict(W=400, S=160, nb=15, sr=16000.0, nc=12, c0=True), (80,),
                         "the reference defaults: one long round, a whole number of 16-bin batches"),
    "tel_23mel_256pt": (dict(W=200, S=80, nb=23, sr=8000.0, nc=13, c0=False), (24, 8),
                        "8 kHz on the zero-stuffed 256-point form: 16 bins plus the 8-bin remainder"),
    "fbank40": (dict(W=400, S=160, nb=40, sr=16000.0, nc=0, c0=False), (32, 16, 8),
                "40 log mel energies, no DCT: the walk's plain form"),
    "long_24mel_13cep": (dict(W=400, S=160, nb=24, sr=16000.0, nc=13, c0=False), (56, 16),
                         "a 56-bin round: longer than a batch of 16 or 32 and a multiple of neither"),
    "fbank80_5rounds": (dict(W=400, S=160, nb=80, sr=16000.0, nc=0, c0=False), (16, 16, 8, 8, 8),
                        "five rounds in the plain form: more than four, the rounds a walk can hold metadata for up front"),
}


def utterances(sh):
    return [synth_utterance(sh["W"] + (f - 1) * sh["S"], 700 + i, sr=sh["sr"]) for i, f in enumerate(FRAMES)]


def place(utts):
    """The utterances at even offsets with a few filler samples in between: (flat PCM, offsets, lengths)."""
    offs, pos = [], 0
    for i, u in enumerate(utts):
        offs.append(pos)
        pos += len(u) + (len(u) & 1) + 2 * (1 + i)
    pcm = np.full(pos + 8, 0x5A5A, np.int16)
    for o, u in zip(offs, utts):
        pcm[o:o + len(u)] = u
    return pcm, offs, [len(u) for u in utts]


def handle(pkg, sh):
    m = pkg.MfccHip(200 * sh["S"] + sh["W"], sh["W"], sh["S"], sh["nb"], sh["sr"], 64.0, sh["sr"] / 2, sh["nc"], sh["c0"], 22.0,
                    pkg.NORM_NONE, pkg.DYN_NONE, 3, 3, True, device=0)
    m.set_window(pkg.reference_window(sh["W"]))
    return m


def run_batch(pkg, sh):
    """The batch through the batch entry: (rows [sum of FRAMES][cols], first row of each utterance, kernel name)."""
    pcm, offs, lens = place(utterances(sh))
    m = handle(pkg, sh)
    try:
        rows, total = m.batch_plan(offs, lens)
        assert total == sum(FRAMES)
        out = m.batch_run_host(pcm)
        return out, [int(r) for r in rows], m.dominant_kernel_name()
    finally:
        m.close()


def plan_rounds(pkg, sh):
    """Round lengths of the 16-lane plan k_front512 walks for the shape, from host code alone: the kernel and the transform
    size a planning handle names, and the plan builder on the tables of that size."""
    kernel = pkg.plan_kernel(window_size=sh["W"], shift=sh["S"], num_banks=sh["nb"], sample_rate=sh["sr"], ceps_len=sh["nc"],
                             want_c0=sh["c0"])
    W2 = 1 << int(np.ceil(np.log2(sh["W"])))
    wt, beg = pkg.host_mel_table(sh["nb"], W2, sh["sr"], 64.0, sh["sr"] / 2, 1.0)
    pl = pkg.host_mel_lane_plan(16, wt, beg, 479)
    return kernel, tuple(int(v) for v in pl["L"])
