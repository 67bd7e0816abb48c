"""The tail stages on the MI355X against tests/tail_ref.py: every delta / delta-delta value against a float64 restatement
of the rows' OWN statics within float32 rounding bounds, the normaliser's statistics against the norm = NONE twin's rows
within theirs, the normalised rows bit for bit.  No oracle and no front-end noise enters a bound.

Each case names the kernel branch it means and asserts, from launch_delta's / run_norm's own conditions restated below
(mfx_tail.hip, mfx_api.cpp), that its shape takes it.  Statics come from real handles through the C ABI: MFCC / PLP for up
to 16 columns, MFCC with ceps_len = 0 for a width that is a filter count, TRAPS for M x K up to 256.
"""
import numpy as np
import pytest

import tail_ref
from conftest import synth_utterance
from tail_ref import assert_norm_consistent, assert_tail_consistent

pytestmark = pytest.mark.gpu

W, S = 400, 160
TRAPS_MK = {129: (43, 3), 150: (15, 10), 230: (23, 10), 255: (15, 17), 256: (16, 16)}   # 255: K = 17, k_traps' scalar store


def make(pkg, cols, dyn=2, l1=3, l2=3, norm=0, nad=True, bns=0, engine=0, plp=False, ibs=200000):
    if cols in TRAPS_MK:
        M, K = TRAPS_MK[cols]
        m = pkg.MfccHip(ibs, W, S, M, 16000.0, 64.0, 8000.0, 0, False, 22.0, norm, dyn, l1, l2, nad, device=0, bug_compat=False,
                        batch_norm_stats=bns, method=pkg.METHOD_TRAPS, traps_len=31, traps_dct_len=K, engine=engine)
    elif cols <= 16:
        m = pkg.MfccHip(ibs, W, S, 26, 16000.0, 64.0, 8000.0, min(cols, 15), cols == 16, 22.0, norm, dyn, l1, l2, nad, device=0,
                        bug_compat=False, batch_norm_stats=bns, engine=engine,
                        method=pkg.METHOD_PLP if plp else pkg.METHOD_MFCC, lpc_order=12 if plp else 0)
    else:                                                   # log mel energies: the width is the filter count
        m = pkg.MfccHip(ibs, W, S, cols, 16000.0, 64.0, 8000.0, 0, False, 22.0, norm, dyn, l1, l2, nad, device=0,
                        bug_compat=False, batch_norm_stats=bns, engine=engine)
    assert m.get_output_data_width() == cols * (1 + dyn)
    m.set_window(pkg.reference_window(W))
    return m


def samples_for(frames):
    return W - S + frames * S + 36


def run_batch(m, utts):
    lens = [u.size for u in utts]
    offs = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
    rows, total = m.batch_plan(offs, lens)
    out = m.batch_run_host(np.concatenate(utts))
    return [out[rows[i]:rows[i] + m.batch_frames(lens[i])] for i in range(len(utts))]


def ragged(D):
    """Frame counts around the delta context and the tile edges of 16 / 32 / 64 rows (k_delta16: two 64-row tiles per
    block), then a silent utterance and a tone of 10 whole periods per shift: identical frames."""
    frames = sorted({1, 2, D, D + 1, 2 * D, 2 * D + 1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 200})
    utts = [synth_utterance(samples_for(t), 300 + t) for t in frames]
    n = samples_for(40)
    utts.append(np.zeros(n, np.int16))
    utts.append(np.round(32767 * np.sin(2 * np.pi * 1000.0 * np.arange(n) / 16000.0)).astype(np.int16))
    return frames + [40, 40], utts


def check_ragged(got, frames, cols, dyn, l1, l2, what):
    worst = {}
    for i, (g, t) in enumerate(zip(got, frames)):
        assert g.shape == (t, cols * (1 + dyn)), (what, i, g.shape)
        w = assert_tail_consistent(g, cols, dyn, l1, l2, "%s, utt %d (%d frames)" % (what, i, t))
        for k, v in w.items():
            worst[k] = max(worst.get(k, 0.0), v)
    for name, g in (("silence", got[-2]), ("tone", got[-1])):
        assert (g[:, :cols] == g[0, :cols]).all(), "%s, %s: identical frames gave different statics" % (what, name)
        assert (g[:, cols:] == 0).all(), "%s, %s: deltas of identical frames must be exactly 0 (max %g)" % (
            what, name, np.abs(g[:, cols:]).max())
    print("%s: worst err / bound %s" % (what, {k: round(v, 3) for k, v in worst.items()}))
    return worst


# ---- launch_delta's branch conditions, restated (mfx_tail.hip) -------------------------------------------------------

def delta_branch(cols, l1, l2, src_pitch, out_pitch):
    """l2 = 0 for dyn = DELTA.  Buffers are allocations of their own: the 16-byte alignment conditions hold."""
    D, groups = l1 + l2, 3 if l2 > 0 else 2
    whole_rows = out_pitch == cols * groups
    if cols <= 16 and l1 > 0 and D <= 16 and src_pitch == 16 and whole_rows:
        return "k_delta16<3,3>" if (l1, l2) == (3, 3) else "k_delta16<0,0>"
    if cols > 16 and cols % 4 == 0 and l1 > 0 and src_pitch % 4 == 0 and whole_rows and \
            ((32 + 2 * D) + (32 + 2 * l2) + 32) * cols * 4 <= 64 * 1024:
        return "k_delta4<32>"
    return "k_delta<true,64>" if cols <= 16 else "k_delta<false,32>"


def batch_src_pitch(cols, dyn, traps):
    """mfx_batch.cpp: up to 16 columns the fused front ends write compact 16-float statics to a scratch buffer for the delta
    stage; wider rows and TRAPS rows are read in place from the output rows."""
    return 16 if cols <= 16 and not traps else cols * (1 + dyn)


DELTA_CASES = [
    # (branch, cols, dyn, l1, l2)
    ("k_delta16<3,3>", 13, 2, 3, 3),
    ("k_delta16<3,3>", 16, 2, 3, 3),
    ("k_delta16<0,0>", 13, 2, 1, 1),
    ("k_delta16<0,0>", 13, 2, 1, 2),
    ("k_delta16<0,0>", 13, 2, 4, 1),
    ("k_delta16<0,0>", 13, 2, 8, 8),
    ("k_delta16<0,0>", 13, 1, 3, 3),
    ("k_delta16<0,0>", 16, 1, 2, 2),
    ("k_delta16<0,0>", 1, 2, 2, 3),
    ("k_delta<true,64>", 13, 2, 10, 10),    # D = 20 > 16
    ("k_delta<true,64>", 16, 2, 9, 8),      # D = 17
    ("k_delta<true,64>", 13, 1, 17, 1),
    ("k_delta4<32>", 20, 2, 3, 3),
    ("k_delta4<32>", 40, 2, 3, 3),
    ("k_delta4<32>", 40, 1, 2, 2),
    ("k_delta4<32>", 80, 2, 3, 3),
    ("k_delta4<32>", 128, 2, 3, 3),
    ("k_delta4<32>", 128, 2, 5, 5),         # 64 512 bytes: the largest k_delta4 tile at 128 columns; (6, 6) is the first beyond 64 KB
    ("k_delta<false,32>", 128, 2, 6, 6),    # the 64 KB fallback: 67 584 bytes as k_delta4
    ("k_delta<false,32>", 17, 2, 3, 3),
    ("k_delta<false,32>", 23, 2, 3, 3),
    ("k_delta<false,32>", 26, 1, 3, 3),
    ("k_delta<false,32>", 150, 2, 1, 2),
    ("k_delta<false,32>", 150, 2, 4, 1),
    ("k_delta<false,32>", 150, 1, 3, 3),
    ("k_delta<false,32>", 230, 2, 3, 3),
    ("k_delta<false,32>", 255, 2, 3, 3),
    ("k_delta<false,32>", 256, 2, 3, 3),    # a multiple of 4, but 116 736 bytes as k_delta4
    ("k_delta<false,32>", 256, 2, 10, 10),  # 159 744 bytes: the largest LDS mfx_create admits
    ("k_delta<false,32>", 129, 2, 2, 5),
]


@pytest.mark.parametrize("branch,cols,dyn,l1,l2", DELTA_CASES, ids=["%s-%dx%d-l%d,%d" % (c[0], c[1], 1 + c[2], c[3], c[4]) for c in DELTA_CASES])
def test_delta_branch(pkg, branch, cols, dyn, l1, l2):
    l2e = l2 if dyn == 2 else 0
    traps = cols in TRAPS_MK
    assert delta_branch(cols, l1, l2e, batch_src_pitch(cols, dyn, traps), cols * (1 + dyn)) == branch
    frames, utts = ragged(l1 + l2e)
    m = make(pkg, cols, dyn, l1, l2)
    got = run_batch(m, utts)
    m.close()
    check_ragged(got, frames, cols, dyn, l1, l2e, "%s, %d columns, dyn %d, l (%d, %d)" % (branch, cols, dyn, l1, l2e))


def test_every_branch_of_launch_delta_is_named():
    assert {c[0] for c in DELTA_CASES} == {"k_delta16<3,3>", "k_delta16<0,0>", "k_delta<true,64>", "k_delta4<32>", "k_delta<false,32>"}


@pytest.mark.parametrize("cols,l1,l2", [(256, 11, 11), (13, 400, 400), (128, 40, 40)])
def test_orders_beyond_the_delta_stage_lds_are_refused_at_create(pkg, cols, l1, l2):
    """(3 R + 2 D + 2 l2) rows of LDS beyond 160 KB: a refusal with a message from mfx_create, not a failed launch.  The
    order below each is admitted (256 columns at (10, 10) runs in test_delta_branch)."""
    with pytest.raises(pkg.MfxError) as e:
        make(pkg, cols, 2, l1, l2)
    assert e.value.status == -5 and "mfx_create" in str(e.value)
    if cols != 256:
        make(pkg, cols, 2, l1 - 10, l2 - 10).close()


# ---- the delta tiles fused into k_front512 ---------------------------------------------------------------------------

@pytest.mark.parametrize("dyn,l1,l2", [(2, 3, 3), (2, 2, 5), (1, 4, 1), (2, 8, 8)])
def test_fused_delta_tiles(pkg, dyn, l1, l2):
    l2e = l2 if dyn == 2 else 0
    frames, utts = ragged(l1 + l2e)
    outs = []
    for engine in (pkg.mfcc.ENGINE_FUSE_DELTA, 0):
        m = make(pkg, 13, dyn, l1, l2, engine=engine)
        outs.append(run_batch(m, utts))
        m.close()
    check_ragged(outs[0], frames, 13, dyn, l1, l2e, "fused delta tiles of k_front512, dyn %d, l (%d, %d)" % (dyn, l1, l2e))
    for a, b in zip(*outs):
        assert np.array_equal(a, b), "fused and separate delta stage differ"


# ---- the streaming path (inline segment; statics at the column pitch: k_delta<true,64>) ------------------------------

@pytest.mark.parametrize("plp", [False, True], ids=["mfcc", "plp"])
@pytest.mark.parametrize("dyn,l1,l2", [(2, 3, 3), (2, 1, 2), (1, 4, 1), (2, 8, 8)])
def test_streaming_blocks(pkg, plp, dyn, l1, l2):
    l2e = l2 if dyn == 2 else 0
    D = l1 + l2e
    assert delta_branch(13, l1, l2e, 13, 13 * (1 + dyn)) == "k_delta<true,64>"
    # a first block of 2 D + 3 frames, then blocks of whole shifts: each delivers as many rows as it brings shifts
    blocks = [samples_for(2 * D + 3)] + [k * S for k in (1, D, 65, 1, 7, D, 65, 2)]
    pcm = synth_utterance(sum(blocks), 17)
    m = make(pkg, 13, dyn, l1, l2, plp=plp, ibs=100 * S + W)
    rows, counts, pos = [], [], 0
    for b in blocks:
        n = m.set_input(pcm[pos:pos + b])
        pos += b
        m.apply()
        rows.append(m.get_output_data(n))
        counts.append(n)
    n = m.flush()
    m.apply()
    rows.append(m.get_output_data(n))
    counts.append(n)
    m.close()
    print("rows per block:", counts)
    assert {1, D, 65} <= set(counts[1:-1]) and counts[-1] == D
    got = np.concatenate(rows)
    assert got.shape[0] == (pcm.size - W) // S + 1
    w = assert_tail_consistent(got, 13, dyn, l1, l2e, "streamed %s" % ("PLP" if plp else "MFCC"))
    print("streaming %s dyn %d l (%d, %d): worst err / bound %s" % ("PLP" if plp else "MFCC", dyn, l1, l2e, w))


# ---- the normaliser --------------------------------------------------------------------------------------------------

NORM_L = (2, 3)                  # D = 5
LDS_SEG = 54 * 1024              # kNormSegLdsBytes
CHUNK = 4096                     # kNormChunkRows


def norm_branch(cols, max_frames, engine):
    """run_norm (mfx_api.cpp) and launch_norm_stats: one block per segment while the rows of the longest segment, rounded
    up to whole 64-row tiles, fit 54 KB of LDS; else statistics + apply, with k_norm_finalize beyond 4096 rows."""
    max_rows = (max_frames + 63) // 64 * 64
    if not (engine & 16) and max_rows * cols * 4 <= LDS_SEG:
        return "k_norm_seg"
    return "k_norm_stats+k_norm_finalize+k_norm_apply" if max_rows > CHUNK else "k_norm_stats+k_norm_apply"


_twins = {}


def twin_rows(pkg, cols, frames_key, utts):
    key = (cols, frames_key)
    if key not in _twins:
        m = make(pkg, cols, 2, *NORM_L, norm=0)
        _twins[key] = run_batch(m, utts)
        m.close()
    return _twins[key]


def check_norm(pkg, cols, engine, frames, seed, expect):
    l1, l2 = NORM_L
    D = l1 + l2
    utts = [synth_utterance(samples_for(t), seed + i) for i, t in enumerate(frames)]
    assert norm_branch(cols, max(frames), engine) == expect
    worst = [0.0, 0.0, 0.0]
    for nad in (True, False):
        xs = twin_rows(pkg, cols, (tuple(frames), seed), utts)
        for kind in (1, 2, 3):
            for bns in (0, 1):
                m = make(pkg, cols, 2, l1, l2, norm=kind, nad=nad, bns=bns, engine=engine)
                ys = run_batch(m, utts)
                G = 3 if nad else 1
                st = m.debug_read(6).reshape(G, len(utts), 2, cols)
                m.close()
                for u, (y, x, t) in enumerate(zip(ys, xs, frames)):
                    what = "%d columns, %s, norm %d nad %d bns %d, utt %d (%d frames)" % (cols, expect, kind, nad, bns, u, t)
                    stat_rows = t - D if (nad and bns == 0 and t > D) else t
                    wm, wk, keep = assert_norm_consistent(y, x, st[:, u], kind, nad, cols, stat_rows, what)
                    worst[0], worst[1] = max(worst[0], wm), max(worst[1], wk)
                    if kind == 2 and t == 1:   # one row: 0 / 0, or 0 over the rounding error of one float32 square
                        assert (~np.isfinite(st[:, u, 1]) | (st[:, u, 1] == 0)).all(), what
                    if not nad:   # the delta groups are those of the NORMALISED statics (columns of degenerate statistics left out)
                        k = keep[0]
                        sub = np.concatenate([y[:, g * cols:(g + 1) * cols][:, k] for g in range(3)], 1)
                        if k.any():
                            w = assert_tail_consistent(sub, int(k.sum()), 2, l1, l2, what + " (finite columns)")
                            worst[2] = max([worst[2]] + list(w.values()))
    print("%d columns, %s: worst err / bound mean %.3g, multiplier %.3g, deltas of normalised statics %.3g" % (
        cols, expect, worst[0], worst[1], worst[2]))


NORM_COLS = [1, 13, 16, 17, 128, 129, 150, 255, 256]
SHORT = [1, 2, 5, 6, 33, 64]     # T <= D: statistics over all T rows; 1 row: degenerate under CVN


@pytest.mark.parametrize("cols", NORM_COLS)
@pytest.mark.parametrize("engine", [0, 16], ids=["default", "two_kernels"])
def test_norm_columns(pkg, cols, engine):
    """k_norm_seg where 64 rows of the width fit its LDS (up to 216 columns), else -- and with engine bit 16 -- the
    two-kernel form; at 129 .. 256 columns k_norm_stats runs one row per pass and its reduction loop not at all."""
    expect = "k_norm_seg" if engine == 0 and cols <= 216 else "k_norm_stats+k_norm_apply"
    check_norm(pkg, cols, engine, SHORT, 500, expect)


def test_norm_segment_longer_than_the_lds(pkg):
    check_norm(pkg, 13, 0, [1100, 64, 3], 520, "k_norm_stats+k_norm_apply")
    check_norm(pkg, 150, 0, [129, 7], 530, "k_norm_stats+k_norm_apply")


def test_norm_utterance_of_more_than_4096_frames(pkg):
    check_norm(pkg, 13, 0, [4200, 70], 540, "k_norm_stats+k_norm_finalize+k_norm_apply")
