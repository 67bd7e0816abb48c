"""Cases of tests/test_tail_bits_gpu.py, shared with tests/golden/make_tail_bits_parent.py (which recorded the rows of commit
90865a5, the last one before the kernels behind the front ends got their shared tile, slicing and launch code): one case per
instantiation or branch of the delta stage, the normaliser, the cepstra from a stored spectrum, TRAPS, splice + affine, the
streaming interface and the session entries.  A batch case is one ragged batch of utterances of 1, 6, 7, 63, 64, 65, 129 and
257 frames with filler in between: with 64-row tiles a one-row tile, 2 D and 2 D + 1 rows at (3, 3), both sides of one tile,
both sides of k_delta16's two-tile block, and a second block.  Every case names the kernel or branch it is there for, and
`branch(case)` derives the same name from the launchers' conditions restated here (mfx_tail.hip, mfx_api.cpp, mfx_traps.hip,
mfx_xform.hip)."""
import hashlib

import numpy as np

import xform_ref as XR
from conftest import synth_utterance

W, S, SR = 400, 160, 16000.0
FRAMES = (1, 6, 7, 63, 64, 65, 129, 257)
FILLER = 0x5A5A
NORM_NONE, CMN, CVN, MINMAX = 0, 1, 2, 3
MFCC, PLP, TRAPS = 0, 1, 3
STREAM_KERNELS, NORM_TWO_KERNELS, TRAPS_VALU, XFORM_VALU = 8, 16, 512, 1024      # mfx_config.engine bits (include/mfx.h)
ALPHAS3 = (1.0, 0.88, 1.12, 0.88, 1.0, 1.12, 1.12, 0.88)                         # three warp factors, runs of one utterance


def _c(want, nb=26, nc=13, c0=False, dyn=2, l=(3, 3), norm=NORM_NONE, engine=0, method=MFCC, lpc=0, L=0, K=0, frames=FRAMES,
       alphas=None, xform=None, unaligned_out=False, kind="batch"):
    return dict(want=want, nb=nb, nc=nc, c0=c0, dyn=dyn, l=l, norm=norm, engine=engine, method=method, lpc=lpc, L=L, K=K,
                frames=tuple(frames), alphas=alphas, xform=xform, unaligned_out=unaligned_out, kind=kind)


def _x(out_dim, left=1, right=1, n_xf=1):
    return dict(out_dim=out_dim, left=left, right=right, n_xf=n_xf)


C2 = dict(nb=40, nc=13, dyn=2, l=(3, 3))
CASES = {
    # ---- delta stage (statics of 26 filters; log mel rows where the width is a filter count)
    "delta16_33": _c("k_delta16<3,3>"),
    "delta16_25": _c("k_delta16<0,0>", l=(2, 5)),
    "delta_fast16_1010": _c("k_delta<true,64>", l=(10, 10)),
    "delta_fast16_unaligned_out": _c("k_delta<true,64>", unaligned_out=True),
    "delta_generic_17": _c("k_delta<false,32>", nb=17, nc=0),
    "delta4_20": _c("k_delta4<32>", nb=20, nc=0),
    "delta4_128": _c("k_delta4<32>", nb=128, nc=0),
    "delta_only_13": _c("k_delta16<0,0>", dyn=1),
    "delta_only_20": _c("k_delta4<32>", nb=20, nc=0, dyn=1),
    # ---- normaliser on 13 columns (after the deltas: three column groups)
    "norm_cmn": _c("k_norm_seg", norm=CMN),
    "norm_cvn": _c("k_norm_seg", norm=CVN),
    "norm_minmax": _c("k_norm_seg", norm=MINMAX),
    "norm_cmn_two_kernels": _c("k_norm_stats+k_norm_apply", norm=CMN, engine=NORM_TWO_KERNELS),
    "norm_cvn_two_kernels": _c("k_norm_stats+k_norm_apply", norm=CVN, engine=NORM_TWO_KERNELS),
    "norm_minmax_two_kernels": _c("k_norm_stats+k_norm_apply", norm=MINMAX, engine=NORM_TWO_KERNELS),
    "norm_cvn_4200_rows": _c("k_norm_stats+k_norm_finalize+k_norm_apply", norm=CVN, frames=FRAMES + (4200,)),
    "norm_cvn_one_column": _c("k_norm_seg", nc=1, norm=CVN),
    # ---- cepstra from a stored spectrum
    "melcep_c2": _c("k_melcep", engine=STREAM_KERNELS, **C2),
    "melcep_runs_c2": _c("k_melcep_runs", alphas=ALPHAS3, **C2),
    "plp_8": _c("k_plp<8>", method=PLP, lpc=8, **C2),
    "plp_12": _c("k_plp<16>", method=PLP, lpc=12, **C2),
    "plp_20": _c("k_plp<32>", method=PLP, lpc=20, **C2),
    "plp_runs_12": _c("k_plp_runs<16>", method=PLP, lpc=12, alphas=ALPHAS3, **C2),
    # ---- TRAPS, L = 31: K = 4 / 10 / 20 are KP = 4 / 16 / 32 on the vector ALUs.  (12 bands at K = 20: the kernel serves at most
    # 256 columns and 15 x 20 are 300, which mfx_create refuses.)
    "traps_k4": _c("k_traps<false,0> R64", nb=15, nc=0, dyn=0, method=TRAPS, L=31, K=4),
    "traps_k10": _c("k_traps<false,0> R32", nb=15, nc=0, dyn=0, method=TRAPS, L=31, K=10),
    "traps_k20": _c("k_traps<false,0> R32", nb=12, nc=0, dyn=0, method=TRAPS, L=31, K=20),
    "traps_k4_valu": _c("k_traps<true,4> R64", nb=15, nc=0, dyn=0, method=TRAPS, L=31, K=4, engine=TRAPS_VALU),
    "traps_k10_valu": _c("k_traps<true,16> R32", nb=15, nc=0, dyn=0, method=TRAPS, L=31, K=10, engine=TRAPS_VALU),
    "traps_k20_valu": _c("k_traps<true,32> R32", nb=12, nc=0, dyn=0, method=TRAPS, L=31, K=20, engine=TRAPS_VALU),
    "traps_16_row_tile": _c("k_traps<false,0> R16", nb=16, nc=0, dyn=0, method=TRAPS, L=101, K=16),
    # ---- splice + affine on 13 + d + dd (39 columns), splice +-1: in_dim 117.  The tile height follows the 40 KB target, and the
    # accumulator tiles per wave (TM) follow it: 64 rows up to 48 outputs (TM 1, 2, 3), 32 rows at 64 and 128 (TM 2, 4), 16 rows at
    # 256 (TM 4); TM 8 and 16 come with the two cases on wide rows
    "xform_16": _c("k_splice_affine<false,1> R64", xform=_x(16)),
    "xform_32": _c("k_splice_affine<false,2> R64", xform=_x(32)),
    "xform_48": _c("k_splice_affine<false,3> R64", xform=_x(48)),
    "xform_64": _c("k_splice_affine<false,2> R32", xform=_x(64)),
    "xform_128": _c("k_splice_affine<false,4> R32", xform=_x(128)),
    "xform_256": _c("k_splice_affine<false,4> R16", xform=_x(256)),
    # (no tile inside 40 KB on wide rows: 64 rows within 160 KB, a wave carries every accumulator tile)
    "xform_256_on_128_columns": _c("k_splice_affine<false,16> R64", nb=64, nc=0, dyn=1, xform=_x(256)),
    "xform_120_on_256_columns": _c("k_splice_affine<false,8> R64", nb=128, nc=0, dyn=1, xform=_x(120)),
    "xform_39_scalar_stores": _c("k_splice_affine<false,3> R64", xform=_x(39)),
    "xform_40_float4_stores": _c("k_splice_affine<false,3> R64", xform=_x(40)),
    "xform_40_valu": _c("k_splice_affine<true,3> R64", xform=_x(40), engine=XFORM_VALU),
    "xform_40_two_transforms": _c("k_splice_affine<false,3> R64", xform=_x(40, n_xf=2)),
    # ---- streaming interface: C2 with CVN in 37-frame blocks and a flush (k_melcep, the inline-segment forms, k_copy_small, run_norm)
    "stream_c2_cvn": _c("k_melcep+k_delta<true,64>+k_norm_seg", norm=CVN, frames=(45, 65, 129, 257), kind="stream", **C2),
    # ---- session entries: three sessions, four ragged pushes, the last final
    "sessions_c1": _c("k_sess_gather+k_delta16<3,3>", frames=(40, 57, 71), kind="sessions"),
}


# ---- the launchers' conditions, restated ------------------------------------------------------------------------------

def stat_cols(c):
    """Columns of the static part of a row."""
    if c["method"] == TRAPS:
        return c["nb"] * c["K"]
    return c["nc"] + (1 if c["c0"] else 0) if c["nc"] > 0 else c["nb"]


def delta_branch(cols, l1, l2, src_pitch, out_pitch, aligned=True):
    """launch_delta (mfx_tail.hip); l2 = 0 for dyn = DELTA."""
    D, groups = l1 + l2, 3 if l2 > 0 else 2
    whole_rows = out_pitch == cols * groups and aligned
    if cols <= 16 and l1 > 0 and D <= 16 and src_pitch == 16 and whole_rows:
        return "k_delta16<3,3>" if (l1, l2) == (3, 3) else "k_delta16<0,0>"
    if cols > 16 and cols % 4 == 0 and l1 > 0 and src_pitch % 4 == 0 and whole_rows and \
            ((32 + 2 * D) + (32 + 2 * l2) + 32) * cols * 4 <= 64 * 1024:
        return "k_delta4<32>"
    return "k_delta<true,64>" if cols <= 16 else "k_delta<false,32>"


def norm_branch(cols, max_frames, engine):
    """run_norm (mfx_api.cpp) and launch_norm_stats: one block per segment while the rows of the longest segment, rounded up
    to whole 64-row tiles, fit 54 KB of LDS; else statistics + apply, with k_norm_finalize beyond 4096 rows."""
    max_rows = (max_frames + 63) // 64 * 64
    if not (engine & NORM_TWO_KERNELS) and max_rows * cols * 4 <= 54 * 1024:
        return "k_norm_seg"
    return "k_norm_stats+k_norm_finalize+k_norm_apply" if max_rows > 4096 else "k_norm_stats+k_norm_apply"


def traps_lds_bytes(R, M, L, K, valu):
    steps, kp = (L + 3) >> 2, 4 if K <= 4 else 16 if K <= 16 else 32
    ops = L * kp if valu else ((K + 15) >> 4) * steps * 64
    return 4 * (((R * M * K + 3) & ~3) + ops + M * ((R + 4 * steps) | 1))


def tile_rows(lds_of):
    """The largest of 64 / 32 / 16 rows inside the 40 KB target, else inside 160 KB (traps_tile_rows, xform_tile_rows)."""
    for cap in (40 * 1024, 160 * 1024):
        for R in (64, 32, 16):
            if lds_of(R) <= cap:
                return R
    return 0


def branch(c):
    """The kernel or branch the case's run takes, from its configuration alone."""
    cols, (l1, l2) = stat_cols(c), c["l"]
    l2e = l2 if c["dyn"] == 2 else 0
    width = cols * (1 + c["dyn"])
    if c["kind"] == "stream":        # statics at the column pitch, one inline segment per block
        return "k_melcep+%s+%s" % (delta_branch(cols, l1, l2e, cols, width), norm_branch(cols, 37, c["engine"]))
    if c["kind"] == "sessions":      # compact 16-float statics, as the batch entries
        return "k_sess_gather+" + delta_branch(cols, l1, l2e, 16, width)
    if c["xform"]:
        x, valu = c["xform"], bool(c["engine"] & XFORM_VALU)
        R = XR.tile_rows(width, x["left"], x["right"], x["out_dim"])
        t = ((x["out_dim"] + 15) // 16 + 4 // (R >> 4) - 1) // (4 // (R >> 4))
        return "k_splice_affine<%s,%d> R%d" % ("true" if valu else "false", t if t <= 4 else 8 if t <= 8 else 16, R)
    if c["method"] == TRAPS:
        valu = bool(c["engine"] & TRAPS_VALU)
        R = tile_rows(lambda r: traps_lds_bytes(r, c["nb"], c["L"], c["K"], valu))
        kp = 4 if c["K"] <= 4 else 16 if c["K"] <= 16 else 32
        return "k_traps<%s,%d> R%d" % ("true" if valu else "false", kp if valu else 0, R)
    if c["norm"]:
        return norm_branch(cols, max(c["frames"]), c["engine"])
    if c["method"] == PLP or c["alphas"] or c["engine"] & STREAM_KERNELS:
        # (no fused front end: spectrum through HBM, then k_melcep / k_plp, their row-run forms under per-utterance factors)
        runs = "_runs" if c["alphas"] else ""
        if c["method"] == PLP:
            return "k_plp%s<%d>" % (runs, 8 if c["lpc"] <= 8 else 16 if c["lpc"] <= 16 else 32)
        return "k_melcep" + runs
    src_pitch = 16 if cols <= 16 else width     # mfx_batch.cpp: compact statics up to 16 columns, else the rows in place
    return delta_branch(cols, l1, l2e, src_pitch, width, aligned=not c["unaligned_out"])


# ---- running a case ---------------------------------------------------------------------------------------------------

def samples_for(frames):
    return W - S + frames * S + 36


def utterances(c):
    return [synth_utterance(samples_for(f), 900 + i) for i, f in enumerate(c["frames"])]


def place(utts):
    """The utterances at even offsets with 2, 4, 6, ... samples of filler in between: (PCM, offsets, lengths)."""
    offs, pos = [], 0
    for i, u in enumerate(utts):
        offs.append(pos)
        pos += len(u) + (len(u) & 1) + 2 * (1 + i)
    pcm = np.full(pos + 8, np.int16(FILLER), np.int16)
    for o, u in zip(offs, utts):
        pcm[o:o + len(u)] = u
    return pcm, offs, [len(u) for u in utts]


def handle(pkg, c, ibs=200000):
    m = pkg.MfccHip(ibs, W, S, c["nb"], SR, 64.0, SR / 2, c["nc"], c["c0"], 22.0, c["norm"], c["dyn"], c["l"][0], c["l"][1], True,
                    device=0, bug_compat=False, engine=c["engine"], method=c["method"], lpc_order=c["lpc"], traps_len=c["L"],
                    traps_dct_len=c["K"])
    m.set_window(pkg.reference_window(W))
    return m


def matrices(c, width):
    x = c["xform"]
    rng = np.random.default_rng(4100 + x["out_dim"])
    in_dim = (x["left"] + x["right"] + 1) * width
    A = (rng.standard_normal((x["n_xf"], x["out_dim"], in_dim)) / np.sqrt(in_dim)).astype(np.float32)
    return A, rng.standard_normal((x["n_xf"], x["out_dim"])).astype(np.float32)


def _run_batch(pkg, c):
    pcm, offs, lens = place(utterances(c))
    m = handle(pkg, c)
    try:
        rows, total = m.batch_plan(offs, lens)
        assert total == sum(c["frames"])
        if c["alphas"]:
            m.batch_set_alphas(np.asarray(c["alphas"], np.float32))
        if c["xform"]:
            A, b = matrices(c, m.get_output_data_width())
            n = c["xform"]["n_xf"]
            m.batch_set_transform(A, b, left=c["xform"]["left"], right=c["xform"]["right"],
                                  utt_xf=np.arange(len(lens), dtype=np.int32) % n if n > 1 else None)
        if c["unaligned_out"]:       # the device entry with d_out 4 bytes past a 16-byte boundary
            import torch
            m.set_stream(torch.cuda.current_stream().cuda_stream)
            width = m.batch_output_width()
            d_pcm = torch.from_numpy(pcm).to("cuda:0")
            d_buf = torch.full((total * width + 8,), float("nan"), dtype=torch.float32, device="cuda:0")
            assert d_buf.data_ptr() % 16 == 0
            m.batch_run_device(d_pcm.data_ptr(), pcm.size, d_buf.data_ptr() + 4)
            m.synchronize()
            out = d_buf.cpu().numpy()[1:1 + total * width].reshape(total, width)
        else:
            out = m.batch_run_host(pcm)
        return [out[r:r + f] for r, f in zip(rows, c["frames"])]
    finally:
        m.close()


def _run_stream(pkg, c):
    """Every utterance as a stream of its own: a first block of 37 frames, blocks of 37 shifts, a flush."""
    got = []
    for u in utterances(c):
        m = handle(pkg, c, ibs=100 * S + W)
        try:
            rows, pos, first = [], 0, True
            while pos < u.size:
                n_in = (W - S if first else 0) + 37 * S
                n = m.set_input(u[pos:pos + n_in])
                pos, first = pos + n_in, False
                m.apply()
                rows.append(m.get_output_data(n))
            n = m.flush()
            m.apply()
            rows.append(m.get_output_data(n))
            got.append(np.concatenate(rows))
        finally:
            m.close()
    return got


def _run_sessions(pkg, c):
    """Three sessions, four pushes of ragged lengths (the last final), each session's rows in push order."""
    utts = utterances(c)
    m = handle(pkg, c)
    try:
        m.sessions_create(len(utts), 8000)
        fed, got = [0] * len(utts), [[] for _ in utts]
        for k in range(4):
            ids, offs, lens, parts, pos = [], [], [], [], 0
            for s, u in enumerate(utts):
                n = u.size - fed[s] if k == 3 else min(u.size - fed[s], (u.size // 4 + 97 * (s + 1) * (k + 1)) & ~1)
                ids.append(s), offs.append(pos), lens.append(n)
                parts += [u[fed[s]:fed[s] + n], np.full(2 * (1 + s) + (n & 1), np.int16(FILLER), np.int16)]
                pos += parts[-2].size + parts[-1].size
                fed[s] += n
            out_rows, counts, total = m.sessions_plan(ids, offs, lens, [int(k == 3)] * len(utts))
            out = m.sessions_run_host(np.concatenate(parts))
            for s, (r0, cnt) in enumerate(zip(out_rows, counts)):
                got[s].append(out[r0:r0 + cnt].copy())
        return [np.concatenate(g) for g in got]
    finally:
        m.close()


def run_case(pkg, name):
    """The case's rows, one float32 array [frames][width] per utterance (stream, session)."""
    c = CASES[name]
    got = {"batch": _run_batch, "stream": _run_stream, "sessions": _run_sessions}[c["kind"]](pkg, c)
    for g, f in zip(got, c["frames"]):
        assert g.ndim == 2 and g.shape[0] == f, (name, g.shape, f)
    return [np.ascontiguousarray(g, np.float32) for g in got]


def stat_rows(c, t):
    """Rows the normaliser's statistics of an utterance of t frames cover (batch entries, norm after the deltas, statistics
    of the block the reference would deliver: mfcccpu.cpp:377-388): the last D rows are flush rows where there are more."""
    D = 0 if c["dyn"] == 0 else c["l"][0] if c["dyn"] == 1 else sum(c["l"])
    return t - D if t > D else t


def assert_finite(name, got):
    """Every row finite -- but for an utterance whose statistics cover ONE row under CVN or MINMAX (1 and 7 frames at
    D = 6): its variance and its range are 0, the multiplier is 1 / 0 and the rows are 0 x inf, in the reference as here
    (tests/test_tail_gpu.py).  Those rows are held by their bit patterns alone."""
    c = CASES[name]
    for g, t in zip(got, c["frames"]):
        if c["kind"] == "batch" and c["norm"] in (CVN, MINMAX) and stat_rows(c, t) == 1:
            continue
        assert np.isfinite(g).all(), "%s: utterance of %d frames has non-finite values" % (name, t)


# ---- what the fixture holds per case ----------------------------------------------------------------------------------

def digests(rows_list):
    """An 8-byte BLAKE2b digest of every row's bytes, utterance after utterance: uint64 [sum of frames]."""
    return np.array([int.from_bytes(hashlib.blake2b(r.tobytes(), digest_size=8).digest(), "little") for g in rows_list for r in g],
                    np.uint64)


def shortest_bits(rows_list):
    """The int32 bit patterns of the rows of the three shortest utterances, in full."""
    order = sorted(range(len(rows_list)), key=lambda i: (len(rows_list[i]), i))[:3]
    return np.concatenate([rows_list[i] for i in order]).view(np.int32)
