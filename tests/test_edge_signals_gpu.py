"""Every row of mfcc.KERNEL_TABLE on the edge signals of tests/edge_signals.py (MI355X, through the C ABI): one batch of all
signals, 40 frames each, against the float64 reference -- log mel energies of the row's ceps_len = 0 twin at EDGE_TOL_LOGMEL,
the row's own cepstra at TOL_MAX / EDGE_TOL_L2 on the scale of the log mel energies -- and, with no reference at all,
identical frames -> identical bits: within an utterance, between an even (E) and an odd (O) placement of the batch, with the
delta stages on, and with the batch in reverse order.  Four rows also stream burst | zero | lsb1 | min; C2 pushes it
through a session.  tests/test_edge_signals_host.py holds the checker to a quarter of the same bars on the CPU.
Run with -s for the worst err / tol per row."""
import numpy as np
import pytest

import __graft_entry__ as G
import edge_signals as ES
from conftest import TOL_MAX

pytestmark = pytest.mark.gpu

KERNEL_TABLE = G.load_package().mfcc.KERNEL_TABLE
IDS = [ES.row_id(what) for what, _, _ in KERNEL_TABLE]
FILL16 = np.int16(ES.FILLER)


def handle(pkg, kw, ceps=None, c0=None, dyn=0):
    sr = kw["sample_rate"]
    W, S = kw["window_size"], kw["shift"]
    m = pkg.MfccHip(200 * S + W, W, S, kw["num_banks"], sr, 64.0, sr / 2, kw["ceps_len"] if ceps is None else ceps,
                    kw.get("want_c0", False) if c0 is None else c0, 22.0, 0, dyn, 3, 3, True, device=0,
                    fft_size=kw.get("fft_size", 0), channels=kw.get("channels", 1), bug_compat=False, engine=kw.get("engine", 0))
    m.set_window(pkg.reference_window(W))
    return m


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.int32)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def place(utts, ch, odd=False):
    """Utterances ([n][ch] each) at even offsets (odd: all moved by one sample) with 2, 4 or 6 samples of 0x5A5A in between:
    (flat PCM, offsets, lengths) in samples per channel."""
    offs, pos = [], 1 if odd else 0
    for i, u in enumerate(utts):
        offs.append(pos)
        pos += len(u)
        pos += (pos + (1 if odd else 0)) & 1
        pos += 2 * (1 + i % 3)
    pcm = np.full((pos + 8, ch), FILL16, np.int16)
    for o, u in zip(offs, utts):
        pcm[o:o + len(u)] = u
    return pcm.reshape(-1), offs, [len(u) for u in utts]


def run(m, utts, ch, odd=False, order=None):
    """The batch in the given order of utterances; returns each utterance's rows in the ORIGINAL order, and the kernel."""
    order = list(range(len(utts))) if order is None else list(order)
    pcm, offs, lens = place([utts[i] for i in order], ch, odd)
    rows, total = m.batch_plan(offs, lens)
    kernel = m.dominant_kernel_name()
    out = m.batch_run_host(pcm)
    assert total == ES.FRAMES * len(utts) and out.shape[0] == total
    got = [None] * len(utts)
    for j, i in enumerate(order):
        got[i] = out[rows[j]:rows[j] + ES.FRAMES]
    return got, kernel


def check_identical_rows(x, name, S, what):
    step = ES.identical_stride(name, S)
    for k in range(step):
        part = bits(x[k::step])
        diff = part != part[:1]
        assert not diff.any(), "%s: %d elements of the rows differ from row %d of identical frames (first: row %d, column %d)" % (
            what, int(diff.sum()), k, *[int(v[0]) for v in np.nonzero(diff)])


def same_arithmetic_under_o(kernel_e, kernel_o, shape):
    """Whether the aligned and the unaligned placement run the same sequence of float operations, so that their rows can be
    compared bit for bit.  Not where O runs another kernel (a window above 512 samples at 1024 points leaves k_front1024 for
    k_front_reg on unaligned frames: another factorisation).  Not on k_front_reg at 1024 points with a window of at most half
    the transform either (mfx_front_generic.hip, TWREG = LOG2M == 9 && PAIR && FUSED && HALF, restated here): its aligned
    build holds the twiddles of passes 1 and 2 in registers, its unaligned build reads them from LDS, and the compiler
    contracts the complex product of the two forms differently -- found by this test on `min`; both placements pass the
    float64 bars, and each is bit-stable in itself."""
    if kernel_e != kernel_o:
        return False
    W2 = shape["fft_size"] or (1 << int(np.ceil(np.log2(shape["W"]))))
    return not (kernel_e == "k_front_reg" and W2 == 1024 and shape["W"] <= 512)


def test_the_rows_that_compare_placements_bit_for_bit():
    """22 mono rows with aligned frames run placement O; three k_front_reg rows take the register-twiddle build under E, and
    of the other 19 those compare O with E bit for bit whose kernel O keeps (on the MI355X all but the three long-window
    k_front1024 rows, which k_front_reg serves on unaligned frames)."""
    with_o = [(ES.row_shape(kw), k) for _, kw, k in KERNEL_TABLE if kw.get("channels", 1) == 1 and kw.get("aligned", True)]
    assert len(with_o) == 22 and sum(same_arithmetic_under_o(k, k, sh) for sh, k in with_o) == 19


@pytest.mark.parametrize("row", range(len(KERNEL_TABLE)), ids=IDS)
def test_edge_signals(pkg, row):
    what, kw, kernel = KERNEL_TABLE[row]
    shape = ES.row_shape(kw)
    S, ch, nb, sr = shape["S"], shape["channels"], shape["nb"], shape["sr"]
    cols = (shape["nc"] + (1 if shape["c0"] else 0)) if shape["nc"] > 0 else nb
    ref = ES.row_reference(kw, pkg.reference_window(shape["W"]))
    names = list(ref)
    utts = [ref[n]["pcm"].reshape(-1, ch) for n in names]
    alike = ES.identical_frame_signals(S, sr, ch)
    with_o = ch == 1 and kw.get("aligned", True)
    M = ES.npr.dct_matrix(nb, shape["nc"], shape["c0"], shape["lift"]) if shape["nc"] > 0 else None
    worst = dict(logmel=0.0, emax=0.0, el2=0.0, dct_max=0.0, dct_l2=0.0)

    # 1. log mel energies of the ceps_len = 0 twin
    twin = handle(pkg, kw, ceps=0, c0=False)
    mel_e, twin_kernel = run(twin, utts, ch)
    twin.close()
    for n, g in zip(names, mel_e):
        r = ref[n]
        e = ES.logmel_errors(g, r["mel"], r["ok"])[0]
        worst["logmel"] = max(worst["logmel"], e / ES.EDGE_TOL_LOGMEL)
    print("\n%s\n  kernel %s (ceps_len = 0 twin: %s); worst |d log E| / EDGE_TOL_LOGMEL = %.3f" % (
        what, kernel, twin_kernel, worst["logmel"]))
    for n, g in zip(names, mel_e):
        ES.assert_logmel_close(g, ref[n]["mel"], "%s, %s (log mel energies)" % (what, n), ok=ref[n]["ok"])
    own_mel = M is not None and twin_kernel == kernel     # (another kernel's rounding noise is other noise)

    # 2. the row itself, under both placements
    m = handle(pkg, kw)
    runs = {"E": run(m, utts, ch)}
    assert runs["E"][1] == kernel, "%s: placement E runs %s" % (what, runs["E"][1])
    if with_o:
        runs["O"] = run(m, utts, ch, odd=True)
    reversed_rows, _ = run(m, utts, ch, order=range(len(utts) - 1, -1, -1))
    m.close()
    figures = []
    for p, (got, _) in runs.items():
        for n, g, gm in zip(names, got, mel_e):
            r = ref[n]
            assert g.shape == (ES.FRAMES, cols) and np.isfinite(g).all(), "%s, %s, placement %s" % (what, n, p)
            good = r["ok"].all(axis=1)
            emax, el2 = ES.rows_errors(g[good], r["c"][good], r["mel"])
            # rows with an ill-conditioned log mel energy: the DCT of the kernel's OWN log mel energies (the twin's), in float64
            dmax, dl2 = ES.rows_errors(g[~good], (gm.astype(np.float64) @ M)[~good], r["mel"]) if own_mel else (0.0, 0.0)
            figures.append((p, n, good, emax, el2, dmax, dl2))
            worst.update(emax=max(worst["emax"], emax / TOL_MAX), el2=max(worst["el2"], el2 / ES.EDGE_TOL_L2),
                         dct_max=max(worst["dct_max"], dmax / TOL_MAX), dct_l2=max(worst["dct_l2"], dl2 / ES.EDGE_TOL_L2))
    print("  worst err / tol over %d utterances x %s: max %.3f, L2 %.3f; rows checked through their own log mel energies: max %.3f, L2 %.3f%s" % (
        len(names), " + ".join(runs), worst["emax"], worst["el2"], worst["dct_max"], worst["dct_l2"],
        "" if with_o else "  (no placement O: %s)" % ("stereo" if ch == 2 else "odd shift")))
    if with_o:
        print("  placement O runs %s" % runs["O"][1])
    for p, (got, _) in runs.items():
        for n, g, gm in zip(names, got, mel_e):
            r = ref[n]
            good = r["ok"].all(axis=1)
            tag = "%s, %s, placement %s" % (what, n, p)
            ES.assert_rows_close(g[good], r["c"][good], r["mel"], tag)
            if own_mel and (~good).any():
                ES.assert_rows_close(g[~good], (gm.astype(np.float64) @ M)[~good], r["mel"], tag + " (DCT of its own log mel energies)")

    # 3. identical frames give identical bits: within the utterance, and between the placements
    for p, (got, _) in runs.items():
        for n in alike:
            check_identical_rows(got[names.index(n)], n, S, "%s, %s, placement %s" % (what, n, p))
    for n in alike:
        check_identical_rows(mel_e[names.index(n)], n, S, "%s, %s, log mel energies" % (what, n))
    if with_o and same_arithmetic_under_o(runs["E"][1], runs["O"][1], shape):
        for n in alike:
            i = names.index(n)
            assert same_bits(runs["E"][0][i], runs["O"][0][i]), "%s, %s: rows differ between placements E and O" % (what, n)

    # 5. the batch in reverse order
    for n, a, b in zip(names, runs["E"][0], reversed_rows):
        assert same_bits(a, b), "%s, %s: rows depend on the utterance's place in the batch" % (what, n)

    # 4. with the row's delta stages
    if kw.get("dyn", 0):
        md = handle(pkg, kw, dyn=kw["dyn"])
        got_d, _ = run(md, utts, ch)
        md.close()
        groups = 1 + kw["dyn"]
        for n, g, s in zip(names, got_d, runs["E"][0]):
            assert g.shape == (ES.FRAMES, groups * cols) and np.isfinite(g).all(), "%s, %s with deltas" % (what, n)
            assert same_bits(g[:, :cols], s), "%s, %s: statics with dyn = %d differ from the dyn = 0 run" % (what, n, kw["dyn"])
            if n in alike and ES.identical_stride(n, S) == 1:
                assert not g[:, cols:].any(), "%s, %s: deltas of identical frames are not exactly 0" % (what, n)


# ---- streaming and sessions ----------------------------------------------------------------------------------------------------

STREAM_ROWS = {"C2": "C2 / C4", "8 kHz telephony, zero-stuffed": "8 kHz telephony", "C3": "C3  16 kHz", "C5 mono": "44.1 kHz mono"}


@pytest.mark.parametrize("name", list(STREAM_ROWS))
def test_edge_stream(pkg, name):
    """burst | zero | lsb1 | min as ONE stream through process_stream in blocks of 37 frames' worth, against the float64
    whole-stream formulas (dyn = 0); C2: the same stream through one session in 100 ms pushes, bit-identical to the batch rows."""
    (what, kw, kernel), = [r for r in KERNEL_TABLE if r[0].startswith(STREAM_ROWS[name])]
    shape = ES.row_shape(kw)
    W, S = shape["W"], shape["S"]
    assert shape["channels"] == 1
    window = pkg.reference_window(W)
    ref = ES.row_reference(kw, window)
    pcm = np.concatenate([ref[n]["pcm"] for n in ("burst", "zero", "lsb1", "min")])
    args = {k: v for k, v in shape.items() if k != "channels"}
    c, mel = ES.reference(pcm, window, **args)
    ok = ES.sensitivity(pcm, window, **args) <= ES.COND_TOL
    good = ok.all(axis=1)
    block = 37 * S + W - S

    twin = handle(pkg, kw, ceps=0, c0=False)
    got_mel = twin.process_stream(pcm, block_samples=block)
    twin.close()
    e = ES.logmel_errors(got_mel, mel, ok)[0]
    m = handle(pkg, kw)
    got = m.process_stream(pcm, block_samples=block)
    emax, el2 = ES.rows_errors(got[good], c[good], mel)
    print("\n%s, streamed: %d frames, worst err / tol: log mel %.3f, max %.3f, L2 %.3f" % (
        what, c.shape[0], e / ES.EDGE_TOL_LOGMEL, emax / TOL_MAX, el2 / ES.EDGE_TOL_L2))
    ES.assert_logmel_close(got_mel, mel, "%s, streamed (log mel energies)" % what, ok=ok)
    assert got.shape == c.shape and np.isfinite(got).all()
    ES.assert_rows_close(got[good], c[good], mel, "%s, streamed" % what)
    if (~good).any():
        M = ES.npr.dct_matrix(shape["nb"], shape["nc"], shape["c0"], shape["lift"])
        ES.assert_rows_close(got[~good], (got_mel.astype(np.float64) @ M)[~good], mel, "%s, streamed (DCT of its own log mel energies)" % what)

    m.close()

    if name == "C2":
        padded = np.concatenate([pcm, np.zeros(2, np.int16)])
        mb = handle(pkg, kw)
        mb.batch_plan([0], [pcm.size])
        want = mb.batch_run_host(padded)
        mb.close()
        push = int(0.1 * shape["sr"])
        ms = handle(pkg, kw)
        ms.sessions_create(1, push)
        parts = []
        for pos in range(0, pcm.size, push):
            piece = pcm[pos:pos + push]
            _, counts, tot = ms.sessions_plan([0], [0], [piece.size], [pos + push >= pcm.size])
            parts.append(ms.sessions_run_host(np.concatenate([piece, np.zeros(2, np.int16)]))[:tot])
        ms.close()
        assert want.shape == c.shape
        assert same_bits(np.concatenate(parts), want), "C2: the session's rows differ from the batch entry's"
