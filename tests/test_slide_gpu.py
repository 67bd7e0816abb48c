"""The sliding-window CMN / CVN of the batch entries (mfx_batch_set_sliding_norm) on the MI355X against tests/slide_ref.py.

Every row must be the restatement's bits, computed from the rows the SAME handle delivers without the attachment: the
definition is double additions, subtractions, divisions, one square root and float32 conversions, each a single correctly
rounded operation on both sides.  Independently of the prefix form, |y - y64| <= B against a direct np.longdouble sum of every
window (slide_ref.bound: derived from the number formats, not measured) wherever every window holds >= 32 rows.

    Figures of an MI355X run (worst err / B over the cases of test_rows_against_float64_sums_of_every_window): CMN 0.429,
    CVN 0.687 -- the restatement's own, the rows being its bits."""
import ctypes as C
import os
import subprocess
import wave

import numpy as np
import pytest

import slide_ref as R
import tensor_ref as TR
import vad_ref as VR
import xform_ref as XR
from conftest import synth_utterance
from placement import OutPlacement

pytestmark = pytest.mark.gpu

W, S, SR = 400, 160, 16000.0
FRAMES = (0, 1, 2, 31, 32, 33, 63, 64, 65, 149, 150, 151, 299, 300, 301, 333, 700)
FULL = np.array([32767, -32767, 32767, -32767], np.int16)   # between the utterances, part of none
CASES = ((300, 1, 0), (301, 1, 0), (32, 1, 0), (2, 1, 0), (1, 1, 0), (4096, 1, 0), (600, 0, 100), (64, 0, 64), (64, 0, 1), (100, 0, 0))
ARG, STATE, CONFIG = -7, -8, -5


def case_id(c):
    return "N%d_%s_min%d" % (c[0], "centre" if c[1] else "trail", c[2])


def base(pkg, **over):
    """16 kHz, 400 / 160 / 512, 13 MFCC + c0 + d + dd, norm = NONE."""
    kw = dict(num_banks=40, ceps_len=13, want_c0=True, norm=pkg.NORM_NONE, dyn=pkg.DYN_ACC, engine=0)
    kw.update(over)
    m = pkg.MfccHip(200000, W, S, kw["num_banks"], SR, 64.0, SR / 2, kw["ceps_len"], kw["want_c0"], 22.0, kw["norm"], kw["dyn"], 3, 3, True,
                    device=0, bug_compat=False, engine=kw["engine"])
    m.set_window(pkg.reference_window(W))
    return m


def utterance(T, seed):
    """T frames at 400 / 160 with a gain envelope (half of every second is quiet: an energy VAD has something to decide)."""
    n = 300 if T == 0 else (T - 1) * S + W + (7 * seed) % S
    x = synth_utterance(n, 900 + seed).astype(np.float64)
    x[(np.arange(n) // (S * 20)) % 2 == 1] /= 64.0
    return np.round(x).astype(np.int16)


def packed(utts):
    """offsets, lengths, pcm: the utterances at even offsets with full-scale fillers in front of, between and behind them."""
    parts, offs, at = [FULL], [], FULL.size
    for u in utts:
        offs.append(at)
        pad = FULL if u.size % 2 == 0 else np.concatenate([FULL, FULL[:1]])
        parts += [u, pad]
        at += u.size + pad.size
    return np.array(offs, np.int64), np.array([u.size for u in utts], np.int64), np.concatenate(parts + [np.zeros(2, np.int16)])


_UTTS = []


def utts():
    if not _UTTS:
        _UTTS.extend(utterance(T, k) for k, T in enumerate(FRAMES))
    return _UTTS


def split(out, rows, frames):
    return [out[int(r):int(r) + int(T)] for r, T in zip(rows, frames)]


def plan(m, us):
    offs, lens, pcm = packed(us)
    rows, total = m.batch_plan(offs, lens)
    frames = [m.batch_frames(int(n)) for n in lens]
    return pcm, rows, total, frames


_RAW = {}


def raw_rows(pkg):
    """The base handle's rows of the utterances WITHOUT the attachment: computed once, shared, never changed."""
    if "base" not in _RAW:
        m = base(pkg)
        pcm, rows, total, frames = plan(m, utts())
        assert frames == list(FRAMES)
        out = m.batch_run_host(pcm)
        m.close()
        out.setflags(write=False)
        _RAW["base"] = (out, rows, total, frames)
    return _RAW["base"]


_WANT = {}


def want_rows(pkg, N, center, mw, nv):
    """The restatement of raw_rows under one setting, whole batch: computed once, shared, never changed."""
    key = (N, center, mw, nv)
    if key not in _WANT:
        out, rows, total, frames = raw_rows(pkg)
        y = np.zeros_like(out)
        for r, T in zip(rows, frames):
            if T:
                y[int(r):int(r) + T] = R.sliding_norm(out[int(r):int(r) + T], N, mw, center, nv, exact=False)[0]
        y.setflags(write=False)
        _WANT[key] = y
    return _WANT[key]


def differ(got, want):
    return int((np.ascontiguousarray(got).view(np.uint32) != np.ascontiguousarray(want).view(np.uint32)).sum())


# ---- 1. bits ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nv", (0, 1), ids=("cmn", "cvn"))
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_every_row_is_the_restatements_bits(pkg, case, nv):
    N, center, mw = case
    out, rows, total, frames = raw_rows(pkg)
    m = base(pkg)
    try:
        pcm, rows2, total2, _ = plan(m, utts())
        assert total2 == total and list(rows2) == list(rows)
        m.batch_set_sliding_norm(N, mw, center, nv)
        assert m.batch_output_width() == 42
        got = m.batch_run_host(pcm)
    finally:
        m.close()
    want = want_rows(pkg, N, center, mw, nv)
    for u, (g, w) in enumerate(zip(split(got, rows, frames), split(want, rows, frames))):
        assert R.same_bits(g, w), "%s nv %d: utterance %d (%d rows): %d elements differ" % (case_id(case), nv, u, frames[u], differ(g, w))
    assert not R.same_bits(got, out)


@pytest.mark.parametrize("case", ((600, 0, 100), (300, 1, 0)), ids=case_id)
def test_one_utterance_of_5000_frames_across_many_chunks(pkg, case):
    N, center, mw = case
    m = base(pkg)
    try:
        pcm, rows, total, frames = plan(m, [utterance(5000, 77)])
        assert frames == [5000]
        raw = m.batch_run_host(pcm)
        for nv in (0, 1):
            m.batch_set_sliding_norm(N, mw, center, nv)
            got = m.batch_run_host(pcm)
            want = R.sliding_norm(raw, N, mw, center, nv, exact=False)[0]
            assert R.same_bits(got, want), "%s nv %d: %d elements differ" % (case_id(case), nv, differ(got, want))
    finally:
        m.close()


# ---- 2. widths -------------------------------------------------------------------------------------------------------

def _fbank(nb, dyn=0):
    return lambda pkg: base(pkg, num_banks=nb, ceps_len=0, want_c0=False, dyn=dyn)


def _plp(pkg):
    m = pkg.MfccHip(200000, W, S, 26, SR, 64.0, SR / 2, 13, False, 22.0, pkg.NORM_NONE, pkg.DYN_ACC, 3, 3, True, device=0, bug_compat=False,
                    method=pkg.METHOD_PLP, lpc_order=12)
    m.set_window(pkg.reference_window(W))
    return m


def _traps(pkg):
    m = pkg.MfccHip(200000, W, S, 15, SR, 64.0, SR / 2, 0, False, 22.0, pkg.NORM_NONE, pkg.DYN_NONE, 3, 3, True, device=0, bug_compat=False,
                    method=pkg.METHOD_TRAPS, traps_len=31, traps_dct_len=10)
    m.set_window(pkg.reference_window(W))
    return m


def _kaldi(nb, nc, flags=0):
    def mk(pkg):
        m = pkg.MfccHip(200000, W, S, nb, SR, 20.0, 0.0, nc, False, 22.0, pkg.NORM_NONE, pkg.DYN_NONE, 2, 2, True, device=0, bug_compat=False,
                        method=pkg.METHOD_KALDI, kaldi_flags=flags)
        m.set_window(pkg.povey_window(W))
        m.kaldi_set_options(0.97, True, True)
        return m
    return mk


WIDTHS = {
    # name: (maker, Wy)
    "w1": (lambda pkg: base(pkg, ceps_len=1, want_c0=False, dyn=pkg.DYN_NONE), 1),
    "w13": (lambda pkg: base(pkg, ceps_len=13, want_c0=False, dyn=pkg.DYN_NONE), 13),
    "w80_kaldi_fbank": (_kaldi(80, 0), 80),
    "w150_traps": (_traps, 150),
    "w256_128_bands_and_deltas": (_fbank(128, dyn=1), 256),
    "plp39": (_plp, 39),
    "kaldi_mfcc13_no_snip_edges_use_energy": (lambda pkg: _kaldi(23, 13, pkg.mfcc.KALDI_NO_SNIP_EDGES | pkg.mfcc.KALDI_USE_ENERGY)(pkg), 13),
}


@pytest.mark.parametrize("name", list(WIDTHS))
def test_widths_and_front_ends(pkg, name):
    maker, Wy = WIDTHS[name]
    m = maker(pkg)
    try:
        assert m.get_output_data_width() == Wy
        lens = [S * T + 250 for T in (3, 40, 70, 130)]          # (every front end frames these: a few to > 128 frames)
        us = [synth_utterance(n, 40 + k) for k, n in enumerate(lens)]
        pcm, rows, total, frames = plan(m, us)
        assert min(frames) >= 1 and max(frames) > 64
        raw = m.batch_run_host(pcm)
        for N, center, mw, nv in ((300, 1, 0, 1), (33, 1, 0, 0), (64, 0, 1, 1)):
            m.batch_set_sliding_norm(N, mw, center, nv)
            got = m.batch_run_host(pcm)
            assert got.shape == (total, Wy)
            for u, (g, x) in enumerate(zip(split(got, rows, frames), split(raw, rows, frames))):
                want = R.sliding_norm(x, N, mw, center, nv, exact=False)[0]
                assert R.same_bits(g, want), "%s N %d: utterance %d: %d elements differ" % (name, N, u, differ(g, want))
    finally:
        m.close()


def test_more_than_256_columns_are_refused(pkg):
    m = _fbank(128, dyn=2)(pkg)
    try:
        assert m.get_output_data_width() == 384
        pcm, rows, total, frames = plan(m, [synth_utterance(4000, 1)])
        raw = m.batch_run_host(pcm)
        assert status_of(m.batch_set_sliding_norm, 300, 0, True, False) == CONFIG
        assert R.same_bits(m.batch_run_host(pcm), raw)
    finally:
        m.close()


# ---- 3. against float64, independently of the prefix form ----------------------------------------------------------------

@pytest.mark.parametrize("nv", (0, 1), ids=("cmn", "cvn"))
def test_rows_against_float64_sums_of_every_window(pkg, nv):
    """N >= 32, T >= 32, min_window >= 32: every window holds >= 32 rows and no row is left out.  |y - y64| <= B at every
    element, y64 from np.longdouble sums of each window (nothing rounded, exact squares), B = slide_ref.bound."""
    out, rows, total, frames = raw_rows(pkg)
    m = base(pkg)
    try:
        pcm, _, _, _ = plan(m, utts())
        for N, center, mw in ((300, 1, 0), (301, 1, 0), (32, 1, 0), (4096, 1, 0), (600, 0, 100), (64, 0, 64)):
            m.batch_set_sliding_norm(N, mw, center, nv)
            got = m.batch_run_host(pcm)
            worst, n = 0.0, 0
            for u, (g, x) in enumerate(zip(split(got, rows, frames), split(out, rows, frames))):
                if frames[u] < 32:
                    continue
                _, y64, _, _, B = R.sliding_norm(x, N, mw, center, nv)
                assert np.isfinite(g).all()
                err = np.abs(g.astype(np.float64) - y64)
                bad = np.argwhere(~(err <= B))
                assert bad.size == 0, "%s nv %d: utterance %d: |y - y64| > B at %d elements, first (row, column) %s: err %.3g, B %.3g" % (
                    case_id((N, center, mw)), nv, u, len(bad), tuple(bad[0]), err[tuple(bad[0])], B[tuple(bad[0])])
                with np.errstate(invalid="ignore", divide="ignore"):
                    worst = max(worst, float(np.nanmax(np.where(B > 0, err / B, 0.0))))
                n += frames[u]
            assert n == sum(T for T in FRAMES if T >= 32)
            print("%s %s: worst err / B %.3g over %d rows" % (case_id((N, center, mw)), "cvn" if nv else "cmn", worst, n))
    finally:
        m.close()


# ---- 4. composition ------------------------------------------------------------------------------------------------------

SET = (300, 0, True, True)   # window, min_window, center, norm_vars: the x-vector recipe's window, with variances


@pytest.mark.parametrize("mode", ("SELECT", "PACK"))
def test_the_vad_decides_on_the_raw_rows_and_moves_the_normalised_ones(pkg, mode):
    out, rows, total, frames = raw_rows(pkg)
    want = want_rows(pkg, 300, True, 0, 1)
    vad = (-1, 0.0, 1.0, 2, 0.6)                                # c0 above the utterance's mean, with a context
    m = base(pkg)
    try:
        pcm, _, _, _ = plan(m, utts())
        m.batch_set_vad(*vad, pkg.VAD_FLAGS)
        assert R.same_bits(m.batch_run_host(pcm), out)
        flags, voiced, thr, tot = m.batch_vad_read()
        assert 0 < tot < total
        m.batch_set_sliding_norm(*SET)
        m.batch_set_vad(*vad, getattr(pkg, "VAD_" + mode))
        got = m.batch_run_host(pcm)
        f2, v2, t2, tot2 = m.batch_vad_read()
        assert np.array_equal(f2, flags) and np.array_equal(v2, voiced) and tot2 == tot
        assert np.array_equal(t2.view(np.uint32), thr.view(np.uint32))
        ref = VR.select_ref(want, rows, frames, flags) if mode == "SELECT" else VR.pack_ref(want, rows, frames, flags)[0]
        assert R.same_bits(got, ref), "%d elements differ" % differ(got, ref)
        # FLAGS with the normaliser: the normalised rows, the same decision
        m.batch_set_vad(*vad, pkg.VAD_FLAGS)
        assert R.same_bits(m.batch_run_host(pcm), want) and np.array_equal(m.batch_vad_read()[0], flags)
    finally:
        m.close()


def test_the_transform_and_the_tensor_read_the_normalised_rows(pkg):
    out, rows, total, frames = raw_rows(pkg)
    want = want_rows(pkg, 300, True, 0, 1)
    rng = np.random.default_rng(21)
    left, right, od = 2, 1, 20
    A = rng.standard_normal((od, (left + right + 1) * 42)).astype(np.float32)
    b = rng.standard_normal(od).astype(np.float32)
    m = base(pkg)
    try:
        pcm, _, _, _ = plan(m, utts())
        m.batch_set_transform(A, b, left=left, right=right)
        m.batch_set_sliding_norm(*SET)
        got = m.batch_run_host(pcm)
        assert got.shape == (total, od)
        XR.assert_xform_consistent(got, want, [int(r) for r in rows], list(frames), A, b, left, right, what="sliding norm + transform")
        m.batch_set_transform(None)
        assert R.same_bits(m.batch_run_host(pcm), want)
        Tp = 320
        m.batch_set_tensor(TR.CHANNEL_MAJOR, TR.F16, Tp, -1.0)
        t = m.batch_run_host(pcm)
        assert t.shape == (len(FRAMES), 42, Tp) and t.dtype == np.float16
        assert TR.same_bits(t, TR.tensor_ref(want, rows, frames, Tp, TR.CHANNEL_MAJOR, TR.F16, -1.0), TR.F16)
    finally:
        m.close()


def test_pasted_pitch_columns_are_normalised_too(pkg):
    m = base(pkg)
    try:
        us = [utterance(T, 30 + k) for k, T in enumerate((150, 33, 301))]
        pcm, rows, total, frames = plan(m, us)
        m.batch_set_pitch(40, 200, window=400, lag_cost=0.1, penalty=0.1)
        m.batch_set_pitch_feats(columns=0, left=20, right=20, delta_window=2, paste=True)
        Wy = m.batch_output_width()
        assert Wy == 45
        wide = m.batch_run_host(pcm)
        m.batch_set_sliding_norm(*SET)
        got = m.batch_run_host(pcm)
        assert got.shape == (total, Wy)
        for u, (g, x) in enumerate(zip(split(got, rows, frames), split(wide, rows, frames))):
            want = R.sliding_norm(x, 300, 0, True, True, exact=False)[0]
            assert R.same_bits(g, want), "utterance %d: %d elements differ" % (u, differ(g, want))
        assert R.same_bits(m.batch_pitch_feats_read(), wide[:, 42:])     # (the read-back stays raw)
        assert status_of(m.batch_clear_pitch) == STATE                    # the row width is held while the normaliser is on
        assert status_of(m.batch_set_pitch_feats, paste=False) == STATE
        m.batch_clear_sliding_norm()
        assert R.same_bits(m.batch_run_host(pcm), wide)
    finally:
        m.close()


def test_a_rates_plan_in_front(pkg):
    a, b = utterance(150, 51), utterance(70, 52)
    pcm = np.concatenate((a[::2], FULL, b, FULL))                # utterance 0 arrives at 8 kHz
    offs, lens, rates = [0, a[::2].size + FULL.size], [a[::2].size, b.size], [8000, 16000]
    m = base(pkg)
    try:
        rows, total = m.batch_plan_rates(offs, lens, rates)
        raw = m.batch_run_host(pcm)
        frames = [int(rows[1] - rows[0]), int(total - rows[1])]
        assert min(frames) > 60
        m.batch_set_sliding_norm(64, 32, False, True)
        got = m.batch_run_host(pcm)
        for u, (g, x) in enumerate(zip(split(got, rows, frames), split(raw, rows, frames))):
            assert R.same_bits(g, R.sliding_norm(x, 64, 32, False, True, exact=False)[0]), u
    finally:
        m.close()


# ---- 5. contract ---------------------------------------------------------------------------------------------------------

def test_alone_in_the_batch_a_second_run_overlap_clear_and_a_new_plan(pkg):
    out, rows, total, frames = raw_rows(pkg)
    want = want_rows(pkg, 300, True, 0, 1)
    m = base(pkg)
    try:
        for u in (16, 11, 4, 1):                                 # 700, 151, 32 frames and 1 frame: each alone
            pcm1, r1, t1, f1 = plan(m, [utts()[u]])
            m.batch_set_sliding_norm(*SET)
            alone = m.batch_run_host(pcm1)
            assert R.same_bits(alone, want[int(rows[u]):int(rows[u]) + frames[u]]), "alone: utterance %d" % u
        pcm, _, _, _ = plan(m, utts())
        assert R.same_bits(m.batch_run_host(pcm), out)           # the new plan dropped the attachment
        m.batch_set_sliding_norm(*SET)
        first = m.batch_run_host(pcm)
        assert R.same_bits(first, want) and R.same_bits(m.batch_run_host(pcm), want)
        m.batch_overlap(True)
        for _ in range(3):                                       # both statics buffers re-used
            assert R.same_bits(m.batch_run_host(pcm), want)
        m.batch_overlap(False)
        m.batch_clear_sliding_norm()
        assert R.same_bits(m.batch_run_host(pcm), out)
        m.batch_clear_sliding_norm()                             # (clearing nothing is no error)
    finally:
        m.close()


@pytest.mark.parametrize("k", (0, 1, 2, 3))
def test_d_out_at_every_4_byte_placement(pkg, k):
    import torch
    out, rows, total, frames = raw_rows(pkg)
    want = want_rows(pkg, 600, False, 100, 1)
    m = base(pkg)
    try:
        m.set_stream(torch.cuda.current_stream().cuda_stream)    # (the guards' fills and the run are then ordered)
        pcm, _, _, _ = plan(m, utts())
        m.batch_set_sliding_norm(600, 100, False, True)
        d_pcm = torch.from_numpy(pcm.copy()).to("cuda:0")
        op = OutPlacement(total, 42, k=k)
        m.batch_run_device(d_pcm.data_ptr(), len(pcm), op.ptr)
        m.synchronize()
        got = op.check("d_out %d floats past a 16-byte boundary" % k).cpu().numpy()
        assert R.same_bits(got, want), "%d elements differ" % differ(got, want)
    finally:
        m.close()


# ---- 6. refusals ---------------------------------------------------------------------------------------------------------

def status_of(fn, *args, **kw):
    try:
        fn(*args, **kw)
        return 0
    except Exception as e:                                   # MfxError (the package is loaded under an alias)
        return e.status


def test_refusals_leave_the_handle_on_its_previous_bits(pkg):
    import stft_drive
    out, rows, total, frames = raw_rows(pkg)
    m = base(pkg)
    try:
        assert status_of(m.batch_set_sliding_norm, 300, 0, True, False) == STATE      # before a plan
        pcm, _, _, _ = plan(m, utts())
        L = m._L
        for bad in ((0, 0, 1, 0), (-1, 0, 1, 0), (4097, 0, 1, 0), (300, -1, 0, 0), (300, 301, 0, 0), (300, 0, 2, 0), (300, 0, -1, 0),
                    (300, 0, 1, 2), (300, 0, 1, -1)):
            assert L.mfx_batch_set_sliding_norm(m._h, *bad) == ARG, bad
            assert R.same_bits(m.batch_run_host(pcm), out), bad
        m.batch_set_sliding_norm(600, 100, False, False)
        kept = m.batch_run_host(pcm)
        assert R.same_bits(kept, want_rows(pkg, 600, False, 100, 0))
        assert L.mfx_batch_set_sliding_norm(m._h, 0, 0, 1, 0) == ARG                   # a refusal keeps the setting in force
        assert R.same_bits(m.batch_run_host(pcm), kept)
    finally:
        m.close()
    for norm in (pkg.NORM_CMN, pkg.NORM_CVN):                    # it replaces the other normalisers, it does not stack on them
        h = base(pkg, norm=norm)
        try:
            assert status_of(h.batch_set_sliding_norm, 300, 0, True, False) == CONFIG  # (before a plan: the configuration first)
            pcm, _, _, _ = plan(h, utts()[:6])
            before = h.batch_run_host(pcm)
            assert status_of(h.batch_set_sliding_norm, 300, 0, True, False) == CONFIG
            assert R.same_bits(h.batch_run_host(pcm), before)
        finally:
            h.close()
    s = stft_drive.make(pkg, 400, 160, 80, SR, post=pkg.LOGMEL_LOG10)
    try:
        x = synth_utterance(8000, 3)
        s.batch_plan([0], [x.size])
        before = s.batch_run_host(x)
        assert status_of(s.batch_set_sliding_norm, 300, 0, True, False) == CONFIG
        assert R.same_bits(s.batch_run_host(x), before)
    finally:
        s.close()


# ---- 7. the entries around it ----------------------------------------------------------------------------------------------

def test_a_sliced_host_run_equals_the_device_entry(pkg):
    """8 utterances, 32 MB of PCM, ascending offsets, pinned buffers: mfx_batch_run_host takes its sliced path (utterances are
    independent under the sliding normaliser) and gives the device entry's bits."""
    import torch
    L = pkg.load_library()
    L.mfx_alloc_pinned.restype, L.mfx_alloc_pinned.argtypes = C.c_void_p, [C.c_size_t]
    L.mfx_free_pinned.restype, L.mfx_free_pinned.argtypes = None, [C.c_void_p]
    one = synth_utterance(2100000, 123)
    n_utt = 8
    offs = [u * one.size for u in range(n_utt)]
    lens = [one.size - 160 * u for u in range(n_utt)]
    pos = n_utt * one.size
    assert pos * 2 >= 32 << 20
    m = base(pkg)
    rows, total = m.batch_plan(offs, lens)
    m.batch_set_sliding_norm(300, 0, True, True)
    p_in, p_out = L.mfx_alloc_pinned(pos * 2), L.mfx_alloc_pinned(total * 42 * 4)
    assert p_in and p_out
    try:
        for u in range(n_utt):
            C.memmove(p_in + 2 * offs[u], one.ctypes.data, one.size * 2)
        rc = L.mfx_batch_run_host(m._h, C.cast(p_in, C.POINTER(C.c_int16)), pos, C.cast(p_out, C.POINTER(C.c_float)))
        assert rc == 0, L.mfx_last_error(m._h)
        got = np.ctypeslib.as_array(C.cast(p_out, C.POINTER(C.c_float)), shape=(total, 42)).copy()
        pcm = torch.from_numpy(np.ctypeslib.as_array(C.cast(p_in, C.POINTER(C.c_int16)), shape=(pos,)).copy()).to("cuda:0")
    finally:
        L.mfx_free_pinned(p_in)
        L.mfx_free_pinned(p_out)
    out = torch.full((total, 42), float("nan"), dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    m.batch_run_device(pcm.data_ptr(), pcm.numel(), out.data_ptr())
    m.synchronize()
    m.close()
    assert R.same_bits(out.cpu().numpy(), got) and np.isfinite(got).all()
    # a row's window ends 150 rows ahead of it: utterance 1, one hop shorter, has utterance 0's rows until the end comes into reach
    T1 = int(rows[2] - rows[1]) - 160
    assert T1 > 12000 and R.same_bits(got[rows[0]:rows[0] + T1], got[rows[1]:rows[1] + T1])


def exe_path():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "asr-featext-opencl_amd", "host", "afet_hip")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", os.path.dirname(exe)])
    return exe


def write_wav(path, pcm):
    with wave.open(str(path), "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(16000)
        w.writeframes(np.ascontiguousarray(pcm, "<i2").tobytes())


def read_htk(path):
    raw = open(path, "rb").read()
    n, size = int.from_bytes(raw[0:4], "big"), int.from_bytes(raw[8:10], "big")
    return np.frombuffer(raw[12:], ">f4").astype(np.float32).reshape(n, size // 4)


def test_driver_cmn_window_equals_the_binding(pkg, a0001, tmp_path):
    exe = exe_path()
    pcms = [a0001, a0001[500:100500].copy(), a0001[1000:81000].copy()]
    args = []
    for i, p in enumerate(pcms):
        write_wav(tmp_path / ("in%d.wav" % i), p)
        args += [str(tmp_path / ("in%d.wav" % i)), str(tmp_path / ("out%d.htk" % i))]
    opts = ["--banks", "40", "--ceps", "13", "--c0", "0", "--norm", "0", "--dyn", "2", "--htk", "--batch-mb", "4"]
    subprocess.check_call([exe] + opts + ["--cmn-window", "300", "--cmn-center", "1", "--cmn-norm-vars"] + args, stdout=subprocess.DEVNULL)
    m = pkg.MfccHip(10000000, 400, 160, 40, 16000.0, 64.0, 8000.0, 13, False, 22.0, pkg.NORM_NONE, pkg.DYN_ACC, 3, 3, True, device=0,
                    engine=pkg.mfcc.ENGINE_STREAM_KERNELS)
    m.set_window(pkg.reference_window(400))
    us = [np.ascontiguousarray(p) for p in pcms]
    pcm, rows, total, frames = plan(m, us)
    raw = m.batch_run_host(pcm)
    m.batch_set_sliding_norm(300, 0, True, True)
    want = m.batch_run_host(pcm)
    m.close()
    for i in range(len(pcms)):
        got = read_htk(tmp_path / ("out%d.htk" % i))
        w = want[int(rows[i]):int(rows[i]) + frames[i]]
        assert got.shape == w.shape and R.same_bits(got, w), "file %d" % i
        assert not R.same_bits(got, raw[int(rows[i]):int(rows[i]) + frames[i]])
    spk = tmp_path / "spk.txt"
    spk.write_text("a\nb\na\n")
    for extra, word in ((["--cmn-window", "300", "--spk-file", str(spk)], "--spk-file"), (["--cmn-window", "5000"], "1 .. 4096"),
                        (["--cmn-window", "300", "--norm", "2"], "--norm 0"), (["--cmn-window", "300", "--batch-mb", "0"], "--batch-mb"),
                        (["--cmn-window", "300", "--online-window", "96"], "--online-window"),
                        (["--cmn-window", "300", "--cmn-min-window", "301"], "--cmn-min-window")):
        r = subprocess.run([exe] + opts + extra + args, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True)
        assert r.returncode != 0 and word in r.stderr, (extra, r.stderr)
