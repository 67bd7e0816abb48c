"""The session transform (mfx_sessions_set_transform; k_sess_xform) on the MI355X.

The oracle is the batch entry with mfx_batch_set_transform on a twin handle of the same configuration: existing, separately
tested code (tests/test_transform_gpu.py), never the code under test.  The rows a session delivers must be the twin's rows
of the whole utterance bit for bit (compared as uint32), however the stream is cut.  One case checks the rows against the
float64 restatement of tests/xform_ref.py as well, every value inside its own gamma_n bound (derived there, not tuned)."""
import ctypes as C

import numpy as np
import pytest

import sess_xform_drive as SD
import xform_ref as XR
from conftest import synth_utterance
from placement import OutPlacement

pytestmark = pytest.mark.gpu

FRAMES = [0, 1, 2, 3, 7, 8, 17, 40, 100]                      # SD.utterances appends a silent utterance of 40 frames
XFORM_VALU, PLAIN = 1024, 4096

_UTTS, _WANT = {}, {}


def utts_of(name, frames=FRAMES, silent=40):
    key = (name, tuple(frames), silent)
    if key not in _UTTS:
        _UTTS[key] = SD.utterances(name, list(frames), silent_frames=silent)
    return _UTTS[key]


def matrices(seed, n_xf, out_dim, in_dim):
    rng = np.random.default_rng(seed)
    A = (rng.standard_normal((n_xf, out_dim, in_dim)) / np.sqrt(in_dim)).astype(np.float32)
    b = rng.standard_normal((n_xf, out_dim)).astype(np.float32)
    return A, b


def shape(pkg, name, left, right, out_dim, n_xf=1, over=None):
    """(kw, A, b) of a case: the configuration and seeded matrices of its in_dim."""
    kw = dict(SD.CONFIGS[name], **(over or {}))
    width = SD.OD.cols_of(kw) * (1 + kw["dyn"])
    A, b = matrices(left * 1000 + right * 10 + out_dim, n_xf, out_dim, (left + right + 1) * width)
    return kw, A, b


def want_rows(pkg, key, kw, utts, A, b, left, right, utt_xf=None, norm=0, nad=True, onorm=None):
    """The oracle's rows (computed once per key, shared, never changed): the batch entry with the same transform."""
    if key not in _WANT:
        t = SD.make(pkg, kw, norm=norm, nad=nad)

        def setup(h):
            if onorm is not None:
                h.batch_set_online_norm(onorm)
            h.batch_set_transform(A, b, left=left, right=right, utt_xf=utt_xf)

        rows = SD.batch_rows(t, utts, setup=setup)
        t.close()
        for r in rows:
            r.setflags(write=False)
        _WANT[key] = rows
    return _WANT[key]


def session_handle(pkg, kw, A, b, left, right, n_sessions, max_push=SD.MAX_PUSH, norm=0, nad=True, onorm=None, engine=None):
    m = SD.make(pkg, kw, norm=norm, nad=nad, **({} if engine is None else dict(engine=engine)))
    if onorm is not None:
        m.sessions_set_online_norm(onorm)
    m.sessions_set_transform(A, b, left=left, right=right)
    assert m.sessions_output_width() == A.shape[-2]
    m.sessions_create(n_sessions, max_push)
    return m


def run_pattern(m, utts, pattern, seed, right, **kw):
    p = SD.PATTERNS[pattern]
    return SD.drive(m, utts, p["n_sessions"], p["cut"], seed, right, subset=p.get("subset", False), **kw)


# ---- 1. the C1 stage: every cut pattern, both entries, odd source offsets -----------------------------------------------

@pytest.mark.parametrize("mode", ("device", "host", "odd_offsets"))
@pytest.mark.parametrize("pattern", sorted(SD.PATTERNS))
def test_c1_splice4_to_40_every_pattern(pkg, pattern, mode):
    """Wd = 39, +-4 -> 40: in_dim 351 is no multiple of 4, three output tiles.  whole_utterance_final delivers pieces of up to
    100 rows: several row groups per session."""
    kw, A, b = shape(pkg, "c1", 4, 4, 40)
    utts = utts_of("c1")
    want = want_rows(pkg, "c1-4-4-40", kw, utts, A[0], b[0], 4, 4)
    assert [len(w) for w in want] == FRAMES + [40] and want[-2].shape[1] == 40
    p = SD.PATTERNS[pattern]
    m = session_handle(pkg, kw, A, b, 4, 4, p["n_sessions"], p.get("max_push", SD.MAX_PUSH))
    try:
        got = run_pattern(m, utts, pattern, 11, 4, host=mode == "host", odd_offsets=mode == "odd_offsets")
        SD.compare("c1", got, want, "xform %s, %s" % (pattern, mode))
    finally:
        m.close()


# ---- 2. shapes ----------------------------------------------------------------------------------------------------------

SHAPES = [
    # (id, configuration, overrides, left, right, out_dim, frames, silent frames)
    ("c1-0-0-o1", "c1", None, 0, 0, 1, FRAMES, 40),
    ("c1-1-1-o16", "c1", None, 1, 1, 16, FRAMES, 40),
    ("c1-1-1-o17", "c1", None, 1, 1, 17, FRAMES, 40),
    ("c1-1-1-o33", "c1", None, 1, 1, 33, FRAMES, 40),
    # most utterances are shorter than `right`: everything at the final push, with both clamps
    ("fbank40-0-32-o24", "fbank40", dict(dyn=0), 0, 32, 24, FRAMES, 40),
    ("c1dyn0-32-32-o256", "c1", dict(dyn=0), 32, 32, 256, FRAMES, 40),        # the 16-tile instantiation
    # Wd = 120, 65 frames of context: in_dim 7800, the row groups per block fall (three short utterances)
    ("stereo44k-32-32-o16", "stereo44k", None, 32, 32, 16, [3, 34, 70], 5),
    ("stereo44k-32-32-o256", "stereo44k", None, 32, 32, 256, [3, 34, 70], 5),
    ("plp12-4-4-o40", "plp12", None, 4, 4, 40, FRAMES, 40),
]


@pytest.mark.parametrize("pattern", ("one_hop_per_push", "random_empty_and_flush"))
@pytest.mark.parametrize("case", SHAPES, ids=[c[0] for c in SHAPES])
def test_shapes(pkg, case, pattern):
    what, name, over, left, right, out_dim, frames, silent = case
    kw, A, b = shape(pkg, name, left, right, out_dim, over=over)
    utts = utts_of(name, frames, silent)
    want = want_rows(pkg, what, kw, utts, A[0], b[0], left, right)
    assert [len(w) for w in want] == list(frames) + [silent]
    p = SD.PATTERNS[pattern]
    m = session_handle(pkg, kw, A, b, left, right, p["n_sessions"])
    try:
        got = run_pattern(m, utts, pattern, 5, right)
        SD.compare(name, got, want, "xform %s, %s" % (what, pattern))
    finally:
        m.close()


def test_thirteen_sessions_leave_the_last_block_partly_filled(pkg):
    """13 open sessions, a hop per push: 13 row groups are three full blocks of four and one of one."""
    kw, A, b = shape(pkg, "c1", 4, 4, 40)
    base = utts_of("c1")
    want10 = want_rows(pkg, "c1-4-4-40", kw, base, A[0], b[0], 4, 4)
    order = [9, 8, 7, 6, 5, 9, 8, 7, 6, 5, 9, 8, 7]             # 13 utterances with frames, all open at once
    utts, want = [base[u] for u in order], [want10[u] for u in order]
    m = session_handle(pkg, kw, A, b, 4, 4, 13)
    try:
        got = SD.drive(m, utts, 13, SD.OD.cut_hop, 3, 4)
        SD.compare("c1", got, want, "xform, 13 sessions")
    finally:
        m.close()


# ---- 3. a transform per session -----------------------------------------------------------------------------------------

def test_per_session_transforms_against_utt_xf(pkg):
    """3 matrices over 7 sessions, matrix 1 unused; ids are reused with a new selection.  A selection on a session that is
    not fresh answers MFX_ERR_STATE and changes nothing."""
    kw, A, b = shape(pkg, "c1", 2, 3, 24, n_xf=3)
    utts = utts_of("c1")
    utt_xf = [0, 2, 2, 0, 2, 0, 0, 2, 0, 2]
    want = want_rows(pkg, "c1-2-3-24-x3", kw, utts, A, b, 2, 3, utt_xf=utt_xf)
    m = session_handle(pkg, kw, A, b, 2, 3, 7, max_push=20000)
    try:
        got = SD.drive(m, utts, 7, SD.OD.cut_random, 17, 3, xf_of=utt_xf)
        SD.compare("c1", got, want, "xform, 3 transforms over 7 sessions")
        # a session that is not fresh
        x = utts[7].reshape(-1)                                 # 40 frames, transform 2 in the batch
        m.sessions_select_transform(3, 2)
        m.sessions_plan([3], [0], [2000])
        m.sessions_run_host(x[:2002])
        with pytest.raises(pkg.MfxError) as e:
            m.sessions_select_transform(3, 0)
        assert e.value.status == -8 and str(e.value)
        _, counts, total = m.sessions_plan([3], [2000], [len(x) - 2000], [1])
        out = m.sessions_run_host(x)
        rows = m.batch_frames(2000) - 6 - 3
        assert total == 40 - rows and np.array_equal(out.view(np.uint32), want[7][rows:].view(np.uint32))   # still transform 2
        # the choice stays with the id across the final push and a reset
        m.sessions_reset(3)
        m.sessions_plan([3], [0], [len(x)], [1])
        assert np.array_equal(m.sessions_run_host(x).view(np.uint32), want[7].view(np.uint32))
        for bad in ((7, 0), (-1, 0), (0, 3), (0, -1)):
            with pytest.raises(pkg.MfxError) as e:
                m.sessions_select_transform(*bad)
            assert e.value.status == -7
        # mfx_sessions_create puts all back to 0
        m.sessions_create(7, 20000)
        w0 = want_rows(pkg, "c1-2-3-24-x3-all0", kw, utts, A, b, 2, 3, utt_xf=[0] * 10)
        m.sessions_plan([3], [0], [len(utts[7])], [1])
        assert np.array_equal(m.sessions_run_host(utts[7].reshape(-1)).view(np.uint32), w0[7].view(np.uint32))
    finally:
        m.close()


@pytest.mark.parametrize("engine", (0, PLAIN), ids=("packed", "plain"))
def test_shuffled_pieces_three_transforms_behind_the_online_normaliser(pkg, engine):
    """The pieces of every push in a random order of ids, over a changing subset of 5 sessions, with empty pushes and flushes:
    caller order, slot order and the packer's order (sorted by transform) all differ.  Three transforms dealt by utterance,
    +2 / -3 -> 24, the online normaliser behind the deltas; the rows are still the twin's, bit for bit."""
    kw, A, b = shape(pkg, "c1", 2, 3, 24, n_xf=3)
    utts = utts_of("c1")
    utt_xf = [u % 3 for u in range(len(utts))]
    want = want_rows(pkg, "c1-2-3-24-x3-onorm-cvn", kw, utts, A, b, 2, 3, utt_xf=utt_xf, norm=2, nad=True, onorm=32)
    assert [len(w) for w in want] == FRAMES + [40]
    m = session_handle(pkg, kw, A, b, 2, 3, 5, norm=2, nad=True, onorm=32, engine=engine)
    try:
        got = SD.drive(m, utts, 5, SD.OD.cut_random_with_empty, 23, 3, subset=True, shuffle=True, xf_of=utt_xf)
        SD.compare("c1", got, want, "xform, shuffled pieces, %s" % ("plain" if engine else "packed"))
    finally:
        m.close()


# ---- 4. behind the online normaliser ------------------------------------------------------------------------------------

@pytest.mark.parametrize("nad", (True, False), ids=("after", "before"))
@pytest.mark.parametrize("kind", (1, 2), ids=("cmn", "cvn"))
def test_online_normaliser_then_transform(pkg, kind, nad):
    kw, A, b = shape(pkg, "c1", 4, 4, 40)
    utts = utts_of("c1")
    want = want_rows(pkg, ("c1-4-4-40-onorm", kind, nad), kw, utts, A[0], b[0], 4, 4, norm=kind, nad=nad, onorm=32)
    m = session_handle(pkg, kw, A, b, 4, 4, 10, norm=kind, nad=nad, onorm=32)
    try:
        got = run_pattern(m, utts, "random_empty_and_flush", 29, 4)
        SD.compare("c1", got, want, "online %s %s + xform" % ("cmn" if kind == 1 else "cvn", "after" if nad else "before"))
    finally:
        m.close()


# ---- 5. engine bits and placement ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("engine", (XFORM_VALU, PLAIN, XFORM_VALU | PLAIN), ids=("valu", "plain", "valu+plain"))
def test_engine_bits_deliver_the_defaults_bits(pkg, engine):
    kw, A, b = shape(pkg, "c1", 4, 4, 40)
    utts = utts_of("c1")
    want = want_rows(pkg, "c1-4-4-40", kw, utts, A[0], b[0], 4, 4)
    assert pkg.mfcc.ENGINE_SESS_XFORM_PLAIN == PLAIN and pkg.mfcc.ENGINE_XFORM_VALU == XFORM_VALU
    for pattern in ("whole_utterance_final", "changing_subset"):
        p = SD.PATTERNS[pattern]
        m = session_handle(pkg, kw, A, b, 4, 4, p["n_sessions"], p.get("max_push", SD.MAX_PUSH), engine=engine)
        try:
            got = run_pattern(m, utts, pattern, 7, 4)
            SD.compare("c1", got, want, "xform engine %d, %s" % (engine, pattern))
        finally:
            m.close()


@pytest.mark.parametrize("engine", (0, PLAIN), ids=("packed", "plain"))
@pytest.mark.parametrize("out_dim", (40, 33))
def test_rows_do_not_depend_on_where_d_out_lies(pkg, out_dim, engine):
    """d_out at every 4-byte position of a 16-byte word inside a guarded allocation: the same bits, the guards intact
    (out_dim 40: whole 16-byte words where the pointer allows; 33: single floats)."""
    kw, A, b = shape(pkg, "c1", 1, 1, out_dim)
    utts = utts_of("c1")
    want = want_rows(pkg, "c1-1-1-o%d-place" % out_dim, kw, utts, A[0], b[0], 1, 1)
    m = session_handle(pkg, kw, A, b, 1, 1, 10, engine=engine)
    try:
        for k in range(4):
            got = SD.drive(m, utts, 10, SD.OD.cut_random, 40 + k, 1, place=lambda rows, width: OutPlacement(rows, width, k))
            SD.compare("c1", got, want, "xform o%d, d_out + %d floats" % (out_dim, k))
    finally:
        m.close()


# ---- 6. state -----------------------------------------------------------------------------------------------------------

def test_reset_mid_stream_and_plan_twice(pkg):
    kw, A, b = shape(pkg, "c1", 4, 4, 40)
    utts = utts_of("c1")
    want = want_rows(pkg, "c1-4-4-40", kw, utts, A[0], b[0], 4, 4)
    x, w = utts[8].reshape(-1), want[8]                         # the 100-frame utterance
    m = session_handle(pkg, kw, A, b, 4, 4, 4, max_push=20000)
    try:
        m.sessions_plan([2], [0], [5000])
        part = m.sessions_run_host(x)
        n5 = m.batch_frames(5000) - 6 - 4
        assert part.shape == (n5, 40) and m.sessions_delivered(2) == n5
        assert np.array_equal(part.view(np.uint32), w[:n5].view(np.uint32))
        m.sessions_reset(2)                                      # the carried rows y go with the rest
        assert m.sessions_delivered(2) == 0
        m.sessions_plan([2], [0], [3000], [0])                   # plan twice, run once: the second plan runs
        _, counts, total = m.sessions_plan([2], [0], [len(x)], [1])
        assert total == len(w) == counts[0]
        out = m.sessions_run_host(x)
        assert np.array_equal(out.view(np.uint32), w.view(np.uint32))
        with pytest.raises(pkg.MfxError) as e:
            m.sessions_run_host(x)
        assert e.value.status == -8
        # a flush delivers up to right + D rows with no new samples
        m.sessions_plan([1], [0], [5000])
        m.sessions_run_host(x)
        _, counts, total = m.sessions_plan([1], [0], [0], [1])
        assert total == 6 + 4
        tail = m.sessions_run_host(np.zeros(2, np.int16))
        cut = SD.make(pkg, kw)
        rows = SD.batch_rows(cut, [utts[8][:5000]], setup=lambda h: h.batch_set_transform(A[0], b[0], left=4, right=4))
        cut.close()
        assert np.array_equal(tail.view(np.uint32), rows[0][n5:].view(np.uint32))
    finally:
        m.close()


def test_batch_plan_streaming_and_transformed_sessions_on_one_handle(pkg):
    """One handle carries a batch plan with a DIFFERENT transform, a streaming sequence and transformed sessions,
    interleaved: each delivers what it delivers alone."""
    kw, A, b = shape(pkg, "c1", 4, 4, 40)
    utts = utts_of("c1")
    want = want_rows(pkg, "c1-4-4-40", kw, utts, A[0], b[0], 4, 4)
    rng = np.random.default_rng(3)
    blocks = [synth_utterance(8000, 900 + k) for k in range(3)]

    def stream_step(h, k):
        n = h.set_input(blocks[k]) if k < len(blocks) else h.flush()
        h.apply()
        return h.get_output_data(n)

    alone = SD.make(pkg, kw)
    want_stream = [stream_step(alone, k) for k in range(len(blocks) + 1)]
    alone.close()
    m = SD.make(pkg, kw)
    try:
        b_pcm = np.concatenate([synth_utterance(9000, 77), synth_utterance(7001, 78), np.zeros(3, np.int16)])
        m.batch_plan([0, 9000], [9000, 7001])
        B = rng.standard_normal((8, 3 * m.get_output_data_width())).astype(np.float32)
        m.batch_set_transform(B, None, left=1, right=1)
        batch_before = m.batch_run_host(b_pcm)
        got_stream = [stream_step(m, 0)]
        m.sessions_set_transform(A, b, left=4, right=4)
        assert m.batch_output_width() == 8 and m.sessions_output_width() == 40
        m.sessions_create(6, SD.MAX_PUSH)
        runs = []

        def on_tick(tick):
            if tick in (1, 3, 5):
                runs.append(m.batch_run_host(b_pcm))
                got_stream.append(stream_step(m, len(got_stream)))

        got = SD.drive(m, utts, 6, SD.OD.cut_random, 31, 4, on_tick=on_tick)
        assert len(runs) == 3 and len(got_stream) == 4
        SD.compare("c1", got, want, "xform, interleaved")
        for r in runs + [m.batch_run_host(b_pcm)]:
            assert r.shape == batch_before.shape and np.array_equal(r.view(np.uint32), batch_before.view(np.uint32))
        for g, w in zip(got_stream, want_stream):
            assert g.shape == w.shape and np.array_equal(g.view(np.uint32), w.view(np.uint32))
    finally:
        m.close()


def test_state_errors_and_clear(pkg):
    L = pkg.load_library()
    kw, A, b = shape(pkg, "c1", 1, 1, 8)
    utts = utts_of("c1")
    m = SD.make(pkg, kw)

    def status(fn):
        with pytest.raises(pkg.MfxError) as e:
            fn()
        assert str(e.value) and L.mfx_last_error(m._h)
        return e.value.status

    try:
        assert status(lambda: m.sessions_select_transform(0, 0)) == -8            # no transform
        wide = np.zeros((1, 4, 23 * 384), np.float32)
        fpt = C.POINTER(C.c_float)
        a = A.ctypes.data_as(fpt)
        for left, right, od, nx, ptr in ((33, 0, 8, 1, a), (0, 33, 8, 1, a), (-1, 0, 8, 1, a), (1, 1, 0, 1, a), (1, 1, 257, 1, a),
                                         (1, 1, 8, 0, a), (1, 1, 8, 1025, a), (1, 1, 8, 1, None)):
            assert L.mfx_sessions_set_transform(m._h, left, right, od, nx, ptr, None) == -7, (left, right, od, nx)
        # in_dim > 8192 cannot be reached inside left, right <= 32 at Wd = 39; at Wd = 384 (128 log mel energies + d + dd) it can
        big = SD.make(pkg, dict(SD.CONFIGS["stereo44k"], ceps_len=0))
        assert big.get_output_data_width() == 384
        assert L.mfx_sessions_set_transform(big._h, 11, 11, 4, 1, wide.ctypes.data_as(fpt), None) == -7    # 23 x 384 = 8832
        assert L.mfx_sessions_set_transform(big._h, 10, 10, 4, 1, wide.ctypes.data_as(fpt), None) == 0     # 21 x 384 = 8064
        big.close()
        m.sessions_set_transform(A, b, left=1, right=1)
        assert status(lambda: m.sessions_select_transform(0, 0)) == -8            # no sessions
        assert m.sessions_output_width() == 8 and m.get_output_data_width() == 39
        m.sessions_create(4, SD.MAX_PUSH)
        assert status(lambda: m.sessions_set_transform(A, b, left=1, right=1)) == -8   # sessions exist
        assert status(lambda: m.sessions_clear_transform()) == -8
        m.sessions_create(0, 0)
        m.sessions_clear_transform()
        assert m.sessions_output_width() == 39
        # after clear + create the rows and the width are those of a handle that never had a transform
        m.sessions_create(4, 20000)
        plain = SD.make(pkg, kw)
        w = SD.batch_rows(plain, [utts[7]])[0]
        plain.close()
        _, counts, total = m.sessions_plan([1], [0], [len(utts[7])], [1])
        out = m.sessions_run_host(utts[7].reshape(-1))
        assert total == 40 and out.shape == (40, 39) and np.array_equal(out.view(np.uint32), w.view(np.uint32))
    finally:
        m.close()


# ---- 7. against the float64 restatement ---------------------------------------------------------------------------------

def test_every_value_within_its_bound_of_the_float64_map(pkg):
    """The rows y from an untransformed SESSION twin; every transformed value inside gamma(351) (|b| + sum |A| |z|) of the
    float64 map (xform_ref.py).  The worst err / bound is printed; DESIGN.md, "Session transform", records it."""
    kw, A, b = shape(pkg, "c1", 4, 4, 40)
    utts = utts_of("c1")
    twin = SD.make(pkg, kw)
    m = session_handle(pkg, kw, A, b, 4, 4, 10)
    try:
        twin.sessions_create(10, SD.MAX_PUSH)
        p = SD.PATTERNS["random_empty_and_flush"]
        y = SD.OD.drive(twin, utts, 10, p["cut"], 13)
        got = SD.drive(m, utts, 10, p["cut"], 13, 4)
        frames = [len(y[u]) for u in range(len(utts))]
        assert frames == FRAMES + [40]
        rows = list(np.cumsum(frames) - frames)
        worst = XR.assert_xform_consistent(np.concatenate([got[u] for u in range(len(utts))]),
                                           np.concatenate([y[u] for u in range(len(utts))]), rows, frames, A[0], b[0], 4, 4,
                                           what="session transform c1 +-4 -> 40")
        print("session transform: worst err / bound = %.4g" % worst)
        assert worst > 0.0
    finally:
        twin.close()
        m.close()
