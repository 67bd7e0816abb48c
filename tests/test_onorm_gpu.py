"""The online (causal, sliding-window) CMN / CVN on the MI355X: the batch attachment (mfx_batch_set_online_norm) against
tests/onorm_ref.py of the norm = NONE twin's rows, and the session entries (mfx_sessions_set_online_norm) against the batch rows.

CMN rows are the restatement's bits: the definition uses double additions, subtractions, one division and the conversion to
float32, each a single correctly rounded operation on both sides.  CVN rows must satisfy |y - y64| <= B with
B = 2^-22 mult64 (|v| + |mean64|) at EVERY element -- four float32 roundings (mean, difference, multiplier, product), each at
most 2^-24 relative to a quantity no larger than mult (|v| + |mean|); derived, not measured -- and the tests print whether
they are the restatement's bits as well (expected where the device's double divide and square root round correctly; not a
condition).  Session rows are compared with the batch rows bit for bit, so there is no tolerance to choose."""
import ctypes as C
import os
import subprocess
import wave

import numpy as np
import pytest

import onorm_drive as OD
import onorm_ref as R
import vad_ref
from placement import OutPlacement
from tail_ref import assert_tail_consistent

pytestmark = pytest.mark.gpu

# frames per utterance: 0, 1, 31, 32, 33, N - 1, N, N + 1, N + 37, 2 N + 7 for N = 32 and N = 96; utterances() appends a
# silent one
WINDOWS = (32, 96)
FRAMES = sorted({0, 1, 31, 32, 33} | {t for N in WINDOWS for t in (N - 1, N, N + 1, N + 37, 2 * N + 7)})
PRIOR_N = 100


def prior_for(wn, seed=5):
    """(count, acc [2][wn]) of 100 rows that look like features: sums of v and of the float32 squares"""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((PRIOR_N, wn)) * 4.0 + rng.standard_normal(wn) * 10.0).astype(np.float32)
    return PRIOR_N, np.stack([x.astype(np.float64).sum(0), (x * x).astype(np.float32).astype(np.float64).sum(0)])


_UTTS, _TWIN = {}, {}


def utts_of(name):
    if name not in _UTTS:
        _UTTS[name] = OD.utterances(name, FRAMES)
    return _UTTS[name]


def twin_rows(pkg, name, key="plain", setup=None, **over):
    """The norm = NONE twin's rows of a configuration: computed once, shared, never changed."""
    if (name, key) not in _TWIN:
        t = OD.make(pkg, OD.CONFIGS[name], norm=0, **over)
        rows = OD.batch_rows(t, utts_of(name), setup=setup)
        t.close()
        for r in rows:
            r.setflags(write=False)
        _TWIN[(name, key)] = rows
    return _TWIN[(name, key)]


def check_rows(ys, xs, kw, kind, nad, N, F=0, p=0, acc=None, what=""):
    """Every utterance's rows against the restatement of the twin's rows; returns the worst err / B (0 for CMN)."""
    cols, dyn = OD.cols_of(kw), kw["dyn"]
    wn = cols * (1 + dyn) if nad else cols
    worst, bits, n = 0.0, True, 0
    for u, (y, x) in enumerate(zip(ys, xs)):
        assert y.shape == x.shape, (what, u, y.shape, x.shape)
        if x.shape[0] == 0:
            continue
        want, y64, m64, mu64 = R.online_norm(x[:, :wn], kind, N, F, p, acc)
        got = y[:, :wn]
        eq = R.same_bits(got, want)
        if kind == R.CMN:
            assert eq, "%s: utterance %d (%d rows): %d elements differ from the restatement" % (
                what, u, x.shape[0], int((got.view(np.uint32) != want.view(np.uint32)).sum()))
        else:
            B = R.bound(x[:, :wn], m64, mu64)
            err = np.abs(got.astype(np.float64) - y64)
            assert np.isfinite(got).all(), "%s: utterance %d: non-finite rows" % (what, u)
            bad = np.argwhere(~(err <= B))
            assert bad.size == 0, "%s: utterance %d: |y - y64| > B at %d elements, first (row, column) %s: err %.3g, B %.3g" % (
                what, u, len(bad), tuple(bad[0]), err[tuple(bad[0])], B[tuple(bad[0])])
            with np.errstate(invalid="ignore", divide="ignore"):
                worst = max(worst, float(np.nanmax(np.where(B > 0, err / B, 0.0))))
            bits = bits and eq
        if not nad and dyn > 0:                               # the deltas of the normalised statics, on the handle's own rows
            assert_tail_consistent(y, cols, dyn, kw["delta_l1"], kw["delta_l2"], "%s, utt %d (deltas of normalised statics)" % (what, u))
        n += x.shape[0]
    assert n > 0
    if kind == R.CVN:
        print("%s: worst err / B %.3g over %d rows; the restatement's bits: %s" % (what, worst, n, bits))
    return worst


# ---- 1. the batch attachment against the restatement -----------------------------------------------------------------

@pytest.mark.parametrize("nad", (True, False), ids=("after", "before"))
@pytest.mark.parametrize("kind", (R.CMN, R.CVN), ids=("cmn", "cvn"))
@pytest.mark.parametrize("name", sorted(OD.CONFIGS))
def test_batch_rows_against_the_restatement(pkg, name, kind, nad):
    kw = OD.CONFIGS[name]
    xs = twin_rows(pkg, name)
    assert [x.shape[0] for x in xs] == FRAMES + [40]
    wn = OD.cols_of(kw) * ((1 + kw["dyn"]) if nad else 1)
    pc, pa = prior_for(wn)
    m = OD.make(pkg, kw, norm=kind, nad=nad)
    try:
        for N, F, p, acc in ((32, 0, 0, None), (96, 0, 0, None), (32, 64, pc, pa), (0, 200, pc, pa)):
            ys = OD.batch_rows(m, utts_of(name), setup=lambda h: h.batch_set_online_norm(N, F, None if acc is None else (p, acc)))
            check_rows(ys, xs, kw, kind, nad, N, F, p, acc, "%s %s %s N=%d F=%d" % (name, "cmn" if kind == 1 else "cvn",
                                                                                     "after" if nad else "before", N, F))
            assert m.debug_read(6).size == 0
    finally:
        m.close()


# ---- 2. what must not change the bits --------------------------------------------------------------------------------

_BASE = {}


def base_rows(pkg, N=32, kind=R.CVN, nad=True, name="c1", prior=False):
    """The batch rows of the online handle of a configuration: computed once, shared, never changed."""
    key = (name, N, kind, nad, prior)
    if key not in _BASE:
        kw = OD.CONFIGS[name]
        wn = OD.cols_of(kw) * ((1 + kw["dyn"]) if nad else 1)
        m = OD.make(pkg, kw, norm=kind, nad=nad)
        rows = OD.batch_rows(m, utts_of(name), setup=lambda h: h.batch_set_online_norm(N, 64 if prior else 0, prior_for(wn) if prior else None))
        m.close()
        for r in rows:
            r.setflags(write=False)
        _BASE[key] = rows
    return _BASE[key]


def test_an_utterances_bits_do_not_depend_on_the_rest_of_the_batch(pkg):
    base = base_rows(pkg)
    utts = utts_of("c1")
    m = OD.make(pkg, OD.CONFIGS["c1"], norm=R.CVN)
    try:
        order = list(range(len(utts)))[::-1]
        got = OD.batch_rows(m, [utts[u] for u in order], setup=lambda h: h.batch_set_online_norm(32))
        for k, u in enumerate(order):
            assert R.same_bits(got[k], base[u]), "reordered: utterance %d" % u
        for u in (len(utts) - 2, 7, 1):                      # 199 frames, 95 frames, 1 frame: each alone
            alone = OD.batch_rows(m, [utts[u]], setup=lambda h: h.batch_set_online_norm(32))
            assert R.same_bits(alone[0], base[u]), "alone: utterance %d" % u
    finally:
        m.close()


def test_stream_kernels_fused_delta_and_overlap_give_the_same_bits(pkg):
    """MFX_ENGINE_STREAM_KERNELS moves the batch to the streaming interface's front-end kernels, and with them the twin's rows
    v: the normaliser is the same function of them (CMN: the restatement's bits of THAT twin's rows).  The fused delta wave
    and the overlapped tail change no bit of the default build's rows."""
    base = base_rows(pkg)
    utts = utts_of("c1")
    kw = OD.CONFIGS["c1"]
    sk = pkg.mfcc.ENGINE_STREAM_KERNELS
    xs = twin_rows(pkg, "c1", "stream_kernels", engine=sk)
    for kind in (R.CMN, R.CVN):
        m = OD.make(pkg, kw, norm=kind, engine=sk)
        ys = OD.batch_rows(m, utts, setup=lambda h: h.batch_set_online_norm(32))
        m.close()
        check_rows(ys, xs, kw, kind, True, 32, what="c1 under MFX_ENGINE_STREAM_KERNELS, kind %d" % kind)
    m = OD.make(pkg, kw, norm=R.CVN, engine=pkg.mfcc.ENGINE_FUSE_DELTA)
    got = OD.batch_rows(m, utts, setup=lambda h: h.batch_set_online_norm(32))
    m.close()
    for u in range(len(utts)):
        assert R.same_bits(got[u], base[u]), "fused delta: utterance %d" % u
    m = OD.make(pkg, OD.CONFIGS["c1"], norm=R.CVN)
    try:
        offs, lens, pcm = OD.layout(utts)
        rows, _ = m.batch_plan(offs, lens)
        m.batch_set_online_norm(32)
        m.batch_overlap(True)
        for _ in range(3):                                   # both statics buffers re-used
            out = m.batch_run_host(pcm.reshape(-1))          # (ends with mfx_synchronize)
        for u in range(len(utts)):
            assert R.same_bits(out[rows[u]:rows[u] + base[u].shape[0]], base[u]), "overlap: utterance %d" % u
    finally:
        m.close()


def test_with_an_alpha_list(pkg):
    kw = OD.CONFIGS["c1"]
    n = len(utts_of("c1"))
    alphas = np.array([0.9, 1.1, 1.0] * n, np.float32)[:n]
    setup = lambda h: h.batch_set_alphas(alphas)
    xs = twin_rows(pkg, "c1", "alphas", setup=setup)
    assert not R.same_bits(xs[-3], twin_rows(pkg, "c1")[-3])  # the list did warp (utterance 10: 1.1)
    for kind in (R.CMN, R.CVN):
        m = OD.make(pkg, kw, norm=kind)
        ys = OD.batch_rows(m, utts_of("c1"), setup=lambda h: (h.batch_set_alphas(alphas), h.batch_set_online_norm(96)))
        m.close()
        check_rows(ys, xs, kw, kind, True, 96, what="c1 with an alpha list, kind %d" % kind)


def test_the_transform_and_the_vad_read_the_normalised_rows(pkg):
    base = base_rows(pkg)
    utts = utts_of("c1")
    ycat = np.concatenate(base)
    frames = [b.shape[0] for b in base]
    rows = np.concatenate([[0], np.cumsum(frames)[:-1]])
    m = OD.make(pkg, OD.CONFIGS["c1"], norm=R.CVN)
    try:
        eye = np.eye(39, dtype=np.float32)
        got = OD.batch_rows(m, utts, setup=lambda h: (h.batch_set_online_norm(32), h.batch_set_transform(eye)))
        assert np.array_equal(np.concatenate(got), ycat), "identity transform: values differ from the normalised rows"
        # the VAD on column 12 of the normalised rows: the threshold within its bound, the flags an exact function of both
        et, ms, ctx, prop = 0.1, 0.5, 2, 0.6
        got = OD.batch_rows(m, utts, setup=lambda h: (h.batch_set_online_norm(32), h.batch_set_vad(12, et, ms, ctx, prop, pkg.mfcc.VAD_SELECT)))
        flags, voiced, thr, total = m.batch_vad_read()
        for u, (r0, T) in enumerate(zip(rows, frames)):
            want_thr, b = vad_ref.thr_ref(base[u][:, 12], et, ms)
            assert abs(float(thr[u]) - want_thr) <= b, (u, thr[u], want_thr, b)
            assert np.array_equal(flags[r0:r0 + T], vad_ref.flags_ref(base[u][:, 12], thr[u], ctx, prop)), u
        assert 0 < total < len(ycat)
        assert R.same_bits(np.concatenate(got), vad_ref.select_ref(ycat, rows, frames, flags))
    finally:
        m.close()


def test_a_sliced_host_run_equals_the_device_entry(pkg):
    """8 utterances, 32 MB of PCM, ascending offsets, pinned buffers: mfx_batch_run_host takes its sliced path (utterances
    are independent under the online normaliser) and gives the device entry's bits."""
    import torch
    from conftest import synth_utterance
    L = pkg.load_library()
    L.mfx_alloc_pinned.restype, L.mfx_alloc_pinned.argtypes = C.c_void_p, [C.c_size_t]
    L.mfx_free_pinned.restype, L.mfx_free_pinned.argtypes = None, [C.c_void_p]
    one = synth_utterance(2100000, 123)
    n_utt = 8
    offs = [u * one.size for u in range(n_utt)]
    lens = [one.size - 160 * u for u in range(n_utt)]
    pos = n_utt * one.size
    assert pos * 2 >= 32 << 20
    m = OD.make(pkg, OD.CONFIGS["c1"], norm=R.CVN)
    rows, total = m.batch_plan(offs, lens)
    m.batch_set_online_norm(96)
    p_in, p_out = L.mfx_alloc_pinned(pos * 2), L.mfx_alloc_pinned(total * 39 * 4)
    assert p_in and p_out
    try:
        for u in range(n_utt):
            C.memmove(p_in + 2 * offs[u], one.ctypes.data, one.size * 2)
        rc = L.mfx_batch_run_host(m._h, C.cast(p_in, C.POINTER(C.c_int16)), pos, C.cast(p_out, C.POINTER(C.c_float)))
        assert rc == 0, L.mfx_last_error(m._h)
        got = np.ctypeslib.as_array(C.cast(p_out, C.POINTER(C.c_float)), shape=(total, 39)).copy()
        pcm = torch.from_numpy(np.ctypeslib.as_array(C.cast(p_in, C.POINTER(C.c_int16)), shape=(pos,)).copy()).to("cuda:0")
    finally:
        L.mfx_free_pinned(p_in)
        L.mfx_free_pinned(p_out)
    out = torch.full((total, 39), float("nan"), dtype=torch.float32, device="cuda:0")
    m.batch_run_device(pcm.data_ptr(), pcm.numel(), out.data_ptr())
    m.synchronize()
    m.close()
    assert R.same_bits(out.cpu().numpy(), got) and np.isfinite(got).all()
    # utterance 1 is utterance 0 cut one hop short: a causal normaliser gives both the same rows up to the deltas' reach
    T1 = int(rows[2] - rows[1]) - 6
    assert T1 > 13000 and R.same_bits(got[rows[0]:rows[0] + T1], got[rows[1]:rows[1] + T1])


@pytest.mark.parametrize("k", (1, 3))
def test_d_out_at_an_odd_offset_inside_a_larger_allocation(pkg, k):
    import torch
    base = base_rows(pkg, N=32, kind=R.CVN, nad=False)
    utts = utts_of("c1")
    offs, lens, pcm = OD.layout(utts)
    m = OD.make(pkg, OD.CONFIGS["c1"], norm=R.CVN, nad=False)
    try:
        _, total = m.batch_plan(offs, lens)
        m.batch_set_online_norm(32)
        d_pcm = torch.from_numpy(pcm.reshape(-1).copy()).to("cuda:0")
        op = OutPlacement(total, 39, k=k)
        m.batch_run_device(d_pcm.data_ptr(), len(pcm), op.ptr)
        m.synchronize()
        got = op.check("batch, d_out %d floats past a 16-byte boundary" % k).cpu().numpy()
        assert R.same_bits(got, np.concatenate(base))
    finally:
        m.close()


# ---- 3. sessions against the batch rows ------------------------------------------------------------------------------

SESS = {   # N, kind, after the deltas, with a prior
    "n32_cvn_before_prior": (32, R.CVN, False, True),
    "n96_cmn_after": (96, R.CMN, True, False),
    "n0_cmn_after": (0, R.CMN, True, False),
    "n32_cmn_after": (32, R.CMN, True, False),
    "n0_cvn_after_prior": (0, R.CVN, True, True),
    "n96_cvn_before": (96, R.CVN, False, False),
    "n32_cvn_after": (32, R.CVN, True, False),
}
SESS_CASES = [(s, p) for s in ("n32_cvn_before_prior", "n96_cmn_after") for p in sorted(OD.PATTERNS)] + \
             [(s, "random_empty_and_flush") for s in sorted(SESS) if s not in ("n32_cvn_before_prior", "n96_cmn_after")]


def session_handle(pkg, name, N, kind, nad, prior, n_sessions, max_push):
    kw = OD.CONFIGS[name]
    wn = OD.cols_of(kw) * ((1 + kw["dyn"]) if nad else 1)
    m = OD.make(pkg, kw, norm=kind, nad=nad)
    m.sessions_set_online_norm(N, 64 if prior else 0, prior_for(wn) if prior else None)
    m.sessions_create(n_sessions, max_push)
    return m


@pytest.mark.parametrize("setting,pattern", SESS_CASES)
def test_session_rows_are_the_batch_rows(pkg, setting, pattern):
    N, kind, nad, prior = SESS[setting]
    want = base_rows(pkg, N, kind, nad, prior=prior)
    p = dict(OD.PATTERNS[pattern])
    n_sessions = p.pop("n_sessions")
    m = session_handle(pkg, "c1", N, kind, nad, prior, n_sessions, p.pop("max_push", OD.MAX_PUSH))
    try:
        got = OD.drive(m, utts_of("c1"), n_sessions, seed=11, odd_offsets=(pattern == "ids_reused"), **p)
        OD.compare("c1", got, want, "%s, %s" % (setting, pattern))
    finally:
        m.close()


def test_session_rows_stereo_120_columns_host_entry_and_placement(pkg):
    want = base_rows(pkg, 32, R.CVN, True, name="stereo44k")
    m = session_handle(pkg, "stereo44k", 32, R.CVN, True, False, 7, OD.MAX_PUSH)
    try:
        got = OD.drive(m, utts_of("stereo44k"), 7, OD.cut_random_with_empty, seed=5, odd_offsets=True,
                       place=lambda total, width: OutPlacement(total, width, k=3))
        OD.compare("stereo44k", got, want, "random, d_out 3 floats past a 16-byte boundary")
        got = OD.drive(m, utts_of("stereo44k"), 7, OD.cut_random, seed=6, host=True)
        OD.compare("stereo44k", got, want, "run_host")
    finally:
        m.close()


def test_reset_in_mid_stream_then_a_fresh_utterance_on_the_same_id(pkg):
    want = base_rows(pkg, 32, R.CVN, True)
    utts = utts_of("c1")
    a, b = len(utts) - 2, len(utts) - 3                       # 199 and 133 frames
    m = session_handle(pkg, "c1", 32, R.CVN, True, False, 4, 33000)
    try:
        rows, counts, total = m.sessions_plan([2], [0], [12000])
        part = m.sessions_run_host(np.concatenate([utts[a][:12000].reshape(-1), np.zeros(2, np.int16)]))
        assert total == m.batch_frames(12000) - 6 > 64 and R.same_bits(part, want[a][:total])
        m.sessions_reset(2)
        assert m.sessions_delivered(2) == 0
        _, _, total = m.sessions_plan([2], [0], [len(utts[b])], [1])
        out = m.sessions_run_host(np.concatenate([utts[b].reshape(-1), np.zeros(2, np.int16)]))
        assert total == len(want[b]) and R.same_bits(out, want[b])
    finally:
        m.close()


# ---- 4. state rules --------------------------------------------------------------------------------------------------

def status_of(fn, *args, **kw):
    try:
        fn(*args, **kw)
        return 0
    except Exception as e:                                   # MfxError (the package is loaded under an alias)
        return e.status


def test_state_rules(pkg):
    ARG, STATE, CONFIG = -7, -8, -5
    kw = OD.CONFIGS["c1"]
    utts = utts_of("c1")
    offs, lens, pcm = OD.layout(utts)
    pcm = pcm.reshape(-1)
    for norm in (0, 3):                                      # NONE and MINMAX: refused, batch and sessions
        h = OD.make(pkg, kw, norm=norm)
        h.batch_plan(offs, lens)
        assert status_of(h.batch_set_online_norm, 32) == CONFIG
        assert status_of(h.sessions_set_online_norm, 32) == CONFIG
        h.close()

    ref = OD.make(pkg, kw, norm=R.CVN)
    never = np.concatenate(OD.batch_rows(ref, utts))         # a handle that never had the attachment
    ref.close()

    m = OD.make(pkg, kw, norm=R.CVN)
    try:
        assert status_of(m.batch_set_online_norm, 32) == STATE               # before a plan
        m.batch_plan(offs, lens)
        acc = np.zeros((2, 39))
        L, dp = m._L, C.POINTER(C.c_double)
        for bad in ((-32, 0, 0, None), (16, 0, 0, None), (48, 0, 0, None), (4128, 0, 0, None), (32, -1, 0, None),
                    (32, (1 << 20) + 1, 0, None), (32, 0, -1, None), (32, 64, 5, None), (32, 64, 0, acc)):
            a = None if bad[3] is None else bad[3].ctypes.data_as(dp)
            assert L.mfx_batch_set_online_norm(m._h, bad[0], bad[1], bad[2], a) == ARG, bad
            assert L.mfx_sessions_set_online_norm(m._h, bad[0], bad[1], bad[2], a) == ARG, bad
        assert R.same_bits(m.batch_run_host(pcm), never)     # every refusal left the handle on the per-utterance normaliser
        # a speaker list and the attachment exclude each other
        ids = np.arange(len(utts), dtype=np.int32) % 3
        m.batch_set_speakers(ids, 3)
        assert status_of(m.batch_set_online_norm, 32) == STATE
        m.batch_set_speakers(None)
        m.batch_set_online_norm(32)
        assert status_of(m.batch_set_speakers, ids, 3) == STATE
        with_on = m.batch_run_host(pcm)
        assert R.same_bits(with_on, np.concatenate(base_rows(pkg))) and not R.same_bits(with_on, never)
        assert m.debug_read(6).size == 0
        # clear: back on the per-utterance normaliser's bits; a new plan drops it too
        m.batch_clear_online_norm()
        assert R.same_bits(m.batch_run_host(pcm), never) and m.debug_read(6).size == 3 * len(utts) * 2 * 13
        m.batch_set_online_norm(32)
        m.batch_plan(offs, lens)
        assert R.same_bits(m.batch_run_host(pcm), never)
        m.batch_set_speakers(ids, 3)                         # (and the list is welcome again)
        m.batch_set_speakers(None)
        # sessions: a CMN / CVN handle without the setter fails as it always did
        assert status_of(m.sessions_create, 2, 1600) == STATE
        assert "session entries do not serve" in L.mfx_last_error(m._h).decode()
        m.sessions_set_online_norm(32)
        m.sessions_create(2, 1600)
        assert status_of(m.sessions_set_online_norm, 96) == STATE            # live sessions
        assert status_of(m.sessions_clear_online_norm) == STATE
        m.sessions_create(0, 0)
        m.sessions_set_online_norm(96)
        m.sessions_clear_online_norm()
        assert status_of(m.sessions_create, 2, 1600) == STATE
    finally:
        m.close()
    t = OD.make(pkg, OD.CONFIGS["traps150"], norm=R.CMN)     # TRAPS handles stay refused by the session entries
    try:
        t.sessions_set_online_norm(32)
        assert status_of(t.sessions_create, 2, 1600) == STATE
    finally:
        t.close()


# ---- 5. the driver ---------------------------------------------------------------------------------------------------

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


def test_driver_online_window_equals_the_binding(pkg, a0001, tmp_path):
    exe = exe_path()
    pcms = [a0001, a0001[500:100500].copy(), a0001[1000:81000].copy()]
    args = []
    for i, p in enumerate(pcms):
        write_wav(tmp_path / ("in%d.wav" % i), p)
        args += [str(tmp_path / ("in%d.wav" % i)), str(tmp_path / ("out%d.htk" % i))]
    opts = ["--banks", "40", "--ceps", "13", "--c0", "0", "--norm", "2", "--dyn", "2", "--htk", "--batch-mb", "4"]
    subprocess.check_call([exe] + opts + ["--online-window", "96"] + args, stdout=subprocess.DEVNULL)
    m = pkg.MfccHip(10000000, 400, 160, 40, 16000.0, 64.0, 8000.0, 13, False, 22.0, pkg.NORM_CVN, pkg.DYN_ACC, 3, 3, True, device=0,
                    engine=pkg.mfcc.ENGINE_STREAM_KERNELS)
    m.set_window(pkg.reference_window(400))
    utts = [p.reshape(-1, 1) for p in pcms]
    want = OD.batch_rows(m, utts, setup=lambda h: h.batch_set_online_norm(96))
    per_utt = OD.batch_rows(m, utts)
    m.close()
    for i in range(len(pcms)):
        got = read_htk(tmp_path / ("out%d.htk" % i))
        assert got.shape == want[i].shape and R.same_bits(got, want[i]), "file %d" % i
        assert not R.same_bits(got, per_utt[i])              # (not the per-utterance normaliser's rows)
    spk = tmp_path / "spk.txt"
    spk.write_text("a\nb\na\n")
    for extra, word in ((["--online-window", "96", "--spk-file", str(spk)], "--spk-file"), (["--online-window", "40"], "multiple of 32"),
                        (["--online-window", "96", "--norm", "3"], "--norm 1 or 2"), (["--online-window", "96", "--batch-mb", "0"], "--batch-mb")):
        r = subprocess.run([exe] + opts + extra + args, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True)
        assert r.returncode != 0 and word in r.stderr, (extra, r.stderr)
