"""Splice + affine transform as the last stage of the batch entries (mfx_batch_set_transform; k_splice_affine) on the MI355X.

The rows y the stage reads are those of a TWIN handle without a transform on the same PCM and plan, so only the new
kernel is under test.  Three kinds of check:
  - exact: an identity placed on one splice slot must return the twin's (clamped) rows bit for bit;
  - bound: every output within Higham's bound of the float64 map of the twin's rows (xform_ref.py: derived, not tuned);
  - bits: the matrix-pipe and the vector form, a second run, the device entry, every utterance alone, the overlap mode
    and the sliced host path must all deliver the same bits.
All shapes 16 kHz, W = 400, S = 160, 512-point FFT."""
import ctypes as C

import numpy as np
import pytest

import xform_ref as XR
from conftest import synth_utterance

pytestmark = pytest.mark.gpu

XFORM_VALU = 1024
W, S, SR = 400, 160, 16000.0
# edge clamps on both sides inside one tile, a frameless utterance, the tile boundaries, more than one tile
FRAMES = [1, 2, 3, 0, 63, 64, 65, 145]

CONFIGS = {
    "mfcc39": dict(nb=40, nc=13, dyn=2, norm=2),                   # 13 + d + dd, CVN after the deltas: normalised rows
    "mfcc13": dict(nb=40, nc=13, dyn=0, norm=0),
    "traps150": dict(nb=15, nc=0, dyn=0, norm=0, method="traps", traps_len=31, traps_dct_len=10),
    "fbank128": dict(nb=64, nc=0, dyn=1, norm=0),                  # 64 log mel energies + d: width 128
}


def make(pkg, name, engine=0, ibs=200000):
    kw = dict(CONFIGS[name])
    method = {"traps": pkg.METHOD_TRAPS}.get(kw.pop("method", None), pkg.METHOD_MFCC)
    m = pkg.MfccHip(ibs, W, S, kw["nb"], SR, 64.0, SR / 2, kw["nc"], False, 22.0, kw["norm"], kw["dyn"], 3, 3, True,
                    device=0, bug_compat=False, engine=engine, method=method,
                    traps_len=kw.get("traps_len", 0), traps_dct_len=kw.get("traps_dct_len", 0))
    m.set_window(pkg.reference_window(W))
    return m


_RAGGED = {}


def ragged():
    """The ragged batch (computed once, never modified): utterances, even offsets, lengths, PCM."""
    if not _RAGGED:
        lens = [300 if T == 0 else (T - 1) * S + W + 7 * (i % 3) for i, T in enumerate(FRAMES)]
        utts = [synth_utterance(n, 70 + i) for i, n in enumerate(lens)]
        offs, pos = [], 0
        for n in lens:
            offs.append(pos)
            pos += n + (n & 1) + 2 * (len(offs) % 2)
        pcm = np.zeros(pos + 8, np.int16)
        for o_, u in zip(offs, utts):
            pcm[o_:o_ + u.size] = u
        for a in (pcm, *utts):
            a.setflags(write=False)
        _RAGGED.update(lens=lens, utts=utts, offs=offs, pcm=pcm)
    return _RAGGED


_TWIN = {}


def twin_rows(pkg, name):
    """(rows, y): the ragged batch through a handle WITHOUT a transform (computed once per configuration)."""
    if name not in _TWIN:
        d = ragged()
        t = make(pkg, name)
        rows, total = t.batch_plan(d["offs"], d["lens"])
        assert [t.batch_frames(n) for n in d["lens"]] == FRAMES and total == sum(FRAMES)
        y = t.batch_run_host(d["pcm"])
        t.close()
        y.setflags(write=False)
        _TWIN[name] = (rows, y)
    return _TWIN[name]


def matrices(seed, n_xf, out_dim, in_dim, bias=True):
    """Seeded transforms with entries of both signs, scaled like a decorrelating map (rows of norm ~1)."""
    rng = np.random.default_rng(seed)
    A = (rng.standard_normal((n_xf, out_dim, in_dim)) / np.sqrt(in_dim)).astype(np.float32)
    b = rng.standard_normal((n_xf, out_dim)).astype(np.float32) if bias else None
    return A, b


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def same_values(a, b):
    """same_bits, except that a NaN may carry another payload: the matrix pipe and the vector ALUs each pass on a NaN of
    the twin's rows (a one-frame utterance under CVN is 0 x inf there) in their own way."""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())


def planned(pkg, name, engine=0):
    d = ragged()
    m = make(pkg, name, engine=engine)
    rows, total = m.batch_plan(d["offs"], d["lens"])
    return m, rows, total


# ---- 1. exact selection ----------------------------------------------------------------------------------------------

def test_identity_on_a_splice_slot_returns_the_twins_rows(pkg):
    d = ragged()
    rows, y = twin_rows(pkg, "mfcc13")
    assert y.shape[1] == 13 and np.isfinite(y).all()
    m, rows_m, total = planned(pkg, "mfcc13")
    assert list(rows_m) == list(rows)
    for j in range(4):                                           # left = 2, right = 1: slot j is frame t + j - 2
        A = np.zeros((13, 4 * 13), np.float32)
        A[np.arange(13), 13 * j + np.arange(13)] = 1.0
        m.batch_set_transform(A, None, left=2, right=1)
        assert m.batch_output_width() == 13
        got = m.batch_run_host(d["pcm"])
        assert got.shape == (total, 13)
        for u, (r0, T) in enumerate(zip(rows, FRAMES)):
            if T:
                want = y[r0 + np.clip(np.arange(T) + j - 2, 0, T - 1)]
                assert same_bits(got[r0:r0 + T], want), "slot %d, utterance %d (%d frames)" % (j, u, T)
    m.close()


# ---- 2. bound against the float64 oracle -----------------------------------------------------------------------------

BOUND_CASES = [
    # (id, configuration, left, right, out_dim, rows per block the launcher must take)
    ("mfcc39-4-4-o40", "mfcc39", 4, 4, 40, 64),          # the C2 stage: in_dim 351, not a multiple of 4
    ("mfcc39-0-0-o1", "mfcc39", 0, 0, 1, 64),
    ("mfcc39-0-0-o15", "mfcc39", 0, 0, 15, 64),
    ("mfcc39-0-0-o16", "mfcc39", 0, 0, 16, 64),
    ("mfcc39-0-0-o17", "mfcc39", 0, 0, 17, 64),
    ("traps150-1-1-o40", "traps150", 1, 1, 40, 32),      # in_dim 450
    # in_dim at the limit: width 128 (64 log mel energies + d) x 64 frames (left 32, right 31) = 8192 exactly
    ("fbank128-32-31-o16", "fbank128", 32, 31, 16, 64),
    ("mfcc39-0-0-o256", "mfcc39", 0, 0, 256, 16),        # out_dim at the limit
    # the remaining tile / accumulator paths: 32 rows per block; 8 and 16 accumulator tiles per wave
    ("mfcc39-4-4-o128", "mfcc39", 4, 4, 128, 32),
    ("mfcc39-0-0-o144", "mfcc39", 0, 0, 144, 32),
    ("fbank128-32-31-o256", "fbank128", 32, 31, 256, 64),
]


@pytest.mark.parametrize("case", BOUND_CASES, ids=[c[0] for c in BOUND_CASES])
def test_every_value_within_its_bound_of_the_float64_map(pkg, case):
    what, name, left, right, out_dim, tile = case
    d = ragged()
    rows, y = twin_rows(pkg, name)
    width = y.shape[1]
    in_dim = (left + right + 1) * width
    assert in_dim <= 8192
    # known to launch, and on the path the case is there for (the launcher's rule, restated in xform_ref)
    assert XR.tile_rows(width, left, right, out_dim) == tile
    assert XR.lds_bytes(tile, width, left, right, out_dim) <= 160 * 1024
    A, b = matrices(len(what), 1, out_dim, in_dim)
    m, rows_m, total = planned(pkg, name)
    m.batch_set_transform(A[0], b[0], left=left, right=right)
    assert m.batch_output_width() == out_dim and m.get_output_data_width() == width
    got = m.batch_run_host(d["pcm"])
    assert got.shape == (total, out_dim)
    worst = XR.assert_xform_consistent(got, y, rows, FRAMES, A, b, left, right, what=what)
    assert worst > 0.0                                           # (the outputs are not trivially exact: something was compared)
    m.close()


# ---- 3. same bits across forms and runs ------------------------------------------------------------------------------

def c2_stage(pkg, engine=0):
    d = ragged()
    rows, y = twin_rows(pkg, "mfcc39")
    A, b = matrices(5, 1, 40, 9 * 39)
    m, _, total = planned(pkg, "mfcc39", engine=engine)
    m.batch_set_transform(A[0], b[0], left=4, right=4)
    return d, rows, m, total, A, b


def test_vector_form_second_run_and_device_entry_give_the_same_bits(pkg):
    import torch
    d, rows, m, total, A, b = c2_stage(pkg)
    got = m.batch_run_host(d["pcm"])
    assert same_bits(m.batch_run_host(d["pcm"]), got)           # a second run
    v = make(pkg, "mfcc39", engine=XFORM_VALU)
    v.batch_plan(d["offs"], d["lens"])
    v.batch_set_transform(A[0], b[0], left=4, right=4)
    vec = v.batch_run_host(d["pcm"])
    assert same_values(vec, got), "vector form differs from the matrix form"
    assert np.isfinite(got[rows[4]:]).all() and same_bits(vec[rows[4]:], got[rows[4]:])
    v.close()
    dev = torch.device("cuda:0")
    pcm = torch.from_numpy(d["pcm"].copy()).to(dev)
    out = torch.full((total, 40), float("nan"), dtype=torch.float32, device=dev)
    m.batch_run_device(pcm.data_ptr(), pcm.numel(), out.data_ptr())
    m.synchronize()
    assert same_bits(out.cpu().numpy(), got), "device entry differs from the host entry"
    m.close()


def test_every_utterance_alone_gives_its_rows_of_the_batch(pkg):
    d, rows, m, total, A, b = c2_stage(pkg)
    got = m.batch_run_host(d["pcm"])
    m.close()
    one = make(pkg, "mfcc39")
    for u, (r0, T) in enumerate(zip(rows, FRAMES)):
        one.batch_plan([d["offs"][u]], [d["lens"][u]])
        one.batch_set_transform(A[0], b[0], left=4, right=4)    # (a plan clears the transform)
        alone = one.batch_run_host(d["pcm"])
        assert alone.shape == (T, 40)
        assert same_bits(alone, got[r0:r0 + T]), "utterance %d (%d frames)" % (u, T)
    one.close()


def test_overlap_mode_gives_the_same_bits(pkg):
    import torch
    d, rows, m, total, A, b = c2_stage(pkg)
    got = m.batch_run_host(d["pcm"])
    m.batch_overlap(True)
    assert m.batch_output_width() == 40
    dev = torch.device("cuda:0")
    pcm = torch.from_numpy(d["pcm"].copy()).to(dev)
    outs = [torch.full((total, 40), float("nan"), dtype=torch.float32, device=dev) for _ in range(3)]
    for o in outs:                                               # three batches in flight: both scratch buffers re-used
        m.batch_run_device(pcm.data_ptr(), pcm.numel(), o.data_ptr())
    m.synchronize()
    for i, o in enumerate(outs):
        assert same_bits(o.cpu().numpy(), got), "overlapped batch %d" % i
    assert same_bits(m.batch_run_host(d["pcm"]), got)
    m.close()


def test_sliced_host_run_with_pinned_buffers_gives_the_same_bits(pkg):
    """The smallest batch that takes the sliced path of mfx_batch_run_host: 8 utterances (two slices), 32 MB of PCM, pinned
    buffers.  Against the same handle's run from pageable buffers (one piece) and, on sampled utterances, the oracle."""
    L = pkg.load_library()
    L.mfx_alloc_pinned.restype, L.mfx_alloc_pinned.argtypes = C.c_void_p, [C.c_size_t]
    L.mfx_free_pinned.restype, L.mfx_free_pinned.argtypes = None, [C.c_void_p]
    rng = np.random.default_rng(21)
    n_utt = 8
    lens = [int(v) for v in rng.integers(2100000, 2110000, size=n_utt)]
    offs, pos = [], 0
    for n in lens:
        offs.append(pos)
        pos += n + int(rng.integers(0, 5))
    assert pos * 2 >= 32 << 20
    pcm = (3000.0 * rng.standard_normal(pos)).astype(np.int16)
    A, b = matrices(6, 2, 40, 9 * 39)
    utt_xf = np.arange(n_utt, dtype=np.int32) % 2
    m = make(pkg, "mfcc39")
    rows, total = m.batch_plan(offs, lens)
    m.batch_set_transform(A, b, left=4, right=4, utt_xf=utt_xf)
    width = m.batch_output_width()
    assert width == 40
    p_in, p_out = L.mfx_alloc_pinned(pos * 2), L.mfx_alloc_pinned(total * width * 4)
    assert p_in and p_out
    try:
        C.memmove(p_in, pcm.ctypes.data, pos * 2)
        rc = L.mfx_batch_run_host(m._h, C.cast(p_in, C.POINTER(C.c_int16)), pos, C.cast(p_out, C.POINTER(C.c_float)))
        assert rc == 0, L.mfx_last_error(m._h)
        got = np.ctypeslib.as_array(C.cast(p_out, C.POINTER(C.c_float)), shape=(total, width)).copy()
    finally:
        L.mfx_free_pinned(p_in)
        L.mfx_free_pinned(p_out)
    assert same_bits(m.batch_run_host(pcm), got)                 # pageable buffers: the whole batch in one piece
    m.close()
    t = make(pkg, "mfcc39")
    t.batch_plan(offs, lens)
    y = t.batch_run_host(pcm)
    t.close()
    sample = [0, 3, 4, 7]                                        # both slices, both transforms
    frames = [(n - W) // S + 1 for n in lens]
    XR.assert_xform_consistent(got, y, [rows[u] for u in sample], [frames[u] for u in sample], A, b, 4, 4,
                               utt_xf=[utt_xf[u] for u in sample], what="sliced")


# ---- 4. per-utterance transforms -------------------------------------------------------------------------------------

UTT_XF = np.array([0, 1, 2, 1, 0, 2, 1, 0], np.int32)           # (utterance 3 has no frame)


@pytest.mark.parametrize("with_alphas", [False, True], ids=["plain", "alphas"])
def test_each_utterance_equals_a_run_alone_with_its_matrix_as_transform_0(pkg, with_alphas):
    d = ragged()
    A, b = matrices(9, 3, 40, 9 * 39)
    alphas = np.array([1.0, 0.9, 1.1, 1.0, 0.9, 0.9, 1.1, 1.0], np.float32)
    m, rows, total = planned(pkg, "mfcc39")
    if with_alphas:
        m.batch_set_alphas(alphas)
    m.batch_set_transform(A, b, left=4, right=4, utt_xf=UTT_XF)
    got = m.batch_run_host(d["pcm"])
    assert got.shape == (total, 40)
    m.close()
    one = make(pkg, "mfcc39")
    for u, (r0, T) in enumerate(zip(rows, FRAMES)):
        one.batch_plan([d["offs"][u]], [d["lens"][u]])
        if with_alphas:
            one.batch_set_alphas(alphas[u:u + 1])
        one.batch_set_transform(A[UTT_XF[u]], b[UTT_XF[u]], left=4, right=4)
        alone = one.batch_run_host(d["pcm"])
        assert same_bits(alone, got[r0:r0 + T]), "utterance %d (%d frames, transform %d)" % (u, T, UTT_XF[u])
    one.close()
    # the transforms matter: utterance 7 (transform 0) differs from the same rows under transform 1
    other = make(pkg, "mfcc39")
    other.batch_plan(d["offs"], d["lens"])
    if with_alphas:
        other.batch_set_alphas(alphas)
    other.batch_set_transform(A[1], b[1], left=4, right=4)
    o1 = other.batch_run_host(d["pcm"])
    other.close()
    assert not same_bits(o1[rows[7]:], got[rows[7]:]) and same_bits(o1[rows[6]:rows[7]], got[rows[6]:rows[7]])


# ---- 5. clearing -----------------------------------------------------------------------------------------------------

def test_clearing_and_replanning_restore_the_twins_bits_and_width(pkg):
    d = ragged()
    rows, y = twin_rows(pkg, "mfcc39")
    A, b = matrices(3, 1, 40, 9 * 39)
    m, _, total = planned(pkg, "mfcc39")
    fresh = make(pkg, "mfcc39")
    assert m.batch_output_width() == 39
    m.batch_set_transform(A[0], b[0], left=4, right=4)
    assert m.batch_output_width() == 40 and m.get_output_data_width() == 39
    name = m.dominant_kernel_name()
    assert name == fresh.dominant_kernel_name()                  # still names the front end
    with_xf = m.batch_run_host(d["pcm"])
    assert with_xf.shape == (total, 40)
    # streaming calls on the same handle are unaffected while the transform is in force
    pcm = synth_utterance(30000, 9)
    streamed = []
    for e in (m, fresh):
        n = e.set_input(pcm)
        e.apply()
        streamed.append(e.get_output_data(n))
    assert streamed[0].shape[1] == 39 and same_bits(streamed[0], streamed[1])
    assert same_bits(m.batch_run_host(d["pcm"]), with_xf)
    # clearing
    m.batch_set_transform(None)
    assert m.batch_output_width() == 39
    assert same_bits(m.batch_run_host(d["pcm"]), y)
    # a new plan clears it too
    m.batch_set_transform(A[0], b[0], left=4, right=4)
    assert m.batch_output_width() == 40
    m.batch_plan(d["offs"], d["lens"])
    assert m.batch_output_width() == 39
    assert same_bits(m.batch_run_host(d["pcm"]), y)
    for e in (m, fresh):
        e.close()


# ---- 6. errors -------------------------------------------------------------------------------------------------------

def status_of(fn, *args, **kw):
    try:
        fn(*args, **kw)
    except Exception as e:      # MfxError
        return getattr(e, "status", None)
    return 0


def raw_set(m, left, right, out_dim, n_xf, A, b=None, utt_xf=None, n_utt=0):
    fpt, ipt = C.POINTER(C.c_float), C.POINTER(C.c_int32)
    return m._L.mfx_batch_set_transform(m._h, left, right, out_dim, n_xf, None if A is None else A.ctypes.data_as(fpt),
                                        None if b is None else b.ctypes.data_as(fpt),
                                        None if utt_xf is None else utt_xf.ctypes.data_as(ipt), n_utt)


def test_refused_calls_leave_the_handle_usable(pkg):
    d = ragged()
    rows, y = twin_rows(pkg, "mfcc39")
    m = make(pkg, "mfcc39")
    big = np.zeros(1024 * 256 * 39 + 64, np.float32)             # (large enough for every shape tried below)
    assert raw_set(m, 0, 0, 8, 1, big) == -8                     # MFX_ERR_STATE: no plan yet
    m.batch_plan(d["offs"], d["lens"])
    ok = np.zeros(len(FRAMES), np.int32)
    for args in [(-1, 0, 8, 1), (33, 0, 8, 1), (0, -1, 8, 1), (0, 33, 8, 1),          # left / right outside 0 .. 32
                 (0, 0, 0, 1), (0, 0, 257, 1), (0, 0, 8, 0), (0, 0, 8, 1025),          # out_dim, n_xf
                 (32, 32, 8, 1)]:                                                       # in_dim = 65 * 39 is fine ...
        want = 0 if args == (32, 32, 8, 1) else -7
        assert raw_set(m, *args, big) == want, args
    m.batch_set_transform(None)
    w128 = make(pkg, "fbank128")
    w128.batch_plan(d["offs"], d["lens"])
    assert raw_set(w128, 32, 32, 8, 1, big) == -7                # ... and 65 * 128 > 8192 is not
    assert raw_set(w128, 32, 31, 8, 1, big) == 0
    w128.close()
    assert raw_set(m, 0, 0, 8, 2, big, None, ok[:-1], len(FRAMES) - 1) == -7          # not the planned count
    bad = ok.copy()
    bad[3] = 2
    assert raw_set(m, 0, 0, 8, 2, big, None, bad, len(FRAMES)) == -7                  # an index outside [0, n_xf)
    bad[3] = -1
    assert raw_set(m, 0, 0, 8, 2, big, None, bad, len(FRAMES)) == -7
    assert raw_set(m, 0, 0, 8, 1, None) == -7                    # no matrix (and not the clearing form)
    assert m.batch_output_width() == 39                          # a refused call changes nothing
    assert same_bits(m.batch_run_host(d["pcm"]), y)
    A, b = matrices(4, 1, 40, 9 * 39)
    m.batch_set_transform(A[0], b[0], left=4, right=4)
    assert raw_set(m, 0, 0, 0, 1, big) == -7 and m.batch_output_width() == 40         # ... nor does it end one in force
    got = m.batch_run_host(d["pcm"])
    XR.assert_xform_consistent(got, y, rows, FRAMES, A, b, 4, 4, what="after refused calls")
    m.close()
