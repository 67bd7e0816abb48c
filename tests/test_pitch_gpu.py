"""Pitch track of the batch entries (mfx_batch_set_pitch; mfx_pitch.hip: k_pitch_nccf, k_pitch_track) on the MI355X.

The definition of include/mfx.h is exact, so the device is held to the host restatement mfx_host_pitch bit for bit -- rho,
lag, rho at the path, index -- on every shape of pitch_ref.SHAPES; the device's rho rows besides stay within pitch_ref's bound
of the float64 oracle, and its track equals the float32 numpy restatement fed with the device's own rho rows.  (The host
restatement meets the same two checks on the same inputs in tests/test_pitch_host.py, on the CPU.)  All at 16 kHz on handles
of window_size 400; utterances at odd sample offsets, each followed directly by a full-scale neighbour."""
import ctypes as C

import numpy as np
import pytest

import pitch_ref as PR

pytestmark = pytest.mark.gpu

TRACK = dict(lag_cost=0.1, penalty=1.0, max_jump=16)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def make(pkg, shift=160, channels=1, norm=0, dyn=0, ibs=200000):
    m = pkg.MfccHip(ibs, 400, shift, 40, 16000.0, 64.0, 8000.0, 12, True, 22.0, norm, dyn, 3, 3, True, device=0, bug_compat=False,
                    channels=channels)
    m.set_window(pkg.reference_window(400))
    return m


def frames_of(rows, total):
    return [int(b - a) for a, b in zip(rows, list(rows[1:]) + [total])]


def set_pitch(m, name, **track):
    c = PR.SHAPES[name]
    k = dict(TRACK, **track)
    m.batch_set_pitch(c["lag_min"], c["lag_max"], window=c["window"], ballast=c.get("ballast", 0.0), lag_cost=k["lag_cost"],
                      penalty=k["penalty"], max_jump=k["max_jump"])


_HOST = {}


def host(pkg, name, u, T, **track):
    """mfx_host_pitch of utterance u of the shape (computed once per parameter set)."""
    k = dict(TRACK, **track)
    key = (name, u, T, tuple(sorted(k.items())))
    if key not in _HOST:
        c = PR.SHAPES[name]
        _HOST[key] = pkg.host_pitch(PR.shape_batch(name)[3][u], T, c["shift"], c["window"], c["lag_min"], c["lag_max"],
                                    c.get("ballast", 0.0), k["lag_cost"], k["penalty"], k["max_jump"], channels=c.get("channels", 1))
    return _HOST[key]


def check_against_host(pkg, name, rows, total, got, refs=True, **track):
    """got = (lag, rho, index, nccf) of the whole batch.  Bit for bit the host's; with refs, also the two reference checks."""
    c = PR.SHAPES[name]
    k = dict(TRACK, **track)
    lag, rho, idx, nccf = got
    assert np.isfinite(nccf).all() and np.isfinite(lag).all() and np.isfinite(rho).all()
    worst = 0.0
    for u, (r0, T) in enumerate(zip(rows, frames_of(rows, total))):
        want = host(pkg, name, u, T, **track)
        sl = slice(int(r0), int(r0) + T)
        assert np.array_equal(bits(nccf[sl]), bits(want[3])), "%s utterance %d: rho rows differ from mfx_host_pitch" % (name, u)
        assert np.array_equal(idx[sl], want[2]), "%s utterance %d: index" % (name, u)
        assert np.array_equal(bits(lag[sl]), bits(want[0])) and np.array_equal(bits(rho[sl]), bits(want[1])), (name, u)
        if refs and T > 0:
            ch = c.get("channels", 1)
            r64, B = PR.nccf_ref(PR.downmix(PR.shape_batch(name)[3][u], ch), T, c["shift"], c["window"], c["lag_min"], c["lag_max"],
                                 c.get("ballast", 0.0))
            err = np.abs(nccf[sl] - r64)
            assert (err <= B).all(), "%s utterance %d: |rho - rho64| exceeds the bound by %.3g" % (name, u, (err - B).max())
            worst = max(worst, float(np.where(B > 0, err / np.where(B > 0, B, 1.0), 0.0).max()))
            l2, r2, i2 = PR.track_ref(nccf[sl], c["lag_min"], c["lag_max"], k["lag_cost"], k["penalty"], k["max_jump"])
            assert np.array_equal(i2, idx[sl]) and np.array_equal(bits(l2), bits(lag[sl])) and np.array_equal(bits(r2), bits(rho[sl])), \
                "%s utterance %d: the track differs from the numpy restatement on the device's rho rows" % (name, u)
    if refs:
        print("%s: worst |rho - rho64| / B = %.4f" % (name, worst))


def run_shape(pkg, name, **track):
    c = PR.SHAPES[name]
    pcm, offs, lens, utts = PR.shape_batch(name)
    m = make(pkg, shift=c["shift"], channels=c.get("channels", 1))
    rows, total = m.batch_plan(offs, lens)
    set_pitch(m, name, **track)
    y = m.batch_run_host(pcm)
    got = m.batch_pitch_read(nccf=True)
    return m, rows, total, y, got


def same(a, b):
    return all(np.array_equal(bits(x) if x.dtype == np.float32 else x, bits(y) if y.dtype == np.float32 else y) for x, y in zip(a, b))


# ---- 1. the ragged batch -------------------------------------------------------------------------------------------------------

def test_ragged_batch_equals_the_host_and_meets_both_references(pkg):
    m, rows, total, y, got = run_shape(pkg, "ragged")
    assert frames_of(rows, total) == [0, 0, 1, 4, 63, 64, 65, 98]
    check_against_host(pkg, "ragged", rows, total, got)
    f0 = m.batch_pitch_read(f0=True)[3]
    assert f0.shape == (total,) and np.allclose(f0, 16000.0 / got[0].astype(np.float64))
    d_pitch, d_index = m.batch_pitch_device()
    assert d_pitch and d_index
    m.close()


def test_rows_do_not_depend_on_the_batch_the_offset_the_run_or_the_entry(pkg):
    import torch
    pcm, offs, lens, utts = PR.shape_batch("ragged")
    m, rows, total, y, got = run_shape(pkg, "ragged")
    # a second run
    y2 = m.batch_run_host(pcm)
    assert np.array_equal(bits(y2), bits(y)) and same(m.batch_pitch_read(nccf=True), got)
    # the device entry (asynchronous on the handle's stream) into arrays of its own
    dev = torch.device("cuda:0")
    t = torch.from_numpy(np.array(pcm)).to(dev)
    out = torch.full((total, y.shape[1]), float("nan"), dtype=torch.float32, device=dev)
    m.batch_run_device(t.data_ptr(), t.numel(), out.data_ptr())
    m.synchronize()
    assert np.array_equal(bits(out.cpu().numpy()), bits(y)) and same(m.batch_pitch_read(nccf=True), got)
    # every utterance alone, at another (even) offset behind other noise
    for u, (r0, T) in enumerate(zip(rows, frames_of(rows, total))):
        alone = np.concatenate((PR.loud(64 + 2 * u, 900 + u), utts[u], PR.loud(50, 950 + u)))
        alone = alone[:alone.size & ~1]
        r1, t1 = m.batch_plan([64 + 2 * u], [lens[u]])
        assert t1 == T
        set_pitch(m, "ragged")                                       # (a plan drops the track)
        m.batch_run_host(alone)
        a = m.batch_pitch_read(nccf=True)
        assert same(a, tuple(g[r0:r0 + T] for g in got)), "utterance %d alone" % u
    m.close()


# ---- 2. shapes -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["k1", "k37", "k281", "k512", "w32", "stereo", "shift1"])
def test_shapes(pkg, name):
    m, rows, total, y, got = run_shape(pkg, name)
    check_against_host(pkg, name, rows, total, got)
    m.close()


@pytest.mark.parametrize("jump", [1, 0])
def test_the_smallest_and_the_full_jump(pkg, jump):
    """max_jump 1, and K - 1 (as 0, and clamped from 511): the same track for the last two."""
    m, rows, total, y, got = run_shape(pkg, "k37", max_jump=jump, lag_cost=0.0, penalty=0.25)
    check_against_host(pkg, "k37", rows, total, got, max_jump=jump, lag_cost=0.0, penalty=0.25)
    if jump == 0:
        set_pitch(m, "k37", max_jump=511, lag_cost=0.0, penalty=0.25)
        m.batch_run_host(PR.shape_batch("k37")[0])
        assert same(m.batch_pitch_read(nccf=True), got)
    m.close()


@pytest.mark.parametrize("name", ["signals", "signals_ballast"])
def test_square_wave_silence_and_dc_give_finite_values_and_the_host_bits(pkg, name):
    m, rows, total, y, got = run_shape(pkg, name)
    check_against_host(pkg, name, rows, total, got)                  # (asserts finiteness first)
    T = frames_of(rows, total)
    silence = slice(int(rows[1]), int(rows[1]) + T[1])
    assert not got[3][silence].any() and (got[2][silence] == 0).all()          # s = 0 / s = ballast with c = 0: rho = 0
    assert (got[0][silence] == PR.SHAPES[name]["lag_min"]).all()
    m.close()


# ---- 3. composition ------------------------------------------------------------------------------------------------------------

def test_the_rows_are_the_same_bits_with_and_without_the_track(pkg):
    """CVN after the deltas, a splice + affine transform and a selecting VAD on one handle, mfx_batch_overlap on."""
    import torch
    pcm, offs, lens, utts = PR.shape_batch("ragged")
    m = make(pkg, norm=2, dyn=2)
    rows, total = m.batch_plan(offs, lens)
    rng = np.random.default_rng(3)
    A = rng.standard_normal((20, 3 * m.get_output_data_width())).astype(np.float32)
    m.batch_set_transform(A, rng.standard_normal(20).astype(np.float32), left=1, right=1)
    m.batch_set_vad(-1, 0.0, 1.0, 2, 0.6, pkg.VAD_SELECT)
    m.batch_overlap(True)
    dev = torch.device("cuda:0")
    t = torch.from_numpy(np.array(pcm)).to(dev)

    def run():
        outs = [torch.full((total, 20), float("nan"), dtype=torch.float32, device=dev) for _ in range(2)]
        for o in outs:                                               # two batches in flight
            m.batch_run_device(t.data_ptr(), t.numel(), o.data_ptr())
        m.synchronize()
        return [o.cpu().numpy() for o in outs]

    plain = run()
    vad = m.batch_vad_read()
    assert m.batch_output_width() == 20
    set_pitch(m, "ragged")
    assert m.batch_output_width() == 20
    with_track = run()
    for a, b in zip(plain + plain[:1], with_track + with_track[1:]):
        assert np.array_equal(bits(a), bits(b))
    assert same(m.batch_vad_read()[:3], vad[:3])
    check_against_host(pkg, "ragged", rows, total, m.batch_pitch_read(nccf=True), refs=False)   # indexed by the plan's rows
    m.batch_clear_pitch()
    assert np.array_equal(bits(run()[0]), bits(plain[0]))
    m.close()


def test_under_a_rates_plan_the_track_is_that_of_the_converted_pcm(pkg):
    a, b = PR.voiced(6000, 41), PR.voiced(9001, 42)
    pcm = np.concatenate((a[::2], PR.loud(5, 43), b, PR.loud(8, 44)))     # utterance 0 arrives at 8 kHz
    pcm = pcm[:pcm.size & ~1]
    offs, lens, rates = [0, 3005], [3000, 9001], [8000, 16000]
    m = make(pkg)
    rows, total = m.batch_plan_rates(offs, lens, rates)
    m.batch_set_pitch(40, 320, **TRACK)
    m.batch_run_host(pcm)
    got = m.batch_pitch_read(nccf=True)
    conv = m.debug_read(8)
    off2, len2, total2 = m.batch_resample_layout()
    assert frames_of(rows, total)[0] > 30 and conv.size >= total2
    m.close()
    t = make(pkg)
    rows2, total_2 = t.batch_plan(off2, len2)
    assert list(rows2) == list(rows) and total_2 == total
    t.batch_set_pitch(40, 320, **TRACK)
    t.batch_run_host(conv[:total2])
    assert same(t.batch_pitch_read(nccf=True), got)
    t.close()


def test_state_and_configuration_errors(pkg):
    L = pkg.load_library()
    pcm, offs, lens, utts = PR.shape_batch("k37")
    m = make(pkg)
    none = (None, None, None)
    assert L.mfx_batch_set_pitch(m._h, 0, 40, 76, 0.0, 0.1, 1.0, 16) == -8             # no plan yet
    assert L.mfx_batch_pitch_read(m._h, *none) == -8 and L.mfx_batch_pitch_device(m._h, None, None) == -8
    m.batch_plan(offs, lens)
    for bad in ((31, 40, 76, 0.0, 0.1, 1.0, 16), (0, 1, 76, 0.0, 0.1, 1.0, 16), (0, 40, 1025, 0.0, 0.1, 1.0, 16),
                (0, 2, 514, 0.0, 0.1, 1.0, 16), (0, 40, 76, -1.0, 0.1, 1.0, 16), (0, 40, 76, 0.0, 1.5, 1.0, 16),
                (0, 40, 76, 0.0, 0.1, float("nan"), 16), (0, 40, 76, 0.0, 0.1, 1.0, 512), (0, 40, 76, 0.0, 0.1, 1.0, -1)):
        assert L.mfx_batch_set_pitch(m._h, *bad) == -7, bad
    assert L.mfx_batch_pitch_read(m._h, *none) == -8                                    # a refused setter attaches nothing
    m.batch_set_pitch(40, 76, window=0, **TRACK)                                        # window 0: the handle's 400
    assert L.mfx_batch_pitch_read(m._h, *none) == -8                                    # before a run
    m.batch_run_host(pcm)
    assert L.mfx_batch_pitch_read(m._h, *none) == 0                                     # any output may be NULL
    first = m.batch_pitch_read(nccf=True)
    m.batch_clear_pitch()
    assert L.mfx_batch_pitch_read(m._h, *none) == -8 and L.mfx_batch_pitch_device(m._h, None, None) == -8
    set_pitch(m, "k37")
    m.batch_run_host(pcm)
    assert same(m.batch_pitch_read(nccf=True), first)                                   # (window 400 spelled out: the same)
    m.batch_plan(offs, lens)                                                            # a new plan drops it
    assert L.mfx_batch_pitch_read(m._h, *none) == -8
    # a batch without rows counts as run, and copies nothing
    rows, total = m.batch_plan([1], [300])
    assert total == 0
    set_pitch(m, "k37")
    m.batch_run_host(pcm)
    assert all(a.shape[0] == 0 for a in m.batch_pitch_read(nccf=True))
    m.close()
    s = pkg.MfccHip(200000, 400, 160, 80, 16000.0, 0.0, 8000.0, 0, False, 22.0, device=0, bug_compat=False,
                    method=pkg.METHOD_STFT_LOGMEL)
    s.set_window(pkg.periodic_hann(400))
    s.batch_plan(offs, lens)
    assert L.mfx_batch_set_pitch(s._h, 0, 40, 76, 0.0, 0.1, 1.0, 16) == -5              # centred frames
    s.close()


def test_sliced_host_run_with_pinned_buffers_gives_the_same_track(pkg):
    """The smallest batch that takes the sliced path of mfx_batch_run_host -- 8 utterances (two slices), 32 MB of PCM, pinned
    buffers: every slice runs the track of its utterance range.  Against the same handle's run from pageable buffers."""
    L = pkg.load_library()
    L.mfx_alloc_pinned.restype, L.mfx_alloc_pinned.argtypes = C.c_void_p, [C.c_size_t]
    L.mfx_free_pinned.restype, L.mfx_free_pinned.argtypes = None, [C.c_void_p]
    rng = np.random.default_rng(23)
    lens = [int(v) for v in rng.integers(2100000, 2110000, size=8)]
    offs, pos = [], 0
    for n in lens:
        offs.append(pos)
        pos += n + (n & 1)
    base = PR.voiced(1 << 16, 77)
    pcm = np.tile(base, pos // base.size + 1)[:pos].copy()
    m = make(pkg, ibs=4000000)
    rows, total = m.batch_plan(offs, lens)
    m.batch_set_pitch(60, 96, penalty=1.0, lag_cost=0.1, max_jump=8)
    y = m.batch_run_host(pcm)
    want = m.batch_pitch_read(nccf=True)
    width = y.shape[1]
    p_in, p_out = L.mfx_alloc_pinned(pcm.nbytes), L.mfx_alloc_pinned(y.nbytes)
    assert p_in and p_out
    try:
        C.memmove(p_in, pcm.ctypes.data, pcm.nbytes)
        rc = L.mfx_batch_run_host(m._h, C.cast(p_in, C.POINTER(C.c_int16)), pcm.size, C.cast(p_out, C.POINTER(C.c_float)))
        assert rc == 0
        got_y = np.ctypeslib.as_array(C.cast(p_out, C.POINTER(C.c_float)), shape=(total, width)).copy()
        assert np.array_equal(bits(got_y), bits(y)) and same(m.batch_pitch_read(nccf=True), want)
    finally:
        m.synchronize()
        L.mfx_free_pinned(p_in), L.mfx_free_pinned(p_out)
    # and the host's bits on the first frames of the last utterance (the last slice's range)
    T = 40
    h = pkg.host_pitch(pcm[offs[7]:offs[7] + lens[7]][:T * 160 + 400 + 96], T, 160, 400, 60, 96, 0.0, 0.1, 1.0, 8)
    r0 = int(rows[7])
    assert np.array_equal(bits(want[3][r0:r0 + T]), bits(h[3]))
    m.close()
