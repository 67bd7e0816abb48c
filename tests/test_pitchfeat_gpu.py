"""Pitch features of the batch entries (mfx_batch_set_pitch_feats; mfx_pitchfeat.hip: k_pitch_feats, k_pitch_paste) on the
MI355X.

The definition of include/mfx.h is in double with the platform's exp, ln and pow, so the device is held to the float64
reference of pitchfeat_ref.py computed from the device's OWN track, within that file's bound B, and to the host restatement
mfx_host_pitch_feats within 2 B (one B each); how many values are the host's bits is printed, not asserted.  What must be
bit for bit is asserted so: the same values alone and in the batch, run after run, through either entry, the sliced path and
at any placement; the first Wd columns of pasted rows against a handle without the paste; the last F against the feats array.
All at 16 kHz on handles of window_size 400, the track at window 400 and lags 40 .. 76 (cheap); utterances at odd sample
offsets, each followed directly by a full-scale neighbour."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

import pitch_ref as PR
import pitchfeat_ref as R
import vad_ref as VR
import xform_ref as XR

pytestmark = pytest.mark.gpu

RATE = 16000.0
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def same(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def make(pkg, norm=0, dyn=0, ibs=200000):
    m = pkg.MfccHip(ibs, 400, 160, 40, RATE, 64.0, 8000.0, 12, True, 22.0, norm, dyn, 3, 3, True, device=0, bug_compat=False)
    m.set_window(pkg.reference_window(400))
    return m


def set_track(m):
    k = R.TRACK
    m.batch_set_pitch(k["lag_min"], k["lag_max"], window=k["window"], lag_cost=k["lag_cost"], penalty=k["penalty"], max_jump=k["max_jump"])


def set_feats(m, s, paste=False):
    m.batch_set_pitch_feats(columns=s["columns"], left=s["left"], right=s["right"], delta_window=s["D"], paste=paste)


def frames_of(rows, total):
    return [int(b - a) for a, b in zip(rows, list(rows[1:]) + [total])]


def planned(pkg, **cfg):
    pcm, offs, lens, utts = R.ragged()
    m = make(pkg, **cfg)
    rows, total = m.batch_plan(offs, lens)
    assert frames_of(rows, total) == list(R.FRAMES)
    return m, pcm, rows, total


def run_device(m, pcm_t, total, width, torch, pad=64, shift=0, fill=float("nan")):
    """mfx_batch_run_device into the middle of a canary array, `shift` floats off its 256-byte alignment; returns the rows and
    asserts that nothing outside [d_out, d_out + total * width) was written."""
    buf = torch.full((total * width + 2 * pad + 8,), fill, dtype=torch.float32, device=pcm_t.device)
    lo = pad + shift
    m.batch_run_device(pcm_t.data_ptr(), pcm_t.numel(), buf.data_ptr() + 4 * lo)
    m.synchronize()
    h = buf.cpu().numpy()
    assert np.isnan(h[:lo]).all() and np.isnan(h[lo + total * width:]).all(), "written outside the run's rows"
    return h[lo:lo + total * width].reshape(total, width).copy()


# ---- 1. numbers ----------------------------------------------------------------------------------------------------------------

def test_ragged_batch_meets_the_reference_and_the_host_at_every_setting(pkg):
    m, pcm, rows, total = planned(pkg)
    set_track(m)
    worst, same_n, n = 0.0, 0, 0
    for s in R.SETTINGS:
        set_feats(m, s)
        y = m.batch_run_host(pcm)
        assert y.shape == (total, m.get_output_data_width())
        lag, rho, idx = m.batch_pitch_read()
        feats = m.batch_pitch_feats_read()
        d, F = m.batch_pitch_feats_device()
        assert d and F == R.n_columns(s["columns"]) and feats.shape == (total, F)
        for r0, T in zip(rows, frames_of(rows, total)):
            sl = slice(int(r0), int(r0) + T)
            what = "%d frames, %s" % (T, s)
            w, _ = R.check(feats[sl], lag[sl], rho[sl], RATE, what=what, **s)
            host = pkg.host_pitch_feats(lag[sl], rho[sl], RATE, columns=s["columns"], left=s["left"], right=s["right"], delta_window=s["D"])
            R.check(host, lag[sl], rho[sl], RATE, what="host, " + what, **s)
            ref, A = R.feats_ref(lag[sl], rho[sl], RATE, **s)
            if T:
                err = np.abs(feats[sl].astype(np.float64) - host.astype(np.float64))
                assert (err <= 2.0 * R.bound(ref, A)).all(), "%s: device and host differ by more than 2 B" % what
            worst, same_n, n = max(worst, w), same_n + int((bits(feats[sl]) == bits(host)).sum()), n + host.size
    print("device: worst err / B = %.4f; %.2f %% of %d values are mfx_host_pitch_feats' bits" % (worst, 100.0 * same_n / n, n))
    m.close()


def test_values_do_not_depend_on_the_batch_the_run_the_entry_or_the_placement(pkg):
    import torch
    pcm, offs, lens, utts = R.ragged()
    m, pcm, rows, total = planned(pkg, norm=2, dyn=2)
    set_track(m)
    s = R.SETTINGS[0]
    set_feats(m, s, paste=True)
    Wy = m.batch_output_width()
    assert Wy == m.get_output_data_width() + 4
    y = m.batch_run_host(pcm)
    feats = m.batch_pitch_feats_read()
    assert y.shape == (total, Wy) and same(y[:, -4:], feats)
    # a second run
    assert same(m.batch_run_host(pcm), y) and same(m.batch_pitch_feats_read(), feats)
    # the device entry, at two alignments of d_out, nothing written outside the rows
    t = torch.from_numpy(np.array(pcm)).to("cuda:0")
    for shift in (0, 1, 3):
        assert same(run_device(m, t, total, Wy, torch, shift=shift), y), "d_out %d floats off" % shift
        assert same(m.batch_pitch_feats_read(), feats)
    # every utterance alone, at another (even) offset behind other noise
    for u, (r0, T) in enumerate(zip(rows, frames_of(rows, total))):
        if T == 0:
            continue
        alone = np.concatenate((PR.loud(64 + 2 * u, 900 + u), utts[u], PR.loud(50, 950 + u)))
        alone = alone[:alone.size & ~1]
        r1, t1 = m.batch_plan([64 + 2 * u], [lens[u]])
        assert t1 == T
        set_track(m)                                                  # (a plan drops the attachments)
        set_feats(m, s, paste=True)
        ya = m.batch_run_host(alone)
        assert same(ya, y[r0:r0 + T]) and same(m.batch_pitch_feats_read(), feats[r0:r0 + T]), "utterance %d alone" % u
    m.close()


def test_sliced_host_run_with_pinned_buffers_gives_the_same_rows_and_feats(pkg):
    """The smallest batch that takes the sliced path of mfx_batch_run_host -- 8 utterances (two slices), 32 MB of PCM, pinned
    buffers -- with the paste in force: every slice runs the track, the features and the paste of its utterance range."""
    L = pkg.load_library()
    L.mfx_alloc_pinned.restype, L.mfx_alloc_pinned.argtypes = C.c_void_p, [C.c_size_t]
    L.mfx_free_pinned.restype, L.mfx_free_pinned.argtypes = None, [C.c_void_p]
    rng = np.random.default_rng(29)
    lens = [int(v) for v in rng.integers(2100000, 2110000, size=8)]
    offs, pos = [], 0
    for n in lens:
        offs.append(pos)
        pos += n + (n & 1)
    base = PR.voiced(1 << 16, 78)
    pcm = np.tile(base, pos // base.size + 1)[:pos].copy()
    m = make(pkg, dyn=2, ibs=4000000)
    rows, total = m.batch_plan(offs, lens)
    set_track(m)
    set_feats(m, R.SETTINGS[0], paste=True)
    y = m.batch_run_host(pcm)                                        # pageable: one piece
    feats = m.batch_pitch_feats_read()
    Wy = y.shape[1]
    assert Wy == m.get_output_data_width() + 4 and same(y[:, -4:], feats)
    p_in, p_out = L.mfx_alloc_pinned(pcm.nbytes), L.mfx_alloc_pinned(y.nbytes)
    assert p_in and p_out
    try:
        C.memmove(p_in, pcm.ctypes.data, pcm.nbytes)
        rc = L.mfx_batch_run_host(m._h, C.cast(p_in, C.POINTER(C.c_int16)), pcm.size, C.cast(p_out, C.POINTER(C.c_float)))
        assert rc == 0
        got = np.ctypeslib.as_array(C.cast(p_out, C.POINTER(C.c_float)), shape=(total, Wy)).copy()
        assert same(got, y) and same(m.batch_pitch_feats_read(), feats)
    finally:
        m.synchronize()
        L.mfx_free_pinned(p_in), L.mfx_free_pinned(p_out)
    # and the reference on the first rows of the last utterance (the last slice's range; left = 75 reaches no further back)
    lag, rho, idx = m.batch_pitch_read()
    r0, T = int(rows[7]), 200
    ref, A = R.feats_ref(lag[r0:r0 + T + 75], rho[r0:r0 + T + 75], RATE, **R.SETTINGS[0])
    err = np.abs(feats[r0:r0 + T].astype(np.float64) - ref[:T])
    assert (err <= R.bound(ref, A)[:T]).all()
    m.close()


# ---- 2. composition ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("overlap", [False, True])
def test_pasted_rows_are_the_unpasted_rows_and_the_feats(pkg, overlap):
    """CVN + deltas; with mfx_batch_overlap two batches in flight."""
    import torch
    m, pcm, rows, total = planned(pkg, norm=2, dyn=2)
    Wd = m.get_output_data_width()
    t = torch.from_numpy(np.array(pcm)).to("cuda:0")
    plain = run_device(m, t, total, Wd, torch)
    set_track(m)
    s = dict(columns=0, left=75, right=75, D=2)
    set_feats(m, s)                                                  # paste = 0: d_out and the width are untouched
    assert m.batch_output_width() == Wd
    assert same(run_device(m, t, total, Wd, torch), plain)
    feats = m.batch_pitch_feats_read()
    set_feats(m, s, paste=True)
    Wy = m.batch_output_width()
    assert Wy == Wd + 3
    m.batch_overlap(overlap)
    outs = [torch.full((total * Wy + 128,), float("nan"), dtype=torch.float32, device="cuda:0") for _ in range(2)]
    for o in outs:
        m.batch_run_device(t.data_ptr(), t.numel(), o.data_ptr() + 4 * 63)     # (an odd float offset)
    m.synchronize()
    for o in outs:
        h = o.cpu().numpy()
        assert np.isnan(h[:63]).all() and np.isnan(h[63 + total * Wy:]).all()
        wide = h[63:63 + total * Wy].reshape(total, Wy)
        assert same(wide[:, :Wd], plain), "the first Wd columns moved"
        assert same(wide[:, Wd:], feats) and same(m.batch_pitch_feats_read(), feats)
    # clear: today's bits and width
    m.batch_clear_pitch_feats()
    assert m.batch_output_width() == Wd and same(run_device(m, t, total, Wd, torch), plain)
    set_feats(m, s, paste=True)
    m.batch_clear_pitch()                                            # (drops the features with the track)
    assert m.batch_output_width() == Wd and same(run_device(m, t, total, Wd, torch), plain)
    m.close()


def test_paste_then_transform_splices_the_wide_rows(pkg):
    m, pcm, rows, total = planned(pkg, norm=2, dyn=2)
    set_track(m)
    set_feats(m, dict(columns=0, left=75, right=75, D=2), paste=True)
    Wy = m.batch_output_width()
    wide = m.batch_run_host(pcm)
    rng = np.random.default_rng(11)
    left, right, od = 2, 1, 20
    A = rng.standard_normal((od, (left + right + 1) * Wy)).astype(np.float32)
    b = rng.standard_normal(od).astype(np.float32)
    m.batch_set_transform(A, b, left=left, right=right)
    assert m.batch_output_width() == od
    got = m.batch_run_host(pcm)
    XR.assert_xform_consistent(got, wide, [int(r) for r in rows], frames_of(rows, total), A, b, left, right, what="paste + transform")
    with pytest.raises(ValueError):                                  # in_dim is C * Wy, not C * Wd
        m.batch_set_transform(np.zeros((od, (left + right + 1) * (Wy - 3)), np.float32), left=left, right=right)
    m.batch_set_transform(None)
    assert m.batch_output_width() == Wy and same(m.batch_run_host(pcm), wide)
    m.close()


@pytest.mark.parametrize("mode", ["SELECT", "PACK"])
def test_paste_then_vad_moves_the_wide_rows(pkg, mode):
    m, pcm, rows, total = planned(pkg, dyn=2)
    frames = frames_of(rows, total)
    vad = (-1, 0.0, 1.0, 2, 0.6)
    m.batch_set_vad(*vad, pkg.VAD_FLAGS)
    m.batch_run_host(pcm)
    flags = m.batch_vad_read()[0]
    m.batch_clear_vad()
    set_track(m)
    set_feats(m, dict(columns=15, left=3, right=0, D=1), paste=True)
    wide = m.batch_run_host(pcm)
    m.batch_set_vad(*vad, getattr(pkg, "VAD_" + mode))
    got = m.batch_run_host(pcm)
    dec = m.batch_vad_read()
    assert np.array_equal(dec[0], flags) and 0 < dec[3] < total     # the decision reads its column where it was
    want = VR.select_ref(wide, rows, frames, flags) if mode == "SELECT" else VR.pack_ref(wide, rows, frames, flags)[0]
    assert got.shape == wide.shape and same(got, want)
    assert same(m.batch_pitch_feats_read(), wide[:, -4:])            # indexed by the plan's rows in every mode
    m.close()


def test_a_rates_plan_works(pkg):
    a, b = PR.voiced(6000, 41), PR.voiced(9001, 42)
    pcm = np.concatenate((a[::2], PR.loud(5, 43), b, PR.loud(8, 44)))     # utterance 0 arrives at 8 kHz
    pcm = pcm[:pcm.size & ~1]
    offs, lens, rates = [0, 3005], [3000, 9001], [8000, 16000]
    m = make(pkg, dyn=2)
    rows, total = m.batch_plan_rates(offs, lens, rates)
    plain = m.batch_run_host(pcm)
    set_track(m)
    s = dict(columns=0, left=75, right=75, D=2)
    set_feats(m, s, paste=True)
    y = m.batch_run_host(pcm)
    lag, rho, idx = m.batch_pitch_read()
    feats = m.batch_pitch_feats_read()
    assert same(y[:, :-3], plain) and same(y[:, -3:], feats)
    for r0, T in zip(rows, frames_of(rows, total)):
        assert T > 30
        R.check(feats[r0:r0 + T], lag[r0:r0 + T], rho[r0:r0 + T], RATE, what="rates plan", **s)
    m.close()


# ---- 3. refusals ---------------------------------------------------------------------------------------------------------------

def test_state_order_rule_and_every_other_refusal(pkg):
    L = pkg.load_library()
    pcm, offs, lens, utts = R.ragged()
    m = make(pkg, dyn=2)
    ok = (0, 75, 75, 2, 2.0, 0.0, 2.0, 10.0)
    assert L.mfx_batch_set_pitch_feats(m._h, *ok, 0) == -8           # no plan yet
    assert L.mfx_batch_pitch_feats_read(m._h, None) == -8 and L.mfx_batch_pitch_feats_device(m._h, None, None) == -8
    rows, total = m.batch_plan(offs, lens)
    assert L.mfx_batch_set_pitch_feats(m._h, *ok, 0) == -8           # no pitch track in force
    set_track(m)
    for bad in ((16,) + ok[1:], (-1,) + ok[1:], (0, -1) + ok[2:], (0, 1025) + ok[2:], (0, 75, -1) + ok[3:], (0, 75, 1025) + ok[3:],
                (0, 75, 75, 0) + ok[4:], (0, 75, 75, 17) + ok[4:], (0, 75, 75, 2, float("nan"), 0.0, 2.0, 10.0),
                (0, 75, 75, 2, 2.0, float("inf"), 2.0, 10.0), (0, 75, 75, 2, 2.0, 0.0, float("-inf"), 10.0),
                (0, 75, 75, 2, 2.0, 0.0, 2.0, float("nan"))):
        assert L.mfx_batch_set_pitch_feats(m._h, *bad, 0) == -7, bad
    assert L.mfx_batch_set_pitch_feats(m._h, *ok, 2) == -7 and L.mfx_batch_set_pitch_feats(m._h, *ok, -1) == -7
    assert L.mfx_batch_pitch_feats_device(m._h, None, None) == -8    # a refused setter attaches nothing
    Wd = m.get_output_data_width()
    assert m.batch_output_width() == Wd
    m.batch_set_pitch_feats()
    assert L.mfx_batch_pitch_feats_read(m._h, None) == -8            # before a run
    plain = m.batch_run_host(pcm)
    assert L.mfx_batch_pitch_feats_read(m._h, None) == 0
    feats3 = m.batch_pitch_feats_read()

    # the order rule: nothing changes Wy while a transform or a VAD is in force
    A = np.zeros((8, Wd), np.float32)
    for attach, clear in ((lambda: m.batch_set_transform(A), lambda: m.batch_set_transform(None)),
                          (lambda: m.batch_set_vad(-1, 0.0, 1.0, 2, 0.6, pkg.VAD_FLAGS), m.batch_clear_vad)):
        attach()
        assert L.mfx_batch_set_pitch_feats(m._h, *ok, 1) == -8       # setting with paste
        assert L.mfx_batch_set_pitch_feats(m._h, 15, *ok[1:], 0) == 0    # without: Wy stays
        assert L.mfx_batch_set_pitch_feats(m._h, *ok, 0) == 0
        clear()
    m.batch_set_pitch_feats(paste=True)
    assert m.batch_output_width() == Wd + 3
    A = np.zeros((8, Wd + 3), np.float32)
    for attach, clear in ((lambda: m.batch_set_transform(A), lambda: m.batch_set_transform(None)),
                          (lambda: m.batch_set_vad(-1, 0.0, 1.0, 2, 0.6, pkg.VAD_SELECT), m.batch_clear_vad)):
        attach()
        assert L.mfx_batch_set_pitch_feats(m._h, *ok, 0) == -8       # dropping the paste
        assert L.mfx_batch_set_pitch_feats(m._h, 15, *ok[1:], 1) == -8   # changing F under paste
        assert L.mfx_batch_clear_pitch_feats(m._h) == -8 and L.mfx_batch_clear_pitch(m._h) == -8
        assert L.mfx_batch_set_pitch_feats(m._h, 11, 3, 0, 1, 1.0, 1.0, 1.0, 1.0, 1) == 0   # F = 3 again: Wy stays
        assert L.mfx_batch_set_pitch_feats(m._h, *ok, 1) == 0
        clear()
    y = m.batch_run_host(pcm)
    assert same(y[:, :Wd], plain) and same(y[:, Wd:], feats3)       # (every refusal above left the attachment as it was)
    m.batch_plan(offs, lens)                                         # a new plan drops it
    assert L.mfx_batch_pitch_feats_read(m._h, None) == -8 and m.batch_output_width() == Wd
    # a batch without rows counts as run
    rows0, total0 = m.batch_plan([1], [300])
    assert total0 == 0
    set_track(m)
    m.batch_set_pitch_feats(paste=True)
    m.batch_run_host(pcm)
    assert m.batch_pitch_feats_read().shape == (0, 3)
    m.close()


# ---- 4. the driver -------------------------------------------------------------------------------------------------------------

def read_htk(path):
    raw = open(path, "rb").read()
    n, period, size, kind = struct.unpack(">iihh", raw[:12])
    return np.frombuffer(raw[12:], ">f4").astype(np.float32).reshape(n, size // 4)


def test_driver_pastes_the_three_default_columns(pkg, orc, tmp_path):
    exe = os.path.join(ROOT, "asr-featext-opencl_amd", "host", "afet_hip")
    assert os.path.exists(exe), "afet_hip is built by build()"
    wavs = []
    for i in range(3):
        dst = tmp_path / ("u%d.wav" % i)
        dst.write_bytes(open(os.path.join(GOLDEN, "a0001.wav" if i != 1 else "a1.wav"), "rb").read())
        wavs.append(str(dst))
    shape = ["--banks", "40", "--ceps", "12", "--c0", "1", "--norm", "0", "--dyn", "2", "--low-freq", "64", "--high-freq", "8000",
             "--bug-compat", "0", "--htk", "--batch-mb", "64"]

    def run(tag, *extra):
        out = tmp_path / tag
        out.mkdir()
        outs = [str(out / ("u%d.htk" % i)) for i in range(len(wavs))]
        pairs = [x for pair in zip(wavs, outs) for x in pair]
        r = subprocess.run([exe, *shape, *extra, *pairs], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
        assert r.returncode == 0, r.stdout[-2000:]
        return [read_htk(o) for o in outs]

    plain = run("plain")
    wide = {(50, 400): run("pitch", "--pitch"), (100, 300): run("pitch2", "--pitch", "--pitch-range", "100:300")}
    again = run("plain2", "--pitch-range", "100:400")               # the range without --pitch: nothing changes
    for a, b in zip(plain, again):
        assert same(a, b)
    # the same files through the Python binding: the driver's batch (even offsets), its track parameters, Kaldi's defaults
    pcms = [orc.read_wav_pcm16(w) for w in wavs]
    sr = pcms[0][1]
    utts = [p[0][:, 0].copy() for p in pcms]
    Wd, Sd = int(sr * 25.0 * 1e-3), int(sr * 10.0 * 1e-3)
    m = pkg.MfccHip(1000000, Wd, Sd, 40, float(sr), 64.0, 8000.0, 12, True, 22.0, 0, 2, 3, 3, True, device=0, bug_compat=False, engine=8)
    m.set_window(pkg.reference_window(Wd))
    offs, pos = [], 0
    for u in utts:
        offs.append(pos)
        pos += u.size + (u.size & 1)
    pcm = np.zeros(pos + 8, np.int16)
    for o_, u in zip(offs, utts):
        pcm[o_:o_ + u.size] = u
    rows, total = m.batch_plan(offs, [u.size for u in utts])
    for (lo, hi), got in wide.items():
        m.batch_set_pitch(int(np.floor(sr / hi)), int(np.ceil(sr / lo)), window=0, ballast=0.0, lag_cost=0.1, penalty=1.0, max_jump=16)
        m.batch_set_pitch_feats(paste=True)
        y = m.batch_run_host(pcm)
        m.batch_clear_pitch()
        for u, (r0, T) in enumerate(zip(rows, frames_of(rows, total))):
            assert got[u].shape == (T, plain[u].shape[1] + 3), "file %d" % u
            assert same(got[u][:, :-3], plain[u]), "file %d: the cepstra moved" % u
            assert same(got[u], y[r0:r0 + T]), "file %d at %d:%d Hz: not the binding's rows" % (u, lo, hi)
    assert not same(wide[(50, 400)][0], wide[(100, 300)][0])         # (the range reaches the track)
    m.close()
