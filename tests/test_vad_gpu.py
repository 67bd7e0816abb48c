"""Energy VAD and voiced-frame selection as the last stage of the batch entries (mfx_batch_set_vad; mfx_vad.hip) on the
MI355X.

The rows y the stage reads are those of a TWIN handle of the same configuration and plan without a VAD, so only the new
stage is under test.  Given y the stage is an exact function but for the threshold's summation order:
  - the thresholds lie within vad_ref.thr_ref's derived bound of the float64 value;
  - the flags EQUAL vad_ref.flags_ref(y[:, column], the threshold as returned), the counts their sums;
  - SELECT / PACK deliver the twin's rows at the voiced frames bit for bit, +0.0 elsewhere, and touch nothing outside d_out.
All shapes 16 kHz, W = 400, S = 160, 512-point FFT.

Condition on the inputs (checked on the CPU with the oracle's rows before any GPU run, see input_condition): over the
utterances of at least 63 frames, the two constant ones left out, between 20 % and 80 % of the frames are voiced for every
parameter set, and every configuration meets an all-voiced and an all-unvoiced utterance."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

import vad_ref as VR
from conftest import GOLDEN, synth_utterance
from placement import OutPlacement

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, S, SR = 400, 160, 16000.0
# edge windows inside one tile, a frameless utterance, the tile boundaries, more than one tile, more than one 4096-row
# chunk of the threshold's sum; then the two constant utterances: digital silence, loud throughout
FRAMES = [1, 2, 3, 0, 63, 64, 65, 145, 4200, 100, 70]
SILENT, LOUD = 9, 10
# gain envelope in frames, (loud, run length): voiced runs of 1, 3, 7 and 40 frames drift across the 64-row tile edges (the
# short cycle is 102 frames long), a loud run longer than the widest window (129 frames) and a quiet one longer than it
SHORT = [(1, 40), (0, 7), (1, 3), (0, 1), (1, 7), (0, 40), (1, 1), (0, 3)]
RUNS = SHORT * 2 + [(1, 900), (0, 1300)]
QUIET = 1.0 / 256.0

CONFIGS = {
    # name: nb, nc, want_c0, dyn, norm, VAD column, energy_threshold of the offset case (energy_mean_scale 0.5 there)
    "mfcc39": dict(nb=40, nc=12, c0=True, dyn=2, norm=0, column=-1, et=-31.0),      # 12 + c0, d, dd; decision on c0
    "mfcc39cvn": dict(nb=40, nc=12, c0=True, dyn=2, norm=2, column=-1, et=0.25),    # CVN after the deltas: NaN rows at T = 1
    "mfcc13": dict(nb=40, nc=12, c0=True, dyn=0, norm=0, column=-1, et=-31.0),      # no deltas: not via the statics scratch
    "fbank128": dict(nb=64, nc=0, c0=False, dyn=1, norm=0, column=0, et=-5.0),      # 64 log mel energies + d; first band
}
PARAMS = [(0, 0.5), (2, 0.6), (32, 0.12), (64, 1.0)]           # (frames_context, proportion_threshold); (2, 0.6): Kaldi's


def cases(name):
    """(et, ms, ctx, p): every parameter set at et = 0, ms = 1, plus one offset case."""
    return [(0.0, 1.0, c, p) for c, p in PARAMS] + [(CONFIGS[name]["et"], 0.5, 2, 0.6)]


def make(pkg, name, engine=0, ibs=200000):
    k = CONFIGS[name]
    m = pkg.MfccHip(ibs, W, S, k["nb"], SR, 64.0, SR / 2, k["nc"], k["c0"], 22.0, k["norm"], k["dyn"], 3, 3, True,
                    device=0, bug_compat=False, engine=engine)
    m.set_window(pkg.reference_window(W))
    return m


def column_of(name, width):
    k = CONFIGS[name]
    return k["column"] if k["column"] >= 0 else width // (1 + k["dyn"]) - 1


def envelope(T, phase):
    g = []
    while len(g) < T + phase:
        for loud, n in RUNS:
            g += [1.0 if loud else QUIET] * n
    return np.asarray(g[phase:phase + T])


_RAGGED = {}


def ragged():
    """The ragged batch (computed once, never modified): utterances, offsets, lengths, PCM."""
    if not _RAGGED:
        lens = [300 if T == 0 else (T - 1) * S + W + 7 * (i % 3) for i, T in enumerate(FRAMES)]
        utts = []
        for i, (n, T) in enumerate(zip(lens, FRAMES)):
            x = synth_utterance(n, 70 + i).astype(np.float64)
            if i == SILENT:
                x[:] = 0.0
            elif i != LOUD and T > 0:
                x *= envelope(T + 3, 29 * i)[np.minimum(np.arange(n) // S, T + 2)]
            utts.append(np.round(x).astype(np.int16))
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


_CONDITION = set()


def input_condition(orc, name):
    """The condition on the test data, on the oracle's rows (CPU), once per configuration."""
    if name in _CONDITION:
        return
    d, k = ragged(), CONFIGS[name]
    cfg = orc.make_config(max(d["lens"]) + 1000, window_size=W, shift=S, num_banks=k["nb"], high_freq=SR / 2, ceps_len=k["nc"],
                          want_c0=k["c0"], norm=k["norm"], dyn=k["dyn"], delta_l1=3, delta_l2=3)
    e = {}
    for u, T in enumerate(FRAMES):
        if T >= 63:
            y = orc.run_utterance(cfg, d["utts"][u], None, bug_compat=False)
            assert y.shape[0] == T
            e[u] = y[:, column_of(name, y.shape[1])]
    seen_all, seen_none = False, False
    for et, ms, ctx, p in cases(name):
        voiced = total = 0
        for u, eu in e.items():
            f = VR.flags_ref(eu, np.float32(VR.thr_ref(eu, et, ms)[0]), ctx, p)
            seen_all, seen_none = seen_all or bool(f.all()), seen_none or not f.any()
            if u not in (SILENT, LOUD):
                voiced, total = voiced + int(f.sum()), total + f.size
        assert 0.2 <= voiced / total <= 0.8, "%s %s: %.3f of the frames voiced" % (name, (et, ms, ctx, p), voiced / total)
    assert seen_all and seen_none, name
    _CONDITION.add(name)


_TWIN = {}


def twin_rows(pkg, orc, name):
    """(rows, y): the ragged batch through a handle WITHOUT a VAD (computed once per configuration)."""
    input_condition(orc, name)
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


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def planned(pkg, name):
    d = ragged()
    m = make(pkg, name)
    rows, total = m.batch_plan(d["offs"], d["lens"])
    return m, rows, total


def check_decision(name, y, rows, frames, got, et, ms, ctx, p, what=""):
    """Thresholds within their bound, flags equal to the rule on y at the returned thresholds, counts their sums."""
    flags, voiced, thr, total_voiced = got
    col = column_of(name, y.shape[1])
    assert flags.shape == (sum(frames),) and set(np.unique(flags)) <= {0, 1}
    for u, (r0, T) in enumerate(zip(rows, frames)):
        e = y[r0:r0 + T, col]
        want, bound = VR.thr_ref(e, et, ms)
        print("%s u%d T=%d thr %r ref %r bound %.3g voiced %d" % (what, u, T, float(thr[u]), want, bound, voiced[u]))
        if T == 0:
            assert thr[u] == np.float32(et) and voiced[u] == 0
            continue
        if np.isnan(want):
            assert np.isnan(thr[u]), (what, u)
        else:
            assert abs(float(thr[u]) - want) <= bound, (what, u, float(thr[u]), want, bound)
        assert np.array_equal(flags[r0:r0 + T], VR.flags_ref(e, thr[u], ctx, p)), (what, u)
        assert voiced[u] == int(flags[r0:r0 + T].sum()), (what, u)
    assert total_voiced == int(flags.sum())


def run_placed(m, pcm, total, width, k=1):
    """One device run into a canary-filled allocation, d_out k floats past a 16-byte boundary: the interior, checked."""
    import torch
    dev = torch.device("cuda:0")
    t = torch.from_numpy(np.array(pcm, np.int16)).to(dev)
    out = OutPlacement(total, width, k=k)
    m.batch_run_device(t.data_ptr(), t.numel(), out.ptr)
    m.synchronize()
    return out.check("k = %d" % k).cpu().numpy()


# ---- 1. FLAGS ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(CONFIGS))
def test_flags_mode_leaves_the_rows_and_decides_by_the_rule(pkg, orc, name):
    d = ragged()
    rows, y = twin_rows(pkg, orc, name)
    m, rows_m, total = planned(pkg, name)
    assert list(rows_m) == list(rows)
    for et, ms, ctx, p in cases(name):
        m.batch_set_vad(CONFIGS[name]["column"], et, ms, ctx, p, pkg.VAD_FLAGS)
        assert m.batch_output_width() == y.shape[1]
        got = m.batch_run_host(d["pcm"])
        assert same_bits(got, y), "FLAGS changed d_out"
        check_decision(name, y, rows, FRAMES, m.batch_vad_read(), et, ms, ctx, p, what="%s %s" % (name, (et, ms, ctx, p)))
    if name == "mfcc39cvn":                                          # NaNs met on the way: the one-frame utterance's row
        r9 = int(rows[SILENT])                                       # holds some, the silent utterance's column nothing else
        assert np.isnan(y[rows[0]]).any() and np.isnan(y[r9:r9 + FRAMES[SILENT], 12]).all()
        assert np.isnan(m.batch_vad_read()[2][SILENT]) and m.batch_vad_read()[1][SILENT] == 0
    m.close()


# ---- 2. SELECT and PACK --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(CONFIGS))
def test_select_and_pack_deliver_the_voiced_rows_and_zeros_inside_d_out(pkg, orc, name):
    d = ragged()
    rows, y = twin_rows(pkg, orc, name)
    m, _, total = planned(pkg, name)
    width = y.shape[1]
    for et, ms, ctx, p in cases(name):
        m.batch_set_vad(CONFIGS[name]["column"], et, ms, ctx, p, pkg.VAD_SELECT)
        got = run_placed(m, d["pcm"], total, width, k=1)
        dec = m.batch_vad_read()
        check_decision(name, y, rows, FRAMES, dec, et, ms, ctx, p, what="select")
        flags = dec[0]
        want = VR.select_ref(y, rows, FRAMES, flags)
        assert same_bits(got, want), "SELECT %s %s" % (name, (et, ms, ctx, p))
        m.batch_set_vad(CONFIGS[name]["column"], et, ms, ctx, p, pkg.VAD_PACK)
        got = run_placed(m, d["pcm"], total, width, k=3)
        dec2 = m.batch_vad_read()
        assert np.array_equal(dec2[0], flags) and same_bits(dec2[2], dec[2]) and dec2[3] == int(flags.sum())
        want, row0 = VR.pack_ref(y, rows, FRAMES, flags)
        assert same_bits(got, want), "PACK %s %s" % (name, (et, ms, ctx, p))
        assert row0[-1] == dec2[3] and all(ptr != 0 for ptr in m.batch_vad_device())
    # the aligned (16-byte) form of the row move gives the same bits as the word form above
    if width % 4 == 0:
        assert same_bits(run_placed(m, d["pcm"], total, width, k=0), want)
    m.close()


# ---- 3. with a transform ---------------------------------------------------------------------------------------------

def test_a_transform_in_force_is_selected_from_and_does_not_move_the_decision(pkg, orc):
    d = ragged()
    rows, y = twin_rows(pkg, orc, "mfcc39")
    rng = np.random.default_rng(11)
    A = (rng.standard_normal((24, 4 * 39)) / np.sqrt(4 * 39)).astype(np.float32)
    b = rng.standard_normal(24).astype(np.float32)
    t, _, total = planned(pkg, "mfcc39")
    t.batch_set_transform(A, b, left=2, right=1)
    z = t.batch_run_host(d["pcm"])                                   # the transform twin
    t.close()
    for order in ("vad first", "transform first"):                   # (the row scratch follows the output width either way)
        m, _, _ = planned(pkg, "mfcc39")
        m.batch_set_vad(-1, 0.0, 1.0, 2, 0.6, pkg.VAD_FLAGS)
        m.batch_run_host(d["pcm"])
        plain = m.batch_vad_read()
        if order == "transform first":
            m.batch_set_transform(A, b, left=2, right=1)
        m.batch_set_vad(-1, 0.0, 1.0, 2, 0.6, pkg.VAD_SELECT)
        if order == "vad first":
            m.batch_set_transform(A, b, left=2, right=1)
        assert m.batch_output_width() == 24
        got = run_placed(m, d["pcm"], total, 24, k=1)
        dec = m.batch_vad_read()
        assert np.array_equal(dec[0], plain[0]) and same_bits(dec[2], plain[2]) and np.array_equal(dec[1], plain[1])
        assert same_bits(got, VR.select_ref(z, rows, FRAMES, dec[0])), order
        m.batch_set_vad(-1, 0.0, 1.0, 2, 0.6, pkg.VAD_PACK)
        assert same_bits(run_placed(m, d["pcm"], total, 24, k=2), VR.pack_ref(z, rows, FRAMES, dec[0])[0]), order
        m.close()


# ---- 4. same bits across runs and forms ------------------------------------------------------------------------------

def select_run(pkg, orc, name="mfcc39"):
    d = ragged()
    rows, y = twin_rows(pkg, orc, name)
    m, _, total = planned(pkg, name)
    m.batch_set_vad(-1, 0.0, 1.0, 2, 0.6, pkg.VAD_SELECT)
    got = m.batch_run_host(d["pcm"])
    dec = m.batch_vad_read()
    check_decision(name, y, rows, FRAMES, dec, 0.0, 1.0, 2, 0.6, what="base")
    assert same_bits(got, VR.select_ref(y, rows, FRAMES, dec[0]))
    return d, rows, y, m, total, got, dec


def same_decision(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and same_bits(a[2], b[2]) and a[3] == b[3]


def test_a_second_run_and_the_overlap_mode_give_the_same_bits(pkg, orc):
    import torch
    d, rows, y, m, total, got, dec = select_run(pkg, orc)
    assert same_bits(m.batch_run_host(d["pcm"]), got) and same_decision(m.batch_vad_read(), dec)
    m.synchronize()
    m.batch_overlap(True)
    dev = torch.device("cuda:0")
    pcm = torch.from_numpy(d["pcm"].copy()).to(dev)
    outs = [torch.full((total, 39), float("nan"), dtype=torch.float32, device=dev) for _ in range(3)]
    for o in outs:                                                   # three batches in flight
        m.batch_run_device(pcm.data_ptr(), pcm.numel(), o.data_ptr())
    m.synchronize()
    for i, o in enumerate(outs):
        assert same_bits(o.cpu().numpy(), got), "overlapped batch %d" % i
    assert same_decision(m.batch_vad_read(), dec)
    m.close()


def test_every_utterance_alone_gives_its_part_of_the_batch(pkg, orc):
    d, rows, y, m, total, got, dec = select_run(pkg, orc)
    m.close()
    one = make(pkg, "mfcc39")
    for u, (r0, T) in enumerate(zip(rows, FRAMES)):
        one.batch_plan([d["offs"][u]], [d["lens"][u]])
        one.batch_set_vad(-1, 0.0, 1.0, 2, 0.6, pkg.VAD_SELECT)     # (a plan clears the VAD)
        alone = one.batch_run_host(d["pcm"])
        a = one.batch_vad_read()
        assert same_bits(alone, got[r0:r0 + T]), "utterance %d (%d frames)" % (u, T)
        assert np.array_equal(a[0], dec[0][r0:r0 + T]) and same_bits(a[2], dec[2][u:u + 1]) and a[1][0] == dec[1][u] == a[3]
    one.close()


def test_a_speaker_list_in_force_composes(pkg, orc):
    d = ragged()
    input_condition(orc, "mfcc39cvn")
    spk = np.array([0, 1, 2, 0, 1, 2, 0, 1, 2, 0, 1], np.int32)
    t, rows, total = planned(pkg, "mfcc39cvn")
    t.batch_set_speakers(spk)
    y = t.batch_run_host(d["pcm"])                                   # the twin: pooled statistics, no VAD
    t.close()
    m, _, _ = planned(pkg, "mfcc39cvn")
    m.batch_set_speakers(spk)
    m.batch_set_vad(-1, 0.0, 1.0, 2, 0.6, pkg.VAD_SELECT)
    got = run_placed(m, d["pcm"], total, 39, k=1)
    dec = m.batch_vad_read()
    check_decision("mfcc39cvn", y, rows, FRAMES, dec, 0.0, 1.0, 2, 0.6, what="speakers")
    assert same_bits(got, VR.select_ref(y, rows, FRAMES, dec[0]))
    assert 0 < dec[3] < total
    m.close()


def test_a_rates_plan_composes(pkg, orc):
    input_condition(orc, "mfcc39")
    d = ragged()
    # utterance 7 arrives at 8 kHz: every second sample of it, the others as they are
    utts = [u[::2].copy() if i == 7 else u for i, u in enumerate(d["utts"])]
    rates = [8000 if i == 7 else 16000 for i in range(len(utts))]
    offs, pos = [], 0
    for u in utts:
        offs.append(pos)
        pos += u.size + (u.size & 1) + 2 * (len(offs) % 2)
    pcm = np.zeros(pos + 8, np.int16)
    for o_, u in zip(offs, utts):
        pcm[o_:o_ + u.size] = u
    lens = [u.size for u in utts]
    t = make(pkg, "mfcc39")
    rows, total = t.batch_plan_rates(offs, lens, rates)
    y = t.batch_run_host(pcm)
    t.close()
    frames = [int(b - a) for a, b in zip(rows, list(rows[1:]) + [total])]
    assert frames[7] >= 100 and frames[8] == 4200
    m = make(pkg, "mfcc39")
    m.batch_plan_rates(offs, lens, rates)
    m.batch_set_vad(-1, 0.0, 1.0, 2, 0.6, pkg.VAD_SELECT)
    got = run_placed(m, pcm, total, 39, k=1)
    dec = m.batch_vad_read()
    check_decision("mfcc39", y, rows, frames, dec, 0.0, 1.0, 2, 0.6, what="rates")
    assert same_bits(got, VR.select_ref(y, rows, frames, dec[0])) and 0 < dec[1][7] < frames[7]
    m.close()


def test_sliced_host_run_with_pinned_buffers_gives_the_same_bits(pkg, orc):
    """The smallest batch that takes the sliced path of mfx_batch_run_host: 8 utterances (two slices), 32 MB of PCM, pinned
    buffers; FLAGS and SELECT stay on it.  Against the same handle's run from pageable buffers (one piece), and PACK (which
    takes the unsliced path from pinned buffers too) against the reference layout."""
    input_condition(orc, "mfcc39")
    L = pkg.load_library()
    L.mfx_alloc_pinned.restype, L.mfx_alloc_pinned.argtypes = C.c_void_p, [C.c_size_t]
    L.mfx_free_pinned.restype, L.mfx_free_pinned.argtypes = None, [C.c_void_p]
    rng = np.random.default_rng(22)
    n_utt = 8
    lens = [int(v) for v in rng.integers(2100000, 2110000, size=n_utt)]
    offs, pos = [], 0
    for n in lens:
        offs.append(pos)
        pos += n + int(rng.integers(0, 5))
    assert pos * 2 >= 32 << 20
    gain = np.repeat(np.where(rng.random(pos // (S * 50) + 1) < 0.5, 1.0, QUIET), S * 50)[:pos]   # runs of 50 frames
    pcm = (3000.0 * rng.standard_normal(pos) * gain).astype(np.int16)
    m = make(pkg, "mfcc39")
    rows, total = m.batch_plan(offs, lens)
    frames = [(n - W) // S + 1 for n in lens]
    p_in, p_out = L.mfx_alloc_pinned(pos * 2), L.mfx_alloc_pinned(total * 39 * 4)
    assert p_in and p_out
    try:
        C.memmove(p_in, pcm.ctypes.data, pos * 2)

        def pinned_run():
            rc = L.mfx_batch_run_host(m._h, C.cast(p_in, C.POINTER(C.c_int16)), pos, C.cast(p_out, C.POINTER(C.c_float)))
            assert rc == 0, L.mfx_last_error(m._h)
            return np.ctypeslib.as_array(C.cast(p_out, C.POINTER(C.c_float)), shape=(total, 39)).copy()

        y = pinned_run()                                             # no VAD yet: the rows y, by the sliced path
        results = {}
        for mode in (pkg.VAD_FLAGS, pkg.VAD_SELECT, pkg.VAD_PACK):
            m.batch_set_vad(-1, 0.0, 1.0, 2, 0.6, mode)
            got = pinned_run()
            dec = m.batch_vad_read()
            assert same_bits(m.batch_run_host(pcm), got) and same_decision(m.batch_vad_read(), dec)   # pageable: one piece
            results[mode] = (got, dec)
    finally:
        L.mfx_free_pinned(p_in)
        L.mfx_free_pinned(p_out)
    m.close()
    dec = results[pkg.VAD_FLAGS][1]
    assert same_bits(results[pkg.VAD_FLAGS][0], y)
    for u in (0, 3, 4, 7):                                           # both slices
        r0, T = int(rows[u]), frames[u]
        e = y[r0:r0 + T, 12]
        want, bound = VR.thr_ref(e, 0.0, 1.0)
        assert abs(float(dec[2][u]) - want) <= bound
        assert np.array_equal(dec[0][r0:r0 + T], VR.flags_ref(e, dec[2][u], 2, 0.6)) and dec[1][u] == dec[0][r0:r0 + T].sum()
    assert 0.2 * total < dec[3] < 0.8 * total
    for mode in (pkg.VAD_SELECT, pkg.VAD_PACK):
        assert same_decision(results[mode][1], dec)
    assert same_bits(results[pkg.VAD_SELECT][0], VR.select_ref(y, rows, frames, dec[0]))
    assert same_bits(results[pkg.VAD_PACK][0], VR.pack_ref(y, rows, frames, dec[0])[0])


# ---- 5. clearing -----------------------------------------------------------------------------------------------------

def test_clearing_and_replanning_restore_the_twins_bits(pkg, orc):
    d, rows, y, m, total, got, dec = select_run(pkg, orc)
    assert not same_bits(got, y)
    m.batch_clear_vad()
    assert same_bits(m.batch_run_host(d["pcm"]), y)
    with pytest.raises(pkg.MfxError) as ei:
        m.batch_vad_read()
    assert ei.value.status == -8
    assert m._L.mfx_batch_vad_device(m._h, None, None, None) == -8
    m.batch_set_vad(-1, 0.0, 1.0, 2, 0.6, pkg.VAD_PACK)
    with pytest.raises(pkg.MfxError) as ei:                          # in force, but no run yet
        m.batch_vad_read()
    assert ei.value.status == -8
    m.batch_plan(d["offs"], d["lens"])                               # a new plan drops it too
    assert same_bits(m.batch_run_host(d["pcm"]), y)
    with pytest.raises(pkg.MfxError) as ei:
        m.batch_vad_read()
    assert ei.value.status == -8
    m.batch_clear_vad()                                              # (clearing twice is fine)
    m.close()


# ---- 6. errors -------------------------------------------------------------------------------------------------------

def test_refused_calls_leave_the_handle_usable(pkg, orc):
    d = ragged()
    rows, y = twin_rows(pkg, orc, "mfcc39")
    m = make(pkg, "mfcc39")
    raw = lambda *a: m._L.mfx_batch_set_vad(m._h, *a)
    assert raw(-1, 0.0, 1.0, 2, 0.6, 0) == -8                        # MFX_ERR_STATE: no plan yet
    m.batch_plan(d["offs"], d["lens"])
    inf, nan = float("inf"), float("nan")
    for args in [(-2, 0.0, 1.0, 2, 0.6, 0), (39, 0.0, 1.0, 2, 0.6, 0),                      # column outside [-1, Wd)
                 (-1, 0.0, 1.0, -1, 0.6, 0), (-1, 0.0, 1.0, 65, 0.6, 0),                     # frames_context outside 0 .. 64
                 (-1, 0.0, 1.0, 2, 0.0, 0), (-1, 0.0, 1.0, 2, -0.5, 0), (-1, 0.0, 1.0, 2, 1.001, 0), (-1, 0.0, 1.0, 2, nan, 0),
                 (-1, inf, 1.0, 2, 0.6, 0), (-1, nan, 1.0, 2, 0.6, 0), (-1, 0.0, -inf, 2, 0.6, 0), (-1, 0.0, nan, 2, 0.6, 0),
                 (-1, 0.0, 1.0, 2, 0.6, 3), (-1, 0.0, 1.0, 2, 0.6, -1)]:                     # unknown mode
        assert raw(*args) == -7, args
    assert raw(38, 0.0, 1.0, 64, 1.0, 0) == 0 and raw(0, 0.0, 1.0, 0, 0.6, 2) == 0          # the corners are accepted
    m.batch_clear_vad()
    assert same_bits(m.batch_run_host(d["pcm"]), y)                  # a refused call changes nothing
    m.batch_set_vad(-1, 0.0, 1.0, 2, 0.6, pkg.VAD_FLAGS)
    assert raw(-1, 0.0, 1.0, 2, 0.6, 9) == -7                        # ... nor does it end a VAD in force
    m.batch_run_host(d["pcm"])
    check_decision("mfcc39", y, rows, FRAMES, m.batch_vad_read(), 0.0, 1.0, 2, 0.6, what="after refused calls")
    m.close()


# ---- 7. the driver ---------------------------------------------------------------------------------------------------

def read_htk(path):
    raw = open(path, "rb").read()
    n, period, size, kind = struct.unpack(">iihh", raw[:12])
    return n, size, kind, np.frombuffer(raw[12:], ">f4").astype(np.float32).reshape(-1, size // 4)


def test_driver_writes_the_voiced_rows_and_is_unchanged_without_vad(pkg, orc, tmp_path):
    exe = os.path.join(ROOT, "asr-featext-opencl_amd", "host", "afet_hip")
    assert os.path.exists(exe), "afet_hip is built by build()"
    wavs = []
    for i in range(3):
        dst = tmp_path / ("u%d.wav" % i)
        dst.write_bytes(open(os.path.join(GOLDEN, "a0001.wav" if i != 1 else "a1.wav"), "rb").read())
        wavs.append(str(dst))
    shape = ["--banks", "40", "--ceps", "12", "--c0", "1", "--norm", "0", "--dyn", "2", "--low-freq", "64", "--high-freq", "8000",
             "--bug-compat", "0", "--htk", "--batch-mb", "64"]
    vad = ["--vad-energy-threshold", "0", "--vad-energy-mean-scale", "1", "--vad-frames-context", "2",
           "--vad-proportion-threshold", "0.6"]

    def run(tag, *extra):
        out = tmp_path / tag
        out.mkdir()
        outs = [str(out / ("u%d.htk" % i)) for i in range(len(wavs))]
        pairs = [x for pair in zip(wavs, outs) for x in pair]
        r = subprocess.run([exe, *shape, *extra, *pairs], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
        assert r.returncode == 0, r.stdout[-2000:]
        return outs

    plain = run("plain")
    voiced = run("vad", "--vad", *vad)
    again = run("plain2", *vad, "--vad-column", "3")                 # VAD options without --vad: nothing changes
    for a, b in zip(plain, again):
        assert open(a, "rb").read() == open(b, "rb").read()
    # the same files through the Python binding: the driver's batch (even offsets, its kernels), SELECT
    pcms = [orc.read_wav_pcm16(w) for w in wavs]
    sr = pcms[0][1]
    assert all(p[1] == sr and p[0].shape[1] == 1 for p in pcms)
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
    y = m.batch_run_host(pcm)
    m.batch_set_vad(-1, 0.0, 1.0, 2, 0.6, pkg.VAD_SELECT)
    sel = m.batch_run_host(pcm)
    flags, cnt, thr, total_voiced = m.batch_vad_read()
    m.close()
    assert 0 < total_voiced < total
    for u, (a, b) in enumerate(zip(plain, voiced)):
        n, size, kind, full = read_htk(a)
        nv, size_v, kind_v, got = read_htk(b)
        r0 = int(rows[u])
        assert same_bits(full, y[r0:r0 + n]) and n == full.shape[0]  # (the binding reproduces the driver's rows)
        assert (size_v, kind_v) == (size, kind) and nv == got.shape[0] == int(cnt[u])
        assert same_bits(got, sel[r0:r0 + nv]) and same_bits(got, full[flags[r0:r0 + n].astype(bool)])
