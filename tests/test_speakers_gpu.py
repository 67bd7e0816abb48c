"""Per-speaker CMN / CVN / MINMAX of the batch entries (mfx_batch_set_speakers) on the MI355X, against tests/spk_ref.py: a
speaker's statistics within tail_ref.norm_stats_ref's bounds of the pooled rows of the norm = NONE twin (no factor on top),
every normalised row bit for bit tail_ref.norm_apply_f32 of the twin's rows with the handle's own statistics; singletons
against the per-utterance normaliser bit for bit; independence, carry, composition with the other batch features, state.
"""
import ctypes as C
import os
import subprocess
import wave

import numpy as np
import pytest

import spk_ref
import xform_ref as XR
from conftest import synth_utterance
from tail_ref import assert_tail_consistent, same_bits

pytestmark = pytest.mark.gpu

W, S = 400, 160
L1, L2 = 2, 3
FRAMES = [1, 2, 7, 64, 65, 200, 4097, 8200]         # the last two cross the 4096-row chunk once and twice
SHAPES = {"13x3": (13, 2), "1x3": (1, 2), "13": (13, 0), "traps256x3": (256, 2)}
KINDS = {1: "cmn", 2: "cvn", 3: "minmax"}


def make(pkg, shape, norm=0, nad=True, bns=0, engine=0, ibs=200000):
    cols, dyn = SHAPES[shape]
    if shape.startswith("traps"):
        m = pkg.MfccHip(ibs, W, S, 16, 16000.0, 64.0, 8000.0, 0, False, 22.0, norm, dyn, L1, L2, nad, device=0, bug_compat=False,
                        batch_norm_stats=bns, method=pkg.METHOD_TRAPS, traps_len=31, traps_dct_len=16, engine=engine)
    else:
        m = pkg.MfccHip(ibs, W, S, 26, 16000.0, 64.0, 8000.0, cols, False, 22.0, norm, dyn, L1, L2, nad, device=0,
                        bug_compat=False, batch_norm_stats=bns, engine=engine)
    assert m.get_output_data_width() == cols * (1 + dyn)
    m.set_window(pkg.reference_window(W))
    return m


def samples_for(frames):
    return W - S + frames * S + 36 if frames > 0 else 0


_utts = {}


def utt(frames, seed):
    key = (frames, seed)
    if key not in _utts:
        _utts[key] = synth_utterance(samples_for(frames), 700 + seed)
    return _utts[key]


def common_utts():
    """The eight frame counts, then the zero-sample utterance."""
    return [utt(t, i) for i, t in enumerate(FRAMES)] + [np.zeros(0, np.int16)], FRAMES + [0]


def layout(utts):
    lens = [u.size for u in utts]
    offs, pos = [], 0
    for n in lens:
        offs.append(pos)
        pos += n + (n & 1)
    pcm = np.zeros(pos + 2, np.int16)
    for o, u in zip(offs, utts):
        pcm[o:o + u.size] = u
    return offs, lens, pcm


def run(m, utts, spk=None, n_spk=None, prior=None, mode=0, setup=None):
    """Plan, (setup), set the list, run: the rows per utterance, and (count, acc, stats) when a list is in force."""
    offs, lens, pcm = layout(utts)
    rows, total = m.batch_plan(offs, lens)
    if setup:
        setup(m)
    if spk is not None:
        m.batch_set_speakers(spk, n_spk, prior=prior, mode=mode)
    out = m.batch_run_host(pcm)
    per = [out[rows[i]:rows[i] + m.batch_frames(lens[i])] for i in range(len(utts))]
    return per, (m.batch_speaker_stats() if spk is not None else None)


_twins = {}


def twin_rows(pkg, shape, key, utts, setup=None):
    if (shape, key) not in _twins:
        t = make(pkg, shape, norm=0)
        _twins[(shape, key)] = run(t, utts, setup=setup)[0]
        t.close()
    return _twins[(shape, key)]


def check_speakers(ys, xs, stats, spk, n_spk, kind, nad, shape, what, prior_rows=None, need_all=True):
    """Every speaker with rows against spk_ref; the delta groups of rows normalised before the deltas against tail_ref."""
    cols, dyn = SHAPES[shape]
    worst = [0.0, 0.0]
    for s in range(n_spk):
        mine = [u for u in range(len(ys)) if spk[u] == s]
        pri = [] if prior_rows is None else prior_rows.get(s, [])
        if sum(xs[u].shape[0] for u in mine) + sum(p.shape[0] for p in pri) == 0:
            continue
        wm, wk, keep = spk_ref.assert_speaker_consistent([ys[u] for u in mine], [xs[u] for u in mine], stats[s], kind, cols, prior=pri,
                                                         what="%s, speaker %d" % (what, s))
        worst = [max(worst[0], wm), max(worst[1], wk)]
        if need_all:
            assert keep.all(), "%s, speaker %d: columns left out: %s" % (what, s, np.argwhere(~keep))
        if not nad and dyn == 2:
            for u in mine:
                k = keep[0]
                if k.any() and 0 < ys[u].shape[0] <= 300:   # (the long ones add nothing the short ones do not show)
                    sub = np.concatenate([ys[u][:, g * cols:(g + 1) * cols][:, k] for g in range(3)], 1)
                    assert_tail_consistent(sub, int(k.sum()), 2, L1, L2, "%s, utt %d (deltas of normalised statics)" % (what, u))
    print("%s: worst err / bound mean %.3g, multiplier %.3g" % (what, worst[0], worst[1]))
    return worst


# ---- 1. singletons: one speaker per utterance is the per-utterance normaliser over all T rows ------------------------

@pytest.mark.parametrize("kind", [1, 2, 3], ids=list(KINDS.values()))
@pytest.mark.parametrize("shape", list(SHAPES))
def test_singletons_equal_the_per_utterance_normaliser_bit_for_bit(pkg, shape, kind):
    cols, dyn = SHAPES[shape]
    utts, frames = common_utts()
    for nad in (False, True):
        m = make(pkg, shape, norm=kind, nad=nad, bns=1)
        want, _ = run(m, utts)
        G = (1 + dyn) if nad else 1
        st_want = m.debug_read(6).reshape(G, len(utts), 2, cols)
        got, (count, acc, stats) = run(m, utts, spk=np.arange(len(utts)), n_spk=len(utts))
        assert m.debug_read(6).size == 0                   # kind 6 has nothing to say while a list is in force
        m.close()
        assert stats.shape == (len(utts), 2, G * cols) and acc.shape == (len(utts), 4, G * cols)
        assert count.tolist() == frames
        for u, t in enumerate(frames):
            what = "%s %s nad %d, utt %d (%d frames)" % (shape, KINDS[kind], nad, u, t)
            assert got[u].shape == (t, cols * (1 + dyn)), what
            assert same_bits(got[u], want[u]), what + ": rows"
            if t > 0:
                st = stats[u].reshape(2, G, cols).transpose(1, 0, 2)
                if kind == 1:
                    st, ref = st[:, :1], st_want[:, u, :1]  # (CMN: the multiplier slot is not read)
                else:
                    ref = st_want[:, u]
                assert same_bits(st, ref), what + ": statistics"
    print("%s %s: rows and statistics of %d singletons equal the per-utterance normaliser's bits" % (shape, KINDS[kind], len(utts)))


# ---- 2. pooling ------------------------------------------------------------------------------------------------------

POOL_IDS = [0, 1, 2, 0, 2, 1, 0, 1, 2, 0, 2, 1]


def pool_utts():
    """12 utterances: the common nine (utterance 8 has no sample: speaker 2 holds it), then 33, 129 and 300 frames."""
    utts, frames = common_utts()
    more = [33, 129, 300]
    return utts + [utt(t, 20 + i) for i, t in enumerate(more)], frames + more


@pytest.mark.parametrize("kind", [1, 2, 3], ids=list(KINDS.values()))
@pytest.mark.parametrize("shape", list(SHAPES))
def test_pooled_statistics_within_bounds_and_rows_bit_for_bit(pkg, shape, kind):
    cols, dyn = SHAPES[shape]
    utts, frames = pool_utts()
    xs = twin_rows(pkg, shape, "pool", utts)
    for nad in (False, True):
        m = make(pkg, shape, norm=kind, nad=nad)
        ys, (count, acc, stats) = run(m, utts, spk=POOL_IDS, n_spk=4)       # speaker 3 has no utterance
        m.close()
        Wn = cols * (1 + dyn) if nad else cols
        assert stats.shape == (4, 2, Wn)
        assert count.tolist() == [sum(t for t, s in zip(frames, POOL_IDS) if s == k) for k in range(3)] + [0]
        assert not np.isfinite(stats[3, 0]).any()           # n = 0: 0 / 0, read by no row
        assert (acc[3, :2] == 0).all()
        for k in range(3):                                  # min and max are exact
            pooled = np.concatenate([xs[u][:, :Wn] for u in range(len(utts)) if POOL_IDS[u] == k])
            assert np.array_equal(acc[k, 2], pooled.min(0)) and np.array_equal(acc[k, 3], pooled.max(0))
        check_speakers(ys, xs, stats, POOL_IDS, 4, kind, nad, shape, "pooling, %s %s nad %d" % (shape, KINDS[kind], nad))


# ---- 3. independence -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind,nad", [(2, True), (3, False), (1, True)], ids=["cvn-after", "minmax-before", "cmn-after"])
def test_a_speakers_bits_do_not_depend_on_the_rest_of_the_batch(pkg, kind, nad):
    utts, frames = pool_utts()
    m = make(pkg, "13x3", norm=kind, nad=nad)
    base, (c0, a0, s0) = run(m, utts, spk=POOL_IDS, n_spk=4)
    # ids relabelled by a permutation
    perm = np.array([2, 3, 0, 1])
    got, (c1, a1, s1) = run(m, utts, spk=perm[POOL_IDS], n_spk=4)
    for u in range(len(utts)):
        assert same_bits(got[u], base[u]), "relabelled ids: utterance %d" % u
    assert same_bits(s1[perm[:3]], s0[:3]) and np.array_equal(a1[perm[:3]], a0[:3]) and np.array_equal(c1[perm], c0)
    # utterances of new speakers appended (and one put in front)
    extra = [utt(50, 40), utt(4100, 41), utt(3, 42)]
    got, _ = run(m, extra[:1] + utts + extra[1:], spk=[5] + POOL_IDS + [4, 6], n_spk=7)
    for u in range(len(utts)):
        assert same_bits(got[1 + u], base[u]), "appended speakers: utterance %d" % u
    # one speaker's utterances alone
    for k in range(3):
        mine = [u for u in range(len(utts)) if POOL_IDS[u] == k]
        got, (c2, a2, s2) = run(m, [utts[u] for u in mine], spk=[0] * len(mine), n_spk=1)
        for i, u in enumerate(mine):
            assert same_bits(got[i], base[u]), "speaker %d alone: utterance %d" % (k, u)
        assert same_bits(s2[0], s0[k]) and np.array_equal(a2[0], a0[k]) and c2[0] == c0[k]
    m.close()


# ---- 4. carry --------------------------------------------------------------------------------------------------------

CARRY_FRAMES = [64, 4097, 7, 200, 8200, 65]
CARRY_IDS = [0, 1, 0, 1, 1, 0]


@pytest.mark.parametrize("kind,nad", [(2, True), (3, False)], ids=["cvn-after", "minmax-before"])
def test_accumulators_carried_into_the_next_batch_give_the_one_batch_bits(pkg, kind, nad):
    utts = [utt(t, 60 + i) for i, t in enumerate(CARRY_FRAMES)]
    m = make(pkg, "13x3", norm=kind, nad=nad)
    one, (c1, a1, s1) = run(m, utts, spk=CARRY_IDS, n_spk=2)
    for k in range(1, 6):
        _, (ca, aa, _) = run(m, utts[:k], spk=CARRY_IDS[:k], n_spk=2)
        rows_b, (cb, ab, sb) = run(m, utts[k:], spk=CARRY_IDS[k:], n_spk=2, prior=(ca, aa))
        assert np.array_equal(cb, c1) and np.array_equal(ab, a1) and same_bits(sb, s1), "split at %d: accumulators / statistics" % k
        for i, u in enumerate(range(k, 6)):
            assert same_bits(rows_b[i], one[u]), "split at %d: utterance %d of batch B" % (k, u)
        rows_a, (cp, ap, sp) = run(m, utts[:k], spk=CARRY_IDS[:k], n_spk=2, prior=(cb, ab), mode=pkg.mfcc.SPK_PRIOR_ONLY)
        assert np.array_equal(cp, c1) and np.array_equal(ap, a1) and same_bits(sp, s1), "split at %d: PRIOR_ONLY read-back" % k
        for u in range(k):
            assert same_bits(rows_a[u], one[u]), "split at %d: utterance %d of batch A under PRIOR_ONLY" % (k, u)
    m.close()


@pytest.mark.parametrize("kind,nad", [(2, True), (3, False)], ids=["cvn-after", "minmax-before"])
def test_two_ranks_merged_on_the_host_then_prior_only(pkg, kind, nad):
    utts = [utt(t, 60 + i) for i, t in enumerate(CARRY_FRAMES)]
    xs = twin_rows(pkg, "13x3", "carry", utts)
    m = make(pkg, "13x3", norm=kind, nad=nad)
    halves = [list(range(r, 6, 2)) for r in range(2)]       # sharding.shard_indices: round-robin
    parts = []
    for idx in halves:
        _, (c, a, _) = run(m, [utts[u] for u in idx], spk=[CARRY_IDS[u] for u in idx], n_spk=2)
        parts.append((c, a))
    count, acc = pkg.sharding.merge_speaker_acc(parts)
    assert count.tolist() == [sum(t for t, s in zip(CARRY_FRAMES, CARRY_IDS) if s == k) for k in range(2)]
    ys, stats = [None] * 6, None
    for idx in halves:
        rows, (c, a, st) = run(m, [utts[u] for u in idx], spk=[CARRY_IDS[u] for u in idx], n_spk=2, prior=(count, acc),
                               mode=pkg.mfcc.SPK_PRIOR_ONLY)
        assert np.array_equal(c, count) and np.array_equal(a, acc)
        assert stats is None or same_bits(st, stats)
        stats = st
        for i, u in enumerate(idx):
            ys[u] = rows[i]
    m.close()
    check_speakers(ys, xs, stats, CARRY_IDS, 2, kind, nad, "13x3", "two ranks merged, %s nad %d" % (KINDS[kind], nad))


# ---- 5. degenerate statistics ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("nad", [False, True], ids=["before", "after"])
def test_degenerate_speakers_under_cvn(pkg, nad):
    """Speaker 0: a single 1-frame utterance (0 / 0, or 0 over the rounding error of one float32 square).  Speaker 1: 40 frames
    of silence (identical rows: the deltas' variance is exactly 0).  Speaker 2: ordinary.  spk_ref requires the non-finite
    columns to be the same on both sides; they are the only ones left out."""
    utts = [utt(1, 80), np.zeros(samples_for(40), np.int16), utt(64, 81), utt(200, 82)]
    ids = [0, 1, 2, 2]
    xs = twin_rows(pkg, "13x3", "degenerate", utts)
    m = make(pkg, "13x3", norm=2, nad=nad)
    ys, (count, acc, stats) = run(m, utts, spk=ids, n_spk=3)
    m.close()
    assert count.tolist() == [1, 40, 264]
    assert (~np.isfinite(stats[0, 1]) | (stats[0, 1] == 0)).all()
    if nad:
        assert not np.isfinite(stats[1, 1, 13:]).any()      # deltas of identical frames: (n - 1) / 0
    check_speakers(ys, xs, stats, ids, 3, 2, nad, "13x3", "degenerate, nad %d" % nad, need_all=False)
    cols = 13
    _, _, keep = spk_ref.assert_speaker_consistent([ys[2], ys[3]], [xs[2], xs[3]], stats[2], 2, cols, what="ordinary speaker")
    assert keep.all()


# ---- 6. composition with the other features of the batch entries ------------------------------------------------------

COMP_FRAMES = [7, 64, 200, 65, 2]
COMP_IDS = [0, 1, 0, 1, 0]


def comp_utts():
    return [utt(t, 90 + i) for i, t in enumerate(COMP_FRAMES)]


def test_with_an_alpha_list(pkg):
    alphas = np.array([0.9, 1.1, 1.0, 0.9, 1.1], np.float32)
    setup = lambda h: h.batch_set_alphas(alphas)
    utts = comp_utts()
    xs = twin_rows(pkg, "13x3", "alphas", utts, setup=setup)
    m = make(pkg, "13x3", norm=2)
    ys, (_, _, stats) = run(m, utts, spk=COMP_IDS, n_spk=2, setup=setup)
    m.close()
    assert not same_bits(xs[0], twin_rows(pkg, "13x3", "plain", utts)[0])       # the list did warp
    check_speakers(ys, xs, stats, COMP_IDS, 2, 2, True, "13x3", "with an alpha list")


def test_with_a_rates_plan_8k_to_16k(pkg):
    utts = [synth_utterance(samples_for(t) // 2 + 40, 95 + i, sr=8000.0) for i, t in enumerate(COMP_FRAMES)]
    offs, lens, pcm = layout(utts)

    def go(h, spk):
        rows, total = h.batch_plan_rates(offs, lens, [8000] * len(utts))
        if spk:
            h.batch_set_speakers(COMP_IDS, 2)
        out = h.batch_run_host(pcm)
        _, conv, _ = h.batch_resample_layout()
        return [out[rows[i]:rows[i] + h.batch_frames(conv[i])] for i in range(len(utts))]

    t = make(pkg, "13x3", norm=0)
    xs = go(t, False)
    t.close()
    m = make(pkg, "13x3", norm=2)
    ys = go(m, True)
    stats = m.batch_speaker_stats()[2]
    m.close()
    assert sum(x.shape[0] for x in xs) > 300
    check_speakers(ys, xs, stats, COMP_IDS, 2, 2, True, "13x3", "with a rates plan")


def test_overlap_mode_and_fused_delta_give_the_same_bits(pkg):
    utts = comp_utts() + [utt(4097, 99)]
    ids = COMP_IDS + [1]
    m = make(pkg, "13x3", norm=2)
    base, (_, a0, s0) = run(m, utts, spk=ids, n_spk=2)
    m.batch_overlap(True)
    offs, lens, pcm = layout(utts)
    for _ in range(3):                                       # both scratch buffers re-used
        out = m.batch_run_host(pcm)                          # (ends with mfx_synchronize)
    rows = m._plan_rows
    for u in range(len(utts)):
        assert same_bits(out[rows[u]:rows[u] + base[u].shape[0]], base[u]), "overlap: utterance %d" % u
    assert same_bits(m.batch_speaker_stats()[2], s0)
    m.close()
    f = make(pkg, "13x3", norm=2, engine=pkg.mfcc.ENGINE_FUSE_DELTA)
    got, (_, a1, s1) = run(f, utts, spk=ids, n_spk=2)
    f.close()
    for u in range(len(utts)):
        assert same_bits(got[u], base[u]), "fused delta: utterance %d" % u
    assert same_bits(s1, s0) and np.array_equal(a1, a0)


def test_with_a_transform(pkg):
    utts = comp_utts()
    m = make(pkg, "13x3", norm=2)
    y, _ = run(m, utts, spk=COMP_IDS, n_spk=2)
    ycat = np.concatenate(y)
    assert np.isfinite(ycat).all()
    eye = np.eye(39, dtype=np.float32)
    got, _ = run(m, utts, spk=COMP_IDS, n_spk=2, setup=lambda h: h.batch_set_transform(eye))
    assert np.array_equal(np.concatenate(got), ycat), "identity transform: values differ from the normalised rows"
    rng = np.random.default_rng(3)
    A = (rng.standard_normal((20, 5 * 39)) / np.sqrt(5 * 39)).astype(np.float32)
    b = rng.standard_normal(20).astype(np.float32)
    got, _ = run(m, utts, spk=COMP_IDS, n_spk=2, setup=lambda h: h.batch_set_transform(A, b, left=2, right=2))
    m.close()
    rows = np.concatenate([[0], np.cumsum(COMP_FRAMES)[:-1]])
    XR.assert_xform_consistent(np.concatenate(got), ycat, rows, COMP_FRAMES, A, b, 2, 2, what="splice 2 + 2 over speaker-normalised rows")


def test_pinned_host_run_of_a_batch_that_would_be_sliced_equals_the_device_entry(pkg):
    """8 utterances, 32 MB of PCM, ascending offsets, pinned buffers: without a list this batch takes the sliced path of
    mfx_batch_run_host; with one it goes through whole (speakers span the slices) and gives the device entry's bits."""
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
    ids = np.arange(n_utt) % 3
    m = make(pkg, "13x3", norm=2)
    rows, total = m.batch_plan(offs, lens)
    m.batch_set_speakers(ids, 3)
    p_in, p_out = L.mfx_alloc_pinned(pos * 2), L.mfx_alloc_pinned(total * 39 * 4)
    assert p_in and p_out
    try:
        for u in range(n_utt):
            C.memmove(p_in + 2 * offs[u], one.ctypes.data, one.size * 2)
        rc = L.mfx_batch_run_host(m._h, C.cast(p_in, C.POINTER(C.c_int16)), pos, C.cast(p_out, C.POINTER(C.c_float)))
        assert rc == 0, L.mfx_last_error(m._h)
        got = np.ctypeslib.as_array(C.cast(p_out, C.POINTER(C.c_float)), shape=(total, 39)).copy()
        s_host = m.batch_speaker_stats()[2]
        dev = torch.device("cuda:0")
        pcm = torch.from_numpy(np.ctypeslib.as_array(C.cast(p_in, C.POINTER(C.c_int16)), shape=(pos,)).copy()).to(dev)
    finally:
        L.mfx_free_pinned(p_in)
        L.mfx_free_pinned(p_out)
    out = torch.full((total, 39), float("nan"), dtype=torch.float32, device=dev)
    m.batch_run_device(pcm.data_ptr(), pcm.numel(), out.data_ptr())
    m.synchronize()
    assert same_bits(out.cpu().numpy(), got)
    assert same_bits(m.batch_speaker_stats()[2], s_host)
    m.close()
    assert np.isfinite(got).all() and not same_bits(got[rows[0]:rows[0] + 100], got[rows[1]:rows[1] + 100])


# ---- 7. state and errors ---------------------------------------------------------------------------------------------

def status_of(fn, *args, **kw):
    try:
        fn(*args, **kw)
        return 0
    except Exception as e:                                   # MfxError (the package is loaded under an alias)
        return e.status


def raw_set(m, ids, n_utt, n_spk, count=None, acc=None, mode=0):
    ids = None if ids is None else np.ascontiguousarray(ids, np.int32)
    count = None if count is None else np.ascontiguousarray(count, np.int64)
    acc = None if acc is None else np.ascontiguousarray(acc, np.float64)
    return m._L.mfx_batch_set_speakers(m._h, None if ids is None else ids.ctypes.data_as(C.POINTER(C.c_int32)), n_utt, n_spk,
                                       None if count is None else count.ctypes.data_as(C.POINTER(C.c_int64)),
                                       None if acc is None else acc.ctypes.data_as(C.POINTER(C.c_double)), mode)


def test_refused_calls_and_state_rules(pkg):
    ARG, STATE, CONFIG = -7, -8, -5
    utts = comp_utts() + [np.zeros(0, np.int16)]
    ids = COMP_IDS + [2]
    n = len(utts)
    plain = make(pkg, "13x3", norm=0)
    plain.batch_plan(*layout(utts)[:2])
    assert raw_set(plain, ids, n, 3) == CONFIG and raw_set(plain, None, 0, 0) == CONFIG
    plain.close()

    ref = make(pkg, "13x3", norm=2, bns=1)
    never, _ = run(ref, utts)                                # a handle that never had a list
    ref.close()

    m = make(pkg, "13x3", norm=2, bns=1)
    assert raw_set(m, ids, n, 3) == STATE                    # before a plan
    assert m._L.mfx_batch_speaker_stats(m._h, None, None, None) == STATE
    offs, lens, pcm = layout(utts)
    m.batch_plan(offs, lens)
    assert m._L.mfx_batch_speaker_stats(m._h, None, None, None) == STATE        # no list
    Wn = 39
    cnt, acc = np.ones(3, np.int64), np.zeros((3, 4, Wn))
    assert raw_set(m, ids, n - 1, 3) == ARG                  # not the planned count
    assert raw_set(m, None, n, 3) == ARG
    assert raw_set(m, [0, 1, 0, 1, 3, 2], n, 3) == ARG       # an id outside [0, n_spk)
    assert raw_set(m, [0, 1, 0, -1, 0, 2], n, 3) == ARG
    assert raw_set(m, ids, n, 0) == ARG and raw_set(m, ids, n, (1 << 20) + 1) == ARG
    assert raw_set(m, ids, n, 3, count=cnt) == ARG and raw_set(m, ids, n, 3, acc=acc) == ARG   # one of the two prior arrays
    assert raw_set(m, ids, n, 3, count=[1, -1, 1], acc=acc) == ARG
    assert raw_set(m, ids, n, 3, mode=1) == ARG              # PRIOR_ONLY without a prior
    assert raw_set(m, ids, n, 3, count=[5, 0, 5], acc=acc, mode=1) == ARG       # speaker 1 has rows and a prior of count 0
    assert raw_set(m, ids, n, 3, count=[5, 5, 0], acc=acc, mode=1) == 0         # speaker 2 holds only the frameless utterance
    assert raw_set(m, ids, n, 3, mode=2) == ARG
    # every refusal left the handle without a list (the accepted call set one: clear it) and on the old bits
    assert raw_set(m, None, 0, 0) == 0
    assert m._L.mfx_batch_speaker_stats(m._h, None, None, None) == STATE
    got = m.batch_run_host(pcm)
    assert same_bits(got, np.concatenate(never))
    # a list: STATE before a run, fine after; any output may be NULL
    m.batch_set_speakers(ids, 3)
    assert status_of(m.batch_speaker_stats) == STATE
    with_list = m.batch_run_host(pcm)
    assert not same_bits(with_list, got)
    assert m._L.mfx_batch_speaker_stats(m._h, None, None, None) == 0
    count, acc1, stats = m.batch_speaker_stats()
    assert count.tolist() == [7 + 200 + 2, 64 + 65, 0]
    # streaming calls on the same handle are unaffected, and leave the list alone
    s_ref = make(pkg, "13x3", norm=2, bns=1)
    want_stream = s_ref.process_stream(utts[2])
    assert status_of(s_ref.sessions_create, 2, 4000) == status_of(m.sessions_create, 2, 4000)
    assert status_of(s_ref.sessions_plan, [0], [0], [1000]) == status_of(m.sessions_plan, [0], [0], [1000])
    s_ref.close()
    assert same_bits(m.process_stream(utts[2]), want_stream)
    assert same_bits(m.batch_run_host(pcm), with_list)
    # cleared by NULL / 0
    m.batch_set_speakers(None)
    assert same_bits(m.batch_run_host(pcm), got) and m.debug_read(6).size == 3 * n * 2 * 13
    assert status_of(m.batch_speaker_stats) == STATE
    # cleared by a new plan
    m.batch_set_speakers(ids, 3)
    assert same_bits(m.batch_run_host(pcm), with_list)
    m.batch_plan(offs, lens)
    assert same_bits(m.batch_run_host(pcm), got)
    assert status_of(m.batch_speaker_stats) == STATE
    m.close()


# ---- 8. the driver ---------------------------------------------------------------------------------------------------

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


def test_driver_spk_file_two_passes_equal_the_binding(pkg, a0001, tmp_path):
    """Six copies / cuts of a0001.wav in two speakers; --batch-mb 1 holds 524 288 samples, which the fifth file crosses:
    two batches (5 + 1 files), the second carrying the first's accumulators.  The rows the driver writes are the rows of ONE
    batch of all six through the binding (the carry property): same kernels (MFX_ENGINE_STREAM_KERNELS), same bits."""
    exe = exe_path()
    cuts = [a0001.size, a0001.size, a0001.size, 100000, a0001.size, 80000]
    assert sum(c + 22 for c in cuts[:4]) < 524288 <= sum(c + 22 for c in cuts[:5])
    labels = ["alice", "bob", "alice", "bob", "bob", "alice"]
    pcms = [a0001[i * 500:i * 500 + c].copy() if c < a0001.size else a0001 for i, c in enumerate(cuts)]
    args = []
    for i, p in enumerate(pcms):
        write_wav(tmp_path / ("in%d.wav" % i), p)
        args += [str(tmp_path / ("in%d.wav" % i)), str(tmp_path / ("out%d.htk" % i))]
    spk_file = tmp_path / "spk.txt"
    spk_file.write_text("\n".join(labels) + "\n")
    opts = ["--banks", "40", "--ceps", "13", "--c0", "0", "--norm", "2", "--dyn", "2", "--htk", "--batch-mb", "1"]
    subprocess.check_call([exe] + opts + ["--spk-file", str(spk_file)] + args, stdout=subprocess.DEVNULL)
    m = pkg.MfccHip(10000000, W, S, 40, 16000.0, 64.0, 8000.0, 13, False, 22.0, pkg.NORM_CVN, pkg.DYN_ACC, 3, 3, True, device=0,
                    engine=pkg.mfcc.ENGINE_STREAM_KERNELS)
    m.set_window(pkg.reference_window(W))
    ids = [0, 1, 0, 1, 1, 0]
    want, _ = run(m, pcms, spk=ids, n_spk=2)
    per_utt, _ = run(m, pcms)
    m.close()
    for i in range(6):
        got = read_htk(tmp_path / ("out%d.htk" % i))
        assert got.shape == want[i].shape
        assert same_bits(got, want[i]), "file %d" % i
        assert not same_bits(got, per_utt[i])                # (not the per-utterance normaliser's rows)
    # refusals that need the files: a file that would take the per-file loop
    short = tmp_path / "short.wav"
    write_wav(short, a0001[:W + 5 * S])                      # 6 frames < 2 D + 1
    one = tmp_path / "one.txt"
    one.write_text("alice\n")
    r = subprocess.run([exe] + opts + ["--spk-file", str(one), str(short), str(tmp_path / "short.htk")], stdout=subprocess.DEVNULL,
                       stderr=subprocess.PIPE, text=True)
    assert r.returncode != 0 and "per-file loop" in r.stderr
    for extra, word in ((["--batch-mb", "0"], "--batch-mb"), (["--devs", "0,0"], "one device")):
        r = subprocess.run([exe] + opts + extra + ["--spk-file", str(spk_file)] + args, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE,
                           text=True)
        assert r.returncode != 0 and word in r.stderr
