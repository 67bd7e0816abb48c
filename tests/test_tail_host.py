"""tests/tail_ref.py earns its trust here, on the CPU: the float32 oracle's rows, the committed vectors of the real
reference and the oracle's normaliser all pass it, and each of seven deliberate mistakes that the 1e-4 end-to-end bar
cannot see fails it.  No GPU."""
import os

import numpy as np
import pytest

import refcases
import tail_ref
from conftest import GOLDEN, synth_utterance
from tail_ref import assert_norm_consistent, assert_tail_consistent, delta_ref

W, S = 400, 160

# (dyn, l1, l2, cols): the five shapes of the first CPU experiment, then orders up to 10
SHAPES = [(2, 3, 3, 13), (2, 1, 2, 13), (2, 4, 1, 12), (1, 2, 2, 13), (2, 2, 4, 23),
          (2, 10, 10, 13), (2, 8, 8, 13), (1, 10, 0, 12), (2, 5, 10, 23), (2, 10, 1, 13)]


def cfg_for(orc, dyn, l1, l2, cols, norm=0, nad=True, ibs=10000000):
    return orc.make_config(ibs, window_size=W, shift=S, num_banks=26, ceps_len=cols, dyn=dyn, delta_l1=l1,
                           delta_l2=max(l2, 1), norm=norm, norm_after_dyn=nad)


def samples_for(frames):
    return W - S + frames * S + 36


@pytest.fixture(scope="module")
def pcm50k():
    return synth_utterance(50000, 5)


def oracle_rows(orc, pcm, dyn, l1, l2, cols, block=0):
    return orc.run_utterance(cfg_for(orc, dyn, l1, l2, cols), pcm, bug_compat=False, block_samples=block)


# ---- 1. the oracle's rows pass ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("dyn,l1,l2,cols", SHAPES)
def test_oracle_rows_pass(orc, pcm50k, dyn, l1, l2, cols):
    whole = oracle_rows(orc, pcm50k, dyn, l1, l2, cols)
    assert whole.shape == (311, cols * (1 + dyn))
    w = assert_tail_consistent(whole, cols, dyn, l1, l2, "whole")
    streamed = oracle_rows(orc, pcm50k, dyn, l1, l2, cols, block=16000)
    assert tail_ref.same_bits(streamed, whole), "streamed rows differ from the whole utterance's"
    ws = assert_tail_consistent(streamed, cols, dyn, l1, l2, "streamed in 16000-sample blocks")
    print("oracle dyn %d l (%d, %d) cols %d: worst err / bound whole %s, streamed %s" % (dyn, l1, l2, cols, w, ws))


def oracle_rows_by_stage(orc, pcm, dyn, l1, l2, cols):
    """The oracle's rows of an utterance of ANY length from its stage functions: statics of a dyn = NONE run, then its
    float32 delta stage (orc_delta_apply, deltacpu.cpp:16-29) over the clamped rows as MfccCpu::do_delta lays them out.
    (The call sequence of run_utterance refuses an utterance of no more than D frames, as the reference does.)"""
    import ctypes as C
    x = orc.run_utterance(cfg_for(orc, 0, l1, l2, cols), pcm, bug_compat=False)
    T = x.shape[0]
    l2p = l2 if dyn == 2 else 0
    D = l1 + l2p
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    xp = np.ascontiguousarray(x[np.clip(np.arange(-D, T + D), 0, T - 1)])
    d = np.zeros((T + 2 * l2p, cols), np.float32)
    orc.lib().orc_delta_apply(fp(xp), cols, T + 2 * l2p, l1, fp(d))
    groups = [x, d[l2p:l2p + T]]
    if dyn == 2:
        dd = np.zeros((T, cols), np.float32)
        orc.lib().orc_delta_apply(fp(d), cols, T, l2, fp(dd))
        groups.append(dd)
    return np.concatenate(groups, 1)


@pytest.mark.parametrize("dyn,l1,l2,cols", SHAPES)
def test_oracle_short_utterances_pass(orc, pcm50k, dyn, l1, l2, cols):
    D = l1 + (l2 if dyn == 2 else 0)
    assert tail_ref.same_bits(oracle_rows_by_stage(orc, pcm50k, dyn, l1, l2, cols), oracle_rows(orc, pcm50k, dyn, l1, l2, cols))
    for frames in (1, 2, D, D + 1, 2 * D + 1):
        pcm = synth_utterance(samples_for(frames), 60 + frames)
        rows = oracle_rows_by_stage(orc, pcm, dyn, l1, l2, cols)
        assert rows.shape[0] == frames
        if frames > 2 * D:   # (a first block of fewer than 2 D frames is refused by the call sequence: DESIGN.md B13)
            assert tail_ref.same_bits(rows, oracle_rows(orc, pcm, dyn, l1, l2, cols))
        w = assert_tail_consistent(rows, cols, dyn, l1, l2, "%d rows" % frames)
        print("oracle dyn %d l (%d, %d) cols %d, %d rows: worst err / bound %s" % (dyn, l1, l2, cols, frames, w))


# ---- 2. the committed vectors of the real reference pass -------------------------------------------------------------

def _vector_cases():
    out = []
    for name, case in refcases.cases().items():
        c = case["cfg"]
        if c["dyn"] != 0 and c["norm"] == 0:
            out.append(name)
    return out


@pytest.mark.parametrize("f32", [False, True], ids=["double_libm", "float_libm"])
@pytest.mark.parametrize("name", _vector_cases())
def test_reference_vectors_pass(name, f32):
    """Rows written by the reference's own compiled mfcccpu.cpp (tests/golden/make_golden.py): its arithmetic, not this
    repository's restatement of it.  The single-block run carries the reference's flush bug B1: the STATIC part
    of its last D rows holds other frames, its deltas are those of the right frames -- they are checked against the statics
    of the multi-block run of the same file, which are the same frames' and free of B1."""
    z = np.load(os.path.join(GOLDEN, "ref_mfcccpu_vectors_f32.npz" if f32 else "ref_mfcccpu_vectors.npz"))
    c = refcases.cases()[name]["cfg"]
    rows = z[name + "/rows"].copy()
    dyn, l1, l2 = c["dyn"], c["delta_l1"], c["delta_l2"]
    cols = rows.shape[1] // (1 + dyn)
    if name == "c1_single":
        multi = z["c1_multi/rows"]
        D = l1 + l2
        assert np.array_equal(rows[:-D, :cols], multi[:-D, :cols]) and not np.array_equal(rows[-D:, :cols], multi[-D:, :cols])
        rows[-D:, :cols] = multi[-D:, :cols]
    w = assert_tail_consistent(rows, cols, dyn, l1, l2, name)
    print("%s (%d rows x %d, l %d %d): worst err / bound %s" % (name, rows.shape[0], cols, l1, l2, w))


# ---- 3. the oracle's normaliser passes -------------------------------------------------------------------------------

def _first_block(orc, cfg, pcm):
    m = orc.OracleMfcc(cfg, bug_compat=False)
    n = m.set_input(pcm)
    m.set_alpha(1.0)
    m.apply()
    rows = m.get_output_data(n)
    st = m.norm_stats() if cfg.norm != 0 else None
    m.close()
    return rows, st


@pytest.mark.parametrize("kind", [1, 2, 3], ids=["CMN", "CVN", "MINMAX"])
@pytest.mark.parametrize("nad", [True, False], ids=["after_dyn", "before_dyn"])
def test_oracle_normaliser_passes(orc, kind, nad):
    """One block of the oracle against its norm = NONE twin: statistics over the rows the block delivers (after the
    deltas) or over its statics with context (before them: all T rows, read from a dyn = NONE twin)."""
    pcm = synth_utterance(samples_for(200), 9)
    dyn, l1, l2, cols = 2, 2, 3, 13
    y, st = _first_block(orc, cfg_for(orc, dyn, l1, l2, cols, norm=kind, nad=nad), pcm)
    x, _ = _first_block(orc, cfg_for(orc, dyn, l1, l2, cols), pcm)
    assert y.shape == x.shape == (200 - (l1 + l2), 3 * cols)
    if nad:
        wm, wk, keep = assert_norm_consistent(y, x, st, kind, True, cols, x.shape[0], "oracle")
    else:
        xs, _ = _first_block(orc, cfg_for(orc, 0, l1, l2, cols), pcm)
        assert xs.shape == (200, cols) and np.array_equal(xs[:x.shape[0]], x[:, :cols])
        ys = tail_ref.norm_apply_f32(xs, st[0, 0], st[0, 1], kind)
        wm, wk, keep = assert_norm_consistent(ys, xs, st, kind, False, cols, 200, "oracle statistics")
        assert tail_ref.same_bits(y[:, :cols], ys[:y.shape[0]]), "normalised statics differ in bits"
    assert keep.all()
    print("oracle norm %d nad %d: worst err / bound mean %.3g, multiplier %.3g" % (kind, nad, wm, wk))


# ---- 4. the check bites ----------------------------------------------------------------------------------------------

def _f32(a):
    return np.asarray(a, np.float64).astype(np.float32)


def _ulps(a, k):
    a = np.asarray(a, np.float32).copy()
    i = a.view(np.int32)
    i += np.where(i >= 0, k, -k).astype(np.int32)      # k units in the last place away from zero
    return a


@pytest.fixture(scope="module")
def bite_rows(orc, pcm50k):
    out = {}
    for shape in ((2, 3, 3, 13), (2, 1, 2, 13)):
        out[shape] = oracle_rows(orc, pcm50k, *shape)
        assert_tail_consistent(out[shape], shape[3], *shape[:3], what="unmodified")
    return out


def _fails(rows, cols, dyn, l1, l2):
    with pytest.raises(AssertionError, match="err / bound"):
        assert_tail_consistent(rows, cols, dyn, l1, l2, "deliberate mistake")


@pytest.mark.parametrize("shape", [(2, 3, 3, 13), (2, 1, 2, 13)])
def test_bites_delta_clamped_at_the_ends(bite_rows, shape):
    dyn, l1, l2, cols = shape
    rows = bite_rows[shape].copy()
    T = rows.shape[0]
    d = rows[:, cols:2 * cols].astype(np.float64)
    dp = d[np.clip(np.arange(-l2, T + l2), 0, T - 1)]          # the mistake: delta rows replicated, not computed
    num, _, den = tail_ref._regress(dp, l2, T, l2)
    rows[:, 2 * cols:] = _f32(num / den)
    assert np.abs(rows[l2:T - l2] - bite_rows[shape][l2:T - l2]).max() < 1e-5    # only the l2 rows at either end change
    _fails(rows, cols, dyn, l1, l2)


def test_bites_l1_l2_swapped(bite_rows):
    _fails(bite_rows[(2, 1, 2, 13)], 13, 2, 2, 1)


def test_bites_denominator_of_l1_used_for_delta_delta(bite_rows):
    rows = bite_rows[(2, 1, 2, 13)].copy()
    den1, den2 = 2.0 * 1, 2.0 * (1 + 4)
    rows[:, 26:] = _f32(rows[:, 26:].astype(np.float64) * den2 / den1)
    _fails(rows, 13, 2, 1, 2)


@pytest.mark.parametrize("shape", [(2, 3, 3, 13), (2, 1, 2, 13)])
def test_bites_one_tap_weight_off_by_one(bite_rows, shape):
    dyn, l1, l2, cols = shape
    rows = bite_rows[shape].copy()
    x = rows[:, :cols].astype(np.float64)
    T = x.shape[0]
    xp = x[np.clip(np.arange(-l1, T + l1), 0, T - 1)]
    den1 = 2.0 * sum(j * j for j in range(1, l1 + 1))
    # weight l1 + 1 on the outermost tap instead of l1
    rows[:, cols:2 * cols] = _f32(rows[:, cols:2 * cols] + (xp[2 * l1:2 * l1 + T] - xp[0:T]) / den1)
    _fails(rows, cols, dyn, l1, l2)


def test_bites_one_delta_element_moved_by_8_ulp(bite_rows):
    """The element where a unit in the last place weighs most against its bound (deltas that cancel to a small value
    have a bound of many of their own ulps: by design, that is what float32 can do there)."""
    shape = (2, 3, 3, 13)
    dyn, l1, l2, cols = shape
    rows = bite_rows[shape].copy()
    d, _, b_d, _ = delta_ref(rows[:, :cols].astype(np.float64), dyn, l1, l2)
    t, c = np.unravel_index(int(np.argmax(np.abs(d) / b_d)), d.shape)
    assert 8 * np.spacing(np.float32(abs(d[t, c]))) > 2 * b_d[t, c]
    rows[t, cols + c] = _ulps(rows[t, cols + c], 8)
    with pytest.raises(AssertionError, match="row %d of 311, column %d of 13" % (t, c)):
        assert_tail_consistent(rows, cols, dyn, l1, l2, "deliberate mistake")


@pytest.mark.parametrize("kind", [2, 3], ids=["CVN", "MINMAX"])
def test_bites_multiplier_moved_by_4_ulp(orc, kind):
    pcm = synth_utterance(samples_for(200), 9)
    y, st = _first_block(orc, cfg_for(orc, 2, 2, 3, 13, norm=kind), pcm)
    x, _ = _first_block(orc, cfg_for(orc, 2, 2, 3, 13), pcm)
    assert_norm_consistent(y, x, st, kind, True, 13, x.shape[0], "unmodified")
    st = st.copy()
    st[1, 1, 5] = _ulps(st[1, 1, 5], 4)
    with pytest.raises(AssertionError, match="multiplier err / bound"):
        assert_norm_consistent(y, x, st, kind, True, 13, x.shape[0], "deliberate mistake")
    # and rows normalised with a multiplier that is not the handle's own
    y2 = y.copy()
    y2[:, 13:26] = tail_ref.norm_apply_f32(x[:, 13:26], st[1, 0], st[1, 1], kind)
    with pytest.raises(AssertionError, match="differ in bits"):
        assert_norm_consistent(y2, x, np.asarray(_first_block(orc, cfg_for(orc, 2, 2, 3, 13, norm=kind), pcm)[1]), kind, True, 13,
                               x.shape[0], "deliberate mistake")


@pytest.mark.parametrize("kind", [1, 2, 3], ids=["CMN", "CVN", "MINMAX"])
def test_bites_statistics_over_all_rows(orc, kind):
    """batch_norm_stats = 0 takes the statistics over the T - D rows the reference's block delivers; statistics over all
    T rows are a different answer, far outside the bounds."""
    dyn, l1, l2, cols = 2, 2, 3, 13
    T, D = 200, 5
    pcm = synth_utterance(samples_for(T), 9)
    x = oracle_rows(orc, pcm, dyn, l1, l2, cols)
    assert x.shape[0] == T
    y_blk, st = _first_block(orc, cfg_for(orc, dyn, l1, l2, cols, norm=kind), pcm)
    y = np.concatenate([tail_ref.norm_apply_f32(x[:, g * cols:(g + 1) * cols], st[g, 0], st[g, 1], kind) for g in range(3)], 1)
    assert tail_ref.same_bits(y[:T - D], y_blk)
    assert_norm_consistent(y, x, st, kind, True, cols, T - D, "the block's statistics")
    wrong = np.empty_like(st)
    for g in range(3):
        mean, mult, _, _ = tail_ref.norm_stats_ref(x[:, g * cols:(g + 1) * cols], kind, T)
        wrong[g, 0], wrong[g, 1] = mean, mult
    y_wrong = np.concatenate([tail_ref.norm_apply_f32(x[:, g * cols:(g + 1) * cols], wrong[g, 0], wrong[g, 1], kind) for g in range(3)], 1)
    with pytest.raises(AssertionError, match="err / bound"):
        assert_norm_consistent(y_wrong, x, wrong, kind, True, cols, T - D, "deliberate mistake")


# ---- 5. orders the delta stage's LDS cannot hold are refused at create -----------------------------------------------

@pytest.mark.parametrize("nb,ceps,l,ok,traps_k", [(16, 0, 10, True, 16), (16, 0, 11, False, 16), (26, 13, 390, True, 0), (26, 13, 400, False, 0),
                                                  (128, 0, 30, True, 0), (128, 0, 40, False, 0)])
def test_create_refuses_orders_beyond_the_delta_lds(pkg, nb, ceps, l, ok, traps_k):
    """launch_delta's largest tile is (3 R + 2 D + 2 l2) rows (R = 64 rows of 16 floats up to 16 columns, else 32 rows of
    `cols` floats) and a block has 160 KB: 256 columns end at l1 = l2 = 10.  Asked of a planning handle (no device)."""
    import ctypes as C
    L = pkg.load_library()
    cfg = pkg.mfcc.MfxConfig(200000, W, S, nb, 16000.0, 64.0, 8000.0, ceps, 0, 22.0, 0, 2, l, l, 1, 0, 1, 0, 0, 0, 0)
    if traps_k:
        cfg.method, cfg.traps_len, cfg.traps_dct_len = pkg.METHOD_TRAPS, 31, traps_k
    cols = nb * traps_k if traps_k else (ceps or nb)
    R, cw = (64, 16) if cols <= 16 else (32, cols)
    assert ((3 * R + 2 * 2 * l + 2 * l) * cw * 4 <= 160 * 1024) == ok
    h = C.c_void_p()
    rc = L.mfx_plan_create(C.byref(cfg), C.byref(h))
    assert rc == (0 if ok else -5)
    if rc == 0:
        L.mfx_destroy(h)
