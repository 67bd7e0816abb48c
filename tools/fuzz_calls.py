"""Dev aid (GPU box): random CALL SEQUENCES on the streaming interface (the reference's ParamBase protocol, parambase.h:23-32,
ASR_OCL.cpp:227-301), legal steps mirrored on the CPU checker, illegal ones thrown in on the product only:

  legal    set_input(block) -> [set_alpha] -> apply [-> apply with another alpha] -> get_output_data(n) [again, or fewer rows]
           ... -> flush -> apply -> get_output_data -> (a new stream on the same handle); on about half the blocks
           a VTLN sweep (apply_alphas over a random subset of {0.9, 1.0, 1.1}) before or after the plain apply(s), the plain rows
           and every alpha's rows then read in random order, into pageable or pinned memory
  illegal  apply / get_output_data with no block, get_output_data before apply or for more rows than the block has, blocks longer
           than get_input_buffer_size(), empty blocks, flush twice, flush on a fresh handle, negative counts, NULL pointers,
           get_output_data_alpha outside the last sweep or on a block that has had a plain apply and no sweep

Checks: plain rows of norm = NONE handles against the checker; of normalised handles with the three-part check of
conftest.assert_normalised_close (norm = NONE twins, product and checker, driven through the same legal steps; statistics from
mfx_debug_read(5)).  Each alpha's rows against a checker object of its own fed every block (norm = NONE), or bit for bit against
a product twin handle of its own (normalised).

The product must answer every illegal step with a status code (or rows nobody specified) -- never crash, never hang -- and the
legal steps that follow must still deliver the checker's rows: state is not corrupted by misuse.

    python tools/fuzz_calls.py [seed] [handles]
"""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as G  # noqa: E402
from conftest import assert_normalised_close  # noqa: E402

pkg = G.load_package()
orc = G.load_oracle()
seed = int(sys.argv[1]) if len(sys.argv) > 1 else 1
n_handles = int(sys.argv[2]) if len(sys.argv) > 2 else 40
rng = np.random.default_rng(seed)
failures = 0
fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
sp = lambda a: a.ctypes.data_as(C.POINTER(C.c_int16))
SWEEP = [0.9, 1.0, 1.1]
L0 = pkg.load_library()
L0.mfx_alloc_pinned.argtypes, L0.mfx_alloc_pinned.restype = [C.c_size_t], C.c_void_p
L0.mfx_free_pinned.argtypes, L0.mfx_free_pinned.restype = [C.c_void_p], None

for hcase in range(n_handles):
    W2 = int(rng.choice([256, 512, 512, 1024, 2048]))
    W = int(rng.integers(W2 // 2 + 1, W2 + 1))
    S = int(rng.integers(max(8, W // 5), W // 2 + 1))
    sr = float(rng.choice([8000.0, 16000.0, 44100.0]))
    nb, nc, c0 = int(rng.choice([15, 26, 40])), int(rng.integers(2, 14)), bool(rng.integers(0, 2))
    dyn = int(rng.integers(0, 3))
    norm = int(rng.choice([0, 0, 1]))
    l1, l2 = int(rng.integers(1, 4)), int(rng.integers(1, 4))
    D = (l1 if dyn else 0) + (l2 if dyn == 2 else 0)
    groups = 1 + dyn
    blk = int(rng.integers((2 * D + 3) * S + W, (2 * D + 40) * S + W))
    window = pkg.reference_window(W)
    what = "handle %3d W %4d S %3d sr %5.0f nb %2d nc %2d c0 %d dyn %d l %d%d norm %d blk %d" % (hcase, W, S, sr, nb, nc, c0, dyn, l1, l2, norm, blk)
    mk = lambda nm: pkg.MfccHip(blk, W, S, nb, sr, 64.0, sr / 2, nc, c0, 22.0, nm, dyn, l1, l2, True, bug_compat=True)
    mkcfg = lambda nm: orc.make_config(blk, window_size=W, shift=S, num_banks=nb, sample_rate=sr, high_freq=sr / 2, ceps_len=nc,
                                       want_c0=c0, norm=nm, dyn=dyn, delta_l1=l1, delta_l2=l2, norm_after_dyn=True)
    m = mk(norm)
    L, h = m._L, m._h
    cfg = mkcfg(norm)
    o = orc.OracleMfcc(cfg, window)
    # per alpha of the sweep: a checker fed every block (norm NONE) or a product twin (normalised: bit for bit); on normalised
    # handles the norm = NONE twins of the plain stream, product and checker
    per_alpha = [orc.OracleMfcc(cfg, window) if norm == 0 else mk(norm) for _ in SWEEP]
    twins0 = [mk(0), orc.OracleMfcc(mkcfg(0), window)] if norm else []
    width, ibs = m.get_output_data_width(), m.get_input_buffer_size()
    cap = m.max_frames_out() + 64
    out = np.zeros(cap * width, np.float32)
    pin_ptr = L0.mfx_alloc_pinned(cap * width * 4)
    pin = np.ctypeslib.as_array(C.cast(pin_ptr, C.POINTER(C.c_float)), shape=(cap * width,))
    nfr = C.c_int32()
    notes = []
    cur_sweep = []   # alphas of the current block's sweep

    def misuse():
        """one illegal call on the product only; returns a description when the answer is not a status code"""
        k = int(rng.integers(0, 10))
        if k == 0:
            rc = L.mfx_apply(h)
        elif k == 1:
            rc = L.mfx_get_output_data(h, fp(out), int(rng.integers(1, cap)))
        elif k == 2:
            big = np.zeros(ibs + int(rng.integers(1, 500)), np.int16)
            rc = L.mfx_set_input(h, sp(big), big.size, C.byref(nfr))
            if rc == 0:
                return "a block longer than get_input_buffer_size() was accepted"
        elif k == 3:
            rc = L.mfx_set_input(h, sp(np.zeros(4, np.int16)), -1, C.byref(nfr))
            if rc == 0:
                return "a negative sample count was accepted"
        elif k == 4:
            rc = L.mfx_set_input(h, None, 100, C.byref(nfr))
            if rc == 0:
                return "a NULL block was accepted"
        elif k == 5:
            rc = L.mfx_get_output_data(h, None, 3)
            if rc == 0:
                return "a NULL output buffer was accepted"
        elif k == 6:
            rc = L.mfx_get_output_data(h, fp(out), -2)
            if rc == 0:
                return "a negative row count was accepted"
        elif k == 7:
            rc = L.mfx_get_output_data(h, fp(out), 1 << 28)
            if rc == 0:
                return "2^28 rows were accepted"
        elif k == 8:
            rc = L.mfx_apply_alphas(h, None, 3)
            if rc == 0:
                return "a NULL alpha list was accepted"
        else:
            idx = int(rng.choice([-1, len(cur_sweep), len(cur_sweep) + int(rng.integers(1, 5))]))
            rc = L.mfx_get_output_data_alpha(h, idx, fp(out), int(rng.integers(1, 50)))
            if rc == 0:
                return "alpha index %d outside the last sweep (%d alphas) was accepted" % (idx, len(cur_sweep))
        return None

    def read(idx, k):
        """k rows of the plain stream (idx None) or of alpha idx of the sweep, into a pageable or a pinned buffer"""
        buf = pin if rng.integers(0, 2) else out
        buf[:k * width] = np.nan
        m._chk(L.mfx_get_output_data(h, fp(buf), k) if idx is None else L.mfx_get_output_data_alpha(h, idx, fp(buf), k))
        return buf[:k * width].reshape(k, width).copy()

    def close_to(y, ref, sc, what):
        """norm NONE: the bar is 1e-4 of the column group's scale over the STREAM so far (sc: that scale per group; a flush block
        of D rows of delta-deltas can lie a hundred times below the stream's scale)"""
        w = ref.shape[1] // groups
        for g_ in range(groups):
            x_, y_ = y[:, g_ * w:(g_ + 1) * w].astype(np.float64), ref[:, g_ * w:(g_ + 1) * w].astype(np.float64)
            sc[g_] = max(sc[g_], np.abs(y_).max())
            if np.abs(x_ - y_).max() > 1e-4 * max(sc[g_], 1e-30) or not np.isfinite(x_).all():
                notes.append("%s differ from the checker's (group %d)" % (what, g_))

    try:
        for e in [m] + [e for e in per_alpha + twins0 if isinstance(e, pkg.MfccHip)]:
            e.set_window(window)
        if rng.integers(0, 3) == 0:   # misuse on a fresh handle (flush before any block: the reference's flush() on an empty segmenter)
            L.mfx_flush(h, C.byref(nfr))
            o2 = orc.OracleMfcc(cfg, window)   # (the checker's flush on a fresh object is defined: 0 frames)
            o2.close()
            for _ in range(int(rng.integers(1, 4))):
                w_ = misuse()
                if w_:
                    notes.append(w_)
        for stream in range(int(rng.integers(1, 4))):     # several files on one handle
            n_total = int(rng.integers(1, 5)) * ibs + int(rng.integers(0, ibs))
            pcm = (4000.0 * rng.standard_normal(n_total)).round().clip(-32768, 32767).astype(np.int16)
            pos = 0
            scale = [0.0] * groups
            scale_n = [0.0] * groups   # (normalised rows)
            scale_a = [[0.0] * groups for _ in SWEEP]
            prev_sweep = []
            while True:
                last = pos >= pcm.size
                if rng.integers(0, 4) == 0 and not last:
                    w_ = misuse()     # between blocks: must not disturb the stream (a refused set_input leaves the state alone)
                    if w_:
                        notes.append(w_)
                if last:
                    a, b = m.flush(), o.flush()
                    fed = [e.flush() for e in per_alpha + twins0]
                else:
                    piece = pcm[pos:pos + ibs]
                    a, b = m.set_input(piece), o.set_input(piece)
                    fed = [e.set_input(piece) for e in per_alpha + twins0]
                    pos += ibs
                cur_sweep = []
                if a != b or any(f != a for f in fed):
                    notes.append("frame counts %d vs %d (twins %s)" % (a, b, fed))
                    break
                if a > 0:
                    # a sweep on about half the blocks; on a normalised handle a flush block re-uses the statistics of the
                    # previous block's sweep at the same index (mfx.h), so it repeats that sweep or has none
                    sweep = [float(x) for x in rng.permutation(SWEEP)[:int(rng.integers(1, len(SWEEP) + 1))]] if rng.integers(0, 2) else []
                    if norm and last:
                        sweep = prev_sweep if rng.integers(0, 2) else []
                    sweep_first = bool(rng.integers(0, 2))
                    if sweep and sweep_first:
                        m.apply_alphas(sweep)
                    alphas = [1.0] if rng.integers(0, 3) else [float(rng.choice([0.9, 1.1])), 1.0]
                    for al in alphas:      # apply may be repeated with another alpha on the same block
                        for e in [m, o] + twins0:
                            e.set_alpha(al)
                            e.apply()
                    if sweep and not sweep_first:
                        m.apply_alphas(sweep)
                    cur_sweep = sweep
                    if not sweep and rng.integers(0, 4) == 0:   # alpha rows of a block that has had a plain apply and no sweep
                        if L.mfx_get_output_data_alpha(h, 0, fp(out), a) == 0:
                            notes.append("alpha rows of a block without a sweep were delivered")
                    want = o.get_output_data(a)
                    want_a = []
                    for e, al in zip(per_alpha, SWEEP):
                        e.set_alpha(al)
                        e.apply()
                        want_a.append(e.get_output_data(a))
                    x0, x0_want = (twins0[0].get_output_data(a), twins0[1].get_output_data(a)) if norm else (None, None)
                    st = m.debug_read(5).reshape(-1, 2, width // groups) if norm else None
                    # the plain rows (again, or fewer rows) and every alpha's rows, in random order
                    reads = [(None, k) for k in ([a] if rng.integers(0, 2) else [a, max(1, a // 2)])]
                    reads += [(i, a if rng.integers(0, 3) else max(1, a // 2)) for i in range(len(sweep))]
                    plain_rows = None
                    for j in rng.permutation(len(reads)):
                        idx, k = reads[j]
                        y = read(idx, k)
                        where = "flush" if last else "a block"
                        if idx is None:
                            plain_rows = y if plain_rows is None or k > plain_rows.shape[0] else plain_rows
                            if norm == 0:
                                close_to(y, want[:k], scale, "rows after %s" % where)
                            elif last:
                                # a flush block's D rows re-use the previous block's statistics (checked there); its deltas can
                                # lie far below the stream's scale, so twin and rows are held to the stream-scale bar above
                                close_to(x0[:k], x0_want[:k], scale, "un-normalised twin's rows after flush")
                                close_to(y, want[:k], scale_n, "plain rows after flush")
                            else:
                                try:
                                    assert_normalised_close(y, want[:k], x0[:k], x0_want[:k], st, o.norm_stats(), groups, True,
                                                            "plain rows after %s" % where, norm=norm)
                                except AssertionError as e:
                                    notes.append((str(e).splitlines() or ["plain rows fail the normalisation check"])[0])
                                close_to(x0[:k], x0_want[:k], scale, "un-normalised twin's rows")
                                close_to(y, want[:k], scale_n, "plain rows")
                        else:
                            ai = SWEEP.index(sweep[idx])
                            if norm == 0:
                                close_to(y, want_a[ai][:k], scale_a[ai], "alpha %.1f rows after %s" % (sweep[idx], where))
                            elif not np.array_equal(y, want_a[ai][:k], equal_nan=True):
                                notes.append("alpha %.1f rows after %s differ from its twin's" % (sweep[idx], where))
                    prev_sweep = sweep
                    if rng.integers(0, 4) == 0:
                        w_ = misuse()
                        if w_:
                            notes.append(w_)
                        if not np.array_equal(read(None, plain_rows.shape[0]), plain_rows, equal_nan=True):
                            notes.append("a refused call changed the plain rows")
                if last or notes:
                    break
            if notes:
                break
            if rng.integers(0, 2):     # a second flush: nothing left (the reference returns the same rows again)
                L.mfx_flush(h, C.byref(nfr))
                for e in [o] + per_alpha + twins0:
                    e.flush()
    except pkg.MfxError as e:
        notes.append("MfxError on a legal step: %s" % e)
    except RuntimeError as e:
        notes.append("checker refused a legal step: %s" % e)
    for e in [m, o] + per_alpha + twins0:
        e.close()
    L0.mfx_free_pinned(pin_ptr)
    failures += bool(notes)
    print("%s: %s" % (what, "ok" if not notes else "FAIL -- " + "; ".join(sorted(set(notes)))), flush=True)
print("seed %d: %d handles, %d failures" % (seed, n_handles, failures))
sys.exit(1 if failures else 0)
