"""Per-utterance warp factors of the batch entries (mfx_batch_set_alphas), the parts that need no GPU: the entry on a
planning handle, and the run-list builder (mfx_host_alpha_runs: the lists the row-run kernels read, built by the code that
builds them for upload) -- its merge rule, its handling of frameless utterances and the clipping to a slab window."""
import ctypes as C
import re
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_exports_and_prototypes_name_the_entry(pkg):
    header = open(os.path.join(ROOT, "include", "mfx.h")).read()
    for name in ("mfx_batch_set_alphas", "mfx_host_alpha_runs"):
        assert re.search(r"\b%s\s*\(" % name, header)
        assert name in pkg.mfcc.EXPORTED_SYMBOLS
        assert getattr(pkg.load_library(), name).argtypes is not None
    assert pkg.load_library().mfx_abi_version() == 2        # a function is added, no struct changes


def test_set_alphas_on_a_planning_handle_is_a_device_error(pkg):
    L = pkg.load_library()
    cfg = pkg.mfcc.MfxConfig(100 * 160 + 400, 400, 160, 40, 16000.0, 64.0, 8000.0, 13, 0, 22.0, 0, 2, 3, 3, 1, 0, 1, 1, 0, 0, 0)
    h = C.c_void_p()
    assert L.mfx_plan_create(C.byref(cfg), C.byref(h)) == 0
    try:
        a = np.ones(1, np.float32)
        assert L.mfx_batch_set_alphas(h, a.ctypes.data_as(C.POINTER(C.c_float)), 1) == -6      # MFX_ERR_DEVICE
        assert L.mfx_batch_set_alphas(h, None, 0) == -6
        assert b"planning handle" in L.mfx_last_error(h)
    finally:
        L.mfx_destroy(h)


def rows_of(runs):
    return [r for a, n in runs for r in range(int(a), int(a + n))]


def test_equal_neighbours_merge_and_unequal_ones_do_not(pkg):
    alphas = np.array([1.0, 0.88, 0.88, 1.12, 1.0, 1.0, 0.88, 1.12, 1.12], np.float32)
    frames = [2, 1, 3, 4, 5, 63, 64, 65, 130]
    tables, off, runs = pkg.mfcc.host_alpha_runs(alphas, frames)
    assert tables.tolist() == [np.float32(1.0), np.float32(0.88), np.float32(1.12)]          # order of first appearance
    assert off.tolist() == [0, 2, 4, 6]
    row = np.concatenate([[0], np.cumsum(frames)])
    assert runs.tolist() == [[0, 2], [row[4], 5 + 63],                    # 1.0: utterance 0; utterances 4 + 5 merged
                             [row[1], 1 + 3], [row[6], 64],               # 0.88: 1 + 2 merged; 6 far away, same table
                             [row[3], 4], [row[7], 65 + 130]]             # 1.12: 3; 7 + 8 merged
    # every row of the batch exactly once, under its own utterance's table
    owner = np.full(row[-1], -1)
    for a in range(len(tables)):
        for r in rows_of(runs[off[a]:off[a + 1]]):
            assert owner[r] == -1
            owner[r] = a
    want = np.concatenate([np.full(f, tables.tolist().index(v)) for v, f in zip(alphas.tolist(), frames)])
    assert np.array_equal(owner, want)


def test_factors_are_compared_bit_for_bit(pkg):
    a = np.float32(0.9)
    b = np.nextafter(a, np.float32(1.0), dtype=np.float32)
    tables, off, runs = pkg.mfcc.host_alpha_runs(np.array([a, b, a], np.float32), [3, 3, 3])
    assert len(tables) == 2 and tables[0] == a and tables[1] == b                            # nothing is quantised
    assert runs.tolist() == [[0, 3], [6, 3], [3, 3]]


def test_frameless_utterances_vanish(pkg):
    # utterance 0 and 2 have no frame: no run of theirs; 1 and 3 (same factor) touch across the frameless one: one run
    tables, off, runs = pkg.mfcc.host_alpha_runs(np.array([0.9, 1.1, 0.9, 1.1, 0.9], np.float32), [0, 4, 0, 5, 7])
    assert tables.tolist() == [np.float32(0.9), np.float32(1.1)]
    assert runs[off[0]:off[1]].tolist() == [[9, 7]]
    assert runs[off[1]:off[2]].tolist() == [[0, 9]]
    # a factor no utterance with frames uses keeps its table (the index space is the caller's list) and owns no run
    tables, off, runs = pkg.mfcc.host_alpha_runs(np.array([0.9, 1.1], np.float32), [0, 4])
    assert len(tables) == 2 and off.tolist() == [0, 0, 1] and runs.tolist() == [[0, 4]]
    tables, off, runs = pkg.mfcc.host_alpha_runs(np.zeros(0, np.float32), [])
    assert len(tables) == 0 and off.tolist() == [0] and runs.shape[0] == 0


def test_clipping_to_consecutive_windows_keeps_every_row_exactly_once(pkg):
    rng = np.random.default_rng(5)
    n = 200
    alphas = rng.choice(np.array([0.8, 0.9, 1.0, 1.1, 1.2], np.float32), size=n)
    frames = rng.choice([0, 1, 3, 4, 5, 63, 64, 65, 130, 1000], size=n)
    total = int(frames.sum())
    tables, off, runs = pkg.mfcc.host_alpha_runs(alphas, frames)
    whole = {a: rows_of(runs[off[a]:off[a + 1]]) for a in range(len(tables))}
    assert sorted(r for v in whole.values() for r in v) == list(range(total))
    for slab in (1, 64, 777, 4096, total, total + 5):
        seen = {a: [] for a in range(len(tables))}
        for w0 in range(0, total, slab):
            t2, off2, runs2 = pkg.mfcc.host_alpha_runs(alphas, frames, window=(w0, slab))
            assert np.array_equal(t2, tables)
            for a in range(len(tables)):
                part = runs2[off2[a]:off2[a + 1]]
                assert all(n_ > 0 and a_ >= w0 and a_ + n_ <= w0 + slab for a_, n_ in part)    # inside the window, none empty
                seen[a] += rows_of(part)
        assert seen == whole, "slab of %d rows" % slab                                        # same rows, same order, once
