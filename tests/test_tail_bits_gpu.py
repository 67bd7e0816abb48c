"""The kernels behind the front ends, one case per instantiation or branch (MI355X; tests/tail_bits_cases.py): the delta
kernels, the normaliser's one- and two-kernel forms, k_melcep / k_plp and their row-run forms, k_traps and k_splice_affine on
both pipes and at every tile height, the streaming interface and the session entries.  Per case: the kernel or branch the
case is there for follows from the launcher's conditions restated beside the cases, the rows are finite (but where the
normaliser's statistics cover a single row: TC.assert_finite; TRAPS, PLP, the
transform and the delta stage have their float64 references in their own suites), and every row is bit for bit the row
recorded from commit 90865a5 on the same GPU (tests/golden/tail_bits_parent.npz, written by
tests/golden/make_tail_bits_parent.py: the rows of the three shortest utterances in full, an 8-byte digest of every row).  The
change after that commit moved these kernels' tile, slicing and launch code into shared pieces (profiles/r07/README.md); the
recorded rows hold the next change to the same.

test_segment_list_beyond_grid_y needs no fixture: 65 537 one-frame utterances, two beyond the grid.y limit, against the same
utterances planned as two halves."""
import os

import numpy as np
import pytest

import tail_bits_cases as TC
from conftest import GOLDEN

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def parent():
    return np.load(os.path.join(GOLDEN, "tail_bits_parent.npz"))


def test_every_case_takes_the_branch_it_names():
    for name, c in TC.CASES.items():
        assert TC.branch(c) == c["want"], (name, TC.branch(c), c["want"])
    wants = " ".join(c["want"] for c in TC.CASES.values())
    for k in ("k_delta16<3,3>", "k_delta16<0,0>", "k_delta<true,64>", "k_delta<false,32>", "k_delta4<32>", "k_norm_seg", "k_norm_finalize",
              "k_melcep", "k_melcep_runs", "k_plp<8>", "k_plp<16>", "k_plp<32>", "k_plp_runs<16>", "k_traps<false,0> R64",
              "k_traps<false,0> R32", "k_traps<false,0> R16", "k_traps<true,4>", "k_traps<true,16>", "k_traps<true,32>",
              "k_splice_affine<false,1>", "k_splice_affine<false,2>", "k_splice_affine<false,3>", "k_splice_affine<false,4>", "k_splice_affine<false,8>", "k_splice_affine<false,16>",
              "k_splice_affine<true,3>", "k_sess_gather"):
        assert k in wants, k


@pytest.mark.parametrize("name", list(TC.CASES))
def test_tail_bits(pkg, parent, name):
    c = TC.CASES[name]
    assert TC.branch(c) == c["want"]
    got = TC.run_case(pkg, name)
    TC.assert_finite(name, got)
    full = TC.shortest_bits(got)
    want_full = parent[name + "__rows"]
    assert full.shape == want_full.shape, (name, full.shape, want_full.shape)
    diff = full != want_full
    assert not diff.any(), "%s: %d elements of the shortest utterances differ from the parent's rows (first: row %d, column %d)" % (
        name, int(diff.sum()), *[int(v[0]) for v in np.nonzero(diff)])
    d, want_d = TC.digests(got), parent[name + "__digests"]
    assert d.shape == want_d.shape, (name, d.shape, want_d.shape)
    bad = np.nonzero(d != want_d)[0]
    if bad.size:
        ends = np.cumsum(c["frames"])
        u = int(np.searchsorted(ends, bad[0], side="right"))
        pytest.fail("%s (%s): %d rows differ from the parent's; the first is row %d of the utterance of %d frames" % (
            name, c["want"], bad.size, int(bad[0] - (ends[u] - c["frames"][u])), c["frames"][u]))


# ---- a segment list longer than grid.y ----------------------------------------------------------------------------------

N_UTT = 65537      # two more than grid.y admits: the launchers cut the list in two slices


@pytest.fixture(scope="module")
def many():
    """65 537 utterances of one frame each (computed once, never modified): noise, every utterance its own."""
    rng = np.random.default_rng(65537)
    pcm = np.clip(np.round(3000.0 * rng.standard_normal(N_UTT * TC.W, dtype=np.float32)), -32768, 32767).astype(np.int16)
    pcm.setflags(write=False)
    return pcm, np.arange(N_UTT, dtype=np.int64) * TC.W, np.full(N_UTT, TC.W, np.int64)


def _c2(pkg, norm):
    m = pkg.MfccHip(200000, TC.W, TC.S, 40, TC.SR, 64.0, TC.SR / 2, 13, False, 22.0, norm, 2, 3, 3, True, device=0, bug_compat=False)
    m.set_window(pkg.reference_window(TC.W))
    return m


def _halves(m, pcm, offs, lens, setup=None):
    """The batch as two plans of at most 65 535 utterances: rows in the whole batch's order."""
    h, out = (N_UTT + 1) // 2, []
    assert h <= 65535
    for a, b in ((0, h), (h, N_UTT)):
        rows, total = m.batch_plan(offs[a:b] - offs[a], lens[a:b])
        assert total == b - a
        if setup:
            setup(m, a, b)
        out.append(m.batch_run_host(pcm[offs[a]:offs[b - 1] + lens[b - 1]]))
    return np.concatenate(out)


def _assert_same_rows(whole, halves, what):
    assert whole.shape == halves.shape == (N_UTT, 39)
    bad = np.nonzero((whole.view(np.int32) != halves.view(np.int32)).any(axis=1))[0]
    assert not bad.size, "%s: %d utterances differ from their rows in a half (first: utterance %d)" % (what, bad.size, int(bad[0]))


def test_segment_list_beyond_grid_y(pkg, many):
    """C2 shape with deltas and CVN: launch_delta and launch_norm_fused run a second slice.  One-row utterances: the deltas
    are zeros and the CVN of a single row is 0 x inf -- compared as bit patterns, NaN payloads included, which holds the
    second slice to having run on its own segments; the rows themselves are compared in the run without the normaliser,
    whole batch against halves, where every row is finite and differs from every other."""
    pcm, offs, lens = many
    m = _c2(pkg, TC.CVN)
    try:
        rows, total = m.batch_plan(offs, lens)
        assert total == N_UTT and (rows == np.arange(N_UTT)).all()
        whole = m.batch_run_host(pcm)
        _assert_same_rows(whole, _halves(m, pcm, offs, lens), "CVN per utterance")
    finally:
        m.close()
    plain = _c2(pkg, TC.NORM_NONE)      # the same without the normaliser: finite rows, every utterance its own
    try:
        plain.batch_plan(offs, lens)
        x = plain.batch_run_host(pcm)
        _assert_same_rows(x, _halves(plain, pcm, offs, lens), "no normaliser")
    finally:
        plain.close()
    assert np.isfinite(x).all() and (x[:, 13:] == 0).all() and len(np.unique(x[:, 0])) > N_UTT // 2
    assert (x[65535:, :13] != x[:2, :13]).any(), "the utterances beyond the first slice have rows of their own"


def test_speaker_list_beyond_grid_y(pkg, many):
    """The same batch with CVN pooled over 3 speakers: launch_spk_sums runs a second slice.  The pooled sums of the whole
    batch are checked on their own -- counts and extrema exactly, sums within the rounding of 65 537 double additions -- and
    then serve as the prior of the two halves (MFX_SPK_PRIOR_ONLY), whose rows must be the whole batch's bit for bit."""
    pcm, offs, lens = many
    spk = (np.arange(N_UTT) % 3).astype(np.int32)
    plain = _c2(pkg, TC.NORM_NONE)
    try:
        plain.batch_plan(offs, lens)
        x = plain.batch_run_host(pcm).astype(np.float64)
    finally:
        plain.close()
    m = _c2(pkg, TC.CVN)
    try:
        m.batch_plan(offs, lens)
        m.batch_set_speakers(spk, 3)
        whole = m.batch_run_host(pcm)
        count, acc, stats = m.batch_speaker_stats()
        # (one-frame utterances: every delta is 0, so is its pooled variance, and those columns are 0 x inf in whole and halves)
        assert np.isfinite(whole[:, :13]).all() and (acc[:, :, 13:] == 0).all()
        for s in range(3):
            xs = x[spk == s]
            assert count[s] == len(xs)
            assert (acc[s, 2] == xs.min(0)).all() and (acc[s, 3] == xs.max(0)).all()
            for k, v in ((0, xs), (1, np.float32(xs) * np.float32(xs))):   # (the squares are float32 products, as the reference's)
                v = np.asarray(v, np.float64)
                assert (np.abs(acc[s, k] - v.sum(0)) <= len(xs) * 2.0 ** -52 * np.abs(v).sum(0)).all(), (s, k)
        halves = _halves(m, pcm, offs, lens,
                         lambda h, a, b: h.batch_set_speakers(spk[a:b], 3, prior=(count, acc), mode=pkg.mfcc.SPK_PRIOR_ONLY))
        _assert_same_rows(whole, halves, "CVN pooled over 3 speakers")
    finally:
        m.close()
