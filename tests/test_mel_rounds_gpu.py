"""k_front512's mel walk, one round class at a time (MI355X, through the batch entry): rounds of 8, 16 and 32 bins, a round
longer than 32 bins that is a multiple of neither 16 nor 32, a plan of one round and one of five; the form with the DCT on the
matrix pipe and the plain form; the zero-stuffed 256-point form -- on one batch of 5, 18 and 37 frames
(tests/mel_rounds_cases.py).  Per case: the plan really has the rounds the case is here for (host code alone), the rows
match the oracle at the project's bar, and they are bit for bit the rows recorded from commit cb8bf57 on the same GPU
(tests/golden/mel_rounds_parent.npz, written by tests/golden/make_mel_rounds_parent.py).  The walk issues a round's reads in
batches of 16 bins plus an 8-bin remainder (mel_batch / mel_round, csrc/mfx_front512.hip;
profiles/r05/abx_c2_mel_round_batches.txt); the recorded commit walked 8 bins per trip.  Any batching has to add the same
products to the same accumulator in the same order."""
import os

import numpy as np
import pytest

import mel_rounds_cases as MC
from conftest import GOLDEN, assert_close

pytestmark = pytest.mark.gpu

BATCHES = (16, 32)   # bins per batch: 16 in the kernel; 32 was measured too (longer ones do not fit the registers)
META_ROUNDS = 4      # rounds whose metadata a walk could hold in registers before it starts (measured, not adopted)


def trips(L, batch):
    """The batches a round of L bins falls into: whole batches, then 16 bins where 32 are the batch, then the 8-bin remainder."""
    assert L % 8 == 0 and L >= 8
    return [batch] * (L // batch) + [16] * (L % batch // 16) + [8] * (L % 16 // 8)


# the round lengths each case's plan must have
WANT = {name: L for name, (sh, L, why) in MC.CASES.items()}


@pytest.fixture(scope="module")
def parent_rows():
    return np.load(os.path.join(GOLDEN, "mel_rounds_parent.npz"))


def test_the_cases_cover_every_round_class(pkg):
    """From the plans alone: between them the cases have rounds of 8, 16 and 32 bins (C2's), a round longer than either batch
    size and a multiple of neither, a plan of one round and one of more rounds than a walk would fetch metadata for up front,
    and both forms of the walk; for either batch size that means a round of the remainder alone, of one batch, of several,
    and of batches plus a remainder."""
    lengths, forms, counts = set(), set(), set()
    for name, (sh, L, why) in MC.CASES.items():
        kernel, got = MC.plan_rounds(pkg, sh)
        assert kernel == "k_front512" and got == L, (name, kernel, got)
        counts.add(len(L))
        forms.add("matrix pipe" if (sh["nc"] > 0 and sh["nb"] <= 40) else "plain")
        lengths.update(L)
    assert {8, 16, 32} <= lengths and forms == {"matrix pipe", "plain"} and 1 in counts and max(counts) > META_ROUNDS
    assert any(v > max(BATCHES) and all(v % b for b in BATCHES) for v in lengths)
    for b in BATCHES:
        seen = {(min(t.count(b), 2), len(t) - t.count(b) > 0) for t in (trips(v, b) for v in lengths)}
        assert seen >= {(0, True), (1, False), (1, True)} and seen & {(2, False), (2, True)}, (b, seen)


@pytest.mark.parametrize("name", list(MC.CASES))
def test_round_batches(pkg, orc, parent_rows, name):
    sh, L, why = MC.CASES[name]
    kernel, got_L = MC.plan_rounds(pkg, sh)
    assert kernel == "k_front512" and got_L == WANT[name], "%s (%s): the plan has rounds %s" % (name, why, got_L)

    rows, first, ran = MC.run_batch(pkg, sh)
    assert ran == "k_front512"
    cols = (sh["nc"] + (1 if sh["c0"] else 0)) if sh["nc"] > 0 else sh["nb"]
    assert rows.shape == (sum(MC.FRAMES), cols) and np.isfinite(rows).all()

    cfg = orc.make_config(200 * sh["S"] + sh["W"], window_size=sh["W"], shift=sh["S"], num_banks=sh["nb"], sample_rate=sh["sr"],
                          ceps_len=sh["nc"], want_c0=sh["c0"], dyn=orc.DYN_NONE)
    window = pkg.reference_window(sh["W"])
    for u, r0, frames in zip(MC.utterances(sh), first, MC.FRAMES):
        want = orc.run_utterance(cfg, u, window)
        assert_close(rows[r0:r0 + frames], want, "%s, utterance of %d frames" % (name, frames))

    assert np.array_equal(parent_rows[name + "__first_rows"], np.asarray(first, np.int32))
    got = np.ascontiguousarray(rows, np.float32).view(np.int32)
    diff = got != parent_rows[name]
    assert not diff.any(), "%s: %d elements differ from the parent's rows (first: row %d, column %d)" % (
        name, int(diff.sum()), *[int(v[0]) for v in np.nonzero(diff)])
