"""The Kaldi front-end kernels, one case per branch (MI355X; tests/kaldi_bits_cases.py): k_kaldi_front at the three DFT lengths,
fbank and MFCC, under the three frame options, and k_kaldi_front_opts under every flag, each under Povey's window or the ramp.
Per case the rows are finite and every row is bit for bit the row recorded from commit b6732e9 on the same GPU
(tests/golden/kaldi_bits_parent.npz, written by tests/golden/make_kaldi_bits_parent.py: the rows of the three shortest non-empty
utterances in full, an 8-byte digest of every row).  The change after that commit moved the wave FFT, the real split and the
mel-span chain into the header the STFT FFT form shares; the recorded rows hold the next change to the same.

The method's FFT is deliberately NOT tied to a summation order (include/mfx.h): the cases here guard refactors.  A change that
alters the transform on purpose re-records them with the committed recorder and proves itself against float64
(tests/test_kaldi_gpu.py)."""
import os

import numpy as np
import pytest

import kaldi_bits_cases as BC
from conftest import GOLDEN

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def parent():
    return np.load(os.path.join(GOLDEN, "kaldi_bits_parent.npz"))


def test_cases_cover_every_branch(parent):
    seen, flags, opts, floors = BC.branches()
    for N in (128, 256, 512):
        for mfcc in (False, True):
            for window in ("povey", "ramp"):
                assert (N, mfcc, False, window) in seen, (N, mfcc, window)                 # k_kaldi_front
    assert {(N, mfcc) for N, mfcc, o, w in seen if o} >= {(256, False), (512, False), (512, True)}   # k_kaldi_front_opts
    assert flags == {0, 1, 2, 2 | 4, 2 | 8, 8, 1 | 2 | 4 | 8}
    assert opts == {"preemph", "remove_dc", "use_power"} and floors == {0.0, 1.0}
    assert {c["shape"].W == BC.fft_size(c["shape"].W) for c in BC.CASES.values() if c["shape"].W > 256} == {False, True}
    assert set(parent.files) == {n + s for n in BC.CASES for s in ("__rows", "__digests")}


@pytest.mark.parametrize("name", list(BC.CASES))
def test_kaldi_bits(pkg, parent, name):
    got = BC.run_case(pkg, name)
    frames = [len(g) for g in got]
    full, want_full = BC.shortest_bits(got), parent[name + "__rows"]
    assert full.shape == want_full.shape, (name, full.shape, want_full.shape)
    diff = full != want_full
    if diff.any():
        row, col = (int(v[0]) for v in np.nonzero(diff))
        for u in BC.shortest(got):
            if row < frames[u]:
                break
            row -= frames[u]
        pytest.fail("%s: %d elements of the shortest utterances differ from the parent's rows (first: utterance %d of %d frames, "
                    "row %d, column %d)" % (name, int(diff.sum()), u, frames[u], row, col))
    d, want_d = BC.digests(got), parent[name + "__digests"]
    assert d.shape == want_d.shape, (name, d.shape, want_d.shape)
    bad = np.nonzero(d != want_d)[0]
    if bad.size:
        ends = np.cumsum(frames)
        u = int(np.searchsorted(ends, bad[0], side="right"))
        pytest.fail("%s: %d rows differ from the parent's; the first is row %d of utterance %d (%d frames)" % (
            name, bad.size, int(bad[0] - (ends[u] - frames[u])), u, frames[u]))
