"""The STFT log-mel kernels, one case per branch (MI355X; tests/stft_bits_cases.py): k_stft_mel at every tile, with one and two
passes over the taps and with padded taps, k_stft_fft_mel at both lengths and tiles, k_stft_post, the three post modes, and
k_sess_stft_mel at both packings beside its plain twin.  Per case: the library names the tile (the packing) the case is there
for, the rows are finite, and every row is bit for bit the row recorded from commit 51f5b97 on the same GPU
(tests/golden/stft_bits_parent.npz, written by tests/golden/make_stft_bits_parent.py: the rows of the three shortest non-empty
utterances in full, an 8-byte digest of every row).  The change after that commit gave the kernels one form rule, one argument
core, one block tail and one overlay; the recorded rows hold the next change to the same.

The FFT form is deliberately NOT tied to a summation order ("STFT log-mel, FFT form"): its cases here guard
refactors.  A change that alters the transform on purpose re-records them with the committed recorder and proves itself
against float64 (tests/test_stft_fft_gpu.py).  The matrix form's chains are pinned by the method itself."""
import os

import numpy as np
import pytest

import stft_bits_cases as BC
from conftest import GOLDEN

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def parent():
    return np.load(os.path.join(GOLDEN, "stft_bits_parent.npz"))


def test_every_case_takes_the_tile_it_names(pkg):
    for name, c in BC.CASES.items():
        assert BC.tile(pkg, c) == c["want"], (name, BC.tile(pkg, c), c["want"])
    batch = {(c["N"] > 512, c["want"]) for c in BC.CASES.values() if c["kind"] == "batch"}
    assert batch == {(False, 64), (False, 32), (True, 16), (True, 8)}
    assert {c["want"] for c in BC.CASES.values() if c["kind"] == "sessions"} == {4, 2}


def test_no_shape_packs_one_group(pkg):
    """The session kernel's block grows with N, S and M, and the largest shape the method accepts still packs 2 groups: no
    case can stand for a packing of 1."""
    assert pkg.mfcc.host_sess_stft_lds_bytes(512, 512, 128) == (125088, 2)


@pytest.mark.parametrize("name", list(BC.CASES))
def test_stft_bits(pkg, parent, name):
    c = BC.CASES[name]
    assert BC.tile(pkg, c) == c["want"]
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
