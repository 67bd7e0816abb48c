"""The two sample-rate converters, one case per path (MI355X; tests/resample_bits_cases.py): k_resample at every R, with the
table staged and unstaged, under 64 KB of LDS and over, mono and stereo, on the ragged batch of tests/test_resample_gpu.py; and
k_sess_resample on one stream cut three ways, with whole-word groups of the caller's array and of the carry slot, the five-word
form, the seam, move-only tiles and a push that mixes a converting and a pass-through session.  Per case: the library names the
geometry the case is there for, a session cut takes the paths it is there for, and every converted sample is bit for bit the one
recorded from commit 7d4edbf on the same GPU (tests/golden/resample_bits_parent.npz, written by
tests/golden/make_resample_bits_parent.py).  The change after that commit gave the two kernels one tile body; the recorded
samples hold the next change to the same."""
import os

import numpy as np
import pytest

import resample_bits_cases as BC
from conftest import GOLDEN

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def parent():
    return np.load(os.path.join(GOLDEN, "resample_bits_parent.npz"))


def test_the_fixture_holds_every_case_and_nothing_else(parent):
    assert sorted(parent.files) == sorted({c["stored"] for c in BC.CASES.values()})


@pytest.mark.parametrize("name", list(BC.CASES))
def test_resample_bits(pkg, parent, name):
    c = BC.CASES[name]
    assert BC.geometry(pkg, c) == c["want"]
    if c["kind"] == "session":
        assert BC.needed(c) <= BC.paths(pkg, c), (name, BC.paths(pkg, c))
    got, want = BC.run_case(pkg, name), parent[c["stored"]]
    assert got.dtype == want.dtype == np.int16 and got.shape == want.shape, (name, got.shape, want.shape)
    diff = np.nonzero(got != want)
    if diff[0].size:
        pytest.fail("%s: %d samples differ from the parent's; the first is sample %d, channel %d: %d, recorded %d" % (
            name, diff[0].size, diff[0][0], diff[1][0], got[diff[0][0], diff[1][0]], want[diff[0][0], diff[1][0]]))
