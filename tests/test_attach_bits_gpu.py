"""What is attached to a planned batch, bit for bit against the commit before the attachments got one utterance tiling for
host and kernels (MI355X; tests/attach_bits_cases.py): the VAD's flags, counts, thresholds, packed_row0 and rows, the online
normaliser's rows, the pitch track with every NCCF row, the pitch features alone and pasted, a speaker list's rows and
statistics, and all of pitch paste, online normaliser and selecting VAD together -- every batch with utterance lengths on,
before and behind the item edges of its tiling, through the device entry.  tests/golden/attach_bits_parent.npz was written by
tests/golden/make_attach_bits_parent.py from commit da4d973's library on the same GPU: float rows of the short utterances as
bit patterns, an 8-byte digest of every row, the integer arrays whole.  The change after that commit moved index arithmetic
only (profiles/r08/README.md), so there is no tolerance: a difference is an edited expression to be found.  The runs over
utterance ranges are held by the sliced-path tests of test_vad_gpu.py, test_onorm_gpu.py, test_pitch_gpu.py and
test_pitchfeat_gpu.py, which compare them with the whole-batch run of the same handle."""
import os

import numpy as np
import pytest

import attach_bits_cases as AC
from conftest import GOLDEN

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def parent():
    return np.load(os.path.join(GOLDEN, "attach_bits_parent.npz"))


def test_the_cases_sit_on_the_item_edges():
    """The lengths follow from the item sizes: the pitch cases from the tile the handle chooses, one lag range per group count."""
    assert AC.tile_frames(160) == AC.tile_frames(280) == 64
    for name, lag_max in (("pitch_two_groups", 160), ("pitch_one_group", 280)):
        tf = AC.tile_frames(lag_max)
        assert AC.CASES[name]["frames"] == (1, tf - 1, tf, tf + 1, 2 * tf + 1)
    assert AC.pitch_groups(40, 160) == 2 and AC.pitch_groups(40, 280) == 1
    for frames, item in ((AC.VAD_FRAMES, 64), (AC.ONORM_FRAMES, 32), (AC.FEAT_FRAMES, 256)):
        assert {item - 1, item, item + 1} <= set(frames), (frames, item)
    assert 4097 in AC.VAD_FRAMES and {4096, 4097, 8200} <= set(AC.SPK_FRAMES)      # (one row, and a few, behind a chunk of 4096)
    assert max(sum(c["frames"]) for c in AC.CASES.values()) <= 17000


def test_the_fixture_holds_every_case(parent):
    assert {k.split("__")[0] for k in parent.files} == set(AC.CASES)


@pytest.mark.parametrize("name", list(AC.CASES))
def test_attach_bits(pkg, parent, name):
    got = AC.record(pkg, name)
    want = {k[len(name) + 2:]: parent[k] for k in parent.files if k.startswith(name + "__")}
    assert sorted(got) == sorted(want), (name, sorted(got), sorted(want))
    for key in sorted(got):     # (every array is looked at: the message names all that differ)
        assert got[key].shape == want[key].shape and got[key].dtype == want[key].dtype, (name, key, got[key].shape, want[key].shape)
    bad = {key: int((got[key] != want[key]).sum()) for key in sorted(got) if (got[key] != want[key]).any()}
    assert not bad, "%s: elements that differ from the parent's, by array: %s" % (name, bad)
