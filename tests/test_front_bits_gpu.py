"""The register front ends, one case per family of instantiations (MI355X, through the batch entry): k_front512's unaligned,
512-tap, stereo, stuffed + stereo, 128- and 64-point, spectrum-only and fused-delta builds, k_front1024's 16- and 12-wave,
unaligned, long-window and no-DCT builds, k_front2048's stereo, mono, any-alignment, 20-row and 32-row builds
(tests/front_bits_cases.py) -- the families tests/test_mel_rounds_gpu.py does not reach.  Per case: the kernel the run
reports, rows finite and at the project's bar against the oracle (mono; a transform longer than the window's power of two as a
window of that many taps with a zero tail, as tests/test_parity_gpu.py does) or, where the oracle does not serve the shape
(stereo), against the float64 reference of tests/edge_signals.py at its bars, and every element bit for bit the row recorded
from commit 64dcbfe on the same GPU (tests/golden/front_bits_parent.npz, written by tests/golden/make_front_bits_parent.py).
The change after that commit moved code between files without changing an instruction of any instantiation
(profiles/r06/README.md); the recorded rows hold the next change of these kernels to the same."""
import os

import numpy as np
import pytest

import edge_signals as ES
import front_bits_cases as FC
from conftest import GOLDEN, assert_close

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def parent_rows():
    return np.load(os.path.join(GOLDEN, "front_bits_parent.npz"))


def test_one_case_per_family():
    kernels = [k for _, k, _ in FC.CASES.values()]
    assert (kernels.count("k_front512"), kernels.count("k_front1024"), kernels.count("k_front2048")) == (8, 6, 5)
    assert [n for n, (sh, _, _) in FC.CASES.items() if FC.fused_wave_runs(sh)] == ["f512_c2_fuse_delta"]


@pytest.mark.parametrize("name", list(FC.CASES))
def test_front_bits(pkg, orc, parent_rows, name):
    sh, kernel, why = FC.CASES[name]
    if sh["engine"] & FC.ENGINE_FUSE_DELTA:
        assert FC.fused_wave_runs(sh), "%s: the plan does not take the fused delta wave" % name
    rows, first, ran = FC.run_batch(pkg, sh)
    assert ran == kernel, "%s (%s): the run reports %s" % (name, why, ran)
    frames, groups = sh["frames"], 1 + sh["dyn"]
    assert rows.shape == (sum(frames), FC.cols(sh)) and np.isfinite(rows).all()

    window = pkg.reference_window(sh["W"])
    utts = FC.utterances(sh)
    if sh["ch"] == 1:
        W2 = sh["fft"] or sh["W"]
        w_o = np.zeros(W2, np.float32)
        w_o[:sh["W"]] = window
        cfg = orc.make_config(200 * sh["S"] + W2, window_size=W2, shift=sh["S"], num_banks=sh["nb"], sample_rate=sh["sr"],
                              ceps_len=sh["nc"], want_c0=sh["c0"], dyn=sh["dyn"], delta_l1=3, delta_l2=3)
        for u, r0, f in zip(utts, first, frames):
            want = orc.run_utterance(cfg, np.concatenate([u[:, 0], np.zeros(W2 - sh["W"], np.int16)]), w_o, bug_compat=False)
            assert_close(rows[r0:r0 + f], want, "%s, utterance of %d frames" % (name, f), groups=groups)
    else:
        assert sh["dyn"] == FC.DYN_NONE
        for u, r0, f in zip(utts, first, frames):
            c, mel = ES.reference(u, window, sh["W"], sh["S"], sh["fft"], sh["nb"], sh["sr"], 64.0, sh["sr"] / 2, sh["nc"], sh["c0"], 22.0,
                                  channels=2)
            ES.assert_rows_close(rows[r0:r0 + f], c, mel, "%s, utterance of %d frames" % (name, f))

    assert np.array_equal(parent_rows[name + "__first_rows"], np.asarray(first, np.int32))
    got = np.ascontiguousarray(rows, np.float32).view(np.int32)
    diff = got != parent_rows[name]
    assert not diff.any(), "%s: %d elements differ from the parent's rows (first: row %d, column %d)" % (
        name, int(diff.sum()), *[int(v[0]) for v in np.nonzero(diff)])
