"""Helpers the GPU suites of the Kaldi front end share (tests/test_kaldi_gpu.py, test_kaldi_sessions_gpu.py,
test_kaldi_windows_gpu.py, test_kaldi_compose_gpu.py) and the host module test_kaldi_windows_host.py: handles, the
float64 oracle of tests/kaldi_ref.py at a handle's shape and options, and the comparison at the project bar.  Test infrastructure
only."""
import numpy as np

import kaldi_ref as KR
from conftest import assert_close


class Shape:
    """W / S / M / C at a sample rate, band edges and lifter; the three frame options; the window by name (kaldi_ref.WINDOWS)."""

    def __init__(self, W, S, M, C, sr=16000.0, low=20.0, high=0.0, Q=22.0, preemph=0.97, remove_dc=True, use_power=True, window="povey"):
        assert window in KR.WINDOWS, window
        self.W, self.S, self.M, self.C, self.sr, self.low, self.high, self.Q = W, S, M, C, sr, low, high, Q
        self.preemph, self.remove_dc, self.use_power, self.window = preemph, remove_dc, use_power, window

    @property
    def cols(self):
        return self.C or self.M

    def id(self):
        return "%d-%d-%d-%d" % (self.W, self.S, self.M, self.C)

    def options(self, **kw):
        s = Shape(self.W, self.S, self.M, self.C, self.sr, self.low, self.high, self.Q, self.preemph, self.remove_dc, self.use_power,
                  self.window)
        for k, v in kw.items():
            setattr(s, k, v)
        return s

    def taps(self):
        """The W taps of the shape's window, float32: what make() sets and oracle() reads."""
        return KR.WINDOWS[self.window](self.W)

    def oracle(self, pcm, energies=False):
        return KR.features(pcm, self.taps(), self.S, self.M, self.sr, self.low, self.high, self.C, self.Q, self.preemph,
                           self.remove_dc, self.use_power, energies=energies)

    def frames(self, n):
        return KR.frame_count(n, self.W, self.S)


FBANK80 = Shape(400, 160, 80, 0)
MFCC13 = Shape(400, 160, 23, 13)


def make(pkg, sh, norm=0, dyn=0, l1=2, l2=2, nad=True, ibs=200000, flags=0, floor=0.0):
    """A Kaldi handle of the shape under the shape's window and options (flags, floor: kaldi_flags and kaldi_energy_floor)."""
    m = pkg.MfccHip(ibs, sh.W, sh.S, sh.M, sh.sr, sh.low, sh.high, sh.C, False, sh.Q, norm, dyn, l1, l2, nad, device=0, bug_compat=False,
                    method=pkg.METHOD_KALDI, kaldi_flags=flags, kaldi_energy_floor=floor)
    m.set_window(pkg.povey_window(sh.W) if sh.window == "povey" else sh.taps())
    m.kaldi_set_options(sh.preemph, sh.remove_dc, sh.use_power)
    return m


def check(got, want, what):
    """At the project bar; returns (max err / scale, rel L2)."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, "%s: shape %s vs %s" % (what, got.shape, want.shape)
    if want.size == 0:
        return 0.0, 0.0
    scale = max(np.abs(want).max(), 1e-30)
    emax = np.abs(got.astype(np.float64) - want).max() / scale
    el2 = np.linalg.norm(got - want) / max(np.linalg.norm(want), 1e-30)
    print("%s: max err / scale = %.3g, rel L2 = %.3g (scale %.3g)" % (what, emax, el2, scale))
    assert_close(got, want, what)
    return emax, el2
