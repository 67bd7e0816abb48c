"""The energy and HTK options of the Kaldi front end (kaldi_flags of mfx_create_kaldi) through the session entries on the MI355X:
USE_ENERGY raw and windowed, with and without HTK_COMPAT, on MFCC-13 + d + dd and on fbank-23 + energy.  The rows of every
stream are the bits the batch entries write for it as one utterance, under three cuts -- one push, pushes of 100 ms, and pushes
of 1 / 0 / 159 / 161 samples across the frame boundaries --, and once more under the online normaliser.  (NO_SNIP_EDGES is
refused by mfx_sessions_create: tests/test_kaldi_opts_gpu.py.)"""
import numpy as np
import pytest

import onorm_drive as OD
from conftest import synth_utterance
from kaldi_drive import Shape
from stft_drive import run_batch, same_bits
from test_kaldi_opts_gpu import EN, HTK, WIN, make

pytestmark = pytest.mark.gpu

W, S = 400, 160
LENGTHS = [399, W, W + 6 * S + 81, W + 17 * S + 159]          # 0, 1, 7 and 18 frames
MAX_PUSH = max(LENGTHS)
FLAGS = {"raw": EN, "windowed": EN | WIN, "raw_htk": EN | HTK, "windowed_htk": EN | WIN | HTK}
CONFIGS = {"mfcc13_d_dd": (Shape(W, S, 23, 13), dict(dyn=2, l1=2, l2=2)), "fbank23": (Shape(W, S, 23, 0), dict())}


def cut_100ms(left, S_, rng):
    n = min(1600, left)
    return n, n == left


class CutAcrossFrames:
    """1, 0, 159, 161 samples, over and over: pushes that end one sample into a hop, empty ones, one short of and one past a hop."""

    def __init__(self):
        self.k = 0

    def __call__(self, left, S_, rng):
        n = min((1, 0, 159, 161)[self.k & 3], left)
        self.k += 1
        return n, n == left


CUTS = {"whole": lambda: OD.cut_whole, "100ms": lambda: cut_100ms, "1_0_159_161": CutAcrossFrames}


def streams():
    return [synth_utterance(n, 600 + i) for i, n in enumerate(LENGTHS)]


@pytest.fixture(scope="module")
def twins(pkg):
    """(config, flags) -> the batch rows of every stream, plain and under the online normaliser"""
    out = {}
    for name, (sh, kw) in CONFIGS.items():
        for fname, flags in FLAGS.items():
            m = make(pkg, sh, flags, **kw)
            plain = run_batch(m, streams())
            m.close()
            m = make(pkg, sh, flags, norm=1, **kw)
            offs = np.cumsum([0] + LENGTHS[:-1]).astype(np.int64)
            rows, total = m.batch_plan(offs, LENGTHS)
            m.batch_set_online_norm(64)
            y = m.batch_run_host(np.concatenate(streams() + [np.zeros(2, np.int16)]))
            online = [y[rows[i]:rows[i] + m.batch_frames(n)] for i, n in enumerate(LENGTHS)]
            m.close()
            assert [p.shape[0] for p in plain] == [0, 1, 7, 18] == [o.shape[0] for o in online]
            out[name, fname] = (plain, online)
    return out


@pytest.mark.parametrize("cut", sorted(CUTS))
@pytest.mark.parametrize("fname", sorted(FLAGS))
@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_session_rows_are_the_batch_twins_bits(pkg, twins, name, fname, cut):
    sh, kw = CONFIGS[name]
    utts = [u.reshape(-1, 1) for u in streams()]
    m = make(pkg, sh, FLAGS[fname], **kw)
    assert m.get_output_data_width() == (39 if sh.C else 24)
    m.sessions_create(3, MAX_PUSH)
    for odd in (False, True):
        got = OD.drive(m, utts, 3, CUTS[cut](), seed=7 + odd, odd_offsets=odd)
        for u, want in enumerate(twins[name, fname][0]):
            assert same_bits(got[u], want), "%s, %s, %s, odd offsets %d: stream %d differs from its batch rows" % (name, fname, cut, odd, u)
    m.close()


@pytest.mark.parametrize("cut", sorted(CUTS))
@pytest.mark.parametrize("fname", ("raw", "windowed_htk"))
@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_session_online_norm_rows_are_the_batch_attachments_bits(pkg, twins, name, fname, cut):
    sh, kw = CONFIGS[name]
    utts = [u.reshape(-1, 1) for u in streams()]
    m = make(pkg, sh, FLAGS[fname], norm=1, **kw)
    m.sessions_set_online_norm(64)
    m.sessions_create(3, MAX_PUSH)
    got = OD.drive(m, utts, 3, CUTS[cut](), seed=11)
    m.close()
    plain, online = twins[name, fname]
    for u, want in enumerate(online):
        assert same_bits(got[u], want), "%s, %s, %s: stream %d differs from the batch attachment's rows" % (name, fname, cut, u)
    assert not same_bits(online[3], plain[3])                        # (the normaliser did move the rows)
