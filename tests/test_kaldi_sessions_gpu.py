"""The Kaldi front end through the session entries on the MI355X: five streams through three session ids, cut whole, at random
with empty pushes and a flush, and in steps of half a hop -- the rows of every stream are the bits the batch entries write for it
as one utterance, fbank-80 and MFCC + d + dd; and the same under the online normaliser (CMN, N = 64) against the batch
attachment's rows."""
import numpy as np
import pytest

import onorm_drive as OD
from conftest import synth_utterance
from kaldi_drive import FBANK80, MFCC13, make
from stft_drive import run_batch, same_bits

pytestmark = pytest.mark.gpu

W, S = 400, 160
# frames: none (a stream shorter than a window), 1, 7, 18 (into the second chunk), 33 and a remainder each
LENGTHS = [399, W, W + 6 * S + 81, W + 17 * S + 159, W + 32 * S + 1]
MAX_PUSH = max(LENGTHS)

CUTS = {
    "whole": OD.cut_whole,
    "random_empty_and_flush": OD.cut_random_with_empty,
    "half_hop": OD.cut_half_hop,
}

CONFIGS = {
    "fbank80": (FBANK80, dict()),
    "mfcc13_d_dd": (MFCC13, dict(dyn=2, l1=2, l2=2)),
}


def streams():
    return [synth_utterance(n, 500 + i) for i, n in enumerate(LENGTHS)]


@pytest.fixture(scope="module")
def twins(pkg):
    """config -> the batch rows of every stream, plain and under the online normaliser"""
    out = {}
    for name, (sh, kw) in CONFIGS.items():
        m = make(pkg, sh, **kw)
        plain = run_batch(m, streams())
        m.close()
        m = make(pkg, sh, norm=1, **kw)
        offs = np.cumsum([0] + LENGTHS[:-1]).astype(np.int64)
        pcm = np.concatenate(streams() + [np.zeros(2, np.int16)])
        rows, total = m.batch_plan(offs, LENGTHS)
        m.batch_set_online_norm(64)
        y = m.batch_run_host(pcm)
        online = [y[rows[i]:rows[i] + m.batch_frames(n)] for i, n in enumerate(LENGTHS)]
        m.close()
        assert [p.shape[0] for p in plain] == [0, 1, 7, 18, 33] == [o.shape[0] for o in online]
        out[name] = (plain, online)
    return out


@pytest.mark.parametrize("cut", sorted(CUTS))
@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_session_rows_are_the_batch_twins_bits(pkg, twins, name, cut):
    sh, kw = CONFIGS[name]
    utts = [u.reshape(-1, 1) for u in streams()]
    m = make(pkg, sh, **kw)
    m.sessions_create(3, MAX_PUSH)
    for odd in (False, True):
        got = OD.drive(m, utts, 3, CUTS[cut], seed=7 + odd, odd_offsets=odd)
        for u, want in enumerate(twins[name][0]):
            assert same_bits(got[u], want), "%s, %s, odd offsets %d: stream %d differs from its batch rows" % (name, cut, odd, u)
    got = OD.drive(m, utts, 3, CUTS[cut], seed=9, host=True)        # the host entry
    for u, want in enumerate(twins[name][0]):
        assert same_bits(got[u], want), (name, cut, "host entry", u)
    m.close()
    print("%s, %s: %d rows per pass, the batch twin's bits" % (name, cut, sum(w.shape[0] for w in twins[name][0])))


@pytest.mark.parametrize("cut", sorted(CUTS))
@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_session_online_norm_rows_are_the_batch_attachments_bits(pkg, twins, name, cut):
    sh, kw = CONFIGS[name]
    utts = [u.reshape(-1, 1) for u in streams()]
    m = make(pkg, sh, norm=1, **kw)
    m.sessions_set_online_norm(64)
    m.sessions_create(3, MAX_PUSH)
    got = OD.drive(m, utts, 3, CUTS[cut], seed=11)
    m.close()
    plain, online = twins[name]
    for u, want in enumerate(online):
        assert same_bits(got[u], want), "%s, %s: stream %d differs from the batch attachment's rows" % (name, cut, u)
    assert not same_bits(online[4], plain[4])                        # (the normaliser did move the rows)
