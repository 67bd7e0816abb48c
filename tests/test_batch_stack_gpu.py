"""The batch entries with everything attached at once: a rates plan, per-utterance warp factors, a speaker list and a splice +
affine transform on the 512-point MFCC + d + dd shape (CVN after the deltas), over utterances of 0 .. 130 frames.

The three entries must deliver the same bits; a new plan must drop all four attachments in one go; a refused plan must leave
all four as they were.  Every comparison is of bits (int32 views of the float32 rows) or of status codes: no tolerance."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

W, S, OUT_HZ = 400, 160, 16000
FRAMES = (0, 1, 15, 16, 17, 64, 65, 130)
RATES = [(OUT_HZ, 8000, 48000)[i % 3] for i in range(len(FRAMES))]
OUT_DIM = 24


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.int32)


def stack_handle(pkg):
    m = pkg.MfccHip(200000, W, S, 40, float(OUT_HZ), 64.0, OUT_HZ / 2, 13, False, 22.0, pkg.NORM_CVN, pkg.DYN_ACC, 3, 3, True, device=0)
    m.set_window(pkg.reference_window(W))
    return m


def batch():
    """(pcm, offsets, lengths) in input-rate samples: utterance i arrives at RATES[i] and converts to about FRAMES[i] frames."""
    from conftest import synth_utterance
    out_len = [W // 2 if t == 0 else W + (t - 1) * S + 7 * i for i, t in enumerate(FRAMES)]
    lens = [(-(-n * r // OUT_HZ) + 1) & ~1 for n, r in zip(out_len, RATES)]
    offs = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
    pcm = np.concatenate([synth_utterance(n, 700 + i, sr=float(r)) for i, (n, r) in enumerate(zip(lens, RATES))] + [np.zeros(2, np.int16)])
    return pcm, offs, np.asarray(lens, np.int64)


def attach_all(m, offs, lens):
    _, total = m.batch_plan_rates(offs, lens, RATES)
    n, wd = len(lens), m.get_output_data_width()
    m.batch_set_alphas(np.array([0.9, 1.0, 1.1], np.float32)[np.arange(n) % 3])
    m.batch_set_speakers(np.arange(n, dtype=np.int32) % 3, n_spk=3)
    rng = np.random.default_rng(5)
    m.batch_set_transform((0.1 * rng.standard_normal((2, OUT_DIM, 5 * wd))).astype(np.float32),
                          rng.standard_normal((2, OUT_DIM)).astype(np.float32), left=2, right=2, utt_xf=np.arange(n, dtype=np.int32) % 2)
    return total


def run_device(m, pcm, total):
    import torch
    dev = torch.device("cuda:0")
    d_pcm = torch.from_numpy(pcm).to(dev)
    d_out = torch.zeros((total, m.batch_output_width()), dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    m.batch_run_device(d_pcm.data_ptr(), pcm.size, d_out.data_ptr())
    m.synchronize()
    return d_out.cpu().numpy()


def status_of(pkg, fn, *args):
    try:
        fn(*args)
    except pkg.MfxError as e:
        return e.status
    return 0


@pytest.fixture(scope="module")
def stack(pkg):
    """A handle with all four attachments in force, its batch, and the rows of the device entry."""
    pcm, offs, lens = batch()
    m = stack_handle(pkg)
    total = attach_all(m, offs, lens)
    yield m, pcm, offs, lens, total, run_device(m, pcm, total)
    m.close()


def test_three_entries_same_bits(pkg, stack):
    m, pcm, offs, lens, total, want = stack
    assert total > sum(FRAMES) - len(FRAMES) and want.shape == (total, OUT_DIM) and np.isfinite(want).all() and np.abs(want).max() > 0
    assert np.array_equal(bits(m.batch_run_host(pcm)), bits(want)), "pageable host entry"
    m.batch_overlap(True)
    try:
        for i in range(2):
            assert np.array_equal(bits(run_device(m, pcm, total)), bits(want)), "overlap on, batch %d" % i
    finally:
        m.batch_overlap(False)


def test_refused_plan_leaves_every_attachment(pkg, stack):
    m, pcm, offs, lens, total, want = stack
    bad = lens.copy()
    bad[3] = -1
    assert status_of(pkg, m.batch_plan, offs, bad) == -7
    m._plan_total = total                                       # (the Python mirror's copy; the refused call never set it)
    assert m.batch_output_width() == OUT_DIM
    assert m.batch_resample_layout()[2] > 0
    assert np.array_equal(bits(run_device(m, pcm, total)), bits(want)), "rows after a refused plan"
    assert 0 < m.batch_speaker_stats()[0].sum() <= total        # (answered: the list is in force and has run)
    assert np.array_equal(bits(m.batch_run_host(pcm)), bits(want))


def test_new_plan_drops_every_attachment(pkg):
    pcm, offs, lens = batch()
    m, fresh = stack_handle(pkg), stack_handle(pkg)
    try:
        total = attach_all(m, offs, lens)
        run_device(m, pcm, total)
        assert m.batch_output_width() == OUT_DIM and 0 < m.batch_speaker_stats()[0].sum() <= total
        _, total = m.batch_plan(offs, lens)
        _, total_f = fresh.batch_plan(offs, lens)
        assert total == total_f
        assert m.batch_output_width() == fresh.batch_output_width() == m.get_output_data_width() == 39
        assert status_of(pkg, m.batch_resample_layout) == status_of(pkg, fresh.batch_resample_layout) == -8
        assert status_of(pkg, m.batch_speaker_stats) == status_of(pkg, fresh.batch_speaker_stats) == -8
        assert m.dominant_kernel_name() == fresh.dominant_kernel_name() == "k_front512"
        assert np.array_equal(bits(run_device(m, pcm, total)), bits(run_device(fresh, pcm, total_f))), "rows of the bare plan"
    finally:
        m.close(), fresh.close()
