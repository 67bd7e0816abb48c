"""k_stft_mel and k_stft_post on the MI355X under windows that weigh every tap (tests/stft_edge.py): the edge signals of
tests/edge_signals.py against the float64 oracle of tests/stft_ref.py at one absolute bar per window, one-hot windows that
name the sample every probed tap reads, and the maximum of k_stft_post over more than 256 blocks.  Every test prints its
worst error over its bar; tests/test_stft_edge_host.py derives the bars and the conditions on the CPU."""
import numpy as np
import pytest

import edge_signals as ES
import stft_edge as SE
import stft_ref
from stft_drive import MATRIX, bits, same_bits

pytestmark = pytest.mark.gpu

IDS = [SE.shape_id(s) for s in SE.SHAPES]


def make(pkg, shape, window, post=SE.LOG10):
    return MATRIX.make(pkg, *shape, window=window, post=post)


def block_rows(pkg, shape):
    return MATRIX.block_rows(pkg, *shape[:3])


def run(m, utts, first=0, order=None):
    """One batch through mfx_batch_run_device, utterances back to back from sample `first` in the given order, the output
    between guard words; every utterance's rows in the ORIGINAL order."""
    import torch
    order = list(range(len(utts))) if order is None else list(order)
    lens = np.array([utts[i].size for i in order], np.int64)
    offs = first + np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
    fill = lambda k: np.full(k, 0x5A5A, np.int16)                                                  # noqa: E731
    pcm_h = np.concatenate([fill(first)] + [utts[i] for i in order] + [fill(2 + (first + int(lens.sum())) % 2)])
    rows, total = m.batch_plan(offs, lens)
    M = m.batch_output_width()
    dev = torch.device("cuda", 0)
    pcm = torch.from_numpy(pcm_h).to(dev)
    lead = 32
    big = torch.full((lead + total * M + 64,), float("nan"), dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    m.batch_run_device(pcm.data_ptr(), pcm_h.size, big.data_ptr() + 4 * lead)
    m.synchronize()
    b = big.cpu().numpy()
    assert np.isnan(b[:lead]).all() and np.isnan(b[lead + total * M:]).all(), "guard words written"
    out = b[lead:lead + total * M].reshape(total, M)
    got = [None] * len(utts)
    for j, i in enumerate(order):
        got[i] = out[rows[j]:rows[j] + m.batch_frames(int(lens[j]))].copy()
    return got


# ---- 1. edge signals ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("window", SE.WINDOWS)
@pytest.mark.parametrize("shape", SE.SHAPES, ids=IDS)
def test_edge_signals(pkg, shape, window):
    N, S, M, sr, low, high = shape
    ref = SE.shape_reference(shape, window)
    names = list(ref)
    utts = [ref[n]["pcm"] for n in names]
    bar = SE.BARS[window]
    m = make(pkg, shape, SE.windows(N)[window])
    got = run(m, utts)
    moved = run(m, utts, first=1, order=range(len(utts) - 1, -1, -1))
    m.close()
    worst = max(SE.errors(g, ref[n]["want"], ref[n]["ok"])[0] for n, g in zip(names, got))
    held = min(ref[n]["ok"].mean() for n in names)
    print("\n%s %s: worst |d L| %.3g / bar %.3g = %.3f (least held share of a signal %.2f)" % (
        SE.shape_id(shape), window, worst, bar, worst / bar, held))
    for n, g in zip(names, got):
        assert g.shape == (stft_ref.frame_count(ref[n]["pcm"].size, N, S), M)
        SE.assert_rows(g, ref[n]["want"], bar, "%s %s, %s" % (SE.shape_id(shape), window, n), ok=ref[n]["ok"])
    # identical frames -> identical bits, on the frames that read no reflected sample
    for n in ES.identical_frame_signals(S, sr):
        g = got[names.index(n)]
        a, b, step = SE.identical_rows(n, ref[n]["pcm"].size, N, S)
        assert b - a >= 30
        for k in range(step):
            part = bits(g[a + k:b:step])
            assert (part == part[:1]).all(), "%s %s, %s: rows of identical frames differ" % (SE.shape_id(shape), window, n)
    # the batch in reverse order from an odd first sample
    for n, g, h in zip(names, got, moved):
        assert same_bits(g, h), "%s %s, %s: rows depend on the utterance's place in the batch" % (SE.shape_id(shape), window, n)


@pytest.mark.parametrize("window", SE.WINDOWS)
def test_edge_signals_ln_and_whisper(pkg, window):
    """The default shape under LN (the bar times ln 10; the floor within 2 ulp of ln 1e-10f) and WHISPER (bar / 4 after the
    map's division by 4; the clamp and the map against the LOG10 rows as test_stft_gpu.test_post_modes does)."""
    shape = SE.SHAPES[0]
    N, S, M, sr, low, high = shape
    ref = SE.shape_reference(shape, window)
    names = list(ref)
    utts = [ref[n]["pcm"] for n in names]
    bar = SE.BARS[window]
    rows = {}
    for post in (SE.LOG10, SE.LN, SE.WHISPER):
        m = make(pkg, shape, SE.windows(N)[window], post)
        rows[post] = run(m, utts)
        m.close()
    worst_ln = worst_wh = 0.0
    for i, n in enumerate(names):
        want, ok = ref[n]["want"], ref[n]["ok"]
        l10, ln, wh = rows[SE.LOG10][i], rows[SE.LN][i], rows[SE.WHISPER][i]
        assert np.isfinite(ln).all() and np.isfinite(wh).all()
        floor = want == SE.FLOOR_WANT
        held = ok & ~floor
        d = np.abs(ln.astype(np.float64) - want * np.log(10.0))
        worst_ln = max(worst_ln, d[held].max(initial=0.0))
        ulp = np.abs(ln[floor].view(np.int32).astype(np.int64) - int(SE.FLOOR_LN.view(np.int32)))
        assert ulp.max(initial=0) <= SE.LN_FLOOR_ULPS, "%s %s: LN floor %d ulp off" % (window, n, ulp.max())
        # WHISPER against the oracle's own map; the clamp's level is the utterance's largest value, itself within the bar
        wmap = (np.maximum(want, want.max() - 8.0) + 4.0) / 4.0
        clamped = want <= want.max() - 8.0
        dw = np.abs(wh.astype(np.float64) - wmap)
        worst_wh = max(worst_wh, dw[held | clamped].max(initial=0.0))
        mapped = (np.maximum(l10, l10.max() - np.float32(8.0)) + np.float32(4.0)) * np.float32(0.25)
        u = np.abs(mapped.view(np.int32).astype(np.int64) - wh.view(np.int32).astype(np.int64))
        assert u.max() <= 2, "%s %s: WHISPER rows %d ulp from the map of the LOG10 rows" % (window, n, u.max())
    print("\n%s %s: LN worst %.3g / %.3g = %.3f; WHISPER worst %.3g / %.3g = %.3f" % (
        SE.shape_id(shape), window, worst_ln, bar * np.log(10.0), worst_ln / (bar * np.log(10.0)), worst_wh, bar / 4, worst_wh / (bar / 4)))
    assert worst_ln <= bar * np.log(10.0)
    assert worst_wh <= bar / 4


# ---- 2. tap probes --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", SE.SHAPES, ids=IDS)
def test_tap_probes(pkg, shape):
    N, S, M, sr, low, high = shape
    R = block_rows(pkg, shape)
    utts = [SE.probe_signal(n) for n in SE.probe_lengths(N, S, R)]
    table = stft_ref.mel_table(M, N, sr, low, high)[0].astype(np.float64)
    m = make(pkg, shape, SE.onehot(N, 0))
    worst, misses = 0.0, []
    for j in SE.probe_taps(N):
        w = SE.onehot(N, j)
        m.set_window(w)
        got = run(m, utts)
        b = stft_ref.basis(w).astype(np.float64)[:, :, j]
        with np.errstate(divide="ignore"):
            rowsum = np.log10(table @ (b[0] ** 2 + b[1] ** 2))
        for u, g in zip(utts, got):
            want = stft_ref.logmel(u, w, S, M, sr, low, high, SE.LOG10)
            assert g.shape == want.shape and np.isfinite(g).all()
            floor = want == SE.FLOOR_WANT
            assert (g[floor] == SE.FLOOR_L10).all(), "tap %d: floor entries are not -10.0f" % j
            d = np.where(floor, 0.0, np.abs(g.astype(np.float64) - want))
            worst = max(worst, d.max(initial=0.0))
            band = int(np.argmax(np.isfinite(rowsum)))
            idx = stft_ref.frame_index(u.size, N, S)[:, j]
            for t in np.nonzero(d.max(axis=1) > SE.ONEHOT_BAR)[0]:
                misses.append("tap %d, %d samples, frame %d: |d L| %.3g; the row reads sample = %d (mod 193), the frame rule "
                              "sample %d = %d (mod 193)" % (j, u.size, t, d[t].max(), SE.probe_decode(float(g[t, band]), rowsum[band]),
                                                            idx[t], idx[t] % SE.PROBE_PERIOD))
    m.close()
    print("\n%s one-hot probes: worst |d L| %.3g / bar %.3g = %.3f" % (SE.shape_id(shape), worst, SE.ONEHOT_BAR, worst / SE.ONEHOT_BAR))
    assert not misses, "%d rows miss the one-hot bar:\n%s" % (len(misses), "\n".join(misses[:20]))


# ---- 3. the maximum of k_stft_post over more than 256 blocks -----------------------------------------------------------------

def test_whisper_maximum_beyond_256_blocks(pkg):
    shape = (32, 1, 4, 16000.0, 0.0, 8000.0)
    N, S, M = shape[:3]
    R = block_rows(pkg, shape)
    rng = np.random.default_rng(0xB10C)
    n = 300 * R * S
    long = rng.integers(-1, 2, n).astype(np.int16)  # +-1 LSB: every band below the 1e-10 floor
    at = 299 * R * S + R // 2                       # inside block 299: the second trip of the stride of 256 slots
    long[at:at + 24] = np.where(rng.integers(0, 2, 24) == 1, 32767, -32768)
    short = rng.integers(-300, 301, 5 * R + 7).astype(np.int16)
    w = SE.windows(N)["ramp"]
    m = make(pkg, shape, w, SE.WHISPER)
    both = run(m, [long, short])
    alone = run(m, [short])[0]
    m.close()
    assert both[0].shape[0] == 300 * R and -(-both[0].shape[0] // R) > 256
    want = stft_ref.logmel(long, w, S, M, *shape[3:], SE.LOG10)
    top = want.max()
    # the clamp's level comes from a block beyond the first 256 and lies a quarter of a decade above everything in front of it
    assert top == want[299 * R:].max() and want[:299 * R].max() < top - 8.0 - 0.25
    bar = SE.BARS["ramp"] / 4
    worst = 0.0
    for u, g in ((long, both[0]), (short, both[1])):
        wh = stft_ref.logmel(u, w, S, M, *shape[3:], SE.WHISPER)
        assert g.shape == wh.shape and np.isfinite(g).all()
        ok = SE.sensitivity(u, w, S, M, *shape[3:]) <= SE.COND_TOL10
        l10 = stft_ref.logmel(u, w, S, M, *shape[3:], SE.LOG10)
        ok |= l10 <= l10.max() - 8.0                 # (clamped entries: the level, not their own value)
        worst = max(worst, np.abs(g.astype(np.float64) - wh)[ok].max())
    print("\nWHISPER over %d blocks: worst |d out| %.3g / bar %.3g = %.3f" % (300, worst, bar, worst / bar))
    assert worst <= bar
    level = (np.float32(both[0].max()) * np.float32(4.0) - np.float32(8.0)) * np.float32(0.25)       # ((mx - 8) + 4) / 4
    on_clamp = (both[0][:299 * R] == both[0][0, 0]).all() and abs(float(both[0][0, 0]) - float(level)) <= 2.0 ** -22
    assert on_clamp, "the quiet blocks do not sit on the clamp"
    assert same_bits(both[1], alone), "the short utterance's rows depend on its neighbour"
