"""Session entries on an STFT log-mel handle (k_sess_stft_mel; k_stft_mel under MFX_ENGINE_SESS_STFT_PLAIN) on the MI355X.

The contract (include/mfx.h, MFX_METHOD_STFT_LOGMEL, "Sessions"): the rows of a push are the bits mfx_batch_run_device writes
for the whole stream as one utterance of a handle of the same configuration, however the stream is cut, wherever the pieces
and d_out lie, packed or plain, with the session transform and the session rates; the counts follow the delivery rule.  The
twin's rows themselves are held against the float64 oracle of tests/stft_ref.py at the project bar (conftest.assert_close);
under the windows of tests/stft_edge.py, which weigh every tap -- tap 0 of a frame is the oldest carried sample --, at that
module's bars."""
import numpy as np
import pytest

import sess_inflight as SI
import sess_stft_drive as SD
import stft_edge as SE
import stft_ref
from conftest import assert_close, synth_utterance

pytestmark = pytest.mark.gpu

PLAIN = 8192
# 0 frames: 0, 200 samples; 201 (1 frame), 319 (1), 320 (2), 2559 (15), 2721 (17), 17 hops + 3, 65 hops (more than a block of 64)
LENGTHS = [0, 200, 201, 319, 320, 2559, 2721, 17 * 160 + 3, 65 * 160]
CUTS = {"whole": SD.cut_whole, "hop": SD.cut_step(160), "half_hop": SD.cut_step(80), "random": SD.cut_random,
        "random_empty": SD.cut_random_empty, "singles_across_200": SD.cut_singles_across(200)}


@pytest.fixture(scope="module")
def whisper_case(pkg, a0001):
    """(streams, the batch twin's rows): computed once, read-only."""
    utts = [synth_utterance(n, 300 + i) for i, n in enumerate(LENGTHS)] + [a0001.copy()]
    m = SD.make(pkg)
    want = SD.twins(m, utts)
    m.close()
    for u, w in zip(utts, want):
        assert w.shape == (SD.frames(len(u), 400, 160), 80)
    return utts, want


def test_twin_rows_against_the_float64_oracle(pkg, whisper_case):
    utts, want = whisper_case
    for u, w in zip(utts, want):
        ref = stft_ref.logmel(u, pkg.periodic_hann(400), 160, 80, 16000.0, 0.0, 8000.0, stft_ref.LOG10)
        assert ref.shape == w.shape
        if w.size:
            assert_close(w, ref, "%d samples" % len(u))


@pytest.mark.parametrize("cut", list(CUTS))
def test_whisper_shape_rows_are_the_batch_twins_bits(pkg, whisper_case, cut):
    utts, want = whisper_case
    m = SD.make(pkg)
    m.sessions_create(6, max(len(u) for u in utts))
    got = SD.drive(m, utts, 6, CUTS[cut], 400, 160, seed=7)
    m.close()
    SD.compare(got, want, cut)
    # (the twin passed the project bar above; the same bits pass it too -- held here against the oracle for one stream)
    ref = stft_ref.logmel(utts[6], pkg.periodic_hann(400), 160, 80, 16000.0, 0.0, 8000.0, stft_ref.LOG10)
    assert_close(got[6], ref, cut)


def test_plain_engine_gives_the_same_bits(pkg, whisper_case):
    utts, want = whisper_case
    for cut in ("whole", "random_empty", "singles_across_200"):
        m = SD.make(pkg, engine=PLAIN)
        m.sessions_create(6, max(len(u) for u in utts))
        got = SD.drive(m, utts, 6, CUTS[cut], 400, 160, seed=7)
        m.close()
        SD.compare(got, want, "plain, " + cut)


# N, S, M, post, stream lengths: 512 / 512 packs two groups per block, takes two passes over the taps and has E = n div S while
# open; 32 / 1 has the longest flush, N / 2 - 1 = 15 rows; 400 / 400 has a hop of a whole window; 64 / 24 at 128 bands; the natural log
SHAPES = {"512_512": (512, 512, 80, SD.LOG10, [0, 256, 257, 511, 512, 1023, 1024, 17 * 512 + 5, 40 * 512]),
          "32_1": (32, 1, 20, SD.LOG10, [0, 16, 17, 18, 31, 33, 100, 531]),
          "400_400": (400, 400, 40, SD.LOG10, [200, 201, 399, 400, 401, 800, 17 * 400 + 399]),
          "64_24_m128": (64, 24, 128, SD.LOG10, [32, 33, 47, 48, 49, 16 * 24, 16 * 24 + 9, 33 * 24 + 23]),
          "ln": (400, 160, 80, SD.LN, [201, 320, 2721, 5000])}


@pytest.mark.parametrize("name", list(SHAPES))
def test_shapes_against_their_batch_twins(pkg, name):
    N, S, M, post, lengths = SHAPES[name]
    utts = [synth_utterance(n, 500 + i) for i, n in enumerate(lengths)]
    m = SD.make(pkg, N, S, M, post=post)
    want = SD.twins(m, utts)
    assert [len(w) for w in want] == [SD.frames(n, N, S) for n in lengths]
    # the flush of the longest stream delivers the frames whose right half is reflected: the rule's count, inside its bound
    st = pkg.mfcc.host_session_stft_step(N, S, (0, 0), lengths[-1], False)
    flush = pkg.mfcc.host_session_stft_step(N, S, st["state"], 0, True)["rows"]
    assert flush == SD.frames(lengths[-1], N, S) - SD.delivered_rows(lengths[-1], N, S, False) <= N // (2 * S) + 1
    print("%s: a flush at %d samples delivers %d rows" % (name, lengths[-1], flush))
    m.sessions_create(3, max(lengths))
    cuts = (SD.cut_whole, lambda n, rng: SD.cut_random(n, rng, empty=True, top=max(3 * S, 40)), SD.cut_step(max(S // 2, 1)))
    for k, cut in enumerate(cuts):
        SD.compare(SD.drive(m, utts, 3, cut, N, S, seed=20 + k), want, "%s cut %d" % (name, k))
    m.close()


def test_packing_mixes_sessions_and_splits_at_group_edges(pkg):
    """37 sessions delivering 1 - 3 rows per push beside one that delivers 15, 16, 17 and 40 rows in the same pushes: blocks of
    four groups hold different sessions, and the long session's rows are cut at 16."""
    rng = np.random.default_rng(3)
    hops = [[int(rng.integers(0, 3))] + [int(k) for k in rng.integers(1, 4, 3)] for _ in range(37)] + [[14, 16, 17, 40]]
    # the first push also brings the N / 2 samples its last frame waits for and 7 + i more (no push ends on a hop; every
    # stream has its own length): it delivers one row more than its hops, every later push as many rows as hops
    lens = {}
    for i, h in enumerate(hops):
        c = [h[0] * 160 + 207 + i] + [k * 160 for k in h[1:]]
        lens[sum(c)] = c
    assert len(lens) == 38
    utts = [synth_utterance(n, 700 + i) for i, n in enumerate(lens)]
    m = SD.make(pkg)
    want = SD.twins(m, utts)
    m.sessions_create(38, 41 * 160)

    def cut(n, rng_):
        return [(k, False) for k in lens[n]] + [(0, True)]

    record = []
    got = SD.drive(m, utts, 38, cut, 400, 160, seed=4, record=record)
    m.close()
    SD.compare(got, want, "packing")
    counts = [sorted(int(c) for c in e["counts"]) for e in record[:4]]
    assert [c[-1] for c in counts] == [15, 16, 17, 40] and all(set(c[:-1]) <= {1, 2, 3} for c in counts)
    assert int(record[4]["total"]) == 0                        # (the flushes: every stream ends on a delivered frame)


def test_placement_and_reuse(pkg, whisper_case):
    utts, want = whisper_case
    pick = [2, 4, 5, 6, 7, 8, 3, 1]
    sub, sub_want = [utts[i] for i in pick], [want[i] for i in pick]
    m = SD.make(pkg)
    m.sessions_create(2, 11000)       # two ids for eight streams: every id is reused right after its final push
    SD.compare(SD.drive(m, sub, 2, SD.cut_random_empty, 400, 160, seed=31, odd=True), sub_want, "odd offsets")
    SD.compare(SD.drive(m, sub, 2, SD.cut_random_empty, 400, 160, seed=32, lead=1), sub_want, "d_out 4 bytes off")
    SD.compare(SD.drive(m, sub, 2, SD.cut_random_empty, 400, 160, seed=33, lead=3), sub_want, "d_out 12 bytes off")
    SD.compare(SD.drive(m, sub, 2, SD.cut_random_empty, 400, 160, seed=34, host=True), sub_want, "run_host")
    SD.compare(SD.drive(m, sub, 2, SD.cut_whole, 400, 160, seed=35, shuffle=False), sub_want, "whole streams, ids reused")
    # a batch run between two pushes of an open session: neither disturbs the other
    x = sub[3]
    m.sessions_plan([0], [0], [1000], [0])
    head = m.sessions_run_host(np.concatenate([x[:1000], np.zeros(2, np.int16)]))
    SD.compare(SD.twins(m, sub[:3]), sub_want[:3], "a batch run on the sessions' handle")
    m.sessions_plan([0], [0], [len(x) - 1000], [1])
    tail = m.sessions_run_host(np.concatenate([x[1000:], np.zeros(2, np.int16)]))
    assert len(head) == 6 and SD.same_bits(np.concatenate([head, tail]), sub_want[3])
    m.close()


def test_session_transform_against_the_batch_transform(pkg, whisper_case):
    utts, want = whisper_case
    pick = [1, 2, 4, 5, 6, 7, 8]
    sub = [utts[i] for i in pick]
    rng = np.random.default_rng(77)
    A = (rng.standard_normal((24, 5 * 80)) * 0.05).astype(np.float32)
    b = rng.standard_normal(24).astype(np.float32)
    for engine in (0, PLAIN):
        m = SD.make(pkg, engine=engine)
        twin = SD.twins(m, sub, setup=lambda h: h.batch_set_transform(A, b, left=2, right=2))
        assert all(t.shape == (SD.frames(len(u), 400, 160), 24) for t, u in zip(twin, sub))
        m.sessions_set_transform(A, b, left=2, right=2)
        m.sessions_create(3, 11000)
        assert m.sessions_output_width() == 24
        for k, cut in enumerate((SD.cut_random_empty, SD.cut_step(80), SD.cut_whole)):
            SD.compare(SD.drive(m, sub, 3, cut, 400, 160, seed=40 + k, right=2), twin, "transform, engine %d, cut %d" % (engine, k))
        m.close()


def test_session_rates_against_the_rates_plan(pkg):
    rates = [8000, 44100, 16000]
    lens = [0, 90, 101, 700, 4001, 9000, 551, 553, 3000, 20011]
    hz = [rates[i % 3] for i in range(len(lens))]
    utts = [synth_utterance(n, 800 + i, sr=float(r)) for i, (n, r) in enumerate(zip(lens, hz))]
    m = SD.make(pkg)
    twin = SD.twins(m, utts, rates=hz)
    m.sessions_set_rates(rates)
    m.sessions_create(4, 21000)
    for k, cut in enumerate((SD.cut_random_empty, SD.cut_whole, SD.cut_step(441))):
        got = SD.drive(m, utts, 4, cut, 400, 160, seed=50 + k, predict=False,
                       select=lambda sid, u: ("sessions_select_rate", (sid, u % 3)))
        SD.compare(got, twin, "rates, cut %d" % k)
    m.close()


def test_pushes_in_flight(pkg, whisper_case):
    """One record of the first test's drive replayed through tests/sess_inflight.py on a side stream: no wait between the
    pushes, a filler in front of each, under its share rule."""
    import torch
    utts, want = whisper_case
    sub, sub_want = utts[:9], want[:9]

    def handle():
        h = SD.make(pkg)
        h.sessions_create(4, 11000)
        return h

    record = []
    m = handle()
    SD.compare(SD.drive(m, sub, 4, SD.cut_random_empty, 400, 160, seed=61, record=record), sub_want, "control")
    m.close()
    assert len(record) >= 12
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        filler = SI.Filler()
    m = handle()
    m.set_stream(stream.cuda_stream)
    SI.calibrate(m, record, stream, filler)
    m.close()
    m = handle()
    m.set_stream(stream.cuda_stream)
    try:
        SI.replay(m, record, stream, filler, what="stft log-mel")
    finally:
        m.close()


def test_refusals(pkg):
    m = SD.make(pkg, post=0)                                    # WHISPER: no maximum of an open stream
    with pytest.raises(pkg.MfxError) as e:
        m.sessions_create(2, 1600)
    assert e.value.status == SD.ERR_STATE and "batch" in str(e.value)
    m.close()
    m = SD.make(pkg)
    with pytest.raises(pkg.MfxError) as e:                      # the streaming interface stays refused for every post
        m.set_input(synth_utterance(4000, 1))
    assert e.value.status == SD.ERR_STATE
    m.sessions_create(2, 1600)
    with pytest.raises(pkg.MfxError) as e:
        m.sessions_plan([0], [0], [1601], [0])
    assert e.value.status == SD.ERR_BUFFER
    m.set_alpha(1.1)                                            # no effect
    u = synth_utterance(1600, 2)
    w = SD.twins(m, [u])
    SD.compare(SD.drive(m, [u], 2, SD.cut_step(400), 400, 160, seed=1), w, "after the refusals")
    m.close()
    t = pkg.MfccHip(200000, 400, 160, 15, 16000.0, 64.0, 8000.0, 0, False, 22.0, device=0, bug_compat=False, method=pkg.METHOD_TRAPS)
    t.set_window(pkg.reference_window(400))
    with pytest.raises(pkg.MfxError) as e:
        t.sessions_create(2, 1600)
    assert e.value.status == SD.ERR_STATE
    t.close()


# ---- windows beyond Hann (tests/stft_edge.py): every tap weighs, so a carry one sample short shows -------------------------

EDGE_SHAPES = {"400_160_80": (400, 160, 80), "34_5_6": (34, 5, 6), "416_104_40": (416, 104, 40), "512_512_80": (512, 512, 80)}


def edge_streams(N, S):
    """Streams of N / 2 (no frame), N / 2 + 1, N / 2 + S, 17 S + 3 and 40 S samples: full-range noise and the synthetic
    utterance in turn."""
    rng = np.random.default_rng(N + S)
    lens = [N // 2, N // 2 + 1, N // 2 + S, 17 * S + 3, 40 * S]
    return [rng.integers(-32768, 32768, n).astype(np.int16) if i % 2 == 0 else synth_utterance(n, 900 + i) for i, n in enumerate(lens)]


@pytest.mark.parametrize("window", ["rect", "ramp", "ends"])
@pytest.mark.parametrize("name", list(EDGE_SHAPES))
def test_windows_beyond_hann(pkg, name, window):
    N, S, M = EDGE_SHAPES[name]
    w = SE.windows(N)[window]
    utts = edge_streams(N, S)
    cuts = {"whole": SD.cut_whole, "hop": SD.cut_step(S), "half_hop": SD.cut_step(max(S // 2, 1)), "random_empty": SD.cut_random_empty,
            "singles_across_half": SD.cut_singles_across(N // 2)}
    m = SD.make(pkg, N, S, M, window=w)
    want = SD.twins(m, utts)
    assert [len(t) for t in want] == [SD.frames(len(u), N, S) for u in utts]
    worst, held = 0.0, []
    for u, t in zip(utts, want):
        if len(t):
            ref = stft_ref.logmel(u, w, S, M, 16000.0, 0.0, 8000.0, stft_ref.LOG10)
            ok = SE.sensitivity(u, w, S, M, 16000.0, 0.0, 8000.0) <= SE.COND_TOL10
            held.append(ok.reshape(-1))
            worst = max(worst, SE.assert_rows(t, ref, SE.BARS[window], "%s %s, twin of %d samples" % (name, window, len(u)), ok=ok))
    assert np.concatenate(held).mean() >= 0.99                  # (noise: all but a stray entry is held)
    print("\n%s %s: the twin's worst |d L| %.3g / bar %.3g = %.3f" % (name, window, worst, SE.BARS[window], worst / SE.BARS[window]))
    for engine in (0, PLAIN):
        if engine:
            m = SD.make(pkg, N, S, M, engine=PLAIN, window=w)
        m.sessions_create(3, max(len(u) for u in utts))         # three ids for five streams
        for k, (cname, cut) in enumerate(cuts.items()):
            SD.compare(SD.drive(m, utts, 3, cut, N, S, seed=70 + k), want, "%s %s engine %d, %s" % (name, window, engine, cname))
        m.close()


def cut_singles_at_every_boundary(N, S):
    """Pushes that end one sample in front of, on and one sample behind every n = N / 2 + k S, the counts at which frame k
    becomes deliverable and the carry moves on by a hop."""
    def cut(n, rng):
        ends = sorted({e for k in range(max(n - N // 2, 0) // S + 2) for e in (N // 2 + k * S - 1, N // 2 + k * S, N // 2 + k * S + 1)
                       if 0 < e < n} | {n})
        out, pos = [], 0
        for e in ends:
            out.append((e - pos, False))
            pos = e
        out[-1] = (out[-1][0], True)
        return out
    return cut


@pytest.mark.parametrize("name", ["400_160_80", "34_5_6"])
def test_tap_probes_through_sessions(pkg, name):
    """One-hot windows on taps 0, 1, N / 2 and N - 1 over the probe signal: every row names the sample it was read from.  Tap 0
    of the first frame of a push is the oldest carried sample, c0 = max(0, E S - N / 2): under Hann it meets an exact zero."""
    N, S, M = EDGE_SHAPES[name]
    utts = [SE.probe_signal(n, start=31 * k) for k, n in enumerate(SE.probe_lengths(N, S, 16))]
    table = stft_ref.mel_table(M, N, 16000.0, 0.0, 8000.0)[0].astype(np.float64)
    worst = 0.0
    for j in (0, 1, N // 2, N - 1):
        w = SE.onehot(N, j)
        b = stft_ref.basis(w).astype(np.float64)[:, :, j]
        with np.errstate(divide="ignore"):
            rowsum = np.log10(table @ (b[0] ** 2 + b[1] ** 2))
        band = int(np.argmax(np.isfinite(rowsum)))
        m = SD.make(pkg, N, S, M, window=w)
        want = SD.twins(m, utts)
        m.sessions_create(3, max(len(u) for u in utts))         # three ids for six streams: every slot is reused
        for k, cut in enumerate((SD.cut_step(S), cut_singles_at_every_boundary(N, S))):
            got = SD.drive(m, utts, 3, cut, N, S, seed=80 + k)
            for s, (u, g, t) in enumerate(zip(utts, got, want)):
                ref = stft_ref.logmel(u, w, S, M, 16000.0, 0.0, 8000.0, stft_ref.LOG10)
                idx = stft_ref.frame_index(len(u), N, S)[:, j] if len(ref) else []
                assert g.shape == ref.shape
                floor = ref == SE.FLOOR_WANT
                d = np.where(floor, 0.0, np.abs(g.astype(np.float64) - ref))
                bad = np.nonzero((d.max(axis=1) > SE.ONEHOT_BAR) | ((g != SE.FLOOR_L10) & floor).any(axis=1))[0]
                assert bad.size == 0, ("%s tap %d cut %d stream %d: %d rows miss the one-hot bar; frame %d reads sample = %d (mod 193), "
                                       "the frame rule sample %d = %d (mod 193)") % (
                    name, j, k, s, bad.size, bad[0], SE.probe_decode(float(g[bad[0], band]), rowsum[band]), idx[bad[0]],
                    (idx[bad[0]] + 31 * s) % SE.PROBE_PERIOD)
                worst = max(worst, d.max(initial=0.0))
            SD.compare(got, want, "%s tap %d cut %d" % (name, j, k))
        m.close()
    print("\n%s one-hot probes through sessions: worst |d L| %.3g / bar %.3g = %.3f" % (name, worst, SE.ONEHOT_BAR, worst / SE.ONEHOT_BAR))
