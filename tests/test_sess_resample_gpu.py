"""Per-session sample-rate conversion in front of a push (mfx_sessions_set_rates; k_sess_resample) on the MI355X.

The contract: a stream fed piece by piece at its own rate delivers the converted samples (mfx_sessions_converted_read) and the
rows that the batch entry delivers for the whole utterance under mfx_batch_plan_rates (mfx_debug_read kind 8, the batch rows),
bit for bit, however the stream is cut.  Feature configuration and signals of tests/test_resample_gpu.py (16 kHz, W = 400, S =
160, 40 mel, 13 cepstra + d + dd; full-scale noise, a 997 Hz sine, a full-scale square wave).  Every comparison is same_bits."""
import numpy as np
import pytest

import sess_resample_drive as RD

pytestmark = pytest.mark.gpu

SR, RATES = RD.SR, RD.RATES
ERR_SMALL, ERR_ARG, ERR_STATE = -1, -7, -8


def check_stream(fleet, key, want, what):
    y, rows = want
    got_y, got_rows = fleet.converted(key), fleet.delivered(key)
    assert got_y.shape == y.shape and np.array_equal(got_y, y), "%s: converted samples differ" % (what,)
    assert RD.same_bits(got_rows, rows), "%s: rows differ" % (what,)


# ---- 1. per rate and channel count, one stream cut four ways -------------------------------------------------------------

@pytest.mark.parametrize("channels", [1, 2])
@pytest.mark.parametrize("rate", RATES)
def test_a_stream_equals_its_batch_twin_however_it_is_cut(pkg, rate, channels):
    L, M, Wh = RD.shape(pkg, rate)
    n = int(0.3 * rate) + 1                                  # 0.3 s after conversion, an odd input length
    x = RD.stream(RATES.index(rate) % 3, n, rate, rate % 97, channels)
    want = RD.twin(pkg, x, rate)
    assert want[1].shape[0] > 20
    m = RD.make(pkg, channels=channels)
    m.sessions_set_rates([rate])
    m.sessions_create(4, n)
    fleet = RD.Fleet(pkg, m, seed=rate + channels)
    cuts = {"one": RD.cut_one(n), "100ms": RD.cut_even(n, rate // 10), "random": RD.cut_random(n, Wh, rate // 10, rate),
            "odd": RD.cut_even(n, rate // 10 + 1)}
    assert {0, 1} <= {c for c, _ in cuts["random"]} and any(1 < c < Wh for c, _ in cuts["random"])
    for sid, (name, cut) in enumerate(cuts.items()):
        RD.feed(fleet, sid, name, rate, x, cut, odd=name == "odd")
        check_stream(fleet, name, want, (rate, channels, name))
    m.close()


def test_12345_hz_is_the_shape_without_a_staged_table(pkg):
    """L = 3200, P = 14: one output per work item and the table read through the caches (what resample_geometry says of it)."""
    h, L, M, P = pkg.mfcc.host_resample_taps(12345, SR)
    assert (L, P) == (3200, 14) and L * (P + 1) > 16384 and 2 * L > pkg.mfcc.host_resample_tile(12345, SR)


# ---- 2. tile edges -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("rate", [48000, 44100])
def test_pieces_around_a_tile_of_the_kernel(pkg, rate):
    L, M, Wh = RD.shape(pkg, rate)
    tile = pkg.mfcc.host_resample_tile(rate, SR)
    edge = -(-tile * M // L)
    lens = [edge - 1, edge, edge + 1, 2 * edge + 3]
    N = sum(lens)
    j = RD.converted_count(pkg, rate, N, False) + 37         # a piece that ends exactly where output j becomes computable
    lens.append((j * M) // L + Wh + 1 - N)
    N += lens[-1]
    assert RD.converted_count(pkg, rate, N, False) == j + 1 and RD.converted_count(pkg, rate, N - 1, False) == j
    j = RD.converted_count(pkg, rate, N, False) + 11         # and one that ends one sample short of it
    lens.append((j * M) // L + Wh - N)
    N += lens[-1]
    assert RD.converted_count(pkg, rate, N, False) == j and RD.converted_count(pkg, rate, N + 1, False) == j + 1
    lens.append(5)
    N += 5
    x = RD.stream(0, N, rate, 7)
    want = RD.twin(pkg, x, rate)
    m = RD.make(pkg)
    m.sessions_set_rates([rate])
    m.sessions_create(1, max(lens))
    fleet = RD.Fleet(pkg, m, seed=rate)
    RD.feed(fleet, 0, "edges", rate, x, RD.cut_lengths(lens))
    check_stream(fleet, "edges", want, (rate, "edges"))
    m.close()


# ---- 3. degenerate streams -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("rate", RATES)
def test_streams_too_short_to_convert_deliver_at_the_final_push(pkg, rate):
    L, M, Wh = RD.shape(pkg, rate)
    m = RD.make(pkg)
    m.sessions_set_rates([rate])
    m.sessions_create(4, 2 * Wh + 1)
    fleet = RD.Fleet(pkg, m, seed=rate)
    totals = (0, 1, Wh, 2 * Wh + 1)
    xs = [RD.stream(k % 3, n, rate, 30 + k) for k, n in enumerate(totals)]
    wants = RD.twins(pkg, xs, [rate] * len(xs))
    for sid, (n, x, want) in enumerate(zip(totals, xs, wants)):
        cut = [(1, False)] * n + [(0, True)]                 # sample by sample, then the flush
        RD.feed(fleet, sid, n, rate, x, cut)
        assert all(len(r) == 0 for r in fleet.rows[n][:-1])  # nothing before the final push: too short for a frame
        check_stream(fleet, n, want, (rate, n))
        assert len(want[0]) == -(-n * L // M)
    m.close()


# ---- 4. a mixed fleet ----------------------------------------------------------------------------------------------------

FLEET_RATES = (48000, 8000, 44100, 12345, SR)


def test_mixed_fleet_with_reuse_reset_and_absent_sessions(pkg):
    rng = np.random.default_rng(77)
    n_sess = 12
    # every session's queue of streams: (key, rate index, samples); the first six ids carry a second stream at another rate
    queue = {}
    for sid in range(n_sess):
        q = [(("a", sid), sid % 5)]
        if sid < 6:
            q.append((("b", sid), (sid + 2) % 5))
        queue[sid] = q
    xs, rates, keys = [], [], []
    streams = {}
    for sid, q in queue.items():
        for key, ri in q:
            rate = FLEET_RATES[ri]
            n = int(rate * (0.25 + 0.25 * rng.random()))
            streams[key] = RD.stream(len(keys) % 3, n, rate, 100 + len(keys))
            xs.append(streams[key]), rates.append(rate), keys.append(key)
    wants = dict(zip(keys, RD.twins(pkg, xs, rates)))
    m = RD.make(pkg)
    m.sessions_set_rates(FLEET_RATES)
    m.sessions_create(n_sess, max(FLEET_RATES) // 10)
    fleet = RD.Fleet(pkg, m, seed=5)
    fed, tick, did_reset = {}, 0, False
    while any(queue.values()):
        pieces = []
        for sid in rng.permutation(n_sess):
            sid = int(sid)
            if not queue[sid]:
                continue
            key, ri = queue[sid][0]
            rate = FLEET_RATES[ri]
            if sid not in fleet.state:
                m.sessions_select_rate(sid, ri)
                fleet.open(sid, key, rate)
                fed[sid] = 0
            if rng.random() < 0.25:
                continue                                     # absent from this push
            x = streams[key]
            n = min(int(rng.integers(0, rate // 10 + 1)), len(x) - fed[sid])
            fin = fed[sid] + n == len(x) and rng.random() < 0.7
            pieces.append((sid, x[fed[sid]:fed[sid] + n], fin))
            fed[sid] += n
            if fin:
                queue[sid].pop(0)
        fleet.push(pieces)
        tick += 1
        if tick == 3 and not did_reset:                      # one session is reset mid-stream and starts its stream again
            sid = next(s for s in fleet.state if fleet.state[s][2] > 0 and fleet.state[s][1] != SR)
            key, rate = fleet.state[sid][0], fleet.state[sid][1]
            with pytest.raises(pkg.MfxError) as e:
                m.sessions_select_rate(sid, 0)               # not fresh
            assert e.value.status == ERR_STATE
            m.sessions_reset(sid)
            fleet.drop(sid)
            fleet.open(sid, key, rate)
            fed[sid] = 0
            did_reset = True
    assert did_reset and any(fleet.launches)
    for key in keys:
        check_stream(fleet, key, wants[key], key)
    m.close()


def test_a_push_of_pass_through_pieces_matches_a_handle_without_rates(pkg):
    rng = np.random.default_rng(3)
    xs = [RD.stream(k % 3, 5000 + 37 * k, SR, 60 + k) for k in range(3)]
    plain = RD.make(pkg)
    plain.sessions_create(4, 1600)
    m = RD.make(pkg)
    m.sessions_set_rates(FLEET_RATES)
    m.sessions_create(4, 1600)
    fa, fb = RD.Fleet(pkg, m, seed=9), RD.Fleet(pkg, plain, seed=9)
    for sid in range(3):
        m.sessions_select_rate(sid, FLEET_RATES.index(SR))
        fa.open(sid, sid, SR), fb.open(sid, sid, SR)
    fed = [0, 0, 0]
    while fa.state:
        pieces = []
        for sid in list(fa.state):
            n = min(int(rng.integers(0, 1601)), len(xs[sid]) - fed[sid])
            pieces.append((sid, xs[sid][fed[sid]:fed[sid] + n], fed[sid] + n == len(xs[sid])))
            fed[sid] += n
        a, b = fa.push(pieces), fb.push(pieces)
        assert RD.same_bits(a, b)
    for sid in range(3):
        assert RD.same_bits(fa.delivered(sid), fb.delivered(sid)) and len(fa.delivered(sid)) > 20
        assert np.array_equal(fa.converted(sid), xs[sid])
    m.close(), plain.close()


# ---- 5. composition ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("rate", [48000, 8000])
def test_online_cvn_behind_the_converter(pkg, rate):
    L, M, Wh = RD.shape(pkg, rate)
    n = int(0.4 * rate) + 3
    x = RD.stream(0, n, rate, 11)
    want = RD.twin(pkg, x, rate, setup=lambda b: b.batch_set_online_norm(64), norm=pkg.NORM_CVN)
    m = RD.make(pkg, norm=pkg.NORM_CVN)
    m.sessions_set_online_norm(64)
    m.sessions_set_rates([rate])
    m.sessions_create(1, rate // 10)
    fleet = RD.Fleet(pkg, m, seed=rate)
    RD.feed(fleet, 0, "cvn", rate, x, RD.cut_random(n, Wh, rate // 10, 5))
    check_stream(fleet, "cvn", want, (rate, "cvn"))
    m.close()


@pytest.mark.parametrize("rate", [48000, 8000])
def test_session_transform_behind_the_converter(pkg, rate):
    L, M, Wh = RD.shape(pkg, rate)
    n = int(0.4 * rate) + 3
    x = RD.stream(1, n, rate, 12)
    rng = np.random.default_rng(rate)
    A = rng.standard_normal((24, 5 * 39)).astype(np.float32)
    b = rng.standard_normal(24).astype(np.float32)
    want = RD.twin(pkg, x, rate, setup=lambda h: h.batch_set_transform(A, b, 2, 2))
    m = RD.make(pkg)
    m.sessions_set_transform(A, b, 2, 2)
    m.sessions_set_rates([rate])
    m.sessions_create(1, rate // 10)
    assert m.sessions_output_width() == 24
    fleet = RD.Fleet(pkg, m, seed=rate)
    RD.feed(fleet, 0, "xf", rate, x, RD.cut_random(n, Wh, rate // 10, 6), right=2)
    check_stream(fleet, "xf", want, (rate, "xf"))
    m.close()


def test_run_host_and_an_odd_placement_of_d_out(pkg):
    from placement import OutPlacement
    rate = 44100
    L, M, Wh = RD.shape(pkg, rate)
    n = int(0.3 * rate)
    x = RD.stream(2, n, rate, 13, 2)
    want = RD.twin(pkg, x, rate)
    m = RD.make(pkg, channels=2)
    m.sessions_set_rates([8000, rate])
    m.sessions_create(2, rate // 10)
    m.sessions_select_rate(0, 1), m.sessions_select_rate(1, 1)
    fleet = RD.Fleet(pkg, m, seed=1)
    RD.feed(fleet, 0, "host", rate, x, RD.cut_even(n, rate // 10), host=True)
    check_stream(fleet, "host", want, "run_host")
    for k in (1, 3):                                         # d_out k floats past a 16-byte boundary, guard words around it
        RD.feed(fleet, 1, ("place", k), rate, x, RD.cut_even(n, rate // 10), place=lambda rows, width: OutPlacement(rows, width, k))
        check_stream(fleet, ("place", k), want, ("placement", k))
    m.close()


# ---- 6. state and errors -------------------------------------------------------------------------------------------------

def status_of(pkg, f, *a):
    with pytest.raises(pkg.MfxError) as e:
        f(*a)
    return e.value.status


def test_state_rules_and_errors(pkg):
    import torch
    m = RD.make(pkg)
    assert status_of(pkg, m.sessions_select_rate, 0, 0) == ERR_STATE            # no rates
    assert status_of(pkg, m.sessions_set_rates, []) == ERR_ARG
    assert status_of(pkg, m.sessions_set_rates, [48000] * 17) == ERR_ARG
    assert status_of(pkg, m.sessions_set_rates, [999]) == ERR_ARG
    assert status_of(pkg, m.sessions_set_rates, [48000], 65) == ERR_ARG
    assert status_of(pkg, m.sessions_set_rates, [SR], 65) == ERR_ARG            # judged for a pass-through rate too
    assert status_of(pkg, m.sessions_set_rates, [SR, 48000], 0, 1.5) == ERR_ARG
    assert status_of(pkg, m.sessions_set_rates, [48000], 0, 1.5) == ERR_ARG
    assert status_of(pkg, m.sessions_set_rates, [16001]) == ERR_ARG             # L = 16000 > 4096
    m.sessions_set_rates([48000, SR])
    assert status_of(pkg, m.sessions_select_rate, 0, 0) == ERR_STATE            # no sessions
    m.sessions_create(2, 4800)
    assert status_of(pkg, m.sessions_set_rates, [8000]) == ERR_STATE
    assert status_of(pkg, m.sessions_clear_rates) == ERR_STATE
    assert status_of(pkg, m.sessions_select_rate, 2, 0) == ERR_ARG
    assert status_of(pkg, m.sessions_select_rate, 0, 2) == ERR_ARG
    assert status_of(pkg, m.sessions_plan, [0], [0], [4801]) == ERR_SMALL       # longer than max_push_samples (input rate)
    x = RD.stream(0, 4800, 48000, 3)
    d_pcm = torch.from_numpy(x.reshape(-1).copy()).to("cuda:0")
    d_out = torch.zeros((64, 39), dtype=torch.float32, device="cuda:0")
    m.sessions_plan([0], [1], [4800])
    assert status_of(pkg, m.sessions_run_device, d_pcm.data_ptr(), 4800, d_out.data_ptr()) == ERR_ARG   # past the input array
    m.sessions_plan([0], [0], [10])                          # fewer than Wh samples: nothing converted, but received
    m.sessions_run_device(d_pcm.data_ptr(), 4800, d_out.data_ptr())
    m.synchronize()
    assert status_of(pkg, m.sessions_select_rate, 0, 1) == ERR_STATE            # the session has samples
    m.sessions_select_rate(1, 1)                             # a fresh one may choose
    m.sessions_reset(0)
    m.sessions_select_rate(0, 1)
    m.close()


def test_clearing_the_rates_gives_back_the_plain_handle_and_neighbours_are_undisturbed(pkg):
    from conftest import synth_utterance
    x = synth_utterance(6000, 41)
    plain = RD.make(pkg)
    plain.sessions_create(2, 4000)

    def push(h):
        out = []
        for a, fin in ((0, 0), (3000, 1)):
            h.sessions_plan([1], [a], [3000], [fin])
            out.append(h.sessions_run_host(x))
        return np.concatenate(out, 0)
    want = push(plain)
    stream_rows = plain.process_stream(x)
    plain.close()
    y8 = RD.stream(0, 3000, 8000, 5)
    tw = RD.twin(pkg, y8, 8000)

    m = RD.make(pkg)
    m.batch_plan([0], [len(x)])
    batch_plain = m.batch_run_host(x)
    m.sessions_set_rates([8000])
    m.sessions_create(2, 3000)
    fleet = RD.Fleet(pkg, m, seed=2)
    fleet.open(0, "s", 8000)
    fleet.push([(0, y8[:1500], False)])
    assert RD.same_bits(m.batch_run_host(x), batch_plain)    # the planned batch, between two pushes
    assert RD.same_bits(m.process_stream(x), stream_rows)    # and a streaming sequence
    m.batch_plan_rates([0], [len(y8)], [8000])
    under_rates = m.batch_run_host(np.concatenate([y8.reshape(-1), np.zeros(2, np.int16)]))
    assert RD.same_bits(under_rates, tw[1])
    fleet.push([(0, y8[1500:], True)])
    check_stream(fleet, "s", tw, "between batch runs")
    assert RD.same_bits(m.batch_run_host(np.concatenate([y8.reshape(-1), np.zeros(2, np.int16)])), tw[1])
    m.sessions_create(0, 0)
    m.sessions_clear_rates()
    m.sessions_create(2, 4000)
    assert RD.same_bits(push(m), want) and want.shape[0] > 0
    m.close()
