"""Session pushes queued back to back: mfx_sessions_run_device is asynchronous on the handle's stream, and a caller plans and
queues push k + 1 while push k has not run.  Every other session test waits after every push; here each case runs twice.

The control pass is an existing synchronised drive on an existing configuration, attachment and push pattern, asserting what
it always asserts (its rows are the batch twin's bits), and recording every push.  The replay (tests/sess_inflight.py) runs
the record on a fresh handle on a torch side stream out of two resident arenas, a filler of torch matrix products in front of
every push, with no wait between the first push and the one synchronize behind the last.  It must deliver the control's rows
bit for bit, leave the NaN guard rows and the PCM arena alone, see mfx_sessions_plan and mfx_sessions_delivered answer as in
the control, and at least three quarters of its pushes must have been queued onto a stream that had not yet reached them (an
event behind the push's filler, queried right after the push is queued): fewer is a failure, never a skip.  A replay with
that share re-uses each pinned staging buffer while the other buffer's upload is still outstanding."""
import numpy as np
import pytest

import onorm_drive as OD
import sess_inflight as SI
import sess_resample_drive as RD
import sess_xform_drive as SD
import test_onorm_gpu as TO
import test_sess_resample_gpu as TR
import test_sess_xform_gpu as TX
import test_sessions_gpu as TS
from conftest import synth_utterance

pytestmark = pytest.mark.gpu

MIN_PUSHES = 12      # each of the two staging buffers is then re-used at least five times


@pytest.fixture(scope="module")
def rig(pkg):
    """(side stream, filler): the filler is sized once, in a synchronised warm-up on a throw-away C1 handle."""
    import torch
    stream = torch.cuda.Stream()
    utts, _ = TS._reference(pkg, "c1")
    record = []
    m = TS._make(pkg, TS.CONFIGS["c1"])
    try:
        m.sessions_create(10, TS.MAX_PUSH)
        TS._drive(m, utts, 10, TS.cut_random, seed=11, record=record)
    finally:
        m.close()
    with torch.cuda.stream(stream):
        filler = SI.Filler()
    m = TS._make(pkg, TS.CONFIGS["c1"])
    try:
        m.set_stream(stream.cuda_stream)
        m.sessions_create(10, TS.MAX_PUSH)
        SI.calibrate(m, record, stream, filler)
    finally:
        m.close()
    return stream, filler


def both(rig, handle, control, what, between=None, own_stream=False, control_handle=None):
    """handle() -> a fresh handle with its sessions; control(m, record) drives it synchronised, asserts the twin's bits and
    fills the record (on control_handle() where the replay's handle differs).  Then the replay on a second handle()."""
    stream, filler = rig
    record = []
    m = (control_handle or handle)()
    try:
        extra = control(m, record)
    finally:
        m.close()
    assert len(record) >= MIN_PUSHES, (what, len(record))
    m = handle()
    try:
        if own_stream:
            return record, SI.replay(m, record, None, None, what=what)
        m.set_stream(stream.cuda_stream)
        return record, SI.replay(m, record, stream, filler, between=between(m, extra) if between else None, what=what)
    finally:
        m.close()


# ---- 1. plain C1 -----------------------------------------------------------------------------------------------------------

def c1_pattern(pkg, rig, pattern, what, **kw):
    """The pattern of test_push_patterns_on_c1 (its own number of driven sessions) on a handle of 10 sessions; the ten
    utterances twice over, so that every id is reused and the pushes are enough."""
    utts, want = TS._reference(pkg, "c1")
    p = dict(TS.PATTERNS[pattern])
    n_sessions = p.pop("n_sessions")

    def handle():
        m = TS._make(pkg, TS.CONFIGS["c1"])
        m.sessions_create(10, TS.MAX_PUSH)
        return m

    def control(m, record):
        got = TS._drive(m, utts + utts, n_sessions, seed=11, record=record, **p)
        TS._compare("c1", got, want + want, what)

    return both(rig, handle, control, what, **kw)


@pytest.mark.parametrize("pattern", ["random_empty_and_flush", "random_odd_offsets", "ids_reused", "changing_subset", "descending_ids"])
def test_c1_push_patterns_in_flight(pkg, rig, pattern):
    c1_pattern(pkg, rig, pattern, "c1 " + pattern)


# ---- 2. the spectrum path (d_slab and the row runs re-used by every push), 1024 points, stereo --------------------------

@pytest.mark.parametrize("name", ["slab4096", "plp12", "fft1024", "stereo44k"])
def test_configurations_in_flight(pkg, rig, name):
    """test_configurations' drive: 7 sessions, random pieces with empty pushes and flushes, odd offsets."""
    kw = TS.CONFIGS[name]
    utts, want = TS._reference(pkg, name)

    def handle():
        m = TS._make(pkg, kw)
        m.sessions_create(7, TS.MAX_PUSH)
        return m

    def control(m, record):
        TS._compare(name, TS._drive(m, utts, 7, TS.cut_random_with_empty, seed=5, odd_offsets=True, record=record), want, "in flight")

    both(rig, handle, control, name)


# ---- 3. the online normaliser: d_state and d_ring carried between queued pushes -------------------------------------------

@pytest.mark.parametrize("setting", ["n32_cvn_before_prior", "n32_cmn_after", "n0_cmn_after", "n0_cvn_after_prior", "n96_cvn_before"])
def test_online_normaliser_in_flight(pkg, rig, setting):
    """test_session_rows_are_the_batch_rows' settings with random_empty_and_flush: CMN and CVN, before and after the deltas,
    windows of 32 and 96 frames and the whole past (window 0)."""
    N, kind, nad, prior = TO.SESS[setting]
    want = TO.base_rows(pkg, N, kind, nad, prior=prior)
    p = dict(OD.PATTERNS["random_empty_and_flush"])
    n_sessions = p.pop("n_sessions")

    def control(m, record):
        OD.compare("c1", OD.drive(m, TO.utts_of("c1"), n_sessions, seed=11, record=record, **p), want, setting + ", in flight")

    both(rig, lambda: TO.session_handle(pkg, "c1", N, kind, nad, prior, n_sessions, OD.MAX_PUSH), control, "onorm " + setting)


# ---- 4. the session transform: the y slots carried between queued pushes -------------------------------------------------

@pytest.mark.parametrize("engine", (0, TX.PLAIN), ids=("packed", "plain"))
def test_shuffled_pieces_three_transforms_behind_the_online_normaliser_in_flight(pkg, rig, engine):
    """test_shuffled_pieces_three_transforms_behind_the_online_normaliser as it stands (+2 / -3 -> 24, online CVN of 32 frames
    behind the deltas), k_sess_xform and MFX_ENGINE_SESS_XFORM_PLAIN."""
    kw, A, b = TX.shape(pkg, "c1", 2, 3, 24, n_xf=3)
    utts = TX.utts_of("c1")
    utt_xf = [u % 3 for u in range(len(utts))]
    want = TX.want_rows(pkg, "c1-2-3-24-x3-onorm-cvn", kw, utts, A, b, 2, 3, utt_xf=utt_xf, norm=2, nad=True, onorm=32)

    def control(m, record):
        got = SD.drive(m, utts, 5, OD.cut_random_with_empty, 23, 3, subset=True, shuffle=True, xf_of=utt_xf, record=record)
        SD.compare("c1", got, want, "xform, shuffled pieces, in flight")

    both(rig, lambda: TX.session_handle(pkg, kw, A, b, 2, 3, 5, norm=2, nad=True, onorm=32, engine=engine), control,
         "xform x3 + cvn, %s" % ("plain" if engine else "packed"))


def test_shuffled_pieces_three_transforms_two_frames_each_side_in_flight(pkg, rig):
    """The same drive with left = right = 2 and no normaliser (row width 39, +-2 -> 24: the transform shape of
    test_session_transform_behind_the_converter): Ex lags E by two rows and rows y are carried from push to push."""
    kw, A, b = TX.shape(pkg, "c1", 2, 2, 24, n_xf=3)
    utts = TX.utts_of("c1")
    utt_xf = [u % 3 for u in range(len(utts))]
    want = TX.want_rows(pkg, "c1-2-2-24-x3", kw, utts, A, b, 2, 2, utt_xf=utt_xf)

    def control(m, record):
        got = SD.drive(m, utts, 5, OD.cut_random_with_empty, 23, 2, subset=True, shuffle=True, xf_of=utt_xf, record=record)
        SD.compare("c1", got, want, "xform +-2, shuffled pieces, in flight")

    both(rig, lambda: TX.session_handle(pkg, kw, A, b, 2, 2, 5), control, "xform x3 +-2")


# ---- 5. session rates: the carry ping-pong and the one scratch of converted pieces ---------------------------------------

def rates_record_is_the_twins(fleet, keys, wants):
    for key in keys:
        TR.check_stream(fleet, key, wants[key], key)


@pytest.mark.parametrize("channels", [1, 2])
@pytest.mark.parametrize("rate", [48000, 8000])
def test_a_converted_stream_in_flight(pkg, rig, rate, channels):
    """test_a_stream_equals_its_batch_twin_however_it_is_cut: one stream cut four ways through four sessions, one after the
    other."""
    L, M, Wh = RD.shape(pkg, rate)
    n = int(0.3 * rate) + 1
    x = RD.stream(RD.RATES.index(rate) % 3, n, rate, rate % 97, channels)
    want = RD.twin(pkg, x, rate)
    cuts = {"one": RD.cut_one(n), "100ms": RD.cut_even(n, rate // 10), "random": RD.cut_random(n, Wh, rate // 10, rate),
            "odd": RD.cut_even(n, rate // 10 + 1)}

    def handle():
        m = RD.make(pkg, channels=channels)
        m.sessions_set_rates([rate])
        m.sessions_create(4, n)
        return m

    def control(m, record):
        fleet = RD.Fleet(pkg, m, seed=rate + channels, record=record)
        for sid, (name, cut) in enumerate(cuts.items()):
            RD.feed(fleet, sid, name, rate, x, cut, odd=name == "odd")
            TR.check_stream(fleet, name, want, (rate, channels, name))

    both(rig, handle, control, "rates %d Hz, %d ch" % (rate, channels))


def test_mixed_fleet_in_flight(pkg, rig):
    """The fleet of test_mixed_fleet_with_reuse_reset_and_absent_sessions: five rates (the pass-through among them) over 12
    sessions, ids reused at another rate, sessions absent from pushes, one session reset in mid-stream; the sessions_select_rate and sessions_reset calls are replayed between the queued pushes."""
    rates_hz = TR.FLEET_RATES
    rng = np.random.default_rng(77)
    n_sess = 12
    queue = {}
    for sid in range(n_sess):
        q = [(("a", sid), sid % 5)]
        if sid < 6:
            q.append((("b", sid), (sid + 2) % 5))
        queue[sid] = q
    xs, rates, keys, streams = [], [], [], {}
    for sid, q in queue.items():
        for key, ri in q:
            rate = rates_hz[ri]
            n = int(rate * (0.25 + 0.25 * rng.random()))
            streams[key] = RD.stream(len(keys) % 3, n, rate, 100 + len(keys))
            xs.append(streams[key]), rates.append(rate), keys.append(key)
    wants = dict(zip(keys, RD.twins(pkg, xs, rates)))

    def handle():
        m = RD.make(pkg)
        m.sessions_set_rates(rates_hz)
        m.sessions_create(n_sess, max(rates_hz) // 10)
        return m

    def control(m, record):
        fleet = RD.Fleet(pkg, m, seed=5, record=record)
        fed, tick, did_reset = {}, 0, False
        while any(queue.values()):
            pieces = []
            for sid in rng.permutation(n_sess):
                sid = int(sid)
                if not queue[sid]:
                    continue
                key, ri = queue[sid][0]
                rate = rates_hz[ri]
                if sid not in fleet.state:
                    fleet.call("sessions_select_rate", sid, ri)
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
                sid = next(s for s in fleet.state if fleet.state[s][2] > 0 and fleet.state[s][1] != RD.SR)
                key, rate = fleet.state[sid][0], fleet.state[sid][1]
                fleet.call("sessions_reset", sid)
                fleet.drop(sid)
                fleet.open(sid, key, rate)
                fed[sid] = 0
                did_reset = True
        assert did_reset and any(fleet.launches)
        rates_record_is_the_twins(fleet, keys, wants)

    both(rig, handle, control, "rates, mixed fleet")


# ---- 6. everything at once: rates + online CVN + a transform ---------------------------------------------------------------

@pytest.mark.parametrize("rate", [48000, 8000])
def test_converter_online_cvn_and_transform_in_flight(pkg, rig, rate):
    """test_online_cvn_behind_the_converter and test_session_transform_behind_the_converter on one handle: the converter, the
    online CVN of 64 frames behind the deltas and the +-2 -> 24 transform behind that."""
    L, M, Wh = RD.shape(pkg, rate)
    n = int(0.4 * rate) + 3
    x = RD.stream(1, n, rate, 12)
    r = np.random.default_rng(rate)
    A = r.standard_normal((24, 5 * 39)).astype(np.float32)
    b = r.standard_normal(24).astype(np.float32)

    def setup(h):
        h.batch_set_online_norm(64)
        h.batch_set_transform(A, b, 2, 2)

    want = RD.twin(pkg, x, rate, setup=setup, norm=pkg.NORM_CVN)

    def handle():
        m = RD.make(pkg, norm=pkg.NORM_CVN)
        m.sessions_set_online_norm(64)
        m.sessions_set_transform(A, b, 2, 2)
        m.sessions_set_rates([rate])
        m.sessions_create(2, rate // 10)
        assert m.sessions_output_width() == 24
        return m

    def control(m, record):
        fleet = RD.Fleet(pkg, m, seed=rate, record=record)
        for sid, seed in enumerate((6, 5)):                      # the stream twice, cut two ways, one session after the other
            RD.feed(fleet, sid, seed, rate, x, RD.cut_random(n, Wh, rate // 10, seed), right=2)
            TR.check_stream(fleet, seed, want, (rate, "cvn + xform", seed))

    both(rig, handle, control, "rates %d Hz + cvn + xform" % rate)


# ---- 7 - 10. host calls between queued pushes, on the plain C1 handle -----------------------------------------------------

def twin_rows(pkg, kw, utts):
    t = TS._make(pkg, kw)
    try:
        rows = OD.batch_rows(t, utts)
    finally:
        t.close()
    return rows


def test_warp_factor_between_utterances_in_flight(pkg, rig):
    """Every session finishes, mfx_set_alpha(0.9) arrives with the pipeline full, the same utterances follow: the earlier rows
    are the alpha = 1.0 twin's, the later ones the alpha = 0.9 twin's (CONFIGS["alpha09"]).  The next push's refresh_mel must
    wait for the queued readers of the old tables before it replaces them."""
    utts, want10 = TS._reference(pkg, "c1")
    want09 = twin_rows(pkg, TS.CONFIGS["alpha09"], utts)
    assert any(len(a) and not np.array_equal(a, b) for a, b in zip(want10, want09))

    def handle():
        m = TS._make(pkg, TS.CONFIGS["c1"])
        m.sessions_create(10, TS.MAX_PUSH)
        return m

    def control(m, record):
        TS._compare("c1", TS._drive(m, utts, 10, TS.cut_random, seed=11, record=record), want10, "alpha 1.0, in flight")
        first = len(record)
        m.set_alpha(0.9)
        TS._compare("c1", TS._drive(m, utts, 10, TS.cut_random, seed=12, record=record), want09, "alpha 0.9, in flight")
        record[first]["calls"].append(("set_alpha", (0.9,)))

    both(rig, handle, control, "c1, set_alpha between utterances")


def c1_fleet(pkg, m, record, utts, want, reset_at=None, host_at=None, on_tick=None):
    """Four sessions of a plain C1 handle in 1000-sample pieces through sess_resample_drive's Fleet (every piece at the
    handle's own rate): the 100-, 65-, 64- and 63-frame utterances first, the short ones on the ids that finish -- an id is
    reused on the push directly behind its final push.  reset_at: session 2 is reset in front of that push and its stream
    starts again from its first sample.  host_at: that push goes through sessions_run_host.  Checks every stream against
    the twin's rows; returns the fleet."""
    fleet = RD.Fleet(pkg, m, seed=8, record=record)
    todo = [9, 8, 7, 6, 5, 4, 3, 2, 1, 0]
    cur, tick = {}, 0
    while todo or cur:
        for sid in range(4):
            if sid not in cur and todo:
                cur[sid] = [todo.pop(0), 0]
                fleet.open(sid, (cur[sid][0], "whole"), RD.SR)
        if tick == reset_at:
            u = cur[2][0]
            assert 0 < cur[2][1] < len(utts[u])
            fleet.call("sessions_reset", 2)
            fleet.drop(2)
            fleet.rows[(u, "dropped")] = fleet.rows[(u, "whole")]
            fleet.open(2, (u, "whole"), RD.SR)
            cur[2][1] = 0
        pieces = []
        for sid in sorted(cur):
            u, fed = cur[sid]
            n = min(1000, len(utts[u]) - fed)
            fin = fed + n == len(utts[u])
            pieces.append((sid, utts[u][fed:fed + n], fin))
            cur[sid][1] += n
            if fin:
                del cur[sid]
        fleet.push(pieces, host=tick == host_at)
        if on_tick:
            on_tick(tick)
        tick += 1
    for u in range(10):
        assert RD.same_bits(fleet.delivered((u, "whole")), want[u]), u
    if reset_at is not None:
        part = fleet.delivered((7, "dropped"))                     # what session 2 had delivered before the reset
        assert 0 < len(part) < len(want[7]) and RD.same_bits(part, want[7][:len(part)])
    return fleet


def c1_handle(pkg):
    m = TS._make(pkg, TS.CONFIGS["c1"])
    m.sessions_create(4, TS.MAX_PUSH)
    return m


def test_reset_in_flight(pkg, rig):
    """sessions_reset(2) between two queued pushes (it keeps the slot parity and does not wait): the reset stream starts again
    from its first sample and delivers the twin's rows from row 0, the other sessions deliver theirs."""
    utts, want = TS._reference(pkg, "c1")
    record, _ = both(rig, lambda: c1_handle(pkg), lambda m, rec: c1_fleet(pkg, m, rec, utts, want, reset_at=4), "c1, reset in flight")
    assert sum(name == "sessions_reset" for e in record for name, _ in e["calls"]) == 1


def test_a_host_entry_push_between_device_pushes(pkg, rig):
    """One sessions_run_host push in the middle (it waits, by contract): its rows and those of the queued pushes before and
    after it are the control's."""
    utts, want = TS._reference(pkg, "c1")
    record, _ = both(rig, lambda: c1_handle(pkg), lambda m, rec: c1_fleet(pkg, m, rec, utts, want, host_at=6), "c1, host push at 6")
    assert [e["host"] for e in record].count(True) == 1 and record[6]["host"] and record[6]["total"] > 0


def test_batch_and_streaming_entries_between_queued_pushes(pkg, rig):
    """test_batch_and_streaming_state_survive_session_pushes without its waits: between queued pushes the handle runs its
    planned batch (its own alpha list and transform; mfx_batch_run_device on resident arrays, three times, never waited for)
    and a streaming block.  mfx_set_input synchronises the handle's stream by its own contract, as the host-entry push does;
    the pushes in front of it and behind it are queued all the same.  All three deliver what they deliver alone."""
    import torch
    stream, _ = rig
    utts, want = TS._reference(pkg, "c1")
    rng = np.random.default_rng(3)
    block = synth_utterance(8000, 900)
    b_pcm = np.concatenate([synth_utterance(9000, 77), synth_utterance(7001, 78), np.zeros(3, np.int16)])
    A = rng.standard_normal((8, 3 * 39)).astype(np.float32)

    def handle():
        m = TS._make(pkg, TS.CONFIGS["c1"])
        m.batch_plan([0, 9000], [9000, 7001])
        m.batch_set_alphas([1.0, 0.9])
        m.batch_set_transform(A, None, left=1, right=1)
        m.sessions_create(4, TS.MAX_PUSH)
        return m

    def stream_block(h):
        n = h.set_input(block)
        h.apply()
        return h.get_output_data(n)

    alone = handle()
    try:
        want_batch, want_stream = alone.batch_run_host(b_pcm), stream_block(alone)
        assert want_batch.shape == (alone.batch_frames(9000) + alone.batch_frames(7001), 8) and len(want_stream) > 0
    finally:
        alone.close()

    def control(m, record):
        batches, blocks = [], []

        def on_tick(tick):                                       # (behind push `tick`: in front of push tick + 1, as in the replay)
            if tick in (1, 4, 7):
                batches.append(m.batch_run_host(b_pcm))
            if tick == 3:
                blocks.append(stream_block(m))
        c1_fleet(pkg, m, record, utts, want, on_tick=on_tick)
        assert len(batches) == 3 and all(RD.same_bits(r, want_batch) for r in batches)
        assert len(blocks) == 1 and RD.same_bits(blocks[0], want_stream)

    got = {}

    def between(m, _):
        with torch.cuda.stream(stream):
            d_b = torch.from_numpy(b_pcm).to("cuda:0")
            d_o = [torch.full(want_batch.shape, float("nan"), dtype=torch.float32, device="cuda:0") for _ in range(3)]
        got["batch"] = d_o

        def batch(k):
            return lambda: m.batch_run_device(d_b.data_ptr(), len(b_pcm), d_o[k].data_ptr())
        return {2: batch(0), 5: batch(1), 8: batch(2), 4: lambda: got.__setitem__("stream", stream_block(m))}

    both(rig, handle, control, "c1 + batch + streaming", between=between)
    for d in got["batch"]:
        assert RD.same_bits(d.cpu().numpy(), want_batch)
    assert RD.same_bits(got["stream"], want_stream)


# ---- 11. the handle's own stream ----------------------------------------------------------------------------------------------

def test_back_to_back_on_the_handles_own_stream(pkg, rig):
    """No mfx_set_stream: the handle runs on the stream it created.  The inputs are made resident, torch.cuda.synchronize(),
    then the pushes go back to back and one mfx_synchronize follows.  No filler can be put on that stream from Python, so
    the in-flight proof does NOT apply to this case: it asserts the bits, the guards, the plan and the delivered counts only."""
    kw = TS.CONFIGS["c1"]
    utts, want = TS._reference(pkg, "c1")

    def handle():
        m = pkg.MfccHip(100 * kw["shift"] + kw["window_size"], kw["window_size"], kw["shift"], kw["num_banks"], kw["sample_rate"],
                        64.0, kw["sample_rate"] / 2, kw["ceps_len"], False, 22.0, pkg.NORM_NONE, kw["dyn"], kw["delta_l1"],
                        kw["delta_l2"], True, device=0, fft_size=kw["fft_size"], channels=kw["channels"], method=kw["method"],
                        lpc_order=kw["lpc_order"], engine=kw["engine"])
        m.set_window(pkg.reference_window(kw["window_size"]))
        m.set_alpha(kw["alpha"])
        m.sessions_create(10, TS.MAX_PUSH)
        return m

    def control(m, record):
        got = TS._drive(m, utts + utts, 10, TS.cut_random, seed=11, odd_offsets=True, record=record)
        TS._compare("c1", got, want + want, "own stream")

    def control_handle():                                        # (on torch's stream: the drive's NaN fills are ordered with the pushes)
        m = TS._make(pkg, kw)
        m.sessions_create(10, TS.MAX_PUSH)
        return m

    both(rig, handle, control, "c1, own stream", own_stream=True, control_handle=control_handle)
