"""Session entries on the GPU: rows delivered push by push are the SAME BITS the batch entries write for the whole
utterance on a twin handle (same configuration, window and warp factor; utterances planned at even offsets), however
the streams are cut into pushes.  The twin is parity-checked against the reference by the other suites; the comparison
here is np.array_equal on the float32 bit patterns, so there is no tolerance to choose."""
import ctypes as C

import numpy as np
import pytest

from conftest import synth_utterance

pytestmark = pytest.mark.gpu

MAX_PUSH = 3000


def _c1(**over):
    kw = dict(window_size=400, shift=160, num_banks=26, sample_rate=16000.0, ceps_len=13, dyn=2, delta_l1=3, delta_l2=3,
              fft_size=0, channels=1, method=0, lpc_order=0, alpha=1.0, engine=0)
    kw.update(over)
    return kw


CONFIGS = {
    "c1": _c1(),
    "dyn_none": _c1(dyn=0),
    "dyn_delta": _c1(dyn=1),
    "fbank40": _c1(num_banks=40, ceps_len=0),
    "plp12": _c1(method=1, lpc_order=12),
    "alpha09": _c1(alpha=0.9),
    "tel8k": _c1(window_size=200, shift=80, num_banks=23, sample_rate=8000.0),
    "fft1024": _c1(num_banks=80, fft_size=1024),
    "stereo44k": _c1(window_size=1102, shift=441, num_banks=128, sample_rate=44100.0, ceps_len=40, channels=2),
    "mono44k": _c1(window_size=1102, shift=441, num_banks=128, sample_rate=44100.0, ceps_len=40),
    "slab4096": _c1(window_size=2400, shift=480, num_banks=64, sample_rate=48000.0),
}


def _make(pkg, kw):
    import torch
    m = pkg.MfccHip(100 * kw["shift"] + kw["window_size"], kw["window_size"], kw["shift"], kw["num_banks"], kw["sample_rate"],
                    64.0, kw["sample_rate"] / 2, kw["ceps_len"], False, 22.0, pkg.NORM_NONE, kw["dyn"], kw["delta_l1"],
                    kw["delta_l2"], True, device=0, fft_size=kw["fft_size"], channels=kw["channels"], method=kw["method"],
                    lpc_order=kw["lpc_order"], engine=kw["engine"])
    # torch's stream: the NaN fills and copies of the tests and the handle's launches are then ordered with each other
    m.set_stream(torch.cuda.current_stream().cuda_stream)
    m.set_window(pkg.reference_window(kw["window_size"]))
    m.set_alpha(kw["alpha"])
    return m


def _D(kw):
    return 0 if kw["dyn"] == 0 else kw["delta_l1"] if kw["dyn"] == 1 else kw["delta_l1"] + kw["delta_l2"]


_REF = {}


def _reference(pkg, name):
    """The utterances of a configuration and the twin handle's batch rows for them: computed once, shared, never changed."""
    if name in _REF:
        return _REF[name]
    kw = CONFIGS[name]
    W, S, D, ch = kw["window_size"], kw["shift"], _D(kw), kw["channels"]
    rng = np.random.default_rng(sum(map(ord, name)))
    utts = []
    for k, T in enumerate([0, 1, D, D + 1, 2 * D, 2 * D + 1, 63, 64, 65, 100]):
        n = int(rng.integers(0, W)) if T == 0 else W + (T - 1) * S + int(rng.integers(0, S))
        x = synth_utterance(n * ch, 7 * len(name) + k, sr=kw["sample_rate"]).reshape(n, ch)
        utts.append(x)
    twin = _make(pkg, kw)
    offs, pos = [], 0
    for x in utts:
        offs.append(pos)
        pos += (len(x) + 1) & ~1
    pcm = np.zeros((pos + 2, ch), np.int16)
    for o, x in zip(offs, utts):
        pcm[o:o + len(x)] = x
    rows, total = twin.batch_plan(offs, [len(x) for x in utts])
    out = twin.batch_run_host(pcm.reshape(-1))
    Ts = [twin.batch_frames(len(x)) for x in utts]
    twin.close()
    assert total == sum(Ts) and sorted(set(Ts)) == sorted({0, 1, D, D + 1, 2 * D, 2 * D + 1, 63, 64, 65, 100})
    want = [out[r:r + T].copy() for r, T in zip(rows, Ts)]
    for w in want:
        w.setflags(write=False)
    _REF[name] = (utts, want)
    return _REF[name]


# ---- how a stream is cut: (utterance samples left) -> (length of the next piece, final?)
def cut_whole(left, S, rng):
    return left, True


def cut_hop(left, S, rng):
    n = min(S, left)
    return n, n == left


def cut_half_hop(left, S, rng):
    n = min(S // 2, left)
    return n, n == left


def cut_random(left, S, rng):
    n = min(int(rng.integers(1, MAX_PUSH + 1)), left)
    return n, n == left


def cut_random_with_empty(left, S, rng):
    """Empty pushes in between, one-sample pushes, and the end always as a zero-sample final push (the flush)."""
    if left == 0:
        return 0, True
    r = rng.random()
    if r < 0.2:
        return 0, False
    if r < 0.3:
        return 1, False
    return min(int(rng.integers(1, MAX_PUSH + 1)), left), False


def _drive(m, utts, n_sessions, cut, seed, odd_offsets=False, subset=False, descending=False, host=False, on_tick=None,
           record=None):
    """Feed the utterances through n_sessions sessions (an id is reused for the next utterance on the push after its final
    one); returns the rows every utterance delivered, in order, and checks the plan's counts against the contract.
    record: a list that takes one entry per push (tests/sess_inflight.py replays them without a wait in between)."""
    import torch
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(seed)
    S, ch, width = m.cfg.shift, max(m.cfg.channels, 1), m.get_output_data_width()
    pending = list(range(len(utts)))
    cur, got = {}, {u: [] for u in range(len(utts))}
    tick = 0
    while pending or cur:
        for sid in range(n_sessions):
            if sid not in cur and pending:
                cur[sid] = [pending.pop(0), 0, 0]              # utterance, samples fed, rows delivered
        active = sorted(cur)
        if subset and len(active) > 1:                         # a changing subset of the open sessions
            keep = [s for s in active if (s + tick) % 3 != 0]
            active = keep or active[:1]
        if descending:
            active = active[::-1]
        ids, offs, lens, fins, parts, pos = [], [], [], [], [], 0
        for sid in active:
            u, fed, _ = cur[sid]
            n, fin = cut(len(utts[u]) - fed, S, rng)
            if odd_offsets and pos % 2 == 0:
                parts.append(rng.integers(-3000, 3000, (1, ch)).astype(np.int16))
                pos += 1
            elif not odd_offsets and rng.random() < 0.5:
                k = int(rng.integers(0, 4))
                parts.append(rng.integers(-3000, 3000, (k, ch)).astype(np.int16))
                pos += k
            ids.append(sid), offs.append(pos), lens.append(n), fins.append(int(fin))
            parts.append(utts[u][fed:fed + n])
            pos += n
        parts.append(np.zeros((2, ch), np.int16))
        pcm = np.concatenate(parts, 0)
        out_rows, counts, total = m.sessions_plan(ids, offs, lens, fins)
        assert total == int(counts.sum()) and list(out_rows) == list(np.cumsum(counts) - counts)
        if host:
            out = m.sessions_run_host(pcm.reshape(-1))
        else:
            d_pcm = torch.from_numpy(pcm.reshape(-1).copy()).to(dev)
            d_out = torch.full((max(total, 1), width), float("nan"), dtype=torch.float32, device=dev)
            m.sessions_run_device(d_pcm.data_ptr(), len(pcm), d_out.data_ptr())
            m.synchronize()
            out = d_out.cpu().numpy()[:total]
        delivered = []
        for sid, n, fin, r0, cnt in zip(ids, lens, fins, out_rows, counts):
            st = cur[sid]
            st[1] += n
            T = m.batch_frames(st[1])
            E = T if fin else max(0, T - _Dm(m))
            assert st[2] + cnt == E, (sid, st, cnt, E, fin)
            st[2] = E
            got[st[0]].append(out[r0:r0 + cnt].copy())
            assert m.sessions_delivered(sid) == (0 if fin else E)
            delivered.append(0 if fin else E)
            if fin:
                del cur[sid]
        if record is not None:
            record.append(dict(calls=[], ids=ids, offs=offs, lens=lens, fins=fins, pcm=pcm, out_rows=out_rows, counts=counts,
                               total=total, rows=np.array(out[:total]), delivered=delivered, host=host))
        if on_tick:
            on_tick(tick)
        tick += 1
    return {u: (np.concatenate(v, 0) if v else np.zeros((0, width), np.float32)) for u, v in got.items()}


def _Dm(m):
    return 0 if m.cfg.dyn == 0 else m.cfg.delta_l1 if m.cfg.dyn == 1 else m.cfg.delta_l1 + m.cfg.delta_l2


def _compare(name, got, want, what):
    rows = 0
    for u, w in enumerate(want):
        g = got[u]
        assert g.shape == w.shape, (name, what, u, g.shape, w.shape)
        assert np.array_equal(g.view(np.uint32), w.view(np.uint32)), (name, what, u, int((g.view(np.uint32) != w.view(np.uint32)).sum()))
        rows += len(w)
    print("sessions %-10s %-28s rows compared: %d" % (name, what, rows))
    assert rows >= sum(len(w) for w in want) and rows > 0
    return rows


PATTERNS = {
    "whole_utterance_final": dict(cut=cut_whole, n_sessions=10, max_push=17000),
    "one_hop_per_push": dict(cut=cut_hop, n_sessions=10),
    "half_hop_per_push": dict(cut=cut_half_hop, n_sessions=10),
    "random_odd_offsets": dict(cut=cut_random, n_sessions=10, odd_offsets=True),
    "random_empty_and_flush": dict(cut=cut_random_with_empty, n_sessions=10),
    "ids_reused": dict(cut=cut_random, n_sessions=6),
    "changing_subset": dict(cut=cut_random, n_sessions=8, subset=True),
    "descending_ids": dict(cut=cut_random, n_sessions=10, descending=True),
}


@pytest.mark.parametrize("pattern", sorted(PATTERNS))
def test_push_patterns_on_c1(pkg, pattern):
    utts, want = _reference(pkg, "c1")
    p = dict(PATTERNS[pattern])
    m = _make(pkg, CONFIGS["c1"])
    try:
        n_sessions = p.pop("n_sessions")
        m.sessions_create(n_sessions, p.pop("max_push", MAX_PUSH))
        got = _drive(m, utts, n_sessions, seed=11, **p)
        _compare("c1", got, want, pattern)
    finally:
        m.close()


@pytest.mark.parametrize("name", [n for n in sorted(CONFIGS) if n != "c1"])
def test_configurations(pkg, name):
    kw = CONFIGS[name]
    if name == "slab4096":       # 4096 points: spectrum through the slab + k_melcep (KERNEL_TABLE, "4096 pt")
        assert pkg.plan_kernel(kw["window_size"], kw["shift"], kw["num_banks"], kw["sample_rate"], kw["ceps_len"], dyn=kw["dyn"]) == "k_front_reg"
    utts, want = _reference(pkg, name)
    m = _make(pkg, kw)
    try:
        m.sessions_create(7, MAX_PUSH)
        got = _drive(m, utts, 7, cut_random_with_empty, seed=5, odd_offsets=True)
        _compare(name, got, want, "random")
    finally:
        m.close()


def test_narrow_loads_give_the_same_bits(pkg):
    """MFX_ENGINE_SESS_NARROW_LOADS: k_sess_gather on 2-byte loads throughout delivers the rows of the default build."""
    utts, want = _reference(pkg, "c1")
    m = _make(pkg, _c1(engine=pkg.mfcc.ENGINE_SESS_NARROW_LOADS))
    try:
        m.sessions_create(10, MAX_PUSH)
        got = _drive(m, utts, 10, cut_random, seed=11, odd_offsets=True)
        _compare("c1", got, want, "narrow loads")
    finally:
        m.close()


def test_run_host_equals_run_device(pkg):
    utts, want = _reference(pkg, "c1")
    outs = []
    for host in (False, True):
        m = _make(pkg, CONFIGS["c1"])
        try:
            m.sessions_create(6, MAX_PUSH)
            outs.append(_drive(m, utts, 6, cut_random, seed=23, odd_offsets=True, host=host))
        finally:
            m.close()
    for u in range(len(utts)):
        assert np.array_equal(outs[0][u].view(np.uint32), outs[1][u].view(np.uint32))
    _compare("c1", outs[1], want, "run_host")


def test_batch_and_streaming_state_survive_session_pushes(pkg):
    """One handle serves a planned batch with a transform, a streaming sequence and sessions, interleaved: every one of
    the three delivers what it delivers alone."""
    kw = CONFIGS["c1"]
    utts, want = _reference(pkg, "c1")
    rng = np.random.default_rng(3)
    S = kw["shift"]
    blocks = [synth_utterance(8000, 900 + k) for k in range(3)]

    def stream_step(h, k):
        if k < len(blocks):
            n = h.set_input(blocks[k])
        else:
            n = h.flush()
        h.apply()
        return h.get_output_data(n)

    alone = _make(pkg, kw)
    want_stream = [stream_step(alone, k) for k in range(len(blocks) + 1)]
    alone.close()

    m = _make(pkg, kw)
    try:
        offs = [0, 9000]
        b_pcm = np.concatenate([synth_utterance(9000, 77), synth_utterance(7001, 78), np.zeros(3, np.int16)])
        m.batch_plan(offs, [9000, 7001])
        A = rng.standard_normal((8, 3 * m.get_output_data_width())).astype(np.float32)
        m.batch_set_transform(A, None, left=1, right=1)
        batch_before = m.batch_run_host(b_pcm)
        got_stream = [stream_step(m, 0)]
        m.sessions_create(6, MAX_PUSH)
        runs = []

        def on_tick(tick):
            if tick in (1, 3, 5):
                runs.append(m.batch_run_host(b_pcm))
                got_stream.append(stream_step(m, len(got_stream)))

        got = _drive(m, utts, 6, cut_random, seed=31, on_tick=on_tick)
        assert len(runs) == 3 and len(got_stream) == 4
        _compare("c1", got, want, "interleaved")
        for r in runs + [m.batch_run_host(b_pcm)]:
            assert r.shape == batch_before.shape == (m.batch_frames(9000) + m.batch_frames(7001), 8)
            assert np.array_equal(r.view(np.uint32), batch_before.view(np.uint32))
        for g, w in zip(got_stream, want_stream):
            assert g.shape == w.shape and np.array_equal(g.view(np.uint32), w.view(np.uint32))
    finally:
        m.close()


def test_reset_plan_twice_and_run_twice(pkg):
    import torch
    dev = torch.device("cuda:0")
    utts, want = _reference(pkg, "c1")
    u = 9                                                      # the 100-frame utterance
    x, w = utts[u].reshape(-1), want[u]
    m = _make(pkg, CONFIGS["c1"])
    try:
        m.sessions_create(4, 20000)
        width = m.get_output_data_width()
        d_pcm = torch.from_numpy(np.concatenate([x, np.zeros(2, np.int16)])).to(dev)
        d_out = torch.full((len(w) + 1, width), float("nan"), dtype=torch.float32, device=dev)

        def run():
            m.sessions_run_device(d_pcm.data_ptr(), len(x), d_out.data_ptr())
            m.synchronize()
            return d_out.cpu().numpy()

        # part of the stream, then reset: the same utterance from the start gives the batch rows again
        m.sessions_plan([2], [0], [5000])
        run()
        assert m.sessions_delivered(2) == m.batch_frames(5000) - 6
        m.sessions_reset(2)
        assert m.sessions_delivered(2) == 0
        # plan twice, run once: the second plan is the one that runs
        m.sessions_plan([2], [0], [3000], [0])
        _, counts, total = m.sessions_plan([2], [0], [len(x)], [1])
        assert total == len(w) and counts[0] == len(w)
        out = run()[:total]
        assert np.array_equal(out.view(np.uint32), w.view(np.uint32))
        print("sessions c1         reset / second plan          rows compared: %d" % len(w))
        # run twice for one plan
        with pytest.raises(pkg.MfxError) as e:
            m.sessions_run_device(d_pcm.data_ptr(), len(x), d_out.data_ptr())
        assert e.value.status == -8 and str(e.value)
        # reset(-1) drops every session and a pending plan
        m.sessions_plan([0, 1], [0, 0], [1000, 2000])
        m.sessions_reset(-1)
        with pytest.raises(pkg.MfxError) as e:
            m.sessions_run_device(d_pcm.data_ptr(), len(x), d_out.data_ptr())
        assert e.value.status == -8
    finally:
        m.close()


def test_error_cases(pkg):
    import torch
    dev = torch.device("cuda:0")
    L = pkg.load_library()
    kw = CONFIGS["c1"]
    d_pcm = torch.zeros(8002, dtype=torch.int16, device=dev)
    d_out = torch.zeros((64, 39), dtype=torch.float32, device=dev)

    def status(m, fn):
        with pytest.raises(pkg.MfxError) as e:
            fn()
        assert str(e.value), "mfx_last_error is empty"
        assert L.mfx_last_error(m._h)
        return e.value.status

    m = _make(pkg, kw)
    try:
        # before mfx_sessions_create
        assert status(m, lambda: m.sessions_plan([0], [0], [10])) == -8
        assert status(m, lambda: m.sessions_run_device(d_pcm.data_ptr(), 8000, d_out.data_ptr())) == -8
        assert status(m, lambda: m.sessions_reset(0)) == -8
        assert L.mfx_sessions_delivered(m._h, 0) == -8
        assert status(m, lambda: m.sessions_create(-1, 10)) == -7
        assert status(m, lambda: m.sessions_create(4, 0)) == -7
        m.sessions_create(4, 1600)
        assert status(m, lambda: m.sessions_plan([4], [0], [10])) == -7          # id outside the range
        assert status(m, lambda: m.sessions_plan([-1], [0], [10])) == -7
        assert status(m, lambda: m.sessions_plan([1, 1], [0, 20], [10, 10])) == -7   # twice in one push
        assert status(m, lambda: m.sessions_plan([0], [0], [-1])) == -7          # negative length
        assert status(m, lambda: m.sessions_plan([0], [-2], [10])) == -7         # negative offset
        assert status(m, lambda: m.sessions_plan([0], [0], [1601])) == -1        # longer than max_push_samples
        assert status(m, lambda: m.sessions_plan([0], [2 ** 63 - 100], [1600])) == -7   # offset + length outside int64
        assert status(m, lambda: m.sessions_reset(4)) == -7
        assert L.mfx_sessions_delivered(m._h, 4) == -7
        # a refused plan leaves nothing pending, and marks no id as seen
        assert status(m, lambda: m.sessions_run_device(d_pcm.data_ptr(), 8000, d_out.data_ptr())) == -8
        m.sessions_plan([1, 0], [0, 1600], [1600, 1600])
        assert status(m, lambda: m.sessions_run_device(d_pcm.data_ptr(), 3199, d_out.data_ptr())) == -7    # a piece past the end
        assert status(m, lambda: m.sessions_run_device(d_pcm.data_ptr() + 2, 4000, d_out.data_ptr())) == -7  # misaligned
        m.sessions_run_device(d_pcm.data_ptr(), 3200, d_out.data_ptr())          # the plan was still pending: it runs
        m.synchronize()
        assert m.sessions_delivered(0) == m.sessions_delivered(1) == m.batch_frames(1600) - 6
        m.sessions_create(0, 0)                                                  # release
        assert status(m, lambda: m.sessions_plan([0], [0], [10])) == -8
    finally:
        m.close()

    # no set_window yet
    m = pkg.MfccHip(16400, 400, 160, 26, 16000.0, 64.0, 8000.0, 13, False, 22.0, pkg.NORM_NONE, pkg.DYN_ACC, 3, 3, True, device=0)
    try:
        m.sessions_create(2, 1600)
        m.sessions_plan([0], [0], [1600])
        assert status(m, lambda: m.sessions_run_device(d_pcm.data_ptr(), 8000, d_out.data_ptr())) == -8
    finally:
        m.close()

    # TRAPS and normalising handles: refused, and the message says the session entries do not serve them
    t = pkg.MfccHip(16400, 400, 160, 23, 16000.0, 64.0, 8000.0, 0, False, 22.0, pkg.NORM_NONE, pkg.DYN_NONE, 3, 3, True, device=0,
                    method=pkg.METHOD_TRAPS)
    try:
        assert status(t, lambda: t.sessions_create(2, 1600)) == -8
        assert "session entries do not serve" in L.mfx_last_error(t._h).decode()
    finally:
        t.close()
    c = pkg.MfccHip(16400, 400, 160, 26, 16000.0, 64.0, 8000.0, 13, False, 22.0, pkg.NORM_CMN, pkg.DYN_ACC, 3, 3, True, device=0)
    try:
        assert status(c, lambda: c.sessions_create(2, 1600)) == -8
        assert "session entries do not serve" in L.mfx_last_error(c._h).decode()
    finally:
        c.close()
