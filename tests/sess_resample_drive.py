"""Helpers of tests/test_sess_resample_gpu.py: the feature configuration and signals of tests/test_resample_gpu.py (restated, so
that the existing file stays as it is), the batch twin of a stream under mfx_batch_plan_rates, cut patterns, and a driver that
runs pushes of several sessions at their own rates and collects every piece's converted samples and rows, checking the plan's
counts against the delivery rule.  Test infrastructure only."""
import numpy as np

W, S, SR = 400, 160, 16000
RATES = (48000, 8000, 44100, 11025, 17600, 12345)
ERR_ARG, ERR_STATE = -7, -8


def make(pkg, channels=1, norm=0, **kw):
    m = pkg.MfccHip(400000, W, S, 40, float(SR), 64.0, SR / 2.0, 13, False, 22.0, norm, 2, 3, 3, True, device=0,
                    bug_compat=False, channels=channels, fft_size=0, method=pkg.METHOD_MFCC, **kw)
    m.set_window(pkg.reference_window(W))
    return m


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def signal(kind, n, rate, seed):
    t = np.arange(n)
    if kind == 0:                                           # full-scale noise
        return np.random.default_rng(900 + seed).integers(-32768, 32768, n).astype(np.int16)
    if kind == 1:                                           # a 997 Hz sine
        return np.rint(30000.0 * np.sin(2 * np.pi * 997.0 * t / rate)).astype(np.int16)
    return np.where((t // 23) % 2 == 0, 32767, -32768).astype(np.int16)   # full-scale square wave: the overshoot saturates


def stream(kind, n, rate, seed, channels=1):
    """[n][channels]; the second channel is another signal kind, so that a channel mix-up shows."""
    cols = [signal((kind + c) % 3, n, rate, seed + 17 * c) for c in range(channels)]
    return np.stack(cols, 1) if n else np.zeros((0, channels), np.int16)


def shape(pkg, rate):
    """(L, M, Wh) of rate -> SR; (1, 1, 0) for the pass-through."""
    if rate == SR:
        return 1, 1, 0
    h, L, M, P = pkg.mfcc.host_resample_taps(rate, SR)
    return L, M, P // 2


def converted_count(pkg, rate, N, final):
    L, M, Wh = shape(pkg, rate)
    if rate == SR:
        return N
    return -(-N * L // M) if final else max(0, -(-(N - Wh) * L // M))


def twins(pkg, xs, rates, setup=None, norm=0, make_handle=None):
    """The batch twins: every stream as one utterance of one batch under mfx_batch_plan_rates (an utterance's samples and
    rows do not depend on its neighbours: tests/test_resample_gpu.py).  Returns per stream (converted [J][ch], rows); a
    stream without samples has neither, by the definition (N_out = 0, T = 0).  make_handle(pkg, channels=, norm=): the handle
    of another configuration at SR (default: this module's make)."""
    mk = make_handle or make
    ch = xs[0].shape[1]
    if not any(len(x) for x in xs):
        m = mk(pkg, channels=ch, norm=norm)
        width = m.get_output_data_width()
        m.close()
        return [(np.zeros((0, ch), np.int16), np.zeros((0, width), np.float32)) for x in xs]
    m = mk(pkg, channels=ch, norm=norm)
    offs, pos, parts = [], 0, []
    for x in xs:
        offs.append(pos)
        parts.append(x)
        pos += len(x)
    parts.append(np.zeros((2 + pos % 2, ch), np.int16))
    row0, total = m.batch_plan_rates(offs, [len(x) for x in xs], list(rates))
    if setup:
        setup(m)
    rows = m.batch_run_host(np.concatenate(parts, 0).reshape(-1))
    y = m.debug_read(8).reshape(-1, ch)
    off, ln, _ = m.batch_resample_layout()
    out = []
    for u, (x, r) in enumerate(zip(xs, rates)):
        J = converted_count(pkg, r, len(x), True)
        assert ln[u] == J
        T = max(m.batch_frames(J), 0)
        a, b = y[off[u]:off[u] + J].copy(), rows[row0[u]:row0[u] + T].copy()
        a.setflags(write=False), b.setflags(write=False)
        out.append((a, b))
    m.close()
    return out


def twin(pkg, x, rate, setup=None, norm=0, make_handle=None):
    return twins(pkg, [x], [rate], setup=setup, norm=norm, make_handle=make_handle)[0]


# ---- cut patterns: lists of (length, final) -------------------------------------------------------------------------------

def cut_one(n):
    return [(n, True)]


def cut_even(n, step):
    out = [(min(step, n - o), False) for o in range(0, n, step)] or [(0, False)]
    out[-1] = (out[-1][0], True)
    return out


def cut_random(n, Wh, top, seed):
    """Pushes of 0, 1 and fewer than Wh samples -- at the start of the stream, where nothing can be converted yet, and again
    between random pieces of up to `top` -- and the end as an empty flush."""
    rng = np.random.default_rng(seed)
    small = [0, 1, max(Wh - 2, 2), 0, Wh - 1]
    out, left = [], n
    while left > 0:
        if small:
            c = small.pop(0)
        else:
            c = int(rng.integers(1, top + 1))
            if rng.random() < 0.5:
                small = [int(rng.integers(0, 2)), int(rng.integers(2, Wh))]
        c = min(c, left)
        out.append((c, False))
        left -= c
    out.append((0, True))
    return out


def cut_lengths(lengths):
    return [(int(c), False) for c in lengths[:-1]] + [(int(lengths[-1]), True)]


# ---- the driver --------------------------------------------------------------------------------------------------------------

class Fleet:
    """Sessions of one handle, each at its rate; push() runs one push and files every piece's converted samples and rows under
    the stream it belongs to.
    record: a list that takes one entry per push, the host calls made through call() in front of it included
    (tests/sess_inflight.py replays them without a wait in between)."""

    def __init__(self, pkg, m, seed=0, record=None):
        self.pkg, self.m, self.rng = pkg, m, np.random.default_rng(seed)
        self.record, self.calls = record, []
        self.ch = max(m.cfg.channels, 1)
        self.state = {}                                   # sid -> [key, rate, N_in, J, rows delivered]
        self.conv, self.rows = {}, {}
        self.launches = []                                # per push: did it convert

    def open(self, sid, key, rate):
        assert sid not in self.state
        self.state[sid] = [key, rate, 0, 0, 0]
        self.conv[key], self.rows[key] = [], []

    def drop(self, sid):
        del self.state[sid]

    def call(self, name, *args):
        """A host call on the handle between two pushes (sessions_select_rate, sessions_reset), noted for the record."""
        getattr(self.m, name)(*args)
        self.calls.append((name, args))

    def push(self, pieces, odd=False, host=False, place=None, right=0, D=6, check_rows=True):
        """pieces: [(sid, samples [n][ch], final)].  odd: every piece on an odd sample of the caller's array."""
        import torch
        m, ch, rng = self.m, self.ch, self.rng
        ids, offs, lens, fins, parts, pos = [], [], [], [], [], 0
        for sid, x, fin in pieces:
            if odd:
                k = 1 if pos % 2 == 0 else 2
            else:
                k = int(rng.integers(0, 4))
            parts.append(rng.integers(-32768, 32768, (k, ch)).astype(np.int16))
            pos += k
            ids.append(sid), offs.append(pos), lens.append(len(x)), fins.append(int(fin))
            parts.append(np.asarray(x, np.int16).reshape(-1, ch))
            pos += len(x)
        parts.append(rng.integers(-32768, 32768, (2 + pos % 2, ch)).astype(np.int16))
        pcm = np.concatenate(parts, 0)
        if odd:
            assert all(o % 2 == 1 for o in offs)
        width = m.sessions_output_width()
        out_rows, counts, total = m.sessions_plan(ids, offs, lens, fins)
        assert total == int(counts.sum()) and list(out_rows) == list(np.cumsum(counts) - counts)
        if host:
            out = m.sessions_run_host(pcm.reshape(-1))
            assert out.shape == (total, width)
        else:
            dev = torch.device("cuda:0")
            d_pcm = torch.from_numpy(pcm.reshape(-1).copy()).to(dev)
            if place is not None and total > 0:
                op = place(total, width)
                m.sessions_run_device(d_pcm.data_ptr(), len(pcm), op.ptr)
                m.synchronize()
                out = op.check("push").cpu().numpy()
            else:
                d_out = torch.full((max(total, 1), width), float("nan"), dtype=torch.float32, device=dev)
                m.sessions_run_device(d_pcm.data_ptr(), len(pcm), d_out.data_ptr())
                m.synchronize()
                out = d_out.cpu().numpy()[:total]
        try:
            conv = m.sessions_converted_read(len(ids))
            self.launches.append(True)
        except self.pkg.MfxError as e:                   # no conversion launch: the converted samples are the caller's own
            assert e.status == ERR_STATE
            conv = None
            self.launches.append(False)
        delivered = []
        for i, (sid, x, fin) in enumerate(pieces):
            st = self.state[sid]
            key, rate = st[0], st[1]
            st[2] += len(x)
            J = converted_count(self.pkg, rate, st[2], fin)
            if conv is not None:
                piece = conv[i]
            else:                                         # (only pass-through pieces, or pieces that convert nothing)
                assert rate == SR or J == st[3]
                piece = np.asarray(x, np.int16).reshape(-1, ch) if rate == SR else np.zeros((0, ch), np.int16)
            assert len(piece) == J - st[3], (sid, rate, st, len(piece), J, fin)
            st[3] = J
            self.conv[key].append(piece)
            if check_rows:
                T = max(m.batch_frames(J), 0)
                Ey = T if fin else max(0, T - D)
                Ex = Ey if fin else max(0, Ey - right)
                assert st[4] + counts[i] == Ex, (sid, st, counts[i], Ex, fin)
                st[4] = Ex
                assert m.sessions_delivered(sid) == (0 if fin else Ex)
                delivered.append(0 if fin else Ex)
            self.rows[key].append(out[out_rows[i]:out_rows[i] + counts[i]].copy())
            if fin:
                del self.state[sid]
        if self.record is not None:
            self.record.append(dict(calls=self.calls, ids=ids, offs=offs, lens=lens, fins=fins, pcm=pcm, out_rows=out_rows,
                                    counts=counts, total=total, rows=np.array(out[:total]),
                                    delivered=delivered if check_rows else None, host=host))
            self.calls = []
        return out

    def converted(self, key):
        return np.concatenate(self.conv[key] + [np.zeros((0, self.ch), np.int16)], 0)

    def delivered(self, key):
        w = self.m.sessions_output_width()
        return np.concatenate(self.rows[key] + [np.zeros((0, w), np.float32)], 0)


def feed(fleet, sid, key, rate, x, cuts, **kw):
    """One stream through one session, cut as `cuts` says."""
    fleet.open(sid, key, rate)
    o = 0
    for n, fin in cuts:
        fleet.push([(sid, x[o:o + n], fin)], **kw)
        o += n
    assert o == len(x)
