"""Helpers of tests/test_sess_stft_gpu.py: STFT log-mel handles, their batch twins, cut patterns, the delivery rule restated, and
a driver that runs streams through a pool of sessions -- one push per round, every open session a piece of it, an id reused
in the push after its final one -- checking the plan's counts against the rule and collecting every stream's rows.  With
record=[...] it notes every push in the format tests/sess_inflight.py replays.  Test infrastructure only."""
import numpy as np

LOG10, LN = 1, 2
ERR_STATE, ERR_BUFFER = -8, -1


def make(pkg, N=400, S=160, M=80, sr=16000.0, post=LOG10, engine=0, window=None):
    m = pkg.MfccHip(200000, N, S, M, sr, 0.0, sr / 2, 0, False, 22.0, device=0, bug_compat=False,
                    method=pkg.METHOD_STFT_LOGMEL, logmel_post=post, engine=engine)
    m.set_window(pkg.periodic_hann(N) if window is None else window)
    return m


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def first_difference(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    if a.shape != b.shape:
        return "shape %s vs %s" % (a.shape, b.shape)
    bad = np.argwhere(a.view(np.uint32) != b.view(np.uint32))
    return "%d values differ, first at row %d column %d" % (len(bad), bad[0][0], bad[0][1])


def frames(n, N, S):
    return 0 if n <= N // 2 else n // S


def delivered_rows(n, N, S, final):
    """E of the delivery rule (include/mfx.h, MFX_METHOD_STFT_LOGMEL, "Sessions")."""
    if final or n <= N // 2:
        return frames(n, N, S)
    return min(n // S, (n - N // 2) // S + 1)


def twins(m, utts, setup=None, rates=None):
    """Every stream as one utterance of one batch on `m` (a handle of the sessions' configuration): the rows the session
    entries must deliver, bit for bit.  setup(m) attaches what the sessions carry (the transform); rates: Hz per stream."""
    lens = np.array([len(u) for u in utts], np.int64)
    offs = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
    pcm = np.concatenate([np.asarray(u, np.int16) for u in utts] + [np.zeros(2 + int(lens.sum()) % 2, np.int16)])
    if rates is None:
        rows, total = m.batch_plan(offs, lens)
    else:
        rows, total = m.batch_plan_rates(offs, lens, list(rates))
    if setup:
        setup(m)
    out = m.batch_run_host(pcm)
    ends = list(rows[1:]) + [total]
    res = [out[int(a):int(b)].copy() for a, b in zip(rows, ends)]
    for r in res:
        r.setflags(write=False)
    return res


# ---- cut patterns: cut(n, rng) -> [(length, final)] ----------------------------------------------------------------------

def cut_whole(n, rng):
    return [(n, True)]


def cut_step(step):
    def cut(n, rng):
        out = [(min(step, n - o), False) for o in range(0, n, step)] or [(0, False)]
        out[-1] = (out[-1][0], True)
        return out
    return cut


def cut_random(n, rng, empty=False, top=700):
    """Pieces of 1 .. top samples (top: several hops, and most pieces no multiple of one); with `empty` also pushes of 0 and
    1 samples, and the end as a flush."""
    out, left = [], n
    while left > 0:
        r = rng.random()
        k = 0 if empty and r < 0.2 else 1 if empty and r < 0.3 else int(rng.integers(1, top + 1))
        k = min(k, left)
        left -= k
        out.append((k, False))
    if empty or not out:
        out.append((0, True))
    else:
        out[-1] = (out[-1][0], True)
    return out


def cut_random_empty(n, rng):
    return cut_random(n, rng, empty=True)


def cut_singles_across(at, count=12):
    """Up to `at - count / 2` samples in one piece, `count` pushes of one sample across n = at, the rest in random pieces."""
    def cut(n, rng):
        out, left = [], n
        for k in [max(at - count // 2, 0)] + [1] * count:
            k = min(k, left)
            left -= k
            out.append((k, False))
        return out + cut_random(left, rng, empty=True)
    return cut


# ---- the driver ------------------------------------------------------------------------------------------------------------

def push(m, pieces, rng, odd=False, host=False, lead=0, guard=3):
    """One push: pieces [(sid, samples, final)] laid out in one PCM array with random gaps (odd: every piece on an odd sample).
    lead: the output starts `lead` floats behind a 64-byte boundary.  Returns (rows [total][width], out_rows, counts, the plan's
    arguments)."""
    import torch
    ids, offs, lens, fins, parts, pos = [], [], [], [], [], 0
    for sid, x, fin in pieces:
        k = (1 if pos % 2 == 0 else 2) if odd else int(rng.integers(0, 4))
        parts.append(rng.integers(-32768, 32768, k).astype(np.int16))
        pos += k
        ids.append(int(sid)), offs.append(pos), lens.append(len(x)), fins.append(int(fin))
        parts.append(np.asarray(x, np.int16))
        pos += len(x)
    parts.append(rng.integers(-32768, 32768, 2 + pos % 2).astype(np.int16))
    pcm = np.concatenate(parts)
    width = m.sessions_output_width()
    out_rows, counts, total = m.sessions_plan(ids, offs, lens, fins)
    assert total == int(counts.sum()) and list(out_rows) == list(np.cumsum(counts) - counts)
    if host:
        out = m.sessions_run_host(pcm)
        assert out.shape == (total, width)
    else:
        dev = torch.device("cuda:0")
        d_pcm = torch.from_numpy(pcm).to(dev)
        big = torch.full((16 + lead + (total + guard) * width,), float("nan"), dtype=torch.float32, device=dev)
        assert big.data_ptr() % 64 == 0
        m.sessions_run_device(d_pcm.data_ptr(), len(pcm), big.data_ptr() + 4 * (16 + lead))
        m.synchronize()
        b = big.cpu().numpy()
        assert np.isnan(b[:16 + lead]).all() and np.isnan(b[16 + lead + total * width:]).all(), "a guard word was written"
        out = b[16 + lead:16 + lead + total * width].reshape(total, width).copy()
        assert np.isfinite(out).all(), "a delivered value was not written"
    return out, out_rows, counts, dict(ids=ids, offs=offs, lens=lens, fins=fins, pcm=pcm, total=total)


def drive(m, utts, n_sessions, cut, N, S, seed=0, right=0, predict=True, odd=False, host=False, lead=0, record=None, select=None,
          shuffle=True):
    """Streams utts[u] through sessions 0 .. n_sessions - 1: utterance u goes to the first free id; every round is ONE push
    with the next piece of every open session; a session whose piece was final is free for the round after.  select(sid, u) ->
    (method name, args) or None: a host call on the fresh session in front of its first push (sessions_select_rate).
    predict: the counts and mfx_sessions_delivered against the delivery rule (right: the transform's look-ahead); off under
    session rates, where n is the converted count.  Returns the rows of every utterance."""
    rng = np.random.default_rng(seed)
    width = m.sessions_output_width()
    queue, free, active, calls = list(range(len(utts))), list(range(n_sessions)), {}, []
    got = [[] for _ in utts]
    while queue or active:
        while free and queue:
            sid, u = free.pop(0), queue.pop(0)
            c = select(sid, u) if select else None
            if c:
                getattr(m, c[0])(*c[1])
                calls.append(c)
            active[sid] = dict(u=u, cuts=list(cut(len(utts[u]), rng)), pos=0, E=0)
        order = sorted(active)
        if shuffle:
            rng.shuffle(order)
        pieces = []
        for sid in order:
            a = active[sid]
            ln, fin = a["cuts"].pop(0)
            pieces.append((sid, utts[a["u"]][a["pos"]:a["pos"] + ln], fin))
            a["pos"] += ln
        out, out_rows, counts, plan = push(m, pieces, rng, odd=odd, host=host, lead=lead)
        delivered = []
        for i, (sid, x, fin) in enumerate(pieces):
            a = active[sid]
            if predict:
                Ey = delivered_rows(a["pos"], N, S, fin)
                Ex = Ey if fin else max(0, Ey - right)
                assert a["E"] + counts[i] == Ex, (sid, a["u"], a["pos"], a["E"], counts[i], Ex, fin)
                a["E"] = Ex
                assert m.sessions_delivered(sid) == (0 if fin else Ex)
                delivered.append(0 if fin else Ex)
            got[a["u"]].append(out[out_rows[i]:out_rows[i] + counts[i]])
            if fin:
                assert a["pos"] == len(utts[a["u"]]) and not a["cuts"]
                del active[sid]
                free.append(sid)
        if record is not None:
            record.append(dict(calls=calls, out_rows=out_rows, counts=counts, rows=np.array(out),
                               delivered=delivered if predict else None, host=host, **plan))
            calls = []
    return [np.concatenate(g + [np.zeros((0, width), np.float32)]) for g in got]


def compare(got, want, what):
    assert len(got) == len(want)
    for u, (g, w) in enumerate(zip(got, want)):
        assert same_bits(g, w), "%s: stream %d (%d rows): %s" % (what, u, len(w), first_difference(g, w))
