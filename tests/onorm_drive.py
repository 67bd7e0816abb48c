"""Helpers of tests/test_onorm_gpu.py: the small configurations, the cut patterns and the session driver of
tests/test_sessions_gpu.py (copied, so that the existing file stays as it is), with the normaliser's kind and place as
parameters of the handle.  Test infrastructure only."""
import numpy as np

from conftest import synth_utterance

MAX_PUSH = 3000


def _c1(**over):
    kw = dict(window_size=400, shift=160, num_banks=26, sample_rate=16000.0, ceps_len=13, dyn=2, delta_l1=3, delta_l2=3,
              fft_size=0, channels=1, method=0, lpc_order=0, alpha=1.0, engine=0, traps_len=0, traps_dct_len=0)
    kw.update(over)
    return kw


CONFIGS = {
    "c1": _c1(),
    "dyn_none": _c1(dyn=0),
    "fbank40": _c1(num_banks=40, ceps_len=0),
    "stereo44k": _c1(window_size=1102, shift=441, num_banks=128, sample_rate=44100.0, ceps_len=40, channels=2),
    "plp12": _c1(method=1, lpc_order=12),
    "traps150": _c1(num_banks=15, ceps_len=0, dyn=0, method=3, traps_len=31, traps_dct_len=10),   # batch entries only
}


def cols_of(kw):
    if kw["method"] == 3:                                    # TRAPS
        return kw["num_banks"] * kw["traps_dct_len"]
    return kw["ceps_len"] if kw["ceps_len"] else kw["num_banks"]


def make(pkg, kw, norm=0, nad=True, **over):
    import torch
    kw = dict(kw, **over)
    m = pkg.MfccHip(100 * kw["shift"] + kw["window_size"], kw["window_size"], kw["shift"], kw["num_banks"], kw["sample_rate"],
                    64.0, kw["sample_rate"] / 2, kw["ceps_len"], False, 22.0, norm, kw["dyn"], kw["delta_l1"],
                    kw["delta_l2"], nad, device=0, fft_size=kw["fft_size"], channels=kw["channels"], method=kw["method"],
                    lpc_order=kw["lpc_order"], engine=kw["engine"], traps_len=kw["traps_len"], traps_dct_len=kw["traps_dct_len"])
    assert m.get_output_data_width() == cols_of(kw) * (1 + kw["dyn"])
    # torch's stream: the NaN fills and copies of the tests and the handle's launches are then ordered with each other
    m.set_stream(torch.cuda.current_stream().cuda_stream)
    m.set_window(pkg.reference_window(kw["window_size"]))
    m.set_alpha(kw["alpha"])
    return m


def utterances(name, frames, silent_frames=40):
    """One utterance per frame count (a few samples past the last frame), then one all-zero utterance."""
    kw = CONFIGS[name]
    W, S, ch = kw["window_size"], kw["shift"], kw["channels"]
    rng = np.random.default_rng(sum(map(ord, name)))
    utts = []
    for k, T in enumerate(frames):
        n = int(rng.integers(0, W)) if T == 0 else W + (T - 1) * S + int(rng.integers(0, S))
        utts.append(synth_utterance(n * ch, 7 * len(name) + k, sr=kw["sample_rate"]).reshape(n, ch))
    utts.append(np.zeros((W + (silent_frames - 1) * S + 11, ch), np.int16))
    return utts


def layout(utts):
    """Even offsets, two samples of slack: (offsets, lengths, pcm [samples][channels])."""
    ch = utts[0].shape[1]
    offs, pos = [], 0
    for x in utts:
        offs.append(pos)
        pos += (len(x) + 1) & ~1
    pcm = np.zeros((pos + 2, ch), np.int16)
    for o, x in zip(offs, utts):
        pcm[o:o + len(x)] = x
    return offs, [len(x) for x in utts], pcm


def batch_rows(m, utts, setup=None):
    """Plan, (setup), run from the host: the rows of every utterance."""
    offs, lens, pcm = layout(utts)
    rows, total = m.batch_plan(offs, lens)
    if setup:
        setup(m)
    out = m.batch_run_host(pcm.reshape(-1))
    return [out[r:r + m.batch_frames(n)].copy() for r, n in zip(rows, lens)]


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


PATTERNS = {
    "whole_utterance_final": dict(cut=cut_whole, n_sessions=10, max_push=33000),
    "one_hop_per_push": dict(cut=cut_hop, n_sessions=13),
    "half_hop_per_push": dict(cut=cut_half_hop, n_sessions=13),
    "random_empty_and_flush": dict(cut=cut_random_with_empty, n_sessions=10),
    "ids_reused": dict(cut=cut_random, n_sessions=4),
    "changing_subset": dict(cut=cut_random, n_sessions=8, subset=True),
}


def D_of(m):
    return 0 if m.cfg.dyn == 0 else m.cfg.delta_l1 if m.cfg.dyn == 1 else m.cfg.delta_l1 + m.cfg.delta_l2


def drive(m, utts, n_sessions, cut, seed, odd_offsets=False, subset=False, host=False, place=None, record=None):
    """Feed the utterances through n_sessions sessions (an id is reused for the next utterance on the push after its final
    one); returns the rows every utterance delivered, in order, and checks the plan's counts against the contract.
    place(total_rows, width): an OutPlacement-like object to run into (its check() is called after every push).
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
        elif place is not None and total > 0:
            d_pcm = torch.from_numpy(pcm.reshape(-1).copy()).to(dev)
            op = place(total, width)
            m.sessions_run_device(d_pcm.data_ptr(), len(pcm), op.ptr)
            m.synchronize()
            out = op.check("push %d" % tick).cpu().numpy()
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
            E = T if fin else max(0, T - D_of(m))
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
        tick += 1
    return {u: (np.concatenate(v, 0) if v else np.zeros((0, width), np.float32)) for u, v in got.items()}


def compare(name, got, want, what):
    rows = 0
    for u, w in enumerate(want):
        g = got[u]
        assert g.shape == w.shape, (name, what, u, g.shape, w.shape)
        assert np.array_equal(g.view(np.uint32), w.view(np.uint32)), (name, what, u, int((g.view(np.uint32) != w.view(np.uint32)).sum()))
        rows += len(w)
    print("online sessions %-10s %-40s rows compared: %d" % (name, what, rows))
    assert rows > 0
    return rows
