"""Helpers of tests/test_sess_xform_gpu.py: the session driver of tests/onorm_drive.py (copied, so that the existing file
stays as it is) with the delivery rule of a session transform -- Ex = max(0, Ey - right) while open, Ey once final -- the
width of mfx_sessions_output_width and a transform per utterance; and a brute-force model of one session's stream for the
host tests.  The configurations, utterances, cut patterns and the batch helper are onorm_drive's own.  Test infrastructure
only."""
import numpy as np

import onorm_drive as OD

CONFIGS, PATTERNS, MAX_PUSH = OD.CONFIGS, OD.PATTERNS, OD.MAX_PUSH
make, utterances, batch_rows, compare, D_of = OD.make, OD.utterances, OD.batch_rows, OD.compare, OD.D_of


def drive(m, utts, n_sessions, cut, seed, right, odd_offsets=False, subset=False, host=False, place=None, xf_of=None, on_tick=None,
          shuffle=False, record=None):
    """Feed the utterances through n_sessions sessions (an id is reused for the next utterance on the push after its final
    one; with xf_of the fresh session is given transform xf_of[u] first); returns the rows every utterance delivered, in
    order, and checks the plan's counts and mfx_sessions_delivered against the transform's delivery rule.
    place(total_rows, width): an OutPlacement-like object to run into (its check() is called after every push).
    shuffle: the pieces of every push in a random order of ids (the planner's caller order then differs from its slot order
    and from the packer's).
    record: a list that takes one entry per push, the sessions_select_transform calls in front of it included
    (tests/sess_inflight.py replays them without a wait in between)."""
    import torch
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(seed)
    S, ch, width = m.cfg.shift, max(m.cfg.channels, 1), m.sessions_output_width()
    pending = list(range(len(utts)))
    cur, got = {}, {u: [] for u in range(len(utts))}
    tick = 0
    while pending or cur:
        calls = []
        for sid in range(n_sessions):
            if sid not in cur and pending:
                cur[sid] = [pending.pop(0), 0, 0]              # utterance, samples fed, rows delivered
                if xf_of is not None:
                    m.sessions_select_transform(sid, xf_of[cur[sid][0]])
                    calls.append(("sessions_select_transform", (sid, xf_of[cur[sid][0]])))
        active = sorted(cur)
        if subset and len(active) > 1:                         # a changing subset of the open sessions
            keep = [s for s in active if (s + tick) % 3 != 0]
            active = keep or active[:1]
        if shuffle:
            active = [active[k] for k in rng.permutation(len(active))]
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
            assert out.shape == (total, width)
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
            T = max(m.batch_frames(st[1]), 0)
            Ey = T if fin else max(0, T - D_of(m))
            Ex = Ey if fin else max(0, Ey - right)
            assert st[2] + cnt == Ex, (sid, st, cnt, Ex, fin)
            st[2] = Ex
            got[st[0]].append(out[r0:r0 + cnt].copy())
            assert m.sessions_delivered(sid) == (0 if fin else Ex)
            delivered.append(0 if fin else Ex)
            if fin:
                del cur[sid]
        if record is not None:
            record.append(dict(calls=calls, ids=ids, offs=offs, lens=lens, fins=fins, pcm=pcm, out_rows=out_rows, counts=counts,
                               total=total, rows=np.array(out[:total]), delivered=delivered, host=host))
        if on_tick:
            on_tick(tick)
        tick += 1
    return {u: (np.concatenate(v, 0) if v else np.zeros((0, width), np.float32)) for u, v in got.items()}


def model_stream(T_of_push, D, left, right):
    """Brute force, from the definition: the pushes of one stream complete T_of_push[k] frames in all after push k (the last
    push is final).  Returns per push (rows delivered, the set of stream rows y its outputs read)."""
    res, Ex = [], 0
    for k, T in enumerate(T_of_push):
        fin = k == len(T_of_push) - 1
        Ey = T if fin else max(0, T - D)
        Ex_new = Ey if fin else max(0, Ey - right)
        last = T_of_push[-1] - 1
        reads = set()
        for t in range(Ex, Ex_new):
            for c in range(-left, right + 1):
                reads.add(min(max(t + c, 0), last))
        res.append((Ex_new - Ex, reads))
        Ex = Ex_new
    return res
