"""Helpers of tests/test_sess_inflight_gpu.py: session pushes queued back to back, with no wait between them.

The four session drives (tests/test_sessions_gpu.py, onorm_drive.py, sess_xform_drive.py, sess_resample_drive.py) wait after
every push.  Run with record=[...] they note every push -- the host calls in front of it, the plan's arguments, its PCM, what
mfx_sessions_plan answered, the rows delivered and what mfx_sessions_delivered must say afterwards.  replay() runs such a
record on a fresh handle of the same configuration out of two resident arenas, behind a filler of plain torch work on the
handle's stream, so that push k is queued while push k - 1 (and the upload out of the other pinned staging buffer) has not
run yet, and compares every push with the record bit for bit.  Test infrastructure only."""
import contextlib
import math
import time

import numpy as np

GUARD = 3            # NaN rows behind every push's rows in the output arena
MARGIN = 4           # the filler lasts MARGIN x the host's time for one plan + run (host jitter between measurement and use)
SHARE = 0.75         # of a replay's pushes must have been queued onto a stream that had not reached them
FILLER_N = 2048      # a @ a on [FILLER_N][FILLER_N] float32: long on the device against the host's cost of launching it


class Filler:
    """`count` times a @ a on a resident float32 matrix, the product discarded into a resident buffer."""

    def __init__(self, n=FILLER_N):
        import torch
        self.a = torch.full((n, n), 1.0 / n, dtype=torch.float32, device="cuda:0")
        self.out = torch.empty_like(self.a)
        self.count = 1
        self.t_host = self.t_unit = float("nan")

    def queue(self):
        import torch
        for _ in range(self.count):
            torch.mm(self.a, self.a, out=self.out)


def _upload(record, dev):
    """The PCM of every push in one device array, every piece of it on an even element (4-byte aligned pointers)."""
    import torch
    parts, offs, pos = [], [], 0
    for e in record:
        x = np.ascontiguousarray(e["pcm"], np.int16).reshape(-1)
        offs.append(pos)
        parts.append(x)
        pos += len(x)
        if pos % 2:
            parts.append(np.zeros(1, np.int16))
            pos += 1
    host = np.concatenate(parts + [np.zeros(2, np.int16)])
    return host, torch.from_numpy(host).to(dev), offs


def calibrate(m, record, stream, filler):
    """The synchronised warm-up on a throw-away handle: t_host, the median wall time of sessions_plan + sessions_run_device
    over the record's pushes; t_unit, the device time of one filler operation between a pair of events; the filler's count
    is ceil(MARGIN t_host / t_unit)."""
    import torch
    dev = torch.device("cuda:0")
    width = m.sessions_output_width()
    with torch.cuda.stream(stream):
        host, d_pcm, offs = _upload(record, dev)
        d_out = torch.empty((max(e["total"] for e in record) + 1, width), dtype=torch.float32, device=dev)
        filler.count = 1
        for _ in range(3):
            filler.queue()
        torch.cuda.synchronize()
        times = []
        for k, e in enumerate(record):
            for name, args in e["calls"]:
                getattr(m, name)(*args)
            t0 = time.perf_counter()
            m.sessions_plan(e["ids"], e["offs"], e["lens"], e["fins"])
            m.sessions_run_device(d_pcm.data_ptr() + 2 * offs[k], len(e["pcm"]), d_out.data_ptr())
            times.append(time.perf_counter() - t0)
            m.synchronize()
        reps = 16
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev0.record()
        for _ in range(reps):
            filler.queue()
        ev1.record()
        torch.cuda.synchronize()
    filler.t_host = float(np.median(times))
    filler.t_unit = ev0.elapsed_time(ev1) * 1e-3 / reps
    filler.count = max(1, math.ceil(MARGIN * filler.t_host / filler.t_unit))
    print("in-flight filler: t_host %.1f us (median of %d pushes), t_unit %.1f us ([%d][%d] float32 a @ a), %d operations per push"
          % (filler.t_host * 1e6, len(times), filler.t_unit * 1e6, FILLER_N, FILLER_N, filler.count))
    return filler


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def replay(m, record, stream=None, filler=None, between=None, what=""):
    """Run the record's pushes on `m` (a fresh handle of the record's configuration, attachments and sessions_create, already
    on `stream`) back to back.  Everything is made resident first; from the first push to the one m.synchronize() behind the
    last nothing here waits (a push recorded with host=True runs through sessions_run_host, which waits by its contract).
    between: {push index: callable}, run in front of that push's filler (other entries of the handle, on resident buffers).
    stream=None, filler=None: the handle's own stream -- no filler can be put there, so no in-flight share is asserted.
    Returns (rows per push, pushes queued onto a stream that had not reached them)."""
    import torch
    dev = torch.device("cuda:0")
    width = m.sessions_output_width()
    between = between or {}
    row0, rows = [], 0
    for e in record:
        row0.append(rows)
        rows += e["total"] + GUARD
    with (torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext()):
        host_pcm, d_pcm, offs = _upload(record, dev)
        d_out = torch.full((rows, width), float("nan"), dtype=torch.float32, device=dev)
        events = [torch.cuda.Event() for _ in record] if filler is not None else []
        pcm_ptr, out_ptr = d_pcm.data_ptr(), d_out.data_ptr()
        ahead, host_rows = [], {}
        torch.cuda.synchronize()
        # ---- nothing below waits, up to m.synchronize()
        for k, e in enumerate(record):
            for name, args in e["calls"]:
                getattr(m, name)(*args)
            if k in between:
                between[k]()
            if filler is not None:
                filler.queue()
                events[k].record()
            out_rows, counts, total = m.sessions_plan(e["ids"], e["offs"], e["lens"], e["fins"])
            # (host arithmetic: it must not depend on how far the device has come)
            assert total == e["total"] and list(out_rows) == list(e["out_rows"]) and list(counts) == list(e["counts"]), (what, k)
            if e["host"]:
                host_rows[k] = m.sessions_run_host(np.ascontiguousarray(e["pcm"]).reshape(-1))
            else:
                m.sessions_run_device(pcm_ptr + 2 * offs[k], len(e["pcm"]), out_ptr + 4 * width * row0[k])
            if filler is not None:
                ahead.append(not events[k].query())
            if e["delivered"] is not None:
                for sid, want in zip(e["ids"], e["delivered"]):
                    assert m.sessions_delivered(sid) == want, (what, k, sid)
        m.synchronize()
        out = d_out.cpu().numpy()
        pcm_back = d_pcm.cpu().numpy()

    # ---- the checks
    got, uploads, fed = [], 0, {}
    for k, e in enumerate(record):
        # (which pinned staging buffer the push's lists went through, counted as mfx_sessions_run_device does)
        for name, args in e["calls"]:
            if name == "sessions_reset":
                fed[args[0]] = 0
        up = any(n > 0 or (f and fed.get(s, 0) > 0) for s, n, f in zip(e["ids"], e["lens"], e["fins"]))
        for s, n, f in zip(e["ids"], e["lens"], e["fins"]):
            fed[s] = 0 if f else fed.get(s, 0) + n
        where = "%s: push %d of %d (staging buffer %s)" % (what, k, len(record), uploads % 2 if up else "unused")
        uploads += up
        total = e["total"]
        arena = out[row0[k]:row0[k] + total + GUARD]
        g = host_rows[k] if e["host"] else arena[:total]
        want = np.asarray(e["rows"], np.float32).reshape(total, width)
        assert g.shape == want.shape, (where, g.shape, want.shape)
        if not _same_bits(g, want):
            bad = np.argwhere(g.view(np.uint32) != want.view(np.uint32))
            r = int(bad[0][0])
            piece = max(i for i, r0 in enumerate(e["out_rows"]) if r0 <= r)
            raise AssertionError("%s: %d values differ from the synchronised pass, first at row %d column %d: piece %d (session %d, "
                                 "its row %d)" % (where, len(bad), r, int(bad[0][1]), piece, e["ids"][piece], r - int(e["out_rows"][piece])))
        guard = arena if e["host"] else arena[total:]
        assert np.isnan(guard).all(), "%s: a guard row was written" % where
        got.append(g.copy())
    assert np.array_equal(pcm_back, host_pcm), "%s: the PCM arena changed" % what
    n_ahead = sum(ahead)
    if filler is not None:
        print("in flight %-44s pushes %3d, queued ahead of the device %3d, rows %d" % (what, len(record), n_ahead, rows - GUARD * len(record)))
        assert n_ahead >= SHARE * len(record), \
            "%s: inconclusive: only %d of %d pushes were queued onto a stream that had not reached them" % (what, n_ahead, len(record))
    return got, n_ahead
