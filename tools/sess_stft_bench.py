"""Dev aid: a push of the session entries on an STFT log-mel handle, median device time per push between two events on the
handle's stream (and the host's time per push around the plan + run pair), all cases in one process:
  (a) N = 400, S = 160, M = 80, LOG10, 1000 sessions, pushes of 100 ms: k_sess_stft_mel (16-frame groups of different
      sessions packed four to a block) -- three times, alternating with
  (b) the same under MFX_ENGINE_SESS_STFT_PLAIN (k_stft_mel, one block per session and push) -- three times; the spread of
      each three is the noise
  (c) the same utterances, whole, as ONE mfx_batch_run_device (median of the repeats; also divided by the pushes)
The rows of (a) and (b) are compared bit for bit with (c)'s on the way.
Kernel times come from a separate run under a kernel trace (rocprofv3 --kernel-trace --stats -- python tools/sess_stft_bench.py).
Usage: sess_stft_bench.py [pushes] [sessions] [push samples]"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as G  # noqa: E402

pkg = G.load_package()
import torch  # noqa: E402

PUSHES = int(sys.argv[1]) if len(sys.argv) > 1 else 50
SESSIONS = int(sys.argv[2]) if len(sys.argv) > 2 else 1000
PUSH = int(sys.argv[3]) if len(sys.argv) > 3 else 1600
N, S, M = 400, 160, 80
LEN = PUSH * PUSHES
PLAIN = pkg.mfcc.ENGINE_SESS_STFT_PLAIN
dev = torch.device("cuda:0")
rng = np.random.default_rng(0)
d_pcm = torch.from_numpy((3000 * rng.standard_normal(SESSIONS * LEN + 2)).astype(np.int16)).to(dev)


def handle(engine=0):
    m = pkg.MfccHip(200000, N, S, M, 16000.0, 0.0, 8000.0, 0, False, 22.0, device=0, bug_compat=False,
                    method=pkg.METHOD_STFT_LOGMEL, logmel_post=pkg.mfcc.LOGMEL_LOG10, engine=engine)
    m.set_window(pkg.periodic_hann(N))
    m.set_stream(torch.cuda.current_stream().cuda_stream)    # the events below are torch's: they must be on the handle's stream
    return m


def batch(reps=9):
    """The whole utterances as one batch run: (median / min device microseconds, the rows [sessions][T][M])."""
    m = handle()
    offs = np.arange(SESSIONS, dtype=np.int64) * LEN
    rows, total = m.batch_plan(offs, np.full(SESSIONS, LEN, np.int64))
    d_out = torch.empty((total, M), dtype=torch.float32, device=dev)
    us = []
    for rep in range(reps + 2):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        m.batch_run_device(d_pcm.data_ptr(), SESSIONS * LEN + 2, d_out.data_ptr())
        b.record()
        torch.cuda.synchronize()
        if rep >= 2:                                         # (the first two warm everything up)
            us.append(1e3 * a.elapsed_time(b))
    out = d_out.cpu().numpy().reshape(SESSIONS, total // SESSIONS, M)
    m.close()
    us.sort()
    return dict(device_us_median=us[len(us) // 2], device_us_min=us[0], device_us_per_push_equivalent=us[len(us) // 2] / PUSHES,
                rows=int(total)), out


def sessions(engine, want):
    """Median / min device microseconds per push; the delivered rows against `want`."""
    m = handle(engine)
    m.sessions_create(SESSIONS, PUSH)
    per = PUSH // S + N // (2 * S) + 2
    d_out = torch.empty((PUSHES, SESSIONS * per, M), dtype=torch.float32, device=dev)
    ids = np.arange(SESSIONS, dtype=np.int32)
    base = np.arange(SESSIONS, dtype=np.int64) * LEN
    lens = np.full(SESSIONS, PUSH, np.int64)
    for rep in range(2):                                      # (the first pass warms everything up)
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(PUSHES)]
        host, plans = 0.0, []
        torch.cuda.synchronize()
        for k in range(PUSHES):
            fin = np.full(SESSIONS, int(k == PUSHES - 1), np.int32)
            t0 = time.perf_counter()
            out_rows, counts, total = m.sessions_plan(ids, base + k * PUSH, lens, fin)
            ev[k][0].record()
            m.sessions_run_device(d_pcm.data_ptr(), SESSIONS * LEN + 2, d_out[k].data_ptr())
            ev[k][1].record()
            host += time.perf_counter() - t0
            plans.append((out_rows, counts))
        torch.cuda.synchronize()
        us = sorted(1e3 * a.elapsed_time(b) for a, b in ev)
    got = d_out.cpu().numpy()
    m.close()
    at = np.zeros(SESSIONS, np.int64)
    for k, (out_rows, counts) in enumerate(plans):            # every push's rows are the batch run's bits
        for s in (0, 1, SESSIONS // 2, SESSIONS - 1):
            g, w = got[k, out_rows[s]:out_rows[s] + counts[s]], want[s, at[s]:at[s] + counts[s]]
            assert g.shape == w.shape and np.array_equal(g.view(np.uint32), w.view(np.uint32)), (engine, k, s)
        at += counts
    assert (at == want.shape[1]).all()
    return dict(device_us_per_push_median=us[len(us) // 2], device_us_per_push_min=us[0],
                host_us_per_push_plan_and_run=1e6 * host / PUSHES, rows=int(at.sum()))


res = dict(pushes=PUSHES, push_samples=PUSH, sessions=SESSIONS, N=N, S=S, M=M,
           groups_per_block=pkg.mfcc.host_sess_stft_lds_bytes(N, S, M)[1], lds_bytes=pkg.mfcc.host_sess_stft_lds_bytes(N, S, M)[0])
res["c_batch"], rows = batch()
res["a_packed"], res["b_plain"] = [], []
for _ in range(3):
    res["a_packed"].append(sessions(0, rows))
    res["b_plain"].append(sessions(PLAIN, rows))
for key in ("a_packed", "b_plain"):
    v = [r["device_us_per_push_median"] for r in res[key]]
    res[key + "_median_us"] = sorted(v)[1]
    res[key + "_spread_us"] = max(v) - min(v)
print(json.dumps(res))
