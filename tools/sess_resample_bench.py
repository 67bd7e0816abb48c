"""Dev aid: what the session rates (mfx_sessions_set_rates) add to a push -- median device time per push between two events on
the handle's stream (and the host's time per push around the plan + run pair), all fleets in one process, C2 shape, 1000
sessions, pushes of 100 ms at every session's own rate:
  (a) no rates set -- three times; the spread of the three is the noise
  (b) all sessions at 48 kHz        (c) all at 8 kHz        (d) all at 44.1 kHz
  (e) an even mix of 48 / 8 / 44.1 / 16 kHz (the 16 kHz quarter is copied into the scratch by the same launch)
  (f) rates set, all sessions pass-through (16 kHz): no conversion launch is queued
Every case also reports launches_per_push = whether the push queued k_sess_resample (mfx_sessions_converted_read answers
MFX_ERR_STATE after a push that did not).  Kernel times come from a separate run under a kernel trace (rocprofv3
--kernel-trace --stats -- python tools/sess_resample_bench.py).
Usage: sess_resample_bench.py [pushes] [sessions] [fleets, e.g. "be": only those letters (a kernel trace of one fleet)]"""
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
N = int(sys.argv[2]) if len(sys.argv) > 2 else 1000
ONLY = sys.argv[3] if len(sys.argv) > 3 else "abcdef"
W, S, SR = 400, 160, 16000
dev = torch.device("cuda:0")


def case(rates):
    """Median / min device microseconds per push of N sessions; session s runs at rates[s % len(rates)] (None: no rates set)."""
    m = pkg.MfccHip(SR * PUSHES // 10, W, S, 40, float(SR), 64.0, 8000.0, 13, False, 22.0, pkg.NORM_NONE, pkg.DYN_ACC, 3, 3, True)
    m.set_window(pkg.reference_window(W))
    m.set_stream(torch.cuda.current_stream().cuda_stream)    # the events below are torch's: they must be on the handle's stream
    of = [SR if rates is None else rates[s % len(rates)] for s in range(N)]
    push = np.array([r // 10 for r in of], np.int64)           # 100 ms of every session's rate
    if rates is not None:
        m.sessions_set_rates(rates)
    m.sessions_create(N, int(push.max()))
    if rates is not None:
        for s in range(N):
            m.sessions_select_rate(s, s % len(rates))
    total_len = push * PUSHES
    base = np.concatenate([[0], np.cumsum(total_len + (total_len & 1))[:-1]]).astype(np.int64)
    n_all = int(base[-1] + total_len[-1] + 2)
    rng = np.random.default_rng(0)
    d_pcm = torch.from_numpy((3000 * rng.standard_normal(n_all)).astype(np.int16)).to(dev)
    width = m.sessions_output_width()
    d_out = torch.empty((N * (SR // 10 // S + 12), width), dtype=torch.float32, device=dev)
    ids = np.arange(N, dtype=np.int32)
    converted = False
    for rep in range(2):                                      # (the first pass warms everything up)
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(PUSHES)]
        host, rows = 0.0, 0
        torch.cuda.synchronize()
        for k in range(PUSHES):
            fin = np.full(N, int(k == PUSHES - 1), np.int32)
            t0 = time.perf_counter()
            _, _, total = m.sessions_plan(ids, base + k * push, push, fin)
            ev[k][0].record()
            m.sessions_run_device(d_pcm.data_ptr(), n_all, d_out.data_ptr())
            ev[k][1].record()
            host += time.perf_counter() - t0
            rows += total
        torch.cuda.synchronize()
        us = sorted(1e3 * a.elapsed_time(b) for a, b in ev)
    if rates is not None:
        converted = int(m._L.mfx_sessions_converted_read(m._h, None, 0, None, None)) >= 0
    want = sum(m.batch_frames(pkg.mfcc.host_resampled_length(int(n), r, SR)) for n, r in zip(total_len, of))
    assert rows == want, (rows, want)
    m.close()
    return dict(device_us_per_push_median=us[len(us) // 2], device_us_per_push_min=us[0],
                host_us_per_push_plan_and_run=1e6 * host / PUSHES, rows=rows, conversion_launch=converted,
                input_samples_per_push=int(push.sum()))


res = dict(pushes=PUSHES, sessions=N)
FLEETS = dict(b_all_48000=[48000], c_all_8000=[8000], d_all_44100=[44100], e_mix_48000_8000_44100_16000=[48000, 8000, 44100, SR],
              f_rates_set_all_pass_through=[SR])
if "a" in ONLY:
    res["a_no_rates"] = [case(None) for _ in range(3)]
    a = [r["device_us_per_push_median"] for r in res["a_no_rates"]]
    res["noise_us"] = max(a) - min(a)
for name, rates in FLEETS.items():
    if name[0] in ONLY:
        res[name] = case(rates)
print(json.dumps(res))
