"""Dev aid: what the session transform (mfx_sessions_set_transform) adds to a push, median device time per push between two
events on the handle's stream (and the host's time per push around the plan + run pair), all cases in one process:
  (a) C2 shape, 1000 sessions, pushes of 100 ms, no transform -- three times; the spread of the three is the noise
  (b) the same with +-4 -> 40 (k_sess_xform, row groups of different sessions packed into one block)
  (c) the same under MFX_ENGINE_SESS_XFORM_PLAIN (k_splice_affine, one segment per session)
  (d) (b) with 16 transforms dealt round-robin
  (e) 256 sessions at in_dim near 8192 -> 256 (fbank 64 + d: Wd = 128, left 32, right 30: in_dim 8064), packed and plain
Kernel times come from a separate run under a kernel trace (rocprofv3 --kernel-trace --stats -- python tools/sess_xform_bench.py).
Usage: sess_xform_bench.py [pushes] [sessions of (a)-(d)] [sessions of (e)]"""
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
N_C2 = int(sys.argv[2]) if len(sys.argv) > 2 else 1000
N_BIG = int(sys.argv[3]) if len(sys.argv) > 3 else 256
W, S, PUSH = 400, 160, 1600
PLAIN = pkg.mfcc.ENGINE_SESS_XFORM_PLAIN
dev = torch.device("cuda:0")


def case(n, nb, nc, dyn, xform=None, n_xf=1, engine=0):
    """Median / min device microseconds per push of n sessions; xform = (left, right, out_dim) or None."""
    LEN = PUSH * PUSHES
    m = pkg.MfccHip(LEN, W, S, nb, 16000.0, 64.0, 8000.0, nc, False, 22.0, pkg.NORM_NONE, dyn, 3, 3, True, engine=engine)
    m.set_window(pkg.reference_window(W))
    m.set_stream(torch.cuda.current_stream().cuda_stream)    # the events below are torch's: they must be on the handle's stream
    rng = np.random.default_rng(0)
    d_pcm = torch.from_numpy((3000 * rng.standard_normal(n * LEN)).astype(np.int16)).to(dev)
    Wd = m.get_output_data_width()
    if xform:
        left, right, od = xform
        in_dim = (left + right + 1) * Wd
        A = (rng.standard_normal((n_xf, od, in_dim)) / np.sqrt(in_dim)).astype(np.float32)
        m.sessions_set_transform(A, rng.standard_normal((n_xf, od)).astype(np.float32), left=left, right=right)
    m.sessions_create(n, PUSH)
    if xform and n_xf > 1:
        for s in range(n):
            m.sessions_select_transform(s, s % n_xf)
    width = m.sessions_output_width()
    d_out = torch.empty((n * (PUSH // S + 8 + (xform[1] if xform else 0)), width), dtype=torch.float32, device=dev)
    ids = np.arange(n, dtype=np.int32)
    base = np.arange(n, dtype=np.int64) * LEN
    lens = np.full(n, PUSH, np.int64)
    for rep in range(2):                                      # (the first pass warms everything up)
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(PUSHES)]
        host, rows = 0.0, 0
        torch.cuda.synchronize()
        for k in range(PUSHES):
            fin = np.full(n, int(k == PUSHES - 1), np.int32)
            t0 = time.perf_counter()
            _, _, total = m.sessions_plan(ids, base + k * PUSH, lens, fin)
            ev[k][0].record()
            m.sessions_run_device(d_pcm.data_ptr(), n * LEN, d_out.data_ptr())
            ev[k][1].record()
            host += time.perf_counter() - t0
            rows += total
        torch.cuda.synchronize()
        us = sorted(1e3 * a.elapsed_time(b) for a, b in ev)
    assert rows == n * m.batch_frames(LEN), (rows, n * m.batch_frames(LEN))
    m.close()
    return dict(device_us_per_push_median=us[len(us) // 2], device_us_per_push_min=us[0],
                host_us_per_push_plan_and_run=1e6 * host / PUSHES, rows=rows, row_width=width)


res = dict(pushes=PUSHES, push_samples=PUSH, sessions_c2=N_C2, sessions_big=N_BIG)
res["a_no_transform"] = [case(N_C2, 40, 13, pkg.DYN_ACC) for _ in range(3)]
res["b_packed_c2_4_4_40"] = case(N_C2, 40, 13, pkg.DYN_ACC, (4, 4, 40))
res["c_plain_c2_4_4_40"] = case(N_C2, 40, 13, pkg.DYN_ACC, (4, 4, 40), engine=PLAIN)
res["d_packed_c2_16_transforms"] = case(N_C2, 40, 13, pkg.DYN_ACC, (4, 4, 40), n_xf=16)
res["e_packed_8064_256"] = case(N_BIG, 64, 0, pkg.mfcc.DYN_DELTA, (32, 30, 256))
res["e_plain_8064_256"] = case(N_BIG, 64, 0, pkg.mfcc.DYN_DELTA, (32, 30, 256), engine=PLAIN)
a = [r["device_us_per_push_median"] for r in res["a_no_transform"]]
res["noise_us"] = max(a) - min(a)
print(json.dumps(res))
