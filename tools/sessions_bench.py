"""Dev aid: the session entries on the C2 shape -- 1000 open streams of 10 s, fed as 100 pushes of 100 ms, PCM resident in
HBM -- beside the two ways the same job is done without them: one streaming handle fed the 1000 utterances one after the
other, and the 1000 complete utterances as one batch run (the ceiling; three runs, their spread is the noise).
Usage: sessions_bench.py [engine bits] [sessions] [pushes]   (engine 2048 = k_sess_gather with 2-byte loads)"""
import ctypes as C
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

ENGINE = int(sys.argv[1]) if len(sys.argv) > 1 else 0
N = int(sys.argv[2]) if len(sys.argv) > 2 else 1000
PUSHES = int(sys.argv[3]) if len(sys.argv) > 3 else 100
W, S, PUSH = 400, 160, 1600
LEN = PUSH * PUSHES
dev = torch.device("cuda:0")


def handle(limit):
    m = pkg.MfccHip(limit, W, S, 40, 16000.0, 64.0, 8000.0, 13, False, 22.0, pkg.NORM_NONE, pkg.DYN_ACC, 3, 3, True, engine=ENGINE)
    m.set_window(pkg.reference_window(W))
    m.set_stream(torch.cuda.current_stream().cuda_stream)   # the events below are torch's: they must be on the handle's stream
    return m


rng = np.random.default_rng(0)
pcm = (3000 * rng.standard_normal(N * LEN)).astype(np.int16)
d_pcm = torch.from_numpy(pcm).to(dev)
res = dict(n_sessions=N, pushes=PUSHES, push_samples=PUSH, engine=ENGINE)

# ---- the session entries
m = handle(LEN)
T = m.batch_frames(LEN)
width = m.get_output_data_width()
m.sessions_create(N, PUSH)
d_out = torch.empty((N * (PUSH // S + 8), width), dtype=torch.float32, device=dev)
ids = np.arange(N, dtype=np.int32)
base = np.arange(N, dtype=np.int64) * LEN
lens = np.full(N, PUSH, np.int64)
for rep in range(2):                                          # (the first pass warms everything up)
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(PUSHES)]
    host, rows = 0.0, 0
    torch.cuda.synchronize()
    t00 = time.perf_counter()
    for k in range(PUSHES):
        fin = np.full(N, int(k == PUSHES - 1), np.int32)
        t0 = time.perf_counter()
        _, _, total = m.sessions_plan(ids, base + k * PUSH, lens, fin)
        ev[k][0].record()
        m.sessions_run_device(d_pcm.data_ptr(), N * LEN, d_out.data_ptr())
        ev[k][1].record()
        host += time.perf_counter() - t0
        rows += total
    torch.cuda.synchronize()
    wall = time.perf_counter() - t00
    dev_us = sorted(1e3 * a.elapsed_time(b) for a, b in ev)
assert rows == N * T, (rows, N * T)
res["sessions"] = dict(device_us_per_push_median=dev_us[len(dev_us) // 2], device_us_per_push_min=dev_us[0],
                       host_us_per_push_plan_and_run=1e6 * host / PUSHES, frames_per_s_whole_run=rows / wall,
                       frames_per_s_device_time=rows / (1e-6 * sum(dev_us)))
m.close()

# ---- comparator 1: one streaming handle, the same utterances one call sequence each (tools/stream_small_bench.py)
m = handle(LEN + S)                                           # (a handle's block limit is rounded down to whole frames)
L, hnd = m._L, m._h
out = np.zeros((T + 64) * width, np.float32)
op = C.cast(out.ctypes.data, C.POINTER(C.c_float))
nfr = C.c_int32()
for rep in range(2):
    frames = 0
    t00 = time.perf_counter()
    for u in range(N):
        ip = C.cast(pcm[u * LEN:(u + 1) * LEN].ctypes.data, C.POINTER(C.c_short))
        L.mfx_set_input(hnd, ip, LEN, C.byref(nfr))
        L.mfx_apply(hnd)
        L.mfx_get_output_data(hnd, op, nfr.value)
        frames += nfr.value
        L.mfx_flush(hnd, C.byref(nfr))
        L.mfx_apply(hnd)
        L.mfx_get_output_data(hnd, op, nfr.value)
        frames += nfr.value
    wall = time.perf_counter() - t00
assert frames == N * T, (frames, N * T)
res["streaming_one_handle"] = dict(frames_per_s=frames / wall, us_per_utterance=1e6 * wall / N)
m.close()

# ---- comparator 2, the ceiling: the complete utterances as one batch run, three times
m = handle(LEN)
_, total = m.batch_plan(base, np.full(N, LEN, np.int64))
d_all = torch.empty((total, width), dtype=torch.float32, device=dev)
ms = []
for rep in range(4):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    m.batch_run_device(d_pcm.data_ptr(), N * LEN, d_all.data_ptr())
    b.record()
    torch.cuda.synchronize()
    if rep:
        ms.append(a.elapsed_time(b))
res["batch_ceiling"] = dict(ms=ms, frames_per_s=[total / (1e-3 * x) for x in ms])
m.close()
print(json.dumps(res))
