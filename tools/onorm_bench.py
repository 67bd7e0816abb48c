"""Online CMN on the C2 workload (1000 x 10 s, 16 kHz, 25/10 ms, 40 mel, 13 cepstra + c0 + d + dd, CMN after the deltas,
window N = 608 frames): what a batch run with the online attachment (mfx_batch_set_online_norm: k_onorm_totals +
k_onorm_offsets + k_onorm_apply, and a scratch in front of them) costs against the per-utterance normaliser it replaces --
  P  per-utterance CMN: the kernels the batch entries ran before the feature (the comparator)
  O  the online attachment, N = 608
  0  norm = NONE: the run without any normaliser
  H  ONE stream of --hour-seconds (3600): the offsets chain at its longest, P beside O
  S  --sessions (1000) sessions at 100 ms pushes through the session entries, with the normaliser and on a norm = NONE handle
P, O, 0 and H are device times of mfx_batch_run_device between HIP events, after warm-up; P is measured twice more at the end
(P2, P3): the spread of its medians is the margin O is read against.  S is the wall time of a push (plan + run + synchronise).
Prints one JSON line.  Per-kernel times come from a separate `rocprofv3 --kernel-trace --stats -- python tools/onorm_bench.py
--only O`.
usage: python tools/onorm_bench.py [--utts 1000] [--seconds 10] [--window 608] [--reps 10] [--warmup 3] [--only P|O|0|H|S]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=1000)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--window", type=int, default=608)
    ap.add_argument("--hour-seconds", type=float, default=3600.0)
    ap.add_argument("--sessions", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", default="")
    a = ap.parse_args()

    import numpy as np
    import torch
    import __graft_entry__ as G
    import bench
    pkg = G.load_package()
    sr, W, S = 16000, 400, 160
    CMN = pkg.NORM_CMN

    def make(norm, ibs):
        m = pkg.MfccHip(ibs, W, S, 40, float(sr), 64.0, 8000.0, 13, True, 22.0, norm, pkg.DYN_ACC, 3, 3, True, device=0)
        m.set_window(pkg.reference_window(W))
        m.set_stream(torch.cuda.current_stream().cuda_stream)
        return m

    def device_time(m, pcm, out):
        for _ in range(a.warmup):
            m.batch_run_device(pcm.data_ptr(), pcm.numel(), out.data_ptr())
        torch.cuda.synchronize()
        ms = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            m.batch_run_device(pcm.data_ptr(), pcm.numel(), out.data_ptr())
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1))
        return float(np.median(ms))

    def batch(norm, online, n_utt, n):
        pcm = bench.synth_pcm_torch(torch, n_utt, n, float(sr), 0, "cuda:0").reshape(-1).contiguous()
        m = make(norm, min(n, 1 << 24) + 1000)
        _, total = m.batch_plan(np.arange(n_utt, dtype=np.int64) * n, np.full(n_utt, n, dtype=np.int64))
        if online:
            m.batch_set_online_norm(a.window)
        out = torch.empty((total, m.get_output_data_width()), dtype=torch.float32, device="cuda:0")
        ms = device_time(m, pcm, out)
        m.close()
        return ms

    def sessions(norm):
        n_push = sr // 10                                    # 100 ms
        m = make(norm, 16000 * 10)
        if norm != pkg.NORM_NONE:
            m.sessions_set_online_norm(a.window)
        m.sessions_create(a.sessions, n_push)
        pcm = bench.synth_pcm_torch(torch, a.sessions, n_push, float(sr), 0, "cuda:0").reshape(-1).contiguous()
        ids = np.arange(a.sessions, dtype=np.int32)
        offs = ids.astype(np.int64) * n_push
        lens = np.full(a.sessions, n_push, dtype=np.int64)
        out = torch.empty((a.sessions * 12, m.get_output_data_width()), dtype=torch.float32, device="cuda:0")
        ms = []
        for k in range(a.warmup + 8 * a.reps):               # (80 pushes: 8 s of every stream, the window is full after 6.1 s)
            t0 = time.perf_counter()
            m.sessions_plan(ids, offs, lens)
            m.sessions_run_device(pcm.data_ptr(), pcm.numel(), out.data_ptr())
            m.synchronize()
            if k >= a.warmup:
                ms.append((time.perf_counter() - t0) * 1e3)
        m.close()
        return float(np.median(ms)), float(np.median(ms[-a.reps:]))

    n = int(a.seconds * sr)
    res = {"utts": a.utts, "seconds": a.seconds, "window": a.window}
    want = a.only or "P,O,0,H,S,P2,P3"
    for key in want.split(","):
        if key in ("P", "P2", "P3"):
            res[key + "_ms"] = batch(CMN, False, a.utts, n)
        elif key == "O":
            res["O_ms"] = batch(CMN, True, a.utts, n)
        elif key == "0":
            res["none_ms"] = batch(pkg.NORM_NONE, False, a.utts, n)
        elif key == "H":
            nh = int(a.hour_seconds * sr)
            res["hour_P_ms"] = batch(CMN, False, 1, nh)
            res["hour_O_ms"] = batch(CMN, True, 1, nh)
        elif key == "S":
            res["sess_push_ms_online"], res["sess_push_ms_online_full_window"] = sessions(CMN)
            res["sess_push_ms_none"], _ = sessions(pkg.NORM_NONE)
    if "P_ms" in res and "O_ms" in res:
        res["O_over_P"] = res["O_ms"] / res["P_ms"]
    ps = [res[k] for k in ("P_ms", "P2_ms", "P3_ms") if k in res]
    if len(ps) > 1:
        res["P_spread"] = (max(ps) - min(ps)) / min(ps)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
