"""Per-utterance VTLN on the C2 workload (1000 x 10 s, 16 kHz, 25/10 ms, 40 mel, 13 cepstra + d + dd): what one batch with
a warp factor per utterance (mfx_batch_set_alphas) costs against the ways to get the same rows without it --
  A  one factor for all, MFX_ENGINE_STREAM_KERNELS: the same kernels without run lists (spectrum kernel + k_melcep)
  B  the per-utterance list, 21 distinct factors (0.80 .. 1.20 in steps of 0.02) dealt round-robin
  C  the same 21 factors sorted, equal ones neighbours (one run per table)
  D  what a caller does without the list: 21 plans + runs of ~utts / 21 utterances each, one factor each, on the default
     fused kernels, timed end to end on the host (mfx_batch_plan and mfx_set_alpha included, one synchronise at the end)
A, B and C are device times of mfx_batch_run_device between HIP events, after warm-up; A is measured twice more at the
end (A2, A3): the spread of its medians is the margin B and C are read against.  --method plp | traps repeats A and B (and
C, D) for PLP (p = 12) and TRAPS (15 mel, L = 31, K = 10).  Prints one JSON line.  Per-kernel times (k_melcep_runs,
k_plp_runs, the spectrum kernel) come from a separate `rocprofv3 --kernel-trace --stats -- python tools/vtln_batch_bench.py
--only B`.
usage: python tools/vtln_batch_bench.py [--method mfcc|plp|traps] [--utts 1000] [--seconds 10] [--reps 10] [--warmup 3]
                                        [--only A|B|C|D]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--method", default="mfcc", choices=["mfcc", "plp", "traps"])
    ap.add_argument("--utts", type=int, default=1000)
    ap.add_argument("--seconds", type=float, default=10.0)
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
    n = int(a.seconds * sr)
    pcm = bench.synth_pcm_torch(torch, a.utts, n, float(sr), 0, "cuda:0").reshape(-1).contiguous()
    offs = np.arange(a.utts, dtype=np.int64) * n
    lens = np.full(a.utts, n, dtype=np.int64)
    grid = (np.float32(0.80) + np.float32(0.02) * np.arange(21, dtype=np.float32)).astype(np.float32)
    round_robin = grid[np.arange(a.utts) % 21]
    shape = {"mfcc": dict(nb=40, nc=13), "plp": dict(nb=40, nc=13, method=pkg.METHOD_PLP, lpc_order=12),
             "traps": dict(nb=15, nc=0, method=pkg.METHOD_TRAPS, traps_len=31, traps_dct_len=10)}[a.method]

    def make(engine=0):
        kw = dict(shape)
        m = pkg.MfccHip(n + 1000, W, S, kw.pop("nb"), float(sr), 64.0, 8000.0, kw.pop("nc"), False, 22.0, pkg.NORM_NONE,
                        pkg.DYN_ACC, 3, 3, True, device=0, engine=engine, **kw)
        m.set_window(pkg.reference_window(W))
        m.set_stream(torch.cuda.current_stream().cuda_stream)
        return m

    def device_time(m, out):
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
        return ms

    def report(m, ms, total, out):
        med = float(np.median(ms))
        return {"kernel": m.dominant_kernel_name(), "ms_median": round(med, 4), "ms_min": round(min(ms), 4),
                "frames": int(total), "frames_per_s": round(total / (med * 1e-3), 1),
                "finite": bool(torch.isfinite(out).all().item())}

    res = {"workload": "C2 %d x %g s, %s" % (a.utts, a.seconds, a.method), "distinct_factors": 21}
    want = lambda k: not a.only or a.only == k
    out = None
    for name, alphas in (("A", None), ("B", round_robin), ("C", np.sort(round_robin)), ("A2", None), ("A3", None)):
        if not want(name[0]):
            continue
        m = make(engine=pkg.mfcc.ENGINE_STREAM_KERNELS)
        rows, total = m.batch_plan(offs, lens)
        if out is None:
            out = torch.empty((total, m.get_output_data_width()), dtype=torch.float32, device="cuda:0")
        if alphas is not None:
            m.batch_set_alphas(alphas)
        res[name] = report(m, device_time(m, out), total, out)
        m.close()
    if want("D"):
        # utterances of one factor are every 21st: the caller regroups them into one contiguous PCM array per factor first
        # (not timed); plan + set_alpha + run per factor are
        m = make()
        groups = []
        for k in range(21):
            idx = np.arange(k, a.utts, 21)
            if idx.size == 0:
                continue
            piece = pcm.reshape(a.utts, n)[torch.from_numpy(idx).to(pcm.device)].reshape(-1).contiguous()
            groups.append((float(grid[k]), piece, np.arange(idx.size, dtype=np.int64) * n, np.full(idx.size, n, dtype=np.int64)))
        width = m.get_output_data_width()
        outs = [torch.empty((m.batch_frames(n) * g[2].size, width), dtype=torch.float32, device="cuda:0") for g in groups]
        ms = []
        for rep in range(a.warmup + a.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for (alpha, piece, o_, l_), dst in zip(groups, outs):
                m.batch_plan(o_, l_)
                m.set_alpha(alpha)
                m.batch_run_device(piece.data_ptr(), piece.numel(), dst.data_ptr())
            torch.cuda.synchronize()
            if rep >= a.warmup:
                ms.append((time.perf_counter() - t0) * 1e3)
        total = sum(o.shape[0] for o in outs)
        res["D"] = report(m, ms, total, torch.cat([o[:1] for o in outs]))
        res["D"]["batches"] = len(groups)
        m.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
