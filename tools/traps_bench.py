"""TRAPS on 1000 x 10 s at 16 kHz (25/10 ms): device time of mfx_batch_run_device around HIP events, after warm-up, for
the shapes (num_banks, traps_len, traps_dct_len) = (15, 31, 10) and (23, 31, 10), without and with delta + delta-delta --
  traps       the fused fbank front end -> k_traps on the matrix pipe (-> k_delta)
  traps_valu  the same with k_traps on the vector ALUs (MFX_ENGINE_TRAPS_VALU)
  fbank       the fbank handle of the same shape (ceps_len = 0) in the same process: the floor TRAPS stands on
Prints one JSON line.  Per-kernel times come from a separate
`rocprofv3 --kernel-trace --stats -- python tools/traps_bench.py --reps 3`; k_traps moves 4 M bytes in and 4 M K bytes out
per frame, printed as k_traps_bytes_per_step for the rate.
usage: python tools/traps_bench.py [--utts 1000] [--seconds 10] [--reps 10] [--warmup 3] [--only traps|traps_valu|fbank]
                                   [--shape M,L,K] [--dyn 0|2]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=1000)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", default="")
    ap.add_argument("--shape", default="")
    ap.add_argument("--dyn", type=int, default=-1)
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
    shapes = [tuple(int(v) for v in a.shape.split(","))] if a.shape else [(15, 31, 10), (23, 31, 10)]
    dyns = [a.dyn] if a.dyn >= 0 else [0, 2]
    res = {"workload": "%d x %g s, 16 kHz" % (a.utts, a.seconds), "runs": []}
    for (M, L, K) in shapes:
        for dyn in dyns:
            variants = [("traps", dict(method=pkg.METHOD_TRAPS, traps_len=L, traps_dct_len=K)),
                        ("traps_valu", dict(method=pkg.METHOD_TRAPS, traps_len=L, traps_dct_len=K, engine=512)),
                        ("fbank", dict())]
            for name, kw in variants:
                if a.only and name != a.only:
                    continue
                m = pkg.MfccHip(n + 1000, W, S, M, float(sr), 64.0, 8000.0, 0, False, 22.0, pkg.NORM_NONE, dyn, 3, 3, True,
                                device=0, **kw)
                m.set_window(pkg.reference_window(W))
                rows, total = m.batch_plan(offs, lens)
                out = torch.empty((total, m.get_output_data_width()), dtype=torch.float32, device="cuda:0")
                m.set_stream(torch.cuda.current_stream().cuda_stream)
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
                med = float(np.median(ms))
                r = {"variant": name, "M": M, "L": L, "K": K, "dyn": dyn, "kernel": m.dominant_kernel_name(),
                     "width": m.get_output_data_width(), "ms_median": round(med, 4), "ms_min": round(min(ms), 4),
                     "frames": int(total), "frames_per_s": round(total / (med * 1e-3), 1),
                     "finite": bool(torch.isfinite(out).all().item())}
                if name != "fbank":
                    r["k_traps_bytes_per_step"] = int(total) * 4 * M * (1 + K)
                res["runs"].append(r)
                m.close()
                del out
    print(json.dumps(res))


if __name__ == "__main__":
    main()
