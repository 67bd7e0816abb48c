"""PLP on the C2 workload (1000 x 10 s, 16 kHz, 25/10 ms, 40 mel, 13 cepstra + d + dd): device time of
mfx_batch_run_device around HIP events, after warm-up, for three versions of the same batch --
  plp        method = PLP, lpc_order = 12 (spectrum kernel + k_plp)
  mfcc_spec  MFCC on MFX_ENGINE_STREAM_KERNELS (the same spectrum kernel + k_melcep: only k_plp vs k_melcep differs)
  mfcc       the default fused MFCC front end
Prints one JSON line.  Per-kernel times come from a separate `rocprofv3 --kernel-trace --stats -- python tools/plp_bench.py`.
usage: python tools/plp_bench.py [--utts 1000] [--seconds 10] [--reps 10] [--warmup 3] [--only plp|mfcc_spec|mfcc]"""
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
    variants = [("plp", dict(method=pkg.METHOD_PLP, lpc_order=12)),
                ("mfcc_spec", dict(engine=pkg.mfcc.ENGINE_STREAM_KERNELS)),
                ("mfcc", dict())]
    res = {"workload": "C2 %d x %g s" % (a.utts, a.seconds)}
    for name, kw in variants:
        if a.only and name != a.only:
            continue
        m = pkg.MfccHip(n + 1000, W, S, 40, float(sr), 64.0, 8000.0, 13, False, 22.0, pkg.NORM_NONE, pkg.DYN_ACC, 3, 3, True,
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
        res[name] = {"kernel": m.dominant_kernel_name(), "ms_median": round(med, 4), "ms_min": round(min(ms), 4),
                     "frames": int(total), "frames_per_s": round(total / (med * 1e-3), 1),
                     "finite": bool(torch.isfinite(out).all().item())}
        m.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
