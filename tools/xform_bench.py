"""Splice + affine transform on C2 (1000 x 10 s at 16 kHz, 25/10 ms, 40 mel, 13 MFCC + d + dd; left = right = 4,
out_dim 40: 351 -> 40): device time of mfx_batch_run_device around HIP events, after warm-up, in one process --
  xform       the handle with one transform in force (k_splice_affine on the matrix pipe as the last launch)
  floor       the SAME handle with the transform cleared, three times: the spread of its medians is the margin
  xform_valu  a handle with MFX_ENGINE_XFORM_VALU (the vector form)
  xform16     with --xf 16: sixteen transforms dealt round-robin over the utterances
Prints one JSON line.  The kernel's own time comes from a separate
`rocprofv3 --kernel-trace --stats -- python tools/xform_bench.py --reps 3`; its flop (2 in_dim out_dim per row) and bytes
(4 Wd read + 4 out_dim written per row) per step are printed for the rates.
usage: python tools/xform_bench.py [--utts 1000] [--seconds 10] [--reps 10] [--warmup 3] [--xf 0|16] [--left 4] [--right 4]
                                   [--out-dim 40]"""
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
    ap.add_argument("--xf", type=int, default=0)
    ap.add_argument("--left", type=int, default=4)
    ap.add_argument("--right", type=int, default=4)
    ap.add_argument("--out-dim", type=int, default=40)
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
    rng = np.random.default_rng(1)

    def handle(engine=0):
        m = pkg.MfccHip(n + 1000, W, S, 40, float(sr), 64.0, 8000.0, 13, False, 22.0, pkg.NORM_NONE, pkg.DYN_ACC, 3, 3, True,
                        device=0, engine=engine)
        m.set_window(pkg.reference_window(W))
        m.batch_plan(offs, lens)
        m.set_stream(torch.cuda.current_stream().cuda_stream)
        return m

    def timed(m, total):
        out = torch.empty((total, m.batch_output_width()), dtype=torch.float32, device="cuda:0")
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
        return {"width": m.batch_output_width(), "ms_median": round(float(np.median(ms)), 4), "ms_min": round(min(ms), 4),
                "finite": bool(torch.isfinite(out).all().item())}

    m = handle()
    total = int(m._plan_total)
    wd = m.get_output_data_width()
    in_dim = (a.left + a.right + 1) * wd
    n_xf = max(a.xf, 1)
    A = (rng.standard_normal((n_xf, a.out_dim, in_dim)) / np.sqrt(in_dim)).astype(np.float32)
    b = rng.standard_normal((n_xf, a.out_dim)).astype(np.float32)
    res = {"workload": "%d x %g s, 16 kHz, 13 MFCC + d + dd, %d -> %d" % (a.utts, a.seconds, in_dim, a.out_dim),
           "frames": total, "kernel": m.dominant_kernel_name(),
           "xform_flop_per_step": 2 * in_dim * a.out_dim * total, "xform_bytes_per_step": 4 * (wd + a.out_dim) * total, "runs": []}
    m.batch_set_transform(A[0], b[0], left=a.left, right=a.right)
    res["runs"].append(dict(variant="xform", **timed(m, total)))
    if a.xf > 1:
        m.batch_set_transform(A, b, left=a.left, right=a.right, utt_xf=np.arange(a.utts, dtype=np.int32) % a.xf)
        res["runs"].append(dict(variant="xform%d" % a.xf, **timed(m, total)))
    m.batch_set_transform(None)
    for i in range(3):
        res["runs"].append(dict(variant="floor", **timed(m, total)))
    m.close()
    v = handle(engine=pkg.mfcc.ENGINE_XFORM_VALU)
    v.batch_set_transform(A[0], b[0], left=a.left, right=a.right)
    res["runs"].append(dict(variant="xform_valu", **timed(v, total)))
    v.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
