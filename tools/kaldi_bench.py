"""Kaldi front end (MFX_METHOD_KALDI) on 1000 x 10 s at 16 kHz, fbank-80 (W = 400, S = 160, Povey window, Kaldi's default
options): device time of mfx_batch_run_device around HIP events on torch's stream, after warm-up, median of --reps.  Beside it,
in the same process and on the same device, the yardstick: the MFCC method's fbank-80 row of the README (k_front512, the
reference's definition: no DC removal, no pre-emphasis), timed the same way -- that kernel is hand-tuned and does less per
frame; there is no pass threshold.
Prints one JSON line.  The kernel's share comes from a separate
`rocprofv3 --kernel-trace --stats -- python tools/kaldi_bench.py --reps 3 --no-yardstick`.
--flags: kaldi_flags of mfx_create_kaldi (1 snip_edges = false, 2 the energy column, 4 windowed energy, 8 HTK order): k_kaldi_front_opts.
usage: python tools/kaldi_bench.py [--utts 1000] [--seconds 10] [--reps 10] [--warmup 3] [--banks 80] [--ceps 0] [--flags 0]
       [--no-yardstick]"""
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
    ap.add_argument("--banks", type=int, default=80)
    ap.add_argument("--ceps", type=int, default=0)
    ap.add_argument("--flags", type=int, default=0)
    ap.add_argument("--no-yardstick", action="store_true")
    a = ap.parse_args()

    import numpy as np
    import torch
    import __graft_entry__ as G
    import bench
    pkg = G.load_package()
    sr, W, S, M, C = 16000, 400, 160, a.banks, a.ceps
    n = int(a.seconds * sr)
    pcm = bench.synth_pcm_torch(torch, a.utts, n, float(sr), 0, "cuda:0").reshape(-1).contiguous()
    offs = np.arange(a.utts, dtype=np.int64) * n
    lens = np.full(a.utts, n, dtype=np.int64)

    def timed(fn):
        for _ in range(a.warmup):
            fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1))
        return float(np.median(ms)), float(min(ms))

    def run(variant, m, cols):
        rows, total = m.batch_plan(offs, lens)
        out = torch.empty((total, cols), dtype=torch.float32, device="cuda:0")
        m.set_stream(torch.cuda.current_stream().cuda_stream)
        med, best = timed(lambda: m.batch_run_device(pcm.data_ptr(), pcm.numel(), out.data_ptr()))
        m.profile_enable(True)
        for _ in range(3):
            m.batch_run_device(pcm.data_ptr(), pcm.numel(), out.data_ptr())
        launches, kms = m.profile_read()
        m.profile_enable(False)
        r = {"variant": variant, "kernel": m.dominant_kernel_name(), "ms_median": round(med, 4), "ms_min": round(best, 4),
             "kernel_ms": round(kms / max(launches, 1), 4), "frames": int(total), "frames_per_s": round(total / (med * 1e-3), 1),
             "finite": bool(torch.isfinite(out).all().item())}
        m.close()
        return r

    res = {"workload": "%d x %g s, 16 kHz, W %d, S %d, %d banks, %d cepstra, kaldi_flags %d" % (a.utts, a.seconds, W, S, M, C, a.flags),
           "runs": []}
    m = pkg.MfccHip(n + 1000, W, S, M, float(sr), 20.0, 0.0, C, False, 22.0, device=0, method=pkg.METHOD_KALDI, kaldi_flags=a.flags)
    m.set_window(pkg.povey_window(W))
    res["runs"].append(run("kaldi", m, m.get_output_data_width()))
    if not a.no_yardstick:
        m = pkg.MfccHip(n + 1000, W, S, M, float(sr), 64.0, sr / 2.0, C, False, 22.0, device=0, method=pkg.METHOD_MFCC)
        m.set_window(pkg.reference_window(W))
        res["runs"].append(run("mfcc method (yardstick)", m, C or M))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
