"""Sample-rate conversion in front of the C2 batch (1000 x 10 s, features at 16 kHz: 25/10 ms, 40 mel, 13 MFCC + d + dd):
device time of mfx_batch_run_device around HIP events, after warm-up, in one process -- per input rate (48, 44.1, 8 kHz)
  resample    the handle under mfx_batch_plan_rates: k_resample, then the front end on the converted PCM
  floor       the SAME handle planned plainly on the already converted PCM, three times: the spread of its medians is
              the margin
Prints one JSON line.  The kernel's own time comes from a separate
`rocprofv3 --kernel-trace --stats -- python tools/resample_bench.py --reps 3`; its flop (2 P per output sample) and bytes
(2 per input sample + 2 per output sample) per step are printed for the rates.
usage: python tools/resample_bench.py [--utts 1000] [--seconds 10] [--reps 10] [--warmup 3] [--rates 48000,44100,8000]"""
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
    ap.add_argument("--rates", default="48000,44100,8000")
    a = ap.parse_args()

    import numpy as np
    import torch
    import __graft_entry__ as G
    import bench
    pkg = G.load_package()
    sr, W, S = 16000, 400, 160

    def timed(m, pcm, total):
        out = torch.empty((max(total, 1), m.batch_output_width()), dtype=torch.float32, device="cuda:0")
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
        return {"ms_median": round(float(np.median(ms)), 4), "ms_min": round(min(ms), 4),
                "finite": bool(torch.isfinite(out).all().item())}

    res = {"workload": "%d x %g s -> 16 kHz, 13 MFCC + d + dd" % (a.utts, a.seconds), "runs": []}
    for r_in in [int(v) for v in a.rates.split(",")]:
        n = int(a.seconds * r_in)
        pcm = bench.synth_pcm_torch(torch, a.utts, n, float(r_in), 0, "cuda:0").reshape(-1).contiguous()
        offs = np.arange(a.utts, dtype=np.int64) * n
        lens = np.full(a.utts, n, dtype=np.int64)
        m = pkg.MfccHip(int(a.seconds * sr) + 1000, W, S, 40, float(sr), 64.0, 8000.0, 13, False, 22.0, pkg.NORM_NONE, pkg.DYN_ACC,
                        3, 3, True, device=0)
        m.set_window(pkg.reference_window(W))
        m.set_stream(torch.cuda.current_stream().cuda_stream)
        rows, total = m.batch_plan_rates(offs, lens, np.full(a.utts, r_in, np.int32))
        taps, L, M, P = pkg.mfcc.host_resample_taps(r_in, sr)
        off, ln, sc_total = m.batch_resample_layout()
        n_out = int(ln.sum())
        res["runs"].append(dict(variant="resample", rate=r_in, L=L, M=M, P=P, frames=total, kernel=m.dominant_kernel_name(),
                                resample_flop_per_step=2 * P * n_out, resample_bytes_per_step=2 * a.utts * n + 2 * n_out,
                                **timed(m, pcm, total)))
        y = torch.from_numpy(np.concatenate([m.debug_read(8), np.zeros(8, np.int16)])).to("cuda:0")
        m.batch_plan(off, ln)
        for _ in range(3):
            res["runs"].append(dict(variant="floor", rate=r_in, **timed(m, y, total)))
        m.close()
        del pcm, y
    print(json.dumps(res))


if __name__ == "__main__":
    main()
