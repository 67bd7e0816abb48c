"""Pitch track on C2 (1000 x 10 s at 16 kHz, 25/10 ms, 40 mel, 12 MFCC + c0 + d + dd; window 400, lags 40 .. 320, max_jump
16): device time of mfx_batch_run_device around HIP events, after warm-up, in one process, on ONE handle --
  floor   the handle without the track, three times: the spread of its medians is the noise
  pitch   the same handle with mfx_batch_set_pitch in force (k_pitch_nccf and k_pitch_track follow the front end on the
          handle's stream, so the difference to the floor is the two kernels' time)
  stream  one utterance of --stream-seconds (an hour), floor and pitch: k_pitch_track is ONE block there, its frames in sequence
The PCM is bench.py's synthetic batch.  Prints one JSON line, with the FMAs of the correlation per step and the bytes the setter
allocated.  Each kernel's own time comes from a separate
`rocprofv3 --kernel-trace --stats -- python tools/pitch_bench.py --reps 3 --stream-seconds 0`.
usage: python tools/pitch_bench.py [--utts 1000] [--seconds 10] [--reps 10] [--warmup 3] [--lag-min 40] [--lag-max 320]
                                   [--max-jump 16] [--stream-seconds 3600]"""
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
    ap.add_argument("--lag-min", type=int, default=40)
    ap.add_argument("--lag-max", type=int, default=320)
    ap.add_argument("--max-jump", type=int, default=16)
    ap.add_argument("--stream-seconds", type=float, default=3600.0)
    a = ap.parse_args()

    import numpy as np
    import torch
    import __graft_entry__ as G
    import bench
    pkg = G.load_package()
    sr, W, S = 16000, 400, 160
    K = a.lag_max - a.lag_min + 1

    def measure(utts, n, reps, warmup):
        pcm = bench.synth_pcm_torch(torch, utts, n, float(sr), 0, "cuda:0").reshape(-1).contiguous()
        offs = np.arange(utts, dtype=np.int64) * n
        lens = np.full(utts, n, dtype=np.int64)
        m = pkg.MfccHip(200000, W, S, 40, float(sr), 64.0, 8000.0, 12, True, 22.0, pkg.NORM_NONE, pkg.DYN_ACC, 3, 3, True, device=0)
        m.set_window(pkg.reference_window(W))
        m.batch_plan(offs, lens)
        m.set_stream(torch.cuda.current_stream().cuda_stream)
        total = int(m._plan_total)
        out = torch.empty((total, m.batch_output_width()), dtype=torch.float32, device="cuda:0")

        def timed():
            for _ in range(warmup):
                m.batch_run_device(pcm.data_ptr(), pcm.numel(), out.data_ptr())
            torch.cuda.synchronize()
            ms = []
            for _ in range(reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                m.batch_run_device(pcm.data_ptr(), pcm.numel(), out.data_ptr())
                e1.record()
                torch.cuda.synchronize()
                ms.append(e0.elapsed_time(e1))
            return {"ms_median": round(float(np.median(ms)), 4), "ms_min": round(min(ms), 4)}

        runs = [dict(variant="floor", **timed()) for _ in range(3)]
        m.batch_set_pitch(a.lag_min, a.lag_max, window=W, ballast=0.0, lag_cost=0.1, penalty=1.0, max_jump=a.max_jump)
        r = timed()
        lag, rho, index = m.batch_pitch_read()
        r["finite"] = bool(np.isfinite(lag).all() and np.isfinite(rho).all())
        r["pitch_minus_floor_ms"] = round(r["ms_median"] - float(np.median([x["ms_median"] for x in runs])), 4)
        runs.append(dict(variant="pitch", **r))
        m.batch_clear_pitch()
        m.close()
        return {"utts": utts, "seconds": n / sr, "frames": total, "correlation_fmas": total * K * W,
                "setter_bytes": total * (6 * K + 12), "runs": runs}

    res = {"workload": "16 kHz, 12 MFCC + c0 + d + dd; pitch window %d, lags %d .. %d, max_jump %d" % (W, a.lag_min, a.lag_max, a.max_jump),
           "batch": measure(a.utts, int(a.seconds * sr), a.reps, a.warmup)}
    if a.stream_seconds > 0:
        res["stream"] = measure(1, int(a.stream_seconds * sr), max(a.reps // 3, 2), 1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
