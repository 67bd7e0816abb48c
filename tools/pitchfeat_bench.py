"""Pitch features on C2 (1000 x 10 s at 16 kHz, 25/10 ms, 40 mel, 12 MFCC + c0 + d + dd = 39 columns; pitch window 400, lags
40 .. 320, max_jump 16): device time of mfx_batch_run_device around HIP events, after warm-up, in one process, on ONE handle --
  track   mfx_batch_set_pitch alone, three times: the parent's launches, the comparator; the spread of its medians is the noise
  feats   + mfx_batch_set_pitch_feats (Kaldi's defaults), paste = 0: k_pitch_feats behind k_pitch_track
  paste   + paste = 1: k_pitch_paste on the tail's stream, rows of width + 3 floats
  xform   + a splice + affine transform over 9 wide rows -> 40 (mfx_batch_set_transform, left = right = 4; the C2 rows are 39
          wide, so the wide rows are 42 and in_dim is 378)
The PCM is bench.py's synthetic batch.  Prints one JSON line.  Each kernel's own time comes from a separate
`rocprofv3 --kernel-trace --stats -- python tools/pitchfeat_bench.py --reps 3`.
usage: python tools/pitchfeat_bench.py [--utts 1000] [--seconds 10] [--reps 10] [--warmup 3] [--lag-min 40] [--lag-max 320]"""
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
    m = pkg.MfccHip(200000, W, S, 40, float(sr), 64.0, 8000.0, 12, True, 22.0, pkg.NORM_NONE, pkg.DYN_ACC, 3, 3, True, device=0)
    m.set_window(pkg.reference_window(W))
    m.batch_plan(offs, lens)
    m.set_stream(torch.cuda.current_stream().cuda_stream)
    total, Wd = int(m._plan_total), m.get_output_data_width()
    out = torch.empty((total, Wd + 3), dtype=torch.float32, device="cuda:0")     # (wide enough for every variant)

    def timed(variant):
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
        return {"variant": variant, "width": m.batch_output_width(), "ms_median": round(float(np.median(ms)), 4), "ms_min": round(min(ms), 4)}

    m.batch_set_pitch(a.lag_min, a.lag_max, window=W, ballast=0.0, lag_cost=0.1, penalty=1.0, max_jump=16)
    runs = [timed("track") for _ in range(3)]
    floor = float(np.median([r["ms_median"] for r in runs]))
    m.batch_set_pitch_feats()
    runs.append(timed("feats"))
    feats = m.batch_pitch_feats_read()
    m.batch_set_pitch_feats(paste=True)
    runs.append(timed("paste"))
    rng = np.random.default_rng(1)
    A = (rng.standard_normal((40, 9 * (Wd + 3))) / 20.0).astype(np.float32)
    m.batch_set_transform(A, None, left=4, right=4)
    runs.append(timed("xform"))
    for r in runs[3:]:
        r["minus_track_ms"] = round(r["ms_median"] - floor, 4)
    m.batch_set_transform(None)
    m.close()
    print(json.dumps({"workload": "16 kHz, 12 MFCC + c0 + d + dd; pitch window %d, lags %d .. %d, max_jump 16; pitch features: Kaldi's "
                                  "defaults" % (W, a.lag_min, a.lag_max),
                      "utts": a.utts, "seconds": a.seconds, "frames": total, "feats_finite": bool(np.isfinite(feats).all()),
                      "setter_bytes": total * 4 * (3 + Wd), "runs": runs}))


if __name__ == "__main__":
    main()
