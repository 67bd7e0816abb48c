"""Sliding-window CMN / CVN on the C2 workload (1000 x 10 s, 16 kHz, 25/10 ms, 40 mel, 13 cepstra + c0 + d + dd): what a batch
run with the sliding attachment (mfx_batch_set_sliding_norm: k_onorm_totals + k_onorm_offsets + k_slide_apply, and a scratch in
front of them) costs, beside the other normalisers in the same process on the same box --
  0   norm = NONE: the run without any normaliser (what the attachment is added to)
  C   sliding, window 300, centred, CMN (the x-vector recipe's setting)
  V   sliding, window 300, centred, CVN
  T   sliding, window 600, not centred, min_window 100, CMN (apply-cmvn-sliding's defaults)
  P   per-utterance CMN after the deltas
  O   the online attachment at N = 608 (CMN)
  H   ONE stream of --hour-seconds (3600): 0, C and O
Device times of mfx_batch_run_device between HIP events, medians after warm-up; X_own_ms = X_ms - none_ms is the attachment's
launches' own time by events (the front end and the deltas are the same launches in both).  0 is measured twice more at the
end (02, 03): the spread of its medians is the margin the differences are read against.  Prints one JSON line.  Per-kernel times
come from a separate `rocprofv3 --kernel-trace --stats -- python tools/slide_bench.py --only C` (V, T, O).
usage: python tools/slide_bench.py [--utts 1000] [--seconds 10] [--reps 10] [--warmup 3] [--only 0,C,V,T,P,O,H]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SLIDING = {"C": (300, 0, True, False), "V": (300, 0, True, True), "T": (600, 100, False, False)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=1000)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--online-window", type=int, default=608)
    ap.add_argument("--hour-seconds", type=float, default=3600.0)
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

    def batch(key, n_utt, n):
        """key: 0 (none), P (per utterance), O (online), or one of SLIDING"""
        pcm = bench.synth_pcm_torch(torch, n_utt, n, float(sr), 0, "cuda:0").reshape(-1).contiguous()
        m = make(pkg.NORM_CMN if key in ("P", "O") else pkg.NORM_NONE, min(n, 1 << 24) + 1000)
        _, total = m.batch_plan(np.arange(n_utt, dtype=np.int64) * n, np.full(n_utt, n, dtype=np.int64))
        if key == "O":
            m.batch_set_online_norm(a.online_window)
        elif key in SLIDING:
            m.batch_set_sliding_norm(*SLIDING[key])
        out = torch.empty((total, m.get_output_data_width()), dtype=torch.float32, device="cuda:0")
        ms = device_time(m, pcm, out)
        m.close()
        return ms

    n = int(a.seconds * sr)
    res = {"utts": a.utts, "seconds": a.seconds, "online_window": a.online_window}
    want = a.only or "0,C,V,T,P,O,H,02,03"
    for key in want.split(","):
        if key in ("0", "02", "03"):
            res["none%s_ms" % key[1:]] = batch("0", a.utts, n)
        elif key in SLIDING or key in ("P", "O"):
            res[key + "_ms"] = batch(key, a.utts, n)
        elif key == "H":
            nh = int(a.hour_seconds * sr)
            for k in ("0", "C", "O"):
                res["hour_%s_ms" % ("none" if k == "0" else k)] = batch(k, 1, nh)
    if "none_ms" in res:
        for key in list(SLIDING) + ["P", "O"]:
            if key + "_ms" in res:
                res[key + "_own_ms"] = res[key + "_ms"] - res["none_ms"]
    zs = [res[k] for k in ("none_ms", "none2_ms", "none3_ms") if k in res]
    if len(zs) > 1:
        res["none_spread"] = (max(zs) - min(zs)) / min(zs)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
