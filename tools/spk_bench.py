"""Per-speaker normalisation on the C2 workload (1000 x 10 s, 16 kHz, 25/10 ms, 40 mel, 13 cepstra + d + dd, CVN after the
deltas): what a batch run with a speaker list (mfx_batch_set_speakers: k_spk_sums + k_spk_finish + k_spk_apply) costs against
the per-utterance normaliser it replaces (k_norm_seg: one read and one write of the rows) --
  P  no list: every utterance's own statistics, the kernels the batch entries ran before the feature (the comparator)
  1  100 speakers x 10 utterances, dealt round-robin (a speaker's utterances lie 100 apart)
  2  one speaker per utterance
  0  norm = NONE: the run without any normaliser (what the stage costs at all)
All are device times of mfx_batch_run_device between HIP events, after warm-up; P is measured twice more at the end (P2, P3):
the spread of its medians is the margin 1 and 2 are read against.  Prints one JSON line with the step times and the ratios
to P.  Per-kernel times come from a separate `rocprofv3 --kernel-trace --stats -- python tools/spk_bench.py --only 1`.
usage: python tools/spk_bench.py [--utts 1000] [--seconds 10] [--speakers 100] [--reps 10] [--warmup 3] [--only P|1|2|0]"""
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
    ap.add_argument("--speakers", type=int, default=100)
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

    def make(norm):
        m = pkg.MfccHip(n + 1000, W, S, 40, float(sr), 64.0, 8000.0, 13, False, 22.0, norm, pkg.DYN_ACC, 3, 3, True, device=0)
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

    res = {"workload": "C2 %d x %g s, 13 MFCC + d + dd, CVN after dyn" % (a.utts, a.seconds)}
    want = lambda k: not a.only or a.only == k
    out = None
    cases = (("P", pkg.NORM_CVN, None), ("1", pkg.NORM_CVN, np.arange(a.utts) % a.speakers), ("2", pkg.NORM_CVN, np.arange(a.utts)),
             ("0", pkg.NORM_NONE, None), ("P2", pkg.NORM_CVN, None), ("P3", pkg.NORM_CVN, None))
    for name, norm, ids in cases:
        if not want(name[0]):
            continue
        m = make(norm)
        rows, total = m.batch_plan(offs, lens)
        if out is None:
            out = torch.empty((total, m.get_output_data_width()), dtype=torch.float32, device="cuda:0")
        if ids is not None:
            m.batch_set_speakers(ids, int(ids.max()) + 1)
        ms = device_time(m, out)
        med = float(np.median(ms))
        res[name] = {"ms_median": round(med, 4), "ms_min": round(min(ms), 4), "frames": int(total),
                     "frames_per_s": round(total / (med * 1e-3), 1), "finite": bool(torch.isfinite(out).all().item())}
        if ids is not None:
            res[name]["speakers"] = int(ids.max()) + 1
        m.close()
    if "P" in res:
        for k in ("1", "2"):
            if k in res:
                res[k]["ratio_to_P"] = round(res[k]["ms_median"] / res["P"]["ms_median"], 4)
        if "0" in res:   # the normalising stage alone: the difference to the run without one
            base = res["0"]["ms_median"]
            for k in ("P", "1", "2"):
                if k in res:
                    res[k]["stage_ms"] = round(res[k]["ms_median"] - base, 4)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
