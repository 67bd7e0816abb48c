"""Energy VAD + voiced-frame selection on C2 (1000 x 10 s at 16 kHz, 25/10 ms, 40 mel, 12 MFCC + c0 + d + dd; decision on c0,
frames_context 2, proportion 0.6): device time of mfx_batch_run_device around HIP events, after warm-up, in one process --
  floor   the handle without a VAD, three times: the spread of its medians is the noise
  flags   MFX_VAD_FLAGS  (threshold, flags, counts; d_out untouched)
  select  MFX_VAD_SELECT (rows built in the scratch, voiced rows moved to the front of every utterance's range)
  pack    MFX_VAD_PACK   (voiced rows of the batch back to back)
The PCM is bench.py's synthetic batch under a gain envelope (runs of 50 frames at gain 1 or 1/256), so that about half of
the rows are voiced.  Prints one JSON line with the bytes the stage moves per step: 4 per row read twice for the decision
(sum, flags), one byte per row of flags, and for SELECT / PACK 4 Wo per voiced row read and 4 Wo per row written.
Each kernel's own time comes from a separate `rocprofv3 --kernel-trace --stats -- python tools/vad_bench.py --reps 3`.
usage: python tools/vad_bench.py [--utts 1000] [--seconds 10] [--reps 10] [--warmup 3] [--ctx 2] [--prop 0.6]"""
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
    ap.add_argument("--ctx", type=int, default=2)
    ap.add_argument("--prop", type=float, default=0.6)
    a = ap.parse_args()

    import numpy as np
    import torch
    import __graft_entry__ as G
    import bench
    pkg = G.load_package()
    sr, W, S = 16000, 400, 160
    n = int(a.seconds * sr)
    pcm = bench.synth_pcm_torch(torch, a.utts, n, float(sr), 0, "cuda:0").reshape(a.utts, n)
    g = torch.Generator(device="cpu").manual_seed(7)
    runs = (n + 50 * S - 1) // (50 * S)
    loud = (torch.rand((a.utts, runs), generator=g) < 0.5).to("cuda:0")
    gain = torch.where(loud, 1.0, 1.0 / 256.0).repeat_interleave(50 * S, dim=1)[:, :n]
    pcm = (pcm.to(torch.float32) * gain).round().to(torch.int16).reshape(-1).contiguous()
    offs = np.arange(a.utts, dtype=np.int64) * n
    lens = np.full(a.utts, n, dtype=np.int64)

    m = pkg.MfccHip(n + 1000, W, S, 40, float(sr), 64.0, 8000.0, 12, True, 22.0, pkg.NORM_NONE, pkg.DYN_ACC, 3, 3, True, device=0)
    m.set_window(pkg.reference_window(W))
    m.batch_plan(offs, lens)
    m.set_stream(torch.cuda.current_stream().cuda_stream)
    total = int(m._plan_total)
    wo = m.batch_output_width()
    out = torch.empty((total, wo), dtype=torch.float32, device="cuda:0")

    def timed():
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
        return {"ms_median": round(float(np.median(ms)), 4), "ms_min": round(min(ms), 4), "finite": bool(torch.isfinite(out).all().item())}

    res = {"workload": "%d x %g s, 16 kHz, 12 MFCC + c0 + d + dd, ctx %d, p %g" % (a.utts, a.seconds, a.ctx, a.prop),
           "frames": total, "width": wo, "kernel": m.dominant_kernel_name(), "runs": []}
    for i in range(3):
        res["runs"].append(dict(variant="floor", **timed()))
    for name, mode in (("flags", pkg.VAD_FLAGS), ("select", pkg.VAD_SELECT), ("pack", pkg.VAD_PACK)):
        m.batch_set_vad(-1, 0.0, 1.0, a.ctx, a.prop, mode)
        r = timed()
        voiced = int(m.batch_vad_read()[3])
        r["voiced"] = voiced
        r["vad_bytes_per_step"] = 9 * total + (0 if mode == pkg.VAD_FLAGS else 4 * wo * (voiced + total))
        res["runs"].append(dict(variant=name, **r))
    m.batch_clear_vad()
    m.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
