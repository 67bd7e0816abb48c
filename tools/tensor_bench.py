"""Dense padded tensor output on two shapes of 1000 x 10 s at 16 kHz -- C2 (25/10 ms, 40 mel, 12 MFCC + c0 + d + dd: 39 columns)
and the Whisper log-mel (N = 400, hop 160, 80 bands) -- in one process, HIP events on the handle's stream, median after warm-up:
  floor      mfx_batch_run_device without the attachment (ragged float32 rows), three times: the spread is the noise
  tm_f32     + MFX_TENSOR_TIME_MAJOR, MFX_DTYPE_F32      cm_f16 / cm_bf16    + MFX_TENSOR_CHANNEL_MAJOR, half / bfloat16
             (t_pad = 0: all utterances are equally long, so nothing is padded or cut)
  pack_*     k_tensor_pack alone on the finished rows (mfx_batch_tensor_from_rows), with the bytes it moves: 4 per element read,
             the element's size written
  torch_*    what the attachment replaces, on the same ragged rows: split by out_rows, pad_sequence, transpose, .to(dtype)
Prints one JSON line per shape.  The kernel's own time also comes from a separate
`rocprofv3 --kernel-trace --stats -- python tools/tensor_bench.py --reps 3`.
usage: python tools/tensor_bench.py [--utts 1000] [--seconds 10] [--reps 10] [--warmup 3] [--shape c2|whisper|both]"""
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
    ap.add_argument("--shape", default="both")
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
    tdt = {pkg.DTYPE_F32: torch.float32, pkg.DTYPE_F16: torch.float16, pkg.DTYPE_BF16: torch.bfloat16}
    variants = (("tm_f32", pkg.TENSOR_TIME_MAJOR, pkg.DTYPE_F32), ("cm_f16", pkg.TENSOR_CHANNEL_MAJOR, pkg.DTYPE_F16),
                ("cm_bf16", pkg.TENSOR_CHANNEL_MAJOR, pkg.DTYPE_BF16))

    def median_ms(step):
        for _ in range(a.warmup):
            step()
        torch.cuda.synchronize()
        ms = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            step()
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1))
        return {"ms_median": round(float(np.median(ms)), 4), "ms_min": round(min(ms), 4)}

    def one(shape):
        if shape == "c2":
            m = pkg.MfccHip(n + 1000, W, S, 40, float(sr), 64.0, 8000.0, 12, True, 22.0, pkg.NORM_NONE, pkg.DYN_ACC, 3, 3, True, device=0)
            m.set_window(pkg.reference_window(W))
        else:
            m = pkg.MfccHip(n + 1000, W, S, 80, float(sr), 0.0, 8000.0, 0, False, 22.0, device=0, bug_compat=False,
                            method=pkg.METHOD_STFT_LOGMEL, logmel_post=pkg.LOGMEL_WHISPER)
            m.set_window(pkg.periodic_hann(W))
        rows, total = m.batch_plan(offs, lens)
        m.set_stream(torch.cuda.current_stream().cuda_stream)
        wo = m.batch_output_width()
        T = int(total) // a.utts
        ragged = torch.empty((int(total), wo), dtype=torch.float32, device="cuda:0")
        run = lambda out: m.batch_run_device(pcm.data_ptr(), pcm.numel(), out.data_ptr())
        res = {"shape": shape, "workload": "%d x %g s, 16 kHz" % (a.utts, a.seconds), "frames": int(total), "width": wo,
               "tile_rows": pkg.host_tensor_tile()[0], "kernel": m.dominant_kernel_name(), "runs": []}
        for _ in range(3):
            res["runs"].append(dict(variant="floor", **median_ms(lambda: run(ragged))))
        torch.cuda.synchronize()
        bounds = [int(r) for r in rows] + [int(total)]
        for name, layout, dtype in variants:
            m.batch_set_tensor(layout, dtype, 0, 0.0)
            nbytes = m.batch_output_bytes()
            out = torch.empty(nbytes, dtype=torch.uint8, device="cuda:0")
            res["runs"].append(dict(variant=name, **median_ms(lambda: run(out))))
            r = median_ms(lambda: m.batch_tensor_from_rows(ragged.data_ptr(), out.data_ptr()))
            moved = 4 * int(total) * wo + nbytes
            r.update(bytes=moved, tb_per_s=round(moved / (r["ms_median"] * 1e-3) / 1e12, 3))
            res["runs"].append(dict(variant="pack_" + name, **r))
            m.batch_clear_tensor()

            def torch_pipeline():
                pieces = [ragged[bounds[u]:bounds[u + 1]] for u in range(a.utts)]
                x = torch.nn.utils.rnn.pad_sequence(pieces, batch_first=True)
                if layout == pkg.TENSOR_CHANNEL_MAJOR:
                    x = x.transpose(1, 2)
                return x.to(tdt[dtype]).contiguous()

            res["runs"].append(dict(variant="torch_" + name, **median_ms(torch_pipeline)))
            want = torch_pipeline()
            got = out.view(tdt[dtype]).reshape(want.shape)
            res["runs"][-1]["equal"] = bool(torch.equal(got, want)) and T == want.shape[1 if layout == pkg.TENSOR_TIME_MAJOR else 2]
        m.close()
        print(json.dumps(res), flush=True)

    for shape in (("c2", "whisper") if a.shape == "both" else (a.shape,)):
        one(shape)


if __name__ == "__main__":
    main()
