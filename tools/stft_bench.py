"""STFT log-mel front end (MFX_METHOD_STFT_LOGMEL) on 1000 x 10 s at 16 kHz, N = 400, S = 160, WHISPER mode, M = 80 and 128:
device time of mfx_batch_run_device around HIP events on torch's stream, after warm-up, median of --reps.  Beside it, in the
same process and on the same device, what a user runs today: torch.stft (center, reflect) + power + mel matmul + log10 /
clamp / map in float32 on the same padded batch (`torch`), timed the same way.
  fma_per_frame   what k_stft_mel issues on the matrix pipe: ceil(N / 4) steps x 2 ceil((N / 2 + 1) / 16) tiles x 1024 / 16 frames
  peak_fraction   2 fma_per_frame frames / time against the 157 TF float32 matrix peak
--dft / --hop / --sr choose another shape (the defaults are the run above); at --dft 1024 or 2048 the handle runs the FFT form,
k_stft_fft_mel, which issues nothing on the matrix pipe: fma_per_frame and peak_fraction are null there.
Prints one JSON line.  The kernel's share comes from a separate
`rocprofv3 --kernel-trace --stats -- python tools/stft_bench.py --reps 3 --no-torch`.
usage: python tools/stft_bench.py [--utts 1000] [--seconds 10] [--reps 10] [--warmup 3] [--banks 80,128] [--no-torch]
                                  [--dft 400] [--hop 160] [--sr 16000]"""
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
    ap.add_argument("--banks", default="80,128")
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--dft", type=int, default=400)
    ap.add_argument("--hop", type=int, default=160)
    ap.add_argument("--sr", type=int, default=16000)
    a = ap.parse_args()

    import numpy as np
    import torch
    import __graft_entry__ as G
    import bench
    pkg = G.load_package()
    sr, N, S = a.sr, a.dft, a.hop
    fft_form = N > 512
    n = int(a.seconds * sr)
    pcm = bench.synth_pcm_torch(torch, a.utts, n, float(sr), 0, "cuda:0").reshape(-1).contiguous()
    offs = np.arange(a.utts, dtype=np.int64) * n
    lens = np.full(a.utts, n, dtype=np.int64)
    win = pkg.periodic_hann(N)
    steps, tiles = (N + 3) // 4, 2 * ((N // 2 + 1 + 15) // 16)
    fma = None if fft_form else steps * tiles * 1024 // 16

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

    res = {"workload": "%d x %g s, %g kHz, N %d, S %d, whisper" % (a.utts, a.seconds, sr / 1000.0, N, S), "fma_per_frame": fma, "runs": []}
    for M in [int(v) for v in a.banks.split(",")]:
        m = pkg.MfccHip(n + 1000, N, S, M, float(sr), 0.0, sr / 2.0, 0, False, 22.0, device=0, method=pkg.METHOD_STFT_LOGMEL)
        m.set_window(win)
        rows, total = m.batch_plan(offs, lens)
        out = torch.empty((total, M), dtype=torch.float32, device="cuda:0")
        m.set_stream(torch.cuda.current_stream().cuda_stream)
        med, best = timed(lambda: m.batch_run_device(pcm.data_ptr(), pcm.numel(), out.data_ptr()))
        m.profile_enable(True)
        for _ in range(3):
            m.batch_run_device(pcm.data_ptr(), pcm.numel(), out.data_ptr())
        launches, kms = m.profile_read()
        m.profile_enable(False)
        res["runs"].append({"variant": "mfx", "M": M, "kernel": m.dominant_kernel_name(), "ms_median": round(med, 4),
                            "ms_min": round(best, 4), "k_stft_mel_ms": round(kms / max(launches, 1), 4), "kernel_ms": round(kms / max(launches, 1), 4), "frames": int(total),
                            "frames_per_s": round(total / (med * 1e-3), 1),
                            "peak_fraction": None if fft_form else round(2.0 * fma * total / (med * 1e-3) / 157e12, 4),
                            "finite": bool(torch.isfinite(out).all().item())})
        if not a.no_torch:
            w, _, _ = pkg.host_slaney_mel_table(M, N, float(sr), 0.0, sr / 2.0)
            wt = torch.from_numpy(w).to("cuda:0")
            hann = torch.from_numpy(win).to("cuda:0")
            x16 = pcm.reshape(a.utts, n)

            def torch_logmel():
                x = x16.to(torch.float32) * (1.0 / 32768.0)
                X = torch.stft(x, N, hop_length=S, window=hann, center=True, pad_mode="reflect", return_complex=True)[..., :-1]
                P = X.real * X.real + X.imag * X.imag
                L = torch.log10(torch.clamp(torch.matmul(wt, P), min=1e-10))
                L = torch.maximum(L, L.amax(dim=(1, 2), keepdim=True) - 8.0)
                return (L + 4.0) * 0.25

            tmed, tbest = timed(torch_logmel)
            ref = torch_logmel().transpose(1, 2).reshape(-1, M)
            res["runs"].append({"variant": "torch", "M": M, "ms_median": round(tmed, 4), "ms_min": round(tbest, 4),
                                "frames_per_s": round(total / (tmed * 1e-3), 1),
                                "max_abs_diff_to_mfx": float((ref - out).abs().max().item())})
            del ref
        m.close()
        del out
    print(json.dumps(res))


if __name__ == "__main__":
    main()
