"""Dev aid (GPU box): from which batch size the fused delta stage of k_front512 wins against front end + k_delta16 -- the
measurement behind kFuseMinFrames (mfx_handle.h).  C2-shaped utterances (998 frames), batches of about 50 k .. 4 M frames,
two handles per size (MFX_ENGINE_NO_FUSE_DELTA, MFX_ENGINE_FUSE_DELTA) timed alternately: ms per step, best and median of 5
rounds of 20 .. 400 steps each.
    python3 tools/fuse_gate_bench.py [engine bits beside MFX_ENGINE_FUSE_DELTA]"""
import os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as G
import torch
pkg = G.load_package()
extra = int(sys.argv[1]) if len(sys.argv) > 1 else 0
n, dev = 160000, torch.device("cuda", 0)
SIZES = (50, 100, 250, 500, 1000, 2000, 4000)
pcm = (3000.0 * torch.randn((max(SIZES), n), device=dev)).round().clamp(-32768, 32767).to(torch.int16)
out = torch.empty((998 * max(SIZES), 39), dtype=torch.float32, device=dev)


def make(engine, n_utt):
    m = pkg.MfccHip(n + 1000, 400, 160, 40, 16000.0, 64.0, 8000.0, 13, False, 22.0, 0, 2, 3, 3, True, engine=engine)
    m.set_window(pkg.reference_window(400))
    m.batch_plan(np.arange(n_utt) * n, np.full(n_utt, n))
    return m


def timed(m, steps):
    """wall time per step over `steps` queued runs (the handle runs on its own stream: drained before and after)"""
    m.synchronize()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        m.batch_run_device(pcm.data_ptr(), pcm.numel(), out.data_ptr())
    m.synchronize()
    return (time.perf_counter() - t0) * 1e3 / steps


for n_utt in SIZES:
    two, fused = make(pkg.mfcc.ENGINE_NO_FUSE_DELTA, n_utt), make(pkg.mfcc.ENGINE_FUSE_DELTA | extra, n_utt)
    assert fused.batch_fuse_info()[0] and not two.batch_fuse_info()[0]
    for m in (two, fused):
        timed(m, max(30, 30000 // n_utt))   # clocks up, tables warm
    t = {"two": [], "fused": []}
    for r in range(5):
        for name, m in (("two", two), ("fused", fused)) if r % 2 == 0 else (("fused", fused), ("two", two)):
            t[name].append(timed(m, max(20, 20000 // n_utt)))
    a, b = np.array(t["two"]), np.array(t["fused"])
    print("%7d frames: two kernels %.4f ms (median %.4f, max %.4f) | fused %.4f ms (median %.4f, max %.4f) | median %+.1f %%" % (
        998 * n_utt, a.min(), np.median(a), a.max(), b.min(), np.median(b), b.max(), 100.0 * (np.median(b) / np.median(a) - 1.0)))
    two.close()
    fused.close()
