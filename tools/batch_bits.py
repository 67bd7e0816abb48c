"""Dev aid: bit digests of the batch and session entries over a fixed, seeded matrix -- to compare two builds of the library
on the same machine (a host-side refactor must leave every line as it was):

    python tools/batch_bits.py > a.txt;  MFX_LIB=build/var/lib_other.so python tools/batch_bits.py > b.txt;  diff a.txt b.txt

One process, one line per case: a SHA-256 of the output bytes of three consecutive runs and the launch count of
mfx_profile_read over them.  A case the library refuses prints the status and mfx_last_error instead, which must match too.
The digests depend on the compiler: they are for comparing builds, not for keeping.

The matrix: one shape per front-end kind (rows of KERNEL_TABLE) + a PLP and a TRAPS handle; eight utterances of 0, 1, 15, 16,
17, 64, 65 and 130 frames back to back (one layout with an odd offset); the attachments none / alphas / rates / transform /
speakers / all four; the device entry, the pageable host entry and the device entry with overlap on; the opt-in fused delta
stage with d_out aligned and 4 bytes off; two long cases (two windows of the spectrum slab with a chunk that ends on the
boundary, a sliced pinned host run); three sessions with four ragged pushes per kind."""
import ctypes as C
import hashlib
import os
import signal
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as G  # noqa: E402

pkg = G.load_package()
import torch  # noqa: E402

signal.alarm(int(os.environ.get("BATCH_BITS_TIMEOUT", "600")))   # the tool's own time limit (SIGALRM ends the process)
dev = torch.device("cuda:0")
FRAMES = (0, 1, 15, 16, 17, 64, 65, 130)
ERR_DEVICE = -6

# (kind, the KERNEL_TABLE row it is taken from)
SHAPES = (
    ("kFront512", "C2 / C4"),
    ("kFront1024", "C3  16 kHz"),
    ("kFront2048", "C5  44.1 kHz stereo"),
    ("kFrontGenFused", "512 pt, more than 128 filters"),
    ("kSpec512", "any shape on the streaming interface's kernels"),
    ("kSpecGen", "4096 pt (50 ms at 48 kHz)"),
)
C2 = dict(window_size=400, shift=160, num_banks=40, sample_rate=16000.0, ceps_len=13, dyn=pkg.DYN_ACC)
EXTRA = (
    ("plp", dict(C2, method=pkg.METHOD_PLP, lpc_order=12)),
    ("traps", dict(window_size=400, shift=160, num_banks=15, sample_rate=16000.0, ceps_len=0, method=pkg.METHOD_TRAPS, traps_len=31,
                   traps_dct_len=10)),
)


def table_row(prefix):
    rows = [kw for what, kw, _ in pkg.KERNEL_TABLE if what.startswith(prefix)]
    assert len(rows) == 1, prefix
    return {k: v for k, v in rows[0].items() if k != "aligned"}


def handle(kw, norm=pkg.NORM_NONE, engine=0, limit=200000):
    W, S, sr = kw["window_size"], kw["shift"], kw["sample_rate"]
    m = pkg.MfccHip(limit, W, S, kw["num_banks"], sr, 64.0, sr / 2, kw["ceps_len"], kw.get("want_c0", False), 22.0, norm,
                    kw.get("dyn", pkg.DYN_NONE), 3, 3, True, device=0, fft_size=kw.get("fft_size", 0), channels=kw.get("channels", 1),
                    engine=kw.get("engine", 0) | engine, method=kw.get("method", pkg.METHOD_MFCC), lpc_order=kw.get("lpc_order", 0),
                    traps_len=kw.get("traps_len", 0), traps_dct_len=kw.get("traps_dct_len", 0))
    m.set_window(pkg.reference_window(W))
    m.profile_enable(True)
    return m


def signal_pcm(n, ch, seed):
    rng = np.random.default_rng(seed)
    t = np.arange(n)[:, None]
    x = 3000 * rng.standard_normal((n, ch)) + 6000 * np.sin(2 * np.pi * 440.0 * t / 16000.0)
    return np.clip(np.round(x), -32768, 32767).astype(np.int16)


def layout(kw, frames, odd=False):
    """Utterances of `frames` frames back to back on even offsets (odd: one sample slipped in before the fourth)."""
    W, S = kw["window_size"], kw["shift"]
    lens = [(W // 2 if t == 0 else W + (t - 1) * S + (7 * i) % S) & ~1 for i, t in enumerate(frames)]
    offs, pos = [], 0
    for i, n in enumerate(lens):
        pos += 1 if (odd and i == 3) else 0
        offs.append(pos)
        pos += n
    return offs, lens, pos + 2


def rated(kw, offs, lens):
    """The same utterances arriving at 8 kHz, 48 kHz and the output rate in turn: (offsets, lengths, rates, samples)."""
    out_hz = int(kw["sample_rate"])
    rates = [(out_hz, 8000, 48000)[i % 3] for i in range(len(lens))]
    in_lens = [(-(-n * r // out_hz) + 1) & ~1 for n, r in zip(lens, rates)]
    in_offs = np.concatenate([[0], np.cumsum(in_lens)[:-1]]).tolist()
    return in_offs, in_lens, rates, int(np.sum(in_lens)) + 2


def attach(m, what, n_utt):
    """Attach `what` to the planned batch; a shape that refuses it raises MfxError (the case is then skipped, by name)."""
    wd = m.get_output_data_width()
    if "alphas" in what:
        m.batch_set_alphas(np.array([0.9, 1.0, 1.1], np.float32)[np.arange(n_utt) % 3])
    if "speakers" in what:
        m.batch_set_speakers(np.arange(n_utt, dtype=np.int32) % 3, n_spk=3)
    if "transform" in what:
        rng = np.random.default_rng(24)
        m.batch_set_transform((0.1 * rng.standard_normal((2, 24, 5 * wd))).astype(np.float32), rng.standard_normal((2, 24)).astype(np.float32),
                              left=2, right=2, utt_xf=np.arange(n_utt, dtype=np.int32) % 2)


def run_device(m, d_pcm, samples, rows, off_floats=0):
    ow = m.batch_output_width()
    buf = torch.zeros(rows * ow + 8, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    m.batch_run_device(d_pcm.data_ptr(), samples, buf.data_ptr() + 4 * off_floats)
    m.synchronize()
    return buf[off_floats:off_floats + rows * ow].cpu().numpy().tobytes()


def report(name, m, fn, runs=3):
    """One line: the digest of `runs` consecutive fn() and the launches they added, or the status the library answered."""
    try:
        m.profile_read(True)
        sha = hashlib.sha256()
        for _ in range(runs):
            sha.update(fn())
        print("%-64s sha256=%s launches=%d" % (name, sha.hexdigest(), m.profile_read(True)[0]), flush=True)
    except pkg.MfxError as e:
        print("%-64s status=%d %s" % (name, e.status, e), flush=True)
        if e.status == ERR_DEVICE:
            sys.exit("device error: nothing more is started")


def planned(kw, what, norm, odd=False, engine=0):
    """A handle with the eight utterances planned and `what` attached: (handle, pcm [samples][ch], rows) or None (refused)."""
    ch = kw.get("channels", 1)
    m = handle(kw, norm, engine)
    offs, lens, samples = layout(kw, FRAMES, odd)
    try:
        if "rates" in what:
            offs, lens, rates, samples = rated(kw, offs, lens)
            _, rows = m.batch_plan_rates(offs, lens, rates)
        else:
            _, rows = m.batch_plan(offs, lens)
        attach(m, what, len(lens))
    except pkg.MfxError as e:
        m.close()
        return None, "status=%d %s" % (e.status, e)
    return (m, signal_pcm(samples, ch, 7), rows), None


SUBSETS = (("none", pkg.NORM_NONE), ("alphas", pkg.NORM_NONE), ("rates", pkg.NORM_NONE), ("transform", pkg.NORM_NONE),
           ("cvn", pkg.NORM_CVN), ("speakers", pkg.NORM_CVN), ("alphas+rates+transform+speakers", pkg.NORM_CVN))


def batch_matrix():
    shapes = [(k, table_row(p)) for k, p in SHAPES] + list(EXTRA)
    for sname, kw in shapes:
        for what, norm in SUBSETS:
            for odd in ((False, True) if what in ("none", "alphas") else (False,)):
                name = "%s %s%s" % (sname, what, " odd" if odd else "")
                got, why = planned(kw, what, norm, odd)
                if got is None:
                    print("%-64s skipped: %s" % (name, why), flush=True)
                    continue
                m, pcm, rows = got
                samples = pcm.shape[0]
                d_pcm = torch.from_numpy(pcm).to(dev)
                print("%-64s kernel=%s rows=%d width=%d" % (name, m.dominant_kernel_name(), rows, m.batch_output_width()), flush=True)
                report(name + " device", m, lambda: run_device(m, d_pcm, samples, rows))
                report(name + " host", m, lambda: m.batch_run_host(pcm).tobytes())
                m.batch_overlap(True)
                report(name + " overlap", m, lambda: run_device(m, d_pcm, samples, rows))
                m.close()


def fuse_delta():
    kw = table_row("C2 / C4")
    for what, norm in (("none", pkg.NORM_NONE), ("transform", pkg.NORM_NONE), ("cvn", pkg.NORM_CVN), ("speakers", pkg.NORM_CVN)):
        got, why = planned(kw, what, norm, engine=2)   # MFX_ENGINE_FUSE_DELTA
        if got is None:
            print("%-64s skipped: %s" % ("fuse_delta " + what, why), flush=True)
            continue
        m, pcm, rows = got
        d_pcm = torch.from_numpy(pcm).to(dev)
        for off in (0, 1):
            report("fuse_delta %s d_out+%d" % (what, 4 * off), m, lambda: run_device(m, d_pcm, pcm.shape[0], rows, off))
        m.close()


def long_slab():
    """Per-utterance alphas, total_rows = 2^17 + 100: the slab walk takes two windows and a chunk ends exactly on the boundary."""
    kw = table_row("C2 / C4")
    frames = (32768, 32768, 32768, 32768, 100)
    m = handle(kw)
    offs, lens, samples = layout(kw, frames)
    _, rows = m.batch_plan(offs, lens)
    assert rows == (1 << 17) + 100
    attach(m, "alphas", len(lens))
    d_pcm = torch.from_numpy(signal_pcm(samples, 1, 11)).to(dev)
    report("long slab alphas rows=%d" % rows, m, lambda: run_device(m, d_pcm, samples, rows))
    m.close()


def long_sliced():
    """A pinned host run that is sliced (16 ascending utterances, 35 MB of PCM), and the same batch through the device entry."""
    kw = table_row("C2 / C4")
    L = pkg.load_library()
    L.mfx_alloc_pinned.argtypes, L.mfx_alloc_pinned.restype = [C.c_size_t], C.c_void_p
    L.mfx_free_pinned.argtypes, L.mfx_free_pinned.restype = [C.c_void_p], None
    offs, lens, samples = layout(kw, (6870,) * 16)
    assert 2 * samples >= 32 << 20
    pcm = signal_pcm(samples, 1, 13)
    for what in ("none", "alphas+transform"):
        m = handle(kw)
        _, rows = m.batch_plan(offs, lens)
        attach(m, what, len(lens))
        ow = m.batch_output_width()
        p_in, p_out = L.mfx_alloc_pinned(2 * samples), L.mfx_alloc_pinned(4 * rows * ow)
        assert p_in and p_out
        h_in = np.ctypeslib.as_array(C.cast(p_in, C.POINTER(C.c_int16)), (samples,))
        h_out = np.ctypeslib.as_array(C.cast(p_out, C.POINTER(C.c_float)), (rows * ow,))
        h_in[:] = pcm[:, 0]

        def sliced():
            h_out[:] = 0
            m._chk(L.mfx_batch_run_host(m._h, C.cast(p_in, C.POINTER(C.c_int16)), samples, C.cast(p_out, C.POINTER(C.c_float))))
            return h_out.tobytes()
        report("long sliced %s pinned host" % what, m, sliced)
        d_pcm = torch.from_numpy(pcm).to(dev)
        report("long sliced %s device" % what, m, lambda: run_device(m, d_pcm, samples, rows))
        m.close()
        L.mfx_free_pinned(p_in), L.mfx_free_pinned(p_out)


def sessions():
    """Per kind (and PLP): three sessions, four ragged pushes each -- an empty one, and a final flush -- rows concatenated."""
    lens = ((1000, 3000, 0), (0, 123, 2999), (2500, 0, 1601), (777, 0, 40))
    for sname, kw in [(k, table_row(p)) for k, p in SHAPES] + [EXTRA[0]]:
        ch = kw.get("channels", 1)
        m = handle(kw)
        try:
            m.sessions_create(3, 3000)
            m.profile_read(True)
            sha, rows = hashlib.sha256(), 0
            for k, ln in enumerate(lens):
                offs = np.concatenate([[0], np.cumsum(ln)[:-1]])
                _, _, total = m.sessions_plan([0, 1, 2], offs, ln, [int(k == 3)] * 3)
                sha.update(m.sessions_run_host(signal_pcm(int(np.sum(ln)) + 2, ch, 20 + k)).tobytes())
                rows += total
            print("%-64s sha256=%s launches=%d rows=%d" % ("sessions " + sname, sha.hexdigest(), m.profile_read(True)[0], rows), flush=True)
        except pkg.MfxError as e:
            print("%-64s status=%d %s" % ("sessions " + sname, e.status, e), flush=True)
            if e.status == ERR_DEVICE:
                sys.exit("device error: nothing more is started")
        m.close()


if __name__ == "__main__":
    print("library: %s" % os.path.basename(pkg.library_path()), file=sys.stderr)
    batch_matrix()
    fuse_delta()
    long_slab()
    long_sliced()
    sessions()
    print("done")
