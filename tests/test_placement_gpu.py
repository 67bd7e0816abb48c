"""Rows of the batch and session entries do not depend on where the caller's buffers lie (include/mfx.h: d_out may have any
4-byte alignment and lie anywhere in a device allocation; nothing outside [d_out, d_out + total_rows * width) is written).

Part 1: d_out at k = 0 .. 3 floats past a 16-byte boundary, between guard bands (tests/placement.py), one case per kernel that
        writes caller memory.  Each case restates its launcher's condition and asserts which side k = 0 and k != 0 take;
        the rows must be the same bits at every k, and at k = 0 the bits of batch_run_host on a fresh handle.
Part 2: PCM offsets past 2^31 and 2^32 elements in an array that is allocated but never filled between the utterances.
Part 3: output rows past 2^32 bytes and 2^31 elements.
The comparisons are on int32 views of the float32 rows: there is no tolerance to choose."""
import time

import numpy as np
import pytest

from conftest import synth_utterance
from placement import OutPlacement, PcmPlacement

pytestmark = pytest.mark.gpu

GIB = float(2 ** 30)
_T0 = time.time()


def torch_dev():
    import torch
    return torch, torch.device("cuda:0")


def handle(pkg, W=400, S=160, nb=40, sr=16000.0, ceps=13, dyn=2, l1=3, l2=3, norm=0, fft=0, ch=1, engine=0, method=0, lpc=0,
           tl=0, tk=0):
    m = pkg.MfccHip(200000, W, S, nb, sr, 64.0, sr / 2, ceps, False, 22.0, norm, dyn, l1, l2, True, device=0, fft_size=fft,
                    channels=ch, bug_compat=False, engine=engine, method=method, lpc_order=lpc, traps_len=tl, traps_dct_len=tk)
    m.set_window(pkg.reference_window(W))
    return m


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.int32)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


# ---- the launchers' conditions, restated ---------------------------------------------------------------------------------

def delta_branch(cols, l1, l2, src_pitch, out_pitch, aligned):
    """launch_delta (mfx_tail.hip); l2 = 0 for dyn = DELTA.  `aligned`: ((uintptr_t)out & 15) == 0 (the statics scratch is
    an allocation of the handle's own: aligned)."""
    D, groups = l1 + l2, 3 if l2 > 0 else 2
    whole_rows = out_pitch == cols * groups
    if cols <= 16 and l1 > 0 and D <= 16 and src_pitch == 16 and whole_rows and aligned:
        return "k_delta16<3,3>" if (l1, l2) == (3, 3) else "k_delta16<0,0>"
    if cols > 16 and cols % 4 == 0 and l1 > 0 and src_pitch % 4 == 0 and whole_rows and aligned and \
            ((32 + 2 * D) + (32 + 2 * l2) + 32) * cols * 4 <= 64 * 1024:
        return "k_delta4<32>"
    return "k_delta<true,64>" if cols <= 16 else "k_delta<false,32>"


def fused_branch(cols, l1, l2, aligned):
    """batch_run_range (mfx_batch.cpp): the fused delta wave of k_front512 needs a 16-byte aligned d_out; without it the
    front end writes the compact statics and launch_delta runs, on the same unaligned d_out."""
    return "fused delta wave" if aligned else "separate " + delta_branch(cols, l1, l2, 16, cols * 3, aligned)


def store_form(cols, pitch, aligned):
    """k_traps (mfx_traps.hip) and k_splice_affine (mfx_xform.hip): 16-byte stores or one float at a time."""
    return "float4" if cols % 4 == 0 and pitch % 4 == 0 and aligned else "scalar"


def norm_branch(cols, max_frames):
    """run_norm (mfx_api.cpp): one block per segment while the longest segment, in whole 64-row tiles, fits 54 KB of LDS."""
    return "k_norm_seg" if (max_frames + 63) // 64 * 64 * cols * 4 <= 54 * 1024 else "k_norm_stats+k_norm_apply"


# ---- part 1 ----------------------------------------------------------------------------------------------------------------

FRAMES = [1, 2, 7, 63, 64, 65, 130]


def ragged(W, S, ch, sr, extra=()):
    """Utterances of FRAMES (+ extra) frames, an empty one and a silent one at mixed even offsets: (pcm elements, offsets,
    lengths, frame counts), offsets and lengths in samples per channel."""
    frames = list(FRAMES) + list(extra)
    utts = [synth_utterance((W + (t - 1) * S + (5 * i) % S) * ch, 900 + i, sr=sr).reshape(-1, ch) for i, t in enumerate(frames)]
    utts.insert(3, synth_utterance((W // 2) * ch, 899, sr=sr).reshape(-1, ch))      # no frame
    frames.insert(3, 0)
    utts.append(np.zeros((W + 39 * S, ch), np.int16))                                # silence
    frames.append(40)
    offs, pos = [], 0
    for i, u in enumerate(utts):
        pos += 2 * (i % 3)
        offs.append(pos)
        pos += (len(u) + 1) & ~1
    pcm = np.zeros((pos + 2, ch), np.int16)
    for o, u in zip(offs, utts):
        pcm[o:o + len(u)] = u
    return pcm, offs, [len(u) for u in utts], frames


def _alphas(m, n):
    m.batch_set_alphas(np.array([0.9, 1.0, 1.1], np.float32)[np.arange(n) % 3])


def _speakers(m, n):
    m.batch_set_speakers(np.arange(n, dtype=np.int32) % 3, n_spk=3)


def _xform(out_dim):
    def setup(m, n):
        rng = np.random.default_rng(out_dim)
        wd = m.get_output_data_width()
        m.batch_set_transform((0.1 * rng.standard_normal((out_dim, 3 * wd))).astype(np.float32),
                              rng.standard_normal(out_dim).astype(np.float32), left=1, right=1)
    return setup


C2 = dict()
CASES = {
    # name: (handle arguments, setup after the plan, extra frame counts, dominant kernel, sides(aligned) -> str, (k = 0, k != 0))
    "mfcc13_acc33": (C2, None, (), "k_front512", lambda a: delta_branch(13, 3, 3, 16, 39, a), ("k_delta16<3,3>", "k_delta<true,64>")),
    "mfcc13_acc25": (dict(l1=2, l2=5), None, (), "k_front512", lambda a: delta_branch(13, 2, 5, 16, 39, a),
                     ("k_delta16<0,0>", "k_delta<true,64>")),
    "mfcc13_fuse_delta": (dict(engine=2), None, (), "k_front512", lambda a: fused_branch(13, 3, 3, a),
                          ("fused delta wave", "separate k_delta<true,64>")),
    "mfcc20_acc33": (dict(ceps=20), None, (), None, lambda a: delta_branch(20, 3, 3, 60, 60, a), ("k_delta4<32>", "k_delta<false,32>")),
    "mfcc13_static": (dict(dyn=0), None, (), "k_front512", None, None),
    "fbank80_static": (dict(nb=80, ceps=0, dyn=0), None, (), "k_front512", None, None),
    "c3_1024pt_static": (dict(nb=80, fft=1024, dyn=0), None, (), "k_front1024", None, None),
    "c5_stereo_2048pt_static": (dict(W=1102, S=441, nb=128, sr=44100.0, ceps=40, ch=2, dyn=0), None, (), "k_front2048", None, None),
    "slab_4096pt_static": (dict(W=2400, S=480, nb=64, sr=48000.0, dyn=0), None, (), "k_front_reg", None, None),
    "plp_static": (dict(method=1, lpc=12, dyn=0), None, (), None, None, None),
    "alpha_list": (C2, _alphas, (), None, lambda a: delta_branch(13, 3, 3, 39, 39, a), ("k_delta<true,64>", "k_delta<true,64>")),
    "cvn_norm_seg": (dict(norm=2), None, (), "k_front512", lambda a: norm_branch(13, 130), ("k_norm_seg", "k_norm_seg")),
    "cvn_two_kernels": (dict(norm=2), None, (1100,), "k_front512", lambda a: norm_branch(13, 1100),
                        ("k_norm_stats+k_norm_apply", "k_norm_stats+k_norm_apply")),
    "speakers3": (dict(norm=2), _speakers, (), "k_front512", None, None),
    "traps_15x10": (dict(nb=15, ceps=0, dyn=0, method=3, tl=31, tk=10), None, (), None, lambda a: store_form(150, 150, a),
                    ("scalar", "scalar")),
    "traps_16x10": (dict(nb=16, ceps=0, dyn=0, method=3, tl=31, tk=10), None, (), None, lambda a: store_form(160, 160, a),
                    ("float4", "scalar")),
    "xform_40": (C2, _xform(40), (), "k_front512", lambda a: store_form(40, 40, a), ("float4", "scalar")),
    "xform_39": (C2, _xform(39), (), "k_front512", lambda a: store_form(39, 39, a), ("scalar", "scalar")),
    "overlap_two_runs": (C2, "overlap", (), "k_front512", lambda a: delta_branch(13, 3, 3, 16, 39, a),
                         ("k_delta16<3,3>", "k_delta<true,64>")),
}


@pytest.mark.parametrize("name", list(CASES))
def test_rows_do_not_depend_on_the_alignment_of_d_out(pkg, name):
    torch, dev = torch_dev()
    kw, setup, extra, kernel, sides, expect = CASES[name]
    if sides is not None:
        assert (sides(True), sides(False)) == expect, "the case does not take the sides of the gate it is named for"
    cfg = dict(W=400, S=160, ch=1, sr=16000.0)
    cfg.update(kw)
    pcm, offs, lens, frames = ragged(cfg["W"], cfg["S"], cfg["ch"], cfg["sr"], extra)

    def prepare():
        m = handle(pkg, **kw)
        rows, total = m.batch_plan(offs, lens)
        if setup == "overlap":
            m.batch_overlap(True)
        elif setup is not None:
            setup(m, len(offs))
        return m, rows, total

    ref_m, rows, total = prepare()
    if kernel is not None:
        assert ref_m.dominant_kernel_name() == kernel
    assert total == sum(frames) and [ref_m.batch_frames(n) for n in lens] == frames
    want = ref_m.batch_run_host(pcm.reshape(-1))
    ref_m.close()

    m, rows, total = prepare()
    width = m.batch_output_width()
    assert want.shape == (total, width)
    d_pcm = PcmPlacement(pcm.size, k=2, device=dev)          # 4 bytes past a 16-byte boundary, inside a larger allocation
    d_pcm.put(0, pcm)
    runs = 2 if setup == "overlap" else 1
    got = {}
    for k in range(4):
        outs = [OutPlacement(total, width, k, device=dev) for _ in range(runs)]
        assert all((o.ptr - 4 * k) % 16 == 0 for o in outs)
        torch.cuda.synchronize()
        for o in outs:
            m.batch_run_device(d_pcm.ptr, pcm.shape[0], o.ptr)
        m.synchronize()
        res = [o.check("%s, d_out %d floats past a 16-byte boundary, run %d" % (name, k, i)).cpu().numpy() for i, o in enumerate(outs)]
        for r in res[1:]:
            assert same_bits(r, res[0]), "%s, k = %d: the second of two overlapped runs differs from the first" % (name, k)
        got[k] = res[0]
    m.close()
    assert same_bits(got[0], want), "%s: rows at an aligned d_out differ from batch_run_host on a fresh handle" % name
    for k in (1, 2, 3):
        diff = bits(got[k]) != bits(got[0])
        assert not diff.any(), "%s: %d elements differ between d_out at k = %d and k = 0 (first at row %d, column %d)" % (
            name, int(diff.sum()), k, *[int(v[0]) for v in np.nonzero(diff)])


def test_every_writer_of_caller_memory_has_a_case():
    assert len(CASES) == 19          # + the session case below


def test_session_rows_do_not_depend_on_the_alignment_of_d_out(pkg):
    """5 sessions, three pushes, the last final; every push's d_out between guards at k = 0 .. 3."""
    torch, dev = torch_dev()
    W, S, width = 400, 160, 39
    assert (delta_branch(13, 3, 3, 16, 39, True), delta_branch(13, 3, 3, 16, 39, False)) == ("k_delta16<3,3>", "k_delta<true,64>")
    frames = [1, 7, 64, 65, 130]
    utts = [synth_utterance(W + (t - 1) * S + 11 * i, 950 + i) for i, t in enumerate(frames)]
    twin = handle(pkg)
    offs, pos = [], 0
    for u in utts:
        offs.append(pos)
        pos += (u.size + 1) & ~1
    whole = np.zeros(pos + 2, np.int16)
    for o, u in zip(offs, utts):
        whole[o:o + u.size] = u
    rows, total = twin.batch_plan(offs, [u.size for u in utts])
    out = twin.batch_run_host(whole)
    twin.close()
    want = [out[r:r + t] for r, t in zip(rows, frames)]

    cuts = [(0, u.size // 3, 2 * u.size // 3 + 1, u.size) for u in utts]
    m = handle(pkg)
    m.sessions_create(len(utts), max(u.size for u in utts))
    got = {}
    for k in range(4):
        m.sessions_reset(-1)
        per = [[] for _ in utts]
        for push in range(3):
            pieces = [u[c[push]:c[push + 1]] for u, c in zip(utts, cuts)]
            po, pos = [], 0
            for i, x in enumerate(pieces):
                pos += 2 * (i % 3)
                po.append(pos)
                pos += (x.size + 1) & ~1
            arr = np.zeros(pos + 2, np.int16)
            for o, x in zip(po, pieces):
                arr[o:o + x.size] = x
            d_pcm = PcmPlacement(arr.size, k=2, device=dev)
            d_pcm.put(0, arr)
            r0, counts, tot = m.sessions_plan(np.arange(len(utts)), po, [x.size for x in pieces], [push == 2] * len(utts))
            o = OutPlacement(tot, width, k, device=dev)
            torch.cuda.synchronize()
            m.sessions_run_device(d_pcm.ptr, arr.size, o.ptr)
            m.synchronize()
            res = o.check("sessions, push %d, d_out %d floats past a 16-byte boundary" % (push, k)).cpu().numpy()
            for i in range(len(utts)):
                per[i].append(res[r0[i]:r0[i] + counts[i]])
        got[k] = [np.concatenate(p) for p in per]
    m.close()
    for i, (g, w) in enumerate(zip(got[0], want)):
        assert same_bits(g, w), "session %d at an aligned d_out differs from the batch rows of its utterance" % i
    for k in (1, 2, 3):
        for i, g in enumerate(got[k]):
            assert same_bits(g, got[0][i]), "session %d: rows differ between d_out at k = %d and k = 0" % (i, k)


# ---- part 2: PCM offsets past 2^31 and 2^32 ------------------------------------------------------------------------------

FAR_N = 2 ** 32 + 2 ** 20           # int16 elements: 8 GiB
_FAR = {}


def free_gib():
    torch, dev = torch_dev()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    return torch.cuda.mem_get_info(dev)[0] / GIB


def far_pcm():
    """The 8 GiB array, allocated once and shared: torch.empty, nothing filled or read between the utterances."""
    torch, dev = torch_dev()
    if "pcm" not in _FAR:
        need = 2 * FAR_N / GIB + 0.25
        free = free_gib()
        if free < need + 2:
            pytest.skip("needs %.2f GiB of HBM (the PCM array and small buffers) and 2 GiB to spare; %.1f GiB are free" % (need, free))
        _FAR["pcm"] = PcmPlacement(FAR_N, k=2, device=dev)
    return _FAR["pcm"]


def release_far_pcm():
    _FAR.clear()
    free_gib()


def far_offsets(odd):
    """Element offsets: 2^31 - 5000 straddles byte 2^32, 2^32 - 6000 straddles element 2^32."""
    return [0, 2 ** 31 - 5000, 2 ** 31 + 2] + ([2 ** 31 + 1] if odd else []) + [2 ** 32 - 6000, 2 ** 32 + 4]


def far_utterances(arr, offsets, n_elems, seed):
    """Noise at every offset (later ones overwrite the overlap with earlier ones), then the utterances as the array holds
    them: `n_elems` elements from each offset."""
    for i, o in enumerate(offsets):
        arr.put(o, synth_utterance(n_elems, seed + i))
    return [arr.interior()[o:o + n_elems].cpu().numpy().copy() for o in offsets]


def lone_rows(m, samples, ch, parity, setup=None, rate=None):
    """The utterance alone on handle m, planned at offset `parity` (0, or 1 so that an odd utterance takes the same build)."""
    torch, dev = torch_dev()
    n = samples.size // ch
    small = torch.zeros(samples.size + parity * ch + 8, dtype=torch.int16, device=dev)
    small[parity * ch:parity * ch + samples.size] = torch.from_numpy(samples).to(dev)
    if rate is None:
        _, total = m.batch_plan([parity], [n])
    else:
        _, total = m.batch_plan_rates([parity], [n], [rate])
    if setup is not None:
        setup(m, 1)
    out = OutPlacement(total, m.batch_output_width(), 0, device=dev)
    torch.cuda.synchronize()
    m.batch_run_device(small.data_ptr(), n + parity, out.ptr)
    m.synchronize()
    return out.check("lone utterance").cpu().numpy()


FAR_CASES = {
    # name: (handle arguments, dominant kernel, odd offset too, input rate)
    "c2_front512_aligned": (dict(), "k_front512", False, None),
    "c2_front512_unaligned": (dict(), "k_front512", True, None),
    "c3_front1024": (dict(nb=80, fft=1024, dyn=0), "k_front1024", False, None),
    "c5_stereo_front2048": (dict(W=1102, S=441, nb=128, sr=44100.0, ceps=40, ch=2), "k_front2048", False, None),
    "front_reg_96_filters": (dict(nb=96, fft=1024, dyn=0), "k_front_reg", False, None),
    "slab_with_alpha_list": (dict(), None, False, None),
    "rates_8k_to_16k": (dict(), "k_front512", True, 8000),
}


@pytest.mark.parametrize("name", list(FAR_CASES))
def test_pcm_offsets_past_2_31_and_2_32(pkg, name):
    """Needs 8.25 GiB of HBM.  Utterances of about 70 frames at elements 0, 2^31 - 5000, 2^31 + 2, (2^31 + 1,) 2^32 - 6000 and
    2^32 + 4 of one array; each one's rows against the same samples alone at offset 0 (1 for the odd one) on a fresh handle."""
    torch, dev = torch_dev()
    kw, kernel, odd, rate = FAR_CASES[name]
    cfg = dict(W=400, S=160, ch=1)
    cfg.update(kw)
    W, S, ch = cfg["W"], cfg["S"], cfg["ch"]
    arr = far_pcm()
    n = W + 69 * S + 18                       # samples per channel at the rate the features are extracted at
    if rate is not None:
        n //= 2
    elem_offs = far_offsets(odd)
    utts = far_utterances(arr, elem_offs, n * ch, 1000)
    offs = [o // ch for o in elem_offs]       # (stereo: every element offset of the list is even)
    with_alphas = name == "slab_with_alpha_list"
    setup = _alphas if with_alphas else None

    m = handle(pkg, **kw)
    if rate is None:
        rows, total = m.batch_plan(offs, [n] * len(offs))
    else:
        rows, total = m.batch_plan_rates(offs, [n] * len(offs), [rate] * len(offs))
    if setup is not None:
        setup(m, len(offs))
    if kernel is not None:
        assert m.dominant_kernel_name() == kernel
    width = m.batch_output_width()
    out = OutPlacement(total, width, 0, device=dev)
    torch.cuda.synchronize()
    m.batch_run_device(arr.ptr, FAR_N // ch, out.ptr)
    m.synchronize()
    got = out.check(name).cpu().numpy()
    m.close()
    T = total // len(offs)
    assert T >= 69 and total == T * len(offs)

    alphas = np.array([0.9, 1.0, 1.1], np.float32)
    ref = handle(pkg, **kw)
    for i, (o, u) in enumerate(zip(elem_offs, utts)):
        one = (lambda mm, _n, a=alphas[i % 3]: mm.batch_set_alphas(np.array([a], np.float32))) if with_alphas else None
        want = lone_rows(ref, u, ch, o & 1, one, rate)
        g = got[rows[i]:rows[i] + T]
        diff = bits(g) != bits(want)
        assert want.shape == g.shape and not diff.any(), "%s: utterance at element %d: %d elements differ from the same samples at offset %d" % (
            name, o, int(diff.sum()), o & 1)
    ref.close()


def test_session_pieces_at_pcm_offsets_past_2_31_and_2_32(pkg):
    """Needs 8.25 GiB of HBM.  One final push of six sessions whose pieces lie at the far offsets of the caller's array
    (k_sess_gather reads them), against the same pieces packed at the start of a small array on a fresh handle."""
    torch, dev = torch_dev()
    W, S = 400, 160
    arr = far_pcm()
    n = W + 69 * S + 18
    offs = far_offsets(True)
    utts = far_utterances(arr, offs, n, 1100)
    ids = np.arange(len(offs))

    def push(m, ptr, total_elems, offsets):
        m.sessions_create(len(offs), n)
        r0, counts, tot = m.sessions_plan(ids, offsets, [n] * len(offs), [1] * len(offs))
        out = OutPlacement(tot, 39, 0, device=dev)
        torch.cuda.synchronize()
        m.sessions_run_device(ptr, total_elems, out.ptr)
        m.synchronize()
        res = out.check("session push").cpu().numpy()
        m.close()
        return [res[r:r + c] for r, c in zip(r0, counts)]

    got = push(handle(pkg), arr.ptr, FAR_N, offs)
    near = [(n + 4) * i + (o & 1) for i, o in enumerate(offs)]       # the same parities
    small = torch.zeros((n + 4) * len(offs) + 8, dtype=torch.int16, device=dev)
    for o, u in zip(near, utts):
        small[o:o + n] = torch.from_numpy(u).to(dev)
    want = push(handle(pkg), small.data_ptr(), small.numel(), near)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g.shape[0] >= 69 and same_bits(g, w), "session piece at element %d differs from the same samples near the start" % offs[i]


# ---- part 3: output rows past 2^32 bytes and 2^31 elements ---------------------------------------------------------------

UTT_FRAMES = 100


def need_or_skip(gib, what):
    release_far_pcm()
    free = free_gib()
    if free < gib + 2:
        pytest.skip("needs %.1f GiB of HBM (%s) and 2 GiB to spare; %.1f GiB are free" % (gib, what, free))


def tiled_pcm(n_elems, seed):
    """One second of synth_utterance noise, tiled on the device: utterances of another length all differ."""
    torch, dev = torch_dev()
    base = torch.from_numpy(synth_utterance(16000, seed)).to(dev)
    return base.repeat((n_elems + 8 + 15999) // 16000)


def chosen(n_utt, crossing_rows):
    """The first and the last utterance, and around every crossing row the utterance before, the one that holds it and the
    one after."""
    us = {0, n_utt - 1}
    for r in crossing_rows:
        u = r // UTT_FRAMES
        assert 1 <= u < n_utt - 1
        us |= {u - 1, u, u + 1}
    return sorted(us)


def run_big(m, pcm, n_utt, L, out, what, setup=None):
    torch, dev = torch_dev()
    rows, total = m.batch_plan(np.arange(n_utt, dtype=np.int64) * L, np.full(n_utt, L, np.int64))
    assert total == n_utt * UTT_FRAMES and out.rows == total
    if setup is not None:
        setup(m, n_utt)
    assert out.width == m.batch_output_width()
    torch.cuda.synchronize()
    m.batch_run_device(pcm.data_ptr(), n_utt * L, out.ptr)
    m.synchronize()
    inner = out.check(what)
    assert out.all_finite(), "%s: non-finite values" % what
    return inner


def compare_alone(inner, lone, pcm, L, us, what, setup=None):
    for u in us:
        want = lone_rows(lone, pcm[u * L:(u + 1) * L].cpu().numpy(), 1, 0, setup)
        g = inner[u * UTT_FRAMES:(u + 1) * UTT_FRAMES].cpu().numpy()
        diff = bits(g) != bits(want)
        assert g.shape == want.shape and not diff.any(), "%s: utterance %d (rows from %d): %d elements differ from the utterance alone" % (
            what, u, u * UTT_FRAMES, int(diff.sum()))


def test_transform_rows_past_2_32_bytes_and_2_31_elements(pkg):
    """Needs 12.5 GiB of HBM.  13 MFCC + d + dd -> transform to 256 columns, 8 389 000 rows: k_splice_affine writes across
    byte 2^32 (row 4 194 304) and element 2^31 (row 8 388 608) of d_out."""
    torch, dev = torch_dev()
    W, S = 400, 160
    L = W + (UTT_FRAMES - 1) * S
    n_utt = -(-(8388608 + 300) // UTT_FRAMES)
    need_or_skip(12.5, "8.0 of output, 2.6 of PCM, 1.8 of the handle's scratch")
    pcm = tiled_pcm(n_utt * L, 77)
    rng = np.random.default_rng(256)
    A = (0.1 * rng.standard_normal((256, 3 * 39))).astype(np.float32)
    b = rng.standard_normal(256).astype(np.float32)
    setup = lambda mm, _n: mm.batch_set_transform(A, b, left=1, right=1)
    out = OutPlacement(n_utt * UTT_FRAMES, 256, 0, device=dev)
    m = handle(pkg)
    inner = run_big(m, pcm, n_utt, L, out, "transform, 256 columns", setup)
    m.close()
    assert out.n > 2 ** 31 and 4 * out.n > 2 ** 32
    lone = handle(pkg)
    compare_alone(inner, lone, pcm, L, chosen(n_utt, [4194304, 8388608]), "transform, 256 columns", setup)
    lone.close()


def test_traps_rows_past_2_31_elements(pkg):
    """Needs 10 GiB of HBM.  TRAPS 15 x 10 with d + dd (450 columns), 4 772 500 rows: k_traps and k_delta<false,32> write
    across element 2^31 (row 4 772 185) and byte 2^32 of d_out; a second run with CMN puts k_norm_stats / k_norm_apply there."""
    torch, dev = torch_dev()
    W, S = 400, 160
    L = W + (UTT_FRAMES - 1) * S
    n_utt = -(-(4772186 + 300) // UTT_FRAMES)
    assert delta_branch(150, 3, 3, 450, 450, True) == "k_delta<false,32>" and norm_branch(150, UTT_FRAMES) == "k_norm_stats+k_norm_apply"
    need_or_skip(10.0, "8.0 of output, 1.5 of PCM, 0.3 of the handle's scratch")
    pcm = tiled_pcm(n_utt * L, 78)
    out = OutPlacement(n_utt * UTT_FRAMES, 450, 0, device=dev)
    assert out.n > 2 ** 31
    cross = [2 ** 31 // 450, 2 ** 30 // 450]
    for norm in (0, 1):
        kw = dict(nb=15, ceps=0, method=3, tl=31, tk=10, norm=norm)
        out.refill()
        m = handle(pkg, **kw)
        inner = run_big(m, pcm, n_utt, L, out, "TRAPS 450 columns, norm %d" % norm)
        m.close()
        lone = handle(pkg, **kw)
        compare_alone(inner, lone, pcm, L, chosen(n_utt, cross), "TRAPS 450 columns, norm %d" % norm)
        lone.close()


def test_plain_rows_at_hop_16_past_2_32_bytes(pkg):
    """Needs 8 GiB of HBM.  39-wide rows at window 400, hop 16: 27 532 200 rows of 156 bytes, k_front512 + k_delta16 across byte
    2^32 of d_out (row 27 531 841: 27 531 000 rows, 4 294 836 000 bytes, would end short of it).  Then with CVN and a speaker list of 7
    speakers: k_spk_sums and k_spk_apply cross it too; there the lone run carries the speaker's utterances."""
    torch, dev = torch_dev()
    W, S = 400, 16
    L = W + (UTT_FRAMES - 1) * S
    n_utt = 275322
    assert delta_branch(13, 3, 3, 16, 39, True) == "k_delta16<3,3>"
    need_or_skip(8.0, "4.0 of output, 1.0 of PCM, 1.7 of the handle's scratch, 0.9 for a speaker alone")
    pcm = tiled_pcm(n_utt * L, 79)
    out = OutPlacement(n_utt * UTT_FRAMES, 39, 0, device=dev)
    cross = 2 ** 32 // 156
    assert cross // UTT_FRAMES < n_utt - 1 and 4 * out.n > 2 ** 32
    us = chosen(n_utt, [cross])

    m = handle(pkg, S=S)
    assert m.dominant_kernel_name() == "k_front512"
    inner = run_big(m, pcm, n_utt, L, out, "39 columns at hop 16")
    m.close()
    lone = handle(pkg, S=S)
    compare_alone(inner, lone, pcm, L, us, "39 columns at hop 16")
    lone.close()

    out.refill()
    m = handle(pkg, S=S, norm=2)
    inner = run_big(m, pcm, n_utt, L, out, "39 columns at hop 16, 7 speakers", lambda mm, n: mm.batch_set_speakers(np.arange(n, dtype=np.int32) % 7, n_spk=7))
    m.close()
    for s in sorted({u % 7 for u in us}):
        mine = np.arange(s, n_utt, 7, dtype=np.int64)
        lone = handle(pkg, S=S, norm=2)
        rows, total = lone.batch_plan(mine * L, np.full(mine.size, L, np.int64))
        lone.batch_set_speakers(np.zeros(mine.size, np.int32), n_spk=1)
        alone = OutPlacement(total, 39, 0, device=dev)
        torch.cuda.synchronize()
        lone.batch_run_device(pcm.data_ptr(), n_utt * L, alone.ptr)
        lone.synchronize()
        a = alone.check("speaker %d alone" % s)
        lone.close()
        for u in us:
            if u % 7 == s:
                g = inner[u * UTT_FRAMES:(u + 1) * UTT_FRAMES].cpu().numpy()
                w = a[(u // 7) * UTT_FRAMES:(u // 7 + 1) * UTT_FRAMES].cpu().numpy()
                assert same_bits(g, w), "speaker %d, utterance %d (rows from %d) differs from the speaker alone" % (s, u, u * UTT_FRAMES)
        del alone, a


def test_zz_the_far_array_is_released():
    """The 8 GiB array does not outlive this file; prints the file's wall time for DESIGN.md (pytest -s)."""
    release_far_pcm()
    assert not _FAR
    print("tests/test_placement_gpu.py: %.1f s since import" % (time.time() - _T0))
