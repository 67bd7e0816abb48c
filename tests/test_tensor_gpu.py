"""Dense padded tensor output (mfx_batch_set_tensor) on the GPU.  Every comparison is exact (a NaN is compared as a NaN).

1. k_tensor_pack alone, through mfx_batch_tensor_from_rows on chosen values: every output width, utterance length and pad
   length at which the kernel takes another path, all layout / type pairs, against tensor_ref.py (torch's CPU conversions)
   AND against the host restatement; and every edge value of the conversions.
2. Placement: d_out at every element offset 0 .. 3 inside a larger allocation of sentinels.
3. In a run: MFCC + d + dd, fbank-80, Whisper log-mel, the 1024-point log-mel; the tensor against the reference built from the
   rows of the same handle before the setter; the ragged rows again after the clear.
4. Composition: the transform, the three VAD modes, the set-last rule, overlap.
5. mfx_batch_run_host, unsliced and sliced, against the device entry."""
import ctypes as C

import numpy as np
import pytest

import stft_drive
import tensor_ref as TR
from conftest import synth_utterance

pytestmark = pytest.mark.gpu

W, S, SR = 400, 160, 16000.0
LAYOUTS = (TR.TIME_MAJOR, TR.CHANNEL_MAJOR)
DTYPES = (TR.F32, TR.F16, TR.BF16)
PAIRS = [(l, d) for l in LAYOUTS for d in DTYPES]
WIDTHS = (1, 13, 39, 40, 80, 128, 256)
TORCH_BITS = {TR.F32: "int32", TR.F16: "int16", TR.BF16: "int16"}
# sentinels: NaN patterns of the element type (positive as signed integers) that no conversion of the tests' finite inputs gives
GUARD = {TR.F32: 0x7FC0BEEF, TR.F16: 0x7EEF, TR.BF16: 0x7FEF}
INSIDE = {TR.F32: 0x7FC0DEAD, TR.F16: 0x7DAD, TR.BF16: 0x7FAD}


def tile_rows(pkg):
    return pkg.host_tensor_tile()[0]


def framed(pkg, nb=40, nc=0, c0=False, dyn=0, ibs=200000):
    """A framed handle at 16 kHz: log mel energies (nc = 0) or MFCC."""
    m = pkg.MfccHip(ibs, W, S, nb, SR, 64.0, SR / 2, nc, c0, 22.0, pkg.NORM_NONE, dyn, 3, 3, True, device=0, bug_compat=False)
    m.set_window(pkg.reference_window(W))
    return m


def samples_for(m, T, stft):
    """Samples of an utterance of T frames on the handle."""
    n = (100 if T == 0 else T * S + 50) if stft else (300 if T == 0 else (T - 1) * S + W)
    assert m.batch_frames(n) == T
    return n


def plan_frames(m, frames, stft=False):
    lens = [samples_for(m, T, stft) for T in frames]
    offs = np.concatenate([[0], np.cumsum([n + (n & 1) for n in lens])[:-1]]).astype(np.int64)
    rows, total = m.batch_plan(offs, lens)
    assert total == sum(frames)
    return offs, lens, rows, total


def width_handle(pkg, Wo):
    """The cheapest handle of output width Wo: fbank / log-mel for the even widths, a transform's out_dim for the rest (set
    after the plan: see planned_width)."""
    if Wo == 40:
        return framed(pkg, nb=40), False, None
    if Wo in (80, 128):
        return stft_drive.make(pkg, 400, 160, Wo, SR, post=pkg.LOGMEL_LOG10), True, None
    return framed(pkg, nb=40), False, Wo


def planned_width(pkg, Wo, frames):
    m, stft, out_dim = width_handle(pkg, Wo)
    offs, lens, rows, total = plan_frames(m, frames, stft)
    if out_dim:
        m.batch_set_transform(np.ones((out_dim, 40), np.float32))
    assert m.batch_output_width() == Wo
    return m, rows, total


_EDGES = []


def edges():
    if not _EDGES:
        e = TR.edge_values()
        e.setflags(write=False)
        _EDGES.append(e)
    return _EDGES[0]


def chosen_rows(total, Wo, seed, nan=True):
    """Random floats over many binades, every third value an edge value of the conversions."""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal(total * Wo) * np.exp2(rng.integers(-30, 18, total * Wo))).astype(np.float32)
    e = edges()
    if not nan:
        e = e[np.isfinite(e.view(np.float32))]
    x[::3] = e[rng.integers(0, e.size, x[::3].size)].view(np.float32)
    return x.reshape(total, Wo)


def run_from_rows(m, d_rows, dtype):
    """The tensor launch alone into an exactly sized allocation of sentinels: the tensor as numpy."""
    import torch
    shape, npdt = m.batch_tensor_shape()
    n = int(np.prod(shape))
    assert m.batch_output_bytes() == n * np.dtype(npdt).itemsize
    out = torch.full((max(n, 1),), INSIDE[dtype], dtype=getattr(torch, TORCH_BITS[dtype]), device="cuda:0")
    torch.cuda.synchronize()                   # (the handle's stream does not wait for torch's)
    m.batch_tensor_from_rows(d_rows.data_ptr(), out.data_ptr())
    m.synchronize()
    return out[:n].cpu().numpy().view(npdt).reshape(shape)


# ---- 1. the kernel alone ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("Wo", WIDTHS)
def test_kernel_alone_equals_the_reference_and_the_host_restatement(pkg, Wo):
    import torch
    R = tile_rows(pkg)
    frames = [0, 1, R - 1, R, R + 1, 2 * R + 1]
    m, rows, total = planned_width(pkg, Wo, frames)
    x = chosen_rows(total, Wo, 100 + Wo)
    d_rows = torch.from_numpy(x).to("cuda:0")
    pad = np.float32(-1.0009765625)            # (between two neighbours of both 16-bit types: the pad is converted, too)
    for t_pad in (0, 1, R, R + 1, 2 * R - 1, 2 * R + 3):
        Tp = t_pad or max(frames)
        for layout, dtype in PAIRS:
            m.batch_set_tensor(layout, dtype, t_pad, pad)
            shape, npdt = m.batch_tensor_shape()
            assert shape == ((len(frames), Tp, Wo) if layout == TR.TIME_MAJOR else (len(frames), Wo, Tp)) and npdt == TR.NP_DTYPE[dtype]
            got = run_from_rows(m, d_rows, dtype)
            what = "Wo %d t_pad %d layout %d dtype %d" % (Wo, t_pad, layout, dtype)
            assert TR.same_bits(got, TR.tensor_ref(x, rows, frames, Tp, layout, dtype, pad), dtype), what
            assert TR.same_bits(got, pkg.host_tensor_pack(x, rows, frames, Tp, layout, dtype, pad), dtype), what
            assert m.batch_tensor_lengths().tolist() == [min(T, Tp) for T in frames], what
    m.close()


@pytest.mark.parametrize("layout,dtype", PAIRS)
def test_kernel_converts_every_edge_value_as_torch_does(pkg, layout, dtype):
    """Every value of tensor_ref.edge_values, as one long utterance of an fbank-40 handle (nothing but the plan is used)."""
    import torch
    e = edges()
    T = (e.size + 39) // 40
    x = np.zeros(T * 40, np.float32)
    x[:e.size] = e.view(np.float32)
    x = x.reshape(T, 40)
    m = framed(pkg, nb=40, ibs=T * S + W)
    _, _, rows, total = plan_frames(m, [T])
    m.batch_set_tensor(layout, dtype, 0, 0.0)
    got = run_from_rows(m, torch.from_numpy(x).to("cuda:0"), dtype)
    m.close()
    want = TR.tensor_ref(x, rows, [T], T, layout, dtype, 0.0)
    if not TR.same_bits(got, want, dtype):                         # name the first few inputs that differ
        g = got if layout == TR.TIME_MAJOR else got.transpose(0, 2, 1)
        w = want if layout == TR.TIME_MAJOR else want.transpose(0, 2, 1)
        gb, wb = np.ascontiguousarray(g).view(TR.BITS_DTYPE[dtype]).reshape(-1), np.ascontiguousarray(w).view(TR.BITS_DTYPE[dtype]).reshape(-1)
        bad = np.nonzero(gb != wb)[0][:8]
        raise AssertionError("differs (NaN payloads aside?) at inputs %s: got %s want %s" % (
            [hex(v) for v in x.reshape(-1).view(np.uint32)[bad]], [hex(v) for v in gb[bad]], [hex(v) for v in wb[bad]]))


# ---- 2. placement ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("layout,dtype", PAIRS)
def test_nothing_outside_the_tensor_is_written_and_the_bits_do_not_depend_on_placement(pkg, layout, dtype):
    """Wo = 39 and Tp = R + 1, both odd: CHANNEL_MAJOR columns of the 16-bit types start on odd half-words wherever d_out lies."""
    import torch
    R = tile_rows(pkg)
    frames = [R + 1, 0, 3, R]
    m, rows, total = planned_width(pkg, 39, frames)
    x = chosen_rows(total, 39, 7, nan=False)
    d_rows = torch.from_numpy(x).to("cuda:0")
    m.batch_set_tensor(layout, dtype, 0, 2.5)
    shape, npdt = m.batch_tensor_shape()
    n, guard = int(np.prod(shape)), 1024
    tdt = getattr(torch, TORCH_BITS[dtype])
    want = TR.tensor_ref(x, rows, frames, R + 1, layout, dtype, 2.5)
    for k in range(4):
        flat = torch.full((guard + k + n + guard,), GUARD[dtype], dtype=tdt, device="cuda:0")
        assert flat.data_ptr() % 16 == 0
        start = guard + k
        for run in range(2):
            flat[start:start + n].fill_(INSIDE[dtype])
            torch.cuda.synchronize()           # (the handle's stream does not wait for torch's)
            m.batch_tensor_from_rows(d_rows.data_ptr(), flat.data_ptr() + start * flat.element_size())
            m.synchronize()
            what = "layout %d dtype %d offset %d run %d" % (layout, dtype, k, run)
            assert bool((flat[:start] == GUARD[dtype]).all()), what + ": write in front of d_out"
            assert bool((flat[start + n:] == GUARD[dtype]).all()), what + ": write past the end of the tensor"
            assert not bool((flat[start:start + n] == INSIDE[dtype]).any()), what + ": an element was never written"
            got = flat[start:start + n].cpu().numpy().view(npdt).reshape(shape)
            assert TR.same_bits(got, want, dtype), what
    m.close()


# ---- 3. in a run ---------------------------------------------------------------------------------------------------------

def device_run(m, pcm, n_bytes):
    """mfx_batch_run_device into an exactly sized allocation (plus sentinels behind it): the bytes written."""
    import torch
    t = torch.from_numpy(np.array(pcm, np.int16)).to("cuda:0")
    out = torch.full((n_bytes + 64,), 0x5A, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()                   # (the handle's stream does not wait for torch's)
    m.batch_run_device(t.data_ptr(), t.numel(), out.data_ptr())
    m.synchronize()
    assert bool((out[n_bytes:] == 0x5A).all()), "write past mfx_batch_output_bytes"
    return out[:n_bytes].cpu().numpy()


def batch_pcm(offs, lens, seed):
    pcm = np.zeros(int(offs[-1]) + int(lens[-1]) + 8, np.int16)
    for i, (o, n) in enumerate(zip(offs, lens)):
        pcm[int(o):int(o) + int(n)] = synth_utterance(int(n), seed + i)
    return pcm


RUN_HANDLES = {
    # name: (maker, stft, width, the layout / type pairs it runs)
    "mfcc39": (lambda pkg: framed(pkg, nb=40, nc=12, c0=True, dyn=2), False, 39, PAIRS),
    "fbank80": (lambda pkg: framed(pkg, nb=80), False, 80, [(TR.TIME_MAJOR, TR.F16), (TR.CHANNEL_MAJOR, TR.F32), (TR.CHANNEL_MAJOR, TR.BF16)]),
    "whisper": (lambda pkg: stft_drive.make(pkg, 400, 160, 80, SR, post=pkg.LOGMEL_WHISPER), True, 80, [(TR.CHANNEL_MAJOR, TR.F16)]),
    "logmel1024": (lambda pkg: stft_drive.make(pkg, 1024, 256, 80, 22050.0, post=pkg.LOGMEL_LOG10, ibs=400000), True, 80,
                   [(TR.CHANNEL_MAJOR, TR.BF16), (TR.TIME_MAJOR, TR.BF16)]),
}


@pytest.mark.parametrize("name", list(RUN_HANDLES))
def test_a_run_delivers_the_tensor_of_its_own_rows_and_the_clear_restores_them(pkg, name):
    maker, stft, width, pairs = RUN_HANDLES[name]
    R = tile_rows(pkg)
    frames = [R - 1, 0, R + 1, R, 37]                       # straddling one tile edge; one utterance without a frame
    m = maker(pkg)
    hop = 256 if name == "logmel1024" else S
    if stft:
        lens = [100 if T == 0 else T * hop + hop // 3 for T in frames]
    else:
        lens = [300 if T == 0 else (T - 1) * S + W + 5 for T in frames]
    assert [m.batch_frames(n) for n in lens] == frames
    offs = np.concatenate([[0], np.cumsum([n + (n & 1) for n in lens])[:-1]]).astype(np.int64)
    rows, total = m.batch_plan(offs, lens)
    pcm = batch_pcm(offs, lens, 300)
    y = m.batch_run_host(pcm)                                 # the ragged rows, before the setter
    assert y.shape == (total, width) and m.batch_output_bytes() == total * width * 4
    for layout, dtype in pairs:
        for t_pad, pad in ((0, 0.0), (R, -80.0)):             # padding to the longest; cutting at the tile edge
            Tp = t_pad or max(frames)
            m.batch_set_tensor(layout, dtype, t_pad, pad)
            want = TR.tensor_ref(y, rows, frames, Tp, layout, dtype, pad)
            got = m.batch_run_host(pcm)
            what = "%s layout %d dtype %d t_pad %d" % (name, layout, dtype, t_pad)
            assert got.shape == want.shape and got.dtype == want.dtype, what
            assert TR.same_bits(got, want, dtype), what
            dev = device_run(m, pcm, m.batch_output_bytes())
            assert np.array_equal(dev, np.ascontiguousarray(got).view(np.uint8).reshape(-1)), what + ": device entry"
            assert m.batch_tensor_lengths().tolist() == [min(T, Tp) for T in frames]
    m.batch_clear_tensor()
    assert m.batch_tensor_shape() is None and m.batch_output_bytes() == total * width * 4
    again = m.batch_run_host(pcm)
    assert again.dtype == np.float32 and np.array_equal(again.view(np.uint32), y.view(np.uint32))
    m.close()


# ---- 4. composition ----------------------------------------------------------------------------------------------------

def mfcc39_batch(pkg):
    R = tile_rows(pkg)
    frames = [R + 40, 0, 2 * R + 5, 90, R]
    m = framed(pkg, nb=40, nc=12, c0=True, dyn=2)
    lens = [300 if T == 0 else (T - 1) * S + W for T in frames]
    offs = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
    rows, total = m.batch_plan(offs, lens)
    pcm = batch_pcm(offs, lens, 500)
    # (a gain envelope, so that an energy VAD has something to decide: half of every utterance is quiet)
    for o, n in zip(offs, lens):
        seg = pcm[int(o):int(o) + int(n)].astype(np.float64)
        seg[(np.arange(n) // (S * 25)) % 2 == 1] /= 256.0
        pcm[int(o):int(o) + int(n)] = np.round(seg).astype(np.int16)
    return m, frames, rows, total, pcm, R


def test_a_transform_in_force_is_packed_at_its_output_width(pkg):
    m, frames, rows, total, pcm, R = mfcc39_batch(pkg)
    rng = np.random.default_rng(3)
    m.batch_set_transform(rng.standard_normal((24, 5 * 39)).astype(np.float32), rng.standard_normal(24).astype(np.float32), left=2, right=2)
    z = m.batch_run_host(pcm)
    assert z.shape == (total, 24)
    for layout, dtype in ((TR.CHANNEL_MAJOR, TR.F16), (TR.TIME_MAJOR, TR.F32)):
        m.batch_set_tensor(layout, dtype, R + 1, 1.0)
        got = m.batch_run_host(pcm)
        assert got.shape == ((5, R + 1, 24) if layout == TR.TIME_MAJOR else (5, 24, R + 1))
        assert TR.same_bits(got, TR.tensor_ref(z, rows, frames, R + 1, layout, dtype, 1.0), dtype)
    m.close()


def test_the_vad_modes_compose_and_a_selecting_vad_decides_the_lengths(pkg):
    m, frames, rows, total, pcm, R = mfcc39_batch(pkg)
    y = m.batch_run_host(pcm)
    # FLAGS: the rows and the lengths are those without the VAD
    m.batch_set_vad(-1, 0.0, 1.0, 2, 0.6, pkg.VAD_FLAGS)
    m.batch_set_tensor(TR.CHANNEL_MAJOR, TR.BF16, 0, -3.0)
    assert m.batch_tensor_lengths().tolist() == frames        # (known before a run: the plan decides them)
    got = m.batch_run_host(pcm)
    assert TR.same_bits(got, TR.tensor_ref(y, rows, frames, max(frames), TR.CHANNEL_MAJOR, TR.BF16, -3.0), TR.BF16)
    assert m.batch_tensor_lengths().tolist() == frames
    m.batch_clear_tensor()
    # SELECT: the voiced rows, then the pad value -- not the +0.0f rows of the ragged form
    m.batch_set_vad(-1, 0.0, 1.0, 2, 0.6, pkg.VAD_SELECT)
    sel = m.batch_run_host(pcm)
    voiced = m.batch_vad_read()[1]
    assert 0 < voiced.sum() < total and (voiced[[0, 2, 3, 4]] > 0).all() and (voiced < np.array(frames))[[0, 2, 3, 4]].all()
    for layout, dtype, t_pad in ((TR.TIME_MAJOR, TR.F32, 0), (TR.CHANNEL_MAJOR, TR.F16, int(voiced.max()) - 1)):
        Tp = t_pad or max(frames)
        m.batch_set_tensor(layout, dtype, t_pad, -7.0)
        with pytest.raises(pkg.MfxError) as ei:                # no run since the setter: the lengths are not decided yet
            m.batch_tensor_lengths()
        assert ei.value.status == -8
        got = m.batch_run_host(pcm)
        assert TR.same_bits(got, TR.tensor_ref(sel, rows, voiced, Tp, layout, dtype, -7.0), dtype)
        dense = got if layout == TR.TIME_MAJOR else got.transpose(0, 2, 1)
        for u in range(5):
            assert (dense[u, min(int(voiced[u]), Tp):] == -7.0).all()
        assert m.batch_tensor_lengths().tolist() == np.minimum(voiced, Tp).tolist()
        assert m.batch_vad_read()[1].tolist() == voiced.tolist()
        with pytest.raises(pkg.MfxError) as ei:                # a VAD in force: the launch alone is refused
            m.batch_tensor_from_rows(1 << 20, 1 << 20)
        assert ei.value.status == -8
        m.batch_clear_tensor()
    # PACK is refused both ways
    m.batch_set_vad(-1, 0.0, 1.0, 2, 0.6, pkg.VAD_PACK)
    with pytest.raises(pkg.MfxError) as ei:
        m.batch_set_tensor(TR.TIME_MAJOR, TR.F32, 0, 0.0)
    assert ei.value.status == -8
    m.batch_clear_vad()
    m.batch_set_tensor(TR.TIME_MAJOR, TR.F32, 0, 0.0)
    with pytest.raises(pkg.MfxError) as ei:
        m.batch_set_vad(-1, 0.0, 1.0, 2, 0.6, pkg.VAD_PACK)
    assert ei.value.status == -8 and "clear the tensor first" in str(ei.value)
    m.close()


def test_the_tensor_is_set_last_and_refused_calls_leave_the_handle_usable(pkg):
    fresh = framed(pkg, nb=40, nc=12, c0=True, dyn=2)
    with pytest.raises(pkg.MfxError) as ei:                    # before a plan
        fresh.batch_set_tensor(TR.TIME_MAJOR, TR.F32, 0, 0.0)
    assert ei.value.status == -8
    fresh.close()
    m, frames, rows, total, pcm, R = mfcc39_batch(pkg)
    y = m.batch_run_host(pcm)
    for bad in ((2, 0, 0), (-1, 0, 0), (0, 3, 0), (0, -1, 0), (0, 0, -1), (0, 0, (1 << 24) + 1)):
        with pytest.raises(pkg.MfxError) as ei:
            m.batch_set_tensor(bad[0], bad[1], bad[2], 0.0)
        assert ei.value.status == -7, bad
    assert m.batch_tensor_shape() is None
    with pytest.raises(pkg.MfxError) as ei:                    # no tensor in force
        m.batch_tensor_lengths()
    assert ei.value.status == -8
    m.batch_set_pitch(32, 200)
    m.batch_set_tensor(TR.TIME_MAJOR, TR.F16, 0, float("nan"))  # (pad_value is not inspected)
    A = np.ones((4, 39), np.float32)
    refused = (lambda: m.batch_set_transform(A), lambda: m._chk(m._L.mfx_batch_set_transform(m._h, 0, 0, 0, 0, None, None, None, 0)),
               lambda: m.batch_set_vad(), lambda: m.batch_clear_vad(), lambda: m.batch_set_pitch_feats(paste=True))
    for call in refused:
        with pytest.raises(pkg.MfxError) as ei:
            call()
        assert ei.value.status == -8 and "clear the tensor first" in str(ei.value)
    m.batch_set_pitch_feats(paste=False)                       # (the row width stays: allowed)
    got = m.batch_run_host(pcm)
    assert TR.same_bits(got, TR.tensor_ref(y, rows, frames, max(frames), TR.TIME_MAJOR, TR.F16, np.float32("nan")), TR.F16)
    # a later plan drops the tensor with the other attachments
    m.batch_plan([0], [W])
    assert m.batch_tensor_shape() is None and m.batch_output_bytes() == 39 * 4
    m.close()


def test_overlap_gives_the_same_tensor_after_synchronize(pkg):
    m, frames, rows, total, pcm, R = mfcc39_batch(pkg)
    m.batch_set_tensor(TR.CHANNEL_MAJOR, TR.F16, 0, 0.0)
    n = m.batch_output_bytes()
    plain = device_run(m, pcm, n)
    m.batch_overlap(True)
    import torch
    t = torch.from_numpy(np.array(pcm, np.int16)).to("cuda:0")
    outs = [torch.full((n,), 0x5A, dtype=torch.uint8, device="cuda:0") for _ in range(3)]
    torch.cuda.synchronize()                   # (the handle's streams do not wait for torch's)
    for o in outs:                                             # queued back to back: tails and front ends overlap
        m.batch_run_device(t.data_ptr(), t.numel(), o.data_ptr())
    m.synchronize()
    for o in outs:
        assert np.array_equal(o.cpu().numpy(), plain)
    m.close()


# ---- 5. the host entry, sliced -----------------------------------------------------------------------------------------

def test_sliced_host_run_with_pinned_buffers_gives_the_device_entrys_bits(pkg):
    """The smallest batch that takes the sliced path of mfx_batch_run_host (the construction of tests/test_vad_gpu.py): 8
    utterances (two slices), 32 MB of PCM, pinned buffers.  The sliced path cuts the tensor by utterance."""
    L = pkg.load_library()
    L.mfx_alloc_pinned.restype, L.mfx_alloc_pinned.argtypes = C.c_void_p, [C.c_size_t]
    L.mfx_free_pinned.restype, L.mfx_free_pinned.argtypes = None, [C.c_void_p]
    rng = np.random.default_rng(23)
    n_utt = 8
    lens = [int(v) for v in rng.integers(2100000, 2110000, size=n_utt)]
    offs, pos = [], 0
    for n in lens:
        offs.append(pos)
        pos += n + int(rng.integers(0, 5))
    assert pos * 2 >= 32 << 20
    pcm = (3000.0 * rng.standard_normal(pos)).astype(np.int16)
    m = framed(pkg, nb=40, nc=12, c0=True, dyn=2)
    rows, total = m.batch_plan(offs, lens)
    frames = [(n - W) // S + 1 for n in lens]
    t_pad = min(frames) - 3                                    # odd or even as it comes; every utterance is cut
    p_in, p_out = L.mfx_alloc_pinned(pos * 2), L.mfx_alloc_pinned(total * 39 * 4)
    assert p_in and p_out
    try:
        C.memmove(p_in, pcm.ctypes.data, pos * 2)

        def pinned_run(n_bytes):
            C.memset(p_out, 0x5A, total * 39 * 4)
            rc = L.mfx_batch_run_host(m._h, C.cast(p_in, C.POINTER(C.c_int16)), pos, C.cast(p_out, C.POINTER(C.c_float)))
            assert rc == 0, L.mfx_last_error(m._h)
            raw = np.ctypeslib.as_array(C.cast(p_out, C.POINTER(C.c_uint8)), shape=(total * 39 * 4,)).copy()
            assert (raw[n_bytes:] == 0x5A).all(), "write past mfx_batch_output_bytes"
            return raw[:n_bytes]

        y = pinned_run(total * 39 * 4).view(np.float32).reshape(total, 39)      # the ragged rows, by the sliced path
        for layout, dtype in ((TR.CHANNEL_MAJOR, TR.F16), (TR.TIME_MAJOR, TR.F32)):
            m.batch_set_tensor(layout, dtype, t_pad, 0.0)
            n = m.batch_output_bytes()
            shape, npdt = m.batch_tensor_shape()
            got = pinned_run(n)
            assert np.array_equal(got, device_run(m, pcm, n))                   # the device entry's bits
            assert np.array_equal(got, np.ascontiguousarray(m.batch_run_host(pcm)).view(np.uint8).reshape(-1))   # pageable: one piece
            assert TR.same_bits(got.view(npdt).reshape(shape), TR.tensor_ref(y, rows, frames, t_pad, layout, dtype, 0.0), dtype)
    finally:
        L.mfx_free_pinned(p_in)
        L.mfx_free_pinned(p_out)
    m.close()
