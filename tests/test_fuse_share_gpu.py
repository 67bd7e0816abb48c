"""The fused delta stage of k_front512 with tile sharing: the delta wave claims the block's tiles from the
head of its list, front-end waves that have run out of frames claim them from the tail and work them off as 16-row sub-tiles
in their own frame slots.  Every case compares d_out bit for bit (int32 views: no tolerance to choose) with the same batch
under MFX_ENGINE_NO_FUSE_DELTA on a fresh handle, between guard bands (tests/placement.py); synchronize() raises if the
bounded wait of a delta or helper wave ever ran out (err_flag).  Which path ran is asserted from mfx_batch_fuse_info and from
the host formulas restated here."""
import numpy as np
import pytest

from conftest import synth_utterance
from placement import OutPlacement, PcmPlacement

pytestmark = pytest.mark.gpu

W, S = 400, 160
MODES = ("share", "no_share", "share_all")


def torch_dev():
    import torch
    return torch, torch.device("cuda:0")


def engine_of(pkg, mode):
    e = pkg.mfcc
    return {"two_kernels": e.ENGINE_NO_FUSE_DELTA, "default": 0, "share": e.ENGINE_FUSE_DELTA,
            "no_share": e.ENGINE_FUSE_DELTA | e.ENGINE_FUSE_NO_SHARE, "share_all": e.ENGINE_FUSE_DELTA | e.ENGINE_FUSE_SHARE_ALL}[mode]


def handle(pkg, mode, ceps=13, dyn=2, l1=3, l2=3):
    m = pkg.MfccHip(700000, W, S, 40, 16000.0, 64.0, 8000.0, ceps, False, 22.0, 0, dyn, l1, l2 if dyn == 2 else 0, True, device=0,
                    bug_compat=False, engine=engine_of(pkg, mode))
    m.set_window(pkg.reference_window(W))
    return m


def sub_tile_fits(l1, l2):
    """delta_share_fits (mfx_kernels.h): statics + context, deltas + context as 16-float rows, 16 output rows of up to 48 floats,
    8 floats of phase -- inside a wave's four 512-float frame slots"""
    return ((16 + 2 * (l1 + l2)) + (16 + 2 * l2)) * 16 + 16 * 48 + 8 <= 4 * 512


def expected_share(mode, l1, l2):
    return {"share": 1, "no_share": 0, "share_all": 2}[mode] if sub_tile_fits(l1, l2) else 0


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.int32)


def pack(utts):
    offs, pos = [], 0
    for u in utts:
        offs.append(pos)
        pos += (u.size + 1) & ~1
    pcm = np.zeros(pos + 8, np.int16)
    for o, u in zip(offs, utts):
        pcm[o:o + u.size] = u
    return pcm, offs, [u.size for u in utts]


def samples(frames):
    return W + (frames - 1) * S if frames > 0 else 0


def tone(frames):
    """whole periods per shift (16 samples | 160): every frame holds the same samples, so delta and delta-delta are exactly 0"""
    n = np.arange(samples(frames))
    return np.round(6000.0 * np.sin(2 * np.pi * n / 16.0)).astype(np.int16)


RAGGED_FRAMES = (1, 2, 6, 7, 13, 63, 64, 65, 129, 200)


def ragged_batch():
    utts = [synth_utterance(samples(t) + 7 * i, 400 + i) for i, t in enumerate(RAGGED_FRAMES)]
    utts += [np.zeros(0, np.int16), np.zeros(samples(30), np.int16), tone(40)]
    return pack(utts)


_REF = {}


def run(pkg, mode, pcm, offs, lens, runs=1, **cfg):
    """rows of `runs` runs on one handle (each between guard bands), and mfx_batch_fuse_info after them"""
    torch, dev = torch_dev()
    m = handle(pkg, mode, **cfg)
    rows, total = m.batch_plan(offs, lens)
    width = m.batch_output_width()
    d_pcm = PcmPlacement(pcm.size, k=0, device=dev)
    d_pcm.put(0, pcm)
    outs = [OutPlacement(total, width, 0, device=dev) for _ in range(runs)]
    torch.cuda.synchronize()
    for o in outs:
        m.batch_run_device(d_pcm.ptr, pcm.size, o.ptr)
    m.synchronize()                                   # (raises if a wave gave up waiting: err_flag)
    got = [o.check("%s run %d" % (mode, i)).cpu().numpy() for i, o in enumerate(outs)]
    info = m.batch_fuse_info()
    m.close()
    return got, rows, info


def reference(pkg, key, pcm, offs, lens, **cfg):
    """the two-kernel rows of a batch, computed once per (batch, configuration) and never written to"""
    k = (key, tuple(sorted(cfg.items())))
    if k not in _REF:
        got, rows, info = run(pkg, "two_kernels", pcm, offs, lens, **cfg)
        assert info[0] is False and info[2] == 0, "MFX_ENGINE_NO_FUSE_DELTA planned or ran the fused form"
        got[0].setflags(write=False)
        _REF[k] = (got[0], rows)
    return _REF[k]


def check(pkg, key, mode, pcm, offs, lens, runs=1, **cfg):
    want, rows = reference(pkg, key, pcm, offs, lens, **cfg)
    got, rows_f, info = run(pkg, mode, pcm, offs, lens, runs=runs, **cfg)
    l1, l2 = cfg.get("l1", 3), cfg.get("l2", 3) if cfg.get("dyn", 2) == 2 else 0
    assert list(rows_f) == list(rows)
    assert info[0] is True and info[2] == runs, "the fused form did not run: %r" % (info,)
    assert info[1] == expected_share(mode, l1, l2), "tile sharing is not what the host formula says: %r" % (info,)
    for i, g in enumerate(got):
        assert g.shape == want.shape
        diff = bits(g) != bits(want)
        assert not diff.any(), "%s %s run %d: %d elements differ from the two-kernel rows (first at row %d, column %d)" % (
            key, mode, i, int(diff.sum()), *[int(v[0]) for v in np.nonzero(diff)])
    return got[0], rows


@pytest.mark.parametrize("l1,l2", [(3, 3), (2, 5), (8, 8)])
@pytest.mark.parametrize("mode", MODES)
def test_ragged_batch(pkg, mode, l1, l2):
    assert (sub_tile_fits(3, 3), sub_tile_fits(2, 5), sub_tile_fits(8, 8)) == (True, True, False)
    pcm, offs, lens = ragged_batch()
    got, rows = check(pkg, "ragged", mode, pcm, offs, lens, l1=l1, l2=l2)
    assert got.shape[0] == sum(RAGGED_FRAMES) + 30 + 40
    t0 = rows[len(RAGGED_FRAMES) + 2]
    assert not got[t0:t0 + 40, 13:].any(), "whole tone periods per shift: delta and delta-delta are exactly 0"
    assert np.isfinite(got).all()


@pytest.mark.parametrize("mode", MODES)
def test_fewer_tiles_than_blocks_fewer_chunks_than_waves(pkg, mode):
    """3 utterances of 40 frames: every front-end wave is idle at once, most blocks have no tile"""
    pcm, offs, lens = pack([synth_utterance(samples(40), 430 + i) for i in range(3)])
    check(pkg, "three_short", mode, pcm, offs, lens)


@pytest.mark.parametrize("mode", MODES)
def test_one_long_utterance(pkg, mode):
    """4000 frames in one utterance: about a block's worth of rows per block at full size, here spread thin -- head and tail
    meet inside every block that has more than one tile, and under share_all the claims alone order the work"""
    pcm, offs, lens = pack([synth_utterance(samples(4000), 440)])
    check(pkg, "one_long", mode, pcm, offs, lens)


@pytest.mark.parametrize("cfg", [dict(ceps=13), dict(ceps=16), dict(ceps=13, dyn=1)], ids=["39", "48", "26"])
@pytest.mark.parametrize("mode", ("share", "share_all"))
def test_row_widths(pkg, mode, cfg):
    pcm, offs, lens = ragged_batch()
    got, _ = check(pkg, "ragged", mode, pcm, offs, lens, **cfg)
    assert got.shape[1] == cfg["ceps"] * (2 if cfg.get("dyn") == 1 else 3)


@pytest.mark.parametrize("mode", ("share", "share_all"))
def test_two_runs_on_one_handle(pkg, mode):
    """s_done and the claim word are set up by every launch"""
    pcm, offs, lens = pack([synth_utterance(samples(t), 450 + i) for i, t in enumerate((700, 129, 64, 1500))])
    check(pkg, "two_runs", mode, pcm, offs, lens, runs=2)


def test_default_gate(pkg):
    """No engine bit: a batch just under the library's lower threshold takes the two kernels, one at it the fused form with
    shared tiles; a plan just over the upper threshold does not fuse.  10-frame utterances keep the batches small; the rows
    of the larger batch are the two-kernel bits."""
    torch, dev = torch_dev()
    probe = handle(pkg, "default")
    min_frames = probe.batch_fuse_info()[3]
    probe.close()
    assert min_frames % 10 == 0 and min_frames > 299400     # above the largest batch the older suites run (300 x 998 frames)
    n_over, n = min_frames // 10, samples(10)
    g = torch.Generator(device=dev)
    g.manual_seed(77)
    d_pcm = (3000.0 * torch.randn((n_over * n + 8,), device=dev, generator=g)).round().clamp(-32768, 32767).to(torch.int16)
    res = {}
    for mode, n_utt in (("default", n_over - 1), ("default", n_over), ("two_kernels", n_over)):
        m = handle(pkg, mode)
        rows, total = m.batch_plan(np.arange(n_utt, dtype=np.int64) * n, np.full(n_utt, n, np.int64))
        assert total == 10 * n_utt
        out = OutPlacement(total, 39, 0, device=dev)
        torch.cuda.synchronize()
        m.batch_run_device(d_pcm.data_ptr(), d_pcm.numel(), out.ptr)
        m.synchronize()
        res[(mode, n_utt)] = (out.check("%s, %d utterances" % (mode, n_utt)), m.batch_fuse_info())
        m.close()
    # the upper side of the gate, from the plan alone (nothing is run): the fused form loses on very long batches
    max_frames = res[("default", n_over)][1][4]
    assert max_frames % 10 == 0 and max_frames >= 998000                  # the headline batch is inside the gate
    m = handle(pkg, "default")
    for n_utt, want in ((max_frames // 10, True), (max_frames // 10 + 1, False)):
        m.batch_plan(np.arange(n_utt, dtype=np.int64) * n, np.full(n_utt, n, np.int64))
        assert m.batch_fuse_info()[0] is want, "%d frames" % (10 * n_utt)
    m.close()
    assert res[("default", n_over - 1)][1][:3] == (False, 1, 0), "a batch under the threshold fused"
    assert res[("default", n_over)][1][:3] == (True, 1, 1), "a batch at the threshold did not fuse"
    assert res[("two_kernels", n_over)][1][0] is False and res[("two_kernels", n_over)][1][2] == 0
    a, b = res[("default", n_over)][0], res[("two_kernels", n_over)][0]
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    under = res[("default", n_over - 1)][0]
    assert torch.equal(under.view(torch.int32), b[:under.shape[0]].view(torch.int32))
