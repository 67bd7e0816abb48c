"""Cases of tests/test_attach_bits_gpu.py, shared with tests/golden/make_attach_bits_parent.py (which recorded what commit
da4d973 gives: the last one before the attachments of a planned batch got one utterance tiling for host and kernels).  One
small ragged batch per case on the C2 shape (tail_bits_cases.W / S, 40 filters, 13 cepstra, deltas and accelerations), its
utterance lengths on, before and behind the item edges of the tiling the case is there for, through the device entry:

    VAD               tiles of 64 rows, chunks of 4096    FLAGS, SELECT and PACK, frames_context 0 and 5
    online normaliser chunks of 32 rows                   windows 0 and 32, CMN and CVN
    pitch track       tiles of tile_frames() frames       a lag range a wave takes two frames of at a time, and one it takes one of
    pitch features    tiles of 256 rows                   paste off and on, and a window that reaches across a whole tile
    speakers          chunks of 4096 rows                 CVN pooled over two speakers
    combined          pasted pitch features, the online normaliser and a selecting VAD in force together

`record(pkg, name)` returns what the fixture holds for a case, name -> array: every row-indexed float array as the bit patterns
of the rows of its utterances of at most FULL_ROWS rows (tail_bits_cases.shortest_bits) and an 8-byte digest of every row
(tail_bits_cases.digests); every integer array and every per-utterance array whole."""
import ctypes as C

import numpy as np

import tail_bits_cases as TC
from conftest import synth_utterance

CMN, CVN = TC.CMN, TC.CVN
FLAGS, SELECT, PACK = 0, 1, 2            # MFX_VAD_*
FULL_ROWS = 129                          # utterances up to this many rows are held in full, the others by their digests
PITCH_SPAN_MAX = 24576                   # kPitchSpanMax (mfx_tables.h)


def tile_frames(lag_max, window=TC.W, shift=TC.S):
    """pitch_tile_frames (mfx_tables.cpp): frames per tile of k_pitch_nccf, 64 unless the tile's padded PCM span is too long."""
    pad = (2 - shift) & 63 if shift >= 64 else 0
    f = 64
    while f > 1:
        last = (f - 1) * shift + window + lag_max - 1
        if last + pad * (last // shift) + 1 <= PITCH_SPAN_MAX:
            break
        f -= 1
    return f


def pitch_groups(lag_min, lag_max):
    """pitch_groups (mfx_pitch.hip): frames a wave of k_pitch_nccf takes at a time."""
    lags = lag_max - (lag_min & ~3) + 1
    return 2 if 2 * ((lags + 255) // 256) > (lags + 127) // 128 else 1


def _pitch_frames(lag_max):
    tf = tile_frames(lag_max)
    return (1, tf - 1, tf, tf + 1, 2 * tf + 1)


def _c(frames, norm=TC.NORM_NONE, vad=None, onorm=None, pitch=None, feats=None, speakers=None, hold=None):
    """hold: the arrays of run_case the fixture keeps for the case (None: all of them)."""
    return dict(frames=tuple(frames), norm=norm, vad=vad, onorm=onorm, pitch=pitch, feats=feats, speakers=speakers, hold=hold)


def _vad(mode, ctx):
    return dict(column=-1, energy_threshold=0.0, energy_mean_scale=1.0, frames_context=ctx, proportion_threshold=0.6, mode=mode)


def _pitch(lag_min, lag_max, max_jump):
    return dict(lag_min=lag_min, lag_max=lag_max, window=0, ballast=1e-3, lag_cost=0.1, penalty=0.1, max_jump=max_jump)


VAD_FRAMES = (1, 0, 63, 64, 65, 129, 4097)
ONORM_FRAMES = (0, 1, 31, 32, 33, 65, 97)
FEAT_FRAMES = (1, 255, 256, 257, 513)
SPK_FRAMES = (1, 4096, 4097, 8200)
P2, P1 = _pitch(40, 160, 0), _pitch(40, 280, 20)      # 121 lags: two frames per wave; 241 lags: one
CASES = {
    "vad_flags_ctx0": _c(VAD_FRAMES, vad=_vad(FLAGS, 0)),
    "vad_flags_ctx5": _c(VAD_FRAMES, vad=_vad(FLAGS, 5)),
    "vad_select_ctx0": _c(VAD_FRAMES, vad=_vad(SELECT, 0)),
    "vad_select_ctx5": _c(VAD_FRAMES, vad=_vad(SELECT, 5)),
    "vad_pack_ctx0": _c(VAD_FRAMES, vad=_vad(PACK, 0)),
    "vad_pack_ctx5": _c(VAD_FRAMES, vad=_vad(PACK, 5)),
    "onorm_cmn_w0": _c(ONORM_FRAMES, norm=CMN, onorm=0),
    "onorm_cmn_w32": _c(ONORM_FRAMES, norm=CMN, onorm=32),
    "onorm_cvn_w0": _c(ONORM_FRAMES, norm=CVN, onorm=0),
    "onorm_cvn_w32": _c(ONORM_FRAMES, norm=CVN, onorm=32),
    # (the rows of a run are not the pitch track's to change, nor the track the features': held where they are made)
    "pitch_two_groups": _c(_pitch_frames(160), pitch=P2, hold=("pitch", "index", "nccf")),
    "pitch_one_group": _c(_pitch_frames(280), pitch=P1, hold=("pitch", "index", "nccf")),
    "feats": _c(FEAT_FRAMES, pitch=P2, feats=dict(left=75, right=75, paste=False), hold=("feats",)),
    "feats_pasted": _c(FEAT_FRAMES, pitch=P2, feats=dict(left=75, right=75, paste=True), hold=("feats", "rows")),
    "feats_window_across_a_tile": _c(FEAT_FRAMES, pitch=P2, feats=dict(left=300, right=260, paste=False), hold=("feats",)),
    "speakers_cvn": _c(SPK_FRAMES, norm=CVN, speakers=(0, 1, 0, 1)),
    "combined": _c((1, 0, 33, 64, 65, 257, 300), norm=CMN, onorm=32, pitch=P2, feats=dict(left=75, right=75, paste=True),
                   vad=_vad(SELECT, 5)),
}


def _hip():
    """The HIP runtime this process already holds (libmfcchip.so is linked against it), for one device-to-host copy."""
    with open("/proc/self/maps") as f:
        for line in f:
            if "libamdhip64" in line:
                return C.CDLL(line.split()[-1])
    raise RuntimeError("no HIP runtime in this process")


def _device_int64(ptr, n):
    out = np.zeros(n, np.int64)
    hip = _hip()
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    assert hip.hipMemcpy(out.ctypes.data, C.c_void_p(ptr), out.nbytes, 2) == 0      # hipMemcpyDeviceToHost
    return out


def run_case(pkg, name):
    """The case through mfx_batch_run_device: name -> array, row-indexed arrays [total_rows][...] whole, and "utt_rows"."""
    import torch
    c = CASES[name]
    utts = [synth_utterance(TC.samples_for(f), 1300 + i) for i, f in enumerate(c["frames"])]
    pcm, offs, lens = TC.place(utts)
    m = TC.handle(pkg, dict(TC.C2, c0=False, norm=c["norm"], engine=0, method=TC.MFCC, lpc=0, L=0, K=0))
    try:
        rows, total = m.batch_plan(offs, lens)
        assert total == sum(c["frames"]) and list(np.diff(list(rows) + [total])) == list(c["frames"])
        if c["pitch"]:
            m.batch_set_pitch(**c["pitch"])
        if c["feats"]:
            m.batch_set_pitch_feats(**c["feats"])
        if c["onorm"] is not None:
            m.batch_set_online_norm(window=c["onorm"])
        if c["speakers"]:
            m.batch_set_speakers(np.asarray(c["speakers"], np.int32), 2)
        if c["vad"]:
            m.batch_set_vad(**c["vad"])
        width = m.batch_output_width()
        d_pcm = torch.from_numpy(pcm).to("cuda:0")
        d_out = torch.full((total, width), float("nan"), dtype=torch.float32, device="cuda:0")
        torch.cuda.synchronize()
        m.batch_run_device(d_pcm.data_ptr(), pcm.size, d_out.data_ptr())
        m.synchronize()
        out = {"utt_rows": np.asarray(rows, np.int64), "rows": d_out.cpu().numpy()}
        if c["vad"]:
            flags, voiced, thr, total_voiced = m.batch_vad_read()
            out.update(flags=flags, voiced=voiced, thr=thr.view(np.int32))
            out["packed_row0"] = _device_int64(m.batch_vad_device()[2], len(lens) + 1)
            assert out["packed_row0"][-1] == total_voiced
        if c["pitch"]:
            lag, rho, index, nccf = m.batch_pitch_read(nccf=True)
            out.update(pitch=np.stack([lag, rho], axis=1), index=index, nccf=nccf)
        if c["feats"]:
            out["feats"] = m.batch_pitch_feats_read()
        if c["speakers"]:
            count, acc, stats = m.batch_speaker_stats()
            out.update(spk_count=count, spk_acc=acc.view(np.int64), spk_stats=stats.view(np.int32))
        return out
    finally:
        m.close()


def _per_utterance(a, utt_rows, frames):
    return [np.ascontiguousarray(a[r:r + f]) for r, f in zip(utt_rows, frames)]


def record(pkg, name):
    """What the fixture holds for the case (see the module's docstring)."""
    c, out, rec = CASES[name], run_case(pkg, name), {}
    utt_rows = out.pop("utt_rows")
    for key, a in out.items():
        if c["hold"] and key not in c["hold"]:
            continue
        if a.dtype == np.float32 and a.ndim == 2 and a.shape[0] == sum(c["frames"]):     # rows, pitch, nccf, feats
            per = _per_utterance(a, utt_rows, c["frames"])
            rec[key + "__digests"] = TC.digests(per)
            if key != "nccf":                                                            # (of every NCCF row a digest, no more)
                rec[key + "__rows"] = TC.shortest_bits([g for g in per if len(g) <= FULL_ROWS])
        else:
            rec[key] = a
    return rec
