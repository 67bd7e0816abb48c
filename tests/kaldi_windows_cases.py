"""What tests/test_kaldi_windows_host.py (CPU) and tests/test_kaldi_windows_gpu.py share: the shape matrix of the Kaldi front end
beyond the Povey window, the seeded faults of the frame-start rule and the end taps as variations of the float64 oracle
(tests/kaldi_ref.py), a float32 restatement of the pipeline on the CPU, and the rule that says in which domain an edge signal is
held under a window.  Test infrastructure only; nothing here needs a device."""
import numpy as np

import kaldi_ref as KR
import vad_ref as VR
from conftest import TOL_L2, TOL_MAX, synth_utterance
from kaldi_drive import MFCC13, Shape

NEW_WINDOWS = ("hamming", "rect", "ramp")

# W / S / M / C (low 20, high 0, Q 22)
MATRIX = (
    Shape(400, 160, 80, 0),
    Shape(400, 160, 23, 13),
    Shape(257, 100, 40, 0),                    # odd W just over 256: the i1 < W guard at N = 512
    Shape(256, 64, 40, 13),                    # W = N: no zero padding
    Shape(129, 40, 23, 13, sr=8000.0),         # odd W just over 128
    Shape(128, 32, 23, 0, sr=8000.0),          # W = N = 128
    Shape(400, 8, 40, 0),                      # log-mel rows 640 > span 520
    Shape(128, 4, 64, 20),                     # rows 1024 > span 188; 7 empty bands feed the DCT
    Shape(65, 1, 64, 0),                       # S = 1 (rows 1024 > span 80)
)
ROWS_OUTGROW_THE_SPAN = ("400-8-40-0", "128-4-64-20", "65-1-64-0")
CHUNK = 16                                     # frames of a block of k_kaldi_front at most


def under(sh, window):
    return sh.options(window=window)


def shape_utterances(sh):
    """The two utterances of a shape as tests/test_kaldi_gpu.py builds them (restated, so that no CPU module imports a GPU test
    module): 45 frames and a remainder -- two full chunks and a cut one --, and 3 frames (4 at S = 1, where the remainder is a
    hop)."""
    return [synth_utterance(sh.W + 44 * sh.S + sh.S // 2, 11, sr=sh.sr), synth_utterance(sh.W + 2 * sh.S + 1, 12, sr=sh.sr)]


def utterance(sh):
    return shape_utterances(sh)[0]


def rows(sh, pcm, taps=None, predecessor=KR.PRED_FIRST, energies=False):
    """Shape.oracle with the taps and the frame-start predecessor open to a seeded fault."""
    return KR.features(pcm, sh.taps() if taps is None else taps, sh.S, sh.M, sh.sr, sh.low, sh.high, sh.C, sh.Q, sh.preemph, sh.remove_dc,
                       sh.use_power, energies=energies, predecessor=predecessor)


def _zeroed(w, i):
    w = w.copy()
    w[i] = 0.0
    return w


# name -> (sh, pcm) -> the rows of a kernel with that fault
FAULTS = {
    "a: predecessor 0": lambda sh, pcm: rows(sh, pcm, predecessor=KR.PRED_ZERO),
    "b: predecessor from in front of the frame": lambda sh, pcm: rows(sh, pcm, predecessor=KR.PRED_BEFORE),
    "c: tap W - 1 dropped": lambda sh, pcm: rows(sh, pcm, taps=_zeroed(sh.taps(), -1)),
    "d: tap 0 dropped": lambda sh, pcm: rows(sh, pcm, taps=_zeroed(sh.taps(), 0)),
    "e: window mirrored": lambda sh, pcm: rows(sh, pcm, taps=sh.taps()[::-1].copy()),
}
# the pairings every shape of MATRIX must give power to: fault -> windows
REQUIRED = {
    "a: predecessor 0": NEW_WINDOWS,
    "b: predecessor from in front of the frame": NEW_WINDOWS,
    "c: tap W - 1 dropped": NEW_WINDOWS,
    "d: tap 0 dropped": ("rect",),
    "e: window mirrored": ("ramp",),
}
POWER = 10.0 * TOL_MAX


def moved(faulty, want):
    """max |faulty - oracle| / max |oracle|: the first figure of conftest.assert_close."""
    return float(np.abs(faulty - want).max() / np.abs(want).max())


# ---- the pipeline in float32 ---------------------------------------------------------------------------------------------------

def restate32(sh, pcm, energies=False):
    """The definition with every operation in float32, on the CPU: float32 mean, one-rounding pre-emphasis, window product, torch's
    float32 rfft, float32 tables, mel product, log and DCT.  Not the kernel's instruction stream: another float32 evaluation of
    the same formula, whose distance to the float64 oracle says how much of the bar rounding alone may take."""
    import torch
    pcm = np.asarray(pcm, np.int16)
    w = sh.taps()
    W, S, M = sh.W, sh.S, sh.M
    N = KR.fft_size(W)
    T = KR.frame_count(pcm.size, W, S)
    cols = M if (sh.C == 0 or energies) else sh.C
    if T == 0:
        return np.zeros((0, cols), np.float32)
    xi = pcm[np.arange(T)[:, None] * S + np.arange(W)[None, :]].astype(np.int64)
    d = xi.astype(np.float32)
    if sh.remove_dc:
        d = d - (xi.sum(axis=1).astype(np.float32) / np.float32(W))[:, None]
    c = float(np.float32(sh.preemph))
    prev = np.concatenate([d[:, :1], d[:, :-1]], axis=1)
    e = (d.astype(np.float64) - c * prev.astype(np.float64)).astype(np.float32)     # (the product is exact in double: one rounding)
    z = np.zeros((T, N), np.float32)
    z[:, :W] = e * w[None, :]
    X = torch.fft.rfft(torch.from_numpy(z), dim=1).numpy()[:, :N // 2]
    assert X.dtype == np.complex64
    P = X.real * X.real + X.imag * X.imag
    if not sh.use_power:
        P = np.sqrt(P)
    E = (P @ KR.mel_table(M, N, sh.sr, sh.low, sh.high)[0].T).astype(np.float32)
    if energies:
        return E
    L = np.log(np.maximum(E, np.float32(KR.FLOOR))).astype(np.float32)
    if sh.C == 0:
        return L
    return (L @ KR.dct(M, sh.C, sh.Q).T).astype(np.float32)


def figures(got, want):
    """(max err / scale, rel L2): the two figures of conftest.assert_close."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return float(np.abs(got - want).max() / max(np.abs(want).max(), 1e-30)), float(np.linalg.norm(got - want) / max(np.linalg.norm(want), 1e-30))


# ---- edge signals ---------------------------------------------------------------------------------------------------------------

EDGE_SHAPE = MATRIX[0]
EDGE_WINDOWS = ("rect", "ramp")
ENERGY_BAR = 1e-4                              # of the frame's largest mel energy: the bar of tests/test_kaldi_gpu.py
ENERGY_SIGNALS = ("tone", "lsb", "ramp", "square", "constant, DC kept")
ROOM = 5.0


def edge_signals():
    """The seven signals of tests/test_kaldi_gpu.py at 400 / 160 (restated): 20 frames and a remainder each."""
    n = EDGE_SHAPE.W + 19 * EDGE_SHAPE.S + 77
    t = np.arange(n)
    imp = np.zeros(n, np.int16)
    imp[n // 2] = 32767
    return {
        "tone": np.round(32767.0 * np.sin(2 * np.pi * 1000.0 * t / 16000.0)).astype(np.int16),
        "lsb": np.where(t % 2 == 0, 1, -1).astype(np.int16),
        "ramp": (t * 3 - 4000).astype(np.int16),
        "square": np.where((t // 8) % 2 == 0, 32767, -32768).astype(np.int16),
        "impulse": imp,
        "constant": np.full(n, 12345, np.int16),
        "silence": np.zeros(n, np.int16),
    }


def edge_cases():
    """name -> (pcm, DC removal): the seven signals, and the constant with DC removal off."""
    sig = edge_signals()
    out = {k: (v, True) for k, v in sig.items()}
    out["constant, DC kept"] = (sig["constant"], False)
    return out


def energy_err(got_log, want_energies):
    """Worst |exp(row) - energy| over the frame's largest energy (the floor applied to the energies, as the rows have it)."""
    want = np.maximum(want_energies, KR.FLOOR)
    e = np.exp(np.asarray(got_log, np.float64))
    return float((np.abs(e - want) / want.max(axis=1, keepdims=True)).max())


_EDGE_PLAN = {}


def edge_plan():
    """(signal, window) -> (how it is held, the float32 restatement's figure there), computed once on the CPU:
      "floor"   constant and silence under DC removal: d = 0 exactly, every element is the floor value;
      "log"     the project bar in the log domain;
      "energy"  ENERGY_BAR of the frame's largest energy -- kept only where the restatement stays ROOM x under it;
      "none"    fits neither bar with ROOM x to spare: listed, not held.
    A signal of ENERGY_SIGNALS that leaves no room in the energy domain falls back to the log domain if it has the room there."""
    if _EDGE_PLAN:
        return _EDGE_PLAN
    for window in EDGE_WINDOWS:
        for name, (pcm, dc) in edge_cases().items():
            sh = under(EDGE_SHAPE, window).options(remove_dc=dc)
            if name in ("constant", "silence"):
                _EDGE_PLAN[(name, window)] = ("floor", 0.0)
                continue
            r32 = restate32(sh, pcm)
            log_fig = figures(r32, rows(sh, pcm))
            en_fig = energy_err(r32, rows(sh, pcm, energies=True))
            log_fits = log_fig[0] * ROOM <= TOL_MAX and log_fig[1] * ROOM <= TOL_L2
            if name in ENERGY_SIGNALS and en_fig * ROOM <= ENERGY_BAR:
                _EDGE_PLAN[(name, window)] = ("energy", en_fig)
            elif log_fits:
                _EDGE_PLAN[(name, window)] = ("log", log_fig[0])
            else:
                _EDGE_PLAN[(name, window)] = ("none", min(en_fig / ENERGY_BAR, log_fig[0] / TOL_MAX))
    return _EDGE_PLAN


# ---- the composition module's inputs (tests/test_kaldi_compose_gpu.py) ------------------------------------------------------------

COMP_SHAPE = MFCC13.options(window="ramp")
COMP_FRAMES = [71, 17, 3, 0]
COMP_LENGTHS = [400 + 70 * 160 + 9, 400 + 16 * 160, 400 + 2 * 160 + 5, 300]
VAD = (0.0, 1.0, 2, 0.6)                       # energy_threshold, energy_mean_scale, frames_context, proportion_threshold


def comp_utts():
    """The utterances of test_kaldi_gpu's composition tests."""
    return [synth_utterance(n, 401 + i) for i, n in enumerate(COMP_LENGTHS)]


def enveloped():
    """comp_utts under the gain envelope of test_tensor_gpu.mfcc39_batch: every second run of 25 frames is 48 dB down."""
    out = []
    for u in comp_utts():
        seg = u.astype(np.float64)
        seg[(np.arange(u.size) // (160 * 25)) % 2 == 1] /= 256.0
        out.append(np.round(seg).astype(np.int16))
    return out


def vad_input_condition():
    """vad_ref's condition on the input, on the CPU: on the long utterance between 20 % and 80 % of the frames are voiced for
    c0 (column 0) and for the default column (the last static one), and the two decisions differ."""
    u = enveloped()[0]
    rows = COMP_SHAPE.oracle(u).astype(np.float32)
    flags = {}
    for col in (0, 12):
        e = rows[:, col]
        flags[col] = VR.flags_ref(e, np.float32(VR.thr_ref(e, VAD[0], VAD[1])[0]), VAD[2], VAD[3])
        share = flags[col].mean()
        print("column %d: %.2f of the %d frames voiced" % (col, share, e.size))
        assert 0.2 <= share <= 0.8, (col, share)
    assert not np.array_equal(flags[0], flags[12])
