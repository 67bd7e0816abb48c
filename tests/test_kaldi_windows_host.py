"""CPU tests behind tests/test_kaldi_windows_gpu.py: that its inputs have power, and why the first suite's had none.

Every test of tests/test_kaldi_gpu.py runs under the Povey window, whose taps 0 and W - 1 are exactly 0.0f.  Three parts of the
definition of include/mfx.h therefore cannot move a row there: the frame-start rule e[0] = fmaf(-c, d[0], d[0]), whether tap 0
and tap W - 1 are read at all, and the i1 < W guard of an odd W; and since every window in use was symmetric, neither could a
window indexed from the wrong end.  Here each of these is seeded as a fault into the float64 oracle (tests/kaldi_ref.py) --
  a  the predecessor of the frame's first sample taken as 0,
  b  ... taken from in front of the frame (x[t S - 1] - mean: what a session path that carries context would do naturally),
  c  tap W - 1 dropped,   d  tap 0 dropped,   e  the window mirrored --
and measured as max |faulty - oracle| / max |oracle| on shape_utterances(sh)[0], for every shape of MATRIX
(tests/kaldi_windows_cases.py).  The condition on the inputs: a, b, c under hamming, rect and ramp, d under rect and e under
ramp reach at least 10 x TOL_MAX = 1e-3 at every shape; under Povey a .. d are exactly 0.0.  (d under hamming falls short: tap
0 is 0.08 and pre-emphasis leaves e[0] = 0.03 d[0]; it is required under rect only.)

The float32 restatement of the pipeline (kaldi_windows_cases.restate32) against the float64 oracle at every shape and new window
keeps the GPU comparison at the unchanged project bar honest: it must leave at least 5 x of room.  The same restatement decides,
per edge signal and window, in which domain the GPU test holds it (kaldi_windows_cases.edge_plan); the table is printed here.

Agreement with a Kaldi or torchaudio binary remains unmeasured: the oracle is the formula of include/mfx.h."""
import ctypes as C

import numpy as np
import pytest

import kaldi_ref as KR
import kaldi_windows_cases as KC
from conftest import TOL_L2, TOL_MAX
from kaldi_drive import Shape
from test_kaldi_host import config

IDS = [s.id() for s in KC.MATRIX]


def test_window_builders():
    for W in (65, 128, 257, 400):
        h, r, p = KR.hamming_window(W), KR.rect_window(W), KR.ramp_window(W)
        assert h.dtype == r.dtype == p.dtype == np.float32 and h.shape == r.shape == p.shape == (W,)
        assert abs(float(h[0]) - 0.08) < 1e-7 and abs(float(h[-1]) - 0.08) < 1e-7
        assert np.abs(h.astype(np.float64) - h[::-1]).max() < 1e-7 and abs(float(h.max()) - 1.0) < 2e-4
        assert (r == 1.0).all()
        assert float(p[-1]) == 1.0 and abs(float(p[0]) - (0.2 + 0.8 / W)) < 1e-7 and (np.diff(p) > 0).all()
        assert KR.povey_window(W)[0] == 0.0 and KR.povey_window(W)[-1] == 0.0
    assert abs(float(KR.hamming_window(400)[200]) - (0.54 - 0.46 * np.cos(2 * np.pi * 200 / 399))) < 1e-7
    assert set(KR.WINDOWS) == {"povey", "hamming", "rect", "ramp"}
    sh = Shape(400, 160, 80, 0, window="ramp")
    assert np.array_equal(sh.taps(), KR.ramp_window(400)) and sh.options(preemph=0.0).window == "ramp"
    assert np.array_equal(Shape(400, 160, 80, 0).taps(), KR.povey_window(400))            # the default is the first suite's


def test_predecessor_keyword_defaults_to_the_definition():
    sh = KC.under(KC.MATRIX[0], "rect")
    pcm = KC.utterance(sh)
    assert np.array_equal(KC.rows(sh, pcm), sh.oracle(pcm))
    assert np.array_equal(KC.rows(sh, pcm, predecessor=KR.PRED_FIRST), sh.oracle(pcm))
    # frame 0 has nothing in front of it: the "in front of the frame" fault is the definition there, and only there
    b = KC.rows(sh, pcm, predecessor=KR.PRED_BEFORE)
    assert np.array_equal(b[0], sh.oracle(pcm)[0]) and not np.array_equal(b[1], sh.oracle(pcm)[1])


@pytest.mark.parametrize("sh", KC.MATRIX, ids=IDS)
def test_matrix_shapes_are_planned_on_the_kaldi_kernel(pkg, sh):
    L = pkg.load_library()
    h = C.c_void_p()
    rc = L.mfx_plan_create(C.byref(config(pkg, W=sh.W, S=sh.S, M=sh.M, C_=sh.C, sr=sh.sr, low=sh.low, high=sh.high, Q=sh.Q)), C.byref(h))
    assert rc == 0, sh.id()
    try:
        assert L.mfx_dominant_kernel_name(h).decode() == "k_kaldi_front"
        assert L.mfx_fft_size(h) == KR.fft_size(sh.W)
    finally:
        L.mfx_destroy(h)
    N = KR.fft_size(sh.W)
    w, beg, ln = KR.mel_table(sh.M, N, sh.sr, sh.low, sh.high)
    assert int(ln.sum()) <= N                                    # the staged mel weights: a bin lies in two bands at most
    lds = pkg.host_kaldi_lds_bytes(sh.W, sh.S, sh.M, sh.C)
    # the two 400 / 160 shapes are the first suite's (44 992 bytes at fbank-80: three blocks per CU); the seven new ones stay
    # under 41 KB
    assert 0 < lds < (48 if (sh.W, sh.S) == (400, 160) else 41) * 1024
    span, rows = (KC.CHUNK - 1) * sh.S + sh.W, KC.CHUNK * sh.M
    if sh.id() in KC.ROWS_OUTGROW_THE_SPAN:
        assert rows > span, "%s no longer has its log-mel rows outgrow the staged span (%d <= %d)" % (sh.id(), rows, span)
    else:
        assert rows <= span
    print("%s: N %d, mel spans sum %d, LDS %d bytes, rows %d vs span %d, empty bands %d" % (sh.id(), N, ln.sum(), lds, rows, span, (ln == 0).sum()))


def test_matrix_covers_what_it_says():
    ids = set(IDS)
    assert set(KC.ROWS_OUTGROW_THE_SPAN) <= ids and len(KC.MATRIX) == 9
    assert {s.W for s in KC.MATRIX} >= {128, 129, 256, 257, 400} and any(s.S == 1 for s in KC.MATRIX)
    assert {KR.fft_size(s.W) for s in KC.MATRIX} == {128, 256, 512}
    sh = next(s for s in KC.MATRIX if s.id() == "128-4-64-20")
    assert int((KR.mel_table(sh.M, 128, sh.sr, sh.low, sh.high)[2] == 0).sum()) == 7


@pytest.mark.parametrize("sh", KC.MATRIX, ids=IDS)
def test_seeded_faults_move_the_rows_under_the_new_windows_and_not_under_povey(sh):
    for window in ("povey",) + KC.NEW_WINDOWS:
        s = KC.under(sh, window)
        pcm = KC.utterance(s)
        assert pcm.size == sh.W + 44 * sh.S + sh.S // 2
        want = s.oracle(pcm)
        assert want.shape == (45, sh.cols)
        for fault, f in KC.FAULTS.items():
            fig = KC.moved(f(s, pcm), want)
            print("%-12s %-8s %-45s moves the rows by %.3g of scale" % (sh.id(), window, fault, fig))
            if window == "povey":
                if not fault.startswith("e"):
                    assert fig == 0.0, "%s under Povey: %s is visible (%.3g)" % (sh.id(), fault, fig)
            elif window in KC.REQUIRED[fault]:
                assert fig >= KC.POWER, "%s under %s: %s moves the rows by %.3g < %.3g" % (sh.id(), window, fault, fig, KC.POWER)


def test_symmetric_windows_cannot_see_a_mirrored_window():
    """Povey, Hamming and the rectangular window are their own mirror images up to the last bit of a tap: fault e moves nothing
    that the bar could see; under the ramp it moves the rows by more than a tenth of the scale."""
    sh = KC.MATRIX[0]
    for window in ("povey", "hamming", "rect"):
        s = KC.under(sh, window)
        pcm = KC.utterance(s)
        fig = KC.moved(KC.FAULTS["e: window mirrored"](s, pcm), s.oracle(pcm))
        print("%s: mirrored window moves the rows by %.3g of scale" % (window, fig))
        assert fig < TOL_MAX / 100
    s = KC.under(sh, "ramp")
    pcm = KC.utterance(s)
    assert KC.moved(KC.FAULTS["e: window mirrored"](s, pcm), s.oracle(pcm)) > 0.1


def test_float32_restatement_leaves_room_under_the_project_bar():
    worst = (0.0, 0.0, "")
    for sh in KC.MATRIX:
        for window in KC.NEW_WINDOWS:
            s = KC.under(sh, window)
            pcm = KC.utterance(s)
            emax, el2 = KC.figures(KC.restate32(s, pcm), s.oracle(pcm))
            print("%-12s %-8s float32 restatement: %.3g of scale, %.3g rel L2 (room %.1fx, %.1fx)" % (sh.id(), window, emax, el2, TOL_MAX / emax,
                                                                                                      TOL_L2 / el2))
            assert emax * KC.ROOM <= TOL_MAX and el2 * KC.ROOM <= TOL_L2, (sh.id(), window, emax, el2)
            if emax > worst[0]:
                worst = (emax, el2, "%s %s" % (sh.id(), window))
    print("float32 restatement, worst: %.3g of scale, %.3g rel L2 at %s" % worst)


def test_vad_input_of_the_composition_module_meets_vad_refs_condition():
    """tests/test_kaldi_compose_gpu.py: between 20 % and 80 % of the long utterance's frames voiced, on c0 and on the default
    column, from the oracle's rows; the two columns decide differently."""
    KC.vad_input_condition()


def test_edge_signal_plan_and_its_room():
    """The room table of the edge signals under rect and ramp: which bar holds which pair on the GPU, from the float32
    restatement's figure alone.  At most one of the sixteen pairs may be left not held."""
    plan = KC.edge_plan()
    assert len(plan) == 16
    for (name, window), (how, fig) in sorted(plan.items()):
        bar = {"floor": 0.0, "log": TOL_MAX, "energy": KC.ENERGY_BAR, "none": 1.0}[how]
        print("%-18s %-5s held: %-6s restatement %.3g (bar %.3g)" % (name, window, how, fig, bar))
        if how in ("log", "energy"):
            assert fig * KC.ROOM <= bar
    for window in KC.EDGE_WINDOWS:
        assert plan[("constant", window)][0] == plan[("silence", window)][0] == "floor"
        assert plan[("impulse", window)][0] == "log"
    not_held = [k for k, v in plan.items() if v[0] == "none"]
    assert len(not_held) <= 1, not_held
    # d = 0 exactly for a constant frame under DC removal, whatever the window: the oracle's rows are the floor
    for window in KC.EDGE_WINDOWS:
        for name in ("constant", "silence"):
            pcm, dc = KC.edge_cases()[name]
            assert (KC.under(KC.EDGE_SHAPE, window).oracle(pcm) == KR.SILENCE).all()


def test_restated_inputs_are_the_first_suites():
    """kaldi_windows_cases restates the utterances, the edge signals and the energy bar of tests/test_kaldi_gpu.py, so that the
    CPU modules depend on no GPU test module; here the copies are held to the originals."""
    import test_kaldi_gpu as G
    assert KC.ENERGY_BAR == G.ENERGY_BAR
    for sh in KC.MATRIX:
        assert all(np.array_equal(a, b) for a, b in zip(KC.shape_utterances(sh), G.shape_utterances(sh)))
    a, b = KC.edge_signals(), G.edge_signals()
    assert list(a) == list(b) and all(np.array_equal(a[k], b[k]) for k in a)
