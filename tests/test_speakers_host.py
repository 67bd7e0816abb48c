"""Per-speaker normalisation of the batch entries (mfx_batch_set_speakers), the parts that need no GPU: the entries on a
planning handle, the list builder (mfx_host_speaker_lists: the lists k_spk_finish walks, built by the code that builds them for
upload), the host merge of the accumulators of several ranks, and the driver's label -> id mapping."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import spk_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("mfx_batch_set_speakers", "mfx_batch_speaker_stats", "mfx_host_speaker_lists")


def test_header_exports_and_prototypes_name_the_entries(pkg):
    header = open(os.path.join(ROOT, "include", "mfx.h")).read()
    L = pkg.load_library()
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, header)
        assert name in pkg.mfcc.EXPORTED_SYMBOLS
        assert getattr(L, name).argtypes is not None
    assert re.search(r"MFX_SPK_POOL\s*=\s*0\s*,\s*MFX_SPK_PRIOR_ONLY\s*=\s*1", header)
    assert (pkg.mfcc.SPK_POOL, pkg.mfcc.SPK_PRIOR_ONLY) == (0, 1)
    assert L.mfx_abi_version() == 2                          # functions are added, no struct changes
    assert len(L.mfx_batch_set_speakers.argtypes) == 7 and len(L.mfx_batch_speaker_stats.argtypes) == 4
    assert L.mfx_host_speaker_lists.restype is C.c_int64 and len(L.mfx_host_speaker_lists.argtypes) == 6


def test_the_entries_on_a_planning_handle_are_device_errors(pkg):
    L = pkg.load_library()
    cfg = pkg.mfcc.MfxConfig(100 * 160 + 400, 400, 160, 40, 16000.0, 64.0, 8000.0, 13, 0, 22.0, 2, 2, 3, 3, 1, 0, 1, 1, 0, 0, 0)
    h = C.c_void_p()
    assert L.mfx_plan_create(C.byref(cfg), C.byref(h)) == 0
    try:
        ids = np.zeros(1, np.int32)
        assert L.mfx_batch_set_speakers(h, ids.ctypes.data_as(C.POINTER(C.c_int32)), 1, 1, None, None, 0) == -6   # MFX_ERR_DEVICE
        assert b"planning handle" in L.mfx_last_error(h)
        assert L.mfx_batch_set_speakers(h, None, 0, 0, None, None, 0) == -6
        assert L.mfx_batch_speaker_stats(h, None, None, None) == -6
    finally:
        L.mfx_destroy(h)


def lists(pkg, ids, frames, n_spk):
    off, lst = pkg.mfcc.host_speaker_lists(ids, frames, n_spk)
    want_off, want_lst = spk_ref.host_lists_ref(ids, frames, n_spk)
    assert off.dtype == np.int32 and lst.dtype == np.int32
    assert off.tolist() == want_off.tolist() and lst.tolist() == want_lst.tolist(), (ids, frames)
    return off.tolist(), lst.tolist()


def test_lists_interleaved_ids_empty_speakers_frameless_utterances(pkg):
    off, lst = lists(pkg, [0, 1, 2, 0, 2, 1, 0, 1, 2, 0, 2, 1], [1, 2, 7, 64, 65, 200, 4097, 8200, 0, 33, 129, 300], 4)
    assert off == [0, 4, 8, 11, 11]                          # speaker 2 owns the frameless utterance 8; speaker 3 owns nothing
    assert lst == [0, 3, 6, 9, 1, 5, 7, 11, 2, 4, 10]
    off, lst = lists(pkg, [3, 3, 0], [5, 0, 0], 5)           # speakers whose every utterance is frameless own nothing either
    assert off == [0, 0, 0, 0, 1, 1] and lst == [0]
    off, lst = lists(pkg, [], [], 3)
    assert off == [0, 0, 0, 0] and lst == []
    off, lst = lists(pkg, [0, 0, 0], [0, 0, 0], 1)
    assert off == [0, 0] and lst == []
    rng = np.random.default_rng(7)
    for n_spk in (1, 2, 17, 300):
        n = 500
        lists(pkg, rng.integers(0, n_spk, size=n), rng.choice([0, 0, 1, 5, 64, 4097], size=n), n_spk)


def test_lists_refuse_an_id_outside_the_range(pkg):
    for ids, n_spk in (([0, 2], 2), ([-1, 0], 2), ([0], 0)):
        with pytest.raises(pkg.MfxError) as e:
            pkg.mfcc.host_speaker_lists(ids, [3] * len(ids), n_spk)
        assert e.value.status == -7
    L = pkg.load_library()                                   # either output may be NULL: the length alone
    ids, fr = np.array([1, 0, 1], np.int32), np.array([2, 0, 9], np.int64)
    assert L.mfx_host_speaker_lists(3, ids.ctypes.data_as(C.POINTER(C.c_int32)), fr.ctypes.data_as(C.POINTER(C.c_int64)), 2, None, None) == 2


def test_merge_speaker_acc_against_numpy(pkg):
    rng = np.random.default_rng(11)
    n_spk, Wn = 5, 39
    parts = []
    for r in range(3):
        count = rng.integers(0, 5000, size=n_spk)
        acc = rng.standard_normal((n_spk, 4, Wn)) * 1e3
        acc[:, 1] = np.abs(acc[:, 1])
        absent = count == 0
        count[1 if r == 1 else 3] = 0                        # a speaker a rank has no rows of: the kernel's neutral elements
        absent = count == 0
        acc[absent, 0], acc[absent, 1] = 0.0, 0.0
        acc[absent, 2], acc[absent, 3] = np.float64(np.float32(3.402823466e+38)), -np.float64(np.float32(3.402823466e+38))
        parts.append((count.astype(np.int64), acc))
    count, acc = pkg.sharding.merge_speaker_acc(parts)
    want_count, want_acc = spk_ref.merge_ref(parts)
    assert count.dtype == np.int64 and acc.dtype == np.float64 and acc.shape == (n_spk, 4, Wn)
    assert np.array_equal(count, want_count)
    assert np.array_equal(acc[:, 2:], want_acc[:, 2:])       # min / max: exact
    # ascending rank order, from rank 0's values as they are: ((a0 + a1) + a2), the same doubles as numpy's fold over 3 ranks
    assert np.array_equal(acc[:, :2], (parts[0][1][:, :2] + parts[1][1][:, :2]) + parts[2][1][:, :2])
    assert np.allclose(acc[:, :2], want_acc[:, :2], rtol=1e-15, atol=0)
    one_c, one_a = pkg.sharding.merge_speaker_acc(parts[:1])
    assert np.array_equal(one_c, parts[0][0]) and np.array_equal(one_a, parts[0][1])
    one_a[0, 0, 0] += 1.0                                    # a copy: the caller's arrays are not touched
    assert one_a[0, 0, 0] != parts[0][1][0, 0, 0]
    with pytest.raises(ValueError):
        pkg.sharding.merge_speaker_acc([])
    with pytest.raises(ValueError):
        pkg.sharding.merge_speaker_acc([parts[0], (parts[1][0][:-1], parts[1][1][:-1])])


def exe_path():
    exe = os.path.join(ROOT, "asr-featext-opencl_amd", "host", "afet_hip")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", os.path.dirname(exe)])
    return exe


def test_driver_maps_labels_to_ids_by_first_appearance(pkg, tmp_path):
    f = tmp_path / "labels.txt"
    f.write_text("bob\nalice\n\n  bob  \ncarol\r\nalice\nBob\n")
    r = subprocess.run([exe_path(), "--selftest-spk-labels", str(f)], stdout=subprocess.PIPE, text=True)
    assert r.returncode == 0
    assert r.stdout.strip() == "4 speakers: 0 1 0 2 1 3"     # blank lines skipped, white space dropped, case kept
    assert subprocess.run([exe_path(), "--selftest-spk-labels", str(tmp_path / "missing.txt")], stderr=subprocess.DEVNULL).returncode == 2


def test_driver_refuses_spk_file_without_what_it_needs(pkg, tmp_path):
    """The refusals that are decided before any device is touched."""
    wav = os.path.join(ROOT, "tests", "golden", "a0001.wav")
    one = tmp_path / "one.txt"
    one.write_text("alice\n")
    files = [wav, str(tmp_path / "a.out")]

    def run(extra):
        r = subprocess.run([exe_path()] + extra + files, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True)
        return r.returncode, r.stderr

    rc, err = run(["--spk-file", str(one), "--norm", "0"])
    assert rc == 2 and "--norm" in err
    rc, err = run(["--spk-file", str(one), "--batch-mb", "0"])
    assert rc == 2 and "--batch-mb" in err
    rc, err = run(["--spk-file", str(one), "--devs", "0,1"])
    assert rc == 2 and "one device" in err
    two = tmp_path / "two.txt"
    two.write_text("alice\nbob\n")
    rc, err = run(["--spk-file", str(two)])
    assert rc == 2 and "2 labels for 1 input files" in err
    rc, err = run(["--spk-file", str(tmp_path / "missing.txt")])
    assert rc == 2
