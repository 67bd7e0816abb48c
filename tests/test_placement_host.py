"""The placement checker (tests/placement.py) against fake writers on CPU tensors: it must see one float past the end, one
before the start, one element left unwritten and a write into the leading floats, and must pass an exact writer at every
4-byte position of d_out.  The GPU tests of tests/test_placement_gpu.py rest on it."""
import numpy as np
import pytest
import torch

from placement import GUARD, GUARD_BITS, INTERIOR_BITS, OutPlacement, PcmPlacement

ROWS, WIDTH = 37, 39


def exact(p):
    p.flat[p.start:p.start + p.n] = torch.arange(p.n, dtype=torch.float32)


def place(k):
    return OutPlacement(ROWS, WIDTH, k, device="cpu")


@pytest.mark.parametrize("k", [0, 1, 2, 3])
def test_exact_writer_passes(k):
    p = place(k)
    assert p.ptr == p.flat.data_ptr() + 4 * (GUARD + k) and (p.ptr - 4 * k) % 16 == 0
    exact(p)
    got = p.check("exact")
    assert got.shape == (ROWS, WIDTH)
    assert np.array_equal(got.numpy().reshape(-1), np.arange(ROWS * WIDTH, dtype=np.float32))
    assert p.all_finite()


@pytest.mark.parametrize("k", [0, 1, 2, 3])
def test_one_float_past_the_end_is_seen(k):
    p = place(k)
    exact(p)
    p.flat[p.start + p.n] = 1.0
    with pytest.raises(AssertionError, match="PAST the end"):
        p.check("past")


@pytest.mark.parametrize("k", [0, 1, 2, 3])
def test_one_float_before_the_start_is_seen(k):
    p = place(k)
    exact(p)
    p.flat[p.guard - 1] = 1.0
    with pytest.raises(AssertionError, match="BEFORE d_out"):
        p.check("before")


@pytest.mark.parametrize("k", [0, 1, 2, 3])
@pytest.mark.parametrize("where", [0, ROWS * WIDTH // 2, ROWS * WIDTH - 1])
def test_one_unwritten_element_is_seen(k, where):
    p = place(k)
    exact(p)
    p.bits[p.start + where] = INTERIOR_BITS
    with pytest.raises(AssertionError, match="never written"):
        p.check("unwritten")


@pytest.mark.parametrize("k", [1, 2, 3])
def test_a_write_into_the_leading_floats_is_seen(k):
    p = place(k)
    exact(p)
    p.flat[p.start - 1] = 1.0
    with pytest.raises(AssertionError, match="leading floats"):
        p.check("leading")


def test_a_write_of_the_same_float_value_is_still_a_write():
    """The guards and the interior both hold NaNs: float comparison could tell neither from the other, nor from a NaN a
    kernel computes.  The int32 view can."""
    p = place(1)
    exact(p)
    p.bits[p.start + p.n + 5] = 0x7FC00000        # a NaN, but not the guard's
    with pytest.raises(AssertionError, match="PAST the end"):
        p.check("nan past")
    q = place(1)
    q.bits[q.start:q.start + q.n] = 0x7FC00000    # every element written with a NaN of another payload: written
    q.check("nan rows")
    assert not q.all_finite()
    assert GUARD_BITS != INTERIOR_BITS


def test_pcm_placement_is_an_interior_view():
    p = PcmPlacement(1001, k=2, device="cpu")
    assert p.ptr == p.flat.data_ptr() + 2 * (GUARD + 2) and p.ptr % 4 == 0 and p.ptr % 16 == 4
    x = np.arange(7, dtype=np.int16)
    p.put(994, x)
    assert np.array_equal(p.interior()[994:].numpy(), x)
    with pytest.raises(AssertionError):
        p.put(995, x)
    with pytest.raises(AssertionError):
        PcmPlacement(10, k=1, device="cpu")      # a 2-byte aligned d_pcm is refused by the entries (MFX_ERR_ARG)
