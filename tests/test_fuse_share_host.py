"""Host side of tile sharing in the fused k_front512 (no GPU): the LDS formula of a delta tile against a laid-out count, which
orders fit a wave's frame slots, the packed claim word under random interleavings of two claimers, and the registers of the
FUSE builds as `make resources` reports them."""
import ctypes as C
import os
import random
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "asr-featext-opencl_amd", "csrc")
SLOTS = 4 * 512          # floats of a wave's four frame slots


def lds_floats(L, rows, l1, l2):
    shares = C.c_int32(-1)
    n = L.mfx_host_delta_tile_lds_floats(rows, l1, l2, C.byref(shares))
    return n, shares.value


def laid_out(rows, l1, l2):
    """delta_tile16's layout, word by word: statics with 2 (l1 + l2) context rows and deltas with 2 l2, as 16-float rows; then the
    output rows at their widest (48 floats) behind a phase of up to 3 floats, read back in whole 16-byte groups"""
    D = l1 + l2
    used = np.zeros(1 << 16, np.int32)
    pos = 0
    for r in range(rows + 2 * D):
        used[pos + 16 * r:pos + 16 * r + 16] += 1
    pos += 16 * (rows + 2 * D)
    for r in range(rows + 2 * l2):
        used[pos + 16 * r:pos + 16 * r + 16] += 1
    pos += 16 * (rows + 2 * l2)
    end = 3 + rows * 48
    used[pos:pos + 4 * ((end + 3) // 4)] += 1
    assert used.max() == 1
    return int(np.nonzero(used)[0][-1]) + 1


def test_sub_tile_formula_against_a_laid_out_count(pkg):
    L = pkg.load_library()
    fits = {}
    for l1 in range(0, 11):
        for l2 in range(0, 11):
            for rows in (16, 64):
                n, shares = lds_floats(L, rows, l1, l2)
                assert n == ((rows + 2 * (l1 + l2)) + (rows + 2 * l2)) * 16 + rows * 48 + 8
                count = laid_out(rows, l1, l2)
                assert count <= n <= count + 8, (rows, l1, l2, n, count)
            n16, shares = lds_floats(L, 16, l1, l2)
            assert shares == (1 if n16 <= SLOTS else 0)
            fits[(l1, l2)] = bool(shares)
    assert fits[(3, 3)] and fits[(2, 5)] and fits[(4, 0)] and fits[(1, 1)] and not fits[(8, 8)]
    assert lds_floats(L, 16, 3, 3)[0] == 1576                       # 6.3 KB of the 8 KB region
    # the bound is monotone: an order that does not fit is not followed by a larger one that does
    for (l1, l2), ok in fits.items():
        if not ok:
            assert not fits.get((l1 + 1, l2), False) and not fits.get((l1, l2 + 1), False)


def claim(L, word, from_head):
    t = C.c_int32(-2)
    w = L.mfx_host_fuse_claim(word, 1 if from_head else 0, C.byref(t))
    return w, t.value


@pytest.mark.parametrize("n_tiles", [0, 1, 2, 3, 17, 61, 1000, 65534])
def test_claim_word_two_claimers_random_interleavings(pkg, n_tiles):
    """Each claimer reads the word, computes its exchange, and the exchange succeeds only if the word is still what it read --
    the kernel's compare-exchange.  Whatever the schedule: every tile exactly once, and the claims end when head > tail."""
    L = pkg.load_library()
    n = C.c_int32(n_tiles)
    w0 = L.mfx_host_fuse_claim(-1, 0, C.byref(n))
    assert w0 == (1 | (n_tiles << 16))
    bad = C.c_int32(65535)
    assert L.mfx_host_fuse_claim(-1, 0, C.byref(bad)) == -1         # one more tile than the word can count
    for seed in range(4 if n_tiles > 100 else 25):
        rng = random.Random(1000 * n_tiles + seed)
        word, taken = w0, []
        seen = {True: None, False: None}         # the word each claimer last read (None: it reads next)
        done = {True: False, False: False}
        while not all(done.values()):
            who = rng.random() < (0.5 if seed % 3 else 0.9)
            if done[who]:
                who = not who
            if seen[who] is None:
                seen[who] = word
                continue
            new, t = claim(L, seen[who], who)
            if t < 0:                             # the word it read was exhausted: it stops (the list only ever shrinks)
                assert (seen[who] & 0xffff) > (seen[who] >> 16)
                done[who] = True
            elif seen[who] == word:               # exchange succeeds
                word = new
                taken.append((t, who))
                seen[who] = None
            else:                                 # exchange fails and returns the word as it stands
                seen[who] = word
        assert sorted(t for t, _ in taken) == list(range(n_tiles))
        assert (word & 0xffff) > (word >> 16) and claim(L, word, True) == (word, -1) and claim(L, word, False) == (word, -1)
        heads = [t for t, who in taken if who]
        tails = [t for t, who in taken if not who]
        assert heads == sorted(heads) and tails == sorted(tails, reverse=True)
        assert not heads or not tails or max(heads) < min(tails)


# scratch bytes per lane of the four FUSE builds k_front512<ALIGNED, false, NM, true> before tile sharing: none may gain any
# (the unaligned builds, and the aligned one of long windows, spill in their frame loop; the headline build does not)
PARENT_SCRATCH = {(True, 13): 0, (True, 16): 20, (False, 13): 48, (False, 16): 48}


def test_no_fuse_build_gains_scratch():
    r = subprocess.run(["make", "-s", "resources", "KERNEL_TUS=mfx_front512"], cwd=CSRC, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-2000:]
    blocks = re.split(r"Function Name: ", r.stdout)[1:]
    found = {}
    for b in blocks:
        m = re.match(r"\S*k_front512ILb([01])ELb0ELi(\d+)ELb1ELb0ELb0EEE", b)
        if m:
            found[(m.group(1) == "1", int(m.group(2)))] = (int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", b).group(1)),
                                                         int(re.search(r"Occupancy \[waves/SIMD\]: (\d+)", b).group(1)))
    assert set(found) == set(PARENT_SCRATCH), sorted(found)
    for k, (scratch, occupancy) in found.items():
        assert scratch <= PARENT_SCRATCH[k], "k_front512<%s, false, %d, true>: %d bytes of scratch, %d before" % (
            k[0], k[1], scratch, PARENT_SCRATCH[k])
        assert occupancy == 4
    assert found[(True, 13)][0] == 0                                 # the build the headline workload runs
