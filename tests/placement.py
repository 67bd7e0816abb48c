"""Buffer placement for the tests of the batch and session entries (test infrastructure only).

include/mfx.h asks nothing of d_out beyond float alignment, so a caller may point it at any row of a larger matrix.
OutPlacement lays one flat tensor out as [guard | k floats | total_rows * width floats | guard] and hands out the address of
the interior: k = 0 .. 3 walks d_out through every 4-byte position of a 16-byte word.  The guards (and the k leading floats)
hold one NaN bit pattern, the interior another; both are compared through an int32 view, so a write of the same float
VALUE -- another NaN included -- is still seen as a write.  After the run check() asserts that the guards and the leading
floats are bit-unchanged and that no interior element still holds the interior pattern, and returns the interior as
[total_rows][width].

PcmPlacement does the same for an int16 PCM array, the base moved by k samples (k even: d_pcm must be 4-byte aligned).
Reads cannot be observed: its guards only document that the array is an interior view of a larger allocation.

Works on CPU tensors too (tests/test_placement_host.py runs the checker against deliberately wrong writers)."""
import torch

GUARD = 4096                  # floats (or samples) on either side
GUARD_BITS = 0x7FC0BEEF       # a quiet NaN
INTERIOR_BITS = 0x7FC0DEAD    # another one: no kernel computes this payload
PCM_GUARD = 0x5A5A
_STEP = 1 << 26               # elements per comparison: the temporaries of a check stay at a few hundred MB


def _count(bits, value, equal):
    """Elements of the int32 view `bits` that are == value (equal) or != value, counted in bounded pieces."""
    n = 0
    for i in range(0, bits.numel(), _STEP):
        piece = bits[i:i + _STEP]
        n += int(((piece == value) if equal else (piece != value)).sum())
    return n


def _first(bits, value, equal):
    for i in range(0, bits.numel(), _STEP):
        piece = bits[i:i + _STEP]
        hit = torch.nonzero((piece == value) if equal else (piece != value))
        if hit.numel():
            return i + int(hit[0])
    return -1


class OutPlacement:
    def __init__(self, total_rows, width, k=0, device="cuda:0", guard=GUARD):
        assert guard >= GUARD and guard % 4 == 0 and 0 <= k
        self.rows, self.width, self.k, self.guard = int(total_rows), int(width), int(k), int(guard)
        self.n = self.rows * self.width
        self.start = self.guard + self.k                      # first interior float
        self.flat = torch.empty(self.start + self.n + self.guard, dtype=torch.float32, device=device)
        assert self.flat.data_ptr() % 16 == 0, "the allocator hands out 16-byte aligned blocks"
        self.bits = self.flat.view(torch.int32)
        self.refill()

    def refill(self):
        self.bits[:self.start].fill_(GUARD_BITS)
        self.bits[self.start + self.n:].fill_(GUARD_BITS)
        for i in range(self.start, self.start + self.n, _STEP):
            self.bits[i:min(i + _STEP, self.start + self.n)].fill_(INTERIOR_BITS)

    @property
    def ptr(self):
        """d_out: k floats past a 16-byte boundary."""
        return self.flat.data_ptr() + 4 * self.start

    def interior(self):
        return self.flat[self.start:self.start + self.n].view(self.rows, self.width)

    def check(self, what=""):
        if self.flat.is_cuda:
            torch.cuda.synchronize(self.flat.device)
        front, back = self.bits[:self.guard], self.bits[self.start + self.n:]
        lead = self.bits[self.guard:self.start]
        inner = self.bits[self.start:self.start + self.n]
        bad = _first(lead, GUARD_BITS, False)
        assert bad < 0, "%s: write into the %d leading floats in front of d_out (float %d of them)" % (what, self.k, bad)
        bad = _first(front, GUARD_BITS, False)
        assert bad < 0, "%s: write %d floats BEFORE d_out (%d guard floats changed)" % (
            what, self.start - bad, _count(front, GUARD_BITS, False))
        bad = _first(back, GUARD_BITS, False)
        assert bad < 0, "%s: write %d floats PAST the end of d_out (%d guard floats changed)" % (
            what, bad + 1, _count(back, GUARD_BITS, False))
        left = _count(inner, INTERIOR_BITS, True)
        if left:
            i = _first(inner, INTERIOR_BITS, True)
            raise AssertionError("%s: %d elements of d_out were never written (first: row %d, column %d)" % (
                what, left, i // max(self.width, 1), i % max(self.width, 1)))
        return self.interior()

    def all_finite(self):
        """isfinite over the whole interior, on the tensor's device, in bounded pieces."""
        inner = self.flat[self.start:self.start + self.n]
        return all(bool(torch.isfinite(inner[i:i + _STEP]).all()) for i in range(0, self.n, _STEP))


class PcmPlacement:
    """[guard | k samples | n int16 elements | guard]; the interior is NOT filled (torch.empty: a sparse array of many GB
    costs nothing but address space that is never touched)."""

    def __init__(self, n_elems, k=0, device="cuda:0", guard=GUARD):
        assert guard >= GUARD and guard % 8 == 0 and k >= 0 and k % 2 == 0, "d_pcm must stay 4-byte aligned"
        self.n, self.k, self.guard = int(n_elems), int(k), int(guard)
        self.start = self.guard + self.k
        self.flat = torch.empty(self.start + self.n + self.guard, dtype=torch.int16, device=device)
        assert self.flat.data_ptr() % 16 == 0
        self.flat[:self.start].fill_(PCM_GUARD)
        self.flat[self.start + self.n:].fill_(PCM_GUARD)

    @property
    def ptr(self):
        return self.flat.data_ptr() + 2 * self.start

    def interior(self):
        return self.flat[self.start:self.start + self.n]

    def put(self, elem_off, samples):
        """Write a numpy int16 array (all channels interleaved) at element elem_off of the interior."""
        x = torch.from_numpy(samples.reshape(-1).copy())
        assert 0 <= elem_off and elem_off + x.numel() <= self.n
        self.flat[self.start + elem_off:self.start + elem_off + x.numel()] = x.to(self.flat.device)
