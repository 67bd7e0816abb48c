"""Records tests/golden/tail_bits_parent.npz: what commit 90865a5 (the kernels behind the front ends before their tile, slicing
and launch code moved into shared pieces) gives for the cases of tests/tail_bits_cases.py, on an MI355X.  Build that commit's
kernels as a variant library and run

    tools/build_variant.sh parent "" 90865a5
    MFX_LIB=build/var/lib_parent.so python3 tests/golden/make_tail_bits_parent.py [out.npz]

Per case: the float32 bit patterns (int32 views) of the rows of the three shortest utterances in full, and an 8-byte BLAKE2b
digest of every row (uint64), utterance after utterance."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import __graft_entry__ as G   # noqa: E402
import tail_bits_cases as TC  # noqa: E402

pkg = G.load_package()
out, failed = {}, []
for name, c in TC.CASES.items():
    assert TC.branch(c) == c["want"], (name, TC.branch(c))
    try:
        got = TC.run_case(pkg, name)
        TC.assert_finite(name, got)
    except (AssertionError, pkg.MfxError) as e:     # (the other cases are still worth seeing)
        failed.append(name)
        print("%-28s FAILED: %r" % (name, e), flush=True)
        continue
    out[name + "__rows"] = TC.shortest_bits(got)
    out[name + "__digests"] = TC.digests(got)
    print("%-28s %-44s rows %5d x %d" % (name, c["want"], sum(len(g) for g in got), got[0].shape[1]), flush=True)
path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "tail_bits_parent.npz")
np.savez_compressed(path, **out)
assert not failed, failed
print("wrote %s (%d bytes), library %s" % (path, os.path.getsize(path), os.environ.get("MFX_LIB") or "in-tree"))
