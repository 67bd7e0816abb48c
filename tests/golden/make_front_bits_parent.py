"""Records tests/golden/front_bits_parent.npz: the rows that commit 64dcbfe (the register front ends before their shared
pieces moved into csrc/mfx_front_dev.h) gives for the cases of tests/front_bits_cases.py, on an MI355X.  Build that commit's
kernels as a variant library and run

    tools/build_variant.sh parent "" 64dcbfe
    MFX_LIB=build/var/lib_parent.so python3 tests/golden/make_front_bits_parent.py [out.npz]

The rows are float32 bit patterns (int32 views), one array per case (at most 125 rows x 80 columns: nothing is cut), with the
first row of each utterance beside them."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import __graft_entry__ as G   # noqa: E402
import front_bits_cases as FC  # noqa: E402

pkg = G.load_package()
out = {}
for name, (sh, kernel, why) in FC.CASES.items():
    rows, first, ran = FC.run_batch(pkg, sh)
    assert ran == kernel and rows.shape == (sum(sh["frames"]), FC.cols(sh)) and np.isfinite(rows).all(), (name, ran, rows.shape)
    out[name] = np.ascontiguousarray(rows, np.float32).view(np.int32)
    out[name + "__first_rows"] = np.asarray(first, np.int32)
    print("%-24s rows %-10s kernel %s" % (name, rows.shape, ran))
path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "front_bits_parent.npz")
np.savez_compressed(path, **out)
print("wrote %s (%d bytes), library %s" % (path, os.path.getsize(path), os.environ.get("MFX_LIB") or "in-tree"))
