"""Records tests/golden/mel_rounds_parent.npz: the rows that commit cb8bf57 (k_front512's mel walk in 8-bin trips, before the
round-sized batches of profiles/r05 were tried) gives for the cases of tests/mel_rounds_cases.py, on an MI355X.  Build that
commit's kernels as a variant library and run

    tools/build_variant.sh parent "" cb8bf57
    MFX_LIB=build/var/lib_parent.so python3 tests/golden/make_mel_rounds_parent.py [out.npz]

The rows are float32 bit patterns (int32 views), one array per case, with the first row of each utterance beside them."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import __graft_entry__ as G   # noqa: E402
import mel_rounds_cases as MC  # noqa: E402

pkg = G.load_package()
out = {}
for name, (sh, L, why) in MC.CASES.items():
    kernel, got_L = MC.plan_rounds(pkg, sh)
    assert kernel == "k_front512" and got_L == L, (name, kernel, got_L)
    rows, first, ran = MC.run_batch(pkg, sh)
    assert ran == "k_front512" and np.isfinite(rows).all(), (name, ran)
    out[name] = np.ascontiguousarray(rows, np.float32).view(np.int32)
    out[name + "__first_rows"] = np.asarray(first, np.int32)
    print("%-18s rounds %-20s rows %s  kernel %s" % (name, L, rows.shape, ran))
path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "mel_rounds_parent.npz")
np.savez_compressed(path, **out)
print("wrote %s (%d bytes), library %s" % (path, os.path.getsize(path), os.environ.get("MFX_LIB") or "in-tree"))
