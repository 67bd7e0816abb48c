"""Records tests/golden/resample_bits_parent.npz: what commit 7d4edbf (k_resample and k_sess_resample before they shared one
tile body, one LDS struct and one launcher core) gives for the cases of tests/resample_bits_cases.py, on an MI355X.  The
kernels' argument structs changed with that work, so the library comes from the WHOLE tree of that commit, not from a variant
linked against this tree's host objects:

    git worktree add --detach ../resample_parent 7d4edbf && make -C ../resample_parent/asr-featext-opencl_amd/csrc
    MFX_LIB=../resample_parent/asr-featext-opencl_amd/libmfcchip.so python3 tests/golden/make_resample_bits_parent.py [out.npz]

Per stored name: the converted int16 samples themselves, [samples][channels].  The three cuts of a session stream must agree
before one of them is stored."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import __graft_entry__ as G        # noqa: E402
import resample_bits_cases as BC   # noqa: E402

pkg = G.load_package()
out, failed = {}, []
for name, c in BC.CASES.items():
    assert BC.geometry(pkg, c) == c["want"], (name, BC.geometry(pkg, c))
    if c["kind"] == "session":
        assert BC.needed(c) <= BC.paths(pkg, c), (name, BC.paths(pkg, c))
    try:
        got = BC.run_case(pkg, name)
    except (AssertionError, pkg.MfxError) as e:     # (the other cases are still worth seeing)
        failed.append(name)
        print("%-28s FAILED: %r" % (name, e), flush=True)
        continue
    if c["stored"] in out and not np.array_equal(out[c["stored"]], got):
        failed.append(name)
        print("%-28s FAILED: differs from the cut recorded as %s" % (name, c["stored"]), flush=True)
        continue
    out[c["stored"]] = got
    print("%-28s tile %4d  R %d  %6d samples x %d, %d at the clamp" % (name, c["want"]["tile_out"], c["want"]["R"], got.shape[0],
                                                                       got.shape[1], int((np.abs(got.astype(np.int32)) >= 32767).sum())),
          flush=True)
path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "resample_bits_parent.npz")
np.savez_compressed(path, **out)
assert not failed, failed
print("wrote %s (%d bytes), library %s" % (path, os.path.getsize(path), os.environ.get("MFX_LIB") or "in-tree"))
