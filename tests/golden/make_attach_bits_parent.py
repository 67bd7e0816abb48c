"""Records tests/golden/attach_bits_parent.npz: what commit da4d973 (the attachments of a planned batch before they got one
utterance tiling for host and kernels) gives for the cases of tests/attach_bits_cases.py, on an MI355X.  Build that commit as a
variant library and run

    tools/build_variant.sh parent "" da4d973        (in a checkout of da4d973: its host objects go with its kernels)
    MFX_LIB=build/var/lib_parent.so python3 tests/golden/make_attach_bits_parent.py [out.npz]

Never from the tree under test: without MFX_LIB the script refuses.  Every case runs twice, on two handles; a case whose two
runs differ in a single bit is reported and left out, and the file is written only when every case is in it."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import __graft_entry__ as G     # noqa: E402
import attach_bits_cases as AC  # noqa: E402

if not os.environ.get("MFX_LIB"):
    sys.exit("MFX_LIB is not set: the fixture is recorded from the parent commit's library, never from this tree")
pkg = G.load_package()
out, left_out = {}, []
for name, c in AC.CASES.items():
    a, b = AC.record(pkg, name), AC.record(pkg, name)
    same = a.keys() == b.keys() and all(a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes() for k in a)
    if not same:
        left_out.append(name)
        print("%-28s NOT REPRODUCIBLE on the parent: left out" % name, flush=True)
        continue
    for k, v in a.items():
        out[name + "__" + k] = v
    print("%-28s frames %-36s %s" % (name, c["frames"], " ".join(sorted(a))), flush=True)
if left_out:
    sys.exit("not written: %s" % left_out)
path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "attach_bits_parent.npz")
np.savez_compressed(path, **out)
print("wrote %s (%d bytes), library %s" % (path, os.path.getsize(path), os.environ["MFX_LIB"]))
