"""Records tests/golden/mel_plan_parent.json: what commit c895d04 (two plan types and two builders, build_mel_lane_plan for 16
lanes and build_mel_wave_plan for 32 / 64, before build_mel_plan replaced them) answers mfx_host_mel_lane_plan for the cases of
tests/mel_plan_cases.py.  Host code only: no GPU is needed.  Build that commit's library and run

    tools/build_variant.sh parent        (in a checkout of c895d04)
    MFX_LIB=build/var/lib_parent.so python3 tests/golden/make_mel_plan_parent.py [out.json]

Never from the tree under test: without MFX_LIB the script refuses.  For every case the file holds the return code (the number
of rounds, or the error) and a SHA-256 over L, row_stride, start, fid and w (null where the call refuses)."""
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [os.path.join(ROOT, "tests")]
import mel_plan_cases as PC  # noqa: E402

if not os.environ.get("MFX_LIB"):
    sys.exit("MFX_LIB is not set: the fixture is recorded from the parent commit's library, never from this tree")
lib = ctypes.CDLL(os.path.abspath(os.environ["MFX_LIB"]))
out = {}
for case in PC.cases():
    rc, digest = PC.plan_digest(lib, case)
    out[PC.key(case)] = [rc, digest]
assert len(out) == len(PC.cases())
path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "mel_plan_parent.json")
with open(path, "w") as f:
    f.write("{\n" + ",\n".join("%s: %s" % (json.dumps(k), json.dumps(out[k])) for k in sorted(out)) + "\n}\n")  # a case per line
refused = sum(1 for rc, _ in out.values() if rc < 0)
print("wrote %s (%d bytes): %d cases, %d refused, library %s" % (path, os.path.getsize(path), len(out), refused, os.environ["MFX_LIB"]))
