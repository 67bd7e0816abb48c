"""Records tests/golden/kaldi_bits_parent.npz: what commit b6732e9 (the Kaldi kernels with their own wave FFT, real split and
mel-span chain, before these became the pieces shared with the STFT FFT form) gives for the cases of tests/kaldi_bits_cases.py,
on an MI355X.  The kernels' argument structs changed with that work, so the library comes from the WHOLE tree of that commit,
not from a variant linked against this tree's host objects:

    git worktree add --detach ../kaldi_parent b6732e9 && make -C ../kaldi_parent/asr-featext-opencl_amd/csrc
    MFX_LIB=../kaldi_parent/asr-featext-opencl_amd/libmfcchip.so python3 tests/golden/make_kaldi_bits_parent.py [out.npz]

Per case: the float32 bit patterns (int32 views) of the rows of the three shortest non-empty utterances in full, and an 8-byte
BLAKE2b digest of every row (uint64), utterance after utterance."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import __graft_entry__ as G    # noqa: E402
import kaldi_bits_cases as BC  # noqa: E402

pkg = G.load_package()
out, failed = {}, []
for name, c in BC.CASES.items():
    try:
        got = BC.run_case(pkg, name)
    except (AssertionError, pkg.MfxError) as e:     # (the other cases are still worth seeing)
        failed.append(name)
        print("%-36s FAILED: %r" % (name, e), flush=True)
        continue
    out[name + "__rows"] = BC.shortest_bits(got)
    out[name + "__digests"] = BC.digests(got)
    print("%-36s rows %4d x %d" % (name, sum(len(g) for g in got), got[1].shape[1]), flush=True)
path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "kaldi_bits_parent.npz")
np.savez_compressed(path, **out)
assert not failed, failed
print("wrote %s (%d bytes), library %s" % (path, os.path.getsize(path), os.environ.get("MFX_LIB") or "in-tree"))
