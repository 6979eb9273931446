"""Records tests/golden/abi_refusals.json: the (status, message) of every refusal in
tests/test_abi_refusals.py, from the library given (a build of the commit before the entry
points moved onto the shared launch skeleton). Needs the device.

    python tests/golden/make_abi_refusals.py LIBRARY [OUT.json]"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

from ldpcsimulation_amd import native  # noqa: E402

native.use_library(sys.argv[1])
import test_abi_refusals as R  # noqa: E402
from conftest import code_path  # noqa: E402

ctx = native.Context(native.Graph.from_alist(code_path(R.PEG)), 0, 8)
nb = native.NbContext(native.NbGraph.from_alist(code_path(R.GF16)), 0, 8)
got = R.run(R.table(ctx, nb))
host = R.run(R.table())
assert all(got[k] == v for k, v in host.items())
assert all(rc < 0 for rc, _ in got.values()), {k: v for k, v in got.items() if v[0] >= 0}
with open(sys.argv[2] if len(sys.argv) > 2 else R.GOLDEN, "w") as f:
    json.dump(got, f, indent=0, sort_keys=True)
    f.write("\n")
print(len(got), "refusals,", len(host), "of them without a device")
