"""Record what the front-end makes of the reference's own energy files, as digests: reference_energy_units.json, read by
tests/test_frontend.py::test_bundled_energies_are_the_references_energies.

  python tests/golden/make_reference_unit_digests.py <checkout of the reference>

Needs a build of thallo_amd/libThallo.so.  For every pair of REF_PAIRS it checks that the reference's file and the bundled energy give the
same translation unit and declarations up to the residuals' names, then stores the SHA-256 of each (no text of the reference is kept).  Run
it again whenever the front-end's output changes.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))

import thallo_amd  # noqa: E402
from test_frontend import REF_PAIRS, _unit_digests  # noqa: E402

if len(sys.argv) != 2 or not os.path.isdir(sys.argv[1]):
    sys.exit(__doc__)
out = {}
for rel, mine in REF_PAIRS:
    ref = _unit_digests(os.path.join(sys.argv[1], rel))
    assert ref == _unit_digests(thallo_amd.energy_file(mine)), (rel, mine)
    out[rel] = {"bundled": mine, **ref}
    print(rel, mine, ref["unit_sha256"][:16], ref["declarations_sha256"][:16])
with open(os.path.join(HERE, "reference_energy_units.json"), "w") as f:
    json.dump(out, f, indent=1)
    f.write("\n")
