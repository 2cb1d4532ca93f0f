"""-m gpu: the rate- and quality-targeted encodes give what a known-good library gave, value for value.  tests/ratepinned.py makes
the calls -- whole images (four geometry groups and one tile, both transforms, split and joint tables, byte targets of 2 x, 1/2 and
1/4 of the plain file and one below the headers, 35 dB, 50 dB and D = 0), a 4:2:0 image, an NV12 surface, a YUY2 frame and batches
of two tiles -- and tests/golden/rate_pinned.json holds their files' hashes, result structs, notes, budgets, unit rows and the hashes
of the four tables (tools/rate_pinned_record.py wrote it)."""
import json
import os

import pytest

import gpuutil as U
import ratepinned

pytestmark = pytest.mark.gpu

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rate_pinned.json")) as _fh:
    PINNED = json.load(_fh)


def test_every_case_is_pinned():
    assert set(PINNED) == set(ratepinned.CASES)


@pytest.mark.parametrize("name", sorted(PINNED))
def test_pinned(name):
    got = json.loads(json.dumps(ratepinned.CASES[name](U.ctx())))
    want = PINNED[name]
    assert got.keys() == want.keys()
    for key in want:
        assert got[key] == want[key], (name, key)
