"""GPU: the PNG and the JPEG encoder write the files the parent of csrc/codec_common.h wrote, byte for byte.
tests/golden/codec_parent.json holds the size and sha256 of every file of the cases of tests/codec_record.py as that commit's
library wrote them on an MI355X (the recorder's head comment says how); the working tree has to write the same files."""
import json
import os

import pytest

import codec_record as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def written():
    from ppst_amd import imageio
    return R.record(imageio)


@pytest.fixture(scope="module")
def parent(golden_dir):
    with open(os.path.join(golden_dir, "codec_parent.json")) as f:
        return json.load(f)


def test_the_record_holds_every_case(parent):
    assert sorted(k for k in parent if k != "_doc") == sorted(c.id for c in R.CASES)


@pytest.mark.parametrize("case", R.CASES, ids=[c.id for c in R.CASES])
def test_files_equal_the_parents(case, written, parent):
    got, want = written[case.id], parent[case.id]
    assert len(got["sizes"]) == case.shape[0]
    assert got["sizes"] == want["sizes"]
    assert got["sha256"] == want["sha256"]
