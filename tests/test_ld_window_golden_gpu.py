"""The four windowed LD entries (mxa_ld_band, mxa_ld_scores, mxa_ld_band_pairwise, mxa_ld_scores_pairwise) bit for bit against the library's own results
as recorded in tests/golden/ld_window_digests.json (commit e43c170: two copies of the window epilogue, two host drivers).  The other windowed tests bound
the scores by a summation bound and check that they reproduce; this one pins every bit of every band and score, so a change of a summation order, of a slot
of the partial buffer or of a window test is reported whatever its size.

tests/golden/make_golden_ld_window.py holds the cases and computes them here exactly as it recorded them, in two child processes (MXA_XPROD_GANG is read
once per process: the second one runs the gang-synchronised kernels).  Compared are sha256 digests of the results' bytes, sentinel-filled band padding
included.  The digests of the seeded inputs are asserted first: a numpy that draws other numbers fails there, not as a kernel change."""
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(GOLDEN_DIR, "ld_window_digests.json")) as fh:
        return json.load(fh)


@pytest.fixture(scope="module")
def computed(tmp_path_factory):
    spec = importlib.util.spec_from_file_location("make_golden_ld_window", os.path.join(GOLDEN_DIR, "make_golden_ld_window.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    return gen.collect(str(tmp_path_factory.mktemp("ld_window")))


def test_inputs_are_the_recorded_ones(golden, computed):
    assert len(golden["inputs"]) == 19 and len(golden["results"]) == 608
    assert computed["inputs"] == golden["inputs"]


@pytest.mark.parametrize("gang", ["classic", "gang2"])
@pytest.mark.parametrize("route", ["plain", "pairwise"])
def test_results_are_the_recorded_bits(golden, computed, route, gang):
    assert computed["inputs"] == golden["inputs"]
    pick = lambda d: {k: v for k, v in d.items() if k.startswith(route + " ") and (" gang=gang2 " in k) == (gang == "gang2")}
    want, got = pick(golden["results"]), pick(computed["results"])
    assert len(want) >= 8 and sorted(got) == sorted(want)
    differ = [k for k in sorted(want) if got[k] != want[k]]
    assert not differ, f"{len(differ)} of {len(want)} results differ from the recorded bits: {differ[:10]}"
    # every result belongs to exactly one of the four groups
    assert all(k.split(" ", 1)[0] in ("plain", "pairwise") for k in golden["results"])
