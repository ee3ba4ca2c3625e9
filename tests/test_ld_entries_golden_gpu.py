"""The general-window LD entries (mxa_ld_window_rows / _scores / _pairs / _apply / _prune, plain and _pairwise, mxa_ld_prune_csr and the operator object) bit
for bit against the library's own results as recorded in tests/golden/ld_entries_digests.json (`recorded_at` names the commit: the last one before the count
scratch got one reader and one host pipeline and the crossproduct unit was split).  The other tests of these entries bound them and check identities between
them; this one pins every bit of every value, CSR position, kept SNP and iteration count.

tests/golden/make_golden_ld_entries.py holds the cases and computes them here exactly as it recorded them, in one child process.  Compared are sha256 digests
over the results of one family (rows and scores, pairs, apply, prune, operator) of one case, sentinel-filled padding included.  The digests of the seeded
inputs are asserted first: a numpy that draws other numbers fails there, not as a kernel change."""
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(GOLDEN_DIR, "ld_entries_digests.json")) as fh:
        return json.load(fh)


@pytest.fixture(scope="module")
def computed(tmp_path_factory):
    spec = importlib.util.spec_from_file_location("make_golden_ld_entries", os.path.join(GOLDEN_DIR, "make_golden_ld_entries.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    return gen.collect(str(tmp_path_factory.mktemp("ld_entries")))


def test_inputs_are_the_recorded_ones(golden, computed):
    # per shape: positions, chromosomes, the distance window, f, two PLINK matrices; 128 cases of five families
    assert len(golden["inputs"]) == 18 and len(golden["results"]) == 640
    assert computed["inputs"] == golden["inputs"]


@pytest.mark.parametrize("family", ["rs", "pairs", "apply", "prune", "op"])
@pytest.mark.parametrize("route", ["plain", "pw"])
def test_results_are_the_recorded_bits(golden, computed, route, family):
    assert computed["inputs"] == golden["inputs"]
    pick = lambda d: {k: v for k, v in d.items() if f" {route} " in k and k.endswith("|" + family)}
    want, got = pick(golden["results"]), pick(computed["results"])
    assert len(want) >= 40 and sorted(got) == sorted(want)
    differ = [k for k in sorted(want) if got[k] != want[k]]
    assert not differ, f"{len(differ)} of {len(want)} results differ from the recorded bits: {differ[:10]}"
    # every result belongs to exactly one of the ten groups
    assert all(k.split(" ")[1] in ("plain", "pw") and k.rsplit("|", 1)[1] in ("rs", "pairs", "apply", "prune", "op") for k in golden["results"])
