"""The fp64 product entries (dgemm_compressed with host and device operands, mxa_dgemm_compressed_device, mxa_gram_matvec and _device) bit for bit against the
library's own results as recorded in tests/golden/dgemm_digests.json (`recorded_at` names the commit: the last one before the host driver of the product moved
from mxa_api.cpp into mxa_product.cpp and was cut into named routes).  The other tests of these entries bound them against the oracle and check identities
between routes; this one pins every bit of C and the route every product takes (mxa_last_path, mxa_last_geometry) on each route of the driver: the guarded
int8 route, the column peel, the fp64 tile, the pair tables, both orientation policies, MXA_GEMM_TR=0, MXA_I8_TN=1, engines 1 / 3 / 4, host operands, gram, the
range fallback, grouped K splits, the host pipeline and a sharded object.

tests/golden/make_golden_dgemm.py holds the cases and computes them here exactly as it recorded them, in one child process (about 5 s).  Compared are, per case,
the sha256 digest over the bytes of C (leading-dimension padding and two sentinel entries included) and the route, and the route itself.  The digests of the
seeded inputs are asserted first: a numpy that draws other numbers fails there, not as a change of the product."""
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
GROUPS = {"small": 288, "variant": 144, "fallback": 64, "grouped": 52, "pipeline": 16, "multi": 8}


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(GOLDEN_DIR, "dgemm_digests.json")) as fh:
        return json.load(fh)


@pytest.fixture(scope="module")
def computed(tmp_path_factory):
    spec = importlib.util.spec_from_file_location("make_golden_dgemm", os.path.join(GOLDEN_DIR, "make_golden_dgemm.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    assert tuple(GROUPS) == gen.GROUPS
    return gen.collect(str(tmp_path_factory.mktemp("dgemm")))


def test_inputs_are_the_recorded_ones(golden, computed):
    # per shape the PLINK matrix and f: four small shapes, two grouped ones, the pipeline's
    assert len(golden["inputs"]) == 14 and len(golden["results"]) == sum(GROUPS.values())
    assert computed["inputs"] == golden["inputs"]
    assert all(k.split("|")[0] in GROUPS for k in golden["results"])


@pytest.mark.parametrize("group", list(GROUPS))
def test_results_are_the_recorded_bits(golden, computed, group):
    assert computed["inputs"] == golden["inputs"]
    pick = lambda d: {k: v for k, v in d.items() if k.startswith(group + "|")}
    want, got = pick(golden["results"]), pick(computed["results"])
    assert len(want) == GROUPS[group] and sorted(got) == sorted(want)
    rerouted = [(k, want[k]["route"], got[k]["route"]) for k in sorted(want) if got[k]["route"] != want[k]["route"]]
    assert not rerouted, f"{len(rerouted)} of {len(want)} products took another route (case, recorded, now): {rerouted[:10]}"
    differ = [k for k in sorted(want) if got[k]["sha"] != want[k]["sha"]]
    assert not differ, f"{len(differ)} of {len(want)} results differ from the recorded bits: {differ[:10]}"
