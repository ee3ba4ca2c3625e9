"""miraculix_amd -- MI355X-native compressed-genotype GEMM engine behind the miraculix C ABI.

The product is the shared library miraculix_amd/lib/libmiraculix_amd.so (C ABI: include/miraculix_amd.h, sources
miraculix_amd/csrc).  These Python modules are the host-side mirror of the reference's Julia binding modules
(src/bindings/Julia/miraculix.jl:114-118: dgemm_compressed, crossproduct, solve, read_plink, compressed_operations), used by
the tests and bench.py exactly as the reference's tests use the Julia modules.  No CPU fallback exists.
"""
from . import lib  # noqa: F401
from . import dgemm_compressed  # noqa: F401
from . import crossproduct  # noqa: F401
from . import compressed_operations  # noqa: F401
from . import read_plink  # noqa: F401
from . import solve  # noqa: F401
from . import assoc  # noqa: F401
from .crossproduct import ld_prune, ld_prune_csr  # noqa: F401
from .assoc import assoc_basis, assoc_linear, assoc_logistic, assoc_logistic_null, assoc_score, assoc_score_firth, assoc_score_spa  # noqa: F401
from .assoc import assoc_logistic_sets, assoc_set, assoc_skat_pvalue  # noqa: F401
from . import mixed  # noqa: F401
from .mixed import assoc_mixed, assoc_mixed_null  # noqa: F401
from .lib import load_shared_library, set_library_path, check_library_handle  # noqa: F401
