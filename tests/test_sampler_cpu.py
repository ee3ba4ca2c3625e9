"""The sampled-rows checker of the full-size tests (_util.check_sampled_rows) on problems small enough for the whole long-double oracle product:
it passes the oracle's own result and catches each of four faults planted in a copy of it -- one flipped element, two swapped rows, rows off by
one, and a relative error of 1e-9 in a row whose values are ~1e-6 of max|C| (below the norm-wise tolerance: only the element-wise bound sees it)."""
import numpy as np
import pytest

from _util import Oracle, check_sampled_rows, make_B, make_problem, pack_plink, unpack_2bit


def _sample(prob, nsample, seed):
    rng = np.random.default_rng(seed)
    ii = np.sort(rng.choice(prob["indiv"], nsample, replace=False))
    ss = np.sort(rng.choice(prob["snps"], nsample, replace=False))
    return dict(snps=prob["snps"], indiv=prob["indiv"], f=prob["f"], ii=ii, ss=ss,
                rows_t=prob["plink_t"][ii], rows_s=prob["plink"][ss])


def _oracle_C(o, prob, trans, n, centered, seed=3):
    k = prob["indiv"] if trans else prob["snps"]
    Bt = make_B(k, n, seed=seed)                              # n x k: row j = column j of B
    C = o.dgemm_dense(trans, prob, Bt, centered).T.copy()     # m x n, like a result of the library
    return np.ascontiguousarray(Bt.T), C


def test_unpack_matches_the_generator_and_the_missing_code():
    prob = make_problem(1003, 37, 1, seed=2, missing_frac=0.1)
    assert np.array_equal(unpack_2bit(prob["plink_t"], 1003), prob["Z"])                # missing (01) -> 0
    assert np.array_equal(unpack_2bit(prob["plink"], 37), prob["Z"].T)
    V = np.random.default_rng(1).integers(0, 4, size=(5, 13))
    P = np.zeros((5, 4), np.uint8)
    for j in range(13):
        P[:, j // 4] |= (V[:, j] << (2 * (j % 4))).astype(np.uint8)
    assert np.array_equal(unpack_2bit(P, 13, is_plink=False), V)


@pytest.mark.parametrize("trans", [0, 1])
@pytest.mark.parametrize("centered", [0, 1])
def test_sampler_passes_the_oracle_and_catches_planted_faults(trans, centered):
    o = Oracle()
    prob = make_problem(1201, 517, 1, seed=7 + trans, missing_frac=0.01)
    n = 6
    B, C = _oracle_C(o, prob, trans, n, centered)
    S = _sample(prob, 24, seed=11)
    rows = S["ss"] if trans else S["ii"]
    cols = [0, 3, 5]
    good = check_sampled_rows(S, trans, B, C, cols, centered)
    assert good["ok"] and good["err"] <= 1e-15 and good["bound_ratio"] <= 1e-3, good
    # the same result as a row block starting at row 100 of a larger matrix (per-shard results): row_offset
    off = 100
    Cb = np.vstack([np.full((off, n), np.nan), C])
    assert check_sampled_rows(S, trans, B, Cb[off:], cols, centered)["ok"]
    Cshift = np.vstack([np.full((off, n), 7.0), C])                      # the block read at the wrong offset: caught
    assert not check_sampled_rows(S, trans, B, Cshift, cols, centered, row_offset=0)["ok"]
    assert check_sampled_rows(S, trans, B, Cshift, cols, centered, row_offset=-off)["ok"]

    r = int(rows[len(rows) // 2])
    j = cols[1]
    faults = {}
    F = C.copy(); F[r, j] = -F[r, j] if abs(F[r, j]) > 1e-3 * np.abs(C).max() else F[r, j] + 1.0     # one flipped element
    faults["flipped element"] = F
    other = int(rows[3]) + 1 if int(rows[3]) + 1 not in set(rows.tolist()) else int(rows[3]) - 1
    F = C.copy(); F[[int(rows[3]), other]] = F[[other, int(rows[3])]]                                 # two swapped rows (one of them sampled)
    faults["swapped rows"] = F
    faults["row offset by one"] = np.vstack([C[1:], C[-1:]])                                        # row r holds row r + 1
    for name, F in faults.items():
        v = check_sampled_rows(S, trans, B, F, cols, centered)
        assert not v["ok"], (name, v)


@pytest.mark.parametrize("trans", [0, 1])
def test_sampler_catches_a_relative_error_in_a_row_far_below_max(trans):
    """A row whose values are ~1e-6 of max|C|: its genotypes sit only where B is scaled by 1e-6.  An error of 1e-9 of its own size is 1e-15 of max|C|,
    far inside the norm-wise 1e-11; the element-wise bound (4 K 2^-53 of the row's own magnitude, ~1e-12 relative here) catches it."""
    o = Oracle()
    snps, indiv, n = 1500, 301, 4
    rng = np.random.default_rng(5)
    Z = rng.integers(0, 3, size=(indiv, snps)).astype(np.int8)
    k = indiv if trans else snps
    small = np.arange(40)                                    # inner indices where B is tiny
    if trans:
        s0 = 123
        Z[:, s0] = 0
        Z[small, s0] = rng.integers(1, 3, size=len(small))  # SNP s0 carried only by individuals 0..39
    else:
        s0 = 77
        Z[s0, :] = 0
        Z[s0, small] = rng.integers(1, 3, size=len(small))  # individual 77 carries only SNPs 0..39
    prob = dict(snps=snps, indiv=indiv, Z=Z, plink=pack_plink(np.ascontiguousarray(Z.T)), plink_t=pack_plink(Z), f=Z.mean(axis=0) / 2.0)
    Bt = make_B(k, n, seed=9)
    Bt[:, small] *= 1e-6
    C = o.dgemm_dense(trans, prob, Bt, 0).T.copy()
    B = np.ascontiguousarray(Bt.T)
    assert np.abs(C[s0]).max() <= 3e-6 * np.abs(C).max()
    S = _sample(prob, 16, seed=4)
    key = "ss" if trans else "ii"
    S[key] = np.unique(np.concatenate([S[key][:15], [s0]]))
    S["rows_s" if trans else "rows_t"] = (prob["plink"] if trans else prob["plink_t"])[S[key]]
    cols = [0, 1, 2, 3]
    good = check_sampled_rows(S, trans, B, C, cols, 0)
    assert good["ok"], good
    F = C.copy()
    F[s0] *= 1.0 + 1e-9
    bad = check_sampled_rows(S, trans, B, F, cols, 0)
    assert bad["err"] <= 1e-11                               # the norm-wise test alone passes it ...
    assert not bad["ok"] and bad["bound_ratio"] > 1.0, bad   # ... the element-wise bound does not
