"""mxa_assoc_set where its pieces, tiles, workgroups and pointer kinds had never run (the first module, tests/test_assoc_set_gpu.py, stops at two pieces, sets of
33 and 1024 entries, 21 items, all-host or all-device pointers, compact leading dimensions, 64 SNP rows and weights in (0.3, 4)).

Accuracy is the rule of the first module (tests/_assoc_set_call.py::check_accuracy): for Phi and each of the six statistics the scaled error against the
long-double evaluation of tests/_assoc_set_ref.py::set_reference must not exceed 16 max(eps, 2^-48), eps = the scaled error of the float64 evaluation of the same
case.  Before a device result is looked at, every accuracy case asserts on the CPU what the rule relies on: every SNP of a set has a called individual, and
eps < 2^-48 (so the bound is 16 * 2^-48 = 5.7e-14 in every case here).  Identities are asserted on bytes.  The padding fields of every row's last byte are dirty
throughout, the weights have both signs unless said otherwise, 5 % of the calls are missing.

Which edge of which kernel each shape is for:
 1 pieces          k_assoc_set_gram's split over the individuals (pieces of 4096 = 64 words; wave v takes the words v, v + 4, ...) and the ascending sum of
                   k_assoc_set_phi: indiv 4096 (one full piece), 4097 (a second piece of one individual), 8192 (two full pieces), 8515 (three pieces, the last
                   of six words: the waves take 2, 2, 1, 1), 12289 (four pieces, the last of one individual); sets {empty, the last row, 17 and 33 entries with
                   repeats}; (n, kh) = (2, 1), (1, 4), (3, 0), (2, 1), (1, 4).
 2 set sizes       the column loop of k_assoc_set_stat strides by 256 threads, its tiles by 16: m in {31, 32, 255, 256, 257, 1023} from 48 SNPs at indiv = 261
                   (66-byte rows: two alignments of a row within a 16-byte word), n = 2, kh = 1.
 3 m = 1024        64 full tiles with n = 2, two pieces (indiv 4099) and rows read in place.
 4 items           k_assoc_set_fold: one thread per (set, trait), 256 per workgroup: 140 sets x n = 2 = 280 items, the sets 127 / 128 on either side of the
                   workgroup edge, empty sets in the middle and at the end, lds = nsets + 3.
 5 pointer kinds   SetStage::run: rows in place or through the bounce buffer (ent_row remapped), stat on the device or through the device copy with
                   ld_stat = nsets, crossed with R, Wt and H on either side: 32 calls.
 6 leading dims    ldr, ldw, ldh > indiv, ldo > snps, lds > nsets; with device results and no scan outputs the stage reads the U that the scan allocated
                   itself at ldo (mxa_assoc.hip: bOwn, v.ldu).
 7 base pointers   assoc_load_word and the 2-D copies from bases off a 16- and 64-byte boundary, at 65-byte rows (indiv 259: every offset within a word).
 8 many rows       ent_row, the D / M column offsets and the bounce-row remap with row numbers up to 699; a set whose bounce rows are one run, one without
                   neighbours (each alone in its batch under MXA_ASSOC_SET_BATCH = 1).
 9 weights         omega of both signs, zeros, an all-zero set, all sets empty (every stage buffer a zero-size request).
10 p-values        the wrapper's hand-over to mxa_assoc_skat_pvalue and its burden line, against mpmath at 50 digits.

Measured on an MI355X (largest scaled error of the device / largest eps of the float64 evaluation; the bound is 5.7e-14 everywhere); all 24 tests passed, no
defect of the library was found:
 1 pieces        Phi 1.1e-15 / 3.7e-16, B 4.4e-18 / 7.7e-18, varB 7.5e-16 / 1.8e-16, Q 4.7e-18 / 8.3e-18, c1 7.5e-16 / 1.8e-16, c2 5.0e-16 / 1.1e-16,
                 c4 4.2e-16 / 1.0e-16; Phi_jj against the scan's var 1.0e-15
 2 set sizes     Phi 3.6e-16 / 3.2e-16, B 7.0e-18 / 4.2e-18, varB 1.5e-17 / 1.5e-17, Q 6.5e-17 / 1.3e-17, c1 1.4e-15 / 7.8e-17 (m = 1023), c2 9.3e-17 / 5.4e-17,
                 c4 2.8e-17 / 2.8e-17
 3 m = 1024      Phi 9.6e-16 / 2.6e-16, B 2.0e-18 / 4.6e-19, varB 1.7e-18 / 4.6e-19, Q 3.7e-18 / 2.2e-18, c1 3.0e-15 / 8.6e-17, c2 1.2e-16 / 1.2e-16,
                 c4 6.0e-17 / 8.5e-17
 4 items         Phi 4.1e-16 / 3.0e-16, B 3.0e-17 / 4.8e-17, varB 3.6e-16 / 4.2e-16, Q 3.1e-17 / 6.3e-17, c1 4.9e-16 / 2.9e-16, c2 2.2e-16 / 2.2e-16,
                 c4 1.5e-16 / 1.8e-16
 8 many rows     Phi 4.4e-16 / 3.3e-16, B 2.0e-17 / 2.8e-17, varB 1.8e-16 / 7.6e-17, Q 4.8e-17 / 2.8e-17, c1 1.8e-16 / 1.1e-16, c2 1.1e-16 / 1.4e-16,
                 c4 1.0e-16 / 5.2e-17
 9 weights       Phi 3.5e-16 / 2.6e-16, B 3.3e-18 / 8.6e-18, varB 2.0e-17 / 6.3e-17, Q 1.6e-17 / 1.6e-17, c1 1.3e-16 / 1.9e-16, c2 6.3e-17 / 8.2e-17,
                 c4 2.2e-17 / 2.6e-17; a set whose weights are all zero gives six +0.0 for every trait (no -0.0), also with every weight's sign flipped
10 p-values      skat_p against mpmath 1.0e-16 (280 items, 256 with positive moments) and 5.9e-17 (the six sizes of test 2); skat_df the rounded value or
                 its neighbour; burden_p bit for bit the header's line, against mpmath 2.6e-15 and 1.1e-15; the libm term (math.erfc against mpmath at the
                 test's arguments) 4.1e-16 = 3.7 u and 1.1e-16 = 1.0 u, below the 16 u at which it would have to be reported; no item had x <= 0
The c1 figures of the large sets (1.4e-15, 3.0e-15) are the ascending sum of m terms in one thread of k_assoc_set_fold, as the 1.1e-15 of the first module's
m = 1024.  Wall time of the module on the MI355X, run alone: 19.9 s, 13.5 s of it in the one test that is the first of the process to import torch and to open the
device through it (pieces, indiv 8515); every other test takes at most 1.5 s.
"""
import functools
import math
from collections import namedtuple

import numpy as np
import pytest

import _assoc_set_ref as sr
import _operands as op
from _assoc_set_call import LD, NAMES, call, case, check_accuracy, same, same_results, same_scan

pytestmark = pytest.mark.gpu

Case = namedtuple("Case", "codes X R Wt H sets weights indiv snps n kh")


@pytest.fixture(scope="module")
def mx():
    import miraculix_amd as m
    m.load_shared_library()
    return m


def signed(rng, m):
    return rng.uniform(0.3, 4.0, m) * rng.choice([-1.0, 1.0], m)


def make_case(indiv, snps, n, kh, sets, weights, seed):
    codes, R, Wt, H = sr.random_case(indiv, snps, n, kh, seed=seed, missing=0.05)
    X = sr.pack_dirty(codes, seed)
    for a in (codes, R, Wt, H, X):
        a.setflags(write=False)
    return Case(codes, X, R, Wt, H, [np.asarray(s, np.int64) for s in sets], weights, indiv, snps, n, kh)


@functools.lru_cache(maxsize=None)
def refs_of(maker, *args):
    """the two evaluations of a case, computed once: (long double, float64)"""
    c = maker(*args)
    return tuple(sr.set_reference(c.codes, c.R, c.Wt, c.H, c.sets, c.weights, dt) for dt in (LD, np.float64))


def run(mx, c, sets=None, weights=None, **kw):
    return call(mx, c.X, c.indiv, c.R, c.Wt, c.H, c.sets if sets is None else sets, c.weights if sets is None else weights, **kw)


def reference_holds(c, refs, label, only=None):
    """on the CPU, before any device result: every SNP of a set has a called individual, and the float64 evaluation is within 2^-48 of the long-double one"""
    used = np.unique(np.concatenate([np.asarray(s, np.int64) for s in c.sets] + [np.zeros(0, np.int64)]))
    assert np.all((c.codes[used] >= 0).any(axis=1)), label
    ld, f64 = refs
    ks = range(len(ld)) if only is None else only
    eps = {"Phi": max(sr.scaled_error(f64[k]["phi"], ld[k]["phi"], ld[k]["sphi"]) for k in ks)}
    for t, name in enumerate(NAMES):
        eps[name] = max(sr.scaled_error(f64[k]["stat"][:, t], ld[k]["stat"][:, t], ld[k]["sstat"][:, t]) for k in ks)
    print(f"{label} eps of the float64 evaluation: " + "  ".join(f"{k} {v:.2e}" for k, v in eps.items()))
    assert all(v < sr.TOL for v in eps.values()), (label, eps)
    return eps


def accurate(got, refs, label, only=None):
    """check_accuracy over the sets `only` (positions in refs) with got holding exactly those sets"""
    if only is not None:
        refs = tuple([r[k] for k in only] for r in refs)
    return check_accuracy(got, refs, label)


# ---- 1. pieces
PIECES = [(4096, 2, 1), (4097, 1, 4), (8192, 3, 0), (8515, 2, 1), (12289, 1, 4)]


@functools.lru_cache(maxsize=None)
def pieces_case(indiv, n, kh):
    snps = 24
    rng = np.random.default_rng([indiv, 51])
    sets = [np.zeros(0, np.int64), np.array([snps - 1]), rng.integers(0, snps, 17), rng.integers(0, snps, 33)]
    assert len(np.unique(sets[2])) < 17 and len(np.unique(sets[3])) < 33                                # with repeats
    return make_case(indiv, snps, n, kh, sets, [signed(rng, len(s)) for s in sets], seed=21)


@pytest.mark.parametrize("indiv,n,kh", PIECES)
def test_pieces_of_the_split_over_the_individuals(mx, indiv, n, kh):
    c, refs = pieces_case(indiv, n, kh), refs_of(pieces_case, indiv, n, kh)
    label = f"pieces indiv {indiv} n {n} kh {kh}"
    assert sr.SPLIT == 4096 and (indiv + sr.SPLIT - 1) // sr.SPLIT == {4096: 1, 4097: 2, 8192: 2, 8515: 3, 12289: 4}[indiv]
    reference_holds(c, refs, label)
    got = run(mx, c)
    eps_phi = accurate(got, refs, label)["Phi"][1]
    worst = 0.0
    for k, s in enumerate(c.sets):
        for t in range(n):
            P = got["phi"][k][t]
            assert same(P, P.T.copy()), (k, t)                                                            # Phi_jj' == Phi_j'j bit for bit
            for j, snp in enumerate(s):
                worst = max(worst, abs(P[j, j] - got["var"][snp, t]) / float(refs[0][k]["sphi"][t][j, j]))
    print(f"{label} Phi_jj against the scan's var, scaled: {worst:.3e}  bound {16 * max(eps_phi, sr.TOL):.3e}")
    assert worst <= 16 * max(eps_phi, sr.TOL)
    assert np.array_equal(got["stat"][0], np.zeros((n, 6)))                                               # the empty set
    if indiv == 8515:
        dev = run(mx, c, device=True)
        assert same_results(got, dev) and same_scan(got, dev), "device operands"
        for batch in (1, 10 ** 9):
            assert same_results(got, run(mx, c, env=dict(MXA_ASSOC_SET_BATCH=batch))), batch
            assert same_results(got, run(mx, c, device=True, env=dict(MXA_ASSOC_SET_BATCH=batch))), batch


# ---- 2. set sizes at the thread-stride and tile edges
EDGE_SIZES = (31, 32, 255, 256, 257, 1023)


@functools.lru_cache(maxsize=None)
def edges_case():
    snps = 48
    rng = np.random.default_rng(52)
    sets = []
    for m in EDGE_SIZES:
        perm = rng.permutation(snps)
        sets.append(perm[:m] if m <= snps else np.concatenate([perm, rng.integers(0, snps, m - snps)]))
    return make_case(261, snps, 2, 1, sets, [signed(rng, len(s)) for s in sets], seed=22)


@pytest.mark.parametrize("m", EDGE_SIZES)
def test_set_sizes_at_the_stride_and_tile_edges(mx, m):
    c, refs = edges_case(), refs_of(edges_case)
    k = EDGE_SIZES.index(m)
    assert len(c.sets[k]) == m and len(np.unique(c.sets[k])) == min(m, c.snps)
    reference_holds(c, refs, f"m {m}", only=[k])
    host = run(mx, c, [c.sets[k]], [c.weights[k]])
    accurate(host, refs, f"m {m}", only=[k])
    dev = run(mx, c, [c.sets[k]], [c.weights[k]], device=True)
    assert same_results(host, dev) and same_scan(host, dev)
    assert all(same(P, P.T.copy()) for P in host["phi"][0])


# ---- 3. the set of 1024 entries: two traits, two pieces, rows in place
@functools.lru_cache(maxsize=None)
def full_case():
    snps = 24
    rng = np.random.default_rng(53)
    sets = [np.concatenate([rng.permutation(snps), rng.integers(0, snps, 1024 - snps)])]
    return make_case(4099, snps, 2, 1, sets, [signed(rng, 1024)], seed=23)


def test_a_set_of_1024_entries_with_two_traits_two_pieces_and_rows_in_place(mx):
    c, refs = full_case(), refs_of(full_case)
    reference_holds(c, refs, "m 1024 indiv 4099")
    dev = run(mx, c, device=True)
    accurate(dev, refs, "m 1024 indiv 4099")
    host = run(mx, c)
    assert same_results(host, dev) and same_scan(host, dev)
    assert all(same(P, P.T.copy()) for P in dev["phi"][0])


# ---- 4. more than 256 (set, trait) items
@functools.lru_cache(maxsize=None)
def many_case():
    snps, nsets = 40, 140
    rng = np.random.default_rng(54)
    sizes = rng.integers(0, 20, nsets)
    sizes[[5, 77, nsets - 1]] = 0
    sizes[[0, 127, 128]] = [19, 17, 16]
    sets = [rng.integers(0, snps, m) for m in sizes]
    return make_case(131, snps, 2, 1, sets, [signed(rng, len(s)) for s in sets], seed=24)


def test_more_than_256_items(mx):
    c, refs = many_case(), refs_of(many_case)
    nsets = len(c.sets)
    sizes = [len(s) for s in c.sets]
    assert nsets * c.n == 280 and sizes[-1] == 0 and sum(m == 0 for m in sizes) >= 3 and max(sizes) == 19
    reference_holds(c, refs, "140 sets")
    got = run(mx, c, lds=nsets + 3)                                       # call() asserts that the rows nsets ... nsets + 2 of every column keep the sentinel
    accurate(got, refs, "140 sets")
    rng = np.random.default_rng(64)
    alone = sorted({0, nsets - 1, 127, 128} | set(int(k) for k in rng.choice(nsets, 18, replace=False)))
    assert len(alone) >= 20
    for k in alone:                                                       # the sets 127 and 128: items 254, 255 | 256, 257
        one = run(mx, c, [c.sets[k]], [c.weights[k]])
        assert same(one["stat"][0], got["stat"][k]) and same(one["phi"][0], got["phi"][k]), k
    for batch in (1, 50):
        cut = run(mx, c, env=dict(MXA_ASSOC_SET_BATCH=batch), lds=nsets + 3)
        assert same_results(got, cut) and same_scan(got, cut), batch
    for k, m in enumerate(sizes):
        if m == 0:
            assert np.array_equal(got["stat"][k], np.zeros((c.n, 6))), k


# ---- 5. pointer kinds crossed
def test_every_combination_of_host_and_device_operands_and_results(mx):
    codes, X, R, Wt, H, sets, weights = case(255, 3, 4, 0.05, True)
    base = call(mx, X, 255, R, Wt, H, sets, weights)
    for dev_out in (False, True):
        for mask in range(16):
            dev_ops = tuple(bool(mask >> b & 1) for b in range(4))          # plink, R, Wt, H
            got = call(mx, X, 255, R, Wt, H, sets, weights, dev_ops=dev_ops, dev_out=dev_out)
            assert same_results(base, got) and same_scan(base, got), (dev_ops, dev_out)
    env = dict(MXA_ASSOC_SET_BATCH=20, MXA_ASSOC_CHUNK_ROWS=7)
    for dev_ops, dev_out in (((True, False, False, False), False), ((False, True, True, True), True)):
        got = call(mx, X, 255, R, Wt, H, sets, weights, dev_ops=dev_ops, dev_out=dev_out, env=env)
        assert same_results(base, got) and same_scan(base, got), (dev_ops, dev_out, env)


# ---- 6. leading dimensions, and the scan's own U at ldo
def test_leading_dimensions_and_omitted_scan_results(mx):
    indiv, n = 255, 3
    codes, X, R, Wt, H, sets, weights = case(indiv, n, 4, 0.05, True)
    nsets, snps = len(sets), X.shape[0]
    base = call(mx, X, indiv, R, Wt, H, sets, weights)
    for device in (False, True):
        for scan in (True, False):                                          # device, scan False: the stage reads the U the scan allocated itself, ld ldo
            for phi in (True, False):
                got = call(mx, X, indiv, R, Wt, H, sets, weights, scan=scan, phi=phi, device=device, ld=(indiv + 3, indiv + 1, indiv + 2), ldo=snps + 5,
                           lds=nsets + 2)                                   # call(): NaN behind every operand column, nothing written behind a result column
                assert same(base["stat"], got["stat"]), (device, scan, phi)
                assert not phi or same_results(base, got), (device, scan, phi)
                assert not scan or same_scan(base, got), (device, scan, phi)


# ---- 7. base pointers off alignment
@functools.lru_cache(maxsize=None)
def unaligned_case():
    snps = 24
    rng = np.random.default_rng(57)
    sets = [rng.integers(0, snps, 17), rng.integers(0, snps, 33)]
    return make_case(259, snps, 2, 1, sets, [signed(rng, len(s)) for s in sets], seed=27)


def test_operands_that_start_off_a_16_and_64_byte_boundary(mx):
    c = unaligned_case()
    assert c.X.shape[1] == 65
    byte_offsets, wide_offsets = tuple(op.BYTE_OFFSETS) + (16, 17), tuple(op.WIDE_OFFSETS) + (2, 3)
    for device in (False, True):
        base = run(mx, c, device=device, offsets=(0, 0, 0, 0))
        assert same_results(base, run(mx, c, device=device))
        for i, off in enumerate(byte_offsets):                              # plink alone, then with R, Wt and H shifted as well (each wide offset at each of them)
            w = [wide_offsets[(i + j) % len(wide_offsets)] for j in range(3)]
            for offsets in ((off, 0, 0, 0), (off, w[0], w[1], w[2])):
                got = run(mx, c, device=device, offsets=offsets)
                assert same_results(base, got) and same_scan(base, got), (device, offsets)
        for k in (1, 2, 3):                                                 # R, Wt, H one at a time
            for w in wide_offsets:
                offsets = tuple(w if j == k else 0 for j in range(4))
                got = run(mx, c, device=device, offsets=offsets)
                assert same_results(base, got) and same_scan(base, got), (device, offsets)


# ---- 8. many rows
@functools.lru_cache(maxsize=None)
def rows_case():
    snps = 700
    rng = np.random.default_rng(58)
    marks = np.array([0, 1, 255, 256, 257, 511, 512, 698, 699])
    apart = np.array([0, 2, 255, 257, 509, 511, 696, 699, 100])
    assert np.all(np.diff(np.sort(apart)) > 1)                              # no two bounce rows are neighbours
    sets = [rng.permutation(np.concatenate([marks, rng.integers(0, snps, 11)])), rng.permutation(np.arange(250, 262)), apart, np.array([snps - 1]),
            np.concatenate([rng.integers(0, snps, 31), [256, 512]])]
    return make_case(67, snps, 2, 1, sets, [signed(rng, len(s)) for s in sets], seed=28)


def test_row_numbers_up_to_699(mx):
    c, refs = rows_case(), refs_of(rows_case)
    reference_holds(c, refs, "700 rows")
    host = run(mx, c)
    accurate(host, refs, "700 rows")
    for kw in (dict(device=True), dict(env=dict(MXA_ASSOC_CHUNK_ROWS=37)), dict(device=True, env=dict(MXA_ASSOC_CHUNK_ROWS=37)),
               dict(env=dict(MXA_ASSOC_SET_BATCH=1)), dict(env=dict(MXA_ASSOC_SET_BATCH=1, MXA_ASSOC_CHUNK_ROWS=37)),      # every set alone in its batch
               dict(device=True, env=dict(MXA_ASSOC_SET_BATCH=1))):
        got = run(mx, c, **kw)
        assert same_results(host, got) and same_scan(host, got), kw


# ---- 9. weights and degenerate calls
@functools.lru_cache(maxsize=None)
def weights_case():
    snps = 24
    rng = np.random.default_rng(59)
    sets = [rng.integers(0, snps, 17), rng.integers(0, snps, 33), rng.permutation(snps)[:5], rng.permutation(snps)[:16]]
    weights = [signed(rng, len(s)) for s in sets]
    weights[0][[0, 5, 16]] = 0.0
    weights[1][rng.permutation(33)[:9]] = 0.0
    weights[2][:] = 0.0
    assert all((w > 0).any() and (w < 0).any() for k, w in enumerate(weights) if k != 2)
    return make_case(257, snps, 2, 1, sets, weights, seed=29)


def test_weights_of_both_signs_zeros_and_sign_flips(mx):
    c, refs = weights_case(), refs_of(weights_case)
    reference_holds(c, refs, "weights")
    got = run(mx, c)
    accurate(got, refs, "weights")
    zero = got["stat"][2]
    print("all-zero weights, the six statistics per trait:", zero.tolist(), "sign bits:", np.signbit(zero).astype(int).tolist())
    assert np.all(zero == 0.0)                                              # six exact zeros (every SNP of the set has a called individual: reference_holds)
    flipped = run(mx, c, c.sets, [-w for w in c.weights])
    assert all(same(a, b) for a, b in zip(flipped["phi"], got["phi"]))
    for k in (0, 1, 3):
        assert np.all(got["stat"][k][:, 0] != 0.0)
        assert same(flipped["stat"][k][:, 0], -got["stat"][k][:, 0]), k     # the sign bit of B
        assert same(flipped["stat"][k][:, 1:], got["stat"][k][:, 1:]), k    # varB, Q, c1, c2, c4
    assert np.all(flipped["stat"][2] == 0.0)
    dev = run(mx, c, device=True)
    assert same_results(got, dev)


@pytest.mark.parametrize("device", [False, True])
@pytest.mark.parametrize("weighted", [False, True])
def test_a_call_whose_sets_are_all_empty(mx, device, weighted):
    c = weights_case()
    sets = [np.zeros(0, np.int64)] * 3
    got = run(mx, c, sets, [np.zeros(0)] * 3 if weighted else None, device=device)        # call(): return 0, the two sentinels of the phi array untouched
    assert got["stat"].shape == (3, c.n, 6) and np.all(got["stat"] == 0.0) and all(P.size == 0 for P in got["phi"])
    plain = run(mx, c)
    assert same_scan(plain, got)


# ---- 10. the p-values of the wrapper
def skat_moments(Q, c1, c2, c4):
    """l = c2^2 / c4 and x = (Q - c1) sqrt(l / c2) + l of the header, as mpmath numbers at 50 digits"""
    import mpmath
    with mpmath.workdps(50):
        Q, c1, c2, c4 = (mpmath.mpf(float(v)) for v in (Q, c1, c2, c4))
        l = c2 * c2 / c4
        return l, (Q - c1) * mpmath.sqrt(l / c2) + l


def burden_line(B, varB):
    """the header's line: erfc(|B| / sqrt(2 varB)); (nan, nan) where the argument is not finite"""
    try:
        v = abs(B) / math.sqrt(2.0 * varB)
    except (ValueError, ZeroDivisionError):
        return math.nan, math.nan
    return (v, math.erfc(v)) if math.isfinite(v) else (v, math.nan)


def check_p_values(res, label):
    """burden_p against the header's line bit for bit and against mpmath's erfc of the same B and varB; skat_p and skat_df against mpmath.
    The bound of burden_p against erfc(v) at 50 digits, v = |B| / sqrt(2 varB), has two parts.  The argument: the double v carries at most three roundings
    (2 varB, the root, the quotient), a relative error of at most 3 u, u = 2^-53; and |d ln erfc(v) / d ln v| = v (2 / sqrt pi) exp(-v^2) / erfc(v) <=
    v (v + sqrt(v^2 + 2)) <= 2 v^2 + 2 v by erfc(v) >= (2 / sqrt pi) exp(-v^2) / (v + sqrt(v^2 + 2)): at most 3 u (2 v'^2 + 2 v') with v' = v (1 + 3 u).  The
    host libm: the largest relative error of math.erfc against mpmath at the doubles v of this very test, measured here, printed, and allowed twice over.
    Returns (the libm term, the largest relative errors of burden_p, skat_p)."""
    import mpmath
    u = 2.0 ** -53
    B, vB, Q, c1, c2, c4 = (np.asarray(a, np.float64).reshape(-1) for a in (res.burden, res.burden_var, res.skat, res.c1, res.c2, res.c4))
    bp, sp, df = (np.asarray(a, np.float64).reshape(-1) for a in (res.burden_p, res.skat_p, res.skat_df))
    lines = [burden_line(float(b), float(v)) for b, v in zip(B, vB)]
    with mpmath.workdps(50):
        libm = max([float(abs(mpmath.mpf(p) - mpmath.erfc(mpmath.mpf(v))) / mpmath.erfc(mpmath.mpf(v))) for v, p in lines if math.isfinite(v) and p > 0] + [0.0])
    print(f"{label} libm: largest relative error of math.erfc over {len(lines)} arguments {libm:.3e} = {libm / u:.2f} u")
    worst_b = worst_s = 0.0
    live = ones = 0
    for i, (v, p) in enumerate(lines):
        assert np.array([bp[i]]).tobytes() == np.array([p]).tobytes() or (math.isnan(p) and math.isnan(bp[i])), (label, "burden_p", i, bp[i], p)
        assert math.isnan(bp[i]) == (not math.isfinite(v)), (label, i)
        if math.isfinite(v):
            with mpmath.workdps(50):
                ref = mpmath.erfc(abs(mpmath.mpf(float(B[i]))) / mpmath.sqrt(2 * mpmath.mpf(float(vB[i]))))
                err = float(abs(mpmath.mpf(float(bp[i])) - ref) / ref) if float(ref) > 0.0 else 0.0
            v1 = v * (1 + 3 * u)
            bound = 3 * u * (2 * v1 * v1 + 2 * v1) + 2 * libm
            worst_b = max(worst_b, err)
            assert err <= bound, (label, "burden_p against mpmath", i, err, bound)
        if not (c2[i] > 0.0 and c4[i] > 0.0):
            assert math.isnan(sp[i]) and math.isnan(df[i]), (label, "skat_p", i)
            continue
        live += 1
        l, x = skat_moments(Q[i], c1[i], c2[i], c4[i])
        near = float(l)
        assert df[i] in (near, np.nextafter(near, np.inf), np.nextafter(near, -np.inf)), (label, "skat_df", i, df[i], near)
        if x <= 0:
            ones += 1
            assert sp[i] == 1.0, (label, "skat_p", i)
            continue
        ref = sr.upper_gamma(l, x)
        if float(ref) > 0.0:
            with mpmath.workdps(50):
                err = float(abs(mpmath.mpf(float(sp[i])) - ref) / ref)
            worst_s = max(worst_s, err)
            assert err <= 2.0 ** -40, (label, "skat_p", i, err)
    print(f"{label} {len(lines)} items, {live} with positive moments, {ones} with x <= 0: burden_p against mpmath {worst_b:.3e}, skat_p {worst_s:.3e} (bound 2^-40 = {2.0 ** -40:.3e})")
    return libm, worst_b, worst_s


@pytest.mark.parametrize("which", ["items", "sizes"])
def test_the_p_values_of_the_wrapper(mx, which):
    c = many_case() if which == "items" else edges_case()
    res = mx.assoc_set(c.X, c.snps, c.indiv, c.R, c.Wt, c.H, c.sets, c.weights)
    assert res.skat_p.shape == (len(c.sets), c.n)
    raw = run(mx, c, phi=False)                                             # the wrapper hands over what the entry returned
    for t, field in enumerate(("burden", "burden_var", "skat", "c1", "c2", "c4")):
        assert same(getattr(res, field), raw["stat"][:, :, t]), field
    empty = np.array([len(s) == 0 for s in c.sets])
    assert np.all(np.isnan(res.skat_p[empty])) and np.all(np.isnan(res.burden_p[empty])) and not np.any(np.isnan(res.skat_p[~empty]))
    libm, _, _ = check_p_values(res, f"p-values {which}")
    print(f"p-values {which}: the libm term is {libm / 2.0 ** -53:.2f} u (above 16 u it is to be reported)")
