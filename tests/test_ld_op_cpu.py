"""The LD operator object without a device: mxa_ld_op_bytes (the one entry that needs none) against numpy on the window families of the GPU tests, its error
cases, the references of tests/_ld_op_ref.py against each other, and the Python wrapper's argument checks, raised before any device call."""
import ctypes

import numpy as np
import pytest

import _ld_apply_ref as ar
import _ld_op_ref as opr
import _ld_ref as ref

SHAPES = (777, 130, 1300)


@pytest.fixture(scope="module")
def mx():
    import miraculix_amd as m
    m.load_shared_library()
    return m


def _windows(snps):
    out = {f"w={w}": ref.fixed_last(snps, w) for w in sorted({w for w in (0, 1, 255, 256, 257, snps - 1) if w < snps})}
    out["chromosomes"] = ar.chromosome_window(snps)
    if snps >= 777:
        out["clusters"] = ar.cluster_window(snps)
    for s in range(3):
        out[f"sweep {s}"] = ref.sweep_window(snps, s)
    return out


def _bytes(mx, snps, last):
    L = mx.lib.check_library_handle()
    e, b = ctypes.c_long(-5), ctypes.c_long(-5)
    rc = L.mxa_ld_op_bytes(snps, mx.lib.ptr(last), ctypes.byref(e), ctypes.byref(b))
    return rc, L.mxa_last_error(), e.value, b.value


@pytest.mark.parametrize("snps", SHAPES)
def test_bytes_is_the_entry_count_and_at_least_the_mirrored_rows(mx, snps):
    for name, last in _windows(snps).items():
        rc, err, entries, nbytes = _bytes(mx, snps, last)
        assert (rc, err) == (0, 0), name
        assert entries == int(ref.rowptr_of(last)[-1]), name
        first = ref.first_of(last)
        mirrored = int((last.astype(np.int64) - first + 1).sum())
        assert mirrored == 2 * entries - snps, name                      # every off-diagonal pair twice, the diagonal once
        assert nbytes >= 8 * (2 * entries - snps), name
        assert nbytes <= 8 * (2 * entries - snps) + 256 * snps, name     # the index arrays and the packing buffer: a fixed number of bytes per SNP
        assert mx.crossproduct.ld_op_bytes(last) == (entries, nbytes), name


def test_bytes_rejects_a_bad_window_and_null_pointers(mx):
    L, p = mx.lib.check_library_handle(), mx.lib.ptr
    snps = 12
    good = ref.fixed_last(snps, 3)
    e, b = ctypes.c_long(-5), ctypes.c_long(-5)

    def run(n=snps, last=good, pe=ctypes.byref(e), pb=ctypes.byref(b)):
        rc = L.mxa_ld_op_bytes(n, p(last), pe, pb)
        return rc, L.mxa_last_error(), e.value, b.value

    untouched = (1, 1, -5, -5)
    below, beyond, decreasing = good.copy(), good.copy(), good.copy()
    below[4] = 3
    beyond[-1] = snps
    decreasing[5] = decreasing[4] - 1
    for bad in (dict(last=below), dict(last=beyond), dict(last=decreasing), dict(n=0), dict(n=-3), dict(last=None), dict(pe=None), dict(pb=None)):
        assert run(**bad) == untouched, bad
    assert run()[:2] == (0, 0)


def test_the_references_agree_with_each_other():
    snps = 60
    last = ref.sweep_window(snps, 1)
    X = np.random.default_rng(2).integers(-3, 4, (snps, 4)).astype(np.float64)
    for make in (opr.dyadic_rows, opr.decay_rows):
        rows = make(last)
        T = ar.dense(rows, last)
        W = opr.windowed(T, last)
        assert np.array_equal(W, W.T) and np.all(np.diag(W) == 1.0) and np.isfinite(W).all()
        assert np.array_equal(rows * 1024, np.round(rows * 1024)) and np.abs(rows).max() == 1.0
        want, _, _ = ar.apply_ref(T, last, X)                            # math.fsum of the products: exact here, as every sum order is
        assert np.array_equal(opr.apply_exact(W, X, -2.0), want - 2.0 * X), make.__name__
    W = opr.windowed(ar.dense(opr.decay_rows(last), last), last)
    assert np.linalg.eigvalsh(W + 1.5 * np.eye(snps)).min() > 0
    b = np.random.default_rng(3).standard_normal(snps)
    x, it, rel, st = opr.cg(W, 1.5, b, 1e-10, 1000)
    assert st == 0 and rel <= 1e-10 and 1 <= it <= snps
    assert opr.true_relres(W, 1.5, x[:, None], b[:, None])[0] <= 2e-10
    assert opr.cg(W, 1.5, np.zeros(snps), 1e-10, 1000)[1:] == (0, 0.0, 0)
    assert opr.cg(W, 1.5, b, 1e-10, 3)[1::2] == (3, 1)
    assert opr.cg(W - 10.0 * np.eye(snps), 0.0, b, 1e-10, 1000)[3] == 2              # negative definite: breakdown at once
    assert opr.cg(np.eye(snps), 0.5, b, 1e-10, 1000)[1] == 1                         # a multiple of the identity: one iteration


def test_python_argument_checks_raise_before_any_device_call(mx):
    cp = mx.crossproduct
    snps, indiv = 6, 8
    X, f, last = np.zeros((snps, 2), np.uint8), np.full(snps, 0.25), np.full(snps, snps - 1, np.int32)
    create = cp.LdOperator.create
    with pytest.raises(ValueError, match="kind needs to be"):
        create(X, snps, indiv, window=2, kind="r2_adj", allele_freq=f)
    with pytest.raises(ValueError, match="Allele frequencies"):
        create(X, snps, indiv, window=2)
    for bad in (dict(), dict(last=last, window=2)):
        with pytest.raises(ValueError, match="exactly one of last and window"):
            create(X, snps, indiv, allele_freq=f, **bad)
    with pytest.raises(ValueError, match="Window needs to be in"):
        create(X, snps, indiv, window=snps, pairwise=True)
    with pytest.raises(ValueError, match="last needs"):
        create(X, snps, indiv, last=last[::-1] - 1, pairwise=True)
    with pytest.raises(ValueError, match="Matrix has wrong dimensions"):
        create(X[:-1], snps, indiv, window=2, pairwise=True)
    with pytest.raises(ValueError, match="rows needs to be"):
        cp.LdOperator.from_rows(last, np.ones(5))
    with pytest.raises(ValueError, match="last needs"):
        cp.LdOperator.from_rows(np.zeros(snps, np.int32), np.ones(snps))
    with pytest.raises(ValueError, match="last needs"):
        cp.ld_op_bytes(np.array([1, 0], np.int32))
    # an operator object whose handle is gone: every method refuses, free() is a no-op
    op = cp.LdOperator(None, snps, last)
    assert op.entries == snps * (snps + 1) // 2 and op.nbytes >= 8 * snps * snps
    for call in (lambda: op.apply(np.ones(snps)), lambda: op.solve(np.ones(snps), 1.0), lambda: op.rows()):
        with pytest.raises(RuntimeError, match="has been freed"):
            call()
    op.free()
    op.free()
