"""What the GPU tests of mxa_assoc_set share (tests/test_assoc_set_gpu.py, tests/test_assoc_set_limits_gpu.py): one raw call of the C entry with every operand
layout the header allows, the comparison on bytes, the accuracy rule, and the cases of the first module (cached, with their two reference evaluations).  The
library is never imported here: call() takes the loaded package as `mx`.

call            per operand host or device (plink, R, Wt, H each independently; the results all on one side), leading dimensions larger than the columns (NaN
                behind every column of an operand, a sentinel behind every column of a result), operands that start off a 64-byte boundary
                (tests/_operands.py::misaligned), the scan's outputs and phi given or omitted, environment variables for the one call.  It asserts what holds for
                every call: return 0, nothing written behind a column, behind row nsets - 1 of stat or behind the last block of phi, omitted results untouched,
                the operands unchanged.
check_accuracy  for Phi and each of the six statistics the scaled error against the long-double evaluation must not exceed 16 max(eps, 2^-48), eps = the
                scaled error of the float64 evaluation on the same case; every figure is printed before any is asserted.
"""
import functools
import os

import numpy as np

import _assoc_set_ref as sr
import _operands as op

LD = sr.LD
SNPS = 24
NAMES = ("B", "varB", "Q", "c1", "c2", "c4")
FILL = -7.5                                     # the sentinel of every result array
OPERANDS = ("plink", "R", "Wt", "H")


def make_sets(snps, seed):
    rng = np.random.default_rng([seed, 31])
    return [np.zeros(0, np.int64), np.array([snps - 1]), np.array([7, 7]), rng.permutation(snps)[:15], np.arange(4, 20), rng.integers(0, snps, 17),
            rng.integers(0, snps, 33)]


@functools.lru_cache(maxsize=None)
def case(indiv, n, kh, missing, weighted):
    codes, R, Wt, H = sr.random_case(indiv, SNPS, n, kh, seed=6, missing=missing)
    sets = make_sets(SNPS, indiv)
    rng = np.random.default_rng([indiv, 41])
    weights = [rng.uniform(0.3, 4.0, len(s)) for s in sets] if weighted else None
    X = sr.pack_dirty(codes, indiv)
    for a in (codes, R, Wt, H, X):
        a.setflags(write=False)
    return codes, X, R, Wt, H, sets, weights


@functools.lru_cache(maxsize=None)
def references(indiv, n, kh, missing, weighted):
    codes, _, R, Wt, H, sets, weights = case(indiv, n, kh, missing, weighted)
    return sr.set_reference(codes, R, Wt, H, sets, weights, LD), sr.set_reference(codes, R, Wt, H, sets, weights, np.float64)


def _dev(a):
    import torch
    return torch.from_numpy(np.array(a, order="C")).to("cuda:0")


def _columns(a, ld):
    """the columns of a (rows, cols) matrix as a C-ordered (cols, ld) array: column-major with leading dimension ld, NaN behind every column"""
    a = np.asarray(a)
    out = np.full((a.shape[1], ld), np.nan)
    out[:, :a.shape[0]] = a.T
    return out


def call(mx, X, indiv, R, Wt, H, sets, weights, scan=True, phi=True, device=False, env=None, dev_ops=None, dev_out=None, ld=None, ldo=None, lds=None,
         offsets=None):
    """one raw call of the C entry: dict(stat (nsets, n, 6), phi: list of (n, m, m) or None, score, var, z (snps, n), nobs) as numpy.
    device: where everything lies, unless dev_ops (four bools: plink, R, Wt, H) or dev_out (the results) say otherwise; ld = (ldr, ldw, ldh), ldo, lds: leading
    dimensions (default: indiv, snps, nsets + 1); offsets = (plink, R, Wt, H): elements behind a 64-byte boundary at which each operand starts (None: as the
    allocator gives it)"""
    L, p = mx.lib.check_library_handle(), mx.lib.ptr
    snps = X.shape[0]
    n = R.shape[1]
    kh = H.shape[1] // n
    dev_ops = (device,) * 4 if dev_ops is None else tuple(bool(d) for d in dev_ops)
    dev_out = device if dev_out is None else bool(dev_out)
    ldr, ldw, ldh = (indiv,) * 3 if ld is None else ld
    ldo = snps if ldo is None else ldo
    ptr = np.zeros(len(sets) + 1, np.int64)
    ptr[1:] = np.cumsum([len(s) for s in sets])
    idx = np.ascontiguousarray(np.concatenate([np.asarray(s, np.int32) for s in sets]) if ptr[-1] else np.zeros(1, np.int32), np.int32)
    wt = None if weights is None else np.ascontiguousarray(np.concatenate([np.asarray(w, np.float64) for w in weights] + [np.zeros(1)]))
    nsets, total = len(sets), int(sum(len(s) ** 2 for s in sets)) * n
    lds = nsets + 1 if lds is None else lds
    plain = [np.ascontiguousarray(X), _columns(R, ldr), _columns(Wt, ldw), _columns(H, ldh) if kh else None]
    ops = []
    for k, o in enumerate(plain):
        if o is None:
            ops.append(None)
        elif offsets is not None and offsets[k] is not None:
            ops.append(op.misaligned(np.array(o), offsets[k], dev_ops[k])[0])
        else:
            ops.append(_dev(o) if dev_ops[k] else o.copy())
    outs = dict(score=np.full((n, ldo), FILL), var=np.full((n, ldo), FILL), z=np.full((n, ldo), FILL), stat=np.full((6 * n, lds), FILL), phi=np.full(total + 2, FILL))
    nobs = np.full(snps, -3, np.int32)
    if dev_out:
        outs = {k: _dev(v) for k, v in outs.items()}
    old = {k: os.environ.get(k) for k in (env or {})}
    try:
        for k, v in (env or {}).items():
            os.environ[k] = str(v)
        rc = L.mxa_assoc_set(p(ops[0]), snps, indiv, p(ops[1]), ldr, p(ops[2]), ldw, p(ops[3]), ldh, n, kh, nsets, p(ptr), p(idx), p(wt),
                             p(outs["score"]) if scan else None, p(outs["var"]) if scan else None, p(outs["z"]) if scan else None, ldo, p(nobs) if scan else None,
                             p(outs["stat"]), lds, p(outs["phi"]) if phi else None)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    assert rc == 0, mx.lib.last_error()
    if dev_out or any(dev_ops):
        import torch
        torch.cuda.synchronize()
    if dev_out:
        outs = {k: v.cpu().numpy() for k, v in outs.items()}
    for o, before, name in zip(ops, plain, OPERANDS):                           # the operands are read only (their NaN padding included)
        assert o is None or same(op.readback(o), before), name
    assert np.all(outs["stat"][:, nsets:] == FILL) and np.all(outs["phi"][total:] == FILL)         # nothing beyond row nsets - 1, nothing behind the last block
    assert all(np.all(outs[k][:, snps:] == FILL) for k in ("score", "var", "z"))                   # nothing beyond row snps - 1 of a column
    if not phi:
        assert np.all(outs["phi"] == FILL)
    if not scan:
        assert all(np.all(outs[k] == FILL) for k in ("score", "var", "z")) and np.all(nobs == -3)
    res = dict(stat=outs["stat"][:, :nsets].reshape(n, 6, nsets).transpose(2, 0, 1).copy(), score=outs["score"][:, :snps].T, var=outs["var"][:, :snps].T,
               z=outs["z"][:, :snps].T, nobs=nobs, phi=None)
    if phi:
        res["phi"], at = [], 0
        for s in sets:
            m = len(s)
            res["phi"].append(outs["phi"][at:at + n * m * m].reshape(n, m, m).transpose(0, 2, 1).copy())
            at += n * m * m
    return res


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def same_results(a, b):
    ok = same(a["stat"], b["stat"])
    if a["phi"] is not None and b["phi"] is not None:
        ok = ok and len(a["phi"]) == len(b["phi"]) and all(same(x, y) for x, y in zip(a["phi"], b["phi"]))
    return ok


def same_scan(a, b):
    return all(same(a[k], b[k]) for k in ("score", "var", "z", "nobs"))


def check_accuracy(got, refs, label):
    ld, f64 = refs
    worst = {}
    for name, pick in [("Phi", lambda r: (r["phi"], r["sphi"]))] + [(NAMES[t], (lambda t: lambda r: (r["stat"][:, t], r["sstat"][:, t]))(t)) for t in range(6)]:
        eps = max(sr.scaled_error(pick(b)[0], *pick(a)) for a, b in zip(ld, f64))
        if name == "Phi":
            err = max(sr.scaled_error(g, *pick(a)) for a, g in zip(ld, got["phi"]))
        else:
            t = NAMES.index(name)
            err = max(sr.scaled_error(got["stat"][k, :, t], *pick(a)) for k, a in enumerate(ld))
        worst[name] = (err, eps)
        print(f"{label} {name:5s} scaled error {err:.3e}  eps {eps:.3e}  bound {16 * max(eps, sr.TOL):.3e}")
    for name, (err, eps) in worst.items():
        assert err <= 16 * max(eps, sr.TOL), (label, name, err, eps)
    return worst
