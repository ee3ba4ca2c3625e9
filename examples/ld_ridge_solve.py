#!/usr/bin/env python3
"""Ridge regression on summary statistics, beta = (R_w + lambda I)^-1 beta_hat -- the system behind LDpred-inf and SBLUP -- on a synthetic genome: genotypes
with LD, a 1 cM window that stops at chromosome ends (ld_window_bounds), marginal effects beta_hat = Z_s^T y / indiv of a simulated trait.  The windowed LD matrix is
staged ONCE on the device (LdOperator.create), then solved by conjugate gradients there for several lambda without repeating a genotype product; the example
checks every solution by applying the operator to it (one more pass over the resident matrix).

usage: ld_ridge_solve.py [--snps 6000] [--indiv 400] [--chromosomes 3] [--cm 1.0] [--causal 50] [--h2 0.5]"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

import miraculix_amd as mx
from miraculix_amd import crossproduct as cp


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--snps", type=int, default=6000)
    ap.add_argument("--indiv", type=int, default=400)
    ap.add_argument("--chromosomes", type=int, default=3)
    ap.add_argument("--cm", type=float, default=1.0)
    ap.add_argument("--causal", type=int, default=50)
    ap.add_argument("--h2", type=float, default=0.5)
    a = ap.parse_args()
    mx.load_shared_library()
    rng = np.random.default_rng(1)
    snps, indiv = a.snps, a.indiv
    # genotypes with LD: a SNP is a fresh draw or a noisy copy of its predecessor; every SNP polymorphic
    Z = np.empty((snps, indiv), np.int8)
    for s in range(snps):
        if s == 0 or rng.random() < 0.1:
            Z[s] = rng.binomial(2, rng.uniform(0.1, 0.9), size=indiv)
        else:
            Z[s] = np.where(rng.random(indiv) < 0.1, rng.integers(0, 3, size=indiv), Z[s - 1])
    const = Z.min(axis=1) == Z.max(axis=1)
    Z[const, 0], Z[const, 1] = 0, 2
    code = np.where(Z == 0, 0, Z + 1).astype(np.uint8)
    code = np.concatenate([code, np.zeros((snps, (-indiv) % 4), np.uint8)], axis=1).reshape(snps, -1, 4)
    plink = np.ascontiguousarray(code[:, :, 0] | (code[:, :, 1] << 2) | (code[:, :, 2] << 4) | (code[:, :, 3] << 6))
    f = Z.astype(np.float64).mean(axis=1) / 2.0
    chrom = np.sort(rng.integers(0, a.chromosomes, size=snps)).astype(np.int32)
    cm = np.concatenate([np.cumsum(rng.exponential(0.01, size=int(k))) for k in np.bincount(chrom, minlength=a.chromosomes) if k])
    last, _ = cp.ld_window_bounds(cm, chrom, max_dist=a.cm)
    # a trait and its marginal effects on standardised genotypes
    Zs = Z.astype(np.float64)
    Zs = (Zs - Zs.mean(axis=1, keepdims=True)) / Zs.std(axis=1, keepdims=True)
    beta = np.zeros(snps)
    beta[rng.choice(snps, a.causal, replace=False)] = rng.standard_normal(a.causal)
    g = Zs.T @ beta
    y = g * np.sqrt(a.h2 / g.var()) + rng.standard_normal(indiv) * np.sqrt(1.0 - a.h2)
    beta_hat = Zs @ (y - y.mean()) / indiv
    entries, nbytes = cp.ld_op_bytes(last)
    print(f"{snps} SNPs x {indiv} individuals on {a.chromosomes} chromosome(s); window {a.cm:g} cM: {entries} LD values, {nbytes / 1e6:.1f} MB on the device")
    with cp.LdOperator.create(plink, snps, indiv, last=last, kind="r", is_plink_format=True, allele_freq=f) as op:
        for lam in (snps / indiv, 0.1 * snps / indiv):                  # LDpred-inf's M / (N h2) at h2 = 1 and a tenth of it
            x, iters, relres, status = op.solve(beta_hat, lam, tol=1e-8, max_iter=2000)
            # the windowed matrix need not be positive definite: a shift that is too small shows as a breakdown, never as a wrong answer
            verdict = cp.LD_OP_STATUS[int(status[0])]
            res = np.linalg.norm(beta_hat - op.apply(x, shift=lam)) / np.linalg.norm(beta_hat)
            print(f"  lambda {lam:8.3f}: {verdict} after {int(iters[0])} iterations, recurrence residual {relres[0]:.2e}, true residual {res:.2e}; "
                  f"corr(beta, true effects) {np.corrcoef(x, beta)[0, 1]:.3f} (marginal {np.corrcoef(beta_hat, beta)[0, 1]:.3f})")
            assert status[0] != 0 or res <= 1e-7, "a converged solve left a residual"
    print("PASS")


if __name__ == "__main__":
    main()
