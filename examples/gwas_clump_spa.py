#!/usr/bin/env python3
"""A case / control scan with few cases, clumped on saddlepoint p-values: a synthetic genome with LD, rare and common alleles and 2 % missing calls, a trait
with 5 % cases (the liability above its 95 % quantile, 12 causal SNPs, two covariates) -> assoc_logistic(spa=True): the logistic score test of every SNP, and
for the SNPs with |z| >= 2 the saddlepoint p-value in the place of the normal one -> ld_prune(priority=log p, pairwise=True, return_owner=True): the clumps of
PLINK's --clump.  Prints how many SNPs pass the threshold by the normal p-value erfc(|z| / sqrt 2) and by the saddlepoint one (with few cases the normal
p-value is too small, the more so the rarer the allele), the largest correction among the SNPs that only the normal p-value lets pass, and how many causal
SNPs lie in a significant clump.

usage: gwas_clump_spa.py [--snps 4000] [--indiv 4000] [--causal 12] [--r2 0.2] [--window 100] [--p 1e-5]"""
import argparse
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

import miraculix_amd as mx
from miraculix_amd import crossproduct as cp


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--snps", type=int, default=4000)
    ap.add_argument("--indiv", type=int, default=4000)
    ap.add_argument("--causal", type=int, default=12)
    ap.add_argument("--r2", type=float, default=0.2)
    ap.add_argument("--window", type=int, default=100, help="SNPs behind a SNP that may share its clump")
    ap.add_argument("--p", type=float, default=1e-5, help="the p-value of a significant clump")
    a = ap.parse_args()
    mx.load_shared_library()
    rng = np.random.default_rng(2)
    snps, indiv = a.snps, a.indiv
    # genotypes with LD: a SNP is a fresh draw (a third of them rare: MAF 0.5-2 %) or a noisy copy of its predecessor; every SNP polymorphic
    Z = np.empty((snps, indiv), np.int8)
    for s in range(snps):
        if s == 0 or rng.random() < 0.15:
            Z[s] = rng.binomial(2, rng.uniform(0.005, 0.02) if rng.random() < 1 / 3 else rng.uniform(0.05, 0.5), size=indiv)
        else:
            Z[s] = np.where(rng.random(indiv) < 0.05, rng.binomial(2, Z[s - 1].mean() / 2, size=indiv), Z[s - 1])
    const = Z.min(axis=1) == Z.max(axis=1)
    Z[const, 0] = 1 - np.minimum(Z[const, 0], 1)
    maf = np.minimum(Z.mean(axis=1) / 2, 1 - Z.mean(axis=1) / 2)
    # the trait: causal SNPs among the common ones, two covariates, 5 % cases
    Zs = Z.astype(np.float64)
    Zs = (Zs - Zs.mean(axis=1, keepdims=True)) / Zs.std(axis=1, keepdims=True)
    causal = np.sort(rng.choice(np.flatnonzero(maf > 0.05), a.causal, replace=False))
    g = Zs[causal].T @ rng.standard_normal(a.causal)
    g *= np.sqrt(0.5 / g.var())
    W = np.column_stack([rng.standard_normal(indiv), rng.integers(0, 2, indiv).astype(np.float64)])
    liability = g + W @ np.array([0.3, -0.4]) + rng.standard_normal(indiv) * np.sqrt(0.5)
    cases = (liability > np.quantile(liability, 0.95)).astype(np.float64)
    code = np.where(rng.random((snps, indiv)) < 0.02, 1, np.where(Z == 0, 0, Z + 1)).astype(np.uint8)
    code = np.concatenate([code, np.zeros((snps, (-indiv) % 4), np.uint8)], axis=1).reshape(snps, -1, 4)
    plink = np.ascontiguousarray(code[:, :, 0] | (code[:, :, 1] << 2) | (code[:, :, 2] << 4) | (code[:, :, 3] << 6))

    res = mx.assoc_logistic(plink, snps, indiv, cases, covariates=W, spa=True, z_cutoff=2.0)
    ok = res.flag != 3
    normal = np.array([math.erfc(abs(z) / math.sqrt(2.0)) if f != 3 else 1.0 for z, f in zip(res.z, res.flag)])
    p = np.where(ok, res.pval, 1.0)                                                    # an uninformative SNP goes last
    print(f"{snps} SNPs x {indiv} individuals, {int(cases.sum())} cases ({100 * cases.mean():.1f} %), {int((maf < 0.02).sum())} SNPs below MAF 2 %: flags 0 / 1 / 2 / 3 = "
          f"{np.bincount(res.flag, minlength=4).tolist()}")
    by_normal, by_spa = normal <= a.p, p <= a.p
    near = np.zeros(snps, bool)
    for c in causal:
        near[max(0, c - a.window):c + a.window + 1] = True
    print(f"p <= {a.p:g}: {int(by_normal.sum())} SNPs by the normal p-value ({int((by_normal & ~near).sum())} of them further than {a.window} SNPs from every causal one), "
          f"{int(by_spa.sum())} by the saddlepoint p-value ({int((by_spa & ~near).sum())})")
    lost = by_normal & ~by_spa
    if lost.any():
        worst = int(np.argmax(np.where(lost, np.log(p) - np.log(np.maximum(normal, 1e-300)), -np.inf)))
        print(f"largest correction among them: SNP {worst}, MAF {maf[worst]:.4f}, z = {res.z[worst]:.2f}: normal p {normal[worst]:.2e}, saddlepoint p {p[worst]:.2e}")
    keep, owner = cp.ld_prune(plink, snps, indiv, window=a.window, min_r2=a.r2, priority=np.log(np.maximum(p, 1e-300)), pairwise=True, return_owner=True)
    index = np.flatnonzero(keep & by_spa)
    in_clump = np.isin(owner[causal], index)
    print(f"clumping at r^2 >= {a.r2:g} within {a.window} SNPs by the saddlepoint p-value: {int(keep.sum())} clumps, {len(index)} with p <= {a.p:g}; causal SNPs in "
          f"such a clump: {int(in_clump.sum())} of {a.causal}")
    assert np.all(p[ok] > 0) and np.all(p[ok] <= 1.0 + 1e-12), "a p-value is out of range"
    print("PASS")


if __name__ == "__main__":
    main()
