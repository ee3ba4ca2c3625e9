#!/usr/bin/env python3
"""A case / control scan with few cases, reported with effect sizes: a synthetic genome of rare and common alleles with 2 % missing calls, a trait with about
5 % cases from a logistic model (two covariates, causal SNPs with known log odds ratios, half of them rare) -> assoc_logistic(spa=True): the logistic score
test of every SNP with saddlepoint p-values -> the hits (p <= the threshold) -> assoc_logistic(firth=True) with z_cutoff at the weakest hit's |z|: the log odds
ratio, its standard error and the likelihood-ratio statistic of the hits by Firth-penalised fits on the device.  Prints one line per hit -- saddlepoint p-value,
the penalised estimate with its standard error, the one-step estimate U / V that a scan gives without a fit, and the truth for a causal SNP -- and how far the
two estimates lie from the truth over the causal hits.

usage: gwas_firth.py [--snps 3000] [--indiv 6000] [--causal 10] [--p 1e-4]"""
import argparse
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

import miraculix_amd as mx


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--snps", type=int, default=3000)
    ap.add_argument("--indiv", type=int, default=6000)
    ap.add_argument("--causal", type=int, default=10)
    ap.add_argument("--p", type=float, default=1e-4, help="the p-value of a hit")
    a = ap.parse_args()
    mx.load_shared_library()
    rng = np.random.default_rng(4)
    snps, indiv = a.snps, a.indiv
    # genotypes: a third of the SNPs rare (MAF 0.5-2 %), the others common; every SNP polymorphic
    f = np.where(rng.random(snps) < 1 / 3, rng.uniform(0.005, 0.02, snps), rng.uniform(0.05, 0.5, snps))
    Z = rng.binomial(2, f[:, None], size=(snps, indiv)).astype(np.int8)
    const = Z.min(axis=1) == Z.max(axis=1)
    Z[const, 0] = 1 - np.minimum(Z[const, 0], 1)
    maf = np.minimum(Z.mean(axis=1) / 2, 1 - Z.mean(axis=1) / 2)
    # the trait: half of the causal SNPs rare with a large effect, half common with a moderate one; two covariates; about 5 % cases
    rare, common = np.flatnonzero(maf < 0.02), np.flatnonzero(maf > 0.05)
    causal = np.concatenate([rng.choice(rare, a.causal // 2, replace=False), rng.choice(common, a.causal - a.causal // 2, replace=False)])
    truth = np.zeros(snps)
    truth[causal] = np.where(maf[causal] < 0.02, 1.6, 0.45) * rng.choice([-1.0, 1.0], len(causal), p=[0.2, 0.8])
    W = np.column_stack([rng.standard_normal(indiv), rng.integers(0, 2, indiv).astype(np.float64)])
    eta = math.log(0.04 / 0.96) + W @ np.array([0.3, -0.4]) + truth[causal] @ (Z[causal] - 2 * f[causal, None])
    cases = (rng.random(indiv) < 1 / (1 + np.exp(-eta))).astype(np.float64)
    code = np.where(rng.random((snps, indiv)) < 0.02, 1, np.where(Z == 0, 0, Z + 1)).astype(np.uint8)
    code = np.concatenate([code, np.zeros((snps, (-indiv) % 4), np.uint8)], axis=1).reshape(snps, -1, 4)
    plink = np.ascontiguousarray(code[:, :, 0] | (code[:, :, 1] << 2) | (code[:, :, 2] << 4) | (code[:, :, 3] << 6))

    spa = mx.assoc_logistic(plink, snps, indiv, cases, covariates=W, spa=True, z_cutoff=2.0)
    p = np.where(spa.flag != 3, spa.pval, 1.0)
    hits = np.flatnonzero(p <= a.p)
    print(f"{snps} SNPs x {indiv} individuals, {int(cases.sum())} cases ({100 * cases.mean():.1f} %), {int((maf < 0.02).sum())} SNPs below MAF 2 %: "
          f"{len(hits)} hits with a saddlepoint p-value <= {a.p:g}, {int(np.isin(causal, hits).sum())} of the {len(causal)} causal SNPs among them")
    if len(hits) == 0:
        print("no hit: nothing to fit")
        print("PASS")
        return
    cutoff = float(np.abs(spa.z[hits]).min())
    fit = mx.assoc_logistic(plink, snps, indiv, cases, covariates=W, firth=True, z_cutoff=cutoff)
    assert np.array_equal(fit.z.view(np.uint64), spa.z.view(np.uint64)), "the scan is the same in both calls"
    print(f"fits at |z| >= {cutoff:.2f}: flags 0 / 1 / 2 / 3 = {np.bincount(fit.flag, minlength=4).tolist()}")
    print("   SNP     MAF       z   saddlepoint p   log OR (Firth)     se    U / V   truth")
    for s in hits[np.argsort(p[hits])]:
        print(f"{s:6d}  {maf[s]:.4f}  {fit.z[s]:6.2f}  {p[s]:14.2e}  {fit.beta[s]:15.3f}  {fit.se[s]:5.3f}  {fit.score[s] / fit.var[s]:7.3f}  " +
              (f"{truth[s]:6.2f}" if truth[s] else "     -"))
    assert np.all(fit.flag[hits] == 1) and np.all(np.isfinite(fit.beta[hits])) and np.all(fit.se[hits] > 0), "a hit without a fit"
    found = np.intersect1d(hits, causal)
    if len(found):
        one_step = fit.score[found] / fit.var[found]
        print(f"over the {len(found)} causal hits: mean |estimate - truth| {np.abs(fit.beta[found] - truth[found]).mean():.3f} (Firth), "
              f"{np.abs(one_step - truth[found]).mean():.3f} (U / V)")
    print("PASS")


if __name__ == "__main__":
    main()
