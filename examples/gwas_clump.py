#!/usr/bin/env python3
"""A genome-wide association scan and its clumping on the device, from packed genotypes and a phenotype to index SNPs: a synthetic genome with LD and 2 % missing
calls, a trait with 20 causal SNPs and two covariates -> assoc_linear (beta, se, t per SNP: y ~ 1 + covariates + x_s, missing calls imputed by the SNP's mean)
-> ld_prune(priority=-|t|, pairwise=True, return_owner=True), the clumps of PLINK's --clump with |t| in the place of the p-value (the same order).  Prints how
many causal SNPs are the index SNP of a clump or lie in the clump of a significant one, and the mean of t^2 by LD-score bin (ld_window_scores_pairwise): the
relation LD-score regression fits.  With --binary the trait is a case / control status (the liability above its 70 % quantile) and the scan is the logistic
score test: assoc_logistic (the null model logit P(y = 1) = [1 | covariates] gamma fitted once on the host, then score, var and z = U / sqrt(V) per SNP), clumped
by -|z|.

usage: gwas_clump.py [--snps 6000] [--indiv 1500] [--chromosomes 3] [--cm 1.0] [--causal 20] [--h2 0.4] [--r2 0.2] [--binary]"""
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
    ap.add_argument("--indiv", type=int, default=1500)
    ap.add_argument("--chromosomes", type=int, default=3)
    ap.add_argument("--cm", type=float, default=1.0)
    ap.add_argument("--causal", type=int, default=20)
    ap.add_argument("--h2", type=float, default=0.4)
    ap.add_argument("--r2", type=float, default=0.2)
    ap.add_argument("--binary", action="store_true", help="a case / control trait, scanned by the logistic score test (assoc_logistic)")
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
    chrom = np.sort(rng.integers(0, a.chromosomes, size=snps)).astype(np.int32)
    cm = np.concatenate([np.cumsum(rng.exponential(0.01, size=int(k))) for k in np.bincount(chrom, minlength=a.chromosomes) if k])
    last, _ = cp.ld_window_bounds(cm, chrom, max_dist=a.cm)
    # the trait: 20 causal SNPs, two covariates (one of them correlated with the genetic value), an offset
    Zs = Z.astype(np.float64)
    Zs = (Zs - Zs.mean(axis=1, keepdims=True)) / Zs.std(axis=1, keepdims=True)
    causal = np.sort(rng.choice(snps, a.causal, replace=False))
    g = Zs[causal].T @ rng.standard_normal(a.causal)
    g *= np.sqrt(a.h2 / g.var())
    W = np.column_stack([rng.standard_normal(indiv) + 0.3 * g, rng.integers(0, 2, indiv).astype(np.float64)])
    y = 170.0 + g + W @ np.array([0.5, -1.0]) + rng.standard_normal(indiv) * np.sqrt(1.0 - a.h2)
    # 2 % missing calls, PLINK coding (00 -> 0, 01 -> missing, 10 -> 1, 11 -> 2)
    code = np.where(rng.random((snps, indiv)) < 0.02, 1, np.where(Z == 0, 0, Z + 1)).astype(np.uint8)
    code = np.concatenate([code, np.zeros((snps, (-indiv) % 4), np.uint8)], axis=1).reshape(snps, -1, 4)
    plink = np.ascontiguousarray(code[:, :, 0] | (code[:, :, 1] << 2) | (code[:, :, 2] << 4) | (code[:, :, 3] << 6))

    if a.binary:
        cases = (y > np.quantile(y, 0.7)).astype(np.float64)                          # 30 % cases
        res = mx.assoc_logistic(plink, snps, indiv, cases, covariates=W)
        t = res.z                                                                     # z = U / sqrt(V) stands in the place of t below
        what = f"logistic score test, {int(cases.sum())} cases"
    else:
        res = mx.assoc_linear(plink, snps, indiv, y, covariates=W)
        t = res.t
        what = f"dof {res.dof}"
    stat = "z" if a.binary else "t"
    ok = np.isfinite(t)
    print(f"{snps} SNPs x {indiv} individuals on {a.chromosomes} chromosome(s), {a.causal} causal SNPs, 2 covariates: {what}, "
          f"{int(res.nobs.min())}..{int(res.nobs.max())} called individuals per SNP, {int((~ok).sum())} SNPs without a statistic")
    t = np.where(ok, t, 0.0)                                                          # an uninformative SNP goes last
    keep, owner = cp.ld_prune(plink, snps, indiv, last=last, min_r2=a.r2, priority=-np.abs(t), pairwise=True, return_owner=True)
    thresh = 5.0                                                                      # |t| of a genome-wide significant clump
    index = np.flatnonzero(keep & (np.abs(t) >= thresh))
    is_index = np.isin(causal, index)
    in_clump = np.isin(owner[causal], index)
    print(f"clumping at r^2 >= {a.r2:g} within {a.cm:g} cM by -|{stat}|: {int(keep.sum())} clumps, {len(index)} with |{stat}| >= {thresh:g}")
    print(f"causal SNPs that are the index SNP of such a clump: {int(is_index.sum())} of {a.causal}; in such a clump: {int(in_clump.sum())} of {a.causal}")
    # mean t^2 against LD score: SNPs that tag more of the genome carry more signal (the slope LD-score regression reads the heritability from)
    score = cp.ld_window_scores_pairwise(plink, snps, indiv, last, adjust=True)
    edges = np.quantile(score, [0.0, 0.25, 0.5, 0.75, 1.0])
    which = np.clip(np.searchsorted(edges, score, side="right") - 1, 0, 3)
    for b in range(4):
        sel = which == b
        print(f"  LD score {edges[b]:7.2f} .. {edges[b + 1]:7.2f}: mean {stat}^2 {float((t[sel] ** 2).mean()):7.2f} over {int(sel.sum())} SNPs")
    assert in_clump.sum() >= 1, "no causal SNP was found"
    print("PASS")


if __name__ == "__main__":
    main()
