#!/usr/bin/env python3
"""Gene-based tests of rare variants: a synthetic exome of genes (sets of neighbouring rare SNPs, MAF 0.2-2 %, 2 % missing calls), a case / control trait from
a logistic model with two covariates in which a few genes are causal -- some with all their rare alleles raising the risk (what the burden test is made for),
some with effects of both signs (what SKAT is made for) -> assoc_logistic_sets: the logistic null on the host, the score scan and the set stage on the device,
weights omega = 1 / sqrt(f (1 - f)).  Prints the top genes by the smaller of the two p-values and where the causal genes rank.

usage: gene_based.py [--genes 300] [--size 12] [--indiv 6000] [--causal 6]"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

import miraculix_amd as mx


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--genes", type=int, default=300)
    ap.add_argument("--size", type=int, default=12, help="SNPs per gene")
    ap.add_argument("--indiv", type=int, default=6000)
    ap.add_argument("--causal", type=int, default=6)
    a = ap.parse_args()
    mx.load_shared_library()
    rng = np.random.default_rng(11)
    genes, m, indiv = a.genes, a.size, a.indiv
    snps = genes * m
    f = rng.uniform(0.002, 0.02, snps)
    Z = rng.binomial(2, f[:, None], size=(snps, indiv)).astype(np.int8)
    sets = [np.arange(g * m, (g + 1) * m) for g in range(genes)]
    causal = rng.choice(genes, a.causal, replace=False)
    effect = np.zeros(snps)
    kind = {}
    for i, g in enumerate(causal):
        hit = rng.choice(sets[g], max(2, m // 2), replace=False)
        if i % 2 == 0:
            effect[hit], kind[g] = 1.1, "one sign"
        else:
            effect[hit], kind[g] = 1.6 * rng.choice([-1.0, 1.0], len(hit)), "both signs"
    W = np.column_stack([rng.standard_normal(indiv), rng.integers(0, 2, indiv).astype(np.float64)])
    eta = -0.4 + W @ np.array([0.3, -0.4]) + effect @ (Z - 2 * f[:, None])
    cases = (rng.random(indiv) < 1 / (1 + np.exp(-eta))).astype(np.float64)
    code = np.where(rng.random((snps, indiv)) < 0.02, 1, np.where(Z == 0, 0, Z + 1)).astype(np.uint8)
    code = np.concatenate([code, np.zeros((snps, (-indiv) % 4), np.uint8)], axis=1).reshape(snps, -1, 4)
    plink = np.ascontiguousarray(code[:, :, 0] | (code[:, :, 1] << 2) | (code[:, :, 2] << 4) | (code[:, :, 3] << 6))
    maf = np.maximum(Z.mean(axis=1) / 2, 0.5 / indiv)
    weights = [1 / np.sqrt(maf[s] * (1 - maf[s])) for s in sets]

    res = mx.assoc_logistic_sets(plink, snps, indiv, cases, W, sets, weights)
    assert res.skat.shape == (genes,) and np.all(np.isfinite(res.burden_p)) and np.all(np.isfinite(res.skat_p)), "a gene without a test"
    best = np.minimum(res.burden_p, res.skat_p)
    order = np.argsort(best)
    rank = {int(g): int(np.flatnonzero(order == g)[0]) + 1 for g in causal}
    print(f"{genes} genes of {m} rare SNPs x {indiv} individuals, {int(cases.sum())} cases ({100 * cases.mean():.1f} %), {len(causal)} causal genes")
    print("  gene   burden z    burden p      SKAT Q      df      SKAT p   causal")
    for g in order[:max(10, a.causal + 4)]:
        print(f"{g:6d}  {res.burden[g] / np.sqrt(res.burden_var[g]):9.2f}  {res.burden_p[g]:10.2e}  {res.skat[g]:10.1f}  {res.skat_df[g]:6.2f}  {res.skat_p[g]:10.2e}   " +
              (kind[int(g)] if int(g) in kind else "-"))
    print("ranks of the causal genes by min(burden p, SKAT p): " + ", ".join(f"gene {g} ({kind[g]}): {r}" for g, r in sorted(rank.items(), key=lambda t: t[1])))
    null = np.setdiff1d(np.arange(genes), causal)
    print(f"share of the {len(null)} other genes with p < 0.05: burden {float((res.burden_p[null] < 0.05).mean()):.3f}, SKAT {float((res.skat_p[null] < 0.05).mean()):.3f}")
    assert sum(r <= 2 * len(causal) for r in rank.values()) >= (len(causal) + 1) // 2, "most causal genes should rank at the top"
    print("PASS")


if __name__ == "__main__":
    main()
