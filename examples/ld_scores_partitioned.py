#!/usr/bin/env python3
"""Partitioned (stratified) LD scores l(i, c) = sum_j r2_ij a_jc in one call -- ldsc's --l2 --annot, the input of S-LDSC -- on a synthetic genome: chromosomes
with positions in centimorgans, a 1 cM window that stops at every chromosome end (ld_window_bounds), and an annotation matrix of a base column of ones plus a
few binary columns.  ld_scores_partitioned applies the window to the annotations without writing its rows; the base column is ld_window_scores up to the order
of the sums, which the example checks within the summation bound 2 m 2^-53 sum|t| (m terms per SNP, the same terms in two fixed orders).

usage: ld_scores_partitioned.py [--snps 6000] [--indiv 400] [--chromosomes 3] [--annot 4] [--cm 1.0] [--adjust]"""
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
    ap.add_argument("--annot", type=int, default=4, help="binary annotation columns next to the base column")
    ap.add_argument("--cm", type=float, default=1.0)
    ap.add_argument("--adjust", action="store_true", help="r^2 - (1 - r^2) / (indiv - 2), the estimator of LD-score regression")
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
    last, rowptr = cp.ld_window_bounds(cm, chrom, max_dist=a.cm)
    annot = np.ones((snps, 1 + a.annot))
    annot[:, 1:] = rng.random((snps, a.annot)) < rng.uniform(0.05, 0.5, size=a.annot)
    reach = last - np.arange(snps)
    print(f"{snps} SNPs x {indiv} individuals on {a.chromosomes} chromosome(s); window {a.cm:g} cM: reach mean {reach.mean():.1f}, max {reach.max()}; "
          f"{len(cp.ld_window_tiles(last))} tiles, {int(rowptr[-1])} pairs that are never stored")
    L = cp.ld_scores_partitioned(plink, snps, indiv, annot, last=last, adjust=a.adjust, is_plink_format=True, allele_freq=f)
    for c in range(annot.shape[1]):
        print(f"  annotation {c} ({'base' if c == 0 else f'{int(annot[:, c].sum())} SNPs'}): mean score {L[:, c].mean():.4f}")
    # the base column against the scores entry: the same terms, summed in two fixed orders
    S = cp.ld_window_scores(plink, snps, indiv, last, adjust=a.adjust, is_plink_format=True, allele_freq=f)
    first = np.searchsorted(last, np.arange(snps), side="left")
    m = (last - first + 1).astype(np.float64)
    r2max = 1.0 + (1.0 / (indiv - 2.0) if a.adjust else 0.0)            # |t| <= 1 + 1 / (indiv - 2): sum|t| <= m r2max
    err = np.abs(L[:, 0] - S)
    bound = 2.0 * m * 2.0 ** -53 * (m * r2max)
    print(f"base column against ld_window_scores: max |difference| {err.max():.3e}, bound {bound.max():.3e}")
    assert np.all(err <= bound), "the base column left the summation bound"
    print("PASS")


if __name__ == "__main__":
    main()
