#!/usr/bin/env python3
"""LD pruning and clumping of a whole PLINK fileset on the device: .bed + .bim (+ .fam) -> a subset of SNPs in which no two within N kb on one chromosome have
r^2 at or above T, chosen in priority order (what `plink --indep-pairwise` / `--clump` and bigsnpr's snp_clumping ask for).  read_bim gives chromosome and bp per
SNP, ld_window_bounds turns them into last[] (no device needed), and ld_prune -- on the pairwise-complete r, a real .bed has missing calls -- runs the pairs and
the greedy selection on the device: the pair list never reaches the host.  Twice: pruning by -MAF (the common allele first), and clumping by a p-value
(synthetic here: a seeded uniform draw; pass your own with --pvalues, one number per line in .bim order), where owner[] gives every dropped SNP's index SNP.

usage: ld_prune_genome.py data.bed [--kb 1000] [--r2 0.2] [--pvalues p.txt] [--out kept.snps]"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

import miraculix_amd as mx
from miraculix_amd import crossproduct as cp
from miraculix_amd import read_plink as rp


def maf_of(plink, snps, indiv):
    """minor allele frequency per SNP over the genotyped individuals (2-bit fields: 0 -> 0, 2 -> 1, 3 -> 2 copies, 1 missing)"""
    P = np.ascontiguousarray(plink, dtype=np.uint8).reshape(snps, -1)
    codes = np.stack([(P >> (2 * q)) & 3 for q in range(4)], axis=-1).reshape(snps, -1)[:, :indiv]
    present = codes != 1
    copies = np.where(codes == 2, 1, np.where(codes == 3, 2, 0))
    f = (copies * present).sum(axis=1) / np.maximum(2 * present.sum(axis=1), 1)
    return np.minimum(f, 1.0 - f)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("bed")
    ap.add_argument("--kb", type=float, default=1000.0, help="window in kilobases (column 4 of the .bim)")
    ap.add_argument("--r2", type=float, default=0.2, help="the r^2 at or above which two SNPs exclude each other")
    ap.add_argument("--pvalues", default=None, help="one p-value per SNP, .bim order (default: a seeded uniform draw)")
    ap.add_argument("--out", default=None, help="the SNPs the pruning keeps, one .bim index per line")
    a = ap.parse_args()
    mx.load_shared_library()
    plink, snps, indiv = rp.read_bed(a.bed)
    chrom, _, bp = rp.read_bim(a.bed)
    last, rowptr_all = cp.ld_window_bounds(bp, chrom, max_dist=1000.0 * a.kb)
    print(f"{snps} SNPs x {indiv} individuals; window {a.kb:g} kb: {int(rowptr_all[-1]) - snps} candidate pairs, r^2 cutoff {a.r2:g}")

    keep, rounds = cp.ld_prune(plink, snps, indiv, last=last, min_r2=a.r2, priority=-maf_of(plink, snps, indiv), pairwise=True, return_rounds=True)
    print(f"pruning by -MAF: {int(keep.sum())} SNPs kept, {rounds} rounds")
    if a.out:
        np.savetxt(a.out, np.flatnonzero(keep), fmt="%d")

    p = np.loadtxt(a.pvalues) if a.pvalues else np.random.default_rng(1).random(snps)
    keep, owner, rounds = cp.ld_prune(plink, snps, indiv, last=last, min_r2=a.r2, priority=p, pairwise=True, return_owner=True, return_rounds=True)
    size = np.bincount(owner, minlength=snps)                                        # a clump: the index SNP and everything it owns
    print(f"clumping by p-value: {int(keep.sum())} clumps, {rounds} rounds; the three largest:")
    for v in np.argsort(-size, kind="stable")[:3]:
        print(f"  index SNP {int(v)} (chr {int(chrom[v])}, bp {int(bp[v])}, p {p[v]:.3g}): {int(size[v])} SNPs")


if __name__ == "__main__":
    main()
