#!/usr/bin/env python3
"""The SNP pairs in LD of a whole PLINK fileset as a table, what `plink --r2 --ld-window-kb N --ld-window-r2 T` writes: .bed + .bim (+ .fam) -> one line
CHR_A BP_A CHR_B BP_B R2 per pair within N kb on one chromosome whose r^2 is at least T.  read_bim gives chromosome and bp per SNP, ld_window_bounds turns them
into last[] (no device needed), and ld_pairs -- on the pairwise-complete r, a real .bed has missing calls -- returns the pairs as CSR, compacted on the device:
the window's rows are never written.

usage: ld_pairs_genome.py data.bed [--kb 1000] [--r2 0.2] [--out pairs.ld]"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

import miraculix_amd as mx
from miraculix_amd import crossproduct as cp
from miraculix_amd import read_plink as rp


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("bed")
    ap.add_argument("--kb", type=float, default=1000.0, help="window in kilobases (column 4 of the .bim)")
    ap.add_argument("--r2", type=float, default=0.2, help="the smallest r^2 that is listed")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    mx.load_shared_library()
    plink, snps, indiv = rp.read_bed(a.bed)
    chrom, _, bp = rp.read_bim(a.bed)
    last, rowptr_all = cp.ld_window_bounds(bp, chrom, max_dist=1000.0 * a.kb)
    rowptr, col, val = cp.ld_pairs(plink, snps, indiv, last=last, min_r2=a.r2, kind="r2", pairwise=True)
    first = np.repeat(np.arange(snps), np.diff(rowptr))                              # SNP A of every pair; col is SNP B
    print(f"{snps} SNPs x {indiv} individuals; window {a.kb:g} kb: {int(rowptr_all[-1]) - snps} candidate pairs, {len(col)} with r^2 >= {a.r2:g}")
    out = open(a.out, "w") if a.out else sys.stdout
    out.write("CHR_A BP_A CHR_B BP_B R2\n")
    for i, j, r2 in zip(first, col, val):
        out.write(f"{int(chrom[i])} {int(bp[i])} {int(chrom[j])} {int(bp[j])} {r2:.6g}\n")
    if a.out:
        out.close()


if __name__ == "__main__":
    main()
