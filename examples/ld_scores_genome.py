#!/usr/bin/env python3
"""LD scores of a whole PLINK fileset in one call: .bed + .bim (+ .fam) -> one score per SNP, with a window in centimorgans (LD-score regression's default is
1 cM) or in kilobases that stops at every chromosome end.  The window is data: read_bim gives chromosome, cM and bp per SNP, ld_window_bounds turns them
into last[] (no device needed), and ld_window_scores_pairwise -- the pairwise-complete r, a real .bed has missing calls -- sums r^2 over each SNP's window.

usage: ld_scores_genome.py data.bed [--cm 1.0 | --kb 1000] [--adjust] [--out scores.txt]"""
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
    ap.add_argument("--cm", type=float, default=None, help="window in centimorgans (column 3 of the .bim)")
    ap.add_argument("--kb", type=float, default=None, help="window in kilobases (column 4 of the .bim)")
    ap.add_argument("--adjust", action="store_true", help="r^2 - (1 - r^2) / (N - 2), the estimator of LD-score regression")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.cm is not None and a.kb is not None:
        ap.error("give --cm or --kb, not both")
    if a.cm is None and a.kb is None:
        a.cm = 1.0
    mx.load_shared_library()
    plink, snps, indiv = rp.read_bed(a.bed)
    chrom, cm, bp = rp.read_bim(a.bed)
    pos, max_dist = (cm, a.cm) if a.cm is not None else (bp, 1000.0 * a.kb)
    last, rowptr = cp.ld_window_bounds(pos, chrom, max_dist=max_dist)
    reach = last - np.arange(snps)
    print(f"{snps} SNPs x {indiv} individuals on {int(chrom.max()) + 1} chromosome(s); window {max_dist:g} {'cM' if a.cm is not None else 'bp'}: "
          f"reach mean {reach.mean():.1f}, max {reach.max()}; {len(cp.ld_window_tiles(last))} tiles, {int(rowptr[-1])} pairs")
    scores = cp.ld_window_scores_pairwise(plink, snps, indiv, last, adjust=a.adjust)
    if a.out:
        np.savetxt(a.out, scores, fmt="%.17g")
    print(f"LD scores: mean {np.nanmean(scores):.4f}, min {np.nanmin(scores):.4f}, max {np.nanmax(scores):.4f}, non-finite {int((~np.isfinite(scores)).sum())}")


if __name__ == "__main__":
    main()
