#!/usr/bin/env python3
"""A scan of related, stratified individuals: two sub-populations with drifted allele frequencies (Balding-Nichols), crossed with sib-ships of four; a trait
with a sub-population shift, a polygenic part from SNPs that are not scanned, and a few causal SNPs among the scanned ones; 1 % missing calls.  No covariate
knows about the sub-populations or the families.  assoc_linear -- the model of unrelated individuals -- is inflated over the whole genome; assoc_mixed
(y = C gamma + g + e, g ~ N(0, sg2 K), leave-one-chromosome-out, GRAMMAR-Gamma calibration, exact variances for the top SNPs) is not.  Prints the genomic
inflation factor lambda_GC = median(chi^2) / 0.4549 of both over the null SNPs and the top hits of both.  (At the small default size K rests on 1200 SNPs per
left-out chromosome and h2 on a noisy Haseman-Elston fit: over seeds the mixed lambda_GC lies between 1.0 and 1.3 where the linear one lies between 1.4 and 2.5.)

usage: gwas_mixed.py [--snps 1600] [--indiv 600] [--chrom 4] [--causal 3] [--fst 0.05] [--shift 0.4] [--seed 14]"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

import miraculix_amd as mx


def simulate(rng, snps, hidden, indiv, fst):
    """(snps + hidden, indiv) allele counts and the sub-population of every individual"""
    total = snps + hidden
    fam = np.arange(indiv) // 4
    fam_pop = np.arange(int(fam[-1]) + 1) % 2
    p0 = rng.uniform(0.1, 0.9, total)
    a = (1 - fst) / fst
    pk = np.stack([rng.beta(p0 * a, (1 - p0) * a) for _ in range(2)])
    parents = rng.random((len(fam_pop), 2, 2, total)) < pk[fam_pop][:, None, None, :]          # family, parent, haplotype, SNP
    pick = rng.integers(0, 2, (indiv, 2, total))
    Z = np.zeros((indiv, total), np.int8)
    for par in range(2):
        hap = parents[fam, par]
        Z += np.where(pick[:, par] == 0, hap[:, 0], hap[:, 1]).astype(np.int8)
    return np.ascontiguousarray(Z.T), fam_pop[fam]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--snps", type=int, default=1600)
    ap.add_argument("--indiv", type=int, default=600)
    ap.add_argument("--chrom", type=int, default=4)
    ap.add_argument("--causal", type=int, default=3)
    ap.add_argument("--fst", type=float, default=0.05)
    ap.add_argument("--shift", type=float, default=0.4)
    ap.add_argument("--seed", type=int, default=14)
    a = ap.parse_args()
    mx.load_shared_library()
    mx.dgemm_compressed.set_options(use_gpu=True, not_center=False, verbose=0)          # the kinship operator needs the centred default
    rng = np.random.default_rng(a.seed)
    snps, indiv, hidden = a.snps, a.indiv, 300
    Z, pop = simulate(rng, snps, hidden, indiv, a.fst)
    zc = Z[snps:].astype(np.float64)
    g = (zc - zc.mean(1, keepdims=True)).T @ rng.standard_normal(hidden)
    g = np.sqrt(0.3) * g / g.std()
    causal = np.sort(rng.choice(snps, a.causal, replace=False))
    xc = Z[causal].astype(np.float64)
    effect = 0.45 * rng.choice([-1.0, 1.0], a.causal)
    y = a.shift * pop + g + effect @ ((xc - xc.mean(1, keepdims=True)) / xc.std(1, keepdims=True)) + np.sqrt(0.7) * rng.standard_normal(indiv)
    code = np.where(rng.random((snps, indiv)) < 0.01, 1, np.where(Z[:snps] == 0, 0, Z[:snps] + 1)).astype(np.uint8)
    code = np.concatenate([code, np.zeros((snps, (-indiv) % 4), np.uint8)], axis=1).reshape(snps, -1, 4)
    plink = np.ascontiguousarray(code[:, :, 0] | (code[:, :, 1] << 2) | (code[:, :, 2] << 4) | (code[:, :, 3] << 6))
    per = snps // a.chrom // 4 * 4                                                       # SNPs per chromosome, a multiple of 4; the last takes the rest
    bounds = [c * per for c in range(a.chrom)] + [snps]

    lin = mx.assoc_linear(plink, snps, indiv, y)
    res = mx.assoc_mixed(plink, snps, indiv, y, chrom_bounds=bounds, loco=True, exact_cutoff=3.0)
    null = np.setdiff1d(np.arange(snps), causal)

    def lam(z):
        z = z[null]
        return float(np.median(z[np.isfinite(z)] ** 2) / 0.4549)
    zm = res.zstat[:, 0]
    print(f"{snps} SNPs on {a.chrom} chromosomes x {indiv} individuals in sib-ships of 4 from 2 sub-populations (F = {a.fst:g}), {a.causal} causal SNPs: "
          f"h2 {res.h2[0]:.3f}, calibration factors {np.array2string(res.gamma[:, 0], precision=3)}, {int(res.flag.sum())} exact variances")
    print(f"lambda_GC assoc_linear: {lam(lin.t):.3f}")
    print(f"lambda_GC assoc_mixed: {lam(zm):.3f}")
    for name, z in (("assoc_linear", lin.t), ("assoc_mixed", zm)):
        top = np.argsort(-np.abs(np.nan_to_num(z)))[:5]
        print(f"top hits {name}: " + ", ".join(f"{s}{'*' if s in causal else ''} ({z[s]:+.2f})" for s in top))
    print("(* = causal)")
    print("PASS")


if __name__ == "__main__":
    main()
