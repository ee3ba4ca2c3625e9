#!/usr/bin/env python3
"""Emit tests/golden/reference_fortran_symbols.json from the reference's own Fortran tests and benchmark harness as oracle/Makefile.ref_fortran links them
against libmiraculix_amd.so (oracle/_ref/fortran, build container only): per program, the shared libraries it needs and the dynamic symbols it leaves
undefined -- what tests/test_abi_cpu.py checks against this library's exports where the programs are not built.  Fixtures are data only."""
import json
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
BIN = os.path.join(os.path.dirname(os.path.dirname(HERE)), "oracle", "_ref", "fortran")
PROGS = ("test_5codesapi.out", "test_5codesapi_t.out", "test_solve.out", "benchmark.out")


def main():
    out = {}
    for p in PROGS:
        path = os.path.join(BIN, p)
        assert os.path.exists(path), f"{path} not built: make -C oracle ref ref_fortran"
        dyn = subprocess.check_output(["readelf", "-d", path], text=True)
        needed = sorted(ln.split("[", 1)[1].split("]", 1)[0] for ln in dyn.splitlines() if "(NEEDED)" in ln)
        undef = sorted({ln.split()[-1].split("@")[0] for ln in subprocess.check_output(["nm", "-D", "--undefined-only", path], text=True).splitlines() if ln.strip()})
        out[p] = {"needed": needed, "undefined": undef}
    dst = os.path.join(HERE, "reference_fortran_symbols.json")
    with open(dst, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print("wrote", dst)


if __name__ == "__main__":
    main()
