#!/usr/bin/env python3
"""Generates tests/golden/reference_prototypes.json: the parameter count of every `void name(...);` prototype in the reference's
C++ headers ({raymarching,gridencoder,shencoder,freqencoder}/src/<name>.h).  Only the counts are stored, no source text.  Runs only
where the reference checkout is (N2M_REFERENCE); tests/test_abi.py reads the committed file.

    python tests/golden/make_golden_abi.py
"""
import json
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from oracle.ref_python import REFERENCE   # noqa: E402  (the checkout's location, N2M_REFERENCE)
HEADERS = (("raymarching", "raymarching.h"), ("gridencoder", "gridencoder.h"), ("shencoder", "shencoder.h"), ("freqencoder", "freqencoder.h"))


def main():
    assert os.path.isdir(REFERENCE), "needs the reference checkout"
    out = {}
    for pkg, hdr in HEADERS:
        src = open(os.path.join(REFERENCE, pkg, "src", hdr)).read()
        out[f"{pkg}/src/{hdr}"] = {m.group(1): len(m.group(2).split(","))
                                   for m in re.finditer(r"void\s+(\w+)\s*\((.*?)\)\s*;", src, flags=re.S)}
    path = os.path.join(HERE, "reference_prototypes.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{path}: {sum(len(v) for v in out.values())} prototypes")


if __name__ == "__main__":
    main()
