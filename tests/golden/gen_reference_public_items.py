#!/usr/bin/env python3
"""Regenerates tests/golden/reference_public_items.json: for every source file of the reference crates the Rust hand-off imports from
(arkworks-rs/ripp: sipp, inner_products, dh_commitments, ip_proofs), the names of the items declared `pub` there.
tests/test_rust_handoff_cpu.py checks the hand-off's imports against this index.  DATA only (file -> item names), no source text.

  python tests/golden/gen_reference_public_items.py <checkout of arkworks-rs/ripp>
"""
import json
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CRATES = ("sipp", "inner_products", "dh_commitments", "ip_proofs")
PUB_ITEM = re.compile(r"^\s*pub\s+(?:fn|struct|trait|type|enum|mod|const)\s+([A-Za-z0-9_]+)\b", flags=re.M)


def index(ref):
    out = {}
    for crate in CRATES:
        src = os.path.join(ref, crate, "src")
        for dirpath, _, files in sorted(os.walk(src)):
            for f in sorted(files):
                if f.endswith(".rs"):
                    path = os.path.join(dirpath, f)
                    out[os.path.relpath(path, ref).replace(os.sep, "/")] = sorted(set(PUB_ITEM.findall(open(path).read())))
    return out


if __name__ == "__main__":
    if len(sys.argv) != 2 or not os.path.isdir(os.path.join(sys.argv[1], "sipp", "src")):
        sys.exit(__doc__)
    with open(os.path.join(HERE, "reference_public_items.json"), "w") as f:
        json.dump(index(sys.argv[1]), f, indent=1, sort_keys=True)
        f.write("\n")
