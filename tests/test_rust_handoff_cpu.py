"""The arkworks hand-off (rust/ripp-hip) cannot be compiled in this image (no Rust toolchain), so what CAN be checked
mechanically is checked here: the Rust sources name no PRIVATE item of the reference (build round 3's dumpers read `proof.gt_elems`, a
private field of sipp::Proof -- rustc E0616), and every item they import from the reference crates is declared `pub` there (checked against
tests/golden/reference_public_items.json, an index of the reference's public items made by tests/golden/gen_reference_public_items.py)."""
import json
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RUST = os.path.join(ROOT, "rust", "ripp-hip")
FILES = ["examples/dump_kat.rs", "examples/dump_kat_377.rs", "src/lib.rs", "src/convert.rs", "src/ffi.rs", "src/fused.rs", "tests/vec_roundtrip.rs"]
REF_PUBLIC = os.path.join(ROOT, "tests", "golden", "reference_public_items.json")

# fields that are private / pub(crate) in the reference: sipp::Proof (sipp/src/lib.rs:32-34), GIPAProof / GIPAAux (gipa.rs:24-77: pub(crate)),
# TIPAProof (tipa/mod.rs:41-65), TIPAWithSSMProof (structured_scalar_message.rs:138-156), AggregateProof (groth16_aggregation.rs:59-69)
PRIVATE_FIELDS = ["gt_elems", "gipa_proof", "final_ck", "final_ck_proof", "r_commitment_steps", "r_base", "r_transcript", "ck_base",
                  "tipa_proof_ab", "tipa_proof_c", "_gipa", "_pair", "_engine", "_digest"]


def strip_comments(src):
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return "\n".join(re.sub(r"//.*$", "", ln) for ln in src.splitlines())


@pytest.mark.parametrize("rel", FILES)
def test_no_private_field_of_the_reference_is_read(rel):
    code = strip_comments(open(os.path.join(RUST, rel)).read())
    hits = [(m.group(0), code[: m.start()].count("\n") + 1) for m in re.finditer(r"\.\s*(%s)\b" % "|".join(PRIVATE_FIELDS), code)]
    assert not hits, f"{rel} reads private fields of the reference (would not compile: E0616): {hits}"


def _flatten(prefix, body):
    """`a::{b, c::{d, e}}` -> [a::b, a::c::d, a::c::e]"""
    body = body.strip()
    if not body.startswith("{"):
        return [prefix + body]
    out, depth, cur = [], 0, ""
    for ch in body[1:-1]:
        if ch == "," and depth == 0:
            out.append(cur); cur = ""
        else:
            depth += ch == "{"; depth -= ch == "}"; cur += ch
    if cur.strip():
        out.append(cur)
    res = []
    for item in out:
        item = item.strip()
        m = re.match(r"([A-Za-z0-9_]+(?:::[A-Za-z0-9_]+)*)::(\{.*\})$", item, flags=re.S)
        res += _flatten(prefix + m.group(1) + "::", m.group(2)) if m else [prefix + item]
    return res


CRATE_DIR = {"ark_sipp": "sipp", "ark_inner_products": "inner_products", "ark_dh_commitments": "dh_commitments", "ark_ip_proofs": "ip_proofs"}


@pytest.mark.parametrize("rel", FILES)
def test_every_item_imported_from_the_reference_is_public_there(rel):
    code = strip_comments(open(os.path.join(RUST, rel)).read())
    paths = []
    for m in re.finditer(r"\buse\s+(ark_(?:sipp|inner_products|dh_commitments|ip_proofs))::(.*?);", code, flags=re.S):
        body = re.sub(r"\s+", "", m.group(2))
        paths += _flatten(m.group(1) + "::", body if body.startswith("{") else "{" + body + "}")
    # fully qualified uses in expressions (ark_inner_products::PairingInnerProduct::<..>)
    for m in re.finditer(r"\b(ark_(?:sipp|inner_products|dh_commitments|ip_proofs))::([A-Za-z_][A-Za-z0-9_]*)\b", code):
        paths.append(m.group(1) + "::" + m.group(2))
    assert paths or rel.endswith(("ffi.rs", "convert.rs", "vec_roundtrip.rs"))
    with open(REF_PUBLIC) as f:
        public = json.load(f)
    for path in sorted(set(paths)):
        parts = path.split("::")
        src_dir = CRATE_DIR[parts[0]] + "/src"
        name, mods = parts[-1], parts[1:-1]
        # the file the item lives in: src/<mods...>.rs or src/<mods...>/mod.rs, src/lib.rs for crate-root items
        cands = ["/".join([src_dir, *mods]) + ".rs", "/".join([src_dir, *mods, "mod.rs"])] if mods else [src_dir + "/lib.rs"]
        files = [c for c in cands if c in public]
        assert files, f"{rel}: module of `{path}` not found in the reference"
        assert name in public[files[0]], f"{rel}: `{path}` is not a public item of the reference ({files[0]})"


def test_design_does_not_call_the_handoff_compiled():
    """DESIGN.md section 5 must say the hand-off has never been through a compiler (there is none here)."""
    text = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "never been through a compiler" in text or "has not been compiled" in text


def test_vector_downloads_are_typed_by_kind():
    """ripp_vec_download writes AFFINE group elements (vec_api.inc: vec_elem_size = sizeof(G1A) / sizeof(G2A) / sizeof(Fr)).  The Rust wrapper must size its
    buffer with the affine FFI structs and refuse a handle of another kind before the call: a projective buffer decodes garbage, a scalar buffer handed
    over for a G1 vector is overrun by 64 n bytes.  (Source-level: there is no Rust toolchain here; rust/ripp-hip/tests/vec_roundtrip.rs is the run-time test.)"""
    code = strip_comments(open(os.path.join(RUST, "src", "fused.rs")).read())
    for fn, buf, kind in (("download_g1a", "RippG1A", "RIPP_VEC_G1"), ("download_g2a", "RippG2A", "RIPP_VEC_G2"), ("download_fr", "RippFr", "RIPP_VEC_FR")):
        m = re.search(r"pub fn %s\(&self\)[^{]*\{(.*?)\n" % fn, code, flags=re.S)
        assert m, fn
        body = m.group(1)
        assert "want_kind(%s" % kind in body and body.index("want_kind") < body.index("ripp_vec_download"), fn
        assert "vec![%s::default(); self.len()]" % buf in body, fn
    # no download may allocate projective elements for ripp_vec_download
    assert not re.search(r"vec!\[RippG[12]J::default\(\); self\.len\(\)\][^;]*;[^;]*ripp_vec_download", code)
    hdr = open(os.path.join(ROOT, "include", "ripp_hip.h")).read()
    ffi = open(os.path.join(RUST, "src", "ffi.rs")).read()
    for name, val in re.findall(r"(RIPP_VEC_[A-Z0-9]+) = (\d+)", hdr):
        assert re.search(r"pub const %s: i32 = %s;" % (name, val), ffi), name
