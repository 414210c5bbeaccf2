"""The Rust side of the drop-in boundary is committed as source (triton-vm-hip/; no cargo in this image): check what can
be checked without a compiler -- the generated `extern "C"` block covers every symbol of include/triton_hip.h with the
right arity, it is up to date with the generator, and the `hip` feature patch applies to the reference tree."""
import hashlib
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def test_ffi_block_covers_the_header():
    from tools import gen_rust_ffi as gen
    from triton_vm_amd.capi import EXPORTED_SYMBOLS

    decls = gen.declarations(open(gen.HEADER).read())
    assert {name for _, name, _ in decls} == set(EXPORTED_SYMBOLS)
    ffi = open(gen.OUT).read()
    for ret, name, params in decls:
        m = re.search(r"pub fn " + name + r"\((.*?)\)( -> [^;]+)?;", ffi, re.S)
        assert m, name
        args = [a for a in m.group(1).replace("\n", " ").split(",") if a.strip()]
        assert len(args) == len(params), name
        assert (m.group(2) is None) == (ret == "void"), name


def test_ffi_block_is_up_to_date(tmp_path):
    from tools import gen_rust_ffi as gen

    committed = open(gen.OUT).read()
    out = gen.OUT
    try:
        gen.OUT = str(tmp_path / "ffi.rs")
        gen.main()
        assert open(gen.OUT).read() == committed, "run python tools/gen_rust_ffi.py"
    finally:
        gen.OUT = out


PATCH = os.path.join(ROOT, "triton-vm-hip", "patches", "triton-vm-hip.patch")
PREIMAGE = os.path.join(ROOT, "tests", "golden", "hip_patch_preimage_digests.json")


def lines_digest(lines):
    return hashlib.sha256("".join(line + "\n" for line in lines).encode()).hexdigest()


def patch_hunks(text):
    """-> {path (without the a/ prefix): [(old_start, old_count, the hunk's pre-image lines: context and removed)]}.  Fails on a hunk
    whose body does not hold the line counts its header states."""
    files, path, hunk = {}, None, None
    for line in text.splitlines():
        if line.startswith("--- "):
            path = line[4:].split("\t")[0].split("/", 1)[1]
            files[path] = []
        elif line.startswith("+++ "):
            continue
        elif line.startswith("@@ "):
            m = re.match(r"@@ -(\d+)(?:,(\d+))? \+(\d+)(?:,(\d+))? @@", line)
            old_start, old_count = int(m.group(1)), int(m.group(2) or 1)
            hunk = [old_start, old_count, [], int(m.group(4) or 1), 0]
            files[path].append(hunk)
        elif hunk is not None and line[:1] in (" ", "-"):
            hunk[2].append(line[1:])
            hunk[4] += line[:1] == " "
        elif hunk is not None and line[:1] == "+":
            hunk[4] += 1
    out = {}
    for path, hunks in files.items():
        for old_start, old_count, pre, new_count, new_seen in hunks:
            assert len(pre) == old_count and new_seen == new_count, f"{path}: hunk at line {old_start} does not match its header"
        out[path] = [(h[0], h[1], h[2]) for h in hunks]
    return out


def test_hip_feature_patch_applies_to_the_reference():
    """the reference tree is not part of this repository: tests/golden/hip_patch_preimage_digests.json holds, for every file the patch
    touches, the SHA-256 of the reference's lines at each hunk's position (tests/golden/make_hip_patch_preimage_digests.py recorded them
    from the reference tree, after `git apply --check` of the patch passed there).  Every hunk's pre-image must hash to them: the patch
    applies to that tree at its stated positions, with no offset and no fuzz."""
    with open(PREIMAGE) as f:
        want = json.load(f)
    text = open(PATCH).read()
    hunks = patch_hunks(text)
    assert sorted(hunks) == sorted(want["files"])
    for path, file_hunks in hunks.items():
        rec = want["files"][path]
        assert [[s, c] for s, c, _ in file_hunks] == [[h["old_start"], h["old_count"]] for h in rec["hunks"]], path
        for (start, count, pre), h in zip(file_hunks, rec["hunks"]):
            assert start - 1 + count <= rec["lines"], f"{path}: hunk at line {start} runs past the file's end"
            assert lines_digest(pre) == h["sha256"], f"{path}: hunk at line {start} does not match the reference's lines there"
    for seam in ("maybe_low_degree_extend_all_columns", "hash_all_ldt_domain_rows", "hip_all_quotients_combined",
                 "split_and_fold", 'hip = ["dep:triton-vm-hip"]'):
        assert seam in text
