#!/usr/bin/env python3
"""Writes tests/golden/hip_patch_preimage_digests.json: for every file that triton-vm-hip/patches/triton-vm-hip.patch touches, the
length of the reference's file and the SHA-256 of its lines at each hunk's position -- what tests/test_rust_shim.py checks the patch
against, so that the test needs no copy of the reference tree.  Runs `git apply --check` of the patch on a copy of the tree first and
writes nothing if it fails.

    python tests/golden/make_hip_patch_preimage_digests.py <the reference workspace: the directory that holds triton-vm/> [out.json]
"""
import json
import os
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def main(workspace, out=None):
    from tests.test_rust_shim import PATCH, PREIMAGE, lines_digest, patch_hunks

    with tempfile.TemporaryDirectory() as tmp:
        shutil.copytree(os.path.join(workspace, "triton-vm"), os.path.join(tmp, "triton-vm"))
        subprocess.check_call(["git", "init", "-q", "."], cwd=tmp)
        subprocess.check_call(["git", "apply", "--check", "-p1", PATCH], cwd=tmp)
    files = {}
    for path, hunks in patch_hunks(open(PATCH).read()).items():
        with open(os.path.join(workspace, path)) as f:
            lines = f.read().splitlines()
        files[path] = {"lines": len(lines),
                       "hunks": [{"old_start": s, "old_count": c, "sha256": lines_digest(lines[s - 1:s - 1 + c])} for s, c, _ in hunks]}
    with open(out or PREIMAGE, "w") as f:
        json.dump({"patch": os.path.relpath(PATCH, ROOT), "files": files}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main(*sys.argv[1:])
