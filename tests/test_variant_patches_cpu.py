"""The committed timing-variant patches (variants/patches/*.json) still apply to this tree: scripts/
build_patched.py refuses a replacement whose `old` text does not occur exactly once, which nothing noticed until the
variant was needed on a GPU visit.  Patches with a `rev` build that commit's sources and those under historical/ are
kept as records: neither is held to the tree."""
import glob
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import build_patched  # noqa: E402

PATCH_DIR = os.path.join(ROOT, "variants", "patches")
PATCHES = sorted(glob.glob(os.path.join(PATCH_DIR, "*.json")))


def test_the_patches_are_found():
    assert len(PATCHES) >= 20
    assert build_patched.make_sources(), "csrc/Makefile lists no SRCS / HDRS"


@pytest.mark.parametrize("path", PATCHES, ids=[os.path.basename(p)[:-5] for p in PATCHES])
def test_patch_applies_to_this_tree(path):
    replacements, _flags, rev = build_patched.load_patch(path)
    if rev:
        return  # (that commit's sources, not the tree's)
    sources = build_patched.make_sources()
    for fname, _old, _new in replacements:
        assert os.path.normpath(fname) in sources, f"{fname}: not in csrc/Makefile's SRCS or HDRS"
    # every `old` exactly once in the named file: the rule build_patched.build enforces (ValueError otherwise)
    build_patched.apply_patch(os.path.join(ROOT, build_patched.CSRC), replacements)


def test_historical_patches_name_their_commit():
    for path in glob.glob(os.path.join(PATCH_DIR, "historical", "*.json")):
        replacements, _flags, rev = build_patched.load_patch(path)
        assert rev and replacements, f"{path}: a historical patch records the commit it last applied to"
