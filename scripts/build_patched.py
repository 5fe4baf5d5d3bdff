"""Timing-only variant builds of libgr.so from a patched copy of the sources (the product sources carry no
ablation switches).  A patch is a JSON list of [file, old, new] text replacements; every `old` must occur
exactly once; {"rev": COMMIT} builds that commit's sources instead of the tree's.  Output: variants/<name>/libgr.so
(GR_LIB_PATH selects it on the GPU box).

    python scripts/build_patched.py NAME PATCH.json [-DMACRO=VALUE ...]

The copy is built by its own csrc/Makefile (the only list of sources and flags), so a variant has every source the
product has and reports the SHA-256 of the patched sources (gr_source_sha256: it does not match the tree's).  Extra
arguments reach hipcc through the Makefile's EXTRA_FLAGS (cache-policy macros such as -DGR_STATE_STORE_POLICY=0);
PATCH.json may be `-` for no text replacements.
"""
import json
import os
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join("generalizableracing_amd", "csrc")


def apply_patch(csrc, patch):
    """The [file, old, new] replacements on the sources under `csrc`, in memory: {file: patched text}.  Every `old`
    occurs exactly once in its file as the earlier replacements left it (tests/test_variant_patches_cpu.py holds every
    committed patch to this rule)."""
    texts = {}
    for fname, old, new in patch:
        s = texts[fname] if fname in texts else open(os.path.join(csrc, fname)).read()
        if s.count(old) != 1:
            raise ValueError(f"{fname}: patch text found {s.count(old)} times: {old[:80]!r}")
        texts[fname] = s.replace(old, new)
    return texts


def make_sources():
    """The source and header files csrc/Makefile builds libgr.so from (its SRCS and HDRS), relative to csrc/."""
    names = []
    for line in open(os.path.join(ROOT, CSRC, "Makefile")):
        if line.startswith(("SRCS :=", "HDRS :=")):
            names += [os.path.normpath(f.replace("$(HERE)", "")) for f in line.split(":=", 1)[1].split()]
    return names


def build(name, patch, extra_flags="", rev=None):
    """Builds variants/<name>/libgr.so from a copy of the tree's sources (or of commit `rev`'s) with `patch`
    applied, by `make` in the copy."""
    tmp = tempfile.mkdtemp(prefix="grvar_")
    try:
        if rev:  # the sources of an earlier commit (a before / after pair on the same box)
            subprocess.run(f"git -C {ROOT} archive {rev} {CSRC} include | tar -x -C {tmp}", shell=True, check=True)
        else:
            shutil.copytree(os.path.join(ROOT, CSRC), os.path.join(tmp, CSRC))
            shutil.copytree(os.path.join(ROOT, "include"), os.path.join(tmp, "include"))
        src = os.path.join(tmp, CSRC)
        if extra_flags.strip() and "EXTRA_FLAGS" not in open(os.path.join(src, "Makefile")).read():
            raise SystemExit(f"{rev}: that commit's Makefile predates EXTRA_FLAGS and would drop {extra_flags.strip()!r}")
        try:
            texts = apply_patch(src, patch)
        except ValueError as e:
            raise SystemExit(str(e))
        for fname, text in texts.items():
            open(os.path.join(src, fname), "w").write(text)
        out = os.path.join(ROOT, "variants", name, "libgr.so")
        os.makedirs(os.path.dirname(out), exist_ok=True)
        subprocess.run(["make", "-C", src, "-j8", f"OUT={out}", f"OBJ={os.path.join(tmp, 'obj')}",
                        f"EXTRA_FLAGS={extra_flags.strip()}"], check=True, stdout=subprocess.DEVNULL)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    print(out)
    return out


def load_patch(path):
    """A patch file: a JSON list of [file, old, new] replacements, or {"replace": [...], "flags": "-D...",
    "rev": COMMIT, "note": "..."} (variants/patches/*.json) -> (replacements, flags, rev)."""
    if path == "-":
        return [], "", None
    p = json.load(open(path))
    if isinstance(p, dict):
        return p.get("replace", []), p.get("flags", ""), p.get("rev")
    return p, "", None


if __name__ == "__main__":
    reps, flags, rev = load_patch(sys.argv[2])
    build(sys.argv[1], reps, " ".join([flags] + sys.argv[3:]), rev)
