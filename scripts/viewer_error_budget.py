"""Write profiles/viewer_error_budget.json: per view of tests/test_gpu_viewer.py::test_gbuffer_matches_float64_restatement
the viewer kernel's depth error against the float64 restatement (tests/viewer_ref.py), the same error of the
restatement evaluated in float32, the bound max(1e-5, 4 x that) the test applies, and the id / normal figures, all
over the pixels outside the restatement's ambiguity mask.

    python scripts/viewer_error_budget.py [--out profiles/viewer_error_budget.json]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import test_gpu_viewer as tv  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "viewer_error_budget.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "viewer_error_budget.py measures on the GPU"
    views = tv.gbuffer_figures(False, check=False) + tv.gbuffer_figures(True, check=False)
    with open(a.out, "w") as f:
        json.dump({"rule": "depth_bound = max(1e-5, 4 x restatement_fp32_depth_error); depth errors are |d - float64| / "
                           "|float64| in norm over the unambiguous pixels; ids must be equal and normals within 1e-3 there",
                   "views": views, "device": torch.cuda.get_device_name(0)}, f, indent=1)


if __name__ == "__main__":
    main()
