#!/usr/bin/env python3
"""Records tests/golden/gridfree_refusals.json and tests/golden/gridfree_chain_bits.npz from the library as built (on the
device: both need handles), so that a change of the host code behind rootMUSIC_linear_array, esprit_linear_array and
root_pipeline can be replayed against the commit before it.  The cases are tests/gridfree_cases.py's; the tests that replay
them are test_cpu_gridfree_refusals.py, test_gpu_gridfree_refusals.py and test_gpu_gridfree_chain.py.
    gridfree_refusals.json    {case: [return code, doa_last_error() text]}
    gridfree_chain_bits.npz   in/<name>: the seeded inputs (int16 streams, complex64 covariance items);
                              <shape>/<form>: outputs as raw 32-bit words (host entries: "rc|text" as bytes)
Run from the repo root:  python tests/golden/make_gridfree_golden.py [--out DIR]
"""
import argparse
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [os.path.join(ROOT, "gr-doa_amd", "python"), os.path.join(ROOT, "tests")]
import gridfree_cases as cases                                # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=HERE)
args = ap.parse_args()
os.makedirs(args.out, exist_ok=True)

refusals = {c[0]: cases.run_refusal(c[0]) for c in cases.REFUSALS}
with open(os.path.join(args.out, "gridfree_refusals.json"), "w") as f:
    json.dump(refusals, f, indent=1, sort_keys=True)
    f.write("\n")
print(f"gridfree_refusals.json: {len(refusals)} cases")

inputs = cases.make_inputs()
bits = cases.run_all_bits(inputs)
path = os.path.join(args.out, "gridfree_chain_bits.npz")
np.savez_compressed(path, **{f"in/{k}": v for k, v in inputs.items()}, **bits)
print(f"gridfree_chain_bits.npz: {len(bits)} arrays, {os.path.getsize(path) / 1024:.0f} KiB")
