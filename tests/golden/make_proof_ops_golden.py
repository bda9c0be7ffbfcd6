"""Writes tests/golden/proof_ops_vectors.json: the cases of
tests/proof_ops_cases.py with the results and texts the restatement of the
reference gives (tests/proof_ops_ref.py).  Unpinned by reference-held vectors:
the reference holds no "simple:v" proof.
Usage: python3 tests/golden/make_proof_ops_golden.py"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [REPO, os.path.join(REPO, "oracle"), os.path.join(REPO, "tests")]

import proof_ops_cases as C  # noqa: E402

if __name__ == "__main__":
    path = os.path.join(HERE, "proof_ops_vectors.json")
    with open(path, "w") as f:
        json.dump(C.golden_document(), f, indent=1)
        f.write("\n")
    print(path, os.path.getsize(path), "bytes")
