"""The host layer's query-proof and tx-proof code (csrc/host/tm_proof_ops_abi.cpp,
built without the engine) under ASan + UBSan, as a stand-alone program
(tests/native/proofops/proofops_san.cpp, its own main) over the golden file.
Nothing is loaded into this interpreter.  No GPU."""
import os
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_golden_file_under_asan_ubsan():
    subprocess.run(["make", "-s", "-C", os.path.join(REPO, "tests", "native", "proofops"), "san"], check=True)
    r = subprocess.run([os.path.join(REPO, "oracle", "_build", "proofops_san"),
                        os.path.join(REPO, "tests", "golden", "proof_ops_vectors.json")],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "\n0 wrong" in r.stdout and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
