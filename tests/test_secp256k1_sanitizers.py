"""The host build of secp256k1.h under ASan + UBSan, as a stand-alone program
(tests/native/secp/secp_san.cpp, its own main) over the golden vectors.
Nothing is loaded into this interpreter.  No GPU."""
import os
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_golden_vectors_under_asan_ubsan():
    subprocess.run(["make", "-s", "-C", os.path.join(REPO, "tests", "native", "secp"), "san"], check=True)
    r = subprocess.run([os.path.join(REPO, "oracle", "_build", "secp_san"),
                        os.path.join(REPO, "tests", "golden", "secp256k1_vectors.json")],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "0 wrong" in r.stdout and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
