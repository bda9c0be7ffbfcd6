"""The strict light-block scanner (csrc/host/light_wire.h) and the host path of
tmv_light_blocks_validate_wire (csrc/host/tm_light_wire_abi.cpp, built without
the engine) under ASan + UBSan, as a stand-alone program
(tests/native/lightwire/lightwire_san.cpp, its own main) over the golden file,
every truncation and every single-byte substitution of its light blocks, each
in a heap buffer of exactly its length.  Nothing is loaded into this
interpreter.  No GPU."""
import os
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_golden_file_under_asan_ubsan():
    subprocess.run(["make", "-s", "-C", os.path.join(REPO, "tests", "native", "lightwire"), "san"], check=True)
    r = subprocess.run([os.path.join(REPO, "oracle", "_build", "lightwire_san"),
                        os.path.join(REPO, "tests", "golden", "light_wire_vectors.json")],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "\n0 wrong" in r.stdout and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
