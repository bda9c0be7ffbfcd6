"""Inputs shared by the CPU and GPU tests of the cached secp256k1 path
(tests/test_secp256k1_comb.py, tests/test_gpu_secp256k1_cache.py)."""
import hashlib

import secp256k1_ref as R
from tendermint_amd.testing import secp256k1_factory as F

N = R.N


def leading_digit(u):
    """(window, digit) of the most significant non-zero 4-bit digit of u."""
    j = (u.bit_length() - 1) // 4
    return j, (u >> (4 * j)) & 15


def key1_cases():
    """Signatures by private key 1 (public key G, so the key's comb is G's):
    the first 4 seeded messages whose u1 and u2 lead with the same digit in
    the same window -- the chain's accumulator then meets its own addend and
    must double -- and the first 4 where they differ.  [(msg, sig, coincide)]"""
    same, other = [], []
    i = 0
    while len(same) < 4 and i < 4000:
        msg = b"secp256k1 comb doubling case %d" % i
        i += 1
        z = hashlib.sha256(msg).digest()
        sig = F.sign_digest(1, z)
        r, s = int.from_bytes(sig[:32], "big"), int.from_bytes(sig[32:], "big")
        w = pow(s, -1, N)
        u1, u2 = int.from_bytes(z, "big") * w % N, r * w % N
        if leading_digit(u1) == leading_digit(u2):
            same.append((msg, sig, True))
        elif len(other) < 4:
            other.append((msg, sig, False))
    return same + other


def commit_jobs():
    """8 commits of 7 secp256k1 validators (full checks), the fourth signature
    of the sixth commit corrupted."""
    import commit_fixtures as CF
    import secp256k1_cases as SC
    from tendermint_amd import host as H
    vals, signers = SC.secp_set(7)
    jobs = []
    for k in range(8):
        bid = CF.random_block_id(20 + k)
        commit = CF.make_commit(signers, SC.CHAIN, 9 + k, 0, bid)
        if k == 5:
            commit = SC.with_sig(commit, 3, SC.flip(commit.signatures[3].signature))
        jobs.append(H.CommitJob(H.MODE_FULL, SC.CHAIN, vals, bid, 9 + k, commit))
    return jobs
