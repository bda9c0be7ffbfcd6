"""Python view of the C++ host layer (include/tmhost.h): the types the
reference's commit verification works on, and thin ctypes calls into
libtmgpu.so's tmv_verify_commit / tmv_vote_sign_bytes / tmv_batch_*.

Mirrors (names and argument meaning):
  crypto.BatchVerifier / batch.CreateBatchVerifier  -> BatchVerifier / create_batch_verifier
  types.VerifyCommit / VerifyCommitLight / VerifyCommitLightTrusting
                                                   -> verify_commit / verify_commit_light /
                                                      verify_commit_light_trusting
Errors are returned as strings (None = ok), byte-identical to the Go error
text; infrastructure failures raise NativeError.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass, field
from typing import List, Optional, Tuple

from . import _native
from ._native import NativeError, TMV_KIND_ED25519, TMV_KIND_SR25519, TMV_KIND_SECP256K1

KIND_OTHER = 255
BLOCK_ID_FLAG_ABSENT, BLOCK_ID_FLAG_COMMIT, BLOCK_ID_FLAG_NIL = 1, 2, 3
MODE_FULL, MODE_LIGHT, MODE_LIGHT_TRUSTING = 0, 1, 2
ZERO_TIME = (-62135596800, 0)

_u8p = ctypes.POINTER(ctypes.c_uint8)


class CBlockID(ctypes.Structure):
    _fields_ = [("hash", _u8p), ("hash_len", ctypes.c_uint32), ("psh_total", ctypes.c_uint32),
                ("psh_hash", _u8p), ("psh_hash_len", ctypes.c_uint32)]


class CValidator(ctypes.Structure):
    _fields_ = [("address", _u8p), ("address_len", ctypes.c_uint32), ("pub_key", _u8p),
                ("pub_key_len", ctypes.c_uint32), ("key_kind", ctypes.c_uint8), ("voting_power", ctypes.c_int64),
                ("proposer_priority", ctypes.c_int64)]


class CCommitSig(ctypes.Structure):
    _fields_ = [("block_id_flag", ctypes.c_uint8), ("validator_address", _u8p),
                ("validator_address_len", ctypes.c_uint32), ("ts_seconds", ctypes.c_int64),
                ("ts_nanos", ctypes.c_int32), ("signature", _u8p), ("signature_len", ctypes.c_uint32)]


class CCommit(ctypes.Structure):
    _fields_ = [("height", ctypes.c_int64), ("round", ctypes.c_int32), ("block_id", CBlockID),
                ("sigs", ctypes.POINTER(CCommitSig)), ("n_sigs", ctypes.c_uint32)]


@dataclass
class BlockID:
    hash: bytes = b""
    psh_total: int = 0
    psh_hash: bytes = b""

    def equals(self, o: "BlockID") -> bool:
        return (self.hash, self.psh_total, self.psh_hash) == (o.hash, o.psh_total, o.psh_hash)


@dataclass
class Validator:
    address: bytes
    pub_key: bytes
    voting_power: int
    key_kind: int = TMV_KIND_ED25519
    proposer_priority: int = 0


@dataclass
class ValidatorSet:
    validators: List[Validator]
    proposer_index: int = -1

    def total_voting_power(self) -> int:
        return sum(v.voting_power for v in self.validators)


@dataclass
class CommitSig:
    block_id_flag: int = BLOCK_ID_FLAG_ABSENT
    validator_address: bytes = b""
    timestamp: Tuple[int, int] = ZERO_TIME
    signature: bytes = b""


@dataclass
class Commit:
    height: int
    round: int
    block_id: BlockID
    signatures: List[CommitSig] = field(default_factory=list)


class _Keep:
    """Holds the ctypes buffers alive for the duration of a call."""

    def __init__(self):
        self.refs = []

    def buf(self, b: bytes):
        if not b:
            return None, 0
        a = (ctypes.c_uint8 * len(b)).from_buffer_copy(b)
        self.refs.append(a)
        return ctypes.cast(a, _u8p), len(b)


def _c_block_id(k: _Keep, b: BlockID) -> CBlockID:
    h, hl = k.buf(b.hash)
    p, pl = k.buf(b.psh_hash)
    return CBlockID(h, hl, b.psh_total, p, pl)


def _np_dtype(struct) -> "np.dtype":
    """numpy view of a ctypes Structure (pointers as uint64), same offsets."""
    import numpy as np
    conv = {ctypes.c_uint8: np.uint8, ctypes.c_uint32: np.uint32, ctypes.c_int32: np.int32,
            ctypes.c_int64: np.int64, ctypes.c_int: np.int32}
    names, formats, offsets = [], [], []
    for name, ty in struct._fields_:
        names.append(name)
        formats.append(conv.get(ty, np.uint64))
        offsets.append(getattr(struct, name).offset)
    return np.dtype({"names": names, "formats": formats, "offsets": offsets, "itemsize": ctypes.sizeof(struct)})


_DT = {}


def _dt(key, struct):
    d = _DT.get(key)
    if d is None:
        d = _DT[key] = _np_dtype(struct)
    return d


def _blob_ptrs(k: _Keep, items: List[bytes]):
    """Concatenate byte strings into one kept buffer; per-item (pointer, len),
    pointer NULL for an empty item (as _Keep.buf)."""
    import numpy as np
    blob = b"".join(items)
    lens = np.fromiter((len(x) for x in items), dtype=np.uint32, count=len(items))
    if not blob:
        return np.zeros(len(items), np.uint64), lens
    buf = np.frombuffer(blob, dtype=np.uint8)
    k.refs.append(blob)
    offs = np.zeros(len(items), np.uint64)
    np.cumsum(lens[:-1], out=offs[1:])
    ptrs = np.where(lens > 0, offs + np.uint64(buf.ctypes.data), np.uint64(0))
    return ptrs, lens


def _c_validators(k: _Keep, vals: ValidatorSet):
    """tmv_validator[] for a validator set, built column-wise."""
    import numpy as np
    dt = _dt("v", CValidator)
    vs = vals.validators
    a = np.zeros(max(1, len(vs)), dtype=dt)
    if vs:
        a["address"][:len(vs)], a["address_len"][:len(vs)] = _blob_ptrs(k, [v.address for v in vs])
        a["pub_key"][:len(vs)], a["pub_key_len"][:len(vs)] = _blob_ptrs(k, [v.pub_key for v in vs])
        a["key_kind"][:len(vs)] = [v.key_kind for v in vs]
        a["voting_power"][:len(vs)] = [v.voting_power for v in vs]
        a["proposer_priority"][:len(vs)] = [v.proposer_priority for v in vs]
    k.refs.append(a)
    return ctypes.cast(a.ctypes.data, ctypes.POINTER(CValidator))


def _c_commit(k: _Keep, commit: Commit) -> CCommit:
    """tmv_commit for a Commit; its tmv_commit_sig[] built column-wise."""
    import numpy as np
    dt = _dt("s", CCommitSig)
    ss = commit.signatures
    n = len(ss)
    a = np.zeros(max(1, n), dtype=dt)
    if n:
        a["block_id_flag"][:n] = [s.block_id_flag for s in ss]
        a["validator_address"][:n], a["validator_address_len"][:n] = _blob_ptrs(k, [s.validator_address for s in ss])
        a["ts_seconds"][:n] = [s.timestamp[0] for s in ss]
        a["ts_nanos"][:n] = [s.timestamp[1] for s in ss]
        a["signature"][:n], a["signature_len"][:n] = _blob_ptrs(k, [s.signature for s in ss])
    k.refs.append(a)
    c = CCommit(commit.height, commit.round, _c_block_id(k, commit.block_id),
                ctypes.cast(a.ctypes.data, ctypes.POINTER(CCommitSig)), n)
    k.refs.append(c)
    return c


def _setup(L):
    if getattr(L, "_tmhost_ready", False):
        return L
    L.tmv_vote_sign_bytes.restype = ctypes.c_size_t
    L.tmv_vote_sign_bytes.argtypes = [ctypes.c_char_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_int32,
                                      ctypes.POINTER(CBlockID), ctypes.c_int64, ctypes.c_int32, _u8p, ctypes.c_size_t]
    L.tmv_vote_template_encode.restype = ctypes.c_size_t
    L.tmv_vote_template_encode.argtypes = [ctypes.c_char_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_int32,
                                           ctypes.POINTER(CBlockID), _u8p, ctypes.c_size_t,
                                           ctypes.POINTER(ctypes.c_uint32)]
    L.tmv_verify_commit.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_char_p, ctypes.POINTER(CValidator),
                                    ctypes.c_uint32, ctypes.c_int32, ctypes.POINTER(CBlockID), ctypes.c_int64,
                                    ctypes.POINTER(CCommit), ctypes.c_int64, ctypes.c_int64, ctypes.c_char_p,
                                    ctypes.c_size_t]
    L.tmv_batch_new.restype = ctypes.c_void_p
    L.tmv_batch_new.argtypes = [ctypes.c_void_p, ctypes.c_uint8]
    L.tmv_batch_add.argtypes = [ctypes.c_void_p, ctypes.c_uint8, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_char_p,
                                ctypes.c_size_t, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_size_t]
    L.tmv_batch_len.restype = ctypes.c_size_t
    L.tmv_batch_len.argtypes = [ctypes.c_void_p]
    L.tmv_batch_verify.argtypes = [ctypes.c_void_p, _u8p, ctypes.POINTER(ctypes.c_int64), ctypes.c_char_p,
                                   ctypes.c_size_t]
    L.tmv_batch_free.argtypes = [ctypes.c_void_p]
    L._tmhost_ready = True
    return L


def vote_sign_bytes(chain_id: str, vote_type: int, height: int, round_: int, block_id: Optional[BlockID],
                    timestamp: Tuple[int, int], lib=None) -> bytes:
    """types.VoteSignBytes through the C++ encoder (tmv_vote_sign_bytes)."""
    L = _setup(lib or _native.lib())
    k = _Keep()
    bid = ctypes.byref(_c_block_id(k, block_id)) if block_id is not None else None
    out = (ctypes.c_uint8 * 512)()
    n = L.tmv_vote_sign_bytes(chain_id.encode(), vote_type, height, round_, bid, timestamp[0], timestamp[1],
                              ctypes.cast(out, _u8p), 512)
    return bytes(out[:n])


def vote_template(chain_id: str, vote_type: int, height: int, round_: int, block_id: Optional[BlockID],
                  lib=None) -> Tuple[bytes, bytes, bytes]:
    """The (head, block, chain) segments of tmv_verify_votes' template through
    the C++ encoder (tmv_vote_template_encode)."""
    L = _setup(lib or _native.lib())
    k = _Keep()
    bid = ctypes.byref(_c_block_id(k, block_id)) if block_id is not None else None
    out = (ctypes.c_uint8 * 1024)()
    lens = (ctypes.c_uint32 * 3)()
    n = L.tmv_vote_template_encode(chain_id.encode(), vote_type, height, round_, bid, ctypes.cast(out, _u8p), 1024,
                                   lens)
    b = bytes(out[:n])
    h, k2 = lens[0], lens[0] + lens[1]
    return b[:h], b[h:k2], b[k2:]


def _commit_call(fn, ctx_handle, mode, chain_id, vals: Optional[ValidatorSet], block_id: Optional[BlockID],
                 height: int, commit: Optional[Commit], trust: Tuple[int, int]) -> Optional[str]:
    k = _Keep()
    cvals, nv, prop = None, 0, -1
    if vals is not None:
        cvals, nv, prop = _c_validators(k, vals), len(vals.validators), vals.proposer_index
    ccommit = ctypes.byref(_c_commit(k, commit)) if commit is not None else None
    bid = ctypes.byref(_c_block_id(k, block_id)) if block_id is not None else None
    err = ctypes.create_string_buffer(4096)
    rc = fn(ctx_handle, mode, chain_id.encode(), cvals, nv, prop, bid, height, ccommit, trust[0], trust[1], err,
            len(err))
    if rc < 0:
        raise NativeError(f"commit verification failed ({rc}): {err.value.decode(errors='replace')}")
    return err.value.decode() if rc == 1 else None


def verify_commit(ctx, chain_id: str, vals, block_id, height, commit) -> Optional[str]:
    L = _setup(_native.lib())
    return _commit_call(L.tmv_verify_commit, ctx.handle, MODE_FULL, chain_id, vals, block_id, height, commit, (0, 1))


def verify_commit_light(ctx, chain_id: str, vals, block_id, height, commit) -> Optional[str]:
    L = _setup(_native.lib())
    return _commit_call(L.tmv_verify_commit, ctx.handle, MODE_LIGHT, chain_id, vals, block_id, height, commit, (0, 1))


def verify_commit_light_trusting(ctx, chain_id: str, vals, commit, trust_level=(1, 3)) -> Optional[str]:
    L = _setup(_native.lib())
    return _commit_call(L.tmv_verify_commit, ctx.handle, MODE_LIGHT_TRUSTING, chain_id, vals, None, 0, commit,
                        trust_level)


class BatchVerifier:
    """crypto.BatchVerifier over tmv_batch_* (crypto/crypto.go:66-76).
    `lib` / a raw context handle select another library exporting the same
    C-ABI (the CPU test harness)."""

    def __init__(self, ctx, key_kind: int, lib=None):
        self._L = _setup(lib or _native.lib())
        self._h = self._L.tmv_batch_new(getattr(ctx, "handle", ctx), key_kind)
        if not self._h:
            raise NativeError("no batch verifier for this key type")
        self.deferred_add_error: Optional[Tuple[int, str]] = None

    def add(self, key_kind: int, pub_key: bytes, msg: bytes, sig: bytes) -> Optional[str]:
        err = ctypes.create_string_buffer(512)
        rc = self._L.tmv_batch_add(self._h, key_kind, pub_key, len(pub_key), msg, len(msg), sig, len(sig), err, 512)
        if rc < 0:
            raise NativeError("tmv_batch_add failed")
        return err.value.decode() if rc == 1 else None

    def __len__(self):
        return self._L.tmv_batch_len(self._h)

    def verify(self) -> Tuple[bool, List[bool]]:
        n = len(self)
        out = (ctypes.c_uint8 * max(1, n))()
        idx = ctypes.c_int64(-1)
        err = ctypes.create_string_buffer(512)
        rc = self._L.tmv_batch_verify(self._h, ctypes.cast(out, _u8p), ctypes.byref(idx), err, 512)
        if rc < 0:
            raise NativeError(f"tmv_batch_verify failed ({rc}): {err.value.decode(errors='replace')}")
        self.deferred_add_error = (idx.value, err.value.decode()) if rc == 2 else None
        return rc == 1, [bool(out[i]) for i in range(n)]

    def __del__(self):
        try:
            if self._h:
                self._L.tmv_batch_free(self._h)
        except Exception:
            pass


def create_batch_verifier(ctx, key_kind: int, lib=None) -> Optional[BatchVerifier]:
    """batch.CreateBatchVerifier (crypto/batch/batch.go:11-21): None for key
    types without batch support (the C-ABI returns NULL for them)."""
    try:
        return BatchVerifier(ctx, key_kind, lib)
    except NativeError:
        return None


def supports_batch_verifier(key_kind: int) -> bool:
    return key_kind in (TMV_KIND_ED25519, TMV_KIND_SR25519)


class PreparedCommitCall:
    """A tmv_verify_commit call with its C structs built once (for timing the
    L3 path without Python marshalling in the loop)."""

    def __init__(self, ctx, mode, chain_id, vals, block_id, height, commit, trust=(0, 1)):
        L = _setup(_native.lib())
        self._L, self._ctx = L, ctx
        k = _Keep()
        arr = _c_validators(k, vals)
        cc = _c_commit(k, commit)
        bid = _c_block_id(k, block_id) if block_id is not None else None
        self._keep = (k, arr, cc, bid)
        self._args = (mode, chain_id.encode(), arr, len(vals.validators), vals.proposer_index,
                      ctypes.byref(bid) if bid is not None else None, height, ctypes.byref(cc), trust[0], trust[1])
        self._err = ctypes.create_string_buffer(4096)

    def __call__(self) -> Optional[str]:
        rc = self._L.tmv_verify_commit(self._ctx.handle, *self._args, self._err, len(self._err))
        if rc < 0:
            raise NativeError(f"tmv_verify_commit failed ({rc}): {self._err.value.decode(errors='replace')}")
        return self._err.value.decode() if rc == 1 else None


class CCommitJob(ctypes.Structure):
    _fields_ = [("mode", ctypes.c_int), ("chain_id", ctypes.c_char_p), ("vals", ctypes.POINTER(CValidator)),
                ("n_vals", ctypes.c_uint32), ("proposer_index", ctypes.c_int32),
                ("block_id", ctypes.POINTER(CBlockID)), ("height", ctypes.c_int64),
                ("commit", ctypes.POINTER(CCommit)), ("trust_num", ctypes.c_int64), ("trust_den", ctypes.c_int64)]


@dataclass
class CommitJob:
    """One commit check: mode MODE_FULL / MODE_LIGHT / MODE_LIGHT_TRUSTING."""
    mode: int
    chain_id: str
    vals: Optional[ValidatorSet]
    block_id: Optional[BlockID]
    height: int
    commit: Optional[Commit]
    trust: Tuple[int, int] = (1, 3)


class PreparedJobs:
    """C structs for a list of CommitJob, built once.  Jobs that share a
    Commit object (by identity) share one tmv_commit, so the engine verifies
    their common signatures once (blocksync checks each commit twice)."""

    def __init__(self, jobs: List[CommitJob]):
        k = _Keep()
        vcache, ccache = {}, {}
        arr = (CCommitJob * max(1, len(jobs)))()
        for j, jb in enumerate(jobs):
            cv, nv, prop = None, 0, -1
            if jb.vals is not None:
                # sets that share one list of validators (a replay's sets between two validator
                # changes: only the proposer moves) share one tmv_validator array
                key = id(jb.vals.validators) if type(jb.vals) is ValidatorSet else id(jb.vals)
                if key not in vcache:
                    vcache[key] = _c_validators(k, jb.vals)
                cv, nv, prop = vcache[key], len(jb.vals.validators), jb.vals.proposer_index
            cc = None
            if isinstance(jb.commit, ViewCommit):  # already a tmv_commit, inside a tmv_block_views object
                cc = jb.commit.ptr
                k.refs.append(jb.commit.owner)
            elif jb.commit is not None:
                key = id(jb.commit)
                if key not in ccache:
                    ccache[key] = _c_commit(k, jb.commit)
                cc = ctypes.pointer(ccache[key])
            bid = None
            if jb.block_id is not None:
                b = _c_block_id(k, jb.block_id)
                k.refs.append(b)
                bid = ctypes.pointer(b)
            cid = jb.chain_id.encode()
            k.refs.append(cid)
            arr[j] = CCommitJob(jb.mode, cid, cv, nv, prop, bid, jb.height, cc, jb.trust[0], jb.trust[1])
        self.keep = (k, vcache, ccache)
        self.arr = arr
        self.n = len(jobs)
        self.stride = 512
        self.errs = ctypes.create_string_buffer(self.stride * max(1, self.n))
        self.results = (ctypes.c_int32 * max(1, self.n))()

    def decode(self) -> List[Optional[str]]:
        out = []
        buf = None  # one copy of the error buffer (ctypes' .raw copies all of it on every access)
        for j in range(self.n):
            if self.results[j]:
                if buf is None:
                    buf = self.errs.raw
                out.append(buf[j * self.stride:(j + 1) * self.stride].split(b"\0", 1)[0].decode())
            else:
                out.append(None)
        return out


def _setup_many(L):
    if not getattr(L, "_tmhost_many", False):
        L.tmv_verify_commits.argtypes = [ctypes.c_void_p, ctypes.POINTER(CCommitJob), ctypes.c_uint32,
                                         ctypes.POINTER(ctypes.c_int32), ctypes.c_char_p, ctypes.c_size_t]
        L._tmhost_many = True
    return L


def run_prepared_jobs(ctx, pj: PreparedJobs) -> int:
    L = _setup_many(_setup(_native.lib()))
    rc = L.tmv_verify_commits(ctx.handle, pj.arr, pj.n, pj.results, pj.errs, pj.stride)
    if rc < 0:
        raise NativeError(f"tmv_verify_commits failed ({rc}): {_native.last_error()}")
    return rc


def verify_commits(ctx, jobs: List[CommitJob]) -> List[Optional[str]]:
    """Cross-commit batching: every job's result equals verify_commit* of that
    job alone; all signatures go to the GPU in one batch."""
    pj = PreparedJobs(jobs)
    run_prepared_jobs(ctx, pj)
    return pj.decode()


# ---------------------------------------------------------------- light client
# light.Verify / VerifyAdjacent / VerifyNonAdjacent (light/verifier.go:33-177)
# and Header.Hash (types/block.go:447-478) through tmv_light_verify_many /
# tmv_header_hashes (include/tmhost.h).

LIGHT_VERIFY, LIGHT_ADJACENT, LIGHT_NON_ADJACENT = 0, 1, 2
LIGHT_OK, LIGHT_ERR_INVALID_HEADER, LIGHT_ERR_OLD_HEADER_EXPIRED, LIGHT_ERR_CANT_TRUST, LIGHT_ERR_OTHER = 0, 1, 2, 3, 4
BLOCK_PROTOCOL = 11  # version/version.go:27


class CBytes(ctypes.Structure):
    _fields_ = [("p", _u8p), ("len", ctypes.c_uint32)]


_HASH_FIELDS = ("last_commit_hash", "data_hash", "validators_hash", "next_validators_hash", "consensus_hash",
                "app_hash", "last_results_hash", "evidence_hash", "proposer_address")


class CHeader(ctypes.Structure):
    _fields_ = ([("version_block", ctypes.c_uint64), ("version_app", ctypes.c_uint64), ("chain_id", ctypes.c_char_p),
                 ("height", ctypes.c_int64), ("time_seconds", ctypes.c_int64), ("time_nanos", ctypes.c_int32),
                 ("last_block_id", CBlockID)] + [(f, CBytes) for f in _HASH_FIELDS])


class CSignedHeader(ctypes.Structure):
    _fields_ = [("header", ctypes.POINTER(CHeader)), ("commit", ctypes.POINTER(CCommit))]


class CValidatorSet(ctypes.Structure):
    _fields_ = [("vals", ctypes.POINTER(CValidator)), ("n_vals", ctypes.c_uint32), ("proposer_index", ctypes.c_int32)]


class CLightJob(ctypes.Structure):
    _fields_ = [("mode", ctypes.c_int), ("trusted", ctypes.POINTER(CSignedHeader)),
                ("trusted_vals", ctypes.POINTER(CValidatorSet)), ("untrusted", ctypes.POINTER(CSignedHeader)),
                ("untrusted_vals", ctypes.POINTER(CValidatorSet)), ("trusting_period_ns", ctypes.c_int64),
                ("now_seconds", ctypes.c_int64), ("now_nanos", ctypes.c_int32),
                ("max_clock_drift_ns", ctypes.c_int64), ("trust_num", ctypes.c_uint64),
                ("trust_den", ctypes.c_uint64)]


@dataclass
class Header:
    """types.Header (types/block.go:338-366)."""
    chain_id: str
    height: int
    time: Tuple[int, int]
    last_block_id: BlockID = field(default_factory=BlockID)
    last_commit_hash: bytes = b""
    data_hash: bytes = b""
    validators_hash: bytes = b""
    next_validators_hash: bytes = b""
    consensus_hash: bytes = b""
    app_hash: bytes = b""
    last_results_hash: bytes = b""
    evidence_hash: bytes = b""
    proposer_address: bytes = b""
    version_block: int = BLOCK_PROTOCOL
    version_app: int = 0


@dataclass
class SignedHeader:
    """types.SignedHeader (types/light.go:131-136)."""
    header: Optional[Header]
    commit: Optional[Commit]

    @property
    def height(self) -> int:
        return self.header.height


@dataclass
class LightBlock:
    """types.LightBlock: a signed header and the validator set at its height."""
    signed_header: SignedHeader
    vals: ValidatorSet
    next_vals: Optional[ValidatorSet] = None

    @property
    def height(self) -> int:
        return self.signed_header.header.height


@dataclass
class LightJob:
    """One light-client verification (the arguments of light.Verify)."""
    trusted: SignedHeader
    trusted_next_vals: Optional[ValidatorSet]
    untrusted: SignedHeader
    untrusted_vals: Optional[ValidatorSet]
    trusting_period_ns: int
    now: Tuple[int, int]
    max_clock_drift_ns: int = 10 * 10**9  # light/client.go:52 defaultMaxClockDrift
    trust: Tuple[int, int] = (1, 3)       # light.DefaultTrustLevel
    mode: int = LIGHT_VERIFY


def _c_bytes(k: _Keep, b: bytes) -> CBytes:
    p, n = k.buf(b)
    return CBytes(p, n)


def _c_header(k: _Keep, h: Header) -> CHeader:
    cid = h.chain_id.encode()
    k.refs.append(cid)
    c = CHeader(h.version_block, h.version_app, cid, h.height, h.time[0], h.time[1], _c_block_id(k, h.last_block_id),
                *[_c_bytes(k, getattr(h, f)) for f in _HASH_FIELDS])
    k.refs.append(c)
    return c


class PreparedLightJobs:
    """C structs for a list of LightJob, built once; headers, commits and
    validator sets shared by object identity are passed once (the engine
    converts and hashes each distinct one once)."""

    def __init__(self, jobs: List[LightJob]):
        k = _Keep()
        hcache, ccache, vcache, shcache = {}, {}, {}, {}

        def header(h):
            if h is None:
                return None
            if id(h) not in hcache:
                hcache[id(h)] = (h, ctypes.pointer(_c_header(k, h)))
            return hcache[id(h)][1]

        def commit(c):
            if c is None:
                return None
            if id(c) not in ccache:
                cc = _c_commit(k, c)
                ccache[id(c)] = (c, ctypes.pointer(cc))
            return ccache[id(c)][1]

        def signed(sh):
            if sh is None:
                return None
            if isinstance(sh, ViewSignedHeader):  # already a tmv_signed_header, inside a views object
                k.refs.append(sh)
                return sh.ptr
            if id(sh) not in shcache:
                s = CSignedHeader(header(sh.header), commit(sh.commit))
                k.refs.append(s)
                shcache[id(sh)] = (sh, ctypes.pointer(s))
            return shcache[id(sh)][1]

        def vset(vs):
            if vs is None:
                return None
            if isinstance(vs, ViewValidatorSet):
                k.refs.append(vs)
                return vs.ptr
            if id(vs) not in vcache:
                s = CValidatorSet(_c_validators(k, vs), len(vs.validators), vs.proposer_index)
                k.refs.append(s)
                vcache[id(vs)] = (vs, ctypes.pointer(s))
            return vcache[id(vs)][1]

        arr = (CLightJob * max(1, len(jobs)))()
        for j, jb in enumerate(jobs):
            arr[j] = CLightJob(jb.mode, signed(jb.trusted), vset(jb.trusted_next_vals), signed(jb.untrusted),
                               vset(jb.untrusted_vals), jb.trusting_period_ns, jb.now[0], jb.now[1],
                               jb.max_clock_drift_ns, jb.trust[0], jb.trust[1])
        self.keep = (k, hcache, ccache, vcache, shcache)
        self.arr, self.n = arr, len(jobs)
        self.stride = 1024
        self.errs = ctypes.create_string_buffer(self.stride * max(1, self.n))
        self.results = (ctypes.c_int32 * max(1, self.n))()

    def decode(self) -> List[Tuple[int, Optional[str]]]:
        out = []
        buf = None  # one copy of the error buffer (ctypes' .raw copies all of it on every access)
        for j in range(self.n):
            kind = self.results[j]
            if kind == LIGHT_OK:
                out.append((kind, None))
                continue
            if buf is None:
                buf = self.errs.raw
            out.append((kind, buf[j * self.stride:(j + 1) * self.stride].split(b"\0", 1)[0].decode()))
        return out


def _setup_light(L):
    if not getattr(L, "_tmhost_light", False):
        L.tmv_light_verify_many.argtypes = [ctypes.c_void_p, ctypes.POINTER(CLightJob), ctypes.c_uint32,
                                            ctypes.POINTER(ctypes.c_int32), ctypes.c_char_p, ctypes.c_size_t]
        L.tmv_header_hashes.argtypes = [ctypes.c_void_p, ctypes.POINTER(CHeader), ctypes.c_uint32, _u8p, _u8p]
        L._tmhost_light = True
    return L


def run_light_jobs(fn, ctx_handle, pj: PreparedLightJobs) -> List[Tuple[int, Optional[str]]]:
    """fn = tmv_light_verify_many (or the CPU harness's twin)."""
    rc = fn(ctx_handle, pj.arr, pj.n, pj.results, pj.errs, pj.stride)
    if rc < 0:
        raise NativeError(f"tmv_light_verify_many failed ({rc}): {_native.last_error()}")
    return pj.decode()


def light_verify_many(ctx, jobs: List[LightJob]) -> List[Tuple[int, Optional[str]]]:
    """Each job's (TMV_LIGHT_* class, error text or None), all jobs in one pass."""
    L = _setup_light(_setup(_native.lib()))
    return run_light_jobs(L.tmv_light_verify_many, ctx.handle, PreparedLightJobs(jobs))


def light_verify(ctx, job: LightJob) -> Tuple[int, Optional[str]]:
    return light_verify_many(ctx, [job])[0]


def header_hashes_call(fn, ctx_handle, headers: List[Header]) -> List[Optional[bytes]]:
    k = _Keep()
    arr = (CHeader * max(1, len(headers)))()
    for i, h in enumerate(headers):
        arr[i] = _c_header(k, h)
    out = (ctypes.c_uint8 * (32 * max(1, len(headers))))()
    has = (ctypes.c_uint8 * max(1, len(headers)))()
    rc = fn(ctx_handle, arr, len(headers), ctypes.cast(out, _u8p), ctypes.cast(has, _u8p))
    if rc < 0:
        raise NativeError(f"tmv_header_hashes failed ({rc})")
    return [bytes(out[32 * i:32 * i + 32]) if has[i] else None for i in range(len(headers))]


def header_hashes(ctx, headers: List[Header]) -> List[Optional[bytes]]:
    """Header.Hash of each header (None where the reference returns nil)."""
    L = _setup_light(_setup(_native.lib()))
    return header_hashes_call(L.tmv_header_hashes, ctx.handle, headers)


# ---------------------------------------------------------------- consensus votes (ADR-064)
VOTE_OK, VOTE_ERR_INVALID_ADDRESS, VOTE_ERR_INVALID_SIGNATURE = 0, 1, 2
PREVOTE_TYPE, PRECOMMIT_TYPE = 1, 2


class CVoteIn(ctypes.Structure):
    _fields_ = [("type", ctypes.c_int32), ("height", ctypes.c_int64), ("round", ctypes.c_int32),
                ("block_id", ctypes.POINTER(CBlockID)), ("ts_seconds", ctypes.c_int64), ("ts_nanos", ctypes.c_int32),
                ("validator_address", _u8p), ("validator_address_len", ctypes.c_uint32),
                ("signature", _u8p), ("signature_len", ctypes.c_uint32), ("key_kind", ctypes.c_uint8),
                ("pub_key", _u8p), ("pub_key_len", ctypes.c_uint32)]


@dataclass
class Vote:
    """types.Vote (types/vote.go:50-62), the fields consensus votes carry."""
    type: int
    height: int
    round: int
    block_id: BlockID
    timestamp: Tuple[int, int]
    validator_address: bytes
    validator_index: int
    signature: bytes = b""
    extension: bytes = b""
    extension_signature: bytes = b""


def verify_vote_batch_call(fn, ctx_handle, chain_id: str, votes: List[Vote], keys: List[Tuple[int, bytes]]
                           ) -> List[int]:
    """votes[i] checked against keys[i] = (key kind, public key); fn =
    tmv_verify_vote_batch (or the CPU harness's twin).  Returns TMV_VOTE_* per vote."""
    k = _Keep()
    arr = (CVoteIn * max(1, len(votes)))()
    for i, (v, (kind, pk)) in enumerate(zip(votes, keys)):
        bid = None
        if v.block_id is not None and (v.block_id.hash or v.block_id.psh_total or v.block_id.psh_hash):
            b = _c_block_id(k, v.block_id)
            k.refs.append(b)
            bid = ctypes.pointer(b)
        a, al = k.buf(v.validator_address)
        s, sl = k.buf(v.signature)
        p, pl = k.buf(pk)
        arr[i] = CVoteIn(v.type, v.height, v.round, bid, v.timestamp[0], v.timestamp[1], a, al, s, sl, kind, p, pl)
    res = (ctypes.c_int32 * max(1, len(votes)))()
    rc = fn(ctx_handle, chain_id.encode(), arr, len(votes), res)
    if rc < 0:
        raise NativeError(f"tmv_verify_vote_batch failed ({rc}): {_native.last_error()}")
    return [res[i] for i in range(len(votes))]


def verify_vote_batch(ctx, chain_id: str, votes: List[Vote], keys: List[Tuple[int, bytes]]) -> List[int]:
    L = _setup(_native.lib())
    if not getattr(L, "_tmhost_votes", False):
        L.tmv_verify_vote_batch.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.POINTER(CVoteIn),
                                            ctypes.c_uint32, ctypes.POINTER(ctypes.c_int32)]
        L._tmhost_votes = True
    return verify_vote_batch_call(L.tmv_verify_vote_batch, ctx.handle, chain_id, votes, keys)


def verify_secp256k1_signatures(ctx, entries: List[Tuple[bytes, bytes, bytes]], key_cache: bool = True) -> List[bool]:
    """PubKey.VerifySignature (crypto/secp256k1/secp256k1.go:206-226) for each (key33, msg, sig64) in one
    engine call: tmv_secp256k1_verify_batch_ex with the keys' comb tables kept on the device, or (key_cache
    false) tmv_secp256k1_verify_batch.  A key or signature of another size is False, as the reference's."""
    import numpy as np
    sized = [i for i, (pk, _, sig) in enumerate(entries) if len(pk) == 33 and len(sig) == 64]
    out = [False] * len(entries)
    if not sized:
        return out
    cat = lambda k: np.frombuffer(b"".join(entries[i][k] for i in sized), np.uint8).copy()  # noqa: E731
    off = np.zeros(len(sized) + 1, np.uint32)
    off[1:] = np.cumsum([len(entries[i][1]) for i in sized])
    call = ctx.secp256k1_verify_batch_ex if key_cache else ctx.secp256k1_verify_batch
    _, valid = call(cat(0), cat(2), cat(1), off)
    for i, v in zip(sized, valid):
        out[i] = bool(v)
    return out


# ---------------------------------------------------------------- vote extensions
VOTE_MODE_VERIFY, VOTE_MODE_VERIFY_AND_EXTENSION, VOTE_MODE_EXTENSION = 0, 1, 2


class CExtVoteIn(ctypes.Structure):
    """tmv_ext_vote_in (include/tmhost.h)."""
    _fields_ = [("vote", CVoteIn), ("extension", _u8p), ("extension_len", ctypes.c_uint32),
                ("extension_signature", _u8p), ("extension_signature_len", ctypes.c_uint32)]


def _setup_vote_ext(L):
    if not getattr(L, "_tmhost_vote_ext", False):
        L.tmv_vote_extension_sign_bytes.restype = ctypes.c_size_t
        L.tmv_vote_extension_sign_bytes.argtypes = [ctypes.c_char_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_char_p,
                                                    ctypes.c_size_t, _u8p, ctypes.c_size_t]
        L.tmv_vote_extension_template_encode.restype = ctypes.c_size_t
        L.tmv_vote_extension_template_encode.argtypes = [ctypes.c_char_p, ctypes.c_int64, ctypes.c_int32, _u8p,
                                                         ctypes.c_size_t]
        L.tmv_verify_extended_votes.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_char_p,
                                                ctypes.POINTER(CExtVoteIn), ctypes.c_uint32,
                                                ctypes.POINTER(ctypes.c_int32), _u8p]
        L._tmhost_vote_ext = True
    return L


def vote_extension_sign_bytes(chain_id: str, height: int, round_: int, extension: bytes, lib=None) -> bytes:
    """types.VoteExtensionSignBytes through the C++ encoder (tmv_vote_extension_sign_bytes)."""
    L = _setup_vote_ext(lib or _native.lib())
    cap = len(extension) + len(chain_id.encode()) + 64
    out = (ctypes.c_uint8 * cap)()
    n = L.tmv_vote_extension_sign_bytes(chain_id.encode(), height, round_, extension, len(extension),
                                        ctypes.cast(out, _u8p), cap)
    return bytes(out[:n])


def vote_extension_template(chain_id: str, height: int, round_: int, lib=None) -> bytes:
    """The tail the extension messages of one (chain_id, height, round) share
    (tmv_vote_extension_template_encode)."""
    L = _setup_vote_ext(lib or _native.lib())
    cap = len(chain_id.encode()) + 32
    out = (ctypes.c_uint8 * cap)()
    n = L.tmv_vote_extension_template_encode(chain_id.encode(), height, round_, ctypes.cast(out, _u8p), cap)
    return bytes(out[:n])


def verify_extended_votes_call(fn, ctx_handle, mode: int, chain_id: str, votes: List[Vote],
                               keys: List[Tuple[int, bytes]]) -> List[Tuple[int, int]]:
    """votes[i] checked against keys[i] = (key kind, public key) as `mode` says
    (VOTE_MODE_*); fn = tmv_verify_extended_votes (or the CPU harness's twin).
    Returns (TMV_VOTE_*, failed signature: 0 none, 1 vote, 2 extension) per vote."""
    k = _Keep()
    n = len(votes)
    arr = (CExtVoteIn * max(1, n))()
    for i, (v, (kind, pk)) in enumerate(zip(votes, keys)):
        bid = None
        if v.block_id is not None and (v.block_id.hash or v.block_id.psh_total or v.block_id.psh_hash):
            b = _c_block_id(k, v.block_id)
            k.refs.append(b)
            bid = ctypes.pointer(b)
        a, al = k.buf(v.validator_address)
        s, sl = k.buf(v.signature)
        p, pl = k.buf(pk)
        e, el = k.buf(v.extension)
        es, esl = k.buf(v.extension_signature)
        arr[i] = CExtVoteIn(CVoteIn(v.type, v.height, v.round, bid, v.timestamp[0], v.timestamp[1], a, al, s, sl, kind,
                                    p, pl), e, el, es, esl)
    res = (ctypes.c_int32 * max(1, n))()
    failed = (ctypes.c_uint8 * max(1, n))()
    rc = fn(ctx_handle, mode, chain_id.encode(), arr, n, res, failed)
    if rc < 0:
        raise NativeError(f"tmv_verify_extended_votes failed ({rc}): {_native.last_error()}")
    return [(res[i], failed[i]) for i in range(n)]


def verify_extended_votes(ctx, mode: int, chain_id: str, votes: List[Vote], keys: List[Tuple[int, bytes]]
                          ) -> List[Tuple[int, int]]:
    """Vote.Verify / VerifyVoteAndExtension / VerifyExtension (types/vote.go:226-276)
    of many votes, their vote and extension signatures in one engine call per key kind."""
    L = _setup_vote_ext(_native.lib())
    return verify_extended_votes_call(L.tmv_verify_extended_votes, ctx.handle, mode, chain_id, votes, keys)


@dataclass
class ExtendedCommitSig:
    """types.ExtendedCommitSig (types/block.go:722-727): a CommitSig with the
    vote extension and its signature."""
    block_id_flag: int = BLOCK_ID_FLAG_ABSENT
    validator_address: bytes = b""
    timestamp: Tuple[int, int] = ZERO_TIME
    signature: bytes = b""
    extension: bytes = b""
    extension_signature: bytes = b""


@dataclass
class ExtendedCommit:
    """types.ExtendedCommit (types/block.go:1003-1011)."""
    height: int
    round: int
    block_id: BlockID
    extended_signatures: List[ExtendedCommitSig] = field(default_factory=list)


# ---------------------------------------------------------------- block part sets and merkle proofs
# tmv_part_set_headers / tmv_part_set_proofs / tmv_parts_verify / tmv_proofs_verify (include/tmhost.h):
# NewPartSetFromData (types/part_set.go:172-200), PartSet.AddPart (types/part_set.go:272-300),
# Proof.ValidateBasic + Proof.Verify (crypto/merkle/proof.go:52-117).
PART_OK, PART_ERR_UNEXPECTED_INDEX, PART_ERR_INVALID_PROOF = 0, 1, 2
ERR_STRIDE = 256


@dataclass
class Proof:
    """merkle.Proof (crypto/merkle/proof.go:26-31)."""
    total: int
    index: int
    leaf_hash: bytes
    aunts: List[bytes] = field(default_factory=list)


@dataclass
class Part:
    """types.Part (types/part_set.go:27-31)."""
    index: int
    bytes: bytes
    proof: Proof


class CProof(ctypes.Structure):
    _fields_ = [("total", ctypes.c_int64), ("index", ctypes.c_int64), ("leaf_hash", CBytes),
                ("aunts", ctypes.POINTER(CBytes)), ("n_aunts", ctypes.c_uint32)]


class CPartIn(ctypes.Structure):
    _fields_ = [("index", ctypes.c_uint32), ("bytes", CBytes), ("proof", CProof), ("set_total", ctypes.c_uint32),
                ("set_hash", CBytes)]


class CProofIn(ctypes.Structure):
    _fields_ = [("proof", CProof), ("leaf", CBytes), ("root", CBytes)]


def _ref_bytes(k: _Keep, b: bytes) -> CBytes:
    """CBytes over b's own buffer (no copy; b is kept alive by k)."""
    if not b:
        return CBytes(None, 0)
    k.refs.append(b)
    return CBytes(ctypes.cast(ctypes.c_char_p(b), _u8p), len(b))


def _c_proof(k: _Keep, p: Proof) -> CProof:
    arr = (CBytes * max(1, len(p.aunts)))()
    for i, a in enumerate(p.aunts):
        arr[i] = _ref_bytes(k, a)
    k.refs.append(arr)
    return CProof(p.total, p.index, _ref_bytes(k, p.leaf_hash), arr, len(p.aunts))


def _setup_merkle(L):
    if not getattr(L, "_tmhost_merkle", False):
        u32p = ctypes.POINTER(ctypes.c_uint32)
        L.tmv_part_set_headers.argtypes = [ctypes.c_void_p, ctypes.POINTER(CBytes), ctypes.c_uint32, ctypes.c_uint32,
                                           u32p, _u8p]
        L.tmv_part_set_proofs.argtypes = [ctypes.c_void_p, ctypes.POINTER(CBytes), ctypes.c_uint32, ctypes.c_uint32,
                                          u32p, _u8p, _u8p, u32p, _u8p, ctypes.c_uint64]
        L.tmv_parts_verify.argtypes = [ctypes.c_void_p, ctypes.POINTER(CPartIn), ctypes.c_uint32,
                                       ctypes.POINTER(ctypes.c_int32), ctypes.c_char_p, ctypes.c_size_t]
        L.tmv_proofs_verify.argtypes = [ctypes.c_void_p, ctypes.POINTER(CProofIn), ctypes.c_uint32,
                                        ctypes.POINTER(ctypes.c_int32), ctypes.c_char_p, ctypes.c_size_t]
        L._tmhost_merkle = True
    return L


def _handle(ctx):
    return ctx.handle if ctx is not None else None


def _texts(results, errs, n):
    raw = errs.raw
    return [None if results[i] == 0 else raw[i * ERR_STRIDE:(i + 1) * ERR_STRIDE].split(b"\0", 1)[0].decode()
            for i in range(n)]


def part_set_headers(ctx, blocks: List[bytes], part_size: int, lib=None) -> List[Tuple[int, bytes]]:
    """NewPartSetFromData(block, part_size).Header() of each block: (total, hash).
    lib: the library to call (default libtmgpu.so; the CPU tests pass the
    host layer built without the engine, with ctx = None)."""
    L = _setup_merkle(lib or _native.lib())
    k = _Keep()
    n = len(blocks)
    arr = (CBytes * max(1, n))()
    for i, b in enumerate(blocks):
        arr[i] = _ref_bytes(k, b)
    totals = (ctypes.c_uint32 * max(1, n))()
    hashes = (ctypes.c_uint8 * (32 * max(1, n)))()
    rc = L.tmv_part_set_headers(_handle(ctx), arr, n, part_size, totals, ctypes.cast(hashes, _u8p))
    if rc < 0:
        raise NativeError(f"tmv_part_set_headers failed ({rc})")
    return [(totals[i], bytes(hashes[32 * i:32 * i + 32])) for i in range(n)]


def part_set_proofs(ctx, blocks: List[bytes], part_size: int, lib=None) -> List[Tuple[int, bytes, List[Proof]]]:
    """As part_set_headers, with every part's merkle.Proof: (total, hash, proofs)."""
    L = _setup_merkle(lib or _native.lib())
    k = _Keep()
    n = len(blocks)
    arr = (CBytes * max(1, n))()
    for i, b in enumerate(blocks):
        arr[i] = _ref_bytes(k, b)
    parts = sum((len(b) + part_size - 1) // part_size for b in blocks) if part_size > 0 else 0  # 0: the library's error
    totals = (ctypes.c_uint32 * max(1, n))()
    hashes = (ctypes.c_uint8 * (32 * max(1, n)))()
    leaves = (ctypes.c_uint8 * (32 * max(1, parts)))()
    aoff = (ctypes.c_uint32 * (parts + 1))()
    cap = 32 * max(1, parts)
    aunts = (ctypes.c_uint8 * (32 * cap))()
    rc = L.tmv_part_set_proofs(_handle(ctx), arr, n, part_size, totals, ctypes.cast(hashes, _u8p),
                               ctypes.cast(leaves, _u8p), aoff, ctypes.cast(aunts, _u8p), cap)
    if rc < 0:
        raise NativeError(f"tmv_part_set_proofs failed ({rc})")
    out, p = [], 0
    lv, av = bytes(leaves), bytes(aunts)
    for b in range(n):
        proofs = []
        for i in range(totals[b]):
            proofs.append(Proof(totals[b], i, lv[32 * p:32 * p + 32],
                                [av[32 * a:32 * a + 32] for a in range(aoff[p], aoff[p + 1])]))
            p += 1
        out.append((totals[b], bytes(hashes[32 * b:32 * b + 32]), proofs))
    return out


def parts_verify(ctx, parts: List[Tuple[Part, int, bytes]], lib=None) -> List[Tuple[int, Optional[str]]]:
    """PartSet.AddPart's checks for each (part, PartSetHeader.Total, PartSetHeader.Hash):
    (PART_*, the reference's error text or None)."""
    L = _setup_merkle(lib or _native.lib())
    k = _Keep()
    n = len(parts)
    arr = (CPartIn * max(1, n))()
    for i, (part, total, hash_) in enumerate(parts):
        arr[i] = CPartIn(part.index, _ref_bytes(k, part.bytes), _c_proof(k, part.proof), total, _ref_bytes(k, hash_))
    results = (ctypes.c_int32 * max(1, n))()
    errs = ctypes.create_string_buffer(ERR_STRIDE * max(1, n))
    rc = L.tmv_parts_verify(_handle(ctx), arr, n, results, errs, ERR_STRIDE)
    if rc < 0:
        raise NativeError(f"tmv_parts_verify failed ({rc})")
    return list(zip(list(results)[:n], _texts(results, errs, n)))


def proofs_verify(ctx, items: List[Tuple[Proof, bytes, bytes]], lib=None) -> List[Optional[str]]:
    """Proof.ValidateBasic then Proof.Verify(root, leaf) of each (proof, leaf, root):
    None or the reference's error text."""
    L = _setup_merkle(lib or _native.lib())
    k = _Keep()
    n = len(items)
    arr = (CProofIn * max(1, n))()
    for i, (proof, leaf, root) in enumerate(items):
        arr[i] = CProofIn(_c_proof(k, proof), _ref_bytes(k, leaf), _ref_bytes(k, root))
    results = (ctypes.c_int32 * max(1, n))()
    errs = ctypes.create_string_buffer(ERR_STRIDE * max(1, n))
    rc = L.tmv_proofs_verify(_handle(ctx), arr, n, results, errs, ERR_STRIDE)
    if rc < 0:
        raise NativeError(f"tmv_proofs_verify failed ({rc})")
    return _texts(results, errs, n)


# ---------------------------------------------------------------- ABCI query proofs and tx proofs
# tmv_proof_ops_verify / tmv_tx_proofs_validate (include/tmhost.h): ProofRuntime.Verify under the default
# runtime (crypto/merkle/proof_op.go:35-69,114-130, proof_value.go:77-98) and TxProof.Validate
# (types/tx.go:286-301), what light/rpc/client.go checks against a trusted header.

@dataclass
class ValueOp:
    """A decoded "simple:v" ProofOp: pop.Key and ValueOp.Proof."""
    key: bytes
    proof: Proof


@dataclass
class ProofOpsItem:
    """One ProofRuntime.Verify call: keys = KeyPathToKeys(keypath), value None = VerifyAbsence."""
    ops: List[ValueOp]
    root: bytes
    keys: List[bytes]
    value: Optional[bytes]


@dataclass
class TxProof:
    """types.TxProof with the Header.DataHash it is validated against."""
    root_hash: bytes
    data: bytes
    proof: Proof
    data_hash: bytes


class CValueOp(ctypes.Structure):
    _fields_ = [("key", CBytes), ("proof", CProof)]


class CProofOpsIn(ctypes.Structure):
    _fields_ = [("ops", ctypes.POINTER(CValueOp)), ("n_ops", ctypes.c_uint32), ("root", CBytes),
                ("keys", ctypes.POINTER(CBytes)), ("n_keys", ctypes.c_uint32), ("value", ctypes.POINTER(CBytes))]


class CTxProofIn(ctypes.Structure):
    _fields_ = [("root_hash", CBytes), ("data", CBytes), ("proof", CProof), ("data_hash", CBytes)]


def _setup_proof_ops(L):
    if not getattr(L, "_tmhost_proof_ops", False):
        L.tmv_proof_ops_verify.argtypes = [ctypes.c_void_p, ctypes.POINTER(CProofOpsIn), ctypes.c_uint32,
                                           ctypes.POINTER(ctypes.c_int32), ctypes.c_char_p, ctypes.c_size_t]
        L.tmv_tx_proofs_validate.argtypes = [ctypes.c_void_p, ctypes.POINTER(CTxProofIn), ctypes.c_uint32,
                                             ctypes.POINTER(ctypes.c_int32), ctypes.c_char_p, ctypes.c_size_t]
        L._tmhost_proof_ops = True
    return L


class PreparedProofOps:
    """The C arrays of a tmv_proof_ops_verify call, built once (tools time the call alone)."""

    def __init__(self, items: List[ProofOpsItem]):
        self.k = k = _Keep()
        self.n = n = len(items)
        self.arr = (CProofOpsIn * max(1, n))()
        for i, it in enumerate(items):
            ops = (CValueOp * max(1, len(it.ops)))()
            for j, op in enumerate(it.ops):
                ops[j] = CValueOp(_ref_bytes(k, op.key), _c_proof(k, op.proof))
            keys = (CBytes * max(1, len(it.keys)))()
            for j, key in enumerate(it.keys):
                keys[j] = _ref_bytes(k, key)
            value = None
            if it.value is not None:
                value = (CBytes * 1)(_ref_bytes(k, it.value))
            k.refs += [ops, keys, value]
            self.arr[i] = CProofOpsIn(ops, len(it.ops), _ref_bytes(k, it.root), keys, len(it.keys),
                                      ctypes.cast(value, ctypes.POINTER(CBytes)) if value is not None else None)
        self.results = (ctypes.c_int32 * max(1, n))()
        self.errs = ctypes.create_string_buffer(ERR_STRIDE * max(1, n))

    def call(self, ctx, lib=None, n=None) -> int:
        """The C call alone, over the first n items (default all): the number of failed items."""
        L = _setup_proof_ops(lib or _native.lib())
        rc = L.tmv_proof_ops_verify(_handle(ctx), self.arr, self.n if n is None else n, self.results, self.errs, ERR_STRIDE)
        if rc < 0:
            raise NativeError(f"tmv_proof_ops_verify failed ({rc})")
        return rc

    def run(self, ctx, lib=None) -> List[Optional[str]]:
        self.call(ctx, lib)
        return _texts(self.results, self.errs, self.n)


def proof_ops_verify(ctx, items: List[ProofOpsItem], lib=None) -> List[Optional[str]]:
    """ProofRuntime.Verify(proof, root, keypath, args) of each item under merkle.DefaultProofRuntime():
    None or the reference's error text (cut to ERR_STRIDE - 1 bytes)."""
    return PreparedProofOps(items).run(ctx, lib)


class PreparedTxProofs:
    """The C array of a tmv_tx_proofs_validate call, built once."""

    def __init__(self, items: List[TxProof]):
        self.k = k = _Keep()
        self.n = n = len(items)
        self.arr = (CTxProofIn * max(1, n))()
        for i, it in enumerate(items):
            self.arr[i] = CTxProofIn(_ref_bytes(k, it.root_hash), _ref_bytes(k, it.data), _c_proof(k, it.proof),
                                     _ref_bytes(k, it.data_hash))
        self.results = (ctypes.c_int32 * max(1, n))()
        self.errs = ctypes.create_string_buffer(ERR_STRIDE * max(1, n))

    def call(self, ctx, lib=None, n=None) -> int:
        """The C call alone, over the first n items (default all): the number of failed items."""
        L = _setup_proof_ops(lib or _native.lib())
        rc = L.tmv_tx_proofs_validate(_handle(ctx), self.arr, self.n if n is None else n, self.results, self.errs, ERR_STRIDE)
        if rc < 0:
            raise NativeError(f"tmv_tx_proofs_validate failed ({rc})")
        return rc

    def run(self, ctx, lib=None) -> List[Optional[str]]:
        self.call(ctx, lib)
        return _texts(self.results, self.errs, self.n)


def tx_proofs_validate(ctx, items: List[TxProof], lib=None) -> List[Optional[str]]:
    """TxProof.Validate(dataHash) of each item: None or the reference's error text."""
    return PreparedTxProofs(items).run(ctx, lib)


# ---------------------------------------------------------------- blocks
# tmv_commit_hash_many / tmv_blocks_validate_basic (include/tmhost.h): Commit.Hash
# (types/block.go:900-918) and Block.ValidateBasic (types/block.go:53-94).

class CBlock(ctypes.Structure):
    _fields_ = [("header", CHeader), ("txs", ctypes.POINTER(CBytes)), ("n_txs", ctypes.c_uint32),
                ("evidence", ctypes.POINTER(CBytes)), ("n_evidence", ctypes.c_uint32),
                ("last_commit", ctypes.POINTER(CCommit))]


@dataclass
class FullBlock:
    """The parts of a types.Block that blocksync's checks read: the header, the
    transactions, the evidence list (ev.Bytes() of each item), the last commit
    and, optionally, the serialised block as received (its part set)."""
    header: Header
    txs: List[bytes] = field(default_factory=list)
    evidence: List[bytes] = field(default_factory=list)
    last_commit: Optional[Commit] = None
    raw: Optional[bytes] = None

    @property
    def height(self) -> int:
        return self.header.height


def _setup_blocks(L):
    if not getattr(L, "_tmhost_blocks", False):
        L.tmv_commit_hash_many.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.POINTER(CCommit)), ctypes.c_uint32,
                                           _u8p, _u8p]
        L.tmv_blocks_validate_basic.argtypes = [ctypes.c_void_p, ctypes.POINTER(CBlock), ctypes.c_uint32,
                                                ctypes.POINTER(ctypes.c_int32), ctypes.c_char_p, ctypes.c_size_t,
                                                _u8p, _u8p]
        L._tmhost_blocks = True
    return L


def commit_hashes(ctx, commits: List[Optional[Commit]], lib=None) -> List[Optional[bytes]]:
    """Commit.Hash of each commit (None for a nil commit).  lib: the library to
    call (default libtmgpu.so; the CPU tests pass the host layer built without
    the engine, with ctx = None)."""
    L = _setup_blocks(lib or _native.lib())
    k = _Keep()
    n = len(commits)
    arr = (ctypes.POINTER(CCommit) * max(1, n))()
    for i, c in enumerate(commits):
        if c is not None:
            arr[i] = ctypes.pointer(_c_commit(k, c))
    out = (ctypes.c_uint8 * (32 * max(1, n)))()
    has = (ctypes.c_uint8 * max(1, n))()
    rc = L.tmv_commit_hash_many(_handle(ctx), arr, n, ctypes.cast(out, _u8p), ctypes.cast(has, _u8p))
    if rc < 0:
        raise NativeError(f"tmv_commit_hash_many failed ({rc})")
    return [bytes(out[32 * i:32 * i + 32]) if has[i] else None for i in range(n)]


class PreparedBlocks:
    """tmv_block[] for a list of FullBlock, built once (on the caller's thread;
    the engine call may run on another)."""

    def __init__(self, blocks: List[FullBlock]):
        self.keep = k = _Keep()
        self.n = n = len(blocks)
        self.arr = (CBlock * max(1, n))()
        for i, b in enumerate(blocks):
            txs = (CBytes * max(1, len(b.txs)))()
            for j, t in enumerate(b.txs):
                txs[j] = _ref_bytes(k, t)
            evs = (CBytes * max(1, len(b.evidence)))()
            for j, e in enumerate(b.evidence):
                evs[j] = _ref_bytes(k, e)
            k.refs += [txs, evs]
            lc = ctypes.pointer(_c_commit(k, b.last_commit)) if b.last_commit is not None else None
            self.arr[i] = CBlock(_c_header(k, b.header), txs, len(b.txs), evs, len(b.evidence), lc)
        self.results = (ctypes.c_int32 * max(1, n))()
        self.errs = ctypes.create_string_buffer(ERR_STRIDE * max(1, n))
        self.hashes = (ctypes.c_uint8 * (32 * max(1, n)))()
        self.has = (ctypes.c_uint8 * max(1, n))()

    def run(self, ctx, lib=None) -> List[Tuple[Optional[str], Optional[bytes]]]:
        L = _setup_blocks(lib or _native.lib())
        rc = L.tmv_blocks_validate_basic(_handle(ctx), self.arr, self.n, self.results, self.errs, ERR_STRIDE,
                                         ctypes.cast(self.hashes, _u8p), ctypes.cast(self.has, _u8p))
        if rc < 0:
            raise NativeError(f"tmv_blocks_validate_basic failed ({rc})")
        texts = _texts(self.results, self.errs, self.n)
        raw = bytes(self.hashes)
        return [(texts[i], raw[32 * i:32 * i + 32] if self.has[i] else None) for i in range(self.n)]


def blocks_validate_basic(ctx, blocks: List[FullBlock], lib=None) -> List[Tuple[Optional[str], Optional[bytes]]]:
    """Block.ValidateBasic of each block: (the reference's error text or None,
    Header.Hash of the header as given, which is Block.Hash() of a block that
    passes, or None where the reference returns nil)."""
    return PreparedBlocks(blocks).run(ctx, lib)


# ---------------------------------------------------------------- blocks from their protobuf bytes
# tmv_blocks_validate_wire / tmv_blocks_parse_wire (include/tmhost.h).

WIRE_OK, WIRE_INVALID, WIRE_NOT_HANDLED = 0, 1, 2
WIRE_REASONS = ("NONE", "TRUNCATED", "WIRE_TYPE", "UNKNOWN_FIELD", "ORDER", "VARINT", "ZERO_PRESENT", "MISSING",
                "TIME", "EVIDENCE", "CHAIN_ID", "LIMIT")


@dataclass
class WireVerdict:
    """One block of tmv_blocks_validate_wire.  result: WIRE_OK / WIRE_INVALID
    (error: Block.ValidateBasic's text) / WIRE_NOT_HANDLED (reason: a name of
    WIRE_REASONS).  hash: Header.Hash of a handled block (None where the
    reference returns nil); part_set_header: (total, hash), or None without a
    part size; block: the decoded view of a handled block, when asked for."""
    result: int
    reason: str = "NONE"
    error: Optional[str] = None
    hash: Optional[bytes] = None
    part_set_header: Optional[Tuple[int, bytes]] = None
    block: Optional[FullBlock] = None


def _setup_block_wire(L):
    if not getattr(L, "_tmhost_block_wire", False):
        u32p, i32p = ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_int32)
        L.tmv_blocks_validate_wire.argtypes = [ctypes.c_void_p, _u8p, u32p, ctypes.c_uint32, ctypes.c_uint32, i32p,
                                               i32p, ctypes.c_char_p, ctypes.c_size_t, _u8p, _u8p, u32p, _u8p,
                                               ctypes.POINTER(ctypes.c_void_p)]
        L.tmv_blocks_parse_wire.argtypes = [_u8p, u32p, ctypes.c_uint32, i32p, ctypes.POINTER(ctypes.c_void_p)]
        L.tmv_block_views_block.restype = ctypes.POINTER(CBlock)
        L.tmv_block_views_block.argtypes = [ctypes.c_void_p, ctypes.c_uint32]
        L.tmv_block_views_free.restype = None
        L.tmv_block_views_free.argtypes = [ctypes.c_void_p]
        L._tmhost_block_wire = True
    return L


class WireWindow:
    """The bytes of a list of serialised blocks in one buffer with their
    offsets (data, block_off), as tmv_blocks_validate_wire takes them."""

    def __init__(self, raws: List[bytes]):
        self.n = n = len(raws)
        blob = b"".join(raws)
        self.data = (ctypes.c_uint8 * max(1, len(blob))).from_buffer_copy(blob or b"\0")
        self.off = (ctypes.c_uint32 * (n + 1))()
        at = 0
        for i, r in enumerate(raws):
            at += len(r)
            self.off[i + 1] = at
        self.raws = raws


def _take(p, n: int) -> bytes:
    return ctypes.string_at(p, n) if n else b""


def _py_block_id(b: CBlockID) -> BlockID:
    return BlockID(_take(b.hash, b.hash_len), b.psh_total, _take(b.psh_hash, b.psh_hash_len))


class _ViewsOwner:
    """A tmv_block_views object and the bytes it points into, freed with the
    last Python object that refers to them."""

    def __init__(self, L, handle, window: WireWindow, free=None):
        self.L, self.handle, self.window = L, handle, window
        self.free = free or L.tmv_block_views_free

    def __del__(self):
        self.free(self.handle)


class ViewCommit:
    """The last commit of a block decoded by tmv_blocks_validate_wire, left
    where it is: a tmv_commit inside a tmv_block_views object.  PreparedJobs
    passes it to tmv_verify_commits by pointer, so a window's signatures are
    never turned into Python objects and back; read as a Commit (height, round,
    block_id, signatures, ==) it is decoded on first use."""

    def __init__(self, ptr, owner: _ViewsOwner):
        self.ptr, self.owner, self._commit = ptr, owner, None

    def decoded(self) -> Commit:
        if self._commit is None:
            lc = self.ptr.contents
            self._commit = Commit(lc.height, lc.round, _py_block_id(lc.block_id),
                                  [CommitSig(s.block_id_flag, _take(s.validator_address, s.validator_address_len),
                                             (s.ts_seconds, s.ts_nanos), _take(s.signature, s.signature_len))
                                   for s in (lc.sigs[j] for j in range(lc.n_sigs))])
        return self._commit

    height = property(lambda self: self.decoded().height)
    round = property(lambda self: self.decoded().round)
    block_id = property(lambda self: self.decoded().block_id)
    signatures = property(lambda self: self.decoded().signatures)

    def __eq__(self, o):
        if isinstance(o, ViewCommit):
            o = o.decoded()
        return self.decoded() == o if isinstance(o, Commit) else NotImplemented

    def __repr__(self):
        return "View" + repr(self.decoded())


def _py_block(c: CBlock, raw: bytes, owner: _ViewsOwner) -> FullBlock:
    """A FullBlock copied out of a tmv_block view; its last commit stays in the view."""
    h = c.header
    hdr = Header((h.chain_id or b"").decode("ascii"), h.height, (h.time_seconds, h.time_nanos),
                 _py_block_id(h.last_block_id), *[_take(getattr(h, f).p, getattr(h, f).len) for f in _HASH_FIELDS],
                 version_block=h.version_block, version_app=h.version_app)
    commit = ViewCommit(c.last_commit, owner) if c.last_commit else None
    return FullBlock(hdr, [_take(c.txs[j].p, c.txs[j].len) for j in range(c.n_txs)], [], commit, raw)


def _py_views(L, views, w: WireWindow) -> List[Optional[FullBlock]]:
    """The handled blocks of a views object, which the blocks' commits keep alive."""
    owner = _ViewsOwner(L, views, w)
    out = []
    for i in range(w.n):
        p = L.tmv_block_views_block(views, i)
        out.append(_py_block(p.contents, w.raws[i], owner) if p else None)
    return out


def blocks_parse_wire(raws: List[bytes], lib=None) -> List[Optional[FullBlock]]:
    """The strict scanner alone: each block decoded from its canonical
    protobuf bytes (its `raw` the bytes themselves), None where the bytes are
    not handled (blocks_validate_wire names the reason)."""
    L = _setup_block_wire(lib or _native.lib())
    w = WireWindow(raws)
    views = ctypes.c_void_p()
    rc = L.tmv_blocks_parse_wire(ctypes.cast(w.data, _u8p), w.off, w.n, None, ctypes.byref(views))
    if rc < 0:
        raise NativeError(f"tmv_blocks_parse_wire failed ({rc})")
    return _py_views(L, views, w)


def blocks_validate_wire(ctx, raws: List[bytes], part_size: int = 0, lib=None, decode: bool = False
                         ) -> List[WireVerdict]:
    """Block.ValidateBasic of each serialised block from its bytes
    (tmv_blocks_validate_wire): a window of at least TMV_DEVICE_BLOCK_MIN
    handled blocks is hashed on the device in one upload.  part_size != 0 adds
    every block's part-set header; decode=True the decoded view of every
    handled block (its last commit a ViewCommit)."""
    L = _setup_block_wire(lib or _native.lib())
    w = WireWindow(raws)
    n, m = w.n, max(1, w.n)
    results, reason = (ctypes.c_int32 * m)(), (ctypes.c_int32 * m)()
    errs = ctypes.create_string_buffer(ERR_STRIDE * m)
    hashes, has = (ctypes.c_uint8 * (32 * m))(), (ctypes.c_uint8 * m)()
    totals, phash = (ctypes.c_uint32 * m)(), (ctypes.c_uint8 * (32 * m))()
    views = ctypes.c_void_p()
    rc = L.tmv_blocks_validate_wire(_handle(ctx), ctypes.cast(w.data, _u8p), w.off, n, part_size, results, reason,
                                    errs, ERR_STRIDE, ctypes.cast(hashes, _u8p), ctypes.cast(has, _u8p), totals,
                                    ctypes.cast(phash, _u8p), ctypes.byref(views) if decode else None)
    if rc < 0:
        raise NativeError(f"tmv_blocks_validate_wire failed ({rc})")
    blocks = _py_views(L, views, w) if decode else [None] * n
    raw_h, raw_p, err_raw = bytes(hashes), bytes(phash), errs.raw
    out = []
    for i in range(n):
        text = None
        if results[i] == WIRE_INVALID:
            text = err_raw[i * ERR_STRIDE:(i + 1) * ERR_STRIDE].split(b"\0", 1)[0].decode()
        out.append(WireVerdict(results[i], WIRE_REASONS[reason[i]], text,
                               raw_h[32 * i:32 * i + 32] if has[i] else None,
                               (totals[i], raw_p[32 * i:32 * i + 32]) if part_size else None, blocks[i]))
    return out


# ---------------------------------------------------------------- light blocks from their protobuf bytes
# tmv_light_blocks_validate_wire / tmv_light_blocks_parse_wire (include/tmhost.h).

LIGHT_WIRE_REASONS = WIRE_REASONS + ("KEY", "PROPOSER", "POWER")


def _py_header(h: CHeader) -> Header:
    return Header((h.chain_id or b"").decode("ascii"), h.height, (h.time_seconds, h.time_nanos),
                  _py_block_id(h.last_block_id), *[_take(getattr(h, f).p, getattr(h, f).len) for f in _HASH_FIELDS],
                  version_block=h.version_block, version_app=h.version_app)


class ViewSignedHeader:
    """The signed header of a light block decoded by
    tmv_light_blocks_validate_wire, left where it is: a tmv_signed_header
    inside a tmv_light_block_views object.  PreparedLightJobs passes it to
    tmv_light_verify_many by pointer; read as a SignedHeader (header, commit,
    height, ==) it is decoded on first use.  A nil header or commit is None."""

    def __init__(self, ptr, owner: _ViewsOwner):
        self.ptr, self.owner, self._header, self._commit = ptr, owner, None, None

    @property
    def header(self) -> Optional[Header]:
        c = self.ptr.contents
        if self._header is None and c.header:
            self._header = _py_header(c.header.contents)
        return self._header

    @property
    def commit(self) -> Optional[Commit]:
        c = self.ptr.contents
        if self._commit is None and c.commit:
            self._commit = ViewCommit(c.commit, self.owner).decoded()
        return self._commit

    @property
    def height(self) -> int:
        return self.ptr.contents.header.contents.height

    def decoded(self) -> SignedHeader:
        return SignedHeader(self.header, self.commit)

    def __eq__(self, o):
        if isinstance(o, ViewSignedHeader):
            o = o.decoded()
        return self.decoded() == o if isinstance(o, SignedHeader) else NotImplemented

    def __repr__(self):
        return "View" + repr(self.decoded())


class ViewValidatorSet:
    """The validator set of a light block decoded by
    tmv_light_blocks_validate_wire: a tmv_validator_set inside the views
    object, passed to tmv_light_verify_many by pointer; read as a ValidatorSet
    (validators, proposer_index, ==) it is decoded on first use."""

    def __init__(self, ptr, owner: _ViewsOwner):
        self.ptr, self.owner, self._vals = ptr, owner, None

    def decoded(self) -> ValidatorSet:
        if self._vals is None:
            c = self.ptr.contents
            self._vals = ValidatorSet([Validator(_take(v.address, v.address_len), _take(v.pub_key, v.pub_key_len),
                                                 v.voting_power, v.key_kind, v.proposer_priority)
                                       for v in (c.vals[j] for j in range(c.n_vals))], c.proposer_index)
        return self._vals

    validators = property(lambda self: self.decoded().validators)
    proposer_index = property(lambda self: self.decoded().proposer_index)

    def total_voting_power(self) -> int:
        return self.decoded().total_voting_power()

    def __eq__(self, o):
        if isinstance(o, ViewValidatorSet):
            o = o.decoded()
        return self.decoded() == o if isinstance(o, ValidatorSet) else NotImplemented

    def __repr__(self):
        return "View" + repr(self.decoded())


@dataclass
class LightWireVerdict:
    """One light block of tmv_light_blocks_validate_wire.  result: WIRE_OK /
    WIRE_INVALID (error: LightBlock.ValidateBasic's text) / WIRE_NOT_HANDLED
    (reason: a name of LIGHT_WIRE_REASONS).  hash: Header.Hash (None where the
    header is nil or has none); vals_hash: ValidatorSet.Hash (None for a nil or
    empty set); signed_header / vals: the views of a handled block, when asked
    for (None where the block has none)."""
    result: int
    reason: str = "NONE"
    error: Optional[str] = None
    hash: Optional[bytes] = None
    vals_hash: Optional[bytes] = None
    signed_header: Optional[ViewSignedHeader] = None
    vals: Optional[ViewValidatorSet] = None


def _setup_light_wire(L):
    if not getattr(L, "_tmhost_light_wire", False):
        u32p, i32p = ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_int32)
        L.tmv_light_blocks_validate_wire.argtypes = [ctypes.c_void_p, ctypes.c_char_p, _u8p, u32p, ctypes.c_uint32,
                                                     i32p, i32p, ctypes.c_char_p, ctypes.c_size_t, _u8p, _u8p, _u8p,
                                                     ctypes.POINTER(ctypes.c_void_p)]
        L.tmv_light_blocks_parse_wire.argtypes = [_u8p, u32p, ctypes.c_uint32, i32p, ctypes.POINTER(ctypes.c_void_p)]
        L.tmv_light_block_views_header.restype = ctypes.POINTER(CSignedHeader)
        L.tmv_light_block_views_header.argtypes = [ctypes.c_void_p, ctypes.c_uint32]
        L.tmv_light_block_views_vals.restype = ctypes.POINTER(CValidatorSet)
        L.tmv_light_block_views_vals.argtypes = [ctypes.c_void_p, ctypes.c_uint32]
        L.tmv_light_block_views_free.restype = None
        L.tmv_light_block_views_free.argtypes = [ctypes.c_void_p]
        L._tmhost_light_wire = True
    return L


def _py_light_views(L, views, w: WireWindow):
    """(signed header view, validator set view) of every light block of a views object."""
    owner = _ViewsOwner(L, views, w, L.tmv_light_block_views_free)
    out = []
    for i in range(w.n):
        sh, vs = L.tmv_light_block_views_header(views, i), L.tmv_light_block_views_vals(views, i)
        out.append((ViewSignedHeader(sh, owner) if sh else None, ViewValidatorSet(vs, owner) if vs else None))
    return out


def light_blocks_parse_wire(raws: List[bytes], lib=None):
    """The strict scanner alone: per light block (reason name, signed header
    view, validator set view), the views None where the bytes are not handled
    or the block has none."""
    L = _setup_light_wire(lib or _native.lib())
    w = WireWindow(raws)
    reason = (ctypes.c_int32 * max(1, w.n))()
    views = ctypes.c_void_p()
    rc = L.tmv_light_blocks_parse_wire(ctypes.cast(w.data, _u8p), w.off, w.n, reason, ctypes.byref(views))
    if rc < 0:
        raise NativeError(f"tmv_light_blocks_parse_wire failed ({rc})")
    return [(LIGHT_WIRE_REASONS[reason[i]],) + v for i, v in enumerate(_py_light_views(L, views, w))]


def light_blocks_validate_wire(ctx, chain_id: str, raws: List[bytes], lib=None, decode: bool = False
                               ) -> List[LightWireVerdict]:
    """LightBlock.ValidateBasic(chain_id) of each serialised light block from
    its bytes (tmv_light_blocks_validate_wire), with Header.Hash and
    ValidatorSet.Hash: a window of at least TMV_DEVICE_HASH_MIN handled light
    blocks is hashed on the device in one upload.  decode=True adds the views
    of every handled block, which go into a LightJob as they are."""
    L = _setup_light_wire(lib or _native.lib())
    w = WireWindow(raws)
    n, m = w.n, max(1, w.n)
    results, reason = (ctypes.c_int32 * m)(), (ctypes.c_int32 * m)()
    errs = ctypes.create_string_buffer(ERR_STRIDE * m)
    hashes, vhashes, has = (ctypes.c_uint8 * (32 * m))(), (ctypes.c_uint8 * (32 * m))(), (ctypes.c_uint8 * m)()
    views = ctypes.c_void_p()
    rc = L.tmv_light_blocks_validate_wire(_handle(ctx), chain_id.encode(), ctypes.cast(w.data, _u8p), w.off, n,
                                          results, reason, errs, ERR_STRIDE, ctypes.cast(hashes, _u8p),
                                          ctypes.cast(has, _u8p), ctypes.cast(vhashes, _u8p),
                                          ctypes.byref(views) if decode else None)
    if rc < 0:
        raise NativeError(f"tmv_light_blocks_validate_wire failed ({rc})")
    vs = _py_light_views(L, views, w) if decode else [(None, None)] * n
    raw_h, raw_v, err_raw = bytes(hashes), bytes(vhashes), errs.raw
    out = []
    for i in range(n):
        text = None
        if results[i] == WIRE_INVALID:
            text = err_raw[i * ERR_STRIDE:(i + 1) * ERR_STRIDE].split(b"\0", 1)[0].decode()
        out.append(LightWireVerdict(results[i], LIGHT_WIRE_REASONS[reason[i]], text,
                                    raw_h[32 * i:32 * i + 32] if has[i] & 1 else None,
                                    raw_v[32 * i:32 * i + 32] if has[i] & 2 else None, vs[i][0], vs[i][1]))
    return out


# ---------------------------------------------------------------- ABCI results and consensus params
# tmv_results_hash_many / tmv_consensus_params_hash / tmv_block_results_verify /
# tmv_consensus_params_verify (include/tmhost.h): the merkle root over abci.MarshalTxResults
# (abci/types/types.go:213-239), HashConsensusParams (types/params.go:385-399) and the checks of the light
# client's BlockResults and ConsensusParams (light/rpc/client.go:264-291, 420-473).

@dataclass
class TxResult:
    """The deterministic fields of abci.ExecTxResult (abci/types/types.go:213-222)."""
    code: int = 0
    data: bytes = b""
    gas_wanted: int = 0
    gas_used: int = 0


@dataclass
class BlockResults:
    """coretypes.ResultBlockResults as the light client checks it: events =
    proto.Marshal(ResponseFinalizeBlock{Events}), last_results_hash = the
    trusted header's at height + 1."""
    height: int
    results: List[TxResult]
    events: bytes
    last_results_hash: bytes


@dataclass
class ConsensusParamsResult:
    """coretypes.ResultConsensusParams' hashed fields with the trusted header's ConsensusHash."""
    height: int
    block_max_bytes: int
    block_max_gas: int
    consensus_hash: bytes


class CTxResult(ctypes.Structure):
    _fields_ = [("code", ctypes.c_uint32), ("data", CBytes), ("gas_wanted", ctypes.c_int64),
                ("gas_used", ctypes.c_int64)]


class CBlockResultsIn(ctypes.Structure):
    _fields_ = [("height", ctypes.c_int64), ("results", ctypes.POINTER(CTxResult)), ("n_results", ctypes.c_uint32),
                ("events", CBytes), ("last_results_hash", CBytes)]


class CConsensusParamsIn(ctypes.Structure):
    _fields_ = [("height", ctypes.c_int64), ("block_max_bytes", ctypes.c_int64), ("block_max_gas", ctypes.c_int64),
                ("consensus_hash", CBytes)]


def _setup_results(L):
    if not getattr(L, "_tmhost_results", False):
        i32p = ctypes.POINTER(ctypes.c_int32)
        L.tmv_results_hash_many.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.POINTER(CTxResult)),
                                            ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(CBytes), ctypes.c_uint32,
                                            _u8p]
        L.tmv_consensus_params_hash.argtypes = [ctypes.c_int64, ctypes.c_int64, _u8p]
        L.tmv_block_results_verify.argtypes = [ctypes.c_void_p, ctypes.POINTER(CBlockResultsIn), ctypes.c_uint32, i32p,
                                               ctypes.c_char_p, ctypes.c_size_t]
        L.tmv_consensus_params_verify.argtypes = [ctypes.c_void_p, ctypes.POINTER(CConsensusParamsIn),
                                                  ctypes.c_uint32, i32p, ctypes.c_char_p, ctypes.c_size_t]
        L._tmhost_results = True
    return L


def _c_tx_results(k: _Keep, results: List[TxResult]):
    arr = (CTxResult * max(1, len(results)))()
    for j, r in enumerate(results):
        arr[j] = CTxResult(r.code, _ref_bytes(k, r.data), r.gas_wanted, r.gas_used)
    k.refs.append(arr)
    return arr


class PreparedResults:
    """The C arrays of a tmv_results_hash_many call, built once (on the
    caller's thread; the engine call may run on another)."""

    def __init__(self, lists: List[List[TxResult]], first: Optional[List[bytes]] = None):
        self.k = k = _Keep()
        self.n = n = len(lists)
        self.ptrs = (ctypes.POINTER(CTxResult) * max(1, n))()
        self.counts = (ctypes.c_uint32 * max(1, n))()
        for i, rs in enumerate(lists):
            self.ptrs[i] = ctypes.cast(_c_tx_results(k, rs), ctypes.POINTER(CTxResult))
            self.counts[i] = len(rs)
        self.first = None
        if first is not None:
            self.first = (CBytes * max(1, n))()
            for i, b in enumerate(first):
                self.first[i] = _ref_bytes(k, b)
        self.out = (ctypes.c_uint8 * (32 * max(1, n)))()

    def run(self, ctx, lib=None) -> List[bytes]:
        L = _setup_results(lib or _native.lib())
        rc = L.tmv_results_hash_many(_handle(ctx), self.ptrs, self.counts, self.first, self.n,
                                     ctypes.cast(self.out, _u8p))
        if rc < 0:
            raise NativeError(f"tmv_results_hash_many failed ({rc})")
        raw = bytes(self.out)
        return [raw[32 * i:32 * i + 32] for i in range(self.n)]


def results_hashes(ctx, lists: List[List[TxResult]], first: Optional[List[bytes]] = None, lib=None) -> List[bytes]:
    """The merkle root over abci.MarshalTxResults of each list of results:
    State.LastResultsHash as ApplyBlock stores it.  first: one leading leaf
    per list (may be empty), the light client's form.  lib: the library to
    call (default libtmgpu.so; the CPU tests pass the host layer built without
    the engine, with ctx = None)."""
    return PreparedResults(lists, first).run(ctx, lib)


def consensus_params_hash(block_max_bytes: int, block_max_gas: int, lib=None) -> bytes:
    """ConsensusParams.HashConsensusParams (types/params.go:385-399)."""
    L = _setup_results(lib or _native.lib())
    out = (ctypes.c_uint8 * 32)()
    rc = L.tmv_consensus_params_hash(block_max_bytes, block_max_gas, ctypes.cast(out, _u8p))
    if rc < 0:
        raise NativeError(f"tmv_consensus_params_hash failed ({rc})")
    return bytes(out)


def block_results_verify(ctx, items: List[BlockResults], lib=None) -> List[Optional[str]]:
    """The checks of the light client's BlockResults after the fetch, for each
    response: None or the reference's error text."""
    L = _setup_results(lib or _native.lib())
    k = _Keep()
    n = len(items)
    arr = (CBlockResultsIn * max(1, n))()
    for i, it in enumerate(items):
        arr[i] = CBlockResultsIn(it.height, _c_tx_results(k, it.results), len(it.results), _ref_bytes(k, it.events),
                                 _ref_bytes(k, it.last_results_hash))
    results = (ctypes.c_int32 * max(1, n))()
    errs = ctypes.create_string_buffer(ERR_STRIDE * max(1, n))
    rc = L.tmv_block_results_verify(_handle(ctx), arr, n, results, errs, ERR_STRIDE)
    if rc < 0:
        raise NativeError(f"tmv_block_results_verify failed ({rc})")
    return _texts(results, errs, n)


def consensus_params_verify(ctx, items: List[ConsensusParamsResult], lib=None) -> List[Optional[str]]:
    """The last two checks of the light client's ConsensusParams, for each
    response: None or the reference's error text."""
    L = _setup_results(lib or _native.lib())
    k = _Keep()
    n = len(items)
    arr = (CConsensusParamsIn * max(1, n))()
    for i, it in enumerate(items):
        arr[i] = CConsensusParamsIn(it.height, it.block_max_bytes, it.block_max_gas, _ref_bytes(k, it.consensus_hash))
    results = (ctypes.c_int32 * max(1, n))()
    errs = ctypes.create_string_buffer(ERR_STRIDE * max(1, n))
    rc = L.tmv_consensus_params_verify(_handle(ctx), arr, n, results, errs, ERR_STRIDE)
    if rc < 0:
        raise NativeError(f"tmv_consensus_params_verify failed ({rc})")
    return _texts(results, errs, n)


# ---- validator-set updates (include/tmhost.h: tmv_validator_set_update / _new / _rotate / _hash_host) ----
# types/validator_set.go:70-234, 362-650 on the host, no engine: what State.Update does to NextValidators.

VALSET_OK, VALSET_ERROR, VALSET_PANIC = 0, 1, 2
KEY_TYPE_NAMES = {TMV_KIND_ED25519: "ed25519", TMV_KIND_SR25519: "sr25519", TMV_KIND_SECP256K1: "secp256k1"}


class ValidatorSetPanic(Exception):
    """The reference panics here (TMV_VALSET_PANIC); the text is the panic's."""


@dataclass
class ValidatorUpdate:
    """abci.ValidatorUpdate: the key and the new power (0 removes the validator)."""
    key_kind: int
    pub_key: bytes
    power: int


class CValidatorUpdate(ctypes.Structure):
    _fields_ = [("key_kind", ctypes.c_uint8), ("pub_key", _u8p), ("pub_key_len", ctypes.c_uint32),
                ("power", ctypes.c_int64)]


def _setup_valset(L):
    if not getattr(L, "_tmhost_valset", False):
        vp, up = ctypes.POINTER(CValidator), ctypes.POINTER(CValidatorUpdate)
        u32p, i32p = ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_int32)
        L.tmv_validator_set_update.argtypes = [vp, ctypes.c_uint32, up, ctypes.c_uint32, ctypes.c_int, _u8p, vp,
                                               ctypes.c_uint32, u32p, ctypes.c_char_p, ctypes.c_size_t]
        L.tmv_validator_set_new.argtypes = [up, ctypes.c_uint32, _u8p, vp, ctypes.c_uint32, u32p, i32p,
                                            ctypes.c_char_p, ctypes.c_size_t]
        L.tmv_validator_set_rotate.argtypes = [vp, ctypes.c_uint32, ctypes.c_int32, ctypes.c_uint32, i32p,
                                               ctypes.c_char_p, ctypes.c_size_t]
        L.tmv_validator_set_hash_host.argtypes = [vp, ctypes.c_uint32, _u8p]
        L._tmhost_valset = True
    return L


def _valset_array(k: _Keep, vals: ValidatorSet):
    """(numpy tmv_validator[], pointer -> the bytes object it points to) for a set."""
    _c_validators(k, vals)
    a = k.refs[-1]
    n = len(vals.validators)
    back = dict(zip(a["address"][:n].tolist(), (v.address for v in vals.validators)))
    back.update(zip(a["pub_key"][:n].tolist(), (v.pub_key for v in vals.validators)))
    return a, back


def _c_updates(k: _Keep, updates):
    import numpy as np
    ups = [u if isinstance(u, ValidatorUpdate) else ValidatorUpdate(*u) for u in updates]
    a = np.zeros(max(1, len(ups)), dtype=_dt("vu", CValidatorUpdate))
    back = {}
    if ups:
        n = len(ups)
        a["pub_key"][:n], a["pub_key_len"][:n] = _blob_ptrs(k, [u.pub_key for u in ups])
        a["key_kind"][:n] = [u.key_kind for u in ups]
        a["power"][:n] = [u.power for u in ups]
        back = dict(zip(a["pub_key"][:n].tolist(), (u.pub_key for u in ups)))
    k.refs.append(a)
    return a, len(ups), back


def _valset_result(rc: int, err, what: str) -> Optional[str]:
    if rc == VALSET_OK:
        return None
    text = err.value.decode(errors="replace")
    if rc == VALSET_ERROR:
        return text
    if rc == VALSET_PANIC:
        raise ValidatorSetPanic(text)
    raise NativeError(f"{what} failed ({rc})")


def _py_valset(out, n: int, back, scratch, proposer_index: int = -1) -> ValidatorSet:
    """The output array of a set call: keys and addresses by the pointers they
    borrow (an input's bytes object, or 20 bytes of the address scratch)."""
    base = ctypes.addressof(scratch) if scratch is not None else 0
    raw = bytes(scratch) if scratch is not None else b""

    def take(p):
        b = back.get(p)
        if b is None:
            b = back[p] = raw[p - base:p - base + 20] if p else b""
        return b
    return ValidatorSet([Validator(take(ap), take(kp), pw, kk, pr) for ap, kp, pw, kk, pr in zip(
        out["address"][:n].tolist(), out["pub_key"][:n].tolist(), out["voting_power"][:n].tolist(),
        out["key_kind"][:n].tolist(), out["proposer_priority"][:n].tolist())], proposer_index)


def validator_set_update(vals: ValidatorSet, updates, allow_deletes: bool = True, lib=None
                         ) -> Tuple[Optional[ValidatorSet], Optional[str]]:
    """ValidatorSet.UpdateWithChangeSet (types/validator_set.go:584-650) on a
    copy: (the new set, None) or (None, the reference's error text); a
    ValidatorSetPanic where the reference panics.  updates: ValidatorUpdate or
    (key kind, key, power); the address follows from the key as NewValidator
    derives it.  The new set's proposer_index is -1: State.Update goes on to
    IncrementProposerPriority(1) (validator_set_rotate)."""
    import numpy as np
    L = _setup_valset(lib or _native.lib())
    k = _Keep()
    a, back = _valset_array(k, vals)
    u, nu, uback = _c_updates(k, updates)
    back.update(uback)
    nv = len(vals.validators)
    scratch = (ctypes.c_uint8 * max(1, 20 * nu))()
    out = np.zeros(max(1, nv + nu), dtype=_dt("v", CValidator))
    n_out = ctypes.c_uint32(0)
    err = ctypes.create_string_buffer(4096)
    vp, up = ctypes.POINTER(CValidator), ctypes.POINTER(CValidatorUpdate)
    rc = L.tmv_validator_set_update(ctypes.cast(a.ctypes.data, vp), nv, ctypes.cast(u.ctypes.data, up), nu,
                                    1 if allow_deletes else 0, ctypes.cast(scratch, _u8p),
                                    ctypes.cast(out.ctypes.data, vp), nv + nu, ctypes.byref(n_out), err, len(err))
    text = _valset_result(rc, err, "tmv_validator_set_update")
    if text is not None:
        return None, text
    return _py_valset(out, n_out.value, back, scratch), None


def new_validator_set(validators, lib=None) -> ValidatorSet:
    """NewValidatorSet (types/validator_set.go:70-80) over (key kind, key,
    power) entries: the set in set order with the priorities and the proposer
    of its first election.  The reference panics on a change set that fails:
    a ValidatorSetPanic with "cannot create validator set: ..."."""
    import numpy as np
    L = _setup_valset(lib or _native.lib())
    k = _Keep()
    u, nu, back = _c_updates(k, validators)
    scratch = (ctypes.c_uint8 * max(1, 20 * nu))()
    out = np.zeros(max(1, nu), dtype=_dt("v", CValidator))
    n_out, prop = ctypes.c_uint32(0), ctypes.c_int32(-1)
    err = ctypes.create_string_buffer(4096)
    vp, up = ctypes.POINTER(CValidator), ctypes.POINTER(CValidatorUpdate)
    rc = L.tmv_validator_set_new(ctypes.cast(u.ctypes.data, up), nu, ctypes.cast(scratch, _u8p),
                                 ctypes.cast(out.ctypes.data, vp), nu, ctypes.byref(n_out), ctypes.byref(prop), err,
                                 len(err))
    text = _valset_result(rc, err, "tmv_validator_set_new")
    if text is not None:  # the change set's errors are panics here
        raise ValidatorSetPanic(text)
    return _py_valset(out, n_out.value, back, scratch, prop.value)


def validator_set_rotate(vals: ValidatorSet, steps: int = 1, times: int = 1, lib=None
                         ) -> Tuple[ValidatorSet, List[int]]:
    """`steps` successive IncrementProposerPriority(times) calls
    (types/validator_set.go:116-138) on a copy, as State.Update makes one per
    block with times = 1: (the set after the last call, the proposer's index
    after each call).  One call with times = k is not k calls with times = 1:
    the reference rescales and centres the priorities once per call."""
    L = _setup_valset(lib or _native.lib())
    k = _Keep()
    _c_validators(k, vals)
    a = k.refs[-1]
    n = len(vals.validators)
    props = (ctypes.c_int32 * max(1, steps))()
    err = ctypes.create_string_buffer(4096)
    rc = L.tmv_validator_set_rotate(ctypes.cast(a.ctypes.data, ctypes.POINTER(CValidator)), n, times, steps, props,
                                    err, len(err))
    text = _valset_result(rc, err, "tmv_validator_set_rotate")
    if text is not None:
        raise NativeError("tmv_validator_set_rotate: " + text)
    prios = a["proposer_priority"][:n].tolist()
    after = ValidatorSet([Validator(v.address, v.pub_key, v.voting_power, v.key_kind, p)
                          for v, p in zip(vals.validators, prios)], props[steps - 1] if steps else vals.proposer_index)
    return after, list(props[:steps])


def validator_set_hash_host(vals: ValidatorSet, lib=None) -> bytes:
    """ValidatorSet.Hash on the host (tmv_validator_set_hash_host): for the
    sets that hold secp256k1 keys, which the device call does not take."""
    L = _setup_valset(lib or _native.lib())
    k = _Keep()
    cv = _c_validators(k, vals)
    out = (ctypes.c_uint8 * 32)()
    rc = L.tmv_validator_set_hash_host(cv, len(vals.validators), ctypes.cast(out, _u8p))
    if rc < 0:
        raise NativeError(f"tmv_validator_set_hash_host failed ({rc})")
    return bytes(out)
