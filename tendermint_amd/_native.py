"""ctypes binding of libtmgpu.so (include/tmverify.h).

Loads the in-tree build (tendermint_amd/_build/libtmgpu.so).  Fails loudly
when it is missing — there is no CPU fallback on the product path.
"""
from __future__ import annotations

import ctypes
import os
import subprocess
import threading

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# TMV_LIB_PATH: an A/B build of the same library (tools/build_ab.sh) for
# measurement runs; the default is the in-tree build
LIB_PATH = os.environ.get("TMV_LIB_PATH") or os.path.join(_HERE, "_build", "libtmgpu.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "tmverify.h")
HEADER_PATHS = [HEADER_PATH, os.path.join(os.path.dirname(_HERE), "include", "tmhost.h")]

TMV_ALL_VALID = 1
TMV_NOT_ALL = 0
TMV_ERR_ARG = -1
TMV_ERR_NO_DEVICE = -2
TMV_ERR_NOMEM = -3
TMV_ERR_LAUNCH = -4
TMV_SR_ADDERR_PUBKEY = -1
TMV_SR_ADDERR_SIG = -2
TMV_KIND_ED25519 = 0
TMV_KIND_SR25519 = 1
TMV_FLAG_KEY_CACHE = 1
TMV_FLAG_BATCH_EQUATION = 2
TMV_FLAG_PER_ENTRY = 4
TMV_BATCHOPT_STATS = 1
TMV_BATCHOPT_SUBCHECK_ON = 2
TMV_BATCHOPT_SUBCHECK_OFF = 4
TMV_MERKLE_PREHASH = 1
TMV_MERKLE_LEAF_HASH_GIVEN = 2
TMV_MERKLE_LONG_LEAVES = 4
TMV_MERKLE_SHORT_LEAVES = 8
TMV_RESULTS_FIRST_LEAF = 1
TMV_SPAN_TAG, TMV_SPAN_PREHASH = 0x100, 0x200  # tmv_leaf_span.flags
TMV_KIND_MIXED = 2
TMV_KIND_SECP256K1 = 3  # include/tmhost.h: 33-byte compressed keys, verified signature by signature
TMV_VOTE_WITH_BLOCK = 0x80000000
# kVoteExtWaveMin (csrc/vote_ext.h): extension payloads from this length on are copied by the whole wave
VOTE_EXT_WAVE_MIN = 96

# tmv_vote (include/tmverify.h), 16 bytes
VOTE_DTYPE = np.dtype([("ts_seconds", "<i8"), ("ts_nanos", "<i4"), ("tmpl", "<u4")])

# Every symbol include/tmverify.h declares (checked by tests/test_boundary.py).
EXPORTS = [
    "tmv_open", "tmv_open_logical", "tmv_close", "tmv_num_devices", "tmv_last_error", "tmv_version",
    "tmv_ed25519_verify_batch", "tmv_ed25519_verify", "tmv_sr25519_verify_batch",
    "tmv_secp256k1_verify_batch", "tmv_secp256k1_verify", "tmv_secp256k1_verify_batch_ex",
    "tmv_secp256k1_key_cache_stats",
    "tmv_verify_mixed_batch", "tmv_ed25519_verify_batch_device", "tmv_verify_mixed_batch_device",
    "tmv_verify_batch_ex", "tmv_key_cache_stats", "tmv_point_cache_stats", "tmv_bucket_entry_stats", "tmv_group_fail_stats",
    "tmv_split_stats",
    "tmv_set_batch_options", "tmv_batch_stats",
    "tmv_subgroup_stats", "tmv_validator_set_hashes",
    "tmv_verify_mixed_batch_ex", "tmv_verify_batch_device_ex", "tmv_verify_batches_device",
    "tmv_verify_votes", "tmv_vote_sign_bytes_device", "tmv_verify_votes_and_extensions",
    "tmv_vote_extension_sign_bytes_device", "tmv_merkle_roots",
    "tmv_merkle_aunt_offsets", "tmv_merkle_proofs", "tmv_merkle_verify_proofs", "tmv_merkle_value_ops",
    "tmv_commit_hashes", "tmv_tx_results_hashes", "tmv_merkle_span_roots", "tmv_merkle_wire_roots",
    "tmv_kernel_timing", "tmv_kernel_timing_read", "tmv_metrics_read", "tmv_metrics_reset",
    # include/tmhost.h
    "tmv_validator_set_update", "tmv_validator_set_new", "tmv_validator_set_rotate", "tmv_validator_set_hash_host",
    "tmv_batch_new", "tmv_batch_add", "tmv_batch_len", "tmv_batch_verify", "tmv_batch_free",
    "tmv_vote_sign_bytes", "tmv_vote_template_encode", "tmv_verify_commit", "tmv_verify_commits",
    "tmv_header_hashes", "tmv_light_verify_many", "tmv_light_verify", "tmv_verify_vote_batch",
    "tmv_part_set_headers", "tmv_part_set_proofs", "tmv_parts_verify", "tmv_proofs_verify",
    "tmv_proof_ops_verify", "tmv_tx_proofs_validate",
    "tmv_commit_hash_many", "tmv_blocks_validate_basic",
    "tmv_blocks_validate_wire", "tmv_blocks_parse_wire", "tmv_block_views_block", "tmv_block_views_free",
    "tmv_light_blocks_validate_wire", "tmv_light_blocks_parse_wire", "tmv_light_block_views_header",
    "tmv_light_block_views_vals", "tmv_light_block_views_free",
    "tmv_results_hash_many", "tmv_consensus_params_hash", "tmv_block_results_verify", "tmv_consensus_params_verify",
    "tmv_vote_extension_sign_bytes", "tmv_vote_extension_template_encode", "tmv_verify_extended_votes",
]


class BatchRef(ctypes.Structure):
    """tmv_batch_ref (include/tmverify.h): one device-resident batch."""
    _fields_ = [("pk", ctypes.c_void_p), ("sig", ctypes.c_void_p), ("msg", ctypes.c_void_p),
                ("msg_off", ctypes.c_void_p), ("n", ctypes.c_uint32), ("msg_bytes", ctypes.c_uint32),
                ("status", ctypes.c_void_p)]


class Metrics(ctypes.Structure):
    """tmv_metrics (include/tmverify.h)."""
    _fields_ = [("calls", ctypes.c_uint64), ("signatures", ctypes.c_uint64), ("max_batch", ctypes.c_uint64),
                ("batch_eq_signatures", ctypes.c_uint64), ("host_signatures", ctypes.c_uint64),
                ("host_seconds", ctypes.c_double), ("h2d_bytes", ctypes.c_uint64), ("d2h_bytes", ctypes.c_uint64),
                ("groups", ctypes.c_uint64), ("groups_failed", ctypes.c_uint64),
                ("located_groups", ctypes.c_uint64), ("fallback_signatures", ctypes.c_uint64),
                ("key_cache_hits", ctypes.c_uint64), ("key_cache_misses", ctypes.c_uint64)]


class VoteTemplate(ctypes.Structure):
    """tmv_vote_template (include/tmverify.h): the shared segments of a commit's votes."""
    _fields_ = [("head", ctypes.c_void_p), ("head_len", ctypes.c_uint32), ("block", ctypes.c_void_p),
                ("block_len", ctypes.c_uint32), ("chain", ctypes.c_void_p), ("chain_len", ctypes.c_uint32)]


def vote_templates(segments):
    """[(head, block, chain) bytes] -> (ctypes array of VoteTemplate, keep-alive buffers)."""
    keep = []
    arr = (VoteTemplate * max(1, len(segments)))()
    for t, segs in enumerate(segments):
        ptrs = []
        for b in segs:
            buf = ctypes.create_string_buffer(bytes(b), max(1, len(b)))
            keep.append(buf)
            ptrs.append((ctypes.cast(buf, ctypes.c_void_p), len(b)))
        arr[t] = VoteTemplate(ptrs[0][0], ptrs[0][1], ptrs[1][0], ptrs[1][1], ptrs[2][0], ptrs[2][1])
    return arr, keep


class VoteExtTemplate(ctypes.Structure):
    """tmv_vote_ext_template (include/tmverify.h): the tail the extensions of one (chain, height, round) share."""
    _fields_ = [("tail", ctypes.c_void_p), ("tail_len", ctypes.c_uint32)]


def vote_ext_templates(tails):
    """[tail bytes] -> (ctypes array of VoteExtTemplate, keep-alive buffers)."""
    keep = []
    arr = (VoteExtTemplate * max(1, len(tails)))()
    for t, b in enumerate(tails):
        buf = ctypes.create_string_buffer(bytes(b), max(1, len(b)))
        keep.append(buf)
        arr[t] = VoteExtTemplate(ctypes.cast(buf, ctypes.c_void_p), len(b))
    return arr, keep


def _ext_args(ext_tmpl, ext_data, ext_off):
    """The (template index, payload bytes, payload offsets) arrays of the extension entries, contiguous."""
    ext_tmpl = np.ascontiguousarray(ext_tmpl, np.uint32)
    ext_off = np.ascontiguousarray(ext_off, np.uint32)
    ext_data = np.ascontiguousarray(ext_data, np.uint8)
    if len(ext_off) != len(ext_tmpl) + 1:
        raise ValueError("ext_off must hold one more entry than ext_tmpl")
    return ext_tmpl, (ext_data if len(ext_data) else np.zeros(1, np.uint8)), ext_off


class NativeError(RuntimeError):
    pass


def build() -> str:
    """Compile libtmgpu.so for gfx950 in-tree (hipcc cross-compiles without a GPU)."""
    subprocess.run(["make", "-s", "-C", os.path.join(_HERE, "csrc")], check=True)
    return LIB_PATH


_lib = None
_lib_lock = threading.Lock()


def lib() -> ctypes.CDLL:
    """Load libtmgpu.so; raises NativeError if it has not been built."""
    global _lib
    with _lib_lock:
        if _lib is not None:
            return _lib
        if not os.path.exists(LIB_PATH):
            raise NativeError(f"{LIB_PATH} missing: run tendermint_amd._native.build() "
                              "(there is no CPU fallback)")
        L = ctypes.CDLL(LIB_PATH)
        u8p = ctypes.POINTER(ctypes.c_uint8)
        i8p = ctypes.POINTER(ctypes.c_int8)
        u32p = ctypes.POINTER(ctypes.c_uint32)
        vp = ctypes.c_void_p
        L.tmv_open.restype = vp
        L.tmv_open.argtypes = [ctypes.c_uint32]
        L.tmv_open_logical.restype = vp
        L.tmv_open_logical.argtypes = [ctypes.c_uint32, ctypes.c_int]
        L.tmv_close.argtypes = [vp]
        L.tmv_num_devices.argtypes = [vp]
        L.tmv_last_error.restype = ctypes.c_char_p
        L.tmv_version.restype = ctypes.c_char_p
        L.tmv_ed25519_verify_batch.argtypes = [vp, u8p, u8p, u8p, u32p, ctypes.c_uint32, u8p]
        L.tmv_ed25519_verify.argtypes = [vp, u8p, u8p, ctypes.c_size_t, u8p, ctypes.c_size_t]
        L.tmv_secp256k1_verify_batch.argtypes = [vp, u8p, u8p, u8p, u32p, ctypes.c_uint32, u8p]
        L.tmv_secp256k1_verify.argtypes = [vp, u8p, ctypes.c_size_t, u8p, ctypes.c_size_t, u8p, ctypes.c_size_t]
        L.tmv_secp256k1_verify_batch_ex.argtypes = [vp, ctypes.c_uint32, u8p, u8p, u8p, u32p, ctypes.c_uint32, u8p]
        L.tmv_secp256k1_key_cache_stats.argtypes = [vp, ctypes.POINTER(ctypes.c_uint64),
                                                    ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint32),
                                                    ctypes.POINTER(ctypes.c_uint32)]
        L.tmv_sr25519_verify_batch.argtypes = [vp, u8p, u8p, u8p, u32p, ctypes.c_uint32, i8p]
        L.tmv_verify_mixed_batch.argtypes = [vp, u8p, u8p, u8p, u8p, u32p, ctypes.c_uint32, i8p]
        L.tmv_verify_batch_ex.argtypes = [vp, ctypes.c_uint8, ctypes.c_uint32, u8p, u8p, u8p, u32p, ctypes.c_uint32,
                                          i8p]
        L.tmv_key_cache_stats.argtypes = [vp, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64),
                                          ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint32)]
        L.tmv_point_cache_stats.argtypes = [vp, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64),
                                            ctypes.POINTER(ctypes.c_uint32)]
        L.tmv_bucket_entry_stats.argtypes = [vp, ctypes.POINTER(ctypes.c_uint64)]
        L.tmv_group_fail_stats.argtypes = [vp] + [ctypes.POINTER(ctypes.c_uint64)] * 3
        L.tmv_split_stats.argtypes = [vp] + [ctypes.POINTER(ctypes.c_uint64)] * 2
        L.tmv_set_batch_options.argtypes = [vp, ctypes.c_uint32, ctypes.c_uint32, u8p, ctypes.c_uint32]
        L.tmv_batch_stats.argtypes = [vp, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64)]
        L.tmv_kernel_timing.argtypes = [vp, ctypes.c_int]
        L.tmv_kernel_timing_read.argtypes = [vp, ctypes.c_char_p, ctypes.POINTER(ctypes.c_double),
                                             ctypes.POINTER(ctypes.c_uint64)]
        L.tmv_subgroup_stats.argtypes = [vp, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64)]
        L.tmv_validator_set_hashes.argtypes = [vp, u8p, u8p, ctypes.POINTER(ctypes.c_int64), u32p,
                                               ctypes.c_uint32, u8p]
        L.tmv_verify_mixed_batch_ex.argtypes = [vp, ctypes.c_uint32, u8p, u8p, u8p, u8p, u32p, ctypes.c_uint32, i8p]
        L.tmv_merkle_roots.argtypes = [vp, u8p, u32p, ctypes.c_uint32, u32p, ctypes.c_uint32, u8p]
        L.tmv_merkle_aunt_offsets.argtypes = [u32p, ctypes.c_uint32, u32p]
        L.tmv_commit_hashes.argtypes = [vp, u8p, u8p, u8p, ctypes.POINTER(ctypes.c_int64),
                                        ctypes.POINTER(ctypes.c_int32), u8p, u8p, u32p, ctypes.c_uint32, u8p]
        L.tmv_merkle_proofs.argtypes = [vp, ctypes.c_uint32, u8p, u32p, ctypes.c_uint32, u32p, ctypes.c_uint32, u8p,
                                        u8p, u32p, u8p]
        i64p = ctypes.POINTER(ctypes.c_int64)
        L.tmv_tx_results_hashes.argtypes = [vp, ctypes.c_uint32, u32p, i64p, i64p, u8p, u32p, u32p, ctypes.c_uint32,
                                            u8p, u32p, u8p]
        L.tmv_merkle_span_roots.argtypes = [vp, u8p, ctypes.c_uint32, u32p, ctypes.c_uint32, u32p, ctypes.c_uint32, u8p]
        L.tmv_merkle_wire_roots.argtypes = [vp, u8p, ctypes.c_uint32, u32p, ctypes.c_uint32, u32p, ctypes.c_uint32, u32p,
                                            ctypes.c_uint32, u8p]
        L.tmv_merkle_verify_proofs.argtypes = [vp, ctypes.c_uint32, ctypes.c_uint32, i64p, i64p, u8p, u8p, u32p, u8p,
                                               u8p, u32p, i8p, u8p, u8p, u8p]
        L.tmv_merkle_value_ops.argtypes = [vp, ctypes.c_uint32, ctypes.c_uint32, u8p, u32p, u32p, u8p, u32p, i64p, i64p,
                                           u8p, u8p, u32p, u8p, u8p, u8p, u8p, u8p, u8p, i8p,
                                           ctypes.POINTER(ctypes.c_int32)]
        L.tmv_verify_batch_device_ex.argtypes = [vp, ctypes.c_int, ctypes.c_uint8, ctypes.c_uint32, vp, vp, vp, vp,
                                                 vp, ctypes.c_uint32, vp, vp]
        L.tmv_verify_batches_device.argtypes = [vp, ctypes.c_int, ctypes.c_uint8, ctypes.c_uint32,
                                                ctypes.POINTER(BatchRef), ctypes.c_uint32, vp]
        L.tmv_verify_votes.argtypes = [vp, ctypes.c_uint8, ctypes.c_uint32, ctypes.POINTER(VoteTemplate),
                                       ctypes.c_uint32, vp, u8p, u8p, ctypes.c_uint32, i8p]
        L.tmv_vote_sign_bytes_device.restype = ctypes.c_int64
        L.tmv_vote_sign_bytes_device.argtypes = [vp, ctypes.POINTER(VoteTemplate), ctypes.c_uint32, vp,
                                                 ctypes.c_uint32, u8p, ctypes.c_size_t, u32p]
        L.tmv_verify_votes_and_extensions.argtypes = [vp, ctypes.c_uint8, ctypes.c_uint32,
                                                      ctypes.POINTER(VoteTemplate), ctypes.c_uint32, vp, ctypes.c_uint32,
                                                      ctypes.POINTER(VoteExtTemplate), ctypes.c_uint32, u32p, u8p, u32p,
                                                      ctypes.c_uint32, u8p, u8p, i8p]
        L.tmv_vote_extension_sign_bytes_device.restype = ctypes.c_int64
        L.tmv_vote_extension_sign_bytes_device.argtypes = [vp, ctypes.POINTER(VoteExtTemplate), ctypes.c_uint32, u32p,
                                                           u8p, u32p, ctypes.c_uint32, u8p, ctypes.c_size_t, u32p]
        L.tmv_ed25519_verify_batch_device.argtypes = [vp, ctypes.c_int, vp, vp, vp, vp, ctypes.c_uint32, vp, vp]
        L.tmv_verify_mixed_batch_device.argtypes = [vp, ctypes.c_int, vp, vp, vp, vp, vp, ctypes.c_uint32, vp, vp]
        L.tmv_metrics_read.argtypes = [vp, ctypes.POINTER(Metrics)]
        L.tmv_metrics_reset.argtypes = [vp]
        _lib = L
        return L


def merkle_lpw(leaves_per_wave: int) -> int:
    """TMV_MERKLE_LPW(l): the flag bits that fix the long-leaf kernel's leaves per wave."""
    return leaves_per_wave << 8


def merkle_aunt_offsets(tree_off: np.ndarray) -> np.ndarray:
    """tmv_merkle_aunt_offsets: prefix sums of every leaf's aunt count (no device work)."""
    tree_off = np.ascontiguousarray(tree_off, np.uint32)
    out = np.zeros(int(tree_off[-1]) + 1, np.uint32)
    rc = lib().tmv_merkle_aunt_offsets(_p(tree_off, ctypes.c_uint32), len(tree_off) - 1, _p(out, ctypes.c_uint32))
    if rc < 0:
        raise NativeError(f"tmv_merkle_aunt_offsets failed ({rc}): {last_error()}")
    return out


def last_error() -> str:
    return lib().tmv_last_error().decode(errors="replace")


def version() -> str:
    """tmv_version(): the library's version with its build id (source
    digest and git HEAD compiled in by csrc/Makefile)."""
    return lib().tmv_version().decode(errors="replace")


def build_info() -> dict:
    """The loaded library's build id against the sources of this tree:
    src_match says whether libtmgpu.so was compiled from them
    (csrc/src_digest.py computes the same digest the Makefile compiled in)."""
    import importlib.util
    v = version()
    fields = dict(kv.split("=", 1) for kv in v.split() if "=" in kv)
    spec = importlib.util.spec_from_file_location("tmv_src_digest", os.path.join(_HERE, "csrc", "src_digest.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    tree = mod.digest()
    return {"version": v, "src_digest_compiled": fields.get("src"), "src_digest_tree": tree,
            "src_match": fields.get("src") == tree, "git_head_compiled": fields.get("git"),
            "library": LIB_PATH}


def _p(a: np.ndarray, t=ctypes.c_uint8):
    return a.ctypes.data_as(ctypes.POINTER(t))


class Context:
    """A tmv_ctx on the devices in ``device_mask`` (0 = all visible)."""

    def __init__(self, device_mask: int = 0, logical: int = 1):
        """logical > 1: test aid (tmv_open_logical), every GPU opened as that
        many logical devices."""
        self._lib = lib()
        self._h = (self._lib.tmv_open(device_mask) if logical == 1
                   else self._lib.tmv_open_logical(device_mask, logical))
        if not self._h:
            raise NativeError("tmv_open failed: " + last_error())

    @property
    def handle(self):
        return self._h

    def close(self):
        if self._h:
            self._lib.tmv_close(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def num_devices(self) -> int:
        return self._lib.tmv_num_devices(self._h)

    @staticmethod
    def _check(rc: int, what: str) -> int:
        if rc < 0:
            raise NativeError(f"{what} failed ({rc}): {last_error()}")
        return rc

    def ed25519_verify_batch(self, pk: np.ndarray, sig: np.ndarray, msg: np.ndarray, off: np.ndarray):
        n = len(off) - 1
        out = np.zeros(max(n, 1), np.uint8)
        msg = msg if len(msg) else np.zeros(1, np.uint8)
        pk = pk if len(pk) else np.zeros(1, np.uint8)
        sig = sig if len(sig) else np.zeros(1, np.uint8)
        rc = self._check(self._lib.tmv_ed25519_verify_batch(self._h, _p(pk), _p(sig), _p(msg),
                                                            _p(off, ctypes.c_uint32), n, _p(out)),
                         "tmv_ed25519_verify_batch")
        return rc == TMV_ALL_VALID, out[:n]

    def ed25519_verify(self, pk: bytes, msg: bytes, sig: bytes) -> bool:
        a = np.frombuffer(pk, np.uint8).copy()
        m = np.frombuffer(msg + b"\0", np.uint8).copy()
        s = np.frombuffer(sig + b"\0", np.uint8).copy()
        rc = self._check(self._lib.tmv_ed25519_verify(self._h, _p(a), _p(m), len(msg), _p(s), len(sig)),
                         "tmv_ed25519_verify")
        return rc == 1

    def secp256k1_verify_batch(self, pk: np.ndarray, sig: np.ndarray, msg: np.ndarray, off: np.ndarray):
        """ECDSA over secp256k1, one verdict per entry; pk: n x 33 compressed keys, sig: n x 64 (r || s)."""
        n = len(off) - 1
        out = np.zeros(max(n, 1), np.uint8)
        msg = msg if len(msg) else np.zeros(1, np.uint8)
        pk = pk if len(pk) else np.zeros(1, np.uint8)
        sig = sig if len(sig) else np.zeros(1, np.uint8)
        rc = self._check(self._lib.tmv_secp256k1_verify_batch(self._h, _p(pk), _p(sig), _p(msg),
                                                              _p(off, ctypes.c_uint32), n, _p(out)),
                         "tmv_secp256k1_verify_batch")
        return rc == TMV_ALL_VALID, out[:n]

    def secp256k1_verify_batch_ex(self, pk: np.ndarray, sig: np.ndarray, msg: np.ndarray, off: np.ndarray,
                                  flags: int = TMV_FLAG_KEY_CACHE):
        """secp256k1_verify_batch with flags: TMV_FLAG_KEY_CACHE verifies against the keys' comb tables kept on
        the device (TMV_SECP_KEY_CACHE_CAPACITY keys); the verdicts are the same."""
        n = len(off) - 1
        out = np.zeros(max(n, 1), np.uint8)
        msg = msg if len(msg) else np.zeros(1, np.uint8)
        pk = pk if len(pk) else np.zeros(1, np.uint8)
        sig = sig if len(sig) else np.zeros(1, np.uint8)
        rc = self._check(self._lib.tmv_secp256k1_verify_batch_ex(self._h, flags, _p(pk), _p(sig), _p(msg),
                                                                 _p(off, ctypes.c_uint32), n, _p(out)),
                         "tmv_secp256k1_verify_batch_ex")
        return rc == TMV_ALL_VALID, out[:n]

    def secp256k1_key_cache_stats(self):
        h, m = ctypes.c_uint64(), ctypes.c_uint64()
        u, c = ctypes.c_uint32(), ctypes.c_uint32()
        self._check(self._lib.tmv_secp256k1_key_cache_stats(self._h, ctypes.byref(h), ctypes.byref(m),
                                                            ctypes.byref(u), ctypes.byref(c)),
                    "tmv_secp256k1_key_cache_stats")
        return {"hits": h.value, "misses": m.value, "used": u.value, "capacity": c.value}

    def secp256k1_verify(self, pk: bytes, msg: bytes, sig: bytes) -> bool:
        a = np.frombuffer(pk + b"\0", np.uint8).copy()
        m = np.frombuffer(msg + b"\0", np.uint8).copy()
        s = np.frombuffer(sig + b"\0", np.uint8).copy()
        rc = self._check(self._lib.tmv_secp256k1_verify(self._h, _p(a), len(pk), _p(m), len(msg), _p(s), len(sig)),
                         "tmv_secp256k1_verify")
        return rc == 1

    def sr25519_verify_batch(self, pk, sig, msg, off):
        n = len(off) - 1
        out = np.zeros(max(n, 1), np.int8)
        msg = msg if len(msg) else np.zeros(1, np.uint8)
        pk = pk if len(pk) else np.zeros(1, np.uint8)
        sig = sig if len(sig) else np.zeros(1, np.uint8)
        rc = self._check(self._lib.tmv_sr25519_verify_batch(self._h, _p(pk), _p(sig), _p(msg),
                                                            _p(off, ctypes.c_uint32), n,
                                                            _p(out, ctypes.c_int8)),
                         "tmv_sr25519_verify_batch")
        return rc == TMV_ALL_VALID, out[:n]

    def verify_mixed_batch(self, kind, pk, sig, msg, off):
        n = len(off) - 1
        out = np.zeros(max(n, 1), np.int8)
        msg = msg if len(msg) else np.zeros(1, np.uint8)
        kind = kind if len(kind) else np.zeros(1, np.uint8)
        pk = pk if len(pk) else np.zeros(1, np.uint8)
        sig = sig if len(sig) else np.zeros(1, np.uint8)
        rc = self._check(self._lib.tmv_verify_mixed_batch(self._h, _p(kind), _p(pk), _p(sig), _p(msg),
                                                          _p(off, ctypes.c_uint32), n, _p(out, ctypes.c_int8)),
                         "tmv_verify_mixed_batch")
        return rc == TMV_ALL_VALID, out[:n]

    def verify_batch_ex(self, key_kind: int, flags: int, pk, sig, msg, off):
        n = len(off) - 1
        out = np.zeros(max(n, 1), np.int8)
        msg = msg if len(msg) else np.zeros(1, np.uint8)
        pk = pk if len(pk) else np.zeros(1, np.uint8)
        sig = sig if len(sig) else np.zeros(1, np.uint8)
        rc = self._check(self._lib.tmv_verify_batch_ex(self._h, key_kind, flags, _p(pk), _p(sig), _p(msg),
                                                       _p(off, ctypes.c_uint32), n, _p(out, ctypes.c_int8)),
                         "tmv_verify_batch_ex")
        return rc == TMV_ALL_VALID, out[:n]

    def verify_votes(self, key_kind: int, flags: int, templates, votes, pk, sig):
        """tmv_verify_votes: templates = [(head, block, chain)], votes = VOTE_DTYPE array."""
        votes = np.ascontiguousarray(votes, VOTE_DTYPE)
        n = len(votes)
        arr, keep = vote_templates(templates)
        out = np.zeros(max(n, 1), np.int8)
        pk = pk if len(pk) else np.zeros(1, np.uint8)
        sig = sig if len(sig) else np.zeros(1, np.uint8)
        rc = self._check(self._lib.tmv_verify_votes(self._h, key_kind, flags, arr, len(templates),
                                                    votes.ctypes.data if n else None, _p(pk), _p(sig), n,
                                                    _p(out, ctypes.c_int8)), "tmv_verify_votes")
        del keep
        return rc == TMV_ALL_VALID, out[:n]

    def vote_sign_bytes_device(self, templates, votes):
        """The messages k_vote_signbytes writes for (templates, votes): (msg bytes, offsets)."""
        votes = np.ascontiguousarray(votes, VOTE_DTYPE)
        n = len(votes)
        arr, keep = vote_templates(templates)
        off = np.zeros(n + 1, np.uint32)
        vp = votes.ctypes.data if n else None
        total = self._check(self._lib.tmv_vote_sign_bytes_device(self._h, arr, len(templates), vp, n, None, 0,
                                                                 _p(off, ctypes.c_uint32)), "tmv_vote_sign_bytes_device")
        msg = np.zeros(max(total, 1), np.uint8)
        self._check(self._lib.tmv_vote_sign_bytes_device(self._h, arr, len(templates), vp, n, _p(msg), len(msg),
                                                         _p(off, ctypes.c_uint32)), "tmv_vote_sign_bytes_device")
        del keep
        return msg[:total].tobytes(), off

    def verify_votes_and_extensions(self, key_kind: int, flags: int, templates, votes, ext_tails, ext_tmpl, ext_data,
                                    ext_off, pk, sig):
        """tmv_verify_votes_and_extensions: the vote entries of verify_votes, then one extension entry per
        ext_tmpl[j] (index into ext_tails) with the payload ext_data[ext_off[j]:ext_off[j+1]]; pk / sig hold the
        vote entries' keys and signatures, then the extension entries'."""
        votes = np.ascontiguousarray(votes, VOTE_DTYPE)
        ext_tmpl, ext_data, ext_off = _ext_args(ext_tmpl, ext_data, ext_off)
        nv, ne = len(votes), len(ext_tmpl)
        arr, keep = vote_templates(templates)
        earr, ekeep = vote_ext_templates(ext_tails)
        out = np.zeros(max(nv + ne, 1), np.int8)
        pk = pk if len(pk) else np.zeros(1, np.uint8)
        sig = sig if len(sig) else np.zeros(1, np.uint8)
        rc = self._check(self._lib.tmv_verify_votes_and_extensions(
            self._h, key_kind, flags, arr, len(templates), votes.ctypes.data if nv else None, nv, earr,
            len(ext_tails), _p(ext_tmpl, ctypes.c_uint32), _p(ext_data), _p(ext_off, ctypes.c_uint32), ne, _p(pk),
            _p(sig), _p(out, ctypes.c_int8)), "tmv_verify_votes_and_extensions")
        del keep, ekeep
        return rc == TMV_ALL_VALID, out[:nv + ne]

    def vote_extension_sign_bytes_device(self, ext_tails, ext_tmpl, ext_data, ext_off):
        """The messages k_vote_ext_signbytes writes for the extension entries: (msg bytes, offsets)."""
        ext_tmpl, ext_data, ext_off = _ext_args(ext_tmpl, ext_data, ext_off)
        n = len(ext_tmpl)
        earr, ekeep = vote_ext_templates(ext_tails)
        off = np.zeros(n + 1, np.uint32)
        args = (self._h, earr, len(ext_tails), _p(ext_tmpl, ctypes.c_uint32), _p(ext_data),
                _p(ext_off, ctypes.c_uint32), n)
        total = self._check(self._lib.tmv_vote_extension_sign_bytes_device(*args, None, 0, _p(off, ctypes.c_uint32)),
                            "tmv_vote_extension_sign_bytes_device")
        msg = np.zeros(max(total, 1), np.uint8)
        self._check(self._lib.tmv_vote_extension_sign_bytes_device(*args, _p(msg), len(msg),
                                                                   _p(off, ctypes.c_uint32)),
                    "tmv_vote_extension_sign_bytes_device")
        del ekeep
        return msg[:total].tobytes(), off

    def verify_mixed_batch_ex(self, flags: int, kind, pk, sig, msg, off):
        n = len(off) - 1
        out = np.zeros(max(n, 1), np.int8)
        msg = msg if len(msg) else np.zeros(1, np.uint8)
        kind = kind if len(kind) else np.zeros(1, np.uint8)
        pk = pk if len(pk) else np.zeros(1, np.uint8)
        sig = sig if len(sig) else np.zeros(1, np.uint8)
        rc = self._check(self._lib.tmv_verify_mixed_batch_ex(self._h, flags, _p(kind), _p(pk), _p(sig), _p(msg),
                                                             _p(off, ctypes.c_uint32), n, _p(out, ctypes.c_int8)),
                         "tmv_verify_mixed_batch_ex")
        return rc == TMV_ALL_VALID, out[:n]

    def kernel_timing(self, enable: bool) -> None:
        """Bracket later launches of the timed kernels with HIP timing events
        on their streams (tmv_kernel_timing)."""
        self._check(self._lib.tmv_kernel_timing(self._h, 1 if enable else 0), "tmv_kernel_timing")

    def kernel_timing_read(self, kernel: str) -> tuple[float, int]:
        """(summed duration in ms, launches) of `kernel` since the last read
        (tmv_kernel_timing_read; waits for the recorded launches)."""
        ms, cnt = ctypes.c_double(0), ctypes.c_uint64(0)
        self._check(self._lib.tmv_kernel_timing_read(self._h, kernel.encode(), ctypes.byref(ms), ctypes.byref(cnt)),
                    "tmv_kernel_timing_read")
        return ms.value, cnt.value

    def set_batch_options(self, group_log2: int = 0, window_bits: int = 0, seed: bytes | None = None,
                          stats: bool = False, subcheck: bool | None = None) -> None:
        """Batch-equation options (tmv_set_batch_options): group size 2^group_log2,
        window bits, a fixed ChaCha20 key (tests only; None = fresh randomness
        per call), group-verdict counting and sub-group bisection (None =
        the default policy)."""
        sp = None
        if seed is not None:
            if len(seed) != 32:
                raise ValueError("seed must be 32 bytes")
            self._seed_buf = np.frombuffer(seed, np.uint8).copy()
            sp = _p(self._seed_buf)
        opt = (TMV_BATCHOPT_STATS if stats else 0) | \
            ({True: TMV_BATCHOPT_SUBCHECK_ON, False: TMV_BATCHOPT_SUBCHECK_OFF}.get(subcheck, 0))
        self._check(self._lib.tmv_set_batch_options(self._h, group_log2, window_bits, sp, opt),
                    "tmv_set_batch_options")

    def validator_set_hashes(self, pk: np.ndarray, kind: np.ndarray, power: np.ndarray,
                             set_off: np.ndarray) -> np.ndarray:
        """ValidatorSet.Hash of each set (tmv_validator_set_hashes): (n_sets, 32) uint8."""
        n_sets = len(set_off) - 1
        out = np.zeros((max(n_sets, 1), 32), np.uint8)
        pk = np.ascontiguousarray(pk, np.uint8) if len(pk) else np.zeros(32, np.uint8)
        kind = np.ascontiguousarray(kind, np.uint8) if len(kind) else np.zeros(1, np.uint8)
        power = np.ascontiguousarray(power, np.int64) if len(power) else np.zeros(1, np.int64)
        set_off = np.ascontiguousarray(set_off, np.uint32)
        self._check(self._lib.tmv_validator_set_hashes(self._h, _p(pk), _p(kind), _p(power, ctypes.c_int64),
                                                       _p(set_off, ctypes.c_uint32), n_sets, _p(out)),
                    "tmv_validator_set_hashes")
        return out[:n_sets]

    def commit_hashes(self, flag: np.ndarray, addr_len: np.ndarray, addr: np.ndarray, ts_seconds: np.ndarray,
                      ts_nanos: np.ndarray, sig_len: np.ndarray, sig: np.ndarray,
                      commit_off: np.ndarray) -> np.ndarray:
        """Commit.Hash of each commit (tmv_commit_hashes): (n_commits, 32) uint8.
        One entry per CommitSig: flag, addr_len (0 or 20), addr (n, 20),
        ts_seconds, ts_nanos, sig_len (0..64), sig (n, 64); commit c holds the
        signatures [commit_off[c], commit_off[c+1])."""
        n_commits = len(commit_off) - 1
        out = np.zeros((max(n_commits, 1), 32), np.uint8)

        def col(a, dtype, width=1):
            a = np.ascontiguousarray(a, dtype)
            return a if a.size else np.zeros(width, dtype)
        flag, addr_len, sig_len = col(flag, np.uint8), col(addr_len, np.uint8), col(sig_len, np.uint8)
        addr, sig = col(addr, np.uint8, 20), col(sig, np.uint8, 64)
        ts_seconds, ts_nanos = col(ts_seconds, np.int64), col(ts_nanos, np.int32)
        commit_off = np.ascontiguousarray(commit_off, np.uint32)
        self._check(self._lib.tmv_commit_hashes(self._h, _p(flag), _p(addr_len), _p(addr),
                                                _p(ts_seconds, ctypes.c_int64), _p(ts_nanos, ctypes.c_int32),
                                                _p(sig_len), _p(sig), _p(commit_off, ctypes.c_uint32), n_commits,
                                                _p(out)), "tmv_commit_hashes")
        return out[:n_commits]

    def tx_results_hashes(self, code: np.ndarray, gas_wanted: np.ndarray, gas_used: np.ndarray, data,
                          data_off: np.ndarray, tree_off: np.ndarray, first=None, first_off=None,
                          flags=None) -> np.ndarray:
        """The merkle root over abci.MarshalTxResults of each tree
        (tmv_tx_results_hashes): (n_trees, 32) uint8.  One entry per result:
        code, gas_wanted, gas_used and the data data[data_off[i]:data_off[i+1]];
        tree t holds the results [tree_off[t], tree_off[t+1]).  With `first`
        (uint8) and `first_off` (n_trees + 1) tree t gets the leading leaf
        first[first_off[t]:first_off[t+1]] (TMV_RESULTS_FIRST_LEAF; `flags`
        overrides).  data: uint8 array, or None for a null pointer."""
        n_trees = len(tree_off) - 1
        out = np.zeros((max(n_trees, 1), 32), np.uint8)

        def col(a, dtype):
            a = np.ascontiguousarray(a, dtype)
            return a if a.size else np.zeros(1, dtype)
        code, gas_wanted, gas_used = col(code, np.uint32), col(gas_wanted, np.int64), col(gas_used, np.int64)
        data_off = np.ascontiguousarray(data_off, np.uint32)
        tree_off = np.ascontiguousarray(tree_off, np.uint32)
        dp = None if data is None else _p(col(data, np.uint8))
        fp = None if first is None else _p(col(first, np.uint8))
        fo = None if first_off is None else np.ascontiguousarray(first_off, np.uint32)
        if flags is None:
            flags = TMV_RESULTS_FIRST_LEAF if first_off is not None else 0
        self._check(self._lib.tmv_tx_results_hashes(self._h, flags, _p(code, ctypes.c_uint32),
                                                    _p(gas_wanted, ctypes.c_int64), _p(gas_used, ctypes.c_int64), dp,
                                                    _p(data_off, ctypes.c_uint32), _p(tree_off, ctypes.c_uint32),
                                                    n_trees, fp, None if fo is None else _p(fo, ctypes.c_uint32),
                                                    _p(out)), "tmv_tx_results_hashes")
        return out[:n_trees]

    def merkle_span_roots(self, data, spans, tree_off: np.ndarray, data_len=None, n_leaves=None) -> np.ndarray:
        """Merkle roots over spans of one buffer (tmv_merkle_span_roots):
        (n_trees, 32) uint8.  data: uint8 array or bytes, or None for a null
        pointer; spans: (n, 3) uint32 rows of (pos, len, flags) with
        TMV_SPAN_TAG | tag byte or TMV_SPAN_PREHASH, or None for a null pointer;
        tree t holds the leaves [tree_off[t], tree_off[t+1]).  data_len /
        n_leaves override the arrays' sizes."""
        n_trees = len(tree_off) - 1
        out = np.zeros((max(n_trees, 1), 32), np.uint8)
        tree_off = np.ascontiguousarray(tree_off, np.uint32)
        if data is not None:
            data = np.frombuffer(data, np.uint8) if isinstance(data, (bytes, bytearray)) else np.ascontiguousarray(
                data, np.uint8)
            if data_len is None:
                data_len = len(data)
            data = data if data.size else np.zeros(1, np.uint8)
        if spans is not None:
            spans = np.ascontiguousarray(spans, np.uint32).reshape(-1, 3)
            if n_leaves is None:
                n_leaves = len(spans)
            spans = spans if spans.size else np.zeros((1, 3), np.uint32)
        self._check(self._lib.tmv_merkle_span_roots(self._h, None if data is None else _p(data), data_len or 0,
                                                    None if spans is None else _p(spans, ctypes.c_uint32),
                                                    n_leaves or 0, _p(tree_off, ctypes.c_uint32), n_trees, _p(out)),
                    "tmv_merkle_span_roots")
        return out[:n_trees]

    def merkle_wire_roots(self, data, spans, val_spans, tree_off: np.ndarray, data_len=None, n_leaves=None,
                          n_val_leaves=None) -> np.ndarray:
        """Merkle roots over spans and validator spans of one buffer
        (tmv_merkle_wire_roots): (n_trees, 32) uint8.  data and spans as for
        merkle_span_roots; val_spans: (n, 3) uint32 rows of (pos, len,
        power_at), or None for a null pointer; tree t holds the leaves
        [tree_off[t], tree_off[t+1]) of spans followed by val_spans.
        data_len / n_leaves / n_val_leaves override the arrays' sizes."""
        n_trees = len(tree_off) - 1
        out = np.zeros((max(n_trees, 1), 32), np.uint8)
        tree_off = np.ascontiguousarray(tree_off, np.uint32)
        if data is not None:
            data = np.frombuffer(data, np.uint8) if isinstance(data, (bytes, bytearray)) else np.ascontiguousarray(
                data, np.uint8)
            if data_len is None:
                data_len = len(data)
            data = data if data.size else np.zeros(1, np.uint8)

        def table(t, n):
            if t is None:
                return None, n or 0
            t = np.ascontiguousarray(t, np.uint32).reshape(-1, 3)
            n = len(t) if n is None else n
            return (t if t.size else np.zeros((1, 3), np.uint32)), n
        spans, n_leaves = table(spans, n_leaves)
        val_spans, n_val_leaves = table(val_spans, n_val_leaves)
        self._check(self._lib.tmv_merkle_wire_roots(self._h, None if data is None else _p(data), data_len or 0,
                                                    None if spans is None else _p(spans, ctypes.c_uint32), n_leaves,
                                                    None if val_spans is None else _p(val_spans, ctypes.c_uint32),
                                                    n_val_leaves, _p(tree_off, ctypes.c_uint32), n_trees, _p(out)),
                    "tmv_merkle_wire_roots")
        return out[:n_trees]

    def merkle_roots(self, data, leaf_off: np.ndarray, tree_off: np.ndarray) -> np.ndarray:
        """merkle.HashFromByteSlices of each tree (tmv_merkle_roots): (n_trees, 32) uint8.
        data: uint8 array, or None for a null pointer."""
        n_trees, n_leaves = len(tree_off) - 1, len(leaf_off) - 1
        out = np.zeros((max(n_trees, 1), 32), np.uint8)
        leaf_off = np.ascontiguousarray(leaf_off, np.uint32)
        tree_off = np.ascontiguousarray(tree_off, np.uint32)
        dp = None if data is None else _p(np.ascontiguousarray(data, np.uint8) if len(data) else np.zeros(1, np.uint8))
        self._check(self._lib.tmv_merkle_roots(self._h, dp, _p(leaf_off, ctypes.c_uint32), n_leaves,
                                               _p(tree_off, ctypes.c_uint32), n_trees, _p(out)), "tmv_merkle_roots")
        return out[:n_trees]

    def merkle_proofs(self, data, leaf_off: np.ndarray, tree_off: np.ndarray, flags: int = 0, aunts: bool = True):
        """merkle.ProofsFromByteSlices of each tree (tmv_merkle_proofs):
        (roots (n_trees, 32), leaf hashes (n_leaves, 32), aunt_off (n_leaves + 1)
        or None, aunts (n_aunts, 32) or None).  Leaf i's aunts, leaf sibling
        first, are aunts[aunt_off[i]:aunt_off[i+1]]; its proof has total = its
        tree's leaf count and index = i - tree_off[t].  data: uint8 array, or
        None for a null pointer."""
        n_trees, n_leaves = len(tree_off) - 1, len(leaf_off) - 1
        leaf_off = np.ascontiguousarray(leaf_off, np.uint32)
        tree_off = np.ascontiguousarray(tree_off, np.uint32)
        dp = None if data is None else _p(np.ascontiguousarray(data, np.uint8) if len(data) else np.zeros(1, np.uint8))
        roots = np.zeros((max(n_trees, 1), 32), np.uint8)
        leaves = np.zeros((max(n_leaves, 1), 32), np.uint8)
        aoff = av = None
        if aunts:
            aoff = merkle_aunt_offsets(tree_off)
            av = np.zeros((max(int(aoff[-1]), 1), 32), np.uint8)
        self._check(self._lib.tmv_merkle_proofs(self._h, flags, dp, _p(leaf_off, ctypes.c_uint32), n_leaves,
                                                _p(tree_off, ctypes.c_uint32), n_trees, _p(roots), _p(leaves),
                                                _p(aoff, ctypes.c_uint32) if aunts else None,
                                                _p(av) if aunts else None), "tmv_merkle_proofs")
        return roots[:n_trees], leaves[:n_leaves], aoff, (av[:int(aoff[-1])] if aunts else None)

    def merkle_verify_proofs(self, total, index, leaf_hash, aunts, aunt_off, root, data=None, leaf_off=None,
                             flags: int = 0):
        """Proof.Verify of n proofs (tmv_merkle_verify_proofs): (all ok,
        status (n,) int8, computed leaf hashes (n, 32), computed roots (n, 32),
        root-is-nil flags (n,)).  Without data / leaf_off the leaf hashes are
        taken as given (TMV_MERKLE_LEAF_HASH_GIVEN)."""
        n = len(total)
        total = np.ascontiguousarray(total, np.int64) if n else np.zeros(1, np.int64)
        index = np.ascontiguousarray(index, np.int64) if n else np.zeros(1, np.int64)
        leaf_hash = np.ascontiguousarray(leaf_hash, np.uint8) if n else np.zeros(32, np.uint8)
        root = np.ascontiguousarray(root, np.uint8) if n else np.zeros(32, np.uint8)
        aunt_off = np.ascontiguousarray(aunt_off, np.uint32)
        aunts = np.ascontiguousarray(aunts, np.uint8) if len(aunts) else np.zeros(32, np.uint8)
        if leaf_off is None:
            flags |= TMV_MERKLE_LEAF_HASH_GIVEN
            dp = lp = None
        else:
            leaf_off = np.ascontiguousarray(leaf_off, np.uint32)
            lp = _p(leaf_off, ctypes.c_uint32)
            dp = None if data is None else _p(np.ascontiguousarray(data, np.uint8) if len(data)
                                              else np.zeros(1, np.uint8))
        status = np.zeros(max(n, 1), np.int8)
        lcalc = np.zeros((max(n, 1), 32), np.uint8)
        rcalc = np.zeros((max(n, 1), 32), np.uint8)
        nil = np.zeros(max(n, 1), np.uint8)
        rc = self._check(self._lib.tmv_merkle_verify_proofs(
            self._h, flags, n, _p(total, ctypes.c_int64), _p(index, ctypes.c_int64), _p(leaf_hash), _p(aunts),
            _p(aunt_off, ctypes.c_uint32), _p(root), dp, lp, _p(status, ctypes.c_int8), _p(lcalc), _p(rcalc),
            _p(nil)), "tmv_merkle_verify_proofs")
        return rc == 0, status[:n], lcalc[:n], rcalc[:n], nil[:n]

    def merkle_value_ops(self, value, value_off, op_off, key, key_off, total, index, leaf_hash, aunts, aunt_off, root,
                         flags: int = 0, skip=()):
        """ValueOp.Run chained per item as ProofOperators.Verify chains it (tmv_merkle_value_ops):
        (all ok, dict of value_digest (n_items, 32), kv_hash_calc (n_ops, 32), leaf_ok (n_ops,),
        root_calc (n_ops, 32), root_nil (n_ops,), status (n_items,) int8, fail_op (n_items,) int32).
        value / key / aunts: uint8 arrays, or None for a null pointer; skip: names of outputs to pass
        as NULL (they come back as None)."""
        value_off = np.ascontiguousarray(value_off, np.uint32)
        op_off = np.ascontiguousarray(op_off, np.uint32)
        key_off = np.ascontiguousarray(key_off, np.uint32)
        aunt_off = np.ascontiguousarray(aunt_off, np.uint32)
        n_items, n_ops = len(op_off) - 1, len(key_off) - 1

        def data(a, width=1):
            if a is None:
                return None
            a = np.ascontiguousarray(a, np.uint8)
            return a if a.size else np.zeros(width, np.uint8)

        value, key, aunts = data(value), data(key), data(aunts, 32)
        leaf_hash, root = data(leaf_hash, 32), data(root, 32)
        total = np.ascontiguousarray(total, np.int64) if n_ops else np.zeros(1, np.int64)
        index = np.ascontiguousarray(index, np.int64) if n_ops else np.zeros(1, np.int64)
        out = {"value_digest": np.zeros((max(n_items, 1), 32), np.uint8),
               "kv_hash_calc": np.zeros((max(n_ops, 1), 32), np.uint8),
               "leaf_ok": np.zeros(max(n_ops, 1), np.uint8),
               "root_calc": np.zeros((max(n_ops, 1), 32), np.uint8),
               "root_nil": np.zeros(max(n_ops, 1), np.uint8),
               "status": np.zeros(max(n_items, 1), np.int8),
               "fail_op": np.zeros(max(n_items, 1), np.int32)}
        types = {"status": ctypes.c_int8, "fail_op": ctypes.c_int32}
        ptr = {k: (None if k in skip else _p(v, types.get(k, ctypes.c_uint8))) for k, v in out.items()}

        def opt(a):
            return None if a is None else _p(a)

        rc = self._check(self._lib.tmv_merkle_value_ops(
            self._h, flags, n_items, opt(value), _p(value_off, ctypes.c_uint32), _p(op_off, ctypes.c_uint32), opt(key),
            _p(key_off, ctypes.c_uint32), _p(total, ctypes.c_int64), _p(index, ctypes.c_int64), opt(leaf_hash),
            opt(aunts), _p(aunt_off, ctypes.c_uint32), opt(root), ptr["value_digest"], ptr["kv_hash_calc"],
            ptr["leaf_ok"], ptr["root_calc"], ptr["root_nil"], ptr["status"], ptr["fail_op"]),
            "tmv_merkle_value_ops")
        size = {"value_digest": n_items, "status": n_items, "fail_op": n_items}
        return rc == 0, {k: (None if k in skip else v[:size.get(k, n_ops)]) for k, v in out.items()}

    def batch_stats(self):
        g, f = ctypes.c_uint64(), ctypes.c_uint64()
        self._check(self._lib.tmv_batch_stats(self._h, ctypes.byref(g), ctypes.byref(f)), "tmv_batch_stats")
        sg, sf = ctypes.c_uint64(), ctypes.c_uint64()
        self._check(self._lib.tmv_subgroup_stats(self._h, ctypes.byref(sg), ctypes.byref(sf)), "tmv_subgroup_stats")
        return {"groups": g.value, "failed": f.value, "subgroups": sg.value, "sub_failed": sf.value}

    def verify_batch_device_ex(self, device: int, key_kind: int, flags: int, d_kind: int, d_pk: int, d_sig: int,
                               d_msg: int, d_off: int, n: int, d_status: int, stream: int = 0) -> None:
        self._check(self._lib.tmv_verify_batch_device_ex(self._h, device, key_kind, flags, d_kind or None, d_pk,
                                                         d_sig, d_msg, d_off, n, d_status, stream or None),
                    "tmv_verify_batch_device_ex")

    def verify_batches_device(self, device: int, key_kind: int, flags: int, refs, stream: int = 0) -> None:
        """refs: sequence of BatchRef (device pointers)."""
        arr = (BatchRef * len(refs))(*refs)
        self._check(self._lib.tmv_verify_batches_device(self._h, device, key_kind, flags, arr, len(refs),
                                                        stream or None), "tmv_verify_batches_device")

    def key_cache_stats(self):
        h, m = ctypes.c_uint64(), ctypes.c_uint64()
        u, c = ctypes.c_uint32(), ctypes.c_uint32()
        self._check(self._lib.tmv_key_cache_stats(self._h, ctypes.byref(h), ctypes.byref(m), ctypes.byref(u),
                                                  ctypes.byref(c)), "tmv_key_cache_stats")
        return {"hits": h.value, "misses": m.value, "used": u.value, "capacity": c.value}

    def point_cache_stats(self):
        """Hits, misses and capacity of the devices' point caches (read from the devices now)."""
        h, m = ctypes.c_uint64(), ctypes.c_uint64()
        c = ctypes.c_uint32()
        self._check(self._lib.tmv_point_cache_stats(self._h, ctypes.byref(h), ctypes.byref(m), ctypes.byref(c)),
                    "tmv_point_cache_stats")
        return {"hits": h.value, "misses": m.value, "slots": c.value}

    def bucket_entry_stats(self) -> int:
        """Bucket entries sorted by the batch equation since stats were switched on (read from the devices now)."""
        v = ctypes.c_uint64()
        self._check(self._lib.tmv_bucket_entry_stats(self._h, ctypes.byref(v)), "tmv_bucket_entry_stats")
        return v.value

    def group_fail_stats(self) -> dict:
        """Failing groups, located groups and entries left one by one of the stats launches (read from the devices now)."""
        f, l, e = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
        self._check(self._lib.tmv_group_fail_stats(self._h, ctypes.byref(f), ctypes.byref(l), ctypes.byref(e)),
                    "tmv_group_fail_stats")
        return {"failed": f.value, "located": l.value, "fallback_entries": e.value}

    def split_stats(self) -> dict:
        """Split groups and high points computed of the stats launches (read from the devices now)."""
        g, h = ctypes.c_uint64(), ctypes.c_uint64()
        self._check(self._lib.tmv_split_stats(self._h, ctypes.byref(g), ctypes.byref(h)), "tmv_split_stats")
        return {"groups_split": g.value, "high_points": h.value}

    def metrics(self) -> dict:
        """tmv_metrics: cumulative counters (plus verifies_per_s_host, the
        end-to-end rate of the host-buffer calls)."""
        m = Metrics()
        self._check(self._lib.tmv_metrics_read(self._h, ctypes.byref(m)), "tmv_metrics_read")
        d = {k: getattr(m, k) for k, _ in Metrics._fields_}
        d["verifies_per_s_host"] = d["host_signatures"] / d["host_seconds"] if d["host_seconds"] else 0.0
        return d

    def metrics_reset(self) -> None:
        self._check(self._lib.tmv_metrics_reset(self._h), "tmv_metrics_reset")

    def ed25519_verify_batch_device(self, device: int, d_pk: int, d_sig: int, d_msg: int, d_off: int, n: int,
                                    d_valid: int, stream: int = 0) -> None:
        self._check(self._lib.tmv_ed25519_verify_batch_device(self._h, device, d_pk, d_sig, d_msg, d_off, n,
                                                              d_valid, stream or None),
                    "tmv_ed25519_verify_batch_device")

    def verify_mixed_batch_device(self, device: int, d_kind: int, d_pk: int, d_sig: int, d_msg: int, d_off: int,
                                  n: int, d_status: int, stream: int = 0) -> None:
        self._check(self._lib.tmv_verify_mixed_batch_device(self._h, device, d_kind, d_pk, d_sig, d_msg, d_off, n,
                                                            d_status, stream or None),
                    "tmv_verify_mixed_batch_device")


_default_ctx = None
_ctx_lock = threading.Lock()


def default_context() -> Context:
    """Process-wide context on all visible GPUs (like voi's global verifier)."""
    global _default_ctx
    with _ctx_lock:
        if _default_ctx is None:
            _default_ctx = Context(0)
        return _default_ctx
