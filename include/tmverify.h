/*
 * tmverify.h — C-ABI of the MI355X signature-verification engine
 * (libtmgpu.so).  Plain pointers and sizes only; no torch or HIP types.
 *
 * This is the L0 replacement behind Tendermint's crypto.BatchVerifier
 * (crypto/crypto.go:66-76).  Each entry point names the reference interface
 * it replaces; INTEGRATION.md shows the cgo binding a maintainer adds to
 * crypto/ed25519, crypto/sr25519 and crypto/batch.
 *
 * Packed batch layout (shared by every batch entry point):
 *   pk      n x 32 bytes, entry i at pk + 32*i
 *   sig     n x 64 bytes, entry i at sig + 64*i  (R || S)
 *   msg     concatenated messages
 *   msg_off n+1 offsets into msg; message i = msg[msg_off[i] .. msg_off[i+1])
 *
 * Return codes of the batch entry points:
 *   TMV_ALL_VALID (1)   n > 0 and every entry verified
 *   TMV_NOT_ALL   (0)   some entry failed, or n == 0 (voi: an empty batch
 *                       verifies false)
 *   < 0                 infrastructure error (no device, allocation, launch,
 *                       TMV_ERR_TIMEOUT);
 *                       the validity vector is then unspecified and the
 *                       caller must not treat any entry as verified.
 */
#ifndef TMVERIFY_H
#define TMVERIFY_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TMV_ALL_VALID 1
#define TMV_NOT_ALL 0
#define TMV_ERR_ARG (-1)
#define TMV_ERR_NO_DEVICE (-2)
#define TMV_ERR_NOMEM (-3)
#define TMV_ERR_LAUNCH (-4)
/* A device wait exceeded $TMV_DEVICE_TIMEOUT_MS (default 60000; 0 = wait
 * forever).  The context's device work is then in an unknown state: the
 * context refuses further work (every call returns TMV_ERR_TIMEOUT); the
 * caller verifies on the CPU and may tmv_close / tmv_open a new context.
 * Pages of the caller's input buffers (pk, sig, msg, kind) that a streamed
 * call had registered for direct DMA stay page-locked after a failed call: the
 * device may still read them, so they are never unregistered under it (and
 * the library keeps no record that could unregister them once reused). */
#define TMV_ERR_TIMEOUT (-5)
/* The OS random source (getrandom) failed while drawing a batch equation's
 * weights (the reference's rand.Reader error, crypto/ed25519/ed25519.go:232);
 * nothing was launched.  tmv_last_error() names the errno. */
#define TMV_ERR_RANDOM (-6)

/* Per-entry sr25519 status (tmv_sr25519_verify_batch, tmv_verify_mixed_batch):
 *   1 valid, 0 invalid, TMV_SR_ADDERR_* = BatchVerifier.Add would have
 *   returned an error (crypto/sr25519/batch.go:30-37). */
#define TMV_SR_ADDERR_PUBKEY (-1)
#define TMV_SR_ADDERR_SIG (-2)

/* Key kinds for tmv_verify_mixed_batch (crypto/batch/batch.go:11-21). */
#define TMV_KIND_ED25519 0
#define TMV_KIND_SR25519 1

typedef struct tmv_ctx tmv_ctx;

/* Open a context on the GPUs selected by device_mask (bit i = HIP device i;
 * 0 = all visible devices).  Builds the per-device base-point tables.
 * Returns NULL on failure (tmv_last_error() says why). */
tmv_ctx *tmv_open(uint32_t device_mask);
/* TEST AID, not for deployments: as tmv_open, but each selected GPU joins the
 * context as `logical` devices (1..8: own streams, lanes, workspaces, key
 * cache), so the multi-device shard / harvest path runs on a one-GPU box.
 * tmv_num_devices then counts logical devices, while the device-pointer entry
 * points still name a GPU by its HIP id (its first logical device).
 * Announces itself on stderr when logical > 1. */
tmv_ctx *tmv_open_logical(uint32_t device_mask, int logical);
void tmv_close(tmv_ctx *ctx);
int tmv_num_devices(const tmv_ctx *ctx);
const char *tmv_last_error(void);
/* "tmverify-mi355x <ver> (gfx950) src=<digest> git=<head>": the source digest
   (tendermint_amd/csrc/src_digest.py over the sources this library is built
   from) and the git HEAD compiled in by the Makefile. */
const char *tmv_version(void);

/* ed25519 batch verification with ZIP-215 semantics.
 * Replaces: crypto/ed25519/ed25519.go:231-233 BatchVerifier.Verify (after the
 * Adds of :209-229 have been collected into the packed arrays; the Go-side
 * Add keeps its type/length checks and error strings).
 * Multi-device contexts shard the batch by contiguous index ranges.
 * valid_out[i] = 1/0 in Add order. */
int tmv_ed25519_verify_batch(tmv_ctx *ctx, const uint8_t *pk, const uint8_t *sig, const uint8_t *msg,
                             const uint32_t *msg_off, uint32_t n, uint8_t *valid_out);

/* Single ed25519 verification.
 * Replaces: crypto/ed25519/ed25519.go:173-180 PubKey.VerifySignature
 * (returns 0 when sig_len != 64, as the reference does).  Returns 1/0 or <0. */
int tmv_ed25519_verify(tmv_ctx *ctx, const uint8_t *pk, const uint8_t *msg, size_t msg_len,
                       const uint8_t *sig, size_t sig_len);

/* secp256k1 ECDSA batch verification, one verdict per entry.
 * Replaces: crypto/secp256k1/secp256k1.go:206-226 PubKey.VerifySignature per
 * entry (btcec ParsePubKey + Go's ecdsa.Verify over SHA-256(msg), lower-S
 * signatures only).  Keys are the 33-byte compressed form, entry i at
 * pk + 33*i -- the only size a validator set can hold (crypto/encoding/
 * codec.go:49-78); sig is r || s, 64 bytes per entry.  valid_out[i] = 1/0: a
 * key that does not parse, r or s out of range and an upper-S signature are
 * 0, never an error.  Runs on the context's first device.  TMV_ERR_ARG for
 * null pointers, msg_off[0] != 0, decreasing offsets, n > 2^26 or more than
 * 2^30 message bytes. */
int tmv_secp256k1_verify_batch(tmv_ctx *ctx, const uint8_t *pk, const uint8_t *sig, const uint8_t *msg,
                               const uint32_t *msg_off, uint32_t n, uint8_t *valid_out);

/* tmv_secp256k1_verify_batch with options.  flags: 0 (the call above) or
 *   TMV_FLAG_KEY_CACHE  keep the keys' comb tables on the device: an LRU of
 *   TMV_SECP_KEY_CACHE_CAPACITY keys (default 4,096; 0 = off) on the
 *   context's first device, apart from the ed25519/sr25519 cache.  A cached
 *   key is the 960 affine multiples d 16^j Q (j < 64, 1 <= d <= 15), 61,440
 *   bytes, so u1 G + u2 Q is 128 additions and no doublings; the table (240
 *   MiB at the default) is allocated at the first cached call, and the first
 *   call that sees a key pays its build.  A call with more distinct keys than
 *   the cache holds, or made when the table found no room, takes the uncached
 *   path transparently.  A key that does not parse takes no slot.
 * Verdicts are identical with and without the flag for every input; the
 * argument rules are those of tmv_secp256k1_verify_batch, and any other flag
 * bit is TMV_ERR_ARG.  No reference counterpart (btcec parses the key per
 * call). */
int tmv_secp256k1_verify_batch_ex(tmv_ctx *ctx, uint32_t flags, const uint8_t *pk, const uint8_t *sig,
                                  const uint8_t *msg, const uint32_t *msg_off, uint32_t n, uint8_t *valid_out);
/* Counters of that cache since tmv_open, per distinct key per call: hits
 * (found), misses (built); used / capacity in keys.  Any pointer may be NULL. */
int tmv_secp256k1_key_cache_stats(tmv_ctx *ctx, uint64_t *hits, uint64_t *misses, uint32_t *used, uint32_t *capacity);

/* Single secp256k1 verification (secp256k1.go:206-226).  Returns 0 without
 * touching the device when pk_len != 33 or sig_len != 64 (the reference
 * returns false for a signature of another size; keys of another size cannot
 * enter a validator set).  Returns 1/0 or <0. */
int tmv_secp256k1_verify(tmv_ctx *ctx, const uint8_t *pk, size_t pk_len, const uint8_t *msg, size_t msg_len,
                         const uint8_t *sig, size_t sig_len);

/* sr25519 batch verification (Schnorrkel, empty signing context).
 * Replaces: crypto/sr25519/batch.go:23-47 Add + Verify.  status_out[i] is
 * 1 / 0 / TMV_SR_ADDERR_*; the return value is TMV_ALL_VALID only if every
 * status is 1. */
int tmv_sr25519_verify_batch(tmv_ctx *ctx, const uint8_t *pk, const uint8_t *sig, const uint8_t *msg,
                             const uint32_t *msg_off, uint32_t n, int8_t *status_out);

/* Mixed ed25519 + sr25519 batch in one launch; kind[i] = TMV_KIND_*.
 * status_out as for sr25519 (ed25519 entries are 1/0). */
int tmv_verify_mixed_batch(tmv_ctx *ctx, const uint8_t *kind, const uint8_t *pk, const uint8_t *sig,
                           const uint8_t *msg, const uint32_t *msg_off, uint32_t n, int8_t *status_out);

/* Batch verification with options.  flags:
 *   TMV_FLAG_KEY_CACHE  keep expanded public keys on the device (LRU of
 *   TMV_KEY_CACHE_CAPACITY keys per device, default 4,096 = voi's cache size,
 *   crypto/ed25519/ed25519.go:31,56).  A cached key is a 64-row comb of -A
 *   (80 KB), so [k]A needs no doublings; the first batch that sees a key
 *   pays its table build.  Batches with more distinct keys than the cache
 *   holds take the uncached path transparently.  Results are identical
 *   either way.
 * Replaces the caching verifier behind crypto/ed25519/ed25519.go:173-233
 * (ed25519) and crypto/sr25519/batch.go:23-47 (sr25519).  status_out as for
 * tmv_sr25519_verify_batch (ed25519 entries are 1/0). */
#define TMV_FLAG_KEY_CACHE 1u
int tmv_verify_batch_ex(tmv_ctx *ctx, uint8_t key_kind, uint32_t flags, const uint8_t *pk, const uint8_t *sig,
                        const uint8_t *msg, const uint32_t *msg_off, uint32_t n, int8_t *status_out);
/* Batch equation (random linear combination), the
 * check voi's BatchVerifier.Verify runs (crypto/ed25519/ed25519.go:231-233,
 * crypto/sr25519/batch.go:44-47): entries are split into groups of
 * 2^group_log2 consecutive signatures of one kind; each group is checked with
 * one multi-scalar multiplication under fresh 128-bit random weights
 * (ed25519: cofactored [8](...) == O, ZIP-215; sr25519: Ristretto identity)
 * and the entries of a failing group are verified one by one, so the
 * validity vector is the same as per-entry verification (false accept
 * probability <= 2^-128 per group, as the reference's).
 *   TMV_FLAG_BATCH_EQUATION  use it for this call
 *   TMV_FLAG_PER_ENTRY       never use it for this call
 * Neither flag: batch equation when n >= $TMV_MSM_MIN (default 32768, key-
 * cached batches 16384; the variable sets both, 0 = never): smaller batches
 * are latency-bound and verify faster per entry.
 * TMV_FLAG_BATCH_EQUATION overrides TMV_FLAG_KEY_CACHE. */
#define TMV_FLAG_BATCH_EQUATION 2u
#define TMV_FLAG_PER_ENTRY 4u
/* group_log2: 0 = default (6) or 5..10; window_bits: 0 = chosen from the group
 * size, or 4..9; seed32: NULL = a fresh getrandom() key per call (production),
 * else a fixed ChaCha20 key (tests: reproducible weights).
 * opt_flags: TMV_BATCHOPT_STATS = count group verdicts (host-buffer calls;
 * costs one small device read per call); TMV_BATCHOPT_SUBCHECK_ON / _OFF =
 * re-check failing groups by sub-groups of 8 before the per-entry fallback
 * (default: for groups of >= 256 entries); with it off,
 * launches of >= $TMV_LOCATE_MIN (400000) entries locate a failing group's
 * one bad entry by a second, index-weighted equation. */
#define TMV_BATCHOPT_STATS 1u
#define TMV_BATCHOPT_SUBCHECK_ON 2u
#define TMV_BATCHOPT_SUBCHECK_OFF 4u
int tmv_set_batch_options(tmv_ctx *ctx, uint32_t group_log2, uint32_t window_bits, const uint8_t *seed32,
                          uint32_t opt_flags);
/* Groups checked / failed since the context was opened (TMV_BATCHOPT_STATS). */
int tmv_batch_stats(tmv_ctx *ctx, uint64_t *groups, uint64_t *groups_failed);
/* ValidatorSet.Hash of n_sets validator sets in one launch (SURVEY §8(f)
 * rank 4): replaces types/validator_set.go:344-350 (merkle.HashFromByteSlices,
 * crypto/merkle/tree.go:11-27, over Validator.Bytes(), types/validator.go:
 * 154-170), as the light client checks it per header (light/verifier.go:266).
 * Set s holds validators [set_off[s], set_off[s+1]) in set order; validator
 * i: pk + 32*i, key_kind[i] (TMV_KIND_ED25519 / TMV_KIND_SR25519; sets that
 * hold 33-byte secp256k1 keys are hashed by the host layer), power[i].  hash_out: n_sets x 32 bytes (an empty
 * set hashes to SHA-256(""), as the reference).  set_off[0] must be 0.
 * Synchronous; 0 or < 0 on error. */
int tmv_validator_set_hashes(tmv_ctx *ctx, const uint8_t *pk, const uint8_t *key_kind, const int64_t *power,
                             const uint32_t *set_off, uint32_t n_sets, uint8_t *hash_out);
/* merkle.HashFromByteSlices of n_trees trees in one launch (crypto/merkle/
 * tree.go:11-27: RFC 6962 leaves SHA-256(0x00 || leaf), inner nodes
 * SHA-256(0x01 || l || r), split at the largest power of two below n).  The
 * host layer uses it for Header.Hash (types/block.go:447-478: 14 proto-encoded
 * fields per header) across a light client's window of headers.
 * Leaf i = data[leaf_off[i], leaf_off[i+1]) (n_leaves + 1 offsets,
 * leaf_off[0] = 0); tree t = leaves [tree_off[t], tree_off[t+1]) (n_trees + 1
 * offsets, tree_off[0] = 0, tree_off[n_trees] = n_leaves; an empty tree
 * hashes to SHA-256("")).  hash_out: n_trees x 32 bytes.  Synchronous; 0 or
 * < 0 on error. */
int tmv_merkle_roots(tmv_ctx *ctx, const uint8_t *data, const uint32_t *leaf_off, uint32_t n_leaves,
                     const uint32_t *tree_off, uint32_t n_trees, uint8_t *hash_out);
/* Commit.Hash of n_commits commits in one launch (types/block.go:900-918:
 * merkle.HashFromByteSlices over the protobuf bytes of every CommitSig,
 * proto/tendermint/types/types.pb.go:1764-1797), which Block.ValidateBasic
 * compares with Header.LastCommitHash for every block blocksync applies
 * (types/block.go:73-75).  Commit c holds the signatures [commit_off[c],
 * commit_off[c+1]) in commit order; signature i: flag[i] (BlockIDFlag, at most
 * 127: one varint byte), addr_len[i] (0 or 20) with the address at addr + 20*i
 * (ignored when addr_len[i] is 0), the timestamp ts_seconds[i] / ts_nanos[i],
 * sig_len[i] (0..64) with the signature at sig + 64*i.  Zero values are
 * omitted as proto3 does; negative seconds or nanos take the 10-byte varint.
 * Seconds outside [-62135596800, 253402300800) or nanos outside [0, 1e9) are
 * outside the reference's domain (StdTimeMarshalTo fails and Commit.Hash
 * panics); they are encoded as plain protobuf int64 / int32 here.
 * hash_out: n_commits x 32 bytes (a commit without signatures hashes to
 * SHA-256("")).  commit_off[0] must be 0.  Any other flag, addr_len or sig_len
 * is TMV_ERR_ARG: the host layer hashes such commits itself.  Synchronous,
 * device 0; at most 2^26 signatures per call; 0 or < 0 on error. */
int tmv_commit_hashes(tmv_ctx *ctx, const uint8_t *flag, const uint8_t *addr_len, const uint8_t *addr,
                      const int64_t *ts_seconds, const int32_t *ts_nanos, const uint8_t *sig_len, const uint8_t *sig,
                      const uint32_t *commit_off, uint32_t n_commits, uint8_t *hash_out);
/* The hash of a block's ABCI results, for n_trees blocks in one launch:
 * merkle.HashFromByteSlices over abci.MarshalTxResults (abci/types/types.go:
 * 213-239), which ApplyBlock stores as State.LastResultsHash
 * (internal/state/execution.go:262-267) and validateBlock compares with the
 * next header's LastResultsHash.  Tree t holds the results [tree_off[t],
 * tree_off[t+1]) (n_trees + 1 offsets, tree_off[0] = 0); result i is code[i],
 * the data data[data_off[i], data_off[i+1]) (n_results + 1 offsets,
 * data_off[0] = 0), gas_wanted[i] and gas_used[i].  Its leaf is the gogoproto
 * encoding of ExecTxResult with fields 1, 2, 5 and 6 alone
 * (abci/types/types.pb.go:3165-3170): [08 uvarint(code)] [12 uvarint(L) data]
 * [28 varint(gas_wanted)] [30 varint(gas_used)], zero and empty fields omitted
 * as proto3 does, a negative gas in the 10-byte two's-complement varint.  Log,
 * info, events and codespace are not hashed and never come here.
 * flags: 0, or TMV_RESULTS_FIRST_LEAF: tree t gets the leading leaf
 * first[first_off[t], first_off[t+1]) (n_trees + 1 offsets; may be empty) in
 * front of its results -- the light client's proto.Marshal(
 * ResponseFinalizeBlock{Events}) (light/rpc/client.go:452-464; the reference's
 * two forms differ, both are as written there).  Without the flag first and
 * first_off are ignored.
 * root_out: n_trees x 32 bytes; a tree without leaves hashes to SHA-256("").
 * One lane hashes one result whatever its length, so one result of many KiB
 * delays the whole call (the host layer keeps such trees on the host).
 * TMV_ERR_ARG: null pointers, offsets that do not start at 0 or decrease, an
 * unknown flag bit, more than 2^26 results or trees, more than 2^30 bytes of
 * data or of leading leaves.  n_trees == 0 returns 0.  Synchronous, device 0;
 * 0 or < 0 on error. */
#define TMV_RESULTS_FIRST_LEAF 1u
int tmv_tx_results_hashes(tmv_ctx *ctx, uint32_t flags, const uint32_t *code, const int64_t *gas_wanted,
                          const int64_t *gas_used, const uint8_t *data, const uint32_t *data_off,
                          const uint32_t *tree_off, uint32_t n_trees, const uint8_t *first, const uint32_t *first_off,
                          uint8_t *root_out);

/* Merkle roots over spans of one buffer: what Block.ValidateBasic hashes lies
 * in a block's protobuf bytes verbatim (a Commit.Hash leaf is the payload of a
 * `signatures` entry, a Data.Hash leaf SHA-256 of a `txs` entry, a Header.Hash
 * leaf a header field's payload behind at most one wrapper tag), so a window
 * of received blocks is hashed from a table of spans, with no columns packed
 * (the host layer's tmv_blocks_validate_wire builds the table; DESIGN.md
 * section 22).
 * Leaf i is SHA-256(0x00 || [tag] || data[pos, pos + len)): the RFC 6962 leaf
 * prefix, with TMV_SPAN_TAG one more byte (the low 8 bits of flags, which are
 * 0 without it), then the span.  With TMV_SPAN_PREHASH it is SHA-256(0x00 ||
 * SHA-256(span)), as Txs.Hash (types/tx.go:34-39); not together with TAG.
 * Tree t holds the leaves [tree_off[t], tree_off[t+1]) (tree_off[0] = 0,
 * tree_off[n_trees] = n_leaves); a tree without leaves hashes to SHA-256("").
 * Spans may overlap and come in any order.  root_out: n_trees x 32 bytes.
 * One upload (bytes, spans and offsets), one k_span_leaves launch, one
 * k_merkle_tree launch, one copy back.  One lane hashes one leaf whatever its
 * length, so one span of many KiB delays the whole call (the host layer keeps
 * such blocks' transactions on the host).
 * TMV_ERR_ARG: null pointers, pos + len > data_len, both flags, an unknown flag
 * bit (a tag byte without TMV_SPAN_TAG among them), offsets that do not start
 * at 0, decrease or do not end at n_leaves, more than 2^26 leaves or trees,
 * more than 2^30 bytes.  n_trees == 0 returns 0.  Synchronous, device 0; 0 or
 * < 0 on error. */
typedef struct { uint32_t pos, len, flags; } tmv_leaf_span;
#define TMV_SPAN_TAG     0x100u /* low 8 bits of flags: one byte hashed between the leaf prefix and the span */
#define TMV_SPAN_PREHASH 0x200u /* leaf = SHA-256(0x00 || SHA-256(span)), as Txs.Hash; not together with TAG */
int tmv_merkle_span_roots(tmv_ctx *ctx, const uint8_t *data, uint32_t data_len,
                          const tmv_leaf_span *leaves, uint32_t n_leaves,
                          const uint32_t *tree_off, uint32_t n_trees, uint8_t *root_out);

/* tmv_merkle_span_roots with ValidatorSet.Hash leaves hashed from the protobuf
 * bytes of the validators themselves: what LightBlock.ValidateBasic hashes
 * (types/light.go:37-60: Header.Hash and ValidatorSet.Hash) for a window of
 * serialised light blocks, in one call.
 * A ValidatorSet.Hash leaf is SimpleValidator{pub_key = 1, voting_power = 2}
 * (types/validator.go:154-170).  In the canonical encoding of Validator
 * {address = 1, pub_key = 2, voting_power = 3, proposer_priority = 4} the two
 * fields lie next to each other, 12 LL <PublicKey> [18 <varint>], and
 * SimpleValidator's bytes are those bytes with the tags replaced, 12 -> 0a and
 * 18 -> 10, whatever the key type.  A validator leaf names that span: pos (the
 * 12), len (to the end of the power's varint), power_at (the 18's offset in
 * the span, or len for a power of 0, which is not encoded).  Its hash is
 *   SHA-256(00 || 0a || data[pos+1, pos+power_at) || 10 || data[pos+power_at+1, pos+len))
 * without the 10 and the tail when power_at == len.  The engine substitutes
 * bytes 0 and power_at of the span and never interprets the rest.
 * Leaves [0, n_leaves) are tmv_merkle_span_roots leaves with its flags and
 * rules; leaves [n_leaves, n_leaves + n_val_leaves) are the validator leaves;
 * tree_off indexes the combined array (tree_off[n_trees] = n_leaves +
 * n_val_leaves), so a tree may hold both kinds.  Either table may be empty.
 * One upload (bytes, both tables and offsets), at most one k_span_leaves
 * launch, one k_valset_span_leaves launch (one lane per validator, one SHA-256
 * block each), one k_merkle_tree launch, one copy back.
 * TMV_ERR_ARG: tmv_merkle_span_roots' cases, and a validator leaf with len < 2,
 * len > 54, power_at < 2, power_at > len or pos + len > data_len, and n_leaves +
 * n_val_leaves > 2^26; everything is checked before anything is uploaded.
 * n_trees == 0 returns 0.  Synchronous, device 0; 0 or < 0 on error. */
typedef struct { uint32_t pos, len, power_at; } tmv_val_span;
int tmv_merkle_wire_roots(tmv_ctx *ctx, const uint8_t *data, uint32_t data_len,
                          const tmv_leaf_span *leaves, uint32_t n_leaves,
                          const tmv_val_span *val_leaves, uint32_t n_val_leaves,
                          const uint32_t *tree_off, uint32_t n_trees, uint8_t *root_out);

/* Merkle inclusion proofs (crypto/merkle/proof.go).  Blocksync's replay loop
 * builds every block's part set (internal/blocksync/reactor.go:563-582:
 * first.MakePartSet -> NewPartSetFromData, types/part_set.go:172-200 ->
 * merkle.ProofsFromByteSlices over the 64 KiB parts) for the BlockID that
 * VerifyCommitLight checks; PartSet.AddPart verifies each received part's
 * proof (types/part_set.go:272-300); Txs.Hash / Txs.Proof run the same tree
 * over SHA-256(tx) (types/tx.go:30-75).
 * flags of both calls:
 *   TMV_MERKLE_PREHASH          the leaf is SHA-256(0x00 || SHA-256(item)):
 *                               the items are hashed first, as Txs.Hash does
 *   TMV_MERKLE_LEAF_HASH_GIVEN  (verify) no leaves are supplied; leaf_hash is
 *                               taken as Proof.Verify's leafHash(leaf)
 *   TMV_MERKLE_LONG_LEAVES / TMV_MERKLE_SHORT_LEAVES, TMV_MERKLE_LPW(8|16|32|64)
 *                               tuning aids: force the long-leaf kernel / the
 *                               byte-wise kernel of tmv_merkle_roots, and the
 *                               long-leaf kernel's leaves per wave.  Default:
 *                               the long-leaf kernel when the leaves average
 *                               >= $TMV_MERKLE_LONG_MIN bytes (512) or with
 *                               TMV_MERKLE_PREHASH, leaves per wave from the
 *                               leaf count.  Results do not depend on them. */
#define TMV_MERKLE_PREHASH 1u
#define TMV_MERKLE_LEAF_HASH_GIVEN 2u
#define TMV_MERKLE_LONG_LEAVES 4u
#define TMV_MERKLE_SHORT_LEAVES 8u
#define TMV_MERKLE_LPW(l) ((uint32_t)(l) << 8)
/* A proof's aunt count depends on (index, total) alone: aunt_off_out[i] is the
 * number of aunts of all leaves before leaf i of n_trees trees laid out as for
 * tmv_merkle_roots (tree_off[n_trees] + 1 entries; no device work). */
int tmv_merkle_aunt_offsets(const uint32_t *tree_off, uint32_t n_trees, uint32_t *aunt_off_out);
/* merkle.ProofsFromByteSlices (proof.go:33-48) of n_trees trees in one call;
 * data, leaf_off, tree_off as for tmv_merkle_roots.  root_out: n_trees x 32
 * (an empty tree: SHA-256("")); leaf_hash_out: n_leaves x 32 (Proof.LeafHash);
 * the aunts of leaf i, leaf sibling first (FlattenAunts, proof.go:197-215),
 * are aunts_out[32*aunt_off[i] .. 32*aunt_off[i+1]) with aunt_off from
 * tmv_merkle_aunt_offsets (anything else is TMV_ERR_ARG).  aunts_out == NULL:
 * roots and leaf hashes only (MakePartSet().Header()).  Proof i has Total =
 * its tree's leaf count and Index = i - tree_off[t].  Synchronous, device 0;
 * limits and errors as tmv_merkle_roots; 0 or < 0. */
int tmv_merkle_proofs(tmv_ctx *ctx, uint32_t flags, const uint8_t *data, const uint32_t *leaf_off, uint32_t n_leaves,
                      const uint32_t *tree_off, uint32_t n_trees, uint8_t *root_out, uint8_t *leaf_hash_out,
                      const uint32_t *aunt_off, uint8_t *aunts_out);
/* Proof.Verify (proof.go:52-68) of n proofs.  Proof i: total[i], index[i],
 * leaf_hash + 32*i, aunts[32*aunt_off[i] .. 32*aunt_off[i+1]) (any count),
 * checked against root + 32*i and the leaf data[leaf_off[i], leaf_off[i+1])
 * (data / leaf_off unused with TMV_MERKLE_LEAF_HASH_GIVEN).  status_out[i], in
 * the reference's order of tests: 0 ok, 1 total < 0, 2 index < 0, 3 the leaf's
 * hash differs from leaf_hash, 4 the root computed from leaf_hash and the
 * aunts (computeHashFromAunts, proof.go:151-181) differs from root or is nil
 * (index >= total, total == 0, or an aunt count that does not fit the path).
 * Optional outputs (NULL to skip): leaf_hash_calc n x 32 (the hashed leaf;
 * leaf_hash itself when given), root_calc n x 32 (zeros when nil), root_nil n.
 * Returns 0 (every status 0), 1 (some not) or < 0; n <= 2^26, leaves <= 2^30
 * bytes, <= 2^28 aunts. */
int tmv_merkle_verify_proofs(tmv_ctx *ctx, uint32_t flags, uint32_t n, const int64_t *total, const int64_t *index,
                             const uint8_t *leaf_hash, const uint8_t *aunts, const uint32_t *aunt_off,
                             const uint8_t *root, const uint8_t *data, const uint32_t *leaf_off, int8_t *status_out,
                             uint8_t *leaf_hash_calc, uint8_t *root_calc, uint8_t *root_nil);

/* Chained value proof operators: ValueOp.Run (crypto/merkle/proof_value.go:
 * 77-98) as ProofOperators.Verify chains it (proof_op.go:39-69), for n_items
 * items in one call -- the merkle work of the light client's
 * ABCIQueryWithOptions (light/rpc/client.go:148-217).  Item i has the input
 * value value[value_off[i], value_off[i+1]) (any length, 0 allowed) and owns
 * the ops [op_off[i], op_off[i+1]), at least one.  Op j, over all
 * n_ops = op_off[n_items]: the key key[key_off[j], key_off[j+1]) (any length),
 * total[j], index[j], leaf_hash + 32*j and the aunts
 * aunts[32*aunt_off[j] .. 32*aunt_off[j+1]), as tmv_merkle_verify_proofs takes
 * them.  With v the item's value for its first op and the root of the op
 * before for the others (the empty string when that root is nil: the
 * reference passes the nil slice on and hashes it),
 *   kv      = SHA-256(0x00 || uvarint(len key) || key || 0x20 || SHA-256(v))
 *   leaf_ok = (kv == leaf_hash)
 *   root    = computeHashFromAunts(index, total, leaf_hash, aunts)
 * (proof.go:151-181; from the *given* leaf hash, as the reference does; nil
 * exactly when tmv_merkle_verify_proofs says nil, so total < 0 and index < 0
 * are no errors here).  An item does not stop at a mismatch.
 * Outputs, any of them NULL to skip.  Per item: value_digest n_items x 32
 * (SHA-256(value)); status_out 0 ok, 3 some op's leaf hash differs, 4 the last
 * op's root is nil or differs from root + 32*i (the numbers of
 * tmv_merkle_verify_proofs); fail_op_out the first op with a mismatch, counted
 * from the item's first op (the last op for status 4, 0 for status 0).  Per
 * op: kv_hash_calc n_ops x 32, leaf_ok n_ops, root_calc n_ops x 32 (zeros when
 * nil), root_nil n_ops.
 * flags: 0, or TMV_MERKLE_LPW(8|16|32|64) to fix the leaves per wave of the
 * value digests (k_merkle_leaves_long's digest-only form; a tuning aid).
 * TMV_ERR_ARG: null inputs, offsets that do not start at 0 or decrease, an
 * item without ops, n_items or n_ops > 2^26, more than 2^30 bytes of values or
 * of keys, more than 2^28 aunts.  Synchronous, device 0.  Returns 0 (every
 * status 0), 1 (some not) or < 0. */
int tmv_merkle_value_ops(tmv_ctx *ctx, uint32_t flags, uint32_t n_items, const uint8_t *value,
                         const uint32_t *value_off, const uint32_t *op_off, const uint8_t *key, const uint32_t *key_off,
                         const int64_t *total, const int64_t *index, const uint8_t *leaf_hash, const uint8_t *aunts,
                         const uint32_t *aunt_off, const uint8_t *root, uint8_t *value_digest, uint8_t *kv_hash_calc,
                         uint8_t *leaf_ok, uint8_t *root_calc, uint8_t *root_nil, int8_t *status_out,
                         int32_t *fail_op_out);

/* Sub-groups of failing groups checked / failed (k_msm_subcheck: a failing
 * group's sub-groups of 8 entries are re-checked with the same equation
 * before entry-by-entry verification; TMV_BATCHOPT_STATS; 0 with
 * the sub-group check off).  No reference counterpart (voi verifies a failing batch
 * entry by entry, crypto/ed25519/ed25519.go:231-233). */
int tmv_subgroup_stats(tmv_ctx *ctx, uint64_t *subgroups, uint64_t *subgroups_failed);
/* Mixed batch with flags (see tmv_verify_mixed_batch). */
int tmv_verify_mixed_batch_ex(tmv_ctx *ctx, uint32_t flags, const uint8_t *kind, const uint8_t *pk,
                              const uint8_t *sig, const uint8_t *msg, const uint32_t *msg_off, uint32_t n,
                              int8_t *status_out);

/* Live kernel timing (profiling aid; bench.py's roofline object).  enable != 0:
 * every later launch of the timed kernels -- "k_msm_accum" (batch-equation
 * bucket sums), "k_msm_wpart" (window running sums), "k_prep_fused" (decode +
 * challenge), "k_secp_prep" and "k_secp_verify" (secp256k1), "k_secp_key_table", "k_secp_prep_cached" and
 * "k_secp_verify_comb" (secp256k1 with TMV_FLAG_KEY_CACHE), "k_merkle_leaves_long",
 * "k_merkle_leaves", "k_merkle_tree_levels", "k_merkle_aunts" and "k_merkle_verify_proofs" (the launches
 * of tmv_merkle_proofs / tmv_merkle_verify_proofs), "k_merkle_digests_long" and "k_merkle_value_ops"
 * (tmv_merkle_value_ops), "k_commit_leaves" (tmv_commit_hashes), "k_result_leaves" (tmv_tx_results_hashes),
 * "k_span_leaves" (tmv_merkle_span_roots, tmv_merkle_wire_roots), "k_valset_span_leaves"
 * (tmv_merkle_wire_roots) -- is bracketed by HIP timing events on the stream it runs on
 * (process-wide, two event records per launch); 0 turns it off.
 * tmv_kernel_timing_read waits for the recorded launches of `kernel`, returns
 * their summed duration and count, and forgets them.  No reference
 * counterpart (Go's benchmarks time whole calls). */
int tmv_kernel_timing(tmv_ctx *ctx, int enable);
int tmv_kernel_timing_read(tmv_ctx *ctx, const char *kernel, double *total_ms, uint64_t *launches);

/* Cumulative key-cache counters over the context's devices. */
int tmv_key_cache_stats(tmv_ctx *ctx, uint64_t *hits, uint64_t *misses, uint32_t *used, uint32_t *capacity);

/* Point cache (decoded ed25519 public keys, one table per device, used by
 * uncached batch-equation launches; TMV_POINT_CACHE_SLOTS): keys served from
 * the table and keys decoded, cumulative since the table was allocated and
 * summed over the context's devices, and the capacity in slots.  The
 * counters are read from the devices on this call only; the caller has
 * waited for the launches it wants counted. */
int tmv_point_cache_stats(tmv_ctx *ctx, uint64_t *hits, uint64_t *misses, uint32_t *slots);

/* Bucket entries the batch equation's sort placed (k_msm_sort, located pass
 * included), cumulative over the launches of this context's devices made
 * while TMV_BATCHOPT_STATS was set.  Entries per signature is the measure of
 * how far runs of one key collapsed (multi-batch launches of one validator
 * set's commits).  Read from the devices on this call only; the caller has
 * waited for the launches it wants counted. */
int tmv_bucket_entry_stats(tmv_ctx *ctx, uint64_t *entries);

/* Group verdicts of the uncached batch-equation launches made while
 * TMV_BATCHOPT_STATS was set, device-pointer launches included (which
 * tmv_batch_stats does not see): groups that failed the equation, failing
 * groups whose one bad entry the located pass named, and entries the located
 * pass left to verify one by one.  Counted on the devices, read on this call
 * only; the caller has waited for the launches it wants counted. */
int tmv_group_fail_stats(tmv_ctx *ctx, uint64_t *groups_failed, uint64_t *groups_located, uint64_t *fallback_entries);

/* Split key scalars of the same launches: groups whose A and B scalars were
 * split into a low and a high half, and the leaders' high points computed
 * for them.  Counted and read as tmv_group_fail_stats. */
int tmv_split_stats(tmv_ctx *ctx, uint64_t *groups_split, uint64_t *high_points);

/* Library metrics (verifies/s, batch size, fallback count, H2D
 * bytes -- the reference exports its own per package through Prometheus,
 * e.g. internal/consensus/metrics.gen.go; a Go shim would publish these).
 * Cumulative since tmv_open or the last tmv_metrics_reset.  The group fields
 * count host-buffer calls made with TMV_BATCHOPT_STATS
 * (tmv_set_batch_options); the rest are always kept. */
typedef struct tmv_metrics {
  uint64_t calls;               /* verification calls (host-buffer and device-resident entry points) */
  uint64_t signatures;          /* entries submitted to them */
  uint64_t max_batch;           /* largest call, in entries */
  uint64_t batch_eq_signatures; /* entries verified through the batch equation */
  uint64_t host_signatures;     /* entries of host-buffer calls */
  double host_seconds;          /* busy wall time of host-buffer calls: the union of their intervals, so calls
                                   in flight together count once (end-to-end rate = host_signatures / it);
                                   a call still in flight is not yet counted */
  uint64_t h2d_bytes;           /* host-to-device bytes of host-buffer calls (zero-copy reads not counted) */
  uint64_t d2h_bytes;           /* device-to-host bytes of host-buffer calls */
  uint64_t groups;              /* batch-equation groups checked (TMV_BATCHOPT_STATS) */
  uint64_t groups_failed;       /* of which failed */
  uint64_t located_groups;      /* failing groups whose one bad entry the located pass named */
  uint64_t fallback_signatures; /* entries verified one by one after failing groups */
  uint64_t key_cache_hits;      /* expanded-key cache (TMV_FLAG_KEY_CACHE) */
  uint64_t key_cache_misses;
} tmv_metrics;
int tmv_metrics_read(tmv_ctx *ctx, tmv_metrics *out);
int tmv_metrics_reset(tmv_ctx *ctx);

/* Device-resident variants: every pointer is device memory on HIP device
 * `device` (inputs already in HBM), `stream` is a hipStream_t (NULL = the
 * context's own stream for that device).  Asynchronous: the call enqueues the
 * kernel and returns TMV_NOT_ALL immediately (the verdict is in d_valid once
 * the stream is synchronised), or <0 on a launch error.  Used by the
 * multi-GPU sharded path (one process per GPU) and by bench.py. */
int tmv_ed25519_verify_batch_device(tmv_ctx *ctx, int device, const uint8_t *d_pk, const uint8_t *d_sig,
                                    const uint8_t *d_msg, const uint32_t *d_msg_off, uint32_t n,
                                    uint8_t *d_valid, void *stream);
int tmv_verify_mixed_batch_device(tmv_ctx *ctx, int device, const uint8_t *d_kind, const uint8_t *d_pk,
                                  const uint8_t *d_sig, const uint8_t *d_msg, const uint32_t *d_msg_off,
                                  uint32_t n, int8_t *d_status, void *stream);
/* Device-resident batch with flags; key_kind TMV_KIND_ED25519, TMV_KIND_SR25519
 * or TMV_KIND_MIXED (then d_kind gives each entry's kind).  d_status as for
 * tmv_sr25519_verify_batch (ed25519 entries 1/0). */
#define TMV_KIND_MIXED 2
int tmv_verify_batch_device_ex(tmv_ctx *ctx, int device, uint8_t key_kind, uint32_t flags, const uint8_t *d_kind,
                               const uint8_t *d_pk, const uint8_t *d_sig, const uint8_t *d_msg,
                               const uint32_t *d_msg_off, uint32_t n, int8_t *d_status, void *stream);

/* Several independent device-resident batches in one pipeline: the batches
 * are gathered into one contiguous batch on the device, verified together
 * (per-entry or batch equation, per flags) and each batch's statuses are
 * written to its own d_status (as tmv_verify_batch_device_ex).  Verdicts are
 * per entry, so this equals n_batches separate calls; it only widens the
 * launches (a node draining a queue of batches, blocksync look-ahead).
 * msg_bytes = msg_off[n] - msg_off[0].  Up to TMV_MAX_BATCHES batches (and
 * 2^26 entries in all); key_kind TMV_KIND_ED25519 or TMV_KIND_SR25519.
 * Asynchronous like the other device-resident entry points. */
#define TMV_MAX_BATCHES 256
typedef struct tmv_batch_ref {
  const uint8_t *pk;
  const uint8_t *sig;
  const uint8_t *msg;
  const uint32_t *msg_off;
  uint32_t n;
  uint32_t msg_bytes;
  int8_t *status;
} tmv_batch_ref;
int tmv_verify_batches_device(tmv_ctx *ctx, int device, uint8_t key_kind, uint32_t flags,
                              const tmv_batch_ref *batches, uint32_t n_batches, void *stream);

/* ---- Device-side vote sign-bytes ----
 * The canonical votes of one commit differ only in the timestamp and in
 * whether field 4 (the BlockID) is present: Commit.VoteSignBytes,
 * types/block.go:836-862, over CanonicalizeVote, types/canonical.go:52-63.
 * The caller encodes the shared fields once per (commit, chain_id) -- a
 * template, see tmv_vote_template_encode in tmhost.h -- and sends 16 bytes
 * per vote instead of the ~120-byte message; the device writes
 *   uvarint(len(body)) || head || [block] || 0x2a uvarint(len(ts)) ts || chain
 * into HBM, where ts = [0x08 uvarint(seconds)] [0x10 uvarint(nanos)] (proto3:
 * zero fields omitted), byte-identical to types.VoteSignBytes. */
typedef struct tmv_vote_template {
  const uint8_t *head;  /* fields 1-3 (type, height, round) */
  uint32_t head_len;
  const uint8_t *block; /* field 4, the commit's BlockID (empty when nil) */
  uint32_t block_len;
  const uint8_t *chain; /* field 6, chain_id (empty when "") */
  uint32_t chain_len;
} tmv_vote_template;

#define TMV_VOTE_WITH_BLOCK 0x80000000u /* tmpl bit: BlockIDFlagCommit, field 4 included */

typedef struct tmv_vote {
  int64_t ts_seconds;
  int32_t ts_nanos;
  uint32_t tmpl; /* template index | TMV_VOTE_WITH_BLOCK */
} tmv_vote;

/* tmv_verify_batch_ex over device-built sign-bytes: entry i signs the
 * message of votes[i].  Same flags, statuses and return values as
 * tmv_verify_batch_ex (TMV_ERR_ARG for a template index >= n_tmpl). */
int tmv_verify_votes(tmv_ctx *ctx, uint8_t key_kind, uint32_t flags, const tmv_vote_template *tmpl,
                     uint32_t n_tmpl, const tmv_vote *votes, const uint8_t *pk, const uint8_t *sig, uint32_t n,
                     int8_t *status_out);

/* The messages the device builds for tmv_verify_votes, copied back (tests,
 * tools).  msg_off_out gets n + 1 offsets; msg_out (capacity msg_cap) the
 * concatenated messages, or is skipped when NULL.  Returns the total length,
 * or < 0 (TMV_ERR_ARG if msg_cap is too small). */
int64_t tmv_vote_sign_bytes_device(tmv_ctx *ctx, const tmv_vote_template *tmpl, uint32_t n_tmpl,
                                   const tmv_vote *votes, uint32_t n, uint8_t *msg_out, size_t msg_cap,
                                   uint32_t *msg_off_out);

/* ---- Vote extensions ----
 * With vote extensions enabled a non-nil precommit carries a second
 * signature of the same key, over VoteExtensionSignBytes
 * (types/vote.go:159-172): CanonicalVoteExtension{extension, height, round,
 * chain_id}, length-delimited,
 *   M    = uvarint(len(body)) || body
 *   body = [0x0a uvarint(E) ext] || tail
 *   tail = [0x11 le64(height)] [0x19 le64(round)] [0x22 uvarint(C) chain_id]
 * (proto3: zero / empty fields omitted).  tail is shared by the precommits of
 * one (chain_id, height, round): the template, see
 * tmv_vote_extension_template_encode in tmhost.h. */
typedef struct tmv_vote_ext_template { const uint8_t *tail; uint32_t tail_len; } tmv_vote_ext_template;

/* tmv_verify_votes plus extension entries in ONE batch: entries [0, n_votes) sign the vote messages of votes[]
 * (exactly as tmv_verify_votes), entries [n_votes, n_votes + n_exts) sign the extension message built from
 * etmpl[ext_tmpl[j]] and ext_data[ext_off[j] .. ext_off[j+1]).  pk / sig / status_out hold n_votes + n_exts
 * entries in that order.  Either count may be 0.  Flags, statuses, return values, limits as tmv_verify_votes;
 * TMV_ERR_ARG for ext_off[0] != 0, decreasing offsets, a template index out of range, a null segment. */
int tmv_verify_votes_and_extensions(tmv_ctx *ctx, uint8_t key_kind, uint32_t flags,
        const tmv_vote_template *tmpl, uint32_t n_tmpl, const tmv_vote *votes, uint32_t n_votes,
        const tmv_vote_ext_template *etmpl, uint32_t n_etmpl, const uint32_t *ext_tmpl,
        const uint8_t *ext_data, const uint32_t *ext_off, uint32_t n_exts,
        const uint8_t *pk, const uint8_t *sig, int8_t *status_out);
/* The extension messages as the device writes them, copied back (tests, tools); as tmv_vote_sign_bytes_device. */
int64_t tmv_vote_extension_sign_bytes_device(tmv_ctx *ctx, const tmv_vote_ext_template *etmpl, uint32_t n_etmpl,
        const uint32_t *ext_tmpl, const uint8_t *ext_data, const uint32_t *ext_off, uint32_t n_exts,
        uint8_t *msg_out, size_t msg_cap, uint32_t *msg_off_out);

#ifdef __cplusplus
}
#endif
#endif /* TMVERIFY_H */
