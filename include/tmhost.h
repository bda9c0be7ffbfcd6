/*
 * tmhost.h — C-ABI of the host layer above the verification engine
 * (libtmgpu.so): the crypto.BatchVerifier object, canonical vote sign-bytes
 * and the commit verifiers, implemented in C++ (tendermint_amd/csrc/host/)
 * over include/tmverify.h.  Plain pointers and sizes only.
 *
 * These are the entry points a Go cgo shim binds:
 *   tmv_batch_*        crypto.BatchVerifier (crypto/crypto.go:66-76) created
 *                      by batch.CreateBatchVerifier (crypto/batch/batch.go:11-21)
 *   tmv_vote_sign_bytes types.VoteSignBytes (types/vote.go:149-157)
 *   tmv_verify_commit  types.VerifyCommit / VerifyCommitLight /
 *                      VerifyCommitLightTrusting (types/validation.go:27,61,96)
 *   tmv_light_verify   light.Verify / VerifyAdjacent / VerifyNonAdjacent
 *                      (light/verifier.go:33-177)
 *   tmv_header_hashes  types.Header.Hash (types/block.go:447-478)
 */
#ifndef TMHOST_H
#define TMHOST_H

#include <stddef.h>
#include <stdint.h>

#include "tmverify.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Key kinds: TMV_KIND_ED25519, TMV_KIND_SR25519 and TMV_KIND_SECP256K1 (33-byte
 * compressed keys, crypto/secp256k1/secp256k1.go; verified signature by
 * signature: no batch verifier, crypto/batch/batch.go:13-20); anything else
 * is a key type this library cannot verify (every signature is wrong). */
#define TMV_KIND_SECP256K1 3
#define TMV_KIND_OTHER 255

/* ---- crypto.BatchVerifier ---- */
typedef struct tmv_batch tmv_batch;

/* batch.CreateBatchVerifier: NULL when key_kind has no batch verifier. */
tmv_batch *tmv_batch_new(tmv_ctx *ctx, uint8_t key_kind);
/* Add: returns 0, or 1 with the reference's error text in err (type and
 * length checks: crypto/ed25519/ed25519.go:209-224,
 * crypto/sr25519/batch.go:23-28).  Curve-decoding failures of sr25519 keys
 * and signatures are reported by tmv_batch_verify (deferred Add error). */
int tmv_batch_add(tmv_batch *b, uint8_t key_kind, const uint8_t *pk, size_t pk_len, const uint8_t *msg,
                  size_t msg_len, const uint8_t *sig, size_t sig_len, char *err, size_t err_cap);
size_t tmv_batch_len(const tmv_batch *b);
/* Verify: 1 all valid, 0 not (or empty), 2 a deferred Add error (index in
 * *add_err_index, text in err), < 0 infrastructure error.  valid_out gets
 * one byte per entry in Add order. */
int tmv_batch_verify(tmv_batch *b, uint8_t *valid_out, int64_t *add_err_index, char *err, size_t err_cap);
void tmv_batch_free(tmv_batch *b);

/* ---- commit data ---- */
typedef struct {
  const uint8_t *hash;
  uint32_t hash_len;
  uint32_t psh_total;
  const uint8_t *psh_hash;
  uint32_t psh_hash_len;
} tmv_block_id;

typedef struct {
  const uint8_t *address;
  uint32_t address_len;
  const uint8_t *pub_key;
  uint32_t pub_key_len;
  uint8_t key_kind;
  int64_t voting_power;
  int64_t proposer_priority;
} tmv_validator;

typedef struct {
  uint8_t block_id_flag; /* 1 absent, 2 commit, 3 nil */
  const uint8_t *validator_address;
  uint32_t validator_address_len;
  int64_t ts_seconds;
  int32_t ts_nanos;
  const uint8_t *signature;
  uint32_t signature_len;
} tmv_commit_sig;

typedef struct {
  int64_t height;
  int32_t round;
  tmv_block_id block_id;
  const tmv_commit_sig *sigs;
  uint32_t n_sigs;
} tmv_commit;

/* types.VoteSignBytes for (chain_id, type, height, round, block_id or NULL
 * for nil, timestamp).  Returns the length; writes min(len, cap) bytes. */
size_t tmv_vote_sign_bytes(const char *chain_id, int32_t vote_type, int64_t height, int32_t round,
                           const tmv_block_id *block_id, int64_t ts_seconds, int32_t ts_nanos, uint8_t *out,
                           size_t cap);

/* The vote template of tmv_verify_votes (tmverify.h) for (chain_id, type,
 * height, round, block_id or NULL for nil): the three segments are written
 * back to back into out (head, then block, then chain) and their lengths
 * into lens[3].  Returns the total length; writes min(total, cap) bytes. */
size_t tmv_vote_template_encode(const char *chain_id, int32_t vote_type, int64_t height, int32_t round,
                                const tmv_block_id *block_id, uint8_t *out, size_t cap, uint32_t lens[3]);

#define TMV_COMMIT_FULL 0           /* types.VerifyCommit */
#define TMV_COMMIT_LIGHT 1          /* types.VerifyCommitLight */
#define TMV_COMMIT_LIGHT_TRUSTING 2 /* types.VerifyCommitLightTrusting */

/* Verify a commit against a validator set.  vals == NULL means a nil
 * validator set, commit == NULL a nil commit.  proposer_index < 0 derives
 * the proposer from priorities.  block_id / height are ignored for
 * LIGHT_TRUSTING; trust_num / trust_den only apply to it.
 * Returns 0 (ok), 1 (verification error; text in err, byte-identical to the
 * reference's error), < 0 infrastructure error. */
int tmv_verify_commit(tmv_ctx *ctx, int mode, const char *chain_id, const tmv_validator *vals, uint32_t n_vals,
                      int32_t proposer_index, const tmv_block_id *block_id, int64_t height, const tmv_commit *commit,
                      int64_t trust_num, int64_t trust_den, char *err, size_t err_cap);

/* Many commit checks in one device batch (cross-commit batching: blocksync
 * look-ahead, light-client sequential headers).  Each job is
 * one tmv_verify_commit call; results[j] = 0 ok / 1 error (text at
 * errs + j*err_stride), identical to calling tmv_verify_commit per job.
 * Jobs that pass the same tmv_commit pointer share signature entries (a
 * commit that blocksync checks light and then full is verified once).
 * Returns the number of failed jobs, or < 0 on an infrastructure error. */
typedef struct {
  int mode;
  const char *chain_id;
  const tmv_validator *vals;
  uint32_t n_vals;
  int32_t proposer_index;
  const tmv_block_id *block_id;
  int64_t height;
  const tmv_commit *commit;
  int64_t trust_num;
  int64_t trust_den;
} tmv_commit_job;

int tmv_verify_commits(tmv_ctx *ctx, const tmv_commit_job *jobs, uint32_t n_jobs, int32_t *results, char *errs,
                       size_t err_stride);

/* ---- consensus votes (ADR-064 batched vote verification) ---- */
/* The parts of a types.Vote (types/vote.go:50-62) Vote.Verify reads, with
 * the signing validator's public key (val.PubKey, looked up by the caller
 * from ValidatorIndex as VoteSet.addVote does, types/vote_set.go:183-199). */
typedef struct {
  int32_t type; /* SignedMsgType: 1 prevote, 2 precommit */
  int64_t height;
  int32_t round;
  const tmv_block_id *block_id; /* NULL (or a nil BlockID) = vote for nil */
  int64_t ts_seconds;
  int32_t ts_nanos;
  const uint8_t *validator_address;
  uint32_t validator_address_len;
  const uint8_t *signature;
  uint32_t signature_len;
  uint8_t key_kind; /* TMV_KIND_ED25519 / TMV_KIND_SR25519 (secp256k1 votes: not verified here) */
  const uint8_t *pub_key;
  uint32_t pub_key_len;
} tmv_vote_in;

#define TMV_VOTE_OK 0
#define TMV_VOTE_ERR_INVALID_ADDRESS 1   /* types.ErrVoteInvalidValidatorAddress */
#define TMV_VOTE_ERR_INVALID_SIGNATURE 2 /* types.ErrVoteInvalidSignature */

/* Vote.Verify(chainID, pubKey) (types/vote.go:226-243: address check, then
 * PubKey.VerifySignature over VoteSignBytes) of n votes in ONE signature
 * batch: the batched vote verification ADR-064 describes for consensus
 * (docs/architecture/adr-064-batch-verification.md:58-64: once 2/3+ of the
 * votes have arrived they are verified together).  results[i] = TMV_VOTE_*,
 * identical to verifying vote i alone.  Returns the number of failed votes,
 * or < 0 on an infrastructure error. */
int tmv_verify_vote_batch(tmv_ctx *ctx, const char *chain_id, const tmv_vote_in *votes, uint32_t n,
                          int32_t *results);

/* ---- vote extensions ---- */
/* types.VoteExtensionSignBytes (types/vote.go:159-172) for (chain_id, height,
 * round, extension).  Returns the length; writes min(len, cap) bytes. */
size_t tmv_vote_extension_sign_bytes(const char *chain_id, int64_t height, int32_t round,
                                     const uint8_t *ext, size_t ext_len, uint8_t *out, size_t cap);
/* The template of tmv_verify_votes_and_extensions (tmverify.h): the bytes the
 * extension messages of one (chain_id, height, round) share.  Returns the
 * length; writes min(len, cap) bytes. */
size_t tmv_vote_extension_template_encode(const char *chain_id, int64_t height, int32_t round, uint8_t *out, size_t cap);

typedef struct { tmv_vote_in vote; const uint8_t *extension; uint32_t extension_len;
                 const uint8_t *extension_signature; uint32_t extension_signature_len; } tmv_ext_vote_in;
#define TMV_VOTE_MODE_VERIFY 0                /* Vote.Verify                 types/vote.go:240-243 */
#define TMV_VOTE_MODE_VERIFY_AND_EXTENSION 1  /* Vote.VerifyVoteAndExtension types/vote.go:249-262 */
#define TMV_VOTE_MODE_EXTENSION 2             /* Vote.VerifyExtension        types/vote.go:266-276 (no address check) */
/* The three ways the reference verifies a vote that may carry an extension, n
 * votes at once, in its order: the address check, the vote signature, then --
 * for non-nil precommits only -- the extension signature over
 * VoteExtensionSignBytes (an extension on a prevote or a nil precommit is not
 * looked at; an extension signature that is empty or not 64 bytes long is an
 * invalid signature).  results[i] = TMV_VOTE_*, identical to verifying vote i
 * alone; failed_sig[i] (may be NULL) = 0 none, 1 the vote's, 2 the
 * extension's.  All ed25519 signatures of the call, votes' and extensions',
 * go out in one engine call with TMV_FLAG_KEY_CACHE, all sr25519 ones in
 * another; secp256k1 ones (33-byte keys, address RIPEMD160(SHA256(key)))
 * through tmv_secp256k1_verify_batch.  Calls with at least
 * TMV_VOTE_EXT_DEVICE_MIN signatures of a kind (environment; default below)
 * build that kind's messages on the device (tmv_verify_votes_and_extensions),
 * smaller ones on the host (tmv_verify_batch_ex).  Returns the number of
 * failed votes, or < 0 on an infrastructure error. */
#define TMV_VOTE_EXT_DEVICE_MIN_DEFAULT 0xffffffffu /* host-built messages: measured faster at 300 .. 210,000 signatures per call, DESIGN.md section 17 */
int tmv_verify_extended_votes(tmv_ctx *ctx, int mode, const char *chain_id, const tmv_ext_vote_in *votes, uint32_t n,
                              int32_t *results /* TMV_VOTE_* */, uint8_t *failed_sig /* may be NULL: 0 none, 1 vote, 2 extension */);

/* ---- light client (light/verifier.go) ---- */
typedef struct {
  const uint8_t *p;
  uint32_t len;
} tmv_bytes;

/* types.Header (types/block.go:338-366); chain_id NUL-terminated. */
typedef struct {
  uint64_t version_block, version_app;
  const char *chain_id;
  int64_t height;
  int64_t time_seconds;
  int32_t time_nanos;
  tmv_block_id last_block_id;
  tmv_bytes last_commit_hash, data_hash, validators_hash, next_validators_hash, consensus_hash, app_hash,
      last_results_hash, evidence_hash, proposer_address;
} tmv_header;

/* types.SignedHeader (types/light.go:131-136); NULL members = nil. */
typedef struct {
  const tmv_header *header;
  const tmv_commit *commit;
} tmv_signed_header;

/* types.ValidatorSet (proposer_index < 0: derived from the priorities). */
typedef struct {
  const tmv_validator *vals;
  uint32_t n_vals;
  int32_t proposer_index;
} tmv_validator_set;

/* Header.Hash (types/block.go:447-478) of n headers; has_hash[i] = 0 when the
 * reference returns nil (empty ValidatorsHash), else hash_out + 32*i holds it.
 * Many headers go to the device in one tmv_merkle_roots launch.  0 or < 0. */
int tmv_header_hashes(tmv_ctx *ctx, const tmv_header *headers, uint32_t n, uint8_t *hash_out, uint8_t *has_hash);

#define TMV_LIGHT_VERIFY 0       /* light.Verify (light/verifier.go:158-177) */
#define TMV_LIGHT_ADJACENT 1     /* light.VerifyAdjacent (light/verifier.go:106-155) */
#define TMV_LIGHT_NON_ADJACENT 2 /* light.VerifyNonAdjacent (light/verifier.go:33-91) */

/* Result classes (light/errors.go:15-40): the reference's error types. */
#define TMV_LIGHT_OK 0
#define TMV_LIGHT_ERR_INVALID_HEADER 1     /* light.ErrInvalidHeader */
#define TMV_LIGHT_ERR_OLD_HEADER_EXPIRED 2 /* light.ErrOldHeaderExpired */
#define TMV_LIGHT_ERR_CANT_TRUST 3         /* light.ErrNewValSetCantBeTrusted */
#define TMV_LIGHT_ERR_OTHER 4              /* a plain error (errors.New / fmt.Errorf) */

/* One light-client verification: the arguments of light.Verify /
 * VerifyAdjacent / VerifyNonAdjacent.  trusted_vals = the trusted header's
 * next validators (unused by VerifyAdjacent); times are UTC; trust level
 * = trust_num / trust_den (tmmath.Fraction). */
typedef struct {
  int mode; /* TMV_LIGHT_VERIFY / _ADJACENT / _NON_ADJACENT */
  const tmv_signed_header *trusted;
  const tmv_validator_set *trusted_vals;
  const tmv_signed_header *untrusted;
  const tmv_validator_set *untrusted_vals;
  int64_t trusting_period_ns;
  int64_t now_seconds;
  int32_t now_nanos;
  int64_t max_clock_drift_ns;
  uint64_t trust_num, trust_den;
} tmv_light_job;

/* Many light verifications in one pass: header and validator-set hashes of
 * all jobs in one device launch each, every commit check of all jobs in one
 * signature batch (tmv_verify_commits).  results[j] = TMV_LIGHT_* class,
 * error text at errs + j*err_stride, each identical to a tmv_light_verify
 * of job j alone.  Returns the number of failed jobs or < 0 (infrastructure). */
int tmv_light_verify_many(tmv_ctx *ctx, const tmv_light_job *jobs, uint32_t n_jobs, int32_t *results, char *errs,
                          size_t err_stride);
/* One job: returns its TMV_LIGHT_* class (text in err) or < 0. */
int tmv_light_verify(tmv_ctx *ctx, const tmv_light_job *job, char *err, size_t err_cap);

/* ---- block part sets and merkle proofs (types/part_set.go, crypto/merkle/proof.go) ---- */
/* Above $TMV_DEVICE_MERKLE_MIN bytes of leaves per call (default 64 MiB: below
 * it a 64 KiB part's serial SHA-256 chain on one lane outlasts 16 host
 * threads) these calls hash on the device
 * (tmv_merkle_proofs / tmv_merkle_verify_proofs, reached through weak
 * references), below it, and in a build without the engine, on the host --
 * the same verdicts and texts either way. */

/* merkle.Proof (proof.go:26-31). */
typedef struct {
  int64_t total, index;
  tmv_bytes leaf_hash;
  const tmv_bytes *aunts;
  uint32_t n_aunts;
} tmv_proof;

/* NewPartSetFromData(data, partSize).Header() (types/part_set.go:172-222) of n
 * serialised blocks: what blocksync's replay loop computes per block
 * (internal/blocksync/reactor.go:563-582, first.MakePartSet) for the BlockID
 * that VerifyCommitLight checks.  total_out[b] = ceil(len / part_size) in the
 * reference's uint32 arithmetic (a partial last part is allowed; empty data:
 * 0 parts and SHA-256("")); hash_out: n x 32.  part_size == 0 is TMV_ERR_ARG.
 * Windows above the engine's 1 GiB take several engine calls.  0 or < 0. */
int tmv_part_set_headers(tmv_ctx *ctx, const tmv_bytes *blocks, uint32_t n, uint32_t part_size, uint32_t *total_out,
                         uint8_t *hash_out);
/* The same with each part's merkle.Proof (Part.Proof, part_set.go:187-191).
 * The parts of all blocks are numbered one after the other (block b's first
 * part is the sum of the totals before it): part p has Proof.Total =
 * total_out[b], Proof.Index = its index in the block, LeafHash =
 * leaf_hash_out + 32*p and the aunts aunts_out[32*aunt_off_out[p] ..
 * 32*aunt_off_out[p+1]), leaf sibling first.  leaf_hash_out holds parts x 32
 * bytes, aunt_off_out parts + 1 entries, aunts_out aunts_cap hashes
 * (TMV_ERR_ARG when that is too few; parts * 32 always suffices). */
int tmv_part_set_proofs(tmv_ctx *ctx, const tmv_bytes *blocks, uint32_t n, uint32_t part_size, uint32_t *total_out,
                        uint8_t *hash_out, uint8_t *leaf_hash_out, uint32_t *aunt_off_out, uint8_t *aunts_out,
                        uint64_t aunts_cap);

/* A received part with the header of the set it is offered to. */
typedef struct {
  uint32_t index;     /* Part.Index */
  tmv_bytes bytes;    /* Part.Bytes */
  tmv_proof proof;    /* Part.Proof */
  uint32_t set_total; /* PartSetHeader.Total */
  tmv_bytes set_hash; /* PartSetHeader.Hash */
} tmv_part_in;

#define TMV_PART_OK 0
#define TMV_PART_ERR_UNEXPECTED_INDEX 1 /* types.ErrPartSetUnexpectedIndex: "error part set unexpected index" */
#define TMV_PART_ERR_INVALID_PROOF 2    /* types.ErrPartSetInvalidProof: "error part set invalid proof" */

/* PartSet.AddPart's checks (types/part_set.go:272-300) for n parts:
 * part.Index >= total, then part.Proof.Verify(ps.Hash(), part.Bytes).  As the
 * reference, it compares neither proof.Index with part.Index nor proof.Total
 * with the header's total.  results[i] = TMV_PART_*, the error's text at
 * errs + i*err_stride (errs may be NULL).  Returns the number of failed parts
 * or < 0. */
int tmv_parts_verify(tmv_ctx *ctx, const tmv_part_in *parts, uint32_t n, int32_t *results, char *errs,
                     size_t err_stride);

/* One proof with the leaf and root it is checked against. */
typedef struct {
  tmv_proof proof;
  tmv_bytes leaf;
  tmv_bytes root;
} tmv_proof_in;

/* Proof.ValidateBasic (proof.go:98-117) then Proof.Verify (proof.go:52-68) of
 * n proofs: results[i] = 0 ok / 1 error with the reference's text at
 * errs + i*err_stride ("negative Total", ..., "invalid root hash: wanted %X
 * got %X", a nil computed root printing as nothing).  Returns the number of
 * failed proofs or < 0. */
int tmv_proofs_verify(tmv_ctx *ctx, const tmv_proof_in *items, uint32_t n, int32_t *results, char *errs,
                      size_t err_stride);

/* ---- ABCI query proofs and tx proofs (light/rpc/client.go) ----
 * What the light client's RPC wrapper checks against a trusted header:
 * ABCIQueryWithOptions (light/rpc/client.go:148-217) runs
 * merkle.DefaultProofRuntime().VerifyValue / VerifyAbsence against AppHash,
 * Tx(hash, prove) (client.go:525-543) runs TxProof.Validate(DataHash).
 * Calls with at least $TMV_DEVICE_PROOF_OPS_MIN ops (tx proofs: items; default
 * 10,000) whose values and keys (txs) average at most
 * $TMV_DEVICE_PROOF_OPS_MAX_BYTES bytes per op (default 1044; staging moves a
 * byte more slowly than the host pool hashes it) go to
 * the device through tmv_merkle_value_ops / tmv_merkle_verify_proofs, in
 * windows of 16,384 ops; the others, and every call of a build without the
 * engine, compute on the host worker pool -- the same verdicts and texts
 * either way.  Both knobs are read on every call.  Of a call that goes to the
 * device, an item whose keys hold more than that many bytes per op, or whose
 * value more than 64 times that, is still hashed on the host: one lane would
 * hash it alone while its window waits.
 * Left to the caller, whose Go shim has the reference's own code for them and
 * none of which is data-parallel: protobuf decoding of ProofOp.Data, the
 * dispatch on ProofOp.Type ("unrecognized proof type"; only "simple:v" ops
 * come here) and KeyPathToKeys (proof_key_path.go:87-110). */

/* A decoded "simple:v" ProofOp: pop.Key and ValueOp.Proof. */
typedef struct {
  tmv_bytes key;
  tmv_proof proof;
} tmv_value_op;

typedef struct {
  const tmv_value_op *ops;
  uint32_t n_ops;
  tmv_bytes root;         /* the expected root (AppHash), any length */
  const tmv_bytes *keys;  /* KeyPathToKeys(keypath), first path part first */
  uint32_t n_keys;
  const tmv_bytes *value; /* NULL: VerifyAbsence (args == nil) */
} tmv_proof_ops_in;

/* ProofRuntime.Verify (crypto/merkle/proof_op.go:124-130) of n items under the
 * default runtime: results[i] = 0 ok / 1 error with the reference's text at
 * errs + i*err_stride, in the reference's order:
 *   every op's Proof.ValidateBasic first (ProofFromProto, proof.go:133-146):
 *     "decoding proof: decoding a proof operator: " + its text;
 *   then per op, for a non-empty op key, "key path has insufficient # of
 *     parts: expected no more keys but got %+v" / "key mismatch on operation
 *     #%d: expected %+v but got %+v" (keys print as raw bytes and are consumed
 *     from the last one backwards), then ValueOp.Run: "expected 1 arg, got 0"
 *     for an absent value (so absence proofs with ops always end there),
 *     "leaf hash mismatch: want %X got %X";
 *   "calculated root hash is invalid: expected %X but got %X" (a nil computed
 *     root prints as nothing and, as in bytes.Equal, equals an empty root);
 *   "keypath not consumed all".
 * An item without ops compares its value with the root; without ops and
 * without a value the reference panics: TMV_ERR_ARG.  Returns the number of
 * failed items or < 0. */
int tmv_proof_ops_verify(tmv_ctx *ctx, const tmv_proof_ops_in *items, uint32_t n, int32_t *results, char *errs,
                         size_t err_stride);

/* types.TxProof with the header's DataHash it is validated against. */
typedef struct {
  tmv_bytes root_hash, data; /* TxProof.RootHash, TxProof.Data */
  tmv_proof proof;           /* TxProof.Proof */
  tmv_bytes data_hash;       /* Header.DataHash */
} tmv_tx_proof_in;

/* TxProof.Validate (types/tx.go:286-301) of n items, in its order: "proof
 * matches different data hash", "proof index cannot be negative", "proof
 * total must be positive" (Total <= 0), and any failure of
 * Proof.Verify(RootHash, SHA-256(Data)) as "proof is not internally
 * consistent".  No ValidateBasic runs: a leaf hash or aunt of another size is
 * hashed as innerHash would.  Results, texts and return value as above. */
int tmv_tx_proofs_validate(tmv_ctx *ctx, const tmv_tx_proof_in *items, uint32_t n, int32_t *results, char *errs,
                           size_t err_stride);

/* ---- blocks (types/block.go) ---- */
/* Calls that hash at least $TMV_DEVICE_BLOCK_MIN commits (default 32, the rule
 * of tmv_header_hashes) go to the device through
 * tmv_commit_hashes / tmv_merkle_proofs / tmv_merkle_roots / tmv_header_hashes
 * (weak references); smaller calls, and a build without the engine, compute
 * on the host -- the same hashes, verdicts and texts either way. */

/* Commit.Hash (types/block.go:900-918) of n commits; commits[i] == NULL is a
 * nil commit (has_hash[i] = 0, hash_out + 32*i zeroed; has_hash may be NULL).
 * On the device path every commit the engine accepts (flags <= 127, addresses
 * of 0 or 20 bytes, signatures of at most 64) goes in one tmv_commit_hashes
 * launch and the others are hashed on the host.  0 or < 0. */
int tmv_commit_hash_many(tmv_ctx *ctx, const tmv_commit *const *commits, uint32_t n, uint8_t *hash_out,
                         uint8_t *has_hash);

/* The parts of a types.Block that Block.ValidateBasic reads.  evidence[i] is
 * ev.Bytes() of evidence item i (EvidenceList.Hash, types/evidence.go: the
 * merkle root over them); last_commit == NULL is a nil LastCommit. */
typedef struct {
  tmv_header header;
  const tmv_bytes *txs;
  uint32_t n_txs;
  const tmv_bytes *evidence;
  uint32_t n_evidence;
  const tmv_commit *last_commit;
} tmv_block;

/* Block.ValidateBasic (types/block.go:53-94) of n blocks, in the reference's
 * order and with its texts:
 *   invalid header: <Header.ValidateBasic>
 *   nil LastCommit
 *   wrong LastCommit: <Commit.ValidateBasic>
 *   wrong Header.LastCommitHash. Expected %X, got %X     (Commit.Hash)
 *   wrong Header.DataHash. Expected %X, got %X           (Txs.Hash, types/tx.go:34-39)
 *   wrong Header.EvidenceHash. Expected %X, got %X       (EvidenceList.Hash)
 * The evidence items arrive encoded: their own ValidateBasic ("invalid
 * evidence (#%d): ...", between the last two checks) is the caller's business
 * and is not run here.  results[i] = 0 ok / 1 error, the text at
 * errs + i*err_stride (errs may be NULL).  hash_out / has_hash (may be NULL):
 * Header.Hash of each header as given, which is Block.Hash() of every block
 * that passes (fillHeader changes nothing there).  A window on the device
 * takes one launch per kind of hash; commits that fail Commit.ValidateBasic are
 * not hashed.  Returns the number of failed blocks, or < 0. */
int tmv_blocks_validate_basic(tmv_ctx *ctx, const tmv_block *blocks, uint32_t n, int32_t *results, char *errs,
                              size_t err_stride, uint8_t *hash_out, uint8_t *has_hash);

/* ---- blocks from their protobuf bytes ---- */
/* A blocksync peer delivers a block as bytes (bcproto.BlockResponse) and the
 * block store keeps it as bytes; almost everything Block.ValidateBasic hashes
 * sits in them verbatim.  tmv_blocks_validate_wire validates a window of
 * blocks from the bytes: data[block_off[i], block_off[i+1]) is the
 * tendermint.types.Block message of block i (n + 1 offsets, block_off[0] = 0,
 * never decreasing).
 *
 * The contract.  Hashing received bytes equals the reference's
 * decode-then-re-encode only for bytes its own Marshal would write, so the
 * scanner (csrc/host/block_wire.h) accepts exactly the canonical gogoproto
 * encoding -- ascending field numbers, declared wire types, no unknown
 * fields, minimal varints, sign-extended int32s, no present zero values, the
 * nullable = false messages present, lengths inside their parent, timestamps
 * in the reference's domain -- which is what every Go node writes.  Everything
 * else is TMV_WIRE_NOT_HANDLED with the first problem in byte order in
 * reason[i]: the caller decodes that block with the reference and uses
 * tmv_blocks_validate_basic.  No verdict is ever given on bytes the scanner
 * did not fully recognise.  Also not handled, on purpose: a non-empty evidence
 * list (EVIDENCE) and a chain_id with a NUL or a byte >= 0x80 (CHAIN_ID);
 * LIMIT: a value the view structs cannot hold (a block_id_flag above 255).
 *
 * Handled blocks: results[i], the text at errs + i*err_stride, hash_out and
 * has_hash are exactly what tmv_blocks_validate_basic returns for the block's
 * view -- same order, same strings.  (The reference's BlockFromProto runs the
 * header's and the commit's ValidateBasic before Block.ValidateBasic: pass or
 * fail is the same, which text comes first may differ.  This call reports
 * Block.ValidateBasic's, which is what validateBlock reports.)  hash_out /
 * has_hash may be NULL; a block that is not handled has has_hash[i] = 0, an
 * empty text and zeroed hash.
 *
 * A call with at least $TMV_DEVICE_BLOCK_MIN handled blocks (default 32) makes
 * one tmv_merkle_span_roots call over the caller's bytes (a weak reference):
 * one upload, one leaf launch and one tree launch for every Commit.Hash,
 * Data.Hash and Header.Hash of the window.  Smaller calls, and a build without
 * the engine, hash the views with the host code of tmv_blocks_validate_basic.
 * A commit that fails Commit.ValidateBasic is not hashed.  A block holding a
 * transaction longer than $TMV_DEVICE_WIRE_MAX_TX bytes (default 1024, as
 * $TMV_DEVICE_RESULTS_MAX_DATA; read on every call) has its Data.Hash computed
 * on the host inside a device call: one lane hashes one leaf.
 *
 * part_size != 0: psh_total_out[i] / psh_hash_out + 32*i =
 * NewPartSetFromData(block i's bytes, part_size).Header() of every block,
 * handled or not, through tmv_part_set_headers under its own device rule.
 * part_size == 0: psh_* are not written and may be NULL.
 *
 * views_out (may be NULL): the views, to be freed with tmv_block_views_free;
 * they point into `data`, which must outlive them.
 * tmv_block_views_block(v, i)->last_commit can go straight into a
 * tmv_commit_job.  Returns the number of blocks that are not TMV_WIRE_OK, or
 * < 0 (then *views_out is NULL). */
#define TMV_WIRE_OK 0          /* Block.ValidateBasic passes */
#define TMV_WIRE_INVALID 1     /* it fails: text at errs + i*err_stride */
#define TMV_WIRE_NOT_HANDLED 2 /* reason[i] = TMV_WIRE_REASON_*: decode with the reference, use tmv_blocks_validate_basic */

#define TMV_WIRE_REASON_NONE 0
#define TMV_WIRE_REASON_TRUNCATED 1     /* a tag, varint or length runs past its enclosing message */
#define TMV_WIRE_REASON_WIRE_TYPE 2     /* a known field with another wire type */
#define TMV_WIRE_REASON_UNKNOWN_FIELD 3
#define TMV_WIRE_REASON_ORDER 4         /* field numbers not ascending, or a scalar twice */
#define TMV_WIRE_REASON_VARINT 5        /* padded, longer than 10 bytes, beyond 64 bits, or outside its 32-bit type */
#define TMV_WIRE_REASON_ZERO_PRESENT 6  /* a zero scalar, empty bytes or empty string that is present */
#define TMV_WIRE_REASON_MISSING 7       /* a nullable = false message is absent */
#define TMV_WIRE_REASON_TIME 8          /* a timestamp outside the reference's domain */
#define TMV_WIRE_REASON_EVIDENCE 9      /* a non-empty evidence list */
#define TMV_WIRE_REASON_CHAIN_ID 10     /* a chain_id with a NUL or a byte >= 0x80 */
#define TMV_WIRE_REASON_LIMIT 11        /* a value the view structs cannot hold */

typedef struct tmv_block_views tmv_block_views;

int tmv_blocks_validate_wire(tmv_ctx *ctx, const uint8_t *data, const uint32_t *block_off, uint32_t n,
                             uint32_t part_size /* 0: no part-set headers */,
                             int32_t *results, int32_t *reason, char *errs, size_t err_stride,
                             uint8_t *hash_out, uint8_t *has_hash,
                             uint32_t *psh_total_out, uint8_t *psh_hash_out,
                             tmv_block_views **views_out /* may be NULL */);
/* The scanner alone: reason[i] (may be NULL) and the views of n blocks.
 * Returns the number of blocks that were not handled, or < 0. */
int tmv_blocks_parse_wire(const uint8_t *data, const uint32_t *block_off, uint32_t n, int32_t *reason,
                          tmv_block_views **out);
const tmv_block *tmv_block_views_block(const tmv_block_views *v, uint32_t i); /* NULL for a block that was not handled */
void tmv_block_views_free(tmv_block_views *v);

/* ---- light blocks from their protobuf bytes (types/light.go) ---- */
/* Statesync's backfill fetches one tendermint.types.LightBlock per height from
 * peers (internal/statesync/reactor.go:437-600) and the light store keeps
 * LightBlocks as marshalled protobuf (light/store/db/db.go); what
 * LightBlock.ValidateBasic hashes -- Header.Hash and ValidatorSet.Hash -- sits
 * in those bytes.  tmv_light_blocks_validate_wire validates a window of light
 * blocks from the bytes: data[block_off[i], block_off[i+1]) is the LightBlock
 * message of block i (n + 1 offsets, block_off[0] = 0, never decreasing).
 *
 * The contract is tmv_blocks_validate_wire's, extended to LightBlock
 * {signed_header = 1, validator_set = 2}, SignedHeader{header = 1, commit = 2},
 * ValidatorSet{validators = 1 repeated, proposer = 2, total_voting_power = 3},
 * Validator{address = 1, pub_key = 2 (nullable = false), voting_power = 3,
 * proposer_priority = 4} and crypto.PublicKey{ed25519 = 1 | secp256k1 = 2 |
 * sr25519 = 3}.  The scanner (csrc/host/light_wire.h) accepts the canonical
 * encoding only, by block_wire.h's rules with one difference: a oneof member
 * is written even when empty, so the zero-absent rule does not apply inside
 * PublicKey.  The message fields are pointers in the reference: absent is nil,
 * present with length 0 is non-nil and empty, and the views keep that apart.
 * Everything else is TMV_WIRE_NOT_HANDLED with the first problem in byte order
 * in reason[i], and so is everything for which LightBlockFromProto
 * (types/light.go:104-128) fails for a reason that is no ValidateBasic failure,
 * or panics:
 *   KEY       a PublicKey whose oneof is unset, or whose key is not 32 / 33 /
 *             32 bytes (crypto/encoding/codec.go:49-78)
 *   PROPOSER  validator_set present without proposer (ValidatorFromProto(nil)),
 *             or a proposer whose message bytes equal no entry of a non-empty
 *             `validators` (the views carry its index; an empty set has none)
 *   POWER     the clipped running sum of the voting powers exceeds
 *             MaxTotalVotingPower (types/validator_set.go:295-309 panics)
 * total_voting_power is scanned and dropped, as ValidatorSetFromProto drops it.
 *
 * Handled blocks: results[i] and the text at errs + i*err_stride are
 * LightBlock.ValidateBasic(chain_id) (types/light.go:37-60), byte for byte:
 * "missing signed header", "missing validator set", "invalid signed header: "
 * + SignedHeader.ValidateBasic, "invalid validator set: " +
 * ValidatorSet.ValidateBasic (types/validator_set.go:82-98), "expected
 * validator hash of header to match validator set hash (%X != %X)".
 * hash_out + 32*i: Header.Hash(), which backfill compares with the trusted
 * LastBlockID.Hash; has_hash[i] bit 0 set when the header has one (a header is
 * present and its ValidatorsHash is not empty).  vals_hash_out + 32*i:
 * ValidatorSet.Hash(); has_hash[i] bit 1 set when it was computed (the set is
 * present and not empty).  All three may be NULL.  Commit.Hash is not part of
 * LightBlock.ValidateBasic and is not computed.
 *
 * A call with at least $TMV_DEVICE_HASH_MIN handled light blocks (the light
 * client's knob, default 32; read on every call) makes one
 * tmv_merkle_wire_roots call over the caller's bytes (a weak reference): one
 * upload and one tree launch for every Header.Hash and every ValidatorSet.Hash
 * of the window, whatever the key types.  Smaller calls, calls above the
 * engine's limits and a build without the engine hash the views on the host --
 * a re-encoding of what the scanner decoded.
 *
 * views_out (may be NULL): the views, freed with tmv_light_block_views_free;
 * they point into `data`, which must outlive them.  The two accessors go
 * straight into a tmv_light_job; both return NULL for a block that was not
 * handled and for a nil signed header / validator set; a nil header or commit
 * inside the tmv_signed_header is NULL.  Returns the number of blocks that are
 * not TMV_WIRE_OK, or < 0 (then *views_out is NULL). */
#define TMV_WIRE_REASON_KEY 12      /* a PublicKey with no oneof member, or a key of the wrong size */
#define TMV_WIRE_REASON_PROPOSER 13 /* a validator set without proposer, or a proposer that is none of its validators */
#define TMV_WIRE_REASON_POWER 14    /* the total voting power exceeds MaxTotalVotingPower */

typedef struct tmv_light_block_views tmv_light_block_views;

int tmv_light_blocks_validate_wire(tmv_ctx *ctx, const char *chain_id, const uint8_t *data,
                                   const uint32_t *block_off, uint32_t n, int32_t *results, int32_t *reason,
                                   char *errs, size_t err_stride, uint8_t *hash_out, uint8_t *has_hash,
                                   uint8_t *vals_hash_out, tmv_light_block_views **views_out /* may be NULL */);
/* The scanner alone: reason[i] (may be NULL) and the views of n light blocks.
 * Returns the number of blocks that were not handled, or < 0. */
int tmv_light_blocks_parse_wire(const uint8_t *data, const uint32_t *block_off, uint32_t n, int32_t *reason,
                                tmv_light_block_views **out);
const tmv_signed_header *tmv_light_block_views_header(const tmv_light_block_views *v, uint32_t i);
const tmv_validator_set *tmv_light_block_views_vals(const tmv_light_block_views *v, uint32_t i);
void tmv_light_block_views_free(tmv_light_block_views *v);

/* ---- ABCI results and consensus params (abci/types/types.go, types/params.go) ---- */
/* Calls with at least $TMV_DEVICE_RESULTS_MIN results (default 4096; DESIGN.md
 * section 21) hash on the device in one tmv_tx_results_hashes call (a weak
 * reference); smaller calls, and a build without the engine, encode and hash
 * on the host worker pool.  Of a call that goes to the device, a tree holding
 * a result whose data exceeds $TMV_DEVICE_RESULTS_MAX_DATA bytes (default
 * 1024: one lane would hash it alone while the call waits, and from 4 KiB on
 * that was measured slower) is still hashed on the host.  Both knobs are read on every call;
 * the hashes, verdicts and texts are the same either way. */

/* The deterministic fields of abci.ExecTxResult (abci/types/types.go:213-222). */
typedef struct {
  uint32_t code;
  tmv_bytes data;
  int64_t gas_wanted, gas_used;
} tmv_tx_result;

/* merkle.HashFromByteSlices over abci.MarshalTxResults(results[i]) for n lists
 * of n_results[i] results each (results[i] may be NULL when n_results[i] is 0).
 * first == NULL: no leading leaf, State.LastResultsHash as ApplyBlock stores it
 * (internal/state/execution.go:262-267).  Else first[i] (may be empty) is
 * hashed as a leaf in front of list i's results, as the light client's
 * BlockResults does with proto.Marshal(ResponseFinalizeBlock{Events})
 * (light/rpc/client.go:452-464).  hash_out: n x 32.  0 or < 0. */
int tmv_results_hash_many(tmv_ctx *ctx, const tmv_tx_result *const *results, const uint32_t *n_results,
                          const tmv_bytes *first, uint32_t n, uint8_t *hash_out);

/* ConsensusParams.HashConsensusParams (types/params.go:385-399): SHA-256 of
 * tmproto.HashedParams, [08 varint(block_max_bytes)] [10 varint(block_max_gas)]
 * with zero fields omitted (max_gas = -1, the common case, takes 10 bytes).
 * One hash, on the host.  0 or TMV_ERR_ARG (out == NULL). */
int tmv_consensus_params_hash(int64_t block_max_bytes, int64_t block_max_gas, uint8_t out[32]);

/* One BlockResults response with the trusted header it is checked against. */
typedef struct {
  int64_t height;                /* ResultBlockResults.Height */
  const tmv_tx_result *results;  /* TxsResults */
  uint32_t n_results;
  tmv_bytes events;              /* proto.Marshal(ResponseFinalizeBlock{Events: FinalizeBlockEvents}) */
  tmv_bytes last_results_hash;   /* LastResultsHash of the trusted header at height + 1 */
} tmv_block_results_in;

/* The checks of the light client's BlockResults after the fetch
 * (light/rpc/client.go:439-470) for n responses, in its order:
 *   height must be greater than zero                     (rpc/coretypes/responses.go:20)
 *   last results %X does not match with trusted last results %X
 * Items that fail the first check are not hashed.  Results, text layout and
 * return value as tmv_proof_ops_verify. */
int tmv_block_results_verify(tmv_ctx *ctx, const tmv_block_results_in *items, uint32_t n, int32_t *results,
                             char *errs, size_t err_stride);

/* One ConsensusParams response with the trusted header's ConsensusHash. */
typedef struct {
  int64_t height;                         /* ResultConsensusParams.BlockHeight */
  int64_t block_max_bytes, block_max_gas; /* ConsensusParams.Block */
  tmv_bytes consensus_hash;               /* ConsensusHash of the trusted header at that height */
} tmv_consensus_params_in;

/* The last two checks of the light client's ConsensusParams
 * (light/rpc/client.go:274-288) for n responses:
 *   height must be greater than zero
 *   params hash %X does not match trusted hash %X
 * ValidateConsensusParams, which runs before them, stays with the caller.
 * ctx is unused (every hash is one block, computed on the host).  Results,
 * text layout and return value as tmv_proof_ops_verify. */
int tmv_consensus_params_verify(tmv_ctx *ctx, const tmv_consensus_params_in *items, uint32_t n, int32_t *results,
                                char *errs, size_t err_stride);

/* ---- validator-set updates (types/validator_set.go:70-234, 362-650) ---- */
/* What State.Update (internal/state/execution.go:527-595) does to
 * NextValidators once per block, on the host and on one thread (DESIGN.md
 * section 24): no engine, no context.  The calls return TMV_VALSET_OK,
 * TMV_VALSET_ERROR (the reference returns an error; its text in err),
 * TMV_VALSET_PANIC (the reference panics; the panic's text in err) or
 * TMV_ERR_ARG.  On anything but TMV_VALSET_OK the outputs are not written. */
#define TMV_VALSET_OK 0
#define TMV_VALSET_ERROR 1
#define TMV_VALSET_PANIC 2

/* One abci.ValidatorUpdate: the key and the new power (0 removes). */
typedef struct {
  uint8_t key_kind;
  const uint8_t *pub_key;
  uint32_t pub_key_len;
  int64_t power;
} tmv_validator_update;

/* ValidatorSet.UpdateWithChangeSet (allow_deletes != 0) of the set vals[0,
 * n_vals) with `changes`.  The address of a change is derived from its key as
 * NewValidator does (SHA-256 truncated to 20 bytes for ed25519 and sr25519,
 * RIPEMD160(SHA256(key)) for secp256k1) into addr_scratch + 20 * i
 * (20 * n_changes bytes, the caller's).  out[0, *n_out) is the new set in set
 * order (power descending, address ascending), out_cap >= n_vals + n_changes.
 * Its entries borrow their pointers: key and address of `vals` for a
 * validator that stays, the key of `changes` and the address in addr_scratch
 * for one that was added or changed; all three must outlive `out`. */
int tmv_validator_set_update(const tmv_validator *vals, uint32_t n_vals, const tmv_validator_update *changes,
                             uint32_t n_changes, int allow_deletes, uint8_t *addr_scratch, tmv_validator *out,
                             uint32_t out_cap, uint32_t *n_out, char *err, size_t err_cap);

/* NewValidatorSet(vals): the change set over an empty set with removals
 * refused, then one IncrementProposerPriority(1) when the set is not empty;
 * *proposer_index is that election's winner (-1 for an empty set).  The
 * reference panics where the change set fails ("cannot create validator set:
 * ...").  Pointers as tmv_validator_set_update, out_cap >= n_vals. */
int tmv_validator_set_new(const tmv_validator_update *vals, uint32_t n_vals, uint8_t *addr_scratch, tmv_validator *out,
                          uint32_t out_cap, uint32_t *n_out, int32_t *proposer_index, char *err, size_t err_cap);

/* `steps` successive IncrementProposerPriority(times) calls on the set, as
 * State.Update makes one per block with times = 1: the priorities of vals are
 * updated in place and proposer_out[s] is the proposer's index after call s.
 * One call with times = k differs from k calls with times = 1: the reference
 * rescales and centres the priorities once per call. */
int tmv_validator_set_rotate(tmv_validator *vals, uint32_t n_vals, int32_t times, uint32_t steps,
                             int32_t *proposer_out, char *err, size_t err_cap);

/* ValidatorSet.Hash of one set on the host: for the sets that hold secp256k1
 * keys, which tmv_validator_set_hashes (tmverify.h) does not take.  0 or
 * TMV_ERR_ARG. */
int tmv_validator_set_hash_host(const tmv_validator *vals, uint32_t n_vals, uint8_t out[32]);

#ifdef __cplusplus
}
#endif
#endif /* TMHOST_H */
