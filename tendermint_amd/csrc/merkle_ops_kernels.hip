// Chained value proof operators on the device: ValueOp.Run
// (crypto/merkle/proof_value.go:77-98) as ProofOperators.Verify chains it
// (proof_op.go:39-69), for many items per launch -- what the light client's
// ABCIQueryWithOptions runs against a trusted header's AppHash
// (light/rpc/client.go:148-217).
//
//   k_merkle_value_ops   one lane per item, a loop over the item's ops.  Op j
//                        hashes the KV leaf
//                          SHA-256(0x00 || uvarint(len key) || key || 0x20 || v)
//                        where v is SHA-256(value) for the first op (from
//                        k_merkle_digests_long, merkle_proof_kernels.hip) and
//                        SHA-256(previous op's root) after it, compares it
//                        with the op's Proof.LeafHash and folds the aunts from
//                        the *given* leaf hash (computeHashFromAunts,
//                        proof.go:151-181, the loop of k_merkle_verify_proofs).
//                        The message length depends on the key, so the lane
//                        builds each 64-byte block in LDS, transposed as
//                        k_commit_leaves keeps its message (word k of lane l at
//                        buf[k * 256 + l]: 16 KiB per block, conflict-free, and
//                        no barrier since a lane reads only what it wrote): a
//                        register array indexed at run time would go to
//                        scratch.  Bytes go in with byte stores; the block is
//                        read back as 16 words and compressed at one call site.
// Hashes are serialised big-endian, as in merkle_proof_kernels.hip.
#include <hip/hip_runtime.h>
#include "ktimer.h"
#include "merkle_ops.h"
#include "sha256_dev.h"

namespace tmv {

namespace {

constexpr int kOpsBlock = 256;

__device__ __forceinline__ void ops_load_hash(uint32_t h[8], const uint8_t *p) {  // 16-byte aligned
  const uint4 *q = reinterpret_cast<const uint4 *>(p);
  const uint4 a = q[0], b = q[1];
  h[0] = a.x; h[1] = a.y; h[2] = a.z; h[3] = a.w;
  h[4] = b.x; h[5] = b.y; h[6] = b.z; h[7] = b.w;
#pragma unroll
  for (int i = 0; i < 8; i++) h[i] = __builtin_bswap32(h[i]);
}

__device__ __forceinline__ void ops_store_hash(uint8_t *p, const uint32_t h[8]) {
  uint4 *q = reinterpret_cast<uint4 *>(p);
  q[0] = make_uint4(__builtin_bswap32(h[0]), __builtin_bswap32(h[1]), __builtin_bswap32(h[2]), __builtin_bswap32(h[3]));
  q[1] = make_uint4(__builtin_bswap32(h[4]), __builtin_bswap32(h[5]), __builtin_bswap32(h[6]), __builtin_bswap32(h[7]));
}

}  // namespace

// vdig: 8 state words of SHA-256(value) per item.  Per-op outputs: kv_out and
// rootc_out n_ops x 32 (16-byte aligned), leaf_ok_out and nil_out n_ops; per
// item: status_out, fail_op_out (include/tmverify.h, tmv_merkle_value_ops).
__global__ void __launch_bounds__(kOpsBlock)
k_merkle_value_ops(uint32_t n_items, const uint32_t *__restrict__ op_off, const uint32_t *vdig,
                   const uint8_t *__restrict__ key, const uint32_t *__restrict__ key_off,
                   const int64_t *__restrict__ total, const int64_t *__restrict__ index,
                   const uint8_t *__restrict__ leaf_hash, const uint8_t *__restrict__ aunts,
                   const uint32_t *__restrict__ aunt_off, const uint8_t *__restrict__ root,
                   uint8_t *__restrict__ kv_out, uint8_t *__restrict__ leaf_ok_out, uint8_t *__restrict__ rootc_out,
                   uint8_t *__restrict__ nil_out, int8_t *__restrict__ status_out, int32_t *__restrict__ fail_op_out) {
  __shared__ uint32_t buf[16 * kOpsBlock];
  const uint32_t lane = threadIdx.x;
  const uint32_t i = blockIdx.x * kOpsBlock + lane;
  if (i >= n_items) return;  // no barrier below
  uint32_t *mine = buf + lane;                                  // word k at mine[k * kOpsBlock]
  uint8_t *mine8 = reinterpret_cast<uint8_t *>(buf) + 4 * lane;  // message byte b of the block: big-endian inside its word
  auto put = [&](uint32_t b, uint32_t v) { mine8[(b >> 2) * (4 * kOpsBlock) + (3 - (b & 3))] = (uint8_t)v; };

  uint32_t v[8];  // the op's input, hashed: SHA-256(value), later SHA-256(root of the op before)
  {
    const uint4 *q = reinterpret_cast<const uint4 *>(vdig + 8ull * i);
    const uint4 a = q[0], b = q[1];
    v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
    v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
  }
  const uint32_t o0 = op_off[i], o1 = op_off[i + 1];
  int32_t first_bad = -1;
  bool last_nil = true;
  uint32_t h[8];  // the last op's root
#pragma unroll
  for (int k = 0; k < 8; k++) h[k] = 0;
  for (uint32_t op = o0; op < o1; op++) {
    // ---- the KV leaf: 0x00 || uvarint(klen) || key || 0x20 || v
    const uint32_t k0 = key_off[op], klen = key_off[op + 1] - k0;
    const uint32_t nv = klen < (1u << 7) ? 1 : klen < (1u << 14) ? 2 : klen < (1u << 21) ? 3 : klen < (1u << 28) ? 4 : 5;
    const uint32_t kp = 1 + nv;          // the key's first byte in the message
    const uint32_t tp = kp + klen;       // the tail's: 0x20 and the 32 digest bytes
    const uint32_t len = tp + 33;        // < 2^31: keys are at most 2^30 bytes
    const uint32_t nblk = (len + 72) / 64;
    uint32_t st[8];
    sha256_init(st);
    for (uint32_t blk = 0; blk < nblk; blk++) {
      const uint32_t lo = 64 * blk;
#pragma unroll
      for (int k = 0; k < 16; k++) mine[k * kOpsBlock] = 0;
      if (blk == 0) {  // mine[0]'s top byte is the 0x00 prefix already
#pragma unroll
        for (int q = 0; q < 5; q++)
          if ((uint32_t)q < nv) put(1 + q, ((klen >> (7 * q)) & 0x7f) | ((uint32_t)q + 1 < nv ? 0x80 : 0));
      }
      // the key bytes of this block: message positions [max(kp, lo), min(tp, lo + 64))
      const uint32_t ka = kp > lo ? kp : lo, kb = tp < lo + 64 ? tp : lo + 64;
      for (uint32_t p = ka; p < kb; p++) put(p - lo, key[k0 + (p - kp)]);
#pragma unroll
      for (int q = 0; q < 33; q++) {
        const uint32_t p = tp + q;
        const uint32_t byte = q == 0 ? 0x20u : (v[(q - 1) >> 2] >> (24 - 8 * ((q - 1) & 3))) & 0xffu;
        if ((p >> 6) == blk) put(p & 63, byte);
      }
      if ((len >> 6) == blk) put(len & 63, 0x80);
      if (blk + 1 == nblk) {  // the bit length
        mine[14 * kOpsBlock] = len >> 29;
        mine[15 * kOpsBlock] = len << 3;
      }
      uint32_t w[16];
#pragma unroll
      for (int k = 0; k < 16; k++) w[k] = mine[k * kOpsBlock];
      sha256_compress(st, w);
    }
    // ---- against the given leaf hash
    ops_load_hash(h, leaf_hash + 32ull * op);
    bool leaf_ok = true;
#pragma unroll
    for (int k = 0; k < 8; k++) leaf_ok = leaf_ok && st[k] == h[k];
    ops_store_hash(kv_out + 32ull * op, st);
    leaf_ok_out[op] = leaf_ok ? 1 : 0;
    if (!leaf_ok && first_bad < 0) first_bad = (int32_t)(op - o0);
    // ---- the root from the given leaf hash: down from (index, total), then the aunts folded upwards
    const int64_t tot = total[op], idx = index[op];
    const uint32_t a0 = aunt_off[op], na = aunt_off[op + 1] - a0;
    bool nil = !(idx >= 0 && idx < tot);
    uint32_t depth = 0;
    uint64_t mask = 0;
    if (!nil) {
      uint64_t t = (uint64_t)tot, x = (uint64_t)idx;
      while (t > 1) {  // at most 63 levels
        const uint64_t k = 1ull << (63 - __clzll((long long)(t - 1)));  // largest power of two < t
        if (x < k) {
          t = k;
        } else {
          mask |= 1ull << depth;
          x -= k;
          t -= k;
        }
        depth++;
      }
      nil = depth != na;
    }
    if (!nil) {
      for (uint32_t j = 0; j < depth; j++) {
        uint32_t a[8], o[8];
        ops_load_hash(a, aunts + 32ull * (a0 + j));
        if ((mask >> (depth - 1 - j)) & 1) sha256_inner(o, a, h);
        else sha256_inner(o, h, a);
#pragma unroll
        for (int k = 0; k < 8; k++) h[k] = o[k];
      }
    } else {
#pragma unroll
      for (int k = 0; k < 8; k++) h[k] = 0;
    }
    ops_store_hash(rootc_out + 32ull * op, h);
    nil_out[op] = nil ? 1 : 0;
    last_nil = nil;
    if (op + 1 < o1) {  // the next op's value is this root; a nil root is passed on as the empty string
      if (nil) {  // SHA-256("")
        v[0] = 0xe3b0c442u; v[1] = 0x98fc1c14u; v[2] = 0x9afbf4c8u; v[3] = 0x996fb924u;
        v[4] = 0x27ae41e4u; v[5] = 0x649b934cu; v[6] = 0xa495991bu; v[7] = 0x7852b855u;
      } else {  // SHA-256 of the 32 root bytes: one block
        uint32_t w[16];
#pragma unroll
        for (int k = 0; k < 8; k++) w[k] = h[k];
        w[8] = 0x80000000u;
#pragma unroll
        for (int k = 9; k < 15; k++) w[k] = 0;
        w[15] = 32 * 8;
        sha256_init(v);
        sha256_compress(v, w);
      }
    }
  }
  uint32_t want[8];
  ops_load_hash(want, root + 32ull * i);
  bool root_ok = !last_nil;
#pragma unroll
  for (int k = 0; k < 8; k++) root_ok = root_ok && want[k] == h[k];
  status_out[i] = first_bad >= 0 ? 3 : !root_ok ? 4 : 0;
  fail_op_out[i] = first_bad >= 0 ? first_bad : !root_ok ? (int32_t)(o1 - o0) - 1 : 0;
}

hipError_t launch_merkle_value_ops(uint32_t n_items, const uint32_t *op_off, const uint32_t *vdig, const uint8_t *key,
                                   const uint32_t *key_off, const int64_t *total, const int64_t *index,
                                   const uint8_t *leaf_hash, const uint8_t *aunts, const uint32_t *aunt_off,
                                   const uint8_t *root, uint8_t *kv_out, uint8_t *leaf_ok_out, uint8_t *rootc_out,
                                   uint8_t *nil_out, int8_t *status_out, int32_t *fail_op_out, hipStream_t stream) {
  if (!n_items) return hipSuccess;
  void *tok = ktimer::begin(ktimer::kMerkleValueOps, stream);
  hipLaunchKernelGGL(k_merkle_value_ops, dim3((n_items + kOpsBlock - 1) / kOpsBlock), dim3(kOpsBlock), 0, stream,
                     n_items, op_off, vdig, key, key_off, total, index, leaf_hash, aunts, aunt_off, root, kv_out,
                     leaf_ok_out, rootc_out, nil_out, status_out, fail_op_out);
  ktimer::end(tok, stream);
  return hipGetLastError();
}

}  // namespace tmv
