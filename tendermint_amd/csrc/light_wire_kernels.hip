// ValidatorSet.Hash leaves from the protobuf bytes of a light block
// (tmv_merkle_wire_roots, include/tmverify.h).  A leaf of ValidatorSet.Hash is
// SimpleValidator{pub_key = 1, voting_power = 2} (types/validator.go:154-170),
// and in the canonical encoding of Validator{address = 1, pub_key = 2,
// voting_power = 3, proposer_priority = 4} those two fields lie next to each
// other: 12 LL <PublicKey> [18 <varint>].  SimpleValidator's bytes are those
// bytes with the two tags replaced, 12 -> 0a and 18 -> 10; the PublicKey
// payload is verbatim for every key type.  So a leaf is hashed from one span
// (pos, len, power_at) of the uploaded buffer with two byte substitutions, and
// the kernel never interprets the rest.
//
//   k_valset_span_leaves   one lane per validator.  The message 00 || span is
//                          3 .. 55 bytes: always one SHA-256 block.
//
// The span's dwords are loaded aligned and shifted to the lane's own byte
// alignment (alignbyte), as k_span_leaves does; the message word q is the
// span's big-endian words q - 1 and q shifted by the one prefix byte.  The two
// substitutions, the 0x80 and the cut at the message's end are compares of the
// byte's place against the unrolled word index.  An aligned load is issued
// only for a dword that holds a byte of the span, so it reaches at most 3
// bytes behind the data, inside the staged copy's padding.  No array is
// indexed at run time, so nothing goes to scratch, and there is no LDS and no
// barrier.
#include <hip/hip_runtime.h>
#include "ktimer.h"
#include "light_wire_hash.h"
#include "sha256_dev.h"
#include "valset.h"

namespace tmv {

namespace {

constexpr int kValSpanBlock = 256;
constexpr int kValSpanWords = 14;  // message words that can hold a byte of 00 || span or the 0x80: 55 + 1 bytes

}  // namespace

__global__ void __launch_bounds__(kValSpanBlock)
k_valset_span_leaves(const uint8_t *__restrict__ data, const tmv_val_span *__restrict__ vals, uint32_t n_vals,
                     uint32_t *__restrict__ node) {
  const uint32_t i = blockIdx.x * kValSpanBlock + threadIdx.x;
  if (i >= n_vals) return;
  const uint32_t *vw = reinterpret_cast<const uint32_t *>(vals) + 3ull * i;
  const uint32_t base = vw[0], len = vw[1], power_at = vw[2];
  const uint32_t mlen = len + 1;                                // 00 || span: 3 .. 55 bytes
  const uint32_t sub = power_at < len ? power_at + 1 : 0xffffu;  // the message byte that becomes 10, or none
  const uint32_t sh = base & 3;
  const uint32_t *dw = reinterpret_cast<const uint32_t *>(data) + (base >> 2);
  const uint32_t ndw = (sh + len + 3) >> 2;  // the dwords that hold a byte of the span: <= 15

  uint32_t d[kValSpanWords + 1];
#pragma unroll
  for (int k = 0; k <= kValSpanWords; k++) d[k] = (uint32_t)k < ndw ? dw[k] : 0;

  uint32_t w[16];
  uint32_t prev = 0;  // the span's big-endian word q - 1; in front of the span: the 00 prefix
#pragma unroll
  for (int q = 0; q < kValSpanWords; q++) {
    const uint32_t cur = __builtin_bswap32(__builtin_amdgcn_alignbyte(d[q + 1], d[q], sh));
    uint32_t word = (prev << 24) | (cur >> 8);  // message bytes 4q .. 4q + 3
    prev = cur;
    if (q == 0) word = (word & 0xff00ffffu) | 0x000a0000u;  // message byte 1, the span's byte 0: 12 -> 0a
    const uint32_t rs = sub - 4u * q;  // the place of the 10 in this word, if < 4
    if (rs < 4u) word = (word & ~(0xff000000u >> (8 * rs))) | (0x10000000u >> (8 * rs));
    const uint32_t re = mlen - 4u * q;  // message bytes from this word on; wraps to a large number behind the end
    if ((int32_t)re <= 0) word = 0;
    else if (re < 4u) word = (word & ~(0xffffffffu >> (8 * re))) | (0x80000000u >> (8 * re));
    if (re == 0) word = 0x80000000u;
    w[q] = word;
  }
  w[14] = 0;
  w[15] = mlen * 8;

  uint32_t st[8];
  sha256_init(st);
  sha256_compress(st, w);
  uint4 *o = reinterpret_cast<uint4 *>(node + 8ull * i);
  o[0] = make_uint4(st[0], st[1], st[2], st[3]);
  o[1] = make_uint4(st[4], st[5], st[6], st[7]);
}

hipError_t launch_wire_roots(const uint8_t *data, const tmv_leaf_span *leaves, uint32_t n_leaves,
                             const tmv_val_span *vals, uint32_t n_vals, const uint32_t *tree_off, uint32_t n_trees,
                             uint32_t max_leaves, uint32_t *node_a, uint32_t *node_b, uint8_t *out,
                             hipStream_t stream) {
  hipError_t e = launch_span_leaves(data, leaves, n_leaves, node_a, stream);
  if (e != hipSuccess) return e;
  if (n_vals) {
    void *tok = ktimer::begin(ktimer::kValsetSpanLeaves, stream);
    hipLaunchKernelGGL(k_valset_span_leaves, dim3((n_vals + kValSpanBlock - 1) / kValSpanBlock),
                       dim3(kValSpanBlock), 0, stream, data, vals, n_vals, node_a + 8ull * n_leaves);
    ktimer::end(tok, stream);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  return launch_merkle_tree(tree_off, n_trees, max_leaves, node_a, node_b, out, stream);
}

}  // namespace tmv
