// Merkle roots over spans of one uploaded buffer (tmv_merkle_span_roots,
// include/tmverify.h): what Block.ValidateBasic hashes sits in the block's
// protobuf bytes verbatim -- a Commit.Hash leaf is the payload of one
// `signatures` entry, a Data.Hash leaf SHA-256 of a `txs` entry, a Header.Hash
// leaf a header field's payload behind at most one wrapper tag -- so a window
// of received blocks is hashed from a table of (pos, len, flags) with no
// column packed on the host.
//
//   k_span_leaves   one lane per leaf, whatever its length: a transaction of
//                   many KiB keeps its wave busy while the others wait, as a
//                   long result does in k_result_leaves (the host layer keeps
//                   such blocks' Data.Hash on the host).
//   k_merkle_tree   (merkle_kernels.hip) the levels of each tree.
//
// The hashed message of a leaf:
//   00            leaf prefix      (absent in the inner hash of a PREHASH leaf)
//   tag           with TMV_SPAN_TAG: the low 8 bits of flags
//   data[pos, pos + len)
// and a PREHASH leaf is SHA-256(00 || SHA-256(span)) (Txs.Hash, types/tx.go:34-39):
// the inner digest stays in registers and the outer hash is one more block.
// A message word inside the span is two aligned dword loads and a byte
// alignment; a word that touches the prefix, the tag or the padding is put
// together byte by byte (the technique of results_kernels.hip).  The aligned
// loads reach at most 3 bytes behind the data, inside the staged copy's
// padding.  No array is indexed at run time, so nothing goes to scratch, and
// there is no LDS and no barrier.
#include <hip/hip_runtime.h>
#include "block_wire_hash.h"
#include "ktimer.h"
#include "sha256_dev.h"
#include "valset.h"

namespace tmv {

namespace {

constexpr int kSpanBlock = 256;

}  // namespace

__global__ void __launch_bounds__(kSpanBlock)
k_span_leaves(const uint8_t *__restrict__ data, const tmv_leaf_span *__restrict__ leaves, uint32_t n_leaves,
              uint32_t *__restrict__ node) {
  const uint32_t i = blockIdx.x * kSpanBlock + threadIdx.x;
  if (i >= n_leaves) return;
  const uint32_t *lw = reinterpret_cast<const uint32_t *>(leaves) + 3ull * i;
  const uint32_t base = lw[0], len = lw[1], flags = lw[2];
  const bool prehash = flags & TMV_SPAN_PREHASH;
  // the bytes in front of the span, first byte lowest: nothing (inner hash), 00, or 00 tag
  const uint32_t head = (flags & TMV_SPAN_TAG) ? (flags & 0xffu) << 8 : 0;
  const uint32_t dlo = prehash ? 0 : ((flags & TMV_SPAN_TAG) ? 2 : 1);
  const uint32_t dhi = dlo + len;           // <= 2 + 2^30
  const uint32_t nblk = (dhi + 72) / 64;    // room for 0x80 and the 8-byte length
  const uint32_t end = 64 * nblk;
  const uint64_t bits = (uint64_t)dhi * 8;
  const uint32_t *dw = reinterpret_cast<const uint32_t *>(data);

  uint32_t st[8];
  sha256_init(st);
  for (uint32_t k = 0; k < nblk; k++) {
    uint32_t w[16];
#pragma unroll
    for (int q = 0; q < 16; q++) {
      const uint32_t p0 = 64 * k + 4 * q;
      uint32_t word = 0;
      if (p0 >= dlo && p0 + 4 <= dhi) {  // four span bytes: two aligned dwords, aligned by the address
        const uint32_t a = base + (p0 - dlo);
        const uint32_t sh = a & 3;
        const uint32_t l = dw[a >> 2];
        const uint32_t h = sh ? dw[(a >> 2) + 1] : 0;  // sh != 0: that dword still holds a byte of this span
        word = __builtin_bswap32(__builtin_amdgcn_alignbyte(h, l, sh));
      } else {
#pragma unroll
        for (int j = 0; j < 4; j++) {
          const uint32_t pos = p0 + j;
          uint32_t b = 0;
          if (pos < dlo) b = (head >> (8 * pos)) & 0xffu;
          else if (pos < dhi) b = data[base + (pos - dlo)];
          else if (pos == dhi) b = 0x80;
          else if (pos >= end - 8) b = (uint32_t)(bits >> (8 * (end - 1 - pos))) & 0xffu;
          word = (word << 8) | b;
        }
      }
      w[q] = word;
    }
    sha256_compress(st, w);
  }
  if (prehash) {  // 00 || the 32-byte digest: one block of 33 bytes
    uint32_t w[16];
    w[0] = st[0] >> 8;
    w[1] = (st[0] << 24) | (st[1] >> 8);
    w[2] = (st[1] << 24) | (st[2] >> 8);
    w[3] = (st[2] << 24) | (st[3] >> 8);
    w[4] = (st[3] << 24) | (st[4] >> 8);
    w[5] = (st[4] << 24) | (st[5] >> 8);
    w[6] = (st[5] << 24) | (st[6] >> 8);
    w[7] = (st[6] << 24) | (st[7] >> 8);
    w[8] = (st[7] << 24) | 0x00800000u;
    w[9] = w[10] = w[11] = w[12] = w[13] = w[14] = 0;
    w[15] = 33 * 8;
    sha256_init(st);
    sha256_compress(st, w);
  }
  uint4 *o = reinterpret_cast<uint4 *>(node + 8ull * i);
  o[0] = make_uint4(st[0], st[1], st[2], st[3]);
  o[1] = make_uint4(st[4], st[5], st[6], st[7]);
}

hipError_t launch_span_leaves(const uint8_t *data, const tmv_leaf_span *leaves, uint32_t n_leaves, uint32_t *node,
                              hipStream_t stream) {
  if (!n_leaves) return hipSuccess;
  void *tok = ktimer::begin(ktimer::kSpanLeaves, stream);
  hipLaunchKernelGGL(k_span_leaves, dim3((n_leaves + kSpanBlock - 1) / kSpanBlock), dim3(kSpanBlock), 0, stream,
                     data, leaves, n_leaves, node);
  ktimer::end(tok, stream);
  return hipGetLastError();
}

hipError_t launch_span_roots(const uint8_t *data, const tmv_leaf_span *leaves, uint32_t n_leaves,
                             const uint32_t *tree_off, uint32_t n_trees, uint32_t max_leaves, uint32_t *node_a,
                             uint32_t *node_b, uint8_t *out, hipStream_t stream) {
  const hipError_t e = launch_span_leaves(data, leaves, n_leaves, node_a, stream);
  if (e != hipSuccess) return e;
  return launch_merkle_tree(tree_off, n_trees, max_leaves, node_a, node_b, out, stream);
}

}  // namespace tmv
