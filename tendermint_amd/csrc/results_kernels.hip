// The hash of a block's ABCI results on the device: merkle.HashFromByteSlices
// over abci.MarshalTxResults (abci/types/types.go:213-239), which ApplyBlock
// stores as State.LastResultsHash (internal/state/execution.go:262-267) and
// the light client's BlockResults recomputes with one leading leaf
// (light/rpc/client.go:452-470).
//
//   k_result_leaves  one lane per result: encode the deterministic fields of
//                    ExecTxResult (abci/types/types.pb.go:3165-3170) behind
//                    the RFC 6962 leaf prefix and hash it.
//   k_merkle_tree    (merkle_kernels.hip) the levels of each tree.
//
// The encoded leaf, prefix included:
//   00                      leaf prefix
//   08 uvarint(code)        omitted when 0
//   12 uvarint(L) data[L]   omitted when empty
//   28 varint(gas_wanted)   omitted when 0; a negative value in the 10-byte
//   30 varint(gas_used)     two's-complement form
// The head (prefix, code, the data's tag and length: at most 13 bytes) and the
// two tail fields (at most 11 bytes each) are packed into 128-bit integers in
// registers, least significant byte first; the data between them is streamed
// from global memory.  A message word that lies inside the data is two aligned
// dword loads and a byte alignment; a word that touches the head, the tail or
// the padding is put together byte by byte from shifts by the byte position.
// No array is indexed at run time, so nothing goes to scratch, and there is no
// LDS and no barrier.
#include <hip/hip_runtime.h>
#include "ktimer.h"
#include "results_hash.h"
#include "sha256_dev.h"
#include "valset.h"

namespace tmv {

namespace {

constexpr int kResultsBlock = 256;
using u128 = unsigned __int128;

// tag || uvarint(u), least significant byte first; *len: its length (2 to 11).
__device__ __forceinline__ u128 tagged_varint(uint32_t tag, uint64_t u, uint32_t *len) {
  u128 p = tag;
  uint32_t n = 1;
  bool live = true;
#pragma unroll
  for (int i = 0; i < 10; i++) {
    const bool more = (u >> 7) != 0;
    const uint32_t b = (uint32_t)(u & 0x7f) | (more ? 0x80u : 0u);
    if (live) {
      p |= (u128)b << (8 * (i + 1));
      n++;
    }
    live = live && more;
    u >>= 7;
  }
  *len = n;
  return p;
}

__device__ __forceinline__ uint32_t byte_of(u128 x, uint32_t at) { return (uint32_t)(x >> (8 * at)) & 0xffu; }

}  // namespace

__global__ void __launch_bounds__(kResultsBlock)
k_result_leaves(const uint32_t *__restrict__ code, const int64_t *__restrict__ gas_wanted,
                const int64_t *__restrict__ gas_used, const uint8_t *__restrict__ data,
                const uint32_t *__restrict__ data_off, uint32_t n_results, const uint32_t *__restrict__ tree_off,
                const uint32_t *__restrict__ node_off, uint32_t n_trees, const uint32_t *__restrict__ first_node,
                uint32_t *__restrict__ node) {
  const uint32_t i = blockIdx.x * kResultsBlock + threadIdx.x;
  if (i >= n_results) {  // the lanes behind the results put each tree's leading leaf in front of it
    const uint32_t t = i - n_results;
    if (first_node && t < n_trees) {
      const uint4 *s = reinterpret_cast<const uint4 *>(first_node + 8ull * t);
      uint4 *o = reinterpret_cast<uint4 *>(node + 8ull * node_off[t]);
      o[0] = s[0];
      o[1] = s[1];
    }
    return;
  }
  uint32_t at = i;  // this result's node
  if (first_node) {
    uint32_t lo = 0, hi = n_trees;  // tree_off[lo] <= i < tree_off[hi]
    while (hi - lo > 1) {
      const uint32_t mid = (lo + hi) >> 1;
      if (tree_off[mid] <= i) lo = mid;
      else hi = mid;
    }
    at = i + lo + 1;
  }

  const uint32_t base = data_off[i], len = data_off[i + 1] - base;
  u128 head = 0;     // byte 0: the leaf prefix 0x00
  uint32_t dlo = 1;  // the head's length, where the data begins
  uint32_t n;
  const uint32_t c = code[i];
  if (c) {
    head |= tagged_varint(0x08, c, &n) << (8 * dlo);
    dlo += n;
  }
  if (len) {
    head |= tagged_varint(0x12, len, &n) << (8 * dlo);
    dlo += n;
  }
  const uint32_t dhi = dlo + len;  // where the data ends
  const uint64_t gw = (uint64_t)gas_wanted[i], gu = (uint64_t)gas_used[i];
  u128 tw = 0, tu = 0;
  uint32_t wl = 0, ul = 0;
  if (gw) tw = tagged_varint(0x28, gw, &wl);
  if (gu) tu = tagged_varint(0x30, gu, &ul);
  const uint32_t total = dhi + wl + ul;     // <= 13 + 2^30 + 22
  const uint32_t nblk = (total + 72) / 64;  // room for 0x80 and the 8-byte length
  const uint32_t end = 64 * nblk;
  const uint64_t bits = (uint64_t)total * 8;
  const uint32_t *dw = reinterpret_cast<const uint32_t *>(data);

  uint32_t st[8];
  sha256_init(st);
  for (uint32_t k = 0; k < nblk; k++) {
    uint32_t w[16];
#pragma unroll
    for (int q = 0; q < 16; q++) {
      const uint32_t p0 = 64 * k + 4 * q;
      uint32_t word = 0;
      if (p0 >= dlo && p0 + 4 <= dhi) {  // four data bytes: two aligned dwords, aligned by the address
        const uint32_t a = base + (p0 - dlo);
        const uint32_t sh = a & 3;
        const uint32_t l = dw[a >> 2];
        const uint32_t h = sh ? dw[(a >> 2) + 1] : 0;  // sh != 0: that dword still holds a byte of this result
        word = __builtin_bswap32(__builtin_amdgcn_alignbyte(h, l, sh));
      } else {
#pragma unroll
        for (int j = 0; j < 4; j++) {
          const uint32_t pos = p0 + j;
          uint32_t b = 0;
          if (pos < dlo) b = byte_of(head, pos);
          else if (pos < dhi) b = data[base + (pos - dlo)];
          else if (pos < dhi + wl) b = byte_of(tw, pos - dhi);
          else if (pos < total) b = byte_of(tu, pos - dhi - wl);
          else if (pos == total) b = 0x80;
          else if (pos >= end - 8) b = (uint32_t)(bits >> (8 * (end - 1 - pos))) & 0xffu;
          word = (word << 8) | b;
        }
      }
      w[q] = word;
    }
    sha256_compress(st, w);
  }
  uint4 *o = reinterpret_cast<uint4 *>(node + 8ull * at);
  o[0] = make_uint4(st[0], st[1], st[2], st[3]);
  o[1] = make_uint4(st[4], st[5], st[6], st[7]);
}

hipError_t launch_results_hashes(const uint32_t *code, const int64_t *gas_wanted, const int64_t *gas_used,
                                 const uint8_t *data, const uint32_t *data_off, uint32_t n_results,
                                 const uint32_t *tree_off, const uint32_t *node_off, uint32_t n_trees,
                                 uint32_t max_leaves, const uint32_t *first_node, uint32_t *node_a, uint32_t *node_b,
                                 uint8_t *out, hipStream_t stream) {
  const uint32_t lanes = n_results + (first_node ? n_trees : 0);
  if (lanes) {
    void *tok = ktimer::begin(ktimer::kResultLeaves, stream);
    hipLaunchKernelGGL(k_result_leaves, dim3((lanes + kResultsBlock - 1) / kResultsBlock), dim3(kResultsBlock), 0,
                       stream, code, gas_wanted, gas_used, data, data_off, n_results, tree_off, node_off, n_trees,
                       first_node, node_a);
    ktimer::end(tok, stream);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return launch_merkle_tree(node_off, n_trees, max_leaves, node_a, node_b, out, stream);
}

}  // namespace tmv
