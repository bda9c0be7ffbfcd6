// Merkle inclusion proofs on the device: merkle.ProofsFromByteSlices
// (crypto/merkle/proof.go:33-48) and Proof.Verify (proof.go:52-68) for many
// trees / proofs per launch -- what NewPartSetFromData (types/part_set.go:
// 172-200) builds over a block's 64 KiB parts on blocksync's replay path
// (internal/blocksync/reactor.go:563-582), what PartSet.AddPart checks for
// every received part (types/part_set.go:272-300), and what Txs.Hash /
// Txs.Proof (types/tx.go:30-75) run over SHA-256(tx).
//
//   k_merkle_leaves_long   RFC 6962 leaf hashes SHA-256(0x00 || leaf) of leaves
//                          of any length, tuned for 64 KiB block parts.  One
//                          wave per workgroup takes `lpw` leaves (8..64, a
//                          launch parameter: few leaves are spread over more
//                          waves).  The wave stages its leaves through LDS in
//                          rounds of 512 bytes per leaf: every global load is
//                          a 16-byte unit per lane, 32 consecutive lanes on 32
//                          consecutive units of one leaf, and only whole
//                          aligned units of the staged buffer are read.  Lane
//                          l then compresses the 8 blocks of its own leaf from
//                          its LDS slot (ds_read_b128; slots are 33 units
//                          apart, so a 16-lane read group touches 16 distinct
//                          16-byte bank slots).  A leaf starts anywhere: its
//                          byte stream sits at shift 0..15 inside its first
//                          unit, undone by a dword select and one v_perm_b32
//                          per message word (which also makes it big-endian).
//                          Leaves of different lengths differ only in their
//                          trip counts.  kPrehash: SHA-256(0x00 ||
//                          SHA-256(item)), the leaf of Txs.Hash.
//   k_merkle_digests_long  the same kernel body without prefix or second
//                          hash: SHA-256(item), the value digests of
//                          tmv_merkle_value_ops (merkle_ops_kernels.hip).
//   k_merkle_tree_levels   k_merkle_tree's pairing and odd promotion (equal to
//                          the split-point tree by TestHashAlternatives), one
//                          workgroup per tree, but every level is kept: level 0
//                          is the leaf array, the levels above follow one
//                          another in the tree's arena (host/merkle_plan.h).
//   k_merkle_aunts         one lane per leaf walks the levels upwards: at a
//                          level of size s, node j's aunt is node j^1 unless j
//                          is the promoted last node of an odd level; leaf
//                          sibling first, as FlattenAunts (proof.go:197-215).
//   k_merkle_verify_proofs one lane per proof, computeHashFromAunts
//                          (proof.go:151-181) without the recursion: walk down
//                          from (index, total) by split points recording
//                          left/right, then fold the aunts upwards.
// Hashes are serialised big-endian, as the roots of merkle_kernels.hip.
#include <hip/hip_runtime.h>
#include "ktimer.h"
#include "merkle_proof.h"
#include "sha256_dev.h"

namespace tmv {

namespace {

constexpr int kSegUnits = kMerkleSegBytes / 16;  // 16-byte units per leaf and staging round
constexpr int kSlotUnits = kSegUnits + 1;         // + the unit the byte shift spills into

__device__ __forceinline__ void load_node(uint32_t h[8], const uint32_t *p) {
  const uint4 *q = reinterpret_cast<const uint4 *>(p);
  const uint4 a = q[0], b = q[1];
  h[0] = a.x; h[1] = a.y; h[2] = a.z; h[3] = a.w;
  h[4] = b.x; h[5] = b.y; h[6] = b.z; h[7] = b.w;
}

__device__ __forceinline__ void store_node(uint32_t *p, const uint32_t h[8]) {
  uint4 *q = reinterpret_cast<uint4 *>(p);
  q[0] = make_uint4(h[0], h[1], h[2], h[3]);
  q[1] = make_uint4(h[4], h[5], h[6], h[7]);
}

// 32 serialised bytes (16-byte aligned) <-> 8 state words
__device__ __forceinline__ void load_hash(uint32_t h[8], const uint8_t *p) {
  load_node(h, reinterpret_cast<const uint32_t *>(p));
#pragma unroll
  for (int i = 0; i < 8; i++) h[i] = __builtin_bswap32(h[i]);
}

__device__ __forceinline__ void store_hash(uint8_t *p, const uint32_t h[8]) {
  uint32_t s[8];
#pragma unroll
  for (int i = 0; i < 8; i++) s[i] = __builtin_bswap32(h[i]);
  store_node(reinterpret_cast<uint32_t *>(p), s);
}

__device__ __forceinline__ void empty_hash(uint32_t h[8]) {  // emptyHash(): SHA-256 of the empty string
  uint32_t w[16];
#pragma unroll
  for (int i = 0; i < 16; i++) w[i] = 0;
  w[0] = 0x80000000u;
  sha256_init(h);
  sha256_compress(h, w);
}

}  // namespace

// data is 16-byte aligned with 16 readable bytes in front of it and readable
// up to the next 16-byte boundary behind its last byte (the runtime's staging).
// LDS: lpw slots of kSlotUnits units, then lpw first-unit indices and lpw
// unit counts.
template <bool kPrehash>
__global__ void __launch_bounds__(64)
k_merkle_leaves_long(const uint8_t *data, const uint32_t *__restrict__ leaf_off, uint32_t n_leaves, uint32_t lpw,
                     uint32_t *__restrict__ node) {
  extern __shared__ uint4 lds[];
  int32_t *s_u0 = reinterpret_cast<int32_t *>(lds + lpw * kSlotUnits);
  uint32_t *s_nu = reinterpret_cast<uint32_t *>(s_u0 + lpw);
  const uint4 *du = reinterpret_cast<const uint4 *>(data);
  const uint32_t lane = threadIdx.x;
  const uint64_t i = (uint64_t)blockIdx.x * lpw + lane;
  const bool active = lane < lpw && i < n_leaves;
  constexpr uint32_t pre = kPrehash ? 0 : 1;  // the 0x00 leaf prefix
  // The message is the byte stream that starts `pre` bytes before the leaf
  // (that byte is overwritten by the prefix): unit u0, shift sh inside it.
  uint32_t total = 0, nblk = 0, nu = 0, sh = 0;
  int32_t u0 = 0;
  if (active) {
    const uint32_t b = leaf_off[i], len = leaf_off[i + 1] - b;
    const int64_t p = (int64_t)b - pre;
    u0 = (int32_t)(p >> 4);
    sh = (uint32_t)(p & 15);
    total = len + pre;
    nblk = (total + 72) / 64;  // room for 0x80 and the 8-byte length
    nu = len ? (uint32_t)((int32_t)(((uint64_t)b + len - 1) >> 4) - u0) + 1 : 0;  // through the last byte's unit
  }
  if (lane < lpw) {
    s_u0[lane] = u0;
    s_nu[lane] = nu;
    if (nu) lds[lane * kSlotUnits] = du[u0];
  }
  __syncthreads();
  const uint32_t nch = (nblk + 7) / 8;
  const uint32_t ds = sh >> 2;
  const uint32_t sel = 0x00010203u + (sh & 3) * 0x01010101u;  // v_perm_b32: bytes sh&3 .. of a dword pair, first byte on top
  const uint64_t bits = (uint64_t)total * 8;
  const uint4 *slot = lds + lane * kSlotUnits;
  uint32_t st[8];
  sha256_init(st);
  for (uint32_t c = 0; __ballot(c < nch) != 0; c++) {
    // units 32c + 1 .. 32c + 32 of every leaf of the wave: a half-wave per leaf
    const uint32_t hl = lane & 31, u = kSegUnits * c + 1 + hl;
#pragma unroll 4
    for (uint32_t s2 = 0; s2 < lpw; s2 += 2) {
      const uint32_t sl = s2 + (lane >> 5);
      if (sl < lpw && u < s_nu[sl]) lds[sl * kSlotUnits + 1 + hl] = du[(int64_t)s_u0[sl] + u];
    }
    __syncthreads();
#pragma unroll 1
    for (uint32_t j = 0; j < 8; j++) {
      const uint32_t blk = 8 * c + j;
      if (blk >= nblk) break;
      uint32_t d[20];
#pragma unroll
      for (int q = 0; q < 5; q++) {
        const uint4 v = slot[4 * j + q];
        d[4 * q] = v.x; d[4 * q + 1] = v.y; d[4 * q + 2] = v.z; d[4 * q + 3] = v.w;
      }
      if (ds & 1) {
#pragma unroll
        for (int q = 0; q < 19; q++) d[q] = d[q + 1];
      }
      if (ds & 2) {
#pragma unroll
        for (int q = 0; q < 17; q++) d[q] = d[q + 2];
      }
      uint32_t w[16];
#pragma unroll
      for (int q = 0; q < 16; q++) w[q] = __builtin_amdgcn_perm(d[q + 1], d[q], sel);
      if (!kPrehash && blk == 0) w[0] &= 0x00ffffffu;  // the leaf prefix
      if (64 * (blk + 1) > total) {  // the message ends in or before this block
#pragma unroll
        for (int q = 0; q < 16; q++) {
          const int rem = (int)total - (int)(64 * blk + 4 * q);  // message bytes from this word on
          if (rem <= 0) {
            w[q] = rem == 0 ? 0x80000000u : 0u;
          } else if (rem < 4) {
            w[q] = (w[q] & (0xffffffffu << (32 - 8 * rem))) | (0x80u << (24 - 8 * rem));
          }
        }
        if (blk + 1 == nblk) {
          w[14] = (uint32_t)(bits >> 32);
          w[15] = (uint32_t)bits;
        }
      }
      sha256_compress(st, w);
    }
    if (lane < lpw) lds[lane * kSlotUnits] = slot[kSegUnits];  // the spill unit opens the next round
    __syncthreads();
  }
  if (!active) return;
  if (kPrehash) {  // SHA-256(0x00 || digest): 33 bytes, one block
    uint32_t w[16];
    w[0] = st[0] >> 8;
#pragma unroll
    for (int q = 1; q < 8; q++) w[q] = (st[q - 1] << 24) | (st[q] >> 8);
    w[8] = (st[7] << 24) | 0x00800000u;
#pragma unroll
    for (int q = 9; q < 15; q++) w[q] = 0;
    w[15] = 33 * 8;
    sha256_init(st);
    sha256_compress(st, w);
  }
  store_node(node + 8ull * i, st);
}

// k_merkle_leaves_long without prefix and without kPrehash's second hash: the
// state words of SHA-256(item).  A kernel of its own, restated line by line:
// as a third mode of the template it moved k_merkle_leaves_long<false>'s
// register count.  Same staging, LDS and launch shape.
__global__ void __launch_bounds__(64)
k_merkle_digests_long(const uint8_t *data, const uint32_t *__restrict__ leaf_off, uint32_t n_leaves, uint32_t lpw,
                      uint32_t *__restrict__ node) {
  extern __shared__ uint4 lds[];
  int32_t *s_u0 = reinterpret_cast<int32_t *>(lds + lpw * kSlotUnits);
  uint32_t *s_nu = reinterpret_cast<uint32_t *>(s_u0 + lpw);
  const uint4 *du = reinterpret_cast<const uint4 *>(data);
  const uint32_t lane = threadIdx.x;
  const uint64_t i = (uint64_t)blockIdx.x * lpw + lane;
  const bool active = lane < lpw && i < n_leaves;
  constexpr uint32_t pre = 0;  // no prefix
  // The message is the byte stream that starts `pre` bytes before the leaf
  // (that byte is overwritten by the prefix): unit u0, shift sh inside it.
  uint32_t total = 0, nblk = 0, nu = 0, sh = 0;
  int32_t u0 = 0;
  if (active) {
    const uint32_t b = leaf_off[i], len = leaf_off[i + 1] - b;
    const int64_t p = (int64_t)b - pre;
    u0 = (int32_t)(p >> 4);
    sh = (uint32_t)(p & 15);
    total = len + pre;
    nblk = (total + 72) / 64;  // room for 0x80 and the 8-byte length
    nu = len ? (uint32_t)((int32_t)(((uint64_t)b + len - 1) >> 4) - u0) + 1 : 0;  // through the last byte's unit
  }
  if (lane < lpw) {
    s_u0[lane] = u0;
    s_nu[lane] = nu;
    if (nu) lds[lane * kSlotUnits] = du[u0];
  }
  __syncthreads();
  const uint32_t nch = (nblk + 7) / 8;
  const uint32_t ds = sh >> 2;
  const uint32_t sel = 0x00010203u + (sh & 3) * 0x01010101u;  // v_perm_b32: bytes sh&3 .. of a dword pair, first byte on top
  const uint64_t bits = (uint64_t)total * 8;
  const uint4 *slot = lds + lane * kSlotUnits;
  uint32_t st[8];
  sha256_init(st);
  for (uint32_t c = 0; __ballot(c < nch) != 0; c++) {
    // units 32c + 1 .. 32c + 32 of every leaf of the wave: a half-wave per leaf
    const uint32_t hl = lane & 31, u = kSegUnits * c + 1 + hl;
#pragma unroll 4
    for (uint32_t s2 = 0; s2 < lpw; s2 += 2) {
      const uint32_t sl = s2 + (lane >> 5);
      if (sl < lpw && u < s_nu[sl]) lds[sl * kSlotUnits + 1 + hl] = du[(int64_t)s_u0[sl] + u];
    }
    __syncthreads();
#pragma unroll 1
    for (uint32_t j = 0; j < 8; j++) {
      const uint32_t blk = 8 * c + j;
      if (blk >= nblk) break;
      uint32_t d[20];
#pragma unroll
      for (int q = 0; q < 5; q++) {
        const uint4 v = slot[4 * j + q];
        d[4 * q] = v.x; d[4 * q + 1] = v.y; d[4 * q + 2] = v.z; d[4 * q + 3] = v.w;
      }
      if (ds & 1) {
#pragma unroll
        for (int q = 0; q < 19; q++) d[q] = d[q + 1];
      }
      if (ds & 2) {
#pragma unroll
        for (int q = 0; q < 17; q++) d[q] = d[q + 2];
      }
      uint32_t w[16];
#pragma unroll
      for (int q = 0; q < 16; q++) w[q] = __builtin_amdgcn_perm(d[q + 1], d[q], sel);
      if (64 * (blk + 1) > total) {  // the message ends in or before this block
#pragma unroll
        for (int q = 0; q < 16; q++) {
          const int rem = (int)total - (int)(64 * blk + 4 * q);  // message bytes from this word on
          if (rem <= 0) {
            w[q] = rem == 0 ? 0x80000000u : 0u;
          } else if (rem < 4) {
            w[q] = (w[q] & (0xffffffffu << (32 - 8 * rem))) | (0x80u << (24 - 8 * rem));
          }
        }
        if (blk + 1 == nblk) {
          w[14] = (uint32_t)(bits >> 32);
          w[15] = (uint32_t)bits;
        }
      }
      sha256_compress(st, w);
    }
    if (lane < lpw) lds[lane * kSlotUnits] = slot[kSegUnits];  // the spill unit opens the next round
    __syncthreads();
  }
  if (!active) return;
  store_node(node + 8ull * i, st);
}

template <int kTreeBlock>
__global__ void __launch_bounds__(kTreeBlock)
k_merkle_tree_levels(const uint32_t *__restrict__ tree_off, uint32_t n_trees, const uint32_t *leafn, uint32_t *arena,
                     uint8_t *__restrict__ root_out) {
  const uint32_t s = blockIdx.x;
  if (s >= n_trees) return;
  const uint32_t base = tree_off[s], n = tree_off[s + 1] - base;
  uint32_t root[8];
  if (n == 0) {
    if (threadIdx.x != 0) return;
    empty_hash(root);
  } else {
    const uint32_t *cur = leafn + 8ull * base;
    uint32_t *nxt = arena + 8ull * ((uint64_t)base + (uint64_t)kMerkleLevelSlack * s);
    uint32_t size = n;
    while (size > 1) {  // block-uniform
      const uint32_t half = size >> 1;
      for (uint32_t i = threadIdx.x; i < half; i += kTreeBlock) {
        uint32_t l[8], r[8], h[8];
        load_node(l, cur + 16ull * i);
        load_node(r, cur + 16ull * i + 8);
        sha256_inner(h, l, r);
        store_node(nxt + 8ull * i, h);
      }
      if ((size & 1) && threadIdx.x == 0) {
        uint32_t h[8];
        load_node(h, cur + 8ull * (size - 1));
        store_node(nxt + 8ull * half, h);
      }
      __syncthreads();  // this level's nodes written (workgroup-scope fence)
      size = half + (size & 1);
      cur = nxt;
      nxt += 8ull * size;
    }
    if (threadIdx.x != 0) return;
    load_node(root, cur);
  }
  store_hash(root_out + 32ull * s, root);
}

// aunts_out == nullptr: leaf hashes only.
__global__ void __launch_bounds__(256)
k_merkle_aunts(const uint32_t *__restrict__ tree_off, uint32_t n_trees, uint32_t n_leaves, const uint32_t *leafn,
               const uint32_t *arena, const uint32_t *__restrict__ aunt_off, uint8_t *__restrict__ leaf_hash_out,
               uint8_t *__restrict__ aunts_out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_leaves) return;
  uint32_t h[8];
  load_node(h, leafn + 8ull * i);
  store_hash(leaf_hash_out + 32ull * i, h);
  if (!aunts_out) return;
  // the leaf's tree: the last t with tree_off[t] <= i (empty trees share offsets)
  uint32_t lo = 0, hi = n_trees;
  while (hi - lo > 1) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (tree_off[mid] <= i) lo = mid; else hi = mid;
  }
  const uint32_t base = tree_off[lo];
  uint32_t size = tree_off[lo + 1] - base, j = i - base;
  const uint32_t *lvl = leafn + 8ull * base;
  const uint32_t *nxt = arena + 8ull * ((uint64_t)base + (uint64_t)kMerkleLevelSlack * lo);
  uint64_t o = aunt_off[i];
  const uint64_t o_end = aunt_off[i + 1];
  while (size > 1) {
    if (!(j == size - 1 && (size & 1))) {  // not the promoted node of an odd level
      if (o >= o_end) return;              // aunt_off not from tmv_merkle_aunt_offsets: never write past the leaf's range
      load_node(h, lvl + 8ull * (j ^ 1));
      store_hash(aunts_out + 32ull * o, h);
      o++;
    }
    j >>= 1;
    size = (size + 1) >> 1;
    lvl = nxt;
    nxt += 8ull * size;
  }
}

// leafn: the proofs' leaves hashed by the leaf kernel, or nullptr when the
// caller vouches for leaf_hash (no leaf test then).  Status as
// tmv_merkle_verify_proofs (include/tmverify.h).
__global__ void __launch_bounds__(256)
k_merkle_verify_proofs(uint32_t n, const int64_t *__restrict__ total, const int64_t *__restrict__ index,
                       const uint8_t *__restrict__ leaf_hash, const uint8_t *__restrict__ aunts,
                       const uint32_t *__restrict__ aunt_off, const uint8_t *__restrict__ root, const uint32_t *leafn,
                       int8_t *__restrict__ status_out, uint8_t *__restrict__ leaf_calc_out,
                       uint8_t *__restrict__ root_calc_out, uint8_t *__restrict__ root_nil_out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int64_t tot = total[i], idx = index[i];
  const uint32_t a0 = aunt_off[i], na = aunt_off[i + 1] - a0;
  uint32_t h[8], lc[8];
  load_hash(h, leaf_hash + 32ull * i);
  bool leaf_ok = true;
  if (leafn) {
    load_node(lc, leafn + 8ull * i);
#pragma unroll
    for (int k = 0; k < 8; k++) leaf_ok = leaf_ok && lc[k] == h[k];
  } else {
#pragma unroll
    for (int k = 0; k < 8; k++) lc[k] = h[k];
  }
  // down from (index, total): bit d of mask = the path goes right at depth d
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
    nil = depth != na;  // aunts left over at total == 1, or none left at total > 1
  }
  if (!nil) {
    for (uint32_t j = 0; j < depth; j++) {  // aunt j pairs with direction depth-1-j
      uint32_t a[8], o[8];
      load_hash(a, aunts + 32ull * (a0 + j));
      if ((mask >> (depth - 1 - j)) & 1) sha256_inner(o, a, h);
      else sha256_inner(o, h, a);
#pragma unroll
      for (int k = 0; k < 8; k++) h[k] = o[k];
    }
  } else {
#pragma unroll
    for (int k = 0; k < 8; k++) h[k] = 0;
  }
  uint32_t want[8];
  load_hash(want, root + 32ull * i);
  bool root_ok = !nil;
#pragma unroll
  for (int k = 0; k < 8; k++) root_ok = root_ok && want[k] == h[k];
  status_out[i] = tot < 0 ? 1 : idx < 0 ? 2 : !leaf_ok ? 3 : !root_ok ? 4 : 0;
  store_hash(leaf_calc_out + 32ull * i, lc);
  store_hash(root_calc_out + 32ull * i, h);
  root_nil_out[i] = nil ? 1 : 0;
}

hipError_t launch_merkle_leaves_long(const uint8_t *data, const uint32_t *leaf_off, uint32_t n_leaves, bool prehash,
                                     uint32_t lpw, uint32_t *node, hipStream_t stream) {
  if (!n_leaves) return hipSuccess;
  if (lpw != 8 && lpw != 16 && lpw != 32 && lpw != 64) return hipErrorInvalidValue;
  const size_t lds_bytes = (size_t)lpw * (16 * kSlotUnits + 8);
  const dim3 grid((n_leaves + lpw - 1) / lpw), block(64);
  void *tok = ktimer::begin(ktimer::kMerkleLeavesLong, stream);
  if (prehash)
    hipLaunchKernelGGL(k_merkle_leaves_long<true>, grid, block, lds_bytes, stream, data, leaf_off, n_leaves, lpw, node);
  else
    hipLaunchKernelGGL(k_merkle_leaves_long<false>, grid, block, lds_bytes, stream, data, leaf_off, n_leaves, lpw,
                       node);
  ktimer::end(tok, stream);
  return hipGetLastError();
}

hipError_t launch_merkle_digests_long(const uint8_t *data, const uint32_t *leaf_off, uint32_t n_items, uint32_t lpw,
                                      uint32_t *node, hipStream_t stream) {
  if (!n_items) return hipSuccess;
  if (lpw != 8 && lpw != 16 && lpw != 32 && lpw != 64) return hipErrorInvalidValue;
  const size_t lds_bytes = (size_t)lpw * (16 * kSlotUnits + 8);
  void *tok = ktimer::begin(ktimer::kMerkleDigestsLong, stream);
  hipLaunchKernelGGL(k_merkle_digests_long, dim3((n_items + lpw - 1) / lpw), dim3(64), lds_bytes, stream, data,
                     leaf_off, n_items, lpw, node);
  ktimer::end(tok, stream);
  return hipGetLastError();
}

hipError_t launch_merkle_proofs(const uint32_t *tree_off, uint32_t n_trees, uint32_t n_leaves, uint32_t max_leaves,
                                const uint32_t *leafn, uint32_t *arena, const uint32_t *aunt_off, uint8_t *root_out,
                                uint8_t *leaf_hash_out, uint8_t *aunts_out, hipStream_t stream) {
  if (!n_trees) return hipSuccess;
  void *tok = ktimer::begin(ktimer::kMerkleTreeLevels, stream);
  // small trees take one wave per tree, as launch_merkle_roots
  if (max_leaves <= 128)
    hipLaunchKernelGGL(k_merkle_tree_levels<64>, dim3(n_trees), dim3(64), 0, stream, tree_off, n_trees, leafn, arena,
                       root_out);
  else
    hipLaunchKernelGGL(k_merkle_tree_levels<256>, dim3(n_trees), dim3(256), 0, stream, tree_off, n_trees, leafn, arena,
                       root_out);
  ktimer::end(tok, stream);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess || !n_leaves) return e;
  tok = ktimer::begin(ktimer::kMerkleAunts, stream);
  hipLaunchKernelGGL(k_merkle_aunts, dim3((n_leaves + 255) / 256), dim3(256), 0, stream, tree_off, n_trees, n_leaves,
                     leafn, arena, aunt_off, leaf_hash_out, aunts_out);
  ktimer::end(tok, stream);
  return hipGetLastError();
}

hipError_t launch_merkle_verify_proofs(uint32_t n, const int64_t *total, const int64_t *index, const uint8_t *leaf_hash,
                                       const uint8_t *aunts, const uint32_t *aunt_off, const uint8_t *root,
                                       const uint32_t *leafn, int8_t *status_out, uint8_t *leaf_calc_out,
                                       uint8_t *root_calc_out, uint8_t *root_nil_out, hipStream_t stream) {
  if (!n) return hipSuccess;
  void *tok = ktimer::begin(ktimer::kMerkleVerify, stream);
  hipLaunchKernelGGL(k_merkle_verify_proofs, dim3((n + 255) / 256), dim3(256), 0, stream, n, total, index, leaf_hash,
                     aunts, aunt_off, root, leafn, status_out, leaf_calc_out, root_calc_out, root_nil_out);
  ktimer::end(tok, stream);
  return hipGetLastError();
}

}  // namespace tmv
