// Commit.Hash on the device (types/block.go:900-918): merkle.HashFromByteSlices
// over the protobuf bytes of every CommitSig, which Block.ValidateBasic
// compares with Header.LastCommitHash (types/block.go:73-75) for each block
// blocksync applies.
//
//   k_commit_leaves  one lane per CommitSig: encode tmproto.CommitSig
//                    (proto/tendermint/types/types.pb.go:1764-1797) behind the
//                    RFC 6962 leaf prefix and hash it.
//   k_merkle_tree    (merkle_kernels.hip) the levels of each commit's tree.
//
// The encoded leaf, prefix included:
//   00                      leaf prefix
//   08 flag                 block_id_flag, omitted when 0
//   12 14 addr[20]          validator_address, omitted when empty
//   1a L ts                 timestamp, always present; ts = 08 varint(seconds)
//                           10 varint(nanos), each part omitted when zero and
//                           a negative value in the 10-byte two's-complement
//                           form (Go's zero time.Time is -62135596800 s)
//   22 len sig[len]         signature, omitted when empty
// at most 1 + 2 + 22 + 24 + 66 = 115 bytes, so one SHA-256 block when it is at
// most 55 bytes (an absent signature: 16) and two otherwise.
//
// The bytes land at positions that depend on the data, so a lane assembles its
// padded message in LDS, not in registers (a register array indexed at run
// time would go to scratch): 32 big-endian words per lane, word k of lane l at
// msg[k * 256 + l] -- every access of a wave falls on 64 consecutive dwords,
// free of bank conflicts, and a lane reads only what it wrote itself, so the
// kernel has no barrier.
#include <hip/hip_runtime.h>
#include "commit_hash.h"
#include "ktimer.h"
#include "sha256_dev.h"
#include "valset.h"

namespace tmv {

namespace {

constexpr int kCommitBlock = 256;
constexpr int kCommitWords = 32;  // two SHA-256 blocks per lane

struct LeafWriter {
  uint32_t *row;  // this lane's word 0
  uint32_t pos;   // next byte of the message
  __device__ __forceinline__ void put(uint32_t b) {
    // byte p of the message is byte 3 - p % 4 of the little-endian word p / 4
    reinterpret_cast<uint8_t *>(row + (pos >> 2) * kCommitBlock)[3 - (pos & 3)] = (uint8_t)b;
    pos++;
  }
  __device__ __forceinline__ void varint(uint64_t u) {
    bool live = true;
#pragma unroll
    for (int i = 0; i < 10; i++) {
      const bool more = (u >> 7) != 0;
      if (live) put((uint32_t)(u & 0x7f) | (more ? 0x80u : 0u));
      live = live && more;
      u >>= 7;
    }
  }
};

__device__ __forceinline__ uint32_t varint_len(uint64_t u) {
  return u == 0 ? 1u : (uint32_t)(70 - __clzll((long long)u)) / 7u;
}

}  // namespace

__global__ void __launch_bounds__(kCommitBlock)
k_commit_leaves(const uint8_t *__restrict__ flag, const uint8_t *__restrict__ addr_len,
                const uint8_t *__restrict__ addr, const int64_t *__restrict__ ts_seconds,
                const int32_t *__restrict__ ts_nanos, const uint8_t *__restrict__ sig_len,
                const uint8_t *__restrict__ sig, uint32_t n_sigs, uint32_t *__restrict__ node) {
  __shared__ uint32_t msg[kCommitWords * kCommitBlock];
  const uint32_t i = blockIdx.x * kCommitBlock + threadIdx.x;
  if (i >= n_sigs) return;  // no barrier below
  uint32_t *row = msg + threadIdx.x;
#pragma unroll
  for (int k = 0; k < kCommitWords; k++) row[k * kCommitBlock] = 0;
  LeafWriter w{row, 1};  // byte 0 is the leaf prefix 0x00

  const uint32_t f = flag[i];
  if (f) {
    w.put(0x08);
    w.put(f & 0x7f);
  }
  if (addr_len[i]) {
    const uint32_t *a = reinterpret_cast<const uint32_t *>(addr + 20ull * i);
    w.put(0x12);
    w.put(20);
#pragma unroll
    for (int k = 0; k < 5; k++) {
      const uint32_t v = a[k];
#pragma unroll
      for (int j = 0; j < 4; j++) w.put((v >> (8 * j)) & 0xff);
    }
  }
  const uint64_t sec = (uint64_t)ts_seconds[i], nan = (uint64_t)(int64_t)ts_nanos[i];
  w.put(0x1a);
  w.put((sec ? 1 + varint_len(sec) : 0) + (nan ? 1 + varint_len(nan) : 0));
  if (sec) {
    w.put(0x08);
    w.varint(sec);
  }
  if (nan) {
    w.put(0x10);
    w.varint(nan);
  }
  const uint32_t sl = min((uint32_t)sig_len[i], 64u);
  if (sl) {
    const uint4 *s = reinterpret_cast<const uint4 *>(sig + 64ull * i);
    w.put(0x22);
    w.put(sl);
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const uint4 q = s[k];
      const uint32_t v[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
      for (int j = 0; j < 16; j++)
        if ((uint32_t)(16 * k + j) < sl) w.put((v[j >> 2] >> (8 * (j & 3))) & 0xff);
    }
  }
  const uint32_t total = w.pos;  // <= 115
  w.put(0x80);
  const bool two = total > 55;
  row[(two ? 31 : 15) * kCommitBlock] = total * 8;  // the bit length fits the last word

  uint32_t st[8], blk[16];
  sha256_init(st);
#pragma unroll
  for (int k = 0; k < 16; k++) blk[k] = row[k * kCommitBlock];
  sha256_compress(st, blk);
  if (two) {
#pragma unroll
    for (int k = 0; k < 16; k++) blk[k] = row[(16 + k) * kCommitBlock];
    sha256_compress(st, blk);
  }
  uint4 *o = reinterpret_cast<uint4 *>(node + 8ull * i);
  o[0] = make_uint4(st[0], st[1], st[2], st[3]);
  o[1] = make_uint4(st[4], st[5], st[6], st[7]);
}

hipError_t launch_commit_hashes(const uint8_t *flag, const uint8_t *addr_len, const uint8_t *addr,
                                const int64_t *ts_seconds, const int32_t *ts_nanos, const uint8_t *sig_len,
                                const uint8_t *sig, uint32_t n_sigs, const uint32_t *commit_off, uint32_t n_commits,
                                uint32_t max_sigs, uint32_t *node_a, uint32_t *node_b, uint8_t *out,
                                hipStream_t stream) {
  if (n_sigs) {
    void *tok = ktimer::begin(ktimer::kCommitLeaves, stream);
    hipLaunchKernelGGL(k_commit_leaves, dim3((n_sigs + kCommitBlock - 1) / kCommitBlock), dim3(kCommitBlock), 0,
                       stream, flag, addr_len, addr, ts_seconds, ts_nanos, sig_len, sig, n_sigs, node_a);
    ktimer::end(tok, stream);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return launch_merkle_tree(commit_off, n_commits, max_sigs, node_a, node_b, out, stream);
}

}  // namespace tmv
