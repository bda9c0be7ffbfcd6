// Device-side vote sign-bytes (tmv_verify_votes): each lane writes one
// vote's canonical message (votes.h) into the batch's message buffer, where
// the verification kernels read it as if the host had sent it.  The host
// sends 16 bytes per vote plus one template per commit instead of ~120 bytes
// of encoded message; the kernel is pure byte movement (HBM/L2-bound, a few
// microseconds per 100k votes next to ~1 ms of verification).
#include <hip/hip_runtime.h>
#include "verify_kernels.h"
#include "votes.h"
#include "vote_ext.h"
#include "ktimer.h"

namespace tmv {

__device__ __forceinline__ uint8_t *put_uvarint(uint8_t *p, uint64_t x) {
  while (x >= 0x80) { *p++ = (uint8_t)(x | 0x80); x >>= 7; }
  *p++ = (uint8_t)x;
  return p;
}

__device__ __forceinline__ uint8_t *put_bytes(uint8_t *p, const uint8_t *src, uint32_t n) {
  for (uint32_t k = 0; k < n; k++) p[k] = src[k];
  return p + n;
}

__global__ void __launch_bounds__(256)
k_vote_signbytes(const tmv_vote *__restrict__ votes, const VoteTab *__restrict__ tab,
                 const uint8_t *__restrict__ blob, const uint32_t *__restrict__ off, uint32_t n,
                 uint8_t *__restrict__ msg) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const tmv_vote v = votes[i];
  const VoteTab t = tab[v.tmpl & ~TMV_VOTE_WITH_BLOCK];
  uint8_t *p = msg + off[i];
  p = put_uvarint(p, vote_body_len(t, v));
  p = put_bytes(p, blob + t.head_at, t.head_len);
  if (v.tmpl & TMV_VOTE_WITH_BLOCK) p = put_bytes(p, blob + t.block_at, t.block_len);
  *p++ = 0x2a;
  p = put_uvarint(p, vote_ts_inner(v.ts_seconds, v.ts_nanos));
  if (v.ts_seconds != 0) { *p++ = 0x08; p = put_uvarint(p, (uint64_t)v.ts_seconds); }
  if (v.ts_nanos != 0) { *p++ = 0x10; p = put_uvarint(p, (uint64_t)(int64_t)v.ts_nanos); }
  put_bytes(p, blob + t.chain_at, t.chain_len);
}

// Template indices are checked on the host (tmv_verify_votes) before launch.
hipError_t launch_vote_signbytes(const tmv_vote *votes, const VoteTab *tab, const uint8_t *blob,
                                 const uint32_t *off, uint32_t n, uint8_t *msg, hipStream_t stream) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(k_vote_signbytes, dim3((n + 255) / 256), dim3(256), 0, stream, votes, tab, blob, off, n, msg);
  return hipGetLastError();
}

// ---- Vote-extension sign-bytes (vote_ext.h) ----
// Lane i writes entry i's prefix (uvarint(len(body)), 0x0a, uvarint(E)) and
// its tail with byte stores, and copies a payload shorter than wave_min
// itself.  Longer payloads are copied by the whole wave, one after the other
// (wave_copy).  Messages are packed back to back, so a dword of msg can hold
// bytes of up to four entries: every store below writes bytes of the entry's
// own [off[i], off[i+1]) only, and no dword shared with a neighbour is ever
// read, modified and written back.

// dst[0, len) = src[0, len) by the 64 lanes of a wave; dst, src and len are
// wave-uniform.  Byte stores up to the first dword of dst that the payload
// owns whole and after the last one; in between, consecutive lanes store
// consecutive dwords, each made of two aligned source dwords funnel-shifted
// by the byte offset between source and destination (as sha512_pq_msg does).
// Loads: the aligned dwords around src reach at most 3 bytes before src and
// 3 bytes past src + len.  The staging keeps them inside its region by
// PADDING, not by clamping: the payload region starts 16-byte aligned (so
// rounding an address down to a dword never leaves it) and is followed by 16
// spare bytes (vote_ext_runtime.h, vote_ext_plan).
__device__ __forceinline__ void wave_copy(uint8_t *dst, const uint8_t *src, uint32_t len, uint32_t lane) {
  uint32_t head = (uint32_t)(-(uintptr_t)dst & 3);
  if (head > len) head = len;
  if (lane < head) dst[lane] = src[lane];
  const uint32_t nd = (len - head) >> 2;
  uint32_t *dw = reinterpret_cast<uint32_t *>(dst + head);
  const uint8_t *s = src + head;
  const uint32_t sh = (uint32_t)((uintptr_t)s & 3);
  const uint32_t *sw = reinterpret_cast<const uint32_t *>((uintptr_t)s - sh);
  if (sh == 0) {
#pragma unroll 4
    for (uint32_t j = lane; j < nd; j += 64) dw[j] = sw[j];
  } else {
#pragma unroll 4
    for (uint32_t j = lane; j < nd; j += 64) dw[j] = __builtin_amdgcn_alignbit(sw[j + 1], sw[j], 8 * sh);
  }
  const uint32_t done = head + 4 * nd;  // len - done is 0..3
  if (lane < len - done) dst[done + lane] = src[done + lane];
}

__global__ void __launch_bounds__(256)
k_vote_ext_signbytes(const VoteExtTab *__restrict__ tab, const uint8_t *__restrict__ blob,
                     const uint32_t *__restrict__ tmpl, const uint32_t *__restrict__ src_off,
                     const uint8_t *__restrict__ data, const uint32_t *__restrict__ off, uint32_t n,
                     uint8_t *__restrict__ msg, uint32_t wave_min) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t lane = threadIdx.x & 63;
  uint32_t len = 0, src = 0, dst = 0;
  bool wide = false;
  if (i < n) {
    const VoteExtTab t = tab[tmpl[i]];
    src = src_off[i];
    len = src_off[i + 1] - src;
    uint8_t *p = msg + off[i];
    p = put_uvarint(p, vote_ext_body_len(t.tail_len, len));
    if (len) { *p++ = 0x0a; p = put_uvarint(p, len); }
    dst = (uint32_t)(p - msg);
    wide = wave_min != 0 && len >= wave_min;
    if (!wide) put_bytes(p, data + src, len);
    put_bytes(p + len, blob + t.tail_at, t.tail_len);
  }
  // the wave's long payloads, entry after entry: source, destination and
  // length of the next one read from its lane, so they are wave-uniform
  uint64_t todo = __ballot(wide);
  while (todo) {
    const int l = __ffsll((unsigned long long)todo) - 1;
    todo &= todo - 1;
    const uint32_t d = __builtin_amdgcn_readlane(dst, l), s = __builtin_amdgcn_readlane(src, l),
                   e = __builtin_amdgcn_readlane(len, l);
    wave_copy(msg + d, data + s, e, lane);
  }
}

// Template indices and offsets are checked on the host (prepare_vote_exts)
// before launch.
hipError_t launch_vote_ext_signbytes(const VoteExtTab *tab, const uint8_t *blob, const uint32_t *tmpl,
                                     const uint32_t *src_off, const uint8_t *data, const uint32_t *off, uint32_t n,
                                     uint8_t *msg, uint32_t wave_min, hipStream_t stream) {
  if (n == 0) return hipSuccess;
  void *tok = ktimer::begin(ktimer::kVoteExtSignbytes, stream);
  hipLaunchKernelGGL(k_vote_ext_signbytes, dim3((n + 255) / 256), dim3(256), 0, stream, tab, blob, tmpl, src_off,
                     data, off, n, msg, wave_min);
  const hipError_t e = hipGetLastError();
  ktimer::end(tok, stream);
  return e;
}

}  // namespace tmv
