// secp256k1 ECDSA verification on the device (crypto/secp256k1/secp256k1.go:
// 206-226, PubKey.VerifySignature), one lane per signature, two kernels:
//   k_secp_prep    SHA-256 of the message, key parsing and decompression, the
//                  range and lower-S tests, w = 1/s, u1 = z w, u2 = r w, and
//                  the signature's table of Q multiples (workspace memory)
//   k_secp_verify  R' = u1 G + u2 Q over 64 interleaved 4-bit windows and the
//                  x(R') mod n == r compare
// and, for keys the runtime keeps on the device (secp256k1.h, comb tables):
//   k_secp_key_table    one wave per missing key, one window per lane: parse
//                       and decompress the key, 16^j Q by doublings, its 15
//                       multiples, one inversion per lane, 15 affine entries
//                       into the key's slot
//   k_secp_prep_cached  k_secp_prep without the key work
//   k_secp_verify_comb  128 additions from G's comb and the slot's, the compare
// Entries that fail a test in k_secp_prep stay in their wave with a valid
// stand-in key (G) and end with status 0: no lane leaves the chain early.
// Inputs are a padded copy made by the runtime: keys at a 48-byte stride,
// signatures at 64, so a lane reads its key and signature as aligned 16-byte
// loads.  Messages are read byte by byte and never past their own end.
#include <hip/hip_runtime.h>
#include "ktimer.h"
#include "secp256k1.h"
#include "secp256k1_launch.h"

namespace tmv {

using namespace secp;

namespace {

// byte k of a little-endian dword array
__device__ __forceinline__ uint32_t byte_at(const uint32_t *d, int k) { return (d[k >> 2] >> (8 * (k & 3))) & 0xffu; }

}  // namespace

__global__ void __launch_bounds__(256)
k_secp_prep(const uint4 *__restrict__ pk48, const uint4 *__restrict__ sig, const uint8_t *__restrict__ msg,
            const uint32_t *__restrict__ msg_off, uint32_t n, uint4 *__restrict__ vin, uint32_t *__restrict__ qtab) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint32_t kd[12], sd[16];
#pragma unroll
  for (int q = 0; q < 3; q++) {
    const uint4 v = pk48[3ull * i + q];
    kd[4 * q] = v.x; kd[4 * q + 1] = v.y; kd[4 * q + 2] = v.z; kd[4 * q + 3] = v.w;
  }
#pragma unroll
  for (int q = 0; q < 4; q++) {
    const uint4 v = sig[4ull * i + q];
    sd[4 * q] = v.x; sd[4 * q + 1] = v.y; sd[4 * q + 2] = v.z; sd[4 * q + 3] = v.w;
  }
  const uint32_t prefix = byte_at(kd, 0);
  uint32_t xw[8], rw[8], sw[8];
#pragma unroll
  for (int k = 0; k < 8; k++) {
    const int b = 29 - 4 * k;  // x is bytes 1..32, big-endian
    xw[k] = (byte_at(kd, b) << 24) | (byte_at(kd, b + 1) << 16) | (byte_at(kd, b + 2) << 8) | byte_at(kd, b + 3);
    rw[k] = __builtin_bswap32(sd[7 - k]);
    sw[k] = __builtin_bswap32(sd[15 - k]);
  }
  const uint32_t base = msg_off[i], len = msg_off[i + 1] - base;
  uint32_t zw[8];
  sha256_words(zw, msg + base, len);
  VerifyInput in;
  ge q;
  verify_prepare(in, q, prefix, xw, rw, sw, zw);
  uint4 *o = vin + 8ull * i;
  o[0] = make_uint4(in.u1.w[0], in.u1.w[1], in.u1.w[2], in.u1.w[3]);
  o[1] = make_uint4(in.u1.w[4], in.u1.w[5], in.u1.w[6], in.u1.w[7]);
  o[2] = make_uint4(in.u2.w[0], in.u2.w[1], in.u2.w[2], in.u2.w[3]);
  o[3] = make_uint4(in.u2.w[4], in.u2.w[5], in.u2.w[6], in.u2.w[7]);
  o[4] = make_uint4(in.r[0], in.r[1], in.r[2], in.r[3]);
  o[5] = make_uint4(in.r[4], in.r[5], in.r[6], in.r[7]);
  o[6] = make_uint4(in.ok, 0, 0, 0);
  build_q_table(qtab + (size_t)kQTableWords * i, q);
}

__global__ void __launch_bounds__(256)
k_secp_verify(const uint4 *__restrict__ vin, const uint32_t *__restrict__ qtab, const uint32_t *__restrict__ gtab,
              uint32_t n, uint8_t *__restrict__ valid) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint4 *p = vin + 8ull * i;
  VerifyInput in;
  uint4 v;
  v = p[0]; in.u1.w[0] = v.x; in.u1.w[1] = v.y; in.u1.w[2] = v.z; in.u1.w[3] = v.w;
  v = p[1]; in.u1.w[4] = v.x; in.u1.w[5] = v.y; in.u1.w[6] = v.z; in.u1.w[7] = v.w;
  v = p[2]; in.u2.w[0] = v.x; in.u2.w[1] = v.y; in.u2.w[2] = v.z; in.u2.w[3] = v.w;
  v = p[3]; in.u2.w[4] = v.x; in.u2.w[5] = v.y; in.u2.w[6] = v.z; in.u2.w[7] = v.w;
  v = p[4]; in.r[0] = v.x; in.r[1] = v.y; in.r[2] = v.z; in.r[3] = v.w;
  v = p[5]; in.r[4] = v.x; in.r[5] = v.y; in.r[6] = v.z; in.r[7] = v.w;
  in.ok = p[6].x;
  valid[i] = verify_chain(in, gtab, qtab + (size_t)kQTableWords * i) ? 1 : 0;
}

// Lane j of a wave builds window j of one key's comb.  The 4 j doublings run
// as 252 steps for the whole wave (lanes past their count keep their value),
// which costs the wave what lane 63 needs anyway.  A key that does not parse
// leaves G's comb in its slot and 0 in slot_ok / miss_ok: its entries fail in
// k_secp_prep_cached and the runtime takes the slot back.
__global__ void __launch_bounds__(256)
k_secp_key_table(const uint4 *__restrict__ pk48, const uint32_t *__restrict__ slot, uint32_t n_keys,
                 uint32_t *__restrict__ table, uint32_t *__restrict__ slot_ok, uint32_t *__restrict__ miss_ok) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t m = t >> 6, j = t & 63;
  if (m >= n_keys) return;  // whole waves: a key is 64 consecutive lanes
  uint32_t kd[12];
#pragma unroll
  for (int q = 0; q < 3; q++) {
    const uint4 v = pk48[3ull * m + q];
    kd[4 * q] = v.x; kd[4 * q + 1] = v.y; kd[4 * q + 2] = v.z; kd[4 * q + 3] = v.w;
  }
  uint32_t xw[8];
#pragma unroll
  for (int k = 0; k < 8; k++) {
    const int b = 29 - 4 * k;
    xw[k] = (byte_at(kd, b) << 24) | (byte_at(kd, b + 1) << 16) | (byte_at(kd, b + 2) << 8) | byte_at(kd, b + 3);
  }
  ge q;
  const bool ok = ge_decompress(q, byte_at(kd, 0), xw);
  gej base;
  gej_set_ge(base, q);
#pragma unroll 1
  for (uint32_t i = 0; i < 4 * (kCombWindows - 1); i++) {
    gej d;
    gej_double(d, base);
    gej_cmov(base, d, i < 4 * j);
  }
  gej pts[kWindowEntries];
  secp::fe pre[kWindowEntries];
  comb_window_multiples(pts, base);
  const uint32_t sl = slot[m];
  comb_store_affine(table + (size_t)kCombWords * sl + kCombEntryWords * kWindowEntries * j, pts, pre, kWindowEntries);
  if (j == 0) {
    slot_ok[sl] = ok ? 1u : 0u;
    miss_ok[m] = ok ? 1u : 0u;
  }
}

// slot[i]: the key's slot, or kSecpNoSlot for a key that cannot parse (the
// host sees the prefix and x >= p).  The record's ok covers the key; word 25
// carries the slot on to k_secp_verify_comb.
__global__ void __launch_bounds__(256)
k_secp_prep_cached(const uint4 *__restrict__ sig, const uint8_t *__restrict__ msg,
                   const uint32_t *__restrict__ msg_off, const uint32_t *__restrict__ slot,
                   const uint32_t *__restrict__ slot_ok, uint32_t n, uint4 *__restrict__ vin) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint32_t sd[16];
#pragma unroll
  for (int q = 0; q < 4; q++) {
    const uint4 v = sig[4ull * i + q];
    sd[4 * q] = v.x; sd[4 * q + 1] = v.y; sd[4 * q + 2] = v.z; sd[4 * q + 3] = v.w;
  }
  uint32_t rw[8], sw[8];
#pragma unroll
  for (int k = 0; k < 8; k++) {
    rw[k] = __builtin_bswap32(sd[7 - k]);
    sw[k] = __builtin_bswap32(sd[15 - k]);
  }
  const uint32_t sl = slot[i];
  const bool key_ok = sl != kSecpNoSlot && slot_ok[sl != kSecpNoSlot ? sl : 0] != 0;
  const uint32_t base = msg_off[i], len = msg_off[i + 1] - base;
  uint32_t zw[8];
  sha256_words(zw, msg + base, len);
  VerifyInput in;
  verify_prepare_cached(in, key_ok, rw, sw, zw);
  uint4 *o = vin + 8ull * i;
  o[0] = make_uint4(in.u1.w[0], in.u1.w[1], in.u1.w[2], in.u1.w[3]);
  o[1] = make_uint4(in.u1.w[4], in.u1.w[5], in.u1.w[6], in.u1.w[7]);
  o[2] = make_uint4(in.u2.w[0], in.u2.w[1], in.u2.w[2], in.u2.w[3]);
  o[3] = make_uint4(in.u2.w[4], in.u2.w[5], in.u2.w[6], in.u2.w[7]);
  o[4] = make_uint4(in.r[0], in.r[1], in.r[2], in.r[3]);
  o[5] = make_uint4(in.r[4], in.r[5], in.r[6], in.r[7]);
  o[6] = make_uint4(in.ok, sl, 0, 0);
}

// An entry without a slot walks G's comb twice as its stand-in.
__global__ void __launch_bounds__(256)
k_secp_verify_comb(const uint4 *__restrict__ vin, const uint32_t *__restrict__ table,
                   const uint32_t *__restrict__ gcomb, uint32_t n, uint8_t *__restrict__ valid) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t *rec = reinterpret_cast<const uint32_t *>(vin + 8ull * i);
  const uint32_t sl = rec[25];
  const uint32_t *qcomb = sl != kSecpNoSlot ? table + (size_t)kCombWords * sl : gcomb;
  valid[i] = verify_chain_comb(rec, gcomb, qcomb) ? 1 : 0;
}

hipError_t launch_secp256k1_key_tables(const uint8_t *pk48, const uint32_t *slot, uint32_t n_keys, uint32_t *table,
                                       uint32_t *slot_ok, uint32_t *miss_ok, hipStream_t stream) {
  if (!n_keys) return hipSuccess;
  void *tk = ktimer::begin(ktimer::kSecpKeyTable, stream);
  hipLaunchKernelGGL(k_secp_key_table, dim3((n_keys + 3) / 4), dim3(256), 0, stream,
                     reinterpret_cast<const uint4 *>(pk48), slot, n_keys, table, slot_ok, miss_ok);
  ktimer::end(tk, stream);
  return hipGetLastError();
}

size_t secp256k1_cached_workspace_bytes(uint32_t n) { return (size_t)n * sizeof(VerifyInput); }
size_t secp256k1_comb_bytes() { return kCombBytes; }

hipError_t launch_secp256k1_verify_cached(const uint8_t *sig, const uint8_t *msg, const uint32_t *msg_off,
                                          const uint32_t *slot, uint32_t n, const uint32_t *gcomb,
                                          const uint32_t *table, const uint32_t *slot_ok, uint8_t *work,
                                          uint8_t *valid, hipStream_t stream) {
  if (!n) return hipSuccess;
  uint4 *vin = reinterpret_cast<uint4 *>(work);
  const dim3 grid((n + 255) / 256), block(256);
  void *tk = ktimer::begin(ktimer::kSecpPrepCached, stream);
  hipLaunchKernelGGL(k_secp_prep_cached, grid, block, 0, stream, reinterpret_cast<const uint4 *>(sig), msg, msg_off,
                     slot, slot_ok, n, vin);
  ktimer::end(tk, stream);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  tk = ktimer::begin(ktimer::kSecpVerifyComb, stream);
  hipLaunchKernelGGL(k_secp_verify_comb, grid, block, 0, stream, vin, table, gcomb, n, valid);
  ktimer::end(tk, stream);
  return hipGetLastError();
}

// Workspace of one launch pair, per entry
size_t secp256k1_workspace_bytes(uint32_t n) { return (size_t)n * (sizeof(VerifyInput) + 4ull * kQTableWords); }

// n entries: pk48 / sig the padded copies, msg_off n + 1 absolute offsets into
// msg, work >= secp256k1_workspace_bytes(n) (256-byte aligned), valid n bytes.
hipError_t launch_secp256k1_verify(const uint8_t *pk48, const uint8_t *sig, const uint8_t *msg,
                                   const uint32_t *msg_off, uint32_t n, const uint32_t *gtab, uint8_t *work,
                                   uint8_t *valid, hipStream_t stream) {
  static_assert(sizeof(VerifyInput) == 128, "k_secp_prep writes 128-byte records");
  if (!n) return hipSuccess;
  uint4 *vin = reinterpret_cast<uint4 *>(work);
  uint32_t *qtab = reinterpret_cast<uint32_t *>(work + (size_t)n * sizeof(VerifyInput));
  const dim3 grid((n + 255) / 256), block(256);
  void *tk = ktimer::begin(ktimer::kSecpPrep, stream);
  hipLaunchKernelGGL(k_secp_prep, grid, block, 0, stream, reinterpret_cast<const uint4 *>(pk48),
                     reinterpret_cast<const uint4 *>(sig), msg, msg_off, n, vin, qtab);
  ktimer::end(tk, stream);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  tk = ktimer::begin(ktimer::kSecpVerify, stream);
  hipLaunchKernelGGL(k_secp_verify, grid, block, 0, stream, vin, qtab, gtab, n, valid);
  ktimer::end(tk, stream);
  return hipGetLastError();
}

}  // namespace tmv
