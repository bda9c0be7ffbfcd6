// Block part sets and merkle proofs of the host layer (include/tmhost.h):
//   tmv_part_set_headers / tmv_part_set_proofs   NewPartSetFromData
//       (types/part_set.go:172-200) -> merkle.ProofsFromByteSlices
//       (crypto/merkle/proof.go:33-48), as blocksync's replay loop runs it per
//       block (internal/blocksync/reactor.go:563-582)
//   tmv_parts_verify     PartSet.AddPart's checks (types/part_set.go:272-300)
//   tmv_proofs_verify    Proof.ValidateBasic + Proof.Verify (proof.go:52-117)
// Large calls hash on the device through tmv_merkle_proofs /
// tmv_merkle_verify_proofs, weak references as tm_host_abi.cpp's secp256k1
// entry: a build of this file without the engine (the CPU test double) loads
// all the same and computes on the host with the merkle code of tm_light.h,
// extended here to proofs -- the same verdicts and texts.  Only the public
// tmv_* C-ABI is used to reach the device (layering).
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../../include/tmhost.h"
#include "../../../include/tmverify.h"
#include "merkle_plan.h"
#include "tm_host_internal.h"
#include "tm_light.h"
#include "tm_proof_common.h"

extern "C" int tmv_merkle_proofs(tmv_ctx *ctx, uint32_t flags, const uint8_t *data, const uint32_t *leaf_off,
                                 uint32_t n_leaves, const uint32_t *tree_off, uint32_t n_trees, uint8_t *root_out,
                                 uint8_t *leaf_hash_out, const uint32_t *aunt_off, uint8_t *aunts_out)
    __attribute__((weak));
extern "C" int tmv_merkle_verify_proofs(tmv_ctx *ctx, uint32_t flags, uint32_t n, const int64_t *total,
                                        const int64_t *index, const uint8_t *leaf_hash, const uint8_t *aunts,
                                        const uint32_t *aunt_off, const uint8_t *root, const uint8_t *data,
                                        const uint32_t *leaf_off, int8_t *status_out, uint8_t *leaf_hash_calc,
                                        uint8_t *root_calc, uint8_t *root_nil) __attribute__((weak));

namespace {

using tmh::Bytes;
using tmh::Digest;
using tmh_internal::parallel_for;
using tmh_proof::digest_out;
using tmh_proof::hex_upper;
using tmh_proof::put;
using tmh_proof::root_from_aunts;
using tmh_proof::validate_basic;

constexpr uint64_t kEngineMaxBytes = 1ull << 30;  // tmv_merkle_proofs' limits per call
constexpr uint64_t kEngineMaxLeaves = 1ull << 26;

// Calls with fewer leaf bytes than this compute on the host.  64 MiB: a
// 64 KiB part is 1,025 dependent SHA-256 blocks, ~4.6 ms on one lane however
// few parts there are.  The device path beats the 16-thread hashlib proxy
// from 12-24 MiB, but this file's own host code from about 48 MiB only; 64 MiB
// is the smallest measured window where it beats both by more than the
// spread between machines.
// TMV_DEVICE_MERKLE_MIN overrides (bytes; read on every call: tests change it).
uint64_t device_merkle_min() {
  const char *e = std::getenv("TMV_DEVICE_MERKLE_MIN");
  return e ? (uint64_t)std::strtoull(e, nullptr, 10) : (64ull << 20);
}

// The device path's copy of the leaves as one array, kept by the calling
// thread between calls: a fresh allocation of tens of MiB costs more in page
// faults than the copy itself (100 x 1 MiB: 38 ms with it, DESIGN.md section
// 15).  Buffers above 256 MiB are given back when the call ends.
struct Concat {
  std::vector<uint8_t> &buf;
  static std::vector<uint8_t> &mine() {
    static thread_local std::vector<uint8_t> b;
    return b;
  }
  Concat() : buf(mine()) {}
  uint8_t *get(size_t n) {
    if (buf.size() < n) {
      buf.clear();  // nothing to carry over
      buf.resize(n);
    }
    return buf.data();
  }
  ~Concat() {
    if (buf.size() > (256u << 20)) std::vector<uint8_t>().swap(buf);
  }
};

Digest leaf_digest(const uint8_t *p, size_t n) {  // leafHash (crypto/merkle/hash.go)
  static const uint8_t zero = 0;
  Digest dg;
  tmh::Sha256Bytes(dg.w, &zero, 1, p, n);
  return dg;
}

// The tree over n >= 1 leaf digests, every level kept (the pairing of
// k_merkle_tree_levels: equal to the split-point tree, TestHashAlternatives);
// aunts of leaf i, leaf sibling first, to aunts + 32 * aunt_off[i] (FlattenAunts).
void tree_host(const Digest *leaves, uint32_t n, uint8_t root[32], const uint32_t *aunt_off, uint8_t *aunts) {
  std::vector<std::vector<Digest>> lv;
  lv.emplace_back(leaves, leaves + n);
  while (lv.back().size() > 1) {
    const std::vector<Digest> &cur = lv.back();
    std::vector<Digest> nxt((cur.size() + 1) / 2);
    for (size_t i = 0; i + 1 < cur.size(); i += 2) tmv::sha256_inner(nxt[i / 2].w, cur[i].w, cur[i + 1].w);
    if (cur.size() & 1) nxt.back() = cur.back();
    lv.push_back(std::move(nxt));
  }
  digest_out(lv.back()[0], root);
  if (!aunts) return;
  for (uint32_t i = 0; i < n; i++) {
    uint64_t o = aunt_off[i];
    size_t j = i;
    for (size_t l = 0; l + 1 < lv.size(); l++, j >>= 1) {
      const size_t s = lv[l].size();
      if (j == s - 1 && (s & 1)) continue;  // promoted: no aunt at this level
      digest_out(lv[l][j ^ 1], aunts + 32 * o++);
    }
  }
}

// One proof against its leaf and root: the status and computed hashes of
// tmv_merkle_verify_proofs.
struct Item {
  const tmv_proof *pr;
  tmv_bytes leaf, root;
};
struct Verdict {
  int status = 0;
  uint8_t leaf_calc[32];
  Bytes root_calc;  // empty: nil
};

bool simple(const Item &it) {  // fits the engine's fixed 32-byte layout
  if (it.pr->leaf_hash.len != 32 || it.root.len != 32) return false;
  for (uint32_t a = 0; a < it.pr->n_aunts; a++)
    if (it.pr->aunts[a].len != 32) return false;
  return true;
}

void verify_host(const Item &it, Verdict &v) {
  const tmv_proof &p = *it.pr;
  digest_out(leaf_digest(it.leaf.p, it.leaf.len), v.leaf_calc);
  v.root_calc = root_from_aunts(p);
  const bool leaf_ok = p.leaf_hash.len == 32 && std::memcmp(p.leaf_hash.p, v.leaf_calc, 32) == 0;
  const bool root_ok = !v.root_calc.empty() && v.root_calc.size() == it.root.len &&
                       std::memcmp(v.root_calc.data(), it.root.p, it.root.len) == 0;
  v.status = p.total < 0 ? 1 : p.index < 0 ? 2 : !leaf_ok ? 3 : !root_ok ? 4 : 0;
}

// Verdicts of all items: the simple ones on the device when the call is large
// enough, in engine calls of at most 1 GiB of leaves; the rest on the host.
int verify_items(tmv_ctx *ctx, const std::vector<Item> &items, std::vector<Verdict> &out) {
  out.assign(items.size(), Verdict());
  std::vector<uint32_t> dev, host;
  uint64_t bytes = 0;
  for (uint32_t i = 0; i < items.size(); i++) {
    if (simple(items[i]) && items[i].leaf.len <= kEngineMaxBytes) {
      dev.push_back(i);
      bytes += items[i].leaf.len;
    } else {
      host.push_back(i);
    }
  }
  if (!tmv_merkle_verify_proofs || !ctx || bytes < device_merkle_min()) {
    host.insert(host.end(), dev.begin(), dev.end());
    dev.clear();
  }
  parallel_for(host.size(), 1, [&](size_t k) { verify_host(items[host[k]], out[host[k]]); });
  Concat concat;
  for (size_t lo = 0; lo < dev.size();) {
    size_t hi = lo;
    uint64_t sz = 0, na = 0;
    while (hi < dev.size() && hi - lo < (1u << 24) && sz + items[dev[hi]].leaf.len <= kEngineMaxBytes &&
           na + items[dev[hi]].pr->n_aunts <= (1u << 28)) {
      sz += items[dev[hi]].leaf.len;
      na += items[dev[hi]].pr->n_aunts;
      hi++;
    }
    if (hi == lo) return TMV_ERR_ARG;  // one proof with more than 2^28 aunts
    const uint32_t m = (uint32_t)(hi - lo);
    std::vector<int64_t> total(m), index(m);
    std::vector<uint8_t> lh(32ull * m), root(32ull * m), aunts(32 * na);
    uint8_t *data = concat.get(sz);
    std::vector<uint32_t> aoff(m + 1, 0), loff(m + 1, 0);
    for (uint32_t k = 0; k < m; k++) {
      const Item &it = items[dev[lo + k]];
      total[k] = it.pr->total;
      index[k] = it.pr->index;
      std::memcpy(lh.data() + 32ull * k, it.pr->leaf_hash.p, 32);
      std::memcpy(root.data() + 32ull * k, it.root.p, 32);
      aoff[k + 1] = aoff[k] + it.pr->n_aunts;
      loff[k + 1] = loff[k] + it.leaf.len;
    }
    parallel_for(m, 16, [&](size_t k) {
      const Item &it = items[dev[lo + k]];
      for (uint32_t a = 0; a < it.pr->n_aunts; a++)
        std::memcpy(aunts.data() + 32ull * (aoff[k] + a), it.pr->aunts[a].p, 32);
      if (it.leaf.len) std::memcpy(data + loff[k], it.leaf.p, it.leaf.len);
    });
    std::vector<int8_t> status(m);
    std::vector<uint8_t> lcalc(32ull * m), rcalc(32ull * m), nil(m);
    const int rc = tmv_merkle_verify_proofs(ctx, 0, m, total.data(), index.data(), lh.data(),
                                            aunts.empty() ? nullptr : aunts.data(), aoff.data(), root.data(),
                                            sz ? data : nullptr, loff.data(), status.data(),
                                            lcalc.data(), rcalc.data(), nil.data());
    if (rc < 0) return rc;
    for (uint32_t k = 0; k < m; k++) {
      Verdict &v = out[dev[lo + k]];
      v.status = status[k];
      std::memcpy(v.leaf_calc, lcalc.data() + 32ull * k, 32);
      if (!nil[k]) v.root_calc.assign(rcalc.begin() + 32ull * k, rcalc.begin() + 32ull * k + 32);
    }
    lo = hi;
  }
  return 0;
}

// NewPartSetFromData for n blocks; leaf_hash_out / aunt_off_out / aunts_out
// may be null (headers only).
int part_sets(tmv_ctx *ctx, const tmv_bytes *blocks, uint32_t n, uint32_t part_size, uint32_t *total_out,
              uint8_t *hash_out, uint8_t *leaf_hash_out, uint32_t *aunt_off_out, uint8_t *aunts_out,
              uint64_t aunts_cap) {
  if (part_size == 0) return TMV_ERR_ARG;
  if (n == 0) return 0;
  if (!blocks || !total_out || !hash_out) return TMV_ERR_ARG;
  std::vector<uint32_t> tree_off(n + 1, 0);
  uint64_t bytes = 0;
  for (uint32_t b = 0; b < n; b++) {
    if (blocks[b].len && !blocks[b].p) return TMV_ERR_ARG;
    const uint64_t t = ((uint64_t)blocks[b].len + part_size - 1) / part_size;
    if ((uint64_t)blocks[b].len + part_size - 1 > 0xffffffffull || tree_off[b] + t > kEngineMaxLeaves * 8)
      return TMV_ERR_ARG;  // the reference's uint32 arithmetic would wrap
    total_out[b] = (uint32_t)t;
    tree_off[b + 1] = tree_off[b] + (uint32_t)t;
    bytes += blocks[b].len;
  }
  const uint32_t parts = tree_off[n];
  std::vector<uint32_t> aoff_tmp;
  const bool want_aunts = aunts_out != nullptr;
  if (want_aunts || aunt_off_out) {
    if (!aunt_off_out) {
      aoff_tmp.resize((size_t)parts + 1);
      aunt_off_out = aoff_tmp.data();
    }
    if (tmh::merkle_aunt_offsets(tree_off.data(), n, aunt_off_out) != 0) return TMV_ERR_ARG;
    if (want_aunts && aunt_off_out[parts] > aunts_cap) return TMV_ERR_ARG;
  }
  std::vector<uint8_t> leaf_tmp;
  if (!leaf_hash_out) {
    leaf_tmp.resize(32ull * std::max<uint32_t>(parts, 1));
    leaf_hash_out = leaf_tmp.data();
  }
  auto part_span = [&](uint32_t b, uint32_t i, const uint8_t *&p, size_t &len) {
    const uint64_t lo = (uint64_t)i * part_size, hi = std::min<uint64_t>(blocks[b].len, lo + part_size);
    p = blocks[b].p + lo;
    len = (size_t)(hi - lo);
  };
  auto host_blocks = [&](uint32_t b0, uint32_t b1) {
    const uint32_t p0 = tree_off[b0], np = tree_off[b1] - p0;
    std::vector<Digest> lv(np);
    std::vector<uint32_t> owner(np);
    for (uint32_t b = b0; b < b1; b++)
      for (uint32_t p = tree_off[b]; p < tree_off[b + 1]; p++) owner[p - p0] = b;
    parallel_for(np, 1, [&](size_t k) {
      const uint32_t b = owner[k];
      const uint8_t *p;
      size_t len;
      part_span(b, (uint32_t)(p0 + k - tree_off[b]), p, len);
      lv[k] = leaf_digest(p, len);
      digest_out(lv[k], leaf_hash_out + 32ull * (p0 + k));
    });
    parallel_for(b1 - b0, 1, [&](size_t k) {
      const uint32_t b = b0 + (uint32_t)k, t = total_out[b];
      if (t == 0) {
        Digest e;
        tmh::Sha256Bytes(e.w, nullptr, 0, nullptr, 0);
        digest_out(e, hash_out + 32ull * b);
      } else {
        tree_host(lv.data() + (tree_off[b] - p0), t, hash_out + 32ull * b,
                  want_aunts ? aunt_off_out + tree_off[b] : nullptr, aunts_out);
      }
    });
  };
  if (!tmv_merkle_proofs || !ctx || bytes < device_merkle_min()) {
    host_blocks(0, n);
    return 0;
  }
  Concat concat;
  for (uint32_t b0 = 0; b0 < n;) {
    if (blocks[b0].len > kEngineMaxBytes || total_out[b0] > kEngineMaxLeaves) {  // not one engine call
      host_blocks(b0, b0 + 1);
      b0++;
      continue;
    }
    uint32_t b1 = b0;
    uint64_t sz = 0;
    while (b1 < n && sz + blocks[b1].len <= kEngineMaxBytes && tree_off[b1 + 1] - tree_off[b0] <= kEngineMaxLeaves) {
      sz += blocks[b1].len;
      b1++;
    }
    const uint32_t p0 = tree_off[b0], np = tree_off[b1] - p0, nt = b1 - b0;
    uint8_t *data = concat.get(sz);
    std::vector<uint32_t> loff(np + 1, 0), toff(nt + 1, 0), aoff;
    std::vector<uint64_t> base(nt + 1, 0);
    for (uint32_t b = b0; b < b1; b++) {
      base[b - b0 + 1] = base[b - b0] + blocks[b].len;
      toff[b - b0 + 1] = tree_off[b + 1] - p0;
      for (uint32_t i = 0; i < total_out[b]; i++)
        loff[tree_off[b] - p0 + i + 1] =
            (uint32_t)(base[b - b0] + std::min<uint64_t>(blocks[b].len, (uint64_t)(i + 1) * part_size));
    }
    parallel_for(nt, 1, [&](size_t k) {
      if (blocks[b0 + k].len) std::memcpy(data + base[k], blocks[b0 + k].p, blocks[b0 + k].len);
    });
    if (want_aunts) {  // the window's offsets: the call's, rebased
      aoff.resize(np + 1);
      for (uint32_t k = 0; k <= np; k++) aoff[k] = aunt_off_out[p0 + k] - aunt_off_out[p0];
    }
    const int rc = tmv_merkle_proofs(ctx, 0, sz ? data : nullptr, loff.data(), np, toff.data(), nt,
                                     hash_out + 32ull * b0, leaf_hash_out + 32ull * p0,
                                     want_aunts ? aoff.data() : nullptr,
                                     want_aunts ? aunts_out + 32ull * aunt_off_out[p0] : nullptr);
    if (rc < 0) return rc;
    b0 = b1;
  }
  return 0;
}

}  // namespace

extern "C" {

int tmv_part_set_headers(tmv_ctx *ctx, const tmv_bytes *blocks, uint32_t n, uint32_t part_size, uint32_t *total_out,
                         uint8_t *hash_out) {
  return part_sets(ctx, blocks, n, part_size, total_out, hash_out, nullptr, nullptr, nullptr, 0);
}

int tmv_part_set_proofs(tmv_ctx *ctx, const tmv_bytes *blocks, uint32_t n, uint32_t part_size, uint32_t *total_out,
                        uint8_t *hash_out, uint8_t *leaf_hash_out, uint32_t *aunt_off_out, uint8_t *aunts_out,
                        uint64_t aunts_cap) {
  if (n && (!leaf_hash_out || !aunt_off_out || !aunts_out)) return TMV_ERR_ARG;
  return part_sets(ctx, blocks, n, part_size, total_out, hash_out, leaf_hash_out, aunt_off_out, aunts_out, aunts_cap);
}

int tmv_parts_verify(tmv_ctx *ctx, const tmv_part_in *parts, uint32_t n, int32_t *results, char *errs,
                     size_t err_stride) {
  if (n == 0) return 0;
  if (!parts || !results) return TMV_ERR_ARG;
  std::vector<Item> items;
  std::vector<uint32_t> who;
  for (uint32_t i = 0; i < n; i++) {
    results[i] = TMV_PART_OK;
    put(errs, err_stride, i, "");
    if (parts[i].index >= parts[i].set_total) {  // part_set.go:280-282
      results[i] = TMV_PART_ERR_UNEXPECTED_INDEX;
      put(errs, err_stride, i, "error part set unexpected index");
      continue;
    }
    items.push_back(Item{&parts[i].proof, parts[i].bytes, parts[i].set_hash});
    who.push_back(i);
  }
  std::vector<Verdict> v;
  const int rc = verify_items(ctx, items, v);
  if (rc < 0) return rc;
  int failed = 0;
  for (size_t k = 0; k < who.size(); k++)
    if (v[k].status != 0) {  // part_set.go:290-292: any Verify error
      results[who[k]] = TMV_PART_ERR_INVALID_PROOF;
      put(errs, err_stride, who[k], "error part set invalid proof");
    }
  for (uint32_t i = 0; i < n; i++) failed += results[i] != TMV_PART_OK;
  return failed;
}

int tmv_proofs_verify(tmv_ctx *ctx, const tmv_proof_in *in, uint32_t n, int32_t *results, char *errs,
                      size_t err_stride) {
  if (n == 0) return 0;
  if (!in || !results) return TMV_ERR_ARG;
  std::vector<Item> items;
  std::vector<uint32_t> who;
  for (uint32_t i = 0; i < n; i++) {
    const std::string e = validate_basic(in[i].proof);
    results[i] = e.empty() ? 0 : 1;
    put(errs, err_stride, i, e);
    if (!e.empty()) continue;
    items.push_back(Item{&in[i].proof, in[i].leaf, in[i].root});
    who.push_back(i);
  }
  std::vector<Verdict> v;
  const int rc = verify_items(ctx, items, v);
  if (rc < 0) return rc;
  int failed = 0;
  for (size_t k = 0; k < who.size(); k++) {
    const uint32_t i = who[k];
    const tmv_proof &p = in[i].proof;
    std::string e;
    switch (v[k].status) {  // proof.go:52-68
      case 1: e = "proof total must be positive"; break;
      case 2: e = "proof index cannot be negative"; break;
      case 3:
        e = "invalid leaf hash: wanted " + hex_upper(v[k].leaf_calc, 32) + " got " +
            hex_upper(p.leaf_hash.p, p.leaf_hash.len);
        break;
      case 4:
        e = "invalid root hash: wanted " + hex_upper(in[i].root.p, in[i].root.len) + " got " +
            hex_upper(v[k].root_calc.data(), v[k].root_calc.size());
        break;
      default: break;
    }
    results[i] = e.empty() ? 0 : 1;
    put(errs, err_stride, i, e);
  }
  for (uint32_t i = 0; i < n; i++) failed += results[i] != 0;
  return failed;
}

}  // extern "C"
