// csrc/host/merkle_plan.h and the host layer's part-set / proof code
// (csrc/host/tm_merkle_abi.cpp, no engine linked) under ASan + UBSan as a
// stand-alone program: part sets built and verified on the host, and the
// aunt offsets of many tree layouts written into exactly-sized heap arrays
// (an overrun is an ASan report), cross-checked against the per-leaf count
// and against the levels the tree kernel writes into its arena.
#include <algorithm>
#include <cstdio>
#include <vector>

#include "../../../include/tmhost.h"
#include "host/merkle_plan.h"

static int g_wrong = 0;
static void expect(bool ok, const char *what, uint64_t a, uint64_t b) {
  if (!ok) {
    if (g_wrong++ < 10) std::printf("WRONG %s (%llu, %llu)\n", what, (unsigned long long)a, (unsigned long long)b);
  }
}

// nodes in the levels above the leaves, as k_merkle_tree_levels lays them out
static uint64_t upper_nodes(uint64_t n) {
  uint64_t sum = 0;
  while (n > 1) {
    n = (n + 1) / 2;
    sum += n;
  }
  return sum;
}

// tmv_part_set_proofs / tmv_parts_verify / tmv_proofs_verify on the host: outputs in exactly-sized
// heap arrays, every part verifies, a flipped byte and odd-sized hashes do not
static void host_layer() {
  const uint32_t sizes[] = {0, 1, 4096, 4097, 3 * 4096 + 17, 100000};
  for (uint32_t part_size : {4096u, 1000u, 7u}) {
    std::vector<std::vector<uint8_t>> data;
    std::vector<tmv_bytes> blocks;
    uint32_t parts = 0;
    for (uint32_t s : sizes) {
      if (part_size == 7 && s > 5000) s = 5000;
      data.emplace_back(s);
      for (uint32_t i = 0; i < s; i++) data.back()[i] = (uint8_t)(i * 131 + s);
      parts += (s + part_size - 1) / part_size;
    }
    for (auto &d : data) blocks.push_back(tmv_bytes{d.empty() ? nullptr : d.data(), (uint32_t)d.size()});
    const uint32_t n = (uint32_t)blocks.size();
    std::vector<uint32_t> total(n), total2(n), aoff((size_t)parts + 1), tree_off(n + 1, 0);
    std::vector<uint8_t> hash(32 * n), hash2(32 * n), leaf(32 * (size_t)parts);
    expect(tmv_part_set_headers(nullptr, blocks.data(), n, part_size, total.data(), hash.data()) == 0, "headers", 0, 0);
    for (uint32_t b = 0; b < n; b++) tree_off[b + 1] = tree_off[b] + total[b];
    expect(tree_off[n] == parts, "parts", tree_off[n], parts);
    std::vector<uint32_t> plan((size_t)parts + 1);
    tmh::merkle_aunt_offsets(tree_off.data(), n, plan.data());
    std::vector<uint8_t> aunts(32 * (size_t)plan[parts] + 1);
    expect(tmv_part_set_proofs(nullptr, blocks.data(), n, part_size, total2.data(), hash2.data(), leaf.data(),
                               aoff.data(), aunts.data(), plan[parts]) == 0, "proofs", 0, 0);
    expect(total == total2 && hash == hash2 && aoff == plan, "headers vs proofs", part_size, 0);
    if (plan[parts])
      expect(tmv_part_set_proofs(nullptr, blocks.data(), n, part_size, total2.data(), hash2.data(), leaf.data(),
                                 aoff.data(), aunts.data(), plan[parts] - 1) == TMV_ERR_ARG, "aunts_cap", 0, 0);
    std::vector<std::vector<tmv_bytes>> av(parts);
    std::vector<tmv_part_in> in;
    for (uint32_t b = 0, p = 0; b < n; b++)
      for (uint32_t i = 0; i < total[b]; i++, p++) {
        for (uint32_t a = aoff[p]; a < aoff[p + 1]; a++) av[p].push_back(tmv_bytes{aunts.data() + 32 * (size_t)a, 32});
        tmv_part_in x{};
        x.index = i;
        const uint32_t lo = i * part_size, hi = std::min<uint32_t>(blocks[b].len, lo + part_size);
        x.bytes = tmv_bytes{blocks[b].p + lo, hi - lo};
        x.proof = tmv_proof{(int64_t)total[b], (int64_t)i, tmv_bytes{leaf.data() + 32 * (size_t)p, 32},
                            av[p].empty() ? nullptr : av[p].data(), (uint32_t)av[p].size()};
        x.set_total = total[b];
        x.set_hash = tmv_bytes{hash.data() + 32 * b, 32};
        in.push_back(x);
      }
    std::vector<int32_t> res(in.size());
    std::vector<char> errs(64 * in.size());
    expect(tmv_parts_verify(nullptr, in.data(), (uint32_t)in.size(), res.data(), errs.data(), 64) == 0, "parts verify",
           part_size, 0);
    // break three of them: a flipped byte, a short leaf hash, index = total
    std::vector<uint8_t> flipped(in.back().bytes.p, in.back().bytes.p + in.back().bytes.len);
    flipped[0] ^= 1;
    in.back().bytes.p = flipped.data();
    in[1].proof.leaf_hash.len = 31;
    in[2].index = in[2].set_total;
    expect(tmv_parts_verify(nullptr, in.data(), (uint32_t)in.size(), res.data(), errs.data(), 64) == 3, "bad parts",
           part_size, 0);
    expect(res.back() == TMV_PART_ERR_INVALID_PROOF && res[1] == TMV_PART_ERR_INVALID_PROOF &&
               res[2] == TMV_PART_ERR_UNEXPECTED_INDEX && res[0] == TMV_PART_OK, "bad part kinds", part_size, 0);
    std::vector<tmv_proof_in> pin;
    for (const tmv_part_in &x : in) pin.push_back(tmv_proof_in{x.proof, x.bytes, x.set_hash});
    std::vector<char> errs2(8 * pin.size());  // texts longer than the stride are cut, never overrun
    expect(tmv_proofs_verify(nullptr, pin.data(), (uint32_t)pin.size(), res.data(), errs2.data(), 8) == 2,
           "proofs verify", part_size, 0);
  }
}

int main() {
  host_layer();
  // one tree of every size up to 1,030; then layouts with empty trees between
  for (uint32_t n = 0; n <= 1030; n++) {
    std::vector<uint32_t> tree_off{0, n};
    std::vector<uint32_t> out((size_t)n + 1);
    expect(tmh::merkle_aunt_offsets(tree_off.data(), 1, out.data()) == 0, "offsets rc", n, 0);
    for (uint32_t i = 0; i < n; i++)
      expect(out[i + 1] - out[i] == tmh::merkle_aunt_count(i, n), "aunt count", i, n);
    expect(upper_nodes(n) <= (uint64_t)n + tmh::kMerkleLevelSlack, "arena slack", n, upper_nodes(n));
  }
  const uint32_t sizes[] = {0, 1, 0, 0, 2, 3, 0, 17, 64, 65, 0, 129, 1000, 0};
  std::vector<uint32_t> tree_off{0};
  for (uint32_t s : sizes) tree_off.push_back(tree_off.back() + s);
  const uint32_t n_trees = (uint32_t)tree_off.size() - 1, n_leaves = tree_off.back();
  std::vector<uint32_t> out((size_t)n_leaves + 1);
  expect(tmh::merkle_aunt_offsets(tree_off.data(), n_trees, out.data()) == 0, "offsets rc", n_trees, 0);
  for (uint32_t t = 0; t < n_trees; t++) {
    for (uint32_t i = tree_off[t]; i < tree_off[t + 1]; i++)
      expect(out[i + 1] - out[i] == tmh::merkle_aunt_count(i - tree_off[t], sizes[t]), "aunt count (many)", i, t);
    // a tree's levels end before the next tree's begin
    expect(tmh::merkle_arena_base(tree_off[t], t) + upper_nodes(sizes[t]) <= tmh::merkle_arena_base(tree_off[t + 1], t + 1),
           "arena overlap", t, sizes[t]);
  }
  expect(tmh::merkle_arena_base(tree_off[n_trees], n_trees) == tmh::merkle_arena_nodes(n_leaves, n_trees), "arena size",
         n_leaves, n_trees);
  std::vector<uint32_t> bad{0, 5, 3};
  std::vector<uint32_t> o6(6);
  expect(tmh::merkle_aunt_offsets(bad.data(), 2, o6.data()) == -1, "decreasing offsets", 0, 0);
  // large totals: depths at the edges of 2^k and 2^k +- 1, up to 2^62
  for (int k = 1; k <= 62; k++) {
    const uint64_t p = 1ull << k;
    expect(tmh::merkle_aunt_count(0, p) == (uint32_t)k, "depth 2^k", 0, p);
    expect(tmh::merkle_aunt_count(p - 1, p) == (uint32_t)k, "depth 2^k last", p - 1, p);
    expect(tmh::merkle_aunt_count(p, p + 1) == 1, "depth 2^k+1 last", p, p + 1);
    expect(tmh::merkle_aunt_count(0, p + 1) == (uint32_t)k + 1, "depth 2^k+1 first", 0, p + 1);
    expect(tmh::merkle_split_point(p) == p / 2 && tmh::merkle_split_point(p + 1) == p, "split", p, 0);
  }
  for (uint32_t n : {0u, 1u, 2048u, 2049u, 4096u, 4097u, 16384u, 16385u, 1u << 26})
    expect((tmh::merkle_leaves_per_wave(n) & (tmh::merkle_leaves_per_wave(n) - 1)) == 0 &&
               tmh::merkle_leaves_per_wave(n) >= 8 && tmh::merkle_leaves_per_wave(n) <= 64,
           "leaves per wave", n, tmh::merkle_leaves_per_wave(n));
  std::printf("%d wrong\n", g_wrong);
  return g_wrong ? 1 : 0;
}
