// The host layer's results code (csrc/host/tm_results_abi.cpp and
// csrc/host/results_encode.h, no engine linked) under ASan + UBSan as a
// stand-alone program: the encoder over the case table of
// tests/results_cases.py (every code, gas and data-length class, the data in
// exactly-sized heap buffers so an overrun is an ASan report) against the
// lengths proto3 gives and the literal encodings of
// tests/golden/tx_results_vectors.json, the roots of trees of many sizes with
// and without a leading leaf, HashConsensusParams, and both verify calls with
// error buffers shorter than the texts.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../../include/tmhost.h"
#include "host/results_encode.h"

static int g_wrong = 0;
static void expect(bool ok, const char *what, uint64_t a, uint64_t b) {
  if (!ok) {
    if (g_wrong++ < 10) std::printf("WRONG %s (%llu, %llu)\n", what, (unsigned long long)a, (unsigned long long)b);
  }
}

struct Res {
  std::vector<uint8_t> data;
  tmv_tx_result r;
};

static Res make(uint32_t code, uint32_t len, int64_t gw, int64_t gu) {
  Res x;
  x.data.resize(len);
  for (uint32_t i = 0; i < len; i++) x.data[i] = (uint8_t)(31 * i + len);
  x.r = tmv_tx_result{code, tmv_bytes{nullptr, len}, gw, gu};
  return x;
}
static void fix(std::vector<Res> &v) {
  for (Res &x : v) x.r.data.p = x.data.empty() ? nullptr : x.data.data();
}

static size_t want_len(const tmv_tx_result &r) {
  return (r.code ? 1 + tmh::UvarintLen(r.code) : 0) + (r.data.len ? 1 + tmh::UvarintLen(r.data.len) + r.data.len : 0) +
         (r.gas_wanted ? 1 + tmh::UvarintLen((uint64_t)r.gas_wanted) : 0) +
         (r.gas_used ? 1 + tmh::UvarintLen((uint64_t)r.gas_used) : 0);
}

static std::string hex(const uint8_t *p, size_t n) {
  static const char d[] = "0123456789abcdef";
  std::string s;
  for (size_t i = 0; i < n; i++) {
    s += d[p[i] >> 4];
    s += d[p[i] & 15];
  }
  return s;
}

int main() {
  // the encoder, every combination of the classes
  std::vector<Res> rs;
  const int64_t gas[] = {0, 1, -1, INT64_MAX, INT64_MIN};
  for (uint32_t code : {0u, 127u, 128u, 0xffffffffu})
    for (int64_t gw : gas)
      for (int64_t gu : gas)
        for (uint32_t len : {0u, 1u, 52u, 53u, 60u, 61u, 116u, 117u, 124u, 125u, 127u, 128u, 16383u, 16384u})
          rs.push_back(make(code, len, gw, gu));
  fix(rs);
  for (const Res &x : rs) {
    tmh::Bytes out;
    tmh::AppendTxResultProto(x.r, out);
    expect(out.size() == want_len(x.r), "encoded length", out.size(), want_len(x.r));
    if (x.r.data.len) {
      const size_t at = (x.r.code ? 1 + tmh::UvarintLen(x.r.code) : 0) + 1 + tmh::UvarintLen(x.r.data.len);
      expect(std::memcmp(out.data() + at, x.data.data(), x.data.size()) == 0, "data bytes", x.r.code, x.r.data.len);
    }
  }
  // the literal encodings (abci/types/types_test.go's inputs)
  struct Lit { uint32_t code; const char *data; int64_t gw, gu; const char *want; };
  const Lit lits[] = {{0, "", 0, 0, ""}, {0, "one", 0, 0, "12036f6e65"}, {14, "", 0, 0, "080e"},
                      {14, "foo", 0, 0, "080e1203666f6f"},
                      {1, "transaction", 1000, 1000, "0801120b7472616e73616374696f6e28e80730e807"}};
  for (const Lit &l : lits) {
    std::vector<uint8_t> d(l.data, l.data + std::strlen(l.data));
    tmv_tx_result r{l.code, tmv_bytes{d.empty() ? nullptr : d.data(), (uint32_t)d.size()}, l.gw, l.gu};
    tmh::Bytes out;
    tmh::AppendTxResultProto(r, out);
    expect(hex(out.data(), out.size()) == l.want, "literal encoding", l.code, out.size());
  }

  // roots of trees of many sizes in one call, with and without a leading leaf
  std::vector<std::vector<tmv_tx_result>> held;
  size_t at = 0;
  for (uint32_t n : {0u, 1u, 2u, 3u, 64u, 65u, 128u, 129u, 257u}) {
    held.emplace_back();
    for (uint32_t i = 0; i < n; i++) held.back().push_back(rs[(at += 7) % rs.size()].r);
  }
  std::vector<const tmv_tx_result *> ptrs;
  std::vector<uint32_t> counts;
  for (auto &h : held) {
    ptrs.push_back(h.empty() ? nullptr : h.data());
    counts.push_back((uint32_t)h.size());
  }
  const uint32_t nt = (uint32_t)ptrs.size();
  std::vector<std::vector<uint8_t>> lead_bytes;
  for (uint32_t t = 0; t < nt; t++) lead_bytes.emplace_back((t % 3) * 100, (uint8_t)t);  // every third one empty
  std::vector<tmv_bytes> leads;
  for (auto &b : lead_bytes) leads.push_back(tmv_bytes{b.empty() ? nullptr : b.data(), (uint32_t)b.size()});
  std::vector<uint8_t> plain(32 * nt), led(32 * nt);
  expect(tmv_results_hash_many(nullptr, ptrs.data(), counts.data(), nullptr, nt, plain.data()) == 0, "hash_many", 0, 0);
  expect(tmv_results_hash_many(nullptr, ptrs.data(), counts.data(), leads.data(), nt, led.data()) == 0,
         "hash_many with leading leaves", 0, 0);
  uint8_t empty[32];
  tmh::TxResultsRootHost(nullptr, 0, nullptr, empty);
  expect(hex(empty, 32) == "e3b0c44298fc1c149afbf4c8996fb92427ae41e4649b934ca495991b7852b855", "empty tree", 0, 0);
  for (uint32_t t = 0; t < nt; t++) {
    uint8_t one[32];
    tmh::TxResultsRootHost(ptrs[t], counts[t], nullptr, one);
    expect(std::memcmp(one, plain.data() + 32 * t, 32) == 0, "root", t, 0);
    tmh::TxResultsRootHost(ptrs[t], counts[t], &leads[t], one);
    expect(std::memcmp(one, led.data() + 32 * t, 32) == 0, "root with a leading leaf", t, 0);
    expect(std::memcmp(plain.data() + 32 * t, led.data() + 32 * t, 32) != 0, "the leading leaf counts", t, 0);
  }
  expect(std::memcmp(plain.data(), empty, 32) == 0, "tree without results", 0, 0);
  // a one-result tree is its leaf hash: SHA-256(0x00 || enc)
  {
    tmh::Bytes enc{0};
    tmh::AppendTxResultProto(held[1][0], enc);
    tmh::Digest d;
    tmh::Sha256Bytes(d.w, nullptr, 0, enc.data(), enc.size());
    uint8_t leaf[32];
    for (int i = 0; i < 8; i++)
      for (int b = 0; b < 4; b++) leaf[4 * i + b] = (uint8_t)(d.w[i] >> (24 - 8 * b));
    expect(std::memcmp(leaf, plain.data() + 32, 32) == 0, "one-leaf tree", 0, 0);
  }
  expect(tmv_results_hash_many(nullptr, nullptr, counts.data(), nullptr, 1, plain.data()) == TMV_ERR_ARG, "null lists", 0, 0);
  const tmv_tx_result *null_list = nullptr;
  uint32_t two = 2;
  expect(tmv_results_hash_many(nullptr, &null_list, &two, nullptr, 1, plain.data()) == TMV_ERR_ARG, "null list", 0, 0);
  expect(tmv_results_hash_many(nullptr, nullptr, nullptr, nullptr, 0, nullptr) == 0, "no lists", 0, 0);

  // HashConsensusParams
  uint8_t ch[32];
  expect(tmv_consensus_params_hash(0, 0, ch) == 0 && std::memcmp(ch, empty, 32) == 0, "params (0, 0)", 0, 0);
  expect(tmv_consensus_params_hash(22020096, -1, ch) == 0, "params", 0, 0);
  expect(tmv_consensus_params_hash(1, 1, nullptr) == TMV_ERR_ARG, "params null", 0, 0);

  // the verify calls, error buffers shorter than the texts
  std::vector<tmv_block_results_in> items;
  for (uint32_t t = 0; t < nt; t++)
    items.push_back(tmv_block_results_in{(int64_t)t + 1, ptrs[t], counts[t], leads[t], tmv_bytes{led.data() + 32 * t, 32}});
  items[2].height = 0;
  items[3].height = -1;
  items[4].last_results_hash = tmv_bytes{plain.data() + 32 * 4, 32};
  items[5].last_results_hash = tmv_bytes{nullptr, 0};
  std::vector<int32_t> res(nt);
  std::vector<char> short_errs(16 * nt), errs(256 * nt);
  expect(tmv_block_results_verify(nullptr, items.data(), nt, res.data(), short_errs.data(), 16) == 4, "block results", 0, 0);
  for (uint32_t t = 0; t < nt; t++) expect(res[t] == (t >= 2 && t <= 5 ? 1 : 0), "block results verdict", t, res[t]);
  expect(std::string(short_errs.data() + 16 * 2) == "height must be ", "text cut to the stride", 0, 0);
  expect(tmv_block_results_verify(nullptr, items.data(), nt, res.data(), errs.data(), 256) == 4, "block results", 1, 0);
  expect(std::string(errs.data() + 256 * 3) == "height must be greater than zero", "height text", 0, 0);
  expect(std::string(errs.data() + 256 * 4).rfind("last results " + std::string(64, '0'), 0) != 0 &&
             std::string(errs.data() + 256 * 4).rfind("last results ", 0) == 0,
         "mismatch text", 0, 0);
  expect(tmv_block_results_verify(nullptr, items.data(), nt, res.data(), nullptr, 0) == 4, "no texts", 0, 0);
  expect(tmv_block_results_verify(nullptr, nullptr, 1, res.data(), nullptr, 0) == TMV_ERR_ARG, "null items", 0, 0);

  tmv_consensus_params_hash(22020096, -1, ch);
  std::vector<tmv_consensus_params_in> ps{{5, 22020096, -1, tmv_bytes{ch, 32}},
                                          {0, 22020096, -1, tmv_bytes{ch, 32}},
                                          {5, 22020097, -1, tmv_bytes{ch, 32}},
                                          {5, 22020096, -1, tmv_bytes{ch, 31}}};
  expect(tmv_consensus_params_verify(nullptr, ps.data(), 4, res.data(), short_errs.data(), 16) == 3, "params verify", 0, 0);
  expect(res[0] == 0 && res[1] == 1 && res[2] == 1 && res[3] == 1, "params verdicts", 0, 0);
  expect(tmv_consensus_params_verify(nullptr, ps.data(), 4, res.data(), errs.data(), 256) == 3, "params verify", 1, 0);
  expect(std::string(errs.data() + 256 * 2).rfind("params hash ", 0) == 0, "params text", 0, 0);
  std::printf("%d wrong\n", g_wrong);
  return g_wrong ? 1 : 0;
}
