// The host layer's block code (csrc/host/tm_block_abi.cpp and
// csrc/host/commit_encode.h, no engine linked) under ASan + UBSan as a
// stand-alone program: CommitSig encodings of every length class written into
// exactly-sized heap buffers (an overrun is an ASan report), Commit.Hash of
// commits of many sizes, and Block.ValidateBasic over a window whose blocks
// fail at every step, with error buffers shorter than the texts.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../../include/tmhost.h"
#include "host/commit_encode.h"

static int g_wrong = 0;
static void expect(bool ok, const char *what, uint64_t a, uint64_t b) {
  if (!ok) {
    if (g_wrong++ < 10) std::printf("WRONG %s (%llu, %llu)\n", what, (unsigned long long)a, (unsigned long long)b);
  }
}

struct Sig {
  std::vector<uint8_t> addr, sig;
  tmv_commit_sig c;
};

// heap copies of exactly the given sizes, so a read past either end is reported
static Sig make_sig(uint8_t flag, uint32_t addr_len, int64_t secs, int32_t nanos, uint32_t sig_len) {
  Sig s;
  s.addr.assign(addr_len, 0xa5);
  s.sig.assign(sig_len, 0x5a);
  s.c = tmv_commit_sig{flag, nullptr, addr_len, secs, nanos, nullptr, sig_len};
  return s;
}
static void fix(std::vector<Sig> &v) {
  for (Sig &s : v) {
    s.c.validator_address = s.addr.empty() ? nullptr : s.addr.data();
    s.c.signature = s.sig.empty() ? nullptr : s.sig.data();
  }
}

static size_t want_len(const tmv_commit_sig &s) {
  const uint64_t sec = (uint64_t)s.ts_seconds, nan = (uint64_t)(int64_t)s.ts_nanos;
  const size_t ts = (sec ? 1 + tmh::UvarintLen(sec) : 0) + (nan ? 1 + tmh::UvarintLen(nan) : 0);
  return (s.block_id_flag ? 1 + tmh::UvarintLen(s.block_id_flag) : 0) +
         (s.validator_address_len ? 1 + tmh::UvarintLen(s.validator_address_len) + s.validator_address_len : 0) + 2 +
         ts + (s.signature_len ? 1 + tmh::UvarintLen(s.signature_len) + s.signature_len : 0);
}

int main() {
  // the encoder, every combination of the length classes
  std::vector<Sig> sigs;
  const int64_t secs[] = {0, 1, -1, -62135596800LL, 253402300799LL, INT64_MIN, INT64_MAX};
  const int32_t nanos[] = {0, 1, 999999999, -1, INT32_MIN};
  for (uint8_t flag : {0, 1, 2, 3, 127, 128, 255})
    for (uint32_t al : {0u, 19u, 20u, 21u, 200u})
      for (int64_t sc : secs)
        for (int32_t nn : nanos)
          for (uint32_t sl : {0u, 1u, 20u, 21u, 28u, 29u, 30u, 63u, 64u, 65u, 300u}) sigs.push_back(make_sig(flag, al, sc, nn, sl));
  fix(sigs);
  for (const Sig &s : sigs) {
    tmh::Bytes out;
    tmh::AppendCommitSigProto(s.c, out);
    expect(out.size() == want_len(s.c), "encoded length", out.size(), want_len(s.c));
  }

  // Commit.Hash of commits of many sizes, nil commits between them
  std::vector<tmv_commit> commits;
  std::vector<std::vector<tmv_commit_sig>> held;
  size_t at = 0;
  for (uint32_t n : {0u, 1u, 2u, 3u, 64u, 65u, 128u, 129u, 257u, 1000u}) {
    held.emplace_back();
    for (uint32_t i = 0; i < n; i++) held.back().push_back(sigs[(at++) % sigs.size()].c);
  }
  for (auto &h : held)
    commits.push_back(tmv_commit{5, 0, tmv_block_id{nullptr, 0, 0, nullptr, 0}, h.empty() ? nullptr : h.data(),
                                 (uint32_t)h.size()});
  std::vector<const tmv_commit *> ptrs;
  for (size_t i = 0; i < commits.size(); i++) {
    ptrs.push_back(&commits[i]);
    if (i % 3 == 1) ptrs.push_back(nullptr);
  }
  std::vector<uint8_t> hashes(32 * ptrs.size()), has(ptrs.size());
  expect(tmv_commit_hash_many(nullptr, ptrs.data(), (uint32_t)ptrs.size(), hashes.data(), has.data()) == 0,
         "commit_hash_many", 0, 0);
  for (size_t i = 0; i < ptrs.size(); i++) {
    expect(has[i] == (ptrs[i] ? 1 : 0), "has_hash", i, has[i]);
    if (!ptrs[i]) continue;
    uint8_t one[32];
    tmh::CommitHashHost(*ptrs[i], one);
    expect(std::memcmp(one, hashes.data() + 32 * i, 32) == 0, "commit hash", i, 0);
  }
  tmv_commit bad = commits[3];
  bad.sigs = nullptr;
  const tmv_commit *bp = &bad;
  expect(tmv_commit_hash_many(nullptr, &bp, 1, hashes.data(), nullptr) == TMV_ERR_ARG, "null sigs", 0, 0);

  // Block.ValidateBasic: a good block, then one failure per step
  std::vector<uint8_t> h32(32, 7), addr(20, 9), tx0(100, 1), tx1(1, 2), ev(33, 3);
  std::vector<tmv_bytes> txs{{tx0.data(), 100}, {tx1.data(), 1}, {nullptr, 0}}, evs{{ev.data(), 33}};
  std::vector<tmv_commit_sig> good_sigs;
  std::vector<Sig> gs;
  for (int i = 0; i < 5; i++) gs.push_back(make_sig(2, 20, 1577836800 + i, i, 64));
  gs.push_back(make_sig(1, 0, -62135596800LL, 0, 0));
  fix(gs);
  for (Sig &s : gs) good_sigs.push_back(s.c);
  tmv_commit lc{4, 0, tmv_block_id{h32.data(), 32, 1, h32.data(), 32}, good_sigs.data(), (uint32_t)good_sigs.size()};
  uint8_t lch[32], dh[32], eh[32];
  tmh::CommitHashHost(lc, lch);
  // the data and evidence hashes come from a first call's error texts
  tmv_block blk{};
  blk.header.version_block = 11;
  blk.header.chain_id = "san";
  blk.header.height = 5;
  blk.header.last_commit_hash = tmv_bytes{lch, 32};
  blk.header.validators_hash = tmv_bytes{h32.data(), 32};
  blk.header.proposer_address = tmv_bytes{addr.data(), 20};
  blk.txs = txs.data();
  blk.n_txs = (uint32_t)txs.size();
  blk.evidence = evs.data();
  blk.n_evidence = 1;
  blk.last_commit = &lc;
  auto hex = [](const std::string &t, size_t at_, uint8_t out[32]) {
    for (int i = 0; i < 32; i++) out[i] = (uint8_t)std::stoi(t.substr(at_ + 2 * i, 2), nullptr, 16);
  };
  int32_t res[8];
  std::vector<char> errs(256 * 8);
  uint8_t bh[32 * 8], hh[8];
  expect(tmv_blocks_validate_basic(nullptr, &blk, 1, res, errs.data(), 256, bh, hh) == 1, "data hash missing", 0, 0);
  std::string t(errs.data());
  expect(t.rfind("wrong Header.DataHash. Expected ", 0) == 0, "data hash text", t.size(), 0);
  if (t.size() >= 32 + 64) hex(t, 32, dh);
  blk.header.data_hash = tmv_bytes{dh, 32};
  expect(tmv_blocks_validate_basic(nullptr, &blk, 1, res, errs.data(), 256, bh, hh) == 1, "evidence hash missing", 0, 0);
  t = errs.data();
  expect(t.rfind("wrong Header.EvidenceHash. Expected ", 0) == 0, "evidence hash text", t.size(), 0);
  if (t.size() >= 36 + 64) hex(t, 36, eh);
  blk.header.evidence_hash = tmv_bytes{eh, 32};
  std::vector<tmv_block> win(8, blk);
  win[1].header.height = 0;                                // invalid header
  win[2].last_commit = nullptr;                            // nil LastCommit
  tmv_commit neg = lc;
  neg.round = -1;
  win[3].last_commit = &neg;                               // wrong LastCommit
  win[4].header.last_commit_hash = tmv_bytes{h32.data(), 32};
  win[5].n_txs = 2;                                        // wrong DataHash
  win[6].n_evidence = 0;                                   // wrong EvidenceHash
  win[7].header.validators_hash = tmv_bytes{nullptr, 0};   // passes; Header.Hash is nil
  std::vector<char> short_errs(8 * 8);  // texts longer than the stride are cut, never overrun
  expect(tmv_blocks_validate_basic(nullptr, win.data(), 8, res, short_errs.data(), 8, bh, hh) == 6, "window", 0, 0);
  const int want_res[8] = {0, 1, 1, 1, 1, 1, 1, 0};
  for (int i = 0; i < 8; i++) expect(res[i] == want_res[i], "window result", i, res[i]);
  expect(hh[0] == 1 && hh[7] == 0, "has_hash of the window", hh[0], hh[7]);
  expect(tmv_blocks_validate_basic(nullptr, win.data(), 8, res, nullptr, 0, nullptr, nullptr) == 6, "no outputs", 0, 0);
  win[5].txs = nullptr;
  expect(tmv_blocks_validate_basic(nullptr, win.data(), 8, res, nullptr, 0, nullptr, nullptr) == TMV_ERR_ARG,
         "null txs", 0, 0);
  std::printf("%d wrong\n", g_wrong);
  return g_wrong ? 1 : 0;
}
