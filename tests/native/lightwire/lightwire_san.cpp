// The strict light-block scanner (csrc/host/light_wire.h) and the host path of
// tmv_light_blocks_validate_wire under ASan + UBSan, as a stand-alone program
// (make -C tests/native/lightwire san; run by tests/test_light_wire_sanitizers.py):
// the light blocks of tests/golden/light_wire_vectors.json, every truncation
// and every single-byte substitution of them (3 values per position), each
// copied into a heap buffer of exactly its length, so that a read past the
// block is a read past the allocation.  Checked besides: a golden light block
// gets the file's verdict text and hashes; the views agree with the result
// (none for a block that was not handled); every pointer of a handled block's
// views lies inside the block's bytes; a second call gives the same answer.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "../../../include/tmhost.h"

namespace {

constexpr size_t kStride = 256;
long checks = 0, wrong = 0;

std::vector<uint8_t> unhex(const std::string &s) {
  std::vector<uint8_t> o;
  for (size_t i = 0; i + 1 < s.size(); i += 2) o.push_back((uint8_t)std::stoi(s.substr(i, 2), nullptr, 16));
  return o;
}

// every "<key>": "<text>" of the file, in order
std::vector<std::string> values_of(const std::string &text, const std::string &key) {
  std::vector<std::string> out;
  const std::string pat = "\"" + key + "\": \"";
  for (size_t at = text.find(pat); at != std::string::npos; at = text.find(pat, at + 1)) {
    const size_t lo = at + pat.size(), hi = text.find('"', lo);
    out.push_back(text.substr(lo, hi - lo));
  }
  return out;
}

struct Verdict {
  int32_t result = -1, reason = -1;
  std::string text;
  uint8_t hash[32] = {}, vals_hash[32] = {}, has = 0;
};

bool inside(const uint8_t *p, uint32_t n, const uint8_t *lo, size_t len) {
  return n == 0 || (p >= lo && p + n <= lo + len);
}

void fail(const char *what) {
  wrong++;
  std::printf("%s\n", what);
}

// One light block through tmv_light_blocks_validate_wire from a heap copy of
// exactly its length.
Verdict run(const std::vector<uint8_t> &block, const char *chain_id) {
  uint8_t *heap = static_cast<uint8_t *>(std::malloc(block.size() ? block.size() : 1));
  if (!block.empty()) std::memcpy(heap, block.data(), block.size());
  const uint32_t off[2] = {0, (uint32_t)block.size()};
  Verdict v;
  char errs[kStride] = {};
  tmv_light_block_views *views = nullptr;
  const int rc = tmv_light_blocks_validate_wire(nullptr, chain_id, block.empty() ? nullptr : heap, off, 1, &v.result,
                                                &v.reason, errs, kStride, v.hash, &v.has, v.vals_hash, &views);
  checks++;
  if (rc < 0 || !views) {
    fail("wire call failed");
  } else {
    v.text = errs;
    const tmv_signed_header *sh = tmv_light_block_views_header(views, 0);
    const tmv_validator_set *vs = tmv_light_block_views_vals(views, 0);
    if ((v.reason == 0) != (v.result != TMV_WIRE_NOT_HANDLED)) fail("reason and result disagree");
    if (v.result == TMV_WIRE_NOT_HANDLED && (sh || vs || v.has)) fail("views or hashes of a block that was not handled");
    if (v.result == TMV_WIRE_OK && (!sh || !vs || !sh->header || !sh->commit || v.has != 3)) fail("a valid block without views");
    if (sh && sh->header) {
      const tmv_header &h = *sh->header;
      const tmv_bytes *f[9] = {&h.last_commit_hash, &h.data_hash, &h.validators_hash, &h.next_validators_hash,
                               &h.consensus_hash, &h.app_hash, &h.last_results_hash, &h.evidence_hash,
                               &h.proposer_address};
      for (const tmv_bytes *b : f)
        if (!inside(b->p, b->len, heap, block.size())) fail("a header field outside the block");
      if (!inside(h.last_block_id.hash, h.last_block_id.hash_len, heap, block.size())) fail("last_block_id outside");
    }
    if (sh && sh->commit)
      for (uint32_t i = 0; i < sh->commit->n_sigs; i++) {
        const tmv_commit_sig &s = sh->commit->sigs[i];
        if (!inside(s.signature, s.signature_len, heap, block.size()) ||
            !inside(s.validator_address, s.validator_address_len, heap, block.size()))
          fail("a commit signature outside the block");
      }
    if (vs) {
      if (vs->proposer_index >= (int32_t)vs->n_vals || (vs->n_vals && vs->proposer_index < 0)) fail("proposer index");
      for (uint32_t i = 0; i < vs->n_vals; i++) {
        const tmv_validator &x = vs->vals[i];
        if (!inside(x.address, x.address_len, heap, block.size()) || !inside(x.pub_key, x.pub_key_len, heap, block.size()))
          fail("a validator outside the block");
        if (x.pub_key_len != (x.key_kind == TMV_KIND_SECP256K1 ? 33u : 32u)) fail("a key of the wrong size in a view");
      }
    }
    // the scanner alone agrees
    int32_t r2 = -1;
    tmv_light_block_views *v2 = nullptr;
    const int rc2 = tmv_light_blocks_parse_wire(block.empty() ? nullptr : heap, off, 1, &r2, &v2);
    if (rc2 < 0 || r2 != v.reason) fail("parse_wire gives another reason");
    tmv_light_block_views_free(v2);
  }
  tmv_light_block_views_free(views);
  std::free(heap);
  return v;
}

}  // namespace

int main(int argc, char **argv) {
  if (argc < 2) {
    std::printf("usage: lightwire_san light_wire_vectors.json\n");
    return 2;
  }
  std::ifstream f(argv[1]);
  std::stringstream ss;
  ss << f.rdbuf();
  const auto wires = values_of(ss.str(), "wire"), hashes = values_of(ss.str(), "header_hash"),
             vhashes = values_of(ss.str(), "vals_hash"), chains = values_of(ss.str(), "chain_id"),
             errors = values_of(ss.str(), "error");
  if (wires.empty() || wires.size() != hashes.size() || wires.size() != vhashes.size() ||
      wires.size() != chains.size() || wires.size() != errors.size()) {
    std::printf("no vectors in %s\n", argv[1]);
    return 2;
  }
  for (size_t k = 0; k < wires.size(); k++) {
    const std::vector<uint8_t> w = unhex(wires[k]);
    const char *chain = chains[k].c_str();
    const Verdict g = run(w, chain);
    if (g.result == TMV_WIRE_NOT_HANDLED || g.has != 3 || std::memcmp(g.hash, unhex(hashes[k]).data(), 32) != 0 ||
        std::memcmp(g.vals_hash, unhex(vhashes[k]).data(), 32) != 0 || g.text != errors[k]) {
      wrong++;
      std::printf("vector %zu: not handled, other hashes or another text '%s'\n", k, g.text.c_str());
    }
    for (size_t n = 0; n < w.size(); n++) run(std::vector<uint8_t>(w.begin(), w.begin() + n), chain);
    for (size_t p = 0; p < w.size(); p++)
      for (uint8_t x : {(uint8_t)(w[p] ^ 0x01), (uint8_t)(w[p] ^ 0x80), (uint8_t)(w[p] + 0x3b)}) {
        std::vector<uint8_t> m = w;
        m[p] = x;
        run(m, chain);
      }
  }
  std::printf("%ld checks\n%ld wrong\n", checks, wrong);
  return wrong ? 1 : 0;
}
