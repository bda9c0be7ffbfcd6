// The strict scanner (csrc/host/block_wire.h) and the host path of
// tmv_blocks_validate_wire under ASan + UBSan, as a stand-alone program
// (make -C tests/native/blockwire san; run by tests/test_block_wire_sanitizers.py):
// the blocks of tests/golden/block_wire_vectors.json, every truncation and
// every single-byte substitution of them (3 values per position), each copied
// into a heap buffer of exactly its length, so that a read past the block is
// a read past the allocation.  Checked besides: a golden block is handled and
// hashes to the file's header_hash; no truncation is handled, but the cut in
// front of last_commit, which leaves the same block with a nil commit; a mutated block
// that is handled gets from tmv_blocks_validate_basic over its view the
// verdict, text and hash that the wire call gave.
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

// every "<key>": "<hex>" of the file, in order
std::vector<std::vector<uint8_t>> values_of(const std::string &text, const std::string &key) {
  std::vector<std::vector<uint8_t>> out;
  const std::string pat = "\"" + key + "\": \"";
  for (size_t at = text.find(pat); at != std::string::npos; at = text.find(pat, at + 1)) {
    const size_t lo = at + pat.size(), hi = text.find('"', lo);
    out.push_back(unhex(text.substr(lo, hi - lo)));
  }
  return out;
}

struct Verdict {
  int32_t result = -1, reason = -1;
  std::string text;
  uint8_t hash[32] = {}, has = 0;
  bool nil_commit = false;  // handled, and the view has no last commit
};

// One block through tmv_blocks_validate_wire from a heap copy of exactly its
// length; a handled block again through the struct path over its view.
Verdict run(const std::vector<uint8_t> &block) {
  uint8_t *heap = static_cast<uint8_t *>(std::malloc(block.size() ? block.size() : 1));
  if (!block.empty()) std::memcpy(heap, block.data(), block.size());
  const uint32_t off[2] = {0, (uint32_t)block.size()};
  Verdict v;
  char errs[kStride] = {};
  uint32_t total = 0;
  uint8_t phash[32];
  tmv_block_views *views = nullptr;
  const int rc = tmv_blocks_validate_wire(nullptr, block.empty() ? nullptr : heap, off, 1, 64, &v.result, &v.reason, errs,
                                          kStride, v.hash, &v.has, &total, phash, &views);
  checks++;
  if (rc < 0 || !views) {
    wrong++;
    std::printf("wire call failed (%d)\n", rc);
  } else {
    v.text = errs;
    const tmv_block *b = tmv_block_views_block(views, 0);
    if ((b != nullptr) != (v.result != TMV_WIRE_NOT_HANDLED) || (v.reason == 0) != (b != nullptr)) {
      wrong++;
      std::printf("view and result disagree\n");
    } else if (b) {
      v.nil_commit = b->last_commit == nullptr;
      int32_t r2 = -1;
      char e2[kStride] = {};
      uint8_t h2[32] = {}, has2 = 0;
      const int rc2 = tmv_blocks_validate_basic(nullptr, b, 1, &r2, e2, kStride, h2, &has2);
      if (rc2 < 0 || r2 != v.result || v.text != e2 || has2 != v.has || std::memcmp(h2, v.hash, 32) != 0) {
        wrong++;
        std::printf("struct path differs: %d '%s' vs %d '%s'\n", v.result, v.text.c_str(), r2, e2);
      }
    }
  }
  tmv_block_views_free(views);
  std::free(heap);
  return v;
}

}  // namespace

int main(int argc, char **argv) {
  if (argc < 2) {
    std::printf("usage: blockwire_san block_wire_vectors.json\n");
    return 2;
  }
  std::ifstream f(argv[1]);
  std::stringstream ss;
  ss << f.rdbuf();
  const auto wires = values_of(ss.str(), "wire"), hashes = values_of(ss.str(), "header_hash");
  if (wires.empty() || wires.size() != hashes.size()) {
    std::printf("no vectors in %s\n", argv[1]);
    return 2;
  }
  for (size_t k = 0; k < wires.size(); k++) {
    const std::vector<uint8_t> &w = wires[k];
    const Verdict g = run(w);
    if (g.result == TMV_WIRE_NOT_HANDLED || !g.has || std::memcmp(g.hash, hashes[k].data(), 32) != 0) {
      wrong++;
      std::printf("vector %zu: not handled or another hash\n", k);
    }
    for (size_t n = 0; n < w.size(); n++) {
      const Verdict t = run(std::vector<uint8_t>(w.begin(), w.begin() + n));
      // cut right in front of last_commit (tag 22), what is left is the canonical block with a nil commit
      const bool nil_form = w[n] == 0x22 && t.nil_commit;
      if (t.result != TMV_WIRE_NOT_HANDLED && !nil_form) {
        wrong++;
        std::printf("vector %zu cut to %zu bytes was handled\n", k, n);
      }
    }
    for (size_t p = 0; p < w.size(); p++)
      for (uint8_t x : {(uint8_t)(w[p] ^ 0x01), (uint8_t)(w[p] ^ 0x80), (uint8_t)(w[p] + 0x3b)}) {
        std::vector<uint8_t> m = w;
        m[p] = x;
        run(m);
      }
  }
  std::printf("%ld checks\n%ld wrong\n", checks, wrong);
  return wrong ? 1 : 0;
}
