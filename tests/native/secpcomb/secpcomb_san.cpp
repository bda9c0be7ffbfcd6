// Stand-alone ASan + UBSan check of the comb-table code of secp256k1.h (the
// cached-key path's host build): every vector of
// tests/golden/secp256k1_vectors.json (one JSON object per line) through
// build_key_comb + secp256k1_verify_comb, against the file's verdict and
// secp256k1_verify's.  Each comb lives in an exact-size heap block, so a read
// or write past a table is an ASan report.  Its own main; nothing is loaded
// into an interpreter.
//   make -C tests/native/secpcomb san && oracle/_build/secpcomb_san tests/golden/secp256k1_vectors.json
#include <cstdio>
#include <fstream>
#include <map>
#include <string>
#include <vector>

#include "../../../tendermint_amd/csrc/secp256k1.h"

using namespace tmv::secp;

static bool field(const std::string &line, const char *key, std::string &out) {
  const std::string k = std::string("\"") + key + "\":\"";
  const size_t at = line.find(k);
  if (at == std::string::npos) return false;
  const size_t end = line.find('"', at + k.size());
  if (end == std::string::npos) return false;
  out = line.substr(at + k.size(), end - at - k.size());
  return true;
}

static std::vector<uint8_t> unhex(const std::string &h) {
  std::vector<uint8_t> b(h.size() / 2);
  for (size_t i = 0; i < b.size(); i++) b[i] = (uint8_t)std::stoi(h.substr(2 * i, 2), nullptr, 16);
  return b;
}

struct KeyComb {
  bool ok;
  std::vector<uint32_t> w;
};

int main(int argc, char **argv) {
  if (argc != 2) { std::fprintf(stderr, "usage: secpcomb_san vectors.json\n"); return 2; }
  std::ifstream f(argv[1]);
  std::string line;
  std::map<std::string, KeyComb> combs;
  int n = 0, wrong = 0;
  while (std::getline(f, line)) {
    std::string name, pk, msg, sig;
    if (!field(line, "pk", pk) || !field(line, "msg", msg) || !field(line, "sig", sig) || !field(line, "name", name))
      continue;
    const bool want = line.find("\"valid\":true") != std::string::npos;
    const std::vector<uint8_t> p = unhex(pk), m = unhex(msg), s = unhex(sig);
    if (p.size() != 33 || s.size() != 64) { std::fprintf(stderr, "unexpected sizes: %s\n", name.c_str()); return 1; }
    auto it = combs.find(pk);
    if (it == combs.end()) {
      KeyComb c;
      c.w.resize(kCombWords);
      c.ok = build_key_comb(c.w.data(), p.data());
      it = combs.emplace(pk, std::move(c)).first;
    }
    uint32_t st[8];
    sha256_words(st, m.data(), (uint32_t)m.size());
    std::vector<uint8_t> z(32);
    for (int i = 0; i < 8; i++)
      for (int k = 0; k < 4; k++) z[4 * i + k] = (uint8_t)(st[i] >> (24 - 8 * k));
    const bool got = secp256k1_verify_comb(it->second.ok, it->second.w.data(), z.data(), s.data());
    const bool plain = secp256k1_verify(p.data(), z.data(), s.data());
    if (got != want || plain != want) { std::fprintf(stderr, "verdict differs: %s\n", name.c_str()); wrong++; }
    n++;
  }
  std::printf("%d vectors, %zu keys, %d wrong\n", n, combs.size(), wrong);
  return n >= 400 && wrong == 0 ? 0 : 1;
}
