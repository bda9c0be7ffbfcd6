// Stand-alone ASan + UBSan check of the host build of secp256k1.h: runs every
// vector of tests/golden/secp256k1_vectors.json (one JSON object per line)
// through secp256k1_verify_msg and compares the verdicts.  Its own main;
// nothing is loaded into an interpreter.
//   make -C tests/native/secp san && oracle/_build/secp_san tests/golden/secp256k1_vectors.json
#include <cstdio>
#include <fstream>
#include <string>
#include <vector>

#include "../../../tendermint_amd/csrc/secp256k1.h"

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

int main(int argc, char **argv) {
  if (argc != 2) { std::fprintf(stderr, "usage: secp_san vectors.json\n"); return 2; }
  std::ifstream f(argv[1]);
  std::string line;
  int n = 0, wrong = 0;
  while (std::getline(f, line)) {
    std::string name, pk, msg, sig;
    if (!field(line, "pk", pk) || !field(line, "msg", msg) || !field(line, "sig", sig) || !field(line, "name", name))
      continue;
    const bool want = line.find("\"valid\":true") != std::string::npos;
    const std::vector<uint8_t> p = unhex(pk), m = unhex(msg), s = unhex(sig);
    // exact-size copies, so a read past any of the three buffers is an ASan report
    const bool got = tmv::secp::secp256k1_verify_msg(p.data(), p.size(), m.data(), m.size(), s.data(), s.size());
    if (got != want) { std::fprintf(stderr, "verdict differs: %s\n", name.c_str()); wrong++; }
    n++;
  }
  std::printf("%d vectors, %d wrong\n", n, wrong);
  return n >= 400 && wrong == 0 ? 0 : 1;
}
