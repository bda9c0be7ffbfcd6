// The host layer's query-proof and tx-proof code (csrc/host/tm_proof_ops_abi.cpp,
// no engine linked) under ASan + UBSan as a stand-alone program: every item of
// tests/golden/proof_ops_vectors.json through tmv_proof_ops_verify and
// tmv_tx_proofs_validate, all at once and one by one, results and texts
// compared with the file's; the inputs live in exactly-sized heap arrays (an
// overrun is an ASan report) and the texts in a buffer of the file's stride.
//   make -C tests/native/proofops san && oracle/_build/proofops_san tests/golden/proof_ops_vectors.json
#include <cstdio>
#include <cstring>
#include <fstream>
#include <map>
#include <memory>
#include <sstream>
#include <string>
#include <vector>

#include "../../../include/tmhost.h"

namespace {

// ---- a small JSON reader: objects, arrays, strings, integers, null
struct Json {
  enum Kind { Null, Num, Str, Arr, Obj } kind = Null;
  long long num = 0;
  std::string str;
  std::vector<Json> arr;
  std::map<std::string, Json> obj;
  const Json &at(const char *k) const { return obj.at(k); }
};

struct Reader {
  const std::string &s;
  size_t i = 0;
  explicit Reader(const std::string &s_) : s(s_) {}
  void ws() { while (i < s.size() && (s[i] == ' ' || s[i] == '\n' || s[i] == '\t' || s[i] == '\r')) i++; }
  bool eat(char c) { ws(); if (i < s.size() && s[i] == c) { i++; return true; } return false; }
  std::string string() {
    std::string out;
    i++;  // the opening quote
    while (i < s.size() && s[i] != '"') {
      if (s[i] == '\\' && i + 1 < s.size()) {
        const char e = s[++i];
        if (e == 'u' && i + 4 < s.size()) { out.push_back((char)std::stoi(s.substr(i + 1, 4), nullptr, 16)); i += 4; }
        else out.push_back(e == 'n' ? '\n' : e == 't' ? '\t' : e);
      } else {
        out.push_back(s[i]);
      }
      i++;
    }
    i++;
    return out;
  }
  Json value() {
    Json j;
    ws();
    if (i >= s.size()) return j;
    if (s[i] == '{') {
      j.kind = Json::Obj;
      i++;
      while (!eat('}')) {
        ws();
        const std::string k = string();
        eat(':');
        j.obj[k] = value();
        eat(',');
      }
    } else if (s[i] == '[') {
      j.kind = Json::Arr;
      i++;
      while (!eat(']')) {
        j.arr.push_back(value());
        eat(',');
      }
    } else if (s[i] == '"') {
      j.kind = Json::Str;
      j.str = string();
    } else if (s.compare(i, 4, "null") == 0) {
      i += 4;
    } else {
      j.kind = Json::Num;
      size_t used = 0;
      j.num = std::stoll(s.substr(i, 24), &used);
      i += used;
    }
    return j;
  }
};

// Byte strings in heap blocks of their exact size
struct Arena {
  std::vector<std::unique_ptr<uint8_t[]>> blocks;
  std::vector<std::unique_ptr<tmv_bytes[]>> lists;
  std::vector<std::unique_ptr<tmv_value_op[]>> ops;
  tmv_bytes hex(const std::string &h) {
    const size_t n = h.size() / 2;
    if (!n) return tmv_bytes{nullptr, 0};
    blocks.emplace_back(new uint8_t[n]);
    for (size_t k = 0; k < n; k++) blocks.back()[k] = (uint8_t)std::stoi(h.substr(2 * k, 2), nullptr, 16);
    return tmv_bytes{blocks.back().get(), (uint32_t)n};
  }
  const tmv_bytes *list(const Json &a) {
    if (a.arr.empty()) return nullptr;
    lists.emplace_back(new tmv_bytes[a.arr.size()]);
    for (size_t k = 0; k < a.arr.size(); k++) lists.back()[k] = hex(a.arr[k].str);
    return lists.back().get();
  }
  tmv_proof proof(const Json &p) {
    const Json &aunts = p.at("aunts");
    return tmv_proof{p.at("total").num, p.at("index").num, hex(p.at("leaf_hash").str), list(aunts),
                     (uint32_t)aunts.arr.size()};
  }
};

int g_wrong = 0;
void expect(bool ok, const char *what, const std::string &name) {
  if (!ok && g_wrong++ < 10) std::printf("WRONG %s: %s\n", what, name.c_str());
}

template <class In, class Fn>
void run(const char *what, Fn fn, const std::vector<In> &in, const Json &docs, size_t stride) {
  const uint32_t n = (uint32_t)in.size();
  auto check = [&](const In *p, uint32_t m, size_t first) {
    std::unique_ptr<int32_t[]> res(new int32_t[m]);
    std::unique_ptr<char[]> errs(new char[stride * m]);
    int want_failed = 0;
    for (uint32_t k = 0; k < m; k++) want_failed += docs.arr[first + k].at("error").kind != Json::Null;
    expect(fn(nullptr, p, m, res.get(), errs.get(), stride) == want_failed, what, "failed count");
    for (uint32_t k = 0; k < m; k++) {
      const Json &d = docs.arr[first + k];
      const Json &e = d.at("error");
      expect(res[k] == (e.kind != Json::Null), what, d.at("name").str);
      expect(std::string(errs.get() + stride * k) == (e.kind == Json::Null ? "" : e.str), what, d.at("name").str + " (text)");
    }
    expect(fn(nullptr, p, m, res.get(), nullptr, 0) == want_failed, what, "no text buffer");
    std::unique_ptr<char[]> cut(new char[8 * m]);  // texts longer than the stride are cut, never overrun
    expect(fn(nullptr, p, m, res.get(), cut.get(), 8) == want_failed, what, "short stride");
  };
  check(in.data(), n, 0);
  for (uint32_t k = 0; k < n; k++) {  // each alone, in an array of exactly one item
    std::unique_ptr<In[]> one(new In[1]);
    one[0] = in[k];
    check(one.get(), 1, k);
  }
  int32_t r = 0;
  expect(fn(nullptr, nullptr, 0, nullptr, nullptr, 0) == 0, what, "empty call");
  expect(fn(nullptr, nullptr, 1, &r, nullptr, 0) == TMV_ERR_ARG, what, "null items");
}

}  // namespace

int main(int argc, char **argv) {
  if (argc != 2) { std::fprintf(stderr, "usage: proofops_san proof_ops_vectors.json\n"); return 2; }
  std::ifstream f(argv[1]);
  if (!f) { std::fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
  std::stringstream ss;
  ss << f.rdbuf();
  const std::string text = ss.str();
  Reader rd(text);
  const Json doc = rd.value();
  const size_t stride = (size_t)doc.at("err_stride").num;
  Arena ar;
  std::vector<tmv_proof_ops_in> ops_in;
  std::vector<std::unique_ptr<tmv_bytes>> values;
  for (const Json &d : doc.at("proof_ops").arr) {
    const Json &ops = d.at("ops");
    tmv_proof_ops_in it{};
    if (!ops.arr.empty()) {
      ar.ops.emplace_back(new tmv_value_op[ops.arr.size()]);
      for (size_t k = 0; k < ops.arr.size(); k++)
        ar.ops.back()[k] = tmv_value_op{ar.hex(ops.arr[k].at("key").str), ar.proof(ops.arr[k].at("proof"))};
      it.ops = ar.ops.back().get();
    }
    it.n_ops = (uint32_t)ops.arr.size();
    it.root = ar.hex(d.at("root").str);
    it.keys = ar.list(d.at("keys"));
    it.n_keys = (uint32_t)d.at("keys").arr.size();
    if (d.at("value").kind != Json::Null) {
      values.emplace_back(new tmv_bytes(ar.hex(d.at("value").str)));
      it.value = values.back().get();
    }
    ops_in.push_back(it);
  }
  run("proof ops", tmv_proof_ops_verify, ops_in, doc.at("proof_ops"), stride);
  tmv_proof_ops_in none{};  // no ops and no value: the reference panics
  int32_t r = 0;
  expect(tmv_proof_ops_verify(nullptr, &none, 1, &r, nullptr, 0) == TMV_ERR_ARG, "proof ops", "no ops and no value");
  // aunts announced and not given: both calls refuse the call, neither reads through the null pointer
  uint8_t h32[32] = {0};
  tmv_value_op no_aunts{tmv_bytes{nullptr, 0}, tmv_proof{2, 0, tmv_bytes{h32, 32}, nullptr, 1}};
  tmv_bytes v{h32, 1};
  tmv_proof_ops_in bad_ops{&no_aunts, 1, tmv_bytes{h32, 32}, nullptr, 0, &v};
  expect(tmv_proof_ops_verify(nullptr, &bad_ops, 1, &r, nullptr, 0) == TMV_ERR_ARG, "proof ops", "null aunts");
  tmv_tx_proof_in bad_tx{tmv_bytes{h32, 32}, v, no_aunts.proof, tmv_bytes{h32, 32}};
  expect(tmv_tx_proofs_validate(nullptr, &bad_tx, 1, &r, nullptr, 0) == TMV_ERR_ARG, "tx proofs", "null aunts");
  std::vector<tmv_tx_proof_in> tx_in;
  for (const Json &d : doc.at("tx_proofs").arr)
    tx_in.push_back(tmv_tx_proof_in{ar.hex(d.at("root_hash").str), ar.hex(d.at("data").str), ar.proof(d.at("proof")),
                                    ar.hex(d.at("data_hash").str)});
  run("tx proofs", tmv_tx_proofs_validate, tx_in, doc.at("tx_proofs"), stride);
  std::printf("%zu + %zu items\n%d wrong\n", ops_in.size(), tx_in.size(), g_wrong);
  return g_wrong ? 1 : 0;
}
