// The vote-extension host layer (csrc/host/tm_vote_ext_abi.cpp,
// vote_ext_encode.h, ripemd160.h; no engine linked) under ASan + UBSan as a
// stand-alone program: extension messages of every length class against the
// device's sizing (csrc/vote_ext.h), the encoders with output buffers shorter
// than the message, and tmv_verify_extended_votes over every mode x vote type
// x nil / non-nil block with extensions and signatures held in exactly-sized
// heap buffers (a read past either end is an ASan report), through both the
// host-built and the device-built message path of the engine double.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "engine_double.h"
#include "host/ripemd160.h"
#include "host/tm_light.h"
#include "vote_ext.h"

static int g_wrong = 0;
static void expect(bool ok, const char *what, uint64_t a, uint64_t b) {
  if (!ok && g_wrong++ < 10) std::printf("WRONG %s (%llu, %llu)\n", what, (unsigned long long)a, (unsigned long long)b);
}

// A keyed hash as the "signature scheme": sig = 64 bytes of FNV-1a over key || message.
static void fake_sign(const uint8_t *pk, size_t pkl, const uint8_t *msg, size_t mlen, uint8_t sig[64]) {
  uint64_t h = 1469598103934665603ull;
  for (size_t i = 0; i < pkl; i++) h = (h ^ pk[i]) * 1099511628211ull;
  for (size_t i = 0; i < mlen; i++) h = (h ^ msg[i]) * 1099511628211ull;
  for (int i = 0; i < 64; i++) {
    h = (h ^ (uint64_t)i) * 1099511628211ull;
    sig[i] = (uint8_t)(h >> 32);
  }
}
int8_t voteext_status(uint8_t, const uint8_t *pk, const uint8_t *msg, size_t mlen, const uint8_t *sig) {
  uint8_t want[64];
  fake_sign(pk, 32, msg, mlen, want);
  return std::memcmp(want, sig, 64) == 0 ? 1 : 0;
}

using Buf = std::unique_ptr<uint8_t[]>;
static Buf heap(const uint8_t *p, size_t n) {  // exactly n bytes (n == 0: a 1-byte block nobody may read)
  Buf b(new uint8_t[n ? n : 1]);
  if (n) std::memcpy(b.get(), p, n);
  return b;
}

int main() {
  // RIPEMD-160 test vectors of the paper
  const struct { const char *m, *hex; } rv[] = {{"", "9c1185a5c5e9fc54612808977ee8f548b2258d31"},
                                                {"abc", "8eb208f7e05d987a9b044a8e98c6b087f15a0bfc"},
                                                {"message digest", "5d0689ef49d2fae572b881b123a85ffa21595f36"}};
  for (const auto &v : rv) {
    uint8_t out[20];
    char hex[41];
    Buf m = heap(reinterpret_cast<const uint8_t *>(v.m), std::strlen(v.m));
    tmh::Ripemd160(m.get(), std::strlen(v.m), out);
    for (int i = 0; i < 20; i++) std::snprintf(hex + 2 * i, 3, "%02x", out[i]);
    expect(std::strcmp(hex, v.hex) == 0, "ripemd160", std::strlen(v.m), 0);
  }

  // encoder vs the device's sizing, and short output buffers
  const std::string chains[] = {"", "c", "test_chain_id", std::string(127, 'x'), std::string(128, 'y'), std::string(300, 'z')};
  const uint32_t lens[] = {0, 1, 92, 93, 127, 128, 255, 16347, 16348, 16383, 16384, 70000};
  for (const std::string &c : chains)
    for (int64_t h : {(int64_t)0, (int64_t)1, INT64_MIN})
      for (int32_t r : {0, 1, -1}) {
        const tmh::Bytes tail = tmh::EncodeVoteExtTail(c, h, r);
        expect(tmv_vote_extension_template_encode(c.c_str(), h, r, nullptr, 0) == tail.size(), "template length", 0, 0);
        for (uint32_t e : lens) {
          Buf ext = heap(std::vector<uint8_t>(e, 0xab).data(), e);
          tmh::Bytes m;
          tmh::AppendVoteExtFromTail(m, tail.data(), tail.size(), ext.get(), e);
          expect(m.size() == tmv::vote_ext_msg_len((uint32_t)tail.size(), e), "device sizing", m.size(), e);
          for (size_t cap : {(size_t)0, (size_t)1, m.size() - 1, m.size()}) {
            Buf out(new uint8_t[cap ? cap : 1]);
            const size_t n = tmv_vote_extension_sign_bytes(c.c_str(), h, r, ext.get(), e, out.get(), cap);
            expect(n == m.size(), "sign bytes length", n, m.size());
            expect(cap == 0 || std::memcmp(out.get(), m.data(), cap) == 0, "sign bytes", cap, e);
          }
        }
      }
  {
    uint8_t out[64];
    const size_t n = tmv_vote_extension_sign_bytes("test_chain_id", 1, 0, reinterpret_cast<const uint8_t *>("extension"), 9, out, 64);
    static const uint8_t want[36] = {0x23, 0x0a, 0x09, 'e', 'x', 't', 'e', 'n', 's', 'i', 'o', 'n', 0x11, 1, 0, 0, 0, 0, 0, 0, 0,
                                     0x22, 0x0d, 't', 'e', 's', 't', '_', 'c', 'h', 'a', 'i', 'n', '_', 'i', 'd'};
    expect(n == 36 && std::memcmp(out, want, 36) == 0, "vector 1", n, 0);
    expect(tmv_vote_extension_sign_bytes("", 0, 0, nullptr, 0, out, 64) == 1 && out[0] == 0, "vector 2", 0, 0);
  }

  // tmv_verify_extended_votes: mode x type x nil x (good, bad vote signature,
  // bad extension signature, extension signature lengths 0 / 63 / 65, wrong address)
  struct Held {
    Buf addr, sig, pk, ext, esig, bh, ph;
    tmv_block_id bid;
  };
  tmv_ctx ctx{0};
  const std::string chain = "san-chain";
  for (int pass = 0; pass < 2; pass++) {
    setenv("TMV_VOTE_EXT_DEVICE_MIN", pass ? "0" : "4000000000", 1);
    for (int mode = 0; mode < 3; mode++) {
      std::vector<Held> held;
      std::vector<tmv_ext_vote_in> in;
      std::vector<int> want, want_failed;
      int k = 0;
      for (int type : {1, 2})
        for (bool nil : {true, false})
          for (int variant = 0; variant < 7; variant++, k++) {
            Held hd;
            uint8_t pk[32];
            for (int i = 0; i < 32; i++) pk[i] = (uint8_t)(k * 7 + i);
            // the address the host layer derives (SHA-256(pk)[:20]); wrong in variant 6
            uint32_t st[8];
            tmh::Sha256Bytes(st, nullptr, 0, pk, 32);
            uint8_t addr[20];
            for (int i = 0; i < 20; i++) addr[i] = (uint8_t)(st[i / 4] >> (24 - 8 * (i % 4)));
            if (variant == 6) addr[3] ^= 1;
            const uint32_t el = (uint32_t)(k * 37 % 300);
            std::vector<uint8_t> ext(el);
            for (uint32_t i = 0; i < el; i++) ext[i] = (uint8_t)(i * 3 + k);
            std::vector<uint8_t> h32(32, (uint8_t)(k + 1));
            tmh::BlockID bid;
            if (!nil) {
              bid.hash = h32;
              bid.part_set_header.total = 3;
              bid.part_set_header.hash = h32;
            }
            tmh::Bytes vm, em;
            tmh::AppendVoteSignBytes(vm, chain, type, 5 + k % 2, k % 3, nil ? nullptr : &bid, tmh::Timestamp{1600000000 + k, k});
            tmh::AppendVoteExtSignBytes(em, chain, 5 + k % 2, k % 3, ext.data(), el);
            uint8_t sig[64], esig[65] = {0};
            fake_sign(pk, 32, vm.data(), vm.size(), sig);
            fake_sign(pk, 32, em.data(), em.size(), esig);
            if (variant == 1) sig[9] ^= 4;
            if (variant == 2) esig[60] ^= 1;
            const uint32_t esl = variant == 3 ? 0 : variant == 4 ? 63 : variant == 5 ? 65 : 64;
            hd.addr = heap(addr, 20), hd.sig = heap(sig, 64), hd.pk = heap(pk, 32), hd.ext = heap(ext.data(), el);
            hd.esig = heap(esig, esl), hd.bh = heap(h32.data(), 32), hd.ph = heap(h32.data(), 32);
            held.push_back(std::move(hd));
            const bool ext_checked = mode != 0 && type == 2 && !nil;
            int w = 0, f = 0;
            if (mode != 2 && variant == 6) w = TMV_VOTE_ERR_INVALID_ADDRESS;
            else if (mode != 2 && variant == 1) w = TMV_VOTE_ERR_INVALID_SIGNATURE, f = 1;
            else if (ext_checked && variant >= 2 && variant <= 5) w = TMV_VOTE_ERR_INVALID_SIGNATURE, f = 2;
            want.push_back(w);
            want_failed.push_back(f);
            tmv_ext_vote_in x{};
            x.vote.type = type, x.vote.height = 5 + k % 2, x.vote.round = k % 3;
            x.vote.ts_seconds = 1600000000 + k, x.vote.ts_nanos = k;
            x.vote.validator_address_len = 20, x.vote.signature_len = 64, x.vote.key_kind = TMV_KIND_ED25519;
            x.vote.pub_key_len = 32, x.extension_len = el, x.extension_signature_len = esl;
            in.push_back(x);
          }
      for (size_t i = 0; i < in.size(); i++) {  // pointers once the buffers stopped moving
        Held &hd = held[i];
        const bool nil = (i / 7) % 2 == 0;
        hd.bid = tmv_block_id{hd.bh.get(), 32, 3, hd.ph.get(), 32};
        in[i].vote.block_id = nil ? nullptr : &hd.bid;
        in[i].vote.validator_address = hd.addr.get(), in[i].vote.signature = hd.sig.get();
        in[i].vote.pub_key = hd.pk.get(), in[i].extension = in[i].extension_len ? hd.ext.get() : nullptr;
        in[i].extension_signature = in[i].extension_signature_len ? hd.esig.get() : nullptr;
      }
      std::vector<int32_t> res(in.size(), -1);
      std::vector<uint8_t> failed(in.size(), 9);
      const int before = voteext_calls_host_built + voteext_calls_device_built;
      const int rc = tmv_verify_extended_votes(&ctx, mode, chain.c_str(), in.data(), (uint32_t)in.size(), res.data(), failed.data());
      int bad = 0;
      for (size_t i = 0; i < in.size(); i++) {
        expect(res[i] == want[i], "result", i, (uint64_t)(mode * 10 + pass));
        expect(failed[i] == want_failed[i], "failed_sig", i, (uint64_t)(mode * 10 + pass));
        bad += want[i] != 0;
      }
      expect(rc == bad, "return value", (uint64_t)rc, (uint64_t)bad);
      expect(voteext_calls_host_built + voteext_calls_device_built - before == 1, "one engine call", 0, 0);
      expect(tmv_verify_extended_votes(&ctx, mode, chain.c_str(), in.data(), (uint32_t)in.size(), res.data(), nullptr) == bad,
             "no failed_sig", 0, 0);
    }
  }
  expect(voteext_calls_device_built > 0 && voteext_calls_host_built > 0, "both paths ran", 0, 0);
  expect(tmv_verify_extended_votes(&ctx, 3, "", nullptr, 0, nullptr, nullptr) == TMV_ERR_ARG, "bad mode", 0, 0);
  expect(tmv_verify_extended_votes(&ctx, 1, nullptr, nullptr, 0, nullptr, nullptr) == 0, "empty call", 0, 0);
  std::printf("%d wrong\n", g_wrong);
  return g_wrong ? 1 : 0;
}
