// csrc/host/stage_layout.h under ASan + UBSan as a stand-alone program: layouts
// over a sweep of region sizes, every region written into a heap buffer of
// exactly dev_bytes (an overrun is an ASan report) and read back, the layouts
// of the entry points at their own limits, and check_offsets over exactly-sized
// offset arrays.
#include <cstdio>
#include <cstring>
#include <vector>

#include "host/stage_layout.h"

static int g_wrong = 0;
static void expect(bool ok, const char *what, uint64_t a, uint64_t b) {
  if (!ok && g_wrong++ < 10) std::printf("WRONG %s (%llu, %llu)\n", what, (unsigned long long)a, (unsigned long long)b);
}

enum Kind { kIn, kInPadded, kScratch, kOut };
struct Region {
  Kind kind;
  size_t bytes, spare, at;
};

// Builds the layout of `r` in order and checks what the header promises.
static tmh::StageLayout build(std::vector<Region> &r) {
  tmh::StageLayout L;
  for (Region &x : r)
    x.at = x.kind == kIn ? L.in(x.bytes, x.spare) : x.kind == kInPadded ? L.in_padded(x.bytes)
         : x.kind == kScratch ? L.scratch(x.bytes) : L.out(x.bytes);
  expect(L.in_bytes <= L.out_at, "in_bytes <= out_at", L.in_bytes, L.out_at);
  expect(L.out_at + L.out_bytes == L.dev_bytes, "out_at + out_bytes == dev_bytes", L.out_at + L.out_bytes, L.dev_bytes);
  expect(L.in_bytes % 16 == 0 && L.out_at % 16 == 0 && L.dev_bytes % 16 == 0, "spans aligned", L.in_bytes, L.out_at);
  for (size_t i = 0; i < r.size(); i++) {
    const size_t lo = r[i].kind == kInPadded ? r[i].at - 16 : r[i].at, hi = r[i].at + r[i].bytes + r[i].spare;
    expect(r[i].at % 16 == 0, "region aligned", i, r[i].at);
    const size_t span_lo = r[i].kind == kScratch ? L.in_bytes : r[i].kind == kOut ? L.out_at : 0;
    const size_t span_hi = r[i].kind == kScratch ? L.out_at : r[i].kind == kOut ? L.dev_bytes : L.in_bytes;
    expect(span_lo <= lo && hi <= span_hi, "region inside its span", i, hi);
    if (r[i].kind == kInPadded) expect(L.pad_at == r[i].at && r[i].at >= 16, "pad_at", L.pad_at, r[i].at);
    for (size_t j = 0; j < i; j++) {
      const size_t hj = r[j].at + r[j].bytes + r[j].spare;
      expect(hj <= lo, "regions disjoint and in order", j, i);
    }
  }
  return L;
}

// The same through memory: a distinct byte per region, zeros in the padding.
static void fill_and_read(std::vector<Region> &r) {
  const tmh::StageLayout L = build(r);
  std::vector<uint8_t> buf(L.dev_bytes, 0xee);
  if (L.pad_at) std::memset(buf.data() + L.pad_at - 16, 0, 16);
  for (size_t i = 0; i < r.size(); i++)
    if (r[i].bytes + r[i].spare) std::memset(buf.data() + r[i].at, (int)(i + 1), r[i].bytes + r[i].spare);
  for (size_t i = 0; i < r.size(); i++) {
    for (size_t k = 0; k < r[i].bytes + r[i].spare; k++)
      if (buf[r[i].at + k] != i + 1) { expect(false, "region overwritten", i, k); break; }
    if (r[i].kind == kInPadded)
      for (size_t k = 1; k <= 16; k++) expect(buf[r[i].at - k] == 0, "padding overwritten", i, k);
  }
}

static void offsets() {
  using tmh::Offsets;
  uint32_t span = 77;
  std::vector<uint32_t> a{0, 3, 3, 10, 12};
  expect(tmh::check_offsets(a.data(), 4, &span) == Offsets::kOk && span == 7, "ok", span, 7);
  expect(tmh::check_offsets(a.data(), 4, nullptr) == Offsets::kOk, "ok, no span wanted", 0, 0);
  std::vector<uint32_t> one{0};
  span = 77;
  expect(tmh::check_offsets(one.data(), 0, &span) == Offsets::kOk && span == 0, "n == 0", span, 0);
  std::vector<uint32_t> five{5};
  expect(tmh::check_offsets(five.data(), 0, &span) == Offsets::kFirstNotZero, "n == 0, first not zero", 0, 0);
  std::vector<uint32_t> b{1, 2, 3};
  expect(tmh::check_offsets(b.data(), 2, &span) == Offsets::kFirstNotZero, "first not zero", 0, 0);
  std::vector<uint32_t> c{0, 5, 4, 9};
  span = 77;
  expect(tmh::check_offsets(c.data(), 3, &span) == Offsets::kDecreasing && span == 77, "decreasing", span, 77);
  std::vector<uint32_t> d{2, 1};  // both wrong: the first entry is reported
  expect(tmh::check_offsets(d.data(), 1, &span) == Offsets::kFirstNotZero, "first not zero before decreasing", 0, 0);
  std::vector<uint32_t> e{0, 0xffffffffu};
  expect(tmh::check_offsets(e.data(), 1, &span) == Offsets::kOk && span == 0xffffffffu, "widest span", span, 0);
}

int main() {
  expect(sizeof(size_t) >= 8, "size_t is 64 bits", sizeof(size_t), 8);
  // 0, 1, around 16, and 8n / 4(n+1) / n for n = 1 mod 4: none of the latter a multiple of 16
  std::vector<size_t> sizes{0, 1, 15, 16, 17};
  for (size_t n : {1, 5, 9, 37, 1001}) {
    sizes.push_back(8 * n);
    sizes.push_back(4 * (n + 1));
    sizes.push_back(n);
  }
  for (size_t a : sizes)
    for (size_t b : sizes)
      for (size_t c : sizes) {
        std::vector<Region> r{{kIn, a, 0, 0},      {kIn, b, 0, 0},      {kInPadded, c, 0, 0},
                              {kIn, a, c % 7, 0},  {kScratch, b, 0, 0}, {kScratch, c, 0, 0},
                              {kOut, a, 0, 0},     {kOut, c, 0, 0},     {kOut, b, 0, 0}};
        fill_and_read(r);
        std::vector<Region> first{{kInPadded, a, 0, 0}, {kOut, b, 0, 0}};  // padding at the very front, no scratch
        fill_and_read(first);
      }
  std::vector<Region> none;
  const tmh::StageLayout empty = build(none);
  expect(empty.dev_bytes == 0 && empty.pad_at == 0, "empty layout", empty.dev_bytes, 0);
  // the largest calls the entry points accept (2^26 entries, 2^30 bytes of data, 2^28 aunts), value ops' shape:
  // arithmetic only, nothing allocated
  const size_t n = (size_t)1 << 26, bytes = (size_t)1 << 30, aunts = (size_t)1 << 28;
  std::vector<Region> big{{kIn, 8 * n, 0, 0},       {kIn, 8 * n, 0, 0},       {kIn, 32 * n, 0, 0},
                          {kIn, 32 * n, 0, 0},      {kIn, 32 * aunts, 0, 0},  {kIn, 4 * (n + 1), 0, 0},
                          {kIn, 4 * (n + 1), 0, 0}, {kIn, 4 * (n + 1), 0, 0}, {kIn, 4 * (n + 1), 0, 0},
                          {kIn, bytes, 0, 0},       {kInPadded, bytes, 0, 0}, {kScratch, 32 * n, 0, 0},
                          {kScratch, 32 * (n + 32 * n), 0, 0},                {kOut, 32 * n, 0, 0},
                          {kOut, 32 * n, 0, 0},     {kOut, 32 * aunts, 0, 0}, {kOut, n, 0, 0},
                          {kOut, 4 * n, 0, 0}};
  const tmh::StageLayout L = build(big);
  unsigned __int128 sum = 16;
  for (const Region &x : big) sum += (unsigned __int128)((x.bytes + 15) / 16) * 16;
  expect(sum == (unsigned __int128)L.dev_bytes, "total at the limits", L.dev_bytes, (uint64_t)sum);
  expect(L.dev_bytes > 32 * aunts && L.in_bytes > 32 * aunts + 2 * bytes, "totals did not wrap", L.dev_bytes,
         L.in_bytes);
  offsets();
  std::printf("%d wrong\n", g_wrong);
  return g_wrong ? 1 : 0;
}
