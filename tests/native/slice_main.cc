// Stand-alone exercise of the sliced GET's host code: resolve_window against a byte-by-byte
// model; slice_find_head_end and slice_layout on exact-size heap copies of well-formed values
// and of every prefix of them; HostCache::get_keyed_slices on the granule and wave-pass seam
// cases, writing into row and response buffers of exactly the needed size; the Range header
// parser on exact-size strings; and how hbm_flight_plan.h plans slices. Built with
// -fsanitize=address,undefined by tests/test_slices.py, so a read past a value or a write past
// a buffer is reported.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "hbm_flight_plan.h"
#include "host_cache.h"
#include "keyed.h"
#include "slice.h"

using namespace shellac;

#define CHECK(c)                                                        \
  do {                                                                  \
    if (!(c)) {                                                         \
      std::fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #c); \
      std::exit(1);                                                     \
    }                                                                   \
  } while (0)

static std::string keyed_value(const std::string& key, const std::string& payload) {
  std::string v(keyed_size(key.size(), payload.size()), '\0');
  write_keyed(reinterpret_cast<uint8_t*>(&v[0]), key, payload.data(), payload.size());
  return v;
}

// An HTTP head of exactly n bytes whose only CR LF CR LF are its last four.
static std::string head_of(size_t n) {
  const std::string base = "HTTP/1.1 200 OK\r\nX-P: ";
  CHECK(n >= base.size() + 4);
  return base + std::string(n - base.size() - 4, 'a') + "\r\n\r\n";
}

static std::string body_of(size_t n, unsigned seed) {
  std::string b(n, '\0');
  unsigned x = seed * 2654435761u + 12345u;
  for (size_t i = 0; i < n; ++i) {
    x = x * 1664525u + 1013904223u;
    b[i] = (char)(x >> 24);
  }
  return b;
}

// ---- resolve_window
static void windows() {
  const uint32_t kinds[] = {kSliceHead, kSliceRange, kSliceFrom, kSliceSuffix};
  for (uint64_t len = 0; len <= 20; ++len)
    for (uint32_t kind : kinds)
      for (uint64_t a = 0; a <= 22; ++a)
        for (uint64_t b = 0; b <= 22; ++b) {
          // the bytes the spec names, one by one
          std::vector<bool> want(len, false);
          bool sat = true;
          if (kind == kSliceRange) {
            sat = a <= b && a < len;
            for (uint64_t i = a; sat && i <= b && i < len; ++i) want[i] = true;
          } else if (kind == kSliceFrom) {
            sat = a < len;
            for (uint64_t i = a; i < len; ++i) want[i] = true;
          } else if (kind == kSliceSuffix) {
            sat = a > 0 && len > 0;
            for (uint64_t i = 0; sat && i < len; ++i) want[i] = i + a >= len;
          }
          uint64_t first = 99, n = 99;
          CHECK(resolve_window(kind, a, b, len, &first, &n) == sat);
          if (!sat || kind == kSliceHead) {
            CHECK(first == 0 && n == 0);
            continue;
          }
          CHECK(n >= 1 && first + n <= len);
          for (uint64_t i = 0; i < len; ++i) CHECK(want[i] == (i >= first && i < first + n));
        }
  uint64_t first, n;
  CHECK(resolve_window(kSliceRange, 0, ~0ull, 10, &first, &n) && first == 0 && n == 10);
  CHECK(resolve_window(kSliceSuffix, ~0ull, 0, 10, &first, &n) && first == 0 && n == 10);
  CHECK(!resolve_window(kSliceFrom, ~0ull, 0, 10, &first, &n));
  CHECK(!resolve_window(kSliceRange, ~0ull, ~0ull, 10, &first, &n));
  CHECK(!resolve_window(kSliceWhole, 0, 0, 10, &first, &n));
}

// ---- where a head ends, on heap copies with no slack behind them
static bool layout_exact(const std::string& v, uint32_t* ho, uint32_t* bo) {
  std::unique_ptr<uint8_t[]> buf(new uint8_t[v.size() ? v.size() : 1]);
  std::memcpy(buf.get(), v.data(), v.size());
  return slice_layout(buf.get(), v.size(), ho, bo);
}

static void layouts() {
  uint32_t ho, bo;
  const std::string pay = head_of(45) + body_of(30, 1);
  const std::string plain = keyed_value("/k", pay);
  CHECK(layout_exact(plain, &ho, &bo) && ho == 4 && bo == 49);
  uint64_t hashes[32];
  for (int i = 0; i < 32; ++i) hashes[i] = 0x0a0d0a0d0a0d0a0dull;  // CR LF CR LF in every hash
  for (size_t nt : {1u, 32u, 33u}) {
    std::string block(tag_block_size(nt), '\0');
    write_tag_block(reinterpret_cast<uint8_t*>(&block[0]), hashes, nt);
    const std::string v = keyed_value("/a\r\n\r\nb", block + pay);
    CHECK(layout_exact(v, &ho, &bo) && ho == 2 + 7 + block.size() && bo == ho + 45);
    // every prefix of the value: never a read past it, and sliceable exactly from the
    // terminator's last byte on
    for (size_t cut = 0; cut <= v.size(); ++cut) {
      uint32_t h2, b2;
      const bool ok = layout_exact(v.substr(0, cut), &h2, &b2);
      CHECK(ok == (cut >= bo));
      if (ok) CHECK(h2 == ho && b2 == bo);
    }
  }
  CHECK(!layout_exact(keyed_value("/k", "HTTP/1.1 200 OK\n\nbody"), &ho, &bo));
  CHECK(!layout_exact(keyed_value("/k", "http/1.1 200 OK\r\n\r\n"), &ho, &bo));
  CHECK(!layout_exact(keyed_value("/k", "\x01" "accept-encoding"), &ho, &bo));
  CHECK(!layout_exact(keyed_value("/k", std::string("\x02\x28", 2) + pay), &ho, &bo));  // 40 tags
  CHECK(!layout_exact(std::string("\xff\xff", 2), &ho, &bo) && !layout_exact("", &ho, &bo));
  CHECK(layout_exact(keyed_value("/k", head_of(kSliceHeadMax)), &ho, &bo) && bo == 4 + kSliceHeadMax);
  CHECK(!layout_exact(keyed_value("/k", head_of(kSliceHeadMax + 1)), &ho, &bo));
}

// ---- the twin, into buffers of exactly the needed size
struct Batch {
  std::vector<std::string> keys;
  std::vector<SliceSpec> specs;
};

static void run_batch(HostCache& hc, const Batch& q, const std::vector<std::string>& values,
                      uint32_t now) {
  const int64_t n = (int64_t)q.keys.size();
  std::vector<Digest> d((size_t)n);
  std::string kb;
  std::vector<int64_t> offs((size_t)n + 1, 0);
  for (int64_t i = 0; i < n; ++i) {
    d[(size_t)i] = digest_bytes(reinterpret_cast<const uint8_t*>(q.keys[(size_t)i].data()),
                                q.keys[(size_t)i].size());
    kb += q.keys[(size_t)i];
    offs[(size_t)i + 1] = (int64_t)kb.size();
  }
  std::unique_ptr<uint8_t[]> kbuf(new uint8_t[kb.size() ? kb.size() : 1]);
  std::memcpy(kbuf.get(), kb.data(), kb.size());
  std::unique_ptr<SliceRow[]> rows(new SliceRow[(size_t)n]);
  uint64_t res[kSliceWords] = {0, 0};
  // too small a buffer (none at all): rows and totals only
  hc.get_keyed_slices(d.data(), kbuf.get(), offs.data(), q.specs.data(), n, rows.get(), nullptr, 0,
                      res, now);
  const uint64_t total = res[kSliceBytes];
  std::unique_ptr<uint8_t[]> out(new uint8_t[total ? total : 1]);
  hc.get_keyed_slices(d.data(), kbuf.get(), offs.data(), q.specs.data(), n, rows.get(), out.get(),
                      total, res, now);
  CHECK(res[kSliceBytes] == total);
  uint64_t at = 0, hits = 0;
  for (int64_t i = 0; i < n; ++i) {
    const SliceRow& r = rows[(size_t)i];
    const std::string& v = values[(size_t)i];
    CHECK(r.out_off == at);
    at += slice_row_bytes(r);
    if (v.empty()) {
      CHECK(r.status == kSliceMiss);
      continue;
    }
    ++hits;
    SliceRow want;
    slice_value_row(&want, q.specs[(size_t)i], reinterpret_cast<const uint8_t*>(v.data()),
                    (uint32_t)v.size(), 5, 0);
    want.out_off = r.out_off;
    CHECK(std::memcmp(&want, &r, sizeof(r)) == 0);
    const uint8_t* const o = out.get() + r.out_off;
    if (r.status == kSliceWholeObj) {
      CHECK(std::memcmp(o, v.data(), v.size()) == 0);
      continue;
    }
    CHECK(std::memcmp(o, v.data(), r.body_off) == 0);
    CHECK(std::memcmp(o + r.head_bytes + r.skew, v.data() + r.body_off + r.win_first, r.win_len) == 0);
  }
  CHECK(at == total && hits == res[kSliceHits]);
}

static void twin() {
  HostCache hc(1u << 20, 256, 8192);
  Batch q;
  std::vector<std::string> values;
  std::vector<std::string> keys, vals;
  // terminators at value offsets 13..16 mod 16 and 1021..1024, 2045..2048 past the granule the
  // search starts in, for head_off of several alignments
  for (size_t klen : {1u, 6u, 13u, 14u, 30u}) {
    const size_t head_off = 2 + klen, start = head_off & ~(size_t)15;
    for (size_t at : {77u, 78u, 79u, 80u, 1021u, 1022u, 1023u, 1024u, 2045u, 2046u, 2047u, 2048u}) {
      std::string key = std::string(1, (char)('A' + keys.size() % 12)) + "/seam/key/padded/to/its/length";
      key.resize(klen);
      keys.push_back(key);
      vals.push_back(keyed_value(key, head_of(start + at - head_off + 4) + body_of(37, (unsigned)at)));
      uint32_t ho, bo;
      CHECK(layout_exact(vals.back(), &ho, &bo) && ho == head_off && bo == start + at + 4);
    }
  }
  keys.push_back("/end");  // a terminator at the very end: an empty body
  vals.push_back(keyed_value("/end", head_of(48)));
  keys.push_back("/vary");
  vals.push_back(keyed_value("/vary", "\x01" "accept-encoding"));
  const uint32_t now = 10;
  for (size_t i = 0; i < keys.size(); ++i) {
    const Digest d = digest_bytes(reinterpret_cast<const uint8_t*>(keys[i].data()), keys[i].size());
    hc.set_one(d, reinterpret_cast<const uint8_t*>(vals[i].data()), (uint32_t)vals[i].size(), 5, 0,
               now);
  }
  const SliceSpec specs[] = {{kSliceHead, 0, 0, 0},   {kSliceRange, 0, 0, 0},  {kSliceRange, 0, 3, 18},
                             {kSliceSuffix, 0, 5, 0}, {kSliceFrom, 0, 36, 0},  {kSliceFrom, 0, 37, 0},
                             {kSliceWhole, 0, 0, 0},  {kSliceSuffix, 0, 0, 0}, {kSliceRange, 0, 9, 2}};
  for (const SliceSpec& sp : specs) {
    Batch b;
    std::vector<std::string> want;
    for (size_t i = 0; i < keys.size(); ++i) {
      b.keys.push_back(keys[i]);
      b.specs.push_back(sp);
      want.push_back(vals[i]);
      if (i % 7 == 0) {  // a miss between the hits
        b.keys.push_back(keys[i] + "?missing");
        b.specs.push_back(sp);
        want.push_back("");
      }
    }
    run_batch(hc, b, want, now);
  }
  run_batch(hc, Batch{}, {}, now);  // an empty batch
  const CacheCounters c = hc.counters();
  CHECK(c.get_ops > c.get_hits && c.get_hits > 0 && c.get_bytes > 0);
}

// ---- the Range header
static bool range(const std::string& s, SliceSpec* sp) {
  const std::string e(s.data(), s.size());  // a heap copy with no slack behind it
  return parse_single_range(e.data(), e.size(), sp);
}

static void range_headers() {
  SliceSpec sp;
  CHECK(range("bytes=0-0", &sp) && sp.kind == kSliceRange && sp.a == 0 && sp.b == 0);
  CHECK(range("bytes=5-", &sp) && sp.kind == kSliceFrom && sp.a == 5);
  CHECK(range("bytes=-7", &sp) && sp.kind == kSliceSuffix && sp.a == 7);
  CHECK(range("bytes=0-99999", &sp) && sp.kind == kSliceRange && sp.a == 0 && sp.b == 99999);
  CHECK(range("  BYTES= 10-20\t", &sp) && sp.kind == kSliceRange && sp.a == 10 && sp.b == 20);
  CHECK(range("bytes=-0", &sp) && sp.kind == kSliceSuffix && sp.a == 0);  // (unsatisfiable: 416)
  CHECK(range("bytes=18446744073709551615-", &sp) && sp.a == ~0ull);
  CHECK(range("bytes=99999999999999999999999-", &sp) && sp.kind == kSliceFrom && sp.a == ~0ull);
  CHECK(range("bytes=1-99999999999999999999999", &sp) && sp.b == ~0ull);
  for (const char* bad : {"", "bytes", "bytes=", "bytes=-", "bytes=5", "bytes=a-b", "bytes=5-2",
                          "bytes=0-1,3-4", "bytes=0-1,", "bytes=,0-1", "bytes=0-1 2", "bytes=0--1",
                          "bytes=0 -1", "items=0-1", "byte=0-1", "bytes =0-1", "bytes=0x1-2",
                          "bytes=+1-2", "bytes=1-2-", "bytes=-1-", "bytess=1-2"})
    CHECK(!range(bad, &sp));
}

// ---- slices in a flight: planned as GETs, one row per request
static void flights() {
  std::vector<HbmReq> q(5);
  q[0].kind = ReqKind::Slice;
  q[0].d = Digest{1, 1};
  q[0].key = "ab";
  q[1].kind = ReqKind::Set;
  q[1].d = Digest{1, 1};
  q[2].kind = ReqKind::Slice;  // another key's: stays in the flight
  q[2].d = Digest{2, 2};
  q[2].key = "";
  q[3].kind = ReqKind::Slice;  // behind a write of its key: the next flight
  q[3].d = Digest{1, 1};
  q[3].key = "cde";
  q[4].kind = ReqKind::Get;
  q[4].d = Digest{3, 3};
  CHECK(plan_take(q, 100) == 3);
  CHECK(plan_take(q, 2) == 2);
  q[1].kind = ReqKind::Barrier;
  CHECK(plan_take(q, 100) == 5);
  const SlicePlan p = plan_slice_rows(q, {0, 2, 3});
  CHECK(p.kbytes == "abcde");
  CHECK((p.offs == std::vector<int64_t>{0, 2, 2, 5}));
  CHECK(plan_slice_rows(q, {}).offs == std::vector<int64_t>{0});
  CHECK(!is_write(ReqKind::Slice) && !is_ctl(ReqKind::Slice));
}

int main() {
  flights();
  windows();
  layouts();
  twin();
  range_headers();
  std::printf("slice_main: ok\n");
  return 0;
}
