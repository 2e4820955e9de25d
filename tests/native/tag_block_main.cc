// Stand-alone exercise of the tag block helpers (keyed.h) and HostCache's tag scan over
// well-formed, hostile and truncated blocks. Built with -fsanitize=address,undefined by
// tests/test_tag_purge.py: every value is copied into an exact-size heap buffer before it is
// parsed, so a read past the value, and a dereference of an unaligned hash, is reported.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "host_cache.h"
#include "keyed.h"

using namespace shellac;

#define CHECK(c)                                                        \
  do {                                                                  \
    if (!(c)) {                                                         \
      std::fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #c); \
      std::exit(1);                                                     \
    }                                                                   \
  } while (0)

static std::string le64(uint64_t h) {
  std::string s(8, '\0');
  for (int b = 0; b < 8; ++b, h >>= 8) s[b] = (char)h;
  return s;
}

static std::string block_of(const std::vector<uint64_t>& hs) {
  std::string b(tag_block_size(hs.size()), '\0');
  CHECK(write_tag_block(reinterpret_cast<uint8_t*>(&b[0]), hs.data(), hs.size()) == b.size());
  return b;
}

// parse / match on an exact-size heap copy at every byte alignment of the start
static bool matches(const std::string& payload, const std::vector<uint64_t>& list,
                    size_t* strip_out = nullptr, bool* over_out = nullptr) {
  bool first = true, res = false;
  for (size_t shift = 0; shift < 8; ++shift) {
    std::unique_ptr<char[]> buf(new char[shift + payload.size()]);
    if (!payload.empty()) std::memcpy(buf.get() + shift, payload.data(), payload.size());
    const uint64_t* hs;
    unsigned nt;
    bool over;
    const size_t strip = parse_tag_block(buf.get() + shift, payload.size(), &hs, &nt, &over);
    CHECK(strip <= payload.size());
    CHECK(strip == 0 || strip == (over ? 2 : 2 + 8 * (size_t)nt));
    uint64_t sum = 0;
    for (unsigned i = 0; i < nt; ++i) sum += tag_block_hash(hs, i);
    (void)sum;
    const bool m = tag_block_matches(buf.get() + shift, payload.size(), list.data(), list.size());
    if (first) {
      res = m;
      if (strip_out) *strip_out = strip;
      if (over_out) *over_out = over;
      first = false;
    }
    CHECK(m == res);
  }
  return res;
}

int main() {
  const uint64_t t = tag_hash("product-4711"), u = tag_hash("other");
  CHECK(t == digest_bytes(reinterpret_cast<const uint8_t*>("product-4711"), 12).lo);
  CHECK(t != u && tag_hash("Product-4711") != t);
  const std::string http = "HTTP/1.1 200 OK\r\n\r\nok";
  size_t strip;
  bool over;

  // ---- the helpers
  CHECK(tag_block_size(0) == 2 && tag_block_size(32) == 2 + 256 && tag_block_size(33) == 2);
  CHECK(block_of({t, u}) == std::string("\x02\x02", 2) + le64(t) + le64(u));
  CHECK(block_of(std::vector<uint64_t>(40, t)) == std::string("\x02\xff", 2));
  CHECK(matches(block_of({u, t}) + http, {t}, &strip, &over) && strip == 18 && !over);
  CHECK(!matches(block_of({u}) + http, {t}));
  CHECK(matches(block_of({u}) + http, {t, t, u}));
  CHECK(!matches(block_of({}) + http, {t}, &strip) && strip == 2);              // ntags = 0
  CHECK(matches("\x02\xff" + http, {t}, &strip, &over) && strip == 2 && over);  // overflow
  CHECK(matches("\x02\xff", {u}));
  for (int nt : {33, 34, 128, 254}) {                                            // malformed
    std::string p = std::string("\x02", 1) + (char)nt;
    for (int i = 0; i < nt; ++i) p += le64(t);
    CHECK(!matches(p + http, {t}, &strip) && strip == 0);
  }
  for (int nt : {1, 2, 4, 32}) {                                                 // truncated
    std::string full = std::string("\x02", 1) + (char)nt;
    for (int i = 0; i < nt; ++i) full += le64(t);
    CHECK(matches(full, {t}));
    for (size_t cut = 0; cut < full.size(); ++cut) {
      CHECK(!matches(full.substr(0, cut), {t}, &strip));
      CHECK(strip == 0);
    }
  }
  CHECK(!matches("", {t}) && !matches("\x02", {t}) && !matches(http, {t}));
  CHECK(!matches("\x01" "accept-encoding", {t}));
  CHECK(!matches(std::string("\x02\x01", 2) + le64(t).substr(0, 7), {t}));
  // one bit off, in each byte of the hash
  for (int bit = 0; bit < 64; ++bit) CHECK(!matches(block_of({t ^ (1ull << bit)}) + http, {t}));

  // ---- whole keyed values, on exact-size copies
  for (size_t klen = 0; klen <= 40; ++klen) {
    const std::string key(klen, 'k');
    for (const std::string& payload :
         {block_of({u, t}) + http, block_of({u}) + http, std::string("\x02\xff", 2),
          std::string("\x02", 1), std::string(), http, std::string("\x02\x04", 2) + le64(t)}) {
      std::string v(keyed_size(klen, payload.size()), '\0');
      write_keyed(reinterpret_cast<uint8_t*>(&v[0]), key, payload.data(), payload.size());
      std::unique_ptr<uint8_t[]> buf(new uint8_t[v.size() ? v.size() : 1]);
      std::memcpy(buf.get(), v.data(), v.size());
      const bool want = tag_block_matches(payload.data(), payload.size(), &t, 1);
      CHECK(keyed_tags_match(buf.get(), v.size(), &t, 1) == want);
      for (size_t cut = 0; cut < 2 + klen && cut < v.size(); ++cut) {  // ends inside the key
        std::unique_ptr<uint8_t[]> c(new uint8_t[cut ? cut : 1]);
        std::memcpy(c.get(), v.data(), cut);
        CHECK(!keyed_tags_match(c.get(), cut, &t, 1));
      }
    }
  }

  // ---- HostCache's scan over the same forms
  HostCache hc(1 << 20, 1 << 10, 4096);
  const uint32_t now = 10;
  struct Obj {
    std::string key, payload;
    bool goes;
  };
  std::vector<Obj> objs;
  int id = 0;
  for (size_t klen : {1, 5, 12, 13, 14, 29, 30, 31, 40}) {
    const std::vector<std::pair<std::string, bool>> forms = {
        {block_of({u, t}) + http, true},
        {block_of({t}), true},
        {block_of({u}) + http, false},
        {block_of({}) + http, false},
        {"\x02\xff" + http, true},
        {std::string("\x02\x21", 2) + std::string(33 * 8, 'x') + http, false},
        {std::string("\x02\xfe", 2) + std::string(254 * 8, 'x') + http, false},
        {std::string("\x02\x04", 2) + le64(t) + "12345", false},
        {"", false},
        {"\x02", false},
        {std::string("\x02\x01", 2) + le64(t).substr(0, 7), false},
        {http, false},
        {"\x01" "accept-encoding", false}};
    for (const auto& f : forms) {
      std::string key(klen, 'a');
      key[0] = (char)(33 + id++ % 200);
      if (klen > 1) key[klen - 1] = (char)(33 + id / 200);
      objs.push_back({key, f.first, f.second});
    }
  }
  // non-keyed junk (purge_cases.garbage_values)
  const std::vector<std::string> junk = {"", "/", std::string("\x88\x13", 2) + "/abc/abc/abc",
                                         std::string("\x0b\x00", 2) + "/abcdefghi",
                                         std::string(40, '\xff'), std::string("\x00\x00", 2)};
  size_t want_gone = 0;
  for (const Obj& o : objs) {
    std::string v(keyed_size(o.key.size(), o.payload.size()), '\0');
    write_keyed(reinterpret_cast<uint8_t*>(&v[0]), o.key, o.payload.data(), o.payload.size());
    const Digest d = digest_bytes(reinterpret_cast<const uint8_t*>(o.key.data()), o.key.size());
    hc.set_one(d, reinterpret_cast<const uint8_t*>(v.data()), (uint32_t)v.size(), 1, 0, now);
    want_gone += o.goes;
  }
  for (size_t i = 0; i < junk.size(); ++i) {
    const std::string name = "junk/" + std::to_string(i);
    const Digest d = digest_bytes(reinterpret_cast<const uint8_t*>(name.data()), name.size());
    hc.set_one(d, reinterpret_cast<const uint8_t*>(junk[i].data()), (uint32_t)junk[i].size(), 1,
               0, now);
  }
  const uint64_t list[3] = {tag_hash("nobody"), t, t};
  CHECK(hc.soften_keyed_tags(list, 3, 77, now + 50, now) == want_gone);
  CHECK(hc.soften_keyed_tags(list, 3, 78, 0, now) == want_gone);
  uint64_t out[2] = {0, 0};
  hc.remove_keyed_tags(list, 3, now, out);
  CHECK(out[0] == want_gone && hc.counters().purged == want_gone);
  size_t live = 0;
  for (const Obj& o : objs) {
    const Digest d = digest_bytes(reinterpret_cast<const uint8_t*>(o.key.data()), o.key.size());
    std::string got;
    uint32_t flags = 0;
    const bool hit = hc.get_one(d, &got, &flags, now);
    CHECK(hit == !o.goes);
    if (hit) {
      CHECK(flags == 1 && got.size() == keyed_size(o.key.size(), o.payload.size()));
      ++live;
    }
  }
  CHECK(live == objs.size() - want_gone);
  hc.remove_keyed_tags(list, 3, now, out);
  CHECK(out[0] == 0 && out[1] == 0);
  bool threw = false;
  try {
    hc.remove_keyed_tags(list, 0, now, out);
  } catch (const std::exception&) {
    threw = true;
  }
  CHECK(threw);
  std::printf("tag_block_main: ok (%zu objects, %zu purged)\n", objs.size(), want_gone);
  return 0;
}
