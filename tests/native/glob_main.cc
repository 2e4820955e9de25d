// Stand-alone exercise of the glob purge's host code: compile_keyed_glob (keyed.h) on every
// refused form and at the limits; keyed_glob_matches on the overlap table, on the subject rule
// (the key ends at its first 0x1f) and on keys of 0, 1 and 65535 bytes, all on exact-size heap
// copies; keyed_value_glob_matches on values whose klen points past their end; the glob
// selector of inspect.h and selector.h (query parsing, list_query_valid, matches_value); and
// HostCache::remove_keyed_glob, soften_keyed_glob and list_keyed(kListGlob) on a small shard.
// Built with -fsanitize=address,undefined by tests/test_glob_purge.py, so a read past a key
// or a value, or a write past a buffer, is reported.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "host_cache.h"
#include "inspect.h"
#include "keyed.h"

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

static bool compiles(const std::string& pat, KeyedGlob* g = nullptr, std::string* why = nullptr) {
  // the pattern on the heap with no slack behind it
  std::unique_ptr<uint8_t[]> buf(new uint8_t[pat.size() ? pat.size() : 1]);
  std::memcpy(buf.get(), pat.data(), pat.size());
  KeyedGlob local;
  return compile_keyed_glob(buf.get(), pat.size(), g ? g : &local, why);
}

// The matcher on an exact-size heap copy of the key.
static bool match(const std::string& pat, const std::string& key) {
  auto g = std::make_unique<KeyedGlob>();
  CHECK(compiles(pat, g.get()));
  std::unique_ptr<uint8_t[]> buf(new uint8_t[key.size() ? key.size() : 1]);
  std::memcpy(buf.get(), key.data(), key.size());
  return keyed_glob_matches(*g, buf.get(), key.size());
}

static bool value_match(const std::string& pat, const std::string& v) {
  auto g = std::make_unique<KeyedGlob>();
  CHECK(compiles(pat, g.get()));
  std::unique_ptr<uint8_t[]> buf(new uint8_t[v.size() ? v.size() : 1]);
  std::memcpy(buf.get(), v.data(), v.size());
  return keyed_value_glob_matches(*g, buf.get(), v.size());
}

static std::string stars(size_t n, const std::string& between) {
  std::string s;
  for (size_t i = 0; i < n; ++i) s += between + "*";
  return s;
}

static void compiler() {
  std::string why;
  for (const std::string& bad :
       {std::string(), std::string("*"), std::string("***"), std::string("\\"),
        std::string("/a/*\\"), std::string("a\\\\\\"), stars(kMaxGlobStars + 1, "a"),
        std::string(kMaxGlobStars + 1, '*') + "a", std::string(kMaxGlobLiteral + 1, 'a'),
        std::string(1000, 'a') + "*" + std::string(25, 'b'),
        std::string("\\*") + std::string(kMaxGlobLiteral, 'a')}) {
    why.clear();
    CHECK(!compiles(bad, nullptr, &why) && !why.empty());
    CHECK(!compiles(bad));  // (no error string wanted)
  }
  KeyedGlob g;
  CHECK(compiles(stars(kMaxGlobStars, "a"), &g) && g.stars == kMaxGlobStars && g.nmid == 7);
  CHECK(g.head_len == 1 && g.tail_len == 0 && g.min_len == 8 && g.lit_bytes == 8);
  CHECK(compiles(std::string(kMaxGlobLiteral, 'a'), &g) && g.stars == 0 && g.nmid == 0);
  CHECK(g.head_len == kMaxGlobLiteral && keyed_glob_used_bytes(g) == keyed_glob_image_bytes());
  CHECK(compiles(std::string(512, 'a') + "*" + std::string(512, 'b'), &g));
  CHECK(g.head_len == 512 && g.tail_len == 512 && g.tail_off == 512);
  CHECK(compiles("a**b", &g) && g.stars == 2 && g.nmid == 0 && g.min_len == 2);
  CHECK(compiles("*a", &g) && g.head_len == 0 && g.tail_len == 1 && g.m0[5] == 0);
  CHECK(compiles("\\*\\\\", &g) && g.stars == 0 && g.lit_bytes == 2 && g.lit[0] == '*');
  CHECK(compiles("/img/*/thumb_*.jpg", &g) && g.nmid == 1 && g.head_len == 5 && g.tail_len == 4);
  CHECK(keyed_glob_used_bytes(g) == kGlobHeaderBytes + 16 && g.m0[0] == 0 && g.m0[2] == 0xff);
  CHECK(g.m0[6] == 0xff && g.m0[7] == 0 && g.p0[2] == '/' && g.p0[6] == '/');
  CHECK(keyed_glob_escape("a\\b*c", true) == "a\\\\b*c");
  CHECK(keyed_glob_escape("a\\b*c", false) == "a\\\\b\\*c");
}

static void matcher() {
  struct Row {
    const char* pat;
    const char* key;
    bool yes;
  };
  for (const Row& r : {Row{"ab*ba", "aba", false}, Row{"ab*ba", "abba", true},
                       Row{"*ab*ab*", "abab", true}, Row{"*ab*ab*", "aab", false},
                       Row{"*a", "bbbba", true}, Row{"a*", "a", true}, Row{"a**b", "ab", true},
                       Row{"a\\*b", "a*b", true}, Row{"a\\*b", "axb", false},
                       Row{"a\\\\b", "a\\b", true}, Row{"abc", "abc", true}, Row{"abc", "abcd", false},
                       Row{"abc", "ab", false}, Row{"*b*", "abc", true}, Row{"*b*", "ac", false}})
    CHECK(match(r.pat, r.key) == r.yes);
  // the subject ends at the first separator; a key that is empty, or starts with one, has none
  const std::string k = std::string("/a.css\x1f") + "gzip";
  CHECK(match("*.css", k) && match("/a.css", k) && match("/a*", k));
  CHECK(!match("*gzip", k) && !match("*.css*gzip", k) && !match(std::string("*\x1f*"), k));
  CHECK(match("*.css", std::string("/a.css\x1f") + "x\x1f.css"));
  CHECK(!match("a*", "") && !match("*a", "") && !match("a*", std::string("\x1f") + "a"));
  // keys of 0, 1 and 65535 bytes
  CHECK(match("a", "a") && match("*a", "a") && match("a*", "a") && !match("b", "a"));
  std::string big(kMaxKeyedKey, 'x');
  big[0] = '/';
  big[kMaxKeyedKey - 1] = 'z';
  big.replace(40000, 5, "HELLO");
  CHECK(match("/*HELLO*z", big) && match("*z", big) && match("/*", big) && match("*LLO*", big));
  CHECK(!match("/*HELLOx*HELLO*z", big) && !match("*y", big) && !match("z*", big));
  CHECK(match("*" + std::string(1023, 'x') + "z", big));
  big[30000] = '\x1f';
  CHECK(!match("*z", big) && !match("*HELLO*", big) && match("/*x", big));
  // a whole value: klen bounds the match, and a klen past the end matches nothing
  CHECK(value_match("/k/*", keyed_value("/k/1", "payload")));
  CHECK(!value_match("/k/*load", keyed_value("/k/1", "payload")));
  CHECK(!value_match("/k/1pay*", keyed_value("/k/1", "payload")));
  CHECK(value_match("/k/1", keyed_value("/k/1", "\x1f/k/1")));
  for (const std::string& v : {std::string(), std::string("/"), std::string("\x05\x00", 2) + "/k/1",
                               std::string("\x88\x13", 2) + "/k/1/k/1", std::string("\xff\xff", 2),
                               std::string("\x00\x00", 2), std::string("\x00\x00", 2) + "/k/1"})
    CHECK(!value_match("/k/*", v) && !value_match("*1", v) && !value_match("*k*", v));
  const std::string full = keyed_value("/k/1", "p");
  for (size_t cut = 0; cut < 6; ++cut) CHECK(!value_match("/k/*", full.substr(0, cut)));
  CHECK(value_match("/k/*", full.substr(0, 6)));
}

static void inspect_helpers() {
  InspectParams p;
  CHECK(parse_inspect_query("glob=%2A%2Fstatic%2F%2A.css&limit=3", &p));
  CHECK(p.which == 4 && p.value == "*/static/*.css" && p.limit == 3);
  CHECK(parse_inspect_query("glob=a%5C%2Ab", &p) && p.value == "a\\*b");
  CHECK(!parse_inspect_query("glob=a*&prefix=a", &p) && !parse_inspect_query("glob=a&glob=b", &p));
  CHECK(!parse_inspect_query("tag=a&glob=b", &p) && !parse_inspect_query("glob=%", &p));
  ListQuery q;
  q.what = KeyedSelector::glob("");
  CHECK(!list_query_valid(q));
  for (const std::string& bad : {std::string("*"), std::string("a\\"), stars(9, "a"),
                                 std::string(1025, 'a')}) {
    std::string why;
    q.what = KeyedSelector::glob(bad, &why);
    CHECK(!list_query_valid(q) && !why.empty() && !q.what.compiled);
  }
  q.what = KeyedSelector::glob("*/static/*");
  CHECK(list_query_valid(q) && q.what.list_mode() == kListGlob);
  q.limit = kMaxListRows + 1;
  CHECK(!list_query_valid(q));
  q.limit = 5;
  const std::string v = keyed_value("h/static/x", "p");
  const uint8_t* const b = reinterpret_cast<const uint8_t*>(v.data());
  CHECK(q.what.matches_value(b, v.size()) && !KeyedSelector::glob("*").matches_value(b, v.size()));
  CHECK(!q.what.matches_value(b, 5));
}

struct Listing {
  uint64_t out[kListWords];
  std::vector<std::string> keys;
};

// One glob listing into buffers of exactly `limit` rows (none for limit 0).
static Listing list(HostCache& hc, const std::string& pat, uint64_t start, uint32_t limit,
                    uint32_t now) {
  const uint32_t key_cap = 64;
  Listing l;
  std::unique_ptr<ListRow[]> rows(limit ? new ListRow[limit] : nullptr);
  std::unique_ptr<uint8_t[]> keys(limit ? new uint8_t[(size_t)limit * key_cap] : nullptr);
  hc.list_keyed(kListGlob, reinterpret_cast<const uint8_t*>(pat.data()), (uint32_t)pat.size(),
                false, nullptr, 0, start, limit, key_cap, now, rows.get(), keys.get(), l.out);
  CHECK(l.out[kListListed] <= limit && l.out[kListListed] <= l.out[kListMatched]);
  for (uint64_t i = 0; i < l.out[kListListed]; ++i) {
    CHECK(i == 0 || rows[i - 1].slot < rows[i].slot);
    CHECK(rows[i].klen <= key_cap - 2 && !(rows[i].bits & kListChanged));
    l.keys.emplace_back(reinterpret_cast<const char*>(keys.get() + i * key_cap) + 2, rows[i].klen);
  }
  return l;
}

static void host_cache() {
  HostCache hc(1 << 20, 1 << 10, 4096);
  const uint32_t now = 10;
  std::map<std::string, std::string> stored;
  for (int i = 0; i < 40; ++i) {
    for (const char* fmt : {"/static/css/%d.css", "/static/js/%d.js", "/api/v1/users/%d",
                            "/img/%d/thumb_a.jpg"}) {
      char buf[64];
      std::snprintf(buf, sizeof(buf), fmt, i);
      stored[buf] = keyed_value(buf, std::string((size_t)i, 'p'));
    }
  }
  const std::string var = "/static/css/1.css";
  stored[var + "\x1f" + "gzip"] = keyed_value(var + "\x1f" + "gzip", "HTTP/ gz");
  for (const auto& kv : stored) {
    const Digest d = digest_bytes(reinterpret_cast<const uint8_t*>(kv.first.data()), kv.first.size());
    hc.set_one(d, reinterpret_cast<const uint8_t*>(kv.second.data()), (uint32_t)kv.second.size(), 7,
               now + 100, now);
  }
  // non-keyed junk (purge_cases.garbage_values): never matched
  const std::vector<std::string> junk = {"", "/", std::string("\x88\x13", 2) + "/abc/abc/abc",
                                         std::string("\x0b\x00", 2) + "/abcdefghi",
                                         std::string(40, '\xff'), std::string("\x00\x00", 2)};
  for (size_t i = 0; i < junk.size(); ++i) {
    const std::string name = "junk/" + std::to_string(i);
    const Digest d = digest_bytes(reinterpret_cast<const uint8_t*>(name.data()), name.size());
    hc.set_one(d, reinterpret_cast<const uint8_t*>(junk[i].data()), (uint32_t)junk[i].size(), 1, 0,
               now);
  }
  const auto want = [&](const std::string& pat, uint64_t* bytes) {
    size_t n = 0;
    *bytes = 0;
    for (const auto& kv : stored)
      if (match(pat, kv.first)) {
        ++n;
        *bytes += item_bytes((uint32_t)kv.second.size());
      }
    return n;
  };
  uint64_t wb = 0;
  for (const std::string& pat : {std::string("*.css"), std::string("/static/*"),
                                 std::string("/img/*/thumb_*.jpg"), std::string("*/1*"),
                                 std::string("/nothing/*"), std::string("*\xff"),
                                 std::string("/api/v1/users/7"), std::string("/*")}) {
    const size_t n = want(pat, &wb);
    const Listing all = list(hc, pat, 0, kMaxListRows, now);
    CHECK(all.out[kListMatched] == n && all.out[kListBytes] == wb && all.out[kListListed] == n);
    for (const std::string& k : all.keys) CHECK(match(pat, k) && stored.count(k));
    const Listing cnt = list(hc, pat, 0, 0, now);  // count only: no buffer at all
    CHECK(cnt.out[kListMatched] == n && cnt.out[kListListed] == 0);
    std::vector<std::string> paged;  // pages of 7 rows through `next`
    for (uint64_t start = 0; start < 4096;) {
      const Listing pg = list(hc, pat, start, 7, now);
      paged.insert(paged.end(), pg.keys.begin(), pg.keys.end());
      start = pg.out[kListNext];
    }
    CHECK(paged == all.keys);
  }
  CHECK(want("*.css", &wb) == 41);  // (the variant goes with its base key)
  // soften: flags and a capped expiry, the count unchanged by a second pass
  KeyedGlob g;
  CHECK(compile_keyed_glob("/static/*.css", &g, nullptr));
  CHECK(hc.soften_keyed_glob(g, 1234, now + 50, now) == 41);
  CHECK(hc.soften_keyed_glob(g, 1234, now + 80, now) == 41);  // (a life is only shortened)
  CHECK(hc.soften_keyed_glob(g, 1234, 0, now + 50) == 0);     // expired at the cap
  // purge
  uint64_t out[2] = {0, 0};
  CHECK(compile_keyed_glob("/img/*/thumb_*.jpg", &g, nullptr));
  const size_t n_img = want("/img/*/thumb_*.jpg", &wb);
  hc.remove_keyed_glob(g, now, out);
  CHECK(out[0] == n_img && n_img == 40 && out[1] == wb);
  hc.remove_keyed_glob(g, now, out);
  CHECK(out[0] == 0 && out[1] == 0);
  CHECK(list(hc, "/*", 0, 0, now).out[kListMatched] == stored.size() - 40);
  CHECK(compile_keyed_glob(std::string(kMaxGlobLiteral, '\xff'), &g, nullptr));
  hc.remove_keyed_glob(g, now, out);
  CHECK(out[0] == 0);
  CHECK(compile_keyed_glob("*", &g, nullptr) == false);
}

int main() {
  compiler();
  matcher();
  inspect_helpers();
  host_cache();
  std::printf("glob_main: ok\n");
  return 0;
}
