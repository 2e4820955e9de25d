// Stand-alone exercise of the invalidation request's host code (selector.h and the tiers
// that carry it out on the host), built with ASan and UBSan by tests/test_invalidation_tiers.py:
// the selector factories on every refused form; matches_value on truncated and garbage values
// held in exact-size heap copies; write_image against image_bytes(); the fills-in-flight rules;
// ObjectCache's one walk as a removal, a soft purge and a listing over objects spread over its
// stripes, some expired; and a TieredBackend purge with a promotion straddling it.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "backend.h"
#include "object_cache.h"
#include "selector.h"

using namespace shellac;
using Kind = KeyedSelector::Kind;

#define CHECK(c)                                                        \
  do {                                                                  \
    if (!(c)) {                                                         \
      std::fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #c); \
      std::exit(1);                                                     \
    }                                                                   \
  } while (0)

static std::string keyed_value(const std::string& key, const std::string& payload) {
  std::string v(keyed_size(key.size(), payload.size()), '\0');
  write_keyed(reinterpret_cast<uint8_t*>(&v[0]), key, payload.data(), payload.size());
  return v;
}

static std::string tagged(const std::vector<std::string>& tags, const std::string& payload) {
  std::vector<uint64_t> hs;
  for (const std::string& t : tags) hs.push_back(tag_hash(t));
  std::string out(tag_block_size(hs.size()), '\0');
  write_tag_block(reinterpret_cast<uint8_t*>(&out[0]), hs.data(), hs.size());
  return out + payload;
}

// matches_value on a heap copy of exactly v.size() bytes: a read past the value is a report
static bool matches(const KeyedSelector& s, const std::string& v) {
  std::unique_ptr<uint8_t[]> buf(new uint8_t[v.size() ? v.size() : 1]);
  std::memcpy(buf.get(), v.data(), v.size());
  return s.matches_value(buf.get(), v.size());
}

static std::vector<uint64_t> hashes(const std::vector<std::string>& tags) {
  std::vector<uint64_t> hs;
  for (const std::string& t : tags) hs.push_back(tag_hash(t));
  return hs;
}

static std::string stars(int n) {
  std::string p;
  for (int i = 0; i < n; ++i) p += "*a";
  return p;
}

static void factories() {
  CHECK(KeyedSelector().valid() && KeyedSelector().kind == Kind::All);
  CHECK(!KeyedSelector::prefix("").valid() && !KeyedSelector::exact("").valid());
  CHECK(KeyedSelector::prefix("a").valid() && KeyedSelector::exact("a").valid());
  CHECK(KeyedSelector::prefix(std::string(kMaxKeyedKey, 'k')).valid());
  CHECK(!KeyedSelector::prefix(std::string(kMaxKeyedKey + 1, 'k')).valid());
  CHECK(!KeyedSelector::exact(std::string(kMaxKeyedKey + 1, 'k')).valid());
  CHECK(!KeyedSelector::tags({}).valid());
  CHECK(KeyedSelector::tags(std::vector<uint64_t>(1, 7)).valid());
  CHECK(KeyedSelector::tags(std::vector<uint64_t>(kMaxPurgeTags, 7)).valid());
  CHECK(!KeyedSelector::tags(std::vector<uint64_t>(kMaxPurgeTags + 1, 7)).valid());
  const std::map<std::string, std::string> refused = {
      {"", "glob: empty pattern"},
      {"***", "glob: stars only (that is a flush)"},
      {"a\\", "glob: dangling backslash"},
      {stars(kMaxGlobStars + 1), "glob: more than 8 stars"},
      {std::string(kMaxGlobLiteral + 1, 'a'), "glob: more than 1024 literal bytes"}};
  for (const auto& kv : refused) {
    std::string why;
    const KeyedSelector s = KeyedSelector::glob(kv.first, &why);
    CHECK(!s.valid() && !s.compiled && why == kv.second && s.pattern == kv.first);
    CHECK(!KeyedSelector::glob(kv.first).valid());  // (no message wanted)
  }
  CHECK(KeyedSelector::glob(stars(kMaxGlobStars)).valid());
  CHECK(KeyedSelector::glob(std::string(kMaxGlobLiteral, 'a')).valid());
  // what no tier scans for: a refused selector, everything, the removal of one key
  const PurgeAction hard = PurgeAction::remove(), soft = PurgeAction::soften(5, 0);
  CHECK(purge_refused(KeyedSelector(), hard) && purge_refused(KeyedSelector(), soft));
  CHECK(purge_refused(KeyedSelector::exact("a"), hard) && !purge_refused(KeyedSelector::exact("a"), soft));
  CHECK(!purge_refused(KeyedSelector::prefix("a"), hard) && purge_refused(KeyedSelector::prefix(""), soft));
  CHECK(purge_refused(KeyedSelector::glob("*"), hard) && !purge_refused(KeyedSelector::glob("a*"), hard));
  CHECK(soft.soft && soft.stale_at == 5 && soft.keep_s == 0 && !hard.soft);
}

static void values() {
  const KeyedSelector all, pre = KeyedSelector::prefix("/abc"), one = KeyedSelector::exact("/abc"),
                      tag = KeyedSelector::tags(hashes({"x", "y"})),
                      glob = KeyedSelector::glob("/a*c");
  const std::vector<const KeyedSelector*> every = {&all, &pre, &one, &tag, &glob};
  const std::string plain = keyed_value("/abc", "HTTP/ plain");
  const std::string longer = keyed_value("/abcd", tagged({"y"}, "HTTP/ tagged"));
  const std::string variant = keyed_value(std::string("/abc\x1f") + "de", tagged({"z"}, "v"));
  const std::string over = keyed_value("/q", tagged(std::vector<std::string>(40, "t"), "o"));
  CHECK(matches(all, plain) && matches(pre, plain) && matches(one, plain) && matches(glob, plain));
  CHECK(!matches(tag, plain));
  CHECK(matches(pre, longer) && !matches(one, longer) && matches(tag, longer));
  CHECK(!matches(glob, longer));
  CHECK(matches(pre, variant) && !matches(one, variant) && matches(glob, variant));
  CHECK(!matches(tag, variant) && matches(tag, over) && !matches(pre, over));
  // the shapes of purge_cases.garbage_values, and every cut of a good value
  const std::vector<std::string> garbage = {
      std::string(), std::string("/"), std::string("\x88\x13", 2) + "/abc/abc/abc",
      std::string("\x0b\x00", 2) + "/abcdefghi", std::string(40, '\xff'), std::string(2, '\0'),
      std::string("\x00\x00", 2) + "/abc"};
  for (const std::string& v : garbage)
    for (const KeyedSelector* s : every) CHECK(!matches(*s, v));
  for (size_t cut = 0; cut < kKeyedPrefix + 4; ++cut)
    for (const KeyedSelector* s : every) CHECK(!matches(*s, plain.substr(0, cut)));
  CHECK(matches(one, plain.substr(0, 6)) && matches(all, plain.substr(0, 6)));
  for (size_t cut = 0; cut <= longer.size(); ++cut)  // a tag block cut anywhere matches nothing
    CHECK(matches(tag, longer.substr(0, cut)) == (cut >= 2 + 5 + 2 + 8));
  // a refused selector selects nothing, whatever its bytes
  CHECK(!matches(KeyedSelector::prefix(""), plain) && !matches(KeyedSelector::glob("*"), plain));
  CHECK(!matches(KeyedSelector::tags({}), longer));
}

static void images() {
  std::vector<KeyedSelector> sels = {KeyedSelector(), KeyedSelector::tags(hashes({"a"})),
                                     KeyedSelector::tags(hashes({"a", "b"})),
                                     KeyedSelector::tags(std::vector<uint64_t>(kMaxPurgeTags, 9)),
                                     KeyedSelector::glob("/img/*/thumb_*.jpg"),
                                     KeyedSelector::glob(std::string(kMaxGlobLiteral, 'g'))};
  for (size_t plen : {1u, 13u, 14u, 15u, 29u, 30u, 31u, 255u, 65535u}) {
    sels.push_back(KeyedSelector::prefix(std::string(plen, 'p')));
    sels.push_back(KeyedSelector::exact(std::string(plen, 'e')));
  }
  for (const KeyedSelector& s : sels) {
    const size_t n = s.image_bytes();
    CHECK(n % kPurgeGranule == 0 && (n == 0) == (s.kind == Kind::All));
    std::unique_ptr<uint8_t[]> buf(new uint8_t[n ? n : 1]);  // exactly n: a byte more is a report
    std::memset(buf.get(), 0xa5, n);
    s.write_image(buf.get());
    if (s.kind == Kind::Tags) {
      CHECK(n == (s.hashes.size() * 8 + 15) / 16 * 16);
      CHECK(std::memcmp(buf.get(), s.hashes.data(), s.hashes.size() * 8) == 0);
      for (size_t b = s.hashes.size() * 8; b < n; ++b) CHECK(buf[b] == 0);
    } else if (s.kind == Kind::Glob) {
      CHECK(n == keyed_glob_used_bytes(*s.compiled) && n <= sizeof(KeyedGlob));
      CHECK(std::memcmp(buf.get(), s.compiled.get(), n) == 0);
    } else if (n) {
      CHECK(n == keyed_prefix_image_bytes(s.pattern.size()));
      std::vector<uint8_t> want(n);
      write_keyed_prefix_image(want.data(), reinterpret_cast<const uint8_t*>(s.pattern.data()),
                               s.pattern.size());
      CHECK(std::memcmp(buf.get(), want.data(), n) == 0);
    }
  }
}

static void fills_in_flight() {
  const std::string base = "h/page", variant = base + '\x1f' + "de";
  const std::vector<uint64_t> xy = hashes({"x", "y"}), none;
  // prefix: on the key the object would be stored under
  CHECK(KeyedSelector::prefix("h/pa").matches_fill(variant, base, nullptr, false));
  CHECK(KeyedSelector::prefix(base + '\x1f').matches_fill(variant, base, nullptr, false));
  CHECK(!KeyedSelector::prefix(base + '\x1f').matches_fill(base, base, nullptr, false));
  CHECK(!KeyedSelector::prefix("h/q").matches_fill(variant, base, &xy, true));
  // exact: on the base key, so every variant goes with its URL
  CHECK(KeyedSelector::exact(base).matches_fill(variant, base, nullptr, false));
  CHECK(!KeyedSelector::exact(variant).matches_fill(variant, base, nullptr, false));
  CHECK(!KeyedSelector::exact("h/pag").matches_fill(base, base, nullptr, false));
  // glob: on the base key
  CHECK(KeyedSelector::glob("*/page").matches_fill(variant, base, nullptr, false));
  CHECK(!KeyedSelector::glob("*de").matches_fill(variant, base, nullptr, false));
  CHECK(!KeyedSelector::glob("*").matches_fill(variant, base, nullptr, false));  // (refused)
  // tags: tagged fills only; an overflowing fill matches any tag purge
  const KeyedSelector y = KeyedSelector::tags(hashes({"q", "y"})), q = KeyedSelector::tags(hashes({"q"}));
  CHECK(y.matches_fill(base, base, &xy, false) && !q.matches_fill(base, base, &xy, false));
  CHECK(!y.matches_fill(base, base, nullptr, false) && !y.matches_fill(base, base, nullptr, true));
  CHECK(q.matches_fill(base, base, &none, true) && !q.matches_fill(base, base, &none, false));
  // a refused prefix or exact selector compares its bytes as given (an empty prefix: every key)
  CHECK(KeyedSelector::prefix("").matches_fill(variant, base, nullptr, false));
  CHECK(KeyedSelector::exact("").matches_fill("", "", nullptr, false));
  CHECK(!KeyedSelector::exact("").matches_fill(base, base, nullptr, false));
}

static Digest digest_of(const std::string& k) {
  return digest_bytes(reinterpret_cast<const uint8_t*>(k.data()), k.size());
}

// 48 live objects and 8 expired ones over 8 stripes; every third is tagged "t".
struct Objects {
  std::map<std::string, std::string> live, dead;  // key -> payload
  Objects() {
    for (int i = 0; i < 56; ++i) {
      const std::string k = (i % 2 ? "/a/" : "/b/") + std::to_string(i) + (i % 4 < 2 ? ".css" : ".js");
      const std::string p = i % 3 ? "HTTP/ " + std::to_string(i) : tagged({"t"}, "HTTP/ t");
      (i < 48 ? live : dead)[k] = p;
    }
  }
  void store(ObjectCache& oc, uint32_t now) const {
    int i = 0;
    for (const auto& kv : live)
      oc.set(kv.first, digest_of(kv.first), kv.second.data(), kv.second.size(), 3,
             i++ % 2 ? 0 : now + 1000, now);
    for (const auto& kv : dead)
      oc.set(kv.first, digest_of(kv.first), kv.second.data(), kv.second.size(), 3, now - 1, now);
  }
};

static void object_cache_walk() {
  const uint32_t now = 1000;
  const Objects objs;
  const std::vector<KeyedSelector> sels = {
      KeyedSelector::prefix("/a/"), KeyedSelector::exact("/b/4.css"), KeyedSelector::exact("/b/4"),
      KeyedSelector::tags(hashes({"nobody", "t"})), KeyedSelector::glob("/*/*.js"),
      KeyedSelector::glob("*.php"), KeyedSelector::prefix("/"), KeyedSelector()};
  for (const KeyedSelector& s : sels)
    for (int action = 0; action < 2; ++action) {  // 0 soften, 1 remove
      ObjectCache oc(8 << 20, 1 << 20, 8);
      objs.store(oc, now);
      std::map<std::string, std::string> want;
      uint64_t bytes = 0;
      for (const auto& kv : objs.live)
        if (matches(s, keyed_value(kv.first, kv.second))) {
          want.insert(kv);
          bytes += keyed_size(kv.first.size(), kv.second.size());
        }
      // the listing: counts over everything, pages of 5 through the cursor, in key order
      ListQuery q{s, 0, {}};
      ListResult r = oc.list(q, now);
      CHECK(r.ok && r.matched == want.size() && r.bytes == bytes && r.objects.empty());
      std::vector<std::string> listed;
      q.limit = 5;
      for (int page = 0; page < 20; ++page) {
        r = oc.list(q, now);
        CHECK(r.ok && r.matched == want.size() && r.objects.size() <= 5);
        for (const ListedObject& o : r.objects) {
          listed.push_back(o.key);
          CHECK(o.ntags == (want.at(o.key)[0] == (char)kTagMarker ? 1 : 0) && o.flags == 3);
        }
        if (r.next.empty()) break;
        q.after = r.next;
      }
      CHECK(listed.size() == want.size());
      for (size_t i = 0; i + 1 < listed.size(); ++i) CHECK(listed[i] < listed[i + 1]);
      const uint64_t objects0 = oc.stats().objects;
      CHECK(objects0 == objs.live.size() + objs.dead.size());
      CHECK(oc.purge(s, action == 0, 77, action == 0 ? now + 50 : 0, now) == want.size());
      CHECK(oc.stats().objects == objects0 - (action ? want.size() : 0));
      for (const auto& kv : objs.live) {
        Bytes payload;
        uint32_t flags = 0, expire = 0;
        const bool hit = oc.get(kv.first, digest_of(kv.first), now, &payload, &flags, &expire);
        const bool selected = want.count(kv.first) != 0;
        CHECK(hit == !(action && selected));
        if (!hit) continue;
        CHECK(std::string(payload->data(), payload->size()) == kv.second);
        CHECK(flags == (selected ? 77u : 3u));
        if (selected) CHECK(expire == now + 50);  // a never-expiring or later life is capped
        else CHECK(expire == 0 || expire == now + 1000);
      }
      CHECK(oc.purge(s, action == 0, 78, 0, now) == (action ? 0 : want.size()));
      // the expired ones were never counted, listed or touched; a look-up drops them
      for (const auto& kv : objs.dead) {
        Bytes payload;
        CHECK(!oc.get(kv.first, digest_of(kv.first), now, &payload, nullptr, nullptr));
      }
    }
  ObjectCache oc(8 << 20, 1 << 20, 8);
  CHECK(!oc.list(ListQuery{KeyedSelector::prefix(""), 5, {}}, now).ok);
  CHECK(!oc.list(ListQuery{KeyedSelector(), kMaxListRows + 1, {}}, now).ok);
}

// A tier whose GET answers are held until release(): the look-up itself runs at once, as an
// asynchronous tier's does on its own thread.
class HeldBackend : public CacheBackend {
 public:
  HeldBackend() : inner_(8 << 20, 1 << 20, 4) {}
  void get(const std::string& key, const Digest& d, Executor* ex, GetCallback done) override {
    inner_.get(key, d, ex, [this, done](bool hit, CacheValue v) {
      held_.push_back([done, hit, v] { done(hit, v); });
    });
  }
  void set(const std::string& key, const Digest& d, Bytes value, uint32_t flags,
           uint32_t ttl_s) override {
    inner_.set(key, d, std::move(value), flags, ttl_s);
  }
  void del(const std::string& key, const Digest& d, Executor* ex, DelCallback done) override {
    inner_.del(key, d, ex, std::move(done));
  }
  void purge(const KeyedSelector& what, const PurgeAction& how, Executor* ex,
             PurgeCallback done) override {
    inner_.purge(what, how, ex, std::move(done));
  }
  void flush() override { inner_.flush(); }
  std::string name() const override { return "held"; }
  void stats(StatList* out) override { inner_.stats(out); }
  void release() {
    std::vector<std::function<void()>> now;
    now.swap(held_);
    for (auto& f : now) f();
  }

 private:
  DramBackend inner_;
  std::vector<std::function<void()>> held_;
};

static uint64_t stat(CacheBackend& be, const std::string& name) {
  StatList st;
  be.stats(&st);
  for (const auto& kv : st)
    if (kv.first == name) return kv.second;
  CHECK(!"no such stat");
  return 0;
}

static void tiered_purge_and_a_straddling_promotion() {
  for (int soft = 0; soft < 2; ++soft) {
    auto l1 = std::make_shared<DramBackend>(8 << 20, 1 << 20, 4);
    auto l2 = std::make_shared<HeldBackend>();
    TieredBackend tiered(l1, l2);
    const std::string key = "/p/1", other = "/q/1";
    const Bytes body = std::make_shared<const std::string>("HTTP/ body");
    l2->set(key, digest_of(key), body, 3, 0);     // in L2 only: a GET promotes it
    tiered.set(other, digest_of(other), body, 3, 0);
    int answers = 0;
    tiered.get(key, digest_of(key), nullptr, [&](bool hit, CacheValue v) {
      CHECK(hit && v.flags == 3);                 // read before the purge
      ++answers;
    });
    CHECK(answers == 0);
    const PurgeAction how = soft ? PurgeAction::soften(77, 0) : PurgeAction::remove();
    int64_t n = -2;
    tiered.purge(KeyedSelector::prefix("/p/"), how, nullptr, [&](int64_t c) { n = c; });
    CHECK(n == 1);                                // L2's copy; L1 held none
    l2->release();                                // the GET's answer arrives after the purge
    CHECK(answers == 1 && stat(tiered, "tier_promote_dropped_purge") == 1);
    CHECK(stat(tiered, "tier_promoted") == 0 && stat(tiered, "tier_purges") == 1);
    bool l1_hit = true;
    l1->get(key, digest_of(key), nullptr, [&](bool hit, CacheValue) { l1_hit = hit; });
    CHECK(!l1_hit);                               // neither the removed object nor a fresh copy
    tiered.get(key, digest_of(key), nullptr, [&](bool hit, CacheValue v) {
      CHECK(hit == (soft != 0) && (!hit || v.flags == 77));
      ++answers;
    });
    l2->release();
    CHECK(answers == 2);
    // what every tier refuses comes back -1 from both levels, and the other object is untouched
    tiered.purge(KeyedSelector::exact(other), PurgeAction::remove(), nullptr, [&](int64_t c) { n = c; });
    CHECK(n == -1);
    tiered.purge(KeyedSelector::glob("*"), how, nullptr, [&](int64_t c) { n = c; });
    CHECK(n == -1);
    tiered.purge(KeyedSelector::tags(hashes({"t"})), how, nullptr, [&](int64_t c) { n = c; });
    CHECK(n == 0);
    tiered.get(other, digest_of(other), nullptr, [&](bool hit, CacheValue v) {
      CHECK(hit && v.flags == 3);
      ++answers;
    });
    CHECK(answers == 3);                          // (an L1 hit: nothing to release)
  }
}

int main() {
  factories();
  values();
  images();
  fills_in_flight();
  object_cache_walk();
  tiered_purge_and_a_straddling_promotion();
  std::printf("selector_main: ok\n");
  return 0;
}
