// Stand-alone exercise of the listing's host code: keyed_ntags (keyed.h) on exact-size heap
// copies of well-formed, hostile and truncated values; HostCache::list_keyed writing into
// row and key buffers of exactly limit rows (every key_cap, the truncation edge, the granule
// edges, every mode, paging through `next`); the HTTP surface's helpers of inspect.h (query
// parsing, percent-decoding and encoding, JSON key escaping, the (shard, slot) cursor) on
// exact-size strings; and the walk's decisions of hbm_flight_plan.h (which shard is asked
// next for how many rows from where, replica filtering, the next page's cursor), driven
// through whole simulated walks. Built with -fsanitize=address,undefined by
// tests/test_list.py, so a read past a value or a write past a buffer is reported.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "hbm_flight_plan.h"
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

static std::string le64(uint64_t h) {
  std::string s(8, '\0');
  for (int b = 0; b < 8; ++b, h >>= 8) s[b] = (char)h;
  return s;
}

static std::string keyed_value(const std::string& key, const std::string& payload) {
  std::string v(keyed_size(key.size(), payload.size()), '\0');
  write_keyed(reinterpret_cast<uint8_t*>(&v[0]), key, payload.data(), payload.size());
  return v;
}

static uint32_t ntags_exact(const std::string& v) {
  std::unique_ptr<uint8_t[]> buf(new uint8_t[v.size() ? v.size() : 1]);
  std::memcpy(buf.get(), v.data(), v.size());
  return keyed_ntags(buf.get(), v.size());
}

struct Listing {
  uint64_t out[kListWords];
  std::vector<ListRow> rows;
  std::vector<std::string> keys;  // the key bytes cut out of each row's area
};

// One call into buffers of exactly `limit` rows (none for limit 0).
static Listing list(HostCache& hc, uint32_t mode, const std::string& prefix, bool exact,
                    const std::vector<uint64_t>& tags, uint64_t start, uint32_t limit,
                    uint32_t key_cap, uint32_t now) {
  Listing l;
  std::unique_ptr<ListRow[]> rows(limit ? new ListRow[limit] : nullptr);
  std::unique_ptr<uint8_t[]> keys(limit ? new uint8_t[(size_t)limit * key_cap] : nullptr);
  hc.list_keyed(mode, reinterpret_cast<const uint8_t*>(prefix.data()), (uint32_t)prefix.size(),
                exact, tags.data(), (uint32_t)tags.size(), start, limit, key_cap, now, rows.get(),
                keys.get(), l.out);
  CHECK(l.out[kListListed] <= limit && l.out[kListListed] <= l.out[kListMatched]);
  for (uint64_t i = 0; i < l.out[kListListed]; ++i) {
    const ListRow& r = rows[i];
    const uint8_t* const area = keys.get() + i * key_cap;
    uint16_t kl;
    std::memcpy(&kl, area, 2);
    CHECK(kl == r.klen && !(r.bits & kListChanged));
    const size_t have = r.klen < key_cap - 2 ? r.klen : key_cap - 2;
    l.rows.push_back(r);
    l.keys.emplace_back(reinterpret_cast<const char*>(area) + 2, have);
  }
  return l;
}

// ---- the HTTP helpers and the walk's decisions
static std::string exact(const std::string& s) {  // a heap copy with no slack behind it
  return std::string(s.data(), s.size());
}

static void http_helpers() {
  std::string out;
  CHECK(percent_decode(exact("a%2Fb%2fc"), &out) && out == "a/b/c");
  CHECK(percent_decode(exact("%252F+"), &out) && out == "%2F+");            // once; '+' stays
  CHECK(percent_decode(exact("%00%1f%C3%A9"), &out) && out == std::string("\0\x1f\xc3\xa9", 4));
  CHECK(percent_decode(exact(""), &out) && out.empty());
  for (const char* bad : {"%", "%2", "abc%", "abc%4", "%zz", "%2g", "%%41"})
    CHECK(!percent_decode(exact(bad), &out));
  for (int c = 0; c < 256; ++c) {  // encode then decode: every byte comes back
    const std::string one(1, (char)c);
    std::string enc, dec;
    percent_encode(one + "/k" + one, &enc);
    for (unsigned char ch : enc) CHECK(ch > 0x20 && ch < 0x7f && ch != '"' && ch != '&');
    CHECK(percent_decode(enc, &dec) && dec == one + "/k" + one);
  }
  InspectParams p;
  CHECK(parse_inspect_query(exact(""), &p) && p.which == 0 && p.limit == 100 && p.after.empty());
  CHECK(parse_inspect_query(exact("prefix=localhost%2Fstatic%2F&limit=7&after=1.256"), &p));
  CHECK(p.which == 1 && p.value == "localhost/static/" && p.limit == 7 && p.after == "1.256");
  CHECK(parse_inspect_query(exact("limit=0&key=a%1Fb"), &p) && p.which == 2 && p.limit == 0);
  CHECK(p.value == std::string("a\x1f" "b"));
  CHECK(parse_inspect_query(exact("tag=a,b%20c&&"), &p) && p.which == 3 && p.value == "a,b c");
  CHECK(parse_inspect_query(exact("limit=4096"), &p) && p.limit == kMaxListRows);
  CHECK(parse_inspect_query(exact("prefix="), &p) && p.which == 1 && p.value.empty());
  for (const char* bad : {"limit=4097", "limit=", "limit=-1", "limit=1e3", "limit=0000001",
                          "limit=1&limit=2", "prefix=a&key=b", "tag=a&tag=b", "after=1&after=2",
                          "what=1", "prefix=%", "=x"})
    CHECK(!parse_inspect_query(exact(bad), &p));
  CHECK(parse_inspect_query(exact("prefix"), &p) && p.which == 1 && p.value.empty());
  out.clear();
  json_escape_key(exact(std::string("a\"b\\c\x1f" "d\x7f\x80\xff\0e/", 13)), &out);
  CHECK(out == "a\\u0022b\\u005cc\\u001fd\\u007f\\u0080\\u00ff\\u0000e/");
  int shard = -1;
  uint64_t slot = 0;
  CHECK(hbm_cursor(3, 4096) == "3.4096");
  CHECK(hbm_cursor_parse(exact("3.4096"), 4, &shard, &slot) && shard == 3 && slot == 4096);
  CHECK(hbm_cursor_parse(exact("4.0"), 4, &shard, &slot) && shard == 4);   // past the last shard
  CHECK(hbm_cursor_parse(exact("0.18446744073709551615"), 1, &shard, &slot) && slot == ~0ull);
  for (const char* bad : {"", ".", "1.", ".1", "5.0", "1.2.3", "a.1", "1.b", "-1.0", "1 .0",
                          "0.18446744073709551616", "0.99999999999999999999999999999999"})
    CHECK(!hbm_cursor_parse(exact(bad), 4, &shard, &slot));
  ListQuery q;
  CHECK(list_query_valid(q) && q.what.list_mode() == kListAll);
  q.limit = kMaxListRows + 1;
  CHECK(!list_query_valid(q));
  q.limit = 1;
  q.what = KeyedSelector::prefix("");
  CHECK(!list_query_valid(q) && q.what.list_mode() == kListPrefix);
  q.what = KeyedSelector::prefix("a");
  CHECK(list_query_valid(q));
  q.what = KeyedSelector::tags({});
  CHECK(!list_query_valid(q) && q.what.list_mode() == kListTags);
  q.what = KeyedSelector::tags(std::vector<uint64_t>(kMaxPurgeTags + 1, 1));
  CHECK(!list_query_valid(q));
  q.what = KeyedSelector::tags(std::vector<uint64_t>(kMaxPurgeTags, 1));
  CHECK(list_query_valid(q));
}

// A walk over simulated shards: shard k holds own[k] objects of its own and repl[k] replicas of
// other shards' objects, replicas and owned rows interleaved in slot order (slot = row index).
// Pages of `limit` through the cursor must hand out every owned object exactly once.
static void walk_decisions(const std::vector<int>& own, const std::vector<int>& repl,
                           uint64_t up_mask, uint32_t limit) {
  const int n = (int)own.size();
  const uint64_t nslots = 64;
  std::vector<std::vector<int>> seen((size_t)n);
  std::vector<std::vector<char>> is_repl((size_t)n);   // replicas first, then alternating
  for (int k = 0; k < n; ++k) {
    int o = 0, p = 0;
    while (o < own[(size_t)k] || p < repl[(size_t)k]) {
      const bool rep = p < repl[(size_t)k] && ((o + p) % 2 == 0 || o >= own[(size_t)k]);
      is_repl[(size_t)k].push_back(rep);
      (rep ? p : o)++;
    }
  }
  std::string after;
  uint32_t skipped_want = 0;
  for (int k = 0; k < n; ++k) skipped_want += !((up_mask >> k) & 1);
  for (int page = 0; page < 1000; ++page) {
    int cur_shard = 0;
    uint64_t cur_slot = 0;
    CHECK(after.empty() || hbm_cursor_parse(after, n, &cur_shard, &cur_slot));
    uint32_t got = 0, skipped = 0;
    uint64_t matched = 0;
    bool have_next = false;
    std::string next;
    int at = -1;
    for (;;) {
      const ListAsk a = list_next_ask(at, cur_shard, cur_slot, have_next, limit - got, up_mask, n);
      skipped += a.skipped;
      if (a.shard < 0) break;
      CHECK(a.shard > at && ((up_mask >> a.shard) & 1) && a.limit <= limit - got);
      at = a.shard;
      const int rows = own[(size_t)at] + repl[(size_t)at];
      CHECK((uint64_t)rows <= nslots);
      matched += (uint64_t)rows;
      uint32_t listed = 0;
      uint64_t next_slot = nslots;
      for (int r = (int)a.start; r < rows; ++r) {
        if (listed == a.limit) {
          next_slot = (uint64_t)r;
          break;
        }
        ++listed;
        const bool replica = is_repl[(size_t)at][(size_t)r];
        if (list_row_is_replica(replica ? (at + 1) % n : at, at)) continue;
        seen[(size_t)at].push_back(r);
        ++got;
      }
      if (!have_next) {
        next = list_cursor_after(at, a.limit, limit - got, next_slot, nslots, n);
        have_next = !next.empty();
      }
    }
    CHECK(got <= limit && skipped == skipped_want);
    uint64_t want_matched = 0;
    for (int k = 0; k < n; ++k)
      if ((up_mask >> k) & 1) want_matched += (uint64_t)(own[(size_t)k] + repl[(size_t)k]);
    CHECK(matched == want_matched);   // the totals cover every shard in service on every page
    if (next.empty()) break;
    after = next;
    CHECK(page < 999);
  }
  for (int k = 0; k < n; ++k) {
    const size_t want = ((up_mask >> k) & 1) ? (size_t)own[(size_t)k] : 0;
    CHECK(seen[(size_t)k].size() == want);
    for (size_t i = 1; i < seen[(size_t)k].size(); ++i)
      CHECK(seen[(size_t)k][i - 1] < seen[(size_t)k][i]);   // once each, in slot order
  }
}

static void flight_plan_decisions() {
  CHECK(!list_row_is_replica(2, 2) && list_row_is_replica(1, 2) && !list_row_is_replica(-1, 2));
  ListAsk a = list_next_ask(-1, 1, 77, false, 10, 0b110, 3);
  CHECK(a.shard == 1 && a.start == 77 && a.limit == 10 && a.skipped == 1);
  a = list_next_ask(-1, 1, 77, false, 10, 0b111, 3);
  CHECK(a.shard == 0 && a.limit == 0 && a.skipped == 0);           // before the cursor: counts
  a = list_next_ask(1, 1, 77, false, 4, 0b111, 3);
  CHECK(a.shard == 2 && a.start == 0 && a.limit == 4);
  a = list_next_ask(1, 1, 77, true, 4, 0b111, 3);
  CHECK(a.shard == 2 && a.limit == 0);                             // the cursor is known: counts
  a = list_next_ask(2, 0, 0, false, 4, 0b111, 3);
  CHECK(a.shard == -1);
  a = list_next_ask(-1, 0, 0, false, 4, 0, 3);
  CHECK(a.shard == -1 && a.skipped == 3);
  CHECK(list_cursor_after(1, 10, 0, 40, 64, 3) == "1.40");
  CHECK(list_cursor_after(1, 10, 0, 64, 64, 3) == "2.0");
  CHECK(list_cursor_after(2, 10, 0, 64, 64, 3).empty());
  CHECK(list_cursor_after(1, 10, 3, 64, 64, 3).empty());
  CHECK(list_cursor_after(1, 0, 0, 5, 64, 3).empty());
  std::vector<HbmReq> qd(3);
  qd[0].kind = ReqKind::Set;
  qd[1].kind = ReqKind::List;
  qd[2].kind = ReqKind::Set;
  CHECK(plan_take(qd, 16) == 2);                                   // a list ends its flight
  for (uint32_t limit : {1u, 2u, 3u, 7u, 64u})
    for (uint64_t up : {0b111ull, 0b101ull, 0b110ull, 0b010ull, 0ull}) {
      walk_decisions({5, 0, 9}, {0, 0, 0}, up, limit);
      walk_decisions({5, 3, 9}, {4, 1, 0}, up, limit);
      walk_decisions({0, 0, 0}, {2, 2, 2}, up, limit);
      walk_decisions({7, 7, 7}, {7, 0, 3}, up, limit);
    }
}

int main() {
  http_helpers();
  flight_plan_decisions();
  const uint64_t t = tag_hash("product-4711"), u = tag_hash("other");
  const std::string http = "HTTP/1.1 200 OK\r\n\r\nok";

  // ---- keyed_ntags on exact-size copies
  for (size_t klen = 0; klen <= 40; ++klen) {
    const std::string key(klen, 'k');
    CHECK(ntags_exact(keyed_value(key, http)) == 0);
    CHECK(ntags_exact(keyed_value(key, "")) == 0);
    CHECK(ntags_exact(keyed_value(key, "\x02")) == 0);
    CHECK(ntags_exact(keyed_value(key, std::string("\x02\x00", 2) + http)) == 0);
    CHECK(ntags_exact(keyed_value(key, std::string("\x02\xff", 2))) == kTagOverflow);
    CHECK(ntags_exact(keyed_value(key, std::string("\x02\x02", 2) + le64(t) + le64(u))) == 2);
    CHECK(ntags_exact(keyed_value(key, std::string("\x02\x02", 2) + le64(t) + le64(u).substr(0, 7))) == 0);
    CHECK(ntags_exact(keyed_value(key, std::string("\x02\x21", 2) + std::string(33 * 8, 'x'))) == 0);
    const std::string full = keyed_value(key, std::string("\x02\x01", 2) + le64(t));
    for (size_t cut = 0; cut < full.size(); ++cut) CHECK(ntags_exact(full.substr(0, cut)) == 0);
    CHECK(ntags_exact(full) == 1);
  }

  // ---- HostCache::list_keyed
  HostCache hc(1 << 20, 1 << 10, 4096);
  const uint64_t nslots = 4096;
  const uint32_t now = 10;
  std::map<std::string, std::string> stored;  // key -> keyed value
  int id = 0;
  for (size_t klen : {1, 11, 12, 13, 14, 15, 16, 27, 28, 29, 30, 31, 45, 46, 61, 62, 63, 64, 84,
                      300, 1021, 1022, 1023, 1100}) {
    for (const std::string& payload :
         {std::string(), http, std::string("\x02\x01", 2) + le64(t) + http,
          std::string("\x02\xff", 2), std::string("\x02\x02", 2) + le64(u) + le64(t)}) {
      std::string key(klen, 'a');
      key[0] = (char)(33 + id % 90);
      if (klen > 1) key[1] = (char)(33 + id / 90);
      ++id;
      stored[key] = keyed_value(key, payload);
    }
  }
  for (const auto& kv : stored) {
    const Digest d = digest_bytes(reinterpret_cast<const uint8_t*>(kv.first.data()), kv.first.size());
    hc.set_one(d, reinterpret_cast<const uint8_t*>(kv.second.data()), (uint32_t)kv.second.size(), 7,
               now + 100, now);
  }
  // non-keyed junk (purge_cases.garbage_values): never listed
  const std::vector<std::string> junk = {"", "/", std::string("\x88\x13", 2) + "/abc/abc/abc",
                                         std::string("\x0b\x00", 2) + "/abcdefghi",
                                         std::string(40, '\xff'), std::string("\x00\x00", 2)};
  for (size_t i = 0; i < junk.size(); ++i) {
    const std::string name = "junk/" + std::to_string(i);
    const Digest d = digest_bytes(reinterpret_cast<const uint8_t*>(name.data()), name.size());
    hc.set_one(d, reinterpret_cast<const uint8_t*>(junk[i].data()), (uint32_t)junk[i].size(), 1, 0,
               now);
  }
  size_t want_tagged = 0;
  uint64_t want_bytes = 0;
  for (const auto& kv : stored) {
    want_tagged += keyed_tags_match(reinterpret_cast<const uint8_t*>(kv.second.data()),
                                    kv.second.size(), &t, 1);
    want_bytes += item_bytes((uint32_t)kv.second.size());
  }
  CHECK(want_tagged == stored.size() / 5 * 3);

  for (uint32_t key_cap : {16u, 32u, 64u, 256u, 1024u}) {
    const Listing all = list(hc, kListAll, "", false, {}, 0, kMaxListRows, key_cap, now);
    CHECK(all.out[kListMatched] == stored.size() && all.out[kListBytes] == want_bytes);
    CHECK(all.out[kListListed] == stored.size() && all.out[kListNext] == nslots);
    for (size_t i = 0; i < all.rows.size(); ++i) {
      const ListRow& r = all.rows[i];
      CHECK(i == 0 || all.rows[i - 1].slot < r.slot);
      CHECK(r.slot < nslots && r.flags == 7 && r.expire == now + 100);
      // the row's object: found by the listed head of the key and its length
      size_t found = 0;
      for (const auto& kv : stored)
        if (kv.first.size() == r.klen && kv.first.compare(0, all.keys[i].size(), all.keys[i]) == 0) {
          ++found;
          CHECK(r.vlen == kv.second.size());
          CHECK(r.ntags == keyed_ntags(reinterpret_cast<const uint8_t*>(kv.second.data()),
                                       kv.second.size()));
        }
      CHECK(found == 1);
      CHECK(all.keys[i].size() == (r.klen < key_cap - 2 ? r.klen : key_cap - 2));
    }
    // count only: no buffer at all
    const Listing cnt = list(hc, kListAll, "", false, {}, 0, 0, key_cap, now);
    CHECK(cnt.out[kListMatched] == stored.size() && cnt.out[kListListed] == 0);
    CHECK(cnt.out[kListNext] == nslots);
    // pages of 1, 7 and 64 rows through `next`, into buffers of exactly that many rows
    for (uint32_t limit : {1u, 7u, 64u}) {
      std::vector<uint64_t> slots;
      uint64_t start = 0;
      while (start < nslots) {
        const Listing p = list(hc, kListAll, "", false, {}, start, limit, key_cap, now);
        CHECK(p.out[kListMatched] == stored.size() && p.out[kListBytes] == want_bytes);
        for (const ListRow& r : p.rows) slots.push_back(r.slot);
        CHECK(p.out[kListNext] == nslots || p.rows.size() == limit);
        start = p.out[kListNext];
      }
      CHECK(slots.size() == all.rows.size());
      for (size_t i = 0; i < slots.size(); ++i) CHECK(slots[i] == all.rows[i].slot);
    }
  }
  // the other modes, the exact flag, the start slot's edges, expiry
  const Listing tagged = list(hc, kListTags, "", false, {u ^ 1, t}, 0, kMaxListRows, 64, now);
  CHECK(tagged.out[kListMatched] == want_tagged && tagged.rows.size() == want_tagged);
  const std::string one = stored.begin()->first;
  const Listing ex = list(hc, kListPrefix, one, true, {}, 0, 8, 1024, now);
  CHECK(ex.out[kListMatched] == 1 && ex.keys.size() == 1 && ex.keys[0] == one);
  const Listing pre = list(hc, kListPrefix, one.substr(0, 1), false, {}, 0, kMaxListRows, 1024, now);
  size_t want_pre = 0;
  for (const auto& kv : stored) want_pre += kv.first[0] == one[0];
  CHECK(pre.out[kListMatched] == want_pre && pre.rows.size() == want_pre);
  const uint64_t last = pre.rows.back().slot;
  CHECK(list(hc, kListPrefix, one.substr(0, 1), false, {}, last, 4, 16, now).rows.size() == 1);
  CHECK(list(hc, kListPrefix, one.substr(0, 1), false, {}, last + 1, 4, 16, now).rows.empty());
  CHECK(list(hc, kListPrefix, one.substr(0, 1), false, {}, nslots, 4, 16, now).rows.empty());
  CHECK(list(hc, kListAll, "", false, {}, 0, 4, 16, now + 100).out[kListMatched] == 0);  // expired
  int threw = 0;
  for (int bad = 0; bad < 6; ++bad) {
    try {
      if (bad == 0) list(hc, kListPrefix, "", false, {}, 0, 4, 16, now);
      if (bad == 1) list(hc, kListTags, "", false, {}, 0, 4, 16, now);
      if (bad == 2) list(hc, kListAll, "", false, {}, nslots + 1, 4, 16, now);
      if (bad == 3) list(hc, kListAll, "", false, {}, 0, kMaxListRows + 1, 16, now);
      if (bad == 4) list(hc, kListAll, "", false, {}, 0, 4, 24, now);
      if (bad == 5) list(hc, 3, "", false, {}, 0, 4, 16, now);
    } catch (const std::exception&) {
      ++threw;
    }
  }
  CHECK(threw == 6);
  std::printf("list_main: ok (%zu objects, %zu tagged)\n", stored.size(), want_tagged);
  return 0;
}
