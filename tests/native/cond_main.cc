// Stand-alone exercise of the conditional sliced GET's host code: cond_find_field and
// cond_matches on exact-size heap copies of values whose validator line starts on the granule
// and wave-pass seams, against a std::string model; conditions whose records overrun their
// range or number more than kCondMaxCandidates, with candidate buffers of exactly the range's
// size; the request-header parsers on exact-size strings; and HostCache::get_keyed_slices with
// conditions, writing into row and response buffers of exactly the needed size. Built with
// -fsanitize=address,undefined by tests/test_conditional.py, so a read past a value, a head or a
// candidate range and a write past a buffer are reported.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "conditional.h"
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

// A head whose header line `line` starts exactly n bytes into it.
static std::string line_at(size_t n, const std::string& line) {
  const std::string base = "HTTP/1.1 200 OK\r\nX-P: ";
  CHECK(n >= base.size() + 2);
  return base + std::string(n - base.size() - 2, 'a') + "\r\n" + line + "\r\n\r\n";
}

static std::unique_ptr<uint8_t[]> exact(const std::string& s) {
  std::unique_ptr<uint8_t[]> b(new uint8_t[s.size() ? s.size() : 1]);
  std::memcpy(b.get(), s.data(), s.size());
  return b;
}

static std::string record(const std::string& t) { return std::string(1, (char)t.size()) + t; }

// ---- the model: the head as a string, lines split at CR LF
static std::string lower(std::string s) {
  for (char& c : s)
    if (c >= 'A' && c <= 'Z') c = (char)(c + 32);
  return s;
}

static bool model_field(const std::string& head, const std::string& name, std::string* val) {
  const size_t e = head.size() - 4;
  size_t p = head.find("\r\n");
  while (p != std::string::npos && p + 2 <= e) {  // every CR LF starts a line behind it
    const size_t s = p + 2;
    const std::string pat = name + ":";
    if (s + pat.size() <= e && lower(head.substr(s, pat.size())) == pat) {
      const size_t c = s + pat.size(), qq = head.find("\r\n", c);
      if (qq - c > kCondLineMax) return false;
      std::string v = head.substr(c, qq - c);
      while (!v.empty() && (v[0] == ' ' || v[0] == '\t')) v.erase(0, 1);
      while (!v.empty() && (v.back() == ' ' || v.back() == '\t')) v.pop_back();
      *val = v;
      return true;
    }
    p = head.find("\r\n", p + 1);
  }
  return false;
}

static bool model_matches(const std::string& head, uint32_t kind, const std::vector<std::string>& cands) {
  if (cands.empty()) return kind == kCondNoneMatch;
  std::string v;
  if (kind == kCondNoneMatch || kind == kCondIfRangeEtag) {
    if (!model_field(head, "etag", &v)) return false;
    const bool weak = v.compare(0, 2, "W/") == 0;
    if (weak) v.erase(0, 2);
    if (v.size() < 2 || v.size() > kCondValueMax || v[0] != '"' || v.back() != '"') return false;
    if (weak && kind == kCondIfRangeEtag) return false;
  } else {
    if (!model_field(head, "last-modified", &v) || v.empty() || v.size() > kCondValueMax) return false;
  }
  for (const std::string& c : cands)
    if (c == v) return true;
  return false;
}

// cond_matches on a copy of the value that ends with its head (nothing behind the blank line)
// and a candidate buffer of exactly the range's size.
static bool matches_exact(const std::string& value, uint32_t kind, const std::vector<std::string>& cands) {
  uint32_t ho, bo;
  CHECK(slice_layout(reinterpret_cast<const uint8_t*>(value.data()), value.size(), &ho, &bo));
  const std::unique_ptr<uint8_t[]> v = exact(value.substr(0, bo));
  std::string rec;
  for (const std::string& c : cands) rec += record(c);
  const std::unique_ptr<uint8_t[]> cb = exact(rec);
  const SliceCond c{kind, (uint32_t)cands.size(), 0, (uint32_t)rec.size()};
  const bool got = cond_matches(v.get(), ho, bo, c, rec.empty() ? nullptr : cb.get());
  CHECK(got == model_matches(value.substr(ho, bo - ho), kind, cands));
  return got;
}

static const std::string kTag = "\"v1\"", kOther = "\"v2\"", kDate = "Wed, 21 Oct 2015 07:28:00 GMT";

static std::vector<std::string> seam_values(std::vector<std::string>* keys) {
  std::vector<std::string> vals;
  for (size_t klen : {1u, 6u, 13u, 14u, 30u}) {
    const size_t head_off = 2 + klen, start = (head_off + 2) & ~(size_t)15;
    for (size_t at : {40u, 41u, 46u, 47u, 48u, 49u, 1010u, 1019u, 1020u, 1021u, 1022u, 1023u, 1024u, 1025u,
                      2046u, 2047u, 2048u, 2049u})
      for (int lm = 0; lm < 2; ++lm) {
        std::string key = std::string(1, (char)('0' + keys->size() % 36)) + "/seam/key/padded/to/its/length";
        key.resize(klen);
        if (klen == 1) key[0] = (char)('0' + keys->size());
        keys->push_back(key);
        const std::string line = lm ? "LAST-modified:\t" + kDate : "eTaG:" + kTag;
        vals.push_back(keyed_value(key, line_at(start + at - head_off, line) + "body bytes"));
      }
  }
  return vals;
}

static void fields() {
  std::vector<std::string> keys;
  size_t hits = 0;
  for (const std::string& v : seam_values(&keys)) {
    hits += matches_exact(v, kCondNoneMatch, {kTag});
    hits += matches_exact(v, kCondModifiedSince, {kDate});
    CHECK(!matches_exact(v, kCondNoneMatch, {kOther}));
    CHECK(!matches_exact(v, kCondIfRangeDate, {kDate + "x", ""}));
    CHECK(matches_exact(v, kCondNoneMatch, {}));
    CHECK(!matches_exact(v, kCondIfRangeEtag, {}));
  }
  CHECK(hits == keys.size());
  const auto value = [](const std::string& lines) {
    return keyed_value("/k", "HTTP/1.1 200 OK\r\n" + lines + "\r\n\r\n" + "body");
  };
  CHECK(matches_exact(value("ETag: " + kTag), kCondNoneMatch, {kOther, kTag}));
  CHECK(matches_exact(value("ETag:" + kTag), kCondIfRangeEtag, {kTag}));
  CHECK(matches_exact(value("ETag: W/" + kTag), kCondNoneMatch, {kTag}));
  CHECK(!matches_exact(value("ETag: W/" + kTag), kCondIfRangeEtag, {kTag}));
  CHECK(!matches_exact(value("X-ETag: " + kTag), kCondNoneMatch, {kTag}));
  CHECK(!matches_exact(value("X-A: etag: " + kTag), kCondNoneMatch, {kTag}));
  CHECK(!matches_exact(value("ETag : " + kTag), kCondNoneMatch, {kTag}));
  CHECK(!matches_exact(value("X-A: b\nETag: " + kTag), kCondNoneMatch, {kTag}));
  CHECK(!matches_exact(value("X-A: b\r\nETag"), kCondNoneMatch, {kTag}));       // the head ends "ETag\r\n\r\n"
  CHECK(!matches_exact(value("X-A: b\r\nETag:"), kCondNoneMatch, {kTag}));      // an empty value
  CHECK(!matches_exact(value("X-A: b\r\nETag: \t "), kCondNoneMatch, {""}));
  CHECK(!matches_exact(value(""), kCondNoneMatch, {kTag}));                     // no header line
  CHECK(matches_exact(value("ETag: " + kTag + "\r\nETag: " + kOther), kCondNoneMatch, {kTag}));
  CHECK(!matches_exact(value("ETag: " + kOther + "\r\nETag: " + kTag), kCondNoneMatch, {kTag}));
  CHECK(matches_exact(value("Last-Modified: " + kDate + "\r\nETag: " + kTag), kCondIfRangeDate, {kDate}));
  for (size_t raw : {511u, 512u, 513u}) {
    const std::string pad(raw - kTag.size(), ' ');
    CHECK(matches_exact(value("ETag:" + pad + kTag), kCondNoneMatch, {kTag}) == (raw <= 512));
    CHECK(matches_exact(value("ETag:" + kTag + pad), kCondNoneMatch, {kTag}) == (raw <= 512));
  }
  for (size_t n : {2u, 3u, 64u, 254u, 255u, 256u}) {
    const std::string t = "\"" + std::string(n - 2, 'x') + "\"";
    CHECK(matches_exact(value("ETag: " + t), kCondNoneMatch, {t.substr(0, 255)}) == (n <= 255));
    const std::string d(n, 'D');
    CHECK(matches_exact(value("Last-Modified: " + d), kCondModifiedSince, {d.substr(0, 255)}) ==
          (n <= 255));
  }
}

// ---- malformed conditions: the candidate buffer is exactly [off, off + len)
static void malformed() {
  const std::string v = keyed_value("/k", "HTTP/1.1 200 OK\r\nETag: " + kTag + "\r\n\r\nbody");
  uint32_t ho, bo;
  CHECK(slice_layout(reinterpret_cast<const uint8_t*>(v.data()), v.size(), &ho, &bo));
  const uint8_t* const p = reinterpret_cast<const uint8_t*>(v.data());
  const std::string rec = record(kTag);
  const auto run = [&](uint32_t kind, uint32_t ncand, const std::string& bytes) {
    const std::unique_ptr<uint8_t[]> cb = exact(bytes);
    const SliceCond c{kind, ncand, 0, (uint32_t)bytes.size()};
    return cond_matches(p, ho, bo, c, cb.get());
  };
  CHECK(run(kCondNoneMatch, 1, rec));
  for (size_t cut = 0; cut < rec.size(); ++cut) CHECK(!run(kCondNoneMatch, 1, rec.substr(0, cut)));
  CHECK(run(kCondNoneMatch, 2, record(kOther) + rec));
  for (size_t cut = 0; cut < rec.size(); ++cut)  // a good first record, the second overruns
    CHECK(!run(kCondNoneMatch, 2, rec + rec.substr(0, cut)));
  CHECK(!run(kCondNoneMatch, 2, rec));
  std::string many;
  for (int i = 0; i < 17; ++i) many += rec;
  CHECK(run(kCondNoneMatch, 16, many.substr(0, 16 * rec.size())));
  CHECK(!run(kCondNoneMatch, 17, many) && !run(kCondNoneMatch, ~0u, rec));
  CHECK(run(kCondNoneMatch, 0, "") && run(kCondNoneMatch, 0, rec));  // "*"
  CHECK(!run(kCondModifiedSince, 0, "") && !run(kCondIfRangeEtag, 0, "") && !run(kCondIfRangeDate, 0, ""));
  CHECK(!run(kCondNone, 1, rec) && !run(5, 1, rec) && !run(~0u, 1, rec));
  const SliceCond star{kCondNoneMatch, 0, 0, 0}, lost{kCondNoneMatch, 1, 0, 5};
  CHECK(cond_matches(p, ho, bo, star, nullptr) && !cond_matches(p, ho, bo, lost, nullptr));
  // a range in the middle of a buffer: only [off, off + len) counts
  const std::string mid = "\x04" + rec + kTag;
  const std::unique_ptr<uint8_t[]> mb = exact(mid);
  CHECK(cond_matches(p, ho, bo, SliceCond{kCondNoneMatch, 1, 1, (uint32_t)rec.size()}, mb.get()));
  CHECK(!cond_matches(p, ho, bo, SliceCond{kCondNoneMatch, 1, 0, 4}, mb.get()));
  // what a condition does to a row
  uint32_t kind = kSliceRange;
  CHECK(cond_outcome(kCondNoneMatch, true, &kind) && kind == kSliceHead);
  kind = kSliceRange;
  CHECK(!cond_outcome(kCondModifiedSince, false, &kind) && kind == kSliceRange);
  CHECK(!cond_outcome(kCondIfRangeEtag, true, &kind) && kind == kSliceRange);
  CHECK(!cond_outcome(kCondIfRangeDate, false, &kind) && kind == kSliceWhole);
  kind = kSliceFrom;
  CHECK(!cond_outcome(kCondNone, true, &kind) && !cond_outcome(77, false, &kind) && kind == kSliceFrom);
  SliceRow r;
  slice_make_row_if(&r, kSliceRange, 0, 9, (uint32_t)v.size(), 5, 0, true, ho, bo, kCondNoneMatch, true);
  CHECK(r.status == kSliceNotModified && r.win_len == 0 && slice_row_payload(r) == bo &&
        slice_row_bytes(r) == align_up(bo, 16));
  slice_make_row_if(&r, kSliceRange, 0, 9, (uint32_t)v.size(), 5, 0, false, 0, 0, kCondNoneMatch, true);
  CHECK(r.status == kSliceWholeObj);
}

// ---- the request headers, on heap copies with no slack behind them
static bool inm(const std::string& s, CondRequest* c) {
  const std::unique_ptr<uint8_t[]> e = exact(s);
  return parse_if_none_match(reinterpret_cast<const char*>(e.get()), s.size(), c);
}
static bool ifr(const std::string& s, CondRequest* c) {
  const std::unique_ptr<uint8_t[]> e = exact(s);
  return parse_if_range(reinterpret_cast<const char*>(e.get()), s.size(), c);
}
static bool ims(const std::string& s, CondRequest* c) {
  const std::unique_ptr<uint8_t[]> e = exact(s);
  return parse_if_modified_since(reinterpret_cast<const char*>(e.get()), s.size(), c);
}

static void headers() {
  CondRequest c;
  CHECK(inm("*", &c) && c.kind == kCondNoneMatch && c.ncand == 0 && c.records.empty());
  CHECK(inm(" * ", &c) && c.ncand == 0);
  CHECK(inm("\"a\"", &c) && c.ncand == 1 && c.records == record("\"a\""));
  CHECK(inm("W/\"a\"", &c) && c.ncand == 1 && c.records == record("\"a\""));
  CHECK(inm(" \"a\" ,\tW/\"b\" ", &c) && c.ncand == 2 && c.records == record("\"a\"") + record("\"b\""));
  CHECK(inm("\"a,b\", \"c\"", &c) && c.ncand == 2 && c.records == record("\"a,b\"") + record("\"c\""));
  CHECK(inm("\"a\",,\"b\",", &c) && c.ncand == 2);
  CHECK(inm("\"\"", &c) && c.ncand == 1 && c.records == record("\"\""));
  std::string list16, big = "\"" + std::string(253, 'x') + "\"";
  for (int i = 0; i < 16; ++i) list16 += (i ? ", \"" : "\"") + std::to_string(i) + "\"";
  CHECK(inm(list16, &c) && c.ncand == 16);
  CHECK(!inm(list16 + ", \"16\"", &c));
  CHECK(inm(big, &c) && c.records.size() == 256 && inm("W/" + big, &c));
  CHECK(!inm("\"" + std::string(254, 'x') + "\"", &c));
  for (const char* bad : {"", " ", ",", "\"a", "a\"", "a", "\"a\" \"b\"", "\"a\"x", "*, \"a\"", "\"a\", *",
                          "w/\"a\"", "W/W/\"a\"", "W/", "W", "\"a b\"", "\"a\x7f\"", "\"a\"\r\n", "**"})
    CHECK(!inm(bad, &c));
  CHECK(ifr("\"a\"", &c) && c.kind == kCondIfRangeEtag && c.ncand == 1 && c.records == record("\"a\""));
  CHECK(ifr(" \"a,b\"\t", &c) && c.records == record("\"a,b\""));
  CHECK(ifr(kDate, &c) && c.kind == kCondIfRangeDate && c.records == record(kDate));
  CHECK(ifr(" " + kDate + " ", &c) && c.records == record(kDate));
  CHECK(ifr(std::string(255, 'x'), &c) && ifr(big, &c) && c.kind == kCondIfRangeEtag);
  for (const std::string& bad : {std::string(""), std::string(" \t"), std::string("W/\"a\""), std::string("\"a"),
                                 std::string("\"a\"b"), std::string("\""), std::string(256, 'x'),
                                 std::string("W/")})
    CHECK(!ifr(bad, &c));
  CHECK(ims(kDate, &c) && c.kind == kCondModifiedSince && c.ncand == 1 && c.records == record(kDate));
  CHECK(ims("  " + kDate + "\t", &c) && c.records == record(kDate));
  CHECK(!ims("", &c) && !ims("  ", &c) && !ims(std::string(256, 'x'), &c) && ims(std::string(255, 'x'), &c));
}

// ---- the twin, into buffers of exactly the needed size
static void twin() {
  HostCache hc(1u << 20, 1024, 8192);
  std::vector<std::string> keys;
  std::vector<std::string> vals = seam_values(&keys);
  keys.push_back("/vary");
  vals.push_back(keyed_value("/vary", "\x01" "accept-encoding"));
  const uint32_t now = 10;
  for (size_t i = 0; i < keys.size(); ++i) {
    const Digest d = digest_bytes(reinterpret_cast<const uint8_t*>(keys[i].data()), keys[i].size());
    hc.set_one(d, reinterpret_cast<const uint8_t*>(vals[i].data()), (uint32_t)vals[i].size(), 5, 0, now);
  }
  struct Form {
    uint32_t kind;
    std::vector<std::string> cands;
  };
  const Form forms[] = {{kCondNone, {}},
                        {kCondNoneMatch, {kTag}},
                        {kCondNoneMatch, {kOther}},
                        {kCondNoneMatch, {}},
                        {kCondModifiedSince, {kDate}},
                        {kCondIfRangeEtag, {kTag}},
                        {kCondIfRangeEtag, {kOther}},
                        {kCondIfRangeDate, {kDate}},
                        {kCondIfRangeDate, {"x"}}};
  const SliceSpec specs[] = {{kSliceRange, 0, 3, 7}, {kSliceWhole, 0, 0, 0}, {kSliceHead, 0, 0, 0},
                             {kSliceRange, 0, 99, 100}};
  size_t not_modified = 0, whole = 0;
  for (const SliceSpec& sp : specs) {
    // one batch: every value under a rotating form, with a miss now and then
    std::vector<std::string> bk, want;
    std::vector<SliceSpec> bs;
    std::vector<SliceCond> bc;
    std::string cbytes;
    for (size_t i = 0; i < keys.size(); ++i) {
      const Form& f = forms[(i + sp.kind) % (sizeof(forms) / sizeof(forms[0]))];
      const uint32_t off = (uint32_t)cbytes.size();
      for (const std::string& c : f.cands) cbytes += record(c);
      bk.push_back(keys[i]);
      bs.push_back(sp);
      bc.push_back(SliceCond{f.kind, (uint32_t)f.cands.size(), off, (uint32_t)cbytes.size() - off});
      want.push_back(vals[i]);
      if (i % 7 == 0) {
        bk.push_back(keys[i] + "?missing");
        bs.push_back(sp);
        bc.push_back(bc.back());
        want.push_back("");
      }
    }
    const int64_t n = (int64_t)bk.size();
    std::vector<Digest> d((size_t)n);
    std::string kb;
    std::vector<int64_t> offs((size_t)n + 1, 0);
    for (int64_t i = 0; i < n; ++i) {
      d[(size_t)i] = digest_bytes(reinterpret_cast<const uint8_t*>(bk[(size_t)i].data()), bk[(size_t)i].size());
      kb += bk[(size_t)i];
      offs[(size_t)i + 1] = (int64_t)kb.size();
    }
    const std::unique_ptr<uint8_t[]> kbuf = exact(kb), cbuf = exact(cbytes);
    std::unique_ptr<SliceRow[]> rows(new SliceRow[(size_t)n]);
    std::unique_ptr<SliceCond[]> conds(new SliceCond[(size_t)n]);
    std::memcpy(conds.get(), bc.data(), (size_t)n * sizeof(SliceCond));
    uint64_t res[kSliceWords] = {0, 0};
    const CacheCounters c0 = hc.counters();
    hc.get_keyed_slices(d.data(), kbuf.get(), offs.data(), bs.data(), n, rows.get(), nullptr, 0, res, now, 0,
                        conds.get(), cbuf.get());
    const uint64_t total = res[kSliceBytes];
    std::unique_ptr<uint8_t[]> out(new uint8_t[total ? total : 1]);
    hc.get_keyed_slices(d.data(), kbuf.get(), offs.data(), bs.data(), n, rows.get(), out.get(), total, res,
                        now, 0, conds.get(), cbuf.get());
    CHECK(res[kSliceBytes] == total);
    uint64_t at = 0, hits = 0, payload = 0;
    for (int64_t i = 0; i < n; ++i) {
      const SliceRow& r = rows[(size_t)i];
      const std::string& v = want[(size_t)i];
      CHECK(r.out_off == at);
      at += slice_row_bytes(r);
      payload += slice_row_payload(r);
      if (v.empty()) {
        CHECK(r.status == kSliceMiss);
        continue;
      }
      ++hits;
      SliceRow w;
      slice_value_row_if(&w, bs[(size_t)i], &bc[(size_t)i], cbuf.get(),
                         reinterpret_cast<const uint8_t*>(v.data()), (uint32_t)v.size(), 5, 0);
      w.out_off = r.out_off;
      CHECK(std::memcmp(&w, &r, sizeof(r)) == 0);
      const uint8_t* const o = out.get() + r.out_off;
      if (r.status == kSliceWholeObj) {
        ++whole;
        CHECK(std::memcmp(o, v.data(), v.size()) == 0);
        continue;
      }
      if (r.status == kSliceNotModified) {
        ++not_modified;
        CHECK(r.win_len == 0 && slice_row_bytes(r) == r.head_bytes);
      }
      CHECK(std::memcmp(o, v.data(), r.body_off) == 0);
      CHECK(std::memcmp(o + r.head_bytes + r.skew, v.data() + r.body_off + r.win_first, r.win_len) == 0);
    }
    const CacheCounters c1 = hc.counters();
    CHECK(at == total && hits == res[kSliceHits]);
    CHECK(c1.get_bytes - c0.get_bytes == 2 * payload && c1.get_hits - c0.get_hits == 2 * hits);
  }
  CHECK(not_modified > 20 && whole > 20);
  // no conditions, and conditions that are all kCondNone: the plain call's rows
  const Digest d = digest_bytes(reinterpret_cast<const uint8_t*>(keys[0].data()), keys[0].size());
  const int64_t offs[2] = {0, (int64_t)keys[0].size()};
  const SliceSpec sp{kSliceRange, 0, 1, 2};
  const SliceCond none{kCondNone, 3, 100, 100};
  SliceRow a, b;
  uint64_t res[kSliceWords];
  hc.get_keyed_slices(&d, reinterpret_cast<const uint8_t*>(keys[0].data()), offs, &sp, 1, &a, nullptr, 0,
                      res, now);
  hc.get_keyed_slices(&d, reinterpret_cast<const uint8_t*>(keys[0].data()), offs, &sp, 1, &b, nullptr, 0,
                      res, now, 0, &none, nullptr);
  CHECK(a.status == kSliceOk && std::memcmp(&a, &b, sizeof(a)) == 0);
}

int main() {
  fields();
  malformed();
  headers();
  twin();
  std::printf("cond_main: ok\n");
  return 0;
}
