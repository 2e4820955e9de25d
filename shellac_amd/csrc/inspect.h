// Cache inspection: what a listing asks of a cache tier and what it answers
// (CacheBackend::list_objects), and the host-only helpers of its HTTP surface
// (GET /_shellac/objects, proxy.cc): the query string, percent-decoding, JSON escaping of key
// bytes, and the HBM tier's (shard, slot) cursor. No I/O and no HIP here:
// tests/native/list_main.cc runs all of it under sanitizers.
#pragma once

#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "keyed.h"
#include "selector.h"

namespace shellac {

struct ListQuery {
  KeyedSelector what;     // which objects (selector.h); the default: all of them
  uint32_t limit = 100;   // objects wanted, <= kMaxListRows; 0: count only
  std::string after;      // the `next` of the page before; empty: from the start
};
inline bool list_query_valid(const ListQuery& q) {
  return q.what.valid() && q.limit <= kMaxListRows;
}

struct ListedObject {
  std::string key;
  bool key_truncated = false;
  uint32_t size = 0;      // stored value bytes (key image and payload)
  int64_t ttl = -1;       // seconds left; -1: never expires
  uint32_t flags = 0;     // the object's flags word (the proxy's freshness time)
  int ntags = 0;          // -1: the overflow block
  bool referenced = false;
  int shard = 0;
};

struct ListResult {
  bool ok = false;          // false: the tier cannot scan its keys, or refused the query
  bool bad_cursor = false;  // `after` is not a cursor of this tier
  uint64_t matched = 0, bytes = 0;  // per stored copy, as a purge's count
  std::vector<ListedObject> objects;
  std::string next;         // empty: nothing follows
  uint32_t shards_skipped = 0;
};

// ---- the HTTP surface ---------------------------------------------------------------------
// Percent-decodes once ("%2F" -> "/", "%252F" -> "%2F"; '+' stays '+'). False on a '%' that
// two hex digits do not follow.
inline bool percent_decode(const std::string& in, std::string* out) {
  out->clear();
  const auto hex = [](char c) -> int {
    if (c >= '0' && c <= '9') return c - '0';
    if (c >= 'a' && c <= 'f') return c - 'a' + 10;
    if (c >= 'A' && c <= 'F') return c - 'A' + 10;
    return -1;
  };
  for (size_t i = 0; i < in.size(); ++i) {
    if (in[i] != '%') {
      out->push_back(in[i]);
      continue;
    }
    if (i + 2 >= in.size()) return false;  // (two digits must follow)
    const int a = hex(in[i + 1]), b = hex(in[i + 2]);
    if (a < 0 || b < 0) return false;
    out->push_back((char)(a * 16 + b));
    i += 2;
  }
  return true;
}

// The inverse, for a cursor that goes back into a query string as it is: every byte but
// letters, digits and "-._~/" as %XX.
inline void percent_encode(const std::string& in, std::string* out) {
  static const char* const kHex = "0123456789ABCDEF";
  for (unsigned char c : in) {
    const bool plain = (c >= '0' && c <= '9') || (c >= 'a' && c <= 'z') || (c >= 'A' && c <= 'Z') ||
                       c == '-' || c == '.' || c == '_' || c == '~' || c == '/';
    if (plain) {
      out->push_back((char)c);
    } else {
      out->push_back('%');
      out->push_back(kHex[c >> 4]);
      out->push_back(kHex[c & 15]);
    }
  }
}

// The parameters of GET /_shellac/objects?prefix=..|key=..|tag=a,b|glob=..[&limit=N]
// [&after=CURSOR], values percent-decoded once. `which`: 0 none (all), 1 prefix, 2 key, 3 tag,
// 4 glob.
struct InspectParams {
  int which = 0;
  std::string value;   // the prefix, the key, the tag list or the glob as written
  uint32_t limit = 100;
  std::string after;
};

// `qs`: what follows the '?' (may be empty). False: an unknown or repeated parameter, two
// selectors, a bad escape, or a limit that is not a number in 0..kMaxListRows.
inline bool parse_inspect_query(const std::string& qs, InspectParams* p) {
  *p = InspectParams();
  bool have_limit = false, have_after = false;
  size_t pos = 0;
  while (pos < qs.size()) {
    size_t e = qs.find('&', pos);
    if (e == std::string::npos) e = qs.size();
    if (e > pos) {
      const std::string item = qs.substr(pos, e - pos);
      const size_t eq = item.find('=');
      const std::string name = item.substr(0, eq);
      std::string val;
      if (!percent_decode(eq == std::string::npos ? "" : item.substr(eq + 1), &val)) return false;
      const int sel = name == "prefix" ? 1 : name == "key" ? 2 : name == "tag" ? 3
                      : name == "glob" ? 4 : 0;
      if (sel) {
        if (p->which) return false;
        p->which = sel;
        p->value = val;
      } else if (name == "limit") {
        if (have_limit || val.empty() || val.size() > 6) return false;
        uint32_t n = 0;
        for (char c : val) {
          if (c < '0' || c > '9') return false;
          n = n * 10 + (uint32_t)(c - '0');
        }
        if (n > kMaxListRows) return false;
        p->limit = n;
        have_limit = true;
      } else if (name == "after") {
        if (have_after) return false;
        p->after = val;
        have_after = true;
      } else {
        return false;
      }
    }
    pos = e + 1;
  }
  return true;
}

// Key bytes as a JSON string's contents: control bytes, '"', '\\', DEL and every byte >= 0x80 as
// \u00XX (a Vary variant's '\x1f' shows as \u001f); the rest as they are.
inline void json_escape_key(const std::string& key, std::string* out) {
  static const char* const kHex = "0123456789abcdef";
  for (unsigned char c : key) {
    if (c < 0x20 || c == '"' || c == '\\' || c >= 0x7f) {
      out->append("\\u00");
      out->push_back(kHex[c >> 4]);
      out->push_back(kHex[c & 15]);
    } else {
      out->push_back((char)c);
    }
  }
}

// ---- the HBM tier's cursor: "<shard>.<slot>" ------------------------------------------------
inline std::string hbm_cursor(int shard, uint64_t slot) {
  return std::to_string(shard) + "." + std::to_string(slot);
}
inline bool hbm_cursor_parse(const std::string& s, int nshards, int* shard, uint64_t* slot) {
  const size_t dot = s.find('.');
  if (dot == std::string::npos || dot == 0 || dot + 1 >= s.size() || s.size() > 32) return false;
  uint64_t a = 0, b = 0;
  for (size_t i = 0; i < s.size(); ++i) {
    if (i == dot) continue;
    if (s[i] < '0' || s[i] > '9') return false;
    uint64_t& x = i < dot ? a : b;
    const uint64_t digit = (uint64_t)(s[i] - '0');
    if (x > (~0ull - digit) / 10) return false;  // (past 2^64 - 1)
    x = x * 10 + digit;
  }
  if (a > (uint64_t)nshards) return false;  // (== nshards: past the last shard, an empty page)
  *shard = (int)a;
  *slot = b;
  return true;
}

}  // namespace shellac
