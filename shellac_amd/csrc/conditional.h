// Conditional sliced GET: a client's validators decided against the stored HTTP head.
//
// A row of a sliced GET (slice.h) may carry one condition: the entity-tags of an If-None-Match,
// the date of an If-Modified-Since, or the validator of an If-Range. The engine (k_slice_plan
// on the GPU, HostCache::get_keyed_slices on the host) looks the stored ETag or Last-Modified up
// in the head it has just found and lets the comparison choose what the row returns: the head
// alone (304), the head and the window (206) or the whole object (200). This header holds what
// both engines, the tiers, the proxy, the bindings and the tests' native program share.
//
// Field lookup. The head is the payload from "HTTP/" through the blank line, value offsets
// [head_off, body_off); e = body_off - 4 is the offset of its CR LF CR LF. A header line starts
// at every p with v[p-2..p) == CR LF, head_off + 2 <= p (the status line is no header line).
// Field `name` is the line with the lowest p for which v[p..p+len(name)+1) equals name ":"
// ASCII-case-insensitively and p + len(name) + 1 <= e; later duplicates are ignored, and a name
// that does not sit at a line start never matches. Its value runs from behind the colon to the
// first CR LF at or after it, SP / HTAB trimmed at both ends; a raw stretch of more than
// kCondLineMax bytes makes the field absent. obs-fold is not unfolded.
//
// Stored validators. An ETag is usable if it is "..." or W/"..." with 2..kCondValueMax bytes
// behind the W/, the first and the last of them DQUOTE (what lies between is not inspected); a
// Last-Modified if its value has 1..kCondValueMax bytes. A value without a head has none.
//
// Comparison. none_match: the list is "*" (ncand == 0), or the stored tag without its W/ equals
// a candidate byte for byte (candidates come without their W/: RFC 9110's weak comparison).
// if_range_etag: the stored tag is strong and equals a candidate. modified_since,
// if_range_date: the stored Last-Modified value equals a candidate byte for byte.
#pragma once

#include <cstddef>
#include <cstdint>
#include <cstring>
#include <string>

#include "slice.h"

namespace shellac {

constexpr uint32_t kCondLineMax = 512;       // raw bytes of a field value, blanks included
constexpr uint32_t kCondValueMax = 255;      // bytes of a validator (a candidate's u8 length)
constexpr uint32_t kCondMaxCandidates = 16;  // entity-tags of one If-None-Match

// Condition kinds (SliceCond::kind). Any other value is answered as kCondNone.
enum : uint32_t {
  kCondNone = 0,
  kCondNoneMatch = 1,      // matched: the head alone, status kSliceNotModified
  kCondModifiedSince = 2,  // (the same)
  kCondIfRangeEtag = 3,    // unmatched: the whole value, as kSliceWhole
  kCondIfRangeDate = 4,    // (the same)
};

// One row's condition. Its candidates are ncand records [u8 len | bytes] packed in
// cond_bytes[off, off + len). ncand == 0 under kCondNoneMatch is "*", under every other kind
// it never matches. Records that overrun len, or ncand > kCondMaxCandidates: never matches.
struct SliceCond {
  uint32_t kind, ncand, off, len;
};
static_assert(sizeof(SliceCond) == 16, "SliceCond is four u32");

SH_HD bool cond_kind_valid(uint32_t kind) { return kind >= kCondNoneMatch && kind <= kCondIfRangeDate; }
// The field a kind compares: ETag (true) or Last-Modified.
SH_HD bool cond_kind_etag(uint32_t kind) { return kind == kCondNoneMatch || kind == kCondIfRangeEtag; }
// Bytes of the field's lower-case name with its colon: "etag:" or "last-modified:".
SH_HD uint32_t cond_name_len(bool etag) { return etag ? 5u : 14u; }
SH_HD uint8_t cond_name_at(bool etag, uint32_t k) {
  return (uint8_t)(etag ? "etag:"[k] : "last-modified:"[k]);
}
SH_HD uint8_t cond_lower(uint8_t c) { return c >= 'A' && c <= 'Z' ? (uint8_t)(c | 0x20) : c; }
SH_HD bool cond_blank(uint8_t c) { return c == ' ' || c == '\t'; }

// Whether the candidate records are well formed: at most kCondMaxCandidates of them, each
// inside cb[0, len). Reads only length bytes inside that range.
SH_HD bool cond_records_ok(uint32_t ncand, const uint8_t* cb, uint32_t len) {
  if (ncand > kCondMaxCandidates) return false;
  uint32_t p = 0;
  for (uint32_t k = 0; k < ncand; ++k) {
    if (p >= len) return false;
    p += 1u + cb[p];
    if (p > len) return false;
  }
  return true;
}

// A stored field value val[0..n) (trimmed) as a validator. True: usable, and val[*o, *o + *m)
// are the bytes a candidate is compared with (an ETag's without its W/); *weak: it had one.
SH_HD bool cond_stored_validator(bool etag, const uint8_t* val, uint32_t n, bool* weak,
                                 uint32_t* o, uint32_t* m) {
  *weak = false;
  *o = 0;
  *m = n;
  if (!etag) return n >= 1 && n <= kCondValueMax;
  if (n >= 2 && val[0] == 'W' && val[1] == '/') {
    *weak = true;
    *o = 2;
    *m = n - 2;
  }
  return *m >= 2 && *m <= kCondValueMax && val[*o] == '"' && val[*o + *m - 1] == '"';
}

// What a condition does to a sliceable row: it may replace the window kind, and returns
// whether the row's status becomes kSliceNotModified. (A value that is not sliceable comes
// back whole whatever the condition.)
SH_HD bool cond_outcome(uint32_t ckind, bool matched, uint32_t* spec_kind) {
  if (ckind == kCondNoneMatch || ckind == kCondModifiedSince) {
    if (matched) {
      *spec_kind = kSliceHead;
      return true;
    }
  } else if (ckind == kCondIfRangeEtag || ckind == kCondIfRangeDate) {
    if (!matched) *spec_kind = kSliceWhole;
  }
  return false;
}

// slice_make_row under a condition of kind ckind whose comparison gave `matched`.
SH_HD void slice_make_row_if(SliceRow* r, uint32_t kind, uint64_t a, uint64_t b, uint32_t vlen,
                             uint32_t flags, uint32_t expire, bool sliceable, uint32_t head_off,
                             uint32_t body_off, uint32_t ckind, bool matched) {
  const bool not_modified = sliceable && cond_outcome(ckind, matched, &kind);
  slice_make_row(r, kind, a, b, vlen, flags, expire, sliceable, head_off, body_off);
  if (not_modified) r->status = kSliceNotModified;
}

// ---- host side --------------------------------------------------------------------------------
// The trimmed value v[*vs, *vs + *vn) of the first `etag` / `last-modified` line of the head
// v[head_off, body_off) of a sliceable value. False: the field is absent.
inline bool cond_find_field(const uint8_t* v, uint32_t head_off, uint32_t body_off, bool etag,
                            uint32_t* vs, uint32_t* vn) {
  const uint32_t nl = cond_name_len(etag), e = body_off - 4;
  for (uint32_t p = head_off + 2; p + nl <= e; ++p) {
    if (v[p - 2] != '\r' || v[p - 1] != '\n') continue;
    uint32_t k = 0;
    while (k < nl && cond_lower(v[p + k]) == cond_name_at(etag, k)) ++k;
    if (k < nl) continue;
    const uint32_t c = p + nl;
    uint32_t q = c;  // (v[e], v[e + 1] are CR LF)
    while (q < e && !(v[q] == '\r' && v[q + 1] == '\n')) ++q;
    if (q - c > kCondLineMax) return false;
    uint32_t s = c, t = q;
    while (s < t && cond_blank(v[s])) ++s;
    while (t > s && cond_blank(v[t - 1])) --t;
    *vs = s;
    *vn = t - s;
    return true;
  }
  return false;
}

// Whether condition c holds for the sliceable value v with the head [head_off, body_off).
inline bool cond_matches(const uint8_t* v, uint32_t head_off, uint32_t body_off,
                         const SliceCond& c, const uint8_t* cond_bytes) {
  if (!cond_kind_valid(c.kind) || (c.ncand && !cond_bytes)) return false;
  const uint8_t* const cb = cond_bytes ? cond_bytes + c.off : nullptr;
  if (!cond_records_ok(c.ncand, cb, c.len)) return false;
  if (c.ncand == 0) return c.kind == kCondNoneMatch;  // "*"
  const bool etag = cond_kind_etag(c.kind);
  uint32_t vs, vn, o, m;
  bool weak;
  if (!cond_find_field(v, head_off, body_off, etag, &vs, &vn)) return false;
  if (!cond_stored_validator(etag, v + vs, vn, &weak, &o, &m)) return false;
  if (weak && c.kind == kCondIfRangeEtag) return false;
  uint32_t p = 0;
  for (uint32_t k = 0; k < c.ncand; ++k) {
    const uint32_t cl = cb[p];
    if (cl == m && std::memcmp(cb + p + 1, v + vs + o, m) == 0) return true;
    p += 1 + cl;
  }
  return false;
}

// slice_value_row under a condition (nullable: none).
inline void slice_value_row_if(SliceRow* r, const SliceSpec& sp, const SliceCond* c,
                               const uint8_t* cond_bytes, const uint8_t* v, uint32_t vlen,
                               uint32_t flags, uint32_t expire) {
  if (!c || c->kind == kCondNone) return slice_value_row(r, sp, v, vlen, flags, expire);
  uint32_t ho = 0, bo = 0;
  const bool ok = slice_layout(v, vlen, &ho, &bo);
  const bool matched = ok && cond_matches(v, ho, bo, *c, cond_bytes);
  slice_make_row_if(r, sp.kind, sp.a, sp.b, vlen, flags, expire, ok, ho, bo, c->kind, matched);
}

// ---- request headers ----------------------------------------------------------------------------
// One request's condition: the kind and its candidate records, as a SliceCond's bytes.
struct CondRequest {
  uint32_t kind = kCondNone;
  uint32_t ncand = 0;
  std::string records;  // [u8 len | bytes] per candidate
  void add(const char* p, size_t n) {
    records.push_back((char)(uint8_t)n);
    records.append(p, n);
    ++ncand;
  }
};

namespace cond_detail {
inline void trim(const char*& v, size_t& n) {
  while (n && cond_blank((uint8_t)v[0])) ++v, --n;
  while (n && cond_blank((uint8_t)v[n - 1])) --n;
}
// Bytes of the opaque-tag "..." at v[0..n) (etagc between the quotes), 0: none.
inline size_t opaque_tag(const char* v, size_t n) {
  if (n < 2 || v[0] != '"') return 0;
  for (size_t k = 1; k < n; ++k) {
    const uint8_t c = (uint8_t)v[k];
    if (c == '"') return k + 1;
    if (c < 0x21 || c == 0x7f) return 0;
  }
  return 0;
}
}  // namespace cond_detail

// The value v[0..n) of an If-None-Match field: "*", or a comma-separated list of entity-tags
// with optional blanks around them (empty elements are skipped; commas inside quotes belong to
// the tag). Candidates lose their W/. False: the header is to be ignored and the request
// answered as without it (a malformed list, no tag, more than kCondMaxCandidates tags, or a
// tag over kCondValueMax bytes with its quotes).
inline bool parse_if_none_match(const char* v, size_t n, CondRequest* out) {
  *out = CondRequest{};
  cond_detail::trim(v, n);
  out->kind = kCondNoneMatch;
  if (n == 1 && v[0] == '*') return true;
  while (n) {
    if (cond_blank((uint8_t)v[0]) || v[0] == ',') {
      ++v, --n;
      continue;
    }
    if (n >= 2 && v[0] == 'W' && v[1] == '/') v += 2, n -= 2;
    const size_t t = cond_detail::opaque_tag(v, n);
    if (!t || t > kCondValueMax || out->ncand == kCondMaxCandidates) return false;
    out->add(v, t);
    v += t, n -= t;
    while (n && cond_blank((uint8_t)v[0])) ++v, --n;
    if (n && v[0] != ',') return false;
  }
  return out->ncand > 0;
}

// The value v[0..n) of an If-Range field. A strong entity-tag gives kCondIfRangeEtag, anything
// that does not start with a DQUOTE or W/ is a date and gives kCondIfRangeDate (compared as
// bytes). False: the validator can never match (a weak or malformed tag, an empty or
// over-long value): no condition is sent and the whole object is asked for.
inline bool parse_if_range(const char* v, size_t n, CondRequest* out) {
  *out = CondRequest{};
  cond_detail::trim(v, n);
  if (n == 0 || n > kCondValueMax) return false;
  if (v[0] == '"') {
    if (cond_detail::opaque_tag(v, n) != n) return false;
    out->kind = kCondIfRangeEtag;
  } else if (n >= 2 && v[0] == 'W' && v[1] == '/') {
    return false;
  } else {
    out->kind = kCondIfRangeDate;
  }
  out->add(v, n);
  return true;
}

// The value v[0..n) of an If-Modified-Since field: the trimmed bytes, compared as bytes.
// False: empty or over-long, the header is ignored.
inline bool parse_if_modified_since(const char* v, size_t n, CondRequest* out) {
  *out = CondRequest{};
  cond_detail::trim(v, n);
  if (n == 0 || n > kCondValueMax) return false;
  out->kind = kCondModifiedSince;
  out->add(v, n);
  return true;
}

}  // namespace shellac
