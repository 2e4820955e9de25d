// Sliced GET: the head and one byte window of a stored HTTP response.
//
// A row of a sliced GET asks for part of one keyed value (keyed.h): the value's stored prefix
// through the end of its HTTP head, plus one window of its body. The engine (k_slice_plan on
// the GPU, HostCache::get_keyed_slices on the host) finds the head's end and cuts the window;
// the rest of the object is never moved. This header holds what both engines, the bindings
// and the tests' native program share: the window kinds, the result row and the pure
// functions that decide them.
//
// A stored value is [u16 klen | key | optional tag block | payload]. The payload is
// *sliceable* if it starts with "HTTP/", the byte sequence CR LF CR LF first occurs at
// payload offset e, and e + 4 <= kSliceHeadMax (the HTTP codec's header limit). Then
//   head_off = 2 + klen + tag block bytes (parse_tag_block's rules)
//   body_off = head_off + e + 4
//   body_len = vlen - body_off
#pragma once

#include <cstddef>
#include <cstdint>
#include <cstring>

#include "keyed.h"
#include "layout.h"

namespace shellac {

constexpr uint32_t kSliceHeadMax = 64u << 10;

// Window kinds (SliceSpec::kind). Any other value is answered as kSliceWhole.
enum : uint32_t {
  kSliceHead = 0,    // the head only, no body bytes
  kSliceRange = 1,   // body bytes a..b inclusive, b clamped to body_len - 1
  kSliceFrom = 2,    // body bytes a..end
  kSliceSuffix = 3,  // the last a bytes (a > body_len: the whole body)
  kSliceWhole = 4,   // the whole value, as a plain GET
};

struct SliceSpec {
  uint32_t kind;
  uint32_t pad;
  uint64_t a, b;
};
static_assert(sizeof(SliceSpec) == 24, "SliceSpec is {u32 kind, u64 a, u64 b}");

// Row status.
enum : uint32_t {
  kSliceMiss = 0,
  kSliceOk = 1,
  kSliceUnsat = 2,     // the head is returned, the window is empty
  kSliceWholeObj = 3,  // kSliceWhole, or the value is not sliceable: the whole value is returned
  kSliceNotModified = 4,  // the row's condition holds (conditional.h): the head, an empty window
};

// One result row. Its bytes in `out`: segment 0 at out_off, the value's first head_bytes
// bytes; segment 1 at out_off + head_bytes, the 16-byte granules of the value that cover the
// window (slice_window_bytes()), the window's first byte at + skew. A miss occupies nothing.
// For kSliceMiss every other field but out_off is 0; for kSliceWholeObj the head and window
// fields are 0; a kSliceNotModified row is a kSliceOk row of kind kSliceHead (win_len = 0).
struct alignas(16) SliceRow {
  uint32_t status;
  uint32_t vlen;    // stored value bytes (the keyed image)
  uint32_t flags;   // ItemHeader::flags
  uint32_t expire;  // absolute expiry, 0 = never
  uint32_t head_off, body_off, body_len;
  uint32_t skew;    // (body_off + win_first) & 15
  uint32_t win_first, win_len;
  uint32_t head_bytes;  // align_up(body_off, 16), or align_up(vlen, 16) for a whole value
  uint32_t pad0;
  uint64_t out_off;  // exclusive scan of the rows' byte counts, in row order
  uint64_t pad1;
};
static_assert(sizeof(SliceRow) == 64, "SliceRow is four 16-byte granules");

// Result words of a sliced GET.
enum : int { kSliceHits = 0, kSliceBytes = 1, kSliceWords = 2 };

// The window of a body of body_len bytes. False: unsatisfiable (*first = *len = 0).
SH_HD bool resolve_window(uint32_t kind, uint64_t a, uint64_t b, uint64_t body_len,
                          uint64_t* first, uint64_t* len) {
  *first = 0;
  *len = 0;
  if (kind == kSliceHead) return true;
  if (body_len == 0) return false;
  if (kind == kSliceRange) {
    if (a >= body_len || a > b) return false;
    if (b >= body_len) b = body_len - 1;
    *first = a;
    *len = b - a + 1;
    return true;
  }
  if (kind == kSliceFrom) {
    if (a >= body_len) return false;
    *first = a;
    *len = body_len - a;
    return true;
  }
  if (kind == kSliceSuffix) {
    if (a == 0) return false;
    if (a > body_len) a = body_len;
    *first = body_len - a;
    *len = a;
    return true;
  }
  return false;
}

// Bytes of a row's segment 1 (an empty window has none).
SH_HD uint32_t slice_window_bytes(uint32_t skew, uint32_t win_len) {
  return win_len ? (uint32_t)align_up((uint64_t)skew + win_len, 16) : 0u;
}
SH_HD uint64_t slice_row_bytes(const SliceRow& r) {
  return r.status == kSliceMiss ? 0 : (uint64_t)r.head_bytes + slice_window_bytes(r.skew, r.win_len);
}
// The bytes a row returns to its caller (what get_bytes counts): the value through the end of
// its head and the window, or the whole value.
SH_HD uint64_t slice_row_payload(const SliceRow& r) {
  return r.status == kSliceMiss       ? 0
         : r.status == kSliceWholeObj ? (uint64_t)r.vlen
                                      : (uint64_t)r.body_off + r.win_len;
}

// The row of a hit (everything but out_off). `sliceable`: head_off / body_off are the
// value's; otherwise, and for kSliceWhole, the whole value is the answer.
SH_HD void slice_make_row(SliceRow* r, uint32_t kind, uint64_t a, uint64_t b, uint32_t vlen,
                          uint32_t flags, uint32_t expire, bool sliceable, uint32_t head_off,
                          uint32_t body_off) {
  *r = SliceRow{};
  r->vlen = vlen;
  r->flags = flags;
  r->expire = expire;
  if (!sliceable || kind >= kSliceWhole) {
    r->status = kSliceWholeObj;
    r->head_bytes = (uint32_t)align_up(vlen, 16);
    return;
  }
  uint64_t first, len;
  const bool ok = resolve_window(kind, a, b, vlen - body_off, &first, &len);
  r->status = ok ? kSliceOk : kSliceUnsat;
  r->head_off = head_off;
  r->body_off = body_off;
  r->body_len = vlen - body_off;
  r->win_first = (uint32_t)first;
  r->win_len = (uint32_t)len;
  r->skew = (body_off + (uint32_t)first) & 15u;
  r->head_bytes = (uint32_t)align_up(body_off, 16);
}

// ---- host side --------------------------------------------------------------------------------
// Whether payload[0..n) is sliceable; *head_len = e + 4, the bytes of its head through the
// blank line.
inline bool slice_find_head_end(const uint8_t* payload, size_t n, size_t* head_len) {
  if (n < 5 || std::memcmp(payload, "HTTP/", 5) != 0) return false;
  const size_t lim = n < kSliceHeadMax ? n : (size_t)kSliceHeadMax;
  for (size_t e = 0; e + 4 <= lim; ++e)
    if (payload[e] == '\r' && payload[e + 1] == '\n' && payload[e + 2] == '\r' &&
        payload[e + 3] == '\n') {
      *head_len = e + 4;
      return true;
    }
  return false;
}

// head_off and body_off of a keyed value v[0..vlen). False: not a sliceable keyed value.
inline bool slice_layout(const uint8_t* v, size_t vlen, uint32_t* head_off, uint32_t* body_off) {
  if (vlen < kKeyedPrefix) return false;
  uint16_t kl;
  std::memcpy(&kl, v, kKeyedPrefix);
  const size_t o = kKeyedPrefix + kl;
  if (o > vlen) return false;
  const uint64_t* hs;
  unsigned nt;
  bool over;
  const size_t h =
      o + parse_tag_block(reinterpret_cast<const char*>(v) + o, vlen - o, &hs, &nt, &over);
  size_t head_len;
  if (!slice_find_head_end(v + h, vlen - h, &head_len)) return false;
  *head_off = (uint32_t)h;
  *body_off = (uint32_t)(h + head_len);
  return true;
}

// The row of a hit on the keyed value v[0..vlen) (everything but out_off).
inline void slice_value_row(SliceRow* r, const SliceSpec& sp, const uint8_t* v, uint32_t vlen,
                            uint32_t flags, uint32_t expire) {
  uint32_t ho = 0, bo = 0;
  const bool ok = sp.kind < kSliceWhole && slice_layout(v, vlen, &ho, &bo);
  slice_make_row(r, sp.kind, sp.a, sp.b, vlen, flags, expire, ok, ho, bo);
}

// ---- Range header -------------------------------------------------------------------------------
// The value v[0..n) of a Range header field as one window spec: "bytes=a-b" (kSliceRange),
// "bytes=a-" (kSliceFrom) or "bytes=-n" (kSliceSuffix), the unit in any letter case, optional
// blanks around the spec. False: the header is to be ignored and the request answered in full
// (RFC 9110 14.2): another unit, more than one range, or no syntactically valid byte range
// (a > b included). Positions past 2^64 - 1 saturate (they lie past every body).
inline bool parse_single_range(const char* v, size_t n, SliceSpec* sp) {
  const auto blank = [](char c) { return c == ' ' || c == '\t'; };
  while (n && blank(v[0])) ++v, --n;
  while (n && blank(v[n - 1])) --n;
  if (n < 6 || v[5] != '=') return false;
  for (int i = 0; i < 5; ++i)
    if ((v[i] | 0x20) != "bytes"[i]) return false;
  v += 6, n -= 6;
  while (n && blank(v[0])) ++v, --n;
  const auto number = [&](uint64_t* x) {  // 1*DIGIT
    size_t d = 0;
    *x = 0;
    for (; d < n && v[d] >= '0' && v[d] <= '9'; ++d) {
      const uint64_t c = (uint64_t)(v[d] - '0');
      *x = *x > (~0ull - c) / 10 ? ~0ull : *x * 10 + c;
    }
    v += d, n -= d;
    return d > 0;
  };
  uint64_t a = 0, b = 0;
  const bool has_a = number(&a);
  if (!n || v[0] != '-') return false;
  ++v, --n;
  const bool has_b = number(&b);
  if (n || (!has_a && !has_b)) return false;  // trailing bytes (a second range), or "-"
  if (has_a && has_b && a > b) return false;
  *sp = SliceSpec{};
  if (!has_a) {
    sp->kind = kSliceSuffix;
    sp->a = b;
  } else {
    sp->kind = has_b ? kSliceRange : kSliceFrom;
    sp->a = a;
    sp->b = has_b ? b : 0;
  }
  return true;
}

}  // namespace shellac
