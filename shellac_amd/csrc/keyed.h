// Full-key object identity for the digest-indexed tiers.
//
// The reference keys memcached objects by the full URL (src/python/shellac/server/
// Server.py:327, :335, :432) and memcached compares whole keys. The HBM and DRAM shards
// index by a 128-bit digest (digest.h), so the backends that front them store each value
// as [u16 key length | key bytes | payload] and accept a hit only if the stored key is
// byte-equal to the requested one: two keys whose digests collide (by accident or by a
// crafted URL) read as a miss, never as each other's object.
#pragma once

#include <cstdint>
#include <cstring>
#include <string>

#include "digest.h"

namespace shellac {

constexpr size_t kKeyedPrefix = 2;
constexpr size_t kMaxKeyedKey = 0xffff;

inline size_t keyed_size(size_t klen, size_t plen) { return kKeyedPrefix + klen + plen; }

inline void write_keyed(uint8_t* dst, const std::string& key, const char* payload, size_t plen) {
  const uint16_t kl = (uint16_t)key.size();
  std::memcpy(dst, &kl, kKeyedPrefix);
  std::memcpy(dst + kKeyedPrefix, key.data(), key.size());
  if (plen) std::memcpy(dst + kKeyedPrefix + key.size(), payload, plen);
}

// True if the stored value v[0..n) belongs to `key`; *payload_off = start of the payload.
inline bool keyed_match(const char* v, size_t n, const std::string& key, size_t* payload_off) {
  if (n < kKeyedPrefix) return false;
  uint16_t kl;
  std::memcpy(&kl, v, kKeyedPrefix);
  if (kl != key.size() || n < kKeyedPrefix + kl) return false;
  if (kl && std::memcmp(v + kKeyedPrefix, key.data(), kl) != 0) return false;
  *payload_off = kKeyedPrefix + kl;
  return true;
}

// ---- prefix purge (HbmCache / HostCache::remove_keyed_prefix) -------------------------------
// A keyed value starts 16-byte aligned in the log and its key starts at value byte 2, so
// the prefix scan compares 16-byte granules of the value against a pattern *image*: the
// prefix shifted by those 2 bytes, with byte masks for the first granule (the key length
// word is not compared) and the last one (bytes past the prefix are not compared).
//   image = [mask of granule 0 | mask of the last granule | G granules of masked pattern]
//   G = ceil((2 + plen) / 16); with G == 1 both masks hold the one combined mask.
constexpr size_t kPurgeGranule = 16;

inline size_t keyed_prefix_granules(size_t plen) {
  return (kKeyedPrefix + plen + kPurgeGranule - 1) / kPurgeGranule;
}
inline size_t keyed_prefix_image_bytes(size_t plen) {
  return (2 + keyed_prefix_granules(plen)) * kPurgeGranule;
}
inline void write_keyed_prefix_image(uint8_t* dst, const uint8_t* prefix, size_t plen) {
  const size_t g = keyed_prefix_granules(plen), end = kKeyedPrefix + plen;
  std::memset(dst, 0, keyed_prefix_image_bytes(plen));
  uint8_t* const m0 = dst;
  uint8_t* const ml = dst + kPurgeGranule;
  uint8_t* const pat = dst + 2 * kPurgeGranule;
  for (size_t b = kKeyedPrefix; b < kPurgeGranule && b < end; ++b) m0[b] = 0xff;
  for (size_t b = 0; b < kPurgeGranule; ++b) {
    const size_t at = (g - 1) * kPurgeGranule + b;
    if (at >= kKeyedPrefix && at < end) ml[b] = 0xff;
  }
  std::memcpy(pat + kKeyedPrefix, prefix, plen);
}

// ---- tag block (purge by surrogate key) ------------------------------------------------------
// A tagged payload starts with a tag block, so that a scan finds an object's tags without
// parsing HTTP:
//   [0x02 | u8 ntags | ntags x u64 little-endian tag hash] [the payload as without tags]
// The proxy's untagged payloads start with "HTTP/" or the Vary marker's 0x01, never 0x02.
// Tag hash = digest_bytes(tag).lo; a colliding hash purges one object too many (a miss, never
// a wrong answer). ntags == kTagOverflow: no hashes follow and the object matches every tag
// purge (the response named more than kMaxObjectTags distinct tags; dropping some silently
// would leave stale objects). ntags in 33..254 is malformed, a block whose hashes do not fit
// is truncated: both match nothing and are not stripped. No padding: inside a keyed value
// the block sits at byte 2 + klen, so the hashes have any byte alignment.
constexpr uint8_t kTagMarker = 0x02;
constexpr unsigned kMaxObjectTags = 32;
constexpr unsigned kTagOverflow = 0xff;
constexpr unsigned kMaxPurgeTags = 64;  // hashes in one purge's list

inline uint64_t tag_hash(const char* tag, size_t n) {
  return digest_bytes(reinterpret_cast<const uint8_t*>(tag), n).lo;
}
inline uint64_t tag_hash(const std::string& tag) { return tag_hash(tag.data(), tag.size()); }

// Bytes of the block for `ntags` distinct tags (more than kMaxObjectTags: the overflow block).
inline size_t tag_block_size(size_t ntags) { return 2 + (ntags > kMaxObjectTags ? 0 : 8 * ntags); }

// Writes the block for hashes[0..ntags) (distinct) at dst; returns tag_block_size(ntags).
inline size_t write_tag_block(uint8_t* dst, const uint64_t* hashes, size_t ntags) {
  dst[0] = kTagMarker;
  if (ntags > kMaxObjectTags) {
    dst[1] = (uint8_t)kTagOverflow;
    return 2;
  }
  dst[1] = (uint8_t)ntags;
  for (size_t i = 0; i < ntags; ++i) {
    uint64_t h = hashes[i];
    for (int b = 0; b < 8; ++b, h >>= 8) dst[2 + 8 * i + b] = (uint8_t)h;
  }
  return 2 + 8 * ntags;
}

// Hash i of a parsed block: `hashes` has no alignment, so it is never dereferenced.
inline uint64_t tag_block_hash(const uint64_t* hashes, unsigned i) {
  const uint8_t* const p = reinterpret_cast<const uint8_t*>(hashes) + 8 * (size_t)i;
  uint64_t h = 0;
  for (int b = 7; b >= 0; --b) h = (h << 8) | p[b];
  return h;
}

// Parses the tag block at the start of payload[0..n). Returns the bytes to strip to reach
// the plain payload; 0: untagged (no marker, or a malformed or truncated block, which matches
// nothing). *hashes points at the *ntags stored hashes (unaligned: read them with
// tag_block_hash); *overflow: the object matches every tag purge (*ntags is 0 then).
inline size_t parse_tag_block(const char* payload, size_t n, const uint64_t** hashes,
                              unsigned* ntags, bool* overflow) {
  *hashes = nullptr;
  *ntags = 0;
  *overflow = false;
  if (n < 2 || (uint8_t)payload[0] != kTagMarker) return 0;
  const unsigned nt = (uint8_t)payload[1];
  if (nt == kTagOverflow) {
    *overflow = true;
    return 2;
  }
  if (nt > kMaxObjectTags || 2 + 8 * (size_t)nt > n) return 0;
  *hashes = reinterpret_cast<const uint64_t*>(payload + 2);
  *ntags = nt;
  return 2 + 8 * (size_t)nt;
}

// Whether the payload's tag block matches a purge of list[0..nlist).
inline bool tag_block_matches(const char* payload, size_t n, const uint64_t* list, size_t nlist) {
  const uint64_t* hs;
  unsigned nt;
  bool over;
  if (!parse_tag_block(payload, n, &hs, &nt, &over)) return false;
  if (over) return true;
  for (unsigned i = 0; i < nt; ++i) {
    const uint64_t h = tag_block_hash(hs, i);
    for (size_t j = 0; j < nlist; ++j)
      if (list[j] == h) return true;
  }
  return false;
}

// The same for a whole keyed value [u16 klen | key | payload].
inline bool keyed_tags_match(const uint8_t* v, size_t vlen, const uint64_t* list, size_t nlist) {
  if (vlen < kKeyedPrefix + 2) return false;
  uint16_t kl;
  std::memcpy(&kl, v, kKeyedPrefix);
  const size_t o = kKeyedPrefix + kl;
  if (o + 2 > vlen) return false;
  return tag_block_matches(reinterpret_cast<const char*>(v) + o, vlen - o, list, nlist);
}

// ---- glob (purge, soft purge and listing by URL wildcard) ------------------------------------
// A pattern is a byte string: '*' matches any run of bytes (the empty run and '/' included),
// '\' makes the next byte literal, every other byte is literal; no '?', no classes. The match
// is anchored at both ends of the *subject*: the stored key up to, not including, its first
// kVarySep byte (the separator vary_key puts before a variant suffix), or the whole key. A
// Vary marker and its variants so match together, by their base key. An empty key never
// matches. The pattern splits at its unescaped stars into a head segment (anchored at the
// start), a tail segment (anchored at the end) and middle segments, each found leftmost, in
// order, between the two; with no star the subject equals the pattern.
// Refused: an empty pattern, stars only (that is flush()), a dangling '\', more than
// kMaxGlobStars stars, more than kMaxGlobLiteral literal bytes.
constexpr unsigned kMaxGlobStars = 8;
constexpr unsigned kMaxGlobLiteral = 1024;  // the 1 KiB of LDS the prefix image gets
constexpr uint8_t kVarySep = 0x1f;

// The compiled pattern, as the device reads it: eight 16-byte granules of header, then the
// literal bytes [head | middle segments in order | tail]. Empty middle segments (adjacent
// stars) are dropped. m0 / p0 are granule 0 of write_keyed_prefix_image for the head's first
// min(head_len, 14) bytes (all zero for an empty head: every record passes).
struct alignas(16) KeyedGlob {
  uint32_t nmid, head_len, tail_len, min_len;  // min_len: the sum of the segment lengths
  uint32_t stars, lit_bytes, tail_off, pad0;   // stars == 0: the subject equals the head
  uint8_t m0[kPurgeGranule], p0[kPurgeGranule];
  uint32_t mid[kMaxGlobStars][2];              // (offset into lit, length), nmid < kMaxGlobStars
  uint8_t lit[kMaxGlobLiteral];
};
constexpr size_t kGlobHeaderBytes = 8 * kPurgeGranule;
static_assert(sizeof(KeyedGlob) == kGlobHeaderBytes + kMaxGlobLiteral, "glob image layout");

inline size_t keyed_glob_image_bytes() { return sizeof(KeyedGlob); }
// The bytes a scan has to read: the header and the literal bytes' granules.
inline uint32_t keyed_glob_used_bytes(const KeyedGlob& g) {
  return (uint32_t)(kGlobHeaderBytes + (g.lit_bytes + kPurgeGranule - 1) / kPurgeGranule *
                                           kPurgeGranule);
}

inline bool compile_keyed_glob(const uint8_t* pat, size_t n, KeyedGlob* out, std::string* error) {
  const auto fail = [&](const char* why) {
    if (error) *error = why;
    return false;
  };
  std::memset(out, 0, sizeof(*out));
  if (n == 0) return fail("glob: empty pattern");
  // segment s = lit[seg_off[s], seg_off[s + 1]); a star closes a segment
  uint32_t seg_off[kMaxGlobStars + 2] = {0};
  uint32_t nlit = 0, stars = 0;
  for (size_t i = 0; i < n; ++i) {
    uint8_t c = pat[i];
    if (c == '*') {
      if (++stars > kMaxGlobStars) return fail("glob: more than 8 stars");
      seg_off[stars] = nlit;
      continue;
    }
    if (c == '\\') {
      if (++i == n) return fail("glob: dangling backslash");
      c = pat[i];
    }
    if (nlit == kMaxGlobLiteral) return fail("glob: more than 1024 literal bytes");
    out->lit[nlit++] = c;
  }
  if (nlit == 0) return fail("glob: stars only (that is a flush)");
  seg_off[stars + 1] = nlit;
  out->stars = stars;
  out->lit_bytes = nlit;
  out->min_len = nlit;
  out->head_len = seg_off[1];
  if (stars) {
    out->tail_off = seg_off[stars];
    out->tail_len = nlit - seg_off[stars];
    for (uint32_t s = 1; s < stars; ++s) {
      const uint32_t len = seg_off[s + 1] - seg_off[s];
      if (!len) continue;
      out->mid[out->nmid][0] = seg_off[s];
      out->mid[out->nmid][1] = len;
      ++out->nmid;
    }
  }
  if (out->head_len) {
    const size_t h = out->head_len < kPurgeGranule - kKeyedPrefix ? out->head_len
                                                                  : kPurgeGranule - kKeyedPrefix;
    uint8_t img[3 * kPurgeGranule];  // (one granule: mask, mask, pattern)
    write_keyed_prefix_image(img, out->lit, h);
    std::memcpy(out->m0, img, kPurgeGranule);
    std::memcpy(out->p0, img + 2 * kPurgeGranule, kPurgeGranule);
  }
  return true;
}
inline bool compile_keyed_glob(const std::string& pat, KeyedGlob* out, std::string* error) {
  return compile_keyed_glob(reinterpret_cast<const uint8_t*>(pat.data()), pat.size(), out, error);
}

// Escapes a literal byte string for compile_keyed_glob: '\' and, unless keep_stars, '*'.
inline std::string keyed_glob_escape(const std::string& s, bool keep_stars) {
  std::string o;
  o.reserve(s.size() + 8);
  for (const char c : s) {
    if (c == '\\' || (c == '*' && !keep_stars)) o.push_back('\\');
    o.push_back(c);
  }
  return o;
}

// The matching algorithm on key[0..klen). Work: at most klen x (longest middle segment)
// byte compares.
inline bool keyed_glob_matches(const KeyedGlob& g, const uint8_t* key, size_t klen) {
  if (klen == 0 || klen < g.min_len) return false;
  const void* const sep = std::memchr(key, kVarySep, klen);
  const size_t slen = sep ? (size_t)(static_cast<const uint8_t*>(sep) - key) : klen;
  if (slen < g.min_len) return false;
  if (g.stars == 0 && slen != g.head_len) return false;
  if (g.head_len && std::memcmp(key, g.lit, g.head_len) != 0) return false;
  if (g.tail_len && std::memcmp(key + slen - g.tail_len, g.lit + g.tail_off, g.tail_len) != 0)
    return false;
  size_t cur = g.head_len;
  const size_t lim = slen - g.tail_len;
  for (uint32_t m = 0; m < g.nmid && m < kMaxGlobStars; ++m) {
    const uint8_t* const seg = g.lit + g.mid[m][0];
    const size_t len = g.mid[m][1];
    bool found = false;
    for (; cur + len <= lim; ++cur)
      if (std::memcmp(key + cur, seg, len) == 0) {
        found = true;
        break;
      }
    if (!found) return false;
    cur += len;
  }
  return true;
}

// The same for a whole keyed value [u16 klen | key | payload] (keyed_tags_match's bounds).
inline bool keyed_value_glob_matches(const KeyedGlob& g, const uint8_t* v, size_t vlen) {
  if (vlen < kKeyedPrefix) return false;
  uint16_t kl;
  std::memcpy(&kl, v, kKeyedPrefix);
  if (kKeyedPrefix + (size_t)kl > vlen) return false;
  return keyed_glob_matches(g, v + kKeyedPrefix, kl);
}

// ---- listing (HbmCache / HostCache::list_keyed) ----------------------------------------------
// One row per listed object, in index-slot order; row r's key area is keys + r * key_cap and
// holds the head of the stored keyed image [u16 klen | key ...]: the granules that hold the
// key, at most key_cap bytes (a key longer than key_cap - 2 bytes comes back truncated).
constexpr uint32_t kMaxListRows = 4096;
constexpr uint32_t kListKeyCapMin = 16, kListKeyCapMax = 1024;
enum : uint32_t { kListPrefix = 0, kListTags = 1, kListAll = 2, kListGlob = 3 };
constexpr uint32_t kListRefBit = 1;   // ListRow::bits: the CLOCK reference bit
constexpr uint32_t kListChanged = 2;  // the entry changed after it was matched (klen = 0)

struct alignas(16) ListRow {
  uint64_t slot;    // index slot
  uint64_t loc;     // the entry's loc word (logical log offset of the record + 1)
  uint64_t d0, d1;  // digest
  uint32_t vlen;    // stored value bytes (the keyed image: 2 + klen + payload)
  uint32_t expire;  // absolute expiry, 0 = never
  uint32_t flags;   // ItemHeader::flags
  uint32_t klen;
  uint32_t ntags;   // 0: no or malformed tag block, kTagOverflow, else the block's count
  uint32_t bits;    // kListRefBit | kListChanged
  uint32_t pad[2];
};
static_assert(sizeof(ListRow) == 64, "ListRow is four 16-byte granules");

// Result words of a listing.
enum : int { kListMatched = 0, kListBytes = 1, kListListed = 2, kListNext = 3, kListWords = 4 };

// ntags of a keyed value as ListRow reports it.
inline uint32_t keyed_ntags(const uint8_t* v, size_t vlen) {
  if (vlen < kKeyedPrefix) return 0;
  uint16_t kl;
  std::memcpy(&kl, v, kKeyedPrefix);
  const size_t o = kKeyedPrefix + kl;
  if (o + 2 > vlen || v[o] != kTagMarker) return 0;
  const unsigned nt = v[o + 1];
  if (nt == kTagOverflow) return kTagOverflow;
  if (nt > kMaxObjectTags || o + 2 + 8 * (size_t)nt > vlen) return 0;
  return nt;
}

}  // namespace shellac
