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

// ---- listing (HbmCache / HostCache::list_keyed) ----------------------------------------------
// One row per listed object, in index-slot order; row r's key area is keys + r * key_cap and
// holds the head of the stored keyed image [u16 klen | key ...]: the granules that hold the
// key, at most key_cap bytes (a key longer than key_cap - 2 bytes comes back truncated).
constexpr uint32_t kMaxListRows = 4096;
constexpr uint32_t kListKeyCapMin = 16, kListKeyCapMax = 1024;
enum : uint32_t { kListPrefix = 0, kListTags = 1, kListAll = 2 };
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
