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

}  // namespace shellac
