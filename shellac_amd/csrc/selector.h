// One invalidation or inspection request, from the HTTP handler down to a shard: which keyed
// values it selects (KeyedSelector) and what is done to them (PurgeAction). Every layer takes
// these two; the matchers, their limits and the device images of keyed.h are applied here and
// nowhere else on the host. No I/O and no HIP: tests/native/selector_main.cc runs all of it
// under sanitizers.
#pragma once

#include <cassert>
#include <cstdint>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "keyed.h"

namespace shellac {

// Which stored values [u16 klen | key | payload]: those whose key starts with (Prefix) or
// equals (Exact) `pattern`, that carry one of the tag hashes in `tags` or the overflow block
// (Tags), whose key up to its first 0x1f matches the glob `pattern` (Glob), or all of them.
// A value type built by the factories, which refuse what every tier refuses: an empty pattern
// or one over kMaxKeyedKey, no tags or more than kMaxPurgeTags, a glob compile_keyed_glob
// refuses. A refused selector keeps its kind and bytes, is not valid() and selects nothing.
// The fields are for reading: a selector is made by a factory and never edited.
struct KeyedSelector {
  enum class Kind : uint8_t { All, Prefix, Exact, Tags, Glob };

  static KeyedSelector prefix(std::string bytes) { return keyed(Kind::Prefix, std::move(bytes)); }
  static KeyedSelector exact(std::string bytes) { return keyed(Kind::Exact, std::move(bytes)); }
  static KeyedSelector tags(std::vector<uint64_t> hashes) {
    KeyedSelector s;
    s.kind = Kind::Tags;
    s.ok = !hashes.empty() && hashes.size() <= kMaxPurgeTags;
    s.hashes = std::move(hashes);
    return s;
  }
  // The one place a request's glob is compiled; `why`: compile_keyed_glob's message.
  static KeyedSelector glob(std::string pattern, std::string* why = nullptr) {
    KeyedSelector s;
    s.kind = Kind::Glob;
    auto g = std::make_shared<KeyedGlob>();
    s.ok = compile_keyed_glob(pattern, g.get(), why);
    if (s.ok) s.compiled = std::move(g);
    s.pattern = std::move(pattern);
    return s;
  }

  bool valid() const { return ok; }
  // the engine's listing mode (HbmCache / HostCache::list_keyed)
  uint32_t list_mode() const {
    return kind == Kind::All ? kListAll : kind == Kind::Tags ? kListTags
           : kind == Kind::Glob ? kListGlob : kListPrefix;
  }

  // Whether the stored value v[0..n) is selected; a value whose klen points past its end never
  // is.
  bool matches_value(const uint8_t* v, size_t n) const {
    if (!ok || n < kKeyedPrefix) return false;
    uint16_t kl;
    std::memcpy(&kl, v, kKeyedPrefix);
    if (kKeyedPrefix + (size_t)kl > n) return false;
    switch (kind) {
      case Kind::All: return kl != 0;
      case Kind::Tags: return keyed_tags_match(v, n, hashes.data(), hashes.size());
      case Kind::Glob: return compiled && keyed_glob_matches(*compiled, v + kKeyedPrefix, kl);
      case Kind::Exact: if (kl != pattern.size()) return false; break;
      case Kind::Prefix: if (kl < pattern.size()) return false; break;
    }
    return std::memcmp(v + kKeyedPrefix, pattern.data(), pattern.size()) == 0;
  }

  // A fill in flight when this purge was taken: would it store a selected object? `key`: the
  // key it would be stored under, `base_key`: its URL's key (an exact or glob purge of the URL
  // covers every variant), `fill_tags`: its tag hashes (null: untagged, which no tag purge
  // selects), `overflow`: it named too many tags, so every tag purge selects it. Prefix and
  // Exact compare the bytes as given, refused or not.
  bool matches_fill(const std::string& key, const std::string& base_key,
                    const std::vector<uint64_t>* fill_tags, bool overflow) const {
    switch (kind) {
      case Kind::All: return true;
      case Kind::Prefix: return key.compare(0, pattern.size(), pattern) == 0;
      case Kind::Exact: return base_key == pattern;
      case Kind::Glob:
        return ok && compiled && keyed_glob_matches(*compiled,
                                        reinterpret_cast<const uint8_t*>(base_key.data()),
                                        base_key.size());
      case Kind::Tags:
        if (!fill_tags) return false;
        if (overflow) return true;
        for (const uint64_t h : *fill_tags)
          for (const uint64_t p : hashes)
            if (p == h) return true;
        return false;
    }
    return false;
  }

  // The image a device scan reads: the prefix image (Prefix, Exact), the compiled glob's bytes
  // in use, the hash list padded to 16 bytes; nothing for All. valid() only.
  size_t image_bytes() const {
    assert(valid() && (kind != Kind::Glob || compiled));
    switch (kind) {
      case Kind::All: return 0;
      case Kind::Tags: return (hashes.size() * sizeof(uint64_t) + 15) & ~(size_t)15;
      case Kind::Glob: return keyed_glob_used_bytes(*compiled);
      default: return keyed_prefix_image_bytes(pattern.size());
    }
  }
  void write_image(uint8_t* dst) const {
    assert(valid() && (kind != Kind::Glob || compiled));
    switch (kind) {
      case Kind::All: return;
      case Kind::Tags:
        std::memset(dst, 0, image_bytes());
        std::memcpy(dst, hashes.data(), hashes.size() * sizeof(uint64_t));
        return;
      case Kind::Glob: std::memcpy(dst, compiled.get(), image_bytes()); return;
      default:
        write_keyed_prefix_image(dst, reinterpret_cast<const uint8_t*>(pattern.data()),
                                 pattern.size());
    }
  }

  Kind kind = Kind::All;
  bool ok = true;
  std::string pattern;                        // Prefix, Exact; Glob: the pattern as written
  std::vector<uint64_t> hashes;               // Tags
  std::shared_ptr<const KeyedGlob> compiled;  // Glob, valid() only

 private:
  static KeyedSelector keyed(Kind k, std::string bytes) {
    KeyedSelector s;
    s.kind = k;
    s.ok = !bytes.empty() && bytes.size() <= kMaxKeyedKey;
    s.pattern = std::move(bytes);
    return s;
  }
};

// What a purge does to the selected objects. Hard: they are removed. Soft: they are kept and
// made stale: the flags word (the proxy's freshness time) becomes stale_at and, with
// keep_s != 0, an object that never expires or expires later than keep_s seconds from now
// expires then (a life is only shortened).
struct PurgeAction {
  bool soft = false;
  uint32_t stale_at = 0, keep_s = 0;
  static PurgeAction remove() { return {}; }
  static PurgeAction soften(uint32_t stale_at, uint32_t keep_s) { return {true, stale_at, keep_s}; }
};

// What no tier carries out as a scan: a refused selector, everything (that is flush()) and the
// removal of one key (that is del()).
inline bool purge_refused(const KeyedSelector& what, const PurgeAction& how) {
  return !what.valid() || what.kind == KeyedSelector::Kind::All ||
         (what.kind == KeyedSelector::Kind::Exact && !how.soft);
}

}  // namespace shellac
