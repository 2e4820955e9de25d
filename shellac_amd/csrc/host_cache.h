// Host-DRAM cache shard with exactly the HBM shard's layout and semantics.
//
// Uses: (a) the cache backend on machines/CI without a GPU, (b) the semantic
// reference the HIP kernels are tested against, (c) the CPU implementation of the
// batch ops when the distributed serving path runs over gloo. Thread-safe (one
// mutex per shard; the proxy stripes keys over several shards for concurrency).
#pragma once

#include <mutex>
#include <string>
#include <vector>

#include "keyed.h"
#include "layout.h"
#include "conditional.h"
#include "slice.h"

namespace shellac {

class HostCache {
 public:
  // evict: 0 FIFO, 1 CLOCK (as ShardConfig::evict); reinsert_max 0 = auto budget.
  HostCache(uint64_t log_bytes, uint64_t nbuckets, uint32_t max_item, int evict = 1,
            uint64_t reinsert_max = 0);
  ~HostCache();
  HostCache(const HostCache&) = delete;
  HostCache& operator=(const HostCache&) = delete;

  void lookup(const Digest* keys, int64_t n, uint64_t* loc, uint64_t* size, uint64_t* off,
              uint32_t now, uint64_t reserve = 0);
  void gather(const uint64_t* loc, const uint64_t* off, int64_t n, uint8_t* out) const;
  void store(const Digest* keys, const uint8_t* values, const uint64_t* val_off,
             const uint32_t* vlen, const uint32_t* flags, const uint32_t* expire, int64_t n,
             uint32_t now, uint64_t bytes_bound = 0);  // 0: the batch's exact bytes
  void remove(const Digest* keys, int64_t n, uint8_t* found, uint32_t now);
  void sweep(uint32_t now, uint64_t* live_entries, uint64_t* live_bytes);
  // Prefix purge of keyed values (HbmCache::remove_keyed_prefix, whose semantic reference
  // this is): removes every live entry whose record is its own (magic, digest, vlen) and
  // whose stored key starts with prefix[0..plen), 1 <= plen <= 65535;
  // out = {entries removed, their item bytes}, also counted as `purged`.
  void remove_keyed_prefix(const uint8_t* prefix, uint32_t plen, uint32_t now, uint64_t out[2]);
  // Soft purge of keyed values (HbmCache::soften_keyed_prefix, whose semantic reference this
  // is): every live entry whose record is its own and whose stored key starts with (exact:
  // equals) prefix[0..plen) gets flags = stale_at and, where expire_cap != 0 and the entry
  // never expires or expires after it, expire = expire_cap — in the index and the record
  // header; nothing else changes. expire_cap is 0 or > now. Returns the live matches.
  uint64_t soften_keyed_prefix(const uint8_t* prefix, uint32_t plen, bool exact, uint32_t stale_at,
                               uint32_t expire_cap, uint32_t now);
  // Tag purge (HbmCache::remove_keyed_tags, whose semantic reference this is): removes every
  // live entry whose record is its own and whose keyed value carries a tag block (keyed.h)
  // matching tags[0..ntags), 1 <= ntags <= 64; out as remove_keyed_prefix.
  void remove_keyed_tags(const uint64_t* tags, uint32_t ntags, uint32_t now, uint64_t out[2]);
  // Soft tag purge: the same matcher with soften_keyed_prefix's action; returns the live matches.
  uint64_t soften_keyed_tags(const uint64_t* tags, uint32_t ntags, uint32_t stale_at,
                             uint32_t expire_cap, uint32_t now);
  // Glob purge and its soft form (HbmCache::remove_keyed_glob / soften_keyed_glob, whose
  // semantic reference these are): the walks above with keyed_value_glob_matches on the
  // compiled pattern; out and the return value as the prefix forms'.
  void remove_keyed_glob(const KeyedGlob& g, uint32_t now, uint64_t out[2]);
  uint64_t soften_keyed_glob(const KeyedGlob& g, uint32_t stale_at, uint32_t expire_cap,
                             uint32_t now);
  // Listing (HbmCache::list_keyed, whose semantic reference this is): the same modes, checks,
  // rows, key areas and result words, in this index's own slot order; `prefix` is the plain
  // prefix (kListGlob: the plain pattern), not a pattern image. No row is ever flagged kListChanged here.
  void list_keyed(uint32_t mode, const uint8_t* prefix, uint32_t plen, bool exact,
                  const uint64_t* tags, uint32_t ntags, uint64_t start_slot, uint32_t limit,
                  uint32_t key_cap, uint32_t now, ListRow* rows, uint8_t* keys,
                  uint64_t out[kListWords]);
  // In-place change of expiry (and flags, nullable) of each row's live entry, in the index
  // and in the record header (HbmCache::touch, whose semantic reference this is). With key
  // bytes (nullable with their offsets) a row only matches a keyed record of exactly that key.
  // hit[i] = 1 iff a live entry was updated, also counted as `touched`.
  void touch(const Digest* keys, const uint32_t* expire, const uint32_t* flags,
             const uint8_t* key_bytes, const int64_t* key_offs, int64_t n, uint8_t* hit,
             uint32_t now);
  // Sliced GET (HbmCache::get_keyed_slices, whose semantic reference this is): the same rows,
  // the same bytes in `out` (nothing when the total exceeds out_cap), the same result words,
  // reference bit and counters, under the same conditions (nullable). Built on slice.h and
  // conditional.h.
  void get_keyed_slices(const Digest* keys, const uint8_t* key_bytes, const int64_t* key_offs,
                        const SliceSpec* spec, int64_t n, SliceRow* rows, uint8_t* out,
                        uint64_t out_cap, uint64_t res[kSliceWords], uint32_t now,
                        uint64_t reserve = 0, const SliceCond* cond = nullptr,
                        const uint8_t* cond_bytes = nullptr);
  void flush();
  // Tests: see HbmCache::debug_bucket / debug_set_entry.
  std::vector<uint64_t> debug_bucket(uint64_t b);
  // {hand (ring index), ring tail, head, the log offset of the hand's item (~0: none)}
  std::vector<uint64_t> debug_hand();
  void debug_set_entry(uint64_t b, int slot, uint64_t d0, uint64_t d1, uint64_t loc,
                       uint32_t vlen, uint32_t expire);
  void debug_set_hand(uint64_t hand, bool catch_up = true);  // HbmCache::debug_set_hand
  uint64_t export_keys(Digest* out, uint64_t out_cap, uint32_t now);
  void save(const std::string& path, const uint64_t user[4]);
  void load(const std::string& path, uint64_t user[4]);
  CacheCounters counters();
  uint64_t head();

  // Single-key conveniences used by the proxy / memcached server. get() copies
  // the value (not the header) into `out` and returns false on miss.
  bool get_one(const Digest& key, std::vector<uint8_t>* out, uint32_t* flags, uint32_t now,
               uint32_t* expire = nullptr);
  bool get_one(const Digest& key, std::string* out, uint32_t* flags, uint32_t now,
               uint32_t* expire = nullptr);
  void set_one(const Digest& key, const uint8_t* value, uint32_t vlen, uint32_t flags,
               uint32_t expire, uint32_t now);

  uint64_t log_bytes() const { return log_bytes_; }
  uint64_t nbuckets() const { return nbuckets_; }
  uint32_t max_item() const { return max_item_; }
  uint64_t reinsert_max() const { return evict_ ? rmax_ : 0; }

 private:
  // The keyed index scans (purge, soft purge, listing). keyed_record: the record of slot k if
  // its entry is live, its own (digest, vlen, magic) and of vmin..max_item value bytes, else
  // null. keyed_scan: act(k, rec, vlen) for every slot, in slot order, whose record passes
  // keyed_record with match.vmin() and whose keyed value passes match(v, vlen). remove_keyed
  // and soften_keyed are the two actions the purges share, with their results and checks.
  uint8_t* keyed_record(uint64_t k, uint32_t now, uint32_t vmin, uint32_t* vlen_out);
  template <class Match, class Act>
  void keyed_scan(uint32_t now, Match match, Act act);
  template <class Match>
  void remove_keyed(uint32_t now, Match match, uint64_t out[2]);
  template <class Match>
  uint64_t soften_keyed(uint32_t now, Match match, uint32_t stale_at, uint32_t expire_cap);
  struct Row {  // one SET row of a (possibly combined) batch
    Digest key;
    const uint8_t* val;
    uint32_t vlen, flags, expire;
    uint64_t from = 0;  // a CLOCK reinsertion: a move of the entry at this loc (see HbmCache)
  };
  bool insert_locked(const Digest& d, uint64_t loc1, uint32_t vlen, uint32_t expire, uint32_t now);
  // mark: a GET (sets the CLOCK reference bit of the entry it finds)
  uint64_t probe_locked(const Digest& d, uint32_t now, uint32_t* vlen, uint64_t reserve = 0,
                        bool mark = false);
  void store_rows_locked(const std::vector<Row>& rows, uint32_t now);
  // CLOCK hand step ahead of a batch of `bytes` log bytes over `n` rows (the device
  // algorithm, sequentially): appends the reinsertion rows to `out`, their records
  // staged in `stage`.
  void reclaim_locked(int64_t n, uint64_t bytes, uint64_t rmax, uint32_t now,
                      std::vector<Row>* out, std::vector<uint8_t>* stage, bool lead_mode);

  uint64_t log_bytes_, nbuckets_, mask_;
  uint32_t max_item_;
  uint8_t* log_ = nullptr;
  size_t log_alloc_ = 0;
  Entry* index_ = nullptr;
  size_t index_alloc_ = 0;
  uint64_t head_ = 0;
  CacheCounters ctr_{};
  mutable std::mutex mu_;
  int evict_ = 1;
  uint64_t rmax_ = 0;
  std::vector<uint64_t> ring_;  // item starts in log order (kRingSkip holes)
  uint64_t ring_tail_ = 0, hand_ = 0;
  uint64_t hand_consumed_ = 0;  // entries the hand consumed last batch (adaptive window)
  bool lead_ = false;  // the hand's mode (layout.h hand_lead, sticky)
  bool catch_up_ = true;  // debug_set_hand
};

// CPU versions of the device batch helpers (same contracts as hbm_cache.h).
void host_exclusive_scan(const uint64_t* in, uint64_t* out, int64_t n);
// src_off[i] == kHostSegSkip (hbm_cache.h kSegSkip): segment i is a gap, nothing read or
// written; nothing at all is copied when dst_off[n] > dst_cap.
constexpr uint64_t kHostSegSkip = ~0ull;
void host_segcopy(const uint8_t* src, const uint64_t* src_off, const uint64_t* dst_off, int64_t n,
                  uint8_t* dst, uint64_t dst_cap = ~0ull);
// Segment i holds seg_len[i] bytes at dst + dst_off[i]; the bytes up to dst_off[i + 1] are
// left as they are, and a segment that does not end within `cap` is dropped.
void host_segcopy_sized(const uint8_t* src, const uint64_t* src_off, const uint64_t* dst_off,
                        const uint64_t* seg_len, int64_t n, uint8_t* dst, uint64_t cap = ~0ull);
void host_digest_keys(const uint8_t* bytes, const int64_t* offs, int64_t n, Digest* out);
void host_route_keys(const Digest* keys, int64_t n, const uint32_t* ring_pts,
                     const int32_t* ring_owner, int32_t npts, int32_t* dest, int64_t* counts,
                     int32_t nranks);
void host_scatter_by_dest(const int32_t* dest, const int64_t* base, int64_t n, int32_t nranks,
                          int64_t* cursor, int64_t* perm);
void host_permute_records(const void* in, const int64_t* perm, int64_t n, int32_t rec_bytes,
                          void* out);

}  // namespace shellac
