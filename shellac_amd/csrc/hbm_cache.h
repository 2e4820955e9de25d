// HBM-resident cache shard (one per MI355X GPU) and its batch operations.
//
// Capability parity: this is the "distributed key/value store" side of Shellac,
// which the reference delegates to memcached through pylibmc
// (src/python/shellac/server/Server.py:79-83 client, :335 get, :432 set with
// time=ttl). The README's roadmap item "replacing Memcached with a
// purpose-built cache" (README.md:79) is what this class is.
//
// Every operation is a *batch* of fixed 16-byte digests on a HIP stream; all
// pointer arguments are device pointers unless stated otherwise. No operation
// allocates or synchronises except where documented (lookup_total, sweep,
// counters, reserve), so the batch pipeline can run back-to-back on a stream.
#pragma once

#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <mutex>
#include <string>
#include <vector>

#include "keyed.h"
#include "layout.h"
#include "conditional.h"
#include "slice.h"

namespace shellac {

// Eviction policies of the value log (ShardConfig::evict).
enum : int { kEvictFifo = 0, kEvictClock = 1 };

struct ShardConfig {
  uint64_t log_bytes = 1ull << 30;  // value-log capacity (multiple of 16)
  uint64_t nbuckets = 1ull << 20;   // power of two, 4 entries (128 B) each
  uint32_t max_item = 1u << 20;     // max value bytes (memcached's 1 MB item limit)
  int device = 0;
  // kEvictClock: items read since the hand last passed get re-appended instead of being
  // overwritten (CLOCK / FIFO-reinsertion, memcached-LRU-like hit ratios under
  // capacity pressure). kEvictFifo: plain circular log.
  int evict = kEvictClock;
  uint64_t reinsert_max = 0;  // reinsertion budget per SET batch (bytes); 0 = auto
  int serve_blocks = 8;       // resident edge-server blocks (serve_get jobs side by side)
};

// What HbmCache::store waits for, completes and queues beyond the plain chain (all optional).
struct StoreOpts {
  // The chain up to the log write runs at once, the index insert waits for this event. A
  // lookup enqueued (on another stream) before this store and followed by the event
  // therefore runs concurrently with the SET's dedupe, sizing and log append: it reads the
  // index and the current head slot, which only the index insert changes, and a `reserve`
  // covering this SET keeps its gather off the bytes the append overwrites.
  hipEvent_t index_after = nullptr;
  // The log append (and what follows) waits for this event; the CLOCK hand, the dedupe and
  // the sizing (reads only) run at once — beside a gather that still reads the region the
  // append will overwrite.
  hipEvent_t append_after = nullptr;
  // Recorded right after the log append (a caller can keep its gather from contending with
  // it).
  hipEvent_t append_done = nullptr;
  // Recorded after the batch's planning kernels (dedupe, sizes, offsets).
  hipEvent_t plan_done = nullptr;
  // Completes with everything this call queued; carried by the chain's last kernel as its
  // completion signal (profiles/r6_hop: ~2.4 us sooner across queues than a recorded
  // event), or recorded when the call queued no chain.
  hipEvent_t done = nullptr;
  // 1 queues only the batch's CLOCK hand and planning, 2 the rest of its chain (0: both).
  // A phase-1 hand is *detached*: it may run as soon as the previous batch's planning is
  // done (`plan_done` of that batch's phase 2), beside that batch's log append and index
  // insert. It reads the head the previous append will reach (the claim word) and the ring
  // tail of the batch before (the last one whose ring entries are written), and its
  // reinsertions are indexed as *moves*: a reinsertion row's insert CASes the entry from
  // the item's old location to the new one, and is dropped when the entry has moved on
  // (a SET or DELETE of the key landed after the hand read the index) — so an early hand
  // can never resurrect a superseded or deleted value. Two hand buffers alternate, so the
  // hand of batch k+1 never writes what batch k's append still reads.
  int phase = 0;
  // false: no CLOCK hand this batch (the append stays within `bytes_bound`; a caller that
  // reserved only that much for it, see would_reclaim).
  bool allow_reclaim = true;
};

class HbmCache {
 public:
  explicit HbmCache(const ShardConfig& cfg);
  ~HbmCache();
  HbmCache(const HbmCache&) = delete;
  HbmCache& operator=(const HbmCache&) = delete;

  // GET phase 1: probe both candidate buckets of every key. Writes, per key,
  // the physical log offset of the item (kMissLoc on miss) and the bytes the
  // item occupies in a GET response (0 on miss); then an exclusive scan of the
  // sizes into off[0..n] (off[n] = total response bytes).
  // `reserve` > 0 treats objects that the next `reserve` appended bytes will
  // overwrite as misses, so SETs may be queued between this lookup and its gather.
  // `total_slot` >= 0 also writes off[n] straight into host slot `total_slot` (pinned,
  // coherent), readable with host_slot() once the stream has passed the lookup: the
  // response size without a D2H copy.
  // `first` (coalesce_keys output, may be null): rows with first[i] != i are duplicates
  // and are answered as misses without touching the index (expand_coalesced fills them
  // in after the gather).
  void lookup(const Digest* keys, int64_t n, uint64_t* loc, uint64_t* size, uint64_t* off,
              uint32_t now, hipStream_t s, uint64_t reserve = 0, int total_slot = -1,
              const uint32_t* first = nullptr);
  // Coalescing lookup: coalesce_keys and lookup(first=...) in one pass — the row that
  // claims a digest probes the index for it; duplicate rows get size 0 (fill them in
  // with expand_coalesced after the gather). `table`: coalesce_table_slots(n) words.
  // `cslot` (optional, u32 [n]): each claiming row's table slot, for
  // expand_coalesced_out to clear; `table_clean`: the caller guarantees a zeroed table
  // (skips the memset).
  // `prefix` (optional, kMaxGrid + 1 words): the blocked lookup — `off` gets one packed word
  // per row, (the row's offset within its lookup workgroup's rows) << 21 | its record bytes
  // (0 for a miss or a duplicate request), `size` is not written (may be null), `loc` is
  // written for claiming rows only, and `prefix` gets the exclusive prefix of the workgroup
  // totals (one small scan instead of the n-row one); returns the row shift of a workgroup
  // (its rows are [b << shift, (b + 1) << shift)), for gather(prefix, shift).
  // Without `prefix`: `off` is the exclusive scan of `size`; returns -1.
  // `index_done`: completes with the kernel that reads (and reference-marks) the index, as
  // that kernel's own completion signal (no marker packet between it and the next kernel
  // of `s`): a SET's index insert on another stream may wait for it.
  int lookup_coalesced(const Digest* keys, int64_t n, uint32_t* table, int64_t table_slots,
                       uint32_t* first, uint64_t* loc, uint64_t* size, uint64_t* off,
                       uint32_t now, hipStream_t s, uint64_t reserve = 0, int total_slot = -1,
                       uint32_t* cslot = nullptr, bool table_clean = false,
                       uint64_t* prefix = nullptr, hipEvent_t index_done = nullptr);
  // Slotted lookup (the routed step's owner side): nslots x slot_rows rows, slot k's
  // rows [k * slot_rows, k * slot_rows + slot_cnt[k]) are requests, the rest padding
  // (size 0, not probed, not counted). off = exclusive scan over all rows.
  // `reserve_dev` (optional, device word): a reserve the stream computes before the
  // probe runs (the routed step's received SET bytes), as lookup's `reserve`.
  void lookup_slots(const Digest* keys, int64_t nslots, int64_t slot_rows,
                    const int64_t* slot_cnt, uint64_t* loc, uint64_t* size, uint64_t* off,
                    uint32_t now, hipStream_t s, const uint64_t* reserve_dev = nullptr);
  uint64_t host_slot(int i) const;
  // Spin until the lookup that was given `total_slot` i has written it (no stream or
  // event synchronisation: the kernel's system-scope store is the signal). Throws after
  // timeout_ms. Each lookup that names a slot must be waited for before the slot is reused.
  uint64_t wait_host_slot(int i, int64_t timeout_ms = 10000) const;
  static constexpr int kHostSlots = 64;
  static constexpr int kHeadSlot = kHostSlots - 2;  // the SET chain publishes the head here
  static constexpr uint64_t kSlotPending = ~0ull;
  static constexpr uint64_t kSlotFailed = ~0ull - 1;  // the edge GET could not complete
  // words of a lookup_coalesced `prefix` (the lookup's workgroups, at most 2048, + 1)
  static constexpr int64_t kLookupPrefixWords = 2049;
  // Edge GET (the proxy's micro-batches, n <= kSmallGetMax): probe + scan + gather in
  // one launch, every key probed once (decoupled look-back scan across workgroups).
  // keys / out / off may be mapped host memory (no copies); off[0..n] is always written;
  // off[n] > out_cap means the output is incomplete (nothing is written past out_cap) and
  // the batch must be repeated into a bigger buffer.
  // `done_slot` >= 0: the kernel's last workgroup writes off[n] (or kSlotFailed) into
  // that host slot after every output byte is visible to the host, so
  // wait_host_slot(done_slot) replaces a stream synchronisation. Launches are ordered on
  // their stream (the look-back state is shared), several may be queued at once with
  // distinct slots.
  void small_get(const Digest* keys, int64_t n, uint8_t* out, uint64_t out_cap, uint64_t* off,
                 uint32_t now, hipStream_t s, int done_slot = -1);
  static constexpr int64_t kSmallGetMax = 1 << 17;
  // Persistent edge-GET server: the same contract as small_get for batches of at most
  // kServeKeys rows, answered by one resident workgroup that polls a ring of jobs in
  // pinned host memory — no kernel launch and no stream per batch. The keys are copied
  // into the ring (host pointer); out / off are device views of mapped memory as for
  // small_get, and the total (or kSlotFailed) lands in host slot `done_slot`.
  // Returns false (nothing queued) when the ring is full or n is out of range; the
  // caller then uses small_get. Each call must eventually be followed by serve_kick()
  // calls while its slot is pending (the server exits when idle or at the end of its
  // lifetime, and serve_kick restarts it if jobs are outstanding). Records a SET
  // overwrites while the server copies them come back with a zeroed magic word (the
  // caller treats them as misses). Not ordered against anything on any stream: the
  // caller keeps GETs of keys with SETs / DELETEs in flight on the stream path.
  static constexpr int kServeKeys = 29;   // a job (5 + 2 per key 16-B granules) is one wave's load
  static constexpr int kServeRing = 16;
  bool serve_get(const Digest* host_keys, int64_t n, uint8_t* out, uint64_t out_cap,
                 uint64_t* off, uint32_t now, int done_slot);
  // The same, ordered after the work queued so far on stream `after` only (what the caller
  // queued there to fill `out` / `off`, or SETs it queued on that stream): an event recorded
  // there is host-polled before the job is queued, so the stream-less server never races it.
  // SETs queued on other streams are not covered (ShardedCache queues its SETs on its side
  // and hand streams: call its sync_sets() first).
  bool serve_get_after(hipStream_t after, const Digest* host_keys, int64_t n, uint8_t* out,
                       uint64_t out_cap, uint64_t* off, uint32_t now, int done_slot);
  void serve_kick();
  // server jobs queued or running (the resident workgroup takes them one at a time: a
  // caller with several batches in flight sends the rest down the launched path)
  uint64_t serve_backlog() const {  // any thread (the batcher, reactors submitting directly)
    uint64_t c = 0;
    for (int b = 0; b < srv_blocks_; ++b)
      c += __atomic_load_n(srv_ctl_ + kSrvCtlConsumed + 8 * b, __ATOMIC_ACQUIRE);
    const uint64_t t = __atomic_load_n(&srv_ticket_, __ATOMIC_RELAXED);
    return t > c ? t - c : 0;
  }
  static constexpr int kServeBlocksMax = 8;
  static constexpr int kSrvCtlConsumed = 24;  // control word of block 0's consumed count
  int serve_blocks() const { return srv_blocks_; }
  // wait_host_slot for a serve_get job: spins, relaunching the server when it exited
  uint64_t serve_wait(int done_slot, int64_t timeout_ms = 10000);
  void serve_stop();  // ask the server to exit and wait for it (outstanding jobs stay queued)
  uint64_t serve_launches() const { return srv_launches_; }
  uint64_t serve_jobs() const { return __atomic_load_n(&srv_ticket_, __ATOMIC_RELAXED); }
  // Phase stamps of the last (up to 64) server jobs, wall-clock ticks of the device:
  // rows of {ticket, poll issued, job seen, probed, copied, publish, n, total bytes}; and the
  // tick rate (kHz).
  std::vector<uint64_t> serve_trace() const;
  uint64_t wall_khz() const { return srv_khz_; }
  // GET phase 2: copy each hit's [ItemHeader | value | pad] to out + off[i]. `out` may be
  // pinned host memory (zero-copy); nothing is written when off[n] > out_cap, so the
  // caller can queue the gather before it knows the total and retry if it did not fit.
  // `first` (a coalesced lookup): the gather's workgroups also write every request's
  // (size, off) from its claimer into out_size / out_off and clear the claimers' slots of
  // the coalescing table (expand_coalesced_out's work, no launch of its own).
  // `prefix`, `shift` (a blocked lookup, lookup_coalesced with a prefix): `off` holds its
  // packed rows, `size` and `cslot` are unused, and all `table_slots` words of `table` are
  // zeroed by streaming stores instead of a store per claimer.
  void gather(const uint64_t* loc, const uint64_t* off, int64_t n, uint8_t* out, hipStream_t s,
              uint64_t out_cap = ~0ull, const uint32_t* first = nullptr,
              const uint64_t* size = nullptr, uint64_t* out_size = nullptr,
              uint64_t* out_off = nullptr, uint32_t* table = nullptr,
              const uint32_t* cslot = nullptr, const uint64_t* prefix = nullptr,
              int shift = 0, int64_t table_slots = 0);
  // SET a batch. values + val_off[i] holds vlen[i] bytes (val_off 16-byte aligned,
  // the buffer readable 16 bytes past every value). Later duplicates of a key in
  // the same batch win. `bytes_bound` must bound sum(item_bytes(vlen)). `o`: the events
  // the chain waits for and completes, and which part of it this call queues (StoreOpts).
  void store(const Digest* keys, const uint8_t* values, const uint64_t* val_off,
             const uint32_t* vlen, const uint32_t* flags, const uint32_t* expire, int64_t n,
             uint64_t bytes_bound, uint32_t now, hipStream_t s, const StoreOpts& o = {});
  // Whether a SET of `bytes_bound` bytes issued now would run the CLOCK hand (the log is
  // within a few batches of wrapping); the answer can only turn true later.
  bool would_reclaim(uint64_t bytes_bound) const {
    return cfg_.evict == kEvictClock && rmax_ && should_reclaim(bytes_bound);
  }
  // SET through captured hipGraphs, for callers with fixed batch sizes and fixed
  // staging buffers (the proxy's micro-batches, padded to a size class with
  // vlen = kSkipVlen rows). The five SET kernels become one graph launch. A graph bakes
  // in its pointers, `n`, `bytes_bound` and `now` and the head slot it reads, so `g`
  // keeps one executable per head-slot parity and is re-captured whenever any of those
  // (or the SET workspace) changes; `now` changes once a second.
  struct StoreGraph {
    hipGraphExec_t exec[2] = {nullptr, nullptr};
    const void* ptrs[6] = {};
    int64_t n = -1;
    uint64_t bound = 0;
    uint32_t now = 0;
    uint64_t ws_gen = 0;
    uint64_t captures = 0, launches = 0;
  };
  void store_graph(StoreGraph* g, const Digest* keys, const uint8_t* values,
                   const uint64_t* val_off, const uint32_t* vlen, const uint32_t* flags,
                   const uint32_t* expire, int64_t n, uint64_t bytes_bound, uint32_t now,
                   hipStream_t s);
  static void destroy_graph(StoreGraph* g);
  // DELETE a batch; found[i] = 1 if a live entry was removed.
  void remove(const Digest* keys, int64_t n, uint8_t* found, uint32_t now, hipStream_t s);
  // Prefix purge of *keyed* values ([u16 klen | key | payload], keyed.h): removes every
  // live entry whose stored key starts with the prefix, exactly as DELETE removes one (the
  // entry's loc is zeroed; the log and the item-start ring stay). `image`: the pattern image
  // write_keyed_prefix_image() made of the prefix (keyed_prefix_image_bytes(plen) bytes,
  // 16-byte aligned, device-readable: device or mapped pinned memory); 1 <= plen <= 65535
  // (an empty prefix is flush()). `out` (device or mapped pinned memory, 2 words) receives
  // {entries removed, their item bytes}; the removed entries are also counted as `purged`.
  // Asynchronous and ordered on `s` like remove(): no allocation, no synchronisation (one
  // purge at a time per shard: the result is accumulated in the shard's scratch words).
  // Dead entries (empty, locked, expired, overwritten) are neither read nor removed nor
  // counted. Defined for keyed values only: on other values it is memory-safe and removes
  // whatever happens to parse as a matching keyed record.
  void remove_keyed_prefix(const uint8_t* image, uint32_t plen, uint32_t now, uint64_t* out,
                           hipStream_t s);
  // Soft purge of keyed values: every live entry whose stored key starts with the pattern
  // (`exact`: equals it) gets flags = stale_at and, where expire_cap != 0 and the entry never
  // expires or expires after it, expire = expire_cap (a life is only shortened) — in place,
  // in the index entry and the record's ItemHeader; the value, loc, vlen and the CLOCK
  // reference bit stay, and so do the ring and the head. `image`, `plen`, the streams and the
  // memory kinds are remove_keyed_prefix's; expire_cap is 0 or > now. `out` (1 word) receives
  // the number of live matching entries, whether or not their words changed. Uses scratch
  // words of its own (one soft purge at a time per shard). Exact when ordered against whole
  // SET chains; refused while a phase-1 batch waits for its phase 2, as touch(). See
  // k_keyed_scan (SoftenAction) for what holds beside a SET chain on another stream.
  void soften_keyed_prefix(const uint8_t* image, uint32_t plen, bool exact, uint32_t stale_at,
                           uint32_t expire_cap, uint32_t now, uint64_t* out, hipStream_t s);
  // Tag purge of keyed values: removes every live entry whose stored value carries, at value
  // byte 2 + klen, a tag block (keyed.h) holding one of tags[0..ntags), 1 <= ntags <= 64, or
  // the overflow block. `tags` holds u64 tag hashes, 8-byte aligned, in device or mapped host
  // memory, and stays valid until the stream has run the call; everything else (`out`'s two
  // words, the `purged` counter, the streams, what holds beside appends) is
  // remove_keyed_prefix's. Uses scratch words of its own.
  void remove_keyed_tags(const uint64_t* tags, uint32_t ntags, uint32_t now, uint64_t* out,
                         hipStream_t s);
  // Soft tag purge: remove_keyed_tags' matcher, soften_keyed_prefix's action, result word and
  // checks (the cap lies after now; refused while a phase-1 batch waits for its phase 2).
  void soften_keyed_tags(const uint64_t* tags, uint32_t ntags, uint32_t stale_at,
                         uint32_t expire_cap, uint32_t now, uint64_t* out, hipStream_t s);
  // Glob purge of keyed values: removes every live entry whose stored key, up to its first
  // kVarySep byte, matches the compiled pattern (keyed.h: '*' wildcards, anchored at both
  // ends). `image`: the KeyedGlob compile_keyed_glob() wrote, `image_bytes` =
  // keyed_glob_used_bytes() of it, 16-byte aligned, in device or mapped host memory, valid
  // until the stream has run the call; everything else (`out`'s two words, the `purged`
  // counter, the streams, what holds beside appends) is remove_keyed_prefix's. Uses scratch
  // words of its own.
  void remove_keyed_glob(const uint8_t* image, uint32_t image_bytes, uint32_t now, uint64_t* out,
                         hipStream_t s);
  // Soft glob purge: remove_keyed_glob's matcher, soften_keyed_prefix's action, result word and
  // checks (the cap lies after now; refused while a phase-1 batch waits for its phase 2).
  void soften_keyed_glob(const uint8_t* image, uint32_t image_bytes, uint32_t stale_at,
                         uint32_t expire_cap, uint32_t now, uint64_t* out, hipStream_t s);
  // List keyed values, read-only: finds every live entry whose stored keyed value matches,
  // counts them and their item bytes over the whole index, and writes the first `limit` of them
  // at slots >= start_slot, in index-slot order, as one ListRow (keyed.h) and one key area each
  // (row r's: keys + r * key_cap, the head of the stored image [u16 klen | key ...], at most
  // key_cap bytes; bytes of the area past the key's granules are left as they are). `mode`:
  // kListPrefix (`image`, `plen`, `exact` as soften_keyed_prefix's), kListTags (`tags`, `ntags`
  // as remove_keyed_tags'), kListGlob (`image`: the compiled pattern, `plen`: its bytes in
  // use, both as remove_keyed_glob's) or kListAll (every plausible keyed value: 1 <= klen, 2 +
  // klen <= vlen; an empty key names no object). limit <= kMaxListRows (0: count only, no row is
  // written and next = nslots); key_cap a multiple of 16 in 16..1024; start_slot <= nslots. `out` (kListWords words) receives
  // {matched, their item bytes, rows listed, next}: next is the slot after the last listed row
  // when further matches follow it (the next page's start_slot), else nslots. `rows`, `keys`
  // and `out` are device or mapped pinned memory. Asynchronous and ordered on `s` like
  // remove_keyed_prefix; the match bitmap and tile counts are a workspace allocated on the
  // first call (that call allocates), and with the scratch words they make it one listing at
  // a time per shard. It writes nothing in the index or the log, counts in no CacheCounters
  // field, and is not refused while a phase-1 batch is pending. See k_list_scan for what holds
  // beside a SET chain on another stream (rows may come back flagged kListChanged).
  void list_keyed(uint32_t mode, const uint8_t* image, uint32_t plen, bool exact,
                  const uint64_t* tags, uint32_t ntags, uint64_t start_slot, uint32_t limit,
                  uint32_t key_cap, uint32_t now, ListRow* rows, uint8_t* keys, uint64_t* out,
                  hipStream_t s);
  // Sliced GET (slice.h): row i asks for the window spec[i] of the keyed value stored under
  // keys[i] with exactly the key key_bytes[key_offs[i] .. key_offs[i + 1]) (touch()'s packed
  // layout; required). rows[i] says what was found (kSliceMiss: no live entry, or another
  // key's record) and where the row's bytes start in `out`: the value's first head_bytes bytes
  // (through the end of its HTTP head, rounded up to a granule), then the 16-byte granules of
  // the value that cover the window. A value that is not a sliceable HTTP response, and a
  // kSliceWhole row, come back whole (kSliceWholeObj). res = {rows that hit, total bytes of
  // `out`}; when the total exceeds out_cap nothing is written to `out`, and `rows` and `res`
  // are still complete (gather's contract). n <= kSmallGetMax. Hits set the CLOCK reference
  // bit and count in get_ops / get_hits / get_bytes (the bytes returned: the value through its
  // head's end plus the window, or the whole value) as a GET's. `reserve` as lookup()'s.
  // All arrays are device or mapped pinned memory. Asynchronous and ordered on `s`; the
  // segment lists, the scan's scratch and the result words are one workspace per shard,
  // allocated on the first call (that call allocates): a call on another stream than the one
  // before waits, on the device, for that one's event, so calls on several streams are safe
  // and run one after the other. See k_slice_plan for what holds beside a SET chain on
  // another stream.
  // `cond` (nullable; device or mapped pinned memory, as `cond_bytes`): one SliceCond per row
  // (conditional.h), decided on the GPU against the stored head by k_slice_plan: a matched
  // none_match / modified_since row returns the head alone under kSliceNotModified, an
  // unmatched if_range_* row the whole value. Without it the call launches
  // the kernel instance without condition arguments, exactly what it launched before.
  void get_keyed_slices(const Digest* keys, const uint8_t* key_bytes, const int64_t* key_offs,
                        const SliceSpec* spec, int64_t n, SliceRow* rows, uint8_t* out,
                        uint64_t out_cap, uint64_t* res, uint32_t now, hipStream_t s,
                        uint64_t reserve = 0, const SliceCond* cond = nullptr,
                        const uint8_t* cond_bytes = nullptr);
  // TOUCH a batch: row i's live entry gets the absolute expiry expire[i] (0 = never) and,
  // with `flags` (nullable), the flags flags[i] — in place, in the index entry and in the
  // record's ItemHeader (the CLOCK hand and the backends read the header); no value byte
  // moves. hit[i] = 1 iff a live entry matched and was updated (counted as `touched`).
  // `key_bytes` + `key_offs` (nullable together; the packed layout of digest_keys: key i =
  // key_bytes[key_offs[i] .. key_offs[i + 1])): the row only matches a record whose stored
  // keyed value ([u16 klen | key | payload], keyed.h) carries exactly that key, so a digest
  // collision cannot change another object's life. Without them the digest decides. Either
  // way the record must be the entry's own (digest, vlen, magic), else the row is a miss.
  // Empty, locked, expired, overwritten and deleted entries are misses and stay as they are;
  // an expiry that is non-zero and <= now kills the object (and is a hit). Rows that repeat
  // a digest: which one wins is unspecified.
  // All arrays are device pointers or mapped pinned memory. Asynchronous and ordered on `s`
  // like remove(): no allocation, no synchronisation. Exact when ordered against whole SET
  // chains (StoreOpts::phase == 0); refused while a phase-1 batch waits for its phase 2 (a
  // detached hand's move rewrites the expiry it staged). See k_touch for what holds beside a
  // SET chain on another stream.
  void touch(const Digest* keys, const uint32_t* expire, const uint32_t* flags,
             const uint8_t* key_bytes, const int64_t* key_offs, int64_t n, uint8_t* hit,
             uint32_t now, hipStream_t s);
  // Reclaim index slots whose items expired or were overwritten. Synchronises;
  // returns {live entries, live item bytes}.
  void sweep(uint32_t now, hipStream_t s, uint64_t* live_entries, uint64_t* live_bytes);
  // Digests of every live entry -> out (device, up to out_cap); returns the live
  // count (may exceed out_cap). Synchronises. Used for rebalancing / migration.
  uint64_t export_keys(Digest* out, uint64_t out_cap, uint32_t now, hipStream_t s);
  // Snapshot / warm restore of the whole shard (index + log + head) to a file;
  // `user` carries 4 caller words (e.g. the epoch). load() needs equal geometry.
  void save(const std::string& path, const uint64_t user[4], hipStream_t s);
  void load(const std::string& path, uint64_t user[4], hipStream_t s);
  // Drop everything (memcached FLUSH).
  void flush(hipStream_t s);
  // Tests: read / overwrite one index bucket (4 entries of {d0, d1, loc, vlen | expire
  // << 32}), synchronously. Builds index states no API call produces in a fixed order
  // (e.g. a dead same-digest entry in a key's first bucket beside its live one).
  std::vector<uint64_t> debug_bucket(uint64_t b);
  // {hand (ring index), ring tail, head, the log offset of the hand's item (~0: none), entries
  // the hand consumed last batch, the effective windows of hand buffers 0 and 1}
  std::vector<uint64_t> debug_hand();
  void debug_set_entry(uint64_t b, int slot, uint64_t d0, uint64_t d1, uint64_t loc,
                       uint32_t vlen, uint32_t expire);
  // Tests: move the CLOCK hand to ring index `hand` (e.g. a lap behind the overwrite), and
  // whether the hand may jump to the first entry the overwrite has not reached
  // (hand_catch_up; false isolates it: a hand left behind then spends its windows on
  // overwritten entries).
  void debug_set_hand(uint64_t hand, bool catch_up = true);
  CacheCounters counters(hipStream_t s);
  uint64_t head(hipStream_t s);

  const ShardConfig& config() const { return cfg_; }
  uint8_t* log_ptr() const { return log_; }
  Entry* index_ptr() const { return index_; }
  uint64_t* head_ptr() const { return head_ + hsel_; }
  // Pre-size the SET workspace for batches of n keys, and with CLOCK the hand's workspaces
  // for the combined batch such a SET runs once the log wraps (allocates; synchronises;
  // call outside capture and before serving).
  void reserve(int64_t n);
  // Bytes of grown-out workspaces not freed yet (their chains still running); frees the
  // ones whose chains have finished first.
  uint64_t retired_bytes();
  uint64_t retired_ever() const { return retired_ever_; }  // bytes ever retired (tests)
  uint64_t hbm_bytes() const;
  uint64_t reinsert_max() const { return cfg_.evict == kEvictClock ? rmax_ : 0; }

 private:
  void ensure_set_ws(int64_t n, hipStream_t s);
  void ensure_rc_ws(int64_t w, hipStream_t s);
  void ensure_cb(int b, int64_t rows, hipStream_t s);
  bool should_reclaim(uint64_t bytes_bound) const;
  uint64_t* cur_ring_tail() const { return head_ + 2 + hsel_; }
  uint64_t* next_ring_tail() const { return head_ + 2 + (hsel_ ^ 1); }
  // Deferred frees (no device-wide synchronisation on the serving path): a grown buffer's
  // old blocks are retired as a group with one event recorded on the growing call's stream
  // after it has waited for the last store queued on every other stream SET work used
  // (`note_stream`; each store records its stream's `last` event when it returns, so no
  // call ever records on a stream the caller may since have destroyed); reap_retired frees
  // a group once its event has completed (every chain that could read the old blocks has
  // finished) — at the start of every store and in sweep; reserve (which synchronises the
  // device) and the destructor free every group.
  struct RetiredGroup {
    std::vector<void*> ptrs;
    std::vector<hipEvent_t> ev;
    uint64_t bytes = 0;
  };
  // One buffer of a growable set: where its pointer lives and its bytes at a capacity of
  // the set. A set's table (set_bufs, hand_bufs, rc_bufs) is its only list: growth, the
  // retired-bytes figure and the destructor all walk it.
  struct Buf {
    void** p;
    uint64_t (*bytes)(uint64_t cap);
  };
  using BufSet = std::vector<Buf>;
  // Retires the set's blocks of capacity `old_cap` (if any), then allocates `cap`.
  void grow_bufs(const BufSet& set, int64_t old_cap, int64_t cap, hipStream_t s);
  void retire_group(const BufSet& set, int64_t cap, hipStream_t s);
  void reap_retired(bool all);
  void note_stream(hipStream_t s);
  void note_store_end(hipStream_t s);
  std::vector<RetiredGroup> retired_;
  uint64_t retired_ever_ = 0;
  struct SetStream {
    hipStream_t s = nullptr;
    hipEvent_t last = nullptr;  // recorded after the last store queued on s
  };
  std::vector<SetStream> set_streams_;
  // The SET workspace's tables are cleared on the stream of the call that grew them;
  // a store on another stream waits for that (ws_ready_) once (ws_ordered_).
  hipEvent_t ws_ready_ = nullptr;
  hipStream_t ws_grow_stream_ = nullptr;
  std::vector<hipStream_t> ws_ordered_;
  void ws_order(hipStream_t s);
  // CLOCK state
  uint64_t* ring_ = nullptr;           // item-start ring (logical locs, kRingSkip holes)
  uint64_t ring_cap_ = 0;
  unsigned long long* rc_ctl_ = nullptr;  // hand, batch bytes, cut, entries scanned
  bool lead_ = false;  // the hand's mode (layout.h hand_lead, sticky; HostCache keeps the same)
  bool catch_up_ = true;  // debug_set_hand
  uint64_t rmax_ = 0;
  int64_t rc_cap_ = 0;
  uint64_t *rc_loc_ = nullptr, *rc_h_ = nullptr, *rc_part_ = nullptr, *rc_hx_ = nullptr;
  BufSet rc_bufs();
  // A batch between its planning and its tail (append, index insert): the rows the chain
  // runs on and the buffers it planned into. A batch with a hand is the combined one:
  // `nmove` reinsertion rows (moves), then the caller's `n`, all in hand buffer `hand`.
  struct Pending {
    const Digest* keys = nullptr;
    const uint8_t* values = nullptr;
    const uint64_t* voff = nullptr;
    const uint32_t *vlen = nullptr, *flags = nullptr, *expire = nullptr;
    int64_t n = 0, rows = 0;       // caller rows; rows of the (combined) batch
    const uint64_t* from = nullptr;
    int64_t nmove = 0;
    int ws = 0;                    // its SET workspace (ws_)
    int hand = -1;                 // its hand buffer (hb_), -1: the hand did not run
    bool active = false;           // pend_ only: a phase 1 waits for its phase 2
  };
  // store(phase=1) queued a batch's CLOCK hand and planning; store(phase=2) runs the rest
  // of its chain from this record
  Pending pend_;
  // The combined SET batch (reinsertion rows, then the batch's own rows) and the staged
  // reinsertion records, two buffers taken in turn (a detached hand fills one while the
  // previous batch's chain still reads the other). `from`: a reinsertion row's old entry
  // loc (a move), 0 for the batch's rows.
  struct HandBuf {
    Digest* keys = nullptr;
    uint64_t* voff = nullptr;
    uint64_t* from = nullptr;
    uint32_t *vlen = nullptr, *flags = nullptr, *expire = nullptr;
    int64_t cap = 0;
    uint8_t* scratch = nullptr;  // staged reinsertions (rmax_ + 64 bytes)
  };
  HandBuf hb_[2];
  static BufSet hand_bufs(HandBuf& h);  // (not `scratch`: fixed size, freed with the cache)
  // SET workspaces, two taken in turn by consecutive batches (ws_next_): a batch's planning
  // (phase 1) may run while the previous batch's append and index insert still use theirs.
  // A graph (store_graph) bakes its workspace in: always the first.
  struct SetWs {
    uint32_t* dd_tab = nullptr;   // dedupe table: 0 = empty, else the key's last row + 1
    uint32_t* dd_slot = nullptr;
    uint64_t *set_size = nullptr, *set_off = nullptr;
    uint32_t* set_claim = nullptr;  // entry each SET row claimed (k_set_fixup)
    uint64_t* set_cnt = nullptr;    // ring ordinal of each stored SET row (CLOCK)
  };
  SetWs ws_[2];
  int ws_next_ = 0;
  static BufSet set_bufs(SetWs& w);

  ShardConfig cfg_;
  uint8_t* log_ = nullptr;
  Entry* index_ = nullptr;
  uint64_t* head_ = nullptr;         // device: logical write head, 2 ping-pong slots
  int hsel_ = 0;                     // slot holding the current head
  uint64_t* cur_head() const { return head_ + hsel_; }
  // furthest log byte any queued SET append will write (monotone; set before the append)
  uint64_t* claim_ptr() const { return head_ + 4; }
  uint64_t* next_head() const { return head_ + (hsel_ ^ 1); }
  CacheCounters* ctr_ = nullptr;     // device counters (64 shards)
  unsigned long long* scratch_ = nullptr;  // device scratch for reductions
  // Its words, a 16-B block of its own per operation: the results of different operations
  // queued on a shard do not meet (one call at a time per operation and shard).
  enum ScratchWord : int {
    kScratchSweep = 0,  // sweep: live entries, live bytes; export_keys: the rows written
    kScratchPurgePrefix = 4,
    kScratchSoftenPrefix = 6,
    kScratchPurgeTags = 8,
    kScratchSoftenTags = 10,
    kScratchList = 12,  // kListWords words
    kScratchPurgeGlob = 16,
    kScratchSoftenGlob = 18,
    kScratchWords = 20
  };
  // The launch of k_keyed_scan<Matcher, Action> over the whole index: the result words at
  // `word` cleared, the scan, its Action::kWords result words copied to `out`, all on `s`.
  template <class Matcher, class Action>
  void keyed_scan(const Matcher& m, const Action& act, uint32_t now, ScratchWord word,
                  uint64_t* out, hipStream_t s);
  uint8_t* list_ws_ = nullptr;       // list_keyed: match bitmap, tile counts and bases
  // get_keyed_slices: result words, segment sources, lengths, offsets, the scan's scratch
  uint8_t* slice_ws_ = nullptr;
  size_t slice_tmp_bytes_ = 0;
  // recorded behind each call on its stream: the workspace's next user on another stream waits
  hipEvent_t slice_done_ = nullptr;
  hipStream_t slice_stream_ = nullptr;
  uint64_t* part_ = nullptr;         // per-workgroup sums: GET sizes, SET sizes, SET counts
  uint64_t* host_buf_ = nullptr;     // pinned scratch for small D2H reads
  uint64_t* host_slots_ = nullptr;   // pinned coherent slots the GPU writes totals into
  // persistent edge-GET server (serve_get): job ring + control words in pinned coherent
  // memory, its own CU-masked stream (a queue of its own: nothing queues behind it)
  void* srv_ring_ = nullptr;
  uint64_t* srv_ctl_ = nullptr;      // [8] exited epoch, [16] stop, [24 + 8 b] block b's consumed
  uint64_t* srv_sync_ = nullptr;     // device: the server blocks' shared idle clock, exit count
  int srv_blocks_ = 1;
  hipStream_t srv_stream_ = nullptr;
  uint64_t srv_ticket_ = 0, srv_epoch_ = 0, srv_launches_ = 0;
  uint64_t srv_idle_ticks_ = 0, srv_life_ticks_ = 0, srv_khz_ = 0;
  uint64_t* srv_trace_ = nullptr;    // pinned: per-job phase stamps (serve_trace)
  bool srv_running_ = false;
  std::mutex srv_mu_;
  void serve_launch_locked();
  unsigned int* done_ctr_ = nullptr; // device: edge-GET workgroups finished + fail flag (self-resetting)
  unsigned long long* lb_state_ = nullptr;  // device: edge-GET look-back words (self-resetting)
  // SET workspaces (ws_): rows either holds, and the mask of their dedupe tables
  int64_t set_cap_ = 0;
  uint32_t dd_mask_ = 0;
  uint64_t ws_gen_ = 0;  // bumped when the SET workspace moves (invalidates graphs)
  std::mutex mu_;
  // The SET chain, one for every caller (store in each phase, store_graph's capture):
  // reclaim_locked (the CLOCK hand, turning the caller's batch into the combined one), then
  // store_plan_locked (dedupe, sizes, offsets), then store_tail_locked (log append, then
  // store_index_locked: index insert and fix-up). `done` (store's; null, or pointing at
  // null: none) is taken by the launch that carries it.
  Pending reclaim_locked(const Pending& own, int64_t w, uint64_t rmax, uint32_t now,
                         hipStream_t s, bool detached);
  void store_plan_locked(const Pending& p, hipStream_t s, bool detached);
  void store_tail_locked(const Pending& p, uint32_t now, hipStream_t s, const StoreOpts& o,
                         hipEvent_t* done);
  void store_index_locked(const Pending& p, uint32_t now, hipStream_t s,
                          hipEvent_t index_after, hipEvent_t* done);
};

// ---- Generic device kernels used by the distributed serving path ----------------

// Exclusive scan of in[0..n) into out[0..n] (out[n] = total), u64.
void device_exclusive_scan(const uint64_t* in, uint64_t* out, int64_t n, void* tmp,
                           size_t tmp_bytes, hipStream_t s);
size_t device_scan_tmp_bytes(int64_t n);

// Load-balanced segmented copy: segment i copies (dst_off[i+1]-dst_off[i]) bytes
// from src + src_off[i] to dst + dst_off[i]. All offsets/lengths multiples of 16.
// src_off[i] == kSegSkip: segment i is a gap (nothing read or written).
constexpr uint64_t kSegSkip = ~0ull;
void segcopy(const uint8_t* src, const uint64_t* src_off, const uint64_t* dst_off, int64_t n,
             uint8_t* dst, hipStream_t s, uint64_t dst_cap = ~0ull);
// Device-count variant (absolute source addresses in src_off): the number of segments is
// *n_dev, read by the kernel, so a segment list the GPU built needs no host read.
void segcopy_dev(const uint64_t* src_off, const uint64_t* dst_off, const int64_t* n_dev,
                 uint8_t* dst, hipStream_t s, uint64_t dst_cap = ~0ull);
// Sized variant: segment i holds seg_len[i] bytes at dst + dst_off[i] (dst_off ascending,
// gaps allowed and left untouched, dst_off[n] = the extent); a segment that does not end
// within `cap` is dropped (the others still land). Offsets / lengths multiples of 16.
void segcopy_sized(const uint8_t* src, const uint64_t* src_off, const uint64_t* dst_off,
                   const uint64_t* seg_len, int64_t n, uint8_t* dst, hipStream_t s,
                   uint64_t cap = ~0ull);
// What the byte mover's partition is made of, for tests that must reach a given path:
// the minimum tile (16-B chunks), the segments staged per pass (modes 0/1/3/4, mode 2, the
// LDS-DMA variant), whether this process runs the LDS-DMA variant (SHELLAC_GLDS), and the
// workgroups each mode is launched with on the current device.
struct SegcopyGeometry {
  int min_tile = 0;
  int stage = 0, stage_sized = 0, stage_glds = 0;
  bool glds = false;
  int grid[5] = {0, 0, 0, 0, 0};
};
SegcopyGeometry segcopy_geometry();

// GET coalescing: first[i] = the row that serves row i (one row per distinct digest
// serves all its duplicates). `table` is scratch of coalesce_table_slots(n) u32 words.
int64_t coalesce_table_slots(int64_t n);
void coalesce_keys(const Digest* keys, int64_t n, uint32_t* table, int64_t table_slots,
                   uint32_t* first, hipStream_t s, uint32_t* cslot = nullptr,
                   bool table_clean = false);
// After the gather of a coalesced lookup: size[i], off[i] of every duplicate row i :=
// those of first[i] (in place), so each request addresses its claimer's record.
void expand_coalesced(const uint32_t* first, int64_t n, uint64_t* size, uint64_t* off,
                      hipStream_t s);

// Out-of-place variant (may overlap the gather): out_size/out_off[i] := size/off of
// first[i] for every row; claimers clear their table slot (cslot from lookup_coalesced)
// so the table is clean for the next batch.
void expand_coalesced_out(const uint32_t* first, int64_t n, const uint64_t* size,
                          const uint64_t* off, uint64_t* out_size, uint64_t* out_off,
                          uint32_t* table, const uint32_t* cslot, hipStream_t s);

// GET records -> a SET batch (shard migration over xGMI: records gathered on one GPU,
// peer-copied to another, stored there). Row i's record is rec[off[i] .. +size[i]]
// (size 0 = miss); a row whose `have_size[i]` (the destination's own lookup, may be null)
// is non-zero is skipped — insert-if-absent, so a migration never overwrites an object
// the destination has stored since. Outputs: vlen = kSkipVlen for skipped rows.
void records_to_set(const uint8_t* rec, const uint64_t* off, const uint64_t* size,
                    const uint64_t* have_size, int64_t n, Digest* keys, uint64_t* val_off,
                    uint32_t* vlen, uint32_t* flags, uint32_t* expire, hipStream_t s);

// Digest packed key bytes: key i = bytes[offs[i] .. offs[i+1]).
void digest_keys(const uint8_t* bytes, const int64_t* offs, int64_t n, Digest* out,
                 hipStream_t s);

// Consistent-hash routing: dest[i] = owner of the first ring point >= ring_position(keys[i])
// (wrapping), counts[r] += #keys routed to r. `counts` must be zeroed by the caller.
void route_keys(const Digest* keys, int64_t n, const uint32_t* ring_pts, const int32_t* ring_owner,
                int32_t npts, int32_t* dest, int64_t* counts, int32_t nranks, hipStream_t s);

// Stable-within-wave scatter of records by destination: pos = base[dest[i]] + rank,
// perm[i] = pos, out[pos] = in[i] for `rec_bytes`-byte records (16 or 32-multiple of 4).
void scatter_by_dest(const int32_t* dest, const int64_t* base, int64_t n, int32_t nranks,
                     int64_t* cursor, int64_t* perm, hipStream_t s);
void permute_records(const void* in, const int64_t* perm, int64_t n, int32_t rec_bytes, void* out,
                     hipStream_t s);

// MFMA smoke kernel (BASELINE.json platform check): C[32x32] = A[32x16] * B[16x32],
// bf16 inputs, fp32 accumulate, one v_mfma_f32_32x32x16_bf16 per wave.
void mfma_hello(const uint16_t* a, const uint16_t* b, float* c, int tiles, hipStream_t s);

}  // namespace shellac
