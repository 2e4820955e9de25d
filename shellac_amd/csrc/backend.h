// Cache backends behind the proxy and the memcached-protocol shard server.
//
// The reference has exactly one: a blocking pylibmc client doing one TCP round
// trip per request inside the reactor (src/python/shellac/server/Server.py:335
// get, :432 set). Here every backend is asynchronous (completions are posted to
// the calling reactor's Executor), so a slow cache never stalls the event loop:
//
//   DramBackend       striped host-DRAM shards (csrc/host_cache.cc), synchronous
//                     fast path, no GPU needed;
//   HbmBackend        one HBM shard per local MI355X (csrc/hbm_cache.hip), fed by a
//                     batcher thread that coalesces the GETs/SETs of all reactors
//                     into one kernel pipeline per GPU per tick (csrc/backend_hbm.cc the
//                     request API and routing, hbm_batcher.cc the batcher, hbm_direct.cc
//                     reactor-direct GETs, hbm_hot.cc hot-object spreading; their shared
//                     types in hbm_backend_impl.h, host-only decisions in hbm_flight_plan.h);
//   MemcachedBackend  memcached binary protocol over TCP to remote nodes (real
//                     memcached or `shellac-cached`), ketama-routed, pipelined on
//                     persistent connections, with node ejection + retry.
#pragma once

#include <cstdlib>

#include <atomic>
#include <condition_variable>
#include <deque>
#include <functional>
#include <memory>
#include <mutex>
#include <shared_mutex>
#include <string>
#include <thread>
#include <unordered_map>
#include <vector>

#include "digest.h"
#include "inspect.h"
#include "host_cache.h"
#include "host_router.h"
#include "ketama.h"
#include "net.h"
#include "object_cache.h"
#include "presence_filter.h"
#include "conditional.h"
#include "slice.h"
#include "stream_buf.h"

namespace shellac {

class HbmCache;

class Executor {
 public:
  virtual ~Executor() = default;
  virtual void post(std::function<void()> fn) = 0;  // run fn on the executor's thread
  // Several completions at once (one lock and one wake-up for a whole GPU batch).
  virtual void post_batch(std::vector<std::function<void()>>& fns) {
    for (auto& f : fns) post(std::move(f));
    fns.clear();
  }
};

struct CacheValue {
  Bytes data;
  uint32_t flags = 0;
  int64_t ttl_left = -1;  // seconds of life left: -1 unknown, 0 never expires
};
using GetCallback = std::function<void(bool hit, CacheValue v)>;
// The answer of a sliced GET (slice.h): part of one stored HTTP response.
struct PartValue {
  // kSliceMiss / kSliceOk / kSliceUnsat / kSliceWholeObj / kSliceNotModified (get_part_if)
  uint32_t status = kSliceMiss;
  Bytes head;    // all but miss and whole: the payload from "HTTP/" through the blank line
  Bytes window;  // the window's bytes; kSliceWholeObj: the whole value, as get() returns it
  uint64_t body_len = 0, first = 0;
  uint32_t flags = 0;
  int64_t ttl_left = -1;  // as CacheValue's
};
using PartCallback = std::function<void(PartValue v)>;
// A whole value, as get() answered it, sliced on the host: what every tier without a sliced
// GET of its own answers, and what a tier that cuts on the GPU must equal.
PartValue slice_cache_value(bool hit, CacheValue v, const SliceSpec& spec);
// The condition of a conditional sliced GET (conditional.h): a kind and its candidate records,
// what parse_if_none_match / parse_if_modified_since / parse_if_range give.
using PartCond = CondRequest;
// slice_cache_value under a condition, decided on the host with conditional.h's functions: a
// matched none_match / modified_since answers the head alone under kSliceNotModified, an
// unmatched if_range_* the whole value.
PartValue slice_cache_value_if(bool hit, CacheValue v, const SliceSpec& spec, const PartCond& cond);
using DelCallback = std::function<void(bool found)>;
// Purge: objects removed or softened, or -1 if the tier cannot scan its keys.
using PurgeCallback = std::function<void(int64_t removed)>;
// In-place touch: 1 touched, 0 not found, -1 the tier cannot do it.
using TouchCallback = std::function<void(int status)>;
// Listing (inspect.h): the answer, ok == false where the tier cannot scan its keys.
using ListCallback = std::function<void(ListResult)>;
using StatList = std::vector<std::pair<std::string, uint64_t>>;

// Asynchronous body compressor for the proxy's -z path: `done` runs on the compressor's
// thread (callers post back to their reactor) with ok = false and the original body when
// compression failed. The GPU implementation is GzipService (deflate.h); the proxy
// itself only sees this interface, so it builds without the HIP runtime.
class Compressor {
 public:
  using Done = std::function<void(bool ok, std::string out)>;
  virtual ~Compressor() = default;
  virtual void submit(std::string body, Done done) = 0;
  // gunzip one member off the caller's thread (output capped at max_out bytes); engines
  // without it return false from can_inflate() and the caller decodes inline
  virtual bool can_inflate() const { return false; }
  virtual void submit_inflate(std::string member, uint64_t max_out, Done done) {
    (void)max_out;
    done(false, std::move(member));
  }
  virtual void stats(StatList* out) = 0;
};

class CacheBackend {
 public:
  virtual ~CacheBackend() = default;
  // `done` runs on `ex`'s thread (inline for synchronous backends).
  virtual void get(const std::string& key, const Digest& d, Executor* ex, GetCallback done) = 0;
  // Sliced GET: the head and one byte window (`spec`, slice.h) of the HTTP response stored
  // under `key`; a value that is no sliceable HTTP response, and a kSliceWhole spec, come back
  // whole (kSliceWholeObj). Ordered and answered as get(). The default gets the whole value
  // and cuts it on the host; HbmBackend cuts on the GPU and moves only the part.
  virtual void get_part(const std::string& key, const Digest& d, const SliceSpec& spec,
                        Executor* ex, PartCallback done) {
    get(key, d, ex, [spec, done = std::move(done)](bool hit, CacheValue v) {
      done(slice_cache_value(hit, std::move(v), spec));
    });
  }
  // Conditional sliced GET: get_part with the client's validators (`cond`), compared with the
  // stored ETag / Last-Modified where the object lies, so one trip answers "not modified" (the
  // head alone, kSliceNotModified), the window, or the whole object. The default gets the whole
  // value and decides and cuts it on the host; HbmBackend decides on the GPU.
  virtual void get_part_if(const std::string& key, const Digest& d, const SliceSpec& spec,
                           const PartCond& cond, Executor* ex, PartCallback done) {
    get(key, d, ex, [spec, cond, done = std::move(done)](bool hit, CacheValue v) {
      done(slice_cache_value_if(hit, std::move(v), spec, cond));
    });
  }
  virtual void set(const std::string& key, const Digest& d, Bytes value, uint32_t flags,
                   uint32_t ttl_s) = 0;
  virtual void del(const std::string& key, const Digest& d, Executor* ex, DelCallback done) = 0;
  // Invalidation (selector.h): carry out `how` on every live object `what` selects: remove it,
  // or (soft) keep it and make it stale. `done` runs once, on `ex`'s thread (inline for
  // synchronous backends), with the number of objects removed, or of live matching objects
  // softened (whether or not their words changed), or -1 where the tier cannot do it (the
  // default: a tier that cannot enumerate its keys, e.g. memcached) and for what every tier
  // refuses (purge_refused: a refused selector, everything, the removal of one key). Objects
  // stored before the call are gone, or stale, when `done` runs; GETs racing the purge may
  // still hit until then.
  virtual void purge(const KeyedSelector& what, const PurgeAction& how, Executor* ex,
                     PurgeCallback done) {
    (void)what;
    (void)how;
    if (!done) return;
    if (ex) ex->post([done] { done(-1); });
    else done(-1);
  }
  // Inspection, read-only: the live objects q.what selects; how many they are and their bytes
  // (per stored copy, as a purge's count), and up to q.limit of them after the cursor q.after,
  // in an order of the tier's own that a cursor pages through exactly (`next`; empty: the
  // end). `done` runs once, on `ex`'s thread (inline for synchronous backends). ok == false:
  // the tier cannot scan its keys (the default), or the query is out of range.
  virtual void list_objects(const ListQuery& q, Executor* ex, ListCallback done) {
    (void)q;
    if (!done) return;
    if (ex) ex->post([done] { done(ListResult{}); });
    else done(ListResult{});
  }
  // Touch: give the live object of exactly `key` the TTL `ttl_s` from now (0 = never expires)
  // and, when `flags` is not null (read before the call returns), new flags, without moving
  // its bytes. A write: ordered with
  // the SETs and DELETEs of the key issued before and after it. `done` runs once, on `ex`'s
  // thread (inline for synchronous backends): 1 touched, 0 no such live object, -1 where the
  // tier cannot do it (the default; memcached's wire TOUCH cannot change flags) — the caller
  // then re-stores the object.
  virtual void touch(const std::string& key, const Digest& d, uint32_t ttl_s,
                     const uint32_t* flags, Executor* ex, TouchCallback done) {
    (void)key;
    (void)d;
    (void)ttl_s;
    (void)flags;
    if (!done) return;
    if (ex) ex->post([done] { done(-1); });
    else done(-1);
  }
  virtual void flush() = 0;
  virtual std::string name() const = 0;
  virtual void stats(StatList* out) = 0;
  // Fault injection / drills: take GPU shard `shard` of this tier out of service (or
  // bring it back). Returns false if the tier has no such shard.
  virtual bool inject_shard_down(int shard, bool down) {
    (void)shard;
    (void)down;
    return false;
  }
  // Reactor-direct submission (HbmBackend's edge server): a reactor thread attaches once
  // with itself as `ex`; its GETs may then be held by the tier and sent to the GPU from
  // the reactor's own loop by direct_service(), which also answers finished ones inline —
  // no batcher-thread hop either way. direct_service() returns true while jobs are
  // outstanding (the loop keeps polling instead of blocking); direct_detach() drains them
  // before the thread exits. Wrappers forward; other tiers ignore them.
  virtual void direct_attach(Executor* ex) { (void)ex; }
  virtual bool direct_service() { return false; }
  virtual void direct_detach() {}
  // Hot-object spreading (HbmBackend on several GPUs): re-plan the replicated hot set now;
  // returns the refresh's counts (empty: the tier has none). Wrappers forward.
  virtual StatList hot_refresh() { return {}; }
};

// 32-bit-point ring over digests, identical to shellac_amd.parallel.ring.ShardRing.
class DigestRing {
 public:
  explicit DigestRing(int nshards, int points_per_shard = 160);
  int owner(const Digest& d) const;
  // Owner among the shards whose bit is set in `alive` (ketama ejection: a dead shard's
  // keys move to the next live point); -1 if none is alive.
  int owner(const Digest& d, uint64_t alive) const;
  const std::vector<std::pair<uint32_t, int>>& points() const { return pts_; }

 private:
  std::vector<std::pair<uint32_t, int>> pts_;
};

// Host-DRAM tier: refcounted immutable objects (object_cache.h) — a hit is shared, not
// copied, and the full key is checked; CLOCK eviction by bytes.
class DramBackend : public CacheBackend {
 public:
  DramBackend(uint64_t bytes, uint32_t max_item, int stripes = 64);
  void get(const std::string& key, const Digest& d, Executor* ex, GetCallback done) override;
  void set(const std::string& key, const Digest& d, Bytes value, uint32_t flags,
           uint32_t ttl_s) override;
  void del(const std::string& key, const Digest& d, Executor* ex, DelCallback done) override;
  void purge(const KeyedSelector& what, const PurgeAction& how, Executor* ex,
             PurgeCallback done) override;
  void list_objects(const ListQuery& q, Executor* ex, ListCallback done) override;
  void touch(const std::string& key, const Digest& d, uint32_t ttl_s, const uint32_t* flags,
             Executor* ex, TouchCallback done) override;
  void flush() override;
  std::string name() const override { return "dram"; }
  void stats(StatList* out) override;
  uint32_t now() const;

 private:
  ObjectCache cache_;
  double epoch_;
};

struct HbmBackendConfig {
  std::vector<int> devices{0};
  uint64_t log_bytes_per_gpu = 8ull << 30;
  uint64_t nbuckets_per_gpu = 1ull << 22;
  uint32_t max_item = 1u << 20;
  int batch_us = 0;           // optional linger for batch-mates (0: natural batching)
  int max_batch = 65536;      // requests per batch at most
  int sweep_interval_s = 10;  // idle-time expiry sweep of every shard (0 = off)
  int spin_us = 50;           // a batcher polls its queue this long before blocking
  bool presence_filter = true;  // answer GETs of never-stored digests on the host
  int depth = 3;              // batches in flight per GPU (pinned staging per batch)
  int evict = 1;              // 0 FIFO, 1 CLOCK (ShardConfig::evict)
  int retry_s = 2;            // an ejected GPU shard is retried after this long
  int batch_timeout_ms = 2000;  // a batch unfinished this long ejects its GPU
  bool flush_on_restore = true;  // a shard back from ejection may hold stale objects
  // ...and is then warmed from its peers over xGMI: the objects of its key range that
  // other shards took while it was out are peer-copied back (hipMemcpyPeerAsync)
  bool warm_restore = true;
  // peer copies of the warm restore: "auto" = direct xGMI where hipDeviceCanAccessPeer
  // says so (peer access enabled at start), staged through pinned host memory otherwise;
  // "staged" forces the host path (tests; a node whose xGMI mapping is broken)
  std::string peer_copy = "auto";
  // Pinned response arenas allocated up front per GPU (depth + 2 of this size): pinning
  // host memory mid-run stalled every socket call on the box for up to ~0.5 s
  uint64_t arena_bytes = 16u << 20;
  // GET batches of at most HbmCache::kServeKeys distinct keys go to the GPU's persistent
  // edge server (HbmCache::serve_get: no launch per batch) unless a SET / DELETE of one
  // of their keys is still in flight; off: every batch is a launch on the stream
  bool edge_server = true;
  // server jobs that may be ahead of a batch sent to it: 2 = a batch waits behind at most
  // one job (~4-9 us) rather than take a launch (~15 us) — c=10 284K vs 252K RPS at 1
  // (profiles/archive/r3_http)
  int serve_backlog = 2;
  // resident edge-server blocks per GPU (ShardConfig::serve_blocks): jobs of different
  // submitters are served side by side; serve_backlog counts jobs per block
  int serve_blocks = 8;
  // CPUs the batcher threads run on (thread i on batcher_cpus[i % size]; empty: unpinned)
  std::vector<int> batcher_cpus;
  // Reactor-direct GETs (CacheBackend::direct_attach): an attached reactor writes its own
  // edge-server jobs (at most kServeKeys distinct keys, while fewer than direct_backlog
  // jobs are queued on the server) and polls their completion words in its loop; larger
  // or write-ordered batches still go through the batcher. Needs edge_server.
  bool direct = true;
  int direct_backlog = 4;
  uint64_t direct_arena_bytes = 1u << 20;  // pinned arenas reserved per GPU for them
  int direct_arenas = 32;
  // Hot-object spreading over the shards (more than one device, and
  // flush_on_restore: a restored shard must not keep replicas it missed writes for). The
  // `hot_objects` most requested objects of a sampled GET stream (one GET in `hot_sample`,
  // a power of two) are replicated on every shard: their SETs / DELETEs are written through
  // to every shard, their GETs go to a designated shard chosen to even out the load
  // (objects above `hot_spray_above` of the sampled GETs, default 1/(4N), are sprayed over
  // all shards). A refresh thread re-plans every `hot_refresh_ms` (0: only on request,
  // HbmBackend::hot_refresh) once `hot_min_samples` samples are in, and fetches the
  // records of newly hot objects from their owners over xGMI (at most hot_fill_budget
  // bytes per refresh, hottest first). 0 objects: plain ketama (every key on its owner).
  int hot_objects = 1024;
  int hot_refresh_ms = 1000;
  int hot_sample = 8;
  uint64_t hot_min_samples = 512;
  uint64_t hot_fill_budget = 256ull << 20;
  double hot_spray_above = 0;  // 0: 1 / (4 * shards)
};

// What an HbmBackend request asks of its shard's batcher. A flight runs its requests by kind,
// in this order: GETs, slices, SETs, DELETEs, touches, hot-replica fills, prefix purges (a barrier
// only reports that its flight has finished).
// A list is a control request of its own kind: it writes nothing, so it marks no fill, no
// shard purge_dirty and no purge generation; it is queued behind the writes queued before it
// and launched at the end of its flight, as a purge.
// A slice (get_part) is a read, planned and ordered as a GET: behind the earlier writes of its
// key, routed to a hot replica as a GET is; it goes through the batcher only.
enum class ReqKind : uint8_t { Get, Set, Del, Barrier, Fill, Purge, Touch, List, Slice };
// changes a key's object: ordered against the key's other requests, counted as pending
constexpr bool is_write(ReqKind k) {
  return k == ReqKind::Set || k == ReqKind::Del || k == ReqKind::Touch;
}
// names no key and answers through Req::ccb on the batcher thread
constexpr bool is_ctl(ReqKind k) {
  return k == ReqKind::Barrier || k == ReqKind::Fill || k == ReqKind::Purge ||
         k == ReqKind::List;
}

struct DigestHash {
  size_t operator()(const Digest& d) const { return (size_t)(d.lo ^ (d.hi * 0x9E3779B97F4A7C15ull)); }
};
struct DigestEq {
  bool operator()(const Digest& a, const Digest& b) const { return a.lo == b.lo && a.hi == b.hi; }
};

// One HBM shard per local MI355X. Each GPU has its own batcher thread: requests are
// routed to their shard's queue by the digest ring, and the batcher keeps up to `depth`
// batches in flight on its stream — GETs as one edge-GET launch that writes hits
// straight into a pinned arena (handed to the reactors as zero-copy ByteRef slices),
// SETs/DELETEs from pinned staging — reaping them in order as their completion slots /
// events fire. A batch that errors or stalls ejects its GPU from the ring (its keys
// fall through to the origin) until retry_s passes and the GPU proves healthy.
class HbmBackend : public CacheBackend {
 public:
  explicit HbmBackend(const HbmBackendConfig& cfg);
  ~HbmBackend() override;
  void get(const std::string& key, const Digest& d, Executor* ex, GetCallback done) override;
  // A ReqKind::Slice request, routed as a GET and never sent reactor-direct: a flight's slices
  // are one HbmCache::get_keyed_slices launch into a pinned arena, and the answer's head and
  // window are slices of that arena. A shard out of service is a miss.
  void get_part(const std::string& key, const Digest& d, const SliceSpec& spec, Executor* ex,
                PartCallback done) override;
  // The same request carrying its condition: the flight's launch then passes one SliceCond per
  // row and k_slice_plan decides each row on the GPU (counted in hbm_cond_slices).
  void get_part_if(const std::string& key, const Digest& d, const SliceSpec& spec,
                   const PartCond& cond, Executor* ex, PartCallback done) override;
  void set(const std::string& key, const Digest& d, Bytes value, uint32_t flags,
           uint32_t ttl_s) override;
  void del(const std::string& key, const Digest& d, Executor* ex, DelCallback done) override;
  // Every shard scans its own index (a selector has no owner, and the hot replicas live on
  // all of them): one ReqKind::Purge request per shard in service carrying the selector and
  // the action, queued behind the writes queued before it, hot replicas and refresh fills
  // included. To this tier a soft purge is a purge: only the launch differs. A shard out of
  // service is marked purge_dirty.
  void purge(const KeyedSelector& what, const PurgeAction& how, Executor* ex,
             PurgeCallback done) override;
  void list_objects(const ListQuery& q, Executor* ex, ListCallback done) override;
  // Routed like del(): to the owner, and for a hot object written through to every shard in
  // service (the answer is the owner's). Queued on the shard's stream behind the writes
  // queued before it; a flight's touches are one key-exact HbmCache::touch launch.
  void touch(const std::string& key, const Digest& d, uint32_t ttl_s, const uint32_t* flags,
             Executor* ex, TouchCallback done) override;
  void flush() override;
  std::string name() const override { return "hbm"; }
  // peer path chosen for src -> dst: 0 same device, 1 direct (peer access), 2 staged
  int peer_path(int src_dev, int dst_dev) const;
  void stats(StatList* out) override;
  bool inject_shard_down(int shard, bool down) override;
  void direct_attach(Executor* ex) override;
  bool direct_service() override;
  void direct_detach() override;

  struct HotFill;
  struct HotRefresh;  // one refresh's state and its steps (hbm_hot.cc)
  // One purge() call fanned out over the shards: each shard's Purge request adds what
  // its scan removed when its flight is reaped; the last one to finish (or fail) answers.
  struct Purge {
    std::atomic<int> left{0};
    std::atomic<int64_t> removed{0};
    Executor* ex = nullptr;
    PurgeCallback cb;
    KeyedSelector what;  // the call's copy: the shards' requests point into it
  };
  // One list_objects call walking the shards in order (backend_hbm.cc list_step): every shard
  // in service scans (the totals cover them all), the shards from the cursor's on are asked
  // for the rows still wanted, one at a time.
  struct ListWalk {
    ListQuery q;
    ListResult res;
    int cur_shard = 0;       // the cursor
    uint64_t cur_slot = 0;
    int shard = -1;          // the shard being asked
    uint32_t asked = 0;      // rows asked of it
    bool have_next = false;  // res.next is set: the shards after it only count
    Executor* ex = nullptr;
    ListCallback cb;
  };
  struct Req {
    ReqKind kind = ReqKind::Get;
    Digest d;
    std::string key;
    Bytes value;
    uint32_t flags = 0, ttl = 0;
    bool has_flags = false;  // Touch: `flags` replaces the object's (else they stay)
    // Purge: what is selected (Purge::what of `purge`, which it keeps alive) and what is done
    std::shared_ptr<const KeyedSelector> what;
    PurgeAction how;
    Executor* ex = nullptr;
    GetCallback gcb;
    DelCallback dcb;
    TouchCallback tcb;
    SliceSpec spec{};  // Slice: the window asked for
    std::shared_ptr<const PartCond> cond;  // Slice: its condition (null: none)
    PartCallback pcb;
    // control requests (is_ctl): runs on the batcher thread once the request's flight has
    // finished on the GPU (ok) or was failed
    std::function<void(bool ok)> ccb;
    std::shared_ptr<HotFill> fill;
    std::shared_ptr<Purge> purge;  // Purge: the call it belongs to
    std::shared_ptr<ListWalk> list;  // List: the walk it belongs to; `flags` holds the rows
    uint64_t list_start = 0;         // asked of this shard, list_start the start slot
  };
  struct Dev;
  struct Direct;
  // One hot-set refresh now (serialised with the refresh thread's); its counts. A no-op
  // with spreading off.
  StatList hot_refresh() override;
  bool hot_spreading() const { return hot_on_; }
  // Tests: `fn` runs once, on the refreshing thread, in the next refresh that gets as far as
  // its fills: after the owners' records have been snapshot, before any fill is queued.
  void debug_before_fill(std::function<void()> fn) {
    std::lock_guard<std::mutex> lk(hot_mu_);
    before_fill_ = std::move(fn);
  }
  // reactor contexts (host slots kDirectSlot0 + kDirectJobs * context + job)
  static constexpr int kDirectJobs = 2, kDirectSlot0 = 32, kDirectMax = 15;

 private:
  // owner among the shards up in `up` (-1: none)
  int owner_of(const Digest& d, uint64_t up) const;
  // a GET's shard: a hot object's designated / sprayed replica when that shard holds the
  // replicas (spread_mask_) and is up, else the owner
  int route_get(const Digest& d);
  void sample_get(const Digest& d);
  void enqueue_ctl(int dev, std::function<void(bool)> cb);
  void hot_loop();
  StatList hot_refresh_locked();
  void enqueue(int dev, Req r);
  void enqueue_many(int dev, std::vector<Req>& rs);
  // set / del / touch: queues the write `r` on its owner, then (a hot object) on every other
  // shard in service; false if no shard is in service. `arm(copy, copies, is_owner)` gives
  // each copy its callback.
  template <typename Arm>
  bool route_write(Req r, Arm&& arm);
  uint32_t now() const;
  // SETs / DELETEs accepted and not yet finished on the GPU, counted per digest hash: a
  // reactor-direct GET of such a key goes through the batcher (ordered after them)
  static constexpr size_t kWpend = 1 << 16;
  void write_begin(uint64_t lo) {
    wpend_[lo & (kWpend - 1)].fetch_add(1, std::memory_order_acq_rel);
  }
  void write_end(uint64_t lo) {
    wpend_[lo & (kWpend - 1)].fetch_sub(1, std::memory_order_acq_rel);
  }
  bool writes_pending(uint64_t lo) const {
    return wpend_[lo & (kWpend - 1)].load(std::memory_order_acquire) != 0;
  }
  void direct_submit(Direct& dc, size_t k);
  void direct_reap(Direct& dc, size_t k, int j);

  HbmBackendConfig cfg_;
  DigestRing ring_;
  std::vector<std::unique_ptr<Dev>> devs_;
  std::unique_ptr<std::atomic<uint32_t>[]> wpend_;
  std::mutex direct_mu_;
  std::vector<std::unique_ptr<Direct>> direct_;
  std::vector<uint8_t> peer_ok_;  // [src * n + dst]: peer access enabled (direct xGMI copies)
  std::atomic<uint64_t> up_mask_{0};  // bit i: shard i serves requests
  double epoch_;
  std::atomic<uint64_t> no_shard_misses_{0};
  // purge() calls begun / answered: a warm restore that overlapped one may have copied
  // objects a peer had not purged yet, and flushes the restored shard again
  std::atomic<uint64_t> purge_started_{0}, purge_done_{0};
  std::atomic<uint64_t> soft_purges_{0};
  // purges by tag taken, hard and soft (they count in purge_started_ / purge_done_ for the
  // restore's overlap check, and are taken out of the `hbm_purges` figure)
  std::atomic<uint64_t> tag_purges_{0};
  std::atomic<uint64_t> glob_purges_{0};  // purges by glob, counted likewise
  void purge_finish(const std::shared_ptr<Purge>& p);
  // list_objects' walk: asks the next shard in service, or answers
  void list_step(std::shared_ptr<ListWalk> w);
  std::atomic<uint64_t> lists_{0};
  std::atomic<uint64_t> slices_{0};  // get_part calls taken
  std::atomic<uint64_t> cond_slices_{0};  // get_part_if calls that carried a condition
  void part_request(const std::string& key, const Digest& d, const SliceSpec& spec,
                    std::shared_ptr<const PartCond> cond, Executor* ex, PartCallback done);
  // ---- hot-object spreading (hot_refresh_locked documents the protocol)
  std::unique_ptr<HostRouter> router_;  // ketama owners + the published hot table
  bool hot_on_ = false;
  // shards holding current replicas of the whole published hot set: a GET may go there
  std::atomic<uint64_t> spread_mask_{0};
  static constexpr int kSampleStripes = 16;
  struct alignas(64) SampleStripe {
    std::mutex mu;
    std::vector<Digest> v;
  };
  std::unique_ptr<SampleStripe[]> samples_;
  std::mutex hot_mu_;  // one refresh at a time; guards the refresh state below
  std::function<void()> before_fill_;  // debug_before_fill
  std::unordered_map<Digest, uint64_t, DigestHash, DigestEq> hot_counts_;
  std::vector<Digest> hot_set_;     // the published hot set, hottest first
  std::vector<int32_t> hot_rank_;   // its designated ranks (-1: sprayed)
  std::vector<double> hot_weights_;
  std::thread hot_th_;
  std::mutex hot_th_mu_;
  std::condition_variable hot_cv_;
  bool hot_stop_ = false;
  // GETs answered by a non-owner replica, sharded by the routing thread's slot (every
  // reactor counts without sharing a line)
  struct alignas(64) SpreadCtr {
    std::atomic<uint64_t> v{0};
  };
  SpreadCtr hot_spread_gets_[16];
  std::atomic<uint64_t> hot_refreshes_{0}, hot_added_{0}, hot_removed_{0}, hot_filled_{0},
      hot_fill_skipped_{0}, hot_fill_failed_{0}, hot_deferred_{0},
      hot_fill_bytes_{0}, hot_refresh_us_{0}, hot_samples_{0}, hot_objects_{0},
      hot_dropped_replicas_{0};
};

// Two-level cache: a small host-DRAM L1 in front of a big L2 (HBM shards or
// remote nodes). L1 hits cost a hash probe on the reactor thread (~us); L1
// misses go to L2 and promote on hit; writes go to both levels.
class TieredBackend : public CacheBackend {
 public:
  // promote_max: L2 hits larger than this stay in L2 only (served from there every time,
  // zero-copy for the HBM tier) instead of being copied into — and churning — the L1.
  TieredBackend(std::shared_ptr<CacheBackend> l1, std::shared_ptr<CacheBackend> l2,
                uint32_t promote_ttl_s = 60, uint64_t promote_max = 32 << 10);
  void get(const std::string& key, const Digest& d, Executor* ex, GetCallback done) override;
  // An L1 hit is sliced on the host; an L1 miss asks L2 with get_part. A partial answer never
  // fills L1 (not even a kSliceWholeObj one: a promotion belongs to get()).
  void get_part(const std::string& key, const Digest& d, const SliceSpec& spec, Executor* ex,
                PartCallback done) override;
  // The same under a condition: an L1 hit is decided on the host, an L1 miss asks L2 with it.
  void get_part_if(const std::string& key, const Digest& d, const SliceSpec& spec,
                   const PartCond& cond, Executor* ex, PartCallback done) override;
  void set(const std::string& key, const Digest& d, Bytes value, uint32_t flags,
           uint32_t ttl_s) override;
  void del(const std::string& key, const Digest& d, Executor* ex, DelCallback done) override;
  // L2 first, then L1, with the purge epoch moved in between; the sum, or -1 if either level
  // cannot. A GET that hit L2 before the purge does not promote its object into L1 after L1
  // was purged or softened (purge_epoch_; del() does the same for one key): the promotion
  // would bring back a removed object, or a fresh copy of a softened one.
  void purge(const KeyedSelector& what, const PurgeAction& how, Executor* ex,
             PurgeCallback done) override;
  void list_objects(const ListQuery& q, Executor* ex, ListCallback done) override;
  // L2 first, then L1; the answer is L2's (on 0 or -1 the caller re-stores the object, which
  // writes both levels). A promotion that straddles the touch is dropped, as for del(): it
  // would carry the pre-touch TTL and flags into L1.
  void touch(const std::string& key, const Digest& d, uint32_t ttl_s, const uint32_t* flags,
             Executor* ex, TouchCallback done) override;
  void flush() override;
  std::string name() const override { return l1_->name() + "+" + l2_->name(); }
  void stats(StatList* out) override;
  bool inject_shard_down(int shard, bool down) override;
  void direct_attach(Executor* ex) override {
    l1_->direct_attach(ex);
    l2_->direct_attach(ex);
  }
  bool direct_service() override {
    const bool a = l1_->direct_service();
    return l2_->direct_service() || a;
  }
  void direct_detach() override {
    l1_->direct_detach();
    l2_->direct_detach();
  }
  StatList hot_refresh() override { return l2_->hot_refresh(); }

 private:
  std::shared_ptr<CacheBackend> l1_, l2_;
  uint32_t promote_ttl_;
  uint64_t promote_max_;
  std::atomic<uint64_t> promoted_{0}, not_promoted_{0};
  std::atomic<uint64_t> l1_hits_{0}, l2_hits_{0}, misses_{0};
  // Purge epoch: moved between the L2 and the L1 pass of a purge or a delete. A GET reads it
  // when it starts and promotes its L2 hit (check + L1 set under the shared lock) only if it
  // has not moved; the move takes the lock exclusively, so a promotion either lands before
  // the L1 pass (which removes it) or sees the new epoch and is dropped.
  std::atomic<uint64_t> purge_epoch_{0};
  std::shared_mutex promote_mu_;
  std::atomic<uint64_t> purges_{0}, promote_dropped_{0};
  void move_purge_epoch();
};

// Fault injection: a decorator that makes the wrapped tier misbehave
// on purpose — GETs answered as misses, SETs dropped, answers delayed, or the whole
// tier "down" (every GET misses, every SET is lost) — with probabilities that can be
// changed while the proxy runs. Used by the failure tests and for drills.
struct FaultSpec {
  double get_miss = 0;    // P(GET answered as a miss without asking the tier)
  double set_drop = 0;    // P(SET silently dropped)
  uint32_t delay_us = 0;  // extra latency before every GET/DEL is answered
  bool down = false;      // tier unreachable
  int gpu_down = -1;      // GPU shard K of the tier ejected (HbmBackend ring ejection)
};
FaultSpec parse_fault_spec(const std::string& spec);  // "get_miss=0.1,set_drop=1,delay_us=500,down"

class FaultBackend : public CacheBackend {
 public:
  FaultBackend(std::shared_ptr<CacheBackend> inner, const FaultSpec& spec, uint64_t seed = 1);
  ~FaultBackend() override;
  void get(const std::string& key, const Digest& d, Executor* ex, GetCallback done) override;
  void set(const std::string& key, const Digest& d, Bytes value, uint32_t flags,
           uint32_t ttl_s) override;
  void del(const std::string& key, const Digest& d, Executor* ex, DelCallback done) override;
  void purge(const KeyedSelector& what, const PurgeAction& how, Executor* ex,
             PurgeCallback done) override {
    inner_->purge(what, how, ex, std::move(done));
  }
  void list_objects(const ListQuery& q, Executor* ex, ListCallback done) override {
    inner_->list_objects(q, ex, std::move(done));
  }
  void touch(const std::string& key, const Digest& d, uint32_t ttl_s, const uint32_t* flags,
             Executor* ex, TouchCallback done) override {
    inner_->touch(key, d, ttl_s, flags, ex, std::move(done));
  }
  void flush() override { inner_->flush(); }
  std::string name() const override { return "fault(" + inner_->name() + ")"; }
  void stats(StatList* out) override;
  bool inject_shard_down(int shard, bool down) override;
  void direct_attach(Executor* ex) override { inner_->direct_attach(ex); }
  bool direct_service() override { return inner_->direct_service(); }
  void direct_detach() override { inner_->direct_detach(); }
  StatList hot_refresh() override { return inner_->hot_refresh(); }
  void set_spec(const FaultSpec& spec);
  FaultSpec spec() const;

 private:
  bool roll(double p);
  void later(std::function<void()> fn);  // run after delay_us on the timer thread
  void timer_loop();

  std::shared_ptr<CacheBackend> inner_;
  mutable std::mutex mu_;
  FaultSpec spec_;
  uint64_t rng_;
  std::atomic<uint64_t> injected_miss_{0}, injected_drop_{0}, injected_delay_{0};
  // delay timer
  std::condition_variable cv_;
  std::deque<std::pair<double, std::function<void()>>> timers_;  // FIFO: one fixed delay
  bool stop_ = false;
  std::thread th_;
};

struct MemcachedConfig {
  std::vector<Addr> servers;
  int retry_timeout_s = 2;     // ejected node is retried after this long
  int connect_timeout_ms = 500;
  int op_timeout_ms = 1000;
};

class MemcachedBackend : public CacheBackend {
 public:
  explicit MemcachedBackend(const MemcachedConfig& cfg);
  ~MemcachedBackend() override;
  void get(const std::string& key, const Digest& d, Executor* ex, GetCallback done) override;
  void set(const std::string& key, const Digest& d, Bytes value, uint32_t flags,
           uint32_t ttl_s) override;
  void del(const std::string& key, const Digest& d, Executor* ex, DelCallback done) override;
  void flush() override;
  std::string name() const override { return "memcached"; }
  void stats(StatList* out) override;

 private:
  struct Pending {
    uint8_t op;
    Executor* ex;
    GetCallback gcb;
    DelCallback dcb;
    double t0;
  };
  struct Node;
  struct Cmd {
    std::string key;
    uint8_t op;
    Bytes value;
    uint32_t flags, ttl;
    Executor* ex;
    GetCallback gcb;
    DelCallback dcb;
  };
  void loop();
  void submit(Cmd c);
  void node_fail(int idx);
  void drain_commands();
  static std::string wire_key(const std::string& key);

  MemcachedConfig cfg_;
  KetamaRing ring_;
  std::vector<std::unique_ptr<Node>> nodes_;
  int epfd_ = -1, evfd_ = -1;
  std::mutex mu_;
  std::vector<Cmd> inbox_;
  std::atomic<bool> stop_{false};
  std::thread th_;
  std::atomic<uint64_t> gets_{0}, hits_{0}, sets_{0}, errors_{0}, ejections_{0};
};

}  // namespace shellac
