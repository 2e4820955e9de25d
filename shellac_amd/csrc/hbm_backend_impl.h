// HbmBackend's internals, shared by its translation units:
//   backend_hbm.cc   construction, routing, the request API, purge fan-out, flush, stats
//   hbm_batcher.cc   Dev: the per-GPU batcher thread (flights, reaping, ejection, restore)
//   hbm_direct.cc    Direct: reactor-direct GETs through the edge server
//   hbm_hot.cc       hot-object spreading: the refresh thread and its protocol
// The host-only decisions they share are in hbm_flight_plan.h (no HIP there).
#pragma once

#include <chrono>
#include <cstdio>
#include <unordered_set>

#include "backend.h"
#include "hbm_cache.h"
#include "hbm_flight_plan.h"
#include "keyed.h"
#include "trace.h"

namespace shellac {

inline double wall_s() {
  return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch())
      .count();
}

#define HB_OK(expr)                                                                   \
  do {                                                                                \
    hipError_t _e = (expr);                                                           \
    if (_e != hipSuccess) throw Error(std::string("HIP: ") + hipGetErrorString(_e) + \
                                      " at " #expr);                                  \
  } while (0)

// Mapped pinned buffer (host pointer + its device view) that grows on demand.
struct Mapped {
  uint8_t* h = nullptr;
  uint8_t* d = nullptr;
  size_t cap = 0;
  void ensure(size_t bytes) {
    if (bytes <= cap) return;
    size_t c = cap ? cap : 4096;
    while (c < bytes) c *= 2;
    release();
    HB_OK(hipHostMalloc(reinterpret_cast<void**>(&h), c, hipHostMallocMapped));
    HB_OK(hipHostGetDevicePointer(reinterpret_cast<void**>(&d), h, 0));
    cap = c;
  }
  void release() {
    if (h) (void)hipHostFree(h);
    h = d = nullptr;
    cap = 0;
  }
  template <typename T>
  T* host() const { return reinterpret_cast<T*>(h); }
  template <typename T>
  T* dev() const { return reinterpret_cast<T*>(d); }
};

// Device buffer that grows on demand (the hot-set refresh's staging; the caller has set
// the device). Growing frees the old block, so only the refresh thread, which owns these,
// grows them, and never while a fill that reads them is still queued.
struct DevBuf {
  void* p = nullptr;
  size_t cap = 0;
  template <typename T>
  T* ensure(size_t bytes) {
    if (bytes > cap) {
      if (p) (void)hipFree(p);
      p = nullptr;
      cap = 0;
      const size_t c = std::max<size_t>({bytes, 4096});
      HB_OK(hipMalloc(&p, c));
      cap = c;
    }
    return static_cast<T*>(p);
  }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
  }
};

// Pinned response arenas. A GET batch gathers into one; its hits are ByteRef slices that
// own a reference, so the arena returns to the pool (not to the allocator) when the last
// response built from it has been written to its client. Pinned allocations and frees
// are slow and hipHostFree waits for the device, so neither happens on a reactor thread:
// give_back() only files the arena; take() (the batcher) picks the smallest one that
// fits and trims the pool beyond kKeepBytes of idle arenas.
class ArenaPool : public std::enable_shared_from_this<ArenaPool> {
 public:
  struct Arena {
    uint8_t* h = nullptr;
    uint8_t* d = nullptr;
    size_t cap = 0;
  };
  static constexpr size_t kKeepBytes = size_t(1) << 30;  // idle arenas kept (per GPU)
  explicit ArenaPool(int device) : device_(device) {}
  ~ArenaPool() {
    for (auto& a : free_) (void)hipHostFree(a.h);
  }
  std::shared_ptr<Arena> take(size_t min_cap) {
    Arena a{};
    std::vector<Arena> trim;
    {
      std::lock_guard<std::mutex> lk(mu_);
      take_best(min_cap, &a);
      while (free_bytes_ > kKeepBytes && !free_.empty()) {  // the smallest idle arenas go
        size_t k = 0;
        for (size_t i = 1; i < free_.size(); ++i)
          if (free_[i].cap < free_[k].cap) k = i;
        free_bytes_ -= free_[k].cap;
        trim.push_back(free_[k]);
        free_.erase(free_.begin() + (long)k);
      }
    }
    for (const Arena& t : trim) {
      (void)hipHostFree(t.h);
      allocated_.fetch_sub(t.cap, std::memory_order_relaxed);
      frees_.fetch_add(1, std::memory_order_relaxed);
    }
    if (!a.h) {
      size_t c = 1u << 20;
      while (c < min_cap) c *= 2;
      HB_OK(hipSetDevice(device_));
      const double t0 = wall_s();
      HB_OK(hipHostMalloc(reinterpret_cast<void**>(&a.h), c, hipHostMallocMapped));
      HB_OK(hipHostGetDevicePointer(reinterpret_cast<void**>(&a.d), a.h, 0));
      const uint64_t us = (uint64_t)((wall_s() - t0) * 1e6);
      if (us > alloc_max_us_.load(std::memory_order_relaxed)) alloc_max_us_.store(us);
      a.cap = c;
      allocated_.fetch_add(c, std::memory_order_relaxed);
      allocs_.fetch_add(1, std::memory_order_relaxed);
    }
    return lend(a);
  }
  // take() without allocating or trimming (no HIP call: safe on a reactor thread); null
  // when no idle arena fits
  std::shared_ptr<Arena> try_take(size_t min_cap) {
    Arena a{};
    {
      std::lock_guard<std::mutex> lk(mu_);
      if (!take_best(min_cap, &a)) return nullptr;
    }
    return lend(a);
  }
  // n arenas of cap bytes into the free list (at start-up, before any traffic)
  void reserve(size_t n, size_t cap) {
    std::vector<std::shared_ptr<Arena>> held;
    for (size_t i = 0; i < n; ++i) held.push_back(take(cap));
  }  // returned to the pool here
  uint64_t allocated() const { return allocated_.load(std::memory_order_relaxed); }
  uint64_t allocs() const { return allocs_.load(std::memory_order_relaxed); }
  uint64_t frees() const { return frees_.load(std::memory_order_relaxed); }
  uint64_t alloc_max_us() const { return alloc_max_us_.load(std::memory_order_relaxed); }

 private:
  // the smallest idle arena of at least min_cap bytes, out of the free list (under mu_)
  bool take_best(size_t min_cap, Arena* a) {
    int best = -1;
    for (size_t i = 0; i < free_.size(); ++i)
      if (free_[i].cap >= min_cap && (best < 0 || free_[i].cap < free_[(size_t)best].cap))
        best = (int)i;
    if (best < 0) return false;
    *a = free_[(size_t)best];
    free_.erase(free_.begin() + best);
    free_bytes_ -= a->cap;
    return true;
  }
  std::shared_ptr<Arena> lend(const Arena& a) {
    auto pool = shared_from_this();
    return std::shared_ptr<Arena>(new Arena(a), [pool](Arena* p) {
      pool->give_back(*p);
      delete p;
    });
  }
  void give_back(const Arena& a) {  // any thread (often a reactor): no HIP call here
    std::lock_guard<std::mutex> lk(mu_);
    free_.push_back(a);
    free_bytes_ += a.cap;
  }
  int device_;
  std::mutex mu_;
  std::vector<Arena> free_;
  size_t free_bytes_ = 0;
  std::atomic<uint64_t> allocated_{0}, allocs_{0}, frees_{0}, alloc_max_us_{0};
};

// Completions grouped per executor: one post_batch (one lock, one wake-up) per reactor.
// answer() is how every request is answered: on its executor when it has one, else inline.
struct PostGroups {
  std::vector<std::pair<Executor*, std::vector<std::function<void()>>>> g;
  std::vector<std::function<void()>>& at(Executor* ex) {
    for (auto& p : g)
      if (p.first == ex) return p.second;
    g.emplace_back(ex, std::vector<std::function<void()>>{});
    return g.back().second;
  }
  template <typename Fn>
  void answer(Executor* ex, Fn&& fn) {
    if (ex) at(ex).push_back(std::forward<Fn>(fn));
    else fn();
  }
  void flush() {
    for (auto& p : g) p.first->post_batch(p.second);
    g.clear();
  }
  // one answer outside a flight (nothing to group)
  template <typename Fn>
  static void answer_now(Executor* ex, Fn&& fn) {
    if (ex) ex->post(std::forward<Fn>(fn));
    else fn();
  }
};

// One batch in flight on a GPU.
struct Flight {
  std::vector<HbmBackend::Req> reqs;
  std::vector<uint32_t> gets, sets, dels, touches, slices;  // request indices by kind
  std::vector<uint32_t> ctls;              // barriers, hot-replica fills and purges
  std::vector<uint32_t> urow;              // GET request -> GPU row (host coalescing)
  size_t rows = 0;                         // distinct GET digests
  Mapped keys, offs;                                           // launch_gets
  Mapped set_keys, set_vals, set_voff, set_meta;               // launch_sets
  Mapped del_keys, del_found;                                  // launch_dels
  // launch_touches: the distinct rows' {digests, key offsets, expiries, flags, hit bytes} and
  // their packed key bytes; trow maps a touch request to its row (the last request of a key wins)
  Mapped touch_rows, touch_kbytes;
  // launch_purges: pattern images (keyed.h) and {removed, bytes} word pairs, one per purge (a
  // soft purge fills the first word: the objects softened); a tag purge's image is its hash list
  Mapped purge_img, purge_out;
  // launch_lists (at most one list a flight: plan_take cuts after it): [pattern image or tag
  // list | 4 result words | rows | key areas], at the offsets below
  Mapped list_buf;
  size_t list_out_off = 0, list_rows_off = 0, list_keys_off = 0;
  // launch_slices: [digests | key offsets | window specs | result rows | result words | key
  // bytes] of the flight's slices, one row per request, at the offsets below; their bytes land
  // in an arena of their own
  Mapped slice_buf;
  size_t slice_offs_off = 0, slice_spec_off = 0, slice_rows_off = 0, slice_res_off = 0,
         slice_kb_off = 0;
  // where some slice of the flight carries a condition: [SliceCond per row | candidate bytes]
  // behind the key bytes
  bool slice_conds = false;
  size_t slice_cond_off = 0, slice_cb_off = 0;
  std::shared_ptr<ArenaPool::Arena> slice_arena;
  void release_mapped() {
    for (Mapped* m : {&keys, &offs, &set_keys, &set_vals, &set_voff, &set_meta, &del_keys,
                      &del_found, &touch_rows, &touch_kbytes, &purge_img, &purge_out, &list_buf,
                      &slice_buf})
      m->release();
  }
  std::vector<uint32_t> trow;
  const uint8_t* touch_hit = nullptr;
  std::shared_ptr<ArenaPool::Arena> arena;
  std::vector<uint64_t> wkeys;  // SET / DELETE / touch digests (lo words) counted in Dev::pend_w
  bool flush = false;           // a flush runs on the stream right before this flight
  hipEvent_t ev = nullptr;
  int slot = -1;
  bool active = false, got = false;
  bool served = false;  // GETs answered by the persistent edge server (no stream launch)
  uint32_t tnow = 0;
  double t0 = 0;
};

// A hot-replica fill queued on a target shard (HbmBackend::HotRefresh): m records gathered
// on their owners and peer-copied into this shard's staging (krec at koff, digests kk),
// stored by the target's batcher in stream order. Rows whose digest had a SET or DELETE
// queued to this shard since the refresh began (Dev::touched) are dropped at launch: the
// write-through copy is newer than the owner's record read here.
struct HbmBackend::HotFill {
  int64_t m = 0;
  const Digest* kk = nullptr;
  const uint8_t* krec = nullptr;
  const uint64_t* koff = nullptr;
  uint64_t* hsize = nullptr;      // mapped host view of the row sizes (0: no record)
  const uint64_t* dsize = nullptr;  // its device view
  Digest* okeys = nullptr;
  uint64_t* ovoff = nullptr;
  uint32_t* ometa = nullptr;
  uint64_t bound = 0;
  std::vector<uint64_t> lo;  // row digests' low words (the touched check)
  // under the target Dev's mu
  bool cancelled = false, launched = false;
  uint64_t skipped = 0, rows = 0;
};

// The hot-set refresh's staging on one GPU (the refresh thread's): as an owner, whose records
// are snapshot ...
struct SnapStaging {
  DevBuf keys, loc, size, off, rec;
  void release() {
    for (DevBuf* b : {&keys, &loc, &size, &off, &rec}) b->release();
  }
};
// ... and as the target of a fill.
struct FillStaging {
  DevBuf keys, rec, off, okeys, voff, meta;
  Mapped size;
  void release() {
    for (DevBuf* b : {&keys, &rec, &off, &okeys, &voff, &meta}) b->release();
    size.release();
  }
  // a fill still reads it on the GPU: leaked, not reused
  void abandon() { *this = FillStaging{}; }
};

struct HbmBackend::Dev {
  HbmBackend* be = nullptr;
  int index = 0, device = 0;
  std::unique_ptr<HbmCache> cache;
  hipStream_t stream = nullptr;
  std::shared_ptr<ArenaPool> pool;
  std::vector<std::unique_ptr<Flight>> flights;
  size_t head = 0, inflight = 0;  // oldest flight, flights launched and not yet freed
  // queue (reactor threads -> batcher)
  std::mutex mu;
  std::condition_variable cv;
  std::vector<Req> q;
  std::atomic<size_t> qn{0};
  std::atomic<bool> spinning{false};
  bool stop = false, flush_req = false;
  bool kick = false;  // the shard's state changed (drill set / lifted): wake an idle batcher
  std::atomic<bool> ctl_pending{false};  // flush / filter rebuild requested (no requests needed)
  std::thread th;
  // health
  std::atomic<bool> forced_down{false};
  // a purge found this shard out of service, or the shard failed one: it may hold purged
  // objects, so its restore flushes it whatever flush_on_restore says
  std::atomic<bool> purge_dirty{false};
  // back in the ring and still pulling its objects from peers: GETs neither skip on the
  // presence filter nor bypass the batcher (they queue behind the migration)
  std::atomic<bool> restoring{false};
  bool failed = false;
  double retry_at = 0;
  // presence filter (this shard's digests)
  std::shared_ptr<PresenceFilter> filt, filt_next;
  uint64_t filt_bits = 0, filt_rebuild_at = 0;
  bool filt_want_rebuild = false;
  // warm restore over xGMI: a stream for peer work on this GPU and the digest ring on
  // the device (route_keys)
  hipStream_t mstream = nullptr;
  hipStream_t sstream = nullptr;  // stats reads (non-blocking: never waits on other streams)
  uint32_t* d_pts = nullptr;
  int32_t* d_own = nullptr;
  int npts = 0;
  // co-table for host GET coalescing (batcher thread only)
  std::vector<int32_t> co_tab;
  // hot-set refresh: digests (lo) being filled into this shard, and those of them that a
  // SET / DELETE queued here since (both under mu)
  std::unordered_set<uint64_t> filling, touched;
  SnapStaging hs;
  FillStaging hf;
  std::atomic<uint64_t> eject_gen{0};  // bumped when the shard leaves service
  struct alignas(64) Ctr {
    std::atomic<uint64_t> v{0};
  };
  // GETs routed to this shard (per-shard load), sharded by the routing thread's slot: the
  // reactors never share a counter line
  static constexpr int kCtrShards = 16;
  Ctr routed_gets[kCtrShards];
  uint64_t routed_total() const {
    uint64_t t = 0;
    for (const Ctr& c : routed_gets) t += c.v.load(std::memory_order_relaxed);
    return t;
  }
  // digests (lo word) with a SET / DELETE in a flight not yet reaped, and flushes in
  // flight: a GET of such a key takes the stream path, ordered after them
  std::unordered_map<uint64_t, uint32_t> pend_w;
  TakeScratch take_scratch;
  uint32_t pend_flush = 0;
  void track_writes(Flight& f, int dir);
  double avg_row_bytes = 4096;
  double avg_slice_bytes = 8192;  // a slice row's bytes in its arena (head and window granules)
  // flushes requested and not yet finished on the GPU (any thread reads it: a
  // reactor-direct GET waits for them by going through the batcher)
  std::atomic<uint32_t> flush_pend{0};
  void flush_done() { flush_pend.fetch_sub(1, std::memory_order_acq_rel); }
  // offsets arrays of the reactor-direct jobs on this GPU (mapped; 32 words per job)
  Mapped direct_offs;
  // stats
  std::atomic<uint64_t> batches{0}, batched_reqs{0}, max_batch{0}, batch_ns{0}, coalesced{0},
      filt_skips{0}, filt_rebuilds{0}, sweeps{0}, live_objects{0}, live_bytes{0},
      key_mismatch{0}, failures{0}, ejections{0}, restores{0}, regathers{0}, arena_misses{0},
      dropped{0}, staged_copies{0}, served_batches{0}, ordered_gets{0},
      migrated{0}, migrate_ns{0}, direct_jobs{0}, direct_reqs{0}, direct_fallbacks{0},
      direct_overflows{0}, direct_timeouts{0}, direct_ns{0}, purged_objects{0},
      purged_bytes{0}, touch_reqs{0}, softened_objects{0}, tag_purged_objects{0},
      tag_softened_objects{0}, glob_purged_objects{0}, glob_softened_objects{0}, slice_reqs{0};

  void loop();
  bool take_batch(std::vector<Req>* out, bool* do_flush, bool* rebuilding);
  bool launch_queued(std::vector<Req>& batch);
  // a flight's stages, in stream order; each stages into its own Flight buffers
  void launch(Flight& f);
  void launch_gets(Flight& f);
  void launch_sets(Flight& f);
  void launch_dels(Flight& f);
  void launch_touches(Flight& f);
  void launch_fills(Flight& f);
  void launch_purges(Flight& f);
  void launch_lists(Flight& f);
  void launch_slices(Flight& f);
  void run_slices(Flight& f);
  void deliver_slices(Flight& f);
  void deliver_list(Flight& f, Req& r);
  bool try_reap(Flight& f, bool block);
  void regather(Flight& f, uint64_t total);
  void deliver_gets(Flight& f);
  void deliver_dels(Flight& f);
  void deliver_touches(Flight& f);
  void finish_ctls(Flight& f);
  void overflow_misses(Flight& f);
  void fail_flight(Flight& f);
  // `unlaunched`: the requests never reached the GPU (their SETs / DELETEs end here)
  void fail_requests(std::vector<Req>& reqs, bool unlaunched);
  void eject(const char* why);
  void maybe_restore();
  uint64_t migrate_from(Dev& src);
  bool migrate_candidates(Dev& src, uint32_t t, std::vector<Digest>* out);
  uint64_t migrate_chunk(Dev& src, const Digest* keys, int64_t m, uint32_t t);
  void sweep();
  void finish_filter_rebuild();
  bool up() const { return (be->up_mask_.load(std::memory_order_acquire) >> index) & 1; }
  void set_up(bool on) {
    if (on) be->up_mask_.fetch_or(1ull << index);
    else be->up_mask_.fetch_and(~(1ull << index));
  }
  ~Dev() {
    (void)hipSetDevice(device);
    if (stream) (void)hipStreamSynchronize(stream);
    for (auto& f : flights) {
      f->release_mapped();
      f->arena.reset();
      f->slice_arena.reset();
      if (f->ev) (void)hipEventDestroy(f->ev);
    }
    direct_offs.release();
    hs.release();
    hf.release();
    cache.reset();
    if (stream) (void)hipStreamDestroy(stream);
    if (mstream) (void)hipStreamDestroy(mstream);
    if (sstream) (void)hipStreamDestroy(sstream);
    (void)hipFree(d_pts);
    (void)hipFree(d_own);
  }
};

// Host slots the edge GET signals completion through: one per flight.
constexpr int kFlightSlot0 = 8;

// A reactor's direct-submission context (one per attached reactor thread, used only by
// that thread): per GPU, the GETs it accepted this loop iteration and up to kDirectJobs
// edge-server jobs in flight, each answered from its own host slot and pinned arena.
struct HbmBackend::Direct {
  static constexpr int kOffWords = 32;  // >= kServeKeys + 1
  struct Job {
    int slot = -1;
    bool busy = false, answered = false;
    std::vector<Req> reqs;
    std::vector<uint32_t> urow;
    Digest keys[HbmCache::kServeKeys];
    size_t rows = 0;
    uint64_t* offs_h = nullptr;
    uint64_t* offs_d = nullptr;
    std::shared_ptr<ArenaPool::Arena> arena;
    uint32_t tnow = 0;
    double t0 = 0;
  };
  struct PerDev {
    std::vector<Req> pending;
    Job jobs[kDirectJobs];
    double avg_row_bytes = 4096;
  };
  int idx = 0;
  Executor* ex = nullptr;  // the attached reactor (null: context free)
  bool poisoned = false;   // a job never completed: the context is not reused
  std::vector<PerDev> dev;
};

// The calling thread's direct context (set by direct_attach on a reactor thread).
struct DirectTls {
  HbmBackend* be = nullptr;
  HbmBackend::Direct* ctx = nullptr;
};
inline thread_local DirectTls tl_direct;

// Record [ItemHeader | u16 klen | key | payload] at base + o (sz bytes, 0 = miss) checked
// against the request's digest and key; a hit is a ByteRef slice that keeps `owner` alive.
inline bool read_hit(const uint8_t* base, uint64_t o, uint64_t sz, const Digest& d,
                     const std::string& key, uint32_t tnow,
                     const std::shared_ptr<const void>& owner, CacheValue* v, bool* mismatch) {
  if (!sz) return false;
  ItemHeader h;
  std::memcpy(&h, base + o, sizeof h);
  if (h.magic != kItemMagic || h.d0 != d.lo || h.d1 != d.hi) return false;
  size_t po = 0;
  const char* val = reinterpret_cast<const char*>(base + o + kItemHeaderBytes);
  if (!keyed_match(val, h.vlen, key, &po)) {
    *mismatch = true;  // digest collision
    return false;
  }
  v->flags = h.flags;
  v->ttl_left = h.expire ? (int64_t)h.expire - (int64_t)tnow : 0;
  v->data = ByteRef(owner, val + po, h.vlen - po);
  return true;
}

// src (on src_dev) -> dst (on dst_dev), ordered on `stream` (dst_dev's): a device copy on
// one GPU, a direct peer DMA where peer access is enabled, else staged through pinned
// host memory in 64 MiB pieces (synchronous; off the request path). `path`: peer_path().
void copy_between(void* dst, int dst_dev, const void* src, int src_dev, size_t bytes,
                  hipStream_t stream, int path);

}  // namespace shellac
