// HbmBackend: the HTTP proxy's (and the memcached node's) cache tier over one HBM shard
// per local MI355X (split from backend.cc so the host-only backends build without ROCm).
//
// Replaces the reference's blocking memcached round trip inside the reactor
// (src/python/shellac/server/Server.py:335 get, :432 set). This file is what the reactors
// call: construction, routing (owners, hot replicas), the request API (get / set / del /
// touch / purge / flush), drills and stats. A request ends up on its shard's queue,
// served by that GPU's batcher thread (hbm_batcher.cc), or for a small GET batch with the
// calling reactor itself (hbm_direct.cc); hbm_hot.cc keeps the replicated hot set current.
// hbm_backend_impl.h has the types they share, hbm_flight_plan.h the host-only decisions.
#include <algorithm>
#include <optional>

#include "hbm_backend_impl.h"

namespace shellac {

HbmBackend::HbmBackend(const HbmBackendConfig& cfg)
    : cfg_(cfg), ring_((int)cfg.devices.size()), epoch_(wall_s()) {
  SH_CHECK(!cfg_.devices.empty() && cfg_.devices.size() <= 64, "HbmBackend needs 1..64 devices");
  SH_CHECK(cfg_.depth >= 1 && kFlightSlot0 + cfg_.depth <= kDirectSlot0,
           "pipeline depth out of range");
  static_assert(kDirectSlot0 + kDirectJobs * kDirectMax <= HbmCache::kHeadSlot,
                "direct host slots overlap the head slot");
  static_assert(Direct::kOffWords >= HbmCache::kServeKeys + 1, "direct offsets too short");
  SH_CHECK(cfg_.direct_backlog >= 1, "direct_backlog must be >= 1");
  wpend_.reset(new std::atomic<uint32_t>[kWpend]);
  for (size_t i = 0; i < kWpend; ++i) wpend_[i].store(0, std::memory_order_relaxed);
  for (size_t i = 0; i < cfg_.devices.size(); ++i) {
    auto d = std::make_unique<Dev>();
    d->be = this;
    d->index = (int)i;
    d->device = cfg_.devices[i];
    HB_OK(hipSetDevice(d->device));
    ShardConfig sc;
    sc.log_bytes = cfg_.log_bytes_per_gpu / 16 * 16;
    sc.nbuckets = cfg_.nbuckets_per_gpu;
    sc.max_item = cfg_.max_item + (uint32_t)keyed_size(kMaxKeyedKey, 0);
    sc.device = d->device;
    sc.evict = cfg_.evict;
    sc.serve_blocks = cfg_.serve_blocks;
    d->cache = std::make_unique<HbmCache>(sc);
    HB_OK(hipStreamCreateWithFlags(&d->stream, hipStreamNonBlocking));
    HB_OK(hipStreamCreateWithFlags(&d->mstream, hipStreamNonBlocking));
    HB_OK(hipStreamCreateWithFlags(&d->sstream, hipStreamNonBlocking));
    {
      const auto& pts = ring_.points();
      std::vector<uint32_t> hp(pts.size());
      std::vector<int32_t> ho(pts.size());
      for (size_t k = 0; k < pts.size(); ++k) {
        hp[k] = pts[k].first;
        ho[k] = pts[k].second;
      }
      d->npts = (int)pts.size();
      HB_OK(hipMalloc(&d->d_pts, std::max<size_t>(1, hp.size()) * sizeof(uint32_t)));
      HB_OK(hipMalloc(&d->d_own, std::max<size_t>(1, ho.size()) * sizeof(int32_t)));
      HB_OK(hipMemcpy(d->d_pts, hp.data(), hp.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
      HB_OK(hipMemcpy(d->d_own, ho.data(), ho.size() * sizeof(int32_t), hipMemcpyHostToDevice));
      // a pageable-memory hipMemcpy may return before its DMA lands; the batcher's
      // non-blocking streams do not wait for the null stream
      HB_OK(hipDeviceSynchronize());
    }
    d->pool = std::make_shared<ArenaPool>(d->device);
    if (cfg_.arena_bytes) d->pool->reserve((size_t)cfg_.depth + 2, (size_t)cfg_.arena_bytes);
    if (cfg_.direct && cfg_.edge_server) {
      // reactors never allocate pinned memory: their arenas and offsets exist up front
      if (cfg_.direct_arenas > 0 && cfg_.direct_arena_bytes)
        d->pool->reserve((size_t)cfg_.direct_arenas, (size_t)cfg_.direct_arena_bytes);
      d->direct_offs.ensure((size_t)kDirectMax * kDirectJobs * Direct::kOffWords * 8);
    }
    for (int k = 0; k < cfg_.depth; ++k) {
      auto f = std::make_unique<Flight>();
      HB_OK(hipEventCreateWithFlags(&f->ev, hipEventDisableTiming));
      f->slot = kFlightSlot0 + k;
      f->keys.ensure(4096 * sizeof(Digest));
      f->offs.ensure(4097 * 8);
      d->flights.push_back(std::move(f));
    }
    d->cache->reserve(4096);
    if (cfg_.presence_filter) {
      // 16 bits per index slot (capped at 256 MiB): ~2 % false positives when a full
      // index's worth of digests has been added since the last rebuild
      const uint64_t slots = cfg_.nbuckets_per_gpu * kEntriesPerBucket;
      d->filt_bits = std::min<uint64_t>(slots * 16, 1ull << 31);
      d->filt_rebuild_at = slots;
      d->filt = std::make_shared<PresenceFilter>(d->filt_bits);
    }
    up_mask_.fetch_or(1ull << i);
    devs_.push_back(std::move(d));
  }
  if (cfg_.direct && cfg_.edge_server) {
    for (int c = 0; c < kDirectMax; ++c) {
      auto dc = std::make_unique<Direct>();
      dc->idx = c;
      dc->dev.resize(devs_.size());
      for (size_t k = 0; k < devs_.size(); ++k)
        for (int j = 0; j < kDirectJobs; ++j) {
          Direct::Job& jb = dc->dev[k].jobs[j];
          const size_t w = ((size_t)c * kDirectJobs + (size_t)j) * Direct::kOffWords;
          jb.slot = kDirectSlot0 + c * kDirectJobs + j;
          jb.offs_h = devs_[k]->direct_offs.host<uint64_t>() + w;
          jb.offs_d = devs_[k]->direct_offs.dev<uint64_t>() + w;
        }
      direct_.push_back(std::move(dc));
    }
  }
  // Peer access between the shards' GPUs (warm restore copies over xGMI). A pair the
  // runtime cannot map, or every pair under peer_copy = "staged", copies through pinned
  // host memory instead (peer_path / copy_between).
  const size_t nd = devs_.size();
  peer_ok_.assign(nd * nd, 0);
  if (cfg_.peer_copy != "staged") {
    for (size_t i = 0; i < nd; ++i)
      for (size_t j = 0; j < nd; ++j) {
        const int a = devs_[i]->device, b = devs_[j]->device;
        if (a == b) continue;
        int can = 0;
        if (hipDeviceCanAccessPeer(&can, b, a) != hipSuccess || !can) continue;
        HB_OK(hipSetDevice(b));  // b (the destination) reads / DMAs from a's memory
        const hipError_t e = hipDeviceEnablePeerAccess(a, 0);
        if (e == hipSuccess || e == hipErrorPeerAccessAlreadyEnabled) peer_ok_[i * nd + j] = 1;
        else (void)hipGetLastError();  // clear the sticky error: the pair stays staged
      }
  }
  if (devs_.size() > 1) {
    // DigestRing's points (tests check the owners agree), answered from the span table
    router_ = std::make_unique<HostRouter>((int)devs_.size());
    if (cfg_.hot_objects > 0 && cfg_.flush_on_restore) {
      SH_CHECK(cfg_.hot_sample >= 1 && (cfg_.hot_sample & (cfg_.hot_sample - 1)) == 0,
               "hot_sample must be a power of two");
      hot_on_ = true;
      samples_.reset(new SampleStripe[kSampleStripes]);
      hot_weights_.assign(devs_.size(), 1.0);
      spread_mask_.store(up_mask_.load());
    }
  }
  for (auto& d : devs_) {
    Dev* dp = d.get();
    dp->th = std::thread([dp] { dp->loop(); });
  }
  if (hot_on_ && cfg_.hot_refresh_ms > 0) hot_th_ = std::thread([this] { hot_loop(); });
}

HbmBackend::~HbmBackend() {
  {
    std::lock_guard<std::mutex> lk(hot_th_mu_);
    hot_stop_ = true;
  }
  hot_cv_.notify_all();
  if (hot_th_.joinable()) hot_th_.join();  // first: a refresh waits on the batchers
  for (auto& d : devs_) {
    {
      std::lock_guard<std::mutex> lk(d->mu);
      d->stop = true;
    }
    d->cv.notify_all();
  }
  for (auto& d : devs_)
    if (d->th.joinable()) d->th.join();
}

uint32_t HbmBackend::now() const { return (uint32_t)(wall_s() - epoch_) + 1; }

int HbmBackend::owner_of(const Digest& d, uint64_t up) const {
  if (devs_.size() == 1) return up & 1 ? 0 : -1;
  const uint64_t all = devs_.size() >= 64 ? ~0ull : (1ull << devs_.size()) - 1;
  if ((up & all) == all) return router_->owner(d);  // the span table: one load, two compares
  return ring_.owner(d, up);  // ketama ejection: the next live point
}

namespace {
thread_local uint64_t tl_spray_seq = 0;  // a reactor's stream position (sprayed objects)
thread_local uint32_t tl_sample_ctr = 0;
std::atomic<unsigned> g_sample_slot{0};
thread_local unsigned tl_sample_slot = g_sample_slot.fetch_add(1, std::memory_order_relaxed);
}  // namespace

int HbmBackend::route_get(const Digest& d) {
  const uint64_t up = up_mask_.load(std::memory_order_acquire);
  if (hot_on_) {
    if (((tl_sample_ctr++) & (uint32_t)(cfg_.hot_sample - 1)) == 0) sample_get(d);
    int r = -1;
    {
      const HostRouter::Read rd(*router_);
      const int hr = rd.hot_rank(d);
      if (hr != HostRouter::kNotHot) r = hr >= 0 ? hr : rd.spray(tl_spray_seq++);
    }
    if (r >= 0 && ((up & spread_mask_.load(std::memory_order_acquire)) >> r) & 1) {
      const int o = owner_of(d, up);
      if (r != o) hot_spread_gets_[tl_sample_slot % 16].v.fetch_add(1, std::memory_order_relaxed);
      return r;
    }
  }
  return owner_of(d, up);
}

void HbmBackend::sample_get(const Digest& d) {
  SampleStripe& st = samples_[tl_sample_slot % kSampleStripes];
  std::lock_guard<std::mutex> lk(st.mu);
  if (st.v.size() < (1u << 16)) st.v.push_back(d);  // bounded while no refresh drains it
}

void HbmBackend::enqueue(int k, Req r) {
  Dev& dv = *devs_[k];
  {
    std::lock_guard<std::mutex> lk(dv.mu);
    if (r.kind == ReqKind::Set && cfg_.presence_filter) {
      dv.filt->add(r.d);
      if (dv.filt_next) dv.filt_next->add(r.d);
    }
    // a write of an object being filled into this shard: the fill must not overwrite it
    if (is_write(r.kind) && !dv.filling.empty() && dv.filling.count(r.d.lo))
      dv.touched.insert(r.d.lo);
    // A purge names no digests, and the records of a refresh under way were read on their
    // owners before it: a fill queued behind it must not store them here after this shard
    // has scanned. Every object being filled counts as written (the fill drops its rows; a
    // replica that is missing reads as a miss and is written through again by the next SET).
    if (r.kind == ReqKind::Purge && !dv.filling.empty())
      dv.touched.insert(dv.filling.begin(), dv.filling.end());
    dv.q.push_back(std::move(r));
    dv.qn.store(dv.q.size(), std::memory_order_release);
  }
  if (!dv.spinning.load(std::memory_order_acquire)) dv.cv.notify_one();
}

void HbmBackend::enqueue_many(int k, std::vector<Req>& rs) {
  if (rs.empty()) return;
  Dev& dv = *devs_[k];
  {
    std::lock_guard<std::mutex> lk(dv.mu);
    for (auto& r : rs) dv.q.push_back(std::move(r));  // GETs only: no filter update
    dv.qn.store(dv.q.size(), std::memory_order_release);
  }
  rs.clear();
  if (!dv.spinning.load(std::memory_order_acquire)) dv.cv.notify_one();
}

void HbmBackend::get(const std::string& key, const Digest& d, Executor* ex, GetCallback done) {
  const int k = route_get(d);
  if (k < 0) {  // every shard ejected: the request falls through to the origin
    no_shard_misses_.fetch_add(1, std::memory_order_relaxed);
    done(false, CacheValue{});
    return;
  }
  Dev& dv = *devs_[k];
  if (devs_.size() > 1)
    dv.routed_gets[tl_sample_slot % Dev::kCtrShards].v.fetch_add(1, std::memory_order_relaxed);
  const bool restoring = dv.restoring.load(std::memory_order_acquire);
  if (cfg_.presence_filter && !restoring && !std::atomic_load(&dv.filt)->maybe(d)) {
    dv.filt_skips.fetch_add(1, std::memory_order_relaxed);  // never stored: no GPU batch
    done(false, CacheValue{});
    return;
  }
  Req r;
  r.kind = ReqKind::Get;
  r.d = d;
  r.key = key;
  r.ex = ex;
  r.gcb = std::move(done);
  // Reactor-direct: the calling reactor sends it to the edge server itself at the end of
  // its loop iteration (direct_service), unless a write or flush of this shard it must
  // stay ordered after has not finished on the GPU yet
  Direct* dc = tl_direct.be == this ? tl_direct.ctx : nullptr;
  if (dc && ex == dc->ex && !restoring && dv.flush_pend.load(std::memory_order_acquire) == 0 &&
      !writes_pending(d.lo)) {
    dc->dev[(size_t)k].pending.push_back(std::move(r));
    return;
  }
  enqueue(k, std::move(r));
}

void HbmBackend::get_part(const std::string& key, const Digest& d, const SliceSpec& spec,
                          Executor* ex, PartCallback done) {
  part_request(key, d, spec, nullptr, ex, std::move(done));
}

void HbmBackend::get_part_if(const std::string& key, const Digest& d, const SliceSpec& spec,
                             const PartCond& cond, Executor* ex, PartCallback done) {
  if (cond.kind == kCondNone) return part_request(key, d, spec, nullptr, ex, std::move(done));
  cond_slices_.fetch_add(1, std::memory_order_relaxed);
  part_request(key, d, spec, std::make_shared<const PartCond>(cond), ex, std::move(done));
}

void HbmBackend::part_request(const std::string& key, const Digest& d, const SliceSpec& spec,
                              std::shared_ptr<const PartCond> cond, Executor* ex,
                              PartCallback done) {
  slices_.fetch_add(1, std::memory_order_relaxed);
  const int k = route_get(d);
  if (k < 0) {  // every shard ejected
    no_shard_misses_.fetch_add(1, std::memory_order_relaxed);
    done(PartValue{});
    return;
  }
  Dev& dv = *devs_[k];
  if (devs_.size() > 1)
    dv.routed_gets[tl_sample_slot % Dev::kCtrShards].v.fetch_add(1, std::memory_order_relaxed);
  if (cfg_.presence_filter && !dv.restoring.load(std::memory_order_acquire) &&
      !std::atomic_load(&dv.filt)->maybe(d)) {
    dv.filt_skips.fetch_add(1, std::memory_order_relaxed);  // never stored: no GPU batch
    done(PartValue{});
    return;
  }
  Req r;
  r.kind = ReqKind::Slice;
  r.d = d;
  r.key = key;
  r.spec = spec;
  r.cond = std::move(cond);
  r.ex = ex;
  r.pcb = std::move(done);
  enqueue(k, std::move(r));  // (the batcher only: the edge server does not cut)
}

// A write goes to its owner and, for a hot object, is written through to every other shard in
// service (write_targets; the replicas must not outlive, or die before, the owner's copy).
// Each copy counts as pending (write_begin) until its flight is reaped or it is failed.
template <typename Arm>
bool HbmBackend::route_write(Req r, Arm&& arm) {
  // held until every copy is queued: a refresh's set_hot returns only after this
  std::optional<HostRouter::Read> rd;
  if (hot_on_) rd.emplace(*router_);
  const uint64_t up = up_mask_.load(std::memory_order_acquire);
  const int o = owner_of(r.d, up);
  if (o < 0) return false;
  const bool hot = rd && rd->hot_rank(r.d) != HostRouter::kNotHot;
  const WriteTargets to = write_targets(o, hot, up, (int)devs_.size());
  const auto send = [&](int shard, Req&& c) {
    arm(c, to.n, shard == o);
    write_begin(c.d.lo);
    enqueue(shard, std::move(c));
  };
  for (int i = 0; i + 1 < to.n; ++i) send(to.shard[i], Req(r));
  send(to.shard[to.n - 1], std::move(r));
  return true;
}

void HbmBackend::set(const std::string& key, const Digest& d, Bytes value, uint32_t flags,
                     uint32_t ttl_s) {
  if (!value || value->size() > cfg_.max_item || key.size() > kMaxKeyedKey) return;
  Req r;
  r.kind = ReqKind::Set;
  r.d = d;
  r.key = key;
  r.value = std::move(value);
  r.flags = flags;
  r.ttl = ttl_s;
  route_write(std::move(r), [](Req&, int, bool) {});  // (no shard in service: dropped)
}

// One answer: found anywhere, once every copy is gone.
void HbmBackend::del(const std::string& key, const Digest& d, Executor* ex, DelCallback done) {
  Req r;
  r.kind = ReqKind::Del;
  r.d = d;
  r.key = key;
  r.ex = ex;
  std::shared_ptr<FanIn<bool>> fan;
  const bool queued = route_write(std::move(r), [&](Req& c, int copies, bool is_owner) {
    if (copies == 1) {
      c.dcb = std::move(done);
      return;
    }
    if (!fan) fan = std::make_shared<FanIn<bool>>(copies, false, fan_any, std::move(done));
    c.dcb = FanIn<bool>::arm(fan, is_owner);
  });
  if (!queued && done) done(false);
}

// A touch is a write, routed like del(). The answer is the owner's, once every copy has
// answered.
void HbmBackend::touch(const std::string& key, const Digest& d, uint32_t ttl_s,
                       const uint32_t* flags, Executor* ex, TouchCallback done) {
  Req r;
  r.kind = ReqKind::Touch;
  r.d = d;
  r.key = key;
  r.ttl = ttl_s;
  r.has_flags = flags != nullptr;
  r.flags = flags ? *flags : 0u;
  r.ex = ex;
  std::shared_ptr<FanIn<int>> fan;
  const bool queued =
      key.size() <= kMaxKeyedKey &&  // (a longer key was never storable)
      route_write(std::move(r), [&](Req& c, int copies, bool is_owner) {
        if (copies == 1) {
          c.tcb = std::move(done);
          return;
        }
        if (!fan) fan = std::make_shared<FanIn<int>>(copies, 0, fan_owner, std::move(done));
        c.tcb = FanIn<int>::arm(fan, is_owner);
      });
  // no shard in service: not found
  if (!queued && done) PostGroups::answer_now(ex, [done] { done(0); });
}

void HbmBackend::enqueue_ctl(int k, std::function<void(bool)> cb) {
  Req r;
  r.kind = ReqKind::Barrier;
  r.d = Digest{0, 0};
  r.ccb = std::move(cb);
  enqueue(k, std::move(r));
}

void HbmBackend::purge_finish(const std::shared_ptr<Purge>& p) {
  if (p->left.fetch_sub(1, std::memory_order_acq_rel) != 1) return;
  purge_done_.fetch_add(1, std::memory_order_acq_rel);
  if (!p->cb) return;
  const int64_t n = p->removed.load(std::memory_order_relaxed);
  PostGroups::answer_now(p->ex, [cb = std::move(p->cb), n]() { cb(n); });
}

// Every shard scans its own index (a selector has no owner, and the hot replicas live on all
// of them): a Purge request per shard in service, launched by its batcher on the shard's
// stream behind the writes queued before it. A soft purge is the same request, fan-out,
// ordering, hot-replica and restore handling; only the launch differs (Dev::launch_purges). A
// shard that is out of service, or fails the purge, is marked so that its restore flushes it.
void HbmBackend::purge(const KeyedSelector& what, const PurgeAction& how, Executor* ex,
                       PurgeCallback done) {
  using Kind = KeyedSelector::Kind;
  if (purge_refused(what, how)) {
    if (done) PostGroups::answer_now(ex, [done]() { done(-1); });
    return;
  }
  if (how.soft && (what.kind == Kind::Prefix || what.kind == Kind::Exact))
    soft_purges_.fetch_add(1, std::memory_order_relaxed);
  if (what.kind == Kind::Tags) tag_purges_.fetch_add(1, std::memory_order_acq_rel);  // (before
  if (what.kind == Kind::Glob) glob_purges_.fetch_add(1, std::memory_order_acq_rel);  // started)
  purge_started_.fetch_add(1, std::memory_order_acq_rel);
  auto p = std::make_shared<Purge>();
  p->ex = ex;
  p->cb = std::move(done);
  p->left.store((int)devs_.size() + 1, std::memory_order_release);  // + this call's own hold
  Req proto;
  proto.kind = ReqKind::Purge;
  proto.d = Digest{0, 0};
  p->what = what;
  proto.what = std::shared_ptr<const KeyedSelector>(p, &p->what);
  proto.how = how;
  proto.purge = p;
  const uint64_t up = up_mask_.load(std::memory_order_acquire);
  for (size_t k = 0; k < devs_.size(); ++k) {
    Dev* dv = devs_[k].get();
    if (!((up >> k) & 1)) {
      dv->purge_dirty.store(true, std::memory_order_release);
      // Back in service meanwhile? Its restore may have taken its last look at the flag
      // before the store above: then it scans like the others (a request queued to a shard
      // that is up runs after the restore, on its batcher).
      if (!dv->up()) {
        purge_finish(p);
        continue;
      }
    }
    Req r = proto;
    r.ccb = [this, p, dv](bool ok) {
      if (!ok) dv->purge_dirty.store(true, std::memory_order_release);
      purge_finish(p);
    };
    enqueue((int)k, std::move(r));
  }
  purge_finish(p);
}

// Inspection: the shards are visited in order, one request at a time (list_next_ask), each
// queued to its shard's batcher behind the writes queued before it. A shard out of service
// is skipped and counted; so is one whose flight fails.
void HbmBackend::list_objects(const ListQuery& q, Executor* ex, ListCallback done) {
  if (!done) return;
  auto w = std::make_shared<ListWalk>();
  w->q = q;
  w->ex = ex;
  w->cb = std::move(done);
  const bool cursor_ok = q.after.empty() || hbm_cursor_parse(q.after, (int)devs_.size(),
                                                              &w->cur_shard, &w->cur_slot);
  if (!list_query_valid(q) || !cursor_ok) {
    ListResult bad;
    bad.ok = list_query_valid(q);
    bad.bad_cursor = !cursor_ok;
    PostGroups::answer_now(ex, [cb = std::move(w->cb), bad]() { cb(bad); });
    return;
  }
  lists_.fetch_add(1, std::memory_order_relaxed);
  w->res.ok = true;
  list_step(std::move(w));
}

void HbmBackend::list_step(std::shared_ptr<ListWalk> w) {
  for (;;) {
    const uint32_t got = (uint32_t)w->res.objects.size();
    const ListAsk a = list_next_ask(w->shard, w->cur_shard, w->cur_slot, w->have_next,
                                    w->q.limit > got ? w->q.limit - got : 0,
                                    up_mask_.load(std::memory_order_acquire), (int)devs_.size());
    w->res.shards_skipped += a.skipped;
    if (a.shard < 0) {
      PostGroups::answer_now(w->ex, [w]() { w->cb(std::move(w->res)); });
      return;
    }
    w->shard = a.shard;
    w->asked = a.limit;
    Dev* const dv = devs_[(size_t)a.shard].get();
    const uint64_t nslots = dv->cache->config().nbuckets * kEntriesPerBucket;
    if (a.start > nslots) {  // (a cursor from another geometry: nothing follows on this shard)
      w->asked = 0;
    }
    Req r;
    r.kind = ReqKind::List;
    r.d = Digest{0, 0};
    r.list = w;
    r.flags = w->asked;
    r.list_start = a.start > nslots ? 0 : a.start;
    r.ccb = [this, w](bool ok) {
      if (!ok) ++w->res.shards_skipped;
      list_step(w);
    };
    enqueue(a.shard, std::move(r));
    return;
  }
}

void HbmBackend::flush() {
  for (auto& d : devs_) {
    {
      std::lock_guard<std::mutex> lk(d->mu);
      if (!d->flush_req) d->flush_pend.fetch_add(1, std::memory_order_acq_rel);
      d->flush_req = true;
      d->ctl_pending.store(true, std::memory_order_release);
    }
    d->cv.notify_one();
  }
}

bool HbmBackend::inject_shard_down(int shard, bool down) {
  if (shard < 0 || shard >= (int)devs_.size()) return false;
  Dev& dv = *devs_[shard];
  dv.forced_down.store(down, std::memory_order_release);
  if (down) {
    dv.eject_gen.fetch_add(1, std::memory_order_acq_rel);
    dv.set_up(false);
    spread_mask_.fetch_and(~(1ull << shard), std::memory_order_acq_rel);  // replicas suspect
    dv.ejections++;
  }
  {
    std::lock_guard<std::mutex> lk(dv.mu);
    dv.kick = true;
  }
  dv.cv.notify_one();  // the batcher restores the shard (flushing it) when forced_down clears
  return true;
}

int HbmBackend::peer_path(int src_dev, int dst_dev) const {
  if (cfg_.peer_copy == "staged") return 2;  // forced (tests run it with one GPU)
  if (src_dev == dst_dev) return 0;
  const size_t nd = devs_.size();
  size_t si = nd, di = nd;
  for (size_t i = 0; i < nd; ++i) {
    if (devs_[i]->device == src_dev) si = i;
    if (devs_[i]->device == dst_dev) di = i;
  }
  return si < nd && di < nd && peer_ok_[si * nd + di] ? 1 : 2;
}

void HbmBackend::stats(StatList* out) {
  CacheCounters t{};
  uint64_t hbm = 0;
  auto sum = [&](std::atomic<uint64_t> Dev::*m) {
    uint64_t s = 0;
    for (auto& d : devs_) s += ((*d).*m).load();
    return s;
  };
  for (auto& d : devs_) {
    (void)hipSetDevice(d->device);
    // a stream of its own, non-blocking: the batcher's may be busy, and the legacy null
    // stream would also wait for the resident edge server; counters are advisory
    const CacheCounters c = d->cache->counters(d->sstream);
    t.get_ops += c.get_ops; t.get_hits += c.get_hits; t.set_ops += c.set_ops;
    t.set_bytes += c.set_bytes; t.set_evicted += c.set_evicted; t.del_ops += c.del_ops;
    t.reinserted += c.reinserted; t.reinsert_bytes += c.reinsert_bytes;
    t.touched += c.touched;
    hbm += d->cache->hbm_bytes();
  }
  out->emplace_back("cache_get_ops", t.get_ops);
  out->emplace_back("cache_get_hits", t.get_hits);
  out->emplace_back("cache_set_ops", t.set_ops);
  out->emplace_back("cache_set_bytes", t.set_bytes);
  out->emplace_back("cache_evicted", t.set_evicted);
  out->emplace_back("cache_reinserted", t.reinserted);
  out->emplace_back("cache_reinsert_bytes", t.reinsert_bytes);
  out->emplace_back("hbm_gpus", devs_.size());
  out->emplace_back("hbm_gpus_up", (uint64_t)__builtin_popcountll(up_mask_.load()));
  out->emplace_back("hbm_bytes", hbm);
  out->emplace_back("hbm_pipeline_depth", (uint64_t)cfg_.depth);
  out->emplace_back("hbm_batches", sum(&Dev::batches));
  out->emplace_back("hbm_batched_requests", sum(&Dev::batched_reqs));
  uint64_t mb = 0;
  for (auto& d : devs_) mb = std::max<uint64_t>(mb, d->max_batch.load());
  out->emplace_back("hbm_max_batch", mb);
  out->emplace_back("hbm_batch_ns_total", sum(&Dev::batch_ns));
  out->emplace_back("hbm_sweeps", sum(&Dev::sweeps));
  out->emplace_back("hbm_live_objects", sum(&Dev::live_objects));
  out->emplace_back("hbm_live_bytes", sum(&Dev::live_bytes));
  out->emplace_back("hbm_coalesced_gets", sum(&Dev::coalesced));
  out->emplace_back("hbm_key_mismatch", sum(&Dev::key_mismatch));
  out->emplace_back("hbm_failures", sum(&Dev::failures));
  out->emplace_back("hbm_ejections", sum(&Dev::ejections));
  out->emplace_back("hbm_restores", sum(&Dev::restores));
  out->emplace_back("hbm_regathers", sum(&Dev::regathers));
  out->emplace_back("hbm_arena_misses", sum(&Dev::arena_misses));
  out->emplace_back("hbm_served_batches", sum(&Dev::served_batches));
  out->emplace_back("hbm_ordered_get_batches", sum(&Dev::ordered_gets));
  out->emplace_back("hbm_direct_jobs", sum(&Dev::direct_jobs));
  out->emplace_back("hbm_direct_requests", sum(&Dev::direct_reqs));
  out->emplace_back("hbm_direct_fallback_requests", sum(&Dev::direct_fallbacks));
  out->emplace_back("hbm_direct_overflows", sum(&Dev::direct_overflows));
  out->emplace_back("hbm_direct_timeouts", sum(&Dev::direct_timeouts));
  // submit -> completion seen by the reactor, summed over jobs
  out->emplace_back("hbm_direct_job_ns_total", sum(&Dev::direct_ns));
  uint64_t sl = 0;
  for (auto& d : devs_) sl += d->cache->serve_launches();
  out->emplace_back("hbm_server_launches", sl);
  out->emplace_back("hbm_staged_peer_copies", sum(&Dev::staged_copies));
  uint64_t direct = 0;
  for (uint8_t v : peer_ok_) direct += v;
  out->emplace_back("hbm_peer_pairs_direct", direct);
  out->emplace_back("hbm_migrated", sum(&Dev::migrated));
  out->emplace_back("hbm_migrate_ns", sum(&Dev::migrate_ns));
  out->emplace_back("hbm_dropped_sets", sum(&Dev::dropped));
  // (prefix purges, hard and soft: the tag purges among the calls begun are counted apart)
  const uint64_t begun = purge_started_.load(), by_tag = tag_purges_.load();
  const uint64_t by_glob = glob_purges_.load(), apart = by_tag + by_glob;
  out->emplace_back("hbm_purges", begun - (apart < begun ? apart : begun));
  out->emplace_back("hbm_purged_objects", sum(&Dev::purged_objects));
  out->emplace_back("hbm_purged_bytes", sum(&Dev::purged_bytes));
  out->emplace_back("hbm_soft_purges", soft_purges_.load());
  out->emplace_back("hbm_softened_objects", sum(&Dev::softened_objects));
  out->emplace_back("hbm_tag_purges", by_tag);
  out->emplace_back("hbm_lists", lists_.load());
  out->emplace_back("hbm_slices", slices_.load());
  out->emplace_back("hbm_cond_slices", cond_slices_.load());
  out->emplace_back("hbm_tag_purged_objects", sum(&Dev::tag_purged_objects));
  out->emplace_back("hbm_tag_softened_objects", sum(&Dev::tag_softened_objects));
  out->emplace_back("hbm_glob_purges", by_glob);
  out->emplace_back("hbm_glob_purged_objects", sum(&Dev::glob_purged_objects));
  out->emplace_back("hbm_glob_softened_objects", sum(&Dev::glob_softened_objects));
  // touch requests taken, and the entries the shards' kernels updated (replicas included)
  out->emplace_back("hbm_touches", sum(&Dev::touch_reqs));
  out->emplace_back("hbm_touched", t.touched);
  out->emplace_back("hbm_no_shard_misses", no_shard_misses_.load());
  // per-shard GET routing (the load hot-object spreading evens out) and the hot set
  for (size_t i = 0; i < devs_.size(); ++i)
    out->emplace_back("hbm_shard_gets_" + std::to_string(i), devs_[i]->routed_total());
  out->emplace_back("hbm_hot_spreading", hot_on_ ? 1 : 0);
  if (hot_on_) {
    out->emplace_back("hbm_hot_objects", hot_objects_.load());
    out->emplace_back("hbm_hot_refreshes", hot_refreshes_.load());
    out->emplace_back("hbm_hot_added", hot_added_.load());
    out->emplace_back("hbm_hot_removed", hot_removed_.load());
    out->emplace_back("hbm_hot_deferred", hot_deferred_.load());
    out->emplace_back("hbm_hot_filled_rows", hot_filled_.load());
    out->emplace_back("hbm_hot_fill_skipped_rows", hot_fill_skipped_.load());
    out->emplace_back("hbm_hot_fill_failures", hot_fill_failed_.load());
    out->emplace_back("hbm_hot_fill_bytes", hot_fill_bytes_.load());
    out->emplace_back("hbm_hot_replicas_dropped", hot_dropped_replicas_.load());
    uint64_t sg = 0;
    for (const SpreadCtr& c : hot_spread_gets_) sg += c.v.load(std::memory_order_relaxed);
    out->emplace_back("hbm_hot_spread_gets", sg);
    out->emplace_back("hbm_hot_samples", hot_samples_.load());
    out->emplace_back("hbm_hot_spread_mask", spread_mask_.load());
    out->emplace_back("hbm_hot_refresh_us_last", hot_refresh_us_.load());
    out->emplace_back("hbm_hot_router_tables", router_->publications());
  }
  uint64_t arena = 0, aallocs = 0, afrees = 0, amax = 0;
  for (auto& d : devs_) {
    amax = std::max<uint64_t>(amax, d->pool->alloc_max_us());
    arena += d->pool->allocated();
    aallocs += d->pool->allocs();
    afrees += d->pool->frees();
  }
  out->emplace_back("hbm_arena_bytes", arena);
  out->emplace_back("hbm_arena_allocs", aallocs);
  out->emplace_back("hbm_arena_frees", afrees);
  out->emplace_back("hbm_arena_alloc_max_us", amax);
  if (cfg_.presence_filter) {
    uint64_t adds = 0;
    for (auto& d : devs_) adds += std::atomic_load(&d->filt)->adds();
    out->emplace_back("hbm_filter_skips", sum(&Dev::filt_skips));
    out->emplace_back("hbm_filter_rebuilds", sum(&Dev::filt_rebuilds));
    out->emplace_back("hbm_filter_adds", adds);
    out->emplace_back("hbm_filter_fill_ppm",
                      (uint64_t)(std::atomic_load(&devs_[0]->filt)->fill() * 1e6));
  }
}

}  // namespace shellac
