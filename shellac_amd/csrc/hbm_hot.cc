// HbmBackend's hot-object spreading: the reference's
// ketama client sends each key to one node (src/python/shellac/server/Server.py:81-83), so a
// hot key loads one GPU. The hot set follows a sampled GET stream; its objects are replicated
// on every shard in service and their GETs spread by the router's designation / spray
// (HbmBackend::route_get, backend_hbm.cc). This file is the refresh: the thread and the
// protocol that moves the replicated set from one plan to the next.
#include <pthread.h>

#include "hbm_backend_impl.h"

namespace shellac {

void HbmBackend::hot_loop() {
  pthread_setname_np(pthread_self(), "shellac-hot");
  std::unique_lock<std::mutex> lk(hot_th_mu_);
  while (!hot_stop_) {
    hot_cv_.wait_for(lk, std::chrono::milliseconds(cfg_.hot_refresh_ms), [&] { return hot_stop_; });
    if (hot_stop_) break;
    lk.unlock();
    try {
      hot_refresh();
    } catch (const std::exception& e) {
      std::fprintf(stderr, "[shellac hbm] hot-set refresh failed: %s\n", e.what());
    }
    lk.lock();
  }
}

StatList HbmBackend::hot_refresh() {
  std::lock_guard<std::mutex> lk(hot_mu_);
  return hot_refresh_locked();
}

namespace {
// waits for n completion callbacks (barriers, fills); ok[i] per callback index
struct Waiter {
  std::mutex mu;
  std::condition_variable cv;
  int left = 0;
  std::vector<int> ok;  // 1 ok, 0 failed, -1 pending
  explicit Waiter(int n) : left(n), ok((size_t)n, -1) {}
  // callback i (it keeps the waiter alive: a request may outlive the refresh's wait)
  static std::function<void(bool)> cb(const std::shared_ptr<Waiter>& w, int i) {
    return [w, i](bool good) {
      std::lock_guard<std::mutex> lk(w->mu);
      w->ok[(size_t)i] = good ? 1 : 0;
      if (--w->left == 0) w->cv.notify_all();
    };
  }
  bool wait(int timeout_ms) {
    std::unique_lock<std::mutex> lk(mu);
    return cv.wait_for(lk, std::chrono::milliseconds(timeout_ms), [&] { return left == 0; });
  }
  int state(int i) {
    std::lock_guard<std::mutex> lk(mu);
    return ok[(size_t)i];
  }
};
}  // namespace

// One refresh's state; its member functions are the protocol's steps, run once each and in
// order by hot_refresh_locked().
struct HbmBackend::HotRefresh {
  explicit HotRefresh(HbmBackend& b) : be(b), N((int)b.devs_.size()), t_start(wall_s()) {}
  HbmBackend& be;
  const int N;
  const double t_start;
  StatList out;
  uint64_t up = 0;  // the shards in service when the refresh planned
  HotPlan plan;
  std::unordered_map<Digest, int32_t, DigestHash, DigestEq> cur;  // the published set's ranks
  DigestSet added;                 // planned and not in the published set
  uint64_t mask0 = 0, heal = 0;    // shards holding the replicas; in service and holding none
  std::vector<uint64_t> gen0;      // the shards' eject_gen at the start
  std::vector<Digest> fill_objs;   // objects to snapshot, hottest first
  uint32_t t = 0;
  int wait_ms = 0;
  std::vector<std::vector<Digest>> by_owner;  // fill_objs by the shard their record is read on
  uint64_t bad = 0;                // shards that failed a barrier, a snapshot or a fill
  struct Snap {
    std::vector<Digest> keys;
    std::vector<uint64_t> size, off;
    uint64_t total = 0;
  };
  std::vector<Snap> snap;          // per owner: its records in Dev::hs
  DigestSet deferred;              // added objects over the fill budget
  std::vector<std::shared_ptr<HotFill>> fills;  // per target shard
  std::vector<int> tgt;            // the shards with a fill queued
  std::shared_ptr<Waiter> fill_wait;
  uint64_t fill_bytes = 0;
  HotTable table;                  // T2
  DigestSet fin;                   // its objects
  std::vector<Digest> gone;        // objects that left the set
  uint64_t dropped = 0;            // their replicas deleted

  Dev& dev(int r) { return *be.devs_[(size_t)r]; }
  bool fold_samples();
  void make_plan();
  void start_recording();
  void publish_t1();
  void barrier_owners();
  void snapshot_owners();
  void budget();
  void queue_fills();
  std::shared_ptr<HotFill> stage_fill(int r);
  void await_fills();
  void stop_recording();
  void publish_t2();
  void drop_cooled();
  void count();
};

// One refresh. The order keeps every GET answered by a copy no older than the last SET /
// DELETE that finished before the GET began (HotSpread's refresh_hot, single process):
//  1. fold the sampled GETs into the decayed counts;
//  2. plan the new hot set from them (plan_hot: top hot_objects, designated greedily from
//     the owners' cold loads, the hottest sprayed);
//  3. every shard in service starts recording writes of the objects about to be filled
//     (Dev::filling / touched);
//  4. router table T1 = the current hot set + the new objects designated to their owners:
//     the new objects' SETs / DELETEs are written through from here on, their GETs still go
//     to their owners. set_hot returns once nothing routes under the old table, so every
//     write routed owner-only has been queued;
//  5. a barrier on each owner: those writes have finished on its GPU;
//  6. the owners look the objects up and gather their records (one snapshot per owner);
//  7. the new objects beyond the fill budget are deferred to a later refresh;
//  8. per target shard, the records of the objects it does not own go over xGMI into its
//     staging (copy_between: hipMemcpyPeerAsync, or staged through pinned host memory) and
//     a fill request is queued behind the shard's writes; the batcher drops the rows with
//     a write queued since step 3 (that copy is newer) and stores the rest;
//  9. wait for every fill;
// 10. stop recording;
// 11. the shards that now hold the whole set join the spread mask, and T2 = the new hot set
//     with its designations is published;
// 12. objects that left the set lose their non-owner replicas (deleted: no SET reaches
//     them any more, and a later promotion must find no stale copy);
// 13. counters.
// Shards that are down, or eject mid-refresh, drop out of the spread mask (a restored
// shard is flushed and rejoins with a full fill at the next refresh).
StatList HbmBackend::hot_refresh_locked() {
  if (!hot_on_) return {};
  TraceRange tr("hbm_backend.hot_refresh");
  HotRefresh r(*this);
  if (!r.fold_samples()) return r.out;  // too few samples yet
  r.make_plan();
  r.start_recording();
  r.publish_t1();
  r.barrier_owners();
  r.snapshot_owners();
  r.budget();
  r.queue_fills();
  r.await_fills();
  r.stop_recording();
  r.publish_t2();
  r.drop_cooled();
  r.count();
  return r.out;
}

// ---- 1. samples -> decayed counts
bool HbmBackend::HotRefresh::fold_samples() {
  uint64_t nsamp = 0;
  for (int i = 0; i < kSampleStripes; ++i) {
    std::vector<Digest> v;
    {
      std::lock_guard<std::mutex> lk(be.samples_[i].mu);
      v.swap(be.samples_[i].v);
    }
    nsamp += v.size();
    for (const Digest& d : v) {
      auto it = be.hot_counts_.find(d);
      if (it != be.hot_counts_.end()) ++it->second;
      else if (be.hot_counts_.size() < (1u << 18)) be.hot_counts_.emplace(d, 1);
    }
  }
  be.hot_samples_.fetch_add(nsamp, std::memory_order_relaxed);
  uint64_t total = 0;
  for (const auto& kv : be.hot_counts_) total += kv.second;
  out.emplace_back("samples", total);
  if (total >= be.cfg_.hot_min_samples) return true;
  out.emplace_back("skipped", 1);
  return false;
}

// ---- 2. the plan, and what it changes
void HbmBackend::HotRefresh::make_plan() {
  up = be.up_mask_.load(std::memory_order_acquire);
  std::vector<std::pair<Digest, uint64_t>> counts(be.hot_counts_.begin(), be.hot_counts_.end());
  for (auto it = be.hot_counts_.begin(); it != be.hot_counts_.end();) {  // halve: recent traffic rules
    it->second >>= 1;
    if (!it->second) it = be.hot_counts_.erase(it);
    else ++it;
  }
  const double above = be.cfg_.hot_spray_above > 0 ? be.cfg_.hot_spray_above : 1.0 / (4.0 * N);
  for (size_t i = 0; i < be.hot_set_.size(); ++i) cur.emplace(be.hot_set_[i], be.hot_rank_[i]);
  // hysteresis: an object already replicated stays unless a new one is twice as hot (the
  // set's tail would otherwise churn on sampling noise: a fill and a delete per object)
  const std::function<bool(const Digest&)> sticky = [&](const Digest& d) { return cur.count(d) > 0; };
  plan = plan_hot(counts, be.cfg_.hot_objects, N, up,
                  [&](const Digest& d) { return be.owner_of(d, up); }, above, 2, &sticky, 2.0);
  for (const Digest& d : plan.hot)
    if (!cur.count(d)) added.insert(d);
  mask0 = be.spread_mask_.load(std::memory_order_acquire) & up;
  heal = up & ~mask0;  // in service, holding no replicas yet (restored, new)
  gen0.resize((size_t)N);
  for (int r = 0; r < N; ++r) gen0[(size_t)r] = dev(r).eject_gen.load();
  // objects to snapshot, hottest first: the new ones, and every planned one for a heal
  for (const Digest& d : plan.hot)
    if (heal || added.count(d)) fill_objs.push_back(d);
}

// ---- 3. record writes of those objects on every shard in service
void HbmBackend::HotRefresh::start_recording() {
  for (int r = 0; r < N; ++r) {
    if (!((up >> r) & 1)) continue;
    Dev& dv = dev(r);
    std::lock_guard<std::mutex> lk(dv.mu);
    dv.filling.clear();
    dv.touched.clear();
    for (const Digest& d : fill_objs) dv.filling.insert(d.lo);
  }
  // A purge already under way may have reached some shards before the recording began and
  // reach the owners only after their barrier: nothing is filled this time (a purge that
  // starts from here on marks the objects itself, in enqueue()).
  const uint64_t done = be.purge_done_.load(std::memory_order_acquire);
  if (be.purge_started_.load(std::memory_order_acquire) != done)
    for (int r = 0; r < N; ++r) {
      Dev& dv = dev(r);
      std::lock_guard<std::mutex> lk(dv.mu);
      dv.touched.insert(dv.filling.begin(), dv.filling.end());
    }
}

// ---- 10.
void HbmBackend::HotRefresh::stop_recording() {
  for (auto& dv : be.devs_) {
    std::lock_guard<std::mutex> lk(dv->mu);
    dv->filling.clear();
    dv->touched.clear();
  }
}

// ---- 4. T1: write-through for the new objects, their GETs at their owners (nothing new:
// the published table already is T1)
void HbmBackend::HotRefresh::publish_t1() {
  if (!added.empty()) {
    std::vector<Digest> h(be.hot_set_);
    std::vector<int32_t> rk(be.hot_rank_);
    for (const Digest& d : plan.hot)
      if (added.count(d)) {
        h.push_back(d);
        rk.push_back(be.owner_of(d, up));
      }
    be.router_->set_hot(h.data(), (int64_t)h.size(), rk.data(), be.hot_weights_.data());
  }
  t = be.now();
  wait_ms = 2 * be.cfg_.batch_timeout_ms + 1000;
}

// ---- 5. barrier on every owner (source) of an object to fill
// (an object of the current set owned by a shard being healed is read from a shard that
// holds its replica: the healed one was flushed, and warm restore leaves hot objects be)
void HbmBackend::HotRefresh::barrier_owners() {
  int replica_src = -1;
  for (int r = 0; r < N && replica_src < 0; ++r)
    if ((mask0 >> r) & 1) replica_src = r;
  by_owner.resize((size_t)N);
  for (const Digest& d : fill_objs) {
    int o = be.owner_of(d, up);
    if (o >= 0 && ((heal >> o) & 1) && replica_src >= 0 && cur.count(d)) o = replica_src;
    if (o >= 0) by_owner[(size_t)o].push_back(d);
  }
  std::vector<int> who;
  for (int o = 0; o < N; ++o)
    if (!by_owner[(size_t)o].empty()) who.push_back(o);
  auto w = std::make_shared<Waiter>((int)who.size());
  for (size_t i = 0; i < who.size(); ++i) be.enqueue_ctl(who[i], Waiter::cb(w, (int)i));
  w->wait(wait_ms);
  for (size_t i = 0; i < who.size(); ++i)
    if (w->state((int)i) != 1) {
      bad |= 1ull << who[i];
      by_owner[(size_t)who[i]].clear();  // its objects are not filled this time
    }
}

// ---- 6. snapshot on each owner
void HbmBackend::HotRefresh::snapshot_owners() {
  snap.resize((size_t)N);
  for (int o = 0; o < N; ++o) {
    Snap& sn = snap[(size_t)o];
    sn.keys = by_owner[(size_t)o];
    const int64_t m = (int64_t)sn.keys.size();
    if (!m) continue;
    Dev& od = dev(o);
    try {
      HB_OK(hipSetDevice(od.device));
      Digest* sk = od.hs.keys.ensure<Digest>((size_t)m * sizeof(Digest));
      uint64_t* sloc = od.hs.loc.ensure<uint64_t>((size_t)m * 8);
      uint64_t* ssz = od.hs.size.ensure<uint64_t>((size_t)(m + 1) * 8);
      uint64_t* soff = od.hs.off.ensure<uint64_t>((size_t)(m + 1) * 8);
      HB_OK(hipMemcpyAsync(sk, sn.keys.data(), (size_t)m * sizeof(Digest), hipMemcpyHostToDevice,
                           od.mstream));
      od.cache->lookup(sk, m, sloc, ssz, soff, t, od.mstream, od.cache->config().log_bytes / 8);
      sn.size.assign((size_t)m + 1, 0);
      sn.off.assign((size_t)m + 1, 0);
      HB_OK(hipMemcpyAsync(sn.size.data(), ssz, (size_t)m * 8, hipMemcpyDeviceToHost, od.mstream));
      HB_OK(hipMemcpyAsync(sn.off.data(), soff, (size_t)(m + 1) * 8, hipMemcpyDeviceToHost,
                           od.mstream));
      HB_OK(hipStreamSynchronize(od.mstream));
      sn.total = sn.off[(size_t)m];
      if (sn.total) {
        uint8_t* srec = od.hs.rec.ensure<uint8_t>(sn.total + 16);
        od.cache->gather(sloc, soff, m, srec, od.mstream);
        HB_OK(hipStreamSynchronize(od.mstream));
      }
    } catch (const std::exception& e) {
      std::fprintf(stderr, "[shellac hbm] hot snapshot on gpu %d failed: %s\n", od.device, e.what());
      bad |= 1ull << o;
      sn = Snap{};
    }
  }
}

// ---- 7. budget: new objects hottest first, (targets) x record bytes each
void HbmBackend::HotRefresh::budget() {
  std::unordered_map<Digest, uint64_t, DigestHash, DigestEq> rec;
  for (const Snap& sn : snap)
    for (size_t i = 0; i < sn.keys.size(); ++i) rec[sn.keys[i]] = sn.size[i];
  const auto rec_bytes = [&](const Digest& d) {
    const auto it = rec.find(d);
    return it == rec.end() ? uint64_t(0) : it->second;
  };
  deferred = hot_fill_deferred(plan.hot, added, rec_bytes,
                               (uint64_t)std::max(1, __builtin_popcountll(up) - 1),
                               be.cfg_.hot_fill_budget);
}

// ---- 8. fills, one per target shard: staged, then queued behind the shard's writes
void HbmBackend::HotRefresh::queue_fills() {
  if (be.before_fill_) {  // tests: between the owners' snapshots and the fills
    std::function<void()> fn;
    fn.swap(be.before_fill_);
    fn();
  }
  fills.resize((size_t)N);
  for (int r = 0; r < N; ++r) {
    if (!((up >> r) & 1) || ((bad >> r) & 1)) continue;
    fills[(size_t)r] = stage_fill(r);
    if (fills[(size_t)r]) tgt.push_back(r);
  }
  fill_wait = std::make_shared<Waiter>((int)tgt.size());
  for (size_t i = 0; i < tgt.size(); ++i) {
    Req q;
    q.kind = ReqKind::Fill;
    q.d = Digest{0, 0};
    q.fill = fills[(size_t)tgt[i]];
    q.ccb = Waiter::cb(fill_wait, (int)i);
    be.enqueue(tgt[i], std::move(q));
  }
}

// Shard r's fill, staged on its GPU (null: it takes no copy, or staging failed): every
// snapshot row of the other owners; size 0 where this shard takes no copy
std::shared_ptr<HbmBackend::HotFill> HbmBackend::HotRefresh::stage_fill(int r) {
  const bool full = (heal >> r) & 1;
  int64_t m = 0;
  uint64_t bytes = 0;
  for (int o = 0; o < N; ++o)
    if (o != r && snap[(size_t)o].total) {
      m += (int64_t)snap[(size_t)o].keys.size();
      bytes += snap[(size_t)o].total;
    }
  if (!m) return nullptr;
  Dev& td = dev(r);
  auto h = std::make_shared<HotFill>();
  try {
    HB_OK(hipSetDevice(td.device));
    Digest* kk = td.hf.keys.ensure<Digest>((size_t)m * sizeof(Digest));
    uint8_t* krec = td.hf.rec.ensure<uint8_t>(bytes + 16);
    uint64_t* koff = td.hf.off.ensure<uint64_t>((size_t)(m + 1) * 8);
    h->okeys = td.hf.okeys.ensure<Digest>((size_t)m * sizeof(Digest));
    h->ovoff = td.hf.voff.ensure<uint64_t>((size_t)m * 8);
    h->ometa = td.hf.meta.ensure<uint32_t>((size_t)m * 12);
    td.hf.size.ensure((size_t)(m + 1) * 8);
    std::vector<Digest> keys;
    std::vector<uint64_t> off;
    keys.reserve((size_t)m);
    off.reserve((size_t)m + 1);
    h->hsize = td.hf.size.host<uint64_t>();
    h->dsize = td.hf.size.dev<uint64_t>();
    uint64_t base = 0;
    int64_t row = 0;
    for (int o = 0; o < N; ++o) {
      const Snap& sn = snap[(size_t)o];
      if (o == r || !sn.total) continue;
      Dev& od = dev(o);
      copy_between(krec + base, td.device, od.hs.rec.p, od.device, sn.total, td.mstream,
                   be.peer_path(od.device, td.device));
      if (be.peer_path(od.device, td.device) == 2) td.staged_copies++;
      for (size_t i = 0; i < sn.keys.size(); ++i, ++row) {
        const Digest& d = sn.keys[i];
        keys.push_back(d);
        off.push_back(base + sn.off[i]);
        const bool want = (full || added.count(d)) && !deferred.count(d);
        h->hsize[row] = want ? sn.size[i] : 0;
        h->lo.push_back(d.lo);
        if (want && sn.size[i]) fill_bytes += sn.size[i];
      }
      base += sn.total;
    }
    off.push_back(base);
    HB_OK(hipMemcpyAsync(kk, keys.data(), (size_t)m * sizeof(Digest), hipMemcpyHostToDevice,
                         td.mstream));
    HB_OK(hipMemcpyAsync(koff, off.data(), (size_t)(m + 1) * 8, hipMemcpyHostToDevice,
                         td.mstream));
    HB_OK(hipStreamSynchronize(td.mstream));
    h->m = m;
    h->kk = kk;
    h->krec = krec;
    h->koff = koff;
    h->bound = bytes + 48 * (uint64_t)m;
    if (be.cfg_.presence_filter) {  // GETs spread here must not skip the replicas
      std::lock_guard<std::mutex> lk(td.mu);
      for (int64_t i = 0; i < m; ++i)
        if (h->hsize[i]) {
          td.filt->add(keys[(size_t)i]);
          if (td.filt_next) td.filt_next->add(keys[(size_t)i]);
        }
    }
  } catch (const std::exception& e) {
    std::fprintf(stderr, "[shellac hbm] hot fill staging on gpu %d failed: %s\n", td.device,
                 e.what());
    bad |= 1ull << r;
    return nullptr;
  }
  return h;
}

// ---- 9. every fill has finished, failed, or is given up on
void HbmBackend::HotRefresh::await_fills() {
  Waiter& w = *fill_wait;
  if (!w.wait(wait_ms)) {
    // a shard that never got to its fill: cancel it if not launched (else it completes
    // with its touched check made in time, and only its buffers must outlive it)
    for (size_t i = 0; i < tgt.size(); ++i) {
      if (w.state((int)i) != -1) continue;
      Dev& td = dev(tgt[i]);
      std::lock_guard<std::mutex> lk(td.mu);
      HotFill& h = *fills[(size_t)tgt[i]];
      if (!h.launched) h.cancelled = true;
      else td.hf.abandon();  // still running on the GPU
    }
  }
  uint64_t rows = 0, skipped = 0;
  for (size_t i = 0; i < tgt.size(); ++i) {
    const int r = tgt[i];
    if (w.state((int)i) != 1) {
      bad |= 1ull << r;
      be.hot_fill_failed_.fetch_add(1, std::memory_order_relaxed);
      continue;
    }
    Dev& td = dev(r);
    std::lock_guard<std::mutex> lk(td.mu);
    rows += fills[(size_t)r]->rows;
    skipped += fills[(size_t)r]->skipped;
  }
  be.hot_filled_.fetch_add(rows, std::memory_order_relaxed);
  be.hot_fill_skipped_.fetch_add(skipped, std::memory_order_relaxed);
  out.emplace_back("filled_rows", rows);
  out.emplace_back("fill_skipped_rows", skipped);
}

// ---- 11. the spread mask, then T2
void HbmBackend::HotRefresh::publish_t2() {
  uint64_t mask = (mask0 | heal) & ~bad;
  for (int r = 0; r < N; ++r)
    if (dev(r).eject_gen.load() != gen0[(size_t)r]) mask &= ~(1ull << r);
  // an added object is spread only if its owner's snapshot held (the owner did not fail)
  DigestSet snapshot_ok;
  for (const Snap& sn : snap) snapshot_ok.insert(sn.keys.begin(), sn.keys.end());
  table = hot_final_table(plan, added, deferred, snapshot_ok, mask, N);
  be.spread_mask_.store(mask, std::memory_order_release);
  for (int r = 0; r < N; ++r)  // an ejection that raced the store above
    if (dev(r).eject_gen.load() != gen0[(size_t)r] || !dev(r).up())
      be.spread_mask_.fetch_and(~(1ull << r), std::memory_order_acq_rel);
  // (an unchanged table is not republished)
  if (!(added.empty() && table.same_as(be.hot_set_, be.hot_rank_, be.hot_weights_)))
    be.router_->set_hot(table.hot.data(), (int64_t)table.hot.size(), table.rank.data(),
                        table.wts.data());
  fin.insert(table.hot.begin(), table.hot.end());
}

// ---- 12. replicas of objects no longer hot (the old set and this refresh's write-through
// set minus the new one) go from every shard but their owner
void HbmBackend::HotRefresh::drop_cooled() {
  for (const Digest& d : be.hot_set_)
    if (!fin.count(d)) gone.push_back(d);
  for (const Digest& d : added)
    if (!fin.count(d)) gone.push_back(d);
  const uint64_t up2 = be.up_mask_.load(std::memory_order_acquire);
  for (const Digest& d : gone) {
    const int o = be.owner_of(d, up2);
    for (int r = 0; r < N; ++r) {
      if (r == o || !((up2 >> r) & 1)) continue;
      Req q;
      q.kind = ReqKind::Del;
      q.d = d;
      be.write_begin(d.lo);
      be.enqueue(r, std::move(q));
      ++dropped;
    }
  }
}

// ---- 13. the published state and the counters
void HbmBackend::HotRefresh::count() {
  be.hot_set_ = std::move(table.hot);
  be.hot_rank_ = std::move(table.rank);
  be.hot_weights_ = table.wts;
  be.hot_objects_.store(be.hot_set_.size(), std::memory_order_relaxed);
  uint64_t n_added = 0;
  for (const Digest& d : added) n_added += fin.count(d);
  be.hot_added_.fetch_add(n_added, std::memory_order_relaxed);
  be.hot_removed_.fetch_add(gone.size(), std::memory_order_relaxed);
  be.hot_deferred_.fetch_add(deferred.size(), std::memory_order_relaxed);
  be.hot_dropped_replicas_.fetch_add(dropped, std::memory_order_relaxed);
  be.hot_fill_bytes_.fetch_add(fill_bytes, std::memory_order_relaxed);
  be.hot_refreshes_.fetch_add(1, std::memory_order_relaxed);
  const uint64_t us = (uint64_t)((wall_s() - t_start) * 1e6);
  be.hot_refresh_us_.store(us, std::memory_order_relaxed);
  out.emplace_back("hot", be.hot_set_.size());
  out.emplace_back("added", n_added);
  out.emplace_back("removed", gone.size());
  out.emplace_back("deferred", deferred.size());
  out.emplace_back("replicas_dropped", dropped);
  out.emplace_back("fill_bytes", fill_bytes);
  out.emplace_back("spread_mask", be.spread_mask_.load());
  out.emplace_back("heal_mask", heal);
  out.emplace_back("failed_mask", bad);
  out.emplace_back("hot_share_ppm", (uint64_t)(plan.hot_share * 1e6));
  double pmax = 0, psum = 0;
  int pn = 0;
  for (int r = 0; r < N; ++r)
    if ((up >> r) & 1) {
      pmax = std::max(pmax, plan.planned[(size_t)r]);
      psum += plan.planned[(size_t)r];
      ++pn;
    }
  out.emplace_back("planned_max_over_mean_ppm",
                   psum > 0 ? (uint64_t)(pmax / (psum / pn) * 1e6) : 0);
  out.emplace_back("refresh_us", us);
}

}  // namespace shellac
