// HbmBackend's reactor-direct submission: the reactor is its own batcher for small GET
// batches — it writes the edge-server job, polls the job's host slot in its loop and answers
// the requests inline. Replaces the reference's blocking mc.get inside the reactor
// (src/python/shellac/server/Server.py:335) without blocking, and without a batcher-thread
// hop either way. HbmBackend::get() (backend_hbm.cc) decides which GETs come here.
#include "hbm_backend_impl.h"

namespace shellac {

void HbmBackend::direct_attach(Executor* ex) {
  if (!ex || direct_.empty() || tl_direct.be == this) return;
  std::lock_guard<std::mutex> lk(direct_mu_);
  for (auto& dc : direct_)
    if (!dc->ex && !dc->poisoned) {
      dc->ex = ex;
      tl_direct = DirectTls{this, dc.get()};
      return;
    }
  // more reactors than contexts: the rest use the batcher
}

void HbmBackend::direct_submit(Direct& dc, size_t k) {
  Dev& dv = *devs_[k];
  Direct::PerDev& pd = dc.dev[k];
  std::vector<Req>& P = pd.pending;
  int free_job = -1;
  for (int j = 0; j < kDirectJobs && free_job < 0; ++j)
    if (!pd.jobs[j].busy) free_job = j;
  // distinct digests (at most kServeKeys: a bigger batch is the batcher's); a linear scan,
  // no table: at most kServeKeys rows, and this thread must not allocate for it
  size_t rows = 0;
  Digest keys[HbmCache::kServeKeys];
  std::vector<uint32_t> urow(P.size());
  bool small = true;
  for (size_t i = 0; i < P.size() && small; ++i) {
    size_t u = 0;
    while (u < rows && !(keys[u].lo == P[i].d.lo && keys[u].hi == P[i].d.hi)) ++u;
    if (u == rows) {
      if (rows == (size_t)HbmCache::kServeKeys) {
        small = false;
        break;
      }
      keys[rows++] = P[i].d;
    }
    urow[i] = (uint32_t)u;
  }
  // both jobs busy with a small batch pending: it goes out when one finishes (a few us)
  if (small && free_job < 0) return;
  bool ok = small && dv.up() && dv.flush_pend.load(std::memory_order_acquire) == 0 &&
            dv.cache->serve_backlog() <
                (uint64_t)cfg_.direct_backlog * (uint64_t)dv.cache->serve_blocks();
  Direct::Job* jb = ok ? &pd.jobs[free_job] : nullptr;
  if (ok) {
    jb->arena = dv.pool->try_take((size_t)(pd.avg_row_bytes * 1.5 * (double)rows) + (64u << 10));
    ok = jb->arena != nullptr;
  }
  if (ok) {
    jb->tnow = now();
    std::copy(keys, keys + rows, jb->keys);
    ok = dv.cache->serve_get(jb->keys, (int64_t)rows, jb->arena->d, jb->arena->cap, jb->offs_d,
                             jb->tnow, jb->slot);
    if (!ok) jb->arena.reset();
  }
  if (!ok) {
    dv.direct_fallbacks.fetch_add(P.size(), std::memory_order_relaxed);
    enqueue_many((int)k, P);
    return;
  }
  jb->rows = rows;
  jb->urow.swap(urow);
  jb->reqs.swap(P);
  P.clear();
  jb->busy = true;
  jb->answered = false;
  jb->t0 = wall_s();
  dv.direct_jobs.fetch_add(1, std::memory_order_relaxed);
  dv.direct_reqs.fetch_add(jb->reqs.size(), std::memory_order_relaxed);
  dv.coalesced.fetch_add(jb->reqs.size() - rows, std::memory_order_relaxed);
}

void HbmBackend::direct_reap(Direct& dc, size_t k, int j) {
  Dev& dv = *devs_[k];
  Direct::PerDev& pd = dc.dev[k];
  Direct::Job& jb = pd.jobs[j];
  const uint64_t total = dv.cache->host_slot(jb.slot);
  if (total == HbmCache::kSlotPending) {
    const double el = wall_s() - jb.t0;
    // the server may have exited (idle / lifetime) just before taking the job
    if (el > 20e-6) dv.cache->serve_kick();
    if (!jb.answered && el * 1e3 > cfg_.batch_timeout_ms) {
      // stalled: answer misses now; the job (arena, slot) stays reserved until it ends
      dv.direct_timeouts.fetch_add(1, std::memory_order_relaxed);
      std::vector<Req> rs;
      rs.swap(jb.reqs);
      jb.answered = true;
      for (auto& r : rs)
        if (r.gcb) r.gcb(false, CacheValue{});
    }
    return;
  }
  dv.direct_ns.fetch_add((uint64_t)((wall_s() - jb.t0) * 1e9), std::memory_order_relaxed);
  std::vector<Req> rs;
  rs.swap(jb.reqs);
  std::shared_ptr<ArenaPool::Arena> arena = std::move(jb.arena);
  const bool answered = jb.answered;
  jb.busy = false;
  jb.answered = false;
  if (answered) return;
  if (total == HbmCache::kSlotFailed) {
    for (auto& r : rs) r.gcb(false, CacheValue{});
    return;
  }
  if (jb.rows) pd.avg_row_bytes = 0.9 * pd.avg_row_bytes + 0.1 * ((double)total / (double)jb.rows);
  if (total > arena->cap) {  // the records did not fit (none written): the batcher regathers
    dv.direct_overflows.fetch_add(1, std::memory_order_relaxed);
    enqueue_many((int)k, rs);
    return;
  }
  // answers first, callbacks after: a callback may issue GETs of its own (into pending)
  std::shared_ptr<const void> owner = arena;
  struct Ans {
    bool hit;
    CacheValue v;
  };
  std::vector<Ans> ans(rs.size());
  for (size_t i = 0; i < rs.size(); ++i) {
    const uint32_t u = jb.urow[i];
    const uint64_t o = jb.offs_h[u], sz = jb.offs_h[u + 1] - o;
    bool mismatch = false;
    ans[i].hit = read_hit(arena->h, o, sz, jb.keys[u], rs[i].key, jb.tnow, owner, &ans[i].v,
                          &mismatch);
    if (mismatch) dv.key_mismatch.fetch_add(1, std::memory_order_relaxed);
  }
  for (size_t i = 0; i < rs.size(); ++i) {
    Req& r = rs[i];
    if (r.ex == dc.ex) r.gcb(ans[i].hit, std::move(ans[i].v));
    else if (r.ex) {
      auto cb = std::move(r.gcb);
      r.ex->post([cb = std::move(cb), a = std::move(ans[i])]() mutable { cb(a.hit, std::move(a.v)); });
    } else {
      r.gcb(ans[i].hit, std::move(ans[i].v));
    }
  }
}

bool HbmBackend::direct_service() {
  Direct* dc = tl_direct.be == this ? tl_direct.ctx : nullptr;
  if (!dc) return false;
  bool busy = false;
  for (size_t k = 0; k < devs_.size(); ++k) {
    Direct::PerDev& pd = dc->dev[k];
    for (int j = 0; j < kDirectJobs; ++j)
      if (pd.jobs[j].busy) direct_reap(*dc, k, j);
    if (!pd.pending.empty()) direct_submit(*dc, k);
    for (int j = 0; j < kDirectJobs; ++j) busy |= pd.jobs[j].busy;
    busy |= !pd.pending.empty();
  }
  return busy;
}

void HbmBackend::direct_detach() {
  Direct* dc = tl_direct.be == this ? tl_direct.ctx : nullptr;
  if (!dc) return;
  for (size_t k = 0; k < devs_.size(); ++k) enqueue_many((int)k, dc->dev[k].pending);
  const double until = wall_s() + cfg_.batch_timeout_ms * 1e-3 + 1.0;
  for (;;) {
    bool busy = false;
    for (size_t k = 0; k < devs_.size(); ++k)
      for (int j = 0; j < kDirectJobs; ++j)
        if (dc->dev[k].jobs[j].busy) {
          direct_reap(*dc, k, j);
          busy |= dc->dev[k].jobs[j].busy;
        }
    if (!busy) break;
    if (wall_s() > until) {
      dc->poisoned = true;  // a job never finished: its arena / slot stay reserved
      break;
    }
    __builtin_ia32_pause();
  }
  tl_direct = DirectTls{};
  std::lock_guard<std::mutex> lk(direct_mu_);
  dc->ex = nullptr;
}

}  // namespace shellac
