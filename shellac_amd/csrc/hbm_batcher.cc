// HbmBackend::Dev: one GPU shard's batcher thread.
//
//   reactors ──get/set/del──▶ queue ──▶ batcher thread ──▶ HIP stream
//                                          │  flight k:   edge GET (keys + offsets in
//                                          │              mapped memory, values into a
//                                          │              pinned arena), SET store,
//                                          │              DELETE, touch, fill, purge, event
//                                          │  up to `depth` flights in flight
//                                          ◀─ reap in order: completion slot / event
//   reactors ◀──post_batch(callbacks)──────┘  hits = ByteRef slices of the arena
//
// A hit never touches a host copy: the GPU writes [ItemHeader | u16 klen | key | payload]
// into pinned memory, the batcher checks the key bytes and hands out a slice of the
// payload that keeps the arena alive until the last client write completes.
#include <pthread.h>

#include <algorithm>

#include "hbm_backend_impl.h"

namespace shellac {

bool HbmBackend::Dev::take_batch(std::vector<Req>* out, bool* do_flush, bool* rebuilding) {
  std::unique_lock<std::mutex> lk(mu);
  ctl_pending.store(false, std::memory_order_relaxed);
  if (q.empty() && !flush_req && !filt_want_rebuild) return false;
  const HbmBackendConfig& cfg = be->cfg_;
  if (cfg.batch_us > 0 && (int)q.size() < cfg.max_batch) {
    // optional linger: trade latency for bigger batches
    const auto deadline = std::chrono::steady_clock::now() + std::chrono::microseconds(cfg.batch_us);
    while (!stop && (int)q.size() < cfg.max_batch &&
           cv.wait_until(lk, deadline) != std::cv_status::timeout) {
    }
  }
  if (filt_want_rebuild) {
    // SETs queued from here on add to filt_next; the ones already queued are in this
    // batch and committed before finish_filter_rebuild() exports the shard's keys
    filt_next = std::make_shared<PresenceFilter>(filt_bits);
    filt_want_rebuild = false;
    *rebuilding = true;
  }
  // (seen as a second origin fetch in test_proxy_reactor_direct_gets when a reactor's GET
  // reached the queue before the batcher took the SET it must stay behind)
  const size_t take = plan_take(q, cfg.max_batch, take_scratch);
  if (take == q.size()) {
    out->swap(q);
  } else {
    out->assign(std::make_move_iterator(q.begin()), std::make_move_iterator(q.begin() + take));
    q.erase(q.begin(), q.begin() + take);
  }
  qn.store(q.size(), std::memory_order_release);
  *do_flush = flush_req;
  flush_req = false;
  return true;
}

// The queued requests become the next flight (or are failed: the shard is out of service);
// a flush or a presence-filter rebuild asked for rides along. False: nothing was queued.
bool HbmBackend::Dev::launch_queued(std::vector<Req>& batch) {
  const HbmBackendConfig& cfg = be->cfg_;
  bool do_flush = false, rebuilding = false;
  batch.clear();
  if (!take_batch(&batch, &do_flush, &rebuilding)) return false;
  if (!up() || failed) {
    fail_requests(batch, true);
    if (do_flush) flush_done();
  } else if (batch.empty()) {
    try {
      // finished before anything else may read the shard: edge-server GETs are not
      // ordered after the stream
      if (do_flush) {
        cache->flush(stream);
        HB_OK(hipStreamSynchronize(stream));
      }
    } catch (const std::exception& e) {
      std::fprintf(stderr, "[shellac hbm] gpu %d flush failed: %s\n", device, e.what());
    }
    if (do_flush) flush_done();
  } else {
    Flight& f = *flights[(head + inflight) % flights.size()];
    f.reqs.swap(batch);
    try {
      if (do_flush) cache->flush(stream);
      f.flush = do_flush;
      launch(f);
      track_writes(f, +1);
      ++inflight;
    } catch (const std::exception& e) {
      std::fprintf(stderr, "[shellac hbm] gpu %d launch failed: %s\n", device, e.what());
      fail_requests(f.reqs, true);
      if (do_flush) flush_done();
      f.flush = false;
      f.reqs.clear();
      f.active = false;
      eject("launch error");
    }
  }
  if (rebuilding) {
    try {
      finish_filter_rebuild();  // export_keys runs after the batch on the stream
    } catch (const std::exception& e) {
      std::fprintf(stderr, "[shellac hbm] presence filter rebuild failed: %s\n", e.what());
      std::lock_guard<std::mutex> lk(mu);
      filt_next.reset();
    }
  } else if (cfg.presence_filter && filt->adds() >= filt_rebuild_at) {
    std::lock_guard<std::mutex> lk(mu);
    filt_want_rebuild = true;
    ctl_pending.store(true, std::memory_order_release);
  }
  return true;
}

void HbmBackend::Dev::loop() {
  const HbmBackendConfig& cfg = be->cfg_;
  (void)hipSetDevice(device);
  const std::string nm = "shellac-hbm" + std::to_string(device);
  pthread_setname_np(pthread_self(), nm.c_str());
  if (!cfg.batcher_cpus.empty()) {  // a core of its own: it spins on the queue and the GPU
    cpu_set_t set;
    CPU_ZERO(&set);
    CPU_SET(cfg.batcher_cpus[(size_t)index % cfg.batcher_cpus.size()], &set);
    (void)pthread_setaffinity_np(pthread_self(), sizeof set, &set);
  }
  std::vector<Req> batch;
  for (;;) {
    bool worked = false;
    // 1. reap the oldest flight (in launch order) once its completion signal fired
    if (inflight) {
      Flight& f = *flights[head];
      bool freed = false;
      try {
        freed = try_reap(f, false);
      } catch (const std::exception& e) {
        std::fprintf(stderr, "[shellac hbm] gpu %d batch failed: %s\n", device, e.what());
        fail_flight(f);
        eject("batch error");
        freed = true;
      }
      if (!freed && f.active && (wall_s() - f.t0) * 1e3 > cfg.batch_timeout_ms) {
        std::fprintf(stderr, "[shellac hbm] gpu %d batch stalled for %d ms\n", device,
                     cfg.batch_timeout_ms);
        fail_flight(f);  // answered as misses; the flight stays busy until the GPU finishes
        eject("stall");
      }
      if (freed) {
        track_writes(f, -1);
        head = (head + 1) % flights.size();
        --inflight;
        worked = true;
      }
    }
    // 2. launch the queued requests as a new flight
    if (inflight < flights.size() &&
        (qn.load(std::memory_order_acquire) || ctl_pending.load(std::memory_order_acquire)))
      worked |= launch_queued(batch);
    if (worked) continue;
    if (inflight) {  // waiting on the GPU: poll (the edge GET signals through host memory)
      if (up()) __builtin_ia32_pause();
      else std::this_thread::sleep_for(std::chrono::microseconds(200));  // ejected, draining
      continue;
    }
    // 3. idle
    if (!up()) maybe_restore();
    if (cfg.spin_us > 0 && qn.load(std::memory_order_acquire) == 0) {
      // poll for up to spin_us before blocking: under steady traffic the next request
      // usually arrives within that window, and catching it saves a futex wake-up
      spinning.store(true, std::memory_order_release);
      const auto until = std::chrono::steady_clock::now() + std::chrono::microseconds(cfg.spin_us);
      while (qn.load(std::memory_order_acquire) == 0 && std::chrono::steady_clock::now() < until)
        __builtin_ia32_pause();
      spinning.store(false, std::memory_order_release);
    }
    std::unique_lock<std::mutex> lk(mu);
    if (stop && q.empty()) return;
    if (!q.empty() || flush_req || filt_want_rebuild || kick) {
      kick = false;
      continue;
    }
    const auto wake = [&] { return stop || !q.empty() || flush_req || filt_want_rebuild || kick; };
    const int wait_s = !up() ? 1 : cfg.sweep_interval_s;
    if (wait_s > 0) {
      if (!cv.wait_for(lk, std::chrono::seconds(wait_s), wake) && up() && cfg.sweep_interval_s > 0) {
        // idle: expire TTL'd objects out of the index now and then
        lk.unlock();
        try {
          sweep();
        } catch (const std::exception& e) {
          std::fprintf(stderr, "[shellac hbm] sweep failed: %s\n", e.what());
        }
      }
    } else {
      cv.wait(lk, wake);
    }
  }
}

// ---------------------------------------------------------------------------------
// a flight's launch: its requests sorted by kind, then one stage per kind in stream order
// ---------------------------------------------------------------------------------
void HbmBackend::Dev::launch(Flight& f) {
  TraceRange tr("hbm_backend.launch");
  for (auto* v : {&f.gets, &f.sets, &f.dels, &f.touches, &f.slices, &f.ctls}) v->clear();
  for (uint32_t i = 0; i < f.reqs.size(); ++i) {
    switch (f.reqs[i].kind) {
      case ReqKind::Get: f.gets.push_back(i); break;
      case ReqKind::Set: f.sets.push_back(i); break;
      case ReqKind::Del: f.dels.push_back(i); break;
      case ReqKind::Touch: f.touches.push_back(i); break;
      case ReqKind::Slice: f.slices.push_back(i); break;
      case ReqKind::Barrier:
      case ReqKind::Fill:
      case ReqKind::Purge:
      case ReqKind::List: f.ctls.push_back(i); break;
    }
  }
  f.tnow = be->now();
  f.t0 = wall_s();
  f.got = f.gets.empty();
  f.active = true;
  f.served = false;
  launch_gets(f);
  launch_slices(f);
  launch_sets(f);
  launch_dels(f);
  launch_touches(f);
  launch_fills(f);
  launch_purges(f);
  launch_lists(f);
  HB_OK(hipEventRecord(f.ev, stream));
  batches++;
  batched_reqs += f.reqs.size();
  uint64_t prev = max_batch.load();
  while (f.reqs.size() > prev && !max_batch.compare_exchange_weak(prev, f.reqs.size())) {
  }
}

// GET: equal digests coalesced on the host (coalesce_gets), then one edge-GET launch: keys
// and offsets in mapped memory, records straight into a pinned arena
void HbmBackend::Dev::launch_gets(Flight& f) {
  const size_t n0 = f.gets.size();
  f.rows = 0;
  if (!n0) return;
  f.urow.resize(n0);
  f.keys.ensure(n0 * sizeof(Digest));
  Digest* hk = f.keys.host<Digest>();
  f.rows = coalesce_gets(f.reqs, f.gets, co_tab, hk, f.urow.data());
  coalesced += n0 - f.rows;
  f.offs.ensure((f.rows + 1) * 8);
  // arena sized from the running average record size (regathered if it falls short)
  const size_t want = (size_t)(avg_row_bytes * 1.5 * (double)f.rows) + (64u << 10);
  f.arena = pool->take(want);
  // small batches go to the resident edge server unless they must stay ordered after a
  // SET / DELETE / flush still in flight (read-your-writes for memcached clients)
  bool ordered = pend_flush > 0 || f.flush;
  for (size_t u = 0; !ordered && !pend_w.empty() && u < f.rows; ++u)
    ordered = pend_w.count(hk[u].lo) != 0;
  if (ordered) ordered_gets++;
  // ... and only while fewer than serve_backlog jobs are ahead of it: the server takes
  // one job at a time, so under load (several batches in flight) the launched path's
  // many workgroups win (profiles/archive/r3_http: c=1000 with every small batch served 0.95M
  // RPS, launched only 1.13M)
  f.served = be->cfg_.edge_server && !ordered && f.rows <= (size_t)HbmCache::kServeKeys &&
             cache->serve_backlog() <
                 (uint64_t)be->cfg_.serve_backlog * (uint64_t)cache->serve_blocks() &&
             cache->serve_get(hk, (int64_t)f.rows, f.arena->d, f.arena->cap,
                              f.offs.dev<uint64_t>(), f.tnow, f.slot);
  if (f.served) served_batches++;
  else
    cache->small_get(f.keys.dev<Digest>(), (int64_t)f.rows, f.arena->d, f.arena->cap,
                     f.offs.dev<uint64_t>(), f.tnow, stream, f.slot);
}

// Slices (get_part): reads, on the stream right after the flight's GETs and before its writes.
// One row per request, everything in mapped memory; the rows' bytes land in an arena of their
// own, sized from the running average (asked again if it falls short, deliver_slices).
// They are answered when the flight's event has completed, that is behind the flight's SETs,
// DELETEs, touches and any purge or list scan that shares the flight, whereas a GET is
// answered as soon as its completion slot fires: a part batched with a scan waits for it.
void HbmBackend::Dev::launch_slices(Flight& f) {
  const size_t n = f.slices.size();
  if (!n) return;
  const SlicePlan p = plan_slice_rows(f.reqs, f.slices);
  f.slice_offs_off = align_up(n * sizeof(Digest), 16);
  f.slice_spec_off = f.slice_offs_off + align_up((n + 1) * 8, 16);
  f.slice_rows_off = f.slice_spec_off + align_up(n * sizeof(SliceSpec), 16);
  f.slice_res_off = f.slice_rows_off + n * sizeof(SliceRow);
  f.slice_kb_off = f.slice_res_off + 16;
  // conditions travel only where some row has one; the launch is the plain one otherwise
  size_t cond_bytes = 0;
  f.slice_conds = false;
  for (uint32_t i : f.slices)
    if (f.reqs[i].cond) {
      f.slice_conds = true;
      cond_bytes += f.reqs[i].cond->records.size();
    }
  f.slice_cond_off = align_up(f.slice_kb_off + p.kbytes.size(), 16);
  f.slice_cb_off = f.slice_cond_off + (f.slice_conds ? n * sizeof(SliceCond) : 0);
  f.slice_buf.ensure(f.slice_cb_off + cond_bytes + 16);
  uint8_t* const hb = f.slice_buf.host<uint8_t>();
  size_t cb_at = 0;
  for (size_t j = 0; j < n; ++j) {
    const Req& r = f.reqs[f.slices[j]];
    reinterpret_cast<Digest*>(hb)[j] = r.d;
    reinterpret_cast<SliceSpec*>(hb + f.slice_spec_off)[j] = r.spec;
    if (!f.slice_conds) continue;
    SliceCond c{};
    if (r.cond) {
      c = SliceCond{r.cond->kind, r.cond->ncand, (uint32_t)cb_at, (uint32_t)r.cond->records.size()};
      std::memcpy(hb + f.slice_cb_off + cb_at, r.cond->records.data(), r.cond->records.size());
      cb_at += r.cond->records.size();
    }
    reinterpret_cast<SliceCond*>(hb + f.slice_cond_off)[j] = c;
  }
  std::memcpy(hb + f.slice_offs_off, p.offs.data(), (n + 1) * 8);
  std::memcpy(hb + f.slice_kb_off, p.kbytes.data(), p.kbytes.size());
  f.slice_arena = pool->take((size_t)(avg_slice_bytes * 1.5 * (double)n) + (64u << 10));
  run_slices(f);
  slice_reqs += n;
}

void HbmBackend::Dev::run_slices(Flight& f) {
  uint8_t* const db = f.slice_buf.dev<uint8_t>();
  std::memset(f.slice_buf.host<uint8_t>() + f.slice_res_off, 0, 16);
  cache->get_keyed_slices(reinterpret_cast<const Digest*>(db), db + f.slice_kb_off,
                          reinterpret_cast<const int64_t*>(db + f.slice_offs_off),
                          reinterpret_cast<const SliceSpec*>(db + f.slice_spec_off),
                          (int64_t)f.slices.size(),
                          reinterpret_cast<SliceRow*>(db + f.slice_rows_off), f.slice_arena->d,
                          f.slice_arena->cap, reinterpret_cast<uint64_t*>(db + f.slice_res_off),
                          f.tnow, stream, 0,
                          f.slice_conds ? reinterpret_cast<const SliceCond*>(db + f.slice_cond_off)
                                        : nullptr,
                          f.slice_conds ? db + f.slice_cb_off : nullptr);
}

// SET: [klen | key | payload] values packed into mapped staging the SET kernels read
// directly (no copies), exact log-bytes bound
void HbmBackend::Dev::launch_sets(Flight& f) {
  const size_t ns = f.sets.size();
  if (!ns) return;
  f.set_keys.ensure(ns * sizeof(Digest));
  f.set_voff.ensure(ns * 8);
  f.set_meta.ensure(ns * 12);
  size_t bytes = 16;
  for (uint32_t i : f.sets)
    bytes += align_up(keyed_size(f.reqs[i].key.size(), f.reqs[i].value->size()), 16);
  f.set_vals.ensure(bytes);
  Digest* kk = f.set_keys.host<Digest>();
  uint64_t* vo = f.set_voff.host<uint64_t>();
  uint32_t* vl = f.set_meta.host<uint32_t>();
  uint32_t* fl = vl + ns;
  uint32_t* ex = vl + 2 * ns;
  uint64_t off = 0, bound = 0;
  for (size_t j = 0; j < ns; ++j) {
    const Req& r = f.reqs[f.sets[j]];
    const size_t sz = keyed_size(r.key.size(), r.value->size());
    write_keyed(f.set_vals.host<uint8_t>() + off, r.key, r.value->data(), r.value->size());
    kk[j] = r.d;
    vo[j] = off;
    vl[j] = (uint32_t)sz;
    fl[j] = r.flags;
    ex[j] = r.ttl ? f.tnow + r.ttl : 0;
    off += align_up(sz, 16);
    bound += item_bytes((uint32_t)sz);
  }
  cache->store(f.set_keys.dev<Digest>(), f.set_vals.dev<uint8_t>(),
               f.set_voff.dev<uint64_t>(), f.set_meta.dev<uint32_t>(),
               f.set_meta.dev<uint32_t>() + ns, f.set_meta.dev<uint32_t>() + 2 * ns,
               (int64_t)ns, bound, f.tnow, stream);
  for (uint32_t i : f.sets) f.reqs[i].value = Bytes();  // staged: drop the reference
}

// DELETE: keys and found flags in mapped memory
void HbmBackend::Dev::launch_dels(Flight& f) {
  const size_t nd = f.dels.size();
  if (!nd) return;
  f.del_keys.ensure(nd * sizeof(Digest));
  f.del_found.ensure(nd);
  for (size_t j = 0; j < nd; ++j) f.del_keys.host<Digest>()[j] = f.reqs[f.dels[j]].d;
  cache->remove(f.del_keys.dev<Digest>(), (int64_t)nd, f.del_found.dev<uint8_t>(), f.tnow,
                stream);
}

// TOUCH: after the flight's SETs and DELETEs (plan_take keeps a write queued behind a touch
// of its key out of the flight). The rows of plan_touch_rows, everything in mapped memory:
// one key-exact launch for the rows that keep their flags, one for those that replace them.
void HbmBackend::Dev::launch_touches(Flight& f) {
  const size_t nt = f.touches.size();
  if (!nt) return;
  TouchPlan p = plan_touch_rows(f.reqs, f.touches);
  const size_t n = p.rows(), nkeep = p.nkeep;
  f.trow.swap(p.trow);
  // {digests | offsets (one array per launch, n + 2 words in all) | expiries | flags | hit}
  const size_t o_offs = align_up(n * sizeof(Digest), 16), o_exp = o_offs + align_up((n + 2) * 8, 16),
               o_fl = o_exp + align_up(n * 4, 16), o_hit = o_fl + align_up(n * 4, 16);
  f.touch_rows.ensure(o_hit + n);
  f.touch_kbytes.ensure(16 + p.kbytes.size());
  uint8_t* const hb = f.touch_rows.host<uint8_t>();
  uint8_t* const db = f.touch_rows.dev<uint8_t>();
  Digest* kk = reinterpret_cast<Digest*>(hb);
  uint32_t* ex = reinterpret_cast<uint32_t*>(hb + o_exp);
  uint32_t* fl = reinterpret_cast<uint32_t*>(hb + o_fl);
  for (size_t row = 0; row < n; ++row) {
    const Req& r = f.reqs[f.touches[p.src[row]]];
    kk[row] = r.d;
    ex[row] = r.ttl ? f.tnow + r.ttl : 0;
    fl[row] = r.flags;
  }
  std::memcpy(hb + o_offs, p.offs.data(), (n + 2) * 8);
  std::memset(hb + o_hit, 0, n);
  f.touch_hit = hb + o_hit;
  std::memcpy(f.touch_kbytes.host<uint8_t>(), p.kbytes.data(), p.kbytes.size());
  const uint8_t* const dkb = f.touch_kbytes.dev<uint8_t>();
  if (nkeep)
    cache->touch(reinterpret_cast<const Digest*>(db), reinterpret_cast<const uint32_t*>(db + o_exp),
                 nullptr, dkb, reinterpret_cast<const int64_t*>(db + o_offs), (int64_t)nkeep,
                 db + o_hit, f.tnow, stream);
  if (n > nkeep)
    cache->touch(reinterpret_cast<const Digest*>(db) + nkeep,
                 reinterpret_cast<const uint32_t*>(db + o_exp) + nkeep,
                 reinterpret_cast<const uint32_t*>(db + o_fl) + nkeep, dkb,
                 reinterpret_cast<const int64_t*>(db + o_offs) + nkeep + 1,
                 (int64_t)(n - nkeep), db + o_hit + nkeep, f.tnow, stream);
  touch_reqs += nt;
}

// Hot-replica fills (after the flight's writes: every write queued before them ran first);
// their staging is the refresh's (FillStaging)
void HbmBackend::Dev::launch_fills(Flight& f) {
  for (uint32_t i : f.ctls) {
    if (f.reqs[i].kind != ReqKind::Fill) continue;
    HotFill& h = *f.reqs[i].fill;
    {
      std::lock_guard<std::mutex> lk(mu);
      if (h.cancelled) continue;  // the refresh gave up on this shard
      h.launched = true;
      for (int64_t j = 0; j < h.m; ++j)
        if (h.hsize[j] && touched.count(h.lo[(size_t)j])) {
          h.hsize[j] = 0;  // a newer write-through copy is (or will be) here
          ++h.skipped;
        } else if (h.hsize[j]) {
          ++h.rows;
        }
    }
    records_to_set(h.krec, h.koff, h.dsize, nullptr, h.m, h.okeys, h.ovoff, h.ometa,
                   h.ometa + h.m, h.ometa + 2 * h.m, stream);
    cache->store(h.okeys, h.krec, h.ovoff, h.ometa, h.ometa + h.m, h.ometa + 2 * h.m, h.m,
                 h.bound, f.tnow, stream);
  }
}

// A selector's device image (selector.h) staged at byte `off` of the mapped buffer `m`; the
// device address of what was written.
static const uint8_t* stage_image(const KeyedSelector& what, Mapped& m, size_t off) {
  what.write_image(m.host<uint8_t>() + off);
  return m.dev<uint8_t>() + off;
}

// Purges: after the SETs and DELETEs queued before them (a purge is its flight's last
// request); selector images and result words in mapped memory
void HbmBackend::Dev::launch_purges(Flight& f) {
  using Kind = KeyedSelector::Kind;
  size_t np = 0, img_bytes = 0;
  for (uint32_t i : f.ctls)
    if (f.reqs[i].kind == ReqKind::Purge) {
      ++np;
      img_bytes += f.reqs[i].what->image_bytes();
    }
  if (!np) return;
  f.purge_img.ensure(img_bytes);
  f.purge_out.ensure(np * 16);
  size_t off = 0, j = 0;
  for (uint32_t i : f.ctls) {
    const Req& r = f.reqs[i];
    if (r.kind != ReqKind::Purge) continue;
    const KeyedSelector& w = *r.what;
    const PurgeAction& a = r.how;
    uint64_t* const res = f.purge_out.host<uint64_t>() + 2 * j;
    res[0] = res[1] = 0;
    uint64_t* const out = f.purge_out.dev<uint64_t>() + 2 * j;
    const uint32_t cap = a.keep_s ? f.tnow + a.keep_s : 0;
    const uint8_t* const img = stage_image(w, f.purge_img, off);
    const uint32_t nb = (uint32_t)w.image_bytes(), plen = (uint32_t)w.pattern.size();
    switch (w.kind) {
      case Kind::Glob:
        if (a.soft) cache->soften_keyed_glob(img, nb, a.stale_at, cap, f.tnow, out, stream);
        else cache->remove_keyed_glob(img, nb, f.tnow, out, stream);
        break;
      case Kind::Tags: {
        const uint64_t* const list = reinterpret_cast<const uint64_t*>(img);
        const uint32_t nt = (uint32_t)w.hashes.size();
        if (a.soft) cache->soften_keyed_tags(list, nt, a.stale_at, cap, f.tnow, out, stream);
        else cache->remove_keyed_tags(list, nt, f.tnow, out, stream);
        break;
      }
      default:  // Prefix, and a soft Exact (purge_refused: no other kind gets here)
        if (a.soft)  // (the flight's SET chains are whole ones)
          cache->soften_keyed_prefix(img, plen, w.kind == Kind::Exact, a.stale_at, cap, f.tnow,
                                     out, stream);
        else cache->remove_keyed_prefix(img, plen, f.tnow, out, stream);
    }
    off += nb;
    ++j;
  }
}

// A list (HbmBackend::list_step): after the flight's writes, as a purge; the selector's image,
// the result words, the rows and the key areas in one mapped buffer. It writes
// nothing in the cache, so neither the filter nor `touched` nor purge_dirty hears of it.
constexpr uint32_t kListBackendKeyCap = 256;  // keys up to 254 bytes come back whole

void HbmBackend::Dev::launch_lists(Flight& f) {
  using Kind = KeyedSelector::Kind;
  for (uint32_t i : f.ctls) {
    const Req& r = f.reqs[i];
    if (r.kind != ReqKind::List) continue;
    const KeyedSelector& w = r.list->q.what;
    const uint32_t limit = r.flags;
    const size_t img = w.image_bytes();
    f.list_out_off = img;
    f.list_rows_off = img + 32;
    f.list_keys_off = f.list_rows_off + (size_t)limit * sizeof(ListRow);
    f.list_buf.ensure(f.list_keys_off + (size_t)limit * kListBackendKeyCap + 16);
    uint8_t* const h = f.list_buf.host<uint8_t>();
    uint8_t* const d = f.list_buf.dev<uint8_t>();
    stage_image(w, f.list_buf, 0);
    std::memset(h + f.list_out_off, 0, 32);
    uint32_t plen = 0;  // the engine's `plen`: the pattern's bytes, or the glob image's in use
    switch (w.kind) {
      case Kind::Glob: plen = (uint32_t)img; break;
      case Kind::Prefix: case Kind::Exact: plen = (uint32_t)w.pattern.size(); break;
      default: break;
    }
    cache->list_keyed(w.list_mode(), d, plen, w.kind == Kind::Exact,
                      reinterpret_cast<const uint64_t*>(d), (uint32_t)w.hashes.size(),
                      r.list_start, limit, kListBackendKeyCap, f.tnow,
                      reinterpret_cast<ListRow*>(d + f.list_rows_off), d + f.list_keys_off,
                      reinterpret_cast<uint64_t*>(d + f.list_out_off), stream);
    return;
  }
}

// The flight has finished: this shard's part of the walk. Rows flagged as changed and hot
// replicas (the digest's owner is another shard) are left out; the counts are per stored copy.
void HbmBackend::Dev::deliver_list(Flight& f, Req& r) {
  ListWalk& w = *r.list;
  const uint8_t* const h = f.list_buf.host<uint8_t>();
  const uint64_t* const out = reinterpret_cast<const uint64_t*>(h + f.list_out_off);
  const ListRow* const rows = reinterpret_cast<const ListRow*>(h + f.list_rows_off);
  w.res.matched += out[kListMatched];
  w.res.bytes += out[kListBytes];
  const uint64_t up = be->up_mask_.load(std::memory_order_acquire);
  for (uint64_t j = 0; j < out[kListListed]; ++j) {
    const ListRow& row = rows[j];
    if (row.bits & kListChanged) continue;
    if (list_row_is_replica(be->owner_of(Digest{row.d0, row.d1}, up), index)) continue;
    const uint8_t* const area = h + f.list_keys_off + j * kListBackendKeyCap;
    ListedObject o;
    const uint32_t have = std::min(row.klen, kListBackendKeyCap - (uint32_t)kKeyedPrefix);
    o.key.assign(reinterpret_cast<const char*>(area) + kKeyedPrefix, have);
    o.key_truncated = row.klen > have;
    o.size = row.vlen;
    o.ttl = row.expire ? (int64_t)row.expire - (int64_t)f.tnow : -1;
    o.flags = row.flags;
    o.ntags = row.ntags == kTagOverflow ? -1 : (int)row.ntags;
    o.referenced = (row.bits & kListRefBit) != 0;
    o.shard = index;
    w.res.objects.push_back(std::move(o));
  }
  const uint64_t nslots = cache->config().nbuckets * kEntriesPerBucket;
  if (!w.have_next) {
    const uint32_t got = (uint32_t)w.res.objects.size();
    const uint32_t still = w.q.limit > got ? w.q.limit - got : 0;
    w.res.next = list_cursor_after(index, w.asked, still, out[kListNext], nslots,
                                   (int)be->devs_.size());
    w.have_next = !w.res.next.empty();
  }
}

// ---------------------------------------------------------------------------------
// reaping
// ---------------------------------------------------------------------------------
// Completion of flight f (non-blocking unless `block`): GET results as soon as the edge
// GET's slot fires, DELETE results and the flight's buffers once its event completes.
bool HbmBackend::Dev::try_reap(Flight& f, bool block) {
  if (!f.got && f.active) {
    const uint64_t total = block ? cache->wait_host_slot(f.slot, be->cfg_.batch_timeout_ms)
                                 : cache->host_slot(f.slot);
    if (total == HbmCache::kSlotPending) {
      if (f.served) cache->serve_kick();  // relaunch the server if it exited meanwhile
      return false;
    }
    if (total == HbmCache::kSlotFailed) throw Error("edge GET reported a failed look-back");
    if (f.rows) avg_row_bytes = 0.9 * avg_row_bytes + 0.1 * ((double)total / (double)f.rows);
    if (total > f.arena->cap) regather(f, total);
    else deliver_gets(f);
    f.got = true;
  }
  if (block) {
    HB_OK(hipEventSynchronize(f.ev));
  } else {
    const hipError_t e = hipEventQuery(f.ev);
    if (e == hipErrorNotReady) return false;
    HB_OK(e);
  }
  if (f.active) {
    deliver_slices(f);
    deliver_dels(f);
    deliver_touches(f);
    finish_ctls(f);
    batch_ns += (uint64_t)((wall_s() - f.t0) * 1e9);
  }
  f.active = false;
  f.reqs.clear();
  f.arena.reset();  // hits hold their own references
  f.slice_arena.reset();
  return true;
}

// Rare: the records (`total` bytes) outgrew the arena (the kernel wrote none of them). A
// second lookup sees exactly the first one's state only when nothing has run since: no
// SET/DELETE in this flight and no later flight queued on the stream. Otherwise the GETs
// answer "miss" (always a valid cache answer: the proxy goes to the origin); reading a newer
// state would reorder them after later SETs.
void HbmBackend::Dev::regather(Flight& f, uint64_t total) {
  if (!(f.sets.empty() && f.dels.empty() && f.touches.empty() && inflight == 1)) {
    overflow_misses(f);
    return;
  }
  regathers++;
  HB_OK(hipEventSynchronize(f.ev));
  f.arena = pool->take(total + (64u << 10));
  cache->small_get(f.keys.dev<Digest>(), (int64_t)f.rows, f.arena->d, f.arena->cap,
                   f.offs.dev<uint64_t>(), f.tnow, stream, f.slot);
  HB_OK(hipEventRecord(f.ev, stream));
  const uint64_t t2 = cache->wait_host_slot(f.slot, be->cfg_.batch_timeout_ms);
  if (t2 == HbmCache::kSlotPending || t2 == HbmCache::kSlotFailed)
    throw Error("edge GET regather failed");
  if (t2 > f.arena->cap) overflow_misses(f);  // cannot happen: state unchanged
  else deliver_gets(f);
}

// The flight's control requests once its event has completed: what a purge's scan removed on
// this shard, and every one's completion callback.
void HbmBackend::Dev::finish_ctls(Flight& f) {
  size_t pj = 0;
  for (uint32_t i : f.ctls) {
    Req& r = f.reqs[i];
    if (r.kind == ReqKind::Purge) {
      const uint64_t* const res = f.purge_out.host<uint64_t>() + 2 * pj++;
      const bool soft = r.how.soft;
      switch (r.what->kind) {
        case KeyedSelector::Kind::Glob:
          (soft ? glob_softened_objects : glob_purged_objects) += res[0];
          break;
        case KeyedSelector::Kind::Tags:
          (soft ? tag_softened_objects : tag_purged_objects) += res[0];
          break;
        default:
          if (soft) {
            softened_objects += res[0];
          } else {
            purged_objects += res[0];
            purged_bytes += res[1];
          }
      }
      if (r.purge) r.purge->removed.fetch_add((int64_t)res[0], std::memory_order_relaxed);
    }
    if (r.kind == ReqKind::List) deliver_list(f, r);
    if (r.ccb) r.ccb(true);
  }
}

// dir = +1 when flight f launches, -1 when it is freed: its SET / DELETE / touch digests and
// its flush count as in flight until then.
void HbmBackend::Dev::track_writes(Flight& f, int dir) {
  if (dir > 0) {
    f.wkeys.clear();
    for (const auto* v : {&f.sets, &f.dels, &f.touches})
      for (uint32_t i : *v) f.wkeys.push_back(f.reqs[i].d.lo);
    for (uint64_t k : f.wkeys) ++pend_w[k];
    if (f.flush) ++pend_flush;
    return;
  }
  for (uint64_t k : f.wkeys) {
    auto it = pend_w.find(k);
    if (it != pend_w.end() && --it->second == 0) pend_w.erase(it);
    be->write_end(k);
  }
  f.wkeys.clear();
  if (f.flush) {
    if (pend_flush) --pend_flush;
    flush_done();
  }
  f.flush = false;
}

void HbmBackend::Dev::deliver_gets(Flight& f) {
  if (f.gets.empty()) return;
  const uint64_t* off = f.offs.host<uint64_t>();
  const Digest* hk = f.keys.host<Digest>();
  const uint8_t* base = f.arena->h;
  // the arena stays alive while any response built from it does
  std::shared_ptr<const void> owner = f.arena;
  PostGroups pg;
  for (size_t j = 0; j < f.gets.size(); ++j) {
    Req& r = f.reqs[f.gets[j]];
    const uint32_t u = f.urow[j];
    const uint64_t o = off[u], sz = off[u + 1] - o;
    CacheValue v;
    bool mismatch = false;
    const bool hit = read_hit(base, o, sz, hk[u], r.key, f.tnow, owner, &v, &mismatch);
    if (mismatch) key_mismatch.fetch_add(1, std::memory_order_relaxed);
    pg.answer(r.ex, [cb = std::move(r.gcb), hit, v = std::move(v)]() mutable {
      cb(hit, std::move(v));
    });
  }
  pg.flush();
}

// The flight's event has completed: its slices' rows and bytes are in host memory. Bytes that
// outgrew the arena (none were written) are asked for again into a bigger one under regather's
// condition (nothing has run since that could have changed what the rows saw), else the
// slices answer "miss". Asking again runs k_slice_plan again, so those rows count twice in
// get_ops / get_hits / get_bytes, as a regathered GET batch's do. A hit's head and window are
// slices of the arena, which stays alive while any response built from it does; the GPU
// matched the key, and the host checks it again against the bytes that arrived.
void HbmBackend::Dev::deliver_slices(Flight& f) {
  const size_t n = f.slices.size();
  if (!n) return;
  const uint8_t* const hb = f.slice_buf.host<uint8_t>();
  const uint64_t* const res = reinterpret_cast<const uint64_t*>(hb + f.slice_res_off);
  avg_slice_bytes = 0.9 * avg_slice_bytes + 0.1 * ((double)res[kSliceBytes] / (double)n);
  bool have = res[kSliceBytes] <= f.slice_arena->cap;
  if (!have && f.sets.empty() && f.dels.empty() && f.touches.empty() && inflight == 1) {
    regathers++;
    f.slice_arena = pool->take(res[kSliceBytes] + (64u << 10));
    run_slices(f);
    HB_OK(hipStreamSynchronize(stream));
    have = res[kSliceBytes] <= f.slice_arena->cap;
  }
  if (!have) arena_misses += n;
  const SliceRow* const rows = reinterpret_cast<const SliceRow*>(hb + f.slice_rows_off);
  const uint8_t* const base = f.slice_arena->h;
  std::shared_ptr<const void> owner = f.slice_arena;
  PostGroups pg;
  for (size_t j = 0; j < n; ++j) {
    Req& r = f.reqs[f.slices[j]];
    const SliceRow& row = rows[j];
    PartValue p;
    if (have && row.status != kSliceMiss) {
      const char* const v = reinterpret_cast<const char*>(base + row.out_off);
      size_t po = 0;
      if (!keyed_match(v, row.vlen, r.key, &po)) {
        key_mismatch.fetch_add(1, std::memory_order_relaxed);
      } else {
        p.status = row.status;
        p.flags = row.flags;
        p.ttl_left = row.expire ? (int64_t)row.expire - (int64_t)f.tnow : 0;
        if (row.status == kSliceWholeObj) {
          p.window = ByteRef(owner, v + po, row.vlen - po);
        } else {
          p.body_len = row.body_len;
          p.first = row.win_first;
          p.head = ByteRef(owner, v + row.head_off, row.body_off - row.head_off);
          p.window = ByteRef(owner, v + row.head_bytes + row.skew, row.win_len);
        }
      }
    }
    if (r.pcb)
      pg.answer(r.ex, [cb = std::move(r.pcb), p = std::move(p)]() mutable { cb(std::move(p)); });
  }
  pg.flush();
}

// Every GET of flight f answers "miss" (its records did not fit the arena).
void HbmBackend::Dev::overflow_misses(Flight& f) {
  arena_misses += f.gets.size();
  std::vector<Req> gets;
  for (uint32_t i : f.gets) gets.push_back(std::move(f.reqs[i]));
  fail_requests(gets, false);
}

void HbmBackend::Dev::deliver_dels(Flight& f) {
  if (f.dels.empty()) return;
  PostGroups pg;
  for (size_t j = 0; j < f.dels.size(); ++j) {
    Req& r = f.reqs[f.dels[j]];
    const bool found = f.del_found.host<uint8_t>()[j] != 0;
    if (r.dcb) pg.answer(r.ex, [cb = std::move(r.dcb), found]() { cb(found); });
  }
  pg.flush();
}

void HbmBackend::Dev::deliver_touches(Flight& f) {
  if (f.touches.empty()) return;
  PostGroups pg;
  for (size_t j = 0; j < f.touches.size(); ++j) {
    Req& r = f.reqs[f.touches[j]];
    const int st = f.touch_hit[f.trow[j]] ? 1 : 0;  // (every request of a key: its row's answer)
    if (r.tcb) pg.answer(r.ex, [cb = std::move(r.tcb), st]() { cb(st); });
  }
  pg.flush();
}

// Requests that cannot run: a GET misses, a DELETE or a touch finds nothing, a SET is
// dropped, a control request hears `false`.
void HbmBackend::Dev::fail_requests(std::vector<Req>& reqs, bool unlaunched) {
  PostGroups pg;
  for (auto& r : reqs) {
    if (unlaunched && is_write(r.kind)) be->write_end(r.d.lo);
    switch (r.kind) {
      case ReqKind::Get:
        if (r.gcb) pg.answer(r.ex, [cb = std::move(r.gcb)]() { cb(false, CacheValue{}); });
        break;
      case ReqKind::Set:
        dropped++;
        break;
      case ReqKind::Del:
        if (r.dcb) pg.answer(r.ex, [cb = std::move(r.dcb)]() { cb(false); });
        break;
      case ReqKind::Touch:
        if (r.tcb) pg.answer(r.ex, [cb = std::move(r.tcb)]() { cb(0); });
        break;
      case ReqKind::Slice:
        if (r.pcb) pg.answer(r.ex, [cb = std::move(r.pcb)]() { cb(PartValue{}); });
        break;
      case ReqKind::Barrier:
      case ReqKind::Fill:
      case ReqKind::Purge:
      case ReqKind::List:
        if (r.ccb) r.ccb(false);
        r.ccb = nullptr;
        break;
    }
  }
  pg.flush();
}

// A failed or stalled flight: its requests are answered (GET miss, DEL not found), the
// flight itself stays reserved until the GPU finishes with its buffers.
void HbmBackend::Dev::fail_flight(Flight& f) {
  failures++;
  if (!f.got) {
    fail_requests(f.reqs, false);
  } else {
    std::vector<Req> rest;
    for (const auto* v : {&f.dels, &f.touches, &f.slices, &f.ctls})
      for (uint32_t i : *v) rest.push_back(std::move(f.reqs[i]));
    fail_requests(rest, false);
  }
  f.got = true;
  f.gets.clear();
  f.slices.clear();
  f.dels.clear();
  f.touches.clear();
  f.ctls.clear();
  f.active = false;
}

// ---------------------------------------------------------------------------------
// ejection, restore, warm migration
// ---------------------------------------------------------------------------------
void HbmBackend::Dev::eject(const char* why) {
  if (up()) {
    std::fprintf(stderr, "[shellac hbm] ejecting gpu %d (%s); retry in %d s\n", device, why,
                 be->cfg_.retry_s);
    ejections++;
  }
  failed = true;
  retry_at = wall_s() + be->cfg_.retry_s;
  eject_gen.fetch_add(1, std::memory_order_acq_rel);
  set_up(false);
  be->spread_mask_.fetch_and(~(1ull << index), std::memory_order_acq_rel);
  std::vector<Req> pending;
  {
    std::lock_guard<std::mutex> lk(mu);
    pending.swap(q);
    qn.store(0, std::memory_order_release);
  }
  fail_requests(pending, true);
}

// Bring an ejected shard back: the fault drill was lifted, or retry_s passed and every
// flight has completed (the GPU answers again). Its contents may be stale (SETs routed
// elsewhere while it was out), so it is flushed unless configured otherwise.
void HbmBackend::Dev::maybe_restore() {
  if (forced_down.load(std::memory_order_acquire)) return;
  if (failed && wall_s() < retry_at) return;
  // (done before started: equal counts mean no purge was under way when they were read)
  const uint64_t purges_done = be->purge_done_.load(std::memory_order_acquire);
  const uint64_t purges_begun = be->purge_started_.load(std::memory_order_acquire);
  const bool dirty = purge_dirty.exchange(false, std::memory_order_acq_rel);
  try {
    for (auto& f : flights) HB_OK(hipEventSynchronize(f->ev));
    if (be->cfg_.flush_on_restore || dirty) cache->flush(stream);
    HB_OK(hipStreamSynchronize(stream));
  } catch (const std::exception&) {
    if (dirty) purge_dirty.store(true, std::memory_order_release);
    retry_at = wall_s() + be->cfg_.retry_s;
    return;
  }
  failed = false;
  for (size_t i = 0; i < inflight; ++i)  // every flight has finished: its writes end
    track_writes(*flights[(head + i) % flights.size()], -1);
  inflight = 0;
  head = 0;
  pend_w.clear();
  pend_flush = 0;
  for (auto& f : flights) {
    f->active = false;
    f->reqs.clear();
    f->arena.reset();
  }
  restores++;
  // Back in the ring first, then warm: objects of this shard's key range that its peers
  // took while it was out are copied back GPU-to-GPU, inserted only where this shard has
  // nothing yet — so a SET that reaches it from now on is never overwritten by an older
  // migrated copy (requests queued meanwhile run after the migration, on this thread).
  restoring.store(true, std::memory_order_release);
  set_up(true);
  uint64_t moved = 0;
  if (be->cfg_.warm_restore && be->cfg_.flush_on_restore) {
    for (auto& other : be->devs_) {
      if (other.get() == this || !other->up()) continue;
      try {
        moved += migrate_from(*other);
      } catch (const std::exception& e) {
        std::fprintf(stderr, "[shellac hbm] warm restore from gpu %d failed: %s\n",
                     other->device, e.what());
      }
    }
  }
  // A purge that overlapped the restore found this shard out of service (purge_dirty) or
  // reached the peers only after their objects were copied here: drop what was warmed (the
  // requests queued since the shard is back run after this, on this thread).
  if (purge_dirty.exchange(false, std::memory_order_acq_rel) ||
      (moved && (purges_done != purges_begun ||
                 be->purge_started_.load(std::memory_order_acquire) != purges_begun))) {
    try {
      cache->flush(stream);
      HB_OK(hipStreamSynchronize(stream));
      moved = 0;
    } catch (const std::exception& e) {
      std::fprintf(stderr, "[shellac hbm] gpu %d flush after a purge failed: %s\n", device,
                   e.what());
      restoring.store(false, std::memory_order_release);
      eject("flush error");
      purge_dirty.store(true, std::memory_order_release);
      return;
    }
  }
  restoring.store(false, std::memory_order_release);
  std::fprintf(stderr, "[shellac hbm] gpu %d back in service (%llu objects warmed from peers)\n",
               device, (unsigned long long)moved);
}

void copy_between(void* dst, int dst_dev, const void* src, int src_dev, size_t bytes,
                  hipStream_t stream, int path) {
  if (!bytes) return;
  if (path == 0) {
    HB_OK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, stream));
  } else if (path == 1) {
    HB_OK(hipMemcpyPeerAsync(dst, dst_dev, src, src_dev, bytes, stream));
  } else {
    const size_t piece = std::min<size_t>(bytes, 64u << 20);
    void* h = nullptr;
    HB_OK(hipHostMalloc(&h, piece, hipHostMallocDefault));
    try {
      HB_OK(hipStreamSynchronize(stream));  // earlier work on dst's stream first
      for (size_t o = 0; o < bytes; o += piece) {
        const size_t n = std::min(piece, bytes - o);
        HB_OK(hipSetDevice(src_dev));
        HB_OK(hipMemcpy(h, static_cast<const uint8_t*>(src) + o, n, hipMemcpyDeviceToHost));
        HB_OK(hipSetDevice(dst_dev));
        HB_OK(hipMemcpy(static_cast<uint8_t*>(dst) + o, h, n, hipMemcpyHostToDevice));
      }
    } catch (...) {
      (void)hipHostFree(h);
      throw;
    }
    HB_OK(hipHostFree(h));
  }
}

// Peer migration src -> this (both GPUs' HbmCache APIs are thread-safe; src's work goes
// on src's migration stream, beside src's own batcher): export src's live digests, route
// them on src's GPU, take the ones this shard owns (migrate_candidates); then per chunk
// (migrate_chunk) look them up and gather their records on src, hipMemcpyPeerAsync the
// records to this GPU, turn them into a SET batch (insert-if-absent against this shard's own
// lookup) and store them; finally delete them from src, where nothing routes any more.
// Chunked so a store stays within half a log.
uint64_t HbmBackend::Dev::migrate_from(Dev& src) {
  TraceRange tr("hbm_backend.migrate");
  const double t0 = wall_s();
  const uint32_t t = be->now();
  std::vector<Digest> mine;
  if (!migrate_candidates(src, t, &mine)) return 0;
  if (be->cfg_.presence_filter && !mine.empty()) {  // GETs routed here must not skip them
    std::lock_guard<std::mutex> lk(mu);
    for (const Digest& d : mine) {
      filt->add(d);
      if (filt_next) filt_next->add(d);
    }
  }
  uint64_t moved = 0;
  const size_t chunk = 65536;
  for (size_t c0 = 0; c0 < mine.size(); c0 += chunk)
    moved += migrate_chunk(src, mine.data() + c0, (int64_t)std::min(chunk, mine.size() - c0), t);
  migrated += moved;
  migrate_ns += (uint64_t)((wall_s() - t0) * 1e9);
  return moved;
}

// On src: its live digests that this shard owns under the full ring, the hot ones left out
// (false: src holds nothing).
bool HbmBackend::Dev::migrate_candidates(Dev& src, uint32_t t, std::vector<Digest>* out) {
  const int W = (int)be->devs_.size();
  std::vector<Digest>& mine = *out;
  HB_OK(hipSetDevice(src.device));
  const uint64_t live = src.cache->export_keys(nullptr, 0, t, src.mstream);
  if (!live) {
    HB_OK(hipSetDevice(device));
    return false;
  }
  Digest* s_keys = nullptr;
  int32_t* s_dest = nullptr;
  int64_t* s_cnt = nullptr;
  HB_OK(hipMalloc(&s_keys, live * sizeof(Digest)));
  HB_OK(hipMalloc(&s_dest, live * sizeof(int32_t)));
  HB_OK(hipMalloc(&s_cnt, W * sizeof(int64_t)));
  std::vector<int32_t> dest;
  std::vector<Digest> keys;
  uint64_t got = 0;
  try {
    got = std::min(live, src.cache->export_keys(s_keys, live, t, src.mstream));
    HB_OK(hipMemsetAsync(s_cnt, 0, W * sizeof(int64_t), src.mstream));
    route_keys(s_keys, (int64_t)got, src.d_pts, src.d_own, src.npts, s_dest, s_cnt, W,
               src.mstream);
    dest.resize(got);
    keys.resize(got);
    HB_OK(hipMemcpyAsync(dest.data(), s_dest, got * sizeof(int32_t), hipMemcpyDeviceToHost,
                         src.mstream));
    HB_OK(hipMemcpyAsync(keys.data(), s_keys, got * sizeof(Digest), hipMemcpyDeviceToHost,
                         src.mstream));
    HB_OK(hipStreamSynchronize(src.mstream));
  } catch (...) {
    (void)hipFree(s_keys); (void)hipFree(s_dest); (void)hipFree(s_cnt);
    throw;
  }
  (void)hipFree(s_dest);
  (void)hipFree(s_cnt);
  for (uint64_t i = 0; i < got; ++i)
    if (dest[i] == index) mine.push_back(keys[i]);
  (void)hipFree(s_keys);
  if (be->hot_on_ && !mine.empty()) {
    // hot objects stay where they are: the peers hold write-through replicas (they keep
    // serving the GETs spread to them), and this shard receives the whole hot set from the
    // next refresh's heal fill before it rejoins the spread mask
    const HostRouter::Read rd(*be->router_);
    mine.erase(std::remove_if(mine.begin(), mine.end(),
                              [&](const Digest& d) { return rd.hot_rank(d) != HostRouter::kNotHot; }),
               mine.end());
  }
  return true;
}

// One chunk of a migration: m digests of src's that this shard owns; returns how many
// objects arrived here.
uint64_t HbmBackend::Dev::migrate_chunk(Dev& src, const Digest* keys, int64_t m, uint32_t t) {
  uint64_t moved = 0;
  const uint64_t rec_cap = std::max<uint64_t>(cache->config().log_bytes / 8, 1u << 20);
  // ---- on src: look the chunk up (misses the tail the next appends will overwrite)
  HB_OK(hipSetDevice(src.device));
  Digest* sk = nullptr;
  uint64_t *sloc = nullptr, *ssize = nullptr, *soff = nullptr;
  uint8_t* srec = nullptr;
  HB_OK(hipMalloc(&sk, m * sizeof(Digest)));
  HB_OK(hipMalloc(&sloc, m * 8));
  HB_OK(hipMalloc(&ssize, (m + 1) * 8));
  HB_OK(hipMalloc(&soff, (m + 1) * 8));
  uint64_t total = 0;
  HB_OK(hipMemcpyAsync(sk, keys, m * sizeof(Digest), hipMemcpyHostToDevice, src.mstream));
  src.cache->lookup(sk, m, sloc, ssize, soff, t, src.mstream, src.cache->config().log_bytes / 8);
  HB_OK(hipMemcpyAsync(&total, soff + m, 8, hipMemcpyDeviceToHost, src.mstream));
  HB_OK(hipStreamSynchronize(src.mstream));
  if (total > rec_cap) total = 0;  // pathological chunk: skip it (objects just miss)
  if (total) {
    HB_OK(hipMalloc(&srec, total + 16));
    src.cache->gather(sloc, soff, m, srec, src.mstream);
    HB_OK(hipStreamSynchronize(src.mstream));
  }
  // ---- to this GPU over xGMI, insert-if-absent, store
  HB_OK(hipSetDevice(device));
  Digest* kk = nullptr;
  uint64_t *koff = nullptr, *ksize = nullptr, *kloc = nullptr, *khave = nullptr,
           *khoff = nullptr, *kvoff = nullptr;
  uint8_t* krec = nullptr;
  uint32_t* kmeta = nullptr;
  Digest* skeys2 = nullptr;
  bool ok = true;
  try {
    if (total) {
      HB_OK(hipMalloc(&kk, m * sizeof(Digest)));
      HB_OK(hipMalloc(&koff, (m + 1) * 8));
      HB_OK(hipMalloc(&ksize, (m + 1) * 8));
      HB_OK(hipMalloc(&kloc, m * 8));
      HB_OK(hipMalloc(&khave, (m + 1) * 8));
      HB_OK(hipMalloc(&khoff, (m + 1) * 8));
      HB_OK(hipMalloc(&kvoff, m * 8));
      HB_OK(hipMalloc(&kmeta, 3 * m * 4));
      HB_OK(hipMalloc(&skeys2, m * sizeof(Digest)));
      HB_OK(hipMalloc(&krec, total + 16));
      const int path = be->peer_path(src.device, device);
      copy_between(krec, device, srec, src.device, total, stream, path);
      copy_between(koff, device, soff, src.device, (m + 1) * 8, stream, path);
      copy_between(ksize, device, ssize, src.device, (m + 1) * 8, stream, path);
      copy_between(kk, device, sk, src.device, m * sizeof(Digest), stream, path);
      if (path == 2) staged_copies++;
      cache->lookup(kk, m, kloc, khave, khoff, t, stream);
      records_to_set(krec, koff, ksize, khave, m, skeys2, kvoff, kmeta, kmeta + m, kmeta + 2 * m,
                     stream);
      cache->store(skeys2, krec, kvoff, kmeta, kmeta + m, kmeta + 2 * m, m, total + 48 * m, t,
                   stream);
      HB_OK(hipStreamSynchronize(stream));
      std::vector<uint64_t> sz(m);
      HB_OK(hipMemcpy(sz.data(), ksize, m * 8, hipMemcpyDeviceToHost));
      for (int64_t i = 0; i < m; ++i) moved += sz[i] ? 1 : 0;
    }
  } catch (...) {
    ok = false;
  }
  for (void* p : {(void*)kk, (void*)koff, (void*)ksize, (void*)kloc, (void*)khave,
                  (void*)khoff, (void*)kvoff, (void*)krec, (void*)kmeta, (void*)skeys2})
    (void)hipFree(p);
  // ---- src no longer serves these digests
  HB_OK(hipSetDevice(src.device));
  if (ok && total) {
    src.cache->remove(sk, m, nullptr, t, src.mstream);
    HB_OK(hipStreamSynchronize(src.mstream));
  }
  for (void* p : {(void*)sk, (void*)sloc, (void*)ssize, (void*)soff, (void*)srec})
    (void)hipFree(p);
  HB_OK(hipSetDevice(device));
  if (!ok) throw Error("peer migration chunk failed");
  return moved;
}

void HbmBackend::Dev::sweep() {
  TraceRange tr("hbm_backend.sweep");
  uint64_t o = 0, b = 0;
  cache->sweep(be->now(), stream, &o, &b);
  live_objects = o;
  live_bytes = b;
  sweeps++;
}

void HbmBackend::Dev::finish_filter_rebuild() {
  TraceRange tr("hbm_backend.filter_rebuild");
  const uint32_t t = be->now();
  const uint64_t live = cache->export_keys(nullptr, 0, t, stream);
  if (live) {
    // the kernel writes the digests straight into mapped host memory (no device buffer)
    Mapped m;
    m.ensure(live * sizeof(Digest));
    uint64_t got = 0;
    try {
      got = std::min(live, cache->export_keys(m.dev<Digest>(), live, t, stream));
    } catch (...) {
      m.release();
      throw;
    }
    for (uint64_t i = 0; i < got; ++i) filt_next->add(m.host<Digest>()[i]);
    m.release();
  }
  std::lock_guard<std::mutex> lk(mu);
  std::atomic_store(&filt, filt_next);
  filt_next.reset();
  filt_rebuild_at = filt->adds() + be->cfg_.nbuckets_per_gpu * kEntriesPerBucket;
  filt_rebuilds++;
}

}  // namespace shellac
