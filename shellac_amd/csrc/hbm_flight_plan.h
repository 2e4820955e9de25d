// HbmBackend's host-only decisions as plain functions over requests: which queued requests
// share a flight, which GETs and touches share a GPU row, which shards a write goes to, how
// the answers of a fanned-out write become one, and what a hot-set refresh fills and
// publishes. No HIP here: the batcher (hbm_batcher.cc), the request API (backend_hbm.cc) and
// the refresh (hbm_hot.cc) call these, and tests/native/native_tests.cc runs them without a GPU.
#pragma once

#include <algorithm>
#include <unordered_set>

#include "backend.h"
#include "keyed.h"

namespace shellac {

using HbmReq = HbmBackend::Req;

// ---- flights ------------------------------------------------------------------------------
// plan_take's sets, kept by the caller so a batcher does not allocate per flight: the write
// digests (lo words) seen so far, and those of them that are touches.
struct TakeScratch {
  std::unordered_set<uint64_t> writes, touches;
};

// How many requests at the front of `q` form the next flight (at least 1 of a non-empty
// queue, at most max(max_batch, 1)). A flight runs its GETs and slices, then its SETs and
// DELETEs, then its touches, then a fill or a purge, so:
//  * a GET or a slice queued behind a write of its key ends the flight before itself (read-your-writes
//    for a client that re-reads right after a fill: it goes into the next flight, which is
//    ordered after this one);
//  * a SET or DELETE queued behind a touch of its key ends the flight before itself (a touch
//    behind a SET or a touch of its key stays: that is the order they run in);
//  * a fill or a purge ends the flight after itself (it runs after the flight's writes, and
//    the writes queued behind a purge must not run before it).
// A barrier never cuts.
inline size_t plan_take(const std::vector<HbmReq>& q, int max_batch, TakeScratch& s) {
  size_t take = std::min(q.size(), (size_t)std::max(max_batch, 1));
  s.writes.clear();
  s.touches.clear();
  for (size_t i = 0; i < take; ++i) {
    const HbmReq& r = q[i];
    switch (r.kind) {
      case ReqKind::Get:
      case ReqKind::Slice:  // (a read: planned as a GET)
        if (!s.writes.empty() && s.writes.count(r.d.lo)) return i;
        break;
      case ReqKind::Set:
      case ReqKind::Del:
        if (!s.touches.empty() && s.touches.count(r.d.lo)) return i;
        s.writes.insert(r.d.lo);
        break;
      case ReqKind::Touch:
        s.writes.insert(r.d.lo);
        s.touches.insert(r.d.lo);
        break;
      case ReqKind::Fill:
      case ReqKind::Purge:
      case ReqKind::List:  // (sees the flight's writes, and one listing runs at a time)
        return i + 1;
      case ReqKind::Barrier:
        break;
    }
  }
  return take;
}
inline size_t plan_take(const std::vector<HbmReq>& q, int max_batch) {
  TakeScratch s;
  return plan_take(q, max_batch, s);
}

// ---- GET rows -----------------------------------------------------------------------------
// Equal digests among a flight's GETs share one GPU row (a hot object under concurrent
// clients is one row and one arena record). rows[0..n) receives the distinct digests in
// order of first appearance (room for gets.size()), urow[j] the row of GET j; `tab` is the
// caller's scratch. Returns n.
inline size_t coalesce_gets(const std::vector<HbmReq>& reqs, const std::vector<uint32_t>& gets,
                            std::vector<int32_t>& tab, Digest* rows, uint32_t* urow) {
  size_t tsz = 16, n = 0;
  while (tsz < 2 * gets.size()) tsz <<= 1;
  tab.assign(tsz, -1);
  for (size_t j = 0; j < gets.size(); ++j) {
    const Digest& d = reqs[gets[j]].d;
    for (size_t h = (size_t)(d.hi ^ (d.hi >> 31)) & (tsz - 1);; h = (h + 1) & (tsz - 1)) {
      const int32_t u = tab[h];
      if (u < 0) {
        tab[h] = (int32_t)n;
        rows[n] = d;
        urow[j] = (uint32_t)n++;
        break;
      }
      if (rows[u].lo == d.lo && rows[u].hi == d.hi) {
        urow[j] = (uint32_t)u;
        break;
      }
    }
  }
  return n;
}

// ---- slice rows ---------------------------------------------------------------------------
// A flight's slices as the rows of one HbmCache::get_keyed_slices launch: one row per request,
// in request order (requests of one key may ask for different windows), the rows' key bytes
// packed with their n + 1 offsets.
struct SlicePlan {
  std::string kbytes;
  std::vector<int64_t> offs;
};
inline SlicePlan plan_slice_rows(const std::vector<HbmReq>& reqs,
                                 const std::vector<uint32_t>& slices) {
  SlicePlan p;
  p.offs.reserve(slices.size() + 1);
  p.offs.push_back(0);
  for (uint32_t i : slices) {
    p.kbytes += reqs[i].key;
    p.offs.push_back((int64_t)p.kbytes.size());
  }
  return p;
}

// ---- touch rows ---------------------------------------------------------------------------
// A flight's touches as the rows of two key-exact HbmCache::touch launches: one row per
// distinct (key bytes, digest) pair, the last request of a pair supplying ttl and flags
// (HbmCache::touch leaves duplicates to the caller); the rows that keep their object's flags
// first, in order of first arrival, then the rows that replace them.
struct TouchPlan {
  size_t nkeep = 0;            // rows [0, nkeep) keep their flags, [nkeep, rows()) replace them
  std::vector<uint32_t> src;   // row -> position in `touches` of the request it carries
  std::vector<uint32_t> trow;  // position in `touches` -> row (every request: its row's answer)
  std::string kbytes;          // the rows' key bytes, packed in row order
  // rows() + 2 words: the first launch's nkeep + 1 key offsets into kbytes, then the second
  // launch's own rows() - nkeep + 1, starting one word further on
  std::vector<int64_t> offs;
  size_t rows() const { return src.size(); }
  const int64_t* offs_keep() const { return offs.data(); }
  const int64_t* offs_replace() const { return offs.data() + nkeep + 1; }
};

inline TouchPlan plan_touch_rows(const std::vector<HbmReq>& reqs,
                                 const std::vector<uint32_t>& touches) {
  TouchPlan p;
  const size_t nt = touches.size();
  // distinct (key, digest) pairs in arrival order; `last`: the last request of each
  std::unordered_map<std::string, uint32_t> seen;
  std::vector<uint32_t> last, pair_of(nt);
  for (size_t j = 0; j < nt; ++j) {
    const HbmReq& r = reqs[touches[j]];
    std::string id = r.key;
    id.append(reinterpret_cast<const char*>(&r.d), sizeof(Digest));
    const auto it = seen.emplace(std::move(id), (uint32_t)last.size());
    if (it.second) last.push_back((uint32_t)j);
    else last[it.first->second] = (uint32_t)j;
    pair_of[j] = it.first->second;
  }
  const size_t n = last.size();
  const auto keeps = [&](uint32_t k) { return !reqs[touches[last[k]]].has_flags; };
  std::vector<uint32_t> order(n), row_of(n);
  for (size_t k = 0; k < n; ++k) order[k] = (uint32_t)k;
  p.nkeep = (size_t)(std::stable_partition(order.begin(), order.end(), keeps) - order.begin());
  p.src.resize(n);
  p.offs.assign(n + 2, 0);
  for (size_t row = 0; row < n; ++row) {
    const size_t second = row >= p.nkeep ? 1 : 0;
    const std::string& key = reqs[touches[last[order[row]]]].key;
    row_of[order[row]] = (uint32_t)row;
    p.src[row] = last[order[row]];
    p.offs[row + second] = (int64_t)p.kbytes.size();
    p.kbytes += key;
    if (row + 1 == p.nkeep || row + 1 == n) p.offs[row + 1 + second] = (int64_t)p.kbytes.size();
  }
  p.trow.resize(nt);
  for (size_t j = 0; j < nt; ++j) p.trow[j] = row_of[pair_of[j]];
  return p;
}

// ---- write routing ------------------------------------------------------------------------
// The shards a SET, DELETE or touch is queued to, in queueing order: its owner, then (a hot
// object is written through to its replicas) every other shard in service, ascending.
struct WriteTargets {
  int n = 0;
  int shard[64];
  const int* begin() const { return shard; }
  const int* end() const { return shard + n; }
};
inline WriteTargets write_targets(int owner, bool hot, uint64_t up_mask, int nshards) {
  WriteTargets t;
  t.shard[t.n++] = owner;
  for (int k = 0; hot && k < nshards && k < 64; ++k)
    if (k != owner && ((up_mask >> k) & 1)) t.shard[t.n++] = k;
  return t;
}

// The answers of a write's n copies folded into one: `takes(answer, from_owner)` says whether
// an answer becomes the result (which starts as `init`); the copy that answers last, on
// whichever thread, calls `done` with it.
template <typename T>
struct FanIn {
  using Takes = bool (*)(T answer, bool from_owner);
  FanIn(int n, T init, Takes takes, std::function<void(T)> done)
      : left(n), result(init), takes(takes), done(std::move(done)) {}
  // the callback of one copy
  static std::function<void(T)> arm(std::shared_ptr<FanIn> f, bool from_owner) {
    return [f = std::move(f), from_owner](T answer) {
      if (f->takes(answer, from_owner)) f->result.store(answer, std::memory_order_relaxed);
      if (f->left.fetch_sub(1, std::memory_order_acq_rel) == 1 && f->done)
        f->done(f->result.load(std::memory_order_relaxed));
    };
  }
  std::atomic<int> left;
  std::atomic<T> result;
  Takes takes;
  std::function<void(T)> done;
};
// DELETE: found anywhere
inline bool fan_any(bool found, bool) { return found; }
// touch: the owner's answer (the replicas follow the owner's copy)
inline bool fan_owner(int, bool from_owner) { return from_owner; }

// ---- listing ------------------------------------------------------------------------------
// A list_objects call visits the shards in ascending order, one at a time. The cursor is
// (shard, slot): shards before the cursor's only count (the totals cover every shard in
// service on every page), the cursor's shard lists from its slot, later shards from slot 0,
// each asked for the rows still wanted; once a shard has more matches than were wanted the
// cursor for the next page is known and the rest only count.
struct ListAsk {
  int shard = -1;       // -1: no shard is left, the walk answers
  uint64_t start = 0;
  uint32_t limit = 0;   // 0: count only
  uint32_t skipped = 0; // shards out of service passed over on the way
};
inline ListAsk list_next_ask(int after_shard, int cur_shard, uint64_t cur_slot, bool have_next,
                             uint32_t wanted, uint64_t up_mask, int nshards) {
  ListAsk a;
  for (int k = after_shard + 1; k < nshards && k < 64; ++k) {
    if (!((up_mask >> k) & 1)) {
      ++a.skipped;
      continue;
    }
    a.shard = k;
    if (k >= cur_shard && !have_next) {
      a.limit = wanted;
      a.start = k == cur_shard ? cur_slot : 0;
    }
    break;
  }
  return a;
}
// A row is a hot replica, dropped from the listing on the host, if its digest's ketama owner
// among the shards in service is another shard than the one that listed it.
inline bool list_row_is_replica(int owner, int shard) { return owner >= 0 && owner != shard; }
// After a shard answered `listed` of the `asked` rows with `next_slot` (nslots: it has no
// further match): the cursor of the next page, if it is known now. Empty: go on.
inline std::string list_cursor_after(int shard, uint32_t asked, uint32_t still_wanted,
                                     uint64_t next_slot, uint64_t nslots, int nshards) {
  if (!asked) return std::string();
  if (next_slot < nslots) return hbm_cursor(shard, next_slot);
  // exhausted exactly as the page filled: the next page starts on the next shard
  if (!still_wanted && shard + 1 < nshards) return hbm_cursor(shard + 1, 0);
  return std::string();
}

// ---- hot-set refresh ----------------------------------------------------------------------
using DigestSet = std::unordered_set<Digest, DigestHash, DigestEq>;

// The fill budget: of the planned objects (hottest first) the added ones whose records,
// copied to `targets` shards each, no longer fit `budget` bytes are deferred to a later
// refresh. rec_bytes(d): the size of d's record in its owner's snapshot (0: none).
template <typename RecBytes>
DigestSet hot_fill_deferred(const std::vector<Digest>& planned, const DigestSet& added,
                               RecBytes rec_bytes, uint64_t targets, uint64_t budget) {
  DigestSet deferred;
  uint64_t spent = 0;
  for (const Digest& d : planned) {
    if (!added.count(d)) continue;
    const uint64_t b = rec_bytes(d) * targets;
    if (spent + b > budget) deferred.insert(d);
    else spent += b;
  }
  return deferred;
}

// The table a refresh publishes last (T2): the planned set without the added objects that
// were deferred or whose owner's snapshot failed, with the planned weights of the shards in
// `mask`; nowhere to spread means no hot set.
struct HotTable {
  std::vector<Digest> hot;
  std::vector<int32_t> rank;
  std::vector<double> wts;
  // equal to the published table (which is then not republished)
  bool same_as(const std::vector<Digest>& hot0, const std::vector<int32_t>& rank0,
               const std::vector<double>& wts0) const {
    return rank == rank0 && wts == wts0 && hot.size() == hot0.size() &&
           std::equal(hot.begin(), hot.end(), hot0.begin(), DigestEq());
  }
};
inline HotTable hot_final_table(const HotPlan& plan, const DigestSet& added,
                                const DigestSet& deferred, const DigestSet& snapshot_ok,
                                uint64_t mask, int nshards) {
  HotTable t;
  for (size_t i = 0; i < plan.hot.size(); ++i) {
    const Digest& d = plan.hot[i];
    if (added.count(d) && (deferred.count(d) || !snapshot_ok.count(d))) continue;
    t.hot.push_back(d);
    t.rank.push_back(plan.rank[i]);
  }
  t.wts.assign((size_t)nshards, 0.0);
  double wsum = 0;
  for (int r = 0; r < nshards; ++r)
    if ((mask >> r) & 1) wsum += (t.wts[(size_t)r] = plan.weights[(size_t)r]);
  if (wsum <= 0) {
    t.hot.clear();
    t.rank.clear();
    t.wts.assign((size_t)nshards, 1.0);
  }
  return t;
}

}  // namespace shellac
