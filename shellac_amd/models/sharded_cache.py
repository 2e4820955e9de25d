"""ShardedCache: the flagship "model" — one logical cache over every GPU of a job.

Reference capability: "a single logical cache out of extra memory across the
entire cluster" (README.md:12, :30) built from ketama-sharded memcached nodes
(src/python/shellac/server/Server.py:79-83). Here each rank owns one
``CacheShard`` (its GPU's HBM) and a ``ShardRing`` assigns digests to ranks.

This module is the facade and the cluster-level operations: the ring, the hot-set
election and replica refresh, incremental migration, failing and restoring a shard,
snapshots and counters. ``get``, ``set``, ``delete``, ``serve`` and ``sync_sets``
dispatch to one of two step objects, which read the knobs set here at call time:

  * ``local_step.LocalStep``: one rank, not routed — every step is purely local; on a
    GPU the pipelined step the headline benchmark times (its streams, events and
    buffers live there);
  * ``routed_step.DeviceRoutedStep``: batches routed between the ranks on the device
    with RCCL all-to-alls (experimental; the phase lists are in that module).

Hot-object replication (SURVEY.md §5.8 "hot-key broadcast"): Zipf-popular
objects are copied into a small per-rank *replica* shard so their GETs never
leave the GPU. ``refresh_replica`` picks the global top-k keys from recent
request samples (one all_gather of candidates + one routed GET). Consistency is
write-through with no extra collective: a SET for a replicated key is fanned out
by the same all-to-all to its owner (main shard) and to every other rank
(replica shard), so a GET issued after a SET step never sees the old value.
"""
from __future__ import annotations

import os
from typing import List, Optional

import torch
import torch.distributed as dist

from ..ops import routing as R
from ..ops.cache import CacheShard
from ..parallel.exchange import MirrorComm, all_gather, all_reduce, allreduce_stats, dist_info
from ..parallel.ring import ShardRing
from .batch import SKIP_VLEN, GetResult, SetBatch, records_to_set_batch  # noqa: F401
from .local_step import LocalStep
from .routed_step import DeviceRoutedStep


class ShardedCache:
    HANDS = ("early", "inline")

    def __init__(self, shard: CacheShard, group=None, points_per_shard: int = 160,
                 replica: Optional[CacheShard] = None, sample_rows: int = 65536,
                 sample_batches: int = 8, data_group=None, routed: Optional[bool] = None,
                 comm_mode: str = "channels", hand: str = "early"):
        self.shard = shard
        self.group = group
        # native routed step: "single" = every collective of a step on one communicator and
        # one stream in a fixed order (cannot deadlock); "channels" (the default) = one
        # communicator per channel (control, reply, SET) on the stream producing its data
        if comm_mode not in ("single", "channels"):
            raise ValueError(f"comm_mode must be 'single' or 'channels', not {comm_mode!r}")
        self.comm_mode = comm_mode
        # Optional second communicator for the value all-to-all: its stream runs the
        # previous step's value transfer while this step's small exchanges proceed.
        self.data_group = data_group if data_group is not None else group
        self.rank, self.world = dist_info(group)
        # routed: batches go through the collectives (routing, all-to-alls, replica tier).
        # Default: with more than one rank. routed=True at world 1 runs the same path over
        # a one-rank group — a real RCCL communicator on one GPU (the test and rehearsal of
        # the multi-GPU step's collective calls that a one-GPU box can run)
        self.routed = self.world > 1 if routed is None else bool(routed)
        self.device = shard.device
        self.ring = ShardRing(list(range(self.world)), points_per_shard)
        self.ring_pts, self.ring_own = self.ring.tensors(self.device)
        self.replica = replica if self.routed else None
        self.sample_rows = sample_rows
        self.sample_batches = sample_batches
        self._samples: List[torch.Tensor] = []
        self._hot: Optional[torch.Tensor] = None   # sorted hot digests [h, 2] (same on all ranks)
        # GPU shards run the routed step through the fused native ops (csrc/router.hip);
        # the framework-op version (_serve_routed) is the CPU path and the test oracle
        self.fused = True
        # incremental migration (set_ring): the keys still to move, how many per chunk, and
        # the keys SET / DELETEd since the ring switch
        self._migrating = None
        self._migrate_chunk = 1 << 18
        self._touched = None
        self._touched_all = None
        # simulated world: request digests -> the digests their owners hold (see serve)
        self.probe_of = None
        # replica refresh: scores of the hot keys (aligned with _hot) and their decay per
        # refresh (_hot_candidates)
        self._hot_score = None
        self.hot_decay = 0.5
        # run SET chains on a side stream, concurrently with GET gathers (GPU shards)
        self.overlap_store = True
        # GET coalescing: the duplicate keys of a batch share one probe and one record
        # (ops.cache.coalesce); False probes and copies every request (bench --no-coalesce)
        self.coalesce = True
        # (Two other N=1 schedules were measured slower and removed: a compacting lookup
        # with bump-allocated response offsets, and the SET planning kernels ahead of the
        # lookup; profiles/archive/r2_step_schedule_ab.md.)
        # (Queuing the SET index insert after the host read the lookup total, with no
        # event between lookup and gather, needs the total published only once every
        # lookup workgroup has released its outputs: a device-scope fence per workgroup,
        # which cost ~30 us per step in k_offsets. Not adopted.)
        # fence scope of the events that order the main and side streams of a step:
        # "system" = torch's events (a system-scope release: L2 write-back + invalidate
        # at every record); "device" / "none" (default) = StreamEvent with a device-scope
        # release / no system fence (both streams are on one GPU; nothing on the host reads
        # what these events order, and every kernel dispatch carries its own release). One
        # box, two rounds: 0.309 / 0.308 ms per step with "device" vs 0.315 / 0.311 with
        # "system" (profiles/archive/r2_event_fence_ab.log); round 4, one box, two rounds each:
        # wrapped 0.3362 / 0.3363 "device" vs 0.3313 / 0.3304 "none", fresh 0.3008 / 0.3004
        # vs 0.2953 / 0.2952 (profiles/archive/r4h_fence)
        self.event_fence = "none"
        # the step's cross-stream events ride on the kernels' own completion signals: the
        # lookup's probe completes `probe` (the index insert's wait), the SET chain's index
        # fix-up completes the step's end (the next lookup's wait), and the log append waits
        # for the step's input event instead of a `start` marker behind the previous chain
        # — no marker packet on the main stream's critical path (each costs ~2.7 us; a stop
        # event is seen ~2.4 us sooner across streams than a recorded one: profiles/r6_hop).
        # Needs StreamEvents (event_fence != "system"). SHELLAC_STOP_EVENTS=0: markers.
        self.stop_events = os.environ.get("SHELLAC_STOP_EVENTS", "1") != "0"
        # fence scope of the events kernels complete as stop events (A/B: SHELLAC_STOP_FENCE)
        self.stop_fence = os.environ.get("SHELLAC_STOP_FENCE", "none")
        # one GPU: the gather waits for the SET batch's log append (see serve)
        self.gather_after_append = False
        # one GPU, a full cache: where the SET batch's CLOCK hand runs (see serve).
        # "early": detached, on a stream of its own, as soon as the previous step's SET
        # planning is done — beside that step's log append, index insert and gather; its
        # reinsertions are indexed as moves (HbmCache::store). "inline": at the head of the
        # SET chain on the side stream, after the lookup is queued.
        if hand not in self.HANDS:
            raise ValueError(f"hand must be one of {self.HANDS}, not {hand!r}")
        self.hand = hand
        # host edge (one rank): GET digests / SET payloads may be pinned host tensors and
        # responses are gathered straight into pinned host memory, as the proxy's HBM
        # tier does (bench.py --edge host)
        self.host_edge = False
        # host edge: the gather writes the response into HBM and a DMA engine copies it to
        # the pinned host buffer (56 GB/s D2H, scripts/pcie_d2h_micro.py) instead of the
        # gather kernel storing over PCIe itself (~38 GB/s)
        self.host_edge_dma = True
        self.gathered_bytes = 0  # response bytes the serving steps produced
        self._stats = {"get_requests": 0, "set_requests": 0, "remote_gets": 0,
                      "replica_hits": 0, "replica_refreshes": 0, "coalesced_gets": 0,
                      "slot_overflow_rows": 0, "reply_dropped_rows": 0}
        # the two serving paths; each holds its own streams, events and buffers
        self._local_step = LocalStep(self)
        self._routed_step = DeviceRoutedStep(self)

    # ------------------------------------------------------------------------------
    @property
    def _engine(self):  # the routed step's native executor (None before its first step)
        return self._routed_step._engine

    @property
    def _calibrations(self) -> int:  # routed steps that took the calibrating path
        return self._routed_step._calibrations

    @property
    def _co_table(self):  # the one-GPU step's coalescing table (the tests check it is left zeroed)
        return self._local_step._co_table

    @property
    def stats(self) -> dict:
        """Serving counters. The native routed step learns its own per-step numbers two
        steps late (it never waits for a step's matrix); reading them here collects every
        step issued so far (waiting for the latest step's all-gather, not for the step)."""
        self._routed_step.harvest()
        return self._stats

    def sync_sets(self) -> None:
        """Order the current stream after the SETs of the last ``serve`` (which leaves its
        SET chain, on a stream of its own, for the next step to join). Every other
        ShardedCache method calls it; call it before using ``self.shard`` directly after a
        ``serve`` (a device synchronisation also does)."""
        self._local_step.join()
        self._routed_step.join()

    def recalibrate(self) -> None:
        """Collective. The routed step sizes its per-peer exchange slots from the demand
        of earlier steps; after a change of batch shape (say, a much larger GET batch)
        the first steps would answer the rows that do not fit as misses until the
        capacities catch up. Calling this on every rank makes the next serve measure the
        new demand exactly (one step with two host reads) instead."""
        self.sync_sets()
        self._routed_step.reset_exchange()

    def _route(self, keys: torch.Tensor):
        return R.route(keys, self.ring_pts, self.ring_own, self.world)

    def _sample(self, keys: torch.Tensor) -> None:
        if self.replica is None:
            return
        self._samples.append(keys[: self.sample_rows])
        if len(self._samples) > self.sample_batches:
            self._samples.pop(0)

    def _is_hot(self, keys: torch.Tensor) -> torch.Tensor:
        """Membership of each digest in the replicated hot set (device op, no sync)."""
        return self._member(keys, self._hot)

    def get(self, keys: torch.Tensor, now: Optional[int] = None,
            probe_keys: Optional[torch.Tensor] = None) -> GetResult:
        """GET a batch (collective when routed). ``probe_keys`` (simulated world only): the
        digests the owners probe for each request."""
        self.sync_sets()
        self._stats["get_requests"] += keys.shape[0]
        if self.routed:
            return self._routed_step.get(keys, now, probe_keys)
        return self._local_step.get(keys, now)

    def serve(self, keys: torch.Tensor, batch: SetBatch, now: Optional[int] = None,
              inputs_ready=None, probe_keys: Optional[torch.Tensor] = None) -> GetResult:
        """One serving step: a GET batch and a SET batch, GETs ordered before SETs
        (``LocalStep.serve``; routed: ``DeviceRoutedStep.serve``).
        ``inputs_ready`` (optional ``torch.cuda.Event``, GPU step): an event after which
        ``keys`` and ``batch`` are complete. The step's planning then starts as soon as the
        previous step allows, not after everything the caller queued on the current stream.
        ``probe_keys`` / ``batch.probe_keys`` (simulated world, routed GPU step only): the
        digests owners probe and store (bench.py --simulate-world maps every key onto one
        the simulated rank owns, so its shard holds 1/N of the key space like a real one)."""
        self._touch(batch.keys)
        self._stats["get_requests"] += keys.shape[0]
        self._stats["set_requests"] += batch.keys.shape[0]
        if self.routed:
            return self._routed_step.serve(keys, batch, now, inputs_ready, probe_keys)
        return self._local_step.serve(keys, batch, now, inputs_ready)

    def set(self, batch: SetBatch, now: Optional[int] = None, if_absent: bool = False) -> None:
        """SET a batch (collective when routed). ``if_absent``: an owner stores a row only
        when it holds no live object of the key (a migration's delivery, which must never
        overwrite a newer value the owner received directly)."""
        self.sync_sets()
        if not if_absent:  # (a migration's own delivery is not a newer write)
            self._touch(batch.keys)
        n = batch.keys.shape[0]
        self._stats["set_requests"] += n
        if self.routed:
            return self._routed_step.set(batch, now, if_absent)
        vlen = batch.vlen
        if if_absent and n:
            have = self.shard.lookup(batch.keys.contiguous(), now).size[:n] > 0
            vlen = torch.where(have, torch.full_like(vlen, SKIP_VLEN), vlen).contiguous()
        self.shard.store(batch.keys, batch.values, batch.val_off, vlen, batch.flags,
                         batch.expire, now)

    def delete(self, keys: torch.Tensor, now: Optional[int] = None) -> torch.Tensor:
        self.sync_sets()
        self._touch(keys)
        if self.routed:
            return self._routed_step.delete(keys, now)
        return self.shard.remove(keys, now)

    # ------------------------------------------------------------------------------
    def _hot_candidates(self, top_k: int, keys: Optional[torch.Tensor],
                        old: Optional[torch.Tensor] = None,
                        old_score: Optional[torch.Tensor] = None):
        """Collective: the global top-k digests by request count (from ``keys`` or the
        recent GET samples), the same on every rank, most requested first (ties in digest
        order: stable sorts of all-gathered / all-reduced counts, identical everywhere),
        and their scores. With the current hot set ``old`` (sorted by lo) and its scores
        from the last refresh, an old key scores decay * its old score + its requests now
        + 1 (hysteresis): the tail of a large hot set is seen a few times per sample at
        most, so a key only displaces a hot one when it is seen more often — the hot set
        follows a drift instead of churning on sampling noise."""
        dev, w = self.device, self.world
        if keys is None:
            keys = torch.cat(self._samples) if self._samples else torch.zeros((0, 2), dtype=torch.int64,
                                                                             device=dev)
        # count by the low digest word (a 1-D sort; two keys sharing it are vanishingly rare)
        if keys.shape[0]:
            ulo, inv, cnt = torch.unique(keys[:, 0].contiguous(), return_inverse=True,
                                         return_counts=True)
            uniq = torch.empty((ulo.numel(), 2), dtype=torch.int64, device=dev)
            uniq[inv] = keys
        else:
            ulo = torch.zeros(0, dtype=torch.int64, device=dev)
            uniq = torch.zeros((0, 2), dtype=torch.int64, device=dev)
            cnt = torch.zeros(0, dtype=torch.int64, device=dev)
        k = min(top_k, uniq.shape[0])
        top = torch.topk(cnt, k).indices if k else cnt[:0]
        cand = torch.zeros((top_k, 2), dtype=torch.int64, device=dev)
        ccnt = torch.zeros(top_k, dtype=torch.int64, device=dev)
        cand[:k] = uniq.index_select(0, top)
        ccnt[:k] = cnt.index_select(0, top)
        all_c = [torch.empty_like(cand) for _ in range(w)]
        all_n = [torch.empty_like(ccnt) for _ in range(w)]
        all_gather(all_c, cand, group=self.group)
        all_gather(all_n, ccnt, group=self.group)
        allc = torch.cat(all_c)
        alln = torch.cat(all_n)
        # merge by the low word (a 1-D sort), in digest order: identical on every rank
        ulo2, inv = torch.unique(allc[:, 0].contiguous(), return_inverse=True)
        u = torch.empty((ulo2.numel(), 2), dtype=torch.int64, device=dev)
        u[inv] = allc
        tot = torch.zeros(u.shape[0], dtype=torch.int64, device=dev).scatter_add_(0, inv, alln)
        # a key enters the hot set only once seen twice (a mirrored world counts every
        # sighting once per simulated rank)
        min_count = 2 * (w if isinstance(self.group, MirrorComm) else 1)
        keep = ((u != 0).any(dim=1)) & (tot >= min_count)  # (drops the padding rows too)
        u, score = u[keep], tot[keep].to(torch.float64)
        if old is not None and old.shape[0]:
            # the old keys' requests in this sample, summed over the ranks
            oc = torch.zeros(old.shape[0], dtype=torch.int64, device=dev)
            if ulo.numel():
                at = torch.clamp(torch.searchsorted(ulo, old[:, 0].contiguous()), max=ulo.numel() - 1)
                oc = torch.where(ulo.index_select(0, at) == old[:, 0], cnt.index_select(0, at), oc)
            all_reduce(oc, group=self.group)
            prev = old_score if old_score is not None else torch.zeros(old.shape[0], dtype=torch.float64,
                                                                       device=dev)
            osc = prev * self.hot_decay + oc.to(torch.float64) + 1.0
            fresh = ~self._member(u, old)
            u = torch.cat([old, u[fresh]])
            score = torch.cat([osc, score[fresh]])
        # (with an old hot set every old key stays in the ranking: the caller picks the
        # top-k among the keys it could put in place)
        order = torch.sort(-score, stable=True).indices
        if old is None or old.shape[0] == 0:
            order = order[:top_k]
        return u.index_select(0, order).contiguous(), score.index_select(0, order).contiguous()

    @staticmethod
    def _member(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
        """Rows of ``a`` that are rows of ``b`` (both [n, 2] digests; b sorted by lo)."""
        if a.shape[0] == 0 or b.shape[0] == 0:
            return torch.zeros(a.shape[0], dtype=torch.bool, device=a.device)
        at = torch.searchsorted(b[:, 0].contiguous(), a[:, 0].contiguous())
        at = torch.clamp(at, max=b.shape[0] - 1)
        return (b.index_select(0, at) == a).all(dim=1)

    def _fetch_into_replica(self, keys: torch.Tensor, now: Optional[int]) -> tuple:
        """Collective. GET ``keys`` through their owners (never the replica) and store the
        records in this rank's replica (keys this rank owns stay out: an owner serves its
        own keys from its main shard). Returns (objects stored, record bytes fetched)."""
        if keys.shape[0] == 0:
            return 0, 0
        saved = self.replica
        self.replica = None                               # fetch through the owners only
        try:
            res = self.get(keys, now, probe_keys=self.probe_of(keys) if self.probe_of else None)
        finally:
            self.replica = saved
        sb = records_to_set_batch(keys, res)
        owner, _ = self._route(keys)
        sb.vlen = torch.where(owner == self.rank, torch.full_like(sb.vlen, SKIP_VLEN), sb.vlen)
        # store in chunks with exact byte bounds (the records buffer can be GBs)
        k = keys.shape[0]
        chunk = 1 << 17
        cuts = list(range(0, k, chunk)) + [k]
        # records of a chunk are scattered in the response buffer: bound by their sizes
        sizes = torch.stack([res.size[cuts[i]:cuts[i + 1]].sum()
                             for i in range(len(cuts) - 1)]).tolist()
        for i in range(len(cuts) - 1):
            a, b = cuts[i], cuts[i + 1]
            self.replica.store(sb.keys[a:b], sb.values, sb.val_off[a:b], sb.vlen[a:b],
                               sb.flags[a:b], sb.expire[a:b], now,
                               bytes_bound=int(sizes[i]) + 48 * (b - a))
        return int((sb.vlen != SKIP_VLEN).sum()), int(sum(sizes))

    def refresh_replica(self, top_k: int, keys: Optional[torch.Tensor] = None,
                        now: Optional[int] = None, budget_bytes: Optional[int] = None,
                        chunk_keys: int = 1 << 16) -> int:
        """Collective. Move the replica tier towards the global top-k keys by request
        frequency (from ``keys`` or the recent GET samples), incrementally: keys that left
        the top-k are deleted from the replica and stop being written through; keys that
        entered it are fetched from their owners, most popular first, until
        ``budget_bytes`` of records have moved (None: all of them) — the rest stay
        un-replicated (served by their owners) and are candidates again at the next
        refresh (fetched ``chunk_keys`` at a time: the budget's granularity). Nothing is
        flushed: the replica keeps serving the keys that stay hot. The hot set changes
        identically on every rank. Returns #objects this call stored."""
        self.sync_sets()
        if self.replica is None:
            return 0
        dev = self.device
        old = self._hot if self._hot is not None else torch.zeros((0, 2), dtype=torch.int64,
                                                                    device=dev)
        ranked, rscore = self._hot_candidates(top_k, keys, old, self._hot_score)  # hottest first
        if ranked.shape[0] == 0 and old.shape[0] == 0:
            return 0
        # newly hot keys (in the top k, not in place yet), most requested first, fetched in
        # chunks under the byte budget
        top = ranked[:top_k]
        added = top[~self._member(top, old)]
        stored = fetched = 0
        took = []
        chunk = max(1, int(chunk_keys))
        for a in range(0, added.shape[0], chunk):
            if budget_bytes is not None and fetched >= budget_bytes:
                break
            part = added[a: a + chunk].contiguous()
            n_st, nb = self._fetch_into_replica(part, now)
            stored += n_st
            fetched += nb
            took.append(part)
        # the new hot set: the top-k of the ranking among the keys that are in place (old
        # ones and the ones fetched now); an old key leaves only for a fetched hotter one
        avail = torch.cat([old] + took) if took else old
        avail = avail.index_select(0, torch.argsort(avail[:, 0])).contiguous()
        new = ranked[self._member(ranked, avail)][:top_k] if avail.shape[0] else avail
        nsorted = new.index_select(0, torch.argsort(new[:, 0])).contiguous()
        dropped = old[~self._member(old, nsorted)].contiguous()
        if dropped.shape[0]:
            self.replica.remove(dropped, now)             # no longer written through
        if new.shape[0] == 0:
            self._hot = self._hot_score = None
        else:
            self._hot = nsorted
            # the scores of the hot keys, aligned with self._hot (the next refresh decays them)
            by_lo = torch.argsort(ranked[:, 0])
            rlo = ranked[:, 0].index_select(0, by_lo).contiguous()
            at = torch.clamp(torch.searchsorted(rlo, nsorted[:, 0].contiguous()), max=rlo.numel() - 1)
            self._hot_score = rscore.index_select(0, by_lo.index_select(0, at)).contiguous()
        changed = dropped.shape[0] + sum(t.shape[0] for t in took)
        # a large change of the hot set changes the traffic matrix: measure it afresh (the
        # fixed-capacity exchange otherwise adapts within a few steps)
        if changed * 4 > max(old.shape[0], 1):
            self._routed_step.reset_exchange()
        self._stats["replica_refreshes"] += 1
        self._stats["replica_added"] = self._stats.get("replica_added", 0) + sum(
            t.shape[0] for t in took)
        self._stats["replica_dropped"] = self._stats.get("replica_dropped", 0) + int(dropped.shape[0])
        self._stats["replica_fetched_bytes"] = self._stats.get("replica_fetched_bytes", 0) + fetched
        return stored

    # ------------------------------------------------------------------------------
    # membership changes: rebalancing, failure, warm recovery, snapshots
    # ------------------------------------------------------------------------------
    def set_ring(self, ring: ShardRing, migrate: bool = True, now: Optional[int] = None,
                 chunk_keys: int = 1 << 18, incremental: bool = False) -> int:
        """Collective. Switch every rank to ``ring``. With ``migrate`` each rank ships
        the live objects it holds that the new ring assigns elsewhere to their new
        owners through the routed SET path (warm rebalancing: no refetch from the
        origin), ``chunk_keys`` objects at a time (bounded memory). ``incremental``: only
        switch the ring and queue the migration; ``migrate_step`` then moves it a byte
        budget at a time between serving steps (meanwhile a moved key's GET misses at its
        new owner until its object arrives — a cache miss, never a wrong answer). Returns
        the number of objects this rank has to migrate."""
        self.sync_sets()
        mkeys = None
        if migrate and self.world > 1:
            keys = self.shard.export_keys(now)
            pts, own = ring.tensors(self.device)
            dest, _ = R.route(keys, pts, own, self.world)
            mkeys = keys[dest != self.rank].contiguous()
        self.ring = ring
        self.ring_pts, self.ring_own = ring.tensors(self.device)
        self._routed_step.reset_exchange()
        self._migrating = mkeys
        self._migrate_chunk = chunk_keys
        # until the migration is done, every key a SET or DELETE names (on any rank, through
        # any path) is remembered: its migrated copy is older than what the new owner got
        self._touched = [] if migrate and self.world > 1 else None
        self._touched_all = None
        moved = int(mkeys.shape[0]) if mkeys is not None else 0
        if migrate and self.world > 1 and not incremental:
            while self.migrate_step(None, now):
                pass
        return moved

    def _touch(self, keys: torch.Tensor) -> None:
        """During an incremental migration: remember keys a SET / DELETE names."""
        t = self._touched
        if t is not None and keys.shape[0]:
            t.append(keys.to(self.device).contiguous().clone())

    def _gather_touched(self) -> None:
        """Collective: merge every rank's keys SET or DELETEd since the ring switch into
        ``_touched_all`` (sorted by lo, the same on every rank), and drop them from this
        rank's migration queue (their old copies here are stale: the new owner has a newer
        value, or the key is gone)."""
        dev = self.device
        mine = (torch.cat(self._touched) if self._touched else
                torch.zeros((0, 2), dtype=torch.int64, device=dev))
        self._touched = []
        cnt = torch.tensor([mine.shape[0]], dtype=torch.int64, device=dev)
        all_reduce(cnt, op=dist.ReduceOp.MAX, group=self.group)
        m = int(cnt)
        if m == 0:
            return
        pad = torch.zeros((m, 2), dtype=torch.int64, device=dev)
        pad[: mine.shape[0]] = mine
        parts = [torch.empty_like(pad) for _ in range(self.world)]
        all_gather(parts, pad, group=self.group)
        allk = torch.cat(parts + ([self._touched_all] if self._touched_all is not None else []))
        allk = allk[(allk != 0).any(dim=1)]
        ulo, inv = torch.unique(allk[:, 0].contiguous(), return_inverse=True)
        u = torch.empty((ulo.numel(), 2), dtype=torch.int64, device=dev)
        u[inv] = allk
        self._touched_all = u  # torch.unique sorts by lo
        q = self._migrating
        if q is not None and q.shape[0]:
            stale = self._member(q, u)
            if bool(stale.any()):
                self.shard.remove(q[stale].contiguous(), None)
                q = q[~stale].contiguous()
                self._migrating = q if q.shape[0] else None

    def migrate_step(self, budget_bytes: Optional[int] = None, now: Optional[int] = None) -> bool:
        """Collective. Move queued migration objects (``set_ring``) to their new owners:
        chunks of ``chunk_keys`` until ``budget_bytes`` of records have moved on this rank
        (None: one chunk). Returns whether any rank has objects left (the same on every
        rank). A key SET or DELETEd anywhere since the ring switch is not migrated (its
        copy here is older than what its new owner holds, or it was deleted), and a
        delivered object is stored only where the new owner holds nothing of the key."""
        self.sync_sets()
        moved_bytes = 0
        while True:
            if self._touched is not None:
                self._gather_touched()
            q = self._migrating
            left = torch.tensor([0 if q is None else int(q.shape[0])], dtype=torch.int64,
                                device=self.device)
            all_reduce(left, op=dist.ReduceOp.MAX, group=self.group)
            if int(left) == 0:
                self._migrating = self._touched = self._touched_all = None
                return False
            part = (q[: self._migrate_chunk] if q is not None
                    else torch.zeros((0, 2), dtype=torch.int64, device=self.device)).contiguous()
            if part.shape[0]:
                lk = self.shard.lookup(part, now)
                data = self.shard.gather(lk)
                n = part.shape[0]
                batch = records_to_set_batch(part, GetResult(data, lk.off[:n], lk.size[:n]))
                moved_bytes += int(lk.off[n])
            else:
                empty = torch.zeros(0, dtype=torch.int64, device=self.device)
                batch = SetBatch(part, torch.zeros(16, dtype=torch.uint8, device=self.device),
                                 empty, empty.to(torch.int32))
            # lands on the new owners (collective), where they hold nothing of the key yet
            self.set(batch, now, if_absent=True)
            if part.shape[0]:
                self.shard.remove(part, now)      # this rank no longer owns them
                self._migrating = q[part.shape[0]:] if q.shape[0] > part.shape[0] else None
            # stop once any rank has used its budget (the decision is collective)
            q = self._migrating
            st = torch.tensor([0 if q is None else int(q.shape[0]),
                               int(budget_bytes is None or moved_bytes >= budget_bytes)],
                              dtype=torch.int64, device=self.device)
            all_reduce(st, op=dist.ReduceOp.MAX, group=self.group)
            if int(st[0]) == 0:
                self._migrating = self._touched = self._touched_all = None
                return False
            if int(st[1]):
                return True

    def fail_shard(self, rank: int) -> None:
        """Collective. Simulate (or react to) the loss of ``rank``'s shard: every rank
        drops it from the ring (its keys remap, like ketama auto-eject) and the lost
        shard's contents are discarded."""
        self.sync_sets()
        if rank not in self.ring.shards:
            return
        self.set_ring(self.ring.without(rank), migrate=False)
        if self.rank == rank:
            self.shard.flush()
        if self.replica is not None:
            self.replica.flush()
            self._hot = self._hot_score = None
            self._routed_step.reset_exchange()

    def restore_shard(self, rank: int, now: Optional[int] = None) -> int:
        """Collective. Re-admit ``rank``; objects written while it was out migrate
        back to it from their interim owners (warm restore from peer shards)."""
        shards = sorted(set(self.ring.shards) | {rank})
        return self.set_ring(ShardRing(shards, self.ring.points_per_shard), migrate=True, now=now)

    def save(self, directory: str) -> str:
        """Snapshot this rank's shard to ``directory/shard-<rank>.snap``."""
        os.makedirs(directory, exist_ok=True)
        path = os.path.join(directory, f"shard-{self.rank}.snap")
        self.sync_sets()
        self.shard.save(path)
        return path

    def load(self, directory: str) -> None:
        self.sync_sets()
        self.shard.load(os.path.join(directory, f"shard-{self.rank}.snap"))

    def counters(self) -> dict:
        self.sync_sets()
        return allreduce_stats(self.shard.counters(), self.device, self.group)
