"""LocalStep: the one-GPU pipelined serving step of ``ShardedCache`` (what the headline
benchmark times): a GET batch and a SET batch per step, the SET chain on a stream of its
own beside the GET path, the gather queued before the host knows its size. The step's
streams, events and buffers live here; its knobs are plain attributes of the owning
``ShardedCache``, read at call time (callers set them between steps).
"""
from __future__ import annotations

from typing import Optional

import torch

from ..ops.cache import StreamEvent, expand
from .._native import core as _core
from .batch import GetResult, SetBatch


def new_event(o, name: str):
    """A cross-stream event of ``o``'s serving steps: torch's (a system-scope release at
    every record) with ``event_fence == "system"``, else a StreamEvent of that fence scope,
    or of ``stop_fence`` if a kernel completes it as its stop event (``end``, ``probe``)."""
    if o.event_fence == "system":
        return torch.cuda.Event()
    stopped = o.stop_events and name in ("end", "probe")
    return StreamEvent(o.stop_fence if stopped else o.event_fence)


def stream_wait(stream, ev) -> None:
    """``stream`` waits for a recorded event (a StreamEvent or a torch.cuda.Event)."""
    if isinstance(ev, StreamEvent):
        ev.wait(stream)
    else:
        stream.wait_event(ev)


class _HostCopy:
    """A response still being copied to host memory (host edge): wait() blocks the host
    until the copy is done."""

    def __init__(self, event):
        self.event = event

    def wait(self):
        self.event.synchronize()


class LocalStep:
    def __init__(self, owner):
        self.o = owner               # the ShardedCache: shard, device, knobs, counters
        # streams (created on first use: a CPU shard never has any)
        self._side = None            # the SET chain's
        self._hand_s = None          # the early CLOCK hand's
        self._copy_stream = None     # host edge: the DMA copy of a response
        # events, cached by name: created with the fence knobs as of their first use
        self._events = {}
        self._ends = [None, None]    # per step parity: recorded after the step's SET chain
        self._last_end = None
        self._nserve = -1            # steps issued so far - 1: the step's event parity
        self._side_pending = False   # the last step's SET chain is not joined yet
        self._planned = False        # the serve pipeline orders the next hand (see serve)
        self._held_steps = []        # the SET batches the last two steps' chains may still read
        self._probe_stopped = False  # the last step lookup completed its `probe` itself
        # buffers
        self._co_table = None        # persistent GET-coalescing table
        self._gather_cap = 0         # response buffer bytes for the unsynced gather
        self._dma = [None, None]     # host edge, per turn: (staging buffer, copy-done event)
        self._last_pending = None    # host edge: the copy the next GetResult waits for
        self._host_out = [None, None]  # host edge: pinned response buffers, taken in turn
        self._host_turn = 1
        self._stage_bufs = [{}, {}]  # host edge: HBM copies of the request batches, per turn
        self._stage_turn = 1

    # ------------------------------------------------------------------------------
    def get(self, keys: torch.Tensor, now: Optional[int]) -> GetResult:
        sh, n = self.o.shard, keys.shape[0]
        if self.o.coalesce:
            lk, first, _ = sh.lookup_coalesced(keys, now)
        else:
            lk, first = sh.lookup(keys, now), None
        data = sh.gather(lk)
        expand(first, lk.size, lk.off)
        return GetResult(data, lk.off[:n], lk.size[:n])

    def join(self) -> None:
        """Order the current stream after the last step's SET chain (serve leaves it for
        the next step)."""
        if self._side_pending:
            stream_wait(torch.cuda.current_stream(self.o.device), self._last_end)
            self._side_pending = False
        self._held_steps = []
        # whatever runs next on the caller's stream (a set, a delete, ...) is not covered by
        # the last serve's plan event: the next early hand follows the caller's stream
        self._planned = False

    def serve(self, keys: torch.Tensor, batch: SetBatch, now, inputs_ready) -> GetResult:
        """One step, GETs ordered before SETs. The GET's extent read (the only host sync)
        is hidden behind the SET kernels: the lookup reserves the SET's log bytes (objects
        the SET may overwrite count as misses) and its kernel writes the total into a
        pinned host slot; the SET is queued, and only then does the host spin on that slot
        to size the gather (no event, no copy)."""
        o = self.o
        sh, n = o.shard, keys.shape[0]
        bound = sh.set_bound(batch.keys.shape[0], batch.values.numel())
        if not sh.is_gpu:
            lk = sh.lookup(keys, now, reserve_bytes=bound)
            sh.store(batch.keys, batch.values, batch.val_off, batch.vlen, batch.flags,
                     batch.expire, now)
            data = sh.gather(lk)
            return GetResult(data, lk.off[:n], lk.size[:n])
        side = self._side_stream() if o.overlap_store else None
        turn = None
        if o.host_edge and o.host_edge_dma and keys.device.type == "cpu":
            # host edge: the GET digests into HBM by DMA on this stream (the lookup reads
            # them from HBM instead of across PCIe); the SET batch likewise on the stream
            # that first reads it (_staged_batch)
            turn = self._stage_turn = 1 - self._stage_turn
            keys = self._staged(turn, "keys", keys)
        if side is not None:
            return self._serve_overlapped(keys, batch, now, inputs_ready, bound, side, turn)
        lk, first, cslot, _ = self._lookup_step(keys, now, bound, None)
        sh.store(batch.keys, batch.values, batch.val_off, batch.vlen, batch.flags,
                 batch.expire, now)
        data = self._gather_unsynced(lk)
        expand(first, lk.size, lk.off)
        return GetResult(data, lk.off[:n], lk.size[:n], self._take_pending())

    def _serve_overlapped(self, keys, batch, now, inputs_ready, bound, side, turn) -> GetResult:
        # The SET chain runs beside the GET path. Streams: the caller's (main: lookup,
        # gather), the SET stream (side: dedupe, sizing, log append, index insert) and, with
        # hand="early", a hand stream (the CLOCK hand of a full cache). Ordering:
        #  * everything that reads the request batches waits for `ready` (inputs_ready, or
        #    the caller's stream as of this call);
        #  * the lookup waits for the previous step's SET chain (a step's GETs see the
        #    previous step's SETs, never this step's);
        #  * the log append waits for the previous step's gather (it overwrites the oldest
        #    region, which that gather may still read; the lookup reserved the SET's bytes,
        #    so this step's gather never reads them); the index insert waits for the lookup;
        #  * the early hand waits for the previous step's SET planning only (it reads the
        #    hand position, the claimed head and the ring the planning leaves) and runs beside
        #    that step's append, index insert and gather; its reinsertions are moves, so a
        #    SET that lands after it read the index makes them no-ops, never stale values.
        o = self.o
        sh, n = o.shard, keys.shape[0]
        main = torch.cuda.current_stream(o.device)
        now = sh.now() if now is None else now
        if inputs_ready is None:
            ready = self._event("inputs")
            ready.record(main)
        else:
            ready = inputs_ready
        early = o.hand == "early"
        k = self._nserve = self._nserve + 1   # this step's event parity
        planned = self._event("planned") if early else None
        # ---- early hand and planning
        if early:
            # the hand and the planning of this batch, on the hand stream: after the
            # previous batch's planning (the stream's order) and the chain of the batch
            # before that (its SET workspace and hand buffer, which this batch reuses)
            hs = self._hand_stream()
            stream_wait(hs, ready)
            if self._planned:
                if self._ends[k % 2] is not None:
                    stream_wait(hs, self._ends[k % 2])
            else:
                # no serve pipeline to follow (first step, or other work since): the
                # caller's stream as of now, which has joined every earlier SET chain
                e = self._event("mainpos")
                e.record(main)
                stream_wait(hs, e)
            with torch.cuda.stream(hs):
                batch = self._staged_batch(turn, batch)
                sh.store(batch.keys, batch.values, batch.val_off, batch.vlen, batch.flags,
                         batch.expire, now, phase=1, plan_done=planned)
        # ---- lookup
        stop = o.stop_events and o.event_fence != "system"
        if self._side_pending:
            stream_wait(main, self._ends[(k - 1) % 2])   # the previous step's SET chain
            self._side_pending = False
        if stop and inputs_ready is None:
            # the append follows the previous step's gather (and everything else queued on
            # main before this call: `ready` marks it); the previous chain precedes it on
            # the side stream itself
            start = ready
        else:
            start = self._event("start")
            start.record(main)               # ... and its gather: the append may overwrite
        ev = self._event("probe")
        try:
            lk, first, cslot, table = self._lookup_step(keys, now, bound, side,
                                                        ev if stop else None)
        except BaseException:
            if early:
                # the planned batch still runs its chain (the native store pairs phase 1
                # with the next phase 2), after the previous gather like any append
                with torch.cuda.stream(side):
                    stream_wait(side, planned)
                    sh.store(batch.keys, batch.values, batch.val_off, batch.vlen, batch.flags,
                             batch.expire, now, append_after=start, phase=2)
                self._end_step(side, k, batch, early)
            raise
        # Safe by construction: the lookup reserved the SET's log bytes, so the gather
        # never reads a region the SET writes, and the gather does not read the index.
        if first is not None:
            out_size = torch.empty(n, dtype=torch.int64, device=o.device)
            out_off = torch.empty(n, dtype=torch.int64, device=o.device)
        if not (stop and self._probe_stopped):
            ev.record(main)
        # ---- SET chain
        appended = self._event("appended") if o.gather_after_append else None
        with torch.cuda.stream(side):
            if early:
                stream_wait(side, planned)    # (the plan followed `ready`)
            else:
                stream_wait(side, ready)
                batch = self._staged_batch(turn, batch)
            end = self._end_event(k) if stop else None
            sh.store(batch.keys, batch.values, batch.val_off, batch.vlen, batch.flags,
                     batch.expire, now, index_after=ev, append_after=start, append_done=appended,
                     phase=2 if early else 0, done=end)
        self._end_step(side, k, batch, early, recorded=end is not None)
        # ---- gather
        if appended is not None:
            # the gather runs after the log append, not beside it: the two byte movers
            # contending for HBM are slower together than one after the other
            stream_wait(main, appended)
        # per-request (size, off) and the table clean-up: the gather's workgroups do them
        # after their copies (no launch, and nothing on the side stream for the next
        # step's lookup to wait for but the SET chain)
        data = self._gather_unsynced(
            lk, None if first is None else (first, out_size, out_off, table, cslot))
        if first is not None:
            return GetResult(data, out_off, out_size, self._take_pending())
        return GetResult(data, lk.off[:n], lk.size[:n], self._take_pending())

    def _end_step(self, side, k: int, batch, early: bool, recorded: bool = False) -> None:
        """After a step's SET chain is queued: its end event (the next step's lookup and the
        step after next's hand wait for it; ``recorded``: the chain's last kernel already
        completes it), the batch kept alive until the chain is joined (the next serve's
        lookup or join)."""
        e = self._end_event(k)
        if not recorded:
            e.record(side)
        self._last_end = e
        self._side_pending = True
        held = self._held_steps
        held.append(batch)
        while len(held) > 2:   # the chain of two steps back is joined by now
            held.pop(0)
        self._planned = early

    def _lookup_step(self, keys, now, bound, side, index_done=None):
        """The step's GET lookup (coalesced unless ``coalesce`` is off): (lookup, first,
        cslot, table). ``index_done`` (a StreamEvent): completed by the lookup's probe
        kernel when the coalescing lookup runs (``_probe_stopped`` says whether it did)."""
        sh = self.o.shard
        self._probe_stopped = False
        if self.o.coalesce:
            table = self._coalesce_table(keys.shape[0]) if side is not None else None
            # with the table (the step's path, whose gather carries the expand tail): block-
            # local offsets, no n-row offsets scan between the lookup and the gather
            lk, first, cslot = sh.lookup_coalesced(keys, now, reserve_bytes=bound, total_slot=0,
                                                   table=table, blocked=table is not None,
                                                   index_done=index_done)
            self._probe_stopped = index_done is not None and sh.is_gpu and keys.shape[0] > 0
            return lk, first, cslot, table
        return sh.lookup(keys, now, reserve_bytes=bound, total_slot=0), None, None, None

    # ---- streams and events ------------------------------------------------------
    def _step_stream(self, i: int):
        """Stream ``i`` of the executor's per-device pool, a hardware queue of its own
        (reserve_step_streams)."""
        dev = self.o.device
        return torch.cuda.ExternalStream(int(_core().step_streams(dev.index)[i]), device=dev)

    def _side_stream(self):
        """The step's SET stream (the executor's): nothing queues behind the caller's
        gather. None for a CPU shard."""
        if self._side is None and self.o.device.type == "cuda":
            # (a high-priority side stream measured the same: 0.3156 vs 0.3161 ms/step)
            self._side = self._step_stream(1)
        return self._side

    def _hand_stream(self):
        """The early CLOCK hand's stream: the executor's plan stream, unused by the one-GPU
        step otherwise."""
        if self._hand_s is None:
            self._hand_s = self._step_stream(0)
        return self._hand_s

    def _event(self, name: str):
        e = self._events.get(name)
        if e is None:
            e = self._events[name] = new_event(self.o, name)
        return e

    def _end_event(self, k: int):
        """The end event of step parity ``k % 2`` (created on first use)."""
        e = self._ends[k % 2]
        if e is None:
            e = self._ends[k % 2] = new_event(self.o, "end")
        return e

    # ---- buffers -----------------------------------------------------------------
    def _coalesce_table(self, n: int) -> torch.Tensor:
        """Persistent, zeroed GET-coalescing table (every serve step leaves it zeroed: the
        gather's expand tail zeroes it whole with streaming stores). Coalescing the next batch
        under this step's gather on a third stream (two tables, ping-pong) was measured
        slower, 0.35 vs 0.30 ms/step: both passes compete for the same memory system."""
        slots = int(_core().coalesce_table_slots(n))
        t = self._co_table
        if t is None or t.numel() < slots:
            t = self._co_table = torch.zeros(slots, dtype=torch.int32, device=self.o.device)
        return t

    def _staged(self, turn: int, name: str, x: Optional[torch.Tensor]):
        """``x`` (pinned host) copied into a persistent HBM buffer of this turn by DMA on the
        current stream (which runs everything that reads the buffer, so the copy of turn t
        two steps later is ordered after those reads)."""
        if x is None:
            return None
        bufs = self._stage_bufs[turn]
        b = bufs.get(name)
        if b is None or b.numel() < x.numel() or b.dtype != x.dtype:
            b = bufs[name] = torch.empty(max(x.numel(), 1), dtype=x.dtype, device=self.o.device)
        d = b[: x.numel()].view(x.shape)
        d.copy_(x, non_blocking=True)
        return d

    def _staged_batch(self, turn: Optional[int], b: SetBatch) -> SetBatch:
        """The SET batch staged into HBM on the current stream (``turn`` None: as it is)."""
        if turn is None:
            return b
        return SetBatch(*(self._staged(turn, f"s{i}", x) for i, x in enumerate(
            (b.keys, b.values, b.val_off, b.vlen, b.flags, b.expire))))

    def _take_pending(self):
        p, self._last_pending = self._last_pending, None
        return p

    def _gather_unsynced(self, lk, expand=None) -> torch.Tensor:
        """Gather a lookup given ``total_slot=0`` without stalling the GPU: the gather
        is queued at once into a buffer sized from earlier steps (the kernel writes
        nothing if the total exceeds it) and the host reads the kernel-written total
        while the gather runs; only an outgrown buffer costs a second gather."""
        o = self.o
        if o.host_edge and o.host_edge_dma and o.device.type == "cuda":
            return self._gather_dma(lk, expand)
        sh = o.shard
        cap = self._gather_cap
        if cap:
            data = self._out_buffer(cap)
            sh.gather(lk, data, out_cap=cap, expand=expand)
        total = sh.host_total(0)
        o.gathered_bytes += total
        if cap and total <= cap:
            return data
        self._gather_cap = max(int(total * 1.25), 1 << 20) // 16 * 16
        # (the expand tail ran with the first gather too: it is idempotent)
        return sh.gather(lk, self._out_buffer(max(total, 16)), expand=expand)

    def _gather_dma(self, lk, expand=None) -> torch.Tensor:
        """Host edge: gather into an HBM staging buffer, then copy [0, total) to the pinned
        host buffer on a copy stream (a DMA engine; the next step's kernels run beside it).
        Two turns: the gather of step k+2 waits for the copy of step k out of its staging
        buffer. The result's ``wait()`` blocks the host until its copy is done."""
        o = self.o
        sh = o.shard
        main = torch.cuda.current_stream(o.device)
        k = self._host_turn = 1 - self._host_turn
        cap = self._gather_cap or (64 << 20)
        stg, done = self._dma[k] if self._dma[k] is not None else (None, None)
        if done is not None:
            main.wait_event(done)  # that turn's copy has read its staging buffer
        if stg is None or stg.numel() < cap:
            stg = torch.empty(cap, dtype=torch.uint8, device=o.device)
        sh.gather(lk, stg, out_cap=cap, expand=expand)
        total = sh.host_total(0)
        o.gathered_bytes += total
        if total > cap:
            self._gather_cap = max(int(total * 1.25), 1 << 20) // 16 * 16
            stg = torch.empty(self._gather_cap, dtype=torch.uint8, device=o.device)
            sh.gather(lk, stg, out_cap=self._gather_cap, expand=expand)
        elif not self._gather_cap:
            self._gather_cap = cap
        n = max(total, 16)
        bufs = self._host_out
        if bufs[k] is None or bufs[k].numel() < n:
            bufs[k] = torch.empty(max(n, self._gather_cap), dtype=torch.uint8, pin_memory=True)
        host = bufs[k][:n]
        if self._copy_stream is None:
            self._copy_stream = torch.cuda.Stream(device=o.device)
        cs = self._copy_stream
        gathered = torch.cuda.Event()
        gathered.record(main)
        cs.wait_event(gathered)
        with torch.cuda.stream(cs):
            host.copy_(stg[:n], non_blocking=True)
        done = torch.cuda.Event()
        done.record(cs)
        self._dma[k] = (stg, done)
        self._last_pending = _HostCopy(done)
        return host

    def _out_buffer(self, nbytes: int) -> torch.Tensor:
        if self.o.host_edge:
            # pinned host memory the gather kernel writes over PCIe; two buffers taken in
            # turn, so a step's response stays valid while the next step runs
            bufs = self._host_out
            k = self._host_turn = 1 - self._host_turn
            if bufs[k] is None or bufs[k].numel() < nbytes:
                bufs[k] = torch.empty(nbytes, dtype=torch.uint8, pin_memory=True)
            return bufs[k][:nbytes]
        return torch.empty(nbytes, dtype=torch.uint8, device=self.o.device)
