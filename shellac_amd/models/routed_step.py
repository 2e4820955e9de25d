"""DeviceRoutedStep: ``ShardedCache``'s device-routed path, where GPU-resident batches
travel between the ranks' shards in all-to-alls. Experimental: no regime has been found
where it beats the host-routed default; it stays because the benchmark's ``--routed``,
``--route device`` and ``--simulate-world`` modes run it (docs/ARCHITECTURE.md, the
paragraph "The device-routed step is experimental").

  GET:  [replica probe] -> route (k_route) -> group by owner (k_scatter,
        k_permute) -> a2a digests -> owner probe + scan (k_probe, hipcub) ->
        a2a sizes -> owner gather (k_segcopy, straight into the a2a send
        buffer) -> a2a values into the caller's response buffer.
  SET:  route (+ fan-out of replicated keys to every rank) -> group -> pack
        payloads (k_segcopy) -> a2a digests, metadata, payloads -> owner store
        (dedupe, scan-allocate, log write, CAS insert) / replica store.

The ring, the group, the replica tier and the hot set belong to the owning
``ShardedCache``, which replaces them (``set_ring``, ``refresh_replica``, ``fail_shard``,
a replica fill that hides the replica): everything here reads them at call time.
"""
from __future__ import annotations

from typing import Optional

import torch
import torch.distributed as dist

from ..ops import routing as R
from ..ops.cache import _event_handle
from ..parallel.exchange import (all_gather, all_gather_rows, all_reduce, all_to_all_rows,
                                 all_to_all_single, exchange_counts, segment_sums, step_comm)
from .._native import core as _core
from .batch import SKIP_VLEN, GetResult, SetBatch
from .local_step import new_event, stream_wait


class _StreamDone:
    """A routed step's reply transfer + assembly, finished on a side stream: wait() makes
    the current stream wait for it (no host synchronisation)."""

    def __init__(self, event):
        self.event = event

    def wait(self):
        torch.cuda.current_stream(self.event.device).wait_event(self.event)
        return True


def _hot_directory(hot: torch.Tensor) -> torch.Tensor:
    """dir[b] = first row of ``hot`` (sorted by signed lo) whose order-preserving unsigned
    image of lo has top-16 bits >= b; b in [0, 65536]. Lets the device membership test
    binary-search ~len(hot)/65536 rows instead of all of them."""
    b = torch.arange(65537, dtype=torch.int64, device=hot.device)
    bounds = (b - 32768) << 48            # signed value whose unsigned image is b << 48
    bounds[-1] = torch.iinfo(torch.int64).max
    d = torch.searchsorted(hot[:, 0].contiguous(), bounds, side="left")
    d[-1] = hot.shape[0]
    return d.contiguous()


class _Phases:
    """Consecutive ROCTX ranges for the phases of one serving step (no-op when
    tracing is off; see shellac_amd.utils.trace)."""

    def __init__(self, prefix: str):
        self.c = _core()
        self.on = self.c.trace_on()
        self.prefix = prefix
        self.open = False

    def next(self, name: str) -> None:
        if not self.on:
            return
        if self.open:
            self.c.trace_pop()
        self.c.trace_push(self.prefix + name)
        self.open = True

    def end(self) -> None:
        if self.on and self.open:
            self.c.trace_pop()
            self.open = False


def _batch_args(b: SetBatch) -> tuple:
    """A SET batch as the native executor's plan / step take it."""
    return (b.keys.data_ptr(), b.vlen.data_ptr(),
            b.flags.data_ptr() if b.flags is not None else 0,
            b.expire.data_ptr() if b.expire is not None else 0,
            b.val_off.data_ptr(), b.values.data_ptr(), b.keys.shape[0])


class DeviceRoutedStep:
    def __init__(self, owner):
        self.o = owner        # the ShardedCache: shards, group, ring, hot set, knobs, counters
        self._engine = None   # the native executor (csrc/router.hip RoutedStep), first fused step
        # the native step's communicator (RCCL / mirror / gloo callbacks); False: none,
        # every step takes the multi-call path (collectives from Python)
        self._ncomm = None
        self._row = self._mat = None  # this rank's statistics row / every rank's
        self._sset = None     # the executor's SET stream
        self._asm = None      # side stream of the routed step's reply assembly
        self._probe_ev = None  # multi-call path: forks the SET stream after the owner probe
        # the routed step's main-shard SET chain is joined by the NEXT step's owner probe
        # (RoutedStep::join_sets), so it runs under that step's planning; its buffers stay
        # referenced until then
        self._held = None
        # buffers the reply all-to-all (on the communicator's own stream) still reads or
        # writes after serve returns: released two steps later, once the current stream
        # has waited for that step's assembly (so the allocator never hands them out while
        # the transfer runs)
        self._inflight = []
        # 65537-entry directory into the hot set, and the hot set it was built for (a
        # refresh installs a new tensor)
        self._hot_dir = self._hot_dir_of = None
        self._calibrations = 0  # steps that took the multi-call path

    # ---- what sync_sets / stats / a changed traffic matrix need ---------------------
    def join(self) -> None:
        """Order the current stream after the SETs of the last native step (whose
        main-shard store may still be running on the executor's SET stream)."""
        e = self._engine
        if e is not None and e.sets_pending:
            e.join_sets(torch.cuda.current_stream(self.o.device).cuda_stream)
            self._held = None
        self.harvest()

    def harvest(self) -> None:
        """The native step's statistics run two steps behind: collect the rest (the host
        waits for the latest step's all-gather, not for the step)."""
        e = self._engine
        if e is not None:
            e.harvest_all()
            self._add_step_stats(e.take_stats())

    def _add_step_stats(self, h) -> None:
        n_local, n_dup, off_rank, over, dropped = h
        st = self.o._stats
        st["remote_gets"] += off_rank
        st["replica_hits"] += n_local - n_dup
        st["coalesced_gets"] += n_dup
        st["slot_overflow_rows"] += over
        st["reply_dropped_rows"] += dropped

    def reset_exchange(self) -> None:
        """The traffic matrix changes (new ring, new hot set): the routed step's next
        serve recalibrates its slot capacities (collective: every rank calls it)."""
        if self._engine is not None:
            self._engine.reset_caps()

    # ---- requester-side pieces get() and _serve_routed share -----------------------
    def _route_gets(self, keys: torch.Tensor, now):
        """Group a GET batch by owner: (the replica tier's lookup or None, rows per
        destination [world + 1], the grouping permutation). Requests the replica holds go
        to the pseudo-rank ``world``: they stay local and sort to the tail."""
        o = self.o
        dest, _ = o._route(keys)
        rl = None
        if o.replica is not None:
            rl = o.replica.lookup(keys, now)           # local copies of hot objects
            local = rl.size[: keys.shape[0]] > 0
            dest = torch.where(local, torch.full_like(dest, o.world), dest)
        counts = torch.bincount(dest.long(), minlength=o.world + 1)
        return rl, counts, R.scatter_positions(dest, counts)

    def _request_extents(self, n, perm, sizes_back, scan, n_remote, local_bytes, rl):
        """Per-request (size, off) in request order. Remote sizes arrive in grouped
        (``perm``) order, ``scan`` is their exclusive scan, the remote records follow
        ``local_bytes`` of replica hits in the response buffer."""
        dev = self.o.device
        if n_remote:
            pos = torch.clamp(perm, max=n_remote - 1)
            rsize = sizes_back.index_select(0, pos)
            roff = scan.index_select(0, pos) + local_bytes
        else:
            rsize = torch.zeros(n, dtype=torch.int64, device=dev)
            roff = torch.zeros(n, dtype=torch.int64, device=dev)
        if rl is None:
            return rsize, roff
        local = rl.size[:n] > 0
        return torch.where(local, rl.size[:n], rsize), torch.where(local, rl.off[:n], roff)

    def _set_rows(self, batch: SetBatch):
        """Routing of a SET batch: (dest int32 [m], keys int64 [m, 2], meta int32 [m, 4],
        val_off [m]). A meta row is [vlen, flags, expire, tier]; hot keys are fanned out to
        every rank (write-through; tier 1 = replica copy); dest == world marks rows that go
        nowhere."""
        o = self.o
        dev, w, n = o.device, o.world, batch.keys.shape[0]
        owner, _ = o._route(batch.keys)
        meta = torch.zeros((n, 4), dtype=torch.int32, device=dev)
        meta[:, 0] = batch.vlen
        if batch.flags is not None:
            meta[:, 1] = batch.flags
        if batch.expire is not None:
            meta[:, 2] = batch.expire
        if o.replica is None or o._hot is None:
            return owner, batch.keys, meta, batch.val_off
        hot = o._is_hot(batch.keys)
        r = torch.arange(w, device=dev, dtype=torch.int32).view(1, w)
        own = owner.view(n, 1)
        valid = (r == own) | hot.view(n, 1)
        dest = torch.where(valid, r.expand(n, w), torch.full((n, w), w, dtype=torch.int32,
                                                             device=dev)).reshape(-1)
        keys = batch.keys.repeat_interleave(w, dim=0)
        meta = meta.repeat_interleave(w, dim=0)
        meta[:, 3] = (r != own).reshape(-1).to(torch.int32)
        return dest, keys, meta, batch.val_off.repeat_interleave(w)

    # ---- get / set / delete ------------------------------------------------------
    def get(self, keys: torch.Tensor, now: Optional[int], probe_keys) -> GetResult:
        o = self.o
        n, w, dev, i64 = keys.shape[0], o.world, o.device, torch.int64
        o._sample(keys)
        rl, counts, perm = self._route_gets(keys, now)
        send_keys = R.permute(keys if probe_keys is None else probe_keys, perm)
        recv_counts = exchange_counts(counts[:w].contiguous(), o.group)
        local_total = rl.off[n:n + 1] if rl is not None else torch.zeros(1, dtype=i64, device=dev)
        host = torch.cat([counts, recv_counts, local_total]).cpu()       # sync 1
        send_rows, n_local = host[:w].tolist(), int(host[w])
        recv_rows = host[w + 1: 2 * w + 1].tolist()
        local_bytes = int(host[2 * w + 1])
        n_remote = n - n_local
        req = all_to_all_rows(send_keys[:n_remote], send_rows, recv_rows, o.group)

        # owner side: probe my shard for everything I received
        lk = o.shard.lookup(req, now)
        m = req.shape[0]
        rc = torch.tensor(recv_rows, dtype=i64, device=dev)
        reply_bytes = segment_sums(lk.off, rc)                   # bytes I send back per source
        got_bytes = exchange_counts(reply_bytes, o.group)        # bytes I receive per owner
        nbytes = torch.cat([reply_bytes, got_bytes]).cpu()       # sync 2
        send_b, recv_b = nbytes[:w].tolist(), nbytes[w:].tolist()
        nsend, nrecv = int(sum(send_b)), int(sum(recv_b))
        reply = torch.empty(max(nsend, 16), dtype=torch.uint8, device=dev)
        o.shard.gather(lk, reply)
        sizes_back = all_to_all_rows(lk.size[:m], recv_rows, send_rows, o.group)
        # response buffer: [local replica hits | remote values]
        data = torch.empty(local_bytes + nrecv + 16, dtype=torch.uint8, device=dev)
        if rl is not None and n_local:
            o.replica.gather(rl, data)
        all_to_all_single(data[local_bytes: local_bytes + nrecv], reply[:nsend],
                          output_split_sizes=recv_b, input_split_sizes=send_b, group=o.group)
        size, off = self._request_extents(n, perm, sizes_back, R.exclusive_scan(sizes_back),
                                          n_remote, local_bytes, rl)
        o._stats["remote_gets"] += n_remote - int(send_rows[o.rank])
        o._stats["replica_hits"] += n_local
        return GetResult(data, off, size)

    def set(self, batch: SetBatch, now: Optional[int], if_absent: bool) -> None:
        o = self.o
        dev, w = o.device, o.world
        dest, keys, meta, val_off = self._set_rows(batch)
        counts = torch.bincount(dest.long(), minlength=w + 1)
        perm = R.scatter_positions(dest, counts)
        send_keys = R.permute(keys, perm)
        send_meta = R.permute(meta, perm)
        nvalid = keys.shape[0] - counts[w:w + 1]
        padded = (send_meta[:, 0].to(torch.int64) + 15) & ~15
        padded = torch.where(torch.arange(keys.shape[0], device=dev) < nvalid, padded,
                             torch.zeros_like(padded))
        dst_off = R.exclusive_scan(padded)
        src_off = R.permute(val_off.view(-1, 1), perm).view(-1)
        seg_bytes = segment_sums(dst_off, counts[:w].contiguous())
        recv_counts = exchange_counts(counts[:w].contiguous(), o.group)
        recv_bytes = exchange_counts(seg_bytes, o.group)
        host = torch.cat([counts[:w], recv_counts, seg_bytes, recv_bytes]).cpu()  # sync 1
        send_rows, recv_rows = host[:w].tolist(), host[w: 2 * w].tolist()
        send_b, recv_b = host[2 * w: 3 * w].tolist(), host[3 * w:].tolist()
        ns = int(sum(send_rows))
        payload = torch.empty(int(sum(send_b)) + 16, dtype=torch.uint8, device=dev)
        R.segcopy(batch.values, src_off[:ns].contiguous(), dst_off[: ns + 1].contiguous(), payload)
        rkeys = all_to_all_rows(send_keys[:ns], send_rows, recv_rows, o.group)
        rmeta = all_to_all_rows(send_meta[:ns], send_rows, recv_rows, o.group)
        rvals = torch.empty(int(sum(recv_b)) + 16, dtype=torch.uint8, device=dev)
        all_to_all_single(rvals[: int(sum(recv_b))], payload[: int(sum(send_b))],
                          output_split_sizes=recv_b, input_split_sizes=send_b, group=o.group)
        rvlen = rmeta[:, 0].contiguous()
        roff = R.exclusive_scan((rvlen.to(torch.int64) + 15) & ~15)[:-1].contiguous()
        tier = rmeta[:, 3]
        skip = torch.full_like(rvlen, SKIP_VLEN)
        main_vlen = torch.where(tier == 0, rvlen, skip)
        if if_absent and rkeys.shape[0]:
            # insert-if-absent (as HbmBackend's warm restore): keys this owner already holds
            # keep their (newer) value
            have = o.shard.lookup(rkeys.contiguous(), now).size[: rkeys.shape[0]] > 0
            main_vlen = torch.where(have, skip, main_vlen)
        o.shard.store(rkeys, rvals, roff, main_vlen.contiguous(),
                      rmeta[:, 1].contiguous(), rmeta[:, 2].contiguous(), now)
        if o.replica is not None and o._hot is not None:  # tier-1 rows only exist then
            o.replica.store(rkeys, rvals, roff, torch.where(tier == 1, rvlen, skip).contiguous(),
                            rmeta[:, 1].contiguous(), rmeta[:, 2].contiguous(), now)

    def delete(self, keys: torch.Tensor, now: Optional[int]) -> torch.Tensor:
        o = self.o
        if o.replica is not None:  # replicas are dropped everywhere (collective)
            cnt = torch.tensor([keys.shape[0]], dtype=torch.int64, device=o.device)
            all_reduce(cnt, op=dist.ReduceOp.MAX, group=o.group)
            pad = torch.zeros((int(cnt), 2), dtype=keys.dtype, device=o.device)
            pad[: keys.shape[0]] = keys
            allk = [torch.empty_like(pad) for _ in range(o.world)]
            all_gather(allk, pad, group=o.group)
            o.replica.remove(torch.cat(allk).contiguous(), now)
        dest, counts = o._route(keys)
        perm = R.scatter_positions(dest, counts)
        send_keys = R.permute(keys, perm)
        recv_counts = exchange_counts(counts, o.group)
        both = torch.cat([counts, recv_counts]).cpu()
        send_rows, recv_rows = both[: o.world].tolist(), both[o.world:].tolist()
        req = all_to_all_rows(send_keys, send_rows, recv_rows, o.group)
        found = o.shard.remove(req, now).to(torch.int32)
        back = all_to_all_rows(found, recv_rows, send_rows, o.group)
        return back.index_select(0, perm).bool()

    # ---- the serving step ----------------------------------------------------------
    def serve(self, keys, batch: SetBatch, now, inputs_ready, probe_keys) -> GetResult:
        """GPU shards run the step through the fused native ops (csrc/router.hip) unless
        the owner's ``fused`` is off; the framework-op version is the CPU path."""
        self.o._sample(keys)
        if self.o.fused and self.o.device.type == "cuda":
            return self._serve_routed_fused(keys, batch, now, inputs_ready, probe_keys)
        return self._serve_routed(keys, batch, now)

    def _serve_routed_fused(self, keys, batch, now, inputs_ready, probe_keys) -> GetResult:
        """``_serve_routed`` run by the native executor (csrc/router.hip, RoutedStep), with
        no host synchronisation between planning and the result (after one calibrating
        step): GET requests and replies travel in fixed-capacity per-peer slots whose
        counts and (size, offset) headers ride in-band, so the all-to-alls need no split
        sizes from the device; capacities every rank agrees on come from the demand the
        ranks all-gathered in earlier steps, and a row that does not fit is a counted
        miss. SETs travel with exact sizes the host reads mid-step, while the GPU is busy
        with the GET exchange queued before. Same results as the framework-op version
        (tests); the reply transfer and the per-request assembly finish on a side stream
        (``GetResult.wait()``), under the next step's planning."""
        c = _core()
        o = self.o
        dev, w, me = o.device, o.world, o.rank
        cur = torch.cuda.current_stream(dev)
        st = cur.cuda_stream
        i64, u8 = torch.int64, torch.uint8
        n = keys.shape[0]
        now = o.shard.now() if now is None else now
        e = self._engine
        if e is None:
            e = self._engine = c.RoutedStep(w, me, dev.index)
            e.single_comm = o.comm_mode == "single"
            k = e.row_words
            self._row = torch.zeros(k, dtype=i64, device=dev)
            self._mat = torch.zeros(w * k, dtype=i64, device=dev)
            # the executor's process-wide streams (plan, SET side, reply + assembly): the
            # multi-call path uses the same ones, so a process keeps to four streams, one
            # hardware queue each (4 per process, taken round robin)
            ss = [int(x) for x in c.step_streams(dev.index)]
            self._sset = torch.cuda.ExternalStream(ss[1], device=dev)
            self._asm = torch.cuda.ExternalStream(ss[2], device=dev)
        e.set_ring(o.ring_pts.data_ptr(), o.ring_own.data_ptr(), o.ring_pts.numel())
        e.set_probe_keys(probe_keys.data_ptr() if probe_keys is not None else 0,
                         batch.probe_keys.data_ptr() if batch.probe_keys is not None else 0)
        hot = o._hot
        fanout = o.replica is not None and hot is not None
        changed = False
        if fanout and self._hot_dir_of is not hot:
            self._hot_dir, self._hot_dir_of = _hot_directory(hot), hot
            changed = True  # a new hot set: the executor rebuilds its hash set
        e.set_hot(hot.data_ptr() if fanout else 0, hot.shape[0] if fanout else 0,
                  self._hot_dir.data_ptr() if fanout else 0, changed)
        rep = o.replica._impl if o.replica is not None else None
        while len(self._inflight) >= 2:
            ev, _bufs = self._inflight.pop(0)
            cur.wait_event(ev)  # long complete: frees the buffers for reuse on this stream
        cap_g, cap_d, cap_l, cal, cal_l = e.prepare(n)
        if self._ncomm is None:
            self._ncomm = step_comm(o.group, dev) or False
            if self._ncomm is not False:
                e.set_comm(self._ncomm)
        # the path must be the same on every rank: `cal` is (every rank derives it from the
        # same all-gathered rows), `cal_l` is per rank (its own local-region history)
        if self._ncomm is not False and not cal:
            return self._serve_native(e, keys, batch, now, n, cap_g, cap_d, cap_l, fanout, rep,
                                      inputs_ready)
        self._calibrations += 1  # (the multi-call path)
        ph = _Phases("serve.")
        ph.next("plan")
        # G = [recv: w-1 slots | self slot | send: w-1 slots] of cap_g digests
        gslot = 16 * cap_g
        G = torch.empty((2 * w - 1) * gslot, dtype=u8, device=dev)
        e.plan(keys.data_ptr(), n, rep, now, *_batch_args(batch), fanout,
               G.data_ptr(), self._row.data_ptr(), st, o.coalesce)
        ph.next("row_allgather")
        all_gather_rows(self._mat, self._row, o.group, peer_blocks=4)
        e.publish(self._mat.data_ptr(), st)
        if cal_l:
            e.calibrate_local()                                   # calibration: host read
        ph.next("request_a2a")
        if w > 1:
            sp = [0 if p == me else gslot for p in range(w)]
            all_to_all_single(G[: (w - 1) * gslot], G[w * gslot:], output_split_sizes=sp,
                              input_split_sizes=sp, group=o.group)
        ph.next("owner")
        e.owner_probe(G.data_ptr(), o.shard._impl, now, st)
        # the SET stream forks here: the probe reserved this step's SET bytes, so the SET
        # exchange and the main-shard SET chain run beside the reply gather
        sset = self._sset
        if self._probe_ev is None:
            self._probe_ev = new_event(o, "routed_probe")
        self._probe_ev.record(cur)
        stream_wait(sset, self._probe_ev)
        if cal:
            dem = torch.empty(w, dtype=i64, device=dev)
            e.owner_demand(dem.data_ptr(), st)
            dmat = torch.empty(w * w, dtype=i64, device=dev)
            all_gather_rows(dmat, dem, o.group, peer_blocks=1)
            e.calibrate_reply(dmat.data_ptr())                    # calibration: host read
        if cal or cal_l:
            cap_g, cap_d, cap_l = e.caps(n)[:3]
        slot_r = 8 * cap_g + cap_d
        # the response buffer: [local capL | w-1 reply slots (recv) | self reply slot]
        Rb = torch.empty(max((w - 1) * slot_r, 16), dtype=u8, device=dev)
        data = torch.empty(cap_l + w * slot_r + 16, dtype=u8, device=dev)
        e.owner_reply(o.shard._impl, Rb.data_ptr(), data.data_ptr(), st)
        work = None
        if w > 1:
            sp = [0 if p == me else slot_r for p in range(w)]
            work = all_to_all_single(data[cap_l: cap_l + (w - 1) * slot_r], Rb[: (w - 1) * slot_r],
                                     output_split_sizes=sp, input_split_sizes=sp,
                                     group=o.data_group, async_op=True)
        e.gather_local(data.data_ptr(), st)
        local_done = torch.cuda.Event()
        local_done.record(cur)
        ph.next("set_exchange")
        h = e.set_splits()           # waits for the published rows: the GPU is still busy
        send, recv = h[:w], h[w:2 * w]
        so, ro = sum(send) - send[me], sum(recv) - recv[me]
        # S: the other ranks' blocks only (own SETs are stored from the batch in place)
        S = torch.empty(so + 16, dtype=u8, device=dev)
        Rs = torch.empty(ro + 16, dtype=u8, device=dev)
        e.pack_sets(S.data_ptr(), sset.cuda_stream)
        if w > 1:
            with torch.cuda.stream(sset):
                all_to_all_single(Rs[:ro], S[:so],
                                  output_split_sizes=[0 if q == me else recv[q] for q in range(w)],
                                  input_split_sizes=[0 if p == me else send[p] for p in range(w)],
                                  group=o.group)
        e.store_sets(Rs.data_ptr(), o.shard._impl, rep, now, st, sset.cuda_stream)
        # the main-shard SET chain reads S / Rs and the batch until the next step's owner
        # probe joins it
        self._held = (S, Rs, batch) if e.sets_pending else None
        ph.next("assemble")
        out = torch.empty((2, n), dtype=i64, device=dev)
        side = self._asm
        side.wait_event(local_done)
        with torch.cuda.stream(side):
            if work is not None:
                work.wait()          # the side stream waits for the reply all-to-all
            e.assemble(data.data_ptr(), out[0].data_ptr(), out[1].data_ptr(), side.cuda_stream)
        self._add_step_stats(h[2 * w: 2 * w + 5])
        self._add_step_stats(e.take_stats())  # earlier native steps' (lagged)
        ph.end()
        return self._result(data, out, (Rb, data))

    def _result(self, data, out, bufs) -> GetResult:
        """A native step's result, pending on the reply transfer and the assembly, which
        run on the executor's assembly stream (one per device for the process, never
        destroyed, so tensors recorded on it are safe)."""
        side = self._asm
        data.record_stream(side)
        out.record_stream(side)
        done = torch.cuda.Event()
        done.record(side)
        self._inflight.append((done, bufs))
        return GetResult(data, out[1], out[0], _pending=_StreamDone(done))

    def _serve_native(self, e, keys, batch, now, n, cap_g, cap_d, cap_l, fanout, rep, inputs_ready):
        """The routed step as one native call (``RoutedStep.step``): every kernel launch
        and collective of the step is issued from C++, none from Python; only the response
        buffers are torch tensors (the caller keeps them). Calibrating steps take the
        multi-call path in ``_serve_routed_fused``."""
        o = self.o
        dev, w = o.device, o.world
        cur = torch.cuda.current_stream(dev)
        slot_r = 8 * cap_g + cap_d
        data = torch.empty(cap_l + w * slot_r + 16, dtype=torch.uint8, device=dev)
        out = torch.empty((2, n), dtype=torch.int64, device=dev)
        h = e.step(keys.data_ptr(), n, rep, now, *_batch_args(batch), fanout,
                   o.coalesce, o.shard._impl, data.data_ptr(), out[0].data_ptr(),
                   out[1].data_ptr(), cur.cuda_stream, 0, 0,
                   _event_handle(inputs_ready), batch.values.numel())
        # the main-shard SET chain (the executor's SET stream, a hardware queue of its own)
        # reads the batch until the next step's probe joins it
        self._held = (batch,) if e.sets_pending else None
        # statistics of the steps two back (the host never waits for this step's matrix)
        self._add_step_stats(h)
        # (the local gather, on the SET stream, writes `data` too: the assembly awaits it)
        return self._result(data, out, (data,))

    def _serve_routed(self, keys, batch, now) -> GetResult:
        """GET + SET step over all ranks with one request exchange and one reply exchange:
        4-5 collectives and 2 host syncs for the whole step instead of 10 and 3 for get()
        followed by set().

          1. route GETs (replica hits stay local) and SETs on the device; ONE tiny
             all-to-all of per-peer [get rows, set rows, set value bytes]; host sync 1.
          2. ONE all-to-all carries, per peer, [GET digests | SET records | SET values],
             assembled by a single gather_segments launch from three tensors. A SET record
             is [digest lo, digest hi, vlen | flags << 32, expire | tier << 32].
          3. owner: de-interleave, lookup; all-to-all of reply sizes; host sync 2.
          4. owner gathers replies straight into the send buffer; the value all-to-all
             runs asynchronously while the SET stores and the local replica gather run
             on the compute stream (GETs of this step see the state before its SETs).
        """
        o = self.o
        dev, w, me = o.device, o.world, o.rank
        n = keys.shape[0]
        i64 = torch.int64
        ph = _Phases("serve.")
        # ---- 1. routing + count exchange
        ph.next("route")
        rl, cnt_g, perm_g = self._route_gets(keys, now)
        gk = R.permute(keys, perm_g)
        dest_s, skeys, smeta, val_off = self._set_rows(batch)
        rec = torch.cat([skeys, smeta.view(i64)], dim=1)
        m = rec.shape[0]
        cnt_s = torch.bincount(dest_s.long(), minlength=w + 1)
        perm_s = R.scatter_positions(dest_s, cnt_s)
        srec = R.permute(rec, perm_s)
        sval = R.permute(val_off.view(-1, 1), perm_s).view(-1)
        vlen = srec[:, 2] & 0xFFFFFFFF
        vlen = torch.where(vlen >= 0x80000000, torch.zeros_like(vlen), vlen)  # skip rows: no bytes
        padded = torch.where(torch.arange(m, device=dev) < m - cnt_s[w], (vlen + 15) & ~15,
                             torch.zeros_like(vlen))
        vscan = R.exclusive_scan(padded)
        vb = segment_sums(vscan, cnt_s[:w].contiguous())
        table = torch.stack([cnt_g[:w], cnt_s[:w], vb], dim=1).contiguous()
        ph.next("count_exchange")
        rtable = torch.empty_like(table)
        all_to_all_single(rtable, table, group=o.group)
        ltot = rl.off[n:n + 1] if rl is not None else torch.zeros(1, dtype=i64, device=dev)
        host = torch.cat([table.view(-1), rtable.view(-1), cnt_g[w:w + 1], ltot]).cpu()  # sync 1
        t = host[: 3 * w].view(w, 3).tolist()
        rt = host[3 * w: 6 * w].view(w, 3).tolist()
        n_local, local_bytes = int(host[6 * w]), int(host[6 * w + 1])
        g_rows, s_rows = [r[0] for r in t], [r[1] for r in t]
        rg_rows, rs_rows = [r[0] for r in rt], [r[1] for r in rt]
        send_b = [16 * a + 32 * b + c for a, b, c in t]
        recv_b = [16 * a + 32 * b + c for a, b, c in rt]
        ns = sum(s_rows)

        # ---- 2. request exchange: per peer [G | R | V]
        ph.next("pack_requests")
        g_start = [sum(g_rows[:p]) for p in range(w)]
        s_start = [sum(s_rows[:p]) for p in range(w)]
        nseg = 2 * w + ns
        seg_len = torch.empty(nseg, dtype=i64, device=dev)
        seg_src = torch.empty(nseg, dtype=i64, device=dev)
        hdr_idx, hdr_len, hdr_src = [], [], []
        for p in range(w):
            hdr_idx += [2 * p + s_start[p], 2 * p + 1 + s_start[p]]
            hdr_len += [16 * g_rows[p], 32 * s_rows[p]]
            hdr_src += [gk.data_ptr() + 16 * g_start[p], srec.data_ptr() + 32 * s_start[p]]
        hdr = torch.tensor([hdr_idx, hdr_len, hdr_src], dtype=i64).to(dev, non_blocking=True)
        seg_len.index_copy_(0, hdr[0], hdr[1])
        seg_src.index_copy_(0, hdr[0], hdr[2])
        if ns:
            peer = torch.repeat_interleave(torch.arange(w, device=dev), cnt_s[:w],
                                           output_size=ns)
            vidx = torch.arange(ns, device=dev) + 2 * peer + 2
            seg_len.index_copy_(0, vidx, padded[:ns])
            seg_src.index_copy_(0, vidx, sval[:ns] + batch.values.data_ptr())
        send = torch.empty(sum(send_b) + 16, dtype=torch.uint8, device=dev)
        R.gather_segments(seg_src, R.exclusive_scan(seg_len), send)
        recv = torch.empty(sum(recv_b) + 16, dtype=torch.uint8, device=dev)
        ph.next("request_a2a")
        all_to_all_single(recv[: sum(recv_b)], send[: sum(send_b)],
                          output_split_sizes=recv_b, input_split_sizes=send_b, group=o.group)

        # ---- 3. owner: de-interleave digests and records, probe
        ph.next("owner_lookup")
        mg, ms = sum(rg_rows), sum(rs_rows)
        body = torch.empty(16 * mg + 32 * ms + 16, dtype=torch.uint8, device=dev)
        q_start = [sum(recv_b[:q]) for q in range(w)]   # source q's block inside `recv`
        src_l = ([recv.data_ptr() + q_start[q] for q in range(w)] +
                 [recv.data_ptr() + q_start[q] + 16 * rg_rows[q] for q in range(w)])
        len_l = [16 * r for r in rg_rows] + [32 * r for r in rs_rows]
        dl = torch.tensor([src_l, len_l], dtype=i64).to(dev, non_blocking=True)
        R.gather_segments(dl[0].contiguous(), R.exclusive_scan(dl[1]), body)
        req = body[: 16 * mg].view(i64).view(mg, 2)
        rrec = body[16 * mg: 16 * mg + 32 * ms].view(i64).view(ms, 4)
        lk = o.shard.lookup(req, now)
        rcv = torch.tensor(rg_rows, dtype=i64).to(dev, non_blocking=True)
        reply_bytes = segment_sums(lk.off, rcv)
        sizes_back = all_to_all_rows(lk.size[:mg], rg_rows, g_rows, o.group)
        n_remote = n - n_local
        gscan = R.exclusive_scan(sizes_back)
        got_bytes = segment_sums(gscan, torch.tensor(g_rows, dtype=i64).to(dev, non_blocking=True))
        ph.next("reply_sizes")
        nb = torch.cat([reply_bytes, got_bytes]).cpu()                    # sync 2
        rep_b, got_b = nb[:w].tolist(), nb[w:].tolist()

        # ---- 4. replies (async) overlapped with SET stores and the replica gather
        ph.next("reply_a2a+set_store")
        reply = torch.empty(max(sum(rep_b), 16), dtype=torch.uint8, device=dev)
        o.shard.gather(lk, reply)
        data = torch.empty(local_bytes + sum(got_b) + 16, dtype=torch.uint8, device=dev)
        work = all_to_all_single(data[local_bytes: local_bytes + sum(got_b)],
                                 reply[: sum(rep_b)], output_split_sizes=got_b,
                                 input_split_sizes=rep_b, group=o.group, async_op=True)
        if rl is not None and n_local:
            o.replica.gather(rl, data)
        if ms:
            meta = rrec[:, 2:].contiguous().view(torch.int32).view(ms, 4)
            rvlen = meta[:, 0].contiguous()
            tier = meta[:, 3]
            # value offsets inside `recv`: source block start + scan within the block
            vpad = (rvlen.to(i64) + 15) & ~15
            vs = R.exclusive_scan(vpad)
            vstart = [q_start[q] + 16 * rg_rows[q] + 32 * rs_rows[q] for q in range(w)]
            rs_t = torch.tensor(rs_rows, dtype=i64).to(dev, non_blocking=True)
            first = torch.cumsum(rs_t, 0) - rs_t
            delta = torch.tensor(vstart, dtype=i64).to(dev, non_blocking=True) - \
                vs.index_select(0, first)
            roff = (vs[:ms] + torch.repeat_interleave(delta, rs_t, output_size=ms)).contiguous()
            skip = torch.full_like(rvlen, SKIP_VLEN)
            rkeys = rrec[:, :2].contiguous()
            o.shard.store(rkeys, recv, roff, torch.where(tier == 0, rvlen, skip).contiguous(),
                          meta[:, 1].contiguous(), meta[:, 2].contiguous(), now)
            if o.replica is not None:
                o.replica.store(rkeys, recv, roff,
                                torch.where(tier == 1, rvlen, skip).contiguous(),
                                meta[:, 1].contiguous(), meta[:, 2].contiguous(), now)
        work.wait()

        # ---- requester: response offsets in request order
        ph.next("assemble")
        size, off = self._request_extents(n, perm_g, sizes_back, gscan, n_remote, local_bytes, rl)
        o._stats["remote_gets"] += n_remote - int(g_rows[me])
        o._stats["replica_hits"] += n_local
        ph.end()
        return GetResult(data, off, size)
