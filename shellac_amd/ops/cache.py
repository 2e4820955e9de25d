"""Tensor-level batch operations on one cache shard (HBM on a GPU, DRAM on the CPU).

This is the compute path of the cache. A ``CacheShard`` on a ``cuda`` device
drives the hand-written HIP kernels in ``csrc/hbm_cache.hip`` (probe, load-
balanced gather, dedupe + scan-allocated log write, two-choice CAS insert); on
the CPU it drives ``csrc/host_cache.cc``, which implements the same layout and
policies and is the semantic reference the kernels are tested against.

Keys are 128-bit digests stored as ``int64`` tensors of shape ``[n, 2]`` (lo, hi)
(see ``csrc/digest.h``). The reference addresses objects by URL string through
pylibmc (src/python/shellac/server/Server.py:327, :335, :432); digests are what
let the GPU path move fixed 16-byte records.
"""
from __future__ import annotations

import time
from dataclasses import dataclass
from typing import Iterable, Optional, Sequence

import numpy as np
import torch

from .._native import core

ITEM_HEADER_BYTES = 32
ITEM_MAGIC = 0x5348A11C
MISS_LOC = (1 << 64) - 1


def _stream_handle(device: torch.device) -> int:
    return torch.cuda.current_stream(device).cuda_stream


def item_bytes(vlen: int) -> int:
    return ITEM_HEADER_BYTES + ((vlen + 15) & ~15)


# ----------------------------------------------------------------------------------
# digests & packing helpers
# ----------------------------------------------------------------------------------
def pack_bytes(items: Sequence[bytes]) -> tuple[np.ndarray, np.ndarray]:
    """Concatenate byte strings -> (uint8 buffer, int64 offsets[n+1])."""
    offs = np.zeros(len(items) + 1, dtype=np.int64)
    np.cumsum([len(x) for x in items], out=offs[1:])
    buf = np.frombuffer(b"".join(items), dtype=np.uint8) if items else np.zeros(0, np.uint8)
    return buf, offs


def digest_strings(keys: Sequence[bytes], device: str | torch.device = "cpu") -> torch.Tensor:
    """128-bit digests of ``keys`` as an int64 tensor [n, 2] (computed on the host)."""
    c = core()
    buf, offs = pack_bytes(list(keys))
    buf = np.ascontiguousarray(buf)
    if buf.size == 0:
        buf = np.zeros(1, np.uint8)
    out = np.zeros((len(keys), 2), dtype=np.int64)
    c.host_digest_keys(buf.ctypes.data, offs.ctypes.data, len(keys), out.ctypes.data)
    return torch.from_numpy(out).to(device)


def digest_packed(buf: torch.Tensor, offs: torch.Tensor) -> torch.Tensor:
    """Digest packed key bytes on the tensors' device (HIP kernel on GPU)."""
    c = core()
    n = offs.numel() - 1
    out = torch.empty((n, 2), dtype=torch.int64, device=buf.device)
    if buf.is_cuda:
        c.digest_keys(buf.data_ptr(), offs.data_ptr(), n, out.data_ptr(), _stream_handle(buf.device))
    else:
        c.host_digest_keys(buf.data_ptr(), offs.data_ptr(), n, out.data_ptr())
    return out


def pack_values(values: Sequence[bytes], device: str | torch.device = "cpu"):
    """Pack values 16-byte aligned (+16 B readable slack) for ``CacheShard.store``.

    Returns (values uint8 tensor, val_off int64 tensor, vlen int32 tensor).
    """
    n = len(values)
    vlen = np.array([len(v) for v in values], dtype=np.int64)
    padded = (vlen + 15) & ~15
    val_off = np.zeros(n, dtype=np.int64)
    if n:
        np.cumsum(padded[:-1], out=val_off[1:])
    total = int(padded.sum()) + 16
    buf = np.zeros(total, dtype=np.uint8)
    for i, v in enumerate(values):
        buf[val_off[i] : val_off[i] + len(v)] = np.frombuffer(v, dtype=np.uint8)
    return (
        torch.from_numpy(buf).to(device),
        torch.from_numpy(val_off).to(device),
        torch.from_numpy(vlen.astype(np.int32)).to(device),
    )


def keyed(key: bytes, payload: bytes) -> bytes:
    """The *keyed* value ``[u16 key length | key | payload]`` the cache backends store for
    full-key identity (``csrc/keyed.h`` ``write_keyed``): what ``remove_keyed_prefix``
    scans. Store it under ``digest_strings([key])``."""
    return core().keyed(bytes(key), bytes(payload))


MAX_OBJECT_TAGS = 32  # keyed.h kMaxObjectTags
MAX_PURGE_TAGS = 64  # keyed.h kMaxPurgeTags


def tag_hash(tag: bytes) -> int:
    """Hash of one surrogate key (``csrc/keyed.h`` ``tag_hash``): the low word of the tag's
    digest. Tags are case-sensitive byte strings."""
    return int(core().tag_hash(bytes(tag)))


def tagged(tags: Iterable[bytes], payload: bytes) -> bytes:
    """``payload`` behind the tag block ``[0x02 | u8 ntags | ntags x u64 LE hash]`` of its
    distinct ``tags`` (``write_tag_block``); more than 32 distinct tags give the overflow
    block ``[0x02 | 0xff]``, which every tag purge matches. Goes into ``keyed`` as the
    payload."""
    hashes = list(dict.fromkeys(tag_hash(t) for t in tags))
    return core().tag_block(hashes) + bytes(payload)


def split_tagged(value: bytes):
    """``(hashes | "overflow" | None, payload)`` of a payload as stored (``parse_tag_block``):
    ``None`` for an untagged payload and for a malformed or truncated block, which are left
    as they are."""
    value = bytes(value)
    strip, hashes, overflow = core().parse_tag_block(value)
    if not strip:
        return None, value
    return ("overflow" if overflow else [int(h) for h in hashes]), value[strip:]


def unpack_records(out: torch.Tensor, off: torch.Tensor, size: torch.Tensor) -> list:
    """Decode GET output ([ItemHeader | value | pad] per hit) -> list of (value, flags) or None."""
    o = out.cpu().numpy()
    offs = off.cpu().numpy()
    sizes = size.cpu().numpy()
    res = []
    for i in range(len(sizes)):
        if sizes[i] == 0:
            res.append(None)
            continue
        base = int(offs[i])
        hdr = o[base : base + ITEM_HEADER_BYTES].view(np.uint32)
        vl, flags, magic = int(hdr[4]), int(hdr[5]), int(hdr[7])
        if magic != ITEM_MAGIC:
            raise RuntimeError(f"corrupt item header at {base}: magic {magic:#x}")
        res.append((o[base + ITEM_HEADER_BYTES : base + ITEM_HEADER_BYTES + vl].tobytes(), flags))
    return res


SLICE_KINDS = {"head": 0, "range": 1, "from": 2, "suffix": 3, "whole": 4}  # slice.h kSlice*
SLICE_STATUS = ("miss", "ok", "unsat", "whole", "not_modified")  # slice.h kSliceMiss ..
# conditional.h kCond*
COND_KINDS = {"none": 0, "none_match": 1, "modified_since": 2, "if_range_etag": 3,
              "if_range_date": 4}
# u32 words of a SliceRow (slice.h); out_off is the u64 at bytes 48..55
_SLICE_WORDS = ("status", "vlen", "flags", "expire", "head_off", "body_off", "body_len", "skew",
                "win_first", "win_len", "head_bytes")


def pack_slice_specs(specs) -> np.ndarray:
    """Window specs -> uint8 [n, 24] rows of ``{u32 kind, u64 a, u64 b}`` (``SliceSpec``).
    A spec is ``(kind,)``, ``(kind, a)`` or ``(kind, a, b)``, kind a name of ``SLICE_KINDS``
    or its number."""
    arr = np.zeros((len(specs), 3), dtype=np.uint64)
    for i, s in enumerate(specs):
        s = tuple(s) if isinstance(s, (tuple, list)) else (s,)
        kind = SLICE_KINDS[s[0]] if isinstance(s[0], str) else int(s[0])
        arr[i] = (kind, int(s[1]) if len(s) > 1 else 0, int(s[2]) if len(s) > 2 else 0)
    return arr.view(np.uint8).reshape(len(specs), 24)


def pack_slice_conds(conds):
    """Row conditions -> ``(uint8 [n, 16] rows of SliceCond {u32 kind, ncand, off, len}, uint8
    candidate bytes)`` (``csrc/conditional.h``). ``conds[i]`` is ``None``, ``("none_match",
    [tag, ...])`` (entity-tags as the client sent them; a ``W/`` is stripped, which gives the
    weak comparison), ``("none_match", "*")``, ``("modified_since", date)``,
    ``("if_range_etag", tag)`` (a weak tag never matches) or ``("if_range_date", date)``. A
    candidate is sent as one ``[u8 len | bytes]`` record and holds at most 255 bytes; a list at
    most 16 tags."""
    rows = np.zeros((len(conds), 4), dtype=np.uint32)
    blob = bytearray()
    for i, c in enumerate(conds):
        if c is None:
            continue
        kind, arg = c
        kind = COND_KINDS[kind] if isinstance(kind, str) else int(kind)
        if kind == COND_KINDS["none_match"]:
            if isinstance(arg, (bytes, bytearray)):
                arg = [arg]
            cands = [] if isinstance(arg, str) and arg == "*" else \
                [bytes(t)[2:] if bytes(t)[:2] == b"W/" else bytes(t) for t in arg]
            if not isinstance(arg, str) and not cands:
                raise ValueError("none_match needs '*' or at least one entity-tag")
        elif kind == COND_KINDS["if_range_etag"]:
            cands = [] if bytes(arg)[:2] == b"W/" else [bytes(arg)]
        else:
            cands = [bytes(arg)]
        if len(cands) > 16 or any(len(t) > 255 for t in cands):
            raise ValueError("a condition holds at most 16 candidates of at most 255 bytes")
        off = len(blob)
        for t in cands:
            blob += bytes([len(t)]) + t
        rows[i] = (kind, len(cands), off, len(blob) - off)
    return rows.view(np.uint8).reshape(len(conds), 16), np.frombuffer(bytes(blob), dtype=np.uint8)


def slice_rows(rows: torch.Tensor) -> list:
    """Decode ``get_keyed_slices`` result rows -> one dict of the ``SliceRow`` fields per row."""
    r = rows.cpu().numpy()
    r32 = r.view(np.uint32).reshape(-1, 16)
    r64 = r.view(np.uint64).reshape(-1, 8)
    res = []
    for i in range(r32.shape[0]):
        f = {name: int(r32[i, k]) for k, name in enumerate(_SLICE_WORDS)}
        f["out_off"] = int(r64[i, 6])
        res.append(f)
    return res


def unpack_slices(rows: torch.Tensor, out: torch.Tensor) -> list:
    """Decode a sliced GET (``CacheShard.get_slices``' dicts) from its rows and response
    buffer; only a row's meaningful bytes are read, not its granules' padding."""
    o = out.cpu().numpy()
    res = []
    for f in slice_rows(rows):
        st, base = SLICE_STATUS[f["status"]], f["out_off"]
        head = window = b""
        if st == "whole":
            window = o[base:base + f["vlen"]].tobytes()
        elif st != "miss":
            head = o[base + f["head_off"]:base + f["body_off"]].tobytes()
            w0 = base + f["head_bytes"] + f["skew"]
            window = o[w0:w0 + f["win_len"]].tobytes()
        res.append({"status": st, "head": head, "window": window, "body_len": f["body_len"],
                    "first": f["win_first"], "vlen": f["vlen"], "flags": f["flags"],
                    "expire": f["expire"]})
    return res


def coalesce(keys: torch.Tensor, table: Optional[torch.Tensor] = None):
    """GET coalescing (request collapsing inside a batch). Returns ``first`` (int32
    [n]): the row that serves row i — one row per distinct digest claims it with a CAS
    in an open-addressing table (``k_coalesce``), its duplicates point at that row.
    Pass it to ``CacheShard.lookup(first=...)`` (duplicates skip the index probe and
    the gather) and call ``expand(first, lookup)`` after the gather, so every request
    addresses its claimer's record. CPU shards: ``None`` (the host engine probes every
    row; results are the same values).
    ``table`` (a caller-owned, zeroed table, see ``CacheShard.lookup_coalesced``):
    returns ``(first, cslot)`` and ``expand_out(..., table, cslot)`` must clean it."""
    if not keys.is_cuda or keys.shape[0] == 0:
        return None if table is None else (None, None)
    c = core()
    n = keys.shape[0]
    cslot = None
    if table is None:
        slots = int(c.coalesce_table_slots(n))
        table = torch.empty(slots, dtype=torch.int32, device=keys.device)
    else:
        slots = table.numel()
        if slots < int(c.coalesce_table_slots(n)) or slots & (slots - 1):
            raise ValueError("coalescing table too small or not a power of two")
        cslot = torch.empty(n, dtype=torch.int32, device=keys.device)
    first = torch.empty(n, dtype=torch.int32, device=keys.device)
    c.coalesce_keys(keys.data_ptr(), n, table.data_ptr(), slots, first.data_ptr(),
                    _stream_handle(keys.device), cslot.data_ptr() if cslot is not None else 0,
                    cslot is not None)
    return first if cslot is None else (first, cslot)


def expand(first: Optional[torch.Tensor], size: torch.Tensor, off: torch.Tensor) -> None:
    """After the gather of a coalesced lookup: duplicate rows take their claimer's
    (size, off), in place (``k_expand``). No-op when ``first`` is None."""
    if first is None:
        return
    n = first.numel()
    core().expand_coalesced(first.data_ptr(), n, size.data_ptr(), off.data_ptr(),
                            _stream_handle(first.device))


def expand_out(first: torch.Tensor, size: torch.Tensor, off: torch.Tensor,
               out_size: torch.Tensor, out_off: torch.Tensor,
               table: Optional[torch.Tensor] = None, cslot: Optional[torch.Tensor] = None) -> None:
    """Out-of-place ``expand`` (``k_expand_out``): out_size/out_off[i] := size/off of
    first[i]. It does not modify size/off, so it may run on another stream while the
    gather reads them. With ``table``/``cslot`` from ``lookup_coalesced(table=...)`` it
    also clears the claimed slots, leaving the table zeroed for the next batch."""
    n = first.numel()
    core().expand_coalesced_out(first.data_ptr(), n, size.data_ptr(), off.data_ptr(),
                                out_size.data_ptr(), out_off.data_ptr(),
                                table.data_ptr() if table is not None else 0,
                                cslot.data_ptr() if cslot is not None else 0,
                                _stream_handle(first.device))


class StreamEvent:
    """A HIP event with a chosen fence scope, for ordering two streams of one GPU.

    ``torch.cuda.Event`` records with the default system-scope release (an L2 write-back
    and invalidate every time); ``fence="device"`` releases to device scope only
    (``hipEventReleaseToDevice``), ``"none"`` disables the system fence
    (``hipEventDisableSystemFence``), ``"system"`` is the default. Both streams must be on
    the same GPU and nothing on the host may read what the event orders."""

    def __init__(self, fence: str = "device", timing: bool = False):
        c = core()
        flags = 0 if timing else int(c.EVENT_DISABLE_TIMING)
        if fence == "device":
            flags |= int(c.EVENT_RELEASE_TO_DEVICE)
        elif fence == "none":
            flags |= int(c.EVENT_DISABLE_SYSTEM_FENCE)
        elif fence != "system":
            raise ValueError(f"unknown fence {fence!r}")
        self.fence = fence
        self.handle = int(c.event_create(flags))

    def record(self, stream: "torch.cuda.Stream") -> None:
        core().event_record(self.handle, stream.cuda_stream)

    def wait(self, stream: "torch.cuda.Stream") -> None:
        """``stream`` waits for the work this event recorded."""
        core().stream_wait_event(stream.cuda_stream, self.handle)

    def query(self) -> bool:
        """Whether the work this event marks (or the kernel that completes it) is done."""
        return bool(core().event_query(self.handle))

    def elapsed_time(self, end: "StreamEvent") -> float:
        """Milliseconds from this event to ``end`` (both created with timing=True);
        waits for ``end``."""
        return float(core().event_elapsed_ms(self.handle, end.handle))

    def __del__(self):
        h = getattr(self, "handle", 0)
        if h:
            try:
                core().event_destroy(h)
            except Exception:  # interpreter shutdown
                pass


def _event_handle(ev) -> int:
    if ev is None:
        return 0
    if isinstance(ev, StreamEvent):
        return ev.handle
    return ev.cuda_event



def _stop_handle(ev) -> int:
    """hipEvent_t a launch completes as its stop event: a ``StreamEvent`` only (a
    ``torch.cuda.Event`` has no handle before its first record)."""
    if ev is None:
        return 0
    if not isinstance(ev, StreamEvent):
        raise TypeError("a stop event must be a StreamEvent")
    return ev.handle


@dataclass
class Lookup:
    loc: torch.Tensor   # int64 [n]  physical log offset (MISS_LOC as -1 on miss)
    # int64 [n+1] response bytes per key (0 = miss); size[n] = 0. None for a blocked lookup
    size: Optional[torch.Tensor]
    # the offsets buffer as the lookup wrote it: the exclusive scan of size (off_raw[n] =
    # total bytes), or, for a blocked lookup (lookup_coalesced(blocked=True)), one packed
    # word per row: (row i's offset within its lookup workgroup's rows [b << shift, (b + 1)
    # << shift)) << 21 | its record bytes, 0 bytes for a miss or a duplicate request, with
    # off_raw[n] unwritten and `loc` written for claiming rows only; `prefix[b]` is the bytes
    # of the workgroups before b (prefix[last + 1] = the total). Read it through `off`, which
    # refuses a blocked lookup: only gather() (with its expand tail, which writes the
    # per-request sizes and offsets) reads those.
    off_raw: torch.Tensor
    prefix: Optional[torch.Tensor] = None
    shift: int = 0

    @property
    def off(self) -> torch.Tensor:
        """int64 [n+1]: the exclusive scan of ``size`` (off[n] = total bytes)."""
        if self.prefix is not None:
            raise ValueError("a blocked lookup holds workgroup-local offsets: the per-request "
                             "offsets come from the gather's expand tail")
        return self.off_raw

    @property
    def n(self) -> int:
        return self.loc.numel()

    def total(self) -> torch.Tensor:
        """Total response bytes (a one-element device tensor)."""
        if self.prefix is None:
            return self.off_raw[self.n:self.n + 1]
        nb = ((self.n - 1) >> self.shift) + 1 if self.n else 0
        return self.prefix[nb:nb + 1]

    def hits(self) -> torch.Tensor:
        return self.size[: self.n] > 0


def reserve_step_streams(device) -> None:
    """Create the routed serving step's streams (plan, SET side, reply + assembly) for
    ``device`` now. A process gets four hardware queues, handed out round robin as
    streams are first used; the step keeps four streams busy at once (with the caller's),
    so it needs them created before anything else makes streams (torch.distributed's
    communicators, other libraries). Idempotent; bench.py calls it right after choosing the
    device, and every GPU ``CacheShard`` does."""
    dev = torch.device(device)
    if dev.type == "cuda":
        core().step_streams(dev.index if dev.index is not None else torch.cuda.current_device())


class CacheShard:
    """One cache shard: an HBM arena on ``cuda:i`` or a DRAM arena on ``cpu``.

    Args:
      log_bytes: capacity of the circular value log.
      nbuckets: index buckets (power of two); 4 entries each, two-choice hashing.
      max_item: largest storable value (memcached parity default 1 MiB).
      evict: "clock" (default: objects read since the eviction hand last passed are
        re-appended instead of overwritten — memcached-LRU-like hit ratios) or "fifo"
        (plain circular log).
      reinsert_max: CLOCK reinsertion budget per SET batch in bytes (0 = auto).
      serve_blocks: resident edge-server blocks (GPU; ``serve_get`` jobs side by side).
    """

    EVICT = {"fifo": 0, "clock": 1}

    def __init__(self, log_bytes: int, nbuckets: int, max_item: int = 1 << 20,
                 device: str | torch.device = "cpu", evict: str = "clock",
                 reinsert_max: int = 0, serve_blocks: int = 8):
        self.device = torch.device(device)
        self.log_bytes = int(log_bytes)
        self.nbuckets = int(nbuckets)
        self.max_item = int(max_item)
        self.evict = evict
        ev = self.EVICT[evict]
        c = core()
        if self.device.type == "cuda":
            idx = self.device.index if self.device.index is not None else torch.cuda.current_device()
            self.device = torch.device("cuda", idx)
            reserve_step_streams(self.device)
            self._impl = c.HbmCache(self.log_bytes, self.nbuckets, self.max_item, idx, ev,
                                    int(reinsert_max), int(serve_blocks))
            self.is_gpu = True
        elif self.device.type == "cpu":
            self._impl = c.HostCache(self.log_bytes, self.nbuckets, self.max_item, ev,
                                     int(reinsert_max))
            self.is_gpu = False
        else:
            raise ValueError(f"unsupported device {self.device}")
        self.epoch = time.time()

    # -- time ---------------------------------------------------------------------
    def now(self) -> int:
        """Seconds since this shard's epoch (the unit of ``expire``)."""
        return int(time.time() - self.epoch) + 1

    def expire_at(self, ttl_seconds: int) -> int:
        return 0 if ttl_seconds <= 0 else self.now() + int(ttl_seconds)

    def _s(self) -> int:
        return _stream_handle(self.device)

    def _check(self, t: torch.Tensor, name: str):
        # a GPU shard also takes pinned host tensors: its kernels read and write them in
        # place over PCIe (the proxy's edge: keys, SET payloads and responses stay in host
        # memory, no staging copies)
        host_ok = self.is_gpu and t.device.type == "cpu" and t.is_pinned()
        if t.device != self.device and not host_ok:
            raise ValueError(f"{name} on {t.device}, shard on {self.device}")
        if not t.is_contiguous():
            raise ValueError(f"{name} must be contiguous")

    # -- GET ----------------------------------------------------------------------
    def lookup(self, keys: torch.Tensor, now: Optional[int] = None,
               reserve_bytes: int = 0, total_slot: int = -1,
               first: Optional[torch.Tensor] = None) -> Lookup:
        """Probe the index. ``reserve_bytes`` > 0 also misses objects that the next
        ``reserve_bytes`` of log appends would overwrite, so a SET of at most that many
        bytes (``set_bound``) may run between this lookup and its gather.
        ``total_slot`` >= 0 (GPU) has the kernel write off[n] into that pinned host slot
        (``host_total``), so the response size needs no device-to-host copy.
        ``first`` (GPU, from ``coalesce``): duplicate rows are answered as empty without
        a probe; ``expand`` fills them in after the gather."""
        self._check(keys, "keys")
        n = keys.shape[0]
        loc = torch.empty(n, dtype=torch.int64, device=self.device)
        size = torch.empty(n + 1, dtype=torch.int64, device=self.device)
        off = torch.empty(n + 1, dtype=torch.int64, device=self.device)
        now = self.now() if now is None else now
        if self.is_gpu:
            if first is not None:
                self._check(first, "first")
                if first.numel() != n or first.dtype != torch.int32:
                    raise ValueError("first must be int32 [n] from coalesce()")
            self._impl.lookup(keys.data_ptr(), n, loc.data_ptr(), size.data_ptr(), off.data_ptr(),
                              now, self._s(), int(reserve_bytes), int(total_slot),
                              first.data_ptr() if first is not None else 0)
        else:
            size[n] = 0
            self._impl.lookup(keys.data_ptr(), n, loc.data_ptr(), size.data_ptr(), off.data_ptr(),
                              now, int(reserve_bytes))
        return Lookup(loc, size, off)

    def lookup_coalesced(self, keys: torch.Tensor, now: Optional[int] = None,
                         reserve_bytes: int = 0, total_slot: int = -1,
                         table: Optional[torch.Tensor] = None, blocked: bool = False,
                         index_done=None):
        """``coalesce`` + ``lookup(first=...)`` fused into one kernel on GPU shards (the
        row that claims a digest probes the index for it). Returns (Lookup, first,
        cslot); duplicate rows have size 0 until ``expand(first, lk.size, lk.off)`` runs
        after the gather. ``table``: a caller-owned, zeroed coalescing table (int32,
        >= ``coalesce_table_slots(n)`` power-of-two slots) — then ``cslot`` holds each
        claimer's slot and ``expand_out`` must run to clean the table again (blocked:
        ``cslot`` is None and the gather's expand tail zeroes the whole table); otherwise
        a temporary table is zeroed here and ``cslot`` is None. ``blocked`` (GPU): the
        Lookup holds packed rows of block-local offsets and sizes (``Lookup.prefix``, no
        ``size``), which only ``gather`` with an ``expand`` tail reads — no n-row offsets
        scan between the lookup and the gather.
        ``index_done`` (GPU, a ``StreamEvent``): completes with the kernel that reads the
        index, as that kernel's own completion signal (a SET's ``index_after``).
        CPU shards: a plain lookup, ``first = cslot = None``."""
        if not self.is_gpu or keys.shape[0] == 0:
            return self.lookup(keys, now, reserve_bytes, total_slot), None, None
        self._check(keys, "keys")
        c = core()
        n = keys.shape[0]
        cslot = None
        table_clean = False
        if table is None:
            slots = int(c.coalesce_table_slots(n))
            table = torch.empty(slots, dtype=torch.int32, device=self.device)
        else:
            slots = table.numel()
            if slots < int(c.coalesce_table_slots(n)) or slots & (slots - 1):
                raise ValueError("coalescing table too small or not a power of two")
            table_clean = True
            if not blocked:  # (a blocked lookup's gather zeroes the whole table: no cslot)
                cslot = torch.empty(n, dtype=torch.int32, device=self.device)
        first = torch.empty(n, dtype=torch.int32, device=self.device)
        loc = torch.empty(n, dtype=torch.int64, device=self.device)
        # (a blocked lookup packs each row's size into its offset word: no size array)
        size = None if blocked else torch.empty(n + 1, dtype=torch.int64, device=self.device)
        off = torch.empty(n + 1, dtype=torch.int64, device=self.device)
        now = self.now() if now is None else now
        prefix = (torch.empty(int(c.LOOKUP_PREFIX_WORDS), dtype=torch.int64, device=self.device)
                  if blocked else None)
        shift = self._impl.lookup_coalesced(keys.data_ptr(), n, table.data_ptr(), slots,
                                            first.data_ptr(), loc.data_ptr(),
                                            size.data_ptr() if size is not None else 0,
                                            off.data_ptr(), now, self._s(), int(reserve_bytes),
                                            int(total_slot),
                                            cslot.data_ptr() if cslot is not None else 0,
                                            table_clean,
                                            prefix.data_ptr() if prefix is not None else 0,
                                            _stop_handle(index_done))
        return Lookup(loc, size, off, prefix, max(int(shift), 0)), first, cslot

    def host_total(self, slot: int, timeout_ms: int = 10000) -> int:
        """Total bytes of the last lookup given ``total_slot=slot``: spins on the pinned
        slot until the kernel has written it (no stream or event synchronisation)."""
        return int(self._impl.wait_host_slot(slot, timeout_ms))

    def small_get(self, keys: torch.Tensor, out_cap: int = 16 << 20,
                  now: Optional[int] = None, done_slot: int = -1):
        """GPU edge GET (the proxy's micro-batch path): probe + scan + gather in one
        kernel, each key probed once. Returns (out bytes, off[n+1]); off[n] > out_cap
        means nothing was copied. ``done_slot`` >= 0: the kernel's last workgroup
        publishes off[n] into that host slot once every output byte is visible;
        ``host_total(done_slot)`` then replaces a stream synchronisation."""
        assert self.is_gpu and keys.shape[0] <= int(core().SMALL_GET_MAX)
        self._check(keys, "keys")
        n = keys.shape[0]
        out = torch.empty(max(int(out_cap), 16), dtype=torch.uint8, device=self.device)
        off = torch.empty(n + 1, dtype=torch.int64, device=self.device)
        self._impl.small_get(keys.data_ptr(), n, out.data_ptr(), int(out_cap), off.data_ptr(),
                             self.now() if now is None else now, self._s(), int(done_slot))
        return out, off

    def serve_get(self, keys: torch.Tensor, out_cap: int = 16 << 20,
                  now: Optional[int] = None, done_slot: int = 5, timeout_ms: int = 10000):
        """The same edge GET answered by the resident edge-server kernel (no launch):
        ``keys`` are host digests; returns (out bytes, off[n+1]) once the server has
        published the job's total into ``done_slot``. None when the job could not be
        queued (ring full, n > SERVE_KEYS). Records a concurrent SET overwrote while
        they were copied come back with a zeroed magic word (treat as misses). The job is
        ordered after the work queued so far on the current stream (the server runs on no
        stream: the binding polls an event recorded there before it queues the job)."""
        assert self.is_gpu
        keys = keys.to("cpu").contiguous()
        n = keys.shape[0]
        out = torch.zeros(max(int(out_cap), 16), dtype=torch.uint8, device=self.device)
        off = torch.zeros(n + 1, dtype=torch.int64, device=self.device)
        if not self._impl.serve_get(keys.data_ptr(), n, out.data_ptr(), int(out_cap),
                                    off.data_ptr(), self.now() if now is None else now,
                                    int(done_slot), self._s()):
            return None
        self._impl.serve_wait(int(done_slot), int(timeout_ms))
        return out, off

    def gather(self, lk: Lookup, out: Optional[torch.Tensor] = None,
               total: Optional[int] = None, out_cap: Optional[int] = None,
               expand=None) -> torch.Tensor:
        """Copy hits into ``out`` (allocated from off[n] if not given: one sync).
        ``out_cap`` (GPU): the kernel writes nothing when off[n] exceeds it, so a gather
        can be queued before the total is known. ``expand`` (GPU, a coalesced lookup):
        (first, out_size, out_off, table, cslot) — the gather also writes every request's
        (size, off) from its claimer and clears the coalescing table (``expand_out``: the
        claimers' ``cslot`` slots, or for a blocked lookup the whole table)."""
        if out is None:
            total = int(lk.total().item()) if total is None else total
            out = torch.empty(max(total, 16), dtype=torch.uint8, device=self.device)
        self._check(out, "out")
        if self.is_gpu:
            cap = out.numel() if out_cap is None else min(int(out_cap), out.numel())
            ex, slots = [0] * 6, 0
            if expand is not None:
                first, osz, ooff, table, cslot = expand
                ex = [first.data_ptr(), lk.size.data_ptr() if lk.size is not None else 0,
                      osz.data_ptr(), ooff.data_ptr(),
                      table.data_ptr() if table is not None else 0,
                      cslot.data_ptr() if cslot is not None else 0]
                slots = table.numel() if table is not None else 0
            elif lk.prefix is not None:
                raise ValueError("a blocked lookup's offsets are read only with an expand tail")
            self._impl.gather(lk.loc.data_ptr(), lk.off_raw.data_ptr(), lk.n, out.data_ptr(),
                              self._s(), cap, *ex,
                              lk.prefix.data_ptr() if lk.prefix is not None else 0, lk.shift,
                              slots)
        else:
            self._impl.gather(lk.loc.data_ptr(), lk.off.data_ptr(), lk.n, out.data_ptr())
        return out

    def get(self, keys: torch.Tensor, now: Optional[int] = None):
        """lookup + gather. Returns (out bytes, off[n], size[n]); record i = out[off[i]:+size[i]]."""
        if not self.is_gpu:
            lk = self.lookup(keys, now)
            return self.gather(lk), lk.off[: lk.n], lk.size[: lk.n]
        lk = self.lookup(keys, now, total_slot=1)
        out = self.gather(lk, total=self.host_total(1))
        return out, lk.off[: lk.n], lk.size[: lk.n]

    # -- SET ----------------------------------------------------------------------
    @staticmethod
    def payload_bound(n: int, payload_bytes: int) -> int:
        """Upper bound of the log bytes ``n`` values from a ``payload_bytes`` buffer
        occupy (32-B header + value, 16-B aligned, per item)."""
        return 48 * int(n) + int(payload_bytes)

    def set_bound(self, n: int, payload_bytes: int) -> int:
        """Upper bound of the log bytes a SET of ``n`` values from a ``payload_bytes``
        buffer appends — its own records plus, under CLOCK, the reinsertions of
        referenced objects it triggers (the ``reserve_bytes`` a lookup that a SET may
        overtake needs)."""
        return self.payload_bound(n, payload_bytes) + int(self._impl.reinsert_max)

    def store(self, keys: torch.Tensor, values: torch.Tensor, val_off: torch.Tensor,
              vlen: torch.Tensor, flags: Optional[torch.Tensor] = None,
              expire: Optional[torch.Tensor] = None, now: Optional[int] = None,
              bytes_bound: Optional[int] = None,
              index_after=None, append_after=None, append_done=None, phase: int = 0,
              plan_done=None, done=None) -> None:
        """SET a batch (later duplicates win). ``bytes_bound`` bounds the log bytes the
        batch appends; the default assumes every byte of ``values`` is stored.
        ``index_after`` (GPU, a recorded ``torch.cuda.Event`` or a ``StreamEvent``):
        dedupe, sizing and the log append run at once, the index insert waits for the
        event — so a lookup followed by that event on another stream overlaps the SET's log
        write (see ``HbmCache::store``). ``append_after`` (GPU, an event): the log append
        waits for it, the CLOCK hand and the SET planning do not (a gather still reading the
        region the append overwrites may run meanwhile). ``append_done`` (GPU, an event):
        recorded right after the log append. ``phase`` (GPU): 1 queues only the batch's
        CLOCK hand (a full cache), 2 the rest of the chain for the same batch; 0 both. A
        phase-1 hand is *detached*: it may run as soon as the previous batch's planning is
        done (``plan_done`` of that batch's phase 2), beside that batch's append and index
        insert — its reinsertions are indexed as moves, dropped when the key's entry has
        moved on (``HbmCache::store``). ``plan_done`` (GPU, an event): recorded after the
        batch's planning kernels. ``done`` (GPU, a ``StreamEvent``): completes with everything
        the call queued, carried by the chain's last kernel as its completion signal."""
        for t, nm in ((keys, "keys"), (values, "values"), (val_off, "val_off"), (vlen, "vlen")):
            self._check(t, nm)
        if vlen.dtype != torch.int32 or val_off.dtype != torch.int64:
            raise TypeError("vlen must be int32 and val_off int64")
        n = keys.shape[0]
        if n == 0:
            if done is not None and self.is_gpu:
                done.record(torch.cuda.current_stream(self.device))   # nothing to carry it
            return
        now = self.now() if now is None else now
        fp = 0 if flags is None else flags.data_ptr()
        ep = 0 if expire is None else expire.data_ptr()
        # the same bound on both twins: the CLOCK hand's reinsertion cap follows from it
        bound = (self.payload_bound(n, values.numel()) if bytes_bound is None
                 else int(bytes_bound))
        if self.is_gpu:
            self._impl.store(keys.data_ptr(), values.data_ptr(), val_off.data_ptr(), vlen.data_ptr(),
                             fp, ep, n, bound, now, self._s(), _event_handle(index_after),
                             _event_handle(append_after), _event_handle(append_done), phase,
                             _event_handle(plan_done), _stop_handle(done))
        elif phase != 1:
            self._impl.store(keys.data_ptr(), values.data_ptr(), val_off.data_ptr(), vlen.data_ptr(),
                             fp, ep, n, now, bound)

    def set_many(self, keys: Sequence[bytes], values: Sequence[bytes], ttl: int = 0,
                 flags: int = 0) -> None:
        d = digest_strings(keys, self.device)
        v, vo, vl = pack_values(values, self.device)
        ex = torch.full((len(keys),), self.expire_at(ttl), dtype=torch.int32, device=self.device)
        fl = torch.full((len(keys),), flags, dtype=torch.int32, device=self.device)
        self.store(d, v, vo, vl, fl, ex)

    def get_many(self, keys: Sequence[bytes]) -> list:
        d = digest_strings(keys, self.device)
        out, off, size = self.get(d)
        return [None if r is None else r[0] for r in unpack_records(out, off, size)]

    # -- DELETE / maintenance ------------------------------------------------------
    def remove(self, keys: torch.Tensor, now: Optional[int] = None) -> torch.Tensor:
        self._check(keys, "keys")
        n = keys.shape[0]
        found = torch.zeros(n, dtype=torch.uint8, device=self.device)
        now = self.now() if now is None else now
        if self.is_gpu:
            self._impl.remove(keys.data_ptr(), n, found.data_ptr(), now, self._s())
        else:
            self._impl.remove(keys.data_ptr(), n, found.data_ptr(), now)
        return found.bool()

    def touch(self, keys: torch.Tensor, expire: torch.Tensor,
              flags: Optional[torch.Tensor] = None, key_bytes=None,
              now: Optional[int] = None) -> torch.Tensor:
        """Change the expiry of live objects in place (``k_touch`` on a GPU shard): row i's
        object gets the absolute expiry ``expire[i]`` (int32, 0 = never; a value <= ``now``
        kills it) and, with ``flags`` (int32 [n]), new flags. The value's bytes do not move.
        ``key_bytes``: ``(uint8 buffer, int64 offsets[n+1])`` tensors as ``pack_bytes`` lays
        keys out; then a row only matches a *keyed* value (``keyed(key, payload)``) that
        carries exactly that key, so a digest collision cannot touch another object.
        Returns ``hit`` (uint8 [n]): 1 where a live object was updated (also counted in
        ``counters()["touched"]``). Asynchronous on the current stream, like ``remove``;
        which of several rows with one digest wins is unspecified."""
        self._check(keys, "keys")
        self._check(expire, "expire")
        n = keys.shape[0]
        if expire.dtype != torch.int32 or expire.numel() != n:
            raise TypeError("expire must be int32 [n]")
        fp = 0
        if flags is not None:
            self._check(flags, "flags")
            if flags.dtype != torch.int32 or flags.numel() != n:
                raise TypeError("flags must be int32 [n]")
            fp = flags.data_ptr()
        kb = ko = 0
        if key_bytes is not None:
            buf, offs = key_bytes
            self._check(buf, "key bytes")
            self._check(offs, "key offsets")
            if buf.dtype != torch.uint8 or offs.dtype != torch.int64 or offs.numel() != n + 1:
                raise TypeError("key_bytes must be (uint8 buffer, int64 offsets[n + 1])")
            kb, ko = buf.data_ptr(), offs.data_ptr()
        hit = torch.zeros(n, dtype=torch.uint8, device=self.device)
        if n == 0:
            return hit
        now = self.now() if now is None else now
        args = (keys.data_ptr(), expire.data_ptr(), fp, kb, ko, n, hit.data_ptr(), now)
        if self.is_gpu:
            self._impl.touch(*args, self._s())
        else:
            self._impl.touch(*args)
        return hit

    def touch_many(self, keys: Sequence[bytes], ttl: int, keyed: bool = True) -> list:
        """``touch`` for byte-string keys, as ``set_many`` / ``get_many``: a new TTL from now
        (<= 0: never expires). ``keyed``: the objects are keyed values and only exact keys
        match. Returns one bool per key."""
        keys = list(keys)
        d = digest_strings(keys, self.device)
        ex = torch.full((len(keys),), self.expire_at(ttl), dtype=torch.int32, device=self.device)
        kb = None
        if keyed:
            buf, offs = pack_bytes(keys)
            buf = np.ascontiguousarray(buf) if buf.size else np.zeros(1, np.uint8)
            kb = (torch.from_numpy(buf.copy()).to(self.device),
                  torch.from_numpy(offs).to(self.device))
        return [bool(x) for x in self.touch(d, ex, key_bytes=kb).tolist()]

    # -- sliced GET -----------------------------------------------------------------
    def get_keyed_slices(self, keys: torch.Tensor, key_bytes, specs: torch.Tensor,
                         out: torch.Tensor, now: Optional[int] = None, reserve_bytes: int = 0,
                         conds=None):
        """Sliced GET (``csrc/slice.h``; ``k_slice_plan`` on a GPU shard): row i asks for the
        window ``specs[i]`` of the keyed value stored under ``keys[i]`` (int64 [n, 2]) with
        exactly the key ``key_bytes`` names (``(uint8 buffer, int64 offsets[n + 1])``, as
        ``touch``). ``specs``: uint8 [n, SLICE_SPEC_BYTES] from ``pack_slice_specs``; ``out``: the
        uint8 response buffer. Returns ``(rows, res)``: uint8 [n, SLICE_ROW_BYTES] result rows
        and int64 [2] ``{rows that hit, total bytes}``; a row's bytes start at its ``out_off``:
        the value's first ``head_bytes`` bytes, then the 16-byte granules that cover the window.
        When the total exceeds ``out.numel()`` nothing is written to ``out``; rows and totals
        are complete. ``n`` <= SMALL_GET_MAX. Asynchronous on the current stream; a shard's
        sliced GETs share one workspace, so calls on different streams run one after the other
        (the later one waits for the earlier one's event on the device).
        ``conds``: ``None``, or ``(uint8 [n, SLICE_COND_BYTES], uint8 candidate bytes)`` on the
        shard's device, from ``pack_slice_conds``: one condition per row, decided by the shard
        against the stored ``ETag`` / ``Last-Modified`` (``k_slice_plan`` on a GPU shard). A
        matched ``none_match`` / ``modified_since`` row returns the head alone with status
        ``SLICE_NOT_MODIFIED``; an unmatched ``if_range_*`` row the whole value. Every row's
        ``[off, off + len)`` must lie inside the candidate bytes (the shard reads nothing of a
        row's candidates outside that range; records that overrun it never match)."""
        c = core()
        self._check(keys, "keys")
        self._check(specs, "specs")
        self._check(out, "out")
        n = keys.shape[0]
        buf, offs = key_bytes
        self._check(buf, "key bytes")
        self._check(offs, "key offsets")
        if buf.dtype != torch.uint8 or offs.dtype != torch.int64 or offs.numel() != n + 1:
            raise TypeError("key_bytes must be (uint8 buffer, int64 offsets[n + 1])")
        if specs.dtype != torch.uint8 or specs.numel() != n * c.SLICE_SPEC_BYTES:
            raise TypeError("specs must be uint8 [n, SLICE_SPEC_BYTES] from pack_slice_specs")
        if out.dtype != torch.uint8:
            raise TypeError("out must be uint8")
        if n > c.SMALL_GET_MAX:
            raise ValueError("sliced GET: at most %d rows a call" % c.SMALL_GET_MAX)
        rows = torch.zeros((n, c.SLICE_ROW_BYTES), dtype=torch.uint8, device=self.device)
        res = torch.zeros(2, dtype=torch.int64, device=self.device)
        now = self.now() if now is None else now
        args = (keys.data_ptr(), buf.data_ptr(), offs.data_ptr(), specs.data_ptr(), n,
                rows.data_ptr(), out.data_ptr(), out.numel(), res.data_ptr(), now)
        cp = (0, 0)
        if conds is not None:
            crow, cbytes = conds
            self._check(crow, "conds")
            self._check(cbytes, "candidate bytes")
            if crow.dtype != torch.uint8 or crow.numel() != n * c.SLICE_COND_BYTES or \
                    cbytes.dtype != torch.uint8:
                raise TypeError("conds must be (uint8 [n, SLICE_COND_BYTES], uint8 bytes) "
                                "from pack_slice_conds")
            cp =(crow.data_ptr(), cbytes.data_ptr() if cbytes.numel() else 0)
        if self.is_gpu:
            self._impl.get_keyed_slices(*args, self._s(), int(reserve_bytes), *cp)
        else:
            self._impl.get_keyed_slices(*args, int(reserve_bytes), *cp)
        return rows, res

    def get_slices(self, keys: Sequence[bytes], specs, now: Optional[int] = None,
                   reserve_bytes: int = 0, out_cap: Optional[int] = None, conds=None) -> list:
        """Sliced GET for byte-string keys: the HTTP head and one byte window of each stored
        response, cut by the shard (the rest of the object is not moved). ``specs[i]`` is
        ``("head",)``, ``("range", a, b)`` (body bytes a..b inclusive, b clamped),
        ``("from", a)``, ``("suffix", a)`` (the last a bytes) or ``("whole",)``. Returns one
        dict per row: ``{status, head, window, body_len, first, vlen, flags, expire}`` with
        ``status`` one of ``"miss"``, ``"ok"``, ``"unsat"`` (the head, an empty window) and
        ``"whole"`` (a ``("whole",)`` row, or a value that is no sliceable HTTP response:
        ``window`` holds the whole stored value, ``head`` is empty). ``head`` is the payload
        from ``HTTP/`` through the blank line. Works on GPU and CPU shards. Synchronises.
        ``out_cap``: the response buffer's bytes; by default it grows until the batch fits (a
        batch that did not fit is asked again, and counted again); an explicit one that is too
        small raises ``ValueError``.
        ``conds``: one condition per row (``pack_slice_conds``' forms, ``None``: none), the
        client's validators, which the shard compares with the stored ``ETag`` /
        ``Last-Modified``: a ``none_match`` / ``modified_since`` row that matches answers
        ``"not_modified"`` (``head`` set, ``window`` empty, whatever its spec: a 304), one that
        does not answers its spec; an ``if_range_*`` row that matches answers its spec (a
        206), one that does not answers ``"whole"`` (a 200)."""
        c = core()
        keys = [bytes(k) for k in keys]
        n = len(keys)
        if len(specs) != n:
            raise ValueError("one window spec per key")
        if conds is not None and len(conds) != n:
            raise ValueError("one condition (or None) per key")
        if n == 0:
            return []
        d = digest_strings(keys, self.device)
        buf, offs = pack_bytes(keys)
        buf = np.ascontiguousarray(buf) if buf.size else np.zeros(1, np.uint8)
        kb = (torch.from_numpy(buf.copy()).to(self.device), torch.from_numpy(offs).to(self.device))
        sp = torch.from_numpy(pack_slice_specs(specs)).to(self.device)
        cd = None
        if conds is not None:
            crow, cbytes = pack_slice_conds(conds)
            cd = (torch.from_numpy(crow.copy()).to(self.device),
                  torch.from_numpy(cbytes.copy()).to(self.device))
        cap = (1 << 20) if out_cap is None else int(out_cap)
        while True:
            out = torch.zeros(max(cap, 16), dtype=torch.uint8, device=self.device)[:cap]
            rows, res = self.get_keyed_slices(d, kb, sp, out, now, reserve_bytes, conds=cd)
            total = int(res.tolist()[1])  # (waits for the stream)
            if total <= cap:
                break
            if out_cap is not None:
                raise ValueError("sliced GET: the batch needs %d bytes, out_cap is %d" % (total, cap))
            cap = total
        return unpack_slices(rows, out)

    def remove_keyed_prefix(self, prefix: bytes, now: Optional[int] = None) -> tuple[int, int]:
        """Prefix purge: remove every live object whose stored key starts with ``prefix``
        (1..65535 bytes; an empty prefix is ``flush``). Returns (objects removed, their
        item bytes); the objects are also counted in ``counters()["purged"]``. Synchronises,
        like ``sweep``. On a GPU shard ``k_keyed_scan<PrefixMatch, RemoveAction>`` walks the index and compares the
        key bytes stored in the value log.

        Defined for *keyed* values only (``keyed(key, payload)``, what the proxy's backends
        store): the key is read from the value. On other values it is memory-safe and
        removes whatever happens to parse as a matching keyed record."""
        prefix = bytes(prefix)
        if not 1 <= len(prefix) <= 0xFFFF:
            raise ValueError("purge prefix must hold 1..65535 bytes")
        now = self.now() if now is None else now
        if not self.is_gpu:
            return tuple(self._impl.remove_keyed_prefix(prefix, now))
        img = np.frombuffer(core().keyed_prefix_image(prefix), dtype=np.uint8)
        image = torch.from_numpy(img.copy()).to(self.device)
        out = torch.empty(2, dtype=torch.int64, device=self.device)
        self._impl.remove_keyed_prefix(image.data_ptr(), len(prefix), now, out.data_ptr(),
                                       self._s())
        removed, nbytes = out.tolist()  # (waits for the stream)
        return int(removed), int(nbytes)

    def soften_keyed_prefix(self, prefix: bytes, stale_at: int, expire_cap: int = 0,
                            exact: bool = False, now: Optional[int] = None) -> int:
        """Soft purge: every live object whose stored key starts with ``prefix`` (``exact``:
        equals it) gets ``flags = stale_at`` and, where ``expire_cap`` is non-zero and the
        object never expires or expires after it, ``expire = expire_cap`` (absolute, in the
        shard's clock, and after ``now``): a life is only shortened. The value, its place and
        the CLOCK reference bit stay. Returns the number of live matching objects, whether
        or not their words changed. Synchronises, like ``remove_keyed_prefix``; on a GPU
        shard ``k_keyed_scan<PrefixMatch, SoftenAction>`` does the scan. Defined for keyed values only."""
        prefix = bytes(prefix)
        if not 1 <= len(prefix) <= 0xFFFF:
            raise ValueError("purge prefix must hold 1..65535 bytes")
        now = self.now() if now is None else now
        stale_at, expire_cap = int(stale_at) & 0xFFFFFFFF, int(expire_cap)
        if expire_cap and expire_cap <= now:
            raise ValueError("soft purge: the expiry cap must lie after now")
        if not self.is_gpu:
            return int(self._impl.soften_keyed_prefix(prefix, bool(exact), stale_at, expire_cap,
                                                      now))
        img = np.frombuffer(core().keyed_prefix_image(prefix), dtype=np.uint8)
        image = torch.from_numpy(img.copy()).to(self.device)
        out = torch.empty(1, dtype=torch.int64, device=self.device)
        self._impl.soften_keyed_prefix(image.data_ptr(), len(prefix), bool(exact), stale_at,
                                       expire_cap, now, out.data_ptr(), self._s())
        return int(out.item())  # (waits for the stream)

    @staticmethod
    def _tag_list(tags: Sequence[bytes]) -> list[int]:
        tags = [bytes(t) for t in tags]
        if not 1 <= len(tags) <= MAX_PURGE_TAGS:
            raise ValueError("tag purge takes 1..64 tags")
        return [tag_hash(t) for t in tags]

    def remove_keyed_tags(self, tags: Sequence[bytes],
                          now: Optional[int] = None) -> tuple[int, int]:
        """Purge by surrogate key: removes every live object whose stored keyed value carries
        a tag block (``tagged``) naming one of ``tags`` (1..64 byte strings), or the overflow
        block. Returns ``(objects removed, their item bytes)``; synchronises, like
        ``remove_keyed_prefix``. On a GPU shard ``k_keyed_scan<TagMatch, RemoveAction>`` does the scan."""
        hashes = self._tag_list(tags)
        now = self.now() if now is None else now
        if not self.is_gpu:
            removed, nbytes = self._impl.remove_keyed_tags(hashes, now)
            return int(removed), int(nbytes)
        lst = torch.from_numpy(np.array(hashes, dtype=np.uint64).view(np.int64)).to(self.device)
        out = torch.empty(2, dtype=torch.int64, device=self.device)
        self._impl.remove_keyed_tags(lst.data_ptr(), len(hashes), now, out.data_ptr(), self._s())
        removed, nbytes = out.tolist()  # (waits for the stream)
        return int(removed), int(nbytes)

    def soften_keyed_tags(self, tags: Sequence[bytes], stale_at: int, expire_cap: int = 0,
                          now: Optional[int] = None) -> int:
        """Soft purge by surrogate key: ``remove_keyed_tags``' matcher with
        ``soften_keyed_prefix``'s action and contract (``flags = stale_at``, the expiry capped
        at ``expire_cap`` and never extended, the count of live matches). Synchronises; on a
        GPU shard ``k_keyed_scan<TagMatch, SoftenAction>`` does the scan."""
        hashes = self._tag_list(tags)
        now = self.now() if now is None else now
        stale_at, expire_cap = int(stale_at) & 0xFFFFFFFF, int(expire_cap)
        if expire_cap and expire_cap <= now:
            raise ValueError("soft purge: the expiry cap must lie after now")
        if not self.is_gpu:
            return int(self._impl.soften_keyed_tags(hashes, stale_at, expire_cap, now))
        lst = torch.from_numpy(np.array(hashes, dtype=np.uint64).view(np.int64)).to(self.device)
        out = torch.empty(1, dtype=torch.int64, device=self.device)
        self._impl.soften_keyed_tags(lst.data_ptr(), len(hashes), stale_at, expire_cap, now,
                                     out.data_ptr(), self._s())
        return int(out.item())  # (waits for the stream)

    def _glob_image(self, pattern: bytes) -> torch.Tensor:
        # (ValueError on a refused pattern: empty, stars only, a dangling backslash, over a limit)
        img = np.frombuffer(core().keyed_glob_image(bytes(pattern)), dtype=np.uint8)
        return torch.from_numpy(img.copy()).to(self.device)

    def remove_keyed_glob(self, pattern: bytes, now: Optional[int] = None) -> tuple[int, int]:
        """Purge by glob: removes every live object whose stored key, up to its first ``0x1f``
        byte (the separator before a Vary variant's suffix), matches ``pattern``: ``*`` is any
        run of bytes (``/`` included), ``\\`` makes the next byte literal, every other byte is
        literal, and the match is anchored at both ends. At most 8 stars and 1024 literal
        bytes; an empty pattern, stars only (that is ``flush``) and a dangling ``\\`` raise
        ``ValueError``. Returns ``(objects removed, their item bytes)``; synchronises, like
        ``remove_keyed_prefix``. On a GPU shard ``k_keyed_scan<GlobMatch, RemoveAction>`` does the scan."""
        image = self._glob_image(pattern)
        now = self.now() if now is None else now
        if not self.is_gpu:
            removed, nbytes = self._impl.remove_keyed_glob(bytes(pattern), now)
            return int(removed), int(nbytes)
        out = torch.empty(2, dtype=torch.int64, device=self.device)
        self._impl.remove_keyed_glob(image.data_ptr(), image.numel(), now, out.data_ptr(),
                                     self._s())
        removed, nbytes = out.tolist()  # (waits for the stream)
        return int(removed), int(nbytes)

    def soften_keyed_glob(self, pattern: bytes, stale_at: int, expire_cap: int = 0,
                          now: Optional[int] = None) -> int:
        """Soft purge by glob: ``remove_keyed_glob``'s matcher with ``soften_keyed_prefix``'s
        action and contract (``flags = stale_at``, the expiry capped at ``expire_cap`` and
        never extended, the count of live matches). Synchronises; on a GPU shard
        ``k_keyed_scan<GlobMatch, SoftenAction>`` does the scan."""
        image = self._glob_image(pattern)
        now = self.now() if now is None else now
        stale_at, expire_cap = int(stale_at) & 0xFFFFFFFF, int(expire_cap)
        if expire_cap and expire_cap <= now:
            raise ValueError("soft purge: the expiry cap must lie after now")
        if not self.is_gpu:
            return int(self._impl.soften_keyed_glob(bytes(pattern), stale_at, expire_cap, now))
        out = torch.empty(1, dtype=torch.int64, device=self.device)
        self._impl.soften_keyed_glob(image.data_ptr(), image.numel(), stale_at, expire_cap, now,
                                     out.data_ptr(), self._s())
        return int(out.item())  # (waits for the stream)

    def list_keyed(self, prefix: Optional[bytes] = None, tags: Optional[Sequence[bytes]] = None,
                   exact: bool = False, start: int = 0, limit: int = 100, key_cap: int = 256,
                   now: Optional[int] = None, glob: Optional[bytes] = None) -> dict:
        """List the live keyed objects whose stored key starts with ``prefix`` (``exact``:
        equals it), or that carry one of ``tags`` (``remove_keyed_tags``' matcher), or whose
        key matches ``glob`` (``remove_keyed_glob``'s matcher; not with ``exact``), or, with
        none of them, all of them. Read-only: the index, the log and the counters stay as they
        are. Returns ``{"matched", "bytes", "next", "rows"}``: the live matches in the whole
        shard and their item bytes (what a hard purge of the same pattern would remove), and
        up to ``limit`` (0..MAX_LIST_ROWS; 0 only counts) row dicts for the matches at index
        slots >= ``start``, in slot order. ``next`` is the ``start`` of the following page, or
        ``None`` when no match lies past the last row. A row holds ``slot``, ``loc``,
        ``digest`` (lo, hi), ``vlen``, ``expire``, ``flags``, ``klen``, ``ntags`` (0: no or
        malformed tag block, 0xff: the overflow block), ``referenced`` (the CLOCK bit),
        ``changed`` and ``key``: the first ``min(klen, key_cap - 2)`` key bytes (``key_cap``: a
        multiple of 16 in 16..1024; ``truncated`` tells a longer key). Synchronises, like
        ``remove_keyed_prefix``; on a GPU shard ``k_list_scan`` / ``k_list_emit`` do the work.
        ``changed`` rows (klen 0, no key) occur only beside SETs on another stream.
        Precondition: one listing at a time per shard (the match bitmap and the result words are
        the shard's): listings on different streams of one shard must be ordered by the caller.
        This method synchronises, so calls from one thread are."""
        c = core()
        if prefix is not None and tags is not None:
            raise ValueError("list by prefix or by tags, not both")
        if glob is not None and (prefix is not None or tags is not None):
            raise ValueError("list by prefix, by tags or by glob, not two of them")
        if exact and prefix is None:
            raise ValueError("exact needs a key")
        limit, key_cap, start = int(limit), int(key_cap), int(start)
        if not 0 <= limit <= c.MAX_LIST_ROWS:
            raise ValueError("list: at most %d rows a call" % c.MAX_LIST_ROWS)
        if key_cap % 16 or not 16 <= key_cap <= 1024:
            raise ValueError("list: key_cap must be a multiple of 16 in 16..1024")
        nslots = 4 * self.nbuckets
        if not 0 <= start <= nslots:
            raise ValueError("list: the start slot lies past the index")
        mode, hashes = c.LIST_ALL, []
        if prefix is not None:
            prefix = bytes(prefix)
            if not 1 <= len(prefix) <= 0xFFFF:
                raise ValueError("list prefix must hold 1..65535 bytes")
            mode = c.LIST_PREFIX
        elif tags is not None:
            hashes = self._tag_list(tags)
            mode = c.LIST_TAGS
        elif glob is not None:
            glob = bytes(glob)
            image = self._glob_image(glob)
            mode = c.LIST_GLOB
        now = self.now() if now is None else now
        rows = torch.zeros((max(limit, 1), c.LIST_ROW_BYTES), dtype=torch.uint8, device=self.device)
        keys = torch.zeros((max(limit, 1), key_cap), dtype=torch.uint8, device=self.device)
        out = torch.zeros(4, dtype=torch.int64, device=self.device)
        if self.is_gpu:
            lst, plen = None, 0
            if mode == c.LIST_PREFIX:
                img = np.frombuffer(c.keyed_prefix_image(prefix), dtype=np.uint8)
                image = torch.from_numpy(img.copy()).to(self.device)
                plen = len(prefix)
            elif mode == c.LIST_GLOB:
                plen = image.numel()      # (the compiled pattern's bytes)
            elif mode == c.LIST_TAGS:
                lst = torch.from_numpy(np.array(hashes, dtype=np.uint64).view(np.int64))
                lst = lst.to(self.device)
            self._impl.list_keyed(mode, image.data_ptr() if plen else 0, plen, bool(exact),
                                  0 if lst is None else lst.data_ptr(), len(hashes), start, limit,
                                  key_cap, now, rows.data_ptr(), keys.data_ptr(), out.data_ptr(),
                                  self._s())
        else:
            self._impl.list_keyed(mode, glob if mode == c.LIST_GLOB else prefix or b"",
                                  bool(exact), hashes, start, limit, key_cap,
                                  now, rows.data_ptr(), keys.data_ptr(), out.data_ptr())
        matched, nbytes, listed, nxt = (int(x) for x in out.tolist())  # (waits for the stream)
        r64 = rows.cpu().numpy().view(np.uint64)
        r32 = rows.cpu().numpy().view(np.uint32)
        kb = keys.cpu().numpy()
        res = []
        for i in range(listed):
            klen, bits = int(r32[i, 11]), int(r32[i, 13])
            have = min(klen, key_cap - 2)
            res.append({
                "slot": int(r64[i, 0]), "loc": int(r64[i, 1]),
                "digest": (int(r64[i, 2]), int(r64[i, 3])),
                "vlen": int(r32[i, 8]), "expire": int(r32[i, 9]), "flags": int(r32[i, 10]),
                "klen": klen, "ntags": int(r32[i, 12]),
                "referenced": bool(bits & 1), "changed": bool(bits & 2),
                "key": kb[i, 2:2 + have].tobytes(), "truncated": klen > have,
            })
        return {"matched": matched, "bytes": nbytes, "next": None if nxt >= nslots else nxt,
                "rows": res}

    def sweep(self, now: Optional[int] = None) -> tuple[int, int]:
        now = self.now() if now is None else now
        return tuple(self._impl.sweep(now, self._s()) if self.is_gpu else self._impl.sweep(now))

    def flush(self) -> None:
        if self.is_gpu:
            self._impl.flush(self._s())
        else:
            self._impl.flush()

    def export_keys(self, now: Optional[int] = None) -> torch.Tensor:
        """Digests of every live object in this shard, int64 [m, 2] on the shard's device."""
        now = self.now() if now is None else now
        cap = 1 << 16
        while True:
            out = torch.empty((cap, 2), dtype=torch.int64, device=self.device)
            if self.is_gpu:
                m = self._impl.export_keys(out.data_ptr(), cap, now, self._s())
            else:
                m = self._impl.export_keys(out.data_ptr(), cap, now)
            if m <= cap:
                return out[:m]
            cap = int(m * 1.25) + 1024

    def save(self, path: str) -> None:
        """Snapshot index + log + head to ``path`` (warm restart)."""
        import struct

        user = [struct.unpack("<Q", struct.pack("<d", self.epoch))[0], 0, 0, 0]
        if self.is_gpu:
            self._impl.save(path, user, self._s())
        else:
            self._impl.save(path, user)

    def load(self, path: str) -> None:
        """Restore a snapshot written by ``save`` (same geometry); expiry times
        stay relative to the saved epoch."""
        import struct

        user = self._impl.load(path, self._s()) if self.is_gpu else self._impl.load(path)
        self.epoch = struct.unpack("<d", struct.pack("<Q", int(user[0])))[0]

    def counters(self) -> dict:
        return self._impl.counters(self._s()) if self.is_gpu else self._impl.counters()

    def head(self) -> int:
        return self._impl.head(self._s()) if self.is_gpu else self._impl.head()

    def reserve(self, n: int) -> None:
        if self.is_gpu:
            self._impl.reserve(n)
