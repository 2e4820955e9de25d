"""The request and response batches of ``ShardedCache`` (re-exported by
``models.sharded_cache``, where callers import them from)."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import torch

SKIP_VLEN = -1  # int32 view of the kSkipVlen sentinel (row not for this tier)


@dataclass
class GetResult:
    """Values for a GET batch, in the caller's request order.

    ``data`` holds [ItemHeader|value|pad] records; request i's record is
    data[off[i] : off[i] + size[i]] (size 0 = miss)."""

    data: torch.Tensor
    off: torch.Tensor
    size: torch.Tensor
    _pending: Optional[object] = None  # value all-to-all still in flight (routed serve)

    def wait(self) -> "GetResult":
        """Order the current stream after the reply transfer. A routed ``serve`` returns
        while its reply all-to-all (and the per-request assembly that reads its in-band
        headers) is still running, so the next step's routing overlaps it; a host-edge
        ``serve`` returns while the DMA copy of its response into host memory runs (then
        this blocks the host until it is done); call this before reading ``data``, ``off``
        or ``size``."""
        if self._pending is not None:
            self._pending.wait()
            self._pending = None
        return self

    def hit_mask(self) -> torch.Tensor:
        return self.size > 0


@dataclass
class SetBatch:
    keys: torch.Tensor      # int64 [n, 2]
    values: torch.Tensor    # uint8 payload buffer (16-B aligned values, +16 slack)
    val_off: torch.Tensor   # int64 [n]
    vlen: torch.Tensor      # int32 [n]
    flags: Optional[torch.Tensor] = None   # int32 [n]
    expire: Optional[torch.Tensor] = None  # int32 [n]
    # simulated world only (bench.py --simulate-world): the digests the owner stores
    probe_keys: Optional[torch.Tensor] = None  # int64 [n, 2]


def records_to_set_batch(keys: torch.Tensor, res: GetResult) -> SetBatch:
    """Turn GET records back into a SET batch (replica fill, shard migration).
    Misses become skip rows."""
    words = res.data[: res.data.numel() // 4 * 4].view(torch.int32)
    hit = res.size > 0
    base = torch.where(hit, torch.div(res.off, 4, rounding_mode="floor"), torch.zeros_like(res.off))
    v = words.index_select(0, base + 4)
    vlen = torch.where(hit, v, torch.full_like(v, SKIP_VLEN))
    flags = words.index_select(0, base + 5)
    expire = words.index_select(0, base + 6)
    val_off = torch.where(hit, res.off + 32, torch.zeros_like(res.off))
    return SetBatch(keys=keys.contiguous(), values=res.data, val_off=val_off.contiguous(),
                    vlen=vlen.contiguous(), flags=flags.contiguous(), expire=expire.contiguous())
