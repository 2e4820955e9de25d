#!/usr/bin/env python3
"""GPU time of an in-place touch (k_touch) against the sequence it replaces.

One CacheShard is filled with N keyed objects ([u16 klen | key | payload], 1 KiB payloads,
48-byte URL-shaped keys; N = 1M by default). Per repetition a seeded random batch of ROWS
stored keys (64K by default) is
  * touched       CacheShard.touch with key bytes: new expiry and flags, in place;
  * get + store   CacheShard.lookup + gather of the same keys, then CacheShard.store of the
                  returned values under a new expiry — what a TOUCH cost before (the lookup's
                  total comes back through a pinned host slot, as in CacheShard.get).
Both are timed with device events around everything they queue (the get's host wait
included), in alternating order within a repetition, after warm-up repetitions. Prints one
JSON line: both medians (min, max), their ratio, and the bytes a touched row moves — what the
kernel reads and writes for this key length, beside the floor of 2 index lines + 48 record
bytes (header + the first key granule).
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from shellac_amd.ops.cache import CacheShard, digest_packed, item_bytes  # noqa: E402

KLEN = 48
PAYLOAD = 1024
VLEN = 2 + KLEN + PAYLOAD
STRIDE = (VLEN + 15) // 16 * 16
PREFIX = b"/bench/touch/"


def make_keys(ids: torch.Tensor):
    """Key bytes [n, KLEN] for object ids: PREFIX, 12 decimal digits of the id, '/', then 'x'."""
    n = ids.numel()
    key = torch.full((n, KLEN), ord("x"), dtype=torch.uint8, device=ids.device)
    for j, ch in enumerate(PREFIX):
        key[:, j] = ch
    d = ids.clone()
    for j in range(12):
        key[:, len(PREFIX) + 11 - j] = (ord("0") + d % 10).to(torch.uint8)
        d //= 10
    key[:, len(PREFIX) + 12] = ord("/")
    return key


def packed_keys(ids: torch.Tensor):
    """(packed key bytes, int64 offsets[n + 1], digests) of the ids' keys."""
    key = make_keys(ids).reshape(-1).contiguous()
    offs = torch.arange(ids.numel() + 1, dtype=torch.int64, device=ids.device) * KLEN
    return key, offs, digest_packed(key, offs)


def make_batch(ids: torch.Tensor):
    """A SET batch of the ids' keyed values (1 KiB payloads)."""
    dev, n = ids.device, ids.numel()
    rows = torch.full((n, STRIDE), ord("p"), dtype=torch.uint8, device=dev)
    rows[:, 0] = KLEN & 0xFF
    rows[:, 1] = KLEN >> 8
    rows[:, 2:2 + KLEN] = make_keys(ids)
    _, _, digests = packed_keys(ids)
    vlen = torch.full((n,), VLEN, dtype=torch.int32, device=dev)
    val_off = torch.arange(n, dtype=torch.int64, device=dev) * STRIDE
    values = torch.cat([rows.reshape(-1), torch.zeros(16, dtype=torch.uint8, device=dev)])
    return digests, values, val_off, vlen


def timed(fn, dev):
    a = torch.cuda.Event(enable_timing=True)
    b = torch.cuda.Event(enable_timing=True)
    a.record()
    r = fn()
    b.record()
    torch.cuda.synchronize(dev)
    return a.elapsed_time(b) * 1e3, r   # us


def summary(ts):
    ts = sorted(ts)
    return {"runs": len(ts), "median_us": round(ts[len(ts) // 2], 1), "min_us": round(ts[0], 1),
            "max_us": round(ts[-1], 1)}


def run(n: int, rows: int, iters: int, warmup: int, dev) -> dict:
    nb = 1
    while nb * 2 < n:       # <= 50 % slot load
        nb *= 2
    item = item_bytes(VLEN)
    # room for the objects and for every get + store repetition's appends: the log never
    # wraps, so no object is lost and the CLOCK hand never runs
    log_bytes = (int(n * item * 1.05) + (iters + warmup + 2) * rows * item + (64 << 20)) // 16 * 16
    shard = CacheShard(log_bytes, nb, 1 << 16, dev)
    step = 1 << 17
    shard.reserve(step)
    now = shard.now()
    for s in range(0, n, step):
        ids = torch.arange(s, min(s + step, n), dtype=torch.int64, device=dev)
        d, v, vo, vl = make_batch(ids)
        ex = torch.full((ids.numel(),), now + 1000, dtype=torch.int32, device=dev)
        shard.store(d, v, vo, vl, None, ex, now=now)
    torch.cuda.synchronize(dev)
    gen = torch.Generator(device="cpu")
    gen.manual_seed(7)
    out = torch.empty(rows * item + 64, dtype=torch.uint8, device=dev)
    vlen = torch.full((rows,), VLEN, dtype=torch.int32, device=dev)
    t_touch, t_gs = [], []
    hits = sets0 = 0
    for it in range(warmup + iters):
        ids = torch.randperm(n, generator=gen)[:rows].to(dev)
        kb, offs, d = packed_keys(ids)
        ex = torch.full((rows,), now + 2000 + it, dtype=torch.int32, device=dev)
        fl = torch.full((rows,), it, dtype=torch.int32, device=dev)
        torch.cuda.synchronize(dev)

        def touch():
            return shard.touch(d, ex, fl, (kb, offs), now=now)

        def get_store():
            lk = shard.lookup(d, now, total_slot=1)
            total = shard.host_total(1)
            shard.gather(lk, out=out, total=total)
            # (the returned records: [32-B header | value], 16-byte aligned)
            shard.store(d, out, lk.off[:rows] + 32, vlen, fl, ex, now=now,
                        bytes_bound=rows * item)
            return total

        order = (touch, get_store) if it % 2 == 0 else (get_store, touch)
        for fn in order:
            us, r = timed(fn, dev)
            if it < warmup:
                continue
            if fn is touch:
                t_touch.append(us)
                hits += int(r.sum().item())
            else:
                t_gs.append(us)
                assert r == rows * item, "a get missed stored objects"
        if it + 1 == warmup:
            sets0 = shard.counters()["set_ops"]
    assert hits == iters * rows, "a touch missed stored objects"
    assert shard.head() < log_bytes, "the log wrapped"
    ngran = (2 + KLEN + 15) // 16
    res = {
        "objects": n, "rows": rows, "key_bytes": KLEN, "value_bytes": VLEN,
        "touch": summary(t_touch), "get_store": summary(t_gs),
        "touched": shard.counters()["touched"],
        "set_ops_by_get_store": shard.counters()["set_ops"] - sets0,
        # per row: what the kernel reads from the shard (2 index lines, the record header, the
        # key's granules), what it writes there (the entry word, header expire and flags), and
        # the row's own inputs and output (digest, expiry, flags, offset, key bytes, hit)
        "touch_row_bytes": {"shard_read": 2 * 128 + 32 + 16 * ngran, "shard_written": 8 + 4 + 4,
                            "row_io": 16 + 4 + 4 + 8 + KLEN + 1,
                            "floor_2_lines_plus_48": 2 * 128 + 48},
        "get_store_row_bytes": {"gathered": item, "appended": item},
    }
    res["get_store_over_touch"] = round(res["get_store"]["median_us"] / res["touch"]["median_us"], 2)
    moved = rows * (res["touch_row_bytes"]["shard_read"] + res["touch_row_bytes"]["shard_written"]
                    + res["touch_row_bytes"]["row_io"])
    res["touch_gb_per_s"] = round(moved / res["touch"]["median_us"] / 1e3, 1)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--objects", type=int, default=1 << 20)
    ap.add_argument("--rows", type=int, default=1 << 16)
    ap.add_argument("--iters", type=int, default=24)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    if a.iters < 20:
        raise SystemExit("at least 20 repetitions")
    if not torch.cuda.is_available():
        raise SystemExit("touch_bench.py needs a GPU")
    dev = torch.device("cuda", 0)
    print(json.dumps(run(a.objects, a.rows, a.iters, a.warmup, dev)), flush=True)


if __name__ == "__main__":
    main()
