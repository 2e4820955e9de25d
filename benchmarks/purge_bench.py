#!/usr/bin/env python3
"""GPU time of a prefix purge (k_purge_prefix) against the index-only scan (k_sweep).

One CacheShard is filled with N keyed objects ([u16 klen | key | payload], 1 KiB payloads,
URL-shaped keys of 40-80 bytes over 16 path families `/f00/` .. `/f15/`), for N = 1M and
8M by default. Timed with device events, per N:
  * sweep          k_sweep: the index-only scan (the yardstick),
  * purge_nomatch  remove_keyed_prefix of a pattern no key starts with (every live entry
                   costs the scattered read of its record's header and first granule),
  * purge_match    remove_keyed_prefix of one family, 1/16 of the objects stored. Families
                   are purged one after the other (a purge cannot be repeated), so the live
                   set shrinks by 1/16 per run; the first run (full shard) is also reported.
Each: median, min, max of the runs, the bytes the kernel must touch (32 B per index slot,
one 64-B read per live entry scanned, the further 16-B key granules of matching records)
and the bandwidth that implies. Prints one JSON line per N.

--soft: the soft purge (k_soften_prefix, soften_keyed_prefix with an expiry cap, so that a
match costs the entry's CAS and both header stores) is measured first on the same filled
shard, with the same shapes: it removes nothing, so every family run scans the full shard.
Its line ("op": "soft", the same fields; purge_match_removed holds the objects softened)
is printed before the hard purge's ("op": "hard").
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from shellac_amd._native import core  # noqa: E402
from shellac_amd.ops.cache import CacheShard, digest_packed, item_bytes  # noqa: E402

FAMILIES = 16
KEY_MIN, KEY_MAX = 40, 80
PAYLOAD = 1024
STRIDE = (2 + KEY_MAX + PAYLOAD + 15) // 16 * 16


def make_batch(ids: torch.Tensor):
    """Keyed values for object ids (on the ids' device): key = /fXX/<12 decimal digits of the
    id>/ then 'x' up to its length (40 + id % 41), payload of 1 KiB after it."""
    dev = ids.device
    n = ids.numel()
    klen = KEY_MIN + (ids * 2654435761 >> 7) % (KEY_MAX - KEY_MIN + 1)
    fam = ids % FAMILIES
    rows = torch.full((n, STRIDE), ord("p"), dtype=torch.uint8, device=dev)
    rows[:, 0] = (klen & 0xFF).to(torch.uint8)
    rows[:, 1] = (klen >> 8).to(torch.uint8)
    key = rows[:, 2:2 + KEY_MAX]
    key[:] = ord("x")
    key[:, 0] = ord("/")
    key[:, 1] = ord("f")
    key[:, 2] = (ord("0") + fam // 10).to(torch.uint8)
    key[:, 3] = (ord("0") + fam % 10).to(torch.uint8)
    key[:, 4] = ord("/")
    d = ids.clone()
    for j in range(12):
        key[:, 5 + 11 - j] = (ord("0") + d % 10).to(torch.uint8)
        d //= 10
    key[:, 17] = ord("/")
    # bytes of the key area past klen belong to the payload
    col = torch.arange(KEY_MAX, device=dev)[None, :]
    mask = col < klen[:, None]
    packed = key[mask]                                   # keys back to back
    offs = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    torch.cumsum(klen, 0, out=offs[1:])
    digests = digest_packed(packed.contiguous(), offs)
    vlen = (2 + klen + PAYLOAD).to(torch.int32)
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


def summary(ts, nbytes):
    ts = sorted(ts)
    med = ts[len(ts) // 2]
    return {"runs": len(ts), "median_us": round(med, 1), "min_us": round(ts[0], 1),
            "max_us": round(ts[-1], 1), "bytes": int(nbytes),
            "gb_per_s": round(nbytes / med / 1e3, 1)}


def run(n: int, iters: int, dev, soft: bool = False) -> list:
    nb = 1
    while nb * 2 < n:       # <= 50 % slot load
        nb *= 2
    avg_item = item_bytes(2 + (KEY_MIN + KEY_MAX) // 2 + PAYLOAD)
    log_bytes = (int(n * avg_item * 1.1) + (64 << 20)) // 16 * 16
    shard = CacheShard(log_bytes, nb, 1 << 16, dev)
    step = 1 << 17
    shard.reserve(step)
    for s in range(0, n, step):
        ids = torch.arange(s, min(s + step, n), dtype=torch.int64, device=dev)
        d, v, vo, vl = make_batch(ids)
        shard.store(d, v, vo, vl)
    torch.cuda.synchronize(dev)
    assert shard.head() < log_bytes, "the log wrapped: objects were overwritten"
    nslots = nb * 4
    c = core()
    now = shard.now()
    stream = torch.cuda.current_stream(dev).cuda_stream
    out = torch.zeros(2, dtype=torch.int64, device=dev)

    def image(prefix: bytes):
        return torch.from_numpy(np.frombuffer(c.keyed_prefix_image(prefix), np.uint8).copy()).to(dev)

    def hard(img, plen):
        shard._impl.remove_keyed_prefix(img.data_ptr(), plen, now, out.data_ptr(), stream)

    def soften(img, plen):
        shard._impl.soften_keyed_prefix(img.data_ptr(), plen, False, 0x5EEDF00D, now + 3600, now,
                                        out.data_ptr(), stream)

    nomatch = image(b"/zzz/")

    def measure(op: str, purge) -> dict:
        live0 = shard.sweep(now)[0]
        for _ in range(3):      # warm-up: code objects, caches
            shard._impl.sweep(now, stream)
            purge(nomatch, 5)
        torch.cuda.synchronize(dev)
        t_sweep = [timed(lambda: shard._impl.sweep(now, stream), dev)[0] for _ in range(iters)]
        t_nomatch = [timed(lambda: purge(nomatch, 5), dev)[0] for _ in range(iters)]
        assert int(out[0]) == 0
        t_match, removed, live = [], [], live0
        match_bytes = []
        for f in range(min(FAMILIES - 4, max(iters, 10))):
            pre = b"/f%02d/" % f
            img = image(pre)
            t_match.append(timed(lambda: purge(img, len(pre)), dev)[0])
            removed.append(int(out[0]))
            match_bytes.append(nslots * 32 + live * 64)   # (a 5-byte prefix ends in granule 0)
            if op == "hard":
                live -= removed[-1]
        res = {
            "op": op,
            "objects": n, "live": int(live0), "index_slots": nslots, "log_bytes": log_bytes,
            "sweep": summary(t_sweep, nslots * 32),
            "purge_nomatch": summary(t_nomatch, nslots * 32 + live0 * 64),
            "purge_match": summary(t_match, float(np.median(match_bytes))),
            "purge_match_first_us": round(t_match[0], 1),
            "purge_match_removed": removed,
            "purged_counter": shard.counters()["purged"],
        }
        res["nomatch_over_sweep"] = round(res["purge_nomatch"]["median_us"] / res["sweep"]["median_us"], 2)
        res["match_over_sweep"] = round(res["purge_match"]["median_us"] / res["sweep"]["median_us"], 2)
        return res

    return ([measure("soft", soften)] if soft else []) + [measure("hard", hard)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--objects", type=str, default="1048576,8388608")
    ap.add_argument("--iters", type=int, default=12)
    ap.add_argument("--soft", action="store_true",
                    help="also measure the soft purge, on the same shard, before the hard one")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("purge_bench.py needs a GPU")
    dev = torch.device("cuda", 0)
    for n in (int(x) for x in a.objects.split(",")):
        for res in run(n, a.iters, dev, a.soft):
            print(json.dumps(res), flush=True)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
