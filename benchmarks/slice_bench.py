#!/usr/bin/env python3
"""Whole-call time of a sliced GET (k_slice_plan) against the whole GET it replaces.

One CacheShard holds keyed HTTP responses ([u16 klen | key | head | body], a 128-byte head,
32-byte URL-shaped keys) of two body sizes, 64 KiB and 1 MiB. Per repetition a seeded random
batch of 256 stored keys of one size is asked for three ways, each into pinned host memory:
  * window   CacheShard.get_keyed_slices with a 4 KiB range at a random body offset per row;
  * head     CacheShard.get_keyed_slices with kSliceHead;
  * whole    CacheShard.lookup + gather of the same keys (the lookup's total comes back through
             a pinned host slot, as in CacheShard.get).
Each is timed on the host around everything it queues and the wait for it (whole-call time),
in rotating order within a repetition, after warm-up repetitions. Prints one JSON line: per
size the medians (min, max), the bytes each way delivered to the host, and the ratios.

--conditional: the stored heads carry a 40-byte ETag line (still 128 bytes in all), and two more
forms join the same rotation on the same shard, both CacheShard.get_keyed_slices with window
kind kSliceWhole and one none_match condition per row (k_slice_plan decides each row on the GPU):
  * cond_match  every row's candidate is the stored tag: 256 heads come back (304s);
  * cond_miss   no row's candidate matches: 256 whole objects come back (200s).
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from shellac_amd.ops.cache import (CacheShard, digest_packed, item_bytes,  # noqa: E402
                                   pack_slice_conds, pack_slice_specs)

KLEN = 32
HEAD_BYTES = 128
PREFIX = b"/bench/slice/"
WINDOW = 4096
ROWS = 256
ETAG = b'"0123456789abcdef0123456789abcd"'   # with "ETag: " and CR LF a 40-byte line


def make_keys(ids: torch.Tensor):
    """Key bytes [n, KLEN] for object ids: PREFIX, 12 decimal digits of the id, then 'x'."""
    n = ids.numel()
    key = torch.full((n, KLEN), ord("x"), dtype=torch.uint8, device=ids.device)
    for j, ch in enumerate(PREFIX):
        key[:, j] = ch
    d = ids.clone()
    for j in range(12):
        key[:, len(PREFIX) + 11 - j] = (ord("0") + d % 10).to(torch.uint8)
        d //= 10
    return key


def packed_keys(ids: torch.Tensor):
    key = make_keys(ids).reshape(-1).contiguous()
    offs = torch.arange(ids.numel() + 1, dtype=torch.int64, device=ids.device) * KLEN
    return key, offs, digest_packed(key, offs)


def http_head(body: int, etag: bool = False) -> bytes:
    h = b"HTTP/1.1 200 OK\r\nContent-Type: application/octet-stream\r\nContent-Length: %d\r\nX-P: " % body
    if etag:  # (a shorter Content-Type makes room for the tag's line)
        h = b"HTTP/1.1 200 OK\r\nContent-Type: text/plain\r\nContent-Length: %d\r\nETag: %s\r\nX-P: " % (
            body, ETAG)
    assert len(h) + 4 <= HEAD_BYTES
    return h + b"a" * (HEAD_BYTES - len(h) - 4) + b"\r\n\r\n"


def store_objects(shard, ids: torch.Tensor, body: int, now: int, etag: bool = False):
    """SET the ids' objects with `body` body bytes."""
    dev, n = ids.device, ids.numel()
    vlen = 2 + KLEN + HEAD_BYTES + body
    stride = (vlen + 15) // 16 * 16
    rows = torch.full((n, stride), ord("b"), dtype=torch.uint8, device=dev)
    rows[:, 0] = KLEN & 0xFF
    rows[:, 1] = KLEN >> 8
    rows[:, 2:2 + KLEN] = make_keys(ids)
    head = torch.from_numpy(np.frombuffer(http_head(body, etag), dtype=np.uint8).copy()).to(dev)
    rows[:, 2 + KLEN:2 + KLEN + HEAD_BYTES] = head
    _, _, digests = packed_keys(ids)
    values = torch.cat([rows.reshape(-1), torch.zeros(16, dtype=torch.uint8, device=dev)])
    shard.store(digests, values, torch.arange(n, dtype=torch.int64, device=dev) * stride,
                torch.full((n,), vlen, dtype=torch.int32, device=dev), None, None, now=now)
    torch.cuda.synchronize(dev)
    return vlen


def summary(ts):
    ts = sorted(ts)
    return {"runs": len(ts), "median_us": round(ts[len(ts) // 2], 1), "min_us": round(ts[0], 1),
            "max_us": round(ts[-1], 1)}


def run(objects_small: int, objects_big: int, iters: int, warmup: int, dev,
        conditional: bool = False) -> dict:
    sizes = {"64KiB": (64 << 10, objects_small, 0), "1MiB": (1 << 20, objects_big, 10 ** 9)}
    max_item = (1 << 20) + 4096
    need = sum(item_bytes(2 + KLEN + HEAD_BYTES + b) * n for b, n, _ in sizes.values())
    shard = CacheShard((int(need * 1.1) + (64 << 20)) // 16 * 16, 1 << 14, max_item, dev)
    now = shard.now()
    vlens = {}
    for name, (body, n, base) in sizes.items():
        step = max(1, (64 << 20) // body)
        for s in range(0, n, step):
            ids = base + torch.arange(s, min(s + step, n), dtype=torch.int64, device=dev)
            vlens[name] = store_objects(shard, ids, body, now, conditional)
    out = torch.empty(ROWS * item_bytes(max(vlens.values())) + 64, dtype=torch.uint8,
                      pin_memory=True)
    gen = torch.Generator(device="cpu")
    gen.manual_seed(11)
    rng = np.random.default_rng(11)
    conds = {}
    if conditional:
        sp_c = torch.from_numpy(pack_slice_specs([("whole",)] * ROWS)).to(dev)
        for form, tag in (("cond_match", ETAG), ("cond_miss", ETAG[:-2] + b'x"')):
            crow, cbytes = pack_slice_conds([("none_match", [tag])] * ROWS)
            conds[form] = (torch.from_numpy(crow.copy()).to(dev), torch.from_numpy(cbytes.copy()).to(dev))
    result = {}
    for name, (body, n, base) in sizes.items():
        ts = {"window": [], "head": [], "whole": [], **{k: [] for k in conds}}
        delivered = {}
        for it in range(warmup + iters):
            ids = base + torch.randperm(n, generator=gen)[:ROWS].to(dev)
            kb, offs, d = packed_keys(ids)
            first = rng.integers(0, body - WINDOW, ROWS)
            sp_w = torch.from_numpy(pack_slice_specs(
                [("range", int(a), int(a) + WINDOW - 1) for a in first])).to(dev)
            sp_h = torch.from_numpy(pack_slice_specs([("head",)] * ROWS)).to(dev)
            torch.cuda.synchronize(dev)

            def window():
                _, res = shard.get_keyed_slices(d, (kb, offs), sp_w, out, now=now)
                return res.tolist()

            def head():
                _, res = shard.get_keyed_slices(d, (kb, offs), sp_h, out, now=now)
                return res.tolist()

            def whole():
                lk = shard.lookup(d, now, total_slot=1)
                total = shard.host_total(1)
                shard.gather(lk, out=out, total=total)
                torch.cuda.synchronize(dev)
                return [int((lk.size[:ROWS] > 0).sum().item()), int(total)]

            def cond_match():
                _, res = shard.get_keyed_slices(d, (kb, offs), sp_c, out, now=now,
                                                conds=conds["cond_match"])
                return res.tolist()

            def cond_miss():
                _, res = shard.get_keyed_slices(d, (kb, offs), sp_c, out, now=now,
                                                conds=conds["cond_miss"])
                return res.tolist()

            fns = [window, head, whole] + ([cond_match, cond_miss] if conditional else [])
            for fn in fns[it % len(fns):] + fns[:it % len(fns)]:
                t0 = time.perf_counter()
                hits, nbytes = fn()
                us = (time.perf_counter() - t0) * 1e6
                assert hits == ROWS, (fn.__name__, hits)
                if it >= warmup:
                    ts[fn.__name__].append(us)
                    delivered[fn.__name__] = int(nbytes)
        r = {k: summary(v) for k, v in ts.items()}
        for k in r:
            r[k]["bytes"] = delivered[k]
        r["whole_over_window"] = round(r["whole"]["median_us"] / r["window"]["median_us"], 2)
        r["whole_over_head"] = round(r["whole"]["median_us"] / r["head"]["median_us"], 2)
        r["bytes_whole_over_window"] = round(delivered["whole"] / delivered["window"], 1)
        if conditional:
            r["whole_over_cond_match"] = round(r["whole"]["median_us"] / r["cond_match"]["median_us"], 2)
            r["cond_miss_over_whole"] = round(r["cond_miss"]["median_us"] / r["whole"]["median_us"], 2)
        result[name] = r
    return {"bench": "slice", "rows": ROWS, "window_bytes": WINDOW, "objects": {
        k: v[1] for k, v in sizes.items()}, "device": torch.cuda.get_device_name(dev),
        **({"conditional": True} if conditional else {}), **result}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--objects-small", type=int, default=4096)
    ap.add_argument("--objects-big", type=int, default=1024)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--conditional", action="store_true",
                    help="store an ETag in every head and time two none_match batches as well")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    print(json.dumps(run(args.objects_small, args.objects_big, args.iters, args.warmup, dev,
                         args.conditional)))


if __name__ == "__main__":
    main()
