#!/usr/bin/env python3
"""GPU time of a prefix purge (k_keyed_scan<PrefixMatch, RemoveAction>) against the index-only scan (k_sweep).

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

--soft: the soft purge (k_keyed_scan<PrefixMatch, SoftenAction>, soften_keyed_prefix with an expiry cap, so that a
match costs the entry's CAS and both header stores) is measured first on the same filled
shard, with the same shapes: it removes nothing, so every family run scans the full shard.
Its line ("op": "soft", the same fields; purge_match_removed holds the objects softened)
is printed before the hard purge's ("op": "hard").

--tags: every object carries a tag block of 4 tags between its key and its payload (keyed.h:
[0x02 | 4 | 4 x u64]; one hash names the object's family, three are its own), and the purge by
tag (k_keyed_scan<TagMatch, RemoveAction> / k_keyed_scan<TagMatch, SoftenAction>) is measured beside the prefix purge on the same shard:
"op": "soft-tags" (it removes nothing) and "hard-tags", with the same fields. A tag purge of
one family's hash matches the same 1/16 of the objects as the prefix purge of that family; a
list of one hash no object carries matches nothing. All no-match runs, of every op, are timed
on the full shard before anything is removed; the hard tag purge then removes the first six
families and the hard prefix purge the next six ("match_live_first": the live objects when
its first matching run began). The yardstick of a tag op is the prefix op's line of the same N.

--list: the listing (k_list_scan / k_list_tiles / k_list_emit, HbmCache::list_keyed) is measured
on the same full shard, before anything is removed ("op": "list"): the count-only form with the
prefix no key starts with, timed in turn with the hard prefix purge of the same pattern (its
yardstick: both read the same lines; "count_over_purge" is the ratio of the medians), then a
list of one family (1/16 of the objects) with limit 100 and with the maximum (4096 rows, 128-byte
key areas).

--glob: the purge by URL glob (k_keyed_scan<GlobMatch, RemoveAction>, HbmCache::remove_keyed_glob) is measured on the same
full shard, before anything is removed ("op": "glob"), timed in turn with the hard prefix purge
that matches nothing (its yardstick, in the same run): a glob with a literal head that matches
nothing (`/nothing/*`: the head-granule reject, the prefix scan's reads), and one with a tail
only (`*.nothing`: every live record's key is read to its end). Each is also given as a ratio of
the prefix purge's median. Once every op's no-match runs are done, and before any other op
removes anything, a glob with a head, a middle and a tail (`/fXX/*/xx*x`) removes one family
(1/16 of the objects stored), in turn with the prefix purge of another family, over the four
families the other ops leave alone ("glob_match", "prefix_match", "match_live_first").
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
TAGS = 4
TAG_BLOCK = 2 + 8 * TAGS
STRIDE = (2 + KEY_MAX + TAG_BLOCK + PAYLOAD + 15) // 16 * 16
FAM_HASH = 0x0123456789ABCDEF      # family f's tag hash: (f + 1) * FAM_HASH; -1: nobody's


def fam_hash(f: int) -> int:
    return (f + 1) * FAM_HASH


def make_batch(ids: torch.Tensor, tags: bool = False):
    """Keyed values for object ids (on the ids' device): key = /fXX/<12 decimal digits of the
    id>/ then 'x' up to its length (40 + id % 41), payload of 1 KiB after it. `tags`: a tag
    block of TAGS hashes between the two: the family's at place id % TAGS, the others unique."""
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
    if tags:
        own = ids[:, None] * TAGS + torch.arange(TAGS, device=dev)[None, :] + 1
        h = own * -0x61C8864680B583EB                    # (wraps: 64 well-mixed bits)
        h[torch.arange(n, device=dev), ids % TAGS] = (fam + 1) * FAM_HASH
        blk = torch.empty((n, TAG_BLOCK), dtype=torch.uint8, device=dev)
        blk[:, 0] = 2
        blk[:, 1] = TAGS
        blk[:, 2:] = h.contiguous().view(torch.uint8).reshape(n, 8 * TAGS)
        at = (2 + klen)[:, None] + torch.arange(TAG_BLOCK, device=dev)[None, :]
        rows[torch.arange(n, device=dev)[:, None], at] = blk
        vlen = (2 + klen + TAG_BLOCK + PAYLOAD).to(torch.int32)
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


def run(n: int, iters: int, dev, soft: bool = False, tags: bool = False,
        listing: bool = False, glob: bool = False) -> list:
    nb = 1
    while nb * 2 < n:       # <= 50 % slot load
        nb *= 2
    avg_item = item_bytes(2 + (KEY_MIN + KEY_MAX) // 2 + PAYLOAD + (TAG_BLOCK if tags else 0))
    log_bytes = (int(n * avg_item * 1.1) + (64 << 20)) // 16 * 16
    shard = CacheShard(log_bytes, nb, 1 << 16, dev)
    step = 1 << 17
    shard.reserve(step)
    for s in range(0, n, step):
        ids = torch.arange(s, min(s + step, n), dtype=torch.int64, device=dev)
        d, v, vo, vl = make_batch(ids, tags)
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

    def tag_list(h: int):
        return torch.tensor([h], dtype=torch.int64, device=dev)

    def hard_tags(lst, nlist):
        shard._impl.remove_keyed_tags(lst.data_ptr(), nlist, now, out.data_ptr(), stream)

    def soften_tags(lst, nlist):
        shard._impl.soften_keyed_tags(lst.data_ptr(), nlist, 0x5EEDF00D, now + 3600, now,
                                      out.data_ptr(), stream)

    # what an op is called with: (pattern in device memory, its length) of a family / of nothing
    # and the record bytes a live entry costs: header + value granule 0 (a 5-byte prefix ends
    # there); the tag matcher reads the block's 34 bytes behind the key as well, one or two
    # more 32-B sectors, counted as 64 B
    by_prefix = (lambda f: (image(b"/f%02d/" % f), 5), (image(b"/zzz/"), 5), 64)
    by_tag = (lambda f: (tag_list(fam_hash(f)), 1), (tag_list(-1), 1), 128)

    def no_match(op: str, purge, args) -> dict:
        nomatch = args[1]
        live0 = shard.sweep(now)[0]
        for _ in range(3):      # warm-up: code objects, caches
            shard._impl.sweep(now, stream)
            purge(*nomatch)
        torch.cuda.synchronize(dev)
        t_sweep = [timed(lambda: shard._impl.sweep(now, stream), dev)[0] for _ in range(iters)]
        t_nomatch = [timed(lambda: purge(*nomatch), dev)[0] for _ in range(iters)]
        assert int(out[0]) == 0
        return {
            "op": op,
            "objects": n, "live": int(live0), "index_slots": nslots, "log_bytes": log_bytes,
            "sweep": summary(t_sweep, nslots * 32),
            "purge_nomatch": summary(t_nomatch, nslots * 32 + live0 * args[2]),
        }

    def match(res: dict, purge, args, families) -> dict:
        op = res["op"]
        live = live_first = shard.sweep(now)[0]
        t_match, removed, match_bytes = [], [], []
        for f in families:
            pat = args[0](f)
            t_match.append(timed(lambda: purge(*pat), dev)[0])
            removed.append(int(out[0]))
            match_bytes.append(nslots * 32 + live * args[2])
            if op.startswith("hard"):
                live -= removed[-1]
        res.update({
            "match_live_first": int(live_first),
            "purge_match": summary(t_match, float(np.median(match_bytes))),
            "purge_match_first_us": round(t_match[0], 1),
            "purge_match_removed": removed,
            "purged_counter": shard.counters()["purged"],
        })
        res["nomatch_over_sweep"] = round(res["purge_nomatch"]["median_us"] / res["sweep"]["median_us"], 2)
        res["match_over_sweep"] = round(res["purge_match"]["median_us"] / res["sweep"]["median_us"], 2)
        return res

    def list_runs() -> dict:
        key_cap, max_rows = 128, c.MAX_LIST_ROWS
        rows = torch.zeros((max_rows, c.LIST_ROW_BYTES), dtype=torch.uint8, device=dev)
        keys = torch.zeros((max_rows, key_cap), dtype=torch.uint8, device=dev)
        res4 = torch.zeros(4, dtype=torch.int64, device=dev)
        nomatch, fam0 = image(b"/zzz/"), image(b"/f00/")

        def lst(img, limit):
            shard._impl.list_keyed(c.LIST_PREFIX, img.data_ptr(), 5, False, 0, 0, 0, limit, key_cap,
                                   now, rows.data_ptr(), keys.data_ptr(), res4.data_ptr(), stream)

        live0 = shard.sweep(now)[0]
        for _ in range(3):
            lst(nomatch, 0)
            hard(nomatch, 5)
            lst(fam0, 100)
            lst(fam0, max_rows)
        torch.cuda.synchronize(dev)
        t_count, t_purge = [], []
        for _ in range(iters):      # in turn: the same shard state, the same neighbours
            t_count.append(timed(lambda: lst(nomatch, 0), dev)[0])
            assert res4.tolist() == [0, 0, 0, nslots]
            t_purge.append(timed(lambda: hard(nomatch, 5), dev)[0])
            assert int(out[0]) == 0
        t_100 = [timed(lambda: lst(fam0, 100), dev)[0] for _ in range(iters)]
        got_100 = res4.tolist()
        t_max = [timed(lambda: lst(fam0, max_rows), dev)[0] for _ in range(iters)]
        got_max = res4.tolist()
        assert got_100[0] == got_max[0] and got_100[2] == 100
        assert got_max[2] == min(max_rows, got_max[0])
        scan_bytes = nslots * 32 + live0 * 64
        r = {
            "op": "list", "objects": n, "live": int(live0), "index_slots": nslots,
            "purge_nomatch": summary(t_purge, scan_bytes),
            "list_count_nomatch": summary(t_count, scan_bytes + nslots // 8 + nslots // 64),
            "list_match_100": summary(t_100, scan_bytes + nslots // 4),
            "list_match_max": summary(t_max, scan_bytes + nslots // 4 + max_rows * (64 + key_cap)),
            "list_matched": got_max[0], "list_rows_max": got_max[2],
        }
        r["count_over_purge"] = round(r["list_count_nomatch"]["median_us"] /
                                      r["purge_nomatch"]["median_us"], 3)
        return r

    def glob_image(pattern: bytes):
        return torch.from_numpy(np.frombuffer(c.keyed_glob_image(pattern), np.uint8).copy()).to(dev)

    def hard_glob(img):
        shard._impl.remove_keyed_glob(img.data_ptr(), img.numel(), now, out.data_ptr(), stream)

    def glob_nomatch_runs() -> dict:
        nomatch = image(b"/zzz/")
        head, tail = glob_image(b"/nothing/*"), glob_image(b"*.nothing")
        live0 = shard.sweep(now)[0]
        for _ in range(3):
            hard(nomatch, 5)
            hard_glob(head)
            hard_glob(tail)
        torch.cuda.synchronize(dev)
        t_prefix, t_head, t_tail = [], [], []
        for _ in range(iters):      # in turn: the same shard state, the same neighbours
            for ts, fn in ((t_prefix, lambda: hard(nomatch, 5)), (t_head, lambda: hard_glob(head)),
                           (t_tail, lambda: hard_glob(tail))):
                ts.append(timed(fn, dev)[0])
                assert int(out[0]) == 0
        # a live entry costs its header and value granule 0 (64 B); the tail-only form reads
        # the key to its end: 42..82 value bytes, the record's first 128 B
        r = {
            "op": "glob", "objects": n, "live": int(live0), "index_slots": nslots,
            "purge_nomatch": summary(t_prefix, nslots * 32 + live0 * 64),
            "glob_head_nomatch": summary(t_head, nslots * 32 + live0 * 64),
            "glob_tail_nomatch": summary(t_tail, nslots * 32 + live0 * 128),
        }
        for name in ("glob_head_nomatch", "glob_tail_nomatch"):
            r[name.replace("glob_", "") + "_over_prefix"] = round(
                r[name]["median_us"] / r["purge_nomatch"]["median_us"], 3)
        return r

    def glob_match_runs(res: dict) -> dict:
        live_first = live = shard.sweep(now)[0]
        t_glob, t_prefix, removed = [], [], []
        for f in range(FAMILIES - 4, FAMILIES):
            if f % 2 == 0:
                img = glob_image(b"/f%02d/*/xx*x" % f)
                t_glob.append(timed(lambda: hard_glob(img), dev)[0])
            else:
                img = image(b"/f%02d/" % f)
                t_prefix.append(timed(lambda: hard(img, 5), dev)[0])
            removed.append(int(out[0]))
            live -= removed[-1]
        res.update({
            "match_live_first": int(live_first), "match_removed": removed,
            "glob_match": summary(t_glob, nslots * 32 + live_first * 64),
            "prefix_match": summary(t_prefix, nslots * 32 + live_first * 64),
        })
        res["match_over_prefix"] = round(res["glob_match"]["median_us"] /
                                         res["prefix_match"]["median_us"], 3)
        return res

    fams = list(range(min(FAMILIES - 4, max(iters, 10))))
    results = []
    # the soft ops remove nothing: each sees the full shard throughout
    for op, purge, args, on in (("soft", soften, by_prefix, soft),
                                ("soft-tags", soften_tags, by_tag, tags)):
        if on:
            results.append(match(no_match(op, purge, args), purge, args, fams))
    if listing:
        results.append(list_runs())
    glob_res = glob_nomatch_runs() if glob else None
    hard_ops = ([("hard-tags", hard_tags, by_tag)] if tags else []) + [("hard", hard, by_prefix)]
    # every hard op's no-match runs first, on the full shard; then the families are shared out
    pending = [(no_match(op, purge, args), purge, args) for op, purge, args in hard_ops]
    if glob:      # the first to remove: the four families the other ops leave alone
        results.append(glob_match_runs(glob_res))
    share = len(fams) // len(pending)
    for j, (res, purge, args) in enumerate(pending):
        results.append(match(res, purge, args, fams[j * share:(j + 1) * share]))
    return results


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--objects", type=str, default="1048576,8388608")
    ap.add_argument("--iters", type=int, default=12)
    ap.add_argument("--soft", action="store_true",
                    help="also measure the soft purge, on the same shard, before the hard one")
    ap.add_argument("--tags", action="store_true",
                    help="store every object with 4 tags and measure the purge by tag (soft and "
                         "hard) beside the prefix purge, on the same shard")
    ap.add_argument("--list", action="store_true",
                    help="also measure the listing (count-only and with rows) on the same full "
                         "shard, in the same run as the prefix purge that matches nothing")
    ap.add_argument("--glob", action="store_true",
                    help="also measure the purge by glob: two patterns that match nothing, in the "
                         "same run as the prefix purge that matches nothing, and one that removes "
                         "a family")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("purge_bench.py needs a GPU")
    dev = torch.device("cuda", 0)
    for n in (int(x) for x in a.objects.split(",")):
        for res in run(n, a.iters, dev, a.soft, a.tags, a.list, a.glob):
            print(json.dumps(res), flush=True)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
