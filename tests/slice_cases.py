"""Scenarios shared by tests/test_slices.py (CPU) and tests/test_slices_gpu.py: stored HTTP
responses as keyed values, a pure-Python model of the sliced GET (csrc/slice.h: where a head
ends, how a window resolves, the row and the bytes a stored value gives), and the runs both
twins (HostCache::get_keyed_slices on the CPU, k_slice_plan on the GPU) are checked with.
Every run takes explicit `now` values, so nothing here waits for a clock."""
import random
import struct

import numpy as np
import pytest
import torch

import purge_cases as pc
import tag_cases as tg
import touch_cases as tc
from shellac_amd import core
from shellac_amd.ops.cache import (digest_strings, keyed, pack_slice_specs, slice_rows, tagged,
                                   unpack_slices)

T0 = tc.T0
CRLF2 = b"\r\n\r\n"
HEAD_MAX = 64 << 10            # slice.h kSliceHeadMax
HEAD, RANGE, FROM, SUFFIX, WHOLE = "head", "range", "from", "suffix", "whole"
FLAGS = 7                      # what store() below stores every object with
M64 = 2 ** 64 - 1


# ------------------------------------------------------------------------------ the model
def find_head_end(payload):
    """Bytes of the head through the blank line, or None if the payload is not sliceable."""
    if not payload.startswith(b"HTTP/"):
        return None
    e = payload.find(CRLF2)
    if e < 0 or e + 4 > HEAD_MAX:
        return None
    return e + 4


def tag_strip(payload):
    """Bytes of the tag block in front of a payload (keyed.h parse_tag_block), 0: none."""
    if len(payload) < 2 or payload[0] != 0x02:
        return 0
    nt = payload[1]
    if nt == 0xFF:
        return 2
    if nt > 32 or 2 + 8 * nt > len(payload):
        return 0
    return 2 + 8 * nt


def layout(value):
    """(head_off, body_off) of a sliceable keyed value, else None."""
    if len(value) < 2:
        return None
    o = 2 + struct.unpack_from("<H", value)[0]
    if o > len(value):
        return None
    h = o + tag_strip(value[o:])
    n = find_head_end(value[h:])
    return None if n is None else (h, h + n)


def resolve_window(kind, a, b, body_len):
    """(satisfiable, first, length)."""
    if kind == HEAD:
        return True, 0, 0
    if body_len == 0:
        return False, 0, 0
    if kind == RANGE:
        if a >= body_len or a > b:
            return False, 0, 0
        return True, a, min(b, body_len - 1) - a + 1
    if kind == FROM:
        return (False, 0, 0) if a >= body_len else (True, a, body_len - a)
    if kind == SUFFIX:
        if a == 0:
            return False, 0, 0
        a = min(a, body_len)
        return True, body_len - a, a
    raise ValueError(kind)


def norm(spec):
    spec = tuple(spec) if isinstance(spec, (tuple, list)) else (spec,)
    return (spec + (0, 0))[:3]


def up16(x):
    return (x + 15) & ~15


def model_fields(value, spec):
    """The SliceRow (without out_off) a hit on `value` gives, and the bytes it returns."""
    kind, a, b = norm(spec)
    f = dict(status=3, vlen=len(value), head_off=0, body_off=0, body_len=0, skew=0, win_first=0,
             win_len=0, head_bytes=up16(len(value)))
    lay = None if kind == WHOLE else layout(value)
    if lay is None:
        return f, len(value)
    ho, bo = lay
    ok, first, ln = resolve_window(kind, a, b, len(value) - bo)
    f.update(status=1 if ok else 2, head_off=ho, body_off=bo, body_len=len(value) - bo,
             skew=(bo + first) & 15, win_first=first, win_len=ln, head_bytes=up16(bo))
    return f, bo + ln


def row_bytes(f):
    if f["status"] == 0:
        return 0
    return f["head_bytes"] + (up16(f["skew"] + f["win_len"]) if f["win_len"] else 0)


MISS = dict(status="miss", head=b"", window=b"", body_len=0, first=0, vlen=0, flags=0, expire=0)
MISS_FIELDS = dict(status=0, vlen=0, head_off=0, body_off=0, body_len=0, skew=0, win_first=0,
                   win_len=0, head_bytes=0)


def model_answer(value, spec, flags=FLAGS, expire=0):
    """What get_slices returns for a hit on `value`."""
    f, _ = model_fields(value, spec)
    if f["status"] == 3:
        return dict(status="whole", head=b"", window=value, body_len=0, first=0,
                    vlen=len(value), flags=flags, expire=expire)
    bo, w0 = f["body_off"], f["body_off"] + f["win_first"]
    return dict(status="ok" if f["status"] == 1 else "unsat", head=value[f["head_off"]:bo],
                window=value[w0:w0 + f["win_len"]], body_len=f["body_len"], first=f["win_first"],
                vlen=len(value), flags=flags, expire=expire)


def model(stored, keys, specs, live=None, flags=FLAGS, expire=0):
    """(answers, fields with out_off, hits, total bytes of `out`, bytes returned) of a batch
    over the dict of stored values; `live`: the keys that hit (default: all stored)."""
    ans, fields, hits, total, payload = [], [], 0, 0, 0
    for k, s in zip(keys, specs):
        if k not in stored or (live is not None and k not in live):
            ans.append(dict(MISS))
            fields.append(dict(MISS_FIELDS, out_off=total))
            continue
        f, p = model_fields(stored[k], s)
        ans.append(model_answer(stored[k], s, flags, expire))
        fields.append(dict(f, out_off=total))
        hits += 1
        total += row_bytes(f)
        payload += p
    return ans, fields, hits, total, payload


# ------------------------------------------------------------------------------- builders
def head_of(n, status=b"200 OK"):
    """An HTTP head of exactly n bytes whose only CR LF CR LF are its last four."""
    base = b"HTTP/1.1 " + status + b"\r\nX-P: "
    assert n >= len(base) + 4, n
    return base + b"a" * (n - len(base) - 4) + CRLF2


def body_of(n, seed=0):
    rng = random.Random(seed * 7919 + n)
    return bytes(rng.getrandbits(8) for _ in range(n))


def obj(key, head_len=40, body_len=50, tags=None, seed=0):
    payload = head_of(head_len) + body_of(body_len, seed)
    return keyed(key, payload if tags is None else tagged(tags, payload))


def store(sh, objs, expire=0, now=T0, digests=None):
    tc.store_at(sh, objs, expire, now=now, flags=FLAGS, digests=digests)


def shards_for(devices, objs=None, **kw):
    kw.setdefault("max_item", 8192)
    shards = [pc.make_shard(d, **kw) for d in devices]
    for sh in shards:
        if objs:
            store(sh, objs)
    return shards


def slices(sh, keys, specs, now=T0, digest_of=None, reserve=0, cap=None, fill=0):
    """One get_keyed_slices call -> (answers, row fields, [hits, total], out as numpy).
    `digest_of`: the keys whose digests the rows carry (a forged collision). `cap`: the
    response buffer's bytes (default: ample), prefilled with `fill`."""
    keys = list(keys)
    d = digest_strings(digest_of if digest_of is not None else keys, sh.device)
    kb = tc.key_tensors(keys, sh.device)
    sp = torch.from_numpy(pack_slice_specs(specs).reshape(len(keys), 24)).to(sh.device)
    if cap is None:
        cap = 64 + sum(2 * 8192 + 64 for _ in keys)
    out = torch.full((max(cap, 16),), fill, dtype=torch.uint8, device=sh.device)[:cap]
    rows, res = sh.get_keyed_slices(d, kb, sp, out, now=now, reserve_bytes=reserve)
    res = [int(x) for x in res.tolist()]               # (waits for the stream)
    fields = slice_rows(rows)
    ans = unpack_slices(rows, out) if res[1] <= cap else None
    return ans, fields, res, out.cpu().numpy()


def check(sh, stored, keys, specs, now=T0, live=None, expire=0):
    """A batch on `sh` gives the model's rows, bytes and totals, and counts as a GET counts."""
    keys, specs = list(keys), list(specs)
    want, wfields, hits, total, payload = model(stored, keys, specs, live, expire=expire)
    c0 = sh.counters()
    ans, fields, res, _ = slices(sh, keys, specs, now)
    c1 = sh.counters()
    assert res == [hits, total], (sh.device, res, hits, total)
    for i, (g, w) in enumerate(zip(fields, wfields)):
        g = {k: g[k] for k in w}
        assert g == w, (sh.device, i, keys[i], specs[i], g, w)
    for i, (g, w) in enumerate(zip(ans, want)):
        assert g == w, (sh.device, i, keys[i], specs[i])
    assert c1["get_ops"] - c0["get_ops"] == len(keys)
    assert c1["get_hits"] - c0["get_hits"] == hits
    assert c1["get_bytes"] - c0["get_bytes"] == payload
    return ans


def window_specs(body_len):
    """Every kind at the edges of a body of body_len bytes."""
    pts = sorted({0, 1, max(body_len - 1, 0), body_len, body_len + 1})
    specs = [(HEAD,), (WHOLE,)]
    for a in pts:
        specs += [(FROM, a), (SUFFIX, a)]
        specs += [(RANGE, a, b) for b in pts]
    specs += [(RANGE, 5, 2), (RANGE, 0, M64), (SUFFIX, M64), (FROM, M64), (RANGE, M64, M64)]
    return specs


BODY_LENS = [0, 1, 15, 16, 17, 1023, 1024, 1025]


# ----------------------------------------------------------------------------------- runs
def run_resolve_window():
    """slice.h resolve_window against the model, every kind at every edge."""
    c = core()
    kinds = {HEAD: c.SLICE_HEAD, RANGE: c.SLICE_RANGE, FROM: c.SLICE_FROM, SUFFIX: c.SLICE_SUFFIX}
    n = 0
    for bl in BODY_LENS:
        for s in window_specs(bl):
            kind, a, b = norm(s)
            if kind == WHOLE:
                continue
            assert tuple(c.resolve_window(kinds[kind], a, b, bl)) == resolve_window(kind, a, b, bl), \
                (s, bl)
            n += 1
    assert n > 200
    # the layout of a value, against the model's
    for v in [obj(b"/k", 40, 10), obj(b"/k", 40, 0), keyed(b"/k", b"HTTP/1.1 200 OK\n\n"),
              obj(b"/k", 40, 10, tags=[b"a", b"b"]), keyed(b"/k", b"\x01accept-encoding"), b"", b"\x05"]:
        got = c.slice_layout(v)
        assert (None if got is None else tuple(got)) == layout(v), v


def run_windows(devices):
    """Every window form over bodies of BODY_LENS bytes, each body twice so that its first
    byte falls on two alignments."""
    objs, keys, specs = {}, [], []
    for bl in BODY_LENS:
        for hl in (40, 53):
            k = b"/w/%d/%d" % (bl, hl)
            objs[k] = obj(k, hl, bl, seed=hl)
            for s in window_specs(bl):
                keys.append(k)
                specs.append(s)
    for sh in shards_for(devices, objs):
        ans = check(sh, objs, keys, specs)
        assert {a["status"] for a in ans} == {"ok", "unsat", "whole"}


def seam_objects():
    """Heads whose CR LF CR LF starts at value offsets 13..16 mod 16, and 1021..1024 and
    2045..2048 bytes past the granule the search starts in (the wave-pass seams), for search
    starts of several alignments."""
    objs = {}
    for klen in (1, 6, 13, 14, 30):
        head_off = 2 + klen
        start = head_off & ~15
        for at in [16 * 4 + r for r in (13, 14, 15, 16)] + [1021, 1022, 1023, 1024, 2045, 2046,
                                                            2047, 2048]:
            n = start + at - head_off + 4          # the terminator starts at value byte start + at
            k = (bytes([65 + len(objs) % 12]) + b"/seam/key/padded/to/its/length")[:klen]
            assert len(k) == klen and k not in objs
            objs[k] = keyed(k, head_of(n) + body_of(37, n))
            assert layout(objs[k]) == (head_off, start + at + 4)
    return objs


def run_seams(devices):
    objs = seam_objects()
    keys = list(objs)
    for sh in shards_for(devices, objs, nbuckets=256):
        for spec in [(HEAD,), (RANGE, 0, 0), (SUFFIX, 5), (FROM, 36), (RANGE, 3, 18)]:
            check(sh, objs, keys, [spec] * len(keys))


def run_klens(devices):
    """klen 1..40: head_off takes every alignment; windows of length 1, ending on and across
    granule edges, the whole body, a suffix longer than the body."""
    objs = {}
    for klen in range(1, 41):
        k = tg.key_of_len(klen, klen)
        objs[k] = obj(k, 30 + 3 * klen, 100, seed=klen)
    keys = list(objs)
    for sh in shards_for(devices, objs, nbuckets=64):
        for spec in [(RANGE, 0, 0), (RANGE, 99, 99), (RANGE, 7, 15), (RANGE, 7, 16), (RANGE, 0, 99),
                     (FROM, 0), (SUFFIX, 1000), (SUFFIX, 1), (RANGE, 16, 47), (HEAD,), (WHOLE,)]:
            check(sh, objs, keys, [spec] * len(keys))


def run_tag_forms(devices):
    """Tag blocks of 0, 1 and 32 tags and the overflow block; a tag hash whose bytes are CR LF
    CR LF, and a key that contains them (neither ends the head); a malformed block."""
    pay = head_of(45) + body_of(60)
    crlf_hash = core().tag_block([0x0A0D0A0D0A0D0A0D])
    objs = {
        b"/t/0": keyed(b"/t/0", pay),
        b"/t/1": keyed(b"/t/1", tagged([b"one"], pay)),
        b"/t/32": keyed(b"/t/32", tagged([b"t%d" % i for i in range(32)], pay)),
        b"/t/over": keyed(b"/t/over", tagged([b"t%d" % i for i in range(33)], pay)),
        b"/t/crlf-hash": keyed(b"/t/crlf-hash", crlf_hash + pay),
        b"/t/\r\n\r\n/key": keyed(b"/t/\r\n\r\n/key", pay),
        b"/t/malformed": keyed(b"/t/malformed", b"\x02\x28" + pay),          # 40 tags: no block
        b"/t/truncated": keyed(b"/t/truncated", b"\x02\x05" + b"x" * 20),
        b"/t/tags-then-garbage": keyed(b"/t/tags-then-garbage", tagged([b"a"], b"not http")),
    }
    assert layout(objs[b"/t/crlf-hash"]) == (2 + 12 + 10, 2 + 12 + 10 + 45)
    assert layout(objs[b"/t/\r\n\r\n/key"])[0] == 2 + 11
    assert layout(objs[b"/t/malformed"]) is None
    keys = list(objs)
    for sh in shards_for(devices, objs, nbuckets=64):
        for spec in [(RANGE, 2, 30), (HEAD,), (SUFFIX, 9)]:
            ans = check(sh, objs, keys, [spec] * len(keys))
            assert [a["status"] for a in ans] == ["ok"] * 6 + ["whole"] * 3


def run_unsliceable(devices):
    """LF LF only, no terminator, a terminator at the very end (an empty body), a Vary marker
    and garbage: whole objects, except the empty body."""
    rng = random.Random(3)
    objs = {
        b"/u/lflf": keyed(b"/u/lflf", b"HTTP/1.1 200 OK\nA: b\n\nbody"),
        b"/u/none": keyed(b"/u/none", b"HTTP/1.1 200 OK\r\nA: b\r\n" + b"x" * 300),
        b"/u/cr-lf-cr": keyed(b"/u/cr-lf-cr", b"HTTP/1.1 200 OK\r\n\r"),
        b"/u/end": keyed(b"/u/end", head_of(48)),
        b"/u/vary": keyed(b"/u/vary", tg.VARY_MARKER),
        b"/u/empty": keyed(b"/u/empty", b""),
        b"/u/http": keyed(b"/u/http", b"HTTP"),
        b"/u/http5": keyed(b"/u/http5", b"HTTP/"),
        b"/u/lower": keyed(b"/u/lower", b"http/1.1 200 OK\r\n\r\nbody"),
        b"/u/shifted": keyed(b"/u/shifted", b" HTTP/1.1 200 OK\r\n\r\nbody"),
    }
    for i in range(20):
        k = b"/u/garbage/%d" % i
        objs[k] = keyed(k, bytes(rng.getrandbits(8) for _ in range(rng.randint(0, 600))))
    keys = list(objs)
    for sh in shards_for(devices, objs, nbuckets=64):
        for spec in [(RANGE, 0, 10), (HEAD,), (SUFFIX, 3), (FROM, 0)]:
            ans = check(sh, objs, keys, [spec] * len(keys))
            by = dict(zip(keys, ans))
            assert by[b"/u/end"]["status"] == ("ok" if spec == (HEAD,) else "unsat")
            assert by[b"/u/end"]["body_len"] == 0 and by[b"/u/end"]["head"] == head_of(48)
            assert all(a["status"] == "whole" for k, a in by.items() if k != b"/u/end")
    # values that are no keyed values of their keys (what garbage under a digest gives): misses
    junk = {b"/j/%d" % i: v for i, v in enumerate(pc.garbage_values())}
    for sh in shards_for(devices, junk, nbuckets=64):
        ans, fields, res, _ = slices(sh, list(junk), [(RANGE, 0, 5)] * len(junk))
        assert res == [0, 0] and all(a == MISS for a in ans)


def run_long_heads(devices):
    """Heads at and past kSliceHeadMax on a shard whose max_item allows them: e + 4 ==
    kSliceHeadMax is the last sliceable one."""
    objs = {}
    for n in (HEAD_MAX - 1, HEAD_MAX, HEAD_MAX + 1, HEAD_MAX + 700):
        k = b"/long/%d" % n
        objs[k] = keyed(k, head_of(n) + body_of(100, n))
    keys = list(objs)
    for sh in shards_for(devices, objs, nbuckets=8, max_item=1 << 17, log_bytes=1 << 20):
        d = digest_strings(keys, sh.device)
        kb = tc.key_tensors(keys, sh.device)
        specs = [(RANGE, 10, 19)] * len(keys)
        sp = torch.from_numpy(pack_slice_specs(specs)).to(sh.device)
        out = torch.zeros(1 << 19, dtype=torch.uint8, device=sh.device)
        rows, res = sh.get_keyed_slices(d, kb, sp, out, now=T0)
        want, wfields, hits, total, _ = model(objs, keys, specs)
        assert [int(x) for x in res.tolist()] == [hits, total]
        assert unpack_slices(rows, out) == want
        assert [f["status"] for f in slice_rows(rows)] == [1, 1, 3, 3]


def run_mixed_batch(devices):
    """kSliceWhole mixed into a batch, duplicate keys, misses."""
    objs = {b"/m/%d" % i: obj(b"/m/%d" % i, 40 + i, 30 + 5 * i, seed=i) for i in range(12)}
    rng = random.Random(9)
    keys, specs = [], []
    for i in range(150):
        keys.append(rng.choice(list(objs) + [b"/m/missing/%d" % (i % 7)]))
        specs.append(rng.choice([(WHOLE,), (HEAD,), (RANGE, rng.randint(0, 40), rng.randint(0, 90)),
                                 (FROM, rng.randint(0, 100)), (SUFFIX, rng.randint(0, 100))]))
    for sh in shards_for(devices, objs, nbuckets=16):
        ans = check(sh, objs, keys, specs)
        assert {a["status"] for a in ans} == {"miss", "ok", "unsat", "whole"}


def run_collision(devices):
    """A value keyed with B under A's digest, and an index entry with A's digest that points
    at B's record (debug_set_entry): a row for A is a miss either way, and B's record, asked for
    under A's digest with B's key bytes, is served."""
    a, b, c = b"/victim/object", b"/attacker/object", b"/bystander"
    for sh in shards_for(devices, None, nbuckets=64):
        vb = obj(b, 40, 20)
        store(sh, {b: vb}, digests={b: a})
        ans, _, res, _ = slices(sh, [a], [(RANGE, 0, 3)])
        assert res == [0, 0] and ans == [MISS]
        ans, _, res, _ = slices(sh, [b], [(RANGE, 0, 3)], digest_of=[a])
        assert res[0] == 1 and ans == [model_answer(vb, (RANGE, 0, 3))]
        # an entry of C's digest pointing at a record that carries another digest
        lo, hi = (int(x) & M64 for x in digest_strings([c], "cpu")[0])
        la, ha = (int(x) & M64 for x in digest_strings([a], "cpu")[0])
        b1, _ = core().bucket_pair(la, ha, sh.nbuckets)
        e = sh._impl.debug_bucket(b1)
        i = next(k for k in range(4) if e[4 * k] == la and e[4 * k + 1] == ha and e[4 * k + 2])
        c1, _ = core().bucket_pair(lo, hi, sh.nbuckets)
        free = [k for k in range(4) if sh._impl.debug_bucket(c1)[4 * k + 2] == 0]
        sh._impl.debug_set_entry(c1, free[0], lo, hi, e[4 * i + 2], e[4 * i + 3] & 0x7FFFFFFF, 0)
        ans, _, res, _ = slices(sh, [c], [(RANGE, 0, 3)])
        assert res == [0, 0] and ans == [MISS]


def run_expired(devices):
    objs = {b"/e/%d" % i: obj(b"/e/%d" % i, 40, 30, seed=i) for i in range(10)}
    keys = list(objs)
    for sh in shards_for(devices, None, nbuckets=64):
        store(sh, objs, expire=T0 + 100)
        check(sh, objs, keys, [(RANGE, 1, 9)] * len(keys), now=T0 + 99, expire=T0 + 100)
        check(sh, objs, keys, [(RANGE, 1, 9)] * len(keys), now=T0 + 100, live=set())


def run_out_cap(devices):
    """A response buffer that is too small: `out` is untouched, rows and totals are complete;
    one of exactly the total's bytes is filled."""
    objs = {b"/c/%d" % i: obj(b"/c/%d" % i, 40 + i, 200, seed=i) for i in range(20)}
    keys = list(objs) + [b"/c/missing"]
    specs = [(RANGE, i, 3 * i + 20) for i in range(len(keys))]
    want, wfields, hits, total, _ = model(objs, keys, specs)
    for sh in shards_for(devices, objs, nbuckets=64):
        for cap in (0, 16, total - 16):
            ans, fields, res, out = slices(sh, keys, specs, cap=cap, fill=0xAB)
            assert res == [hits, total] and ans is None
            assert (out == 0xAB).all(), (sh.device, cap)
            assert [{k: f[k] for k in w} for f, w in zip(fields, wfields)] == wfields
        ans, fields, res, out = slices(sh, keys, specs, cap=total, fill=0xAB)
        assert res == [hits, total] and ans == want


def run_after_the_log_lapped(devices):
    """After SET batches lapped the log: every row is the model's answer for an object that
    still hits, and a miss for one that was overwritten."""
    objs = {b"/lap/%d" % i: obj(b"/lap/%d" % i, 40 + i % 30, 300, seed=i) for i in range(300)}
    keys = list(objs)
    for sh in shards_for(devices, None, nbuckets=1 << 10, log_bytes=1 << 19, evict="fifo"):
        store(sh, objs)
        tg.lap_the_log(sh, laps=0.75, now=T0)
        live = set(tc.live_at(sh, objs, T0))
        assert 0 < len(live) < len(objs), len(live)
        check(sh, objs, keys, [(RANGE, 5, 50)] * len(keys), live=live)
        tg.lap_the_log(sh, laps=0.5, now=T0)
        assert tc.live_at(sh, objs, T0) == set()
        check(sh, objs, keys, [(HEAD,)] * len(keys), live=set())


def referenced(sh, key, now=T0):
    rows = sh.list_keyed(prefix=key, exact=True, now=now)["rows"]
    assert len(rows) == 1, (key, rows)
    return rows[0]["referenced"]


def run_reference_bit(devices):
    """A slice hit sets the CLOCK reference bit, as a GET hit does; a miss (no such key, or a
    digest collision) sets none."""
    a, b = b"/ref/a", b"/ref/b"
    objs = {a: obj(a), b: obj(b)}
    for sh in shards_for(devices, objs, nbuckets=64):
        assert not referenced(sh, a) and not referenced(sh, b)
        slices(sh, [b"/ref/missing"], [(HEAD,)])
        slices(sh, [b"/ref/x"], [(HEAD,)], digest_of=[b])      # b's digest, another key: a miss
        assert not referenced(sh, a) and not referenced(sh, b)
        slices(sh, [a], [(RANGE, 0, 0)])
        assert referenced(sh, a) and not referenced(sh, b)
        slices(sh, [b], [(WHOLE,)])
        assert referenced(sh, b)


def run_batch_sizes(devices):
    """An empty batch, one row, and 65 rows (more than one workgroup's waves)."""
    objs = {b"/n/%d" % i: obj(b"/n/%d" % i, 40 + i, 64 + i, seed=i) for i in range(65)}
    keys = list(objs)
    for sh in shards_for(devices, objs, nbuckets=64):
        ans, fields, res, _ = slices(sh, [], [])
        assert ans == [] and fields == [] and res == [0, 0]
        assert sh.get_slices([], []) == []
        check(sh, objs, keys[:1], [(SUFFIX, 9)])
        check(sh, objs, keys, [(RANGE, i, 2 * i) for i in range(65)])


def run_get_slices(devices):
    """The byte-string front end: the same answers, a response buffer that grows, and an
    explicit one that is too small."""
    objs = {b"/g/%d" % i: obj(b"/g/%d" % i, 60, 3000, seed=i) for i in range(8)}
    keys = list(objs) + [b"/g/missing"]
    specs = [(RANGE, 0, 99), (FROM, 2990), (SUFFIX, 7), (HEAD,), (WHOLE,), (RANGE, 5000, 6000),
             (RANGE, 0, 99999), (RANGE, 0, 0), (HEAD,)]
    want = model(objs, keys, specs)[0]
    for sh in shards_for(devices, objs, nbuckets=64):
        assert sh.get_slices(keys, specs, now=T0) == want
        many = keys * 60
        assert sh.get_slices(many, [(WHOLE,)] * len(many), now=T0) == \
            model(objs, many, [(WHOLE,)] * len(many))[0]          # > 1 MiB: the buffer grows
        with pytest.raises(ValueError):
            sh.get_slices(keys, specs, now=T0, out_cap=64)
        with pytest.raises(ValueError):
            sh.get_slices(keys, specs[:-1], now=T0)


# ---------------------------------------------------------------------------------- tiers
def backend_payloads():
    """{key: payload as a tier stores it}: plain and tagged responses, an empty body, a Vary
    marker, garbage."""
    return {
        b"/p/plain": head_of(60) + body_of(500, 1),
        b"/p/tagged": tagged([b"a", b"b"], head_of(47) + body_of(333, 2)),
        b"/p/overflow": tagged([b"t%d" % i for i in range(40)], head_of(30) + body_of(64, 3)),
        b"/p/empty-body": head_of(52),
        b"/p/vary": tg.VARY_MARKER,
        b"/p/garbage": b"not an http response at all",
        b"/p/big": head_of(200) + body_of(40000, 4),
    }


def model_part(payload, spec, flags=FLAGS):
    """What CacheBackend.get_parts answers for a hit on `payload` (ttl left out)."""
    kind, a, b = norm(spec)
    strip = tag_strip(payload)
    n = None if kind == WHOLE else find_head_end(payload[strip:])
    if n is None:
        return dict(status=3, head=b"", window=payload, body_len=0, first=0, flags=flags)
    body = payload[strip + n:]
    ok, first, ln = resolve_window(kind, a, b, len(body))
    return dict(status=1 if ok else 2, head=payload[strip:strip + n],
                window=body[first:first + ln], body_len=len(body), first=first, flags=flags)


PART_MISS = dict(status=0, head=b"", window=b"", body_len=0, first=0, flags=0)
PART_SPECS = [(RANGE, 0, 0), (RANGE, 5, 20), (FROM, 30), (SUFFIX, 7), (RANGE, 0, 99999), (HEAD,),
              (WHOLE,), (RANGE, 99999, 100000), (SUFFIX, 0), (RANGE, 16, 31)]


def parts(be, keys, specs, digest_of=None):
    from shellac_amd.ops.cache import SLICE_KINDS
    nums = [(SLICE_KINDS[norm(s)[0]],) + norm(s)[1:] for s in specs]
    got = be.get_parts(list(keys), nums, digest_of=digest_of)
    for g in got:
        g.pop("ttl")
    return got


def run_backend_parts(be, settle=lambda keys: None, ttl=0):
    """get_part on a tier: every kind over every payload form, a miss, and a batch that mixes
    them, against the model."""
    objs = backend_payloads()
    for k, v in objs.items():
        be.set(k, v, FLAGS, ttl)
    settle(list(objs))
    keys = list(objs) + [b"/p/missing"]
    for spec in PART_SPECS:
        got = parts(be, keys, [spec] * len(keys))
        want = [model_part(objs[k], spec) if k in objs else PART_MISS for k in keys]
        for k, g, w in zip(keys, got, want):
            assert g == w, (k, spec)
    mixed_keys = [keys[i % len(keys)] for i in range(64)]
    mixed = [PART_SPECS[(i * 7) % len(PART_SPECS)] for i in range(64)]
    got = parts(be, mixed_keys, mixed)
    want = [model_part(objs[k], s) if k in objs else PART_MISS for k, s in zip(mixed_keys, mixed)]
    assert got == want
    return objs


# ---------------------------------------------------------------------------------- proxy
class RangeOrigin:
    """An origin with deterministic bodies per path that says `Accept-Ranges: bytes`, counts
    its requests per (method, path), and ignores Range itself. /vary/*: one variant per
    User-Agent; /gz/*: gzip-coded for a client that asks for it; /teapot/*: a cacheable 203."""

    def __init__(self):
        import gzip
        import threading
        from collections import Counter
        from http.server import BaseHTTPRequestHandler, ThreadingHTTPServer
        self.hits = Counter()
        outer = self

        class H(BaseHTTPRequestHandler):
            protocol_version = "HTTP/1.1"
            disable_nagle_algorithm = True

            def log_message(self, *a):
                pass

            def _reply(self, head):
                outer.hits[(self.command, self.path)] += 1
                body = outer.body(self.path, self.headers.get("User-Agent"))
                self.send_response(203 if self.path.startswith("/teapot/") else 200)
                self.send_header("Content-Type", "application/octet-stream")
                self.send_header("Accept-Ranges", "bytes")
                self.send_header("Cache-Control", "max-age=600")
                if self.path.startswith("/vary/"):
                    self.send_header("Vary", "User-Agent")
                if self.path.startswith("/gz/") and "gzip" in (self.headers.get("Accept-Encoding") or ""):
                    body = gzip.compress(body)
                    self.send_header("Content-Encoding", "gzip")
                self.send_header("Content-Length", str(len(body)))
                self.end_headers()
                if not head:
                    self.wfile.write(body)

            def do_GET(self):
                self._reply(False)

            def do_HEAD(self):
                self._reply(True)

        class S(ThreadingHTTPServer):
            daemon_threads = True
            allow_reuse_address = True

        self._srv = S(("127.0.0.1", 0), H)
        self.port = self._srv.server_address[1]
        self._th = threading.Thread(target=self._srv.serve_forever, daemon=True)

    @staticmethod
    def body(path, ua=None):
        seed = sum(path.encode()) + (sum(ua.encode()) if ua and path.startswith("/vary/") else 0)
        return b"<" + path.encode() + b">" + body_of(1000 + seed % 97, seed)

    def start(self):
        self._th.start()
        return self

    def stop(self):
        self._srv.shutdown()
        self._srv.server_close()


def fetch(c, path, headers=None, method="GET"):
    r = c.get(path, headers=headers or {}, method=method)
    h = {k.lower(): v for k, v in r.headers().items()}
    return r.status(), h, r.body().read()


def proxy_partial_round_trip(px, origin, settle=lambda paths: None):
    """--partial-hits over any tier: 206 for every single-range form, 416, the forms that
    ignore the header, HEAD hit and miss, a Vary'd URL, pipelined order, and the counters.
    `settle(paths)` runs after a fill (an asynchronous tier stores it a moment after the
    response)."""
    from shellac_amd.utils.httpclient import HttpClient
    c = HttpClient(port=px.port)
    full = RangeOrigin.body("/r/1")
    n = len(full)
    st, h, b = fetch(c, "/r/1", {"Range": "bytes=0-9"})       # a miss: answered in full
    assert (st, b) == (200, full) and h.get("accept-ranges") == "bytes"
    settle(["/r/1"])
    st, h, b = fetch(c, "/r/1")
    assert (st, b) == (200, full) and origin.hits[("GET", "/r/1")] == 1
    assert h.get("accept-ranges") == "bytes"                  # the fill kept it
    for rg, (a, z) in {"bytes=0-0": (0, 0), "bytes=5-": (5, n - 1), "bytes=-7": (n - 7, n - 1),
                       "bytes=0-99999": (0, n - 1), "bytes=16-47": (16, 47),
                       "bytes=%d-%d" % (n - 1, n - 1): (n - 1, n - 1)}.items():
        st, h, b = fetch(c, "/r/1", {"Range": rg})
        assert st == 206 and b == full[a:z + 1], (rg, st, len(b))
        assert h["content-range"] == "bytes %d-%d/%d" % (a, z, n), (rg, h)
        assert h["content-length"] == str(z - a + 1) and h["content-type"] == "application/octet-stream"
    for rg in ("bytes=%d-" % n, "bytes=99999-100000", "bytes=-0"):
        st, h, b = fetch(c, "/r/1", {"Range": rg})
        assert (st, b) == (416, b"") and h["content-range"] == "bytes */%d" % n, (rg, st, h)
    for hdr in ({"Range": "bytes=0-1,3-4"}, {"Range": "bytes=0-1", "If-Range": '"x"'},
                {"Range": "items=0-1"}, {"Range": "bytes=5-2"}, {"Range": "bytes=abc"}):
        st, h, b = fetch(c, "/r/1", hdr)
        assert (st, b) == (200, full) and "content-range" not in h, hdr
    # HEAD: a hit is the stored head without a body, the origin is not contacted; a miss is
    # forwarded and not cached
    st, h, b = fetch(c, "/r/1", method="HEAD")
    assert (st, b) == (200, b"") and h["content-length"] == str(n)
    assert "content-range" not in h and origin.hits[("HEAD", "/r/1")] == 0
    st, h, b = fetch(c, "/r/never", method="HEAD")
    assert (st, b) == (200, b"") and origin.hits[("HEAD", "/r/never")] == 1
    assert h["content-length"] == str(len(RangeOrigin.body("/r/never")))
    assert fetch(c, "/r/never", method="HEAD")[0] == 200 and origin.hits[("HEAD", "/r/never")] == 2
    assert origin.hits[("GET", "/r/never")] == 0
    # a Vary'd URL: the variant of this request is cut, another one is a miss
    va, vb = RangeOrigin.body("/vary/1", "ua-a"), RangeOrigin.body("/vary/1", "ua-b")
    assert fetch(c, "/vary/1", {"User-Agent": "ua-a"})[2] == va
    settle(["/vary/1"])
    st, h, b = fetch(c, "/vary/1", {"User-Agent": "ua-a", "Range": "bytes=3-40"})
    assert st == 206 and b == va[3:41] and h["content-range"] == "bytes 3-40/%d" % len(va)
    st, h, b = fetch(c, "/vary/1", {"User-Agent": "ua-a"}, method="HEAD")
    assert st == 200 and h["content-length"] == str(len(va))
    assert origin.hits[("HEAD", "/vary/1")] == 0
    st, h, b = fetch(c, "/vary/1", {"User-Agent": "ua-b", "Range": "bytes=3-40"})
    assert (st, b) == (200, vb) and origin.hits[("GET", "/vary/1")] == 2
    # pipelined: the answers come back in request order
    reqs = [("/r/1", {"Range": "bytes=1-3"}), ("/r/1", {}), ("/r/1", {"Range": "bytes=-2"}),
            ("/r/miss-in-between", {}), ("/r/1", {"Range": "bytes=%d-" % n}),
            ("/r/1", {"Range": "bytes=7-7"})]
    c.send(b"".join(HttpClient.request_bytes(p, headers=hd) for p, hd in reqs))
    got = [c.read_response() for _ in reqs]
    assert [r.status() for r in got] == [206, 200, 206, 200, 416, 206]
    assert [r.body().read() for r in got] == [full[1:4], full, full[-2:],
                                              RangeOrigin.body("/r/miss-in-between"), b"", full[7:8]]
    st = px.stats()
    assert st["range_206"] == 6 + 1 + 3 and st["range_416"] == 3 + 1 and st["head_hits"] == 2
    assert st["range_requests"] == 1 + 6 + 3 + 2 + 4 and st["partial_fallbacks"] == 0
    assert origin.hits[("GET", "/r/1")] == 1
    c.close()
    return st
