"""Scenarios shared by tests/test_list.py (CPU) and tests/test_list_gpu.py: a Python model of
the listing (which stored values match, and what a row must say about each), and the runs the
twins (HostCache on the CPU, k_list_scan / k_list_emit on the GPU) are checked with. Every
shard is compared with the model of what it holds itself, as sets keyed by key bytes: slot
numbers differ between the twins. Every run takes explicit `now` values. Then the runners of
the tiers' list_objects and of the proxy's GET /_shellac/objects and PURGE dry run."""
import json
import struct
import threading

import purge_cases as pc
import soften_cases as sc
import tag_cases as tg
import touch_cases as tc
from shellac_amd.ops.cache import digest_strings, item_bytes, keyed, pack_values, tag_hash, tagged

T0, TTL0 = tc.T0, tc.TTL0
MAX_ROWS = 4096
OVERFLOW = 0xFF


# ---- the model
def key_of(value):
    """The key a stored value carries as a keyed value, or None if it is not one."""
    if len(value) < 2:
        return None
    klen = struct.unpack("<H", value[:2])[0]
    return value[2:2 + klen] if 2 + klen <= len(value) else None


def ntags_of(value):
    """ListRow::ntags of a keyed value: 0 (no or malformed block), n, or 0xff (overflow)."""
    o = 2 + struct.unpack("<H", value[:2])[0]
    if o + 2 > len(value) or value[o] != 0x02:
        return 0
    nt = value[o + 1]
    if nt == OVERFLOW:
        return OVERFLOW
    return 0 if nt > 32 or o + 2 + 8 * nt > len(value) else nt


def value_listed(value, prefix=None, tags=None, exact=False):
    key = key_of(value)
    if key is None:
        return False
    if prefix is not None:
        return key == prefix if exact else key.startswith(prefix)
    if tags is not None:
        return tg.value_matches(value, {tag_hash(t) for t in tags})
    return len(key) >= 1


def model_rows(records, key_cap=256, **query):
    """{(key bytes as listed, klen): (vlen, expire, flags, ntags, truncated)} and the item
    bytes of the records ({stored-under key: (value, flags, expire)}) the query matches."""
    want, nbytes = {}, 0
    for value, flags, expire in records.values():
        if not value_listed(value, **query):
            continue
        key = key_of(value)
        ident = (key[:key_cap - 2], len(key))
        assert ident not in want, "the scenario's keys must stay distinct when cut"
        want[ident] = (len(value), expire, flags, ntags_of(value), len(key) > key_cap - 2)
        nbytes += item_bytes(len(value))
    return want, nbytes


def rows_view(rows):
    return {(r["key"], r["klen"]): (r["vlen"], r["expire"], r["flags"], r["ntags"], r["truncated"])
            for r in rows}


def assert_slot_order(rows, nslots):
    slots = [r["slot"] for r in rows]
    assert all(a < b for a, b in zip(slots, slots[1:])), "slots must ascend strictly"
    assert all(0 <= s < nslots for s in slots)
    assert not any(r["changed"] for r in rows), "no row may be flagged in a stream-ordered run"


def check_list(sh, objs, now, key_cap=1024, **query):
    """One listing of everything the query matches on `sh`, against the model of what `sh`
    holds at `now`. Returns the rows."""
    records = tc.records_at(sh, objs, now)
    want, want_bytes = model_rows(records, key_cap, **query)
    r = sh.list_keyed(limit=MAX_ROWS, key_cap=key_cap, now=now, **query)
    assert (r["matched"], r["bytes"], r["next"]) == (len(want), want_bytes, None), \
        (sh.device, query, r["matched"], len(want))
    assert_slot_order(r["rows"], 4 * sh.nbuckets)
    assert len(r["rows"]) == len(want)
    assert rows_view(r["rows"]) == want, (sh.device, query)
    # the count-only form
    c = sh.list_keyed(limit=0, key_cap=key_cap, now=now, **query)
    assert c == {"matched": len(want), "bytes": want_bytes, "next": None, "rows": []}
    return r["rows"]


def listed_keys(rows):
    return {r["key"] for r in rows}


def pages(sh, limit, now, start=0, **query):
    """Every row from `start` on, fetched `limit` at a time through `next`."""
    rows, totals = [], set()
    while start is not None:
        r = sh.list_keyed(start=start, limit=limit, now=now, **query)
        totals.add((r["matched"], r["bytes"]))
        assert len(r["rows"]) <= limit
        assert r["next"] is None or (len(r["rows"]) == limit and r["next"] > r["rows"][-1]["slot"])
        rows += r["rows"]
        start = r["next"]
    assert len(totals) == 1, "matched and bytes are the same on every page"
    return rows, totals.pop()


def shards_for(devices, objs=None, **kw):
    return tg.make_shards(devices, objs, **kw)


# ---- the matcher
def run_boundary_patterns(devices):
    for plen in pc.BOUNDARY_PLENS:
        pat, objs, must_go = pc.boundary_objects(plen)
        for sh in shards_for(devices, objs):
            now = sh.now()
            assert listed_keys(check_list(sh, objs, now, prefix=pat)) == must_go, plen
            assert listed_keys(check_list(sh, objs, now, prefix=pat, exact=True)) == {pat}, plen
            assert listed_keys(check_list(sh, objs, now)) == set(objs), plen


def run_garbage(devices):
    junk = pc.garbage_values()
    good = {b"/g/%d" % i: keyed(b"/g/%d" % i, b"p" * i) for i in range(5)}
    for sh in shards_for(devices, {**junk, **good}):
        now = sh.now()
        objs = {**junk, **good}
        before = sh.get_many(list(objs))
        assert listed_keys(check_list(sh, objs, now)) == set(good)
        assert check_list(sh, objs, now, prefix=b"/abc") == []
        assert check_list(sh, objs, now, prefix=b"\xff") == []
        assert check_list(sh, objs, now, prefix=b"g") == []
        assert check_list(sh, objs, now, tags=[tg.TARGET, b"a"]) == []
        assert sh.get_many(list(objs)) == before


def run_expired(devices):
    fresh = {b"/x/keep/%d" % i: keyed(b"/x/keep/%d" % i, tagged([b"x"], b"v")) for i in range(10)}
    dying = {b"/x/ttl/%d" % i: keyed(b"/x/ttl/%d" % i, tagged([b"x"], b"v")) for i in range(7)}
    objs = {**fresh, **dying}
    for sh in shards_for(devices):
        tc.store_at(sh, fresh, 0)
        tc.store_at(sh, dying, T0 + 5)
        for query in ({"prefix": b"/x/"}, {"tags": [b"x"]}, {}):
            assert listed_keys(check_list(sh, objs, T0 + 4, **query)) == set(objs)
            assert listed_keys(check_list(sh, objs, T0 + 5, **query)) == set(fresh)


def run_dead_entries(devices):
    """Beside the live entry a dead one of the same digest (expired, pointing at the same
    record) and a locked slot: one row, one object counted."""
    for sh in shards_for(devices):
        key, val, b2, free, loc = tg.dead_entries(sh)
        before = sh._impl.debug_bucket(b2)
        for query in ({"prefix": key}, {"prefix": key, "exact": True}, {"tags": [tg.TARGET]}):
            r = sh.list_keyed(limit=MAX_ROWS, **query)
            assert (r["matched"], r["bytes"]) == (1, item_bytes(len(val))), query
            assert [x["key"] for x in r["rows"]] == [key] and r["rows"][0]["loc"] == loc
        assert sh.list_keyed(limit=MAX_ROWS)["matched"] == 4          # and the three /pre/ ones
        assert sh._impl.debug_bucket(b2) == before


def run_tag_forms(devices):
    """tag_cases' block forms, the alignment sweep and the near misses: the tag matcher, and
    ntags as 0, n and 0xff."""
    forms, must_go = tg.block_form_objects()
    near, near_go = tg.near_miss_objects()
    sweep = tg.alignment_objects()
    for objs, go in ((forms, must_go), (near, near_go), (sweep, None)):
        for sh in shards_for(devices, objs):
            now = sh.now()
            got = listed_keys(check_list(sh, objs, now, tags=[tg.TARGET]))
            if go is not None:
                assert got == go
            else:
                assert len(got) == 40 * 6
            check_list(sh, objs, now, tags=[b"decoy-%d" % i for i in range(63)] + [tg.TARGET])
            rows = check_list(sh, objs, now)
            seen = {r["ntags"] for r in rows}
            if objs is forms:
                assert {0, 1, OVERFLOW} <= seen
            if objs is sweep:
                assert seen == {1, 2, 32}
    for sh in shards_for(devices):
        for bad in ({"tags": []}, {"tags": [b"t%d" % i for i in range(65)]}, {"prefix": b""},
                    {"limit": MAX_ROWS + 1}, {"key_cap": 8}, {"key_cap": 24}, {"key_cap": 1040},
                    {"start": 4 * sh.nbuckets + 1}, {"prefix": b"/", "tags": [b"a"]}):
            try:
                sh.list_keyed(**bad)
            except Exception:
                continue
            raise AssertionError("list_keyed took %r" % (bad,))


# ---- rows
def run_rows_say_what_was_stored(devices):
    """vlen, expire, flags and klen of every row, over mixed expiries, at several times."""
    objs = pc.family_objects(1200, seed=13)
    for sh in shards_for(devices):
        sc.store_mixed(sh, objs, flags=0xC0FFEE)
        for now in (T0, T0 + 50, T0 + TTL0, T0 + 10 ** 6):
            rows = check_list(sh, objs, now)
            assert {r["expire"] for r in rows} == {e for e in sc.EXPIRIES if e == 0 or e > now}
        assert len(check_list(sh, objs, T0, prefix=b"/static/")) > 100


def run_reference_bit(devices):
    """1 after a GET; 0 again once the CLOCK hand has re-appended the object."""
    for sh in shards_for(devices):
        objs = {k: keyed(k, b"v" * 40) for k in (b"/ref/read", b"/ref/unread")}
        tc.store_at(sh, objs, 0)
        assert tc.live_at(sh, {b"/ref/read": objs[b"/ref/read"]}, T0)
        rows = sh.list_keyed(prefix=b"/ref/", now=T0)["rows"]
        assert {r["key"]: r["referenced"] for r in rows} == {b"/ref/read": True,
                                                             b"/ref/unread": False}
    for sh in shards_for(devices):
        assert sh.evict == "clock"
        hot = {b"/hot/%d" % i: keyed(b"/hot/%d" % i, b"h" * 900) for i in range(20)}
        tc.store_at(sh, hot, 0)
        for _ in range(2):
            assert tc.live_at(sh, hot, T0) == set(hot)
        rows = sh.list_keyed(prefix=b"/hot/", now=T0)["rows"]
        assert len(rows) == 20 and all(r["referenced"] for r in rows)
        locs = {r["key"]: r["loc"] for r in rows}
        tg.lap_the_log(sh, now=T0)
        rows = sh.list_keyed(prefix=b"/hot/", now=T0)["rows"]
        assert len(rows) == 20 and sh.counters()["reinserted"] >= 20
        assert not any(r["referenced"] for r in rows)
        assert all(r["loc"] > locs[r["key"]] for r in rows)          # re-appended, not the old record
        assert_slot_order(rows, 4 * sh.nbuckets)


def run_key_cap_edges(devices):
    """The truncation edge (the image head holds the 2-byte klen word: key_cap - 2 key bytes
    fit) and keys whose images end on granule edges."""
    for key_cap in (16, 64):
        klens = [key_cap - 3, key_cap - 2, key_cap - 1, key_cap, key_cap + 20, 300,
                 11, 12, 13, 27, 28]                       # images of 13, 14, 15, 29, 30 bytes
        objs = {}
        for idx, klen in enumerate(klens):
            k = bytes([48 + idx]) + (b"/key/" + b"0123456789abcdef" * 20)[:klen - 1]
            assert len(k) == klen
            objs[k] = keyed(k, b"payload-%d" % idx if idx % 2 else b"")
        for sh in shards_for(devices, objs):
            now = sh.now()
            rows = check_list(sh, objs, now, key_cap=key_cap)
            assert len(rows) == len(klens)
            for r in rows:
                assert r["truncated"] == (r["klen"] > key_cap - 2)
                assert len(r["key"]) == min(r["klen"], key_cap - 2)
            assert len(check_list(sh, objs, now, key_cap=key_cap, prefix=b"0/key/")) == 1


# ---- limit and paging
def sparse_index(sh, n=700):
    """Objects left in the first three and the last three of the index's 16 tiles only (the
    ten tiles between are emptied by DELETEs). Returns ({key: value}, the full listing)."""
    assert 4 * sh.nbuckets == 4096
    objs = {b"/sp/%d" % i: keyed(b"/sp/%d" % i, b"s" * (i % 50)) for i in range(n)}
    pc.store(sh, objs)
    rows = sh.list_keyed(prefix=b"/sp/", limit=MAX_ROWS)["rows"]
    middle = [r["key"] for r in rows if 3 <= r["slot"] // 256 < 13]
    assert sh.remove(digest_strings(middle, sh.device)).all()
    kept = {k: v for k, v in objs.items() if k not in set(middle)}
    full = check_list(sh, kept, sh.now(), prefix=b"/sp/")
    tiles = {r["slot"] // 256 for r in full}
    assert tiles and 0 in tiles and 15 in tiles and not tiles & set(range(3, 13))
    return kept, full


def strip(rows):
    return [(r["slot"], r["key"], r["vlen"], r["loc"]) for r in rows]


def run_limits_and_starts(devices):
    for sh in shards_for(devices):
        kept, full = sparse_index(sh)
        now, m, nslots = sh.now(), len(full), 4 * sh.nbuckets
        nbytes = sum(item_bytes(len(v)) for v in kept.values())
        assert m > 64
        mid = full[m // 2]["slot"]
        starts = [0, full[0]["slot"], full[0]["slot"] + 1, mid, mid + 1, 37, 64, 256, 3 * 256,
                  13 * 256, 13 * 256 - 1, full[-1]["slot"], full[-1]["slot"] + 1, nslots - 1,
                  nslots]
        for start in starts:
            rest = [r for r in full if r["slot"] >= start]
            for limit in sorted({0, 1, 2, len(rest) - 1, len(rest), len(rest) + 1, m - 1, m,
                                 m + 1} - {-1}):
                r = sh.list_keyed(prefix=b"/sp/", start=start, limit=limit, now=now)
                assert (r["matched"], r["bytes"]) == (m, nbytes), (start, limit)
                assert strip(r["rows"]) == strip(rest[:limit]), (sh.device, start, limit)
                want_next = rest[limit - 1]["slot"] + 1 if 0 < limit < len(rest) else None
                assert r["next"] == want_next, (sh.device, start, limit, r["next"], want_next)


def run_paging(devices):
    for sh in shards_for(devices):
        kept, full = sparse_index(sh)
        now = sh.now()
        nbytes = sum(item_bytes(len(v)) for v in kept.values())
        for limit in (1, 7, 64, 1000):
            rows, totals = pages(sh, limit, now, prefix=b"/sp/")
            assert strip(rows) == strip(full), (sh.device, limit)
            assert totals == (len(full), nbytes)
        rows, _ = pages(sh, 7, now)                           # all mode pages the same way
        assert strip(rows) == strip(full)


# ---- state
def run_after_the_log_lapped(devices):
    objs = pc.family_objects(6000, seed=11, max_payload=1500)
    shards = shards_for(devices, objs)
    assert len({sh.head() for sh in shards}) == 1 and shards[0].head() > 3 * shards[0].log_bytes
    for sh in shards:
        now = sh.now()
        n_all = len(check_list(sh, objs, now))
        n_static = len(check_list(sh, objs, now, prefix=b"/static/"))
        assert 0 < n_static < n_all < len(objs) // 2


def run_purges_and_lists_agree(devices):
    objs = tg.tagged_families(1500)
    for sh in shards_for(devices, objs):
        now = sh.now()
        c0, h0 = sh.counters(), sh.head()
        r = sh.list_keyed(prefix=b"/api/", limit=0, now=now)
        t = sh.list_keyed(tags=[b"mod-3", b"fam:/img/"], limit=0, now=now)
        sh.list_keyed(limit=MAX_ROWS, now=now)
        sh.list_keyed(prefix=b"/api/", limit=7, start=100, key_cap=16, now=now)
        assert sh.counters() == c0 and sh.head() == h0       # a list counts and moves nothing
        check_list(sh, objs, now, prefix=b"/api/")
        assert r["matched"] > 100 and t["matched"] > 100
        assert sh.remove_keyed_prefix(b"/api/", now=now) == (r["matched"], r["bytes"])
        assert check_list(sh, objs, now, prefix=b"/api/") == []
        t2 = sh.list_keyed(tags=[b"mod-3", b"fam:/img/"], limit=0, now=now)
        assert 0 < t2["matched"] <= t["matched"]
        assert sh.remove_keyed_tags([b"mod-3", b"fam:/img/"], now=now) == (t2["matched"], t2["bytes"])
        assert check_list(sh, objs, now, tags=[b"mod-3", b"fam:/img/"]) == []
        assert len(check_list(sh, objs, now)) > 0


def run_soft_purged_objects(devices):
    objs = pc.family_objects(400, seed=17)
    for sh in shards_for(devices):
        tc.store_at(sh, objs, T0 + 500, flags=1)
        cap = T0 + 80
        n = sh.soften_keyed_prefix(b"/static/", sc.STALE_AT, cap, now=T0)
        rows = check_list(sh, objs, T0, prefix=b"/static/")
        assert n == len(rows) > 0
        assert {(r["flags"], r["expire"]) for r in rows} == {(sc.STALE_AT, cap)}
        rest = [r for r in check_list(sh, objs, T0) if not r["key"].startswith(b"/static/")]
        assert rest and {(r["flags"], r["expire"]) for r in rest} == {(1, T0 + 500)}
        assert check_list(sh, objs, cap, prefix=b"/static/") == []


def run_while_phase1_pending(devices):
    for sh in shards_for(devices):
        old = {b"/p/old/%d" % i: keyed(b"/p/old/%d" % i, b"o") for i in range(6)}
        tc.store_at(sh, old, 0)
        new = {b"/p/new/%d" % i: keyed(b"/p/new/%d" % i, b"n") for i in range(4)}
        keys = list(new)
        d = digest_strings(keys, sh.device)
        v, vo, vl = pack_values([new[k] for k in keys], sh.device)
        ex = tc.i32([0] * 4, sh.device)
        sh.store(d, v, vo, vl, None, ex, now=T0, phase=1)
        r = sh.list_keyed(prefix=b"/p/", limit=MAX_ROWS, now=T0)      # not refused
        assert listed_keys(r["rows"]) == set(old) and r["matched"] == 6
        assert_slot_order(r["rows"], 4 * sh.nbuckets)
        sh.store(d, v, vo, vl, None, ex, now=T0, phase=2)
        assert listed_keys(check_list(sh, {**old, **new}, T0, prefix=b"/p/")) == set(old) | set(new)


# ---- the backends (CacheBackend::list_objects) and the proxy (GET /_shellac/objects, dry run)
def backend_objects(n_a=6, n_b=4):
    """{key: payload}: /i/a/* tagged x, /i/b/* tagged y, a URL with its Vary variant (the
    variant's key holds '\\x1f') and a key with bytes >= 0x80. Keys carry the proxy's host."""
    objs = {b"localhost/i/a/%d" % i: tagged([b"x"], b"HTTP/ a%d" % i) for i in range(n_a)}
    objs.update({b"localhost/i/b/%d" % i: tagged([b"y"], b"HTTP/ b%d" % i) for i in range(n_b)})
    objs[b"localhost/i/v"] = b"\x01accept-encoding"
    objs[b"localhost/i/v\x1fgzip"] = b"HTTP/ variant"
    objs[b"localhost/i/\xc3\xa9t\xe9"] = b"HTTP/ high bytes"
    return objs


def backend_list_all(be, limit, **query):
    """Every object of the query, `limit` a page through `next`; (objects, pages' totals)."""
    objs, totals, after = [], set(), b""
    for _ in range(10000):
        r = be.list_objects(limit=limit, after=after, **query)
        assert r is not None
        totals.add((r["matched"], r["bytes"], r["shards_skipped"]))
        assert len(r["objects"]) <= limit
        objs += r["objects"]
        if r["next"] is None:
            return objs, totals
        after = r["next"]
    raise AssertionError("the cursor never ended")


def run_backend_listing(be, settle=lambda keys: None, item_size=lambda key, val: len(val)):
    """A tier's list_objects over backend_objects: modes, counts, paging, rows."""
    objs = backend_objects()
    for k, v in objs.items():
        be.set(k, v, 7, 0)
    settle(list(objs))
    want_bytes = sum(item_size(k, keyed(k, v)) for k, v in objs.items())
    for limit in (1, 5, 100):
        got, totals = backend_list_all(be, limit)
        assert sorted(o["key"] for o in got) == sorted(objs), limit
        assert totals == {(len(objs), want_bytes, 0)}, (limit, totals)
    for o in got:
        v = objs[o["key"]]
        assert o["size"] == 2 + len(o["key"]) + len(v) and o["ttl"] is None and o["flags"] == 7
        assert o["tags"] == (1 if v.startswith(b"\x02") else 0) and not o["key_truncated"]
    a = be.list_objects(prefix=b"localhost/i/a/")
    assert a["matched"] == 6 and len(a["objects"]) == 6 and a["next"] is None
    assert be.list_objects(key=b"localhost/i/v")["matched"] == 1
    assert be.list_objects(prefix=b"localhost/i/v\x1f")["matched"] == 1
    assert be.list_objects(tags=[b"x"])["matched"] == 6
    assert be.list_objects(tags=[b"nobody", b"y", b"x"])["matched"] == 10
    c = be.list_objects(prefix=b"localhost/i/", limit=0)
    assert (c["matched"], c["objects"], c["next"]) == (len(objs), [], None)
    assert be.list_objects(tags=[]) is None and be.list_objects(limit=5000) is None
    assert be.list_objects(tags=[b"t%d" % i for i in range(65)]) is None
    assert be.purge_prefix(b"localhost/i/a/") == 6
    assert be.list_objects(prefix=b"localhost/i/a/")["matched"] == 0
    return objs


def inspect(c, query=""):
    """(status, parsed JSON or raw body, raw body) of GET /_shellac/objects<query>."""
    r = c.get("/_shellac/objects" + query)
    body = r.body().read()
    return r.status(), (json.loads(body) if r.status() == 200 else body), body


def key_bytes(obj):
    return obj["key"].encode("latin-1")


def dry_run(c, path, mode=None, tags=None):
    headers = {"X-Purge-Dry-Run": "1", "X-Purge-Soft": "1"}       # (soft is ignored)
    if mode:
        headers["X-Purge-Mode"] = mode
    if tags is not None:
        headers[tg.TAG_HEADER] = tags
    r = c.get(path, method="PURGE", headers=headers)
    body = r.body().read()
    return r.status(), (json.loads(body) if r.status() == 200 else body)


def proxy_inspect_round_trip(px, be, origin, settle=lambda keys: None):
    """GET /_shellac/objects in every mode, escaping, limit / after, and the dry run in its
    three modes: every object stays a hit, a fill in flight is still stored, and the following
    real purge removes what the dry run counted. `px` runs with inspect and purge "loopback",
    tg.TAG_HEADER and no grace, over the backend `be`."""
    from shellac_amd.utils.httpclient import HttpClient
    objs = backend_objects()
    for k, v in objs.items():
        be.set(k, v, 0, 0)
    settle(list(objs))
    c = HttpClient(port=px.port)
    st, r, raw = inspect(c)
    assert st == 200 and r["mode"] == "all" and r["matched"] == r["listed"] == len(objs)
    assert r["next"] is None and r["shards_skipped"] == 0
    assert sorted(key_bytes(o) for o in r["objects"]) == sorted(objs)
    for o in r["objects"]:
        v = objs[key_bytes(o)]
        assert o["size"] == 2 + len(key_bytes(o)) + len(v) and o["ttl"] is None
        assert o["tags"] == (1 if v.startswith(b"\x02") else 0) and o["key_truncated"] is False
        assert "fresh_for" not in o and isinstance(o["referenced"], bool)
    assert b"localhost/i/v\\u001fgzip" in raw and b"/i/\\u00c3\\u00a9t\\u00e9" in raw
    assert all(b < 0x80 for b in raw)
    # the modes; values are percent-decoded once
    st, r, _ = inspect(c, "?prefix=localhost/i/a/")
    assert (r["mode"], r["matched"], r["listed"]) == ("prefix", 6, 6)
    assert inspect(c, "?prefix=localhost%2Fi%2Fb%2F")[1]["matched"] == 4
    assert inspect(c, "?prefix=localhost%252Fi%252Fb%252F")[1]["matched"] == 0
    assert inspect(c, "?prefix=localhost/i/%C3%A9")[1]["matched"] == 1
    st, r, _ = inspect(c, "?key=localhost/i/v")
    assert (r["mode"], r["matched"]) == ("key", 1) and key_bytes(r["objects"][0]) == b"localhost/i/v"
    assert inspect(c, "?key=localhost/i/v%1Fgzip")[1]["matched"] == 1
    assert inspect(c, "?tag=x")[1]["matched"] == 6
    st, r, _ = inspect(c, "?tag=x,y,nobody")
    assert (r["mode"], r["matched"]) == ("tag", 10)
    # limit and after
    for limit in (1, 4):
        keys, after = [], None
        for _ in range(100):
            q = "?prefix=localhost/i/&limit=%d" % limit + ("&after=" + after if after else "")
            st, r, _ = inspect(c, q)
            assert st == 200 and r["matched"] == len(objs) and r["listed"] == len(r["objects"]) <= limit
            keys += [key_bytes(o) for o in r["objects"]]
            after = r["next"]
            if after is None:
                break
        assert sorted(keys) == sorted(objs) and len(set(keys)) == len(keys), limit
    st, r, _ = inspect(c, "?limit=0")
    assert (r["matched"], r["listed"], r["objects"], r["next"]) == (len(objs), 0, [], None)
    # refusals
    for bad in ("?limit=abc", "?limit=4097", "?prefix=a&key=b", "?nonsense=1", "?prefix=%zz",
                "?prefix=", "?tag=", "?tag=" + ",".join("t%d" % i for i in range(65))):
        assert inspect(c, bad)[0] == 400, bad
    # ---- the dry run: prefix, exact (with its variants), tag
    listed = inspect(c, "?prefix=localhost/i/a/")[1]
    st, d = dry_run(c, "/i/a/", "prefix")
    assert (st, d) == (200, {"mode": "prefix", "dry_run": True, "matched": 6,
                             "bytes": listed["bytes"]}) and d["bytes"] > 0
    st, d = dry_run(c, "/i/v")
    assert st == 200 and d == {"mode": "exact", "dry_run": True, "matched": 1, "bytes": d["bytes"],
                               "variants": 1}
    st, d = dry_run(c, "/ignored", "tag", "y")
    assert st == 200 and d == {"mode": "tag", "dry_run": True, "tags": 1, "matched": 4,
                               "bytes": inspect(c, "?tag=y")[1]["bytes"]}
    assert dry_run(c, "/ignored", "tag", None)[0] == 400
    assert dry_run(c, "/i/nothing/", "prefix")[1]["matched"] == 0
    assert all(be.get(k) is not None for k in objs)            # every object is still a hit
    # a fill in flight across a dry run is still stored (purged_since is untouched)
    origin.delays["/slow/d"] = 0.4
    got = {}
    th = threading.Thread(
        target=lambda: got.update(b=HttpClient(port=px.port).get("/slow/d").body().read()))
    th.start()
    assert origin.wait_seen("/slow/d", 1)
    assert dry_run(c, "/slow/", "prefix")[1]["matched"] == 0
    assert dry_run(c, "/slow/d")[1]["matched"] == 0
    th.join()
    assert got["b"] == origin.body("/slow/d")
    settle([b"localhost/slow/d"])
    assert be.get(b"localhost/slow/d") is not None
    st = px.stats()
    assert st["fills_not_cached_purged"] == 0 and st["purge_requests"] == 0
    assert st["purged_objects"] == 0 and st["purge_dry_runs"] == 6 and st["inspect_requests"] > 20
    # the real purges remove what the dry runs counted
    assert pc.purge(c, "/i/a/", prefix=True) == (200, {"mode": "prefix", "purged": 6})
    assert pc.purge(c, "/i/v") == (200, {"mode": "exact", "found": True, "variants": 1})
    assert tg.tag_purge(c, "y") == (200, {"mode": "tag", "tags": 1, "purged": 4})
    assert inspect(c)[1]["matched"] == len(objs) - 6 - 2 - 4 + 1          # + /slow/d
    c.close()


def non_loopback_address():
    """An address of this host that is not loopback, or None."""
    import socket
    try:
        infos = socket.getaddrinfo(socket.gethostname(), None, socket.AF_INET)
    except OSError:
        return None
    for info in infos:
        if not info[4][0].startswith("127."):
            return info[4][0]
    return None
