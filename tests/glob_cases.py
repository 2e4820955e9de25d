"""Scenarios shared by tests/test_glob_purge.py (CPU) and tests/test_glob_purge_gpu.py: the
Python model of the glob matcher (a regex on the key's base, the key up to its first 0x1f),
and the runs the twins (HostCache on the CPU; k_keyed_scan<GlobMatch, RemoveAction>, k_keyed_scan<GlobMatch, SoftenAction> and
k_list_scan<GlobMatch> on the GPU) are checked with, in the hard, soft and list forms. Every
shard is compared with the model of what it holds itself."""
import json
import random
import re

import list_cases as lc
import purge_cases as pc
import soften_cases as sc
import tag_cases as tg
import touch_cases as tc
from shellac_amd import core
from shellac_amd.ops.cache import digest_strings, item_bytes, keyed, pack_values

T0, TTL0, NOWS = tc.T0, tc.TTL0, tc.NOWS
M64 = tc.M64
SEP = b"\x1f"
MAX_STARS, MAX_LITERAL = 8, 1024
REFUSED = [b"", b"*", b"***", b"/a/*\\", b"\\", b"a*" * 9, b"*" * 9 + b"a", b"a" * 1025,
           b"a" * 1000 + b"*" + b"b" * 25]


# ---- the model
def segments(pattern):
    """The literal segments between the unescaped stars; ValueError on a refused pattern."""
    segs, i, stars = [b""], 0, 0
    while i < len(pattern):
        c = pattern[i:i + 1]
        if c == b"*":
            segs.append(b"")
            stars += 1
        else:
            if c == b"\\":
                i += 1
                if i == len(pattern):
                    raise ValueError("dangling backslash")
                c = pattern[i:i + 1]
            segs[-1] += c
        i += 1
    if not pattern or not any(segs) or stars > MAX_STARS or sum(map(len, segs)) > MAX_LITERAL:
        raise ValueError("refused pattern")
    return segs


def regex(pattern):
    return re.compile(b".*".join(map(re.escape, segments(pattern))), re.S)


def matches(pattern, key):
    """The model: the regex, anchored, on the key's base; an empty key never matches."""
    return bool(key) and regex(pattern).fullmatch(key.split(SEP, 1)[0]) is not None


def value_matches(pattern, value):
    key = lc.key_of(value)
    return key is not None and matches(pattern, key)


def model_purge(objs, live, pattern):
    """(count, item bytes, survivors) a glob purge must give on the live set."""
    gone = {k for k in live if value_matches(pattern, objs[k])}
    return len(gone), sum(item_bytes(len(objs[k])) for k in gone), live - gone


def esc(literal):
    """A literal byte string as a pattern."""
    return literal.replace(b"\\", b"\\\\").replace(b"*", b"\\*")


# ---- checks
def check_count(shards, objs, live, pattern, now=None):
    """The read-only forms: list_keyed(glob=, limit=0) and a flags-only soft purge both count
    the model's matches on every shard; returns the count."""
    want_n, want_bytes, _ = model_purge(objs, live, pattern)
    for sh in shards:
        r = sh.list_keyed(glob=pattern, limit=0, now=now)
        assert (r["matched"], r["bytes"], r["rows"], r["next"]) == (want_n, want_bytes, [], None), \
            (sh.device, pattern, r["matched"], want_n)
    return want_n


def check_purge(shards, objs, live, pattern):
    """Hard-purge `pattern` on every shard (they hold the same live set): count, bytes and
    survivors are the model's, the survivors are bit-identical to what was stored, `purged`
    moves by the count."""
    want_n, want_bytes, survivors = model_purge(objs, live, pattern)
    for sh in shards:
        before = sh.counters()["purged"]
        got = sh.remove_keyed_glob(pattern)
        assert got == (want_n, want_bytes), (sh.device, pattern, got, want_n)
        after = tg.live_values(sh, objs)
        assert set(after) == survivors, (sh.device, pattern, sorted(set(after) ^ survivors)[:5])
        assert all(after[k] == objs[k] for k in survivors), (sh.device, pattern)
        assert sh.counters()["purged"] - before == want_n
    purged = {sh.counters()["purged"] for sh in shards}
    assert len(purged) == 1, purged
    return want_n, survivors


def check_all_forms(shards, objs, pattern, must_go=None):
    """List (with rows), soften (flags only) and hard-purge `pattern` on shards that hold all
    of `objs`: each form takes exactly the model's keys, which are `must_go` where given."""
    live = set(objs)
    want = {k for k in live if value_matches(pattern, objs[k])}
    if must_go is not None:
        assert want == set(must_go), (pattern, sorted(want ^ set(must_go))[:4])
    for sh in shards:
        assert set(tg.live_values(sh, objs)) == live
        r = sh.list_keyed(glob=pattern, limit=lc.MAX_ROWS, key_cap=1024)
        lc.assert_slot_order(r["rows"], 4 * sh.nbuckets)
        assert lc.listed_keys(r["rows"]) == want and r["matched"] == len(want), \
            (sh.device, pattern, sorted(lc.listed_keys(r["rows"]) ^ want)[:4])
        assert sh.soften_keyed_glob(pattern, 77) == len(want), (sh.device, pattern)
        assert sh.remove_keyed_glob(pattern)[0] == len(want), (sh.device, pattern)
        assert set(tg.live_values(sh, objs)) == live - want, (sh.device, pattern)
    return want


def shards_for(devices, objs=None, **kw):
    return tg.make_shards(devices, objs, **kw)


# ---- 1. families
FAMILY_PATTERNS = [b"*/static/*", b"/static/*.html", b"*.html", b"/api/*/users/*", b"/nothing/*",
                   b"*.nothing", b"/*"]


def run_families(devices, n=3000):
    objs = pc.family_objects(n)
    shards = shards_for(devices, objs)
    live = tg.equalise_live(shards, objs)
    assert len(live) > 0.96 * n
    one = sorted(k for k in live if k.startswith(b"/img/"))[0]
    counts = {p: check_count(shards, objs, live, p) for p in FAMILY_PATTERNS + [esc(one)]}
    assert counts[b"/*"] == counts[b"*.html"] == len(live) and counts[esc(one)] == 1
    assert counts[b"/nothing/*"] == counts[b"*.nothing"] == 0
    assert 0 < counts[b"/static/*.html"] == counts[b"*/static/*"] < len(live)
    assert 0 < counts[b"/api/*/users/*"] < len(live)
    for sh in shards:      # the soft form counts the same (flags only: nothing else changes)
        assert sh.soften_keyed_glob(b"/api/*/users/*", 5) == counts[b"/api/*/users/*"]
    total = 0
    for p in (b"/nothing/*", b"*.nothing", esc(one), b"/api/*/users/*", b"/static/*.html",
              b"*/static/*", b"*.html", b"/*"):
        got, live = check_purge(shards, objs, live, p)
        total += got
    assert live == set() and total > 0.96 * n
    assert all(sh.sweep()[0] == 0 for sh in shards)


# ---- 2. granule boundaries
LOWER = b"abcdefghijklmnopqrstuvwxyz0123456789"


def _flip(b, i):
    return b[:i] + bytes([b[i] ^ 0x01]) + b[i + 1:]     # (stays in LOWER's classes or near them)


def _filler(n, salt):
    """n bytes of upper-case filler, distinct per salt where n >= 2: never part of a segment."""
    return (b"%c%c" % (65 + salt % 26, 65 + salt // 26 % 26) + b"QZ" * n)[:n]


def boundary_cases(seglen, seed=3):
    """For a segment of `seglen` bytes: [(pattern, {key: value}, keys that match)] with the
    segment as the head, the tail and a middle."""
    rng = random.Random(seed * 1000 + seglen)
    seg = bytes(rng.choice(LOWER) for _ in range(seglen))
    val = lambda k: keyed(k, b"payload-%d" % (len(k) % 7))
    out = []
    # head: equal and followed by more match; a flipped first or last byte and a shorter key miss
    keys = {"equal": seg, "longer": seg + b"MORE/x.html", "first": _flip(seg, 0) + b"TAIL",
            "last": _flip(seg, seglen - 1) + b"TAIL"}
    if seglen > 1:
        keys["short"] = seg[:-1]
    out.append((seg + b"*", {k: val(k) for k in keys.values()}, {keys["equal"], keys["longer"]}))
    # tail: the key (it starts at value byte 2) ends exactly at a granule end, one byte before,
    # one byte after
    objs, go = {}, set()
    for salt, rest in enumerate((0, 15, 1)):
        klen = seglen + 3
        while (2 + klen) % 16 != rest:
            klen += 1
        k = _filler(klen - seglen, salt) + seg
        objs[k] = val(k)
        go.add(k)
        for j, miss in enumerate((_flip(seg, 0), _flip(seg, seglen - 1))):
            k = _filler(klen - seglen, 10 + 2 * salt + j) + miss
            objs[k] = val(k)
        k = _filler(klen - seglen, 20 + salt) + seg + b"X"          # the segment, not at the end
        objs[k] = val(k)
    out.append((b"*" + seg, objs, go))
    # middle: at offset 0, 13, 14 and klen - len of a 64-byte key (longer where the segment is)
    objs, go = {}, set()
    klen = 64 if seglen <= 48 else seglen + 16
    for salt, at in enumerate((0, 13, 14, klen - seglen)):
        k = _filler(at, salt) + seg + _filler(klen - at - seglen, 30 + salt)
        assert len(k) == klen
        objs[k] = val(k)
        go.add(k)
        k = _filler(at, 40 + salt) + _flip(seg, seglen - 1) + _filler(klen - at - seglen, 50 + salt)
        objs[k] = val(k)
    out.append((b"*" + seg + b"*", objs, go))
    return out


def run_boundaries(devices, seglen):
    bystanders = pc.family_objects(40, seed=seglen)
    for pattern, objs, must_go in boundary_cases(seglen):
        allobjs = {**objs, **{k: v for k, v in bystanders.items() if not matches(pattern, k)}}
        got = check_all_forms(shards_for(devices, allobjs), allobjs, pattern)
        assert got == must_go, (seglen, pattern[:20], sorted(got ^ must_go)[:3])


# ---- 3. bounded by klen
def run_bounded_by_klen(devices):
    objs = {
        # the key is the pattern's head and the payload continues like the pattern
        b"/bound/he": keyed(b"/bound/he", b"ad/x.css and more"),
        # the payload holds the tail segment, the key does not
        b"/bound/head/x": keyed(b"/bound/head/x", b".css"),
        b"/bound/head/y.cs": keyed(b"/bound/head/y.cs", b"s"),
        # a separator in the payload is no separator: the subject is the whole key
        b"/bound/head/z.css.bak": keyed(b"/bound/head/z.css.bak", SEP + b".css" + SEP),
        b"/bound/head/ok.css": keyed(b"/bound/head/ok.css", SEP + b"payload"),
        # the middle segment straddles the key's end
        b"/bound/head/mid": keyed(b"/bound/head/mid", b"dle/q.css"),
    }
    for pattern, go in ((b"/bound/head/*.css", {b"/bound/head/ok.css"}),
                        (b"/bound/head*", set(objs) - {b"/bound/he"}),
                        (b"*/middle/*", set()), (b"*.css", {b"/bound/head/ok.css"})):
        check_all_forms(shards_for(devices, objs), objs, pattern, go)


# ---- 4. overlaps and order
OVERLAPS = [(b"ab*ba", b"aba", False), (b"ab*ba", b"abba", True), (b"*ab*ab*", b"abab", True),
            (b"*ab*ab*", b"aab", False), (b"*a", b"bbbba", True), (b"a*", b"a", True),
            (b"a**b", b"ab", True), (b"a\\*b", b"a*b", True), (b"a\\*b", b"axb", False),
            (b"a\\\\b", b"a\\b", True), (b"a\\\\b", b"ab", False)]


def run_overlaps(devices):
    objs = {k: keyed(k, b"v-" + k) for _, k, _ in OVERLAPS}
    for pattern in sorted({p for p, _, _ in OVERLAPS}):
        table = {k for p, k, yes in OVERLAPS if p == pattern and yes}
        no = {k for p, k, yes in OVERLAPS if p == pattern and not yes}
        got = check_all_forms(shards_for(devices, objs), objs, pattern)
        assert table <= got and not no & got, (pattern, got)
    for p, k, yes in OVERLAPS:
        assert core().glob_match(p, k) is yes and matches(p, k) is yes, (p, k)


# ---- 5. variants
def run_variants(devices):
    k = b"localhost/site/main.css"
    v1, v2 = k + SEP + b"gzip", k + SEP + b"br"
    objs = {k: keyed(k, b"\x01accept-encoding"), v1: keyed(v1, b"HTTP/ gz"),
            v2: keyed(v2, b"HTTP/ br"), b"localhost/site/main.js": keyed(b"localhost/site/main.js", b"j"),
            b"gzip": keyed(b"gzip", b"a key that ends like v1")}
    check_all_forms(shards_for(devices, objs), objs, b"*" + k[-4:], {k, v1, v2})
    check_all_forms(shards_for(devices, objs), objs, b"*zip", {b"gzip"})     # v1's end: not v1
    check_all_forms(shards_for(devices, objs), objs, b"*main.css*gzip", set())
    check_all_forms(shards_for(devices, objs), objs, esc(k), {k, v1, v2})    # starless: the base
    check_all_forms(shards_for(devices, objs), objs, b"*" + SEP + b"*", set())


# ---- 6. long keys
def run_long_keys(devices):
    rng = random.Random(41)
    mid = bytes(rng.choice(LOWER) for _ in range(300))
    head, tail = b"/long/head/", b".tail"
    # the filler repeats the segment's first 299 bytes with another last byte: near misses
    near = mid[:299] + b"#"
    fill = (near * 10)[:3000 - len(head) - len(tail) - 300]
    key = head + fill + mid + tail
    assert len(key) == 3000 and key.count(mid) == 1
    miss = head + fill + _flip(mid, 299) + tail
    objs = {key: keyed(key, b"p" * 100), miss: keyed(miss, b"q" * 100),
            b"/long/head/short.tail": keyed(b"/long/head/short.tail", mid)}
    pattern = head + b"*" + mid + b"*" + tail
    for sh in shards_for(devices, objs):
        assert set(tg.live_values(sh, objs)) == set(objs)
        r = sh.list_keyed(glob=pattern, limit=10, key_cap=1024)
        assert r["matched"] == 1 and r["rows"][0]["klen"] == 3000 and r["rows"][0]["truncated"]
        assert r["rows"][0]["key"] == key[:1022]
        assert sh.soften_keyed_glob(pattern, 9) == 1
        assert sh.list_keyed(glob=b"*" + mid + tail, limit=0)["matched"] == 1       # as the tail
        assert sh.list_keyed(glob=head + fill[:1000] + b"*", limit=0)["matched"] == 2  # a long head
        assert sh.remove_keyed_glob(pattern) == (1, item_bytes(len(objs[key])))
        assert set(tg.live_values(sh, objs)) == set(objs) - {key}


# ---- 7. random sweep
def sweep_keys(n=2000, seed=23):
    rng = random.Random(seed)
    keys = set()
    while len(keys) < n:
        keys.add(bytes(rng.choice(b"ab/") for _ in range(rng.randint(1, 40))))
    return sorted(keys)


def sweep_patterns(n=200, seed=29):
    rng = random.Random(seed)
    pats = []
    while len(pats) < n:
        p = bytes(rng.choice(b"ab/*" if rng.random() < 0.7 else b"ab/")
                  for _ in range(rng.randint(1, 12)))
        if p.count(b"*") <= MAX_STARS and p.strip(b"*"):
            pats.append(p)
    return pats


def run_random_sweep(devices):
    keys = sweep_keys()
    objs = {k: keyed(k, b"v" * (len(k) % 9)) for k in keys}
    shards = shards_for(devices, objs)
    live = tg.equalise_live(shards, objs)
    assert len(live) >= 0.99 * len(keys)
    pats = sweep_patterns()
    counts = [check_count(shards, objs, live, p) for p in pats]
    assert sum(1 for c in counts if c) > 50 and sum(1 for c in counts if not c) > 20
    hard = [p for p, c in zip(pats, counts) if 0 < c < 400][:10]
    assert len(hard) == 10
    for p in hard:
        _, live = check_purge(shards, objs, live, p)
    assert live


# ---- 8. garbage values
def run_garbage(devices):
    junk = pc.garbage_values()
    good = {b"/abc/%d" % i: keyed(b"/abc/%d" % i, b"p" * i) for i in range(5)}
    objs = {**junk, **good}
    shards = shards_for(devices, objs)
    before = [sh.get_many(list(objs)) for sh in shards]
    for p in (b"*/", b"*/abc", b"*\xff", b"\xff*", b"*abcdefghi", b"/abc*", b"*\x00*",
              b"x" * 1024, b"\xff" * 38 + b"*", b"*" + b"\xff" * 1023 + b"*\xff"):
        want = len([v for v in objs.values() if value_matches(p, v)])
        for sh in shards:
            assert sh.list_keyed(glob=p, limit=0)["matched"] == want, (sh.device, p[:12])
            assert sh.soften_keyed_glob(p, 3) == want
        if want == 0:
            for sh in shards:
                assert sh.remove_keyed_glob(p) == (0, 0)
    assert [sh.get_many(list(objs)) for sh in shards] == before
    for sh in shards:
        assert sh.remove_keyed_glob(b"/abc*")[0] == 5
    assert len({tuple(sh.get_many(list(objs))) for sh in shards}) == 1


# ---- 9. refused patterns
def run_refused(devices):
    for sh in shards_for(devices, {b"/r/1": keyed(b"/r/1", b"v")}):
        for bad in REFUSED:
            for call in (lambda: sh.remove_keyed_glob(bad), lambda: sh.soften_keyed_glob(bad, 5),
                         lambda: sh.list_keyed(glob=bad)):
                try:
                    call()
                except ValueError:
                    continue
                raise AssertionError("%s took the pattern %r" % (sh.device, bad[:12]))
        for bad in ({"glob": b"/r/*", "prefix": b"/r/"}, {"glob": b"/r/*", "tags": [b"a"]},
                    {"glob": b"/r/*", "exact": True}):
            try:
                sh.list_keyed(**bad)
            except ValueError:
                continue
            raise AssertionError("list_keyed took %r" % (bad,))
        # the limits themselves are accepted
        assert sh.list_keyed(glob=b"*/*r*/*1*" + b"*" * 3)["matched"] == 1        # 8 stars
        assert sh.remove_keyed_glob(b"a" * 1024) == (0, 0)
        assert sh.get_many([b"/r/1"]) == [keyed(b"/r/1", b"v")]
    for bad in REFUSED:
        try:
            core().keyed_glob_image(bad)
        except ValueError:
            continue
        raise AssertionError("compiled %r" % bad[:12])


# ---- 10. liveness
def run_expired_are_not_counted(devices):
    for sh in shards_for(devices):
        fresh = {b"/x/keep/%d" % i: keyed(b"/x/keep/%d" % i, b"v") for i in range(10)}
        dying = {b"/x/ttl/%d" % i: keyed(b"/x/ttl/%d" % i, b"v") for i in range(7)}
        pc.store(sh, fresh)
        pc.store(sh, dying, ttl=5)
        later = sh.now() + 100
        assert sh.list_keyed(glob=b"/x/*", limit=0)["matched"] == 17
        assert sh.list_keyed(glob=b"/x/*", limit=0, now=later)["matched"] == len(fresh)
        assert sh.soften_keyed_glob(b"*/ttl/*", 9, now=later) == 0
        assert sh.soften_keyed_glob(b"/x/*", 9, now=later) == len(fresh)
        assert sh.remove_keyed_glob(b"/x/*", now=later)[0] == len(fresh)


def run_dead_entries(devices):
    """test_dead_same_digest_entry_is_not_counted's construction: beside the live entry a dead
    one of its digest (expired, pointing at the very same record) and a locked slot."""
    for form in ("list", "soft", "hard"):
        for sh in shards_for(devices):
            key, val, b2, free, loc = tg.dead_entries(sh)
            before = sh._impl.debug_bucket(b2)
            if form == "list":
                r = sh.list_keyed(glob=b"*/object", limit=10)
                assert (r["matched"], r["bytes"]) == (1, item_bytes(len(val)))
                assert [x["key"] for x in r["rows"]] == [key] and r["rows"][0]["loc"] == loc
                assert sh.list_keyed(glob=b"/*", limit=0)["matched"] == 4    # and the three /pre/
            elif form == "soft":
                assert sh.soften_keyed_glob(b"*/object", 9) == 1     # (flags only)
                assert sh.get_many([key]) == [val]
            if form != "hard":
                assert sh._impl.debug_bucket(b2) == before
                continue
            assert sh.remove_keyed_glob(b"/tw*/object") == (1, item_bytes(len(val)))
            assert sh.counters()["purged"] == 1
            after = sh._impl.debug_bucket(b2)
            assert after[4 * free[0] + 2] == loc and after[4 * free[1] + 2] == M64 - 1
            assert sh.get_many([key]) == [None]


def run_after_the_log_lapped(devices):
    objs = pc.family_objects(6000, seed=11, max_payload=1500)
    shards = shards_for(devices, objs)
    assert len({sh.head() for sh in shards}) == 1 and shards[0].head() > 3 * shards[0].log_bytes
    live = tg.equalise_live(shards, objs)
    assert 0 < len(live) < len(objs) // 2
    for p in (b"*/static/*", b"/api/*/users/*.html", b"*7.html"):
        assert check_count(shards, objs, live, p) > 0
    n, live = check_purge(shards, objs, live, b"/static/*.html")
    assert 0 < n < n + len(live)
    n, live = check_purge(shards, objs, live, b"*/v1/*")
    assert n > 0 and live


# ---- 11. the soft form
def model_soften(model, objs, pattern, stale_at, expire_cap, now):
    out, n = dict(model), 0
    for k, (e, _) in model.items():
        if (e and e <= now) or not value_matches(pattern, objs[k]):
            continue
        n += 1
        if expire_cap and (e == 0 or e > expire_cap):
            e = expire_cap
        out[k] = (e, stale_at)
    return n, out


def check_soften(shards, objs, model, pattern, expire_cap, stale_at=sc.STALE_AT, now=T0):
    """tg.check_soften with the glob matcher: the count is the model's, twice in a row;
    afterwards flags, header expiry and liveness at NOWS are the model's for every object, and
    the objects that do not match are bit-identical."""
    want_n, model2 = model_soften(model, objs, pattern, stale_at, expire_cap, now)
    want = sc.want_snapshot(objs, model2)
    for sh in shards:
        was = sc.snapshot(sh, objs)
        for _ in range(2):
            got = sh.soften_keyed_glob(pattern, stale_at, expire_cap, now=now)
            assert got == want_n, (sh.device, pattern, expire_cap, got, want_n)
        after = sc.snapshot(sh, objs)
        assert after == want, (sh.device, pattern, expire_cap)
        for t in NOWS:
            for k, rec in was[t].items():
                if not value_matches(pattern, objs[k]):
                    assert after[t].get(k) == rec, (sh.device, t, k)
    return want_n, model2


def run_soft_form(devices):
    objs = pc.family_objects(400, seed=19)
    for cap in sc.CAPS:
        shards = shards_for(devices)
        for sh in shards:
            sc.store_mixed(sh, objs)
        models = [sc.model_of(sh, objs) for sh in shards]
        assert all(m == models[0] for m in models) and set(models[0]) == set(objs)
        n, model = check_soften(shards, objs, models[0], b"/static/*.html", cap)
        assert 50 < n < len(objs)
        # a second, wider pass with a late cap: lives are only ever shortened
        n2, model = check_soften(shards, objs, model, b"*/static/*", T0 + 10 ** 6,
                                 stale_at=sc.STALE_AT + 1)
        assert n2 == n
        if cap:
            assert all(e for k, (e, f) in model.items() if f == sc.STALE_AT + 1)
            assert all(e <= cap for k, (e, f) in model.items() if f == sc.STALE_AT + 1)
        # past a cap that has run out the objects are dead: a later pass counts fewer
        n3, _ = check_soften(shards, objs, model, b"*.html", 0, now=T0 + 90)
        assert n3 < len(objs)


def run_reference_bit(devices):
    for sh in shards_for(devices):
        objs = {k: keyed(k, b"v" * 40) for k in (b"/ref/read", b"/ref/unread")}
        tc.store_at(sh, objs, T0 + 500, flags=1)
        assert tc.live_at(sh, {b"/ref/read": objs[b"/ref/read"]}, T0)
        assert tc.ref_bit(sh, b"/ref/read") == (True, T0 + 500)
        assert sh.soften_keyed_glob(b"*/*read", 5, T0 + 100, now=T0) == 2
        assert tc.ref_bit(sh, b"/ref/read") == (True, T0 + 100)
        assert tc.ref_bit(sh, b"/ref/unread") == (False, T0 + 100)
        assert tc.records_at(sh, objs, T0 + 99) == {k: (v, 5, T0 + 100) for k, v in objs.items()}
        assert tc.records_at(sh, objs, T0 + 100) == {}
        try:
            sh.soften_keyed_glob(b"/ref/*", 5, T0, now=T0)       # the cap must lie after now
        except Exception:
            continue
        raise AssertionError("took a cap that does not lie after now")


def run_refused_while_phase1_pending(devices):
    for sh in shards_for(devices):
        objs = {b"/p/%d" % i: keyed(b"/p/%d" % i, b"v") for i in range(4)}
        keys = list(objs)
        d = digest_strings(keys, sh.device)
        v, vo, vl = pack_values([objs[k] for k in keys], sh.device)
        ex = tc.i32([0] * 4, sh.device)
        sh.store(d, v, vo, vl, None, ex, now=T0, phase=1)
        try:
            sh.soften_keyed_glob(b"/p/*", 5, now=T0)
        except Exception as e:
            assert "phase-1" in str(e)
        else:
            raise AssertionError("softened while a phase-1 batch was pending")
        assert sh.list_keyed(glob=b"/p/*", limit=0, now=T0)["matched"] == 0      # not refused
        sh.store(d, v, vo, vl, None, ex, now=T0, phase=2)
        assert sh.soften_keyed_glob(b"/p/*", 5, T0 + 9, now=T0) == 4
        assert sc.model_of(sh, objs) == {k: (T0 + 9, 5) for k in keys}


# ---- 12. listing
def run_listing(devices):
    objs = pc.family_objects(1200, seed=13)
    pattern = b"/static/*.html"
    for sh in shards_for(devices):
        sc.store_mixed(sh, objs, flags=0xC0FFEE)
        for now in (T0, T0 + 50, T0 + TTL0):
            records = tc.records_at(sh, objs, now)
            want = {(lc.key_of(v), len(lc.key_of(v))): (len(v), e, f, 0, False)
                    for v, f, e in records.values() if value_matches(pattern, v)}
            want_bytes = sum(item_bytes(n) for n, _, _, _, _ in want.values())
            c0, h0 = sh.counters(), sh.head()
            r = sh.list_keyed(glob=pattern, limit=lc.MAX_ROWS, key_cap=256, now=now)
            assert (r["matched"], r["bytes"], r["next"]) == (len(want), want_bytes, None)
            lc.assert_slot_order(r["rows"], 4 * sh.nbuckets)
            assert lc.rows_view(r["rows"]) == want and len(r["rows"]) == len(want) > 100
            for limit in (1, 7, 64, 1000):                       # pages concatenate
                if limit == 1 and now != T0:
                    continue
                rows, totals = lc.pages(sh, limit, now, glob=pattern)
                assert lc.strip(rows) == lc.strip(r["rows"]), (sh.device, limit)
                assert totals == (len(want), want_bytes)
            assert sh.counters() == c0 and sh.head() == h0       # a list counts and moves nothing
            assert tc.records_at(sh, objs, now) == records
        c = sh.list_keyed(glob=pattern, limit=0, now=T0)
        assert sh.remove_keyed_glob(pattern, now=T0) == (c["matched"], c["bytes"])
        assert sh.list_keyed(glob=pattern, limit=0, now=T0)["matched"] == 0
        assert sh.list_keyed(limit=0, now=T0)["matched"] > 0


# ---- the backends (CacheBackend::purge_glob / soften_glob / list_objects) and the proxy
def run_backend_glob(be, settle=lambda keys: None):
    """A tier's purge_glob, soften_glob and list_objects(glob=) over lc.backend_objects."""
    objs = lc.backend_objects()
    for k, v in objs.items():
        be.set(k, v, 7, 0)
    settle(list(objs))
    count = lambda p: len([k for k in objs if matches(p, k)])
    for p in (b"localhost/i/a/*", b"*/i/*/1", b"*/v", b"*", b"*/nothing"):
        if p == b"*":
            assert be.list_objects(glob=p) is None
            continue
        r = be.list_objects(glob=p)
        assert r["matched"] == count(p) == len(r["objects"]) and r["next"] is None, p
        assert sorted(o["key"] for o in r["objects"]) == sorted(k for k in objs if matches(p, k))
    assert count(b"*/v") == 2                              # the marker and its variant
    got, totals = lc.backend_list_all(be, 3, glob=b"localhost/i/*")
    assert sorted(o["key"] for o in got) == sorted(objs) and len(totals) == 1
    for bad in REFUSED:
        assert be.purge_glob(bad) == -1 and be.soften_glob(bad, 5) == -1, bad[:12]
        assert be.list_objects(glob=bad) is None
    assert be.soften_glob(b"*/i/b/*", 1234, keep_s=100) == 4
    assert be.soften_glob(b"*/i/b/*", 1234, keep_s=100) == 4
    assert be.purge_glob(b"*/i/*/1") == 2
    assert be.purge_glob(b"*/i/*/1") == 0
    assert be.purge_glob(b"*/v") == 2
    assert be.list_objects(glob=b"localhost/i/*")["matched"] == len(objs) - 4
    assert be.get(b"localhost/i/a/0") is not None and be.get(b"localhost/i/a/1") is None
    return objs


def glob_purge(c, path, soft=False, dry=False):
    headers = {"X-Purge-Mode": "glob"}
    if soft:
        headers["X-Purge-Soft"] = "1"
    if dry:
        headers["X-Purge-Dry-Run"] = "1"
    r = c.get(path, method="PURGE", headers=headers)
    body = r.body().read()
    return r.status(), (json.loads(body) if r.status() == 200 else body)


def proxy_glob_round_trip(px, origin, settle=lambda: None):
    """Fill a few URL families through the proxy, then PURGE by glob: inspection, the dry run,
    the hard form (a Vary'd URL's variants go with it), a literal '?' and '\\', refused
    patterns. `px` runs with purge and inspect "loopback" and no grace over a tg.TagOrigin."""
    from shellac_amd.utils.httpclient import HttpClient
    c = HttpClient(port=px.port)
    hits = lambda p: len(origin.seen(p))
    css = ["/g/a/%d.css" % i for i in range(5)]
    js = ["/g/a/%d.js" % i for i in range(5)]
    other = ["/g/b/1.css", "/g/q?x=1", "/g/qyx=1"]
    origin.vary["/g/a/v.css"] = "X-Lang"
    langs = [{"X-Lang": "de"}, {"X-Lang": "fr"}]
    for _ in range(2):
        for p in css + js + other:
            assert c.get(p).status() == 200
        for h in langs:
            assert c.get("/g/a/v.css", headers=h).body().read() == origin.body("/g/a/v.css")
        settle()
    assert all(hits(p) == 1 for p in css + js + other), origin.log
    assert hits("/g/a/v.css") == 2
    st, r, _ = lc.inspect(c, "?glob=*/g/a/*.css")
    assert st == 200 and (r["mode"], r["matched"], r["listed"]) == ("glob", 8, 8)   # + marker, 2 variants
    keys = sorted(lc.key_bytes(o) for o in r["objects"])
    assert [k for k in keys if SEP not in k] == sorted(
        b"localhost" + p.encode() for p in css + ["/g/a/v.css"])
    assert len([k for k in keys if k.startswith(b"localhost/g/a/v.css" + SEP)]) == 2
    assert lc.inspect(c, "?glob=%2A%2Fg%2Fa%2F%2A.js")[1]["matched"] == 5     # decoded once
    assert lc.inspect(c, "?glob=%252A.js")[1]["matched"] == 0
    assert lc.inspect(c, "?glob=localhost/g/q?x=*")[1]["matched"] == 1
    for bad in ("?glob=", "?glob=*", "?glob=**", "?glob=a%5C", "?glob=*&prefix=a",
                "?glob=a*&tag=x", "?glob=" + "a*" * 9, "?glob=" + "a" * 1025):
        assert lc.inspect(c, bad)[0] == 400, bad
    # the dry run counts and removes nothing
    st, d = glob_purge(c, "/g/a/*.css", dry=True)
    assert (st, d) == (200, {"mode": "glob", "dry_run": True, "matched": 8, "bytes": r["bytes"]})
    assert glob_purge(c, "/g/a/*.css", soft=True, dry=True)[1] == d          # (soft is ignored)
    for p in css:
        assert c.get(p).status() == 200
    assert all(hits(p) == 1 for p in css)
    # the hard form
    assert glob_purge(c, "/g/a/*.css") == (200, {"mode": "glob", "purged": 8})
    assert glob_purge(c, "/g/a/*.css") == (200, {"mode": "glob", "purged": 0})
    for p in css + js + other:
        assert c.get(p).status() == 200
    for h in langs:
        assert c.get("/g/a/v.css", headers=h).status() == 200
    assert all(hits(p) == 2 for p in css) and all(hits(p) == 1 for p in js + other)
    assert hits("/g/a/v.css") == 4                         # both variants went with their URL
    settle()
    # a '?' is literal: /g/q?x=1 goes, /g/qyx=1 stays
    assert glob_purge(c, "/g/q?x=*") == (200, {"mode": "glob", "purged": 1})
    c.get("/g/q?x=1").body().read(), c.get("/g/qyx=1").body().read()
    assert hits("/g/q?x=1") == 2 and hits("/g/qyx=1") == 1
    # a backslash in the URL is literal too (escaped before compiling): nothing matches, no 400
    assert glob_purge(c, "/g/a/*\\") == (200, {"mode": "glob", "purged": 0})
    # without grace a soft glob purge is a hard one, and says so
    assert glob_purge(c, "/g/b/*", soft=True) == (200, {"mode": "glob", "soft": False, "purged": 1})
    # refused patterns
    for bad in ("/" + "a*" * 9, "/" + "a" * 1100 + "*"):
        st, body = glob_purge(c, bad)
        assert st == 400 and b"error" in body and b"glob" in body, (bad[:12], st, body)
    st = px.stats()
    assert st["purge_glob_requests"] == 5 and st["purge_dry_runs"] == 2
    assert st["purged_objects"] == 10 and st["purge_requests"] == 7
    c.close()


def soft_glob_304_round_trip(px, be, origin, settle=lambda: None):
    """sc.soft_purge_304_round_trip with the glob matcher: /s/a.css is fetched through `px`
    (grace on, a long TTL: it is fresh), then soft-purged by `/s/*.css`: the next GET is
    answered from the cache at once while exactly one conditional request reaches the origin;
    its 304 touches the object in place and the GET after that is fresh again. /s/a.js is not
    touched. `origin` is a tg.TagOrigin."""
    from shellac_amd.utils.httpclient import HttpClient
    path = "/s/a.css"
    origin.cc304[path] = "max-age=60"
    c = HttpClient(port=px.port)
    for p in (path, "/s/a.js"):
        assert c.get(p).body().read() == origin.body(p)
    settle()
    assert c.get(path).body().read() == origin.body(path)            # fresh: a plain hit
    assert origin.seen(path) == [(path, None, 200)]
    assert glob_purge(c, "/s/*.css", soft=True) == (
        200, {"mode": "glob", "soft": True, "softened": 1})
    assert c.get(path).body().read() == origin.body(path)            # stale, at once
    log = origin.wait_seen(path, 2)
    assert log[1:] == [(path, '"v1"', 304)], log
    assert tc.wait_stat(px, "revalidate_touched", 1) == 1
    assert c.get(path).body().read() == origin.body(path)            # fresh again
    st = px.stats()
    assert {k: st[k] for k in tc.GRACE_COUNTERS} == {
        "stale_served": 1, "revalidations": 1, "revalidated_304": 1, "revalidate_touched": 1,
        "revalidate_restored": 0, "revalidate_errors": 0}
    assert origin.seen(path) == log and len(origin.seen("/s/a.js")) == 1
    assert st["softened_objects"] == 1 and st["soft_purge_requests"] == 1
    assert st["purge_glob_requests"] == 1 and st["purged_objects"] == 0
    assert glob_purge(c, "/s/*.css") == (200, {"mode": "glob", "purged": 1})
    assert be.get(b"localhost/s/a.js") is not None
    c.close()
