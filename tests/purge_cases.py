"""Scenarios shared by tests/test_purge.py (CPU) and tests/test_purge_gpu.py: keyed objects
over a handful of path families, a Python model of a prefix purge, and the runs both twins
(HostCache on the CPU, k_keyed_scan<PrefixMatch, RemoveAction> on the GPU) are checked with."""
import json
import random
import struct

from shellac_amd.ops.cache import CacheShard, item_bytes, keyed
from shellac_amd.utils.httpclient import HttpClient

FAMILIES = [b"/static/js/", b"/static/css/", b"/static/", b"/api/v1/users/", b"/api/v2/",
            b"/img/", b"/"]

# prefix lengths at the 16-byte granule boundaries of a key that starts at value byte 2:
# granule 0 ends after key byte 13, granule 1 after 29, granule 2 after 45
BOUNDARY_PLENS = [1, 13, 14, 15, 16, 17, 29, 30, 31, 46, 47, 300]


def make_shard(device="cpu", **kw):
    kw.setdefault("log_bytes", 1 << 20)
    kw.setdefault("nbuckets", 1 << 10)
    kw.setdefault("max_item", 4096)
    return CacheShard(device=device, **kw)


def family_objects(n, seed=7, max_payload=300):
    """n distinct keyed objects: {key: keyed value} with URL-shaped keys over FAMILIES."""
    rng = random.Random(seed)
    objs = {}
    while len(objs) < n:
        fam = rng.choice(FAMILIES)
        key = fam + b"%x/%d.html" % (rng.getrandbits(24), len(objs))
        objs[key] = keyed(key, bytes(rng.getrandbits(8) for _ in range(rng.randint(0, max_payload))))
    return objs


def store(shard, objs, batch=512, ttl=0):
    keys = list(objs)
    for i in range(0, len(keys), batch):
        ks = keys[i:i + batch]
        shard.set_many(ks, [objs[k] for k in ks], ttl=ttl)


def live_keys(shard, keys, batch=1024):
    """The keys that hit now (and the bytes they return must be what was stored)."""
    keys = list(keys)
    live = set()
    for i in range(0, len(keys), batch):
        ks = keys[i:i + batch]
        for k, v in zip(ks, shard.get_many(ks)):
            if v is not None:
                live.add(k)
    return live


def model_purge(objs, live, prefix):
    """(count, item bytes, survivors) a purge of `prefix` must give on the live set."""
    gone = {k for k in live if k.startswith(prefix)}
    return len(gone), sum(item_bytes(len(objs[k])) for k in gone), live - gone


def boundary_objects(plen, seed=3):
    """For a pattern of `plen` bytes: (pattern, objects, the keys the purge must remove)."""
    rng = random.Random(seed * 1000 + plen)
    pat = b"/" + bytes(rng.choice(b"abcdefghijklmnopqrstuvwxyz0123456789") for _ in range(plen - 1))
    flip = lambda b, i: b[:i] + bytes([b[i] ^ 0x01]) + b[i + 1:]
    cases = {
        "equal": pat,                             # a key equal to the pattern: removed
        "longer": pat + b"tail/x.html",           # removed
        "longer1": pat + b"Z",                    # removed
        "first": flip(pat, 0) + b"tail",          # differs in the first pattern byte only
        "last": flip(pat, plen - 1) + b"tail",    # differs in the last pattern byte only
    }
    if plen > 1:
        cases["short"] = pat[:-1]                 # shorter than the pattern, equal to its head
    objs = {key: keyed(key, b"payload-" + name.encode() * (plen % 7))
            for name, key in cases.items()}
    if plen > 2:
        # the key is the pattern's head and the payload continues like the pattern (the
        # value's bytes [2, 2 + plen) equal the pattern): the compare is bounded by klen
        head = pat[:plen // 2]
        objs[head] = keyed(head, pat[len(head):] + b"more")
    must_go = {cases["equal"], cases["longer"], cases["longer1"]}
    return pat, objs, must_go


def garbage_values():
    """Non-keyed values a purge must survive: empty, one byte, a klen larger than the
    value, klen exactly past the end, 0xff fill."""
    return {
        b"garbage/empty": b"",
        b"garbage/one": b"/",
        b"garbage/klen-huge": struct.pack("<H", 5000) + b"/abc" * 3,
        b"garbage/klen-past-end": struct.pack("<H", 11) + b"/abcdefghi",   # 2 + 11 > 12
        b"garbage/ff": b"\xff" * 40,
        b"garbage/two": struct.pack("<H", 0),
    }


def clock_never_resurrects(sh):
    """Objects whose reference bits are set are purged; SET batches then drive the CLOCK
    hand over their ring entries (well past a lap of the log): they stay misses."""
    hot = {b"/hot/%d" % i: keyed(b"/hot/%d" % i, b"h" * 900) for i in range(150)}
    cold = {b"/cold/%d" % i: keyed(b"/cold/%d" % i, b"c" * 900) for i in range(150)}
    store(sh, hot)
    store(sh, cold)
    for _ in range(2):
        assert live_keys(sh, hot) == set(hot)      # reference bits set
        assert live_keys(sh, cold) == set(cold)
    assert sh.remove_keyed_prefix(b"/hot/")[0] == len(hot)
    written = 0
    batch_no = 0
    while written < 3 * sh.log_bytes:
        fill = {b"/fill/%d/%d" % (batch_no, i): keyed(b"/fill/%d/%d" % (batch_no, i), b"f" * 700)
                for i in range(200)}
        store(sh, fill, batch=200)
        written += sum(item_bytes(len(v)) for v in fill.values())
        batch_no += 1
        assert live_keys(sh, hot) == set()
    c = sh.counters()
    assert c["reinserted"] > 0   # the hand did give second chances (to the cold, read set)
    return c


# ---- the proxy's PURGE method
def purge(c, path, prefix=False):
    r = c.get(path, method="PURGE", headers={"X-Purge-Mode": "prefix"} if prefix else None)
    body = r.body().read()
    return r.status(), (json.loads(body) if r.status() == 200 else body)


def prefix_purge_round_trip(px, origin, settle=lambda: None):
    """Fill /a/1..20 and /b/1..20 through the proxy, PURGE /a/ in prefix mode, then an exact
    PURGE. `settle` runs after each round of fills (an asynchronous tier stores them a
    moment after the responses)."""
    c = HttpClient(port=px.port)
    a = [f"/a/{i}" for i in range(1, 21)]
    b = [f"/b/{i}" for i in range(1, 21)]
    for p in a + b:
        assert c.get(p).status() == 200
    settle()
    for p in a + b:
        assert c.get(p).status() == 200
    assert all(origin.hits[p] == 1 for p in a + b)
    assert purge(c, "/a/", prefix=True) == (200, {"mode": "prefix", "purged": 20})
    for p in a + b:
        assert f"<html>{p} #".encode() in c.get(p).body().read()
    assert all(origin.hits[p] == 2 for p in a), origin.hits
    assert all(origin.hits[p] == 1 for p in b), origin.hits
    settle()
    # exact purge of one URL
    assert purge(c, "/b/3") == (200, {"mode": "exact", "found": True, "variants": 0})
    assert purge(c, "/b/3") == (200, {"mode": "exact", "found": False, "variants": 0})
    c.get("/b/3")
    c.get("/b/30")
    assert origin.hits["/b/3"] == 2 and origin.hits["/b/2"] == 1
    st = px.stats()
    assert st["purge_requests"] == 3 and st["purged_objects"] == 21
    c.close()
