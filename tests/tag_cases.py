"""Scenarios shared by tests/test_tag_purge.py (CPU) and tests/test_tag_purge_gpu.py: a Python
model of the tag block and of a purge by tag, builders for tagged, hostile and truncated
values, the runs the twins (HostCache on the CPU, k_keyed_scan<TagMatch, RemoveAction> / k_keyed_scan<TagMatch, SoftenAction> on the GPU) are
checked with, and a small origin that emits a tag header. Every engine run takes explicit
`now` values, so nothing here waits for a clock."""
import gzip
import json
import struct
import threading
import time
from http.server import BaseHTTPRequestHandler, ThreadingHTTPServer

import purge_cases as pc
import soften_cases as sc
import touch_cases as tc
from shellac_amd import core
from shellac_amd.ops.cache import digest_strings, item_bytes, keyed, tag_hash, tagged

T0, TTL0, NOWS = tc.T0, tc.TTL0, tc.NOWS
M64 = 2 ** 64 - 1
TARGET = b"product-4711"          # the tag most runs purge
HTTP = b"HTTP/1.1 200 OK\r\nContent-Length: 2\r\n\r\nok"
VARY_MARKER = b"\x01accept-encoding"


# ---- the model: the tag block of csrc/keyed.h, parsed in Python
def block(hashes):
    """[0x02 | ntags | hashes], built here and not by the code under test."""
    return b"\x02" + bytes([len(hashes)]) + b"".join(struct.pack("<Q", h) for h in hashes)


def value_matches(value, hashes):
    """Whether a purge of the tag hashes `hashes` matches the keyed value `value`."""
    if len(value) < 4:
        return False
    o = 2 + struct.unpack("<H", value[:2])[0]
    if o + 2 > len(value) or value[o] != 0x02:
        return False
    nt = value[o + 1]
    if nt == 0xFF:
        return True
    if nt > 32 or o + 2 + 8 * nt > len(value):
        return False
    stored = struct.unpack("<%dQ" % nt, value[o + 2:o + 2 + 8 * nt])
    return any(h in hashes for h in stored)


def model_purge(objs, live, tags):
    """(count, item bytes, survivors) a purge of `tags` must give on the live set."""
    hs = {tag_hash(t) for t in tags}
    gone = {k for k in live if value_matches(objs[k], hs)}
    return len(gone), sum(item_bytes(len(objs[k])) for k in gone), live - gone


def live_values(sh, keys, now=None, batch=1024):
    """{key: value} of the keys that hit."""
    keys = list(keys)
    if now is not None:
        return {k: v for k, (v, _, _) in tc.records_at(sh, keys, now).items()}
    got = {}
    for i in range(0, len(keys), batch):
        ks = keys[i:i + batch]
        got.update({k: v for k, v in zip(ks, sh.get_many(ks)) if v is not None})
    return got


def equalise_live(shards, objs):
    """test_purge_gpu._check_twins' equalisation for any number of shards: the keys only some
    hold (an insert at a high index load evicts a live entry, and which one depends on the
    order of the inserts) are DELETEd; the cap is the existing one. Returns the common set."""
    lives = [set(live_values(sh, objs)) for sh in shards]
    common = set.intersection(*lives)
    assert len(common) >= 0.99 * max(len(l) for l in lives)
    for sh, live in zip(shards, lives):
        extra = sorted(live - common)
        if extra:
            assert sh.remove(digest_strings(extra, sh.device)).all()
    return common


def check_purge(shards, objs, live, tags):
    """Purge `tags` on every shard (they hold the same live set): count, bytes and survivors
    are the model's, and the surviving objects are bit-identical to what was stored."""
    want_n, want_bytes, survivors = model_purge(objs, live, tags)
    for sh in shards:
        before = sh.counters()["purged"]
        assert sh.remove_keyed_tags(tags) == (want_n, want_bytes), (sh.device, tags)
        after = live_values(sh, objs)
        assert set(after) == survivors, (sh.device, tags, set(after) ^ survivors)
        assert all(after[k] == objs[k] for k in survivors), (sh.device, tags)
        assert sh.counters()["purged"] - before == want_n
    return want_n, survivors


def make_shards(devices, objs=None, **kw):
    shards = [pc.make_shard(d, **kw) for d in devices]
    for sh in shards:
        if objs:
            pc.store(sh, objs)
    return shards


# ---- builders
def key_of_len(klen, idx):
    """A key of exactly `klen` bytes, distinct per idx (idx < 190)."""
    return bytes([33 + idx]) + (b"/key/of/some/length/that/goes/on/and/on/for/a/while")[:klen - 1]


def other_tags(n, salt):
    return [b"other-%d-%d" % (salt, i) for i in range(n)]


def alignment_objects():
    """Key lengths 1..40, so the block's offset (2 + klen) mod 16 takes every value and the
    header, ntags and each hash straddle granule and dword boundaries in every way; 1, 2 and
    32 tags; TARGET first, last, in the middle, and absent. {key: value}."""
    objs = {}
    for klen in range(1, 41):
        idx = 0
        for nt in (1, 2, 32):
            places = {0, nt - 1, nt // 2, None}
            for at in sorted(places, key=lambda p: -1 if p is None else p):
                tags = other_tags(nt, klen * 100 + idx)
                if at is not None:
                    tags[at] = TARGET
                k = key_of_len(klen, idx)
                idx += 1
                assert k not in objs and len(k) == klen
                objs[k] = keyed(k, tagged(tags, HTTP + b"%d" % klen))
                assert value_matches(objs[k], {tag_hash(TARGET)}) == (at is not None)
    return objs


BLOCK_KLENS = [1, 5, 12, 13, 14, 29, 30, 31]


def block_form_objects():
    """({key: value}, the keys a purge of TARGET must remove): well-formed, empty, overflow,
    malformed and truncated blocks and untagged payloads, each at key lengths that put the
    block's two header bytes in one granule, across two, and at a granule's end."""
    t = tag_hash(TARGET)
    forms = {
        "one": (block([t]) + HTTP, True),
        "nt0": (b"\x02\x00" + HTTP, False),                       # no tags: never matches
        "overflow": (b"\x02\xff" + HTTP, True),                   # matches any list
        "overflow-bare": (b"\x02\xff", True),
        "nt33": (b"\x02" + bytes([33]) + struct.pack("<Q", t) * 33 + HTTP, False),
        "nt254": (b"\x02" + bytes([254]) + struct.pack("<Q", t) * 254 + HTTP, False),
        "cut-in-hashes": (b"\x02\x04" + struct.pack("<Q", t) + b"\x00" * 5, False),
        "cut-after-key": (b"", False),
        "cut-after-marker": (b"\x02", False),
        "plain-02": (b"\x02\x01" + struct.pack("<Q", t)[:7], False),   # too few bytes follow
        "http": (HTTP, False),
        "vary-marker": (VARY_MARKER, False),
        "http-then-hash": (b"HTTP/" + block([t]), False),
    }
    objs, must_go = {}, set()
    for klen in BLOCK_KLENS:
        for idx, (name, (payload, goes)) in enumerate(forms.items()):
            k = key_of_len(klen, 20 + idx)            # (apart from alignment_objects' keys)
            objs[k] = keyed(k, payload)
            if goes:
                must_go.add(k)
    return objs, must_go


def near_miss_objects():
    """Stored hashes one bit away from TARGET's, in the low and in the high dword (and in
    every byte of the hash), beside exact ones. ({key: value}, the keys that match TARGET)."""
    t = tag_hash(TARGET)
    objs, must_go = {}, set()
    for klen in (7, 13, 14, 15, 16):
        for idx, bit in enumerate([0, 7, 8, 31, 32, 33, 56, 63, None]):
            k = key_of_len(klen, 40 + idx)
            hs = [tag_hash(b"a"), t if bit is None else t ^ (1 << bit), tag_hash(b"b")]
            objs[k] = keyed(k, block(hs) + HTTP)
            if bit is None:
                must_go.add(k)
    return objs, must_go


def tagged_families(n, seed=7):
    """pc.family_objects with tag blocks: object i carries its family's tag, `mod-<i % 16>`
    and two tags of its own. {key: value}."""
    plain = pc.family_objects(n, seed=seed)
    objs = {}
    for i, k in enumerate(plain):
        fam = next(f for f in pc.FAMILIES if k.startswith(f))
        payload = plain[k][2 + len(k):]
        objs[k] = keyed(k, tagged([b"fam:" + fam, b"mod-%d" % (i % 16), b"own-%d" % i,
                                   b"own2-%d" % i], payload))
    return objs


# ---- the soft form: sc.check_soften's contract with the tag matcher
def model_soften(model, objs, tags, stale_at, expire_cap, now):
    hs = {tag_hash(t) for t in tags}
    out, n = dict(model), 0
    for k, (e, _) in model.items():
        if (e and e <= now) or not value_matches(objs[k], hs):
            continue
        n += 1
        if expire_cap and (e == 0 or e > expire_cap):
            e = expire_cap
        out[k] = (e, stale_at)
    return n, out


def check_soften(shards, objs, model, tags, expire_cap, stale_at=sc.STALE_AT, now=T0):
    """Soften `tags` on every shard (they hold the live set `model`): the count is the
    model's, twice in a row; afterwards flags, header expiry and liveness at NOWS are the
    model's for every object, and the objects that do not match are bit-identical."""
    hs = {tag_hash(t) for t in tags}
    want_n, model2 = model_soften(model, objs, tags, stale_at, expire_cap, now)
    want = sc.want_snapshot(objs, model2)
    for sh in shards:
        was = sc.snapshot(sh, objs)
        for _ in range(2):
            got = sh.soften_keyed_tags(tags, stale_at, expire_cap, now=now)
            assert got == want_n, (sh.device, tags, expire_cap, got, want_n)
        after = sc.snapshot(sh, objs)
        assert after == want, (sh.device, tags, expire_cap)
        for t in NOWS:
            for k, rec in was[t].items():
                if not value_matches(objs[k], hs):
                    assert after[t].get(k) == rec, (sh.device, t, k)
    return want_n, model2


# ---- CLOCK
def lap_the_log(sh, laps=1.25, now=None):
    head0 = sh.head()
    batch_no = 0
    while sh.head() < head0 + int(laps * sh.log_bytes):
        fill = {b"/fill/%d/%d" % (batch_no, i): keyed(b"/fill/%d/%d" % (batch_no, i), b"f" * 700)
                for i in range(200)}
        if now is None:
            pc.store(sh, fill, batch=200)
        else:
            tc.store_at(sh, fill, 0, now=now, batch=200)
        batch_no += 1


def clock_keeps_the_tags(sh):
    """Tagged objects that were read are re-appended by the CLOCK hand while SET batches lap
    the log: they keep their blocks, and a tag purge afterwards finds them. Returns (objects
    alive after the lap, the purge's count, alive after it, reinsertions)."""
    assert sh.evict == "clock"
    hot = {b"/hot/%d" % i: keyed(b"/hot/%d" % i, tagged([b"hot", b"n%d" % i], b"h" * 900))
           for i in range(20)}
    pc.store(sh, hot)
    for _ in range(2):
        assert live_values(sh, hot) == hot                      # reference bits set
    lap_the_log(sh)
    alive = live_values(sh, hot)
    assert all(alive[k] == hot[k] for k in alive)
    n = sh.remove_keyed_tags([b"hot"])[0]
    return len(alive), n, len(live_values(sh, hot)), sh.counters()["reinserted"]


def clock_never_resurrects(sh):
    """pc.clock_never_resurrects with a tag purge: purged objects whose reference bits were
    set stay misses while the hand passes their ring entries."""
    hot = {b"/hot/%d" % i: keyed(b"/hot/%d" % i, tagged([b"hot"], b"h" * 900)) for i in range(150)}
    cold = {b"/cold/%d" % i: keyed(b"/cold/%d" % i, tagged([b"cold"], b"c" * 900))
            for i in range(150)}
    pc.store(sh, hot)
    pc.store(sh, cold)
    for _ in range(2):
        assert set(live_values(sh, hot)) == set(hot)
        assert set(live_values(sh, cold)) == set(cold)
    assert sh.remove_keyed_tags([b"hot"])[0] == len(hot)
    written, batch_no = 0, 0
    while written < 3 * sh.log_bytes:
        fill = {b"/fill/%d/%d" % (batch_no, i): keyed(b"/fill/%d/%d" % (batch_no, i), b"f" * 700)
                for i in range(200)}
        pc.store(sh, fill, batch=200)
        written += sum(item_bytes(len(v)) for v in fill.values())
        batch_no += 1
        assert live_values(sh, hot) == {}
    c = sh.counters()
    assert c["reinserted"] > 0
    return c


def clock_keeps_the_softening(sh):
    """sc.clock_keeps_the_softening with the tag matcher."""
    assert sh.evict == "clock"
    hot = {b"/hot/%d" % i: keyed(b"/hot/%d" % i, tagged([b"hot"], b"h" * 900)) for i in range(20)}
    tc.store_at(sh, hot, T0 + 1000, flags=1)
    for _ in range(2):
        assert tc.live_at(sh, hot, T0) == set(hot)
    cap = T0 + TTL0
    assert sh.soften_keyed_tags([b"hot"], sc.STALE_AT, cap, now=T0) == 20
    lap_the_log(sh, now=T0)
    recs = tc.records_at(sh, hot, cap - 1)
    for k, (v, _, _) in recs.items():
        assert v == hot[k]
    return ({k: (f, e) for k, (_, f, e) in recs.items()}, tc.live_at(sh, hot, cap),
            sh.counters()["reinserted"])


def dead_entries(s):
    """test_dead_same_digest_entry_is_not_counted's shape: beside the live entry of a tagged
    object a dead one with its digest (expired, pointing at the very same record) and a
    locked slot. Returns (b2, the two made-up slots, loc)."""
    key = b"/twin/object"
    val = keyed(key, tagged([TARGET], b"t" * 100))
    s.set_many([b"/pre/%d" % i for i in range(3)], [keyed(b"/pre/%d" % i, b"p") for i in range(3)])
    s.set_many([key], [val])
    lo, hi = (int(x) & M64 for x in digest_strings([key], "cpu")[0])
    b1, b2 = core().bucket_pair(lo, hi, s.nbuckets)
    e1, e2 = s._impl.debug_bucket(b1), s._impl.debug_bucket(b2)
    i = next(k for k in range(4) if e1[4 * k] == lo and e1[4 * k + 1] == hi and e1[4 * k + 2])
    free = [k for k in range(4) if e2[4 * k + 2] == 0]
    loc, vx = e1[4 * i + 2], e1[4 * i + 3]
    s._impl.debug_set_entry(b2, free[0], lo, hi, loc, vx & 0xFFFFFFFF, 1)      # expired at t=1
    s._impl.debug_set_entry(b2, free[1], lo, hi, M64 - 1, vx & 0xFFFFFFFF, 0)  # locked
    return key, val, b2, free, loc


# ---- the proxy
TAG_HEADER = "Surrogate-Key"


class TagOrigin:
    """A small origin that emits a tag header. Per path: `tags` (the header's value; absent:
    no header), `delays` (seconds between logging the request and answering), `gzip` (the
    body goes out gzip-coded), `vary` (a Vary header's value). Every path serves `body <path>` with an ETag and answers
    a matching If-None-Match with 304."""

    def __init__(self, header=TAG_HEADER):
        self.tags, self.delays, self.gzip, self.vary = {}, {}, set(), {}
        self.cc304 = {}
        self.log = []          # (path, If-None-Match or None, status sent)
        self.lock = threading.Lock()
        outer = self

        class Handler(BaseHTTPRequestHandler):
            protocol_version = "HTTP/1.1"

            def do_GET(self):
                path = self.path
                inm = self.headers.get("If-None-Match")
                status = 304 if inm == '"v1"' else 200
                with outer.lock:                    # (logged on arrival, before any delay)
                    outer.log.append((path, inm, status))
                if outer.delays.get(path):
                    time.sleep(outer.delays[path])
                body = b"" if status == 304 else outer.wire_body(path)
                self.send_response(status)
                self.send_header("ETag", '"v1"')
                if path in outer.tags:
                    self.send_header(header, outer.tags[path])
                if status == 304:
                    if path in outer.cc304:
                        self.send_header("Cache-Control", outer.cc304[path])
                else:
                    if path in outer.vary:
                        self.send_header("Vary", outer.vary[path])
                    if path in outer.gzip:
                        self.send_header("Content-Encoding", "gzip")
                    self.send_header("Content-Type", "text/plain")
                    self.send_header("Content-Length", str(len(body)))
                self.end_headers()
                if body:
                    self.wfile.write(body)

            def log_message(self, *a):
                pass

        self._srv = ThreadingHTTPServer(("127.0.0.1", 0), Handler)
        self._srv.daemon_threads = True
        self.port = self._srv.server_address[1]
        self._th = threading.Thread(target=self._srv.serve_forever, daemon=True)

    @staticmethod
    def body(path):
        return f"body {path} ".encode() * 8

    def wire_body(self, path):
        return gzip.compress(self.body(path), mtime=0) if path in self.gzip else self.body(path)

    def seen(self, path):
        with self.lock:
            return [e for e in self.log if e[0] == path]

    def wait_seen(self, path, n, timeout=5.0):
        deadline = time.time() + timeout
        while len(self.seen(path)) < n and time.time() < deadline:
            time.sleep(0.005)
        return self.seen(path)

    def start(self):
        self._th.start()
        return self

    def stop(self):
        self._srv.shutdown()
        self._srv.server_close()


def tag_purge(c, tags, soft=False, header=TAG_HEADER, path="/ignored"):
    headers = {"X-Purge-Mode": "tag"}
    if tags is not None:
        headers[header] = tags
    if soft:
        headers["X-Purge-Soft"] = "1"
    r = c.get(path, method="PURGE", headers=headers)
    body = r.body().read()
    return r.status(), (json.loads(body) if r.status() == 200 else body)


def fetch(c, path, headers=None):
    """(status, headers without the per-response ones, body) of a GET."""
    r = c.get(path, headers=headers)
    body = r.body().read()
    hdrs = {k.lower(): v for k, v in r.headers().items() if k.lower() not in ("date", "age")}
    return r.status(), hdrs, body


# ---- the engine runs both test files make (CPU: the host twin; GPU: the kernel and the twin)
def run_alignment_sweep(devices):
    objs = alignment_objects()
    shards = make_shards(devices, objs)
    live = equalise_live(shards, objs)
    assert live == set(objs)
    n, survivors = check_purge(shards, objs, live, [TARGET])
    assert n == 40 * 6 and len(survivors) == 40 * 3     # per klen: 1 + 2 + 3 carry TARGET
    assert check_purge(shards, objs, survivors, [TARGET])[0] == 0
    # what is left goes by its own tags: a list of two, the second matching
    k = sorted(survivors)[0]
    klen = len(k)
    assert check_purge(shards, objs, survivors, [b"nobody", b"other-%d-0" % (klen * 100)])[0] == 1


def run_block_forms(devices):
    objs, must_go = block_form_objects()
    shards = make_shards(devices, objs)
    live = equalise_live(shards, objs)
    assert live == set(objs)
    # a list that names nothing stored: the overflow blocks alone match
    over = {k for k in objs if objs[k][2 + len(k):2 + len(k) + 2] == b"\x02\xff"}
    assert len(over) == 2 * len(BLOCK_KLENS)
    fresh = make_shards(devices, objs)
    n, left = check_purge(fresh, objs, live, [b"no-such-tag"])
    assert n == len(over) and left == live - over
    n, left = check_purge(shards, objs, live, [TARGET])
    assert n == len(must_go) and left == live - must_go
    assert check_purge(shards, objs, left, [TARGET, b"x", b"y"])[0] == 0


def run_garbage(devices):
    junk = pc.garbage_values()
    shards = make_shards(devices, junk)
    before = [sh.get_many(list(junk)) for sh in shards]
    for tags in ([TARGET], [b"a", b"b"], [b"t%d" % i for i in range(64)]):
        want = model_purge(junk, set(junk), tags)[:2]
        assert want == (0, 0)
        for sh in shards:
            assert sh.remove_keyed_tags(tags) == want, (sh.device, tags)
            assert sh.soften_keyed_tags(tags, 77, T0 + 50, now=T0) == 0
    assert [sh.get_many(list(junk)) for sh in shards] == before


def run_near_misses(devices):
    objs, must_go = near_miss_objects()
    decoys = [b"decoy-%d" % i for i in range(63)]
    for tags in ([TARGET], [b"decoy", TARGET], decoys + [TARGET], [TARGET, TARGET],
                 [TARGET, b"a"], [b"a", b"b", TARGET, b"a"]):
        shards = make_shards(devices, objs)
        live = equalise_live(shards, objs)
        n, _ = check_purge(shards, objs, live, tags)
        # (an object that matches several list entries counts once: b"a" is on every object)
        assert n == (len(objs) if b"a" in tags else len(must_go)), tags
    for sh in make_shards(devices):
        for bad in ([], [b"t%d" % i for i in range(65)]):
            for call in (lambda: sh.remove_keyed_tags(bad),
                         lambda: sh.soften_keyed_tags(bad, 5)):
                try:
                    call()
                except Exception:
                    continue
                raise AssertionError("a list of %d tags was taken" % len(bad))
        try:
            sh.soften_keyed_tags([b"a"], 1, expire_cap=T0, now=T0)
        except Exception:
            continue
        raise AssertionError("a cap at now was taken")


def run_families(devices, n=3000):
    """~3000 tagged objects in 4096 index slots (relocated entries are scanned too), purged
    family by family, by a shared tag, then the rest."""
    objs = tagged_families(n)
    shards = make_shards(devices, objs)
    live = equalise_live(shards, objs)
    assert len(live) > 0.96 * n
    total = 0
    for tags in ([b"fam:/static/js/"], [b"nothing"], [b"mod-3", b"mod-11"],
                 [b"fam:" + f for f in pc.FAMILIES]):
        got, live = check_purge(shards, objs, live, tags)
        total += got
    assert live == set() and total > 0.96 * n
    assert all(sh.sweep()[0] == 0 for sh in shards)


def run_after_the_log_lapped(devices):
    plain = pc.family_objects(6000, seed=11, max_payload=1500)
    objs = {k: keyed(k, tagged([b"fam:" + next(f for f in pc.FAMILIES if k.startswith(f))],
                               v[2 + len(k):])) for k, v in plain.items()}
    shards = make_shards(devices, objs)
    assert len({sh.head() for sh in shards}) == 1 and shards[0].head() > 3 * shards[0].log_bytes
    live = equalise_live(shards, objs)
    assert 0 < len(live) < len(objs) // 2
    n, _ = check_purge(shards, objs, live, [b"fam:/static/"])
    assert 0 < n < len(live)


def run_expired_are_not_counted(devices):
    for sh in make_shards(devices):
        fresh = {b"/x/keep/%d" % i: keyed(b"/x/keep/%d" % i, tagged([b"x"], b"v"))
                 for i in range(10)}
        dying = {b"/x/ttl/%d" % i: keyed(b"/x/ttl/%d" % i, tagged([b"x"], b"v"))
                 for i in range(7)}
        pc.store(sh, fresh)
        pc.store(sh, dying, ttl=5)
        assert sh.soften_keyed_tags([b"x"], 9, now=sh.now() + 100) == len(fresh)
        assert sh.remove_keyed_tags([b"x"], now=sh.now() + 100)[0] == len(fresh)


def run_dead_entries(devices):
    for sh in make_shards(devices):
        key, val, b2, free, loc = dead_entries(sh)
        assert sh.remove_keyed_tags([TARGET]) == (1, item_bytes(len(val)))
        assert sh.counters()["purged"] == 1
        after = sh._impl.debug_bucket(b2)
        assert after[4 * free[0] + 2] == loc and after[4 * free[1] + 2] == M64 - 1  # left alone
        assert sh.get_many([key]) == [None]
    for sh in make_shards(devices):
        key, val, b2, free, loc = dead_entries(sh)
        before = sh._impl.debug_bucket(b2)
        assert sh.soften_keyed_tags([TARGET], 9) == 1     # (flags only: the entry's words stay)
        assert sh._impl.debug_bucket(b2) == before
        assert sh.get_many([key]) == [val]


def run_soft_form(devices):
    objs = {**block_form_objects()[0], **alignment_objects()}
    for cap in sc.CAPS:
        shards = make_shards(devices)
        for sh in shards:
            sc.store_mixed(sh, objs)
        models = [sc.model_of(sh, objs) for sh in shards]
        assert all(m == models[0] for m in models) and set(models[0]) == set(objs)
        n, model = check_soften(shards, objs, models[0], [TARGET], cap)
        assert n == 240 + 3 * len(BLOCK_KLENS)
        # a second pass with another list: lives are only ever shortened
        n2, model = check_soften(shards, objs, model, [b"no-such", TARGET], T0 + 10 ** 6,
                                 stale_at=sc.STALE_AT + 1)
        assert n2 <= n
        if cap:
            assert all(e for k, (e, f) in model.items() if f == sc.STALE_AT + 1)


def run_reference_bit(devices):
    for sh in make_shards(devices):
        objs = {k: keyed(k, tagged([b"ref"], b"v" * 40)) for k in (b"/ref/read", b"/ref/unread")}
        tc.store_at(sh, objs, T0 + 500, flags=1)
        assert tc.live_at(sh, {b"/ref/read": objs[b"/ref/read"]}, T0)
        assert tc.ref_bit(sh, b"/ref/read") == (True, T0 + 500)
        assert sh.soften_keyed_tags([b"ref"], 5, T0 + 100, now=T0) == 2
        assert tc.ref_bit(sh, b"/ref/read") == (True, T0 + 100)
        assert tc.ref_bit(sh, b"/ref/unread") == (False, T0 + 100)
        assert tc.records_at(sh, objs, T0 + 99) == {k: (v, 5, T0 + 100) for k, v in objs.items()}
        assert tc.records_at(sh, objs, T0 + 100) == {}


def run_refused_while_phase1_pending(devices):
    from shellac_amd.ops.cache import pack_values
    for sh in make_shards(devices):
        objs = {b"/p/%d" % i: keyed(b"/p/%d" % i, tagged([b"p"], b"v")) for i in range(4)}
        keys = list(objs)
        d = digest_strings(keys, sh.device)
        v, vo, vl = pack_values([objs[k] for k in keys], sh.device)
        ex = tc.i32([0] * 4, sh.device)
        sh.store(d, v, vo, vl, None, ex, now=T0, phase=1)
        try:
            sh.soften_keyed_tags([b"p"], 5, now=T0)
        except Exception as e:
            assert "phase-1" in str(e)
        else:
            raise AssertionError("softened while a phase-1 batch was pending")
        sh.store(d, v, vo, vl, None, ex, now=T0, phase=2)
        assert sh.soften_keyed_tags([b"p"], 5, T0 + 9, now=T0) == 4
        assert sc.model_of(sh, objs) == {k: (T0 + 9, 5) for k in keys}


def purge_by_tag_round_trip(px, origin, settle=lambda paths: None, prefix="localhost"):
    """Paths tagged `x y`, `y`, untagged, and with 40 tags are filled through the proxy; PURGE
    tag `y` removes the first, the second and the overflowing one (purged: 3); the untagged
    one still hits; each purged one is fetched again exactly once."""
    from shellac_amd.utils.httpclient import HttpClient
    origin.tags.update({"/t/xy": "x y", "/t/y": "y",
                        "/t/many": " ".join("m%d" % i for i in range(40))})
    paths = ["/t/xy", "/t/y", "/t/none", "/t/many"]
    c = HttpClient(port=px.port)
    for p in paths:
        assert c.get(p).body().read() == origin.body(p)
    settle(paths)
    for p in paths:
        assert c.get(p).body().read() == origin.body(p)
    assert all(len(origin.seen(p)) == 1 for p in paths)
    assert tag_purge(c, "y") == (200, {"mode": "tag", "tags": 1, "purged": 3})
    for _ in range(2):
        for p in paths:
            assert c.get(p).body().read() == origin.body(p)
        settle(paths)
    assert [len(origin.seen(p)) for p in paths] == [2, 2, 1, 2]
    assert tag_purge(c, "nobody-has-this, nor-this") == (200, {"mode": "tag", "tags": 2,
                                                               "purged": 1})   # the overflow
    st = px.stats()
    assert st["tag_purge_requests"] == 2 and st["tag_purged_objects"] == 4
    assert st["tagged_fills"] == 3 + 3 and st["purged_objects"] == 0
    c.close()
