"""Scenarios shared by tests/test_touch.py (CPU) and tests/test_touch_gpu.py: keyed objects
with expiries, a Python model of an in-place touch, and the runs both twins (HostCache on the
CPU, k_touch on the GPU) are checked with. Every run takes explicit `now` values, so nothing
here waits for a clock."""
import random
import struct
import threading
import time
from http.server import BaseHTTPRequestHandler, ThreadingHTTPServer

import numpy as np
import torch

import purge_cases as pc
from shellac_amd.ops.cache import (digest_strings, item_bytes, keyed, pack_bytes, pack_values,
                                   unpack_records)

T0 = 10          # the `now` objects are stored at
TTL0 = 100       # ... with this TTL: they expire at T0 + TTL0
M64 = 2 ** 64 - 1
REF_BIT = 1 << 31


def i32(values, device):
    """uint32 values as the int32 tensor the shard takes."""
    return torch.from_numpy(np.asarray(values, dtype=np.uint32).view(np.int32).copy()).to(device)


def key_tensors(keys, device):
    buf, offs = pack_bytes(list(keys))
    buf = np.ascontiguousarray(buf) if buf.size else np.zeros(1, np.uint8)
    return torch.from_numpy(buf.copy()).to(device), torch.from_numpy(offs).to(device)


def store_at(sh, objs, expire, now=T0, flags=0, digests=None, batch=512):
    """Store {key: value} with one absolute expiry at `now`. `digests`: {key: the key whose
    digest the value is stored under} (a forged collision)."""
    keys = list(objs)
    for i in range(0, len(keys), batch):
        ks = keys[i:i + batch]
        d = digest_strings([digests.get(k, k) if digests else k for k in ks], sh.device)
        v, vo, vl = pack_values([objs[k] for k in ks], sh.device)
        sh.store(d, v, vo, vl, i32([flags] * len(ks), sh.device), i32([expire] * len(ks), sh.device),
                 now=now)


def touch(sh, keys, expire, flags=None, key_bytes=True, now=T0, digest_of=None):
    """Touch `keys` (byte strings) to the absolute expiries `expire`; returns hit as a list.
    `key_bytes` False: digests only. `digest_of`: the keys whose digests the rows carry (a
    forged collision: the row's key bytes are `keys`)."""
    keys = list(keys)
    d = digest_strings(digest_of if digest_of is not None else keys, sh.device)
    hit = sh.touch(d, i32(expire, sh.device),
                   None if flags is None else i32(flags, sh.device),
                   key_tensors(keys, sh.device) if key_bytes else None, now=now)
    return [int(x) for x in hit.tolist()]


def records_at(sh, keys, now, batch=2048):
    """{key: (value, flags, header expire)} of the keys that hit at `now`."""
    keys = list(keys)
    got = {}
    for i in range(0, len(keys), batch):
        ks = keys[i:i + batch]
        out, off, size = sh.get(digest_strings(ks, sh.device), now=now)
        o, offs = out.cpu().numpy(), off.cpu().numpy()
        for k, o_i, r in zip(ks, offs, unpack_records(out, off, size)):
            if r is not None:
                hdr = o[int(o_i):int(o_i) + 32].view(np.uint32)
                got[k] = (r[0], r[1], int(hdr[6]))
    return got


def live_at(sh, objs, now):
    """The keys of `objs` that hit at `now`; what they return must be what was stored."""
    got = records_at(sh, objs, now)
    for k, (v, _, _) in got.items():
        assert v == objs[k], k
    return set(got)


def model_live(model, now):
    return {k for k, (e, _) in model.items() if e == 0 or e > now}


NOWS = [T0, T0 + 49, T0 + 50, T0 + 99, T0 + 100, T0 + 499, T0 + 500, T0 + 100000]


def mixed_touch(sh, n=1000, seed=21):
    """n keyed objects that expire at T0 + TTL0; a seeded half of them (and some keys that
    were never stored) is touched to mixed expiries — never, sooner, later, the past, `now`
    itself — with new flags. Returns what the shard answered and the model's view:
    (hit, the model's hit, {now: live set}, {now: the model's live set}, touched counter,
    {key: (flags, header expire)} of the survivors at T0)."""
    objs = pc.family_objects(n, seed=seed)
    store_at(sh, objs, T0 + TTL0, flags=1)
    assert live_at(sh, objs, T0) == set(objs)      # precondition: no insert lost a key
    rng = random.Random(seed)
    model = {k: (T0 + TTL0, 1) for k in objs}
    picked = rng.sample(sorted(objs), n // 2) + [b"/never/stored/%d" % i for i in range(37)]
    rng.shuffle(picked)
    choices = [0, T0 + 50, T0 + 500, T0 - 5, T0]
    exp = [rng.choice(choices) for _ in picked]
    fl = [rng.getrandbits(32) for _ in picked]
    hit = touch(sh, picked, exp, fl)
    want = []
    for k, e, f in zip(picked, exp, fl):
        want.append(1 if k in model else 0)
        if k in model:
            model[k] = (e, f)
    live = {t: live_at(sh, objs, t) for t in NOWS}
    want_live = {t: model_live(model, t) for t in NOWS}
    meta = {k: (f, e) for k, (_, f, e) in records_at(sh, objs, T0).items()}
    assert meta == {k: (model[k][1], model[k][0]) for k in want_live[T0]}
    return hit, want, live, want_live, sh.counters()["touched"], meta


def forged_collision(sh):
    """A value keyed with B stored under A's digest: a touch of A that gives A's key bytes
    must miss and leave the expiry alone; the digest alone hits."""
    a, b = b"/victim/object", b"/attacker/object"
    objs = {b: keyed(b, b"payload of b")}
    store_at(sh, objs, T0 + TTL0, digests={b: a})
    d_a = digest_strings([a], sh.device)

    def alive(now):
        return bool((sh.get(d_a, now=now)[2] > 0).item())
    assert alive(T0 + TTL0 - 1) and not alive(T0 + TTL0)
    out = [touch(sh, [a], [T0 + 500])]                        # A's bytes: not A's record
    out.append((alive(T0 + TTL0 - 1), alive(T0 + TTL0)))      # unchanged
    out.append(touch(sh, [b], [T0 + 500], digest_of=[a]))     # B's bytes under A's digest: hit
    out.append((alive(T0 + 499), alive(T0 + 500)))
    out.append(touch(sh, [a], [0], key_bytes=False))          # the digest alone decides
    out.append(alive(T0 + 10 ** 6))
    out.append(sh.counters()["touched"])
    return out


FORGED_WANT = [[0], (True, False), [1], (True, False), [1], True, 2]


def dead_entries(sh):
    """Expired, deleted, purged and lapped objects: a touch misses and revives nothing. The
    shard must be FIFO with a 256 KiB log, so the lap is exact."""
    assert sh.evict == "fifo" and sh.log_bytes == 256 << 10
    fam = {name: {b"/%s/%d" % (name, i): keyed(b"/%s/%d" % (name, i), name * 20) for i in range(8)}
           for name in (b"lapped", b"expired", b"deleted", b"purged", b"alive")}
    store_at(sh, fam[b"lapped"], 0)
    fill = {b"/fill/%d" % i: keyed(b"/fill/%d" % i, b"f" * 1000) for i in range(300)}
    store_at(sh, fill, 0, batch=100)                          # > one lap of the log
    assert sh.head() > sh.log_bytes + 8 * item_bytes(200)
    store_at(sh, fam[b"expired"], T0 + 5)
    for name in (b"deleted", b"purged", b"alive"):
        store_at(sh, fam[name], T0 + TTL0)
    assert sh.remove(digest_strings(list(fam[b"deleted"]), sh.device)).all()
    assert sh.remove_keyed_prefix(b"/purged/", now=T0)[0] == 8
    now = T0 + 5                                              # the `expired` family just died
    keys = [k for name in fam for k in fam[name]]
    hit = touch(sh, keys, [0] * len(keys), now=now)
    hit2 = touch(sh, keys, [0] * len(keys), key_bytes=False, now=now)
    allobjs = {k: v for name in fam for k, v in fam[name].items()}
    live = live_at(sh, allobjs, now)
    want = [1 if k in fam[b"alive"] else 0 for k in keys]
    return hit, hit2, want, live, set(fam[b"alive"]), sh.counters()["touched"]


def clock_keeps_the_touch(sh):
    """Objects that were read (reference bit set) are touched to a later expiry and new
    flags, then SET batches lap the log, so the CLOCK hand re-appends them from their record
    headers: they come back with the new expiry and flags. Returns (live past the old expiry,
    {key: (flags, header expire)} there, live past the new one, reinsertions)."""
    assert sh.evict == "clock"
    hot = {b"/hot/%d" % i: keyed(b"/hot/%d" % i, b"h" * 900) for i in range(20)}
    store_at(sh, hot, T0 + TTL0, flags=1)
    for _ in range(2):
        assert live_at(sh, hot, T0) == set(hot)               # reference bits set
    new_exp, new_flags = T0 + 1000, 0xC0FFEE00
    assert touch(sh, list(hot), [new_exp] * 20, [new_flags] * 20) == [1] * 20
    head0 = sh.head()
    batch_no = 0
    while sh.head() < head0 + sh.log_bytes + (sh.log_bytes >> 2):
        fill = {b"/fill/%d/%d" % (batch_no, i): keyed(b"/fill/%d/%d" % (batch_no, i), b"f" * 700)
                for i in range(200)}
        store_at(sh, fill, 0, batch=200)
        batch_no += 1
    t = T0 + TTL0 + 50                                        # past the old expiry
    recs = records_at(sh, hot, t)
    for k, (v, _, _) in recs.items():
        assert v == hot[k]
    return (set(recs), {k: (f, e) for k, (_, f, e) in recs.items()},
            live_at(sh, hot, new_exp), sh.counters()["reinserted"])


def near_miss_keys(key):
    """Keys that differ from `key` by one byte: shorter, longer, last byte, first byte."""
    flip = lambda b, i: b[:i] + bytes([b[i] ^ 0x01]) + b[i + 1:]
    return [key[:-1], key + b"x", flip(key, len(key) - 1), flip(key, 0)]


def exact_key_only(sh, klen, seed=5):
    """One keyed object whose key holds `klen` bytes. Rows that carry its digest but a key one
    byte off must miss; the exact key hits. Returns (near-miss hits, alive past the old
    expiry after them, exact hit, alive past the old expiry after it)."""
    rng = random.Random(seed * 1000 + klen)
    key = b"/" + bytes(rng.choice(b"abcdefghijklmnopqrstuvwxyz0123456789") for _ in range(klen - 1))
    obj = {key: keyed(key, b"payload " * (klen % 5))}
    store_at(sh, obj, T0 + TTL0)
    near = near_miss_keys(key)
    t = T0 + TTL0 + 1
    h1 = touch(sh, near, [T0 + 500] * len(near), digest_of=[key] * len(near))
    a1 = live_at(sh, obj, t)
    h2 = touch(sh, [key], [T0 + 500])
    a2 = live_at(sh, obj, t)
    return h1, a1, h2, a2, key


KLENS = [1, 13, 14, 15, 29, 30, 31, 45, 46, 47, 300]


def keyed_matches(value, key):
    """keyed.h keyed_match: whether the stored value is a keyed value of exactly `key`."""
    if len(value) < 2:
        return False
    kl = struct.unpack("<H", value[:2])[0]
    return kl == len(key) and len(value) >= 2 + kl and value[2:2 + kl] == key


def garbage_touch(sh):
    """Un-keyed values touched with key bytes: every stored digest against a handful of key
    strings. Returns ({(stored key, key bytes): hit}, the model's, live at T0 + TTL0 + 1)."""
    junk = pc.garbage_values()
    store_at(sh, junk, T0 + TTL0)
    probes = [b"", b"/", b"/abc", b"\xff", b"\xff" * 38, b"/abcdefghi", b"/abcdefghij",
              b"x" * 300, b"y" * 65535]
    got, want = {}, {}
    for p in probes:
        hit = touch(sh, [p] * len(junk), [T0 + 500] * len(junk), digest_of=list(junk))
        for k, h in zip(junk, hit):
            got[(k, p)] = h
            want[(k, p)] = int(keyed_matches(junk[k], p))
    return got, want, live_at(sh, junk, T0 + TTL0 + 1)


class EtagOrigin:
    """A small origin for the grace tests: every path serves `body <path> <etag>` with an
    ETag, answers a matching If-None-Match with 304 (no body), and logs what it was asked.
    Per path: `etags` (change it and the next conditional request gets a full 200), `modes`
    ("ok", "503", or "drop": the connection is closed without an answer, an origin that is
    down), `delays` (seconds before answering) and `cache_control`."""

    def __init__(self):
        self.etags, self.modes, self.delays, self.cache_control = {}, {}, {}, {}
        self.cc304 = {}        # Cache-Control of a path's 304s (`cache_control`: the others)
        self.log = []          # (path, If-None-Match or None, status sent; 0 = dropped)
        self.lock = threading.Lock()
        outer = self

        class Handler(BaseHTTPRequestHandler):
            protocol_version = "HTTP/1.1"

            def do_GET(self):
                path = self.path
                inm = self.headers.get("If-None-Match")
                delay = outer.delays.get(path, 0)
                if delay:
                    time.sleep(delay)
                mode = outer.modes.get(path, "ok")
                etag = outer.etags.get(path, '"v1"')
                if mode == "drop":
                    outer._note(path, inm, 0)
                    self.close_connection = True
                    return
                if mode == "503":
                    outer._note(path, inm, 503)
                    self._send(503, b"origin is sick", None, path)
                elif inm == etag:
                    outer._note(path, inm, 304)
                    self._send(304, b"", etag, path)
                else:
                    outer._note(path, inm, 200)
                    self._send(200, outer.body(path, etag), etag, path)

            def _send(self, status, body, etag, path):
                self.send_response(status)
                if etag:
                    self.send_header("ETag", etag)
                cc = outer.cc304 if status == 304 else outer.cache_control
                if path in cc:
                    self.send_header("Cache-Control", cc[path])
                if status != 304:
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
    def body(path, etag):
        return f"body {path} {etag}".encode()

    def _note(self, path, inm, status):
        with self.lock:
            self.log.append((path, inm, status))

    def seen(self, path):
        with self.lock:
            return [e for e in self.log if e[0] == path]

    def wait_seen(self, path, n, timeout=5.0):
        """The log entries of `path` once there are at least n of them."""
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


def wait_stat(px, name, value, timeout=5.0):
    """The proxy's counter `name` once it has reached `value`."""
    deadline = time.time() + timeout
    while px.stats()[name] < value and time.time() < deadline:
        time.sleep(0.005)
    return px.stats()[name]


GRACE_COUNTERS = ["stale_served", "revalidations", "revalidated_304", "revalidate_touched",
                  "revalidate_restored", "revalidate_errors"]


def revalidate_304_round_trip(px, origin, path="/a"):
    """`path` was fetched through `px` (ttl=1, grace on) more than a second ago. A GET is
    served the old body at once; the origin then sees exactly one conditional request and
    sends no body; the object is touched in place and the next GET is fresh."""
    from shellac_amd.utils.httpclient import HttpClient
    # the 304 renews it for a minute (taken from the 304's Cache-Control), so "fresh again"
    # below does not depend on where the second boundaries of a 1 s TTL fall
    origin.cc304[path] = "max-age=60"
    st0, n0 = px.stats(), len(origin.seen(path))
    c = HttpClient(port=px.port)
    r = c.get(path)
    assert r.status() == 200 and r.body().read() == origin.body(path, '"v1"')
    log = origin.wait_seen(path, n0 + 1)
    assert log[n0:] == [(path, '"v1"', 304)], log
    assert wait_stat(px, "revalidate_touched", st0["revalidate_touched"] + 1) == \
        st0["revalidate_touched"] + 1
    r = c.get(path)                                   # fresh again: no origin request
    assert r.status() == 200 and r.body().read() == origin.body(path, '"v1"')
    st1 = px.stats()
    assert {k: st1[k] - st0[k] for k in GRACE_COUNTERS} == {
        "stale_served": 1, "revalidations": 1, "revalidated_304": 1, "revalidate_touched": 1,
        "revalidate_restored": 0, "revalidate_errors": 0}
    assert origin.seen(path) == log
    assert [e[2] for e in log].count(200) == 1        # one full body ever: the first fetch
    c.close()
    return st0, st1


def ref_bit(sh, key):
    """The CLOCK reference bit and the expiry of `key`'s index entry."""
    lo, hi = (int(x) & M64 for x in digest_strings([key], "cpu")[0])
    from shellac_amd import core
    for b in core().bucket_pair(lo, hi, sh.nbuckets):
        e = sh._impl.debug_bucket(b)
        for k in range(4):
            if e[4 * k] == lo and e[4 * k + 1] == hi and e[4 * k + 2]:
                return bool(e[4 * k + 3] & REF_BIT), e[4 * k + 3] >> 32
    return None
