"""Purge by surrogate key (CPU): the tag block helpers, CacheShard.remove_keyed_tags /
soften_keyed_tags on the host twin against a Python model, CacheBackend.purge_tags /
soften_tags on the host tiers, the proxy's --tag-header over the DRAM backend, and the host
code under sanitizers. The GPU side is tests/test_tag_purge_gpu.py."""
import os
import shutil
import struct
import subprocess
import threading
import time

import pytest

import purge_cases as pc
import soften_cases as sc
import tag_cases as tg
import touch_cases as tc
from shellac_amd import core
from shellac_amd.ops.cache import keyed, split_tagged, tag_hash, tagged
from shellac_amd.server.proxy import Server, build_arg_parser, make_backend
from shellac_amd.utils.fakemc import FakeMemcached
from shellac_amd.utils.httpclient import HttpClient

CPU = ["cpu"]
T0 = tg.T0


# ---------------------------------------------------------------------------- the tag block
def test_tag_hash_is_the_low_word_of_the_digest():
    assert tag_hash(b"product-4711") == core().digest(b"product-4711")[0]
    assert tag_hash(b"Product-4711") != tag_hash(b"product-4711")     # case-sensitive


def test_tagged_and_split_tagged_round_trip():
    body = b"HTTP/1.1 200 OK\r\n\r\nhello"
    v = tagged([b"x", b"y", b"x"], body)                              # duplicates collapse
    assert v == tg.block([tag_hash(b"x"), tag_hash(b"y")]) + body
    assert split_tagged(v) == ([tag_hash(b"x"), tag_hash(b"y")], body)
    assert tagged([], body) == b"\x02\x00" + body and split_tagged(tagged([], body)) == ([], body)
    many = [b"t%d" % i for i in range(32)]
    assert split_tagged(tagged(many, body)) == ([tag_hash(t) for t in many], body)
    assert tagged(many + [b"one-more"], body) == b"\x02\xff" + body   # overflow: no hashes
    assert split_tagged(b"\x02\xff" + body) == ("overflow", body)
    # untagged, malformed and truncated payloads are left as they are
    for raw in (body, b"\x01accept-encoding", b"", b"\x02", b"\x02\x21" + b"\x00" * 400,
                b"\x02\xfe" + b"\x00" * 4000, b"\x02\x02" + b"\x00" * 15):
        assert split_tagged(raw) == (None, raw)


# ------------------------------------------------------------------ shard engine (host twin)
def test_host_alignment_sweep():
    tg.run_alignment_sweep(CPU)


def test_host_block_forms():
    tg.run_block_forms(CPU)


def test_host_garbage_values():
    tg.run_garbage(CPU)


def test_host_near_misses_list_sizes_and_refused_lists():
    tg.run_near_misses(CPU)


def test_host_tagged_families_match_the_model():
    tg.run_families(CPU)


def test_host_purge_after_the_log_lapped():
    tg.run_after_the_log_lapped(CPU)


def test_host_expired_entries_are_not_counted():
    tg.run_expired_are_not_counted(CPU)


def test_host_dead_same_digest_entry_and_locked_slot_are_left_alone():
    tg.run_dead_entries(CPU)


def test_host_soft_form_over_expiries_and_caps():
    tg.run_soft_form(CPU)


def test_host_reference_bit_survives_a_tag_softening():
    tg.run_reference_bit(CPU)


def test_host_clock_hand_keeps_the_tags_and_resurrects_nothing():
    alive, n, left, reinserted = tg.clock_keeps_the_tags(pc.make_shard("cpu"))
    assert alive == n == 20 and left == 0 and reinserted >= 20
    assert tg.clock_never_resurrects(pc.make_shard("cpu"))["purged"] == 150
    meta, live_at_cap, reinserted = tg.clock_keeps_the_softening(pc.make_shard("cpu"))
    assert len(meta) == 20 and reinserted >= 20 and live_at_cap == set()
    assert set(meta.values()) == {(sc.STALE_AT, T0 + sc.TTL0)}


# -------------------------------------------------------------------------------- backends
def _ttl_near(got, want):
    return got is not None and want - 2 <= got[2] <= want


def _fill(be):
    fam = {"xy": [b"/p/xy/%d" % i for i in range(8)], "y": [b"/q/y/%d" % i for i in range(8)],
           "none": [b"/p/none/%d" % i for i in range(8)], "z": [b"/q/z/%d" % i for i in range(8)]}
    tags = {"xy": [b"x", b"y"], "y": [b"y"], "z": [b"z"]}
    vals = {}
    for f, keys in fam.items():
        for k in keys:
            vals[k] = tagged(tags[f], b"HTTP/" + k) if f in tags else b"HTTP/" + k
            be.set(k, vals[k], 3, 500)
    return fam, vals


@pytest.mark.parametrize("kind", ["dram", "fault"])
def test_dram_backend_purge_tags(kind):
    be = make_backend("dram", dram_mb=16, **({"fault": ""} if kind == "fault" else {}))
    fam, vals = _fill(be)
    assert be.purge_tags([b"y"]) == 16
    assert be.get_many(fam["xy"] + fam["y"]) == [None] * 16
    assert be.get_many(fam["none"] + fam["z"]) == [(vals[k], 3) for k in fam["none"] + fam["z"]]
    assert be.purge_tags([b"y"]) == 0
    assert be.purge_tags([b"nobody", b"z", b"z"]) == 8
    assert be.purge_tags([]) == -1 and be.purge_tags([b"t%d" % i for i in range(65)]) == -1
    assert be.soften_tags([], 5) == -1
    assert be.get_many(fam["none"]) == [(vals[k], 3) for k in fam["none"]]


def test_dram_backend_soften_tags_then_touch_makes_it_fresh_and_the_tags_remain():
    be = make_backend("dram", dram_mb=16)
    fam, vals = _fill(be)
    be.set(b"/never", tagged([b"y"], b"HTTP/never"), 3, 0)
    assert be.soften_tags([b"y"], 1234, keep_s=100) == 17
    assert be.soften_tags([b"y"], 1234, keep_s=100) == 17               # the same count again
    for k in fam["xy"] + fam["y"]:
        got = be.get_ttl(k)
        assert got[:2] == (vals[k], 1234) and _ttl_near(got, 100)
    assert _ttl_near(be.get_ttl(b"/never"), 100)
    for k in fam["none"] + fam["z"]:
        got = be.get_ttl(k)
        assert got[:2] == (vals[k], 3) and _ttl_near(got, 500)
    k = fam["xy"][0]
    assert be.touch(k, 400, flags=4321) == 1
    got = be.get_ttl(k)
    assert got[:2] == (vals[k], 4321) and _ttl_near(got, 400)       # fresh again, the block kept
    assert be.purge_tags([b"x"]) == 8                                    # and still found by tag


def test_memcached_tier_answers_minus_one():
    f = FakeMemcached().start()
    try:
        mc = make_backend("memcached", caches=[("127.0.0.1", f.port)])
        mc.set(b"/m/1", tagged([b"y"], b"v"), 3, 50)
        assert mc.purge_tags([b"y"]) == -1 and mc.soften_tags([b"y"], 8, keep_s=10) == -1
        tiered = make_backend("memcached", caches=[("127.0.0.1", f.port)], l1_mb=8)
        assert tiered.purge_tags([b"y"]) == -1 and tiered.soften_tags([b"y"], 8) == -1
    finally:
        f.stop()


def test_tiered_backend_purges_and_softens_both_levels():
    c = core()
    l1, l2 = c.dram_backend(8 << 20, 1 << 20), c.dram_backend(8 << 20, 1 << 20)
    be = c.tiered_backend(l1, l2)
    for i in range(10):
        be.set(b"/a/%d" % i, tagged([b"a"], b"a%d" % i), 3, 500)     # writes go to both levels
        be.set(b"/b/%d" % i, tagged([b"b"], b"b%d" % i), 3, 500)
    l2.set(b"/a/only-l2", tagged([b"a"], b"deep"), 3, 500)
    assert be.soften_tags([b"a"], 1234, keep_s=100) == 2 * 10 + 1
    for tier in (l1, l2):
        for i in range(10):
            got = tier.get_ttl(b"/a/%d" % i)
            assert got[:2] == (tagged([b"a"], b"a%d" % i), 1234) and _ttl_near(got, 100)
            assert tier.get_ttl(b"/b/%d" % i)[1] == 3
    assert be.get(b"/a/only-l2") == (tagged([b"a"], b"deep"), 1234)     # promoted stale
    assert be.purge_tags([b"a"]) == 2 * 11
    assert l1.get(b"/a/3") is None and l2.get(b"/a/3") is None and be.get(b"/a/only-l2") is None
    assert be.get(b"/b/3") == (tagged([b"b"], b"b3"), 3)
    assert be.stats()["tier_purges"] == 2


def test_promotion_that_straddles_a_tag_softening_is_dropped():
    """A GET finds nothing in L1 and is on its way through a slow L2 when the soft tag purge
    passes both levels: its promotion is dropped, so L1 gets no copy the purge did not see."""
    c = core()
    l1, inner = c.dram_backend(8 << 20, 1 << 20), c.dram_backend(8 << 20, 1 << 20)
    l2 = c.fault_backend(inner, "delay_us=150000", 1)
    be = c.tiered_backend(l1, l2)
    inner.set(b"/s/1", tagged([b"s"], b"deep"), 3, 500)
    got = {}
    th = threading.Thread(target=lambda: got.update(r=be.get(b"/s/1")))
    th.start()
    time.sleep(0.03)                                   # the GET is inside L2's delay
    assert be.soften_tags([b"s"], 1234, keep_s=100) == 1
    th.join()
    assert got["r"] is not None and got["r"][0] == tagged([b"s"], b"deep")
    assert l1.get(b"/s/1") is None
    assert be.stats()["tier_promote_dropped_purge"] == 1
    assert inner.get(b"/s/1") == (tagged([b"s"], b"deep"), 1234)


# --------------------------------------------------------------------------------- proxy
def _proxy(origin_port, backend=None, **kw):
    kw.setdefault("purge", "loopback")
    kw.setdefault("tag_header", tg.TAG_HEADER)
    if backend is None:
        backend = make_backend("dram", dram_mb=16)
    return Server([("127.0.0.1", origin_port)], port=0, backend=backend, **kw).start()


@pytest.fixture
def origin():
    o = tg.TagOrigin().start()
    yield o
    o.stop()


def test_proxy_purge_by_tag(origin):
    with _proxy(origin.port) as px:
        tg.purge_by_tag_round_trip(px, origin)
        text = HttpClient(port=px.port).get("/_shellac/metrics").body().read().decode()
        for line in ("shellac_tag_purge_requests 2", "shellac_tag_purged_objects 4",
                     "shellac_tag_softened_objects 0", "shellac_tagged_fills 6"):
            assert line in text, line


def test_clients_never_see_a_block_and_the_tier_holds_one(origin):
    be = make_backend("dram", dram_mb=16)
    origin.tags.update({"/c/plain": "x, y", "/c/gz": "x", "/c/vary": "x\ty", "/c/close": "y"})
    origin.gzip.add("/c/gz")
    origin.vary["/c/vary"] = "X-Lang"
    with _proxy(origin.port, backend=be) as px:
        c = HttpClient(port=px.port)
        cases = [("/c/plain", None), ("/c/gz", None), ("/c/gz", {"Accept-Encoding": "gzip"}),
                 ("/c/vary", {"X-Lang": "de"}), ("/c/vary", {"X-Lang": "fr"})]
        miss = [tg.fetch(c, p, h) for p, h in cases]
        hit = [tg.fetch(c, p, h) for p, h in cases]
        assert hit == miss
        for (p, _), (status, hdrs, body) in zip(cases, hit):
            assert status == 200 and body == origin.body(p)
            assert hdrs["surrogate-key"] == origin.tags[p]          # passed on as it is
        assert [len(origin.seen(p)) for p in ("/c/plain", "/c/gz", "/c/vary")] == [1, 1, 2]
        # the last response of a connection (Connection: close) is cut from the plain object too
        first = tg.fetch(c, "/c/close")
        c2 = HttpClient(port=px.port)
        last = tg.fetch(c2, "/c/close", {"Connection": "close"})
        assert last[2] == first[2] == origin.body("/c/close") and last[0] == 200
        assert last[1]["connection"] == "close" and len(origin.seen("/c/close")) == 1
        assert {k: v for k, v in last[1].items() if k not in ("connection", "keep-alive")} == \
            {k: v for k, v in first[1].items() if k not in ("connection", "keep-alive")}
        # what the tier holds does start with the block; the Vary marker has none
        x, y = tag_hash(b"x"), tag_hash(b"y")
        stored = be.get(b"localhost/c/plain")[0]
        assert stored.startswith(tg.block([x, y]) + b"HTTP/1.1 200")
        assert split_tagged(stored)[0] == [x, y]
        assert be.get(b"localhost/c/gz")[0].startswith(tg.block([x]) + b"HTTP/1.1 200")
        assert be.get(b"localhost/c/vary")[0].startswith(b"\x01")
        assert px.stats()["tagged_fills"] == 5
        # a Vary'd variant goes by its tags like any object
        assert tg.tag_purge(c, "x")[1]["purged"] == 4
        c.close()


def test_soft_tag_purge_with_grace(origin):
    path = "/s/a"
    origin.tags[path] = "x y"
    origin.cc304[path] = "max-age=60"
    be = make_backend("dram", dram_mb=16)
    with _proxy(origin.port, backend=be, ttl=60, grace=30) as px:
        c = HttpClient(port=px.port)
        assert c.get(path).body().read() == origin.body(path)
        assert c.get(path).body().read() == origin.body(path)            # fresh: a plain hit
        assert origin.seen(path) == [(path, None, 200)]
        assert tg.tag_purge(c, "y", soft=True) == (
            200, {"mode": "tag", "soft": True, "tags": 1, "softened": 1})
        assert c.get(path).body().read() == origin.body(path)            # stale, at once
        log = origin.wait_seen(path, 2)
        assert log[1:] == [(path, '"v1"', 304)], log
        assert tc.wait_stat(px, "revalidate_touched", 1) == 1
        assert c.get(path).body().read() == origin.body(path)            # fresh again
        st = px.stats()
        assert {k: st[k] for k in tc.GRACE_COUNTERS} == {
            "stale_served": 1, "revalidations": 1, "revalidated_304": 1, "revalidate_touched": 1,
            "revalidate_restored": 0, "revalidate_errors": 0}
        assert origin.seen(path) == log
        assert st["tag_softened_objects"] == 1 and st["tag_purge_requests"] == 1
        assert split_tagged(be.get(b"localhost" + path.encode())[0])[0] == \
            [tag_hash(b"x"), tag_hash(b"y")]
        # a second tag purge still matches it
        assert tg.tag_purge(c, "x") == (200, {"mode": "tag", "tags": 1, "purged": 1})
        c.close()


def test_soft_tag_purge_without_grace_is_a_hard_one(origin):
    origin.tags["/ng/1"] = "y"
    with _proxy(origin.port) as px:
        c = HttpClient(port=px.port)
        c.get("/ng/1")
        assert tg.tag_purge(c, "y", soft=True) == (
            200, {"mode": "tag", "soft": False, "tags": 1, "purged": 1})
        c.get("/ng/1")
        assert len(origin.seen("/ng/1")) == 2
        c.close()


def test_revalidation_that_restores_the_object_stores_it_with_its_block(origin):
    """The object vanishes between the stale hit and the 304: the touch finds nothing and the
    stale object is stored again — with its tag block, so a tag purge still finds it."""
    path = "/rs/a"
    origin.tags[path] = "y"
    origin.cc304[path] = "max-age=60"
    be = make_backend("dram", dram_mb=16)
    with _proxy(origin.port, backend=be, ttl=60, grace=30) as px:
        c = HttpClient(port=px.port)
        c.get(path).body().read()
        assert tg.tag_purge(c, "y", soft=True)[1]["softened"] == 1
        origin.delays[path] = 0.3
        assert c.get(path).body().read() == origin.body(path)            # stale; the 304 is slow
        assert len(origin.wait_seen(path, 2)) == 2                       # (it has arrived)
        assert be.delete(b"localhost" + path.encode())
        assert tc.wait_stat(px, "revalidate_restored", 1) == 1
        stored = be.get(b"localhost" + path.encode())[0]
        assert split_tagged(stored)[0] == [tag_hash(b"y")]
        assert c.get(path).body().read() == origin.body(path)
        assert tg.tag_purge(c, "y")[1]["purged"] == 1
        c.close()


def test_fill_fetched_before_a_tag_purge_is_delivered_but_not_stored(origin):
    origin.tags.update({"/slow/a": "x y", "/slow/many": " ".join("m%d" % i for i in range(40)),
                        "/slow/other": "z"})
    for p in ("/slow/a", "/slow/many", "/slow/other"):
        origin.delays[p] = 0.4
    be = make_backend("dram", dram_mb=16)
    with _proxy(origin.port, backend=be, threads=2) as px:
        got = {}

        def get(p):
            got[p] = HttpClient(port=px.port).get(p).body().read()
        ths = [threading.Thread(target=get, args=(p,)) for p in origin.delays]
        for th in ths:
            th.start()
        for p in origin.delays:
            origin_deadline = time.time() + 3
            while not origin.seen(p) and time.time() < origin_deadline:
                time.sleep(0.005)
        c = HttpClient(port=px.port)
        assert tg.tag_purge(c, "y") == (200, {"mode": "tag", "tags": 1, "purged": 0})
        for th in ths:
            th.join()
        assert got == {p: origin.body(p) for p in origin.delays}        # delivered
        st = px.stats()
        assert st["fills_not_cached_purged"] == 2                       # /slow/a and the overflow
        assert be.get(b"localhost/slow/a") is None and be.get(b"localhost/slow/many") is None
        assert be.get(b"localhost/slow/other") is not None
        c.close()


def test_refusals(origin):
    origin.tags["/r/1"] = "y"
    be = make_backend("dram", dram_mb=16)
    with _proxy(origin.port, backend=be, tag_header="") as px:       # no --tag-header
        c = HttpClient(port=px.port)
        c.get("/r/1")
        st, body = tg.tag_purge(c, "y")
        assert st == 400 and b"error" in body
        assert be.get(b"localhost/r/1")[0].startswith(b"HTTP/1.1 200")   # stored without a block
        assert px.stats()["tagged_fills"] == 0
        c.close()
    with _proxy(origin.port) as px:
        c = HttpClient(port=px.port)
        assert tg.tag_purge(c, None)[0] == 400                        # no tags
        assert tg.tag_purge(c, " , \t")[0] == 400
        assert tg.tag_purge(c, " ".join("t%d" % i for i in range(65)))[0] == 400
        assert tg.tag_purge(c, " ".join("t%d" % i for i in range(64)))[0] == 200
        assert tg.tag_purge(c, " ".join(["t1"] * 70))[1] == {"mode": "tag", "tags": 1, "purged": 0}
        ip = _non_loopback_address()
        if ip is not None:
            try:
                ext = HttpClient(host=ip, port=px.port, timeout=3)
            except OSError:
                ext = None
            if ext is not None:
                assert tg.tag_purge(ext, "y")[0] == 403
                assert px.stats()["purge_denied"] == 1
        c.close()
    f = FakeMemcached().start()
    try:
        mc = make_backend("memcached", caches=[("127.0.0.1", f.port)])
        with _proxy(origin.port, backend=mc, grace=30) as px:
            c = HttpClient(port=px.port)
            assert tg.tag_purge(c, "y")[0] == 501
            assert tg.tag_purge(c, "y", soft=True)[0] == 501         # as the prefix form
            c.close()
    finally:
        f.stop()


def _non_loopback_address():
    import socket
    try:
        infos = socket.getaddrinfo(socket.gethostname(), None, socket.AF_INET)
    except OSError:
        return None
    for info in infos:
        if not info[4][0].startswith("127."):
            return info[4][0]
    return None


def test_a_stored_block_is_stripped_when_the_option_is_off(origin):
    """A restart without --tag-header over a tier that still holds tagged objects."""
    be = make_backend("dram", dram_mb=16)
    obj = b"HTTP/1.1 200 OK\r\nContent-Length: 5\r\nConnection: keep-alive\r\n\r\nhello"
    be.set(b"localhost/old/1", tagged([b"x"], obj), 0, 500)
    be.set(b"localhost/old/2", b"\x02\xff" + obj, 0, 500)
    with _proxy(origin.port, backend=be, tag_header="") as px:
        c = HttpClient(port=px.port)
        for p in ("/old/1", "/old/2"):
            r = c.get(p)
            assert r.status() == 200 and r.body().read() == b"hello"
        assert origin.log == []
        c.close()


def test_cli_accepts_tag_header():
    assert build_arg_parser().parse_args(["--tag-header", "xkey"]).tag_header == "xkey"
    assert build_arg_parser().parse_args([]).tag_header == ""


# ------------------------------------------------------------------- host code, sanitized
def test_tag_block_helpers_and_host_scan_under_sanitizers(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++ on this machine")
    root = os.path.join(os.path.dirname(__file__), "..")
    csrc = os.path.join(root, "shellac_amd", "csrc")
    exe = str(tmp_path / "tag_block_main")
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", "-I", csrc,
           os.path.join(os.path.dirname(__file__), "native", "tag_block_main.cc"),
           os.path.join(csrc, "host_cache.cc"), "-o", exe, "-lpthread"]
    b = subprocess.run(cmd, capture_output=True, text=True)
    if b.returncode != 0 and ("asan" in b.stderr.lower() or "ubsan" in b.stderr.lower()) and \
            "cannot find" in b.stderr:
        pytest.skip("the toolchain lacks the sanitizer runtime: " + b.stderr.strip()[-200:])
    assert b.returncode == 0, b.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    assert "tag_block_main: ok" in r.stdout
