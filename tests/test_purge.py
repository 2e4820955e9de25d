"""Cache invalidation (CPU): CacheShard.remove_keyed_prefix on the host twin against a
Python dict model, CacheBackend.purge_prefix on the host tiers, and the proxy's PURGE
method over the DRAM backend. The GPU side is tests/test_purge_gpu.py."""
import json
import socket
import threading
import time

import pytest

import purge_cases as pc
from shellac_amd import core
from shellac_amd.ops.cache import digest_strings, item_bytes, keyed
from shellac_amd.server.proxy import Server, make_backend
from shellac_amd.utils.fakemc import FakeMemcached
from shellac_amd.utils.httpclient import HttpClient
from shellac_amd.utils.origin import Origin


# ------------------------------------------------------------------ shard engine (host twin)
def test_keyed_helper_matches_the_stored_layout():
    v = keyed(b"/a/b", b"payload")
    assert v == b"\x04\x00/a/bpayload"
    assert keyed(b"", b"") == b"\x00\x00"


@pytest.mark.parametrize("prefix", [b"/static/", b"/static/js/", b"/api/v1/users/", b"/",
                                    b"/nothing/here/"])
def test_prefix_purge_against_dict_model(prefix):
    sh = pc.make_shard()
    objs = pc.family_objects(2000)
    pc.store(sh, objs)
    live = pc.live_keys(sh, objs)
    assert len(live) > 1900  # (the shard holds them: the model is not vacuous)
    want_n, want_bytes, survivors = pc.model_purge(objs, live, prefix)
    assert sh.remove_keyed_prefix(prefix) == (want_n, want_bytes)
    assert pc.live_keys(sh, objs) == survivors
    assert sh.counters()["purged"] == want_n
    # idempotent: nothing left to remove, the counter stays
    assert sh.remove_keyed_prefix(prefix) == (0, 0)
    assert sh.counters()["purged"] == want_n


@pytest.mark.parametrize("plen", pc.BOUNDARY_PLENS)
def test_prefix_length_granule_boundaries(plen):
    sh = pc.make_shard()
    pat, objs, must_go = pc.boundary_objects(plen)
    assert len(pat) == plen
    bystanders = pc.family_objects(50, seed=plen)
    bystanders = {k: v for k, v in bystanders.items() if not k.startswith(pat)}
    pc.store(sh, {**objs, **bystanders})
    n, nbytes = sh.remove_keyed_prefix(pat)
    assert n == len(must_go)
    assert nbytes == sum(item_bytes(len(objs[k])) for k in must_go)
    got = dict(zip(objs, sh.get_many(list(objs))))
    for k in objs:
        assert (got[k] is None) == (k in must_go), (plen, k)
    assert pc.live_keys(sh, bystanders) == set(bystanders)


def test_key_equal_to_pattern_is_removed_and_shorter_key_is_not():
    sh = pc.make_shard()
    sh.set_many([b"/abc", b"/ab"], [keyed(b"/abc", b"x"), keyed(b"/ab", b"x")])
    assert sh.remove_keyed_prefix(b"/abc")[0] == 1
    assert sh.get_many([b"/abc", b"/ab"]) == [None, keyed(b"/ab", b"x")]


def test_difference_in_first_or_last_pattern_byte():
    sh = pc.make_shard()
    keys = [b"/abcdefghijklmnopqrstuvwxyz/1", b"!abcdefghijklmnopqrstuvwxyz/1",
            b"/abcdefghijklmnopqrstuvwxyZ/1"]
    sh.set_many(keys, [keyed(k, b"p") for k in keys])
    assert sh.remove_keyed_prefix(b"/abcdefghijklmnopqrstuvwxyz")[0] == 1
    assert [v is None for v in sh.get_many(keys)] == [True, False, False]


def test_compare_is_bounded_by_the_key_length():
    """Key `/a` with a payload that starts `bc`: the value reads `/abc...` from byte 2, but
    the key is only `/a`, so the pattern `/abc` does not match it."""
    sh = pc.make_shard()
    sh.set_many([b"/a"], [keyed(b"/a", b"bcdef")])
    assert sh.remove_keyed_prefix(b"/abc") == (0, 0)
    assert sh.get_many([b"/a"]) == [keyed(b"/a", b"bcdef")]
    assert sh.remove_keyed_prefix(b"/a")[0] == 1


def test_short_and_garbage_values_are_safe():
    sh = pc.make_shard()
    junk = pc.garbage_values()
    pc.store(sh, junk)
    for pat in (b"/", b"/abc", b"\xff", b"\xff" * 38, b"/abcdefghi", b"x" * 300):
        n, _ = sh.remove_keyed_prefix(pat)
        # only a value that parses as a keyed record with a matching key may go
        assert n == sum(1 for v in junk.values()
                        if len(v) >= 2 and 2 + int.from_bytes(v[:2], "little") <= len(v)
                        and int.from_bytes(v[:2], "little") >= len(pat)
                        and v[2:2 + len(pat)] == pat), pat
    # the klen fields that point past the value never matched anything
    assert sh.get_many([b"garbage/klen-huge", b"garbage/klen-past-end"]) == \
        [junk[b"garbage/klen-huge"], junk[b"garbage/klen-past-end"]]
    assert sh.get_many([b"garbage/empty", b"garbage/one"]) == [b"", b"/"]


def test_expired_and_deleted_entries_are_not_counted():
    sh = pc.make_shard()
    fresh = {b"/x/keep/%d" % i: keyed(b"/x/keep/%d" % i, b"v") for i in range(10)}
    dying = {b"/x/ttl/%d" % i: keyed(b"/x/ttl/%d" % i, b"v") for i in range(7)}
    deleted = {b"/x/del/%d" % i: keyed(b"/x/del/%d" % i, b"v") for i in range(5)}
    pc.store(sh, fresh)
    pc.store(sh, deleted)
    pc.store(sh, dying, ttl=5)
    assert sh.remove(digest_strings(list(deleted))).all()
    later = sh.now() + 100  # the TTL'd entries have expired by then
    assert sh.remove_keyed_prefix(b"/x/", now=later)[0] == len(fresh)
    assert sh.counters()["purged"] == len(fresh)


def test_empty_prefix_raises():
    sh = pc.make_shard()
    with pytest.raises(Exception):
        sh.remove_keyed_prefix(b"")
    with pytest.raises(Exception):
        sh._impl.remove_keyed_prefix(b"", 1)
    with pytest.raises(Exception):
        core().keyed_prefix_image(b"")


def test_purge_after_the_log_lapped():
    """More than 3x the log written: entries of overwritten records are dead (not counted),
    and the count is the model's over the keys that still hit."""
    sh = pc.make_shard()
    # (payloads up to 1500 B: the ~1300 objects a full log holds stay far below the 4096
    # index slots, so no index eviction, whose victims differ between the twins, interferes)
    objs = pc.family_objects(6000, seed=11, max_payload=1500)
    assert sum(item_bytes(len(v)) for v in objs.values()) > 3 * sh.log_bytes
    pc.store(sh, objs)
    live = pc.live_keys(sh, objs)
    assert 0 < len(live) < len(objs) // 2
    want_n, want_bytes, survivors = pc.model_purge(objs, live, b"/static/")
    assert want_n > 0
    assert sh.remove_keyed_prefix(b"/static/") == (want_n, want_bytes)
    assert pc.live_keys(sh, objs) == survivors


def test_clock_hand_does_not_resurrect_purged_objects():
    pc.clock_never_resurrects(pc.make_shard())


# ------------------------------------------------------------------------------ backends
def _fill_backend(be, fams=(b"/a/", b"/b/"), n=30):
    keys = {f: [f + b"%d" % i for i in range(n)] for f in fams}
    for f in fams:
        for k in keys[f]:
            be.set(k, b"value of " + k, 0, 0)
    return keys


def test_dram_backend_purge_prefix():
    be = make_backend("dram", dram_mb=16)
    keys = _fill_backend(be)
    assert be.purge_prefix(b"/a/") == 30
    assert be.get_many(keys[b"/a/"]) == [None] * 30
    assert all(v is not None for v in be.get_many(keys[b"/b/"]))
    assert be.purge_prefix(b"/a/") == 0
    assert be.purge_prefix(b"/b/1") == 11  # /b/1 and /b/10../b/19
    assert be.stats()["cache_objects"] == 19


def test_tiered_backend_purges_both_levels_and_drops_stale_promotions():
    c = core()
    l1, l2 = c.dram_backend(8 << 20, 1 << 20), c.dram_backend(8 << 20, 1 << 20)
    be = c.tiered_backend(l1, l2)
    keys = _fill_backend(be)                 # writes go to both levels
    l2.set(b"/a/only-l2", b"deep", 0, 0)
    assert be.get(b"/a/only-l2") == (b"deep", 0)   # an L2 hit, promoted into L1
    assert l1.get(b"/a/only-l2") is not None
    assert be.purge_prefix(b"/a/") == 2 * 30 + 2
    for tier in (be, l1, l2):
        assert tier.get_many(keys[b"/a/"] + [b"/a/only-l2"]) == [None] * 31
        assert all(v is not None for v in tier.get_many(keys[b"/b/"]))
    assert be.stats()["tier_purges"] == 1


def test_tiered_delete_removes_the_key_from_both_levels():
    c = core()
    l1, l2 = c.dram_backend(8 << 20, 1 << 20), c.dram_backend(8 << 20, 1 << 20)
    be = c.tiered_backend(l1, l2)
    be.set(b"/k/both", b"x", 0, 0)
    l2.set(b"/k/deep", b"y", 0, 0)
    assert be.get(b"/k/deep") == (b"y", 0) and l1.get(b"/k/deep") is not None   # promoted
    assert be.delete(b"/k/both") is True and be.delete(b"/k/deep") is True
    assert be.delete(b"/k/both") is False
    for tier in (be, l1, l2):
        assert tier.get_many([b"/k/both", b"/k/deep"]) == [None, None]


def test_every_tier_refuses_an_empty_prefix():
    c = core()
    dram = make_backend("dram", dram_mb=16)
    dram.set(b"/a/1", b"v", 0, 0)
    tiered = c.tiered_backend(c.dram_backend(8 << 20, 1 << 20), c.dram_backend(8 << 20, 1 << 20))
    for be in (dram, tiered, make_backend("dram", dram_mb=16, fault="")):
        assert be.purge_prefix(b"") == -1
    assert dram.get(b"/a/1") == (b"v", 0)    # and nothing was flushed


def test_tier_that_cannot_scan_answers_minus_one():
    f = FakeMemcached().start()
    try:
        be = make_backend("memcached", caches=[("127.0.0.1", f.port)])
        assert be.purge_prefix(b"/a/") == -1
        tiered = make_backend("memcached", caches=[("127.0.0.1", f.port)], l1_mb=8)
        assert tiered.purge_prefix(b"/a/") == -1
    finally:
        f.stop()


def test_fault_backend_forwards_purge():
    be = make_backend("dram", dram_mb=16, fault="")
    _fill_backend(be)
    assert be.purge_prefix(b"/b/") == 30


# --------------------------------------------------------------------------------- proxy
@pytest.fixture
def origin():
    o = Origin(body_bytes=200).start()
    yield o
    o.stop()


def make_proxy(origin_port, backend=None, **kw):
    if backend is None:
        kw.setdefault("backend_kind", "dram")
        kw.setdefault("dram_mb", 32)
    return Server([("127.0.0.1", origin_port)], port=0, backend=backend, **kw).start()


purge = pc.purge


def test_proxy_prefix_and_exact_purge(origin):
    with make_proxy(origin.port, purge="loopback") as px:
        pc.prefix_purge_round_trip(px, origin)


def test_proxy_exact_purge_removes_every_vary_variant(origin):
    with make_proxy(origin.port, purge="loopback") as px:
        c = HttpClient(port=px.port)
        for _ in range(2):
            for ua in ("alpha", "beta"):
                r = c.get("/vary/ua/1", headers={"User-Agent": ua})
                assert f"ua={ua}".encode() in r.body().read()
        assert origin.hits["/vary/ua/1"] == 2
        assert purge(c, "/vary/ua/1") == (200, {"mode": "exact", "found": True, "variants": 2})
        for ua in ("alpha", "beta"):
            c.get("/vary/ua/1", headers={"User-Agent": ua})
        assert origin.hits["/vary/ua/1"] == 4  # both variants went back to the origin


def test_proxy_pipelined_purge_keeps_response_order(origin):
    with make_proxy(origin.port, purge="any") as px:
        c = HttpClient(port=px.port)
        c.get("/p/1")
        c.send(HttpClient.request_bytes("/p/1") +
               HttpClient.request_bytes("/p/1", method="PURGE") +
               HttpClient.request_bytes("/p/1") +
               HttpClient.request_bytes("/p/", method="PURGE", headers={"X-Purge-Mode": "prefix"}) +
               HttpClient.request_bytes("/p/2"))
        rs = [c.read_response() for _ in range(5)]
        assert b"/p/1 #1 " in rs[0].body().read()
        assert json.loads(rs[1].body().read()) == {"mode": "exact", "found": True, "variants": 0}
        assert b"/p/1 #2 " in rs[2].body().read()
        # the second GET's fetch is usually still out when the prefix purge runs (nothing to
        # remove, and its fill is then not stored); either way /p/1 is gone afterwards
        r3 = json.loads(rs[3].body().read())
        assert r3["mode"] == "prefix" and r3["purged"] in (0, 1)
        assert b"/p/2 #1 " in rs[4].body().read()
        assert b"/p/1 #3 " in c.get("/p/1").body().read()


def test_proxy_purge_off_forwards_the_method_upstream(origin):
    with make_proxy(origin.port) as px:   # purge="off" is the default
        c = HttpClient(port=px.port)
        c.get("/off/1")
        r = c.get("/off/1", method="PURGE")
        assert r.status() == 501 and b"Unsupported method" in r.body().read()  # the origin's answer
        c2 = HttpClient(port=px.port)
        c2.get("/off/1")
        assert origin.hits["/off/1"] == 1     # still cached
        assert px.stats()["purge_requests"] == 0


def test_purge_admission_predicate():
    """Who may PURGE, as the reactor decides it from the peer address of the connection:
    `loopback` admits 127/8 only, `any` everybody, `off` nobody (the method is not handled)."""
    allowed = core().purge_allowed
    for ip in ("127.0.0.1", "127.0.0.2", "127.255.255.254"):
        assert allowed("loopback", ip) and allowed("any", ip) and not allowed("off", ip)
    for ip in ("10.0.0.5", "192.168.1.127", "126.255.255.255", "128.0.0.1", "1.0.0.127",
               "0.0.0.0", "255.255.255.255"):
        assert not allowed("loopback", ip), ip
        assert allowed("any", ip) and not allowed("off", ip)


def _non_loopback_address():
    try:
        infos = socket.getaddrinfo(socket.gethostname(), None, socket.AF_INET)
    except OSError:
        return None
    for info in infos:
        ip = info[4][0]
        if not ip.startswith("127."):
            return ip
    return None


def test_proxy_purge_loopback_only(origin):
    """purge="loopback": a client on 127/8 may purge; one that reaches the proxy through
    another local address (where the host has one) gets 403 and nothing is removed."""
    with make_proxy(origin.port, purge="loopback") as px:
        c = HttpClient(port=px.port)
        c.get("/lo/1")
        ip = _non_loopback_address()
        if ip is not None:
            try:
                ext = HttpClient(host=ip, port=px.port, timeout=3)
            except OSError:
                ext = None
            if ext is not None:
                r = ext.get("/lo/", method="PURGE", headers={"X-Purge-Mode": "prefix"})
                assert r.status() == 403
                c.get("/lo/1")
                assert origin.hits["/lo/1"] == 1
                assert px.stats()["purge_denied"] == 1
        assert purge(c, "/lo/", prefix=True) == (200, {"mode": "prefix", "purged": 1})
    with pytest.raises(ValueError):
        Server([("127.0.0.1", origin.port)], port=0, purge="everyone")


def test_proxy_prefix_purge_is_501_where_the_tier_cannot_scan(origin):
    f = FakeMemcached().start()
    try:
        with make_proxy(origin.port, backend_kind="memcached", caches=[("127.0.0.1", f.port)],
                        purge="loopback") as px:
            c = HttpClient(port=px.port)
            st, _ = purge(c, "/m/", prefix=True)
            assert st == 501
            st, body = purge(c, "/m/1")
            assert st == 200 and body == {"mode": "exact", "found": False, "variants": -1}
    finally:
        f.stop()


def test_fill_in_flight_is_not_cached_after_a_purge():
    """A miss fetched from the origin before a purge and completed after it is delivered
    but not stored: the next GET goes to the origin again."""
    o = Origin(body_bytes=100, delay_s=0.3).start()
    try:
        with make_proxy(o.port, purge="loopback", threads=2) as px:
            got = {}

            def first():
                got["r"] = HttpClient(port=px.port).get("/slow/x").body().read()

            th = threading.Thread(target=first)
            th.start()
            deadline = time.time() + 5
            while o.hits["/slow/x"] == 0 and time.time() < deadline:
                time.sleep(0.005)   # the fetch is out (the origin holds it for 0.3 s)
            assert o.hits["/slow/x"] == 1
            c = HttpClient(port=px.port)
            st, body = purge(c, "/slow/", prefix=True)
            assert st == 200 and body["purged"] == 0
            th.join()
            assert b"/slow/x #1 " in got["r"]
            assert b"/slow/x #2 " in c.get("/slow/x").body().read()
            assert o.hits["/slow/x"] == 2
            assert b"/slow/x #2 " in c.get("/slow/x").body().read()   # and that one is cached
            assert px.stats()["fills_not_cached_purged"] == 1
    finally:
        o.stop()


def test_metrics_carry_the_purge_counters(origin):
    with make_proxy(origin.port, purge="loopback") as px:
        c = HttpClient(port=px.port)
        c.get("/m/1")
        purge(c, "/m/", prefix=True)
        text = c.get("/_shellac/metrics").body().read().decode()
        assert "shellac_purge_requests 1" in text
        assert "shellac_purged_objects 1" in text


def test_cli_has_the_purge_flag():
    from shellac_amd.server.proxy import build_arg_parser

    p = build_arg_parser()
    assert p.parse_args(["-s", "x"]).purge == "off"
    assert p.parse_args(["-s", "x", "--purge", "loopback"]).purge == "loopback"
