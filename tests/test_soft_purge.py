"""Soft purge (CPU): CacheShard.soften_keyed_prefix on the host twin against a Python model,
CacheBackend.soften_prefix on the host tiers, and the proxy's PURGE with X-Purge-Soft over
the DRAM backend with --grace. The GPU side is tests/test_soft_purge_gpu.py."""
import threading
import time

import pytest

import purge_cases as pc
import soften_cases as sc
import touch_cases as tc
from shellac_amd import core
from shellac_amd.ops.cache import digest_strings, keyed
from shellac_amd.server.proxy import Server, make_backend
from shellac_amd.utils.fakemc import FakeMemcached
from shellac_amd.utils.httpclient import HttpClient
from shellac_amd.utils.origin import Origin

T0 = sc.T0


# ------------------------------------------------------------------ shard engine (host twin)
@pytest.fixture(scope="module")
def objects():
    return pc.family_objects(1000)


def _an_existing_key(objs):
    return sorted(k for k in objs if k.startswith(b"/static/"))[0]


@pytest.mark.parametrize("cap", sc.CAPS)
@pytest.mark.parametrize("pattern,exact", [
    (b"/static/", False), (b"/static/js/", False), (b"/api/v1/users/", False), (b"/", False),
    (b"/nothing/here/", False), (b"/static/", True), (None, True), (b"/nothing/here/", True)])
def test_host_soften_matches_the_model(objects, pattern, exact, cap):
    sh = pc.make_shard()
    sc.store_mixed(sh, objects)
    model = sc.model_of(sh, objects)
    assert len(model) > 950          # (the shard holds them: the model is not vacuous)
    assert {e for e, _ in model.values()} == set(sc.EXPIRIES)
    if pattern is None:
        pattern = _an_existing_key(objects)      # exact mode: one URL
    n, _ = sc.check_soften([sh], objects, model, pattern, exact, cap)
    assert n == sum(sc.matches(k, pattern, exact) for k in model)
    if exact:
        assert n == (0 if pattern.endswith(b"/") else 1)
    elif pattern != b"/nothing/here/":
        assert n > 0


def test_successive_soft_purges_only_ever_shorten_a_life(objects):
    """A cap, then a later cap, then none: the second and third leave every expiry where the
    first put it; the flags follow the last one."""
    sh = pc.make_shard()
    sc.store_mixed(sh, objects)
    model = sc.model_of(sh, objects)
    _, model = sc.check_soften([sh], objects, model, b"/static/", False, T0 + 80, stale_at=11)
    _, model = sc.check_soften([sh], objects, model, b"/static/", False, T0 + 300, stale_at=12)
    _, model = sc.check_soften([sh], objects, model, b"/", False, 0, stale_at=13)
    static = [k for k in model if k.startswith(b"/static/")]
    assert static and all(0 < model[k][0] <= T0 + 80 for k in static)
    assert all(f == 13 for _, f in model.values())
    # past the cap the objects are gone: a soft purge at that time counts only what is live
    late = T0 + 80
    want = sum(1 for k, (e, _) in model.items() if k.startswith(b"/static/") and (e == 0 or e > late))
    assert want == 0
    assert sh.soften_keyed_prefix(b"/static/", 14, 0, now=late) == 0


@pytest.mark.parametrize("exact", [False, True])
@pytest.mark.parametrize("plen", pc.BOUNDARY_PLENS)
def test_host_pattern_length_granule_boundaries(plen, exact):
    pat, objs, must_prefix = sc.exact_boundary_objects(plen)
    sh = pc.make_shard()
    tc.store_at(sh, objs, T0 + sc.TTL0, flags=1)
    model = sc.model_of(sh, objs)
    assert set(model) == set(objs)
    n, model2 = sc.check_soften([sh], objs, model, pat, exact, T0 + 50)
    softened = {k for k in objs if model2[k][1] == sc.STALE_AT}
    assert softened == ({pat} if exact else {k for k in objs if k.startswith(pat)})
    assert must_prefix <= {k for k in objs if k.startswith(pat)} and n == len(softened)


def test_garbage_values_are_only_softened_as_keyed_matches():
    sh = pc.make_shard()
    junk = pc.garbage_values()
    tc.store_at(sh, junk, T0 + sc.TTL0, flags=1)
    for pat in (b"/", b"/abc", b"\xff", b"\xff" * 38, b"/abcdefghi", b"x" * 300):
        for exact in (False, True):
            def parses(v):
                kl = int.from_bytes(v[:2], "little")
                return (len(v) >= 2 and 2 + kl <= len(v) and v[2:2 + len(pat)] == pat and
                        (kl == len(pat) if exact else kl >= len(pat)))
            want = {k for k, v in junk.items() if parses(v)}
            assert sh.soften_keyed_prefix(pat, 77, 0, exact=exact, now=T0) == len(want), pat
            meta = sc.model_of(sh, junk)
            assert {k for k, (_, f) in meta.items() if f == 77} >= want
    # none of them parses as a matching keyed record: every one reads back unchanged
    assert sc.model_of(sh, junk) == {k: (T0 + sc.TTL0, 1) for k in junk}
    assert tc.live_at(sh, junk, T0) == set(junk)


def test_dead_entries_are_neither_counted_nor_written():
    sh = pc.make_shard()
    fam = {name: {b"/x/%s/%d" % (name, i): keyed(b"/x/%s/%d" % (name, i), b"v") for i in range(6)}
           for name in (b"keep", b"ttl", b"del", b"purged")}
    tc.store_at(sh, fam[b"ttl"], T0 + 5, flags=1)
    for name in (b"keep", b"del", b"purged"):
        tc.store_at(sh, fam[name], 0, flags=1)
    assert sh.remove(digest_strings(list(fam[b"del"])), now=T0).all()
    assert sh.remove_keyed_prefix(b"/x/purged/", now=T0)[0] == 6
    assert sh.soften_keyed_prefix(b"/x/", 9, T0 + 500, now=T0 + 5) == 6
    allobjs = {k: v for f in fam.values() for k, v in f.items()}
    assert sc.model_of(sh, allobjs, T0 + 5) == {k: (T0 + 500, 9) for k in fam[b"keep"]}
    # the expired ones were not written: seen from before their expiry they are unchanged
    assert {k: v for k, v in sc.model_of(sh, allobjs, T0).items() if k in fam[b"ttl"]} == \
        {k: (T0 + 5, 1) for k in fam[b"ttl"]}


def test_reference_bit_survives_a_softening_and_a_get_still_hits():
    sh = pc.make_shard()
    key = b"/ref/object"
    tc.store_at(sh, {key: keyed(key, b"r" * 50)}, T0 + 500, flags=1)
    assert tc.ref_bit(sh, key) == (False, T0 + 500)
    assert tc.live_at(sh, {key: keyed(key, b"r" * 50)}, T0) == {key}      # a GET sets the bit
    assert tc.ref_bit(sh, key) == (True, T0 + 500)
    assert sh.soften_keyed_prefix(b"/ref/", 5, T0 + 100, now=T0) == 1
    assert tc.ref_bit(sh, key) == (True, T0 + 100)
    assert tc.records_at(sh, [key], T0 + 99) == {key: (keyed(key, b"r" * 50), 5, T0 + 100)}
    assert tc.records_at(sh, [key], T0 + 100) == {}


def test_clock_hand_reappends_a_softened_object_with_its_flags_and_cap():
    meta, live_at_cap, reinserted = sc.clock_keeps_the_softening(pc.make_shard())
    assert len(meta) == 20 and reinserted >= 20
    assert set(meta.values()) == {(sc.STALE_AT, T0 + sc.TTL0)}
    assert live_at_cap == set()


def test_soften_refuses_malformed_arguments():
    sh = pc.make_shard()
    with pytest.raises(Exception):
        sh.soften_keyed_prefix(b"", 1)
    with pytest.raises(Exception):
        sh._impl.soften_keyed_prefix(b"", False, 1, 0, T0)
    with pytest.raises(Exception):
        sh.soften_keyed_prefix(b"/a", 1, expire_cap=T0, now=T0)      # the cap is not after now
    with pytest.raises(Exception):
        sh._impl.soften_keyed_prefix(b"/a", False, 1, T0 - 1, T0)


# ------------------------------------------------------------------------------ backends
def _ttl_near(got, want):
    return got is not None and want - 2 <= got[2] <= want


def test_dram_backend_soften_prefix():
    be = make_backend("dram", dram_mb=16)
    be.set(b"/a/never", b"v1", 3, 0)
    be.set(b"/a/long", b"v2", 3, 500)
    be.set(b"/a/short", b"v3", 3, 20)
    be.set(b"/a", b"v4", 3, 500)
    be.set(b"/b/1", b"v5", 3, 500)
    assert be.soften_prefix(b"/a/", 1234, keep_s=100) == 3
    assert be.soften_prefix(b"/a/", 1234, keep_s=100) == 3          # the same count again
    assert _ttl_near(be.get_ttl(b"/a/never"), 100) and be.get_ttl(b"/a/never")[:2] == (b"v1", 1234)
    assert _ttl_near(be.get_ttl(b"/a/long"), 100) and be.get_ttl(b"/a/long")[:2] == (b"v2", 1234)
    assert _ttl_near(be.get_ttl(b"/a/short"), 20) and be.get_ttl(b"/a/short")[:2] == (b"v3", 1234)
    assert _ttl_near(be.get_ttl(b"/a"), 500) and be.get_ttl(b"/a")[:2] == (b"v4", 3)
    assert _ttl_near(be.get_ttl(b"/b/1"), 500) and be.get_ttl(b"/b/1")[:2] == (b"v5", 3)
    # exact mode: the key itself, not what it is a prefix of; keep_s 0 leaves the expiry alone
    assert be.soften_prefix(b"/a", 99, exact=True) == 1
    assert _ttl_near(be.get_ttl(b"/a"), 500) and be.get_ttl(b"/a")[:2] == (b"v4", 99)
    assert be.get_ttl(b"/a/long")[1] == 1234
    assert be.soften_prefix(b"/a/lon", 5, exact=True) == 0
    # never extended
    assert be.soften_prefix(b"/a/", 1235, keep_s=400) == 3
    assert _ttl_near(be.get_ttl(b"/a/long"), 100)
    assert be.stats()["cache_objects"] == 5


def test_forged_digest_collision_is_not_softened():
    """An object keyed /attacker/x stored under /victim/x's digest: a soft purge of the
    victim's URL or prefix goes by the stored key and leaves it alone."""
    be = make_backend("dram", dram_mb=16)
    be.set(b"/attacker/x", b"payload", 7, 500, digest_of=b"/victim/x")
    assert be.get_with_digest(b"/attacker/x", b"/victim/x") == (b"payload", 7)
    assert be.soften_prefix(b"/victim/x", 1234, keep_s=10, exact=True) == 0
    assert be.soften_prefix(b"/victim/", 1234, keep_s=10) == 0
    assert be.get_with_digest(b"/attacker/x", b"/victim/x") == (b"payload", 7)
    assert be.get(b"/victim/x") is None


def test_every_tier_refuses_an_empty_pattern():
    c = core()
    dram = make_backend("dram", dram_mb=16)
    dram.set(b"/a/1", b"v", 3, 0)
    tiered = c.tiered_backend(c.dram_backend(8 << 20, 1 << 20), c.dram_backend(8 << 20, 1 << 20))
    for be in (dram, tiered, make_backend("dram", dram_mb=16, fault="")):
        assert be.soften_prefix(b"", 5) == -1
        assert be.soften_prefix(b"", 5, exact=True) == -1
    assert dram.get(b"/a/1") == (b"v", 3)


def test_fault_backend_forwards_and_memcached_cannot():
    be = make_backend("dram", dram_mb=16, fault="")
    be.set(b"/f/1", b"v", 3, 0)
    assert be.soften_prefix(b"/f/", 8) == 1 and be.get(b"/f/1") == (b"v", 8)
    f = FakeMemcached().start()
    try:
        mc = make_backend("memcached", caches=[("127.0.0.1", f.port)])
        mc.set(b"/m/1", b"v", 3, 50)
        assert mc.soften_prefix(b"/m/", 8, keep_s=10) == -1
        tiered = make_backend("memcached", caches=[("127.0.0.1", f.port)], l1_mb=8)
        assert tiered.soften_prefix(b"/m/", 8, keep_s=10) == -1
    finally:
        f.stop()


def test_tiered_backend_softens_both_levels():
    c = core()
    l1, l2 = c.dram_backend(8 << 20, 1 << 20), c.dram_backend(8 << 20, 1 << 20)
    be = c.tiered_backend(l1, l2)
    for i in range(10):
        be.set(b"/a/%d" % i, b"a%d" % i, 3, 500)          # writes go to both levels
        be.set(b"/b/%d" % i, b"b%d" % i, 3, 500)
    l2.set(b"/a/only-l2", b"deep", 3, 500)
    assert be.soften_prefix(b"/a/", 1234, keep_s=100) == 2 * 10 + 1
    for tier in (l1, l2):
        for i in range(10):
            got = tier.get_ttl(b"/a/%d" % i)
            assert got[:2] == (b"a%d" % i, 1234) and _ttl_near(got, 100)
            got = tier.get_ttl(b"/b/%d" % i)
            assert got[:2] == (b"b%d" % i, 3) and _ttl_near(got, 500)
    # an L2 hit after the soft purge promotes the stale copy, not a fresh one
    assert be.get(b"/a/only-l2") == (b"deep", 1234)
    assert l1.get(b"/a/only-l2") == (b"deep", 1234)
    assert be.stats()["tier_purges"] == 1


def test_promotion_that_straddles_a_soft_purge_is_dropped():
    """A GET finds nothing in L1 and is on its way through a slow L2 when the soft purge
    passes both levels: its promotion is dropped, so L1 gets no copy the purge did not see."""
    c = core()
    l1, inner = c.dram_backend(8 << 20, 1 << 20), c.dram_backend(8 << 20, 1 << 20)
    l2 = c.fault_backend(inner, "delay_us=150000", 1)
    be = c.tiered_backend(l1, l2)
    inner.set(b"/s/1", b"deep", 3, 500)
    got = {}
    th = threading.Thread(target=lambda: got.update(r=be.get(b"/s/1")))
    th.start()
    time.sleep(0.03)                                   # the GET is inside L2's delay
    assert be.soften_prefix(b"/s/", 1234, keep_s=100) == 1
    th.join()
    assert got["r"] is not None and got["r"][0] == b"deep"
    assert l1.get(b"/s/1") is None
    assert be.stats()["tier_promote_dropped_purge"] == 1
    assert inner.get(b"/s/1") == (b"deep", 1234)


# --------------------------------------------------------------------------------- proxy
def _proxy(origin_port, backend=None, **kw):
    kw.setdefault("purge", "loopback")
    if backend is None:
        backend = make_backend("dram", dram_mb=16)
    return Server([("127.0.0.1", origin_port)], port=0, backend=backend, **kw).start()


@pytest.fixture
def etag_origin():
    o = tc.EtagOrigin().start()
    yield o
    o.stop()


@pytest.fixture
def origin():
    o = Origin(body_bytes=100).start()
    yield o
    o.stop()


def test_soft_prefix_purge_serves_stale_once_and_a_304_makes_it_fresh(etag_origin):
    with _proxy(etag_origin.port, ttl=60, grace=30) as px:
        body = sc.soft_purge_304_round_trip(px, etag_origin, "/sp/a")
        assert body == {"mode": "prefix", "soft": True, "softened": 1}
        text = HttpClient(port=px.port).get("/_shellac/metrics").body().read().decode()
        assert "shellac_soft_purge_requests 1" in text
        assert "shellac_softened_objects 1" in text


def test_changed_object_is_served_stale_once_then_replaced(etag_origin):
    o = etag_origin
    with _proxy(o.port, ttl=60, grace=30) as px:
        c = HttpClient(port=px.port)
        assert c.get("/ch/b").body().read() == o.body("/ch/b", '"v1"')
        o.etags["/ch/b"] = '"v2"'
        assert sc.soft_purge(c, "/ch/", prefix=True) == \
            (200, {"mode": "prefix", "soft": True, "softened": 1})
        assert c.get("/ch/b").body().read() == o.body("/ch/b", '"v1"')      # stale, at once
        assert o.wait_seen("/ch/b", 2)[1] == ("/ch/b", '"v1"', 200)         # conditional, a full answer
        # (the tier is polled, not the proxy: a connection is good for 1000 requests)
        deadline = time.time() + 5
        while o.body("/ch/b", '"v2"') not in px.backend.get(b"localhost/ch/b")[0] and \
                time.time() < deadline:
            time.sleep(0.005)
        assert c.get("/ch/b").body().read() == o.body("/ch/b", '"v2"')
        assert len(o.seen("/ch/b")) == 2                                    # and it is fresh
        assert px.stats()["stale_served"] >= 1


def test_origin_down_serves_the_object_until_the_capped_expiry_and_not_after(etag_origin):
    """ttl=600, grace=2: the soft purge caps the object's life at now + 2 s. With the origin
    down it is served (stale) inside that window and is a miss after it."""
    o = etag_origin
    with _proxy(o.port, ttl=600, grace=2) as px:
        c = HttpClient(port=px.port)
        assert c.get("/dn/c").body().read() == o.body("/dn/c", '"v1"')
        left = px.backend.get_ttl(b"localhost/dn/c")[2]
        assert 590 <= left <= 602
        o.modes["/dn/c"] = "drop"
        t_purge = time.time()
        assert sc.soft_purge(c, "/dn/", prefix=True)[1]["softened"] == 1
        assert 0 <= px.backend.get_ttl(b"localhost/dn/c")[2] <= 2          # shortened to the grace
        # (whole-second clocks: a cap of now + 2 leaves more than a second of life)
        r = c.get("/dn/c")
        assert r.status() == 200 and r.body().read() == o.body("/dn/c", '"v1"')
        assert tc.wait_stat(px, "revalidate_errors", 1) == 1
        assert px.stats()["stale_served"] == 1
        time.sleep(max(0.0, t_purge + 3.1 - time.time()))
        assert c.get("/dn/c").status() == 502                               # gone, and no origin
        assert px.backend.get(b"localhost/dn/c") is None


def test_exact_mode_softens_the_url_and_its_vary_variants_but_no_sibling(origin):
    with _proxy(origin.port, ttl=60, grace=30) as px:
        c = HttpClient(port=px.port)
        for _ in range(2):
            for ua in ("alpha", "beta"):
                r = c.get("/vary/ua/1", headers={"User-Agent": ua})
                assert f"ua={ua}".encode() in r.body().read()
            assert c.get("/vary/ua/10").status() == 200
        assert origin.hits["/vary/ua/1"] == 2 and origin.hits["/vary/ua/10"] == 1
        # the marker at the URL's key and the two variants under it
        assert sc.soft_purge(c, "/vary/ua/1") == \
            (200, {"mode": "exact", "soft": True, "softened": 1, "variants": 2})
        for ua in ("alpha", "beta"):
            r = c.get("/vary/ua/1", headers={"User-Agent": ua})       # stale, from the cache
            assert f"ua={ua}".encode() in r.body().read()
        assert tc.wait_stat(px, "revalidations", 2) == 2     # both variants were stale
        assert px.stats()["stale_served"] == 2
        # the sibling URL with the same prefix stayed fresh
        c.get("/vary/ua/10", headers={"User-Agent": "alpha"})
        st = px.stats()
        assert st["stale_served"] == 2 and st["revalidations"] == 2
        assert st["soft_purge_requests"] == 1 and st["softened_objects"] == 3
        assert st["purged_objects"] == 0


def test_revalidation_in_flight_when_the_soft_purge_arrives_does_not_make_it_fresh(etag_origin):
    o = etag_origin
    with _proxy(o.port, ttl=60, grace=30) as px:
        c = HttpClient(port=px.port)
        assert c.get("/rv/e").body().read() == o.body("/rv/e", '"v1"')
        assert sc.soft_purge(c, "/rv/", prefix=True)[1]["softened"] == 1
        o.delays["/rv/e"] = 0.3
        o.cc304["/rv/e"] = "max-age=60"
        assert c.get("/rv/e").body().read() == o.body("/rv/e", '"v1"')     # starts a revalidation
        assert tc.wait_stat(px, "revalidations", 1) == 1
        assert sc.soft_purge(c, "/rv/", prefix=True)[1]["softened"] == 1   # ...and overtakes it
        assert o.wait_seen("/rv/e", 2)[1] == ("/rv/e", '"v1"', 304)
        assert tc.wait_stat(px, "revalidated_304", 1) == 1
        assert tc.wait_stat(px, "fills_not_cached_purged", 1) == 1
        st = px.stats()
        assert st["revalidate_touched"] == 0 and st["revalidate_restored"] == 0
        o.delays["/rv/e"] = 0
        # still stale: the next hit is served from the cache and revalidates again
        assert c.get("/rv/e").body().read() == o.body("/rv/e", '"v1"')
        assert o.wait_seen("/rv/e", 3)[2] == ("/rv/e", '"v1"', 304)
        assert tc.wait_stat(px, "revalidate_touched", 1) == 1
        assert px.stats()["stale_served"] == 2


def test_without_grace_a_soft_purge_is_a_hard_one(origin):
    with _proxy(origin.port, ttl=60) as px:
        c = HttpClient(port=px.port)
        for p in ("/ng/1", "/ng/2", "/ng/3"):
            c.get(p)
        assert sc.soft_purge(c, "/ng/1") == \
            (200, {"mode": "exact", "soft": False, "found": True, "variants": 0})
        assert sc.soft_purge(c, "/ng/", prefix=True) == \
            (200, {"mode": "prefix", "soft": False, "purged": 2})
        assert px.backend.get(b"localhost/ng/2") is None
        c.get("/ng/2")
        assert origin.hits["/ng/2"] == 2
        st = px.stats()
        assert st["soft_purge_requests"] == 0 and st["softened_objects"] == 0
        assert st["purge_requests"] == 2 and st["purged_objects"] == 3


def test_over_a_memcached_tier_a_soft_purge_is_a_hard_one(origin):
    f = FakeMemcached().start()
    try:
        be = make_backend("memcached", caches=[("127.0.0.1", f.port)])
        with _proxy(origin.port, backend=be, ttl=60, grace=30) as px:
            c = HttpClient(port=px.port)
            c.get("/mc/1")
            deadline = time.time() + 3
            while b"localhost/mc/1" not in f.data and time.time() < deadline:
                time.sleep(0.01)
            status, body = sc.soft_purge(c, "/mc/1")
            assert (status, body) == (200, {"mode": "exact", "soft": False, "found": True,
                                            "variants": -1})
            assert b"localhost/mc/1" not in f.data
            c.get("/mc/1")
            assert origin.hits["/mc/1"] == 2
            assert sc.soft_purge(c, "/mc/", prefix=True)[0] == 501   # as the hard prefix purge
            assert px.stats()["soft_purge_requests"] == 0
    finally:
        f.stop()


def test_request_without_the_header_gets_the_unchanged_answer(origin):
    with _proxy(origin.port, ttl=60, grace=30) as px:
        pc.prefix_purge_round_trip(px, origin)
        st = px.stats()
        assert st["soft_purge_requests"] == 0 and st["softened_objects"] == 0
        c = HttpClient(port=px.port)
        c.get("/h/1")
        # any other value of the header is not a soft purge
        r = c.get("/h/1", method="PURGE", headers={"X-Purge-Soft": "0"})
        assert r.body().read() == b'{"mode":"exact","found":true,"variants":0}\n'
