"""Soft purge on the GPU: k_keyed_scan<PrefixMatch, SoftenAction> against its host twin and the Python model, the
HBM backend's soft purge request, hot replicas, and the proxy's PURGE with X-Purge-Soft over
the HBM tier."""
import time

import pytest

import purge_cases as pc
import soften_cases as sc
import touch_cases as tc
from shellac_amd import core
from shellac_amd.ops.cache import digest_strings, keyed, pack_values
from shellac_amd.server.proxy import Server, hot_refresh, make_backend

pytestmark = pytest.mark.gpu

T0, M64 = sc.T0, 2 ** 64 - 1


def _twins(cuda_dev, objs, mixed=True, **kw):
    g, h = pc.make_shard(cuda_dev, **kw), pc.make_shard("cpu", **kw)
    for sh in (g, h):
        if mixed:
            sc.store_mixed(sh, objs)
        else:
            tc.store_at(sh, objs, T0 + sc.TTL0, flags=1)
    return g, h


# ------------------------------------------------------------------- twins and the model
@pytest.fixture(scope="module")
def objects():
    """~3000 objects in 4096 index slots: both buckets of many pairs fill, so relocated
    entries are scanned too."""
    return pc.family_objects(3000)


def test_twin_comparison_over_path_families(cuda_dev, objects):
    g, h = _twins(cuda_dev, objects)
    model = sc.equalise(g, h, objects)
    assert len(model) > 2900
    a_key = sorted(k for k in model if k.startswith(b"/img/"))[0]
    counts, chain = [], []
    for pattern, exact, cap in [(b"/static/js/", False, T0 + 80), (b"/nothing/here/", False, 0),
                                (a_key, True, T0 + 80), (b"/static/", True, T0 + 80),
                                (b"/api/v1/users/", False, T0 + 10 ** 6), (b"/", False, T0 + 300)]:
        n, model = sc.check_soften([g, h], objects, model, pattern, exact, cap,
                                   stale_at=sc.STALE_AT + len(counts), chain=chain)
        counts.append(n)
    assert counts[0] > 0 and counts[1:4] == [0, 1, 0] and counts[4] > 0
    assert counts[5] == len(model) > 2900                         # b"/" reached every object
    assert all(f == sc.STALE_AT + 5 for _, f in model.values())
    assert g.counters()["touched"] == h.counters()["touched"] == 0   # the op has no counter


@pytest.mark.parametrize("exact", [False, True])
@pytest.mark.parametrize("plen", pc.BOUNDARY_PLENS)
def test_twin_comparison_at_granule_boundaries(cuda_dev, plen, exact):
    pat, objs, must_prefix = sc.exact_boundary_objects(plen)
    bystanders = {k: v for k, v in pc.family_objects(50, seed=plen).items()
                  if not k.startswith(pat)}
    allobjs = {**objs, **bystanders}
    g, h = _twins(cuda_dev, allobjs, mixed=False)
    model = sc.equalise(g, h, allobjs)
    assert set(model) == set(allobjs)
    n, model2 = sc.check_soften([g, h], allobjs, model, pat, exact, T0 + 50)
    softened = {k for k in allobjs if model2[k][1] == sc.STALE_AT}
    assert softened == ({pat} if exact else must_prefix | {k for k in objs if k.startswith(pat)})
    assert n == len(softened) and (exact or must_prefix <= softened)


def test_twin_comparison_on_garbage_values(cuda_dev):
    junk = pc.garbage_values()
    g, h = _twins(cuda_dev, junk, mixed=False)
    before = g.get_many(list(junk))
    for pat in (b"/", b"/abc", b"\xff", b"\xff" * 38, b"/abcdefghi", b"x" * 300, b"y" * 65535):
        for exact in (False, True):
            got = [sh.soften_keyed_prefix(pat, 77, T0 + 50, exact=exact, now=T0) for sh in (g, h)]
            assert got[0] == got[1] == 0, (pat, exact)     # none parses as a matching record
    # nothing outside a record was written: values, flags, expiries and liveness as before
    assert g.get_many(list(junk)) == h.get_many(list(junk)) == before
    assert sc.snapshot(g, junk) == sc.snapshot(h, junk)
    assert sc.model_of(g, junk) == {k: (T0 + sc.TTL0, 1) for k in junk}
    with pytest.raises(Exception):
        g.soften_keyed_prefix(b"", 1)
    with pytest.raises(Exception):
        g.soften_keyed_prefix(b"/a", 1, expire_cap=T0, now=T0)


def test_twin_comparison_after_the_log_lapped(cuda_dev):
    # (payloads up to 1500 B: the ~1300 objects a full log holds stay far below the 4096
    # index slots, so no index eviction, whose victims differ between the twins, interferes)
    objs = pc.family_objects(6000, seed=11, max_payload=1500)
    g, h = _twins(cuda_dev, objs)
    assert g.head() == h.head() > 3 * g.log_bytes
    model = sc.equalise(g, h, objs)
    assert 0 < len(model) < len(objs) // 2
    n, _ = sc.check_soften([g, h], objs, model, b"/static/", False, T0 + 80)
    assert 0 < n < len(model)


@pytest.mark.parametrize("dev", ["cuda", "cpu"])
def test_dead_entries_are_neither_counted_nor_written(cuda_dev, dev):
    """An expired family, and beside one live entry a dead entry with the same digest
    (expired, pointing at the very same record) and a locked slot: only the live entries are
    counted, and the dead ones keep every word."""
    nb = 1 << 10
    s = pc.make_shard(cuda_dev if dev == "cuda" else "cpu")
    dying = {b"/twin/ttl/%d" % i: keyed(b"/twin/ttl/%d" % i, b"v") for i in range(7)}
    tc.store_at(s, dying, T0 + 5, flags=1)
    key = b"/twin/object"
    tc.store_at(s, {b"/pre/%d" % i: keyed(b"/pre/%d" % i, b"p") for i in range(3)}, 0)
    tc.store_at(s, {key: keyed(key, b"t" * 100)}, T0 + 500, flags=1)
    lo, hi = (int(x) & M64 for x in digest_strings([key], "cpu")[0])
    b1, b2 = core().bucket_pair(lo, hi, nb)
    e1, e2 = s._impl.debug_bucket(b1), s._impl.debug_bucket(b2)
    i = next(k for k in range(4) if e1[4 * k] == lo and e1[4 * k + 1] == hi and e1[4 * k + 2])
    free = [k for k in range(4) if e2[4 * k + 2] == 0]
    loc, vx = e1[4 * i + 2], e1[4 * i + 3]
    s._impl.debug_set_entry(b2, free[0], lo, hi, loc, vx & 0xFFFFFFFF, 1)      # expired at t=1
    s._impl.debug_set_entry(b2, free[1], lo, hi, M64 - 1, vx & 0xFFFFFFFF, 0)  # locked
    assert s.soften_keyed_prefix(b"/twin/", 9, T0 + 100, now=T0 + 5) == 1
    after1, after2 = s._impl.debug_bucket(b1), s._impl.debug_bucket(b2)
    assert after2[4 * free[0]:4 * free[0] + 4] == [lo, hi, loc, (vx & 0xFFFFFFFF) | (1 << 32)]
    assert after2[4 * free[1]:4 * free[1] + 4] == [lo, hi, M64 - 1, vx & 0xFFFFFFFF]
    assert after1[4 * i + 2] == loc and after1[4 * i + 3] >> 32 == T0 + 100
    assert tc.records_at(s, [key], T0 + 5) == {key: (keyed(key, b"t" * 100), 9, T0 + 100)}
    # the expired family was not written: seen from before its expiry it is unchanged
    assert sc.model_of(s, dying, T0) == {k: (T0 + 5, 1) for k in dying}


def test_reference_bit_survives_a_softening_and_a_get_still_hits(cuda_dev):
    sh = pc.make_shard(cuda_dev)
    objs = {k: keyed(k, b"v" * 40) for k in (b"/ref/read", b"/ref/unread")}
    tc.store_at(sh, objs, T0 + 500, flags=1)
    assert tc.live_at(sh, {b"/ref/read": objs[b"/ref/read"]}, T0)
    assert tc.ref_bit(sh, b"/ref/read") == (True, T0 + 500)
    assert sh.soften_keyed_prefix(b"/ref/", 5, T0 + 100, now=T0) == 2
    assert tc.ref_bit(sh, b"/ref/read") == (True, T0 + 100)
    assert tc.ref_bit(sh, b"/ref/unread") == (False, T0 + 100)
    assert tc.records_at(sh, objs, T0 + 99) == {k: (v, 5, T0 + 100) for k, v in objs.items()}
    assert tc.records_at(sh, objs, T0 + 100) == {}
    # flags only (no cap): the words of the entry stay
    assert sh.soften_keyed_prefix(b"/ref/", 6, 0, now=T0) == 2
    assert tc.ref_bit(sh, b"/ref/read") == (True, T0 + 100)


def test_twin_comparison_clock_hand_keeps_the_softening(cuda_dev):
    g = sc.clock_keeps_the_softening(pc.make_shard(cuda_dev))
    h = sc.clock_keeps_the_softening(pc.make_shard("cpu"))
    assert g == h
    meta, live_at_cap, reinserted = g
    assert len(meta) == 20 and reinserted >= 20
    assert set(meta.values()) == {(sc.STALE_AT, T0 + sc.TTL0)}
    assert live_at_cap == set()


def test_soften_is_refused_while_a_detached_hand_is_pending(cuda_dev):
    sh = pc.make_shard(cuda_dev)
    objs = {b"/p/%d" % i: keyed(b"/p/%d" % i, b"v") for i in range(4)}
    keys = list(objs)
    d = digest_strings(keys, sh.device)
    v, vo, vl = pack_values([objs[k] for k in keys], sh.device)
    ex = tc.i32([0] * 4, sh.device)
    sh.store(d, v, vo, vl, None, ex, now=T0, phase=1)
    with pytest.raises(Exception, match="phase-1"):
        sh.soften_keyed_prefix(b"/p/", 5, now=T0)
    sh.store(d, v, vo, vl, None, ex, now=T0, phase=2)
    assert sh.soften_keyed_prefix(b"/p/", 5, T0 + 9, now=T0) == 4
    assert sc.model_of(sh, objs) == {k: (T0 + 9, 5) for k in keys}


# ------------------------------------------------------------------------------ HbmBackend
def _wait_get(be, key, timeout=5.0):
    deadline = time.time() + timeout
    while time.time() < deadline:
        r = be.get(key)
        if r is not None:
            return r
        time.sleep(0.005)
    return None


def _ttl_near(got, want):
    return got is not None and want - 3 <= got[2] <= want


def test_hbm_backend_soft_purge_behind_queued_sets_softens_them_too():
    be = make_backend("hbm", gpus=[0], hbm_gb=0.25)
    a = [b"/q/a/%d" % i for i in range(64)]
    b = [b"/q/b/%d" % i for i in range(64)]
    for k in a + b:
        be.set(k, b"value of " + k * 5, 3, 5000)
    # queued right behind the SETs: it runs after them on the shard's stream
    assert be.soften_prefix(b"/q/a/", 1234, keep_s=100) == 64
    for k in a:
        got = be.get_ttl(k)
        assert got[:2] == (b"value of " + k * 5, 1234) and _ttl_near(got, 100), (k, got)
    for k in b:
        got = be.get_ttl(k)
        assert got[:2] == (b"value of " + k * 5, 3) and _ttl_near(got, 5000), (k, got)
    assert be.soften_prefix(b"/q/a/", 1235) == 64                  # the same count; flags only
    assert _ttl_near(be.get_ttl(a[0]), 100) and be.get_ttl(a[0])[1] == 1235
    assert be.soften_prefix(b"/q/a/7", 99, exact=True) == 1
    assert be.get(a[7])[1] == 99 and be.get(b"/q/a/70") is None and be.get(a[6])[1] == 1235
    assert be.soften_prefix(b"", 5) == -1
    st = be.stats()
    assert st["hbm_soft_purges"] == 3 and st["hbm_softened_objects"] == 64 + 64 + 1
    assert st["hbm_purged_objects"] == 0 and st["hbm_purges"] == 3
    # a SET queued behind the soft purge is not caught by it
    be.set(b"/q/a/new", b"fresh", 3, 0)
    assert _wait_get(be, b"/q/a/new") == (b"fresh", 3)


def test_soft_purge_softens_hot_replicas_on_every_shard():
    """Two shards on GPU 0 with hot spreading: a soft purge scans every shard, so a spread GET
    of a softened hot key shows the stale flags wherever it lands."""
    be = core().hbm_backend([0, 0], 64 << 20, 1 << 14, 1 << 16, 0, hot_objects=64,
                            hot_refresh_ms=0, hot_sample=1)
    a = [b"/hp/a/%d" % i for i in range(200)]
    b = [b"/hp/b/%d" % i for i in range(200)]
    for k in a + b:
        be.set(k, b"v-" + k * 4, 3, 0)
    assert _wait_get(be, b[-1]) is not None and _wait_get(be, a[-1]) is not None
    hot = a[:16] + b[:16]
    for _ in range(40):
        be.get_many(hot)
    info = hot_refresh(be)
    assert info["hot"] >= 32 and info["spread_mask"] == 3, info
    st0 = be.stats()
    n = be.soften_prefix(b"/hp/a/", 1234, keep_s=100)
    assert n > 200                # the owners' copies and replicas of the hot ones
    got = be.get_many(a[:16] * 16)                 # every replica the spread can pick
    assert got == [(b"v-" + k * 4, 1234) for k in a[:16]] * 16
    assert be.get_many(a) == [(b"v-" + k * 4, 1234) for k in a]
    assert be.get_many(b) == [(b"v-" + k * 4, 3) for k in b]
    for _ in range(4):
        for k in a[:16]:
            assert _ttl_near(be.get_ttl(k), 100)
    st = be.stats()
    assert st["hbm_softened_objects"] - st0["hbm_softened_objects"] == n
    assert st["hbm_hot_spread_gets"] > st0["hbm_hot_spread_gets"]


def test_soft_purge_overlapping_a_hot_refresh_leaves_no_fresh_copy():
    """A hot-set refresh snapshots the new hot objects on their owners and only later queues
    the replica fills. A soft purge queued in between scans the target shard before its fill:
    the fill must not store the pre-purge (fresh) records there. Afterwards no GET finds a
    fresh copy of a softened object on any replica."""
    be = core().hbm_backend([0, 0], 64 << 20, 1 << 14, 1 << 16, 0, hot_objects=64,
                            hot_refresh_ms=0, hot_sample=1)
    a = [b"/hr/a/%d" % i for i in range(100)]
    b = [b"/hr/b/%d" % i for i in range(100)]
    for k in a + b:
        be.set(k, b"v-" + k * 4, 3, 0)
    assert _wait_get(be, b[-1]) is not None and _wait_get(be, a[-1]) is not None
    hot = a[:16] + b[:16]
    for _ in range(40):
        be.get_many(hot)
    info, softened = core().hot_refresh_softening(be, b"/hr/a/", 1234, 100)
    assert info["hot"] >= 32 and info["added"] >= 32, info   # the first refresh: all new
    assert softened == 100         # the owners' copies; no replica existed yet
    for _ in range(4):
        got = be.get_many(a[:16] * 16)                       # wherever the spread sends it
        # (a hot object whose fill row was dropped may miss on its replica: a miss is a valid
        # answer; what is returned is never the fresh copy)
        assert all(g in (None, (b"v-" + k * 4, 1234)) for g, k in zip(got, a[:16] * 16)), got
    assert be.get_many(a[16:]) == [(b"v-" + k * 4, 1234) for k in a[16:]]
    got = be.get_many(b)
    assert all(g in (None, (b"v-" + k * 4, 3)) for g, k in zip(got, b))
    assert all(g == (b"v-" + k * 4, 3) for g, k in zip(got[16:], b[16:]))


def test_proxy_soft_purge_over_the_hbm_backend():
    """One HTTP round trip over --cache hbm: soft prefix purge, a stale hit, a 304, then
    fresh — the object is softened and extended on the GPU, and no SET reaches the shard."""
    be = make_backend("hbm", gpus=[0], hbm_gb=0.25)
    o = tc.EtagOrigin().start()
    try:
        with Server([("127.0.0.1", o.port)], port=0, backend=be, ttl=60, grace=30,
                    purge="loopback") as px:
            def settle():  # the tier stores a fill a moment after the response went out
                assert _wait_get(be, b"localhost/sp/a") is not None
            sc.soft_purge_304_round_trip(px, o, "/sp/a", settle)
            st = be.stats()
            assert st["cache_set_ops"] == 1
            assert st["hbm_soft_purges"] == 1 and st["hbm_softened_objects"] == 1
            assert st["hbm_touches"] == 1 and st["hbm_touched"] == 1
            assert _ttl_near(be.get_ttl(b"localhost/sp/a"), 60 + 30)   # the 304's max-age + grace
    finally:
        o.stop()
