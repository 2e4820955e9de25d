"""Cache invalidation on the GPU: k_keyed_scan<PrefixMatch, RemoveAction> against its host twin and a Python model,
the HBM backend's purge request, hot replicas, and the proxy's PURGE over the HBM tier."""
import time

import numpy as np
import pytest
import torch

import purge_cases as pc
from shellac_amd import core
from shellac_amd.ops.cache import digest_strings, item_bytes, keyed
from shellac_amd.server.proxy import Server, hot_refresh, make_backend
from shellac_amd.utils.origin import Origin

pytestmark = pytest.mark.gpu

M64 = 2 ** 64 - 1


@pytest.fixture(scope="module")
def objects():
    """~3000 objects in 4096 index slots: both buckets of many pairs fill, so relocated
    entries are scanned too."""
    return pc.family_objects(3000)


def _twins(cuda_dev, objs, **kw):
    g, h = pc.make_shard(cuda_dev, **kw), pc.make_shard("cpu", **kw)
    for sh in (g, h):
        pc.store(sh, objs)
    return g, h


def _check_twins(g, h, objs, prefix):
    live_g, live_h = pc.live_keys(g, objs), pc.live_keys(h, objs)
    # At this index load an insert now and then finds both buckets full and evicts a live
    # entry; which one depends on the order the GPU's lanes insert in, so a twin may hold a
    # key or two the other lost. Those are DELETEd first: both twins then hold the same set.
    common = live_g & live_h
    assert len(common) >= 0.99 * max(len(live_g), len(live_h))
    for sh, live in ((g, live_g), (h, live_h)):
        extra = sorted(live - common)
        if extra:
            assert sh.remove(digest_strings(extra, sh.device)).all()
    want_n, want_bytes, survivors = pc.model_purge(objs, common, prefix)
    got_h = h.remove_keyed_prefix(prefix)
    got_g = g.remove_keyed_prefix(prefix)
    assert got_g == got_h == (want_n, want_bytes)
    assert pc.live_keys(g, objs) == pc.live_keys(h, objs) == survivors
    assert g.counters()["purged"] == h.counters()["purged"]
    return want_n


def test_twin_comparison_over_path_families(cuda_dev, objects):
    g, h = _twins(cuda_dev, objects)
    live0 = pc.live_keys(g, objects) & pc.live_keys(h, objects)
    assert len(live0) > 2900
    total = 0
    for prefix in (b"/static/js/", b"/nothing/here/", b"/static/", b"/api/v1/users/", b"/"):
        total += _check_twins(g, h, objects, prefix)
    assert total == len(live0) and g.counters()["purged"] == total
    assert g.sweep()[0] == h.sweep()[0] == 0


@pytest.mark.parametrize("plen", pc.BOUNDARY_PLENS)
def test_twin_comparison_at_granule_boundaries(cuda_dev, plen):
    pat, objs, must_go = pc.boundary_objects(plen)
    bystanders = {k: v for k, v in pc.family_objects(50, seed=plen).items()
                  if not k.startswith(pat)}
    allobjs = {**objs, **bystanders}
    g, h = _twins(cuda_dev, allobjs)
    assert _check_twins(g, h, allobjs, pat) == len(must_go)
    got = dict(zip(objs, g.get_many(list(objs))))
    for k in objs:
        assert (got[k] is None) == (k in must_go), (plen, k)


def test_twin_comparison_on_garbage_values(cuda_dev):
    junk = pc.garbage_values()
    g, h = _twins(cuda_dev, junk)
    for pat in (b"/", b"/abc", b"\xff", b"\xff" * 38, b"/abcdefghi", b"x" * 300, b"y" * 65535):
        assert g.remove_keyed_prefix(pat) == h.remove_keyed_prefix(pat), pat
    assert g.get_many(list(junk)) == h.get_many(list(junk))
    with pytest.raises(Exception):
        g.remove_keyed_prefix(b"")


def test_twin_comparison_after_the_log_lapped(cuda_dev):
    # (payloads up to 1500 B: the ~1300 objects a full log holds stay far below the 4096
    # index slots, so no index eviction, whose victims differ between the twins, interferes)
    objs = pc.family_objects(6000, seed=11, max_payload=1500)
    g, h = _twins(cuda_dev, objs)
    assert g.head() == h.head() > 3 * g.log_bytes
    assert 0 < _check_twins(g, h, objs, b"/static/") < len(objs)


def test_expired_entries_are_not_counted(cuda_dev):
    g = pc.make_shard(cuda_dev)
    fresh = {b"/x/keep/%d" % i: keyed(b"/x/keep/%d" % i, b"v") for i in range(10)}
    dying = {b"/x/ttl/%d" % i: keyed(b"/x/ttl/%d" % i, b"v") for i in range(7)}
    pc.store(g, fresh)
    pc.store(g, dying, ttl=5)
    assert g.remove_keyed_prefix(b"/x/", now=g.now() + 100)[0] == len(fresh)


@pytest.mark.parametrize("dev", ["cuda", "cpu"])
def test_dead_same_digest_entry_is_not_counted(cuda_dev, dev):
    """A dead entry with the key's digest (expired, pointing at the very same record)
    beside the live one, and a locked slot: only the live entry is removed and counted."""
    nb = 1 << 10
    s = pc.make_shard(cuda_dev if dev == "cuda" else "cpu")
    key = b"/twin/object"
    s.set_many([b"/pre/%d" % i for i in range(3)], [keyed(b"/pre/%d" % i, b"p") for i in range(3)])
    s.set_many([key], [keyed(key, b"t" * 100)])
    lo, hi = (int(x) & M64 for x in digest_strings([key], "cpu")[0])
    b1, b2 = core().bucket_pair(lo, hi, nb)
    e1, e2 = s._impl.debug_bucket(b1), s._impl.debug_bucket(b2)
    i = next(k for k in range(4) if e1[4 * k] == lo and e1[4 * k + 1] == hi and e1[4 * k + 2])
    free = [k for k in range(4) if e2[4 * k + 2] == 0]
    loc, vx = e1[4 * i + 2], e1[4 * i + 3]
    s._impl.debug_set_entry(b2, free[0], lo, hi, loc, vx & 0xFFFFFFFF, 1)      # expired at t=1
    s._impl.debug_set_entry(b2, free[1], lo, hi, M64 - 1, vx & 0xFFFFFFFF, 0)  # locked
    assert s.remove_keyed_prefix(b"/twin/") == (1, item_bytes(len(keyed(key, b"t" * 100))))
    assert s.counters()["purged"] == 1
    after = s._impl.debug_bucket(b2)
    assert after[4 * free[0] + 2] == loc and after[4 * free[1] + 2] == M64 - 1  # left alone
    assert s.get_many([key]) == [None]


def test_clock_hand_does_not_resurrect_purged_objects_gpu(cuda_dev):
    c = pc.clock_never_resurrects(pc.make_shard(cuda_dev))
    assert c["purged"] == 150


def test_purge_beside_sets_on_a_second_stream(cuda_dev):
    """A purge on one stream while SET batches on another append to the log, lapping it
    (FIFO, so the twin tells exactly which records get overwritten): memory-safe through
    the header re-check, and no object outside the prefix is lost — the survivors include
    every non-matching key stored before the purge was queued that the SETs did not
    overwrite (that set comes from the host twin)."""
    base = pc.family_objects(2000, seed=5)
    fills = [{b"/fill/%d/%d" % (b, i): keyed(b"/fill/%d/%d" % (b, i), b"f" * 600)
              for i in range(400)} for b in range(3)]
    # (8192 index slots for 3200 keys: no index eviction, whose victim could differ between
    # a concurrent and a sequential insert)
    g, h = _twins(cuda_dev, base, evict="fifo", nbuckets=1 << 11)
    s1, s2 = torch.cuda.Stream(cuda_dev), torch.cuda.Stream(cuda_dev)
    torch.cuda.synchronize(cuda_dev)
    prefix = b"/static/"
    img = torch.from_numpy(np.frombuffer(core().keyed_prefix_image(prefix), np.uint8).copy())
    img = img.to(cuda_dev)
    out = torch.zeros(2, dtype=torch.int64, device=cuda_dev)
    torch.cuda.synchronize(cuda_dev)
    with torch.cuda.stream(s2):
        pc.store(g, fills[0], batch=400)
    with torch.cuda.stream(s1):
        g._impl.remove_keyed_prefix(img.data_ptr(), len(prefix), g.now(), out.data_ptr(),
                                    s1.cuda_stream)
    with torch.cuda.stream(s2):
        for f in fills[1:]:
            pc.store(g, f, batch=400)
    torch.cuda.synchronize(cuda_dev)
    for f in fills:
        pc.store(h, f, batch=400)
    assert g.head() == h.head() > g.log_bytes
    must_survive = {k for k in pc.live_keys(h, base) if not k.startswith(prefix)}
    assert must_survive
    live = pc.live_keys(g, {**base, **fills[-1]})
    assert must_survive <= live
    assert set(fills[-1]) <= live
    removed = int(out[0].item())
    assert 0 <= removed <= sum(k.startswith(prefix) for k in base)
    assert g.counters()["purged"] == removed


# ------------------------------------------------------------------------------ HbmBackend
def _wait_get(be, key, timeout=5.0):
    deadline = time.time() + timeout
    while time.time() < deadline:
        r = be.get(key)
        if r is not None:
            return r
        time.sleep(0.005)
    return None


@pytest.mark.parametrize("edge_server", [True, False])
def test_hbm_backend_purge_prefix(edge_server):
    be = make_backend("hbm", gpus=[0], hbm_gb=0.25, edge_server=edge_server)
    fam = {f: [f + b"%d" % i for i in range(64)] for f in (b"/a/", b"/b/")}
    for f in fam:
        for k in fam[f]:
            be.set(k, b"value of " + k * 5, 0, 0)
    assert _wait_get(be, fam[b"/b/"][-1]) is not None
    assert all(v is not None for v in be.get_many(fam[b"/a/"] + fam[b"/b/"]))
    assert be.purge_prefix(b"/a/") == 64
    # after `done` every GET path misses: the launched and the served / reactor-direct ones
    for _ in range(3):
        assert be.get_many(fam[b"/a/"]) == [None] * 64
        assert all(be.get(k) is None for k in fam[b"/a/"][:8])
    assert all(v == (b"value of " + k * 5, 0) for k, v in zip(fam[b"/b/"], be.get_many(fam[b"/b/"])))
    assert be.purge_prefix(b"/a/") == 0
    st = be.stats()
    assert st["hbm_purges"] == 2 and st["hbm_purged_objects"] == 64
    assert st["hbm_purged_bytes"] == sum(item_bytes(len(keyed(k, b"value of " + k * 5)))
                                         for k in fam[b"/a/"])
    # a SET queued behind the purge is not caught by it
    be.set(b"/a/new", b"fresh", 0, 0)
    assert _wait_get(be, b"/a/new") == (b"fresh", 0)
    assert be.purge_prefix(b"") == -1   # refused by every tier (that is flush())


@pytest.mark.parametrize("purge_while_out", [False, True])
def test_shard_out_of_service_during_a_purge_is_flushed_on_restore(purge_while_out):
    """flush_on_restore off: a shard back from ejection keeps its objects — unless a purge
    arrived while it was out. It could not scan then, so its restore flushes it and no
    purged object comes back with it (the control run keeps everything)."""
    be = core().hbm_backend([0], 64 << 20, 1 << 14, 1 << 16, 0, flush_on_restore=False,
                            warm_restore=False)
    fam = {f: [f + b"%d" % i for i in range(32)] for f in (b"/a/", b"/b/")}
    for f in fam:
        for k in fam[f]:
            be.set(k, b"v-" + k, 0, 0)
    assert _wait_get(be, fam[b"/b/"][-1]) is not None
    assert core().inject_shard_down(be, 0, True)
    assert be.get(fam[b"/a/"][0]) is None            # out of the ring: everything misses
    if purge_while_out:
        assert be.purge_prefix(b"/a/") == 0          # no shard in service scanned anything
    core().inject_shard_down(be, 0, False)
    deadline = time.time() + 5
    while be.stats()["hbm_gpus_up"] == 0 and time.time() < deadline:
        time.sleep(0.02)
    assert be.stats()["hbm_gpus_up"] == 1
    got = be.get_many(fam[b"/a/"] + fam[b"/b/"])
    if purge_while_out:
        assert got == [None] * 64
    else:
        assert all(g == (b"v-" + k, 0) for g, k in zip(got, fam[b"/a/"] + fam[b"/b/"]))


def test_purge_removes_hot_replicas_on_every_shard():
    """Two shards on GPU 0 with hot spreading: after a refresh the hot objects live on both
    shards; a prefix purge scans every shard, so a spread GET of a purged hot key misses
    wherever it lands."""
    be = core().hbm_backend([0, 0], 64 << 20, 1 << 14, 1 << 16, 0, hot_objects=64,
                            hot_refresh_ms=0, hot_sample=1)
    a = [b"/hp/a/%d" % i for i in range(200)]
    b = [b"/hp/b/%d" % i for i in range(200)]
    for k in a + b:
        be.set(k, b"v-" + k * 4, 0, 0)
    assert _wait_get(be, b[-1]) is not None and _wait_get(be, a[-1]) is not None
    hot = a[:16] + b[:16]
    for _ in range(40):
        be.get_many(hot)
    info = hot_refresh(be)
    assert info["hot"] >= 32 and info["spread_mask"] == 3, info
    assert all(v is not None for v in be.get_many(hot * 8))
    st0 = be.stats()
    n = be.purge_prefix(b"/hp/a/")
    assert n > 200                # the owners' copies and replicas of the hot ones
    assert be.get_many(a[:16] * 16) == [None] * 256   # every replica the spread can pick
    assert be.get_many(a) == [None] * 200
    assert all(v == (b"v-" + k * 4, 0) for k, v in zip(b, be.get_many(b)))
    st = be.stats()
    assert st["hbm_purged_objects"] - st0["hbm_purged_objects"] == n
    assert st["hbm_hot_spread_gets"] > 0


def test_purge_between_a_refresh_snapshot_and_its_fill_resurrects_nothing():
    """A hot-set refresh snapshots the new hot objects on their owners and only later queues
    the replica fills. A purge queued in between scans the target shard before its fill: the
    fill must not store the pre-purge records there (a purge has no digests to mark, so it
    marks every object being filled as written). After `done`, no GET finds a purged
    object on any replica; the objects outside the prefix are still served."""
    be = core().hbm_backend([0, 0], 64 << 20, 1 << 14, 1 << 16, 0, hot_objects=64,
                            hot_refresh_ms=0, hot_sample=1)
    a = [b"/hr/a/%d" % i for i in range(100)]
    b = [b"/hr/b/%d" % i for i in range(100)]
    for k in a + b:
        be.set(k, b"v-" + k * 4, 0, 0)
    assert _wait_get(be, b[-1]) is not None and _wait_get(be, a[-1]) is not None
    hot = a[:16] + b[:16]
    for _ in range(40):
        be.get_many(hot)
    info, removed = core().hot_refresh_purging(be, b"/hr/a/")
    assert info["hot"] >= 32 and info["added"] >= 32, info   # the first refresh: all new
    assert removed == 100          # the owners' copies; no replica existed yet
    for _ in range(4):
        assert be.get_many(a[:16] * 16) == [None] * 256      # wherever the spread sends it
    assert be.get_many(a) == [None] * 100
    got = be.get_many(b)
    # (a hot /b/ object whose fill row was dropped may miss on its replica: a miss is a
    # valid answer; what it returns is never anything but its value)
    assert all(g in (None, (b"v-" + k * 4, 0)) for g, k in zip(got, b))
    assert all(g == (b"v-" + k * 4, 0) for g, k in zip(got[16:], b[16:]))
    assert be.purge_prefix(b"/hr/a/") == 0                   # nothing of it anywhere


def test_proxy_purge_over_the_hbm_backend():
    be = make_backend("hbm", gpus=[0], hbm_gb=0.25)
    o = Origin(body_bytes=200).start()
    try:
        with Server([("127.0.0.1", o.port)], port=0, backend=be, threads=2,
                    purge="loopback") as px:
            def settle():  # the tier stores a fill a moment after the response went out
                assert _wait_get(be, b"localhost/b/20") is not None
                assert _wait_get(be, b"localhost/a/20") is not None
            pc.prefix_purge_round_trip(px, o, settle)
    finally:
        o.stop()
