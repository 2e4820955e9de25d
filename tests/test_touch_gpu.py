"""In-place touch on the GPU: k_touch against its host twin on the scenarios of
tests/test_touch.py, batch and key-length edges of the 16-lane groups, the CLOCK reference
bit, un-keyed values, and a touch beside SETs on a second stream."""
import random
import time

import pytest
import torch

import purge_cases as pc
import touch_cases as tc
from shellac_amd import core
from shellac_amd.ops.cache import digest_strings, keyed
from shellac_amd.server.proxy import Server, hot_refresh, make_backend
from shellac_amd.utils.httpclient import HttpClient

pytestmark = pytest.mark.gpu


def test_twin_comparison_mixed_expiries(cuda_dev):
    # 1000 objects in 4096 slots: no insert finds both buckets full (mixed_touch asserts that
    # each twin holds every stored key before the touch)
    g = tc.mixed_touch(pc.make_shard(cuda_dev))
    h = tc.mixed_touch(pc.make_shard("cpu"))
    assert g[0] == h[0] == g[1]                     # hit vectors, and the model's
    for now in tc.NOWS:
        assert g[2][now] == h[2][now] == g[3][now], now
    assert g[4] == h[4] == sum(g[1])                # counters
    assert g[5] == h[5]                             # flags and header expiries


def test_twin_comparison_forged_collision(cuda_dev):
    assert tc.forged_collision(pc.make_shard(cuda_dev)) == tc.FORGED_WANT
    assert tc.forged_collision(pc.make_shard("cpu")) == tc.FORGED_WANT


def test_twin_comparison_dead_entries(cuda_dev):
    kw = dict(log_bytes=256 << 10, evict="fifo")
    g = tc.dead_entries(pc.make_shard(cuda_dev, **kw))
    h = tc.dead_entries(pc.make_shard("cpu", **kw))
    assert g == h
    hit, hit2, want, live, alive, touched = g
    assert hit == want and hit2 == want and live == alive and touched == 2 * len(alive)


def test_twin_comparison_clock_hand_keeps_the_touch(cuda_dev):
    g = tc.clock_keeps_the_touch(pc.make_shard(cuda_dev))
    h = tc.clock_keeps_the_touch(pc.make_shard("cpu"))
    assert g[:3] == h[:3]
    live, meta, live_after, reinserted = g
    assert len(live) == 20 and reinserted >= 20
    assert set(meta.values()) == {(0xC0FFEE00, tc.T0 + 1000)}
    assert live_after == set()


@pytest.fixture(scope="module")
def stocked():
    """3500 keyed objects on both twins (32768 slots: no insert finds both buckets full) and
    absent keys to mix in; shared by the batch-size cases, which touch disjoint slices."""
    kw = dict(log_bytes=4 << 20, nbuckets=1 << 13)
    objs = pc.family_objects(3500, seed=31, max_payload=120)
    g, h = pc.make_shard(torch.device("cuda", 0), **kw), pc.make_shard("cpu", **kw)
    for sh in (g, h):
        tc.store_at(sh, objs, tc.T0 + tc.TTL0)
        assert tc.live_at(sh, objs, tc.T0) == set(objs)
    return g, h, objs


# the 16-lane groups (4 per wave, 16 per workgroup): 1, 3..5 rows, 15..17, 255..257; 5000 and
# 40000 rows span many workgroups, the last more than one pass of the grid-stride loop
# (2048 workgroups x 16 rows)
@pytest.mark.parametrize("rows", [1, 3, 4, 5, 15, 16, 17, 255, 256, 257, 5000, 40000])
def test_batch_sizes(stocked, rows):
    g, h, objs = stocked
    rng = random.Random(rows)
    present = sorted(objs)
    if rows >= 5000:    # ~30 % absent digests (5000), mostly absent (40000)
        npres = min(int(rows * 0.7), len(present))
        keys = rng.sample(present, npres) + [b"/absent/%d/%d" % (rows, i)
                                              for i in range(rows - npres)]
        rng.shuffle(keys)
    else:
        keys = rng.sample(present, rows)
    exp = [rng.choice([0, tc.T0 + 300 + rows % 97, tc.T0 + 5000]) for _ in keys]
    fl = [rng.getrandbits(32) for _ in keys]
    want = [1 if k in objs else 0 for k in keys]
    c0 = g.counters()["touched"], h.counters()["touched"]
    hg, hh = tc.touch(g, keys, exp, fl), tc.touch(h, keys, exp, fl)
    assert hg == hh == want
    assert g.counters()["touched"] - c0[0] == h.counters()["touched"] - c0[1] == sum(want)
    t = tc.T0 + tc.TTL0 + 1
    mg, mh = tc.records_at(g, objs, t), tc.records_at(h, objs, t)
    assert mg == mh
    for k, e, f in zip(keys, exp, fl):
        if k in objs:
            assert mg[k] == (objs[k], f, e), k


@pytest.mark.parametrize("klen", tc.KLENS)
def test_only_the_exact_key_is_touched(cuda_dev, klen):
    g = tc.exact_key_only(pc.make_shard(cuda_dev), klen)
    h = tc.exact_key_only(pc.make_shard("cpu"), klen)
    assert g == h
    h1, a1, h2, a2, key = g
    assert h1 == [0, 0, 0, 0] and a1 == set()
    assert h2 == [1] and a2 == {key}


def test_reference_bit_survives_a_touch(cuda_dev):
    sh = pc.make_shard(cuda_dev)
    objs = {k: keyed(k, b"v") for k in (b"/ref/read", b"/ref/unread")}
    tc.store_at(sh, objs, tc.T0 + tc.TTL0)
    assert tc.live_at(sh, {b"/ref/read": objs[b"/ref/read"]}, tc.T0)
    assert tc.ref_bit(sh, b"/ref/read") == (True, tc.T0 + tc.TTL0)
    assert tc.touch(sh, list(objs), [tc.T0 + 500] * 2) == [1, 1]
    assert tc.ref_bit(sh, b"/ref/read") == (True, tc.T0 + 500)
    assert tc.ref_bit(sh, b"/ref/unread") == (False, tc.T0 + 500)


def test_twin_comparison_on_garbage_values(cuda_dev):
    g = tc.garbage_touch(pc.make_shard(cuda_dev))
    h = tc.garbage_touch(pc.make_shard("cpu"))
    assert g == h
    got, want, live = g
    assert got == want and live == {b"garbage/two"}


def test_touch_is_refused_while_a_detached_hand_is_pending(cuda_dev):
    sh = pc.make_shard(cuda_dev)
    objs = {b"/p/%d" % i: keyed(b"/p/%d" % i, b"v") for i in range(4)}
    keys = list(objs)
    d = digest_strings(keys, sh.device)
    from shellac_amd.ops.cache import pack_values
    v, vo, vl = pack_values([objs[k] for k in keys], sh.device)
    ex = tc.i32([0] * 4, sh.device)
    sh.store(d, v, vo, vl, None, ex, now=tc.T0, phase=1)
    with pytest.raises(Exception, match="phase-1"):
        sh.touch(d, ex, now=tc.T0)
    sh.store(d, v, vo, vl, None, ex, now=tc.T0, phase=2)
    assert tc.touch(sh, keys, [tc.T0 + 9] * 4) == [1] * 4


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


def test_hbm_backend_touch_reaches_every_replica_and_keeps_write_order():
    """Two shards on GPU 0 with hot spreading: a hot object's touch is written through, so a
    GET shows the new TTL and flags whichever replica answers; a touch queued between two
    SETs of a key lands between them."""
    be = core().hbm_backend([0, 0], 64 << 20, 1 << 14, 1 << 16, 0, hot_objects=64,
                            hot_refresh_ms=0, hot_sample=1)
    keys = [b"/ht/%d" % i for i in range(200)]
    for k in keys:
        be.set(k, b"v-" + k * 4, 1, 50)
    assert _wait_get(be, keys[-1]) is not None and _wait_get(be, keys[0]) is not None
    hot = keys[:16]
    for _ in range(40):
        be.get_many(hot)
    info = hot_refresh(be)
    assert info["hot"] >= 16 and info["spread_mask"] == 3, info
    st0 = be.stats()
    # every hot object: its GETs go to its designated shard, which for about half of them is
    # not the owner, so the answers below come from owners' copies and from replicas
    for k in hot:
        assert be.touch(k, 5000, flags=7) == 1
    for _ in range(4):
        for k in hot:
            got = be.get_ttl(k)
            assert got[:2] == (b"v-" + k * 4, 7) and _ttl_near(got, 5000), (k, got)
    st1 = be.stats()
    assert all(st1[f"hbm_shard_gets_{i}"] > st0[f"hbm_shard_gets_{i}"] for i in (0, 1))
    assert st1["hbm_hot_spread_gets"] > st0["hbm_hot_spread_gets"]      # replicas answered
    assert st1["hbm_touched"] - st0["hbm_touched"] == 2 * len(hot)      # both copies of each
    assert be.touch(keys[100], 6000) == 1     # a cold object: the owner only, flags kept
    got = be.get_ttl(keys[100])
    assert got[:2] == (b"v-" + keys[100] * 4, 1) and _ttl_near(got, 6000)
    assert be.touch(b"/ht/absent", 6000) == 0
    # another key that carries a stored key's digest touches nothing
    assert be.touch(b"/ht/forged", 9000, digest_of=keys[101]) == 0
    assert _ttl_near(be.get_ttl(keys[101]), 50)
    st2 = be.stats()
    assert st2["hbm_touched"] - st1["hbm_touched"] == 1       # the cold one, on its owner
    assert st2["hbm_touches"] - st0["hbm_touches"] == 2 * len(hot) + 3   # requests, per shard
    # SET, touch, SET of one key, issued back to back: the touch sees the first SET, and
    # the second SET's expiry stands
    assert be.set_touch_set(b"/ht/order", b"first", 50, 5000, b"second", 70) == 1
    got = _wait_get(be, b"/ht/order")
    deadline = time.time() + 5
    while got[0] != b"second" and time.time() < deadline:
        got = be.get(b"/ht/order")
    got = be.get_ttl(b"/ht/order")
    assert got[:2] == (b"second", 0) and _ttl_near(got, 70), got


def test_hbm_backend_touch_on_an_ejected_shard_answers_not_found():
    be = core().hbm_backend([0], 64 << 20, 1 << 14, 1 << 16, 0, flush_on_restore=False,
                            warm_restore=False)
    be.set(b"/ej/k", b"v", 0, 50)
    assert _wait_get(be, b"/ej/k") is not None
    assert be.touch(b"/ej/k", 500) == 1
    assert core().inject_shard_down(be, 0, True)
    assert be.touch(b"/ej/k", 900) == 0
    core().inject_shard_down(be, 0, False)


def test_proxy_revalidation_over_the_hbm_tier_touches_in_place():
    """The 304 scenario over --cache hbm: the stale object is extended by a touch on the
    GPU — no SET reaches the shard across the revalidation."""
    be = make_backend("hbm", gpus=[0], hbm_gb=0.25)
    o = tc.EtagOrigin().start()
    try:
        with Server([("127.0.0.1", o.port)], port=0, backend=be, ttl=1, grace=30) as px:
            c = HttpClient(port=px.port)
            assert c.get("/a").body().read() == o.body("/a", '"v1"')
            assert _wait_get(be, b"localhost/a") is not None     # the fill is asynchronous
            c.close()
            time.sleep(1.2)
            sets0 = be.stats()["cache_set_ops"]
            tc.revalidate_304_round_trip(px, o, "/a")
            st = be.stats()
            assert st["cache_set_ops"] == sets0
            assert st["hbm_touches"] == 1 and st["hbm_touched"] == 1
            assert _ttl_near(be.get_ttl(b"localhost/a"), 60 + 30)   # the 304's max-age + grace
    finally:
        o.stop()


def test_touch_beside_sets_on_a_second_stream(cuda_dev):
    """Touches on one stream while SET batches on another append to the log and lap it (FIFO,
    so the twin tells which records get overwritten): memory-safe, every object returns its
    own bytes, and each base object the SETs did not overwrite ends with either its old or
    its new expiry and flags — never anything else."""
    kw = dict(evict="fifo", nbuckets=1 << 11)
    base = pc.family_objects(1500, seed=5)
    fills = [{b"/fill/%d/%d" % (b, i): keyed(b"/fill/%d/%d" % (b, i), b"f" * 600)
              for i in range(400)} for b in range(3)]
    g, h = pc.make_shard(cuda_dev, **kw), pc.make_shard("cpu", **kw)
    for sh in (g, h):
        tc.store_at(sh, base, tc.T0 + tc.TTL0, flags=1)
    keys = sorted(base)
    d = digest_strings(keys, cuda_dev)
    kb = tc.key_tensors(keys, cuda_dev)
    ex, fl = tc.i32([tc.T0 + 500] * len(keys), cuda_dev), tc.i32([2] * len(keys), cuda_dev)
    s1, s2 = torch.cuda.Stream(cuda_dev), torch.cuda.Stream(cuda_dev)
    torch.cuda.synchronize(cuda_dev)
    with torch.cuda.stream(s2):
        tc.store_at(g, fills[0], 0, batch=400)
    with torch.cuda.stream(s1):
        hit = g.touch(d, ex, fl, kb, now=tc.T0)
    with torch.cuda.stream(s2):
        for f in fills[1:]:
            tc.store_at(g, f, 0, batch=400)
    torch.cuda.synchronize(cuda_dev)
    for f in fills:
        tc.store_at(h, f, 0, batch=400)
    assert g.head() == h.head() > g.log_bytes
    survivors = tc.live_at(h, base, tc.T0)
    assert survivors
    recs = tc.records_at(g, {**base, **fills[-1]}, tc.T0)
    for k, (v, f, e) in recs.items():
        assert v == {**base, **fills[-1]}[k], k
    assert survivors <= set(recs) and set(fills[-1]) <= set(recs)
    hit = dict(zip(keys, hit.tolist()))
    for k in survivors:
        assert recs[k][1:] == ((2, tc.T0 + 500) if hit[k] else (1, tc.T0 + tc.TTL0)), k
    for k in fills[-1]:
        assert recs[k][1:] == (0, 0), k
    assert g.counters()["touched"] == sum(hit.values())
