"""Scenarios shared by tests/test_soft_purge.py (CPU) and tests/test_soft_purge_gpu.py: a
Python model of a soft purge, helpers that read flags and header expiries back, and the runs
both twins (HostCache on the CPU, k_keyed_scan<PrefixMatch, SoftenAction> on the GPU) are checked with. Every run
takes explicit `now` values, so nothing here waits for a clock."""
import json

import purge_cases as pc
import touch_cases as tc
from shellac_amd.ops.cache import digest_strings, keyed

T0, TTL0, NOWS = tc.T0, tc.TTL0, tc.NOWS
STALE_AT = 0x5EEDF00D          # the freshness time a soft purge writes (any 32-bit word)
EXPIRIES = [0, T0 + 50, T0 + TTL0, T0 + 500]     # never, and three lives
# expiry caps: none, below some of EXPIRIES, above all of them (caps "never" only)
CAPS = [0, T0 + 80, T0 + 10 ** 6]


def matches(key, pattern, exact):
    return key == pattern if exact else key.startswith(pattern)


def model_soften(model, pattern, exact, stale_at, expire_cap, now):
    """{key: (expire, flags)} -> (count, model'): every key live at `now` that matches gets
    flags = stale_at and, where the cap is non-zero and the key never expires or expires
    after it, expire = cap. The count is the live matches, changed or not."""
    out, n = dict(model), 0
    for k, (e, _) in model.items():
        if (e and e <= now) or not matches(k, pattern, exact):
            continue
        n += 1
        if expire_cap and (e == 0 or e > expire_cap):
            e = expire_cap
        out[k] = (e, stale_at)
    return n, out


def store_mixed(sh, objs, flags=1):
    """Store `objs` at T0, the i-th key with expiry EXPIRIES[i % 4]."""
    keys = list(objs)
    for j, e in enumerate(EXPIRIES):
        tc.store_at(sh, {k: objs[k] for k in keys[j::len(EXPIRIES)]}, e, flags=flags)


def model_of(sh, objs, now=T0):
    """{key: (header expire, flags)} of the keys of `objs` that hit at `now`."""
    return {k: (e, f) for k, (_, f, e) in tc.records_at(sh, objs, now).items()}


def snapshot(sh, objs):
    """{now: {key: (value, flags, header expire)}} at each of NOWS: value, flags, expiry and
    liveness of every object."""
    return {t: tc.records_at(sh, objs, t) for t in NOWS}


def want_snapshot(objs, model):
    return {t: {k: (objs[k], model[k][1], model[k][0]) for k in tc.model_live(model, t)}
            for t in NOWS}


def check_soften(shards, objs, model, pattern, exact, expire_cap, stale_at=STALE_AT, now=T0,
                 chain=None):
    """Soften `pattern` on every shard of `shards` (they hold the same live set, `model`):
    the count is the model's, twice in a row; afterwards flags, header expiry and liveness
    at NOWS are the model's for every object, and the objects that do not match are
    bit-identical to what they were. Returns (count, model'). `chain` (a list, empty at
    first) carries the snapshots from one call to the next over the same shards."""
    before = chain[:] if chain else [snapshot(sh, objs) for sh in shards]
    if chain is not None:
        del chain[:]
    want_n, model2 = model_soften(model, pattern, exact, stale_at, expire_cap, now)
    want = want_snapshot(objs, model2)
    for sh, was in zip(shards, before):
        for _ in range(2):
            got = sh.soften_keyed_prefix(pattern, stale_at, expire_cap, exact=exact, now=now)
            assert got == want_n, (sh.device, pattern, exact, expire_cap, got, want_n)
        after = snapshot(sh, objs)
        if chain is not None:
            chain.append(after)
        assert after == want, (sh.device, pattern, exact, expire_cap)
        for t in NOWS:
            for k, rec in was[t].items():
                if not matches(k, pattern, exact):
                    assert after[t].get(k) == rec, (sh.device, t, k)
    return want_n, model2


def equalise(g, h, objs, now=T0):
    """test_purge_gpu._check_twins' equalisation: at a high index load an insert now and then
    evicts a live entry, and which one depends on the order the GPU's lanes insert in. The
    keys only one twin holds are DELETEd; returns the common model."""
    mg, mh = model_of(g, objs, now), model_of(h, objs, now)
    common = set(mg) & set(mh)
    assert len(common) >= 0.99 * max(len(mg), len(mh))
    for sh, m in ((g, mg), (h, mh)):
        extra = sorted(set(m) - common)
        if extra:
            assert sh.remove(digest_strings(extra, sh.device), now=now).all()
    assert {k: mg[k] for k in common} == {k: mh[k] for k in common}
    return {k: mh[k] for k in common}


def exact_boundary_objects(plen):
    """pc.boundary_objects(plen) plus the near misses of the pattern itself (one byte longer,
    one byte shorter, last / first byte differing): an exact soft purge matches the key that
    equals the pattern and nothing else."""
    pat, objs, must_prefix = pc.boundary_objects(plen)
    for k in tc.near_miss_keys(pat):
        if k and k not in objs:
            objs[k] = keyed(k, b"near miss")
    return pat, objs, must_prefix


def clock_keeps_the_softening(sh):
    """tc.clock_keeps_the_touch for a soft purge: objects that were read (reference bit set)
    are softened with a cap below their expiry, then SET batches lap the log, so the CLOCK
    hand re-appends them from their record headers: they come back with the softened flags
    and the capped expiry. Returns ({key: (flags, header expire)} just before the cap, the
    live set at the cap, reinsertions)."""
    assert sh.evict == "clock"
    hot = {b"/hot/%d" % i: keyed(b"/hot/%d" % i, b"h" * 900) for i in range(20)}
    tc.store_at(sh, hot, T0 + 1000, flags=1)
    for _ in range(2):
        assert tc.live_at(sh, hot, T0) == set(hot)               # reference bits set
    cap = T0 + TTL0
    assert sh.soften_keyed_prefix(b"/hot/", STALE_AT, cap, now=T0) == 20
    head0 = sh.head()
    batch_no = 0
    while sh.head() < head0 + sh.log_bytes + (sh.log_bytes >> 2):
        fill = {b"/fill/%d/%d" % (batch_no, i): keyed(b"/fill/%d/%d" % (batch_no, i), b"f" * 700)
                for i in range(200)}
        tc.store_at(sh, fill, 0, batch=200)
        batch_no += 1
    recs = tc.records_at(sh, hot, cap - 1)
    for k, (v, _, _) in recs.items():
        assert v == hot[k]
    return ({k: (f, e) for k, (_, f, e) in recs.items()}, tc.live_at(sh, hot, cap),
            sh.counters()["reinserted"])


# ---- the proxy's PURGE method with X-Purge-Soft
def soft_purge(c, path, prefix=False, soft=True):
    headers = {}
    if prefix:
        headers["X-Purge-Mode"] = "prefix"
    if soft:
        headers["X-Purge-Soft"] = "1"
    r = c.get(path, method="PURGE", headers=headers or None)
    body = r.body().read()
    return r.status(), (json.loads(body) if r.status() == 200 else body)


def soft_purge_304_round_trip(px, origin, path, settle=lambda: None):
    """`path` is fetched through `px` (grace on, a long TTL: it is fresh), then soft-purged by
    prefix: the next GET is answered from the cache at once (stale_served + 1) while exactly
    one conditional request reaches the origin; its 304 touches the object in place and the
    GET after that is fresh again (no origin request)."""
    from shellac_amd.utils.httpclient import HttpClient
    origin.cc304[path] = "max-age=60"
    c = HttpClient(port=px.port)
    assert c.get(path).body().read() == origin.body(path, '"v1"')
    settle()
    assert c.get(path).body().read() == origin.body(path, '"v1"')     # fresh: a plain hit
    assert origin.seen(path) == [(path, None, 200)]
    st0 = px.stats()
    assert st0["stale_served"] == 0
    status, body = soft_purge(c, path[:path.rindex("/") + 1], prefix=True)
    assert status == 200 and body["mode"] == "prefix" and body["soft"] is True
    assert body["softened"] >= 1
    assert c.get(path).body().read() == origin.body(path, '"v1"')     # stale, at once
    log = origin.wait_seen(path, 2)
    assert log[1:] == [(path, '"v1"', 304)], log
    assert tc.wait_stat(px, "revalidate_touched", 1) == 1
    assert c.get(path).body().read() == origin.body(path, '"v1"')     # fresh again
    st1 = px.stats()
    assert {k: st1[k] - st0[k] for k in tc.GRACE_COUNTERS} == {
        "stale_served": 1, "revalidations": 1, "revalidated_304": 1, "revalidate_touched": 1,
        "revalidate_restored": 0, "revalidate_errors": 0}
    assert origin.seen(path) == log
    assert st1["soft_purge_requests"] == 1 and st1["softened_objects"] == body["softened"]
    c.close()
    return body
