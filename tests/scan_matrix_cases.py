"""Scenarios shared by tests/test_scan_matrix.py (CPU) and tests/test_scan_matrix_gpu.py: the
matrix of the keyed index scans, matcher (prefix, exact key, tag list, glob) x action (list,
soften, remove), on one tiny shard whose index is 1024 slots (four tiles of the listing), for a
pattern that matches nothing, one that matches some and one that matches every live object.
The twins (HostCache on the CPU, k_keyed_scan / k_list_scan on the GPU) are each compared with
a Python model of the objects they hold. Every run takes an explicit `now`."""
import glob_cases as gc
import list_cases as lc
import purge_cases as pc
import tag_cases as tg
import touch_cases as tc
from shellac_amd.ops.cache import digest_strings, item_bytes, keyed, tagged

T0 = tc.T0
NOW = T0 + 100
NBUCKETS = 256                           # 1024 index slots
KLENS = [13, 14, 15, 29, 30, 31]         # 2 + klen on either side of a 16-B granule edge
LONG_KLENS = [60, 63, 64, 67, 70]
PER_KLEN = 48                            # 6 x 48 + 12 = 300 live objects
EVERY_TAG = b"every-tagged-object"


def key_of_len(klen, i):
    """A distinct key of exactly `klen` bytes: family /s/ or /d/, ending .js or .css."""
    fam = b"/s/" if i % 3 else b"/d/"
    end = b".js" if i % 2 else b".css"
    stem = b"%04d" % i
    k = fam + stem + b"x" * (klen - len(fam) - len(stem) - len(end)) + end
    assert len(k) == klen
    return k


def objects():
    """({key: value} live, {key: value} that have expired at NOW). Every other object carries a
    tag block; the payloads are a few bytes to a few hundred."""
    live, dead = {}, {}
    i = 0
    for klen in KLENS * PER_KLEN + LONG_KLENS * 2 + [LONG_KLENS[0], LONG_KLENS[-1]]:
        k = key_of_len(klen, i)
        payload = b"HTTP/" + bytes([65 + i % 26]) * (i * 7 % 300)
        if i % 2 == 0:
            payload = tagged([EVERY_TAG, b"grp-%d" % (i % 8 // 2)], payload)
        live[k] = keyed(k, payload)
        i += 1
    for klen in KLENS * 5:
        k = key_of_len(klen, i)
        dead[k] = keyed(k, tagged([EVERY_TAG, b"grp-1"], b"HTTP/ expired"))
        i += 1
    assert len(live) == 300 and len(dead) == 30
    return live, dead


def is_tagged(value):
    return lc.ntags_of(value) != 0


# (matcher, what it matches) -> (which live objects the shard stores, the query)
ONE = key_of_len(KLENS[0], 0)
CASES = {
    ("prefix", "none"): (None, dict(prefix=b"/q/")),
    ("prefix", "some"): (None, dict(prefix=b"/s/0")),
    ("prefix", "all"): (None, dict(prefix=b"/")),
    ("exact", "none"): (None, dict(prefix=ONE[:-1], exact=True)),
    ("exact", "some"): (None, dict(prefix=ONE, exact=True)),
    ("exact", "all"): (lambda k, v: k == ONE, dict(prefix=ONE, exact=True)),   # one live object
    ("tags", "none"): (None, dict(tags=[b"nobody", b"grp-9"])),
    ("tags", "some"): (None, dict(tags=[b"nobody", b"grp-1", b"grp-3"])),
    ("tags", "all"): (lambda k, v: is_tagged(v), dict(tags=[EVERY_TAG])),      # tagged ones only
    ("glob", "none"): (None, dict(glob=b"/s/*.php")),
    ("glob", "some"): (None, dict(glob=b"/*0*.js")),
    ("glob", "all"): (None, dict(glob=b"/*/*.*s")),
}


def model_matches(value, prefix=None, exact=False, tags=None, glob=None):
    if glob is not None:
        return gc.value_matches(glob, value)
    return lc.value_listed(value, prefix=prefix, tags=tags, exact=exact)


def equalise(shards, objs):
    """The keys live at NOW on every shard; a key only some hold (an insert into a full bucket
    pair evicts, and which entry depends on the order of inserts) is DELETEd."""
    lives = [set(tg.live_values(sh, objs, now=NOW)) for sh in shards]
    common = set.intersection(*lives)
    assert len(common) >= 0.98 * max(len(l) for l in lives)
    for sh, live in zip(shards, lives):
        extra = sorted(live - common)
        if extra:
            assert sh.remove(digest_strings(extra, sh.device), now=NOW).all()
    return common


def listed_all(sh):
    r = sh.list_keyed(limit=lc.MAX_ROWS, key_cap=1024, now=NOW)
    lc.assert_slot_order(r["rows"], 4 * sh.nbuckets)
    assert r["matched"] == len(r["rows"]) and r["next"] is None
    return lc.listed_keys(r["rows"])


def run_case(devices, matcher, kind):
    keep, query = CASES[(matcher, kind)]
    live_objs, dead_objs = objects()
    if keep is not None:
        live_objs = {k: v for k, v in live_objs.items() if keep(k, v)}
    objs = {**live_objs, **dead_objs}
    shards = [pc.make_shard(d, nbuckets=NBUCKETS) for d in devices]
    for sh in shards:
        tc.store_at(sh, dict(list(live_objs.items())[0::2]), 0)            # never expire
        tc.store_at(sh, dict(list(live_objs.items())[1::2]), T0 + 1000)
        tc.store_at(sh, dead_objs, T0 + 50)
    live = equalise(shards, objs)
    assert live <= set(live_objs) and len(live) >= 0.98 * len(live_objs)
    want = {k for k in live if model_matches(objs[k], **query)}
    want_bytes = sum(item_bytes(len(objs[k])) for k in want)
    assert {"none": not want, "some": 0 < len(want) < len(live), "all": want == live}[kind], \
        (matcher, kind, len(want), len(live))
    for sh in shards:
        purged0 = sh.counters()["purged"]
        assert listed_all(sh) == live, sh.device
        r = sh.list_keyed(limit=0, now=NOW, **query)
        assert (r["matched"], r["bytes"]) == (len(want), want_bytes), (sh.device, matcher, kind, r)
        if matcher in ("prefix", "exact"):
            n = sh.soften_keyed_prefix(query["prefix"], 77, exact=query.get("exact", False),
                                       now=NOW)
        elif matcher == "tags":
            n = sh.soften_keyed_tags(query["tags"], 77, now=NOW)
        else:
            n = sh.soften_keyed_glob(query["glob"], 77, now=NOW)
        assert n == len(want), (sh.device, matcher, kind, n, len(want))
        assert sh.counters()["purged"] == purged0, "a soft purge counts nothing as purged"
        survivors = live
        if matcher != "exact":           # (the hard purge has no exact form)
            if matcher == "prefix":
                got = sh.remove_keyed_prefix(query["prefix"], now=NOW)
            elif matcher == "tags":
                got = sh.remove_keyed_tags(query["tags"], now=NOW)
            else:
                got = sh.remove_keyed_glob(query["glob"], now=NOW)
            assert got == (len(want), want_bytes), (sh.device, matcher, kind, got)
            survivors = live - want
            assert sh.counters()["purged"] - purged0 == len(want)
        assert listed_all(sh) == survivors, (sh.device, matcher, kind)
        after = tg.live_values(sh, objs, now=NOW)
        assert after == {k: objs[k] for k in survivors}, (sh.device, matcher, kind)
