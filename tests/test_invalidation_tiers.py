"""The invalidation request through every host tier: the matrix of tests/scan_matrix_cases.py
(matcher x a pattern that matches none, some or all) as a count-only listing, a soft purge and
a removal, through DramBackend, TieredBackend(Dram, Dram), FaultBackend(Dram) and the memcached
tier, each compared with the Python model of the objects stored.

The tiers take relative TTLs from a clock of their own, so an object cannot be stored already
expired without waiting for it: the matrix' 300 live objects are stored here, and its expired
ones go through the same walk where a clock can be passed, ObjectCache's in
tests/native/selector_main.cc. TieredBackend and FaultBackend are so not shown here passing
over an expired object; both hand the request to DramBackend, whose ObjectCache does."""
import pytest

import scan_matrix_cases as sm
from shellac_amd import core
from shellac_amd.utils.fakemc import FakeMemcached

FLAGS, STALE = 3, 77
TIERS = ["dram", "tiered", "fault", "memcached"]


@pytest.fixture(scope="module")
def live_objects():
    return sm.objects()[0]


@pytest.fixture(scope="module")
def memcached():
    f = FakeMemcached().start()
    yield f
    f.stop()


def _tier(kind, memcached):
    """(the tier, stored copies per object; 0: the tier cannot scan)."""
    c = core()
    dram = lambda: c.dram_backend(8 << 20, 1 << 20)
    if kind == "dram":
        return dram(), 1
    if kind == "tiered":
        return c.tiered_backend(dram(), dram()), 2         # writes go to both levels
    if kind == "fault":
        return c.fault_backend(dram(), ""), 1
    be = c.memcached_backend("127.0.0.1:%d" % memcached.port)
    be.flush()
    return be, 0


def _api(be, matcher, query):
    """(list, soften, remove) of the matcher as calls on the Python handle; remove is None for
    the exact matcher (the hard purge of one key is a delete)."""
    if matcher in ("prefix", "exact"):
        p, exact = query["prefix"], query.get("exact", False)
        return (lambda: be.list_objects(**({"key": p} if exact else {"prefix": p}), limit=0),
                lambda: be.soften_prefix(p, STALE, exact=exact),
                None if exact else lambda: be.purge_prefix(p))
    if matcher == "tags":
        return (lambda: be.list_objects(tags=query["tags"], limit=0),
                lambda: be.soften_tags(query["tags"], STALE),
                lambda: be.purge_tags(query["tags"]))
    return (lambda: be.list_objects(glob=query["glob"], limit=0),
            lambda: be.soften_glob(query["glob"], STALE),
            lambda: be.purge_glob(query["glob"]))


@pytest.mark.parametrize("tier", TIERS)
@pytest.mark.parametrize("matcher,kind", sorted(sm.CASES))
def test_list_soften_and_remove_match_the_model(live_objects, memcached, tier, matcher, kind):
    keep, query = sm.CASES[(matcher, kind)]
    objs = {k: v for k, v in live_objects.items() if keep is None or keep(k, v)}
    payload = {k: v[2 + len(k):] for k, v in objs.items()}
    be, copies = _tier(tier, memcached)
    for i, (k, p) in enumerate(payload.items()):
        be.set(k, p, FLAGS, 0 if i % 2 == 0 else 1000)
    want = {k for k, v in objs.items() if sm.model_matches(v, **query)}
    assert {"none": not want, "some": 0 < len(want) < len(objs), "all": want == set(objs)}[kind]
    lister, soften, remove = _api(be, matcher, query)
    if not copies:                                   # memcached: "cannot", and nothing changes
        assert lister() is None and soften() == -1 and (remove is None or remove() == -1)
        assert all(be.get(k) == (payload[k], FLAGS) for k in objs)
        return
    r = lister()                                     # (a tiered listing is L2's: one copy each)
    assert (r["matched"], r["bytes"]) == (len(want), sum(len(objs[k]) for k in want))
    assert r["objects"] == [] and r["next"] is None
    assert soften() == copies * len(want)
    for k in objs:
        assert be.get(k) == (payload[k], STALE if k in want else FLAGS), k
    survivors = set(objs)
    if remove is not None:
        assert remove() == copies * len(want)
        survivors -= want
        assert remove() == 0
    for k in objs:
        assert be.get(k) == ((payload[k], STALE if k in want else FLAGS)
                             if k in survivors else None), k
    assert lister()["matched"] == len(want & survivors)


def test_a_glob_beside_another_selector_is_refused():
    """The handle's list_objects takes one selector: a glob given with a prefix, a key or tags
    answers None, as a refused query does, and lists nothing by either."""
    be, _ = _tier("dram", None)
    be.set(b"/a/1.css", b"HTTP/ a", FLAGS, 0)
    assert be.list_objects(glob=b"*.css")["matched"] == 1
    assert be.list_objects(prefix=b"/a/")["matched"] == 1
    assert be.list_objects(glob=b"*.css", prefix=b"/a/") is None
    assert be.list_objects(glob=b"*.css", key=b"/a/1.css") is None
    assert be.list_objects(glob=b"*.css", tags=[b"t"]) is None


# ------------------------------------------------------------------- host code, sanitized
def test_selector_host_code_under_sanitizers(tmp_path):
    """tests/native/selector_main.cc (its own main): the selector's factories, matcher,
    device images and fills-in-flight rules, ObjectCache's one walk as a removal, a soft purge
    and a listing (expired objects among them, under an explicit clock) and a TieredBackend
    purge with a promotion straddling it, built with ASan and UBSan, as test_glob_purge.py
    runs glob_main.cc."""
    import os
    import shutil
    import subprocess
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++ on this machine")
    here = os.path.dirname(__file__)
    csrc = os.path.join(here, "..", "shellac_amd", "csrc")
    exe = str(tmp_path / "selector_main")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    # the toolchain is probed first, with a program of one line: only a toolchain that cannot
    # link the sanitizers' runtimes skips; the real build below must then succeed
    probe = tmp_path / "probe.cc"
    probe.write_text("int main() { return 0; }\n")
    pb = subprocess.run([gxx, *san, str(probe), "-o", str(tmp_path / "probe")],
                        capture_output=True, text=True)
    if pb.returncode != 0:
        pytest.skip("the toolchain cannot link the sanitizers: " + pb.stderr.strip()[-200:])
    cmd = [gxx, "-std=c++17", "-O1", "-g", *san, "-I", csrc,
           os.path.join(here, "native", "selector_main.cc"),
           *(os.path.join(csrc, f) for f in ("object_cache.cc", "backend.cc", "ketama.cc")),
           "-o", exe, "-lpthread"]
    b = subprocess.run(cmd, capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    assert "selector_main: ok" in r.stdout
