"""Purge, soft purge and listing by URL glob on the CPU: the host matcher against the regex
model, HostCache's glob walks (the semantic reference of k_keyed_scan<GlobMatch, RemoveAction> / k_keyed_scan<GlobMatch, SoftenAction> /
k_list_scan<GlobMatch>) over the scenarios of tests/glob_cases.py, the DRAM, tiered and
memcached tiers, the proxy's PURGE with X-Purge-Mode: glob and /_shellac/objects?glob= over
DRAM, and the host-only code under sanitizers."""
import itertools
import os
import shutil
import subprocess
import threading

import pytest

import glob_cases as gc
import list_cases as lc
import purge_cases as pc
import soften_cases as sc
import tag_cases as tg
import touch_cases as tc
from shellac_amd import core
from shellac_amd.server.proxy import Server, make_backend
from shellac_amd.utils.fakemc import FakeMemcached
from shellac_amd.utils.httpclient import HttpClient
from shellac_amd.utils.origin import Origin

CPU = ["cpu"]


# ------------------------------------------------------------------------------- matcher
def test_host_matcher_against_the_regex_exhaustively():
    """Every pattern of up to 6 bytes from {a, b, *} against every key of up to 8 bytes from
    {a, b}: 558,523 pairs with the empty and the stars-only patterns (both sides refuse them)."""
    match = core().glob_match
    keys = [bytes(k) for n in range(9) for k in itertools.product(b"ab", repeat=n)]
    pairs = refused = 0
    for n in range(7):
        for p in itertools.product(b"ab*", repeat=n):
            p = bytes(p)
            pairs += len(keys)
            if not p.strip(b"*"):
                refused += 1
                with pytest.raises(ValueError):
                    match(p, b"a")
                with pytest.raises(ValueError):
                    gc.regex(p)
                continue
            rx = gc.regex(p)
            for k in keys:
                assert match(p, k) == (bool(k) and rx.fullmatch(k) is not None), (p, k)
    assert pairs == 558523 and refused == 7


def test_host_matcher_subject_ends_at_the_first_separator_and_escapes():
    match = core().glob_match
    for p, k, yes in gc.OVERLAPS:
        assert match(p, k) is yes, (p, k)
    k = b"/a.css" + gc.SEP + b"gzip"
    assert match(b"*.css", k) and match(b"/a.css", k) and not match(b"*gzip", k)
    assert not match(b"*.css*gzip", k) and not match(b"*" + gc.SEP + b"*", k)
    assert match(b"*.css", b"/a.css" + gc.SEP + b"x" + gc.SEP + b"y")
    assert not match(b"a*", b"") and not match(b"a*", gc.SEP + b"a")
    for bad in gc.REFUSED:
        with pytest.raises(ValueError):
            match(bad, b"a")
    img = core().keyed_glob_image(b"/img/*/thumb_*.jpg")
    assert len(img) % 16 == 0 and 128 < len(img) <= 128 + 1024
    assert len(core().keyed_glob_image(b"a" * 1024)) == 128 + 1024
    assert core().MAX_GLOB_STARS == 8 and core().MAX_GLOB_LITERAL == 1024 and core().LIST_GLOB == 3


# ---------------------------------------------------------------------- HostCache's walks
def test_host_families_match_the_model():
    gc.run_families(CPU)


@pytest.mark.parametrize("seglen", pc.BOUNDARY_PLENS)
def test_host_segments_at_granule_boundaries(seglen):
    gc.run_boundaries(CPU, seglen)


def test_host_match_is_bounded_by_klen():
    gc.run_bounded_by_klen(CPU)


def test_host_overlaps_and_order():
    gc.run_overlaps(CPU)


def test_host_variants_go_with_their_base_key():
    gc.run_variants(CPU)


def test_host_long_keys():
    gc.run_long_keys(CPU)


def test_host_random_sweep():
    gc.run_random_sweep(CPU)


def test_host_garbage_values():
    gc.run_garbage(CPU)


def test_host_refused_patterns():
    gc.run_refused(CPU)


def test_host_expired_and_dead_entries_are_not_counted():
    gc.run_expired_are_not_counted(CPU)
    gc.run_dead_entries(CPU)


def test_host_after_the_log_lapped():
    gc.run_after_the_log_lapped(CPU)


def test_host_soft_form_over_expiries_and_caps():
    gc.run_soft_form(CPU)


def test_host_reference_bit_survives_a_glob_softening():
    gc.run_reference_bit(CPU)


def test_host_listing_rows_pages_and_the_purge_that_follows():
    gc.run_listing(CPU)


# -------------------------------------------------------------------------------- backends
def _ttl_near(got, want):
    return got is not None and want - 2 <= got[2] <= want


@pytest.mark.parametrize("kind", ["dram", "fault"])
def test_dram_backend_purges_softens_and_lists_by_glob(kind):
    be = make_backend("dram", dram_mb=16, **({"fault": ""} if kind == "fault" else {}))
    objs = gc.run_backend_glob(be)
    be = make_backend("dram", dram_mb=16)
    for k, v in objs.items():
        be.set(k, v, 3, 500)
    be.set(b"localhost/i/b/never", b"HTTP/ never", 3, 0)
    assert be.soften_glob(b"*/i/b/*", 1234, keep_s=100) == 5
    for k in [k for k in objs if k.startswith(b"localhost/i/b/")] + [b"localhost/i/b/never"]:
        got = be.get_ttl(k)
        assert got[1] == 1234 and _ttl_near(got, 100), (k, got)
    for k in [k for k in objs if not k.startswith(b"localhost/i/b/")]:
        got = be.get_ttl(k)
        assert got[:2] == (objs[k], 3) and _ttl_near(got, 500), (k, got)
    assert be.touch(b"localhost/i/b/1", 400, flags=4321) == 1           # fresh again
    assert be.get_ttl(b"localhost/i/b/1")[1] == 4321


def test_tiered_backend_purges_and_softens_both_levels():
    c = core()
    l1, l2 = c.dram_backend(8 << 20, 1 << 20), c.dram_backend(8 << 20, 1 << 20)
    be = c.tiered_backend(l1, l2)
    for i in range(10):
        be.set(b"/a/%d.css" % i, b"a%d" % i, 3, 500)          # writes go to both levels
        be.set(b"/b/%d.js" % i, b"b%d" % i, 3, 500)
    l2.set(b"/a/only-l2.css", b"deep", 3, 500)
    assert be.list_objects(glob=b"*.css")["matched"] == 11    # (the listing is L2's)
    assert be.soften_glob(b"*.css", 1234, keep_s=100) == 2 * 10 + 1
    for tier in (l1, l2):
        for i in range(10):
            got = tier.get_ttl(b"/a/%d.css" % i)
            assert got[:2] == (b"a%d" % i, 1234) and _ttl_near(got, 100)
            assert tier.get_ttl(b"/b/%d.js" % i)[1] == 3
    assert be.get(b"/a/only-l2.css") == (b"deep", 1234)        # promoted stale
    assert be.purge_glob(b"/a/*") == 2 * 11
    assert l1.get(b"/a/3.css") is None and l2.get(b"/a/3.css") is None
    assert be.get(b"/a/only-l2.css") is None and be.get(b"/b/3.js") == (b"b3", 3)
    assert be.purge_glob(b"*") == -1 and be.soften_glob(b"", 5) == -1
    assert be.stats()["tier_purges"] >= 2


def test_memcached_tier_answers_minus_one():
    f = FakeMemcached().start()
    try:
        mc = make_backend("memcached", caches=[("127.0.0.1", f.port)])
        mc.set(b"/m/1.css", b"v", 3, 50)
        assert mc.purge_glob(b"*.css") == -1 and mc.soften_glob(b"*.css", 8, keep_s=10) == -1
        assert mc.list_objects(glob=b"*.css") is None
        tiered = make_backend("memcached", caches=[("127.0.0.1", f.port)], l1_mb=8)
        assert tiered.purge_glob(b"*.css") == -1 and tiered.soften_glob(b"*.css", 8) == -1
    finally:
        f.stop()


# ---------------------------------------------------------------------------------- proxy
@pytest.fixture
def origin():
    o = tg.TagOrigin().start()
    yield o
    o.stop()


def _proxy(origin_port, backend=None, **kw):
    kw.setdefault("purge", "loopback")
    kw.setdefault("inspect", "loopback")
    if backend is None:
        backend = make_backend("dram", dram_mb=16)
    return Server([("127.0.0.1", origin_port)], port=0, backend=backend, **kw).start()


def test_proxy_purge_by_glob_dry_run_and_inspection(origin):
    with _proxy(origin.port, threads=2) as px:
        gc.proxy_glob_round_trip(px, origin)
        c = HttpClient(port=px.port)
        assert '"purge_glob_requests":5' in c.get("/_shellac/stats").body().read().decode()
        text = c.get("/_shellac/metrics").body().read().decode()
        assert "shellac_purge_glob_requests 5" in text and "shellac_purged_objects 10" in text
        c.close()


def test_soft_glob_purge_with_grace_serves_stale_then_revalidates(origin):
    be = make_backend("dram", dram_mb=16)
    with _proxy(origin.port, backend=be, ttl=60, grace=30) as px:
        gc.soft_glob_304_round_trip(px, be, origin)


def test_fill_fetched_before_a_glob_purge_is_delivered_but_not_stored(origin):
    origin.vary["/slow/v.css"] = "X-Lang"
    for p in ("/slow/a.css", "/slow/v.css", "/slow/other.js"):
        origin.delays[p] = 0.4
    be = make_backend("dram", dram_mb=16)
    with _proxy(origin.port, backend=be, threads=2) as px:
        got = {}

        def get(p):
            got[p] = HttpClient(port=px.port).get(p, headers={"X-Lang": "de"}).body().read()
        ths = [threading.Thread(target=get, args=(p,)) for p in origin.delays]
        for th in ths:
            th.start()
        for p in origin.delays:
            assert origin.wait_seen(p, 1)
        c = HttpClient(port=px.port)
        assert gc.glob_purge(c, "/slow/*.css") == (200, {"mode": "glob", "purged": 0})
        for th in ths:
            th.join()
        assert got == {p: origin.body(p) for p in origin.delays}        # delivered
        assert px.stats()["fills_not_cached_purged"] == 2               # a.css and v.css's variant
        assert be.get(b"localhost/slow/a.css") is None and be.get(b"localhost/slow/v.css") is None
        assert be.list_objects(glob=b"*/slow/*")["matched"] == 1
        assert be.get(b"localhost/slow/other.js") is not None
        c.close()


def test_glob_purge_refusals(origin):
    with _proxy(origin.port) as px:
        c = HttpClient(port=px.port)
        ip = lc.non_loopback_address()
        if ip is not None:
            try:
                ext = HttpClient(host=ip, port=px.port, timeout=3)
            except OSError:
                ext = None
            if ext is not None:
                assert gc.glob_purge(ext, "/x/*")[0] == 403
                assert gc.glob_purge(ext, "/x/*", dry=True)[0] == 403
                assert px.stats()["purge_denied"] == 2
        c.close()
    f = FakeMemcached().start()
    try:
        mc = make_backend("memcached", caches=[("127.0.0.1", f.port)])
        with _proxy(origin.port, backend=mc, grace=30) as px:
            c = HttpClient(port=px.port)
            assert gc.glob_purge(c, "/a/*")[0] == 501
            assert gc.glob_purge(c, "/a/*", soft=True)[0] == 501         # as the prefix form
            assert gc.glob_purge(c, "/a/*", dry=True)[0] == 501
            assert lc.inspect(c, "?glob=*/a/*")[0] == 501
            c.close()
    finally:
        f.stop()


def test_requests_in_prefix_mode_answer_as_before():
    """purge_cases' round trip, byte for byte."""
    o = Origin(body_bytes=200).start()
    try:
        be = make_backend("dram", dram_mb=16)
        with Server([("127.0.0.1", o.port)], port=0, backend=be, purge="loopback",
                    inspect="loopback") as px:
            pc.prefix_purge_round_trip(px, o)
            assert px.stats()["purge_glob_requests"] == 0
    finally:
        o.stop()


# ------------------------------------------------------------------- host code, sanitized
def test_glob_host_code_under_sanitizers(tmp_path):
    """tests/native/glob_main.cc (its own main): the pattern compiler on every refused form,
    the matcher on the overlap table and at the key lengths' ends, values whose klen points
    past their end, inspect.h's glob selector and HostCache's purge, soften and list by glob,
    built with ASan and UBSan, as test_list.py runs list_main.cc."""
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++ on this machine")
    here = os.path.dirname(__file__)
    csrc = os.path.join(here, "..", "shellac_amd", "csrc")
    exe = str(tmp_path / "glob_main")
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
           os.path.join(here, "native", "glob_main.cc"), os.path.join(csrc, "host_cache.cc"),
           "-o", exe, "-lpthread"]
    b = subprocess.run(cmd, capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    assert "glob_main: ok" in r.stdout
