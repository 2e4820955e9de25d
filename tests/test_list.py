"""Listing on the CPU: HostCache::list_keyed (the semantic reference of k_list_scan /
k_list_emit) against the Python model of tests/list_cases.py, the DRAM, tiered and memcached
tiers' list_objects, the proxy's GET /_shellac/objects and PURGE dry run over DRAM, and the
host-only helpers under sanitizers."""
import os
import shutil
import subprocess

import pytest

import list_cases as lc
import purge_cases as pc
import tag_cases as tg
from shellac_amd import core
from shellac_amd.server.proxy import Server, build_arg_parser, make_backend
from shellac_amd.utils.fakemc import FakeMemcached
from shellac_amd.utils.httpclient import HttpClient
from shellac_amd.utils.origin import Origin

CPU = ["cpu"]


# ------------------------------------------------------------------------------- matcher
def test_boundary_patterns_prefix_exact_and_all():
    lc.run_boundary_patterns(CPU)


def test_garbage_values_are_never_listed():
    lc.run_garbage(CPU)


def test_expired_entries_are_not_listed_or_counted():
    lc.run_expired(CPU)


def test_dead_same_digest_entry_and_locked_slot_are_not_listed():
    lc.run_dead_entries(CPU)


def test_tag_mode_block_forms_alignment_near_misses_and_refused_arguments():
    lc.run_tag_forms(CPU)


# ---------------------------------------------------------------------------------- rows
def test_rows_say_what_was_stored():
    lc.run_rows_say_what_was_stored(CPU)


def test_reference_bit_after_a_get_and_after_the_clock_hand():
    lc.run_reference_bit(CPU)


def test_key_cap_truncation_edge_and_granule_edges():
    lc.run_key_cap_edges(CPU)


# ---------------------------------------------------------------------- limit and paging
def test_limits_and_start_slots_over_a_sparse_index():
    lc.run_limits_and_starts(CPU)


def test_pages_concatenate_to_the_one_call_listing():
    lc.run_paging(CPU)


# --------------------------------------------------------------------------------- state
def test_after_the_log_lapped():
    lc.run_after_the_log_lapped(CPU)


def test_list_then_purge_removes_what_was_counted_and_changes_nothing_itself():
    lc.run_purges_and_lists_agree(CPU)


def test_soft_purged_objects_list_with_their_new_words():
    lc.run_soft_purged_objects(CPU)


def test_list_while_a_phase1_batch_is_pending():
    lc.run_while_phase1_pending(CPU)


# ------------------------------------------------------------------------------- backends
@pytest.mark.parametrize("kind", ["dram", "fault"])
def test_dram_backend_lists_sorted_by_key(kind):
    be = make_backend("dram", dram_mb=16, **({"fault": ""} if kind == "fault" else {}))
    lc.run_backend_listing(be)
    be = make_backend("dram", dram_mb=16)
    for k, v in lc.backend_objects().items():
        be.set(k, v, 0, 50)
    r = be.list_objects(limit=5)
    keys = [o["key"] for o in r["objects"]]
    assert keys == sorted(lc.backend_objects())[:5] and r["next"] == keys[-1]   # "after this key"
    assert all(48 <= o["ttl"] <= 50 for o in r["objects"])
    assert be.get(keys[0]) is not None
    assert [o["referenced"] for o in be.list_objects(key=keys[0])["objects"]] == [True]


def test_memcached_tier_cannot_list_and_the_tiered_backend_answers_from_l2():
    f = FakeMemcached().start()
    try:
        mc = make_backend("memcached", caches=[("127.0.0.1", f.port)])
        mc.set(b"/m/1", b"v", 3, 50)
        assert mc.list_objects() is None and mc.list_objects(prefix=b"/m/", limit=0) is None
        assert make_backend("memcached", caches=[("127.0.0.1", f.port)], l1_mb=8).list_objects() is None
    finally:
        f.stop()
    c = core()
    l1, l2 = c.dram_backend(8 << 20, 1 << 20), c.dram_backend(8 << 20, 1 << 20)
    be = c.tiered_backend(l1, l2)
    for i in range(10):
        be.set(b"/a/%d" % i, b"a%d" % i, 3, 500)        # writes go to both levels
    l2.set(b"/a/only-l2", b"deep", 3, 500)
    l1.set(b"/a/only-l1", b"shallow", 3, 500)
    r = be.list_objects(prefix=b"/a/")
    assert r["matched"] == 11 and b"/a/only-l2" in {o["key"] for o in r["objects"]}


# ---------------------------------------------------------------------------------- proxy
@pytest.fixture
def origin():
    o = tg.TagOrigin().start()
    yield o
    o.stop()


def _proxy(origin_port, backend, **kw):
    kw.setdefault("purge", "loopback")
    kw.setdefault("inspect", "loopback")
    kw.setdefault("tag_header", tg.TAG_HEADER)
    return Server([("127.0.0.1", origin_port)], port=0, backend=backend, **kw).start()


def test_proxy_inspect_and_dry_run_over_dram(origin):
    be = make_backend("dram", dram_mb=16)
    with _proxy(origin.port, be, threads=2) as px:
        lc.proxy_inspect_round_trip(px, be, origin)
        text = HttpClient(port=px.port).get("/_shellac/metrics").body().read().decode()
        assert "shellac_purge_dry_runs 6" in text and "shellac_inspect_requests" in text


def test_inspect_off_forwards_the_url_upstream(origin):
    be = make_backend("dram", dram_mb=16)
    with _proxy(origin.port, be, inspect="off") as px:
        c = HttpClient(port=px.port)
        r = c.get("/_shellac/objects?prefix=x")
        assert r.status() == 200 and r.body().read() == origin.body("/_shellac/objects?prefix=x")
        assert origin.seen("/_shellac/objects?prefix=x") and px.stats()["inspect_requests"] == 0
        c.close()


def test_ttl_and_fresh_for_with_grace(origin):
    be = make_backend("dram", dram_mb=16)
    with _proxy(origin.port, be, grace=30, ttl=100) as px:
        c = HttpClient(port=px.port)
        assert c.get("/g/1").status() == 200
        (o,) = lc.inspect(c, "?key=localhost/g/1")[1]["objects"]
        assert 125 <= o["ttl"] <= 130          # the object lives ttl + grace
        assert 95 <= o["fresh_for"] <= 100     # and is fresh for ttl
        c.close()


def test_inspect_refusals(origin):
    be = make_backend("dram", dram_mb=16)
    with _proxy(origin.port, be, tag_header="") as px:               # no --tag-header
        c = HttpClient(port=px.port)
        assert lc.inspect(c, "?tag=x")[0] == 400
        assert lc.dry_run(c, "/x", "tag", "x")[0] == 400
        ip = lc.non_loopback_address()
        if ip is not None:
            try:
                ext = HttpClient(host=ip, port=px.port, timeout=3)
            except OSError:
                ext = None
            if ext is not None:
                assert lc.inspect(ext)[0] == 403
                assert lc.dry_run(ext, "/x", "prefix")[0] == 403
        c.close()
    f = FakeMemcached().start()
    try:
        mc = make_backend("memcached", caches=[("127.0.0.1", f.port)])
        with _proxy(origin.port, mc) as px:
            c = HttpClient(port=px.port)
            assert lc.inspect(c)[0] == 501 and lc.inspect(c, "?prefix=/a")[0] == 501
            assert lc.dry_run(c, "/a/", "prefix")[0] == 501 and lc.dry_run(c, "/a")[0] == 501
            assert lc.dry_run(c, "/a", "tag", "y")[0] == 501
            c.close()
    finally:
        f.stop()


def test_requests_without_the_new_header_answer_as_before():
    """purge_cases' round trip, byte for byte, with inspection switched on."""
    o = Origin(body_bytes=200).start()
    try:
        be = make_backend("dram", dram_mb=16)
        with Server([("127.0.0.1", o.port)], port=0, backend=be, purge="loopback",
                    inspect="loopback") as px:
            pc.prefix_purge_round_trip(px, o)
    finally:
        o.stop()


def test_cli_accepts_inspect():
    assert build_arg_parser().parse_args(["--inspect", "loopback"]).inspect == "loopback"
    assert build_arg_parser().parse_args([]).inspect == "off"


# ------------------------------------------------------------------- host code, sanitized
def test_listing_host_code_under_sanitizers(tmp_path):
    """tests/native/list_main.cc (its own main): keyed_ntags, HostCache::list_keyed with
    exact-size buffers, the HTTP helpers of inspect.h and the walk's decisions of
    hbm_flight_plan.h, built with ASan and UBSan, as test_tag_purge.py runs tag_block_main.cc."""
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++ on this machine")
    here = os.path.dirname(__file__)
    csrc = os.path.join(here, "..", "shellac_amd", "csrc")
    exe = str(tmp_path / "list_main")
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
           os.path.join(here, "native", "list_main.cc"), os.path.join(csrc, "host_cache.cc"),
           "-o", exe, "-lpthread"]
    b = subprocess.run(cmd, capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    assert "list_main: ok" in r.stdout
