"""Sliced GET on the CPU: csrc/slice.h and HostCache::get_keyed_slices (the semantic reference
of k_slice_plan) against the Python model of tests/slice_cases.py, and the host code under
sanitizers."""
import os
import shutil
import subprocess

import pytest

import slice_cases as sl

CPU = ["cpu"]


# ------------------------------------------------------------------------- model and slice.h
def test_resolve_window_and_layout_against_the_model():
    sl.run_resolve_window()


def test_every_window_form_at_every_body_edge():
    sl.run_windows(CPU)


# ----------------------------------------------------------------------------- the head's end
def test_head_ends_on_granule_and_wave_pass_seams():
    sl.run_seams(CPU)


def test_every_head_alignment_and_windows_on_granule_edges():
    sl.run_klens(CPU)


def test_tag_blocks_and_terminator_bytes_in_hashes_and_keys():
    sl.run_tag_forms(CPU)


def test_values_that_are_not_sliceable_come_back_whole():
    sl.run_unsliceable(CPU)


def test_heads_at_and_past_the_head_limit():
    sl.run_long_heads(CPU)


# ----------------------------------------------------------------------------------- batches
def test_mixed_kinds_duplicates_and_misses_in_one_batch():
    sl.run_mixed_batch(CPU)


def test_digest_collisions_are_misses():
    sl.run_collision(CPU)


def test_expired_entries_are_misses():
    sl.run_expired(CPU)


def test_out_cap_too_small_leaves_out_untouched():
    sl.run_out_cap(CPU)


def test_after_the_log_lapped():
    sl.run_after_the_log_lapped(CPU)


def test_reference_bit_after_a_slice_hit_and_not_after_a_miss():
    sl.run_reference_bit(CPU)


def test_batch_sizes_empty_one_and_65():
    sl.run_batch_sizes(CPU)


def test_get_slices_front_end():
    sl.run_get_slices(CPU)


# ------------------------------------------------------------------- host code, sanitized
def test_slice_host_code_under_sanitizers(tmp_path):
    """tests/native/slice_main.cc (its own main): slice.h and HostCache::get_keyed_slices on
    the seam cases with exact-size buffers, built with ASan and UBSan, as test_list.py runs
    list_main.cc."""
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++ on this machine")
    here = os.path.dirname(__file__)
    csrc = os.path.join(here, "..", "shellac_amd", "csrc")
    exe = str(tmp_path / "slice_main")
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
           os.path.join(here, "native", "slice_main.cc"), os.path.join(csrc, "host_cache.cc"),
           "-o", exe, "-lpthread"]
    b = subprocess.run(cmd, capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    assert "slice_main: ok" in r.stdout


# ------------------------------------------------------------------------------------ tiers
from shellac_amd import core  # noqa: E402
from shellac_amd.server.proxy import Server, build_arg_parser, make_backend  # noqa: E402
from shellac_amd.utils.fakemc import FakeMemcached  # noqa: E402
from shellac_amd.utils.httpclient import HttpClient  # noqa: E402


@pytest.mark.parametrize("kind", ["dram", "fault"])
def test_default_get_part_over_the_dram_backend(kind):
    be = make_backend("dram", dram_mb=16, **({"fault": ""} if kind == "fault" else {}))
    sl.run_backend_parts(be)


def test_default_get_part_over_a_memcached_node():
    f = FakeMemcached().start()
    try:
        sl.run_backend_parts(make_backend("memcached", caches=[("127.0.0.1", f.port)]))
    finally:
        f.stop()


def test_tiered_backend_slices_l1_hits_asks_l2_and_never_fills_l1_from_a_part():
    c = core()
    l1, l2 = c.dram_backend(8 << 20, 1 << 20), c.dram_backend(8 << 20, 1 << 20)
    be = c.tiered_backend(l1, l2)
    objs = sl.run_backend_parts(be)                       # written to both levels: L1 hits
    st = be.stats()
    assert st["tier_l1_hits"] > 0 and st["tier_l2_hits"] == 0
    deep = sl.head_of(50) + sl.body_of(300, 9)
    l2.set(b"/only/l2", deep, sl.FLAGS, 0)
    for spec in [(sl.RANGE, 4, 19), (sl.HEAD,), (sl.WHOLE,), (sl.SUFFIX, 3)]:
        assert sl.parts(be, [b"/only/l2"], [spec]) == [sl.model_part(deep, spec)]
    st = be.stats()
    assert st["tier_l2_hits"] == 4 and st["tier_promoted"] == 0
    assert st["l1_cache_objects"] == len(objs) and l1.get(b"/only/l2") is None
    assert be.get(b"/only/l2")[0] == deep and l1.get(b"/only/l2") is not None   # get() promotes


# ------------------------------------------------------------------------------------ proxy
@pytest.fixture
def origin():
    o = sl.RangeOrigin().start()
    yield o
    o.stop()


def _proxy(origin, backend, **kw):
    kw.setdefault("partial_hits", True)
    return Server([("127.0.0.1", origin.port)], port=0, backend=backend, **kw).start()


def test_proxy_partial_hits_over_dram(origin):
    be = make_backend("dram", dram_mb=16)
    with _proxy(origin, be, threads=2) as px:
        sl.proxy_partial_round_trip(px, origin)
        text = HttpClient(port=px.port).get("/_shellac/metrics").body().read().decode()
        assert "shellac_range_206 10" in text and "shellac_head_hits 2" in text


def test_proxy_partial_hits_fall_back_to_a_whole_get(origin):
    """A gzip-coded object for a client that did not ask for gzip, an object stale under
    --grace (soft-purged: stale at once) and a stored status other than 200 are answered as
    without the option."""
    be = make_backend("dram", dram_mb=16)
    with _proxy(origin, be, grace=30, purge="loopback") as px:
        c = HttpClient(port=px.port)
        full = sl.RangeOrigin.body("/r/stale")
        assert sl.fetch(c, "/r/stale")[2] == full
        assert sl.fetch(c, "/r/stale", {"Range": "bytes=0-4"})[0] == 206
        assert c.get("/r/stale", method="PURGE", headers={"X-Purge-Soft": "1"}).status() == 200
        st, h, b = sl.fetch(c, "/r/stale", {"Range": "bytes=0-4"})
        assert (st, b) == (200, full)                      # served stale, whole, and revalidated
        assert px.stats()["partial_fallbacks"] == 1 and px.stats()["stale_served"] == 1
        c.close()
    be = make_backend("dram", dram_mb=16)
    with _proxy(origin, be) as px:
        c = HttpClient(port=px.port)
        gz = sl.RangeOrigin.body("/gz/1")
        assert sl.fetch(c, "/gz/1", {"Accept-Encoding": "gzip"})[2] == gz      # stored gzip-coded
        st, h, b = sl.fetch(c, "/gz/1", {"Range": "bytes=0-9"})
        assert (st, b) == (200, gz) and "content-encoding" not in h
        assert px.stats()["partial_fallbacks"] == 1 and px.stats()["range_206"] == 0
        assert origin.hits[("GET", "/gz/1")] == 1
        c.close()
    be = make_backend("dram", dram_mb=16)
    with _proxy(origin, be, policy="reference") as px:
        c = HttpClient(port=px.port)
        tea = sl.RangeOrigin.body("/teapot/1")
        assert sl.fetch(c, "/teapot/1")[0] == 203
        st, h, b = sl.fetch(c, "/teapot/1", {"Range": "bytes=0-9"})
        assert (st, b) == (203, tea) and px.stats()["partial_fallbacks"] == 1
        assert origin.hits[("GET", "/teapot/1")] == 1
        c.close()


def test_the_same_requests_without_the_flag_answer_as_before(origin):
    be = make_backend("dram", dram_mb=16)
    with _proxy(origin, be, partial_hits=False) as px:
        c = HttpClient(port=px.port)
        full = sl.RangeOrigin.body("/r/1")
        for hdr in ({}, {"Range": "bytes=0-0"}, {"Range": "bytes=-7"}, {"Range": "bytes=99999-"}):
            st, h, b = sl.fetch(c, "/r/1", hdr)
            assert (st, b) == (200, full) and "accept-ranges" not in h and "content-range" not in h
        assert origin.hits[("GET", "/r/1")] == 1
        assert sl.fetch(c, "/r/1", method="HEAD")[0] == 200
        assert origin.hits[("HEAD", "/r/1")] == 1                     # a HEAD goes upstream
        st = px.stats()
        assert st["range_requests"] == st["head_hits"] == st["partial_fallbacks"] == 0
        c.close()


def test_cli_accepts_partial_hits():
    assert build_arg_parser().parse_args(["--partial-hits"]).partial_hits is True
    assert build_arg_parser().parse_args([]).partial_hits is False
