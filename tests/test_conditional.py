"""Conditional sliced GET on the CPU: csrc/conditional.h and HostCache::get_keyed_slices with
conditions (the semantic reference of k_slice_plan with conditions) against the Python model of
tests/cond_cases.py, the request-header parsers, and the host code under sanitizers."""
import os
import shutil
import subprocess

import pytest

import cond_cases as cc

CPU = ["cpu"]


# ------------------------------------------------------------------- model and conditional.h
def test_comparison_rules_against_rfc_9110_weak_and_strong():
    cc.run_model_against_rfc()


def test_request_header_parsers_against_the_rules():
    cc.run_parsers()


def test_pack_slice_conds_packs_the_documented_records():
    cc.run_pack_slice_conds()


# --------------------------------------------------------------------------- the field lookup
def test_line_start_at_every_granule_phase_and_head_alignment():
    cc.run_line_phases(CPU)


def test_line_start_name_and_colon_across_the_wave_pass_seams():
    cc.run_seams(CPU)


def test_validator_first_last_both_and_at_the_head_limit():
    cc.run_positions(CPU)


def test_name_forms_decoys_and_duplicates():
    cc.run_names(CPU)


def test_value_lengths_blanks_stretch_and_weak_tags_under_each_kind():
    cc.run_values(CPU)


def test_candidate_lists_star_and_malformed_conditions():
    cc.run_candidates(CPU)


# ------------------------------------------------------------------------------- row outcomes
def test_every_kind_matched_and_not_over_every_window_form():
    cc.run_outcomes(CPU)


# ----------------------------------------------------------------------------------- batches
def test_batch_sizes_mixed_rows_and_no_conditions_equal_the_plain_call():
    cc.run_batches(CPU)


def test_out_cap_too_small_leaves_out_untouched():
    cc.run_out_cap(CPU)


def test_after_the_log_lapped():
    cc.run_after_the_log_lapped(CPU)


def test_reference_bit_after_a_not_modified_hit_and_not_after_a_miss():
    cc.run_reference_bit(CPU)


def test_get_slices_front_end_with_conditions():
    cc.run_get_slices(CPU)


# ------------------------------------------------------------------- host code, sanitized
def test_conditional_host_code_under_sanitizers(tmp_path):
    """tests/native/cond_main.cc (its own main): conditional.h, the header parsers and
    HostCache::get_keyed_slices with conditions on the seam cases with exact-size buffers,
    built with ASan and UBSan, as test_slices.py runs slice_main.cc."""
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++ on this machine")
    here = os.path.dirname(__file__)
    csrc = os.path.join(here, "..", "shellac_amd", "csrc")
    exe = str(tmp_path / "cond_main")
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
           os.path.join(here, "native", "cond_main.cc"), os.path.join(csrc, "host_cache.cc"),
           "-o", exe, "-lpthread"]
    b = subprocess.run(cmd, capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    assert "cond_main: ok" in r.stdout


# ------------------------------------------------------------------------------------ tiers
from shellac_amd import core  # noqa: E402
from shellac_amd.server.proxy import make_backend  # noqa: E402
from shellac_amd.utils.fakemc import FakeMemcached  # noqa: E402

import slice_cases as sl  # noqa: E402


@pytest.mark.parametrize("kind", ["dram", "fault"])
def test_default_get_part_if_over_the_dram_backend(kind):
    be = make_backend("dram", dram_mb=16, **({"fault": ""} if kind == "fault" else {}))
    cc.run_backend_parts(be)


def test_default_get_part_if_over_a_memcached_node():
    f = FakeMemcached().start()
    try:
        cc.run_backend_parts(make_backend("memcached", caches=[("127.0.0.1", f.port)]))
    finally:
        f.stop()


def test_tiered_backend_decides_l1_hits_asks_l2_with_the_condition_and_never_fills_l1():
    c = core()
    l1, l2 = c.dram_backend(8 << 20, 1 << 20), c.dram_backend(8 << 20, 1 << 20)
    be = c.tiered_backend(l1, l2)
    objs = cc.run_backend_parts(be)                       # written to both levels: L1 hits
    st = be.stats()
    assert st["tier_l1_hits"] > 0 and st["tier_l2_hits"] == 0
    deep = cc.head_lines([b"ETag: " + cc.TAG]) + sl.body_of(300, 9)
    l2.set(b"/only/l2", deep, sl.FLAGS, 0)
    asks = [((sl.RANGE, 4, 19), ("none_match", [cc.TAG]), cc.NOT_MODIFIED),
            ((sl.RANGE, 4, 19), ("none_match", [cc.OTHER]), 1),
            ((sl.RANGE, 4, 19), ("if_range_etag", cc.OTHER), 3),
            ((sl.WHOLE,), ("none_match", "*"), cc.NOT_MODIFIED)]
    for spec, cond, status in asks:
        got = cc.parts(be, [b"/only/l2"], [spec], [cond])
        assert got == [cc.model_part(deep, spec, cond)] and got[0]["status"] == status
    st = be.stats()
    assert st["tier_l2_hits"] == 4 and st["tier_promoted"] == 0
    assert st["l1_cache_objects"] == len(objs) and l1.get(b"/only/l2") is None


# ------------------------------------------------------------------------------------ proxy
from shellac_amd.server.proxy import Server, build_arg_parser  # noqa: E402
from shellac_amd.utils.httpclient import HttpClient  # noqa: E402


@pytest.fixture
def origin():
    o = cc.CondOrigin().start()
    yield o
    o.stop()


def _proxy(origin, backend, **kw):
    kw.setdefault("partial_hits", True)
    kw.setdefault("conditional_hits", True)
    return Server([("127.0.0.1", origin.port)], port=0, backend=backend, **kw).start()


def test_proxy_conditional_hits_over_dram(origin):
    be = make_backend("dram", dram_mb=16)
    with _proxy(origin, be, threads=2) as px:
        cc.proxy_conditional_round_trip(px, origin)


def test_proxy_conditional_hits_over_the_tiered_backend(origin):
    c = core()
    be = c.tiered_backend(c.dram_backend(8 << 20, 1 << 20), c.dram_backend(8 << 20, 1 << 20))
    with _proxy(origin, be) as px:
        cc.proxy_conditional_round_trip(px, origin)


def test_proxy_stale_object_under_grace_is_a_304_and_one_background_revalidation(origin):
    be = make_backend("dram", dram_mb=16)
    with _proxy(origin, be, grace=30, purge="loopback") as px:
        c = HttpClient(port=px.port)
        p = "/c/stale"
        full, tag = cc.CondOrigin.body(p), cc.CondOrigin.etag(p)
        assert sl.fetch(c, p)[2] == full
        assert cc.is_304(sl.fetch(c, p, {"If-None-Match": tag.decode()}), tag)
        assert c.get(p, method="PURGE", headers={"X-Purge-Soft": "1"}).status() == 200
        assert cc.is_304(sl.fetch(c, p, {"If-None-Match": tag.decode()}), tag)     # served stale
        st = px.stats()
        assert st["stale_served"] == 1 and st["revalidations"] == 1 and st["not_modified_304"] == 2
        assert sl.fetch(c, p, {"If-None-Match": '"o"'})[::2] == (200, full)
        c.close()


def test_proxy_conditional_hits_without_partial_hits(origin):
    """Without --partial-hits a 304 is still answered from the cache; Range and If-Range are
    ignored as before, and a HEAD goes upstream."""
    be = make_backend("dram", dram_mb=16)
    with _proxy(origin, be, partial_hits=False) as px:
        c = HttpClient(port=px.port)
        p = "/c/1"
        full, tag = cc.CondOrigin.body(p), cc.CondOrigin.etag(p)
        assert sl.fetch(c, p)[2] == full
        st, h, b = sl.fetch(c, p, {"If-None-Match": tag.decode()})
        assert (st, b) == (304, b"") and h["etag"].encode() == tag
        assert sl.fetch(c, p, {"Range": "bytes=0-3", "If-Range": tag.decode()})[::2] == (200, full)
        assert sl.fetch(c, p, {"Range": "bytes=0-3", "If-None-Match": '"o"'})[::2] == (200, full)
        assert sl.fetch(c, p, {"If-None-Match": tag.decode()}, method="HEAD")[0] == 200
        assert origin.hits[("HEAD", p)] == 1 and origin.hits[("GET", p)] == 1
        c.close()


def test_the_same_requests_without_the_flag_answer_as_before(origin):
    be = make_backend("dram", dram_mb=16)
    with _proxy(origin, be, conditional_hits=False) as px:
        c = HttpClient(port=px.port)
        p = "/c/1"
        full, tag = cc.CondOrigin.body(p), cc.CondOrigin.etag(p).decode()
        assert sl.fetch(c, p)[2] == full
        for hdr in ({"If-None-Match": tag}, {"If-None-Match": "*"}, {"If-Modified-Since": cc.DATE.decode()},
                    {"Range": "bytes=0-3", "If-Range": tag}, {"Range": "bytes=0-3", "If-Range": '"o"'}):
            st, h, b = sl.fetch(c, p, hdr)
            assert (st, b) == (200, full) and "content-range" not in h, hdr
        assert sl.fetch(c, p, {"Range": "bytes=0-3", "If-None-Match": tag})[::2] == (206, full[:4])
        st, h, b = sl.fetch(c, p, {"If-None-Match": tag}, method="HEAD")
        assert (st, b) == (200, b"") and origin.hits[("HEAD", p)] == 0
        assert origin.hits[("GET", p)] == 1
        st = px.stats()
        assert st["conditional_requests"] == st["not_modified_304"] == 0
        assert st["if_range_matched"] == st["if_range_failed"] == 0 and st["range_206"] == 1
        c.close()


def test_cli_accepts_conditional_hits():
    assert build_arg_parser().parse_args(["--conditional-hits"]).conditional_hits is True
    assert build_arg_parser().parse_args([]).conditional_hits is False
