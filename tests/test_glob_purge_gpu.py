"""Purge, soft purge and listing by URL glob on the GPU: k_keyed_scan<GlobMatch, RemoveAction> / k_keyed_scan<GlobMatch, SoftenAction> /
k_list_scan<GlobMatch> against the host twin and the regex model over the scenarios of
tests/glob_cases.py, the HBM backend's glob requests with hot replicas, and the proxy's
X-Purge-Mode: glob and /_shellac/objects?glob= over the HBM tier."""
import time

import pytest

import glob_cases as gc
import purge_cases as pc
import tag_cases as tg
from shellac_amd import core
from shellac_amd.server.proxy import Server, hot_refresh, make_backend

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------- twins and the model
def test_twin_families(cuda_dev):
    gc.run_families([cuda_dev, "cpu"])


@pytest.mark.parametrize("seglen", pc.BOUNDARY_PLENS)
def test_twin_segments_at_granule_boundaries(cuda_dev, seglen):
    gc.run_boundaries([cuda_dev, "cpu"], seglen)


def test_twin_match_is_bounded_by_klen(cuda_dev):
    gc.run_bounded_by_klen([cuda_dev, "cpu"])


def test_twin_overlaps_and_order(cuda_dev):
    gc.run_overlaps([cuda_dev, "cpu"])


def test_twin_variants_go_with_their_base_key(cuda_dev):
    gc.run_variants([cuda_dev, "cpu"])


def test_twin_long_keys(cuda_dev):
    gc.run_long_keys([cuda_dev, "cpu"])


def test_twin_random_sweep(cuda_dev):
    gc.run_random_sweep([cuda_dev, "cpu"])


def test_twin_garbage_values(cuda_dev):
    gc.run_garbage([cuda_dev, "cpu"])


def test_twin_refused_patterns(cuda_dev):
    gc.run_refused([cuda_dev, "cpu"])


def test_expired_and_dead_entries_are_not_counted(cuda_dev):
    gc.run_expired_are_not_counted([cuda_dev])
    gc.run_dead_entries([cuda_dev])


def test_twin_after_the_log_lapped(cuda_dev):
    gc.run_after_the_log_lapped([cuda_dev, "cpu"])


def test_twin_soft_form_over_expiries_and_caps(cuda_dev):
    gc.run_soft_form([cuda_dev, "cpu"])


def test_reference_bit_survives_a_glob_softening(cuda_dev):
    gc.run_reference_bit([cuda_dev])


def test_soften_is_refused_while_a_phase1_batch_is_pending(cuda_dev):
    gc.run_refused_while_phase1_pending([cuda_dev])


def test_twin_listing_rows_pages_and_the_purge_that_follows(cuda_dev):
    gc.run_listing([cuda_dev, "cpu"])


# ------------------------------------------------------------------------------ HbmBackend
def _wait_get(be, key, timeout=5.0):
    deadline = time.time() + timeout
    while time.time() < deadline:
        r = be.get(key)
        if r is not None:
            return r
        time.sleep(0.005)
    return None


def _wait_matched(be, pattern, n, timeout=5.0):
    """Until the tier lists `n` objects under `pattern` (it stores a fill a moment after the
    response went out); the count it saw last."""
    deadline = time.time() + timeout
    got = -1
    while time.time() < deadline:
        got = be.list_objects(glob=pattern, limit=0)["matched"]
        if got == n:
            break
        time.sleep(0.005)
    return got


@pytest.mark.parametrize("edge_server", [True, False])
def test_hbm_backend_purges_softens_and_lists_by_glob(edge_server):
    be = make_backend("hbm", gpus=[0], hbm_gb=0.25, edge_server=edge_server)
    st0 = be.stats()

    def settle(keys):
        assert _wait_get(be, keys[-1]) is not None
    gc.run_backend_glob(be, settle)
    # a SET queued behind the purge is not caught by it
    be.set(b"localhost/i/a/1", b"HTTP/ fresh", 0, 0)
    assert _wait_get(be, b"localhost/i/a/1") == (b"HTTP/ fresh", 0)
    st = be.stats()
    assert st["hbm_glob_purges"] == 5 and st["hbm_glob_purged_objects"] == 4
    assert st["hbm_glob_softened_objects"] == 8
    for name in ("hbm_purges", "hbm_soft_purges", "hbm_purged_objects", "hbm_softened_objects",
                 "hbm_tag_purges", "hbm_tag_purged_objects"):
        assert st[name] == st0[name] == 0, name


def test_glob_purge_removes_hot_replicas_on_every_shard_and_a_refresh_brings_none_back():
    """Two shards on GPU 0 with hot spreading: after a refresh the hot objects live on both
    shards; a glob purge scans every shard in service, so a spread GET of a purged hot key
    misses wherever it lands, before and after the next refresh."""
    be = core().hbm_backend([0, 0], 64 << 20, 1 << 14, 1 << 16, 0, hot_objects=64,
                            hot_refresh_ms=0, hot_sample=1)
    a = [b"/hp/a/%d.css" % i for i in range(200)]
    b = [b"/hp/b/%d.js" % i for i in range(200)]
    for k in a + b:
        be.set(k, b"v-" + k * 4, 0, 0)
    assert _wait_get(be, b[-1]) is not None and _wait_get(be, a[-1]) is not None
    hot = a[:16] + b[:16]
    for _ in range(40):
        be.get_many(hot)
    info = hot_refresh(be)
    assert info["hot"] >= 32 and info["spread_mask"] == 3, info
    assert all(v is not None for v in be.get_many(hot * 8))
    assert be.list_objects(glob=b"/hp/*.css", limit=0)["matched"] > 200    # per stored copy
    n_soft = be.soften_glob(b"/hp/*.css", 77)
    n = be.purge_glob(b"/hp/*.css")
    assert n == n_soft > 200           # the owners' copies and replicas of the hot ones
    assert be.get_many(a[:16] * 16) == [None] * 256   # every replica the spread can pick
    assert be.get_many(a) == [None] * 200
    assert all(v == (b"v-" + k * 4, 0) for k, v in zip(b, be.get_many(b)))
    for _ in range(10):
        be.get_many(hot)
    hot_refresh(be)
    assert be.get_many(a[:16] * 16) == [None] * 256
    assert be.purge_glob(b"/hp/*.css") == 0
    assert all(v == (b"v-" + k * 4, 0) for k, v in zip(b, be.get_many(b)))
    st = be.stats()
    assert st["hbm_glob_purged_objects"] == n and st["hbm_glob_softened_objects"] == n
    assert st["hbm_purged_objects"] == 0 and st["hbm_hot_spread_gets"] > 0


# ----------------------------------------------------------------------------------- proxy
def test_proxy_glob_purge_dry_run_and_inspection_over_the_hbm_backend():
    be = make_backend("hbm", gpus=[0], hbm_gb=0.25)
    o = tg.TagOrigin().start()
    try:
        with Server([("127.0.0.1", o.port)], port=0, backend=be, threads=2, purge="loopback",
                    inspect="loopback") as px:
            def settle():          # 13 URLs, the Vary marker and its two variants
                assert _wait_matched(be, b"localhost/g/*", 16) == 16
            gc.proxy_glob_round_trip(px, o, settle)
            st = be.stats()
            assert st["hbm_glob_purges"] == 5 and st["hbm_glob_purged_objects"] == 10
            # (lists: 4 accepted inspections, 2 dry runs and at least one per settle, of 3)
            assert st["hbm_purges"] == 0 and st["hbm_lists"] >= 9
    finally:
        o.stop()


def test_proxy_soft_glob_purge_with_grace_over_the_hbm_backend():
    be = make_backend("hbm", gpus=[0], hbm_gb=0.25)
    o = tg.TagOrigin().start()
    try:
        with Server([("127.0.0.1", o.port)], port=0, backend=be, threads=2, purge="loopback",
                    ttl=60, grace=30) as px:
            def settle():
                assert _wait_get(be, b"localhost/s/a.js") is not None
                assert _wait_get(be, b"localhost/s/a.css") is not None
            gc.soft_glob_304_round_trip(px, be, o, settle)
            st = be.stats()
            assert st["hbm_glob_softened_objects"] == 1 and st["hbm_glob_purged_objects"] == 1
    finally:
        o.stop()
