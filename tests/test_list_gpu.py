"""Listing on the GPU: k_list_scan / k_list_tiles / k_list_emit against the host twin and the
Python model of tests/list_cases.py (as sets keyed by key bytes: the twins' slot numbers
differ; on each device the slots ascend strictly), beside SETs on a second stream, then the
HBM backend's list_objects (one and two shards, hot replicas, a shard out of service) and the
proxy's GET /_shellac/objects and PURGE dry run over --cache hbm."""
import time

import pytest
import torch

import list_cases as lc
import purge_cases as pc
import tag_cases as tg
from shellac_amd import core
from shellac_amd.ops.cache import item_bytes, keyed, tagged
from shellac_amd.server.proxy import Server, hot_refresh, make_backend

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------- matcher
def test_twin_boundary_patterns_prefix_exact_and_all(cuda_dev):
    lc.run_boundary_patterns([cuda_dev, "cpu"])


def test_twin_garbage_values_are_never_listed(cuda_dev):
    lc.run_garbage([cuda_dev, "cpu"])


def test_expired_entries_are_not_listed_or_counted(cuda_dev):
    lc.run_expired([cuda_dev])


def test_dead_same_digest_entry_and_locked_slot_are_not_listed(cuda_dev):
    lc.run_dead_entries([cuda_dev])


def test_twin_tag_mode_block_forms_alignment_near_misses_and_refused_arguments(cuda_dev):
    lc.run_tag_forms([cuda_dev, "cpu"])


# ---------------------------------------------------------------------------------- rows
def test_twin_rows_say_what_was_stored(cuda_dev):
    lc.run_rows_say_what_was_stored([cuda_dev, "cpu"])


def test_reference_bit_after_a_get_and_after_the_clock_hand(cuda_dev):
    lc.run_reference_bit([cuda_dev])


def test_twin_key_cap_truncation_edge_and_granule_edges(cuda_dev):
    lc.run_key_cap_edges([cuda_dev, "cpu"])


# ---------------------------------------------------------------------- limit and paging
def test_limits_and_start_slots_over_a_sparse_index(cuda_dev):
    lc.run_limits_and_starts([cuda_dev])


def test_pages_concatenate_to_the_one_call_listing(cuda_dev):
    lc.run_paging([cuda_dev])


def test_small_index_of_less_than_one_tile(cuda_dev):
    """8 buckets: 32 slots, one partial tile (the padding of the tile counts is all the scan
    sees past it)."""
    objs = {b"/s/%d" % i: keyed(b"/s/%d" % i, b"v" * i) for i in range(12)}
    for sh in tg.make_shards([cuda_dev, "cpu"], objs, nbuckets=8):
        now = sh.now()
        full = lc.check_list(sh, objs, now, prefix=b"/s/")
        assert len(full) >= 8
        rows, _ = lc.pages(sh, 3, now, prefix=b"/s/")
        assert lc.strip(rows) == lc.strip(full)
        assert sh.list_keyed(prefix=b"/s/", start=32, now=now)["rows"] == []


# --------------------------------------------------------------------------------- state
def test_twin_after_the_log_lapped(cuda_dev):
    lc.run_after_the_log_lapped([cuda_dev, "cpu"])


def test_twin_list_then_purge_removes_what_was_counted_and_changes_nothing_itself(cuda_dev):
    lc.run_purges_and_lists_agree([cuda_dev, "cpu"])


def test_twin_soft_purged_objects_list_with_their_new_words(cuda_dev):
    lc.run_soft_purged_objects([cuda_dev, "cpu"])


def test_list_while_a_phase1_batch_is_pending(cuda_dev):
    lc.run_while_phase1_pending([cuda_dev])


def test_list_beside_sets_on_a_second_stream(cuda_dev):
    """test_tag_purge_beside_sets_on_a_second_stream with a listing: listings on one stream
    while SET batches on another append to the log and lap it (FIFO). The run ends clean; every
    unflagged row names an object that was stored, with its own key and vlen; rows may be
    flagged in any number; nothing is lost or changed by the listings."""
    base = tg.tagged_families(2000, seed=5)
    fills = [{b"/fill/%d/%d" % (b, i): keyed(b"/fill/%d/%d" % (b, i), b"f" * 600)
              for i in range(400)} for b in range(3)]
    g, h = tg.make_shards([cuda_dev, "cpu"], base, evict="fifo", nbuckets=1 << 11)
    stored = {**base, **{k: v for f in fills for k, v in f.items()}}
    s1, s2 = torch.cuda.Stream(cuda_dev), torch.cuda.Stream(cuda_dev)
    now = g.now()
    got = []
    torch.cuda.synchronize(cuda_dev)
    with torch.cuda.stream(s2):
        pc.store(g, fills[0], batch=400)
    with torch.cuda.stream(s1):
        got.append(g.list_keyed(limit=lc.MAX_ROWS, now=now))
    with torch.cuda.stream(s2):
        pc.store(g, fills[1], batch=400)
    with torch.cuda.stream(s1):
        got.append(g.list_keyed(prefix=b"/static/", limit=lc.MAX_ROWS, now=now))
        got.append(g.list_keyed(tags=[b"fam:/static/"], limit=lc.MAX_ROWS, now=now))
    with torch.cuda.stream(s2):
        pc.store(g, fills[2], batch=400)
    torch.cuda.synchronize(cuda_dev)
    for f in fills:
        pc.store(h, f, batch=400)
    assert g.head() == h.head() > g.log_bytes
    for r in got:
        slots = [x["slot"] for x in r["rows"]]
        assert all(a < b for a, b in zip(slots, slots[1:]))
        assert 0 <= len(r["rows"]) <= r["matched"] <= len(stored)
        for x in r["rows"]:
            if x["changed"]:
                assert x["klen"] == 0 and x["key"] == b""
            else:
                assert x["key"] in stored and x["vlen"] == len(stored[x["key"]]), x
                assert x["klen"] == len(x["key"])
    # the listings wrote nothing: the shard holds what the twin holds after the same SETs
    # (up to the inserts' own evictions at a high index load, tag_cases.equalise_live's bound)
    live_g, live_h = tg.live_values(g, stored), tg.live_values(h, stored)
    assert all(v == stored[k] for k, v in live_g.items()) and set(fills[-1]) <= set(live_g)
    assert len(set(live_g) & set(live_h)) >= 0.99 * max(len(live_g), len(live_h))


# ------------------------------------------------------------------------------ HbmBackend
def _wait_keys(be, keys, timeout=5.0):
    deadline = time.time() + timeout
    for k in keys:
        while be.get(k) is None:
            assert time.time() < deadline, k
            time.sleep(0.005)


def _hbm_size(key, val):
    return item_bytes(len(val))


@pytest.mark.parametrize("gpus", [[0], [0, 0]])
def test_hbm_backend_lists_and_pages_across_shards(gpus):
    be = core().hbm_backend(gpus, 64 << 20, 1 << 14, 1 << 16, 0, hot_objects=0)
    lc.run_backend_listing(be, settle=lambda keys: _wait_keys(be, keys), item_size=_hbm_size)
    # a list queued right behind SETs sees them (it is queued to each shard behind its writes)
    more = [b"/q/%d" % i for i in range(300)]
    for k in more:
        be.set(k, b"HTTP/ " + k, 0, 0)
    r = be.list_objects(prefix=b"/q/", limit=0)
    assert r["matched"] == 300 and r["shards_skipped"] == 0
    got, totals = lc.backend_list_all(be, 64, prefix=b"/q/")
    assert sorted(o["key"] for o in got) == sorted(more) and len(totals) == 1
    shards = {o["shard"] for o in got}
    assert shards == set(range(len(gpus)))
    # within a page the shards ascend, and a page of the second shard starts where it says
    assert [o["shard"] for o in got] == sorted(o["shard"] for o in got)
    assert be.list_objects(after=b"nonsense") is None and be.list_objects(after=b"9.0") is None
    assert be.list_objects(after=b"%d.0" % len(gpus))["objects"] == []
    assert be.stats()["hbm_lists"] >= 10


def test_hbm_backend_lists_hot_replicas_once():
    be = core().hbm_backend([0, 0], 64 << 20, 1 << 14, 1 << 16, 0, hot_objects=64,
                            hot_refresh_ms=0, hot_sample=1)
    a = [b"/hp/a/%d" % i for i in range(200)]
    for k in a:
        be.set(k, tagged([b"a"], b"v-" + k * 4), 0, 0)
    _wait_keys(be, a[-3:])
    for _ in range(40):
        be.get_many(a[:16])
    info = hot_refresh(be)
    assert info["hot"] >= 16 and info["spread_mask"] == 3, info
    got, totals = lc.backend_list_all(be, 37, prefix=b"/hp/a/")
    keys = [o["key"] for o in got]
    assert sorted(keys) == sorted(a)                          # every object once
    (matched, _, skipped), = totals
    assert matched > 200 and skipped == 0                     # counted per stored copy
    assert matched == be.purge_prefix(b"/hp/a/")              # as the purge counts


def test_hbm_backend_skips_and_counts_a_shard_out_of_service():
    be = core().hbm_backend([0, 0], 64 << 20, 1 << 14, 1 << 16, 0, hot_objects=0,
                            flush_on_restore=False, warm_restore=False)
    keys = [b"/d/%d" % i for i in range(200)]
    for k in keys:
        be.set(k, b"HTTP/ " + k, 0, 0)
    _wait_keys(be, keys[-3:])
    full, _ = lc.backend_list_all(be, 1000, prefix=b"/d/")
    on1 = sorted(o["key"] for o in full if o["shard"] == 1)
    assert len(full) == 200 and 0 < len(on1) < 200
    assert core().inject_shard_down(be, 0, True)
    got, totals = lc.backend_list_all(be, 50, prefix=b"/d/")
    assert sorted(o["key"] for o in got) == on1 and totals == {(len(on1), totals.copy().pop()[1], 1)}
    core().inject_shard_down(be, 0, False)


def test_proxy_inspect_and_dry_run_over_the_hbm_backend():
    be = make_backend("hbm", gpus=[0], hbm_gb=0.25)
    o = tg.TagOrigin().start()
    try:
        with Server([("127.0.0.1", o.port)], port=0, backend=be, threads=2, purge="loopback",
                    inspect="loopback", tag_header=tg.TAG_HEADER) as px:
            lc.proxy_inspect_round_trip(px, be, o, settle=lambda keys: _wait_keys(be, keys))
            assert be.stats()["hbm_lists"] > 20 and be.stats()["hbm_purges"] >= 2
    finally:
        o.stop()
