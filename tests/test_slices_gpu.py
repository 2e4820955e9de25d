"""Sliced GET on the GPU: k_slice_plan / k_slice_offsets and the byte mover against the host
twin and the Python model of tests/slice_cases.py (every run checks each device's rows,
window bytes and totals against the model, so the twins agree with each other; only a row's
meaningful bytes are compared, not its granules' padding), and beside SETs on a second
stream."""
import pytest
import torch

import purge_cases as pc
import slice_cases as sl
import tag_cases as tg
from shellac_amd.ops.cache import item_bytes, keyed

pytestmark = pytest.mark.gpu


def test_twin_every_window_form_at_every_body_edge(cuda_dev):
    sl.run_windows([cuda_dev, "cpu"])


def test_twin_head_ends_on_granule_and_wave_pass_seams(cuda_dev):
    sl.run_seams([cuda_dev, "cpu"])


def test_twin_every_head_alignment_and_windows_on_granule_edges(cuda_dev):
    sl.run_klens([cuda_dev, "cpu"])


def test_twin_tag_blocks_and_terminator_bytes_in_hashes_and_keys(cuda_dev):
    sl.run_tag_forms([cuda_dev, "cpu"])


def test_twin_values_that_are_not_sliceable_come_back_whole(cuda_dev):
    sl.run_unsliceable([cuda_dev, "cpu"])


def test_twin_heads_at_and_past_the_head_limit(cuda_dev):
    sl.run_long_heads([cuda_dev, "cpu"])


def test_twin_mixed_kinds_duplicates_and_misses_in_one_batch(cuda_dev):
    sl.run_mixed_batch([cuda_dev, "cpu"])


def test_digest_collisions_are_misses(cuda_dev):
    sl.run_collision([cuda_dev, "cpu"])


def test_expired_entries_are_misses(cuda_dev):
    sl.run_expired([cuda_dev, "cpu"])


def test_out_cap_too_small_leaves_out_untouched(cuda_dev):
    sl.run_out_cap([cuda_dev, "cpu"])


def test_twin_after_the_log_lapped(cuda_dev):
    sl.run_after_the_log_lapped([cuda_dev, "cpu"])


def test_reference_bit_after_a_slice_hit_and_not_after_a_miss(cuda_dev):
    sl.run_reference_bit([cuda_dev, "cpu"])


def test_batch_sizes_empty_one_and_65(cuda_dev):
    sl.run_batch_sizes([cuda_dev, "cpu"])


def test_get_slices_front_end(cuda_dev):
    sl.run_get_slices([cuda_dev, "cpu"])


def test_slices_beside_sets_on_a_second_stream(cuda_dev):
    """test_list_beside_sets_on_a_second_stream with sliced GETs: batches on one stream while
    SET batches on another append to the log and lap it (FIFO), each with a reserve that covers
    the SETs queued so far. The run ends clean; every row is a miss or exactly the model's
    answer for the object that was stored, and the batches asked while their objects cannot
    have been reached yet (by the head plus the reserve) hit on every row; nothing stored is
    changed by the sliced GETs."""
    base = {b"/b/%d" % i: sl.obj(b"/b/%d" % i, 40 + i % 50, 250 + i % 100, seed=i)
            for i in range(1500)}
    fills = [{b"/fill/%d/%d" % (b, i): keyed(b"/fill/%d/%d" % (b, i), b"f" * 600)
              for i in range(400)} for b in range(6)]
    g, h = tg.make_shards([cuda_dev, "cpu"], base, evict="fifo", nbuckets=1 << 11,
                          log_bytes=2 << 20)
    stored = {**base, **{k: v for f in fills for k, v in f.items()}}
    bound = [g.set_bound(len(f), sum(sl.up16(len(v)) for v in f.values()) + 16) for f in fills]
    # base fills 617 KB of the 2 MiB log and a fill appends 262 KB: after fill k the head plus
    # the reserve of k + 1 fills stays below the log's end for k < 2 and reaches 114 KB into
    # the base objects (fewer than 300 of them) for k = 2, so these batches must hit
    assert sum(item_bytes(len(v)) for v in base.values()) == 617264
    assert sum(item_bytes(len(v)) for v in fills[0].values()) == 262400 and bound[0] == 268816
    s1, s2 = torch.cuda.Stream(cuda_dev), torch.cuda.Stream(cuda_dev)
    now = g.now()
    keys = list(base)
    asks = [(keys[1000:1500], [(sl.RANGE, 3, 40)] * 500, True),
            (keys[500:1000], [(sl.SUFFIX, 17)] * 500, True),
            (keys[300:500], [(sl.RANGE, 16, 200)] * 200, True),
            (keys[0:500], [(sl.FROM, 100)] * 500, False),
            (keys[500:1000], [(sl.HEAD,)] * 500, False),
            (keys[1000:1500], [(sl.RANGE, 0, 0)] * 500, False)]
    got = []
    torch.cuda.synchronize(cuda_dev)
    for k, (f, (ks, specs, _)) in enumerate(zip(fills, asks)):
        with torch.cuda.stream(s2):
            pc.store(g, f, batch=400)
        with torch.cuda.stream(s1):
            got.append(sl.slices(g, ks, specs, now=now, reserve=sum(bound[:k + 1])))
    torch.cuda.synchronize(cuda_dev)
    for f in fills:
        pc.store(h, f, batch=400)
    assert g.head() == h.head() > g.log_bytes
    for (ks, specs, must_hit), (ans, fields, res, _) in zip(asks, got):
        hits = 0
        for k, s, a in zip(ks, specs, ans):
            if a["status"] == "miss":
                assert a == sl.MISS
            else:
                assert a == sl.model_answer(base[k], s, flags=0), (k, s)
                hits += 1
        assert res[0] == hits and (hits == len(ks) or not must_hit), (hits, len(ks))
    # the sliced GETs wrote nothing but reference bits: the shard holds what the twin holds
    live_g, live_h = tg.live_values(g, stored), tg.live_values(h, stored)
    assert all(v == stored[k] for k, v in live_g.items()) and set(fills[-1]) <= set(live_g)
    assert len(set(live_g) & set(live_h)) >= 0.99 * max(len(live_g), len(live_h))


# ------------------------------------------------------------------------------ HbmBackend
import time  # noqa: E402

from shellac_amd import core  # noqa: E402
from shellac_amd.server.proxy import Server, hot_refresh, make_backend  # noqa: E402


def _wait_keys(be, keys, timeout=5.0):
    deadline = time.time() + timeout
    for k in keys:
        while be.get(k) is None:
            assert time.time() < deadline, k
            time.sleep(0.005)


@pytest.mark.parametrize("gpus", [[0], [0, 0]])
def test_hbm_backend_get_part_equals_the_host_cut(gpus):
    be = core().hbm_backend(gpus, 64 << 20, 1 << 14, 1 << 16, 0, hot_objects=0)
    objs = sl.run_backend_parts(be, settle=lambda keys: _wait_keys(be, keys))
    st = be.stats()
    assert st["hbm_slices"] >= 10 * (len(objs) + 1) + 64 and st["hbm_key_mismatch"] == 0
    # read-your-writes: a part asked for right behind its SET is planned behind it
    for i in range(50):
        k, v = b"/ryw/%d" % i, sl.head_of(40) + sl.body_of(100 + i, i)
        be.set(k, v, sl.FLAGS, 0)
        assert sl.parts(be, [k], [(sl.SUFFIX, 5)]) == [sl.model_part(v, (sl.SUFFIX, 5))]
    # more bytes than a flight's arena holds, asked at once: a flight with others queued behind
    # it answers misses, as an overflowing GET batch does
    want = sl.model_part(objs[b"/p/big"], (sl.WHOLE,))
    got = sl.parts(be, [b"/p/big"] * 64, [(sl.WHOLE,)] * 64)
    assert all(g in (want, sl.PART_MISS) for g in got) and want in got
    # a forged collision: another key under this key's digest is a miss
    be.set(b"/attacker", sl.head_of(40) + b"evil", 0, 0, digest_of=b"/victim")
    assert sl.parts(be, [b"/victim"], [(sl.RANGE, 0, 1)]) == [sl.PART_MISS]
    assert sl.parts(be, [b"/attacker"], [(sl.RANGE, 0, 1)], digest_of=b"/victim")[0]["window"] == b"ev"


def test_hbm_backend_asks_again_for_a_part_that_outgrew_its_arena():
    """One part larger than the smallest pinned arena (1 MiB), alone on its stream: the
    flight's bytes do not fit, deliver_slices takes a bigger arena and runs the sliced GET
    again, and the answer is the host cut."""
    be = core().hbm_backend([0], 64 << 20, 1 << 12, 2 << 20, 0, hot_objects=0)
    v = sl.head_of(100) + sl.body_of(1000, 5) * 1500
    be.set(b"/wide", v, sl.FLAGS, 0)
    for n, spec in enumerate([(sl.WHOLE,), (sl.FROM, 10), (sl.RANGE, 1400000, 1400099)]):
        assert sl.parts(be, [b"/wide"], [spec]) == [sl.model_part(v, spec)]
        st = be.stats()                      # (no GET ran: the regathers are the slices')
        assert st["hbm_regathers"] >= min(n + 1, 2) and st["hbm_arena_misses"] == 0


def test_hbm_backend_get_part_from_hot_replicas_and_with_a_shard_out_of_service():
    be = core().hbm_backend([0, 0], 64 << 20, 1 << 14, 1 << 16, 0, hot_objects=64,
                            hot_refresh_ms=0, hot_sample=1, flush_on_restore=True)
    objs = {b"/hp/%d" % i: sl.head_of(40 + i % 9) + sl.body_of(200 + i, i) for i in range(200)}
    for k, v in objs.items():
        be.set(k, v, sl.FLAGS, 0)
    _wait_keys(be, list(objs)[-3:])
    keys = list(objs)
    for _ in range(40):
        be.get_many(keys[:16])
    info = hot_refresh(be)
    assert info["hot"] >= 16 and info["spread_mask"] == 3, info
    spec = (sl.RANGE, 7, 77)
    want = [sl.model_part(objs[k], spec) for k in keys]
    for _ in range(4):                                   # hot keys are answered by either shard
        assert sl.parts(be, keys, [spec] * len(keys)) == want
    assert be.stats()["hbm_hot_spread_gets"] > 0
    be2 = core().hbm_backend([0, 0], 64 << 20, 1 << 14, 1 << 16, 0, hot_objects=0,
                             flush_on_restore=False, warm_restore=False)
    for k, v in objs.items():
        be2.set(k, v, sl.FLAGS, 0)
    _wait_keys(be2, keys[-3:])
    assert sl.parts(be2, keys, [spec] * len(keys)) == want
    assert core().inject_shard_down(be2, 0, True)
    got = sl.parts(be2, keys, [spec] * len(keys))
    assert all(g in (w, sl.PART_MISS) for g, w in zip(got, want))
    assert 0 < sum(g == sl.PART_MISS for g in got) < len(keys)    # shard 0's keys are misses
    core().inject_shard_down(be2, 0, False)


def test_proxy_partial_hits_over_the_hbm_backend():
    be = make_backend("hbm", gpus=[0], hbm_gb=0.25)
    o = sl.RangeOrigin().start()
    try:
        with Server([("127.0.0.1", o.port)], port=0, backend=be, threads=2,
                    partial_hits=True) as px:
            sl.proxy_partial_round_trip(
                px, o, settle=lambda paths: _wait_keys(be, [b"localhost" + p.encode() for p in paths]))
            assert be.stats()["hbm_slices"] >= 20
    finally:
        o.stop()
