"""Conditional sliced GET on the GPU: k_slice_plan with conditions against the host twin and the Python
model of tests/cond_cases.py (every run checks each device's rows, bytes, result words and
get_bytes against the model, so the twins agree with each other), and beside SETs on a second
stream."""
import pytest
import torch

import cond_cases as cc
import purge_cases as pc
import slice_cases as sl
import tag_cases as tg
from shellac_amd.ops.cache import item_bytes, keyed

pytestmark = pytest.mark.gpu


def test_twin_line_start_at_every_granule_phase_and_head_alignment(cuda_dev):
    cc.run_line_phases([cuda_dev, "cpu"])


def test_twin_line_start_name_and_colon_across_the_wave_pass_seams(cuda_dev):
    cc.run_seams([cuda_dev, "cpu"])


def test_twin_validator_first_last_both_and_at_the_head_limit(cuda_dev):
    cc.run_positions([cuda_dev, "cpu"])


def test_twin_name_forms_decoys_and_duplicates(cuda_dev):
    cc.run_names([cuda_dev, "cpu"])


def test_twin_value_lengths_blanks_stretch_and_weak_tags_under_each_kind(cuda_dev):
    cc.run_values([cuda_dev, "cpu"])


def test_twin_candidate_lists_star_and_malformed_conditions(cuda_dev):
    cc.run_candidates([cuda_dev, "cpu"])


def test_twin_every_kind_matched_and_not_over_every_window_form(cuda_dev):
    cc.run_outcomes([cuda_dev, "cpu"])


def test_twin_batch_sizes_mixed_rows_and_no_conditions_equal_the_plain_call(cuda_dev):
    cc.run_batches([cuda_dev, "cpu"])


def test_out_cap_too_small_leaves_out_untouched(cuda_dev):
    cc.run_out_cap([cuda_dev, "cpu"])


def test_twin_after_the_log_lapped(cuda_dev):
    cc.run_after_the_log_lapped([cuda_dev, "cpu"])


def test_reference_bit_after_a_not_modified_hit_and_not_after_a_miss(cuda_dev):
    cc.run_reference_bit([cuda_dev, "cpu"])


def test_get_slices_front_end_with_conditions(cuda_dev):
    cc.run_get_slices([cuda_dev, "cpu"])


def _etag_obj(i):
    """slice_cases.obj(key, 40 + i % 50, 250 + i % 100, seed=i) with an ETag line in a head of
    the same size."""
    k = b"/b/%d" % i
    head = cc.head_lines([b'ETag: "%04d"' % i, b"X-P: " + b"a" * (i % 50)])
    assert len(head) == 40 + i % 50
    return k, keyed(k, head + sl.body_of(250 + i % 100, i))


def test_conditional_slices_beside_sets_on_a_second_stream(cuda_dev):
    """test_slices_beside_sets_on_a_second_stream with conditions: the same object counts,
    sizes, log and reserves, every object with an ETag, and half of each batch's rows carrying
    the tag that matches. Every row is a miss or exactly the model's answer for the stored
    object, and the batches asked while their objects cannot have been reached yet hit on every
    row; nothing stored is changed."""
    base = dict(_etag_obj(i) for i in range(1500))
    fills = [{b"/fill/%d/%d" % (b, i): keyed(b"/fill/%d/%d" % (b, i), b"f" * 600)
              for i in range(400)} for b in range(6)]
    g, h = tg.make_shards([cuda_dev, "cpu"], base, evict="fifo", nbuckets=1 << 11,
                          log_bytes=2 << 20)
    stored = {**base, **{k: v for f in fills for k, v in f.items()}}
    bound = [g.set_bound(len(f), sum(sl.up16(len(v)) for v in f.values()) + 16) for f in fills]
    # (the sums test_slices_beside_sets_on_a_second_stream reasons from)
    assert sum(item_bytes(len(v)) for v in base.values()) == 617264
    assert sum(item_bytes(len(v)) for v in fills[0].values()) == 262400 and bound[0] == 268816
    s1, s2 = torch.cuda.Stream(cuda_dev), torch.cuda.Stream(cuda_dev)
    now = g.now()
    keys = list(base)

    def conds(ks, form):
        out = []
        for j, k in enumerate(ks):
            tag = b'"%04d"' % int(k[3:])
            arg = tag if j % 2 == 0 else cc.OTHER
            out.append((form, [arg]) if form == "none_match" else (form, arg))
        return out

    asks = [(keys[1000:1500], [(sl.RANGE, 3, 40)] * 500, "none_match", True),
            (keys[500:1000], [(sl.SUFFIX, 17)] * 500, "if_range_etag", True),
            (keys[300:500], [(sl.WHOLE,)] * 200, "none_match", True),
            (keys[0:500], [(sl.FROM, 100)] * 500, "none_match", False),
            (keys[500:1000], [(sl.HEAD,)] * 500, "if_range_etag", False),
            (keys[1000:1500], [(sl.RANGE, 0, 0)] * 500, "none_match", False)]
    got = []
    torch.cuda.synchronize(cuda_dev)
    for k, (f, (ks, specs, form, _)) in enumerate(zip(fills, asks)):
        with torch.cuda.stream(s2):
            pc.store(g, f, batch=400)
        with torch.cuda.stream(s1):
            got.append(cc.slices(g, ks, specs, conds(ks, form), now=now, reserve=sum(bound[:k + 1])))
    torch.cuda.synchronize(cuda_dev)
    for f in fills:
        pc.store(h, f, batch=400)
    assert g.head() == h.head() > g.log_bytes
    for (ks, specs, form, must_hit), (ans, fields, res, _) in zip(asks, got):
        hits = 0
        for k, s, c, a in zip(ks, specs, conds(ks, form), ans):
            if a["status"] == "miss":
                assert a == sl.MISS
            else:
                assert a == cc.model_answer(base[k], s, c, flags=0), (k, s, c)
                hits += 1
        assert res[0] == hits and (hits == len(ks) or not must_hit), (hits, len(ks))
        if must_hit:
            want = {"none_match": ["not_modified", "whole" if specs[0] == (sl.WHOLE,) else "ok"],
                    "if_range_etag": ["ok", "whole"]}[form]
            assert [a["status"] for a in ans] == want * (len(ks) // 2)
    live_g, live_h = tg.live_values(g, stored), tg.live_values(h, stored)
    assert all(v == stored[k] for k, v in live_g.items()) and set(fills[-1]) <= set(live_g)
    assert len(set(live_g) & set(live_h)) >= 0.99 * max(len(live_g), len(live_h))


# ------------------------------------------------------------------------------ HbmBackend
import time  # noqa: E402

from shellac_amd import core  # noqa: E402


def _wait_keys(be, keys, timeout=5.0):
    deadline = time.time() + timeout
    for k in keys:
        while be.get(k) is None:
            assert time.time() < deadline, k
            time.sleep(0.005)


@pytest.mark.parametrize("gpus", [[0], [0, 0]])
def test_hbm_backend_get_part_if_equals_the_host_decision_and_cut(gpus):
    be = core().hbm_backend(gpus, 64 << 20, 1 << 14, 1 << 16, 0, hot_objects=0)
    objs = cc.run_backend_parts(be, settle=lambda keys: _wait_keys(be, keys))
    st = be.stats()
    assert st["hbm_cond_slices"] >= 5 * 11 * (len(objs) + 1) and st["hbm_key_mismatch"] == 0
    assert st["hbm_slices"] > st["hbm_cond_slices"]
    # read-your-writes: a conditional part asked right behind its SET is planned behind it
    for i in range(20):
        k, tag = b"/ryw/%d" % i, b'"t%d"' % i
        v = cc.head_lines([b"ETag: " + tag]) + sl.body_of(100 + i, i)
        be.set(k, v, sl.FLAGS, 0)
        cond = ("none_match", [tag if i % 2 else cc.OTHER])
        assert cc.parts(be, [k], [(sl.SUFFIX, 5)], [cond]) == [cc.model_part(v, (sl.SUFFIX, 5), cond)]
    # a forged collision: another key under this key's digest is a miss under a condition too
    be.set(b"/attacker", cc.head_lines([b"ETag: " + cc.TAG]) + b"evil", 0, 0, digest_of=b"/victim")
    assert cc.parts(be, [b"/victim"], [(sl.WHOLE,)], [("none_match", "*")]) == [sl.PART_MISS]


def test_hbm_backend_asks_again_with_the_conditions_when_the_arena_falls_short():
    """One part larger than the smallest pinned arena, alone on its stream, under conditions:
    the flight's bytes do not fit, deliver_slices takes a bigger arena and runs the sliced GET
    again with the same conditions; a matched none_match needs no second ask."""
    be = core().hbm_backend([0], 64 << 20, 1 << 12, 2 << 20, 0, hot_objects=0)
    v = cc.head_lines([b"ETag: " + cc.TAG, b"X-P: " + b"a" * 60]) + sl.body_of(1000, 5) * 1500
    be.set(b"/wide", v, sl.FLAGS, 0)
    asks = [((sl.WHOLE,), ("none_match", [cc.TAG]), 0), ((sl.WHOLE,), ("none_match", [cc.OTHER]), 1),
            ((sl.RANGE, 10, 19), ("if_range_etag", cc.OTHER), 1), ((sl.RANGE, 10, 19), ("if_range_etag", cc.TAG), 1)]
    for spec, cond, regathers in asks:
        assert cc.parts(be, [b"/wide"], [spec], [cond]) == [cc.model_part(v, spec, cond)]
        st = be.stats()
        assert st["hbm_regathers"] >= regathers and st["hbm_arena_misses"] == 0
    assert be.stats()["hbm_regathers"] <= 3


def test_proxy_conditional_hits_over_the_hbm_backend():
    from shellac_amd.server.proxy import Server, make_backend
    be = make_backend("hbm", gpus=[0], hbm_gb=0.25)
    o = cc.CondOrigin().start()
    try:
        with Server([("127.0.0.1", o.port)], port=0, backend=be, threads=2, partial_hits=True,
                    conditional_hits=True) as px:
            cc.proxy_conditional_round_trip(
                px, o, settle=lambda paths: _wait_keys(be, [b"localhost" + p.encode() for p in paths]))
            st = be.stats()
            assert st["hbm_cond_slices"] >= 40 and st["hbm_slices"] > st["hbm_cond_slices"]
    finally:
        o.stop()
