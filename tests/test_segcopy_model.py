"""The byte mover's NumPy model, its case builders and the host twins, without a GPU:
every case family of tests/test_segcopy_gpu.py runs here through ``host_segcopy`` /
``host_segcopy_sized`` against ``ref_segcopy``, and asserts from ``plan_passes`` — fed with
today's kernel constants and assumed grids of 1, 1 536 and 4 096 workgroups — that it reaches
the path it is named for. Byte-exact throughout."""
import numpy as np
import pytest
import torch

from shellac_amd.ops import routing as R

import segcopy_cases as SC

CPU = torch.device("cpu")
STAGES = {"modes 0/3/4": SC.TODAY["stage"], "mode 2": SC.TODAY["stage_sized"],
          "lds-dma": SC.TODAY["stage_glds"]}
MIN_TILE = SC.TODAY["min_tile"]


def _same(got, want, what):
    bad = SC.first_diff(got, want)
    assert not bad, f"{what}: {bad}"


# ---- the model against hand-made expectations ------------------------------------------
def test_ref_segcopy_by_hand():
    src = np.arange(256, dtype=np.uint8)
    before = SC.sentinel(96)
    so = np.array([32, SC.SKIP, 0], dtype=np.int64)
    do = np.array([0, 16, 48, 64], dtype=np.int64)
    want = before.copy()
    want[0:16] = src[32:48]
    want[48:64] = src[0:16]
    assert np.array_equal(SC.ref_segcopy(before, src, so, do), want)
    assert np.array_equal(SC.ref_segcopy(before, src, so, do, cap=64), want)
    assert np.array_equal(SC.ref_segcopy(before, src, so, do, cap=48), before)
    assert np.array_equal(SC.ref_segcopy(before, src, so, do, n=1)[16:], before[16:])
    # mode 2: lengths 16 / 0 / 16 in rooms of 16 / 32 / 16, the last one past cap
    so2 = np.array([32, 64, 0], dtype=np.int64)
    ln = np.array([16, 0, 16], dtype=np.int64)
    w2 = before.copy()
    w2[0:16] = src[32:48]
    assert np.array_equal(SC.ref_segcopy(before, src, so2, do, seg_len=ln, cap=63), w2)
    w2[48:64] = src[0:16]
    assert np.array_equal(SC.ref_segcopy(before, src, so2, do, seg_len=ln, cap=64), w2)
    assert before[5] == (5 * 131 + 7) & 255 and SC.sentinel(4, 300)[1] == (301 * 131 + 7) & 255


def test_plan_passes_by_hand():
    # 3000 chunks on 2 workgroups: span = 1536; a 16-B segment every chunk
    off = np.arange(3001, dtype=np.int64) * 16
    p = SC.plan_passes(off, 2, 1024, 1024)
    assert p["span"] == 1536 and len(p["wgs"]) == 2
    a, b = p["wgs"]
    assert (a["r0"], a["r1"], a["ja"], a["jb"], a["starts"]) == (0, 1536, 0, 1535, [0, 1024])
    assert (b["r0"], b["r1"], b["ja"], b["jb"], b["starts"]) == (1536, 3000, 1536, 2999,
                                                                 [1536, 2560])
    assert not a["skip"] and a["head_out"] == 0 and a["tail_out"] == 0
    # one segment of 3000 chunks: both workgroups start and end inside it
    p = SC.plan_passes(np.array([0, 48000]), 2, 1024, 1024)
    a, b = p["wgs"]
    assert a["ja"] == a["jb"] == b["ja"] == b["jb"] == 0
    assert (a["tail_out"], b["head_out"], b["tail_out"]) == (1464, 1536, 0)
    # 4 segments, 6 empty, 2 segments, staged 4 at a time: the second pass starts in the
    # run (index 4), moves to its last member (index 10, which holds bytes) and ends there
    off = np.array([0, 16, 32, 48, 64, 64, 64, 64, 64, 64, 64, 80, 96])
    w = SC.plan_passes(off, 8, 1024, 4)["wgs"]
    assert len(w) == 1 and w[0]["starts"] == [0, 10] and w[0]["skip"] and w[0]["skipped"] == 6
    # fewer chunks than one tile per workgroup: the minimum tile decides
    assert SC.plan_passes(np.array([0, 16 * 2048]), 1000, 1024, 1024)["span"] == 1024
    assert SC.plan_passes(np.array([0, 0, 0]), 4, 1024, 1024)["wgs"] == []


# ---- every small family: coverage on paper, bytes through the host twin ----------------
def _small(stage):
    return SC.small_mode0_cases(np.random.default_rng(40), stage, MIN_TILE)


@pytest.mark.parametrize("stage", STAGES.values(), ids=STAGES.keys())
def test_small_families_reach_their_paths(stage):
    for c in _small(stage):
        for grid in SC.ASSUMED_GRIDS:
            SC.check_coverage(c, grid, MIN_TILE, stage)


@pytest.mark.parametrize("stage", STAGES.values(), ids=STAGES.keys())
def test_small_families_host_twin(stage):
    for c in _small(stage):
        for mode in (0, 3, 7):
            _same(*SC.run_case(c, CPU, mode), f"mode {mode}: {c.description}")
        if not (c.src_off == SC.SKIP).any():
            _same(*SC.run_case(c.sized(), CPU, 2), f"sized: {c.description}")


@pytest.mark.parametrize("grid", SC.ASSUMED_GRIDS)
def test_workgroup_boundary_families(grid):
    rng = np.random.default_rng(41)
    for c in SC.big_mode0_cases(rng, grid, MIN_TILE):
        assert int(c.dst_off[-1]) >= 64 << 20
        for stage in STAGES.values():
            SC.check_coverage(c, grid, MIN_TILE, stage)
        if grid == SC.ASSUMED_GRIDS[-1]:   # the bytes once: the host twin knows no grid
            _same(*SC.run_case(c, CPU, 0), c.description)
            _same(*SC.run_case(c.sized(), CPU, 2), "sized: " + c.description)


def test_sized_family_host_twin():
    stage = SC.TODAY["stage_sized"]
    for c in SC.sized_cases(np.random.default_rng(42), stage, MIN_TILE):
        for grid in SC.ASSUMED_GRIDS:
            SC.check_coverage(c, grid, MIN_TILE, stage)
        got, want = SC.run_case(c, CPU, 2)
        _same(got, want, c.description)
        if c.cap is not None:   # the drop rule did drop, and something was kept
            assert not np.array_equal(want, SC.sentinel(c.dst_bytes)), c.description
            kept_all = SC.ref_segcopy(SC.sentinel(c.dst_bytes), c.src, c.src_off, c.dst_off,
                                      seg_len=c.seg_len)
            assert not np.array_equal(want, kept_all), c.description


def test_sized_drop_rule_by_hand():
    c = SC.sized_cases(np.random.default_rng(42), SC.TODAY["stage_sized"], MIN_TILE)[3]
    _, want = SC.run_case(c, CPU, 2)
    d20 = int(c.dst_off[20])
    s21 = int(c.src_off[21])
    assert c.cap == d20 + 48 and int(c.seg_len[20]) == 64 and int(c.seg_len[21]) == 48
    assert np.array_equal(want[d20:d20 + 48], c.src[s21:s21 + 48])          # the shorter one
    assert np.array_equal(want[d20 + 48:], SC.sentinel(c.dst_bytes)[d20 + 48:])  # all later


# ---- the contract corners --------------------------------------------------------------
def test_host_segcopy_skips_a_gap_segment():
    """src_off == kSegSkip is a gap on the host too (it used to copy from src + ~0)."""
    src = torch.arange(64, dtype=torch.uint8)
    so = torch.tensor([16, SC.SKIP, 0], dtype=torch.int64)
    do = torch.tensor([0, 16, 1 << 20, (1 << 20) + 16], dtype=torch.int64)
    dst = torch.full(((1 << 20) + 32,), 0xAB, dtype=torch.uint8)
    R.segcopy(src, so, do, dst)
    assert torch.equal(dst[:16], src[16:32]) and torch.equal(dst[1 << 20:(1 << 20) + 16], src[:16])
    assert bool((dst[16:1 << 20] == 0xAB).all()) and bool((dst[-16:] == 0xAB).all())
    assert R.SEG_SKIP == SC.SKIP


def test_dst_cap_boundary_host():
    c = SC.skip_mix_case(np.random.default_rng(43))
    total = int(c.dst_off[-1])
    before = SC.sentinel(c.dst_bytes)
    for mode in (0, 3):
        got, want = SC.run_case(c, CPU, mode, cap=total)
        _same(got, want, "cap == total")
        assert not np.array_equal(got, before)
        got, want = SC.run_case(c, CPU, mode, cap=total - 16)
        _same(got, want, "total == cap + 16")
        assert np.array_equal(got, before)


def test_device_count_host():
    c, n_dev = SC.poisoned_count_case(np.random.default_rng(44))
    got, want = SC.run_case(c, CPU, 3, n_dev=n_dev)
    _same(got, want, c.description)
    assert not (got == 0xEE).all() and not np.array_equal(got, SC.sentinel(c.dst_bytes))
    got, want = SC.run_case(c, CPU, 3, n_dev=0)
    _same(got, want, "count 0")
    assert np.array_equal(got, SC.sentinel(c.dst_bytes))


def test_offsets_above_the_gap_shrunk():
    """The two 4 GiB shapes of the GPU suite with a gap of 1 MiB."""
    for run in (SC.run_gap_4g, SC.run_src_4g):
        for what, got, want in run(CPU, gap=1 << 20):
            _same(got, want, f"{run.__name__}: {what}")
            if what in ("head", "tail", "source offsets above the gap"):
                assert not np.array_equal(got, SC.sentinel(got.size, 0)), what
