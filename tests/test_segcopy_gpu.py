"""k_segcopy, the byte mover under every GET, SET, CLOCK staging copy and routed pack, in
each of its modes against the NumPy model of tests/segcopy_cases.py. GPU only.

Every case asserts from ``plan_passes``, fed with ``segcopy_geometry()`` of this device,
that it reaches the path it is named for (a second staging pass, the skip over an empty
run, a workgroup boundary inside a segment, ...), then compares the whole destination,
sentinel-filled beforehand, byte for byte. Mode 0 cases run through mode 3 (the count in a
device word) and ``gather_segments`` (absolute addresses) too; mode 2 has its own family;
the LDS-DMA variant runs in a child process; mode 1 is checked through the log image a SET
batch leaves."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from shellac_amd.ops import routing as R
from shellac_amd.ops.cache import (ITEM_HEADER_BYTES, ITEM_MAGIC, CacheShard, digest_strings,
                                   item_bytes, pack_values)

import segcopy_cases as SC

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def geom(core):
    assert torch.cuda.is_available(), "GPU test scheduled on a machine without a GPU"
    torch.cuda.set_device(0)
    g = core.segcopy_geometry()
    print(f"\nsegcopy geometry: {g}")
    return g


def _check(case, dev, geom, mode, **kw):
    """Coverage from plan_passes on this device's grid, then the bytes."""
    grid, min_tile, tsc = SC.geometry_for(geom, 0 if mode == 7 else mode)
    plan = SC.check_coverage(case, grid, min_tile, tsc)
    got, want = SC.run_case(case, dev, mode, **kw)
    bad = SC.first_diff(got, want)
    print(f"mode {mode} {case.description}: {SC.plan_summary(plan)}")
    assert not bad, f"mode {mode}: {case.description}: {bad}"
    return got


FAMILIES = {
    "degenerate": lambda rng, T, mt: SC.degenerate_cases(rng, T),
    "pass_count": lambda rng, T, mt: SC.pass_count_cases(rng, T),
    "empty_run": SC.empty_run_cases,
    "gap_mix": lambda rng, T, mt: [SC.skip_mix_case(rng)],
}


@pytest.mark.parametrize("family", FAMILIES)
def test_small_families_gather(cuda_dev, geom, family):
    """Families 1-3 and the gap mix, each within one minimum tile: mode 0, mode 3 and
    gather_segments on the same arrays."""
    cases = FAMILIES[family](np.random.default_rng(40), geom["stage"], geom["min_tile"])
    for c in cases:
        for mode in (0, 3, 7):
            _check(c, cuda_dev, geom, mode)


@pytest.mark.parametrize("family", ["degenerate", "pass_count", "empty_run"])
def test_small_families_sized(cuda_dev, geom, family):
    """The same shapes built for mode 2's staged count, every length its whole room."""
    cases = FAMILIES[family](np.random.default_rng(40), geom["stage_sized"], geom["min_tile"])
    for c in cases:
        _check(c.sized(), cuda_dev, geom, 2)


@pytest.mark.parametrize("which", [0, 1], ids=["one_48MiB_segment", "built_boundaries"])
def test_workgroup_boundaries(cuda_dev, geom, which):
    """65 MiB: the span exceeds the minimum tile; workgroups that start and end inside one
    segment, and boundaries on the first / last chunk of a segment and on a segment start."""
    for mode in (0, 3, 2):
        grid, min_tile, _ = SC.geometry_for(geom, mode)   # the boundaries follow the mode's grid
        c = SC.big_mode0_cases(np.random.default_rng(41), grid, min_tile)[which]
        if which == 1:
            assert {"head_out_1", "tail_out_1", "aligned"} <= set(c.expect), (grid, c.expect)
        _check(c.sized() if mode == 2 else c, cuda_dev, geom, mode)


def test_sized_family(cuda_dev, geom):
    """Mode 2: gaps of 16 B - 64 KiB, lengths of 0 and of the whole room, a segment ending
    exactly at cap (kept), one ending at cap + 16 (dropped) before a shorter one that fits
    (kept), a dropped segment across a workgroup boundary."""
    for c in SC.sized_cases(np.random.default_rng(42), geom["stage_sized"], geom["min_tile"]):
        got = _check(c, cuda_dev, geom, 2)
        if c.cap is not None:
            assert not np.array_equal(got, SC.sentinel(c.dst_bytes)), c.description


def test_dst_cap_boundary(cuda_dev, geom):
    c = SC.skip_mix_case(np.random.default_rng(43))
    total = int(c.dst_off[-1])
    before = SC.sentinel(c.dst_bytes)
    for mode in (0, 3):
        got = _check(c, cuda_dev, geom, mode, cap=total)          # total == cap: copies
        assert not np.array_equal(got, before)
        got = _check(c, cuda_dev, geom, mode, cap=total - 16)     # total == cap + 16: nothing
        assert np.array_equal(got, before)


def test_device_count(cuda_dev, geom):
    """Mode 3 reads its count on the device: 0 moves nothing, and the entries past a count
    smaller than the arrays (decreasing offsets, sources of another byte) never show."""
    c, n_dev = SC.poisoned_count_case(np.random.default_rng(44))
    got, want = SC.run_case(c, cuda_dev, 3, n_dev=n_dev)
    assert not SC.first_diff(got, want), SC.first_diff(got, want)
    assert not np.array_equal(got, SC.sentinel(c.dst_bytes))
    got, want = SC.run_case(c, cuda_dev, 3, n_dev=0)
    assert np.array_equal(got, SC.sentinel(c.dst_bytes)) and np.array_equal(got, want)


def test_absolute_addresses_from_three_tensors(cuda_dev):
    """gather_segments out of three tensors, one of them the destination's neighbour in the
    same allocation."""
    rng = np.random.default_rng(45)
    blk = 1 << 15
    parts = [SC._src(rng, blk) for _ in range(3)]
    sizes = rng.integers(0, 40, size=300) * 16
    dst_off = np.zeros(301, dtype=np.int64)
    np.cumsum(sizes, out=dst_off[1:])
    nbytes = int(dst_off[-1]) + SC.SLACK
    alloc = torch.empty(nbytes + blk, dtype=torch.uint8, device=cuda_dev)
    dst, neighbour = alloc[:nbytes], alloc[nbytes:]
    tens = [torch.from_numpy(parts[0]).to(cuda_dev), torch.from_numpy(parts[1]).to(cuda_dev),
            neighbour]
    neighbour.copy_(torch.from_numpy(parts[2]))
    which = rng.integers(0, 3, size=300)
    inner = rng.integers(0, (blk - 640) // 16, size=300) * 16
    addrs = np.array([tens[w].data_ptr() + o for w, o in zip(which, inner)], dtype=np.int64)
    before = SC.sentinel(nbytes)
    dst.copy_(torch.from_numpy(before))
    R.gather_segments(torch.from_numpy(addrs).to(cuda_dev), torch.from_numpy(dst_off).to(cuda_dev),
                      dst)
    want = SC.ref_segcopy(before, np.concatenate(parts), which * blk + inner, dst_off)
    assert not SC.first_diff(dst.cpu().numpy(), want), SC.first_diff(dst.cpu().numpy(), want)
    assert np.array_equal(neighbour.cpu().numpy(), parts[2])


def _room_for_4g(dev):
    free = torch.cuda.mem_get_info(dev)[0]
    if free < (12 << 30):
        pytest.skip(f"{free >> 20} MiB of HBM free, the 4 GiB shapes need 12 GiB")


def test_gap_of_4gib_destination_offsets_above_2_32(cuda_dev):
    """A 4 GiB kSegSkip segment before the last segments: their destination offsets are
    above 2^32; the gap's bytes (three 64 KiB windows of it) stay as they were."""
    _room_for_4g(cuda_dev)
    for what, got, want in SC.run_gap_4g(cuda_dev):
        assert not SC.first_diff(got, want), f"{what}: {SC.first_diff(got, want)}"
    torch.cuda.empty_cache()


def test_source_offsets_above_2_32(cuda_dev):
    _room_for_4g(cuda_dev)
    for what, got, want in SC.run_src_4g(cuda_dev):
        assert not SC.first_diff(got, want), f"{what}: {SC.first_diff(got, want)}"
    torch.cuda.empty_cache()


def test_lds_dma_variant_in_a_child_process():
    """SHELLAC_GLDS=1 is read once per process: a fresh interpreter runs the mode-0 families
    1-5, built for the variant's staged count, against the model and exits non-zero on the
    first mismatch."""
    env = dict(os.environ, SHELLAC_GLDS="1", SHELLAC_NO_AUTOBUILD="1")
    p = subprocess.run([sys.executable, "-m", "tests.segcopy_cases", "--device"], cwd=ROOT,
                       env=env, capture_output=True, text=True, timeout=240)
    print(p.stdout[-6000:], p.stderr[-3000:])
    assert p.returncode == 0, (p.returncode, p.stdout[-2000:], p.stderr[-2000:])
    assert p.stdout.startswith("glds True"), p.stdout[:200]
    assert "FAIL" not in p.stdout


def test_append_image_in_the_log(cuda_dev):
    """Mode 1, the SET append: after each batch the records' physical range is copied out of
    the log (gather_segments from log_ptr + P % cap, P = the head before the store plus the
    running sum of item_bytes) and compared with the records built in NumPy: the 32-byte
    header {digest lo, hi, vlen, flags, expire, magic}, then the value. The pad up to the
    16-byte boundary is not compared: the kernel copies whole 16-byte chunks of the value
    buffer and defines no pad of its own (item_bytes only reserves the room). A record that
    starts below cap runs on into the slack past it, contiguous. Rows that store nothing
    (SKIP_VLEN, a value above max_item, the earlier of two rows with one key) must not
    shift the others. Batches stay above 256 rows: smaller ones take the fused small-SET
    kernel, not the byte mover."""
    from shellac_amd.models.batch import SKIP_VLEN

    cap, max_item = 1 << 20, 4096
    shard = CacheShard(cap, 1 << 12, max_item, cuda_dev)
    log_ptr = int(shard._impl.log_ptr)
    rng = np.random.default_rng(46)
    straddled, batch = 0, 0
    while shard.head() <= 2 * cap:
        n = 300
        lens = rng.integers(0, 3301, size=n)
        lens[7] = 5000                       # above max_item: no record
        lens[11], lens[12] = 0, 1            # the shortest records
        keys = [b"/append/%d/%d" % (batch, i) for i in range(n)]
        keys[40] = keys[250]                 # one key twice: the later row wins, row 40 stores nothing
        skip = np.zeros(n, dtype=bool)
        skip[[3, 100, 299]] = True
        # records just under cap / 2: trim the longest values until the bound holds
        while CacheShard.payload_bound(n, int(((lens + 15) & ~15).sum()) + 16) > cap // 2:
            lens[np.argsort(lens)[-2]] //= 2   # ([-1] is the row above max_item)
        vals = [rng.bytes(int(l)) for l in lens]
        d = digest_strings(keys)
        v, vo, vl = pack_values(vals)
        vl[torch.from_numpy(skip)] = SKIP_VLEN
        fl = torch.from_numpy(rng.integers(0, 1 << 31, size=n).astype(np.int32))
        ex = torch.from_numpy(rng.integers(0, 1 << 31, size=n).astype(np.int32))
        head = shard.head()
        shard.store(d.to(cuda_dev), v.to(cuda_dev), vo.to(cuda_dev), vl.to(cuda_dev),
                    fl.to(cuda_dev), ex.to(cuda_dev), now=5)
        stored = [i for i in range(n) if not skip[i] and lens[i] <= max_item and i != 40]
        sizes = np.array([item_bytes(int(lens[i])) for i in stored], dtype=np.int64)
        off = np.zeros(len(stored) + 1, dtype=np.int64)
        np.cumsum(sizes, out=off[1:])
        assert shard.head() == head + int(off[-1]), (batch, shard.head(), head, int(off[-1]))
        phys = (head + off[:-1]) % cap
        straddled += int(((phys + sizes) > cap).sum())
        img = torch.zeros(int(off[-1]), dtype=torch.uint8, device=cuda_dev)
        R.gather_segments(torch.from_numpy(phys + log_ptr).to(cuda_dev),
                          torch.from_numpy(off).to(cuda_dev), img)
        img = img.cpu().numpy()
        dn = d.numpy()
        for k, i in enumerate(stored):
            hdr = np.zeros(ITEM_HEADER_BYTES, dtype=np.uint8)
            hdr[0:16] = dn[i].view(np.uint8)
            hdr[16:32] = np.array([int(lens[i]), int(fl[i]), int(ex[i]), ITEM_MAGIC],
                                  dtype=np.uint32).view(np.uint8)
            want = np.concatenate([hdr, np.frombuffer(vals[i], dtype=np.uint8)])
            got = img[off[k]:off[k] + want.size]
            assert np.array_equal(got, want), (batch, i, SC.first_diff(got, want))
        batch += 1
    assert batch >= 4 and straddled >= 1, (batch, straddled)
