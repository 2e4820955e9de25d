"""The one-GPU step's blocked GET path — packed lookup rows (offset << 21 | bytes), the
prefix of the lookup workgroups' totals, the gather's expand tail and its dense clear of
the coalescing table — against the uncoalesced step on a twin shard: every request's size
and record bytes. GPU only."""
import numpy as np
import pytest
import torch

from shellac_amd.models.batch import SetBatch
from shellac_amd.models.sharded_cache import ShardedCache
from shellac_amd.ops.cache import CacheShard, digest_strings, item_bytes, pack_values

pytestmark = pytest.mark.gpu

NOW = 10
PRESENT, ABSENT = 200, 50


def _set_batch(keys, vals, dev):
    v, vo, vl = pack_values(vals, dev)
    return SetBatch(digest_strings(keys).to(dev), v, vo, vl)


class Twins:
    """Two shards with the same content behind two steps: uncoalesced (the reference) and
    coalesced (the blocked path under test)."""

    def __init__(self, dev, keys, vals, max_item=1 << 16, log=64 << 20):
        self.dev = dev
        self.steps = []
        for co in (False, True):
            sc = ShardedCache(CacheShard(log, 1 << 12, max_item, dev))
            sc.coalesce = co
            sc.set(_set_batch(keys, vals, dev), now=NOW)
            self.steps.append(sc)
        self.ref, self.co = self.steps
        self.nset = 0

    def side_batch(self):
        """A small SET batch of keys no GET asks for (a step serves GETs before SETs)."""
        k = self.nset = self.nset + 1
        return _set_batch([b"/side/%d/%d" % (k, i) for i in range(16)],
                          [b"s%d" % i * 5 for i in range(16)], self.dev)

    def serve_both(self, keys):
        b = self.side_batch()
        out = [sc.serve(keys, b, now=NOW).wait() for sc in self.steps]
        torch.cuda.synchronize()
        return out


def _words(res, width):
    """Request i's record as `width` 8-byte words (zero past its size), and the sizes."""
    size = res.size.to(torch.int64)
    assert int(size.max()) <= width * 8 and int((size & 15).max()) == 0
    data = res.data
    pad = (-data.numel()) % 8
    if pad:
        data = torch.cat([data, data.new_zeros(pad)])
    w = data.view(torch.int64)
    col = torch.arange(width, device=size.device)
    live = col[None, :] < (size[:, None] >> 3)
    idx = torch.where(live, (res.off.to(torch.int64)[:, None] >> 3) + col[None, :], 0)
    return torch.where(live, w[idx], 0), size


def assert_same(ref, got, max_bytes):
    """Every request: the same size and the same record bytes."""
    width = max_bytes // 8
    assert ref.size.numel() == got.size.numel()
    n, step = ref.size.numel(), max(1, (1 << 27) // (width * 8))
    for s in range(0, n, step):   # bounded temporaries for a wide or a long batch
        part = [type(r)(r.data, r.off[s:s + step], r.size[s:s + step]) for r in (ref, got)]
        (wr, sr), (wg, sg) = _words(part[0], width), _words(part[1], width)
        assert torch.equal(sr, sg)
        assert torch.equal(wr, wg)


def _table_zero(sc):
    return sc._co_table is not None and int(sc._co_table.abs().sum()) == 0


@pytest.fixture(scope="module")
def pool():
    """~200 present keys with 64..~1900-byte values and ~50 absent ones, on twin shards."""
    if not torch.cuda.is_available():
        pytest.fail("GPU test scheduled on a machine without a GPU")
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(7)
    keys = [b"/p/%d" % i for i in range(PRESENT)]
    vals = [rng.integers(0, 256, size=64 + 9 * i, dtype=np.uint8).tobytes()
            for i in range(PRESENT)]
    tw = Twins(dev, keys, vals)
    tw.present = digest_strings(keys).to(dev)
    tw.absent = digest_strings([b"/absent/%d" % i for i in range(ABSENT)]).to(dev)
    tw.max_bytes = int(item_bytes(64 + 9 * (PRESENT - 1)))
    return tw


def _mixed(tw, n, seed):
    g = torch.Generator().manual_seed(seed)
    both = torch.cat([tw.present, tw.absent])
    return both.index_select(0, torch.randint(0, both.shape[0], (n,), generator=g).to(tw.dev))


@pytest.mark.parametrize("n", [1, 1023, 1024, 1025, 3000])
def test_duplicates_and_misses_across_lookup_workgroups(pool, n):
    keys = _mixed(pool, n, n)
    ref, got = pool.serve_both(keys)
    assert_same(ref, got, pool.max_bytes)
    assert bool((ref.size > 0).any()) or n == 1
    assert _table_zero(pool.co)


def test_all_miss_block(pool):
    """Rows 1024-2047 (the whole second lookup workgroup) are absent keys: two equal block
    prefixes, and a run of 1024 empty segments inside the response."""
    keys = _mixed(pool, 3000, 11)
    g = torch.Generator().manual_seed(12)
    keys[1024:2048] = pool.absent.index_select(
        0, torch.randint(0, ABSENT, (1024,), generator=g).to(pool.dev))
    ref, got = pool.serve_both(keys)
    assert int(ref.size[1024:2048].sum()) == 0 and int(ref.size[2048:].sum()) > 0
    assert_same(ref, got, pool.max_bytes)
    assert _table_zero(pool.co)


def test_table_reuse_with_disjoint_key_sets(pool):
    """Two consecutive steps whose key sets share nothing: the second finds no claim of the
    first in the table."""
    half = PRESENT // 2
    for lo, seed in ((0, 21), (half, 22)):
        g = torch.Generator().manual_seed(seed)
        ids = torch.randint(lo, lo + half, (2500,), generator=g).to(pool.dev)
        ref, got = pool.serve_both(pool.present.index_select(0, ids))
        assert int((ref.size == 0).sum()) == 0
        assert_same(ref, got, pool.max_bytes)


def test_first_step_and_outgrown_capacity(cuda_dev):
    """A step with no remembered response capacity, and one whose remembered capacity is 16
    bytes (the gather runs twice, its tail too): right answers, and the step's table is all
    zero after each."""
    rng = np.random.default_rng(3)
    keys = [b"/r/%d" % i for i in range(64)]
    vals = [rng.integers(0, 256, size=100 + i, dtype=np.uint8).tobytes() for i in range(64)]
    tw = Twins(cuda_dev, keys, vals)
    d = digest_strings(keys + [b"/r/none"]).to(cuda_dev)
    g = torch.Generator().manual_seed(5)
    req = d.index_select(0, torch.randint(0, 65, (2100,), generator=g).to(cuda_dev))
    width = int(item_bytes(163))
    ref, got = tw.serve_both(req)            # first step
    assert_same(ref, got, width)
    assert _table_zero(tw.co)
    for sc in tw.steps:
        sc._local_step._gather_cap = 16      # outgrown: the retry path
    ref2, got2 = tw.serve_both(req)
    assert_same(ref2, got2, width)
    assert torch.equal(ref2.size, ref.size) and int(ref.size.sum()) > 16
    assert _table_zero(tw.co)
    ref3, got3 = tw.serve_both(req)          # and the step after a retry
    assert_same(ref3, got3, width)
    assert _table_zero(tw.co)


def test_size_field_holds_a_max_item_record(cuda_dev):
    """One value of exactly max_item bytes (1 MiB: bit 20 of the packed 21-bit size field)
    among 64-byte values."""
    max_item = 1 << 20
    rng = np.random.default_rng(4)
    keys = [b"/m/%d" % i for i in range(40)]
    vals = [rng.integers(0, 256, size=64, dtype=np.uint8).tobytes() for _ in keys]
    vals[17] = rng.integers(0, 256, size=max_item, dtype=np.uint8).tobytes()
    tw = Twins(cuda_dev, keys, vals, max_item=max_item)
    d = digest_strings(keys).to(cuda_dev)
    g = torch.Generator().manual_seed(6)
    ids = torch.randint(0, 40, (1500,), generator=g)
    ids[3], ids[1400] = 17, 17
    ref, got = tw.serve_both(d.index_select(0, ids.to(cuda_dev)))
    assert int(ref.size[3]) == int(item_bytes(max_item)) == max_item + 32
    assert_same(ref, got, int(item_bytes(max_item)))
    assert _table_zero(tw.co)


def test_two_rows_of_chunks_per_lookup_workgroup(pool):
    """n = 2048 * 1024 + 1025: more 1024-key chunks than lookup workgroups, so each takes two
    (row shift 11) and the last one a partial chunk."""
    n = 2048 * 1024 + 1025
    g = torch.Generator().manual_seed(31)
    ids = torch.randint(0, 24, (n,), generator=g).to(pool.dev)
    few = torch.cat([pool.present[:20], pool.absent[:4]])
    keys = few.index_select(0, ids)
    ref, got = pool.serve_both(keys)
    assert_same(ref, got, int(item_bytes(64 + 9 * 19)))
    assert _table_zero(pool.co)
    # the blocked lookup itself: its row shift, and the total its gather publishes
    sh = pool.co.shard
    table = torch.zeros_like(pool.co._co_table)
    lk, first, cslot = sh.lookup_coalesced(keys, NOW, table=table, blocked=True)
    assert lk.shift == 11 and lk.size is None and cslot is None
    osz, ooff = (torch.empty(n, dtype=torch.int64, device=pool.dev) for _ in range(2))
    out = torch.empty(1 << 20, dtype=torch.uint8, device=pool.dev)
    sh.gather(lk, out, expand=(first, osz, ooff, table, cslot))
    assert torch.equal(osz, ref.size.to(torch.int64))
    distinct = torch.unique(ids)
    assert int(lk.total()) == int(sum(int(ref.size[ids == k][0]) for k in distinct.tolist()))
    assert int(table.abs().sum()) == 0
