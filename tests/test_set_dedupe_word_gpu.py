"""The SET chain's one-word dedupe table (a slot is 0 or the key's last row + 1, the key read
through that row) against the host engine given the same batches: afterwards a GET of every
key returns the same value on both, and the SET counters are equal. Every batch has more
than 256 rows, so it takes the kernel chain and not the fused small-batch kernel. GPU only."""
import numpy as np
import pytest
import torch

from shellac_amd.ops.cache import CacheShard, digest_strings, pack_values, unpack_records

pytestmark = pytest.mark.gpu

NOW = 10
MAX_ITEM = 1 << 12


class Pair:
    """A GPU shard and its host twin, fed the same batches."""

    def __init__(self, dev):
        self.dev = dev
        self.g = CacheShard(1 << 24, 1 << 12, MAX_ITEM, dev)
        self.h = CacheShard(1 << 24, 1 << 12, MAX_ITEM, "cpu")

    def store(self, keys, vals):
        assert len(keys) > 256
        d = digest_strings(keys)
        v, vo, vl = pack_values(vals)
        self.g.store(d.to(self.dev), v.to(self.dev), vo.to(self.dev), vl.to(self.dev), now=NOW)
        self.h.store(d, v, vo, vl, now=NOW)

    def check(self, keys):
        """Every key: the same answer on both engines (returned: the GPU's values)."""
        d = digest_strings(keys)
        og, fg, sg = self.g.get(d.to(self.dev), now=NOW)
        oh, fh, sh = self.h.get(d, now=NOW)
        assert torch.equal(sg.cpu(), sh)
        rg, rh = unpack_records(og, fg, sg), unpack_records(oh, fh, sh)
        assert rg == rh
        cg, ch = self.g.counters(), self.h.counters()
        for k in ("set_ops", "set_dropped", "set_bytes"):
            assert cg[k] == ch[k], (k, cg[k], ch[k])
        return [None if r is None else r[0] for r in rg]


def _vals(rng, n, lo=1, hi=600):
    return [rng.integers(0, 256, size=int(rng.integers(lo, hi)), dtype=np.uint8).tobytes()
            for _ in range(n)]


def test_distinct_keys_fill_half_of_a_fresh_table(cuda_dev):
    """1000 distinct keys in a fresh 1024-row workspace: 2048 slots at ~49 % load, so rows
    meet slots other keys own and walk on."""
    p = Pair(cuda_dev)
    rng = np.random.default_rng(1)
    keys = [b"/d/%d" % i for i in range(1000)]
    vals = _vals(rng, 1000)
    p.store(keys, vals)
    assert p.check(keys + [b"/d/none"]) == vals + [None]
    assert p.g.counters()["set_dropped"] == 0


def test_last_of_three_rows_in_three_workgroups_wins(cuda_dev):
    p = Pair(cuda_dev)
    rng = np.random.default_rng(2)
    keys = [b"/t/%d" % i for i in range(1000)]
    vals = _vals(rng, 1000)
    for r in (3, 300, 900):
        keys[r] = b"/t/same"
    vals[3], vals[300], vals[900] = b"a" * 40, b"b" * 50, b"c" * 60
    p.store(keys, vals)
    got = p.check(keys)
    assert got[3] == got[300] == got[900] == b"c" * 60
    assert p.g.counters()["set_dropped"] == 2


def test_every_key_twice(cuda_dev):
    p = Pair(cuda_dev)
    rng = np.random.default_rng(3)
    base = [b"/w/%d" % i for i in range(400)]
    order = rng.permutation(800)
    keys = [base[j % 400] for j in order]
    vals = _vals(rng, 800)
    p.store(keys, vals)
    last = {}
    for k, v in zip(keys, vals):
        last[k] = v
    assert p.check(base) == [last[k] for k in base]
    assert p.g.counters()["set_dropped"] == 400


def test_three_batches_leave_the_table_clean(cuda_dev):
    """Keys A, then disjoint keys B, then A again with new values: every row resets its slot,
    so no batch meets a word of the one before."""
    p = Pair(cuda_dev)
    rng = np.random.default_rng(4)
    a = [b"/a/%d" % i for i in range(700)]
    b = [b"/b/%d" % i for i in range(700)]
    va, vb, va2 = _vals(rng, 700), _vals(rng, 700), _vals(rng, 700)
    p.store(a, va)
    p.store(b, vb)
    p.store(a, va2)
    assert p.check(a + b) == va2 + vb
    assert p.g.counters()["set_dropped"] == 0


def test_oversized_last_writer(cuda_dev):
    """A row above max_item whose key also has an earlier valid row: the host engine decides
    whether the oversized last writer shadows it."""
    p = Pair(cuda_dev)
    rng = np.random.default_rng(5)
    keys = [b"/o/%d" % i for i in range(600)]
    vals = _vals(rng, 600)
    keys[500] = keys[20]
    vals[500] = b"x" * (MAX_ITEM + 16)
    keys[40] = keys[450]                 # and the other order: oversized first, valid last
    vals[40] = b"y" * (MAX_ITEM + 1)
    p.store(keys, vals)
    got = p.check(keys)
    assert got[450] == vals[450]
