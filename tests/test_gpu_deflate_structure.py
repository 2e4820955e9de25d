"""Structure of what the GPU deflate kernels (k_lz77, k_plan, k_slot_scan, k_emit in
csrc/deflate.hip) write, read back bit by bit with tests/deflate_ref.py. zlib accepts any
legal stream, so a round trip alone cannot see a match that reaches into the block before,
a missing sync-flush marker, a device plan that differs from the host planner's, k_emit
disagreeing with the host emitter, or output that depends on the batch around a body.

Every comparison is exact. Per body: zlib gives it back; every block decodes with an empty
window; one data block per 32 KiB, BFINAL on the last only, the empty stored block after
every non-final Huffman block, no block larger than its stored encoding; and the host
emitter ``deflate_tokens_cpu`` (same planner, compiled for the host) turns the traced
tokens of each block into exactly the GPU's bytes."""
import functools
import random
import zlib

import pytest

import deflate_ref as ref
from inflate_cases import html

pytestmark = pytest.mark.gpu

BLOCK = 32768
SIZES = (list(range(71)) + [127, 128, 129] + list(range(255, 260)) + [4095, 4096, 4097]
         + [32767, 32768, 32769] + [65535, 65536, 65537] + [3 * BLOCK])
PERIODS = (1, 2, 3, 4, 63, 64, 65, 257, 258, 259)
KINDS = ["random", "run", "two", "fib", "deep", "all256", "html"] + [f"period{p}" for p in PERIODS]


@functools.lru_cache(None)
def fib_block():
    """A full block of literals with Fibonacci counts (1, 1, 2, 3, ... over 21 symbols, the
    rest shared by three more): an unlimited Huffman code would be 20 bits deep, so the
    planner has to apply the 15-bit limit."""
    fib = [1, 1]
    while len(fib) < 21:
        fib.append(fib[-1] + fib[-2])
    rest = BLOCK - sum(fib)
    counts = fib + [rest // 3, rest // 3, rest - 2 * (rest // 3)]
    out = bytearray()
    for s, c in enumerate(counts):
        out += bytes([40 + s]) * c
    random.Random(13).shuffle(out)
    assert len(out) == BLOCK
    return bytes(out)


@functools.lru_cache(None)
def deep_block():
    """A full block that provably needs the length limit. Literal counts 1, 2, 3, 5, ...,
    144 continue the end-of-block symbol's count of 1 as a Fibonacci sequence, so every
    Huffman merge adds one level to the rarest codes (11 levels); the other 32392 bytes are
    spread evenly over 200 more symbols, a balanced tree 6 to 7 levels deep on top of that.
    No 4-byte word occurs twice, so k_lz77 can find no match and the histogram k_plan sees
    is exactly these counts: the unlimited code is 17 bits deep."""
    fib = [1, 2]
    while len(fib) < 11:
        fib.append(fib[-1] + fib[-2])
    rest = BLOCK - sum(fib)
    counts = fib + [rest // 200 + (1 if k < rest % 200 else 0) for k in range(200)]
    pool = bytearray()
    for s, c in enumerate(counts):
        pool += bytes([s]) * c
    for seed in range(100):
        out = bytearray(pool)
        random.Random(seed).shuffle(out)
        if len({bytes(out[i:i + 4]) for i in range(BLOCK - 3)}) == BLOCK - 3:
            break
    else:
        raise AssertionError("no shuffle without a repeated 4-byte word")
    freq = [0] * 286
    for s, c in enumerate(counts):
        freq[s] = c
    freq[256] = 1
    assert max(ref.huffman_lengths(freq, 40)) == 17
    return bytes(out)


def body(kind, n):
    rng = random.Random(f"{kind}/{n}")
    if kind == "random":
        return rng.randbytes(n)
    if kind == "run":
        return bytes([rng.randrange(256)]) * n
    if kind == "two":
        return bytes(rng.choice(b"<>") for _ in range(n))
    if kind == "fib":
        return (fib_block() * (n // BLOCK + 1))[:n]
    if kind == "deep":
        return (deep_block() * (n // BLOCK + 1))[:n]
    if kind == "all256":
        p = list(range(256))
        rng.shuffle(p)
        return (bytes(p) * (n // 256 + 1))[:n]
    if kind == "html":
        return html(rng, n)
    p = rng.randbytes(int(kind[6:]))
    return (p * (n // len(p) + 1))[:n]


@pytest.fixture
def gz(cuda_dev):
    from shellac_amd.ops.gzip import engine

    return engine(cuda_dev.index or 0)


def tok32(t):
    return t if isinstance(t, int) else 0x80000000 | (t[0] << 16) | (t[1] - 1)


def check_structure(core, raw, data):
    """Checks 1-4 of the module docstring for one raw stream; returns its traced data
    blocks (the sync-flush markers left out)."""
    assert zlib.decompress(raw, -15) == data
    blocks = ref.trace(raw, empty_window=True)  # raises if a match leaves its block
    nblk = max(1, -(-len(data) // BLOCK))
    i, out = 0, []
    for j in range(nblk):
        part = data[j * BLOCK:(j + 1) * BLOCK]
        fin = j == nblk - 1
        b = blocks[i]
        i += 1
        assert b.start_bit % 8 == 0 and b.data == part and b.final == fin, (j, b)
        end = -(-b.end_bit // 8)
        if b.btype != 0 and not fin:  # the sync-flush marker: an empty stored block
            mark = blocks[i]
            i += 1
            assert mark.btype == 0 and mark.data == b"" and not mark.final, (j, mark)
            assert mark.start_bit == b.end_bit
            end = mark.end_bit // 8
            assert raw[end - 4:end] == b"\0\0\xff\xff"
        mine = raw[b.start_bit // 8:end]
        assert len(mine) <= 5 + len(part), (j, b)
        if b.btype == 0:
            n = len(part)
            assert mine == bytes([1 if fin else 0]) + n.to_bytes(2, "little") + \
                (n ^ 0xFFFF).to_bytes(2, "little") + part, (j, b)
        else:
            host = core.deflate_tokens_cpu([tok32(t) for t in b.tokens], part, fin)
            assert host == mine, f"block {j} ({b}): host emitter {len(host)} B, GPU {len(mine)} B"
        out.append(b)
    assert i == len(blocks) and end == len(raw), "blocks or bytes after the last data block"
    return out


@pytest.mark.parametrize("kind", KINDS)
def test_corpus_structure(gz, core, kind):
    bodies = [body(kind, n) for n in SIZES]
    raws = gz.deflate(bodies)
    members = gz.compress(bodies)
    deepest = 0
    for data, raw, m in zip(bodies, raws, members):
        assert m[:10] == b"\x1f\x8b\x08\0\0\0\0\0\0\xff" and m[10:-8] == raw, len(data)
        assert zlib.decompress(m, 31) == data
        for b in check_structure(core, raw, data):
            if b.btype == 2:
                deepest = max(deepest, max(b.ll_lens))
    if kind == "deep":
        assert deepest == 15, "the planner on the device did not apply the length limit"


def test_matches_do_not_reach_across_blocks(gz, core):
    """The same 1000 random bytes at offset 0 and near offset 31700 of one block, and on
    both sides of a 32 KiB boundary: the second copy may be matched only inside its own
    block (and not at all across the boundary)."""
    rng = random.Random(17)
    rep = rng.randbytes(1000)
    fill = bytes(rng.choice(b"0123456789abcdef") for _ in range(2 * BLOCK))
    one = rep + fill[:30700] + rep + fill[:68]
    assert len(one) == BLOCK
    two = fill[:BLOCK - 1000] + rep + rep + fill[:5000]
    edge = fill[:BLOCK - 500] + rep + fill[:3000]  # one copy, cut by the boundary
    raws = gz.deflate([one, two, edge, one + one])
    far = 0
    for data, raw in zip((one, two, edge, one + one), raws):
        for b in check_structure(core, raw, data):
            far = max([far] + [d for _, d in (t for t in (b.tokens or []) if not isinstance(t, int))])
    assert far >= 31700  # the second copy in `one` was found in its own block


def coverage_bodies():
    """Full blocks over a 64-symbol alphabet with planted matches of every length symbol's
    first length and distances from every distance symbol. A match cannot cross its lane's
    512-byte segment, so every plant starts at a segment start and ends inside it; far
    distances get several plants, since the parse looks at 12 chain candidates only."""
    rng = random.Random(19)
    lengths = [l for l in ref.LBASE if l >= 4] + [130, 257]
    bodies, li = [], 0
    for blk in range(3):
        buf = bytearray(rng.randrange(32, 96) for _ in range(BLOCK))
        need = {ds: 3 if ds >= 27 else 2 for ds in range(30)}  # 63 plants, one per segment
        plan = {}
        for s in range(63, 0, -1):
            fits = [ds for ds in range(30) if ref.DBASE[ds] <= 512 * s and need[ds] > 0]
            if fits:
                plan[s] = max(fits)
                need[plan[s]] -= 1
        for s in sorted(plan):
            p, ds = 512 * s, plan[s]
            top = min(512 * s, ref.DBASE[ds] + (1 << ref.DEXT[ds]) - 1, 32767)
            dist = rng.choice((ref.DBASE[ds], top))
            length = lengths[li % len(lengths)]
            li += 1
            for k in range(length):
                buf[p + k] = buf[p + k - dist]
            if buf[p + length] == buf[p + length - dist]:
                buf[p + length] ^= 1  # the match ends where the plant ends
        bodies.append(bytes(buf))
    return bodies


def test_symbol_coverage(gz, core):
    """Over planted full blocks and low-entropy text the traces show every distance
    symbol 0..29 and every length symbol 258..285. Length symbol 257 (a 3-byte match)
    cannot come out of k_lz77: a candidate enters a position's hash chain only with the
    same hash of its 4-byte word, two words with the same first 3 bytes differ in the top
    byte, and the multiplicative hash (odd multiplier, top 12 bits kept) maps those to
    different buckets; a match cut by the end of a lane's segment is not searched for
    unless 4 bytes remain. So every match k_lz77 emits has 4 bytes or more."""
    rng = random.Random(23)
    bodies = coverage_bodies() + [bytes(rng.choice(b"0123456789abcdef") for _ in range(BLOCK)),
                                  html(rng, BLOCK), body("two", BLOCK)]
    lsyms, dsyms = set(), set()
    for data, raw in zip(bodies, gz.deflate(bodies)):
        for b in check_structure(core, raw, data):
            for t in b.tokens or []:
                if not isinstance(t, int):
                    lsyms.add(ref.len_symbol(t[0])[0])
                    dsyms.add(ref.dist_symbol(t[1])[0])
    assert set(range(30)) - dsyms == set(), "distance symbols never emitted"
    assert set(range(258, 286)) - lsyms == set(), "length symbols never emitted"


def test_batch_invariance(gz):
    """A body's bytes do not depend on its position in a batch, on its neighbours, or on
    what the grow-only staging buffers held before."""
    picks = [body(k, n) for k in KINDS for n in (0, 1, 63, 259, 4097, 32769)]
    picks += [body("html", 3 * BLOCK), body("fib", 65537), body("random", 65536)]
    alone = [gz.compress([b])[0] for b in picks]
    alone_raw = [gz.deflate([b])[0] for b in picks]
    assert [a[10:-8] for a in alone] == alone_raw
    rng = random.Random(29)
    others = [html(rng, rng.randrange(0, 70000)) for _ in range(40)] + [rng.randbytes(40000), b""]
    for i, b in enumerate(picks[::7]):
        for at in (0, len(others) // 2, len(others)):
            batch = others[:at] + [b] + others[at:]
            assert gz.compress(batch)[at] == alone[7 * i], (7 * i, at)
    assert gz.compress(picks) == alone
    assert gz.compress(picks[::-1]) == alone[::-1]
    big = [html(rng, 150000) for _ in range(60)] + [rng.randbytes(100000) for _ in range(20)]
    assert all(zlib.decompress(o, 31) == b for b, o in zip(big, gz.compress(big)))
    assert [gz.compress([b])[0] for b in picks] == alone
    assert gz.deflate(picks) == alone_raw


def test_many_blocks(gz):
    """More than 2048 blocks in one batch: k_slot_scan gives each of its 1024 threads 3
    blocks. 2500 bodies of 0..40 bytes with empty ones interleaved, plus 20 multi-block
    bodies in the middle of them."""
    rng = random.Random(31)
    bodies = [b"" if i % 5 == 0 else html(rng, 1 + i % 40) if i % 2 else rng.randbytes(1 + i % 40)
              for i in range(2500)]
    multi = [html(rng, rng.randrange(BLOCK + 1, 4 * BLOCK)) for _ in range(10)]
    multi += [rng.randbytes(2 * BLOCK + 1), b"z" * (3 * BLOCK), html(rng, 2 * BLOCK)] * 3 + [
        html(rng, 5 * BLOCK + 77)]
    assert len(multi) == 20
    for k, m in enumerate(multi):
        bodies.insert(100 + 117 * k, m)
    blocks = sum(max(1, -(-len(b) // BLOCK)) for b in bodies)
    assert blocks > 2048 and -(-blocks // 1024) == 3
    before = gz.stats()
    out = gz.compress(bodies)
    after = gz.stats()
    assert after.blocks - before.blocks == blocks
    assert after.inputs - before.inputs == len(bodies)
    assert after.in_bytes - before.in_bytes == sum(map(len, bodies))
    assert len(out) == len(bodies)
    for b, o in zip(bodies, out):
        assert zlib.decompress(o, 31) == b
