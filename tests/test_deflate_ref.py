"""The bit-level DEFLATE reference of the GPU gzip tests (tests/deflate_ref.py) against
zlib, on the CPU: what its encoders build decodes with zlib to the intended bytes, its
tracing inflater reproduces zlib's output on zlib-made streams of every kind, and every
malformed member of tests/inflate_cases.py is rejected by zlib — the asserts that pin the
oracle the GPU tests rely on."""
import random
import zlib

import pytest

import deflate_ref as ref
import inflate_cases as ic

GROUPS = {
    "copies": ic.copy_cases,
    "stored": ic.stored_cases,
    "dynamic": ic.dynamic_cases,
    "ring": ic.ring_cases,
    "framing": ic.framing_cases,
    "sizes": lambda: ic.size_cases()[0],
    "malformed": ic.malformed_cases,
    "bitflips": lambda: ic.bitflip_cases()[0],
}


@pytest.fixture(scope="module")
def groups():
    return {k: f() for k, f in GROUPS.items()}


@pytest.mark.parametrize("group", list(GROUPS))
def test_cases_are_what_they_claim(groups, group):
    """Valid cases: zlib decodes the raw stream and the member to the intended bytes.
    Malformed cases: zlib.decompressobj(31) raises or ends with eof false."""
    n_valid = n_bad = 0
    for c in groups[group]:
        ok, out = ic.zlib_oracle(c.member, 64 << 20)
        if c.valid:
            n_valid += 1
            assert ok, c.name
            if c.raw is not None:
                assert zlib.decompress(c.raw, -15) == c.body, c.name
                assert out == c.body, c.name
        elif c.valid is False:
            n_bad += 1
            assert not ok, c.name
    assert n_valid + n_bad > 0
    if group in ("copies", "stored", "dynamic", "ring"):
        assert n_bad == 0
    if group == "malformed":
        assert n_bad > 100 and n_valid == 1


def test_trace_agrees_with_zlib_about_every_case(groups):
    """The tracing inflater accepts exactly the streams zlib accepts, with zlib's bytes
    (raw streams of the cases that were built from one; framing is zlib's business)."""
    for group in ("copies", "stored", "dynamic", "ring", "malformed"):
        for c in groups[group]:
            if c.raw is None:
                continue
            d = zlib.decompressobj(-15)
            try:
                want = d.decompress(c.raw)
                want = want if d.eof else None
            except zlib.error:
                want = None
            try:
                got, used = ref.inflate(c.raw)
            except ref.DeflateError:
                got = None
            assert got == want, (group, c.name)
            if want is not None:
                assert used == len(c.raw) - len(d.unused_data), (group, c.name)


def test_copy_cases_cover_what_they_name(groups):
    toks = [t for c in groups["copies"] for b in ref.trace(c.raw) for t in b.tokens
            if not isinstance(t, int)]
    assert {l for l, _ in toks} == set(range(3, 259))
    assert set(range(1, 66)) <= {d for _, d in toks}
    assert set(ref.DBASE) | {b - 1 for b in ref.DBASE[1:]} | {32768} <= {d for _, d in toks}
    assert (258, 32768) in toks
    starts = set()  # output offsets at which a copy starts
    for c in groups["copies"]:
        pos = 0
        for t in ref.trace(c.raw)[0].tokens:
            if isinstance(t, int):
                pos += 1
            else:
                starts.add(pos)
                pos += t[0]
    for k in (1, 2):
        assert {32768 * k + d for d in range(-258, 2)} <= starts
    for period in (1, 2, 3, 63, 64, 65):
        assert any(d == period and l > d for l, d in toks)


def _bodies():
    rng = random.Random(77)
    return [b"", b"a", b"abc" * 5, ic.html(rng, 70000), rng.randbytes(40000),
            bytes(rng.choice(b"ab") for _ in range(50000)), b"\0" * 100000,
            bytes(range(256)) * 200 + ic.html(rng, 5000)]


def _check_trace(raw, body):
    blocks = ref.trace(raw)
    assert b"".join(b.data for b in blocks) == body
    assert [b.final for b in blocks] == [False] * (len(blocks) - 1) + [True]
    assert blocks[0].start_bit == 0 and (blocks[-1].end_bit + 7) // 8 == len(raw)
    for a, b in zip(blocks, blocks[1:]):
        assert a.end_bit == b.start_bit and a.out_start + len(a.data) == b.out_start
    for b in blocks:
        if b.btype == 0:
            assert b.tokens is None
        else:
            assert ref.apply_tokens(b.tokens, body[:b.out_start]) == b.data
            assert ref.kraft(b.ll_lens) <= 1 << 15 and b.ll_lens[256]
    return blocks


@pytest.mark.parametrize("level", [0, 1, 6, 9])
def test_trace_reproduces_zlib_levels(level):
    for body in _bodies():
        z = zlib.compressobj(level, zlib.DEFLATED, -15)
        blocks = _check_trace(z.compress(body) + z.flush(), body)
        if level == 0:
            assert all(b.btype == 0 for b in blocks)


@pytest.mark.parametrize("strategy", [zlib.Z_FIXED, zlib.Z_RLE, zlib.Z_HUFFMAN_ONLY])
def test_trace_reproduces_zlib_strategies(strategy):
    for body in _bodies():
        z = zlib.compressobj(6, zlib.DEFLATED, -15, 8, strategy)
        blocks = _check_trace(z.compress(body) + z.flush(), body)
        toks = [t for b in blocks if b.tokens for t in b.tokens if not isinstance(t, int)]
        if strategy == zlib.Z_FIXED:
            assert all(b.btype in (0, 1) for b in blocks)
        if strategy == zlib.Z_RLE:
            assert all(d == 1 for _, d in toks)
        if strategy == zlib.Z_HUFFMAN_ONLY:
            assert not toks


def test_trace_reproduces_zlib_mem_level_1():
    most = 0
    for body in _bodies():
        z = zlib.compressobj(6, zlib.DEFLATED, -15, 1)
        most = max(most, len(_check_trace(z.compress(body) + z.flush(), body)))
    assert most > 100  # a 128-symbol buffer: a block every few hundred bytes of text


@pytest.mark.parametrize("flush", [zlib.Z_SYNC_FLUSH, zlib.Z_FULL_FLUSH])
def test_trace_reproduces_zlib_flushes(flush):
    for body in _bodies():
        z = zlib.compressobj(6, zlib.DEFLATED, -15)
        half = len(body) // 2
        first = z.compress(body[:half]) + z.flush(flush)
        raw = first + z.compress(body[half:]) + z.flush()
        blocks = _check_trace(raw, body)
        # the flush marker: an empty stored block that ends where the first part ends
        marks = [b for b in blocks if b.btype == 0 and not b.data and b.end_bit == 8 * len(first)]
        assert len(marks) == 1 and raw[len(first) - 4:len(first)] == b"\0\0\xff\xff"
        if flush == zlib.Z_FULL_FLUSH:  # the second part does not reach into the first
            tail = ref.trace(raw, start_bit=8 * len(first))
            assert b"".join(b.data for b in tail) == body[half:]


def test_empty_window_mode():
    """With an empty window per block a reference before the block's own start is an
    error; the same stream decodes in the normal mode."""
    w = ref.BitWriter()
    ref.fixed_block(w, list(b"abcdef"), False)
    ref.fixed_block(w, [120, (3, 1), (4, 4)], False)  # inside the block: fine
    ref.fixed_block(w, [121, (3, 2)], True)            # reaches the 4 of the block before
    raw = w.getvalue()
    assert b"".join(b.data for b in ref.trace(raw)) == zlib.decompress(raw, -15)
    with pytest.raises(ref.DeflateError, match="too far back"):
        ref.trace(raw, empty_window=True)
    w = ref.BitWriter()
    ref.fixed_block(w, list(b"abcdef"), False)
    ref.stored_block(w, b"", False)
    ref.fixed_block(w, [120, (3, 1), (4, 4)], True)
    blocks = ref.trace(w.getvalue(), empty_window=True)
    assert [b.btype for b in blocks] == [1, 0, 1] and blocks[2].tokens == [120, (3, 1), (4, 4)]


def test_stored_blocks_from_any_bit_offset():
    for lits in range(8):
        w = ref.BitWriter()
        ref.fixed_block(w, [65] + [200] * lits, False)
        start = w.bitpos
        for n in (0, 1, 65535):
            ref.stored_block(w, bytes(n % 251 for _ in range(n)), n == 65535)
        raw = w.getvalue()
        blocks = ref.trace(raw)
        assert blocks[1].start_bit == start and [len(b.data) for b in blocks[1:]] == [0, 1, 65535]
        assert b"".join(b.data for b in blocks) == zlib.decompress(raw, -15)


def test_symbol_tables_and_huffman_lengths():
    for length in range(3, 259):
        s, nb, v = ref.len_symbol(length)
        assert ref.LBASE[s - 257] + v == length and v < (1 << nb) and nb == ref.LEXT[s - 257]
    for dist in range(1, 32769):
        s, nb, v = ref.dist_symbol(dist)
        assert ref.DBASE[s] + v == dist and v < (1 << nb) and nb == ref.DEXT[s]
    rng = random.Random(8)
    for limit, n in ((15, 286), (7, 19), (15, 30)):
        for _ in range(20):
            freq = [0] * n
            for k in rng.sample(range(n), rng.randrange(1, n + 1)):
                freq[k] = int(1.7 ** rng.randrange(0, 40)) + 1
            lens = ref.huffman_lengths(freq, limit)
            assert max(lens) <= limit and ref.kraft(lens) == 1 << 15
            assert all(l for f, l in zip(freq, lens) if f)


def test_gzip_wrap_fields():
    body = b"hello hello hello"
    z = zlib.compressobj(6, zlib.DEFLATED, -15)
    raw = z.compress(body) + z.flush()
    m = ref.gzip_wrap(raw, body, fextra=b"xy", fname=b"n", fcomment=b"c", fhcrc=True)
    assert m[3] == 0x1E and m[10:14] == b"\x02\x00xy" and m[14:18] == b"n\0c\0"
    assert int.from_bytes(m[18:20], "little") == zlib.crc32(m[:18]) & 0xFFFF
    assert zlib.decompress(m, 31) == body
    assert ref.gzip_wrap(raw, body)[:10] == b"\x1f\x8b\x08\0\0\0\0\0\0\xff"
    assert ref.gzip_wrap(raw, body, crc=1, isize=2)[-8:] == b"\x01\0\0\0\x02\0\0\0"
