"""The gzip members the inflate tests decode, built with deflate_ref. Shared by
test_deflate_ref.py (CPU: the valid ones decode with zlib to the intended bytes, the
malformed ones are rejected by zlib) and test_gpu_inflate.py (GPU: k_inflate must agree
with zlib on every one). Not collected by pytest. Everything is seeded."""
import gzip
import random
import zlib
from collections import namedtuple

import deflate_ref as ref

# member: the gzip member; raw / body: its DEFLATE stream and the bytes it was built to
# decode to (None where the member was not built from a valid stream); valid: True when
# zlib must accept it, False when zlib must reject it, None when only the oracle decides;
# may_decline: the GPU path may answer None although zlib accepts (gunzip_batch must still
# give zlib's bytes); must_decline: the GPU path must answer None although zlib accepts.
Case = namedtuple("Case", "name member raw body valid may_decline must_decline")


def case(name, raw, body, valid=True, may_decline=False, must_decline=False, **wrap):
    return Case(name, ref.gzip_wrap(raw, body, **wrap), raw, body, valid, may_decline, must_decline)


def member_case(name, member, valid, **kw):
    return Case(name, member, None, None, valid, kw.get("may_decline", False),
                kw.get("must_decline", False))


def html(rng, n):
    """The HTML-like text of test_gpu_gzip.py (same generator, same seeds)."""
    words = [b"cache", b"proxy", b"<div class=\"item\">", b"</div>", b"memcached", b"GPU",
             b"<a href=\"/static/obj/", b"\">", b"</a>", b"HBM", b"\n", b"  "]
    out = bytearray()
    while len(out) < n:
        out += rng.choice(words)
        if rng.random() < 0.1:
            out += str(rng.randrange(10 ** 6)).encode()
    return bytes(out[:n])


class Tokens:
    """A token list under construction, with the output it stands for."""

    def __init__(self, seed):
        self.rng = random.Random(seed)
        self.toks = []
        self.out = bytearray()

    @property
    def opos(self):
        return len(self.out)

    def lit(self, n=1):
        for _ in range(n):
            b = self.rng.randrange(256)
            self.toks.append(b)
            self.out.append(b)

    def copy(self, length, dist):
        assert 3 <= length <= 258 and 1 <= dist <= min(self.opos, 32768), (length, dist, self.opos)
        self.toks.append((length, dist))
        if dist >= length:
            self.out += self.out[self.opos - dist:self.opos - dist + length]
        else:
            for _ in range(length):
                self.out.append(self.out[-dist])

    def fill_to(self, target):
        """Long copies at random distances (and a few literals) up to exactly ``target``."""
        assert target >= self.opos
        if self.opos < 300:
            self.lit(min(300, target) - self.opos)
        while self.opos < target:
            left = target - self.opos
            if left < 3 or self.rng.random() < 0.05:
                self.lit()
            else:
                self.copy(min(258, left), self.rng.randint(1, min(self.opos, 32768)))

    def fixed(self, name, **kw):
        w = ref.BitWriter()
        ref.fixed_block(w, self.toks, True)
        return case(name, w.getvalue(), bytes(self.out), **kw)


# ------------------------------------------------------------------------------------
# copies: fixed-Huffman members from tokens


def copy_cases():
    cases = []
    t = Tokens(1)  # every length, across the first and second window wrap
    t.fill_to(32768)
    for length in range(3, 259):
        t.copy(length, t.rng.randint(1, 32768))
        t.lit()
    t.fill_to(70000)
    cases.append(t.fixed("every length 3..258"))
    t = Tokens(2)  # every distance 1..65 at lengths below, at and above the distance
    t.fill_to(20000)
    for dist in range(1, 66):
        for length in (3, 63, 64, 65, 130, 258):
            t.copy(length, dist)
            t.lit()
    t.fill_to(72000)
    cases.append(t.fixed("every distance 1..65"))
    t = Tokens(3)  # the first and the last distance of every distance symbol
    t.fill_to(33000)
    ends = sorted(set(ref.DBASE) | {b - 1 for b in ref.DBASE[1:]} | {32768})
    for dist in ends:
        t.copy(t.rng.choice((3, 64, 200, 258)), dist)
        t.lit()
    t.copy(258, 32768)
    t.copy(258, 32768)
    t.fill_to(70000)
    for dist in ends:
        t.copy(258, dist)
    cases.append(t.fixed("distance symbol bounds, 32768 x 258"))
    # a copy that starts at 32768 k + delta, delta in -258..+1, k = 1 and 2
    deltas = list(range(-258, 2))
    for i in range(len(deltas)):
        t = Tokens(100 + i)
        j = (i + 130) % 260
        for k, delta in ((1, deltas[i]), (2, deltas[j])):
            t.fill_to(32768 * k + delta)
            far = min(t.opos, 32768)  # 32768 itself from the first wrap on
            dist = (far if (delta + k) % 3 == 0 else
                    t.rng.randint(1, 63) if (delta + k) % 3 == 1 else t.rng.randint(64, far))
            t.copy(258 if delta % 2 == 0 else t.rng.randint(3, 258), dist)
        t.fill_to(32768 * 2 + 700)
        cases.append(t.fixed(f"copies at the window wrap, deltas {deltas[i]} and {deltas[j]}"))
    # copies around the multiples of the 1024-byte output flush
    for j, delta in enumerate((-258, -257, -129, -65, -64, -63, -2, -1, 0, 1)):
        t = Tokens(400 + j)
        for k in range(1, 70):
            t.fill_to(1024 * k + delta)
            t.copy(t.rng.choice((3, 64, 65, 258)), t.rng.choice((1, 63, 64, min(t.opos, 1000), min(t.opos, 32768))))
        cases.append(t.fixed(f"copies at the output flush, delta {delta}"))
    t = Tokens(5)  # overlapping copies (dist < len)
    t.fill_to(30000)
    for _ in range(12):
        for period in (1, 2, 3, 63, 64, 65):
            for length in (period + 1, 2 * period + 1, 66, 129, 258):
                if 3 <= length <= 258:
                    t.lit(period)
                    t.copy(length, period)
    t.fill_to(max(t.opos, 70000))
    cases.append(t.fixed("overlapping copies at periods 1 2 3 63 64 65"))
    return cases


# ------------------------------------------------------------------------------------
# stored blocks

STORED_LENS = [0, 1, 2047, 2048, 2049, 8191, 8193, 65535]


def stored_cases():
    rng = random.Random(21)
    cases = []
    for n in STORED_LENS:
        data = rng.randbytes(n)
        w = ref.BitWriter()
        ref.stored_block(w, data, True)
        cases.append(case(f"one final stored block of {n}", w.getvalue(), data))
        w = ref.BitWriter()  # between two Huffman blocks
        ref.fixed_block(w, list(b"head"), False)
        ref.stored_block(w, data, False)
        ref.fixed_block(w, list(b"tail") + [(4, 4)], True)
        cases.append(case(f"stored block of {n} between fixed blocks", w.getvalue(),
                          b"head" + data + b"tailtail"))
    w, body = ref.BitWriter(), b""
    for i, n in enumerate(STORED_LENS + [0, 0, 5]):
        data = rng.randbytes(n)
        ref.stored_block(w, data, i == len(STORED_LENS) + 2)
        body += data
    cases.append(case("stored blocks in a row", w.getvalue(), body))
    for nine in range(8):  # the Huffman block ends at bit (2 + nine) % 8
        w = ref.BitWriter()
        toks = [65, 66] + [200 + k for k in range(nine)]
        ref.fixed_block(w, toks, False)
        assert w.bitpos % 8 == (2 + nine) % 8
        data = rng.randbytes(3000)
        ref.stored_block(w, data, False)
        ref.fixed_block(w, [(258, 3000)], True)
        body = bytes(toks) + data
        cases.append(case(f"stored block after a block ending at bit {(2 + nine) % 8}",
                          w.getvalue(), body + ref.apply_tokens([(258, 3000)], body)))
    for seed in (22, 23):
        body = random.Random(seed).randbytes(200000)
        cases.append(member_case(f"zlib level 0, 200 KB, seed {seed}", gzip.compress(body, 0, mtime=0), True))
    return cases


# ------------------------------------------------------------------------------------
# dynamic blocks

SKEW = list(range(1, 15)) + [15, 15]  # a complete code with two 15-bit codes


def _dyn(name, toks, ll, dl, body=None, **kw):
    w = ref.BitWriter()
    ref.dynamic_block(w, toks, True, ll, dl, **kw)
    return case(name, w.getvalue(), ref.apply_tokens(toks) if body is None else body)


def dynamic_cases():
    rng = random.Random(31)
    cases = []
    # code lengths of 15 in both tables; the 15-bit codes are used
    ll = [0] * 264
    syms = list(range(97, 111)) + [256, 263]  # 'a'..'n' get 1..14 bits, 256 and 263 get 15
    for s, l in zip(syms, SKEW):
        ll[s] = l
    dl = SKEW[:]  # distance symbols 0..13 get 1..14 bits, 14 and 15 get 15
    toks = [rng.choice(range(97, 111)) for _ in range(400)]
    for dist in (1, 2, 5, 30, 100, 129, 193, 255, 256):
        toks += [(9, dist), 110, 109]
    cases.append(_dyn("code lengths of 15", toks, ll, dl))
    # one distance code of one bit (an incomplete set zlib allows), used with bit 0
    toks = list(b"abcabc") + [(50, 1), 100, (258, 1), (3, 1)]
    ll, _ = ref.lengths_for(toks)
    cases.append(_dyn("a single one-bit distance code", toks, ll, [1]))
    # no distance code at all
    toks = list(rng.randbytes(50)) * 4
    ll, _ = ref.lengths_for(toks)
    cases.append(_dyn("no distance code, literals only", toks, ll, [0]))
    # a repeat run from the literal/length lengths into the distance lengths
    ll = [0] * 264
    for s in list(range(97, 105)) + list(range(256, 264)):
        ll[s] = 4
    dl = [4] * 16
    toks = list(b"abcdefgh") * 8 + [(2 + k, 1 + 7 * k) for k in range(1, 8)]
    c = _dyn("a repeat run across the HLIT/HDIST boundary", toks, ll, dl)
    assert any(s == 16 and at < 264 < at + n for s, _, at, n in
               ref.rle_code_lengths(ll + dl)), "no repeat crosses the boundary"
    cases.append(c)
    # HCLEN: 5 code-length codes is the fewest a valid block can have (with 4 only the
    # length 0 and the repeat codes exist, so there is no end-of-block code); and all 19
    ll = [8] * 255 + [0, 8]  # literals 0..254 and the end code, 8 bits each
    toks = list(rng.randbytes(300).replace(b"\xff", b"\x00"))
    cases.append(_dyn("HCLEN 5", toks, ll, [0], use_repeats=False, hclen=5,
                      cl_lens=[1] + [0] * 7 + [1] + [0] * 10))
    toks = list(html(rng, 3000))
    ll, dl = ref.lengths_for(toks)
    cases.append(_dyn("HCLEN 19 with trailing zeros", toks, ll, dl, hclen=19))
    ll = [0] * 257
    for s, l in zip(list(range(14)) + [255, 256], SKEW):
        ll[s] = l  # lengths 1 and 15 force the last code-length code (15) to be sent
    toks = [rng.choice(range(14)) for _ in range(200)] + [255]
    cases.append(_dyn("HCLEN 19 by need", toks, ll, [0], use_repeats=False))
    # HLIT 257 / 286, HDIST 1 / 30
    toks = list(html(rng, 2000))
    ll, _ = ref.lengths_for(toks, hlit=257)
    cases.append(_dyn("HLIT 257, HDIST 1", toks, ll, [0]))
    t = Tokens(32)
    t.fill_to(33000)
    t.copy(258, 32768)
    t.copy(258, 24577)
    t.copy(3, 1)
    ll, dl = ref.lengths_for(t.toks)
    assert len(ll) == 286 and len(dl) == 30
    cases.append(_dyn("HLIT 286, HDIST 30", t.toks, ll, dl, body=bytes(t.out)))
    cases.append(_dyn("HLIT 286, HDIST 30, no repeat codes", t.toks, ll, dl, body=bytes(t.out),
                      use_repeats=False))
    return cases


# ------------------------------------------------------------------------------------
# ring refill: block headers and symbols at every offset of the 8 KiB input ring


def ring_cases():
    cases = []
    for seed in (41, 42):
        rng = random.Random(seed)
        body = bytes(rng.choice(b"abcdefgh<>/ \n") for _ in range(100000))
        c = zlib.compressobj(6, zlib.DEFLATED, 31, 1)
        cases.append(member_case(f"zlib memLevel 1, 100 KB, seed {seed}", c.compress(body) + c.flush(), True))
    rng = random.Random(43)
    for n in (4095, 4096, 4097, 8191, 8192, 8193, 20000):
        # fixed block of 8-bit literals: 3 + 8 k + 7 bits = k + 2 bytes
        body = bytes(rng.randrange(144) for _ in range(n - 2))
        w = ref.BitWriter()
        ref.fixed_block(w, list(body), True)
        assert len(w.getvalue()) == n
        cases.append(case(f"fixed block of {n} bytes", w.getvalue(), body))
        body = rng.randbytes(n - 5)
        w = ref.BitWriter()
        ref.stored_block(w, body, True)
        assert len(w.getvalue()) == n
        cases.append(case(f"stored block of {n} bytes", w.getvalue(), body))
        # zlib's dynamic blocks up to the last byte, after a stored block that pads to n
        body = html(rng, 3 * n)
        z = zlib.compressobj(6, zlib.DEFLATED, -15)
        raw = z.compress(body) + z.flush()
        pad = n - len(raw) - 5
        if pad >= 0:
            w = ref.BitWriter()
            head = rng.randbytes(pad)
            ref.stored_block(w, head, False)
            cases.append(case(f"stored then zlib blocks, {n} bytes", w.getvalue() + raw, head + body))
    return cases


# ------------------------------------------------------------------------------------
# gzip framing


def framing_cases():
    rng = random.Random(51)
    body = html(rng, 3000)
    z = zlib.compressobj(6, zlib.DEFLATED, -15)
    raw = z.compress(body) + z.flush()
    ex = b"ab\x04\x00data"
    cases = [
        case("plain header", raw, body),
        case("FEXTRA", raw, body, fextra=ex),
        case("FNAME", raw, body, fname=b"index.html"),
        case("FCOMMENT", raw, body, fcomment=b"a comment"),
        case("FHCRC correct", raw, body, fhcrc=True, may_decline=True),
        case("all four fields", raw, body, fextra=ex, fname=b"n", fcomment=b"c", fhcrc=True,
             may_decline=True),
        case("FEXTRA + FNAME + FCOMMENT", raw, body, fextra=ex, fname=b"", fcomment=b""),
        case("FHCRC correct, FEXTRA of 0 bytes", raw, body, fextra=b"", fhcrc=True, may_decline=True),
        case("FHCRC correct, FEXTRA of 65535 bytes", raw, body, fextra=rng.randbytes(65535),
             fhcrc=True, may_decline=True),
        case("FEXTRA of 0 bytes", raw, body, fextra=b""),
        case("FEXTRA of 65535 bytes", raw, body, fextra=rng.randbytes(65535)),
        case("wrong FHCRC", raw, body, fhcrc=(zlib.crc32(b"\x1f\x8b\x08\x02\0\0\0\0\0\xff") ^ 1) & 0xFFFF,
             valid=False),
        case("wrong FHCRC after FNAME", raw, body, fname=b"x", fhcrc=0x1234, valid=False),
        case("reserved FLG bit 5", raw, body, flg_extra=0x20, valid=False),
        case("reserved FLG bit 6", raw, body, flg_extra=0x40, valid=False),
        case("reserved FLG bit 7", raw, body, flg_extra=0x80, valid=False),
        case("reserved FLG bits with FNAME", raw, body, fname=b"x", flg_extra=0xE0, valid=False),
        case("FTEXT", raw, body, flg_extra=1),
        case("CM 7", raw, body, cm=7, valid=False),
        case("CM 0", raw, body, cm=0, valid=False),
    ]
    good = ref.gzip_wrap(raw, body)
    m = bytearray(ref.gzip_wrap(raw, body, fextra=ex))
    m[10:12] = (len(m)).to_bytes(2, "little")  # XLEN runs past the end of the member
    cases.append(member_case("FEXTRA length past the end", bytes(m), False))
    m = bytearray(ref.gzip_wrap(b"", b"", fextra=b""))
    m[10:12] = b"\xff\xff"
    cases.append(member_case("FEXTRA length past the end of a tiny member", bytes(m), False))
    m = ref.gzip_wrap(raw, body, fname=b"")
    cases.append(member_case("unterminated FNAME", m[:10] + bytes(x or 1 for x in m[10:]), False))
    m = ref.gzip_wrap(raw, body, fcomment=b"")
    cases.append(member_case("unterminated FCOMMENT", m[:10] + bytes(x or 1 for x in m[10:]), False))
    cases.append(member_case("wrong magic", b"\x1f\x8c" + good[2:], False))
    empty = gzip.compress(b"", mtime=0)
    assert len(empty) == 20
    for n in range(18):
        cases.append(member_case(f"member of {n} bytes", empty[:n], False))
    cases.append(member_case("empty body", empty, True))
    return cases


# ------------------------------------------------------------------------------------
# sizes, caps and the trailer


def size_cases():
    """(cases, ISIZE): test with max_out = ISIZE and ISIZE - 1."""
    rng = random.Random(61)
    body = html(rng, 5000)
    z = zlib.compressobj(6, zlib.DEFLATED, -15)
    raw = z.compress(body) + z.flush()
    t = Tokens(62)
    t.fill_to(5000 - 258)
    t.copy(258, 100)  # the output ends with a copy
    w = ref.BitWriter()
    ref.stored_block(w, body, True)
    cases = [
        case("exact", raw, body),
        t.fixed("exact, ends with a copy"),
        case("exact, stored", w.getvalue(), body),
        case("ISIZE one less", raw, body, isize=4999, valid=False),
        case("ISIZE one more", raw, body, isize=5001, valid=False),
        t.fixed("ISIZE one less, ends with a copy", isize=4999, valid=False),
        case("ISIZE one less, stored", w.getvalue(), body, isize=4999, valid=False),
        case("wrong CRC", raw, body, crc=zlib.crc32(body) ^ 0x80000000, valid=False),
        case("wrong CRC, low bit", raw, body, crc=zlib.crc32(body) ^ 1, valid=False),
    ]
    return cases, 5000


# ------------------------------------------------------------------------------------
# malformed streams: one member per error exit of the kernel, and what zlib rejects beyond


def _bad(name, w, body=b"", **kw):
    return case(name, w.getvalue(), body, valid=False, **kw)


def malformed_cases():
    rng = random.Random(71)
    cases = []
    W = ref.BitWriter
    w = W()
    ref.stored_block(w, b"hello", True, nlen=0x1234)
    cases.append(_bad("LEN/NLEN mismatch", w, b"hello"))
    w = W()
    ref.stored_block(w, b"0123456789", True, length=1000)
    cases.append(_bad("stored length past the input", w, b"0123456789"))
    w = W()
    ref.stored_block(w, b"0123456789", True, length=18)  # ends inside the trailer
    cases.append(_bad("stored length into the trailer", w, b"0123456789"))
    w = W()
    w.bits(1, 1)
    w.bits(3, 2)
    w.bits(0, 13)
    cases.append(_bad("BTYPE 3", w))
    w = W()
    ref.fixed_block(w, list(b"ok"), False)
    w.bits(0, 1)
    w.bits(3, 2)
    cases.append(_bad("BTYPE 3 after a good block", w, b"ok"))
    toks = list(b"abcabcabc") + [(6, 3)]
    body = ref.apply_tokens(toks)
    ll, dl = ref.lengths_for(toks)
    for hlit in (287, 288):
        w = W()
        ref.dynamic_block(w, toks, True, ll + [0] * (hlit - len(ll)), dl)
        cases.append(_bad(f"HLIT {hlit}", w, body))
    for hdist in (31, 32):
        w = W()
        ref.dynamic_block(w, toks, True, ll, dl + [0] * (hdist - len(dl)))
        cases.append(_bad(f"HDIST {hdist}", w, body))
    w = W()
    ref.dynamic_block(w, toks, True, ll, dl, cl_lens=[1, 1, 1] + [2] * 16, hclen=19)
    cases.append(_bad("over-subscribed code-length code", w, body))
    # an incomplete code-length code (three 2-bit codes): once with only its codes in use,
    # once with the unused fourth code in the stream
    cl = [0] * 19
    cl[0] = cl[3] = cl[4] = 2
    lits = [0] * 257
    for s in (97, 98, 99, 100, 256, 101, 102, 103):
        lits[s] = 3
    w = W()
    ref.dynamic_block(w, list(b"abcdabcd"), True, lits, [0], cl_lens=cl, use_repeats=False)
    cases.append(_bad("incomplete code-length code", w, b"abcdabcd"))
    w = W()
    w.bits(1, 1)
    w.bits(2, 2)
    w.bits(0, 5)
    w.bits(0, 5)
    w.bits(15, 4)
    for k in range(19):
        w.bits(cl[ref.CL_ORDER[k]], 3)
    w.code(3, 2)  # the code no symbol has
    w.bits(0, 64)
    cases.append(_bad("invalid code-length code", w))
    w = W()
    ref.dynamic_header(w, True, ll, dl, ops=[(16, 0)] + [(s, x) for s, x, _, _ in
                                                         ref.rle_code_lengths(ll + dl)][3:])
    cases.append(_bad("repeat with no previous length", w))
    w = W()
    ops = [(s, x) for s, x, _, _ in ref.rle_code_lengths(ll + dl)]
    ref.dynamic_header(w, True, ll, dl, ops=ops[:-1] + [(18, 127)])
    w.bits(0, 64)
    cases.append(_bad("repeat past HLIT + HDIST", w))
    w = W()
    ops = [(s, x) for s, x, _, _ in ref.rle_code_lengths(ll[:-1] + dl)]
    ref.dynamic_header(w, True, ll, dl, ops=ops + [(17, 7)])
    w.bits(0, 64)
    cases.append(_bad("zero repeat past HLIT + HDIST", w))
    noeob = ll[:]
    noeob[0], noeob[256] = ll[256], 0  # the set stays complete
    w = W()
    ref.dynamic_header(w, True, noeob, dl)
    w.bits(0, 64)
    cases.append(_bad("no end-of-block code", w))
    # HCLEN 4 leaves only the length 0 and the repeat codes: no block with it is valid
    cl4 = [0] * 19
    cl4[0] = cl4[18] = 1
    w = W()
    ref.dynamic_header(w, True, [0] * 257, [0], cl_lens=cl4, hclen=4, ops=[(18, 127), (18, 109)])
    w.bits(0, 64)
    cases.append(_bad("HCLEN 4", w))
    # a literal/length set of one one-bit code (allowed) whose other code is used
    one = [0] * 256 + [1]
    w = W()
    ref.dynamic_header(w, True, one, [0])
    w.bits(1, 1)
    w.bits(0, 32)
    cases.append(_bad("invalid literal/length code", w))
    w = W()
    ref.dynamic_header(w, True, one, [0])
    w.bits(0, 1)  # the same header is fine when only the end code is used
    cases.append(case("one-bit end-of-block code alone", w.getvalue(), b""))
    for sym in (286, 287):
        w = W()
        ref.fixed_block(w, list(b"abc"), False, eob=False)
        ref.fixed_symbol(w, sym)
        w.bits(0, 32)
        cases.append(_bad(f"fixed symbol {sym}", w, b"abc"))
    for ds in (30, 31):
        w = W()
        ref.fixed_block(w, list(b"abcdef"), False, eob=False)
        ref.fixed_symbol(w, 257)
        w.code(ds, 5)
        w.bits(0, 48)
        cases.append(_bad(f"fixed distance code {ds}", w, b"abcdef"))
    # a distance symbol of a dynamic set that has no code for it
    toks2 = list(b"abcabc")
    w = W()
    ll2, _ = ref.lengths_for(toks2 + [(3, 1)])
    ref.dynamic_block(w, toks2, True, ll2, [1], eob=False)
    w.code(ref.canonical_codes(ll2)[257], ll2[257])
    w.bits(1, 1)  # the unused half of the one-bit distance code
    w.bits(0, 32)
    cases.append(_bad("invalid distance code", w, b"abcabc"))
    for n, dist in ((0, 1), (5, 6), (300, 32768), (32767, 32768)):
        w = W()
        lits = list(rng.randbytes(n))
        ref.fixed_block(w, lits + [(3, dist), 65], True)
        cases.append(_bad(f"distance {dist} at output {n}", w, bytes(lits) + b"AAAA"))
    body = html(rng, 1000)
    for name, toks3 in (("literal", list(body) + [33]), ("copy", list(body) + [(258, 7)]),
                        ("long copy", list(body[:900]) + [(258, 900)])):
        w = W()
        ref.fixed_block(w, toks3, True)
        cases.append(_bad(f"output past ISIZE by a {name}", w, body))
    w = W()
    ref.fixed_block(w, list(body), False)
    ref.stored_block(w, b"extra", True)
    cases.append(_bad("output past ISIZE by a stored block", w, body))
    # the stream ends before the trailer, or after it begins
    z = zlib.compressobj(6, zlib.DEFLATED, -15)
    raw = z.compress(body) + z.flush()
    for junk in (b"\0", b"\0" * 5, rng.randbytes(5), rng.randbytes(4096), raw):
        cases.append(case(f"{len(junk)} junk bytes before the trailer", raw + junk, body, valid=False))
    w = W()
    ref.stored_block(w, body, True)
    cases.append(case("junk after a final stored block", w.getvalue() + b"\0\0\xff\xff", body, valid=False))
    cases.append(case("stream one byte short", raw[:-1], body, valid=False))
    good = ref.gzip_wrap(raw, body)
    cases.append(member_case("m + m", good + good, None, must_decline=True))
    cases.append(member_case("m + junk", good + b"\0" * 8, None, must_decline=True))
    # code sets zlib rejects: over-subscribed, and incomplete unless one one-bit code
    toks = list(b"abcabcabc") + [(6, 3)]
    body = ref.apply_tokens(toks)
    ll, dl = ref.lengths_for(toks)  # dl: one bit each for distance symbols 0 and 2
    assert dl == [1, 0, 1]
    # each stream below uses only codes that decode the same way with or without the
    # defect in the set, so nothing but the check of the set itself can reject it
    spare, _ = ref.lengths_for(toks + [120])
    spare[120] = 0  # the code of literal 120 is left unassigned
    for name, l2, d2 in (
            ("over-subscribed literal/length set", ll[:120] + [15] + ll[121:], dl),
            ("over-subscribed distance set", ll, [1, 15, 1]),
            ("heavily over-subscribed distance set", ll, [1, 1, 1, 1]),
            ("incomplete literal/length set", spare, dl),
            ("incomplete distance set: one 2-bit code", ll, [0, 0, 2]),
            ("incomplete distance set: 1 + 2 bits", ll, [2, 0, 1]),
            ("incomplete distance set: one 15-bit code short", ll, list(range(1, 16)))):
        w = W()
        ref.dynamic_block(w, toks, True, l2, d2)
        cases.append(_bad(name, w, body))
    # truncation of a valid member at every 7th prefix length
    m = gzip.compress(html(rng, 1500), 6, mtime=0)
    for n in range(0, len(m), 7):
        cases.append(member_case(f"valid member cut to {n} of {len(m)} bytes", m[:n], False))
    return cases


def bitflip_cases():
    body = html(random.Random(5), 2048)
    m = gzip.compress(body, 6, mtime=0)
    cases = [member_case("unflipped", m, True)]
    flips = [(i, b) for i in range(10) for b in range(8)]
    flips += [(i, b) for i in range(len(m) - 8, len(m)) for b in range(8)]
    flips += [(i, i % 8) for i in range(10, len(m) - 8)]
    for i, b in flips:
        x = bytearray(m)
        x[i] ^= 1 << b
        cases.append(member_case(f"bit {b} of byte {i} flipped", bytes(x), None))
    return cases, body


def zlib_oracle(member, cap):
    """(accepted, output): what zlib makes of one gzip member with ``cap`` output bytes."""
    assert cap > 0
    d = zlib.decompressobj(31)
    try:
        o = d.decompress(member, cap)
    except zlib.error:
        return False, None
    return (True, o) if d.eof else (False, None)
