"""A bit-level DEFLATE (RFC 1951) and gzip (RFC 1952) reference for the tests: pure Python,
no dependencies, written for clarity. Not collected by pytest.

* ``BitWriter`` and the block encoders build streams from explicit token lists (a literal
  is an int 0..255, a match a ``(length, distance)`` pair), including streams zlib would
  never make and malformed ones (raw bit / code emission).
* ``trace`` is an inflater that records, per block, BFINAL, BTYPE, the bit offsets of its
  start and end, the literal/length and distance code lengths and the token list. It is as
  strict as zlib about code sets. With ``empty_window=True`` every block is decoded with
  an empty window: a back-reference before the block's own first byte is an error.
"""
import zlib

LBASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99,
         115, 131, 163, 195, 227, 258]
LEXT = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DBASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025,
         1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577]
DEXT = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12,
        12, 13, 13]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
FIXED_LL = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_D = [5] * 32


class DeflateError(ValueError):
    pass


def len_symbol(length):
    """(symbol 257..285, extra bit count, extra value) of a match length 3..258."""
    if length == 258:
        return 285, 0, 0
    s = max(i for i in range(28) if LBASE[i] <= length)
    return 257 + s, LEXT[s], length - LBASE[s]


def dist_symbol(dist):
    """(symbol 0..29, extra bit count, extra value) of a match distance 1..32768."""
    s = max(i for i in range(30) if DBASE[i] <= dist)
    return s, DEXT[s], dist - DBASE[s]


def canonical_codes(lengths):
    """RFC 1951 §3.2.2: code value per symbol (0 where the length is 0). Over-subscribed
    sets still get values (masked to their length), so malformed headers can be written."""
    count = [0] * 17
    for l in lengths:
        count[l] += 1
    count[0] = 0
    nxt = [0] * 17
    code = 0
    for b in range(1, 17):
        code = (code + count[b - 1]) << 1
        nxt[b] = code
    out = []
    for l in lengths:
        if l:
            out.append(nxt[l] & ((1 << l) - 1))
            nxt[l] += 1
        else:
            out.append(0)
    return out


def kraft(lengths):
    """Sum of 2^-len over the coded symbols, as a fraction of 1 << 15."""
    return sum(1 << (15 - l) for l in lengths if l)


def huffman_lengths(freq, limit):
    """Code lengths of a complete prefix code with lengths <= limit for the symbols whose
    frequency is non-zero (a lone symbol gets a partner, so the set is complete)."""
    n = len(freq)
    used = [i for i in range(n) if freq[i]]
    lens = [0] * n
    if len(used) < 2:
        a = used[0] if used else 0
        lens[a] = 1
        lens[1 if a == 0 else 0] = 1
        return lens
    import heapq

    heap = [(freq[i], i, (i,)) for i in used]
    heapq.heapify(heap)
    tie = n
    depth = dict.fromkeys(used, 0)
    while len(heap) > 1:
        fa, _, sa = heapq.heappop(heap)
        fb, _, sb = heapq.heappop(heap)
        for s in sa + sb:
            depth[s] += 1
        heapq.heappush(heap, (fa + fb, tie, sa + sb))
        tie += 1
    for s in used:
        lens[s] = min(depth[s], limit)
    total, full = sum(1 << (limit - lens[s]) for s in used), 1 << limit
    while total > full:  # clamping over-subscribed the set: lengthen the rarest longest code
        s = max((s for s in used if lens[s] < limit), key=lambda s: (lens[s], -freq[s]))
        total -= 1 << (limit - lens[s] - 1)
        lens[s] += 1
    while total < full:  # fill the gap by shortening codes that fit
        fits = [s for s in used if lens[s] > 1 and total + (1 << (limit - lens[s])) <= full]
        s = max(fits, key=lambda s: (lens[s], freq[s]))
        total += 1 << (limit - lens[s])
        lens[s] -= 1
    return lens


class BitWriter:
    """LSB-first bit stream (RFC 1951 §3.1.1)."""

    def __init__(self):
        self.buf = bytearray()
        self.acc = 0
        self.n = 0

    @property
    def bitpos(self):
        return 8 * len(self.buf) + self.n

    def bits(self, value, nbits):
        """A data element: least significant bit first."""
        self.acc |= (value & ((1 << nbits) - 1)) << self.n
        self.n += nbits
        while self.n >= 8:
            self.buf.append(self.acc & 0xFF)
            self.acc >>= 8
            self.n -= 8

    def code(self, code, length):
        """A Huffman code: most significant bit first."""
        rev = 0
        for i in range(length):
            rev |= ((code >> i) & 1) << (length - 1 - i)
        self.bits(rev, length)

    def align(self):
        if self.n:
            self.bits(0, 8 - self.n)

    def raw(self, data):
        assert self.n == 0
        self.buf += data

    def getvalue(self):
        """The stream so far, the last byte zero-padded."""
        return bytes(self.buf) + (bytes([self.acc]) if self.n else b"")


def apply_tokens(tokens, prefix=b""):
    """The bytes a token list stands for (after ``prefix`` as earlier output)."""
    out = bytearray(prefix)
    for t in tokens:
        if isinstance(t, int):
            out.append(t)
        else:
            length, dist = t
            assert 1 <= dist <= len(out)
            if dist >= length:
                out += out[len(out) - dist:len(out) - dist + length]
            else:
                for _ in range(length):
                    out.append(out[-dist])
    return bytes(out[len(prefix):])


def stored_block(w, data, final, nlen=None, length=None):
    """A stored block from any bit offset; ``nlen`` / ``length`` override the fields."""
    w.bits(1 if final else 0, 1)
    w.bits(0, 2)
    w.align()
    ln = len(data) if length is None else length
    w.bits(ln, 16)
    w.bits((ln ^ 0xFFFF) if nlen is None else nlen, 16)
    w.raw(data)


def put_tokens(w, tokens, ll_lens, d_lens, eob=True):
    """The tokens (and the end-of-block code) with canonical codes of the given lengths."""
    llc, dc = canonical_codes(ll_lens), canonical_codes(d_lens)
    for t in tokens:
        if isinstance(t, int):
            assert ll_lens[t], ("literal without a code", t)
            w.code(llc[t], ll_lens[t])
        else:
            ls, lb, lv = len_symbol(t[0])
            ds, db, dv = dist_symbol(t[1])
            assert ll_lens[ls] and d_lens[ds], ("match without a code", t)
            w.code(llc[ls], ll_lens[ls])
            w.bits(lv, lb)
            w.code(dc[ds], d_lens[ds])
            w.bits(dv, db)
    if eob:
        w.code(llc[256], ll_lens[256])


def fixed_block(w, tokens, final, eob=True):
    w.bits(1 if final else 0, 1)
    w.bits(1, 2)
    put_tokens(w, tokens, FIXED_LL, FIXED_D, eob)


def fixed_symbol(w, sym):
    """One literal/length symbol 0..287 of the fixed code (286 and 287 are invalid)."""
    w.code(canonical_codes(FIXED_LL)[sym], FIXED_LL[sym])


def rle_code_lengths(seq, use_repeats=True):
    """Code-length symbols for ``seq`` (litlen lengths followed by distance lengths):
    (symbol, extra value, first index, count) per element. Runs do not stop at the
    boundary between the two tables."""
    ops, i = [], 0
    while i < len(seq):
        v, r = seq[i], 1
        while i + r < len(seq) and seq[i + r] == v:
            r += 1
        if not use_repeats:
            ops += [(v, 0, i + k, 1) for k in range(r)]
            i += r
            continue
        at = i
        i += r
        if v == 0:
            while r >= 11:
                k = min(r, 138)
                ops.append((18, k - 11, at, k))
                at, r = at + k, r - k
            if r >= 3:
                ops.append((17, r - 3, at, r))
                at, r = at + r, 0
        else:
            ops.append((v, 0, at, 1))
            at, r = at + 1, r - 1
            while r >= 3:
                k = min(r, 6)
                ops.append((16, k - 3, at, k))
                at, r = at + k, r - k
        ops += [(v, 0, at + k, 1) for k in range(r)]
    return ops


CL_EXTRA = {16: 2, 17: 3, 18: 7}


def dynamic_header(w, final, ll_lens, d_lens, *, use_repeats=True, cl_lens=None, hclen=None,
                   ops=None, hlit=None, hdist=None):
    """BFINAL, BTYPE 10 and the code tables. ``ll_lens`` has HLIT entries (257..286 for a
    valid block), ``d_lens`` HDIST entries (1..30). ``cl_lens`` (19 code-length code
    lengths), ``hclen`` (4..19), ``ops`` (the code-length symbols as (symbol, extra value)
    pairs) and the ``hlit`` / ``hdist`` counts written to the header can be forced, for
    unusual and malformed headers. Returns the ops written."""
    if ops is None:
        ops = [(s, x) for s, x, _, _ in rle_code_lengths(list(ll_lens) + list(d_lens), use_repeats)]
    if cl_lens is None:
        freq = [0] * 19
        for s, _ in ops:
            freq[s] += 1
        cl_lens = huffman_lengths(freq, 7)
    if hclen is None:
        hclen = 19
        while hclen > 4 and cl_lens[CL_ORDER[hclen - 1]] == 0:
            hclen -= 1
    w.bits(1 if final else 0, 1)
    w.bits(2, 2)
    w.bits((len(ll_lens) if hlit is None else hlit) - 257, 5)
    w.bits((len(d_lens) if hdist is None else hdist) - 1, 5)
    w.bits(hclen - 4, 4)
    for k in range(hclen):
        w.bits(cl_lens[CL_ORDER[k]], 3)
    clc = canonical_codes(cl_lens)
    for s, x in ops:
        w.code(clc[s], cl_lens[s])
        if s >= 16:
            w.bits(x, CL_EXTRA[s])
    return ops


def dynamic_block(w, tokens, final, ll_lens, d_lens, eob=True, **header):
    """A dynamic-Huffman block from caller-given code lengths (see dynamic_header)."""
    ops = dynamic_header(w, final, ll_lens, d_lens, **header)
    put_tokens(w, tokens, list(ll_lens) + [0] * (288 - len(ll_lens)),
               list(d_lens) + [0] * (32 - len(d_lens)), eob)
    return ops


def lengths_for(tokens, hlit=None, hdist=None):
    """Complete code lengths (<= 15 bits) that fit the tokens; trimmed to the smallest
    HLIT / HDIST, or padded with zeros to the given ones."""
    lf, df = [0] * 286, [0] * 30
    lf[256] = 1
    for t in tokens:
        if isinstance(t, int):
            lf[t] += 1
        else:
            lf[len_symbol(t[0])[0]] += 1
            df[dist_symbol(t[1])[0]] += 1
    ll = huffman_lengths(lf, 15)
    dl = huffman_lengths(df, 15) if any(df) else [0] * 30
    nl = max(257, max(i for i in range(286) if ll[i]) + 1) if hlit is None else hlit
    nd = max(1, max([i for i in range(30) if dl[i]] + [0]) + 1) if hdist is None else hdist
    assert not any(ll[nl:]) and not any(dl[nd:])
    return ll[:nl], dl[:nd]


def gzip_wrap(raw, body, *, fextra=None, fname=None, fcomment=None, fhcrc=None, flg_extra=0,
              crc=None, isize=None, cm=8):
    """A gzip member around the raw DEFLATE stream ``raw`` of ``body``. ``fextra`` /
    ``fname`` / ``fcomment`` are bytes (the strings without their terminator); ``fhcrc`` is
    True for the correct header checksum or an int to force one; ``flg_extra`` is OR-ed
    into FLG; ``crc`` / ``isize`` override the trailer."""
    flg = flg_extra
    flg |= 4 if fextra is not None else 0
    flg |= 8 if fname is not None else 0
    flg |= 16 if fcomment is not None else 0
    flg |= 2 if fhcrc is not None else 0
    h = bytearray([0x1F, 0x8B, cm, flg, 0, 0, 0, 0, 0, 0xFF])
    if fextra is not None:
        h += len(fextra).to_bytes(2, "little") + fextra
    if fname is not None:
        h += fname + b"\0"
    if fcomment is not None:
        h += fcomment + b"\0"
    if fhcrc is not None:
        v = (zlib.crc32(bytes(h)) & 0xFFFF) if fhcrc is True else fhcrc
        h += v.to_bytes(2, "little")
    c = zlib.crc32(body) if crc is None else crc
    n = len(body) if isize is None else isize
    return bytes(h) + raw + (c & 0xFFFFFFFF).to_bytes(4, "little") + (n & 0xFFFFFFFF).to_bytes(4, "little")


# ------------------------------------------------------------------------------------
# tracing inflater


class Block:
    """One traced block. ``tokens`` is None for a stored block (``data`` has its bytes)."""

    __slots__ = ("final", "btype", "start_bit", "end_bit", "ll_lens", "d_lens", "tokens",
                 "data", "out_start")

    def __repr__(self):
        return (f"Block(final={self.final}, btype={self.btype}, bits={self.start_bit}.."
                f"{self.end_bit}, out={self.out_start}+{len(self.data)})")


class _Reader:
    def __init__(self, raw, bit):
        self.raw = raw
        self.pos = bit >> 3
        self.acc = 0
        self.cnt = 0
        if bit & 7:
            self.bits(bit & 7)

    @property
    def bitpos(self):
        return 8 * self.pos - self.cnt

    def bits(self, n):
        while self.cnt < n:
            if self.pos >= len(self.raw):
                raise DeflateError("stream ends inside a block")
            self.acc |= self.raw[self.pos] << self.cnt
            self.pos += 1
            self.cnt += 8
        v = self.acc & ((1 << n) - 1)
        self.acc >>= n
        self.cnt -= n
        return v


class _Code:
    """Canonical decoder, strict as zlib's inflate_table: an over-subscribed set is an
    error, an incomplete one too unless ``single_ok`` and its only code has one bit."""

    def __init__(self, lengths, what, single_ok):
        self.count = count = [0] * 16
        for l in lengths:
            count[l] += 1
        count[0] = 0
        left = 1
        for b in range(1, 16):
            left = 2 * left - count[b]
            if left < 0:
                raise DeflateError(f"over-subscribed {what} set")
        mx = max([b for b in range(1, 16) if count[b]] + [0])
        if left > 0 and mx and not (single_ok and mx == 1):
            raise DeflateError(f"incomplete {what} set")
        offs = [0] * 17
        for b in range(1, 16):
            offs[b + 1] = offs[b] + count[b]
        self.symbol = [0] * offs[16]
        for s, l in enumerate(lengths):
            if l:
                self.symbol[offs[l]] = s
                offs[l] += 1

    def decode(self, r, what):
        code = first = index = 0
        for b in range(1, 16):
            code |= r.bits(1)
            c = self.count[b]
            if code - c < first:
                return self.symbol[index + code - first]
            index += c
            first = (first + c) << 1
            code <<= 1
        raise DeflateError(f"invalid {what} code")


def _read_tables(r):
    hlit, hdist, hclen = r.bits(5) + 257, r.bits(5) + 1, r.bits(4) + 4
    if hlit > 286 or hdist > 30:
        raise DeflateError("too many length or distance symbols")
    cl = [0] * 19
    for k in range(hclen):
        cl[CL_ORDER[k]] = r.bits(3)
    clc = _Code(cl, "code lengths", False)
    if not any(cl):  # zlib reads such a table as one-bit zeros; there is never an end code
        raise DeflateError("invalid code -- missing end-of-block")
    lens = []
    while len(lens) < hlit + hdist:
        s = clc.decode(r, "code lengths")
        if s < 16:
            lens.append(s)
            continue
        if s == 16:
            if not lens:
                raise DeflateError("repeat with no previous length")
            v, rep = lens[-1], 3 + r.bits(2)
        elif s == 17:
            v, rep = 0, 3 + r.bits(3)
        else:
            v, rep = 0, 11 + r.bits(7)
        if len(lens) + rep > hlit + hdist:
            raise DeflateError("repeat runs past the tables")
        lens += [v] * rep
    if lens[256] == 0:
        raise DeflateError("invalid code -- missing end-of-block")
    return lens[:hlit], lens[hlit:]


def trace(raw, *, empty_window=False, start_bit=0):
    """Decode the DEFLATE stream in ``raw`` from ``start_bit`` to its final block and return
    the list of Blocks; ``b"".join(b.data for b in blocks)`` is the output. Raises
    DeflateError on anything zlib's inflate would reject."""
    r = _Reader(raw, start_bit)
    out = bytearray()
    blocks = []
    while True:
        b = Block()
        b.start_bit = r.bitpos
        b.out_start = len(out)
        b.final = bool(r.bits(1))
        b.btype = r.bits(2)
        b.ll_lens = b.d_lens = b.tokens = None
        floor = len(out) if empty_window else 0
        if b.btype == 0:
            r.acc = r.cnt = 0
            ln, nl = r.bits(16), r.bits(16)
            if ln ^ 0xFFFF != nl:
                raise DeflateError("stored block lengths do not match")
            if r.pos + ln > len(raw):
                raise DeflateError("stream ends inside a stored block")
            out += raw[r.pos:r.pos + ln]
            r.pos += ln
        elif b.btype == 3:
            raise DeflateError("invalid block type")
        else:
            if b.btype == 1:
                ll, dl = FIXED_LL, FIXED_D
                llc, dc = _Code(ll, "literal/lengths", True), _Code(dl, "distances", True)
            else:
                ll, dl = _read_tables(r)
                llc, dc = _Code(ll, "literal/lengths", True), _Code(dl, "distances", True)
            b.ll_lens, b.d_lens, b.tokens = list(ll), list(dl), []
            toks = b.tokens
            while True:
                s = llc.decode(r, "literal/length")
                if s < 256:
                    out.append(s)
                    toks.append(s)
                elif s == 256:
                    break
                else:
                    if s > 285:
                        raise DeflateError("invalid literal/length code")
                    length = LBASE[s - 257] + r.bits(LEXT[s - 257])
                    ds = dc.decode(r, "distance")
                    if ds > 29:
                        raise DeflateError("invalid distance code")
                    dist = DBASE[ds] + r.bits(DEXT[ds])
                    if dist > len(out) - floor:
                        raise DeflateError("invalid distance too far back")
                    toks.append((length, dist))
                    if dist >= length:
                        out += out[len(out) - dist:len(out) - dist + length]
                    else:
                        for _ in range(length):
                            out.append(out[-dist])
        b.end_bit = r.bitpos
        b.data = bytes(out[b.out_start:])
        blocks.append(b)
        if b.final:
            return blocks


def inflate(raw):
    """(output, bytes consumed) of the DEFLATE stream at the start of ``raw``."""
    blocks = trace(raw)
    return b"".join(b.data for b in blocks), (blocks[-1].end_bit + 7) // 8
