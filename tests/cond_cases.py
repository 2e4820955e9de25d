"""Scenarios shared by tests/test_conditional.py (CPU) and tests/test_conditional_gpu.py: a
pure-Python model of the conditional sliced GET (csrc/conditional.h: where a field of the stored
head is found, which stored validators are usable, how a client's candidates compare, and what
the outcome does to a row), written from the rules and not by calling the bindings, and the runs
both twins (HostCache::get_keyed_slices on the CPU, k_slice_plan with conditions on the GPU) are checked
with. The model of the unconditional row is tests/slice_cases.py's. Every run takes explicit
`now` values, so nothing here waits for a clock."""
import itertools
import random

import numpy as np
import pytest
import torch

import slice_cases as sl
import tag_cases as tg
import touch_cases as tc
from shellac_amd import core
from shellac_amd.ops.cache import (digest_strings, keyed, pack_slice_conds, pack_slice_specs,
                                   slice_rows, tagged, unpack_slices)

T0 = sl.T0
HEAD, RANGE, FROM, SUFFIX, WHOLE = sl.HEAD, sl.RANGE, sl.FROM, sl.SUFFIX, sl.WHOLE
NONE_MATCH, MODIFIED_SINCE, IF_RANGE_ETAG, IF_RANGE_DATE = 1, 2, 3, 4   # conditional.h kCond*
KIND_NUM = {"none_match": 1, "modified_since": 2, "if_range_etag": 3, "if_range_date": 4}
LINE_MAX, VALUE_MAX, MAX_CANDIDATES = 512, 255, 16
NOT_MODIFIED = 4                                                        # slice.h kSliceNotModified
TAG, OTHER = b'"v1"', b'"v2"'
DATE, LATER = b"Wed, 21 Oct 2015 07:28:00 GMT", b"Wed, 21 Oct 2015 07:28:01 GMT"


# ------------------------------------------------------------------------------ the model
def find_field(head, name):
    """The trimmed value of the first `name` line of a head (HTTP/ through the blank line),
    None: absent."""
    e = len(head) - 4
    pat = name + b":"
    for p in range(2, e + 1):
        if head[p - 2:p] != b"\r\n" or p + len(pat) > e or head[p:p + len(pat)].lower() != pat:
            continue
        c = p + len(pat)
        q = head.index(b"\r\n", c)
        if q - c > LINE_MAX:
            return None
        return head[c:q].strip(b" \t")
    return None


def stored_etag(head):
    """(weak, opaque tag with its quotes) of a usable stored ETag, else None."""
    v = find_field(head, b"etag")
    if v is None:
        return None
    weak = v.startswith(b"W/")
    op = v[2:] if weak else v
    if not 2 <= len(op) <= VALUE_MAX or op[:1] != b'"' or op[-1:] != b'"':
        return None
    return weak, op


def stored_date(head):
    v = find_field(head, b"last-modified")
    return v if v is not None and 1 <= len(v) <= VALUE_MAX else None


def records_of(blob, ncand):
    """The candidates of ncand [u8 len | bytes] records inside blob, None: malformed."""
    if ncand > MAX_CANDIDATES:
        return None
    out, p = [], 0
    for _ in range(ncand):
        if p >= len(blob) or p + 1 + blob[p] > len(blob):
            return None
        out.append(blob[p + 1:p + 1 + blob[p]])
        p += 1 + blob[p]
    return out


def raw_of(cond):
    """(kind number, candidates as sent or None if malformed, bytes behind the row's range) of
    a condition: None, the forms of CacheShard.get_slices, or ("raw", kind, ncand, records,
    tail): a hand-made SliceCond whose range is `records` and is followed by `tail`."""
    if cond is None:
        return 0, [], b""
    if cond[0] == "raw":
        _, kind, ncand, blob, tail = cond
        return kind, records_of(blob, ncand), tail
    kind, arg = KIND_NUM[cond[0]], cond[1]
    if kind == NONE_MATCH:
        if arg == "*":
            return kind, [], b""
        return kind, [t[2:] if t.startswith(b"W/") else t for t in arg], b""
    if kind == IF_RANGE_ETAG and arg.startswith(b"W/"):
        return kind, [], b""                      # a weak tag can never match: no candidate
    return kind, [arg], b""


def matched(value, cond):
    """Whether the condition holds for the stored keyed value."""
    kind, cands, _ = raw_of(cond)
    lay = sl.layout(value)
    if lay is None or cands is None or not 1 <= kind <= 4:
        return False
    if not cands:
        return kind == NONE_MATCH                 # "*"
    head = value[lay[0]:lay[1]]
    if kind in (NONE_MATCH, IF_RANGE_ETAG):
        st = stored_etag(head)
        if st is None or (st[0] and kind == IF_RANGE_ETAG):
            return False
        return st[1] in cands
    d = stored_date(head)
    return d is not None and d in cands


def model_fields(value, spec, cond):
    """The SliceRow (without out_off) and the bytes returned of a hit under a condition."""
    kind = raw_of(cond)[0]
    if sl.layout(value) is None or not 1 <= kind <= 4:
        return sl.model_fields(value, spec)
    m = matched(value, cond)
    if kind in (NONE_MATCH, MODIFIED_SINCE):
        if not m:
            return sl.model_fields(value, spec)
        f, p = sl.model_fields(value, (HEAD,))
        return dict(f, status=NOT_MODIFIED), p
    return sl.model_fields(value, spec if m else (WHOLE,))


def model_answer(value, spec, cond, flags=sl.FLAGS, expire=0):
    f, _ = model_fields(value, spec, cond)
    if f["status"] == 3:
        return sl.model_answer(value, (WHOLE,), flags, expire)
    if f["status"] == NOT_MODIFIED:
        return dict(sl.model_answer(value, (HEAD,), flags, expire), status="not_modified")
    return sl.model_answer(value, spec, flags, expire)


def model(stored, keys, specs, conds, live=None, flags=sl.FLAGS, expire=0):
    """slice_cases.model under conditions."""
    ans, fields, hits, total, payload = [], [], 0, 0, 0
    for k, s, c in zip(keys, specs, conds):
        if k not in stored or (live is not None and k not in live):
            ans.append(dict(sl.MISS))
            fields.append(dict(sl.MISS_FIELDS, out_off=total))
            continue
        f, p = model_fields(stored[k], s, c)
        ans.append(model_answer(stored[k], s, c, flags, expire))
        fields.append(dict(f, out_off=total))
        hits += 1
        total += sl.row_bytes(f)
        payload += p
    return ans, fields, hits, total, payload


# The direct statement of RFC 9110 8.8.3.2 the comparison rules are checked against.
def rfc_opaque(tag):
    return tag[2:] if tag.startswith(b"W/") else tag


def rfc_weak_equal(a, b):
    return rfc_opaque(a) == rfc_opaque(b)


def rfc_strong_equal(a, b):
    return not a.startswith(b"W/") and not b.startswith(b"W/") and a == b


# ------------------------------------------------------------------------------- builders
def head_lines(lines, status=b"200 OK"):
    return b"HTTP/1.1 " + status + b"\r\n" + b"".join(ln + b"\r\n" for ln in lines) + b"\r\n"


STATUS_LINE = 17               # bytes of "HTTP/1.1 200 OK\r\n"
MIN_BEFORE = STATUS_LINE + 7   # the first offset line_at() can place a line at


def line_at(n, line, after=()):
    """A head whose header line `line` starts exactly n bytes into it (n >= MIN_BEFORE)."""
    pad = n - MIN_BEFORE
    assert pad >= 0, n
    h = head_lines([b"X-P: " + b"a" * pad, line, *after])
    assert h[n - 2:n + len(line)] == b"\r\n" + line
    return h


def obj(key, head, body_len=50, tags=None, seed=0):
    payload = head + sl.body_of(body_len, seed)
    return keyed(key, payload if tags is None else tagged(tags, payload))


def pack(conds, device):
    """(SliceCond rows, candidate bytes) on `device`, packed here and not by pack_slice_conds;
    a raw condition's tail lies directly behind its range."""
    rows = np.zeros((len(conds), 4), dtype=np.uint32)
    blob = bytearray()
    for i, c in enumerate(conds):
        if c is None:
            continue
        off = len(blob)
        if c[0] == "raw":
            _, kind, ncand, rec, tail = c
            blob += rec
            n = len(rec)
            blob += tail
        else:
            kind, cands, _ = raw_of(c)
            ncand = len(cands)
            for t in cands:
                blob += bytes([len(t)]) + t
            n = len(blob) - off
        rows[i] = (kind, ncand, off, n)
    b = np.frombuffer(bytes(blob), dtype=np.uint8) if blob else np.zeros(0, np.uint8)
    return (torch.from_numpy(rows.view(np.uint8).reshape(len(conds), 16).copy()).to(device),
            torch.from_numpy(b.copy()).to(device))


def slices(sh, keys, specs, conds, now=T0, digest_of=None, reserve=0, cap=None, fill=0):
    """slice_cases.slices with one condition per row (`conds` None: the unconditional call)."""
    keys = list(keys)
    d = digest_strings(digest_of if digest_of is not None else keys, sh.device)
    kb = tc.key_tensors(keys, sh.device)
    sp = torch.from_numpy(pack_slice_specs(specs).reshape(len(keys), 24)).to(sh.device)
    if cap is None:
        cap = 64 + sum(2 * sh.max_item + 64 for _ in keys)
    out = torch.full((max(cap, 16),), fill, dtype=torch.uint8, device=sh.device)[:cap]
    rows, res = sh.get_keyed_slices(d, kb, sp, out, now=now, reserve_bytes=reserve,
                                    conds=None if conds is None else pack(conds, sh.device))
    res = [int(x) for x in res.tolist()]               # (waits for the stream)
    fields = slice_rows(rows)
    ans = unpack_slices(rows, out) if res[1] <= cap else None
    return ans, fields, res, out.cpu().numpy()


def check(sh, stored, keys, specs, conds, now=T0, live=None, expire=0):
    """A batch on `sh` gives the model's rows, bytes and totals, and counts as a GET counts."""
    keys, specs, conds = list(keys), list(specs), list(conds)
    want, wfields, hits, total, payload = model(stored, keys, specs, conds, live, expire=expire)
    c0 = sh.counters()
    ans, fields, res, _ = slices(sh, keys, specs, conds, now)
    c1 = sh.counters()
    assert res == [hits, total], (sh.device, res, hits, total)
    for i, (g, w) in enumerate(zip(fields, wfields)):
        g = {k: g[k] for k in w}
        assert g == w, (sh.device, i, keys[i], specs[i], conds[i], g, w)
    for i, (g, w) in enumerate(zip(ans, want)):
        assert g == w, (sh.device, i, keys[i], specs[i], conds[i])
    assert c1["get_ops"] - c0["get_ops"] == len(keys)
    assert c1["get_hits"] - c0["get_hits"] == hits
    assert c1["get_bytes"] - c0["get_bytes"] == payload
    return ans


def check_rows(devices, objs, rows, chunk=64, **kw):
    """rows: (key, spec, cond, expected status or None). Every device answers every row as
    the model does, in batches of at most `chunk` rows, and with the status the case names."""
    kw.setdefault("nbuckets", 1 << 12)
    for sh in sl.shards_for(devices, objs, **kw):
        for i in range(0, len(rows), chunk):
            part = rows[i:i + chunk]
            ans = check(sh, objs, [r[0] for r in part], [r[1] for r in part], [r[2] for r in part])
            for r, a in zip(part, ans):
                assert r[3] is None or a["status"] == r[3], (sh.device, r, a["status"])


def both(key, spec=(RANGE, 2, 9)):
    """A stored TAG's two none_match rows: the one that matches and the one that does not."""
    return [(key, spec, ("none_match", [TAG]), "not_modified"),
            (key, spec, ("none_match", [OTHER]), "ok")]


# ----------------------------------------------------------------------------------- runs
def run_model_against_rfc():
    """The model's (and, through cond_matches, conditional.h's) comparison against RFC 9110
    8.8.3.2, exhaustively over short tag pairs: If-None-Match is the weak comparison, If-Range
    the strong one."""
    c = core()
    opaque = [b'""', b'"a"', b'"b"', b'"ab"', b'"a,b"', b'"W/"', b'"A"']
    tags = opaque + [b"W/" + t for t in opaque]
    n = 0
    for stored, client in itertools.product(tags, tags):
        v = obj(b"/k", head_lines([b"ETag: " + stored]))
        for form, rule in (("none_match", rfc_weak_equal), ("if_range_etag", rfc_strong_equal)):
            cond = (form, [client]) if form == "none_match" else (form, client)
            assert matched(v, cond) == rule(stored, client), (stored, client, form)
            kind, cands, _ = raw_of(cond)
            rec = b"".join(bytes([len(t)]) + t for t in cands)
            assert c.cond_matches(v, kind, len(cands), rec) == rule(stored, client), (stored, client)
            n += 1
    assert n == 2 * 14 * 14


def model_if_none_match(v):
    """[candidates] ('*': []) of an If-None-Match value, None: ignored. Written from the
    grammar: OWS, '*' alone, or #entity-tag with commas inside quotes belonging to the tag."""
    v = v.strip(b" \t")
    if v == b"*":
        return []
    out, i = [], 0
    while i < len(v):
        if v[i] in b" \t,":
            i += 1
            continue
        if v[i:i + 2] == b"W/":
            i += 2
        if v[i:i + 1] != b'"':
            return None
        j = i + 1
        while j < len(v) and v[j] != 0x22:
            if v[j] < 0x21 or v[j] == 0x7F:
                return None
            j += 1
        if j >= len(v):
            return None
        out.append(v[i:j + 1])
        i = j + 1
        while i < len(v) and v[i] in b" \t":
            i += 1
        if i < len(v) and v[i] != 0x2C:
            return None
    if not out or len(out) > MAX_CANDIDATES or any(len(t) > VALUE_MAX for t in out):
        return None
    return out


def run_parsers():
    """parse_if_none_match / parse_if_range / parse_if_modified_since against the rules."""
    c = core()
    big, toobig = b'"' + b"x" * 253 + b'"', b'"' + b"x" * 254 + b'"'
    cases = [b"*", b" * ", b'"a"', b'W/"a"', b'"a", "b"', b'"a","b"', b' "a" ,\tW/"b" ', b'"a,b", "c"',
             b'"a" "b"', b'"a', b'a"', b"", b" ", b",", b'"a",', b',"a"', b'"a",,"b"', b"*, \"a\"",
             b'"a", *', b'w/"a"', b'"a b"', b'"a\x7f"', b'"\xff"', big, toobig, b'W/' + big,
             b", ".join(b'"%d"' % i for i in range(16)), b", ".join(b'"%d"' % i for i in range(17)),
             b'""', b'W/""', b'"a"x', b'W/W/"a"', b'"a"\r\n']
    seen = set()
    for v in cases:
        want = model_if_none_match(v)
        got = c.parse_if_none_match(v)
        seen.add(want is None)
        if want is None:
            assert got is None, v
        else:
            kind, ncand, rec = got
            assert (kind, ncand) == (NONE_MATCH, len(want)) and records_of(rec, ncand) == want, v
    assert seen == {True, False}
    assert model_if_none_match(b'"a,b", "c"') == [b'"a,b"', b'"c"']
    assert model_if_none_match(b'W/"a"') == [b'"a"'] and model_if_none_match(toobig) is None
    for v, want in [(b'"a"', (IF_RANGE_ETAG, b'"a"')), (b' "a,b" ', (IF_RANGE_ETAG, b'"a,b"')),
                    (b'W/"a"', None), (b'"a', None), (b'"a"b', None), (b"", None), (b" \t", None),
                    (DATE, (IF_RANGE_DATE, DATE)), (b" " + DATE + b"\t", (IF_RANGE_DATE, DATE)),
                    (b"x" * 255, (IF_RANGE_DATE, b"x" * 255)), (b"x" * 256, None), (toobig, None),
                    (big, (IF_RANGE_ETAG, big))]:
        got = c.parse_if_range(v)
        if want is None:
            assert got is None, v
        else:
            assert (got[0], got[1], records_of(got[2], 1)) == (want[0], 1, [want[1]]), v
    for v, want in [(DATE, DATE), (b"  " + DATE + b" ", DATE), (b"", None), (b"x" * 256, None)]:
        got = c.parse_if_modified_since(v)
        assert (got is None) if want is None else \
            ((got[0], got[1], records_of(got[2], 1)) == (MODIFIED_SINCE, 1, [want])), v


def run_pack_slice_conds():
    """pack_slice_conds packs what this module's own packing packs."""
    conds = [None, ("none_match", [TAG]), ("none_match", "*"), ("none_match", [b'W/"a"', b'"b,c"']),
             ("modified_since", DATE), ("if_range_etag", TAG), ("if_range_etag", b"W/" + TAG),
             ("if_range_date", DATE), None, ("none_match", [b'"%d"' % i for i in range(16)])]
    rows, blob = pack_slice_conds(conds)
    wrows, wblob = pack(conds, "cpu")
    assert rows.shape == (len(conds), core().SLICE_COND_BYTES) == (len(conds), 16)
    assert (torch.from_numpy(rows.copy()) == wrows).all() and bytes(blob) == bytes(wblob.numpy())
    with pytest.raises(ValueError):
        pack_slice_conds([("none_match", [b'"%d"' % i for i in range(17)])])
    with pytest.raises(ValueError):
        pack_slice_conds([("modified_since", b"x" * 256)])
    with pytest.raises(ValueError):
        pack_slice_conds([("none_match", [])])


def run_line_phases(devices):
    """The validator's line starts at head offsets 24..39 (16 consecutive granule phases) for
    key lengths 1..16 (every head_off mod 16), with a tag block and without one, for both
    names: the row that matches is a 304, the one that does not is its window."""
    objs, rows = {}, []
    for ti, tags in enumerate((None, [b"t1", b"t2", b"t3"])):
        for klen in range(1, 17):
            for p in range(MIN_BEFORE, MIN_BEFORE + 16):
                for ni, line in enumerate((b"ETag: " + TAG, b"Last-Modified: " + DATE)):
                    k = tg.key_of_len(klen, (p - MIN_BEFORE) + 16 * ti + 32 * ni)
                    assert k not in objs
                    objs[k] = obj(k, line_at(p, line), 40, tags, seed=p)
                    ho, _ = sl.layout(objs[k])
                    assert ho == 2 + klen + (26 if tags else 0)
                    if ni == 0:
                        rows += both(k)
                    else:
                        rows += [(k, (RANGE, 2, 9), ("modified_since", DATE), "not_modified"),
                                 (k, (RANGE, 2, 9), ("modified_since", LATER), "ok")]
    assert len(objs) == 2 * 16 * 16 * 2
    check_rows(devices, objs, rows)


SEAM_AT = list(range(1008, 1027)) + list(range(2032, 2051))


def run_seams(devices):
    """The line start, the name and the colon straddle the search's 1 KiB pass boundaries: the
    line starts 1008..1026 and 2032..2050 bytes past the first granule the search loads (so
    1022..1025 and 2046..2049 among them, and every split of "etag:" and "last-modified:"
    across the boundary), for search starts of several alignments."""
    objs, rows = {}, []
    for klen in (1, 6, 13, 14, 30):
        head_off = 2 + klen
        start = (head_off + 2) & ~15
        for at in SEAM_AT:
            for ni, line in enumerate((b"eTaG:" + TAG, b"LAST-modified:\t" + DATE)):
                k = (bytes([48 + len(objs) % 76]) + b"/seam/key/padded/to/its/length")[:klen]
                if klen == 1:
                    k = bytes([48 + SEAM_AT.index(at) + 40 * ni])
                assert len(k) == klen and k not in objs
                objs[k] = obj(k, line_at(start + at - head_off, line), 37, seed=at)
                cond, no = (("none_match", [TAG]), ("none_match", [OTHER])) if ni == 0 else \
                    (("if_range_date", DATE), ("if_range_date", LATER))
                rows += [(k, (RANGE, 1, 5), cond, "not_modified" if ni == 0 else "ok"),
                         (k, (RANGE, 1, 5), no, "ok" if ni == 0 else "whole")]
    check_rows(devices, objs, rows, log_bytes=4 << 20)


def run_positions(devices):
    """The validator as the first header line and as the last one, both validators in either
    order, a head of kSliceHeadMax - 64 bytes with the ETag on its last line, and a head past
    the limit (unsliceable: whole, never a 304)."""
    et, lm = b"ETag: " + TAG, b"Last-Modified: " + DATE
    heads = {
        b"/pos/first": head_lines([et, b"X-A: b", b"X-C: d"]),
        b"/pos/last": head_lines([b"X-A: b", b"X-C: d", et]),
        b"/pos/only": head_lines([et]),
        b"/pos/both": head_lines([et, lm]),
        b"/pos/both-reversed": head_lines([b"X-A: b", lm, et]),
        b"/pos/none": head_lines([b"X-A: b"]),
        b"/pos/no-lines": head_lines([]),
    }
    objs = {k: obj(k, h) for k, h in heads.items()}
    rows = []
    for k in objs:
        has = b"none" not in k and b"no-lines" not in k
        rows += [(k, (FROM, 3), ("none_match", [TAG]), "not_modified" if has else "ok"),
                 (k, (FROM, 3), ("none_match", [OTHER]), "ok"),
                 (k, (FROM, 3), ("if_range_etag", TAG), "ok" if has else "whole"),
                 (k, (FROM, 3), ("none_match", "*"), "not_modified")]
        has = b"both" in k
        rows += [(k, (FROM, 3), ("modified_since", DATE), "not_modified" if has else "ok"),
                 (k, (FROM, 3), ("if_range_date", DATE), "ok" if has else "whole"),
                 (k, (FROM, 3), ("if_range_date", LATER), "whole")]
    check_rows(devices, objs, rows)
    n = sl.HEAD_MAX - 64
    long_ok = line_at(n - len(et) - 4, et)
    assert len(long_ok) == n
    past = line_at(sl.HEAD_MAX, et)
    big = {b"/pos/long": obj(b"/pos/long", long_ok, 100), b"/pos/past": obj(b"/pos/past", past, 100)}
    assert sl.layout(big[b"/pos/past"]) is None
    rows = []
    for cond in [("none_match", [TAG]), ("none_match", "*"), ("modified_since", DATE),
                 ("if_range_etag", TAG), ("if_range_date", DATE), ("none_match", [OTHER])]:
        rows += [(b"/pos/long", (RANGE, 0, 9), cond, None), (b"/pos/past", (RANGE, 0, 9), cond, "whole")]
    rows[0] = rows[0][:3] + ("not_modified",)
    check_rows(devices, big, rows, nbuckets=8, max_item=1 << 17, log_bytes=1 << 20)


def run_names(devices):
    """The name in any letter case; decoys that are no ETag line; duplicates: the first wins."""
    heads = {
        b"/n/ETag": ([b"ETag: " + TAG], True),
        b"/n/etag": ([b"etag: " + TAG], True),
        b"/n/ETAG": ([b"ETAG: " + TAG], True),
        b"/n/eTaG": ([b"X-A: b", b"eTaG: " + TAG], True),
        b"/n/x-etag": ([b"X-ETag: " + TAG], False),
        b"/n/in-value": ([b"X-A: b etag: " + TAG], False),
        b"/n/in-value-2": ([b"X-A: \retag: " + TAG], False),
        b"/n/blank-before-colon": ([b"ETag : " + TAG], False),
        b"/n/bare-lf": ([b"X-A: b\nETag: " + TAG], False),
        b"/n/bare-cr": ([b"X-A: b\rETag: " + TAG], False),
        b"/n/no-colon-at-end": ([b"X-A: b", b"ETag"], False),
        b"/n/cr-for-dash": ([b"Last\rModified: " + DATE], False),
        b"/n/dup-match-first": ([b"ETag: " + TAG, b"ETag: " + OTHER], True),
        b"/n/dup-match-second": ([b"ETag: " + OTHER, b"X-A: b", b"ETag: " + TAG], False),
        b"/n/dup-unusable-first": ([b"ETag: v1", b"ETag: " + TAG], False),
    }
    objs = {k: obj(k, head_lines(ls)) for k, (ls, _) in heads.items()}
    # the name at the start of the body, and as the bytes of the blank line's position
    objs[b"/n/in-body"] = keyed(b"/n/in-body", head_lines([b"X-A: b"]) + b"ETag: " + TAG + b"\r\n\r\nbody")
    objs[b"/n/body-line"] = keyed(b"/n/body-line",
                                  head_lines([b"X-A: b"]) + b"\r\nETag: " + TAG + b"\r\n\r\nbody")
    rows = []
    for k in objs:
        hit = heads.get(k, (None, False))[1]
        rows += [(k, (SUFFIX, 4), ("none_match", [TAG]), "not_modified" if hit else "ok"),
                 (k, (SUFFIX, 4), ("if_range_etag", TAG), "ok" if hit else "whole"),
                 (k, (SUFFIX, 4), ("modified_since", DATE), "ok"),
                 (k, (SUFFIX, 4), ("if_range_date", DATE), "whole")]
    rows += [(b"/n/dup-match-second", (HEAD,), ("none_match", [OTHER]), "not_modified"),
             (b"/n/dup-match-first", (HEAD,), ("none_match", [OTHER]), "ok")]
    check_rows(devices, objs, rows)


def quoted(n, fill=b"x"):
    """An opaque tag of n bytes with its quotes."""
    return b'"' + fill * (n - 2) + b'"'


def run_values(devices):
    """Tag lengths around the compare's 64-byte steps and the 255-byte limit, OWS, the 512-byte
    raw stretch, empty and unquoted values, W/ on either side under each kind, tags that differ
    in one byte, commas inside quotes."""
    objs, rows = {}, []

    def add(name, lines, cases, spec=(RANGE, 0, 3), body_len=30):
        k = b"/v/" + name
        objs[k] = obj(k, head_lines(lines), body_len)
        rows.extend((k, spec, cond, st) for cond, st in cases)

    for n in (2, 3, 15, 16, 17, 63, 64, 65, 254, 255, 256):
        t = quoted(n)
        ok = n <= VALUE_MAX
        cases = [(("raw", NONE_MATCH, 1, bytes([255]) + t[:255], b""), "ok")] if not ok else \
            [(("none_match", [t]), "not_modified"), (("if_range_etag", t), "ok")]
        if n > 2 and ok:
            cases += [(("none_match", [t[:-2] + b'y"']), "ok"), (("none_match", [b'"y' + t[2:]]), "ok"),
                      (("none_match", [t[:-2] + b'"']), "ok"), (("if_range_etag", b'"y' + t[2:]), "whole")]
        cases += [(("none_match", "*"), "not_modified")]
        add(b"len/%d" % n, [b"ETag: " + t], cases)
        add(b"weak-len/%d" % n, [b"ETag: W/" + t],
            [(("none_match", [t]) if ok else ("none_match", [OTHER]), "not_modified" if ok else "ok"),
             (("if_range_etag", t) if ok else ("if_range_etag", OTHER), "whole")])
        d = b"D" * min(n, 300)
        add(b"date-len/%d" % n, [b"Last-Modified: " + d],
            [(("modified_since", d[:255]), "not_modified" if ok else "ok"),
             (("if_range_date", d[:255]), "ok" if ok else "whole"),
             (("modified_since", d[:-1] + b"E") if ok else ("modified_since", b"E"), "ok")])
    blanks = [b"", b" ", b"\t", b" \t" * 10]
    for i, (lead, trail) in enumerate(itertools.product(blanks, blanks)):
        add(b"ows/%d" % i, [b"ETag:" + lead + TAG + trail, b"Last-Modified:" + lead + DATE + trail],
            [(("none_match", [TAG]), "not_modified"), (("none_match", [OTHER]), "ok"),
             (("modified_since", DATE), "not_modified"), (("if_range_date", DATE), "ok"),
             (("if_range_etag", TAG), "ok")])
    for raw_len in (511, 512, 513, 600):
        pad = raw_len - len(TAG)
        st = raw_len <= LINE_MAX
        add(b"stretch/lead/%d" % raw_len, [b"ETag:" + b" " * pad + TAG],
            [(("none_match", [TAG]), "not_modified" if st else "ok"),
             (("if_range_etag", TAG), "ok" if st else "whole")])
        add(b"stretch/trail/%d" % raw_len, [b"ETag:" + TAG + b"\t" * pad, b"ETag: " + TAG],
            [(("none_match", [TAG]), "not_modified" if st else "ok")])
    for i, v in enumerate([b"", b" ", b" \t ", b"v1", b'"', b'"v1', b'v1"', b"W/", b'W/"', b'w/"v1"',
                           b'W/v1', b'"v1" x']):
        add(b"unusable/%d" % i, [b"ETag:" + v, b"Last-Modified:" + (v if not v.strip() else b"")],
            [(("none_match", [v.strip() or TAG]), "ok"), (("none_match", [TAG]), "ok"),
             (("if_range_etag", TAG), "whole"), (("modified_since", DATE), "ok"),
             (("none_match", "*"), "not_modified")])
    for i, (sw, cw) in enumerate(itertools.product((b"", b"W/"), (b"", b"W/"))):
        nm = "not_modified"
        add(b"weak/%d" % i, [b"ETag: " + sw + TAG, b"Last-Modified: " + DATE],
            [(("none_match", [cw + TAG]), nm), (("none_match", [cw + OTHER]), "ok"),
             (("if_range_etag", cw + TAG), "ok" if not sw and not cw else "whole"),
             (("modified_since", cw + DATE), nm if not cw else "ok"),
             (("if_range_date", cw + DATE), "ok" if not cw else "whole"),
             # a candidate that keeps its W/ on the wire is compared byte for byte
             (("raw", NONE_MATCH, 1, bytes([len(cw + TAG)]) + cw + TAG, b""), nm if not cw else "ok")])
    add(b"comma", [b'ETag: "a,b"'],
        [(("none_match", [b'"a,b"']), "not_modified"), (("none_match", [b'"a"', b'b"']), "ok"),
         (("none_match", [b'"a', b'b"']), "ok"), (("if_range_etag", b'"a,b"'), "ok")])
    check_rows(devices, objs, rows, log_bytes=4 << 20)


def run_candidates(devices):
    """1 and 16 candidates with the match first, last and absent; '*'; no candidates under the
    other kinds; records that overrun the row's range (the bytes that would complete them lie
    directly behind it) and 17 candidates: unmatched."""
    k = b"/c/obj"
    objs = {k: obj(k, head_lines([b"ETag: " + TAG, b"Last-Modified: " + DATE]))}
    others = [b'"o%d"' % i for i in range(16)]
    nm = "not_modified"
    rec = bytes([len(TAG)]) + TAG
    cases = [
        (("none_match", [TAG]), nm), (("none_match", [OTHER]), "ok"),
        (("none_match", [TAG] + others[:15]), nm), (("none_match", others[:15] + [TAG]), nm),
        (("none_match", others[:7] + [TAG] + others[:8]), nm), (("none_match", others), "ok"),
        (("none_match", [TAG[:-1] + b"x", b"", TAG + b"x", TAG]), nm),
        (("none_match", "*"), nm),
        (("raw", MODIFIED_SINCE, 0, b"", b""), "ok"), (("raw", IF_RANGE_ETAG, 0, b"", b""), "whole"),
        (("raw", IF_RANGE_DATE, 0, b"", b""), "whole"),
        (("raw", NONE_MATCH, 0, rec, b""), nm),                       # '*' with unused bytes
        # the record's length byte says 4, the range holds 3 of them and the tail the rest
        (("raw", NONE_MATCH, 1, rec[:-1], rec[-1:]), "ok"), (("raw", NONE_MATCH, 1, rec[:1], rec[1:]), "ok"),
        (("raw", NONE_MATCH, 1, b"", rec), "ok"), (("raw", IF_RANGE_ETAG, 1, rec[:-2], rec[-2:]), "whole"),
        # a good first record, the second one overruns: the whole condition is void
        (("raw", NONE_MATCH, 2, rec + rec[:-1], rec[-1:]), "ok"),
        (("raw", NONE_MATCH, 2, rec, rec), "ok"),
        (("raw", NONE_MATCH, 17, rec * 17, b""), "ok"), (("raw", IF_RANGE_ETAG, 17, rec * 17, b""), "whole"),
        (("raw", NONE_MATCH, 16, rec * 16, b""), nm), (("raw", NONE_MATCH, 0xFFFFFFFF, rec, b""), "ok"),
        (("raw", MODIFIED_SINCE, 2, b"\x01x" + bytes([len(DATE)]) + DATE, b""), nm),
        (("raw", 5, 1, rec, b""), "ok"), (("raw", 0xFFFFFFFF, 1, rec, b""), "ok"),   # no such kind
        (("raw", 0, 1, rec, b""), "ok"),
    ]
    rows = [(k, (RANGE, 1, 2), cond, st) for cond, st in cases]
    check_rows(devices, objs, rows, chunk=65)


def run_outcomes(devices):
    """Each kind, matched and not, over every window form (an unsatisfiable range among
    them); none_match matched with a range is a 304, not a 206; values that are not sliceable,
    misses, expired entries and forged digest collisions under every kind."""
    k, e = b"/o/obj", b"/o/empty-body"
    objs = {k: obj(k, head_lines([b"ETag: " + TAG, b"Last-Modified: " + DATE]), 100),
            e: obj(e, head_lines([b"ETag: " + TAG, b"Last-Modified: " + DATE]), 0),
            b"/o/vary": keyed(b"/o/vary", tg.VARY_MARKER),
            b"/o/garbage": keyed(b"/o/garbage", b"ETag: " + TAG + b"\r\n\r\n"),
            b"/o/lflf": keyed(b"/o/lflf", b"HTTP/1.1 200 OK\nETag: " + TAG + b"\n\nbody")}
    conds = {("none_match", (TAG,)): True, ("none_match", (OTHER,)): False,
             ("modified_since", DATE): True, ("modified_since", LATER): False,
             ("if_range_etag", TAG): True, ("if_range_etag", OTHER): False,
             ("if_range_date", DATE): True, ("if_range_date", LATER): False}
    specs = {(HEAD,): "ok", (RANGE, 10, 19): "ok", (FROM, 90): "ok", (SUFFIX, 7): "ok", (WHOLE,): "whole",
             (RANGE, 100, 200): "unsat", (RANGE, 5, 2): "unsat", (SUFFIX, 0): "unsat"}
    rows = []
    for (kind, arg), m in conds.items():
        cond = (kind, list(arg)) if kind == "none_match" else (kind, arg)
        for spec, plain in specs.items():
            if kind in ("none_match", "modified_since"):
                st = "not_modified" if m else plain
            else:
                st = plain if m else "whole"
            rows.append((k, spec, cond, st))
            rows.append((e, spec, cond, {"ok": "ok" if spec == (HEAD,) else "unsat"}.get(st, st)))
        for u in (b"/o/vary", b"/o/garbage", b"/o/lflf"):
            rows.append((u, (RANGE, 0, 3), cond, "whole"))
        rows.append((b"/o/missing", (RANGE, 0, 3), cond, "miss"))
    rows.append((k, (RANGE, 0, 3), ("none_match", "*"), "not_modified"))
    rows.append((b"/o/vary", (HEAD,), ("none_match", "*"), "whole"))
    check_rows(devices, objs, rows)
    all_conds = [(kk, list(a)) if kk == "none_match" else (kk, a) for kk, a in conds] + [("none_match", "*")]
    for sh in sl.shards_for(devices, None, nbuckets=64):
        # expired
        sl.store(sh, {k: objs[k]}, expire=T0 + 100)
        check(sh, objs, [k] * len(all_conds), [(RANGE, 1, 9)] * len(all_conds), all_conds,
              now=T0 + 99, expire=T0 + 100)
        ans = check(sh, objs, [k] * len(all_conds), [(RANGE, 1, 9)] * len(all_conds), all_conds,
                    now=T0 + 100, live=set())
        assert all(a == sl.MISS for a in ans)
        # a value keyed with B stored under A's digest: a row for A is a miss under every kind,
        # and B's record, asked for under A's digest with B's key bytes, is decided
        a, b = b"/victim/object", b"/attacker/object"
        vb = obj(b, head_lines([b"ETag: " + TAG, b"Last-Modified: " + DATE]), 20)
        sl.store(sh, {b: vb}, digests={b: a})
        ans, _, res, _ = slices(sh, [a] * len(all_conds), [(RANGE, 0, 3)] * len(all_conds), all_conds)
        assert res == [0, 0] and all(x == sl.MISS for x in ans)
        ans, _, res, _ = slices(sh, [b] * len(all_conds), [(RANGE, 0, 3)] * len(all_conds), all_conds,
                                digest_of=[a] * len(all_conds))
        assert res[0] == len(all_conds)
        assert ans == [model_answer(vb, (RANGE, 0, 3), c) for c in all_conds]


def batch_objects(n, prefix=b"/b/"):
    """n objects with their own tags and dates: {key: value}, {key: (tag, date)}."""
    objs, vals = {}, {}
    for i in range(n):
        k = prefix + b"%d" % i
        vals[k] = (b'"tag-%d"' % i, b"Date %d" % i)
        lines = [b"X-I: %d" % i] * (i % 4) + [b"ETag: " + vals[k][0], b"Last-Modified: " + vals[k][1]]
        objs[k] = obj(k, head_lines(lines), 64 + i, seed=i)
    return objs, vals


def mixed_rows(objs, vals, n, seed=5, missing=True):
    rng = random.Random(seed)
    keys, specs, conds = [], [], []
    pool = list(objs) + ([b"/b/missing/1", b"/b/missing/2"] if missing else [])
    for i in range(n):
        k = rng.choice(pool)
        tag, date = vals.get(k, (TAG, DATE))
        keys.append(k)
        specs.append(rng.choice([(WHOLE,), (HEAD,), (RANGE, rng.randint(0, 40), rng.randint(0, 90)),
                                 (FROM, rng.randint(0, 100)), (SUFFIX, rng.randint(0, 100))]))
        conds.append(rng.choice([None, None, ("none_match", [tag]), ("none_match", [OTHER, tag]),
                                 ("none_match", [OTHER]), ("none_match", "*"),
                                 ("modified_since", date), ("modified_since", LATER),
                                 ("if_range_etag", tag), ("if_range_etag", b"W/" + tag),
                                 ("if_range_date", date), ("if_range_date", LATER)]))
    return keys, specs, conds


def run_batches(devices):
    """Batches of 0, 1 and 65 rows; conditional and unconditional rows mixed, duplicates of a
    key under different conditions, misses; `conds` None and all-None conditions equal the
    unconditional call row for row."""
    objs, vals = batch_objects(65)
    keys = list(objs)
    for sh in sl.shards_for(devices, objs, nbuckets=64):
        ans, fields, res, _ = slices(sh, [], [], [])
        assert ans == [] and fields == [] and res == [0, 0]
        assert sh.get_slices([], [], conds=[]) == []
        check(sh, objs, keys[:1], [(SUFFIX, 9)], [("none_match", [vals[keys[0]][0]])])
        check(sh, objs, keys[:1], [(SUFFIX, 9)], [None])
        ans = check(sh, objs, keys, [(RANGE, i, 2 * i) for i in range(65)],
                    [("none_match", [vals[k][0]]) if i % 2 else ("if_range_date", vals[k][1])
                     for i, k in enumerate(keys)])
        assert [a["status"] for a in ans] == ["ok", "not_modified"] * 32 + ["ok"]
        ks, specs, conds = mixed_rows(objs, vals, 65)
        ans = check(sh, objs, ks, specs, conds)
        assert {a["status"] for a in ans} >= {"miss", "ok", "whole", "not_modified"}
        same = [keys[3]] * 8
        ans = check(sh, objs, same, [(RANGE, 0, 9)] * 8,
                    [None, ("none_match", [vals[keys[3]][0]]), ("none_match", [OTHER]),
                     ("if_range_etag", OTHER), ("if_range_etag", vals[keys[3]][0]), None,
                     ("modified_since", vals[keys[3]][1]), ("if_range_date", LATER)])
        assert [a["status"] for a in ans] == ["ok", "not_modified", "ok", "whole", "ok", "ok",
                                              "not_modified", "whole"]
        ks, specs, _ = mixed_rows(objs, vals, 65, seed=6)
        plain = sl.slices(sh, ks, specs)
        for conds in (None, [None] * 65):
            got = slices(sh, ks, specs, conds)
            assert got[0] == plain[0] and got[1] == plain[1] and got[2] == plain[2]
            assert (got[3] == plain[3]).all()
        check(sh, objs, ks, specs, [None] * 65)


def run_out_cap(devices):
    """A response buffer that is too small: `out` is untouched, rows and totals are complete;
    one of exactly the total's bytes is filled."""
    objs, vals = batch_objects(20)
    keys = list(objs) + [b"/b/missing"]
    specs = [(RANGE, i, 3 * i + 20) for i in range(len(keys))]
    conds = [[None, ("none_match", [vals.get(k, (TAG,))[0]]), ("if_range_etag", OTHER),
              ("none_match", [OTHER])][i % 4] for i, k in enumerate(keys)]
    want, wfields, hits, total, _ = model(objs, keys, specs, conds)
    for sh in sl.shards_for(devices, objs, nbuckets=64):
        for cap in (0, 16, total - 16):
            ans, fields, res, out = slices(sh, keys, specs, conds, cap=cap, fill=0xAB)
            assert res == [hits, total] and ans is None
            assert (out == 0xAB).all(), (sh.device, cap)
            assert [{k: f[k] for k in w} for f, w in zip(fields, wfields)] == wfields
        ans, fields, res, out = slices(sh, keys, specs, conds, cap=total, fill=0xAB)
        assert res == [hits, total] and ans == want


def run_after_the_log_lapped(devices):
    """After SET batches lapped the log: every row is the model's answer for an object that
    still hits, and a miss for one that was overwritten."""
    objs, vals = batch_objects(300, b"/lap/")
    keys = list(objs)
    conds = [[("none_match", [vals[k][0]]), ("if_range_date", LATER), ("modified_since", LATER),
              ("if_range_etag", vals[k][0])][i % 4] for i, k in enumerate(keys)]
    for sh in sl.shards_for(devices, None, nbuckets=1 << 10, log_bytes=1 << 19, evict="fifo"):
        sl.store(sh, objs)
        tg.lap_the_log(sh, laps=0.75, now=T0)
        live = set(tc.live_at(sh, objs, T0))
        assert 0 < len(live) < len(objs), len(live)
        for i in range(0, 300, 60):
            check(sh, objs, keys[i:i + 60], [(RANGE, 5, 50)] * 60, conds[i:i + 60], live=live)
        tg.lap_the_log(sh, laps=0.5, now=T0)
        assert tc.live_at(sh, objs, T0) == set()
        check(sh, objs, keys[:60], [(HEAD,)] * 60, conds[:60], live=set())


def run_reference_bit(devices):
    """A not_modified hit sets the CLOCK reference bit, as a GET hit does; a miss sets none."""
    a, b = b"/ref/a", b"/ref/b"
    objs = {a: obj(a, head_lines([b"ETag: " + TAG])), b: obj(b, head_lines([b"ETag: " + TAG]))}
    nm = [("none_match", [TAG])]
    for sh in sl.shards_for(devices, objs, nbuckets=64):
        assert not sl.referenced(sh, a) and not sl.referenced(sh, b)
        slices(sh, [b"/ref/missing"], [(WHOLE,)], nm)
        slices(sh, [b"/ref/x"], [(WHOLE,)], nm, digest_of=[b])   # b's digest, another key: a miss
        assert not sl.referenced(sh, a) and not sl.referenced(sh, b)
        ans = slices(sh, [a], [(WHOLE,)], nm)[0]
        assert ans[0]["status"] == "not_modified"
        assert sl.referenced(sh, a) and not sl.referenced(sh, b)
        slices(sh, [b], [(RANGE, 0, 1)], [("if_range_etag", OTHER)])
        assert sl.referenced(sh, b)


def run_get_slices(devices):
    """The byte-string front end with conditions: the model's answers, a buffer that grows."""
    objs, vals = batch_objects(8, b"/g/")
    keys = list(objs) + [b"/g/missing"]
    t = {k: vals.get(k, (TAG, DATE)) for k in keys}
    specs = [(RANGE, 0, 9), (FROM, 60), (WHOLE,), (HEAD,), (WHOLE,), (RANGE, 5000, 6000),
             (RANGE, 0, 99999), (RANGE, 0, 0), (HEAD,)]
    conds = [("none_match", [t[keys[0]][0]]), ("none_match", [b"W/" + t[keys[1]][0], OTHER]),
             ("none_match", "*"), None, ("modified_since", t[keys[4]][1]),
             ("if_range_etag", t[keys[5]][0]), ("if_range_etag", b"W/" + t[keys[6]][0]),
             ("if_range_date", t[keys[7]][1]), ("none_match", [TAG])]
    want = model(objs, keys, specs, conds)[0]
    assert [w["status"] for w in want] == ["not_modified"] * 3 + ["ok", "not_modified", "unsat",
                                                                   "whole", "ok", "miss"]
    for sh in sl.shards_for(devices, objs, nbuckets=64):
        assert sh.get_slices(keys, specs, now=T0, conds=conds) == want
        assert sh.get_slices(keys, specs, now=T0, conds=[None] * len(keys)) == \
            sh.get_slices(keys, specs, now=T0) == sl.model(objs, keys, specs)[0]
        with pytest.raises(ValueError):
            sh.get_slices(keys, specs, now=T0, conds=conds[:-1])


# ---------------------------------------------------------------------------------- tiers
def backend_payloads():
    """{key: payload as a tier stores it}: responses with validators, plain and tagged, an
    empty body, a weak tag, no validators, a Vary marker, garbage, a big body."""
    both_lines = [b"ETag: " + TAG, b"Last-Modified: " + DATE]
    return {
        b"/p/plain": head_lines(both_lines) + sl.body_of(500, 1),
        b"/p/tagged": tagged([b"a", b"b"], line_at(61, b"etag:" + TAG, [b"Last-Modified: " + DATE])
                             + sl.body_of(333, 2)),
        b"/p/overflow": tagged([b"t%d" % i for i in range(40)], head_lines(both_lines) + sl.body_of(64, 3)),
        b"/p/empty-body": head_lines(both_lines),
        b"/p/weak": head_lines([b"ETag: W/" + TAG]) + sl.body_of(100, 5),
        b"/p/no-validators": sl.head_of(60) + sl.body_of(100, 6),
        b"/p/vary": tg.VARY_MARKER,
        b"/p/garbage": b"ETag: " + TAG + b"\r\n\r\nnot an http response at all",
        b"/p/big": line_at(1030, b"ETag: " + TAG) + sl.body_of(40000, 4),
    }


def model_part(payload, spec, cond, flags=sl.FLAGS):
    """What CacheBackend.get_parts answers for a hit on `payload` under a condition."""
    a = model_answer(keyed(b"", payload), spec, cond, flags)
    if a["status"] == "whole":
        return dict(status=3, head=b"", window=payload, body_len=0, first=0, flags=flags)
    return dict(status={"ok": 1, "unsat": 2, "not_modified": NOT_MODIFIED}[a["status"]], head=a["head"],
                window=a["window"], body_len=a["body_len"], first=a["first"], flags=flags)


PART_CONDS = [None, ("none_match", [TAG]), ("none_match", [OTHER, b"W/" + TAG]), ("none_match", [OTHER]),
              ("none_match", "*"), ("modified_since", DATE), ("modified_since", LATER),
              ("if_range_etag", TAG), ("if_range_etag", OTHER), ("if_range_etag", b"W/" + TAG),
              ("if_range_date", DATE), ("if_range_date", LATER)]


def parts(be, keys, specs, conds, digest_of=None):
    from shellac_amd.ops.cache import SLICE_KINDS
    nums = [(SLICE_KINDS[sl.norm(s)[0]],) + sl.norm(s)[1:] for s in specs]
    packed = []
    for c in conds:
        kind, cands, _ = raw_of(c)
        packed.append(None if c is None else
                      (kind, len(cands), b"".join(bytes([len(t)]) + t for t in cands)))
    got = be.get_parts(list(keys), nums, digest_of=digest_of, conds=packed)
    for g in got:
        g.pop("ttl")
    return got


def run_backend_parts(be, settle=lambda keys: None, ttl=0):
    """get_part_if on a tier: every condition form over every payload form and window kind, a
    miss, and batches that mix conditional and unconditional parts, against the model (the host
    cut and decision of the whole value)."""
    objs = backend_payloads()
    for k, v in objs.items():
        be.set(k, v, sl.FLAGS, ttl)
    settle(list(objs))
    keys = list(objs) + [b"/p/missing"]
    seen = set()
    for spec in [(sl.RANGE, 5, 20), (sl.WHOLE,), (sl.HEAD,), (sl.SUFFIX, 7), (sl.RANGE, 99999, 100000)]:
        for cond in PART_CONDS:
            got = parts(be, keys, [spec] * len(keys), [cond] * len(keys))
            want = [model_part(objs[k], spec, cond) if k in objs else sl.PART_MISS for k in keys]
            for k, g, w in zip(keys, got, want):
                assert g == w, (k, spec, cond)
                seen.add(g["status"])
    assert seen == {0, 1, 2, 3, NOT_MODIFIED}
    # all-None conditions and no conditions: get_part's answers
    assert parts(be, keys, [(sl.RANGE, 5, 20)] * len(keys), [None] * len(keys)) == \
        sl.parts(be, keys, [(sl.RANGE, 5, 20)] * len(keys))
    mixed_keys = [keys[i % len(keys)] for i in range(64)]
    mixed = [sl.PART_SPECS[(i * 7) % len(sl.PART_SPECS)] for i in range(64)]
    mconds = [PART_CONDS[(i * 5) % len(PART_CONDS)] for i in range(64)]
    got = parts(be, mixed_keys, mixed, mconds)
    want = [model_part(objs[k], s, c) if k in objs else sl.PART_MISS
            for k, s, c in zip(mixed_keys, mixed, mconds)]
    assert got == want
    return objs


# ---------------------------------------------------------------------------------- proxy
class CondOrigin(sl.RangeOrigin):
    """slice_cases.RangeOrigin whose responses carry validators: `ETag: "<path>"` (per variant
    under /vary/, weak under /weak/), `Last-Modified: DATE` and `Expires`; /missing/* is a
    cacheable 404. It ignores the client's conditions itself (every answer is in full), and
    counts its requests per (method, path)."""

    def __init__(self):
        import gzip
        import threading
        from collections import Counter
        from http.server import BaseHTTPRequestHandler, ThreadingHTTPServer
        self.hits = Counter()
        outer = self

        class H(BaseHTTPRequestHandler):
            protocol_version = "HTTP/1.1"
            disable_nagle_algorithm = True

            def log_message(self, *a):
                pass

            def _reply(self, head):
                outer.hits[(self.command, self.path)] += 1
                ua = self.headers.get("User-Agent")
                body = outer.body(self.path, ua)
                self.send_response(404 if self.path.startswith("/missing/") else 200)
                self.send_header("Content-Type", "application/octet-stream")
                self.send_header("Accept-Ranges", "bytes")
                self.send_header("Cache-Control", "max-age=600")
                self.send_header("ETag", outer.etag(self.path, ua).decode())
                self.send_header("Last-Modified", DATE.decode())
                self.send_header("Expires", "Thu, 01 Jan 2099 00:00:00 GMT")
                self.send_header("X-Private", "not for a 304")
                if self.path.startswith("/vary/"):
                    self.send_header("Vary", "User-Agent")
                if self.path.startswith("/gz/") and "gzip" in (self.headers.get("Accept-Encoding") or ""):
                    body = gzip.compress(body)
                    self.send_header("Content-Encoding", "gzip")
                self.send_header("Content-Length", str(len(body)))
                self.end_headers()
                if not head:
                    self.wfile.write(body)

            def do_GET(self):
                self._reply(False)

            def do_HEAD(self):
                self._reply(True)

        class S(ThreadingHTTPServer):
            daemon_threads = True
            allow_reuse_address = True

        self._srv = S(("127.0.0.1", 0), H)
        self.port = self._srv.server_address[1]
        self._th = threading.Thread(target=self._srv.serve_forever, daemon=True)

    @staticmethod
    def etag(path, ua=None):
        t = b'"' + path.encode() + (b"|" + ua.encode() if ua and path.startswith("/vary/") else b"") + b'"'
        return b"W/" + t if path.startswith("/weak/") else t


NOT_MODIFIED_HEADERS = {"server", "cache-control", "date", "etag", "expires", "last-modified", "vary",
                        "connection"}


def is_304(resp, etag, vary=False):
    """`resp` (status, headers, body) is the 304 the proxy builds: exactly the listed headers."""
    st, h, b = resp
    assert (st, b) == (304, b""), (st, len(b))
    want = NOT_MODIFIED_HEADERS - (set() if vary else {"vary"})
    assert set(h) == want, sorted(h)
    assert h["etag"].encode() == etag and h["last-modified"].encode() == DATE
    assert h["cache-control"] == "max-age=600" and h["connection"] == "keep-alive"
    return True


def proxy_conditional_round_trip(px, origin, settle=lambda paths: None):
    """--conditional-hits (with --partial-hits) over any tier: the 304, 200 and 206 answers to
    If-None-Match, If-Modified-Since and Range + If-Range, a Vary'd URL, a gzip-coded object, a
    stored 404, a HEAD, pipelined order and the counters. `settle(paths)` runs after a fill."""
    from shellac_amd.utils.httpclient import HttpClient
    c = HttpClient(port=px.port)
    fetch = sl.fetch
    p = "/c/1"
    full, tag = CondOrigin.body(p), CondOrigin.etag(p).decode()
    n = len(full)
    st, h, b = fetch(c, p, {"If-None-Match": tag})                 # a miss: answered in full
    assert (st, b) == (200, full)
    settle([p])
    asked = lambda: origin.hits[("GET", p)]
    assert asked() == 1
    # If-None-Match
    for inm in (tag, "*", "W/" + tag, '"x", %s' % tag, ", ".join(['"t%d"' % i for i in range(15)] + [tag]),
                ' "a,b" ,\t%s ' % tag):
        assert is_304(fetch(c, p, {"If-None-Match": inm}), tag.encode()), inm
    n304 = 6
    for inm in ('"other"', ", ".join('"t%d"' % i for i in range(16)), '"x" %s' % tag, tag[:-1], "",
                ", ".join(['"t%d"' % i for i in range(16)] + [tag])):       # no match, or malformed
        st, h, b = fetch(c, p, {"If-None-Match": inm})
        assert (st, b) == (200, full) and h["etag"] == tag, inm
    # If-Modified-Since: the exact Last-Modified value only; ignored beside If-None-Match
    assert is_304(fetch(c, p, {"If-Modified-Since": DATE.decode()}), tag.encode())
    assert is_304(fetch(c, p, {"If-Modified-Since": " " + DATE.decode() + " "}), tag.encode())
    assert fetch(c, p, {"If-Modified-Since": LATER.decode()})[::2] == (200, full)
    assert fetch(c, p, {"If-None-Match": '"other"', "If-Modified-Since": DATE.decode()})[::2] == (200, full)
    assert is_304(fetch(c, p, {"If-None-Match": tag, "If-Modified-Since": LATER.decode()}), tag.encode())
    n304 += 3
    # If-Match / If-Unmodified-Since: answered as today
    assert fetch(c, p, {"If-Match": tag, "If-None-Match": tag})[::2] == (200, full)
    assert fetch(c, p, {"If-Unmodified-Since": DATE.decode(), "If-Modified-Since": DATE.decode()})[::2] == \
        (200, full)
    st, h, b = fetch(c, p, {"If-Match": tag, "Range": "bytes=0-3"})
    assert (st, b) == (206, full[:4])
    assert fetch(c, p, {"If-Match": tag, "Range": "bytes=0-3", "If-Range": tag})[::2] == (200, full)
    # Range + If-Range
    st, h, b = fetch(c, p, {"Range": "bytes=5-20", "If-Range": tag})
    assert (st, b) == (206, full[5:21]) and h["content-range"] == "bytes 5-20/%d" % n
    st, h, b = fetch(c, p, {"Range": "bytes=-7", "If-Range": DATE.decode()})
    assert (st, b) == (206, full[-7:]) and h["content-range"] == "bytes %d-%d/%d" % (n - 7, n - 1, n)
    st, h, b = fetch(c, p, {"Range": "bytes=%d-" % n, "If-Range": tag})
    assert st == 416 and h["content-range"] == "bytes */%d" % n
    for ifr in ('"changed"', "W/" + tag, LATER.decode(), tag[:-1]):
        st, h, b = fetch(c, p, {"Range": "bytes=5-20", "If-Range": ifr})
        assert (st, b) == (200, full) and "content-range" not in h, ifr
    assert fetch(c, p, {"Range": "bytes=0-1,3-4", "If-Range": tag})[::2] == (200, full)
    assert is_304(fetch(c, p, {"Range": "bytes=5-20", "If-None-Match": tag}), tag.encode())
    assert is_304(fetch(c, p, {"Range": "bytes=5-20", "If-Range": tag, "If-None-Match": tag}), tag.encode())
    assert fetch(c, p, {"Range": "bytes=5-20", "If-Range": tag, "If-None-Match": '"o"'})[::2] == (200, full)
    st, h, b = fetch(c, p, {"Range": "bytes=5-20", "If-None-Match": '"o"'})
    assert (st, b) == (206, full[5:21])
    n304 += 2
    assert asked() == 1
    # a weak stored tag: If-None-Match matches it, If-Range never does
    wfull, wtag = CondOrigin.body("/weak/1"), CondOrigin.etag("/weak/1").decode()
    assert fetch(c, "/weak/1")[2] == wfull
    settle(["/weak/1"])
    assert is_304(fetch(c, "/weak/1", {"If-None-Match": wtag[2:]}), wtag.encode())
    assert is_304(fetch(c, "/weak/1", {"If-None-Match": wtag}), wtag.encode())
    assert fetch(c, "/weak/1", {"Range": "bytes=0-3", "If-Range": wtag[2:]})[::2] == (200, wfull)
    n304 += 2
    # a Vary'd URL: the variant's validators decide
    va, ta = CondOrigin.body("/vary/1", "ua-a"), CondOrigin.etag("/vary/1", "ua-a").decode()
    tb = CondOrigin.etag("/vary/1", "ua-b").decode()
    assert fetch(c, "/vary/1", {"User-Agent": "ua-a"})[2] == va
    settle(["/vary/1"])
    assert is_304(fetch(c, "/vary/1", {"User-Agent": "ua-a", "If-None-Match": ta}), ta.encode(), vary=True)
    assert fetch(c, "/vary/1", {"User-Agent": "ua-a", "If-None-Match": tb})[::2] == (200, va)
    st, h, b = fetch(c, "/vary/1", {"User-Agent": "ua-a", "Range": "bytes=3-40", "If-Range": ta})
    assert (st, b) == (206, va[3:41])
    assert origin.hits[("GET", "/vary/1")] == 1
    n304 += 1
    # a gzip-coded object and a client without gzip: decoded, 200
    gz, tg_ = CondOrigin.body("/gz/1"), CondOrigin.etag("/gz/1").decode()
    assert fetch(c, "/gz/1", {"Accept-Encoding": "gzip"})[2] == gz
    settle(["/gz/1"])
    st, h, b = fetch(c, "/gz/1", {"If-None-Match": tg_})
    assert (st, b) == (200, gz) and "content-encoding" not in h
    assert is_304(fetch(c, "/gz/1", {"If-None-Match": tg_, "Accept-Encoding": "gzip"}), tg_.encode(),
                  vary=True)                            # (a gzip-coded fill is stored with a Vary line)
    assert origin.hits[("GET", "/gz/1")] == 1
    n304 += 1
    # a stored 404: no 304
    nf, tn = CondOrigin.body("/missing/1"), CondOrigin.etag("/missing/1").decode()
    assert fetch(c, "/missing/1")[::2] == (404, nf)
    settle(["/missing/1"])
    assert fetch(c, "/missing/1", {"If-None-Match": tn})[::2] == (404, nf)
    assert fetch(c, "/missing/1", {"If-None-Match": "*"})[::2] == (404, nf)
    assert origin.hits[("GET", "/missing/1")] == 1
    # HEAD (served from the cache under --partial-hits and policy rfc)
    assert is_304(fetch(c, p, {"If-None-Match": tag}, method="HEAD"), tag.encode())
    st, h, b = fetch(c, p, {"If-None-Match": '"o"'}, method="HEAD")
    assert (st, b) == (200, b"") and h["content-length"] == str(n) and origin.hits[("HEAD", p)] == 0
    n304 += 1
    # pipelined: the answers come back in request order
    reqs = [(p, {"If-None-Match": tag}), (p, {}), (p, {"Range": "bytes=1-3", "If-Range": tag}),
            ("/c/miss-in-between", {"If-None-Match": tag}), (p, {"If-Modified-Since": DATE.decode()}),
            (p, {"Range": "bytes=1-3", "If-Range": '"o"'}), (p, {"If-None-Match": '"o"'})]
    c.send(b"".join(HttpClient.request_bytes(pp, headers=hd) for pp, hd in reqs))
    got = [c.read_response() for _ in reqs]
    assert [r.status() for r in got] == [304, 200, 206, 200, 304, 200, 200]
    assert [r.body().read() for r in got] == [b"", full, full[1:4], CondOrigin.body("/c/miss-in-between"),
                                              b"", full, full]
    n304 += 2
    assert asked() == 1
    st = px.stats()
    assert st["not_modified_304"] == n304
    assert st["if_range_matched"] == 3 + 1 + 1 and st["if_range_failed"] == 4 + 1 + 1
    assert st["conditional_requests"] > st["not_modified_304"] + st["if_range_matched"]
    text = HttpClient(port=px.port).get("/_shellac/metrics").body().read().decode()
    assert "shellac_not_modified_304 %d" % n304 in text and "shellac_conditional_requests " in text
    assert "shellac_if_range_matched 5" in text and "shellac_if_range_failed 6" in text
    c.close()
    return st
