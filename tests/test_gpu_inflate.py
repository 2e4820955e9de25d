"""k_inflate (csrc/deflate.hip) against zlib on members zlib would never make and on
malformed ones, built bit by bit with tests/deflate_ref.py (tests/inflate_cases.py).

The oracle rule of every test: for a member m, ``d = zlib.decompressobj(31); o =
d.decompress(m, cap)``. If that raises or ``d.eof`` is false, the GPU path must answer
None; otherwise it must answer exactly ``o`` (or, where the case says so, None with
``gunzip_batch`` still returning ``o``). The GPU path must accept no more than zlib does:
the contract of ``GpuGzip::inflate`` is that whatever it declines goes through zlib, which
reports the error. Each group is one ``inflate`` call, so one launch decodes the whole
batch and the members must not disturb each other."""
import zlib

import pytest

import inflate_cases as ic

pytestmark = pytest.mark.gpu

CAP = 64 << 20


@pytest.fixture
def gz(cuda_dev):
    from shellac_amd.ops.gzip import engine

    return engine(cuda_dev.index or 0)


def check(gz, cases, cap=CAP, pinned=True):
    """One inflate call for all the cases; every answer against the oracle rule. With
    ``pinned`` zlib's verdict must also be the one the case was built for."""
    from shellac_amd.ops.gzip import gunzip_batch

    got = gz.inflate([c.member for c in cases], cap)
    assert len(got) == len(cases)
    wrong, declined = [], []
    for c, g in zip(cases, got):
        ok, o = ic.zlib_oracle(c.member, cap)
        if pinned and c.valid is not None:
            assert ok == c.valid, f"{c.name}: the case is not what it was built to be"
        if not ok:
            if g is not None:
                wrong.append(f"{c.name}: zlib rejects it, the GPU path returned {len(g)} bytes")
        elif c.must_decline or (c.may_decline and g is None):
            if g is not None:
                wrong.append(f"{c.name}: must be declined, the GPU path returned {len(g)} bytes")
            declined.append((c, o))
        elif g != o:
            wrong.append(f"{c.name}: zlib gives {len(o)} bytes, the GPU path "
                         + ("None" if g is None else f"{len(g)} other bytes"))
    assert not wrong, f"{len(wrong)} of {len(cases)} members:\n" + "\n".join(wrong)
    if declined:  # the zlib fallback still serves them
        back = gunzip_batch([c.member for c, _ in declined], gz.device, max_out=cap)
        assert back == [o for _, o in declined]


def test_copies(gz):
    """Every length, every distance 1..65, the bounds of every distance symbol, distance
    32768, copies that start at 32768 k - 258 .. 32768 k + 1 and around the output flush,
    overlapping copies at periods 1, 2, 3, 63, 64, 65: fixed-Huffman members built from
    tokens, 45 to 72 KB of output each."""
    cases = ic.copy_cases()
    assert all(c.valid and len(c.body) > 45000 for c in cases)
    check(gz, cases)


def test_stored_blocks(gz):
    cases = ic.stored_cases()
    assert all(c.valid for c in cases)
    check(gz, cases)


def test_dynamic_blocks(gz):
    cases = ic.dynamic_cases()
    assert all(c.valid for c in cases)
    check(gz, cases)


def test_ring_refill(gz):
    cases = ic.ring_cases()
    assert all(c.valid for c in cases)
    check(gz, cases)


def test_framing(gz):
    check(gz, ic.framing_cases())


def test_sizes_and_caps(gz):
    cases, isize = ic.size_cases()
    check(gz, cases, isize)
    assert all(ic.zlib_oracle(c.member, isize - 1) == (False, None) for c in cases)
    check(gz, cases, isize - 1, pinned=False)
    check(gz, cases)


def test_malformed_streams(gz):
    """One member per error exit of the kernel and per thing zlib rejects beyond those;
    the valid members in the batch still decode."""
    cases = ic.malformed_cases()
    assert sum(c.valid is False for c in cases) > 100
    check(gz, cases + ic.dynamic_cases())


def test_single_bit_flips(gz):
    cases, body = ic.bitflip_cases()
    flipped = cases[1:]
    assert len(flipped) == 692
    rejected = sum(not ic.zlib_oracle(c.member, CAP)[0] for c in flipped)
    assert rejected >= 0.9 * len(flipped), rejected  # 642 of 692; the other 50 decode unchanged
    assert zlib.decompress(cases[0].member, 31) == body
    check(gz, cases)
