"""The segmented byte mover (k_segcopy and its host twins) against a plain NumPy model.

Shared by tests/test_segcopy_model.py (CPU: the host twins, the model and the case
builders) and tests/test_segcopy_gpu.py (the kernel in every mode):

  * ``ref_segcopy``   what the destination must hold afterwards: slice assignment per segment;
  * ``plan_passes``   the partition arithmetic of the kernel's header replayed per workgroup
                      (span, r0/r1, ja/jb, the pass starts, the skip over an empty run). It
                      copies no byte: it is the coverage oracle, every case asserts from it
                      that it reaches the path it is named for on the grid it runs on;
  * case builders     the smallest shapes that reach each path, built from the geometry
                      (``core().segcopy_geometry()`` on a GPU, today's constants on the CPU);
  * runners           one case through ``ops.routing`` on any device, whole destination back.

Everything is byte-exact. ``python -m tests.segcopy_cases --device`` runs the mode-0
families on cuda:0 against the model and exits non-zero on the first mismatch (the LDS-DMA
variant is chosen per process by SHELLAC_GLDS, hence a process of its own).
"""
from __future__ import annotations

import sys
from typing import NamedTuple, Optional

import numpy as np

SKIP = -1                 # kSegSkip (all ones) in an int64 offset array
CHUNK = 16
GIB4 = 1 << 32
SLACK = 256               # sentinel bytes kept past every destination's extent

# the constants of today's kernel, for the tests that run without a GPU
TODAY = {"min_tile": 1024, "stage": 1024, "stage_sized": 768, "stage_glds": 512}
ASSUMED_GRIDS = (1, 1536, 4096)


def sentinel(n: int, start: int = 0) -> np.ndarray:
    """Position-dependent fill of destination bytes [start, start + n)."""
    i = np.arange(start, start + n, dtype=np.int64)
    return ((i * 131 + 7) & 255).astype(np.uint8)


# ----------------------------------------------------------------------------------
# the model
# ----------------------------------------------------------------------------------
def ref_window(lo, hi, src_bytes, src_off, dst_off, *, seg_len=None, cap=None, n=None,
               before=None):
    """Expected destination bytes [lo, hi) (``before``: their prior content, default the
    sentinel). Mode 0/3 (``seg_len`` None): nothing changes when dst_off[n] > cap; else
    every segment whose source is not SKIP is assigned. Mode 2: segment i writes its
    seg_len[i] bytes (never more than the room up to dst_off[i + 1]) only when
    dst_off[i] + seg_len[i] <= cap."""
    n = len(src_off) if n is None else int(n)
    out = sentinel(hi - lo, lo) if before is None else np.array(before, dtype=np.uint8)
    assert out.size == hi - lo
    if n == 0:
        return out
    cap = (1 << 64) - 1 if cap is None else int(cap)
    if seg_len is None and int(dst_off[n]) > cap:
        return out
    for i in range(n):
        d0, d1 = int(dst_off[i]), int(dst_off[i + 1])
        if seg_len is None:
            if int(src_off[i]) == SKIP:
                continue
            ln = d1 - d0
        else:
            if d0 + int(seg_len[i]) > cap:
                continue
            ln = min(int(seg_len[i]), d1 - d0)
        a, b = max(d0, lo), min(d0 + ln, hi)
        if a < b:
            s0 = int(src_off[i]) + (a - d0)
            out[a - lo:b - lo] = src_bytes[s0:s0 + (b - a)]
    return out


def ref_segcopy(dst_before, src_bytes, src_off, dst_off, *, seg_len=None, cap=None, n=None):
    """The whole expected destination (see ``ref_window``)."""
    return ref_window(0, len(dst_before), src_bytes, src_off, dst_off, seg_len=seg_len,
                      cap=cap, n=n, before=dst_before)


def tile_span(nchunks: int, grid: int, min_tile: int) -> int:
    span = (nchunks + grid - 1) // grid
    span = (span + 255) & ~255
    return max(span, min_tile)


def plan_passes(dst_off, grid: int, min_tile: int, tsc: int, n: Optional[int] = None):
    """Per workgroup that owns chunks: its chunk range, first / last segment, the pass
    starts, whether a pass start fell inside a run of empty segments and was moved to the
    run's last member (``skip``), and how many chunks of its first / last segment lie
    outside its range (``head_out`` / ``tail_out``: non-zero = the boundary is inside a
    segment)."""
    off = np.asarray(dst_off, dtype=np.int64)
    n = len(off) - 1 if n is None else int(n)
    off = off[:n + 1]
    total = int(off[n])
    nchunks = total >> 4
    span = tile_span(nchunks, grid, min_tile)
    wgs = []
    for b in range(grid):
        r0 = b * span
        r1 = min(r0 + span, nchunks)
        if r0 >= r1:
            break
        ja = int(np.searchsorted(off, r0 << 4, side="right")) - 1
        jb = int(np.searchsorted(off, (r1 << 4) - 1, side="right")) - 1
        ja, jb = max(ja, 0), max(jb, 0)
        starts, skip, skipped = [], False, 0
        j0 = ja
        while j0 <= jb:
            if ja < j0 < jb and off[j0 + 1] == off[j0]:
                last = int(np.searchsorted(off[:jb + 1], off[j0], side="right")) - 1
                skip, skipped = True, skipped + (last - j0)
                j0 = last
            starts.append(j0)
            j0 += tsc
        wgs.append({
            "wg": b, "r0": r0, "r1": r1, "ja": ja, "jb": jb, "starts": starts,
            "passes": len(starts), "skip": skip, "skipped": skipped,
            "head_out": r0 - (int(off[ja]) >> 4),
            "tail_out": (int(off[jb + 1]) >> 4) - r1,
        })
    return {"span": span, "nchunks": nchunks, "wgs": wgs}


def plan_summary(plan) -> str:
    w = plan["wgs"]
    if not w:
        return "workgroups 0"
    p = [x["passes"] for x in w]
    return (f"workgroups {len(w)} span {plan['span']} passes {min(p)}..{max(p)} "
            f"skip {sum(x['skip'] for x in w)}")


# ----------------------------------------------------------------------------------
# cases
# ----------------------------------------------------------------------------------
class Case(NamedTuple):
    src: np.ndarray
    src_off: np.ndarray      # int64, SKIP = a gap (modes 0 / 3)
    dst_off: np.ndarray      # int64 [n + 1]
    seg_len: Optional[np.ndarray]   # int64 [n], mode 2 only
    description: str
    expect: dict             # what plan_passes must report (see check_coverage)
    cap: Optional[int] = None

    @property
    def n(self) -> int:
        return len(self.src_off)

    @property
    def dst_bytes(self) -> int:
        return int(self.dst_off[-1]) + SLACK

    def sized(self, description=None) -> "Case":
        """The same shape for mode 2: every segment as long as its room."""
        assert not (self.src_off == SKIP).any()
        return self._replace(seg_len=np.diff(self.dst_off),
                             description=description or self.description)


def _src(rng, nbytes):
    return np.frombuffer(rng.bytes(nbytes), dtype=np.uint8).copy()


def _from_sizes(rng, sizes, desc, expect, src_bytes=1 << 16):
    sizes = np.asarray(sizes, dtype=np.int64)
    assert (sizes % CHUNK == 0).all()
    src_bytes = max(src_bytes, int(sizes.max(initial=0)) + CHUNK)
    src = _src(rng, src_bytes)
    room = (src_bytes - sizes) // CHUNK
    src_off = (rng.integers(0, 1 << 62, size=len(sizes)) % (room + 1)) * CHUNK
    dst_off = np.zeros(len(sizes) + 1, dtype=np.int64)
    np.cumsum(sizes, out=dst_off[1:])
    return Case(src, src_off.astype(np.int64), dst_off, None, desc, expect)


def degenerate_cases(rng, T):
    one = {"one_wg": True, "passes": 1, "skip": False}
    return [
        _from_sizes(rng, [16], "n=1 of 16 B", one),
        _from_sizes(rng, [0], "n=1 of 0 B", {"no_wg": True}),
        _from_sizes(rng, [0] * 5000, "5000 empty segments", {"no_wg": True}),
        _from_sizes(rng, [0] * 3000 + [16] + [0] * 3000, "3000 empty, 16 B, 3000 empty",
                    dict(one, ja=3000, jb=3000)),
    ]


def pass_count_cases(rng, T):
    """`count` segments in one tile: 16 B at every third index, at every pass start (so no
    pass starts in an empty run) and at the last index; the others empty."""
    out = []
    for count in (T - 1, T, T + 1, 2 * T, 2 * T + 5):
        j = np.arange(count)
        sizes = np.where((j % 3 == 0) | (j % T == 0) | (j == count - 1), 16, 0)
        out.append(_from_sizes(rng, sizes, f"{count} segments, stage {T}",
                               {"one_wg": True, "passes": -(-count // T), "skip": False,
                                "ja": 0, "jb": count - 1}))
    # three passes, the second and third beginning inside a run of empty segments
    p = 3 if T % 3 else 5
    count = 2 * T + 2 * p + 1
    sizes = np.where(np.arange(count) % p == 0, 16, 0)
    out.append(_from_sizes(rng, sizes, f"[16 B, {p - 1} empty] x {count // p + 1}, stage {T}",
                           {"one_wg": True, "passes": 3, "skip": True, "skips": 2}))
    # three tiles of [16 B, empty] pairs: workgroups whose first segment is not segment 0
    # take two passes and more (the one case of this family above one tile)
    sizes = np.where(np.arange(6 * 1024) % 2 == 0, 16, 0)
    out.append(_from_sizes(rng, sizes, "[16 B, empty] x 3072, three tiles", {"tiles": 3}))
    return out


def empty_run_cases(rng, T, min_tile):
    """T - 1 segments of 16 B, a run of R empty ones across the pass boundary, then 16-B
    segments up to one tile (and the same with the run reaching the end of the list)."""
    tail = max(1, min(8, min_tile - (T - 1)))
    out = []
    for R in (1, 2, T - 1, T, T + 1, 5 * T):
        out.append(_from_sizes(rng, [16] * (T - 1) + [0] * R + [16] * tail,
                               f"{T - 1} x 16 B, {R} empty, {tail} x 16 B",
                               {"one_wg": True, "skip": R >= 2, "passes_min": 2}))
        out.append(_from_sizes(rng, [16] * (T - 1) + [0] * R,
                               f"{T - 1} x 16 B, then {R} empty to the end",
                               {"one_wg": True, "passes": 1, "skip": False, "jb": T - 2}))
    return out


BIG_TOTAL = 65 << 20   # above 64 MiB: the span exceeds the minimum tile up to 4096 workgroups


def big_segment_case(rng):
    """One 48 MiB segment among 16 B - 4 KiB ones, 65 MiB and more in all: the workgroups
    inside the big segment start and end in the same segment."""
    small = lambda k: rng.integers(1, 257, size=k) * 16
    a, b = small(4300), small(4300)
    sizes = np.concatenate([a, [48 << 20], b])
    while sizes.sum() < BIG_TOTAL:
        sizes = np.concatenate([sizes, small(256)])
    return _from_sizes(rng, sizes, "one 48 MiB segment among 16 B - 4 KiB ones",
                       {"multi_wg": True, "inside_one_segment": True},
                       src_bytes=(48 << 20) + (1 << 16))


def boundary_case(rng, grid, min_tile):
    """65 MiB cut so that one workgroup boundary leaves exactly the first chunk of a segment
    to the workgroup before it, one leaves exactly the last chunk of a segment to the
    workgroup after it, and one coincides with a segment start."""
    nchunks = BIG_TOTAL >> 4
    span = tile_span(nchunks, grid, min_tile)
    cuts = set(range(0, nchunks + 1, (256 << 10) >> 4))
    nb = (nchunks - 1) // span   # interior boundaries
    want = {}
    if nb >= 1:
        cuts.add(1 * span - 1)   # a segment starts one chunk before boundary 1
        cuts.discard(1 * span)
        want["head_out_1"] = True
    if nb >= 2:
        cuts.add(2 * span + 1)   # a segment ends one chunk after boundary 2
        cuts.discard(2 * span)
        want["tail_out_1"] = True
    if nb >= 3:
        cuts.add(3 * span)       # a segment starts on boundary 3
        want["aligned"] = True
    c = np.array(sorted(cuts), dtype=np.int64)
    return _from_sizes(rng, np.diff(c) * 16, f"65 MiB, boundaries built for a grid of {grid}",
                       dict(want, multi_wg=True), src_bytes=1 << 20)


def skip_mix_case(rng):
    sizes = rng.integers(0, 26, size=40) * 16          # 0 - 400 B, within one tile
    c = _from_sizes(rng, sizes, "40 segments of 0 - 400 B, a third of them gaps",
                    {"one_wg": True, "passes": 1})
    c.src_off[rng.permutation(40)[:13]] = SKIP
    return c


def small_mode0_cases(rng, T, min_tile):
    """Families 1, 2, 3 and the gap mix: each within one minimum tile."""
    return (degenerate_cases(rng, T) + pass_count_cases(rng, T)
            + empty_run_cases(rng, T, min_tile) + [skip_mix_case(rng)])


def big_mode0_cases(rng, grid, min_tile):
    return [big_segment_case(rng), boundary_case(rng, grid, min_tile)]


def sized_cases(rng, T, min_tile):
    """Mode 2 only: gaps after every segment, lengths of 0 and of the whole room, and the
    drop rule at `cap`."""
    out = []
    # a gap of 16 B - 64 KiB after every segment
    ln = rng.integers(1, 129, size=40) * 16
    gap = (2 ** rng.uniform(4, 16, size=40)).astype(np.int64) // 16 * 16
    gap[0], gap[1] = 16, 64 << 10
    c = _from_sizes(rng, ln + gap, "a gap of 16 B - 64 KiB after every segment", {})
    out.append(c._replace(seg_len=ln))
    # lengths 0, part of the room, the whole room
    room = rng.integers(1, 12, size=90) * 16
    ln = room.copy()
    ln[0::3] = 0
    ln[1::3] = (room[1::3] // 32) * 16
    c = _from_sizes(rng, room, "lengths of 0, of half the room and of the whole room",
                    {"one_wg": True, "passes": 1})
    out.append(c._replace(seg_len=ln))
    # the drop rule: sizes 64 B each, segment 20 ends exactly at cap
    c = _from_sizes(rng, [64] * 40, "a segment ending exactly at cap is kept, later ones dropped",
                    {"one_wg": True, "passes": 1})
    out.append(c._replace(seg_len=np.diff(c.dst_off), cap=int(c.dst_off[21])))
    # segment 20 would end at cap + 16 and has no room of its own; segment 21 starts at the
    # same offset, is shorter, ends exactly at cap and is kept
    room = np.array([64] * 20 + [0, 48] + [64] * 10)
    c = _from_sizes(rng, room, "a segment ending at cap + 16 is dropped, the shorter next one kept",
                    {"one_wg": True, "passes": 1})
    ln = room.copy()
    ln[20] = 64
    out.append(c._replace(seg_len=ln, cap=int(c.dst_off[20]) + 48))
    # a dropped segment across the boundary of the first two tiles (any grid above 1)
    tile = min_tile * 16
    room = np.array([tile - 4096, 8192, 4096, 4096])
    c = _from_sizes(rng, room, "a dropped segment straddling a workgroup boundary",
                    {"straddle": 1})
    out.append(c._replace(seg_len=room.copy(), cap=int(c.dst_off[2]) - 16))
    return out


def check_coverage(case: Case, grid: int, min_tile: int, tsc: int):
    """Assert from plan_passes that `case` reaches what it is named for; returns the plan."""
    plan = plan_passes(case.dst_off, grid, min_tile, tsc)
    w, e, d = plan["wgs"], case.expect, case.description
    if e.get("no_wg"):
        assert not w, d
        return plan
    assert w, d
    if e.get("one_wg"):
        assert len(w) == 1 and plan["nchunks"] <= min_tile, d
    if grid == 1:   # one workgroup owns everything: no boundary to look at
        return plan
    if "tiles" in e:
        assert plan["span"] == min_tile and len(w) == e["tiles"], (d, len(w))
        assert all(x["passes"] >= 2 for x in w) and w[-1]["ja"] > 0, d
    if e.get("multi_wg"):
        assert len(w) > 1 and plan["span"] > min_tile, (d, len(w), plan["span"])
    for k in ("passes", "ja", "jb"):
        if k in e:
            assert w[0][k] == e[k], (d, k, w[0][k], e[k])
    if "passes_min" in e:
        assert w[0]["passes"] >= e["passes_min"], d
    if "skip" in e:
        assert any(x["skip"] for x in w) == e["skip"], (d, "skip")
    if "skips" in e:   # passes that began inside an empty run
        s = w[0]["starts"]
        moved = sum(1 for a, b in zip(s, s[1:]) if b - a != tsc)
        assert moved == e["skips"], (d, s)
    if e.get("inside_one_segment"):
        assert any(x["ja"] == x["jb"] and x["head_out"] > 0 and x["tail_out"] > 0 for x in w), d
    if e.get("head_out_1"):
        assert any(x["head_out"] == 1 for x in w), d
    if e.get("tail_out_1"):
        assert any(x["tail_out"] == 1 for x in w), d
    if e.get("aligned"):
        assert any(x["wg"] == 3 and x["head_out"] == 0 for x in w), d
    if "straddle" in e:
        j = e["straddle"]
        assert len(w) >= 2 and w[0]["jb"] == j and w[1]["ja"] == j and w[1]["head_out"] > 0, d
    return plan


# ----------------------------------------------------------------------------------
# runners (any device: the ops pick the kernel or the host twin)
# ----------------------------------------------------------------------------------
def run_case(case: Case, device, mode: int, cap=None, n_dev=None):
    """One case through ops.routing; returns (got, want), whole destinations.
    mode 0: segcopy; 3: segcopy_dev (absolute addresses, count in a device word);
    7: gather_segments (absolute addresses); 2: segcopy_sized."""
    import torch

    from shellac_amd.ops import routing as R

    cap = case.cap if cap is None else cap
    src = torch.from_numpy(case.src).to(device)
    so = torch.from_numpy(case.src_off).to(device)
    do = torch.from_numpy(case.dst_off).to(device)
    before = sentinel(case.dst_bytes)
    dst = torch.from_numpy(before.copy()).to(device)
    n = case.n
    if mode == 0:
        R.segcopy(src, so, do, dst, dst_cap=cap)
    elif mode in (3, 7):
        addrs = torch.where(so == SKIP, so, so + src.data_ptr())
        if mode == 7:
            R.gather_segments(addrs, do, dst)
        else:
            n = case.n if n_dev is None else n_dev
            R.segcopy_dev(addrs, do, torch.tensor([n], dtype=torch.int64, device=device), dst,
                          dst_cap=cap)
    elif mode == 2:
        R.segcopy_sized(src, so, do, torch.from_numpy(case.seg_len).to(device), dst, cap=cap)
    else:
        raise ValueError(mode)
    got = dst.cpu().numpy()
    want = ref_segcopy(before, case.src, case.src_off, case.dst_off,
                       seg_len=case.seg_len if mode == 2 else None, cap=cap, n=n)
    return got, want


def first_diff(got, want) -> str:
    if got.shape != want.shape:
        return f"shapes {got.shape} / {want.shape}"
    bad = np.flatnonzero(got != want)
    if bad.size == 0:
        return ""
    i = int(bad[0])
    return (f"{bad.size} bytes differ, first at {i} (chunk {i >> 4}): got {int(got[i])}, "
            f"want {int(want[i])}, last at {int(bad[-1])}")


def poisoned_count_case(rng):
    """Mode 3 with fewer segments than the arrays hold: the entries past the count carry
    offsets that decrease and sources full of another byte; none may show."""
    c = _from_sizes(rng, rng.integers(1, 9, size=80) * 16, "80 segments, the count says 50", {})
    n_dev = 50
    dst_off = c.dst_off.copy()
    top = int(dst_off[-1])
    dst_off[n_dev + 1:] = top - 16 * np.arange(1, 81 - n_dev)   # decreasing, inside the buffer
    src = c.src.copy()
    src[-4096:] = 0xEE
    src_off = c.src_off.copy()
    src_off[n_dev:] = len(src) - 4096
    return Case(src, src_off, dst_off, None, c.description, {}), n_dev


def run_gap_4g(device, gap=GIB4):
    """[4 KiB of segments][one `gap`-byte SKIP segment][64 KiB of segments]: the destination
    offsets after the gap lie above it. The destination is not initialised as a whole: the
    head, the tail and three 64 KiB windows of the gap hold the sentinel before and are
    compared after. Returns a list of (what, got, want)."""
    import torch

    from shellac_amd.ops import routing as R

    rng = np.random.default_rng(50)
    head = rng.integers(1, 17, size=32) * 16
    head = np.concatenate([head, [4096 - head.sum() % 4096]])
    tail = rng.integers(1, 129, size=60) * 16
    c = _from_sizes(rng, np.concatenate([head, [16], tail]), "gap", {}, src_bytes=1 << 16)
    k = len(head)
    c.src_off[k] = SKIP
    c.dst_off[k + 1:] += gap - 16
    g0, g1, end = int(c.dst_off[k]), int(c.dst_off[k + 1]), int(c.dst_off[-1])
    w = min(64 << 10, gap // 4)
    mid = (g0 + gap // 2) // 16 * 16 + 16
    windows = [("head", 0, g0), ("gap start", g0, g0 + w), ("gap middle", mid, mid + w),
               ("gap end", g1 - w, g1), ("tail", g1, end + SLACK)]
    dst = torch.empty(end + SLACK, dtype=torch.uint8, device=device)
    for _, lo, hi in windows:
        dst[lo:hi] = torch.from_numpy(sentinel(hi - lo, lo)).to(device)
    R.segcopy(torch.from_numpy(c.src).to(device), torch.from_numpy(c.src_off).to(device),
              torch.from_numpy(c.dst_off).to(device), dst)
    return [(what, dst[lo:hi].cpu().numpy(), ref_window(lo, hi, c.src, c.src_off, c.dst_off))
            for what, lo, hi in windows]


def run_src_4g(device, gap=GIB4):
    """A source of `gap` + 64 KiB bytes of which the first and the last 64 KiB hold data:
    segments alternate between the two, so every other source offset is above `gap`."""
    import torch

    from shellac_amd.ops import routing as R

    rng = np.random.default_rng(51)
    blk = 64 << 10
    lo_b, hi_b = _src(rng, blk), _src(rng, blk)
    sizes = rng.integers(1, 65, size=200) * 16
    model_off = (rng.integers(0, (blk - 1024) // 16, size=200) * 16).astype(np.int64)
    model_off[1::2] += blk                       # in the model the two blocks are adjacent
    real_off = model_off.copy()
    real_off[1::2] += gap - blk
    dst_off = np.zeros(201, dtype=np.int64)
    np.cumsum(sizes, out=dst_off[1:])
    src = torch.empty(gap + blk, dtype=torch.uint8, device=device)
    src[:blk] = torch.from_numpy(lo_b).to(device)
    src[gap:] = torch.from_numpy(hi_b).to(device)
    before = sentinel(int(dst_off[-1]) + SLACK)
    dst = torch.from_numpy(before.copy()).to(device)
    R.segcopy(src, torch.from_numpy(real_off).to(device), torch.from_numpy(dst_off).to(device), dst)
    want = ref_segcopy(before, np.concatenate([lo_b, hi_b]), model_off, dst_off)
    return [("source offsets above the gap", dst.cpu().numpy(), want)]


def geometry_for(geom: dict, mode: int, glds: bool = False):
    """(grid, min_tile, staged segments per pass) of a mode from segcopy_geometry()."""
    tsc = geom["stage_sized"] if mode == 2 else geom["stage_glds"] if glds else geom["stage"]
    return geom["grid"][mode], geom["min_tile"], tsc


# ----------------------------------------------------------------------------------
# the mode-0 families on cuda:0 in a process of their own (SHELLAC_GLDS is read once)
# ----------------------------------------------------------------------------------
def device_main() -> int:
    import torch

    from shellac_amd._native import core

    dev = torch.device("cuda", 0)
    geom = core().segcopy_geometry()
    grid, min_tile, tsc = geometry_for(geom, 0, glds=geom["glds"])
    print(f"glds {geom['glds']} grid {grid} min_tile {min_tile} stage {tsc}", flush=True)
    rng = np.random.default_rng(40)
    for c in small_mode0_cases(rng, tsc, min_tile) + big_mode0_cases(rng, grid, min_tile):
        plan = check_coverage(c, grid, min_tile, tsc)
        got, want = run_case(c, dev, 0)
        bad = first_diff(got, want)
        print(f"{'FAIL' if bad else 'ok  '} {c.description}: {plan_summary(plan)} {bad}", flush=True)
        if bad:
            return 1
    free = torch.cuda.mem_get_info(dev)[0]
    if free < (12 << 30):
        print(f"4 GiB shapes not run: {free >> 20} MiB free", flush=True)
        return 0
    for run in (run_gap_4g, run_src_4g):
        for what, got, want in run(dev):
            bad = first_diff(got, want)
            print(f"{'FAIL' if bad else 'ok  '} {run.__name__} {what} {bad}", flush=True)
            if bad:
                return 1
        torch.cuda.empty_cache()
    return 0


if __name__ == "__main__":
    if "--device" not in sys.argv:
        sys.exit("usage: python -m tests.segcopy_cases --device")
    sys.exit(device_main())
