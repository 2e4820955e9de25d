#!/usr/bin/env python3
"""Host path of a purge through HbmBackend: the time of one `purge_prefix` call on the Python
handle, from the call to its answer, for a prefix no key starts with on a small index, so
that the scan itself is a few microseconds and what is left is the request's way through the
backend: the selector, the fan-out, the batcher's flight, the launch and the completion.

One shard on GPU 0 with 1024 index slots holding 200 objects; 20 warm-up calls, then --calls
(200) timed calls. Prints one JSON line: the mean, the median and the extremes in
microseconds. Run it from two checkouts to compare them."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from shellac_amd import core  # noqa: E402


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--label", default="")
    a = ap.parse_args()
    be = core().hbm_backend([0], 64 << 20, 256, hot_objects=0, sweep_interval_s=0)
    for i in range(200):
        be.set(b"/obj/%d" % i, b"HTTP/ %d" % i, 0, 0)
    assert be.get(b"/obj/199") is not None
    for _ in range(20):
        assert be.purge_prefix(b"/nothing/") == 0
    us = []
    for _ in range(a.calls):
        t0 = time.perf_counter()
        n = be.purge_prefix(b"/nothing/")
        us.append((time.perf_counter() - t0) * 1e6)
        assert n == 0
    print(json.dumps({"bench": "purge_host_path", "label": a.label, "calls": a.calls,
                      "mean_us": round(statistics.fmean(us), 2),
                      "median_us": round(statistics.median(us), 2),
                      "min_us": round(min(us), 2), "max_us": round(max(us), 2)}))


if __name__ == "__main__":
    main()
