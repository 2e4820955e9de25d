"""bench.py contract on the CPU: the distributed serving step rehearsed over gloo
(world 2, DRAM shards) must print exactly one well-formed JSON line and return
correct values (--check)."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    import socket

    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


@pytest.mark.parametrize("route", ["host", "device"])
def test_bench_cpu_rehearsal_world2(route):
    """host: each rank serves the requests for the keys it owns (the default); device: the
    all-to-all routed step over gloo."""
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()),
           os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "3", "--warmup", "1",
           "--device", "cpu", "--batch", "4096", "--sets", "512", "--keys-per-gpu", "32768",
           "--log-gb", "0.125", "--replicate", "4096", "--replica-gb", "0.03",
           "--sample-batches", "2", "--check", "--route", route]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd="/tmp")
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout
    out = json.loads(lines[0])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step",
              "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config"):
        assert k in out
    assert out["n_gpus"] == 2 and out["steps"] == 3 and out["warmup"] == 1
    assert out["config"]["global_batch"] == 2 * (4096 + 512)
    assert out["get_hit_ratio"] == 1.0
    assert out["config"]["routing"] == ("host" if route == "host" else "device (all-to-all)")
    assert out["config"]["replicated_hot_objects"] == (0 if route == "host" else 4096)
    assert "0 mismatches" in p.stderr
    if route == "host":
        # each rank serves its true share of the one global stream (unequal batches), hot
        # objects sprayed: the shares stay within 5 % of the mean, and the native host
        # router sends every request where the tensor routing did
        import re

        assert re.search(r"check: 0 of \d+ hit records name another key", p.stderr)
        hr = out["host_routing"]
        assert hr["rank_share_max_over_mean"] <= 1.05
        assert hr["host_route_agrees_with_device"] is True and hr["host_route_req_per_s"] > 0
        assert hr["spread_hot_objects"] > 0 and len(out["log_fresh"]["rank_ms_per_step"]) == 2
        assert sum(hr["rank_requests_per_step"]) >= 2 * (4096 + 512)
        # the headline never claims more than the host routers can feed
        cap = hr["host_route_job_capacity_req_per_s"]
        assert out["value"] == pytest.approx(min(hr["job_rate_req_per_s"], cap), rel=1e-6)
        assert hr["router_feeds_job"] == (cap >= hr["job_rate_req_per_s"])
        assert hr["value_bounded_by_router"] == (not hr["router_feeds_job"])
    else:
        assert "check: 0 of 4096 hit records name another key" in p.stderr


def test_router_bound_caps_the_host_routed_headline():
    """value = min(job rate, N x the measured router rate): router_feeds_job == False can
    no longer coexist with a headline above the routers' capacity."""
    sys.path.insert(0, ROOT)
    import bench

    out = {"value": 100.0, "ms_per_step": 2.0, "host_routing": {"rank_share_max_over_mean": 1.0}}
    r = bench.router_bound(out, 30.0, 2)  # the routers feed 60 requests/s
    hr = r["host_routing"]
    assert r["value"] == 60.0 and r["ms_per_step"] == round(2.0 * 100 / 60, 4)
    assert hr["router_feeds_job"] is False and hr["value_bounded_by_router"] is True
    assert hr["job_rate_req_per_s"] == 100.0 and hr["rank_share_max_over_mean"] == 1.0
    r = bench.router_bound(out, 80.0, 2)  # 160 >= 100: the job rate stands
    assert r["value"] == 100.0 and r["ms_per_step"] == 2.0
    assert r["host_routing"]["router_feeds_job"] is True
    assert r["host_routing"]["value_bounded_by_router"] is False


SMALL = ["--steps", "2", "--warmup", "1", "--device", "cpu", "--batch", "2048", "--sets", "256",
         "--keys-per-gpu", "8192", "--log-gb", "0.0625", "--replicate", "1024",
         "--replica-gb", "0.01", "--sample-batches", "1", "--batches", "2", "--no-uncoalesced"]


def test_bench_self_launches_ranks_without_torchrun():
    """--gpus 4 with no launcher: bench.py starts its own 4-rank child job (no exec) and
    the JSON reports 4 GPUs' worth of work."""
    env = {k: v for k, v in os.environ.items()
           if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "4", *SMALL],
                       capture_output=True, text=True, timeout=600, cwd="/tmp", env=env)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout
    out = json.loads(lines[0])
    assert out["n_gpus"] == 4
    assert out["config"]["global_batch"] == 4 * (2048 + 256)
    assert "launching 4 ranks" in p.stderr


def test_bench_rank_count_mismatch_exits_nonzero():
    """A launcher that started fewer ranks than --gpus must not yield a number."""
    env = dict(os.environ, WORLD_SIZE="1", RANK="0", LOCAL_RANK="0")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "8", *SMALL],
                       capture_output=True, text=True, timeout=300, cwd="/tmp", env=env)
    assert p.returncode != 0
    assert not [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert "refusing" in p.stderr


def test_bench_more_gpus_than_devices_exits_nonzero():
    """--gpus N on a node with fewer devices: a clear message and no number, instead of
    several ranks silently sharing a device (here: no GPU at all)."""
    env = dict(os.environ, WORLD_SIZE="2", RANK="0", LOCAL_RANK="0", HIP_VISIBLE_DEVICES="")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2",
                        "--steps", "1", "--warmup", "0"],
                       capture_output=True, text=True, timeout=300, cwd="/tmp", env=env)
    assert p.returncode == 2, p.stderr[-2000:]
    assert not [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert "GPUs on this node" in p.stderr


def test_bench_simulated_host_routed_world_cpu(tmp_path):
    """--simulate-world 4 --route host: rank 0's owner share of the Zipf stream over its
    1/4 of a 4x key space (one process, no mirrored collectives). --dump-outputs writes the
    last timed step's GET response as float arrays that agree with each other."""
    import numpy as np

    dump = tmp_path / "dump"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "2",
                        "--warmup", "1", "--device", "cpu", "--batch", "2048", "--sets", "256",
                        "--keys-per-gpu", "8192", "--log-gb", "0.125", "--batches", "2",
                        "--no-uncoalesced", "--simulate-world", "4", "--route", "host",
                        "--check", "--dump-outputs", str(dump)],
                       capture_output=True, text=True, timeout=600, cwd="/tmp")
    assert p.returncode == 0, p.stderr[-3000:]
    out = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][0])
    assert out["config"]["routing"] == "host" and out["simulated_world"] == 4
    assert out["config"]["keys_total"] == 4 * 8192
    assert out["get_hit_ratio"] == 1.0
    assert "0 mismatches" in p.stderr
    arrays = {f.stem: np.load(f) for f in dump.iterdir()}
    assert sorted(arrays) == ["record_bytesum", "records", "records_index", "request_index",
                              "size"]
    assert all(a.dtype in (np.float32, np.float64) for a in arrays.values())
    assert sum(a.nbytes for a in arrays.values()) <= 64 * 1000 * 1000
    n = arrays["size"].shape[0]
    assert n > 0 and np.array_equal(arrays["request_index"], np.arange(n))
    assert (arrays["size"] > 0).all()           # every key is held: no miss
    rows = arrays["records_index"].astype(np.int64)
    assert np.array_equal(arrays["records"].sum(axis=1), arrays["record_bytesum"][rows])
    # a record is [32-byte header | value | pad to 16]: word 4 of the header is the length
    vlen = arrays["records"][:, 16] + 256 * arrays["records"][:, 17]
    assert np.array_equal(32 + (vlen.astype(np.int64) + 15) // 16 * 16, arrays["size"][rows])


def test_capture_outputs_reads_each_request_record():
    """capture_outputs() on a hand-made response: sizes, byte sums and sampled
    records follow (off, size) of each request, a miss counts as nothing, and the sample
    is the same from call to call."""
    import numpy as np
    import torch

    sys.path.insert(0, ROOT)
    import bench
    from shellac_amd.models.sharded_cache import GetResult

    data = (torch.arange(4096, dtype=torch.int64) % 251).to(torch.uint8)
    off = torch.tensor([48, 999999, 0, 1024], dtype=torch.int64)   # request 1: a miss
    size = torch.tensor([48, 0, 32, 112], dtype=torch.int64)
    a = bench.capture_outputs(GetResult(data, off, size), max_val=80)
    assert a["size"].tolist() == [48, 0, 32, 112]
    assert set(a) == {"size", "record_bytesum", "request_index", "records", "records_index"}
    want = [float(data[o: o + s].sum()) for o, s in ((48, 48), (0, 0), (0, 32), (1024, 112))]
    assert a["record_bytesum"].tolist() == want
    assert a["records"].shape == (4, 32 + 80) and sorted(a["records_index"].tolist()) == [0, 1, 2, 3]
    for row, i in zip(a["records"], a["records_index"].astype(int)):
        o, s = int(off[i]) if size[i] else 0, int(size[i])
        assert np.array_equal(row[:s], data[o: o + s].numpy()) and not row[s:].any()
    b = bench.capture_outputs(GetResult(data, off, size), max_val=80)
    assert all(np.array_equal(a[k], b[k]) for k in a)


def test_sharded_cache_surface_bench_reads():
    """The ShardedCache surface bench.py and the tests drive, on a CPU shard at world 1:
    the names bench.py reads with their values before any step, every knob's default, and
    one serve and one get that return what a set stored."""
    import torch

    from shellac_amd.models.sharded_cache import SetBatch, ShardedCache
    from shellac_amd.ops.cache import CacheShard, digest_strings, pack_values, unpack_records

    env = {k: os.environ.pop(k, None) for k in ("SHELLAC_STOP_EVENTS", "SHELLAC_STOP_FENCE")}
    try:
        sc = ShardedCache(CacheShard(1 << 22, 1 << 12, 1 << 14, "cpu"))
    finally:
        os.environ.update({k: v for k, v in env.items() if v is not None})
    assert sc._hot is None and sc._engine is None
    assert getattr(sc, "_calibrations", 0) == 0
    assert sc.gathered_bytes == 0 and sc.routed is False and sc.world == 1
    assert sc.stats == dict.fromkeys(
        ("get_requests", "set_requests", "remote_gets", "replica_hits", "replica_refreshes",
         "coalesced_gets", "slot_overflow_rows", "reply_dropped_rows"), 0)
    sc.stats["replica_added"] = 1          # refresh_replica adds keys to the same dict
    assert sc.stats.pop("replica_added") == 1
    b = torch.tensor([[-5, 1], [0, 2], [7, 3]], dtype=torch.int64)   # sorted by lo
    a = torch.tensor([[0, 2], [7, 4], [9, 9]], dtype=torch.int64)    # same row, hi differs, absent
    assert ShardedCache._member(a, b).tolist() == [True, False, False]
    assert ShardedCache._member(a, b[:0]).tolist() == [False] * 3
    knobs = {"coalesce": True, "overlap_store": True, "event_fence": "none",
             "stop_events": True, "stop_fence": "none", "gather_after_append": False,
             "hand": "early", "host_edge": False, "host_edge_dma": True, "fused": True,
             "comm_mode": "channels", "hot_decay": 0.5, "probe_of": None}
    assert {k: vars(sc)[k] for k in knobs} == knobs   # plain attributes of the cache itself

    keys = [f"/k{i}".encode() for i in range(300)]
    v1 = [f"v1:{i}".encode() * (1 + i % 11) for i in range(300)]
    dg = digest_strings(keys)
    sc.set(SetBatch(dg, *pack_values(v1)))

    def values(res):
        return [r[0] if r else None for r in unpack_records(res.data, res.off, res.size)]

    assert values(sc.get(dg)) == v1
    # a step's GETs see the state before its SETs; the next get sees them
    v2 = [b"v2:" + k for k in keys[:100]]
    res = sc.serve(dg, SetBatch(digest_strings(keys[:100]), *pack_values(v2))).wait()
    assert values(res) == v1
    sc.sync_sets()
    assert values(sc.get(dg)) == v2 + v1[100:]
    assert values(sc.get(digest_strings([b"/absent"]))) == [None]
    assert sc.stats["get_requests"] == 901 and sc.stats["set_requests"] == 400
    assert sc._engine is None   # no routed step ran


@pytest.mark.gpu
def test_bench_host_routed_ranks_on_one_gpu():
    """The N>1 default's flow (host-routed ranks, barriers and reductions between steps,
    per-rank shard populate of different sizes) with two processes sharing the box's GPU
    over gloo: one JSON line, --check clean. (The flow once deadlocked in populate: each
    rank's cache routed over the default group.)"""
    p = subprocess.run([sys.executable, "-u", os.path.join(ROOT, "bench.py"), "--gpus", "2",
                        "--bounce", "--route", "host", "--check", "--steps", "3", "--warmup",
                        "1", "--no-uncoalesced", "--full"],
                       capture_output=True, text=True, timeout=300, cwd="/tmp",
                       env={**os.environ, "SHELLAC_BENCH_STACKS": "60"})
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout
    out = json.loads(lines[0])
    assert out["config"]["routing"] == "host" and out["n_gpus"] == 2
    # the headline is the full cache (working set 0.8 of the log: evictions, hit ratio < 1);
    # the fresh cache holds every key
    assert out["headline_phase"] == "log_pressured"
    assert out["working_set_over_capacity"] >= 0.8
    assert 0.9 <= out["get_hit_ratio"] <= 1.0
    assert out["log_fresh"]["owner_hit_ratio"] == 1.0
    assert "check: 0 mismatches in 200 sampled GETs" in p.stderr
    assert " 0 of " in p.stderr and "hit records name another key" in p.stderr


@pytest.mark.gpu
def test_bench_pooled_capacity_mode_on_one_gpu():
    """scripts/pooled_capacity.sh's mode, smaller: a fixed total key space (--keys-total) over a
    simulated 2-rank host-routed job, a 4 GiB shard log half the rank's working set (large
    enough for the hand's lead mode, layout.h hand_lead, as the bench's logs), SETs walking
    every key and fresh GET batches (--set-walk): evictions miss some requests, the replicas
    of spread hot objects stay (they are read every step), --check clean."""
    p = subprocess.run([sys.executable, "-u", os.path.join(ROOT, "bench.py"),
                        "--simulate-world", "2", "--route", "host", "--keys-total", str(16 << 20),
                        "--pressured-gb", "4", "--log-gb", "2", "--set-walk",
                        "--walk-get-batches", "32", "--overfull-fill", "0", "--check",
                        "--steps", "3", "--warmup", "1", "--no-uncoalesced", "--no-smoke", "--full"],
                       capture_output=True, text=True, timeout=300, cwd="/tmp")
    assert p.returncode == 0, p.stderr[-3000:]
    out = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][0])
    pr = out["log_pressured"]
    assert out["config"]["keys_total"] == 16 << 20
    assert pr["working_set_over_capacity"] > 1.5
    assert pr["get_batches_cycled"] == 32 and pr["set_batches_cycled"] >= 120
    # a cache holding half the keys: some misses, but the Zipf head (hot replicas included)
    # stays resident (0.67 when the CLOCK hand fell behind the overwrite and lost them)
    assert 0.85 < pr["request_hit_ratio"] < 1.0, pr
    assert "check: 0 mismatches in 200 sampled GETs" in p.stderr


@pytest.mark.gpu
def test_bench_plain_run_times_only_the_headline(tmp_path):
    """Without --full a run fills the headline's full cache, times the K steps there and
    stops: no secondary block, no smoke check; the result line keeps its headline fields,
    --check is clean and --dump-outputs holds the last timed step's response."""
    import numpy as np

    dump = tmp_path / "dump"
    p = subprocess.run([sys.executable, "-u", os.path.join(ROOT, "bench.py"), "--gpus", "1",
                        "--steps", "3", "--warmup", "1", "--keys-per-gpu", str(1 << 20),
                        "--batch", str(1 << 18), "--sets", str(1 << 14),
                        "--walk-get-batches", "16", "--check", "--dump-outputs", str(dump)],
                       capture_output=True, text=True, timeout=300, cwd="/tmp")
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout
    out = json.loads(lines[0])
    assert out["metric"] == "cache_ops_per_s" and out["unit"] == "requests/s"
    assert out["higher_is_better"] is True and out["dtype"] == "uint8"
    assert out["steps"] == 3 and out["warmup"] == 1 and out["ms_per_step"] > 0
    assert out["value"] == pytest.approx(((1 << 18) + (1 << 14)) / out["ms_per_step"] * 1e3,
                                         rel=1e-3)
    assert out["headline_phase"] == "log_pressured"
    pr = out["log_pressured"]
    assert pr["ms_per_step"] == out["ms_per_step"] and pr["stream"] == "walk"
    assert pr["fill_steps"] >= 2 * pr["set_batches_cycled"] == 128
    assert "request_hit_ratio" not in pr and "lap_steps" not in pr
    for k in ("log_fresh", "log_wrapped", "log_pressured_cycled", "log_overfull",
              "uncoalesced_ops_per_s", "hot_drift", "spread_drift"):
        assert out[k] is None, k
    assert out["smoke"] == {} and "ms_per_step_median_gpu_events" not in out
    assert "check: 0 mismatches in 200 sampled GETs" in p.stderr
    size = np.load(dump / "size.npy")
    assert size.shape == (1 << 18,) and 0.8 < (size > 0).mean() <= 1.0
    rows = np.load(dump / "records_index.npy").astype(np.int64)
    rec = np.load(dump / "records.npy")
    assert np.array_equal(rec.sum(axis=1), np.load(dump / "record_bytesum.npy")[rows])


@pytest.mark.gpu
def test_bench_spread_drift_block_on_one_gpu():
    """The spread_drift block (simulated host-routed world): each epoch drifts the
    popularity order, refreshes the spread hot set incrementally (hotspread.refresh_hot) and
    times steps of the drifted stream; the request shares stay even and every epoch reports
    what the refresh added and dropped."""
    p = subprocess.run([sys.executable, "-u", os.path.join(ROOT, "bench.py"),
                        "--simulate-world", "2", "--route", "host", "--keys-per-gpu", str(1 << 20),
                        "--drift-epochs", "2", "--spread-drift-steps", "4", "--overfull-fill", "0",
                        "--steps", "3", "--warmup", "1", "--no-uncoalesced", "--no-smoke", "--full"],
                       capture_output=True, text=True, timeout=300, cwd="/tmp")
    assert p.returncode == 0, p.stderr[-3000:]
    out = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][0])
    sd = out["spread_drift"]
    assert sd is not None and sd["epochs"] == 2 and len(sd["per_epoch"]) == 2
    for e in sd["per_epoch"]:
        assert e["hot_added"] > 0 and e["hot_added"] == e["hot_removed"]
        assert e["rank_share_max_over_mean"] < 1.05
        assert e["ms_per_step"] > 0 and 0.0 < e["request_hit_ratio"] <= 1.0
