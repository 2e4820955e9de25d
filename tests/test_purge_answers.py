"""The HTTP answers of PURGE and /_shellac/objects, byte for byte: every mode (exact, prefix,
tag, glob) as a dry run, a soft and a hard purge, and every refusal, over a DRAM tier with and
without --grace and over the memcached tier; then the purge and inspection counters of
/_shellac/stats. The tables are in tests/purge_answer_cases.py."""
import pytest

import purge_answer_cases as pa
from shellac_amd import core
from shellac_amd.server.proxy import Server, make_backend
from shellac_amd.utils.fakemc import FakeMemcached
from shellac_amd.utils.origin import Origin


@pytest.fixture(scope="module")
def origin():
    o = Origin(body_bytes=50).start()           # never asked: no request here is a GET miss
    yield o
    o.stop()


def _check(got, sequence, want):
    assert len(got) == len(sequence) == len(want)
    for (name, _), answer in zip(sequence, got):
        assert answer == want[name], name


@pytest.mark.parametrize("config", ["dram_grace", "dram", "memcached_grace"])
def test_answers_and_counters(origin, config):
    mc = FakeMemcached().start() if config.startswith("memcached") else None
    try:
        be = (make_backend("memcached", caches=[("127.0.0.1", mc.port)]) if mc
              else make_backend("dram", dram_mb=16))
        pa.fill(be, pa.OBJECTS)
        with Server([("127.0.0.1", origin.port)], port=0, backend=be, purge="any",
                    inspect="any", tag_header=pa.TAG_HEADER,
                    grace=60 if config.endswith("grace") else 0) as px:
            _check(pa.run(px.port, pa.SEQUENCE), pa.SEQUENCE, pa.ANSWERS[config])
            assert pa.counters(px) == pa.STATS[config]
    finally:
        if mc:
            mc.stop()


def test_empty_keys_and_no_tag_header(origin):
    be = make_backend("dram", dram_mb=16)
    pa.fill(be, pa.URL_OBJECTS)
    with Server([("127.0.0.1", origin.port)], port=0, backend=be, purge="any", inspect="any",
                grace=60, key_host=False) as px:
        _check(pa.run(px.port, pa.URL_SEQUENCE), pa.URL_SEQUENCE, pa.URL_ANSWERS)
        assert pa.counters(px) == pa.URL_STATS


def test_the_loopback_rule():
    allowed = core().purge_allowed
    assert allowed("any", "10.1.2.3") and allowed("any", "127.0.0.1")
    assert allowed("loopback", "127.0.0.1") and allowed("loopback", "127.8.9.10")
    assert not allowed("loopback", "10.1.2.3") and not allowed("loopback", "128.0.0.1")
    assert not allowed("off", "127.0.0.1") and not allowed("off", "10.1.2.3")
