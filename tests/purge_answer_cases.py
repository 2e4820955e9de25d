"""The case tables of tests/test_purge_answers.py: a fixed set of stored objects, a fixed
sequence of PURGE and /_shellac/objects requests, and for each proxy configuration the answers
(status, reason phrase, body) and the counters of /_shellac/stats afterwards, as literals. The
literals follow the documented answer formats; the order of a handler's checks and which
counters move on which path are what the tables pin."""
from shellac_amd.ops.cache import tagged
from shellac_amd.utils.httpclient import HttpClient

TAG_HEADER = "Surrogate-Key"
SEP = b"\x1f"
MANY = [b"m%d" % i for i in range(40)]               # more than 32 tags: the overflow block

# key -> payload as stored (the proxy never parses them on these paths)
OBJECTS = {
    b"localhost/a/1.css": b"HTTP/ a1",
    b"localhost/a/2.css": tagged([b"x", b"y"], b"HTTP/ a2"),
    b"localhost/a/3.js": tagged([b"y"], b"HTTP/ a3"),
    b"localhost/b/1.css": b"HTTP/ b1",
    b"localhost/b/2.js": tagged([b"z"], b"HTTP/ b2"),
    b"localhost/v/page": b"\x01X-Lang",                                   # a Vary marker
    b"localhost/v/page" + SEP + b"de": tagged([b"x"], b"HTTP/ v de"),
    b"localhost/v/page" + SEP + b"fr": b"HTTP/ v fr",
    b"other.example/a/1.css": b"HTTP/ o1",
    b"other.example/a/2.css": tagged([b"y"], b"HTTP/ o2"),
    b"localhost/many": tagged(MANY, b"HTTP/ many"),
    b"localhost/c/only": b"HTTP/ only",
}
# the second proxy keys by the URL alone (key_host off), so a request line without a URL
# reaches the handlers with an empty key
URL_OBJECTS = {b"/k/1": b"HTTP/ k1", b"/k/2": b"HTTP/ k2", SEP + b"odd": b"HTTP/ odd"}

COUNTERS = ["purge_requests", "purged_objects", "purge_denied", "soft_purge_requests",
            "softened_objects", "tag_purge_requests", "tag_purged_objects",
            "tag_softened_objects", "purge_glob_requests", "inspect_requests", "purge_dry_runs"]


def fill(be, objects):
    for k, v in objects.items():
        be.set(k, v, 1 << 31, 500)


def purge(path, mode=None, soft=False, dry=False, tags=None, host=None):
    h = {}
    if host:
        h["Host"] = host
    if mode:
        h["X-Purge-Mode"] = mode
    if soft:
        h["X-Purge-Soft"] = "1"
    if dry:
        h["X-Purge-Dry-Run"] = "1"
    if tags is not None:
        h[TAG_HEADER] = tags
    return ("PURGE", path, h)


def inspect(query):
    return ("GET", "/_shellac/objects" + query, {})


T65 = ",".join("t%d" % i for i in range(65))
T64 = ",".join("t%d" % i for i in range(64))
STARS9 = "/" + "*/" * 9
LONG = "/" + "a" * 1020                               # with "localhost": 1030 literal bytes

# (name, request): the order matters, later answers count what earlier purges left
SEQUENCE = [
    ("dry exact", purge("/v/page", dry=True)),
    ("dry prefix", purge("/a/", "prefix", dry=True)),
    ("dry tag", purge("/ignored", "tag", dry=True, tags="y")),
    ("dry glob", purge("/*.css", "glob", dry=True)),
    ("dry prefix other host", purge("/a/", "prefix", dry=True, host="other.example")),
    ("soft exact", purge("/v/page", soft=True)),
    ("soft prefix", purge("/a/", "Prefix", soft=True)),
    ("soft tag", purge("/ignored", "tag", soft=True, tags="z nobody")),
    ("soft glob", purge("/b/*", "glob", soft=True)),
    ("hard tag", purge("/ignored", "TAG", tags="x")),
    ("hard exact", purge("/v/page")),
    ("hard exact again", purge("/v/page")),
    ("hard prefix", purge("/a/", "prefix")),
    ("hard glob", purge("/*/*.js", "glob")),
    ("hard prefix other host", purge("/a/", "prefix", host="other.example")),
    ("dry exact no variants", purge("/c/only", dry=True)),
    ("dry glob, soft ignored", purge("/c/*", "glob", dry=True, soft=True)),
    ("unknown mode is exact", purge("/c/nothing", "regex")),
    ("tag: no header", purge("/ignored", "tag")),
    ("tag: separators only", purge("/ignored", "tag", tags=" ,\t, ")),
    ("tag: 65 tags", purge("/ignored", "tag", tags=T65)),
    ("tag: 65 tags soft", purge("/ignored", "tag", tags=T65, soft=True)),
    ("tag: 64 tags", purge("/ignored", "tag", tags=T64)),
    ("dry tag: no header", purge("/ignored", "tag", dry=True)),
    ("dry tag: 65 tags", purge("/ignored", "tag", dry=True, tags=T65)),
    ("glob: 9 stars", purge(STARS9, "glob")),
    ("glob: 9 stars soft", purge(STARS9, "glob", soft=True)),
    ("glob: 9 stars dry", purge(STARS9, "glob", dry=True)),
    ("glob: 1030 literal bytes", purge(LONG, "glob")),
    ("glob: backslash is literal", purge("/c/\\*", "glob")),
    ("inspect all", inspect("?limit=0")),
    ("inspect prefix", inspect("?prefix=localhost/&limit=0")),
    ("inspect key", inspect("?key=localhost/c/only&limit=0")),
    ("inspect tag", inspect("?tag=z,y&limit=0")),
    ("inspect glob", inspect("?glob=*only&limit=0")),
    # (no cursor is bad to the DRAM tier, where it means "after this key": this pins a 200
    # listing and is no cover for the 400 "bad cursor" answer, which only a cursor the HBM tier
    # refuses can draw; tests/test_list_gpu.py checks that tier's refusal on the handle)
    ("inspect cursor", inspect("?prefix=localhost/&limit=0&after=%FFnot-a-key")),
    ("inspect: empty prefix", inspect("?prefix=")),
    ("inspect: empty key", inspect("?key=")),
    ("inspect: no tags", inspect("?tag=,")),
    ("inspect: 65 tags", inspect("?tag=" + T65)),
    ("inspect: glob stars only", inspect("?glob=**")),
    ("inspect: glob empty", inspect("?glob=")),
    ("inspect: glob dangling", inspect("?glob=a%5C")),
    ("inspect: glob 9 stars", inspect("?glob=" + "*a" * 9)),
    ("inspect: glob long", inspect("?glob=" + "a" * 1025)),
    ("inspect: bad limit", inspect("?limit=4097")),
    ("inspect: unknown parameter", inspect("?what=1")),
    ("inspect: two selectors", inspect("?prefix=a&key=b")),
    ("inspect: bad escape", inspect("?prefix=%zz")),
]

# the second proxy: no --tag-header, keys without the host, the URL may be empty
URL_SEQUENCE = [
    ("empty key: dry exact", purge("", dry=True)),
    ("empty key: dry prefix", purge("", "prefix", dry=True)),
    ("empty key: dry glob", purge("", "glob", dry=True)),
    ("empty key: soft exact", purge("", soft=True)),
    ("empty key: soft prefix", purge("", "prefix", soft=True)),
    ("empty key: soft glob", purge("", "glob", soft=True)),
    ("empty key: exact", purge("")),
    ("empty key: prefix", purge("", "prefix")),
    ("empty key: glob", purge("", "glob")),
    ("stars only: glob", purge("**", "glob")),
    ("stars only: dry glob", purge("*", "glob", dry=True)),
    ("no tag header: tag", purge("/k/1", "tag", tags="a")),
    ("no tag header: soft tag", purge("/k/1", "tag", tags="a", soft=True)),
    ("no tag header: dry tag", purge("/k/1", "tag", tags="a", dry=True)),
    ("no tag header: inspect", inspect("?tag=a")),
    ("prefix still works", purge("/k/", "prefix", dry=True)),
]


def run(port, sequence):
    """[(status, reason, body)] of the sequence's requests, one connection."""
    c = HttpClient(port=port)
    out = []
    for _, (method, path, headers) in sequence:
        r = c.get(path, method=method, headers=headers)
        out.append((r.status(), r.message(), r.body().read().decode("latin-1")))
    c.close()
    return out


def counters(px):
    st = px.stats()
    return {k: st[k] for k in COUNTERS}


# ---- the answers --------------------------------------------------------------------------
NO_TAGS = (400, "Bad Request", '{"mode":"tag","error":"the request names no tags"}\n')
TOO_MANY = (400, "Bad Request", '{"mode":"tag","error":"more than 64 tags"}\n')
NO_TAG_HEADER = (400, "Bad Request", '{"mode":"tag","error":"no tag header is configured"}\n')
STARS = (400, "Bad Request", '{"mode":"glob","error":"glob: more than 8 stars"}\n')
LITERAL = (400, "Bad Request", '{"mode":"glob","error":"glob: more than 1024 literal bytes"}\n')
STARS_ONLY = (400, "Bad Request", '{"mode":"glob","error":"glob: stars only (that is a flush)"}\n')
EMPTY_GLOB = (400, "Bad Request", '{"mode":"glob","error":"glob: empty pattern"}\n')
DANGLING = (400, "Bad Request", '{"mode":"glob","error":"glob: dangling backslash"}\n')
BAD_QUERY = (400, "Bad Request", '{"error":"bad query"}\n')
BAD_PATTERN = (400, "Bad Request", '{"error":"empty or oversized pattern"}\n')


def cannot(head):
    return (501, "Not Implemented", head + '"error":"the cache tier cannot scan its keys"}\n')


def ok(body):
    return (200, "OK", body + "\n")


def listing(mode, matched, nbytes):
    return ok('{"mode":"%s","matched":%d,"bytes":%d,"listed":0,"next":null,"shards_skipped":0,'
              '"objects":[]}' % (mode, matched, nbytes))


# the same over every tier: refused before the tier is asked
REFUSALS = {
    "tag: no header": NO_TAGS,
    "tag: separators only": NO_TAGS,
    "tag: 65 tags": TOO_MANY,
    "tag: 65 tags soft": TOO_MANY,
    "dry tag: no header": NO_TAGS,
    "dry tag: 65 tags": TOO_MANY,
    "glob: 9 stars": STARS,
    "glob: 9 stars soft": STARS,
    "glob: 9 stars dry": STARS,
    "glob: 1030 literal bytes": LITERAL,
    "inspect: empty prefix": BAD_PATTERN,
    "inspect: empty key": BAD_PATTERN,
    "inspect: no tags": NO_TAGS,
    "inspect: 65 tags": TOO_MANY,
    "inspect: glob stars only": STARS_ONLY,
    "inspect: glob empty": EMPTY_GLOB,
    "inspect: glob dangling": DANGLING,
    "inspect: glob 9 stars": STARS,
    "inspect: glob long": LITERAL,
    "inspect: bad limit": BAD_QUERY,
    "inspect: unknown parameter": BAD_QUERY,
    "inspect: two selectors": BAD_QUERY,
    "inspect: bad escape": BAD_QUERY,
}

# the dry runs answer the same with and without --grace
DRAM_DRY = {
    "dry exact": ok('{"mode":"exact","dry_run":true,"matched":1,"bytes":25,"variants":2}'),
    "dry prefix": ok('{"mode":"prefix","dry_run":true,"matched":3,"bytes":108}'),
    "dry tag": ok('{"mode":"tag","dry_run":true,"tags":1,"matched":4,"bytes":150}'),
    "dry glob": ok('{"mode":"glob","dry_run":true,"matched":3,"bytes":99}'),
    "dry prefix other host": ok('{"mode":"prefix","dry_run":true,"matched":2,"bytes":72}'),
    "dry exact no variants":
        ok('{"mode":"exact","dry_run":true,"matched":1,"bytes":28,"variants":0}'),
    "dry glob, soft ignored": ok('{"mode":"glob","dry_run":true,"matched":1,"bytes":28}'),
    "unknown mode is exact": ok('{"mode":"exact","found":false,"variants":0}'),
    "tag: 64 tags": ok('{"mode":"tag","tags":64,"purged":0}'),
    "glob: backslash is literal": ok('{"mode":"glob","purged":0}'),
    "hard exact again": ok('{"mode":"exact","found":false,"variants":0}'),
    "hard prefix other host": ok('{"mode":"prefix","purged":2}'),
    "inspect key": listing("key", 1, 28),
    "inspect tag": listing("tag", 0, 0),
    "inspect glob": listing("glob", 1, 28),
}

ANSWERS = {
    # DRAM, --grace 60: the soft requests soften, the hard ones then remove what is left
    "dram_grace": {**REFUSALS, **DRAM_DRY, **{
        "soft exact": ok('{"mode":"exact","soft":true,"softened":1,"variants":2}'),
        "soft prefix": ok('{"mode":"prefix","soft":true,"softened":3}'),
        "soft tag": ok('{"mode":"tag","soft":true,"tags":2,"softened":2}'),
        "soft glob": ok('{"mode":"glob","soft":true,"softened":2}'),
        "hard tag": ok('{"mode":"tag","tags":1,"purged":3}'),
        "hard exact": ok('{"mode":"exact","found":true,"variants":1}'),
        "hard prefix": ok('{"mode":"prefix","purged":2}'),
        "hard glob": ok('{"mode":"glob","purged":1}'),
        "inspect all": listing("all", 2, 55),
        "inspect prefix": listing("prefix", 2, 55),
        "inspect cursor": listing("prefix", 2, 55),
    }},
    # DRAM without --grace: a soft request is a hard purge that says "soft":false
    "dram": {**REFUSALS, **DRAM_DRY, **{
        "soft exact": ok('{"mode":"exact","soft":false,"found":true,"variants":2}'),
        "soft prefix": ok('{"mode":"prefix","soft":false,"purged":3}'),
        "soft tag": ok('{"mode":"tag","soft":false,"tags":2,"purged":2}'),
        "soft glob": ok('{"mode":"glob","soft":false,"purged":1}'),
        "hard tag": ok('{"mode":"tag","tags":1,"purged":0}'),
        "hard exact": ok('{"mode":"exact","found":false,"variants":0}'),
        "hard prefix": ok('{"mode":"prefix","purged":0}'),
        "hard glob": ok('{"mode":"glob","purged":0}'),
        "inspect all": listing("all", 1, 28),
        "inspect prefix": listing("prefix", 1, 28),
        "inspect cursor": listing("prefix", 1, 28),
    }},
    # memcached, --grace 60: the tier cannot scan; exact mode still deletes the URL's object
    "memcached_grace": {**REFUSALS, **{
        "dry exact": cannot('{"mode":"exact","dry_run":true,'),
        "dry prefix": cannot('{"mode":"prefix","dry_run":true,'),
        "dry tag": cannot('{"mode":"tag","dry_run":true,"tags":1,'),
        "dry glob": cannot('{"mode":"glob","dry_run":true,'),
        "dry prefix other host": cannot('{"mode":"prefix","dry_run":true,'),
        "soft exact": ok('{"mode":"exact","soft":false,"found":true,"variants":-1}'),
        "soft prefix": cannot('{"mode":"prefix","soft":false,'),
        "soft tag": cannot('{"mode":"tag","soft":false,'),
        "soft glob": cannot('{"mode":"glob","soft":false,'),
        "hard tag": cannot('{"mode":"tag",'),
        "hard exact": ok('{"mode":"exact","found":false,"variants":-1}'),
        "hard exact again": ok('{"mode":"exact","found":false,"variants":-1}'),
        "hard prefix": cannot('{"mode":"prefix",'),
        "hard glob": cannot('{"mode":"glob",'),
        "hard prefix other host": cannot('{"mode":"prefix",'),
        "dry exact no variants": cannot('{"mode":"exact","dry_run":true,'),
        "dry glob, soft ignored": cannot('{"mode":"glob","dry_run":true,'),
        "unknown mode is exact": ok('{"mode":"exact","found":false,"variants":-1}'),
        "tag: 64 tags": cannot('{"mode":"tag",'),
        "glob: backslash is literal": cannot('{"mode":"glob",'),
        "inspect all": cannot('{"mode":"all",'),
        "inspect prefix": cannot('{"mode":"prefix",'),
        "inspect key": cannot('{"mode":"key",'),
        "inspect tag": cannot('{"mode":"tag",'),
        "inspect glob": cannot('{"mode":"glob",'),
        "inspect cursor": cannot('{"mode":"prefix",'),
    }},
}

# A refused tag list or glob is a 400 after purge_requests moved (tag_purge_requests and
# purge_glob_requests move only once the request is accepted); a dry run moves purge_dry_runs
# alone; soft_purge_requests counts soft exact, prefix and glob answers, never tag ones.
STATS = {
    "dram_grace": dict(purge_requests=20, purged_objects=7, purge_denied=0,
                       soft_purge_requests=3, softened_objects=8, tag_purge_requests=3,
                       tag_purged_objects=3, tag_softened_objects=2, purge_glob_requests=3,
                       inspect_requests=19, purge_dry_runs=7),
    "dram": dict(purge_requests=20, purged_objects=9, purge_denied=0, soft_purge_requests=0,
                 softened_objects=0, tag_purge_requests=3, tag_purged_objects=2,
                 tag_softened_objects=0, purge_glob_requests=3, inspect_requests=19,
                 purge_dry_runs=7),
    "memcached_grace": dict(purge_requests=20, purged_objects=1, purge_denied=0,
                            soft_purge_requests=0, softened_objects=0, tag_purge_requests=3,
                            tag_purged_objects=0, tag_softened_objects=0, purge_glob_requests=3,
                            inspect_requests=19, purge_dry_runs=7),
}

# An empty key: the exact form deletes nothing and scans for variants under "\x1f" (one
# object's key starts so); the prefix form is refused by the tier (an empty prefix is a
# flush), which reads as "cannot scan"; a dry run that the tier refuses still counts.
URL_ANSWERS = {
    "empty key: dry exact": cannot('{"mode":"exact","dry_run":true,'),
    "empty key: dry prefix": cannot('{"mode":"prefix","dry_run":true,'),
    "empty key: dry glob": EMPTY_GLOB,
    "empty key: soft exact": ok('{"mode":"exact","soft":false,"found":false,"variants":1}'),
    "empty key: soft prefix": cannot('{"mode":"prefix","soft":false,'),
    "empty key: soft glob": EMPTY_GLOB,
    "empty key: exact": ok('{"mode":"exact","found":false,"variants":0}'),
    "empty key: prefix": cannot('{"mode":"prefix",'),
    "empty key: glob": EMPTY_GLOB,
    "stars only: glob": STARS_ONLY,
    "stars only: dry glob": STARS_ONLY,
    "no tag header: tag": NO_TAG_HEADER,
    "no tag header: soft tag": NO_TAG_HEADER,
    "no tag header: dry tag": NO_TAG_HEADER,
    "no tag header: inspect": NO_TAG_HEADER,
    "prefix still works": ok('{"mode":"prefix","dry_run":true,"matched":2,"bytes":28}'),
}
URL_STATS = dict(purge_requests=9, purged_objects=1, purge_denied=0, soft_purge_requests=0,
                 softened_objects=0, tag_purge_requests=0, tag_purged_objects=0,
                 tag_softened_objects=0, purge_glob_requests=0, inspect_requests=1,
                 purge_dry_runs=3)
