// pybind11 bindings for the shellac_amd native core (_shellac_core).
//
// Device-side entry points take raw device pointers and a hipStream_t as Python
// ints (tensor.data_ptr(), torch.cuda.current_stream().cuda_stream) so the core
// does not link against libtorch; the Python layer (shellac_amd/ops) owns
// allocation through PyTorch's caching allocator.
#include <pybind11/pybind11.h>
#include <pybind11/stl.h>

#include <hip/hip_runtime_api.h>

#include "bind_parts.h"
#include "hbm_cache.h"
#include "host_cache.h"
#include "keyed.h"
#include "trace.h"

namespace py = pybind11;
using namespace shellac;

namespace {

template <typename T>
T* P(uintptr_t p) { return reinterpret_cast<T*>(p); }
hipStream_t S(uintptr_t s) { return reinterpret_cast<hipStream_t>(s); }

py::dict counters_dict(const CacheCounters& c) {
  py::dict d;
  d["get_ops"] = c.get_ops;
  d["get_hits"] = c.get_hits;
  d["get_bytes"] = c.get_bytes;
  d["set_ops"] = c.set_ops;
  d["set_bytes"] = c.set_bytes;
  d["set_dropped"] = c.set_dropped;
  d["set_evicted"] = c.set_evicted;
  d["del_ops"] = c.del_ops;
  d["del_hits"] = c.del_hits;
  d["swept"] = c.swept;
  d["get_coalesced"] = c.get_coalesced;
  d["reinserted"] = c.reinserted;
  d["reinsert_bytes"] = c.reinsert_bytes;
  d["reinsert_lost"] = c.reinsert_lost;
  d["purged"] = c.purged;
  d["touched"] = c.touched;
  return d;
}

}  // namespace

PYBIND11_MODULE(_shellac_core, m) {
  m.doc() = "shellac_amd native core: HBM/DRAM cache shards, HTTP codec, reactor, protocols";

  m.attr("ENTRY_BYTES") = (int)sizeof(Entry);
  m.attr("BUCKET_BYTES") = (int)kBucketBytes;
  m.attr("ITEM_HEADER_BYTES") = (int)kItemHeaderBytes;
  m.attr("SMALL_GET_MAX") = (int64_t)HbmCache::kSmallGetMax;
  m.attr("LOOKUP_PREFIX_WORDS") = (int64_t)HbmCache::kLookupPrefixWords;
  m.attr("SERVE_KEYS") = (int64_t)HbmCache::kServeKeys;
  m.attr("ITEM_MAGIC") = kItemMagic;
  m.attr("MISS_LOC") = py::int_(kMissLoc);
  m.attr("LIST_PREFIX") = (int)kListPrefix;
  m.attr("LIST_TAGS") = (int)kListTags;
  m.attr("LIST_ALL") = (int)kListAll;
  m.attr("LIST_GLOB") = (int)kListGlob;
  m.attr("MAX_GLOB_STARS") = (int)kMaxGlobStars;
  m.attr("MAX_GLOB_LITERAL") = (int)kMaxGlobLiteral;
  m.attr("LIST_ROW_BYTES") = (int)sizeof(ListRow);
  m.attr("MAX_LIST_ROWS") = (int)kMaxListRows;
  m.attr("SLICE_HEAD") = (int)kSliceHead;
  m.attr("SLICE_RANGE") = (int)kSliceRange;
  m.attr("SLICE_FROM") = (int)kSliceFrom;
  m.attr("SLICE_SUFFIX") = (int)kSliceSuffix;
  m.attr("SLICE_WHOLE") = (int)kSliceWhole;
  m.attr("SLICE_MISS") = (int)kSliceMiss;
  m.attr("SLICE_OK") = (int)kSliceOk;
  m.attr("SLICE_UNSAT") = (int)kSliceUnsat;
  m.attr("SLICE_WHOLE_OBJ") = (int)kSliceWholeObj;
  m.attr("SLICE_NOT_MODIFIED") = (int)kSliceNotModified;
  m.attr("SLICE_HEAD_MAX") = (int)kSliceHeadMax;
  m.attr("SLICE_COND_BYTES") = (int)sizeof(SliceCond);
  m.attr("COND_NONE") = (int)kCondNone;
  m.attr("COND_NONE_MATCH") = (int)kCondNoneMatch;
  m.attr("COND_MODIFIED_SINCE") = (int)kCondModifiedSince;
  m.attr("COND_IF_RANGE_ETAG") = (int)kCondIfRangeEtag;
  m.attr("COND_IF_RANGE_DATE") = (int)kCondIfRangeDate;
  m.attr("COND_LINE_MAX") = (int)kCondLineMax;
  m.attr("COND_VALUE_MAX") = (int)kCondValueMax;
  m.attr("COND_MAX_CANDIDATES") = (int)kCondMaxCandidates;
  m.attr("SLICE_ROW_BYTES") = (int)sizeof(SliceRow);
  m.attr("SLICE_SPEC_BYTES") = (int)sizeof(SliceSpec);

  m.def("digest", [](py::bytes b) {
    std::string s = b;
    Digest d = digest_bytes(reinterpret_cast<const uint8_t*>(s.data()), s.size());
    return py::make_tuple(d.lo, d.hi);
  }, "128-bit digest (lo, hi) of a byte string");
  m.def("item_bytes", [](uint32_t vlen) { return item_bytes(vlen); });
  m.def("keyed", [](py::bytes key, py::bytes payload) {
    const std::string k = key, p = payload;
    SH_CHECK(k.size() <= kMaxKeyedKey, "key too long for a keyed value");
    std::string v(keyed_size(k.size(), p.size()), '\0');
    write_keyed(reinterpret_cast<uint8_t*>(&v[0]), k, p.data(), p.size());
    return py::bytes(v);
  }, "the keyed value [u16 key length | key | payload] the backends store");
  m.def("keyed_prefix_image", [](py::bytes prefix) {
    const std::string p = prefix;
    SH_CHECK(p.size() >= 1 && p.size() <= kMaxKeyedKey, "purge prefix must hold 1..65535 bytes");
    std::string img(keyed_prefix_image_bytes(p.size()), '\0');
    write_keyed_prefix_image(reinterpret_cast<uint8_t*>(&img[0]),
                             reinterpret_cast<const uint8_t*>(p.data()), p.size());
    return py::bytes(img);
  }, "pattern image of a purge prefix for HbmCache.remove_keyed_prefix");
  m.def("keyed_glob_image", [](py::bytes pattern) {
    const std::string p = pattern;
    KeyedGlob g;
    std::string why;
    if (!compile_keyed_glob(p, &g, &why)) throw py::value_error(why);
    return py::bytes(reinterpret_cast<const char*>(&g), keyed_glob_used_bytes(g));
  }, "compiled glob pattern ('*' wildcards, '\\' escapes) for HbmCache.remove_keyed_glob; "
     "ValueError on a refused pattern");
  m.def("glob_match", [](py::bytes pattern, py::bytes key) {
    const std::string p = pattern, k = key;
    KeyedGlob g;
    std::string why;
    if (!compile_keyed_glob(p, &g, &why)) throw py::value_error(why);
    return keyed_glob_matches(g, reinterpret_cast<const uint8_t*>(k.data()), k.size());
  }, "the host glob matcher on a stored key (its subject ends at the first 0x1f)");
  m.def("tag_hash", [](py::bytes tag) {
    const std::string t = tag;
    return tag_hash(t);
  }, "hash of one surrogate key (tag): the low word of its digest");
  m.def("tag_block", [](const std::vector<uint64_t>& hashes) {
    std::string b(tag_block_size(hashes.size()), '\0');
    write_tag_block(reinterpret_cast<uint8_t*>(&b[0]), hashes.data(), hashes.size());
    return py::bytes(b);
  }, "the tag block [0x02 | ntags | hashes] for distinct hashes (more than 32: overflow)");
  m.def("parse_tag_block", [](py::bytes payload) {
    const std::string p = payload;
    const uint64_t* hs;
    unsigned nt;
    bool over;
    const size_t strip = parse_tag_block(p.data(), p.size(), &hs, &nt, &over);
    std::vector<uint64_t> out;
    for (unsigned i = 0; i < nt; ++i) out.push_back(tag_block_hash(hs, i));
    return py::make_tuple(strip, out, over);
  }, "(bytes to strip, hashes, overflow) of the tag block at the start of a payload");
  m.def("resolve_window", [](uint32_t kind, uint64_t a, uint64_t b, uint64_t body_len) {
    uint64_t first = 0, len = 0;
    const bool ok = resolve_window(kind, a, b, body_len, &first, &len);
    return py::make_tuple(ok, first, len);
  }, "(satisfiable, first, length) of a window spec over a body of body_len bytes (slice.h)");
  m.def("slice_layout", [](py::bytes value) -> py::object {
    const std::string v = value;
    uint32_t ho = 0, bo = 0;
    if (!slice_layout(reinterpret_cast<const uint8_t*>(v.data()), v.size(), &ho, &bo))
      return py::none();
    return py::make_tuple(ho, bo);
  }, "(head_off, body_off) of a sliceable keyed value, else None (slice.h)");
  m.def("cond_matches", [](py::bytes value, uint32_t kind, uint32_t ncand, py::bytes records) {
    const std::string v = value, r = records;
    uint32_t ho = 0, bo = 0;
    if (!slice_layout(reinterpret_cast<const uint8_t*>(v.data()), v.size(), &ho, &bo)) return false;
    const SliceCond c{kind, ncand, 0, (uint32_t)r.size()};
    return cond_matches(reinterpret_cast<const uint8_t*>(v.data()), ho, bo, c,
                        reinterpret_cast<const uint8_t*>(r.data()));
  }, "whether a condition (kind, ncand, candidate records) holds for a keyed value (conditional.h)");
  const auto cond_tuple = [](bool ok, const CondRequest& c) -> py::object {
    if (!ok) return py::none();
    return py::make_tuple(c.kind, c.ncand, py::bytes(c.records));
  };
  m.def("parse_if_none_match", [cond_tuple](py::bytes value) {
    const std::string v = value;
    CondRequest c;
    return cond_tuple(parse_if_none_match(v.data(), v.size(), &c), c);
  }, "(kind, ncand, records) of an If-None-Match value, None: the header is ignored");
  m.def("parse_if_range", [cond_tuple](py::bytes value) {
    const std::string v = value;
    CondRequest c;
    return cond_tuple(parse_if_range(v.data(), v.size(), &c), c);
  }, "(kind, 1, record) of an If-Range value, None: it can never match (ask for the whole object)");
  m.def("parse_if_modified_since", [cond_tuple](py::bytes value) {
    const std::string v = value;
    CondRequest c;
    return cond_tuple(parse_if_modified_since(v.data(), v.size(), &c), c);
  }, "(kind, 1, record) of an If-Modified-Since value, None: the header is ignored");
  m.def("bucket_pair", [](uint64_t lo, uint64_t hi, uint64_t nbuckets) {
    const Digest d{lo, hi};
    return std::vector<uint64_t>{bucket1(d, nbuckets - 1), bucket2(d, nbuckets - 1)};
  });

  // ---------------- device (HIP) ----------------
  py::class_<HbmCache::StoreGraph>(m, "StoreGraph")
      .def(py::init<>())
      .def_readonly("captures", &HbmCache::StoreGraph::captures)
      .def_readonly("launches", &HbmCache::StoreGraph::launches)
      .def("destroy", [](HbmCache::StoreGraph& g) { HbmCache::destroy_graph(&g); });

  py::class_<HbmCache>(m, "HbmCache")
      .def(py::init([](uint64_t log_bytes, uint64_t nbuckets, uint32_t max_item, int device,
                       int evict, uint64_t reinsert_max, int serve_blocks) {
             ShardConfig c;
             c.log_bytes = log_bytes;
             c.nbuckets = nbuckets;
             c.max_item = max_item;
             c.device = device;
             c.evict = evict;
             c.reinsert_max = reinsert_max;
             c.serve_blocks = serve_blocks;
             return new HbmCache(c);
           }),
           py::arg("log_bytes"), py::arg("nbuckets"), py::arg("max_item"), py::arg("device"),
           py::arg("evict") = (int)kEvictClock, py::arg("reinsert_max") = 0,
           py::arg("serve_blocks") = 8)
      .def_property_readonly("serve_blocks", &HbmCache::serve_blocks)
      .def_property_readonly("reinsert_max", &HbmCache::reinsert_max)
      .def("lookup", [](HbmCache& c, uintptr_t keys, int64_t n, uintptr_t loc, uintptr_t size,
                        uintptr_t off, uint32_t now, uintptr_t s, uint64_t reserve, int slot,
                        uintptr_t first) {
        py::gil_scoped_release nogil;
        c.lookup(P<const Digest>(keys), n, P<uint64_t>(loc), P<uint64_t>(size), P<uint64_t>(off),
                 now, S(s), reserve, slot, P<const uint32_t>(first));
      }, py::arg("keys"), py::arg("n"), py::arg("loc"), py::arg("size"), py::arg("off"),
         py::arg("now"), py::arg("stream"), py::arg("reserve") = 0, py::arg("total_slot") = -1,
         py::arg("first") = 0)
      .def("lookup_coalesced", [](HbmCache& c, uintptr_t keys, int64_t n, uintptr_t table,
                                  int64_t slots, uintptr_t first, uintptr_t loc, uintptr_t size,
                                  uintptr_t off, uint32_t now, uintptr_t s, uint64_t reserve,
                                  int slot, uintptr_t cslot, bool table_clean, uintptr_t prefix,
                                  uintptr_t index_done) {
        py::gil_scoped_release nogil;
        return c.lookup_coalesced(P<const Digest>(keys), n, P<uint32_t>(table), slots,
                                  P<uint32_t>(first), P<uint64_t>(loc), P<uint64_t>(size),
                                  P<uint64_t>(off), now, S(s), reserve, slot, P<uint32_t>(cslot),
                                  table_clean, P<uint64_t>(prefix),
                                  reinterpret_cast<hipEvent_t>(index_done));
      }, py::arg("keys"), py::arg("n"), py::arg("table"), py::arg("slots"), py::arg("first"),
         py::arg("loc"), py::arg("size"), py::arg("off"), py::arg("now"), py::arg("stream"),
         py::arg("reserve") = 0, py::arg("total_slot") = -1, py::arg("cslot") = 0,
         py::arg("table_clean") = false, py::arg("prefix") = 0, py::arg("index_done") = 0)
      .def("small_get", [](HbmCache& c, uintptr_t keys, int64_t n, uintptr_t out,
                           uint64_t out_cap, uintptr_t off, uint32_t now, uintptr_t s,
                           int done_slot) {
        py::gil_scoped_release nogil;
        c.small_get(P<const Digest>(keys), n, P<uint8_t>(out), out_cap, P<uint64_t>(off), now,
                    S(s), done_slot);
      }, py::arg("keys"), py::arg("n"), py::arg("out"), py::arg("out_cap"), py::arg("off"),
         py::arg("now"), py::arg("stream"), py::arg("done_slot") = -1)
      // ordered after `stream` only (the caller's current stream; 0 = the null stream): the
      // resident server runs on no stream, so what the caller queued there to fill `out` /
      // `off` (or SETs queued on that stream) lands before the job is queued; SETs a
      // ShardedCache queued on its own streams need its sync_sets() first
      .def("serve_get", [](HbmCache& c, uintptr_t host_keys, int64_t n, uintptr_t out,
                           uint64_t out_cap, uintptr_t off, uint32_t now, int done_slot,
                           uintptr_t stream) {
        py::gil_scoped_release nogil;
        return c.serve_get_after(S(stream), P<const Digest>(host_keys), n, P<uint8_t>(out),
                                 out_cap, P<uint64_t>(off), now, done_slot);
      }, py::arg("host_keys"), py::arg("n"), py::arg("out"), py::arg("out_cap"), py::arg("off"),
         py::arg("now"), py::arg("done_slot"), py::arg("stream") = 0)
      .def("serve_wait", [](HbmCache& c, int slot, int64_t timeout_ms) {
        py::gil_scoped_release nogil;
        return c.serve_wait(slot, timeout_ms);
      }, py::arg("slot"), py::arg("timeout_ms") = 10000)
      .def("serve_kick", [](HbmCache& c) {
        py::gil_scoped_release nogil;
        c.serve_kick();
      })
      .def("serve_stop", [](HbmCache& c) {
        py::gil_scoped_release nogil;
        c.serve_stop();
      })
      .def("serve_trace", &HbmCache::serve_trace)
      .def_property_readonly("wall_khz", &HbmCache::wall_khz)
      .def_property_readonly("serve_launches", &HbmCache::serve_launches)
      .def_property_readonly("serve_jobs", &HbmCache::serve_jobs)
      .def("host_slot", &HbmCache::host_slot)
      .def("wait_host_slot", [](const HbmCache& c, int i, int64_t timeout_ms) {
        py::gil_scoped_release nogil;
        return c.wait_host_slot(i, timeout_ms);
      }, py::arg("slot"), py::arg("timeout_ms") = 10000)
      .def("gather", [](HbmCache& c, uintptr_t loc, uintptr_t off, int64_t n, uintptr_t out,
                        uintptr_t s, uint64_t out_cap, uintptr_t first, uintptr_t size,
                        uintptr_t out_size, uintptr_t out_off, uintptr_t table, uintptr_t cslot,
                        uintptr_t prefix, int shift, int64_t table_slots) {
        py::gil_scoped_release nogil;
        c.gather(P<const uint64_t>(loc), P<const uint64_t>(off), n, P<uint8_t>(out), S(s),
                 out_cap, P<const uint32_t>(first), P<const uint64_t>(size), P<uint64_t>(out_size),
                 P<uint64_t>(out_off), P<uint32_t>(table), P<const uint32_t>(cslot),
                 P<const uint64_t>(prefix), shift, table_slots);
      }, py::arg("loc"), py::arg("off"), py::arg("n"), py::arg("out"), py::arg("stream"),
         py::arg("out_cap") = ~0ull, py::arg("first") = 0, py::arg("size") = 0,
         py::arg("out_size") = 0, py::arg("out_off") = 0, py::arg("table") = 0,
         py::arg("cslot") = 0, py::arg("prefix") = 0, py::arg("shift") = 0,
         py::arg("table_slots") = 0)
      .def("store_graph", [](HbmCache& c, HbmCache::StoreGraph& g, uintptr_t keys,
                             uintptr_t values, uintptr_t val_off, uintptr_t vlen, uintptr_t flags,
                             uintptr_t expire, int64_t n, uint64_t bytes_bound, uint32_t now,
                             uintptr_t s) {
        py::gil_scoped_release nogil;
        c.store_graph(&g, P<const Digest>(keys), P<const uint8_t>(values),
                      P<const uint64_t>(val_off), P<const uint32_t>(vlen),
                      P<const uint32_t>(flags), P<const uint32_t>(expire), n, bytes_bound, now,
                      S(s));
      })
      .def("store", [](HbmCache& c, uintptr_t keys, uintptr_t values, uintptr_t val_off,
                       uintptr_t vlen, uintptr_t flags, uintptr_t expire, int64_t n,
                       uint64_t bytes_bound, uint32_t now, uintptr_t s, uintptr_t index_after,
                       uintptr_t append_after, uintptr_t append_done, int phase,
                       uintptr_t plan_done, uintptr_t done) {
        py::gil_scoped_release nogil;
        StoreOpts o;
        o.index_after = reinterpret_cast<hipEvent_t>(index_after);
        o.append_after = reinterpret_cast<hipEvent_t>(append_after);
        o.append_done = reinterpret_cast<hipEvent_t>(append_done);
        o.plan_done = reinterpret_cast<hipEvent_t>(plan_done);
        o.done = reinterpret_cast<hipEvent_t>(done);
        o.phase = phase;
        c.store(P<const Digest>(keys), P<const uint8_t>(values), P<const uint64_t>(val_off),
                P<const uint32_t>(vlen), P<const uint32_t>(flags), P<const uint32_t>(expire), n,
                bytes_bound, now, S(s), o);
      }, py::arg("keys"), py::arg("values"), py::arg("val_off"), py::arg("vlen"),
         py::arg("flags"), py::arg("expire"), py::arg("n"), py::arg("bytes_bound"), py::arg("now"),
         py::arg("stream"), py::arg("index_after") = 0, py::arg("append_after") = 0,
         py::arg("append_done") = 0, py::arg("phase") = 0, py::arg("plan_done") = 0,
         py::arg("done") = 0)
      .def("remove", [](HbmCache& c, uintptr_t keys, int64_t n, uintptr_t found, uint32_t now,
                        uintptr_t s) {
        py::gil_scoped_release nogil;
        c.remove(P<const Digest>(keys), n, P<uint8_t>(found), now, S(s));
      })
      // image: keyed_prefix_image(prefix) in device-readable memory; out: 2 words (device
      // or mapped pinned memory); asynchronous on the stream
      .def("remove_keyed_prefix", [](HbmCache& c, uintptr_t image, uint32_t plen, uint32_t now,
                                     uintptr_t out, uintptr_t s) {
        py::gil_scoped_release nogil;
        c.remove_keyed_prefix(P<const uint8_t>(image), plen, now, P<uint64_t>(out), S(s));
      }, py::arg("image"), py::arg("plen"), py::arg("now"), py::arg("out"), py::arg("stream"))
      // image as above; out: 1 word; asynchronous on the stream
      .def("soften_keyed_prefix", [](HbmCache& c, uintptr_t image, uint32_t plen, bool exact,
                                     uint32_t stale_at, uint32_t expire_cap, uint32_t now,
                                     uintptr_t out, uintptr_t s) {
        py::gil_scoped_release nogil;
        c.soften_keyed_prefix(P<const uint8_t>(image), plen, exact, stale_at, expire_cap, now,
                              P<uint64_t>(out), S(s));
      }, py::arg("image"), py::arg("plen"), py::arg("exact"), py::arg("stale_at"),
         py::arg("expire_cap"), py::arg("now"), py::arg("out"), py::arg("stream"))
      // tags: ntags u64 hashes (device or mapped host memory); out: 2 words; asynchronous
      .def("remove_keyed_tags", [](HbmCache& c, uintptr_t tags, uint32_t ntags, uint32_t now,
                                   uintptr_t out, uintptr_t s) {
        py::gil_scoped_release nogil;
        c.remove_keyed_tags(P<const uint64_t>(tags), ntags, now, P<uint64_t>(out), S(s));
      }, py::arg("tags"), py::arg("ntags"), py::arg("now"), py::arg("out"), py::arg("stream"))
      // out: 1 word; asynchronous on the stream
      .def("soften_keyed_tags", [](HbmCache& c, uintptr_t tags, uint32_t ntags, uint32_t stale_at,
                                   uint32_t expire_cap, uint32_t now, uintptr_t out, uintptr_t s) {
        py::gil_scoped_release nogil;
        c.soften_keyed_tags(P<const uint64_t>(tags), ntags, stale_at, expire_cap, now,
                            P<uint64_t>(out), S(s));
      }, py::arg("tags"), py::arg("ntags"), py::arg("stale_at"), py::arg("expire_cap"),
         py::arg("now"), py::arg("out"), py::arg("stream"))
      // image: keyed_glob_image(pattern) in device-readable memory, image_bytes its length;
      // out: 2 words; asynchronous on the stream
      .def("remove_keyed_glob", [](HbmCache& c, uintptr_t image, uint32_t image_bytes,
                                   uint32_t now, uintptr_t out, uintptr_t s) {
        py::gil_scoped_release nogil;
        c.remove_keyed_glob(P<const uint8_t>(image), image_bytes, now, P<uint64_t>(out), S(s));
      }, py::arg("image"), py::arg("image_bytes"), py::arg("now"), py::arg("out"),
         py::arg("stream"))
      // out: 1 word; asynchronous on the stream
      .def("soften_keyed_glob", [](HbmCache& c, uintptr_t image, uint32_t image_bytes,
                                   uint32_t stale_at, uint32_t expire_cap, uint32_t now,
                                   uintptr_t out, uintptr_t s) {
        py::gil_scoped_release nogil;
        c.soften_keyed_glob(P<const uint8_t>(image), image_bytes, stale_at, expire_cap, now,
                            P<uint64_t>(out), S(s));
      }, py::arg("image"), py::arg("image_bytes"), py::arg("stale_at"), py::arg("expire_cap"),
         py::arg("now"), py::arg("out"), py::arg("stream"))
      // mode: LIST_PREFIX (image, plen, exact), LIST_TAGS (tags, ntags), LIST_GLOB (image:
      // keyed_glob_image's, plen: its length) or LIST_ALL; rows:
      // limit x LIST_ROW_BYTES, keys: limit x key_cap, out: 4 words {matched, bytes, listed,
      // next} (device or mapped pinned memory); asynchronous on the stream
      .def("list_keyed", [](HbmCache& c, uint32_t mode, uintptr_t image, uint32_t plen, bool exact,
                            uintptr_t tags, uint32_t ntags, uint64_t start, uint32_t limit,
                            uint32_t key_cap, uint32_t now, uintptr_t rows, uintptr_t keys,
                            uintptr_t out, uintptr_t s) {
        py::gil_scoped_release nogil;
        c.list_keyed(mode, P<const uint8_t>(image), plen, exact, P<const uint64_t>(tags), ntags,
                     start, limit, key_cap, now, P<ListRow>(rows), P<uint8_t>(keys),
                     P<uint64_t>(out), S(s));
      }, py::arg("mode"), py::arg("image"), py::arg("plen"), py::arg("exact"), py::arg("tags"),
         py::arg("ntags"), py::arg("start"), py::arg("limit"), py::arg("key_cap"), py::arg("now"),
         py::arg("rows"), py::arg("keys"), py::arg("out"), py::arg("stream"))
      // spec: n x SLICE_SPEC_BYTES, rows: n x SLICE_ROW_BYTES, res: 2 words {hits, bytes}
      // (device or mapped pinned memory); asynchronous on the stream
      .def("get_keyed_slices", [](HbmCache& c, uintptr_t keys, uintptr_t key_bytes,
                                  uintptr_t key_offs, uintptr_t spec, int64_t n, uintptr_t rows,
                                  uintptr_t out, uint64_t out_cap, uintptr_t res, uint32_t now,
                                  uintptr_t s, uint64_t reserve, uintptr_t cond,
                                  uintptr_t cond_bytes) {
        py::gil_scoped_release nogil;
        c.get_keyed_slices(P<const Digest>(keys), P<const uint8_t>(key_bytes),
                           P<const int64_t>(key_offs), P<const SliceSpec>(spec), n,
                           P<SliceRow>(rows), P<uint8_t>(out), out_cap, P<uint64_t>(res), now, S(s),
                           reserve, P<const SliceCond>(cond), P<const uint8_t>(cond_bytes));
      }, py::arg("keys"), py::arg("key_bytes"), py::arg("key_offs"), py::arg("spec"), py::arg("n"),
         py::arg("rows"), py::arg("out"), py::arg("out_cap"), py::arg("res"), py::arg("now"),
         py::arg("stream"), py::arg("reserve") = 0, py::arg("cond") = 0,
         py::arg("cond_bytes") = 0)
      // flags / key_bytes + key_offs: 0 = none; asynchronous on the stream
      .def("touch", [](HbmCache& c, uintptr_t keys, uintptr_t expire, uintptr_t flags,
                       uintptr_t key_bytes, uintptr_t key_offs, int64_t n, uintptr_t hit,
                       uint32_t now, uintptr_t s) {
        py::gil_scoped_release nogil;
        c.touch(P<const Digest>(keys), P<const uint32_t>(expire), P<const uint32_t>(flags),
                P<const uint8_t>(key_bytes), P<const int64_t>(key_offs), n, P<uint8_t>(hit), now,
                S(s));
      }, py::arg("keys"), py::arg("expire"), py::arg("flags"), py::arg("key_bytes"),
         py::arg("key_offs"), py::arg("n"), py::arg("hit"), py::arg("now"), py::arg("stream"))
      .def("sweep", [](HbmCache& c, uint32_t now, uintptr_t s) {
        uint64_t live = 0, bytes = 0;
        {
          py::gil_scoped_release nogil;
          c.sweep(now, S(s), &live, &bytes);
        }
        return py::make_tuple(live, bytes);
      })
      .def("flush", [](HbmCache& c, uintptr_t s) { c.flush(S(s)); })
      .def("debug_bucket", &HbmCache::debug_bucket)
      .def("debug_hand", &HbmCache::debug_hand)
      .def("debug_set_entry", &HbmCache::debug_set_entry)
      .def("debug_set_hand", &HbmCache::debug_set_hand, py::arg("hand"), py::arg("catch_up") = true)
      .def("retired_bytes", &HbmCache::retired_bytes, py::call_guard<py::gil_scoped_release>())
      .def_property_readonly("retired_ever", &HbmCache::retired_ever)
      .def("export_keys", [](HbmCache& c, uintptr_t out, uint64_t cap, uint32_t now, uintptr_t s) {
        py::gil_scoped_release nogil;
        return c.export_keys(P<Digest>(out), cap, now, S(s));
      })
      .def("save", [](HbmCache& c, const std::string& path, std::vector<uint64_t> user, uintptr_t s) {
        user.resize(4);
        py::gil_scoped_release nogil;
        c.save(path, user.data(), S(s));
      })
      .def("load", [](HbmCache& c, const std::string& path, uintptr_t s) {
        std::vector<uint64_t> user(4);
        {
          py::gil_scoped_release nogil;
          c.load(path, user.data(), S(s));
        }
        return user;
      })
      .def("counters", [](HbmCache& c, uintptr_t s) { return counters_dict(c.counters(S(s))); })
      .def("head", [](HbmCache& c, uintptr_t s) { return c.head(S(s)); })
      .def("reserve", &HbmCache::reserve)
      .def("hbm_bytes", &HbmCache::hbm_bytes)
      .def_property_readonly("log_ptr", [](HbmCache& c) { return (uintptr_t)c.log_ptr(); })
      .def_property_readonly("index_ptr", [](HbmCache& c) { return (uintptr_t)c.index_ptr(); })
      .def_property_readonly("head_ptr", [](HbmCache& c) { return (uintptr_t)c.head_ptr(); });

  m.def("scan_tmp_bytes", &device_scan_tmp_bytes);
  m.def("exclusive_scan", [](uintptr_t in, uintptr_t out, int64_t n, uintptr_t tmp,
                             size_t tmp_bytes, uintptr_t s) {
    device_exclusive_scan(P<const uint64_t>(in), P<uint64_t>(out), n, P<void>(tmp), tmp_bytes,
                          S(s));
  });
  m.def("trace_enable", [](bool on) { trace_enable(on); });
  m.def("trace_on", []() { return trace_on(); });
  m.def("trace_push", [](const std::string& name) { trace_push(name.c_str()); });
  m.def("trace_pop", []() { trace_pop(); });
  m.def("trace_mark", [](const std::string& name) { trace_mark(name.c_str()); });
  m.def("segcopy", [](uintptr_t src, uintptr_t src_off, uintptr_t dst_off, int64_t n,
                      uintptr_t dst, uintptr_t s, uint64_t dst_cap) {
    segcopy(P<const uint8_t>(src), P<const uint64_t>(src_off), P<const uint64_t>(dst_off), n,
            P<uint8_t>(dst), S(s), dst_cap);
  }, py::arg("src"), py::arg("src_off"), py::arg("dst_off"), py::arg("n"), py::arg("dst"),
     py::arg("stream"), py::arg("dst_cap") = ~0ull);
  m.def("segcopy_sized", [](uintptr_t src, uintptr_t src_off, uintptr_t dst_off,
                            uintptr_t seg_len, int64_t n, uintptr_t dst, uintptr_t s,
                            uint64_t cap) {
    segcopy_sized(P<const uint8_t>(src), P<const uint64_t>(src_off), P<const uint64_t>(dst_off),
                  P<const uint64_t>(seg_len), n, P<uint8_t>(dst), S(s), cap);
  }, py::arg("src"), py::arg("src_off"), py::arg("dst_off"), py::arg("seg_len"), py::arg("n"),
     py::arg("dst"), py::arg("stream"), py::arg("cap") = ~0ull);
  m.def("segcopy_dev", [](uintptr_t src_off, uintptr_t dst_off, uintptr_t n_dev, uintptr_t dst,
                          uintptr_t s, uint64_t dst_cap) {
    segcopy_dev(P<const uint64_t>(src_off), P<const uint64_t>(dst_off), P<const int64_t>(n_dev),
                P<uint8_t>(dst), S(s), dst_cap);
  }, py::arg("src_off"), py::arg("dst_off"), py::arg("n_dev"), py::arg("dst"),
     py::arg("stream"), py::arg("dst_cap") = ~0ull);
  m.def("segcopy_geometry", []() {
    const SegcopyGeometry g = segcopy_geometry();
    py::dict grid;
    for (int mode = 0; mode < 5; ++mode) grid[py::int_(mode)] = g.grid[mode];
    py::dict d;
    d["min_tile"] = g.min_tile;
    d["stage"] = g.stage;
    d["stage_sized"] = g.stage_sized;
    d["stage_glds"] = g.stage_glds;
    d["glds"] = g.glds;
    d["grid"] = grid;
    return d;
  });
  m.def("coalesce_table_slots", &coalesce_table_slots);
  m.def("coalesce_keys", [](uintptr_t keys, int64_t n, uintptr_t table, int64_t slots,
                            uintptr_t first, uintptr_t s, uintptr_t cslot, bool table_clean) {
    coalesce_keys(P<const Digest>(keys), n, P<uint32_t>(table), slots, P<uint32_t>(first), S(s),
                  P<uint32_t>(cslot), table_clean);
  }, py::arg("keys"), py::arg("n"), py::arg("table"), py::arg("slots"), py::arg("first"),
     py::arg("stream"), py::arg("cslot") = 0, py::arg("table_clean") = false);
  m.def("expand_coalesced", [](uintptr_t first, int64_t n, uintptr_t size, uintptr_t off,
                               uintptr_t s) {
    expand_coalesced(P<const uint32_t>(first), n, P<uint64_t>(size), P<uint64_t>(off), S(s));
  });
  m.def("expand_coalesced_out", [](uintptr_t first, int64_t n, uintptr_t size, uintptr_t off,
                                   uintptr_t out_size, uintptr_t out_off, uintptr_t table,
                                   uintptr_t cslot, uintptr_t s) {
    expand_coalesced_out(P<const uint32_t>(first), n, P<const uint64_t>(size),
                         P<const uint64_t>(off), P<uint64_t>(out_size), P<uint64_t>(out_off),
                         P<uint32_t>(table), P<const uint32_t>(cslot), S(s));
  });
  m.def("digest_keys", [](uintptr_t bytes, uintptr_t offs, int64_t n, uintptr_t out,
                          uintptr_t s) {
    digest_keys(P<const uint8_t>(bytes), P<const int64_t>(offs), n, P<Digest>(out), S(s));
  });
  m.def("route_keys", [](uintptr_t keys, int64_t n, uintptr_t pts, uintptr_t owner, int32_t npts,
                         uintptr_t dest, uintptr_t counts, int32_t nranks, uintptr_t s) {
    route_keys(P<const Digest>(keys), n, P<const uint32_t>(pts), P<const int32_t>(owner), npts,
               P<int32_t>(dest), P<int64_t>(counts), nranks, S(s));
  });
  m.def("scatter_by_dest", [](uintptr_t dest, uintptr_t base, int64_t n, int32_t nranks,
                              uintptr_t cursor, uintptr_t perm, uintptr_t s) {
    scatter_by_dest(P<const int32_t>(dest), P<const int64_t>(base), n, nranks, P<int64_t>(cursor),
                    P<int64_t>(perm), S(s));
  });
  m.def("permute_records", [](uintptr_t in, uintptr_t perm, int64_t n, int32_t rec_bytes,
                              uintptr_t out, uintptr_t s) {
    permute_records(P<const void>(in), P<const int64_t>(perm), n, rec_bytes, P<void>(out), S(s));
  });
  m.def("mfma_hello", [](uintptr_t a, uintptr_t b, uintptr_t c, int tiles, uintptr_t s) {
    mfma_hello(P<const uint16_t>(a), P<const uint16_t>(b), P<float>(c), tiles, S(s));
  });
  // Cross-stream ordering with events whose fence scope the caller picks (torch's events
  // use the default: a system-scope release/acquire, i.e. an L2 write-back and invalidate at
  // every record). Two streams of one GPU only need device scope.
  m.attr("EVENT_DISABLE_TIMING") = (unsigned)hipEventDisableTiming;
  m.attr("EVENT_DISABLE_SYSTEM_FENCE") = (unsigned)hipEventDisableSystemFence;
  m.attr("EVENT_RELEASE_TO_DEVICE") = (unsigned)hipEventReleaseToDevice;
  m.def("event_create", [](unsigned flags) {
    hipEvent_t e = nullptr;
    SH_CHECK(hipEventCreateWithFlags(&e, flags) == hipSuccess, "hipEventCreateWithFlags failed");
    return reinterpret_cast<uintptr_t>(e);
  });
  m.def("event_destroy", [](uintptr_t e) { (void)hipEventDestroy(reinterpret_cast<hipEvent_t>(e)); });
  m.def("event_elapsed_ms", [](uintptr_t a, uintptr_t b) {
    float ms = 0.f;
    SH_CHECK(hipEventSynchronize(reinterpret_cast<hipEvent_t>(b)) == hipSuccess &&
                 hipEventElapsedTime(&ms, reinterpret_cast<hipEvent_t>(a),
                                     reinterpret_cast<hipEvent_t>(b)) == hipSuccess,
             "hipEventElapsedTime failed");
    return ms;
  });
  m.def("event_query", [](uintptr_t e) {  // true: the work the event marks is complete
    return hipEventQuery(reinterpret_cast<hipEvent_t>(e)) == hipSuccess;
  });
  m.def("event_record", [](uintptr_t e, uintptr_t s) {
    SH_CHECK(hipEventRecord(reinterpret_cast<hipEvent_t>(e), S(s)) == hipSuccess,
             "hipEventRecord failed");
  });
  m.def("stream_wait_event", [](uintptr_t s, uintptr_t e) {
    SH_CHECK(hipStreamWaitEvent(S(s), reinterpret_cast<hipEvent_t>(e), 0) == hipSuccess,
             "hipStreamWaitEvent failed");
  });
  // raw streams a caller owns (tests: a stream destroyed while a cache still remembers it)
  m.def("stream_create", []() {
    hipStream_t st = nullptr;
    SH_CHECK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking) == hipSuccess,
             "hipStreamCreateWithFlags failed");
    return reinterpret_cast<uintptr_t>(st);
  });
  m.def("stream_destroy", [](uintptr_t s) {
    SH_CHECK(hipStreamSynchronize(S(s)) == hipSuccess && hipStreamDestroy(S(s)) == hipSuccess,
             "hipStreamDestroy failed");
  });
  m.def("device_count", []() {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
  });

  // ---------------- host (DRAM) ----------------
  py::class_<HostCache>(m, "HostCache")
      .def(py::init<uint64_t, uint64_t, uint32_t, int, uint64_t>(), py::arg("log_bytes"),
           py::arg("nbuckets"), py::arg("max_item"), py::arg("evict") = 1,
           py::arg("reinsert_max") = 0)
      .def_property_readonly("reinsert_max", &HostCache::reinsert_max)
      .def("lookup", [](HostCache& c, uintptr_t keys, int64_t n, uintptr_t loc, uintptr_t size,
                        uintptr_t off, uint32_t now, uint64_t reserve) {
        py::gil_scoped_release nogil;
        c.lookup(P<const Digest>(keys), n, P<uint64_t>(loc), P<uint64_t>(size), P<uint64_t>(off),
                 now, reserve);
      }, py::arg("keys"), py::arg("n"), py::arg("loc"), py::arg("size"), py::arg("off"),
         py::arg("now"), py::arg("reserve") = 0)
      .def("gather", [](HostCache& c, uintptr_t loc, uintptr_t off, int64_t n, uintptr_t out) {
        py::gil_scoped_release nogil;
        c.gather(P<const uint64_t>(loc), P<const uint64_t>(off), n, P<uint8_t>(out));
      })
      .def("store", [](HostCache& c, uintptr_t keys, uintptr_t values, uintptr_t val_off,
                       uintptr_t vlen, uintptr_t flags, uintptr_t expire, int64_t n,
                       uint32_t now, uint64_t bytes_bound) {
        py::gil_scoped_release nogil;
        c.store(P<const Digest>(keys), P<const uint8_t>(values), P<const uint64_t>(val_off),
                P<const uint32_t>(vlen), P<const uint32_t>(flags), P<const uint32_t>(expire), n,
                now, bytes_bound);
      }, py::arg("keys"), py::arg("values"), py::arg("val_off"), py::arg("vlen"), py::arg("flags"),
         py::arg("expire"), py::arg("n"), py::arg("now"), py::arg("bytes_bound") = 0)
      .def("remove", [](HostCache& c, uintptr_t keys, int64_t n, uintptr_t found, uint32_t now) {
        py::gil_scoped_release nogil;
        c.remove(P<const Digest>(keys), n, P<uint8_t>(found), now);
      })
      .def("remove_keyed_prefix", [](HostCache& c, py::bytes prefix, uint32_t now) {
        const std::string p = prefix;
        uint64_t out[2] = {0, 0};
        c.remove_keyed_prefix(reinterpret_cast<const uint8_t*>(p.data()), (uint32_t)p.size(), now,
                              out);
        return py::make_tuple(out[0], out[1]);
      }, py::arg("prefix"), py::arg("now"))
      .def("soften_keyed_prefix", [](HostCache& c, py::bytes prefix, bool exact, uint32_t stale_at,
                                     uint32_t expire_cap, uint32_t now) {
        const std::string p = prefix;
        return c.soften_keyed_prefix(reinterpret_cast<const uint8_t*>(p.data()),
                                     (uint32_t)p.size(), exact, stale_at, expire_cap, now);
      }, py::arg("prefix"), py::arg("exact"), py::arg("stale_at"), py::arg("expire_cap"),
         py::arg("now"))
      .def("remove_keyed_tags", [](HostCache& c, std::vector<uint64_t> tags, uint32_t now) {
        uint64_t out[2] = {0, 0};
        c.remove_keyed_tags(tags.data(), (uint32_t)tags.size(), now, out);
        return py::make_tuple(out[0], out[1]);
      }, py::arg("tags"), py::arg("now"))
      .def("soften_keyed_tags", [](HostCache& c, std::vector<uint64_t> tags, uint32_t stale_at,
                                   uint32_t expire_cap, uint32_t now) {
        return c.soften_keyed_tags(tags.data(), (uint32_t)tags.size(), stale_at, expire_cap, now);
      }, py::arg("tags"), py::arg("stale_at"), py::arg("expire_cap"), py::arg("now"))
      .def("remove_keyed_glob", [](HostCache& c, py::bytes pattern, uint32_t now) {
        const std::string p = pattern;
        KeyedGlob g;
        std::string why;
        if (!compile_keyed_glob(p, &g, &why)) throw py::value_error(why);
        uint64_t out[2] = {0, 0};
        c.remove_keyed_glob(g, now, out);
        return py::make_tuple(out[0], out[1]);
      }, py::arg("pattern"), py::arg("now"))
      .def("soften_keyed_glob", [](HostCache& c, py::bytes pattern, uint32_t stale_at,
                                   uint32_t expire_cap, uint32_t now) {
        const std::string p = pattern;
        KeyedGlob g;
        std::string why;
        if (!compile_keyed_glob(p, &g, &why)) throw py::value_error(why);
        return c.soften_keyed_glob(g, stale_at, expire_cap, now);
      }, py::arg("pattern"), py::arg("stale_at"), py::arg("expire_cap"), py::arg("now"))
      // rows, keys, out: host buffers as HbmCache.list_keyed's; prefix: the plain prefix
      // (LIST_GLOB: the plain pattern)
      .def("list_keyed", [](HostCache& c, uint32_t mode, py::bytes prefix, bool exact,
                            std::vector<uint64_t> tags, uint64_t start, uint32_t limit,
                            uint32_t key_cap, uint32_t now, uintptr_t rows, uintptr_t keys,
                            uintptr_t out) {
        const std::string p = prefix;
        c.list_keyed(mode, reinterpret_cast<const uint8_t*>(p.data()), (uint32_t)p.size(), exact,
                     tags.data(), (uint32_t)tags.size(), start, limit, key_cap, now,
                     P<ListRow>(rows), P<uint8_t>(keys), P<uint64_t>(out));
      }, py::arg("mode"), py::arg("prefix"), py::arg("exact"), py::arg("tags"), py::arg("start"),
         py::arg("limit"), py::arg("key_cap"), py::arg("now"), py::arg("rows"), py::arg("keys"),
         py::arg("out"))
      // host buffers as HbmCache.get_keyed_slices'
      .def("get_keyed_slices", [](HostCache& c, uintptr_t keys, uintptr_t key_bytes,
                                  uintptr_t key_offs, uintptr_t spec, int64_t n, uintptr_t rows,
                                  uintptr_t out, uint64_t out_cap, uintptr_t res, uint32_t now,
                                  uint64_t reserve, uintptr_t cond, uintptr_t cond_bytes) {
        py::gil_scoped_release nogil;
        c.get_keyed_slices(P<const Digest>(keys), P<const uint8_t>(key_bytes),
                           P<const int64_t>(key_offs), P<const SliceSpec>(spec), n,
                           P<SliceRow>(rows), P<uint8_t>(out), out_cap, P<uint64_t>(res), now,
                           reserve, P<const SliceCond>(cond), P<const uint8_t>(cond_bytes));
      }, py::arg("keys"), py::arg("key_bytes"), py::arg("key_offs"), py::arg("spec"), py::arg("n"),
         py::arg("rows"), py::arg("out"), py::arg("out_cap"), py::arg("res"), py::arg("now"),
         py::arg("reserve") = 0, py::arg("cond") = 0, py::arg("cond_bytes") = 0)
      .def("touch", [](HostCache& c, uintptr_t keys, uintptr_t expire, uintptr_t flags,
                       uintptr_t key_bytes, uintptr_t key_offs, int64_t n, uintptr_t hit,
                       uint32_t now) {
        py::gil_scoped_release nogil;
        c.touch(P<const Digest>(keys), P<const uint32_t>(expire), P<const uint32_t>(flags),
                P<const uint8_t>(key_bytes), P<const int64_t>(key_offs), n, P<uint8_t>(hit), now);
      }, py::arg("keys"), py::arg("expire"), py::arg("flags"), py::arg("key_bytes"),
         py::arg("key_offs"), py::arg("n"), py::arg("hit"), py::arg("now"))
      .def("sweep", [](HostCache& c, uint32_t now) {
        uint64_t live = 0, bytes = 0;
        c.sweep(now, &live, &bytes);
        return py::make_tuple(live, bytes);
      })
      .def("flush", &HostCache::flush)
      .def("debug_bucket", &HostCache::debug_bucket)
      .def("debug_hand", &HostCache::debug_hand)
      .def("debug_set_entry", &HostCache::debug_set_entry)
      .def("debug_set_hand", &HostCache::debug_set_hand, py::arg("hand"), py::arg("catch_up") = true)
      .def("export_keys", [](HostCache& c, uintptr_t out, uint64_t cap, uint32_t now) {
        return c.export_keys(P<Digest>(out), cap, now);
      })
      .def("save", [](HostCache& c, const std::string& path, std::vector<uint64_t> user) {
        user.resize(4);
        c.save(path, user.data());
      })
      .def("load", [](HostCache& c, const std::string& path) {
        std::vector<uint64_t> user(4);
        c.load(path, user.data());
        return user;
      })
      .def("counters", [](HostCache& c) { return counters_dict(c.counters()); })
      .def("head", &HostCache::head)
      .def("get", [](HostCache& c, py::bytes key, uint32_t now) -> py::object {
        std::string k = key;
        Digest d = digest_bytes(reinterpret_cast<const uint8_t*>(k.data()), k.size());
        std::vector<uint8_t> v;
        uint32_t flags = 0;
        if (!c.get_one(d, &v, &flags, now)) return py::none();
        return py::bytes(reinterpret_cast<const char*>(v.data()), v.size());
      })
      .def("set", [](HostCache& c, py::bytes key, py::bytes value, uint32_t flags,
                     uint32_t expire, uint32_t now) {
        std::string k = key, v = value;
        Digest d = digest_bytes(reinterpret_cast<const uint8_t*>(k.data()), k.size());
        c.set_one(d, reinterpret_cast<const uint8_t*>(v.data()), (uint32_t)v.size(), flags, expire,
                  now);
      });

  m.def("host_exclusive_scan", [](uintptr_t in, uintptr_t out, int64_t n) {
    host_exclusive_scan(P<const uint64_t>(in), P<uint64_t>(out), n);
  });
  m.def("host_segcopy", [](uintptr_t src, uintptr_t src_off, uintptr_t dst_off, int64_t n,
                           uintptr_t dst, uint64_t dst_cap) {
    host_segcopy(P<const uint8_t>(src), P<const uint64_t>(src_off), P<const uint64_t>(dst_off), n,
                 P<uint8_t>(dst), dst_cap);
  }, py::arg("src"), py::arg("src_off"), py::arg("dst_off"), py::arg("n"), py::arg("dst"),
     py::arg("dst_cap") = ~0ull);
  m.def("host_segcopy_sized", [](uintptr_t src, uintptr_t src_off, uintptr_t dst_off,
                                 uintptr_t seg_len, int64_t n, uintptr_t dst, uint64_t cap) {
    host_segcopy_sized(P<const uint8_t>(src), P<const uint64_t>(src_off),
                       P<const uint64_t>(dst_off), P<const uint64_t>(seg_len), n, P<uint8_t>(dst),
                       cap);
  }, py::arg("src"), py::arg("src_off"), py::arg("dst_off"), py::arg("seg_len"), py::arg("n"),
     py::arg("dst"), py::arg("cap") = ~0ull);
  m.def("host_digest_keys", [](uintptr_t bytes, uintptr_t offs, int64_t n, uintptr_t out) {
    host_digest_keys(P<const uint8_t>(bytes), P<const int64_t>(offs), n, P<Digest>(out));
  });
  m.def("host_route_keys", [](uintptr_t keys, int64_t n, uintptr_t pts, uintptr_t owner,
                              int32_t npts, uintptr_t dest, uintptr_t counts, int32_t nranks) {
    host_route_keys(P<const Digest>(keys), n, P<const uint32_t>(pts), P<const int32_t>(owner),
                    npts, P<int32_t>(dest), P<int64_t>(counts), nranks);
  });
  m.def("host_scatter_by_dest", [](uintptr_t dest, uintptr_t base, int64_t n, int32_t nranks,
                                   uintptr_t cursor, uintptr_t perm) {
    host_scatter_by_dest(P<const int32_t>(dest), P<const int64_t>(base), n, nranks,
                         P<int64_t>(cursor), P<int64_t>(perm));
  });
  m.def("host_permute_records", [](uintptr_t in, uintptr_t perm, int64_t n, int32_t rec_bytes,
                                   uintptr_t out) {
    host_permute_records(P<const void>(in), P<const int64_t>(perm), n, rec_bytes, P<void>(out));
  });

  bind_http(m);
  bind_net(m);
  bind_router(m);
  bind_deflate(m);
}
