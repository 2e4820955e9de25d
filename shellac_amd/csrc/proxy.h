// The caching reverse proxy: native epoll reactors, pipelined client connections,
// pooled upstream connections, asynchronous cache backends.
//
// Reference map (src/python/shellac/server/Server.py):
//   C1 reactor loop            run()                 :442-478   -> Reactor::loop
//   C2 listener / accept       __init__/_new_connection :70-77, :137-153 -> accept_all
//   C3 client table + keep-alive policy (30 s / 1000 req) :22-24, :150-166 -> Client, gc()
//   C4 upstream pool + balancer _get_upstream_fd      :86-134   -> pick_upstream
//   C5 request path            _read_requests        :302-378  -> on_request
//   C6 response path           _read_responses       :380-440  -> on_upstream_response
//   C7 ordered pipelining      _responses/_stream_map :39-43, :342, :369-374 -> Slot FIFO
//   C9 write path              _write_response/_write_request :227-292 -> flush_client/flush_upstream
//   C12 teardown               _close_client/_close_upstream :168-217 -> close_client/close_upstream
// Deliberate fixes: reactor threads with SO_REUSEPORT and a real backlog (ref:
// one thread, listen(1)); non-blocking upstream connect (ref blocks, :126);
// EPOLLOUT armed only while bytes are pending (ref spins on idle upstreams, :439);
// client EOF closes the connection (ref leaks it until GC); atime starts at
// accept (ref starts at 0 so GC may kill fresh clients, :151); a non-keep-alive
// upstream no longer tears down its client (ref :423-425) — pending requests get
// a 502 instead; responses of departed clients still fill the cache.
#pragma once

#include <atomic>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "backend.h"
#include "net.h"

namespace shellac {

struct ProxyConfig {
  std::string bind = "0.0.0.0";
  uint16_t port = 8080;               // -p (Server.py:512)
  std::vector<Addr> upstreams;        // -s
  int threads = 1;
  std::vector<int> cpus;  // reactor i runs on cpus[i % size] (empty: unpinned)
  // > 0: a reactor that had work within the last spin_us polls epoll without sleeping
  // (a dedicated core: no wake-up IPI or idle-state exit per request under load)
  int spin_us = 0;
  uint32_t ttl = 170;                 // -t (Server.py:514)
  // --grace S (0 = off): a cacheable response is kept for ttl + S seconds and its flags word
  // holds the unix time at which it stops being fresh. A hit past that time is served stale
  // at once while one background request per key revalidates it upstream (If-None-Match /
  // If-Modified-Since from the stored head): a 304 extends the object in place
  // (CacheBackend::touch), any other cacheable answer replaces it, and an origin that fails
  // leaves the stale object servable until its hard expiry (RFC 5861; under policy rfc a
  // response's own stale-while-revalidate / stale-if-error replace S for that object).
  uint32_t grace = 0;
  bool compress = false;              // -z: gzip uncompressed text before caching
  // >= 0: that GPU does the -z compression, batched across reactors (deflate.h
  // GzipService, one window of gzip_batch_us; the binding installs it with
  // Proxy::set_compressor); the response completes when it returns
  int gzip_gpu = -1;
  int gzip_batch_us = 200;
  bool cache_enabled = true;
  std::string policy = "rfc";         // "rfc" | "reference" (cache every response)
  bool kill_switch = true;            // GET /kill stops the proxy (Server.py:329-331)
  bool kill_loopback_only = true;
  // The PURGE method (cache invalidation): "off" (a PURGE request is handled like any other
  // method: forwarded upstream), "loopback" (clients on 127/8 only, others get 403), "any".
  // `PURGE <url>` removes the URL's object and all its Vary variants; with the header
  // `X-Purge-Mode: prefix` every object whose key starts with the URL's key. With the header
  // `X-Purge-Soft: 1` and grace != 0 the same objects are kept and made stale now instead
  // (PurgeAction::soften; their lives capped at now + grace, never extended);
  // without grace, or where the tier cannot, it is a hard purge answered with "soft":false.
  std::string purge = "off";
  // Purge by surrogate key (Varnish xkey, Fastly Surrogate-Key, Cloudflare Cache-Tag): the
  // name of the response header that lists an object's tags, separated by spaces, tabs or
  // commas; empty (the default) turns the feature off. A response that carries it is stored
  // behind a tag block (keyed.h; more than 32 distinct tags: the overflow block) and the
  // header is passed on as it is. `PURGE` with `X-Purge-Mode: tag` takes 1..64 tags from the
  // request's header of this name (the URL is ignored) and removes every object that
  // carries one of them; with `X-Purge-Soft: 1` and grace they are made stale instead. A
  // stored tag block is stripped from a hit whether or not the option is set.
  // `PURGE` with `X-Purge-Mode: glob` (no option of its own: `purge` governs it) takes the
  // URL's key as a pattern in which '*' matches any run of bytes and removes, or with
  // `X-Purge-Soft: 1` and grace softens, every object whose key up to its first 0x1f matches
  // it from end to end (keyed.h), Vary variants with their URL.
  std::string tag_header;
  // "off" (the default: /_shellac/objects is an ordinary URL), "loopback" or "any": who may
  // GET /_shellac/objects, the listing of what is cached (by ?prefix=, ?key=, ?tag=a,b,
  // ?glob=PATTERN or everything, &limit= and &after= to page). Read-only.
  std::string inspect = "off";
  // Partial hits (off by default: every request is answered as without it). A cache-eligible
  // GET with `Range: bytes=` holding exactly one range and no `If-Range`, and under policy rfc
  // a HEAD, ask the tier for the object's head and one byte window (CacheBackend::get_part;
  // the HBM tier cuts them on the GPU) and are answered from the cache: 206 Partial Content
  // with Content-Range, 416 with `Content-Range: bytes */length`, or the stored head without
  // a body. Several ranges, other units, invalid specs and If-Range ignore the header (200, as
  // RFC 9110 allows). What cannot be answered exactly from head and window (a stored status
  // other than 200, Transfer-Encoding, a Content-Length that is not the body's, a gzip-coded
  // object for a client that did not ask for gzip, an object already stale under grace, a
  // value that is no sliceable response) is answered as without the option after a whole GET
  // (`partial_fallbacks`). A HEAD miss is forwarded and its response not cached, as without
  // it. Fills keep the origin's Accept-Ranges header instead of dropping it.
  bool partial_hits = false;
  // Answer a client's own validators from the cache (default off: every request is answered
  // as without it). A cacheable GET without Authorization, and a HEAD that partial_hits serves,
  // with If-None-Match (else If-Modified-Since; neither beside If-Match or
  // If-Unmodified-Since) asks the tier with CacheBackend::get_part_if, which compares the
  // stored ETag / Last-Modified where the object lies (on the GPU for the HBM tier): a match
  // whose stored status is 200 is answered 304 Not Modified from the stored head (counted in
  // `not_modified_304`, and as a hit), anything else as without the header. With partial_hits,
  // `Range` + `If-Range` is one trip too: 206 if the validator matches (strong tag, or the
  // Last-Modified value byte for byte), the whole object in a 200 if not. If-Modified-Since
  // matches only the exact Last-Modified value; stored headers are not updated from a 304.
  bool conditional_hits = false;
  // cache key = Host + URL (ref: URL only). The Python/CLI layer defaults it on for
  // policy rfc (vhosts must not share entries) and off for policy reference.
  bool key_host = false;
  int client_timeout = 30;            // CLIENT_TIMEOUT (Server.py:23)
  int client_max_reqs = 1000;         // CLIENT_MAX_REQS (Server.py:24)
  std::string balance = "random";     // random (ref :123) | roundrobin | leastconn
  int upstream_retry_s = 2;           // a failed upstream is skipped for this long
  // Active health checks (the reference's "todo: check that servers are responsive",
  // Server.py:532): when `health_path` is set, a checker thread sends
  // `GET <health_path>` to every upstream each `health_interval_ms`; `health_fails`
  // consecutive failures (connect error, timeout, or a status >= 400) take it out of
  // rotation, `health_passes` consecutive successes bring it back.
  std::string health_path;
  int health_interval_ms = 1000;
  int health_timeout_ms = 500;
  int health_fails = 2;
  int health_passes = 1;
  bool decode_gzip = false;           // inflate + re-deflate every miss like the reference
  // cap on any inflate the proxy runs (--decode-gzip bodies, identity variants for
  // clients without gzip): a larger body is a decompression bomb and fails (502)
  uint64_t max_inflate_bytes = 64ull << 20;
  // Responses whose body exceeds this are streamed to the client as they arrive and not
  // cached (the reference buffers every object whole, Server.py:408-421).
  uint64_t stream_bytes = 1 << 20;
  // A streamed response stops reading its upstream while this much waits for the
  // client, and resumes below a quarter of it.
  uint64_t stream_high_water = 8 << 20;
  int backlog = 1024;
  int max_fds = 1 << 16;  // fd table reserved at start (capped by RLIMIT_NOFILE)
  std::string server_name = "Shellac/0.2.0";
};

class Reactor;

class Proxy {
 public:
  Proxy(const ProxyConfig& cfg, std::shared_ptr<CacheBackend> backend);
  ~Proxy();
  void start();               // bind + spawn reactor threads
  void wait();                // block until stop()
  void stop();
  bool running() const { return running_; }
  uint16_t port() const { return port_; }
  std::string stats_json();
  const ProxyConfig& config() const { return cfg_; }
  CacheBackend* backend() { return backend_.get(); }
  // -z compression off the reactor threads (before start(); null = zlib inline)
  void set_compressor(std::shared_ptr<Compressor> c) { gzip_ = std::move(c); }

  // upstream health (shared by all reactors): passive (failed connects) and active
  bool upstream_up(int idx, double now) const;
  bool upstream_healthy(int idx) const { return !health_down_[idx].load(); }
  void upstream_failed(int idx, double now);
  int next_rr() { return rr_++; }

  // Purges and fills in flight: a miss fetched from the origin before a purge must not be
  // stored after it. Every purge takes a generation and is remembered in a small ring; a
  // fetch remembers the generation when it is forwarded, and its fill is delivered but not
  // cached if a newer purge matches its key or the ring has wrapped past its generation.
  static constexpr size_t kPurgeRing = 64;
  uint64_t purge_generation() const { return purge_gen_.load(std::memory_order_acquire); }
  void note_purge(KeyedSelector what);
  // `key`: the key the object would be stored under; `base_key`: its URL key (an exact
  // purge of the URL covers every variant)
  // `tags`: the object's tag hashes (null: it has none), `overflow`: it named too many — a
  // tag purge since `gen` that names one of them, or any tag purge for an overflowing
  // object, refuses the fill as a key purge does (KeyedSelector::matches_fill has the rules)
  bool purged_since(uint64_t gen, const std::string& key, const std::string& base_key,
                    const std::vector<uint64_t>* tags = nullptr, bool overflow = false);

 private:
  friend class Reactor;
  ProxyConfig cfg_;
  std::shared_ptr<CacheBackend> backend_;
  std::vector<std::unique_ptr<Reactor>> reactors_;
  std::vector<std::thread> threads_;
  // declared after reactors_: released before them (a GzipService joins its thread
  // then), so a late completion still posts into a live reactor
  std::shared_ptr<Compressor> gzip_;
  std::atomic<bool> running_{false};
  uint16_t port_ = 0;
  std::unique_ptr<std::atomic<double>[]> up_down_until_;
  std::unique_ptr<std::atomic<bool>[]> health_down_;
  std::atomic<uint64_t> health_checks_{0}, health_transitions_{0};
  std::thread health_th_;
  void health_loop();
  std::atomic<int> rr_{0};
  struct PurgeRec {
    uint64_t gen = 0;
    KeyedSelector what;
  };
  std::atomic<uint64_t> purge_gen_{0};
  std::mutex purge_mu_;
  std::vector<PurgeRec> purge_ring_;  // slot gen % kPurgeRing
  std::mutex wait_mu_;
  double start_time_ = 0;
};

// Who may PURGE (ProxyConfig::purge) and what counts as a loopback client: the predicates
// the reactor applies to a connection's peer address (IPv4, host byte order) at accept and
// to a PURGE request. "off" admits nobody (the method is not handled at all).
inline bool ipv4_is_loopback(uint32_t addr_host_order) { return (addr_host_order >> 24) == 127; }
inline bool purge_allowed(const std::string& mode, bool client_loopback) {
  return mode == "any" || (mode == "loopback" && client_loopback);
}

// The stats JSON (Proxy::stats_json) as Prometheus text-format samples (GET
// /_shellac/metrics): nested keys joined with '_' under `shellac_`, array elements as an
// `i` label, string fields as labels of `shellac_info`.
std::string prometheus_text(const std::string& stats_json);

}  // namespace shellac
