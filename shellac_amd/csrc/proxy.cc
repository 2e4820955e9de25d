// Native caching reverse proxy (see proxy.h for the reference map and fixes).
#include "proxy.h"

#include <poll.h>
#include <sys/epoll.h>
#include <pthread.h>
#include <sys/eventfd.h>
#include <sys/timerfd.h>
#include <sys/uio.h>

#include <algorithm>
#include <cctype>
#include <chrono>
#include <cstdlib>
#include <cmath>
#include <cstdio>
#include <ctime>
#include <deque>
#include <random>
#include <sstream>
#include <unordered_map>

#include "http.h"
#include "keyed.h"

namespace shellac {

namespace {

constexpr uint64_t kListenId = 1, kEventId = 2, kTimerId = 3, kFirstConnId = 16;
constexpr int kHistBuckets = 40;

std::string simple_response(int code, const char* reason, const std::string& server,
                            const std::string& body, const char* ctype = "text/plain",
                            bool close = false) {
  std::string s = "HTTP/1.1 " + std::to_string(code) + " " + reason + "\r\nServer: " + server +
                  "\r\nContent-Type: " + ctype + "\r\nContent-Length: " +
                  std::to_string(body.size()) + "\r\nConnection: " +
                  (close ? "close" : "keep-alive") + "\r\n\r\n";
  return s + body;
}

bool contains_ci(const std::string* h, const char* needle) {
  if (!h) return false;
  return to_lower(*h).find(needle) != std::string::npos;
}

// Cache-Control max-age / s-maxage (seconds), -1 if absent.
long cc_max_age(const std::string* cc) {
  if (!cc) return -1;
  const std::string s = to_lower(*cc);
  long best = -1;
  for (const char* k : {"s-maxage=", "max-age="}) {
    const size_t p = s.find(k);
    if (p != std::string::npos) {
      best = std::strtol(s.c_str() + p + std::strlen(k), nullptr, 10);
      break;
    }
  }
  return best;
}

// A Cache-Control directive `name=N` (seconds; `name` lower case with its '='), -1 if absent.
long cc_seconds(const std::string* cc, const char* name) {
  if (!cc) return -1;
  const std::string s = to_lower(*cc);
  const size_t p = s.find(name);
  if (p == std::string::npos) return -1;
  return std::strtol(s.c_str() + p + std::strlen(name), nullptr, 10);
}

uint32_t unix_now() { return (uint32_t)time(nullptr); }

// The value of header `lname` ("etag:", lower case with its colon) in a serialized
// response's head, trimmed; empty if the head has none.
std::string object_header(std::string_view ov, std::string_view lname) {
  const size_t eoh = ov.find("\r\n\r\n");
  if (eoh == std::string_view::npos) return std::string();
  size_t pos = ov.find("\r\n");
  while (pos != std::string_view::npos && pos < eoh) {
    const size_t ls = pos + 2;
    const size_t le = ov.find("\r\n", ls);
    const std::string_view line = ov.substr(ls, le - ls);
    if (line.size() > lname.size()) {
      bool match = true;
      for (size_t i = 0; i < lname.size() && match; ++i)
        match = (char)std::tolower((unsigned char)line[i]) == lname[i];
      if (match) {
        size_t a = lname.size(), b = line.size();
        while (a < b && (line[a] == ' ' || line[a] == '\t')) ++a;
        while (b > a && (line[b - 1] == ' ' || line[b - 1] == '\t')) --b;
        return std::string(line.substr(a, b - a));
      }
    }
    pos = le;
  }
  return std::string();
}

// ---- content negotiation + Vary (policy "rfc") ----------------------------------------
// The proxy forces `Accept-Encoding: gzip` upstream (Server.py:358), so one URL is cached
// once, usually gzip-coded; a client that did not ask for gzip gets the identity variant
// decoded from it on the way out (deliver()). Responses that Vary on request headers
// other than Accept-Encoding are stored per variant: a marker under the URL key names the
// headers, and the object lives under URL + the request's values of those headers.
const std::string kVaryMarker = "\x01SHELLAC-VARY\n";  // objects always start with "HTTP/"

bool is_vary_marker(std::string_view v) {
  return v.size() >= kVaryMarker.size() && v.compare(0, kVaryMarker.size(), kVaryMarker) == 0;
}

std::vector<std::string> split_names(const std::string& list) {
  std::vector<std::string> out;
  size_t i = 0;
  while (i <= list.size()) {
    size_t j = list.find(',', i);
    if (j == std::string::npos) j = list.size();
    size_t a = i, b = j;
    while (a < b && (list[a] == ' ' || list[a] == '\t')) ++a;
    while (b > a && (list[b - 1] == ' ' || list[b - 1] == '\t')) --b;
    if (b > a) out.push_back(to_lower(list.substr(a, b - a)));
    i = j + 1;
  }
  return out;
}

// Request headers a response varies on, sorted, without accept-encoding (negotiated by
// the proxy itself); {"*"} = varies on something outside the request (never cached).
std::vector<std::string> vary_names(const HttpParser& r) {
  std::vector<std::string> names;
  for (const auto& h : r.headers()) {
    if (h.first != "vary") continue;
    for (auto& n : split_names(h.second)) {
      if (n == "*") return {"*"};
      if (n != "accept-encoding" && std::find(names.begin(), names.end(), n) == names.end())
        names.push_back(std::move(n));
    }
  }
  std::sort(names.begin(), names.end());
  return names;
}

std::vector<std::string> marker_names(std::string_view v) {
  return split_names(std::string(v.substr(kVaryMarker.size())));
}

// Secondary key of one variant: URL key + the request's values of the varied headers.
// Repeated headers combine in order with "," (RFC 7230 §3.2.2: `X: a` + `X: b` is the
// same field value as `X: a,b`, so they select the same variant), and each combined value
// is length-prefixed, so no value bytes (separators included) can forge another key.
// Names are tokens from the response's Vary header (no separator bytes).
std::string vary_key(const std::string& base, const std::vector<std::string>& names,
                     const std::vector<Header>& req) {
  std::string k = base;
  k += '\x1f';
  std::string v;
  for (const auto& n : names) {
    v.clear();
    bool first = true;
    for (const auto& h : req)
      if (h.first == n) {
        if (!first) v += ',';
        v += h.second;
        first = false;
      }
    k += n;
    k += '=';
    k += std::to_string(v.size());
    k += ':';
    k += v;
  }
  return k;
}

// Does the serialized response's head carry Content-Encoding: gzip?
bool object_is_gzip(std::string_view ov) {
  const size_t eoh = ov.find("\r\n\r\n");
  if (eoh == std::string_view::npos) return false;
  size_t pos = ov.find("\r\n");
  while (pos != std::string_view::npos && pos < eoh) {
    const size_t ls = pos + 2;
    const size_t le = ov.find("\r\n", ls);
    const std::string_view line = ov.substr(ls, le - ls);
    static constexpr std::string_view kCe = "content-encoding:";
    if (line.size() > kCe.size()) {
      bool match = true;
      for (size_t i = 0; i < kCe.size() && match; ++i)
        match = (char)std::tolower((unsigned char)line[i]) == kCe[i];
      if (match) return to_lower(std::string(line.substr(kCe.size()))).find("gzip") != std::string::npos;
    }
    pos = le;
  }
  return false;
}

// Identity variant of a gzip-coded cached response (body inflated, capped at `cap` bytes;
// Content-Encoding dropped, Content-Length recomputed, Vary kept). nullptr on a corrupt
// or oversized body.
Bytes identity_variant(const Bytes& obj, uint64_t cap) {
  HttpParser r(false);
  r.parse(obj->data(), obj->size());
  if (!r.message_complete() && !r.finish()) return nullptr;
  std::string body;
  if (!gzip_decompress(r.body(), &body, cap)) return nullptr;
  r.remove_header("content-encoding");
  r.mutable_body() = std::move(body);
  return std::make_shared<const std::string>(r.serialize());
}

}  // namespace

struct Slot {
  uint64_t seq = 0;
  StreamBuf out;
  bool ready = false;
  bool streaming = false;  // response bytes flow out before the response is complete
  uint64_t stream_up = 0;  // id of the upstream feeding a streamed response
  bool close_after = false;
  std::string fwd;  // serialized request for the miss path (built on the first forward)
  // The parsed request, kept (not serialized) while the cache answers: a hit never pays
  // for re-serializing a request it does not forward. Returned to the reactor's pool.
  std::unique_ptr<HttpParser> req;
  std::string key;
  std::string base_key;  // URL (+Host) key; `key` becomes a variant key after a Vary marker
  Digest d{};
  bool lookup = false, head = false, client_gzip = false;
  bool vary_probe = false;  // `key` is a variant key (second lookup after a marker)
  // --partial-hits: the request asks the tier for the object's head and the window `spec`
  // (a Range GET, or a HEAD under policy rfc, which has lookup == false)
  bool part = false;
  SliceSpec spec{};
  // --conditional-hits: the client's validators the tier compares with the stored ones
  // (kCondNone: the request is not conditional); `ranged`: it carries a usable Range
  PartCond cond;
  bool ranged = false;
  // request headers, kept for the miss path when a response may Vary (policy rfc)
  std::shared_ptr<const std::vector<Header>> req_headers;
  Bytes vary_marker;  // --grace: the URL's marker a variant lookup went through
  int attempts = 0;
  double t0 = 0;
};

struct Conn {
  int fd = -1;
  int kind = 0;  // 0 client, 1 upstream
  uint64_t id = 0;
  double ctime = 0, atime = 0;
  bool dead = false;
  bool out_armed = false;
  bool in_paused = false;  // EPOLLIN withheld (backpressure from a slow client)
  virtual ~Conn() = default;
};

struct Upstream;

struct Client : Conn {
  std::unique_ptr<HttpParser> req = std::make_unique<HttpParser>(true);
  std::deque<std::unique_ptr<Slot>> slots;
  uint64_t next_seq = 1;
  Upstream* up = nullptr;
  int nreq = 0;
  bool closing = false;  // stop parsing (bad request / EOF)
  bool eof = false;      // peer finished sending: close after the last response
  bool loopback = false;
};

struct Pend {
  uint64_t client_id, seq;
  std::string key;
  Digest d;
  bool lookup, head, client_gzip;
  std::string base_key;
  std::shared_ptr<const std::vector<Header>> req_headers;
  uint64_t purge_gen = 0;  // Proxy::purge_generation() when the fetch was forwarded
  // A background revalidation (--grace): no client slot (client_id 0); `stale` is the object
  // that was served stale, `marker` its URL's Vary marker (null: the key is the URL's).
  bool reval = false;
  Bytes stale, marker;
  // `stale` as the tier holds it, with its tag block (null: it has none): what a
  // revalidation stores again
  Bytes stale_raw;
};

struct Upstream : Conn {
  int server = 0;
  bool connected = false;
  StreamBuf out;
  std::unique_ptr<HttpParser> resp;
  std::deque<Pend> pend;
  Client* owner = nullptr;
  double ka_timeout = -1;
  int ka_max = 1 << 30;
  int count = 0;
  bool streaming = false;       // the front response is being streamed through
  bool stream_chunked = false;  // ... re-framed as chunked (unknown length)
};

// The distinct tags of a tag header's value: split on space, tab and comma, empty tokens
// dropped, duplicates collapsed; as hashes (keyed.h tag_hash), in order of first appearance.
static std::vector<uint64_t> tag_hashes_of(const std::string& value) {
  std::vector<uint64_t> out;
  size_t pos = 0;
  while (pos < value.size()) {
    const size_t e = std::min(value.find_first_of(" \t,", pos), value.size());
    if (e > pos) {
      const uint64_t h = tag_hash(value.data() + pos, e - pos);
      if (std::find(out.begin(), out.end(), h) == out.end()) out.push_back(h);
    }
    pos = e + 1;
  }
  return out;
}

// The 400 body of a tag list no selector can be made of.
static std::string bad_tags(bool no_header, const KeyedSelector& what) {
  return std::string("{\"mode\":\"tag\",\"error\":\"") +
         (no_header              ? "no tag header is configured"
          : what.hashes.empty() ? "the request names no tags"
                                : "more than 64 tags") + "\"}";
}
static std::string bad_glob(const std::string& why) {
  return "{\"mode\":\"glob\",\"error\":\"" + why + "\"}";
}

// What a PURGE asks. X-Purge-Mode (any case) names the mode: none or an unknown one is exact.
//   exact : the object of the request's key, then `variants`, its Vary variants;
//   prefix: every object whose key starts with the request's key;
//   tag   : every object that carries one of the 1..64 tags in the request's header named by
//           ProxyConfig::tag_header (the URL is ignored);
//   glob  : the request's key (Host + URL with key_host, else the URL) is the pattern, '*' the
//           wildcard: every '\\' is escaped before compiling, so every other byte of the URL is
//           literal, a '?' before a query string included. An object is selected when its
//           key, up to the first '\x1f', matches (keyed.h), a Vary marker with its variants.
struct PurgeRequest {
  KeyedSelector what, variants;
  bool soft = false, dry_run = false;  // (a dry run ignores `soft`: nothing changes either way)
  bool exact() const { return what.kind == KeyedSelector::Kind::Exact; }
  bool by_tag() const { return what.kind == KeyedSelector::Kind::Tags; }
  // how an answer begins, and its "tags" field (tag mode only)
  std::string head() const {
    using Kind = KeyedSelector::Kind;
    return std::string("{\"mode\":\"") + (what.kind == Kind::Prefix ? "prefix" : by_tag() ? "tag"
                                          : what.kind == Kind::Glob ? "glob" : "exact") + "\",";
  }
  std::string tags_field() const {
    return by_tag() ? "\"tags\":" + std::to_string(what.hashes.size()) + "," : std::string();
  }
};

// The request's headers and key into *rq; *bad: not empty: the request is a 400 with this body
// (a tag list or a glob no selector can be made of). An empty key makes a refused prefix or exact
// selector that goes on to the tier, which answers "cannot".
static void parse_purge(const HttpParser& q, const std::string& key, const ProxyConfig& cfg,
                        PurgeRequest* rq, std::string* bad) {
  const std::string* h = q.header("x-purge-mode");
  const std::string mode = h ? to_lower(*h) : std::string();
  h = q.header("x-purge-soft");
  rq->soft = h && *h == "1";
  h = q.header("x-purge-dry-run");
  rq->dry_run = h && *h == "1";
  if (mode == "tag") {
    const std::string* list = cfg.tag_header.empty() ? nullptr : q.header(cfg.tag_header);
    rq->what = KeyedSelector::tags(list ? tag_hashes_of(*list) : std::vector<uint64_t>());
    if (!rq->what.valid()) *bad = bad_tags(cfg.tag_header.empty(), rq->what);
  } else if (mode == "glob") {
    std::string why;
    rq->what = KeyedSelector::glob(keyed_glob_escape(key, true), &why);
    if (!rq->what.valid()) *bad = bad_glob(why);
  } else if (mode == "prefix") {
    rq->what = KeyedSelector::prefix(key);
  } else {
    rq->what = KeyedSelector::exact(key);
    rq->variants = KeyedSelector::prefix(key + '\x1f');
  }
}

class Reactor : public Executor {
 public:
  Reactor(Proxy* px, int id, int listen_fd);
  ~Reactor() override;
  void loop();
  void post(std::function<void()> fn) override;
  void post_batch(std::vector<std::function<void()>>& fns) override;
  void wake() {
    uint64_t one = 1;
    (void)!write(evfd_, &one, 8);
  }

  // stats (read by Proxy::stats_json from another thread)
  std::atomic<uint64_t> requests{0}, hits{0}, misses{0}, upstream_reqs{0}, responses{0},
      bytes_out{0}, errors{0}, clients{0}, upstreams{0}, accepts{0}, gc_closed{0},
      cache_sets{0}, bad_requests{0}, upstream_failures{0}, retries{0}, collapsed{0},
      streamed{0}, stream_pauses{0}, gzip_gpu_bodies{0}, gzip_gpu_inflated{0}, identity_decoded{0},
      vary_stored{0},
      vary_hits{0}, purge_requests{0}, purged_objects{0}, purge_denied{0}, fills_purged{0},
      soft_purge_requests{0}, softened_objects{0}, tag_purge_requests{0},
      tag_purged_objects{0}, tag_softened_objects{0}, tagged_fills{0}, inspect_requests{0},
      purge_dry_runs{0}, purge_glob_requests{0};
  // --partial-hits: Range requests asked of the cache, their 206 and 416 answers, HEADs
  // answered from the cache, and requests answered from a whole GET after all
  std::atomic<uint64_t> range_requests{0}, range_206{0}, range_416{0}, head_hits{0},
      partial_fallbacks{0};
  // --conditional-hits: requests asked of the cache under a condition, their 304 answers, and
  // how If-Range validators compared
  std::atomic<uint64_t> conditional_requests{0}, not_modified_304{0}, if_range_matched{0},
      if_range_failed{0};
  // --grace: stale hits served, background revalidations started, their 304s, the objects
  // those extended in place / stored again, and revalidations the origin failed
  std::atomic<uint64_t> stale_served{0}, revalidations{0}, revalidated_304{0},
      revalidate_touched{0}, revalidate_restored{0}, revalidate_errors{0};
  // event-loop health: the longest iteration (events handled between two epoll_waits)
  // and how many took over 10 ms — a reactor that stalls stops accepting connections
  std::atomic<uint64_t> loop_max_us{0}, loop_slow{0}, client_resets{0};
  // longest single step per kind: accept, client event, upstream event, posted
  // completions, timer (gc)
  std::atomic<uint64_t> phase_max_us[5] = {};
  void phase_done(int k, double t0) {
    const uint64_t us = (uint64_t)((now_s() - t0) * 1e6);
    if (us > phase_max_us[k].load(std::memory_order_relaxed)) phase_max_us[k].store(us);
  }
  std::atomic<uint64_t> hist[kHistBuckets] = {};

 private:
  void accept_all();
  void on_client(Client* c, uint32_t ev);
  void on_upstream(Upstream* u, uint32_t ev);
  void on_request(Client* c);
  void on_purge(Client* c, Slot* s, const HttpParser& q, const std::string& key);
  using PurgeRef = std::shared_ptr<const PurgeRequest>;
  void hard_purge(uint64_t cid, uint64_t seq, const PurgeRef& rq, bool soft_asked);
  void soft_purge(uint64_t cid, uint64_t seq, const PurgeRef& rq);
  void dry_purge(uint64_t cid, uint64_t seq, const PurgeRef& rq);
  void answer_purge(uint64_t cid, uint64_t seq, int code, const char* reason,
                    const std::string& body);
  void on_inspect(Client* c, Slot* s, const std::string& qs);
  void on_cache(uint64_t cid, uint64_t seq, bool hit, CacheValue v);
  void ask_part(Slot* s, uint64_t cid);
  void on_part(uint64_t cid, uint64_t seq, PartValue p);
  bool answer_part(Client* c, Slot* s, const PartValue& p);
  bool not_modified_exact(const Slot* s, std::string_view hv) const;
  void answer_not_modified(Client* c, Slot* s, std::string_view hv);
  void forward(Client* c, Slot* s);
  static std::string upstream_request(HttpParser& q);
  std::unique_ptr<HttpParser> take_parser();
  void give_parser(std::unique_ptr<HttpParser> p);
  std::vector<std::unique_ptr<HttpParser>> parser_pool_;
  void on_upstream_response(Upstream* u);
  void finish_response(HttpParser& r, const Pend& p);
  void rewrite_response_headers(HttpParser& r);
  void pause_input(Conn* c, bool paused);
  void rearm(Conn* c);
  bool maybe_stream(Upstream* u);
  void resume_stream(uint64_t up_id);
  void stream_out(Upstream* u, std::string data, bool last);
  Upstream* pick_upstream(Client* c);
  Upstream* connect_upstream();  // a new connection to a server in rotation (no owner yet)
  int choose_server();
  // --grace (ProxyConfig::grace)
  uint32_t grace_for(const HttpParser& r) const;
  void revalidate(Slot* s, const Bytes& stale, const Bytes& raw);
  void revalidation_answered(HttpParser& r, const Pend& p);
  void revalidation_failed(const Pend& p);
  // keys whose revalidation failed: no new attempt before this time (upstream_retry_s)
  std::unordered_map<std::string, double> reval_retry_at_;
  void flush_client(Client* c);
  void flush_upstream(Upstream* u);
  // `tail` (optional): bytes sent right after `data`, shared, not copied (a 206's window)
  void complete_slot(Client* c, Slot* s, Bytes data, Bytes tail = nullptr);
  void deliver(Client* c, Slot* s, Bytes obj);
  void fail_pend(Pend& p, int code, const char* reason);
  void release_waiters(const std::string& key, Bytes obj);
  void close_client(Client* c);
  void close_upstream(Upstream* u);
  void arm(Conn* c, bool out);
  void gc();
  Client* find_client(uint64_t id);
  Slot* find_slot(Client* c, uint64_t seq);
  void drain_posted();
  bool cacheable_response(const HttpParser& r, uint32_t* ttl) const;

  Proxy* px_;
  const ProxyConfig& cfg_;
  int id_;
  int epfd_ = -1, listen_fd_ = -1, evfd_ = -1, timerfd_ = -1;
  uint64_t next_id_ = kFirstConnId;
  std::unordered_map<uint64_t, Conn*> conns_;
  std::vector<Upstream*> pool_;
  std::vector<Conn*> graveyard_;
  std::mutex post_mu_;
  std::vector<std::function<void()>> posted_;
  // the loop is busy-polling (epoll_wait(0), posted work drained every pass): posters
  // skip the eventfd write — a syscall on their side and a read on this one, per
  // completion (the HBM batcher posts one per GPU batch)
  std::atomic<bool> spinning_{false};
  std::mt19937 rng_;
  std::vector<char> buf_;
  // collapsed forwarding: key -> requests waiting on the in-flight miss of the
  // same object (only the first one goes upstream)
  std::unordered_map<std::string, std::vector<std::pair<uint64_t, uint64_t>>> inflight_;
  // servers that answered "Connection: close": never pipeline onto them
  std::vector<char> server_nka_;
};

// =====================================================================================
Reactor::Reactor(Proxy* px, int id, int listen_fd)
    : px_(px), cfg_(px->cfg_), id_(id), listen_fd_(listen_fd), rng_(1234 + id), buf_(1 << 16),
      server_nka_(px->cfg_.upstreams.size(), 0) {
  epfd_ = epoll_create1(EPOLL_CLOEXEC);
  evfd_ = eventfd(0, EFD_NONBLOCK | EFD_CLOEXEC);
  timerfd_ = timerfd_create(CLOCK_MONOTONIC, TFD_NONBLOCK | TFD_CLOEXEC);
  itimerspec its{};
  its.it_interval.tv_sec = 1;
  its.it_value.tv_sec = 1;
  timerfd_settime(timerfd_, 0, &its, nullptr);
  epoll_event ev{};
  ev.events = EPOLLIN;
  ev.data.u64 = kListenId;
  epoll_ctl(epfd_, EPOLL_CTL_ADD, listen_fd_, &ev);
  ev.data.u64 = kEventId;
  epoll_ctl(epfd_, EPOLL_CTL_ADD, evfd_, &ev);
  ev.data.u64 = kTimerId;
  epoll_ctl(epfd_, EPOLL_CTL_ADD, timerfd_, &ev);
}

Reactor::~Reactor() {
  for (auto& kv : conns_) {
    close(kv.second->fd);
    delete kv.second;
  }
  for (Conn* c : graveyard_) delete c;
  close(listen_fd_);
  close(evfd_);
  close(timerfd_);
  close(epfd_);
}

void Reactor::post(std::function<void()> fn) {
  bool was_empty;
  {
    std::lock_guard<std::mutex> lk(post_mu_);
    was_empty = posted_.empty();
    posted_.push_back(std::move(fn));
  }
  // a non-empty queue already has a wake-up pending; a spinning loop needs none
  if (was_empty && !spinning_.load(std::memory_order_seq_cst)) wake();
}

void Reactor::post_batch(std::vector<std::function<void()>>& fns) {
  if (fns.empty()) return;
  bool was_empty;
  {
    std::lock_guard<std::mutex> lk(post_mu_);
    was_empty = posted_.empty();
    if (was_empty) {
      posted_.swap(fns);
    } else {
      for (auto& f : fns) posted_.push_back(std::move(f));
    }
  }
  fns.clear();
  if (was_empty && !spinning_.load(std::memory_order_seq_cst)) wake();
}

void Reactor::drain_posted() {
  std::vector<std::function<void()>> fns;
  {
    std::lock_guard<std::mutex> lk(post_mu_);
    fns.swap(posted_);
  }
  for (auto& f : fns) f();
}

void Reactor::arm(Conn* c, bool out) {
  if (c->dead || c->out_armed == out) return;
  c->out_armed = out;
  rearm(c);
}

void Reactor::pause_input(Conn* c, bool paused) {
  if (c->dead || c->in_paused == paused) return;
  c->in_paused = paused;
  rearm(c);
}

void Reactor::rearm(Conn* c) {
  epoll_event ev{};
  ev.events = (c->in_paused ? 0u : (uint32_t)(EPOLLIN | EPOLLRDHUP)) |
              (c->out_armed ? (uint32_t)EPOLLOUT : 0u);
  ev.data.u64 = c->id;
  epoll_ctl(epfd_, EPOLL_CTL_MOD, c->fd, &ev);
}

void Reactor::loop() {
  epoll_event evs[256];
  const double spin_s = cfg_.spin_us * 1e-6;
  double last_work = now_s();
  // the cache tier may take this thread's GETs directly (HbmBackend: the reactor writes
  // the edge-server job and polls its completion below, no batcher thread either way)
  CacheBackend* const be = px_->backend_.get();
  if (be) be->direct_attach(this);
  bool direct_busy = false;
  while (px_->running_) {
    const bool spin = spin_s > 0 && now_s() - last_work < spin_s;
    int timeout_ms = 0;
    if (spin) {
      spinning_.store(true, std::memory_order_seq_cst);
    } else {
      // leaving the spin: a poster that still saw spinning_ did not write the eventfd,
      // so look at the queue after clearing the flag (both seq_cst: one of the two sides
      // sees the other) and block only when it is empty
      spinning_.store(false, std::memory_order_seq_cst);
      std::lock_guard<std::mutex> lk(post_mu_);
      timeout_ms = posted_.empty() && !direct_busy ? 100 : 0;
    }
    const int n = epoll_wait(epfd_, evs, 256, timeout_ms);
    const double t_it = n > 0 ? now_s() : 0;
    if (n > 0 && spin_s > 0) last_work = t_it;
    for (int i = 0; i < n; ++i) {
      const uint64_t id = evs[i].data.u64;
      const double t0 = now_s();
      if (id == kListenId) {
        accept_all();
        phase_done(0, t0);
      } else if (id == kEventId) {
        uint64_t v;
        (void)!read(evfd_, &v, 8);
      } else if (id == kTimerId) {
        uint64_t v;
        (void)!read(timerfd_, &v, 8);
        gc();
        phase_done(4, t0);
      } else {
        auto it = conns_.find(id);
        if (it == conns_.end() || it->second->dead) continue;
        Conn* c = it->second;
        if (c->kind == 0) {
          on_client(static_cast<Client*>(c), evs[i].events);
          phase_done(1, t0);
        } else {
          on_upstream(static_cast<Upstream*>(c), evs[i].events);
          phase_done(2, t0);
        }
      }
    }
    {
      const double t0 = now_s();
      drain_posted();
      // GETs this iteration accepted go to the GPU now; finished ones are answered here
      if (be) {
        direct_busy = be->direct_service();
        if (direct_busy && spin_s > 0) last_work = t0;
      }
      phase_done(3, t0);
    }
    for (Conn* c : graveyard_) delete c;
    graveyard_.clear();
    if (n > 0) {
      const uint64_t us = (uint64_t)((now_s() - t_it) * 1e6);
      if (us > loop_max_us.load(std::memory_order_relaxed)) loop_max_us.store(us);
      if (us > 10000) loop_slow.fetch_add(1, std::memory_order_relaxed);
    }
  }
  if (be) be->direct_detach();  // answers (or hands to the batcher) what it still holds
}

void Reactor::accept_all() {
  for (;;) {
    sockaddr_in sa{};
    socklen_t len = sizeof sa;
    const int fd = accept4(listen_fd_, reinterpret_cast<sockaddr*>(&sa), &len,
                           SOCK_NONBLOCK | SOCK_CLOEXEC);
    if (fd < 0) return;
    set_nodelay(fd);
    auto* c = new Client();
    c->fd = fd;
    c->kind = 0;
    c->id = next_id_++;
    c->ctime = c->atime = now_s();
    c->loopback = ipv4_is_loopback(ntohl(sa.sin_addr.s_addr));
    conns_[c->id] = c;
    epoll_event ev{};
    ev.events = EPOLLIN | EPOLLRDHUP;
    ev.data.u64 = c->id;
    epoll_ctl(epfd_, EPOLL_CTL_ADD, fd, &ev);
    accepts++;
    clients++;
  }
}

Client* Reactor::find_client(uint64_t id) {
  auto it = conns_.find(id);
  if (it == conns_.end() || it->second->dead || it->second->kind != 0) return nullptr;
  return static_cast<Client*>(it->second);
}

Slot* Reactor::find_slot(Client* c, uint64_t seq) {
  for (auto& s : c->slots)
    if (s->seq == seq) return s.get();
  return nullptr;
}

// ---------------------------------------------------------------------------------
// client side
// ---------------------------------------------------------------------------------
void Reactor::on_client(Client* c, uint32_t ev) {
  if (ev & EPOLLOUT) flush_client(c);
  if (c->dead) return;
  if (ev & (EPOLLIN | EPOLLRDHUP | EPOLLHUP | EPOLLERR)) {
    for (;;) {
      const ssize_t r = recv(c->fd, buf_.data(), buf_.size(), 0);
      if (r > 0) {
        c->atime = now_s();
        const char* p = buf_.data();
        size_t n = (size_t)r;
        while (n > 0 && !c->dead && !c->closing) {
          const size_t used = c->req->parse(p, n);
          p += used;
          n -= used;
          if (c->req->error()) {
            bad_requests++;
            auto s = std::make_unique<Slot>();
            s->seq = c->next_seq++;
            s->out.write(simple_response(400, "Bad Request", cfg_.server_name, "bad request\n",
                                         "text/plain", true));
            s->out.close();
            s->ready = true;
            s->close_after = true;
            c->slots.push_back(std::move(s));
            c->closing = true;
            break;
          }
          if (c->req->message_complete()) {
            on_request(c);
            if (c->dead) return;
            if (c->req) c->req->reset();
            else c->req = take_parser();  // the request moved into its slot
          } else if (used == 0) {
            break;
          }
        }
        if (c->dead) return;
        if ((size_t)r < buf_.size()) break;
        continue;
      }
      if (r == 0) {  // client EOF: finish every queued response, then close
        c->eof = true;
        c->closing = true;
        if (c->slots.empty()) close_client(c);
        else flush_client(c);
        return;
      }
      if (errno == EAGAIN || errno == EWOULDBLOCK) break;
      // a client that resets its connection has just gone away; not a proxy error
      if (errno == ECONNRESET) client_resets++;
      else errors++;
      close_client(c);
      return;
    }
    flush_client(c);
  }
}

void Reactor::on_request(Client* c) {
  HttpParser& q = *c->req;
  c->nreq++;
  requests++;
  const std::string url = q.url();
  if (cfg_.kill_switch && url == "/kill" && (!cfg_.kill_loopback_only || c->loopback)) {
    // KILL SWITCH (Server.py:329-331: sys.exit(0))
    std::fprintf(stderr, "[shellac] /kill received; shutting down\n");
    px_->stop();
    return;
  }
  auto s = std::make_unique<Slot>();
  Slot* sp = s.get();
  s->seq = c->next_seq++;
  s->t0 = now_s();
  s->close_after = !q.keep_alive() || c->nreq >= cfg_.client_max_reqs;
  if (url == "/_shellac/stats" || url == "/_shellac/metrics") {
    // the same counters as JSON, or in the Prometheus text format for a scraper
    const bool prom = url == "/_shellac/metrics";
    s->out.write(simple_response(200, "OK", cfg_.server_name,
                                 prom ? prometheus_text(px_->stats_json()) : px_->stats_json(),
                                 prom ? "text/plain; version=0.0.4" : "application/json",
                                 s->close_after));
    s->out.close();
    s->ready = true;
    c->slots.push_back(std::move(s));
    flush_client(c);
    return;
  }
  const std::string& method = q.method();
  if (cfg_.inspect != "off" && method == "GET" && url.compare(0, 17, "/_shellac/objects") == 0 &&
      (url.size() == 17 || url[17] == '?')) {
    c->slots.push_back(std::move(s));
    on_inspect(c, sp, url.size() > 18 ? url.substr(18) : std::string());
    return;
  }
  if (method == "PURGE" && cfg_.purge != "off") {
    const std::string* host = q.header("host");
    const std::string key = cfg_.key_host && host ? *host + url : url;  // as a GET's
    c->slots.push_back(std::move(s));
    on_purge(c, sp, q, key);
    return;
  }
  s->head = method == "HEAD";
  s->client_gzip = contains_ci(q.header("accept-encoding"), "gzip");
  const std::string* host = q.header("host");
  s->key = cfg_.key_host && host ? *host + url : url;  // reference key: URL (Server.py:327)
  s->base_key = s->key;
  s->d = digest_bytes(reinterpret_cast<const uint8_t*>(s->key.data()), s->key.size());
  s->lookup = px_->cfg_.cache_enabled &&
              (cfg_.policy == "reference" || method == "GET") && !q.header("authorization");
  const bool cached_get = s->lookup && method == "GET";
  if (cfg_.partial_hits && px_->cfg_.cache_enabled && !q.header("authorization")) {
    if (cached_get) {
      const std::string* rg = q.header("range");
      s->part = rg && (cfg_.conditional_hits || !q.header("if-range")) &&
                parse_single_range(rg->data(), rg->size(), &s->spec);
      s->ranged = s->part;
    } else if (!s->lookup && s->head && cfg_.policy == "rfc") {
      s->spec = SliceSpec{};
      s->spec.kind = kSliceHead;
      s->part = true;
    }
  }
  // --conditional-hits (RFC 9110 13.2.2, reduced): If-None-Match is the condition, else
  // If-Modified-Since; a request with If-Match or If-Unmodified-Since is not conditional here.
  // If-Range counts only beside a usable Range, and a row carries one condition: with a
  // 304-condition as well the row asks for the whole object ("If-Range means 200 in full").
  if (cfg_.conditional_hits && px_->cfg_.cache_enabled && !q.header("authorization") &&
      (cached_get || s->part) && !q.header("if-match") && !q.header("if-unmodified-since")) {
    PartCond pc;
    if (const std::string* inm = q.header("if-none-match")) {
      if (parse_if_none_match(inm->data(), inm->size(), &pc)) s->cond = std::move(pc);
    } else if (const std::string* ims = q.header("if-modified-since")) {
      if (parse_if_modified_since(ims->data(), ims->size(), &pc)) s->cond = std::move(pc);
    }
    const std::string* ifr = s->ranged ? q.header("if-range") : nullptr;
    if (ifr && s->cond.kind == kCondNone && parse_if_range(ifr->data(), ifr->size(), &pc)) {
      s->cond = std::move(pc);
    } else if (ifr) {  // beside a 304-condition, or a validator that can never match
      if (s->cond.kind == kCondNone) if_range_failed++;
      s->ranged = false;
      s->part = s->cond.kind != kCondNone;
    }
    if (s->cond.kind != kCondNone) {
      conditional_requests++;
      if (!s->ranged && cached_get) {  // no usable Range: the whole object, or a 304
        s->spec = SliceSpec{};
        s->spec.kind = kSliceWhole;
        s->part = true;
      }
    }
  } else if (s->ranged && q.header("if-range")) {  // (If-Match beside it: as without the option)
    s->ranged = s->part = false;
  }
  if (s->lookup || s->part) s->req = std::move(c->req);  // serialized only if the cache misses
  else s->fwd = upstream_request(q);
  c->slots.push_back(std::move(s));
  if (sp->part) {
    if (sp->ranged) range_requests++;
    ask_part(sp, c->id);
  } else if (sp->lookup) {
    const uint64_t cid = c->id, seq = sp->seq;
    px_->backend_->get(sp->key, sp->d, this, [this, cid, seq](bool hit, CacheValue v) {
      on_cache(cid, seq, hit, std::move(v));
    });
  } else {
    forward(c, sp);
  }
}

// PURGE (ProxyConfig::purge): the request holds its slot like any other (pipelined order is
// kept) and is answered when the backend's callbacks arrive. One pipeline for every mode
// (PurgeRequest): the loopback rule (403), the request counters, what parse_purge refused
// (400), "no cache" (501), then
//   dry run (X-Purge-Dry-Run: 1): what the purge would hit, from the count-only list
//           (CacheBackend::list_objects with limit 0); nothing is removed or softened and
//           note_purge is not called, so a fill in flight is still stored;
//   soft    (X-Purge-Soft: 1 with --grace): the objects are kept and made stale now
//           (PurgeAction::soften: freshness time = now, life capped at now + grace), so the
//           next request is answered from the stale copy and revalidated in the background;
//   hard    otherwise, and where the tier answers a soft purge with -1: the objects are
//           removed, and a request that asked for a soft purge is told "soft":false.
// note_purge is called before the tier is touched, for a soft purge too: a fill or a
// revalidation that left before it must not store the object, or make it fresh again
// (purged_since drops it; a softened object stays stale and the next hit revalidates).
// Exact mode is two steps: the URL's object (for a URL whose responses Vary, the marker: a
// delete, or a soft scan), then its variants, which live under vary_key(base, ...) = base +
// '\x1f' + ...; deleting only the marker would make them reachable again once a new marker is
// stored. A tier that cannot scan answers 501, exact mode `"variants":-1`.
void Reactor::on_purge(Client* c, Slot* s, const HttpParser& q, const std::string& key) {
  const uint64_t cid = c->id, seq = s->seq;
  if (!purge_allowed(cfg_.purge, c->loopback)) {
    purge_denied++;
    answer_purge(cid, seq, 403, "Forbidden", "{\"error\":\"purge is allowed from loopback only\"}");
    return;
  }
  PurgeRequest rq;
  std::string bad;
  parse_purge(q, key, cfg_, &rq, &bad);
  if (!rq.dry_run) purge_requests++;
  if (!bad.empty()) {
    answer_purge(cid, seq, 400, "Bad Request", bad);
    return;
  }
  if (!px_->backend_ || !px_->cfg_.cache_enabled) {
    answer_purge(cid, seq, 501, "Not Implemented", "{\"error\":\"no cache\"}");
    return;
  }
  const PurgeRef r = std::make_shared<const PurgeRequest>(std::move(rq));
  if (r->dry_run) {
    purge_dry_runs++;
    dry_purge(cid, seq, r);
    return;
  }
  if (r->what.kind == KeyedSelector::Kind::Tags) tag_purge_requests++;
  if (r->what.kind == KeyedSelector::Kind::Glob) purge_glob_requests++;
  px_->note_purge(r->what);  // before the tier is touched: fills in flight are refused
  if (r->soft && cfg_.grace) soft_purge(cid, seq, r);  // (without --grace staleness has no meaning)
  else hard_purge(cid, seq, r, r->soft);
}

static const char* const kCannotScan = "\"error\":\"the cache tier cannot scan its keys\"}";

void Reactor::soft_purge(uint64_t cid, uint64_t seq, const PurgeRef& r) {
  CacheBackend* be = px_->backend_.get();
  const PurgeAction how = PurgeAction::soften(unix_now(), cfg_.grace);
  be->purge(r->what, how, this, [this, be, cid, seq, r, how](int64_t n) {
    if (n < 0) {  // the tier cannot: a hard purge that says so
      hard_purge(cid, seq, r, true);
      return;
    }
    const auto answer = [this, cid, seq, r, n](const int64_t* variants) {
      const uint64_t all = (uint64_t)n + (uint64_t)(variants && *variants > 0 ? *variants : 0);
      if (r->by_tag()) {
        tag_softened_objects += all;
      } else {
        soft_purge_requests++;
        softened_objects += all;
      }
      answer_purge(cid, seq, 200, "OK",
                   r->head() + "\"soft\":true," + r->tags_field() + "\"softened\":" +
                       std::to_string(n) +
                       (variants ? ",\"variants\":" + std::to_string(*variants < 0 ? -1 : *variants)
                                 : std::string()) + "}");
    };
    if (!r->exact()) {
      answer(nullptr);
      return;
    }
    be->purge(r->variants, how, this, [answer](int64_t m) { answer(&m); });
  });
}

// `soft_asked`: the request asked for a soft purge that cannot be had, which the answer says
// ("soft":false). Without it the answers are what they always were.
void Reactor::hard_purge(uint64_t cid, uint64_t seq, const PurgeRef& r, bool soft_asked) {
  CacheBackend* be = px_->backend_.get();
  const std::string head = r->head() + (soft_asked ? "\"soft\":false," : "");
  if (r->exact()) {
    const std::string& key = r->what.pattern;
    const Digest d = digest_bytes(reinterpret_cast<const uint8_t*>(key.data()), key.size());
    be->del(key, d, this, [this, be, cid, seq, r, head](bool found) {
      be->purge(r->variants, PurgeAction::remove(), this, [this, cid, seq, found, head](int64_t n) {
        purged_objects += (found ? 1 : 0) + (uint64_t)(n > 0 ? n : 0);
        answer_purge(cid, seq, 200, "OK",
                     head + "\"found\":" + (found ? "true" : "false") +
                         ",\"variants\":" + std::to_string(n < 0 ? -1 : n) + "}");
      });
    });
    return;
  }
  be->purge(r->what, PurgeAction::remove(), this, [this, cid, seq, r, head](int64_t n) {
    if (n < 0) {
      answer_purge(cid, seq, 501, "Not Implemented", head + kCannotScan);
      return;
    }
    (r->by_tag() ? tag_purged_objects : purged_objects) += (uint64_t)n;
    answer_purge(cid, seq, 200, "OK",
                 head + r->tags_field() + "\"purged\":" + std::to_string(n) + "}");
  });
}

void Reactor::dry_purge(uint64_t cid, uint64_t seq, const PurgeRef& r) {
  CacheBackend* be = px_->backend_.get();
  const std::string head = r->head() + "\"dry_run\":true," + r->tags_field();
  be->list_objects(ListQuery{r->what, 0, {}}, this, [this, be, cid, seq, r, head](ListResult l) {
    if (!l.ok) {
      answer_purge(cid, seq, 501, "Not Implemented", head + kCannotScan);
      return;
    }
    const std::string counts = head + "\"matched\":" + std::to_string(l.matched) +
                               ",\"bytes\":" + std::to_string(l.bytes);
    if (!r->exact()) {
      answer_purge(cid, seq, 200, "OK", counts + "}");
      return;
    }
    be->list_objects(ListQuery{r->variants, 0, {}}, this, [this, cid, seq, counts](ListResult m) {
      answer_purge(cid, seq, 200, "OK",
                   counts + ",\"variants\":" + std::to_string(m.ok ? (int64_t)m.matched : -1) + "}");
    });
  });
}

// GET /_shellac/objects (ProxyConfig::inspect): what is cached under ?prefix=, at ?key=, with
// one of ?tag=a,b, matching ?glob=PATTERN, or at all; &limit=N objects a page (default 100), &after=<the page
// before's "next">. Values are percent-decoded once. The cursor in "next" is written
// percent-encoded, so it goes into &after= as it is. Objects flagged as changed by the engine
// never reach here (the tier drops them).
void Reactor::on_inspect(Client* c, Slot* s, const std::string& qs) {
  const uint64_t cid = c->id, seq = s->seq;
  if (!purge_allowed(cfg_.inspect, c->loopback)) {
    answer_purge(cid, seq, 403, "Forbidden",
                 "{\"error\":\"inspection is allowed from loopback only\"}");
    return;
  }
  inspect_requests++;
  InspectParams p;
  if (!parse_inspect_query(qs, &p)) {
    answer_purge(cid, seq, 400, "Bad Request", "{\"error\":\"bad query\"}");
    return;
  }
  ListQuery q{KeyedSelector(), p.limit, p.after};
  const char* mode = "all";
  std::string bad;
  if (p.which == 1 || p.which == 2) {
    mode = p.which == 2 ? "key" : "prefix";
    q.what = p.which == 2 ? KeyedSelector::exact(p.value) : KeyedSelector::prefix(p.value);
    if (!q.what.valid()) bad = "{\"error\":\"empty or oversized pattern\"}";
  } else if (p.which == 3) {
    mode = "tag";
    q.what = KeyedSelector::tags(cfg_.tag_header.empty() ? std::vector<uint64_t>()
                                                         : tag_hashes_of(p.value));
    if (!q.what.valid()) bad = bad_tags(cfg_.tag_header.empty(), q.what);
  } else if (p.which == 4) {  // (the pattern as written: '*' the wildcard, '\\' escapes)
    mode = "glob";
    std::string why;
    q.what = KeyedSelector::glob(p.value, &why);
    if (!q.what.valid()) bad = bad_glob(why);
  }
  if (!bad.empty()) {
    answer_purge(cid, seq, 400, "Bad Request", bad);
    return;
  }
  CacheBackend* be = px_->backend_.get();
  if (!be || !px_->cfg_.cache_enabled) {
    answer_purge(cid, seq, 501, "Not Implemented", "{\"error\":\"no cache\"}");
    return;
  }
  const std::string m = mode;
  const bool grace = cfg_.grace != 0;
  be->list_objects(q, this, [this, cid, seq, m, grace](ListResult r) {
    if (r.bad_cursor) {
      answer_purge(cid, seq, 400, "Bad Request", "{\"error\":\"bad cursor\"}");
      return;
    }
    if (!r.ok) {
      answer_purge(cid, seq, 501, "Not Implemented",
                   "{\"mode\":\"" + m + "\",\"error\":\"the cache tier cannot scan its keys\"}");
      return;
    }
    std::string b = "{\"mode\":\"" + m + "\",\"matched\":" + std::to_string(r.matched) +
                    ",\"bytes\":" + std::to_string(r.bytes) +
                    ",\"listed\":" + std::to_string(r.objects.size()) + ",\"next\":";
    if (r.next.empty()) {
      b += "null";
    } else {
      b += '"';
      percent_encode(r.next, &b);
      b += '"';
    }
    b += ",\"shards_skipped\":" + std::to_string(r.shards_skipped) + ",\"objects\":[";
    const int64_t now = (int64_t)unix_now();
    bool first = true;
    for (const ListedObject& o : r.objects) {
      if (!first) b += ',';
      first = false;
      b += "{\"key\":\"";
      json_escape_key(o.key, &b);
      b += std::string("\",\"key_truncated\":") + (o.key_truncated ? "true" : "false") +
           ",\"size\":" + std::to_string(o.size) +
           ",\"ttl\":" + (o.ttl < 0 ? std::string("null") : std::to_string(o.ttl));
      if (grace) b += ",\"fresh_for\":" + std::to_string((int64_t)o.flags - now);
      b += ",\"tags\":" + std::to_string(o.ntags) +
           ",\"referenced\":" + (o.referenced ? "true" : "false") +
           ",\"shard\":" + std::to_string(o.shard) + "}";
    }
    answer_purge(cid, seq, 200, "OK", b + "]}");
  });
}

void Reactor::answer_purge(uint64_t cid, uint64_t seq, int code, const char* reason,
                           const std::string& body) {
  Client* c = find_client(cid);
  if (!c) return;
  Slot* s = find_slot(c, seq);
  if (!s || s->ready) return;
  complete_slot(c, s, std::make_shared<const std::string>(simple_response(
                          code, reason, cfg_.server_name, body + "\n", "application/json")));
}

void Reactor::on_cache(uint64_t cid, uint64_t seq, bool hit, CacheValue v) {
  Client* c = find_client(cid);
  if (!c) return;
  Slot* s = find_slot(c, seq);
  if (!s || s->ready) return;
  // A value stored behind a tag block (whether or not --tag-header is set now): everything
  // below sees the plain object, a zero-copy slice; `raw` is what a revalidation stores again
  Bytes raw;
  if (hit && v.data && v.data->size() && (uint8_t)v.data->data()[0] == kTagMarker) {
    const uint64_t* hs;
    unsigned nt;
    bool over;
    if (const size_t strip = parse_tag_block(v.data->data(), v.data->size(), &hs, &nt, &over)) {
      raw = v.data;
      v.data = raw.sub(strip, raw->size() - strip);
    }
  }
  if (hit && v.data && is_vary_marker(v.data->view())) {
    // the URL's responses Vary: look the variant of this request up under its own key
    // (a marker found by a variant lookup, or without the request, counts as a miss)
    if (cfg_.policy == "rfc" && !s->vary_probe && s->req) {
      s->key = vary_key(s->base_key, marker_names(v.data->view()), s->req->headers());
      s->d = digest_bytes(reinterpret_cast<const uint8_t*>(s->key.data()), s->key.size());
      s->vary_probe = true;
      if (cfg_.grace) s->vary_marker = v.data;
      px_->backend_->get(s->key, s->d, this, [this, cid, seq](bool h2, CacheValue v2) {
        on_cache(cid, seq, h2, std::move(v2));
      });
      return;
    }
    hit = false;
  }
  if (hit && v.data) {
    hits++;
    if (s->vary_probe) vary_hits++;
    // --conditional-hits with the whole object here (a tier's whole answer, a fallback, a
    // stale object): the same decision with the same functions, so every path answers alike
    bool not_modified = false;
    size_t head_len = 0;
    if ((s->cond.kind == kCondNoneMatch || s->cond.kind == kCondModifiedSince) &&
        slice_find_head_end(reinterpret_cast<const uint8_t*>(v.data->data()), v.data->size(),
                            &head_len)) {
      const SliceCond sc{s->cond.kind, s->cond.ncand, 0, (uint32_t)s->cond.records.size()};
      not_modified =
          cond_matches(reinterpret_cast<const uint8_t*>(v.data->data()), 0, (uint32_t)head_len, sc,
                       reinterpret_cast<const uint8_t*>(s->cond.records.data())) &&
          not_modified_exact(s, v.data->view().substr(0, head_len));
    }
    // --grace: past its freshness time (the flags word) the object is served stale, and
    // revalidated in the background (before deliver(): that gives the parsed request back)
    if (cfg_.grace && v.flags && unix_now() >= v.flags) {
      stale_served++;
      revalidate(s, v.data, raw);
    }
    if (not_modified) {
      answer_not_modified(c, s, v.data->view().substr(0, head_len));
      return;
    }
    deliver(c, s, v.data);
    return;
  }
  misses++;
  auto it = inflight_.find(s->key);
  if (it != inflight_.end()) {  // same object already being fetched: wait for it
    collapsed++;
    it->second.emplace_back(cid, seq);
    return;
  }
  inflight_[s->key];  // this request leads the fetch
  forward(c, s);
}

// ---- partial hits (ProxyConfig::partial_hits) -------------------------------------------
void Reactor::ask_part(Slot* s, uint64_t cid) {
  const uint64_t seq = s->seq;
  const auto done = [this, cid, seq](PartValue p) { on_part(cid, seq, std::move(p)); };
  if (s->cond.kind != kCondNone)
    px_->backend_->get_part_if(s->key, s->d, s->spec, s->cond, this, done);
  else
    px_->backend_->get_part(s->key, s->d, s->spec, this, done);
}

// Whether a 304 is the exact answer to the slot's matched condition for the stored head: the
// stored status is 200, and the object is not gzip-coded for a client without gzip under rfc.
bool Reactor::not_modified_exact(const Slot* s, std::string_view hv) const {
  const size_t sp = hv.find(' ');
  if (sp == std::string_view::npos || hv.substr(sp + 1, 3) != "200" ||
      (hv.size() > sp + 4 && hv[sp + 4] != ' ' && hv[sp + 4] != '\r'))
    return false;
  return s->client_gzip || cfg_.policy != "rfc" || !object_is_gzip(hv);
}

// 304 Not Modified from the stored head: the header lines a 304 carries (RFC 9110 15.4.5), no
// body and no Content-Length. It counts as a hit.
void Reactor::answer_not_modified(Client* c, Slot* s, std::string_view hv) {
  std::string out = "HTTP/1.1 304 Not Modified\r\nServer: " + cfg_.server_name + "\r\n";
  size_t pos = hv.find("\r\n");
  while (pos != std::string_view::npos && pos + 2 < hv.size()) {
    const size_t ls = pos + 2, le = hv.find("\r\n", ls);
    if (le == std::string_view::npos || le == ls) break;  // the blank line
    const std::string_view line = hv.substr(ls, le - ls);
    const std::string low = to_lower(std::string(line.substr(0, line.find(':'))));
    if (low == "cache-control" || low == "content-location" || low == "date" || low == "etag" ||
        low == "expires" || low == "last-modified" || low == "vary") {
      out.append(line);
      out += "\r\n";
    }
    pos = le;
  }
  out += "Connection: keep-alive\r\n\r\n";
  not_modified_304++;
  complete_slot(c, s, std::make_shared<const std::string>(std::move(out)));
}

// The tier's answer to a Range GET or a HEAD. Answered here: 206, 416, a HEAD's stored head.
// Everything else goes the way it goes without the option: a Range GET as a miss or, through
// a whole GET, as a hit (on_cache); a HEAD upstream, its response not cached.
void Reactor::on_part(uint64_t cid, uint64_t seq, PartValue p) {
  Client* c = find_client(cid);
  if (!c) return;
  Slot* s = find_slot(c, seq);
  if (!s || s->ready) return;
  const bool head_only = !s->lookup;  // a HEAD under policy rfc
  if (p.status == kSliceWholeObj && p.window && cfg_.policy == "rfc" && !s->vary_probe && s->req) {
    // the URL's Vary marker (behind a tag block or not): the variant is asked for the same way
    Bytes m = p.window;
    const uint64_t* hs;
    unsigned nt;
    bool over;
    if (const size_t strip = parse_tag_block(m->data(), m->size(), &hs, &nt, &over))
      m = m.sub(strip, m->size() - strip);
    if (is_vary_marker(m->view())) {
      s->key = vary_key(s->base_key, marker_names(m->view()), s->req->headers());
      s->d = digest_bytes(reinterpret_cast<const uint8_t*>(s->key.data()), s->key.size());
      s->vary_probe = true;
      if (cfg_.grace) s->vary_marker = m;
      ask_part(s, cid);
      return;
    }
  }
  const bool if_range = s->cond.kind == kCondIfRangeEtag || s->cond.kind == kCondIfRangeDate;
  if (if_range && p.status != kSliceMiss)
    (p.status == kSliceWholeObj ? if_range_failed : if_range_matched)++;
  if (p.status == kSliceNotModified && p.head && not_modified_exact(s, p.head->view()) &&
      !(cfg_.grace && p.flags && unix_now() >= p.flags)) {  // (stale: on_cache revalidates)
    hits++;
    if (s->vary_probe) vary_hits++;
    answer_not_modified(c, s, p.head->view());
    return;
  }
  if ((p.status == kSliceOk || p.status == kSliceUnsat) && (s->ranged || head_only) &&
      answer_part(c, s, p))
    return;
  // (a conditional request whose whole object came back was answered as it asked)
  if (p.status != kSliceMiss && !(p.status == kSliceWholeObj && s->cond.kind != kCondNone))
    partial_fallbacks++;
  if (head_only) {  // forwarded, as every HEAD is without the option
    s->key = s->base_key;
    forward(c, s);
    return;
  }
  if (p.status == kSliceMiss) {
    on_cache(cid, seq, false, CacheValue{});
  } else if (p.status == kSliceWholeObj) {  // the whole value is here already
    CacheValue v;
    v.data = std::move(p.window);
    v.flags = p.flags;
    v.ttl_left = p.ttl_left;
    on_cache(cid, seq, true, std::move(v));
  } else {
    px_->backend_->get(s->key, s->d, this, [this, cid, seq](bool hit, CacheValue v) {
      on_cache(cid, seq, hit, std::move(v));
    });
  }
}

// Answers the request from the stored head and the window if that is exact; false: it is not.
bool Reactor::answer_part(Client* c, Slot* s, const PartValue& p) {
  const std::string_view hv = p.head->view();
  const bool head_only = !s->lookup;
  // an object already stale under --grace needs the whole object (revalidate)
  if (cfg_.grace && p.flags && unix_now() >= p.flags) return false;
  if (!object_header(hv, "transfer-encoding:").empty()) return false;
  const std::string cl = object_header(hv, "content-length:");
  if (cl.empty() || cl.find_first_not_of("0123456789") != std::string::npos ||
      std::strtoull(cl.c_str(), nullptr, 10) != p.body_len)
    return false;
  if (!head_only) {
    // "HTTP/1.x 200 ..."
    const size_t sp = hv.find(' ');
    if (sp == std::string_view::npos || hv.substr(sp + 1, 3) != "200" ||
        (hv.size() > sp + 4 && hv[sp + 4] != ' ' && hv[sp + 4] != '\r'))
      return false;
    if (!s->client_gzip && cfg_.policy == "rfc" && object_is_gzip(hv)) return false;
  }
  hits++;
  if (s->vary_probe) vary_hits++;
  if (head_only) {
    head_hits++;
    complete_slot(c, s, p.head);
    return true;
  }
  if (p.status == kSliceUnsat) {
    range_416++;
    complete_slot(c, s, std::make_shared<const std::string>(
                            "HTTP/1.1 416 Range Not Satisfiable\r\nServer: " + cfg_.server_name +
                            "\r\nContent-Range: bytes */" + std::to_string(p.body_len) +
                            "\r\nContent-Length: 0\r\nConnection: keep-alive\r\n\r\n"));
    return true;
  }
  // 206: the stored header lines, the window's length and where it lies
  std::string out = "HTTP/1.1 206 Partial Content\r\n";
  out.reserve(hv.size() + 96);
  size_t pos = hv.find("\r\n");
  while (pos != std::string_view::npos && pos + 2 < hv.size()) {
    const size_t ls = pos + 2, le = hv.find("\r\n", ls);
    if (le == std::string_view::npos || le == ls) break;  // the blank line
    const std::string_view line = hv.substr(ls, le - ls);
    const std::string low = to_lower(std::string(line.substr(0, line.find(':'))));
    if (low != "content-length" && low != "content-range") {
      out.append(line);
      out += "\r\n";
    }
    pos = le;
  }
  const uint64_t len = p.window ? p.window->size() : 0;
  out += "Content-Length: " + std::to_string(len) + "\r\nContent-Range: bytes " +
         std::to_string(p.first) + "-" + std::to_string(p.first + len - 1) + "/" +
         std::to_string(p.body_len) + "\r\n\r\n";
  range_206++;
  complete_slot(c, s, std::make_shared<const std::string>(std::move(out)), p.window);
  return true;
}

// The last response on a connection announces the close (cached objects carry
// "Connection: keep-alive" from the fill, Server.py:414-415).
static Bytes with_connection_close(const Bytes& obj) {
  const std::string_view ov = obj.view();
  const size_t eoh = ov.find("\r\n\r\n");
  if (eoh == std::string::npos) return obj;
  std::string head(ov.substr(0, eoh + 2));
  std::string out;
  out.reserve(obj->size() + 8);
  size_t pos = 0;
  while (pos < head.size()) {
    size_t e = head.find("\r\n", pos);
    if (e == std::string::npos) e = head.size();
    const std::string line = head.substr(pos, e - pos);
    const std::string low = to_lower(line.substr(0, line.find(':')));
    if (pos == 0 || (low != "connection" && low != "keep-alive")) {
      out += line;
      out += "\r\n";
    }
    pos = e + 2;
  }
  out += "Connection: close\r\n\r\n";
  out.append(ov.substr(eoh + 4));
  return std::make_shared<const std::string>(std::move(out));
}

// A cached (or just fetched) object to one client: under policy rfc a gzip-coded object
// goes to a client without `Accept-Encoding: gzip` as its identity variant.
void Reactor::deliver(Client* c, Slot* s, Bytes obj) {
  if (obj && !s->client_gzip && !s->head && cfg_.policy == "rfc" && object_is_gzip(obj->view())) {
    if (px_->gzip_ && px_->gzip_->can_inflate()) {
      // the GPU gzip service inflates it in a batch (zlib on its thread as the fallback);
      // the slot completes on this reactor when it returns, if the client is still there
      auto rp = std::make_shared<HttpParser>(false);
      rp->parse(obj->data(), obj->size());
      if (rp->message_complete() || rp->finish()) {
        std::string member = std::move(rp->mutable_body());
        const uint64_t cid = c->id, seq = s->seq;
        px_->gzip_->submit_inflate(
            std::move(member), cfg_.max_inflate_bytes,
            [this, rp, cid, seq](bool ok, std::string out) {
              post([this, rp, cid, seq, ok, out = std::move(out)]() mutable {
                Client* c2 = find_client(cid);
                Slot* s2 = c2 ? find_slot(c2, seq) : nullptr;
                if (!s2 || s2->ready) return;
                if (!ok) {
                  errors++;
                  complete_slot(c2, s2, std::make_shared<const std::string>(simple_response(
                                            502, "Bad Gateway", cfg_.server_name,
                                            "undecodable gzip object\n")));
                  return;
                }
                rp->remove_header("content-encoding");
                rp->mutable_body() = std::move(out);
                identity_decoded++;
                gzip_gpu_inflated++;
                complete_slot(c2, s2, std::make_shared<const std::string>(rp->serialize()));
              });
            });
        return;
      }
    }
    Bytes id = identity_variant(obj, cfg_.max_inflate_bytes);
    if (!id) {
      errors++;
      complete_slot(c, s, std::make_shared<const std::string>(simple_response(
                              502, "Bad Gateway", cfg_.server_name, "undecodable gzip object\n")));
      return;
    }
    identity_decoded++;
    obj = std::move(id);
  }
  complete_slot(c, s, std::move(obj));
}

void Reactor::complete_slot(Client* c, Slot* s, Bytes data, Bytes tail) {
  if (s->req) give_parser(std::move(s->req));
  if (s->close_after && data) data = with_connection_close(data);
  s->out.write_shared(std::move(data));
  if (tail && tail->size()) s->out.write_shared(std::move(tail));
  s->out.close();
  s->ready = true;
  const double us = (now_s() - s->t0) * 1e6;
  const int b = us < 1 ? 0 : std::min(kHistBuckets - 1, 1 + (int)std::log2(us));
  hist[b]++;
  flush_client(c);
}

void Reactor::flush_client(Client* c) {
  // Head-of-line ordered write of every *ready* response slot (Server.py:236-239),
  // many pipelined responses per writev.
  if (c->dead) return;
  for (;;) {
    iovec iov[64];
    int cnt = 0;
    size_t want = 0;
    for (auto& s : c->slots) {
      if (!(s->ready || s->streaming) || cnt >= 64) break;
      const int k = s->out.iov(iov + cnt, 64 - cnt);
      for (int j = 0; j < k; ++j) want += iov[cnt + j].iov_len;
      cnt += k;
      if (!s->ready) break;  // a response still streaming holds back its successors
    }
    if (cnt == 0) break;
    const ssize_t w = writev(c->fd, iov, cnt);
    if (w < 0) {
      if (errno == EAGAIN || errno == EWOULDBLOCK) {
        arm(c, true);
        return;
      }
      if (errno == ECONNRESET || errno == EPIPE) client_resets++;
      else errors++;
      close_client(c);
      return;
    }
    bytes_out += (uint64_t)w;
    c->atime = now_s();
    size_t left = (size_t)w;
    while (!c->slots.empty() && (c->slots.front()->ready || c->slots.front()->streaming)) {
      Slot* s = c->slots.front().get();
      const size_t take = std::min<size_t>(left, s->out.pending());
      s->out.ack(take);
      left -= take;
      if (!s->out.complete()) break;
      const bool last = s->close_after;
      if (s->stream_up) resume_stream(s->stream_up);
      c->slots.pop_front();
      if (last) {  // "Connection: close" / max requests reached / bad request
        close_client(c);
        return;
      }
    }
    if (!c->slots.empty()) {
      Slot* f = c->slots.front().get();
      if (f->streaming && f->stream_up && f->out.pending() < cfg_.stream_high_water / 4)
        resume_stream(f->stream_up);
    }
    if ((size_t)w < want) {
      arm(c, true);
      return;
    }
  }
  if (c->eof && c->slots.empty()) {
    close_client(c);
    return;
  }
  arm(c, false);
}

void Reactor::close_client(Client* c) {
  if (c->dead) return;
  c->dead = true;
  epoll_ctl(epfd_, EPOLL_CTL_DEL, c->fd, nullptr);
  close(c->fd);
  conns_.erase(c->id);
  clients--;
  if (c->up) {
    // release the pooled upstream (Server.py:189-192); its in-flight responses
    // still complete and fill the cache
    if (c->up->owner == c) c->up->owner = nullptr;
    c->up = nullptr;
  }
  for (auto& s : c->slots)  // a stream paused for this client drains (and is dropped)
    if (s->stream_up) resume_stream(s->stream_up);
  graveyard_.push_back(c);
}

// ---------------------------------------------------------------------------------
// upstream side
// ---------------------------------------------------------------------------------
int Reactor::choose_server() {
  const int n = (int)cfg_.upstreams.size();
  if (n == 0) return -1;
  const double t = now_s();
  std::vector<int> up;
  for (int i = 0; i < n; ++i)
    if (px_->upstream_up(i, t)) up.push_back(i);
  if (up.empty()) return -1;
  if (cfg_.balance == "roundrobin") return up[(size_t)px_->next_rr() % up.size()];
  if (cfg_.balance == "leastconn") {
    std::vector<int> load(n, 0);
    for (Upstream* u : pool_) load[u->server] += (int)u->pend.size() + (u->owner ? 1 : 0);
    int best = up[0];
    for (int i : up)
      if (load[i] < load[best]) best = i;
    return best;
  }
  return up[std::uniform_int_distribution<size_t>(0, up.size() - 1)(rng_)];  // Server.py:123
}

Upstream* Reactor::pick_upstream(Client* c) {
  const double t = now_s();
  auto valid = [&](Upstream* u) {
    if (u->dead || !px_->upstream_healthy(u->server)) return false;
    if (u->count >= u->ka_max) return false;
    return u->ka_timeout < 0 || t - u->atime < u->ka_timeout;
  };
  if (c->up && valid(c->up)) return c->up;  // affinity (Server.py:94-101)
  if (c->up) {
    if (c->up->owner == c) c->up->owner = nullptr;
    c->up = nullptr;
  }
  for (Upstream* u : pool_) {  // reuse a free pooled connection (Server.py:103-116)
    if (!u->owner && valid(u) && px_->upstream_up(u->server, t)) {
      u->owner = c;
      c->up = u;
      return u;
    }
  }
  Upstream* u = connect_upstream();
  if (u) {
    u->owner = c;
    c->up = u;
  }
  return u;
}

Upstream* Reactor::connect_upstream() {
  const double t = now_s();
  for (int attempt = 0; attempt < (int)cfg_.upstreams.size() + 1; ++attempt) {
    const int srv = choose_server();
    if (srv < 0) return nullptr;
    const int fd = connect_nonblock(cfg_.upstreams[srv]);  // non-blocking (ref blocks, :126)
    if (fd < 0) {
      px_->upstream_failed(srv, t);
      upstream_failures++;
      continue;
    }
    auto* u = new Upstream();
    if (server_nka_[srv]) u->ka_max = 1;
    u->fd = fd;
    u->kind = 1;
    u->id = next_id_++;
    u->server = srv;
    u->ctime = u->atime = t;
    conns_[u->id] = u;
    pool_.push_back(u);
    epoll_event ev{};
    ev.events = EPOLLIN | EPOLLRDHUP | EPOLLOUT;
    ev.data.u64 = u->id;
    epoll_ctl(epfd_, EPOLL_CTL_ADD, fd, &ev);
    u->out_armed = true;
    upstreams++;
    return u;
  }
  return nullptr;
}

// The request as forwarded upstream: gzip forced (Server.py:358), hop-by-hop headers
// dropped, the upstream connection kept alive for the pool.
std::string Reactor::upstream_request(HttpParser& q) {
  q.set_header("accept-encoding", "gzip");
  q.remove_header("proxy-connection");
  q.remove_header("keep-alive");
  q.set_header("connection", "keep-alive");
  return q.serialize();
}

std::unique_ptr<HttpParser> Reactor::take_parser() {
  if (parser_pool_.empty()) return std::make_unique<HttpParser>(true);
  auto p = std::move(parser_pool_.back());
  parser_pool_.pop_back();
  return p;
}

void Reactor::give_parser(std::unique_ptr<HttpParser> p) {
  if (!p || parser_pool_.size() >= 4096) return;
  p->reset();
  parser_pool_.push_back(std::move(p));
}

void Reactor::forward(Client* c, Slot* s) {
  s->attempts++;
  if (s->fwd.empty() && s->req) {
    if (s->lookup && cfg_.policy == "rfc")  // a Vary'd response is keyed by these
      s->req_headers = std::make_shared<const std::vector<Header>>(s->req->headers());
    s->fwd = upstream_request(*s->req);
    give_parser(std::move(s->req));
  }
  Upstream* u = pick_upstream(c);
  if (!u) {
    complete_slot(c, s, std::make_shared<const std::string>(simple_response(
                            503, "Service Unavailable", cfg_.server_name, "no upstream available\n")));
    return;
  }
  u->out.write(s->fwd);
  u->pend.push_back(Pend{c->id, s->seq, s->key, s->d, s->lookup, s->head, s->client_gzip,
                        s->base_key, s->req_headers, px_->purge_generation()});
  u->count++;
  upstream_reqs++;
  flush_upstream(u);
}

// ---- grace and revalidation (ProxyConfig::grace) --------------------------------------
// Seconds a response may be served past its TTL: the configured grace, or under policy rfc
// the response's own stale-while-revalidate / stale-if-error (the larger; 0: none).
uint32_t Reactor::grace_for(const HttpParser& r) const {
  if (!cfg_.grace) return 0;
  if (cfg_.policy != "rfc") return cfg_.grace;
  const std::string* cc = r.header("cache-control");
  const long swr = cc_seconds(cc, "stale-while-revalidate="), sie = cc_seconds(cc, "stale-if-error=");
  if (swr < 0 && sie < 0) return cfg_.grace;
  return (uint32_t)std::max<long>(std::max(swr, sie), 0);
}

// A stale hit starts the key's background revalidation unless one (or a miss's fetch) is
// already under way on this reactor — the waiters table collapses them, and later stale
// hits are simply served stale — or the last one failed less than upstream_retry_s ago.
// The request is the client's own (so a Vary'd variant is asked for with its headers), made
// conditional on the stored object's validators; it holds no client slot.
void Reactor::revalidate(Slot* s, const Bytes& stale, const Bytes& raw) {
  if (!s->req || s->req->method() != "GET" || inflight_.count(s->key)) return;
  const double t = now_s();
  const auto back = reval_retry_at_.find(s->key);
  if (back != reval_retry_at_.end()) {
    if (t < back->second) return;
    reval_retry_at_.erase(back);
  }
  HttpParser& q = *s->req;
  Pend p{0, 0, s->key, s->d, true, false, true, s->base_key, nullptr, px_->purge_generation()};
  if (cfg_.policy == "rfc")
    p.req_headers = std::make_shared<const std::vector<Header>>(q.headers());
  p.reval = true;
  p.stale = stale;
  p.stale_raw = raw;
  p.marker = s->vary_marker;
  // the stored validators replace whatever conditions the client sent
  for (const char* h : {"if-none-match", "if-modified-since", "if-match", "if-unmodified-since",
                        "if-range", "range"})
    q.remove_header(h);
  const std::string etag = object_header(stale->view(), "etag:");
  const std::string lm = object_header(stale->view(), "last-modified:");
  if (!etag.empty()) q.set_header("if-none-match", etag);
  if (!lm.empty()) q.set_header("if-modified-since", lm);
  const std::string fwd = upstream_request(q);
  revalidations++;
  Upstream* u = nullptr;
  for (Upstream* x : pool_)  // an idle pooled connection, else a new one
    if (!x->owner && x->pend.empty() && !x->dead && px_->upstream_healthy(x->server) &&
        px_->upstream_up(x->server, t) && x->count < x->ka_max &&
        (x->ka_timeout < 0 || t - x->atime < x->ka_timeout)) {
      u = x;
      break;
    }
  if (!u) u = connect_upstream();
  if (!u) {
    revalidation_failed(p);
    return;
  }
  inflight_[s->key];  // misses of the key that arrive meanwhile wait for the answer
  u->out.write(fwd);
  u->pend.push_back(std::move(p));
  u->count++;
  upstream_reqs++;
  flush_upstream(u);
}

// The origin failed the revalidation (no upstream, connect failure, a dead connection or a
// 5xx): nothing is stored, the stale object stays servable until its hard expiry
// (stale-if-error), and the key is not tried again for upstream_retry_s.
void Reactor::revalidation_failed(const Pend& p) {
  revalidate_errors++;
  if (reval_retry_at_.size() > 4096) reval_retry_at_.clear();
  reval_retry_at_[p.key] = now_s() + cfg_.upstream_retry_s;
  release_waiters(p.key, nullptr);  // misses that queued behind it fetch for themselves
}

// 304: the stored object is good for another (ttl, grace) — from the 304's Cache-Control
// when it has one — and is extended in place; a tier that cannot touch (memcached), or that
// lost the object meanwhile, gets the stale object stored again. The stored headers are not
// rewritten from the 304. A PURGE of the key since the request left wins: nothing is touched.
// 5xx: a failure.
void Reactor::revalidation_answered(HttpParser& r, const Pend& p) {
  if (r.status() != 304) {
    revalidation_failed(p);
    return;
  }
  revalidated_304++;
  // (the stored object's tags: a 304's own tag header is ignored, as its other headers are)
  std::vector<uint64_t> tags;
  bool tagged = false, over = false;
  if (p.stale_raw) {
    const uint64_t* hs;
    unsigned nt;
    tagged = parse_tag_block(p.stale_raw->data(), p.stale_raw->size(), &hs, &nt, &over) != 0;
    for (unsigned i = 0; i < nt; ++i) tags.push_back(tag_block_hash(hs, i));
  }
  if (px_->purged_since(p.purge_gen, p.key, p.base_key, tagged ? &tags : nullptr, over)) {
    fills_purged++;
    release_waiters(p.key, nullptr);
    return;
  }
  uint32_t ttl = cfg_.ttl;
  const long ma = cfg_.policy == "rfc" ? cc_max_age(r.header("cache-control")) : -1;
  if (ma > 0) ttl = (uint32_t)ma;
  const uint32_t grace = grace_for(r), hard = ttl + grace;
  const uint32_t fresh_until = grace ? unix_now() + ttl : 0;
  CacheBackend* be = px_->backend_.get();
  const auto extend = [this, be, hard, fresh_until](const std::string& key, const Digest& d,
                                                     const Bytes& obj, bool count) {
    be->touch(key, d, hard, &fresh_until, this, [this, be, key, d, obj, hard, fresh_until,
                                                  count](int st) {
      if (st == 1) {
        if (count) revalidate_touched++;
        return;
      }
      be->set(key, d, obj, fresh_until, hard);
      if (count) revalidate_restored++;
    });
  };
  if (p.marker && p.key != p.base_key)
    extend(p.base_key, digest_bytes(reinterpret_cast<const uint8_t*>(p.base_key.data()),
                                    p.base_key.size()), p.marker, false);
  extend(p.key, p.d, p.stale_raw ? p.stale_raw : p.stale, true);  // (stored with its tag block)
  reval_retry_at_.erase(p.key);
  release_waiters(p.key, p.stale);
}

void Reactor::flush_upstream(Upstream* u) {
  if (u->dead) return;
  if (!u->connected) {
    arm(u, true);
    return;
  }
  while (u->out.pending()) {
    iovec iov[64];
    const int cnt = u->out.iov(iov, 64);
    const ssize_t w = writev(u->fd, iov, cnt);
    if (w < 0) {
      if (errno == EAGAIN || errno == EWOULDBLOCK) {
        arm(u, true);
        return;
      }
      close_upstream(u);
      return;
    }
    u->out.ack((uint64_t)w);
    u->atime = now_s();
  }
  u->out.release_acked();
  arm(u, false);
}

void Reactor::release_waiters(const std::string& key, Bytes obj) {
  auto it = inflight_.find(key);
  if (it == inflight_.end()) return;
  std::vector<std::pair<uint64_t, uint64_t>> waiters;
  waiters.swap(it->second);
  inflight_.erase(it);
  for (auto& w : waiters) {
    Client* c = find_client(w.first);
    if (!c) continue;
    Slot* s = find_slot(c, w.second);
    if (!s || s->ready) continue;
    if (obj) {
      hits++;
      deliver(c, s, obj);
    } else {
      forward(c, s);  // uncacheable ("hit-for-pass"): each waiter fetches its own copy
    }
  }
}

void Reactor::fail_pend(Pend& p, int code, const char* reason) {
  if (p.reval) {  // no client to answer and no retry: the next stale hit tries again
    revalidation_failed(p);
    return;
  }
  if (p.lookup && code != 502) release_waiters(p.key, nullptr);
  Client* c = find_client(p.client_id);
  if (!c) {
    if (p.lookup) release_waiters(p.key, nullptr);
    return;
  }
  Slot* s = find_slot(c, p.seq);
  if (!s || s->ready) return;
  if (s->attempts < 3 && code == 502) {  // idempotent retry on another connection
    retries++;
    if (c->up && c->up->dead) c->up = nullptr;
    forward(c, s);
    return;
  }
  if (p.lookup) release_waiters(p.key, nullptr);
  complete_slot(c, s, std::make_shared<const std::string>(
                          simple_response(code, reason, cfg_.server_name, "upstream failed\n")));
}

void Reactor::on_upstream(Upstream* u, uint32_t ev) {
  if ((ev & EPOLLOUT) && !u->connected) {
    int err = 0;
    socklen_t el = sizeof err;
    getsockopt(u->fd, SOL_SOCKET, SO_ERROR, &err, &el);
    if (err) {
      px_->upstream_failed(u->server, now_s());
      upstream_failures++;
      close_upstream(u);
      return;
    }
    u->connected = true;
  }
  if (ev & EPOLLOUT) flush_upstream(u);
  if (u->dead) return;
  if (!(ev & (EPOLLIN | EPOLLRDHUP | EPOLLHUP | EPOLLERR))) return;
  for (;;) {
    const ssize_t r = recv(u->fd, buf_.data(), buf_.size(), 0);
    if (r > 0) {
      u->atime = now_s();
      const char* p = buf_.data();
      size_t n = (size_t)r;
      while (n > 0 && !u->dead) {
        if (u->pend.empty()) {  // unsolicited bytes: protocol error
          close_upstream(u);
          return;
        }
        if (!u->resp) {
          u->resp = std::make_unique<HttpParser>(cfg_.decode_gzip);
          u->resp->set_max_decoded_bytes(cfg_.max_inflate_bytes);
          u->resp->set_no_body(u->pend.front().head);
          u->resp->set_eof_body(true);
        }
        const size_t used = u->resp->parse(p, n);
        p += used;
        n -= used;
        if (u->resp->error()) {
          close_upstream(u);
          return;
        }
        if (u->resp->message_complete()) {
          on_upstream_response(u);
          if (u->dead) return;
        } else if (u->resp->headers_complete() && maybe_stream(u)) {
          stream_out(u, std::move(u->resp->mutable_body()), false);
          u->resp->mutable_body().clear();
          if (used == 0) break;
        } else if (used == 0) {
          break;
        }
      }
      if ((size_t)r < buf_.size()) return;
      continue;
    }
    if (r == 0) {
      if (u->resp && u->resp->finish() && !u->pend.empty()) on_upstream_response(u);
      close_upstream(u);
      return;
    }
    if (errno == EAGAIN || errno == EWOULDBLOCK) return;
    close_upstream(u);
    return;
  }
}

bool Reactor::cacheable_response(const HttpParser& r, uint32_t* ttl) const {
  *ttl = cfg_.ttl;
  if (cfg_.policy == "reference") return true;  // Server.py:431-432 caches everything
  switch (r.status()) {
    case 200: case 203: case 204: case 300: case 301: case 404: case 405: case 410: case 414:
    case 501:
      break;
    default:
      return false;
  }
  const std::string* cc = r.header("cache-control");
  if (contains_ci(cc, "no-store") || contains_ci(cc, "private") || contains_ci(cc, "no-cache"))
    return false;
  if (r.header("set-cookie")) return false;
  const long ma = cc_max_age(cc);
  if (ma == 0) return false;
  if (ma > 0) *ttl = (uint32_t)ma;
  return true;
}

void Reactor::on_upstream_response(Upstream* u) {
  Pend p = std::move(u->pend.front());
  u->pend.pop_front();
  std::unique_ptr<HttpParser> rp = std::move(u->resp);
  HttpParser& r = *rp;
  const bool ka = r.keep_alive();
  const auto kap = r.keep_alive_params();
  responses++;
  if (u->streaming) {  // tail of a streamed response: nothing is cached
    u->pend.push_front(std::move(p));
    stream_out(u, std::move(r.mutable_body()), true);
    p = std::move(u->pend.front());
    u->pend.pop_front();
    u->streaming = false;
    if (p.lookup) release_waiters(p.key, nullptr);
    if (!ka) {
      server_nka_[u->server] = 1;
      close_upstream(u);
      return;
    }
    server_nka_[u->server] = 0;
    u->ka_timeout = kap.first;
    u->ka_max = kap.second;
    return;
  }
  if (p.reval && (r.status() == 304 || r.status() >= 500)) {
    // a background revalidation's 304 or failure (any other answer is a fill like a miss's)
    revalidation_answered(r, p);
    if (!ka) {
      server_nka_[u->server] = 1;
      close_upstream(u);
      return;
    }
    server_nka_[u->server] = 0;
    u->ka_timeout = kap.first;
    u->ka_max = kap.second;
    return;
  }
  rewrite_response_headers(r);
  const std::string* ce = r.header("content-encoding");
  bool deferred = false;
  // -z: under rfc the stored variant is gzip whichever client leads the fetch (a client
  // without gzip gets the identity variant from deliver()); the reference policy keeps
  // compressing only for gzip clients
  if (cfg_.compress && !ce && (p.client_gzip || cfg_.policy == "rfc") && r.body().size() >= 256) {
    const std::string* ct = r.header("content-type");
    if (ct && (contains_ci(ct, "text/") || contains_ci(ct, "json") || contains_ci(ct, "javascript") ||
               contains_ci(ct, "xml"))) {
      if (px_->gzip_) {
        // GPU: the body joins the current batch window; the response completes (cache
        // store, client slot, collapsed waiters) on this reactor when the batch returns.
        // Keep-alive bookkeeping of the upstream below does not wait for it.
        std::shared_ptr<HttpParser> rs(std::move(rp));
        auto ps = std::make_shared<Pend>(std::move(p));
        std::string body = std::move(rs->mutable_body());
        px_->gzip_->submit(std::move(body), [this, rs, ps](bool ok, std::string out) {
          post([this, rs, ps, ok, out = std::move(out)]() mutable {
            rs->mutable_body() = std::move(out);
            if (ok) {
              rs->set_header("content-encoding", "gzip");
              rs->set_header("vary", "Accept-Encoding");
              gzip_gpu_bodies++;
            }
            finish_response(*rs, *ps);
          });
        });
        deferred = true;
      } else {
        r.mutable_body() = gzip_compress(r.body(), 6);
        r.set_header("content-encoding", "gzip");
        r.set_header("vary", "Accept-Encoding");
      }
    }
  }
  if (!deferred) finish_response(r, p);
  if (!ka) {
    server_nka_[u->server] = 1;
    close_upstream(u);  // remaining pipelined requests are retried elsewhere
    return;
  }
  server_nka_[u->server] = 0;
  u->ka_timeout = kap.first;
  u->ka_max = kap.second;
}

// Cache store, client slot and collapsed waiters of a complete upstream response.
void Reactor::finish_response(HttpParser& r, const Pend& p) {
  Bytes obj;
  const bool rfc = cfg_.policy == "rfc";
  std::vector<std::string> vnames;
  if (rfc && !p.head) {
    vnames = vary_names(r);
    // one cache entry serves both codings: say so to downstream caches
    if (r.header("content-encoding") && !contains_ci(r.header("vary"), "accept-encoding")) {
      const std::string* v = r.header("vary");
      r.set_header("vary", v ? *v + ", Accept-Encoding" : std::string("Accept-Encoding"));
    }
  }
  if (p.head) {
    const std::string* cl = r.header("content-length");
    const uint64_t len = cl ? std::strtoull(cl->c_str(), nullptr, 10) : 0;
    obj = std::make_shared<const std::string>(r.serialize_head(len, cl != nullptr));
  } else {
    obj = std::make_shared<const std::string>(r.serialize());
  }
  uint32_t ttl = cfg_.ttl;
  bool cached = false, waiters_share = true;
  if (p.lookup && !p.head && cacheable_response(r, &ttl)) {
    // --grace: kept `grace` seconds past the TTL, the flags word says when it stops being
    // fresh (0 with grace off: stored exactly as without the option)
    const uint32_t grace = grace_for(r), hard_ttl = ttl + grace;
    const uint32_t fresh_until = grace ? unix_now() + ttl : 0;
    // --tag-header: the response's tags; the stored value is the tag block, then the object
    std::vector<uint64_t> tags;
    const std::string* th = cfg_.tag_header.empty() ? nullptr : r.header(cfg_.tag_header);
    if (th) tags = tag_hashes_of(*th);
    const bool tagged = !tags.empty(), over = tags.size() > kMaxObjectTags;
    Bytes stored = obj;
    if (tagged) {
      auto v = std::make_shared<std::string>(tag_block_size(tags.size()), '\0');
      write_tag_block(reinterpret_cast<uint8_t*>(&(*v)[0]), tags.data(), tags.size());
      v->append(obj->data(), obj->size());
      stored = std::shared_ptr<const std::string>(std::move(v));
    }
    if (px_->purged_since(p.purge_gen, p.key, p.base_key, tagged ? &tags : nullptr, over)) {
      // fetched before a purge of this key (or of one of its tags): delivered (the collapsed
      // waiters share it as they would have), not stored
      fills_purged++;
      cached = true;
      if (!vnames.empty())
        waiters_share = vnames[0] != "*" && p.req_headers &&
                        p.key == vary_key(p.base_key, vnames, *p.req_headers);
    } else if (vnames.empty()) {
      cached = true;
      // Server.py:432 mc.set(key, obj, time=ttl)
      px_->backend_->set(p.key, p.d, stored, fresh_until, hard_ttl);
      cache_sets++;
      if (tagged) tagged_fills++;
    } else if (vnames[0] != "*" && p.req_headers) {
      // Vary: marker under the URL key, the object under this request's variant key
      const std::string vk = vary_key(p.base_key, vnames, *p.req_headers);
      std::string marker = kVaryMarker;
      for (size_t i = 0; i < vnames.size(); ++i) marker += (i ? "," : "") + vnames[i];
      const Digest bd = digest_bytes(reinterpret_cast<const uint8_t*>(p.base_key.data()),
                                     p.base_key.size());
      const Digest vd = digest_bytes(reinterpret_cast<const uint8_t*>(vk.data()), vk.size());
      px_->backend_->set(p.base_key, bd, std::make_shared<const std::string>(std::move(marker)),
                         fresh_until, hard_ttl);
      px_->backend_->set(vk, vd, stored, fresh_until, hard_ttl);  // (the marker gets no block)
      cache_sets++;
      if (tagged) tagged_fills++;
      vary_stored++;
      cached = true;
      // requests collapsed onto the URL key may carry other header values: they fetch
      // their own variant; those collapsed onto this variant key share it
      waiters_share = p.key == vk;
    }  // Vary: * (or no request headers kept): not cacheable
  }
  if (Client* c = find_client(p.client_id)) {
    if (Slot* s = find_slot(c, p.seq)) {
      if (!s->ready) deliver(c, s, obj);
    }
  }
  if (p.lookup) release_waiters(p.key, cached && waiters_share ? obj : nullptr);
}

void Reactor::rewrite_response_headers(HttpParser& r) {
  // header rewrite (Server.py:412-416)
  r.set_header("server", cfg_.server_name);
  r.set_header("keep-alive", "timeout=5, max=100");
  r.set_header("connection", "keep-alive");
  if (!cfg_.partial_hits) r.remove_header("accept-ranges");  // (with it, ranges are served)
}

bool Reactor::maybe_stream(Upstream* u) {
  if (u->streaming) return true;
  HttpParser& r = *u->resp;
  const Pend& p = u->pend.front();
  if (p.head || p.reval || r.body_decoded()) return false;  // (a revalidation has no client)
  const int64_t cl = r.content_length();
  const bool big = (!r.chunked() && cl >= 0 && (uint64_t)cl > cfg_.stream_bytes) ||
                   r.body().size() > cfg_.stream_bytes;
  if (!big) return false;
  Client* c = find_client(p.client_id);
  Slot* s = c ? find_slot(c, p.seq) : nullptr;
  u->streaming = true;
  u->stream_chunked = r.chunked() || cl < 0;
  streamed++;
  rewrite_response_headers(r);
  if (s && s->close_after) r.set_header("connection", "close");
  std::string head;
  if (u->stream_chunked) {
    head = r.serialize_head(0, false);
    head.insert(head.size() - 2, "Transfer-Encoding: chunked\r\n");
  } else {
    head = r.serialize_head((uint64_t)cl, true);
  }
  stream_out(u, std::move(head), false);
  return true;
}

// Append streamed bytes to the front request's client slot (`last` ends the response).
// Body pieces are re-framed as chunks when the length is unknown.
void Reactor::stream_out(Upstream* u, std::string data, bool last) {
  const Pend& p = u->pend.front();
  Client* c = find_client(p.client_id);
  Slot* s = c ? find_slot(c, p.seq) : nullptr;
  if (!s || s->ready) return;  // client gone: drain and drop
  const bool is_head = !s->streaming;
  std::string framed;
  if (!is_head && u->stream_chunked) {
    if (!data.empty()) {
      char hx[24];
      std::snprintf(hx, sizeof hx, "%zx\r\n", data.size());
      framed = hx;
      framed += data;
      framed += "\r\n";
    }
    if (last) framed += "0\r\n\r\n";
  } else {
    framed = std::move(data);
  }
  s->streaming = true;
  s->stream_up = u->id;
  if (!framed.empty()) s->out.write_shared(std::make_shared<const std::string>(std::move(framed)));
  if (last) {
    s->out.close();
    s->ready = true;
    const double us = (now_s() - s->t0) * 1e6;
    const int b = us < 1 ? 0 : std::min(kHistBuckets - 1, 1 + (int)std::log2(us));
    hist[b]++;
  }
  flush_client(c);
  if (!last && !c->dead && s->out.pending() > cfg_.stream_high_water && !u->in_paused) {
    stream_pauses++;
    pause_input(u, true);
  }
}

void Reactor::resume_stream(uint64_t up_id) {
  auto it = conns_.find(up_id);
  if (it != conns_.end() && !it->second->dead && it->second->in_paused)
    pause_input(it->second, false);
}

void Reactor::close_upstream(Upstream* u) {
  if (u->dead) return;
  u->dead = true;
  epoll_ctl(epfd_, EPOLL_CTL_DEL, u->fd, nullptr);
  close(u->fd);
  conns_.erase(u->id);
  upstreams--;
  pool_.erase(std::remove(pool_.begin(), pool_.end(), u), pool_.end());
  if (u->owner && u->owner->up == u) u->owner->up = nullptr;
  u->owner = nullptr;
  std::deque<Pend> pend;
  pend.swap(u->pend);
  graveyard_.push_back(u);
  if (u->streaming && !pend.empty()) {  // bytes already left: the client cannot be answered
    u->streaming = false;
    Pend p = std::move(pend.front());
    pend.pop_front();
    if (p.lookup) release_waiters(p.key, nullptr);
    if (Client* c = find_client(p.client_id)) close_client(c);
  }
  for (auto& p : pend) fail_pend(p, 502, "Bad Gateway");
}

void Reactor::gc() {
  // Client keep-alive policy (Server.py:155-166): idle timeout / max requests.
  const double t = now_s();
  std::vector<Client*> idle;
  std::vector<Upstream*> stale;
  for (auto& kv : conns_) {
    Conn* c = kv.second;
    if (c->dead) continue;
    if (c->kind == 0) {
      auto* cl = static_cast<Client*>(c);
      if (cl->slots.empty() &&
          (t - cl->atime >= cfg_.client_timeout || cl->nreq >= cfg_.client_max_reqs))
        idle.push_back(cl);
    } else {
      auto* u = static_cast<Upstream*>(c);
      if (u->pend.empty() && !u->owner && u->ka_timeout >= 0 &&
          (t - u->atime >= u->ka_timeout || u->count >= u->ka_max))
        stale.push_back(u);
    }
  }
  for (Client* c : idle) {
    gc_closed++;
    close_client(c);
  }
  for (Upstream* u : stale) close_upstream(u);
}

// =====================================================================================
// Proxy
// =====================================================================================
Proxy::Proxy(const ProxyConfig& cfg, std::shared_ptr<CacheBackend> backend)
    : cfg_(cfg), backend_(std::move(backend)) {
  SH_CHECK(!cfg_.upstreams.empty(), "no upstream web servers specified");
  cfg_.tag_header = to_lower(cfg_.tag_header);  // (parsed header names are lower case)
  SH_CHECK(cfg_.threads >= 1, "threads >= 1");
  if (cfg_.cache_enabled) SH_CHECK(backend_ != nullptr, "cache enabled without a backend");
  up_down_until_.reset(new std::atomic<double>[cfg_.upstreams.size()]);
  health_down_.reset(new std::atomic<bool>[cfg_.upstreams.size()]);
  for (size_t i = 0; i < cfg_.upstreams.size(); ++i) {
    up_down_until_[i] = 0;
    health_down_[i] = false;
  }
}

Proxy::~Proxy() {
  stop();
  for (auto& t : threads_)
    if (t.joinable()) t.join();
  if (health_th_.joinable()) health_th_.join();
}

bool Proxy::upstream_up(int idx, double now) const {
  return !health_down_[idx].load(std::memory_order_relaxed) && now >= up_down_until_[idx].load();
}

// One health probe: connect, `GET path`, read the status line; true for a status < 400
// within the timeout. Blocking I/O with poll() deadlines on the checker thread only.
static bool probe_upstream(const Addr& a, const std::string& path, int timeout_ms) {
  const double deadline = now_s() + timeout_ms * 1e-3;
  auto left_ms = [&] { return std::max(0, (int)((deadline - now_s()) * 1e3)); };
  const int fd = connect_nonblock(a);
  if (fd < 0) return false;
  bool ok = false;
  pollfd pfd{fd, POLLOUT, 0};
  if (poll(&pfd, 1, left_ms()) == 1 && (pfd.revents & POLLOUT)) {
    int err = 0;
    socklen_t el = sizeof err;
    getsockopt(fd, SOL_SOCKET, SO_ERROR, &err, &el);
    const std::string req = "GET " + path + " HTTP/1.1\r\nHost: " + a.host +
                            "\r\nUser-Agent: shellac-health\r\nConnection: close\r\n\r\n";
    if (!err && send(fd, req.data(), req.size(), MSG_NOSIGNAL) == (ssize_t)req.size()) {
      std::string head;
      char buf[512];
      while (head.find("\r\n") == std::string::npos && left_ms() > 0) {
        pfd = pollfd{fd, POLLIN, 0};
        if (poll(&pfd, 1, left_ms()) != 1) break;
        const ssize_t k = recv(fd, buf, sizeof buf, 0);
        if (k <= 0) break;
        head.append(buf, (size_t)k);
      }
      // "HTTP/1.x SSS ..."
      if (head.size() >= 12 && head.compare(0, 5, "HTTP/") == 0) {
        const int status = std::atoi(head.c_str() + 9);
        ok = status >= 100 && status < 400;
      }
    }
  }
  close(fd);
  return ok;
}

void Proxy::health_loop() {
  const size_t n = cfg_.upstreams.size();
  std::vector<int> fails(n, 0), passes(n, 0);
  while (running_) {
    for (size_t i = 0; i < n && running_; ++i) {
      const bool ok = probe_upstream(cfg_.upstreams[i], cfg_.health_path, cfg_.health_timeout_ms);
      health_checks_++;
      if (ok) {
        fails[i] = 0;
        if (health_down_[i] && ++passes[i] >= cfg_.health_passes) {
          health_down_[i] = false;
          health_transitions_++;
        }
      } else {
        passes[i] = 0;
        if (!health_down_[i] && ++fails[i] >= cfg_.health_fails) {
          health_down_[i] = true;
          health_transitions_++;
        }
      }
    }
    // sleep in small slices so stop() is prompt
    const double until = now_s() + cfg_.health_interval_ms * 1e-3;
    while (running_ && now_s() < until)
      std::this_thread::sleep_for(std::chrono::milliseconds(
          std::min(20, std::max(1, (int)((until - now_s()) * 1e3)))));
  }
}

void Proxy::upstream_failed(int idx, double now) {
  up_down_until_[idx] = now + cfg_.upstream_retry_s;
}

void Proxy::start() {
  SH_CHECK(!running_, "already running");
  reserve_fd_table(cfg_.max_fds);
  start_time_ = now_s();
  const int first = listen_tcp(cfg_.bind, cfg_.port, cfg_.threads > 1, cfg_.backlog);
  port_ = local_port(first);
  running_ = true;
  for (int i = 0; i < cfg_.threads; ++i) {
    const int fd = i == 0 ? first : listen_tcp(cfg_.bind, port_, true, cfg_.backlog);
    reactors_.emplace_back(new Reactor(this, i, fd));
  }
  for (size_t i = 0; i < reactors_.size(); ++i) {
    Reactor* rp = reactors_[i].get();
    threads_.emplace_back([this, rp, i] {
      pin_thread(cfg_.cpus, i);
      const std::string nm = "shellac-rx" + std::to_string(i);  // per-thread CPU accounting
      pthread_setname_np(pthread_self(), nm.c_str());
      rp->loop();
    });
  }
  if (!cfg_.health_path.empty()) health_th_ = std::thread([this] { health_loop(); });
}

void Proxy::wait() {
  for (auto& t : threads_)
    if (t.joinable()) t.join();
}

void Proxy::stop() {
  running_ = false;
  for (auto& r : reactors_) r->wake();
}

namespace {
// A minimal reader of the stats JSON above (objects, arrays, numbers, strings; no escapes
// beyond \" are ever produced), flattened into Prometheus samples: nested keys join with
// '_' under the `shellac_` prefix, array elements become an `i` label, and string fields
// (server, backend) become labels of one `shellac_info` sample.
struct PromFlat {
  const std::string& j;
  size_t p = 0;
  std::ostringstream out;
  std::vector<std::pair<std::string, std::string>> info;
  explicit PromFlat(const std::string& s) : j(s) {}
  void ws() {
    while (p < j.size() && (j[p] == ' ' || j[p] == '\n' || j[p] == '\t' || j[p] == '\r')) ++p;
  }
  std::string str() {
    std::string r;
    ++p;  // opening quote
    while (p < j.size() && j[p] != '"') {
      if (j[p] == '\\' && p + 1 < j.size()) ++p;
      r += j[p++];
    }
    ++p;
    return r;
  }
  static std::string clean(const std::string& k) {
    std::string r;
    for (char c : k) r += (std::isalnum((unsigned char)c) || c == '_') ? c : '_';
    return r;
  }
  void value(const std::string& name, const std::string& label) {
    ws();
    if (p >= j.size()) return;
    const char c = j[p];
    if (c == '{') {
      ++p;
      for (;;) {
        ws();
        if (p < j.size() && j[p] == '}') {
          ++p;
          return;
        }
        const std::string k = str();
        ws();
        ++p;  // ':'
        value(name.empty() ? clean(k) : name + "_" + clean(k), label);
        ws();
        if (p < j.size() && j[p] == ',') ++p;
      }
    } else if (c == '[') {
      ++p;
      for (int i = 0;; ++i) {
        ws();
        if (p < j.size() && j[p] == ']') {
          ++p;
          return;
        }
        value(name, "i=\"" + std::to_string(i) + "\"");
        ws();
        if (p < j.size() && j[p] == ',') ++p;
      }
    } else if (c == '"') {
      info.emplace_back(name, str());
    } else {
      const size_t a = p;
      while (p < j.size() && j[p] != ',' && j[p] != '}' && j[p] != ']' && !std::isspace((unsigned char)j[p])) ++p;
      out << "shellac_" << name;
      if (!label.empty()) out << "{" << label << "}";
      out << " " << j.substr(a, p - a) << "\n";
    }
  }
};
}  // namespace

std::string prometheus_text(const std::string& stats_json) {
  PromFlat f(stats_json);
  f.value("", "");
  std::ostringstream o;
  if (!f.info.empty()) {
    o << "shellac_info{";
    for (size_t i = 0; i < f.info.size(); ++i) {
      std::string v;
      for (char c : f.info[i].second) v += (c == '"' || c == '\\') ? '_' : c;
      o << (i ? "," : "") << f.info[i].first << "=\"" << v << "\"";
    }
    o << "} 1\n";
  }
  o << f.out.str();
  return o.str();
}

void Proxy::note_purge(KeyedSelector what) {
  std::lock_guard<std::mutex> lk(purge_mu_);
  if (purge_ring_.empty()) purge_ring_.resize(kPurgeRing);
  const uint64_t gen = purge_gen_.load(std::memory_order_relaxed) + 1;
  purge_ring_[gen % kPurgeRing] = PurgeRec{gen, std::move(what)};
  purge_gen_.store(gen, std::memory_order_release);
}

bool Proxy::purged_since(uint64_t gen, const std::string& key, const std::string& base_key,
                         const std::vector<uint64_t>* tags, bool overflow) {
  if (purge_gen_.load(std::memory_order_acquire) == gen) return false;  // the common case
  std::lock_guard<std::mutex> lk(purge_mu_);
  const uint64_t cur = purge_gen_.load(std::memory_order_relaxed);
  if (cur - gen > kPurgeRing) return true;  // the ring wrapped past this fetch: assume purged
  for (uint64_t g = gen + 1; g <= cur; ++g)
    if (purge_ring_[g % kPurgeRing].what.matches_fill(key, base_key, tags, overflow)) return true;
  return false;
}

std::string Proxy::stats_json() {
  uint64_t req = 0, hit = 0, miss = 0, ur = 0, resp = 0, bo = 0, err = 0, cl = 0, up = 0, acc = 0,
           gcc = 0, sets = 0, bad = 0, uf = 0, rt = 0, col = 0, stm = 0, stp = 0, lmax = 0,
           lslow = 0, idd = 0, vst = 0, vh = 0, prq = 0, pob = 0, pdn = 0, fpg = 0, spr = 0,
           sob = 0, tpr = 0, tpo = 0, tso = 0, tgf = 0, insp = 0, pdr = 0, pgr = 0;
  uint64_t ph[5] = {};  // --partial-hits
  uint64_t ch[4] = {};  // --conditional-hits
  uint64_t pmax[5] = {}, crst = 0;
  uint64_t gr[6] = {};  // --grace: stale hits, revalidations and their outcomes
  uint64_t h[kHistBuckets] = {};
  for (auto& r : reactors_) {
    req += r->requests; hit += r->hits; miss += r->misses; ur += r->upstream_reqs;
    resp += r->responses; bo += r->bytes_out; err += r->errors; cl += r->clients;
    up += r->upstreams; acc += r->accepts; gcc += r->gc_closed; sets += r->cache_sets;
    bad += r->bad_requests; uf += r->upstream_failures; rt += r->retries; col += r->collapsed;
    stm += r->streamed; stp += r->stream_pauses;
    lmax = std::max<uint64_t>(lmax, r->loop_max_us);
    lslow += r->loop_slow;
    crst += r->client_resets;
    idd += r->identity_decoded;
    vst += r->vary_stored;
    vh += r->vary_hits;
    prq += r->purge_requests; pob += r->purged_objects; pdn += r->purge_denied;
    fpg += r->fills_purged;
    spr += r->soft_purge_requests; sob += r->softened_objects;
    tpr += r->tag_purge_requests; tpo += r->tag_purged_objects;
    tso += r->tag_softened_objects; tgf += r->tagged_fills;
    insp += r->inspect_requests; pdr += r->purge_dry_runs;
    pgr += r->purge_glob_requests;
    ph[0] += r->range_requests; ph[1] += r->range_206; ph[2] += r->range_416;
    ph[3] += r->head_hits; ph[4] += r->partial_fallbacks;
    ch[0] += r->conditional_requests; ch[1] += r->not_modified_304;
    ch[2] += r->if_range_matched; ch[3] += r->if_range_failed;
    gr[0] += r->stale_served; gr[1] += r->revalidations; gr[2] += r->revalidated_304;
    gr[3] += r->revalidate_touched; gr[4] += r->revalidate_restored;
    gr[5] += r->revalidate_errors;
    for (int k = 0; k < 5; ++k) pmax[k] = std::max<uint64_t>(pmax[k], r->phase_max_us[k]);
    for (int b = 0; b < kHistBuckets; ++b) h[b] += r->hist[b];
  }
  uint64_t total = 0;
  for (uint64_t v : h) total += v;
  auto pct = [&](double q) -> double {
    if (!total) return 0;
    uint64_t acc2 = 0;
    for (int b = 0; b < kHistBuckets; ++b) {
      acc2 += h[b];
      if (acc2 >= q * total) return b == 0 ? 1.0 : std::pow(2.0, b);  // bucket upper bound (us)
    }
    return std::pow(2.0, kHistBuckets);
  };
  std::ostringstream o;
  o << "{\"server\":\"" << cfg_.server_name << "\",\"uptime_s\":" << (now_s() - start_time_)
    << ",\"threads\":" << cfg_.threads << ",\"requests\":" << req << ",\"cache_hits\":" << hit
    << ",\"cache_misses\":" << miss << ",\"upstream_requests\":" << ur
    << ",\"upstream_responses\":" << resp << ",\"cache_fills\":" << sets
    << ",\"bytes_out\":" << bo << ",\"errors\":" << err << ",\"bad_requests\":" << bad
    << ",\"upstream_failures\":" << uf << ",\"retries\":" << rt << ",\"collapsed\":" << col
    << ",\"streamed\":" << stm << ",\"stream_pauses\":" << stp << ",\"clients\":" << cl
    << ",\"upstream_conns\":" << up << ",\"accepts\":" << acc << ",\"gc_closed\":" << gcc
    << ",\"client_resets\":" << crst << ",\"identity_decoded\":" << idd
    << ",\"vary_stored\":" << vst << ",\"vary_hits\":" << vh
    << ",\"purge_requests\":" << prq << ",\"purged_objects\":" << pob
    << ",\"purge_denied\":" << pdn << ",\"fills_not_cached_purged\":" << fpg
    << ",\"soft_purge_requests\":" << spr << ",\"softened_objects\":" << sob
    << ",\"tag_purge_requests\":" << tpr << ",\"tag_purged_objects\":" << tpo
    << ",\"tag_softened_objects\":" << tso << ",\"tagged_fills\":" << tgf
    << ",\"purge_glob_requests\":" << pgr
    << ",\"inspect_requests\":" << insp << ",\"purge_dry_runs\":" << pdr
    << ",\"range_requests\":" << ph[0] << ",\"range_206\":" << ph[1]
    << ",\"range_416\":" << ph[2] << ",\"head_hits\":" << ph[3]
    << ",\"partial_fallbacks\":" << ph[4]
    << ",\"conditional_requests\":" << ch[0] << ",\"not_modified_304\":" << ch[1]
    << ",\"if_range_matched\":" << ch[2] << ",\"if_range_failed\":" << ch[3]
    << ",\"stale_served\":" << gr[0] << ",\"revalidations\":" << gr[1]
    << ",\"revalidated_304\":" << gr[2] << ",\"revalidate_touched\":" << gr[3]
    << ",\"revalidate_restored\":" << gr[4] << ",\"revalidate_errors\":" << gr[5]
    << ",\"loop_max_us\":" << lmax << ",\"loop_slow\":" << lslow
    << ",\"loop_phase_max_us\":{\"accept\":" << pmax[0] << ",\"client\":" << pmax[1]
    << ",\"upstream\":" << pmax[2] << ",\"posted\":" << pmax[3] << ",\"timer\":" << pmax[4]
    << "}"
    << ",\"latency_us\":{\"p50\":" << pct(0.5) << ",\"p99\":" << pct(0.99) << ",\"samples\":"
    << total << "}";
  if (gzip_) {
    uint64_t gb = 0, gi = 0;
    for (auto& r : reactors_) {
      gb += r->gzip_gpu_bodies;
      gi += r->gzip_gpu_inflated;
    }
    StatList gs;
    gzip_->stats(&gs);
    o << ",\"gzip_gpu\":{\"completed\":" << gb << ",\"identity_served\":" << gi;
    for (const auto& kv : gs) o << ",\"" << kv.first << "\":" << kv.second;
    o << "}";
  }
  o << ",\"health_checks\":" << health_checks_.load()
    << ",\"health_transitions\":" << health_transitions_.load() << ",\"upstreams_up\":[";
  const double tn = now_s();
  for (size_t i = 0; i < cfg_.upstreams.size(); ++i) o << (i ? "," : "") << (upstream_up((int)i, tn) ? 1 : 0);
  o << "]";
  if (backend_) {
    StatList st;
    backend_->stats(&st);
    o << ",\"backend\":\"" << backend_->name() << "\",\"cache\":{";
    for (size_t i = 0; i < st.size(); ++i)
      o << (i ? "," : "") << "\"" << st[i].first << "\":" << st[i].second;
    o << "}";
  }
  o << "}";
  return o.str();
}

}  // namespace shellac
