// The bucket pipeline (crossbow_amd/csrc/bucket_pipeline.h) on the CPU, under
// ASan + UBSan (tests/test_bucket_pipeline.py builds and runs it): the two
// geometry rules against values worked out by hand from their formulas, the
// narrowing of an argument struct to one bucket, and the order in which the
// two templates enqueue a step, taken down by lanes that only record what
// they are asked to do.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "bucket_pipeline.h"

using namespace cbx::host;

#define CHECK(cond)                                                        \
  do {                                                                     \
    if (!(cond)) {                                                         \
      std::fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
      std::exit(1);                                                        \
    }                                                                      \
  } while (0)

// ---------------------------------------------------------------------------
// Geometry
// ---------------------------------------------------------------------------
static int grids = 0;

// The buckets tile [0, n4) without gap or overlap, every start is a multiple
// of the pad, only the last bucket is short.
static void check_grid(const BucketGrid &g, int64_t n4, int64_t b4, int64_t nb, int64_t last_len) {
  CHECK(g.b4 == b4 && g.nb == nb && g.n4 == n4);
  int64_t at = 0;
  for (int64_t b = 0; b < g.nb; ++b) {
    const Bucket k = g.bucket(b);
    CHECK(k.index == b && k.start4 == g.start_of(b) && k.len4 == g.len_of(b));
    CHECK(k.first == (b == 0) && k.last == (b == g.nb - 1));
    CHECK(k.start4 == at);
    CHECK(k.start4 % kBucketPad4 == 0);
    CHECK(k.last ? (k.len4 <= g.b4 && (n4 == 0 || k.len4 > 0)) : k.len4 == g.b4);
    at += k.len4;
  }
  CHECK(at == n4);
  CHECK(g.len_of(g.nb - 1) == last_len);
  ++grids;
}

static void test_geometry() {
  CHECK(kBucketPad4 == 1024 && kDefaultBuckets == 8);
  // by_count: b4 = ceil(ceil(n4 / request) / 1024) * 1024, nb = ceil(n4 / b4)
  check_grid(BucketGrid::by_count(9984, 5), 9984, 2048, 5, 1792);  // ceil(9984 / 5) = 1997 -> 2048; 9984 - 4 * 2048
  check_grid(BucketGrid::by_count(9984, 0), 9984, 2048, 5, 1792);  // 0: 8 asked, 1248 -> 2048: the same grid
  check_grid(BucketGrid::by_count(9984, -3), 9984, 2048, 5, 1792);
  check_grid(BucketGrid::by_count(9984, 8), 9984, 2048, 5, 1792);
  check_grid(BucketGrid::by_count(9984, 1), 9984, 9984, 1, 9984);
  check_grid(BucketGrid::by_count(74752, 37), 74752, 2048, 37, 1024);  // 2021 -> 2048; 74752 - 36 * 2048
  check_grid(BucketGrid::by_count(0, 0), 0, 0, 1, 0);
  check_grid(BucketGrid::by_count(1280, 8), 1280, 1024, 2, 256);  // a bulk that is not whole pads
  // by_elements: b4 = ceil(floor(elements / 4) / 1024) * 1024, or from floor(n4 / 8) at G > 1
  check_grid(BucketGrid::by_elements(10240, 4096, 2), 10240, 1024, 10, 1024);
  check_grid(BucketGrid::by_elements(10240, 0, 2), 10240, 2048, 5, 2048);  // 1280 -> 2048
  check_grid(BucketGrid::by_elements(10240, 0, 1), 10240, 10240, 1, 10240);
  check_grid(BucketGrid::by_elements(10240, 3, 1), 10240, 10240, 1, 10240);  // 3 / 4 = 0 float4s: one bucket
  check_grid(BucketGrid::by_elements(10240, 1000000, 2), 10240, 10240, 1, 10240);
  check_grid(BucketGrid::whole(10240), 10240, 10240, 1, 10240);
  // where the two rules part: 8193 / 8 is 1025 -> 2048 by the ceiling
  // (5 buckets), 1024 -> 1024 by the floor (9 buckets)
  check_grid(BucketGrid::by_count(8193, 8), 8193, 2048, 5, 1);
  check_grid(BucketGrid::by_elements(8193, 0, 2), 8193, 1024, 9, 1);
}

// ---------------------------------------------------------------------------
// range_of / with_tail, on stand-ins with the members of SmaArgs / AvgArgs
// (snapshots) and SsgdArgs (none).
// ---------------------------------------------------------------------------
struct V4 {
  float x[4];
};
struct WithSnapshots {
  const V4 *s[4];
  V4 *w[4];
  V4 *z, *last, *acc;
  const V4 *D;
  int64_t n4;
  int nrep;
  int64_t tail_lo, tail_hi;
};
struct WithoutSnapshots {
  V4 *w[4];
  V4 *z, *last, *acc;
  const V4 *D;
  int64_t n4;
  int nrep;
  int64_t tail_lo, tail_hi;
};

static void test_ranges() {
  std::vector<V4> buf(7 * 64);
  V4 *const base = buf.data();
  auto at = [&](int k) { return base + k * 64; };
  WithSnapshots a = {};
  a.nrep = 2;
  a.s[0] = at(0);
  a.s[1] = nullptr;  // a model that reads no snapshot of this replica
  a.w[0] = at(1);
  a.w[1] = at(2);
  a.z = at(3);
  a.last = nullptr;
  a.acc = at(4);
  a.D = at(5);
  a.n4 = 64;
  const WithSnapshots b = range_of(a, 24, 16);
  CHECK(b.s[0] == at(0) + 24 && b.s[1] == nullptr);
  CHECK(b.w[0] == at(1) + 24 && b.w[1] == at(2) + 24);
  CHECK(b.w[2] == nullptr && b.s[2] == nullptr);  // past nrep: untouched
  CHECK(b.z == at(3) + 24 && b.last == nullptr && b.acc == at(4) + 24 && b.D == at(5) + 24);
  CHECK(b.n4 == 16 && b.nrep == 2 && b.tail_lo == 0 && b.tail_hi == 0);
  CHECK(a.z == at(3) && a.n4 == 64);  // the source is left as it was
  CHECK((const char *)b.z - (const char *)a.z == 24 * 16);  // float4s, 16 bytes each
  a.last = at(6);
  CHECK(range_of(a, 8, 8).last == at(6) + 8);
  // The tail: a buffer of n = 64 * 4 + 3 floats whose bulk is 64 float4s; a
  // launch that starts at float4 48 sees floats [64, 67) of the buffer at
  // [ (64 - 48) * 4, 259 - 48 * 4 ) = [64, 67) relative to its pointers.
  const WithSnapshots t = with_tail(range_of(a, 48, 16), 64, 259, 48);
  CHECK(t.tail_lo == 64 && t.tail_hi == 67 && t.n4 == 16 && t.z == at(3) + 48);
  const WithSnapshots t0 = with_tail(a, 64, 259, 0);  // the whole buffer in one launch
  CHECK(t0.tail_lo == 256 && t0.tail_hi == 259 && t0.z == at(3));
  WithoutSnapshots c = {};
  c.nrep = 1;
  c.w[0] = at(1);
  c.z = at(3);
  c.acc = at(4);
  c.D = c.acc;  // one rank: K reads D = acc
  const WithoutSnapshots d = with_tail(range_of(c, 32, 32), 64, 257, 32);
  CHECK(d.w[0] == at(1) + 32 && d.z == at(3) + 32 && d.last == nullptr && d.acc == at(4) + 32 && d.D == d.acc);
  CHECK(d.n4 == 32 && d.tail_lo == 128 && d.tail_hi == 129);
}

// ---------------------------------------------------------------------------
// The order
// ---------------------------------------------------------------------------
struct Op {
  int dev;
  char stream;  // 'S' the step's stream, 'C' the comm stream, 'G' the group bracket
  std::string op;
  int64_t b;
};

struct Recorder {
  std::vector<Op> log;  // everything, in the order the host issued it
  int current = -1;     // the device select() made current
  int fail_dev = -1;    // launch_a of bucket fail_b on this device returns fail_code
  int64_t fail_b = -1;
  int fail_code = 0;
  size_t size_at_failure = 0;
};

struct Lane {
  Recorder *r;
  int dev;
  const BucketGrid *g;
  int note(char stream, const char *op, int64_t b) {
    CHECK(r->current == dev);  // every call follows a select() of its own lane
    r->log.push_back({dev, stream, op, b});
    return 0;
  }
  int launch(const char *op, const Bucket &b) {
    CHECK(b.start4 == g->start_of(b.index) && b.len4 == g->len_of(b.index));
    CHECK(b.first == (b.index == 0) && b.last == (b.index == g->nb - 1));
    return note('S', op, b.index);
  }
  int select() {
    r->current = dev;
    return 0;
  }
  int launch_a(const Bucket &b) {
    if (dev == r->fail_dev && b.index == r->fail_b) {
      r->size_at_failure = r->log.size();
      return r->fail_code;
    }
    return launch("A", b);
  }
  int launch_b(const Bucket &b) { return launch("B", b); }
  int launch_k(const Bucket &b) { return launch("K", b); }
  int all_reduce(const Bucket &b, bool on_comm) { return note(on_comm ? 'C' : 'S', "AR", b.index); }
  int record_a(int64_t b) { return note('S', "ra", b); }
  int wait_a(int64_t b) { return note('C', "wa", b); }
  int record_r(int64_t b) { return note('C', "rr", b); }
  int wait_r(int64_t b) { return note('S', "wr", b); }
};

struct Run {
  Recorder rec;
  BucketGrid grid;
  std::vector<Lane> lanes;
  Run(int G, int64_t nb) {
    grid = BucketGrid::by_count(nb * 1024 - 512, nb);  // nb buckets of 1024 float4s, the last one short
    CHECK(grid.nb == nb);
    for (int k = 0; k < G; ++k) lanes.push_back({&rec, k, &grid});
  }
  auto begin() {
    return [this] {
      rec.log.push_back({-1, 'G', "begin", -1});
      return 0;
    };
  }
  auto end() {
    return [this] {
      rec.log.push_back({-1, 'G', "end", -1});
      return 0;
    };
  }
  // What device `dev` received on `stream`, as "A0 ra0 A1 ...".
  std::string stream_log(int dev, char stream) const {
    std::string s;
    for (const Op &o : rec.log) {
      if (o.dev != dev || o.stream != stream) continue;
      if (!s.empty()) s += ' ';
      s += o.op + std::to_string(o.b);
    }
    return s;
  }
  // Position in the host's order of device dev's `op` of bucket b (-1: absent; it occurs once).
  long find(int dev, const char *op, int64_t b) const {
    long at = -1;
    for (size_t i = 0; i < rec.log.size(); ++i)
      if (rec.log[i].dev == dev && rec.log[i].op == op && rec.log[i].b == b) {
        CHECK(at < 0);
        at = (long)i;
      }
    return at;
  }
  char stream_of(int dev, const char *op, int64_t b) const { return rec.log[(size_t)find(dev, op, b)].stream; }
};

// The safety property, stated directly on the host's order.  Operations on
// one stream run in the order they were enqueued, so "enqueued after, on the
// same stream" is "runs after".
static void check_safety(const Run &run, int G, const char *consumer, bool collective, bool entry_only) {
  const int64_t nb = run.grid.nb;
  const bool piped = collective && nb > 1;
  for (int k = 0; k < G; ++k)
    for (int64_t b = 0; b < nb; ++b) {
      const long ar = run.find(k, "AR", b), use = run.find(k, consumer, b);
      CHECK(use >= 0 && (ar >= 0) == collective);
      if (collective) CHECK(ar < use);
      if (!piped) {  // in order on the step's stream, no event touched
        for (const char *ev : {"ra", "wa", "rr", "wr"}) CHECK(run.find(k, ev, b) < 0);
        if (collective) CHECK(run.stream_of(k, "AR", b) == 'S');
        continue;
      }
      CHECK(run.stream_of(k, "AR", b) == 'C');
      // AR(b) after the record of a(b), and after the comm stream's wait on it
      // (reduce_apply: the one entry event, a(0), stands before every AR)
      const int64_t a = entry_only ? 0 : b;
      const long ra = run.find(k, "ra", a), wa = run.find(k, "wa", a);
      CHECK(ra >= 0 && ra < wa && wa < ar);
      if (!entry_only) CHECK(run.find(k, "A", b) < ra);  // a(b) is recorded behind A(b)
      if (entry_only && b > 0) CHECK(run.find(k, "ra", b) < 0 && run.find(k, "wa", b) < 0);
      // r(b) is recorded after AR(b), on the same stream
      const long rr = run.find(k, "rr", b), wr = run.find(k, "wr", b);
      CHECK(ar < rr && run.stream_of(k, "rr", b) == 'C');
      // B(b) / K(b) after the step's stream waits on r(b), which is recorded by then
      CHECK(rr < wr && wr < use && run.stream_of(k, "wr", b) == 'S' && run.stream_of(k, consumer, b) == 'S');
    }
  // the group bracket encloses exactly one all-reduce per device, and nothing else
  size_t i = 0, brackets = 0;
  const std::vector<Op> &log = run.rec.log;
  while (i < log.size()) {
    if (log[i].stream != 'G') {
      CHECK(log[i].op != "AR");  // none outside a bracket
      ++i;
      continue;
    }
    CHECK(log[i].op == "begin");
    const int64_t b = log[i + 1].b;
    for (int k = 0; k < G; ++k) {
      const Op &o = log[i + 1 + (size_t)k];
      CHECK(o.dev == k && o.op == "AR" && o.b == b);
    }
    CHECK(log[i + 1 + (size_t)G].stream == 'G' && log[i + 1 + (size_t)G].op == "end");
    i += (size_t)G + 2;
    ++brackets;
  }
  CHECK(brackets == (collective ? (size_t)nb : 0));
}

static int orders = 0;

static void test_accumulate_reduce_apply(int G) {
  const char *step[6] = {nullptr,
                         "A0 AR0 B0",
                         "A0 ra0 A1 ra1 wr0 B0 wr1 B1",
                         nullptr,
                         nullptr,
                         "A0 ra0 A1 ra1 wr0 B0 A2 ra2 wr1 B1 A3 ra3 wr2 B2 A4 ra4 wr3 B3 wr4 B4"};
  const char *comm[6] = {nullptr,
                         "",
                         "wa0 AR0 rr0 wa1 AR1 rr1",
                         nullptr,
                         nullptr,
                         "wa0 AR0 rr0 wa1 AR1 rr1 wa2 AR2 rr2 wa3 AR3 rr3 wa4 AR4 rr4"};
  for (int64_t nb : {1, 2, 5}) {
    Run run(G, nb);
    CHECK(accumulate_reduce_apply(run.lanes, run.grid, run.begin(), run.end()) == 0);
    for (int k = 0; k < G; ++k) {
      CHECK(run.stream_log(k, 'S') == step[nb]);
      CHECK(run.stream_log(k, 'C') == comm[nb]);
    }
    check_safety(run, G, "B", true, false);
    ++orders;
  }
}

static void test_reduce_apply(int G) {
  const char *step[6] = {nullptr, "AR0 K0", "ra0 wr0 K0 wr1 K1", nullptr, nullptr,
                         "ra0 wr0 K0 wr1 K1 wr2 K2 wr3 K3 wr4 K4"};
  const char *comm[6] = {nullptr, "", "wa0 AR0 rr0 AR1 rr1", nullptr, nullptr,
                         "wa0 AR0 rr0 AR1 rr1 AR2 rr2 AR3 rr3 AR4 rr4"};
  const char *alone[6] = {nullptr, "K0", "K0 K1", nullptr, nullptr, "K0 K1 K2 K3 K4"};
  for (int64_t nb : {1, 2, 5}) {
    Run run(G, nb);
    CHECK(reduce_apply(run.lanes, run.grid, true, run.begin(), run.end()) == 0);
    for (int k = 0; k < G; ++k) {
      CHECK(run.stream_log(k, 'S') == step[nb]);
      CHECK(run.stream_log(k, 'C') == comm[nb]);
    }
    check_safety(run, G, "K", true, true);
    // no collective at all: K only, no event, no bracket
    Run solo(G, nb);
    CHECK(reduce_apply(solo.lanes, solo.grid, false, solo.begin(), solo.end()) == 0);
    for (int k = 0; k < G; ++k) {
      CHECK(solo.stream_log(k, 'S') == alone[nb]);
      CHECK(solo.stream_log(k, 'C').empty());
    }
    CHECK(solo.rec.log.size() == (size_t)(G * nb));
    check_safety(solo, G, "K", false, true);
    orders += 2;
  }
}

// A lane whose launch of A(1) fails ends the walk with its code; nothing more
// is enqueued on any device.
static void test_failure(int G) {
  Run run(G, 5);
  run.rec.fail_dev = G - 1;
  run.rec.fail_b = 1;
  run.rec.fail_code = -7;
  CHECK(accumulate_reduce_apply(run.lanes, run.grid, run.begin(), run.end()) == -7);
  CHECK(run.rec.size_at_failure > 0 && run.rec.log.size() == run.rec.size_at_failure);
  CHECK(run.stream_log(G - 1, 'S') == "A0 ra0");
  CHECK(run.stream_log(G - 1, 'C') == "wa0 AR0 rr0");
  CHECK(run.stream_log(0, 'S') == (G == 1 ? "A0 ra0" : "A0 ra0 A1 ra1"));
  CHECK(run.find(0, "B", 0) < 0);
  // and a bracket that fails to open: no collective is issued
  Run shut(G, 2);
  auto refuse = [] { return -3; };
  CHECK(reduce_apply(shut.lanes, shut.grid, true, refuse, shut.end()) == -3);
  for (const Op &o : shut.rec.log) CHECK(o.op != "AR" && o.op != "K" && o.stream != 'G');
}

int main() {
  test_geometry();
  test_ranges();
  for (int G : {1, 2}) {
    test_accumulate_reduce_apply(G);
    test_reduce_apply(G);
    test_failure(G);
  }
  std::printf("ok %d grids, %d orders\n", grids, orders);
  return 0;
}
