// bucket_pipeline.h -- the bucketed all-reduce pipeline of the barrier steps:
// how a model is cut into buckets, how a step's argument struct is narrowed to
// one bucket, and the order in which a step's kernels, collectives, event
// records and waits are enqueued.  Plain C++, no HIP or RCCL: the order and
// the geometry are tested on the CPU (tests/native/bucket_pipeline_test.cpp).
//
// A model of n4 float4s is cut into nb buckets of b4 float4s, whole kPadFloat4
// units, the last one possibly short.  With one bucket a step runs in order on
// its stream and touches no event.  With more, a second stream per device runs
// the all-reduce of one bucket beside the kernels of the next:
//
// accumulate_reduce_apply (SMA over the caller's buffers, elastic averaging,
// Polyak-Ruppert): kernel A accumulates the device's replicas into acc, acc is
// all-reduced into D, kernel B applies D.
//   stream      : A(0) A(1) [wait r(0)] B(0) A(2) [wait r(1)] B(1) ... [wait r(nb-1)] B(nb-1)
//   comm_stream : [wait a(0)] AR(0) [wait a(1)] AR(1) ...
// reduce_apply (synchronous SGD): acc is complete when the step begins.
//   stream      : [entry] [wait r(0)] K(0) [wait r(1)] K(1) ...
//   comm_stream : [wait entry] AR(0) AR(1) ...
// a(b) is recorded on the stream after A(b), r(b) on the comm stream after
// AR(b); the entry is a(0), recorded before anything else.  AR(b) reads what
// A(b) wrote only after a(b), B(b) / K(b) read what AR(b) wrote only after
// r(b).  The next step's A(0) follows this step's last B on the same stream
// and its AR(b) waits for its A(b), so no buffer is rewritten while still in
// use.
//
// A lane is one device of a step: the door (sync_steps.hip for the context,
// sma_seam.hip for the caller's buffers) makes it of its device, the step's
// stream and the argument struct.  The two templates call, each returning a
// status code (negative: the walk ends there with that code):
//   select()                          make the lane's device current
//   launch_a / launch_b / launch_k (const Bucket &)
//   all_reduce(const Bucket &, bool on_comm)   on the comm stream, or on the step's
//   record_a(b) / wait_a(b)           on the step's stream / the comm stream waits
//   record_r(b) / wait_r(b)           on the comm stream / the step's stream waits
// and group_begin() / group_end() around the all-reduces of one bucket (the
// ncclGroupStart / ncclGroupEnd bracket; a collective inside it is enqueued
// when the bracket closes).  What only one door needs (timing events, the
// step's stop event) lives inside that door's lane methods.
#pragma once

#include <algorithm>
#include <cstdint>

namespace cbx::host {

// cbx::kPadFloat4 (sma_internal.h, which needs HIP): bucket starts are whole
// kernel trips.  context_internal.h asserts that the two agree.
constexpr int64_t kBucketPad4 = 1024;
// Buckets of the G > 1 pipeline when none were asked for.
constexpr int64_t kDefaultBuckets = 8;

struct Bucket {
  int64_t index, start4, len4;  // float4s [start4, start4 + len4) of every buffer
  bool first, last;
};

struct BucketGrid {
  int64_t b4 = 0, nb = 1;  // float4s per bucket, buckets
  int64_t n4 = 0;

  int64_t start_of(int64_t b) const { return b * b4; }
  int64_t len_of(int64_t b) const { return std::min(b4, n4 - b * b4); }
  Bucket bucket(int64_t b) const { return {b, start_of(b), len_of(b), b == 0, b == nb - 1}; }

  // The seam's rule, from a requested bucket count (cbx_sma_plan_set_buckets;
  // 0: kDefaultBuckets): the bucket is the ceiling of n4 / count, rounded up
  // to whole pads, so fewer buckets than asked for may result.
  static BucketGrid by_count(int64_t n4, int64_t requested) {
    const int64_t pad = kBucketPad4, req = requested > 0 ? requested : kDefaultBuckets;
    BucketGrid g;
    g.n4 = g.b4 = n4;
    if (req > 1 && n4 > 0) g.b4 = ((n4 + req - 1) / req + pad - 1) / pad * pad;
    g.nb = g.b4 > 0 ? (n4 + g.b4 - 1) / g.b4 : 1;
    return g;
  }
  // The context's rule, from a bucket size in elements (cbx_set_bucket_elements;
  // 0: kDefaultBuckets at G > 1, else one bucket): the floor of the division,
  // rounded up to whole pads.
  static BucketGrid by_elements(int64_t n4, int64_t bucket_elems, int G) {
    const int64_t pad = kBucketPad4;
    BucketGrid g;
    g.n4 = g.b4 = n4;
    if (bucket_elems > 0) g.b4 = ((bucket_elems / 4 + pad - 1) / pad) * pad;
    else if (G > 1) g.b4 = ((n4 / kDefaultBuckets + pad - 1) / pad) * pad;
    if (g.b4 <= 0 || g.b4 > n4) g.b4 = n4;
    g.nb = g.b4 > 0 ? (n4 + g.b4 - 1) / g.b4 : 1;
    return g;
  }
  static BucketGrid whole(int64_t n4) { return {n4, 1, n4}; }
};

// ---------------------------------------------------------------------------
// A step's argument struct (SmaArgs, AvgArgs, SsgdArgs of sma_internal.h) over
// float4s [start4, start4 + len4) of every buffer.  A null `last` or `s[r]`
// stays null.
// ---------------------------------------------------------------------------
template <class Args>
auto advance_snapshots(Args &a, int64_t start4, int) -> decltype((void)a.s[0]) {
  for (int r = 0; r < a.nrep; ++r)
    if (a.s[r]) a.s[r] += start4;
}
template <class Args>
void advance_snapshots(Args &, int64_t, long) {}  // SsgdArgs has no snapshots

template <class Args>
Args range_of(const Args &a, int64_t start4, int64_t len4) {
  Args b = a;
  advance_snapshots(b, start4, 0);
  for (int r = 0; r < b.nrep; ++r) b.w[r] += start4;
  b.z += start4;
  if (b.last) b.last += start4;
  b.acc += start4;
  b.D += start4;
  b.n4 = len4;
  return b;
}

// Caller-owned buffers of n floats whose first n4b float4s are the bulk: the
// elements past it, done by extra workgroups of the launch that covers the
// buffers' end; float indices relative to pointers advanced by start4 float4s.
template <class Args>
Args with_tail(Args a, int64_t n4b, int64_t n, int64_t start4) {
  a.tail_lo = (n4b - start4) * 4;
  a.tail_hi = n - start4 * 4;
  return a;
}

// ---------------------------------------------------------------------------
// The order.
// ---------------------------------------------------------------------------
#define CBX_LANE_TRY(expr)   \
  do {                       \
    int rc_ = (expr);        \
    if (rc_ < 0) return rc_; \
  } while (0)

// The all-reduce of bucket b on every lane, in one group.
template <class Lanes, class Begin, class End>
int all_reduce_group(Lanes &lanes, const Bucket &b, bool on_comm, Begin group_begin, End group_end) {
  CBX_LANE_TRY(group_begin());
  for (auto &l : lanes) {
    CBX_LANE_TRY(l.select());
    CBX_LANE_TRY(l.all_reduce(b, on_comm));
  }
  CBX_LANE_TRY(group_end());
  return 0;
}

template <class Lanes, class Begin, class End>
int accumulate_reduce_apply(Lanes &lanes, const BucketGrid &g, Begin group_begin, End group_end) {
  const bool piped = g.nb > 1;
  // Kernel B of bucket b on every lane, once its all-reduce has landed.
  auto apply = [&](int64_t b) -> int {
    for (auto &l : lanes) {
      CBX_LANE_TRY(l.select());
      if (piped) CBX_LANE_TRY(l.wait_r(b));
      CBX_LANE_TRY(l.launch_b(g.bucket(b)));
    }
    return 0;
  };
  for (int64_t b = 0; b < g.nb; ++b) {
    for (auto &l : lanes) {
      CBX_LANE_TRY(l.select());
      CBX_LANE_TRY(l.launch_a(g.bucket(b)));
      if (piped) {
        CBX_LANE_TRY(l.record_a(b));
        CBX_LANE_TRY(l.wait_a(b));
      }
    }
    CBX_LANE_TRY(all_reduce_group(lanes, g.bucket(b), piped, group_begin, group_end));
    if (!piped) continue;
    for (auto &l : lanes) {
      CBX_LANE_TRY(l.select());
      CBX_LANE_TRY(l.record_r(b));
    }
    if (b >= 1) CBX_LANE_TRY(apply(b - 1));
  }
  return apply(g.nb - 1);
}

// `collective` false: no all-reduce at all (one rank, or a step that is not
// split: K reads D = acc), K of every bucket in order.
template <class Lanes, class Begin, class End>
int reduce_apply(Lanes &lanes, const BucketGrid &g, bool collective, Begin group_begin, End group_end) {
  const bool piped = collective && g.nb > 1;
  if (piped)
    for (auto &l : lanes) {  // everything accumulated into acc so far, in stream order
      CBX_LANE_TRY(l.select());
      CBX_LANE_TRY(l.record_a(0));
      CBX_LANE_TRY(l.wait_a(0));
    }
  for (int64_t b = 0; b < g.nb; ++b) {
    if (collective) CBX_LANE_TRY(all_reduce_group(lanes, g.bucket(b), piped, group_begin, group_end));
    for (auto &l : lanes) {
      CBX_LANE_TRY(l.select());
      if (piped) {
        CBX_LANE_TRY(l.record_r(b));
        CBX_LANE_TRY(l.wait_r(b));
      }
      CBX_LANE_TRY(l.launch_k(g.bucket(b)));
    }
  }
  return 0;
}

#undef CBX_LANE_TRY

}  // namespace cbx::host
