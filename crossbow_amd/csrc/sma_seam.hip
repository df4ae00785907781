// sma_seam.hip -- the synchronisation steps over buffers the CALLER owns, for
// a Crossbow build that keeps its own model manager, model buffers and task
// side (modelmanager.c, model.c, executioncontext.c) and replaces only these
// function bodies:
//   crossbowSynchronisationSMA (clib-multigpu/synch/sma.c:233-248 -> :13-231)
//   crossbowKernelOptimiserSMA (kernels/optimisers/sma.cu:3-100)
//   (the two in one launch for a tau = 1 build: cbx_sma_plan_step_and_optimise)
//   crossbowSynchronisationSynchronousSGD (synch/synchronoussgd.c:13-106)
//   crossbowKernelOptimiserSynchronousSGD (kernels/optimisers/synchronoussgd.cu:3-56)
//   crossbowSynchronisationSynchronousElasticAveragingSGD
//     (synch/synchronouseamsgd.c:307 -> :5-101, :106-305)
//   crossbowSynchronisationPolyakRuppert (synch/polyakruppert.c:319 -> :5-138, :140-317)
//   crossbowCudnnBatchNormParamsSynchroniseEstimatedMeanAndVariable
//     (cudnn/cudnnbatchnormparams.c:157-222)
//
// The context API (context.hip) owns an arena whose buffers are padded to
// whole kernel trips; the reference's buffers hold exactly `elements` floats.
// So every launch here runs the bulk of the buffers through the same float4
// kernels (n4b float4s, a multiple of kTailQuantum4) and the last < 4 *
// kTailQuantum4 elements on extra workgroups of the same launch, one float per
// lane (the kernels' TAIL instantiations, sma_kernels.hip), with the same fma
// sequence per element: the results equal the context path's and the
// oracle's bit for bit.
//
// The plan owns what the step needs beyond the caller's buffers: the
// accumulator and the all-reduced difference (base->gradient and base->diff
// in the reference, sma.c:66,82) with the 256-byte control block that carries
// the Phase-D request count through the all-reduce, and -- unless the caller
// hands over its own (executioncontext.c:185-201) -- the RCCL communicators.
//
// With several ranks the SMA, averaging and S-SGD steps are bucketed: each
// supplies its lanes (PlanLane) and bucket_pipeline.h holds the order in
// which they are enqueued, its diagrams, and the bucket geometry.
#include "context_internal.h"
#include "optimise_plan.h"
#include "task_ssgd_internal.h"

using namespace cbx::host;

namespace {

bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

int cus_of_current_device(int *cus) {
  int dev = 0;
  HIP_TRY(hipGetDevice(&dev));
  static std::atomic<int> cache[cbx::kMaxDevices * 4] = {};
  if (dev >= 0 && dev < (int)(sizeof(cache) / sizeof(cache[0])) && cache[dev].load(std::memory_order_relaxed) > 0) {
    *cus = cache[dev].load(std::memory_order_relaxed);
    return CBX_OK;
  }
  int n = 0;
  HIP_TRY(hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev));
  if (dev >= 0 && dev < (int)(sizeof(cache) / sizeof(cache[0]))) cache[dev].store(n, std::memory_order_relaxed);
  *cus = n;
  return CBX_OK;
}

// Largest prefix of an n-float buffer that the float4 kernels cover without
// bounds checks, in float4s.  Their loops need whole waves' chunks (64 lanes
// x unroll float4s, every launch shape here has unroll <= 4); bucket starts
// stay on kPadFloat4.  A smaller tail is fewer scalar workgroups: ResNet-50's
// n = 25,557,032 leaves 40 elements (2,088 at kPadFloat4 granularity, whose
// tail workgroups cost ~7 us per fused step on separately allocated buffers:
// scripts/seam_layout_ab.py, profiles/r02/seam_layout_trace/).
constexpr int64_t kTailQuantum4 = 256;
static_assert(cbx::kPadFloat4 % kTailQuantum4 == 0, "bucket starts must stay on whole chunks");
int64_t bulk_float4s(int64_t n) { return (n / 4) / kTailQuantum4 * kTailQuantum4; }

}  // namespace

struct cbx_sma_plan {
  static constexpr int kClipSlots = 64;
  struct Dev {
    int hip_id = 0;
    int num_cus = 256;
    ncclComm_t comm = nullptr;
    bool own_comm = false;
    char *scratch = nullptr;  // [ctrl | acc (padded)] [ctrl | D (padded)]
    float *acc_ctrl = nullptr;
    float *D_ctrl = nullptr;
    // Bucketed pipeline (G > 1): the all-reduces run on this stream beside
    // kernel A of the next bucket; per bucket, kernel A done / all-reduce done.
    hipStream_t comm_stream = nullptr;
    std::vector<hipEvent_t> ev_a, ev_r;
    int global = 0;  // rank in the communicator (0: the default device)
    // Batch-norm statistics averaging: segment table and packed scratch.
    cbx::BnSegment *bn_table = nullptr;
    size_t bn_table_bytes = 0;
    float *bn_scratch = nullptr;
    size_t bn_scratch_bytes = 0;
    cbx::StatsScratch stats;  // cbx_sma_plan_buffer_stats: piece table, slab, results
    cbx::VarTables var_tables;  // cbx_sma_plan_set_variables: chunk table, bounds, multipliers
    // cbx_sma_plan_optimise_clipped: record and slab per slot, allocated on a
    // slot's first use (clip_mu held).
    cbx::ClipScratch clip[kClipSlots];
  };
  std::mutex clip_mu;
  int clip_norm_policy = cbx::clip_norm_policy();
  std::vector<uint32_t> var_bounds;  // cbx_sma_plan_set_variables: nvars + 1 running offsets (empty: not set)
  std::vector<Dev> devs;
  int64_t n = 0;
  int64_t n4b = 0;  // bulk float4s
  int ranks = 1;    // ranks of the communicator (1: no collective)
  int buckets = 0;  // G > 1: 0 = kDefaultBuckets, 1 = in order on the caller's stream
  cbx::LaunchConfig cfg;
  cbx::LaunchConfig apply_cfg = cbx::sma_apply_launch_config();
  cbx::LaunchConfig ssgd_apply_cfg = cbx::ssgd_apply_launch_config();
  cbx::LaunchConfig avg_cfg = cbx::averaging_launch_config();  // cbx_ea_plan_step / cbx_pr_plan_step: fused and kernel A
  cbx::LaunchConfig task_barrier_cfg = cbx::task_barrier_launch_config();  // cbx_sma_plan_step_and_optimise
  // cbx_sma_plan_set_timing: the one-rank fused launches stamp their own start
  // and stop into a ring of kTimedSteps event pairs (no marker packets).
  static constexpr int kTimedSteps = 256;
  bool timing = false;
  std::vector<std::pair<hipEvent_t, hipEvent_t>> timed;
  int64_t timed_steps = 0;  // launches stamped since timing was switched on
  cbx::Timing next_timing() {
    if (!timing) return {};
    const auto &e = timed[(size_t)(timed_steps++ % kTimedSteps)];
    return {e.first, e.second};
  }
};

namespace {

int ensure_pipeline(cbx_sma_plan *p, int64_t nb) {
  for (auto &d : p->devs) {
    HIP_TRY(hipSetDevice(d.hip_id));
    if (!d.comm_stream) HIP_TRY(hipStreamCreateWithFlags(&d.comm_stream, hipStreamNonBlocking));
    while ((int64_t)d.ev_a.size() < nb) {
      hipEvent_t a, r;
      HIP_TRY(hipEventCreateWithFlags(&a, hipEventDisableTiming));
      HIP_TRY(hipEventCreateWithFlags(&r, hipEventDisableTiming));
      d.ev_a.push_back(a);
      d.ev_r.push_back(r);
    }
  }
  return CBX_OK;
}

// A lane of a bucketed step over the caller's buffers (bucket_pipeline.h holds
// the order and the diagrams): the plan's device k, the caller's stream, and
// the all-reduce of `src` into the plan's D.  The tail rides the last bucket:
// its launches take it (bucket_args) and its all-reduce extends to n.
struct PlanLane : PipelineLane {
  cbx_sma_plan *p;
  PlanLane(cbx_sma_plan *plan, int k, void *const *streams, float *src, bool ctrl)
      : PipelineLane{plan->devs[k].hip_id, plan->devs[k].num_cus, static_cast<hipStream_t>(streams[k]),
                     plan->devs[k].comm_stream, plan->devs[k].ev_a, plan->devs[k].ev_r, plan->devs[k].comm, src,
                     plan->devs[k].D_ctrl + cbx::kCtrlFloats, plan->n, ctrl},
        p(plan) {}
  template <class Args>
  Args bucket_args(const Args &a, const Bucket &b) const {
    const Args r = range_of(a, b.start4, b.len4);
    return b.last ? with_tail(r, p->n4b, p->n, b.start4) : r;
  }
};

struct SmaPlanLane : PlanLane {
  const cbx::SmaArgs &args;
  bool mom;
  int launch_a(const Bucket &b) {
    HIP_TRY(cbx::launch_sma_accumulate(bucket_args(args, b), b.first, on_device(p->cfg), stream));
    return CBX_OK;
  }
  int launch_b(const Bucket &b) {
    HIP_TRY(cbx::launch_sma_apply(bucket_args(args, b), mom, on_device(p->apply_cfg), stream));
    return CBX_OK;
  }
};

struct AveragingPlanLane : PlanLane {
  const cbx::AvgArgs &args;
  cbx::AvgModel model;
  int launch_a(const Bucket &b) {
    HIP_TRY(cbx::launch_averaging_accumulate(model, bucket_args(args, b), on_device(p->avg_cfg), stream));
    return CBX_OK;
  }
  int launch_b(const Bucket &b) {
    HIP_TRY(cbx::launch_averaging_apply(model, bucket_args(args, b), on_device(p->apply_cfg), stream));
    return CBX_OK;
  }
};

struct SsgdPlanLane : PlanLane {
  const cbx::SsgdArgs &args;
  int launch_k(const Bucket &b) {
    HIP_TRY(cbx::launch_ssgd_apply(bucket_args(args, b), on_device(p->ssgd_apply_cfg), stream));
    return CBX_OK;
  }
};

// Per device: its locked replicas from `first` on, in id order (sma.c:69-73,
// common.c:208).  Each one's device index and buffers are checked (`s` null:
// the step takes no snapshots; `bad_buffers`: the step's refusal, with the
// replica's id), its w is appended to its device's arguments, and `append`
// adds what else the step keeps of replica `id` at slot a.nrep.
template <class Args, class Append>
int gather_replicas(std::vector<Args> &args, int first, int nreplicas, const int *replica_device, const int *locked,
                    float *const *w, const float *const *s, const char *bad_buffers, Append append) {
  const int G = (int)args.size();
  for (int id = first; id < nreplicas; ++id) {
    if (!locked[id]) continue;
    const int k = replica_device[id];
    if (k < 0 || k >= G) return fail(CBX_ERR_INVALID, "replica %d on device %d of %d", id, k, G);
    if (!w[id] || !aligned16(w[id]) || (s && (!s[id] || !aligned16(s[id])))) return fail(CBX_ERR_INVALID, bad_buffers, id);
    Args &a = args[k];
    if (a.nrep >= cbx::kMaxReplicas)
      return fail(CBX_ERR_UNSUPPORTED, "more than %d locked replicas on one device", cbx::kMaxReplicas);
    a.w[a.nrep] = reinterpret_cast<cbx::v4f *>(w[id]);
    append(a, id);
    ++a.nrep;
  }
  return CBX_OK;
}
const char *const kBadReplicaBuffers = "replica %d: buffers must be non-null and 16-byte aligned";

// The elastic-averaging (synch/synchronouseamsgd.c:5-101, :106-305) and
// Polyak-Ruppert (synch/polyakruppert.c:5-138, :140-317) barriers over the
// caller's buffers: the context's averaging_step (sync_steps.hip) with the
// plan's scratch for acc / D.  One rank: the fused kernel.  Several: kernel A,
// the all-reduce of acc into D, kernel B, bucketed as cbx_sma_plan_step is,
// with no control block.  Everything is validated before the first launch.
// Returns the raised copy flags among the locked replicas from `first` on
// (Polyak-Ruppert; 0 for elastic averaging).
int averaging_plan_step(cbx_sma_plan *p, const char *what, bool polyak, void *const *streams, float *const *z,
                        float *const *last, int nreplicas, const int *replica_device, float *const *w,
                        const float *const *s, const int *locked, const int *copy, float alpha, int clock,
                        int first) {
  if (!p) return fail(CBX_ERR_INVALID, "null plan");
  const int G = (int)p->devs.size();
  // synchronouseamsgd.c:55 reads the replica's data on one device, :184 its snapshot on several
  const cbx::AvgModel model = polyak ? cbx::kPolyak : (p->ranks > 1 ? cbx::kElasticS : cbx::kElasticW);
  const bool snap = model == cbx::kElasticS;
  if (!streams || !z || nreplicas < 0 ||
      (nreplicas > 0 && (!replica_device || !w || !locked || (polyak && !copy) || (snap && !s))))
    return fail(CBX_ERR_INVALID, "%s: missing arguments", what);
  if (polyak && clock < 0) return fail(CBX_ERR_INVALID, "%s: clock %d is negative", what, clock);  // polyakruppert.c:16
  if (first < 0 || first > nreplicas) return fail(CBX_ERR_INVALID, "first replica %d out of range", first);
  std::vector<cbx::AvgArgs> args(G);
  for (int k = 0; k < G; ++k) {
    std::memset(&args[k], 0, sizeof(cbx::AvgArgs));
    float *l = polyak && last ? last[k] : nullptr;  // model.c:116-120: base->last may not exist
    if (!z[k] || !aligned16(z[k]) || !aligned16(l))
      return fail(CBX_ERR_INVALID, "device %d: base buffers must be non-null and 16-byte aligned", k);
  }
  int copies = 0;
  TRY(gather_replicas(args, first, nreplicas, replica_device, locked, w, snap ? s : nullptr, kBadReplicaBuffers,
                      [&](cbx::AvgArgs &a, int id) {
                        if (snap) a.s[a.nrep] = reinterpret_cast<const cbx::v4f *>(s[id]);
                        if (polyak && copy[id]) {  // polyakruppert.c:126
                          a.copy_mask |= 1ull << a.nrep;
                          ++copies;
                        }
                      }));
  const BucketGrid grid = BucketGrid::by_count(p->n4b, p->buckets);
  if (p->ranks > 1 && grid.nb > 1) TRY(ensure_pipeline(p, grid.nb));
  std::vector<AveragingPlanLane> lanes;
  for (int k = 0; k < G; ++k) {
    auto &d = p->devs[k];
    cbx::AvgArgs &a = args[k];
    a.z = reinterpret_cast<cbx::v4f *>(z[k]);
    a.last = polyak && last ? reinterpret_cast<cbx::v4f *>(last[k]) : nullptr;
    a.acc = reinterpret_cast<cbx::v4f *>(d.acc_ctrl + cbx::kCtrlFloats);
    a.D = reinterpret_cast<const cbx::v4f *>(d.D_ctrl + cbx::kCtrlFloats);
    a.n4 = p->n4b;
    a.alpha = alpha;
    if (polyak) {
      a.scale = (float)(1.0 / (double)(float)nreplicas);      // polyakruppert.c:15
      a.running = (float)(1.0 / (double)(float)(clock + 1));  // :16
    }
    lanes.push_back({PlanLane(p, k, streams, d.acc_ctrl + cbx::kCtrlFloats, false), a, model});
  }
  if (p->ranks == 1) {
    PlanLane &l = lanes[0];
    TRY(l.select());
    HIP_TRY(cbx::launch_averaging_fused(model, with_tail(args[0], p->n4b, p->n, 0), l.on_device(p->avg_cfg), l.stream,
                                        p->next_timing()));
    return copies;
  }
  TRY(accumulate_reduce_apply(lanes, grid, group_begin, group_end));
  return copies;
}

}  // namespace

extern "C" {

int cbx_ea_plan_step(cbx_sma_plan *p, void *const *streams, float *const *z, int nreplicas, const int *replica_device,
                     float *const *w, const float *const *s, const int *locked, float alpha, int first) {
  TraceRange trace("cbx_ea_plan_step");
  const int rc = averaging_plan_step(p, "cbx_ea_plan_step", false, streams, z, nullptr, nreplicas, replica_device, w,
                                     s, locked, nullptr, alpha, 0, first);
  return rc < 0 ? rc : CBX_OK;
}

int cbx_pr_plan_step(cbx_sma_plan *p, void *const *streams, float *const *z, float *const *last, int nreplicas,
                     const int *replica_device, float *const *w, const int *locked, const int *copy, float alpha,
                     int clock, int first) {
  TraceRange trace("cbx_pr_plan_step");
  return averaging_plan_step(p, "cbx_pr_plan_step", true, streams, z, last, nreplicas, replica_device, w, nullptr,
                             locked, copy, alpha, clock, first);
}

int cbx_sma_plan_free(cbx_sma_plan *p) {
  if (!p) return CBX_OK;
  for (auto &d : p->devs) {
    (void)hipSetDevice(d.hip_id);
    (void)hipDeviceSynchronize();
    if (d.own_comm && d.comm) (void)ncclCommDestroy(d.comm);
    if (d.scratch) (void)hipFree(d.scratch);
    if (d.bn_table) (void)hipFree(d.bn_table);
    if (d.bn_scratch) (void)hipFree(d.bn_scratch);
    cbx::stats_free(d.stats);
    cbx::var_tables_free(d.var_tables);
    for (cbx::ClipScratch &cs : d.clip) cbx::clip_scratch_free(cs);
    for (hipEvent_t e : d.ev_a) (void)hipEventDestroy(e);
    for (hipEvent_t e : d.ev_r) (void)hipEventDestroy(e);
    if (d.comm_stream) (void)hipStreamDestroy(d.comm_stream);
  }
  for (auto &e : p->timed) {
    (void)hipEventDestroy(e.first);
    (void)hipEventDestroy(e.second);
  }
  delete p;
  return CBX_OK;
}

int cbx_sma_plan_set_timing(cbx_sma_plan *p, int on) {
  if (!p) return fail(CBX_ERR_INVALID, "null plan");
  if (on && p->timed.empty()) {
    HIP_TRY(hipSetDevice(p->devs[0].hip_id));
    for (int k = 0; k < cbx_sma_plan::kTimedSteps; ++k) {
      hipEvent_t a, b;
      HIP_TRY(hipEventCreate(&a));
      HIP_TRY(hipEventCreate(&b));
      p->timed.emplace_back(a, b);
    }
  }
  p->timing = on != 0;
  p->timed_steps = 0;
  return CBX_OK;
}

int cbx_sma_plan_timing_history(cbx_sma_plan *p, float *ms, int count) {
  if (!p) return fail(CBX_ERR_INVALID, "null plan");
  if (!ms || count < 0) return fail(CBX_ERR_INVALID, "cbx_sma_plan_timing_history: bad arguments");
  const int64_t have = std::min<int64_t>(p->timed_steps, cbx_sma_plan::kTimedSteps);
  const int64_t take = std::min<int64_t>(count, have);
  for (int64_t k = 0; k < take; ++k) {  // oldest first
    const auto &e = p->timed[(size_t)((p->timed_steps - take + k) % cbx_sma_plan::kTimedSteps)];
    HIP_TRY(hipEventSynchronize(e.second));
    HIP_TRY(hipEventElapsedTime(&ms[k], e.first, e.second));
  }
  return (int)take;
}

int cbx_sma_plan_create(cbx_sma_plan **out, const int *devices, int ndevices, long long elements,
                        void *const *comms) {
  if (!out || !devices || ndevices <= 0 || ndevices > cbx::kMaxDevices)
    return fail(CBX_ERR_INVALID, "cbx_sma_plan_create: need 1..%d devices", cbx::kMaxDevices);
  *out = nullptr;
  // model.h:35 `int bytes`; the kernels address a buffer with 32-bit byte offsets.
  if (elements <= 0 || elements * 4 + 4096 >= (1ll << 32))
    return fail(CBX_ERR_INVALID, "cbx_sma_plan_create: %lld elements out of range", elements);
  cbx_sma_plan *p = new cbx_sma_plan();
  p->n = elements;
  p->n4b = bulk_float4s(elements);
  p->devs.resize(ndevices);
  const int64_t pad = cbx::kPadFloat4;
  const int64_t n4 = ((elements + 3) / 4 + pad - 1) / pad * pad;
  const size_t half = ((size_t)cbx::kCtrlFloats * 4 + (size_t)n4 * 16 + 255) / 256 * 256;
  for (int k = 0; k < ndevices; ++k) {
    auto &d = p->devs[k];
    int rc = probe_device(devices[k], &d.num_cus);
    if (rc < 0) {
      std::string msg = g_last_error;
      cbx_sma_plan_free(p);
      return fail(rc, "%s", msg.c_str());
    }
    d.hip_id = devices[k];
    hipError_t e = hipMalloc(reinterpret_cast<void **>(&d.scratch), 2 * half);
    if (e == hipSuccess) e = hipMemset(d.scratch, 0, 2 * half);
    if (e != hipSuccess) {
      cbx_sma_plan_free(p);
      return fail(CBX_ERR_HIP, "plan scratch of %zu bytes: %s", 2 * half, hipGetErrorString(e));
    }
    d.acc_ctrl = reinterpret_cast<float *>(d.scratch);
    d.D_ctrl = reinterpret_cast<float *>(d.scratch + half);
  }
  if (comms) {
    for (int k = 0; k < ndevices; ++k) {
      p->devs[k].comm = static_cast<ncclComm_t>(comms[k]);
      if (!p->devs[k].comm) {
        cbx_sma_plan_free(p);
        return fail(CBX_ERR_INVALID, "cbx_sma_plan_create: null communicator for device %d", k);
      }
    }
    int count = 0;
    ncclResult_t r = ncclCommCount(p->devs[0].comm, &count);
    for (int k = 0; r == ncclSuccess && k < ndevices; ++k) r = ncclCommUserRank(p->devs[k].comm, &p->devs[k].global);
    if (r != ncclSuccess) {
      cbx_sma_plan_free(p);
      return fail(CBX_ERR_RCCL, "ncclCommCount / ncclCommUserRank: %s", ncclGetErrorString(r));
    }
    p->ranks = count;
  } else if (ndevices > 1) {
    // executioncontext.c:185-201
    std::vector<ncclComm_t> cs(ndevices);
    ncclResult_t r = ncclCommInitAll(cs.data(), ndevices, devices);
    if (r != ncclSuccess) {
      cbx_sma_plan_free(p);
      return fail(CBX_ERR_RCCL, "ncclCommInitAll: %s", ncclGetErrorString(r));
    }
    for (int k = 0; k < ndevices; ++k) {
      p->devs[k].comm = cs[k];
      p->devs[k].own_comm = true;
      p->devs[k].global = k;
    }
    p->ranks = ndevices;
  }
  if (p->ranks < ndevices) {
    cbx_sma_plan_free(p);
    return fail(CBX_ERR_INVALID, "communicator of %d ranks for %d local devices", p->ranks, ndevices);
  }
  *out = p;
  return CBX_OK;
}

int cbx_sma_plan_step(cbx_sma_plan *p, void *const *streams, float *const *z, float *const *last, int nreplicas,
                      const int *replica_device, float *const *w, const float *const *s, const int *locked,
                      const int *copy, float alpha, float momentum, int first) {
  TraceRange trace("cbx_sma_plan_step");
  if (!p) return fail(CBX_ERR_INVALID, "null plan");
  const int G = (int)p->devs.size();
  if (!streams || !z || nreplicas < 0 || (nreplicas > 0 && (!replica_device || !w || !s || !locked || !copy)))
    return fail(CBX_ERR_INVALID, "cbx_sma_plan_step: missing arguments");
  if (first < 0 || first > nreplicas) return fail(CBX_ERR_INVALID, "first replica %d out of range", first);
  const bool mom = momentum > 0.0f;  // sma.c:150: base momentum forced to 0.9 when > 0
  if (mom && !last) return fail(CBX_ERR_INVALID, "base momentum > 0 needs the base models' last buffers");
  std::vector<cbx::SmaArgs> args(G);
  int copies_total = 0;
  for (int k = 0; k < G; ++k) {
    std::memset(&args[k], 0, sizeof(cbx::SmaArgs));
    if (!z[k] || !aligned16(z[k]) || (mom && (!last[k] || !aligned16(last[k]))))
      return fail(CBX_ERR_INVALID, "device %d: base buffers must be non-null and 16-byte aligned", k);
  }
  TRY(gather_replicas(args, first, nreplicas, replica_device, locked, w, s, kBadReplicaBuffers,
                      [&](cbx::SmaArgs &a, int id) {
                        a.s[a.nrep] = reinterpret_cast<const cbx::v4f *>(s[id]);
                        if (copy[id]) {
                          a.copies += 1.0f;  // sma.c:113-120
                          ++copies_total;
                        }
                      }));
  // G > 1: kernel A, the grouped all-reduce of the control block + acc
  // (common.c:14-54), kernel B.  One bucket: everything in order on each
  // device's stream, the reference's structure.  nb > 1 buckets (the
  // default): the all-reduce of bucket k runs on a stream of the plan's,
  // beside kernel A of bucket k+1 (accumulate_reduce_apply, bucket_pipeline.h).
  // The control block rides bucket 0; the tail rides the last bucket.
  const BucketGrid grid = BucketGrid::by_count(p->n4b, p->buckets);
  if (p->ranks > 1 && grid.nb > 1) TRY(ensure_pipeline(p, grid.nb));
  std::vector<SmaPlanLane> lanes;
  for (int k = 0; k < G; ++k) {
    auto &d = p->devs[k];
    cbx::SmaArgs &a = args[k];
    a.z = reinterpret_cast<cbx::v4f *>(z[k]);
    a.last = mom ? reinterpret_cast<cbx::v4f *>(last[k]) : nullptr;
    a.acc = reinterpret_cast<cbx::v4f *>(d.acc_ctrl + cbx::kCtrlFloats);
    a.D = reinterpret_cast<const cbx::v4f *>(d.D_ctrl + cbx::kCtrlFloats);
    a.ctrl_out = d.acc_ctrl;
    a.ctrl_in = d.D_ctrl;
    a.n4 = p->n4b;
    a.alpha = alpha;  // sma.c:33
    lanes.push_back({PlanLane(p, k, streams, d.acc_ctrl + cbx::kCtrlFloats, true), a, mom});
  }
  if (p->ranks == 1) {
    // One GPU: the all-reduce of one buffer is the identity, so Phases A + C
    // (+ D) fuse into one pass, as in the context's G = 1 step.
    PlanLane &l = lanes[0];
    TRY(l.select());
    HIP_TRY(cbx::launch_sma_fused(with_tail(args[0], p->n4b, p->n, 0), mom, copies_total > 0, l.on_device(p->cfg),
                                  l.stream, p->next_timing()));
    return copies_total > 0 ? 1 : 0;
  }
  TRY(accumulate_reduce_apply(lanes, grid, group_begin, group_end));
  return copies_total > 0 ? 1 : 0;
}

// crossbowKernelOptimiserSMA of every stepping replica and
// crossbowSynchronisationSMA in one launch over the caller's buffers: the
// context's cbx_step_and_synchronise (context.hip) with the caller's rates,
// flags and stream order.  One device, one rank: kernel A of the split path is
// not fused.  The bulk runs the context's float4 loop, the elements past it the
// kernel's TAIL workgroups (task_barrier_kernels.hip).  Everything is
// validated before the launch; the plan queues no wait of its own.
// SeamVariables: cbx_sma_plan_step_and_optimise_variables, the same call over the
// plan's variable table (task_barrier_variables_kernels.hip).  SeamClipped:
// cbx_sma_plan_step_and_optimise_clipped, with every stepping replica's norm
// pass over its slot's scratch on streams[0] in front of the launch and the
// clipped step inside it (task_barrier_clipped_kernels.hip).
// SeamClippedVariables: cbx_sma_plan_step_and_optimise_clipped_variables, both:
// the norm passes, then the kernel that clips and reads the plan's variable
// table (task_barrier_clipped_variables_kernels.hip); when nobody steps, the
// per-variable launch.
namespace {
int clip_slot(cbx_sma_plan *p, const char *what, int k, int slot, cbx::ClipScratch **out);
enum SeamMode { SeamPlain, SeamVariables, SeamClipped, SeamClippedVariables };
struct SeamClip {
  const int *slot = nullptr;
  float max_norm = 0.0f;
  int skip_nonfinite = 0;
};
}  // namespace

static int plan_step_and_optimise(cbx_sma_plan *p, void *const *streams, float *const *z, float *const *last,
                                  int nreplicas, const int *replica_device, float *const *w, float *const *s,
                                  float *const *g, float *const *rlast, const int *locked, const int *copy,
                                  const int *step, const float *learning_rate, float alpha, float momentum,
                                  float replica_momentum, float weight_decay, int first, unsigned flags,
                                  SeamMode mode, const SeamClip &clip = SeamClip()) {
  const bool variables = mode == SeamVariables || mode == SeamClippedVariables;
  const bool clipped = mode == SeamClipped || mode == SeamClippedVariables;
  const char *me = mode == SeamClippedVariables ? "cbx_sma_plan_step_and_optimise_clipped_variables"
                   : clipped                    ? "cbx_sma_plan_step_and_optimise_clipped"
                   : variables                  ? "cbx_sma_plan_step_and_optimise_variables"
                                                : "cbx_sma_plan_step_and_optimise";
  TraceRange trace(me);
  if (!p) return fail(CBX_ERR_INVALID, "null plan");
  if (variables && p->var_bounds.empty()) return fail(CBX_ERR_STATE, "%s before cbx_sma_plan_set_variables", me);
  if (clipped && (!(clip.max_norm >= 0.0f) || std::isinf(clip.max_norm)))
    return fail(CBX_ERR_INVALID, "%s: max_norm %g is negative, NaN or infinite", me, (double)clip.max_norm);
  if (clipped && clip.skip_nonfinite != 0 && clip.skip_nonfinite != 1)
    return fail(CBX_ERR_INVALID, "%s: skip_nonfinite %d is neither 0 nor 1", me, clip.skip_nonfinite);
  if (!streams || !z || nreplicas < 0 ||
      (nreplicas > 0 && (!replica_device || !w || !s || !g || !locked || !copy || !step || !learning_rate)))
    return fail(CBX_ERR_INVALID, "%s: missing arguments", me);
  if (flags & ~CBX_STEP_DISCARD_TASK_OUTPUTS) return fail(CBX_ERR_INVALID, "%s: unknown flag bits 0x%x", me, flags);
  if (first < 0 || first > nreplicas) return fail(CBX_ERR_INVALID, "%s: first replica %d out of range", me, first);
  const bool keep = (flags & CBX_STEP_DISCARD_TASK_OUTPUTS) == 0;
  const bool mom = momentum > 0.0f;           // sma.c:150: base momentum forced to 0.9 when > 0
  const bool rmom = replica_momentum > 0.0f;  // sma.cu:45
  if (mom && !last) return fail(CBX_ERR_INVALID, "%s: base momentum > 0 needs the base model's last buffer", me);
  for (int id = 0; id < nreplicas; ++id) {
    if (!step[id]) continue;
    if (!locked[id]) return fail(CBX_ERR_INVALID, "%s: stepping replica %d is not locked for this barrier", me, id);
    if (id < first) return fail(CBX_ERR_INVALID, "%s: stepping replica %d is below the first replica %d", me, id, first);
    if (rmom && !rlast) return fail(CBX_ERR_INVALID, "%s: replica momentum > 0 needs the replicas' last buffers", me);
  }
  if (p->devs.size() != 1 || p->ranks != 1)
    return fail(CBX_ERR_UNSUPPORTED, "%s: a plan of %d devices and %d ranks; the task steps are fused into the one-GPU "
                "barrier only, not into kernel A of the split path", me, (int)p->devs.size(), p->ranks);
  if (!z[0] || !aligned16(z[0]) || (mom && (!last[0] || !aligned16(last[0]))))
    return fail(CBX_ERR_INVALID, "%s: base buffers must be non-null and 16-byte aligned", me);
  cbx::TaskBarrierArgs a;
  std::memset(&a, 0, sizeof(a));
  int copies = 0, participating = 0;
  bool steps = false;
  int slot_of[cbx::kMaxReplicas];  // clipped: the slot of participating replica k, or -1
  uint64_t slots_taken = 0;
  static_assert(cbx_sma_plan::kClipSlots <= 64, "one bit per slot");
  for (int id = first; id < nreplicas; ++id) {  // increasing id order, sma.c:69
    if (!locked[id]) continue;
    if (replica_device[id] != 0) return fail(CBX_ERR_INVALID, "%s: replica %d on device %d of 1", me, id, replica_device[id]);
    const bool st = step[id] != 0;
    if (!w[id] || !aligned16(w[id])) return fail(CBX_ERR_INVALID, "%s: replica %d: w must be non-null and 16-byte aligned", me, id);
    // a stepping replica's s is only written, and not at all under the discard flag
    if ((!s[id] && (!st || keep)) || !aligned16(s[id]))
      return fail(CBX_ERR_INVALID, "%s: replica %d: s must be non-null and 16-byte aligned", me, id);
    if (st && (!g[id] || !aligned16(g[id])))
      return fail(CBX_ERR_INVALID, "%s: stepping replica %d: g must be non-null and 16-byte aligned", me, id);
    if (st && rmom && (!rlast[id] || !aligned16(rlast[id])))
      return fail(CBX_ERR_INVALID, "%s: stepping replica %d: replica momentum > 0 needs a 16-byte aligned last buffer", me, id);
    if (clipped && st) {
      if (!clip.slot) return fail(CBX_ERR_INVALID, "%s: stepping replica %d without a slot list", me, id);
      const int sl = clip.slot[id];
      if (sl < 0 || sl >= cbx_sma_plan::kClipSlots)
        return fail(CBX_ERR_INVALID, "%s: stepping replica %d: slot %d out of range [0, %d)", me, id, sl,
                    cbx_sma_plan::kClipSlots);
      if ((slots_taken >> sl) & 1ull)
        return fail(CBX_ERR_INVALID, "%s: stepping replica %d: slot %d is another stepping replica's", me, id, sl);
      slots_taken |= 1ull << sl;
    }
    if (++participating > cbx::kMaxReplicas) continue;  // counted on, refused below
    const int k = a.nrep++;
    slot_of[k] = clipped && st ? clip.slot[id] : -1;
    a.w[k] = reinterpret_cast<cbx::v4f *>(w[id]);
    a.s[k] = reinterpret_cast<cbx::v4f *>(s[id]);
    if (st) {
      steps = true;
      a.step_mask |= 1ull << k;
      a.g[k] = reinterpret_cast<cbx::v4f *>(g[id]);
      a.last[k] = rmom ? reinterpret_cast<cbx::v4f *>(rlast[id]) : nullptr;
      a.rate[k] = -1.0f * learning_rate[id];  // sma.cu:43
    }
    if (copy[id]) ++copies;  // sma.c:113-120
  }
  if (participating > cbx::kMaxReplicas)
    return fail(CBX_ERR_UNSUPPORTED, "%s: %d participating replicas, more than %d on one device", me, participating,
                cbx::kMaxReplicas);
  a.z = reinterpret_cast<cbx::v4f *>(z[0]);
  a.blast = mom ? reinterpret_cast<cbx::v4f *>(last[0]) : nullptr;
  a.n4 = p->n4b;
  a.alpha = alpha;  // sma.c:33
  a.momentum = steps && rmom ? replica_momentum : 0.0f;
  a.wd = steps && weight_decay > 0.0f ? weight_decay : 0.0f;
  a.copy = copies > 0 ? 1 : 0;
  a.tail_lo = p->n4b * 4;  // the elements past the last whole chunk ride the same launch
  a.tail_hi = p->n;
  auto &d = p->devs[0];
  HIP_TRY(hipSetDevice(d.hip_id));
  cbx::LaunchConfig cfg = p->task_barrier_cfg;
  cfg.num_cus = d.num_cus;
  if (clipped && steps) {
    // The norm passes in id order on the launch's stream, each over its slot's
    // scratch (allocated on first use), as cbx_sma_plan_optimise_clipped runs
    // them: the records are the sequence's bits.  No wait is queued.
    cbx::ClipRecordPtrs records;
    std::memset(&records, 0, sizeof(records));
    cbx::ClipScratch *cs[cbx::kMaxReplicas] = {};
    for (int k = 0; k < a.nrep; ++k)  // every scratch before the first launch: a failed allocation bumps no counter
      if (slot_of[k] >= 0) TRY(clip_slot(p, me, 0, slot_of[k], &cs[k]));
    for (int k = 0; k < a.nrep; ++k) {
      if (!cs[k]) continue;
      HIP_TRY(cbx::launch_gradient_norm(reinterpret_cast<const float *>(a.g[k]), p->n, *cs[k], clip.max_norm,
                                        clip.skip_nonfinite == 1, p->clip_norm_policy,
                                        static_cast<hipStream_t>(streams[0])));
      records.p[k] = cs[k]->record();
    }
    if (variables)
      HIP_TRY(cbx::launch_task_barrier_clipped_variables(a, d.var_tables, records, keep, cfg,
                                                         static_cast<hipStream_t>(streams[0]), p->next_timing()));
    else
      HIP_TRY(cbx::launch_task_barrier_clipped(a, records, keep, cfg, static_cast<hipStream_t>(streams[0]),
                                               p->next_timing()));
  } else if (variables)
    HIP_TRY(cbx::launch_task_barrier_variables(a, d.var_tables, keep, cfg, static_cast<hipStream_t>(streams[0]),
                                               p->next_timing()));
  else
    HIP_TRY(cbx::launch_task_barrier(a, keep, cfg, static_cast<hipStream_t>(streams[0]), p->next_timing()));
  return copies > 0 ? 1 : 0;
}

int cbx_sma_plan_step_and_optimise(cbx_sma_plan *p, void *const *streams, float *const *z, float *const *last,
                                   int nreplicas, const int *replica_device, float *const *w, float *const *s,
                                   float *const *g, float *const *rlast, const int *locked, const int *copy,
                                   const int *step, const float *learning_rate, float alpha, float momentum,
                                   float replica_momentum, float weight_decay, int first, unsigned flags) {
  return plan_step_and_optimise(p, streams, z, last, nreplicas, replica_device, w, s, g, rlast, locked, copy, step,
                                learning_rate, alpha, momentum, replica_momentum, weight_decay, first, flags, SeamPlain);
}

int cbx_sma_plan_step_and_optimise_variables(cbx_sma_plan *p, void *const *streams, float *const *z,
                                             float *const *last, int nreplicas, const int *replica_device,
                                             float *const *w, float *const *s, float *const *g, float *const *rlast,
                                             const int *locked, const int *copy, const int *step,
                                             const float *learning_rate, float alpha, float momentum,
                                             float replica_momentum, float weight_decay, int first, unsigned flags) {
  return plan_step_and_optimise(p, streams, z, last, nreplicas, replica_device, w, s, g, rlast, locked, copy, step,
                                learning_rate, alpha, momentum, replica_momentum, weight_decay, first, flags,
                                SeamVariables);
}

int cbx_sma_plan_step_and_optimise_clipped(cbx_sma_plan *p, void *const *streams, float *const *z, float *const *last,
                                           int nreplicas, const int *replica_device, float *const *w, float *const *s,
                                           float *const *g, float *const *rlast, const int *locked, const int *copy,
                                           const int *step, const float *learning_rate, const int *slot,
                                           float max_norm, int skip_nonfinite, float alpha, float momentum,
                                           float replica_momentum, float weight_decay, int first, unsigned flags) {
  SeamClip clip;
  clip.slot = slot;
  clip.max_norm = max_norm;
  clip.skip_nonfinite = skip_nonfinite;
  return plan_step_and_optimise(p, streams, z, last, nreplicas, replica_device, w, s, g, rlast, locked, copy, step,
                                learning_rate, alpha, momentum, replica_momentum, weight_decay, first, flags,
                                SeamClipped, clip);
}

int cbx_sma_plan_step_and_optimise_clipped_variables(cbx_sma_plan *p, void *const *streams, float *const *z,
                                                     float *const *last, int nreplicas, const int *replica_device,
                                                     float *const *w, float *const *s, float *const *g,
                                                     float *const *rlast, const int *locked, const int *copy,
                                                     const int *step, const float *learning_rate, const int *slot,
                                                     float max_norm, int skip_nonfinite, float alpha, float momentum,
                                                     float replica_momentum, float weight_decay, int first,
                                                     unsigned flags) {
  SeamClip clip;
  clip.slot = slot;
  clip.max_norm = max_norm;
  clip.skip_nonfinite = skip_nonfinite;
  return plan_step_and_optimise(p, streams, z, last, nreplicas, replica_device, w, s, g, rlast, locked, copy, step,
                                learning_rate, alpha, momentum, replica_momentum, weight_decay, first, flags,
                                SeamClippedVariables, clip);
}

// The task steps of kernels/optimisers/synchronouseamsgd.cu of every stepping
// replica and the one-device elastic-averaging barrier
// (synch/synchronouseamsgd.c:42-90) in one launch over the caller's buffers:
// the context's cbx_step_and_synchronise_elastic (context.hip) with the
// caller's rates and stream order.  No `last`, `copy` or base momentum: the
// barrier has none.  The bulk runs the context's float4 loop, the elements past
// it the kernel's TAIL workgroups (task_elastic_kernels.hip).  Everything is
// validated before the launch; the plan queues no wait of its own.
// cbx_ea_plan_step_and_optimise_clipped_variables (`policies`) is the same call
// with two switches.  clip.slot != NULL: every stepping replica's norm pass
// over its slot's scratch on streams[0] in front of the launch, and the clipped
// step inside it, as SeamClipped above has them.  use_variables: the step reads
// the plan's variable table.  The kernel is the one of what is on
// (libcrossbow_sma_elastic_policies.so); with both off, or clipping alone and
// nobody stepping, it is the plain call's launch.
static int ea_plan_step_and_optimise(cbx_sma_plan *p, void *const *streams, float *const *z, int nreplicas,
                                     const int *replica_device, float *const *w, float *const *s, float *const *g,
                                     float *const *rlast, const int *locked, const int *step,
                                     const float *learning_rate, float alpha, float replica_momentum,
                                     float weight_decay, int first, unsigned flags, bool policies,
                                     const SeamClip &clip = SeamClip(), int use_variables = 0) {
  const char *me = policies ? "cbx_ea_plan_step_and_optimise_clipped_variables" : "cbx_ea_plan_step_and_optimise";
  const bool clipped = clip.slot != nullptr, variables = use_variables == 1;
  TraceRange trace(me);
  if (!p) return fail(CBX_ERR_INVALID, "null plan");
  if (use_variables != 0 && use_variables != 1)
    return fail(CBX_ERR_INVALID, "%s: use_variables %d is neither 0 nor 1", me, use_variables);
  if (variables && p->var_bounds.empty()) return fail(CBX_ERR_STATE, "%s with variables before cbx_sma_plan_set_variables", me);
  if (clipped && (!(clip.max_norm >= 0.0f) || std::isinf(clip.max_norm)))
    return fail(CBX_ERR_INVALID, "%s: max_norm %g is negative, NaN or infinite", me, (double)clip.max_norm);
  if (clipped && clip.skip_nonfinite != 0 && clip.skip_nonfinite != 1)
    return fail(CBX_ERR_INVALID, "%s: skip_nonfinite %d is neither 0 nor 1", me, clip.skip_nonfinite);
  if (!streams || !z || nreplicas < 0 || (nreplicas > 0 && (!replica_device || !w || !locked || !step)))
    return fail(CBX_ERR_INVALID, "%s: missing arguments", me);
  if (flags & ~CBX_STEP_DISCARD_TASK_OUTPUTS) return fail(CBX_ERR_INVALID, "%s: unknown flag bits 0x%x", me, flags);
  if (first < 0 || first > nreplicas) return fail(CBX_ERR_INVALID, "%s: first replica %d out of range", me, first);
  const bool keep = (flags & CBX_STEP_DISCARD_TASK_OUTPUTS) == 0;
  const bool rmom = replica_momentum > 0.0f;  // sma.cu:45
  for (int id = 0; id < nreplicas; ++id) {
    if (!step[id]) continue;
    if (!locked[id]) return fail(CBX_ERR_INVALID, "%s: stepping replica %d is not locked for this barrier", me, id);
    if (id < first) return fail(CBX_ERR_INVALID, "%s: stepping replica %d is below the first replica %d", me, id, first);
    if (!g || !learning_rate) return fail(CBX_ERR_INVALID, "%s: a stepping replica needs g and learning_rate", me);
    if (keep && !s) return fail(CBX_ERR_INVALID, "%s: a stepping replica whose outputs are kept needs s", me);
    if (rmom && !rlast) return fail(CBX_ERR_INVALID, "%s: replica momentum > 0 needs the replicas' last buffers", me);
  }
  if (p->devs.size() != 1 || p->ranks != 1)
    return fail(CBX_ERR_UNSUPPORTED, "%s: a plan of %d devices and %d ranks; the task steps are fused into the one-GPU "
                "barrier only, not into kernel A of the split path", me, (int)p->devs.size(), p->ranks);
  if (!z[0] || !aligned16(z[0])) return fail(CBX_ERR_INVALID, "%s: base buffers must be non-null and 16-byte aligned", me);
  cbx::TaskBarrierArgs a;
  std::memset(&a, 0, sizeof(a));
  int participating = 0;
  bool steps = false;
  int slot_of[cbx::kMaxReplicas];  // clipped: the slot of participating replica k, or -1
  uint64_t slots_taken = 0;
  for (int id = first; id < nreplicas; ++id) {  // increasing id order, synchronouseamsgd.c:46
    if (!locked[id]) continue;
    if (replica_device[id] != 0) return fail(CBX_ERR_INVALID, "%s: replica %d on device %d of 1", me, id, replica_device[id]);
    const bool st = step[id] != 0;
    if (!w[id] || !aligned16(w[id])) return fail(CBX_ERR_INVALID, "%s: replica %d: w must be non-null and 16-byte aligned", me, id);
    // s is only written, by a stepping replica whose outputs are kept
    if (st && keep && (!s[id] || !aligned16(s[id])))
      return fail(CBX_ERR_INVALID, "%s: stepping replica %d: s must be non-null and 16-byte aligned", me, id);
    if (st && (!g[id] || !aligned16(g[id])))
      return fail(CBX_ERR_INVALID, "%s: stepping replica %d: g must be non-null and 16-byte aligned", me, id);
    if (st && rmom && (!rlast[id] || !aligned16(rlast[id])))
      return fail(CBX_ERR_INVALID, "%s: stepping replica %d: replica momentum > 0 needs a 16-byte aligned last buffer", me, id);
    if (clipped && st) {
      const int sl = clip.slot[id];
      if (sl < 0 || sl >= cbx_sma_plan::kClipSlots)
        return fail(CBX_ERR_INVALID, "%s: stepping replica %d: slot %d out of range [0, %d)", me, id, sl,
                    cbx_sma_plan::kClipSlots);
      if ((slots_taken >> sl) & 1ull)
        return fail(CBX_ERR_INVALID, "%s: stepping replica %d: slot %d is another stepping replica's", me, id, sl);
      slots_taken |= 1ull << sl;
    }
    if (++participating > cbx::kMaxReplicas) continue;  // counted on, refused below
    const int k = a.nrep++;
    slot_of[k] = clipped && st ? clip.slot[id] : -1;
    a.w[k] = reinterpret_cast<cbx::v4f *>(w[id]);
    if (st) {
      steps = true;
      a.step_mask |= 1ull << k;
      a.s[k] = keep ? reinterpret_cast<cbx::v4f *>(s[id]) : nullptr;
      a.g[k] = reinterpret_cast<cbx::v4f *>(g[id]);
      a.last[k] = rmom ? reinterpret_cast<cbx::v4f *>(rlast[id]) : nullptr;
      a.rate[k] = -1.0f * learning_rate[id];  // sma.cu:43
    }
  }
  if (participating > cbx::kMaxReplicas)
    return fail(CBX_ERR_UNSUPPORTED, "%s: %d participating replicas, more than %d on one device", me, participating,
                cbx::kMaxReplicas);
  a.z = reinterpret_cast<cbx::v4f *>(z[0]);
  a.n4 = p->n4b;
  a.alpha = alpha;  // synchronouseamsgd.c:13
  a.momentum = steps && rmom ? replica_momentum : 0.0f;
  a.wd = steps && weight_decay > 0.0f ? weight_decay : 0.0f;
  a.tail_lo = p->n4b * 4;  // the elements past the last whole chunk ride the same launch
  a.tail_hi = p->n;
  auto &d = p->devs[0];
  HIP_TRY(hipSetDevice(d.hip_id));
  cbx::LaunchConfig cfg = p->task_barrier_cfg;
  cfg.num_cus = d.num_cus;
  hipStream_t st0 = static_cast<hipStream_t>(streams[0]);
  if (clipped && steps) {
    // The norm passes in id order on the launch's stream, each over its slot's
    // scratch (allocated on first use), as cbx_sma_plan_optimise_clipped runs
    // them: the records are the sequence's bits.  No wait is queued.
    cbx::ClipRecordPtrs records;
    std::memset(&records, 0, sizeof(records));
    cbx::ClipScratch *cs[cbx::kMaxReplicas] = {};
    for (int k = 0; k < a.nrep; ++k)  // every scratch before the first launch: a failed allocation bumps no counter
      if (slot_of[k] >= 0) TRY(clip_slot(p, me, 0, slot_of[k], &cs[k]));
    for (int k = 0; k < a.nrep; ++k) {
      if (!cs[k]) continue;
      HIP_TRY(cbx::launch_gradient_norm(reinterpret_cast<const float *>(a.g[k]), p->n, *cs[k], clip.max_norm,
                                        clip.skip_nonfinite == 1, p->clip_norm_policy, st0));
      records.p[k] = cs[k]->record();
    }
    if (variables) HIP_TRY(cbx::launch_task_elastic_clipped_variables(a, d.var_tables, records, keep, cfg, st0, p->next_timing()));
    else HIP_TRY(cbx::launch_task_elastic_clipped(a, records, keep, cfg, st0, p->next_timing()));
  } else if (variables)
    HIP_TRY(cbx::launch_task_elastic_variables(a, d.var_tables, keep, cfg, st0, p->next_timing()));
  else
    HIP_TRY(cbx::launch_task_elastic(a, keep, cfg, st0, p->next_timing()));
  return CBX_OK;
}

int cbx_ea_plan_step_and_optimise(cbx_sma_plan *p, void *const *streams, float *const *z, int nreplicas,
                                  const int *replica_device, float *const *w, float *const *s, float *const *g,
                                  float *const *rlast, const int *locked, const int *step, const float *learning_rate,
                                  float alpha, float replica_momentum, float weight_decay, int first, unsigned flags) {
  return ea_plan_step_and_optimise(p, streams, z, nreplicas, replica_device, w, s, g, rlast, locked, step,
                                   learning_rate, alpha, replica_momentum, weight_decay, first, flags, false);
}

int cbx_ea_plan_step_and_optimise_clipped_variables(cbx_sma_plan *p, void *const *streams, float *const *z,
                                                    int nreplicas, const int *replica_device, float *const *w,
                                                    float *const *s, float *const *g, float *const *rlast,
                                                    const int *locked, const int *step, const float *learning_rate,
                                                    const int *slot, float max_norm, int skip_nonfinite,
                                                    int use_variables, float alpha, float replica_momentum,
                                                    float weight_decay, int first, unsigned flags) {
  SeamClip clip;
  clip.slot = slot;
  clip.max_norm = max_norm;
  clip.skip_nonfinite = skip_nonfinite;
  return ea_plan_step_and_optimise(p, streams, z, nreplicas, replica_device, w, s, g, rlast, locked, step,
                                   learning_rate, alpha, replica_momentum, weight_decay, first, flags, true, clip,
                                   use_variables);
}

// crossbowSynchronisationSynchronousSGD (synch/synchronoussgd.c:13-106) over
// the caller's buffers: the all-reduce of every device's accumulated,
// lr-scaled gradient, the 1/wpc scale, the base momentum (the configured one,
// not forced to 0.9), z += D, the reset of the accumulator and base ->
// replica copies (common.c:198-220), in one apply pass per bucket.  G = 1 runs
// the multi-GPU algorithm with the identity all-reduce (the reference's
// single-GPU variant is err(), :5-11), as the context does.
int cbx_ssgd_plan_step(cbx_sma_plan *p, void *const *streams, float *const *z, float *const *last, float *const *acc,
                       int nreplicas, const int *replica_device, float *const *w, const int *locked, float momentum,
                       int wpc, int first) {
  TraceRange trace("cbx_ssgd_plan_step");
  if (!p) return fail(CBX_ERR_INVALID, "null plan");
  const int G = (int)p->devs.size();
  if (!streams || !z || !acc || nreplicas < 0 || (nreplicas > 0 && (!replica_device || !w || !locked)))
    return fail(CBX_ERR_INVALID, "cbx_ssgd_plan_step: missing arguments");
  if (wpc <= 0) return fail(CBX_ERR_INVALID, "S-SGD needs the work per clock (wpc %d)", wpc);
  if (first < 0 || first > nreplicas) return fail(CBX_ERR_INVALID, "first replica %d out of range", first);
  const bool mom = momentum > 0.0f;  // synchronoussgd.c:64
  if (mom && !last) return fail(CBX_ERR_INVALID, "momentum > 0 needs the base models' last buffers");
  std::vector<cbx::SsgdArgs> args(G);
  for (int k = 0; k < G; ++k) {
    cbx::SsgdArgs &a = args[k];
    std::memset(&a, 0, sizeof(a));
    if (!z[k] || !acc[k] || !aligned16(z[k]) || !aligned16(acc[k]) || (mom && (!last[k] || !aligned16(last[k]))))
      return fail(CBX_ERR_INVALID, "device %d: base buffers must be non-null and 16-byte aligned", k);
    a.z = reinterpret_cast<cbx::v4f *>(z[k]);
    a.last = mom ? reinterpret_cast<cbx::v4f *>(last[k]) : nullptr;
    a.acc = reinterpret_cast<cbx::v4f *>(acc[k]);
    a.D = p->ranks == 1 ? a.acc : reinterpret_cast<const cbx::v4f *>(p->devs[k].D_ctrl + cbx::kCtrlFloats);
    a.n4 = p->n4b;
    a.ratio = (float)(1.0 / (double)(float)wpc);  // :55
    a.momentum = mom ? momentum : 0.0f;
  }
  TRY(gather_replicas(args, first, nreplicas, replica_device, locked, w, nullptr,
                      "replica %d: buffer must be 16-byte aligned", [](cbx::SsgdArgs &, int) {}));
  // Buckets as in the SMA step; at G > 1 with more than one, the all-reduce
  // of bucket k+1 runs on the plan's stream beside the apply of bucket k
  // (reduce_apply, bucket_pipeline.h).  One rank: no collective, one launch.
  const BucketGrid grid = p->ranks == 1 ? BucketGrid::whole(p->n4b) : BucketGrid::by_count(p->n4b, p->buckets);
  if (p->ranks > 1 && grid.nb > 1) TRY(ensure_pipeline(p, grid.nb));
  std::vector<SsgdPlanLane> lanes;
  for (int k = 0; k < G; ++k)
    lanes.push_back({PlanLane(p, k, streams, acc[k], false), args[k]});
  return reduce_apply(lanes, grid, p->ranks > 1, group_begin, group_end);
}

// The task steps of kernels/optimisers/synchronoussgd.cu of every stepping
// replica, in id order, and the one-device synchronous-SGD barrier
// (synch/synchronoussgd.c:13-106, common.c:198-220) in one launch over the
// caller's buffers: the context's cbx_step_and_synchronise_ssgd (context.hip)
// with the caller's rates and stream order.  cbx_ssgd_plan_step plus g, step,
// learning_rate, weight_decay and flags.  The bulk runs the context's float4
// loop, the elements past it the kernel's TAIL workgroups
// (task_ssgd_kernels.hip).  Everything is validated before the launch; the plan
// queues no wait of its own.
int cbx_ssgd_plan_step_and_optimise(cbx_sma_plan *p, void *const *streams, float *const *z, float *const *last,
                                    float *const *acc, int nreplicas, const int *replica_device, float *const *w,
                                    float *const *g, const int *locked, const int *step, const float *learning_rate,
                                    float momentum, float weight_decay, int wpc, int first, unsigned flags) {
  const char *me = "cbx_ssgd_plan_step_and_optimise";
  TraceRange trace(me);
  if (!p) return fail(CBX_ERR_INVALID, "null plan");
  if (!streams || !z || !acc || nreplicas < 0 || (nreplicas > 0 && (!replica_device || !w || !locked || !step)))
    return fail(CBX_ERR_INVALID, "%s: missing arguments", me);
  if (flags & ~CBX_STEP_DISCARD_TASK_OUTPUTS) return fail(CBX_ERR_INVALID, "%s: unknown flag bits 0x%x", me, flags);
  if (wpc <= 0) return fail(CBX_ERR_INVALID, "%s: S-SGD needs the work per clock (wpc %d)", me, wpc);
  if (first < 0 || first > nreplicas) return fail(CBX_ERR_INVALID, "%s: first replica %d out of range", me, first);
  const bool keep = (flags & CBX_STEP_DISCARD_TASK_OUTPUTS) == 0;
  const bool mom = momentum > 0.0f;     // synchronoussgd.c:64
  const bool wd = weight_decay > 0.0f;  // synchronoussgd.cu:20
  if (mom && !last) return fail(CBX_ERR_INVALID, "%s: momentum > 0 needs the base model's last buffer", me);
  for (int id = 0; id < nreplicas; ++id) {
    if (!step[id]) continue;
    if (!locked[id]) return fail(CBX_ERR_INVALID, "%s: stepping replica %d is not locked for this barrier", me, id);
    if (id < first) return fail(CBX_ERR_INVALID, "%s: stepping replica %d is below the first replica %d", me, id, first);
    if (!g || !learning_rate) return fail(CBX_ERR_INVALID, "%s: a stepping replica needs g and learning_rate", me);
  }
  if (p->devs.size() != 1 || p->ranks != 1)
    return fail(CBX_ERR_UNSUPPORTED, "%s: a plan of %d devices and %d ranks; the task steps are fused into the one-GPU "
                "barrier only; use cbx_ssgd_accumulate_buffers and cbx_ssgd_plan_step", me, (int)p->devs.size(), p->ranks);
  if (!z[0] || !acc[0] || !aligned16(z[0]) || !aligned16(acc[0]) || (mom && (!last[0] || !aligned16(last[0]))))
    return fail(CBX_ERR_INVALID, "%s: base buffers must be non-null and 16-byte aligned", me);
  cbx::TaskSsgdArgs a;
  std::memset(&a, 0, sizeof(a));
  int participating = 0;
  for (int id = first; id < nreplicas; ++id) {  // increasing id order: the steps' enqueue order, and common.c:208
    if (!locked[id]) continue;
    if (replica_device[id] != 0) return fail(CBX_ERR_INVALID, "%s: replica %d on device %d of 1", me, id, replica_device[id]);
    const bool st = step[id] != 0;
    if (!w[id] || !aligned16(w[id])) return fail(CBX_ERR_INVALID, "%s: replica %d: w must be non-null and 16-byte aligned", me, id);
    // a replica that only joins is one write stream: its g may be NULL
    if (st && (!g[id] || !aligned16(g[id])))
      return fail(CBX_ERR_INVALID, "%s: stepping replica %d: g must be non-null and 16-byte aligned", me, id);
    if (++participating > cbx::kMaxReplicas) continue;  // counted on, refused below
    a.w[a.nrecv++] = reinterpret_cast<cbx::v4f *>(w[id]);
    if (!st) continue;
    const int k = a.nstep++;
    a.sw[k] = reinterpret_cast<const cbx::v4f *>(w[id]);
    a.g[k] = reinterpret_cast<cbx::v4f *>(g[id]);
    a.rate[k] = -1.0f * learning_rate[id];  // synchronoussgd.cu:46
  }
  if (participating > cbx::kMaxReplicas)
    return fail(CBX_ERR_UNSUPPORTED, "%s: %d participating replicas, more than %d on one device", me, participating,
                cbx::kMaxReplicas);
  a.z = reinterpret_cast<cbx::v4f *>(z[0]);
  a.last = mom ? reinterpret_cast<cbx::v4f *>(last[0]) : nullptr;
  a.acc = reinterpret_cast<cbx::v4f *>(acc[0]);
  a.n4 = p->n4b;
  a.wd = a.nstep > 0 && wd ? weight_decay : 0.0f;
  a.ratio = (float)(1.0 / (double)(float)wpc);  // synchronoussgd.c:55
  a.momentum = mom ? momentum : 0.0f;
  a.tail_lo = p->n4b * 4;  // the elements past the last whole chunk ride the same launch
  a.tail_hi = p->n;
  auto &d = p->devs[0];
  HIP_TRY(hipSetDevice(d.hip_id));
  cbx::LaunchConfig cfg = p->task_barrier_cfg;
  cfg.num_cus = d.num_cus;
  HIP_TRY(cbx::launch_task_ssgd(a, keep, cfg, static_cast<hipStream_t>(streams[0]), p->next_timing()));
  return CBX_OK;
}

// crossbowKernelOptimiserSynchronousSGD (kernels/optimisers/synchronoussgd.cu:
// 3-56) over the caller's buffers, one pass: weight decay into the replica's
// gradient, then the lr-scaled gradient added into the device's base-model
// gradient.  On `stream` = the device's model-synchronisation stream, after
// it waits for the task's gradient (:37-40), so the tasks of a clock add in
// stream order.
int cbx_ssgd_accumulate_buffers(void *stream, const float *w, float *g, float *acc, long long elements,
                                float learning_rate, float weight_decay) {
  TraceRange trace("cbx_ssgd_accumulate_buffers");
  if (elements <= 0 || elements * 4 + 4096 >= (1ll << 32))
    return fail(CBX_ERR_INVALID, "cbx_ssgd_accumulate_buffers: %lld elements out of range", elements);
  if (!g || !acc || (weight_decay > 0.0f && !w)) return fail(CBX_ERR_INVALID, "cbx_ssgd_accumulate_buffers: missing buffers");
  if (!aligned16(g) || !aligned16(acc) || (weight_decay > 0.0f && !aligned16(w)))
    return fail(CBX_ERR_INVALID, "cbx_ssgd_accumulate_buffers: buffers must be 16-byte aligned");
  int cus = 256;
  TRY(cus_of_current_device(&cus));
  cbx::SsgdArgs a;
  std::memset(&a, 0, sizeof(a));
  a.wsrc = reinterpret_cast<const cbx::v4f *>(w);
  a.g = reinterpret_cast<cbx::v4f *>(g);
  a.acc = reinterpret_cast<cbx::v4f *>(acc);
  a.n4 = bulk_float4s(elements);
  a.rate = -1.0f * learning_rate;  // :46
  a.wd = weight_decay;
  a.tail_lo = a.n4 * 4;
  a.tail_hi = elements;
  cbx::LaunchConfig cfg = cbx::aux_launch_config();
  cfg.num_cus = cus;
  HIP_TRY(cbx::launch_ssgd_accumulate(a, cfg, static_cast<hipStream_t>(stream)));
  return CBX_OK;
}

// crossbowCudnnBatchNormParamsSynchroniseEstimatedMeanAndVariable
// (cudnn/cudnnbatchnormparams.c:157-222) over the caller's statistics buffers,
// the same packed all-reduce as cbx_average_batchnorm_stats, on the plan's
// stream; device-synchronises before and after, as the reference does.
int cbx_sma_plan_average_batchnorm(cbx_sma_plan *p, int layers, const int *elements, float *const *mean,
                                   float *const *variance, const int *updated) {
  TraceRange trace("cbx_sma_plan_average_batchnorm");
  if (!p) return fail(CBX_ERR_INVALID, "null plan");
  if (layers < 0 || (layers > 0 && (!elements || !mean || !variance || !updated)))
    return fail(CBX_ERR_INVALID, "bad batch-norm statistics arguments");
  if (layers == 0 || p->ranks == 1) return CBX_OK;  // :165-166: nothing to average with one device
  TRY(ensure_pipeline(p, 1));
  std::vector<BnDevice> devs;
  for (auto &d : p->devs)
    devs.push_back({d.hip_id, d.global, d.comm, d.comm_stream, &d.bn_table, &d.bn_table_bytes, &d.bn_scratch,
                    &d.bn_scratch_bytes});
  return bn_average(devs, layers, elements, mean, variance, updated);
}

int cbx_sma_plan_set_buckets(cbx_sma_plan *p, int buckets) {
  if (!p) return fail(CBX_ERR_INVALID, "null plan");
  if (buckets < 0 || buckets > 4096) return fail(CBX_ERR_INVALID, "plan buckets must be 0..4096, got %d", buckets);
  p->buckets = buckets;
  return CBX_OK;
}

int cbx_sma_plan_buffer_stats(cbx_sma_plan *p, int k, void *stream, const float *ref, const float *const *bufs,
                              int nbufs, const long long *var_elements, int nvars, cbx_buffer_stats *ref_out,
                              cbx_buffer_stats *out, cbx_buffer_stats *ref_vars, cbx_buffer_stats *vars) {
  TraceRange trace("cbx_sma_plan_buffer_stats");
  if (!p) return fail(CBX_ERR_INVALID, "null plan");
  if (k < 0 || k >= (int)p->devs.size()) return fail(CBX_ERR_INVALID, "plan device %d out of range", k);
  if (!ref_out || (nbufs > 0 && !out) || nbufs < 0 || nbufs > cbx::kMaxReplicas || nvars < 0)
    return fail(CBX_ERR_INVALID, "cbx_sma_plan_buffer_stats: bad buffer count or null result array");
  auto &d = p->devs[k];
  HIP_TRY(hipSetDevice(d.hip_id));
  const size_t nb = (size_t)nbufs + 1, V = nvars > 0 ? (size_t)nvars : 1;
  std::vector<cbx_buffer_stats> totals(nb), pv;
  const bool want_vars = ref_vars || vars;
  if (want_vars) pv.resize(V * nb);
  TRY(cbx::stats_run(d.stats, static_cast<hipStream_t>(stream), ref, bufs, nbufs, var_elements, nvars, p->n,
                     totals.data(), want_vars ? pv.data() : nullptr));
  *ref_out = totals[0];
  for (int i = 0; i < nbufs; ++i) out[i] = totals[1 + i];
  for (size_t v = 0; v < V; ++v) {
    if (ref_vars) ref_vars[v] = pv[v * nb];
    for (int i = 0; vars && i < nbufs; ++i) vars[(size_t)i * V + v] = pv[v * nb + 1 + i];
  }
  return CBX_OK;
}

int cbx_sma_optimise_buffers(void *stream, float *w, float *g, float *last, float *s, long long elements,
                             float learning_rate, float momentum, float weight_decay) {
  TraceRange trace("cbx_sma_optimise_buffers");
  if (elements <= 0 || elements * 4 + 4096 >= (1ll << 32))
    return fail(CBX_ERR_INVALID, "cbx_sma_optimise_buffers: %lld elements out of range", elements);
  if (!w || !g || !s || (momentum > 0.0f && !last))
    return fail(CBX_ERR_INVALID, "cbx_sma_optimise_buffers: missing buffers");
  if (!aligned16(w) || !aligned16(g) || !aligned16(s) || (momentum > 0.0f && !aligned16(last)))
    return fail(CBX_ERR_INVALID, "cbx_sma_optimise_buffers: buffers must be 16-byte aligned");
  hipStream_t st = static_cast<hipStream_t>(stream);
  int cus = 256;
  TRY(cus_of_current_device(&cus));
  cbx::OptArgs a;
  std::memset(&a, 0, sizeof(a));
  a.w = reinterpret_cast<cbx::v4f *>(w);
  a.g = reinterpret_cast<cbx::v4f *>(g);
  a.last = momentum > 0.0f ? reinterpret_cast<cbx::v4f *>(last) : nullptr;
  a.s = reinterpret_cast<cbx::v4f *>(s);
  a.n4 = bulk_float4s(elements);
  a.rate = -1.0f * learning_rate;  // sma.cu:43
  a.momentum = momentum;
  a.wd = weight_decay;
  cbx::LaunchConfig cfg = cbx::aux_launch_config();
  cfg.num_cus = cus;
  a.tail_lo = a.n4 * 4;  // the elements past the last whole trip ride the same launch
  a.tail_hi = elements;
  HIP_TRY(cbx::launch_sma_optimise(a, cfg, st));
  return CBX_OK;
}

int cbx_sma_plan_set_variables(cbx_sma_plan *p, const long long *var_elements, const float *multipliers, int nvars) {
  TraceRange trace("cbx_sma_plan_set_variables");
  if (!p) return fail(CBX_ERR_INVALID, "null plan");
  if (!var_elements || nvars <= 0) return fail(CBX_ERR_INVALID, "cbx_sma_plan_set_variables: no variables");
  cbx::OptimisePlan plan;
  if (!cbx::build_optimise_plan(var_elements, nvars, p->n, &plan))
    return fail(CBX_ERR_INVALID,
                "cbx_sma_plan_set_variables: %d variables with a negative count, or not summing to the plan's %lld "
                "elements", nvars, (long long)p->n);
  for (auto &d : p->devs) {
    HIP_TRY(hipSetDevice(d.hip_id));
    HIP_TRY(hipDeviceSynchronize());  // no step in flight still reads the tables being replaced
    HIP_TRY(cbx::var_tables_upload(d.var_tables, plan.chunks.data(), plan.chunks.size(), plan.bounds.data(),
                                   multipliers, (uint32_t)nvars));
  }
  p->var_bounds = plan.bounds;
  return CBX_OK;
}

int cbx_sma_plan_optimise_variables(cbx_sma_plan *p, int k, void *stream, float *w, float *g, float *last, float *s,
                                    float learning_rate, float momentum, float weight_decay, int first_var,
                                    int nvars) {
  TraceRange trace("cbx_sma_plan_optimise_variables");
  if (!p) return fail(CBX_ERR_INVALID, "null plan");
  if (k < 0 || k >= (int)p->devs.size()) return fail(CBX_ERR_INVALID, "plan device %d out of range", k);
  if (p->var_bounds.empty())
    return fail(CBX_ERR_STATE, "cbx_sma_plan_optimise_variables before cbx_sma_plan_set_variables");
  const int V = (int)p->var_bounds.size() - 1;
  if (first_var < 0 || nvars < 0 || first_var > V || nvars > V - first_var)
    return fail(CBX_ERR_INVALID, "cbx_sma_plan_optimise_variables: variables [%d, %d + %d) out of range [0, %d)",
                first_var, first_var, nvars, V);
  if (!w || !g || !s || (momentum > 0.0f && !last))
    return fail(CBX_ERR_INVALID, "cbx_sma_plan_optimise_variables: missing buffers");
  if (!aligned16(w) || !aligned16(g) || !aligned16(s) || (momentum > 0.0f && !aligned16(last)))
    return fail(CBX_ERR_INVALID, "cbx_sma_plan_optimise_variables: buffers must be 16-byte aligned");
  if (nvars == 0) return CBX_OK;
  auto &d = p->devs[k];
  HIP_TRY(hipSetDevice(d.hip_id));
  cbx::VarOptArgs a;
  std::memset(&a, 0, sizeof(a));
  a.w = reinterpret_cast<cbx::v4f *>(w);
  a.g = reinterpret_cast<cbx::v4f *>(g);
  a.last = momentum > 0.0f ? reinterpret_cast<cbx::v4f *>(last) : nullptr;
  a.s = reinterpret_cast<cbx::v4f *>(s);
  a.lo = p->var_bounds[(size_t)first_var];
  a.hi = p->var_bounds[(size_t)first_var + (size_t)nvars];
  a.rate = -1.0f * learning_rate;  // sma.cu:43
  a.momentum = momentum;
  a.wd = weight_decay;
  cbx::LaunchConfig cfg = cbx::aux_launch_config();
  cfg.num_cus = d.num_cus;
  HIP_TRY(cbx::launch_sma_optimise_variables(d.var_tables, a, cfg, static_cast<hipStream_t>(stream)));
  return CBX_OK;
}

namespace {

// The slot's scratch on plan device k (the current device), allocated and
// zeroed on first use.
int clip_slot(cbx_sma_plan *p, const char *what, int k, int slot, cbx::ClipScratch **out) {
  if (!p) return fail(CBX_ERR_INVALID, "null plan");
  if (k < 0 || k >= (int)p->devs.size()) return fail(CBX_ERR_INVALID, "plan device %d out of range", k);
  if (slot < 0 || slot >= cbx_sma_plan::kClipSlots)
    return fail(CBX_ERR_INVALID, "%s: slot %d out of range [0, %d)", what, slot, cbx_sma_plan::kClipSlots);
  auto &d = p->devs[k];
  HIP_TRY(hipSetDevice(d.hip_id));
  std::lock_guard<std::mutex> lock(p->clip_mu);
  if (!d.clip[slot].dev) HIP_TRY(cbx::clip_scratch_alloc(d.clip[slot], p->n));
  *out = &d.clip[slot];
  return CBX_OK;
}

}  // namespace

int cbx_sma_plan_optimise_clipped(cbx_sma_plan *p, int k, int slot, void *stream, float *w, float *g, float *last,
                                  float *s, float learning_rate, float momentum, float weight_decay, float max_norm,
                                  int skip_nonfinite, int use_variables) {
  TraceRange trace("cbx_sma_plan_optimise_clipped");
  if (!p) return fail(CBX_ERR_INVALID, "null plan");
  if (!(max_norm >= 0.0f) || std::isinf(max_norm))
    return fail(CBX_ERR_INVALID, "cbx_sma_plan_optimise_clipped: max_norm %g is negative, NaN or infinite",
                (double)max_norm);
  if (skip_nonfinite != 0 && skip_nonfinite != 1)
    return fail(CBX_ERR_INVALID, "cbx_sma_plan_optimise_clipped: skip_nonfinite %d is neither 0 nor 1", skip_nonfinite);
  if (use_variables != 0 && use_variables != 1)
    return fail(CBX_ERR_INVALID, "cbx_sma_plan_optimise_clipped: use_variables %d is neither 0 nor 1", use_variables);
  if (use_variables && p->var_bounds.empty())
    return fail(CBX_ERR_STATE, "cbx_sma_plan_optimise_clipped with variables before cbx_sma_plan_set_variables");
  if (!w || !g || !s || (momentum > 0.0f && !last))
    return fail(CBX_ERR_INVALID, "cbx_sma_plan_optimise_clipped: missing buffers");
  if (!aligned16(w) || !aligned16(g) || !aligned16(s) || (momentum > 0.0f && !aligned16(last)))
    return fail(CBX_ERR_INVALID, "cbx_sma_plan_optimise_clipped: buffers must be 16-byte aligned");
  cbx::ClipScratch *cs = nullptr;
  TRY(clip_slot(p, "cbx_sma_plan_optimise_clipped", k, slot, &cs));
  auto &d = p->devs[k];
  hipStream_t st = static_cast<hipStream_t>(stream);
  cbx::LaunchConfig cfg = cbx::aux_launch_config();
  cfg.num_cus = d.num_cus;
  HIP_TRY(cbx::launch_gradient_norm(g, p->n, *cs, max_norm, skip_nonfinite == 1, p->clip_norm_policy, st));
  if (use_variables) {
    cbx::VarOptArgs a;
    std::memset(&a, 0, sizeof(a));
    a.w = reinterpret_cast<cbx::v4f *>(w);
    a.g = reinterpret_cast<cbx::v4f *>(g);
    a.last = momentum > 0.0f ? reinterpret_cast<cbx::v4f *>(last) : nullptr;
    a.s = reinterpret_cast<cbx::v4f *>(s);
    a.lo = 0;
    a.hi = p->var_bounds.back();
    a.rate = -1.0f * learning_rate;  // sma.cu:43
    a.momentum = momentum;
    a.wd = weight_decay;
    HIP_TRY(cbx::launch_sma_optimise_variables_clipped(d.var_tables, a, cs->record(), cfg, st));
    return CBX_OK;
  }
  cbx::OptArgs a;
  std::memset(&a, 0, sizeof(a));
  a.w = reinterpret_cast<cbx::v4f *>(w);
  a.g = reinterpret_cast<cbx::v4f *>(g);
  a.last = momentum > 0.0f ? reinterpret_cast<cbx::v4f *>(last) : nullptr;
  a.s = reinterpret_cast<cbx::v4f *>(s);
  a.n4 = p->n4b;
  a.rate = -1.0f * learning_rate;  // sma.cu:43
  a.momentum = momentum;
  a.wd = weight_decay;
  a.tail_lo = a.n4 * 4;  // the elements past the last whole trip ride the same launch
  a.tail_hi = p->n;
  HIP_TRY(cbx::launch_sma_optimise_clipped(a, cs->record(), cfg, st));
  return CBX_OK;
}

int cbx_sma_plan_gradient_norm(cbx_sma_plan *p, int k, int slot, void *stream, const float *g, float max_norm,
                               int skip_nonfinite, int loads, float *pass_ms, float *reduce_ms) {
  TraceRange trace("cbx_sma_plan_gradient_norm");
  if (!p) return fail(CBX_ERR_INVALID, "null plan");
  if (!(max_norm >= 0.0f) || std::isinf(max_norm) || (skip_nonfinite != 0 && skip_nonfinite != 1) || loads < -1 ||
      loads > 1)
    return fail(CBX_ERR_INVALID, "cbx_sma_plan_gradient_norm: max_norm %g, skip_nonfinite %d or loads %d out of range",
                (double)max_norm, skip_nonfinite, loads);
  if (!g || !aligned16(g)) return fail(CBX_ERR_INVALID, "cbx_sma_plan_gradient_norm: g must be non-null and 16-byte aligned");
  cbx::ClipScratch *cs = nullptr;
  TRY(clip_slot(p, "cbx_sma_plan_gradient_norm", k, slot, &cs));
  hipStream_t st = static_cast<hipStream_t>(stream);
  hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
  const bool timed = pass_ms || reduce_ms;
  int rc = CBX_OK;
  auto run = [&]() -> int {
    if (timed)
      for (hipEvent_t &e : ev) HIP_TRY(hipEventCreate(&e));
    HIP_TRY(cbx::launch_gradient_norm(g, p->n, *cs, max_norm, skip_nonfinite == 1,
                                      loads < 0 ? p->clip_norm_policy : loads, st, {ev[0], ev[1]}, {ev[2], ev[3]}));
    HIP_TRY(hipStreamSynchronize(st));
    if (pass_ms) HIP_TRY(hipEventElapsedTime(pass_ms, ev[0], ev[1]));
    if (reduce_ms) HIP_TRY(hipEventElapsedTime(reduce_ms, ev[2], ev[3]));
    return CBX_OK;
  };
  rc = run();
  for (hipEvent_t e : ev)
    if (e) (void)hipEventDestroy(e);
  return rc;
}

int cbx_sma_plan_clip_stats(cbx_sma_plan *p, int k, int slot, void *stream, cbx_clip_stats *out) {
  TraceRange trace("cbx_sma_plan_clip_stats");
  if (!out) return fail(CBX_ERR_INVALID, "cbx_sma_plan_clip_stats: null result");
  cbx::ClipScratch *cs = nullptr;
  TRY(clip_slot(p, "cbx_sma_plan_clip_stats", k, slot, &cs));
  hipStream_t st = static_cast<hipStream_t>(stream);
  HIP_TRY(hipMemcpyAsync(out, cs->record(), sizeof(*out), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  return CBX_OK;
}

}  // extern "C"
