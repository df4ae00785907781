/*
 * crossbow_sma.h -- C-ABI of the MI355X-native synchronous model averaging
 * (SMA) path of Crossbow.  Library: crossbow_amd/libcrossbow_sma.so
 * (hipcc, gfx950).  Plain C types only; no HIP or torch types cross it.
 *
 * The entry points are the ones Crossbow's JNI glue binds for the model path
 * (clib-multigpu/GPU.c, header clib-multigpu/uk_ac_imperial_lsds_crossbow_device_TheGPU.h).
 * Each declaration cites the JNI native it replaces.  The reference keeps a
 * process-global context (static theGPU, GPU.c:12); this ABI passes it as an
 * explicit handle and the JNI shim (crossbow_amd/csrc/jni/) keeps the global.
 *
 * Error behaviour: the reference prints and exit(1)s on every failure
 * (clib-multigpu/debug.h:37-57).  Here every function returns a status
 * (CBX_OK or a negative CBX_ERR_*), cbx_last_error() holds the message, and
 * the JNI shim restores "fatal = process exit".  Functions documented as
 * returning a count return it when >= 0.
 */
#ifndef CROSSBOW_SMA_H_
#define CROSSBOW_SMA_H_

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CBX_ABI_VERSION 1

#define CBX_OK               0
#define CBX_ERR_INVALID     -1  /* bad argument                                   */
#define CBX_ERR_STATE       -2  /* call out of order (e.g. sync before manager)   */
#define CBX_ERR_HIP         -3  /* HIP runtime failure                            */
#define CBX_ERR_RCCL        -4  /* RCCL failure                                   */
#define CBX_ERR_IO          -5  /* checkpoint file I/O                            */
#define CBX_ERR_NO_DEVICE   -6  /* no usable MI355X (gfx950) device               */
#define CBX_ERR_BARRIER     -7  /* BSP barrier could not lock every replica       */
#define CBX_ERR_UNSUPPORTED -8  /* outside this library's scope   */

/* Update model ids, uk/ac/imperial/lsds/crossbow/types/UpdateModel.java:5 */
#define CBX_UPDATE_DEFAULT           0   /* single GPU: synch/default.c, optimisers/default.cu */
#define CBX_UPDATE_WORKER            1   /* synchronous SGD: synch/synchronoussgd.c */
#define CBX_UPDATE_SYNCHRONOUSEAMSGD 3   /* SMA (clib-multigpu/utils.h:56-57), or elastic averaging: cbx_set_elastic_average */
#define CBX_UPDATE_POLYAK_RUPPERT    6   /* synch/polyakruppert.c */
#define CBX_UPDATE_SMA               7

/* Synchronisation models, types/SynchronisationModel.java:5 */
#define CBX_SYNC_BSP 0
#define CBX_SYNC_SSP 1
#define CBX_SYNC_ASP 2

/* Per-model buffers, clib-multigpu/model.h:22-87 */
#define CBX_BUF_DATA     0   /* base: z ; replica: w                    */
#define CBX_BUF_GRADIENT 1   /* base: acc (Phase A output)              */
#define CBX_BUF_DIFF     2   /* base: D (all-reduced) ; replica: s      */
#define CBX_BUF_LAST     3   /* momentum buffer; exists iff momentum>0  */

typedef struct cbx_context cbx_context;

int         cbx_abi_version (void);
const char *cbx_last_error (void);
/* Number of visible gfx950 devices (0 on a host without one). */
int         cbx_device_count (int *count);

/* ---- execution context ------------------------------------------------ */
/* TheGPU.init([I...)  GPU.c:21-63 -> executioncontext.c:152-345.
 * One process drives `ndevices` local GPUs; RCCL comms via ncclCommInitAll
 * (executioncontext.c:185-201), indexed by rank, not device id.          */
int cbx_init (cbx_context **ctx, const int *devices, int ndevices);
/* One process per GPU (torch.distributed launch): rank r of n drives one
 * device; `unique_id` (128 bytes) comes from cbx_get_unique_id on rank 0. */
int cbx_get_unique_id (unsigned char unique_id[128]);
int cbx_init_rank (cbx_context **ctx, int device, int nranks, int rank,
		const unsigned char unique_id[128]);
/* TheGPU.free()  GPU.c:65-75 -> executioncontext.c:728-898 */
int cbx_free (cbx_context *ctx);

/* ---- model registration (Model.GPURegister, Model.java:338-371) ------- */
/* TheGPU.setModel(II)                      GPU.c:672-681  */
int cbx_set_model (cbx_context *ctx, int variables, int bytes);
/* TheGPU.setModelVariable(II[II)           GPU.c:683-696  */
int cbx_set_model_variable (cbx_context *ctx, int id, int order, int ndims,
		const int *shape, int capacity);
/* TheGPU.setModelVariableBuffer(IILjava/nio/ByteBuffer;)  GPU.c:698-708 */
int cbx_set_model_variable_buffer (cbx_context *ctx, int id, int order, const void *src);
/* TheGPU.setModelVariableLearningRateMultiplier(IIF)  GPU.c:710-719.  Stored,
 * and conf.irregular counts every value other than 1
 * (executioncontext.c:1592-1605).  The replica step honours it where the
 * reference does (crossbowModelGetLearningRateForVariable, model.c:159-177):
 * in cbx_replica_optimise once cbx_set_variable_learning_rates is on, and in
 * cbx_replica_optimise_variables always.  May be called before or after
 * cbx_set_model_manager.  After it, the call blocks: it waits for every
 * local device to drain, then copies the one value into the device tables,
 * so the next step enqueued on any stream uses it.                        */
int cbx_set_model_variable_learning_rate_multiplier (cbx_context *ctx, int id, int order, float multiplier);
/* TheGPU.setModelWorkPerClock(I)           GPU.c:721-730  */
int cbx_set_model_work_per_clock (cbx_context *ctx, int wpc);
/* TheGPU.setUpdateModelType(I)             GPU.c:732-741.  0..7 are stored;
 * cbx_synchronise runs 0, 1, 3, 6 and 7 (see there).                      */
int cbx_set_update_model_type (cbx_context *ctx, int type);
/* The reference's compile-time ELASTIC_AVERAGE (executioncontext.c:2287-2295)
 * as a run-time switch.  0 (the default, the reference's default build):
 * update model SYNCHRONOUSEAMSGD (3) runs SMA, exactly as SMA (7) does.
 * 1: it runs the elastic-averaging barrier
 * (crossbowSynchronisationSynchronousElasticAveragingSGD,
 * synch/synchronouseamsgd.c:5-305).  SMA (7) is unaffected either way.
 * May be set before or after cbx_set_model_manager; any other value is
 * CBX_ERR_INVALID.                                                        */
int cbx_set_elastic_average (cbx_context *ctx, int enable);
/* Whether cbx_replica_optimise steps every variable with its own learning
 * rate, rate * multiplier (model.c:165-173), as the reference's optimisers do
 * when a multiplier other than 1 was registered (conf.irregular > 0,
 * model.c:167).  0 (the default): one rate for the whole model, whatever
 * multipliers are set, bit for bit the step as it was.  1: under SMA (7)
 * and SYNCHRONOUSEAMSGD (3), with elastic averaging on or off, variable v
 * steps with r_v = -rate * m_v (one fp32 multiply) whenever
 * conf.irregular > 0; with conf.irregular == 0 the one-rate kernel runs.
 * WORKER and DEFAULT keep ignoring the multipliers with the switch on.  The
 * lookup tables are built and uploaded to every local device by
 * cbx_set_model_manager; replicas added later (cbx_add_model) use them too.
 * A model whose variables do not tile its elements (a capacity above
 * 4 x elements) or that was registered as raw bytes has no variable ranges:
 * with the switch on and conf.irregular > 0 its cbx_replica_optimise is
 * CBX_ERR_UNSUPPORTED, with a message that names the variable.  May be set
 * before or after cbx_set_model_manager; any value other than 0 or 1 is
 * CBX_ERR_INVALID.                                                        */
int cbx_set_variable_learning_rates (cbx_context *ctx, int enable);

/* ---- solver (SolverConf.GPURegister, SolverConf.java:355-409) --------- */
/* TheGPU.setLearningRateDecayPolicy*  GPU.c:743-821 */
int cbx_set_learning_rate_decay_policy_fixed (cbx_context *ctx, float rate);
int cbx_set_learning_rate_decay_policy_inv (cbx_context *ctx, float rate, double gamma, double power);
int cbx_set_learning_rate_decay_policy_step (cbx_context *ctx, float rate, double gamma, int size);
int cbx_set_learning_rate_decay_policy_multistep (cbx_context *ctx, float rate, double gamma,
		int warmuptasks, int nsteps, const int *steps);
int cbx_set_learning_rate_decay_policy_exp (cbx_context *ctx, float rate, double gamma);
/* TheGPU.setLearningRateDecayPolicyCircular([FI[FI)  GPU.c:803-822: rate[3],
 * momentum[3]; stored, and a learning-rate query then fails with
 * CBX_ERR_UNSUPPORTED as the reference's does (solverconfiguration.c:155-157). */
int cbx_set_learning_rate_decay_policy_circular (cbx_context *ctx, const float *rate, int superconvergence,
		const float *momentum, int step);
/* TheGPU.setBaseModelMomentum(F)  GPU.c:823-832 (stored, unused: sma.c:152) */
int cbx_set_base_model_momentum (cbx_context *ctx, float momentum);
/* TheGPU.setMomentum(FI)          GPU.c:834-843 */
int cbx_set_momentum (cbx_context *ctx, float momentum, int method);
/* TheGPU.setWeightDecay(F)        GPU.c:845-854 */
int cbx_set_weight_decay (cbx_context *ctx, float decay);
/* TheGPU.setEamsgdAlpha(F)        GPU.c:856-865 */
int cbx_set_eamsgd_alpha (cbx_context *ctx, float alpha);
/* TheGPU.setEamsgdTau(I)          GPU.c:867-876 */
int cbx_set_eamsgd_tau (cbx_context *ctx, int tau);

/* ---- model manager ---------------------------------------------------- */
/* TheGPU.setModelManager(II)  GPU.c:878-886 -> executioncontext.c:1720-1764:
 * finalise, push theModel, one base model per GPU, `replicas` per GPU placed
 * round-robin (replica j*G+d on device d, modelmanager.c:51-64).           */
int cbx_set_model_manager (cbx_context *ctx, int replicas, int type);

/* ---- the barrier path (ModelManager.trySynchronise, ModelManager.java:293-353) */
/* TheGPU.lockAny()   GPU.c:1113-1120 -> executioncontext.c:2197-2211.
 * Returns the locked count (BSP: the replica count, or CBX_ERR_BARRIER).  */
int cbx_lock_any (cbx_context *ctx);
/* TheGPU.merge(Z)    GPU.c:1122-1131 -> executioncontext.c:2219-2245.
 * *first = first locked replica id, or -1 when no locked replica has an
 * update (the JNI return value).                                          */
int cbx_merge (cbx_context *ctx, int pull, int *first);
/* TheGPU.synchronise(IIIZ)  GPU.c:1133-1140 -> executioncontext.c:2262-2334
 * -> synch/sma.c:233-248.  Enqueues the SMA step on each device's model
 * synchronisation stream and returns without blocking the host.  Update
 * models SMA (7) and SYNCHRONOUSEAMSGD (3) run SMA; WORKER (1) runs the
 * synchronous-SGD barrier (synch/synchronoussgd.c:13-106, needs the work
 * per clock); DEFAULT (0) copies the base model to every locked replica
 * (synch/default.c:5-43; one GPU only, as in the reference: more devices
 * give CBX_ERR_UNSUPPORTED); any other is CBX_ERR_UNSUPPORTED.
 * With cbx_set_elastic_average on, SYNCHRONOUSEAMSGD (3) runs elastic
 * averaging instead (synch/synchronouseamsgd.c): every locked replica moves
 * towards z by alpha * (w_i - z) and z by the sum of those moves; no
 * momentum, the copy flags are neither read nor cleared.  On one device the
 * difference is taken from the replica's data, on several from its snapshot
 * (as the reference does), each device sums its own replicas and the sums
 * are all-reduced, so z differs from the reference's single chain in
 * summation order only.
 * POLYAK_RUPPERT (6) runs synch/polyakruppert.c: acc = sum of w_i / p over
 * the locked replicas (p = cbx_num_replicas, all of them), all-reduced;
 * w_i moves towards z as above unless alpha is 0; then
 * z += (acc - z) / (clock + 1), so over clocks 0, 1, ... z is the running
 * average of the replica mean.  The base `last` buffer, where it exists,
 * is left holding acc - z; only replicas whose copy flag is raised become
 * z, and only their flag is cleared.  clock < 0 is CBX_ERR_INVALID.
 * Both use the in-order bucketed all-reduce (cbx_set_bucket_elements) at
 * G > 1, whatever cbx_set_allreduce_algorithm says.                       */
int cbx_synchronise (cbx_context *ctx, int first, int clock, int autotune, int push);
/* The same step for a model manager whose buffers live in host memory
 * (north_star: "starts and ends in host memory", databuffer.c:95-122):
 * result-identical to cbx_stage_in + cbx_synchronise + cbx_stage_out, but
 * the flat buffers are cut into `buckets` (1..4096) and the pinned H2D of
 * bucket k+1 and the D2H of bucket k-1 run beside the kernels of bucket k
 * on their own streams, so the step costs about max(H2D, D2H) of PCIe time
 * instead of the sum.  Async like cbx_synchronise; cbx_wait / the step
 * event cover the downloads.  The reference has no such call (its `push`
 * argument is unused, executioncontext.c:2264); update model WORKER runs
 * the three calls unpipelined, and so do elastic averaging and
 * POLYAK_RUPPERT.                                                         */
int cbx_synchronise_staged (cbx_context *ctx, int first, int clock, int autotune, int buckets);
/* The replicas' pending task steps and the one-GPU SMA barrier in one pass
 * over memory.  With tau = 1 every task step is followed by a barrier before
 * the replica is read again; the two calls read and write each w_i twice and
 * pass s_i through memory only for the barrier to read it back.
 *
 * tasks[id], one entry for every id in 0..cbx_num_replicas: >= 0 means replica
 * id holds a gradient in `g` that has not been applied; the call takes its
 * step for that task number and then averages it.  -1 means the replica takes
 * part in the barrier as it does in cbx_synchronise, with its s and w as they
 * are.  streams[id] is the stream on which replica id's `g` was produced; an
 * entry may be NULL (the sync stream), and so may `streams` itself.  The launch
 * is ordered behind every such stream the way cbx_synchronise is ordered behind
 * cbx_replica_optimise on a task stream.  Asynchronous like cbx_synchronise.
 *
 * The contract.  With flags == 0 the call leaves every buffer (z, the base
 * `last`, every w_i, last_i, s_i and g_i) bit for bit, and every piece of host
 * state (copy flags, clocks, `updates`, the step event, one timing-history
 * entry), as if the caller had made
 *   cbx_replica_optimise (ctx, id, tasks[id], streams[id])  for every id with
 *                                                           tasks[id] >= 0,
 *   cbx_synchronise (ctx, first, clock, autotune, 0).
 * A learning-rate query that raises a replica's copy flag (MULTISTEP at its
 * boundary) triggers Phase D in this same call, as it does in the sequence.
 *
 * With CBX_STEP_DISCARD_TASK_OUTPUTS, s_i and g_i of the stepping replicas are
 * not written at all (they keep what they held); everything else is as above.
 * In return the caller promises that such a replica steps again, through
 * either call, before it next joins a barrier with tasks[id] == -1 (or through
 * cbx_synchronise), and before anyone reads its s or g: cbx_model_stats with
 * CBX_BUF_DIFF or CBX_BUF_GRADIENT, cbx_replica_read of them, or a step
 * through the sma.c seam on those buffers.
 *
 * Everything is checked before the first side effect: a refused call changes
 * no buffer, flag or clock, and cbx_last_error names the cause.
 * CBX_ERR_INVALID: tasks is NULL; a tasks[id] < -1; an unknown flag bit; a
 * stepping replica that is not local, not locked (cbx_lock_any) or below
 * `first`.  CBX_ERR_UNSUPPORTED: more than one device, or cbx_set_force_split
 * on (kernel A of the split path is not fused); an update model other than SMA
 * (7) or SYNCHRONOUSEAMSGD (3) without elastic averaging; gradient clipping on;
 * cbx_set_variable_learning_rates on with a multiplier that is not 1; Nesterov
 * momentum on a stepping replica; stepping replicas whose momentum or weight
 * decay differ.  CBX_ERR_STATE: replica momentum without a `last` buffer.
 * A model with per-variable rates takes cbx_step_and_synchronise_variables
 * below, elastic averaging cbx_step_and_synchronise_elastic; this call keeps
 * its refusals.                                                            */
#define CBX_STEP_DISCARD_TASK_OUTPUTS 1u
int cbx_step_and_synchronise (cbx_context *ctx, int first, int clock, int autotune,
                              const int *tasks, void *const *streams, unsigned flags);
/* cbx_step_and_synchronise for a model with per-variable learning rates
 * (cbx_set_variable_learning_rates on and a multiplier that is not 1; the
 * reference's crossbowModelGetLearningRateForVariable, model.c:159-177, which
 * every optimiser of the reference honours).  Same parameters, same checks and
 * refusals in the same order and before the first side effect, except that
 * variable rates are honoured, not refused; gradient clipping stays
 * CBX_ERR_UNSUPPORTED.  A model whose variables do not tile its elements is
 * CBX_ERR_UNSUPPORTED with the reason cbx_replica_optimise gives.
 *
 * The arithmetic.  Per element of variable v and per stepping replica i
 *   r_iv = rate_i * mult[v],  rate_i = -lr_i  (one fp32 multiply, as in
 *                                              cbx_replica_optimise)
 * and then cbx_step_and_synchronise's sequence with r_iv in place of rate_i.
 * A replica that only joins, the base momentum, Phase D and
 * CBX_STEP_DISCARD_TASK_OUTPUTS are as in that call.
 *
 * The contract.  With flags == 0 every buffer and every piece of host state is
 * left bit for bit as after
 *   cbx_replica_optimise (ctx, id, tasks[id], streams[id])  (variable rates on)
 *                                     for every id with tasks[id] >= 0, in id order,
 *   cbx_synchronise (ctx, first, clock, autotune, 0).
 * With the discard flag, s_i and g_i of the stepping replicas keep what they
 * held.  The pad floats behind the model's elements step as a pseudo-variable
 * of multiplier 1: a zero pad stays zero.
 *
 * With cbx_set_variable_learning_rates off, or every multiplier 1, the call is
 * cbx_step_and_synchronise: the same kernel, the same bits.                */
int cbx_step_and_synchronise_variables (cbx_context *ctx, int first, int clock, int autotune,
                                        const int *tasks, void *const *streams, unsigned flags);
/* cbx_step_and_synchronise with gradient clipping on (cbx_set_gradient_clip):
 * every stepping replica's gradient is clipped to the global L2 norm, and a
 * step whose gradient holds a NaN or an infinity is skipped, inside the one
 * pass.  Same parameters, same checks and refusals in the same order and before
 * the first side effect, except that clipping is honoured, not refused.
 * cbx_set_variable_learning_rates on with a multiplier that is not 1 stays
 * CBX_ERR_UNSUPPORTED in this call: take
 * cbx_step_and_synchronise_clipped_variables below.  A refused call launches
 * no norm pass and bumps no counter of any record.
 *
 * The norm.  For every stepping replica, in id order, the norm pass and its
 * reduce (the launches cbx_replica_optimise makes) go on streams[id] where
 * given, else on the sync stream, in front of the fused launch, which is ordered
 * behind them.  They leave S, K, scale, the flags and the running counts in the
 * replica's cbx_clip_stats record on the device.
 *
 * The arithmetic.  Per element and per stepping replica i
 *   g = scale_i * g           one fp32 multiply, before weight decay
 * and then cbx_step_and_synchronise's sequence; scale_i and the flags are read
 * from replica i's own record on the device.  A kept g_i is always written, as
 * the clipped step writes it even without momentum and weight decay.  When the
 * record carries the skip bit, w_i as the step sees it, g_i and last_i keep
 * every bit (signalling NaNs and payloads included), s_i = w_i is a bit copy
 * (written when outputs are kept), and the replica joins the barrier with
 * s = w and w' = w.  Skipped wins over clipped.  The replicas of one call may
 * differ: one unclipped at scale 1, one clipped, one skipped, one only joining.
 *
 * The contract.  With flags == 0, z, the base `last`, every replica's w, s, g
 * and `last`, every replica's 48-byte cbx_clip_stats record (S, K, scale,
 * flags and the three running counts) and every piece of host state are left
 * bit for bit as after
 *   cbx_replica_optimise (ctx, id, tasks[id], streams[id])  (clipping on)
 *                                     for every id with tasks[id] >= 0, in id order,
 *   cbx_synchronise (ctx, first, clock, autotune, 0).
 * With CBX_STEP_DISCARD_TASK_OUTPUTS, s_i and g_i of the stepping replicas are
 * not written; everything else is as above.
 *
 * With clipping off the call is cbx_step_and_synchronise: the same kernel, the
 * same bits, and no launch for the norm.                                    */
int cbx_step_and_synchronise_clipped (cbx_context *ctx, int first, int clock, int autotune,
                                      const int *tasks, void *const *streams, unsigned flags);
/* cbx_step_and_synchronise with gradient clipping on (cbx_set_gradient_clip)
 * and per-variable learning rates (cbx_set_variable_learning_rates on and a
 * multiplier that is not 1) at once.  Same parameters, same checks and
 * refusals in the same order and before the first side effect, except that
 * neither of the two is refused.  A model whose variables do not tile its
 * elements, a padded model too large for the chunk table and a stepping replica
 * without clip scratch stay refused.  A refused call launches no norm pass and
 * bumps no counter of any record.
 *
 * The norm passes are cbx_step_and_synchronise_clipped's: per stepping replica
 * in id order on streams[id] where given, else on the sync stream, in front of
 * the fused launch.
 *
 * The arithmetic.  Per element of variable v and per stepping replica i, one
 * fp32 operation each:
 *   g = scale_i * g                      the record's scale, before weight decay
 *   g = fma (wd, w, g)                   (wd > 0)
 *   s = w
 *   r_iv = rate_i * mult[v]              rate_i = -lr_i
 *   g = r_iv * g; g = fma (mu, last_i, g); last_i = g; w' = fma (1, g, w)   (momentum)
 *   w' = fma (r_iv, g, w)                                                   (none)
 * With the record's skip bit, s_i = w_i is a bit copy and w_i, g_i and last_i
 * keep every bit.  Skipped wins over clipped.  A kept g_i is always written.
 * Then the barrier of cbx_step_and_synchronise for every participating replica,
 * Phase D in the same launch.
 *
 * The contract.  With flags == 0, z, the base `last`, every replica's w, s, g
 * and `last`, every replica's cbx_clip_stats record and every piece of host
 * state are left bit for bit as after
 *   cbx_replica_optimise (ctx, id, tasks[id], streams[id])  (both on)
 *                                     for every id with tasks[id] >= 0, in id order,
 *   cbx_synchronise (ctx, first, clock, autotune, 0).
 * With CBX_STEP_DISCARD_TASK_OUTPUTS, s_i and g_i of the stepping replicas are
 * not written.
 *
 * With clipping on and every multiplier 1 (or variable rates off) the call is
 * cbx_step_and_synchronise_clipped; with clipping off it is
 * cbx_step_and_synchronise_variables; with both off, cbx_step_and_synchronise:
 * the same kernel, the same bits.  When no replica steps there is no norm pass
 * and no record is touched.                                                 */
int cbx_step_and_synchronise_clipped_variables (cbx_context *ctx, int first, int clock, int autotune,
                                                const int *tasks, void *const *streams, unsigned flags);
/* The pending task steps of the locked replicas and the one-GPU
 * elastic-averaging barrier in one launch: cbx_step_and_synchronise for EA-SGD
 * (update model SYNCHRONOUSEAMSGD (3) with cbx_set_elastic_average on; the
 * reference's ELASTIC_AVERAGE build, kernels/optimisers/synchronouseamsgd.cu
 * and synch/synchronouseamsgd.c:42-90), which the four calls above refuse.
 * Same parameters: tasks[id] is replica id's task number, or -1 when it only
 * joins the barrier; streams[id] the stream its gradient was produced on (NULL:
 * the sync stream), behind which the launch is ordered.  Asynchronous.
 *
 * The arithmetic.  Per element and per participating replica i (locked, id >=
 * first) in ascending id order, one fp32 operation per reference call:
 *   stepping (tasks[id] >= 0), rate_i = -learning_rate (conf_i, tasks[id]):
 *     g = fma (wd, w, g)                                            (wd > 0)
 *     s = w                                                         (outputs kept)
 *     g = rate_i * g; g = fma (mu, last_i, g); last_i = g; w' = fma (1, g, w)   (mu > 0)
 *     w' = fma (rate_i, g, w)                                                   (mu = 0)
 *   only joining: w' = w_i
 *   all: d = fma (-1, z, w'); w_i = fma (-alpha, d, w'); acc = fma (alpha, d, acc)
 * then z = fma (1, acc, z), acc starting from +0.  d is taken from the stepped
 * w', not from a snapshot; there is no base momentum (the base `last` is not
 * touched) and no Phase D: copy flags are neither read nor cleared, so a
 * learning-rate query of this call that raises a replica's copy flag
 * (MULTISTEP at its boundary) leaves it raised, as the sequence does.
 *
 * The contract.  With flags == 0 the call leaves every buffer (z, every w_i,
 * last_i, s_i and g_i) bit for bit, and every piece of host state (copy flags,
 * clocks, `updates`, the step event, one timing-history entry), as if the
 * caller had made
 *   cbx_replica_optimise (ctx, id, tasks[id], streams[id])  for every id with
 *                                                           tasks[id] >= 0,
 *   cbx_synchronise (ctx, first, clock, autotune, 0).
 * With CBX_STEP_DISCARD_TASK_OUTPUTS, s_i and g_i of the stepping replicas are
 * not written at all; this barrier never reads s_i, so the promise that goes
 * with the flag is only that nobody else reads them before the replica steps
 * again.  When nobody steps the call is cbx_synchronise under elastic averaging.
 *
 * Everything is checked before the first side effect: a refused call changes
 * no buffer, flag or clock, and cbx_last_error names the cause.
 * CBX_ERR_INVALID: as cbx_step_and_synchronise.  CBX_ERR_UNSUPPORTED: more than
 * one device, or cbx_set_force_split on; an update model other than
 * SYNCHRONOUSEAMSGD (3) with elastic averaging on (plain SMA takes
 * cbx_step_and_synchronise); gradient clipping on, or
 * cbx_set_variable_learning_rates on with a multiplier that is not 1 (both take
 * cbx_step_and_synchronise_elastic_clipped_variables below); Nesterov
 * momentum on a stepping replica; stepping replicas whose momentum or weight
 * decay differ.  CBX_ERR_STATE: replica momentum without a `last` buffer.
 * The launch shape is cbx_set_task_barrier_kernel_config's.                 */
int cbx_step_and_synchronise_elastic (cbx_context *ctx, int first, int clock, int autotune,
                                      const int *tasks, void *const *streams, unsigned flags);
/* cbx_step_and_synchronise_elastic for an EA-SGD context with gradient clipping
 * (cbx_set_gradient_clip), per-variable learning rates
 * (cbx_set_variable_learning_rates with a multiplier that is not 1), or both:
 * what cbx_step_and_synchronise_clipped_variables is to the SMA barrier.  The
 * parameters, the checks and their order are cbx_step_and_synchronise_elastic's;
 * neither feature is refused.  Asynchronous.
 *
 * The norm passes are cbx_step_and_synchronise_clipped's: with clipping on, per
 * stepping replica in id order on streams[id] where given, else on the sync
 * stream, in front of the fused launch.  When no replica steps there is no norm
 * pass and no record is touched.
 *
 * The arithmetic.  Per element of variable v and per participating replica i in
 * ascending id order, one fp32 operation each:
 *   stepping (tasks[id] >= 0), rate_i = -learning_rate (conf_i, tasks[id]):
 *     g = scale_i * g                      clipping on: the record's scale, before weight decay
 *     g = fma (wd, w, g)                   (wd > 0)
 *     s = w                                (outputs kept)
 *     r = rate_i * mult[v]                 per-variable rates on; else r = rate_i
 *     g = r * g; g = fma (mu, last_i, g); last_i = g; w' = fma (1, g, w)   (mu > 0)
 *     w' = fma (r, g, w)                                                   (mu = 0)
 *     With the record's skip bit, s_i = w_i is a bit copy, g_i and last_i keep
 *     every bit and w' = w_i.  Skipped wins over clipped.  With clipping on a
 *     kept g_i is always written.
 *   only joining: w' = w_i
 *   all: d = fma (-1, z, w'); w_i = fma (-alpha, d, w'); acc = fma (alpha, d, acc)
 * then z = fma (1, acc, z), acc starting from +0.  No base momentum and no
 * Phase D, as in cbx_step_and_synchronise_elastic: copy flags are neither read
 * nor cleared.
 *
 * The contract.  With flags == 0, z, every replica's w, s, g and `last`, every
 * replica's cbx_clip_stats record and every piece of host state are left bit
 * for bit as after
 *   cbx_replica_optimise (ctx, id, tasks[id], streams[id])  (the same features on)
 *                                     for every id with tasks[id] >= 0, in id order,
 *   cbx_synchronise (ctx, first, clock, autotune, 0)
 * under update model 3 with elastic averaging on.  With
 * CBX_STEP_DISCARD_TASK_OUTPUTS, s_i and g_i of the stepping replicas are not
 * written.  It moves (28R + 8) n bytes, (20R + 8) n with the discard flag, where
 * the sequence moves (36R + 8) n; the norm passes add 4R n to each.
 *
 * With one feature off the call launches the kernel of the other; with both
 * off, or with clipping alone and nobody stepping, it is
 * cbx_step_and_synchronise_elastic: the same kernel, the same bits.
 *
 * Everything is checked before the first side effect: a refused call launches
 * no norm pass and changes no buffer, flag, clock or record.  The refusals are
 * cbx_step_and_synchronise_elastic's without the two features, and
 * CBX_ERR_UNSUPPORTED with per-variable rates on for a model whose variables do
 * not tile its elements and for a padded model too large for the chunk table;
 * CBX_ERR_STATE for a stepping replica without clip scratch.                 */
int cbx_step_and_synchronise_elastic_clipped_variables (cbx_context *ctx, int first, int clock, int autotune,
                                                        const int *tasks, void *const *streams, unsigned flags);
/* The pending task steps of the locked replicas and the one-GPU
 * synchronous-SGD barrier in one launch: cbx_step_and_synchronise for update
 * model WORKER (1; kernels/optimisers/synchronoussgd.cu:3-56 and
 * synch/synchronoussgd.c:13-106 with common.c:198-220), which the calls above
 * refuse.  Same parameters: tasks[id] is replica id's task number, or -1 when it
 * only joins the barrier; streams[id] the stream its gradient was produced on
 * (NULL: the sync stream), behind which the launch is ordered.  Asynchronous.
 *
 * The arithmetic.  Per element, one fp32 operation per reference call:
 *   acc = the device's base gradient as the call finds it (not assumed zero)
 *   per stepping replica i (tasks[id] >= 0) in ASCENDING ID ORDER,
 *   rate_i = -learning_rate (conf_i, tasks[id]):
 *     gv = g_i
 *     gv = fma (wd, w_i, gv); g_i = gv              (wd > 0; g_i written with outputs kept)
 *     acc = fma (rate_i, gv, acc)
 *   D = ratio * acc, a plain multiply, ratio = (float) (1.0 / (double) (float) wpc)
 *   D = fma (mu, last, D); last = D                 (base momentum mu > 0: the model's, not 0.9)
 *   z = fma (1, D, z)
 *   base gradient = +0
 *   w_i = z for every participating replica (locked, id >= first), stepping or
 *   only joining.
 * The accumulator depends on the order of its additions: the sequence below adds
 * in enqueue order, so it is the sequence in ascending id order that this call
 * equals.  w_i of a stepping replica is read only when wd > 0, before it is
 * overwritten; a replica that only joins is one written buffer, its g, s and
 * last are not read.  Replica momentum, s, the per-variable multipliers
 * (cbx_set_variable_learning_rates) and the copy flags play no part, as in
 * cbx_replica_optimise and cbx_synchronise under WORKER; a learning-rate query
 * of this call that raises a replica's copy flag (MULTISTEP at its boundary)
 * leaves it raised, as the sequence does.
 *
 * The contract.  With flags == 0 the call leaves every buffer (z, the base
 * `last` and gradient, every w_i, g_i, s_i and last_i) bit for bit, and every
 * piece of host state (copy flags, clocks, `updates`, the step event, one
 * timing-history entry), as if the caller had made, on one device,
 *   cbx_replica_optimise (ctx, id, tasks[id], streams[id])  for every id with
 *                                       tasks[id] >= 0, in ascending id order,
 *   cbx_synchronise (ctx, first, clock, autotune, 0).
 * With CBX_STEP_DISCARD_TASK_OUTPUTS, g_i of the stepping replicas is not
 * written; that differs from the sequence only when wd > 0 (without weight
 * decay the step writes no g_i and the flag selects the same kernel).  The
 * promise that goes with the flag is cbx_step_and_synchronise's: nobody reads
 * g_i before the replica's next gradient overwrites it.  When nobody steps the
 * call is cbx_synchronise under WORKER.
 *
 * Everything is checked before the first side effect: a refused call changes
 * no buffer, flag or clock, and cbx_last_error names the cause and the calls to
 * take instead.  CBX_ERR_INVALID: as cbx_step_and_synchronise, and first.
 * CBX_ERR_UNSUPPORTED: more than one device, or cbx_set_force_split on; an
 * update model other than WORKER; gradient clipping on; Nesterov momentum
 * (momentumMethod 1) on a stepping replica; stepping replicas whose weight
 * decay differs; more than 64 participating replicas; a learning-rate policy
 * the library does not have.  CBX_ERR_STATE: no work per clock (wpc <= 0); a
 * STEP policy with size 0 or an LSR policy without warm-up tasks, refused
 * before any replica's query has raised a flag.
 * The launch shape is cbx_set_task_barrier_kernel_config's.                 */
int cbx_step_and_synchronise_ssgd (cbx_context *ctx, int first, int clock, int autotune,
                                   const int *tasks, void *const *streams, unsigned flags);
/* TheGPU.unlockAny() GPU.c:1142-1149 -> modelmanager.c:233-245           */
int cbx_unlock_any (cbx_context *ctx);

/* ---- checkpoint / resume ---------------------------------------------- */
/* TheGPU.checkpointModel(String)   GPU.c:1151-1163 -> executioncontext.c:2340-2367.
 * Waits as cbx_wait does, so it refuses (CBX_ERR_STATE) to store a model a
 * poisoned peer-read step left undefined (cbx_peer_import below). */
int cbx_checkpoint_model (cbx_context *ctx, const char *dir);
/* TheGPU.overrideModelData(String) GPU.c:1165-1176 -> executioncontext.c:2369-2388.
 * Drains the streams without that check: loading a checkpoint is a way back. */
int cbx_override_model_data (cbx_context *ctx, const char *dir);
/* Batch-norm running statistics in the checkpoint.  After the model files,
 * executioncontext.c:2352-2364 / 2375-2386 walk the dataflow's BATCHNORM
 * operators and call crossbowCudnnBatchNormParams{Store,Load}Estimated-
 * MeanAndVariable (cudnn/cudnnbatchnormparams.c:102-143) with the
 * operator's id.  The dataflow stays with the caller, so it registers each
 * BN operator's buffers here once (where executioncontext.c:1280-1290 sets
 * them per device); cbx_checkpoint_model / cbx_override_model_data then
 * store / load gpu-%02d-bn-avg-%03d.dat and gpu-%02d-bn-var-%03d.dat
 * (global device id, op id; raw fp32, `elements` floats) in the same
 * directory as the model files.  mean/variance[k]: device pointers on
 * LOCAL device k; a device whose pair is both NULL holds no copy and is
 * skipped (:110-111).  Registering an op again replaces it; elements == 0
 * removes it.                                                             */
int cbx_register_batchnorm_stats (cbx_context *ctx, int op, int elements,
		float *const *mean, float *const *variance);
/* TheGPU.addModel() / delModel()   GPU.c:1178-1199 (autotune; also called
 * by cbx_synchronise for autotune > 0 / < 0, executioncontext.c:2321-2328).
 * add: one new replica per device, ids size .. size+G-1 (id size+g on device
 * g), each a copy of device g's first replica (all four buffers and its
 * solver state, modelmanager.c:362-470, model.c:202-306), left locked for the
 * barrier's unlockAny.  New buffers get their own allocation: pointers
 * returned earlier stay valid.  del: drops ids size-G .. size-1
 * (modelmanager.c:473-557); CBX_ERR_STATE if that would leave none.      */
int cbx_add_model (cbx_context *ctx);
int cbx_del_model (cbx_context *ctx);

/* ---- model statistics and replica divergence --------------------------- */
/* The reference can only checksum a buffer on the host, with a loop on every
 * store and load (clib-multigpu/databuffer.c:141-162, called at :218 and
 * :255, behind its COMPUTE_CHECKSUM debug switch).  Here one pass over HBM
 * reduces the base model and every local replica on the device, per model
 * variable and per buffer (crossbow_amd/csrc/stats_kernels.hip).  Sums are
 * accumulated in fp64 from the first add, in an order that depends on the
 * variable list alone: two calls on the same data return the same bits.    */
typedef struct cbx_buffer_stats {
  double sum;                   /* sum of x over finite x                        */
  double sum_sq;                /* sum of x*x over finite x                      */
  double dist_sq;               /* sum of (x - ref)^2 where x and ref are both finite;
                                   0 for the reference buffer itself            */
  unsigned long long nonfinite; /* NaN or +-inf among x                          */
  float  max_abs;               /* max |x| over finite x, 0 if there is none     */
  unsigned int reserved;        /* 0                                             */
} cbx_buffer_stats;             /* 40 bytes, no implicit padding                 */
/* The registered variables in ascending offset order; index v below is the
 * position in that order.  A model registered as raw bytes (no variables),
 * or one whose variables do not tile its elements (a capacity above its
 * shape's bytes), reports one variable: op -1, order 0, every element.
 * CBX_ERR_STATE before cbx_set_model_manager.                             */
int cbx_model_variable_count (cbx_context *ctx, int *count);
int cbx_model_variable_info (cbx_context *ctx, int v, int *op, int *order,
		long long *offset_elements, long long *elements);
/* kind CBX_BUF_DATA measures every w against z, CBX_BUF_DIFF every s against
 * z (anything else: CBX_ERR_INVALID).  base[k]: z of local device k (dist_sq
 * 0); replicas[id] for every id in 0..cbx_num_replicas, zeroed for a replica
 * of another process; base_vars[k * V + v] and replica_vars[id * V + v] the
 * same per variable (V = cbx_model_variable_count; either may be NULL).
 * Blocking: drains the library's streams as the checkpoint does (no poison
 * check: looking at a damaged model is its job, so a broken peer-read step
 * does not refuse it), launches on each local device's sync stream and
 * returns with the numbers on the host.  It only reads model buffers, so a
 * cross-step pipeline stays valid.  Every local replica is covered, locked
 * or not: a caller who wants consistent numbers calls it between
 * cbx_lock_any and cbx_unlock_any.                                        */
int cbx_model_stats (cbx_context *ctx, int kind, cbx_buffer_stats *base, cbx_buffer_stats *replicas,
		cbx_buffer_stats *base_vars, cbx_buffer_stats *replica_vars);
/* Device milliseconds of the last cbx_model_stats on local device `local`,
 * from the dispatches' own timestamps: the pass over memory alone, and the
 * pass with its two reductions; -1 before the first call.                 */
int cbx_model_stats_last_ms (cbx_context *ctx, int local, float *pass_ms, float *total_ms);
/* Checkpoint guard, default off.  When on, cbx_checkpoint_model first runs
 * the reduction over z and every local w (and over the base and replica
 * `last` when momentum > 0) and, if any holds a non-finite value, returns
 * CBX_ERR_STATE naming the first such buffer and variable; it then creates
 * no directory and does not advance the version numbering.                */
int cbx_set_checkpoint_guard (cbx_context *ctx, int enable);

/* ---- batch-norm running statistics ----------------------------------- */
/* crossbowCudnnBatchNormParamsSynchroniseEstimatedMeanAndVariable
 * (cudnn/cudnnbatchnormparams.c:157-222; its caller is commented out at
 * executioncontext.c:2268, so this is opt-in), for `layers` BN layers in
 * one all-reduce.  mean/variance[k * layers + l] are device pointers of
 * layer l (elements[l] floats) on LOCAL device k; updated[k * layers + l]
 * is that layer's "updates > 0" on that device.  Per layer, the default
 * device (global device 0) always counts and every other device counts iff
 * updated; every device ends with (sum of counted) / count (unscaled when
 * count == 1).  No-op with one device (:165-166).  Device-synchronises
 * before and after, as the reference does (:171, :218).  The sum order is
 * RCCL's, not device order: equal to the reference within fp32 rounding. */
int cbx_average_batchnorm_stats (cbx_context *ctx, int layers, const int *elements,
		float *const *mean, float *const *variance, const int *updated);

/* ---- task-side replica access (modelmanager.c:147-204) ---------------- */
int cbx_replica_lock (cbx_context *ctx, int id);       /* crossbowModelManagerGet   */
int cbx_replica_unlock (cbx_context *ctx, int id);     /* crossbowModelManagerRelease */
int cbx_replica_task_done (cbx_context *ctx, int id);  /* callbackhandler.c:149-165: updates++ */
int cbx_replica_clock (cbx_context *ctx, int id);
/* crossbowSolverConfGetLearningRate (solverconfiguration.c:116-162) on the
 * replica's own configuration: may raise its _copy flag (LR drop).        */
int cbx_replica_learning_rate (cbx_context *ctx, int id, int task, float *rate);
int cbx_replica_get_copy (cbx_context *ctx, int id);
int cbx_replica_set_copy (cbx_context *ctx, int id, int flag);
/* ---- the theta queue: which replica a task runs on -------------------- */
/* The model manager's theta queue (thetaqueue.c, modelmanager.c:121-132)
 * has one slot per replica id: free, reserved by a task, or disabled.
 * TheGPU.acquireAccess([I)  GPU.c:888-903 -> modelmanager.c:180-190:
 * reserve the next enabled replica of this process in round-robin order,
 * waiting (spinning) until it is free; returns its id and sets *clock to
 * its clock.  CBX_ERR_STATE if every replica here is disabled (the
 * reference spins forever).                                              */
int cbx_acquire_access (cbx_context *ctx, int *clock);
/* TheGPU.upgradeAccess(Integer,[I)  GPU.c:905-921 -> modelmanager.c:192-198:
 * refresh *clock of a reserved replica and return 1, or return 0 (Java
 * null: the task processor re-acquires) once that replica is gone.       */
int cbx_upgrade_access (cbx_context *ctx, int id, int *clock);
/* crossbowModelManagerGetNextOrWait (modelmanager.c:147-167), the execute
 * paths that pick the replica natively (executioncontext.c:2018, 2130):
 * reserve the next replica, wait until its clock >= bound, lock it.
 * Returns its id.  Blocks until a barrier advances the clock.            */
int cbx_get_next_or_wait (cbx_context *ctx, int bound);
/* crossbowModelManagerRelease (modelmanager.c:200-204), from the callback
 * handler after a task (callbackhandler.c:155): unlock the replica and free
 * its theta slot.  CBX_ERR_STATE if the slot is not reserved.             */
int cbx_replica_release (cbx_context *ctx, int id);
/* Disable (flag 1) or re-enable (0) a replica's theta slot
 * (crossbowThetaQueueDisable / Enable, thetaqueue.c:182-206; delModel
 * disables the slots of the replicas it removes).  lockAny then counts it,
 * so BSP still holds, but does not lock it, so the step, unlockAny and the
 * clock leave it alone (modelmanager.c:217-222).  Disabling returns 0, or 1
 * when a task holds the reservation (the slot stays enabled, :199-201);
 * enabling a reserved slot is CBX_ERR_STATE (:182-184).                   */
int cbx_replica_set_disabled (cbx_context *ctx, int id, int flag);
/* crossbowKernelOptimiserSMA (kernels/optimisers/sma.cu:3-100), fused into
 * one pass: the replica's local step for task `task`, which produces the
 * snapshot s (replica->diff) and the new w that the next synchronise()
 * averages.  The learning rate comes from the replica's solver
 * configuration (may raise its _copy flag, solverconfiguration.c:133,147).
 * Enqueued on `stream` (a hipStream_t; NULL = the replica device's sync
 * stream); the sync stream waits for it (sma.cu:79-81) from the library's
 * next call that works on the device (synchronise, wait, staging, reads,
 * writes, add / del, free): the wait is queued then, not at once, so it is
 * not pending on another hardware queue while the update runs.
 * The library keeps one event per caller stream with an update whose wait
 * it has not yet seen complete: a stream it has not seen first drops the
 * entries whose event has completed (their update is done), so task
 * streams that come and go leave nothing behind; at 64 entries per device
 * the pending waits are queued on the sync stream at once (and, if that
 * frees none, the oldest entry's event is waited for on the host).
 * cbx_task_wait_count reports the table's size.  Nesterov
 * momentum is CBX_ERR_UNSUPPORTED, as in the reference (sma.cu:46-48).
 * Under update model WORKER the step is crossbowKernelOptimiserSynchronousSGD
 * (synchronoussgd.cu:3-56) instead: weight decay, then the lr-scaled
 * gradient is added into the device's base-model gradient on the sync
 * stream, to be all-reduced and applied at the next barrier.  Under
 * DEFAULT it is crossbowKernelOptimiserDefault (default.cu:3-131): the
 * replica and its device's base model take the same step, in one pass on
 * the sync stream (the task stream waits for it).  Elastic averaging
 * (SYNCHRONOUSEAMSGD with cbx_set_elastic_average) keeps the SMA step: the
 * reference's optimisers/synchronouseamsgd.cu is the same call sequence.
 * POLYAK_RUPPERT has no step here (CBX_ERR_UNSUPPORTED): the reference's
 * optimisers/polyakruppert.cu is a stub, so the caller brings its own local
 * step and updates the replica's data itself.
 * With cbx_set_variable_learning_rates on (SMA and SYNCHRONOUSEAMSGD only)
 * and a multiplier other than 1 registered, every variable steps with its
 * own rate: see there.                                                     */
int cbx_replica_optimise (cbx_context *ctx, int id, int task, void *stream);
/* The per-operator step, crossbowStreamSynchronousEamsgdModelUpdate
 * (stream.c:422-479): cbx_replica_optimise's step on the variables
 * registered under operator `op` only (orders 1..count), so that the update
 * of layer k can overlap the backward pass of layer k-1.  It always steps
 * with the per-variable rate (multipliers apply iff conf.irregular > 0,
 * model.c:167), whatever cbx_set_variable_learning_rates says.  Floats
 * outside those variables are not written, not even with their own value,
 * so steps of different operators may run on different streams.  Variables
 * that are neighbours in the buffer share one launch, else one launch per
 * run of neighbours.  g and last keep sma.cu's sign (they hold the
 * negative-rate values; stream.c:455-467 scales by +rate and subtracts: the
 * same w, g and last of the opposite sign), so whole-model and per-operator
 * steps mix on one replica; the snapshot s = w is taken per element here
 * too.  Everything cbx_replica_optimise does around its launch happens per
 * call: the learning-rate query (idempotent for a repeated `task`), the
 * wait for the last barrier, the deferred sync-stream wait, the Nesterov
 * and missing-`last` refusals.  An operator without variables is CBX_OK
 * without a launch (stream.c:499-501); `op` out of range is
 * CBX_ERR_INVALID; WORKER, DEFAULT and POLYAK_RUPPERT are
 * CBX_ERR_UNSUPPORTED, and so is a model without variable ranges
 * (cbx_set_variable_learning_rates).                                       */
int cbx_replica_optimise_variables (cbx_context *ctx, int id, int task, int op, void *stream);

/* ---- gradient clipping by global norm, non-finite skip ----------------- */
/* An extension: the reference has no gradient clipping.  Opt-in, off by
 * default; off, cbx_replica_optimise is exactly the step above (no extra
 * launch, the same kernels).  On, every cbx_replica_optimise under SMA (7) or
 * SYNCHRONOUSEAMSGD (3), one rate or per-variable rates, first reduces the
 * replica's gradient on the device, on the caller's stream, with no host
 * round trip (crossbow_amd/csrc/clip_kernels.hip).  Per call, with
 * c = max_norm and g the replica's gradient as the backward pass left it,
 * over exactly the model's n floats (a buffer's pad is never read):
 *   1. S = sum of (double)g_i * (double)g_i over finite g_i, accumulated in
 *      fp64 from the first add in an order that is a fixed function of n
 *      alone (never of the CU count, cbx_set_aux_kernel_config or the
 *      stream); K = the count of non-finite g_i.
 *   2. clipped = c > 0 && S > (double)c * (double)c (the product is exact,
 *      the decision takes no square root);
 *      scale = clipped ? (float)((double)c / sqrt (S)) : 1.0f.
 *   3. skipped = skip_nonfinite && K > 0.
 *   4. Not skipped: g_i = scale * g_i, one fp32 multiply before weight decay
 *      (clipping acts on the raw gradient), then the step's sequence
 *      unchanged; g is written back.  With scale == 1.0f the result is bit
 *      for bit the plain step's.  A non-finite g_i with skip_nonfinite == 0
 *      propagates exactly as it does in the plain step.
 *   5. Skipped: s = w is still written (the snapshot says "no local
 *      movement", what the next barrier's d = s - z must see); w, g and last
 *      are not written at all.
 *   6. The replica's record on the device is updated: the last S, K, scale,
 *      flags, and running counts (a step both clipped and skipped counts in
 *      both).  Steps of one replica are ordered by the caller, as for w and g.
 * The host side of the step (learning-rate query, _copy, the Nesterov and
 * missing-`last` refusals, the deferred sync-stream wait) happens exactly as
 * in the plain step, also for a skipped one.
 * max_norm == 0: no clipping; both arguments 0: off.  A negative, NaN or
 * infinite max_norm, or a flag other than 0 / 1, is CBX_ERR_INVALID.  May be
 * called before or after cbx_set_model_manager.  While the feature is on,
 * cbx_replica_optimise_variables is CBX_ERR_UNSUPPORTED (the global norm does
 * not exist until every operator's gradient does), and so is
 * cbx_replica_optimise under WORKER and DEFAULT.  With several devices per
 * context every local device's replicas carry their own record and slab; that
 * path has not run on several devices.                                      */
int cbx_set_gradient_clip (cbx_context *ctx, float max_norm, int skip_nonfinite);
#define CBX_CLIP_CLIPPED 1u     /* cbx_clip_stats.flags: the last step was scaled   */
#define CBX_CLIP_SKIPPED 2u     /*                       the last step was skipped  */
typedef struct cbx_clip_stats {
  double sum_sq;                    /* S of the last step                            */
  unsigned long long nonfinite;     /* K of the last step                            */
  float  scale;                     /* the last step's scale (1 when not clipped)    */
  unsigned int flags;               /* CBX_CLIP_CLIPPED | CBX_CLIP_SKIPPED           */
  unsigned long long steps;         /* steps taken with the feature on               */
  unsigned long long clipped_steps; /* of those, clipped                             */
  unsigned long long skipped_steps; /* of those, skipped                             */
} cbx_clip_stats;                   /* 48 bytes, no implicit padding                 */
/* Blocking: drains as cbx_replica_read does, then copies replica `id`'s
 * record back.  All zeros before the replica's first step with the feature
 * on.                                                                       */
int cbx_replica_clip_stats (cbx_context *ctx, int id, cbx_clip_stats *out);
/* Entries in local device `local`'s table of deferred task-stream waits
 * (see cbx_replica_optimise; at most 64). */
int cbx_task_wait_count (cbx_context *ctx, int local);
/* Global device index a replica lives on (id % G). */
int cbx_replica_device (cbx_context *ctx, int id);
/* 1 if the replica lives in this process. */
int cbx_replica_is_local (cbx_context *ctx, int id);

int cbx_num_replicas (cbx_context *ctx);       /* R * G (modelmanager->size) */
int cbx_num_devices (cbx_context *ctx);        /* G, all ranks               */
int cbx_num_local_devices (cbx_context *ctx);
int cbx_local_device_index (cbx_context *ctx, int local); /* global index    */
long long cbx_model_elements (cbx_context *ctx);

/* ---- buffers ---------------------------------------------------------- */
/* Device pointers (for the task-side kernels that produce w and s).       */
int cbx_replica_buffer (cbx_context *ctx, int id, int kind, void **dev_ptr);
int cbx_base_buffer (cbx_context *ctx, int device, int kind, void **dev_ptr);
/* Blocking copies of a whole buffer (model->bytes) to/from host memory.   */
int cbx_replica_write (cbx_context *ctx, int id, int kind, const void *src, size_t bytes);
int cbx_replica_read (cbx_context *ctx, int id, int kind, void *dst, size_t bytes);
int cbx_base_write (cbx_context *ctx, int device, int kind, const void *src, size_t bytes);
int cbx_base_read (cbx_context *ctx, int device, int kind, void *dst, size_t bytes);

/* Pinned-host staging of the synchronisation buffers (databuffer.c:95-122).
 * stage_in pushes z, last, s_i, w_i; stage_out pulls z, last, w_i.  Async on
 * the sync stream(s); host views are the pinned mirrors below.            */
int cbx_stage_in (cbx_context *ctx);
int cbx_stage_out (cbx_context *ctx);
int cbx_replica_host_buffer (cbx_context *ctx, int id, int kind, void **host_ptr);
int cbx_base_host_buffer (cbx_context *ctx, int device, int kind, void **host_ptr);
/* Block until every local sync stream has drained.  One process per GPU
 * with the peer-read form imported: CBX_ERR_STATE if a drained step on this
 * rank may have read a failed rank's buffers (its poison check found a
 * broken word, cbx_peer_import below): this rank's z and last are then
 * undefined, until cbx_resync_base. */
int cbx_wait (cbx_context *ctx);
/* The event (a hipEvent_t, as void*) recorded on local device `local`'s sync
 * stream at the end of every synchronise(): it stands for the reference's
 * base->updated, synched[dev] and each locked replica's replica->updated
 * (sma.c:115,177,204,222), which this pipeline completes at the same point.
 * Task-side streams wait on it before using a replica again.  Query it
 * after each synchronise(): with timing on it is the stop event the step's
 * last dispatch timestamps (no extra marker), so the handle changes.      */
int cbx_step_event (cbx_context *ctx, int local, void **event);

/* ---- measurement ------------------------------------------------------ */
#define CBX_T_KERNEL    0   /* fused kernel, or kernel A (G > 1)       */
#define CBX_T_ALLREDUCE 1   /* RCCL all-reduce (G > 1)                 */
#define CBX_T_APPLY     2   /* kernel B (G > 1)                        */
#define CBX_T_STEP      3   /* whole synchronise() on the device (staged: incl. copies) */
#define CBX_T_H2D       4   /* last cbx_stage_in, or uploads of the last staged step   */
#define CBX_T_D2H       5   /* last cbx_stage_out, or downloads of the last staged step */
#define CBX_T_COUNT     6
/* When enabled, HIP events bracket each launch on the sync stream.       */
int cbx_set_timing (cbx_context *ctx, int enable);
/* Stream-order check, a debug aid (event-ordering assertions).
 * When on (it turns timing on too), every split step -- kernel A /
 * collective / kernel B per bucket, G > 1 or forced -- records per-bucket
 * timestamps of its last two steps.  cbx_check_order then blocks on them
 * and verifies, per device, that each bucket's collective started after
 * its kernel A ended, that kernel B started after its collective and after
 * the previous B, and that the later step's kernel A(k) started after the
 * earlier step's B(k) (or its last B, when the later step joined the whole
 * stream).  Returns the number of steps checked (0..2 per device), or
 * CBX_ERR_STATE naming the first violation.  Checked steps are consumed; to
 * check cross-step overlap, run two steps back to back between checks.
 * The peer-read and host-staged steps are not recorded.                   */
int cbx_set_order_check (cbx_context *ctx, int enable);
int cbx_check_order (cbx_context *ctx);
/* Milliseconds of the last step on local device `local`, CBX_T_COUNT floats
 * (blocks on the recorded events); -1 for a span the step did not have.   */
int cbx_last_timing (cbx_context *ctx, int local, float *ms);
/* Per-launch history of the last steps (up to 1024) on local device `local`:
 * `which` is CBX_T_KERNEL, CBX_T_ALLREDUCE, CBX_T_APPLY or CBX_T_STEP; fills
 * ms[0..count) oldest first and returns count.  For a pipelined split step
 * (2..64 buckets, order check off; the last 64 such steps) KERNEL, ALLREDUCE
 * and APPLY are the step's summed busy spans of kernels A, collectives and
 * kernels B: each dispatch's stop minus the latest event that bounded its
 * start (the previous dispatch on its stream, the events the stream waited
 * on), so each includes its dispatch latency and any sharing of the GPU
 * with the other streams' work.  Both this and cbx_last_timing report -1
 * for a span a step did not keep.                                         */
int cbx_timing_history (cbx_context *ctx, int local, int which, float *ms, int max);
/* Launch geometry for the SMA kernels: threads per block (multiple of 64),
 * workgroups per CU for the grid-stride loop (0 = one float4 per thread),
 * load/store policy (0 plain, 1 nontemporal), float4s per thread per trip. */
int cbx_set_kernel_config (cbx_context *ctx, int block, int blocks_per_cu, int policy, int unroll);
/* Occupancy cap for the SMA kernels, in waves per CU: 1..32, 0 = none, -1
 * = auto (the default: about 56 buffer streams, reads plus writes, in
 * flight per CU, i.e. 2 waves for the R = 8 step, 11 for kernel B, 8 for
 * the optimiser step).  Enforced through reserved LDS per
 * workgroup (so the smallest reachable cap is 2 workgroups per CU).      */
int cbx_set_kernel_occupancy (cbx_context *ctx, int waves_per_cu);
/* Launch geometry of the per-task kernels (the replica optimiser step and
 * the S-SGD task/barrier kernels): threads per block (64..512, multiple of
 * 64), float4s per lane (1 or 2), occupancy cap in waves per CU as above. */
int cbx_set_aux_kernel_config (cbx_context *ctx, int block, int unroll, int waves_per_cu);
/* Launch geometry of the write-heavy barrier kernels (the DEFAULT broadcast
 * and the S-SGD apply), same arguments as above; defaults are per kernel
 * (256 / 1 / 8 and 64 / 2 / 3, measured).                                */
int cbx_set_barrier_kernel_config (cbx_context *ctx, int block, int unroll, int waves_per_cu);
/* Launch geometry of kernel B of the G > 1 split SMA path (Phase C,
 * sma.c:135-183: 3 reads + 2 writes per element): block 64..256, unroll 1,
 * 2 or 4, occupancy cap as above.  Default 64 / 2 / auto.                 */
int cbx_set_apply_kernel_config (cbx_context *ctx, int block, int unroll, int waves_per_cu);
/* Launch geometry of the fused and accumulate-only kernels of the
 * elastic-averaging and Polyak-Ruppert barriers (R + 1 or 2R + 1 reads,
 * R + 1 or R + 2 writes per element): block 64..256, unroll 1, 2 or 4,
 * occupancy cap as above.  Default 64 / 1 / auto (4 waves per CU at R = 8,
 * measured: scripts/bench_averaging.py --sweep).  Their apply kernel at
 * G > 1 follows cbx_set_apply_kernel_config, and all of them the load/store
 * policy of cbx_set_kernel_config.                                         */
int cbx_set_averaging_kernel_config (cbx_context *ctx, int block, int unroll, int waves_per_cu);
/* Launch geometry of cbx_step_and_synchronise's kernel (3R + 2 reads and
 * 2R + 2 or 4R + 2 writes per element with momentum): block 64..256, unroll
 * 1 or 2, occupancy cap as above.  Default 64 / 1 / auto (2 waves per CU at
 * R = 8, measured: scripts/bench_step_and_synchronise.py --sweep); the
 * load/store policy is cbx_set_kernel_config's.                            */
int cbx_set_task_barrier_kernel_config (cbx_context *ctx, int block, int unroll, int waves_per_cu);
/* Bucketed pipeline for G > 1: kernel A / all-reduce / kernel B per bucket
 * of `bucket_elements` floats; 0 (default) = 8 buckets when G > 1, one at
 * G = 1; a value >= n = one bucket, all in order on the sync stream.  With
 * more than one bucket the all-reduce of bucket k runs on a second stream
 * beside kernel A of bucket k+1, and the kernels are timed as summed busy
 * spans (cbx_timing_history).                                             */
int cbx_set_bucket_elements (cbx_context *ctx, long long bucket_elements);
/* How the bucketed pipeline overlaps (G > 1, or forced split): 0 (default)
 * within a step only; 1 also across steps: kernels A run on their own
 * stream and A(k) waits only for B(k) of the previous step, so the next
 * step's first buckets run while this step's last all-reduces are on the
 * link.  Any other C-ABI call between two steps that may enqueue device
 * work makes the next step join the whole sync stream first.  Same results
 * bit for bit in both modes.                                              */
int cbx_set_pipeline_mode (cbx_context *ctx, int mode);
/* Mode 1: kernel A(k) waits for kernel B of the previous step once
 * per `stride` buckets, on B(k + stride - 1), which implies the earlier
 * ones.  1 (default) waits per bucket; larger strides pay fewer
 * cross-queue waits for less overlap between steps.  1..4096.            */
int cbx_set_cross_wait_stride (cbx_context *ctx, int stride);
/* Split path with buckets (every pipeline mode): all-reduce `group`
 * buckets behind one wait of the all-reduce stream on kernel A of the
 * group's last bucket, instead of one wait per bucket.  1 (default) is the
 * per-bucket order.  Larger groups pay fewer cross-queue waits (~10 us of
 * queue latency each) and start each group's all-reduces later.  Same
 * results bit for bit.  1..4096.  No reference counterpart: the bucket
 * pipeline itself is this library's (common.c:14-54 all-reduces one flat
 * buffer).                                                                */
int cbx_set_allreduce_group (cbx_context *ctx, int group);
/* How the SMA step's all-reduce crosses devices (G > 1):
 *   CBX_ALLREDUCE_RCCL (0, default): grouped ncclAllReduce, bucketed and
 *     pipelined as configured above (synch/common.c:3-57);
 *   CBX_ALLREDUCE_PEER (1): one process over every device (cbx_init with G
 *     devices), or one process per GPU once cbx_peer_import has mapped every
 *     rank's buffers (below).  No RCCL pass: after hipDeviceEnablePeerAccess
 *     (or the IPC mapping), device g sums shard g of every device's acc by
 *     direct peer reads, then
 *     kernel B on each device reads every shard of D from its owner
 *     (two-shot over all xGMI links at once; the reference's non-NCCL path
 *     copies peer buffers, common.c:64-95).  Bucketed and pipelined like
 *     the all-reduce (bucket size, modes, strides, groups above): the
 *     reduction of bucket k runs on the all-reduce stream beside kernel A of
 *     bucket k+1 and waits for kernel A(k) of EVERY device; kernel B(k) waits
 *     for every device's reduction of k.  Sums in device order: bit-exact
 *     against the rank-order oracle and identical on every device.  The
 *     host-staged step and S-SGD keep RCCL.
 *   CBX_ALLREDUCE_RSAG (2): every process form.  Per bucket, RCCL
 *     reduce-scatter of acc (the control block rides a grouped 64-float
 *     all-reduce), the base momentum on this rank's shard only
 *     (last = fma(0.9, last, D)), RCCL all-gather of last, then kernel B
 *     adds the gathered D' to z.  The all-reduce's link bytes; the momentum
 *     pass (12 B per element) runs on 1/G of the bucket; every rank ends
 *     with the same z and last (SURVEY 8(e) variant 1).  G must divide 1024
 *     (powers of two up to 16).  The host-staged step and S-SGD keep the
 *     all-reduce.
 * CBX_ERR_STATE for PEER on a one-process-per-GPU context before
 * cbx_peer_import.                                                         */
#define CBX_ALLREDUCE_RCCL 0
#define CBX_ALLREDUCE_PEER 1
#define CBX_ALLREDUCE_RSAG 2
int cbx_set_allreduce_algorithm (cbx_context *ctx, int algorithm);
/* The peer-read all-reduce with one process per GPU (cbx_init_rank, G > 1;
 * no reference counterpart: the reference runs one process over every GPU,
 * executioncontext.c:185-201, and its non-NCCL path copies peer buffers,
 * common.c:64-95).  After cbx_set_model_manager on every rank:
 *   1. cbx_peer_export(ctx, blob, &bytes) writes this rank's handles into
 *      `blob` (CBX_PEER_BLOB_BYTES): the IPC handles (hipIpcGetMemHandle)
 *      of its acc and D buffers, which move out of the model arena into
 *      allocations of their own (below 2 GiB - 2 MiB each: ROCm 7.0's IPC
 *      keeps an allocation's size in 32 bits, and an open of 2 GiB or more
 *      never returns; CBX_ERR_UNSUPPORTED above); rank 0
 *      also creates the page of completion flags (POSIX shared memory) and
 *      names it in its blob;
 *   2. the caller gathers every rank's blob, in rank order, over its own
 *      control plane (bench.py: gloo all_gather);
 *   3. cbx_peer_import(ctx, blobs, nranks) maps every other rank's acc and
 *      D (hipIpcOpenMemHandle; the ranks open in turn; a rank that has not
 *      opened its handles 120 s into the import fails everyone's import) and
 *      pins the flag page
 *      (hipHostRegister).  It succeeds on every rank or on none: a rank
 *      whose opens failed fails every rank's import.
 * Then CBX_ALLREDUCE_PEER is accepted.  The ranks' streams order each
 * other through the flags: a rank writes the step's sequence number after
 * its kernel A / reduction of a bucket (hipStreamWriteValue64), the others
 * wait for it (hipStreamWaitValue64 >=); the pipeline, its modes, strides,
 * groups and the sums' device order are the single-process form's.  Same
 * results bit for bit.  At most 4096 buckets.  cbx_free then waits (up to
 * 60 s in all, streams polled) until every rank is done with this rank's
 * memory; if a dead peer left this rank's streams waiting, it writes the
 * release into every rank's flags itself.  Every rank calls export, import
 * and free.
 * Failure (the reference's answer to any failure is exit(1), debug.h:37; the
 * invariant at stake is that every GPU applies the same D to the same z,
 * synch/sma.c:168-174):
 *   - A step that fails part-way on a rank (its call returns the error; that
 *     rank's z, last and replicas are undefined from it on, as for a
 *     poisoned step) sets that rank's broken word on the page, then releases
 *     its flags (from the host, and again behind its queued flag writes), so
 *     no other rank's stream waits forever.
 *   - A released flag lets a wait pass whether or not the data it guards was
 *     written, so a step another rank had already enqueued may read the
 *     failed rank's stale acc or D.  So after each step's last kernel B, on
 *     the same stream (every load of the step's kernels B has returned), one
 *     wave reads every rank's broken word and, if one is set, records the
 *     step's sequence number on the page.  cbx_wait on that rank then
 *     returns CBX_ERR_STATE naming the
 *     step: its z and last are undefined from that step on.  A step whose
 *     cbx_wait reports nothing read only data that was complete (any stale
 *     read needs a release, and the broken word comes before it).
 *   - From the moment any rank's broken word is visible to a rank, that
 *     rank refuses EVERY collective step (cbx_synchronise and
 *     cbx_synchronise_staged in every all-reduce form and update model, and
 *     cbx_average_batchnorm_stats) with CBX_ERR_STATE, releasing its own
 *     flags first, until cbx_resync_base.  The decision is each rank's own,
 *     made from the page when it is called.  A job that keeps the peer-read
 *     form across steps always recovers (every later step is refused or
 *     reported).  A job that switches to an RCCL collective while a failure
 *     is still on its way to some rank can leave that rank inside a
 *     collective the others refuse; every rank's cbx_resync_base then fails
 *     within its 60 s bounds and the job must end, as the reference's does.
 *     After a failure on any rank, every rank stops stepping and calls
 *     cbx_resync_base.
 * Same results bit for bit as before whenever no rank fails.              */
#define CBX_PEER_BLOB_BYTES 256
int cbx_peer_export (cbx_context *ctx, void *blob, size_t *bytes);
int cbx_peer_import (cbx_context *ctx, const void *blobs, int nranks);
/* Re-synchronise the base models after a failure (or at any time): every
 * rank calls it (a collective over the RCCL communicator).  Releases this
 * rank's flags if it knows of a failure, waits (up to 60 s, polled) until its
 * streams drain, broadcasts z and last (device buffers, padded length) from
 * rank `root`, and, once every rank has drained and received them, clears
 * this rank's flag words, broken and poison words and restarts the form's
 * step numbering; a second barrier keeps every rank from starting a step
 * before every rank's words are clear.  Afterwards z and last are identical
 * on every rank and every form is accepted again.  Replicas (w_i, s_i) are
 * left as they are (a Phase-D copy request resets them to z).  No-op at
 * G = 1.                                                                  */
int cbx_resync_base (cbx_context *ctx, int root);
/* How cbx_synchronise_staged moves the model between the pinned host mirror
 * and the device (north_star: the path starts and ends in host memory):
 *   CBX_STAGING_ZEROCOPY (0, default): the SMA kernels read their inputs
 *     from the host mirror over PCIe and write their outputs to it and to
 *     the device, both link directions at once, no copy engine;
 *   CBX_STAGING_DMA (1): copy-engine uploads and downloads per bucket on
 *     their own streams, overlapping the kernels (databuffer.c:95-122 is the
 *     reference's synchronous staging).
 * Both leave host and device exactly as cbx_stage_in + cbx_synchronise +
 * cbx_stage_out do.                                                        */
#define CBX_STAGING_ZEROCOPY 0
#define CBX_STAGING_DMA 1
int cbx_set_staging_mode (cbx_context *ctx, int mode);
/* One process over several local devices (cbx_init): who enqueues each
 * device's share of a barrier step (the SMA split and peer-read steps).
 *   0   one thread, every device in turn, collectives grouped across the
 *       devices (the reference's ResultCollector thread, common.c:14-54);
 *   1   one thread per local device, each issuing its own device's kernels
 *       and collectives (NCCL's thread-per-device use of ncclCommInitAll's
 *       communicators); the call returns once every device's work is
 *       enqueued, as before;
 *  -1   (default) 0: the reference's form, until measured otherwise on
 *       distinct devices (bench.py's warm-up tuner times 0 against 1).
 * Same work on the same streams in the same per-device order: results are
 * identical (a threaded peer-read step orders its cross-device waits behind
 * the other devices' event records).  At 8 devices and 8 buckets one thread
 * may spend longer enqueuing a step than the GPUs spend running it
 * (DESIGN.md section 6).                                                   */
int cbx_set_enqueue_threads (cbx_context *ctx, int mode);
/* Force the multi-GPU pipeline (kernel A + RCCL all-reduce + kernel B) even
 * at G = 1 (a one-rank communicator), so a single-GPU host exercises it.  */
int cbx_set_force_split (cbx_context *ctx, int force);
/* Synthetic inputs of BASELINE.md 2.3, generated on the device:
 * z ~ N(0,.05^2), s_i = z + N(0,.01^2), w_i = s_i + N(0,.001^2),
 * last ~ N(0,.001^2); seeds derive from `seed` ^ buffer id.               */
int cbx_fill_synthetic (cbx_context *ctx, unsigned long long seed);
/* Float4 device-to-device copy ceiling on local device 0: `bytes` per
 * buffer, `iters` timed launches; writes achieved GB/s (read + write).    */
int cbx_bench_copy (cbx_context *ctx, size_t bytes, int iters, float *gbps);

/* ---- the sma.c seam: buffers owned by the caller ------------------------
 * For a Crossbow build that keeps its own model manager, model buffers and
 * task side (modelmanager.c, model.c, executioncontext.c, the callback and
 * task handlers, all untouched) and replaces only two function bodies:
 *   crossbowSynchronisationSMA (synch/sma.c:233-248 -> :13-231)
 *       -> cbx_sma_plan_step
 *   crossbowKernelOptimiserSMA (kernels/optimisers/sma.cu:3-100)
 *       -> cbx_sma_optimise_buffers
 * (or, with tau = 1, both in one launch: cbx_sma_plan_step_and_optimise)
 * and, further down, the synchronous-SGD pair (cbx_ssgd_plan_step,
 * cbx_ssgd_accumulate_buffers), the elastic-averaging barrier
 * (cbx_ea_plan_step) and the Polyak-Ruppert barrier (cbx_pr_plan_step)
 * (INTEGRATION.md section 1b shows the bodies).  Buffers hold exactly
 * `elements` floats (no padding) and must be 16-byte aligned, as hipMalloc's
 * are.  Same kernels and arithmetic as the context path: bit-exact against
 * the oracle at one GPU and in rank order.  No context is involved.       */
typedef struct cbx_sma_plan cbx_sma_plan;
/* What the step needs beyond the caller's buffers, per device: the Phase-A
 * accumulator and the all-reduced difference (base->gradient, base->diff in
 * sma.c:66,82) with the control block that carries the Phase-D request
 * count, and the communicators: `comms` = the caller's ncclComm_t per device
 * (ctx->comms of executioncontext.c:185-201, as void*), or NULL to create
 * them with ncclCommInitAll over `devices` (ndevices > 1).  `devices` are
 * HIP device ids; `elements` = model->elements (model.h:35).             */
int cbx_sma_plan_create (cbx_sma_plan **plan, const int *devices, int ndevices, long long elements,
                         void *const *comms);
int cbx_sma_plan_free (cbx_sma_plan *plan);
/* G > 1: cut the step into `buckets` buckets and run the all-reduce of
 * bucket k on a stream of the plan's beside kernel A of bucket k+1 (as the
 * context's pipeline does; the caller's stream still orders the step
 * against its other work).  0 (default) = 8 buckets; 1 = the reference's
 * order, everything on the caller's stream.  Same results bit for bit.    */
int cbx_sma_plan_set_buckets (cbx_sma_plan *plan, int buckets);
/* Measurement aid for a one-rank plan (scripts/bench_averaging_seam.py):
 * with `on`, the fused launch of every step (cbx_sma_plan_step,
 * cbx_sma_plan_step_and_optimise, cbx_ea_plan_step, cbx_pr_plan_step) stamps
 * its own start and stop, as the
 * context's cbx_set_timing does, into a ring of the last 256 steps; no
 * marker packet is added to the caller's stream.  Switching it (on or off)
 * empties the ring.  cbx_sma_plan_timing_history waits for the last of them
 * and writes the kernel times (ms) of the last `count` timed steps, oldest
 * first; returns how many it wrote.  Steps with several ranks are not timed. */
int cbx_sma_plan_set_timing (cbx_sma_plan *plan, int on);
int cbx_sma_plan_timing_history (cbx_sma_plan *plan, float *ms, int count);
/* One SMA step (sma.c:13-231), enqueued on the caller's streams, async:
 *   streams[k]        dev->modelSynchronisationStream of devices[k] (hipStream_t)
 *   z[k], last[k]     baseModels[k]->data->dev / ->last->dev (last may be NULL
 *                     when momentum is 0, model.c:116-120)
 *   nreplicas         modelmanager->size; for replica id:
 *     replica_device[id]  position in `devices` of replicas[id]->dev
 *     w[id], s[id]        replicas[id]->data->dev, replicas[id]->diff->dev
 *     locked[id]          modelmanager->locked[id]
 *     copy[id]            replicas[id]->conf->_copy
 *   alpha             defaultModel->conf->alpha (sma.c:33)
 *   momentum          the base model's conf->momentum: > 0 applies the
 *                     hard-coded 0.9 (sma.c:150-152)
 *   first             replicas below it take no part (sma.c:69)
 * Locked replicas at or above `first` are averaged in id order per device.
 * Returns 1 when Phase D ran (a locked replica from `first` on had _copy:
 * every such replica now equals its device's base model; the caller resets
 * their _copy, sma.c:217-220), 0 when not.  The caller's events
 * (base->updated, synched[dev], replica->updated) are recorded on the same
 * streams after the call, as sma.c:115,177,204,222 do.  One step at a time
 * per plan (the reference's single ResultCollector thread): the scratch is
 * the plan's.  streams[k] must be the same stream on every call of a plan
 * (as dev->modelSynchronisationStream is): with buckets, the next step's
 * all-reduce of bucket k is ordered after this step's last kernel B only
 * through that stream, so a different stream would let it overwrite the
 * plan's D while B still reads it.  With a communicator that spans processes, each process
 * passes only its own replicas as locked; a Phase-D request on any rank
 * reaches every rank through the all-reduced control block, so the return
 * value reports this process's requests only.                           */
int cbx_sma_plan_step (cbx_sma_plan *plan, void *const *streams, float *const *z, float *const *last,
                       int nreplicas, const int *replica_device, float *const *w, const float *const *s,
                       const int *locked, const int *copy, float alpha, float momentum, int first);
/* The stepping replicas' task steps and the SMA step above in ONE launch over
 * the caller's buffers (one device, one rank): what cbx_step_and_synchronise
 * is to a context, for a tau = 1 build that replaces the pair
 * crossbowKernelOptimiserSMA + crossbowSynchronisationSMA.  It moves
 * (28R + 16) n bytes, or (20R + 16) n with the discard flag, where the two
 * calls move (40R + 16) n.  Arguments named as for cbx_sma_plan_step mean
 * the same; for replica id:
 *     g[id]               replicas[id]->gradient->dev
 *     rlast[id]           replicas[id]->last->dev (used iff replica_momentum > 0;
 *                         otherwise `rlast` itself may be NULL)
 *     step[id]            != 0: the replica holds a gradient that has not been
 *                         applied and takes its task step in this call; 0: it
 *                         joins the barrier with its s and w as they are
 *     learning_rate[id]   crossbowSolverConfGetLearningRate (conf, task) of a
 *                         stepping replica, positive, as cbx_sma_optimise_buffers
 *                         takes it; read only where step[id] != 0.  The caller
 *                         has made that query already, so the _copy flag it may
 *                         raise is in copy[]
 *   momentum          the base model's, as for cbx_sma_plan_step
 *   replica_momentum, weight_decay   the stepping replicas' conf values, one
 *                     pair for all of them
 *   flags             0 or CBX_STEP_DISCARD_TASK_OUTPUTS
 * The contract.  With flags == 0 every buffer (z, the base `last`, every w,
 * rlast, s and g) is left bit for bit as after
 *   cbx_sma_optimise_buffers (streams[0], w[id], g[id], rlast[id], s[id],
 *       elements, learning_rate[id], replica_momentum, weight_decay)
 *                                 for every id with step[id] != 0, in id order,
 *   cbx_sma_plan_step (plan, streams, z, last, nreplicas, replica_device, w, s,
 *       locked, copy, alpha, momentum, first).
 * With CBX_STEP_DISCARD_TASK_OUTPUTS, s[id] and g[id] of the stepping replicas
 * are not written at all (s[id] may then be NULL); the caller makes the promise
 * stated at cbx_step_and_synchronise.  Returns 1 when Phase D ran (every
 * participating w equals the new z; rlast, and s and g when kept, hold the
 * step's values all the same), 0 when not.
 * One launch on streams[0], asynchronous.  The plan adds no waits of its own:
 * the caller orders streams[0] behind whatever produced each stepping
 * replica's g (an event wait, as sma.c:63 waits on its events).  With
 * cbx_sma_plan_set_timing on, the launch stamps itself into the plan's ring.
 * Everything is checked before the launch: a refused call writes nothing, and
 * cbx_last_error names the cause.  CBX_ERR_INVALID: a NULL plan, streams, z, or
 * (nreplicas > 0) replica_device, w, s, g, locked, copy, step or
 * learning_rate; `last` NULL with momentum > 0, `rlast` NULL with
 * replica_momentum > 0 and a stepping replica; an unknown flag bit; `first`
 * out of range; a stepping replica that is not locked or is below `first`; a
 * participating replica on a device other than 0, with a NULL w[id], with a
 * NULL s[id] (unless it steps under the discard flag) or a buffer that is not
 * 16-byte aligned; a stepping replica with a NULL g[id], or with a NULL
 * rlast[id] when replica_momentum > 0.  CBX_ERR_UNSUPPORTED: a plan with more
 * than one device or a communicator of more than one rank (kernel A is not
 * fused); more than 64 participating replicas.  Nesterov momentum stays the
 * caller's err() (sma.cu:46-48): the call has no method argument.         */
int cbx_sma_plan_step_and_optimise (cbx_sma_plan *plan, void *const *streams,
                                    float *const *z, float *const *last,
                                    int nreplicas, const int *replica_device,
                                    float *const *w, float *const *s, float *const *g, float *const *rlast,
                                    const int *locked, const int *copy, const int *step,
                                    const float *learning_rate,
                                    float alpha, float momentum, float replica_momentum, float weight_decay,
                                    int first, unsigned flags);
/* cbx_sma_plan_step_and_optimise with a learning rate per variable: stepping
 * replica id steps variable v with r = (-learning_rate[id]) * multipliers[v],
 * one fp32 multiply, over the table that cbx_sma_plan_set_variables installed
 * (CBX_ERR_STATE without one).  Parameters, checks and refusals are those of
 * cbx_sma_plan_step_and_optimise.  With flags == 0 every buffer is left bit
 * for bit as after
 *   cbx_sma_plan_optimise_variables (plan, 0, streams[0], w[id], g[id], rlast[id],
 *       s[id], learning_rate[id], replica_momentum, weight_decay, 0, all variables)
 *                                 for every id with step[id] != 0, in id order,
 *   cbx_sma_plan_step (plan, streams, z, last, nreplicas, replica_device, w, s,
 *       locked, copy, alpha, momentum, first);
 * with CBX_STEP_DISCARD_TASK_OUTPUTS, s[id] and g[id] of the stepping replicas
 * are not written.  Nothing at or past `elements` is read or written.       */
int cbx_sma_plan_step_and_optimise_variables (cbx_sma_plan *plan, void *const *streams,
                                              float *const *z, float *const *last,
                                              int nreplicas, const int *replica_device,
                                              float *const *w, float *const *s, float *const *g,
                                              float *const *rlast,
                                              const int *locked, const int *copy, const int *step,
                                              const float *learning_rate,
                                              float alpha, float momentum, float replica_momentum,
                                              float weight_decay, int first, unsigned flags);
/* cbx_sma_plan_step_and_optimise with the clipped step of
 * cbx_sma_plan_optimise_clipped: stepping replica id takes the record of
 * slot[id] (the plan's device 0), whose norm pass and reduce the call launches
 * on streams[0] in front of the fused launch, in id order; the slot's scratch
 * is allocated on first use.  The arithmetic is cbx_step_and_synchronise_clipped's:
 * g = scale * g before weight decay, a kept g[id] always written, and a replica
 * whose record carries the skip bit keeps w (as the step sees it), g and rlast
 * bit for bit, takes s = w and joins the barrier so.  max_norm == 0 and
 * skip_nonfinite == 0 still run the reduction and count the step.  With
 * flags == 0 every buffer and every slot's record is left bit for bit as after
 *   cbx_sma_plan_optimise_clipped (plan, 0, slot[id], streams[0], w[id], g[id],
 *       rlast[id], s[id], learning_rate[id], replica_momentum, weight_decay,
 *       max_norm, skip_nonfinite, 0)     for every id with step[id] != 0, in id order,
 *   cbx_sma_plan_step (plan, streams, z, last, nreplicas, replica_device, w, s,
 *       locked, copy, alpha, momentum, first);
 * with CBX_STEP_DISCARD_TASK_OUTPUTS, s[id] and g[id] of the stepping replicas
 * are not written.  Checks and refusals are cbx_sma_plan_step_and_optimise's,
 * all before the first launch (a refused call bumps no counter), and
 * CBX_ERR_INVALID besides: max_norm negative, NaN or infinite; skip_nonfinite
 * neither 0 nor 1; a NULL `slot` with a stepping replica; a stepping replica's
 * slot outside [0, 64); two stepping replicas sharing a slot.  slot[id] of a
 * replica that does not step is not read.  The plan queues no wait of its own. */
int cbx_sma_plan_step_and_optimise_clipped (cbx_sma_plan *plan, void *const *streams,
                                            float *const *z, float *const *last,
                                            int nreplicas, const int *replica_device,
                                            float *const *w, float *const *s, float *const *g,
                                            float *const *rlast,
                                            const int *locked, const int *copy, const int *step,
                                            const float *learning_rate,
                                            const int *slot, float max_norm, int skip_nonfinite,
                                            float alpha, float momentum, float replica_momentum,
                                            float weight_decay, int first, unsigned flags);
/* cbx_sma_plan_step_and_optimise_clipped with a learning rate per variable:
 * stepping replica id clips through the record of slot[id] and steps variable v
 * with r = (-learning_rate[id]) * multipliers[v] over the table that
 * cbx_sma_plan_set_variables installed (CBX_ERR_STATE without one, before any
 * other check but the NULL plan).  Parameters, checks and refusals are
 * cbx_sma_plan_step_and_optimise_clipped's, the arithmetic
 * cbx_step_and_synchronise_clipped_variables'.  With flags == 0 every buffer
 * and every slot's record is left bit for bit as after
 *   cbx_sma_plan_optimise_clipped (plan, 0, slot[id], streams[0], w[id], g[id],
 *       rlast[id], s[id], learning_rate[id], replica_momentum, weight_decay,
 *       max_norm, skip_nonfinite, 1)     for every id with step[id] != 0, in id order,
 *   cbx_sma_plan_step (plan, streams, z, last, nreplicas, replica_device, w, s,
 *       locked, copy, alpha, momentum, first);
 * with CBX_STEP_DISCARD_TASK_OUTPUTS, s[id] and g[id] of the stepping replicas
 * are not written.  When no replica steps the call is
 * cbx_sma_plan_step_and_optimise_variables'.  Nothing at or past `elements` is
 * read or written.                                                          */
int cbx_sma_plan_step_and_optimise_clipped_variables (cbx_sma_plan *plan, void *const *streams,
                                                      float *const *z, float *const *last,
                                                      int nreplicas, const int *replica_device,
                                                      float *const *w, float *const *s, float *const *g,
                                                      float *const *rlast,
                                                      const int *locked, const int *copy, const int *step,
                                                      const float *learning_rate,
                                                      const int *slot, float max_norm, int skip_nonfinite,
                                                      float alpha, float momentum, float replica_momentum,
                                                      float weight_decay, int first, unsigned flags);
/* The statistics reduction of cbx_model_stats over caller-owned buffers of
 * exactly the plan's `elements` floats on the plan's device k (where a
 * Crossbow build would checksum, databuffer.c:141-162): `ref` against
 * bufs[0..nbufs) (0..64 buffers).  var_elements[0..nvars) are the variables'
 * float counts in offset order and must sum to `elements`; nvars = 0 means
 * one variable.  ref_out: 1 record; out: nbufs; ref_vars: nvars (or 1);
 * vars: [i * nvars + v]; the last two may be NULL.  The scratch is the
 * plan's (one call at a time per plan device).  Enqueues on `stream`
 * (hipStream_t of that device) and blocks on it before returning.          */
int cbx_sma_plan_buffer_stats (cbx_sma_plan *plan, int k, void *stream, const float *ref,
                               const float *const *bufs, int nbufs, const long long *var_elements, int nvars,
                               cbx_buffer_stats *ref_out, cbx_buffer_stats *out, cbx_buffer_stats *ref_vars,
                               cbx_buffer_stats *vars);
/* The replica's optimiser step of one task (sma.cu:3-100) in one pass over
 * its buffers, on `stream` (hipStream_t, the task stream; the current HIP
 * device must be the buffers'): w = model->data, g = model->gradient
 * (updated in place, as the reference leaves it), last = model->last (used
 * iff momentum > 0), s = model->diff (the snapshot of w before the update);
 * learning_rate = crossbowSolverConfGetLearningRate (conf, task)
 * (solverconfiguration.c:116-162); momentum, weight_decay from the conf.
 * Nesterov momentum stays the caller's err() (sma.cu:46-48).             */
int cbx_sma_optimise_buffers (void *stream, float *w, float *g, float *last, float *s, long long elements,
                              float learning_rate, float momentum, float weight_decay);
/* The same step with a learning rate per variable
 * (crossbowModelGetLearningRateForVariable, model.c:159-177), whole or on a
 * range of variables (crossbowStreamSynchronousEamsgdModelUpdate,
 * stream.c:422-479).  cbx_sma_plan_set_variables attaches the lookup tables
 * to the plan: var_elements[0..nvars) are the variables' float counts in
 * offset order and must sum to the plan's `elements`; multipliers[0..nvars)
 * are v->learningRateMultiplier (NULL: all 1).  It blocks (every plan device
 * is drained, then the tables are uploaded to it); calling it again replaces
 * the tables.  cbx_sma_plan_optimise_variables steps variables
 * [first_var, first_var + nvars) of caller-owned, unpadded, 16-byte-aligned
 * buffers of `elements` floats on plan device k, asynchronously on `stream`,
 * with r_v = -learning_rate * multiplier_v (it always multiplies: a caller
 * without irregular rates keeps calling cbx_sma_optimise_buffers).  Floats
 * outside the range are not written.  g and last keep sma.cu's sign, as in
 * cbx_replica_optimise_variables.  nvars == 0 is CBX_OK without a launch.  */
int cbx_sma_plan_set_variables (cbx_sma_plan *plan, const long long *var_elements, const float *multipliers,
                                int nvars);
int cbx_sma_plan_optimise_variables (cbx_sma_plan *plan, int k, void *stream, float *w, float *g, float *last,
                                     float *s, float learning_rate, float momentum, float weight_decay,
                                     int first_var, int nvars);
/* The step with gradient clipping by global norm and the non-finite skip
 * (cbx_set_gradient_clip: the same semantics, kernels and bits of S on the
 * same data), over caller-owned, unpadded, 16-byte-aligned buffers of the
 * plan's `elements` floats on plan device k, asynchronously on `stream`:
 * norm pass, reduce and step.  `slot` in [0, 64) names plan-owned scratch
 * (record and slab, allocated on the slot's first use), so 64 replicas can be
 * in flight; steps that share a slot are ordered by the caller.
 * use_variables == 1 (needs cbx_sma_plan_set_variables): the per-variable
 * step over every variable; 0: cbx_sma_optimise_buffers' step.  max_norm and
 * skip_nonfinite as in cbx_set_gradient_clip, both 0 included (the reduction
 * still runs and the record counts the step).  cbx_sma_plan_clip_stats
 * blocks on `stream`, then copies the slot's record back: all zeros before
 * the slot's first step.                                                   */
int cbx_sma_plan_optimise_clipped (cbx_sma_plan *plan, int k, int slot, void *stream, float *w, float *g,
                                   float *last, float *s, float learning_rate, float momentum, float weight_decay,
                                   float max_norm, int skip_nonfinite, int use_variables);
int cbx_sma_plan_clip_stats (cbx_sma_plan *plan, int k, int slot, void *stream, cbx_clip_stats *out);
/* The reduction alone (norm pass and reduce, no step) over g on plan device k,
 * blocking on `stream`: a caller's look at its gradient's norm, and the
 * measurement of the two launches.  The slot's record is updated as a step's
 * reduction updates it (it counts a step).  loads: 0 plain, 1 nontemporal
 * loads of g, -1 the library's choice.  pass_ms / reduce_ms (either may be
 * NULL): device milliseconds of the two dispatches, from their own
 * timestamps.                                                              */
int cbx_sma_plan_gradient_norm (cbx_sma_plan *plan, int k, int slot, void *stream, const float *g, float max_norm,
                                int skip_nonfinite, int loads, float *pass_ms, float *reduce_ms);
/* The same seam for update model WORKER (synchronous SGD):
 * crossbowSynchronisationSynchronousSGD (synch/synchronoussgd.c:13-106) ->
 * cbx_ssgd_plan_step, over acc[k] = baseModels[k]->gradient->dev (the
 * accumulated lr-scaled task gradients; reset to 0 by the step), z, last
 * (used iff momentum > 0: the base model's conf->momentum, NOT forced to
 * 0.9), the locked replicas from `first` on (set to their device's new base
 * model, common.c:198-220) and wpc = defaultBaseModel->wpc (D *= 1/wpc).
 * Buckets as cbx_sma_plan_set_buckets sets them at G > 1; one rank always
 * runs one apply pass (no all-reduce to overlap), whatever the setting.
 * streams[k] must be the same stream on every call, as for cbx_sma_plan_step.
 * crossbowKernelOptimiserSynchronousSGD (kernels/optimisers/synchronoussgd.cu:
 * 3-56) -> cbx_ssgd_accumulate_buffers: g += weight_decay * w, then
 * acc += -learning_rate * g, on `stream` = the device's model-synchronisation
 * stream once it has waited for the task's gradient (:37-40).            */
/* crossbowCudnnBatchNormParamsSynchroniseEstimatedMeanAndVariable
 * (cudnn/cudnnbatchnormparams.c:157-222) over the caller's statistics
 * buffers: arguments as cbx_average_batchnorm_stats, with k the position in
 * the plan's devices (the default device is rank 0 of the communicator).
 * No-op with one rank.  Device-synchronises before and after.             */
int cbx_sma_plan_average_batchnorm (cbx_sma_plan *plan, int layers, const int *elements, float *const *mean,
                                    float *const *variance, const int *updated);
int cbx_ssgd_plan_step (cbx_sma_plan *plan, void *const *streams, float *const *z, float *const *last,
                        float *const *acc, int nreplicas, const int *replica_device, float *const *w,
                        const int *locked, float momentum, int wpc, int first);
int cbx_ssgd_accumulate_buffers (void *stream, const float *w, float *g, float *acc, long long elements,
                                 float learning_rate, float weight_decay);
/* The stepping replicas' task steps (kernels/optimisers/synchronoussgd.cu:3-56)
 * and the one-device synchronous-SGD barrier (synch/synchronoussgd.c:13-106,
 * common.c:198-220) in one launch over the caller's buffers of exactly
 * `elements` floats: what cbx_step_and_synchronise_ssgd is to a context, for a
 * tau = 1 S-SGD build.  With R replicas and base momentum it moves
 * (8R + 24) n bytes where the calls move (16R + 24) n; with weight decay
 * (16R + 24) n, or (12R + 24) n with the discard flag, against (24R + 24) n.
 * It is cbx_ssgd_plan_step plus g, step, learning_rate, weight_decay and flags:
 * arguments named as there, or as for cbx_sma_plan_step_and_optimise, mean the
 * same.  g[id] may be NULL for a replica that only joins (step[id] == 0: it is
 * one written buffer); `g` and `learning_rate` themselves may be NULL when
 * nobody steps; `last` may be NULL, and is not used, when momentum == 0.  The
 * arithmetic is cbx_step_and_synchronise_ssgd's, the stepping replicas in
 * ascending id order, the accumulator starting from what acc[0] holds.
 * The contract.  With flags == 0 every buffer (z, last, acc, every w and g) is
 * left bit for bit as after
 *   cbx_ssgd_accumulate_buffers (streams[0], w[id], g[id], acc[0], elements,
 *       learning_rate[id], weight_decay)
 *                                 for every id with step[id] != 0, in id order,
 *   cbx_ssgd_plan_step (plan, streams, z, last, acc, nreplicas, replica_device,
 *       w, locked, momentum, wpc, first)   on a one-device, one-rank plan.
 * With CBX_STEP_DISCARD_TASK_OUTPUTS, g[id] of the stepping replicas is not
 * written (a difference only when weight_decay > 0).  Nothing at or past
 * `elements` is read or written: the last elements ride the same launch on
 * extra workgroups in front.  One launch on streams[0], asynchronous; the caller
 * orders streams[0] behind the gradients.  With cbx_sma_plan_set_timing on, the
 * launch stamps itself into the plan's ring.
 * Everything is checked before the launch, as in cbx_ea_plan_step_and_optimise:
 * CBX_ERR_INVALID for a missing argument, an unknown flag bit, wpc <= 0, `first`
 * out of range, a stepping replica that is not locked or below `first`, a
 * participating replica on a device other than 0 or with a missing or
 * misaligned buffer; CBX_ERR_UNSUPPORTED for a plan with more than one device
 * or rank, and for more than 64 participating replicas.  Returns CBX_OK or an
 * error.                                                                   */
int cbx_ssgd_plan_step_and_optimise (cbx_sma_plan *plan, void *const *streams, float *const *z, float *const *last,
                                     float *const *acc, int nreplicas, const int *replica_device,
                                     float *const *w, float *const *g, const int *locked, const int *step,
                                     const float *learning_rate, float momentum, float weight_decay,
                                     int wpc, int first, unsigned flags);
/* The same seam for the two averaging barriers, over an existing plan: they
 * share its acc / D scratch, communicators, comm stream, per-bucket events
 * and cbx_sma_plan_set_buckets with the SMA and S-SGD steps, so any sequence
 * of these steps on one plan is safe, one step at a time, streams[k] the
 * same stream on every call (as for cbx_sma_plan_step).  Arguments named as
 * for cbx_sma_plan_step mean the same.  Locked replicas at or above `first`
 * go in id order per device; more than 64 of them on one device is
 * CBX_ERR_UNSUPPORTED.  One rank: one fused launch on the caller's stream.
 * Several: kernel A, ncclAllReduce of acc into D, kernel B, bucketed as the
 * S-SGD step (AR(k) on the plan's stream beside A(k+1), B(k) after it; 1
 * bucket = everything in order on the caller's stream).  No control block
 * travels with these steps.  Same kernels and arithmetic as the context's
 * update models 3 (with cbx_set_elastic_average) and 6: the buffers' last
 * elements, past the last whole float4 chunk, run one float per lane on
 * extra workgroups of the same launches with the same fma sequence.
 *
 * crossbowSynchronisationSynchronousElasticAveragingSGD
 * (synch/synchronouseamsgd.c:307 -> :5-101 on one device, :106-305 on
 * several) -> cbx_ea_plan_step.  The difference d = x - z is taken from
 * w[id] when the plan's communicator has one rank (:55) and from the
 * snapshot s[id] = replicas[id]->diff->dev when it has several (:184); `s`
 * may be NULL with one rank.  No momentum; the copy flags are not read.
 * The task step kernels/optimisers/synchronouseamsgd.cu is, per element,
 * what cbx_sma_optimise_buffers already runs (weight decay, scale, momentum,
 * last, the snapshot into diff, apply): use it unchanged.
 * Returns CBX_OK or an error.                                              */
int cbx_ea_plan_step (cbx_sma_plan *plan, void *const *streams, float *const *z, int nreplicas,
                      const int *replica_device, float *const *w, const float *const *s, const int *locked,
                      float alpha, int first);
/* The stepping replicas' task steps (kernels/optimisers/synchronouseamsgd.cu)
 * and the one-device elastic-averaging barrier (synch/synchronouseamsgd.c:42-90)
 * in one launch over the caller's buffers of exactly `elements` floats: what
 * cbx_step_and_synchronise_elastic is to a context, for a tau = 1 EA-SGD build.
 * It moves (28R + 8) n bytes, or (20R + 8) n with the discard flag, where the
 * two calls move (36R + 8) n.  Arguments named as for
 * cbx_sma_plan_step_and_optimise mean the same; there is no `last`, no `copy`
 * and no base momentum, as the barrier has none.  s[id] may be NULL for a
 * replica that only joins (the barrier reads no snapshot on one device) and for
 * one that steps under CBX_STEP_DISCARD_TASK_OUTPUTS; `s` itself may be NULL
 * when every s[id] may.
 * The contract.  With flags == 0 every buffer (z, every w, rlast, s and g) is
 * left bit for bit as after
 *   cbx_sma_optimise_buffers (streams[0], w[id], g[id], rlast[id], s[id],
 *       elements, learning_rate[id], replica_momentum, weight_decay)
 *                                 for every id with step[id] != 0, in id order,
 *   cbx_ea_plan_step (plan, streams, z, nreplicas, replica_device, w, NULL,
 *       locked, alpha, first)     on a one-device, one-rank plan.
 * With the discard flag, s[id] and g[id] of the stepping replicas are not
 * written.  Nothing at or past `elements` is read or written: the last elements
 * ride the same launch on extra workgroups in front.  One launch on streams[0],
 * asynchronous; the caller orders streams[0] behind the gradients.  With
 * cbx_sma_plan_set_timing on, the launch stamps itself into the plan's ring.
 * Everything is checked before the launch, as in cbx_sma_plan_step_and_optimise:
 * CBX_ERR_INVALID for a missing argument, an unknown flag bit, `first` out of
 * range, a stepping replica that is not locked or below `first`, a participating
 * replica on a device other than 0 or with a missing or misaligned buffer;
 * CBX_ERR_UNSUPPORTED for a plan with more than one device or rank, and for
 * more than 64 participating replicas.  Returns CBX_OK or an error.        */
int cbx_ea_plan_step_and_optimise (cbx_sma_plan *plan, void *const *streams, float *const *z,
                                   int nreplicas, const int *replica_device,
                                   float *const *w, float *const *s, float *const *g, float *const *rlast,
                                   const int *locked, const int *step, const float *learning_rate,
                                   float alpha, float replica_momentum, float weight_decay,
                                   int first, unsigned flags);
/* cbx_ea_plan_step_and_optimise with the stepping replicas' gradients clipped
 * by global norm, a learning rate per variable, or both: what
 * cbx_sma_plan_step_and_optimise_clipped_variables is to the SMA barrier, and
 * cbx_step_and_synchronise_elastic_clipped_variables to a context.  The
 * arguments of cbx_ea_plan_step_and_optimise mean the same.
 * Clipping is on iff slot != NULL.  slot[id], max_norm and skip_nonfinite are
 * cbx_sma_plan_step_and_optimise_clipped's: every stepping replica names a slot
 * of its own in [0, 64), whose scratch is allocated on first use; its norm
 * pass and reduce run on streams[0] in id order in front of the launch, and
 * its record is read back with cbx_sma_plan_clip_stats.  max_norm == 0 with
 * skip_nonfinite == 0 still reduces and counts.  When nobody steps there is no
 * norm pass and no record is touched.
 * use_variables is 0 or 1; with 1 the step of variable v uses
 * learning_rate[id] * mult[v] of the table of cbx_sma_plan_set_variables.
 * With slot == NULL and use_variables == 0 the call is
 * cbx_ea_plan_step_and_optimise: the same kernel, the same bits.
 * The contract.  With flags == 0 every buffer (z, every w, rlast, s and g) and
 * every slot's record is left bit for bit as after, for every id with
 * step[id] != 0 in id order,
 *   clipping on:  cbx_sma_plan_optimise_clipped (plan, 0, slot[id], streams[0], w[id], g[id],
 *                     rlast[id], s[id], learning_rate[id], replica_momentum, weight_decay,
 *                     max_norm, skip_nonfinite, use_variables)
 *   rates only:   cbx_sma_plan_optimise_variables (plan, 0, streams[0], w[id], g[id], rlast[id],
 *                     s[id], learning_rate[id], replica_momentum, weight_decay, 0, nvars)
 *   neither:      cbx_sma_optimise_buffers (...) as above
 * and then cbx_ea_plan_step (plan, streams, z, nreplicas, replica_device, w,
 * NULL, locked, alpha, first).  With the discard flag, s[id] and g[id] of the
 * stepping replicas are not written.  Nothing at or past `elements` is read or
 * written.  One-device, one-rank plans only.
 * Everything is checked before the first launch.  CBX_ERR_INVALID: as
 * cbx_ea_plan_step_and_optimise, and a max_norm that is negative, NaN or
 * infinite, a skip_nonfinite or use_variables that is neither 0 nor 1, a
 * stepping replica's slot out of range or named twice.  CBX_ERR_STATE:
 * use_variables without a table.  CBX_ERR_UNSUPPORTED: a plan with more than
 * one device or rank; more than 64 participating replicas.
 * Returns CBX_OK or an error.                                              */
int cbx_ea_plan_step_and_optimise_clipped_variables (cbx_sma_plan *plan, void *const *streams, float *const *z,
                                   int nreplicas, const int *replica_device,
                                   float *const *w, float *const *s, float *const *g, float *const *rlast,
                                   const int *locked, const int *step, const float *learning_rate,
                                   const int *slot, float max_norm, int skip_nonfinite, int use_variables,
                                   float alpha, float replica_momentum, float weight_decay,
                                   int first, unsigned flags);
/* crossbowSynchronisationPolyakRuppert (synch/polyakruppert.c:319 -> :5-138
 * on one device, :140-317 on several) -> cbx_pr_plan_step.  The average is
 * over p = nreplicas = modelmanager->size (:15): every replica of every
 * rank, locked or not (a process passes the other ranks' replicas as
 * unlocked).  last[k] = baseModels[k]->last->dev may be NULL (and `last`
 * itself, model.c:116-120); where given it is left holding L = D - z
 * (:98-104).  clock = the step's clock (:16), >= 0 or CBX_ERR_INVALID.
 * With alpha == 0 the replicas are read and not written (:72).  A locked
 * replica from `first` on whose copy[id] is raised becomes its device's new
 * z (:122-137) and is not written before that; a request stays local to
 * its device.  Returns the number of this process's such replicas (>= 0):
 * the caller resets their _copy (:131).  Errors are negative.  The
 * reference's task step optimisers/polyakruppert.cu is a stub.             */
int cbx_pr_plan_step (cbx_sma_plan *plan, void *const *streams, float *const *z, float *const *last,
                      int nreplicas, const int *replica_device, float *const *w, const int *locked,
                      const int *copy, float alpha, int clock, int first);

#ifdef __cplusplus
}
#endif

#endif /* CROSSBOW_SMA_H_ */
