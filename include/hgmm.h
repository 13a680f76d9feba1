/*
 * hgmm.h -- C ABI of the MI355X-native (gfx950) GMM / hierarchical-GMM EM engine.
 *
 * This is the drop-in boundary for the EM hot path of
 * somanshu25/GPU-Accelerated-Point-Cloud-Registration-Using-Hierarchical-GMM.
 * The reference has no FFI seam of its own: its seam is Python duck typing
 * (`cupy.get_array_module(X)` in src/python/gmm_waymo/src/gmm_impl.py:19,31,54,68 and the
 * single host->device hop in src/python/gmm_waymo/src/gmm.py:72-80).  Each entry point
 * below names the reference function(s) it replaces (paths relative to the upstream
 * repository root).  INTEGRATION.md shows the ctypes binding a maintainer adds.
 *
 * Conventions
 *   - plain C types only; every function returns 0 on success or a negative hgmm_status.
 *     hgmm_last_error(ctx) returns a human-readable description of the last failure.
 *   - "host" pointers are borrowed for the duration of the call; "dev" pointers are device
 *     addresses obtained from hgmm_alloc() (or any hipMalloc'd buffer on ctx's device).
 *   - one context per device / per rank, no global state; a context is not re-entrant,
 *     distinct contexts may be driven from distinct threads.
 *   - all kernels run on the context's own HIP stream; calls that return host data
 *     synchronise that stream, all others are asynchronous.
 *   - cov_type: 0 = diag ([J,3] per-axis), 1 = spherical ([J]);
 *     variant : 0 = "W" (gmm_waymo/src/gmm_impl.py), 1 = "G" (gmmreg_gpu/gmm_impl.py)
 *     -- the two flavours differ in eps / regularisation, see SURVEY.md 8(a).
 *   - `inv_std` is what the reference calls `inv_cov` (it is 1/sigma, not 1/sigma^2).
 */
#ifndef HGMM_H
#define HGMM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct hgmm_ctx hgmm_ctx;

enum hgmm_status {
    HGMM_OK = 0,
    HGMM_ERR_HIP = -1,        /* a HIP runtime call failed */
    HGMM_ERR_ARG = -2,        /* invalid argument / unsupported size */
    HGMM_ERR_STATE = -3,      /* call sequence error (e.g. no points set) */
    HGMM_ERR_RCCL = -4,       /* an RCCL call failed */
    HGMM_ERR_NODEVICE = -5    /* no usable gfx950 device */
};

enum { HGMM_COV_DIAG = 0, HGMM_COV_SPHERICAL = 1 };
enum { HGMM_VARIANT_W = 0, HGMM_VARIANT_G = 1 };

/* kernels that the in-library profiler times with hipEvents (hgmm_profile_*) */
enum hgmm_kernel_id {
    HGMM_K_FLAT_ESTEP = 0,    /* materialising E-step (writes log_resp[N,J]) */
    HGMM_K_FLAT_FUSED = 1,    /* fused E+M sufficient-statistics kernel      */
    HGMM_K_FLAT_MSTEP = 2,    /* M-step moments from materialised resp       */
    HGMM_K_TREE_ESTEP = 3,    /* HGMM level E-step (8 children / point)      */
    HGMM_K_TREE_LOGLIK = 4,   /* HGMM level log-likelihood (all level nodes) */
    HGMM_K_TREE_REG = 5,      /* HGMM registration E-step (tree descent)     */
    HGMM_K_UTIL_FILL = 6,     /* hgmm_util_fill_f32 (HBM write-ceiling probe) */
    HGMM_K_FULL_PASS = 7,     /* full-cov flat EM: denominators + arg-max + log-likelihood */
    HGMM_K_FULL_MOMENTS = 8,  /* full-cov flat EM: fp64-MFMA sufficient statistics */
    HGMM_K_KMEANS_ASSIGN = 9, /* KMeans initialiser: nearest-centre assignment */
    HGMM_K_KMEANS_ACCUM = 10, /* KMeans initialiser: per-cluster sums */
    HGMM_K_ALLREDUCE = 11,    /* the sufficient-statistics all-reduce (RCCL / host backend), N > 1 only */
    HGMM_K_FULL_FUSED = 12,   /* full-cov flat EM, one pass: denominators + arg-max + q + fp64-MFMA statistics */
    HGMM_K_TREE_SCORE = 13,   /* HGMM score of a moved target (tree descent, per-point outputs + summary) */
    HGMM_K_FLAT_BOUNDARY = 14, /* flat EM between two iterations: reduction + M-step + next table + stop rule */
    HGMM_K_VOXEL = 15,        /* voxel-grid down-sample: the whole launch set (box, keys, sort, heads, centroids) */
    HGMM_K_COUNT = 16
};

/* ---- lifecycle ------------------------------------------------------------------ */
int hgmm_version(void);
int hgmm_device_count(int* count);
int hgmm_create(int device_id, hgmm_ctx** out);
int hgmm_destroy(hgmm_ctx* ctx);
const char* hgmm_last_error(const hgmm_ctx* ctx);  /* ctx may be NULL: last create() error */
int hgmm_device_info(hgmm_ctx* ctx, char* name, int name_len, int* compute_units,
                     int64_t* hbm_bytes);
int hgmm_synchronize(hgmm_ctx* ctx);

/* ---- device memory (what cupy.asarray / cupy.asnumpy did: gmm.py:73-80, 95) ------ */
int hgmm_alloc(hgmm_ctx* ctx, size_t bytes, void** dev_out);
int hgmm_free(hgmm_ctx* ctx, void* dev);
int hgmm_h2d(hgmm_ctx* ctx, void* dev_dst, const void* host_src, size_t bytes);
int hgmm_d2h(hgmm_ctx* ctx, void* host_dst, const void* dev_src, size_t bytes);
/* device -> device on the context's stream, nothing waits (cupy.ndarray.copy() / astype(copy=True)) */
int hgmm_d2d(hgmm_ctx* ctx, void* dev_dst, const void* dev_src, size_t bytes);
/* Host-visible scalars: `count` doubles (<= 4096) of pinned host memory owned by the context that kernels write
 * directly (dev_out is the address they use, host_out the one the host reads).  With an event recorded behind the
 * producing kernel a value is read without draining the stream: what a 0-d CuPy array is to the reference's loops
 * (`lower_bound = log_prob_norm`, gmm_impl.py:136, read by `abs(change) < tol` while the M-step is still running).
 * The same array is returned on every call (count only grows it before its first use). */
int hgmm_host_scalars(hgmm_ctx* ctx, int count, double** host_out, double** dev_out);
/* 64 event slots on the context's stream: record marks the work enqueued so far, wait blocks the host until that
 * work (and only that) is done. */
#define HGMM_EVENT_SLOTS 64
int hgmm_event_record(hgmm_ctx* ctx, int slot);
int hgmm_event_wait(hgmm_ctx* ctx, int slot);
/* Elementwise float32 arithmetic on device arrays, enqueued on the context's stream (IEEE: bitwise NumPy's results
 * for + - * / sqrt): out[i] = a[i] op (dev_b ? dev_b[i] : scalar); RSUB / RDIV take the operands the other way round;
 * SQRT / EXP / LOG ignore the second operand.  out may alias a or b.  This is the `inv_cov = 1 / (xp.sqrt(covariances
 * + 1e-6) + eps)` of a caller's own EM loop (gmm_impl.py:134) without a trip to the host. */
enum hgmm_elementwise_op {
    HGMM_EW_ADD = 0, HGMM_EW_SUB = 1, HGMM_EW_RSUB = 2, HGMM_EW_MUL = 3, HGMM_EW_DIV = 4, HGMM_EW_RDIV = 5,
    HGMM_EW_SQRT = 6, HGMM_EW_EXP = 7, HGMM_EW_LOG = 8, HGMM_EW_MAX = 9, HGMM_EW_MIN = 10
};
int hgmm_elementwise_f32(hgmm_ctx* ctx, int op, int64_t n, const float* dev_a, const float* dev_b, float scalar,
                         float* dev_out);

/* ---- point cloud ------------------------------------------------------------------
 * Replaces `dev_X = cupy.asarray(X.astype(np.float32))` (gmm_waymo/src/gmm.py:73) and
 * `cuda.to_device(points)` (hgmm/hgmm_gpu.py:513).  xyz is host row-major [n,3]. */
int hgmm_set_points_f32(hgmm_ctx* ctx, const float* xyz, int64_t n);
int hgmm_set_points_f64(hgmm_ctx* ctx, const double* xyz, int64_t n);
int64_t hgmm_num_points(const hgmm_ctx* ctx);
/* Several resident clouds per context -- what any number of `cupy.asarray(frame)` arrays are to the reference (the H2D
 * copy of every frame in gmm_waymo/src/waymoutils.py, `dev_X` in gmm.py:73): a handle owns its device copy (float32
 * rows + float64 structure of arrays, like hgmm_set_points_*), hgmm_points_bind makes it the cloud every following
 * call of the context works on -- a pointer swap: nothing is copied, nothing waits, kernels already enqueued keep the
 * cloud they were launched on.  bind(ctx, NULL) goes back to the cloud of hgmm_set_points_* (the one-cloud shortcut,
 * which stays).  Destroying the bound handle leaves nothing bound.  Handles must be destroyed before their context. */
typedef struct hgmm_points hgmm_points;
int hgmm_points_create_f32(hgmm_ctx* ctx, const float* xyz, int64_t n, hgmm_points** out);
int hgmm_points_create_f64(hgmm_ctx* ctx, const double* xyz, int64_t n, hgmm_points** out);
int hgmm_points_bind(hgmm_ctx* ctx, hgmm_points* points);
int hgmm_points_destroy(hgmm_ctx* ctx, hgmm_points* points);
int64_t hgmm_points_count(const hgmm_points* points);
/* The float32 rows [n,3] of a resident cloud back on the host (`cupy.asnumpy(dev_X)`): what a caller needs to draw the
 * reference's initial parameters (init_gmm_params samples the HOST array, gmm_waymo/src/gmm_impl.py:26-41) for a cloud it
 * only holds as a handle.  points = NULL: the cloud the context is working on.  Synchronises the context's stream. */
int hgmm_points_download_f32(hgmm_ctx* ctx, const hgmm_points* points, float* xyz_out);

/* ---- flat GMM EM (diag / spherical) ------------------------------------------------
 * hgmm_flat_estep   <- e_step()            gmm_waymo gmm_impl.py:105-116, gmmreg_gpu gmm_impl.py:55-61
 *                      (+ estimate_log_prob[_spherical] 53-78)
 * hgmm_flat_predict <- predict()           gmm_waymo gmm_impl.py:147-155, gmmreg_gpu gmm_impl.py:88-91
 * hgmm_flat_mstep   <- m_step()            gmm_waymo gmm_impl.py:90-103 (+81-88), gmmreg_gpu gmm_impl.py:46-52
 * hgmm_flat_train   <- train_gmm()         gmm_waymo gmm_impl.py:118-145, gmmreg_gpu gmm_impl.py:63-85
 *
 * mu [J,3], inv_std / cov [J,3] (diag) or [J] (spherical), w [J]: host float32.
 * dev_log_resp [N,J] row-major, dev_lpn [N], dev_argmax [N]: device buffers or NULL.    */
int hgmm_flat_estep(hgmm_ctx* ctx, int cov_type, int variant, int J,
                    const float* mu, const float* inv_std, const float* w,
                    float* dev_log_resp, float* dev_lpn, int32_t* dev_argmax,
                    double* mean_lpn_out);
/* The same E-step without waiting for it: the kernels are enqueued on the context's stream, the host parameter
 * arrays have been copied to the context's pinned staging ring when the call returns (the caller may reuse them),
 * and the mean log-normaliser is written to the DEVICE double dev_mean_lpn (or NULL) by a one-workgroup kernel
 * behind the E-step.  This is what the reference's e_step() is under CuPy (gmm_impl.py:105-116 returns device
 * arrays, nothing synchronises): a following hgmm_flat_mstep overlaps its host work with this kernel. */
int hgmm_flat_estep_async(hgmm_ctx* ctx, int cov_type, int variant, int J,
                          const float* mu, const float* inv_std, const float* w,
                          float* dev_log_resp, float* dev_lpn, int32_t* dev_argmax, double* dev_mean_lpn);
/* E-step / M-step with the PARAMETERS in device arrays (dense, the host layouts: mu [J,3], inv_std / cov [J,3] or
 * [J], w [J]) -- what the reference's functions are when they are handed CuPy arrays (`xp = cupy.get_array_module(X)`,
 * gmm_impl.py:91, 106): nothing is staged, nothing is downloaded, nothing waits.  hgmm_flat_mstep_dev writes the new
 * parameters to the caller's device arrays; dev_centre_hint may be NULL.  dev_mean_lpn may be a host-visible scalar
 * (hgmm_host_scalars). */
int hgmm_flat_estep_dev(hgmm_ctx* ctx, int cov_type, int variant, int J,
                        const float* dev_mu, const float* dev_inv_std, const float* dev_w,
                        float* dev_log_resp, float* dev_lpn, int32_t* dev_argmax, double* dev_mean_lpn);
int hgmm_flat_mstep_dev(hgmm_ctx* ctx, int cov_type, int variant, int J,
                        const float* dev_resp, int is_log, const float* dev_centre_hint,
                        float* dev_w, float* dev_mu, float* dev_cov);
int hgmm_flat_predict_dev(hgmm_ctx* ctx, int cov_type, int variant, int J,
                          const float* dev_mu, const float* dev_inv_std, const float* dev_w,
                          int32_t* dev_labels);
/* The store pacer of the two N x J writers (hgmm_flat_estep*, hgmm_flat_log_prob): *target_gbs_out = the rate the next
 * paced launch offers its rows at (GB/s; 0 = un-paced), *steps_down_out / *steps_up_out = how often the context's
 * controller has lowered it / raised it for good since the context was created.  The rate starts just below the write
 * path's congestion knee; three launches in a row that run more than 6 % longer than the rate explains lower it by 2 %;
 * after a run of clean launches it is raised by 2 % on probation (one long launch takes that back and caps the rate).
 * Measurement aid, no reference counterpart. */
int hgmm_pace_info(hgmm_ctx* ctx, double* target_gbs_out, int* steps_down_out, int* steps_up_out);
/* Forget what the controller has learnt (rate, ceiling, counters): the next paced launch starts at the initial rate again.
 * A rate that congested once is remembered as a ceiling -- rightly while its cause lasts (another stream writing, a hot
 * chip), wrongly for ever: the controller forgets a ceiling by itself after 10 000 clean launches below it
 * (HGMM_PACE_FORGET=<n>); a caller that knows the cause is gone says so here.  Measurement aid, no reference counterpart. */
int hgmm_pace_reset(hgmm_ctx* ctx);
/* Un-normalised per-pair log-densities log N(x_i; mu_j, diag) -> dev_log_prob [N,J]
 * (estimate_log_prob / estimate_log_prob_spherical, gmm_waymo gmm_impl.py:53-78). */
int hgmm_flat_log_prob(hgmm_ctx* ctx, int cov_type, int J, const float* mu, const float* inv_std,
                       float* dev_log_prob);
int hgmm_flat_predict(hgmm_ctx* ctx, int cov_type, int variant, int J,
                      const float* mu, const float* inv_std, const float* w,
                      int32_t* dev_labels);
/* dev_resp: [N,J] responsibilities (is_log = 0) or log-responsibilities (is_log = 1, the
 * exp() of train_gmm's `m_step(X, xp.exp(log_resp))` is then fused into the read).
 * centre_hint [J,3] (host, may be NULL): moments are accumulated about it to avoid the
 * raw-second-moment cancellation; results are mathematically independent of it.        */
int hgmm_flat_mstep(hgmm_ctx* ctx, int cov_type, int variant, int J,
                    const float* dev_resp, int is_log, const float* centre_hint,
                    float* w_out, float* mu_out, float* cov_out);
/* Whole loop device-resident (fused E+M, no N x J traffic).  mu/cov/w: in = initial,
 * out = final.  lls has room for max_iter floats.                                      */
int hgmm_flat_train(hgmm_ctx* ctx, int cov_type, int variant, int J, int max_iter, float tol,
                    float* mu, float* cov, float* w, float* inv_std_out,
                    float* lls_out, int* n_iter_out, int* converged_out);
/* The same loop split so a caller (bench, streaming refit) can time / interleave steps:
 * begin uploads the initial parameters, step enqueues `iters` EM iterations without
 * synchronising, end synchronises and downloads.                                       */
int hgmm_flat_train_begin(hgmm_ctx* ctx, int cov_type, int variant, int J, float tol,
                          const float* mu, const float* cov, const float* w, int lls_capacity);
int hgmm_flat_train_step(hgmm_ctx* ctx, int iters);
int hgmm_flat_train_end(hgmm_ctx* ctx, float* mu, float* cov, float* w, float* inv_std_out,
                        float* lls_out, int* n_iter_out, int* converged_out);
/* B independent fits in ONE launch set -- B x train_gmm() of either flavour (gmm_waymo gmm_impl.py:118-145, gmmreg_gpu
 * gmm_impl.py:63-85): the reference's streaming driver fits frame after frame, and a fit of a scan-sized cloud is a chain of
 * launches that leaves most of the chip idle.  clouds [B] are handles of this context (hgmm_points_create_*).
 * SEMANTICS.  Member b is hgmm_flat_train on a context whose cloud is clouds[b], with no weights in force: its mu, cov, w,
 * inv_std, lls, n_iter and converged come out BIT FOR BIT as the serial entry returns them, whatever B is and whoever the
 * neighbours are.  The members differ in their cloud and its size, in their initial parameters and in the iteration at which
 * the device-side stop rule fires; they share cov_type, variant, J, max_iter and tol.  A handle may occur several times
 * (K restarts of one resident cloud: K slots, K initialisations, the caller keeps the best log-likelihood); two slots with
 * the same handle and the same initialisation return the same bits.  The arrays are member-major: mu [B][J][3], cov and
 * inv_std_out [B][J][3] (diag) or [B][J] (spherical), w [B][J], lls_out [B][max(max_iter, 1)] (member b's first n_iter[b]
 * entries are written), n_iter_out and converged_out [B].
 * LAUNCHES.  One `begin` launch per call; per iteration one fused E+M launch over the workgroups of all members (each member
 * has the grid the serial launch gives a cloud of its size), one reduce and one finalize launch; one group of download
 * packets and one synchronisation at the end.  max_iter iterations are enqueued blind, like hgmm_flat_train: a member that has
 * stopped costs every later launch a workgroup that returns at its stop word.
 * LIMITS.  J <= 1024: only the one-pass fused path is batched, the chunked path of larger J stays serial.  1 <= B <= 4096.
 * The members' partial buffers together -- sum_b grid_b x 7 x Jpad x 4 bytes, Jpad = J rounded up to 256 -- are at most
 * 8 GiB.  No communicator.
 * REFUSALS, each before anything resident is touched (hgmm_last_error says why).  HGMM_ERR_ARG: B out of range; clouds NULL
 * or a NULL member; a handle of another context; NULL mu, cov, w, n_iter_out or converged_out; max_iter < 0; a bad cov_type or
 * variant and flavour G with spherical covariances (hgmm_flat_train's own texts); J outside 1..1024; partial buffers above
 * the limit (the message names the figure).  HGMM_ERR_STATE under a communicator.
 * LEFT ALONE.  The batch works in buffers of its own and reads the handles' float32 rows and nothing else of the context: the
 * bound cloud, its flat weights, the serial train loop (a hgmm_flat_train_begin ... _end in progress included) with its
 * parameter block, table, partials, control words and trace, the store pacer, the resident tree, forest, target and voxel
 * result are what they were.  PER-POINT WEIGHTS ARE IGNORED: a handle owns none (hgmm_flat_set_weights), so the weights in
 * force on the context -- also when the bound handle is a member -- do not enter; fit a weighted cloud with hgmm_flat_train. */
int hgmm_flat_train_batch(hgmm_ctx* ctx, int B, hgmm_points* const* clouds /* [B] */,
                          int cov_type, int variant, int J, int max_iter, float tol,
                          float* mu      /* [B][J][3]          in = initial, out = final */,
                          float* cov     /* [B][J][3] | [B][J] in / out */,
                          float* w       /* [B][J]             in / out */,
                          float* inv_std_out /* as cov, may be NULL */,
                          float* lls_out /* [B][max(max_iter,1)], may be NULL */,
                          int32_t* n_iter_out /* [B] */, int32_t* converged_out /* [B] */);
/* hgmm_flat_train_batch with per-point weights that belong to a SLOT OF THIS CALL, not to a handle: s [B] host pointers, s[b]
 * the n_b float32 weights of slot b or NULL (the slot is unweighted); s == NULL is hgmm_flat_train_batch.  Handles still own
 * no weights, and hgmm_points_bind / hgmm_flat_set_weights keep their semantics.
 * SEMANTICS.  Slot b is the sequence hgmm_points_bind(clouds[b]); hgmm_flat_set_weights(s[b], n_b); hgmm_flat_train(...): all
 * seven outputs come out BIT FOR BIT as that sequence returns them, whatever B is and whoever the neighbours are.  S_b, what
 * the M-step divides by, is the float64 host sum of s[b] in index order, as hgmm_flat_set_weights forms it.  A zero weight
 * makes the row absent, NaN coordinates included.  A slot with s[b] == NULL has the unweighted serial fit's bits (so has a
 * slot whose weights are all 1).  One handle may fill several slots with different weights: bootstrap restarts, a caller's
 * own reweighting.
 * LAUNCHES.  The weights of all weighted slots are packed into ONE buffer of the batch's own and uploaded once, before the
 * begin launch; nothing is uploaded between iterations.  The fused launch's workgroups form two segments, the unweighted
 * slots' (the kernels of hgmm_flat_train_batch) and the weighted slots' (the same body with the serial kernels' weight
 * switch); a segment is launched when it is not empty: a mixed batch costs one more fused launch per iteration, a batch of one
 * kind what hgmm_flat_train_batch costs.  Reduce and finalize stay one launch each.
 * LIMITS.  Those of hgmm_flat_train_batch.  The call packs the weights on the host (one pass over them, with the checks).
 * REFUSALS, each before anything resident is touched.  Every refusal of hgmm_flat_train_batch; and, per slot, the value checks of
 * hgmm_flat_set_weights -- a NaN, infinite or negative weight, all-zero weights -- as HGMM_ERR_ARG with a message that names
 * the slot and the index.  (The length of s[b] cannot be checked: it is n_b by contract.)
 * LEFT ALONE.  Everything hgmm_flat_train_batch leaves alone; the context's own flat weights are neither read nor written. */
int hgmm_flat_train_batch_weighted(hgmm_ctx* ctx, int B, hgmm_points* const* clouds /* [B] */,
                                   const float* const* s /* NULL: none; s[b] NULL: slot b unweighted; else host [n_b] */,
                                   int cov_type, int variant, int J, int max_iter, float tol,
                                   float* mu, float* cov, float* w, float* inv_std_out, float* lls_out,
                                   int32_t* n_iter_out /* [B] */, int32_t* converged_out /* [B] */);
/* The batched fit fed from the resident voxel result (hgmm_voxel_downsample_*): slot b is member members[b] of it.
 * SEMANTICS.  Slot b is the sequence hgmm_voxel_to_points(members[b], weighted ? HGMM_VOXEL_W_FLAT : 0); hgmm_flat_train(...),
 * bit for bit: the rows are (float)centroid, the weights (float)count, and S_b is the member's raw point count as a double
 * (hgmm_voxel_to_points' rule).  Unlike that sequence the call does not touch the resident cloud or its weights.  A member
 * may fill several slots.  Outputs as hgmm_flat_train_batch.
 * LAUNCHES.  ONE hand-over launch, whatever B is, writes every slot's rows and weights into buffers of the batch's own; then
 * the launch set of hgmm_flat_train_batch_weighted (weighted: the weighted segment only; else the unweighted one).  No launch
 * per member, no host pass over points or counts, no allocation once the buffers have their size.
 * LIMITS.  Those of hgmm_flat_train_batch.  weighted: a member that stands for 2^24 raw points or more is refused (a count
 * could round as a float32 weight, and S_b would no longer be the weights' sum): hand such a member over with
 * hgmm_voxel_to_points, which sums the counts on the device, and fit it with hgmm_flat_train.
 * REFUSALS.  HGMM_ERR_STATE without a voxel result; HGMM_ERR_ARG for a member outside the result, B < 1, NULL members, a
 * member of 2^24 raw points (weighted); every refusal of hgmm_flat_train_batch that does not concern handles.
 * LEFT ALONE.  Everything hgmm_flat_train_batch leaves alone.  The voxel result is read, not consumed:
 * hgmm_voxel_downsample_get returns the same bytes afterwards. */
int hgmm_flat_train_batch_voxels(hgmm_ctx* ctx, int B, const int32_t* members /* [B] of the voxel result */, int weighted,
                                 int cov_type, int variant, int J, int max_iter, float tol,
                                 float* mu, float* cov, float* w, float* inv_std_out, float* lls_out,
                                 int32_t* n_iter_out /* [B] */, int32_t* converged_out /* [B] */);
/* Sufficient statistics of ONE fused E+M pass on this context's points (after the
 * all-reduce when a communicator is attached): stats [J,7] doubles laid out
 * (s0, a_x, a_y, a_z, b_x, b_y, b_z) with a = sum r (x - mu_old), b = sum r (x - mu_old)^2,
 * plus sum_i lpn_i and the (global) point count.                                        */
int hgmm_flat_stats(hgmm_ctx* ctx, int cov_type, int variant, int J,
                    const float* mu, const float* inv_std, const float* w,
                    double* stats_out, double* sum_lpn_out, double* n_points_out);
/* Per-point weights for the flat (diag / spherical) fit.  The reference has no counterpart: its pipeline voxel-down-samples
 * a scan (run_gmm_static.py:28) and fits the centroids as if each were one point.  Point i with weight s_i >= 0 counts as
 * s_i points.  Let S = sum_i s_i (a float64 sum on the host, in index order, of the float32 values the device holds).  Three
 * statements of the reference change and nothing else does:
 *   M-step          (gmm_waymo gmm_impl.py:90-103, gmmreg_gpu gmm_impl.py:46-52)  resp_ij becomes s_i resp_ij in every sum and
 *                   nk / n becomes nk / S; the + eps terms of both flavours stay where they are, after the sums;
 *   log-likelihood  behind the stop rule (gmm_impl.py:113,136)  mean_i lpn_i becomes sum_i s_i lpn_i / S;
 *   hgmm_flat_stats the statistics and sum_lpn are the s-weighted sums, n_points_out = S.
 * Unchanged: log_resp, the per-point lpn, arg-max, predict, estimate_log_prob, the initialisers (the KMeans seeding of
 * flavour G does NOT see the weights) and the full-covariance, KMeans and tree entries (the full-covariance fit's weights are
 * the SOURCE weights of the tree build: the unweighted entries ignore them; hgmm_fullcov_fit_weighted /
 * hgmm_fullcov_estep_weighted honour them, and never these).
 * Integer weights are repetition (up to the order of summation).  A ZERO WEIGHT MAKES THE ROW ABSENT WHATEVER ITS
 * COORDINATES: the weighted kernels skip such a row instead of multiplying by zero, so a row of NaNs with s = 0 leaves every
 * result finite (a mask).  s == 1 everywhere gives the unweighted results bit for bit; s == 2 everywhere gives exactly twice
 * the hgmm_flat_stats outputs.
 * The weights ATTACH TO THE CLOUD THE CONTEXT IS WORKING ON -- the float32 rows of hgmm_set_points_* or of a bound handle:
 * HGMM_ERR_STATE without one, and with the forest cloud of hgmm_set_points_batch_* resident (it has no float32 rows).
 * Whatever changes the resident cloud drops them: hgmm_set_points_f32 / _f64, hgmm_points_bind (of another cloud),
 * hgmm_set_points_batch_f32 / _f64, hgmm_points_destroy of the bound handle.  A handle does not own weights: they do not
 * survive binding another cloud and coming back (per-handle ownership is out of scope; set them again after the bind).
 * s == NULL: no weights (the unweighted kernels run, every result what it was, bit for bit).  n must equal the resident
 * count; a NaN, infinite or negative weight (hgmm_last_error names its index) and all-zero weights are refused on the host
 * before anything is touched: HGMM_ERR_ARG, and the previous weights stay in force.
 * Honoured by hgmm_flat_train, hgmm_flat_train_begin / _step / _end, hgmm_flat_stats, hgmm_flat_mstep, hgmm_flat_mstep_dev
 * and by the MEAN written by hgmm_flat_estep, _async and _dev -- under a communicator too: each rank holds the weights of its
 * shard, and the point-count slot that travels with the statistics carries the rank's S.  IGNORED by everything else.       */
int hgmm_flat_set_weights(hgmm_ctx* ctx, const float* s /* host [n]; NULL = no weights */, int64_t n);

/* All-reduces this context has enqueued on its communicator so far, and the level-iterations hgmm_tree_build has enqueued
 * behind a level's stop (each costs two all-reduces on unchanged operands): under a communicator every rank must issue
 * the same collectives, so each rank tops its queue up to min(iterations + tree_ahead, budget) per level -- 2 surplus
 * iterations per level by default (round 5: up to 15).  Either pointer may be NULL.                                    */
int hgmm_comm_stats(hgmm_ctx* ctx, unsigned long long* collectives_out, unsigned long long* surplus_tree_iterations_out);

/* ---- per-context options ---------------------------------------------------------------------------------------------
 * The library reads the environment ONCE, in hgmm_create: every option below starts from HGMM_<NAME IN CAPITALS> when
 * that variable is set, else from its default, and can be changed per context afterwards.  Each option selects a path
 * that data also reaches (another J, another cloud size, a failed factorisation) or a documented operating mode; the table
 * is in INTEGRATION.md and tests/test_config_gpu.py runs every option against its golden.  There is no reference
 * counterpart: the reference has no configuration beyond its call arguments.
 *   estep_target_gbs (-1)   store pacing of e_step()'s kernel: -1 controlled, 0 un-paced, > 0 fixed rate in GB/s
 *   pace_start (6600), pace_forget (10000)   the pacing controller's start rate / clean launches until a learnt ceiling is forgotten
 *   predict_single_row (0)  predict() on the general single-row kernel
 *   tree_no_chol (0), tree_rel (0)   symmetric form of the tree pdfs' exponent / relative reach test of the level log-likelihood
 *   tree_ahead (2), tree_tickets (0), tree_overlap (1)   hgmm_tree_build's host look-ahead, where its stop rule runs, E-step
 *                           of iteration e + 1 inside iteration e's log-likelihood launch
 *   fullcov_two_pass (0)    two-kernel form of hgmm_fullcov_fit's iteration (the path of J > 1024)
 *   kmpp_two_launches (0), kmeans_acc_regs (0)   the KMeans initialiser's paths for > 16.7 M points / k > 1024
 *   ipc_timeout_s (20)      seconds the peer exchange waits for a peer before the collective is reported as failed        */
int hgmm_config_count(void);
const char* hgmm_config_name(int index);                      /* NULL beyond hgmm_config_count() - 1 */
int hgmm_config_set(hgmm_ctx* ctx, const char* name, int value);
int hgmm_config_get(hgmm_ctx* ctx, const char* name, int* value_out);

/* ---- hierarchical GMM (8-ary tree, full 3x3 covariance, float64) -------------------
 * hgmm_tree_build     <- buildGMMTree()     hgmm/hgmm_cupy_cpu_working.py:122-160 (CPU twin,
 *                        canonical) == hgmm/hgmm_gpu.py:466-548 (kernels 107-115, 387-426)
 * hgmm_tree_set_nodes <- GMMTree._nodes     hgmm_cupy_cpu_working.py:334,341
 * hgmm_tree_reg_estep <- gmmTreeRegESTep()  hgmm_cupy_cpu_working.py:202-228 == hgmm_gpu.py:550-577
 *
 * T = 8 (8^L - 1) / 7 nodes.  init_mu [T,3] host float64 (RNG stays with the caller).
 * Outputs pi [T], mu [T,3], cov [T,3,3] host float64; leaf_idx [N] = currentIdx after the
 * last level (may be NULL); iters_per_level [L]; q_trace[q_capacity] (may be NULL).     */
int hgmm_tree_build(hgmm_ctx* ctx, int L, double ls, double ld, const double* init_mu,
                    double sig2, int max_iters_per_level,
                    double* pi_out, double* mu_out, double* cov_out, int32_t* leaf_idx_out,
                    int32_t* iters_per_level_out, double* q_trace_out, int q_capacity,
                    int* q_len_out);
int hgmm_tree_set_nodes(hgmm_ctx* ctx, int L, const double* pi, const double* mu,
                        const double* cov);
/* Arithmetic type of the pdf evaluations behind hgmm_tree_build's STOP RULE.  The reference has both: its CPU twin is
 * float64 throughout (hgmm_cupy_cpu_working.py; the default here and the parity reference), its GPU file float32
 * throughout (`points.astype(np.float32)`, float32 node and moment arrays: hgmm/hgmm_gpu.py:472, 478-484).
 * HGMM_PRECISION_F32_PDF: the level log-likelihood q = sum_i log max(sum_j pi_j N(x_i; j), eps) (logLikelihoodValue,
 * hgmm_gpu.py:107-115) evaluates its N x 8^(l+1) Gaussians in packed float32 on coordinates relative to the workgroup's
 * first point (formed in float64), with log() and the sum over the points in float64 -- on clouds of any size and in
 * hgmm_tree_build_batch (round 6; round 5: clouds of >= 400 000 points only).  Level 0 of a small cloud or a forest needs
 * no such kernel in either mode: its q comes out of the float64 E-step's own eight terms.  The E-step, the moments and
 * the M-step stay float64: a level that stops after the same number of iterations yields the float64 tree bit for bit; q
 * itself differs by ~1e-7 relative (|dq| < 1 % of the smallest stop threshold in use on every cloud tried,
 * tests/test_tree_gpu.py, tests/test_tree_batch_gpu.py).
 * The flat FULL-covariance fit (hgmm_fullcov_fit / hgmm_fullcov_estep, J <= 1024) under the same setting takes its
 * float32-TILE kernel (round 6): pdfs from head + tail differences in packed float32, the 16-point tile of un-normalised
 * responsibilities in float32, the statistics' products on v_mfma_f32_16x16x4_f32 about the cloud's centroid (float
 * partials per 256 points, added in float64); row sums, 1 / den, log() and the M-step float64.  1.69 -> 1.21 ms per
 * launch at N = 10^6, J = 800; against the float64 fit after 3 iterations there: pi 2e-6, mu 2e-7, Sigma 7e-6 of a
 * component's variance, 2 of 10^6 labels (tests/test_fullcov_gpu.py).  float64 stays the default and the parity reference.
 * Stays in force for the context until set again. */
enum { HGMM_PRECISION_F64 = 0, HGMM_PRECISION_F32_PDF = 1 };
int hgmm_tree_set_precision(hgmm_ctx* ctx, int precision);
/* Registration target cloud (host [n,3] float64), kept resident across iterations. */
int hgmm_tree_set_target(hgmm_ctx* ctx, const double* xyz, int64_t n);
/* E-step of the registration loop on the resident target transformed on the fly by
 * x' = scale * R x + t (R row-major [3,3]; pass NULL for identity).  Outputs host
 * float64 m0 [T], m1 [T,3], m2 [T,3,3].                                                 */
int hgmm_tree_reg_estep(hgmm_ctx* ctx, const double* rot, const double* t, double scale,
                        double lambda_c, double* m0_out, double* m1_out, double* m2_out);
/* E-step + normal equations of one registration iteration (GMMTree.expectation_step + the least-squares
 * system of GMMTree.maximization_step, hgmm/hgmm_gpu.py:722-752), entirely on the device: out28 (host) =
 * the 21 upper-triangle entries (row-major) of A^T A, the 6 of A^T b, and b^T b of the reference's stacked
 * twist system  [ s_i x n | n ] x = n . (mu_i - s_i); the caller solves the 6 x 6 system and composes the
 * twist (hgmm_gpu.py:620-664), residual q = b^T b - x . A^T b.  Deterministic (fixed-point moment sums). */
int hgmm_tree_reg_normal(hgmm_ctx* ctx, const double* rot, const double* t, double scale,
                         double lambda_c, double* out28);
/* The registration loop of GMMTree.registration (src/python/hgmm/hgmm_gpu.py:754-768) run by the library: per
 * iteration hgmm_tree_reg_normal on the device, then on the host the 6 x 6 solve, q = max(b'b - x.A'b, 0), the
 * composition of the twist with (rot, t) (twist_mul, hgmm_gpu.py:634-664) and the reference's stop rule
 * |q - q_prev| < tol.  rot [9] row-major and t [3] are updated in place; *q_prev_inout: NaN = no previous q.
 * status: 0 = max_iter iterations done, 1 = stopped by tol, 2 = the normal equations of the NEXT iteration are too
 * ill-conditioned (or not finite): the caller runs that iteration with the reference's stacked least squares
 * (eigh + QR on the host) and may call again.  trace (optional): per iteration rot, t, q.
 * Per-context option reg_device_solve = 1 (hgmm_config_set; off by default -- the host solve is the parity reference):
 * the whole loop runs on the device -- Cholesky solve of the 6 x 6 system, twist, stop rule and the fixed-point encoding
 * of the next E-step in one device thread behind the normal equations, the host only follows a progress word.  Status 2
 * is decided by the host path's own rule, in the same function (lambda_min <= 1e-11 lambda_max, behind a Cholesky
 * certificate of the opposite): the device never goes on where the host hands over.  The Cholesky pivots alone do not
 * decide it -- smallest pivot / largest diagonal entry >= lambda_min / lambda_max, so small pivots imply the rule and the
 * rule does not imply small pivots.  Where both go on: the same trajectory to ~1e-12 on well-conditioned pairs, in general
 * to the order of cond(A^T A) 2^-52 |twist| per iteration (device sin / cos, fused multiply-adds, Cholesky instead of
 * pivoted elimination).  Not under a communicator.      */
int hgmm_tree_register(hgmm_ctx* ctx, double* rot, double* t, double scale, double lambda_c, int max_iter, double tol,
                       double* q_prev_inout, int* iters_out, int* status_out, double* trace);
/* Mahalanobis GATE of the registration E-step (robustness to clutter and partial overlap).  The reference has no counterpart:
 * gmmTreeRegESTep (hgmm_cupy_cpu_working.py:202-228 == hgmm_gpu.py:550-577), the function whose accumulation this restricts,
 * normalises the eight children's responsibilities among themselves, so a point that belongs to none of them still gets
 * gamma ~ 1 for the least bad child and pulls that node's moments with full weight.  With a finite gate a target point
 * y = scale * R x + t that would contribute to node s at a level (it has not stopped there and its responsibility is >= 1e-15)
 * contributes iff
 *     (y - mu_s)^T Sigma_s^-1 (y - mu_s) <= maha2_gate,
 * the quantity hgmm_tree_score reports as maha2.  The DESCENT is not gated: a point gated out at a coarse level still moves
 * to its arg-max child, may contribute at a finer level and stops where it stops without the gate.  A point with a
 * non-finite coordinate (NaN form) contributes nothing under a finite gate.  The sums stay the deterministic fixed-point
 * sums of the ungated E-step.  maha2_gate = +inf (the default): off -- the ungated kernels run and every result is what it
 * was, bit for bit.  NaN or a gate <= 0: HGMM_ERR_ARG, the previous gate stays.  Suggested values: the chi-square quantiles
 * of 3 degrees of freedom (11.34 = 99 %, 16.27 = 99.9 %).
 * Honoured by every entry that runs the registration E-step -- hgmm_tree_reg_estep, hgmm_tree_reg_normal,
 * hgmm_tree_register, hgmm_tree_register_multi, hgmm_tree_register_batch, with reg_device_solve and under a communicator
 * alike (the gate is per point: the ranks' shards still add up exactly) -- and by nothing else: hgmm_tree_score* keep their
 * own maha2_max argument, the build has no such step.  Stays in force for the context until set again. */
int hgmm_tree_set_reg_gate(hgmm_ctx* ctx, double maha2_gate);
int hgmm_tree_get_reg_gate(hgmm_ctx* ctx, double* maha2_gate_out);
/* ---- batched HGMM: B independent scan pairs per launch set ("forest") ------------------------------------------------
 * The reference's unit of work is ONE pair -- registration_gmmtree(source, target) (hgmm/hgmm_gpu.py:802-807) =
 * buildGMMTree(source) (hgmm_gpu.py:466-548) + GMMTree.registration(target) (hgmm_gpu.py:754-768, E-step 550-577) -- a
 * chain of ~350 small launches for a 40 k-point scan.  These entries run B such pairs through the SAME launches; every
 * pair's tree, iteration counts, q trace and (R, t) are bitwise those of hgmm_tree_build / hgmm_tree_register on that pair
 * alone (same device functions, same chunks and orders of summation, same host steps).  No communicator.
 *
 * hgmm_set_points_batch_f64   B host arrays [counts[b],3] become ONE resident cloud, cloud after cloud (float64 view only:
 *                             the flat EM entry points refuse it)
 * hgmm_tree_build_batch       <- B x buildGMMTree on the resident cloud's B consecutive pieces (each < 400 000 points);
 *                             init_mu [B][T][3]; outputs (each may be NULL) pi [B][T], mu [B][T][3], cov [B][T][3][3],
 *                             iters [B][L], q_trace [B][q_capacity] + q_len [B] (levels back to back, as hgmm_tree_build).
 *                             The levels run in lock-step: a level lasts as long as its slowest cloud.
 * hgmm_tree_get_nodes_batch   tree b of the resident forest (host tables, as hgmm_tree_build returns them)
 * hgmm_tree_set_targets_batch <- B x hgmm_tree_set_target
 * hgmm_tree_register_batch    <- B x hgmm_tree_register on (tree b, target b): rot [B][9], t [B][3], q_prev [B] (NaN: none)
 *                             updated in place; iters [B]; status [B] as hgmm_tree_register's (a pair that meets status 2
 *                             leaves the batch at that iteration: the caller finishes it through the serial entries);
 *                             trace (optional) [B][max_iter][13].  The 6 x 6 solves stay on the host unless the context's
 *                             reg_device_solve option is set (see hgmm_tree_register): then one device thread per pair.    */
int hgmm_set_points_batch_f64(hgmm_ctx* ctx, int B, const double* const* xyz, const int64_t* counts);
/* ... and from float32 rows (the scans' files, `points.astype(np.float32)` of hgmm/hgmm_gpu.py:472): widened to float64 on
 * the device -- exactly, so every result equals the float64 entry's on the widened arrays -- half the bytes per upload and
 * no conversion pass on the host.  hgmm_tree_set_targets_batch_f32 likewise.                                           */
int hgmm_set_points_batch_f32(hgmm_ctx* ctx, int B, const float* const* xyz, const int64_t* counts);
int hgmm_tree_build_batch(hgmm_ctx* ctx, int B, const int64_t* counts, int L, double ls, double ld,
                          const double* init_mu, double sig2, int max_iters_per_level,
                          double* pi_out, double* mu_out, double* cov_out, int32_t* iters_out,
                          double* q_trace_out, int q_capacity, int32_t* q_len_out);
int hgmm_tree_get_nodes_batch(hgmm_ctx* ctx, int b, double* pi_out, double* mu_out, double* cov_out);
int hgmm_tree_set_targets_batch(hgmm_ctx* ctx, int B, const double* const* xyz, const int64_t* counts);
int hgmm_tree_set_targets_batch_f32(hgmm_ctx* ctx, int B, const float* const* xyz, const int64_t* counts);
int hgmm_tree_register_batch(hgmm_ctx* ctx, int B, double* rot, double* t, double scale, double lambda_c,
                             int max_iter, double tol, double* q_prev_inout, int32_t* iters_out,
                             int32_t* status_out, double* trace);
/* ---- score of a cloud against a tree: labels, Mahalanobis distance, fitness ---------------------------------------------
 * "Did the registration work?"  The reference has no counterpart of the score itself (GMMTree.registration returns the
 * transformation and the least-squares residual q only); the DESCENT it is taken along is gmmTreeRegESTep's
 * (hgmm_cupy_cpu_working.py:202-228 == hgmm_gpu.py:550-577), by the device function the registration E-step itself calls:
 * every point y = scale * R x + t of the resident target (hgmm_tree_set_target; rot / t NULL = identity, as
 * hgmm_tree_reg_estep) moves level by level to the first maximum of pi_k N(y; k) over the eight children (the first child
 * when their sum is <= 1e-15) and stops at a node whose complexity is <= lambda_c, at the latest on level L - 1.  Its node s
 * is the last node reached; lambda_c < 0 therefore labels every point by a node of the last level ("predict").
 * Per point (each array may be NULL):
 *   node  [n] int32    index into the node tables (its level follows from the index)
 *   maha2 [n] float64  (y - mu_s)^T Sigma_s^-1 (y - mu_s); +inf when node s is dead (pi_s = 0 or det Sigma_s < 1e-15)
 *   logp  [n] float64  log pi_s - log((2 pi)^3 det Sigma_s) / 2 - maha2 / 2, formed in log space; -inf for a dead node.
 *                      The path's own term of the level's mixture density: a lower bound of it.
 * A point with a NaN or infinite coordinate (after the pose) gets maha2 = logp = NaN and whatever node the comparisons of
 * the descent led to (NaN compares false: the first child at every level); it is never an inlier and adds to slot 0 only
 * (and to slots 5 / 6 if its node is dead / above the last level).
 * summary [8] (always written), inlier_i = maha2_i <= maha2_max:
 *   [0] n   [1] inliers   [2] sum of maha2 over inliers   [3] sum of |y - mu_s|^2 over inliers   [4] sum of logp over inliers
 *   [5] points whose node is dead   [6] points that stopped above level L - 1   [7] 0 (reserved)
 * fitness = [1] / [0], inlier rmse = sqrt([3] / [1]), Mahalanobis rms = sqrt([2] / [1]), mean log density = [4] / [1] are the
 * caller's to form.  Deterministic: every 256-point workgroup adds its own six sums and one workgroup adds the workgroups'
 * shares in a fixed order (no floating-point atomics), so two calls return the same bits.
 * hgmm_tree_score_batch: the same for all B pairs (tree b, target b) of the resident forest (hgmm_tree_build_batch +
 * hgmm_tree_set_targets_batch) at the poses rot [B][9], t [B][3] (NULL = identity) in one launch, summaries [B][8] only
 * (the per-point arrays of one member: the serial entry) -- bit for bit the serial entry's summary on that pair alone.
 * Every pair is scored, also one that left hgmm_tree_register_batch with status 2.
 * Errors: HGMM_ERR_STATE without a tree / target / forest + targets or under a communicator (sharded targets are not
 * scored); HGMM_ERR_ARG when maha2_max is NaN or summary_out is NULL.                                                     */
int hgmm_tree_score(hgmm_ctx* ctx, const double* rot, const double* t, double scale, double lambda_c, double maha2_max,
                    int32_t* node_out, double* maha2_out, double* logp_out, double* summary_out /* [8] */);
int hgmm_tree_score_batch(hgmm_ctx* ctx, int B, const double* rot /* [B,9] */, const double* t /* [B,3] */, double scale,
                          double lambda_c, double maha2_max, double* summary_out /* [B,8] */);
/* ---- multi-start: K start poses of ONE pair per launch set ---------------------------------------------------------------
 * hgmm_tree_register is a local method: it follows the twist updates from its start to the nearest minimum.  These entries
 * run it from K starts at once on the SERIAL state -- the tree of hgmm_tree_build / hgmm_tree_set_nodes and the target of
 * hgmm_tree_set_target, both resident once -- and score the K outcomes, so that the caller keeps the start the score likes
 * best.  They neither read nor disturb a resident forest or the serial entries' own sums.
 * hgmm_tree_register_multi   <- K x hgmm_tree_register from (rot[k], t[k]): rot [K][9], t [K][3], q_prev [K] (NaN: none)
 *                            updated in place; iters [K]; status [K] with hgmm_tree_register's codes 0 / 1 / 2 (a hypothesis
 *                            that stops costs the remaining launches one load; one that meets status 2 leaves at that
 *                            iteration and the caller finishes it through the serial entries, as a pair of a batch); trace
 *                            (optional) [K][max_iter][13].  One E-step launch of K x ceil(n / 256) workgroups and one
 *                            normal-equations launch of K workgroups per iteration; the 6 x 6 solves on the host unless the
 *                            context's reg_device_solve option is set (then one device thread per hypothesis).
 * hgmm_tree_score_multi      <- K x hgmm_tree_score at the poses rot [K][9], t [K][3], summaries [K][8] only (the per-point
 *                            arrays of one pose: the serial entry).
 * The moments are 64-bit fixed-point integer sums and the score's shares are added in a fixed order, so hypothesis k comes out
 * bit for bit as the serial entry from that start / at that pose.
 * Errors: HGMM_ERR_STATE without a tree or a target, or under a communicator; HGMM_ERR_ARG for K < 1 (or > 4096), NULL
 * rot / t (the poses are the input: no identity default), NULL outputs, a NaN maha2_max.                                   */
int hgmm_tree_register_multi(hgmm_ctx* ctx, int K, double* rot /* [K,9] */, double* t /* [K,3] */, double scale,
                             double lambda_c, int max_iter, double tol, double* q_prev_inout /* [K], NaN = none */,
                             int32_t* iters_out /* [K] */, int32_t* status_out /* [K] */,
                             double* trace /* optional [K,max_iter,13] */);
int hgmm_tree_score_multi(hgmm_ctx* ctx, int K, const double* rot /* [K,9] */, const double* t /* [K,3] */, double scale,
                          double lambda_c, double maha2_max, double* summary_out /* [K,8] */);
/* ---- batched multi-start: R hypotheses over the resident FOREST, each naming its pair --------------------------------------
 * The two remedies combined: the pairs of hgmm_tree_build_batch[_rows] + hgmm_tree_set_targets_batch[_f32] /
 * hgmm_voxel_to_targets_batch stay resident once, and R start poses -- any number per pair, in any order; a pair without one
 * takes no part -- run through the launches of one.  Hypothesis r reads tree pair[r] and target pair[r] (and that pair's
 * weights and weight sum: the hypotheses of a pair share them) and owns slice r of everything that is written.
 * hgmm_tree_register_batch_multi <- R x hgmm_tree_register, replacing a loop of hgmm_tree_register_multi over pairs set
 *                            up serially: rot [R][9], t [R][3], q_prev [R] (NaN: none) updated in place; iters [R]; status [R]
 *                            with hgmm_tree_register's codes (a hypothesis that stops costs the remaining launches one load;
 *                            one that meets status 2 leaves at that iteration, its neighbours -- the other hypotheses of its
 *                            own pair included -- unaffected, and the caller finishes it through the serial entries); trace
 *                            (optional) [R][max_iter][13].  Per iteration one E-step launch of R x ceil(longest target / 256)
 *                            workgroups and one normal-equations launch of R; the 6 x 6 solves on the host unless
 *                            reg_device_solve is set.  The Mahalanobis gate and the targets' weights are honoured.
 * hgmm_tree_score_batch_multi <- R x hgmm_tree_score (replacing hgmm_tree_score_multi per pair) at the poses rot [R][9],
 *                            t [R][3], summaries [R][8] only.
 * Hypothesis r comes out bit for bit as hgmm_tree_set_nodes(hgmm_tree_get_nodes_batch(pair[r])) + hgmm_tree_set_target (+ its
 * weights) + hgmm_tree_register / hgmm_tree_score from / at its pose, whatever R is, wherever r sits and whoever its neighbours
 * are; with pair = 0..B-1 the entries return what hgmm_tree_register_batch / hgmm_tree_score_batch return.  They work in sums
 * and a table of their own (32 T bytes of sums per hypothesis: 1.2 MB at L = 5, 9.6 MB at L = 6) and leave the state of
 * hgmm_tree_register_batch / _score_batch, of the serial entries and of the serial multi-start alone.
 * Errors, each before anything resident is touched: HGMM_ERR_STATE without a forest or targets, with B trees but another number
 * of targets, or under a communicator; HGMM_ERR_ARG for R < 1, NULL pair / rot / t (the poses are the input: no identity
 * default) or NULL outputs, pair[r] outside 0..B-1 (the message names r), a NaN maha2_max, more than 2^31 - 1 workgroups, and
 * sums above HGMM_TREE_BATCH_MULTI_MAX_BYTES (the message names the largest R that fits: split the list, any subset is a call). */
#define HGMM_TREE_BATCH_MULTI_MAX_BYTES 4294967296ull /* 4 GiB: 3584 hypotheses at L = 5, 448 at L = 6 */
int hgmm_tree_register_batch_multi(hgmm_ctx* ctx, int R, const int32_t* pair /* [R], each in 0..B-1 */, double* rot /* [R,9] */,
                                   double* t /* [R,3] */, double scale, double lambda_c, int max_iter, double tol,
                                   double* q_prev_inout /* [R], NaN = none */, int32_t* iters_out /* [R] */,
                                   int32_t* status_out /* [R] */, double* trace /* optional [R,max_iter,13] */);
int hgmm_tree_score_batch_multi(hgmm_ctx* ctx, int R, const int32_t* pair /* [R] */, const double* rot /* [R,9] */,
                                const double* t /* [R,3] */, double scale, double lambda_c, double maha2_max,
                                double* summary_out /* [R,8] */);
/* Per-point WEIGHTS of the registration target.  The reference has no counterpart: gmmTreeRegESTep
 * (hgmm_cupy_cpu_working.py:202-228 == hgmm_gpu.py:550-577) counts every target point as one unit of evidence, although its
 * own pipeline voxel-downsamples the scans first (run_gmm_static.py:28).  A target point i with weight w_i >= 0 adds
 * w_i * gamma to a node's moments where it added gamma -- a voxel centroid with its count, a return weighted by range or
 * incidence, the caller's own M-estimator weights (e.g. from hgmm_tree_score's maha2).  Everything else is what it was: the
 * DESCENT, the stop rule and the Mahalanobis gate do not see the weight, the 1e-15 floor is tested on gamma (not on
 * w_i gamma), the sums stay the deterministic fixed-point sums, whose encoding takes the sum of the weights (a float64 sum
 * on the host, in index order; all-reduced under a communicator) where it took the number of points.  A zero weight adds
 * nothing.  w == 1 everywhere gives the unweighted results bit for bit, w == 2 everywhere exactly twice the moments.
 * The moments are LINEAR IN THE WEIGHTS AT ANY POSITIVE SCALE: the encoding's fractional bits follow the exponent of the sum
 * (sum < 2^e: 62 - e bits, above and below 1 alike), so weights in [0, 1] whose sum is far below 1 are summed at the relative
 * resolution counts are; c w gives c times the moments of w to the same relative bound for any c > 0, and exactly so -- bit
 * for bit -- when c is a power of two.  The registration M-step, however, READS WEIGHTS AS POINT COUNTS: like the
 * reference's it leaves a node with m0 < float32 eps (1.19e-7) out of the twist system, so weights scaled down until the
 * nodes' m0 reach that threshold lose nodes, and in the end the whole system (status 2).
 * The weights ATTACH TO THE RESIDENT TARGET: hgmm_tree_set_target (serial, multi-start) resp.
 * hgmm_tree_set_targets_batch[_f32] (batch) first -- HGMM_ERR_STATE without one -- and uploading a new target drops them.
 * w == NULL: no weights (the unweighted kernels run, every result what it was, bit for bit); in the batch w[b] == NULL leaves
 * pair b unweighted (bitwise its unweighted results).  n resp. counts[b] must equal the resident counts; a NaN, infinite or
 * negative weight (hgmm_last_error names its index) and a cloud whose weights are all zero are refused: HGMM_ERR_ARG, and
 * the previous weights stay in force.
 * Honoured by hgmm_tree_reg_estep, hgmm_tree_reg_normal, hgmm_tree_register, hgmm_tree_register_multi (the K hypotheses share
 * the one array), hgmm_tree_register_batch -- with reg_device_solve, with a finite gate and under a communicator alike (each
 * rank holds the weights of its shard) -- and by the summaries of hgmm_tree_score, hgmm_tree_score_batch and
 * hgmm_tree_score_multi: summary[0] = sum of w, summary[1..6] = the w-weighted sums of what they are without weights, added in
 * the same fixed order; the per-point arrays node / maha2 / logp are not weighted.  NOT honoured by the build (hgmm_tree_build*:
 * the weights of a SOURCE cloud are hgmm_tree_set_source_weights', below) nor by any flat, full-covariance or KMeans entry:
 * they ignore them (the flat fit has weights of its own: hgmm_flat_set_weights; the full-covariance fit and the KMeans
 * initialiser take the SOURCE weights: the unweighted entries ignore them; hgmm_fullcov_fit_weighted /
 * hgmm_fullcov_estep_weighted and hgmm_kmeans_plusplus_weighted / _step_weighted / _lloyd_weighted honour them).             */
int hgmm_tree_set_target_weights(hgmm_ctx* ctx, const double* w /* host [n]; NULL = no weights */, int64_t n);
int hgmm_tree_set_target_weights_batch(hgmm_ctx* ctx, int B,
                                       const double* const* w /* w == NULL: none; w[b] == NULL: pair b unweighted */,
                                       const int64_t* counts);
/* Per-point weights of the SOURCE cloud, for the tree build.  The reference has no counterpart: buildGMMTree
 * (hgmm_cupy_cpu_working.py:122-198) counts every source point as one unit of evidence, although its own pipeline
 * voxel-downsamples both scans first (run_gmm_static.py:28).  A source point i with weight w_i >= 0 counts as w_i points.
 * Three statements of the reference change and nothing else does:
 *   gmmTreeEStep        (C:162-191, accumulate C:95-106)  the moments are sum_i w_i gamma_ij (1, x_i, x_i x_i^T); the 1e-15
 *                       floor is tested on gamma (not on w_i gamma), and the arg-max child -- the partition -- does not see
 *                       the weight;
 *   mlEstimator         (C:109-119)  pi_j = m0_j / W with W = sum_i w_i (a float64 sum on the host, in index order) where it
 *                       was m0_j / N; the m0 < ld rule, mu and cov are unchanged and see the weighted moments;
 *   logLikelihoodValue  (C:72-85)    q = sum_i w_i log max(sum_j [pi_j >= eps] pi_j N(x_i; j), eps); the stop rule
 *                       |q - q_prev| < ls is unchanged -- with counts as weights ls means for 2 000 centroids what it
 *                       means for the 40 000 points they stand for.
 * Integer weights are repetition (the build of (X, c) is the build of X with row i repeated c_i times, up to the order of
 * summation); a zero weight makes a point absent: it is still partitioned, it adds nothing.  w == 1 everywhere gives the
 * unweighted tree, iteration counts and q trace bit for bit; w == 2 everywhere with ls and ld doubled gives the unweighted
 * tables and iteration counts at (ls, ld) bit for bit and exactly twice the q trace.  Non-finite coordinates are not covered.
 * The weights ATTACH TO THE CLOUD THE CONTEXT IS WORKING ON: the serial entry to the float64 view of hgmm_set_points_* or of
 * a bound handle, the batch entry to the resident forest cloud of hgmm_set_points_batch_* -- HGMM_ERR_STATE without one.
 * Whatever changes the resident cloud drops them: hgmm_set_points_f32 / _f64, hgmm_points_bind (of another cloud),
 * hgmm_set_points_batch_f32 / _f64, hgmm_points_destroy of the bound handle.
 * w == NULL: no weights (the unweighted kernels run, every result what it was, bit for bit); in the batch w[b] == NULL leaves
 * cloud b unweighted (bitwise its unweighted tree, next to weighted neighbours).  n resp. counts[b] must equal the resident
 * counts; a NaN, infinite or negative weight (hgmm_last_error names its index) and a cloud whose weights are all zero are
 * refused on the host before anything is touched: HGMM_ERR_ARG, and the previous weights stay in force.
 * Honoured by hgmm_tree_build (serial entry) and hgmm_tree_build_batch (batch entry), in both precisions of
 * hgmm_tree_set_precision, by the flat full-covariance entries that ask for them (serial weights: hgmm_fullcov_fit_weighted,
 * hgmm_fullcov_estep_weighted, below), by the KMeans entries that ask for them (serial weights: hgmm_kmeans_plusplus_weighted,
 * hgmm_kmeans_step_weighted, hgmm_kmeans_lloyd_weighted, below), and by nothing else.  IGNORED by the stand-alone steps below
 * (hgmm_tree_estep, hgmm_tree_mstep, hgmm_tree_loglik and the generic E-step kernel behind them), by every flat entry (the
 * flat fit has weights of its own: hgmm_flat_set_weights), by hgmm_fullcov_fit / hgmm_fullcov_estep and hgmm_kmeans_plusplus /
 * _step / _lloyd / _labels (the unweighted entries ignore them; `_weighted` honours them), and by the registration and score
 * entries (their weights are the TARGET's, above).  Under a communicator hgmm_tree_build with
 * weights resident returns HGMM_ERR_STATE: sharded weighted builds are not supported.                                        */
int hgmm_tree_set_source_weights(hgmm_ctx* ctx, const double* w /* host [n]; NULL = no weights */, int64_t n);
int hgmm_tree_set_source_weights_batch(hgmm_ctx* ctx, int B,
                                       const double* const* w /* w == NULL: none; w[b] == NULL: cloud b unweighted */,
                                       const int64_t* counts);
/* The steps buildGMMTree is made of, one at a time (reference function granularity).  Node tables
 * hold T nodes (any T >= 8, need not be a complete tree).
 * hgmm_tree_estep  <- gmmTreeEStep()       hgmm_cupy_cpu_working.py:162-191: parent_idx[N] arbitrary
 *                     (-1 = root), returns moments of ALL nodes + currentIdx[N]
 * hgmm_tree_mstep  <- gmmTreeMStep()       hgmm_cupy_cpu_working.py:193-198: ML update (with the
 *                     m0 < ld rule) of nodes [j_begin, j_end) in place
 * hgmm_tree_loglik <- logLikelihoodValue() hgmm_cupy_cpu_working.py:72-85 over nodes [j_begin, j_end) */
int hgmm_tree_estep(hgmm_ctx* ctx, int64_t T, const double* pi, const double* mu, const double* cov,
                    const int32_t* parent_idx, double* m0_out, double* m1_out, double* m2_out,
                    int32_t* current_idx_out);
int hgmm_tree_mstep(hgmm_ctx* ctx, int64_t T, const double* m0, const double* m1, const double* m2,
                    int64_t j_begin, int64_t j_end, double n_points, double ld, double* pi_inout,
                    double* mu_inout, double* cov_inout);
int hgmm_tree_loglik(hgmm_ctx* ctx, int64_t T, const double* pi, const double* mu, const double* cov,
                     int64_t j_begin, int64_t j_end, double* q_out);
/* Work actually done by the level log-likelihood kernels since the last hgmm_tree_build / hgmm_tree_set_nodes /
 * stand-alone step started (measurement aid for bench.py, no reference counterpart): *pairs_out = number of
 * (point, node) pairs whose pdf was evaluated -- the reference's logLikelihoodValue (hgmm_gpu.py:107-115) visits all
 * N x 8^(l+1); nodes with pi < eps contribute exactly 0 there and nodes whose pdf underflows to 0.0 for every point
 * of a workgroup are rejected per workgroup here, so the count is smaller --, *flags_out bit 0 = some node's
 * Sigma^-1 was not numerically positive definite (the kernels then evaluate the symmetric quadratic form). */
int hgmm_tree_stats(hgmm_ctx* ctx, unsigned long long* pairs_out, int* flags_out);
/* smallest eigenvalue / trace per node (complexity(), hgmm_cupy_cpu_working.py:87-91) */
int hgmm_tree_node_complexity(hgmm_ctx* ctx, double* cplx_out);

/* ---- flat GMM EM, FULL 3x3 covariance (float64) --------------------------------------
 * The reference's Python has no flat full-covariance EM; its in-scope definition
 * is ONE tree level with branching J: the CPU twin run with its module global n_node = J and
 * maxTreeLevel = 1 (hgmm_cupy_cpu_working.py:30, 62-198): pi0 = 1/J, cov0 = sig2 I,
 * gamma = pi N / sum, gammas < 1e-15 dropped, m0 < ld -> (pi = 0, mu = 0, cov = I), stop when
 * |q - q_prev| < ls.  Statistics are the 10 floats per cluster (m0, m1[3], unique m2[6]) that
 * the multi-GPU all-reduce exchanges; they are contracted on the fp64 matrix cores.
 * hgmm_fullcov_estep returns one E-step's moments in the reference layout m0[J], m1[J,3],
 * m2[J,3,3] + hard labels + the level log-likelihood q of the given parameters.            */
int hgmm_fullcov_fit(hgmm_ctx* ctx, int J, double ls, double ld, const double* init_mu, double sig2,
                     int max_iters, double* pi_out, double* mu_out, double* cov_out,
                     int32_t* labels_out, double* q_trace_out, int q_capacity, int* q_len_out);
int hgmm_fullcov_estep(hgmm_ctx* ctx, int J, const double* pi, const double* mu, const double* cov,
                       double* m0_out, double* m1_out, double* m2_out, int32_t* labels_out,
                       double* q_out);
/* The same fit and E-step under the SOURCE weights resident on the context (hgmm_tree_set_source_weights, or
 * hgmm_voxel_to_points(..., HGMM_VOXEL_W_TREE): the counts, with no host trip).  Same argument lists.  The call says what it
 * wants: there is no weight storage, setter, drop rule or switch of its own, and hgmm_fullcov_fit / hgmm_fullcov_estep keep
 * ignoring the weights -- their results are bit for bit what they are, with weights resident or not.
 * The fit is ONE weighted tree level with branching J, i.e. the three statements of hgmm_tree_set_source_weights, with
 * W = the weights' float64 host sum in index order (a voxel member: its raw count):
 *   moments         m = sum_i w_i gamma_ij (1, x_i, x_i x_i^T); the 1e-15 floor is tested on gamma, not on w gamma, and the
 *                   arg-max label does not see the weight;
 *   M-step          pi_j = m0_j / W; the m0 < ld rule, mu and cov are unchanged and see the weighted moments;
 *   log-likelihood  q = sum_i w_i log max(sum_{pi_j >= eps} pi_j N(x_i; j), eps); the stop rule |q - q_prev| < ls is unchanged.
 * A zero weight makes a point add nothing; it is still labelled.  Non-finite coordinates are not covered, as in the tree
 * build.  w == 1 everywhere gives the unweighted entry's outputs bit for bit, in both precisions; w == 2 everywhere with ls
 * and ld doubled gives the unweighted tables, labels and iteration count bit for bit and exactly twice the q trace; integer
 * weights are repetition, up to the order of summation.
 * All three kernel paths take the weights (one-pass float64, the float32 tile of hgmm_tree_set_precision, two-pass): the
 * weight multiplies the point's feature row -- the B operand of the matrix product -- and its log term.  In the float32 tile
 * it is converted to float32 once; the statistics' origin stays the unweighted centroid (a reference point only).
 * Refused before anything resident is touched: HGMM_ERR_STATE without a float64 view, without resident source weights (set
 * them, or call the unweighted entry; a forest cloud's weights are not these) and under a communicator (sharded weighted
 * fits are not supported, as for the weighted tree build); every HGMM_ERR_ARG of the unweighted entries.                    */
int hgmm_fullcov_fit_weighted(hgmm_ctx* ctx, int J, double ls, double ld, const double* init_mu, double sig2,
                              int max_iters, double* pi_out, double* mu_out, double* cov_out,
                              int32_t* labels_out, double* q_trace_out, int q_capacity, int* q_len_out);
int hgmm_fullcov_estep_weighted(hgmm_ctx* ctx, int J, const double* pi, const double* mu, const double* cov,
                                double* m0_out, double* m1_out, double* m2_out, int32_t* labels_out,
                                double* q_out);
/* B clouds fitted by the same launches: the members of the resident FOREST cloud (hgmm_set_points_batch_f64 / _f32,
 * hgmm_voxel_to_points_batch; counts [B] must equal its member counts), one J, ls, ld, sig2 and budget for all of them.
 * init_mu [B][J][3]; the _rows entry takes init_rows [B][J] instead, row numbers WITHIN each member, and gathers the initial
 * means on the device (as hgmm_tree_build_batch_rows does: a voxel batch needs no host trip).
 * THE CONTRACT.  Member b comes out bit for bit as the serial call on that cloud alone -- hgmm_set_points_f64 plus
 * hgmm_fullcov_fit, or hgmm_fullcov_fit_weighted under that member's weights --, whatever B is and whoever its neighbours
 * are: pi_out [B][J], mu_out [B][J][3], cov_out [B][J][3][3], labels_out [sum counts] (member after member; may be NULL),
 * q_trace_out [B][q_capacity] (may be NULL) and q_len_out [B].  Every member has the serial launch's grid (min(tiles, CUs)
 * workgroups and the serial tile-to-workgroup map inside them), its own first point as the origin, its own partials, shares
 * of q, tables, control word, stop rule, q trace and its own Cholesky flag: a member whose Sigma^-1 fails the factorisation
 * takes the symmetric form alone.  An iteration of all members is four launches (M-step over B J components, the one-pass
 * kernel over the sum of the members' grids, the reduction over B J workgroups, B sums of q each applying its member's stop
 * rule); the workgroups of a stopped member return at once and the call ends when every member has stopped.
 * weighted != 0: under the forest cloud's SOURCE weights (hgmm_tree_set_source_weights_batch, or the counts of
 * hgmm_voxel_to_points_batch(..., HGMM_VOXEL_W_TREE)); W_b = the member's float64 host sum in index order (a voxel member:
 * its raw count); a member whose w[b] was NULL carries 1.0 and gives its UNWEIGHTED serial fit bit for bit.  weighted == 0
 * ignores resident weights, like hgmm_fullcov_fit.
 * Refused by name before anything resident is touched: HGMM_ERR_STATE without a resident forest cloud, B other than its
 * member count, under a communicator, with hgmm_tree_set_precision(HGMM_PRECISION_F32_PDF) in force (the batch is the one-pass
 * float64 kernel only and never runs float64 where the serial call would not), with the fullcov_two_pass option set, or with
 * weighted != 0 and no resident forest weights; HGMM_ERR_ARG for B outside 1..4096, counts[b] differing from the resident
 * member, J < 1 or J16 = 16 ceil(J / 16) > 1024 (the two-pass path of the serial entry), NULL init_mu / init_rows / pi_out /
 * mu_out / cov_out / q_len_out, a row number outside its member, and partials of all members above 8 GiB together.        */
int hgmm_fullcov_fit_batch(hgmm_ctx* ctx, int B, const int64_t* counts /* [B] */, int J, double ls, double ld,
                           const double* init_mu /* [B][J][3] */, double sig2, int max_iters, int weighted,
                           double* pi_out /* [B][J] */, double* mu_out /* [B][J][3] */, double* cov_out /* [B][J][3][3] */,
                           int32_t* labels_out /* [sum counts] or NULL */, double* q_trace_out /* [B][q_capacity] or NULL */,
                           int q_capacity, int32_t* q_len_out /* [B] */);
int hgmm_fullcov_fit_batch_rows(hgmm_ctx* ctx, int B, const int64_t* counts /* [B] */, int J, double ls, double ld,
                                const int64_t* init_rows /* [B][J] */, double sig2, int max_iters, int weighted,
                                double* pi_out, double* mu_out, double* cov_out, int32_t* labels_out, double* q_trace_out,
                                int q_capacity, int32_t* q_len_out);

/* ---- KMeans initialiser (float64, on the resident cloud) -------------------------------
 * Replaces the scikit-learn call the GMMReg flavour seeds its EM with
 * (gmmreg_gpu/gmm_impl.py:18-24: KMeans(n_clusters=k, random_state=1, max_iter=50, n_init=1).fit(X),
 * X = the caller's float64 points, gmm.py:79).  The host side (kmeans.py) draws the random
 * numbers, applies the stop rule and relocates empty clusters exactly as scikit-learn does; the
 * two O(N k) parts run on the device:
 * hgmm_kmeans_plusplus  greedy k-means++ seeding.  first_id = the first centre (host-drawn),
 *                       rand_vals[(k-1) * n_trials] = the uniforms of every later step in draw
 *                       order; per step: candidates = searchsorted(cumsum(closest), rand * pot),
 *                       keep the candidate with the lowest potential (first minimum).
 *                       ids_out[k] = chosen point indices, centers_out[k,3] their coordinates.
 * hgmm_kmeans_step      one Lloyd assignment with the given centres: nearest centre per point
 *                       (first minimum), sums_out[k,4] = (sum x, sum y, sum z, count) per cluster,
 *                       inertia = sum of squared distances to the nearest centre, n_changed =
 *                       labels that differ from the previous step's (reset_labels != 0: from -1).
 *                       With a communicator attached the three results are all-reduced.
 * hgmm_kmeans_labels    labels[n] / squared distance to the assigned centre of the last step. */
/* Host-side (no device work): column means / variances / centred copy of an [n,3] float64 cloud, bit for bit what
 * NumPy's X.mean(axis=0), np.var(X, axis=0), X - mean give on a C-ordered array -- the preprocessing of
 * sklearn.cluster.KMeans.fit behind src/python/gmmreg_gpu/gmm_impl.py:20-21. */
int hgmm_kmeans_center_f64(const double* x_host, int64_t n, double* mean3, double* var3, double* xc_out);
int hgmm_kmeans_plusplus(hgmm_ctx* ctx, int k, int64_t first_id, const double* rand_vals, int n_trials,
                         int64_t* ids_out, double* centers_out);
int hgmm_kmeans_step(hgmm_ctx* ctx, int k, const double* centers, int reset_labels, double* sums_out,
                     double* inertia_out, int64_t* n_changed_out);
int hgmm_kmeans_labels(hgmm_ctx* ctx, int32_t* labels_out, double* min_dist2_out);
/* hgmm_kmeans_lloyd     the whole Lloyd loop on the device (single rank): per iteration assignment, sums,
 *                       centres = sums * (1 / count), summed squared centre shift and scikit-learn's stop
 *                       rules in its order (unchanged labels -> strict; shift <= tol_abs; max_iter), several
 *                       iterations enqueued per host synchronisation.  centers_inout: in = start, out = the
 *                       centres after n_iter completed iterations.  An iteration that leaves a cluster empty
 *                       is handed back unfinished (needs_host = 1, its sums[k,4] / changed-label count in
 *                       sums_out / n_changed_out, centres untouched) for the host's relocation rule.        */
int hgmm_kmeans_lloyd(hgmm_ctx* ctx, int k, double* centers_inout, int max_iter, double tol_abs,
                      int reset_labels, int* n_iter_out, int* strict_out, int* needs_host_out,
                      double* sums_out, int64_t* n_changed_out);
/* The same three entries under the SOURCE weights resident on the context (hgmm_tree_set_source_weights, or
 * hgmm_voxel_to_points(..., HGMM_VOXEL_W_TREE): the counts, with no host trip) = the semantics of scikit-learn 1.7.2's
 * KMeans(...).fit(X, sample_weight=w).  Same argument lists.  The call says what it wants: there is no weight storage, setter,
 * drop rule or switch of its own, and hgmm_kmeans_plusplus / _step / _lloyd keep ignoring the weights -- their results are bit
 * for bit what they are, with weights resident or not; hgmm_kmeans_labels is unchanged and serves both.  Point i counts as
 * w_i >= 0 points; whatever is summed over points carries the weight, nothing else does:
 *   seeding   closest_i stays the unweighted squared distance; the potential is sum w_i closest_i, the candidates are
 *             searchsorted(cumsum(w closest), rand * pot) clipped to n - 1, a candidate's potential is
 *             sum w_i min(closest_i, d2(x_i, cand)), first minimum wins.  (The first seed is the host's draw: first_id.)
 *   Lloyd     assignment, labels, per-point distance and changed-label count do not see the weights; sums_out[k,4] =
 *             (sum w x, sum w y, sum w z, sum w) per cluster, centres = sums * (1 / weight), inertia = sum w_i d2_i; a cluster
 *             is EMPTY when its weight is 0 (a cluster that holds only zero-weight points included): hgmm_kmeans_lloyd_weighted
 *             then hands the iteration to the host (needs_host = 1) as the unweighted loop does for a count of 0.  Centre
 *             shift and the three stop rules are unchanged, in their order.
 * A zero weight leaves the point labelled; it adds nothing to sums, weight or inertia, and the threshold search never lands
 * on it.  The weighted kernels keep the traversal and summation order of their unweighted twins: w == 1 everywhere gives the
 * unweighted entries' outputs bit for bit (seeds, labels, sums, centres, inertia, n_iter); w == 2 everywhere gives the
 * unweighted seeds, labels, centres and n_iter bit for bit and exactly twice the sums, weights and inertia; integer weights
 * are repetition, up to the order of summation.  Non-finite coordinates are not covered, as in the tree build.
 * Refused before anything resident is touched: HGMM_ERR_STATE without a float64 view, without resident source weights (set
 * them, or call the unweighted entry; a forest cloud's weights are not these) and under a communicator (sharded weighted
 * fits are not supported, as for the weighted tree build and the weighted full-covariance fit); HGMM_ERR_ARG from
 * hgmm_kmeans_plusplus_weighted for a cloud beyond the one-launch-per-centre seeding form (16.7 M points: the two-launch form
 * of larger clouds is unweighted only); every HGMM_ERR_ARG of the unweighted entries.                                        */
int hgmm_kmeans_plusplus_weighted(hgmm_ctx* ctx, int k, int64_t first_id, const double* rand_vals, int n_trials,
                                  int64_t* ids_out, double* centers_out);
int hgmm_kmeans_step_weighted(hgmm_ctx* ctx, int k, const double* centers, int reset_labels,
                              double* sums_out /* [k,4]: w-sums + weight */, double* inertia_out, int64_t* n_changed_out);
int hgmm_kmeans_lloyd_weighted(hgmm_ctx* ctx, int k, double* centers_inout, int max_iter, double tol_abs,
                               int reset_labels, int* n_iter_out, int* strict_out, int* needs_host_out,
                               double* sums_out, int64_t* n_changed_out);
/* B clouds seeded and clustered by the same launches -- B x KMeans(k, ...).fit(X_b) of the GMMReg flavour's initialiser
 * (gmmreg_gpu/gmm_impl.py:18-24): a scan-sized cloud fills a small part of the chip, and the serial chain is one launch per
 * centre and five per Lloyd iteration.  Works on the resident batch cloud of hgmm_set_points_batch_f64 / _f32, whose B
 * consecutive pieces the caller has centred already; counts [B] must equal the resident members.
 * SEMANTICS.  Member b is the sequence hgmm_set_points_f64(member b); hgmm_kmeans_plusplus(k, first_ids[b], rand_vals[b], ...);
 * hgmm_kmeans_lloyd(..., max_iter, tol_abs[b], reset_labels = 1, ...) and, when the loop did not stop strictly, one more
 * hgmm_kmeans_step against the final centres -- what KMeans.fit drives.  Its seed ids, seed coordinates, final centres, n_iter,
 * strict, the labels of the last assignment and the non-strict inertia come out BIT FOR BIT as that sequence returns them,
 * whatever B is, wherever b sits and whoever its neighbours are: every member gets the serial geometry of a cloud of its size
 * (256-point blocks, 16-block seeding workgroups, 512-point assignment workgroups, the accumulator's workgroup count and
 * contiguous runs, the slot / LDS-or-register choice by k and kmeans_acc_regs, the reduce order, the update rule) and runs the
 * serial kernels' bodies on tables of its own.  The members share k, n_trials and max_iter; each has its size, first seed,
 * uniforms rand_vals [B][k-1][n_trials], start and tol_abs [B].  Either the seeding inputs (first_ids, and rand_vals when
 * k > 1) or init_centres [B][k][3] are given: an explicit start skips the seeding, leaves ids_out unwritten and reports itself
 * in seeds_out (which may then be NULL).
 * Outputs are member-major: ids_out [B][k], seeds_out and centres_out [B][k][3], n_iter_out, strict_out, status_out and
 * inertia_out [B] (0 for a member that stopped strictly: the host forms that inertia, as KMeans.fit does), labels_out [total]
 * (may be NULL) member after member as the clouds lie in the resident cloud.
 * EMPTY CLUSTERS.  A member whose iteration meets an empty cluster leaves the batch at that iteration: status_out[b] = 1, its
 * seeds are valid, its other outputs are unspecified, its neighbours are unaffected.  The caller runs it through the serial
 * entries from its seeds (kmeans.py does); there is no batched relocation.
 * THE CLOUD COPY.  The serial kernels rely on a cloud whose row 0 is buffer-aligned and whose padding rows read as the
 * origin; in the packed batch cloud a member starts at any row and is followed by its neighbour.  One launch therefore copies
 * the members into a buffer of the batch's own, each at a multiple of 4096 rows with zero rows behind it (at most 4095 rows
 * per member): every member sees what the serial cloud shows.
 * LAUNCHES.  One copy launch; per centre one fused seeding launch over the workgroups of all members (the one-launch-per-centre
 * form, whatever kmpp_two_launches says); per Lloyd iteration the five launches of the serial loop plus the update, each over
 * all members, eight iterations per synchronisation, until every member is done (a stopped member's workgroups return at its
 * `done` word); one more assignment for the members that did not stop strictly; one group of download packets.  Nothing is
 * launched per member.
 * LIMITS.  1 <= B <= 4096.  A member has at most 16 777 216 points (4096 seeding workgroups, the one-launch form), the
 * batch cloud fewer than 2^31 - 1024 in all.  The
 * members' per-cluster partial sums together are at most 8 GiB.  No communicator.  Unweighted: resident source weights are
 * ignored, as hgmm_kmeans_plusplus / _lloyd ignore them.
 * REFUSALS, each before anything resident is touched (hgmm_last_error names the member where there is one).  HGMM_ERR_ARG: B
 * out of range; k outside 1..16384; k > counts[b]; n_trials outside 1..16; first_ids[b] out of range; a NULL required
 * argument; both or neither of the seeding inputs and init_centres; max_iter < 0; a member or the partial sums above the
 * limits.  HGMM_ERR_STATE: no resident batch cloud, B or counts that differ from it, a communicator.
 * LEFT ALONE.  The batch works in buffers of its own and reads the resident cloud's float64 view and nothing else: the serial
 * KMeans entries' buffers (labels, distances -- a later hgmm_kmeans_step(reset_labels = 0) counts its changes against what it
 * counted them against before), the resident weights, the tree, the forest, the targets, the voxel result and the flat state
 * are what they were. */
int hgmm_kmeans_fit_batch(hgmm_ctx* ctx, int B, const int64_t* counts /* [B] */, int k,
                          const int64_t* first_ids /* [B] | NULL */, const double* rand_vals /* [B][k-1][n_trials] | NULL */,
                          int n_trials, const double* init_centres /* [B][k][3] | NULL */, int max_iter,
                          const double* tol_abs /* [B] */, int64_t* ids_out /* [B][k] */, double* seeds_out /* [B][k][3] */,
                          double* centres_out /* [B][k][3] */, int32_t* n_iter_out /* [B] */, int32_t* strict_out /* [B] */,
                          int32_t* status_out /* [B] */, double* inertia_out /* [B] */, int32_t* labels_out /* [total] | NULL */);

/* ---- L2 GMMReg: Gauss transform (float64) ---------------------------------------------
 * out[k, i] = sum_j weights[k, j] exp(-|points_i - centres_j|^2 / h^2),  k < n_weights <= 8
 * = GaussTransform(centres, h).compute(points, weights) of gmmreg_gpu/transforms.py:43-86, which
 * cost_functions.py:29-40 evaluates with the target means as centres, the transformed source means
 * as points, h = sqrt(2) sigma and the weight rows phi_t / z, phi_t mu_t / z (one call = the value
 * and the gradient of the L2 cost).  Host arrays in and out (mixture sizes).                    */
int hgmm_gauss_transform(hgmm_ctx* ctx, const double* centres, int n_centres, const double* points,
                         int n_points, const double* weights, int n_weights, double h, double* out);

/* ---- L2 GMMReg: resident mixtures, fused rigid cost + gradient sums for R poses per launch set (float64) ----------------
 * The BFGS solve of the L2 registration (gmmreg.py:62-121) evaluates RigidCostFunction.__call__ (cost_functions.py:29-68)
 * on mixtures that never change while it runs; only the seven parameters do.  hgmm_l2_set_pairs makes the mixtures of B
 * (source, target) pairs resident; hgmm_l2_cost evaluates R hypotheses on them in two launches and one download.
 * Hypothesis r names a pair p = pair[r], a pose (rot[r] row-major, t[r]) and a kernel width sigma[r].  With x_i, phis_i the
 * pair's source centres and weights, mut_j, phit_j its target's, y_i = rot x_i + t, z = (2 pi sigma^2)^(3/2):
 *     e_ij = exp(-|y_i - mut_j|^2 / 2 sigma^2)      g0_i = sum_j (phit_j / z) e_ij      g1_i = sum_j (phit_j mut_j / z) e_ij
 *     grad_i = phis_i (g0_i y_i - g1_i) / 2 sigma^2                                  (compute_l2_dist, cost_functions.py:29-40)
 *     out[r] = { f = -sum_i phis_i g0_i ;  sum_i grad_i (3) ;  M = sum_i grad_i (x) x_i  (3 x 3 row-major: g.T @ mu_source,
 *                cost_functions.py:62-68) }
 * The quaternion chain rule (so.diff_rot_from_quaternion, with the reference's quirks) stays with the caller.
 * DETERMINISTIC AND INDEPENDENT: a workgroup handles 64 source centres against at most 256 target centres, reduces its 13
 * sums across the wave in a fixed order and writes one record; a second kernel adds a hypothesis' records in (source
 * block, target split) order.  That map is a function of (J_s, J_t) alone -- not of R, of the hypothesis' or the pair's
 * position, or of the device -- and there are no floating-point atomics: out[r] is bit for bit what the R = 1 call returns.
 * hgmm_l2_set_pairs: Js [B], Jt [B] component counts; mu_s [sum Js][3], phi_s [sum Js], mu_t [sum Jt][3], phi_t [sum Jt] are
 * host float64 arrays, the pairs' rows back to back.  LIFETIME: the set belongs to the context; a later successful call
 * replaces it, a refused call leaves it as it was, hgmm_destroy frees it.  Nothing else of the context is touched.
 * REFUSALS (hgmm_last_error names each).  hgmm_l2_set_pairs, HGMM_ERR_ARG: a NULL argument; B outside 1..HGMM_L2_MAX_PAIRS;
 * a pair with Js < 1 or Jt < 1 ("J < 1"); more than 2^31 - 1 centres in all.  hgmm_l2_cost, HGMM_ERR_ARG: a NULL argument;
 * R outside 1..HGMM_L2_MAX_HYP; pair[r] out of range; sigma[r] not positive (NaN included); the records of one call above
 * 1 GiB.  HGMM_ERR_STATE: no resident pairs.  A NON-FINITE POSE IS NOT REFUSED: a NaN in it makes its 13 outputs NaN, the other
 * hypotheses' are what they would have been, and the optimiser deals with it. */
#define HGMM_L2_MAX_PAIRS 65536
#define HGMM_L2_MAX_HYP 4096
#define HGMM_L2_NOUT 13
int hgmm_l2_set_pairs(hgmm_ctx* ctx, int B, const int32_t* Js /* [B] */, const double* mu_s /* [sum Js][3] */,
                      const double* phi_s /* [sum Js] */, const int32_t* Jt /* [B] */, const double* mu_t /* [sum Jt][3] */,
                      const double* phi_t /* [sum Jt] */);
int hgmm_l2_cost(hgmm_ctx* ctx, int R, const int32_t* pair /* [R] */, const double* rot /* [R][9] */,
                 const double* t /* [R][3] */, const double* sigma /* [R] */, double* out /* [R][13] */);

/* ---- L2 GMMReg: the whole BFGS solve of R hypotheses on the device, in lock-step (float64) --------------------------------
 * The reference solves theta = (qw, qx, qy, qz, tx, ty, tz) with SciPy's BFGS (gmmreg.py:98-107: method='BFGS', jac=True,
 * tol=opt_tol, options={'maxiter': opt_maxiter}) on RigidCostFunction (cost_functions.py:43-68).  hgmm_l2_solve runs that
 * solve for R hypotheses on the resident pairs of hgmm_l2_set_pairs without the host between two launches: hypothesis r
 * starts at theta0[r] on pair[r] at kernel width sigma[r].  One evaluation is two launches -- the fused cost kernel over the
 * current trial poses, then one wave per hypothesis that adds its records (the 13 sums have the bits hgmm_l2_cost returns for
 * that pose), does the quaternion chain rule (so.quaternion_matrix with its identity rule for |q|^2 < 4 eps,
 * so.diff_rot_from_quaternion with the reference's quirks), one transition of the line search / BFGS state machine and the next
 * trial pose, and stores a progress word the host follows.  The state stays on the device; the outputs are downloaded once.
 * THE OPTIMISER is SciPy 1.15's: _minimize_bfgs over line_search_wolfe1 (dcsrch, c1 = 1e-4, c2 = 0.9, xtol = 1e-14, steps in
 * 1e-100..1e100, at most 100 evaluations per line search), gtol on the infinity norm, old_old_fval = f0 + |g|_2 / 2, rhok = 1000
 * when yk.sk == 0, its NaN and non-finite-f endings -- restated in float64 with + - x / sqrt only, contraction off, in ONE
 * written-down order (csrc/l2_device.h; tests/_l2_solve_model.py is the same in scalar Python, which the device meets bit for
 * bit).  ONE DELIBERATE DIFFERENCE: when dcsrch fails SciPy tries a second line search (line_search_wolfe2) and ends with
 * status 2 at the last accepted iterate only if that fails too; here the solve ends there at once with status 2 (on the
 * multi-start scenario the second search rescued 0 of 25 failures at 12-14 evaluations each: profiles/l2_device_solve.md).
 * nfev therefore differs from SciPy's by design; x, f, nit and status are what compare.
 * OUTPUTS per hypothesis: theta_out the last accepted iterate, f_out its cost, grad_out (may be NULL) its gradient, nit_out the
 * accepted steps, nfev_out the evaluations, status_out: 0 gtol met, 1 max_iter reached, 2 line search failed (or f not finite),
 * 3 NaN.  INDEPENDENT: hypothesis r of any call has the bits of the R = 1 call; no floating-point atomics.  The result is a
 * function of the arguments and the resident set alone, which the entry leaves untouched.
 * hgmm_l2_solve_each is the same with max_iter [R] and gtol [R] of each hypothesis' own.
 * REFUSALS (hgmm_last_error names each; nothing resident is touched).  HGMM_ERR_ARG: a NULL argument (grad_out excepted); R outside
 * 1..HGMM_L2_MAX_HYP; pair[r] out of range; sigma[r] not positive (NaN included); max_iter < 1; gtol negative or NaN; the
 * records of one call above 1 GiB.  HGMM_ERR_STATE: no resident pairs.  A NON-FINITE OR ZERO-LENGTH START QUATERNION IS NOT
 * REFUSED: that hypothesis ends with status 3 after its first evaluation, the others are what they would have been. */
int hgmm_l2_solve(hgmm_ctx* ctx, int R, const int32_t* pair /* [R] */, const double* theta0 /* [R][7] */,
                  const double* sigma /* [R] */, int max_iter, double gtol, double* theta_out /* [R][7] */,
                  double* f_out /* [R] */, double* grad_out /* [R][7] | NULL */, int32_t* nit_out /* [R] */,
                  int32_t* nfev_out /* [R] */, int32_t* status_out /* [R] */);
int hgmm_l2_solve_each(hgmm_ctx* ctx, int R, const int32_t* pair /* [R] */, const double* theta0 /* [R][7] */,
                       const double* sigma /* [R] */, const int32_t* max_iter /* [R] */, const double* gtol /* [R] */,
                       double* theta_out /* [R][7] */, double* f_out /* [R] */, double* grad_out /* [R][7] | NULL */,
                       int32_t* nit_out /* [R] */, int32_t* nfev_out /* [R] */, int32_t* status_out /* [R] */);

/* ---- voxel-grid down-sample: centroids + counts, one cloud or B clouds per launch set -----------------------------------
 * Every pipeline of the reference voxel-down-samples its scans first -- o3.voxel_down_sample at hgmm/hgmm_gpu.py:786 and
 * 829-830, run_gmm_static.py:28, waymoutils.py:99, gmmreg.py:203-204 -- and the counts are what the weight entries above
 * (hgmm_tree_set_target_weights, hgmm_tree_set_source_weights, hgmm_flat_set_weights) are fed with.  These entries replace
 * those calls: one point per occupied voxel, the mean of the points inside it, and the number of points it stands for.
 * SEMANTICS: pointcloud_io.voxel_down_sample(P, voxel, return_counts=True) on P as float64 is the definition, and the
 * result has its bits:
 *   origin    min_i P_i - voxel / 2 per axis
 *   index     floor((P - origin) / voxel) per axis: one IEEE subtraction, one IEEE division, one floor, in float64 (no
 *             reciprocal, no fused multiply-add)
 *   order     voxels in ascending lexicographic (ix, iy, iz) order; with the extents (nx, ny, nz) of the bounding box the
 *             sort key is (ix ny + iy) nz + iz, in a batch with the cloud number above the largest cloud's key bits
 *   centroid  per axis the float64 sum of the voxel's points in ASCENDING POINT INDEX, started from +0.0 (a voxel that
 *             holds only -0.0 comes out as +0.0), divided once by the count converted to float64
 * float32 rows (_f32) are widened to float64 on the device, exactly: the result is the _f64 entry's on the widened array.
 * Deterministic: min / max are exact in any order, the sort of (key, row) is stable, one thread adds a voxel's points one
 * after the other -- no floating-point atomics; two calls return the same bits.  A VOXEL WITH VERY MANY POINTS MAKES THAT
 * WALK LONG (a cloud that falls into one voxel is added up by one thread): accepted, the order of summation is not traded
 * for speed.
 * The batch entries down-sample B clouds by the SAME launches (one launch set whatever B is); every member's result is
 * bit for bit the serial entry's on it alone.  m_out [B] (serial: [1]) receives the number of voxels per cloud.
 * The calls come in pairs because M is not known beforehand: hgmm_voxel_downsample_get copies the LAST successful call's
 * result -- centroids [sum m][3] float64 and counts [sum m] int64, cloud after cloud; either may be NULL -- and returns
 * HGMM_ERR_STATE when no down-sample has succeeded on the context.
 * REFUSALS (HGMM_ERR_ARG, hgmm_last_error says why, the previous result stays in place): a voxel size that is NaN, infinite
 * or <= 0; n < 1 (a batch: any count < 1, B < 1); a non-finite coordinate (found by the bounding-box pass on the device; the
 * message names the first such row); a voxel grid of nx ny nz >= 2^63 cells; cloud bits + key bits > 64 in a batch; n, or
 * the batch's total, >= 2^31.
 * A call works in buffers of its own on the context's stream: the resident cloud, its weights, a forest, a target and a tree
 * are what they were.  The profiler times the whole launch set as one entry, HGMM_K_VOXEL.                                  */
int hgmm_voxel_downsample_f64(hgmm_ctx* ctx, const double* xyz /* host [n,3] */, int64_t n, double voxel, int64_t* m_out);
int hgmm_voxel_downsample_f32(hgmm_ctx* ctx, const float* xyz /* host [n,3] */, int64_t n, double voxel, int64_t* m_out);
int hgmm_voxel_downsample_batch_f64(hgmm_ctx* ctx, int B, const double* const* xyz, const int64_t* counts, double voxel,
                                    int64_t* m_out /* [B] */);
int hgmm_voxel_downsample_batch_f32(hgmm_ctx* ctx, int B, const float* const* xyz, const int64_t* counts, double voxel,
                                    int64_t* m_out /* [B] */);
int hgmm_voxel_downsample_get(hgmm_ctx* ctx, double* centroids_out /* [sum m,3] */, int64_t* counts_out /* [sum m] */);

/* ---- the voxel result handed to its consumers on the device: no download, no second upload --------------------------------
 * The last successful down-sample of a context is its VOXEL RESULT: B member clouds, member k with m[k] voxels that stand
 * for n[k] raw points.  It stays resident until the next successful down-sample; every successful down-sample increments
 * the context's serial number, by which a caller can tell whether a member it remembers is still the one resident.
 * hgmm_voxel_result_info describes it (any pointer may be NULL; m and n are [B]); HGMM_ERR_STATE without one, like _get.
 *
 * The four hand-overs copy members to where the existing setters put host arrays.  Each is DEFINED by a sequence of
 * existing entries and leaves the context in the state of that sequence, bit for bit -- every later result (tree build,
 * flat statistics and fit, float32 download, registration E-step, registration, score) has that sequence's bits -- without
 * running it: ONE launch per call whatever B is, no host pass over the points or the weights.  With (cent, cnt) =
 * hgmm_voxel_downsample_get's arrays, cent_k / cnt_k the rows of member k:
 *   hgmm_voxel_to_points(k, weights)          hgmm_set_points_f64(cent_k, m[k]);
 *                                             weights & HGMM_VOXEL_W_TREE: hgmm_tree_set_source_weights((double)cnt_k, m[k]);
 *                                             weights & HGMM_VOXEL_W_FLAT: hgmm_flat_set_weights((float)cnt_k, m[k])
 *   hgmm_voxel_to_target(k, weighted)         hgmm_tree_set_target(cent_k, m[k]);
 *                                             weighted: hgmm_tree_set_target_weights((double)cnt_k, m[k])
 *   hgmm_voxel_to_points_batch(B, members, weighted)
 *                                             hgmm_set_points_batch_f64 of the clouds cent_members[b];
 *                                             weighted: hgmm_tree_set_source_weights_batch of (double)cnt_members[b]
 *   hgmm_voxel_to_targets_batch(B, members, weighted)
 *                                             hgmm_tree_set_targets_batch of the clouds cent_members[b];
 *                                             weighted: hgmm_tree_set_target_weights_batch of (double)cnt_members[b]
 * That state includes the zero padding of the float64 planes and of the weights, the float32 rows (float)centroid (the forest
 * cloud has none), everything a new resident cloud / new target resets, and the weight sums: the tree's and the targets' are
 * (double)n[k] -- counts are integers, their sum is the member's raw point count in any order -- and the flat fit's is the
 * float64 sum of the float32 values (float)cnt (n[k] again unless a count reaches 2^24; then it is summed on the device, as
 * integers).  The targets' extent bound is sqrt(max_i ((x x + y y) + z z)) with separately rounded products and sums, the
 * maximum taken by integer atomics on the bits: hgmm_tree_set_target's and hgmm_tree_set_targets_batch's number.
 * The result is COPIED, not moved: hgmm_voxel_downsample_get returns what it returned, and a member may be handed over any
 * number of times, to several slots of one batch too (members = {3, 0, 0, 2} is legal).
 * The source hand-overs do not wait for the device; the target hand-overs wait once, for the extent bounds.
 * REFUSALS, each checked before anything resident is touched (the resident cloud, target, weights, forest and the voxel
 * result stay what they were; hgmm_last_error says why): HGMM_ERR_STATE without a voxel result; HGMM_ERR_ARG for a member
 * outside [0, B_result), B < 1 (targets: B > 4096), NULL members, bits of `weights` other than the two below, more than
 * 0x7fffffff - 1024 target points in all.  A runtime failure part-way leaves nothing bound / no target.                       */
#define HGMM_VOXEL_W_TREE 1   /* the counts as source weights of the tree build (hgmm_tree_set_source_weights) */
#define HGMM_VOXEL_W_FLAT 2   /* the counts as weights of the flat fit (hgmm_flat_set_weights) */
int hgmm_voxel_result_info(hgmm_ctx* ctx, int* B_out, int64_t* m_out /* [B] */, int64_t* n_out /* [B] */, uint64_t* serial_out);
int hgmm_voxel_to_points(hgmm_ctx* ctx, int member, int weights /* HGMM_VOXEL_W_* bits */);
int hgmm_voxel_to_target(hgmm_ctx* ctx, int member, int weighted);
int hgmm_voxel_to_points_batch(hgmm_ctx* ctx, int B, const int32_t* members /* [B] */, int weighted);
int hgmm_voxel_to_targets_batch(hgmm_ctx* ctx, int B, const int32_t* members /* [B] */, int weighted);

/* Rows of the resident cloud's float64 view on the host: out[j] = row rows[j] (a forest cloud: rows of the concatenated
 * cloud) -- how a caller reads back what is resident, whichever way it got there.  HGMM_ERR_STATE without a float64 view;
 * HGMM_ERR_ARG for k < 0, NULL pointers or a row outside the cloud (the message names its position and value).
 * hgmm_tree_build_rows / hgmm_tree_build_batch_rows are hgmm_tree_build / hgmm_tree_build_batch with init_mu[j] = the float64
 * row init_rows[j] of the resident cloud (batch: init_rows [B][T], row numbers WITHIN each cloud), gathered on the device into
 * the place init_mu is uploaded to: bit for bit the same build, no host copy of the cloud needed.  They work on any
 * resident cloud, not only one that came from a voxel result; a row outside its cloud is HGMM_ERR_ARG and nothing is touched. */
int hgmm_points_rows_f64(hgmm_ctx* ctx, const int64_t* rows /* [k] */, int64_t k, double* out /* [k,3] */);
int hgmm_tree_build_rows(hgmm_ctx* ctx, int L, double ls, double ld, const int64_t* init_rows /* [T] */,
                         double sig2, int max_iters_per_level,
                         double* pi_out, double* mu_out, double* cov_out, int32_t* leaf_idx_out,
                         int32_t* iters_per_level_out, double* q_trace_out, int q_capacity,
                         int* q_len_out);
int hgmm_tree_build_batch_rows(hgmm_ctx* ctx, int B, const int64_t* counts, int L, double ls, double ld,
                               const int64_t* init_rows /* [B][T] */, double sig2, int max_iters_per_level,
                               double* pi_out, double* mu_out, double* cov_out, int32_t* iters_out,
                               double* q_trace_out, int q_capacity, int32_t* q_len_out);

/* ---- multi-GPU: one context per rank, RCCL over xGMI --------------------------------
 * New functionality (the reference is single-GPU).  With a communicator attached,
 * hgmm_flat_train*, hgmm_flat_stats and hgmm_tree_build all-reduce their per-cluster
 * sufficient statistics (and the point count) across ranks before every M-step.        */
int hgmm_comm_unique_id(void* id128_out);                       /* 128 bytes */
int hgmm_comm_init_rank(hgmm_ctx* ctx, int nranks, int rank, const void* id128);
int hgmm_comm_destroy(hgmm_ctx* ctx);
/* Test backend behind the same all-reduce call sites: the ranks are processes of ONE machine that
 * meet in the POSIX shared-memory object `name` (they may share a GPU, which RCCL does not allow), every
 * all-reduce goes device -> host -> summed in rank order -> device.  For exercising the N > 1 path on a
 * single-GPU box; not a performance path.                                                          */
/* `name` (here and in hgmm_comm_init_ipc) must be unique to the JOB -- rank 0 creates the object, the others join the
 * object of that name: give it a token the ranks agreed on beforehand (bench.py: a random token of rank 0, handed out
 * over the TCP star; tests: the pid of the launching process).  Joiners refuse an object whose creator is gone (pid
 * in the same pid namespace) or that is older than 10 minutes in a foreign one, but a crashed earlier job's object
 * under the SAME name whose creator's pid has been recycled cannot be told apart from the live one.                  */
int hgmm_comm_init_host(hgmm_ctx* ctx, int nranks, int rank, const char* name);
/* One-shot exchange backend behind the same all-reduce call sites (the message is 57 KB, latency is
 * everything): the ranks are processes of ONE node, one GPU each.  Every rank owns an exchange buffer in uncached
 * device memory, exported with hipIpcGetMemHandle and mapped by all peers (the handles meet in the POSIX shared-memory
 * object `name`).  An all-reduce is ONE kernel per rank: each workgroup writes its 4 KB piece of the rank's slice
 * into the slot this rank owns in EVERY peer's buffer (plain stores over xGMI), releases a sequence flag per piece and
 * peer, waits for the same piece of every peer in its own buffer and adds the slices up in RANK ORDER -- so all ranks
 * hold bitwise the same sum, with no ring, no tree and no proxy thread.  Slots are double-buffered by the parity of
 * the collective's sequence number (stream order makes that enough).  A peer that never arrives raises an error word
 * after ~20 s instead of hanging the GPU: the next synchronising call fails.  Two ranks may share one GPU (tests). */
int hgmm_comm_init_ipc(hgmm_ctx* ctx, int nranks, int rank, const char* name);
int hgmm_comm_allreduce_f64(hgmm_ctx* ctx, double* host_inout, int n, int op /*0 sum,1 max*/);

/* ---- profiling (hipEvent pairs around the hot kernels, on the context's stream) ---- */
int hgmm_profile_enable(hgmm_ctx* ctx, int on);
int hgmm_profile_reset(hgmm_ctx* ctx);
int hgmm_profile_get(hgmm_ctx* ctx, int kernel_id, double* total_ms_out, int64_t* launches_out);
/* Phase clocks of the one-pass full-covariance kernels (a profiling aid like the event profiler above; no reference
 * counterpart): enable = 1 arms them -- the following hgmm_fullcov_estep / hgmm_fullcov_fit launches record, per wave of
 * workgroup 7, the clock64() cycles spent in phase A (pdfs -> tile), phase B (row sums, arg-max), phase C (statistics on
 * the matrix cores) and waiting at the phases' barriers; enable = 0 disarms them and copies the last launch's
 * clocks_out[8 waves][4] (A, B, C, wait).  profiles/r06/fullcov_phase_clocks.log is made with it.                      */
int hgmm_fullcov_phase_clocks(hgmm_ctx* ctx, int enable, int64_t* clocks_out);
/* Streams `value` into n float32 of a device buffer with 16-byte (optionally non-temporal)
 * stores: the pure-write HBM ceiling the E-step's log_resp stream is compared with. */
int hgmm_util_fill_f32(hgmm_ctx* ctx, float* dev, int64_t n, float value, int nontemporal);

#ifdef __cplusplus
}
#endif
#endif /* HGMM_H */
