// Internal context of libhgmm_hip.so (not part of the C ABI).
#pragma once
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <string>
#include <cstring>
#include <utility>
#include <vector>

#include "../../include/hgmm.h"
#include "flat_pace.h"
#include "point_weights.h"

namespace hgmm {

constexpr float FLAT_EPS = 1e-8f;     // gmm_waymo gmm_impl.py:15 / gmmreg_gpu gmm_impl.py:16
constexpr int FLAT_NSTAT = 7;         // s0, a[3], b[3]
constexpr int FLAT_CM_STRIDE = 8;     // floats per component of a component-major partial: the 7 statistics + one pad = 32 bytes
constexpr int FLAT_MAX_J = 1024;      // single-pass kernels (all parameters of a lane in registers)
constexpr int FLAT_MAX_J_CHUNKED = 16384;  // chunked path (832-component chunks)
constexpr int FLAT_MAX_BLOCKS = 2048; // persistent grid upper bound (partials buffer)

// A growable device buffer owned by the context.
struct DevBuf {
    void* p = nullptr;
    size_t cap = 0;
    template <class T> T* as() const { return reinterpret_cast<T*>(p); }
};

// Per-point weights of a resident cloud or target -- or of the forest's B clouds / targets, back to back -- : the buffer,
// whether it is in force, and the weights' sums (on the host in index order).  Consumers read ptr() and total() and nothing
// else; the writers are upload_weights (tree_host.h), hgmm_flat_set_weights, the hand-overs of voxel_handover.hip and
// whatever replaces the cloud or the target (drop).
template <class T> struct WeightSet {
    DevBuf buf;                       // T [n] or [n_pad], parallel to the points (a forest's unweighted member: 1.0 per point)
    bool on = false;
    std::vector<double> sums;         // (on) one per member, a serial set: one; an unweighted member: its count
    const T* ptr() const { return on ? buf.as<T>() : nullptr; }                           // NULL: no weights in force
    double total(int64_t n, int b = 0) const { return on ? sums[b] : (double)n; }          // what pi = m0 / W divides by
    void drop() { on = false; }                                                            // (the buffer stays allocated)
    void publish(std::vector<double> s) { sums = std::move(s); on = true; }
};
using MemberWeights = WeightSet<double>;     // (the forest's: B members)

struct EventPair { hipEvent_t a, b; int kernel; };

enum FlatKernel { FLAT_K_NONE, FLAT_K_ESTEP /* materialising E-step */, FLAT_K_MSTEP /* M-step from resp */, FLAT_K_FUSED /* fused EM */ };

struct FlatState {
    int cov_type = 0, variant = 0, J = 0, Jpad = 0;
    float tol = 0.f;
    int lls_cap = 0;
    int launched = 0;                 // EM iterations enqueued since train_begin
    bool active = false;
    bool chunked = false;             // J > FLAT_MAX_J: 832-component chunks
    int nchunks = 1;
    FlatKernel last_kernel = FLAT_K_NONE;   // what this context enqueued last (flat_kernels.hip: note_launch)
    bool last_estep_rows4 = false;    // the last materialising E-step ran the four-rows-in-flight kernel (its waves' row order:
                                      // flat_weighted_lpn_partials_kernel re-plays it)
    bool idle_since_launch = true;    // the host has drained the stream since the last of these launches (ctx_stream_sync)
};

// One member of a batched flat fit (hgmm_flat_train_batch, flat_kernels.hip): what the serial loop keeps in the context --
// the cloud, its grid, the parameter block, the packed table, the partials, the statistics, the trace and the control words --
// as one row of a table on the device.  The batched kernels find their member by workgroup (the fused launch: a table of
// (member, local block) per workgroup; the others: blockIdx.y) and read everything else from here.
struct FlatBatchMember {
    const float* X;                   // float [n,3]: the handle's x_aos
    int64_t n;
    int block0, nblocks;              // the member's workgroups in the fused launch: [block0, block0 + nblocks)
    float* params;                    // float [10][Jpad]  cov | mu | w | inv, the layout of f_block
    float* pack;                      // float [PK_ROWS][Jpad]
    float* partials;                  // float [nblocks][7][Jpad]
    double* lpn_partials;             // double [nblocks]
    double* stats;                    // double [7 * Jpad + 2]
    float* lls;                       // float [lls_cap]
    int* ctl;                         // int [16], the layout of f_ctl: stop (even), n_iter, converged, stop (odd); float prev at [8]
    const float* SW;                  // float [n] per-point weights of this SLOT (a handle owns none), or NULL: unweighted
    double wn;                        // what flat_w.total(n) is to the serial launchers: the slot's weight sum S_b, or (double)n
};
// One slot of a batched fit as its entries hand it to the launch set (flat_batch_run, flat_kernels.hip): device pointers only.
struct FlatBatchSlot {
    const float* X;                   // float [n,3]
    int64_t n;
    const float* SW;                  // float [n] on the device, or NULL
    double wn;                        // S_b, or (double)n
};
constexpr int FLAT_BATCH_MAX = 4096;                              // members per call
constexpr unsigned long long FLAT_BATCH_MAX_PARTIALS = 8ull << 30;   // bytes of all members' partial buffers together
constexpr int FLAT_BATCH_CTL_WORDS = 16;
constexpr int KM_BATCH_MAX = 4096;                                // members per hgmm_kmeans_fit_batch
constexpr unsigned long long KM_BATCH_MAX_PARTIALS = 8ull << 30;  // bytes of all members' per-cluster partial sums together

// The store pacer's measurement ring (its rate controller: flat_pace.h): the last few paced E-step launches are bracketed
// by event pairs that are looked at -- never waited for -- when the next one is launched (flat_kernels.hip, pace_poll).
struct PaceRing {
    static constexpr int RING = 4;
    hipEvent_t ev[RING][2] = {};
    double tgt_at[RING] = {}, bytes_at[RING] = {};
    unsigned head = 0, tail = 0;
    bool have_events = false;
    // what a launch is judged by: wall-clock stamps the kernel's workgroups leave in pinned host memory -- [RING][2][STAMP_WG]:
    // start and end per workgroup -- so that nothing the host, the queue or a profiler puts around the launch counts as
    // the memory system's answer (the event pair only says WHEN the stamps are complete; it is the fall-back measure if
    // the buffer could not be had)
    static constexpr int STAMP_WG = 1024;
    unsigned long long* stamps = nullptr;       // host address
    unsigned long long* stamps_dev = nullptr;   // the same memory as the device sees it
    int grid_at[RING] = {};
};

// Per-context options.  Each starts from the environment variable HGMM_<NAME IN CAPITALS>, read ONCE -- in hgmm_create, the
// only getenv of the library -- and can be set per context afterwards (hgmm_config_set / Context.config_set).  Every option
// selects a path that is also reached by data (another J, another cloud size, a failed factorisation) or is a documented
// operating mode; each is listed in INTEGRATION.md and run against its golden by tests/test_config_gpu.py.  Round 5 had
// 46 environment switches read at call time; the tuning knobs among them are fixed at their measured values now and
// the rejected variants are gone with their code.
enum ConfigKey {
    CFG_ESTEP_TARGET_GBS,      // store pacing of the materialising E-step: -1 controlled (default), 0 un-paced, > 0 fixed rate in GB/s
    CFG_PACE_START,            // rate the controller starts from, GB/s
    CFG_PACE_FORGET,           // clean launches after which a ceiling learnt under congestion is forgotten
    CFG_PREDICT_SINGLE_ROW,    // predict() on the general single-row kernel (the path of layouts the 4-row kernel is not built for)
    CFG_TREE_NO_CHOL,          // symmetric instead of triangular form of the pdfs' exponent (the fallback of a failed factorisation)
    CFG_TREE_REL,              // relative reach test of the level log-likelihood (large clouds; gives up the bitwise q for ~3 %)
    CFG_TREE_AHEAD,            // iterations the host keeps enqueued ahead of the device in hgmm_tree_build (0: batches + control-word copy)
    CFG_TREE_TICKETS,          // stop rule in the log-likelihood's last workgroup instead of the next launch
    CFG_TREE_OVERLAP,          // small clouds: iteration e + 1's E-step rides in iteration e's log-likelihood launch
    CFG_FULLCOV_TWO_PASS,      // two-kernel form of the full-covariance iteration (the path of J > 1024)
    CFG_KMPP_TWO_LAUNCHES,     // k-means++ step and tail as two launches (the path of > 16.7 M points)
    CFG_KMEANS_ACC_REGS,       // Lloyd sums in registers instead of LDS tables (the path of k > 1024)
    CFG_IPC_TIMEOUT_S,         // seconds the peer exchange waits for a peer's flag before it reports the collective as failed
    CFG_REG_DEVICE_SOLVE,      // registration loop without the host: 6 x 6 solve, twist, stop rule and the next encoding on the device
    CFG_COUNT
};
struct ConfigSpec { const char* name; int dflt, lo, hi; };
extern const ConfigSpec CONFIG_SPECS[CFG_COUNT];

// The context's pinned, coherent hand-over block (tree_host.h: hand_over): what a running kernel stores there at system
// scope the polling host sees at once.  For B pairs / clouds:
//   [0, 32)  two control-word slots (TreeCtl) of the batch scheme's asynchronous copies
//   [64 ..)  B progress words  (stopped << 32 | iterations)  of the builds and of the registration loop on the device
//   then     B sequence words + (256-aligned) B x 28 numbers: the registration's normal equations on their way to the host
struct TreeCtl;                            // tree_device.h
template <class T> struct HostDev { T* host; T* dev; };   // one location, as the host and as the device address it
struct HandOver {
    char* host = nullptr;
    char* dev = nullptr;
    size_t cap = 0;
    int B = 0;
    unsigned long long seq = 0;            // sequence number of the last hand-over through the block
    static size_t seq_off(int B) { return 64 + (((size_t)B * 8 + 63) & ~(size_t)63); }
    static size_t out_off(int B) { return (seq_off(B) + (size_t)B * 8 + 255) & ~(size_t)255; }
    static size_t bytes(int B) { return out_off(B) + (size_t)B * 28 * sizeof(double); }
    template <class T> HostDev<T> at(size_t off) const { return {reinterpret_cast<T*>(host + off), reinterpret_cast<T*>(dev + off)}; }
    TreeCtl* ctl_slot(int s) const { return reinterpret_cast<TreeCtl*>(host + 16 * (size_t)s); }   // (host side only: copy targets)
    HostDev<unsigned long long> progress(int b) const { return at<unsigned long long>(64 + (size_t)b * 8); }
    HostDev<unsigned long long> sequence(int b) const { return at<unsigned long long>(seq_off(B) + (size_t)b * 8); }
    HostDev<double> out28(int b) const { return at<double>(out_off(B) + (size_t)b * 28 * sizeof(double)); }
};

struct HostComm;                           // hgmm_api.hip
struct IpcComm;                            // hgmm_api.hip: one-shot peer-to-peer exchange over mapped peer memory

struct TreeState {
    int L = 0;
    int T = 0;
    bool nodes_ready = false;
    bool pdf_f32 = false;             // hgmm_tree_set_precision: the level log-likelihood's pdfs in float32 (large clouds)
    double reg_gate = INFINITY;       // hgmm_tree_set_reg_gate: squared Mahalanobis gate of the registration E-step (+inf: off)
    double mu_rmax = -1.0;            // largest |mu_j| of the node table (< 0: not known on the host yet)
    bool momq_clean = false;          // every word of t_momq is zero (tree_host.h: MomqScope)
    bool multi_momq_clean = false;    // ... of tm_momq, the sums of hgmm_tree_register_multi's K hypotheses
    unsigned long long surplus_iterations = 0;   // (communicator) level-iterations enqueued behind a level's stop, all builds
};

// A FOREST: B independent clouds whose trees are built / whose targets are registered by the same launches
// (tree_batch.hip: hgmm_tree_build_batch, hgmm_tree_set_targets_batch, hgmm_tree_register_batch)
struct ForestState {
    int B = 0, L = 0, T = 0;
    bool nodes_ready = false;
    std::vector<int64_t> counts;          // points per cloud (they lie back to back in the context's resident cloud)
    std::vector<double> mu_rmax;          // largest |mu_j| per tree (extent bound of the fixed-point moments)
    int tg_B = 0;
    std::vector<int64_t> tg_counts, tg_first;
    std::vector<double> tg_rmax;          // largest |x| per target
    int64_t tg_pad = 0;
    bool momq_clean = false;              // every word of fr_momq is zero (tree_host.h: MomqScope)
    bool multi_momq_clean = false;        // ... of fm_momq, the sums of hgmm_tree_register_batch_multi's R hypotheses
    MemberWeights tg_w;                   // hgmm_tree_set_target_weights_batch: [tg_pad] parallel to fr_tg; new targets drop them
    std::vector<int64_t> src_counts;      // hgmm_set_points_batch_*: the resident cloud's members (empty: not a batch cloud)
    MemberWeights src_w;                  // hgmm_tree_set_source_weights_batch: [n_pad] parallel to x_soa64; a new cloud drops them
};

// The resident pairs of the fused L2 GMMReg cost (gmmreg_kernels.hip).  One pair on the device: where its centres lie in
// the concatenated arrays.  Its launch shape -- source blocks x target splits -- follows from (Js, Jt) alone.
struct L2Pair { int s_first, Js, t_first, Jt; };
struct L2Set {
    int B = 0;                        // 0: nothing resident
    int wg_max = 0;                   // the largest workgroup count of one hypothesis among the resident pairs (grid.x)
    std::vector<L2Pair> pairs;        // host copy of the device table (hgmm_l2_cost's checks and launch shape)
    DevBuf mix;                       // double mu_s [sum Js][3] | phi_s [sum Js] | mu_t [sum Jt][3] | phi_t [sum Jt], then L2Pair [B]
    DevBuf work;                      // per call: L2Hyp [R], then double records [R][wg_max][13]; hgmm_l2_solve: L2Hyp [R],
                                      // L2SolveState [R] (l2_device.h), then the records
    char* pin = nullptr;              // pinned, device-visible: L2Hyp [HGMM_L2_MAX_HYP] on their way in, then double
    char* pin_dev = nullptr;          // [HGMM_L2_MAX_HYP][13] the finish kernel writes (hipHostFree: hgmm_destroy)
};

}  // namespace hgmm

// A point cloud resident in HBM that outlives the calls made on it (hgmm_points_create_*): the float32 row-major copy the
// flat EM reads and the float64 structure-of-arrays copy of the HGMM / KMeans kernels.  Any number per context.
struct hgmm_points {
    hgmm_ctx* ctx = nullptr;
    int64_t n = 0, n_pad = 0;
    hgmm::DevBuf x_aos, x_soa64;
};

struct hgmm_ctx {
    int cfg[hgmm::CFG_COUNT] = {};    // hgmm::ConfigKey -> value (hgmm_create: defaults, then the environment)
    int flat_boundary = 2;            // launches between two flat EM iterations: 2 reduce + finalize, 1 flat_boundary_kernel (measured
                                      // no faster; HGMM_FLAT_BOUNDARY, read with the options in hgmm_create)
    int device = 0;
    int cus = 256;
    int wall_khz = 0;                 // rate of wall_clock64() on this device (StorePacer, flat_kernels.hip)
    hipStream_t stream = nullptr;
    std::string err;

    // ---- points -----------------------------------------------------------------
    int64_t n = 0;                    // local points
    // x_aos / x_soa64 are VIEWS of the cloud the kernels work on: the context's own one (own_points, hgmm_set_points_*) or
    // a caller-held handle (hgmm_points_bind); the memory belongs to whoever `bound` names
    hgmm::DevBuf x_aos;               // float [n,3]  (flat EM; wave-uniform scalar loads)
    hgmm::DevBuf x_soa64;             // double [3][n_pad] (HGMM; lanes across points)
    hgmm_points own_points;           // the one-cloud shortcut's storage
    hgmm_points* bound = nullptr;     // nullptr: nothing resident yet
    bool have_f32 = false, have_f64 = false;
    int64_t n_pad = 0;
    // per-point weights of the resident cloud; whatever changes the resident cloud drops them (hgmm_api.hip: bind_points)
    hgmm::WeightSet<double> src;      // [n_pad], parallel to x_soa64 (level-0 order): hgmm_tree_set_source_weights, read by the
                                      // tree build, the weighted full-covariance fit and the weighted KMeans entries
    hgmm::WeightSet<float> flat_w;    // [n], parallel to the rows of x_aos: hgmm_flat_set_weights, the flat (diag / spherical) EM
    hgmm::DevBuf f_lpn_rows;          // float [n] the rows' log-normalisers when a weighted E-step's caller brings no dev_lpn

    // ---- flat EM ----------------------------------------------------------------
    hgmm::FlatState flat;
    hgmm::PaceRate pace;                      // the store pacer's rate (flat_pace.h) ...
    hgmm::PaceRing pace_ring;                 // ... and what it is measured with
    hgmm::DevBuf f_block;                     // float [10][Jpad]: the allocation behind the four arrays below
    hgmm::DevBuf f_mu, f_cov, f_w, f_inv;     // float model parameters (reference layout): NON-OWNING slices of f_block
    hgmm::DevBuf f_pack;                      // float [PK_ROWS = 8][Jpad] packed E-step params (flat_kernels.hip: mu, g, c, w)
    hgmm::DevBuf f_partials;                  // float [blocks][7][Jpad], or [blocks][Jpad][8] from the train loop's fused kernel
    hgmm::DevBuf f_lpn_partials;              // double [blocks]
    hgmm::DevBuf f_stats;                     // double [7*Jpad + 2]  (+ sum lpn, + n)
    hgmm::DevBuf f_lls;                       // float [cap]
    hgmm::DevBuf f_ctl;                       // int  [4]: done, n_iter, converged, pad ; float prev
    hgmm::DevBuf f_hint;                      // float [3][Jpad] centre hint for m-step
    hgmm::DevBuf f_cm, f_cs, f_ca, f_lpn2;    // chunked path: per-chunk (max, sum, arg-max) [C][n], lpn2 [n]
    // batched fit (hgmm_flat_train_batch): buffers of its own, nothing above is touched
    hgmm::DevBuf fb_tab;                      // FlatBatchMember [B], then int2 (member, local block) per workgroup of the fused launch
    hgmm::DevBuf fb_params;                   // float [B][10][Jpad]
    hgmm::DevBuf fb_pack;                     // float [B][PK_ROWS][Jpad]
    hgmm::DevBuf fb_partials;                 // float [sum of the members' grids][7][Jpad]
    hgmm::DevBuf fb_lpn_partials;             // double [sum of the members' grids]
    hgmm::DevBuf fb_stats;                    // double [B][7 * Jpad + 2]
    hgmm::DevBuf fb_lls;                      // float [B][cap]
    hgmm::DevBuf fb_ctl;                      // int [B][16]
    hgmm::DevBuf fb_sw;                       // float: the weights of the weighted slots of one call, slot after slot
    hgmm::DevBuf fb_x;                        // float [sum m][3]: the rows of hgmm_flat_train_batch_voxels, slot after slot
    hgmm::DevBuf scratch;
    double* h_scalars = nullptr;              // pinned, device-visible scalars (hgmm_host_scalars)
    int h_scalars_n = 0;
    hipEvent_t ev_slots[64] = {};             // hgmm_event_record / hgmm_event_wait
    // pinned host ring for small parameter uploads / result downloads (hgmm_api.hip: stage_*): a pageable
    // hipMemcpyAsync is staged by the runtime behind the stream's pending work, a pinned one is a plain DMA packet
    void* h_stage = nullptr;
    size_t h_stage_cap = 0, h_stage_off = 0;

    // ---- tree -------------------------------------------------------------------
    hgmm::TreeState tree;
    hgmm::DevBuf t_pi, t_mu, t_cov;           // double node tables [T], [T,3], [T,9]
    hgmm::DevBuf t_prep;                      // double [T][12] : inv(6) coef logc pi mu(3) -> see tree_kernels
    hgmm::DevBuf t_cplx;                      // double [T]
    hgmm::HandOver hand;                      // pinned hand-over block of the tree / forest drivers
    hipEvent_t tree_ev[2] = {nullptr, nullptr};   // the batch scheme's events, one per control-word slot (tree_host.h: run_batches)
    hgmm::DevBuf exp_tab2;                    // double [2048] 2^(j/2048) for the throughput kernels' exp (tree_kernels.hip)
    hgmm::DevBuf t_tickets;                   // uint: two-level arrival counters of the last-workgroup reductions, 4 KB apart
    hgmm::DevBuf t_flags;                     // int [4] tree flags + uint64 executed-pair counter (tree_kernels.hip)
    hgmm::DevBuf t_mom;                       // double [T][10]
    hgmm::DevBuf t_momq;                      // uint64 [T][10]  registration E-step: fixed-point moments
    hgmm::DevBuf t_parent, t_current;         // int32 [n]
    hgmm::DevBuf t_perm;                      // int32 [n]  points sorted by parent
    hgmm::DevBuf t_xs3;                       // double [3][n_pad] third coordinate buffer (L > 2)
    hgmm::DevBuf t_w2, t_w3;                  // double [n_pad] the source weights' ping-pong beside t_parent / t_xs3 (weighted builds only)
    hgmm::DevBuf t_seg;                       // int32 segment tables
    hgmm::DevBuf t_chunks;                    // int32 chunk descriptors
    hgmm::DevBuf t_partials;                  // double per-chunk partial moments
    hgmm::DevBuf t_q;                         // double per-block q partials + result
    hgmm::DevBuf t_llp;                       // double [node chunks][n_pad] log-likelihood partial sums
    hgmm::DevBuf t_qtrace;                    // double [max iterations per level] q of the running level
    hgmm::DevBuf tgt_soa64;                   // double [3][m_pad] registration target
    int64_t tgt_n = 0, tgt_pad = 0;
    double tgt_rmax = 0.0;                    // largest |x| of the target (extent bound of the fixed-point moments)
    hgmm::WeightSet<double> tgt_w;            // [m_pad] per-point weights of the target (hgmm_tree_set_target_weights); a new
                                              // target drops them

    // ---- forest (batched trees: tree_batch.hip) ------------------------------------
    hgmm::ForestState forest;
    hgmm::DevBuf fr_pi, fr_mu, fr_cov, fr_prep, fr_mom;   // node tables [B T], as t_pi ... t_mom
    hgmm::DevBuf fr_clouds;                   // ForestCloud [B] + int flags [B]
    hgmm::DevBuf fr_q;                        // double: the clouds' shares of q
    hgmm::DevBuf fr_trace;                    // double [B][L][trace_cap]
    hgmm::DevBuf fr_tg;                       // double [3][tg_pad] the targets, back to back
    hgmm::DevBuf fr_momq;                     // uint64 [B T][4] registration sums
    hgmm::DevBuf ff_clocks;                   // int64 [8][4] phase clocks of the one-pass full-covariance kernels (armed: ff_clocks_on)
    bool ff_clocks_on = false;
    hgmm::DevBuf ff_origin;                   // double [256][3] partial coordinate sums: origin of the float32 full-covariance statistics
    hgmm::DevBuf fr_reg;                      // per-pair registration table + the 28 numbers per pair + per-pair r2max words
    // multi-start (hgmm_tree_register_multi / _score_multi): K start poses on the SERIAL tree and target, buffers of their own
    hgmm::DevBuf tm_momq;                     // uint64 [K][T][4] registration sums, one slice per hypothesis
    hgmm::DevBuf tm_reg;                      // per-hypothesis registration table + the 28 numbers per hypothesis
    // batched multi-start (hgmm_tree_register_batch_multi / _score_batch_multi): R hypotheses over the forest, likewise
    hgmm::DevBuf fm_momq;                     // uint64 [R][T][4]
    hgmm::DevBuf fm_reg;                      // per-hypothesis registration table + the 28 numbers per hypothesis

    // ---- KMeans initialiser (float64, on x_soa64) -----------------------------------
    hgmm::DevBuf km_closest;                  // double [n_pad] k-means++: min squared distance so far
    hgmm::DevBuf km_block;                    // double block sums / prefix / candidate partials
    hgmm::DevBuf km_centres;                  // double [k][3] + padded [k][4]
    hgmm::DevBuf km_ids;                      // int64 [k] chosen point ids + candidates
    hgmm::DevBuf km_rand;                     // double [(k-1) * trials] host-drawn uniforms
    hgmm::DevBuf km_labels;                   // int32 [n_pad]
    hgmm::DevBuf km_mind2;                    // double [n_pad]
    hgmm::DevBuf km_partial;                  // double [blocks][k_alloc][4]
    hgmm::DevBuf km_out;                      // double [4k + 2] sums, inertia, changed (+ scratch)
    int64_t km_labels_n = -1;
    // batched initialiser (hgmm_kmeans_fit_batch, kmeans_batch.h): buffers of its own, nothing above is touched
    hgmm::DevBuf kb_tab;                      // KmBatchMember [B], then (member, local index) per workgroup of the four sized launches
    hgmm::DevBuf kb_x;                        // double: the members' copies of their clouds, [3][n_pad_b] each, n_pad_b a multiple of 4096
    hgmm::DevBuf kb_points;                   // double closest | double mind2 | int32 labels, [sum n_pad_b] each; int32 [n_pad] packed labels
    hgmm::DevBuf kb_blocks;                   // double: the members' block / group / candidate tables, then their inertia partials
    hgmm::DevBuf kb_partial;                  // double: the members' [nb_acc_b][k_alloc][4]
    hgmm::DevBuf kb_small;                    // per member: seeds, centres, padded centres, candidates, sums, uniforms, ids, control words

    // batched full-covariance fit (hgmm_fullcov_fit_batch, fullcov_batch.h): buffers of its own, nothing above is touched
    hgmm::DevBuf fc_tab;                      // FcBatchMember [B], then (member, local block) per workgroup of the fused launch
    hgmm::DevBuf fc_tables;                   // double [B][J16] x (pi 1 | mu 3 | cov 9 | prep PREP_N | mom NMOM)
    hgmm::DevBuf fc_partials;                 // double [sum of the members' grids][J16][NMOM]
    hgmm::DevBuf fc_small;                    // double shares of q [sum of the grids] | q [B] | traces [B][cap]; TreeCtl [B]; int flags [B]
    hgmm::DevBuf fc_labels;                   // int32 [2][n_pad] the two arg-max buffers on the forest cloud's rows, then [n_pad] the result

    // ---- L2 GMMReg Gauss transform ---------------------------------------------------
    hgmm::DevBuf gt_buf;                      // double: centres, points, weights, per-split partial sums
    // resident mixtures of the fused rigid cost (hgmm_l2_set_pairs / hgmm_l2_cost, gmmreg_kernels.hip): buffers of their own.
    // LIFETIME: l2 is replaced as a whole by a successful hgmm_l2_set_pairs (a refused one leaves it alone), read by
    // hgmm_l2_cost and freed by hgmm_destroy; nothing else of the context reads or writes it
    hgmm::L2Set l2;

    // ---- voxel-grid down-sample (voxel_kernels.hip): buffers of its own, nothing above is touched --------
    hgmm::DevBuf vx_in;                       // the clouds' rows as uploaded, back to back: float or double [total][3]
    hgmm::DevBuf vx_tab;                      // int64 first row [B + 1], VoxelBox [B], VoxelGrid [B], uint32 M + first voxel [B]
    hgmm::DevBuf vx_keys, vx_keys2;           // uint64 [total] voxel keys, unsorted / sorted
    hgmm::DevBuf vx_rows, vx_rows2;           // uint32 [total] row indices, unsorted / sorted
    hgmm::DevBuf vx_heads;                    // uint32 [total] first sorted position of every voxel (M of them in use)
    hgmm::DevBuf vx_tmp;                      // temporary storage of the sort and of the compaction
    hgmm::DevBuf vx_cent, vx_cnt;             // the last result: double [M][3] centroids, int64 [M] counts, cloud after cloud
    bool vx_have = false;                     // a down-sample has succeeded on this context
    int64_t vx_m = 0;                         // its M (all clouds)
    // the voxel result by member (hgmm_voxel_result_info, the hand-overs of voxel_handover.hip): member k has vx_mb[k] voxels,
    // rows [vx_first[k], vx_first[k] + vx_mb[k]) of vx_cent / vx_cnt, and stands for vx_nb[k] raw points
    std::vector<int64_t> vx_mb, vx_nb, vx_first;
    unsigned long long vx_serial = 0;         // successful down-samples of this context so far
    hgmm::DevBuf vx_hand;                     // hand-over tables: int64 destination first rows [B + 1], source first rows [B]; 3 words

    // ---- multi-GPU --------------------------------------------------------------
    ncclComm_t comm = nullptr;                // RCCL over xGMI (one GPU per rank)
    hgmm::HostComm* hcomm = nullptr;          // host shared-memory communicator (tests: ranks may share a GPU)
    hgmm::IpcComm* icomm = nullptr;           // one-shot exchange: every rank writes its slice into every peer's buffer (xGMI)
    volatile unsigned* icomm_err = nullptr;   // pinned host word an exchange kernel raises when a peer never arrived
    int nranks = 1, rank = 0;
    hgmm::DevBuf comm_buf;
    bool comm_on() const { return comm != nullptr || hcomm != nullptr || icomm != nullptr; }
    unsigned long long collectives = 0;       // all-reduces this context has enqueued on its communicator (hgmm_comm_stats)

    // ---- profiling --------------------------------------------------------------
    bool profiling = false;
    std::vector<hgmm::EventPair> events;
    size_t events_used = 0;
    double prof_ms[HGMM_K_COUNT] = {0};
    int64_t prof_n[HGMM_K_COUNT] = {0};
};

namespace hgmm {
// a region of the context's pinned staging ring (hgmm_api.hip); reused only after a stream synchronisation
constexpr size_t STAGE_RING_BYTES = 4u << 20;
int stage_reserve(hgmm_ctx* c, size_t bytes, void** out);
// `bytes` of host memory on their way to `dev`: copied into a region of the ring, one DMA packet behind the stream's work
int stage_h2d(hgmm_ctx* c, void* dev, const void* host, size_t bytes);
// a small table on its way to the device: through the ring while it fits (<= 256 KB), else copied from `host` directly
int upload_table(hgmm_ctx* c, void* dev, const void* host, size_t bytes);

// B clouds back to back with a table of first rows: the cloud row i belongs to, the largest b with first[b] <= i
__device__ inline int find_cloud(const int64_t* __restrict__ first, int B, int64_t i) {
    int lo = 0, hi = B - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (first[mid] <= i) lo = mid; else hi = mid - 1;
    }
    return lo;
}

}  // namespace hgmm

// Every wait for the context's stream goes through here: the E-step's grid policy (flat_kernels.hip, estep_rows_grid)
// wants to know whether the chip has been idle since the last bandwidth-bound launch.
inline hipError_t ctx_stream_sync(hgmm_ctx* c) {
    const hipError_t e = hipStreamSynchronize(c->stream);
    c->flat.idle_since_launch = true;
    // an exchange kernel that waited in vain for a peer's slice has produced garbage: every result read after this
    // synchronisation would be wrong, so the wait itself fails (hipErrorLaunchTimeOut -> HGMM_ERR_HIP at the call site)
    if (e == hipSuccess && c->icomm_err && *c->icomm_err) return hipErrorLaunchTimeOut;
    return e;
}


namespace hgmm {

// Results of an API call on their way to the caller's (pageable) arrays: every add() enqueues ONE asynchronous DMA into
// the pinned ring behind the kernels already on the stream (arrays above `limit` bytes, or whatever no longer fits half the
// ring, go straight to their destination), finish() synchronises once and hands the ring's regions out with plain memcpys.
// (Copied straight into pageable memory each array is staged by the runtime and waited for in turn, ~17 us apiece.)
struct StagedDownloads {
    hgmm_ctx* c;
    struct Pending { void* dst; const void* src; size_t bytes; };
    std::vector<Pending> pending;
    size_t staged = 0;
    hipError_t e = hipSuccess;
    size_t limit;
    explicit StagedDownloads(hgmm_ctx* ctx, size_t per_array_limit = 256u << 10) : c(ctx), limit(per_array_limit) {}
    void add(void* dst, const void* dev_src, size_t bytes) {
        if (e != hipSuccess || !dst || bytes == 0) return;
        void* st = nullptr;
        if (bytes <= limit && staged + bytes + 256 <= STAGE_RING_BYTES / 2 && stage_reserve(c, bytes, &st) == 0) {
            staged += (bytes + 255) & ~(size_t)255;
            e = hipMemcpyAsync(st, dev_src, bytes, hipMemcpyDeviceToHost, c->stream);
            pending.push_back({dst, st, bytes});
        } else {
            e = hipMemcpyAsync(dst, dev_src, bytes, hipMemcpyDeviceToHost, c->stream);
        }
    }
    // (hipSuccess, or the first error of a copy / of the synchronisation)
    hipError_t finish() {
        // always drain the stream, also after a failed add(): copies enqueued before the failure may still be in flight
        // into the caller's memory (a stack array in kmeans_kernels.hip), and the ring is only free once they are done
        const hipError_t es = ctx_stream_sync(c);
        if (e == hipSuccess) e = es;
        if (e == hipSuccess)
            for (const Pending& pd : pending) std::memcpy(pd.dst, pd.src, pd.bytes);
        if (es == hipSuccess) c->h_stage_off = 0;          // the stream is idle: every region of the ring is free
        pending.clear();
        return e;
    }
};

inline int fail(hgmm_ctx* c, int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (c) c->err = buf;
    return code;
}

// scan_weights (point_weights.h) of the n weights at w; a refusal in the weight entries' words, under the caller's `label`
template <class T>
inline int check_point_weights(hgmm_ctx* c, const char* label, const T* w, int64_t n, double* sum_out) {
    const WeightScan s = scan_weights(w, n);
    if (s.verdict == WEIGHTS_BAD_VALUE)
        return fail(c, HGMM_ERR_ARG, "%s: weight %lld is %g (weights must be finite and >= 0)", label, (long long)s.index, s.value);
    if (s.verdict == WEIGHTS_ALL_ZERO) return fail(c, HGMM_ERR_ARG, "%s: all %lld weights are zero", label, (long long)n);
    if (s.verdict == WEIGHTS_SUM_NOT_FINITE) return fail(c, HGMM_ERR_ARG, "%s: the weights' sum is not finite", label);
    *sum_out = s.sum;
    return HGMM_OK;
}

// The _weighted entries of the full-covariance fit and of KMeans: their own refusals (include/hgmm.h), made before anything
// resident is touched; on success *wts is the resident source-weight array [n_pad], on the row index of x_soa64
inline int source_weights_ready(hgmm_ctx* c, const char* what, const double** wts) {
    if (!c->have_f64 || c->n <= 0) return fail(c, HGMM_ERR_STATE, "%s: set points first", what);
    if (!c->src.ptr() || c->src.buf.cap < sizeof(double) * (size_t)c->n_pad)
        return fail(c, HGMM_ERR_STATE, "%s: no source weights are resident (set them with hgmm_tree_set_source_weights or "
                    "hgmm_voxel_to_points(..., HGMM_VOXEL_W_TREE), or call the unweighted entry)", what);
    if (c->comm_on())
        return fail(c, HGMM_ERR_STATE, "%s: the context has a communicator; sharded weighted fits are not supported", what);
    *wts = c->src.ptr();
    return HGMM_OK;
}

#define HGMM_HIP(ctx, call)                                                              \
    do {                                                                                 \
        hipError_t e_ = (call);                                                          \
        if (e_ != hipSuccess)                                                            \
            return hgmm::fail((ctx), HGMM_ERR_HIP, "%s failed: %s (%s:%d)", #call,       \
                              hipGetErrorString(e_), __FILE__, __LINE__);                \
    } while (0)

#define HGMM_NCCL(ctx, call)                                                             \
    do {                                                                                 \
        ncclResult_t r_ = (call);                                                        \
        if (r_ != ncclSuccess)                                                           \
            return hgmm::fail((ctx), HGMM_ERR_RCCL, "%s failed: %s (%s:%d)", #call,      \
                              ncclGetErrorString(r_), __FILE__, __LINE__);               \
    } while (0)

// First statement of every extern "C" entry that takes a context: the current HIP device is a property of the calling
// THREAD, so a caller that drives two contexts from one thread, or one context from several, gets the context's own
// device for every allocation, event and launch the entry makes (include/hgmm.h: "distinct contexts may be driven from
// distinct threads").  hipSetDevice on the device that is already current is a thread-local compare.
#define HGMM_ENTER(ctx)                                                                  \
    do {                                                                                 \
        if (!(ctx)) return HGMM_ERR_ARG;                                                 \
        HGMM_HIP((ctx), hipSetDevice((ctx)->device));                                    \
    } while (0)

#define HGMM_TRY(expr)                   \
    do {                                 \
        int rc_ = (expr);                \
        if (rc_ != HGMM_OK) return rc_;  \
    } while (0)

int ensure(hgmm_ctx* c, DevBuf& b, size_t bytes);
// (hgmm_api.hip) the cloud `p` becomes the one every kernel of the context works on; storage for n points in `p`
void bind_points(hgmm_ctx* c, hgmm_points* p);
int points_alloc(hgmm_ctx* c, hgmm_points* p, int64_t n);
// (voxel_handover.hip) rows[k] (device, row numbers of the resident cloud's float64 view) -> out [k][3] (device): one launch
int gather_rows(hgmm_ctx* c, const int64_t* dev_rows, int64_t k, double* dev_out);
// (voxel_handover.hip) init_rows [k] of hgmm_tree_build_rows / _batch_rows (host; `first`: what is added to every `per` rows,
// NULL: nothing) -> scratch [k][3], the place the builds read their initial means from.  The rows have been checked.
int stage_init_rows(hgmm_ctx* c, const int64_t* rows, int64_t k, const int64_t* first, int64_t per);
// (flat_kernels.hip) the batched flat fit behind hgmm_flat_train_batch, _weighted and _voxels: flat_batch_check is every
// refusal the three share (nothing is touched), flat_batch_run the launch set over slots whose rows and weights are on the
// device already.  `what` names the entry in the messages.
int flat_batch_check(hgmm_ctx* c, const char* what, int B, int cov_type, int variant, int J, int max_iter, const float* mu,
                     const float* cov, const float* w, const int32_t* n_iter_out, const int32_t* converged_out);
int flat_batch_run(hgmm_ctx* c, const char* what, int B, const FlatBatchSlot* slots, int cov_type, int variant, int J,
                   int max_iter, float tol, float* mu, float* cov, float* w, float* inv_std_out, float* lls_out,
                   int32_t* n_iter_out, int32_t* converged_out);

// profiling brackets: record an event pair around one kernel launch when enabled
struct ProfScope {
    hgmm_ctx* c;
    EventPair* ev = nullptr;
    ProfScope(hgmm_ctx* ctx, int kernel);
    ~ProfScope();
};
int profile_collect(hgmm_ctx* c);

// ---- the instantiation of a kernel family for run-time flags -------------------------------------------------------------
// kernel_for<FAMILY>(flag, flag, ...) is FAMILY::kernel<flag, flag, ...>(): a family is a struct whose static member
// template `kernel` names the instantiation for its compile-time flags.  The one place a further flag is added.
template <class FAMILY, bool... FLAGS>
inline auto kernel_for() { return FAMILY::template kernel<FLAGS...>(); }
template <class FAMILY, bool... FLAGS, class... REST>
inline auto kernel_for(bool flag, REST... rest) {
    return flag ? kernel_for<FAMILY, FLAGS..., true>(rest...) : kernel_for<FAMILY, FLAGS..., false>(rest...);
}

// the communicator's all-reduces (hgmm_api.hip)
int allreduce_f64_dev(hgmm_ctx* c, double* dev, size_t n);
int allreduce_f64_oop(hgmm_ctx* c, const double* src, double* dst, size_t n);
int allreduce_i64_dev(hgmm_ctx* c, long long* dev, size_t n);      // exact (integer) sum, in place

}  // namespace hgmm
