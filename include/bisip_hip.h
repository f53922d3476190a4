/*
 * bisip_hip.h -- C ABI of libbisip_hip.so, the MI355X (gfx950) implementation of
 * BISIP's ensemble-MCMC log-probability hot path.
 *
 * This is the drop-in boundary.  Every entry point replaces a
 * piece of the reference's per-walker Python/Cython path with its batched
 * (walker-vectorised) form; citations are relative to /root/reference:
 *
 *   bisip_ctx_create      the walker-independent operands the reference binds into
 *                         emcee's `args` tuple and the model's precompute:
 *                         src/bisip/models.py:108-109 (forward, bounds, w, zn, zn_err),
 *                         src/bisip/models.py:200-213 (taus, log_taus, c_exp),
 *                         src/bisip/utils.py:138-144 (zn, zn_err, w layout)
 *   bisip_ctx_set_bounds  `model.params.update(...)` between fits; param_bounds is
 *                         re-read at fit() time: src/bisip/models.py:176-179, 102-109
 *   bisip_logprob[_dev]   Inversion._log_probability for W rows at once:
 *                         src/bisip/models.py:59-76 fused with the forward models of
 *                         src/bisip/cython_funcs.pyx:33-108
 *   bisip_forward[_dev]   Model.forward(theta, w) for W rows at once:
 *                         src/bisip/models.py:217-229, 256-271, 295-305, 335-349
 *                         (the loop of src/bisip/utils.py:33-34)
 *
 * Conventions: plain pointers and sizes, no framework types.  All arrays are
 * C-contiguous IEEE binary64.  theta is (W, ndim) row-major -- the layout emcee
 * hands to log_prob_fn -- and row i of the input produces element i of the
 * output.  Functions return 0 on success and a negative BISIP_E* code on failure;
 * bisip_last_error() then describes the failure (thread-local string).
 * A context is bound to one device and is not thread-safe.
 */
#ifndef BISIP_HIP_H
#define BISIP_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2: entry points added since 1 (all additions, nothing changed or removed): loglike_z, forward_percentiles,
 * column / grouped / columns percentiles, forward_spectrum(s) / forward_columns, stretch_run_sharded + rccl_*, ctx_set_spectrum_offset,
 * ctx_reduced_check, polydecomp_reduced_estimates, read_tables; BISIP_VARIANT_REDUCED_COMP, BISIP_ERCCL.
 * 3: clock_probe_dev, ctx_reduced_guard, polydecomp_reduced_reference, stretch_run_sharded_sim_dev (additions only).
 * 4: chain_shell_rows_dev (+ _workspace), ctx_reduced_guard_rows, ensemble_gram_dev (+ _workspace),
 *    fp64_stream_probe_dev (+ _lanes), stretch_run_philox_dev (+ stretch_philox_inline) (additions only).
 * 5: chain_autocorr_time_dev (+ _workspace) (additions only).
 * 6: rtd_integrals_dev, rtd_columns_dev (additions only); chain_range_dev, chain_histograms_dev,
 *    chain_pair_histograms_dev, then chain_trace_dev (+ _workspace, _lds_walkers), then chain_rhat_dev (+ _workspace),
 *    then chain_cov_dev and chain_best_sample_dev (+ _workspace), then forward_columns_kind_dev,
 *    forward_percentiles_kind and response_moments_dev (+ _workspace) with BISIP_RESPONSE_RI / _PA, then
 *    fit_quality_dev (+ _workspace), then reduced_emulate and ctx_reduced_operands, then q_columns_dev and
 *    loo_columns_dev (+ _workspace), then rtd_descriptors_dev and rtd_descriptors_host, then predictive_check_dev
 *    (+ _workspace), then mode_order_dev and mode_order_host, then gauss_newton_dev, map_fit_dev and lm_step_host came
 *    later under the same number (additions only: a caller that needs them looks the symbols up). */
#define BISIP_ABI_VERSION 6

/* model_id -- the four reference model classes (src/bisip/models.py:182,232,274,308) */
#define BISIP_MODEL_POLYDECOMP 0 /* PolynomialDecomposition -> Decomp_cyth  */
#define BISIP_MODEL_COLECOLE   1 /* PeltonColeCole          -> ColeCole_cyth */
#define BISIP_MODEL_DIAS2000   2 /* Dias2000                -> Dias2000_cyth */
#define BISIP_MODEL_SHIN2015   3 /* Shin2015                -> Shin2015_cyth */

/* kernel formulation for PolynomialDecomposition (other models have one) */
#define BISIP_VARIANT_AUTO      0 /* fastest formulation that holds the parity tolerance: REDUCED, else
                                     REDUCED_COMP, else COLLAPSED (see bisip_ctx_reduced_error) */
#define BISIP_VARIANT_FAITHFUL  1 /* sum_k M_k*K[j,k], the reference's loop structure     */
#define BISIP_VARIANT_COLLAPSED 2 /* Z_j = R0*(1 - sum_p a_p*G[j,p])                       */
#define BISIP_VARIANT_REDUCED   3 /* QR-reduced chi^2: (P+2)x(P+2) triangular form         */
#define BISIP_VARIANT_WAVE      4 /* collapsed operands, one wave per walker, LDS-staged
                                     spectrum, wavefront-shuffle reduction (N <= 64)        */
#define BISIP_VARIANT_REDUCED_COMP 5 /* the QR-reduced form in compensated (double-double row
                                     sums) arithmetic: for nearly collinear designs        */

/* status codes */
#define BISIP_OK          0
#define BISIP_EINVAL     -1 /* bad argument (shape, null pointer, unsupported size) */
#define BISIP_EHIP       -2 /* a HIP runtime call failed                             */
#define BISIP_ENOMEM     -3
#define BISIP_EUNSUPPORTED -4
#define BISIP_ERCCL     -5 /* an RCCL call failed                                   */

/* representation of a model response (bisip_amd/response.py) */
#define BISIP_RESPONSE_RI 0 /* real and imaginary part: what forward returns                          */
#define BISIP_RESPONSE_PA 1 /* amplitude hypot(re, im) and MINUS the phase, -atan2(im, re), in rad    */

#define BISIP_MAX_NDIM 16
#define BISIP_MAX_MODES 5
#define BISIP_MAX_POLY_DEG 10

typedef struct bisip_ctx bisip_ctx;

/* Model-specific description.  Unused fields are ignored. */
typedef struct bisip_model_desc {
    int n_modes;            /* COLECOLE: number of Cole-Cole modes D (ndim = 1+3D)        */
    int poly_deg;           /* POLYDECOMP: P (ndim = P+2)                                 */
    int n_taus;             /* POLYDECOMP: S, length of the relaxation-time grid           */
    double c_exp;           /* POLYDECOMP: fixed Cole-Cole exponent (1 Debye, 0.5 Warburg) */
    const double *taus;     /* POLYDECOMP: (S,)       = 10**log_tau                        */
    const double *log_taus; /* POLYDECOMP: (P+1, S)   = log_tau**i, row-major              */
} bisip_model_desc;

/* Create a context on `device`.  w (N,), zn (2,N) [row 0 real, row 1 imaginary],
 * zn_err (2,N), lo/hi (ndim,) are copied; the caller keeps ownership. */
int bisip_ctx_create(bisip_ctx **out, int device, int model_id, int N, const double *w,
                     const double *zn, const double *zn_err, int ndim, const double *lo,
                     const double *hi, const bisip_model_desc *desc);

/* Batch of independent spectra (BASELINE config 5): n_spectra spectra that share the model
 * shape, N and the prior box; w (E,N), zn (E,2,N), zn_err (E,2,N).  The same entry points
 * then take theta (E*Wp, ndim) with rows [e*Wp, (e+1)*Wp) belonging to spectrum e (W must
 * be a multiple of E).  PolynomialDecomposition: desc->taus/log_taus are shared by all
 * spectra.  One reference Inversion object per spectrum: src/bisip/models.py:41-57. */
int bisip_batch_create(bisip_ctx **out, int device, int model_id, int n_spectra, int N,
                       const double *w, const double *zn, const double *zn_err, int ndim,
                       const double *lo, const double *hi, const bisip_model_desc *desc);
int bisip_ctx_nspectra(const bisip_ctx *ctx);

void bisip_ctx_destroy(bisip_ctx *ctx);

/* Replace the prior box (strict inequalities, lo < theta < hi).  PolynomialDecomposition: the reduced form's
 * expansion points are chosen again for the new box; where their operands live in device memory (a batch; a lone
 * spectrum's compensated tier from degree 6 on) the call waits for the device's earlier work before it rewrites them. */
int bisip_ctx_set_bounds(bisip_ctx *ctx, const double *lo, const double *hi);

/* Choose the kernel formulation (BISIP_VARIANT_*). */
int bisip_ctx_set_variant(bisip_ctx *ctx, int variant);
int bisip_ctx_get_variant(const bisip_ctx *ctx);

/* theta (W,ndim) host -> logp (W,) host.  Synchronous. */
int bisip_logprob(bisip_ctx *ctx, const double *theta, int64_t W, double *logp);

/* Same with device-resident buffers, asynchronous on `stream` (a hipStream_t;
 * NULL = the default stream). */
int bisip_logprob_dev(bisip_ctx *ctx, const double *d_theta, int64_t W, double *d_logp,
                      void *stream);

/* theta (W,ndim) -> Z (W,2,N). */
int bisip_forward(bisip_ctx *ctx, const double *theta, int64_t W, double *Z);
int bisip_forward_dev(bisip_ctx *ctx, const double *d_theta, int64_t W, double *d_Z,
                      void *stream);
/* Batch context: forward of rows that ALL belong to spectrum `spectrum` (the model response over one
 * spectrum's chain: utils.get_model_percentile per spectrum of a survey, src/bisip/utils.py:17-35). */
int bisip_forward_spectrum_dev(bisip_ctx *ctx, int64_t spectrum, const double *d_theta, int64_t W,
                               double *d_Z, void *stream);
/* The same responses written COLUMN-major, d_cols (n_spectra, 2N, W / n_spectra): one contiguous column per
 * (spectrum, part, frequency) -- the layout bisip_columns_percentiles_dev reads, so the model-space bands of
 * a survey need no transposition.  Any number of rows per spectrum. */
int bisip_forward_columns_dev(bisip_ctx *ctx, int64_t first_spectrum, int64_t n_spectra, const double *d_theta,
                              int64_t W, double *d_cols, void *stream);
/* ... in the representation `kind` (BISIP_RESPONSE_*).  RI: the same kernel and the same bits as
 * bisip_forward_columns_dev.  PA: column j of a spectrum holds the amplitude hypot(re, im) and column N + j MINUS the
 * phase, -atan2(im, re), in rad and in [-pi, pi] (no unwrapping) -- the device library's hypot and atan2 of every
 * sample's own response (the amplitude is not selected on re * re + im * im), so bisip_columns_percentiles_dev gives
 * the amplitude / phase bands of the posterior from these columns as it gives the Re / Im ones: no second kernel, no
 * second pass.  BISIP_EINVAL for any other kind. */
int bisip_forward_columns_kind_dev(bisip_ctx *ctx, int64_t first_spectrum, int64_t n_spectra, const double *d_theta,
                                   int64_t W, double *d_cols, int kind, void *stream);
/* ... or to n_spectra consecutive spectra starting with first_spectrum, W / n_spectra rows each
 * (a multiple of 64 when n_spectra > 1), in one launch. */
int bisip_forward_spectra_dev(bisip_ctx *ctx, int64_t first_spectrum, int64_t n_spectra, const double *d_theta,
                              int64_t W, double *d_Z, void *stream);

/* Gaussian log-likelihood of a model response the caller evaluated itself: Z (W,2,N)
 * [row 0 real, row 1 imaginary per walker] -> (W,)  =  -0.5*sum((zn - Z)^2/zn_err^2 +
 * 2 ln zn_err^2).  Inversion._log_likelihood(theta, f, x, y, yerr) with a callable f that is
 * not the model's own forward: src/bisip/models.py:59-62 (the host runs f, the reduction is
 * this kernel).  No prior.  Single-spectrum contexts only. */
int bisip_loglike_z(bisip_ctx *ctx, const double *Z, int64_t W, double *loglike);
int bisip_loglike_z_dev(bisip_ctx *ctx, const double *d_Z, int64_t W, double *d_loglike,
                        void *stream);

/* ---- device-resident stretch move (the emcee inner loop the reference runs around the
 * log-probability: src/bisip/models.py:111-118; algorithm: emcee StretchMove with a
 * red/blue split, a = stretch scale) -------------------------------------------------
 * One half-step moves the walkers of the active half.  Slot t moves walker active[t]
 * along the line through walker partner[t] (a member of the complementary half):
 *     q = c - (c - s)*zz[t];   accept iff factor[t] + logp(q) - logp(s) > logu[t]
 * where the caller supplies factor = (ndim-1)*ln(zz) and logu = ln(u) from its RNG
 * stream (bisip_amd/sampler.py documents the stream order).  All pointers are device
 * pointers; coords (W,ndim) and logp (W,) are updated in place; optional chain_row
 * (W,ndim) / logp_row (W,) receive the post-move state of the moved walkers and
 * naccept (W,) counts acceptances; status gets bit 0 set if a proposal's
 * log-probability is NaN. */
typedef struct bisip_stretch_args {
    double *coords;
    double *logp;
    const int32_t *active;
    const int32_t *partner;
    const double *zz;
    const double *factor;
    const double *logu;
    int64_t n_slots;   /* slots in this half-step                                    */
    int64_t slot_lo;   /* eval: first slot evaluated by this rank                    */
    int64_t slot_hi;   /* eval: one past the last slot evaluated by this rank        */
    double *block;     /* eval: out (slot_hi-slot_lo, ndim+2) = row, logp, accepted  */
                       /* apply: in, the all-gathered (world*pad, ndim+2) buffer     */
    double *chain_row; /* may be NULL */
    double *logp_row;  /* may be NULL */
    int32_t *naccept;  /* may be NULL */
    int32_t *status;   /* required */
    int64_t pad;       /* apply: rows per rank slab in `block`                       */
    int32_t world;     /* apply: number of ranks that produced `block`               */
    int64_t walkers_per_spectrum; /* batch contexts: Wp (even); walker i belongs to spectrum
                                     i / Wp.  Ignored (may be 0) for single-spectrum contexts */
} bisip_stretch_args;

/* Single-rank half-step: evaluate all n_slots slots and update the state (one launch). */
int bisip_stretch_half_dev(bisip_ctx *ctx, const bisip_stretch_args *args, void *stream);
/* Sharded half-step: evaluate slots [slot_lo, slot_hi) into args->block ... (single-spectrum contexts: a batch of
 * spectra shards as whole replicas; BISIP_EUNSUPPORTED for a batch context) */
int bisip_stretch_eval_dev(bisip_ctx *ctx, const bisip_stretch_args *args, void *stream);
/* ... and, after the caller's all-gather of the blocks, apply all n_slots slots. */
int bisip_stretch_apply_dev(bisip_ctx *ctx, const bisip_stretch_args *args, void *stream);

/* Run n_steps whole iterations (2 half-steps each) back to back on `stream` with no host
 * round trip.  `first` holds the pointers of step 0 / half 0; the random-stream arrays are
 * laid out (n_steps, 2, nh) with nh = (W+1)/2 (half 0 has ceil(W/2) slots, half 1
 * floor(W/2)); chain_row / logp_row advance by W*ndim / W per step.  For a batch context W
 * is the TOTAL number of walkers E*Wp and the arrays are (n_steps, 2, E, Wp/2).
 * thin_by >= 1: only every thin_by-th iteration is stored (chain_row / logp_row then hold
 * n_steps/thin_by rows; n_steps must be a multiple of thin_by). */
int bisip_stretch_run_dev(bisip_ctx *ctx, const bisip_stretch_args *first, int64_t W,
                          int64_t n_steps, int64_t thin_by, void *stream);

/* ---- the same move with the walkers sharded over the GPUs of one node (one process per GPU,
 * RCCL over xGMI; the reference's only parallel hook is fit(pool=...) -> emcee's pool.map over
 * walkers, src/bisip/models.py:84,91-94,115).  Every rank holds the whole ensemble and the same
 * random stream, evaluates slots [rank's block) of each half-step, and one all-gather per
 * half-step rebuilds the state on every rank.
 *
 * bisip_stretch_run_sharded_dev: n_steps whole iterations, per half-step
 *     eval (this rank's slots -> its slab of the gather buffer)  ->  ncclAllGather (in place)
 *     ->  apply (every slot -> state + chain)
 * all enqueued on `stream` with no host round trip.  Arguments as for bisip_stretch_run_dev
 * (first->block / pad / world / slot_lo / slot_hi are ignored: the library owns the gather
 * buffer, allocated once per context, ceil(slots/world)*(ndim+2) doubles per rank).  `comm` is
 * an ncclComm_t whose ranks all make this call with the same arguments: one made by
 * bisip_rccl_comm_create, or an existing one (e.g. PyTorch's ProcessGroupNCCL._comm_ptr()).
 * The chain is bit-identical to bisip_stretch_run_dev's on every rank.  RCCL is bound at run
 * time (dlopen of librccl.so.1); BISIP_EUNSUPPORTED when it is absent, BISIP_ERCCL when a call
 * fails.  Single-spectrum contexts only (a batch of spectra shards as whole replicas). */
int bisip_stretch_run_sharded_dev(bisip_ctx *ctx, void *comm, const bisip_stretch_args *first,
                                  int64_t W, int64_t n_steps, int64_t thin_by, void *stream);

/* Test aid: the same loop with EVERY rank of a `world`-rank group evaluated on this device, one after
 * another, each into the slab of the gather buffer it would have sent, and no collective -- the slot
 * ranges, pads and slab offsets a multi-rank run depends on, checkable on one GPU (odd ensembles, more ranks
 * than slots, empty shards).  The chain equals the fused single-GPU chain bit for bit. */
int bisip_stretch_run_sharded_sim_dev(bisip_ctx *ctx, int world, const bisip_stretch_args *first, int64_t W,
                                      int64_t n_steps, int64_t thin_by, void *stream);

/* Stand-alone communicator for callers without one: rank 0 fills a BISIP_RCCL_ID_BYTES id
 * (ncclGetUniqueId), ships it to the other ranks by any means, and every rank creates its
 * communicator on `device` (ncclCommInitRank: collective over the `world` ranks). */
#define BISIP_RCCL_ID_BYTES 128
int bisip_rccl_unique_id(void *id);
int bisip_rccl_comm_create(void **comm, int world, int rank, const void *id, int device);
int bisip_rccl_comm_destroy(void *comm);

/* A batch context that holds spectra [first_spectrum, first_spectrum + E) of a larger survey
 * (one block per GPU): bisip_stretch_draw_dev then keys spectrum e's stream by its index in the
 * SURVEY, so every spectrum's chain is the same however the survey is split over GPUs.
 * Default 0.  (The reference has no batch object: a survey is a loop over Inversion objects,
 * src/bisip/models.py:41-57.) */
int bisip_ctx_set_spectrum_offset(bisip_ctx *ctx, int64_t first_spectrum);

/* Fill the random-stream arrays on the device (counter-based Philox4x32-10; the contract
 * is documented in bisip_amd/csrc/sampler_kernels.h and bisip_amd/sampler.py).
 * d_perm (n_steps,3) = per-step affine split (A, A^-1 mod W, B).  W = walkers per ensemble;
 * a batch context draws for all its spectra: arrays (n_steps, 2, E, W/2), global walker ids. */
int bisip_stretch_draw_dev(bisip_ctx *ctx, int64_t W, double a, uint64_t seed, int64_t step0,
                           int64_t n_steps, const int32_t *d_perm, int32_t *d_active,
                           int32_t *d_partner, double *d_zz, double *d_factor, double *d_logu,
                           void *stream);

/* bisip_stretch_run_dev for the Philox stream WITHOUT its arrays: every half-step launch draws its slots' entries
 * (walker, partner, z, (ndim-1) ln z, ln u) from their counters in place -- the same numbers bisip_stretch_draw_dev
 * writes, so the chain is that of draw + run bit for bit -- and nothing of the stream is written, stored or read:
 * at a million walkers the arrays are 34 MB per iteration, a fifth of the half-step's traffic, and drawing them
 * took a quarter of its time.  first->active / partner / zz / factor / logu are ignored (may be null); a, seed,
 * step0, d_perm as for bisip_stretch_draw_dev (d_perm: this chunk's n_steps rows).  Only where
 * bisip_stretch_philox_inline(ctx, W) returns 1 -- a single ensemble big enough for the packed-state half-step
 * (ndim <= 7, >= 131,072 walkers) -- otherwise BISIP_EUNSUPPORTED: draw, then run.  (emcee draws its stream on the
 * host, src/bisip/models.py:111-118 -> EnsembleSampler.run_mcmc.) */
int bisip_stretch_philox_inline(const bisip_ctx *ctx, int64_t W);
int bisip_stretch_run_philox_dev(bisip_ctx *ctx, const bisip_stretch_args *first, int64_t W, int64_t n_steps,
                                 int64_t thin_by, double a, uint64_t seed, int64_t step0, const int32_t *d_perm,
                                 void *stream);

/* Persistent sampler: one workgroup per ensemble runs n_steps iterations inside ONE launch
 * (ensemble in LDS, workgroup barrier between half-steps, several lanes per walker for the
 * models with a frequency loop).  Reads the same pre-drawn random stream as
 * bisip_stretch_run_dev -- arrays (n_steps, 2, E, nh), nh = (walkers_per_ensemble+1)/2,
 * global walker ids -- and produces bit-identical results.  Requires
 * walkers_per_ensemble*(ndim+1)*8 <= 65536 bytes of LDS and ceil(walkers_per_ensemble/2)
 * <= 512; otherwise returns BISIP_EUNSUPPORTED (use bisip_stretch_run_dev).
 * n_walkers = n_ensembles * walkers_per_ensemble. */
typedef struct bisip_persist_args {
    double *coords;              /* (n_walkers, ndim) in/out */
    double *logp;                /* (n_walkers,)      in/out */
    int64_t n_walkers;
    int64_t walkers_per_ensemble;
    int64_t n_steps;
    int64_t thin_by;
    const int32_t *active;       /* random stream, as in bisip_stretch_args */
    const int32_t *partner;
    const double *zz;
    const double *factor;
    const double *logu;
    double *chain;               /* (n_steps/thin_by, n_walkers, ndim) or NULL */
    double *logp_chain;          /* (n_steps/thin_by, n_walkers) or NULL */
    int32_t *naccept;            /* (n_walkers,) or NULL */
    int32_t *status;             /* required */
} bisip_persist_args;
int bisip_stretch_persistent_dev(bisip_ctx *ctx, const bisip_persist_args *args, void *stream);

/* ---- differential-evolution and snooker moves beside the stretch move (emcee's DEMove and DESnookerMove, the
 * mixture emcee advises for multimodal targets; the reference hands `moves` to emcee: src/bisip/models.py:84,111-118).
 * Launch-per-half-step path, rng = Philox, one rank; single-spectrum and batch contexts.  The red/blue halves and the
 * active walker of slot t are the stretch contract's; partners are members of the complementary half (Nc members),
 * addressed by rank r -> walker pi^-1(2r + 1 - h).
 *   DE (ter Braak 2006):  q_k = s_k + gamma (ca_k - cb_k), gamma = g0 (1 + sigma n), n ~ N(0,1); factor = 0
 *   snooker (ter Braak & Vrugt 2008):  d = s - z, n2 = sum d_k^2, u = d / sqrt(n2), p1 = sum u_k z1_k,
 *        p2 = sum u_k z2_k, q_k = s_k + u_k (gammas (p1 - p2)), m2 = sum (q_k - z_k)^2,
 *        factor = 0.5 (ndim - 1) (ln m2 - ln n2); n2 == 0 is a rejection that raises no flag
 *   (sums over k = 0 .. ndim-1, multiply then add, nothing contracted)
 *   accept iff (factor + logp(q)) - logp(s) > logu; a NaN log-probability sets status bit 0, -inf rejects.
 * emcee 3's snooker divides by sqrt(norm) and takes the logs of the norms, not of their squares: that is not the
 * published move and is not what runs here.  bisip_amd/moves.py states moves and stream in NumPy.
 *
 * The stream extends the Philox contract (bisip_amd/csrc/sampler_kernels.h, DrawArgs): same key, the counter's
 * fourth word names the purpose, purposes 0-2 keep every number they give.
 *   3, counter (k, 0, 0, 3):        the iteration's move among weighted moves (host: moves.py, move_schedule)
 *   4, counter (t, k, h | e<<1, 4): i0 = (x0 Nc) >> 32; i1 = (x1 (Nc-1)) >> 32, +1 if >= i0;
 *                                   i2 = (x2 (Nc-2)) >> 32, +1 if >= min(i0,i1), then +1 if >= max(i0,i1)
 *                                   DE: a, b = i0, i1;  snooker: z, z1, z2 = i0, i1, i2
 *   5, counter (t, k, h | e<<1, 5): n = sqrt(-2 ln(1 - u53(x0,x1))) cos(2 pi u53(x2,x3))
 *   logu: the purpose-1 number of the slot.
 *
 * bisip_move_args: `stretch` holds the state, the chain rows and the counters of bisip_stretch_args, and -- for the
 * stretch iterations of a mixture -- the arrays bisip_stretch_draw_dev wrote; the other fields are the arrays of
 * bisip_move_draw_dev, laid out alike ((n_steps, 2, E, nh), global walker ids; p2 is 0 where Nc < 3). */
#define BISIP_MOVE_STRETCH 0
#define BISIP_MOVE_DE 1
#define BISIP_MOVE_SNOOKER 2
typedef struct bisip_move_args {
    bisip_stretch_args stretch;
    const int32_t *active;
    const int32_t *p0;
    const int32_t *p1;
    const int32_t *p2;
    const double *gamma;   /* DE: g0 (1 + sigma n) */
    const double *logu;
    double snooker_gamma;  /* snooker: gammas */
} bisip_move_args;

/* Fill the arrays of purposes 4, 5 and 1 for n_steps iterations (arguments as for bisip_stretch_draw_dev).
 * BISIP_EINVAL for W < 4 (a half of fewer than two members has no pair). */
int bisip_move_draw_dev(bisip_ctx *ctx, int64_t W, uint64_t seed, int64_t step0, int64_t n_steps,
                        const int32_t *d_perm, double de_g0, double de_sigma, int32_t *d_active, int32_t *d_p0,
                        int32_t *d_p1, int32_t *d_p2, double *d_gamma, double *d_logu, void *stream);

/* One half-step of move `kind` (BISIP_MOVE_*; BISIP_MOVE_STRETCH is bisip_stretch_half_dev on args->stretch).
 * W = walkers per ensemble.  BISIP_EINVAL when the complementary half has fewer than 2 members (DE: W >= 4) or 3
 * (snooker: W >= 6); BISIP_EUNSUPPORTED for the faithful / wave formulation, as the stretch dispatch says. */
int bisip_move_half_dev(bisip_ctx *ctx, const bisip_move_args *args, int kind, int64_t W, void *stream);

/* n_steps whole iterations back to back on `stream`: iteration k runs move kinds[k] (a HOST array of BISIP_MOVE_*,
 * read before the call returns).  `first`, W, thin_by as for bisip_stretch_run_dev; every array advances by nh per
 * half-step.  A run whose kinds are all BISIP_MOVE_STRETCH is bisip_stretch_run_dev's chain bit for bit -- but not
 * its speed for one ensemble of 131,072 walkers or more: the state stays in its plain layout here, so a stretch
 * iteration runs the plain half-step, never the packed-state one, and the stream always comes from its arrays. */
int bisip_move_run_dev(bisip_ctx *ctx, const bisip_move_args *first, const int32_t *kinds, int64_t W,
                       int64_t n_steps, int64_t thin_by, void *stream);

/* Posterior mean and (population) standard deviation of every parameter, per ensemble, of a
 * chain resident in device memory -- the device form of get_param_mean / get_param_std
 * (src/bisip/utils.py:55-85: np.mean / np.std over the flattened chain) for batches whose
 * chains are too big to be worth copying to the host.
 * d_chain points at the first sample to use; sample k is at d_chain + k*sample_stride
 * doubles and holds (n_ensembles*walkers_per_ensemble, ndim) rows, ensemble e owning rows
 * [e*Wp, (e+1)*Wp).  (discard/thin of get_chain: offset the pointer, multiply the stride.)
 * d_mean, d_std: (n_ensembles, ndim); ndim 1 ... BISIP_MAX_NDIM, n_ensembles < 2^31.
 * Two passes over the chain (mean, then centred squares), each in this order; E = n_ensembles, Wp =
 * walkers_per_ensemble, n = n_samples, integer divisions round down:
 *   splits = max(1, min(ceil(4096 / E), n / 4)); split sp takes samples [n * sp / splits, n * (sp + 1) / splits).
 *   Lanes: of 256, the first lanes = (256 / ndim) * ndim work.  Lane t owns the doubles t, t + lanes, t + 2 lanes, ...
 *     of the Wp * ndim doubles that the ensemble has in a sample; every one of them is parameter t % ndim.
 *   Accumulators: four per lane, each from 0.0.  The samples of the split go in groups of four from its start: within a
 *     group, for each of the lane's doubles in turn, sample s + j goes to accumulator j (j = 0, 1, 2, 3 in this order).
 *     The one to three samples left over go to accumulator 0, sample after sample, the lane's doubles in turn.  The
 *     lane's sum is (a0 + a1) + (a2 + a3).
 *   Per parameter q of a split: the sums of lanes q, q + ndim, q + 2 ndim, ... (< lanes) are added in ascending order
 *     onto 0.0.  Per (ensemble, parameter): the splits' sums are added in ascending order onto 0.0.
 *   Pass 0: an accumulator adds x.  mean = sum / count, count = double(n) * double(Wp).
 *   Pass 1: d = x - mean (one rounding), the accumulator becomes fma(d, d, acc) (one rounding).  std = sqrt(sum / count).
 * IEEE throughout: a NaN in an (ensemble, parameter) makes its mean and std NaN; +inf or -inf alone that mean and a NaN
 * std; both, two NaN; nothing else changes.  Squares that leave binary64's range give std = +inf or 0.
 * d_work: bisip_chain_moments_workspace() DOUBLES, not bytes (every later *_workspace counts bytes): E * splits * ndim,
 * 0 when n_samples, n_ensembles or ndim is below 1.  BISIP_EINVAL and nothing written for a null pointer, a shape out of
 * range or sample_stride < E * Wp * ndim.  The plan depends on the shape alone, never on the device.  No atomics: the same
 * bits on every call (chainview.ordered_moments gives them in NumPy).  64-bit offsets.  Asynchronous on stream. */
int64_t bisip_chain_moments_workspace(int64_t n_samples, int64_t n_ensembles, int ndim);
int bisip_chain_moments_dev(const double *d_chain, int64_t n_samples, int64_t sample_stride,
                            int64_t n_ensembles, int64_t walkers_per_ensemble, int ndim,
                            double *d_mean, double *d_std, double *d_work, void *stream);

/* The second and fourth moments of every (ensemble, parameter) about a given centre: d_m2 and d_m4 (n_ensembles, ndim), the
 * means of (x - c)^2 and (x - c)^4 over the N = n_samples * walkers_per_ensemble values, c = d_center[e, q] (n_ensembles,
 * ndim) -- what the Monte-Carlo error of the standard deviation is made of (bisip_amd/diagnostics.py: mcse_sd).  Chain
 * layout, d_chain / sample_stride conventions and the order as for pass 1 of bisip_chain_moments_dev: its splits, lanes,
 * four accumulators per lane and per moment, (a0 + a1) + (a2 + a3), lanes and then splits in ascending order onto 0.0.
 * Per value: d = x - c (one rounding), q = d * d (one rounding), acc2 = fma(d, d, acc2), acc4 = fma(q, q, acc4); m = sum /
 * count, count = double(n) * double(Wp).  IEEE throughout: a centre or a value that is not finite makes both moments of
 * its (ensemble, parameter) NaN or +inf, nothing else changes.
 * d_work: bisip_chain_central_moments_workspace() DOUBLES, as bisip_chain_moments_workspace counts, times two.
 * BISIP_EINVAL and nothing written for a null pointer, a shape out of range or sample_stride < E * Wp * ndim.  No atomics:
 * the same bits on every call (diagnostics.ordered_central_moments gives them in NumPy).  Asynchronous on stream. */
int64_t bisip_chain_central_moments_workspace(int64_t n_samples, int64_t n_ensembles, int ndim);
int bisip_chain_central_moments_dev(const double *d_chain, int64_t n_samples, int64_t sample_stride,
                                    int64_t n_ensembles, int64_t walkers_per_ensemble, int ndim,
                                    const double *d_center, double *d_m2, double *d_m4, double *d_work, void *stream);

/* Percentiles of every parameter, per ensemble, of a chain resident in device memory -- the
 * device form of get_param_percentile (src/bisip/utils.py:37-53: np.percentile(chain, p,
 * axis=0), linear interpolation; the reference's default p is [2.5, 50, 97.5]).  Chain layout,
 * d_chain / sample_stride conventions as for bisip_chain_moments_dev.  percentiles: host array
 * (n_percentiles,) in [0, 100].  d_out: (n_percentiles, n_ensembles, ndim).  d_work:
 * bisip_chain_percentiles_workspace() BYTES of device memory (two column-major copies of the
 * used samples + the sort's scratch; 0 is returned for a shape that is not supported:
 * more than 2^31 values).  At most 8 percentiles per call are found by selecting the order statistics they
 * need (asynchronous on stream), more by sorting the columns (after a short synchronous upload); the doubles
 * are numpy.percentile's either way. */
int64_t bisip_chain_percentiles_workspace(int64_t n_samples, int64_t n_ensembles,
                                          int64_t walkers_per_ensemble, int ndim, int n_percentiles);
int bisip_chain_percentiles_dev(const double *d_chain, int64_t n_samples, int64_t sample_stride,
                                int64_t n_ensembles, int64_t walkers_per_ensemble, int ndim,
                                const double *percentiles, int n_percentiles, double *d_out,
                                void *d_work, int64_t work_bytes, void *stream);

/* Integrated autocorrelation time of every parameter, per ensemble, of a chain resident in device
 * memory -- emcee's integrated_time (emcee/autocorr.py 3.1: function_1d, auto_window) with the walkers
 * of each ensemble averaged.  Chain layout, d_chain / sample_stride conventions as for
 * bisip_chain_moments_dev.  Every series is centred, its autocorrelation taken as direct lag sums and
 * divided by lag 0; f = mean over the ensemble's walkers, taus = 2 cumsum(f) - 1 (sequential), and the
 * window is the first lag k where k < c*taus_k is false (n_samples - 1 when taus_0 is NaN: a constant
 * walker).  c: finite and > 0.  d_tau: (n_ensembles, ndim) = taus[window], in units of the samples
 * given; d_window: (n_ensembles, ndim) int64 or NULL.  Lags go in rounds; an (ensemble, parameter)
 * whose window is found stops there.  The tol check of integrated_time is the caller's.  d_work:
 * bisip_chain_autocorr_time_workspace() BYTES of device memory (mean and lag 0 of every series, one
 * round of lags per series, O(n_ensembles*ndim); 0 for a shape that is not supported).  No floating-
 * point atomics: the same chain gives the same bits.  Asynchronous on stream. */
int64_t bisip_chain_autocorr_time_workspace(int64_t n_samples, int64_t n_ensembles,
                                            int64_t walkers_per_ensemble, int ndim);
int bisip_chain_autocorr_time_dev(const double *d_chain, int64_t n_samples, int64_t sample_stride,
                                  int64_t n_ensembles, int64_t walkers_per_ensemble, int ndim, double c,
                                  double *d_tau, int64_t *d_window, void *d_work, void *stream);

/* Integrating parameters of PolynomialDecomposition for every used sample of a chain resident in device
 * memory -- what docs/tutorials/decomposition.ipynb (the get_m cell: m = sum_p a_p log_tau**p, total_m =
 * np.sum(m)) computes by hand from the posterior mean, here per posterior sample.  theta = (r0, a_0, ..., a_P),
 * ascending powers, ndim = P + 2 (2 ... BISIP_MAX_NDIM).  Chain layout, d_chain / sample_stride conventions
 * as for bisip_chain_moments_dev.  d_power_sums: (ndim,) device doubles S_k = sum_l log_tau_l^k, k = 0 ... P+1,
 * on the model's log_tau grid; d_norm_factor: (n_ensembles,) device doubles.  d_out: (n_samples,
 * n_ensembles*walkers_per_ensemble, 3) = (m_total = sum_p a_p S_p, log_tau_mean = sum_p a_p S_{p+1} / m_total,
 * m_norm = m_total / (r0 * norm_factor)) -- a chain of ndim = 3 that bisip_chain_moments_dev and
 * bisip_chain_percentiles_dev summarise unchanged.  Explicit fma, IEEE division (NaN / inf where m_total is 0).
 * Asynchronous on stream. */
int bisip_rtd_integrals_dev(const double *d_chain, int64_t n_samples, int64_t sample_stride, int64_t n_ensembles,
                            int64_t walkers_per_ensemble, int ndim, const double *d_power_sums,
                            const double *d_norm_factor, double *d_out, void *stream);

/* The relaxation time distribution m_l = sum_p a_p log_tau_l**p of every used sample -- the curves the
 * decomposition tutorial plots after its get_m cell (docs/tutorials/decomposition.ipynb) -- for ensembles
 * [first_ensemble, first_ensemble + count): d_cols (count*n_tau, n_samples*walkers_per_ensemble), one column
 * per (ensemble, l), row s*walkers_per_ensemble + w: what bisip_columns_percentiles_dev takes.  Same chain and
 * theta conventions as bisip_rtd_integrals_dev; d_log_tau: (n_tau,) device doubles.  Horner with fma.
 * Asynchronous on stream. */
int bisip_rtd_columns_dev(const double *d_chain, int64_t n_samples, int64_t sample_stride, int64_t n_ensembles,
                          int64_t walkers_per_ensemble, int ndim, int64_t first_ensemble, int64_t count,
                          const double *d_log_tau, int n_tau, double *d_cols, void *stream);

/* The relaxation descriptors of every used sample: where the RTD of that sample peaks and the cumulative relaxation
 * times at which the fractions q_1 ... q_J of its chargeability have accumulated (tau_10, tau_50, tau_90 of Nordsiek &
 * Weller, 2008) -- what a reader of the tutorial's RTD plots (docs/tutorials/decomposition.ipynb, after the get_m cell)
 * takes off the curve of the posterior mean by eye, here per posterior sample.  Same chain and theta conventions as
 * bisip_rtd_integrals_dev; d_log_tau: (n_tau,) device doubles, strictly ascending (the caller's to check); d_q: (n_q,)
 * device doubles in (0, 1] (the caller's to check), 1 <= n_q <= 8.  With m_l by Horner with fma as
 * bisip_rtd_columns_dev, c_l = m_l > 0 ? m_l : 0, g_l = g_{l-1} + c_l in ascending l and total = g_{n_tau-1}:
 * d_out (n_samples, n_ensembles*walkers_per_ensemble, 2 + n_q) = (log_tau_peak, m_peak, log_tau_q1, ..., log_tau_qJ);
 * the peak is the first l of the largest m_l; log_tau_q = log_tau_0 if g_0 >= t = q * total, else
 * fma((t - g_{k-1}) / c_k, log_tau_k - log_tau_{k-1}, log_tau_{k-1}) at the first k with g_k >= t.  A row whose total
 * is not finite and positive gives NaN throughout.  The statement in full: bisip_amd/decomposition.py.  A chain of
 * ndim = 2 + n_q that bisip_chain_moments_dev, bisip_chain_percentiles_dev and bisip_chain_hdi_dev summarise unchanged.
 * Asynchronous on stream. */
int bisip_rtd_descriptors_dev(const double *d_chain, int64_t n_samples, int64_t sample_stride, int64_t n_ensembles,
                              int64_t walkers_per_ensemble, int ndim, const double *d_log_tau, int n_tau,
                              const double *d_q, int n_q, double *d_out, void *stream);

/* Host-only, no GPU: the same rows by the same row function (csrc/rtd_descriptors.h) on the CPU -- every pointer a host
 * pointer -- which is what tests/test_gpu_relaxation.py holds bisip_rtd_descriptors_dev to, bit for bit. */
int bisip_rtd_descriptors_host(const double *chain, int64_t n_samples, int64_t sample_stride, int64_t n_ensembles,
                               int64_t walkers_per_ensemble, int ndim, const double *log_tau, int n_tau,
                               const double *q, int n_q, double *out);

/* The modes of every used sample of a PeltonColeCole chain put in order, and the per-mode descriptors of the ordered
 * row.  A multi-mode Cole-Cole posterior is symmetric under exchange of its modes; ordering them by one parameter group
 * makes the labelling identifiable.  theta = (r0, m_1..m_K, log_tau_1..K, c_1..K), n_modes = K in 1 ... BISIP_MAX_MODES,
 * ndim = 1 + 3K.  Chain layout, d_chain / sample_stride conventions as for bisip_chain_moments_dev.  key_group: 0 orders by
 * m, 1 by log_tau, 2 by c -- ascending by IEEE <, -0.0 and +0.0 tie, every NaN after +inf, NaNs tie, ties keep the stored
 * order (np.argsort(key, kind='stable')).  Each output is optional (a null pointer: not asked for, no stores); at least
 * one is required:
 *   d_ordered (n_samples, n_ensembles*walkers_per_ensemble, 1 + 3K): the row with position j of each group holding the
 *     values of mode perm[j] -- copies, the bits of the chain;
 *   d_desc (n_samples, n_ensembles*walkers_per_ensemble, 1 + 2K) = (m_total, log_tau_cc_1..K, log_tau_peak_1..K) of the
 *     ordered row: m_total = (..(m'_1 + m'_2) + ..) by plain additions, log_tau_cc_j = log_tau'_j + log1p(-m'_j) / c'_j
 *     (the time constant of the conductivity-form Cole-Cole model, tau (1 - m)^(1/c)), log_tau_peak_j = log_tau'_j +
 *     log1p(-m'_j) / (2 c'_j) (1/omega at which the phase of mode j alone peaks); IEEE division: -inf or NaN at m = 1, c = 0;
 *   d_moved (n_samples, n_ensembles*walkers_per_ensemble) bytes: 1 where the order differs from the stored one.
 * The statement in full: bisip_amd/modes.py.  d_ordered and d_desc are chains that bisip_chain_moments_dev,
 * bisip_chain_percentiles_dev and bisip_chain_hdi_dev summarise unchanged.  Asynchronous on stream. */
int bisip_mode_order_dev(const double *d_chain, int64_t n_samples, int64_t sample_stride, int64_t n_ensembles,
                         int64_t walkers_per_ensemble, int n_modes, int key_group, double *d_ordered, double *d_desc,
                         unsigned char *d_moved, void *stream);

/* Host-only, no GPU: the same rows by the same row function (csrc/mode_order.h) on the CPU -- every pointer a host
 * pointer -- which is what tests/test_gpu_modes.py holds bisip_mode_order_dev to: bit for bit on ordered, moved and m_total
 * (log1p is the host's here and the device's there). */
int bisip_mode_order_host(const double *chain, int64_t n_samples, int64_t sample_stride, int64_t n_ensembles,
                          int64_t walkers_per_ensemble, int n_modes, int key_group, double *ordered, double *desc,
                          unsigned char *moved);

/* The shapes of the posterior of a chain resident in device memory: the counts the reference draws in
 * plot_histograms (src/bisip/plotlib.py:56-90: np.histogram of every parameter, bins = 25) and in plot_corner
 * (src/bisip/plotlib.py:233-259: corner's 1-D and pairwise 2-D histograms, bins = 20).  Chain layout, d_chain /
 * sample_stride conventions as for bisip_chain_moments_dev; ndim 1 ... BISIP_MAX_NDIM (pairs: from 2).
 * Bin edges are made on the host (np.linspace) and uploaded: d_edges (n_ensembles, ndim, bins + 1) doubles, ascending.
 * Value x is in bin i iff edges[i] <= x < edges[i+1]; x == edges[bins] is in the last bin; anything else (outside the
 * edges, NaN) is counted nowhere -- the integers of np.histogram / np.histogram2d with the same edges.
 *   bisip_chain_range_dev: d_out (n_ensembles, ndim, 2) = min and max of the FINITE values of every (ensemble,
 *     parameter) ((+inf, -inf) when there is none); d_nonfinite (n_ensembles, ndim) int64 = how many values are NaN
 *     or +-inf (np.histogram's range=None refuses those).
 *   bisip_chain_histograms_dev: d_counts (n_ensembles, ndim, bins) int64, all parameters in one pass over the chain.
 *   bisip_chain_pair_histograms_dev: d_counts (n_ensembles, ndim (ndim - 1) / 2, bins, bins) int64, pairs (j, k), j < k,
 *     in np.triu_indices(ndim, 1) order; counts[e, q, a, b] = rows with parameter j_q in bin a and k_q in bin b; a row
 *     outside the edges in either coordinate is left out of that pair only.  Pairs whose counters do not fit the
 *     LDS of one workgroup together go in groups (one more read of the chain per group).
 * LDS counters, integer atomics only: the same chain gives the same integers.  No workspace; BISIP_EUNSUPPORTED
 * when the edges and counters of the parameters (1-D) or of a single pair (2-D: bins up to ~125) exceed 64 KiB of LDS.
 * Any number of values per call (64-bit offsets).  Asynchronous on stream, no host synchronisation. */
int bisip_chain_range_dev(const double *d_chain, int64_t n_samples, int64_t sample_stride, int64_t n_ensembles,
                          int64_t walkers_per_ensemble, int ndim, double *d_out, int64_t *d_nonfinite, void *stream);
int bisip_chain_histograms_dev(const double *d_chain, int64_t n_samples, int64_t sample_stride, int64_t n_ensembles,
                               int64_t walkers_per_ensemble, int ndim, const double *d_edges, int bins,
                               int64_t *d_counts, void *stream);
int bisip_chain_pair_histograms_dev(const double *d_chain, int64_t n_samples, int64_t sample_stride,
                                    int64_t n_ensembles, int64_t walkers_per_ensemble, int ndim, const double *d_edges,
                                    int bins, int64_t *d_counts, void *stream);

/* Per-step walker statistics of a chain resident in device memory -- the trace that the reference's plot_traces
 * (src/bisip/plotlib.py:17-54) draws as one line per walker, reduced along the walker axis: for every used sample s,
 * ensemble e and parameter q the percentiles and the mean of the walkers_per_ensemble values the ensemble holds at that
 * sample.  Chain layout, d_chain / sample_stride conventions as for bisip_chain_moments_dev; ndim 1 ... BISIP_MAX_NDIM
 * (ndim = 1: a stored log-probability tensor (n_samples, walkers)).  percentiles: host array in [0, 100] with 0 ... 8
 * entries, passed by value (no upload, no wait).
 *   d_pct (n_percentiles, n_samples, n_ensembles, ndim): np.percentile of the Wp values, the same double -- order
 *     statistics floor((Wp-1) p/100) and the next, numpy's _lerp (t >= 0.5 ? y - d (1-t) : x + d t); NaN if any of the
 *     values is NaN.  Not touched when n_percentiles = 0.
 *   d_mean (n_samples, n_ensembles, ndim) or NULL: their sum in a fixed order (value w goes to partial sum w mod 64, the 64
 *     partial sums are added pairwise 32, 16, ... 1 apart) divided by Wp.  No floating-point atomics: the same bits on
 *     every call.  Asking for neither is an error.
 * Ensembles of up to bisip_chain_trace_lds_walkers(ndim) walkers (the power of two whose padded columns fit the 64 KiB
 * of LDS a workgroup may allocate statically) are read once and sorted in LDS, one workgroup per (sample, ensemble) or
 * per group of small ensembles, and need no workspace.  Bigger ones go in slabs of samples through a column-major copy
 * and the selection kernel of bisip_columns_percentiles_dev: bisip_chain_trace_workspace() BYTES, at most 256 MiB or
 * one sample of the chain, whichever is larger (0: none needed; < 0: shape not supported).  The results do not depend on
 * the path.  Asynchronous on stream, no host synchronisation. */
int64_t bisip_chain_trace_workspace(int64_t n_samples, int64_t n_ensembles, int64_t walkers_per_ensemble, int ndim,
                                    int n_percentiles);
int bisip_chain_trace_lds_walkers(int ndim);
int bisip_chain_trace_dev(const double *d_chain, int64_t n_samples, int64_t sample_stride, int64_t n_ensembles,
                          int64_t walkers_per_ensemble, int ndim, const double *percentiles, int n_percentiles,
                          double *d_pct, double *d_mean, void *d_work, int64_t work_bytes, void *stream);

/* Per-walker moments along the STEP axis and the Gelman-Rubin potential scale reduction of a chain resident in device
 * memory (bisip_amd/convergence.py holds the definitions: walker_moments, gelman_rubin): which ensembles have converged
 * and which walkers are stuck, without moving the chain.  Walkers of an ensemble sampler are not independent chains:
 * R-hat here is a screening number beside the autocorrelation time, not a replacement for it.  Chain layout, d_chain /
 * sample_stride conventions as for bisip_chain_moments_dev; ndim 1 ... BISIP_MAX_NDIM (ndim = 1: a stored
 * log-probability tensor (n_samples, walkers)).  splits = 1: a chain is a walker's whole series, L = n_samples;
 * splits = 2: its first and its last L = n_samples / 2 samples are two chains (the middle sample of an odd n_samples is
 * in neither), which also shows drift.  BISIP_EINVAL when n_samples < 2 * splits or splits * walkers_per_ensemble < 2.
 *   d_mean, d_var (splits, n_ensembles, walkers_per_ensemble, ndim): mean and variance (ddof = 1) of every chain, from
 *     sums shifted by the chain's first sample c: d = x - c, S1 += d, S2 += d * d (product rounded on its own), in
 *     ascending sample order from 0.0; mean = c + S1 / L, var = (S2 - S1 * S1 / L) / (L - 1), 0 where that is negative.
 *     Short chains of few columns are cut into segments: want = max(1, 262144 / (splits * 256 * ceil(C / 256))), C =
 *     n_ensembles * walkers_per_ensemble * ndim; seg_len = max(32, ceil(L / want)); segment g sums samples [g * seg_len,
 *     (g + 1) * seg_len) of the half from 0.0 with the same c, and the segments' sums are added in ascending order.
 *   d_rhat (n_ensembles, ndim): over the M = splits * walkers_per_ensemble chains c = half * walkers_per_ensemble + w:
 *     sqrt((L - 1) / L + Bn / Wn), Wn = sum(var) / M, Bn = the variance (ddof = 1) of the means, from sums shifted by the
 *     mean of chain 0 as above.  Chain c goes to partial sum c mod 64, in turn; the 64 partial sums are added pairwise
 *     32, 16, ..., 1 apart.  IEEE: NaN when Wn and Bn are 0, inf when only Wn is; a NaN or +-inf in a chain makes its
 *     variance and the R-hat of that (ensemble, parameter) non-finite and nothing else.
 * Each of the three may be NULL, not all.  The chain is read once, coalesced.  d_work: bisip_chain_rhat_workspace()
 * BYTES (0: none needed -- n_ensembles >= 256 with splits * walkers_per_ensemble * ndim <= 4096 and one segment, a
 * survey; < 0: shape not supported), the segments' sums and the chain moments when the caller does not take them.  The
 * plan depends on the shape alone, never on the device.  No floating-point atomics: the same bits on every call
 * (convergence.ordered_rhat gives them in NumPy).  64-bit offsets.  Asynchronous on stream, no host synchronisation. */
int64_t bisip_chain_rhat_workspace(int64_t n_samples, int64_t n_ensembles, int64_t walkers_per_ensemble, int ndim,
                                   int splits);
int bisip_chain_rhat_dev(const double *d_chain, int64_t n_samples, int64_t sample_stride, int64_t n_ensembles,
                         int64_t walkers_per_ensemble, int ndim, int splits, double *d_mean, double *d_var,
                         double *d_rhat, void *d_work, int64_t work_bytes, void *stream);

/* Posterior covariance of every ensemble's used samples of a chain resident in device memory: np.cov(rows.T, ddof=1) of
 * the N = n_samples * walkers_per_ensemble rows that get_chain(discard, thin, flat=True) gives of the ensemble's walkers
 * (bisip_amd/covariance.py holds the definitions: flat_cov, corr_from_cov).  Chain layout, d_chain / sample_stride
 * conventions as for bisip_chain_moments_dev; ndim 1 ... BISIP_MAX_NDIM.  BISIP_EINVAL when N < 2.
 *   d_cov (n_ensembles, ndim, ndim), full and symmetric: [j, k] and [k, j] hold the same bits.  d_mean (n_ensembles,
 *   ndim), may be NULL.
 * One pass with shifted sums: c_j = parameter j of walker 0 of the ensemble's first used sample, d = x - c, S_j = sum d_j,
 * P_jk = sum d_j * d_k (the product rounded on its own, no fma), mean_j = c_j + S_j / N, cov_jk = (P_jk - (S_j * S_k) / N)
 * / (N - 1); a diagonal entry < 0 becomes 0, a NaN stays.  A NaN or +-inf in parameter j of an ensemble makes row and
 * column j of its matrix non-finite and nothing else.
 * Order of every sum.  Rows are numbered r = k * walkers_per_ensemble + w.  n_ensembles >= 256: one segment of N rows;
 * else want = 2048 / n_ensembles, seg_rows = max(1024, ceil(N / want)) (never above 2^30), nseg = ceil(N / seg_rows).
 * Row i of a segment goes to slot i mod T, T = 256 for ndim <= 8 and 64 above; a slot adds its rows in ascending order
 * from 0.0; the slots are added pairwise within each run of 64, 32, 16, ..., 1 apart, the four runs of T = 256 then in
 * ascending order; segments in ascending order.  d_work: bisip_chain_cov_workspace() BYTES (0: none needed, one segment;
 * < 0: shape not supported) for the segments' sums, 8-byte aligned.  The plan depends on the shape alone, never on the device.  No
 * floating-point atomics: the same bits on every call (covariance.ordered_cov gives them in NumPy).  The chain is read
 * once, whole 128-byte lines through LDS.  64-bit offsets.  Asynchronous on stream, no host synchronisation. */
int64_t bisip_chain_cov_workspace(int64_t n_samples, int64_t n_ensembles, int64_t walkers_per_ensemble, int ndim);
int bisip_chain_cov_dev(const double *d_chain, int64_t n_samples, int64_t sample_stride, int64_t n_ensembles,
                        int64_t walkers_per_ensemble, int ndim, double *d_mean, double *d_cov,
                        void *d_work, int64_t work_bytes, void *stream);

/* The stored sample of largest log-probability of every ensemble -- the maximum-a-posteriori point of the run.  d_chain /
 * chain_stride as above; d_logp (n_samples, n_ensembles * walkers_per_ensemble), sample k at d_logp + k * logp_stride.
 *   d_index (n_ensembles): np.argmax(np.where(np.isnan(lp), -np.inf, lp)) over the ensemble's values in the order k *
 *   walkers_per_ensemble + w: a NaN never wins, the lowest index wins among equals, 0 when all are NaN or -inf.
 *   d_best_logp (n_ensembles): the stored value at that index, bit for bit.  d_theta (n_ensembles, ndim): that sample.
 * Each of the three may be NULL, not all; d_chain may be NULL when d_theta is.  (value, index) pairs are compared, never
 * values alone: exact whatever the order.  n_ensembles >= 256: one segment; else seg_rows = max(4096, ceil(N / (2048 /
 * n_ensembles))).  d_work: bisip_chain_best_sample_workspace() BYTES (0: none needed; < 0: shape not supported), 8-byte aligned.
 * Asynchronous on stream, no host synchronisation. */
int64_t bisip_chain_best_sample_workspace(int64_t n_samples, int64_t n_ensembles, int64_t walkers_per_ensemble);
int bisip_chain_best_sample_dev(const double *d_chain, int64_t chain_stride, const double *d_logp, int64_t logp_stride,
                                int64_t n_samples, int64_t n_ensembles, int64_t walkers_per_ensemble, int ndim,
                                double *d_theta, double *d_best_logp, int64_t *d_index,
                                void *d_work, int64_t work_bytes, void *stream);

/* Highest-density intervals of every parameter, per ensemble, of a chain resident in device memory: the shortest interval
 * that holds a given share of each column's values (ArviZ's unimodal hdi; bisip_amd/interval.py holds the definition in
 * NumPy).  Chain layout, d_chain / sample_stride conventions as for bisip_chain_moments_dev (discard: an offset, thin: a
 * stride, padding allowed); ndim 1 ... BISIP_MAX_NDIM.  A column is one parameter of one ensemble over its N = n_samples *
 * walkers_per_ensemble values, numbered k * walkers_per_ensemble + w; s is the column sorted.  windows: host array
 * (n_windows,), 1 <= n_windows <= 8, of K = floor(mass * N) computed by the caller, each in [1, N - 1] (so N >= 2); M = N - K.
 *   width[i] = s[i + K] - s[i], i = 0 ... M - 1; a NaN width (inf - inf) is read as +inf; i* = the lowest i of smallest
 *   width; the interval is (s[i*], s[i* + K]).  A column that holds a NaN gives (NaN, NaN) and i* = 0.
 *   d_out (n_windows, 2, n_ensembles, ndim): lower ends, then upper ends.  d_index (n_windows, n_ensembles, ndim): i*, may
 *   be NULL.
 * Subtractions and comparisons of the same doubles as the definition: equal results (the sign of a zero is not pinned).
 * Two paths, the same results.  full: the columns are gathered, all sorted (segmented radix sort), and one workgroup per
 * (column, window) takes the argmin over (width, i).  tails: only s[0 .. M-1] and s[K .. N-1] are ever read, so the order
 * statistics a = s[M-1] and b = s[K] of every column are selected without a sort, per window the values < a and > b are
 * compacted into two buffers of M (open slots take the threshold: equal doubles), and only these 2 x columns segments of M
 * are sorted.  Path rule, from the shape and the windows alone: tails when N >= 4096 and every window has 8 * M <= N (and
 * 2 * columns * max M < 2^31), else full; the environment variable BISIP_HDI_PATH=full|tails, read on every call by both
 * functions, forces one.  Measured on an MI355X (benchmarks/interval_bench.py, medians of 5, the
 * paths alternating; profiles/r05_interval_bench.jsonl): 512 ensembles x 128,000 values x 7, mass 0.95 (M = N / 20): tails
 * 8.0 ms, full 34.6 ms (the parent's gather + sort of everything: 31.0 ms); masses (0.5, 0.9, 0.95) in one call (M = N / 2, N /
 * 10, N / 20): tails 50.0 ms, full 35.5 ms; seven columns of 160,000: 0.51 against 5.4 ms, and 4.1 against 5.5 ms.  The rule
 * lies between the two measured points, on the safe side: the tails never run where they were measured slower.
 * d_work: bisip_chain_hdi_workspace() BYTES (< 0: shape or windows refused; more than 2^31 values: the sort's limit), with
 * c = align256(8 * N * columns), columns = n_ensembles * ndim, t = align256(8 * 2 * columns * max M):
 *   full: 2 c + scratch(N * columns, columns);  tails: c + align256(16 * n_windows * columns) + align256(8 * columns) +
 *   align256(4 * columns) + 2 t + scratch(2 * columns * max M, 2 * columns); scratch(items, segments) = align256(align256(8 *
 *   items) + 16 * segments + 65536), a bound on what the library's segmented sort asks for (BISIP_EUNSUPPORTED if it ever
 *   asks for more): the workspace is sized without a device.
 * Asynchronous on stream, no host synchronisation. */
int64_t bisip_chain_hdi_workspace(int64_t n_samples, int64_t n_ensembles, int64_t walkers_per_ensemble, int ndim,
                                  int n_windows, const int64_t *windows);
int bisip_chain_hdi_dev(const double *d_chain, int64_t n_samples, int64_t sample_stride, int64_t n_ensembles,
                        int64_t walkers_per_ensemble, int ndim, const int64_t *windows, int n_windows, double *d_out,
                        int64_t *d_index, void *d_work, int64_t work_bytes, void *stream);

/* Effective sample size of every (ensemble, parameter) of a chain resident in device memory: the estimator of Vehtari,
 * Gelman, Simpson, Carpenter and Buerkner (2021) as Stan and ArviZ compute it (bisip_amd/ess.py holds the definition in
 * NumPy: ess_of_chains).  Walkers of an ensemble sampler are not independent chains: the between-chain term is a
 * screening device, as R-hat is.  Chain layout, d_chain / sample_stride conventions as for bisip_chain_moments_dev
 * (discard: an offset, thin: a stride, padding allowed); ndim 1 ... BISIP_MAX_NDIM (ndim = 1: a stored log-probability).
 * splits = 1: a chain is a walker's whole series, L = n_samples; splits = 2: its first and its last L = n_samples / 2
 * samples are two chains (the middle sample of an odd n_samples is in neither).  M = splits * walkers_per_ensemble chains
 * c = half * walkers_per_ensemble + w, S = L * M.  BISIP_EINVAL when n_samples < 2 * splits.
 *   d_threshold == NULL (n_threshold = 0): the series are the values; d_ess (n_ensembles, ndim).
 *   d_threshold (n_threshold, n_ensembles, ndim), 1 <= n_threshold <= 8: the series are the indicators x <= thr ? 1.0 :
 *     0.0, taken on load; d_ess (n_threshold, n_ensembles, ndim).  A NaN threshold gives NaN.
 *   Per (threshold, ensemble, parameter): NaN when a value of its chains is not finite; S when max - min < 1e-15; else with
 *   y = series - its chain's mean (the mean from sums shifted by the chain's first sample: a constant chain is centred to
 *   exact zeros), abar_k = sum over the chains of sum_{t < L - k} y_t y_{t + k} (pairs inside the half, fma), / L / M;
 *   mean_var = abar_0 L / (L - 1); var_plus = abar_0 + the variance (ddof = 1, two passes) of the chain means when M > 1;
 *   rho_k = 1 - (mean_var - abar_k) / var_plus; Geyer's initial positive sequence over pairs (rho_{t+1}, rho_{t+2}), t = 1,
 *   3, ... while t < L - 3 and the pair consumed last sums to > 0; the initial monotone sequence (a pair whose sum
 *   exceeds its predecessor's becomes twice that one's mean) and tau = -1 + 2 sum_{k <= max_t} rho_k + rho_{max_t + 1}
 *   are taken pair by pair on the way, so no rho is stored; tau >= 1 / log10(S); ESS = S / tau.
 * Work: the lag sums go in rounds of Lr = 64 * min(ceil(L / 64), max(1, ceil(512 / (tiles * n_series)))) lags, tiles =
 * ceil(C / 64), C = n_ensembles * walkers_per_ensemble * ndim, n_series = max(1, n_threshold) * splits: (tile of 64 series)
 * x (block of 64 lags) workgroups, the centred samples through LDS, 16 lag accumulators per lane; the round's sums are
 * added over the chains in groups of 256, groups in ascending order; one wave per (threshold, ensemble, parameter)
 * continues the sequence and marks it done when it ends; tiles whose sequences are all done leave later rounds at once.
 * d_work: bisip_chain_ess_workspace() BYTES (0: shape not supported): three doubles per series, Lr doubles per series
 * and per (pair, chain group), the scan's state.  The plan depends on the shape alone.  No floating-point atomics: the
 * same bits on every call.  64-bit offsets.  Asynchronous on stream, no host synchronisation between rounds. */
int64_t bisip_chain_ess_workspace(int64_t n_samples, int64_t n_ensembles, int64_t walkers_per_ensemble, int ndim,
                                  int splits, int n_threshold);
int bisip_chain_ess_dev(const double *d_chain, int64_t n_samples, int64_t sample_stride, int64_t n_ensembles,
                        int64_t walkers_per_ensemble, int ndim, int splits, const double *d_threshold, int n_threshold,
                        double *d_ess, void *d_work, int64_t work_bytes, void *stream);

/* The same of the squares about a centre: bisip_chain_ess_dev on the series (x - c) * (x - c), c = d_center[e, q]
 * (n_ensembles, ndim), taken on load as the indicators are -- one subtraction and one multiplication, each rounded -- so
 * the bits are those of bisip_chain_ess_dev on a stored chain of these squares.  d_ess (n_ensembles, ndim): the effective
 * sample size that the standard deviation's Monte-Carlo error is taken with (bisip_amd/diagnostics.py: ess_sd).  A
 * centre that is NaN gives NaN (as does one that is infinite: every square is).  Everything else, the checks and the
 * work included, as for bisip_chain_ess_dev without thresholds; d_work: bisip_chain_ess_workspace(..., n_threshold = 0). */
int bisip_chain_ess_squares_dev(const double *d_chain, int64_t n_samples, int64_t sample_stride, int64_t n_ensembles,
                                int64_t walkers_per_ensemble, int ndim, int splits, const double *d_center, double *d_ess,
                                void *d_work, int64_t work_bytes, void *stream);

/* Rank-normalisation of a chain resident in device memory, what the bulk effective sample size is taken of
 * (bisip_amd/ess.py: z_scale).  Chain layout, d_chain / sample_stride conventions as above.  Per (ensemble, parameter)
 * the N = n_samples * walkers_per_ensemble values are ranked from 1, ties sharing the mean of their ranks (-0.0 and 0.0
 * are equal), and z = ndtri((r - 3 / 8) / (N + 1 / 4)) with Wichura's AS 241 routine PPND16 in double, in the order of
 * operations of the definition.  d_z (n_samples, n_ensembles * walkers_per_ensemble, ndim), contiguous, in the order of
 * the chain.  A value that is not finite makes every z of its (ensemble, parameter) NaN and no other.
 * The columns are gathered and sorted (the library's segmented radix sort: n_ensembles * N * ndim < 2^31 values, else
 * BISIP_EUNSUPPORTED -- the caller goes in passes of ensembles), then one thread per chain element finds, by two binary
 * searches of its sorted column, how many values are smaller and how many are not larger: no index goes through the sort.
 * d_work: bisip_chain_rank_normalize_workspace() BYTES (0: shape not supported) = 2 align256(8 * items) +
 * scratch(items, n_ensembles * ndim), items = n_ensembles * N * ndim, scratch as for bisip_chain_hdi_workspace.
 * Asynchronous on stream, no host synchronisation. */
int64_t bisip_chain_rank_normalize_workspace(int64_t n_samples, int64_t n_ensembles, int64_t walkers_per_ensemble, int ndim);
int bisip_chain_rank_normalize_dev(const double *d_chain, int64_t n_samples, int64_t sample_stride, int64_t n_ensembles,
                                   int64_t walkers_per_ensemble, int ndim, double *d_z, void *d_work, int64_t work_bytes,
                                   void *stream);

/* The same of the folded values fabs(x - c), c = d_center[e, q] (n_ensembles, ndim; the median, for the folded R-hat of
 * bisip_amd/diagnostics.py: rank_rhat).  The fold is one IEEE subtraction and fabs, applied where a value is read: on the
 * gathered columns, in place, before the sort, and on the element before its two searches -- no chain-sized intermediate,
 * and the bits of bisip_chain_rank_normalize_dev on a stored chain of the folded values.  Same sort, same searches, same
 * PPND16.  A centre or a value that is not finite makes every z of its (ensemble, parameter) NaN and no other.
 * d_work: bisip_chain_rank_normalize_workspace() of the same shape.  The checks as for bisip_chain_rank_normalize_dev. */
int bisip_chain_rank_normalize_folded_dev(const double *d_chain, int64_t n_samples, int64_t sample_stride,
                                          int64_t n_ensembles, int64_t walkers_per_ensemble, int ndim,
                                          const double *d_center, double *d_z, void *d_work, int64_t work_bytes, void *stream);

/* np.percentile(rows, p, axis=0) for a device-resident (n_rows, n_cols) array (linear rule):
 * d_out (n_percentiles, n_cols).  Workspace in BYTES (0: more than 2^31 values). */
int64_t bisip_column_percentiles_workspace(int64_t n_rows, int n_cols, int n_percentiles);
int bisip_column_percentiles_dev(const double *d_rows, int64_t n_rows, int n_cols,
                                 const double *percentiles, int n_percentiles, double *d_out,
                                 void *d_work, int64_t work_bytes, void *stream);

/* np.percentile of n_columns contiguous columns of n values each (d_cols (n_columns, n): what
 * bisip_forward_columns_dev writes): d_out (n_percentiles, n_columns).  Selection of the order statistics,
 * no workspace, asynchronous on stream. */
int bisip_columns_percentiles_dev(const double *d_cols, int64_t n_columns, int64_t n, const double *percentiles,
                                  int n_percentiles, double *d_out, void *stream);

/* The same for n_groups stacked arrays (n_groups, n_rows, n_cols) in one sort: d_out
 * (n_percentiles, n_groups, n_cols) -- the model responses of many spectra's chains at once. */
int64_t bisip_grouped_percentiles_workspace(int64_t n_groups, int64_t n_rows, int n_cols, int n_percentiles);
int bisip_grouped_percentiles_dev(const double *d_rows, int64_t n_groups, int64_t n_rows, int n_cols,
                                  const double *percentiles, int n_percentiles, double *d_out,
                                  void *d_work, int64_t work_bytes, void *stream);

/* Percentiles of the MODEL response over a chain -- utils.get_model_percentile
 * (src/bisip/utils.py:17-35: a Python loop of forward() over the chain, then np.percentile
 * over axis 0) in one call: theta (W, ndim) host -> forward on the device -> per-(part,
 * frequency) percentiles on the device -> out (n_percentiles, 2, N) host.  Only theta goes up
 * and n_percentiles*2N doubles come back (the responses are written column by column and the order
 * statistics selected from the columns: the same doubles as np.percentile).  Single-spectrum contexts. */
int bisip_forward_percentiles(bisip_ctx *ctx, const double *theta, int64_t W,
                              const double *percentiles, int n_percentiles, double *out);
/* The same in the representation `kind` (BISIP_RESPONSE_*): PA gives np.percentile of the amplitude and of minus the
 * phase of every sample's response, out (n_percentiles, 2, N); RI the bits of bisip_forward_percentiles. */
int bisip_forward_percentiles_kind(bisip_ctx *ctx, const double *theta, int64_t W, const double *percentiles,
                                   int n_percentiles, int kind, double *out);

/* Mean and standard deviation (ddof = 0) of the MODEL RESPONSE over the used samples of a chain resident in device memory,
 * for n_spectra consecutive spectra of the context starting with first_spectrum: np.mean / np.std over axis 0 of forward
 * (kind RI) or of its amplitude and minus phase (kind PA) of the R = n_samples * walkers_per_ensemble rows that
 * get_chain(discard, thin, flat=True) gives of each spectrum's walkers (bisip_amd/response.py holds the definitions:
 * response_pa, response_moments).  Fused: the chain is read where it lies, the model evaluated in registers; no response
 * is written to memory.
 *   d_chain: walker 0 of spectrum first_spectrum in the first used sample; sample k at d_chain + k * sample_stride
 *   (doubles), row (e * walkers_per_ensemble + w) * ndim of it belongs to walker w of spectrum first_spectrum + e --
 *   discard / thin are a pointer offset and a stride multiple, as for bisip_chain_moments_dev.
 *   d_mean, d_std (n_spectra, 2, N) each; either may be NULL, not both.
 * One pass with shifted sums per (part, frequency): c = the response of walker 0 of the spectrum's first used sample,
 * d = x - c, S = sum d, P = sum d * d (the product rounded on its own, no fma), mean = c + S / R, var = (P - (S * S) / R)
 * / R with < 0 -> 0 (a NaN stays), std = sqrt(var).  A row with a parameter that is not finite counts as NaN: it makes
 * the means and stds of ITS spectrum non-finite and no other spectrum's.
 * Order of every sum.  Rows are numbered r = k * walkers_per_ensemble + w.  n_spectra >= 256: one segment of R rows;
 * else want = 2048 / n_spectra, seg_rows = max(1024, ceil(R / want)) (never above 2^30), nseg = ceil(R / seg_rows).  A
 * workgroup of 256 threads takes one (spectrum, segment): row i of the segment goes to slot i mod 256; a slot adds its
 * rows in ascending order from 0.0; the slots are added pairwise within each run of 64, 32, 16, ..., 1 apart, the four
 * runs then in ascending order; segments in ascending order.  (The frequencies go in tiles of 8, each a pass over the
 * segment's rows: 32 running sums per lane; the tiling changes no sum.)  d_work:
 * bisip_response_moments_workspace() BYTES (0: none needed, one segment; < 0: shape not supported) for the segments'
 * sums and the shifts, 8-byte aligned.  The plan depends on the shape alone, never on the device.  No floating-point
 * atomics: the same bits on every call (response.ordered_response_moments gives them in NumPy from the same responses).
 * 64-bit offsets.  Asynchronous on stream, no host synchronisation.  BISIP_EINVAL for an unknown kind. */
int64_t bisip_response_moments_workspace(bisip_ctx *ctx, int64_t n_samples, int64_t n_spectra, int64_t walkers_per_ensemble);
int bisip_response_moments_dev(bisip_ctx *ctx, int64_t first_spectrum, int64_t n_spectra, const double *d_chain,
                               int64_t n_samples, int64_t sample_stride, int64_t walkers_per_ensemble, int kind,
                               double *d_mean, double *d_std, void *d_work, int64_t work_bytes, void *stream);

/* FIT QUALITY per data point (Re and Im at each frequency) over the used samples of a chain resident in device memory:
 * with q = (y - Z)^2 * iv of a row -- y the normalised measurement, Z = forward(row), iv the context's inverse variance
 * (the record's rec[0..3]); d = y - Z, t = d * d, q = t * iv, each rounded on its own --
 *   d_mean_q = mean of q over the R rows (near 1: the point is fitted to its error bar),
 *   d_var_q  = variance of q with ddof = 1 (R = 1: NaN),
 *   d_lmeh   = log(mean(exp(-q / 2))), evaluated as -m / 2 + log(mean(exp(-(q - m) / 2))), m = min q,
 * (n_spectra, 2, N) each; any may be NULL, not all three.  WAIC and the per-point misfit are made of these
 * (bisip_amd/fitquality.py holds the definitions: pointwise_q, fit_sums, waic).  Chain layout, d_chain, first_spectrum,
 * argument checks and error codes: those of bisip_response_moments_dev; fused in the same way, nothing but the outputs is
 * written.  A row with a parameter that is not finite counts as q = NaN: it makes the three outputs of ITS spectrum NaN
 * at every point and no other spectrum's.
 * Order.  Segments and row slots are those of bisip_response_moments_dev (the same plan; a slot takes its rows in
 * ascending order; slots pairwise within each run of 64, 32, 16, ..., 1 apart, the four runs then in ascending order;
 * segments in ascending order).  mean_q, var_q: shifted sums, c = q of walker 0 of the spectrum's first used sample,
 * d = q - c, S = sum d, P = sum d * d (the product rounded on its own), mean_q = c + S / R, var_q = (P - (S * S) / R) /
 * (R - 1) with < 0 -> 0 (a NaN stays).  lmeh: every slot keeps (m, s), empty (+inf, 0); a row q >= m gives s = s +
 * exp(-(q - m) / 2), a row q < m gives s = s * exp(-(m - q) / 2) + 1, m = q (one exp per row, nothing fused); two pairs
 * merge to m' = min(m_a, m_b), the side with the larger m scaled by exp(-(m - m') / 2), the other (both, when equal)
 * not, s' = s_a + s_b, along the same tree as the sums; lmeh = -m / 2 + log(s / R).  exp and log are the device
 * library's.  (The frequencies go in tiles of 4, each a pass over the segment's rows: 32 doubles of state per lane; the
 * tiling changes no output.)  d_work: bisip_fit_quality_workspace() BYTES (0: none needed, one segment; < 0: shape not
 * supported) for the segments' states and the shifts, 8-byte aligned.  No floating-point atomics: the same bits on every
 * call (fitquality.ordered_fit_sums gives those of mean_q and var_q in NumPy from the same responses, and lmeh in the
 * same order with NumPy's exp).  64-bit offsets.  Asynchronous on stream, no host synchronisation. */
int64_t bisip_fit_quality_workspace(bisip_ctx *ctx, int64_t n_samples, int64_t n_spectra, int64_t walkers_per_ensemble);
int bisip_fit_quality_dev(bisip_ctx *ctx, int64_t first_spectrum, int64_t n_spectra, const double *d_chain,
                          int64_t n_samples, int64_t sample_stride, int64_t walkers_per_ensemble, double *d_mean_q,
                          double *d_var_q, double *d_lmeh, void *d_work, int64_t work_bytes, void *stream);

/* POSTERIOR PREDICTIVE CHECKS of every spectrum over the used samples of a chain resident in device memory
 * (bisip_amd/predictive.py holds the definitions: predictive_sums, predictive_check).  The noise is Gaussian with known
 * sigma, so every check is the mean over the R rows of a closed-form function of the row's residuals; no random numbers.
 * Per row and point, d = y - Z, t = d * d, q = t * iv as for bisip_fit_quality_dev; per row, T = sum of q (frequencies
 * ascending, Re before Im of each, from 0.0), qmax = max q and C = the adjacent frequency pairs, within Re and within Im,
 * whose d < 0 differs (0 ... 2N - 2).
 *   d_pit (n_spectra, 2, N)          = mean of Phi(d sqrt(iv)) = P(y_rep <= y | y) of the point, evaluated as erfc(-a) / 2
 *                                      with h = sqrt(iv / 2) correctly rounded (the halving is exact) and a = d * h,
 *   d_row (n_spectra, 3)             = chi2_mean = mean of T;  p_chi2 = mean of Q(N, T / 2), Q the regularised upper
 *                                      incomplete gamma function = P(chi2_2N >= T);  p_max = mean of
 *                                      -expm1(2N * log1p(-erfc(sqrt(qmax / 2)))) = P(max of 2N |eps| >= sqrt(qmax)),
 *   d_sign_changes (n_spectra, 2N-1) = the histogram of C (int64),
 * any may be NULL, not all three; an output not asked for stays untouched.  Q(N, x) = exp(-x) sum_{k < N} x^k / k! with
 * every term positive: x < N ascending from exp(-x), term = (term * x) / k; x >= N descending from
 * exp(((N - 1) log x - x) - log((N - 1)!)), term = (term * k) / x; a sum that rounds above 1 is 1; the host passes
 * log((N - 1)!), summed in long double.
 * Chain layout, d_chain, first_spectrum, argument checks, error codes and the alignment rule: those of
 * bisip_fit_quality_dev; fused in the same way, the model evaluated in registers, no response and no residual written.  A
 * row with a parameter that is not finite, or whose T is not finite, counts in no bin and makes d_pit and d_row of ITS
 * spectrum NaN and no other spectrum's: the bins of a spectrum add up to its good rows.
 * Order.  Segments and row slots are those of bisip_fit_quality_dev (the same plan; a slot takes its rows in ascending
 * order; slots pairwise within each run of 64, 32, 16, ..., 1 apart, the four runs then in ascending order; segments in
 * ascending order), plain sums from 0.0 (every term is in [0, 1] or >= 0: no shift), divided by R at the end; nothing is
 * fused.  The histogram: 32-bit integer atomics in LDS per workgroup, 64-bit integer atomics into the output, which the
 * entry point zeroes on the stream: any order gives the same counts.  No floating-point atomics: the same bits on every
 * call (predictive.ordered_predictive_sums gives those of chi2_mean and the counts in NumPy from the same responses, and
 * the others in the same order with glibc's functions).  exp, log, log1p, expm1, erfc are the device library's.  (The row
 * sums take one pass over the chain, pit a second in tiles of 8 frequencies; the tiling changes no output.)
 * d_work: bisip_predictive_check_workspace() BYTES (always > 0; < 0: shape not supported), the segments' sums, 8-byte
 * aligned.  BISIP_EUNSUPPORTED for d_row or d_sign_changes above N = 700, where exp(-x) underflows with x < N (d_pit alone
 * is served).  64-bit offsets.  Asynchronous on stream, no host synchronisation. */
int64_t bisip_predictive_check_workspace(bisip_ctx *ctx, int64_t n_samples, int64_t n_spectra, int64_t walkers_per_ensemble);
int bisip_predictive_check_dev(bisip_ctx *ctx, int64_t first_spectrum, int64_t n_spectra, const double *d_chain,
                               int64_t n_samples, int64_t sample_stride, int64_t walkers_per_ensemble, double *d_pit,
                               double *d_row, long long *d_sign_changes, void *d_work, int64_t work_bytes, void *stream);

/* The maximum a posteriori point before any chain exists: a multi-start Levenberg-Marquardt fit of the Gaussian misfit
 * inside the prior box, with a central-difference Jacobian (bisip_amd/mapfit.py holds the definitions: normal_equations,
 * lm_fit; csrc/lm_step.h the dense step).  The context's box must be finite (BISIP_EINVAL otherwise).  Per parameter j,
 * range_j = hi_j - lo_j: the stencil step is h_j = 1e-6 range_j and the inner box [lo_j + h_j, hi_j - h_j].
 *
 * bisip_gauss_newton_dev: the normal equations at S given points for each of n_spectra consecutive spectra starting with
 * first_spectrum, d_theta (n_spectra, S, ndim), taken as they are (not clipped).  y and iv = 1 / sigma^2 from the
 * frequency's record as for bisip_fit_quality_dev, Z the bits of bisip_forward:
 *   d = y - Z(theta);  dZ_j = (Z(theta + h_j e_j) - Z(theta - h_j e_j)) / (2 h_j);
 *   d_chi2 (n_spectra, S) = sum (d d) iv;  d_g (n_spectra, S, ndim): g_j = -sum (dZ_j d) iv;
 *   d_A (n_spectra, S, ndim, ndim): A_jk = sum (dZ_j dZ_k) iv;
 * every sum over the frequencies in ascending order, the real part before the imaginary one, from 0.0, every product and
 * sum rounded on its own (no fma): the bits of mapfit.ordered_normal_equations from bisip_forward's responses at the
 * 2 ndim + 1 stencil points.  A point with a parameter that is not finite gives NaN in its outputs and leaves the other
 * points alone.  Any output may be null (no stores).  n_spectra * S < 2^31.  Asynchronous on stream.
 *
 * bisip_map_fit_dev: the whole loop of mapfit.lm_fit from S starts per spectrum, d_starts (n_spectra, S, ndim), each
 * clipped into the inner box first; one launch, no host round trip.  lambda starts at 1e-3.  One iteration at theta:
 * the normal equations; parameter j is FIXED when theta_j is on the inner lower bound with g_j > 0 or on the inner upper
 * bound with g_j < 0, or when A_jj is 0 (its row, column and g_j are 0 then and its step is 0 either way), every other
 * is free; D = diag(A_ff) (no entry of it is 0, by the rule before); pred = g_f' A_ff^-1 g_f / 2 by Cholesky in the order csrc/lm_step.h
 * states (+inf when A_ff is not positive definite); status 0 (converged) when pred <= pred_tol; status 2 (cap) when
 * max_iter iterations are done (0 <= max_iter <= 1000); else the candidates lambda, 10 lambda, ..., at most 12, each
 * clip(theta + delta) onto the inner box with (A_ff + lambda D) delta = -g_f by Cholesky (a failed factorisation is a
 * rejected candidate); the first whose chi2 is finite and strictly lower becomes theta and lambda = max(its lambda / 10,
 * 1e-12); status 1 (stalled) when none is.  Outputs, per (spectrum, start), any may be null: d_theta (., ndim) the
 * result; d_chi2; d_logp = -chi2 / 2 + the spectrum's constant (-sum ln sigma^2), the log-probability there; d_pred;
 * d_A (., ndim, ndim) the Gauss-Newton Hessian there; d_iterations, d_status int64.  A start's result depends on nothing
 * but the start.  A start with a NaN ends stalled with NaN in theta and chi2.  Asynchronous on stream. */
int bisip_gauss_newton_dev(bisip_ctx *ctx, int64_t first_spectrum, int64_t n_spectra, const double *d_theta, int64_t S,
                           double *d_chi2, double *d_g, double *d_A, void *stream);
int bisip_map_fit_dev(bisip_ctx *ctx, int64_t first_spectrum, int64_t n_spectra, const double *d_starts, int64_t S,
                      int64_t max_iter, double pred_tol, double *d_theta, double *d_chi2, double *d_logp, double *d_pred,
                      double *d_A, int64_t *d_iterations, int64_t *d_status, void *stream);

/* Host-only, no GPU: the dense step of one iteration by the functions the kernel calls (csrc/lm_step.h), every pointer a
 * host pointer.  A (ndim, ndim), g, theta, lo, hi (ndim; the PRIOR box, the inner box is taken from it), 1 <= ndim <= 16.
 * fixed: bit j set where parameter j is fixed; pred as above; delta and trial (ndim) of the candidate with this lambda
 * (lambda <= 0: the undamped system), NaN when its factorisation failed, *ok = 0 then.  Any output may be null. */
int bisip_lm_step_host(int ndim, const double *A, const double *g, const double *theta, const double *lo, const double *hi,
                       double lambda, double *delta, double *trial, double *pred, int64_t *fixed, int *ok);

/* PSIS-LOO, step 1: the Re / Im columns that bisip_forward_columns_dev wrote for n_spectra consecutive spectra starting
 * with first_spectrum -- d_cols (n_spectra, 2N, rows_per_spectrum) -- become, where they lie, the squared standardised
 * residuals q = (y - Z)^2 * iv of their data point: y and iv from the frequency's record as for bisip_fit_quality_dev,
 * d = y - Z, t = d * d, q = t * iv, each rounded on its own (the bits of fitquality.pointwise_q).  Nothing is summed.
 * 64-bit offsets; asynchronous on stream. */
int bisip_q_columns_dev(bisip_ctx *ctx, int64_t first_spectrum, int64_t n_spectra, double *d_cols, int64_t rows_per_spectrum,
                        void *stream);

/* PSIS-LOO, step 2 (Vehtari, Simpson, Gelman, Yao & Gabry; bisip_amd/loo.py holds the definition: psis_loo_columns), no
 * context: d_q (columns, n) contiguous columns of n >= 2 values q, the log importance ratio of a value being q / 2.  Per
 * column, with s = sort(q), qmax = s[n - 1], u = s[n - tail_len - 1], r(x) = exp((x - qmax) / 2), eu = r(u): the tail is
 * the values > u, n_tail <= tail_len of them (ties at u stay in the body).  n_tail <= 4: khat = +inf, sigma = NaN, weights
 * w = r.  Else the generalised Pareto distribution is fitted to x = r(tail) - eu in ascending order (Zhang & Stephens with
 * the weakly informative prior: m = 30 + floor(sqrt(n_tail)) profile points b_j, k_j = mean(log1p(-b_j x)), L_j = n_tail
 * ((log(-b_j / k_j) - k_j) - 1), w_j = 1 / sum_i exp(L_i - L_j), b = sum b_j w_j, k = mean(log1p(-b x)), sigma = -k / b,
 * khat = k n_tail / (n_tail + 10) + 5 / (n_tail + 10); a khat that is not finite becomes +inf, sigma NaN and w = r) and the
 * tail's weights are w_i = min(eu + (sigma expm1(-khat log1p(-p_i))) / khat, 1), p_i = (i + 0.5) / n_tail.
 *   d_elpd_rel = (-qmax / 2 + log((n - n_tail) + sum_tail w / r)) - log(sum_body r + sum_tail w)   (unsmoothed: w / r is 1),
 *   d_khat, d_sigma, d_ntail (int64): (columns,) each; any may be NULL, not all four.
 * A column that holds a NaN gives NaN elpd_rel, khat and sigma and n_tail = 0, and touches no other column.
 * Order.  u and qmax are order statistics (the selection of bisip_columns_percentiles_dev, raw).  Body sum: the column in
 * chunks of 4096 values; value i of a chunk goes to slot i mod 256, a slot adds r of its values <= u in ascending order from
 * 0.0 (a value of the tail adds 0.0); slots pairwise within each run of 64, 32, 16, ..., 1 apart, the four runs then in
 * ascending order; chunks in ascending order.  The tail is sorted (one segmented sort of columns * tail_len values, open
 * slots padded with u).  Profile point j: x_i to slot i mod 64 in ascending order, slots pairwise 32 ... 1 apart.  The
 * softmax denominators and b: ascending.  k, sum w and sum w / r: element i to slot i mod 256 in ascending order, then the
 * tree of the body sum.  exp, log, log1p, expm1 are the device library's; nothing is fused.  No floating-point atomics
 * (integer atomics reserve the tail's slots; the sort removes their order): the same bits on every call
 * (loo.ordered_columns restates the order with NumPy's functions).  64-bit offsets.
 * d_work: bisip_loo_columns_workspace() BYTES (< 0: shape refused).  BISIP_EINVAL: null, n < 2, tail_len outside [1, n - 1],
 * short workspace; BISIP_EUNSUPPORTED: columns * tail_len > 2^31 - 1 (one sort), tail_len > 51,528 (256 profile points).
 * Asynchronous on stream, no host synchronisation. */
int64_t bisip_loo_columns_workspace(int64_t n, int64_t columns, int64_t tail_len);
int bisip_loo_columns_dev(const double *d_q, int64_t n, int64_t columns, int64_t tail_len, double *d_elpd_rel, double *d_khat,
                          double *d_sigma, int64_t *d_ntail, void *d_work, int64_t work_bytes, void *stream);

/* BRIDGE SAMPLING: the log marginal likelihood of every ensemble of a chain resident in device memory (Meng & Wong 1996 with a
 * multivariate-normal proposal, arranged as Gronau et al. 2017; bisip_amd/evidence.py holds the definitions: bridge_terms,
 * bridge_iterate, bridge_evidence).  Four steps, no context; the log-probability of the proposal's draws between the second
 * and the third is bisip_logprob_dev's.  The proposal of ensemble e: d_mean (n_ensembles, ndim), d_chol (n_ensembles, ndim,
 * ndim) the LOWER Cholesky factor L, row-major (the upper triangle is never read), d_const (n_ensembles) = c = sum_j log L_jj +
 * (ndim / 2) log(2 pi), taken by the caller.  log_g(x) = -0.5 sum_j z_j^2 - c with L z = x - mu.
 * All four: no workspace, no floating-point atomics (the same bits on every call), 64-bit offsets, asynchronous on stream,
 * no host synchronisation; BISIP_EINVAL and nothing written for a null pointer (d_f2, d_l2 excepted) or a shape out of range
 * (ndim outside 1 ... BISIP_MAX_NDIM, a count < 1, a stride smaller than one sample).
 *
 * Step 1: d_l (n_ensembles, N), N = n_samples * walkers_per_ensemble, column r = k * walkers_per_ensemble + w of ensemble e:
 * l = logp - log_g(x) of walker w of the ensemble in used sample k.  Chain layout, d_chain / sample_stride as for
 * bisip_chain_cov_dev; d_logp / logp_stride as for bisip_chain_best_sample_dev.  Order of every operation, each rounded once:
 * d_j = x_j - mu_j; acc = d_j, acc = fma(-L_jk, z_k, acc) for k = 0 ... j - 1 ascending, z_j = acc / L_jj; m = fma(z_j, z_j,
 * m) for j ascending from 0.0; log_g = fma(-0.5, m, -c); l = logp - log_g.  evidence.ordered_logg gives the same bits in
 * NumPy.  A logp or a parameter that is -inf, +inf or NaN propagates by IEEE to its own l and no other.  Rows are cut into
 * segments as bisip_chain_cov_dev cuts them and a tile of 256 rows is staged through LDS in whole lines; L and mu are read
 * once per workgroup; one lane takes one row.  No sum crosses a row: the cut changes no bit. */
int bisip_bridge_logg_dev(const double *d_chain, int64_t n_samples, int64_t sample_stride, int64_t n_ensembles,
                          int64_t walkers_per_ensemble, int ndim, const double *d_logp, int64_t logp_stride,
                          const double *d_mean, const double *d_chol, const double *d_const, double *d_l, void *stream);

/* Step 2: n_draws draws of every ensemble's proposal.  d_theta (n_ensembles * n_draws, ndim), rows [e * n_draws, (e + 1) *
 * n_draws) of ensemble e -- the row layout bisip_logprob_dev takes of a batch context -- and d_logg (n_ensembles * n_draws)
 * their log_g.  Draw i (numbered first_draw + i, 64 bits) of ensemble e takes its normal pair p = 0 ... ceil(ndim / 2) - 1 from
 * philox4x32_10(counter = (lo32(first_draw + i), hi32(first_draw + i), first_ensemble + e, 0x42520000 | p), key = (lo32(seed),
 * hi32(seed))) = (v0, v1, v2, v3): u0 = u53(v0, v1), u1 = u53(v2, v3) (53-bit uniforms in [0, 1)), rad = sqrt(-2 log(1 - u0)),
 * (z_2p, z_2p+1) = (rad * cospi(2 u1), rad * sinpi(2 u1)).  The samplers' streams keep counter word 3 in {0, 1, 2}: the domains
 * cannot meet.  theta_j = mu_j, theta_j = fma(L_jk, z_k, theta_j) for k = 0 ... j ascending; m = fma(z_j, z_j, m) for j
 * ascending from 0.0, log_g = fma(-0.5, m, -c).  A draw is a function of (seed, first_ensemble + e, first_draw + i) alone:
 * a call for draws [0, n) equals, bit for bit, calls for [0, k) and [k, n).  The integers are exact; log, sqrt and sincospi are
 * the device library's.  first_ensemble + n_ensembles <= 2^32, n_draws <= 2^40.  One lane per draw. */
int bisip_bridge_draw_dev(const double *d_mean, const double *d_chol, const double *d_const, int64_t n_ensembles, int ndim,
                          int64_t n_draws, uint64_t seed, uint64_t first_draw, int64_t first_ensemble, double *d_theta,
                          double *d_logg, void *stream);

/* Step 3, elementwise: with l2 = d_logp2 - d_logg2 (n_ensembles, n2) (the log-probability of the draws, -inf outside the prior
 * box, and their log_g) and d_l1 (n_ensembles, n1) of step 1,
 *   d_a1 (n_ensembles, n2) = exp(-(l2 - lstar_e)),   d_a2 (n_ensembles, n1) = exp(l1 - lstar_e),
 * lstar = d_lstar (n_ensembles).  d_l2 (n_ensembles, n2) takes l2 itself; it may be NULL and may be d_logp2 or d_logg2.  Each
 * subtraction and the negation are rounded on their own; exp is the device library's.  l2 = -inf gives a1 = +inf exactly; a NaN
 * stays a NaN. */
int bisip_bridge_scale_dev(const double *d_l1, int64_t n1, const double *d_logp2, const double *d_logg2, int64_t n2,
                           int64_t n_ensembles, const double *d_lstar, double *d_l2, double *d_a1, double *d_a2, void *stream);

/* Step 4: the iteration.  s1 = d_s1[e], s2 = 1 - s1; from r = 1:
 *   r' = (sum_i f1_i / n2) / (sum_j f2_j / n1),  f1_i = 1 / (s1 + (s2 * r) * a1_i),  f2_j = 1 / fma(s1, a2_j, s2 * r),
 * until |r' - r| <= tol * r' or maxiter passes (>= 1) are done.  A pass whose r' is not a positive finite number (a sum that is
 * not finite, a denominator of 0, every a1 = +inf) ends the ensemble there with r = NaN.  a1 = +inf and a2 = +inf contribute
 * exactly 0.  d_r (n_ensembles): the final r -- log_ml = log(r) + lstar is the caller's, the kernel takes no log;
 * d_iterations (n_ensembles, int64): passes done; d_moments (n_ensembles, 4): mean and population variance of f1, then of f2,
 * at the final r; d_f2 (n_ensembles, n1) or NULL: f2 at the final r.
 * Order.  One workgroup of 256 threads per ensemble loops on the device.  Term i of a sum goes to slot i mod 256; a slot adds
 * its terms in ascending order from 0.0; the slots are added pairwise within each run of 64, 32, 16, ..., 1 apart; the four runs
 * in ascending order; a mean is sum / double(count).  The variances are a second pass at the final r: d = f - mean, acc =
 * fma(d, d, acc) per slot, the same tree, / double(count).  Only + - * / and fma: evidence.ordered_iterate gives the same bits,
 * the pass count included. */
int bisip_bridge_iterate_dev(const double *d_a1, int64_t n2, const double *d_a2, int64_t n1, int64_t n_ensembles,
                             const double *d_s1, double tol, int64_t maxiter, double *d_r, int64_t *d_iterations,
                             double *d_moments, double *d_f2, void *stream);

/* Host: the stretch move's random stream in numpy.random.RandomState order for n_steps
 * iterations of a W-walker ensemble (the contract is bisip_amd/sampler.py:draw_step).
 * mt_key[624] / *mt_pos are RandomState.get_state()[1:3], advanced in place exactly as
 * NumPy would.  Outputs are (n_steps, 2, (W+1)/2): active and partner walker ids, stretch
 * factor zz and accept uniform u (the caller takes the logs). */
int bisip_numpy_stretch_stream(uint32_t *mt_key, int32_t *mt_pos, int64_t W, double a,
                               int64_t n_steps, int32_t *active, int32_t *partner, double *zz,
                               double *u);

/* Host, after the fact: how far are log-probabilities that a QR-reduced kernel produced from the
 * reduced form evaluated from the unrounded operands (in long double; in binary128 for a spectrum on the
 * compensated tier, whose operands come from a QR in binary128)?  theta (W, ndim) and logp (W,)
 * are host arrays -- typically a sampler's final ensemble and its log-probabilities (batch context:
 * the (E*Wp, ndim) layout of bisip_logprob).  *worst_rel = max |logp - reference| / max(1, |reference|)
 * over the rows inside the prior.  BISIP_VARIANT_AUTO picks a formulation from an ESTIMATE made on
 * probe rows when the context is created; this measures the same quantity where the walkers ended
 * up.  PolynomialDecomposition contexts only (BISIP_EUNSUPPORTED otherwise). */
int bisip_ctx_reduced_check(bisip_ctx *ctx, const double *theta, int64_t W, const double *logp, double *worst_rel);

/* bisip_logprob (the host-buffer entry emcee calls) measures the QR-reduced kernel it ran on up to 256
 * rows of the caller's own batch -- on a context's first call and every 2^n-th after it -- the way
 * bisip_ctx_reduced_check does.  Past 2e-11 a context on BISIP_VARIANT_AUTO moves to the next
 * formulation (compensated, then per-frequency) and evaluates the batch again with it; the choice holds
 * until bisip_ctx_set_bounds.  A caller-forced variant is measured and left alone.  enable: 1 / 0 turn
 * the guard on (default) / off, anything else leaves it; outputs (each may be NULL): checks made so far,
 * the worst relative error any of them saw, how many times the context changed formulation.
 * The device-pointer entry bisip_logprob_dev never synchronises and cannot guard itself: its callers hold
 * the rows and bring some of them to bisip_ctx_reduced_guard_rows (the device sampler does, chunk by chunk,
 * before it keeps a chunk).
 * The guard's findings are CONTEXT STATE: an escalation is remembered by the context, and every later launch on
 * it -- bisip_logprob_dev and the stretch-move entries included -- runs the formulation the guard moved to.  A
 * context that only ever sees device-pointer calls keeps the formulation its estimate chose; so a host-loop
 * sampler (guarded) and a device sampler on two contexts of the same spectrum may, after an escalation, run
 * different kernels (both within the tolerance the guard enforces; the chains then differ in the last bits).
 * bisip_logprob updates that state and the context's workspace: like every entry that takes a context it is
 * not re-entrant for ONE context (contexts are not shared across threads without locking). */
int bisip_ctx_reduced_guard(bisip_ctx *ctx, int enable, int64_t *n_checks, double *worst_rel, int *escalations);

/* The guard for callers whose rows live on the DEVICE (bisip_logprob_dev and the stretch-move entries never
 * synchronise, so they cannot measure themselves): the caller brings a few rows and the log-probabilities the
 * context's kernel gave them to the host -- the device sampler brings rows of its initial ensemble and, chunk by
 * chunk, the stored samples nearest to the shell logp = 0 (bisip_chain_shell_rows_dev), and does so BEFORE it
 * keeps a chunk -- and this call measures them as bisip_ctx_reduced_check does (rows outside the prior and NaN
 * rows are skipped; batch context: the (E*m, ndim) layout, m rows per spectrum).  *worst_rel: the measurement.
 * *escalated = 1: it was past 2e-11, the context runs on BISIP_VARIANT_AUTO and has just moved to the next
 * formulation, exactly as bisip_logprob's guard moves it -- the caller's log-probabilities of this and every
 * later row are stale: re-evaluate its state and re-run what it ran (the device sampler restores the chunk's
 * initial state and runs the chunk again: its random stream is counter-based or saved).  A caller-forced
 * variant, a context whose guard is off, or one that already runs the per-frequency form: measured (or not
 * at all), never moved.  PolynomialDecomposition contexts only (BISIP_EUNSUPPORTED otherwise). */
int bisip_ctx_reduced_guard_rows(bisip_ctx *ctx, const double *theta, int64_t W, const double *logp,
                                 double *worst_rel, int *escalated);

/* Per ensemble the k stored samples whose |log-probability| is smallest -- where the relative parity tolerance
 * max(1, |logp|) has denominator 1 and a kernel's absolute error shows -- of a chain resident in device memory:
 * d_chain (n_samples, n_ensembles*walkers_per_ensemble, ndim), d_logp (n_samples, n_ensembles*walkers_per_ensemble),
 * both contiguous.  d_out (n_ensembles, k + n_stride, ndim + 1): each row = a sample's theta followed by its
 * log-probability; slots no sample fills (fewer than k finite log-probabilities) are NaN rows.  Selection on
 * the bits of |logp| to 24 bits (exponent + 13 bits of mantissa): every sample nearer than the k-th is
 * there; of the samples that tie with the k-th to that resolution (1e-4 relative) the first to arrive fill the
 * remaining slots (ties != 0) or none does (ties == 0: the selected SET is then the same in every run and on
 * every rank of a sharded run, which therefore take the same decision from it with no collective).
 * n_stride > 0 (<= 256, <= walkers_per_ensemble) appends n_stride evenly spaced walkers of the FIRST sample.  d_work:
 * bisip_chain_shell_rows_workspace(n_ensembles) bytes.  Asynchronous on stream.  (No reference counterpart:
 * it serves the guard above; the run it guards is src/bisip/models.py:111-118.) */
int64_t bisip_chain_shell_rows_workspace(int64_t n_ensembles);
int bisip_chain_shell_rows_dev(const double *d_chain, const double *d_logp, int64_t n_samples, int64_t n_ensembles,
                               int64_t walkers_per_ensemble, int ndim, int k, int n_stride, int ties, double *d_out,
                               void *d_work, void *stream);

/* Sums and second moments of an ensemble's positions, shifted by walker 0: d_coords (W, ndim) device ->
 * d_out (ndim + ndim (ndim + 1) / 2) device = S_j = sum_i (x_ij - x_0j), then P_jk = sum_i (x_ij - x_0j)(x_ik - x_0k)
 * for k >= j, row by row.  What emcee's initial-state test -- the condition number of the centred, column-scaled
 * positions, raised inside emcee.EnsembleSampler.run_mcmc (src/bisip/models.py:111-118) -- needs of a big
 * ensemble that is on the device anyway: the host forms the centred Gram matrix P - S S^T / W and decides
 * (bisip_amd/sampler.py:walkers_independent); a NaN or an inf anywhere makes the sums non-finite.  ndim <= 8
 * (BISIP_EUNSUPPORTED beyond: the sums live in registers).  d_work: bisip_ensemble_gram_workspace() doubles.
 * Fixed summation order; asynchronous on stream. */
int64_t bisip_ensemble_gram_workspace(int64_t W, int ndim);
int bisip_ensemble_gram_dev(const double *d_coords, int64_t W, int ndim, double *d_out, double *d_work, void *stream);

/* Host: read n_files 5-column spectrum files (freq, amp, pha, amp_err, pha_err; comma separated,
 * `headers` lines skipped, '#' comments and blank lines ignored -- what the reference reads one
 * at a time with np.loadtxt(skiprows=headers, delimiter=','), src/bisip/utils.py:121-123) on
 * `threads` host threads (<= 0: as many as the process may use, at most 16) into tables
 * (n_files, n_rows, 5).  status[i] = 0: table i is filled
 * with exactly the doubles np.loadtxt yields; 1: file i is not in the plain format, cannot be
 * read, or does not hold n_rows rows -- read that one the reference's way (the Python host does,
 * so such files behave and fail as in the reference).  No GPU involved. */
int bisip_read_tables(const char *const *paths, int64_t n_files, int headers, int64_t n_rows,
                      double *tables, int32_t *status, int threads);

/* Host: one Philox4x32-10 block (counter[4], key[2]) -> out[4]; for known-answer tests. */
void bisip_philox4x32(const uint32_t *counter, const uint32_t *key, uint32_t *out);

/* Introspection */
int bisip_ctx_ndim(const bisip_ctx *ctx);
int bisip_ctx_nfreq(const bisip_ctx *ctx);
int bisip_ctx_device(const bisip_ctx *ctx);
/* Which loop the per-frequency models (ColeCole, Shin, Dias2000) run for the current prior box and frequencies; bits:
 *   1  shared reciprocals, exponents unclamped: the box keeps every denominator product normal (ColeCole with
 *      one or two modes, Shin and Dias2000: one reciprocal per pair of frequencies 2k, 2k+1 -- up to four
 *      denominators -- and a last unpaired frequency its own; ColeCole with three modes and more: one per group
 *      of up to four of a frequency's denominators);
 *   2  (only with 1; ColeCole up to three modes, Shin) geometric frequency grid: SOME spectrum's
 *      ln w_{16k+q} = ln w_{16k} + q*step (q < 16) to 4e-15 (bisip_frequency_grid_step), and every spectrum that is on
 *      such a grid takes its exponentials once per block of sixteen frequencies and steps them by multiplication
 *      (a batch decides per spectrum).  The environment variable BISIP_NO_GRID, read when a context is
 *      created, switches bit 2 off (measurement aid).
 * 0 for PolynomialDecomposition and for boxes widened past the limits. */
int bisip_ctx_loop_flags(const bisip_ctx *ctx);
/* Host-only: 1 and *step = the common step of ln w when w[0..N) is such a grid (N >= 8), else 0 and *step = 0. */
int bisip_frequency_grid_step(int N, const double *w, double *step);
/* Walker-independent part of the log-likelihood, -0.5*sum(2*ln(sigma^2)). */
double bisip_ctx_loglike_const(const bisip_ctx *ctx);
/* Name of the kernel bisip_logprob_dev launches for the current variant. */
const char *bisip_ctx_kernel_name(const bisip_ctx *ctx);
/* PolynomialDecomposition: worst relative log-probability error of the QR-reduced kernel for the
 * current prior box, estimated by emulating its double arithmetic on the host against long
 * double on ~200 probe rows per spectrum -- uniform in the box, clouds of small coefficients,
 * clouds around the least-squares solution and draws from the Gaussian posterior, the flat
 * valley where a sampler's walkers sit -- (0 for other models).  BISIP_VARIANT_AUTO runs the plain
 * reduced kernel while its estimate is <= 1e-12 (and 2N >= poly_deg+2), else the compensated one
 * while ITS estimate is <= 1e-12, else the collapsed form.  The value returned is the estimate of
 * the reduced kernel the current variant runs (or, when that is the collapsed form, of the better
 * of the two). */
double bisip_ctx_reduced_error(const bisip_ctx *ctx);

/* PolynomialDecomposition: how many spectra of the context run the plain (*n_plain) and the compensated
 * (*n_comp) QR-reduced kernel at the moment; both 0 when the per-frequency form runs.  A batch on
 * BISIP_VARIANT_AUTO decides per spectrum -- every spectrum runs what a context of its own would run, inside
 * one launch; a forced variant, and a batch whose mix bisip_logprob's guard closed, run one tier for all. */
int bisip_ctx_reduced_tiers(const bisip_ctx *ctx, int64_t *n_plain, int64_t *n_comp);

/* Host-only inspection of the walker-independent PolynomialDecomposition operands the
 * context precomputes (no GPU needed; used by the CPU-side tests).  Outputs:
 * G_re/G_im (N, P+1);  R (n,n) upper triangle row-major, bhat (n,), e (n,), rest (1,)
 * with n = P+2 (see BISIP_VARIANT_REDUCED);  lconst (1,) = -0.5*sum(2 ln sigma^2). */
int bisip_polydecomp_operands(int N, const double *w, const double *zn, const double *zn_err,
                              const bisip_model_desc *desc, double *G_re, double *G_im,
                              double *R, double *bhat, double *e, double *rest,
                              double *lconst);

/* Host-only: the error estimates behind BISIP_VARIANT_AUTO for one spectrum and prior box (what
 * bisip_ctx_reduced_error reports for a context): worst relative log-probability error of the
 * plain (est[0]) and the compensated (est[1]) QR-reduced kernel, from emulating their double
 * arithmetic against long double on the probe rows.  No GPU needed. */
int bisip_polydecomp_reduced_estimates(int N, const double *w, const double *zn, const double *zn_err,
                                       const bisip_model_desc *desc, const double *lo,
                                       const double *hi, double *est);

/* Measurement aid (no reference counterpart): ONE wavefront that reads the shader clock counter
 * (s_memtime) and the constant 100 MHz counter (s_memrealtime), idles for window_us and reads both
 * again; d_out (4 x int64, device) = shader ticks begin/end, 100 MHz ticks begin/end.  Enqueued on a
 * stream of its own beside a kernel under measurement it tells the engine clock the chip holds under
 * that kernel's load -- fp64-dense kernels run at 1.9-2.1 GHz, not at the 2.4 GHz the issue peak is
 * quoted at (benchmarks/micro/collapsed_r3.hip) -- without touching the kernel itself. */
int bisip_clock_probe_dev(int64_t *d_out, double window_us, void *stream);

/* Measurement aid (no reference counterpart): the rate a stream of INDEPENDENT fp64 FMAs reaches on this chip --
 * no dependency to wait for, no memory, 8 waves per SIMD on every compute unit, operands with full mantissas --
 * i.e. the ceiling a compute-bound log-probability kernel can be held to: 0.82-0.89 of the nominal
 * 1024 SIMDs x 2.4 GHz / 4 cycles with real data (the chip holds 2.2-2.3 GHz under it and a wave-instruction
 * takes 4.25-4.45 cycles; benchmarks/micro/fp64_stream_ceiling.hip).  One launch: every wave issues 32 * rounds
 * v_fma_f64; *wave_instructions (host, optional) = the launch's total.  d_out: bisip_fp64_stream_probe_lanes()
 * doubles on the device (written so that nothing is optimised away).  The caller times the launch. */
int64_t bisip_fp64_stream_probe_lanes(void);
int bisip_fp64_stream_probe_dev(double *d_out, int rounds, int64_t *wave_instructions, void *stream);

/* Host-only yardstick (no GPU, no prior): the PolynomialDecomposition log-likelihood
 * -0.5 (chi^2 + sum 2 ln sigma^2) of src/bisip/models.py:59-62 + cython_funcs.pyx:75-94 for W rows of theta,
 * from the QR-reduced form with NOTHING rounded to double on the way: kernel sums, Householder QR and
 * Q^T y in x87 long double, every row q_i - sum_j R_ij b_j accumulated as an unevaluated sum of two long
 * doubles.  Agrees with a 60-digit evaluation of the reference's per-frequency formula to ~1e-12 where
 * the reference's own double arithmetic is 1e-9 ... 1e-7 away (rows on the shell logp = 0 of degree 8-10
 * designs; tests/test_oracle_golden.py pins it with mpmath).  It is what bisip_ctx_reduced_check,
 * bisip_logprob's guard and the estimate behind BISIP_VARIANT_AUTO measure against.  Needs 2N >= poly_deg+2. */
int bisip_polydecomp_reduced_reference(int N, const double *w, const double *zn, const double *zn_err,
                                       const bisip_model_desc *desc, const double *theta, int64_t W, double *logp);

/* Host-only, no context, no GPU: what the QR-reduced kernels STORE for W rows of theta (W, n), bit for bit -- the
 * host emulation of their double arithmetic that the estimates behind BISIP_VARIANT_AUTO are measured on
 * (operation for operation; an fma is one rounding).  n = poly_deg + 2 (2 ... BISIP_MAX_POLY_DEG + 2); comp = 0:
 * the plain tier, 1: the compensated one.  Operands as a kernel holds them: R the packed upper triangle, row-major,
 * n (n + 1) / 2 doubles; Rlo its low word, as many floats (comp = 1 only; may be NULL otherwise, like elo);
 * bhat, e, elo (n,); rest; lconst; the prior box lo, hi (n,).  out[i] = -inf for a row outside the OPEN box (a NaN
 * or an on-bound value is outside), else fma(-0.5, chi^2, lconst) -- inf and NaN where the kernel's own sums
 * overflow.  tests/test_gpu_reduced_bits.py holds every instantiation and launch route of the kernels to it. */
int bisip_reduced_emulate(int n, int comp, const double *R, const float *Rlo, const double *bhat, const double *e,
                          const double *elo, double rest, double lconst, const double *lo, const double *hi,
                          const double *theta, int64_t W, double *out);

/* Host-only (reads the context, launches nothing, estimates nothing): the host copies of the operands the device
 * holds for spectrum `spectrum` of a PolynomialDecomposition context on QR-reduced tier `tier` (0 plain, 1
 * compensated) under the current prior box, in the layout bisip_reduced_emulate takes: R, Rlo (tier 1; may be NULL
 * for tier 0), bhat, e, elo, *rest and *lconst (the spectrum's own).  *runs = 1 when the context's present
 * effective variant sends this spectrum through this tier (a batch on BISIP_VARIANT_AUTO decides per spectrum),
 * else 0.  BISIP_EINVAL for another model, a bad index or tier, and a tier whose operands do not exist for that
 * spectrum under the current box (never asked for by a variant, or a batch spectrum that runs the other tier). */
int bisip_ctx_reduced_operands(const bisip_ctx *ctx, int64_t spectrum, int tier, double *R, float *Rlo, double *bhat,
                               double *e, double *elo, double *rest, double *lconst, int *runs);

int bisip_abi_version(void);
int bisip_device_count(void);
const char *bisip_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* BISIP_HIP_H */
