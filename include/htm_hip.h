/*
 * htm_hip.h -- C ABI of libhtm_hip.so: the MI355X (gfx950) implementation of HypoTremorMCMC's
 * per-proposal likelihood inner loop (step 5, `hypo_tremor_mcmc`).
 *
 * The reference has no FFI for this path: the boundary is the Fortran derived type `forward`
 * (reference src/cls_forward.f90:6-41) plus the chain bookkeeping of `mcmc` / `parallel`
 * (src/cls_mcmc.f90:7-53, src/cls_parallel.f90:7-22) driven by `program main`
 * (src/hypo_tremor_mcmc.f90:236-284).  Each entry point below names the reference interface it
 * replaces.  The Fortran ISO_C_BINDING module that re-creates `type forward` on top of these symbols is
 * hypotremormcmc_amd/fortran/cls_forward_hip.f90 over htm_c_api.f90 (shown in INTEGRATION.md).
 *
 * Conventions
 *   - plain C, no C++/torch types; every function returns 0 on success, a negative HTM_E* code otherwise;
 *     htm_last_error() gives the message of the last failure on the calling thread.
 *   - all floating-point data is IEEE fp64; integers are 32-bit unless stated.
 *   - 2-D observation arrays are (n_sta, n_events) column-major exactly as in the reference
 *     (src/cls_forward.f90:62-69): element (j, i) at [i * n_sta + j], station index fastest.
 *   - hypocentre vectors are xyz-interleaved, 3 * n_events long (src/cls_forward.f90:109-111).
 *   - event ids (evt_id) are 1-based like the reference.
 *   - host pointers unless a parameter name starts with d_ (device pointer, same device as the handle).
 *   - a handle is not thread-safe; calls are synchronous unless stated (the reference is single-threaded
 *     per rank with strictly synchronous calls).
 *   - there is NO CPU fallback: every entry point fails with HTM_ENODEVICE when no gfx950 device is usable.
 */
#ifndef HTM_HIP_H
#define HTM_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HTM_OK          0
#define HTM_EINVAL     -1   /* bad argument */
#define HTM_ENODEVICE  -2   /* no usable HIP device */
#define HTM_EHIP       -3   /* a HIP runtime call failed */
#define HTM_ESTATE     -4   /* call not valid in the handle's current state */
#define HTM_EOVERFLOW  -5   /* a record buffer overflowed (lock-step mode without drain) */
#define HTM_EDESYNC    -6   /* ranks disagree on the iteration number in the swap exchange */

typedef struct htm_forward htm_forward;
typedef struct htm_chains  htm_chains;

const char *htm_last_error(void);
int         htm_abi_version(void);          /* bumped when this header changes incompatibly */
int         htm_device_count(int *n);       /* number of visible HIP devices */
/* The GPU behind a device ordinal as (PCI domain << 16 | bus << 8 | device): the same number in every process that sees this
 * GPU, whatever ordinal HIP_VISIBLE_DEVICES / ROCR_VISIBLE_DEVICES gave it there -- what ranks compare to find out that they
 * share a GPU (htm_chains_share_gpu; the reference has one MPI rank per CPU core and no such notion, src/mod_mpi.f90). */
int         htm_device_physical_id(int device, int *id);

/* ------------------------------------------------------------------------------------------------
 * `type forward`                                                  reference: src/cls_forward.f90
 * ---------------------------------------------------------------------------------------------- */

/* constructor `forward(n_sta, n_events, sta_x, sta_y, sta_z, obs, use_amp, use_time)`  (:40-96).
 * `obs` is passed as its four arrays (what obs%get_t_obs() .. get_a_stdv() return, :71-74).  All inputs
 * are copied (the reference deep-copies too, :50-74); the missing-data rule of :76-92 is applied here. */
int htm_forward_create(int n_sta, int n_events,
                       const double *sta_x, const double *sta_y, const double *sta_z,
                       const double *t_obs, const double *t_stdv,
                       const double *a_obs, const double *a_stdv,
                       int use_time, int use_amp, int device, htm_forward **out);
int htm_forward_destroy(htm_forward *h);

/* fp32 forward / fp64 accept (BASELINE configs[4]; the reference is fp64 throughout, so this mode has no reference
 * counterpart and carries a STATISTICAL tolerance): forward_fp32 = 1 makes every kernel of this
 * handle compute the synthetic travel times / amplitudes (src/cls_forward.f90:115-118, :201-204 -- distance, sqrt,
 * division, log) in single precision and stream the observations as float (half the bytes of a full
 * evaluation); the weighted demean sums (:125-132), residuals, the misfit sum (:281-299) and the Metropolis
 * decision (src/cls_mcmc.f90:194-199) stay fp64.  n_sta <= 128.  Call before htm_chains_create. */
int htm_forward_set_precision(htm_forward *h, int forward_fp32);

/* Bytes of the packed per-event observation records this handle holds: built when a chain set that can run
 * the specialised chain master is created on the handle, one copy per forward precision used since; 0 otherwise. */
int htm_forward_obs_pack_bytes(htm_forward *h, int64_t *bytes);

/* Run all work of this handle (and of chain sets created from it) on the caller's HIP stream, e.g.
 * torch's current stream so that RCCL collectives enqueued by torch.distributed order with our kernels.
 * hip_stream is used as given: NULL is HIP's default (null) stream -- which is what torch's default
 * stream is.  htm_forward_reset_stream goes back to the handle's own non-blocking stream. */
int htm_forward_set_stream(htm_forward *h, void *hip_stream);
int htm_forward_reset_stream(htm_forward *h);

/* `calc_log_likelihood(hypo, t_corr, vs, a_corr, qs, log_likelihood)`  (:268-303) */
int htm_forward_loglik_full(htm_forward *h, const double *hypo, const double *t_corr, double vs,
                            const double *a_corr, double qs, double *log_likelihood);

/* `partially_update_log_likelihood(evt_id, hypo_old, log_likelihood_old, hypo, t_corr, vs, a_corr, qs,
 * log_likelihood)`  (:307-362).  Only event evt_id of hypo_old / hypo is read by the reference, so the two
 * models are passed as that event's xyz triplets. */
int htm_forward_loglik_partial(htm_forward *h, int evt_id, const double hypo_old_xyz[3],
                               double log_likelihood_old, const double hypo_xyz[3],
                               const double *t_corr, double vs, const double *a_corr, double qs,
                               double *log_likelihood);

/* `calc_travel_time` (:100-138) / `calc_amp` (:183-222): out arrays are (n_sta, n_events), demeaned */
int htm_forward_travel_time(htm_forward *h, const double *hypo, const double *t_corr, double vs,
                            double *t_syn);
int htm_forward_amp(htm_forward *h, const double *hypo, const double *a_corr, double qs, double vs,
                    double *a_syn);
/* `calc_travel_time_single` (:142-179) / `calc_amp_single` (:226-264): out arrays are n_sta long */
int htm_forward_travel_time_single(htm_forward *h, int evt_id, const double *hypo, const double *t_corr,
                                   double vs, double *t_syn);
int htm_forward_amp_single(htm_forward *h, int evt_id, const double *hypo, const double *a_corr,
                           double qs, double vs, double *a_syn);

/* Batched full evaluation: n_models independent (hypo, t_corr, vs, a_corr, qs) sets in ONE launch --
 * what a chain-parallel caller needs instead of n_models calls of :268-303.  Stacked model-major:
 * hypo [n_models][3E], t_corr/a_corr [n_models][S], vs/qs/out [n_models]. */
int htm_forward_loglik_full_batch(htm_forward *h, int n_models, const double *hypo, const double *t_corr,
                                  const double *vs, const double *a_corr, const double *qs,
                                  double *log_likelihood);
/* Same with every array already resident in HBM (device pointers).  Asynchronous on the handle's stream;
 * d_log_likelihood is valid after htm_forward_sync().  This is the kernel bench.py prices against the
 * HBM roofline. */
int htm_forward_loglik_full_batch_dev(htm_forward *h, int n_models, const double *d_hypo,
                                      const double *d_t_corr, const double *d_vs, const double *d_a_corr,
                                      const double *d_qs, double *d_log_likelihood);
int htm_forward_sync(htm_forward *h);

/* Wall-clock-free timing of the last htm_forward_loglik_full_batch_dev launches: brackets `reps`
 * launches with HIP events on the handle's stream and returns the average kernel time in microseconds. */
int htm_forward_time_full_batch_dev(htm_forward *h, int n_models, const double *d_hypo,
                                    const double *d_t_corr, const double *d_vs, const double *d_a_corr,
                                    const double *d_qs, double *d_log_likelihood, int reps,
                                    double *avg_us);

/* THE MAP GRID of htm_forward_locate* and htm_hypo_density*: grid9 = {x0, dx, nx, y0, dy, ny, z0, dz, nz}, nine doubles in host
 * memory, the counts as doubles with integral values.  Every axis {v0, dv, n} needs a finite origin v0, a finite cell size
 * dv > 0 and an integer n in 1..4096; anything else is HTM_EINVAL before any device call.  The centre of cell i of an axis is
 * v0 + (i + 0.5) * dv, one multiplication then one addition, unfused; the linear index of a cell is ix + nx (iy + ny iz). */

/* Location posteriors on a grid under a FIXED structure.  With t_corr, vs, a_corr, qs fixed the
 * log-likelihood of :268-303 is a sum of independent per-event terms; the term l of every event of the handle is taken at
 * every cell centre of grid9 (the map grid, above; and nx ny nz <= 2^31 - 1).  The handle's stations, observations, use_time / use_amp and missing-data
 * rule are used as they stand, always through its fp64 arrays (whatever htm_forward_set_precision says; the fp32 evaluation of these entry points is
 * htm_forward_locate_set_precision's, below).  t_corr, a_corr
 * [n_sta], host pointers.  prior5 [n_events][5] = {mu_x, mu_y, w_xy, z0, w_z} or NULL (flat prior): the log prior of a cell is
 * the sum of the normalised Gaussian log densities N(mu_x, w_xy), N(mu_y, w_xy) in x and y and of the normalised depth prior
 * of src/cls_model.f90:178-185, log(z - z0) - 2 log w_z - (z - z0)^2 / (2 w_z^2) for z > z0 and -inf otherwise.  The log
 * posterior of a cell is lp = l + log prior; a cell whose lp is NaN or -inf is EXCLUDED from everything below (a centre on a
 * station gives log 0 in the amplitude term, as in the reference).
 * loc [n_events][16] = the best cell's linear index (ties: the lowest; -1 when every cell is excluded, and then the other 15
 * are NaN), its centre x, y, z, lp there, l there, log(sum exp(lp) dx dy dz), the posterior mean x, y, z and the covariance
 * xx, xy, xz, yy, yz, zz under the weights exp(lp - lp_best) of the included cells.  marg [n_events][nx + ny + nz] or NULL: the
 * three axis marginals of those weights, each summing to 1 (NaN for an event without an included cell).  Sums of weights, the
 * log evidence, the mean (against sum_i m_i |x_i|) and the variances are good to 1e-12 relative; a mixed moment c_ij to
 * 1e-12 sd_i sd_j + 8 epsilon (X_i sd_j + X_j sd_i), X the largest |coordinate| of the axis (it is formed from row sums).  vol
 * [n_events][nz][ny][nx] or NULL: every cell's lp as computed, NaN and -inf kept.
 * NULL handle or output, vs or qs not finite or <= 0, a bad grid, w_xy or w_z <= 0: HTM_EINVAL before any device call.
 * Synchronous.  Every sum has a fixed order: two calls give the same bits.  The events go to the device in batches so that no
 * launch passes 2^32 - 1 work-items and the workspace, the device copy of vol included, stays under HTM_LOCATE_MB MiB
 * (environment, default 1024; one event at the least; what is counted: htm_forward_locate_plan, below); the result does not
 * depend on it. */
int htm_forward_locate(htm_forward *h, const double *t_corr, double vs, const double *a_corr, double qs,
                       const double *grid9, const double *prior5, double *loc, double *marg, double *vol);

/* The same with the structure MARGINALISED over n_draws draws of it: t_corr, a_corr [n_draws][n_sta], vs, qs
 * [n_draws], host pointers -- draws of p(structure | calibration data), e.g. thinned records of a calibration run's sample
 * files; 1 <= n_draws <= 4096.  The term of a cell is l = log((1 / n_draws) sum_k exp(l_k)), l_k the term htm_forward_locate
 * takes there under draw k, evaluated as m + (log(sum_k exp(l_k - m)) - log n_draws) with m the largest l_k: one draw gives l_1
 * itself, and the outputs of htm_forward_locate bit for bit; n equal draws give one draw's bits.  A cell where any l_k is NaN
 * is NaN (a centre on a station, under every draw); a draw with l_k = -inf has weight 0, and a cell where every draw has is
 * -inf.  lp = l + log prior, and everything from there on -- exclusion, loc (loc[5] is the marginalised l at the best cell),
 * marg, vol, their layouts and error bounds -- is htm_forward_locate's; a cell's l is good to 1e-12 of the largest sum of
 * absolute terms among its draws.
 * Refused with HTM_EINVAL before any device call: whatever htm_forward_locate refuses; n_draws outside 1..4096; a vs[k] or
 * qs[k] that is not finite or <= 0 (the message names the draw).  The table of the draws is part of the workspace under
 * HTM_LOCATE_MB (htm_forward_locate_plan): when it and one event do not fit, HTM_EINVAL names the variable.  Synchronous; every sum has a fixed order,
 * the draws are taken in their order: two calls give the same bits, and the bits do not depend on the batching. */
int htm_forward_locate_marginal(htm_forward *h, int n_draws, const double *t_corr, const double *vs, const double *a_corr,
                                const double *qs, const double *grid9, const double *prior5, double *loc, double *marg,
                                double *vol);

/* What every draw weighs for every window: the inputs of htm_forward_locate_marginal, and
 * log_z [n_events][n_draws]: log_z[e][k] is the log evidence htm_forward_locate returns in loc[6] for event e under draw k, the
 *   log of the sum of exp(lp) dx dy dz over the cells that are included UNDER THAT DRAW (a cell whose lp is NaN or -inf under
 *   draw k is left out of draw k); -inf when draw k leaves no cell.  It is good to 2e-12 A, A the largest sum of absolute terms
 *   of an included cell (1e-12 A a cell's value, as above; 1e-12 A the sums).
 * summary [n_events][4] or NULL = {n_eff, w_max, k_max, log_evidence}: with the normalised weights w_k = exp(log_z_k) / sum_k'
 *   exp(log_z_k'), the draws' effective number n_eff = 1 / sum_k w_k^2 (1 .. n_draws), the largest weight, the lowest index
 *   that has it, and log((1 / n_draws) sum_k exp(log_z_k)).  log_evidence equals htm_forward_locate_marginal's loc[6] to the same
 *   2e-12 A whenever a cell's NaN pattern is the same under all draws, which finite corrections always give.  An event with no
 *   included cell under any draw: log_z -inf throughout, n_eff, w_max, log_evidence NaN, k_max -1.
 * n equal draws give n equal columns bit for bit, n_eff == n_draws and w_max == 1 / n_draws exactly.  n_eff near 1 (w_max >
 * 0.5: one draw outweighs all the others together) says that the marginalised intervals of that window are one structure's:
 * n_draws was too small for it.
 * Refused with HTM_EINVAL before any device call: whatever htm_forward_locate_marginal refuses, with its messages, and a NULL
 * log_z.  The workspace of an event and the draws' table stay under HTM_LOCATE_MB as there (htm_forward_locate_plan), and when
 * the table and one event do not fit, HTM_EINVAL names the variable.  Synchronous; every sum has a fixed order and there are no
 * floating-point atomics: two calls give the same bits, and the bits do not depend on the batching. */
int htm_forward_locate_draw_evidence(htm_forward *h, int n_draws, const double *t_corr, const double *vs, const double *a_corr,
                                     const double *qs, const double *grid9, const double *prior5, double *log_z,
                                     double *summary);

/* SINGLE-PRECISION FORWARD of the three entry points above: forward_fp32 = 1 makes htm_forward_locate,
 * htm_forward_locate_marginal and htm_forward_locate_draw_evidence on this handle, and nothing else, form the synthetic travel
 * time and amplitude of a (cell, station) in fp32; 0 (a new handle's setting) is the fp64 arithmetic, bit for bit in every
 * output what a handle gives on which this was never called.  It is independent of htm_forward_set_precision, which governs
 * step 5's kernels only and leaves these entry points alone; there is no limit on n_sta.  The rule (event_misfit's fp32 rule
 * at a cell centre):
 *   - the three coordinate differences, cell centre minus station, are formed in fp64 and then rounded to float;
 *   - d = sqrt(fma(dz, dz, fma(dy, dy, dx dx))) in float, the hardware's v_sqrt_f32;
 *   - log2 d by the hardware's v_log_f32, once per (cell, station) whatever the number of draws;
 *   - per structure or draw, in float, from the float copies (round to nearest) of 1 / vs, pi f / (qs vs), t_corr and a_corr:
 *     the travel time fma(d, 1 / vs, -t_corr) and the amplitude fma(-d, pi f / (qs vs), -fma(log2 d, (float)ln 2, a_corr)) --
 *     ln d is folded into the draw's own fma and never formed by itself;
 *   - each synthetic is promoted to double BEFORE the observation is subtracted.
 * The observations and precisions (NOT rounded to float, unlike step 5's mode), the first station's shift, the shifted sums,
 * a cell's term and everything behind it -- prior, best cell, weights, reduces, marginals, moments, evidences, the
 * log-mean-exp over draws -- stay fp64.  Excluded cells keep their meaning (a centre on a station with amplitudes in use:
 * log2 0 = -inf, the term NaN); one draw still gives htm_forward_locate's very bits; two calls give the same bits, whatever
 * the batching.  A cell's term differs from the fp64 one by a few 2^-24 of sum_j precision_j |demeaned residual_j| scale_j,
 * scale_j the magnitude of the terms of station j's synthetic (tests/locate_fp32_restatement.py states and pins the bound).
 * NULL handle, or a value other than 0 or 1: HTM_EINVAL, and the setting stays as it was. */
int htm_forward_locate_set_precision(htm_forward *h, int forward_fp32);

/* STACKED DENSITY of the windows' grid posteriors: what htm_hypo_density is for the samples of step 5, for
 * windows that were located on the grid -- formed on the device, batch after batch; nothing of size n_events x cells crosses
 * to the host.  n_draws = 0: the fixed structure of htm_forward_locate (vs and qs point to one value each, t_corr, a_corr
 * [n_sta]); n_draws >= 1: the inputs of htm_forward_locate_marginal.  layer [n_events] gives every window its layer, or NULL
 * with n_layer == 1 (every window in layer 0).  THE RULE:
 *   - a window e whose layer L_e lies in 0 .. n_layer - 1 and that has an included cell puts the mass
 *     m_e(c) = exp(lp_e(c) - lp_best,e) * (1 / W_e) into cell c: the subtraction first (it is exact for the cells that matter),
 *     then the exponential, then the product with the reciprocal, which is formed once per window.  lp_e(c) and lp_best,e are
 *     the very numbers that the entry points above return in vol and loc[4]; W_e = sum_c exp(lp_e(c) - lp_best,e) is the
 *     weight sum as they form it for the marginals (good to 1e-12 relative), kept from that reduce, not recomputed from loc[6];
 *   - excluded cells (lp NaN or -inf) get nothing;
 *   - a window whose layer is outside 0 .. n_layer - 1 takes no part and is in nobody's tally, as in htm_hypo_density;
 *   - a window without an included cell (loc[0] = -1) is counted in tally[L][1] and adds nothing; every other window of the
 *     layer is counted in tally[L][0] and adds one unit of mass;
 *   - stack[L][c] is the sum of m_e(c) over the layer's windows in ascending event order, sequentially, starting from 0;
 *   - xy [n_layer][ny][nx] is the sum of the finished stack over iz, xz [n_layer][nz][nx] over iy, yz [n_layer][nz][ny] over
 *     ix, each in an order that depends on the grid alone.
 * stack [n_layer][nz][ny][nx] or NULL; tally [n_layer][2], doubles with integral values; xy, xz, yz and tally are required.
 * loc [n_events][16] and marg [n_events][nx + ny + nz] may be NULL; where given they are bit for bit what htm_forward_locate /
 * htm_forward_locate_marginal return.  A stacked cell is good to (2e-12 + n 2^-53) relative of the rule applied to vol and
 * loc[4], n the layer's windows; a layer's stack and each of its maps sum to tally[L][0] to (2e-12 + cells 2^-53) relative.
 * htm_forward_locate_set_precision applies: it changes lp, and the stack consumes lp.
 * No floating-point atomics: two calls give the same bits, and the bits do not depend on HTM_LOCATE_MB -- a cell's running
 * total goes through memory unchanged from one batch to the next.  The workspace per event of a batch holds the event's volume,
 * and the stacks, their maps, their tallies and the windows' layers are counted once per call (htm_forward_locate_plan).
 * Refused with HTM_EINVAL and a message before any device call, the outputs untouched: whatever those two entry points refuse;
 * n_layer < 1; layer == NULL with n_layer != 1; a NULL xy, xz, yz or tally; n_layer (cells + nx ny + nx nz + ny nz + 2) above
 * 2^31 - 1; the once-per-call part and one event not fitting under HTM_LOCATE_MB (the message names the variable).
 * Synchronous. */
int htm_forward_locate_stack(htm_forward *h, int n_draws, const double *t_corr, const double *vs, const double *a_corr,
                             const double *qs, const double *grid9, const double *prior5, const int *layer, int n_layer,
                             double *loc, double *marg, double *xy, double *xz, double *yz, double *stack, double *tally);

/* PER-STATION RESIDUALS, SOURCE TERMS AND FIT of every window under the fixed structure of htm_forward_locate:
 * how well a window fits where it was located, which stations disagree, and the two numbers that the forward model demeans away.
 * The arguments up to marg are htm_forward_locate's.  THE RULE, for event e, a data type d that the handle uses (t: travel
 * times, a: amplitudes), station j and cell c:
 *   - r_dj(c) is the synthetic minus the observation (src/cls_forward.f90:115-118, :201-204), p_dj the handle's precision (the
 *     missing-data rule as it stands: precision 1);
 *   - the OFFSET m_d(c) = sum_j p_dj r_dj(c) / sum_j p_dj, the reference's t_mean / a_mean (:125-132, :210-217): the
 *     precision-weighted mean time residual is an origin-time shift, and -m_a is the log source amplitude;
 *   - the RESIDUAL rho_dj(c) = m_d(c) - r_dj(c): the observation minus the demeaned synthetic, with the sign of :284 and :295;
 *   - chi2_d(c) = sum_j p_dj rho_dj(c)^2, formed in one pass from the shifted sums (u = r - r_0, r_0 the first station's):
 *     m = r_0 + (sum p u) / sum p, chi2 = sum p u^2 - (sum p u)^2 / sum p;
 *   - the posterior is the one the same call returns: the weights w(c) = exp(lp(c) - lp_best) on the included cells and 0 on the
 *     others, W their sum as the marginals' reduce forms it, the best cell loc[0];
 *   - a posterior mean is taken ABOUT THE BEST CELL, as the mean position is: mean(q) = q(best) + (sum_c w(c) (q(c) - q(best)))
 *     / W, so a posterior that sits in one cell gives q(best) exactly; the offset's variance from u = m(c) - m(best) as
 *     sum w u^2 / W - (sum w u / W)^2, floored at 0 before the square root;
 *   - an excluded cell contributes by selection, never by 0 * value: its residual may be NaN or infinite.
 * res [n_events][n_sta][4] = {rho_t(best), mean(rho_t), rho_a(best), mean(rho_a)} per station.
 * fit [n_events][10], per data type, time first: {m(best), mean(m), sd(m), chi2(best), mean(chi2)}; loc[5] equals
 *   -0.5 (chi2_t(best) + chi2_a(best)) - (the constants of :283-286 and :294-297) to htm_forward_locate's bound on a term.
 * A data type that the handle does not use gives NaN; an event without an included cell gives NaN throughout.  res, the two m
 * entries and the chi2 entries are good to 1e-12 of the sum of the absolute values of their terms; the variance to 1e-12 of itself
 * plus 8 epsilon Xbar sd, Xbar the posterior mean of |synthetic| + |observation| and their p-weighted means.
 * loc [n_events][16] and marg may be NULL; where given they are bit for bit what htm_forward_locate returns for the same
 * arguments and precision setting.  htm_forward_locate_set_precision applies: with fp32 set the posterior and the synthetics
 * inside the residuals come from the same single-precision forward; observations, precisions, offsets, sums and everything
 * behind them stay fp64.  A per-station posterior spread is not given: it needs m(c) while station j is in hand, a second
 * evaluation of every distance.  Draws of the structure are not taken.
 * Refused with HTM_EINVAL before any device call: whatever htm_forward_locate refuses, with its messages (a NULL loc is not
 * refused), and a NULL res or fit.  Synchronous.  Every sum has a fixed order and there are no floating-point atomics: two calls
 * give the same bits, and the bits do not depend on HTM_LOCATE_MB.  The workspace per event of a batch holds the event's volume
 * (htm_forward_locate_plan). */
int htm_forward_locate_residuals(htm_forward *h, const double *t_corr, double vs, const double *a_corr, double qs,
                                 const double *grid9, const double *prior5, double *loc, double *marg, double *res, double *fit);

/* A BOX OF ITS OWN PER EVENT: htm_forward_locate (n_draws == 0: vs and qs point to one value each, t_corr,
 * a_corr [n_sta]) or htm_forward_locate_marginal (1 <= n_draws <= 4096: their inputs) with every event on a grid of its own, in
 * one launch per batch -- the fine pass of a coarse-to-fine refinement, whose boxes the caller chooses.  origin3 [n_events][3],
 * host pointer, is ABSOLUTE: event e is evaluated on the grid {origin3[e][0], dx, nx, origin3[e][1], dy, ny, origin3[e][2], dz,
 * nz}, the cell sizes and counts grid9's.  grid9's own three origins must pass the map grid's checks and are otherwise not read.
 * THE RULE: for every event e, loc[e], marg[e] and vol[e] are bit for bit what htm_forward_locate (n_draws == 0) or
 * htm_forward_locate_marginal returns in row e for the same handle, structure, precision setting and prior, with that event's
 * grid as grid9.  So loc[e][0] is the cell's linear index WITHIN THE EVENT'S BOX, and loc[e][1..3] and [7..9] are absolute
 * coordinates; the prior's tables are made per event on that event's grid; a posterior is conditional on the event's box.
 * The origins travel with the batch: the result does not depend on HTM_LOCATE_MB, which counts 32 bytes more per event
 * (htm_forward_locate_plan, `boxes`).  htm_forward_locate_set_precision applies.  The evidences of the draws, the stack and the
 * residual pass take no boxes.
 * Refused with HTM_EINVAL and a message before any device call: whatever those two entry points refuse, with their texts; a
 * NULL origin3; an origin that is not finite (the message names the event and the axis).  Synchronous; every sum has a fixed
 * order and there are no floating-point atomics: two calls give the same bits. */
int htm_forward_locate_boxes(htm_forward *h, int n_draws, const double *t_corr, const double *vs, const double *a_corr,
                             const double *qs, const double *grid9, const double *origin3, const double *prior5,
                             double *loc, double *marg, double *vol);

/* THE WORKSPACE AND THE BATCHES of the six entry points above, worked out without a handle and without a device: what a call
 * of that shape would allocate and how many events it would send at a time, or the refusal it would meet, with the same code
 * and text.  HTM_LOCATE_MB is read from the environment as a call reads it.  The request names what a call says through its
 * arguments: `job` 0 htm_forward_locate, 1 htm_forward_locate_marginal, 2 htm_forward_locate_draw_evidence (n_draws 0 for
 * job 0, 1..4096 otherwise); `volume`: vol is asked for; `prior`: prior5 is given; n_layer >= 1: htm_forward_locate_stack
 * (jobs 0 and 1; 0: no stack) with `layer` given or not; forward_fp32: htm_forward_locate_set_precision's setting;
 * `residuals`: htm_forward_locate_residuals (job 0, without `volume` and without a stack); `boxes`: htm_forward_locate_boxes
 * (jobs 0 and 1 with or without `volume` and `prior`; without a stack and without `residuals`).
 * THE FORMULA, stated here once.  With cells = nx ny nz, n_marg = nx + ny + nz, rows = max(1, min(ny, 256, 4096 / nx)) x-rows
 * per tile, tpl = ceil(ny / rows) tiles per z-layer, n_tiles = nz tpl, stride = 4 + nx + 2 rows doubles per tile, Kpad = n_draws
 * padded to whole blocks of 8:
 *   per event of a batch, bytes:
 *     jobs 0, 1   8 (n_tiles stride + 16 + 2 n_marg + [cells: with vol, or stacked] + [1: stacked]) + 80 n_sta + 32
 *     job 2       8 (n_tiles Kpad 2 + n_draws + 4 + n_marg) + 80 n_sta + 32
 *     (the prior's n_marg is counted with a flat prior too, where nothing is allocated for it);
 *     with `residuals`, on top of job 0's:  8 (cells + 1 + (2 n_sta + 4) + n_rblk (2 n_sta + 6) + 4 n_sta + 10) -- the kept
 *     volume, the weight sum w, the residuals and sums at the best cell, the partial records of n_rblk = ceil(cells / 1024) blocks
 *     of cells, res and fit;
 *     with `boxes`, on top of job 0's or 1's:  8 * 4 -- the event's box origin x0, y0, z0 and one unused, two aligned pairs;
 *   the draws' table, once per call (jobs 1, 2):  P (n_sta + 1) Kpad + 8 (2 n_sta + 2) n_draws, a pair P = 16 bytes, 8 with
 *     forward_fp32;
 *   the stack, once per call:  8 n_layer (cells + nx ny + nx nz + ny nz + 2) + 4 n_events where `layer` is given.
 * nb, the events of a batch, is the smallest of n_events and nb_limit[0..3]: 65535 (a launch's grid), (2^32 - 1) / (256
 * n_tiles) -- with `residuals` (2^32 - 1) / (256 max(n_tiles, n_rblk)) -- and (2^32 - 257) / n_sta (the work-items of a launch), and floor((HTM_LOCATE_MB 2^20 - table - stack) / per event),
 * itself at most 65535; and 1 at the least.  len_*: the elements of every device array, per event of a batch (sta .. w) and
 * once per call (dtc .. layer), and the residuals' (rbase .. fit) and the boxes' (org) per event of a batch; 0: the call has no
 * such array.
 * HTM_EINVAL, in this order: a NULL argument or a request that no entry point makes; a bad grid; more than 2^31 - 1 cells;
 * HTM_LOCATE_MB not positive; the draws' table and one event above it; n_layer (cells + nx ny + nx nz + ny nz + 2) above
 * 2^31 - 1; the stack, the table and one event above HTM_LOCATE_MB.  (A call checks the prior's widths after the cells.) */
#define HTM_LOCATE_FIXED          0
#define HTM_LOCATE_MARGINAL       1
#define HTM_LOCATE_DRAW_EVIDENCE  2
typedef struct htm_locate_request {
    int32_t n_sta, n_events;
    int32_t job, n_draws;
    int32_t volume, prior;
    int32_t n_layer, layer;
    int32_t forward_fp32;
    int32_t residuals;                                /* htm_forward_locate_residuals (job 0, no volume, no stack) */
    int32_t boxes;                                    /* htm_forward_locate_boxes (jobs 0 and 1, no stack, no residuals) */
} htm_locate_request;
typedef struct htm_locate_plan {
    int64_t rows, tpl, stride;
    int64_t cells, n_tiles, n_marg, map_cells;        /* map_cells = nx ny + nx nz + ny nz */
    int64_t n_draws, n_draws_padded;
    int64_t len_sta, len_ev, len_part, len_logz, len_sum, len_loc, len_marg, len_prior, len_vol, len_w;
    int64_t len_dtc, len_dac, len_rk, len_corr, len_vq, len_stack, len_xy, len_xz, len_yz, len_tally, len_layer;
    double per_event_bytes, table_bytes, fixed_bytes;
    int64_t nb_limit[4];
    int64_t nb;
    int64_t len_rbase, len_rpart, len_res, len_fit;   /* per event of a batch, of a request with `residuals`; 0 otherwise */
    int64_t len_org;                                  /* per event of a batch, of a request with `boxes`: 4; 0 otherwise */
} htm_locate_plan;
int htm_forward_locate_plan(const htm_locate_request *request, const double *grid9, htm_locate_plan *plan);

/* ------------------------------------------------------------------------------------------------
 * Device-resident chains: `type mcmc` x n_chains inside `type parallel`
 *                          reference: src/cls_mcmc.f90, src/cls_parallel.f90, src/hypo_tremor_mcmc.f90
 * ---------------------------------------------------------------------------------------------- */

/* One `type model` (src/cls_model.f90:5-27) per parameter group, stacked chain-major.  Every pointer is
 * [n_chains][nx] with nx = 3*n_events (hypo), n_sta (t_corr, a_corr) or 1 (vs, qs).  mu/sigma/step_size/
 * prior_type may be NULL for a group that is never perturbed (solve_* = 0; the reference leaves them
 * unset too, src/hypo_tremor_mcmc.f90:133-137). */
typedef struct {
    const double  *x;
    const double  *mu;
    const double  *sigma;
    const double  *step_size;
    const int32_t *prior_type;   /* 0 Gaussian, 1 Rayleigh (src/cls_model.f90:9) */
} htm_model_init;

/* Most chains one rank holds (htm_chains_create refuses more).  Up to 32 a rank may run any of the main loops; 33..64 run
 * the loop with barriers (htm_chains_master_stats reports it). */
#define HTM_MAX_CHAINS 64

typedef struct {
    int            n_chains;      /* chains on this rank, 1..HTM_MAX_CHAINS (para%get_n_chains()) */
    int            n_procs;       /* ranks in the job               (mpi_comm_size)       */
    int            rank;          /* this rank                      (mpi_comm_rank)       */
    htm_model_init hypo, t_corr, vs, a_corr, qs;
    const double  *temp;          /* [n_chains] initial temperatures (src/hypo_tremor_mcmc.f90:202-208) */
    int            solve_vs, solve_t_corr, solve_qs, solve_a_corr;   /* -> proposal mix, src/cls_mcmc.f90:91-108 */
    uint32_t       rng_state[4];  /* mod_random's (x, y, z, w) after the rank's set-up draws */
    int            n_burn;        /* parameters are recorded only for i > n_burn (src/hypo_tremor_mcmc.f90:272) */
    int            n_interval;    /* record when mod(i, n_interval) == 1          (:271) */
    int            lik_capacity;  /* record-buffer sizes (records held on the device between drains); */
    int            sample_capacity; /* 0 = defaults */
} htm_chains_init;

int htm_chains_create(htm_forward *h, const htm_chains_init *init, htm_chains **out);
int htm_chains_destroy(htm_chains *hc);

/* Single-rank job (n_procs == 1): run n_iter iterations of the main loop
 * (src/hypo_tremor_mcmc.f90:236-284: propose -> forward -> judge per chain, then swap_temperature),
 * entirely on the device.  Synchronous; records are drained into host memory as needed. */
int htm_chains_run(htm_chains *hc, int n_iter);

/* Lock-step multi-rank iteration (n_procs >= 1).  step_begin enqueues propose -> forward -> judge for all
 * chains of this rank and fills this rank's swap record; the caller all-gathers the records of all ranks
 * (RCCL through torch.distributed, or MPI) into a device buffer [n_procs][record_bytes] and hands it to
 * step_end, which enqueues the temperature swap of src/cls_parallel.f90:100-216.  Nothing here blocks the
 * host; all work is stream-ordered. */
int htm_chains_step_begin(htm_chains *hc);
int htm_chains_swap_record(htm_chains *hc, void **d_record, size_t *record_bytes);
int htm_chains_step_end(htm_chains *hc, const void *d_gathered_records);
/* The same loop driven from C: n_iter lock-step iterations, each = step_begin + all-gather of the swap
 * records + step_end, all enqueued on the handle's stream without host synchronisation.  `allgather` has
 * ncclAllGather's signature (RCCL: pass &ncclAllGather and the rank's ncclComm_t; count is in elements of
 * dtype 8 = ncclFloat64); d_gathered must hold n_procs * record_bytes.  Returns the function's first
 * non-zero status as HTM_EHIP. */
typedef int (*htm_allgather_fn)(const void *sendbuff, void *recvbuff, size_t count, int dtype, void *comm,
                                void *stream);
int htm_chains_run_lockstep(htm_chains *hc, int n_iter, htm_allgather_fn allgather, void *comm,
                            void *d_gathered);
/* Host-staged form of the same exchange for MPI programs (the Fortran driver): after step_begin,
 * swap_record_host waits for the iteration and copies this rank's record (4 + 2*n_chains doubles) to host memory;
 * the caller all-gathers the records of all ranks (MPI_Allgather) and hands the n_procs records back with
 * step_end_host, which stages them in device memory.  Costs two small PCIe copies per iteration: a
 * compatibility path -- the RCCL path above keeps everything on the device. */
int htm_chains_swap_record_host(htm_chains *hc, double *record);
int htm_chains_step_end_host(htm_chains *hc, const double *gathered_records);
/* Persistent lock-step: the swap exchange of src/cls_parallel.f90:100-216 INSIDE the kernel.  Each rank owns an
 * inbox in its GPU's memory; a rank's kernel writes its swap record straight into every rank's inbox (peer-mapped
 * memory over xGMI, tagged 8-byte granules, system-scope stores) and polls its own -- no kernel boundary and no
 * collective per iteration, so the kernel stays resident over all iterations like the single-rank loop.
 *   xchg_handle   allocates the inbox and returns its IPC handle (HTM_XCHG_HANDLE_BYTES bytes);
 *   xchg_connect  takes the handles of ALL ranks in rank order (exchanged by the caller: MPI_Allgather, or
 *                 torch.distributed's all-gather over RCCL), `handle_bytes` apart, and maps the peers' inboxes
 *                 (n_procs == 1: handles may be NULL);
 *   xchg_probe    (optional, collective) a one-wave kernel writes a token into every rank's inbox and waits up to
 *                 `seconds` for all ranks' tokens in its own: proves at set-up that peer writes reach a polling kernel
 *                 (the call count of the set is part of the token: a repeated probe never passes on an earlier one's tokens);
 *   run_lockstep_direct  n_iter lock-step iterations; synchronous; every rank must call it with the same n_iter.
 * The transport-agnostic step_begin / step_end protocol above stays available (and is what a rank falls back to
 * when peer mapping is refused). */
#define HTM_XCHG_HANDLE_BYTES 64
int htm_chains_xchg_handle(htm_chains *hc, void *handle, size_t handle_bytes);
int htm_chains_xchg_connect(htm_chains *hc, const void *handles, size_t handle_bytes);
int htm_chains_xchg_probe(htm_chains *hc, unsigned token, double seconds);
int htm_chains_run_lockstep_direct(htm_chains *hc, int n_iter);
/* RCCL from a C / Fortran host (no Python): a communicator over librccl, bound at run time with dlopen (inside a
 * PyTorch process its copy is reused).  Rank 0 calls htm_comm_unique_id and broadcasts the HTM_COMM_ID_BYTES bytes
 * (MPI_Bcast in hypo_tremor_mcmc_hip_mpi); every rank then calls htm_comm_create (collective = ncclCommInitRank).
 * htm_chains_run_lockstep_comm = htm_chains_run_lockstep with ncclAllGather on that communicator: the swap of
 * src/cls_parallel.f90:100-216 as one RCCL all-gather per iteration, enqueued on the chains' stream without host
 * synchronisation.  htm_comm_allgather moves any bytes (e.g. the inboxes' IPC handles of the persistent lock-step).
 * RCCL wants one device per rank: two ranks on one GPU are refused by ncclCommInitRank. */
typedef struct htm_comm htm_comm;
#define HTM_COMM_ID_BYTES 128
int htm_comm_unique_id(void *id, size_t id_bytes);
int htm_comm_create(const void *id, size_t id_bytes, int rank, int n_ranks, int device, htm_comm **out);
int htm_comm_destroy(htm_comm *c);
int htm_comm_allgather(htm_comm *c, const void *d_send, void *d_recv, size_t bytes_per_rank, void *hip_stream);
int htm_chains_run_lockstep_comm(htm_chains *hc, int n_iter, htm_comm *c);
int htm_chains_sync(htm_chains *hc);        /* wait + raise device-side error flags */
int htm_chains_drain(htm_chains *hc);       /* sync + move device record buffers to host memory */

int htm_chains_iterations_done(htm_chains *hc, int *n);

/* Checkpoint / resume of a chain set (the reference has none, a 4 M-iteration production run
 * restarts from scratch).  The blob holds everything the main loop carries from one iteration to the next:
 * iteration counter, mod_random state at the consumed position, the five parameter vectors, temperatures,
 * log-likelihoods and proposal counters of every chain.  Priors, step sizes, observations and record
 * buffers are NOT in it: load into a chain set created from the same inputs (shapes are checked).
 * Continuing after load gives the bits of the uninterrupted run.  Not valid while a lock-step iteration is
 * in flight (between step_begin and step_end).  A load clears this rank's swap-record inbox (its tags are iteration
 * numbers, and iterations are about to be run again): for a multi-rank job every rank loads, then the ranks meet at a
 * barrier before the next htm_chains_run_lockstep_direct. */
int htm_chains_checkpoint_size(htm_chains *hc, size_t *bytes);
int htm_chains_checkpoint_save(htm_chains *hc, void *blob, size_t bytes);
int htm_chains_checkpoint_load(htm_chains *hc, const void *blob, size_t bytes);

/* chain state (`pt%get_mc(j)` + getters of src/cls_mcmc.f90:252-420); chain is 0-based; NULLs skipped */
int htm_chains_get_state(htm_chains *hc, int chain, double *hypo, double *t_corr, double *vs,
                         double *a_corr, double *qs, double *temp, double *log_likelihood,
                         int32_t n_propose[7], int32_t n_accept[7]);
int htm_chains_get_rng(htm_chains *hc, uint32_t state[4]);
/* Several ranks share this rank's GPU (`ranks_on_this_gpu` of them, this one included): every rank's persistent launch must be
 * resident at once (master and workers of a launch wait for each other), so each takes its share of the CUs.  Call before the
 * chain set's first launch; the environment variable HTM_RANKS_PER_GPU, if set, stands instead.  (The reference has no
 * counterpart: `mpirun -np N` ranks are CPU processes, src/cls_parallel.f90.) */
int htm_chains_share_gpu(htm_chains *hc, int ranks_on_this_gpu);
/* the chain's current log-likelihood alone (one 8-byte copy): what the reference's progress report prints every 1 000
 * iterations for chain 1 (`mc%one_step_summary`, src/cls_mcmc.f90:230-237) */
int htm_chains_get_loglik(htm_chains *hc, int chain, double *log_likelihood);

/* What the reference streams to likelihoodRR.out (src/hypo_tremor_mcmc.f90:279): (iteration, value) in
 * file order, plus the chain index that produced it. */
int htm_chains_lik_count(htm_chains *hc, int *n);
int htm_chains_lik_read(htm_chains *hc, int32_t *iter, int32_t *chain, double *log_likelihood);
/* What goes to vs/hypo/t_corr/qs/a_corr.RR.out (:273-277), sample k in file order */
int htm_chains_sample_count(htm_chains *hc, int *n);
int htm_chains_sample_read(htm_chains *hc, int k, int32_t *iter, int32_t *chain, double *vs, double *qs,
                           double *hypo, double *t_corr, double *a_corr);
int htm_chains_clear_records(htm_chains *hc);

/* Per-step trace for parity debugging: rows {iter, chain, type(1..7), index(1-based), prior_ok, accepted,
 * used_full, 0} and {x_new, loglik_proposed, loglik_after, temp}.  capacity 0 disables. */
int htm_chains_enable_steplog(htm_chains *hc, int capacity);
int htm_chains_steplog_read(htm_chains *hc, int *n, int32_t *irows, double *drows);

/* Kernel timing collected with HIP events inside htm_chains_run (stream-ordered, no extra syncs):
 * total device time of the last run in microseconds and the number of graph replays issued. */
int htm_chains_last_run_stats(htm_chains *hc, double *device_us, int *graph_launches,
                              int64_t *full_evals, int64_t *partial_evals);

/* Health of the in-kernel hand-off since the chain set was created: *orders_put_aside = how many times worker block 0 put an
 * order aside because the commit it names did not show within 20 us (0 in a healthy run: the chain waves take such orders
 * back themselves; the other worker blocks behave alike).  Synchronises with the handle's stream. */
int htm_chains_handoff_stats(htm_chains *hc, int64_t *orders_put_aside);

/* Which main loop the single-rank / lock-step launches of this chain set run on, and the health of its speculation:
 * *single_rank_loop / *lockstep_loop = 5 / 6 the pipelined master (csrc/htm_pipe.hpp), 3 / 4 the free-running chain master
 * (csrc/htm_flow.hpp), 0 / 2 the loop with workgroup barriers, -1 the two-kernel path; *flushes = how often the pipelined
 * master threw its speculative records away since the chain set was created (rare at production sizes).  No reference
 * counterpart (diagnostics).  Synchronises with the handle's stream. */
int htm_chains_master_stats(htm_chains *hc, int *single_rank_loop, int *lockstep_loop, int64_t *flushes);

/* *on = 1 if the latest single-rank launch of this chain set ran the free-running master's instantiation that is specialised on
 * what the job fixes (one rank, at most 8 chains, 64 or 128 stations with both data types, no step log: DESIGN.md 3.0; htm_chains_master_stats reports loop 3 for it as for the generic one), else 0.  The library selects
 * it from what it observes; HTM_FAST=0 in the environment at htm_chains_create forces the generic instantiation.
 * *worker_blocks (may be NULL) = the worker blocks of a launch.  No reference counterpart (diagnostics). */
int htm_chains_fixed_master(htm_chains *hc, int *on, int *worker_blocks);

/* *n_chains, *ring = the chain count and the ring size (positions of the stream window in LDS) that the latest single-rank launch
 * held as compile-time constants: the specialised master's sized instantiation (8 chains on a ring of 512: DESIGN.md 3.0), for
 * which htm_chains_fixed_master reports 1 as well.  0, 0: the launch was no sized one, or nothing was launched yet.  HTM_SIZED=0
 * in the environment at htm_chains_create keeps the sized instantiation out (A/B runs, tests).  No reference counterpart
 * (diagnostics). */
int htm_chains_sized_master(htm_chains *hc, int *n_chains, int *ring);

/* The launch plan of a chain set: which chain-master loop each mode runs and the shape it is launched with.  htm_chains_create
 * works it out from the job, the environment (the HTM_* switches) and a few facts it asks the device; htm_chains_plan runs the
 * same rules on facts the caller supplies and needs no device, so the plan of any shape can be asked on a machine without a GPU.
 * No reference counterpart (diagnostics, tests). */
typedef struct htm_plan_job {
    int32_t n_chains, n_procs, n_sta, n_events;
    int32_t forward_fp32, use_time, use_amp;
} htm_plan_job;
typedef struct htm_plan_device {      /* all 0 where htm_chains_create does not ask (HTM_PERSIST=0; no pipelined master) */
    int32_t n_cu;                     /* compute units */
    int32_t blocks_per_cu;            /* resident blocks per CU of a k_mcmc launch at (512 threads, step_smem): the smallest over the loops */
    int32_t pipe_blocks_per_cu[2];    /* ... of the pipelined master's two loops at their own LDS size, when one is asked for */
} htm_plan_device;
typedef struct htm_launch_plan {
    int64_t persist, flow, flow_fixed, wide, flow_lock, mb_blocks, pipe, pipe_lock, pipe_smem, pipe_ring;
    int64_t ring_size, wmax, step_smem, worker_cap, blocks_fit, nw;
    int64_t n_workers, mirror_n, mirror_steps;
    int64_t loop[3][2];               /* the loop (0..8, csrc/htm_plan.hpp loop_for) of the single-rank run, one lock-step iteration
                                       * per launch and persistent lock-step, [..][0] without and [..][1] with a step log */
    int64_t loop_built[3][2];         /* 1: the library holds that loop's kernel for this job */
} htm_launch_plan;
/* A shape that htm_chains_create refuses gives the same code here, and htm_last_error() the same text. */
int htm_chains_plan(const htm_plan_job *job, const htm_plan_device *device, htm_launch_plan *plan);
/* the plan this chain set was created with (htm_chains_share_gpu may have lowered n_workers since) and, if `seen` is not NULL,
 * the device facts it was planned with */
int htm_chains_get_plan(htm_chains *hc, htm_launch_plan *plan, htm_plan_device *seen);

/* Same work as htm_chains_run, but every kernel is launched eagerly and bracketed by its own pair of HIP
 * events on the handle's stream, so that the average duration of each kernel comes from the run itself:
 * k_step (proposals + partial updates + judge + swap; may cover several iterations per launch) and k_full
 * (batched full evaluations).  Returns sums in microseconds and launch counts; the chains advance by
 * n_iter iterations exactly as with htm_chains_run. */
int htm_chains_profile(htm_chains *hc, int n_iter, double *step_us, int *step_launches, double *full_us,
                       int *full_launches, int64_t *full_evals, int64_t *partial_evals);

/* self-test of the wave-level reduction and RNG device code against straightforward device loops;
 * returns 0 when they agree bit for bit */
/* ------------------------------------------------------------------------------------------------
 * Step-6 order statistics       reference: src/cls_statistics.f90:216-264, :345-431
 * The reference sorts every parameter's n_mod recorded samples (quick_sort, src/mod_sort.f90) and prints
 * the elements il = int(0.025*n_mod), im = int(0.5*n_mod), iu = int(0.975*n_mod) (1-based, single-
 * precision products) of the sorted column.  htm_quantiles returns exactly those elements without sorting:
 * samples [n_mod][n_par] row-major (one recorded model per row), ranks_1based[3] = {il, im, iu} or any other
 * three ranks in 1..n_mod (any order, repeats allowed), out [n_par][3]; n_mod <= INT_MAX, else HTM_EINVAL before any device
 * call, as for a rank outside 1..n_mod.  A column is ordered as a total order on the bits of its doubles: -NaN < -inf < ... <
 * -0.0 < +0.0 < ... < +inf < +NaN, NaNs among themselves by payload; the element returned keeps its bits.  Host
 * pointers; synchronous.  The _dev form takes device
 * pointers (ld = row stride in doubles) and is asynchronous on `hip_stream` (NULL = the null stream). */
int htm_quantiles(int device, const double *samples, long n_mod, long n_par, const int ranks_1based[3],
                  double *out);
int htm_quantiles_dev(int device, const double *d_samples, long n_mod, long n_par, long ld,
                      const int ranks_1based[3], double *d_out, void *hip_stream);

/* ------------------------------------------------------------------------------------------------
 * Convergence diagnostics of recorded samples: split R-hat and effective sample size per parameter,
 * Vehtari et al. 2021 / Stan without rank normalisation (with it: htm_diagnose_rank below).  samples [n_seq*n_draws][n_par] row-major, sequence m in
 * rows m*n_draws .. (m+1)*n_draws - 1.  Every sequence is split into its first and its last n = n_draws/2 draws; the
 * biased autocovariances of the 2 n_seq split sequences are averaged for lags 0..L, L = min(n - 1, max_lag).
 * out [n_par][4] = {rhat, ess, tau, lags}: ess = 2 n_seq n / tau; lags = the lag at which Geyer's pair sums first went
 * negative, or -1 if none did by L (ess is then an upper bound); a constant column gives four NaN.  acov, if not
 * NULL, receives the averaged autocovariances [(L+1)][n_par].  n_draws >= 4, n_seq, n_par, max_lag >= 1,
 * n_seq * n_draws <= INT_MAX, else HTM_EINVAL before any device call.  Every sum has a fixed order: two calls give
 * the same bits.  Host pointers; synchronous.  The _dev form takes device pointers (ld = row stride in doubles) and
 * is asynchronous on `hip_stream` (NULL = the null stream). */
int htm_diagnose(int device, const double *samples, long n_seq, long n_draws, long n_par, int max_lag,
                 double *out, double *acov);
int htm_diagnose_dev(int device, const double *d_samples, long n_seq, long n_draws, long n_par, long ld,
                     int max_lag, double *d_out, double *d_acov, void *hip_stream);

/* ------------------------------------------------------------------------------------------------
 * Rank-normalised diagnostics (Vehtari et al. 2021): what the split R-hat and ESS above miss -- sequences
 * that agree in location but not in scale, heavy tails, and whether the ends of the 2.5 % / 97.5 % intervals of the .stat
 * files were sampled enough.
 * htm_rank_normalize: samples [n_rows][n_par] row-major; r = the 1-based average rank of an element among the n_rows of
 * its column (ties share the mean of their positions, -0.0 = +0.0), z [n_rows][n_par] = Phi^-1((r - 3/8) / (n_rows + 1/4));
 * fold != 0 ranks |x - med| instead, med = the mean of the order statistics (n_rows+1)/2 and n_rows/2+1.  ranks, if not
 * NULL, receives r (exact half-integers).  2 <= n_rows <= INT_MAX, n_par >= 1.  The _dev form: ld, ld_z = row strides in
 * doubles of d_samples and of d_z and d_ranks; columns n_par .. ld_z - 1 are not touched.
 * htm_diagnose_rank: samples and shape rules as htm_diagnose; out [n_par][4] = {rhat_bulk, rhat_folded, ess_bulk, ess_tail}:
 * htm_diagnose's R-hat and ESS of z and of the folded z, and the smaller ESS of the indicators [x <= q05], [x >= q95] of
 * the column's 5 % and 95 % quantiles.  An entry is NaN where its matrix's column is constant.  The R-hat to report is
 * the larger of the two.  All rows are ranked, also the middle row that an odd n_draws drops from the split.
 * The columns are sorted in batches whose workspace stays under HTM_RANK_MB MiB (environment, default 2048); the result
 * does not depend on it, and two calls give the same bits.  A shape that needs a launch beyond 2^32 - 1 work-items is
 * HTM_EINVAL before any device call.  Host pointers: synchronous; _dev: device pointers, asynchronous on `hip_stream`. */
int htm_rank_normalize(int device, const double *samples, long n_rows, long n_par, int fold, double *z, double *ranks);
int htm_rank_normalize_dev(int device, const double *d_samples, long n_rows, long n_par, long ld, int fold,
                           double *d_z, long ld_z, double *d_ranks, void *hip_stream);
int htm_diagnose_rank(int device, const double *samples, long n_seq, long n_draws, long n_par, int max_lag, double *out);
int htm_diagnose_rank_dev(int device, const double *d_samples, long n_seq, long n_draws, long n_par, long ld,
                          int max_lag, double *d_out, void *hip_stream);

/* ------------------------------------------------------------------------------------------------
 * Location error ellipsoids of recorded samples.  hypo [n_mod][3 n_win] row-major, one recorded model per
 * row, window w in columns 3w, 3w+1, 3w+2 (the record of hypo.RR.out); pivots [n_mod][n_piv] pair with it row by row (vs, qs;
 * NULL when n_piv = 0).  out [n_win][22] = mean[3], cov[6] (xx, xy, xz, yy, yz, zz; divisor n_mod - 1), lambda[3] (the
 * covariance's eigenvalues, descending), V[9] (row-major, column k = the unit axis of lambda_k, its component of largest
 * magnitude positive), q = the rank_1based-th smallest squared Mahalanobis distance sum_k ((x - mean) . v_k)^2 / lambda_k of
 * the window's n_mod samples: the ellipsoid with semi-axes sqrt(q lambda_k) along v_k holds exactly rank_1based of them.
 * piv_corr [n_win][3][n_piv] = the correlation coefficients of x, y, z with every pivot (NULL when n_piv = 0), NaN where the
 * pivot or the coordinate is constant.  A window with a constant coordinate, or whose smallest eigenvalue is not positive,
 * keeps its mean and covariance (the entries of a constant coordinate are exactly 0); its lambda, V and q are NaN.
 * 4 <= n_mod <= INT_MAX, n_win >= 1, 0 <= n_piv <= 4, 1 <= rank_1based <= n_mod, ld >= 3 n_win, ld_piv >= n_piv, else
 * HTM_EINVAL before any device call, as for a shape that needs a launch beyond 2^32 - 1 work-items.  The distances are
 * taken in batches of windows (multiples of 64) whose workspace stays under HTM_ELLIPSOID_MB MiB (environment, default
 * 1024; one wave's 64 windows at the least); the result does not depend on it, and two calls give the same bits.  Host
 * pointers: synchronous; _dev: device pointers (ld, ld_piv = row strides in doubles; columns beyond 3 n_win are never read),
 * asynchronous on `hip_stream`. */
int htm_hypo_ellipsoid(int device, const double *hypo, const double *pivots, long n_mod, long n_win, int n_piv,
                       long rank_1based, double *out, double *piv_corr);
int htm_hypo_ellipsoid_dev(int device, const double *d_hypo, long ld, const double *d_pivots, long ld_piv,
                           long n_mod, long n_win, int n_piv, long rank_1based,
                           double *d_out, double *d_piv_corr, void *hip_stream);

/* ------------------------------------------------------------------------------------------------
 * Stacked density maps of recorded samples.  hypo as for the ellipsoids; layer [n_win] gives every window
 * its layer (a time bin, say), NULL puts every window in layer 0 of n_layer = 1; a window whose layer lies outside
 * 0 .. n_layer - 1 takes no part and is in nobody's tally.  grid9: the map grid (above htm_forward_locate; host memory in both
 * forms).  On an axis {v0, dv, n} a coordinate v has q = (v - v0) / dv (a true
 * fp64 division); it is inside iff 0 <= q < n (cells are half-open, the box's top edge is outside, as are NaN and +-inf) and
 * then lies in cell floor(q).  A sample counts iff its three coordinates are inside, and then once in each output:
 * xy [n_layer][ny][nx], xz [n_layer][nz][nx], yz [n_layer][nz][ny], vol [n_layer][nz][ny][nx] (or NULL), and
 * tally [n_layer][2] = {inside, outside}.  So every map of a layer sums to the layer's inside, and inside + outside is n_mod
 * times the layer's windows.  The call zeroes the outputs before it counts; the counts are exact and the same for every
 * order of the adds, row-slab count (HTM_DENSITY_SLABS) and counting path (HTM_DENSITY_LDS = 0 | 1 forbids or forces the
 * LDS-resident maps, which take a grid with nx ny + nx nz + ny nz <= 8192; forced on a larger grid: HTM_EINVAL).
 * n_mod, n_win, n_layer >= 1; ld >= 3 n_win; what the map grid asks of every axis; at most
 * 2^31 - 1 counters over all layers and requested outputs; else HTM_EINVAL before any device call, as for a shape that needs a
 * launch beyond 2^32 - 1 work-items.  Host pointers: synchronous, the rows in batches under HTM_DENSITY_MB MiB (environment,
 * default 1024) whose counts are added on the host; _dev: device pointers (ld = row stride in doubles; columns beyond
 * 3 n_win are never read), asynchronous on `hip_stream`. */
int htm_hypo_density(int device, const double *hypo, long n_mod, long n_win, const int *layer, int n_layer,
                     const double *grid9, unsigned long long *xy, unsigned long long *xz, unsigned long long *yz,
                     unsigned long long *vol, unsigned long long *tally);
int htm_hypo_density_dev(int device, const double *d_hypo, long ld, long n_mod, long n_win, const int *d_layer, int n_layer,
                         const double *grid9, unsigned long long *d_xy, unsigned long long *d_xz, unsigned long long *d_yz,
                         unsigned long long *d_vol, unsigned long long *d_tally, void *hip_stream);

/* ------------------------------------------------------------------------------------------------
 * Step 4, `hypo_tremor_select`   reference: src/cls_selector.f90:75-132, src/mod_regress.f90
 * For every detected window: the station of largest amplitude is taken as the epicentre (depth z_guess), the
 * amplitudes are corrected for geometrical spreading (+ ln d), and arrival time and amplitude are regressed
 * against distance with weights 1/err^2.  t, t_err, a, a_err: (n_sta, n_win) column-major = the columns 4-7 of the
 * opt_data.NNNNNN.dat files; out[n_win][6] = {vs, b, t0, a0, cc_t, cc_a}: the columns of a regress.dat row after
 * the window id (src/hypo_tremor_select.f90:124-125).  The station of largest amplitude is Fortran maxloc(a) as the
 * reference's compiler evaluates it: the first station whose a is not NaN is the candidate, -inf
 * included; a later one replaces it only if its a is strictly greater, so ties go to the lower index; a window whose
 * a are all NaN takes station 1.  NaN and inf inputs give NaN or inf outputs as the reference's arithmetic does.
 * n_sta >= 3; n_win < 2^26 - 3 (a wave per window: 64 n_win work-items in one launch).  Host pointers; synchronous. */
int htm_select_regress(int device, int n_sta, int n_win, const double *sta_x, const double *sta_y,
                       const double *sta_z, double z_guess, const double *t, const double *t_err,
                       const double *a, const double *a_err, double *out);

/* ------------------------------------------------------------------------------------------------
 * Step 2, `hypo_tremor_correlate`       reference: src/cls_correlator.f90:179-235, src/mod_signal_process.f90
 * Windowed cross-correlations of station envelopes.  d_env: n_sta rows of n_smp amplitudes, row stride ld_env
 * doubles.  Window w (0-based) of a station is samples w*n_step .. w*n_step+n-1; it is tapered (nleng = int(0.05 n)
 * cosine samples at each end), demeaned and divided by its norm (:207-223; a window of zero energy gives an all-zero
 * correlogram and cc_max = 0, where the reference reuses a stale buffer).  For the pairs pair0 .. pair0+n_pairs-1 of
 * the station-file order (1,2), (1,3), ..., (2,3), ... (0-based index), every window and every lag:
 *     d_cc[(w*n + j)*ld_cc + p] = sum_m r_i[m] * r_j[(m + k) mod n],  k = (j - n/2) mod n,
 * i.e. row j holds lag j - n/2, negative lags first (:234-235), one column per pair -- the layout htm_quantiles_dev
 * selects over with n_mod = n_win*n, ld = ld_cc.  d_cc_max[w*ld_cc + p] = max_j of that window.  n even in 2..4096
 * (the reference refuses odd n, :179-182), (n_win-1)*n_step + n <= n_smp <= ld_env, ld_cc >= n_pairs, and one launch:
 * n_win*n_pairs*min(1024, n rounded up to 64) work-items below 2^32; anything else is HTM_EINVAL, returned before
 * any device call.  Device pointers; asynchronous on `hip_stream` (NULL = the null stream). */
int htm_xcorr_dev(int device, const double *d_env, long ld_env, long n_smp, int n_sta, int n, int n_step, int n_win,
                  int pair0, int n_pairs, double *d_cc, long ld_cc, double *d_cc_max, void *hip_stream);
/* the same with host pointers, for tests: env [n_sta][n_smp], cc [n_win*n][n_pairs], cc_max [n_win][n_pairs].
 * Synchronous. */
int htm_xcorr(int device, const double *env, long n_smp, int n_sta, int n, int n_step, int n_win, int pair0,
              int n_pairs, double *cc, double *cc_max);

/* ------------------------------------------------------------------------------------------------
 * Step 3, `hypo_tremor_measure`                 reference: src/cls_measurer.f90:405-523
 * Per detected window (one workgroup each): optimize_cc (:463-523) -- r = taper(x) / sum(x^2), for every pair
 * i < j the first maximum of the circular correlation in natural order (Fortran maxloc), lag = idx*dt for
 * idx < n/2 else (idx - n)*dt, t(i) = -sum_j lag(i,j) / n_sta and t_stdv(i) = sqrt(sum_{j!=i} (t(j) - t(i) -
 * lag(i,j))^2 / (n_sta - 2)), both summed serially in j; a station of zero energy has lag 0 against every
 * station (the reference divides 0 by 0).  Then optimize_amp (:405-459) -- each station shifted by nint(t/dt),
 * rel(i,j) = log(sxy / sxx(i)), amp and amp_stdv as t and t_stdv; any sxy < 0 gives amp = amp_stdv = 0 for the
 * whole window (:430-434).  x [n_det][n_sta][n] raw envelope windows; t, t_stdv, amp, amp_stdv [n_det][n_sta].
 * n_sta >= 3, 2 <= n <= 4096, dt > 0.  The windows go in launches of at most HTM_MEASURE_MB MiB (environment,
 * default 256) of inputs and workspace, at least one window each; the results do not depend on it.  Host
 * pointers; synchronous. */
int htm_measure_windows(int device, int n_sta, int n, double dt, int n_det, const double *x, double *t,
                        double *t_stdv, double *amp, double *amp_stdv);

/* ------------------------------------------------------------------------------------------------
 * Batched fp64 complex FFT (step 1's transforms)
 * Rows of n interleaved complex values (re, im doubles), row stride ld in complex elements:
 *     out[row][k] = sum_j in[row][j] exp(direction 2 pi i j k / n),  direction = -1 forward, +1 backward,
 * unnormalised both ways.  Lengths whose prime factors are 2, 3, 5 and 7 run as Stockham passes of radix 2, 3, 4, 5
 * and 7; any other length by Bluestein with a power-of-two inner transform.  Twiddle and chirp tables are built in
 * long double on the host once per (device, n), uploaded synchronously and kept for the life of the process.
 * 1 <= n <= 2^24, batch >= 1, ld_in, ld_out >= n; in place (d_in == d_out, ld_in == ld_out) or on disjoint buffers;
 * one launch holds fewer than 2^32 work-items (batch * n, or batch * m for Bluestein's inner length m); anything
 * else is HTM_EINVAL before any device call.  Only the n values of each row are written.  In place and out of place
 * give the same bits.  Device pointers; the workspace is allocated stream-ordered on `hip_stream` (NULL = the null
 * stream), so the call is asynchronous after a plan's first build. */
int htm_fft_dev(int device, const double *d_in, long ld_in, double *d_out, long ld_out, long n, long batch, int direction,
                void *hip_stream);
/* the same with host pointers, for tests: in [batch][ld_in], out [batch][ld_out] complex (padding of out kept).
 * Synchronous. */
int htm_fft(int device, const double *in, long ld_in, double *out, long ld_out, long n, long batch, int direction);

/* ------------------------------------------------------------------------------------------------
 * Step 1, `hypo_tremor_convert`   reference: src/cls_convertor.f90:84-443, src/mod_signal_process.f90:10-26
 * Smoothed, merged envelope of one station: segments of n samples every n2 = n/2 of a record of N = n_total
 * samples; segment j covers stream samples [j n2, j n2 + n), samples at or beyond N read as 0; the segments are
 * j = 0 .. last, last = (N - n) / n2 + 1.  Per segment and component: detrend (least-squares line in the 1-based
 * index), cosine taper (nleng = int(0.05 n)), forward DFT X, Y[0] = 0, Y[k] = 2 w(k) X[k] for 1 <= k <= n/2, 0 above,
 * with the band weight w of bins k1..k4 = k_band (k < k1: 0, [k1, k2): 0.5 (1 - cos((k-k1) pi / (k2-k1))),
 * [k2, k3): 1, [k3, k4): 0.5 (1 + cos((k-k3) pi / (k4-k3))), k >= k4: 0), e = |backward DFT(Y) / n|, two box
 * smoothings of half width h with the reference's windows (1-based i: i <= h: sum e[1..i+h] / (i+h); h < i <= n-h:
 * sum e[i-h+1..i+h] / (2h+1); i > n-h: sum e[i-h+1..n] / (n+h-i+1)), and the merge
 * sqrt((e1 fac1)^2 + (e2 fac2)^2).  Segment j keeps the stream samples [start(j), end(j)): start = 0 for j = 0, else
 * j n2 + n/4; end = N for j = last, else j n2 + n - n/4.  These ranges tile [0, N).  The output holds the kept
 * samples g that are multiples of n_fac, value k = g / n_fac.
 * One call handles segments j0 .. j1: d_x1, d_x2 are the two components from stream sample j0 n2 on, holding
 * min(N, j1 n2 + n) - j0 n2 float32 samples each; d_out receives values ceil(start(j0) / n_fac) ..
 * ceil(end(j1) / n_fac) - 1.  n a multiple of 4 in 4..2^24, N >= n, 1 <= n_fac <= n/2, 0 <= h <= 4096 with 2h <= n,
 * 0 <= k1 <= k2 <= k3 <= k4, 0 <= j0 <= j1 <= last, and 2 (j1 - j0 + 1) n (or Bluestein's 2 (j1 - j0 + 1) m) below
 * 2^32; anything else is HTM_EINVAL before any device call.  Device memory: about 80 n bytes per segment of workspace
 * (Bluestein lengths: 48 n + 64 m), allocated stream-ordered.  Device pointers; asynchronous on `hip_stream` (NULL =
 * the null stream) after the FFT plan of n is built. */
int htm_convert_dev(int device, const float *d_x1, const float *d_x2, long n_total, int n, int n_fac, int h,
                    const int k_band[4], double fac1, double fac2, long j0, long j1, double *d_out, void *hip_stream);
/* the same with host pointers, for tests.  Synchronous. */
int htm_convert(int device, const float *x1, const float *x2, long n_total, int n, int n_fac, int h, const int k_band[4],
                double fac1, double fac2, long j0, long j1, double *out);

int htm_selftest(int device);

/* y[i] = fn(x[i]) for n host values, fn = the forward model's own fp64 routines: which = 0 the logarithm of the amplitude
 * term (reference src/cls_forward.f90:204, `log(d)`), 1 the square root of the squared distance (:115-117), 2 the device
 * library's sqrt (what 1 must equal), 3 the device library's log -- the one used by the Rayleigh prior ratio
 * (reference src/cls_model.f90:184-185, `log(x_new - mu) - log(x_old - mu)`: a term of the Metropolis decision, so the test
 * compares it with the host libm the reference links).  Lets a test measure them against a wider-precision result (stated
 * bound of the logarithm: < 1 ulp).  The wave-level sums of the likelihood (cls_forward.f90:125-132, :210-217, :281-299) have
 * their own modes: 4 = every lane's sum of its wave's 64 values on the matrix pipe (n a multiple of 64), 5 / 6 = x is four blocks
 * of n / 4 values, a wave's four sums taken at once (5) or one by one (6) -- a test compares the associations bit for bit
 * (n a multiple of 256).  The forms the specialised chain master runs with loop constants in vector registers: 7 = the logarithm
 * of mode 0 with its ten constants read from registers (must equal mode 0 bit for bit), 8 / 9 = the sums of mode 5 with the lane
 * classes read from two registers, four values at once (8) or as two pairs (9) (must equal mode 6; n a multiple of 256).
 * Synchronous. */
int htm_selftest_math(int device, int which, const double *x, double *y, int n);

/* mod_random's generator (reference src/mod_random.f90:60-74) is linear over GF(2): the state after n draws is
 * T^n * state.  Host-only (no device needed): used to seek in a rank's stream and by the tests that pin the
 * jump tables of the device generator.  state = {x, y, z, w} as in mod_random.f90:30. */
int htm_rng_jump(const uint32_t state_in[4], unsigned long long n_draws, uint32_t state_out[4]);

#ifdef __cplusplus
}
#endif
#endif /* HTM_HIP_H */
