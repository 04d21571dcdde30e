/* chs_hip.h -- C ABI of the MI355X (gfx950) Cahn-Hilliard timestep engine.
 *
 * Drop-in boundary for ONE hot path of uncertaintyhub/chsimpy: the per-timestep
 * solver loop.  The reference has no FFI of its own; the seam is the Python
 * method pair
 *     Solver.prepare()                 chsimpy/solver.py:84-135
 *     Solver.solve_or_resume(nsteps)   chsimpy/solver.py:137-252
 * (called from chsimpy/simulator.py:41,43,69 and examples/benchmark.py:72-74).
 * A ctypes-backed `Solver` look-alike (chsimpy_amd/solver.py) binds exactly the
 * entry points below; INTEGRATION.md shows the stub a chsimpy maintainer would add.
 *
 * Conventions
 *   - plain pointers and sizes only; the caller owns every host buffer, the
 *     library owns the device buffers for the lifetime of the handle;
 *   - one opaque handle per simulation, one HIP stream and one pair of pinned staging
 *     chunks per handle -> 8 handles can live on 8 devices of a node, and several on one
 *     device move their fields concurrently (ensemble runs, chsimpy/experiment.py:84-126).
 *     Library-owned state outside the handles: the thread-local last-error string and the
 *     pool of parked engines (a mutex-protected free list, see chs_create / chs_pool_clear);
 *   - every call is synchronous on return;
 *   - return value: CHS_OK (0) or a negative CHS_E* code; chs_last_error()
 *     gives the text.
 */
#ifndef CHS_HIP_H
#define CHS_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CHS_OK 0
#define CHS_EINVAL (-1)   /* bad argument / unsupported configuration            */
#define CHS_EHIP (-2)     /* a HIP runtime call failed                           */
#define CHS_ENAN (-3)     /* a recorded scalar became NaN (chsimpy/timedata.py:10) */
#define CHS_ESTATE (-4)   /* call order violated (e.g. step before prepare:
                             the assert at chsimpy/solver.py:139)                */
#define CHS_ECHECK (-5)   /* a self-check of a device result failed (chs_components) */
/* -6: a look would cost more than its caller allows (chs_thickness: WORK > max_work; chs_geodesic: max_rounds; chs_skeleton: max_subiters).  Written relative to CHS_ECHECK:
 * tests/test_components_host.py reads the literal codes above and holds CHS_ECHECK to be the last of them. */
#define CHS_ELIMIT (CHS_ECHECK - 1)

/* arithmetic type of the device path */
#define CHS_F64 0
#define CHS_F32 1

/* transform engine */
#define CHS_ENGINE_AUTO 0   /* fast for N = 2^k in [128, 8192]; else chirp for
                               CHS_CHIRP_AUTO_MIN_N <= N <= 4096; else direct    */
#define CHS_ENGINE_DIRECT 1 /* dense cosine-matrix products, any N >= 8          */
#define CHS_ENGINE_FAST 2   /* LDS-staged FFT-based row/column DCT passes        */
#define CHS_ENGINE_CHIRP 3  /* chirp-z (Bluestein) line transforms on power-of-two
                               FFTs in LDS, any N in [8, 4096]                   */
/* The smallest N that CHS_ENGINE_AUTO gives to the chirp engine: max(129, N*) with N* the smallest probed N from which
 * the chirp engine measures at least 1.1x the direct engine's steps per second at every larger probe
 * (tools/chirp_bench.py, profiles/r08_chirp.txt).  Measured N* = 100 (1.6x there, 2.0x at 129,
 * 5.8x at 1000, 10.7x at 4000); the floor of 129 keeps the small grids, N = 64 and N = 100, on the direct engine. */
#define CHS_CHIRP_AUTO_MIN_N 129

/* stop reasons (chsimpy/solver.py:133,198,246) */
#define CHS_STOP_NONE 0
#define CHS_STOP_ENERGY 1
#define CHS_STOP_TIME_LIMIT 2

/* Scalars the loop reads.  They are what chsimpy/solution.py:25-55 derives from
 * chsimpy/parameters.py:24-61; the host wrapper computes them exactly as the
 * reference does and hands them over. */
typedef struct chs_consts {
  int32_t N;              /* grid is N x N                       parameters.py:25 */
  int32_t dtype;          /* CHS_F64 | CHS_F32                                    */
  int32_t device;         /* HIP device ordinal                                   */
  int32_t engine;         /* CHS_ENGINE_*                                         */
  int32_t adaptive_time;  /* parameters.py:57 ; solver.py:177-193                 */
  int32_t full_sim;       /* parameters.py:50 ; solver.py:245-249                 */
  double RT;              /* R*temp                              solution.py:31   */
  double BRT;             /* B*R*temp                            solution.py:32   */
  double B;               /*                                     parameters.py:31 */
  double A0, A1;          /* func_A0(temp), func_A1(temp)        solution.py:34-35 */
  double Amr;             /* 1/Am                                solution.py:33   */
  double kappa_tilde;     /*                                     solution.py:39-48 */
  double L;               /*                                     parameters.py:26 */
  double delx;            /* L/(N-1)                             solution.py:28   */
  double delt;            /* initial time step                   parameters.py:36 */
  double delt_max;        /*                                     parameters.py:37 */
  double M_tilde;         /*                                     parameters.py:38 */
  double threshold;       /*                                     parameters.py:41 */
  double time_limit_s;    /* time_max*60, <= 0: none             solver.py:151-153 */
} chs_consts;

/* Solver-side state that survives between solve_or_resume calls
 * (chsimpy/solver.py:50-54) plus the Solution counters (solution.py:57-61). */
typedef struct chs_state {
  double delt;            /* solver.py:54, updated by 185-188   */
  double time_delta_sum;  /* solver.py:51,195                   */
  double time_passed;     /* solver.py:52,196                   */
  double tau0;            /* solution.py:58 ; solver.py:243     */
  double t0;              /* solution.py:59 ; solver.py:244     */
  int64_t computed_steps; /* solution.py:60 ; solver.py:134,240 */
  int32_t skip_check;     /* solver.py:50,249                   */
  int32_t stop_reason;    /* CHS_STOP_*                         */
} chs_state;

typedef struct chs_handle_s* chs_handle;

/* Create an engine for one simulation.  `lambda` is the host-computed 1-D table
 * lam_i = 2cos(pi i/(N-1)) - 2, i = 0..N-1 (chsimpy/utils.py:34-36); the N x N
 * grids CHeig/Seig of utils.py:39-49 are never materialised, they are formed on
 * the fly from this table and the current delt.
 * Environment (read here, test hooks): CHS_ADAPT_SWEEP=1 keeps the separate sweep
 * of U for the adaptive-step column sums instead of the fused row kernel's;
 * CHS_ADAPT_SPARSE=0 issues the adaptive step's reduction launches and the gate on every step instead of only on
 * the steps whose step-size rule fires; CHS_LAM_BY_COLMIN=0 leaves the coefficients of a firing step to the gated
 * bookkeeping instead of the reduction's last block; CHS_GATE_EARLY=1 (experiment, measured equal) lets that
 * bookkeeping publish the coefficients ahead of the step's record;
 * CHS_BATCH_STEPS=n issues the steps of a call n at a time (default 1024, 256 with a stop rule armed) -- between
 * batches the host looks at the device's stop flag, see chs_step_n.
 * chs_destroy parks up to four engines (fields up to 160 MB) instead of freeing them and chs_create takes a
 * parked engine of the same device, N, dtype, transform engine and lambda table into use again with the new
 * constants -- an ensemble creates one engine per member; a run on such an engine is bit for bit the run on
 * a new one.  The parked engines hold at most 3 GiB of device memory together (the least recently parked
 * ones are freed first); chs_pool_clear() frees them all.  CHS_ENGINE_POOL=0 (read at both calls) switches
 * the pool off.  A handle must not be used after chs_destroy either way.
 * CHS_TEST_GATE_WITHHOLD=1 (test hook, read by chs_step_n; compiled in only when the library is built with
 * -DCHS_TEST_HOOKS=1, which __graft_entry__.build() does -- a build without it ignores the variable): the in-launch
 * bookkeeping of stop-rule / adaptive runs never publishes its decision, so that the waiting workgroups run into
 * their bounded timeout -> chs_step_n returns CHS_EHIP. */
int chs_create(const chs_consts* consts, const double* lambda, chs_handle* out);
int chs_destroy(chs_handle h);
/* Free every parked engine of this process (all devices); chs_pool_count: how many are parked right now. */
int chs_pool_clear(void);
int chs_pool_count(void);

/* Upload the N x N row-major float64 field (the reference's U_init / solution.U).
 * Replaces `U = self.U_init.copy()` (solver.py:85) and `U = self.solution.U`
 * (solver.py:158). */
int chs_set_U(chs_handle h, const double* host_U);
/* The same without a host array, for the reference's default start field (solver.py:78-82):
 * U[r][c] = base + scale * (rand - 0.5), rand = draw r*N+c of numpy's PCG64 `Generator.random`
 * started from the 128-bit `state` / `inc` ({high word, low word}) -- bit-identical to
 * `XXX + XXX*0.01*(rng.random((N,N)) - 0.5)` with base = XXX, scale = XXX*0.01. */
int chs_init_U_pcg64(chs_handle h, double base, double scale, const uint64_t state[2], const uint64_t inc[2]);
/* Download the current field (solver.py:251 `self.solution.U = U`). */
int chs_get_U(chs_handle h, double* host_U);

/* Step-0 diagnostics of solver.py:100-127 on the current field.  Fills
 * row0 = [it=0, E, E2, SA=0, domtime=0, Ra, L2=0, PS, delt] (column order of
 * chsimpy/timedata.py:9) and resets computed_steps=1, tau0=t0=0,
 * stop_reason=None (solver.py:128-135).  delt / time_delta_sum / skip_check
 * are NOT reset, exactly as in the reference. */
int chs_prepare(chs_handle h, double row0[9]);

/* Run up to `nsteps` iterations of solver.py:165-249 on the device without any
 * per-step host synchronisation (the launches go out in batches; once the device
 * has raised its stop flag no further batch is issued, so a run that stops early
 * does not pay for the rest of ntmax).  On entry hat_U = dctn(U) is re-derived
 * (solver.py:159) and the coefficients CHeig/Seig are those of consts.delt again
 * (solver.py:154-155) until the adaptive step regenerates them (189-193).  The caller passes the iteration count of
 * range(itbegin, nsteps) (solver.py:160-165).  `rows` receives one 9-column
 * timedata row per completed step ([nsteps][9], column order timedata.py:9);
 * `*steps_done` how many were completed (fewer than nsteps after an energy or
 * time-limit stop, which are decided on the device, solver.py:197-199,242-249).
 * Returns CHS_ENAN when a recorded scalar is NaN (timedata.py:10); the rows up
 * to and including the NaN row are still returned, the field is unspecified then
 * (the reference raises before it assigns solution.U, solver.py:251).
 * The device keeps the field of intermediate steps in registers where nothing can
 * observe it; chs_get_U after the call returns the field of the last completed step
 * in every mode -- also after an energy or time-limit stop, where it is rebuilt from
 * hat_U -- exactly as `self.solution.U = U` after the reference's loop
 * (solver.py:197-199, 242-251).
 * CHS_EHIP with "gave up waiting" (the bounded wait of the in-launch bookkeeping ran out; only ever seen with
 * the test hook): *steps_done = 0 and the device holds no consistent state of a completed step -- the handle
 * is un-prepared and field-less afterwards: chs_step_n returns CHS_ESTATE until chs_set_U / chs_init_U_pcg64
 * and chs_prepare have been called again. */
int chs_step_n(chs_handle h, int64_t nsteps, int32_t flags, double* rows, int64_t* steps_done);
/* flags for chs_step_n */
#define CHS_STEP_CARRY_HAT 1 /* do not re-derive hat_U on entry: continue the loop of the
                                previous call (used to feed per-step host jitter noise while
                                keeping the reference's carried hat_U, solver.py:206-211) */

#define CHS_STEP_REDERIVE_HAT 2 /* recompute hat_U = dctn(U) on entry (the literal solver.py:159) even when the
                                  previous call left the loop's state on the device.  Without it a call with a
                                  fixed time step that follows a completed call (no new field, state or noise
                                  in between) continues that call's loop: hat_U is carried instead of being
                                  recomputed from the field it was inverted to -- the same array up to
                                  rounding -- and the sequence of calls gives bit for bit what one call gives.
                                  (implies that the call's last step prepares no continuation, like
                                  CHS_STEP_LAST_CALL, unless CHS_STEP_KEEP_T1 is given too) */
#define CHS_STEP_KEEP_T1 8     /* with CHS_STEP_REDERIVE_HAT: hat_U = dctn(U) is recomputed on entry, but the row
                                  transform of EnergieEut(U) for the first step -- a function of the unchanged field
                                  alone, which the last step of a completed predecessor left on the device as every
                                  step inside a call does -- is taken over instead of being computed again (bit for
                                  bit the same run); such a call's own last step prepares it for a successor */
#define CHS_STEP_LAST_CALL 4   /* the run ends with this call: its last step does not prepare a continuation (the
                                  forward row pass of a step that will not come); a later call is still correct,
                                  it enters through hat_U = dctn(U) */

int chs_get_state(chs_handle h, chs_state* out);
int chs_set_state(chs_handle h, const chs_state* in);

/* U += jitter * (2*noise - 1) with host-supplied noise (solver.py:210-211).  The
 * reference draws `noise` from its seeded host generator; keeping the draw on the
 * host keeps its stream bit-identical.  hat_U is left untouched, as in the
 * reference. */
int chs_set_jitter_noise(chs_handle h, double jitter, const double* host_noise);
/* The same with the noise drawn on the device: the stream of numpy's PCG64 (`Generator.random`,
 * the reference's default generator, solver.py:78-82,211) continued from the 128-bit `state` and
 * `inc` of the host generator ({high word, low word}); every step consumes N*N draws in C order.
 * The caller advances its own generator by N*N per completed step afterwards
 * (`bit_generator.advance`).  jitter outside (0, 0.1) or a later chs_set_jitter_noise switches it off. */
int chs_set_jitter_pcg64(chs_handle h, double jitter, const uint64_t state[2], const uint64_t inc[2]);

/* Test / diagnostic hooks (not on the reference seam). */
/* 2-D orthonormal DCT-II (inverse=0) or DCT-III (inverse=1) of a host array
 * through the handle's transform engine: scipy.fftpack.dctn/idctn(norm='ortho')
 * as called at solver.py:159,201,208. */
int chs_dctn(chs_handle h, const double* host_in, double* host_out, int inverse);
/* EnergieEut of solver.py:166-175 for the current field. */
int chs_get_mu(chs_handle h, double* host_mu);
/* Device math primitives evaluated elementwise on `device` (accuracy tests):
 * which = 0: log(a)   1: log(a/b)   2: EnergieEut(a) with (RT,BRT,A0,A1) = b[0..3]
 *         3: bulk energy density(a) with (RT,B,A0,A1) = b[0..3]  (solver.py:218-221)
 *         4: log(a) for a > 0 (division-based variant)
 *         5: log(a) for a > 0, table-driven (the variant the fused row kernel uses) */
int chs_test_math(int device, int which, const double* a, const double* b, double* out, int64_t n);
/* The other inline functions of chs_math.h, each called elementwise as the step kernels call it (accuracy tests).
 * `in` holds four input columns of n doubles each (column c at in + c*n; a column a code does not read may hold
 * anything), `consts` eight uniform constants, `out` receives two output columns of n doubles (out1 is 0 where a code
 * has one result).  The physics codes read consts = {RT, B, BRT, A0, A1, sE0}.  The fp32 codes convert every input
 * and constant to float first -- exact when the caller has rounded them to float -- compute in float and return the
 * result widened to double.  A domain word is returned as what chs_log_dom_bad says of it, 0 or 1, never folded into NaN.
 *   which  function                                       in0..in3         out0, out1
 *   10     chs_div_pos                                    d, sig           quotient, the reciprocal seed rcp(sig)
 *   11     chs_div_pos1                                   d, sig           quotient, the reciprocal seed rcp(sig)
 *   12     chs_energy_mu_from_logs<true, true>            U, Uinv, lU, lV  sE (from sE0), mu
 *   13     chs_energy_mu_from_logs<true, false>           U, Uinv, lU, lV  sE (from sE0), 0
 *   14     chs_energy_mu_from_logs<false, true>           U, Uinv, lU, lV  sE0 untouched, mu
 *   15     one point of the fused fp64 row kernel:        u                sE (from sE0), mu
 *          uinv = 1 - u, two chs_log_unit_tab_f64, chs_energy_mu_from_logs<true, true>
 *   16     the same chain                                 u                mu, domain word bad
 *   17/18  chs_energy_from_logs / chs_mu_from_logs <double>        U, Uinv, lU, lV  value
 *   19/20  chs_energy_from_logs_fast / chs_mu_from_logs_fast <double>   "            value
 *   21-24  the four of 17-20 in <float>                                "            value
 *   25     chs_dt_integrand, delt_max = consts[0]         mu               value
 *   26     chs_dt_integrand_fast, the double form, the same arguments
 *   27     chs_dt_integrand_fast, the float form, the same arguments
 *   28     chs_spectral<double>, lam1 = consts[0], lam2 = consts[1]   hatU, hatMu, li, lj   value
 *   29     chs_spectral<float, false>, the same arguments
 *   30     chs_spectral_f32, the same arguments
 *   31     chs_logf                                       x                value
 *   32     chs_log_ratio<float>                           a, b             value
 *   33     chs_mu<float>                                  U                value
 *   34     chs_energy_density<float>                      U                value
 *   35     chs_log_unit_tab<float>                        x                value, domain word bad
 *   36     chs_log_unit_tab<double>                       x                value, domain word bad
 * CHS_EINVAL for a null argument, n outside [1, 2^28] or another code. */
int chs_test_math_cols(int device, int which, const double* in, const double* consts, double* out, int64_t n);
/* Which engine the handle resolved to (CHS_ENGINE_DIRECT / CHS_ENGINE_FAST / CHS_ENGINE_CHIRP). */
int chs_engine(chs_handle h);

/* Measurement hooks used by bench.py. */
#define CHS_NKERNELS 8
/* Names of the per-step kernels of the resolved engine, slot i (NULL beyond). */
const char* chs_kernel_name(chs_handle h, int slot);
/* Run `nsteps` steps with HIP events bracketing every kernel launch on the
 * handle's stream; ms[i] receives the summed device time of slot i, calls[i]
 * its launch count.  Results are identical to chs_step_n. */
int chs_profile_steps(chs_handle h, int64_t nsteps, double ms[CHS_NKERNELS], int64_t calls[CHS_NKERNELS]);
/* Device time (ms, HIP events on the handle's stream) of the last chs_step_n. */
double chs_last_step_ms(chs_handle h);

/* ---- Radially averaged structure factor of the current field ------------------------------
 * C = dctn(U - mean(U), norm='ortho') through the handle's own transform engine; the power of mode (i, j) is C[i][j]^2,
 * that of mode (0, 0) counts as 0.  The mode's bin is the integer nearest to sqrt(i^2 + j^2), decided in integer
 * arithmetic: with s = i^2 + j^2 the one b with b^2 - b < s <= b^2 + b (b = 0 for s = 0; no tie exists).  Bins run
 * 0 .. nb-1, nb = bin(N-1, N-1) + 1 = chs_structure_factor_bins(N); every mode is counted, the corners included.
 * ssum[b] receives the sum of the power over the modes of bin b, float64 whatever the handle's element type.  How many
 * modes a bin has is a function of N alone and left to the caller (chsimpy_amd/spectrum.py: bin_sizes, and S, k1 and
 * the characteristic length 2N/k1 derived from ssum).
 * Works on any handle that holds a field (else CHS_ESTATE) -- before and after chs_prepare, between two chs_step_n
 * calls -- and is deterministic: two calls on one field return the same bits.  It uses only device arrays that are
 * dead between two calls, so the run does not notice it: the chs_step_n that follows gives bit for bit what it gives
 * behind a chs_get_U in the same place, a continued loop (see CHS_STEP_REDERIVE_HAT) included.
 * nbins != chs_structure_factor_bins(N): CHS_EINVAL, the expected value in the message. */
int32_t chs_structure_factor_bins(int32_t N);   /* nb(N); CHS_EINVAL for N outside [1, 16384] */
int chs_structure_factor(chs_handle h, double* ssum, int32_t nbins);
/* Device time (ms, HIP events) of the three parts of the handle's last chs_structure_factor: ms[0] the sweeps (mean,
 * U - mean), ms[1] the transform, ms[2] the binning (both stages).  CHS_ESTATE before the first call. */
int chs_structure_factor_last_ms(chs_handle h, double ms[3]);

/* ---- Morphology of the thresholded field: area, interface length, Euler number -------------
 * Foreground: X[i][j] = ((double)U[i][j] < t) for the N x N field U and a finite threshold t -- a strict comparison in
 * double on the stored element (an fp32 handle's element widened); a NaN pixel and a pixel equal to t are background.
 * Windows: X padded with one ring of background has (N+1)^2 windows of 2 x 2 pixels; window (i, j), 0 <= i, j <= N,
 * holds X[i-1][j-1], X[i-1][j], X[i][j-1], X[i][j], pixels outside the grid being 0.
 * Classes: every window is counted by its number n = 0 .. 4 of foreground pixels, the n = 2 windows apart as the two
 * diagonal patterns (QD) and the four adjacent ones (Q2).
 * Border count: the foreground pixels of row 0, plus row N-1, plus column 0, plus column N-1 (a corner pixel counts
 * twice): the foreground pixel edges that lie on the box.
 * Result: the seven int64 words Q0, Q1, Q2, QD, Q3, Q4, border at the indices below.  What follows from them is exact
 * integer arithmetic and left to the caller (chsimpy_amd/morphology.py):
 *   n_A = (Q1 + 2 Q2 + 2 QD + 3 Q3 + 4 Q4) / 4   foreground pixels; SA = n_A / N^2
 *   perimeter = Q1 + Q2 + 2 QD + Q3               unit edges between foreground and background, the ring included
 *   perimeter_inner = perimeter - border          4-adjacent unlike pixel pairs inside the grid
 *   euler8 = (Q1 - Q3 - 2 QD) / 4                 8-connected foreground components minus 4-connected holes
 *   euler4 = (Q1 - Q3 + 2 QD) / 4                 4-connected foreground components minus 8-connected holes
 * Works on any handle that holds a field (else CHS_ESTATE), between two chs_step_n calls too: one sweep that reads the
 * field alone and writes buffers of its own, so the run does not notice it, and integer sums, so two looks return the
 * same bits.  CHS_EINVAL for a null argument or a threshold that is not finite. */
#define CHS_MORPH_WORDS 7
#define CHS_MORPH_Q0 0
#define CHS_MORPH_Q1 1
#define CHS_MORPH_Q2 2
#define CHS_MORPH_QD 3
#define CHS_MORPH_Q3 4
#define CHS_MORPH_Q4 5
#define CHS_MORPH_BORDER 6
int chs_morphology(chs_handle h, double threshold, int64_t out[CHS_MORPH_WORDS]);
/* Device time (ms, HIP events) of the handle's last chs_morphology, both kernels.  CHS_ESTATE before the first look. */
int chs_morphology_last_ms(chs_handle h, double* ms);

/* ---- Connected components of the thresholded field: droplet count, sizes, spanning ---------
 * Foreground, for the N x N field U and a finite threshold t:
 *   side = CHS_CC_BELOW: X[i][j] = ((double)U[i][j] < t), exactly the foreground of chs_morphology: a NaN pixel and a
 *     pixel equal to t are background;
 *   side = CHS_CC_ABOVE: the complement inside the grid, !((double)U[i][j] < t): a NaN pixel and a pixel equal to t
 *     are foreground.
 * Connectivity: 4 joins edge neighbours, 8 joins edge and corner neighbours.  No wrap-around; nothing outside the grid
 * is foreground.
 * Components: a component is a maximal connected set of foreground pixels; its `first` is the smallest linear index
 * i*N + j of its pixels; the components are numbered 0 .. C-1 by ascending `first`.  That numbering is unique, so a
 * look returns the same bits at every call, whatever order the device worked in.
 * Table: one row of CHS_CC_COLS int32 per component: first, area, imin, imax, jmin, jmax (the bounding box, inclusive).
 * Summary: CHS_CC_WORDS int64 words at the indices below:
 *   COUNT          C
 *   AREA           foreground pixels = the sum of the areas
 *   LARGEST        the largest area, 0 if there is no component
 *   SUMSQ          the sum of area^2 (at most N^4: fits up to N = 8192)
 *   INNER          components whose bounding box touches none of rows 0 and N-1 and columns 0 and N-1
 *   SPANNING       components with imin == 0 && imax == N-1, or jmin == 0 && jmax == N-1
 *   LARGEST_FIRST  the `first` of the largest component, the smallest `first` on a tie, -1 if there is none
 * Labels: int32 [N][N], the component number of the pixel, -1 for background.
 * With the words of chs_morphology at the same t: euler8 = COUNT(below, 8) - INNER(above, 4) and
 * euler4 = COUNT(below, 4) - INNER(above, 8).
 * A look works on any handle that holds a field (else CHS_ESTATE), between two chs_step_n calls too: it reads the field
 * alone and writes buffers of its own (allocated at the first look, freed with the handle), so the run does not notice
 * it; everything is integer, so two looks return the same bits.  Table and labels of the last look stay available as a
 * snapshot until the next look.  Every look checks its own labelling in the sweep that gathers the table (equal labels
 * across every joined pixel pair, every label a root no larger than its pixel) and the caps of its loops: a failed
 * check returns CHS_ECHECK and chs_last_error says which.  CHS_EINVAL for a null argument, a threshold that is not
 * finite, a connectivity other than 4 or 8, a side other than 0 or 1, N above 16384, or `rows` not the COUNT of the
 * last look; CHS_ESTATE for _table / _labels / _last_ms without a look. */
#define CHS_CC_WORDS 7
#define CHS_CC_COUNT 0
#define CHS_CC_AREA 1
#define CHS_CC_LARGEST 2
#define CHS_CC_SUMSQ 3
#define CHS_CC_INNER 4
#define CHS_CC_SPANNING 5
#define CHS_CC_LARGEST_FIRST 6
#define CHS_CC_COLS 6
#define CHS_CC_BELOW 0
#define CHS_CC_ABOVE 1
int chs_components(chs_handle h, double threshold, int32_t connectivity, int32_t side, int64_t out[CHS_CC_WORDS]);
int chs_components_table(chs_handle h, int64_t rows, int32_t* out);   /* [rows][CHS_CC_COLS]; rows == COUNT of the last look */
int chs_components_labels(chs_handle h, int32_t* out);                /* [N][N] of the last look */
/* Device time (ms, HIP events) of the handle's last look, first launch to last (the host's wait for the count in it). */
int chs_components_last_ms(chs_handle h, double* ms);
/* The extents of the tile a workgroup labels in LDS (what the tests size their fields by). */
int chs_components_tile(int32_t* rows, int32_t* cols);

/* ---- Distance transform of the thresholded field: domain widths, widest point, histogram ----
 * Foreground X: exactly that of chs_components.  side = CHS_CC_BELOW: X[i][j] = ((double)U[i][j] < t), a NaN pixel and
 * a pixel equal to t are background; side = CHS_CC_ABOVE: the complement inside the grid.  t is finite.
 * Squared distance: D2[i][j], an int32, is 0 for a background pixel and, for a foreground pixel, the minimum over all
 * background pixels (k, l) OF THE GRID of (i-k)^2 + (j-l)^2: the exact squared Euclidean distance to the nearest
 * background pixel.  No wrap-around, and the box walls are not background (scipy.ndimage.distance_transform_edt's
 * convention).  A grid without any background pixel has D2 = CHS_DT_INF = 1 << 30 everywhere: above 2 (N-1)^2 for
 * every N a handle takes, and d^2 + CHS_DT_INF stays inside int32.
 * Radius bin of a foreground pixel: k = isqrt(D2), k^2 <= D2 < (k+1)^2, computed in integers.
 * Histogram: hist[k], int64, the foreground pixels in bin k; its length is chs_distance_bins(N) = isqrt(2 (N-1)^2) + 1;
 * CHS_DT_INF pixels are in no bin.
 * Summary: CHS_DT_WORDS int64 words at the indices below:
 *   FG           foreground pixels
 *   D2MAX        the largest D2 over the foreground pixels with D2 < CHS_DT_INF, 0 if there is none
 *   D2MAX_FIRST  the smallest linear index i*N + j attaining D2MAX; -1 if FG == 0 or every foreground pixel is INF
 *                (the maximum of (D2, -index), a total order: every reduction order gives the same words)
 *   SUMD2        the sum of D2 over those same pixels
 *   NINF         pixels with D2 == CHS_DT_INF: 0 or N^2
 * A look works on any handle that holds a field (else CHS_ESTATE), between two chs_step_n calls too: it reads the field
 * alone and writes buffers of its own (allocated at the first look, freed with the handle), so the run does not notice
 * it; everything is integer, so two looks return the same bits.  Histogram and map of the last look stay available
 * until the next look.  Every loop of the kernels has a cap it cannot reach; one that reaches it makes the look return
 * CHS_ECHECK and chs_last_error names it.  CHS_EINVAL for a null argument, a threshold that is not finite, a side other
 * than 0 or 1, or nbins != chs_distance_bins(N) (the message gives the expected value); CHS_ESTATE for _hist / _map /
 * _last_ms without a look. */
#define CHS_DT_WORDS 5
#define CHS_DT_FG 0
#define CHS_DT_D2MAX 1
#define CHS_DT_D2MAX_FIRST 2
#define CHS_DT_SUMD2 3
#define CHS_DT_NINF 4
#define CHS_DT_INF (1 << 30)
int32_t chs_distance_bins(int32_t N);   /* 0 for N < 1 */
int chs_distance(chs_handle h, double threshold, int32_t side, int64_t out[CHS_DT_WORDS]);
int chs_distance_hist(chs_handle h, int32_t nbins, int64_t* out);   /* [nbins] of the last look */
int chs_distance_map(chs_handle h, int32_t* out);                   /* [N][N] D2 of the last look */
/* Device time (ms, HIP events) of the handle's last look, first launch to last. */
int chs_distance_last_ms(chs_handle h, double* ms);
/* The kernels' geometry (what the tests size their fields by): the rows of a band of the vertical pass, and the
 * consecutive pixels of a row that one wavefront pass of the horizontal pass covers. */
int chs_distance_tile(int32_t* band_rows, int32_t* row_chunk);

/* ---- Local thickness of a phase of the thresholded field: the pore-size distribution ----
 * Foreground X and squared distance D2: exactly those of chs_distance -- `side`, the NaN and threshold conventions, the
 * walls that are no background, CHS_DT_INF.  A thickness look is a distance look first, on the handle's distance buffers:
 * afterwards chs_distance_hist / _map return that look's D2.
 * Local thickness: T2[p], an int32, is 0 for a background pixel and, for a foreground pixel p,
 *     T2[p] = max { D2[c] : c foreground, D2[c] < CHS_DT_INF, |p - c|^2 < D2[c] }
 * the squared radius of the largest disc that fits inside the phase and covers p (Hildebrand and Rueegsegger): the open
 * disc of squared radius D2[c] about c holds no background pixel.  Discs are clipped at the walls; a disc may poke out of
 * the grid.  A grid without any background pixel has T2 = CHS_DT_INF everywhere, with KEPT = WORK = 0.
 * Radius bin of a foreground pixel: k = isqrt(T2), as in chs_distance.  Histogram: hist[k], int64, the foreground pixels
 * in bin k; its length is chs_distance_bins(N); CHS_DT_INF pixels are in no bin.
 * The centres that are painted.  E(R, a, b) is the maximum of |q - (a, b)|^2 over the lattice points q with |q|^2 < R: by
 * symmetry one function of R for the four axis neighbours (a, b) and one for the four diagonal ones,
 * chs_thickness_reach(R, diagonal) -- the function the kernel compiles; 0 for R outside [1, CHS_DT_INF).  A centre c with
 * R = D2[c] is DROPPED iff one of its 8 neighbours c' = c + (a, b) inside the grid is foreground, has D2[c'] <
 * CHS_DT_INF and D2[c'] > E(R, a, b): every pixel of c's disc is then inside the disc of c', whose value is larger.
 * E >= R, so D2 rises strictly along a chain of drops and every chain ends at a kept centre: the map does not depend on
 * the rule, KEPT and WORK do.  With rho(R) = isqrt(R - 1), the largest integer with rho^2 < R, WORK is the sum over the
 * kept centres of (2 rho + 1)^2: the unclipped bounding boxes, known before anything is painted.
 * Summary: CHS_TH_WORDS int64 words at the indices below:
 *   FG      foreground pixels
 *   T2MAX   the largest T2 over the foreground pixels with T2 < CHS_DT_INF, 0 if there is none
 *   NMAX    the pixels with T2 == T2MAX (0 if there is none)
 *   SUMT2   the sum of T2 over the foreground pixels with T2 < CHS_DT_INF
 *   NINF    pixels with T2 == CHS_DT_INF: 0 or N^2
 *   KEPT    the centres the rule keeps
 *   WORK    the sum of their bounding boxes
 * The work limit.  The look can be arbitrarily expensive on a field no run produces (one background pixel in a full
 * grid: WORK of the order N^4).  max_work = 0 means chs_thickness_work_default(N) = K N^2 (K: DESIGN.md section 3m; 0
 * for N < 1); a negative max_work or one above 16 times the default is CHS_EINVAL.  When WORK > max_work nothing is
 * painted -- the paint kernel reads WORK on the device and returns -- and the call returns CHS_ELIMIT, chs_last_error
 * naming both numbers: that look has no thickness result (its fetches return CHS_ESTATE), the distance look of the same
 * call is complete and can be fetched; of `out` KEPT and WORK are set and every other word is 0.
 * A look works on any handle that holds a field (else CHS_ESTATE), between two chs_step_n calls too: it reads the field
 * alone and writes buffers of its own, so the run does not notice it; everything is integer -- maxima and sums -- so two
 * looks return the same bits.  Histogram and map of the last look stay available until the next look.  The look checks
 * itself: FG, T2MAX and NINF equal the distance look's FG, D2MAX and NINF, no scan reached its cap; a violation is
 * CHS_ECHECK.  CHS_EINVAL (the last look undisturbed) for a null argument, a threshold that is not finite, a side other
 * than 0 or 1, max_work out of range, or nbins != chs_distance_bins(N) (the message gives the expected value);
 * CHS_ESTATE for _hist / _map / _last_ms without a look. */
#define CHS_TH_WORDS 7
#define CHS_TH_FG 0
#define CHS_TH_T2MAX 1
#define CHS_TH_NMAX 2
#define CHS_TH_SUMT2 3
#define CHS_TH_NINF 4
#define CHS_TH_KEPT 5
#define CHS_TH_WORK 6
int64_t chs_thickness_work_default(int32_t N);            /* 0 for N < 1 */
int32_t chs_thickness_reach(int32_t R, int32_t diagonal);  /* E(R, axis) or E(R, diagonal) */
int chs_thickness(chs_handle h, double threshold, int32_t side, int64_t max_work, int64_t out[CHS_TH_WORDS]);
int chs_thickness_hist(chs_handle h, int32_t nbins, int64_t* out);   /* [nbins] of the last look */
int chs_thickness_map(chs_handle h, int32_t* out);                   /* [N][N] T2 of the last look */
/* Device time (ms, HIP events) of the handle's last look, the distance look inside included. */
int chs_thickness_last_ms(chs_handle h, double* ms);

/* ---- Geodesic look at a phase of the thresholded field: tortuosity and reach ----
 * Foreground, `side` (0 below, 1 above) and `connectivity` (4 or 8) are those of chs_components, with no wrap-around.  A
 * geodesic look is a components look first, on the handle's component buffers: afterwards chs_components_table / _labels
 * return that look.
 * Source and target.  `source` is one of four walls: 0 is row 0, 1 is row N-1, 2 is column 0, 3 is column N-1.  The
 * target is the opposite wall.  The depth k of a pixel is its distance in pixels from the source wall along that axis, 0
 * to N-1.
 * Steps.  A path moves from a foreground pixel to a foreground neighbour.  At connectivity 4 an axial step costs 1 and
 * there is no diagonal step: UNIT = 1.  At connectivity 8 an axial step costs 3 and a diagonal step 4 (the 3-4 chamfer
 * metric): UNIT = 3.  A diagonal step needs only its two end pixels to be foreground -- the rule that makes them one
 * component at connectivity 8.  In free space G / UNIT lies within [0.9428, 1.0541] of the Euclidean length.
 * The map.  G[p] is an int32: -1 for background, 0 for a foreground pixel on the source wall, otherwise the smallest
 * cost of a path from any such pixel to p; CHS_GEO_INF (INT32_MAX) marks a foreground pixel that no path reaches.  At N =
 * 8192 a path costs less than 4 * 2^26, so int32 holds.
 * Result words: CHS_GEO_WORDS int64 words at the indices below:
 *   FG               foreground pixels
 *   SOURCES          foreground pixels on the source wall
 *   REACHED          reached pixels, sources included
 *   TARGET_FG        foreground pixels on the target wall
 *   TARGET_REACHED   reached pixels on the target wall
 *   GMIN_TARGET      smallest G on the target wall; -1 when none is reached
 *   GMIN_TARGET_POS  smallest position along the wall (column for sources 0 and 1, row for 2 and 3) that has
 *                    GMIN_TARGET; -1 when none
 *   GSUM_TARGET      sum of G over the reached target pixels
 *   GMAX             largest G of a reached pixel; -1 when none
 *   GMAX_FIRST       smallest linear index i*N + j with G == GMAX; -1 when none
 *   GSUM             sum of G over the reached pixels
 *   UNIT             1 or 3
 *   CC_COUNT         components of the components look
 *   CC_REACHED       components that hold a source pixel
 *   ROUNDS           relaxation rounds used (0 without a source pixel)
 *   LIMIT            the round limit that applied
 * Every word but ROUNDS is unique for a given field and arguments; ROUNDS may differ from look to look and is only ever
 * compared with bounds.
 * Histogram: chs_geodesic_bins(N) = 4N bins of int64.  Bin d counts the reached pixels with G / UNIT == d (integer
 * division); the last bin takes everything at or beyond 4N - 1.  Its running sum is the accessible amount of phase within
 * depth d of the face.
 * Profile: [N][3] int64: for every depth k the foreground pixels, the reached pixels and the sum of G over the reached
 * pixels of that line.  Line N-1 repeats TARGET_FG, TARGET_REACHED and GSUM_TARGET.
 * The round limit.  The map is relaxed tile by tile (64 x 64) in rounds, a launch each, until no tile is active.
 * max_rounds = 0 means chs_geodesic_rounds_default(N) = 32 nt^2 + 64, nt = ceil(N / 64): the rounds of a one-pixel
 * serpentine corridor through the whole grid, plus slack.  A negative max_rounds or one above 16 times the default is
 * CHS_EINVAL.  When the limit is used up and tiles are still active the call returns CHS_ELIMIT, chs_last_error naming
 * the rounds and the limit: there is no geodesic result (its fetches return CHS_ESTATE), the components look of the call
 * stays valid; of `out` ROUNDS and LIMIT are set and every other word is 0.
 * A look works on any handle that holds a field (else CHS_ESTATE), between two chs_step_n calls too: it reads the labels
 * of its components look and writes buffers of its own, so the run does not notice it.  The look checks itself in the
 * sweep that fills the words: (a) for every reached pixel p and every foreground neighbour q under the step rule, G[q] <=
 * G[p] + w; (b) every reached pixel with G > 0 has a neighbour q with G[q] + w == G[p]; (c) G == 0 holds exactly on the
 * foreground of the source wall; (d) no unreached foreground pixel has a reached foreground neighbour -- (a) to (c)
 * together prove that G holds the shortest-path costs.  Then REACHED equals the summed area of the components whose table
 * row holds a source pixel, TARGET_REACHED > 0 exactly when one of them touches the target wall, and REACHED <= FG.  A
 * violation is CHS_ECHECK.  The argument checks, in this order and before the last look is touched: a null argument, a
 * threshold that is not finite, the connectivity, the side, the source, max_rounds (all CHS_EINVAL), then the field
 * (CHS_ESTATE).  CHS_EINVAL for nbins != chs_geodesic_bins(N) (the message gives the expected value); CHS_ESTATE for
 * _hist / _profile / _map / _last_ms without a look. */
#define CHS_GEO_INF 0x7fffffff
#define CHS_GEO_WORDS 16
#define CHS_GEO_FG 0
#define CHS_GEO_SOURCES 1
#define CHS_GEO_REACHED 2
#define CHS_GEO_TARGET_FG 3
#define CHS_GEO_TARGET_REACHED 4
#define CHS_GEO_GMIN_TARGET 5
#define CHS_GEO_GMIN_TARGET_POS 6
#define CHS_GEO_GSUM_TARGET 7
#define CHS_GEO_GMAX 8
#define CHS_GEO_GMAX_FIRST 9
#define CHS_GEO_GSUM 10
#define CHS_GEO_UNIT 11
#define CHS_GEO_CC_COUNT 12
#define CHS_GEO_CC_REACHED 13
#define CHS_GEO_ROUNDS 14
#define CHS_GEO_LIMIT 15
int32_t chs_geodesic_bins(int32_t N);              /* 4N; 0 for N < 1 */
int64_t chs_geodesic_rounds_default(int32_t N);    /* 32 nt^2 + 64; 0 for N < 1 */
int chs_geodesic(chs_handle h, double threshold, int32_t connectivity, int32_t side, int32_t source, int64_t max_rounds,
                 int64_t out[CHS_GEO_WORDS]);
int chs_geodesic_hist(chs_handle h, int32_t nbins, int64_t* out);   /* [nbins] of the last look */
int chs_geodesic_profile(chs_handle h, int64_t* out);               /* [N][3] of the last look */
int chs_geodesic_map(chs_handle h, int32_t* out);                   /* [N][N] G of the last look */
/* Device time (ms, HIP events) of the handle's last look, the components look inside included; _relax_ms: of its
 * relaxation rounds alone, the host's looks at the round counter between them included. */
int chs_geodesic_last_ms(chs_handle h, double* ms);
int chs_geodesic_relax_ms(chs_handle h, double* ms);

/* ---- Skeleton of a phase of the thresholded field: its medial network ----
 * Foreground X and squared distance D2: exactly those of chs_distance -- `side`, the NaN and threshold conventions,
 * CHS_DT_INF.  A skeleton look is a distance look first, on the handle's distance buffers: afterwards chs_distance_hist /
 * _map return that look's D2.  The mask that is thinned is D2 > 0.  For the thinning everything outside the box is
 * background; the foreground is 8-connected and the background 4-connected; there is no connectivity argument.
 * Neighbourhood: the neighbours of a pixel are x0 .. x7 clockwise from north: N, NE, E, SE, S, SW, W, NW (north is row
 * i - 1, east column j + 1).  B = sum of x_k.  The Yokoi 8-connectivity number is
 *     Y = sum over k in {0, 2, 4, 6} of  (not x_k) and (x_{k+1} or x_{k+2}),   indices mod 8.
 * Sub-iteration: one of direction d deletes, synchronously (all pixels read, then all deletions), every foreground pixel
 * whose neighbour in direction d is background, with Y == 1 and B >= 2.  Sub-iteration i = 1, 2, ... has direction
 * (N, S, E, W)[(i - 1) mod 4].  This is Rosenfeld's directional deletion of simple border points that are no end points:
 * it keeps the 8-components of the phase and the 4-components of the background.
 * Skeleton: the plane after the first four consecutive sub-iterations that delete nothing; SUBITERS is the index of the
 * last sub-iteration that deleted a pixel, 0 if none did.  Every sub-iteration is a function of the plane before it, so
 * plane and SUBITERS are unique: the device returns the bits of the numpy model (chsimpy_amd/skeleton.py).
 * Result words: CHS_SK_WORDS int64 words at the indices below; B and Y are taken in the skeleton:
 *   FG          foreground pixels
 *   PIXELS      skeleton pixels
 *   ISOLATED    skeleton pixels with B = 0
 *   ENDS        skeleton pixels with B = 1
 *   Y1 .. Y4    skeleton pixels by Yokoi number: edge, link, branch, crossing (Y = 0 is the rest)
 *   AXIAL       pairs of skeleton pixels that are 4-adjacent
 *   DIAGONAL    pairs of skeleton pixels that are diagonally adjacent
 *   SUMD2       the sum of D2 over the skeleton pixels with D2 < CHS_DT_INF
 *   D2MAX       the largest such D2, 0 if there is none
 *   D2MIN_LINK  the smallest D2 over the Y == 2 pixels, the narrowest neck; 0 if there is none (CHS_DT_INF where the grid
 *               has no background pixel)
 *   NINF        skeleton pixels with D2 == CHS_DT_INF
 *   EULER8      the Euler number of the skeleton at 8-connectivity, from 2 x 2 pattern counts:
 *               PIXELS - AXIAL - DIAGONAL + (windows of exactly three pixels) + 3 (full windows); it equals that of the
 *               phase, (Q1 - Q3 - 2 QD) / 4 of chs_morphology
 *   SUBITERS    as above
 *   LIMIT       the limit of this look
 * Histogram: hist[k], int64, length chs_distance_bins(N): the skeleton pixels with isqrt(D2) == k, the width distribution
 * along the network; CHS_DT_INF pixels are in no bin.
 * Plane: N x ceil(N / 64) uint64 words; bit j of word w of a row is column 64 w + j; the bits at or beyond N are zero.
 * The limit.  max_subiters = 0 means chs_skeleton_subiters_default(N) = 4 N + 64: twice what a full grid needs (2 N or 2 N + 1
 * with its four quiet sub-iterations) plus slack -- a searched bound, not a proven one; 0 for
 * N < 1.  A negative max_subiters or one above 16 defaults is CHS_EINVAL.  A look whose SUBITERS + 4 exceeds the limit --
 * the limit used up while a pixel was deleted in its last four sub-iterations -- returns CHS_ELIMIT, chs_last_error naming
 * both numbers: that look has no skeleton result (its fetches return CHS_ESTATE), the distance look of the same call is
 * complete and can be fetched; of `out` SUBITERS (the last deleting sub-iteration seen) and LIMIT are set and every other
 * word is 0.
 * A look works on any handle that holds a field (else CHS_ESTATE), between two chs_step_n calls too: it reads the field
 * alone (through the distance look) and writes buffers of its own, so the run does not notice it; everything is integer,
 * so two looks return the same bits.  Histogram and plane of the last look stay available until the next look.  The look
 * checks itself: EULER8 equals the Euler number of the phase, PIXELS <= FG, FG equals the distance look's, PIXELS ==
 * ISOLATED + ENDS + (pixels with B >= 2), SUBITERS + 4 <= the sub-iterations issued; a violation is CHS_ECHECK.
 * CHS_EINVAL (the last look undisturbed) for a null argument, a threshold that is not finite, a side other than 0 or 1,
 * max_subiters out of range, or nbins != chs_distance_bins(N) (the message gives the expected value); CHS_ESTATE for
 * _hist / _plane / _last_ms / _thin_ms without a look. */
#define CHS_SK_WORDS 17
#define CHS_SK_FG 0
#define CHS_SK_PIXELS 1
#define CHS_SK_ISOLATED 2
#define CHS_SK_ENDS 3
#define CHS_SK_Y1 4
#define CHS_SK_Y2 5
#define CHS_SK_Y3 6
#define CHS_SK_Y4 7
#define CHS_SK_AXIAL 8
#define CHS_SK_DIAGONAL 9
#define CHS_SK_SUMD2 10
#define CHS_SK_D2MAX 11
#define CHS_SK_D2MIN_LINK 12
#define CHS_SK_NINF 13
#define CHS_SK_EULER8 14
#define CHS_SK_SUBITERS 15
#define CHS_SK_LIMIT 16
int64_t chs_skeleton_subiters_default(int32_t N);   /* 4 N + 64; 0 for N < 1 */
int chs_skeleton(chs_handle h, double threshold, int32_t side, int64_t max_subiters, int64_t out[CHS_SK_WORDS]);
int chs_skeleton_hist(chs_handle h, int32_t nbins, int64_t* out);   /* [nbins] of the last look */
int chs_skeleton_plane(chs_handle h, uint64_t* out);                /* [N][ceil(N / 64)] of the last look */
/* Device time (ms, HIP events) of the handle's last look, the distance look inside included; _thin_ms: of its
 * sub-iterations alone, the host's looks at the counter between them included. */
int chs_skeleton_last_ms(chs_handle h, double* ms);
int chs_skeleton_thin_ms(chs_handle h, double* ms);

/* ---- Transport look at a phase of the thresholded field: effective diffusivity ----
 * Foreground and walls.  `threshold`, `side` (0 below, 1 above) and the NaN convention are those of chs_components at
 * connectivity 4, with no wrap-around.  A transport look is a components look at connectivity 4 first, on the handle's
 * component buffers: afterwards chs_components_table / _labels return that look.  `source` is 0 to 3 as in chs_geodesic
 * (0 is row 0, 1 is row N-1, 2 is column 0, 3 is column N-1); the target is the opposite wall; the depth k of a pixel is
 * its distance from the source wall along that axis.
 * Active set.  The active pixels are those of the components whose bounding box touches both the source wall and the
 * target wall.  Every other pixel carries no flux and takes no part in the solve; this also keeps the system non-singular.
 * System.  One unknown c_p per active pixel.  Two 4-adjacent active pixels share a bond of conductance 1.  An active pixel
 * on the source wall has a bond of conductance 2 to the wall face, which is held at c = 1 (the face is half a pixel away);
 * an active pixel on the target wall has a bond of conductance 2 to the wall face, which is held at c = 0.  No flux passes
 * through the other two walls or into pixels that are not active.  A c = b is the balance of every pixel: b_p = 2 on the
 * source wall and 0 elsewhere; A is symmetric positive definite.
 * Results.  F_in = sum over the source wall of 2 (1 - c_p); F_out = sum over the target wall of 2 c_p; cut[k], k = 0 .. N,
 * is the flux through the face between depth k-1 and depth k, so cut[0] = F_in and cut[N] = F_out.  For the exact
 * solution all cuts equal F*, and D_eff / D_0 = F* (the box is square and the difference of c is 1).  The formation factor
 * is 1 / F*; with the porosity eps = FG / N^2 the tortuosity factor is eps / F*.
 * Certificate.  With r = b - A c evaluated from the returned c the following hold exactly (maximum principle: the adjoint
 * potentials lie in [0, 1]): |F_out - F*| <= |r|_1 and |F_in - F*| <= |r|_1; |cut[k] - F_out| = |sum over depth >= k of
 * r_p| <= |r|_1.
 * Acceptance.  A look succeeds only if RES1 <= tol min(F_in, F_out), RES1 being the 1-norm of the true residual,
 * recomputed from the final c in a closing sweep; the recurrence residual of the iteration does not count.  `tol` is the
 * relative accuracy of D_eff that the caller asks for, in [1e-12, 1e-2]; 1e-6 is what the Python side passes by default.
 * The look checks this itself, and that every cut lies within RES1 of F_OUT up to the rounding of the sums; a
 * failure is CHS_ECHECK.
 * Words: CHS_TRN_WORDS int64 words at the indices below (CHS_TR_ is the tracking look's prefix):
 *   FG, ACTIVE           foreground pixels, active pixels
 *   CC_COUNT             components of the components look
 *   CC_SPANNING          those of them whose bounding box touches both walls
 *   SRC_PIXELS           active pixels on the source wall
 *   TGT_PIXELS           active pixels on the target wall
 *   BONDS                pairs of 4-adjacent active pixels
 *   ITERS                conjugate-gradient iterations
 *   CHECKS               closing sweeps, each a true residual
 *   LIMIT                the iteration limit that applied
 * Values: CHS_TRN_VALS doubles: F_IN, F_OUT, RES1, RESINF (the largest |r_p|), CUT_MIN, CUT_MAX (over the N + 1 cuts),
 * CSUM (the sum of c over the active pixels), TOL.
 * Profile: double [N+1][3], one row per face or depth k: cut[k], the sum of c at depth k, the active pixels at depth k;
 * row N holds zeros in the last two columns.
 * Map: double [N][N]: c on the active pixels, -1.0 on the background, -2.0 on foreground that is not active.
 * The solve is in fp64 whatever the engine's element type; the field is read only through the components look.  Plain
 * conjugate gradients without a preconditioner and without restarts, matrix-free on 64 x 64 tiles; every sum has a
 * fixed order, so two looks at one field return the same bits in map, profile and values.
 * No spanning component: ACTIVE == 0 is a good look; no iteration runs, ITERS = 0 and every value is 0 (TOL too): D_eff =
 * 0 is the answer.
 * The limit.  max_iters bounds the iterations: 0 means chs_transport_iters_default(N) = 48 N + 64, a searched bound
 * (evolved fields near the percolation threshold needed up to 21 N; at N = 4096 that is tens of thousands of iterations and many
 * seconds -- the look is meant for N <= 2048); a negative max_iters or one above 16 defaults is CHS_EINVAL.  A solve that is
 * not accepted within the limit returns CHS_ELIMIT, chs_last_error naming the iterations and the limit: ITERS and LIMIT
 * are filled and every other word and value is 0; there is no transport result (its fetches return CHS_ESTATE); the
 * components look of the call is complete.
 * A look works on any handle that holds a field (else CHS_ESTATE), between two chs_step_n calls too: it writes buffers of
 * its own, so the run does not notice it.  The argument checks, in this order and before the last look is touched: a null
 * argument, a threshold that is not finite, the side, the source, tol, max_iters (all CHS_EINVAL), then the field
 * (CHS_ESTATE).  CHS_ESTATE for _profile / _map / _last_ms / _solve_ms without a look. */
#define CHS_TRN_WORDS 10
#define CHS_TRN_FG 0
#define CHS_TRN_ACTIVE 1
#define CHS_TRN_CC_COUNT 2
#define CHS_TRN_CC_SPANNING 3
#define CHS_TRN_SRC_PIXELS 4
#define CHS_TRN_TGT_PIXELS 5
#define CHS_TRN_BONDS 6
#define CHS_TRN_ITERS 7
#define CHS_TRN_CHECKS 8
#define CHS_TRN_LIMIT 9
#define CHS_TRN_VALS 8
#define CHS_TRN_F_IN 0
#define CHS_TRN_F_OUT 1
#define CHS_TRN_RES1 2
#define CHS_TRN_RESINF 3
#define CHS_TRN_CUT_MIN 4
#define CHS_TRN_CUT_MAX 5
#define CHS_TRN_CSUM 6
#define CHS_TRN_TOL 7
int64_t chs_transport_iters_default(int32_t N);    /* 48 N + 64; 0 for N < 1 */
int chs_transport(chs_handle h, double threshold, int32_t side, int32_t source, double tol, int64_t max_iters,
                  int64_t words[CHS_TRN_WORDS], double vals[CHS_TRN_VALS]);
int chs_transport_profile(chs_handle h, double* out);   /* [N + 1][3] of the last look */
int chs_transport_map(chs_handle h, double* out);       /* [N][N] of the last look */
/* Device time (ms, HIP events) of the handle's last look, the components look inside included; _solve_ms: of its
 * iterations and closing sweeps alone, the host's looks at the scalars between them included. */
int chs_transport_last_ms(chs_handle h, double* ms);
int chs_transport_solve_ms(chs_handle h, double* ms);

/* ---- Chord lengths (linear intercepts) of both phases, along rows and columns ----
 * For the N x N field U and a finite threshold t:
 * Phase 0 is the foreground of chs_components with CHS_CC_BELOW: X[i][j] = ((double)U[i][j] < t); a NaN pixel and a
 * pixel equal to t are not phase 0.  Phase 1 is the complement inside the grid.  There is no side argument: one look
 * gives both.
 * Direction CHS_CH_ROWS = 0: the lines are the rows, a chord runs along j.  Direction CHS_CH_COLS = 1: the lines are the
 * columns, a chord runs along i.
 * A chord is a maximal run of consecutive pixels of one phase within one line; its length c is in [1, N].  No
 * wrap-around.
 * Class CHS_CH_INNER = 0: both ends are bounded by the other phase.  Class CHS_CH_CUT = 1: the chord touches a wall: it
 * begins at index 0, or ends at N-1, or both; a run of length N is one cut chord.
 * Histogram: hist[phase][dir][cls][c], int64, 2*2*2*(N+1) entries in that order: the chords of length c.  Bin 0 is
 * always 0.  chs_chords_bins(N) = N + 1, and 0 for N < 1.
 * Summary: CHS_CH_WORDS = 24 int64 words, six per (phase, dir) in the order phase, dir, at the indices below: N_INNER,
 * SUM_INNER, SUM2_INNER, MAX_INNER, N_CUT, SUM_CUT -- the count, the sum of c, the sum of c^2 and the largest c of the
 * class (0 without one).  The largest value is N^3, inside int64 for every N a handle takes.
 * A look works on any handle that holds a field (else CHS_ESTATE), between two chs_step_n calls too: it reads the field
 * alone and writes buffers of its own (allocated at the first look, freed with the handle), so the run does not notice
 * it; everything is integer, so two looks return the same bits.  The histogram of the last look stays available until
 * the next look.  The look checks itself: per direction the chords of both phases and classes add up to N^2 pixels and
 * the cut chords of both phases are N to 2 N, and every loop of the kernels has a cap it cannot reach; a violation makes
 * the look return CHS_ECHECK and chs_last_error names it.  CHS_EINVAL for a null argument, a threshold that is not
 * finite or nbins != chs_chords_bins(N) (the message gives the expected value); CHS_ESTATE for _hist / _last_ms
 * without a look. */
#define CHS_CH_WORDS 24
#define CHS_CH_ROWS 0
#define CHS_CH_COLS 1
#define CHS_CH_INNER 0
#define CHS_CH_CUT 1
#define CHS_CH_N_INNER 0
#define CHS_CH_SUM_INNER 1
#define CHS_CH_SUM2_INNER 2
#define CHS_CH_MAX_INNER 3
#define CHS_CH_N_CUT 4
#define CHS_CH_SUM_CUT 5
int32_t chs_chords_bins(int32_t N);   /* 0 for N < 1 */
int chs_chords(chs_handle h, double threshold, int64_t out[CHS_CH_WORDS]);
int chs_chords_hist(chs_handle h, int32_t nbins, int64_t* out);        /* [2][2][2][nbins] of the last look */
/* Device time (ms, HIP events) of the handle's last look, first launch to last. */
int chs_chords_last_ms(chs_handle h, double* ms);
/* The kernels' geometry (what the tests size their fields by): the pixels of a line in one word, the lines of a
 * workgroup of the walk, and the lengths below which a chord goes to the workgroup's histogram. */
int chs_chords_tile(int32_t* word_bits, int32_t* lines_per_group, int32_t* local_bins);

/* ---- Composition: the values of the field themselves -- range, sums, histogram, central moments, exact order
 * statistics ----
 * Every value is the element widened to double first, for fp32 handles too.  A pixel is NaN, infinite or finite.
 * chs_composition, for a finite threshold t, 1 <= nbins <= CHS_CMP_MAX_BINS and a range [lo, hi] (both finite with
 * lo <= hi, or both NaN: the field's own MIN and MAX), in two sweeps over the field without a host round trip between:
 *   iw: N_TOTAL = N^2; N_NAN; N_INF, the pixels that are +inf or -inf; N_BELOW, the pixels with x < t (the foreground of
 *       chs_components with CHS_CC_BELOW: a NaN and x == t are not below, -inf is); N_UNDER, the pixels with x < lo, -inf
 *       among them; N_OVER, those with x > hi, +inf among them; NBINS as given.
 *   fw: MIN and MAX over the finite pixels (the infinite ones are counted by N_INF and would leave no range to bin);
 *       SUM and SUM_BELOW, the sums of x over the finite pixels and over the finite pixels below t; CENTER = SUM /
 *       (N_TOTAL - N_NAN - N_INF), brought into [MIN, MAX] where rounding left it an ulp outside; M2, M3, M4, the sums of (x - CENTER)^p over the finite pixels, not divided; LO, HI and
 *       SCALE = nbins / (HI - LO) in double, 0 unless HI > LO: the numbers the bins were formed with.
 *   the histogram, int64 [nbins]: a finite x with LO <= x <= HI is in bin min(nbins - 1, (int64)((x - LO) * SCALE)), a
 *       subtraction and a multiplication in double (a product that is not below nbins, a NaN product included, is
 *       bin nbins - 1).  A NaN pixel goes nowhere: sum(hist) + N_UNDER + N_OVER + N_NAN = N^2.
 * A field without a finite pixel is no error: MIN = MAX = CENTER = LO = HI = NaN (with the field's own range), SCALE = 0,
 * an empty histogram.
 * The float sums are bit for bit the same from look to look: every thread adds a fixed number of elements in a fixed
 * order, every workgroup stores its partial sums into a slot of its own and one workgroup reduces the slots by a fixed
 * tree; no float atomics.  Their error bound: DESIGN.md section 3h; chs_composition_tile gives its operands.
 * chs_composition_select: values[k] = the ranks[k]-th smallest pixel (0-based, ranks in [0, N^2), any order, repeats
 * allowed), exactly, in the order of np.sort: a NaN of either sign sorts last and comes back as a NaN; -0.0 and +0.0 are
 * neighbours and may come back as either.  1 <= nq <= CHS_CMP_MAX_RANKS.  A look of its own: it needs no chs_composition
 * before it and leaves the histogram of the last one where it is; chs_composition_last_ms reports the later of the two.
 * Both work on any handle that holds a field (else CHS_ESTATE), between two chs_step_n calls too: they read the field
 * alone and write buffers of their own (allocated at the first look, freed with the handle), so the run does not notice
 * them.  The histogram of the last chs_composition stays available until the next one.  The looks check themselves (the
 * pixels add up as above, N_BELOW <= N^2, MIN <= SUM / n <= MAX within the error bound of SUM, and for every selected rank r the keys below the one
 * found are at most r and r is below that count plus the count of keys equal to it): a violation is CHS_ECHECK and
 * chs_last_error names it.  CHS_EINVAL, the last look undisturbed: a null argument, a threshold that is not finite,
 * nbins outside [1, CHS_CMP_MAX_BINS], exactly one of lo and hi NaN, lo > hi, an infinite bound, nq outside
 * [1, CHS_CMP_MAX_RANKS], a rank outside [0, N^2), a fetch with another nbins than the look's.  CHS_ESTATE for _hist
 * without a chs_composition, for _last_ms without either. */
#define CHS_CMP_MAX_BINS 4096
#define CHS_CMP_MAX_RANKS 8
#define CHS_CMP_IWORDS 7
#define CHS_CMP_N_TOTAL 0
#define CHS_CMP_N_NAN 1
#define CHS_CMP_N_INF 2
#define CHS_CMP_N_BELOW 3
#define CHS_CMP_N_UNDER 4
#define CHS_CMP_N_OVER 5
#define CHS_CMP_NBINS 6
#define CHS_CMP_FWORDS 11
#define CHS_CMP_MIN 0
#define CHS_CMP_MAX 1
#define CHS_CMP_SUM 2
#define CHS_CMP_SUM_BELOW 3
#define CHS_CMP_CENTER 4
#define CHS_CMP_M2 5
#define CHS_CMP_M3 6
#define CHS_CMP_M4 7
#define CHS_CMP_LO 8
#define CHS_CMP_HI 9
#define CHS_CMP_SCALE 10
int chs_composition(chs_handle h, double threshold, int32_t nbins, double lo, double hi,
                    int64_t iw[CHS_CMP_IWORDS], double fw[CHS_CMP_FWORDS]);   /* lo and hi both NaN: the field's own min, max */
int chs_composition_hist(chs_handle h, int32_t nbins, int64_t* out);          /* [nbins] of the last look */
int chs_composition_select(chs_handle h, int32_t nq, const int64_t* ranks, double* values);
/* Device time (ms, HIP events) of the handle's last chs_composition or chs_composition_select, first launch to last. */
int chs_composition_last_ms(chs_handle h, double* ms);
/* The kernels' geometry: a workgroup of `threads` threads takes tiles of threads * elems_per_thread consecutive
 * elements, every max_groups-th one where the field has more tiles than that; the digits of the radix select have
 * digit_bits bits.  A thread adds E = elems_per_thread * ceil(tiles / groups) elements one after the other, with tiles =
 * ceil(N^2 / (threads * elems_per_thread)) and groups = min(tiles, max_groups); the trees above it are
 * D = log2(threads) + ceil(log2(max_groups)) deep. */
int chs_composition_tile(int32_t* elems_per_thread, int32_t* threads, int32_t* max_groups, int32_t* digit_bits);

/* ---- Two-point correlation: the pair counts of both phases at every displacement ----
 * For the N x N field U, a finite threshold t and an integer rmax with 1 <= rmax <= chs_two_point_max_r(N), where
 * chs_two_point_max_r(N) = min(N - 1, CHS_TP_MAX_R = 256), and 0 for N < 2:
 * Phases: those of chs_chords.  Phase 0 is X[i][j] = ((double)U[i][j] < t); a NaN pixel and a pixel equal to t are not
 * phase 0.  Phase 1 is the complement inside the grid.
 * Displacements: (dy, dx) with 0 <= dy <= rmax and -rmax <= dx <= rmax.  The other half-plane is the mirror image
 * (c(-dy, -dx) = c(dy, dx)) and is not stored.
 * Pair count: c[p][dy][dx + rmax], int64, laid out as [2][rmax + 1][2 rmax + 1]: the number of positions (i, j) for which
 * (i, j) and (i + dy, j + dx) are both inside the grid and both of phase p.  There is no wrap-around.  The window holds
 * pairs(dy, dx) = (N - dy)(N - |dx|) positions.  chs_two_point_size(N, rmax) = 2 (rmax + 1)(2 rmax + 1), and 0 for
 * arguments out of range.
 * Summary: CHS_TP_WORDS = 8 int64 words.  N_BELOW, N_ABOVE: c[p][0][rmax], the pixels of the phase.  ADJ_ROWS_BELOW,
 * ADJ_COLS_BELOW, ADJ_ROWS_ABOVE, ADJ_COLS_ABOVE: c[p] at (dy, dx) = (0, 1), the neighbours within a row, and at (1, 0),
 * the neighbours within a column.  SUM_BELOW, SUM_ABOVE: the sum of all entries of c[p].
 * Everything is an integer and every sum is order-free: two looks return the same bits.
 * A look works on any handle that holds a field (else CHS_ESTATE), between two chs_step_n calls too: it reads the field
 * alone and writes buffers of its own (allocated at the first look, freed with the handle; a look with another rmax
 * re-sizes the count table), so the run does not notice it.  The count table of the last look stays available until the
 * next look.  The look checks itself: N_BELOW + N_ABOVE = N^2; the row dy = 0 of both tables is symmetric in dx;
 * c[0] + c[1] <= pairs entry by entry and no entry is negative; a violation makes the look return CHS_ECHECK and
 * chs_last_error names it.  CHS_EINVAL, the last look undisturbed, for a null argument, a threshold that is not finite,
 * rmax out of range, N above 16384, or n != chs_two_point_size(N, rmax of the last look) on fetch (the message gives the
 * expected value); CHS_ESTATE for _counts / _last_ms without a look. */
#define CHS_TP_MAX_R 256
#define CHS_TP_WORDS 8
#define CHS_TP_N_BELOW 0
#define CHS_TP_N_ABOVE 1
#define CHS_TP_ADJ_ROWS_BELOW 2
#define CHS_TP_ADJ_COLS_BELOW 3
#define CHS_TP_ADJ_ROWS_ABOVE 4
#define CHS_TP_ADJ_COLS_ABOVE 5
#define CHS_TP_SUM_BELOW 6
#define CHS_TP_SUM_ABOVE 7
#define CHS_TP_CHUNK 2048 /* the pixels of a row that one workgroup of the pair kernel owns (chs_two_point_tile gives the rest) */
int32_t chs_two_point_max_r(int32_t N);                 /* 0 for N < 2 */
int64_t chs_two_point_size(int32_t N, int32_t rmax);    /* 0 for arguments out of range */
int chs_two_point(chs_handle h, double threshold, int32_t rmax, int64_t out[CHS_TP_WORDS]);
int chs_two_point_counts(chs_handle h, int64_t n, int64_t* out);   /* [2][rmax + 1][2 rmax + 1] of the last look */
/* Device time (ms, HIP events) of the handle's last look, first launch to last. */
int chs_two_point_last_ms(chs_handle h, double* ms);
/* The kernels' geometry (what the tests size their fields by): the pixels of a row in one word, the rows of a band of
 * the pair kernel, and the lanes of its workgroup; a workgroup owns band_rows rows of CHS_TP_CHUNK pixels. */
int chs_two_point_tile(int32_t* word_bits, int32_t* band_rows, int32_t* lanes);

/* ---- Sub-pixel interface: contour length, orientation and curvature of the level set U = t ----
 * Setting.  The N x N field U[i][j], i the row (y) and j the column (x), N >= 2; every value widened to double; a finite
 * threshold t.  A pixel is below when (double)U < t -- phase 0 of chs_chords: a NaN and a pixel equal to t are not below.
 * Cell (i, j), 0 <= i, j <= N - 2, has the corners a = U[i][j], b = U[i][j+1], c = U[i+1][j], d = U[i+1][j+1] and the
 * code below(a) + 2 below(b) + 4 below(c) + 8 below(d).
 * Vertices.  One on every grid edge whose two pixels p and q (p the one with the lower index) are unlike: lo the below
 * value, hi the other, s = (t - lo) / (hi - lo), s = 0.5 if either value is not finite; the vertex lies at the fraction s
 * from p if p is below and at 1 - s otherwise.  In cell coordinates a cell's vertices are T = (x_T, 0), B = (x_B, 1),
 * L = (0, y_L), R = (1, y_R).
 * Segments, from the first vertex to the second: codes 1, 14: L-T; 2, 13: T-R; 4, 11: L-B; 8, 7: B-R; 3, 12: L-R;
 * 5, 10: T-B; 6 (a saddle): T-R and L-B; 9 (a saddle): L-T and B-R -- in a saddle every below corner is cut off on its
 * own, the below phase being 4-connected as for the Euler number euler4.  For a segment from P to Q, every operation
 * rounded on its own: dx = Q.x - P.x, dy = Q.y - P.y, l = sqrt(dx dx + dy dy); txx = dx dx / l, txy = dx dy / l,
 * tyy = dy dy / l, each 0 where l == 0.  A cell's ell is the sum of its l, at most two terms in the order above.
 * Curvature, for a crossed cell that is no saddle and has 1 <= i, j <= N - 3, with A(di, dj) = U[i+di][j+dj]:
 *   ux  = ((A(0,1) + A(1,1)) - (A(0,0) + A(1,0))) 0.5,   uy = ((A(1,0) + A(1,1)) - (A(0,0) + A(0,1))) 0.5
 *   uxy = (A(1,1) - A(1,0)) - (A(0,1) - A(0,0))
 *   uxx = (((A(0,2) - A(0,1)) - (A(0,0) - A(0,-1))) + ((A(1,2) - A(1,1)) - (A(1,0) - A(1,-1)))) 0.25
 *   uyy = (((A(2,0) - A(1,0)) - (A(0,0) - A(-1,0))) + ((A(2,1) - A(1,1)) - (A(0,1) - A(-1,1)))) 0.25
 *   g2  = ux ux + uy uy,   kappa = ((uxx (uy uy) - (2 (ux uy)) uxy) + uyy (ux ux)) / (g2 sqrt(g2))
 * the divergence of grad U / |grad U|: positive where the below phase is convex, in 1 / pixel.  A crossed cell that is no
 * saddle and lacks the full stencil is a wall cell; one whose 16 stencil values are not all finite or whose kappa is not
 * finite is a bad cell.  Wall cells, bad cells and saddles take no part in the curvature results; they are counted.
 * Fixed point: fix(x) = (int64)(x 2^30), truncated; lengths are summed as fix(ell), order-free.
 * words, CHS_CT_WORDS int64: CELLS_ONE (one or three below corners), CELLS_TWO (codes 3, 5, 10, 12), SADDLES,
 *   VERTICES_ROWS and VERTICES_COLS (unlike neighbours within a row, within a column), ENDS (vertices on the four
 *   outermost grid lines), SEGMENTS, CELLS_CURV, CELLS_WALL, CELLS_BAD, L_FIX (fix(ell) over all cells), L_CURV_FIX (over
 *   the curvature cells), HIST_UNDER, HIST_OVER, N_BELOW, N_NONFINITE (the pixels that are NaN or infinite).
 * sums, CHS_CT_SUMS doubles: TXX, TXY, TYY over all segments; K1 = sum ell kappa, KA = sum ell |kappa|, K2 = sum ell
 *   (kappa kappa) over the curvature cells.  They are bit for bit the same from look to look: the crossed cells of a
 *   workgroup's tile are queued in row-major order, thread q adds the queue's entries q, q + threads, ... in that order,
 *   the workgroup joins its threads by a fixed tree into a slot of its own and one workgroup joins the slots, each of its
 *   threads every fin_threads-th slot in order and then a fixed tree; no float atomics.
 * The histogram, for 1 <= bins <= CHS_CT_MAX_BINS and a finite kmax > 0, with SCALE = bins / (2 kmax) in double: a
 *   curvature cell with kappa in [-kmax, kmax] is in bin min(bins - 1, (int64)((kappa + kmax) SCALE)); kappa < -kmax is
 *   counted by HIST_UNDER, kappa > kmax by HIST_OVER.  int64 [2][bins]: the cells per bin, then their fix(ell) per bin.
 * The map, if want_map != 0: double [2][N-1][N-1]: ell per cell, 0 where the cell is not crossed; then kappa per cell,
 *   NaN where the cell is not a curvature cell.  It exists until the next look; a look without want_map frees it.
 * A look works on any handle that holds a field (else CHS_ESTATE), between two chs_step_n calls too: it reads the field
 * alone and writes buffers of its own, so the run does not notice it.  The look checks itself: SEGMENTS = CELLS_ONE +
 * CELLS_TWO + 2 SADDLES; 2 SEGMENTS = 2 (VERTICES_ROWS + VERTICES_COLS) - ENDS; CELLS_CURV + CELLS_WALL + CELLS_BAD =
 * CELLS_ONE + CELLS_TWO; the histogram's cells + HIST_UNDER + HIST_OVER = CELLS_CURV; the histogram's lengths add up to
 * L_CURV_FIX at most, and to it when HIST_UNDER + HIST_OVER = 0; |TXX + TYY - L_FIX / 2^30| is within the sums' error
 * bound plus SEGMENTS 2^-30 (skipped where the sums are not finite); a violation is CHS_ECHECK and chs_last_error names
 * it.  CHS_EINVAL, the last look undisturbed: a null argument, a threshold or kmax that is not finite, kmax <= 0, bins
 * outside [1, CHS_CT_MAX_BINS], N < 2 or above 16384, a fetch with another size than the look's (the message gives the
 * expected value).  CHS_ESTATE for a fetch or _last_ms without a look, for _map after a look without want_map. */
#define CHS_CT_MAX_BINS 1024
#define CHS_CT_WORDS 16
#define CHS_CT_CELLS_ONE 0
#define CHS_CT_CELLS_TWO 1
#define CHS_CT_SADDLES 2
#define CHS_CT_VERTICES_ROWS 3
#define CHS_CT_VERTICES_COLS 4
#define CHS_CT_ENDS 5
#define CHS_CT_SEGMENTS 6
#define CHS_CT_CELLS_CURV 7
#define CHS_CT_CELLS_WALL 8
#define CHS_CT_CELLS_BAD 9
#define CHS_CT_L_FIX 10
#define CHS_CT_L_CURV_FIX 11
#define CHS_CT_HIST_UNDER 12
#define CHS_CT_HIST_OVER 13
#define CHS_CT_N_BELOW 14
#define CHS_CT_N_NONFINITE 15
#define CHS_CT_SUMS 6
#define CHS_CT_TXX 0
#define CHS_CT_TXY 1
#define CHS_CT_TYY 2
#define CHS_CT_K1 3
#define CHS_CT_KA 4
#define CHS_CT_K2 5
#define CHS_CT_FIX_BITS 30
int chs_contour(chs_handle h, double threshold, int32_t bins, double kmax, int32_t want_map, int64_t words[CHS_CT_WORDS],
                double sums[CHS_CT_SUMS]);
int chs_contour_hist(chs_handle h, int32_t bins, int64_t* out);   /* [2][bins] of the last look */
int chs_contour_map(chs_handle h, int64_t n, double* out);        /* n = 2 (N-1)^2: [2][N-1][N-1] of the last look */
/* Device time (ms, HIP events) of the handle's last look, first launch to last. */
int chs_contour_last_ms(chs_handle h, double* ms);
/* The kernels' geometry (what the tests size their fields by, and the operands of the sums' error bound): a workgroup of
 * `threads` threads owns tile_w x tile_h cells; a thread adds at most 2 tile_w tile_h / threads terms one after the other,
 * a thread of the finishing workgroup ceil(tiles / fin_threads) slots, tiles = ceil((N-1) / tile_w) ceil((N-1) / tile_h);
 * the trees above them are log2(threads) and log2(fin_threads) deep. */
int chs_contour_tile(int32_t* tile_w, int32_t* tile_h, int32_t* threads, int32_t* fin_threads);

/* ---- Droplet shapes: moments, perimeter, holes and composition of every component -----------
 * The foreground X, the connectivity (4 or 8), the side, the components and their numbering by ascending `first` are
 * exactly those of chs_components.  A shapes look labels the field itself, by running the phases of chs_components on the
 * handle's component buffers: a shapes look IS ALSO a components look of the same (threshold, connectivity, side), and
 * afterwards chs_components_table and chs_components_labels return that labelling.  One more sweep over the field, the
 * labels and the numbers then fills a table of its own, int64 [C][CHS_SH_COLS], one row per component k, which stays valid
 * until the next shapes look on the handle (a later chs_components does not touch it).
 * Pixel (i, j) has p = i N + j and x = (double)U[i][j].  Columns:
 *   FIRST      that of the component table
 *   AREA       pixels of k
 *   PAIRS_H    pixels (i, j) of k whose right neighbour (i, j+1) is foreground
 *   PAIRS_V    pixels (i, j) of k whose lower neighbour (i+1, j) is foreground
 *   PAIRS_D    connectivity 8 only, otherwise 0: the diagonal foreground pairs {(i,j), (i+1,j+1)} and {(i,j+1), (i+1,j)},
 *              each counted for the component of its upper pixel
 *   TRIPLES    connectivity 8 only, otherwise 0: the 2 x 2 cells with exactly three foreground pixels, counted for the
 *              component of the cell's first foreground pixel in the order a = (i,j), b = (i,j+1), c = (i+1,j),
 *              d = (i+1,j+1)
 *   QUADS      the 2 x 2 cells with four foreground pixels, counted for the component of the cell's upper left pixel
 *   WALL       unit pixel edges of k that lie on the grid's boundary (a corner pixel has two)
 *   SI, SJ, SII, SJJ, SIJ   the sums of i, j, i^2, j^2, i j over the pixels of k
 *   SU_FIX     the sum of fix(x) over the pixels of k with fabs(x) <= 4.0
 *   SUU_FIX    the sum of fix(x x) over the same pixels, the product rounded once in double
 *   N_OUTSIDE  pixels of k with !(fabs(x) <= 4.0): NaN, infinite, or far outside the physical range
 * fix(y) = (int64)(y 2^30), truncated (CHS_CT_FIX_BITS).  All pixels of a pair or a cell that is counted belong to one
 * component under the connectivity it is counted for; the "counted for" rules only make the owner unique.  With
 * N <= 16384 no sum reaches 2^63: SII, SJJ, SIJ stay below 2^28 2^28 = 2^56, SUU_FIX below 2^28 2^34 = 2^62.  Every cell is
 * an integer and every accumulation an integer add, so the table does not depend on the order the device worked in: it is
 * the numpy model's (chsimpy_amd/shapes.py) bit for bit, for both element types.
 * Summary, CHS_SH_WORDS int64: the seven words of chs_components; the column sums of AREA, PAIRS_H, PAIRS_V, PAIRS_D,
 * TRIPLES, QUADS, WALL, N_OUTSIDE; HOLES = the sum over k of 1 - euler_k, with euler_k = AREA - PAIRS_H - PAIRS_V + QUADS at
 * connectivity 4 and AREA - PAIRS_H - PAIRS_V - PAIRS_D + TRIPLES + 3 QUADS at connectivity 8 (1 - euler_k: the holes of the
 * component taken alone); INNER_ROUND = the components with WALL == 0.  They are reduced on the device from the table.
 * The look checks itself: every label the sweep meets has a component number, and the areas of the table add up to the
 * AREA of the components look; a violation is CHS_ECHECK.  Arguments and states are checked as by chs_components, with the
 * same codes in the same order; `rows` must be the COUNT of the last shapes look.  The run does not notice the look. */
#define CHS_SH_COLS 16
#define CHS_SH_FIRST 0
#define CHS_SH_AREA 1
#define CHS_SH_PAIRS_H 2
#define CHS_SH_PAIRS_V 3
#define CHS_SH_PAIRS_D 4
#define CHS_SH_TRIPLES 5
#define CHS_SH_QUADS 6
#define CHS_SH_WALL 7
#define CHS_SH_SI 8
#define CHS_SH_SJ 9
#define CHS_SH_SII 10
#define CHS_SH_SJJ 11
#define CHS_SH_SIJ 12
#define CHS_SH_SU_FIX 13
#define CHS_SH_SUU_FIX 14
#define CHS_SH_N_OUTSIDE 15
#define CHS_SH_WORDS 17
#define CHS_SH_SUM_AREA 7
#define CHS_SH_SUM_PAIRS_H 8
#define CHS_SH_SUM_PAIRS_V 9
#define CHS_SH_SUM_PAIRS_D 10
#define CHS_SH_SUM_TRIPLES 11
#define CHS_SH_SUM_QUADS 12
#define CHS_SH_SUM_WALL 13
#define CHS_SH_SUM_N_OUTSIDE 14
#define CHS_SH_HOLES 15
#define CHS_SH_INNER_ROUND 16
int chs_shapes(chs_handle h, double threshold, int32_t connectivity, int32_t side, int64_t out[CHS_SH_WORDS]);
int chs_shapes_table(chs_handle h, int64_t rows, int64_t* out);   /* [rows][CHS_SH_COLS]; rows == COUNT of the last shapes look */
/* Device time (ms, HIP events) of the sweep and the summary of the handle's last shapes look alone: the labelling before
 * them is timed by chs_components_last_ms. */
int chs_shapes_last_ms(chs_handle h, double* ms);

/* ---- Droplet tracking: the labelling of now overlapped with that of an earlier look ---------
 * A FRAME is the component-number image of a track look: int32 [N][N], -1 for background, the numbering that of
 * chs_components (by ascending `first`), together with its count CA and its (threshold, connectivity, side).  A handle
 * keeps at most one frame, on the device.
 * Pixel p has a = frame[p] and b = its number in the current look; its key is (a, b).  The PAIR TABLE is int64 [P][3]: one
 * row (a, b, n) for every key other than (-1, -1) that at least one pixel has, n being the number of such pixels, the rows
 * sorted by (a, b).  Rows with b = -1 are the pixels droplet a lost to the background, rows with a = -1 the ground
 * droplet b gained from it.  Every cell is an integer and every accumulation an integer add, so the table does not depend
 * on the order the device worked in: it is the numpy model's (chsimpy_amd/tracking.py) bit for bit, for both element types.
 * A track look IS a shapes look (and so a components look) of the same (threshold, connectivity, side): arguments and
 * states are checked by it, the same codes in the same order, and afterwards chs_shapes_table, chs_components_table and
 * chs_components_labels return this labelling.  If the handle holds a frame, the look then overlaps the frame with the
 * current labelling.  With keep != 0 the current number image becomes the frame (two images are swapped, nothing is
 * copied); keep == 0 leaves the frame as it is, which compares many later times against one reference.  The frame's
 * (threshold, connectivity, side) need not be the look's.
 * The frame survives steps, chs_set_U and later chs_components and chs_shapes looks; it goes with chs_track_reset and with
 * the handle.  A rejected call leaves the frame, the last pair table and the last time in place.
 * Words, CHS_TR_WORDS int64: the 17 of chs_shapes; HAVE_PREV (1 where the look found a frame); PREV_COUNT = CA; PAIRS = P;
 * OVERLAP, the pixels with a >= 0 and b >= 0; LOST, a >= 0 and b = -1; GAINED, a = -1 and b >= 0; HEADS, the pixels with a
 * key other than (-1, -1) that differs from the key of the left and of the upper neighbour (a wall counts as different):
 * the raster-first pixel of every key is one, so P <= HEADS, and HEADS sizes the hash table; SLOTS, the slots of that
 * table, the power of two >= 2 HEADS and at least 1024.  Without a frame HAVE_PREV = 0 and the words behind it are 0.
 * A table above 2 GiB (16 bytes a slot: more than 2^26 heads, which only noise at N > 8192 has) is refused with CHS_EHIP,
 * the code of an allocation the device refuses, and a message.
 * The look checks itself: the rows' n and the (-1, -1) pixels add up to N^2, the rows with a >= 0 to the frame's area, the
 * rows with b >= 0 to the AREA of the components look, P <= HEADS, and no insert ran out of slots; a violation is
 * CHS_ECHECK.  The run does not notice the look. */
#define CHS_TR_WORDS 25
#define CHS_TR_HAVE_PREV 17
#define CHS_TR_PREV_COUNT 18
#define CHS_TR_PAIRS 19
#define CHS_TR_OVERLAP 20
#define CHS_TR_LOST 21
#define CHS_TR_GAINED 22
#define CHS_TR_HEADS 23
#define CHS_TR_SLOTS 24
int chs_track(chs_handle h, double threshold, int32_t connectivity, int32_t side, int32_t keep, int64_t out[CHS_TR_WORDS]);
int chs_track_pairs(chs_handle h, int64_t rows, int64_t* out);   /* [rows][3]; rows == PAIRS of the last track look */
int chs_track_reset(chs_handle h);                               /* drop the frame; the buffers stay */
/* Device time (ms, HIP events) of the overlap passes of the handle's last track look alone (the host's wait for HEADS
 * between them left out): the labelling and the shape table before them are timed by chs_components_last_ms and
 * chs_shapes_last_ms. */
int chs_track_last_ms(chs_handle h, double* ms);

const char* chs_last_error(void);
const char* chs_version(void);

/* ---- Batches: B ensemble members advanced together --------------------------------------------------------------
 * A batch holds B members of the same N, dtype and device and runs the engine a single handle of its members would run:
 *   - the fast engine at N in {128, 256, 512, 1024, 2048} (engine = CHS_ENGINE_AUTO or CHS_ENGINE_FAST): its members
 *     either all keep a fixed time step or all adapt it (adaptive_time, solver.py:177-193: each member by its own rule,
 *     counter and delt_max);
 *   - the chirp engine at every other N in [CHS_BATCH_CHIRP_MIN_N, CHS_BATCH_CHIRP_MAX_N] = [8, 4096], where engine =
 *     CHS_ENGINE_CHIRP asks for it or CHS_ENGINE_AUTO resolves to it (N >= CHS_CHIRP_AUTO_MIN_N, not a power of two):
 *     fixed time step only, and no seat queue (chs_batch_step_n_queued returns CHS_EINVAL).
 * Every other scalar of chs_consts -- A0, A1, full_sim, time_limit_s, delt, delt_max, threshold, ... -- is the member's
 * own.  Each step kernel is launched once for all members, so that the short dependent chains of small grids overlap
 * each other on the device (the chirp engine's step: 13 launches for the whole batch).  For every member m the semantics
 * are those of chs_prepare / chs_step_n / chs_get_state on a single handle created from consts[m] with the batch's
 * engine; every chs_batch_step_n is a literal solve_or_resume call (hat_U = dctn(U) recomputed on entry, solver.py:159;
 * U stored at the end), and a member of a chirp batch is bit for bit its single chirp handle stepped with
 * CHS_STEP_REDERIVE_HAT.  One lambda table for all members.
 * chs_batch_create returns CHS_EINVAL (chs_last_error says why) for B < 1, members that differ in N, dtype or device,
 * an N that neither engine's batch takes (engine = CHS_ENGINE_CHIRP at one of the fast batch's five sizes included:
 * those are batches of the fast engine only), engine = CHS_ENGINE_DIRECT, a member of a fast batch whose adaptive_time
 * differs from member 0's, or a member of a chirp batch with adaptive_time set (the message names the first such
 * member).  Jitter has no batched counterpart.  `member` = -1 addresses every member where noted. */
#define CHS_BATCH_CHIRP_MIN_N 8
#define CHS_BATCH_CHIRP_MAX_N 4096
#define CHS_BATCH_MAX_MEMBERS 65535 /* B of chs_batch_create: the member is a grid dimension of every batched launch */
typedef struct chs_batch_s* chs_batch;
int chs_batch_create(const chs_consts* consts /*[B]*/, int32_t B, const double* lambda, chs_batch* out);
int chs_batch_destroy(chs_batch b);
/* The engine the batch's members run (what chs_engine reports for each of them): CHS_ENGINE_FAST or CHS_ENGINE_CHIRP. */
int chs_batch_engine(chs_batch b);
int chs_batch_set_U(chs_batch b, int32_t member, const double* host_U);           /* member -1: all */
int chs_batch_init_U_pcg64(chs_batch b, int32_t member, double base, double scale,
                           const uint64_t state[2], const uint64_t inc[2]);        /* member -1: all */
int chs_batch_get_U(chs_batch b, int32_t member, double* host_U);
/* chs_prepare of every member; rows0[m] = member m's step-0 record.  CHS_ENAN when one of them is NaN (the others
 * are prepared all the same). */
int chs_batch_prepare(chs_batch b, double* rows0 /*[B][9]*/);
/* nsteps[m] iterations of member m (0: the member sits the call out, its state and field unchanged); `flags` is
 * reserved and must be 0.  rows[m] (stride: the largest nsteps) receives member m's timedata rows, steps_done[m] how
 * many, status[m] CHS_OK or CHS_ENAN.  A member that stops (energy rule, time limit, NaN) is frozen while the others
 * go on; the call ends when every member has halted or done its steps.  Returns CHS_ENAN when any member hit NaN (the
 * rows of the others stay valid).  chs_batch_get_U(m) afterwards returns the field of m's last completed step. */
int chs_batch_step_n(chs_batch b, const int64_t* nsteps /*[B]*/, int32_t flags,
                     double* rows /*[B][max nsteps][9]*/, int64_t* steps_done /*[B]*/, int32_t* status /*[B]*/);
int chs_batch_get_state(chs_batch b, int32_t member, chs_state* out);
int chs_batch_set_state(chs_batch b, int32_t member, const chs_state* in);
/* The seat queue: chs_batch_step_n with the members taking turns on the device.  Every step kernel is launched over
 * `seats` seats; when the member in a seat stops (energy rule, time limit, NaN) or has done its nsteps, the next
 * member that waits takes the seat on the device, without a host round trip -- members take seats in member order, a
 * seat changes hands in front of an even step of the call (so that every member walks its column tiles in the order it
 * would in chs_batch_step_n).  Member by member the call means what chs_batch_step_n means, and its results are bit
 * for bit those of chs_batch_step_n: a literal solve_or_resume call, the same stop rules, NaN handling and rebuild of U
 * after a stop; nsteps[m] = 0 sits the call out.  A batch of R members is a queue of R members: seats >= R behaves
 * like chs_batch_step_n; seats < 1, flags != 0 and a chirp batch (it has no queue) return CHS_EINVAL.  The rows are kept by the batch as the polls of
 * the call copy them out of the members' rings (no [R][max nsteps][9] array: 72 MB per member at ntmax = 1e6) until
 * the next queued call; chs_batch_member_rows hands over the first n <= steps_done[member] of them. */
int chs_batch_step_n_queued(chs_batch b, int32_t seats, const int64_t* nsteps /*[R]*/, int32_t flags,
                            int64_t* steps_done /*[R]*/, int32_t* status /*[R]*/);
int chs_batch_member_rows(chs_batch b, int32_t member, double* rows /*[n][9]*/, int64_t n);
/* chs_structure_factor of member `member` (ssum[nbins]), or of every member for member = -1 (ssum[B][nbins]): the
 * sweep and the binning are then launched once with the member as a grid dimension, the transform once per member
 * (a chirp batch: once for all, four launches).  Member by member the result is bit for bit that of the member's single
 * handle on the same field, and of the call with its own number.  The members' states, fields and records stay
 * untouched: their next call is bit for bit what it is without the look. */
int chs_batch_structure_factor(chs_batch b, int32_t member, double* ssum /*[nbins] or [B][nbins]*/, int32_t nbins);
/* chs_morphology of member `member` (threshold[1], out[CHS_MORPH_WORDS]), or of every member for member = -1
 * (threshold[B], out[B][CHS_MORPH_WORDS]: one launch pair over all members, each with its own threshold).  Member by
 * member the words are those of the member's single handle on the same field.  The members' states, fields and records
 * stay untouched.  CHS_EINVAL for a member outside [-1, B). */
int chs_batch_morphology(chs_batch b, int32_t member, const double* threshold, int64_t* out);
/* chs_components of member `member` (in [0, B), else CHS_EINVAL) on the batch's stream; one set of buffers for the batch,
 * so table and labels are those of the batch's last look, whichever member it was.  The words, the table and the labels
 * are those of the member's single handle on the same field.  The members' states, fields and records stay untouched. */
int chs_batch_components(chs_batch b, int32_t member, double threshold, int32_t connectivity, int32_t side, int64_t out[CHS_CC_WORDS]);
int chs_batch_components_table(chs_batch b, int64_t rows, int32_t* out);
int chs_batch_components_labels(chs_batch b, int32_t* out);
/* chs_distance of member `member` (in [0, B), else CHS_EINVAL) on the batch's stream; one set of buffers for the batch,
 * so histogram and map are those of the batch's last look, whichever member it was.  Words, histogram and map are those
 * of the member's single handle on the same field.  The members' states, fields and records stay untouched. */
int chs_batch_distance(chs_batch b, int32_t member, double threshold, int32_t side, int64_t out[CHS_DT_WORDS]);
int chs_batch_distance_hist(chs_batch b, int32_t nbins, int64_t* out);
int chs_batch_distance_map(chs_batch b, int32_t* out);
/* chs_chords of member `member` (in [0, B), else CHS_EINVAL) on the batch's stream; one set of buffers for the batch,
 * so the histogram is that of the batch's last look, whichever member it was.  Words and histogram are those of the
 * member's single handle on the same field.  The members' states, fields and records stay untouched. */
int chs_batch_chords(chs_batch b, int32_t member, double threshold, int64_t out[CHS_CH_WORDS]);
int chs_batch_chords_hist(chs_batch b, int32_t nbins, int64_t* out);
/* chs_composition and chs_composition_select of member `member` (in [0, B), else CHS_EINVAL) on the batch's stream; one
 * set of buffers for the batch, so the histogram and the time are those of the batch's last look, whichever member it
 * was.  Words, histogram and values are those of the member's single handle on the same field.  The members' states,
 * fields and records stay untouched.  (The geometry has no handle: chs_composition_tile.) */
int chs_batch_composition(chs_batch b, int32_t member, double threshold, int32_t nbins, double lo, double hi,
                          int64_t iw[CHS_CMP_IWORDS], double fw[CHS_CMP_FWORDS]);
int chs_batch_composition_hist(chs_batch b, int32_t nbins, int64_t* out);
int chs_batch_composition_select(chs_batch b, int32_t member, int32_t nq, const int64_t* ranks, double* values);
int chs_batch_composition_last_ms(chs_batch b, double* ms);
/* chs_two_point of member `member` (in [0, B), else CHS_EINVAL) on the batch's stream; one set of buffers for the batch,
 * so the count table and the time are those of the batch's last look, whichever member it was.  Words and counts are those
 * of the member's single handle on the same field.  The members' states, fields and records stay untouched. */
int chs_batch_two_point(chs_batch b, int32_t member, double threshold, int32_t rmax, int64_t out[CHS_TP_WORDS]);
int chs_batch_two_point_counts(chs_batch b, int64_t n, int64_t* out);
int chs_batch_two_point_last_ms(chs_batch b, double* ms);
/* chs_contour of member `member` (in [0, B), else CHS_EINVAL) on the batch's stream; one set of buffers for the batch,
 * so the histogram, the map and the time are those of the batch's last look, whichever member it was.  Words, sums,
 * histogram and map are those of the member's single handle on the same field, bit for bit.  The members' states, fields
 * and records stay untouched. */
int chs_batch_contour(chs_batch b, int32_t member, double threshold, int32_t bins, double kmax, int32_t want_map,
                      int64_t words[CHS_CT_WORDS], double sums[CHS_CT_SUMS]);
int chs_batch_contour_hist(chs_batch b, int32_t bins, int64_t* out);
int chs_batch_contour_map(chs_batch b, int64_t n, double* out);
int chs_batch_contour_last_ms(chs_batch b, double* ms);
/* chs_shapes of member `member` (in [0, B), else CHS_EINVAL) on the batch's stream; one set of component buffers and one
 * set of shape buffers for the batch, so the tables are those of the batch's last look, whichever member it was.  Words
 * and table are those of the member's single handle on the same field.  The members' states, fields and records stay
 * untouched. */
int chs_batch_shapes(chs_batch b, int32_t member, double threshold, int32_t connectivity, int32_t side, int64_t out[CHS_SH_WORDS]);
int chs_batch_shapes_table(chs_batch b, int64_t rows, int64_t* out);
/* chs_track of member `member` (in [0, B), else CHS_EINVAL) on the batch's stream.  The frame is per member, allocated
 * at that member's first track look, and chs_batch_track_reset drops that member's; the component and shape buffers, the
 * hash table and the row list are the batch's one set, so the tables and the pair table are those of the batch's last
 * look, whichever member it was.  Words and pairs are those of the member's single handle on the same fields.  The
 * members' states, fields and records stay untouched. */
int chs_batch_track(chs_batch b, int32_t member, double threshold, int32_t connectivity, int32_t side, int32_t keep,
                    int64_t out[CHS_TR_WORDS]);
int chs_batch_track_pairs(chs_batch b, int64_t rows, int64_t* out);
int chs_batch_track_reset(chs_batch b, int32_t member);
/* chs_thickness of member `member` (in [0, B), else CHS_EINVAL) on the batch's stream; one set of distance buffers and
 * one set of thickness buffers for the batch, so histogram, map and time are those of the batch's last look, whichever
 * member it was (and chs_batch_distance_hist / _map those of the distance look inside).  Words, histogram and map are
 * those of the member's single handle on the same field.  The members' states, fields and records stay untouched. */
int chs_batch_thickness(chs_batch b, int32_t member, double threshold, int32_t side, int64_t max_work, int64_t out[CHS_TH_WORDS]);
int chs_batch_thickness_hist(chs_batch b, int32_t nbins, int64_t* out);
int chs_batch_thickness_map(chs_batch b, int32_t* out);
int chs_batch_thickness_last_ms(chs_batch b, double* ms);
/* chs_geodesic of member `member` (in [0, B), else CHS_EINVAL) on the batch's stream; one set of component buffers and
 * one set of geodesic buffers for the batch, so histogram, profile, map and time are those of the batch's last look,
 * whichever member it was (and chs_batch_components_table / _labels those of the components look inside).  Words,
 * histogram, profile and map are those of the member's single handle on the same field.  The members' states, fields and
 * records stay untouched. */
int chs_batch_geodesic(chs_batch b, int32_t member, double threshold, int32_t connectivity, int32_t side, int32_t source,
                       int64_t max_rounds, int64_t out[CHS_GEO_WORDS]);
int chs_batch_geodesic_hist(chs_batch b, int32_t nbins, int64_t* out);
int chs_batch_geodesic_profile(chs_batch b, int64_t* out);
int chs_batch_geodesic_map(chs_batch b, int32_t* out);
int chs_batch_geodesic_last_ms(chs_batch b, double* ms);
/* chs_skeleton of member `member` (in [0, B), else CHS_EINVAL) on the batch's stream; one set of distance buffers and one
 * set of skeleton buffers for the batch, so histogram, plane and times are those of the batch's last look, whichever
 * member it was (and chs_batch_distance_hist / _map those of the distance look inside).  Words, histogram and plane are
 * those of the member's single handle on the same field.  The members' states, fields and records stay untouched. */
int chs_batch_skeleton(chs_batch b, int32_t member, double threshold, int32_t side, int64_t max_subiters, int64_t out[CHS_SK_WORDS]);
int chs_batch_skeleton_hist(chs_batch b, int32_t nbins, int64_t* out);
int chs_batch_skeleton_plane(chs_batch b, uint64_t* out);
int chs_batch_skeleton_last_ms(chs_batch b, double* ms);
int chs_batch_skeleton_thin_ms(chs_batch b, double* ms);
/* chs_transport of member `member` (in [0, B), else CHS_EINVAL) on the batch's stream; one set of component buffers and
 * one set of transport buffers for the batch, so profile, map and times are those of the batch's last look, whichever
 * member it was (and chs_batch_components_table / _labels those of the components look inside).  Words, values, profile
 * and map are those of the member's single handle on the same field.  The members' states, fields and records stay
 * untouched. */
int chs_batch_transport(chs_batch b, int32_t member, double threshold, int32_t side, int32_t source, double tol, int64_t max_iters,
                        int64_t words[CHS_TRN_WORDS], double vals[CHS_TRN_VALS]);
int chs_batch_transport_profile(chs_batch b, double* out);
int chs_batch_transport_map(chs_batch b, double* out);
int chs_batch_transport_last_ms(chs_batch b, double* ms);
int chs_batch_transport_solve_ms(chs_batch b, double* ms);

#ifdef __cplusplus
}
#endif
#endif /* CHS_HIP_H */
