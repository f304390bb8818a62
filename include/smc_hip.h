/*
 * include/smc_hip.h -- C ABI of libsmc_hip.so, the MI355X (gfx950) engine for the particle
 * inner loop of adaptive likelihood-tempered SMC.
 *
 * The reference (maruchitatsuki/python-based-Sequential-Monte-Carlo-method-with-likelihood-tempering)
 * has no FFI: its boundary is a set of Python names.  Each entry point
 * below names the reference statements it replaces (file:line relative to the reference root).
 * The Python host side (python-based-..._amd/binding.py) binds exactly these symbols with ctypes;
 * INTEGRATION.md shows the stub a reference maintainer would add.
 *
 * Conventions
 *   - plain C types only; every function returns 0 on success, non-zero on error, and
 *     smc_last_error(ctx) returns the message (ctx may be NULL for creation errors);
 *   - the caller owns host buffers (C-contiguous float64 / int64 / uint8); the library owns all
 *     device memory inside the opaque context; one context per (process, device); a context is
 *     not thread-safe;
 *   - particles are AoS (N,d) at this edge, exactly like the reference's p_pred / p_filt arrays,
 *     and SoA d x N in HBM (transposed by the upload / download calls);
 *   - the two particle sets of the reference are addressed by SMC_SET_PRED (p_pred with lk,
 *     Micmem_settings.py:85; Micmem_SMC_main.py:98) and SMC_SET_FILT (p_filt with lk1,
 *     Micmem_settings.py:118,127);
 *   - every arithmetic step is IEEE float64; integers are used only for offspring counts and flags;
 *   - multi-GPU: one context per rank, each owning the contiguous block
 *     [rank*n_local, (rank+1)*n_local) of the global particle order.  Entry points that take
 *     "_local"/"_global" arguments compute this rank's partial; the host combines partials with the
 *     smc_comm_* collectives (RCCL).  With one rank the same calls are used with world size 1.
 */
#ifndef SMC_HIP_H
#define SMC_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SMC_ABI_VERSION 3    /* 2: smc_meth_sweep_check writes FIVE words (round 3 added the cancelled count); smc_mh_sweeps_device_rng
                              * 3: smc_work_totals; smc_mh_sweeps_device_rng takes the methanation model too and returns the sweep counters;
                              *    smc_meth_dae_host's stats have five words (round 5)
                              * (still 3: smc_set_share_replicates / smc_mm_share_info and smc_set_start_reject / smc_mm_start_reject_info /
                              *    smc_mm_reject_threshold only ADD entry points; the binding tolerates their absence in an older A/B build;
                              *    likewise the user-model functions ...4 to ...7: noise models, inputs, events and, with
                              *    smc_set_model_user7 / smc_user_censor_check / check7 / dump_source7, censored observations) */
#define SMC_MAX_DIM 8        /* parameters per particle (3 for Michaelis-Menten, 5 for methanation) */
#define SMC_MAX_ESS_CAND 16  /* tempering candidates evaluated by one smc_ess_partials call */
#define SMC_MAX_RANKS 64

#define SMC_SET_PRED 0
#define SMC_SET_FILT 1

#define SMC_PRIOR_UNIFORM 0 /* {"dist":"uniform","low","high"}  Micmem_settings.py:63-67 */
#define SMC_PRIOR_NORMAL 1  /* {"dist":"normal","mu","sigma"}   Micmem_settings.py:55-59 */
#define SMC_PRIOR_FLAT 2    /* no factor in cal_prior (sigma under normal_pred without taylor,
                             * methanation_functions.py:132-138 multiplies num_est_params-1 densities) */
/* the families of smc_set_prior_ex (documented there); smc_set_prior refuses them */
#define SMC_PRIOR_LOGNORMAL 3   /* {"dist":"lognormal","mu","sigma"}                 of log x */
#define SMC_PRIOR_GAMMA 4       /* {"dist":"gamma","shape","scale"} */
#define SMC_PRIOR_BETA 5        /* {"dist":"beta","a","b","low","high"}              on (low, high) */
#define SMC_PRIOR_TRUNCNORMAL 6 /* {"dist":"truncnormal","mu","sigma","low","high"}  "halfnormal": mu 0, low 0, high +inf */

/* what the Metropolis acceptance does with the prior */
#define SMC_PRIOR_MODE_MASK 0        /* pp = exp(px*g) * p0            Micmem_SMC_main.py:224-233, SMC_methanation_main.py:376-389 */
#define SMC_PRIOR_MODE_RATIO_MASK 1  /* pp = exp(px*g) * (p0_2/p0_1) * p0   SMC_methanation_main.py:320-349 (normal_pred, taylor) */
#define SMC_PRIOR_MODE_RATIO 2       /* pp = exp(px*g) * (p0_2/p0_1), no reset of proposals   :358-374 (normal_pred) */

typedef struct smc_ctx smc_ctx;

int smc_abi_version(void);
/* NULL ctx: message of the last failed smc_create / context-less call in this thread. */
const char *smc_last_error(const smc_ctx *ctx);

/* Context with capacity for n_local particles of dimension dim on HIP device `device`.
 * n_global = world * n_local (pass n_local for a single GPU).  Replaces the buffer allocations of
 * Micmem_settings.py:85,118-127. */
int smc_create(smc_ctx **out, int device, int64_t n_local, int64_t n_global, int dim);
void smc_destroy(smc_ctx *ctx);
int smc_synchronize(smc_ctx *ctx);
/* Name/arch of the device the context runs on (e.g. "gfx950"). */
int smc_device_info(smc_ctx *ctx, char *name, int name_len, char *arch, int arch_len, int *cu_count);

/* ---- model + prior ------------------------------------------------------------------------ */
/* Michaelis-Menten data set (Micmem_settings.py:103-115) and solver tolerances (SciPy defaults
 * rtol=1e-3, atol=1e-6 of the solve_ivp call at Micmem_likelihood.py:24-30).  t and P_obs are
 * n_ex x n_t row-major, S0 has n_ex entries.  n_ex <= 16, n_t <= 256. */
int smc_set_model_mm(smc_ctx *ctx, const double *t, const double *P_obs, const double *S0, int n_ex, int n_t,
                     int est_sigma, double sigma_fixed, double rtol, double atol);
/* Methanation model (configs 4-5) for the resident sets: smc_loglik and smc_mh_step_* then evaluate
 * cal_parallel_new (methanation_functions.py:44-65) per particle: the particle's `dim` estimated values are
 * scattered into the 9-vector base_params at est_position (:80), my_model integrates the DAE of each of the
 * n_data experiments (K8, parity unpinned against IDA) and my_loglike compares the outlet flows with obs.
 * cond: n_data x 10 (Ca_in,Cb_in,Cc_in,Cd_in,Ce_in,T_in,T_jacket,u_in,void,dz = the first ten entries of p0,
 * methanation_set_likelihood.py:164); guess: n_data x 357; obs: 5 x n_data; base_params: 9. */
int smc_set_model_methanation(smc_ctx *ctx, const double *cond, const double *guess, const double *obs, int n_data,
                              const double *base_params, const int *est_position, int est_sigma, double sigma_fixed,
                              double tf, double rtol, double atol);
/* User model (the reference's README.md:4 "modify for your problem", i.e. a new
 * Micmem_likelihood.py): `source` is HIP device code defining, for the state y[n_states] of an ODE,
 *   __device__ void   smc_user_y0 (const double *theta, const double *cond, double *y);            initial state at t[e][0]
 *   __device__ void   smc_user_rhs(double t, const double *y, const double *theta, const double *cond, double *dydt);
 *   __device__ double smc_user_obs(double t, const double *y, const double *theta, const double *cond);   what obs is compared with
 * (theta: the particle's `dim` values; cond: the n_cond numbers of experiment e).  It is compiled at run time (hiprtc,
 * gfx950) into a kernel that restates solve_ivp(RK45, t_eval = t[e], rtol, atol) and the Gaussian log-likelihood of
 * Micmem_likelihood.py:17-33,62-73 with sigma = the last parameter (est_sigma) or sigma_fixed; smc_loglik and
 * smc_mh_step_* then use it.  t, obs: n_ex x n_t; cond: n_ex x n_cond.  A source that does not compile fails with
 * hiprtc's log in smc_last_error.  A model is DESCRIBED BY ONE STRUCT, smc_user_model_spec below, and set by
 * smc_set_model_user_spec; what decides the text of the compiled kernel is the smaller smc_user_source_spec, which
 * smc_user_model_check_spec only compiles (no GPU needed): 0 ok, 1 compile error (log), 2 bad arguments.  Every feature is
 * documented once, at its fields; a feature whose fields are zero / NULL is absent, and the model then takes the path, and
 * gives the bits, it had before the feature existed.
 * Optional fourth ingredient, a COST HINT (a source that contains the name must define it):
 *   __device__ double smc_user_cost(const double *theta);      rough number of RK45 step attempts of one solve with theta
 * Sweeps then hand the solves of particles above 220 attempts out before the index-ordered ones and run those above 3700
 * one per wave on wave-uniform operands (the built-in Michaelis-Menten kernel's stiff list and solo phase, smc_set_stiff_first
 * switches both off) - a sweep over a prior population is bounded by its longest serial solve, which should start first -
 * and heterogeneous Metropolis sweeps of 16 384 particles or more are handed out by cost class and in phase (smc_set_cost_order).
 * The hint changes the order of independent solves only, never a result; it may be crude, and NaN counts as cheap.
 * The functions may call   double smc_div(double a, double b)   for a / b: the source is compiled twice, in two namespaces
 * (so: device functions and constants only, nothing extern "C") - once with the six-operation division of the built-in
 * kernel (v_rcp, one Newton step, one correction: equal to a / b for normal operands and quotients up to a last bit in about one pair of 2^44, NaN where a / b
 * needs a subnormal or infinite divisor or a * (1 / b) overflows), once with IEEE division; a step attempt runs on the first
 * and is repeated on the second whenever its error norm is not finite.  smc_user_y0, smc_user_obs and smc_user_cost always
 * run with IEEE division.
 * Integrator (the field `method` of both structs; an unknown method fails or returns 2):
 *   SMC_USER_METHOD_RK45  explicit RK45, as above (the default);
 *   SMC_USER_METHOD_BDF   solve_ivp(method="BDF") as SciPy 1.15's bdf.py has it (variable-order NDF 1-5, Newton with at most four
 *                         iterations, LU of I - c J with partial pivoting, BdfDenseOutput at t) - for a STIFF model, where
 *                         RK45 runs on its stability limit.  The source is compiled once, with smc_div(a, b) = a / b, and may
 *                         define a fifth ingredient (a source that contains the name must define it):
 *   __device__ void smc_user_jac(double t, const double *y, const double *theta, const double *cond, double *J);
 *                         J[i * n_states + j] = d dydt[i] / d y[j]; without it J is formed by forward differences as
 *                         SciPy's num_jac does.  One attempt of the sweep counters (rk_attempts) is one BDF step attempt;
 *                         smc_user_sweep_counters reports the rest of the work. */
#define SMC_USER_MAX_STATES 8
#define SMC_USER_METHOD_RK45 0
#define SMC_USER_METHOD_BDF 1
#define SMC_USER_MAX_OBS 8
#define SMC_USER_MAX_INPUTS 8
#define SMC_USER_MAX_KNOTS 4096
#define SMC_USER_MAX_EVENTS 256
#define SMC_USER_MAX_EVENT_VALUES 8
#define SMC_USER_MAX_ROOTS 4        /* event functions of a source with state-triggered events (smc_user_root) */
#define SMC_USER_MAX_ROOT_FIRES 256 /* ... and how often they may fire in one solve */
/* BOTH STRUCTS START WITH struct_size, the caller's sizeof: the library reads min(struct_size, its own sizeof) bytes over zeros, so
 * a field that a later feature appends reads as absent for a caller built before it.  A struct_size that ends before the fields
 * every caller has (smc_user_source_spec: through n_obs; smc_user_model_spec: through atol) or exceeds the library's own struct
 * is refused: the functions return 2, or fail with a message that names struct_size.  Zero the struct, set struct_size, then
 * the fields in use. */
/* What decides the text of the run-time compiled kernel; each field is explained at the field of the same name below. */
typedef struct smc_user_source_spec {
    size_t struct_size;
    const char *source;
    int n_states;   /* 1 .. SMC_USER_MAX_STATES */
    int dim;        /* parameters per particle, 1 .. SMC_MAX_DIM */
    int method;     /* SMC_USER_METHOD_* */
    int n_obs;      /* 0: the one-output source; 1 .. SMC_USER_MAX_OBS: the multi-output source */
    int noise;      /* 0: the sigma rule, 1: a noise model, 2: one with a proportional part */
    int n_cond;     /* with inputs or events: the numbers in front of the tables of a cond row */
    int n_in, n_knot;
    int n_ev, n_val;
    int censor;     /* != 0: censored observations; needs noise = 1 or 2 */
} smc_user_source_spec;
/* A user model: its source, data, likelihood and tolerances. */
typedef struct smc_user_model_spec {
    size_t struct_size;
    const char *source;
    int n_states;
    int method;
    /* SEVERAL OBSERVED OUTPUTS, MISSING DATA, RAGGED ROWS: n_obs = 1 .. SMC_USER_MAX_OBS outputs per data time (n_obs = 0: the
     * ONE-OUTPUT MODEL, obs n_ex x n_t compared with smc_user_obs, a NaN given to it makes logL NaN, and obs_scale, the noise
     * arrays, inputs, events and censor must all be absent); the source defines
     *   __device__ void smc_user_obs_vec(double t, const double *y, const double *theta, const double *cond, double *out);   out[0 .. n_obs)
     * (with n_obs = 1 a source may define smc_user_obs instead; a source that contains the name smc_user_obs_vec must define it).
     * t: n_ex x n_t, obs: n_ex x n_t x n_obs, row-major.  NaN in obs = not measured: the entry adds nothing to the squared residuals
     * nor to m_e, the number of finite entries of experiment e.  A row of t may end in a run of NaN times: that experiment has
     * n_t_e times, is integrated to t[e][n_t_e - 1], and obs at its NaN times is ignored.  The finite times of a row strictly
     * increase and every row has one; obs holds no infinite value; obs_scale (n_obs relative scales s_k, NULL = ones) is finite
     * and > 0 - otherwise the set function fails with the reason.  With sigma as before (the last parameter or sigma_fixed):
     *   logL = sum_e [ -m_e / 2 log(2 pi sigma^2) - sum_(observed i,k of e) log s_k - sum_(observed) ((obs - model) / s_k)^2 / (2 sigma^2) ]
     * (sigma <= 0: -inf; an experiment with m_e = 0 adds 0).  Exact early rejection applies as before.  In a source spec n_obs >= 1
     * selects the multi-output source (a dump also writes user_obs_args.h); n_obs outside 0 .. SMC_USER_MAX_OBS returns 2. */
    int n_obs;
    const double *t, *obs, *cond, *obs_scale;
    int n_ex, n_t, n_cond;
    int est_sigma;          /* the sigma rule: != 0 sigma is the last parameter, else sigma_fixed */
    double sigma_fixed;
    /* A NOISE MODEL: a noise level per output, and noise that grows with the signal.  add_index == NULL (then add_fixed,
     * prop_index, prop_fixed NULL too) is the SIGMA RULE above (est_sigma / sigma_fixed); otherwise est_sigma and sigma_fixed are
     * not used.  Data, source and obs_scale as above.  Output k has an additive level a_k and a proportional
     * coefficient b_k, each one of the particle's parameters or a fixed number: add_index[k] is a parameter number in [0, dim), or
     * -1 for add_fixed[k], which must then be finite and > 0; prop_index / prop_fixed in the same way with prop_fixed[k] >= 0; NULL
     * for both means no proportional part.  Several outputs may name one parameter.  With f_ik the model's output and s_k = obs_scale:
     *   sd_ik^2 = (a_k s_k)^2 + (b_k f_ik)^2
     *   logL    = sum over observed (e,i,k) [ -1/2 log(2 pi) - log sd_ik - (obs_ik - f_ik)^2 / (2 sd_ik^2) ]
     * (any a_k <= 0 or b_k < 0: -inf; an experiment without an observation adds 0; NaN and ragged rows as above).
     * Exact early rejection applies: the kernels accumulate the excess of every term over its floor log(a_k s_k).
     * smc_user_predict, smc_user_predict_at and smc_user_predict_summary work as for every user model; the summary's noise != 0
     * draws pred + sd_ik z with the particle's own a_k, b_k and prediction.  A specification that is the sigma rule's model - no
     * proportional part and every add_index dim - 1, or every output fixed to one value - takes the sigma rule's path and gives
     * its bits.  Everything else that breaks a rule, and a data set whose image (40 + 8 n_ex words larger than the sigma rule's)
     * exceeds the LDS table, fails with the reason (for the table: bytes needed and available).
     * Limits: model constants and noise parameters together number at most SMC_MAX_DIM; a purely proportional model (a_k = 0) does
     * not exist - the floor needs a_k > 0 - and a small fixed a_k stands in for it.
     * smc_user_noise_check applies the rules of the specification alone (no GPU, no context: the reason is in smc_last_error(NULL)).
     * In a source spec noise = 0 is the sigma rule's source, 1 a noise model's, 2 one with the proportional part compiled in (one
     * log1p and one division per observed value; without it neither is compiled). */
    const int *add_index;
    const double *add_fixed;
    const int *prop_index;
    const double *prop_fixed;
    double rtol, atol;      /* SciPy's defaults are 1e-3, 1e-6 */
    /* TIME-VARYING MEASURED INPUTS: a feed rate, a temperature ramp, a logged
     * inlet concentration - n_in = 1 .. SMC_USER_MAX_INPUTS profiles u_k(t) per experiment, linear between their knots, which the
     * model reads from any of its functions (smc_user_y0, smc_user_rhs, smc_user_jac, smc_user_obs, smc_user_obs_vec) as
     *   double smc_input(const double *cond, int k, double t);      input k in [0, n_in) of this experiment at time t
     * `cond` is the pointer the function was handed - the handle to the experiment; cond[0 .. n_cond) read as before.  The value is
     * np.interp(t, tk, u_k) over the row's finite knots tk[0] < ... < tk[m-1]: u[0] for t <= tk[0], u[m-1] for t >= tk[m-1], else
     * with j the last knot <= t
     *   u[j] + s_j (t - tk[j]),   s_j = (u[j+1] - u[j]) / (tk[j+1] - tk[j])   (the slope is formed once, on the host, by IEEE division);
     * m = 1 is a constant.  It EQUALS u[j] at t == tk[j] and NEVER LEAVES [min(u[j], u[j+1]), max(u[j], u[j+1])] (clamped), and it
     * is the same number in both namespaces of an RK45 source.  user_models.input_value is the definition in NumPy.  The
     * integrators do NOT stop at knots: as solve_ivp with np.interp inside f, they step over the kinks under their own step
     * control (a switch is a steep ramp between two close knots).  What does stop the integrator, and changes the state by a jump,
     * is a scheduled event: ev_t below.
     * Data: in_t n_ex x n_knot, a row by the row rules of t (a strictly increasing finite run of at least one knot, then only NaN);
     * in_u n_ex x n_knot x n_in, finite at the row's finite knots (and every slope finite) and ignored past them; n_knot <=
     * SMC_USER_MAX_KNOTS.  Anything else fails with the row, the knot and the rule.  smc_user_input_check applies these rules alone
     * (no GPU, no context: the reason is in smc_last_error(NULL)).
     * n_in == 0 needs in_t == in_u == NULL: a model without inputs, its path and its bits.  The table lies behind each
     * experiment's cond numbers in device memory (n_cond + K + n_in (2 K + 1) doubles per experiment, K = the power of two >=
     * n_knot: the compiled knot capacity); the LDS table and its limits are those of a model without inputs.  A source that calls smc_input is compiled only for a model with inputs: without them the
     * compilation stops with "smc_input: this model has no inputs".  smc_loglik, smc_mh_step_*, early rejection, the cost hint,
     * smc_user_predict and the BDF counters work as for every user model.
     * A source spec holds the geometry the source is compiled for: n_cond, n_in and n_knot (n_in = 0: a model without inputs;
     * n_knot is then not used).  A dump then also writes user_input.h.
     * DESIGNS: t_new == NULL (the data's design) uses the data's inputs.  An explicit design of smc_user_predict_at /
     * smc_user_predict_summary needs design inputs with the same n_ex_new, set beforehand by smc_user_set_design_inputs (in_t_new
     * n_ex_new x n_knot_new, in_u_new n_ex_new x n_knot_new x n_in, the rules above; no row may hold more finite knots than K) and
     * held until replaced; both pointers NULL clears them.  Without matching design inputs the call fails with the reason.  A design
     * that runs in groups of experiments carries each group's rows of the table. */
    const double *in_t, *in_u;
    int n_in, n_knot;
    /* SCHEDULED EVENTS (doses, feed additions, washouts, resets): at known times the state changes by a jump and the integrator
     * stops there.  Each experiment e has a row of event times ev_t[e][0 .. n_ev) and per event n_val numbers
     * ev_v[e][j][0 .. n_val) (a dose amount, a target compartment, ...).  The source of a model with events defines one more
     * ingredient (a source that contains the name must define it) and may call smc_event_value from it:
     *     __device__ void smc_user_event(int j, double t, double *y, const double *theta, const double *cond);   // y changed in place
     *     double smc_event_value(const double *cond, int j, int k);     // value k of event j of this experiment
     * cond is the handle to the experiment, as for smc_input, which smc_user_event may read too; smc_user_event always runs with
     * IEEE division, like smc_user_y0.
     * A solve of experiment e is the chain of solve_ivp calls a SciPy user would write.  With t0 = t[e][0] and t_end the row's last
     * finite time the events that fire are those with t0 < tau_j < t_end, in order; segment s is solve_ivp(f, (a, b), y, method,
     * t_eval = the row's data times in (a, b] (the first: [t0, b]), rtol, atol) with b the next firing event time or t_end; at an
     * event smc_user_event(j, tau_j, y, ...) is applied to the segment's end state and the next segment starts afresh from
     * (tau_j, y): RK45 with a new first derivative, select_initial_step over the new interval and no memory of a rejected step, BDF
     * at order 1 with a new Jacobian and the initial step rule.  A data time equal to tau_j sees the state before the event, the
     * next representable time after it the state after.  An event with tau_j >= t_end never fires; a segment may hold no data
     * time; rk_attempts counts step attempts only; a failed segment fails the solve as before (info bit 30, NaN from the stop on).
     * The TIMES of these events are data: they cannot depend on theta (amounts can, through smc_user_event).  An event whose time
     * follows from the state - and so from theta - is a state-triggered event, below.
     * Row rules: a row of ev_t is a strictly increasing finite run and then only NaN - it may have no event at all; every finite
     * event time is > t[e][0]; the values are finite at a row's finite events and ignored past them.  Anything else fails with the
     * row, the event and the rule.  smc_user_event_check applies these rules alone (no GPU, no context; the reason in
     * smc_last_error(NULL)).
     * ev_t (n_ex x n_ev), ev_v (n_ex x n_ev x n_val; NULL with n_val == 0), n_ev <= SMC_USER_MAX_EVENTS, 0 <= n_val <=
     * SMC_USER_MAX_EVENT_VALUES.  n_ev == 0 needs both pointers NULL: a model without events, its path and its bits.  A source spec
     * holds the geometry n_ev, n_val the source is compiled for (and n_cond; a dump then also writes user_event.h); a source that defines or calls the event names compiles only for a model
     * with events ("smc_user_event: this model has no events"), and a model with events needs a source with smc_user_event.
     * smc_user_set_design_events: the events of an explicit design of smc_user_predict_at / smc_user_predict_summary (the what-if
     * dosing regimen; nothing is compiled again): n_ex_new rows of n_ev_new <= the model's n_ev events, held until replaced, both
     * pointers NULL clears them.  An explicit design on a model with events without design events of the same n_ex_new fails with
     * the reason; t_new == NULL uses the data's events.
     * STATE-TRIGGERED EVENTS (a feed that switches on when the substrate runs out, a re-dose when a level falls to a threshold, a
     * relay, a tank that overflows): the switching time is where a function of the state crosses zero, which solve_ivp users write
     * as events=.  They need no field: the contract lives in the source, like smc_user_jac and smc_user_cost.  A source that
     * contains the name smc_user_root has state-triggered events and defines all three of
     *     __device__ const int smc_user_root_dir[] = {-1, 0};   // one entry per event function: -1 falling, +1 rising, 0 either
     *     __device__ void smc_user_root(double t, const double *y, const double *theta, const double *cond, double *g);   // g[0 .. n_root)
     *     __device__ void smc_user_root_event(int k, double t, double *y, const double *theta, const double *cond);      // y changed in place
     * n_root, the length of smc_user_root_dir, is 1 .. SMC_USER_MAX_ROOTS.  Both functions always run with IEEE division (in an
     * RK45 source: the smc_user_ieee compilation) and may call smc_input and smc_event_value where the model has those features.
     * A source with smc_user_root and without smc_user_root_dir or smc_user_root_event, more than SMC_USER_MAX_ROOTS entries, or a
     * direction that is not written as one of the integers -1, 0, +1 does not compile, with a message that says so.  The structs,
     * SMC_ABI_VERSION and smc_user_spec_layout are what they were; explicit designs need nothing new, the functions travel with
     * the compiled kernel; a dump of such a source also writes user_root.h.
     * A solve is the chain of solve_ivp calls with every event function terminal, in the arithmetic of SciPy 1.15 (ivp.py,
     * base.py; user_models.root_chain is the chain, user_models.brentq the root solver, both in Python).
     *   Start of a segment - the start of the solve, after a scheduled event, after a triggered one: g = smc_user_root(t, y) there.
     *   Detection: after every accepted step g_new = smc_user_root(t_new, y_new) on the solver's own y_new.  Event k is active when
     * up = g_k <= 0 and g_new_k >= 0 (direction +1 or 0) or down = g_k >= 0 and g_new_k <= 0 (direction -1 or 0) - find_active_events;
     * a NaN is never active.  With no active event g = g_new and nothing else changes.
     *   Locating the root: for each active event brentq(s -> g_k(s, sol(s)), t_old, t_new, xtol = rtol = 4 * 2.220446049250313e-16,
     * maxiter = 100) on that step's dense output sol (RK45: the quartic; BDF: BdfDenseOutput after the step).  The earliest root
     * wins, on a tie the lowest k.
     *   Truncating the step: t* = that root, y* = sol(t*).  The data times <= t* the step covers are served from sol, so a data
     * time equal to t* sees the state before the jump and the next representable time the state after it.
     *   Restart: smc_user_root_event(k, t*, y*), then the next segment starts afresh from (t*, y*) - as after a scheduled event:
     * RK45 with a new first derivative, select_initial_step over the rest of the segment and no memory of a rejected step, BDF at
     * order 1 with a new Jacobian and the initial step rule - and runs to the segment's bound, the next scheduled event time or
     * the row's end.
     *   Failures: a brentq that does not converge, meets a non-finite value, or finds g_k of one sign at both ends of the step
     * (sol(t_new) is not y_new to the last bit; SciPy raises there) fails the solve - info bit 30, NaN from the stop on, as a
     * failed segment does.  So does a root equal to the start of its own segment: the jump left the state on a firing surface
     * (g_k == 0 in a firing direction), and the chain of solve_ivp calls would stop there for ever.  So does fire number
     * SMC_USER_MAX_ROOT_FIRES + 1 of a solve.  A fired event is otherwise free.
     *   Edge cases: a root at the row's end finishes the solve.  At t* equal to a scheduled event's time the triggered jump is
     * applied first, then the scheduled one, and one restart follows.  rk_attempts counts step attempts only: evaluations of the
     * event functions and the right-hand sides of a restart are none; BDF's step counter counts the truncated step, as SciPy does.
     * A source whose event functions never fire gives the bits of the same source without the names. */
    const double *ev_t, *ev_v;
    int n_ev, n_val;
    /* CENSORED OBSERVATIONS: a value the assay could not quantify - below the
     * limit of quantification in a washout tail, above the upper limit at a peak - is neither dropped (NaN) nor taken for a
     * measurement of the limit, but contributes the probability of lying beyond it (Beal's M3).  censor: n_ex x n_t x n_obs flags
     * beside obs, 0: obs is the measured value (the term of the functions above); -1: left-censored, the true value is <= obs, which
     * holds the lower limit; +1: right-censored, the true value is >= obs, the upper limit.  With sd_ik as under A NOISE MODEL:
     *   logL = sum over quantified (e,i,k) [ -1/2 log(2 pi) - log sd_ik - (obs_ik - f_ik)^2 / (2 sd_ik^2) ] + sum over censored log Phi(z_ik),
     *   z_ik = (obs_ik - f_ik) / sd_ik  (left),   (f_ik - obs_ik) / sd_ik  (right);      any a_k <= 0 or b_k < 0: -inf.
     * user_models.censored_loglik is the definition in NumPy.  The kernels add x = -log Phi(z) >= 0 as
     *   z > 0:  -log1p(-erfc(z / sqrt 2) / 2),      z <= 0:  z^2 / 2 - log(erfcx(-z / sqrt 2) / 2)
     * - accurate in both tails, never negative - to the sums of a noise model; a censored value's floor is 0 and m_e, m_ek count
     * quantified values only, so exact early rejection applies unchanged.
     * Rules: every flag is -1, 0 or +1; a nonzero flag stands on a finite value at a finite time of its row.  Anything else fails
     * with the row, the time, the output and the rule.  smc_user_censor_check applies these rules alone to t and obs that
     * the data rules accept (no GPU, no context; the reason in smc_last_error(NULL)); c_n_ex, c_n_t, c_n_obs: the shape of
     * censor itself, which must be that of obs.
     * censor NULL or all zeros: a model without censored observations, its path and its bits.  With a flag set the model is a noise model: add_index == NULL forms the equivalent specification - every
     * output at parameter dim - 1 under est_sigma, else fixed at sigma_fixed, obs_scale as given.  Limits, times and events
     * combine freely; a record of the LDS table holds the flags in its pad word (n_obs even) or grows by 16 bytes (n_obs odd), and a
     * table that no longer fits fails with the bytes needed and available.  smc_user_predict returns lk under this likelihood;
     * designs (smc_user_predict_at, smc_user_predict_summary) carry no observations and run as before.
     * In a source spec censor != 0 is the source compiled with SMC_USER_CENSOR (it needs noise = 1 or 2); a dump then also writes
     * user_censor.h. */
    const signed char *censor;
    /* COUNT OBSERVATIONS (no field: the contract lives in the source, as state-triggered events do): epidemic case counts, colony
     * counts, read counts, detector events.  A multi-output source (n_obs >= 1) that contains the name smc_user_obs_family defines
     *     __device__ const int smc_user_obs_family[] = {0, 2, 1};   // one entry per output
     * 0: a Gaussian output (everything above), 1: Poisson, 2: negative binomial.  The library reads the integer literals behind the
     * first "smc_user_obs_family[" of the text (a comment or a use of the name is passed over) and hands them to the kernel as
     * compile-time constants.  Another length than n_obs, an entry that is none of 0, 1, 2, or the name in a one-output source
     * (n_obs = 0) is refused (check_spec: does not compile) with the rule.  An all-zero list is a model without counts: its earlier
     * path and bits.
     *   For a count output the model output f is the MEAN mu and the variance is mu + (b_k mu)^2, b_k the output's proportional
     * entry (prop_index[k] / prop_fixed[k]): negative binomial b_k > 0, size phi_k = 1 / b_k^2 - b_k is the coefficient of variation
     * of the extra-Poisson scatter -; Poisson: no prop_index, or prop_index[k] = -1 with prop_fixed[k] = 0.  The additive entry of a
     * count output is not used and must be fixed at 1, its obs_scale 1; a censor flag on a count is refused.
     *   A model with a count output takes the noise path, never the sigma rule's: add_index == NULL forms the specification with the
     * Gaussian outputs from est_sigma / sigma_fixed and the count outputs fixed at 1 (so a negative-binomial output, which needs its
     * b_k, is refused there, and so is est_sigma != 0 without a Gaussian output).
     *   Data: a finite value of a count output is a non-negative integer <= 2^53; NaN is "not measured" as ever.
     *   Likelihood (user_models.count_loglik is the definition in NumPy; y = obs, mu = f):
     *     Poisson   log p = -c(y) - x,  c(y) = lgamma(y + 1) - y log y + y (the saturated model: a data constant, summed per experiment
     *               on the host as C_e),  x = bd0(y, mu) = y log(y / mu) + mu - y;  x = mu for y = 0
     *     neg. binomial  log p = -x;  u = b^2 mu, phi = 1 / b^2, n = phi + y, n p = n / (1 + u), n q = mu (1 + b^2 y) / (1 + u), L = log1p(b^2 y):
     *               x = L - [stirlerr(n) - stirlerr(phi) - stirlerr(y) - bd0(phi, n p) - bd0(y, n q)] - 1/2 [L - log(2 pi y)];  y = 0: phi log1p(u)
     *     Loader's saddle-point form: bd0(x, m) = x log(x / m) + m - x, by its series in (x - m) / (x + m) where |x - m| < 0.1 (x + m);
     *               stirlerr(n) = lgamma(n + 1) - (n + 1/2) log n + n - 1/2 log(2 pi), as written up to n = 15, by its series above
     *   x is clamped at >= 0; mu NaN gives NaN (a failed output's route); mu < 0, mu = +inf, or mu = 0 with y > 0 give logL = -inf;
     *   mu = 0 with y = 0 gives x = 0; any b_k < 0, or b_k <= 0 on a negative-binomial output: logL = -inf.  m_e, m_ek count Gaussian
     *   quantified values only:   lk = sum_e [ (-m_e / 2) log(2 pi) - sum_k m_ek log(a_k s_k) - C_e - X_e ].
     * In this form no large numbers cancel and no lgamma of an argument above 16 is taken: every term is within 1e-11 max(1, |term|)
     * of its 60-digit value for counts up to 2^53, means from 1e-300 y to 1e5 y and b from 10 down to 1e-6, where the negative
     * binomial has become the Poisson (tests/test_likelihood_terms_truth.py).  Below b = 1e-7 phi + y no longer holds a small y:
     * declare the output Poisson, or keep the prior off 0 (a gamma or log-normal prior does: PRIOR FAMILIES at smc_set_prior_ex).
     * Early rejection stays exact (the
     * floors do not depend on the solve); the LDS table does not grow.  smc_user_predict returns lk under this
     * likelihood, designs give the mean; smc_user_predict_summary with noise = 1 is refused (it draws Gaussian noise only), noise = 2
     * draws replicated counts, and smc_user_pointwise_summary_opt ranks the observed counts among them (the PIT).
     * smc_user_obs_family and smc_user_count_check below apply the rules without a GPU.  A dump of such a source also writes
     * user_count.h. */
} smc_user_model_spec;
/* DISPATCH, one rule over the fields (an absent feature takes the earlier path, and its bits with it):
 *   n_obs == 0                        the one-output model; obs_scale, a noise array, inputs, events or censor given: refused;
 *   n_in == 0 / n_ev == 0             in_t, in_u / ev_t, ev_v must be NULL;
 *   censor NULL or all zeros          no censoring; else the data rules run, then the flags' rules, and the model takes the noise
 *                                     path - with add_index NULL under the specification formed from est_sigma / sigma_fixed;
 *   add_index given                   the specification's rules run; one that is the sigma rule's model (no prop_index, no
 *                                     censoring, every output at the last parameter or fixed at one value) takes the sigma rule's path;
 *   add_index NULL                    the sigma rule; another noise array given: refused.
 * Messages about the consistency of the arguments start with the name of the called function, a feature's own messages with the
 * name of the entry point that introduced it (smc_set_model_user5: inputs, 6: events, 7: censoring, 3 / 4: the LDS table). */
int smc_set_model_user_spec(smc_ctx *ctx, const smc_user_model_spec *spec);
int smc_user_model_check_spec(const smc_user_source_spec *spec, char *log, int log_cap);
/* smc_user_model_dump_source_spec writes exactly what hiprtc is given for the spec into the existing directory `dir`: smc_user_model.hip (the user's functions
 * followed by the library's kernel) and the headers it includes - to read, or to compile off line
 * (`hipcc --offload-arch=gfx950 -O3 -ffp-contract=on -fno-fast-math -I dir -S dir/smc_user_model.hip`; the build container's
 * tests run the compiler's uniformity analysis on it).  0 ok, 1 a file could not be written, 2 bad arguments.  No GPU needed. */
int smc_user_model_dump_source_spec(const smc_user_source_spec *spec, const char *dir);
/* sizeof and, in declaration order, offsetof of every field of smc_user_source_spec (which = 0) or smc_user_model_spec (which = 1)
 * as this library was compiled: returns sizeof, or -1 for another `which`, and fills offsets[0 .. min(cap, fields)).  A binding
 * that mirrors the structs compares its own layout with it. */
int smc_user_spec_layout(int which, int *offsets, int cap);
/* the rules of one feature alone (no GPU, no context: the reason is in smc_last_error(NULL)), and the inputs / events of a design */
int smc_user_noise_check(int n_obs, int dim, const int *add_index, const double *add_fixed, const int *prop_index,
                         const double *prop_fixed);
int smc_user_input_check(const double *in_t, const double *in_u, int n_ex, int n_in, int n_knot);
int smc_user_event_check(const double *t, const double *ev_t, const double *ev_v, int n_ex, int n_t, int n_ev, int n_val);
int smc_user_censor_check(const double *t, const double *obs, const signed char *censor, int n_ex, int n_t, int n_obs, int c_n_ex,
                          int c_n_t, int c_n_obs);
/* count observations: the family list of a source - the number of entries (the first min(n, cap) of them in family, as written:
 * whether an entry is 0, 1 or 2 is smc_user_count_check's rule), 0 for a source without the name smc_user_obs_family, -1 for a
 * list that is not written as one (the reason in smc_last_error(NULL)) ... */
int smc_user_obs_family(const char *source, int *family, int cap);
/* ... and the rules of a model with that list (n_family entries): the list against n_obs (0: the one-output model), then - for
 * t n_ex x n_t and obs n_ex x n_t x n_obs - the data rules, the flags' rules (censor NULL: none), and the rules of COUNT
 * OBSERVATIONS over obs_scale (NULL: ones), est_sigma and the noise arrays (NULL: absent) and the values.  n_family = 0: nothing
 * to check. */
int smc_user_count_check(const int *family, int n_family, const double *t, const double *obs, const signed char *censor,
                         const double *obs_scale, int n_ex, int n_t, int n_obs, int est_sigma, const int *add_index,
                         const double *add_fixed, const int *prop_index, const double *prop_fixed);
int smc_user_set_design_inputs(smc_ctx *ctx, const double *in_t_new, const double *in_u_new, int n_ex_new, int n_knot_new);
int smc_user_set_design_events(smc_ctx *ctx, const double *ev_t_new, const double *ev_v_new, int n_ex_new, int n_ev_new);
/* EARLIER ENTRY POINTS, kept with their signatures, return codes and messages: each fills the fields named by its arguments and
 * leaves every other field zero.  Where they take an n_obs it is 1 .. SMC_USER_MAX_OBS (0 is refused, not the one-output model).
 *   smc_set_model_user         n_obs = 0, method RK45: source, n_states, t, obs, cond, n_ex, n_t, n_cond, est_sigma, sigma_fixed, rtol, atol
 *   smc_set_model_user2        ... and method
 *   smc_set_model_user3        n_obs and obs_scale as well; no noise arrays (never the noise path), inputs, events, censor
 *   smc_set_model_user4        as 3 with the four noise arrays in place of est_sigma / sigma_fixed; a NULL add_index is refused
 *   smc_set_model_user5        as 3 and 4 together (add_index NULL: the sigma rule), and in_t, in_u, n_in, n_knot
 *   smc_set_model_user6        ... and ev_t, ev_v, n_ev, n_val
 *   smc_set_model_user7        every field
 *   smc_user_model_check / dump_source       source, n_states, dim; method RK45, n_obs = 0
 *   ...2                       ... and method
 *   ...3                       ... and n_obs
 *   ...4                       ... and noise = 1, or 2 with `proportional` != 0
 *   ...5                       ... noise as given, and n_cond, n_in, n_knot
 *   ...6                       ... and n_ev, n_val
 *   ...7                       every field */
int smc_set_model_user(smc_ctx *ctx, const char *source, int n_states, const double *t, const double *obs, const double *cond,
                       int n_ex, int n_t, int n_cond, int est_sigma, double sigma_fixed, double rtol, double atol);
int smc_set_model_user2(smc_ctx *ctx, const char *source, int n_states, const double *t, const double *obs, const double *cond,
                        int n_ex, int n_t, int n_cond, int est_sigma, double sigma_fixed, double rtol, double atol, int method);
int smc_user_model_check(const char *source, int n_states, int dim, char *log, int log_cap);
int smc_user_model_check2(const char *source, int n_states, int dim, int method, char *log, int log_cap);
int smc_user_model_dump_source(const char *source, int n_states, int dim, const char *dir);
int smc_user_model_dump_source2(const char *source, int n_states, int dim, int method, const char *dir);
int smc_set_model_user3(smc_ctx *ctx, const char *source, int n_states, int n_obs, const double *t, const double *obs,
                        const double *cond, const double *obs_scale, int n_ex, int n_t, int n_cond, int est_sigma, double sigma_fixed,
                        double rtol, double atol, int method);
int smc_user_model_check3(const char *source, int n_states, int dim, int method, int n_obs, char *log, int log_cap);
int smc_user_model_dump_source3(const char *source, int n_states, int dim, int method, int n_obs, const char *dir);
int smc_set_model_user4(smc_ctx *ctx, const char *source, int n_states, int n_obs, const double *t, const double *obs,
                        const double *cond, const double *obs_scale, int n_ex, int n_t, int n_cond, const int *add_index,
                        const double *add_fixed, const int *prop_index, const double *prop_fixed, double rtol, double atol, int method);
int smc_user_model_check4(const char *source, int n_states, int dim, int method, int n_obs, int proportional, char *log, int log_cap);
int smc_user_model_dump_source4(const char *source, int n_states, int dim, int method, int n_obs, int proportional, const char *dir);
int smc_set_model_user5(smc_ctx *ctx, const char *source, int n_states, int n_obs, const double *t, const double *obs,
                        const double *cond, const double *obs_scale, int n_ex, int n_t, int n_cond, const int *add_index,
                        const double *add_fixed, const int *prop_index, const double *prop_fixed, double rtol, double atol, int method,
                        int est_sigma, double sigma_fixed, const double *in_t, const double *in_u, int n_in, int n_knot);
int smc_user_model_check5(const char *source, int n_states, int dim, int method, int n_obs, int noise, int n_cond, int n_in, int n_knot,
                          char *log, int log_cap);
int smc_user_model_dump_source5(const char *source, int n_states, int dim, int method, int n_obs, int noise, int n_cond, int n_in,
                                int n_knot, const char *dir);
int smc_set_model_user6(smc_ctx *ctx, const char *source, int n_states, int n_obs, const double *t, const double *obs,
                        const double *cond, const double *obs_scale, int n_ex, int n_t, int n_cond, const int *add_index,
                        const double *add_fixed, const int *prop_index, const double *prop_fixed, double rtol, double atol, int method,
                        int est_sigma, double sigma_fixed, const double *in_t, const double *in_u, int n_in, int n_knot,
                        const double *ev_t, const double *ev_v, int n_ev, int n_val);
int smc_user_model_check6(const char *source, int n_states, int dim, int method, int n_obs, int noise, int n_cond, int n_in, int n_knot,
                          int n_ev, int n_val, char *log, int log_cap);
int smc_user_model_dump_source6(const char *source, int n_states, int dim, int method, int n_obs, int noise, int n_cond, int n_in,
                                int n_knot, int n_ev, int n_val, const char *dir);
int smc_set_model_user7(smc_ctx *ctx, const char *source, int n_states, int n_obs, const double *t, const double *obs,
                        const double *cond, const double *obs_scale, int n_ex, int n_t, int n_cond, const int *add_index,
                        const double *add_fixed, const int *prop_index, const double *prop_fixed, double rtol, double atol, int method,
                        int est_sigma, double sigma_fixed, const double *in_t, const double *in_u, int n_in, int n_knot,
                        const double *ev_t, const double *ev_v, int n_ev, int n_val, const signed char *censor);
int smc_user_model_check7(const char *source, int n_states, int dim, int method, int n_obs, int noise, int n_cond, int n_in, int n_knot,
                          int n_ev, int n_val, int censor, char *log, int log_cap);
int smc_user_model_dump_source7(const char *source, int n_states, int dim, int method, int n_obs, int noise, int n_cond, int n_in,
                                int n_knot, int n_ev, int n_val, int censor, const char *dir);
/* Model PREDICTIONS of a user model (any of the three set functions; RK45 or BDF), for n host particles (n x dim, AoS; any n -
 * run in chunks of n_local): lk[n] as smc_loglik computes it and, unless pred is NULL, pred[((p * n_ex + e) * n_t + i) * n_obs + k]
 * = output k at t[e][i], written for every finite time whether or not obs is measured there; NaN past a row's end and from
 * where a solve failed on.  Raw outputs, not divided by s_k.  Own staging buffers: the particle sets and their lk are not
 * touched.  No early rejection.  n_failed / attempts (may be NULL) and, for BDF, smc_user_sweep_counters report THIS call's
 * work.  A model of smc_set_model_user / 2 is predicted by a kernel compiled at its first call and needs data that
 * smc_set_model_user3 would accept with no NaN. */
int smc_user_predict(smc_ctx *ctx, const double *particle, int64_t n, double *lk, double *pred, int64_t *n_failed, int64_t *attempts);
/* Predictions on a DESIGN other than the data's: t_new (n_ex_new x n_t_new) and cond_new (n_ex_new x n_cond), by the row rules
 * of smc_set_model_user3 - a finite strictly increasing run, then only NaN; t_new[e][0] is the initial time; integration runs to
 * the row's last finite time.  Replaces setting the model again with all-NaN observations in order to predict at other times or
 * for an experiment that was never run.  pred[((p * n_ex_new + e) * n_t_new + i) * n_obs + k], NaN past a row's end and from
 * where a solve failed on; raw outputs.  t_new == NULL: the data's own design - pred, n_failed and attempts are then those of
 * smc_user_predict, bit for bit (and the data-side refusal of a one-output model applies).  An explicit design works for every
 * user model (a model of smc_set_model_user / 2 through its prediction kernel, compiled at the first call).  The design reaches
 * the kernel as a second LDS image with every observation NaN: no recompile.  A design whose image exceeds the kernel's LDS table
 * runs in groups of consecutive experiments; n_failed then counts a particle once per group in which one of its solves failed.
 * Fails with the reason for a design that breaks the row rules, and with the bytes needed and available when a single row does
 * not fit the table.  Own staging buffers: the particle sets and their lk are not touched. */
int smc_user_predict_at(smc_ctx *ctx, const double *particle, int64_t n, const double *t_new, const double *cond_new, int n_ex_new,
                        int n_t_new, double *pred, int64_t *n_failed, int64_t *attempts);
/* Posterior predictive SUMMARIES of a resident particle set, formed on the device: replaces downloading the set, smc_user_predict
 * of it (n x n_ex x n_t x n_obs doubles over the bus) and a reduction on the host.  set: SMC_SET_PRED or SMC_SET_FILT, its n_local
 * particles equally weighted (the resampled posterior).  Design as smc_user_predict_at (t_new == NULL: the data's).  A cell is
 * (experiment e, time i, output k), index c = (e * n_t_new + i) * n_obs + k.  Per cell, over the m = n_finite[c] finite
 * predictions (NaN past a row's end and where a solve failed): mean[c], sd[c] (population, two-pass; summed in a fixed order, a
 * repeated call returns the same bits), and for every probs[j] (0 < n_probs <= 16, each in [0, 1]) the order statistics of ranks
 * floor and ceil of (m - 1) probs[j] in lower[j * cells + c] and upper[j * cells + c] - the elements numpy.nanquantile picks with
 * method "lower" / "higher"; exact (a radix select), no sketch.  m = 0: NaN in all of them.
 * noise != 0: the summaries are of replicated observations pred + sigma_p s_k z - sigma_p the particle's last parameter (est_sigma)
 * or sigma_fixed, s_k the model's obs_scale, z a standard normal (Philox4x32-10, Box-Muller) keyed by (seed, global_offset + p,
 * c): independent of the staging groups.  noise == 0 draws nothing.  noise = 1 (SMC_PRED_NOISE_GAUSSIAN) on a model with a count
 * output is refused: it calls no count sampler.
 * noise = 2 (SMC_PRED_NOISE_FAMILY): replicated observations of EVERY family.  A Gaussian output gets noise = 1's value, bit for bit
 * (block 0 of the cell's Philox stream); a count output's value is a count drawn with the prediction as its mean - Poisson, or
 * negative binomial with the particle's b_k (mean mu, variance mu + (b_k mu)^2: Poisson(mu b_k^2 G), G ~ Gamma(1 / b_k^2, 1)) - from
 * blocks 1, 2, .. of the same stream: inversion below a mean of 10, Hoermann's PTRS from there on, Marsaglia-Tsang for the gamma
 * (csrc/count_draw.h; tests/count_draw_reference.py is the same in NumPy).  The draw is NaN, and leaves n_finite like a failed
 * solve, for a mean that is NaN, negative, infinite or >= 2^52 and for a b_k that is not finite and > 0 on a negative-binomial
 * output.  On a model without count outputs noise = 2 is noise = 1.
 * Staging: predictions plus keys, 2 x n_local x n_t_new x n_obs x 8 B per experiment, stay within max_staging_bytes (0: most of the
 * free device memory) by running groups of experiments; a single experiment that does not fit is refused with the bytes needed.
 * Nothing with a particle axis leaves the device: cells x (3 + 2 n_probs) numbers and the counters come back in one
 * synchronisation.  The particle sets, their lk, the accept flags and smc_work_totals stay as they were.  n_failed / attempts as
 * smc_user_predict_at.  kernel_ms (may be NULL): [0] the prediction sweeps, [1] the summary kernels, from events.
 * Several ranks: the summary describes THIS rank's block of particles only; merging order statistics across ranks is not done. */
#define SMC_PRED_NOISE_GAUSSIAN 1
#define SMC_PRED_NOISE_FAMILY 2
int smc_user_predict_summary(smc_ctx *ctx, int set, const double *t_new, const double *cond_new, int n_ex_new, int n_t_new,
                             const double *probs, int n_probs, int noise, uint64_t seed, int64_t global_offset,
                             size_t max_staging_bytes, double *mean, double *sd, double *lower, double *upper, int64_t *n_finite,
                             int64_t *n_failed, int64_t *attempts, double *kernel_ms);
/* POINTWISE LOG-LIKELIHOOD of a user model (any set function; RK45 or BDF), on the data's design - there are no observations
 * elsewhere.  A cell is (experiment e, time i, output k), index c = (e * n_t + i) * n_obs + k (a one-output model: n_obs = 1); it
 * is OBSERVED when obs is finite at a finite time of its row (a censored value is observed).  The term l of an observed cell for
 * a particle with prediction f, a_k, b_k its output's noise parameters (the sigma rule: a_k = sigma, b_k = 0), s_k its scale:
 *   Gaussian, quantified   -1/2 log(2 pi) - 1/2 log sd^2 - r^2 / (2 sd^2),  sd^2 = (a_k s_k)^2 + (b_k f)^2,  r = obs - f
 *   censored               log Phi(z), z = r / sd (at or below obs) or -r / sd (at or above obs)
 *   Poisson                log of the Poisson probability of the count obs under the mean f
 *   negative binomial      ... of the negative-binomial one with mean f and variance f + (b_k f)^2
 * NaN where the cell is not observed or f is NaN (a failed solve, or the model's own NaN); -inf in every other observed cell of a
 * particle whose parameters make logL -inf (an a_k <= 0, a b_k < 0, b_k <= 0 on a negative-binomial output).  The sum of a
 * particle's terms is its logL (smc_user_predict's lk) up to the order of the sum.  user_models.pointwise_loglik is the
 * definition in NumPy.
 * smc_user_pointwise: n host particles (n x dim, AoS; any n, in chunks of n_local) -> ll[p * cells + c].  Own staging; the sets and
 * their lk are not touched; n_failed / attempts as smc_user_predict. */
int smc_user_pointwise(smc_ctx *ctx, const double *particle, int64_t n, double *ll, int64_t *n_failed, int64_t *attempts);
/* ... and its per-cell STATISTICS over a resident particle set, formed on the device - what lppd / WAIC and a PIT histogram are made
 * of; replaces downloading the set, smc_user_predict of it and the family terms on the host.  set: SMC_SET_PRED or SMC_SET_FILT,
 * its n_local particles equally weighted.  Per cell c, over the particles whose term is not NaN (-inf counts): n[c], max[c],
 * sum_exp[c] = sum exp(l - max), mean[c] = sum l / n, m2[c] = sum (l - mean)^2 (two-pass) - raw, so that the statistics of several
 * ranks' blocks merge (user_models.pointwise_merge): lpd = max + log(sum_exp / n), var = m2 / (n - 1).  n = 0: NaN in all but n.
 * pit[c], for an observed quantified Gaussian cell: the mean of Phi((obs - f) / sd) over the particles with a finite f and valid
 * noise parameters; NaN elsewhere (a censored cell has none; a count cell's is formed from replicated draws by
 * smc_user_pointwise_summary_opt below, and stays NaN here).  Every sum runs per thread in index
 * order and then through a fixed tree (no atomics): a repeated call returns the same bits, and so does any max_staging_bytes.
 * Staging as smc_user_predict_summary's (predictions plus terms, 2 x n_local x n_t x n_obs x 8 B per experiment) plus 1/32 of it
 * for the PIT partials, within max_staging_bytes (0: most of the free device memory) by running groups of experiments; a single
 * experiment that does not fit is refused with the bytes needed.  cells x 6 numbers and the counters come back in one
 * synchronisation.  The particle sets, their lk, the accept flags and smc_work_totals stay as they were.  kernel_ms (may be
 * NULL): [0] the prediction sweeps, [1] the pointwise kernels, from events.  Several ranks: THIS rank's block only. */
int smc_user_pointwise_summary(smc_ctx *ctx, int set, size_t max_staging_bytes, int64_t *n, double *max, double *sum_exp, double *mean,
                               double *m2, double *pit, int64_t *n_failed, int64_t *attempts, double *kernel_ms);
/* ... with options; opts == NULL is smc_user_pointwise_summary, bit for bit (which is this call with NULL).
 * count_pit != 0: the PIT of COUNT cells, without a CDF.  For every observed count cell c with observation y, over the particles with
 * a finite prediction f and valid noise parameters - their number is pit_n[c] - a replicated count is drawn with mean f (Poisson, or
 * negative binomial with the particle's b_k; the sampler of smc_user_predict_summary's noise = 2) from the Philox stream keyed by
 * (seed, global_offset + p, tag 0x504954, c); pit_below[c] counts the draws < y and pit_equal[c] those == y (a NaN draw, f < 0 or
 * >= 2^52, is neither).  below / n estimates F(y - 1) and equal / n the mass at y: user_models.count_pit and pit_histogram make the
 * randomised PIT and the non-randomised histogram of them.  Integer counts: blocks of particles and ranks merge by addition, and
 * staging groups cannot change them.  All three are 0 on every other cell, and on a model without count outputs.  pit stays NaN
 * on count cells; every other result is the one of a call without options.  Staging grows by 4 B per 32 particles and cell. */
typedef struct smc_pointwise_opts {
    int count_pit;
    uint64_t seed;
    int64_t global_offset;
    int64_t *pit_below, *pit_equal, *pit_n;      /* cells each; needed with count_pit != 0 */
} smc_pointwise_opts;
int smc_user_pointwise_summary_opt(smc_ctx *ctx, int set, size_t max_staging_bytes, const smc_pointwise_opts *opts, int64_t *n,
                                   double *max, double *sum_exp, double *mean, double *m2, double *pit, int64_t *n_failed,
                                   int64_t *attempts, double *kernel_ms);
/* BDF user model: device-counted work of the LAST smc_loglik / smc_mh_step_* sweep, in the manner of
 * smc_meth_sweep_counters: out = {accepted BDF steps, Newton iterations, LU factorisations, Jacobian evaluations} summed over
 * the sweep's solves (masked proposals left out).  Fails with a message for an RK45 model. */
int smc_user_sweep_counters(smc_ctx *ctx, int64_t out[4]);
/* Methanation model: device-counted work of the LAST smc_loglik / smc_mh_step_* call (the counts the K8
 * roofline is built from): out = {accepted BDF steps, Newton iterations, Jacobian factorisations, failed solves}. */
int smc_meth_sweep_counters(smc_ctx *ctx, int64_t out[4]);
/* Completeness of the LAST methanation sweep: out = {DAE solves asked for (live (particle, experiment) pairs), solves
 * finished, live items whose status was still the pre-sweep poison value when the likelihood was formed, waves that were
 * incomplete at a dequeue, solves NOT started because their proposal was already certain to be rejected}.  A sweep with
 * out[1] + out[4] != out[0] or out[2], out[3] != 0 makes smc_loglik / smc_mh_step_* fail (the reference's counterpart is
 * the bare except of methanation_set_likelihood.py:234-254: there a lost solve would surface as an exception at ray.get).
 * Exact early rejection (smc_set_early_reject, default on) also covers the methanation sweeps: the accept test
 * exp((lk2 - lk1) * gamma) >= rr (SMC_methanation_main.py:376-383) has lk1 and rr fixed beforehand and my_loglike only
 * falls with every experiment added to it, so a proposal that fails the test on the experiments finished SO FAR is
 * rejected exactly as the full computation would reject it and its remaining DAE solves are skipped (out[4]); the sweep
 * runs experiment-major so that a proposal's experiments come up one after the other.  p_filt, lk1, accept flags and
 * counts are unchanged; lk2 of such a proposal is never formed (debug capture switches the feature off). */
int smc_meth_sweep_check(smc_ctx *ctx, int64_t out[5]);
/* Outlet flows (n x n_data x 5, the F_k of methanation_set_likelihood.py:204-208; -10000 where the solve failed, :244-249)
 * and solver status (n x n_data: 0 solved, 1 given up, -1 not solved in this sweep = masked proposal) of the LAST sweep -
 * what my_model returns per particle before my_loglike reduces it (the reference keeps them as C_l_ for its plots). */
int smc_meth_download_solves(smc_ctx *ctx, double *flows, int32_t *status, int64_t n);
/* Independent priors, one per parameter: kind[i] in {SMC_PRIOR_UNIFORM, SMC_PRIOR_NORMAL, SMC_PRIOR_FLAT}; (a,b) =
 * (low,high) or (mu,sigma).  Used by the support mask of cal_prior (Micmem_SMC_main.py:60-90,
 * 224-228) and by smc_sample_prior_device.  Any other kind is refused with the parameter's index ("Unknown prior kind: parameter i:
 * kind k ..."); for a family of smc_set_prior_ex the message names that entry point. */
int smc_set_prior(smc_ctx *ctx, const int *kind, const double *a, const double *b, int dim);
/* PRIOR FAMILIES on a positive or bounded parameter (priors.py is the definition in NumPy).  kind[i] may also be
 *   SMC_PRIOR_LOGNORMAL    (a, b) = (mu, sigma) of log x, sigma > 0      support x > 0            k = -L - (L - mu)^2 / (2 sigma^2), L = log x
 *   SMC_PRIOR_GAMMA        (a, b) = (shape, scale), both > 0             support x > 0            k = (shape - 1) log x - x / scale
 *   SMC_PRIOR_BETA         (a, b) > 0, lo < hi finite                    support lo < x < hi      k = (a - 1) log u + (b - 1) log1p(-u),
 *                                                                                                 u = (x - lo) / (hi - lo)
 *   SMC_PRIOR_TRUNCNORMAL  (a, b) = (mu, sigma), sigma > 0, lo < hi,     support lo <= x <= hi    k = -y^2 / 2, y = (x - mu) / sigma
 *                          either bound may be infinite
 * k is the LOG-KERNEL: the log-density without its normaliser, which cancels in the Metropolis ratio (the device needs no lgamma
 * and no erf).  lo / hi are read for SMC_PRIOR_BETA and SMC_PRIOR_TRUNCNORMAL only and may be NULL when neither kind is present;
 * for the kinds of smc_set_prior, (a, b) mean what they mean there.  Outside its support a family's density is exactly 0 (k =
 * -inf), never NaN - at x = +inf too; a NaN argument gives NaN and counts as outside.  A beta's test is made on u as rounded as well
 * (0 < u < 1): an x within an ulp of an end is outside.
 * In the propose kernels of all three model families, with P the product of the densities of the smc_set_prior kinds (as before)
 * and K the sum of k over the parameters of the new kinds: a proposal is in support iff P(cand) > 0 and every new-kind parameter of
 * it is in its support - otherwise it is reset to the current point and rejected (SMC_PRIOR_MODE_RATIO keeps its one exception: a
 * candidate outside the support of a smc_set_prior kind alone is not reset there, as before; one outside a new kind's is, so that
 * no model is solved at a negative level or fraction).  In the ratio modes p0_2 / p0_1 = P(cand) / P(cur) * exp(K(cand) - K(cur))
 * for a candidate in support and 0 otherwise.  SMC_PRIOR_MODE_MASK applies the support alone, as it does for a normal: A DENSITY
 * ONLY ACTS UNDER SMC_PRIOR_MODE_RATIO_MASK / SMC_PRIOR_MODE_RATIO.  With no new kind the kernels take the path, and give the
 * bits, they had before.
 * smc_sample_prior_device draws a new kind from the uniform supply of csrc/count_draw.h keyed by (seed, global particle, tag
 * 0x505249, cell = parameter index) - csrc/prior_draw.h: exp(mu + sigma z); scale * Gamma(shape) by Marsaglia-Tsang; G1 / (G1 + G2)
 * of two such gammas on one supply, mapped to (lo, hi); mu + sigma z repeated until it lies in [lo, hi] - while the parameters
 * of the smc_set_prior kinds keep their stream and their bits whatever stands beside them.
 * Rules: a, b as listed (finite); a gamma's shape and a beta's a, b at least 1/16 (the draw's boost u^(1 / shape) underflows to 0 with
 * probability exp(-745 shape): below the bound a gamma draw could be exactly 0, outside its support, and a beta draw 0 / 0); lo < hi, finite for a beta, not NaN for a truncated normal; a truncated normal keeps at least half
 * of its mass, Phi((hi - mu) / sigma) - Phi((lo - mu) / sigma) >= 1/2 (formed with erfc) - the draw is by rejection and under this
 * rule a dry supply (NaN) has probability at most 2^-254; for less mass use a uniform or a shifted normal.  A broken rule fails with
 * the parameter's index and the rule.  smc_prior_check applies the rules alone (no GPU, no context: the reason is in
 * smc_last_error(NULL)). */
int smc_set_prior_ex(smc_ctx *ctx, const int *kind, const double *a, const double *b, const double *lo, const double *hi, int dim);
int smc_prior_check(const int *kind, const double *a, const double *b, const double *lo, const double *hi, int dim);
/* SMC_PRIOR_MODE_*: default SMC_PRIOR_MODE_MASK (the live branch of both reference drivers). */
int smc_set_prior_mode(smc_ctx *ctx, int mode);

/* Resampling scheme of smc_resample_phase1/2 (BASELINE.json names systematic resampling; the reference implements
 * only the residual-systematic variant, Micmem_SMC_main.py:147-184, which stays the default):
 *   SMC_RESAMPLE_RESIDUAL_SYSTEMATIC  trunc(N w_i) copies + systematic draws on the residuals
 *   SMC_RESAMPLE_SYSTEMATIC           systematic draws on the weights themselves (thresholds (u + k)/N)
 *   SMC_RESAMPLE_MULTINOMIAL          N iid draws: the thresholds are the order statistics of N uniforms, produced on
 *                                     the device as normalised partial sums of N+1 exponentials (Philox, seeded by
 *                                     the bits of `wrand`); offspring land sorted by ancestor like the other schemes */
#define SMC_RESAMPLE_RESIDUAL_SYSTEMATIC 0
#define SMC_RESAMPLE_SYSTEMATIC 1
#define SMC_RESAMPLE_MULTINOMIAL 2
/* Exact early rejection in the Metropolis sweeps of the Michaelis-Menten model (default: on).  The accept test
 * exp((lk2-lk1)*gamma)*p0 >= rr (Micmem_SMC_main.py:231-236) has lk1 and rr fixed before the proposal is solved, and lk2 = sum
 * over the experiments of c0 - sum(residual^2)/(2 sigma^2) only decreases while a solve accumulates residuals.  A solve
 * whose proposal fails the test even with the sums accumulated SO FAR (0 for experiments still running) is stopped: the
 * proposal is rejected exactly as the completed computation would reject it - p_filt, lk1, accept flags and counts are
 * unchanged; only rk_attempts is smaller, a step-size underflow in the skipped part of a solve cannot be reported (the
 * reference would raise there; none occurs on this model), and the lk2 of such a proposal is never formed (the debug
 * capture therefore switches the feature off).  It removes the long solves that dominate the early tempering steps:
 * they are proposals with Vmax/Km in the thousands whose other experiments already rule them out. */
int smc_set_early_reject(smc_ctx *ctx, int enable);
/* Michaelis-Menten sweeps hand the predictably long solves (Vmax > 60 Km: RK45 runs on its stability limit for ~3.7 Vmax/Km
 * attempts) out BEFORE the index-ordered items (default: on), so that the serial chains that bound a sweep start at its
 * beginning, and run the stiffest of them (Vmax > 1000 Km, at most one solve per wave of the sweep's grid) SOLO: one wave per solve on
 * wave-uniform operands from the first attempt (0.33 - smc_set_fast_tail - instead of ~0.55 us per attempt while the rest of the population
 * keeps the other lanes busy).  The order in which independent (particle, experiment) solves run - and the lane count they
 * run on - changes no result: the reference's one-Ray-task-per-particle fan-out (Micmem_likelihood.py:83-87) leaves it to its
 * scheduler too; 0 restores round 2's plain index order (A/B timing, tests).  Methanation: the same switch selects the
 * misfit order of the experiments in the early-rejection sweeps (smc_meth_sweep_check). */
int smc_set_stiff_first(smc_ctx *ctx, int enable);
/* Michaelis-Menten Metropolis sweeps over a heterogeneous population hand their index-ordered solves out by cost class
 * (Vmax / Km of the proposal, four classes per octave, counting sort on the device) and in phase, so that the 64 solves a wave
 * starts together are alike: same results (the order of independent solves is free, as for smc_set_stiff_first), 20-25 % less
 * time for the sweeps of the middle of a run.  Default: on; needs smc_set_in_phase on.  0: A/B timing, tests. */
int smc_set_cost_order(smc_ctx *ctx, int enable);
/* A Michaelis-Menten solve that runs alone in its wave (a solo solve, the last survivor of a sweep) performs the attempts that
 * neither produce an output nor meet a special case in a hand-written instruction sequence (csrc/mm_rk45.h:
 * mm_fast_uniform_attempts: ~140 instead of ~190 instructions per attempt, the Dormand-Prince tableau resident in scalar
 * registers); every other attempt goes through the compiled step function.  Default: on.  The results are the same bit for
 * bit (tests/test_gpu_parity.py compares on and off); 0 is for that comparison and for A/B timing.  Parity mode
 * (smc_set_exact_pow) never uses it. */
int smc_set_fast_tail(smc_ctx *ctx, int enable);
/* Replicate experiments of a Michaelis-Menten data set - the same S0 and the same n_t data times, BIT FOR BIT - integrate the same
 * initial value problem for every particle: the same RK45 attempts, the same accept / reject decisions, the same dense-output
 * values; only P_obs differs.  smc_set_model_mm groups them (smc_mm_group_replicates) and a sweep then integrates ONCE per group
 * and accumulates the sums of squared residuals of both experiments of a pair (default: on; the environment variable
 * SMC_SHARE_REPLICATES=0 turns it off whatever this switch says, for A/B runs of one build under an unchanged caller).  Every result is the same bit for bit
 * (tests/test_gpu_shared_replicates.py compares on and off); the attempt counts keep their meaning "per experiment, as the
 * reference counts them": the partner's record repeats its primary's count, so rk_attempts includes attempts nobody executed -
 * smc_mm_share_info says how many.  A data set without replicates runs the same kernels whatever the switch says. */
int smc_set_share_replicates(smc_ctx *ctx, int enable);
/* The grouping itself, a pure host function (no device is touched): t is n_ex x n_t, S0 n_ex; primary[g] / partner[g] (-1: none)
 * receive the experiments of solve group g (both arrays n_ex long, unused entries -1), groups in order of first appearance, the
 * primary the lowest index, at most one partner: a condition that appears three or more times becomes pairs plus, if odd, a
 * single.  Returns the number of groups, or -1 for bad arguments. */
int smc_mm_group_replicates(const double *t, const double *S0, int n_ex, int n_t, int *primary, int *partner);
/* n_solve: solves per particle a sweep schedules now (the groups when sharing is on, else n_ex); shared_attempts: device-counted
 * RK45 attempts since the last smc_timing_reset that are in rk_attempts (smc_work_totals out[1], the sweeps' own counts) but were
 * not executed - the partners' copies.  Either pointer may be NULL.  Synchronises the stream. */
int smc_mm_share_info(smc_ctx *ctx, int *n_solve, int64_t *shared_attempts);
/* Rejection at start (Michaelis-Menten Metropolis sweeps, default: on; no effect unless smc_set_early_reject is on; the environment
 * variable SMC_START_REJECT=0 turns it off whatever this switch says).  The proposal kernel computes, per particle, the sum of squared
 * residuals from which the accept test is certain to fail (smc_mm_reject_threshold); an item of a later pass of the solve queue
 * adds up the sums its siblings have already published and, if they reach that threshold, is cancelled before its first attempt.
 * Every result is the same bit for bit (tests/test_gpu_start_reject.py compares on and off); only the attempt counters and the
 * solved / cancelled split differ, and depend on timing.  Off, the proposal kernel computes no thresholds and the solve kernel -
 * the same kernel, with a flag in its arguments clear - skips the look at one wave-uniform branch per started item.  On, the host
 * still drops both for the sweeps that follow a sweep which left fewer than 1 item in 100 unstarted (a posterior-like population
 * would pay the loads for nothing), until the next likelihood sweep of the context announces a new population. */
int smc_set_start_reject(smc_ctx *ctx, int enable);
/* not_started: (particle, experiment) items of this context's Michaelis-Menten Metropolis sweeps that were cancelled with no attempt
 * at all, since smc_create - device-counted by the accept kernel, summed on the host when a sweep's counters are read. */
int smc_mm_start_reject_info(smc_ctx *ctx, int64_t *not_started);
/* The threshold itself, a pure host function (no device is touched; the propose kernel evaluates the same inline function): finished
 * sums of squared residuals that add up to at least the returned value make the accept test
 *   exp((sum_k (c0 - S_k / (2 sigma^2)) - lk1) * gamma) * pratio >= rr,   c0 = -n_t / 2 * log(2 pi sigma^2),  k < n_ex,
 * fail in double precision whatever the other S_k >= 0 are.  pratio: 1.0 in SMC_PRIOR_MODE_MASK.  0 where the test fails with no
 * residual at all; +inf ("never") for every doubtful input: in_support == 0, rr outside (0, 1], sigma <= 0, gamma <= 0, pratio not
 * positive and finite, NaN or infinite arguments, and where the terms of a positive threshold cancel to three digits or more. */
double smc_mm_reject_threshold(double lk1, double gamma, double rr, double sigma, int n_ex, int n_t, double pratio, int in_support);
/* Michaelis-Menten Metropolis sweeps over a homogeneous population (the previous sweep of the context had fewer than one
 * (particle, experiment) solve in 20 000 with more than 64 RK45 attempts - counted on the device) run their waves IN PHASE
 * (default: on): a wave waits up to 12 attempts for all 64 lanes to finish before it starts its next 64 items, so that the
 * lanes stay at the same point of their trajectories and the dense-output loop runs as long as the average lane needs, not
 * the busiest (csrc/solve_sched.h).  Scheduling only: no result changes.  0 = hand out as soon as 24 lanes are idle, always. */
int smc_set_in_phase(smc_ctx *ctx, int enable);
/* Parity mode of the Michaelis-Menten step controller (default: off).  SciPy evaluates error_norm ** -0.2 (rk.py:155,169)
 * and x ** (1 / 5) (common.py:130) with libm's pow and the DOUBLE exponents -0.2 / 0.2 (= 1/5 + 1.1e-17).  The fast
 * device form (hardware log2 / exp2 seed + one correction, <= 1.5 ulp about the fifth root) differs from that in the last
 * bit of many arguments; on RK45's stability limit one such bit can flip one accept / reject decision and the solve then
 * follows another, equally valid step sequence (logL equal to 1e-8 ... 1e-6 only).  enable != 0 finishes the fast value to
 * the CORRECTLY ROUNDED pow(x, -0.2) / pow(x, 0.2) (double-double residual, csrc/pow_fifth_exact.h; checked against a 113-bit
 * reference on the CPU) - what libm returns except for about 8 of 10^4 arguments where glibc's own pow is not correctly
 * rounded - AND evaluates the Runge-Kutta stages, the error estimate and select_initial_step with every product and sum
 * rounded separately, in NumPy's order (no fused multiply-add; mm_rk45.h: rk_attempt_core_exact), as the CPU checker does:
 * the device then walks the checker's step sequence attempt for attempt, also in the stiff band
 * (test_stiff_band_parity_and_its_tolerance).  About 60 more operations per attempt.  run_smc switches it on with
 * rng="numpy" (the reference's stream) and the drop-in sim_particle uses it; the device-RNG default keeps the fast form. */
int smc_set_exact_pow(smc_ctx *ctx, int enable);
int smc_set_resampling(smc_ctx *ctx, int scheme);

/* ---- particle movement -------------------------------------------------------------------- */
int smc_upload_particles(smc_ctx *ctx, int set, const double *aos, int64_t n);   /* (n,d) -> SoA */
int smc_download_particles(smc_ctx *ctx, int set, double *aos, int64_t n);
int smc_upload_lk(smc_ctx *ctx, int set, const double *lk, int64_t n);
int smc_download_lk(smc_ctx *ctx, int set, double *lk, int64_t n);
/* r_ac, the ever-accepted flags of the current tempering step (Micmem_SMC_main.py:187,241). */
int smc_download_accept_flags(smc_ctx *ctx, uint8_t *flags, int64_t n);
/* Diagnostics (tools/sweep_tail_census.py): the per-(experiment, particle) record of the last Michaelis-Menten sweep over n
 * particles, info[e * n + p] = RK45 attempts | cancelled by early rejection << 29 | failed << 30.  n_ex * n entries. */
int smc_download_item_info(smc_ctx *ctx, int32_t *info, int64_t n);
/* ... and its sums of squared residuals, sums[e * n + p] (after a Metropolis sweep with early rejection: -1 for a cancelled solve). */
int smc_download_item_sums(smc_ctx *ctx, double *sums, int64_t n);
/* p_pred, lk = p_filt.copy(), lk1.copy() (Micmem_SMC_main.py:251-252): device-to-device. */
int smc_commit_filt_to_pred(smc_ctx *ctx);
/* Device-RNG prior draw into SMC_SET_PRED (replaces sample_prior, Micmem_settings.py:69-87, in
 * device-RNG mode): Philox4x32-10 keyed by (seed, global particle index, parameter). */
int smc_sample_prior_device(smc_ctx *ctx, uint64_t seed, int64_t global_offset);

/* ---- A2: likelihood sweep ----------------------------------------------------------------- */
/* sim_particle (Micmem_likelihood.py:79-92) on the resident set: lk[i] = log_likelihood_mm_multi(
 * theta_i) (Micmem_likelihood.py:35-77).  n_failed counts particles with a failed RK45 solve (their
 * lk is NaN; the reference raises there).  rk_attempts (optional) receives the device-counted number
 * of RK45 step attempts summed over particles x experiments (flop accounting). */
int smc_loglik(smc_ctx *ctx, int set, int64_t *n_failed, int64_t *rk_attempts);
/* Same for a host batch (the drop-in sim_particle surface): particle (n,3) in, lk[n] out and, when
 * pred != NULL, the model predictions C_l_ as n x n_ex x n_t (P_model, Micmem_likelihood.py:32,74).
 * Any n up to the context capacity. Does not disturb the resident sets. */
int smc_mm_loglik_host(smc_ctx *ctx, const double *particle, int64_t n, double *lk, double *pred, int64_t *n_failed,
                       int64_t *rk_attempts);

/* ---- A3/A4: tempered weights, ESS ---------------------------------------------------------- */
/* max(lk) over this rank's SMC_SET_PRED block (Micmem_SMC_main.py:116). */
int smc_max_lk_local(smc_ctx *ctx, double *max_lk);
/* For k < n_cand: sum_w[k] = sum_i exp((lk_i-max_lk)*gm[k]), sum_w2[k] = sum_i exp(...)^2 over this
 * rank's block (Micmem_SMC_main.py:118,124-134; ess = sum_w^2 / sum_w2 / N).  n_cand <= SMC_MAX_ESS_CAND. */
int smc_ess_partials(smc_ctx *ctx, double max_lk, const double *gm, int n_cand, double *sum_w, double *sum_w2);
/* The same two reductions over ALL ranks: the partial stays on the device, RCCL reduces it
 * in place on the context's stream (allreduce MAX of 1 f64 / SUM of 2 n_cand f64) and ONE read-back follows - no
 * device->host->device->host round trip per collective.  With one rank (no communicator) they equal the calls above. */
int smc_max_lk_global(smc_ctx *ctx, double *max_lk);
int smc_ess_partials_global(smc_ctx *ctx, double max_lk, const double *gm, int n_cand, double *sum_w, double *sum_w2);
/* One call, ONE synchronisation for a batch of the back-off search (Micmem_SMC_main.py:116-134): max(lk) over all ranks
 * (with_max != 0; it stays on the device), then the sums of up to 32 candidate increments in two back-to-back 16-candidate
 * passes that read the maximum from device memory, one all-reduce, one read-back.  sum_w / sum_w2: n_cand values, the same
 * numbers smc_max_lk_global + smc_ess_partials_global return (same kernels, same order of additions).  with_max == 0 reuses
 * the maximum of the previous call (the search going on beyond its first 32 candidates). */
int smc_ess_search_global(smc_ctx *ctx, const double *gm, int n_cand, int with_max, double *max_lk, double *sum_w,
                          double *sum_w2);

/* ---- A5: residual-systematic resampling (Micmem_SMC_main.py:147-184) ------------------------ */
/* Phase 1: with w_i = exp((lk_i-max_lk)*gm)/sum_weight_global, p_is_i = trunc(w_i*N_global) and the
 * residual w_i - p_is_i/N_global: returns this rank's sum of residuals and of p_is. */
int smc_resample_phase1(smc_ctx *ctx, double max_lk, double gm, double sum_weight_global, double *residual_sum_local,
                        int64_t *count_sum_local);
/* Phase 2: residual_prefix = sum of the residual sums of lower ranks; wrand = rand()/N_global (:156).
 * Adds the systematic offspring (:165-174) and builds the inclusive offspring scan.  Returns this
 * rank's total offspring. */
int smc_resample_phase2(smc_ctx *ctx, double max_lk, double gm, double sum_weight_global, double residual_prefix,
                        double wrand, int64_t *offspring_local);
/* Offspring counts p_is (after phase 2), for inspection / parity tests. */
int smc_download_offspring(smc_ctx *ctx, int64_t *p_is, int64_t n);
/* Phase 3 (:178-184): this rank's offspring occupy global output slots [out_base, out_base+offspring)
 * in ancestor order.  Slots owned by this rank are written straight into SMC_SET_FILT; slots owned by
 * other ranks are exchanged with grouped RCCL send/recv (smc_comm_init must have been called when
 * world > 1).  out_base_all / offspring_all: arrays of length world (the allgathered values).
 * Slots >= total offspring keep the content the reference's persistent p_filt would hold
 * (zeros before the first tempering step, the previous p_pred row afterwards). */
int smc_resample_phase3(smc_ctx *ctx, const int64_t *out_base_all, const int64_t *offspring_all, int first_step);
/* The send / receive plan phase 3 executes on rank `rank` of `world` (host arithmetic only: needs neither a context nor a
 * GPU).  Arrays of length world: send_off / send_cnt (one contiguous block per peer in the send staging, in particles),
 * src_lo (first local offspring index of the block for peer q; for q == rank the block that stays), recv_off / recv_cnt
 * (receive staging) and recv_row (first row of SMC_SET_FILT the block of peer q is spread over); own[3] = {src_lo, count,
 * first row} of the offspring that stay on the rank; stale_lo = first row nobody writes (n_local if none).  Any output
 * pointer may be NULL.  Returns 1 if out_base_all is not the exclusive prefix of offspring_all, 2 on bad arguments.
 * Sender and receiver plans must agree - send_cnt of rank s towards r == recv_cnt of rank r from s - and every row of every
 * rank must be written exactly once: tests/test_exchange_plan.py checks both for world sizes 2..8 without a GPU. */
int smc_exchange_plan(int world, int rank, int64_t n_local, const int64_t *out_base_all, const int64_t *offspring_all,
                      int64_t *send_off, int64_t *send_cnt, int64_t *src_lo, int64_t *recv_off, int64_t *recv_cnt,
                      int64_t *recv_row, int64_t *own, int64_t *stale_lo);
/* Micmem_SMC_main.py:147-184 across all ranks in one call: phase 1 -> all-gather of (residual sum, integer copies) ->
 * residual prefix of the lower ranks as a running sum in rank order (:165-167) -> phase 2 -> all-gather of the offspring
 * counts -> phase 3.  Two synchronisations instead of six.  n_offspring = sum of p_is over all particles (== N unless the
 * reference's stale-row case, :178-184, occurs), count_sum = sum of trunc(w*N) (the reference prints N - count_sum as n_tmp). */
int smc_resample_global(smc_ctx *ctx, double max_lk, double gm, double sum_weight_global, double wrand, int first_step,
                        int64_t *n_offspring, int64_t *count_sum);

/* The same resampling ENQUEUED: with one rank no number of it has to visit the host (the residual prefix of the lower ranks is
 * zero, the gather kernel reads the offspring total on the device), so the call returns without a synchronisation and the
 * Metropolis sweeps can be enqueued right behind it.  smc_resample_result - call it after your next synchronisation - returns
 * the two numbers the driver logs (n_offspring, count_sum as above) and fails if the resampler produced more offspring than
 * particles (the reference's IndexError, :180).  With several ranks smc_resample_enqueue is smc_resample_global. */
int smc_resample_enqueue(smc_ctx *ctx, double max_lk, double gm, double sum_weight_global, double wrand, int first_step);
int smc_resample_result(smc_ctx *ctx, int64_t *n_offspring, int64_t *count_sum);

/* Page-locked host memory for results (process-wide, valid until smc_pinned_free - also after smc_destroy): a download into it
 * is one DMA transfer; into pageable memory the runtime stages through its own buffers and copies on the host. */
int smc_pinned_alloc(size_t bytes, void **out);
int smc_pinned_free(void *p);

/* ---- A6: proposal covariance (np.cov(p_filt.T, bias=True), Micmem_SMC_main.py:212) ---------- */
/* sums[d] = sum_i theta_i over this rank's SMC_SET_FILT block. */
int smc_moment_sums_local(smc_ctx *ctx, double *sums);
/* centered[d*d] (row-major, symmetric) = sum_i (theta_i-mean)(theta_i-mean)^T over this rank's block. */
int smc_moment_centered_local(smc_ctx *ctx, const double *mean, double *centered);

/* ---- A7-A9: one random-walk Metropolis iteration, fused with the likelihood ------------------ */
/* Host-RNG (parity) mode.  noise is the (n,d) array np.random.multivariate_normal returned
 * (Micmem_SMC_main.py:220), rr the n uniforms of :235.  Performs :220-241 on SMC_SET_FILT in place:
 * proposal = p_filt + noise*mhstep_ratio; support mask p0; proposal reset where p0 == 0; lk2 =
 * likelihood(proposal); accept r = exp((lk2-lk1)*gamma)*p0 >= rr; select p_filt, lk1; r_ac = max(r_ac, r).
 * Outputs (local): accepted_now = sum(r), accepted_ever = sum(r_ac). */
int smc_mh_step_host_rng(smc_ctx *ctx, double gamma, double mhstep_ratio, const double *noise, const double *rr,
                         int64_t n, int64_t *accepted_now, int64_t *accepted_ever, int64_t *n_failed,
                         int64_t *rk_attempts);
/* Device-RNG mode.  noise_i = z_i @ transform (transform is d x d row-major, i.e. NumPy's
 * sqrt(s)[:,None]*v factor of cov_m), z_i and rr_i from Philox4x32-10 keyed by (seed, global particle
 * index = global_offset+i, stream).  Everything else as above. */
int smc_mh_step_device_rng(smc_ctx *ctx, double gamma, double mhstep_ratio, const double *transform, uint64_t seed,
                           uint64_t stream, int64_t global_offset, int64_t *accepted_now, int64_t *accepted_ever,
                           int64_t *n_failed, int64_t *rk_attempts);
/* One whole Metropolis iteration of the device-RNG mode on the stream (Micmem_SMC_main.py:212-241), every rank calling it
 * together: cov_m = np.cov(p_filt.T, bias=True) * w_cov (:212-215), the factor NumPy's legacy multivariate_normal multiplies
 * standard normals with - (u,s,v) = svd(cov_m), sqrt(s)[:,None]*v - computed on the device (cov_m is symmetric: a Jacobi
 * eigen-decomposition, |lambda| sorted descending, largest component of each row positive), then proposal, support mask,
 * likelihood, accept/select as in smc_mh_step_device_rng, then the accept counts summed over the ranks.  ONE synchronisation.
 * Moments: the first call after anything else wrote SMC_SET_FILT (upload, resampling, smc_mh_step_*) takes np.cov's own
 * two-pass route (column sums -> all-reduce -> sums centred about the global mean -> all-reduce); for the Michaelis-Menten
 * model every later call gets them from the accept kernel of the call before, which accumulates the moments of the
 * particles it selects about the previous mean - no pass over the particles, and moments + accept counts travel in ONE
 * all-reduce of d + d(d+1)/2 + 3 doubles.  w_cov: d x d (Micmem_settings.py:94-97).  accepted_now, accepted_ever and
 * n_failed are totals over ALL ranks, rk_attempts_local is this rank's; cov_m (optional, d x d) receives the global cov_m. */
int smc_mh_iteration_device_rng(smc_ctx *ctx, double gamma, double mhstep_ratio, const double *w_cov, uint64_t seed,
                                uint64_t stream, int64_t global_offset, int64_t *accepted_now, int64_t *accepted_ever,
                                int64_t *n_failed, int64_t *rk_attempts_local, double *cov_m);
/* A BATCH of those iterations with the loop control of Micmem_SMC_main.py:243-249 on the device: n_iter (1 .. 32) iterations are
 * enqueued back to back and the call synchronises ONCE.  After every iteration a one-block kernel takes the reference's
 * decision on the counts summed over all ranks: `break` when r_ac.sum() > thr_stop (= r_th * n_particle, :243-246) - every
 * kernel of the remaining iterations then returns at once - else mhstep_ratio *= 0.5 when r_ac.sum() < thr_halve
 * (= r_threshold_min * n_particle, :247-249); a failed solve also ends the loop.  Pass the two thresholds as the doubles
 * Python computes; counts are compared as exact doubles.  Iteration i draws with Philox stream stream0 + i and otherwise is
 * smc_mh_iteration_device_rng's iteration, bit for bit.  Outputs: n_done iterations ran (1 <= n_done <= n_iter), stopped != 0
 * if the loop ended by its break (or a failure) - otherwise the caller may enqueue the next batch with mhstep_ratio =
 * ratio_next; per iteration i < n_done (arrays of n_iter entries, each optional): accepted_now/ever and n_failed (all ranks),
 * rk_attempts_local (this rank), ratio_used (the mhstep_ratio it drew with), cov_m (n_iter x d x d, row-major).
 * sweep_counters (optional, n_iter x SMC_SWEEP_COUNTER_WORDS): this rank's device counters as iteration i left them, in the
 * order n_failed, rk_attempts (methanation: BDF steps), accepted_now, accepted_ever, newton_iters, factorisations, failed_solves,
 * expected_solves, completed_solves, unsolved_items, wave_split, cancelled_solves, long_items, solved_items - what
 * smc_meth_sweep_counters / smc_meth_sweep_check return after a single sweep (after the batch they describe its last sweep).
 * Michaelis-Menten (carried moments: one all-reduce per iteration) and methanation (np.cov's two passes per iteration: two
 * all-reduces, the second one carrying the counts); every kernel of an iteration tests the stop flag first, the experiment
 * order of the methanation sweeps is formed on the device.  A user model takes smc_mh_iteration_device_rng. */
#define SMC_SWEEP_COUNTER_WORDS 14
int smc_mh_sweeps_device_rng(smc_ctx *ctx, double gamma, double mhstep_ratio, const double *w_cov, uint64_t seed,
                             uint64_t stream0, int n_iter, double thr_stop, double thr_halve, int64_t global_offset,
                             int *n_done, int *stopped, double *ratio_next, int64_t *accepted_now, int64_t *accepted_ever,
                             int64_t *n_failed, int64_t *rk_attempts_local, double *ratio_used, double *cov_m,
                             int64_t *sweep_counters);
/* The first half of that iteration on its own (no model needed): cov_m = np.cov(p_filt.T, bias=True) * w_cov over all ranks
 * (:212-215) and the factor sqrt(s)[:,None]*v of its SVD, both d x d row-major; either output may be NULL. */
int smc_proposal_factor_device(smc_ctx *ctx, const double *w_cov, double *cov_m, double *transform);
/* The d x d factor (row-major) the last smc_mh_iteration_device_rng drew its proposals with. */
int smc_mh_iteration_last_transform(smc_ctx *ctx, double *transform);
/* r_ac = zeros (Micmem_SMC_main.py:187). */
int smc_reset_accept_flags(smc_ctx *ctx);
/* Copies of the last proposals/lk2 for parity tests (valid after an MH step when enabled). */
int smc_set_debug_capture(smc_ctx *ctx, int enable);
int smc_download_debug_proposals(smc_ctx *ctx, double *aos, double *lk2, uint8_t *p0, uint8_t *r, int64_t n);

/* ---- collectives (RCCL over xGMI) ------------------------------------ */
/* unique id = 128 bytes from smc_comm_get_unique_id on rank 0, broadcast by the launcher. */
int smc_comm_get_unique_id(uint8_t id[128]);
int smc_comm_init(smc_ctx *ctx, const uint8_t id[128], int rank, int world);
/* What RCCL itself says about the communicator of this context: ncclCommCount / ncclCommUserRank / ncclCommCuDevice
 * (count = 0, user_rank = device = -1 when there is none: a single rank needs no communicator).  A launcher can check
 * that RCCL saw as many ranks as it started. */
int smc_comm_info(smc_ctx *ctx, int *count, int *user_rank, int *device);
int smc_comm_allreduce_sum_f64(smc_ctx *ctx, double *inout, int n);
int smc_comm_allreduce_max_f64(smc_ctx *ctx, double *inout, int n);
int smc_comm_allreduce_sum_i64(smc_ctx *ctx, int64_t *inout, int n);
int smc_comm_allgather_f64(smc_ctx *ctx, const double *in, int n, double *out /* world*n */);
int smc_comm_allgather_i64(smc_ctx *ctx, const int64_t *in, int n, int64_t *out /* world*n */);
int smc_comm_barrier(smc_ctx *ctx);

/* ---- test and probe hooks (NOT part of the drop-in surface) -------------------------------------
 * Compiled into the library always (tests/ call them through the same C ABI), declared only when the includer asks:
 * a reference-side binding never needs them. */
#ifdef SMC_ENABLE_DEBUG_API
/* One-rank rehearsal of the particle exchange with real RCCL calls: rows [row, row+cnt) of the PRED set go through
 * the send staging, an ncclSend/ncclRecv pair addressed to this rank itself and the receive staging into rows
 * [dst_row, dst_row+cnt) of the FILT set (theta and lk) - step 3 of smc_resample_phase3 for a self-addressed block.
 * Needs a communicator (smc_comm_init with SMC_FORCE_RCCL=1 on one rank). */
/* Probes (tools/sort_probe.py): every Michaelis-Menten likelihood sweep hands its index-ordered items out in the uploaded order
 * (a permutation of 0 .. n-1: position -> particle) with the given in-phase patience; order == NULL switches it off. */
int smc_debug_set_order(smc_ctx *ctx, const int32_t *order, int64_t n, int patience);
int smc_debug_rccl_self_exchange(smc_ctx *ctx, int64_t row, int64_t cnt, int64_t dst_row);
/* Loopback rehearsal of the multi-rank path on ONE device: `peers` are the `world` contexts of one process
 * (peers[rank] == ctx), typically one host thread per rank.  smc_resample_phase3 then only packs (gathers own
 * slots, stages remote ones, synchronises its stream); after a barrier between the threads every rank calls
 * smc_resample_phase3_pull, which copies its incoming slots out of the peers' staging buffers (device-to-
 * device) instead of the RCCL send/recv pairs.  Everything else (kernels, offsets, counts) is the RCCL path. */
int smc_debug_set_local_peers(smc_ctx *ctx, smc_ctx **peers, int rank, int world);
int smc_resample_phase3_pull(smc_ctx *ctx);
/* ... and with the collectives INSIDE the engine (after smc_debug_set_local_peers on every peer, at most 8): the *_global entry
 * points, smc_resample_enqueue, smc_mh_iteration_device_rng and smc_mh_sweeps_device_rng then take their world > 1 branches with
 * every ncclAllReduce / ncclAllGather / send-recv pair replaced by its counterpart among the peer contexts (events between
 * their streams, a host barrier between their threads; sums in rank order) - the stop / no-op logic of a speculative batch and
 * the matched reductions run bit for bit as they would over RCCL.  Every peer thread must make the same calls. */
int smc_debug_peer_collectives(smc_ctx *ctx, int enable);
#endif /* SMC_ENABLE_DEBUG_API */

/* ---- measurement ------------------------------------------------------------------------------ */
/* HIP-event timing of the kernels launched on the context's stream: smc_timing_reset clears the
 * accumulators; smc_timing_get returns, for kernel class `which`, launches and total milliseconds
 * measured with hipEvents recorded on that stream around each launch (enabled by smc_timing_enable). */
#define SMC_T_LOGLIK 0
#define SMC_T_MH 1
#define SMC_T_ESS 2
#define SMC_T_RESAMPLE 3
#define SMC_T_MOMENTS 4
#define SMC_T_MAX 5
#define SMC_T_SOLVE 6 /* the persistent RK45 solve kernel alone (inside LOGLIK / MH sweeps) */
#define SMC_T_COUNT 7
int smc_timing_enable(smc_ctx *ctx, int enable);
int smc_timing_reset(smc_ctx *ctx);
int smc_timing_get(smc_ctx *ctx, int which, int64_t *launches, double *total_ms);
/* Device-counted work of the Michaelis-Menten sweeps since the last smc_timing_reset (always on; bench.py's roofline numerator):
 * out[0] (particle, experiment) solves that ran to t_bound and produced their n_t dense outputs - cancelled (exact early
 *        rejection) and masked (out of support) proposals do not count;
 * out[1] RK45 attempts of all solves, finished or cancelled;
 * out[2] launches of the solve kernel that had work;  out[3] launches of a speculative batch (smc_mh_sweeps_device_rng) that
 *        found the loop already ended and returned at once. */
int smc_work_totals(smc_ctx *ctx, int64_t out[4]);

/* ---- methanation model (configs 4-5): context-free building blocks ---------------------------------------
 * State layout as in the reference: 357 = 7 fields x 51 axial nodes, field-major X[f*51+i],
 * f in {Ca,Cb,Cc,Cd,Ce,T,u} (SMC_methanation/methanation_set_likelihood.py:85-91); params = the
 * 18-tuple p0 of my_model (:164): 10 inlet/geometry scalars then the 8 kinetic parameters.
 * Context-free calls on host buffers (they allocate and free device memory per call), parity-tested through the
 * ABI: residual, rate law and likelihood are pinned by the reference's own functions; smc_meth_dae_host (below)
 * is the DAE integration replacing my_model/IDA (:144-277), parity-unpinned (no IDA in the image). */
const char *smc_meth_last_error(void);
/* res[n][357] = reaction(t, X, dX, params) (methanation_set_likelihood.py:69-139). */
int smc_meth_residual_host(int device, const double *X, const double *dX, const double *params, int64_t n,
                           double *res);
/* out[j] = func_rCH4(T, Ca, Cb, Cc, Cd, kin) (:44-58); in is n x 5 (T,Ca,Cb,Cc,Cd), kin n x 8. */
int smc_meth_rate_host(int device, const double *in, const double *kin, int64_t n, double *out);
/* lk[j] = my_loglike(y_j, data, sigma_j, n_data) (:280-300); y is n x 5 x n_data, data 5 x n_data. */
int smc_meth_loglike_host(int device, const double *y, const double *data, const double *sigma, int64_t n, int n_data,
                          double *lk);

/* The body of my_model (:161-208) for n_solves independent (particle, experiment) pairs: integrate
 * F(t,X,X';p0) = 0 from X(0) = y0 (the driver's guess, SMC_methanation_main.py:47-58), X'(0) = 0 to tf with a
 * variable-order BDF (rtol/atol as Assimulo's IDA defaults 1e-6) and map the outlet node to the five
 * standard-state flows (:204-208).  PARITY UNPINNED against IDA (see csrc/meth_dae.h).  A failed solve
 * (status != 0) returns the reference's sentinel flows -10000 (:244-249).
 * p0_all: n_solves x 18, y0_all: n_solves x 357, flows: n_solves x 5, y_final (optional): n_solves x 357,
 * status: n_solves, stats (optional, FIVE words since ABI 3): sums of steps, rejected steps, Newton failures, Newton iterations,
 * factorisations of the iteration matrix. */
int smc_meth_dae_host(int device, const double *p0_all, const double *y0_all, int64_t n_solves, double tf, double rtol,
                      double atol, double h0, double S, double P_stp, double *flows, double *y_final, int32_t *status,
                      int64_t *stats, double *kernel_ms);

#ifdef __cplusplus
}
#endif
#endif /* SMC_HIP_H */
