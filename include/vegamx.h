/*
 * vegamx.h - C ABI of the MI355X-native Vega model + chi2 engine (libvegamx.so).
 *
 * The engine replaces, for batches of parameter points, the per-evaluation hot path of
 * andreicuceu/vega that sits behind
 *     VegaInterface.compute_model / chi2 / log_lik   (reference vega/vega_interface.py:208-387)
 *     Model.compute                                   (reference vega/model.py:157-187)
 * i.e. PowerSpectrum.compute (vega/power_spectrum.py:87-196), PktoXi.compute
 * (vega/pktoxi.py:99-163), CorrelationFunction.compute (vega/correlation_func.py:117-198),
 * Metals.compute (vega/metals.py:258-367), BroadbandPolynomials.compute
 * (vega/broadband_poly.py:74-198), the distortion-matrix product (vega/model.py:143-144)
 * and the Gaussian chi2 (vega/vega_interface.py:295-319).
 *
 * Beside evaluations the handle runs whole loops that consist of them where their state lives: fits (vmx_fit_migrad),
 * an ensemble MCMC sampler (vmx_ensemble_run), a nested sampler (vmx_nested_run, vmx_nested_run_phantoms, vmx_nested_run_many, vmx_nested_run_many_phantoms) and a tempered SMC sampler (vmx_smc_run, vmx_smc_run_many, vmx_smc_run_kept, vmx_smc_run_many_kept), both
 * with the evidence, the counterparts of
 * the reference's iminuit / PolyChord callers (vega/minimizer.py, vega/samplers/polychord.py, bin/run_vega_mpi.py).
 *
 * The reference is pure Python and has no FFI of its own; the binding a maintainer adds is the
 * ctypes layer shown in INTEGRATION.md (vega_amd/engine.py is that binding).
 *
 * Conventions
 *   - plain C types only; all host buffers are owned by the caller; the engine owns device memory;
 *   - every function returns 0 on success, a negative code on failure, and vmx_last_error()
 *     then describes the failure (thread-local string);
 *   - parameter points are rows of `theta` (row-major [B][n_params], fp64); a descriptor refers
 *     to a parameter by its column ("slot"); slot -1 means "absent" (Python None);
 *   - per-walker numerical failures (spline argument out of range = the reference's
 *     VegaBoundsError, NaN/Inf in the Arinyo term = VegaArinyoError) never fail the call: they
 *     set status[b] != 0 and chi2[b] = 1e100, the reference's sentinel
 *     (vega/vega_interface.py:268-279);
 *   - one engine handle = one HIP device + one stream; calls on a handle must be serialised by
 *     the caller; distinct handles are independent.  No global mutable state.
 */
#ifndef VEGAMX_H
#define VEGAMX_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct vmx_engine vmx_engine;

#define VMX_MAX_ELL 4          /* ell = 0, 2, 4, 6 (reference pktoxi.py:39,45) */
#define VMX_MAX_SMOOTH 3       /* Gaussian-type smoothing terms per pipeline */

enum { VMX_HCD_NONE = 0, VMX_HCD_ROGERS = 1, VMX_HCD_SINC = 2, VMX_HCD_FVOIGT = 3 };
enum { VMX_NL_NONE = 0, VMX_NL_ARINYO = 1, VMX_NL_MCDONALD = 2 };
enum { VMX_VD_NONE = 0, VMX_VD_GAUSS = 1, VMX_VD_LORENTZ = 2 };
enum { VMX_SCALE_UNIT = 0, VMX_SCALE_AP_AT = 1, VMX_SCALE_AISO_EPS = 2, VMX_SCALE_PHI_ALPHA = 3 };
enum { VMX_PKLIN_PEAK = 0, VMX_PKLIN_SMOOTH = 1, VMX_PKLIN_FULL = 2 };
enum { VMX_EVOL_STD = 0, VMX_EVOL_CROOM = 1 };
enum { VMX_MAT_DISTORTION = 0, VMX_MAT_INVCOV = 1, VMX_MAT_METAL = 2 };
enum { VMX_BB_PRE_MUL = 0, VMX_BB_PRE_ADD = 1, VMX_BB_POST_MUL = 2, VMX_BB_POST_ADD = 3 };
enum { VMX_BB_POLY = 0, VMX_BB_SKY = 1 };

/* status bits written per walker */
enum { VMX_STATUS_OK = 0, VMX_STATUS_BOUNDS = 1, VMX_STATUS_ARINYO = 2, VMX_STATUS_NONFINITE = 4,
       VMX_STATUS_NOT_CONSTANT = 8 };

/* A tracer's (bias, beta): two of the three slots must be present
 * (reference vega/utils.py:45-82 _tracer_bias_beta). */
typedef struct {
    int32_t bias_slot;
    int32_t bias_eta_slot;
    int32_t beta_slot;
    int32_t is_lya;        /* name == 'LYA': receives the UV / HCD effective bias */
    int32_t discrete;      /* tracer type 'discrete': receives the velocity-dispersion term */
    int32_t vd_sigma_slot; /* sigma_velo_disp_{gauss,lorentz}_<name>, -1 if not discrete */
    int32_t evol_kind;     /* VMX_EVOL_* (reference correlation_func.py:301-370) */
    int32_t alpha_slot;    /* alpha_<name> */
} vmx_tracer;

/* One P(k,mu) -> xi(r,mu) chain (a core peak / smooth component or one metal pair). */
typedef struct {
    vmx_tracer tracer[2];
    int32_t same_tracer;            /* tracer2 is tracer1 (utils.py:103-104) */
    int32_t growth_rate_slot;       /* 'growth_rate', -1 -> growth_rate_default */
    double  growth_rate_default;    /* 0.970386 (utils.py:60) or a fixed override */
    int32_t fast_metals;            /* Kaiser term without b1*b2 (power_spectrum.py:220-221) */
    int32_t pk_lin_kind;            /* VMX_PKLIN_* (model.py:177,182,184) */
    int32_t is_peak;                /* params['peak'] */

    int32_t uvb, heii;              /* power_spectrum.py:224-261 */
    int32_t bias_gamma_slot, bias_prim_slot, lambda_uv_slot, bias_gamma_e_slot, lambda_heii_slot;

    int32_t hcd_model;              /* VMX_HCD_*  (power_spectrum.py:263-358) */
    int32_t bias_hcd_slot, beta_hcd_slot, l0_hcd_slot;
    double  l0_default;             /* L0_sinc default 1 (power_spectrum.py:299) */

    int32_t nl_model;               /* VMX_NL_* after the skip-nl-model-in-peak rule */
    int32_t arinyo_slot[6];         /* q1, q2, kv, av, bv, kp  (q2 may be -1 -> 0) */
    double  arinyo_power;           /* 1 two Lya tracers, 0.5 one, 0 none (:472-477) */

    int32_t gk_table;               /* id from vmx_add_gk_table, -1: no G(k) */
    int32_t mock_los_slot;          /* -1, or the parameter p a mock's line-of-sight bin follows when p is sampled
                                     * (`mock-los-smoothing = growth | amplitude`, power_spectrum.py:143-160): one more
                                     * factor sinc(k_par mock_los_size (1 + theta[p]) / 2) per walker in the mu loop; the
                                     * static G table then holds the other binning factors only */
    double  mock_los_size;          /* the mock's bin size (`mock-bin-size`) */

    int32_t peak_nl;                /* apply compute_peak_nl (power_spectrum.py:382-417) */
    int32_t sigma_nl_par_slot, sigma_nl_per_slot;

    /* Gaussian smoothing terms: factor exp(-w (k_par^2 s_par^2 + k_perp^2 s_perp^2)) each
     * (power_spectrum.py:504-553, utils.py:396-420) */
    int32_t n_smooth;
    int32_t smooth_par_slot[VMX_MAX_SMOOTH], smooth_per_slot[VMX_MAX_SMOOTH];
    double  smooth_weight[VMX_MAX_SMOOTH];
    int32_t exp_par_slot, exp_per_slot;   /* exp smoothing (power_spectrum.py:560-586), -1 none */

    int32_t vd_kind;                /* VMX_VD_* (power_spectrum.py:588-636) */
    double  damping_scale;          /* <= 0: none (power_spectrum.py:192-194) */
    int32_t damping_power;

    int32_t n_ell;                  /* multipoles 0, 2, .. 2 (n_ell - 1) */
    int32_t scale_mode;             /* VMX_SCALE_* (scale_parameters.py:38-230) */
    int32_t scale_slot[2];
    int32_t drp_slot;               /* drp_<discrete tracer>, -1 none (correlation_func.py:65-69) */
    int32_t croom_slot[2];          /* croom_par0, croom_par1 */
    int32_t radiation;              /* QSO radiation term (correlation_func.py:446-489); 2: on the rescaled coordinates
                                     * (`rescale-coords-systematics`, :470-472) */
    int32_t rad_slot[4];            /* strength, asymmetry, lifetime, decrease */
    int32_t uv_shotnoise;           /* UV-background shot noise (correlation_func.py:649-686); 2: with the reference's
                                     * `rescale-coords-systematics` separation (:681-682) */
    int32_t uvsn_slot[3];           /* uv_shotnoise_amp, lambda_uv, bias_gamma (or bias_gamma_e) */
    int32_t single_ell;             /* -1, or ell / 2: return that multipole xi_ell(r') alone (pktoxi.py:122-155) */
    double  z_eff;
} vmx_pipe_desc;

/* One metal pair's contribution: bias1*bias2*factor * M . xi_pair (metals.py:286-334). */
typedef struct {
    int32_t pipeline;               /* id from vmx_add_pipeline */
    vmx_tracer tracer[2];           /* bias slots as seen by Metals.compute (after single-metal-beta) */
    int32_t same_tracer;
    int32_t growth_rate_slot;
    double  growth_rate_default;
    int32_t extra_bias_slot;        /* bias_<m1>_<m2> (separate-metal-auto-biases), -1 none */
    int32_t apply_bias;             /* fast_metal_bias: multiply by the bias product afterwards */
    double  multiplicity;           /* 2 for distinct metals in an auto-correlation (:238-239) */
    int32_t amplitude_slot;         /* -1, or a parameter multiplying the contribution: with `no-metal-decomp = False`
                                     * (model.py:120-123, :186) a pair enters twice, its smooth-spectrum pipeline as is
                                     * and its peak-spectrum pipeline times bao_amp */
    int32_t in_direct;              /* 1: the pair is part of a direct_pk evaluation (model.py:188-207 calls _compute_model with
                                     * the caller's spectrum: with `no-metal-decomp = False` the metal terms are computed on it,
                                     * :120-123 - the smooth-spectrum entries; with the default decomposition they are left out) */
} vmx_metal_desc;

typedef struct {
    int32_t n_model;                /* undistorted model bins */
    int32_t n_dist;                 /* distorted model bins (= output size) */
    int32_t pipe_peak, pipe_smooth; /* pipeline ids */
    int32_t bao_amp_slot;
} vmx_item_desc;

const char* vmx_last_error(void);
/* sizeof() of the structs as compiled (0 tracer, 1 pipe, 2 metal, 3 item, 4 vmx_fit_spec, 5 vmx_fit_options, 6 vmx_fit_result,
 * 7 vmx_fit_stats, 8 vmx_ensemble_spec, 9 vmx_ensemble_options, 10 vmx_ensemble_stats, 11 vmx_nested_spec, 12 vmx_nested_options,
 * 13 vmx_nested_stats, 14 vmx_smc_spec, 15 vmx_smc_options, 16 vmx_smc_stats, 17 vmx_nested_clusters,
 * 18 vmx_nested_set_options, 19 vmx_nested_phantoms, 20 vmx_nested_set_phantoms, 21 vmx_smc_keep,
 * 23 vmx_ensemble_moves, 24 vmx_ensemble_adapt, 25 vmx_ensemble_slice, 27 vmx_ensemble_cov; 22 and 26 are vacant and answer -1, as every index
 * that names no struct): lets a foreign
 * binding verify its struct layout at load time. */
int vmx_struct_size(int32_t which);

int vmx_create(vmx_engine** out, int device);
void vmx_destroy(vmx_engine* e);

/* Template grids (vega_interface.py:690-696; power_spectrum.py:72-81; pktoxi.py:37,55).
 * pk_peak = pk_full - pk_smooth as formed by the caller (model.py:177);
 * delta2 = k^3 pk_fid / (2 pi^2) (power_spectrum.py:462).  n_mu = num_bins_muk (power_spectrum.py:52-58; default 1000): at
 * most 2048 - the mu tables of the P(k,mu) kernels live in LDS. */
int vmx_set_template(vmx_engine* e, int32_t nk, const double* k, const double* pk_peak,
                     const double* pk_smooth, const double* pk_full, const double* delta2,
                     int32_t n_mu);

/* The linear operator P_ell(k) -> cubic-spline coefficients of xi_ell on the uniform ln r knot
 * grid x0 + h*i: FFTLog (mcfit.P2xi call of pktoxi.py:141) followed by the not-a-knot spline of
 * pktoxi.py:144.  op is row-major [n_coef][nk]; n_coef = n_knots + 2. */
int vmx_set_fftlog(vmx_engine* e, int32_t ell_index, const double* op, int32_t n_coef,
                   double x0, double h, int32_t n_knots);
/* Evaluate the xi splines outside their knot range by polynomial extension instead of flagging the walker
 * (the reference's legacy old_fftlog path uses splev, which extrapolates; pktoxi.py:276-277). */
/* `fht_extrap = True` (reference vega/pktoxi.py:41,141: mcfit.P2xi(...)(pk_ell, extrap=True)): the FFTLog's input is padded
 * with power laws through its end segments instead of zeros - n_left samples F[0] (F[1] / F[0])^-t and n_right samples
 * F[n-1] (F[n-1] / F[n-2])^t, t = 1, 2, ...  Call BEFORE vmx_set_template; the operators of vmx_set_fftlog then have
 * nk + n_left + n_right columns, [samples | left pads t = 1.. | right pads t = 1..] (vega_amd/fftlog_op.xi_operator(extrap=True)),
 * and the engine forms the pad samples per walker, multipole and pipeline on the device.  0 / 0 end segments (a spectrum
 * smoothed to exact zeros at the template's last wavenumbers) give NaN there as in the reference: VMX_STATUS_NONFINITE. */
int vmx_set_fftlog_padding(vmx_engine* e, int32_t n_left, int32_t n_right);
int vmx_set_spline_extrapolation(vmx_engine* e, int32_t enabled);

/* Voigt-profile table of model-hcd = fvoigt: F(L0 k_par) by linear interpolation in (x, f), 1 below the table and
 * 0 above it (np.interp(..., left=1, right=0), power_spectrum.py:360-380).  x must be increasing. */
int vmx_set_fvoigt_table(vmx_engine* e, const double* x, const double* f, int32_t n);

/* G(k) binning table for one (bin_size_rp, bin_size_rt) pair (power_spectrum.py:481-502).
 * Returns the table id (>= 0). */
int vmx_add_gk_table(vmx_engine* e, double bin_size_rp, double bin_size_rt);
/* The same with the mock-binning factor of power_spectrum.py:143-160 folded in: G(bin sizes) * G(mock sizes);
 * a size of 0 leaves its sinc out (`mock-los-smoothing = only-los` -> mock_size_rt = 0). */
int vmx_add_gk_table_mock(vmx_engine* e, double bin_size_rp, double bin_size_rt, double mock_size_rp,
                      double mock_size_rt);

/* Returns the pipeline id (>= 0).  r, mu, z, rel_z_evol, xi_growth: [n] (correlation_func.py:46-80,252). */
int vmx_add_pipeline(vmx_engine* e, const vmx_pipe_desc* desc, int32_t n, const double* r,
                     const double* mu, const double* z, const double* rel_z_evol,
                     const double* xi_growth);

/* `new-bias-evolution` (correlation_func.py:238-299): in a cross-correlation the two tracers evolve with their own
 * redshifts z -/+ rp / (2 D_H(z)).  rel_z_1 / rel_z_2 [n] = (1 + z_tracer) / (1 + z_eff) per bin for the pipeline's
 * first / second tracer as given to vmx_add_pipeline; replaces the common rel_z_evol of that call. */
int vmx_pipeline_set_tracer_evolution(vmx_engine* e, int32_t pipeline, const double* rel_z_1,
                                      const double* rel_z_2, int32_t n);

/* Odd-multipole terms of a cross-correlation component (correlation_func.py:150-155, pktoxi.py:321-382):
 * coef [4][n_coef] = cubic B-spline coefficients (knots x0 + h i in ln r) of the Hamilton-FFTLog transforms of the
 * component's isotropic linear spectrum, in the order rel ell=1, rel ell=3, asy ell=0, asy ell=2;
 * slots = {Arel1, Arel3, Aasy0, Aasy2, Aasy3}. */
int vmx_pipeline_set_odd_terms(vmx_engine* e, int32_t pipeline, const double* coef, int32_t n_coef, double x0,
                               double h, int32_t relativistic, int32_t asymmetry, const int32_t* slots);

/* The same splines as a linear operator of the component's spectrum, for `direct_pk` (reference vega/model.py:188-207: the
 * caller's spectrum is then the pk_lin of the odd-multipole terms too, correlation_func.py:491-551): op[4][n_coef][nk], term
 * order as `coef` above, coef_term = op_term . pk (vega_amd/fftlog_op.hamilton_spline_operator).  vmx_set_direct_pk forms the
 * walkers' coefficient rows with it (one product per pipeline); without it a pipeline with odd terms refuses direct_pk. */
int vmx_pipeline_set_odd_operator(vmx_engine* e, int32_t pipeline, const double* op, int32_t n_coef, int32_t nk);

/* A(tau) table of the UV shot-noise term on the uniform grid tau0 + dtau i (correlation_func.py:597-647):
 * np.interp with left = a[0], right = 0. */
int vmx_set_shotnoise_table(vmx_engine* e, const double* a, int32_t n, double tau0, double dtau);

/* Returns the item id (>= 0). */
int vmx_add_item(vmx_engine* e, const vmx_item_desc* desc);
int vmx_item_add_metal(vmx_engine* e, int32_t item, const vmx_metal_desc* desc);
/* `fast_metals` (metals.py:144-169): a metal x metal correlation frozen at the first evaluation.  The metal is
 * added with desc.pipeline = -1 and contributes bias_product * xi[bin] with this static vector (already
 * multiplied by its metal matrix and multiplicity-free: desc.multiplicity still applies). */
int vmx_item_set_metal_static(vmx_engine* e, int32_t item, int32_t index, const double* xi, int32_t n_model);
/* Exact static form of a metal pair whose P(k,mu) is the bias-free Kaiser polynomial times static factors only
 * (power_spectrum.py:198-222 with fast_metals; no HCD / UV / non-linear / smoothing / velocity-dispersion term, fixed
 * coordinates): xi = Y0 + (beta1 + beta2) Y1 + beta1 beta2 Y2 with three static vectors (after the pair's metal matrix,
 * redshift evolution and growth).  basis = [3][n_model]; the metal is added with desc.pipeline = -1, its tracers
 * provide beta1, beta2 and the bias product per walker. */
int vmx_item_set_metal_basis(vmx_engine* e, int32_t item, int32_t index, const double* basis, int32_t n_model);
/* Set-up hook used to extract those vectors with the engine itself: while enabled, every tracer of a bias-free
 * (fast_metals) pipeline takes beta = `beta` instead of its parameters. */
int vmx_set_metal_beta_override(vmx_engine* e, int32_t enabled, double beta);

/* Parameter-level blinding (vega_interface.py:389-421 `_get_lcl_prms`, utils.py:375-393 `apply_blinding`): every
 * walker is mapped theta[p] -> scale[p] * theta[p] + shift[p] before anything reads it (model and priors alike).
 * The reference's blinding is shift = pi - exp(v^2) on the blinded names and (scale, shift) = (0, 1) on the
 * full-shape scale parameters it pins to 1.  scale, shift: [n_params] host arrays, or NULL, NULL to switch it off.
 * While a transform is set the device entry point stages the walkers through the engine's own buffer. */
int vmx_set_parameter_transform(vmx_engine* e, const double* scale, const double* shift);

/* Additive template of the non-peak component: v += amp * vec[bin] before the pre-distortion broadband
 * (DESI instrumental systematics, model.py:133-135, correlation_func.py:553-595).  amp = theta[slot], or
 * default_amp when slot = -1. */
int vmx_item_set_additive_template(vmx_engine* e, int32_t item, const double* vec, int32_t n_model,
                                   int32_t slot, double default_amp);

/* Broadband term (broadband_poly.py:119-198).
 *  VMX_BB_POLY: slots[n_coef] coefficient slots, basis [n_coef][n] = r1^i r2^j per coefficient;
 *  VMX_BB_SKY:  slots = {scale, sigma}, basis [2][n] = {rt, window(0/1)}.
 * n = n_model for pre terms, n_dist for post terms. */
int vmx_item_add_broadband(vmx_engine* e, int32_t item, int32_t position, int32_t func,
                           int32_t n_coef, const int32_t* slots, const double* basis, int32_t n);

/* Dense row-major matrices.  VMX_MAT_DISTORTION [n_dist][n_model] (model.py:143-144);
 * VMX_MAT_INVCOV [n_masked][n_masked] (vega_interface.py:316); VMX_MAT_METAL [n_model][n_pair]
 * with `index` = position of the metal in the order of vmx_item_add_metal (metals.py:338-367).
 * A matrix that is never set is the identity (data.py:77-78, :683-684). */
/* A metal matrix in Kronecker form, M = A (x) B on the bin order rt-fastest (index = rt + n_rt * rp): what
 * `new_metals` builds (metals.py:501-655: np.einsum('ij,kl->ikjl', rp_1d_dmat, rt_1d_dmat)), and with b_rt = NULL
 * (B = identity) the rp-only form (metals.py:354-358, :657-752).  The product M xi = A Xi B^T is applied as two small
 * products per walker instead of one [n_model]^2 product.  a_rp [n_rp][n_rp], b_rt [n_rt][n_rt], row-major;
 * n_rp * n_rt = n_model of the item = bins of the pair's pipeline. */
int vmx_item_set_metal_kron(vmx_engine* e, int32_t item, int32_t index, const double* a_rp, int32_t n_rp,
                            const double* b_rt, int32_t n_rt);
int vmx_item_set_matrix(vmx_engine* e, int32_t item, int32_t kind, int32_t index, int32_t rows,
                        int32_t cols, const double* dense);
/* The distortion matrix in CSR form, as the reference holds it (scipy.sparse.csr_array: data.py:342-346, :456-459; the
 * product of model.py:143-144): indptr [rows + 1] (int64), indices [nnz] (int32, STRICTLY ascending within a row: no duplicates - checked), values [nnz].
 * Replaces vmx_item_set_matrix(VMX_MAT_DISTORTION) for matrices sparse enough that streaming 12 bytes per non-zero beats
 * 8 bytes per entry; every batch size takes the CSR kernel then (8 walkers per pass over the matrix).  Before
 * vmx_finalize. */
int vmx_item_set_matrix_csr(vmx_engine* e, int32_t item, int32_t rows, int32_t cols, const int64_t* indptr,
                            const int32_t* indices, const double* values);
/* Indices (into the n_dist model bins) kept by the model mask (data.py:410). */
int vmx_item_set_mask(vmx_engine* e, int32_t item, const int32_t* idx, int32_t n_masked);
/* Masked data vector, or the current Monte-Carlo mock (vega_interface.py:311-315). */
int vmx_item_set_data(vmx_engine* e, int32_t item, const double* masked_data, int32_t n_masked);

/* Monte-Carlo fits of many mocks at once (vega/analysis.py:224-302 evaluates one mock at a time): a pool of
 * masked mock data vectors [n_mocks][n_masked] per item, and per walker the pool row it is compared with
 * (vmx_set_mock_index; -1 or a NULL index array = the item's own data vector).  Both may be called after
 * vmx_finalize; the index array applies to the following vmx_eval* calls. */
int vmx_item_set_mock_pool(vmx_engine* e, int32_t item, const double* pool, int32_t n_mocks, int32_t n_masked);
int vmx_set_mock_index(vmx_engine* e, const int32_t* index, int32_t B);
/* Mocks made on the device: the lower Cholesky factor L [n_masked][n_masked] of the (scaled) masked covariance and the fiducial
 * model on the masked bins - a mock is fiducial + L . (standard-normal draws), reference vega/data.py:737-753.  Kept until replaced;
 * used by vmx_fit_migrad with a mock stream.  vmx_item_get_mock_pool copies the first n_mocks rows of an item's pool to the host
 * (the MOCKS table of the result file, reference vega/output.py:442-520). */
int vmx_item_set_mock_factor(vmx_engine* e, int32_t item, const double* chol, const double* fiducial, int32_t n_masked);
int vmx_item_get_mock_pool(vmx_engine* e, int32_t item, double* pool, int32_t n_mocks, int32_t n_masked);
/* Page-locked host memory for buffers the library reads asynchronously - the `draws` of a vmx_mock_stream above all: from
 * pageable memory every wave's upload is staged (and, behind some runtimes, pinned page by page while the producer is still
 * first-touching the buffer: 20 ms of a 290-ms run).  Owned by the engine: vmx_host_free, or vmx_destroy at the latest. */
int vmx_host_alloc(vmx_engine* e, void** out, int64_t bytes);
int vmx_host_free(vmx_engine* e, void* p);

/* Global-covariance mode (vega_interface.py:295-304): inverse of the masked global covariance over
 * the concatenation of all items' masked bins, in item order. */
int vmx_set_global_invcov(vmx_engine* e, const double* invcov, int32_t n);

int vmx_add_prior(vmx_engine* e, int32_t slot, double mean, double sigma);

/* Allocate the per-batch workspace.  After this the engine is immutable except for
 * vmx_item_set_data / vmx_item_set_matrix(INVCOV) / vmx_set_global_invcov. */
int vmx_finalize(vmx_engine* e, int32_t n_params, int32_t max_batch);
/* Before vmx_finalize.  enabled = 0: pipelines whose P(k,mu) is the Kaiser polynomial times static factors keep their per-walker
 * P(k) -> xi path instead of the static spline-coefficient basis derived from the template's spectra (default 1: the basis).
 * Needed for direct_pk evaluations that include such pipelines (vmx_metal_desc::in_direct): a caller-supplied spectrum has no
 * static basis; vmx_set_direct_pk refuses them otherwise. */
int vmx_set_static_poly(vmx_engine* e, int32_t enabled);

/* Total output size per walker: sum of n_dist over items, in item order. */
int vmx_model_size(vmx_engine* e);
/* Column of a pipeline in the P_ell(k) / spline-coefficient stage buffers (vmx_debug_read 0 and 2, laid out
 * [ell][walker * n_columns + column][k]); pipelines whose multipoles are never formed per walker (Kaiser polynomial
 * times static factors: they carry a static coefficient basis) have none: the value is then -3 - n_columns. */
int vmx_pipeline_column(vmx_engine* e, int32_t pipeline);

/* Precondition of the QSO radiation term (vmx_pipe_desc::radiation): no bin of such a pipeline may have r_perp = 0.  The term
 * divides by r_shift^2 = (r_par' + delta_rp)^2 + r_perp'^2 through a reciprocal square root without a guard; with r_perp = 0 a
 * walker's delta_rp can cancel a bin centre, and that bin's model is then NaN (VMX_STATUS_NONFINITE for the walker).  Grids of
 * bin centres have r_perp > 0 everywhere. */
/* Evaluate B parameter points.  theta [B][n_params] host memory.
 * chi2 [B] (may be NULL), model [B][vmx_model_size] (may be NULL), status [B] (may be NULL).
 * Synchronous: outputs are valid on return. */
int vmx_eval(vmx_engine* e, const double* theta, int32_t B, double* chi2, double* model,
             int32_t* status);

/* Same with theta / chi2 already in device memory (no host copies, no synchronisation: the work
 * is enqueued on the engine stream; use vmx_sync).  d_model may be NULL. */
int vmx_eval_device(vmx_engine* e, const double* d_theta, int32_t B, double* d_chi2,
                    double* d_model, int32_t* d_status);
int vmx_sync(vmx_engine* e);
/* vmx_eval_device for walkers that bring their own Monte-Carlo mock rows: d_mock_index [B] (device memory) holds, per walker, the
 * row of the items' mock pools it is compared with (-1: the item's data vector) - what vmx_set_mock_index states from the host
 * for the calls that follow, stated per call from HBM here, so that two batches with different rows can be in flight (lanes).
 * chi2 only; always eager launches (no captured graph: the batch size is expected to change from call to call).  The rows must
 * lie inside the pools (the caller wrote them; the fit driver below checks its own on the host). */
int vmx_eval_device_mocks(vmx_engine* e, const double* d_theta, int32_t B, double* d_chi2, int32_t* d_status,
                          const int32_t* d_mock_index);

/* Fits where the walkers live.  The reference minimises chi2 one MIGRAD after the other - vega/minimizer.py:66-97 per fit
 * (iminuit.Minuit(chi2, ...).migrad(ncall): a bias-only pre-fit, then the full fit from its result), vega/analysis.py:224-308 per
 * Monte-Carlo mock, bin/run_vega_mc_mpi.py:52-71 per rank.  vmx_fit_migrad runs n_fits such fits together ON THE DEVICE: every
 * fit is a resumable MIGRAD state machine (vega_amd/csrc/vmx_migrad.h - Minuit2 strategy 1 restated decision for decision:
 * internal coordinates, seed, two-point gradient, line search, Davidon update, HESSE, iminuit's `iterate` re-runs - tested on the
 * CPU under sanitizers against the per-fit reference coroutine of vega_amd/migrad.py) advanced by one thread; a round = one
 * kernel that consumes the chi2 values of every fit's last request and runs its bookkeeping up to the next one, a scan, one
 * kernel that writes the requested points as parameter rows (Minuit's transforms in the kernel), and the engine's chain over
 * those rows in chunks on alternating lanes.  Parameter rows, chi2 values and the fits' states never leave HBM; the host reads
 * ONE integer per round (the number of rows) and the results at the end.  A fit's sequence of function values is Minuit's own;
 * the fits advance at their own pace (a fit that converges goes on to HESSE / its next object while others iterate).
 *
 *   spec      the Minuit objects of a fit (1 or 2 stages; stage 1 starts from stage 0's result): free parameter columns, limits,
 *             step sizes; errordef `up`, tolerance, call limit, iminuit's `iterate` (reference: 1.0, 0.1, 100000, 5)
 *   theta0    [n_fits][n_params] host: start values and the values of the columns held fixed, per fit
 *   mock_row  [n_fits] host or NULL: the pool row (vmx_item_set_mock_pool) fit f is fitted to; NULL: the items' data
 *   opt       const_hint = vmx_set_constant_nl_hint's level for the rows of a round, or -1: derived here (a column varies when a
 *             stage frees it or the fits' rows differ in it - what vmx_eval derives from host walkers); NULL: -1, 512, 2;
 *             chunk = rows per engine call (0: 512); lanes = batches in flight (0: 2); mocks: see vmx_mock_stream - NULL: the
 *             pools hold the mocks already
 *   results   [n_stages] host arrays the caller owns: x [n_fits][n] internal minimum, ext [n_fits][n] its external values,
 *             V [n_fits][n][n] internal error matrix, fval, edm, flags (VMX_FIT_* bits), nfcn (function calls of the stage, re-runs
 *             included), n_iter
 * Synchronous; calls on a handle stay serialised by the caller.  Every argument is checked before anything runs (-1 and
 * vmx_last_error, the engine untouched).  A run that fails later (-2: a HIP error, a stalled producer of a mock stream) leaves the
 * engine usable with its hint / lanes restored; `results` and, with a mock stream, the items' mock pools then hold unspecified rows. */
#define VMX_FIT_MAXN 32
#define VMX_FIT_MAX_STAGES 2
enum { VMX_FIT_VALID = 1, VMX_FIT_HESSE_FAILED = 2, VMX_FIT_ACCURATE = 4, VMX_FIT_AT_CALL_LIMIT = 8, VMX_FIT_MADE_POSDEF = 16 };
typedef struct {
    int32_t n;
    int32_t col[VMX_FIT_MAXN];
    int32_t has_lo[VMX_FIT_MAXN], has_hi[VMX_FIT_MAXN];
    double lo[VMX_FIT_MAXN], hi[VMX_FIT_MAXN];
    double err[VMX_FIT_MAXN];
} vmx_fit_stage;
typedef struct {
    int32_t n_stages, n_params, iterate, maxfcn;
    double up, tol;
    vmx_fit_stage stage[VMX_FIT_MAX_STAGES];
} vmx_fit_spec;
/* Mocks made while their fits run (vmx_fit_migrad): the normal draws arrive from a producer on the host - the reference draws them
 * from NumPy's legacy global generator, mock after mock, a mock's correlations in turn (vega/data.py:748-757), and that stream is
 * sequential by construction - while everything else of a mock happens on the device, wave by wave: mock = fiducial + L . draws
 * with the chain's product kernels (L, fiducial: vmx_item_set_mock_factor), its row of every item's pool, its rows of the
 * quadratic form's linear terms.  Wave w (mocks [w wave, (w + 1) wave)) joins the fits at round w - a fixed schedule: what a round
 * evaluates never depends on how fast the draws arrive; the host waits for the producer when it is behind. */
typedef struct {
    int32_t n_mocks;                    /* = n_fits: fit f is fitted to mock f */
    int32_t wave;                       /* mocks per wave (0: 64) */
    const double* draws;                /* host [n_mocks][stride]: a mock's standard-normal draws, its items' side by side in item order */
    int64_t stride;
    const volatile int32_t* n_drawn;    /* host: mocks whose draws are complete (the producer counts up, release order) */
    double timeout_seconds;             /* give up when the producer stalls (0: 600) */
} vmx_mock_stream;
typedef struct { int32_t const_hint, chunk, lanes, reserved; const vmx_mock_stream* mocks; } vmx_fit_options;
typedef struct {
    double* x; double* ext; double* V; double* fval; double* edm;
    int32_t* flags; int64_t* nfcn; int32_t* n_iter;
} vmx_fit_result;
typedef struct {
    int64_t rounds, evaluations, engine_calls, fits_unfinished;
    int64_t calls_by_batch[8];          /* engine calls with 1, 2-4, 5-16, 17-64, 65-256, 257-1024, 1025-4096, more rows */
    int64_t evaluations_by_batch[8];
    double seconds, seconds_setup, seconds_rounds;
    double seconds_host_waiting;        /* of seconds_rounds: the host blocked on the stream (the GPU working) */
    double gpu_idle_seconds_between_rounds;     /* HIP events around the host's turn of every round: the stream empty */
    double seconds_waiting_for_draws;   /* mock stream: the host waiting for the producer at a wave's round */
    double seconds_enqueuing_waves;     /* mock stream: host time of the waves' copies and launches */
    double seconds_enqueuing_rounds;    /* host time of the rounds' own launches (advance, scan, emit) */
    double seconds_enqueuing_calls;     /* host time of the engine calls' launches */
} vmx_fit_stats;
int vmx_fit_migrad(vmx_engine* e, const vmx_fit_spec* spec, int32_t n_fits, const double* theta0, const int32_t* mock_row,
                   const vmx_fit_options* opt, vmx_fit_result* results, vmx_fit_stats* stats);
/* Posterior sampling where the walkers live: the affine-invariant ensemble sampler (Goodman & Weare 2010, emcee's stretch move
 * with randomize_split = False), every decision pinned in vega_amd/csrc/vmx_ensemble.h.  The reference samples through
 * PolyChord / pocoMC (bin/run_vega_mpi.py), which call log_lik one point at a time; here a half-step is one small kernel that
 * decides the half just evaluated, records chain rows when due and proposes the next half, then the engine's chain over the W/2
 * proposal rows in chunks of `chunk` (two lanes alternate when the quadratic form serves them).  The host enqueues the whole
 * segment and synchronises once, at the end.
 *   spec      n_params = the engine's; n sampled columns col[n] with their box [lo, hi] (finite, lo < hi); the stretch scale a > 1;
 *             log_norm (lnL = log_norm - 0.5 chi2, chi2 with the Gaussian priors); seed / stream (the Philox key; stream 0 for
 *             now, reserved for a rank); theta_fixed[n_params], the row that supplies the columns not sampled
 *   W         walkers, even and >= 2 n
 *   x, lnL, accepted   [W][n], [W], [W] host: the walkers' state, read at entry and written back at exit
 *   step0     global index of the first step (the random stream and the chain's thinning count from the start of the run: a run
 *             cut into calls gives the same chain)
 *   thin      a chain row after every step s with (s + 1) % thin == 0: chain [rows][W][n], chain_lnL [rows][W] (host, NULL: not
 *             kept), rows = (step0 + n_steps) / thin - step0 / thin
 *   opt       const_hint (-1: derived - a column varies when it is sampled), chunk (rows per engine call, 0: max_batch), lanes
 *             (0: 2); NULL: -1, 0, 0
 * Refused before anything runs (-1, vmx_last_error, the engine untouched): W odd or < 2 n, a column out of range or repeated, a
 * non-finite limit or lo >= hi, a <= 1, thin < 1, a start walker outside the box or with a non-finite lnL.  A HIP failure later
 * returns -2 and leaves the engine usable. */
#define VMX_ENS_MAXN 64
typedef struct {
    int32_t n_params, n;
    const int32_t* col; const double* lo; const double* hi;
    double a, log_norm;
    uint64_t seed, stream;
    const double* theta_fixed;
} vmx_ensemble_spec;
typedef struct { int32_t const_hint, chunk, lanes, reserved; } vmx_ensemble_options;
typedef struct {
    int64_t steps, proposals, accepted, rejected_outside_box, rejected_failed_model, engine_calls;
    double seconds, seconds_enqueuing;
    int64_t host_synchronisations;
    int32_t const_hint, lanes;          /* what the call ran with */
} vmx_ensemble_stats;
int vmx_ensemble_run(vmx_engine* e, const vmx_ensemble_spec* spec, int32_t W, double* x, double* lnL, int64_t* accepted,
                     int64_t step0, int32_t n_steps, int32_t thin, double* chain, double* chain_lnL,
                     const vmx_ensemble_options* opt, vmx_ensemble_stats* stats);
/* E independent ensembles advanced together: a posterior for every Monte-Carlo mock, or the replicas of one run, as one device run.
 * A run of W = 32 - 64 walkers hands the engine batches of 16 - 32 rows, far below what it is fast at; here the half-steps of all
 * ensembles are decided by one kernel of E work-groups (k_ens_half: work-group e owns ensemble e, nothing crosses ensembles; the
 * single run is this routine with E = 1) and their E W/2 proposal rows go through the engine as one stream of chunks
 * of `chunk` on two lanes.  Ensemble e is by construction the chain the single run makes with spec->stream = streams[e] on the
 * same data; its chi2 is evaluated in batches of another shape, so that its lnL may differ from the single run's in the last bits
 * (E = 1 has the single run's batches and gives its chain bit for bit).
 *   spec      as for the single run; spec->stream is not read
 *   E, W      ensembles (>= 1) of W walkers each, W even and >= 2 n
 *   streams   [E] the Philox stream of every ensemble (repeats allowed: equal streams on equal data give equal chains)
 *   mock_row  [E] the row of the items' mock pools ensemble e is compared with, 0 <= row < n_mocks of every item's pool, repeats
 *             allowed (the row of every engine row is written once per call, not per half-step); NULL: every ensemble reads the
 *             installed data
 *   x, lnL, accepted   [E][W][n], [E][W], [E][W] host: the walkers' state, read at entry and written back at exit
 *   step0, n_steps, thin   as for the single run, shared by the ensembles
 *   chain, chain_lnL       [E][rows][W][n], [E][rows][W] (host, NULL: not kept)
 *   stats     the totals over the ensembles; per_ensemble [E][3] (NULL: not wanted): accepted, rejected outside the box, rejected
 *             for a failed model, of this call
 * Refused before anything runs (-1, vmx_last_error, the engine untouched): whatever the single run refuses, for every ensemble;
 * E < 1; streams NULL; a mock row that is negative or not below n_mocks; mock rows while an item has no pool; E W beyond the
 * engine's int32 row count or a chain beyond size_t.  A HIP failure later returns -2 and leaves the engine usable. */
int vmx_ensemble_run_many(vmx_engine* e, const vmx_ensemble_spec* spec, int32_t E, int32_t W,
                          const uint64_t* streams, const int32_t* mock_row,
                          double* x, double* lnL, int64_t* accepted,
                          int64_t step0, int32_t n_steps, int32_t thin,
                          double* chain, double* chain_lnL,
                          const vmx_ensemble_options* opt,
                          vmx_ensemble_stats* stats, int64_t* per_ensemble);
/* The same run with every walker's move drawn from a mixture of the stretch move, the differential-evolution move (ter Braak
 * 2006, emcee's DEMove) and the snooker move (ter Braak & Vrugt 2008, emcee's DESnookerMove): what an emcee user writes as
 * moves=[(DEMove(), 0.8), (DESnookerMove(), 0.2)].  The stretch move's acceptance falls with the number of sampled parameters and
 * one point on a line through one partner rarely crosses between separated modes; both new moves are red-blue moves like it (a
 * walker of the active half moves using walkers of the other half alone: two distinct ones for DE, three for the snooker), so
 * the half-step, the box rule and the decision are unchanged.  Every expression, the second Philox block (counter (k, s, h, 1):
 * move choice and jitter) and the rule of the distinct partners are pinned in vega_amd/csrc/vmx_ensemble.h.  The half-step kernel
 * is k_ens_half_moves, beside k_ens_half: one work-group per ensemble, the same decide / record / propose order.
 *   moves     weights[3]: (stretch, DE, snooker), each >= 0, of positive sum (they need not add up to 1; a pure move has the
 *             others 0); gamma0: the DE scale (emcee's default 2.38 / sqrt(2 n), computed by the caller); sigma: the relative
 *             width of the DE jitter, gamma = gamma0 (1 + sigma g) with g triangular on (-1, 1) (default 1e-5); gamma_s: the
 *             snooker scale (default 1.7); flags, reserved: 0.  NULL runs exactly vmx_ensemble_run_many (k_ens_half).  Weights
 *             (1, 0, 0) give the chain of vmx_ensemble_run_many bit for bit through the other kernel.
 *   everything else as for vmx_ensemble_run_many; the single run is E = 1 with streams = &stream.
 * The statistics are those of vmx_ensemble_run_many: a snooker proposal that is none (the walker on its partner, a factor that is
 * not finite) counts with the rejections outside the box.
 * Refused before anything runs (-1, vmx_last_error, the engine untouched): whatever vmx_ensemble_run_many refuses; a negative or
 * non-finite weight or a zero sum of weights; a DE weight with W / 2 < 2; a snooker weight with W / 2 < 3; gamma0 or gamma_s
 * non-positive or non-finite; sigma negative or non-finite; flags or reserved not 0. */
typedef struct {
    double weights[3];
    double gamma0, sigma, gamma_s;
    uint32_t flags, reserved;
} vmx_ensemble_moves;
int vmx_ensemble_run_many_moves(vmx_engine* e, const vmx_ensemble_spec* spec, int32_t E, int32_t W,
                                const uint64_t* streams, const int32_t* mock_row,
                                double* x, double* lnL, int64_t* accepted,
                                int64_t step0, int32_t n_steps, int32_t thin,
                                double* chain, double* chain_lnL,
                                const vmx_ensemble_options* opt,
                                vmx_ensemble_stats* stats, int64_t* per_ensemble,
                                const vmx_ensemble_moves* moves);
/* Parallel tempering (Swendsen & Wang 1986; ptemcee): G ladders of T ensembles each, the rungs of a ladder differing only in the
 * beta that multiplies lnL in the Metropolis decision, with swaps of walkers between adjacent rungs - what lets the cold rung
 * cross between separated modes, and what gives the evidence from the rungs' lnL records (stepping stones or thermodynamic
 * integration, on the host: vega_amd/ensemble.py).  The run is vmx_ensemble_run_many_moves over the G T ensembles (ladder g owns
 * g T .. g T + T - 1, rung 0 cold) through the half-step kernel k_ens_half_pt; after every swap_every-th step one more small
 * kernel, k_ens_swap (one work-group per ladder), exchanges walkers from the hottest pair of rungs down, between the deciding
 * half-step and the next proposal.  It needs no likelihood row - lnL is stored untempered - and no host wait: the call keeps its
 * single synchronisation.  The tempered decision, the rotation that pairs the walkers, the swap rule and their two Philox blocks
 * (counters (k, s, t, 2) and (0, s, t, 3), key (seed, stream of the ladder's rung 0)) are pinned in vega_amd/csrc/vmx_ensemble.h.
 *   G, T, W   ladders (>= 1) of T rungs (1 <= T <= VMX_PT_MAXT) of W walkers each, W even and >= 2 n
 *   betas     [T]: betas[0] = 1 > betas[1] > ... > betas[T - 1] >= 0, shared by the ladders.  With beta = 1 a rung's decisions are
 *             those of vmx_ensemble_run_many_moves bit for bit; with beta = 0 a rung samples the box (a proposal outside it, or
 *             with a failed model, is still rejected)
 *   streams   [G T] the Philox stream of every rung
 *   mock_row  [G] the row of the items' mock pools ladder g is compared with; NULL: the installed data
 *   x, lnL, accepted   [G T][W][n], [G T][W], [G T][W] host: the state, read at entry and written back at exit; lnL is
 *             log_norm - 0.5 chi2 on every rung.  A swap exchanges positions and lnL; accepted stays with the slot
 *   step0, n_steps, thin   as for vmx_ensemble_run_many
 *   swap_every  a sweep after every global step s with (s + 1) % swap_every == 0, before that step's chain row (a run cut into
 *             calls swaps at the same steps); 0: no swaps - every rung is then the plain ensemble at its beta
 *   chain, chain_lnL       [G T][rows][W][n], [G T][rows][W] (host, NULL: not kept): the records of all rungs
 *   stats, per_ensemble [G T][3]   as for vmx_ensemble_run_many
 *   moves     as for vmx_ensemble_run_many_moves; NULL: the stretch move
 *   swaps     [G][T - 1][2] (NULL: not wanted): per pair of rungs (t, t + 1) the swaps proposed and accepted in this call
 * Refused before anything runs (-1, vmx_last_error, the engine untouched): whatever vmx_ensemble_run_many_moves refuses; G < 1;
 * T < 1 or T > VMX_PT_MAXT; betas NULL, betas[0] != 1, a beta that is not finite, negative or not below the one before it;
 * swap_every < 0; G T W beyond the engine's int32 row count. */
#define VMX_PT_MAXT 64
int vmx_ensemble_run_pt(vmx_engine* e, const vmx_ensemble_spec* spec, int32_t G, int32_t T, int32_t W,
                        const double* betas, const uint64_t* streams, const int32_t* mock_row,
                        double* x, double* lnL, int64_t* accepted,
                        int64_t step0, int32_t n_steps, int32_t thin, int32_t swap_every,
                        double* chain, double* chain_lnL,
                        const vmx_ensemble_options* opt,
                        vmx_ensemble_stats* stats, int64_t* per_ensemble,
                        const vmx_ensemble_moves* moves, int64_t* swaps);
/* Adaptive ladders (Vousden, Farr & Mandel 2016; ptemcee's adaptation_lag / adaptation_time): the run above with a ladder of its
 * own for every one of the G ladders, whose intermediate betas move after every swap sweep so that all adjacent pairs of rungs come
 * to swap at the same rate; the adjustment decays, so that the chain becomes a proper one.  The swap kernel is k_ens_swap_adapt
 * beside k_ens_swap - the same grid, pairs, rotation, swap rule and counters: it gathers the sweep's accepted swaps per pair of
 * rungs in LDS, and behind the last pair one thread moves the ladder (at most T - 2 exponentials, the pinned pexp) before the
 * half-step kernel that follows on the stream reads it.  No host wait and no likelihood row.  The rule and its guard are pinned in
 * vega_amd/csrc/vmx_ensemble.h, the fourth part:
 *     A_t = accepted_t / W of this sweep for the pair (t, t + 1); time = (s + 1) / swap_every - 1, the sweeps before this one;
 *     kappa = (lag / (time + lag)) / adapt->time; for i = 0 .. T - 3: the gap 1 / beta[i + 1] - 1 / beta[i] of the old ladder is
 *     multiplied by pexp(kappa (A_i - A_{i+1})) and the new 1 / beta[i + 1] is 1 / beta[0] plus the gaps so far.
 * betas[.][0] = 1 and betas[.][T - 1] never move.  A new ladder that is not one the sampler takes (not finite, not strictly
 * decreasing - a positive last beta can be crossed) is dropped: the old one stays for that sweep and adapt_skipped[g] counts it.
 *   betas     [G][T], in and out: every ladder as vmx_ensemble_run_pt takes one; at exit the ladders after the call's last sweep
 *   adapt     lag, time: ptemcee's adaptation_lag and adaptation_time, in sweeps, finite and positive (its defaults 10000, 100);
 *             adapt_until: the sweep after global step s adapts iff s < adapt_until (negative: always; 0: never - the chain
 *             of vmx_ensemble_run_pt for equal ladders); flags, reserved: 0
 *   beta_hist [sweeps][G][T] (NULL: not kept), sweeps = (step0 + n_steps) / swap_every - step0 / swap_every: the ladders after
 *             every sweep of this call, adapting or not
 *   adapt_skipped  [G] (NULL: not wanted): the sweeps of this call whose adjustment the guard dropped
 *   everything else as for vmx_ensemble_run_pt.  time depends on the global step alone: a run cut into calls adapts identically.
 * Refused before anything runs (-1, vmx_last_error, the engine untouched): whatever vmx_ensemble_run_pt refuses; T < 3;
 * swap_every < 1; adapt NULL; lag or time not finite and positive; flags or reserved not 0; any of the G ladders not in order. */
typedef struct {
    double lag, time;
    int64_t adapt_until;
    uint32_t flags, reserved;
} vmx_ensemble_adapt;
int vmx_ensemble_run_pt_adapt(vmx_engine* e, const vmx_ensemble_spec* spec, int32_t G, int32_t T, int32_t W,
                              double* betas, const uint64_t* streams, const int32_t* mock_row,
                              double* x, double* lnL, int64_t* accepted,
                              int64_t step0, int32_t n_steps, int32_t thin, int32_t swap_every,
                              double* chain, double* chain_lnL,
                              const vmx_ensemble_options* opt,
                              vmx_ensemble_stats* stats, int64_t* per_ensemble,
                              const vmx_ensemble_moves* moves, int64_t* swaps,
                              const vmx_ensemble_adapt* adapt, double* beta_hist, int64_t* adapt_skipped);
/* Ensemble slice sampling (Karamanis & Beutler 2021, zeus's differential move) for the E ensembles of vmx_ensemble_run_many: a
 * walker's update takes its direction from two walkers of the other half and its step from a slice-sampling bracket along it, so
 * no update is rejected, and the scale of the direction tunes itself.  A trial point outside the box is answered by the walker's
 * machine itself: every engine row is a real evaluation, none a walker's own position.  The counters, the machine, the tuning
 * rule and the packing of a round are pinned in vega_amd/csrc/vmx_ensemble.h, the fifth part.  The run goes in rounds
 * (k_ens_slice_advance: one work-group per running ensemble, one lane per walker; k_ens_slice_emit: the requests of all ensembles
 * behind each other); the host reads one integer per round and hands the engine that many rows in chunks of `chunk`.
 *   slice     mu0: the scale a caller starts mu from (default 1; the library reads mu, not mu0, but refuses a bad mu0);
 *             tune_steps: the steps with global index s < tune_steps tune mu (their rows are no stationary chain: discard them);
 *             max_expansions (<= 32, per side) and max_contractions (<= 64): the caps of one update; flags: 0
 *   mu        [E], in and out: the scale of every ensemble, positive and finite
 *   slice_counts   [E][8] (NULL: not wanted), of this call: updates, updates that moved the walker, engine rows, expansions,
 *             contractions, box answers, failed-model answers, updates that ended capped or had a null direction
 *   stats     proposals = updates, accepted = moved; host_synchronisations = rounds + 1
 *   accepted  counts, per walker, the updates that moved it
 *   everything else as for vmx_ensemble_run_many; spec->a is not read.  The single run is E = 1.
 * Refused before anything runs (-1, vmx_last_error, the engine untouched): whatever vmx_ensemble_run_many refuses; W < 4 (two
 * partners in the other half); mu0 or an entry of mu not positive and finite; tune_steps < 0; a cap < 1 or beyond 32 / 64;
 * flags != 0; slice or mu NULL. */
#define VMX_SLICE_COUNTS 8
#define VMX_SLICE_MAX_EXPANSIONS 32
#define VMX_SLICE_MAX_CONTRACTIONS 64
typedef struct { double mu0; int32_t tune_steps, max_expansions, max_contractions, flags; } vmx_ensemble_slice;
int vmx_ensemble_run_slice(vmx_engine* e, const vmx_ensemble_spec* spec, int32_t E, int32_t W,
                           const uint64_t* streams, const int32_t* mock_row,
                           double* x, double* lnL, int64_t* accepted,
                           int64_t step0, int32_t n_steps, int32_t thin,
                           double* chain, double* chain_lnL,
                           const vmx_ensemble_options* opt, vmx_ensemble_stats* stats,
                           const vmx_ensemble_slice* slice, double* mu, int64_t* slice_counts);
/* The covariance move: vmx_ensemble_run_many_moves with a fourth member in the mixture, a Metropolis step whose increment has the
 * covariance of the complementary half scaled by gamma_c - emcee's WalkMove taken over the whole other half, with the
 * Roberts-Gelman-Gilks scale 2.38 / sqrt(n).  The stretch, DE and snooker moves take their direction from one, two or three
 * partners; this one uses what the other half knows about the posterior's shape.  It is a red-blue move like them: the factor
 * depends on the other half alone, so the half-step, the box rule and the decision are unchanged.  The mean, the covariance, its
 * lower Cholesky factor C (the operation order of vmx_ns::cholesky; a pivot that is not positive: diag(sqrt(cov_aa)), counted as a
 * fallback), the variate z of a 64-bit word (the centred sum of its four 16-bit fields: unit variance, symmetric, not normal), the
 * further Philox blocks (counter (k, s, h, 2 + b / 4)) and the proposal y = s + gamma_c (C z) are pinned in
 * vega_amd/csrc/vmx_ensemble.h, the sixth part.  The half-step kernel is k_ens_half_cov: between the decision and the proposals
 * the ensemble's work-group computes the factor in LDS, every entry by one thread with the pinned serial expression, so that the
 * factor is the serial one bit for bit.
 *   cov       weight: the move's weight beside moves->weights (stretch, DE, snooker), >= 0 - the four need a positive sum, and
 *             moves must not be NULL when the weight is positive; scale: gamma_c (default 2.38 / sqrt(n), computed by the caller);
 *             flags, reserved: 0.  NULL, or weight 0, runs exactly vmx_ensemble_run_many_moves.
 *   fallbacks [E] (NULL: not wanted), of this call: the half-steps whose factor fell back to the diagonal
 *   everything else as for vmx_ensemble_run_many_moves; the single run is E = 1.
 * Refused before anything runs (-1, vmx_last_error, the engine untouched): whatever vmx_ensemble_run_many_moves refuses; a
 * negative or non-finite cov weight; a zero sum over the four weights; a cov weight with W / 2 < 2; a scale that is not positive
 * and finite; flags or reserved not 0.
 * vmx_ensemble_cov_factor runs the factor stage alone, for tests and diagnostics: the halves x [E][H][n] (2 <= H, 1 <= n <=
 * VMX_ENS_MAXN, n <= H not required) give mean [E][n], factor [E][n][n] (lower, the strict upper triangle 0) and flag [E] (1: the
 * Cholesky factor, 0: the diagonal fallback).  The engine gives the device and the stream; nothing of it is read or changed. */
typedef struct { double weight, scale; uint32_t flags, reserved; } vmx_ensemble_cov;
int vmx_ensemble_run_many_cov(vmx_engine* e, const vmx_ensemble_spec* spec, int32_t E, int32_t W,
                              const uint64_t* streams, const int32_t* mock_row,
                              double* x, double* lnL, int64_t* accepted,
                              int64_t step0, int32_t n_steps, int32_t thin,
                              double* chain, double* chain_lnL,
                              const vmx_ensemble_options* opt,
                              vmx_ensemble_stats* stats, int64_t* per_ensemble,
                              const vmx_ensemble_moves* moves, const vmx_ensemble_cov* cov, int64_t* fallbacks);
int vmx_ensemble_cov_factor(vmx_engine* e, int32_t E, int32_t H, int32_t n, const double* x, double* mean, double* factor,
                            int32_t* flag);
/* A chain store: the recorded rows of E ensembles of W walkers over n columns kept on the device, positions [E][capacity][W][n]
 * and lnL [E][capacity][W], and reduced there (vega_amd/csrc/vmx_chain.h pins every sum).  A store belongs to the engine it was
 * created on and is destroyed with it at the latest.
 *   create    E >= 1, 2 <= W <= 1024, 1 <= n <= VMX_ENS_MAXN, capacity_rows >= 0.  A failed allocation returns -2 and leaves the
 *             engine usable.
 *   reserve   grows the capacity to capacity_rows (never shrinks); the stored rows are kept.
 *   rows      the rows stored, per ensemble.
 *   append    uploads `rows` rows of every ensemble from the host, chain [E][rows][W][n] and chain_lnl [E][rows][W], behind the
 *             stored ones (the `python` driver's rows, synthetic chains).
 *   fetch     the rows [row0, row0 + rows) as chain [E][rows][W][n] and chain_lnl [E][rows][W] - the layout the run entries write;
 *             either pointer may be NULL.
 *   vmx_ensemble_set_chain_store   while a store is attached (NULL: detached) every ensemble run - vmx_ensemble_run and all the
 *             vmx_ensemble_run_* entries - appends the rows it records device to device, one pitched copy per array on the engine's
 *             stream behind the half-step kernels.  The call's host `chain` / `chain_lnL` may then be NULL: nothing of the chain
 *             is copied to the host, and the call's single wait stays single.  A run of G ladders of T rungs needs E = G T.
 *   summary   over the rows [first_row, rows) of every ensemble, with Sokal's window constant c (emcee: 5): count [E] (= (rows -
 *             first_row) W), mean [E][n], covariance [E][n][n] (two passes, ddof 1 over rows x walkers), tau [E][n] and window
 *             [E][n] (emcee's integrated autocorrelation time by direct lag sums up to the window).  Any output may be NULL; tau
 *             and window both NULL skip the autocorrelation, mean and covariance both NULL the moments' second pass.
 * Refused before anything runs (-1, vmx_last_error, engine and store untouched): a NULL engine or store; sizes outside the ranges
 * above, or whose product overflows; an attached store whose (E, W, n) is not the run's, or without room for the run's rows; rows
 * beyond the capacity (append); row0 + rows beyond the rows stored (fetch); first_row outside [0, rows) or a c that is not positive
 * and finite (summary).
 *   order_stats   exact order statistics of every (ensemble, column) over the rows [first_row, rows) (vega_amd/csrc/
 *             vmx_chain_select.h pins the order): with N = (rows - first_row) W values per column, values[e][d][r] is the
 *             ranks[r]-th smallest of them (0 <= ranks[r] < N) in the total order -inf < ... < -0 < +0 < ... < +inf < NaN - a stored
 *             value's own bits, or the canonical NaN.  The ranks may come in any order and may repeat; the answer does not depend
 *             on the other ranks asked.  A radix select on the device, no floating-point operation: bitwise reproducible.
 *   best      the largest lnL of every ensemble over the rows [first_row, rows) x walkers: lnl_max [E], its row [E] (counted from
 *             row 0 of the store) and walker [E], and the position [E][n] there (position may be NULL).  A NaN never wins, -inf
 *             may; among equal values the lowest (row, walker) wins.  An ensemble without a candidate (all NaN): row -1, walker
 *             -1, lnl_max and position NaN.
 * Both take one host wait, on the engine's stream, like summary.  Refused before anything runs (-1, vmx_last_error, engine and store
 * untouched): a NULL store or a NULL output (position alone may be NULL); first_row outside [0, rows); n_ranks outside [1,
 * VMX_CHAIN_MAX_RANKS]; a rank outside [0, N); N >= 2^31 (order_stats).  A failed allocation returns -2 and leaves the engine usable. */
#define VMX_CHAIN_MAX_RANKS 32
typedef struct vmx_chain_store vmx_chain_store;
int vmx_chain_store_create(vmx_engine* e, int32_t E, int32_t W, int32_t n, int64_t capacity_rows, vmx_chain_store** out);
int vmx_chain_store_destroy(vmx_chain_store* store);
int vmx_chain_store_reserve(vmx_chain_store* store, int64_t capacity_rows);
int vmx_chain_store_rows(vmx_chain_store* store, int64_t* rows);
int vmx_chain_store_append(vmx_chain_store* store, int64_t rows, const double* chain, const double* chain_lnl);
int vmx_chain_store_fetch(vmx_chain_store* store, int64_t row0, int64_t rows, double* chain, double* chain_lnl);
int vmx_chain_store_summary(vmx_chain_store* store, int64_t first_row, double c, int64_t* count, double* mean, double* covariance,
                            double* tau, int64_t* window);
int vmx_chain_store_order_stats(vmx_chain_store* store, int64_t first_row, int32_t n_ranks, const int64_t* ranks,
                                double* values /* [E][n][n_ranks] */);
int vmx_chain_store_best(vmx_chain_store* store, int64_t first_row, double* lnl_max /* [E] */,
                         int64_t* row /* [E], counted from row 0 of the store */, int32_t* walker /* [E] */, double* position /* [E][n] */);
int vmx_ensemble_set_chain_store(vmx_engine* e, vmx_chain_store* store);
/* A sample store: E weighted, ragged sample sets over n columns kept on the device - the posterior samples of nested or SMC runs -
 * positions [E][capacity][n], lnL [E][capacity] and weights [E][capacity], and reduced there (vega_amd/csrc/vmx_chain_weighted.h
 * pins every sum and the order statistic).  Set e has count[e] rows, 0 <= count[e] <= capacity; nothing behind them is ever read.
 * A store belongs to the engine it was created on and is destroyed with it at the latest.
 *   create    E >= 1, 1 <= n <= VMX_ENS_MAXN, 0 <= capacity_rows < 2^31; every set starts empty.
 *   put       replaces set `set` by `count` rows from the host, x [count][n], lnl [count] and w [count]; count 0 empties it.  The
 *             weights need not sum to 1; each must be finite and >= 0 (they are scanned here, where the rows are).
 *   counts    the rows of every set [E].
 *   fetch     the rows of set `set`, x [count][n], lnl [count] and w [count]; any pointer may be NULL.
 *   summary   per set: S [E] (the sum of the weights), n_eff [E] (Kish: 1 / sum p^2 with p = w / S), mean [E][n], covariance
 *             [E][n][n] (two passes, sum p dx dx^T / (1 - sum p^2)), total [E] (M, the sum of the integer weights m = floor(w /
 *             w_max 2^32)) and w_max [E].  Every sum of doubles is a stride-halving tree whose shape depends on count alone.  NaN,
 *             not an error, where a set cannot say: count = 0 or S = 0 (mean, covariance, n_eff); one row with all the weight
 *             (covariance).
 *   order_stats   weighted order statistics of every (set, column): values[e][d][r] is the smallest stored value v of column d, in
 *             the total order -inf < ... < -0 < +0 < ... < +inf < NaN, with sum_{x <= v} m >= targets[e][r] - a stored value's own
 *             bits, or the canonical NaN - for 1 <= targets[e][r] <= M_e, in any order, repeats allowed.  The inverted-CDF quantile
 *             q of set e is the value at max(1, ceil(q M_e)).  A radix select over integer sums: no floating-point operation once
 *             the integer weights are made, bitwise reproducible.  A set with M = 0 ignores its targets and answers NaN.
 *   best      the largest lnL of every set: lnl_max [E], its row index [E] and the position [E][n] there (position may be NULL).  A
 *             NaN never wins, ties go to the lowest row; a set without a candidate: index -1, lnl_max and position NaN.
 * summary, order_stats and best take one host wait each, on the engine's stream.  Refused before anything runs (-1, vmx_last_error,
 * engine and store untouched): a NULL engine, store or output (position and the pointers of fetch may be NULL); sizes outside the
 * ranges above; a set outside [0, E); count beyond the capacity; a weight that is negative, NaN or infinite; n_targets outside [1,
 * VMX_SAMPLE_MAX_TARGETS]; a target of 0 or above M_e for a set with M_e > 0.  A failed allocation returns -2 and leaves the engine
 * usable. */
#define VMX_SAMPLE_MAX_TARGETS 16
typedef struct vmx_sample_store vmx_sample_store;
int vmx_sample_store_create(vmx_engine* e, int32_t E, int32_t n, int64_t capacity_rows, vmx_sample_store** out);
int vmx_sample_store_destroy(vmx_sample_store* store);
int vmx_sample_store_put(vmx_sample_store* store, int32_t set, int64_t count, const double* x, const double* lnl, const double* w);
int vmx_sample_store_counts(vmx_sample_store* store, int64_t* counts /* [E] */);
int vmx_sample_store_fetch(vmx_sample_store* store, int32_t set, double* x, double* lnl, double* w);
int vmx_sample_store_summary(vmx_sample_store* store, double* S, double* n_eff, double* mean, double* covariance, uint64_t* total,
                             double* w_max);
int vmx_sample_store_order_stats(vmx_sample_store* store, int32_t n_targets, const uint64_t* targets /* [E][n_targets] */,
                                 double* values /* [E][n][n_targets] */);
int vmx_sample_store_best(vmx_sample_store* store, double* lnl_max /* [E] */, int64_t* index /* [E] */, double* position /* [E][n] */);
/* Evidence where the live points live: nested sampling (Skilling 2006) by slice sampling in the whitened unit cube (the scheme of
 * PolyChord, which the reference runs in bin/run_vega_mpi.py), every decision pinned in vega_amd/csrc/vmx_nested.h.  An iteration
 * kills the K live points of lowest lnL, whitens with the survivors' covariance and lets K threads each walk num_repeats slice
 * steps from a random survivor under lnL > L*; the end points replace the dead.  One small kernel heads the iteration
 * (k_ns_iteration); then rounds: k_ns_advance gives every thread the answer to its last request, advances its state machine and
 * compacts the next requests into the engine's rows, the host reads the row count (one mapped word) and enqueues the engine's
 * chain over the rows in chunks of `chunk` (two lanes alternate when the quadratic form serves them).  When no thread asks any
 * more the same kernel has written the live and the newly dead lnL beside the word, and `stop` decides whether to go on.
 *   spec      n_params = the engine's; n sampled columns col[n] with their box [lo, hi] (finite, lo < hi: the uniform prior);
 *             nlive live points, K threads, num_repeats slice steps per thread; log_norm (lnL = log_norm - 0.5 chi2); seed /
 *             stream (the Philox key); theta_fixed[n_params], the row that supplies the columns not sampled
 *   live_u, live_lnl   [nlive][n] in the unit cube, [nlive] host: the run's state, read at entry (unless opt->draw_live) and
 *             written back at exit; *iteration the global index of the next iteration, advanced by the iterations done (a run
 *             cut into calls is the same run)
 *   dead_u, dead_lnl, dead_nlive   [n_iterations K][n], [n_iterations K], [n_iterations K] host: the deaths of this call in
 *             order, each with the live count at its death (nlive - j for the j-th of an iteration); stats->iterations K rows
 *             are written
 *   opt       const_hint (-1: derived - a column varies when it is sampled), chunk (rows per engine call, 0: max_batch), lanes
 *             (0: 2), draw_live (nonzero: *iteration must be 0; the live points are drawn from the Philox blocks (i, 0, j, 2) and
 *             evaluated first), stop (called after every iteration with the iterations done in the run, the K newly dead lnL and
 *             the live lnL; nonzero ends the call; NULL: all n_iterations run), user (handed to stop); NULL: -1, 0, 0, 0, NULL
 *   stats     host_waits = rounds + iterations + 1 (the copy back) + 1 with draw_live
 * Refused before anything runs (-1, vmx_last_error, the engine untouched): n outside 1 .. 32, nlive outside n + 2 .. 4096, K
 * outside 1 .. nlive - n - 1, num_repeats < 1, a column out of range or repeated, a non-finite limit or lo >= hi, a live point
 * outside the cube or with a NaN lnL (without draw_live).  A HIP failure later returns -2 and leaves the engine usable. */
#define VMX_NS_MAXN 32
#define VMX_NS_MAX_LIVE 4096
typedef struct {
    int32_t n_params, n;
    const int32_t* col; const double* lo; const double* hi;
    int32_t nlive, K, num_repeats, reserved;
    double log_norm;
    uint64_t seed, stream;
    const double* theta_fixed;
} vmx_nested_spec;
typedef int32_t (*vmx_nested_stop)(void* user, int64_t iterations, const double* dead_lnl, const double* live_lnl);
typedef struct {
    int32_t const_hint, chunk, lanes, draw_live;
    vmx_nested_stop stop; void* user;
} vmx_nested_options;
typedef struct {
    int64_t iterations, rounds, rows, rows_own_position, engine_calls, host_waits;
    double seconds, seconds_enqueuing;
    int32_t const_hint, lanes;          /* what the call ran with */
} vmx_nested_stats;
int vmx_nested_run(vmx_engine* e, const vmx_nested_spec* spec, double* live_u, double* live_lnl, int64_t* iteration,
                   int32_t n_iterations, double* dead_u, double* dead_lnl, int32_t* dead_nlive,
                   const vmx_nested_options* opt, vmx_nested_stats* stats);
/* The same run with the survivors of every iteration split into clusters, every cluster whitened on its own and persistent ids
 * (the reference's [Polychord] do_clustering; the rule, pinned: vega_amd/csrc/vmx_nested.h "clustering").  After the kill one launch
 * of k_ns_knn (a grid over the survivors, the points streamed through LDS) lists every survivor's VMX_NS_KNN nearest others, one
 * work-group (k_ns_cluster) turns the lists into components, at most VMX_NS_MAX_CLUSTERS clusters, ids, means and factors; every
 * thread then walks with the factor of its start point's cluster and its end point inherits that cluster's id.  All arguments
 * before `clusters` are those of vmx_nested_run, with its checks and its statistics.
 *   clusters  flags: VMX_NS_CLUSTER to cluster; 0 runs exactly what vmx_nested_run runs and touches nothing else in the struct
 *             live_cluster [nlive] host: the id of every live point (0: never labelled), read at entry, written back at exit
 *             next_id      [1] host: the next unused id (a new run: 1), read at entry, written back at exit; with live_cluster
 *                          it is part of the run's state, so that a run cut into calls stays the same run
 *             dead_cluster [n_iterations K] host: beside dead_u / dead_lnl, the id every dead point held when it was killed
 * Refused in addition (-1): clusters NULL, unknown flags; with VMX_NS_CLUSTER a missing array, next_id < 1 or so large that the
 * call could overflow it, an id outside 0 .. next_id - 1. */
#define VMX_NS_KNN 8
#define VMX_NS_MAX_CLUSTERS 8
#define VMX_NS_CLUSTER 1u
typedef struct {
    int32_t* live_cluster; int32_t* next_id; int32_t* dead_cluster;
    uint32_t flags, reserved;
} vmx_nested_clusters;
int vmx_nested_run_clustered(vmx_engine* e, const vmx_nested_spec* spec, double* live_u, double* live_lnl, int64_t* iteration,
                             int32_t n_iterations, double* dead_u, double* dead_lnl, int32_t* dead_nlive,
                             const vmx_nested_options* opt, vmx_nested_stats* stats, const vmx_nested_clusters* clusters);
/* The same run (with or without clustering) keeping the accepted points inside the threads' walks - the reference's [Polychord]
 * boost_posterior; the rule, pinned: vega_amd/csrc/vmx_nested.h "boost".  Every thread of an iteration makes num_repeats slice
 * steps and only its end point joins the live points; the num_repeats - 1 accepted points before it were evaluated under the
 * same constraint and are each a uniform draw from the contour.  k_ns_advance_phantoms / k_ns_advance_phantoms_clustered are
 * k_ns_advance / k_ns_advance_clustered with one more step: after a thread's advance its lane asks vmx_ns::phantom_of and
 * vmx_ns::phantom_kept, a second prefix scan gives the kept points of the round their places behind a running count (one
 * work-group: no atomic decides a place), and the lanes write the record one column per lane.  The base run - dead record, live
 * points, statistics, random streams - is bit for bit the one without `phantoms`; no likelihood row is added.
 *   clusters  NULL: what vmx_nested_run runs; else as for vmx_nested_run_clustered
 *   phantoms  fraction: every phantom point (k, t, r) is kept iff u01(word 0 of the Philox block (k, t, r, 3)) < fraction;
 *                       0 (or phantoms NULL) runs exactly vmx_nested_run / vmx_nested_run_clustered and touches nothing in the struct
 *             capacity: rows of the arrays below, at least n_iterations K (num_repeats - 1): what the call can keep at the most
 *             u [capacity][n], lnl, birth [capacity], iteration (int64), thread, repeat [capacity] host: the kept points in the
 *                       order they were accepted (round by round, threads ascending within a round: sort by the tags for the
 *                       canonical order), their lnL, the L* they were accepted under and (iteration, thread, repeat)
 *             cluster [capacity] host: the id of the thread's cluster, what its end point inherits; read with clustering only
 *                       (then required), else it may be NULL
 *             count:    out, the rows written
 *             flags, reserved: 0
 * The record comes back in the copy that brings the dead record: stats->host_waits is what it is without phantoms.
 * Refused in addition (-1, the engine untouched): a fraction outside [0, 1] or NaN, a missing array, a capacity below
 * n_iterations K (num_repeats - 1), non-zero flags. */
typedef struct {
    double fraction;
    int64_t capacity;
    double* u; double* lnl; double* birth;
    int64_t* iteration; int32_t* thread; int32_t* repeat; int32_t* cluster;
    int64_t count;
    uint32_t flags, reserved;
} vmx_nested_phantoms;
int vmx_nested_run_phantoms(vmx_engine* e, const vmx_nested_spec* spec, double* live_u, double* live_lnl, int64_t* iteration,
                            int32_t n_iterations, double* dead_u, double* dead_lnl, int32_t* dead_nlive,
                            const vmx_nested_options* opt, vmx_nested_stats* stats, const vmx_nested_clusters* clusters,
                            vmx_nested_phantoms* phantoms);
/* The clustering of one iteration on host arrays, the two kernels' unit-test entry: m points u[m][n] (finite) with previous ids
 * prev_id[m] (0: none; all below *next_id) on `device`.  Writes ids[m] (every point's new id), *k_used (the neighbour level 3 .. 8
 * the components were taken at), *n_clusters (1 .. VMX_NS_MAX_CLUSTERS), means [VMX_NS_MAX_CLUSTERS][n] and factors
 * [VMX_NS_MAX_CLUSTERS][n][n] (the clusters in their order: size descending, then smallest member ascending; rows beyond
 * *n_clusters are zero) and moves *next_id past the ids it handed out.  Refused (-1): n outside 1 .. 32, m outside 2 .. 4096, a
 * coordinate that is not finite, an id outside 0 .. *next_id - 1.  A HIP failure returns -2. */
int vmx_nested_cluster_points(int32_t device, const double* u, int32_t m, int32_t n, const int32_t* prev_id, int32_t* next_id,
                              int32_t* ids, int32_t* k_used, int32_t* n_clusters, double* means, double* factors);
/* E independent nested-sampling runs advanced together: log Z and a weighted posterior for every Monte-Carlo mock, or the replicas
 * of one run, as one device run (the rule, pinned: vega_amd/csrc/vmx_nested.h "a set of runs").  A run of a few hundred live points
 * hands the engine a fraction of a batch per round and stops the host every round; here a set round is at most three launches
 * for the whole set - k_ns_set_head (one work-group per run whose iteration begins: k_ns_iteration's body), k_ns_set_advance (one
 * per run still in the set: every thread takes the answer of the engine row it asked for and advances; the run counts its
 * requests; a run that asks for nothing ends its iteration there) and k_ns_set_emit (the requests of all runs packed into the
 * engine's rows [0, total) in ascending (run, thread) order, the offsets a sum of the counts in list order) - then one host wait,
 * and the total rows go through the engine as one stream of chunks of `chunk` on two lanes.  Runs do not wait for each other's
 * iterations: a run whose iteration ended in round r is headed in round r + 1.  Run e is by construction the run vmx_nested_run
 * makes with spec->stream = streams[e] on the data of mock_row[e]; its chi2 is evaluated in batches of another shape, so that
 * its lnL may differ from the single run's in the last bits (E = 1 has the single run's batches and gives it bit for bit).
 * Clustering is not part of the set.
 *   spec      as for the single run; spec->stream is not read
 *   E         runs (>= 1) of spec->nlive live points and spec->K threads each
 *   streams   [E] the Philox stream of every run (repeats allowed)
 *   mock_row  [E] the row of the items' mock pools run e is compared with, 0 <= row < n_mocks of every item's pool, repeats
 *             allowed; NULL: every run reads the installed data
 *   live_u, live_lnl   [E][nlive][n], [E][nlive] host: the runs' state, read at entry (unless opt->draw_live), written back at exit
 *   iteration [E] the global index of every run's next iteration (runs may enter at different ones), advanced by iterations_done
 *   status    [E] out: 0 the run is still going (n_iterations used up), 1 its stop callback ended it, 2 with draw_live no live
 *             point has a finite lnL - the run is never entered, its arrays are left as they were, its iterations_done is 0 and
 *             the call does not fail
 *   n_iterations   at most so many iterations per run in this call
 *   dead_u, dead_lnl, dead_nlive   [E][n_iterations K][n], [E][n_iterations K] x 2 host: every run's deaths as the single run
 *             records them; iterations_done[e] K rows of run e are written
 *   iterations_done   [E] out
 *   opt       vmx_nested_options with the stop callback of a set: stop(user, run, iterations, dead_lnl [K], live_lnl [nlive]) is
 *             called after every iteration of every run with the iterations done in that run; nonzero ends that run alone.
 *             draw_live applies to every run (every iteration[e] must then be 0).
 *   stats     the totals over the runs; rounds: the set rounds; host_waits = set rounds + 1 (the copy back) + 1 with draw_live.
 *             per_run [E][3] (NULL: not wanted): rows evaluated (the nlive drawn ones included), rows that were a thread's own
 *             position, set rounds the run took part in
 * Refused before anything runs (-1, vmx_last_error, the engine untouched): whatever the single run refuses, for every run; E < 1;
 * streams NULL; a mock row that is negative or not below n_mocks; mock rows while an item has no pool; E nlive beyond the
 * engine's int32 row count or a record beyond size_t; draw_live with a non-zero iteration[e].  A HIP failure later returns -2
 * and leaves the engine usable. */
typedef int32_t (*vmx_nested_set_stop)(void* user, int32_t run, int64_t iterations, const double* dead_lnl, const double* live_lnl);
typedef struct {
    int32_t const_hint, chunk, lanes, draw_live;
    vmx_nested_set_stop stop; void* user;
} vmx_nested_set_options;
int vmx_nested_run_many(vmx_engine* e, const vmx_nested_spec* spec, int32_t E,
                        const uint64_t* streams, const int32_t* mock_row,
                        double* live_u, double* live_lnl,
                        int64_t* iteration,
                        int32_t* status,
                        int32_t n_iterations,
                        double* dead_u, double* dead_lnl, int32_t* dead_nlive,
                        int32_t* iterations_done,
                        const vmx_nested_set_options* opt, vmx_nested_stats* stats, int64_t* per_run);
/* The same set with every run keeping the accepted points inside its threads' walks (boost_posterior for a set; the rule, pinned:
 * vega_amd/csrc/vmx_nested.h "a set of runs", boost).  The advance launch is k_ns_set_advance_phantoms: one work-group per active
 * run advances that run's threads, asks vmx_ns::phantom_of and vmx_ns::phantom_kept under the run's own stream, and writes the
 * round's kept points into the run's own part of one record [E][capacity] behind the run's own running count (a prefix scan inside
 * the work-group: nothing crosses runs, no atomic decides a place); a run whose iteration ends in that launch records first.  The
 * base runs - dead records, live points, statuses, statistics, the engine's batches - are bit for bit those of vmx_nested_run_many;
 * no likelihood row is added.  The arguments before `phantoms` are those of vmx_nested_run_many, with its checks.
 *   phantoms  fraction: as for vmx_nested_run_phantoms, the same for every run; 0 (or phantoms NULL) runs exactly
 *                       vmx_nested_run_many - its kernels, k_ns_set_advance among them - and touches nothing in the struct
 *             capacity: rows per run of the arrays below, at least n_iterations K (num_repeats - 1)
 *             u [E][capacity][n], lnl, birth [E][capacity], iteration (int64), thread, repeat [E][capacity] host: run e's kept
 *                       points in rows e capacity .. e capacity + count[e] - 1, in the order the run accepted them (sort by the
 *                       tags for the canonical order); the rows behind them, up to iterations_done[e] K (num_repeats - 1), may be
 *                       overwritten with anything
 *             count [E] host, out: the rows written per run (0 for a run that was never entered)
 *             flags, reserved: 0
 * The counts stay on the device while the set runs and come back, with the record, in the copy that brings the dead records:
 * stats->host_waits is what it is without phantoms.
 * Refused in addition (-1, the engine untouched): a fraction outside [0, 1] or NaN, a missing array, a capacity below
 * n_iterations K (num_repeats - 1), non-zero flags. */
typedef struct {
    double fraction;
    int64_t capacity;
    double* u; double* lnl; double* birth;
    int64_t* iteration; int32_t* thread; int32_t* repeat;
    int64_t* count;
    uint32_t flags, reserved;
} vmx_nested_set_phantoms;
int vmx_nested_run_many_phantoms(vmx_engine* e, const vmx_nested_spec* spec, int32_t E,
                                 const uint64_t* streams, const int32_t* mock_row,
                                 double* live_u, double* live_lnl,
                                 int64_t* iteration,
                                 int32_t* status,
                                 int32_t n_iterations,
                                 double* dead_u, double* dead_lnl, int32_t* dead_nlive,
                                 int32_t* iterations_done,
                                 const vmx_nested_set_options* opt, vmx_nested_stats* stats, int64_t* per_run,
                                 vmx_nested_set_phantoms* phantoms);
/* Evidence and an equal-weight posterior where the particles live: tempered sequential Monte Carlo (the scheme of pocoMC, the
 * reference's second sampler in bin/run_vega_mpi.py, without its normalising flow), every decision pinned in
 * vega_amd/csrc/vmx_smc.h.  N particles walk from the prior (beta = 0) to the posterior (beta = 1); a stage picks the next beta by
 * bisection on the effective sample size of the importance weights, resamples systematically, whitens with the particles'
 * covariance (k_smc_stage: one work-group per run, once per stage) and moves all particles by `sweeps` Metropolis sweeps under
 * L^beta: k_smc_move decides the sweep just evaluated, adapts the proposal scale and writes the N rows of the next one, then the
 * engine's chain runs over them in chunks of `chunk` (two lanes alternate when the quadratic form serves them).  A whole stage is
 * enqueued at once; the host waits once per stage, on a mapped word that carries beta.
 *   spec      n_params = the engine's; n sampled columns col[n] with their box [lo, hi] (finite, lo < hi: the uniform prior);
 *             N particles, sweeps per stage, 0 < ess < 1 (the ladder keeps ESS >= ess N); log_norm (lnL = log_norm - 0.5 chi2);
 *             seed / stream (the Philox key); theta_fixed[n_params], the row that supplies the columns not sampled
 *   u, lnl    [N][n] in the unit cube, [N] host: the particles, read at entry (unless opt->draw) and written back at exit;
 *             *stage the global index of the next stage, *beta its starting inverse temperature, *scale the proposal scale -
 *             all advanced by the call (a run cut into calls is the same run).  *beta >= 1: nothing is left to do.
 *   n_stages  at most so many stages; the call ends after the stage that reaches beta = 1
 *   rec, rec_lnl, rec_anc   [n_stages][VMX_SMC_REC], [n_stages][N], [n_stages][N] host: per stage beta_{t-1}, beta_t, ESS(beta_t),
 *             accepted moves, the scale after the stage, 1 if the factor is the Cholesky factor (0: the diagonal fallback), rows
 *             that were a particle's own position, moves rejected by a failed model; the lnL before reweighting; the ancestors.
 *             stats->stages rows are written
 *   opt       const_hint (-1: derived - a column varies when it is sampled), chunk (rows per engine call, 0: max_batch), lanes
 *             (0: 2), draw (nonzero: *stage must be 0; the particles are drawn from the Philox blocks (i, 0, j, 5), evaluated, and
 *             *beta = 0, *scale = 2.38 sqrt(3 / n)); NULL: -1, 0, 0, 0
 *   stats     host_waits = stages + 1 (the copy back) + 1 with draw (the start: how many particles have a finite lnL)
 * Refused before anything runs (-1, vmx_last_error, the engine untouched): n outside 1 .. 32, N outside max(2 n + 2, 8) .. 4096,
 * ess outside (0, 1), sweeps < 1, a column out of range or repeated, a non-finite limit or lo >= hi, and without draw a particle
 * outside the cube or with a NaN lnL, no particle with a finite lnL, beta outside [0, 1], a scale that is not positive.  A HIP
 * failure later returns -2 and leaves the engine usable; so does a run that cannot go on (every start particle failed, or fewer
 * than ess N particles carry weight so that beta cannot advance) - the caller's arrays are then left as they were. */
#define VMX_SMC_MAX_PARTICLES 4096
#define VMX_SMC_REC 8
typedef struct {
    int32_t n_params, n;
    const int32_t* col; const double* lo; const double* hi;
    int32_t N, sweeps;
    double ess, log_norm;
    uint64_t seed, stream;
    const double* theta_fixed;
} vmx_smc_spec;
typedef struct { int32_t const_hint, chunk, lanes, draw; } vmx_smc_options;
typedef struct {
    int64_t stages, sweeps, rows, rows_own_position, accepted, rejected_failed_model, engine_calls, host_waits;
    double seconds, seconds_enqueuing;
    int32_t const_hint, lanes;          /* what the call ran with */
} vmx_smc_stats;
int vmx_smc_run(vmx_engine* e, const vmx_smc_spec* spec, double* u, double* lnl, int64_t* stage, double* beta, double* scale,
                int32_t n_stages, double* rec, double* rec_lnl, int32_t* rec_anc, const vmx_smc_options* opt,
                vmx_smc_stats* stats);
/* E independent SMC runs advanced together: log Z and an equal-weight posterior for every Monte-Carlo mock, or the replicas of one
 * run, as one device run.  A run of N = 256 - 512 particles hands the engine one batch per sweep and stops the host once per
 * stage; here the same kernels are launched with one work-group per run still going (work-group a owns run active[a], nothing
 * crosses runs: the single run is the set of one, through one host body), the A N rows of a sweep go through the engine as one
 * stream of chunks of `chunk` on two lanes, and the host waits once per stage round for the whole set.  Run e is by construction
 * the run vmx_smc_run makes with spec->stream = streams[e] on the data of mock_row[e]; its chi2 is evaluated in batches of another
 * shape, so that its lnL may differ from the single run's in the last bits (E = 1 has the single run's batches and gives it bit
 * for bit).
 *   spec      as for the single run; spec->stream is not read
 *   E         runs (>= 1) of spec->N particles each
 *   streams   [E] the Philox stream of every run (repeats allowed: equal streams on equal data give equal runs)
 *   mock_row  [E] the row of the items' mock pools run e is compared with, 0 <= row < n_mocks of every item's pool, repeats
 *             allowed (the kernel that opens a round writes the row of every engine row); NULL: every run reads the installed data
 *   u, lnl    [E][N][n], [E][N] host: the particles, read at entry (unless opt->draw) and written back at exit
 *   stage, beta, scale   [E] each: the runs' own state, as the single run's - runs may enter at different stages and
 *             temperatures, Philox counters use the run's own stage index; a run with beta >= 1 at entry is left alone.  A set
 *             cut into calls is the same set.
 *   status    [E] out: 0 the run is still going (n_stages used up), 1 it has reached beta = 1, 2 no particle has a finite lnL, 3
 *             its ladder cannot advance (fewer than ess N particles carry weight).  A run with status 2 or 3 does not fail the
 *             call: its u / lnl / stage / beta / scale are left as they were at entry and its stages_done is 0.
 *   n_stages  at most so many stage rounds; a round advances every run still going by one stage; after each round the runs with
 *             status != 0 leave the active list (which stays in ascending run order) and the others' rows move up to A N
 *             contiguous engine rows
 *   rec, rec_lnl, rec_anc   [E][n_stages][VMX_SMC_REC], [E][n_stages][N], [E][n_stages][N] host: the record of every run as the
 *             single run writes it; stages_done[e] rows of run e are written
 *   stages_done   [E] out: the stages run e was advanced by
 *   opt       as for the single run; draw applies to every run (every stage[e] must then be 0)
 *   stats     the totals over the runs (stages: the sum of stages_done); host_waits = stage rounds + 1 (the copy back) + 1 with
 *             draw.  per_run [E][4] (NULL: not wanted): accepted moves, rows that were a particle's own position, moves rejected
 *             for a failed model (all three 0 for a failed run), rows evaluated
 * Refused before anything runs (-1, vmx_last_error, the engine untouched): whatever the single run refuses, for every run; E < 1;
 * streams NULL; a mock row that is negative or not below n_mocks; mock rows while an item has no pool; E N beyond the engine's
 * int32 row count or a record beyond size_t.  A HIP failure later returns -2 and leaves the engine usable. */
int vmx_smc_run_many(vmx_engine* e, const vmx_smc_spec* spec, int32_t E,
                     const uint64_t* streams, const int32_t* mock_row,
                     double* u, double* lnl,
                     int64_t* stage, double* beta, double* scale,
                     int32_t* status,
                     int32_t n_stages,
                     double* rec, double* rec_lnl, int32_t* rec_anc,
                     int32_t* stages_done,
                     const vmx_smc_options* opt, vmx_smc_stats* stats, int64_t* per_run);
/* Kept populations and posterior rounds (vmx_smc.h: "kept populations and posterior rounds"): the calls above with a record of the
 * positions every stage reweighted - what a weighted posterior over all stages' particles needs (vega_amd/smc.py:
 * recycled_weights) - and with further stages at beta = 1 that only whiten and move, so that a run yields more than N points.
 *   keep->rec_u         [n_stages][N][n] host ([E][n_stages][N][n] for the set), or NULL: row k is the particles at the entry of
 *                       the call's stage k - the positions of rec_lnl's row k.  It lives in the workspace beside rec_lnl and comes
 *                       back in the copy that brings the record.
 *   keep->topups_left   [1] ([E] for the set) in/out, or NULL (no round owed): the posterior rounds the run still owes.  A run
 *                       with beta >= 1 and rounds owed is not finished: its next stage is a posterior round (no bisection, no
 *                       weights, no resampling; identity ancestors; record row beta_prev = beta = 1, ESS = the particles with a
 *                       finite lnL), which pays one.  n_stages bounds ladder stages and posterior rounds together, one record row
 *                       each; the Philox stage index keeps counting, so that a run is the same however it is cut.
 *   keep->flags         0
 * keep == NULL, or rec_u == NULL with no round owed, launches the kernels of vmx_smc_run / vmx_smc_run_many; otherwise the stage
 * heads are k_smc_stage_kept (smc_stage under its KEPT flag), the sweeps k_smc_move as they are - the same kernels with one
 * work-group per run still going.  In a set, runs on the ladder and runs in posterior rounds stand side by side in one launch; a
 * run at beta = 1 that owes rounds has status 0 and stays in the active list, and gets status 1 in the round that pays its last
 * one.
 *   stats     single run: a ladder stage waits on beta as before; the posterior rounds of a call need no decision of the host and
 *             are enqueued back to back with one wait: host_waits = ladder stages + (1 if the call ran a posterior round) + 1 (the
 *             copy back) + 1 with draw.  The set keeps one wait per round: host_waits = rounds + 1 + 1 with draw.
 * Refused before anything runs (-1): whatever the base calls refuse; non-zero flags; a negative topups_left; rounds owed while
 * rec_u is NULL; a record beyond size_t.  A run entered with beta = 1 and rounds owed is accepted. */
typedef struct { double* rec_u; int32_t* topups_left; int32_t flags; } vmx_smc_keep;
int vmx_smc_run_kept(vmx_engine* e, const vmx_smc_spec* spec, double* u, double* lnl, int64_t* stage, double* beta, double* scale,
                     int32_t n_stages, double* rec, double* rec_lnl, int32_t* rec_anc, const vmx_smc_keep* keep,
                     const vmx_smc_options* opt, vmx_smc_stats* stats);
int vmx_smc_run_many_kept(vmx_engine* e, const vmx_smc_spec* spec, int32_t E,
                          const uint64_t* streams, const int32_t* mock_row,
                          double* u, double* lnl,
                          int64_t* stage, double* beta, double* scale,
                          int32_t* status,
                          int32_t n_stages,
                          double* rec, double* rec_lnl, int32_t* rec_anc,
                          int32_t* stages_done,
                          const vmx_smc_keep* keep,
                          const vmx_smc_options* opt, vmx_smc_stats* stats, int64_t* per_run);
/* The table level (vmx_set_constant_nl_hint) that batches whose rows differ only in the columns varies[n_params] != 0 allow - what
 * vmx_fit_migrad and vmx_ensemble_run derive when they are given const_hint = -1; a caller that evaluates such batches itself
 * sets it with vmx_set_constant_nl_hint. */
int vmx_derived_const_hint(vmx_engine* e, const int32_t* varies);
/* direct_pk (vega_interface.py:208-248 -> model.py:188-207): while set, every item's model is its smooth pipeline
 * (no peak component, no metals with the default no-metal-decomp; additive broadband terms enter once) evaluated with
 * the linear spectrum pk[b][nk] of walker b (host pointer, e.g. the output of a Boltzmann code per parameter point)
 * instead of the fiducial template.  pk = NULL returns to the template. */
int vmx_set_direct_pk(vmx_engine* e, const double* pk, int32_t B, int32_t nk);

/* `Model.compute(pars, pk_full, pk_smooth)` (model.py:157-187) takes the linear spectra per call: replace the
 * template's spectra (pk_peak = pk_full - pk_smooth as formed by the caller, model.py:177) after vmx_finalize.  The
 * Arinyo term keeps the fiducial Delta^2(k) of vmx_set_template (power_spectrum.py:72-73, :462).  nk must equal the
 * template's. */
int vmx_set_linear_spectra(vmx_engine* e, const double* pk_peak, const double* pk_smooth, const double* pk_full,
                           int32_t nk);

/* Small-scale marginalisation coefficients (vega_interface.py:546-579 `compute_marg_coeff`; returned by
 * chi2 / log_lik(..., return_marg_coeff=True), :282-325, which is what the PolyChord adapter calls,
 * samplers/polychord.py:106-113): coeff = M . (data - model[mask]) with the static matrix
 * M = `marg_diff2coeff_matrix` [n_templates][n_masked] (data.py:762-828).  Set before vmx_finalize;
 * vmx_marg_coeff applies it to the residuals of the LAST evaluation (B = its batch size) with the engine's product
 * kernels and copies out [B][n_templates] (host pointer; synchronous). */
int vmx_item_set_marg_matrix(vmx_engine* e, int32_t item, const double* m, int32_t n_templates, int32_t n_masked);
int vmx_marg_coeff(vmx_engine* e, int32_t item, double* out, int32_t B);
/* The same coefficients as derived columns of walkers that live in HBM - what a sampler stores beside every point
 * (samplers/polychord.py:106-113).  The residual is linear in the dx = x' - x0' that the quadratic form of chi2 contracts
 * (vmx_set_quadratic_form), so coeff = c0 - G dx with G = M S DM' [n_templates][nq] and c0 = M r0 per data vector / mock, folded
 * once when the form's tensors are built and refreshed with them (data, mock pool, reference point).  The call runs the chain up
 * to the walkers' vectors (table level of vmx_set_constant_nl_hint and the mock rows of vmx_set_mock_index honoured), then per item
 * one skinny product (split-K slabs added in fixed order) and one kernel that writes d_out[b][offset(item) + i], row-major with
 * leading dimension ld_out >= the total count; NaN in every column of a walker whose status is not 0.  No chi2, no model
 * vector, no distortion product, no residual; enqueued on the engine's stream without host synchronisation or host copy
 * (vmx_sync, vmx_stream).  Where the quadratic form does not apply (global covariance, multiplicative or non-polynomial
 * post-distortion broadband, direct_pk, the form switched off) the same call takes the full chain and applies M to its
 * residuals, still device to device.  d_status [B] may be NULL.  vmx_debug_read(what = 4)[8] reports the form the call took.
 * vmx_marg_layout: the columns of `item` (offset, count; either may be NULL; count 0 for an item without a map), items in the
 * order of vmx_add_item; returns the total number of columns (item = -1: only that). */
int vmx_marg_coeff_device(vmx_engine* e, const double* d_theta, int32_t B, double* d_out, int32_t ld_out, int32_t* d_status);
int vmx_marg_layout(vmx_engine* e, int32_t item, int32_t* offset, int32_t* count);

/* The mu sums of the P(k,mu) stage.  The reference sums P(k,mu) L_ell(mu) over 1000 midpoints in mu
 * (power_spectrum.py:76-77, pktoxi.py:138).  node_rule != 0 (the default): for wavenumbers up to 24 / (largest bin size)
 * the engine evaluates the first 48 and the last 48 of those midpoints and 82 fixed nodes in between - two 32-point
 * Gauss-Legendre panels for the integral plus ONE one-sided nine-point finite-difference stencil per end for the h^2, h^4
 * and h^6 end corrections of the Euler-Maclaurin formula - which reproduces the 1000-point sums, not the integral, to
 * <= 1e-13 of the largest k^3 P_ell over the whole parameter box of vmx_set_mu_rule_box (tests/test_mu_quadrature.py: the
 * reference's prior limits and wider, corners included); larger wavenumbers, and the model options
 * that are not smooth in mu (exponential smoothing, Voigt / sinc HCD, McDonald), keep the plain loop.  node_rule = 0:
 * the 1000-point loop everywhere (VMX_EXACT_MU in the environment does the same).  Returns the setting in effect.
 * Tiers: in the level-2 kernel (vmx_set_constant_nl_hint) a k tile whose largest wavenumber is at most 0.0058 / 0.11 h/Mpc
 * takes a 42- / 82-node rule of the same generator (4 + 4 midpoints and one 16-point panel / 16 + 16 and one 32-point panel,
 * the same stencils): there k^3 P_ell is orders of magnitude below its largest value, and each tier adds <= 1e-14 of that
 * (vega_amd/mu_quadrature.py: TIERS, tests/test_mu_tiers.py).  The choice depends on the tile alone.  VMX_NO_MU_TIERS in the
 * environment (read by vmx_set_template) keeps the main rule on every tile. */
int vmx_set_mu_quadrature(vmx_engine* e, int32_t node_rule);
/* Applicability guard of that rule (before vmx_finalize).  The rule is validated on a parameter box - the prior limits
 * of the reference's vega/parameters/default_values.txt for every parameter that shapes P(k,mu) other than polynomially,
 * widened where the tests go further (tests/test_mu_quadrature.py: >= 100 draws incl. corners, 1e-12).  A walker with
 * theta[slots[i]] outside [lo[i], hi[i]] (or NaN) is not trusted to it: its P(k,mu) blocks run the reference's 1000-point
 * loop itself, decided per walker on the device (k_prologue), so a sampler that wanders off gets slower, never different.
 * vmx_debug_read(what = 4)[7] counts such walkers since vmx_finalize.  n = 0: no guard. */
int vmx_set_mu_rule_box(vmx_engine* e, int32_t n, const int32_t* slots, const double* lo, const double* hi);
/* The extra nodes of that rule as the engine built them: mu[n], w[n] (weights in units of one midpoint); returns n
 * (also when the buffers are NULL or too small, without writing). */
int vmx_get_mu_nodes(vmx_engine* e, double* mu, double* w, int32_t capacity);

/* Lanes.  lanes = 2: chi2-only vmx_eval_device calls (model == NULL, 64 walkers or more, the quadratic form in use)
 * alternate between the engine's own per-batch workspace and a second one - a clone that BORROWS every static tensor
 * (matrices, tables, operators; no copy) and owns its workspace, its per-batch tables and its stream - so that two
 * independent batches are in flight and the kernels of one fill the partly idle first / last block rounds of the other's
 * (an ensemble sampler's half-ensembles, Monte-Carlo realisations, the nested sampler's threads: vmx_nested_run; the reference's
 * bin/run_vega_mc_mpi.py:54-65 gives every rank such independent work).  Per batch the arithmetic, and therefore every bit
 * of chi2, is that of one lane.  A call returns once its kernels are enqueued, as before; vmx_sync waits for both lanes;
 * vmx_last_stream is the stream of the last vmx_eval_device (to order a consumer after it with an event; vmx_stream stays
 * the first lane's).  Any call that changes what an evaluation computes (data, mocks, covariances, parameter transform,
 * quadrature, ...) or needs the first lane's buffers (vmx_eval, model output) waits for / retires the second lane - it is
 * re-made on demand.  lanes = 1 (the default): one batch in flight. */
int vmx_set_lanes(vmx_engine* e, int32_t lanes);
void* vmx_last_stream(vmx_engine* e);

/* chi2-only evaluations (model == NULL) as a static quadratic form.  Without a multiplicative post-distortion
 * broadband the model on the fitted bins is linear in x' = [pre-distortion vector ; additive post-distortion broadband
 * coefficients], model = S DM' x' (model.py:143-149), so
 *     chi2 = r0^T C^-1 r0 - 2 dx^T (DM'^T S^T C^-1 r0) + dx^T (DM'^T S^T C^-1 S DM') dx,   dx = x' - x0',  r0 = data - S DM' x0'
 * with ONE static symmetric matrix per item in place of the distortion product (model.py:143-144) and the C^-1 product
 * (vega_interface.py:316): about half the matrix work of an evaluation, identical results to rounding.  theta_ref
 * [n_params] is the expansion point (x0' = its vector; any point the model can be evaluated at - the configured
 * parameter values - keeps the three terms small next to the signal); NULL switches the form off.  The tensors are
 * built with the engine's own kernels at the next chi2-only evaluation and refreshed when data, mocks or inverse
 * covariances change.  Not used with a global covariance, a multiplicative or non-polynomial post-distortion
 * broadband, direct_pk, or when a model output is requested (those run the full chain).  Returns 1 when the
 * configuration is eligible, 0 when it is not (the call is then a no-op). */
int vmx_set_quadratic_form(vmx_engine* e, const double* theta_ref);
/* Which form of that quadratic form the chi2-only evaluations take.  With C^-1 = U^T U (the library factors the inverse
 * covariance it was given) the same chi2 is || U r0 - F dx ||^2 with the static F = U S DM' [n_masked][nq]: 2 n_masked nq flops per
 * walker instead of the nq^2 of the half-form Q'.  kind = 0 (default): the cheaper one per engine - Q' for model grids that are the
 * data grid (2500 / 5000 bins against 1590 / 3180 fitted ones), the factored form when the model grid is much finer (a
 * `distortion-file` with COEFMOD >= 2, reference vega/data.py:441-473: nq = 10 000 against 1590); 1: Q'; 2: the factored form.
 * The two agree to rounding (the sum of squares has no cancellation at all); vmx_debug_read(what = 4)[8] reports the form the last
 * evaluation took (0: full chain, 1: Q', 2: factored).  After vmx_finalize; the tensors are rebuilt at the next chi2-only call.
 * Within the Q' form, batches of more than 8 walkers may take the quadratic term alone as || L dx ||^2 from a lower-trapezoidal
 * root L [n_masked][nq] of Q' (Householder reflectors on F, built at set-up when n_masked < nq makes it the cheaper product);
 * linear term, constants and the reported form stay those of Q'.  VMX_NO_QUAD_ROOT=1 keeps the half-triangle contraction. */
int vmx_set_quadratic_form_kind(vmx_engine* e, int32_t kind);

/* Samplers usually keep the Arinyo non-linear parameters fixed.  When they are identical for every walker of a
 * batch the factor D_NL(k,mu) G(k,mu) is tabulated once per batch instead of being exponentiated per walker and
 * grid point (level 1).  When the parameters of every Gaussian factor - smoothing (power_spectrum.py:526-556), peak
 * broadening (:382-417), Gaussian velocity dispersion (:504-524) - are shared as well, those factors join the table and a
 * second table serves the peak component (level 2): the HCD term is then the only exponential left per walker and
 * (k, mu).  A table is kept across evaluations while its parameters do not change.  vmx_eval (host theta) detects the
 * level by itself; for vmx_eval_device the caller states it here: enabled = 0 none, 1 level 1, 2 level 2.
 * A walker whose table parameters differ from the first walker's while the hint is on gets
 * status VMX_STATUS_NOT_CONSTANT and chi2 = 1e100 - never a silently wrong value. */
int vmx_set_constant_nl_hint(vmx_engine* e, int32_t enabled);
/* The engine's HIP stream (hipStream_t as an opaque pointer), so that a caller can order its own work - e.g. an
 * RCCL collective on the chi2 buffer - after vmx_eval_device without a host synchronisation. */
void* vmx_stream(vmx_engine* e);

/* Stage taps for parity tests: copy an internal buffer of the last evaluation to the host.
 * what: 0 = P_ell(k) [n_ell_max][B*n_columns][nk_pad] (vmx_pipeline_column); 1 = xi per pipeline [B][n] (index = pipeline);
 * 2 = spline coefficients; 3 = metal correlation after its metal matrix [B][pad32(n_model)] (index = metal, in the
 * global order of vmx_item_add_metal).
 * 4 = {live wavenumbers of the P(k,mu) stage in the last evaluation, k up to which the mu node rule applies (0: off),
 * nodes per wavenumber of that rule (the mean over the wavenumbers on it, where k tiles took shorter tiers), leading wavenumbers whose tiles took the rule in the last evaluation, table level of
 * the last evaluation (vmx_set_constant_nl_hint), first and last spline-coefficient row the last evaluation's bins read,
 * walkers that left the mu rule's box since vmx_finalize, form of the last evaluation (vmx_set_quadratic_form_kind)}.
 * 5 = the assembled pre-distortion vector [B][pad32(n_model)] of item `index` as the last full-chain evaluation handed it to
 * the distortion product (refused after a chi2-only evaluation and after a single walker's fused product, which keeps none).
 * 4 has one more entry, [9]: the bins kernels the last evaluation launched, a mask of VMX_ROUTE_* (kept with a captured chain,
 * so it holds for a replayed graph too; VMX_ROUTE_POLY_BINS says what set-up launched).
 * And [10]: the form the FFTLog o spline product (coefficients = operator x P_ell) of the last evaluation took, a mask of
 * VMX_FFT_* with the streaming kernel's columns per pass above VMX_FFT_NB_SHIFT (kept with a captured chain like [9]; 0: the
 * evaluation had no such product).  The table level and the nodes per wavenumber ([4], [2]) are those of the evaluation itself
 * as well, replayed graph or not.
 * The operands of the spline-bins stage, for an oracle that starts where the kernels start (host-side copies, no kernel):
 * 6 = the walkers' scalars [B][n_pipelines][VMX_DEBUG_NS] of the last evaluation; 7 = where the entries the bins read sit in
 * such a row: {VMX_DEBUG_NS, then the indices in the order of VMX_DEBUG_SCALARS};
 * 8 = the per-bin static arrays of pipeline `index` as uploaded, [8][n]: r, r_par, r_perp, z, rel z, ln rel z (std::log on the
 * host: read it, do not recompute it), ln rel z of the second tracer, growth;
 * 9 = the spline grid: {n_coef, ncp, same_grid, extrapolate, n_columns (pipelines with a column of per-walker coefficients), then per ell (4): x0, h, inv_h, xlast}, and of pipeline
 * `index`: {column (-1: none), n, n_pad, split_evol, static basis (-1: none), static bins (1: PipeDev::poly_bins_off >= 0),
 * odd_x0, odd_h, odd_ncoef};
 * 10 = x' - x0' of item `index` after a chi2-only evaluation [B][nq_pad]; 11 = its x0' [nq_pad];
 * 12 = the static basis on the bins of pipeline `index` [3][n_pad] (refused for a pipeline without: "none").
 * 13 = the groups of lean pipelines whose bins arrive pre-summed: {groups, then of group `index`: members, n, n_pad, presum, per
 * member (pipeline, factor kind 0: 1, 1: theta[factor index], 2: the metal pair's bias product, factor index)} - {groups} alone
 * for an index outside; 14 = the pre-summed array [B][n_pad] of group `index` after an evaluation that summed on the way.
 * 18, 19 = the same for the groups of static-coordinate pipelines; 15 = the static coefficient basis
 * [n_ell_max][n_static][3][ncp] (a pipeline's place: the static basis of tap 9); 16 = the odd-multipole coefficient rows
 * [4][odd_ncoef] of pipeline `index`; 17 = the metal pairs' walker factors [B][3][n_metals] (bias product x multiplicity,
 * beta1 + beta2, beta1 beta2) of the last evaluation.
 * 4 [11] = 1 when the last Q' evaluation took its quadratic term from the trapezoidal root of Q' (below), 0 otherwise.
 * 20 = that root of item `index`, L [n_masked][nq_pad] with L^T L = Q' and L[i][j] = 0 for j > i + nq - n_masked; 21 = Q' itself in
 * half form [nq][nq_pad] (below the diagonal, half the diagonal on it) - "none" for an engine that holds no such tensor.
 * Returns the number of doubles written (<= capacity) or a negative error. */
int64_t vmx_debug_read(vmx_engine* e, int32_t what, int32_t index, double* out, int64_t capacity);
#define VMX_DEBUG_NS 40
#define VMX_DEBUG_SCALARS(X) X(AP) X(AT) X(DRP) X(EV1A) X(EV1B) X(EV2A) X(EV2B) X(BIAS1) X(BB1) X(BIAS2) X(BB2) \
                             X(RAD_S) X(RAD_A) X(RAD_L) X(RAD_D) X(RAD_IL) X(RAD_ID)
enum { VMX_ROUTE_GENERAL = 1,            /* k_xi_bins<false> */
       VMX_ROUTE_STATIC_TAPS = 2,        /* k_xi_bins<true> */
       VMX_ROUTE_STATIC = 4,             /* k_xi_bins_static */
       VMX_ROUTE_STATIC_NW = 8,          /* k_xi_bins_static_nw<4> */
       VMX_ROUTE_LEAN = 16,              /* k_xi_bins_lean<2, .> */
       VMX_ROUTE_GROUP = 32,             /* k_xi_bins_group<2, .> */
       VMX_ROUTE_STATIC_GROUP = 64,      /* k_xi_bins_static_group<2> */
       VMX_ROUTE_ASSEMBLE_QUAD = 128,    /* k_xi_assemble_quad */
       VMX_ROUTE_ASSEMBLE_QUAD_GENERAL = 256,    /* ... with an item on its general branch (not a plain pair) */
       VMX_ROUTE_QUAD_PLAIN = 512,       /* k_xi_quad_plain<2, .> */
       VMX_ROUTE_SAME_GRID = 1024,       /* the SAME = true instantiations (one ln r grid for every multipole) */
       VMX_ROUTE_POLY_BINS = 2048 };     /* set-up ran k_poly_bins */
enum { VMX_FFT_GEMV1 = 1,               /* k_gemv1: a single column, x in LDS */
       VMX_FFT_GEMV = 2,                /* k_gemv<NB>: at most 8 columns, NB = (mask >> VMX_FFT_NB_SHIFT) of them per pass */
       VMX_FFT_MFMA64 = 4,              /* k_gemm_nt44<KC_FFTLOG>: 64 x 64 tiles, two buffers */
       VMX_FFT_MFMA32 = 8,              /* k_gemm_nt44<KC_FFTLOG, 2, 32>: 64 x 32 tiles */
       VMX_FFT_RING = 16,               /* k_gemm_nt44<KC_FFTLOG, 4>: 64 x 64 tiles, four-buffer ring */
       VMX_FFT_BATCH_X = 32,            /* MFMA forms: the multipoles folded into grid.x ... */
       VMX_FFT_BATCH_Y = 64,            /* ... or in grid.y (the streaming kernels keep them in grid.z: neither bit) */
       VMX_FFT_K_LIMIT = 128,           /* the kernel was handed the device column limit (live wavenumbers, tap 4 [0]) */
       VMX_FFT_NB_SHIFT = 8 };
/* The device math functions of the kernels, elementwise on host arrays (a trivial kernel of its own; for tests against
 * extended precision): which = 0 vmx_log, 1 vmx_exp, 2 vmx_rsqrt.  x [n] -> out [n]. */
int vmx_debug_math(vmx_engine* e, int32_t which, const double* x, int64_t n, double* out);
/* A process-wide debug switch (tests): while on != 0, device scratch of plain doubles that a call takes without clearing it is
 * filled with 0xFF bytes - NaN doubles - when it is allocated and at every call that finds it large enough from an earlier one,
 * so that a read of what no writer of the call covered shows as NaN in the call's outputs.  Buffers that are uploaded whole,
 * hold integers or carry structs are left alone.  Off (the default) nothing is filled and no call differs.  Returns the
 * switch as it was. */
int vmx_debug_poison_scratch(int on);

/* Stand-alone distortion-style product y[b] = A x[b] through the same kernels the evaluation
 * uses (bench / roofline measurement of the distortion-matrix step).  d_A row-major [rows][cols] with
 * cols a multiple of 32 (zero padded), d_x [B][cols], d_y [B][pad32(rows)], all device pointers (B <= 8 streams
 * the matrix once; larger B takes the MFMA path, split-K partial sums added in fixed order);
 * enqueued on the engine stream.  On the MFMA path both operands must stay below 4 GiB (the kernel addresses them with
 * 32-bit byte offsets): larger ones are refused before anything is launched.  The same limit holds for the distortion,
 * metal and inverse-covariance matrices of vmx_item_set_matrix and for the matrices of the quadratic form. */
int vmx_matvec_device(vmx_engine* e, const double* d_A, int32_t rows, int32_t cols,
                      const double* d_x, int32_t B, double* d_y);

/* Host-pointer convenience around the same product: Y[b] = A X[b] for row-major host arrays A [rows][cols],
 * X [B][cols], Y [B][rows] (padding, upload and download inside; synchronous).  Used once per Monte-Carlo run for
 * mock = fiducial + cholesky(C) . randn (data.py:751-753) on all mocks at once. */
int vmx_matmul_host(vmx_engine* e, const double* A, int32_t rows, int32_t cols, const double* X, int32_t B,
                    double* Y);

/* Restrict the event pairs of vmx_set_profiling to the kernel classes whose bit (1 << class index, the index
 * vmx_kernel_name enumerates) is set: timing one class perturbs a timed run far less than timing all of them.
 * vmx_set_profiling(e, 1) resets the mask to all classes.  Bits 28-31 of a mask other than 0xffffffff hold a sampling
 * stride minus one: n > 0 times every (n + 1)-th launch of the selected classes only (an event pair costs the queue a few
 * microseconds - several per cent of a 0.3 ms step when one sits in every step). */
int vmx_set_profiling_mask(vmx_engine* e, uint32_t kernel_class_mask);

/* Per-kernel timing with HIP events on the engine stream.  When enabled every kernel launch of
 * vmx_eval* is bracketed by events; vmx_get_timings returns the accumulated milliseconds and
 * launch counts per kernel class since the last reset. */
#define VMX_N_KERNELS 13
int vmx_set_profiling(vmx_engine* e, int32_t enabled);
int vmx_get_timings(vmx_engine* e, double* ms, int64_t* launches, int32_t reset);
const char* vmx_kernel_name(int32_t kernel_class);

#ifdef __cplusplus
}
#endif
#endif /* VEGAMX_H */
