// libvegamx.so - host side of the C ABI declared in include/vegamx.h (gfx950 only).
//
// One engine handle owns one HIP device, one stream, the static tensors (template grids, G(k)
// tables, FFTLog+spline operators, coordinates, distortion / metal / inverse-covariance matrices)
// and a per-batch workspace sized at vmx_finalize.  vmx_eval* enqueues the kernel chain of
// vmx_device.h on the engine stream.
#include "vmx_device.h"
#include "vmx_fit.h"
#include "vmx_ensemble.h"
#include "vmx_nested.h"
#include "vmx_smc.h"
#include "vmx_chain.h"
#include "vmx_chain_select.h"
#include "vmx_chain_weighted.h"

#include <atomic>
#include <cmath>
#include <chrono>
#include <thread>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <queue>
#include <utility>
#include <string>
#include <vector>

#ifndef VMX_MAX_LANES
#define VMX_MAX_LANES 2             // (three lanes measured at the end of round 4 with an experiment build: no gain over two)
#endif

static thread_local std::string g_err;

const char* vmx_last_error(void) { return g_err.c_str(); }

static int fail(int code, const std::string& msg) { g_err = msg; return code; }

#define HIP_OK(call)                                                                         \
    do {                                                                                     \
        hipError_t err__ = (call);                                                           \
        if (err__ != hipSuccess)                                                             \
            return fail(-2, std::string(#call) + ": " + hipGetErrorString(err__));           \
    } while (0)

#define REQUIRE(cond, msg)                                                                   \
    do { if (!(cond)) return fail(-1, std::string("invalid argument: ") + msg); } while (0)

namespace {

static const uint64_t VMX_PART_SENTINEL = 0x7ff8dead0000beefull;      // a NaN payload no arithmetic produces (k_gemv1 MODE 2 slots)


enum KernelClass {
    KC_PROLOGUE = 0, KC_PK, KC_FFTLOG, KC_XI, KC_METAL, KC_ASSEMBLE, KC_DISTORTION, KC_POST,
    KC_INVCOV, KC_CHI2, KC_MATVEC, KC_OTHER, KC_QUAD
};
const char* kKernelNames[VMX_N_KERNELS] = {
    "prologue", "pk_multipoles", "fftlog_spline_product", "xi_bins", "metal_matrix_product",
    "assemble", "distortion_product", "post", "invcov_product", "chi2", "matvec_api", "other",
    "quadratic_form_product"};

// vmx_debug_poison_scratch: with the switch on, device scratch of plain doubles that is taken without being cleared - alloc(count,
// false) and every ensure() - is filled with 0xFF bytes (NaN doubles), so that a read of what no writer of the call covered shows
// in the call's outputs.  Off (the default): no fill, no launch, nothing else differs.
static std::atomic<int> g_poison_scratch{0};

// The fill of the whole buffer, ordered by two device-wide waits: the first ends whatever an earlier call may still have in
// flight on any stream (every driver ends in a host wait already, so it finds nothing), the second ends the fill before the
// caller enqueues the call's first use on whichever stream it takes.  Integer buffers are never filled: a poisoned index would
// be an address.
template <typename T>
static int poison_fill(T*, size_t) { return 0; }
static int poison_fill(double* p, size_t count)
{
    if (!g_poison_scratch.load(std::memory_order_relaxed) || !p) return 0;
    hipError_t err = hipDeviceSynchronize();
    if (err == hipSuccess) err = hipMemset(p, 0xFF, count * sizeof(double));
    if (err == hipSuccess) err = hipDeviceSynchronize();
    if (err != hipSuccess) return fail(-2, std::string("poison fill: ") + hipGetErrorString(err));
    return 0;
}

template <typename T>
struct DevBuf {
    T* p = nullptr;
    size_t n = 0;
    bool borrowed = false;      // a copy of a DevBuf is a non-owning view (the second lane of an engine shares the static tensors)
    DevBuf() = default;
    DevBuf(const DevBuf& o) : p(o.p), n(o.n), borrowed(true) {}
    DevBuf& operator=(const DevBuf& o) { if (this != &o) { release(); p = o.p; n = o.n; borrowed = true; } return *this; }
    void forget() { if (borrowed) { p = nullptr; n = 0; borrowed = false; } }
    // room for `count` elements as hipMalloc hands it out (never poisoned: for buffers that are overwritten whole, or carry structs)
    int alloc_raw(size_t count) {
        release();
        if (count == 0) count = 1;
        hipError_t err = hipMalloc((void**)&p, count * sizeof(T));
        if (err != hipSuccess) return fail(-2, std::string("hipMalloc: ") + hipGetErrorString(err));
        n = count;
        return 0;
    }
    int alloc(size_t count, bool zero = true) {
        if (alloc_raw(count)) return -2;
        if (zero) {
            hipError_t err = hipMemset(p, 0, n * sizeof(T));
            if (err != hipSuccess) return fail(-2, std::string("hipMemset: ") + hipGetErrorString(err));
            return 0;
        }
        return poison_fill(p, n);
    }
    int upload(const T* host, size_t count) {
        if (alloc_raw(count)) return -2;        // (exempt from poison: the copy overwrites the whole buffer)
        hipError_t err = hipMemcpy(p, host, count * sizeof(T), hipMemcpyHostToDevice);
        if (err != hipSuccess) return fail(-2, std::string("hipMemcpy: ") + hipGetErrorString(err));
        return 0;
    }
    void release() { if (p && !borrowed) (void)hipFree(p); p = nullptr; n = 0; borrowed = false; }
    ~DevBuf() { release(); }
};

// dense row-major [rows][cols] host matrix -> device [rows][ld] with zero padded columns
static int upload_padded(DevBuf<double>& buf, const double* host, int rows, int cols, int ld)
{
    if (buf.alloc((size_t)rows * ld, true)) return -2;
    hipError_t err = hipMemcpy2D(buf.p, (size_t)ld * sizeof(double), host, (size_t)cols * sizeof(double),
                                 (size_t)cols * sizeof(double), rows, hipMemcpyHostToDevice);
    if (err != hipSuccess) return fail(-2, std::string("hipMemcpy2D: ") + hipGetErrorString(err));
    return 0;
}

// Inverse covariances are stored in "half form": L[i][j] = (C[i][j] + C[j][i]) / 2 below the diagonal, C[i][i] / 2 on
// it and 0 above, so that r^T C^-1 r = 2 r^T (L r) exactly in exact arithmetic - the product then needs the lower
// triangle only (half the flops, and half the bytes for a single walker).
static std::vector<double> half_form(const double* c, int n)
{
    std::vector<double> out((size_t)n * n, 0.0);
    for (int i = 0; i < n; ++i) {
        for (int j = 0; j < i; ++j) out[(size_t)i * n + j] = 0.5 * (c[(size_t)i * n + j] + c[(size_t)j * n + i]);
        out[(size_t)i * n + i] = 0.5 * c[(size_t)i * n + i];
    }
    return out;
}

struct MetalHost {
    MetalDev dev{};
    DevBuf<double> mat, svec, basis, kron_a, kron_b;
    int rows = 0, cols = 0;
};

struct ItemHost {
    ItemDev dev{};
    std::vector<MetalHost*> metals;
    DevBuf<double> dm, cinv, data, vec, dist, res, z, mock_pool, add_vec;
    DevBuf<double> marg, marg_out;      // marg_diff2coeff matrix [n_templates][n_masked_pad], coefficients [max_batch][pad]
    // quadratic form of chi2 (vmx_device.h): W = DM'^T S^T C^-1 [nq][n_masked_pad] is kept so that new data / mocks only
    // redo the linear terms
    DevBuf<double> q_mat, q_w, q_lin, q_c0, q_x0, q_x, q_z;
    // ... in its factored form (vmx_set_quadratic_form_kind): U with C^-1 = U^T U [n_masked][n_masked_pad], F = U S DM'
    // [n_masked][nq_pad], u0 = U r0 per data vector / mock [rows][n_masked_pad], slabs of F dx [slab_rows][n_masked_pad]
    DevBuf<double> q_u, q_f, q_u0, q_y;
    DevBuf<double> q_root;      // [n_masked][nq_pad]: lower-trapezoidal L with L^T L = Q' (quad_build), when n_masked < nq
    // marginalisation coefficients folded into that form (vmx_marg_coeff_device): G = M S DM' [n_templates][nq_pad] (static),
    // c0 = M r0 per data vector / mock [rows][pad(n_templates)], slabs of G dx (or of M . residual) [mg_rows][pad(n_templates)]
    DevBuf<double> mg_g, mg_c0, mg_y;
    // mocks made on the device (vmx_item_set_mock_factor, vmx_fit_migrad with a mock stream): Cholesky factor [n_masked][pad] and
    // fiducial [pad]; the full C^-1 and the masked reference model of the quadratic form, kept for the per-wave linear terms;
    // per-wave scratch (draws, noise, residual rows, C^-1 rows)
    DevBuf<double> mc_chol, mc_fid, q_cfull, q_m0, mc_z, mc_noise, mc_r0, mc_t;
    bool has_factor = false;
    std::vector<double> h_q_c0;         // host copy of q_c0 (the single-walker chain adds the constants on the host)
    DevBuf<int64_t> q_basis_off;
    int q_rows = 0;                     // rows of q_lin / q_c0 (1 + mocks)
    int n_templates = 0;
    int n_mocks = 0;
    DevBuf<int32_t> inv_mask;
    DevBuf<int64_t> csr_ptr; DevBuf<int32_t> csr_idx; DevBuf<double> csr_val;      // CSR distortion matrix
    int64_t csr_nnz = 0; bool has_csr = false;
    std::vector<int32_t> mask_idx;
    bool has_dm = false, has_cinv = false, has_mask = false, has_data = false;
    bool lean_pair = false;             // k_xi_quad_plain applies: plain_pair, or that but for a radiation term on the smooth component
};

// Device-resident fits (vmx_fit_migrad): buffers kept between calls, grown on demand
struct FitWorkspace {
    DevBuf<double> state;               // [F] vmx_migrad::FitStateT<N> (N: vmx_fit_migrad picks the capacity)
    DevBuf<vmx_migrad::Spec> spec;
    DevBuf<double> base, theta, chi2;
    DevBuf<int32_t> mock_row, count, offset, done, mock, status;
    DevBuf<double> ox[vmx_migrad::MAX_STAGES], oext[vmx_migrad::MAX_STAGES], oV[vmx_migrad::MAX_STAGES], ofval[vmx_migrad::MAX_STAGES], oedm[vmx_migrad::MAX_STAGES];
    DevBuf<int32_t> oflags[vmx_migrad::MAX_STAGES], oiter[vmx_migrad::MAX_STAGES];
    DevBuf<int64_t> onfcn[vmx_migrad::MAX_STAGES];
    int32_t* pin_word = nullptr; int32_t* dpin_word = nullptr;       // mapped host memory: rows of the round, fits still running
    std::vector<hipEvent_t> ev_gap;                                   // pairs around the host's turn of a round (GPU idle time)
    ~FitWorkspace() {
        if (pin_word) (void)hipHostFree(pin_word);
        for (auto& ev : ev_gap) (void)hipEventDestroy(ev);
    }
};
// (under vmx_debug_poison_scratch a buffer that is still large enough is filled too: the stale contents of an earlier, larger call)
template <typename T>
static int ensure(DevBuf<T>& b, size_t count) { return b.n >= count && b.p ? poison_fill(b.p, b.n) : b.alloc(count, false); }
// ensure() for a double buffer that carries structs (indices and counts among the doubles): exempt from poison
static int ensure_structs(DevBuf<double>& b, size_t count) { return b.n >= count && b.p ? 0 : b.alloc_raw(count); }

// What the three samplers share: the engine's rows and its answers, the fixed row and the sampled box, grown on demand
struct BoxDev {
    double* theta; const double* chi2; const int32_t* status;                   // the engine's rows [rows][P] and its answers [rows]
    const double* fixed; const int32_t* inv; const double* lo; const double* hi;    // inv[p]: sampled index of column p, or -1
};
struct BoxWorkspace {
    DevBuf<double> theta, chi2, fixed, lo, hi;
    DevBuf<int32_t> status, inv;
    // room for `rows` rows of P columns; the fixed row, the box of the n sampled columns and their places go up on `st`
    int upload(size_t rows, int P, int n, const double* h_fixed, const double* h_lo, const double* h_hi, const std::vector<int32_t>& h_inv,
               hipStream_t st, BoxDev& D)
    {
        if (ensure(theta, rows * P) || ensure(chi2, rows) || ensure(status, rows) || ensure(fixed, P) || ensure(inv, P) || ensure(lo, n) ||
            ensure(hi, n)) return -2;
        HIP_OK(hipMemcpyAsync(fixed.p, h_fixed, (size_t)P * sizeof(double), hipMemcpyHostToDevice, st));
        HIP_OK(hipMemcpyAsync(inv.p, h_inv.data(), (size_t)P * sizeof(int32_t), hipMemcpyHostToDevice, st));
        HIP_OK(hipMemcpyAsync(lo.p, h_lo, (size_t)n * sizeof(double), hipMemcpyHostToDevice, st));
        HIP_OK(hipMemcpyAsync(hi.p, h_hi, (size_t)n * sizeof(double), hipMemcpyHostToDevice, st));
        D = BoxDev{theta.p, chi2.p, status.p, fixed.p, inv.p, lo.p, hi.p};
        return 0;
    }
};

// The engine's rows out of the unit cube: the fixed row with the sampled columns mapped into the box, u(r, d) the cube coordinate
// d of row r (a lane keeps its column: what the column needs is read once, the rows go round the waves); the rows land at the
// engine's rows row0 .. row0 + rows - 1
template <int THREADS, typename U>
__device__ inline void write_cube_rows(const BoxDev& B, int P, size_t row0, int rows, U u)
{
    for (int p = threadIdx.x % 64; p < P; p += 64) {
        const int d = B.inv[p];
        const double fixed = B.fixed[p], lo = d < 0 ? 0.0 : B.lo[d], hi = d < 0 ? 0.0 : B.hi[d];
#pragma unroll 4
        for (int r = threadIdx.x / 64; r < rows; r += THREADS / 64) {
            double v = fixed;
            if (d >= 0) v = vmx_ns::map_cube(lo, hi, u(r, d));
            B.theta[(row0 + (size_t)r) * P + p] = v;
        }
    }
}
template <int THREADS, typename U>
__device__ inline void write_cube_rows(const BoxDev& B, int P, int rows, U u)
{
    write_cube_rows<THREADS>(B, P, (size_t)0, rows, u);
}

// Ensemble sampling (vmx_ensemble_run, vmx_ensemble_run_many): the walkers' state of the E ensembles, the proposals of a half and
// the chain record, grown on demand
struct EnsWorkspace {
    BoxWorkspace box;
    DevBuf<double> x, lnl, prop, factor, chain, chain_lnl;
    DevBuf<int64_t> acc, n_box, n_fail;
    DevBuf<int32_t> inside, col;
    DevBuf<int32_t> mock;               // the mock row of every engine row [E H], written once per call that names mocks
    DevBuf<uint64_t> streams;           // the ensembles' Philox streams [E]
    DevBuf<double> beta;                // parallel tempering: the ladder [T] (adaptive ladders: [G][T]) ...
    DevBuf<int64_t> swaps;              // ... and the call's swap counters [G][T - 1][2]
    DevBuf<double> beta_hist;           // adaptive ladders: the ladders after every sweep of the call [sweeps][G][T] ...
    DevBuf<int64_t> adapt_skipped;      // ... and the sweeps whose adjustment the guard dropped [G]
    DevBuf<int64_t> cov_fallbacks;      // the covariance move: the half-steps of the call whose factor fell back to the diagonal [E]
    // ensemble slice sampling (vmx_ensemble_run_slice), sized once per (E, W, n): the active half's machines [E][H] and directions
    // [E][H][n], the walkers' rows and the rows' walkers [E][H], the scales [E], the counts [E][8] and the open step's expansions
    // and contractions [E][2], the half-steps done [E], whether a half is open [E], the running list and its counts [E]
    DevBuf<vmx_ens::SliceWalker> sl_wk;
    DevBuf<double> sl_eta, sl_mu;
    DevBuf<int32_t> sl_slot, sl_row, sl_open, sl_active, sl_count, sl_mock_row;
    DevBuf<int64_t> sl_counts, sl_step, sl_q;
    // mapped host memory: the round's total; per ensemble its requests of the round; the running list (pinned)
    int32_t* pin_word = nullptr; int32_t* dpin_word = nullptr; int32_t* pin_count = nullptr; int32_t* dpin_count = nullptr;
    int32_t* pin_active = nullptr; size_t pin_runs = 0;
    ~EnsWorkspace() {
        if (pin_word) (void)hipHostFree(pin_word);
        if (pin_count) (void)hipHostFree(pin_count);
        if (pin_active) (void)hipHostFree(pin_active);
    }
};

struct EnsDev {
    double* x; double* lnl; int64_t* acc; int64_t* n_box; int64_t* n_fail;      // [E][W][n], [E][W], [E][W] x 3
    double* prop; double* factor; int32_t* inside;                              // the active half's proposals [E][H][n], [E][H] x 2
    BoxDev box;                                                                 // rows [E H][P]: ensemble e's at [e H, (e + 1) H)
    const int32_t* col;                                                         // (a walker writes its own row: the sampled columns listed)
    double* chain; double* chain_lnl;                                           // [E][rows][W][n], [E][rows][W] (nullptr: not kept)
    const uint64_t* streams;                                                    // [E]
    int64_t rows;                                                               // chain rows of this call, per ensemble
    int32_t W, n, P, thin;
    double a, log_norm;
    uint64_t seed;
    int64_t step0;
};

// The moves of vmx_ensemble_run_many_moves as the kernel reads them: the thresholds of the mixture and the moves' scales
struct EnsMovesDev { double t0, t1, gamma0, sigma, gamma_s; };

// Parallel tempering (vmx_ensemble_run_pt; vmx_ensemble.h, "parallel tempering"): G ladders of T rungs are G T ensembles, ensemble
// g T + t on the rung of beta[t].  What the kernels read beside EnsDev: the ladder and the call's swap counters.
struct EnsPtDev {
    const double* beta;                 // [T], or [G][T] with the ladder stride T
    int64_t* swaps;                     // [G][T - 1][2]: proposed, accepted
    int32_t T;
    int32_t stride;                     // ladder g reads beta + g stride: 0, the ladder all share; T, a ladder of its own
};
enum { ENS_PT_DECIDE = 1, ENS_PT_RECORD = 2, ENS_PT_PROPOSE = 4 };

// The covariance move (vmx_ensemble_run_many_cov; vmx_ensemble.h, the sixth part) as k_ens_half_cov reads it beside EnsMovesDev:
// the third threshold, the scale gamma_c and the call's fallback counters
struct EnsCovDev { double t2, scale; int64_t* fallbacks; };     // fallbacks [E]

// The factor of a half in LDS: C [n][ld], ld = n | 1 - an odd row stride, so that the threads of a Cholesky column, which read
// rows i, i + 1, ... at the same k, fall on different banks (with ld = 64 all of them would fall on one) - the mean, the
// covariance's diagonal for the fallback, and whether every pivot was positive.  n^2 + 3 n doubles at most: 34.3 KB at n = 64.
struct EnsCovLds {
    double C[VMX_ENS_MAXN * (VMX_ENS_MAXN + 1)];
    double mean[VMX_ENS_MAXN], diag[VMX_ENS_MAXN];
    int good;
};
__device__ __forceinline__ int ens_cov_ld(int n) { return n | 1; }

// The factor stage: the work-group computes vmx_ens::half_factor of the half c[H][n] into L, every entry by exactly one thread
// with the pinned function of that entry, so that the result is the serial one bit for bit.  Means: a thread per column.
// Covariance: a thread per entry of the lower triangle, strided by the block.  Cholesky: column by column in place; thread 0 takes
// the pivot, the entries below it go to different threads; a barrier after the pivot, one after the column.  A pivot that is not
// positive is written to LDS and read by all threads after the barrier: they leave the loop together, and write the diagonal
// fallback.  Returns whether the factor is the Cholesky factor; L is complete and visible to the block on return.
__device__ __forceinline__ bool ens_factor_stage(EnsCovLds& L, const double* c, int H, int n)
{
    const int ld = ens_cov_ld(n), entries = n * (n + 1) / 2;
    for (int a = threadIdx.x; a < n; a += blockDim.x) L.mean[a] = vmx_ens::half_mean_entry(a, c, H, n);
    if (threadIdx.x == 0) L.good = 1;
    __syncthreads();
    for (int q = threadIdx.x; q < entries; q += blockDim.x) {
        int a, b;
        vmx_ens::tri_entry(q, a, b);
        const double v = vmx_ens::half_cov_entry(a, b, c, L.mean, H, n);
        L.C[a * ld + b] = v;
        if (a == b) L.diag[a] = v;
    }
    __syncthreads();
    for (int j = 0; j < n; ++j) {
        if (threadIdx.x == 0) {
            const double s = vmx_ens::chol_pivot(j, L.C, ld);
            if (s > 0.0) L.C[j * ld + j] = sqrt(s);
            else L.good = 0;
        }
        __syncthreads();
        if (!L.good) break;         // (the same word for every thread, written before the barrier and not again)
        const double piv = L.C[j * ld + j];
        for (int i = j + 1 + threadIdx.x; i < n; i += blockDim.x) L.C[i * ld + j] = vmx_ens::chol_entry(i, j, L.C, ld, piv);
        __syncthreads();
    }
    const bool good = L.good != 0;
    if (!good)
        for (int q = threadIdx.x; q < entries; q += blockDim.x) {
            int a, b;
            vmx_ens::tri_entry(q, a, b);
            L.C[a * ld + b] = a == b ? vmx_ens::fallback_entry(L.diag[a]) : 0.0;
        }
    __syncthreads();
    return good;
}

// One half-step of the sampler, the body of the three kernels below.  A grid of E work-groups: work-group e owns ensemble e
// (partners read the half decided just before, a dependency across the whole ensemble; nothing crosses ensembles, so
// __syncthreads() is the only barrier) under the Philox stream streams[e].  Decide the proposals of half h_dec at step s_dec
// (s_dec < 0: none), record the chain row when step s_dec is complete and due, then propose half h_prop at step s_prop
// (s_prop < 0: none) and write the engine's rows, so that the E H proposal rows of a half-step are one stream of chunks for the
// engine.  Every loop strides by the block, so that the chain does not depend on the block size.  Every expression: vmx_ensemble.h.
//   MOVES: the move of every walker is drawn from a mixture of the stretch, differential-evolution and snooker moves
// (vmx_ensemble.h, "the differential-evolution and snooker moves") with a Philox block of its own; without, no block is drawn and
// the move is the stretch move.  The decision does not know the move: the proposal left its factor and whether it is inside.  The
// partners' rows - up to three distinct walkers - are read from the half decided just before; the snooker move passes three times
// over the n columns of its four rows.
//   PT: the rung's beta is in the decision (accept_tempered); without, no beta is read.
//   `what` names the parts to run: all three between two half-steps without a sweep; with a sweep due, ENS_PT_DECIDE alone, then
// k_ens_swap, then ENS_PT_RECORD | ENS_PT_PROPOSE, so that the row of step s_dec and the next proposals see the walkers after the
// swaps.
//   COV (with MOVES): the mixture has the covariance move as its fourth member.  Between the barrier that follows the decision
// and the propose loop the work-group computes the factor of the other half into Lc (ens_factor_stage), and thread 0 counts a
// fallback; a walker that draws the move writes its variates into its proposal row and multiplies them by the factor in place.
constexpr int ENS_THREADS = 1024;
template <bool MOVES, bool PT, bool COV>
__device__ __forceinline__ void ens_half(const EnsDev& D, const EnsMovesDev& M, const EnsPtDev& Pt, const EnsCovDev& Cv,
                                         EnsCovLds* Lc, int64_t s_dec, int h_dec, int64_t s_prop, int h_prop, int what)
{
    static_assert(!COV || (MOVES && !PT), "the covariance move: a member of the mixture, untempered");
    const int W = D.W, H = W / 2, n = D.n;
    const size_t e = blockIdx.x;
    const uint64_t stream = D.streams[e];
    const double beta = PT ? Pt.beta[(e / (size_t)Pt.T) * (size_t)Pt.stride + e % (size_t)Pt.T] : 1.0;
    double* const x = D.x + e * W * n;
    double* const lnl = D.lnl + e * W;
    int64_t* const acc = D.acc + e * W;
    int64_t* const n_box = D.n_box + e * W;
    int64_t* const n_fail = D.n_fail + e * W;
    double* const prop = D.prop + e * H * n;
    double* const factor = D.factor + e * H;
    int32_t* const inside_of = D.inside + e * H;
    const double* const chi2 = D.box.chi2 + e * H;
    const int32_t* const status = D.box.status + e * H;
    double* const theta = D.box.theta + e * H * D.P;
    if (s_dec >= 0) {
        if (what & ENS_PT_DECIDE)
            for (int k = threadIdx.x; k < H; k += blockDim.x) {
                const int w = h_dec * H + k;
                const vmx_ens::Block b = vmx_ens::step_block(k, s_dec, h_dec, D.seed, stream);
                const double c2 = chi2[k];
                const bool inside = inside_of[k] != 0, ok = vmx_ens::model_ok(status[k], c2);
                const double lnl_new = vmx_ens::log_lik(D.log_norm, c2);
                if (PT ? vmx_ens::accept_tempered(inside, ok, factor[k], beta, lnl_new, lnl[w], b.w[2])
                       : vmx_ens::accept(inside, ok, factor[k], lnl_new, lnl[w], b.w[2])) {
                    for (int d = 0; d < n; ++d) x[(size_t)w * n + d] = prop[(size_t)k * n + d];
                    lnl[w] = lnl_new;
                    acc[w] += 1;
                } else if (!inside) n_box[w] += 1;
                else if (!ok) n_fail[w] += 1;
            }
        if ((what & ENS_PT_RECORD) && h_dec == 1 && (s_dec + 1) % D.thin == 0 && (D.chain || D.chain_lnl)) {
            __syncthreads();
            const size_t r = e * D.rows + (size_t)((s_dec + 1) / D.thin - D.step0 / D.thin - 1);
            if (D.chain)
                for (int q = threadIdx.x; q < W * n; q += blockDim.x) D.chain[r * W * n + q] = x[q];
            if (D.chain_lnl)
                for (int q = threadIdx.x; q < W; q += blockDim.x) D.chain_lnl[r * W + q] = lnl[q];
        }
    }
    if (s_prop < 0 || !(what & ENS_PT_PROPOSE)) return;
    __syncthreads();            // (the partners of the next half are the walkers just decided)
    const double* const other = x + (size_t)(1 - h_prop) * H * n;
    if (COV) {
        // (the entry refuses a cov weight with H < 2)
        const bool good = ens_factor_stage(*Lc, other, H, n);
        if (threadIdx.x == 0 && !good) Cv.fallbacks[e] += 1;
    }
    for (int k = threadIdx.x; k < H; k += blockDim.x) {
        const int w = h_prop * H + k;
        const vmx_ens::Block b = vmx_ens::step_block(k, s_prop, h_prop, D.seed, stream);
        const vmx_ens::Block m = MOVES ? vmx_ens::move_block(k, s_prop, h_prop, D.seed, stream) : vmx_ens::Block{};
        const int move = COV ? vmx_ens::move_choice4(m.w[0], M.t0, M.t1, Cv.t2)
                             : (MOVES ? vmx_ens::move_choice(m.w[0], M.t0, M.t1) : (int)vmx_ens::MOVE_STRETCH);
        const int64_t j1 = vmx_ens::partner(b.w[0], H);
        const double* c1 = other + (size_t)j1 * n;
        const double* s = x + (size_t)w * n;
        double* y = prop + (size_t)k * n;
        double f = 0.0;
        bool in = true;
        if (move == vmx_ens::MOVE_STRETCH) {
            const double z = vmx_ens::stretch_z(D.a, b.w[1]);
            for (int d = 0; d < n; ++d) y[d] = vmx_ens::propose(c1[d], s[d], z);
            f = vmx_ens::log_factor(n, z);
        } else if (COV && move == vmx_ens::MOVE_COV) {
            vmx_ens::cov_variates(n, k, s_prop, h_prop, D.seed, stream, y);
            vmx_ens::cov_propose(n, s, Lc->C, ens_cov_ld(n), Cv.scale, y);
        } else {
            // (the entry refuses a DE weight with H < 2 and a snooker weight with H < 3: the indices below are in range)
            const int64_t j2 = vmx_ens::partner2(b.w[1], H, j1);
            const double* c2 = other + (size_t)j2 * n;
            if (move == vmx_ens::MOVE_DE) {
                const double gamma = vmx_ens::de_gamma(M.gamma0, M.sigma, m.w[1], m.w[2]);
                for (int d = 0; d < n; ++d) y[d] = vmx_ens::de_propose(s[d], c1[d], c2[d], gamma);
            } else {
                const int64_t j3 = vmx_ens::partner3(b.w[3], H, j1, j2);
                in = vmx_ens::snooker_propose(n, s, c1, c2, other + (size_t)j3 * n, M.gamma_s, y, f);
            }
        }
        for (int d = 0; d < n; ++d) in = in && y[d] >= D.box.lo[d] && y[d] <= D.box.hi[d];
        factor[k] = f;
        inside_of[k] = in ? 1 : 0;
        // (a proposal outside the box is rejected whatever the model says: the engine evaluates the walker's own position)
        double* row = theta + (size_t)k * D.P;
        for (int p = 0; p < D.P; ++p) row[p] = D.box.fixed[p];
        for (int d = 0; d < n; ++d) row[D.col[d]] = in ? y[d] : s[d];
    }
}

// The default path (vmx_ensemble_run, vmx_ensemble_run_many): the stretch move, the untempered decision, all three parts
__global__ __launch_bounds__(ENS_THREADS) void k_ens_half(EnsDev D, int64_t s_dec, int h_dec, int64_t s_prop, int h_prop)
{
    ens_half<false, false, false>(D, EnsMovesDev{}, EnsPtDev{}, EnsCovDev{}, nullptr, s_dec, h_dec, s_prop, h_prop, ENS_PT_DECIDE | ENS_PT_RECORD | ENS_PT_PROPOSE);
}

// The mixture of moves (vmx_ensemble_run_many_moves), the untempered decision, all three parts
__global__ __launch_bounds__(ENS_THREADS) void k_ens_half_moves(EnsDev D, EnsMovesDev M, int64_t s_dec, int h_dec, int64_t s_prop,
                                                                int h_prop)
{
    ens_half<true, false, false>(D, M, EnsPtDev{}, EnsCovDev{}, nullptr, s_dec, h_dec, s_prop, h_prop, ENS_PT_DECIDE | ENS_PT_RECORD | ENS_PT_PROPOSE);
}

// A ladder's half-step (vmx_ensemble_run_pt, vmx_ensemble_run_pt_adapt): the parts that `what` names.  A run without moves comes
// with the thresholds of the pure stretch move (t0 = t1 = 1: the chain of k_ens_half).
__global__ __launch_bounds__(ENS_THREADS) void k_ens_half_pt(EnsDev D, EnsMovesDev M, EnsPtDev Pt, int64_t s_dec, int h_dec,
                                                             int64_t s_prop, int h_prop, int what)
{
    ens_half<true, true, false>(D, M, Pt, EnsCovDev{}, nullptr, s_dec, h_dec, s_prop, h_prop, what);
}

// The mixture with the covariance move (vmx_ensemble_run_many_cov), the untempered decision, all three parts
__global__ __launch_bounds__(ENS_THREADS) void k_ens_half_cov(EnsDev D, EnsMovesDev M, EnsCovDev Cv, int64_t s_dec, int h_dec,
                                                              int64_t s_prop, int h_prop)
{
    __shared__ EnsCovLds L;
    ens_half<true, false, true>(D, M, EnsPtDev{}, Cv, &L, s_dec, h_dec, s_prop, h_prop, ENS_PT_DECIDE | ENS_PT_RECORD | ENS_PT_PROPOSE);
}

// The factor stage alone (vmx_ensemble_cov_factor): work-group e factors the half x[e][H][n] and writes mean[e][n], the factor
// [e][n][n] with its strict upper triangle 0, and flag[e] - 1 the Cholesky factor, 0 the diagonal fallback
__global__ __launch_bounds__(ENS_THREADS) void k_ens_cov_factor(const double* x, int H, int n, double* mean, double* factor, int32_t* flag)
{
    __shared__ EnsCovLds L;
    const size_t e = blockIdx.x;
    const bool good = ens_factor_stage(L, x + e * H * n, H, n);
    const int ld = ens_cov_ld(n);
    for (int a = threadIdx.x; a < n; a += blockDim.x) mean[e * n + a] = L.mean[a];
    for (int q = threadIdx.x; q < n * n; q += blockDim.x) {
        const int a = q / n, b = q % n;
        factor[e * n * n + q] = b <= a ? L.C[a * ld + b] : 0.0;
    }
    if (threadIdx.x == 0) flag[e] = good ? 1 : 0;
}

// The swap sweep after global step s: one work-group per ladder (nothing crosses ladders, so __syncthreads() between the T - 1
// pairs of rungs is the only barrier), the pairs of rungs from the hottest down.  The threads stride over the W pairs of walkers
// of a pair of rungs; the rotation makes them disjoint, so a thread reads and writes its own two rows alone.  No likelihood row:
// lnL is stored untempered.  Every expression: vmx_ensemble.h.
//   ens_swap_pairs: the pairs of (rung t - 1, rung t) of ladder g that the calling thread owns, decided with the betas bc (cold)
// and bh (hot) and exchanged, rows and lnL; returns how many it swapped.  The callers keep the barriers and the counts.
__device__ __forceinline__ unsigned int ens_swap_pairs(const EnsDev& D, size_t g, int T, int t, double bc, double bh, int64_t s,
                                                       uint64_t stream)
{
    const int W = D.W, n = D.n;
    const size_t cold = g * T + (size_t)(t - 1), hot = cold + 1;
    double* const xc = D.x + cold * W * n;
    double* const xh = D.x + hot * W * n;
    double* const lc = D.lnl + cold * W;
    double* const lh = D.lnl + hot * W;
    const int64_t r = vmx_ens::swap_shift(vmx_ens::shift_block(s, t, D.seed, stream).w[0], W);
    unsigned int took = 0;
    for (int k = threadIdx.x; k < W; k += blockDim.x) {
        const int64_t j = vmx_ens::swap_partner(k, r, W);
        const vmx_ens::Block b = vmx_ens::swap_block(k, s, t, D.seed, stream);
        const double l_cold = lc[k], l_hot = lh[j];
        if (vmx_ens::swap_accept(bc, bh, l_cold, l_hot, b.w[0])) {
            double* pc = xc + (size_t)k * n;
            double* ph = xh + (size_t)j * n;
            for (int d = 0; d < n; ++d) { const double v = pc[d]; pc[d] = ph[d]; ph[d] = v; }
            lc[k] = l_hot;
            lh[j] = l_cold;
            took += 1;
        }
    }
    return took;
}

__global__ __launch_bounds__(ENS_THREADS) void k_ens_swap(EnsDev D, EnsPtDev Pt, int64_t s)
{
    const int W = D.W, T = Pt.T;
    const size_t g = blockIdx.x;
    const uint64_t stream = D.streams[g * T];
    int64_t* const swaps = Pt.swaps + g * (size_t)(T - 1) * 2;
    for (int t = T - 1; t >= 1; --t) {
        const unsigned long long took = ens_swap_pairs(D, g, T, t, Pt.beta[t - 1], Pt.beta[t], s, stream);
        if (took) atomicAdd((unsigned long long*)&swaps[2 * (t - 1) + 1], took);
        if (threadIdx.x == 0) swaps[2 * (t - 1)] += W;
        __syncthreads();        // (rung t - 1 is the hot rung of the next pair)
    }
}

// Adaptive ladders (vmx_ensemble_run_pt_adapt; vmx_ensemble.h, the fourth part): what k_ens_swap_adapt reads beside EnsPtDev
struct EnsAdaptDev {
    double* beta;                       // [G][T]: the ladders, which the kernel moves (Pt.beta reads the same array)
    double* hist;                       // [sweeps of the call][G][T]: the ladders after every sweep (nullptr: not kept)
    int64_t* skipped;                   // [G]: the sweeps whose adjustment the guard dropped
    double lag, tau;
    int64_t sweep0;                     // the sweeps before the call's first step
    int32_t swap_every, G;
};

// k_ens_swap over ladders of their own that move: the same grid - one work-group per ladder - the same pairs, rotation, swap rule
// and counters.  The ladder is read into LDS once, so that every pair of the sweep decides with the old ladder; the sweep's accepted
// swaps per pair of rungs are gathered in LDS by integer atomics (order-independent; W may exceed the block).  After the barrier
// behind the last pair one thread runs ladder_adjust - at most T - 2 = 62 exponentials - and writes the ladder, the history row and
// the guard's count; the k_ens_half_pt(record | propose) that follows on the stream decides with the new betas.  `adapt` 0: a
// sweep past adapt_until, which moves nothing.
__global__ __launch_bounds__(ENS_THREADS) void k_ens_swap_adapt(EnsDev D, EnsPtDev Pt, EnsAdaptDev A, int64_t s, int adapt)
{
    __shared__ double beta[vmx_ens::PT_MAXT];
    __shared__ unsigned int took_of[vmx_ens::PT_MAXT];
    const int W = D.W, T = Pt.T;
    const size_t g = blockIdx.x;
    const uint64_t stream = D.streams[g * T];
    int64_t* const swaps = Pt.swaps + g * (size_t)(T - 1) * 2;
    double* const ladder = A.beta + g * (size_t)T;
    for (int t = threadIdx.x; t < T; t += blockDim.x) { beta[t] = ladder[t]; took_of[t] = 0u; }
    __syncthreads();
    for (int t = T - 1; t >= 1; --t) {
        const unsigned int took = ens_swap_pairs(D, g, T, t, beta[t - 1], beta[t], s, stream);
        if (took) atomicAdd(&took_of[t - 1], took);
        __syncthreads();        // (rung t - 1 is the hot rung of the next pair; the pair's count is whole)
        if (threadIdx.x == 0) {
            swaps[2 * (t - 1)] += W;
            swaps[2 * (t - 1) + 1] += (int64_t)took_of[t - 1];
        }
    }
    if (threadIdx.x != 0) return;
    const int64_t time = vmx_ens::sweep_time(s, A.swap_every);
    if (adapt) {
        if (!vmx_ens::ladder_adjust(beta, took_of, T, (int64_t)W, time, A.lag, A.tau)) A.skipped[g] += 1;
        for (int t = 1; t + 1 < T; ++t) ladder[t] = beta[t];
    }
    if (A.hist) {
        double* const row = A.hist + ((size_t)(time - A.sweep0) * (size_t)A.G + g) * (size_t)T;
        for (int t = 0; t < T; ++t) row[t] = beta[t];
    }
}

// Ensemble slice sampling (vmx_ensemble_run_slice; vmx_ensemble.h, the fifth part): what the two kernels of a round read beside
// EnsDev (its prop / factor / inside / n_box / n_fail are not used).  Ensemble e's parts of the per-walker arrays start at e H.
struct EnsSliceDev {
    vmx_ens::SliceWalker* wk;           // [E][H] the machines of the active half
    double* eta;                        // [E][H][n] their directions
    int32_t* slot;                      // [E][H] the engine row of a walker's request (k_ens_slice_emit makes it global)
    int32_t* row_walker;                // [E][H] the walker of an ensemble's r-th request
    double* mu;                         // [E] the scales, in and out
    int64_t* counts;                    // [E][SLICE_COUNTS]
    int64_t* step_counts;               // [E][2] expansions and contractions of the step that is open
    int64_t* q;                         // [E] half-steps done in this call
    int32_t* open;                      // [E] a half is open: its machines hold requests
    const int32_t* active;              // [A] the ensembles still running, ascending
    int32_t* count;                     // [A] the requests of ensemble active[a] in this round
    int32_t* host_count;                // [E] mapped: the same per ensemble
    int32_t* host_word;                 // mapped: the round's total
    const int32_t* mock_row;            // [E] the pool row of every ensemble, or nullptr
    int32_t* mock;                      // the mock row of every engine row
    int32_t A, n_steps, tune_steps, max_e, max_c;
};

// One pass over the walkers of the active half h of step s of ensemble e: OPEN, every walker opens its update; else every walker
// with a request out takes the answer of its row.  Either way the machines settle and the requesting walkers are numbered in
// walker order (a ballot per wave, the waves' counts through LDS; the lanes stride beyond the block): slot[k] the walker's place
// among the ensemble's requests, row_walker the inverse.  Returns the ensemble's requests.  Every expression: vmx_ensemble.h.
template <bool OPEN>
__device__ __forceinline__ int ens_slice_pass(const EnsDev& D, const EnsSliceDev& S, size_t e, int64_t s, int h, double mu, int32_t* s_wave)
{
    const int W = D.W, H = W / 2, n = D.n;
    const uint64_t stream = D.streams[e];
    const double* const x = D.x + e * W * n + (size_t)h * H * n;
    const double* const lnl = D.lnl + e * W + (size_t)h * H;
    const double* const other = D.x + e * W * n + (size_t)(1 - h) * H * n;
    vmx_ens::SliceWalker* const wk = S.wk + e * H;
    double* const eta = S.eta + e * H * n;
    int32_t* const slot = S.slot + e * H;
    int32_t* const row_walker = S.row_walker + e * H;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, waves = (blockDim.x + 63) >> 6;
    int total = 0;
    for (int base = 0; base < H; base += blockDim.x) {
        const int k = base + threadIdx.x;
        int asks = 0;
        if (k < H) {
            vmx_ens::SliceWalker w;
            if (OPEN) {
                vmx_ens::slice_open(w, eta + (size_t)k * n, n, x + (size_t)k * n, lnl[k], other, H, mu, D.box.lo, D.box.hi, S.max_e,
                                    S.max_c, k, s, h, D.seed, stream);
                wk[k] = w;
            } else {
                w = wk[k];
                if (w.asks) {
                    const int row = slot[k];
                    vmx_ens::slice_advance(w, n, x + (size_t)k * n, eta + (size_t)k * n, D.box.lo, D.box.hi, D.log_norm,
                                           D.box.status[row], D.box.chi2[row], S.max_e, S.max_c, k, s, h, D.seed, stream);
                    wk[k] = w;
                }
            }
            asks = w.asks;
        }
        const unsigned long long m = __ballot(asks);
        if (lane == 0) s_wave[wave] = __popcll(m);
        __syncthreads();
        int before = 0, all = 0;
        for (int i = 0; i < waves; ++i) { const int c = s_wave[i]; before += i < wave ? c : 0; all += c; }
        if (asks) {
            const int local = total + before + __popcll(m & ((1ull << lane) - 1ull));
            slot[k] = local;
            row_walker[local] = k;
        }
        total += all;
        __syncthreads();        // (the waves' counts are rewritten by the next stride)
    }
    return total;
}

// a wave's sum of `mine` into the LDS word (integers: the order does not matter)
__device__ __forceinline__ void ens_slice_add(unsigned long long* word, unsigned long long mine)
{
    for (int off = 32; off > 0; off >>= 1) mine += __shfl_xor(mine, off, 64);
    if ((threadIdx.x & 63) == 0 && mine) atomicAdd(word, mine);
}

// A round of the set, first kernel: one work-group per running ensemble, one lane per walker of the active half.  Every walker
// with a request out takes its answer and the machines settle.  While the ensemble asks for nothing its half is over: the half is
// committed - positions, lnL, the moved counter, the counts (integer sums through LDS: the order does not matter) - at a step's
// end the scale is tuned while the step is below tune_steps and the chain row written when due, and unless the call's steps are
// done the next half opens.  Nothing crosses ensembles; __syncthreads() is the only barrier.  Holds 144 B of LDS.
__global__ __launch_bounds__(ENS_THREADS) void k_ens_slice_advance(EnsDev D, EnsSliceDev S)
{
    __shared__ int32_t s_wave[ENS_THREADS / 64];
    __shared__ unsigned long long s_cnt[vmx_ens::SLICE_COUNTS];
    __shared__ double s_mu;
    const int a = blockIdx.x, W = D.W, H = W / 2, n = D.n;
    const size_t e = (size_t)S.active[a];
    int64_t q = S.q[e];
    bool open = S.open[e] != 0;
    if (threadIdx.x == 0) s_mu = S.mu[e];
    __syncthreads();
    int total = 0;
    if (open) total = ens_slice_pass<false>(D, S, e, vmx_ens::slice_step(D.step0, q), vmx_ens::slice_half(q), s_mu, s_wave);
    while (total == 0) {
        if (open) {
            const int64_t s = vmx_ens::slice_step(D.step0, q);
            const int h = vmx_ens::slice_half(q);
            double* const x = D.x + e * W * n + (size_t)h * H * n;
            double* const lnl = D.lnl + e * W + (size_t)h * H;
            int64_t* const acc = D.acc + e * W + (size_t)h * H;
            if (threadIdx.x < vmx_ens::SLICE_COUNTS) s_cnt[threadIdx.x] = 0ull;
            __syncthreads();
            unsigned long long mine[vmx_ens::SLICE_COUNTS] = {0ull, 0ull, 0ull, 0ull, 0ull, 0ull, 0ull, 0ull};
            for (int k = threadIdx.x; k < H; k += blockDim.x)
                acc[k] += vmx_ens::slice_commit(S.wk[e * H + k], n, x + (size_t)k * n, S.eta + (e * H + k) * n, lnl + k, mine);
            // (every index a constant, so that the lane's counts stay in registers; a wave adds its lanes' first)
            ens_slice_add(&s_cnt[0], mine[0]); ens_slice_add(&s_cnt[1], mine[1]); ens_slice_add(&s_cnt[2], mine[2]);
            ens_slice_add(&s_cnt[3], mine[3]); ens_slice_add(&s_cnt[4], mine[4]); ens_slice_add(&s_cnt[5], mine[5]);
            ens_slice_add(&s_cnt[6], mine[6]); ens_slice_add(&s_cnt[7], mine[7]);
            __syncthreads();        // (the half is committed: the next half's partners, the chain row)
            if (threadIdx.x == 0) {
                int64_t* const counts = S.counts + e * vmx_ens::SLICE_COUNTS;
                for (int i = 0; i < vmx_ens::SLICE_COUNTS; ++i) counts[i] += (int64_t)s_cnt[i];
                int64_t* const step = S.step_counts + e * 2;
                step[0] += (int64_t)s_cnt[vmx_ens::SC_EXPANSIONS];
                step[1] += (int64_t)s_cnt[vmx_ens::SC_CONTRACTIONS];
                if (h == 1) {
                    if (vmx_ens::slice_tune_due(s, S.tune_steps)) s_mu = vmx_ens::slice_tune(s_mu, step[0], step[1]);
                    step[0] = step[1] = 0;
                }
            }
            if (h == 1 && (s + 1) % D.thin == 0 && (D.chain || D.chain_lnl)) {
                const size_t r = e * D.rows + (size_t)((s + 1) / D.thin - D.step0 / D.thin - 1);
                const double* const xe = D.x + e * W * n;
                const double* const le = D.lnl + e * W;
                if (D.chain)
                    for (int i = threadIdx.x; i < W * n; i += blockDim.x) D.chain[r * W * n + i] = xe[i];
                if (D.chain_lnl)
                    for (int i = threadIdx.x; i < W; i += blockDim.x) D.chain_lnl[r * W + i] = le[i];
            }
            __syncthreads();        // (the scale of the next half; s_cnt is zeroed again)
            q += 1;
            open = false;
        }
        if (q >= 2 * (int64_t)S.n_steps) break;
        total = ens_slice_pass<true>(D, S, e, vmx_ens::slice_step(D.step0, q), vmx_ens::slice_half(q), s_mu, s_wave);
        open = true;
    }
    if (threadIdx.x == 0) {
        S.q[e] = q;
        S.open[e] = open ? 1 : 0;
        S.mu[e] = s_mu;
        S.count[a] = total;
    }
}

// ... second kernel, the packing: ensemble active[a] owns the engine's rows offset .. offset + count[a] - 1, offset the sum of the
// counts before it in list order (vmx_ens::slice_offsets), its requests in walker order.  Every slot becomes a global row; the
// rows are written one column per lane - the fixed row with the sampled columns at the trial point, the row's walker, trial and
// direction read once per row by the lanes of a wave; the rows' mocks, the ensemble's count and (work-group 0) the total go out.
__global__ __launch_bounds__(ENS_THREADS) void k_ens_slice_emit(EnsDev D, EnsSliceDev S)
{
    const int a = blockIdx.x, W = D.W, H = W / 2, n = D.n, P = D.P;
    const size_t e = (size_t)S.active[a];
    int offset = 0;
    for (int b = 0; b < a; ++b) offset += S.count[b];
    const int cnt = S.count[a];
    const int h = vmx_ens::slice_half(S.q[e]);
    const int32_t* const row_walker = S.row_walker + e * H;
    const vmx_ens::SliceWalker* const wk = S.wk + e * H;
    const double* const eta = S.eta + e * H * n;
    const double* const x = D.x + e * W * n + (size_t)h * H * n;
    for (int r = threadIdx.x; r < cnt; r += blockDim.x) S.slot[e * H + row_walker[r]] = offset + r;
    for (int p = threadIdx.x % 64; p < P; p += 64) {
        const int d = D.box.inv[p];
        const double fixed = D.box.fixed[p];
        for (int r = threadIdx.x / 64; r < cnt; r += blockDim.x / 64) {
            const int k = row_walker[r];
            double v = fixed;
            if (d >= 0) v = vmx_ens::slice_point(x[(size_t)k * n + d], wk[k].t, eta[(size_t)k * n + d]);
            D.box.theta[((size_t)offset + r) * P + p] = v;
        }
    }
    if (S.mock_row) {
        const int m = S.mock_row[e];
        for (int i = threadIdx.x; i < cnt; i += blockDim.x) S.mock[offset + i] = m;
    }
    if (threadIdx.x == 0) {
        S.host_count[e] = cnt;
        if (a == 0) {
            int total = 0;
            for (int b = 0; b < S.A; ++b) total += S.count[b];
            *S.host_word = total;
        }
    }
}

// Nested sampling (vmx_nested_run): live points, the threads' state machines, the rows of a round and the dead record
struct NsWorkspace {
    BoxWorkspace box;
    DevBuf<double> live_u, live_lnl, mean, cov, chol, lstar, dead_u, dead_lnl;
    DevBuf<double> th;                  // [K] vmx_ns::Thread
    DevBuf<int32_t> rank, surv, killed, slot, dead_n;
    DevBuf<int64_t> counters;
    // clustering (vmx_nested_run_clustered): ids, the neighbour lists and link levels, the survivors' and the threads' clusters
    DevBuf<int32_t> live_cluster, dead_cluster, nn, cslot, tslot, cl_id, cl_size, cl_info;
    DevBuf<uint8_t> lev;
    DevBuf<double> cl_mean, cl_cov, cl_chol;
    // boost (vmx_nested_run_phantoms): the call's phantom record and its running count
    DevBuf<double> ph_u, ph_lnl, ph_birth;
    DevBuf<int64_t> ph_it, ph_count;
    DevBuf<int32_t> ph_thread, ph_repeat, ph_cluster;
    int32_t info_host[4] = {0, 0, 0, 0};                             // what goes up into cl_info (it outlives the copy)
    int32_t* pin_word = nullptr; int32_t* dpin_word = nullptr;       // mapped host memory: rows of the round
    double* pin_lnl = nullptr; double* dpin_lnl = nullptr;           // ... and, when an iteration ends, live lnL [nlive] + dead lnL [K]
    size_t pin_lnl_n = 0;
    // a set of runs (vmx_nested_run_many): the lists and the iterations done [3][E] (pinned, and on the device), the counts of the
    // round per list entry and per run (mapped), streams, first iterations and mocks
    DevBuf<int32_t> set_ctl, set_count, mock_row, mock;
    DevBuf<uint64_t> streams;
    DevBuf<int64_t> it0;
    int32_t* set_host = nullptr; int32_t* pin_count = nullptr; int32_t* dpin_count = nullptr; size_t set_runs = 0;
    ~NsWorkspace() {
        if (pin_word) (void)hipHostFree(pin_word);
        if (pin_lnl) (void)hipHostFree(pin_lnl);
        if (set_host) (void)hipHostFree(set_host);
        if (pin_count) (void)hipHostFree(pin_count);
    }
};

// The clustering of m points (vmx_nested.h "clustering"): position p is row row_of(surv, p) of u and of ids
struct NsClusterDev {
    const double* u; const int32_t* surv;                   // [rows][n], [m] (nullptr: the rows themselves)
    int32_t* ids;                                           // [rows]: the previous ids in, the new ones out
    int32_t* nn; uint8_t* lev; int32_t* slot;               // [m][KNN] neighbours and their link levels, [m] the cluster of every point
    int32_t* cl_id; int32_t* cl_size; int32_t* info;        // [MAX_CLUSTERS] x 2; info: the level used, the cluster count, next_id
    double* mean; double* cov; double* chol;                // [MAX_CLUSTERS] x [n], [n][n], [n][n]
    int32_t m, n;
};

struct NsDev {
    double* live_u; double* live_lnl;                       // [nlive][n], [nlive]
    int32_t* rank; int32_t* surv; int32_t* killed;          // [nlive], [nlive - K], [K]
    double* mean; double* cov; double* chol; double* lstar; // [n], [n][n], [n][n], [1]
    vmx_ns::Thread* th; int32_t* slot;                      // [K]: the machines, and the row of each one's last request (-1: none)
    double* dead_u; double* dead_lnl; int32_t* dead_n;      // the call's record [iterations][K] ([n])
    BoxDev box;
    int32_t* host_word; double* host_lnl; int64_t* counters;        // counters[0]: rows that were a thread's own position
    int32_t nlive, K, n, P, num_repeats;
    double log_norm;
    uint64_t seed, stream;
};

// what a run with clustering hands its kernels beside NsDev (the kernels of a run without it take NsDev alone, as they did):
// cl.ids is live_cluster [nlive]; the record's ids [iterations][K]; the cluster of every thread's start [K]
struct NsClusterRun {
    NsClusterDev cl; int32_t* dead_cluster; int32_t* tslot;
    int32_t phase;                                          // k_ns_iteration_clustered: 0 the kill, 1 (after the clustering) the starts
};

// what a run that keeps phantom points hands its advance kernel beside NsDev (vmx_nested.h "boost"): the call's record
// [capacity] ([n]), the rows written so far, the kept fraction
struct NsPhantomRun {
    double* u; double* lnl; double* birth;
    int64_t* iteration; int32_t* thread; int32_t* repeat; int32_t* cluster;     // cluster: with clustering only
    int64_t* count;
    int64_t capacity;
    double fraction;
};

constexpr int NS_THREADS = 1024;
constexpr int NS_KNN_THREADS = 256;

// The KNN nearest others of every point, one point per lane with its coordinates in registers: the points stream through LDS in
// tiles of NS_KNN_THREADS x NP doubles (NP >= n, the rest zeros, which add +0.0 to a sum that is never negative: the bits of
// vmx_ns::dist2 over n).  Every lane reads the same tile entry at the same time - a broadcast, no bank conflict - and keeps its
// sorted list by insertion; (d2, position) is a total order, so the lists do not depend on the tiling.
template <int NP>
__global__ __launch_bounds__(NS_KNN_THREADS) void k_ns_knn(NsClusterDev C)
{
    __shared__ double tile[NS_KNN_THREADS * NP];
    const int m = C.m, n = C.n;
    const int i = blockIdx.x * NS_KNN_THREADS + threadIdx.x;
    double x[NP], d[vmx_ns::KNN];
    int32_t p[vmx_ns::KNN];
#pragma unroll
    for (int a = 0; a < NP; ++a) x[a] = (i < m && a < n) ? C.u[(size_t)vmx_ns::row_of(C.surv, i) * n + a] : 0.0;
#pragma unroll
    for (int s = 0; s < vmx_ns::KNN; ++s) { d[s] = INFINITY; p[s] = vmx_ns::NO_NEIGHBOUR; }
    for (int j0 = 0; j0 < m; j0 += NS_KNN_THREADS) {
        const int count = min(NS_KNN_THREADS, m - j0);
        __syncthreads();
        for (int e = threadIdx.x; e < count * NP; e += NS_KNN_THREADS) {
            const int j = e / NP, a = e % NP;
            tile[e] = a < n ? C.u[(size_t)vmx_ns::row_of(C.surv, j0 + j) * n + a] : 0.0;
        }
        __syncthreads();
        if (i >= m) continue;
        for (int j = 0; j < count; ++j) {
            const double d2 = vmx_ns::dist2(x, tile + j * NP, NP);
            if (j0 + j != i) vmx_ns::nn_insert(d, p, d2, j0 + j);
        }
    }
    if (i < m) {
#pragma unroll
        for (int s = 0; s < vmx_ns::KNN; ++s) C.nn[(size_t)i * vmx_ns::KNN + s] = p[s] == vmx_ns::NO_NEIGHBOUR ? -1 : p[s];
    }
}

// Neighbour lists to factors in one work-group: link levels, min-label propagation with pointer jumping to its fixed point (which
// no schedule changes; at most m sweeps per level, levels 2 .. KNN), sizes and the order of the sizeable components, the loose
// points to their nearest clustered one, the ids, then mean and covariance with one lane per (cluster, entry) and the factor with
// one lane per cluster.  Every decision: vmx_nested.h.
__global__ __launch_bounds__(NS_THREADS) void k_ns_cluster(NsClusterDev C)
{
    __shared__ int32_t s_lab[vmx_ns::MAX_LIVE];             // labels; later the previous ids
    __shared__ int32_t s_size[vmx_ns::MAX_LIVE];            // component sizes; later every point's cluster
    __shared__ int32_t s_slot0[vmx_ns::MAX_LIVE];           // the cluster of a point of a sizeable component, -1: loose
    __shared__ int32_t s_flag, s_count, s_root[vmx_ns::MAX_CLUSTERS], s_csize[vmx_ns::MAX_CLUSTERS], s_cid[vmx_ns::MAX_CLUSTERS];
    __shared__ unsigned long long s_best[vmx_ns::MAX_CLUSTERS];
    constexpr int KNN = vmx_ns::KNN, MAXC = vmx_ns::MAX_CLUSTERS;
    const int m = C.m, n = C.n, tid = threadIdx.x;
    volatile int32_t* lab = s_lab;
    for (int e = tid; e < m * KNN; e += NS_THREADS) C.lev[e] = (uint8_t)vmx_ns::link_level(C.nn, e / KNN, e % KNN);
    for (int i = tid; i < m; i += NS_THREADS) s_lab[i] = i;
    if (tid == 0) s_flag = 0;
    __syncthreads();
    int k = 2, before = 0;
    for (;; ++k) {
        for (int sweep = 0; sweep < m; ++sweep) {
            bool changed = false;
            for (int i = tid; i < m; i += NS_THREADS) {
                const int32_t mine = lab[i];
                int32_t l = mine;
                for (int q = 0; q < k; ++q)
                    if (C.lev[(size_t)i * KNN + q] <= k) l = min(l, lab[C.nn[(size_t)i * KNN + q]]);
                l = min(l, lab[l]);
                if (l < mine) { lab[i] = l; changed = true; }
            }
            if (changed) s_flag = 1;
            __syncthreads();
            const int again = s_flag;
            __syncthreads();
            if (tid == 0) s_flag = 0;
            __syncthreads();
            if (!again) break;
        }
        if (tid == 0) s_count = 0;
        __syncthreads();
        int roots = 0;
        for (int i = tid; i < m; i += NS_THREADS) roots += s_lab[i] == i ? 1 : 0;
        if (roots) atomicAdd(&s_count, roots);
        __syncthreads();
        const int count = s_count;
        __syncthreads();
        if ((k >= 3 && count == before) || k == KNN) break;
        before = count;
    }
    for (int i = tid; i < m; i += NS_THREADS) s_size[i] = 0;
    if (tid < MAXC) { s_root[tid] = -1; s_csize[tid] = 0; s_cid[tid] = 0; s_best[tid] = 0; }
    __syncthreads();
    for (int i = tid; i < m; i += NS_THREADS) atomicAdd(&s_size[s_lab[i]], 1);
    __syncthreads();
    const int sizeable = 2 * n + 2;
    for (int i = tid; i < m; i += NS_THREADS) {
        if (s_lab[i] != i || s_size[i] < sizeable) continue;
        int rank = 0;
        for (int r = 0; r < m; ++r)
            rank += (s_lab[r] == r && s_size[r] >= sizeable && (s_size[r] > s_size[i] || (s_size[r] == s_size[i] && r < i))) ? 1 : 0;
        if (rank < MAXC) s_root[rank] = i;
    }
    __syncthreads();
    int nc = 0;
    for (int c = 0; c < MAXC; ++c) nc += s_root[c] >= 0 ? 1 : 0;
    for (int i = tid; i < m; i += NS_THREADS) {
        int32_t c0 = nc == 0 ? 0 : -1;
        for (int c = 0; c < nc; ++c)
            if (s_lab[i] == s_root[c]) c0 = c;
        s_slot0[i] = c0;
    }
    if (nc == 0) nc = 1;
    __syncthreads();
    int32_t* s_slot = s_size;
    int32_t* s_prev = s_lab;
    for (int i = tid; i < m; i += NS_THREADS) {
        int32_t c = s_slot0[i];
        if (c < 0) {
            const double* x = C.u + (size_t)vmx_ns::row_of(C.surv, i) * n;
            double bd = INFINITY;
            int32_t bp = vmx_ns::NO_NEIGHBOUR;
            for (int j = 0; j < m; ++j) {
                if (s_slot0[j] < 0) continue;
                const double d2 = vmx_ns::dist2(x, C.u + (size_t)vmx_ns::row_of(C.surv, j) * n, n);
                if (vmx_ns::nearer(d2, j, bd, bp)) { bd = d2; bp = j; }
            }
            c = s_slot0[bp];
        }
        s_slot[i] = c;
        C.slot[i] = c;
        s_prev[i] = C.ids[vmx_ns::row_of(C.surv, i)];
        atomicAdd(&s_csize[c], 1);
    }
    __syncthreads();
    for (int i = tid; i < m; i += NS_THREADS) {
        const int32_t id = s_prev[i], c = s_slot[i];
        if (id == 0) continue;
        int32_t same = 0;
        for (int j = 0; j < m; ++j) same += (s_slot[j] == c && s_prev[j] == id) ? 1 : 0;
        atomicMax(&s_best[c], (unsigned long long)vmx_ns::id_key(same, id));
    }
    __syncthreads();
    if (tid == 0) {
        uint64_t best[MAXC];
        int32_t ids[MAXC], next = C.info[2];
        for (int c = 0; c < MAXC; ++c) { best[c] = s_best[c]; ids[c] = 0; }
        vmx_ns::assign_ids(nc, best, &next, ids);
        for (int c = 0; c < MAXC; ++c) { s_cid[c] = ids[c]; C.cl_id[c] = ids[c]; C.cl_size[c] = s_csize[c]; }
        C.info[0] = k; C.info[1] = nc; C.info[2] = next;
    }
    __syncthreads();
    for (int i = tid; i < m; i += NS_THREADS) C.ids[vmx_ns::row_of(C.surv, i)] = s_cid[s_slot[i]];
    for (int e = tid; e < nc * n; e += NS_THREADS) {
        const int c = e / n, a = e % n;
        C.mean[e] = vmx_ns::cluster_mean_entry(a, C.u, C.surv, s_slot, m, c, s_csize[c], n);
    }
    __syncthreads();
    for (int e = tid; e < nc * n * n; e += NS_THREADS) {
        const int c = e / (n * n), a = e % (n * n) / n, b = e % n;
        if (b > a) continue;
        const double v = vmx_ns::cluster_cov_entry(a, b, C.u, C.surv, s_slot, C.mean + (size_t)c * n, m, c, s_csize[c], n);
        C.cov[(size_t)c * n * n + a * n + b] = v;
        C.cov[(size_t)c * n * n + b * n + a] = v;
    }
    __syncthreads();
    if (tid < nc) (void)vmx_ns::whiten(n, C.cov + (size_t)tid * n * n, C.chol + (size_t)tid * n * n);
}

// the initial live points: u from the Philox blocks (i, 0, j, 2), and their rows for the engine
__global__ __launch_bounds__(NS_THREADS) void k_ns_draw_live(NsDev D)
{
    for (int i = threadIdx.x; i < D.nlive; i += blockDim.x) vmx_ns::draw_live(i, D.n, D.seed, D.stream, D.live_u + (size_t)i * D.n);
    __syncthreads();
    write_cube_rows<NS_THREADS>(D.box, D.P, D.nlive, [&](int r, int d) { return D.live_u[(size_t)r * D.n + d]; });
}

__global__ __launch_bounds__(NS_THREADS) void k_ns_live_lnl(NsDev D)
{
    for (int i = threadIdx.x; i < D.nlive; i += blockDim.x) D.live_lnl[i] = vmx_ns::lnl_of(D.box.status[i], D.box.chi2[i], D.log_norm);
}

// The head of iteration `it` (record row `rec` of this call) in one work-group: rank the live points by counting, append the K
// deaths to the record, the survivors' mean and covariance (one lane per entry), the factor (one lane: n <= 32), L*, and every
// thread at its start.  Every expression: vmx_nested.h.  CLUSTER (k_ns_iteration_clustered): two launches around k_ns_knn /
// k_ns_cluster - X.phase 0 kills, records the ids the dead held and lists the survivors; X.phase 1 starts the threads and notes the
// cluster of every start.  Without it (k_ns_iteration) X is not there and the code is what it was.
template <bool CLUSTER>
__device__ __forceinline__ void ns_iteration(const NsDev& D, const NsClusterRun& X, int64_t it, int64_t rec)
{
    __shared__ double s_lnl[vmx_ns::MAX_LIVE];
    __shared__ int32_t s_rank[vmx_ns::MAX_LIVE];
    const int nlive = D.nlive, K = D.K, n = D.n, m = nlive - K;
    if constexpr (CLUSTER) {
        if (X.phase == 1) {
            for (int k = threadIdx.x; k < K; k += blockDim.x) {
                const int64_t choice = vmx_ns::start_choice(k, it, m, D.seed, D.stream);
                const int i = D.surv[choice];
                vmx_ns::start(D.th[k], n, D.live_u + (size_t)i * n, D.live_lnl[i]);
                D.slot[k] = -1;
                X.tslot[k] = X.cl.slot[choice];
            }
            return;
        }
    }
    for (int i = threadIdx.x; i < nlive; i += blockDim.x) s_lnl[i] = D.live_lnl[i];
    __syncthreads();
    for (int i = threadIdx.x; i < nlive; i += blockDim.x) {
        const int r = vmx_ns::rank_of(i, s_lnl, nlive);
        s_rank[i] = r;
        D.rank[i] = r;
        if (r < K) {
            D.killed[r] = i;
            const size_t row = (size_t)rec * K + r;
            for (int d = 0; d < n; ++d) D.dead_u[row * n + d] = D.live_u[(size_t)i * n + d];
            D.dead_lnl[row] = s_lnl[i];
            D.dead_n[row] = nlive - r;
            if constexpr (CLUSTER) X.dead_cluster[row] = X.cl.ids[i];
            if (r == K - 1) *D.lstar = s_lnl[i];
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < nlive; i += blockDim.x) {
        if (s_rank[i] < K) continue;
        int pos = 0;
        for (int j = 0; j < i; ++j) pos += s_rank[j] >= K ? 1 : 0;
        D.surv[pos] = i;
    }
    if constexpr (CLUSTER) return;
    for (int a = threadIdx.x; a < n; a += blockDim.x) D.mean[a] = vmx_ns::mean_entry(a, D.live_u, s_rank, nlive, K, n);
    __syncthreads();
    for (int q = threadIdx.x; q < n * n; q += blockDim.x) {
        const int a = q / n, b = q % n;
        if (b > a) continue;
        const double c = vmx_ns::cov_entry(a, b, D.live_u, s_rank, D.mean, nlive, K, n);
        D.cov[a * n + b] = c;
        D.cov[b * n + a] = c;
    }
    __syncthreads();
    if (threadIdx.x == 0) (void)vmx_ns::whiten(n, D.cov, D.chol);
    for (int k = threadIdx.x; k < K; k += blockDim.x) {
        const int i = D.surv[vmx_ns::start_choice(k, it, m, D.seed, D.stream)];
        vmx_ns::start(D.th[k], n, D.live_u + (size_t)i * n, s_lnl[i]);
        D.slot[k] = -1;
    }
}

__global__ __launch_bounds__(NS_THREADS) void k_ns_iteration(NsDev D, int64_t it, int64_t rec)
{
    ns_iteration<false>(D, NsClusterRun{}, it, rec);
}

__global__ __launch_bounds__(NS_THREADS) void k_ns_iteration_clustered(NsDev D, NsClusterRun X, int64_t it, int64_t rec)
{
    ns_iteration<true>(D, X, it, rec);
}

// One answer for every thread that asked, in one work-group: lane by lane (contiguous threads per lane, so that the compaction
// keeps their order) read chi2 / status of the thread's row, advance its machine, then scan the requests of the threads still
// running and emit their rows (the fixed row with the sampled columns mapped out of the cube) and the row count to the host's
// word.  When nothing is asked for the iteration is over: the end points take the killed points' slots, and the live and the
// newly dead lnL go to the host beside the word.  CLUSTER (k_ns_advance_clustered): every thread walks with the factor of its
// start's cluster, and its end point inherits that cluster's id.  PHANTOM (k_ns_advance_phantoms, _clustered): after its advance
// every lane asks whether the call accepted a point inside the walk and whether the thinning keeps it (*keeps: one bit per thread
// of the lane, as `asks`); ns_record_phantoms writes them.  Without it the code is what it was.
template <bool CLUSTER, bool PHANTOM = false>
__device__ __forceinline__ int ns_advance_threads(const NsDev& D, const NsClusterRun& X, int64_t it, int32_t* s_scan, int32_t* s_row_thread,
                                                  double fraction = 0.0, uint32_t* keeps = nullptr)
{
    const int K = D.K, n = D.n;
    const int per = (K + NS_THREADS - 1) / NS_THREADS;
    const int k0 = threadIdx.x * per;
    vmx_ns::Iteration I{D.chol, *D.lstar, it, D.seed, D.stream, n, D.num_repeats};
    int mine = 0;
    uint32_t asks = 0;
    for (int j = 0; j < per; ++j) {
        const int k = k0 + j;
        if (k >= K) break;
        vmx_ns::Thread& T = D.th[k];
        if (T.state == vmx_ns::S_DONE) continue;
        const int row = D.slot[k];
        const double answer = row >= 0 ? vmx_ns::lnl_of(D.box.status[row], D.box.chi2[row], D.log_norm) : -INFINITY;
        if constexpr (CLUSTER) I.C = X.cl.chol + (size_t)X.tslot[k] * n * n;
        if constexpr (PHANTOM) {
            const int32_t state_before = T.state, inside_before = T.inside;
            if (vmx_ns::advance(T, I, k, answer)) { asks |= 1u << j; mine += 1; }
            const int32_t r = vmx_ns::phantom_of(state_before, inside_before, answer, I.lstar, T, I.num_repeats);
            if (r > 0 && vmx_ns::phantom_kept(k, it, r, fraction, D.seed, D.stream)) *keeps |= 1u << j;
        } else {
            if (vmx_ns::advance(T, I, k, answer)) { asks |= 1u << j; mine += 1; }
        }
    }
    s_scan[threadIdx.x] = mine;
    __syncthreads();
    for (int step = 1; step < NS_THREADS; step <<= 1) {
        const int v = threadIdx.x >= step ? s_scan[threadIdx.x - step] : 0;
        __syncthreads();
        s_scan[threadIdx.x] += v;
        __syncthreads();
    }
    const int total = s_scan[NS_THREADS - 1];
    int row = s_scan[threadIdx.x] - mine;
    int own = 0;
    for (int j = 0; j < per; ++j) {
        const int k = k0 + j;
        if (k >= K) break;
        if (asks & (1u << j)) {
            D.slot[k] = row;
            if (s_row_thread) s_row_thread[row] = k;
            own += D.th[k].inside ? 0 : 1;
            row += 1;
        } else D.slot[k] = -1;
    }
    if (own) atomicAdd((unsigned long long*)D.counters, (unsigned long long)own);
    __syncthreads();
    return total;
}

// the end of an iteration: the end points take the killed points' slots, the live and the newly dead lnL go to the host
template <bool CLUSTER>
__device__ __forceinline__ void ns_iteration_end(const NsDev& D, const NsClusterRun& X, int64_t rec)
{
    const int K = D.K, n = D.n;
    for (int k = threadIdx.x; k < K; k += blockDim.x) {
        const int i = D.killed[k];
        const vmx_ns::Thread& T = D.th[k];
        for (int d = 0; d < n; ++d) D.live_u[(size_t)i * n + d] = T.x[d];
        D.live_lnl[i] = T.lnl;
        if constexpr (CLUSTER) X.cl.ids[i] = X.cl.cl_id[X.tslot[k]];
        D.host_lnl[D.nlive + k] = D.dead_lnl[(size_t)rec * K + k];
    }
    __syncthreads();
    for (int i = threadIdx.x; i < D.nlive; i += blockDim.x) D.host_lnl[i] = D.live_lnl[i];
}

// The kept phantom points of the round (`keeps`: this lane's threads, bit j = thread k0 + j) behind the F.count rows the call has
// written: a second scan over s_scan (free again after ns_advance_threads' last barrier) places them in thread order, s_list holds
// the accepting threads, and the lanes write the record one column per lane.  A kept point's thread goes on walking: T.x is the
// accepted point, T.lnl its lnL, T.repeat its index.  The running count goes to the host beside the row count (HOST_COUNT; a set of
// runs keeps every run's count in device memory: that word is the set's total).
template <bool CLUSTER, bool HOST_COUNT = true>
__device__ __forceinline__ void ns_record_phantoms(const NsDev& D, const NsClusterRun& X, const NsPhantomRun& F, int64_t it, uint32_t keeps,
                                                   int32_t* s_scan, int32_t* s_list)
{
    const int K = D.K, n = D.n;
    const int per = (K + NS_THREADS - 1) / NS_THREADS;
    const int k0 = threadIdx.x * per;
    const int mine = __popc(keeps);
    s_scan[threadIdx.x] = mine;
    __syncthreads();
    for (int step = 1; step < NS_THREADS; step <<= 1) {
        const int v = threadIdx.x >= step ? s_scan[threadIdx.x - step] : 0;
        __syncthreads();
        s_scan[threadIdx.x] += v;
        __syncthreads();
    }
    const int total = s_scan[NS_THREADS - 1];
    const int64_t base = *F.count;
    int place = s_scan[threadIdx.x] - mine;
    for (int j = 0; j < per; ++j)
        if (keeps & (1u << j)) s_list[place++] = k0 + j;
    __syncthreads();                    // (the list is whole, and every lane has read the count)
    // (capacity >= iterations K (num_repeats - 1) was checked before the run: the guard never bites)
    const int64_t left = F.capacity > base ? F.capacity - base : 0;
    const int room = left < (int64_t)total ? (int)left : total;
    for (int e = threadIdx.x; e < room * n; e += NS_THREADS) {
        const int p = e / n, d = e % n;
        F.u[(size_t)(base + p) * n + d] = D.th[s_list[p]].x[d];
    }
    const double lstar = *D.lstar;
    for (int p = threadIdx.x; p < room; p += NS_THREADS) {
        const int k = s_list[p];
        const vmx_ns::Thread& T = D.th[k];
        const size_t row = (size_t)(base + p);
        F.lnl[row] = T.lnl;
        F.birth[row] = lstar;
        F.iteration[row] = it;
        F.thread[row] = k;
        F.repeat[row] = T.repeat;
        if constexpr (CLUSTER) F.cluster[row] = X.cl.cl_id[X.tslot[k]];
    }
    if (threadIdx.x == 0) {
        *F.count = base + total;
        if constexpr (HOST_COUNT) *(long long*)(D.host_word + 2) = (long long)(base + total);
    }
}

template <bool CLUSTER, bool PHANTOM = false>
__device__ __forceinline__ void ns_advance(const NsDev& D, const NsClusterRun& X, int64_t it, int64_t rec, const NsPhantomRun& F = NsPhantomRun{})
{
    __shared__ int32_t s_scan[NS_THREADS];
    __shared__ int32_t s_row_thread[vmx_ns::MAX_LIVE];
    int total;
    if constexpr (PHANTOM) {
        __shared__ int32_t s_phantom_thread[vmx_ns::MAX_LIVE];
        uint32_t keeps = 0;
        total = ns_advance_threads<CLUSTER, true>(D, X, it, s_scan, s_row_thread, F.fraction, &keeps);
        ns_record_phantoms<CLUSTER>(D, X, F, it, keeps, s_scan, s_phantom_thread);
    } else {
        total = ns_advance_threads<CLUSTER>(D, X, it, s_scan, s_row_thread);
    }
    write_cube_rows<NS_THREADS>(D.box, D.P, total, [&](int r, int d) {
        const vmx_ns::Thread& T = D.th[s_row_thread[r]];
        return T.inside ? T.y[d] : T.x[d];
    });
    if (total == 0) ns_iteration_end<CLUSTER>(D, X, rec);
    if (threadIdx.x == 0) *D.host_word = total;
}

__global__ __launch_bounds__(NS_THREADS) void k_ns_advance(NsDev D, int64_t it, int64_t rec)
{
    ns_advance<false>(D, NsClusterRun{}, it, rec);
}

__global__ __launch_bounds__(NS_THREADS) void k_ns_advance_clustered(NsDev D, NsClusterRun X, int64_t it, int64_t rec)
{
    ns_advance<true>(D, X, it, rec);
}

__global__ __launch_bounds__(NS_THREADS) void k_ns_advance_phantoms(NsDev D, NsPhantomRun F, int64_t it, int64_t rec)
{
    ns_advance<false, true>(D, NsClusterRun{}, it, rec, F);
}

__global__ __launch_bounds__(NS_THREADS) void k_ns_advance_phantoms_clustered(NsDev D, NsClusterRun X, NsPhantomRun F, int64_t it, int64_t rec)
{
    ns_advance<true, true>(D, X, it, rec, F);
}

// A set of runs (vmx_nested_run_many; vmx_nested.h "a set of runs"): a work-group owns one run - the functions above over that
// run's part of every array (`run0` is the view of run 0) under the stream streams[run] - and nothing crosses runs except the
// row offsets: the engine's rows are shared, a thread's slot is its global row.  Run r is at record row done[r] of the call and
// at iteration it0[r] + done[r] of its own count.
struct NsSetDev {
    NsDev run0;
    const int32_t* active;              // [A] the runs not OUT, ascending
    const int32_t* heading;             // [H] those of them whose iteration has to be headed
    const int32_t* done;                // [E] iterations done in this call
    const int64_t* it0;                 // [E] the runs' iteration at entry
    const uint64_t* streams;            // [E] Philox streams
    const int32_t* mock_row;            // [E] the pool row of every run, or nullptr
    int32_t* mock;                      // the mock row of every engine row (k_ns_set_emit / k_ns_set_draw_live write it)
    int32_t* count;                     // [A] the requests of run active[a] in this round
    int32_t* host_count;                // [E] mapped: per run its requests of the round (the draw: whether a live lnL is finite)
    int32_t rec_rows, A;                // record rows per run; the length of the active list
};

__device__ __forceinline__ NsDev ns_view(const NsSetDev& S, int run)
{
    NsDev D = S.run0;
    const size_t r = (size_t)run, nlive = (size_t)D.nlive, K = (size_t)D.K, n = (size_t)D.n, rec = (size_t)S.rec_rows * K;
    D.live_u += r * nlive * n; D.live_lnl += r * nlive; D.rank += r * nlive; D.surv += r * nlive; D.killed += r * K;
    D.mean += r * n; D.cov += r * n * n; D.chol += r * n * n; D.lstar += r;
    D.th += r * K; D.slot += r * K;
    D.dead_u += r * rec * n; D.dead_lnl += r * rec; D.dead_n += r * rec;
    D.host_lnl += r * (nlive + K); D.counters += r;
    D.stream = S.streams[r];
    return D;
}

// the initial live points of every active run, run active[a] at the engine's rows a nlive .. (a + 1) nlive - 1
__global__ __launch_bounds__(NS_THREADS) void k_ns_set_draw_live(NsSetDev S)
{
    const int run = S.active[blockIdx.x];
    const NsDev D = ns_view(S, run);
    const size_t row0 = (size_t)blockIdx.x * D.nlive;
    for (int i = threadIdx.x; i < D.nlive; i += blockDim.x) {
        vmx_ns::draw_live(i, D.n, D.seed, D.stream, D.live_u + (size_t)i * D.n);
        if (S.mock_row) S.mock[row0 + i] = S.mock_row[run];
    }
    __syncthreads();
    write_cube_rows<NS_THREADS>(D.box, D.P, row0, D.nlive, [&](int r, int d) { return D.live_u[(size_t)r * D.n + d]; });
}

// ... their lnL, and to the host whether any of a run's is finite
__global__ __launch_bounds__(NS_THREADS) void k_ns_set_live_lnl(NsSetDev S)
{
    const int run = S.active[blockIdx.x];
    const NsDev D = ns_view(S, run);
    const size_t row0 = (size_t)blockIdx.x * D.nlive;
    int finite = 0;
    for (int i = threadIdx.x; i < D.nlive; i += blockDim.x) {
        const double l = vmx_ns::lnl_of(D.box.status[row0 + i], D.box.chi2[row0 + i], D.log_norm);
        D.live_lnl[i] = l;
        finite |= l > -INFINITY ? 1 : 0;
    }
    const int any = __syncthreads_or(finite);
    if (threadIdx.x == 0) S.host_count[run] = any ? 1 : 0;
}

// the head of the next iteration of every run of the heading list: k_ns_iteration's body on that run's view
__global__ __launch_bounds__(NS_THREADS) void k_ns_set_head(NsSetDev S)
{
    const int run = S.heading[blockIdx.x];
    const NsDev D = ns_view(S, run);
    ns_iteration<false>(D, NsClusterRun{}, S.it0[run] + S.done[run], (int64_t)S.done[run]);
}

// One answer for every thread of every active run (k_ns_advance's body up to the rows): the threads' slots hold their place among
// the run's own requests, count[a] the run's requests; a run that asks for nothing ends its iteration here.  Holds 4 KB of LDS.
__global__ __launch_bounds__(NS_THREADS) void k_ns_set_advance(NsSetDev S)
{
    __shared__ int32_t s_scan[NS_THREADS];
    const int run = S.active[blockIdx.x];
    const NsDev D = ns_view(S, run);
    const int total = ns_advance_threads<false>(D, NsClusterRun{}, S.it0[run] + S.done[run], s_scan, nullptr);
    if (total == 0) ns_iteration_end<false>(D, NsClusterRun{}, (int64_t)S.done[run]);
    if (threadIdx.x == 0) S.count[blockIdx.x] = total;
}

// run `run`'s part of the set's phantom record [E][capacity] (vmx_ns::set_phantom_row) and its own running count: F is run 0's
__device__ __forceinline__ NsPhantomRun ns_phantom_view(const NsPhantomRun& F, int run, int n)
{
    NsPhantomRun G = F;
    const size_t r = (size_t)vmx_ns::set_phantom_row(run, F.capacity, 0, 0);
    G.u += r * (size_t)n; G.lnl += r; G.birth += r; G.iteration += r; G.thread += r; G.repeat += r;
    G.count += run;
    return G;
}

// k_ns_set_advance keeping the kept phantom points of the round (vmx_nested_run_many_phantoms): the advance with the PHANTOM step,
// then the placing scan and the column writes of ns_record_phantoms on the run's own part of the record behind the run's own
// count - nothing crosses runs, no atomic decides a place - and then the end of the iteration.  Holds 4 KB + 16 KB of LDS.
__global__ __launch_bounds__(NS_THREADS) void k_ns_set_advance_phantoms(NsSetDev S, NsPhantomRun F)
{
    __shared__ int32_t s_scan[NS_THREADS];
    __shared__ int32_t s_phantom_thread[vmx_ns::MAX_LIVE];
    const int run = S.active[blockIdx.x];
    const NsDev D = ns_view(S, run);
    const int64_t it = S.it0[run] + S.done[run];
    uint32_t keeps = 0;
    const int total = ns_advance_threads<false, true>(D, NsClusterRun{}, it, s_scan, nullptr, F.fraction, &keeps);
    ns_record_phantoms<false, false>(D, NsClusterRun{}, ns_phantom_view(F, run, D.n), it, keeps, s_scan, s_phantom_thread);
    if (total == 0) ns_iteration_end<false>(D, NsClusterRun{}, (int64_t)S.done[run]);
    if (threadIdx.x == 0) S.count[blockIdx.x] = total;
}

// The packing: run active[a] owns the engine's rows offset[a] .. offset[a] + count[a] - 1, offset[a] the sum of the counts before
// it in list order (vmx_ns::row_offsets), its requests in thread order.  Every slot becomes a global row, the rows and their
// mocks are written, the run's count and (work-group 0) the total go to the host.  Holds 16 KB of LDS.
__global__ __launch_bounds__(NS_THREADS) void k_ns_set_emit(NsSetDev S)
{
    __shared__ int32_t s_row_thread[vmx_ns::MAX_LIVE];
    const int a = blockIdx.x, run = S.active[a];
    const NsDev D = ns_view(S, run);
    int offset = 0;
    for (int b = 0; b < a; ++b) offset += S.count[b];
    const int cnt = S.count[a];
    for (int k = threadIdx.x; k < D.K; k += blockDim.x) {
        const int local = D.slot[k];
        if (local < 0) continue;
        s_row_thread[local] = k;
        D.slot[k] = offset + local;
    }
    __syncthreads();
    write_cube_rows<NS_THREADS>(D.box, D.P, (size_t)offset, cnt, [&](int r, int d) {
        const vmx_ns::Thread& T = D.th[s_row_thread[r]];
        return T.inside ? T.y[d] : T.x[d];
    });
    if (S.mock_row) {
        const int m = S.mock_row[run];
        for (int i = threadIdx.x; i < cnt; i += blockDim.x) S.mock[offset + i] = m;
    }
    if (threadIdx.x == 0) {
        S.host_count[run] = cnt;
        if (a == 0) {
            int total = 0;
            for (int b = 0; b < S.A; ++b) total += S.count[b];
            *D.host_word = total;
        }
    }
}

// Tempered SMC (vmx_smc_run): the particles, their proposals, the weights of a stage, the rows of a sweep and the stage record
// (rec_u: the positions every stage reweighted, for vmx_smc_run_kept / vmx_smc_run_many_kept only)
struct SmcWorkspace {
    BoxWorkspace box;
    DevBuf<double> u, lnl, u2, lnl2, w, cum, mean, cov, chol, state, prop, uacc, rec, rec_lnl, rec_u;
    DevBuf<int32_t> inside, zero, rec_anc;
    DevBuf<int64_t> counters;
    // mapped host memory [runs][4]: beta, accepted, scale of the stage, the start's count; the active list (pinned)
    double* pin = nullptr; double* dpin = nullptr; int32_t* pin_active = nullptr; size_t runs = 0;
    // the list, streams, stages and mocks of the runs on the device
    DevBuf<int32_t> active, mock_row, mock;
    DevBuf<uint64_t> streams;
    DevBuf<int64_t> stage0;
    ~SmcWorkspace()
    {
        if (pin) (void)hipHostFree(pin);
        if (pin_active) (void)hipHostFree(pin_active);
    }
};

struct SmcDev {
    double* u; double* lnl; double* u2; double* lnl2;               // [N][n], [N], and where the resampled copies are gathered
    double* w; double* cum;                                         // [N] weights at beta_t, their cumulative sums
    const int32_t* zero;                                            // [N] zeros: every particle is a "survivor" for vmx_ns::cov_entry
    double* mean; double* cov; double* chol;                        // [n], [n][n], [n][n]
    double* state;                                                  // [0] beta, [1] scale
    double* prop; double* uacc; int32_t* inside;                    // the sweep's proposals [N][n], deciding uniforms [N], in the cube [N]
    BoxDev box;                                                     // rows [N][P]
    double* rec; double* rec_lnl; int32_t* rec_anc;                 // the call's record [stages][VMX_SMC_REC], [stages][N], [stages][N]
    int64_t* counters;                                              // the stage's accepted, own-position rows, failed models
    double* host;                                                   // mapped: [0] beta_t, [1] accepted, [2] scale, [3] finite start lnL
    int32_t N, n, P, sweeps;
    double ess, log_norm;
    uint64_t seed, stream;
};

constexpr int SMC_THREADS = vmx_smc::LANES;
constexpr int SMC_PER = vmx_smc::MAX_PARTICLES / SMC_THREADS;

// the rows of the engine: from the proposal where it lies inside the cube and from the particle's own position elsewhere
__device__ inline void smc_write_rows(const SmcDev& D, bool proposals)
{
    const int n = D.n;
    write_cube_rows<SMC_THREADS>(D.box, D.P, D.N, [&](int r, int d) {
        return proposals && D.inside[r] ? D.prop[(size_t)r * n + d] : D.u[(size_t)r * n + d];
    });
}

// the start particles: u from the Philox blocks (i, 0, j, 5), beta = 0, the start scale, and their rows for the engine
__device__ __forceinline__ void smc_start(const SmcDev& D)
{
    for (int i = threadIdx.x; i < D.N; i += blockDim.x) vmx_smc::draw_start(i, D.n, D.seed, D.stream, D.u + (size_t)i * D.n);
    if (threadIdx.x == 0) { D.state[0] = 0.0; D.state[1] = vmx_smc::start_scale(D.n); }
    __syncthreads();
    smc_write_rows(D, false);
}

__device__ __forceinline__ void smc_start_lnl(const SmcDev& D)
{
    __shared__ int s_finite;
    if (threadIdx.x == 0) s_finite = 0;
    __syncthreads();
    for (int i = threadIdx.x; i < D.N; i += blockDim.x) {
        const double v = vmx_ns::lnl_of(D.box.status[i], D.box.chi2[i], D.log_norm);
        D.lnl[i] = v;
        if (v > -INFINITY) atomicAdd(&s_finite, 1);
    }
    __syncthreads();
    if (threadIdx.x == 0) D.host[3] = (double)s_finite;
}

// S1 and S2 of the weights at dbeta by vmx_smc.h's stride-halving tree: lane t holds the entries t, t + 1024 .. of the padded array
// (the tree's first levels add exactly those), the levels below 1024 run in shared memory
__device__ inline void smc_sums(double dbeta, const double (&d)[SMC_PER], int J, int W, double* s_a, double* s_b, double& s1, double& s2)
{
    VMX_NO_CONTRACT
    double a[SMC_PER], b[SMC_PER];
#pragma unroll
    for (int j = 0; j < SMC_PER; ++j) {
        const double w = j < J ? vmx_smc::weight(dbeta, d[j]) : 0.0;
        a[j] = w;
        b[j] = vmx_smc::square(w);
    }
#pragma unroll
    for (int s = SMC_PER / 2; s >= 1; s /= 2) {
        if (s < J) {
#pragma unroll
            for (int j = 0; j < s; ++j) { a[j] = a[j] + a[j + s]; b[j] = b[j] + b[j + s]; }
        }
    }
    __syncthreads();            // (the sums of the call before have been read)
    s_a[threadIdx.x] = a[0];
    s_b[threadIdx.x] = b[0];
    __syncthreads();
    for (int s = W / 2; s >= 1; s /= 2) {
        if ((int)threadIdx.x < s) {
            s_a[threadIdx.x] = s_a[threadIdx.x] + s_a[threadIdx.x + s];
            s_b[threadIdx.x] = s_b[threadIdx.x] + s_b[threadIdx.x + s];
        }
        __syncthreads();
    }
    s1 = s_a[0];
    s2 = s_b[0];
}

// the particles' mean and covariance (one lane per entry) and the factor (one lane: n <= 32) into record row `rec`
__device__ __forceinline__ void smc_precondition(const SmcDev& D, int64_t rec)
{
    const int N = D.N, n = D.n, tid = threadIdx.x;
    for (int a = tid; a < n; a += SMC_THREADS) D.mean[a] = vmx_ns::mean_entry(a, D.u, D.zero, N, 0, n);
    __syncthreads();
    for (int q = tid; q < n * n; q += SMC_THREADS) {
        const int a = q / n, b = q % n;
        if (b > a) continue;
        const double c = vmx_ns::cov_entry(a, b, D.u, D.zero, D.mean, N, 0, n);
        D.cov[a * n + b] = c;
        D.cov[b * n + a] = c;
    }
    __syncthreads();
    if (tid == 0) D.rec[(size_t)rec * VMX_SMC_REC + 5] = vmx_ns::whiten(n, D.cov, D.chol) ? 1.0 : 0.0;
}

// The head of a posterior round (vmx_smc.h: a stage entered with beta = 1): the record row (1, 1, the particles with a finite lnL),
// the lnL at entry, identity ancestors; the particles stay where they are and beta stays 1.
__device__ __forceinline__ void smc_round_head(const SmcDev& D, int64_t rec)
{
    __shared__ int s_finite;
    const int N = D.N, tid = threadIdx.x;
    if (tid == 0) s_finite = 0;
    __syncthreads();
    int c = 0;
    for (int i = tid; i < N; i += SMC_THREADS) {
        const double v = D.lnl[i];
        D.rec_lnl[(size_t)rec * N + i] = v;
        D.rec_anc[(size_t)rec * N + i] = i;
        c += v > -INFINITY ? 1 : 0;
    }
    if (c) atomicAdd(&s_finite, c);
    __syncthreads();
    if (tid == 0) {
        double* r = D.rec + (size_t)rec * VMX_SMC_REC;
        r[0] = 1.0; r[1] = 1.0; r[2] = (double)s_finite;
        D.counters[0] = 0; D.counters[1] = 0; D.counters[2] = 0;
    }
}

// The head of stage `stage` (record row `rec` of this call) in one work-group: the next beta by bisection on the effective sample
// size (every sum in the fixed order of vmx_smc.h), the record, the cumulative weights, the ancestors, the gather, the particles'
// mean and covariance (one lane per entry) and the factor (one lane: n <= 32).  beta_t goes to D.state[0]; NaN: no particle has a
// finite lnL.
// KEPT (vmx_smc_run_kept): the particles at entry go to row `rec` of rec_u [stages][N][n] first, and a stage entered with beta = 1
// is a posterior round: smc_round_head in place of everything up to the gather.
template <bool KEPT = false>
__device__ __forceinline__ void smc_stage(const SmcDev& D, int64_t stage, int64_t rec, double* rec_u = nullptr)
{
    VMX_NO_CONTRACT
    __shared__ double s_a[SMC_THREADS], s_b[SMC_THREADS];
    const int N = D.N, n = D.n, tid = threadIdx.x;
    const int M = vmx_smc::pad_pow2(N), J = M > SMC_THREADS ? M / SMC_THREADS : 1, W = M < SMC_THREADS ? M : SMC_THREADS;
    const double beta_prev = D.state[0];
    if constexpr (KEPT) {
        if (rec_u)
            for (int q = tid; q < N * n; q += SMC_THREADS) rec_u[(size_t)rec * N * n + q] = D.u[q];
        if (vmx_smc::posterior_round(beta_prev)) {
            smc_round_head(D, rec);
            __syncthreads();
            smc_precondition(D, rec);
            return;
        }
    }
    double d[SMC_PER];
    double top = -INFINITY;
#pragma unroll
    for (int j = 0; j < SMC_PER; ++j) {
        const int i = tid + j * SMC_THREADS;
        d[j] = j < J && i < N ? D.lnl[i] : -INFINITY;
        if (j < J && i < N) D.rec_lnl[(size_t)rec * N + i] = d[j];
        top = fmax(top, d[j]);
    }
    s_a[tid] = top;
    __syncthreads();
    for (int s = SMC_THREADS / 2; s >= 1; s /= 2) {
        if (tid < s) s_a[tid] = fmax(s_a[tid], s_a[tid + s]);
        __syncthreads();
    }
    top = s_a[0];
    if (top == -INFINITY) {
        if (tid == 0) { D.state[0] = NAN; D.host[0] = NAN; }
        return;
    }
#pragma unroll
    for (int j = 0; j < SMC_PER; ++j) d[j] = d[j] - top;       // (-inf stays -inf: weight 0, as the padding)

    const double target = D.ess * (double)N;
    double s1, s2, beta = 1.0;
    smc_sums(1.0 - beta_prev, d, J, W, s_a, s_b, s1, s2);
    if (!(vmx_smc::ess_of(s1, s2) >= target)) {
        double lo = beta_prev, hi = 1.0;
        for (int it = 0; it < vmx_smc::BISECTIONS; ++it) {
            const double mid = vmx_smc::midpoint(lo, hi);
            smc_sums(mid - beta_prev, d, J, W, s_a, s_b, s1, s2);
            if (vmx_smc::ess_of(s1, s2) >= target) lo = mid; else hi = mid;
        }
        beta = lo;
        smc_sums(beta - beta_prev, d, J, W, s_a, s_b, s1, s2);
    }
    const double dbeta = beta - beta_prev;
#pragma unroll
    for (int j = 0; j < SMC_PER; ++j) {
        const int i = tid + j * SMC_THREADS;
        if (j < J && i < N) D.w[i] = vmx_smc::weight(dbeta, d[j]);
    }
    if (tid == 0) {
        double* r = D.rec + (size_t)rec * VMX_SMC_REC;
        r[0] = beta_prev; r[1] = beta; r[2] = vmx_smc::ess_of(s1, s2);
        D.state[0] = beta;
        D.counters[0] = 0; D.counters[1] = 0; D.counters[2] = 0;
    }
    __syncthreads();

    // cumulative weights: lane j sums its segment, the totals are scanned, every entry takes the scanned total before its segment
    const int L = vmx_smc::segment_length(N);
    s_a[tid] = vmx_smc::segment_sums(tid, D.w, s1, N, D.cum);
    __syncthreads();
    for (int step = 1; step < SMC_THREADS; step <<= 1) {
        const double v = tid >= step ? s_a[tid] + s_a[tid - step] : s_a[tid];
        __syncthreads();
        s_a[tid] = v;
        __syncthreads();
    }
    const double pre = tid > 0 ? s_a[tid - 1] : 0.0;
    for (int i = tid * L; i < (tid + 1) * L && i < N; ++i) D.cum[i] = i == N - 1 ? 1.0 : pre + D.cum[i];
    __syncthreads();

    const double v = vmx_smc::resample_uniform(stage, D.seed, D.stream);
    for (int i = tid; i < N; i += SMC_THREADS) {
        const int a = vmx_smc::ancestor(D.cum, N, vmx_smc::position(v, i, N));
        D.rec_anc[(size_t)rec * N + i] = a;
        for (int c = 0; c < n; ++c) D.u2[(size_t)i * n + c] = D.u[(size_t)a * n + c];
        D.lnl2[i] = D.lnl[a];
    }
    __syncthreads();
    for (int q = tid; q < N * n; q += SMC_THREADS) D.u[q] = D.u2[q];
    for (int i = tid; i < N; i += SMC_THREADS) D.lnl[i] = D.lnl2[i];
    __syncthreads();

    smc_precondition(D, rec);
}

// One sweep boundary in one work-group (the acceptance count steers the scale of every particle's next proposal): decide sweep
// s_dec of the stage from chi2 / status of each particle's row (s_dec < 0: none), adapt the scale, then propose sweep s_prop
// (s_prop < 0: none - the stage is over: its counts go to the record and beta, acceptance and scale to the host's words) and
// write the N rows of the engine.  Every expression: vmx_smc.h.
__device__ __forceinline__ void smc_move(const SmcDev& D, int64_t stage, int s_dec, int s_prop, int64_t rec)
{
    __shared__ int s_cnt[3];
    __shared__ double s_C[vmx_smc::MAXN * vmx_smc::MAXN];
    __shared__ double s_scale;
    const int N = D.N, n = D.n, tid = threadIdx.x;
    if (isnan(D.state[0])) return;          // (no particle had a finite lnL: the host ends the run)
    if (s_dec >= 0) {
        if (tid < 3) s_cnt[tid] = 0;
        __syncthreads();
        const double beta = D.state[0];
        int acc = 0, own = 0, failed = 0;
        for (int i = tid; i < N; i += SMC_THREADS) {
            const double c2 = D.box.chi2[i];
            const bool inside = D.inside[i] != 0, ok = vmx_ens::model_ok(D.box.status[i], c2);
            const double lnl_new = vmx_ns::lnl_of(D.box.status[i], c2, D.log_norm);
            if (vmx_smc::accept(inside, ok, beta, lnl_new, D.lnl[i], D.uacc[i])) {
                for (int c = 0; c < n; ++c) D.u[(size_t)i * n + c] = D.prop[(size_t)i * n + c];
                D.lnl[i] = lnl_new;
                acc += 1;
            } else if (!inside) own += 1;
            else if (!ok) failed += 1;
        }
        if (acc) atomicAdd(&s_cnt[0], acc);
        if (own) atomicAdd(&s_cnt[1], own);
        if (failed) atomicAdd(&s_cnt[2], failed);
        __syncthreads();
        if (tid == 0) {
            const double scale = vmx_smc::adapt(D.state[1], s_cnt[0], N);
            D.state[1] = scale;
            for (int q = 0; q < 3; ++q) D.counters[q] += s_cnt[q];
            if (s_prop < 0) {
                double* r = D.rec + (size_t)rec * VMX_SMC_REC;
                r[3] = (double)D.counters[0]; r[4] = scale; r[6] = (double)D.counters[1]; r[7] = (double)D.counters[2];
                D.host[1] = r[3]; D.host[2] = scale; D.host[0] = beta;
            }
        }
    }
    if (s_prop < 0) return;
    __syncthreads();
    for (int q = tid; q < n * n; q += SMC_THREADS) s_C[q] = D.chol[q];
    if (tid == 0) s_scale = D.state[1];
    __syncthreads();
    const double scale = s_scale;
    for (int i = tid; i < N; i += SMC_THREADS) {
        double ua = 0.0;
        const bool in = vmx_smc::propose(i, stage, s_prop, n, s_C, scale, D.u + (size_t)i * n, D.seed, D.stream,
                                         D.prop + (size_t)i * n, ua);
        D.uacc[i] = ua;
        D.inside[i] = in ? 1 : 0;
    }
    __syncthreads();
    smc_write_rows(D, true);
}

// The kernels, for a set of runs (vmx_smc_run_many; vmx_smc_run is the set of one): work-group a of a launch owns run active[a] -
// the functions above over that run's part of every array - and the engine rows a N .. (a + 1) N - 1; nothing crosses runs.
// `run0` is the view of run 0 on the rows of slot 0.  Every active run is at record row `round` of the call and at stage
// stage0[run] + round of its own count.
struct SmcSetDev {
    SmcDev run0;
    const int32_t* active;              // [A] the runs still going, ascending
    const uint64_t* streams;            // [E] Philox streams
    const int64_t* stage0;              // [E] the runs' stage at entry
    const int32_t* mock_row;            // [E] the pool row of every run, or nullptr
    int32_t* mock;                      // [E N] the mock row of every engine row (the kernels that open a round write it)
    int32_t rec_rows;                   // record rows per run
};

__device__ __forceinline__ SmcDev smc_view(const SmcSetDev& S, int& run)
{
    SmcDev D = S.run0;
    const size_t a = blockIdx.x, r = (size_t)S.active[a], N = (size_t)D.N, n = (size_t)D.n;
    run = (int)r;
    D.u += r * N * n; D.lnl += r * N; D.u2 += r * N * n; D.lnl2 += r * N; D.w += r * N; D.cum += r * N;
    D.mean += r * n; D.cov += r * n * n; D.chol += r * n * n; D.state += r * 2;
    D.prop += r * N * n; D.uacc += r * N; D.inside += r * N;
    D.box.theta += a * N * (size_t)D.P; D.box.chi2 += a * N; D.box.status += a * N;
    D.rec += r * (size_t)S.rec_rows * VMX_SMC_REC; D.rec_lnl += r * (size_t)S.rec_rows * N; D.rec_anc += r * (size_t)S.rec_rows * N;
    D.counters += r * 3; D.host += r * 4;
    D.stream = S.streams[r];
    return D;
}

// the mock of the engine rows of this work-group's slot
__device__ __forceinline__ void smc_write_mock(const SmcSetDev& S, int run)
{
    if (!S.mock_row) return;
    const int N = S.run0.N, m = S.mock_row[run];
    for (int i = threadIdx.x; i < N; i += SMC_THREADS) S.mock[(size_t)blockIdx.x * N + i] = m;
}

__global__ __launch_bounds__(SMC_THREADS) void k_smc_start(SmcSetDev S)
{
    int run;
    const SmcDev D = smc_view(S, run);
    smc_write_mock(S, run);
    smc_start(D);
}

__global__ __launch_bounds__(SMC_THREADS) void k_smc_start_lnl(SmcSetDev S)
{
    int run;
    const SmcDev D = smc_view(S, run);
    smc_start_lnl(D);
}

__global__ __launch_bounds__(SMC_THREADS) void k_smc_stage(SmcSetDev S, int64_t round)
{
    int run;
    const SmcDev D = smc_view(S, run);
    smc_stage(D, S.stage0[run] + round, round);
}

// (rec_u [E][rec_rows][N][n])
__global__ __launch_bounds__(SMC_THREADS) void k_smc_stage_kept(SmcSetDev S, int64_t round, double* rec_u)
{
    int run;
    const SmcDev D = smc_view(S, run);
    if (rec_u) rec_u += (size_t)run * (size_t)S.rec_rows * (size_t)D.N * (size_t)D.n;
    smc_stage<true>(D, S.stage0[run] + round, round, rec_u);
}

__global__ __launch_bounds__(SMC_THREADS) void k_smc_move(SmcSetDev S, int64_t round, int s_dec, int s_prop)
{
    int run;
    const SmcDev D = smc_view(S, run);
    if (s_dec < 0) smc_write_mock(S, run);
    smc_move(D, S.stage0[run] + round, s_dec, s_prop, round);
}

}  // namespace

// A chain store (vmx_chain_store_*; vmx_chain.h): the recorded rows of E ensembles on the device and the scratch of their summary
struct vmx_chain_store {
    vmx_engine* engine = nullptr;
    int E = 0, W = 0, n = 0;
    int64_t capacity = 0, rows = 0;
    DevBuf<double> x, lnl;              // [E][capacity][W][n], [E][capacity][W]
    // the summary's scratch, grown on demand: series sums and means [E][W][n] each, the centred series [E][n][T][W], the results
    DevBuf<double> sums, centred, out;
    DevBuf<int64_t> window;
    // the scratch of the order statistics and the best row (vmx_chain_select.h): the keys [E][n][T W] (64-bit keys held in a buffer
    // of doubles, so that the poison mode reaches them: its fill is the NaN key), the values [E][n][ranks] or lnL [E] + position
    // [E][n], and the best index [E]
    DevBuf<double> sel_keys, sel_out;
    DevBuf<int64_t> sel_index;
};

// A sample store (vmx_sample_store_*; vmx_chain_weighted.h): E weighted, ragged sample sets on the device and the scratch of their
// reductions
struct vmx_sample_store {
    vmx_engine* engine = nullptr;
    int E = 0, n = 0;
    int64_t capacity = 0;
    DevBuf<double> x, lnl, w;           // [E][capacity][n], [E][capacity], [E][capacity]
    DevBuf<int64_t> counts;             // [E]: the rows of every set, where the kernels read them
    std::vector<int64_t> h_counts;      // ... and where the entries check them
    std::vector<uint64_t> h_total;      // [E]: M of every set as put computed it on the host (the bound of a target)
    // scratch, grown on demand (64-bit integers held in buffers of doubles, so that the poison mode reaches them): the integer
    // weights [E][capacity], the trees' terms [E][padded(capacity) / 2], w_max / S / s2 / M / mean / covariance [E][4 + n + n n],
    // the keys [E][n][capacity], the targets [E][U], the values [E][n][U] or lnL [E] + position [E][n], the best index [E] (the one
    // buffer outside those helpers: an int64 buffer like the chain store's sel_index - integers are never poisoned, and
    // k_wchain_best writes every entry)
    DevBuf<double> m, tree, stats, keys, targets, out;
    DevBuf<int64_t> index;
};

// Whether the quadratic term of the Q' form may run over the trapezoidal root of Q' (quad_build).  false: only with VMX_QUAD_ROOT=1.
constexpr bool QUAD_ROOT_DEFAULT = true;

struct vmx_engine {
    int device = 0;
    hipStream_t stream = nullptr;
    // correlation items are independent between xi_bins and chi2: item q > 0 runs on aux[q-1] (fork / join events)
    hipStream_t cur = nullptr;
    std::vector<hipStream_t> aux;
    hipEvent_t ev_fork = nullptr;
    std::vector<hipEvent_t> ev_join;
    bool finalized = false;
    // Second lane (vmx_set_lanes): a clone that borrows every static tensor and owns its per-batch workspace and stream;
    // chi2-only device evaluations alternate between the two, so that independent batches overlap on the GPU.
    std::vector<vmx_engine*> lanes;        // lanes 1 .. n_lanes - 1 (lane 0 is this engine), made on demand
    int n_lanes = 1;
    int64_t lane_calls = 0;
    hipStream_t last_stream = nullptr;      // the stream the last vmx_eval_device ran on
    const int32_t* call_mock = nullptr;     // per-call mock rows of the walkers (device pointer; vmx_eval_device_mocks, vmx_fit_migrad)
    FitWorkspace* fitws = nullptr;
    EnsWorkspace* ensws = nullptr;
    std::vector<vmx_chain_store*> chain_stores;    // every store created on this engine and not yet destroyed
    vmx_chain_store* chain_store = nullptr;        // the one the ensemble runs append to (vmx_ensemble_set_chain_store)
    std::vector<vmx_sample_store*> sample_stores;  // every sample store created on this engine and not yet destroyed
    NsWorkspace* nsws = nullptr;
    SmcWorkspace* smcws = nullptr;
    // a likelihood session (vmx_fit_migrad and the three samplers): lane_wait, when set, is the event at which the rows of the second
    // lane's calls are complete (its stream waits for it); ev_rows is the session's event for that, ev_lane the one that joins the
    // second lane back to `stream`.  Both are made on first use.
    hipEvent_t lane_wait = nullptr, ev_rows = nullptr, ev_lane = nullptr;

    int nk = 0, nkp = 0, n_mu = 0;
    int n_rows = 0, n_extra = 0, mu_lo = 0, mu_hi = 0;     // node rule of the mu sums (vmx_set_mu_quadrature)
    int mu_tiers = 1;                                      // VMX_NO_MU_TIERS: 1 - the main rule for every k tile of k_pk_tab2
    vmx_plan::MuTierDesc mu_tier[vmx_plan::MU_TIERS] = {};
    std::vector<uint16_t> zmap64, zmap16;                  // launch order and tiers of k_pk_tab2's k tiles (vmx_plan::plan_mu_tiles)
    int last_tab2_kt = 0;                                  // tile width of the last k_pk_tab2 launch (0: none)
    DevBuf<double> node_w, mu_img, mu_img_w;
    std::vector<int32_t> rule_slot; std::vector<double> rule_lo, rule_hi;     // vmx_set_mu_rule_box
    DevBuf<int32_t> d_rule_slot; DevBuf<double> d_rule_lo, d_rule_hi;
    double k_node_max = 0.0; bool mu_nodes_on = true;
    DevBuf<double> k, pklin, delta2, mu, sq1mmu2, lnmu, wl, gk, gk_mom, fv_x, fv_f, xtab;
    std::vector<int32_t> const_slots;        // parameters a level-1 table depends on (the Arinyo set)
    std::vector<int32_t> const_slots2;       // ... a level-2 table: + everything that enters a Gaussian factor
    DevBuf<int32_t> d_const_slots, d_const_slots2, d_xtab_pipe, d_xtab_partner;
    DevBuf<double> xtab_k;
    std::vector<int32_t> xi_static_taps, xi_static_bins;     // k_xi_bins<true> / k_xi_bins_static launch lists (set by poly_basis_build)
    DevBuf<int32_t> d_xi_static_taps, d_xi_static_bins;
    DevBuf<unsigned long long> gemm_trace;   // VMX_GEMM_TRACE=<file>: block timeline of the last FFTLog product, written by vmx_sync
    size_t gemm_trace_blocks = 0;
    DevBuf<unsigned long long> pk_trace;     // VMX_PK_TRACE=<file>: block timeline of the last k_pk_tab2 launch, written by vmx_sync
    size_t pk_trace_blocks = 0;
    std::vector<int32_t> w_groups;           // shared-W groups (indices into pk_groups): k_pk_w for large batches
    DevBuf<int32_t> d_w_groups;
    bool no_pk_w = false;                    // VMX_NO_PK_W: the shared-W groups stay in k_pk_multipoles
    std::vector<Tab2Group> tab2_groups;      // the groups with tables, as k_pk_tab2 takes them (cross groups first)
    DevBuf<double> xtab_key;
    int n_xtab = 0;
    int const_hint = 0;              // vmx_set_constant_nl_hint: table level the caller vouches for (device-resident theta)
    int fv_n = 0;
    struct GkSpec { double rp, rt, mock_rp, mock_rt; };   // G(rp, rt) * G(mock_rp, mock_rt); a zero size = factor 1
    std::vector<GkSpec> gk_tables;
    std::vector<double> h_k, h_mu;

    int n_coef = 0, ncp = 0, n_knots = 0;
    DevBuf<double> op;          // [VMX_MAX_ELL][ncp][nkp]
    bool op_set[VMX_MAX_ELL] = {false, false, false, false};
    bool extrapolate = false;
    double x0[VMX_MAX_ELL] = {0}, h[VMX_MAX_ELL] = {0};

    std::vector<PipeDev> pipes;
    std::vector<double> h_r, h_mu_c, h_z, h_relz, h_lnrelz, h_lnrelz2, h_growth;
    DevBuf<double> cr, cmu, crp, crt, cz, crelz, clnrelz, clnrelz2, cgrowth;
    DevBuf<PipeDev> d_pipes;
    std::vector<PkGroup> pk_groups;
    DevBuf<PkGroup> d_pk_groups;
    std::vector<int32_t> pk_members, pk_poly, pk_static;     // pk_static: polynomial pipelines with a static coefficient basis
    DevBuf<int32_t> d_pk_members, d_pk_poly, d_pk_static, d_pipe_active;
    DevBuf<double> poly_coef, poly_bins;
    int64_t poly_bins_total = 0;
    int n_active = 0;
    bool poly_dirty = true;

    std::vector<ItemHost*> items;
    std::vector<MetalHost*> metals;
    DevBuf<ItemDev> d_items;
    DevBuf<MetalDev> d_metals;
    std::vector<double> h_bb, h_odd, h_odd_op;
    std::map<int, int64_t> odd_op_off;        // pipeline -> its odd-multipole operator in odd_op (vmx_pipeline_set_odd_operator)
    DevBuf<double> bb_basis, odd_coef, odd_op, odd_dyn, sn_a;
    int sn_n = 0; double sn_tau0 = 0.0, sn_dtau = 1.0;

    std::vector<int32_t> prior_slot;
    std::vector<double> prior_mean, prior_sigma;
    DevBuf<int32_t> d_prior_slot;
    DevBuf<double> d_prior_mean, d_prior_sigma;

    DevBuf<double> gcinv, gres, gz;
    int g_n = 0, g_ld = 0;

    int n_params = 0, max_batch = 0, model_size = 0, slab_rows = 0;
    int pad_l = 0, pad_r = 0;           // vmx_set_fftlog_padding
    int fact_slab_rows = 0;          // rows of the factored form's slabs of F dx (small rows: up to 4 K splits of a full batch)
    std::map<int, std::vector<int>> group_splits;     // K splits of the grouped launches per (stage, batch size)
    // tapes of the quadratic-form launches per number of walker tiles: the blocks' entries, their queues, the partial-sum slots
    // (root = true: the tape runs over the items' trapezoidal roots and stores partial tiles - ypart holds, item after item,
    // max_segs slabs of [64 tn walkers][n_masked_pad]; segs the segment counts per (item's row tile, walker tile); y_off / seg_off
    // where an item's share of the two begins)
    struct QuadList {
        DevBuf<GemmWork> work; DevBuf<int32_t> queue, nt_off; DevBuf<double> part; int n_blocks = 0; int n_entries = 0;
        bool root = false; DevBuf<double> ypart; DevBuf<int32_t> segs; std::vector<int64_t> y_off; std::vector<int32_t> seg_off; int max_segs = 0;
    };
    std::map<int, QuadList*> quad_lists;     // by number of walker tiles
    std::vector<void*> host_allocs;          // vmx_host_alloc: pinned host buffers handed to the caller, freed with the engine at the latest
    std::map<int, QuadList*> cinv_lists;     // the same tape over the inverse covariances (chi2 of the full chain), by walker tiles
    DevBuf<double> zero_row;                 // zeros, as long as the longest padded residual: that contraction has no linear term
    int quad_blocks = 0;             // persistent blocks of the quadratic-form launch: 2 per CU
    std::vector<double> host_key, pending_key;   // vmx_eval: shared parameters the level-2 tables hold / seen in the last call
    bool host_key_valid = false, skip_xtab_once = false;
    bool fft_ring = true, fft_ring_attr = false;     // (false: the device refused the ring's 128 KB of LDS - the two-buffer kernel then)
    // pre-summed bins (xi_sum_plan): groups of the lean / static-coordinate pipelines of an item, and what assemble_bin is told
    bool xi_sums = true;             // VMX_NO_XI_SUMS: one array per pipeline, as the general kernels write them
    bool sums_dirty = true;
    std::vector<XiLeanGroup> lean_groups; std::vector<XiStaticGroup> static_groups;
    std::vector<int32_t> lean_single;                // lean pipelines that keep their own array: k_xi_bins_lean serves them, as without sums
    std::vector<int32_t> static_single;              // static-coordinate pipelines that keep their own array
    DevBuf<XiLeanGroup> d_lean_groups; DevBuf<XiStaticGroup> d_static_groups; DevBuf<ItemSums> d_item_sums;
    DevBuf<int32_t> d_static_single;
    bool sums_any = false;
    // (members per array: four lean, sixteen static-coordinate pipelines - measured at B = 512: groups of 2 / 3 lean members
    // 462k / 477k evaluations / s against 474k, 4 / 8 static members 472k / 473k)
    bool xi_lean = true;             // VMX_NO_XI_LEAN: every per-walker pipeline's bins by the general k_xi_bins
    std::vector<int32_t> xi_lean_pipes, xi_rest_pipes;      // the active pipelines k_xi_bins_lean serves / the others
    DevBuf<int32_t> d_xi_rest_pipes;
    bool ring_allowed = true;        // one batch in flight only: a 128 KB block leaves the other lane's kernels no room on its CU
    int last_tab_level = 0;          // table level of the last chain (vmx_debug_read what = 4)
    bool no_tab2 = false;            // VMX_NO_TAB2: level-1 tables only (the Gaussian factors stay in the mu loop)
    bool no_cinv_tape = false;       // VMX_NO_CINV_TAPE: chi2 of the full chain by the C^-1 products + k_chi2 at every batch size
    bool pk_small_attr = false;      // the single-walker P(k) shape asked for its > 64 KB of LDS
    bool kron_attr = false;          // k_metal_kron asked for its dynamic LDS
    DevBuf<double> mv_part;          // split-K slabs of the stand-alone product
    int64_t xi_total = 0, xim_total = 0;
    DevBuf<double> theta, scal, metal_bias, pl, coef, xi, xim, model, chi2;
    DevBuf<int32_t> status, mock_index, k_live, coef_win;
    DevBuf<double> pk_direct;        // [max_batch][nkp] per-walker linear spectra of the direct_pk mode
    bool direct = false;
    std::vector<int32_t> h_mock_index;
    int last_B = 0;
    bool last_full = false;          // the last evaluation ran the full chain (model and residuals are valid)
    bool last_taps = true;           // ... wrote the per-pipeline bins (vmx_debug_read what = 1)
    // quadratic form of chi2: used when only chi2 is asked for (see vmx_set_quadratic_form)
    std::vector<double> theta_ref;
    bool quad_eligible = false, quad_mat_dirty = true, quad_lin_dirty = true, no_fuse = false;
    bool static_poly = true;         // vmx_set_static_poly
    int quad_kind = 0;               // vmx_set_quadratic_form_kind: 0 = the cheaper form, 1 = Q', 2 = factored
    bool quad_factored = false;      // the form the tensors were built for
    bool quad_root = false;          // every item holds the trapezoidal root of its Q' (quad_build): tapes may run over it
    bool no_quad_root = false;       // VMX_NO_QUAD_ROOT: the quadratic term stays the half-triangle contraction
    bool force_quad_root = false;    // VMX_QUAD_ROOT=force: the root wherever it can be built, whatever the tapes' prices (tests)
    bool last_root = false;          // the last Q' evaluation ran the tape over the roots (vmx_debug_read 4 [11])
    struct MargReq { double* out; int64_t ld_out; int32_t* status; };
    const MargReq* marg_req = nullptr;      // set while vmx_marg_coeff_device runs the chain: derived columns instead of chi2
    int marg_slab_rows = 0;          // rows of the items' mg_y (K slabs of G dx)
    int last_form = 0;               // form of the last evaluation: 0 full chain, 1 Q', 2 factored (vmx_debug_read 4 [8])
    // bins kernels of the last evaluation (vmx_debug_read 4 [9], VMX_ROUTE_*); route_setup: those of set-up.  A replayed graph runs
    // no host code: graph_route keeps the mask and last_taps of each captured chain.
    int last_route = 0, route_setup = 0;
    // form of the FFTLog o spline product of the last evaluation (vmx_debug_read 4 [10], VMX_FFT_*): set where it is launched
    int last_fft_form = 0;
    struct ChainFacts { int route = 0; bool taps = true; int fft_form = 0; int tab2_kt = 0; };
    std::map<int, ChainFacts> graph_route;
    // VMX_TRACE_HOST: host-side phases of vmx_eval accumulated in nanoseconds (staging, enqueue, wait), printed at destroy
    bool trace_host = false; double host_ns[3] = {0, 0, 0}; int64_t host_calls = 0;
    EngineDev dev{};

    // host path: pinned staging buffers and one captured graph per batch size
    double* pin_theta = nullptr; double* pin_chi2 = nullptr; int32_t* pin_status = nullptr;
    std::vector<double> blind_scale, blind_shift;       // parameter-level blinding (empty = off); device copy [2][n_params]
    DevBuf<double> d_blind;
    double* dpin_theta = nullptr; double* dpin_chi2 = nullptr; int32_t* dpin_status = nullptr;   // device views
    int64_t* pin_done = nullptr; int64_t* dpin_done = nullptr; int64_t done_seq = 0;          // completion word of single-walker calls
    // single-walker quadratic form: one number per block of the last products (k_gemv1 MODE 2), added up by the host
    double* pin_part = nullptr; double* dpin_part = nullptr;
    int host_reduce_items = 0, host_reduce_blocks[VMX_MAX_GROUP] = {0};
    bool no_host_reduce = false;     // VMX_NO_HOST_REDUCE
    std::map<int, hipGraphExec_t> graphs;
    bool use_graphs = true;

    // profiling
    bool profiling = false;
    uint32_t prof_mask = 0xffffffffu;     // kernel classes that get event pairs while profiling
    int prof_stride = 1; int64_t prof_count[32] = {};      // ... every prof_stride-th launch of each of them (vmx_set_profiling_mask)
    struct Span { hipEvent_t a, b; int kc; };
    std::vector<Span> spans;
    size_t span_used = 0;
    double ms[VMX_N_KERNELS] = {0};
    int64_t launches[VMX_N_KERNELS] = {0};

    ~vmx_engine() {
        for (auto* l : lanes) { (void)hipStreamSynchronize(l->stream); delete l; }
        lanes.clear();
        for (auto* it : items) delete it;
        for (auto* m : metals) delete m;
        for (auto& s : spans) { (void)hipEventDestroy(s.a); (void)hipEventDestroy(s.b); }
        for (auto& g : graphs) (void)hipGraphExecDestroy(g.second);
        for (auto& q : quad_lists) delete q.second;
        for (auto& q : cinv_lists) delete q.second;
        for (void* p : host_allocs) (void)hipHostFree(p);
        delete fitws;
        delete ensws;
        for (auto* c : chain_stores) delete c;
        for (auto* c : sample_stores) delete c;
        delete nsws;
        delete smcws;
        if (pin_theta) (void)hipHostFree(pin_theta);
        if (pin_chi2) (void)hipHostFree(pin_chi2);
        if (pin_status) (void)hipHostFree(pin_status);
        if (pin_done) (void)hipHostFree(pin_done);
        if (pin_part) (void)hipHostFree(pin_part);
        for (auto& a : aux) (void)hipStreamDestroy(a);
        for (auto& ev : ev_join) (void)hipEventDestroy(ev);
        if (ev_fork) (void)hipEventDestroy(ev_fork);
        if (ev_rows) (void)hipEventDestroy(ev_rows);
        if (ev_lane) (void)hipEventDestroy(ev_lane);
        if (stream) (void)hipStreamDestroy(stream);
    }
};

namespace {

// Anything that changes what an evaluation computes retires the second lane (it borrows the static tensors and copies
// the host-side state at the moment it is made); the next two-lane evaluation makes a fresh one.
static void drop_lane(vmx_engine* e)
{
    if (!e) return;
    for (auto* l : e->lanes) { (void)hipStreamSynchronize(l->stream); delete l; }
    e->lanes.clear();
}
static void wait_lane(vmx_engine* e) { if (e) for (auto* l : e->lanes) (void)hipStreamSynchronize(l->stream); }

struct ScopedTimer {
    vmx_engine* e; int idx = -1;
    ScopedTimer(vmx_engine* eng, int kc) : e(eng) {
        if (!e->profiling || !((e->prof_mask >> kc) & 1u)) return;
        if (e->prof_stride > 1 && (e->prof_count[kc]++ % e->prof_stride) != 0) return;
        if (e->span_used == e->spans.size()) {
            vmx_engine::Span s{};
            if (hipEventCreate(&s.a) != hipSuccess || hipEventCreate(&s.b) != hipSuccess) return;
            e->spans.push_back(s);
        }
        idx = (int)e->span_used++;
        e->spans[idx].kc = kc;
        (void)hipEventRecord(e->spans[idx].a, e->cur);
    }
    ~ScopedTimer() { if (idx >= 0) (void)hipEventRecord(e->spans[idx].b, e->cur); }
};

static void collect_spans(vmx_engine* e)
{
    for (size_t i = 0; i < e->span_used; ++i) {
        float t = 0.f;
        if (hipEventElapsedTime(&t, e->spans[i].a, e->spans[i].b) == hipSuccess) {
            e->ms[e->spans[i].kc] += t;
            e->launches[e->spans[i].kc] += 1;
        }
    }
    e->span_used = 0;
}

// true when `peak` evaluates the same P(k,mu) factors as `smooth` apart from the peak-only Gaussian
// broadening (and the k-only linear spectrum): then both are produced by one pass of k_pk_multipoles
static bool pk_stage_compatible(const vmx_pipe_desc& smooth, const vmx_pipe_desc& peak)
{
    vmx_pipe_desc a = smooth, b = peak;
    if (a.is_peak || !b.is_peak || a.peak_nl || !b.peak_nl) return false;
    // neutralise the fields that are allowed to differ, then compare everything the P(k) stage reads
    b.is_peak = a.is_peak; b.pk_lin_kind = a.pk_lin_kind; b.peak_nl = a.peak_nl;
    b.sigma_nl_par_slot = a.sigma_nl_par_slot; b.sigma_nl_per_slot = a.sigma_nl_per_slot;
    b.scale_mode = a.scale_mode; b.scale_slot[0] = a.scale_slot[0]; b.scale_slot[1] = a.scale_slot[1];
    b.radiation = a.radiation;
    return std::memcmp(&a, &b, sizeof(vmx_pipe_desc)) == 0;
}

// true when two pipelines without amplitude-dependent mu structure share the factor W(k, mu) (G table, Gaussian
// exponent, velocity dispersion): they may differ in the tracers' bias / beta, the linear spectrum and the xi stage
static bool w_stage_compatible(const vmx_pipe_desc& a, const vmx_pipe_desc& b)
{
    if (a.gk_table != b.gk_table || a.is_peak != b.is_peak || a.peak_nl != b.peak_nl) return false;
    if (a.mock_los_slot >= 0 || b.mock_los_slot >= 0) return false;        // (a per-walker factor of the mu loop)
    if (a.peak_nl && (a.sigma_nl_par_slot != b.sigma_nl_par_slot || a.sigma_nl_per_slot != b.sigma_nl_per_slot ||
                      a.growth_rate_slot != b.growth_rate_slot || a.growth_rate_default != b.growth_rate_default))
        return false;
    if (a.n_smooth != b.n_smooth || a.exp_par_slot != b.exp_par_slot || a.exp_per_slot != b.exp_per_slot) return false;
    for (int i = 0; i < a.n_smooth; ++i)
        if (a.smooth_par_slot[i] != b.smooth_par_slot[i] || a.smooth_per_slot[i] != b.smooth_per_slot[i] ||
            a.smooth_weight[i] != b.smooth_weight[i]) return false;
    if (a.vd_kind != b.vd_kind) return false;
    for (int q = 0; q < 2; ++q)
        if (a.vd_kind != VMX_VD_NONE && (a.tracer[q].discrete != b.tracer[q].discrete ||
                                         (a.tracer[q].discrete && a.tracer[q].vd_sigma_slot != b.tracer[q].vd_sigma_slot)))
            return false;
    return a.hcd_model == VMX_HCD_NONE && b.hcd_model == VMX_HCD_NONE && a.nl_model == VMX_NL_NONE &&
           b.nl_model == VMX_NL_NONE;
}

// compile-time specialisation of the mu loop that matches a pipeline (PKV_GENERIC when none does)
static int pk_variant(const vmx_pipe_desc& d, bool paired)
{
    const bool rare = d.hcd_model == VMX_HCD_SINC || d.hcd_model == VMX_HCD_FVOIGT || d.nl_model == VMX_NL_MCDONALD || d.exp_par_slot >= 0 ||
                      d.mock_los_slot >= 0 ||
                      (d.fast_metals && (d.tracer[0].is_lya || d.tracer[1].is_lya) &&
                       (d.uvb || d.heii || d.hcd_model != VMX_HCD_NONE));
    if (rare) return PKV_GENERIC;
    // no mu-dependent factor besides the Kaiser polynomial and the static G table: closed form in the moments
    if (!rare && !paired && !d.is_peak && !d.peak_nl && d.hcd_model == VMX_HCD_NONE && d.nl_model == VMX_NL_NONE &&
        d.n_smooth == 0 && d.exp_par_slot < 0 && d.vd_kind == VMX_VD_NONE)
        return PKV_POLY;
    const bool rogers = d.hcd_model == VMX_HCD_ROGERS;
    const bool hcd1 = rogers && d.tracer[0].is_lya, hcd2 = rogers && d.tracer[1].is_lya;
    const bool arinyo = d.nl_model == VMX_NL_ARINYO;
    const bool lorentz = d.vd_kind == VMX_VD_LORENTZ;
    const bool vd1 = lorentz && d.tracer[0].discrete, vd2 = lorentz && d.tracer[1].discrete;
    if (vd1 || d.gk_table < 0) return PKV_GENERIC;
    if (d.same_tracer) {
        if (hcd1 && arinyo && paired && !vd2) return PKV_AUTO_CORE;
        if (!hcd1 && !arinyo && !paired && !vd2) return PKV_PLAIN_SAME;
        return PKV_GENERIC;
    }
    if (hcd1 && !hcd2 && arinyo && paired && vd2) return PKV_CROSS_CORE;
    if (!hcd1 && !hcd2 && !arinyo && !paired) return vd2 ? PKV_PLAIN_PAIR_VD : PKV_PLAIN_PAIR;
    return PKV_GENERIC;
}

// k_gemm_nt44 forms its DMA source addresses as 32-bit byte offsets from the operand's base (vmx_device.h: oa / ox in setup()):
// the last byte of an operand of `rows` rows of `ld` doubles has to lie below 4 GiB.  (The streaming kernels index with size_t.)
static const uint64_t GEMM44_OPERAND_LIMIT = 1ull << 32;
static bool gemm44_addressable(int64_t rows, int64_t ld) { return (uint64_t)rows * (uint64_t)ld * sizeof(double) < GEMM44_OPERAND_LIMIT; }
#define GEMM44_LIMIT_MSG "an operand of the MFMA product kernel must stay below 4 GiB (2^32 bytes: 32-bit DMA byte offsets)"

// the single-walker streaming kernel keeps x in LDS
static bool gemv1_applies(int N, int K) { return N == 1 && K <= 5120 && (size_t)K * sizeof(double) <= 48 * 1024; }

// CSR distortion product of one item for B walkers -> it->dist (one slab)
static void launch_csr(vmx_engine* e, ItemHost* it, int B)
{
    const ItemDev& d = it->dev;
    ScopedTimer timer(e, KC_DISTORTION);
    const int rows = d.d.n_dist;
#define VMX_CSR(NB) hipLaunchKernelGGL(k_csr_spmm<NB>, dim3((rows + 3) / 4, (B + NB - 1) / NB), dim3(256), 0, e->cur, it->csr_ptr.p, \
                                       it->csr_idx.p, it->csr_val.p, rows, it->vec.p, d.n_model_pad, B, it->dist.p, d.n_dist_pad)
    if (B == 1) VMX_CSR(1);
    else if (B == 2) VMX_CSR(2);
    else if (B <= 4) VMX_CSR(4);
    else VMX_CSR(8);
#undef VMX_CSR
}

// persistent blocks of the single-walker streaming kernel (2 per CU), rows strided over them
static int gemv1_blocks(int M)
{
    int blocks = 512;
    while ((M + blocks - 1) / blocks > GEMV1_MAX_ROWS) blocks *= 2;
    return blocks > M ? M : blocks;
}

// Tiling of one MFMA product: fills the tile / split fields of `g`, returns the number of K slabs and, in *per_xcd,
// the blocks each XCD runs for it.  `other_tiles`: tiles of the other problems of the same launch.
static int plan_gemm(vmx_engine* e, GemmArgs& g, int nbatch, int slab_rows_avail, const int32_t* k_limit, bool tri,
                     int other_tiles, int* per_xcd, int forced_split = 0)
{
    constexpr int BM = GEMM_BM, BN = GEMM_BN, BK = GEMM_BK;
    const int tm = (g.M + BM - 1) / BM, tn = (g.N + BN - 1) / BN;
    const int tm_eff = tri ? (tm + 1) / 2 : tm;       // a triangular matrix pairs its row tiles (k_gemm_nt)
    const int tiles = tm_eff * tn * nbatch + other_tiles;
    // split K (1, 2, 4 or 8 ways: a split belongs to whole XCDs) until the launch has at least 512 blocks (2 per CU);
    // partial sums go to separate slabs, which the consumer kernels re-read: more splits cost there
    int nsplit = 1;
    while (nsplit < 8 && tiles * nsplit < 512) nsplit *= 2;
    if (forced_split > 0) nsplit = forced_split;
    while (nsplit > 1 && (int64_t)nsplit * g.N > slab_rows_avail) nsplit /= 2;
    int klen = ((g.K + nsplit - 1) / nsplit + BK - 1) / BK * BK;
    while (nsplit > 1 && (int64_t)klen * (nsplit - 1) >= g.K) { nsplit /= 2; klen = ((g.K + nsplit - 1) / nsplit + BK - 1) / BK * BK; }
    g.nsplit = nsplit; g.klen = klen; g.d_slab = (int64_t)g.N * g.ldd;
    g.tm = tm; g.tn = tn; g.k_limit = k_limit; g.tri = tri ? 1 : 0;
    const int ngroups = 8 / nsplit;
    *per_xcd = ((tm_eff + ngroups - 1) / ngroups) * tn;
    if (g.m_window && nsplit == 1) *per_xcd = tm_eff * ((tn + 7) / 8);     // walker tiles over the XCDs (k_gemm_nt44: n_major)
    return nsplit;
}

// K splits of the problems of one grouped launch.  A CU works through its blocks one after the other (the SIMDs issue
// from the oldest wave first, so the second resident block only fills gaps), which makes a launch a list-scheduling
// problem: blocks of `stages / split` K stages (+ a fixed start / end cost), handed in launch order to the first free of
// the 256 CUs.  Every combination of 1 / 2 / 4 / 8-way splits is simulated (up to three problems; beyond that the
// block-count rule of plan_gemm applies) and the shortest makespan wins, extra slabs charged with their write + re-read
// at ~3 TB/s.
// (vmx_plan::choose_group_splits, vmx_plan.h: both models, run on the CPU by tests/test_planner_host.py)
using vmx_plan::SplitProblem;
using vmx_plan::choose_group_splits;

static int gemm_tiles(int M, int N, bool tri)
{
    const int tm = (M + GEMM_BM - 1) / GEMM_BM, tn = (N + GEMM_BN - 1) / GEMM_BN;
    return (tri ? (tm + 1) / 2 : tm) * tn;
}

static void launch_gemm_group(vmx_engine* e, int kc, const GemmGroup& G, int per_xcd_total, int nbatch)
{
    constexpr int BM = GEMM_BM, BN = GEMM_BN, BK = GEMM_BK;
    dim3 grid(8 * per_xcd_total, nbatch), block(256);
    // the four-block 4x4x4 MFMA kernel runs every full product (distortion and metal matrices, FFTLog o spline,
    // stand-alone products); the short triangular C^-1 products are faster on the 16x16x4 kernel, whose two resident
    // blocks hide each other's start and end (0.093 against 0.103 - 0.126 ms: two short passes per block)
    if (kc != KC_INVCOV) {
        block = dim3(GEMM44_THREADS);
        // (a windowed FFTLog launch carries its batch - the multipoles - inside grid.x: GemmGroup::batch_in_x)
        GemmGroup Gx = G;
        dim3 gridx = grid;
        // (when the launch has the chip to itself; with several batches in flight the late starters fill the other lane's gaps)
        const bool batch_x = e->ring_allowed;
        if (batch_x && kc == KC_FFTLOG && G.n == 1 && G.p[0].m_window && G.work == nullptr && nbatch > 1) { Gx.batch_in_x = nbatch; gridx = dim3(grid.x * nbatch, 1); }
        switch (kc) {
            case KC_QUAD: hipLaunchKernelGGL((k_gemm_nt44<KC_QUAD>), grid, block, 0, e->cur, G); break;
            case KC_DISTORTION: hipLaunchKernelGGL((k_gemm_nt44<KC_DISTORTION>), grid, block, 0, e->cur, G); break;
            case KC_METAL: hipLaunchKernelGGL((k_gemm_nt44<KC_METAL>), grid, block, 0, e->cur, G); break;
            case KC_FFTLOG:
                e->last_fft_form = G.p[0].k_limit ? VMX_FFT_K_LIMIT : 0;
                if (getenv("VMX_GEMM_TRACE")) {
                    e->gemm_trace_blocks = (size_t)2 * grid.x * grid.y;       // (the 64 x 32 tiling has up to twice the blocks)
                    if (e->gemm_trace.n < 4 * e->gemm_trace_blocks) (void)e->gemm_trace.alloc(4 * e->gemm_trace_blocks, true);
                    else (void)hipMemsetAsync(e->gemm_trace.p, 0, 4 * e->gemm_trace_blocks * sizeof(unsigned long long), e->cur);
                    const_cast<GemmGroup&>(G).trace = e->gemm_trace.p;
                }
                // The four-stage ring pays when the launch has about one live tile per CU: a lone block then streams at its own
                // pace (B = 256: 49 -> 44 us).  With fewer tiles its slower dispatch (128 KB of LDS per block) costs more than
                // it gains (B = 64: 32 -> 35 us); with more, two resident two-buffer blocks hide each other's latencies better
                // (B = 1024: 103 -> 138 us).  The live rows are device data: a third of the operator's rows is the estimate.
                if (G.n == 1 && G.p[0].m_window && G.p[0].nsplit == 1 && !G.p[0].tri) {
                    // about one live 64 x 64 tile per CU (the operator's live rows are device data: a third of them is the
                    // estimate): 64 x 32 tiles instead - twice the blocks, two per CU, each covering the other's bubbles
                    const int64_t est = (int64_t)G.p[0].tn * nbatch * ((G.p[0].tm * 3 + 9) / 10);
                    if (est >= 96 && est <= 384) {
                        GemmGroup G2 = G;
                        const int tn32 = (G.p[0].N + 31) / 32;
                        G2.p[0].tn = tn32;
                        const dim3 grid2 = batch_x ? dim3(8 * G.p[0].tm * ((tn32 + 7) / 8) * nbatch, 1) : dim3(8 * G.p[0].tm * ((tn32 + 7) / 8), nbatch);
                        G2.batch_in_x = batch_x ? nbatch : 0;         // (the live blocks of all multipoles first in launch order)
                        // (+ 24 KB of unused dynamic LDS: 72 KB per block = two per CU.  With its own 48 KB the dispatcher packs three
                        // blocks on a CU before it moves on and leaves a third of the CUs empty.)
                        const size_t pad = 24 * 1024;
                        e->last_fft_form |= VMX_FFT_MFMA32 | (G2.batch_in_x ? VMX_FFT_BATCH_X : VMX_FFT_BATCH_Y);
                        hipLaunchKernelGGL((k_gemm_nt44<KC_FFTLOG, 2, 32>), grid2, block, pad, e->cur, G2);
                        break;
                    }
                }
                e->last_fft_form |= Gx.batch_in_x ? VMX_FFT_BATCH_X : VMX_FFT_BATCH_Y;
                if (e->fft_ring && e->ring_allowed && G.n == 1 && G.p[0].m_window) {
                    const int64_t est = (int64_t)G.p[0].tn * nbatch * ((G.p[0].tm * 3 + 9) / 10);
                    if (est < 160 || est > 320) { e->last_fft_form |= VMX_FFT_MFMA64; hipLaunchKernelGGL((k_gemm_nt44<KC_FFTLOG>), gridx, block, 0, e->cur, Gx); break; }
                    constexpr size_t ring_bytes = (size_t)4 * (GEMM_BM + GEMM_BN) * GEMM_BK * sizeof(double);
                    if (!e->fft_ring_attr) {
                        if (hipFuncSetAttribute((const void*)k_gemm_nt44<KC_FFTLOG, 4>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)ring_bytes) != hipSuccess) {
                            (void)hipGetLastError();
                            e->fft_ring = false;
                            e->last_fft_form |= VMX_FFT_MFMA64;
                            hipLaunchKernelGGL((k_gemm_nt44<KC_FFTLOG>), gridx, block, 0, e->cur, Gx);
                            break;
                        }
                        e->fft_ring_attr = true;
                    }
                    e->last_fft_form |= VMX_FFT_RING;
                    hipLaunchKernelGGL((k_gemm_nt44<KC_FFTLOG, 4>), gridx, block, ring_bytes, e->cur, Gx);
                } else { e->last_fft_form |= VMX_FFT_MFMA64; hipLaunchKernelGGL((k_gemm_nt44<KC_FFTLOG>), gridx, block, 0, e->cur, Gx); }
                break;
            default: hipLaunchKernelGGL((k_gemm_nt44<KC_OTHER>), grid, block, 0, e->cur, G); break;
        }
        return;
    }
    hipLaunchKernelGGL((k_gemm_nt<BM, BN, BK, KC_INVCOV>), grid, block, 0, e->cur, G);
}

// D[n][m] = sum_k A[m][k] X[n][k]; returns the number of K slabs written (consumer sums them).
static int launch_product(vmx_engine* e, int kc, const double* A, int lda, int64_t a_batch, int M, int K,
                          const double* X, int ldx, int64_t x_batch, int N, double* D, int ldd,
                          int64_t d_batch, int nbatch, int slab_rows_avail, const int32_t* k_limit = nullptr,
                          int fused_item = -1, bool tri = false, const int32_t* m_window = nullptr)
{
    GemmArgs g{};
    g.A = A; g.lda = lda; g.a_batch = a_batch;
    g.X = X; g.ldx = ldx; g.x_batch = x_batch;
    g.D = D; g.ldd = ldd; g.d_batch = d_batch;
    g.M = M; g.N = N; g.K = K; g.tri = tri ? 1 : 0; g.m_window = m_window;
    ScopedTimer timer(e, kc);
    if (gemv1_applies(N, K)) {
        // persistent streaming kernel: 2 blocks per CU, rows strided over blocks
        g.nsplit = 1; g.klen = K; g.d_slab = 0;
        const int blocks = gemv1_blocks(M);
        dim3 grid(blocks, 1, nbatch), block(256);
        const size_t shmem = (size_t)K * sizeof(double);
        if (kc == KC_FFTLOG) e->last_fft_form = VMX_FFT_GEMV1;
        if (fused_item >= 0) {
            if (K <= 2560) hipLaunchKernelGGL((k_gemv1<5, 1>), grid, block, shmem, e->cur, g, e->dev, fused_item);
            else hipLaunchKernelGGL((k_gemv1<10, 1>), grid, block, shmem, e->cur, g, e->dev, fused_item);
        } else {
            if (K <= 2560) hipLaunchKernelGGL((k_gemv1<5, 0>), grid, block, shmem, e->cur, g, e->dev, 0);
            else hipLaunchKernelGGL((k_gemv1<10, 0>), grid, block, shmem, e->cur, g, e->dev, 0);
        }
        return 1;
    }
    if (N <= 8) {
        g.nsplit = 1; g.klen = K; g.d_slab = 0;
        dim3 grid((M + 3) / 4, 1, nbatch), block(256);
        // (the streaming kernels read whole rows: no column limit; their batch is grid.z)
        if (kc == KC_FFTLOG) e->last_fft_form = VMX_FFT_GEMV | ((N == 1 ? 1 : N == 2 ? 2 : N <= 4 ? 4 : 8) << VMX_FFT_NB_SHIFT);
        switch (N) {
            case 1: hipLaunchKernelGGL(k_gemv<1>, grid, block, 0, e->cur, g); break;
            case 2: hipLaunchKernelGGL(k_gemv<2>, grid, block, 0, e->cur, g); break;
            case 3: case 4: hipLaunchKernelGGL(k_gemv<4>, grid, block, 0, e->cur, g); break;
            default: hipLaunchKernelGGL(k_gemv<8>, grid, block, 0, e->cur, g); break;
        }
        return 1;
    }
    GemmGroup G{};
    int per_xcd = 0;
    const int nsplit = plan_gemm(e, g, nbatch, slab_rows_avail, k_limit, tri, 0, &per_xcd);
    G.p[0] = g; G.n = 1; G.seq_end[0] = per_xcd;
    launch_gemm_group(e, kc, G, per_xcd, nbatch);
    return nsplit;
}

}  // namespace

// capacity N of the fit states and fits per block T: N = the smallest of 4 / 8 / 16 / 32 that holds the stages; T x the state's
// size fits a CU's LDS (vmx_fit.h).  One fit per block: the threads of a wave are in different phases of their fits and a wave
// executes the union of its threads' paths (vmx_fit.h)
template <int N, int T>
static int fit_launch_round(const FitDev& D, hipStream_t st, size_t emit_lds, bool set_attr)
{
    constexpr size_t lds = (size_t)T * fit_lds_stride<N>() * sizeof(double);
    static_assert(lds <= 160 * 1024 - 1024, "fit states of a block must fit a CU's LDS");
    if (set_attr && lds > 64 * 1024)
        HIP_OK(hipFuncSetAttribute((const void*)k_fit_advance<N, T>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    if (set_attr) return 0;
    hipLaunchKernelGGL((k_fit_advance<N, T>), dim3((D.F + T - 1) / T), dim3(FIT_THREADS), lds, st, D);
    hipLaunchKernelGGL(k_fit_scan, dim3(1), dim3(1024), 0, st, D);
    hipLaunchKernelGGL((k_fit_emit<N>), dim3(D.F), dim3(64), emit_lds, st, D);
    return 0;
}
static int fit_round(int cap, const FitDev& D, hipStream_t st, size_t emit_lds, bool set_attr)
{
    switch (cap) {
    case 4: return fit_launch_round<4, 1>(D, st, emit_lds, set_attr);
    case 8: return fit_launch_round<8, 1>(D, st, emit_lds, set_attr);
    case 16: return fit_launch_round<16, 1>(D, st, emit_lds, set_attr);
    default: return fit_launch_round<32, 1>(D, st, emit_lds, set_attr);
    }
}
static size_t fit_state_bytes(int cap)
{
    switch (cap) {
    case 4: return sizeof(vmx_migrad::FitStateT<4>);
    case 8: return sizeof(vmx_migrad::FitStateT<8>);
    case 16: return sizeof(vmx_migrad::FitStateT<16>);
    default: return sizeof(vmx_migrad::FitStateT<32>);
    }
}

extern "C" {

int vmx_struct_size(int32_t which)
{
    switch (which) {
        case 0: return (int)sizeof(vmx_tracer);
        case 1: return (int)sizeof(vmx_pipe_desc);
        case 2: return (int)sizeof(vmx_metal_desc);
        case 3: return (int)sizeof(vmx_item_desc);
        case 4: return (int)sizeof(vmx_fit_spec);
        case 5: return (int)sizeof(vmx_fit_options);
        case 6: return (int)sizeof(vmx_fit_result);
        case 7: return (int)sizeof(vmx_fit_stats);
        case 8: return (int)sizeof(vmx_ensemble_spec);
        case 9: return (int)sizeof(vmx_ensemble_options);
        case 10: return (int)sizeof(vmx_ensemble_stats);
        case 11: return (int)sizeof(vmx_nested_spec);
        case 12: return (int)sizeof(vmx_nested_options);
        case 13: return (int)sizeof(vmx_nested_stats);
        case 14: return (int)sizeof(vmx_smc_spec);
        case 15: return (int)sizeof(vmx_smc_options);
        case 16: return (int)sizeof(vmx_smc_stats);
        case 17: return (int)sizeof(vmx_nested_clusters);
        case 18: return (int)sizeof(vmx_nested_set_options);
        case 19: return (int)sizeof(vmx_nested_phantoms);
        case 20: return (int)sizeof(vmx_nested_set_phantoms);
        case 21: return (int)sizeof(vmx_smc_keep);
        case 23: return (int)sizeof(vmx_ensemble_moves);           // (22 stays vacant: see vegamx.h)
        case 24: return (int)sizeof(vmx_ensemble_adapt);
        case 25: return (int)sizeof(vmx_ensemble_slice);
        case 27: return (int)sizeof(vmx_ensemble_cov);             // (26 stays vacant: see vegamx.h)
        default: return -1;
    }
}

int vmx_create(vmx_engine** out, int device)
{
    REQUIRE(out != nullptr, "out is null");
    int count = 0;
    HIP_OK(hipGetDeviceCount(&count));
    if (count <= 0) return fail(-3, "no HIP device available: the vegamx engine has no CPU fallback");
    REQUIRE(device >= 0 && device < count, "device index out of range");
    HIP_OK(hipSetDevice(device));
    auto* e = new vmx_engine();
    e->device = device;
    hipError_t err = hipStreamCreate(&e->stream);
    if (err != hipSuccess) { delete e; return fail(-2, std::string("hipStreamCreate: ") + hipGetErrorString(err)); }
    e->cur = e->stream;
    *out = e;
    return 0;
}

void vmx_destroy(vmx_engine* e)
{
    if (!e) return;
    if (e->trace_host && e->host_calls)
        std::fprintf(stderr, "[vegamx] host phases of vmx_eval over %lld calls: staging %.2f us, enqueue %.2f us, wait %.2f us\n",
                     (long long)e->host_calls, e->host_ns[0] / e->host_calls * 1e-3, e->host_ns[1] / e->host_calls * 1e-3,
                     e->host_ns[2] / e->host_calls * 1e-3);
    (void)hipSetDevice(e->device);
    (void)hipStreamSynchronize(e->stream);
    delete e;
}

int vmx_set_template(vmx_engine* e, int32_t nk, const double* k, const double* pk_peak,
                     const double* pk_smooth, const double* pk_full, const double* delta2, int32_t n_mu)
{
    REQUIRE(e && !e->finalized, "engine is null or already finalized");
    REQUIRE(nk > 8 && n_mu > 0, "bad template sizes");
    REQUIRE(n_mu <= 2048, "num_bins_muk above 2048: the mu tables of the P(k,mu) kernels no longer fit a CU's LDS (the reference's default is 1000)");
    HIP_OK(hipSetDevice(e->device));
    e->nk = nk; e->nkp = vmx_pad(nk + e->pad_l + e->pad_r); e->n_mu = n_mu;      // (the rows of P_ell carry the FFTLog's power-law pads behind the samples)
    const int nkp = e->nkp;
    std::vector<double> buf(nkp, 0.0);
    e->h_k.assign(k, k + nk);
    std::copy(k, k + nk, buf.begin());
    for (int i = nk; i < nkp; ++i) buf[i] = k[nk - 1];
    if (e->k.upload(buf.data(), nkp)) return -2;
    std::vector<double> pl(3 * (size_t)nkp, 0.0);
    std::copy(pk_peak, pk_peak + nk, pl.begin());
    std::copy(pk_smooth, pk_smooth + nk, pl.begin() + nkp);
    std::copy(pk_full, pk_full + nk, pl.begin() + 2 * (size_t)nkp);
    if (e->pklin.upload(pl.data(), pl.size())) return -2;
    std::fill(buf.begin(), buf.end(), 0.0);
    std::copy(delta2, delta2 + nk, buf.begin());
    if (e->delta2.upload(buf.data(), nkp)) return -2;

    // mu grid: midpoint rule on [0, 1] (power_spectrum.py:76-77); Legendre weights
    // L_ell(mu) (2 ell + 1) / n_mu (pktoxi.py:37,55,138)
    // Node rule of the mu sums.  The reference sums P(k,mu) L_ell(mu) over n_mu midpoints (power_spectrum.py:76-77,
    // pktoxi.py:138).  For an integrand f that is smooth on [a, b] = [mu_lo, n_mu - mu_hi] / n_mu the midpoint sum over
    // that range is, by the Euler-Maclaurin formula (D = d/dmu, h = 1 / n_mu),
    //     sum_j f(mu_j) = (1/h) int_a^b f - (h/24) [Df(b) - Df(a)] + (7 h^3 / 5760) [D^3 f(b) - D^3 f(a)] - O(h^5 D^5 f),
    // so the engine keeps the first mu_lo and the last mu_hi midpoints (where sharp features of the model sit: the
    // Gaussian smoothing / non-linear broadening, the HCD exponential and mu^bv of the Arinyo term at 0; a smoothing that
    // is stronger across than along the line of sight at 1) and replaces the middle by two 32-point Gauss-Legendre
    // panels plus one-sided finite-difference stencils for the two derivative terms: 84 extra nodes with fixed weights.
    // Checked against the reference's own sums over the parameter ranges of the tests: <= 1.2e-13 of the largest
    // k^3 P_ell (tests/test_mu_quadrature.py); used for wavenumbers up to k_node_max (smooth enough for the bin size),
    // the plain midpoint loop above it and for the rarely used model options that are not smooth in mu.
    std::vector<double> node_mu, node_w;
    if (n_mu == 1000) {
        // (round 3: 48 + 48 kept midpoints, two 32-point panels and ONE nine-point one-sided stencil per end that carries the
        // first, third and fifth derivative terms of the Euler-Maclaurin formula at once - 178 nodes, 7e-14 of the largest
        // k^3 M_n over the guard's whole parameter box; round 2's 96 + 96 + 84 with five-point stencils reached 1e-13)
        // The generator and the tiers are vmx_plan.h's (mu_rule_extra, build_mu_tiers - run on the CPU by tests/test_mu_tiers.py).
        // Behind the main rule's 82 extra nodes lie those of up to two shorter rules for the k tiles of k_pk_tab2 whose
        // k^3 M_n carries no weight (+50: 16 + 16 kept midpoints, one 32-point panel; +34: 4 + 4 and one 16-point panel); the
        // numbers and their validation: vega_amd/mu_quadrature.py TIERS, tests/test_mu_tiers.py.
        e->mu_tiers = getenv("VMX_NO_MU_TIERS") ? 1 : vmx_plan::MU_TIERS;
        vmx_plan::build_mu_tiers(n_mu, e->mu_tiers, node_mu, node_w, e->mu_tier);
        e->mu_lo = e->mu_tier[0].lo; e->mu_hi = e->mu_tier[0].hi;
        e->n_extra = e->mu_tier[0].x_cnt;
    }
    // (n_extra: the main rule's nodes - what every kernel but k_pk_tab2 loops over; the tables hold all tiers' rows)
    e->n_rows = n_mu + (int)node_mu.size();
    if (e->node_w.upload(node_w.data(), node_w.size())) return -2;
    const int n_rows = e->n_rows;
    std::vector<double> mu(n_rows), sq(n_rows), lnm(n_rows), wl(4 * (size_t)n_mu);
    for (int j = n_mu; j < n_rows; ++j) {
        const double m = node_mu[j - n_mu];
        mu[j] = m; sq[j] = std::sqrt(std::max(1.0 - m * m, 0.0)); lnm[j] = std::log(m);
    }
    for (int j = 0; j < n_mu; ++j) {
        const double m = (j + 0.5) / n_mu, m2 = m * m;
        mu[j] = m; sq[j] = std::sqrt(1.0 - m2); lnm[j] = std::log(m);
        const double dmu = 1.0 / n_mu;
        wl[j] = dmu * 1.0 * 1.0;
        wl[n_mu + j] = dmu * (0.5 * (3.0 * m2 - 1.0)) * 5.0;
        wl[2 * (size_t)n_mu + j] = dmu * (0.125 * ((35.0 * m2 - 30.0) * m2 + 3.0)) * 9.0;
        wl[3 * (size_t)n_mu + j] = dmu * (0.0625 * (((231.0 * m2 - 315.0) * m2 + 105.0) * m2 - 5.0)) * 13.0;
    }
    e->h_mu = mu;
    {
        // the LDS image of k_pk_tab2's node tables: {mu^2, mu^4} of the midpoints, {mu, mu^2, mu^4, w} of the extra nodes
        // (one image per tier, each of the main rule's size: a block copies the midpoints and its tier's nodes in one run)
        const size_t img_size = 2 * (size_t)n_mu + 4 * (size_t)e->n_extra;
        std::vector<double> img(img_size), img_t(img_size * vmx_plan::MU_TIERS, 0.0);
        for (int j = 0; j < n_mu; ++j) { const double m2 = mu[j] * mu[j]; img[2 * (size_t)j] = m2; img[2 * (size_t)j + 1] = m2 * m2; }
        for (int t = 0; t < vmx_plan::MU_TIERS; ++t) {
            double* dst = &img_t[img_size * t];
            std::copy(img.begin(), img.begin() + 2 * (size_t)n_mu, dst);
            for (int j = 0; j < e->mu_tier[t].x_cnt; ++j) {
                const int r = e->mu_tier[t].x_off + j;
                const double m = mu[n_mu + r], m2 = m * m;
                double* q = dst + 2 * (size_t)n_mu + 4 * (size_t)j;
                q[0] = m; q[1] = m2; q[2] = m2 * m2; q[3] = node_w[r];
            }
        }
        if (e->mu_img.upload(img_t.data(), img_t.size())) return -2;
        // ... and of k_pk_w's: the same midpoints, {mu^2, mu^4, mu^6, w} of the extra nodes
        for (int j = 0; j < e->n_extra; ++j) {
            const double m = mu[n_mu + j], m2 = m * m;
            double* q = &img[2 * (size_t)n_mu + 4 * (size_t)j];
            q[0] = m2; q[1] = m2 * m2; q[2] = m2 * m2 * m2; q[3] = node_w[j];
        }
        if (e->mu_img_w.upload(img.data(), img.size())) return -2;
    }
    if (e->mu.upload(mu.data(), n_rows) || e->sq1mmu2.upload(sq.data(), n_rows) || e->lnmu.upload(lnm.data(), n_rows) || e->wl.upload(wl.data(), wl.size())) return -2;
    return 0;
}

int vmx_set_fftlog_padding(vmx_engine* e, int32_t n_left, int32_t n_right)
{
    REQUIRE(e && !e->finalized && e->nk == 0, "vmx_set_fftlog_padding (before vmx_set_template)");
    REQUIRE(n_left >= 0 && n_right >= 0 && n_left + n_right <= 16384, "vmx_set_fftlog_padding: pad lengths");
    e->pad_l = n_left; e->pad_r = n_right;
    return 0;
}

int vmx_set_fftlog(vmx_engine* e, int32_t ell_index, const double* op, int32_t n_coef, double x0, double h,
                   int32_t n_knots)
{
    REQUIRE(e && !e->finalized && e->nk > 0, "set the template first");
    REQUIRE(ell_index >= 0 && ell_index < VMX_MAX_ELL, "ell_index out of range");
    REQUIRE(n_coef == n_knots + 2 && n_knots >= 4, "n_coef must be n_knots + 2");
    HIP_OK(hipSetDevice(e->device));
    const int ncp = vmx_pad(n_coef);
    if (e->op.p == nullptr) {
        e->n_coef = n_coef; e->ncp = ncp; e->n_knots = n_knots;
        if (e->op.alloc((size_t)VMX_MAX_ELL * ncp * e->nkp, true)) return -2;
    }
    REQUIRE(n_coef == e->n_coef, "all multipoles must share the knot count");
    const size_t width = (size_t)(e->nk + e->pad_l + e->pad_r) * sizeof(double);       // samples [| left pads | right pads]
    HIP_OK(hipMemcpy2D(e->op.p + (size_t)ell_index * ncp * e->nkp, (size_t)e->nkp * sizeof(double), op, width, width, n_coef,
                       hipMemcpyHostToDevice));
    e->x0[ell_index] = x0; e->h[ell_index] = h; e->op_set[ell_index] = true;
    return 0;
}

int vmx_set_spline_extrapolation(vmx_engine* e, int32_t enabled)
{
    REQUIRE(e && !e->finalized, "vmx_set_spline_extrapolation");
    e->extrapolate = enabled != 0;
    return 0;
}

int vmx_set_fvoigt_table(vmx_engine* e, const double* x, const double* f, int32_t n)
{
    REQUIRE(e && !e->finalized && x && f && n >= 2, "vmx_set_fvoigt_table");
    for (int i = 1; i < n; ++i) REQUIRE(x[i] > x[i - 1], "the fvoigt table abscissae must be increasing");
    HIP_OK(hipSetDevice(e->device));
    if (e->fv_x.upload(x, n) || e->fv_f.upload(f, n)) return -2;
    e->fv_n = n;
    return 0;
}

int vmx_add_gk_table_mock(vmx_engine* e, double bin_size_rp, double bin_size_rt, double mock_size_rp, double mock_size_rt)
{
    if (!e || e->finalized || e->nk == 0) return fail(-1, "invalid argument: set the template first");
    for (size_t i = 0; i < e->gk_tables.size(); ++i) {
        const auto& g = e->gk_tables[i];
        if (g.rp == bin_size_rp && g.rt == bin_size_rt && g.mock_rp == mock_size_rp && g.mock_rt == mock_size_rt) return (int)i;
    }
    e->gk_tables.push_back({bin_size_rp, bin_size_rt, mock_size_rp, mock_size_rt});
    return (int)e->gk_tables.size() - 1;
}

int vmx_add_gk_table(vmx_engine* e, double bin_size_rp, double bin_size_rt)
{
    return vmx_add_gk_table_mock(e, bin_size_rp, bin_size_rt, 0.0, 0.0);
}

int vmx_add_pipeline(vmx_engine* e, const vmx_pipe_desc* desc, int32_t n, const double* r, const double* mu,
                     const double* z, const double* rel_z_evol, const double* xi_growth)
{
    if (!e || e->finalized || !desc || n <= 0) return fail(-1, "invalid argument: vmx_add_pipeline");
    if (desc->n_ell < 1 || desc->n_ell > VMX_MAX_ELL) return fail(-1, "invalid argument: n_ell");
    if (desc->gk_table >= (int)e->gk_tables.size()) return fail(-1, "invalid argument: gk_table id");
    if (desc->mock_los_slot >= 0 && !(desc->mock_los_size > 0.0)) return fail(-1, "invalid argument: mock_los_size");
    if (desc->n_smooth < 0 || desc->n_smooth > VMX_MAX_SMOOTH) return fail(-1, "invalid argument: n_smooth");
    PipeDev p{};
    p.d = *desc;
    p.poly_basis = -1; p.col = -1; p.poly_bins_off = -1; p.odd_dyn_off = -1;
    // The P(k) stage is symmetric in the two tracers: keep the Lya-like tracer first (and a discrete
    // tracer last) so that the specialised mu loops see one canonical order.
    if (!p.d.same_tracer && ((!p.d.tracer[0].is_lya && p.d.tracer[1].is_lya) ||
                             (p.d.tracer[0].is_lya == p.d.tracer[1].is_lya && p.d.tracer[0].discrete &&
                              !p.d.tracer[1].discrete))) {
        std::swap(p.d.tracer[0], p.d.tracer[1]);
        p.tracers_swapped = 1;
    }
    p.n = n;
    p.coord_off = (int64_t)e->h_r.size();
    e->h_r.insert(e->h_r.end(), r, r + n);
    e->h_mu_c.insert(e->h_mu_c.end(), mu, mu + n);
    e->h_z.insert(e->h_z.end(), z, z + n);
    e->h_relz.insert(e->h_relz.end(), rel_z_evol, rel_z_evol + n);
    for (int i = 0; i < n; ++i) { e->h_lnrelz.push_back(std::log(rel_z_evol[i])); e->h_lnrelz2.push_back(std::log(rel_z_evol[i])); }
    // extremes of |rp| and rt over the bins with r != 0: k_prologue bounds the rescaled separations with them
    p.rp_absmin = 1e300; p.rp_absmax = 0.0; p.rt_min = 1e300; p.rt_max = 0.0;
    for (int i = 0; i < n; ++i) {
        if (r[i] == 0.0) continue;
        const double rp = std::fabs(r[i] * mu[i]), rt = r[i] * std::sqrt(std::max(0.0, 1.0 - mu[i] * mu[i]));
        p.rp_absmin = std::min(p.rp_absmin, rp); p.rp_absmax = std::max(p.rp_absmax, rp);
        p.rt_min = std::min(p.rt_min, rt); p.rt_max = std::max(p.rt_max, rt);
    }
    if (p.rp_absmin > p.rp_absmax) { p.rp_absmin = 0.0; p.rt_min = 0.0; }       // no bin with r != 0
    e->h_growth.insert(e->h_growth.end(), xi_growth, xi_growth + n);
    e->pipes.push_back(p);
    return (int)e->pipes.size() - 1;
}

int vmx_pipeline_set_tracer_evolution(vmx_engine* e, int32_t pipeline, const double* rel_z_1, const double* rel_z_2, int32_t n)
{
    REQUIRE(e && !e->finalized && rel_z_1 && rel_z_2, "vmx_pipeline_set_tracer_evolution");
    REQUIRE(pipeline >= 0 && pipeline < (int)e->pipes.size(), "pipeline id");
    PipeDev& p = e->pipes[pipeline];
    REQUIRE(n == p.n, "tracer evolution size");
    REQUIRE(p.d.tracer[0].evol_kind == VMX_EVOL_STD && p.d.tracer[1].evol_kind == VMX_EVOL_STD,
            "Croom model is not supported with new bias evol");
    // vmx_add_pipeline may have swapped the tracers into its canonical order
    const bool swapped = p.tracers_swapped != 0;
    for (int i = 0; i < n; ++i) {
        e->h_lnrelz[(size_t)p.coord_off + i] = std::log((swapped ? rel_z_2 : rel_z_1)[i]);
        e->h_lnrelz2[(size_t)p.coord_off + i] = std::log((swapped ? rel_z_1 : rel_z_2)[i]);
    }
    p.split_evol = 1;
    return 0;
}

int vmx_pipeline_set_odd_terms(vmx_engine* e, int32_t pipeline, const double* coef, int32_t n_coef, double x0,
                               double h, int32_t relativistic, int32_t asymmetry, const int32_t* slots)
{
    REQUIRE(e && !e->finalized && coef && slots, "vmx_pipeline_set_odd_terms");
    REQUIRE(pipeline >= 0 && pipeline < (int)e->pipes.size(), "pipeline id");
    REQUIRE(n_coef >= 4 && h > 0.0, "spline description");
    PipeDev& p = e->pipes[pipeline];
    p.odd_rel = relativistic != 0; p.odd_asy = asymmetry != 0; p.odd_ncoef = n_coef;
    p.odd_x0 = x0; p.odd_h = h;
    for (int i = 0; i < 5; ++i) {
        const bool needed = (i < 2) ? p.odd_rel : p.odd_asy;
        REQUIRE(!needed || slots[i] >= 0, "amplitude slot of an odd-multipole term");
        p.odd_slot[i] = slots[i];
    }
    p.odd_off = (int64_t)e->h_odd.size();
    p.odd_dyn_off = -1; p.odd_dyn_ld = 0;
    e->h_odd.insert(e->h_odd.end(), coef, coef + (size_t)4 * n_coef);
    return 0;
}

int vmx_pipeline_set_odd_operator(vmx_engine* e, int32_t pipeline, const double* op, int32_t n_coef, int32_t nk)
{
    REQUIRE(e && !e->finalized && op, "vmx_pipeline_set_odd_operator (before vmx_finalize)");
    REQUIRE(pipeline >= 0 && pipeline < (int)e->pipes.size(), "pipeline id");
    PipeDev& p = e->pipes[pipeline];
    REQUIRE((p.odd_rel || p.odd_asy) && n_coef == p.odd_ncoef && nk == e->nk, "vmx_pipeline_set_odd_operator: after vmx_pipeline_set_odd_terms, same shapes");
    // rows [4 n_coef] of nkp doubles (zero tails): the operand layout of the product kernels
    const size_t rows = (size_t)4 * n_coef;
    e->odd_op_off[pipeline] = (int64_t)e->h_odd_op.size();
    e->h_odd_op.resize(e->h_odd_op.size() + rows * e->nkp, 0.0);
    double* dst = e->h_odd_op.data() + e->odd_op_off[pipeline];
    for (size_t r = 0; r < rows; ++r) std::copy(op + r * nk, op + (r + 1) * nk, dst + r * e->nkp);
    return 0;
}

int vmx_set_shotnoise_table(vmx_engine* e, const double* a, int32_t n, double tau0, double dtau)
{
    REQUIRE(e && !e->finalized && a && n >= 2 && dtau > 0.0, "vmx_set_shotnoise_table");
    HIP_OK(hipSetDevice(e->device));
    if (e->sn_a.upload(a, n)) return -2;
    e->sn_n = n; e->sn_tau0 = tau0; e->sn_dtau = dtau;
    return 0;
}

int vmx_item_set_additive_template(vmx_engine* e, int32_t item, const double* vec, int32_t n_model, int32_t slot,
                                   double default_amp)
{
    REQUIRE(e && !e->finalized && vec, "vmx_item_set_additive_template");
    REQUIRE(item >= 0 && item < (int)e->items.size(), "item id");
    ItemHost* it = e->items[item];
    REQUIRE(n_model == it->dev.d.n_model, "template size");
    HIP_OK(hipSetDevice(e->device));
    if (it->add_vec.upload(vec, n_model)) return -2;
    it->dev.add_vec = it->add_vec.p; it->dev.add_slot = slot; it->dev.add_default = default_amp;
    return 0;
}

int vmx_add_item(vmx_engine* e, const vmx_item_desc* desc)
{
    if (!e || e->finalized || !desc) return fail(-1, "invalid argument: vmx_add_item");
    const int np = (int)e->pipes.size();
    if (desc->pipe_peak < 0 || desc->pipe_peak >= np || desc->pipe_smooth < 0 || desc->pipe_smooth >= np)
        return fail(-1, "invalid argument: pipeline id");
    if (e->pipes[desc->pipe_peak].n != desc->n_model || e->pipes[desc->pipe_smooth].n != desc->n_model)
        return fail(-1, "invalid argument: core pipelines must have n_model bins");
    if (desc->bao_amp_slot < 0) return fail(-1, "invalid argument: bao_amp slot");
    auto* it = new ItemHost();
    it->dev.d = *desc;
    it->dev.n_model_pad = vmx_pad(desc->n_model);
    it->dev.n_dist_pad = vmx_pad(desc->n_dist);
    it->dev.metal_begin = (int)e->metals.size();
    it->dev.add_vec = nullptr; it->dev.add_slot = -1; it->dev.add_default = 0.0;
    e->items.push_back(it);
    return (int)e->items.size() - 1;
}

int vmx_item_add_metal(vmx_engine* e, int32_t item, const vmx_metal_desc* desc)
{
    REQUIRE(e && !e->finalized && desc, "vmx_item_add_metal");
    REQUIRE(item == (int)e->items.size() - 1, "metals must be added to the most recent item");
    REQUIRE(desc->pipeline >= -1 && desc->pipeline < (int)e->pipes.size(), "metal pipeline id");
    ItemHost* it = e->items[item];
    REQUIRE((int)it->metals.size() < VMX_MAX_METALS, "too many metals");
    auto* m = new MetalHost();
    m->dev.d = *desc;
    m->dev.mat_off = -1;
    m->dev.svec = nullptr;
    m->dev.basis = nullptr;
    it->metals.push_back(m);
    e->metals.push_back(m);
    it->dev.n_metals = (int)it->metals.size();
    return (int)it->metals.size() - 1;
}

int vmx_item_set_metal_static(vmx_engine* e, int32_t item, int32_t index, const double* xi, int32_t n_model)
{
    REQUIRE(e && !e->finalized && xi, "vmx_item_set_metal_static");
    REQUIRE(item >= 0 && item < (int)e->items.size(), "item id");
    ItemHost* it = e->items[item];
    REQUIRE(index >= 0 && index < (int)it->metals.size(), "metal index");
    REQUIRE(n_model == it->dev.d.n_model, "static metal correlation size");
    MetalHost* m = it->metals[index];
    REQUIRE(m->dev.d.pipeline == -1, "a static correlation replaces the pipeline: add the metal with pipeline = -1");
    HIP_OK(hipSetDevice(e->device));
    if (m->svec.upload(xi, (size_t)n_model)) return -2;
    m->dev.svec = m->svec.p;
    return 0;
}

int vmx_item_set_metal_basis(vmx_engine* e, int32_t item, int32_t index, const double* basis, int32_t n_model)
{
    REQUIRE(e && !e->finalized && basis, "vmx_item_set_metal_basis");
    REQUIRE(item >= 0 && item < (int)e->items.size(), "item id");
    ItemHost* it = e->items[item];
    REQUIRE(index >= 0 && index < (int)it->metals.size(), "metal index");
    REQUIRE(n_model == it->dev.d.n_model, "metal basis size");
    MetalHost* m = it->metals[index];
    REQUIRE(m->dev.d.pipeline == -1, "a static basis replaces the pipeline: add the metal with pipeline = -1");
    HIP_OK(hipSetDevice(e->device));
    if (upload_padded(m->basis, basis, 3, n_model, vmx_pad(n_model))) return -2;
    m->dev.basis = m->basis.p;
    return 0;
}

int vmx_set_parameter_transform(vmx_engine* e, const double* scale, const double* shift)
{
    REQUIRE(e && e->finalized, "vmx_set_parameter_transform");
    drop_lane(e);
    REQUIRE((scale == nullptr) == (shift == nullptr), "scale and shift are given together");
    HIP_OK(hipSetDevice(e->device));
    HIP_OK(hipStreamSynchronize(e->stream));
    e->blind_scale.clear(); e->blind_shift.clear();
    if (!scale) return 0;
    e->blind_scale.assign(scale, scale + e->n_params);
    e->blind_shift.assign(shift, shift + e->n_params);
    if (e->d_blind.n < (size_t)2 * e->n_params && e->d_blind.alloc((size_t)2 * e->n_params)) return -2;
    HIP_OK(hipMemcpy(e->d_blind.p, scale, (size_t)e->n_params * sizeof(double), hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(e->d_blind.p + e->n_params, shift, (size_t)e->n_params * sizeof(double), hipMemcpyHostToDevice));
    return 0;
}

int vmx_set_metal_beta_override(vmx_engine* e, int32_t enabled, double beta)
{
    REQUIRE(e && e->finalized, "vmx_set_metal_beta_override");
    drop_lane(e);
    e->dev.beta_override_on = enabled ? 1 : 0;
    e->dev.beta_override = beta;
    // captured graphs hold the previous value: drop them
    HIP_OK(hipSetDevice(e->device));
    HIP_OK(hipStreamSynchronize(e->stream));
    for (auto& g : e->graphs) (void)hipGraphExecDestroy(g.second);
    e->graphs.clear(); e->graph_route.clear();
    return 0;
}

int vmx_item_add_broadband(vmx_engine* e, int32_t item, int32_t position, int32_t func, int32_t n_coef,
                           const int32_t* slots, const double* basis, int32_t n)
{
    REQUIRE(e && !e->finalized, "vmx_item_add_broadband");
    REQUIRE(item >= 0 && item < (int)e->items.size(), "item id");
    REQUIRE(position >= 0 && position < 4, "position");
    ItemHost* it = e->items[item];
    REQUIRE(it->dev.n_bb[position] < VMX_MAX_BB, "too many broadband terms");
    const bool pre = position == VMX_BB_PRE_MUL || position == VMX_BB_PRE_ADD;
    REQUIRE(n == (pre ? it->dev.d.n_model : it->dev.d.n_dist), "broadband basis size");
    REQUIRE(func == VMX_BB_POLY || func == VMX_BB_SKY, "broadband func");
    REQUIRE(n_coef > 0 && n_coef <= 16, "at most 16 coefficients per broadband term");
    REQUIRE(func != VMX_BB_SKY || n_coef == 2, "sky term takes {scale, sigma}");
    BBTermDev& t = it->dev.bb[position][it->dev.n_bb[position]++];
    t.func = func; t.n_coef = n_coef;
    for (int i = 0; i < n_coef; ++i) { REQUIRE(slots[i] >= 0, "broadband slot"); t.slot[i] = slots[i]; }
    t.basis_off = (int64_t)e->h_bb.size();
    e->h_bb.insert(e->h_bb.end(), basis, basis + (size_t)n_coef * n);
    return 0;
}

int vmx_item_set_matrix(vmx_engine* e, int32_t item, int32_t kind, int32_t index, int32_t rows, int32_t cols,
                        const double* dense)
{
    REQUIRE(e && dense, "vmx_item_set_matrix");
    drop_lane(e);
    REQUIRE(item >= 0 && item < (int)e->items.size(), "item id");
    HIP_OK(hipSetDevice(e->device));
    ItemHost* it = e->items[item];
    if (kind == VMX_MAT_DISTORTION) {
        REQUIRE(!e->finalized, "distortion matrix must be set before vmx_finalize");
        REQUIRE(rows == it->dev.d.n_dist && cols == it->dev.d.n_model, "distortion matrix shape");
        REQUIRE(!it->has_csr, "the item already has a CSR distortion matrix");
        REQUIRE(gemm44_addressable(rows, it->dev.n_model_pad), "distortion matrix: " GEMM44_LIMIT_MSG);
        if (upload_padded(it->dm, dense, rows, cols, it->dev.n_model_pad)) return -2;
        it->has_dm = true;
    } else if (kind == VMX_MAT_INVCOV) {
        REQUIRE(it->has_mask, "set the mask before the inverse covariance");
        REQUIRE(rows == it->dev.n_masked && cols == rows, "inverse covariance shape");
        REQUIRE(gemm44_addressable(rows, it->dev.n_masked_pad), "inverse covariance: " GEMM44_LIMIT_MSG);
        const std::vector<double> half = half_form(dense, rows);
        e->quad_mat_dirty = true;
        if (e->finalized) {
            REQUIRE(it->has_cinv, "an identity inverse covariance cannot be replaced after vmx_finalize");
            HIP_OK(hipStreamSynchronize(e->stream));
            HIP_OK(hipMemcpy2D(it->cinv.p, (size_t)it->dev.n_masked_pad * sizeof(double), half.data(),
                               (size_t)cols * sizeof(double), (size_t)cols * sizeof(double), rows,
                               hipMemcpyHostToDevice));
        } else {
            if (upload_padded(it->cinv, half.data(), rows, cols, it->dev.n_masked_pad)) return -2;
            it->has_cinv = true;
        }
    } else if (kind == VMX_MAT_METAL) {
        REQUIRE(!e->finalized, "metal matrices must be set before vmx_finalize");
        REQUIRE(index >= 0 && index < (int)it->metals.size(), "metal index");
        MetalHost* m = it->metals[index];
        REQUIRE(m->dev.d.pipeline >= 0, "a static metal correlation takes no matrix");
        REQUIRE(rows == it->dev.d.n_model && cols == e->pipes[m->dev.d.pipeline].n, "metal matrix shape");
        REQUIRE(gemm44_addressable(rows, vmx_pad(cols)), "metal matrix: " GEMM44_LIMIT_MSG);
        if (upload_padded(m->mat, dense, rows, cols, vmx_pad(cols))) return -2;
        m->rows = rows; m->cols = cols;
        m->dev.mat_off = 0;
        m->dev.mat_ld = vmx_pad(cols);
    } else return fail(-1, "invalid argument: matrix kind");
    return 0;
}

int vmx_item_set_matrix_csr(vmx_engine* e, int32_t item, int32_t rows, int32_t cols, const int64_t* indptr,
                            const int32_t* indices, const double* values)
{
    REQUIRE(e && !e->finalized && indptr && indices && values, "vmx_item_set_matrix_csr (before vmx_finalize)");
    REQUIRE(item >= 0 && item < (int)e->items.size(), "item id");
    ItemHost* it = e->items[item];
    REQUIRE(rows == it->dev.d.n_dist && cols == it->dev.d.n_model, "distortion matrix shape");
    REQUIRE(!it->has_dm, "the item already has a dense distortion matrix");
    // validity and canonical form (vmx_plan.h: the set-up of the quadratic form scatters the rows - last write wins - where
    // the product adds them, so duplicates would disagree)
    if (const char* why = vmx_plan::csr_problem(rows, cols, indptr, indices); why[0]) return fail(-1, std::string("invalid argument: CSR matrix: ") + why);
    const int64_t nnz = indptr[rows];
    HIP_OK(hipSetDevice(e->device));
    if (it->csr_ptr.upload(indptr, (size_t)rows + 1) || it->csr_idx.upload(indices, (size_t)std::max<int64_t>(nnz, 1)) ||
        it->csr_val.upload(values, (size_t)std::max<int64_t>(nnz, 1))) return -2;
    it->csr_nnz = nnz; it->has_csr = true;
    return 0;
}

int vmx_item_set_metal_kron(vmx_engine* e, int32_t item, int32_t index, const double* a_rp, int32_t n_rp,
                            const double* b_rt, int32_t n_rt)
{
    REQUIRE(e && !e->finalized && a_rp, "vmx_item_set_metal_kron (before vmx_finalize)");
    REQUIRE(item >= 0 && item < (int)e->items.size(), "item id");
    ItemHost* it = e->items[item];
    REQUIRE(index >= 0 && index < (int)it->metals.size(), "metal index");
    MetalHost* m = it->metals[index];
    REQUIRE(m->dev.d.pipeline >= 0, "a static metal correlation takes no matrix");
    REQUIRE(n_rp > 0 && n_rt > 0 && n_rp * n_rt == it->dev.d.n_model && n_rp * n_rt == e->pipes[m->dev.d.pipeline].n,
            "Kronecker factors: n_rp * n_rt must be the item's (and the pair's) bin count");
    REQUIRE((size_t)(2 * n_rp * n_rt + std::max(n_rp * n_rp, n_rt * n_rt)) * sizeof(double) <= 160 * 1024,
            "Kronecker factors too large for the LDS kernel: pass the dense matrix instead");
    HIP_OK(hipSetDevice(e->device));
    if (m->kron_a.upload(a_rp, (size_t)n_rp * n_rp)) return -2;
    if (b_rt && m->kron_b.upload(b_rt, (size_t)n_rt * n_rt)) return -2;
    m->dev.kron_a = m->kron_a.p; m->dev.kron_b = b_rt ? m->kron_b.p : nullptr;
    m->dev.kron_nrp = n_rp; m->dev.kron_nrt = n_rt;
    m->dev.mat_off = 0;                 // "has a matrix": its product lives in the metal-product buffer
    return 0;
}

int vmx_item_set_mask(vmx_engine* e, int32_t item, const int32_t* idx, int32_t n_masked)
{
    REQUIRE(e && !e->finalized && idx, "vmx_item_set_mask");
    REQUIRE(item >= 0 && item < (int)e->items.size(), "item id");
    ItemHost* it = e->items[item];
    REQUIRE(n_masked > 0 && n_masked <= it->dev.d.n_dist, "mask size");
    HIP_OK(hipSetDevice(e->device));
    std::vector<int32_t> inv(it->dev.d.n_dist, -1);
    for (int i = 0; i < n_masked; ++i) {
        REQUIRE(idx[i] >= 0 && idx[i] < it->dev.d.n_dist && inv[idx[i]] < 0, "mask index");
        inv[idx[i]] = i;
    }
    it->mask_idx.assign(idx, idx + n_masked);
    if (it->inv_mask.upload(inv.data(), inv.size())) return -2;
    it->dev.n_masked = n_masked;
    it->dev.n_masked_pad = vmx_pad(n_masked);
    it->has_mask = true;
    return 0;
}

int vmx_item_set_data(vmx_engine* e, int32_t item, const double* masked_data, int32_t n_masked)
{
    REQUIRE(e && masked_data, "vmx_item_set_data");
    drop_lane(e);
    REQUIRE(item >= 0 && item < (int)e->items.size(), "item id");
    ItemHost* it = e->items[item];
    REQUIRE(it->has_mask && n_masked == it->dev.n_masked, "data size must match the mask");
    HIP_OK(hipSetDevice(e->device));
    e->quad_lin_dirty = true;
    if (it->has_data) {
        HIP_OK(hipStreamSynchronize(e->stream));
        HIP_OK(hipMemcpy(it->data.p, masked_data, (size_t)n_masked * sizeof(double), hipMemcpyHostToDevice));
    } else {
        if (it->data.upload(masked_data, n_masked)) return -2;
        it->has_data = true;
    }
    return 0;
}

int vmx_item_set_mock_pool(vmx_engine* e, int32_t item, const double* pool, int32_t n_mocks, int32_t n_masked)
{
    REQUIRE(e && e->finalized && pool, "vmx_item_set_mock_pool (after vmx_finalize)");
    drop_lane(e);
    REQUIRE(item >= 0 && item < (int)e->items.size(), "item id");
    ItemHost* it = e->items[item];
    REQUIRE(n_mocks > 0 && n_masked == it->dev.n_masked, "mock pool shape");
    HIP_OK(hipSetDevice(e->device));
    HIP_OK(hipStreamSynchronize(e->stream));
    if (it->mock_pool.upload(pool, (size_t)n_mocks * n_masked)) return -2;
    it->n_mocks = n_mocks;
    e->quad_lin_dirty = true;
    it->dev.mock_pool = it->mock_pool.p;
    // the item table lives in device memory: patch this item's entry
    HIP_OK(hipMemcpy(e->d_items.p + item, &it->dev, sizeof(ItemDev), hipMemcpyHostToDevice));
    return 0;
}

int vmx_item_set_mock_factor(vmx_engine* e, int32_t item, const double* chol, const double* fiducial, int32_t n_masked)
{
    REQUIRE(e && e->finalized && chol && fiducial, "vmx_item_set_mock_factor (after vmx_finalize)");
    REQUIRE(item >= 0 && item < (int)e->items.size(), "item id");
    ItemHost* it = e->items[item];
    REQUIRE(n_masked == it->dev.n_masked, "mock factor: [n_masked][n_masked]");
    HIP_OK(hipSetDevice(e->device));
    wait_lane(e);
    HIP_OK(hipStreamSynchronize(e->stream));
    const int nmp = it->dev.n_masked_pad;
    if (upload_padded(it->mc_chol, chol, n_masked, n_masked, nmp) || upload_padded(it->mc_fid, fiducial, 1, n_masked, nmp)) return -2;
    it->has_factor = true;
    return 0;
}

int vmx_item_get_mock_pool(vmx_engine* e, int32_t item, double* pool, int32_t n_mocks, int32_t n_masked)
{
    REQUIRE(e && e->finalized && pool, "vmx_item_get_mock_pool");
    REQUIRE(item >= 0 && item < (int)e->items.size(), "item id");
    ItemHost* it = e->items[item];
    REQUIRE(n_mocks > 0 && n_mocks <= it->n_mocks && n_masked == it->dev.n_masked && it->mock_pool.p, "mock pool shape");
    HIP_OK(hipSetDevice(e->device));
    wait_lane(e);
    HIP_OK(hipStreamSynchronize(e->stream));
    HIP_OK(hipMemcpy(pool, it->mock_pool.p, (size_t)n_mocks * n_masked * sizeof(double), hipMemcpyDeviceToHost));
    return 0;
}

int vmx_host_alloc(vmx_engine* e, void** out, int64_t bytes)
{
    REQUIRE(e && out && bytes > 0, "vmx_host_alloc");
    HIP_OK(hipSetDevice(e->device));
    void* p = nullptr;
    HIP_OK(hipHostMalloc(&p, (size_t)bytes, hipHostMallocDefault));
    e->host_allocs.push_back(p);
    *out = p;
    return 0;
}

int vmx_host_free(vmx_engine* e, void* p)
{
    REQUIRE(e && p, "vmx_host_free");
    auto it = std::find(e->host_allocs.begin(), e->host_allocs.end(), p);
    REQUIRE(it != e->host_allocs.end(), "vmx_host_free: not a buffer of vmx_host_alloc on this engine");
    HIP_OK(hipSetDevice(e->device));
    HIP_OK(hipStreamSynchronize(e->stream));       // (no copy out of it may still be queued)
    wait_lane(e);
    e->host_allocs.erase(it);
    HIP_OK(hipHostFree(p));
    return 0;
}

int vmx_set_mock_index(vmx_engine* e, const int32_t* index, int32_t B)
{
    REQUIRE(e && e->finalized, "vmx_set_mock_index (after vmx_finalize)");
    drop_lane(e);
    REQUIRE(B >= 0 && B <= e->max_batch, "batch exceeds max_batch");
    HIP_OK(hipSetDevice(e->device));
    for (int b = 0; b < e->max_batch; ++b) e->h_mock_index[b] = -1;
    if (index) {
        for (int b = 0; b < B; ++b) {
            for (auto* it : e->items) REQUIRE(index[b] < 0 || index[b] < it->n_mocks, "mock index exceeds the pool");
            e->h_mock_index[b] = index[b];
        }
    }
    HIP_OK(hipStreamSynchronize(e->stream));
    HIP_OK(hipMemcpy(e->mock_index.p, e->h_mock_index.data(), (size_t)e->max_batch * sizeof(int32_t), hipMemcpyHostToDevice));
    return 0;
}

int vmx_set_global_invcov(vmx_engine* e, const double* invcov, int32_t n)
{
    REQUIRE(e && invcov && n > 0, "vmx_set_global_invcov");
    drop_lane(e);
    HIP_OK(hipSetDevice(e->device));
    const std::vector<double> half = half_form(invcov, n);
    if (e->finalized) {
        REQUIRE(e->g_n == n, "global inverse covariance size changed");
        HIP_OK(hipStreamSynchronize(e->stream));
        HIP_OK(hipMemcpy2D(e->gcinv.p, (size_t)e->g_ld * sizeof(double), half.data(), (size_t)n * sizeof(double),
                           (size_t)n * sizeof(double), n, hipMemcpyHostToDevice));
        return 0;
    }
    e->g_n = n; e->g_ld = vmx_pad(n);
    return upload_padded(e->gcinv, half.data(), n, n, e->g_ld);
}

int vmx_add_prior(vmx_engine* e, int32_t slot, double mean, double sigma)
{
    REQUIRE(e && !e->finalized && slot >= 0 && sigma != 0.0, "vmx_add_prior");
    e->prior_slot.push_back(slot); e->prior_mean.push_back(mean); e->prior_sigma.push_back(sigma);
    return 0;
}

static int poly_basis_build(vmx_engine* e);
static int xi_sum_plan(vmx_engine* e);

int vmx_finalize(vmx_engine* e, int32_t n_params, int32_t max_batch)
{
    REQUIRE(e && !e->finalized, "vmx_finalize");
    REQUIRE(n_params > 0 && max_batch > 0, "n_params / max_batch");
    REQUIRE(e->nk > 0 && !e->pipes.empty() && !e->items.empty(), "template, pipelines and items are required");
    REQUIRE(e->items.size() <= 16, "at most 16 correlation items");
    REQUIRE(e->pipes.size() * sizeof(PipeDev) <= 48 * 1024, "too many pipelines for the prologue's descriptor stage");
    for (int i = 0; i < VMX_MAX_ELL; ++i) REQUIRE(e->op_set[i], "all four FFTLog operators are required");
    HIP_OK(hipSetDevice(e->device));
    const int Bm = max_batch;
    e->n_params = n_params; e->max_batch = Bm;
    // split-K slabs are re-read by the consumer kernels: at most 1024 walker rows of slabs per product (measured
    // best in the full chain, where the items overlap on separate streams and fill the chip anyway)
    e->slab_rows = Bm > 1024 ? Bm : 1024;
    e->fact_slab_rows = std::max(1024, std::min(4 * Bm, 8192));
    if (getenv("VMX_NO_GRAPH")) e->use_graphs = false;
    if (getenv("VMX_TRACE_HOST")) e->trace_host = true;
    {
        int cus = 256;
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, e->device) != hipSuccess || cus <= 0) { (void)hipGetLastError(); cus = 256; }
        e->quad_blocks = 2 * cus;
    }
    if (getenv("VMX_NO_TAB2")) e->no_tab2 = true;
    if (getenv("VMX_NO_CINV_TAPE")) e->no_cinv_tape = true;
    if (getenv("VMX_NO_QUAD_ROOT") || (!QUAD_ROOT_DEFAULT && !getenv("VMX_QUAD_ROOT"))) e->no_quad_root = true;
    if (getenv("VMX_QUAD_ROOT") && !std::strcmp(getenv("VMX_QUAD_ROOT"), "force")) e->force_quad_root = !e->no_quad_root;
    if (getenv("VMX_NO_PK_W")) e->no_pk_w = true;
    if (getenv("VMX_NO_HOST_REDUCE")) e->no_host_reduce = true;
    if (getenv("VMX_NO_XI_LEAN")) e->xi_lean = false;
    if (getenv("VMX_NO_XI_SUMS")) e->xi_sums = false;

    // every slot must index a theta column and the combinations the kernels rely on must be present
    auto slot_ok = [&](int s) { return s < n_params; };
    for (auto& p : e->pipes) {
        const vmx_pipe_desc& d = p.d;
        const int slots[] = {d.tracer[0].bias_slot, d.tracer[0].bias_eta_slot, d.tracer[0].beta_slot,
                             d.tracer[0].vd_sigma_slot, d.tracer[0].alpha_slot, d.tracer[1].bias_slot,
                             d.tracer[1].bias_eta_slot, d.tracer[1].beta_slot, d.tracer[1].vd_sigma_slot,
                             d.tracer[1].alpha_slot, d.growth_rate_slot, d.bias_gamma_slot, d.bias_prim_slot,
                             d.lambda_uv_slot, d.bias_gamma_e_slot, d.lambda_heii_slot, d.bias_hcd_slot,
                             d.beta_hcd_slot, d.l0_hcd_slot, d.sigma_nl_par_slot, d.sigma_nl_per_slot,
                             d.exp_par_slot, d.exp_per_slot, d.scale_slot[0], d.scale_slot[1], d.drp_slot,
                             d.croom_slot[0], d.croom_slot[1], d.mock_los_slot};
        for (int s : slots) REQUIRE(slot_ok(s), "pipeline slot exceeds n_params");
        for (int i = 0; i < 6; ++i) REQUIRE(slot_ok(d.arinyo_slot[i]), "arinyo slot exceeds n_params");
        for (int i = 0; i < d.n_smooth; ++i)
            REQUIRE(d.smooth_par_slot[i] >= 0 && d.smooth_per_slot[i] >= 0 && slot_ok(d.smooth_par_slot[i]) &&
                    slot_ok(d.smooth_per_slot[i]), "smoothing slot");
        for (int q = 0; q < 2; ++q) {
            const vmx_tracer& t = d.tracer[q];
            const int have = (t.bias_slot >= 0) + (t.bias_eta_slot >= 0) + (t.beta_slot >= 0);
            REQUIRE(have >= 2, "each tracer needs two of (bias, bias_eta, beta)");
            REQUIRE(t.evol_kind == VMX_EVOL_CROOM ? (d.croom_slot[0] >= 0 && d.croom_slot[1] >= 0) : t.alpha_slot >= 0,
                    "bias-evolution slot");
            REQUIRE(d.vd_kind == VMX_VD_NONE || !t.discrete || t.vd_sigma_slot >= 0, "velocity dispersion slot");
        }
        REQUIRE(!d.uvb || (d.bias_gamma_slot >= 0 && d.bias_prim_slot >= 0 && d.lambda_uv_slot >= 0), "UVB slots");
        REQUIRE(!d.heii || (d.bias_gamma_e_slot >= 0 && d.bias_prim_slot >= 0 && d.lambda_heii_slot >= 0), "HeII slots");
        REQUIRE(d.hcd_model == VMX_HCD_NONE || (d.bias_hcd_slot >= 0 && d.beta_hcd_slot >= 0), "HCD slots");
        REQUIRE(d.hcd_model != VMX_HCD_ROGERS || d.l0_hcd_slot >= 0, "L0_hcd slot");
        REQUIRE(d.hcd_model != VMX_HCD_FVOIGT || e->fv_n >= 2, "model-hcd = fvoigt needs vmx_set_fvoigt_table");
        REQUIRE(d.nl_model != VMX_NL_ARINYO || (d.arinyo_slot[0] >= 0 && d.arinyo_slot[2] >= 0 && d.arinyo_slot[3] >= 0 &&
                                                d.arinyo_slot[4] >= 0 && d.arinyo_slot[5] >= 0), "Arinyo slots");
        REQUIRE(!d.peak_nl || d.sigma_nl_par_slot >= 0 || d.sigma_nl_per_slot >= 0, "sigmaNL slots");
        REQUIRE((d.exp_par_slot >= 0) == (d.exp_per_slot >= 0), "exp smoothing slots");
        REQUIRE(d.scale_mode == VMX_SCALE_UNIT || (d.scale_slot[0] >= 0 && d.scale_slot[1] >= 0), "scale slots");
        if (d.radiation) for (int i = 0; i < 4; ++i) REQUIRE(d.rad_slot[i] >= 0 && slot_ok(d.rad_slot[i]), "radiation slots");
        if (d.uv_shotnoise) {
            for (int i = 0; i < 3; ++i) REQUIRE(d.uvsn_slot[i] >= 0 && slot_ok(d.uvsn_slot[i]), "UV shot-noise slots");
            REQUIRE(e->sn_n >= 2, "UV shot noise needs vmx_set_shotnoise_table");
        }
    }
    for (auto* m : e->metals) {
        const vmx_metal_desc& d = m->dev.d;
        for (int q = 0; q < 2; ++q) {
            const vmx_tracer& t = d.tracer[q];
            REQUIRE(slot_ok(t.bias_slot) && slot_ok(t.bias_eta_slot) && slot_ok(t.beta_slot), "metal slot exceeds n_params");
            REQUIRE(!d.apply_bias || (t.bias_slot >= 0) + (t.bias_eta_slot >= 0) + (t.beta_slot >= 0) >= 2,
                    "each metal tracer needs two of (bias, bias_eta, beta)");
        }
        REQUIRE(slot_ok(d.growth_rate_slot) && slot_ok(d.extra_bias_slot), "metal slot exceeds n_params");
    }
    for (auto* it : e->items) {
        REQUIRE(slot_ok(it->dev.d.bao_amp_slot), "bao_amp slot exceeds n_params");
        REQUIRE(slot_ok(it->dev.add_slot), "additive-template slot exceeds n_params");
        for (int pos = 0; pos < 4; ++pos)
            for (int q = 0; q < it->dev.n_bb[pos]; ++q)
                for (int c = 0; c < it->dev.bb[pos][q].n_coef; ++c)
                    REQUIRE(slot_ok(it->dev.bb[pos][q].slot[c]), "broadband slot exceeds n_params");
    }

    // G(k) tables
    const size_t gk_stride = (size_t)e->n_rows * e->nkp;
    if (!e->gk_tables.empty()) {
        // (+ 16 rows: k_pk_w requests its table rows four steps ahead without checking for the end)
        if (e->gk.alloc(gk_stride * e->gk_tables.size() + (size_t)16 * e->nkp, true)) return -2;
        for (size_t t = 0; t < e->gk_tables.size(); ++t) {
            dim3 grid((e->nkp + 255) / 256, e->n_rows), block(256);
            hipLaunchKernelGGL(k_gk_table, grid, block, 0, e->stream, e->gk.p + t * gk_stride, e->k.p, e->mu.p,
                               e->nk, e->nkp, e->n_rows, e->gk_tables[t].rp, e->gk_tables[t].rt, e->gk_tables[t].mock_rp, e->gk_tables[t].mock_rt);
        }
        HIP_OK(hipGetLastError());
    }
    {
        const size_t nt = e->gk_tables.size();
        if (e->gk_mom.alloc((nt + 1) * 6 * (size_t)e->nkp, true)) return -2;
        for (size_t t = 0; t <= nt; ++t)
            hipLaunchKernelGGL(k_gk_moments, dim3((e->nkp + 63) / 64), dim3(64), 0, e->stream,
                               e->gk_mom.p + t * 6 * (size_t)e->nkp, t < nt ? e->gk.p + t * gk_stride : nullptr,
                               e->mu.p, e->nkp, e->n_mu);
        HIP_OK(hipGetLastError());
    }

    // coordinates and pipelines
    {
        std::vector<double> rp(e->h_r.size()), rt(e->h_r.size());
        for (size_t i = 0; i < rp.size(); ++i) {
            const double r = e->h_r[i], m = e->h_mu_c[i];
            rp[i] = r * m; rt[i] = r * std::sqrt(1.0 - m * m);        // correlation_func.py:216-217
        }
        if (e->crp.upload(rp.data(), rp.size()) || e->crt.upload(rt.data(), rt.size())) return -2;
    }
    if (e->cr.upload(e->h_r.data(), e->h_r.size()) || e->cmu.upload(e->h_mu_c.data(), e->h_mu_c.size()) ||
        e->cz.upload(e->h_z.data(), e->h_z.size()) || e->crelz.upload(e->h_relz.data(), e->h_relz.size()) ||
        e->clnrelz.upload(e->h_lnrelz.data(), e->h_lnrelz.size()) || e->clnrelz2.upload(e->h_lnrelz2.data(), e->h_lnrelz2.size()) ||
        e->cgrowth.upload(e->h_growth.data(), e->h_growth.size())) return -2;
    int64_t xi_off = 0;
    for (auto& p : e->pipes) { p.n_pad = vmx_pad(p.n); p.xi_off = xi_off; xi_off += (int64_t)Bm * p.n_pad; }
    e->xi_total = xi_off;
    const int n_pipe = (int)e->pipes.size();
    {
        // direct_pk with odd-multipole terms: where a pipeline's per-walker coefficient rows live (EngineDev::odd_dyn)
        int64_t off = 0;
        for (auto& kv : e->odd_op_off) {
            PipeDev& p = e->pipes[kv.first];
            p.odd_dyn_ld = vmx_pad(4 * p.odd_ncoef);
            p.odd_dyn_off = off;
            off += (int64_t)Bm * p.odd_dyn_ld;
        }
    }
    if (e->d_pipes.upload(e->pipes.data(), e->pipes.size())) return -2;

    // P(k,mu) work groups: an item's peak component rides along with its smooth component when the two
    // differ only by the peak broadening
    {
        std::vector<char> taken(e->pipes.size(), 0);
        e->pk_groups.clear();
        for (auto* it : e->items) {
            const int ps = it->dev.d.pipe_smooth, pk = it->dev.d.pipe_peak;
            if (ps != pk && !taken[ps] && !taken[pk] && pk_stage_compatible(e->pipes[ps].d, e->pipes[pk].d)) {
                e->pk_groups.push_back({ps, pk, 0, 0, 0, -1});
                taken[ps] = taken[pk] = 1;
            }
        }
        // unpaired pipelines: those without any amplitude-dependent mu structure (no HCD / UV-in-the-loop / NL)
        // that share the amplitude-free factor W are evaluated by one mu loop per shared-W group
        e->pk_members.clear();
        e->pk_poly.clear();
        for (int p = 0; p < (int)e->pipes.size(); ++p) {
            if (taken[p]) continue;
            const int variant = pk_variant(e->pipes[p].d, false);
            const bool plain = variant == PKV_PLAIN_SAME || variant == PKV_PLAIN_PAIR || variant == PKV_PLAIN_PAIR_VD;
            if (variant == PKV_POLY) { e->pk_poly.push_back(p); taken[p] = 1; continue; }
            if (!plain) { e->pk_groups.push_back({p, -1, variant, 0, 0, -1}); taken[p] = 1; continue; }
            PkGroup g{p, -1, PKV_SHARED_W, 0, (int32_t)e->pk_members.size(), -1};
            for (int q = p; q < (int)e->pipes.size(); ++q) {
                if (taken[q]) continue;
                const int vq = pk_variant(e->pipes[q].d, false);
                const bool plain_q = vq == PKV_PLAIN_SAME || vq == PKV_PLAIN_PAIR || vq == PKV_PLAIN_PAIR_VD;
                if (plain_q && w_stage_compatible(e->pipes[p].d, e->pipes[q].d)) {
                    e->pk_members.push_back(q); taken[q] = 1; ++g.n_members;
                }
            }
            e->pk_groups.push_back(g);
        }
        e->n_xtab = 0;
        e->const_slots.clear();
        e->const_slots2.clear();
        auto add_slot = [](std::vector<int32_t>& v, int slot) {
            if (slot >= 0 && std::find(v.begin(), v.end(), slot) == v.end()) v.push_back(slot);
        };
        for (auto& g : e->pk_groups) {
            if (g.peak_partner >= 0) g.variant = pk_variant(e->pipes[g.pipe].d, true);
            // core groups with the Arinyo term can run against per-batch tables (EngineDev::xtab_level)
            if (g.variant == PKV_AUTO_CORE || g.variant == PKV_CROSS_CORE) {
                g.xtab = e->n_xtab++;
                for (int i = 0; i < 6; ++i) add_slot(e->const_slots, e->pipes[g.pipe].d.arinyo_slot[i]);
                // level 2: whatever k_prologue forms ga / gb from, for the pipeline and its peak partner
                for (int pq : {g.pipe, g.peak_partner}) {
                    if (pq < 0) continue;
                    const vmx_pipe_desc& d = e->pipes[pq].d;
                    if (d.peak_nl) {
                        add_slot(e->const_slots2, d.sigma_nl_par_slot); add_slot(e->const_slots2, d.sigma_nl_per_slot);
                        if (d.sigma_nl_par_slot < 0 || d.sigma_nl_per_slot < 0) add_slot(e->const_slots2, d.growth_rate_slot);
                    }
                    for (int i = 0; i < d.n_smooth; ++i) { add_slot(e->const_slots2, d.smooth_par_slot[i]); add_slot(e->const_slots2, d.smooth_per_slot[i]); }
                    for (int q = 0; q < 2; ++q)
                        if (d.vd_kind == VMX_VD_GAUSS && d.tracer[q].discrete) add_slot(e->const_slots2, d.tracer[q].vd_sigma_slot);
                }
            }
        }
        for (int slot : e->const_slots) add_slot(e->const_slots2, slot);
        // two tables per group (level 2: the pipeline's and its peak partner's); + 4 x 32 rows: the mu loop requests its table
        // rows four steps ahead without checking for the end
        if (e->n_xtab > 0 && (e->xtab.alloc(((size_t)e->n_xtab * 2 * e->n_rows + 128) * e->nkp, true) ||
                              e->xtab_k.alloc((size_t)e->n_xtab * 4 * e->nkp, true))) return -2;
        {
            std::vector<int32_t> xp((size_t)e->n_xtab + 1, -1), xq((size_t)e->n_xtab + 1, -1);
            for (auto& g : e->pk_groups) if (g.xtab >= 0) { xp[g.xtab] = g.pipe; xq[g.xtab] = g.peak_partner; }
            e->tab2_groups.clear();
            for (int cross = 1; cross >= 0; --cross)
                for (auto& g : e->pk_groups) {
                    if (g.xtab < 0 || (g.variant == PKV_CROSS_CORE) != (cross == 1)) continue;
                    const vmx_pipe_desc& d = e->pipes[g.pipe].d;
                    Tab2Group t{};
                    t.pipe = g.pipe; t.partner = g.peak_partner; t.xtab = g.xtab; t.cross = cross;
                    t.kind_s = d.pk_lin_kind; t.kind_q = e->pipes[g.peak_partner].d.pk_lin_kind;
                    t.uvb = d.uvb; t.heii = d.heii; t.lya1 = d.tracer[0].is_lya; t.lya2 = d.tracer[1].is_lya;
                    t.damping_power = d.damping_power; t.damping_scale = d.damping_scale;
                    e->tab2_groups.push_back(t);          // (col_s / col_q: once the active columns are numbered)
                }
            std::vector<double> key((size_t)2 * e->n_xtab * VMX_XTAB_KEY + 1, std::nan(""));     // [held][seen by the running evaluation]
            if (e->d_xtab_pipe.upload(xp.data(), xp.size()) || e->d_xtab_partner.upload(xq.data(), xq.size()) ||
                e->xtab_key.upload(key.data(), key.size())) return -2;
            e->host_key_valid = false; e->pending_key.clear();
        }
        e->const_slots.push_back(-1);
        e->const_slots2.push_back(-1);
        if (e->d_const_slots.upload(e->const_slots.data(), e->const_slots.size()) ||
            e->d_const_slots2.upload(e->const_slots2.data(), e->const_slots2.size())) return -2;
        e->const_slots.pop_back();
        e->const_slots2.pop_back();
        e->pk_members.push_back(-1);
        if (e->d_pk_members.upload(e->pk_members.data(), e->pk_members.size())) return -2;
        // polynomial pipelines without any k-dependent walker term: their spline coefficients are linear in the Kaiser
        // coefficients with static vectors (k_poly_basis + the FFTLog operator, once) - no P(k,mu), no FFTLog column per
        // walker.  Every other pipeline gets a column of the P_ell / coefficient buffers.
        {
            std::vector<int32_t> keep;
            e->pk_static.clear();
            for (int p : e->pk_poly) {
                const vmx_pipe_desc& d = e->pipes[p].d;
                // (not with fht_extrap: the pads are not linear in P_ell)
                if (!d.uvb && !d.heii && !(d.damping_scale > 0.0) && e->static_poly && e->pad_l + e->pad_r == 0 && !getenv("VMX_NO_STATIC_POLY")) {
                    PipeDev& pd = e->pipes[p];
                    pd.poly_basis = (int32_t)e->pk_static.size();
                    e->pk_static.push_back(p);
                    // static coordinates as well (no rescaling, no delta_rp, no odd-multipole terms): the basis is
                    // evaluated on the bins once (k_poly_bins)
                    if (d.scale_mode == VMX_SCALE_UNIT && d.drp_slot < 0 && !pd.odd_rel && !pd.odd_asy && d.radiation != 2 &&
                        d.uv_shotnoise != 2 && !getenv("VMX_NO_STATIC_BINS")) {
                        pd.poly_bins_off = e->poly_bins_total;
                        e->poly_bins_total += (int64_t)3 * vmx_pad(pd.n);
                    }
                } else keep.push_back(p);
            }
            e->pk_poly.swap(keep);
            e->n_active = 0;
            for (auto& pd : e->pipes) {
                if (pd.poly_basis >= 0) pd.col = -1;
                else pd.col = e->n_active++;
            }
            for (auto& t : e->tab2_groups) { t.col_s = e->pipes[t.pipe].col; t.col_q = e->pipes[t.partner].col; }
            if (e->d_pipes.upload(e->pipes.data(), e->pipes.size())) return -2;
            e->pk_static.push_back(-1);
            if (e->d_pk_static.upload(e->pk_static.data(), e->pk_static.size())) return -2;
            e->pk_static.pop_back();
            std::vector<int32_t> active;
            for (int p = 0; p < (int)e->pipes.size(); ++p) if (e->pipes[p].col >= 0) active.push_back(p);
            // ... of which k_xi_bins_lean takes those that are a spline sum with the standard evolution (+ radiation)
            e->xi_lean_pipes.clear(); e->xi_rest_pipes.clear();
            for (int p : active) {
                const PipeDev& P = e->pipes[p];
                const vmx_pipe_desc& d = P.d;
                const bool lean = e->xi_lean && !e->extrapolate && d.tracer[0].evol_kind == VMX_EVOL_STD && d.tracer[1].evol_kind == VMX_EVOL_STD &&
                                  !d.uv_shotnoise && !P.odd_rel && !P.odd_asy && d.single_ell < 0 && (!d.radiation || !d.is_peak) &&      // (the radiating pair's peak: faster by the general kernel)
                                  (int)e->xi_lean_pipes.size() < VMX_XI_LEAN_MAX;
                (lean ? e->xi_lean_pipes : e->xi_rest_pipes).push_back(p);
            }
            {
                std::vector<int32_t> rest = e->xi_rest_pipes;
                rest.push_back(-1);
                if (e->d_xi_rest_pipes.upload(rest.data(), rest.size())) return -2;
            }
            active.push_back(-1);
            if (e->d_pipe_active.upload(active.data(), active.size())) return -2;
        }
        e->pk_poly.push_back(-1);
        if (e->d_pk_poly.upload(e->pk_poly.data(), e->pk_poly.size())) return -2;
        e->pk_poly.pop_back();
        if (e->d_pk_groups.upload(e->pk_groups.data(), e->pk_groups.size())) return -2;
        {
            e->w_groups.clear();
            for (size_t gi = 0; gi < e->pk_groups.size(); ++gi) if (e->pk_groups[gi].variant == PKV_SHARED_W) e->w_groups.push_back((int32_t)gi);
            std::vector<int32_t> wl = e->w_groups;
            wl.push_back(-1);
            if (e->d_w_groups.upload(wl.data(), wl.size())) return -2;
        }
    }

    // metals
    int64_t xim_off = 0;
    std::vector<MetalDev> metals;
    for (auto* it : e->items)
        for (auto* m : it->metals) {
            REQUIRE(m->dev.d.pipeline >= 0 || m->dev.svec || m->dev.basis, "metal without pipeline and without static correlation");
            if (m->dev.mat_off >= 0) { m->dev.xim_off = xim_off; xim_off += (int64_t)Bm * it->dev.n_model_pad; }
            metals.push_back(m->dev);
        }
    e->xim_total = xim_off;
    metals.push_back(MetalDev{});
    if (e->d_metals.upload(metals.data(), metals.size())) return -2;

    // items
    int64_t model_off = 0, masked_off = 0;
    std::vector<ItemDev> items;
    for (auto* it : e->items) {
        REQUIRE(it->has_mask && it->has_data, "every item needs a mask and a data vector");
        ItemDev& d = it->dev;
        d.model_off = model_off; model_off += d.d.n_dist;
        d.masked_off = masked_off; masked_off += d.n_masked;
        REQUIRE(it->has_dm || it->has_csr || d.d.n_dist == d.d.n_model, "identity distortion needs n_dist == n_model");
        if (it->vec.alloc((size_t)Bm * d.n_model_pad, true)) return -2;
        if (it->res.alloc((size_t)Bm * d.n_masked_pad, true)) return -2;
        if ((it->has_dm || it->has_csr) && it->dist.alloc((size_t)e->slab_rows * d.n_dist_pad, true)) return -2;
        if (it->has_cinv && it->z.alloc((size_t)e->slab_rows * d.n_masked_pad, true)) return -2;
        d.dm = it->has_dm ? it->dm.p : nullptr; d.dm_ld = d.n_model_pad;
        d.dm_ptr = it->has_csr ? it->csr_ptr.p : nullptr; d.dm_idx = it->csr_idx.p; d.dm_val = it->csr_val.p;
        d.cinv = it->has_cinv ? it->cinv.p : nullptr; d.cinv_ld = d.n_masked_pad;
        d.inv_mask = it->inv_mask.p; d.data = it->data.p;
        d.vec = it->vec.p; d.dist = it->dist.p; d.res = it->res.p; d.z = it->z.p;
        items.push_back(d);
    }
    e->model_size = (int)model_off;
    if (e->d_items.upload(items.data(), items.size())) return -2;
    if (e->gcinv.p) {
        REQUIRE(e->g_n == (int)masked_off, "global inverse covariance size must equal the total masked size");
        if (e->gres.alloc((size_t)Bm * e->g_ld, true) || e->gz.alloc((size_t)e->slab_rows * e->g_ld, true)) return -2;
    }

    if (e->bb_basis.upload(e->h_bb.data(), e->h_bb.size() ? e->h_bb.size() : 0)) return -2;
    if (e->odd_coef.upload(e->h_odd.data(), e->h_odd.size())) return -2;
    if (!e->h_odd_op.empty()) {
        // direct_pk with odd-multipole terms: the operators, and the walkers' coefficient rows [pipelines with one][Bm][ld]
        if (e->odd_op.upload(e->h_odd_op.data(), e->h_odd_op.size())) return -2;
        int64_t total = 0;
        for (auto& kv : e->odd_op_off) total += (int64_t)Bm * e->pipes[kv.first].odd_dyn_ld;       // (offsets: set with the descriptors above)
        if (e->odd_dyn.alloc((size_t)total, true)) return -2;
    }
    for (auto& p : e->pipes)
        for (int i = 0; i < 5; ++i) REQUIRE(p.odd_slot[i] < n_params, "odd-multipole slot exceeds n_params");
    if (!e->prior_slot.empty()) {
        for (int s : e->prior_slot) REQUIRE(s < n_params, "prior slot exceeds n_params");
        if (e->d_prior_slot.upload(e->prior_slot.data(), e->prior_slot.size()) ||
            e->d_prior_mean.upload(e->prior_mean.data(), e->prior_mean.size()) ||
            e->d_prior_sigma.upload(e->prior_sigma.data(), e->prior_sigma.size())) return -2;
    }

    // workspace (pad regions are zeroed once here and never written afterwards)
    const size_t ncols = (size_t)Bm * n_pipe, acols = (size_t)Bm * std::max(e->n_active, 1);
    if (e->theta.alloc((size_t)Bm * n_params) || e->scal.alloc(ncols * VMX_NS) ||
        e->metal_bias.alloc((size_t)Bm * 3 * (e->metals.size() + 1)) ||
        e->pl.alloc((size_t)VMX_MAX_ELL * acols * e->nkp) || e->coef.alloc((size_t)VMX_MAX_ELL * acols * e->ncp) ||
        e->xi.alloc((size_t)e->xi_total) || e->xim.alloc((size_t)e->xim_total) ||
        e->model.alloc((size_t)Bm * e->model_size) || e->chi2.alloc(Bm) || e->status.alloc(Bm) || e->k_live.alloc(8)) return -2;
    {
        const int32_t empty_window[2] = {0x7fffffff, -1};
        if (e->coef_win.upload(empty_window, 2)) return -2;
    }
    e->h_mock_index.assign(Bm, -1);
    if (e->mock_index.upload(e->h_mock_index.data(), Bm)) return -2;

    EngineDev& D = e->dev;
    D = EngineDev{};
    D.nk = e->nk; D.nkp = e->nkp; D.n_mu = e->n_mu; D.n_ell = VMX_MAX_ELL;
    D.pad_l = e->pad_l; D.pad_r = e->pad_r; D.pipe_active = e->d_pipe_active.p;
    D.n_rows = e->n_rows; D.n_extra = e->n_extra; D.mu_lo = e->mu_lo; D.mu_hi = e->mu_hi; D.node_w = e->node_w.p; D.mu_img = e->mu_img.p; D.mu_img_w = e->mu_img_w.p;
    {
        // the node rule needs the integrand smooth on the scale of its panels: the binning sincs oscillate with k x bin
        // size, so wavenumbers beyond 24 / (largest bin size) [6 h/Mpc for 4 Mpc/h bins] keep the midpoint loop
        double size = 4.0;
        for (auto& g : e->gk_tables) size = std::max(std::max(size, g.rp), std::max(g.rt, std::max(g.mock_rp, g.mock_rt)));
        e->k_node_max = 24.0 / size;
        if (getenv("VMX_EXACT_MU") || e->n_extra == 0) e->mu_nodes_on = false;
        D.k_node_max = e->mu_nodes_on ? e->k_node_max : 0.0;
        // which k tile of k_pk_tab2 takes which tier, and the launch order of the tiles (vmx_plan.h)
        for (int t = 0; t < vmx_plan::MU_TIERS; ++t) D.mu_tier[t] = e->mu_tier[t];
        e->zmap64 = vmx_plan::plan_mu_tiles(e->h_k.data(), e->nk, 64, e->k_node_max, e->mu_tiers, VMX_TAB2_ZMAP);
        e->zmap16 = vmx_plan::plan_mu_tiles(e->h_k.data(), e->nk, 16, e->k_node_max, e->mu_tiers, VMX_TAB2_ZMAP);
    }
    for (int sl : e->rule_slot) REQUIRE(sl < n_params, "mu-rule box slot exceeds n_params");
    if (!e->rule_slot.empty() && (e->d_rule_slot.upload(e->rule_slot.data(), e->rule_slot.size()) ||
                                  e->d_rule_lo.upload(e->rule_lo.data(), e->rule_lo.size()) ||
                                  e->d_rule_hi.upload(e->rule_hi.data(), e->rule_hi.size()))) return -2;
    D.rule_slot = e->d_rule_slot.p; D.rule_lo = e->d_rule_lo.p; D.rule_hi = e->d_rule_hi.p; D.n_rule = (int)e->rule_slot.size();
    D.k = e->k.p; D.pklin = e->pklin.p; D.delta2 = e->delta2.p; D.mu = e->mu.p; D.sq1mmu2 = e->sq1mmu2.p; D.lnmu = e->lnmu.p;
    D.wl = e->wl.p; D.fv_x = e->fv_x.p; D.fv_f = e->fv_f.p; D.fv_n = e->fv_n; D.gk = e->gk.p; D.gk_mom = e->gk_mom.p; D.xtab = e->xtab.p; D.const_slots = e->d_const_slots.p; D.n_const_slots = 0; D.xtab_pipe = e->d_xtab_pipe.p; D.n_xtab = e->n_xtab; D.xtab_key = e->xtab_key.p; D.xtab_partner = e->d_xtab_partner.p; D.xtab_k = e->xtab_k.p; D.xtab_level = 0; D.n_gk = (int)e->gk_tables.size();
    D.n_coef = e->n_coef; D.ncp = e->ncp; D.extrapolate = e->extrapolate ? 1 : 0;
    for (int i = 0; i < VMX_MAX_ELL; ++i) {
        D.x0[i] = e->x0[i]; D.h[i] = e->h[i]; D.inv_h[i] = 1.0 / e->h[i]; D.xlast[i] = e->x0[i] + e->h[i] * (e->n_knots - 1);
    }
    D.same_grid = 1;
    for (int i = 1; i < VMX_MAX_ELL; ++i)
        if (e->op_set[i] && (!e->op_set[0] || D.x0[i] != D.x0[0] || D.inv_h[i] != D.inv_h[0] || D.xlast[i] != D.xlast[0])) D.same_grid = 0;
#ifdef VMX_EXP_NO_SAME_GRID           // (experiment build: the per-multipole instances on a common grid - scripts/gpu_same_grid.py checks the bits)
    D.same_grid = 0;
#endif
    D.n_pipe = n_pipe; D.pipes = e->d_pipes.p;
    D.n_active = e->n_active; D.n_static = (int)e->pk_static.size();
    if (!e->pk_static.empty() && e->poly_coef.alloc((size_t)VMX_MAX_ELL * e->pk_static.size() * 3 * e->ncp, true)) return -2;
    D.poly_coef = e->poly_coef.p;
    if (e->poly_bins_total > 0 && e->poly_bins.alloc((size_t)e->poly_bins_total, true)) return -2;
    D.poly_bins = e->poly_bins.p;
    D.cr = e->cr.p; D.cmu = e->cmu.p; D.crp = e->crp.p; D.crt = e->crt.p; D.cz = e->cz.p; D.crelz = e->crelz.p; D.clnrelz = e->clnrelz.p; D.clnrelz2 = e->clnrelz2.p; D.cgrowth = e->cgrowth.p;
    D.n_items = (int)e->items.size(); D.items = e->d_items.p;
    D.metals = e->d_metals.p; D.n_metals_total = (int)e->metals.size();
    D.bb_basis = e->bb_basis.p;
    D.odd_coef = e->odd_coef.p; D.odd_dyn = e->odd_dyn.p;
    D.sn_a = e->sn_a.p; D.sn_n = e->sn_n; D.sn_tau0 = e->sn_tau0; D.sn_dtau = e->sn_dtau;
    D.n_priors = (int)e->prior_slot.size();
    D.prior_slot = e->d_prior_slot.p; D.prior_mean = e->d_prior_mean.p; D.prior_sigma = e->d_prior_sigma.p;
    D.n_params = n_params;
    D.theta = e->theta.p; D.scal = e->scal.p; D.metal_bias = e->metal_bias.p; D.pl = e->pl.p; D.coef = e->coef.p;
    D.xi = e->xi.p; D.xim = e->xim.p; D.model = e->model.p; D.chi2 = e->chi2.p; D.status = e->status.p; D.k_live = e->k_live.p; D.coef_win = e->coef_win.p; D.pk_trace = nullptr; D.mock_index = e->mock_index.p;
    D.model_size = e->model_size;
    D.gcinv = e->gcinv.p; D.g_n = e->g_n; D.g_ld = e->g_ld; D.gres = e->gres.p; D.gz = e->gz.p;

    for (size_t q = 1; q < e->items.size(); ++q) {
        hipStream_t st = nullptr; hipEvent_t ev = nullptr;
        HIP_OK(hipStreamCreate(&st));
        HIP_OK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
        e->aux.push_back(st); e->ev_join.push_back(ev);
    }
    HIP_OK(hipEventCreateWithFlags(&e->ev_fork, hipEventDisableTiming));

    HIP_OK(hipHostMalloc((void**)&e->pin_theta, (size_t)Bm * n_params * sizeof(double), hipHostMallocMapped));
    HIP_OK(hipHostMalloc((void**)&e->pin_chi2, (size_t)Bm * sizeof(double), hipHostMallocMapped));
    HIP_OK(hipHostMalloc((void**)&e->pin_status, (size_t)Bm * sizeof(int32_t), hipHostMallocMapped));
    HIP_OK(hipHostMalloc((void**)&e->pin_done, sizeof(int64_t), hipHostMallocMapped));
    *e->pin_done = 0;
    if (hipHostMalloc((void**)&e->pin_part, (size_t)VMX_MAX_GROUP * 1024 * sizeof(double), hipHostMallocMapped) != hipSuccess ||
        hipHostGetDevicePointer((void**)&e->dpin_part, e->pin_part, 0) != hipSuccess) { (void)hipGetLastError(); e->dpin_part = nullptr; }
    if (getenv("VMX_NO_DONE_WORD") || hipHostGetDevicePointer((void**)&e->dpin_done, e->pin_done, 0) != hipSuccess) { (void)hipGetLastError(); e->dpin_done = nullptr; }
    if (!getenv("VMX_NO_ZERO_COPY") &&
        (hipHostGetDevicePointer((void**)&e->dpin_theta, e->pin_theta, 0) != hipSuccess ||
         hipHostGetDevicePointer((void**)&e->dpin_chi2, e->pin_chi2, 0) != hipSuccess ||
         hipHostGetDevicePointer((void**)&e->dpin_status, e->pin_status, 0) != hipSuccess)) {
        (void)hipGetLastError();
        e->dpin_theta = nullptr; e->dpin_chi2 = nullptr; e->dpin_status = nullptr;     // staging copies instead
    }

    // the quadratic form of chi2 needs a model that is linear in [x ; additive post-distortion coefficients]
    e->quad_eligible = e->gcinv.p == nullptr && e->items.size() <= 16;
    for (auto* it : e->items) {
        int na = 0;
        if (it->dev.n_bb[VMX_BB_POST_MUL]) e->quad_eligible = false;
        for (int q = 0; q < it->dev.n_bb[VMX_BB_POST_ADD]; ++q) {
            if (it->dev.bb[VMX_BB_POST_ADD][q].func != VMX_BB_POLY) e->quad_eligible = false;
            na += it->dev.bb[VMX_BB_POST_ADD][q].n_coef;
        }
        if (na > VMX_MAX_QUAD_COEF) e->quad_eligible = false;
    }
    if (getenv("VMX_NO_QUAD")) e->quad_eligible = false;

    HIP_OK(hipStreamSynchronize(e->stream));
    e->finalized = true;
    if (poly_basis_build(e) || xi_sum_plan(e)) { e->finalized = false; return -2; }
    return 0;
}

int vmx_model_size(vmx_engine* e) { return e ? e->model_size : -1; }

int vmx_pipeline_column(vmx_engine* e, int32_t pipeline)
{
    REQUIRE(e && e->finalized && pipeline >= 0 && pipeline < (int)e->pipes.size(), "vmx_pipeline_column");
    return e->pipes[pipeline].col >= 0 ? e->pipes[pipeline].col : -3 - e->n_active;     // (< -2: no column; the count is -3 - value)
}

// The quadratic-form launch as a persistent tape ("stream-K"): the cut, the slot numbering and the block queues are planned by
// vmx_plan::plan_quad_tape (vmx_plan.h - plain C++, run under sanitizers by tests/test_planner_host.py), a pure function of
// (problem shapes, walker tiles, blocks).
// cost of starting / finishing an entry in K stages (fitted from the block trace: duration = 1.98 us stages + 7.3 us entries
// + 9.8), and the share of a piece moved from the blocks dispatched second to those dispatched first (B = 256: 145.1 us at 0,
// 142.6 at 0.12 - 0.16, 144.0 at 0.2, 149.6 at 0.4)
constexpr double QUAD_ENTRY_STAGES = 4.0, QUAD_SKEW = 0.12;
// The tape over the trapezoidal roots (vmx_plan::TapeProblem::k_off > 0): its entries end with the plain store of their partial
// tile - no E tile to wait for, no row sums - so an entry is charged less than a contraction's; a K stage at 1.98 us and the
// reducer's reads of the partial tiles at ~3 TB/s (+ 2 stages for what it costs beyond k_chi2_parts) price it against the triangle.
constexpr double QUAD_ROOT_ENTRY_STAGES = 2.5, QUAD_STAGE_US = 1.98, QUAD_ROOT_BYTES_PER_US = 3.0e6, QUAD_ROOT_REDUCER_STAGES = 2.0;
// The equal-cost pieces of the tape are dealt to the XCDs by their place in K (the heavy and the light ones separately, so that
// the skew keeps its meaning): same pieces, same slots, the same sums bit for bit - 12 % fewer L2 misses of the walker operand
// (493 -> 435 MB per launch at B = 256), the same launch time with one batch in flight and ~1 % less with two (round 4).
constexpr bool QUAD_K_BANDS = true;

static vmx_engine::QuadList* quad_build_tape(vmx_engine* e, int B)
{
    const int tn = (B + GEMM_BN - 1) / GEMM_BN;
    std::vector<vmx_plan::TapeProblem> probs;
    for (auto* it : e->items) probs.push_back({it->dev.nq, it->dev.nq_pad});
    // (k_bands = false: dealing the pieces to the XCDs by their place in K takes 12 % off the launch's L2 misses - 493 -> 435 MB at
    // B = 256 - and nothing off its time: 151.4 us either way, round 4; the sums are the same bit for bit)
    vmx_plan::Tape T = vmx_plan::plan_quad_tape(probs, tn, e->quad_blocks, QUAD_ENTRY_STAGES, QUAD_SKEW, GEMM_BM, GEMM_BK, QUAD_K_BANDS);
    auto* ql = new vmx_engine::QuadList();
    if (e->quad_root && !e->no_quad_root) {
        // The same launch over the items' trapezoidal roots (|| L dx ||^2 instead of 2 dx^T (L' dx)): fewer K stages when n_masked <
        // nq, but its entries store partial tiles that k_chi2_root reads back.  Both tapes are priced in K stages - a piece's
        // capacity is the launch's length - and the root pays for the reducer's traffic on top.
        std::vector<vmx_plan::TapeProblem> roots;
        for (auto* it : e->items) roots.push_back({it->dev.n_masked, it->dev.nq_pad, it->dev.nq - it->dev.n_masked});
        vmx_plan::Tape R = vmx_plan::plan_quad_tape(roots, tn, e->quad_blocks, QUAD_ROOT_ENTRY_STAGES, QUAD_SKEW, GEMM_BM, GEMM_BK, QUAD_K_BANDS, true);
        double bytes = 0.0;
        for (size_t q = 0; q < roots.size(); ++q)
            for (int t = R.tile_off[q]; t < R.tile_off[q + 1]; ++t)
                for (int nt = 0; nt < tn; ++nt) bytes += 8.0 * GEMM_BM * GEMM_BN * R.seg_count[(size_t)t * tn + nt];
        const double reducer_stages = bytes / QUAD_ROOT_BYTES_PER_US / QUAD_STAGE_US + QUAD_ROOT_REDUCER_STAGES;
        if ((R.capacity + reducer_stages < T.capacity || e->force_quad_root) && !R.work.empty()) {
            ql->root = true;
            ql->max_segs = R.max_segs;
            int64_t y = 0;
            for (size_t q = 0; q < roots.size(); ++q) {
                ql->y_off.push_back(y); ql->seg_off.push_back(R.tile_off[q] * tn);
                y += (int64_t)R.max_segs * tn * GEMM_BN * e->items[q]->dev.n_masked_pad;
            }
            if (ql->ypart.alloc((size_t)y, true) || ql->segs.upload(R.seg_count.data(), R.seg_count.size())) { delete ql; return nullptr; }
            T = std::move(R);
        }
    }
    ql->n_blocks = T.n_blocks;
    ql->n_entries = (int)T.n_slots;
    if (T.work.empty()) T.work.push_back(GemmWork{-1, 0, 0, 0, 0, 0, 0, 0});
    if (ql->work.upload(T.work.data(), T.work.size()) || ql->queue.upload(T.queue.data(), T.queue.size()) ||
        ql->nt_off.upload(T.nt_off.data(), T.nt_off.size()) ||
        ql->part.alloc(std::max<size_t>((size_t)T.n_slots, 1) * 128, true)) { delete ql; return nullptr; }
    return ql;
}

// the launch itself: every block walks its queue of the tape and leaves contraction partials in the tape's slots
static void quad_launch_list(vmx_engine* e, vmx_engine::QuadList* ql, int B)
{
    GemmGroup G{};
    for (size_t q = 0; q < e->items.size(); ++q) {
        ItemHost* it = e->items[q];
        const ItemDev& d = it->dev;
        GemmArgs g{};
        g.A = it->q_mat.p; g.lda = d.nq_pad; g.X = it->q_x.p; g.ldx = d.nq_pad; g.D = it->q_z.p; g.ldd = d.nq_pad;
        g.M = d.nq; g.N = B; g.K = d.nq_pad; g.tri = 1; g.nsplit = 1; g.klen = d.nq_pad;
        g.d_slab = (int64_t)B * d.nq_pad;
        g.tm = (d.nq + GEMM_BM - 1) / GEMM_BM; g.tn = (B + GEMM_BN - 1) / GEMM_BN;
        g.part = ql->part.p; g.lin = it->q_lin.p; g.lin_row = e->call_mock ? e->call_mock : e->mock_index.p; g.lin_pool = d.mock_pool ? 1 : 0;
        g.row0 = vmx_plan::tape_row0(d.nq, GEMM_BM);       // (the tape's K ranges are those of this tiling)
        if (ql->root) {
            // the trapezoidal root in place of the half form: n_masked rows, the partial tile of K segment s stored to slab s
            g.A = it->q_root.p; g.M = d.n_masked; g.tri = 0; g.part = nullptr;
            g.D = ql->ypart.p + ql->y_off[q]; g.ldd = d.n_masked_pad; g.d_slab = (int64_t)g.tn * GEMM_BN * d.n_masked_pad;
            g.tm = (d.n_masked + GEMM_BM - 1) / GEMM_BM;
            g.row0 = vmx_plan::tape_row0(d.n_masked, GEMM_BM);
        }
        G.p[G.n++] = g;
    }
    G.work = ql->work.p;
    G.queue = ql->queue.p;
    if (getenv("VMX_QUAD_TRACE")) {          // block timeline of this launch (debugging aid, written by vmx_sync as VMX_GEMM_TRACE is)
        e->gemm_trace_blocks = (size_t)ql->n_blocks;
        if (e->gemm_trace.n < 4 * e->gemm_trace_blocks) (void)e->gemm_trace.alloc(4 * e->gemm_trace_blocks, true);
        else (void)hipMemsetAsync(e->gemm_trace.p, 0, 4 * e->gemm_trace_blocks * sizeof(unsigned long long), e->cur);
        G.trace = e->gemm_trace.p;
    }
    hipLaunchKernelGGL((k_gemm_nt44<KC_QUAD>), dim3(ql->n_blocks, 1), dim3(GEMM44_THREADS), 0, e->cur, G);
}

static vmx_engine::QuadList* quad_work_list(vmx_engine* e, int B)
{
    // a tape depends on the batch size through its number of walker tiles only
    const int tn = (B + GEMM_BN - 1) / GEMM_BN;
    auto found = e->quad_lists.find(tn);
    if (found != e->quad_lists.end()) return found->second;
    vmx_engine::QuadList* ql = quad_build_tape(e, B);
    if (ql) e->quad_lists[tn] = ql;
    return ql;
}

// chi2 of the full chain, r^T C^-1 r = 2 r^T (L r) with the half-form inverse covariance L, is the same contraction as the
// quadratic form's: the tape over the items' covariances (or over the global one), the residuals as walker vectors, no linear
// term.  (Round 5: the 16x16x4 product + slabs + k_chi2 took 98 us at B = 256 where this launch takes ~30.)
static bool cinv_tape_applies(const vmx_engine* e, int B)
{
    if (B <= 8 || e->no_cinv_tape) return false;
    if (e->gcinv.p) return true;
    if (e->items.size() > VMX_MAX_GROUP) return false;
    for (auto* it : e->items) if (!it->has_cinv) return false;
    return true;
}

static vmx_engine::QuadList* cinv_work_list(vmx_engine* e, int B)
{
    const int tn = (B + GEMM_BN - 1) / GEMM_BN;
    auto found = e->cinv_lists.find(tn);
    if (found != e->cinv_lists.end()) return found->second;
    std::vector<vmx_plan::TapeProblem> probs;
    int longest = 0;
    if (e->gcinv.p) { probs.push_back({e->g_n, e->g_ld}); longest = e->g_ld; }
    else for (auto* it : e->items) { probs.push_back({it->dev.n_masked, it->dev.n_masked_pad}); longest = std::max(longest, (int)it->dev.n_masked_pad); }
    if (e->zero_row.n < (size_t)longest && e->zero_row.alloc((size_t)longest, true)) return nullptr;
    vmx_plan::Tape T = vmx_plan::plan_quad_tape(probs, tn, e->quad_blocks, QUAD_ENTRY_STAGES, QUAD_SKEW, GEMM_BM, GEMM_BK, QUAD_K_BANDS);
    auto* ql = new vmx_engine::QuadList();
    ql->n_blocks = T.n_blocks;
    ql->n_entries = (int)T.n_slots;
    if (T.work.empty()) T.work.push_back(GemmWork{-1, 0, 0, 0, 0, 0, 0, 0});
    if (ql->work.upload(T.work.data(), T.work.size()) || ql->queue.upload(T.queue.data(), T.queue.size()) ||
        ql->nt_off.upload(T.nt_off.data(), T.nt_off.size()) ||
        ql->part.alloc(std::max<size_t>((size_t)T.n_slots, 1) * 128, true)) { delete ql; return nullptr; }
    e->cinv_lists[tn] = ql;
    return ql;
}

static void cinv_launch_list(vmx_engine* e, vmx_engine::QuadList* ql, int B)
{
    GemmGroup G{};
    auto add = [&](const double* A, const double* X, int n, int ld) {
        GemmArgs g{};
        g.A = A; g.lda = ld; g.X = X; g.ldx = ld; g.D = nullptr; g.ldd = ld;
        g.M = n; g.N = B; g.K = ld; g.tri = 1; g.nsplit = 1; g.klen = ld;
        g.d_slab = (int64_t)B * ld;
        g.tm = (n + GEMM_BM - 1) / GEMM_BM; g.tn = (B + GEMM_BN - 1) / GEMM_BN;
        g.part = ql->part.p; g.lin = e->zero_row.p; g.lin_row = nullptr; g.lin_pool = 0;
        g.row0 = vmx_plan::tape_row0(n, GEMM_BM);
        G.p[G.n++] = g;
    };
    if (e->gcinv.p) add(e->gcinv.p, e->gres.p, e->g_n, e->g_ld);
    else for (auto* it : e->items) add(it->cinv.p, it->res.p, it->dev.n_masked, it->dev.n_masked_pad);
    G.work = ql->work.p;
    G.queue = ql->queue.p;
    hipLaunchKernelGGL((k_gemm_nt44<KC_QUAD>), dim3(ql->n_blocks, 1), dim3(GEMM44_THREADS), 0, e->cur, G);
}

// static spline-coefficient basis of the polynomial pipelines: C[ell][basis][i] = OP_ell . V_i[ell] (k_poly_basis), with the
// product kernels of the chain; redone when the linear spectra change (vmx_set_linear_spectra)
static int poly_basis_build(vmx_engine* e)
{
    e->poly_dirty = false;
    const int ns = (int)e->pk_static.size();
    e->xi_static_taps.clear(); e->xi_static_bins.clear();
    e->sums_dirty = true;
    if (ns == 0) return 0;
    DevBuf<double> V;
    const int64_t rows = (int64_t)ns * 3;
    if (V.alloc((size_t)VMX_MAX_ELL * rows * e->nkp, true)) return -2;
    e->cur = e->stream;
    hipLaunchKernelGGL(k_poly_basis, dim3((e->nkp + 255) / 256, ns), dim3(256), 0, e->stream, e->dev, e->d_pk_static.p, V.p);
    launch_product(e, KC_OTHER, e->op.p, e->nkp, (int64_t)e->ncp * e->nkp, e->n_coef, e->nkp,
                   V.p, e->nkp, rows * e->nkp, (int)rows, e->poly_coef.p, e->ncp, rows * e->ncp, VMX_MAX_ELL, (int)rows);
    HIP_OK(hipGetLastError());
    if (e->poly_bins_total > 0) {
        std::vector<int32_t> ok(ns, 1);
        DevBuf<int32_t> d_ok;
        if (d_ok.upload(ok.data(), ok.size())) return -2;
        int max_n = 0;
        for (int p : e->pk_static) max_n = std::max(max_n, (int)e->pipes[p].n);
        hipLaunchKernelGGL(k_poly_bins, dim3((max_n + 255) / 256, ns, 3), dim3(256), 0, e->stream, e->dev, e->d_pk_static.p,
                           e->poly_bins.p, d_ok.p);
        e->route_setup |= VMX_ROUTE_POLY_BINS;
        HIP_OK(hipGetLastError());
        HIP_OK(hipStreamSynchronize(e->stream));
        HIP_OK(hipMemcpy(ok.data(), d_ok.p, ok.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
        bool changed = false;
        for (int sb = 0; sb < ns; ++sb)
            if (!ok[sb] && e->pipes[e->pk_static[sb]].poly_bins_off >= 0) { e->pipes[e->pk_static[sb]].poly_bins_off = -1; changed = true; }
        if (changed) HIP_OK(hipMemcpy(e->d_pipes.p, e->pipes.data(), e->pipes.size() * sizeof(PipeDev), hipMemcpyHostToDevice));
    }
    HIP_OK(hipStreamSynchronize(e->stream));
    for (int p : e->pk_static) (e->pipes[p].poly_bins_off >= 0 ? e->xi_static_bins : e->xi_static_taps).push_back(p);
    std::vector<int32_t> a = e->xi_static_taps, b = e->xi_static_bins;
    a.push_back(-1); b.push_back(-1);
    if (e->d_xi_static_taps.upload(a.data(), a.size()) || e->d_xi_static_bins.upload(b.data(), b.size())) return -2;
    return 0;
}

// enqueue the whole kernel chain for the B parameter points already in e->theta
// Kronecker-form metal matrices of an item: one launch, one block per (walker, metal) (k_metal_kron)
static void launch_metal_kron(vmx_engine* e, const EngineDev& D, ItemHost* it, int B)
{
    int item = 0;
    for (size_t q = 0; q < e->items.size(); ++q) if (e->items[q] == it) item = (int)q;
    size_t shmem = 0;
    for (auto* m : it->metals) {
        if (!m->dev.kron_a) continue;
        const int n = m->dev.kron_nrp * m->dev.kron_nrt;
        shmem = std::max(shmem, (size_t)(2 * n + std::max(m->dev.kron_nrp * m->dev.kron_nrp, m->dev.kron_nrt * m->dev.kron_nrt)) * sizeof(double));
    }
    if (shmem == 0) return;
    ScopedTimer t(e, KC_METAL);
    if (!e->kron_attr) { (void)hipFuncSetAttribute((const void*)k_metal_kron, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024); e->kron_attr = true; }
    hipLaunchKernelGGL(k_metal_kron, dim3(B, (unsigned)it->metals.size()), dim3(256), shmem, e->cur, D, item, B);
}

// k_xi_quad_plain serves items that are plain peak / smooth pairs without additive template or pre-distortion broadband
static bool xi_plain_args(vmx_engine* e, XiPlainArgs& A)
{
    if (e->items.size() > VMX_MAX_GROUP || e->extrapolate || e->direct) return false;
    for (size_t q = 0; q < e->items.size(); ++q) {
        const ItemHost* it = e->items[q];
        const ItemDev& d = it->dev;
        if (!it->lean_pair || d.add_vec || d.n_bb[VMX_BB_PRE_MUL] || d.n_bb[VMX_BB_PRE_ADD]) return false;
        const PipeDev& Ps = e->pipes[d.d.pipe_smooth];
        const PipeDev& Pp = e->pipes[d.d.pipe_peak];
        if (Ps.d.n_ell != Pp.d.n_ell || Ps.d.single_ell >= 0 || Pp.d.single_ell >= 0 || Ps.col < 0 || Pp.col < 0) return false;
        XiPlainItem& I = A.it[q];
        I.coord_off = Pp.coord_off; I.q_x0 = it->q_x0.p; I.q_x = it->q_x.p;
        I.n_model = d.d.n_model; I.nq = d.nq; I.nq_pad = d.nq_pad; I.pipe_s = d.d.pipe_smooth; I.pipe_p = d.d.pipe_peak;
        I.col_s = Ps.col; I.col_p = Pp.col; I.n_ell = Ps.d.n_ell; I.split_evol = Pp.split_evol; I.bao_slot = d.d.bao_amp_slot;
        I.item = (int32_t)q;
        I.radiation = Ps.d.radiation;
    }
    return true;
}

// Which bins arrive pre-summed (ItemSums): per item, the lean per-walker pipelines in groups of four and the static-coordinate
// pipelines in groups of sixteen, each member with the factor it enters the item's vector with.  A pipeline with a second
// reader of its own array - another metal pair (fast_metals sharing), a metal matrix product - keeps that array (lean_single:
// k_xi_bins_lean serves it as without sums; static_single for the static-coordinate ones).  A pure function of the engine's configuration; rebuilt when the static basis is.
static int xi_sum_plan(vmx_engine* e)
{
    e->sums_dirty = false;
    e->lean_groups.clear(); e->static_groups.clear(); e->static_single.clear(); e->lean_single.clear();
    e->sums_any = false;
    const int np = (int)e->pipes.size();
    struct Role { int item = -1, fkind = 0, findex = 0, metal = -1, refs = 0; bool plain = true; };
    std::vector<Role> role(np);
    int metal_base = 0;
    for (int q = 0; q < (int)e->items.size(); ++q) {
        const ItemHost* it = e->items[q];
        const vmx_item_desc& d = it->dev.d;
        auto take = [&](int p, int fkind, int findex, int metal, bool plain) {
            if (p < 0 || p >= np) return;
            Role& r = role[p];
            r.refs += 1; r.item = q; r.fkind = fkind; r.findex = findex; r.metal = metal; r.plain = r.plain && plain;
        };
        take(d.pipe_smooth, 0, 0, -1, true);
        if (d.pipe_peak != d.pipe_smooth) take(d.pipe_peak, 1, d.bao_amp_slot, -1, true);
        else role[d.pipe_smooth].plain = false;
        for (int m = 0; m < (int)it->metals.size(); ++m) {
            const MetalDev& md = it->metals[m]->dev;
            if (md.d.pipeline >= 0) take(md.d.pipeline, 2, metal_base + m, m, !md.basis && !md.svec && md.mat_off < 0 && m < 64);
        }
        metal_base += (int)it->metals.size();
    }
    std::vector<ItemSums> sums(e->items.size());
    for (size_t q = 0; q < sums.size(); ++q) { sums[q] = ItemSums{}; sums[q].n_pad = e->items[q]->dev.n_model_pad; }
    auto member_of = [&](int p) {
        const PipeDev& P = e->pipes[p];
        XiMember M{};
        M.coord_off = P.coord_off; M.poly_off = P.poly_bins_off; M.pipe = p; M.col = P.col; M.n_ell = P.d.n_ell;
        M.split_evol = P.split_evol; M.radiation = P.d.is_peak ? 0 : P.d.radiation; M.same_tracer = P.d.same_tracer;
        M.fkind = role[p].fkind; M.findex = role[p].findex;
        return M;
    };
    auto groupable = [&](int p) {
        const Role& r = role[p];
        return e->xi_sums && r.refs == 1 && r.plain && r.item >= 0 && e->pipes[p].n_pad == e->items[r.item]->dev.n_model_pad &&
               sums[r.item].n_arrays < 8;
    };
    auto mark = [&](int p) {
        const Role& r = role[p];
        ItemSums& sm = sums[r.item];
        if (r.fkind == 0) sm.core_smooth = 1;
        else if (r.fkind == 1) sm.core_peak = 1;
        else sm.metal_mask |= 1ull << r.metal;
    };
    // the lean per-walker pipelines
    for (int q = 0; q < (int)e->items.size(); ++q) {
        XiLeanGroup G{};
        auto flush = [&]() {
            if (G.n_members == 0) return;
            if (G.n_members == 1) e->lean_single.push_back(G.m[0].pipe);       // (a sum of one: the plain array, read with its factor as before)
            else {
                sums[q].off[sums[q].n_arrays++] = G.out_off;
                for (int m = 0; m < G.n_members; ++m) mark(G.m[m].pipe);
                e->sums_any = true;
                e->lean_groups.push_back(G);
            }
            G = XiLeanGroup{};
        };
        for (int p : e->xi_lean_pipes) {
            if (role[p].item != q || !groupable(p)) continue;
            const PipeDev& P = e->pipes[p];
            if (G.n_members == 0) { G.out_off = P.xi_off; G.n = P.n; G.n_pad = P.n_pad; G.presum = 1; }
            G.m[G.n_members++] = member_of(p);
            if (G.n_members == VMX_XI_GROUP_MEMBERS || sums[q].n_arrays >= 7) flush();
        }
        flush();
    }
    for (int p : e->xi_lean_pipes) {
        bool placed = false;
        for (auto& G : e->lean_groups) for (int m = 0; m < G.n_members; ++m) placed = placed || G.m[m].pipe == p;
        for (int s1 : e->lean_single) placed = placed || s1 == p;
        // a pipeline whose array has another reader (a metal matrix product, a sharing pair) is evaluated by the kernel that serves
        // it when nothing is summed: its bins - and what a matrix makes of their last bits - do not depend on what the other
        // pipelines of the engine do (k_xi_bins_group and k_xi_bins_lean are compiled apart and round apart)
        if (!placed) e->lean_single.push_back(p);
    }
    // the static-coordinate pipelines (standard evolution, nothing added: what k_xi_bins_static_nw serves)
    auto static_lean = [&](int p) {
        const PipeDev& P = e->pipes[p];
        const vmx_pipe_desc& d = P.d;
        return d.tracer[0].evol_kind == VMX_EVOL_STD && d.tracer[1].evol_kind == VMX_EVOL_STD && !d.uv_shotnoise && !P.odd_rel && !P.odd_asy &&
               (!d.radiation || d.is_peak);
    };
    for (int q = 0; q < (int)e->items.size(); ++q) {
        XiStaticGroup G{};
        auto flush = [&]() {
            if (G.n_members == 0) return;
            if (G.n_members == 1) { e->static_single.push_back(G.m[0].pipe); G = XiStaticGroup{}; return; }
            sums[q].off[sums[q].n_arrays++] = G.out_off;
            for (int m = 0; m < G.n_members; ++m) mark(G.m[m].pipe);
            e->sums_any = true;
            e->static_groups.push_back(G);
            G = XiStaticGroup{};
        };
        for (int p : e->xi_static_bins) {
            if (role[p].item != q || !groupable(p) || !static_lean(p)) continue;
            const PipeDev& P = e->pipes[p];
            if (G.n_members == 0) { G.out_off = P.xi_off; G.n = P.n; G.n_pad = P.n_pad; G.presum = 1; }
            G.m[G.n_members++] = member_of(p);
            if (G.n_members == VMX_XI_SGROUP_MEMBERS) flush();
        }
        flush();
    }
    for (int p : e->xi_static_bins) {
        bool placed = false;
        for (auto& G : e->static_groups) for (int m = 0; m < G.n_members; ++m) placed = placed || G.m[m].pipe == p;
        for (int s1 : e->static_single) placed = placed || s1 == p;
        if (!placed) e->static_single.push_back(p);
    }
    HIP_OK(hipSetDevice(e->device));
    if (!e->lean_groups.empty() && e->d_lean_groups.upload(e->lean_groups.data(), e->lean_groups.size())) return -2;
    if (!e->static_groups.empty() && e->d_static_groups.upload(e->static_groups.data(), e->static_groups.size())) return -2;
    if (e->d_item_sums.upload(sums.data(), sums.size())) return -2;
    std::vector<int32_t> single = e->static_single;
    single.push_back(-1);
    if (e->d_static_single.upload(single.data(), single.size())) return -2;
    return 0;
}

static int marg_products(vmx_engine* e, const EngineDev& D, int B, bool folded);

static int run_chain(vmx_engine* e, int B, int tab_mode, bool zero_copy = false, const double* d_theta = nullptr,
                     double* d_chi2 = nullptr, int32_t* d_status = nullptr, bool quad = false,
                     const double* theta_by_value = nullptr)
{
    EngineDev D = e->dev;
    if (e->call_mock) D.mock_index = e->call_mock;      // (this call's walkers bring their own mock rows)
    // tab_mode: table level of the P(k,mu) stage (EngineDev::xtab_level)
    D.xtab_level = tab_mode;
    e->last_tab_level = tab_mode;
    D.n_const_slots = tab_mode >= 2 ? (int)e->const_slots2.size() : tab_mode ? (int)e->const_slots.size() : 0;
    if (tab_mode >= 2) D.const_slots = e->d_const_slots2.p;
    if (zero_copy) {
        D.theta_host = e->dpin_theta; D.theta_copy = e->theta.p; D.src_host = 1;
        D.chi2_host = e->dpin_chi2; D.status_host = e->dpin_status;
    } else if (d_theta) {
        // device entry point, eager launches: the first kernel reads the caller's walkers in place and the last one
        // writes the caller's outputs - no staging copies
        D.theta_host = d_theta; D.theta_copy = e->theta.p; D.src_host = 0;
        D.chi2_host = d_chi2; D.status_host = d_status;
    }
    if (theta_by_value && zero_copy && B == 1 && e->dpin_done && !e->profiling) { D.done_host = e->dpin_done; D.done_seq = ++e->done_seq; }
    const int n_pipe = D.n_pipe;
    const bool skip_xtab = e->skip_xtab_once;
    e->skip_xtab_once = false;
    bool xtab_launched = !(tab_mode && !skip_xtab);
    D.xtab_block0 = 0;
    {
        ScopedTimer t(e, KC_PROLOGUE);
        // grid = (2 n_pipe + 1 slots: the P(k,mu) half and the xi half of every pipeline's scalars, the walker-level values) x (chunks of PRO_T walkers) [+ the blocks that check the P(k,mu) tables against walker 0:
        // k_xtab's grid, flattened]; LDS of a block: the constant-slot list with walker 0's values,
        // the mu rule's box, its walkers
        const int n_pro = (2 * n_pipe + 1) * ((B + PRO_T - 1) / PRO_T);
        const size_t lds = ((size_t)2 * D.n_const_slots + (size_t)3 * e->rule_slot.size() + (size_t)PRO_T * (e->n_params | 1)) * sizeof(double);
        int n_tab = 0;
        // (walkers in mapped host memory: a thousand table blocks would each cross PCIe for walker 0 - k_xtab follows instead)
        if (!xtab_launched && !(zero_copy && !theta_by_value)) {
            const int rows = XTAB_ROWS * (256 / PRO_T);
            n_tab = ((e->nkp + PRO_T - 1) / PRO_T) * ((e->n_rows + rows - 1) / rows) * e->n_xtab;
            D.xtab_block0 = n_pro;
            xtab_launched = true;
        }
#ifdef VMX_EXP_PRO_TRACE
        if (getenv("VMX_PK_TRACE")) {
            if (!e->pk_trace.p && e->pk_trace.alloc(65536, true)) return -2;
            e->pk_trace_blocks = 2 * (size_t)n_pro;
            D.pk_trace = e->pk_trace.p;
        }
#endif
        if (lds > 160 * 1024 - 256) return fail(-1, "too many parameters for k_prologue's walker rows in LDS (64 x n_params doubles)");
        if (lds > 64 * 1024) {
            // beyond ~125 parameters the rows need more than the default 64 KB of dynamic LDS: the function attribute is the
            // driver's, per device and monotone - the largest request so far is remembered per device
            static std::mutex mu;
            static size_t allowed[64] = {};
            std::lock_guard<std::mutex> lock(mu);
            size_t& a = allowed[e->device & 63];
            if (lds > a) {
                HIP_OK(hipFuncSetAttribute((const void*)k_prologue, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
                HIP_OK(hipFuncSetAttribute((const void*)k_prologue_byval, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
                a = lds;
            }
        }
#ifdef VMX_EXP_SKIP_SMALL
        // experiment build (timing only, results are wrong): what the step costs without this launch - the bound of what folding
        // it into its neighbour can give
        static const int exp_skip = getenv("VMX_EXP_SKIP") ? atoi(getenv("VMX_EXP_SKIP")) : 0;
        static int exp_calls = 0;
        if ((exp_skip & 2) && ++exp_calls > 64) goto exp_no_prologue;
#endif
        if (zero_copy && theta_by_value) {
            // (eager launches only: a captured graph would replay the walker it was captured with)
            ThetaArg ta;
            std::memcpy(ta.v, theta_by_value, (size_t)B * e->n_params * sizeof(double));
            hipLaunchKernelGGL(k_prologue_byval, dim3(n_pro + n_tab), dim3(PRO_T), lds, e->stream, ta, D, B);
        } else
            hipLaunchKernelGGL(k_prologue, dim3(n_pro + n_tab), dim3(PRO_T), lds, e->stream, D, B);
#ifdef VMX_EXP_SKIP_SMALL
        exp_no_prologue:;
#endif
    }
    {
        ScopedTimer t(e, KC_PK);
        // reduction scratch + (unless every looping group runs against its D_NL table) the mu^bv tables
        bool need_mubv = false;
        for (auto& g : e->pk_groups)
            if (e->pipes[g.pipe].d.nl_model == VMX_NL_ARINYO && !(tab_mode && g.xtab >= 0)) need_mubv = true;
        size_t shmem = ((need_mubv ? (size_t)e->n_rows : 0) + 2048) * sizeof(double);
        // + the (mu^2, mu^4) table of the tabulated and shared-W mu loops (the large-batch shapes; 40 KB per block at most,
        // four blocks per CU)
        bool want_mu_tab = false;
        for (auto& g : e->pk_groups)
            if ((tab_mode && g.xtab >= 0) || g.variant == PKV_SHARED_W) want_mu_tab = true;
        int mu_tab_off = want_mu_tab ? (int)(shmem / sizeof(double)) : -1;
        if (want_mu_tab) shmem += (size_t)2 * e->n_mu * sizeof(double);
        const int n_groups = (int)e->pk_groups.size();
        if (!xtab_launched)
            hipLaunchKernelGGL(k_xtab, dim3((e->nkp + 255) / 256, (e->n_rows + XTAB_ROWS - 1) / XTAB_ROWS, e->n_xtab), dim3(256), 0, e->stream, D);
        if (!e->pk_poly.empty())
            hipLaunchKernelGGL(k_pk_poly, dim3(B, (int)e->pk_poly.size()), dim3(256), 0, e->stream, D, e->d_pk_poly.p, B);
        int tm = tab_mode;
        // level-2 groups run in their own kernel; the general one follows for whatever else the configuration has
        int n_other = n_groups;
        if (tab_mode >= 2 && e->n_xtab > 0) {
            n_other = n_groups - e->n_xtab;
            // (the node tables' image, + [2 terms][2 walkers][64 wavenumbers] of UV / HeII bias terms behind it)
            const size_t sh1 = std::max<size_t>(2048, (size_t)2 * e->n_mu + 4 * e->n_extra + 256 + 16) * sizeof(double);     // (+ the waves' votes)
            if (sh1 > 64 * 1024) {
                // (num_bins_muk near its limit of 4096: the node tables alone are 64 KB - the driver's per-device attribute, monotone)
                static std::mutex mu;
                static size_t allowed[64] = {};
                std::lock_guard<std::mutex> lock(mu);
                size_t& a = allowed[e->device & 63];
                if (sh1 > a) {
                    HIP_OK(hipFuncSetAttribute((const void*)k_pk_tab2<64, 4, 2>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sh1));
                    HIP_OK(hipFuncSetAttribute((const void*)k_pk_tab2<64, 4, 1>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sh1));
                    HIP_OK(hipFuncSetAttribute((const void*)k_pk_tab2<16, 16, 1>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sh1));
                    a = sh1;
                }
            }
#ifdef VMX_EXP_PRO_TRACE       // (experiment build: the trace buffer holds k_prologue's stamps, scripts/gpu_pro_trace.py)
            D.pk_trace = nullptr;
            if (false) {
#else
            if (getenv("VMX_PK_TRACE")) {
#endif
                e->pk_trace_blocks = (size_t)B * ((e->nk + 7) / 8) * e->tab2_groups.size();     // (an upper bound: unused entries stay zero)
                if (!e->pk_trace.p && e->pk_trace.alloc(4 * (size_t)e->max_batch * ((e->nk + 7) / 8) * e->tab2_groups.size(), true)) return -2;
                D.pk_trace = e->pk_trace.p;
            }
            for (size_t first = 0; first < e->tab2_groups.size(); first += VMX_TAB2_GROUPS) {
                Tab2Args A{};
                const int n = (int)std::min<size_t>(VMX_TAB2_GROUPS, e->tab2_groups.size() - first);
                for (int q = 0; q < n; ++q) A.g[q] = e->tab2_groups[first + q];
                const bool wide = (int64_t)B * e->n_xtab >= 24;
                const std::vector<uint16_t>& zmap = wide ? e->zmap64 : e->zmap16;
                A.n_z = (int32_t)zmap.size();           // (0: plain order, main rule)
                std::copy(zmap.begin(), zmap.end(), A.zmap);
                e->last_tab2_kt = wide ? 64 : 16;
                if (wide) {
                    if (B >= 64)
                        hipLaunchKernelGGL((k_pk_tab2<64, 4, 2>), dim3((B + 1) / 2, n, (e->nk + 63) / 64), dim3(256), std::max(sh1, (size_t)4096 * sizeof(double)), e->stream, D, A, B);
                    else
                        hipLaunchKernelGGL((k_pk_tab2<64, 4, 1>), dim3(B, n, (e->nk + 63) / 64), dim3(256), sh1, e->stream, D, A, B);
                } else      // (8 x 32 blocks for a single walker measured the same: 12 us)
                    hipLaunchKernelGGL((k_pk_tab2<16, 16, 1>), dim3(B, n, (e->nk + 15) / 16), dim3(256), sh1, e->stream, D, A, B);
            }
        }
        // the shared-W groups in their own kernel (large batches)
        const int n_w = ((int64_t)B * (int)e->w_groups.size() >= 24 && !e->no_pk_w) ? (int)e->w_groups.size() : 0;
        if (n_w > 0) {
            n_other -= n_w;
            tm |= 32;
            const size_t shw = std::max<size_t>((size_t)2 * 6 * 256, (size_t)2 * e->n_mu + 4 * e->n_extra + 16) * sizeof(double);    // (+ the waves' votes)
            if (B >= 64)        // (four walkers per thread: 161 registers, 465 against 426 us for the stage at B = 512)
                hipLaunchKernelGGL((k_pk_w<2>), dim3((B + 1) / 2, n_w, (e->nk + 63) / 64), dim3(256), shw, e->stream, D, e->d_pk_groups.p, e->d_pk_members.p, e->d_w_groups.p, B);
            else
                hipLaunchKernelGGL((k_pk_w<1>), dim3(B, n_w, (e->nk + 63) / 64), dim3(256), shw, e->stream, D, e->d_pk_groups.p, e->d_pk_members.p, e->d_w_groups.p, B);
        }
        if (n_other == 0) {}
        else {
            // the instantiation without the run-time-switched loops needs fewer registers (4 instead of 3 waves per
            // SIMD): use it whenever every group has a specialised loop
            bool generic = false;
            for (auto& g : e->pk_groups) if (g.variant == PKV_GENERIC) generic = true;
            const PkGroup* gp = e->d_pk_groups.p;
            const int32_t* mp = e->d_pk_members.p;
#define VMX_LAUNCH_PK(KT, MS)                                                                                        \
            do {                                                                                                     \
                const dim3 grid(B, n_groups, (e->nk + (KT) - 1) / (KT));                                             \
                if (generic) hipLaunchKernelGGL((k_pk_multipoles<KT, MS, 1, true>), grid, dim3(256), shmem, e->stream, D, gp, mp, tm, B, mu_tab_off);   \
                else hipLaunchKernelGGL((k_pk_multipoles<KT, MS, 1, false>), grid, dim3(256), shmem, e->stream, D, gp, mp, tm, B, mu_tab_off);         \
            } while (0)
            if ((int64_t)B * n_groups >= 24) VMX_LAUNCH_PK(64, 4);
            else if ((int64_t)B * n_groups >= 4) VMX_LAUNCH_PK(16, 16);
            else {
                // + the block's slice of the G table, staged in LDS ([n_mu][8])
                shmem = ((size_t)e->n_rows + 2048 + (size_t)8 * e->n_rows) * sizeof(double);
                mu_tab_off = -1;
                if (!e->pk_small_attr) {
                    HIP_OK(hipFuncSetAttribute((const void*)k_pk_multipoles<8, 32, 1, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shmem));
                    HIP_OK(hipFuncSetAttribute((const void*)k_pk_multipoles<8, 32, 1, false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shmem));
                    e->pk_small_attr = true;
                }
                VMX_LAUNCH_PK(8, 32);
            }
#undef VMX_LAUNCH_PK
        }
    }
    {
        const int64_t ncols = (int64_t)B * e->n_active;
        const bool pads = e->pad_l + e->pad_r > 0;
        e->last_fft_form = 0;
        if (ncols > 0 && pads) {
            // fht_extrap: the power-law pads of every (multipole, pipeline, walker) row, behind its samples
            ScopedTimer t(e, KC_FFTLOG);
            hipLaunchKernelGGL(k_pk_extrap, dim3((unsigned)(VMX_MAX_ELL * ncols)), dim3(256), 0, e->stream, D, B);
        }
        if (ncols > 0)      // (with pads the product runs over the whole row: the live-wavenumber limit is about the samples)
            launch_product(e, KC_FFTLOG, e->op.p, e->nkp, (int64_t)e->ncp * e->nkp, e->n_coef, e->nkp,
                           e->pl.p, e->nkp, ncols * e->nkp, (int)ncols, e->coef.p, e->ncp, ncols * e->ncp,
                           VMX_MAX_ELL, 0, pads ? nullptr : e->k_live.p, -1, false, e->coef_win.p);
    }
    // chi2-only small batches of items without metal terms: bins + quadratic-form entries in one kernel
    bool xi_fused = quad && (size_t)n_pipe == 2 * e->items.size();
    for (auto* it : e->items) if (!it->metals.empty() || it->dev.d.pipe_peak == it->dev.d.pipe_smooth) xi_fused = false;
    e->last_taps = !(xi_fused && B > 8);
    int route = D.same_grid ? VMX_ROUTE_SAME_GRID : 0;
    if (xi_fused) {
        ScopedTimer t(e, KC_XI);
        int max_nq = 0;
        for (auto* it : e->items) max_nq = std::max(max_nq, (int)it->dev.nq_pad);
        XiPlainArgs XA{};
        // (two walkers per thread: 41 us at B = 256 against 53 with one; four measured the same as two)
        if (B > 8 && xi_plain_args(e, XA)) {
            route |= VMX_ROUTE_QUAD_PLAIN;
            hipLaunchKernelGGL((D.same_grid ? k_xi_quad_plain<2, true> : k_xi_quad_plain<2, false>), dim3((max_nq + 255) / 256, (B + 1) / 2, (unsigned)e->items.size()), dim3(256), 0, e->stream, D, XA, 0, B);
        } else {
            route |= VMX_ROUTE_ASSEMBLE_QUAD;
            for (auto* it : e->items) if (!it->dev.plain_pair) route |= VMX_ROUTE_ASSEMBLE_QUAD_GENERAL;
            hipLaunchKernelGGL(k_xi_assemble_quad, dim3((max_nq + 255) / 256, B, (unsigned)e->items.size()), dim3(256), 0, e->stream, D, 0, B <= 8 ? 1 : 0);
        }
    } else {
        ScopedTimer t(e, KC_XI);
        int max_n = 0;
        for (auto& p : e->pipes) max_n = p.n > max_n ? p.n : max_n;
        // bins that arrive pre-summed (xi_sum_plan): large chi2-only or model batches of engines with lean pipelines
        const bool use_sums = B > 8 && !e->direct && e->xi_lean && e->xi_sums && !e->extrapolate;
        const bool sums_on = use_sums && e->sums_any && !e->sums_dirty;      // (the plan is made with the static basis, outside any capture)
        if (sums_on) { D.sums = e->d_item_sums.p; D.sums_on = 1; e->last_taps = false; }
        if (sums_on && !e->lean_groups.empty()) {
            // (walkers per thread of the lean kernels: 1 / 2 / 4 measured the same - the stage is bound by its dependent lookups)
            const dim3 grid((max_n + 255) / 256, (unsigned)e->lean_groups.size(), (B + 1) / 2);
            route |= VMX_ROUTE_GROUP;
            hipLaunchKernelGGL((D.same_grid ? k_xi_bins_group<2, true> : k_xi_bins_group<2, false>), grid, dim3(256), 0, e->stream, D, e->d_lean_groups.p, B);
            if (!e->lean_single.empty()) {
                XiLeanArgs LA{};
                for (size_t q = 0; q < e->lean_single.size(); ++q) {
                    const PipeDev& P = e->pipes[e->lean_single[q]];
                    XiLeanPipe& L = LA.p[q];
                    L.coord_off = P.coord_off; L.xi_off = P.xi_off; L.n = P.n; L.n_pad = P.n_pad; L.pipe = e->lean_single[q]; L.col = P.col;
                    L.n_ell = P.d.n_ell; L.split_evol = P.split_evol; L.radiation = P.d.is_peak ? 0 : P.d.radiation;
                }
                const dim3 single((max_n + 255) / 256, (unsigned)e->lean_single.size(), (B + 1) / 2);
                route |= VMX_ROUTE_LEAN;
                hipLaunchKernelGGL((D.same_grid ? k_xi_bins_lean<2, true> : k_xi_bins_lean<2, false>), single, dim3(256), 0, e->stream, D, LA, B);
            }
            if (!e->xi_rest_pipes.empty()) {
                route |= VMX_ROUTE_GENERAL;
                hipLaunchKernelGGL(k_xi_bins<false>, dim3((max_n + 255) / 256, (unsigned)e->xi_rest_pipes.size(), B), dim3(256), 0, e->stream, D, e->d_xi_rest_pipes.p);
            }
        } else if (B > 8 && !e->direct && !e->xi_lean_pipes.empty()) {
            XiLeanArgs LA{};
            for (size_t q = 0; q < e->xi_lean_pipes.size(); ++q) {
                const PipeDev& P = e->pipes[e->xi_lean_pipes[q]];
                XiLeanPipe& L = LA.p[q];
                L.coord_off = P.coord_off; L.xi_off = P.xi_off; L.n = P.n; L.n_pad = P.n_pad; L.pipe = e->xi_lean_pipes[q]; L.col = P.col;
                L.n_ell = P.d.n_ell; L.split_evol = P.split_evol; L.radiation = P.d.is_peak ? 0 : P.d.radiation;
            }
            const dim3 grid((max_n + 255) / 256, (unsigned)e->xi_lean_pipes.size(), (B + 1) / 2);
            route |= VMX_ROUTE_LEAN;
            hipLaunchKernelGGL((D.same_grid ? k_xi_bins_lean<2, true> : k_xi_bins_lean<2, false>), grid, dim3(256), 0, e->stream, D, LA, B);
            if (!e->xi_rest_pipes.empty()) {
                route |= VMX_ROUTE_GENERAL;
                hipLaunchKernelGGL(k_xi_bins<false>, dim3((max_n + 255) / 256, (unsigned)e->xi_rest_pipes.size(), B), dim3(256), 0, e->stream, D, e->d_xi_rest_pipes.p);
            }
        } else if (e->n_active > 0) {
            route |= VMX_ROUTE_GENERAL;
            hipLaunchKernelGGL(k_xi_bins<false>, dim3((max_n + 255) / 256, e->n_active, B), dim3(256), 0, e->stream, D, e->d_pipe_active.p);
        }
        if (!e->pk_static.empty())
        {
            // static-basis pipelines: tap form, and the ones already evaluated on their (static) bins
            if (!e->xi_static_taps.empty()) {
                route |= VMX_ROUTE_STATIC_TAPS;
                hipLaunchKernelGGL(k_xi_bins<true>, dim3((max_n + 255) / 256, (unsigned)e->xi_static_taps.size(), B), dim3(256), 0, e->stream, D, e->d_xi_static_taps.p);
            }
            if (sums_on && !e->xi_static_bins.empty()) {
                if (!e->static_groups.empty()) {
                    const dim3 grid((max_n + 255) / 256, (unsigned)e->static_groups.size(), (B + 1) / 2);
                    route |= VMX_ROUTE_STATIC_GROUP;
                    hipLaunchKernelGGL(k_xi_bins_static_group<2>, grid, dim3(256), 0, e->stream, D, e->d_static_groups.p, B);
                }
                if (!e->static_single.empty()) {
                    route |= VMX_ROUTE_STATIC;
                    hipLaunchKernelGGL(k_xi_bins_static, dim3((max_n + 255) / 256, (unsigned)e->static_single.size(), B), dim3(256), 0, e->stream, D, e->d_static_single.p);
                }
            } else if (!e->xi_static_bins.empty()) {
                bool lean = e->xi_lean && B > 8 && (int)e->xi_static_bins.size() <= VMX_XI_LEAN_MAX;
                for (int p : e->xi_static_bins) {
                    const PipeDev& P = e->pipes[p];
                    const vmx_pipe_desc& d = P.d;
                    lean = lean && d.tracer[0].evol_kind == VMX_EVOL_STD && d.tracer[1].evol_kind == VMX_EVOL_STD && !d.uv_shotnoise &&
                           !P.odd_rel && !P.odd_asy && (!d.radiation || d.is_peak);
                }
                if (lean) {
                    XiLeanArgs LA{};
                    for (size_t q = 0; q < e->xi_static_bins.size(); ++q) {
                        const PipeDev& P = e->pipes[e->xi_static_bins[q]];
                        XiLeanPipe& L = LA.p[q];
                        L.coord_off = P.coord_off; L.xi_off = P.xi_off; L.poly_off = P.poly_bins_off; L.n = P.n; L.n_pad = P.n_pad;
                        L.pipe = e->xi_static_bins[q]; L.split_evol = P.split_evol; L.same_tracer = P.d.same_tracer;
                    }
                    // (four walkers per thread load the three basis values and the two per-bin factors once: 96 -> 51 us at B = 512)
                    const dim3 grid((max_n + 255) / 256, (unsigned)e->xi_static_bins.size(), (B + 3) / 4);
                    route |= VMX_ROUTE_STATIC_NW;
                    hipLaunchKernelGGL(k_xi_bins_static_nw<4>, grid, dim3(256), 0, e->stream, D, LA, B);
                } else {
                    route |= VMX_ROUTE_STATIC;
                    hipLaunchKernelGGL(k_xi_bins_static, dim3((max_n + 255) / 256, (unsigned)e->xi_static_bins.size(), B), dim3(256), 0, e->stream, D, e->d_xi_static_bins.p);
                }
            }
        }
    }
    e->last_route = route;
    // dense metal-matrix products of an item (no split-K: the consumer reads one slab)
    auto metal_products = [&](ItemHost* it) {
        launch_metal_kron(e, D, it, B);
        for (auto* m : it->metals) {
            if (m->dev.mat_off < 0 || m->dev.kron_a) continue;
            const PipeDev& P = e->pipes[m->dev.d.pipeline];
            launch_product(e, KC_METAL, m->mat.p, m->dev.mat_ld, 0, m->rows, m->dev.mat_ld,
                           e->xi.p + P.xi_off, P.n_pad, 0, B, e->xim.p + m->dev.xim_off, it->dev.n_model_pad, 0, 1, 0);
        }
    };
    if (quad) {
        // chi2 only: x' - x0' per item, ONE half-triangle product with the static Q' per item, reduction (vmx_device.h)
        e->cur = e->stream;
        int max_nq = 0;
        for (auto* it : e->items) { max_nq = std::max(max_nq, (int)it->dev.nq_pad); metal_products(it); }
        if (!xi_fused) {
            ScopedTimer t(e, KC_ASSEMBLE);
            hipLaunchKernelGGL(k_assemble_quad, dim3((max_nq + 255) / 256, B, (unsigned)e->items.size()), dim3(256), 0, e->cur, D);
        }
        if (e->marg_req) {
            // derived columns only (vmx_marg_coeff_device): G dx per item with templates instead of the form's own product
            e->last_form = e->quad_factored ? 2 : 1;
            if (marg_products(e, D, B, true)) return -2;
            e->last_B = B;
            e->last_full = false;
            return 0;
        }
        SlabInfo qs{};
        for (size_t q = 0; q < e->items.size(); ++q) qs.z[q] = 1;
        if (e->quad_factored) {
            // chi2 = sum over items of || u0 - F dx ||^2: one rectangular product per item (all of them in one launch for B > 8,
            // split-K slabs summed in fixed order by the reduction), then the sum of squares
            if (B > 8 && e->items.size() <= VMX_MAX_GROUP) {
                GemmGroup G{};
                int tiles_total = 0, per_xcd_total = 0;
                for (auto* it : e->items) tiles_total += gemm_tiles(it->dev.n_masked, B, false);
                std::vector<size_t> by_size(e->items.size());
                for (size_t q = 0; q < by_size.size(); ++q) by_size[q] = q;
                std::stable_sort(by_size.begin(), by_size.end(), [&](size_t a, size_t b) {
                    const ItemDev& da = e->items[a]->dev; const ItemDev& db = e->items[b]->dev;
                    return (int64_t)da.n_masked * da.nq > (int64_t)db.n_masked * db.nq; });
                std::vector<int>& splits = e->group_splits[3 * 100000 + B];
                if (splits.empty()) {
                    std::vector<SplitProblem> sp;
                    for (size_t q : by_size) {
                        const ItemDev& d = e->items[q]->dev;
                        int max_split = 1;
                        while (max_split < 8 && (int64_t)max_split * 2 * B <= e->fact_slab_rows) max_split *= 2;
                        sp.push_back({gemm_tiles(d.n_masked, B, false), (d.nq_pad + GEMM_BK - 1) / GEMM_BK, (int64_t)B * d.n_masked_pad * 8, max_split,
                                      (d.n_masked + GEMM_BM - 1) / GEMM_BM, (B + GEMM_BN - 1) / GEMM_BN});
                    }
                    splits = choose_group_splits(sp, true);
                    if (splits.empty()) splits.push_back(0);
                }
                size_t gi = 0;
                for (size_t q : by_size) {
                    ItemHost* it = e->items[q];
                    const ItemDev& d = it->dev;
                    GemmArgs g{};
                    g.A = it->q_f.p; g.lda = d.nq_pad; g.X = it->q_x.p; g.ldx = d.nq_pad; g.D = it->q_y.p; g.ldd = d.n_masked_pad;
                    g.M = d.n_masked; g.N = B; g.K = d.nq_pad;
                    int per_xcd = 0;
                    const int forced = gi < splits.size() ? splits[gi] : 0;
                    ++gi;
                    qs.z[q] = plan_gemm(e, g, 1, e->fact_slab_rows, nullptr, false, tiles_total - gemm_tiles(d.n_masked, B, false), &per_xcd, forced);
                    per_xcd_total += per_xcd;
                    G.p[G.n] = g; G.seq_end[G.n] = per_xcd_total; ++G.n;
                }
                ScopedTimer t(e, KC_QUAD);
                launch_gemm_group(e, KC_QUAD, G, per_xcd_total, 1);
            } else {
                for (size_t q = 0; q < e->items.size(); ++q) {
                    ItemHost* it = e->items[q];
                    const ItemDev& d = it->dev;
                    qs.z[q] = launch_product(e, KC_QUAD, it->q_f.p, d.nq_pad, 0, d.n_masked, d.nq_pad, it->q_x.p, d.nq_pad, 0, B,
                                             it->q_y.p, d.n_masked_pad, 0, 1, e->fact_slab_rows);
                }
            }
            {
                ScopedTimer t(e, KC_CHI2);
                hipLaunchKernelGGL(k_chi2_quad<true>, dim3(B), dim3(CHI2_THREADS), 0, e->stream, D, B, qs);
            }
            HIP_OK(hipGetLastError());
            e->last_B = B;
            e->last_full = false;
            e->last_form = 2;
            return 0;
        }
        e->last_form = 1;
        e->last_root = false;
        if (B > 8 && e->items.size() <= VMX_MAX_GROUP) {
            // the persistent tape: every block the same work to a stage, contraction partials in the tape's slots
            vmx_engine::QuadList* ql = quad_work_list(e, B);
            if (!ql) return -2;
            {
                ScopedTimer t(e, KC_QUAD);
                quad_launch_list(e, ql, B);
            }
            e->last_root = ql->root;
            if (ql->root) {
                // the launch left partial tiles of L dx: the reducer squares and adds them, and the linear term with them
                RootArgs R{};
                for (size_t q = 0; q < e->items.size(); ++q) {
                    const ItemDev& d = e->items[q]->dev;
                    const int tn = (B + GEMM_BN - 1) / GEMM_BN;
                    R.p[q] = {ql->ypart.p + ql->y_off[q], (int64_t)tn * GEMM_BN * d.n_masked_pad, ql->segs.p + ql->seg_off[q],
                              (int32_t)d.n_masked_pad, (int32_t)d.n_masked, vmx_plan::tape_row0(d.n_masked, GEMM_BM), tn};
                }
                ScopedTimer t(e, KC_CHI2);
                hipLaunchKernelGGL(k_chi2_root, dim3(B), dim3(CHI2_ROOT_THREADS), 0, e->stream, D, B, R);
                HIP_OK(hipGetLastError());
                e->last_B = B;
                e->last_full = false;
                return 0;
            }
            // the launch left contraction partials instead of the product: a small kernel adds them up
            ScopedTimer t(e, KC_CHI2);
#ifdef VMX_EXP_SKIP_SMALL
            static const int exp_skip1 = getenv("VMX_EXP_SKIP") ? atoi(getenv("VMX_EXP_SKIP")) : 0;
            static int exp_calls1 = 0;
            if (!((exp_skip1 & 1) && ++exp_calls1 > 64))
#endif
            hipLaunchKernelGGL(k_chi2_parts, dim3((B + 3) / 4), dim3(256), 0, e->stream, D, B, (const double*)ql->part.p,
                               (const int32_t*)ql->nt_off.p, 1);
            HIP_OK(hipGetLastError());
            e->last_B = B;
            e->last_full = false;
            return 0;
        } else if (B == 1 && D.done_host && e->dpin_part && !e->no_host_reduce && e->items.size() <= VMX_MAX_GROUP) {     // (Q' form)
            // single walker through the host entry: every block of the streaming products leaves its share of the contraction
            // in mapped host memory, the host adds them up (vmx_eval) - no chi2 kernel
            bool ok = true;
            for (auto* it : e->items) ok = ok && gemv1_applies(1, it->dev.nq_pad) && gemv1_blocks(it->dev.nq) <= 1024 && it->dev.nq_pad <= 2560 * 2;
            if (ok) {
                e->host_reduce_items = (int)e->items.size();
                for (size_t q = 0; q < e->items.size(); ++q) {
                    ItemHost* it = e->items[q];
                    const ItemDev& d = it->dev;
                    const int mock = (d.mock_pool && e->h_mock_index[0] >= 0) ? e->h_mock_index[0] : -1;
                    GemmArgs g{};
                    g.A = it->q_mat.p; g.lda = d.nq_pad; g.X = it->q_x.p; g.ldx = d.nq_pad; g.D = it->q_z.p; g.ldd = d.nq_pad;
                    g.M = d.nq; g.N = 1; g.K = d.nq_pad; g.tri = 1; g.nsplit = 1; g.klen = d.nq_pad;
                    g.part = e->dpin_part + q * 1024; g.lin = it->q_lin.p + (size_t)(mock >= 0 ? 1 + mock : 0) * d.nq_pad;
                    const int blocks = gemv1_blocks(d.nq);
                    e->host_reduce_blocks[q] = blocks;
                    ScopedTimer t(e, KC_QUAD);
                    const int last = q + 1 == e->items.size() ? 1 : 0;
                    if (d.nq_pad <= 2560) hipLaunchKernelGGL((k_gemv1<5, 2>), dim3(blocks), dim3(256), (size_t)d.nq_pad * sizeof(double), e->stream, g, D, last);
                    else hipLaunchKernelGGL((k_gemv1<10, 2>), dim3(blocks), dim3(256), (size_t)d.nq_pad * sizeof(double), e->stream, g, D, last);
                }
                HIP_OK(hipGetLastError());
                e->last_B = B;
                e->last_full = false;
                return 0;
            }
            for (size_t q = 0; q < e->items.size(); ++q) {
                ItemHost* it = e->items[q];
                const ItemDev& d = it->dev;
                qs.z[q] = launch_product(e, KC_QUAD, it->q_mat.p, d.nq_pad, 0, d.nq, d.nq_pad, it->q_x.p, d.nq_pad, 0, B,
                                         it->q_z.p, d.nq_pad, 0, 1, e->slab_rows, nullptr, -1, true);
            }
        } else {
            for (size_t q = 0; q < e->items.size(); ++q) {
                ItemHost* it = e->items[q];
                const ItemDev& d = it->dev;
                qs.z[q] = launch_product(e, KC_QUAD, it->q_mat.p, d.nq_pad, 0, d.nq, d.nq_pad, it->q_x.p, d.nq_pad, 0, B,
                                         it->q_z.p, d.nq_pad, 0, 1, e->slab_rows, nullptr, -1, true);
            }
        }
        {
            ScopedTimer t(e, KC_CHI2);
            hipLaunchKernelGGL(k_chi2_quad<false>, dim3(B), dim3(CHI2_THREADS), 0, e->stream, D, B, qs);
        }
        HIP_OK(hipGetLastError());
        e->last_B = B;
        e->last_full = false;
        return 0;
    }
    e->last_form = 0;
    SlabInfo slabs{};
    for (size_t q = 0; q < e->items.size(); ++q) slabs.z[q] = 1;
    const bool grouped = B > 8 && e->items.size() <= VMX_MAX_GROUP;
    if (grouped) {
        // Large batches: the items advance together on one stream and their products share launches - every tile of
        // every item's distortion product (then of every C^-1 product) is in flight at once.
        e->cur = e->stream;
        int max_model = 0, max_dist = 0;
        for (auto* it : e->items) {
            max_model = std::max(max_model, (int)it->dev.d.n_model); max_dist = std::max(max_dist, (int)it->dev.d.n_dist);
            metal_products(it);
        }
        {
            ScopedTimer t(e, KC_ASSEMBLE);
            hipLaunchKernelGGL(k_assemble_all, dim3((max_model + 255) / 256, B, (unsigned)e->items.size()), dim3(256), 0, e->cur, D);
        }
        SlabInfo dslabs{};
        for (size_t q = 0; q < e->items.size(); ++q) dslabs.z[q] = 1;
        for (int stage = 0; stage < 2; ++stage) {       // 0: distortion products, 1: C^-1 products
            if (stage == 1 && (e->gcinv.p || cinv_tape_applies(e, B))) break;
            GemmGroup G{};
            int tiles_total = 0, per_xcd_total = 0;
            for (auto* it : e->items) {
                const ItemDev& d = it->dev;
                if (stage == 0 ? it->has_dm : it->has_cinv)
                    tiles_total += stage == 0 ? gemm_tiles(d.d.n_dist, B, false) : gemm_tiles(d.n_masked, B, true);
            }
            // largest problem first: its blocks are the long ones, and the short blocks of the others then fill the tail
            std::vector<size_t> by_size(e->items.size());
            for (size_t q = 0; q < by_size.size(); ++q) by_size[q] = q;
            std::stable_sort(by_size.begin(), by_size.end(), [&](size_t a, size_t b) {
                const ItemDev& da = e->items[a]->dev; const ItemDev& db = e->items[b]->dev;
                return stage == 0 ? (int64_t)da.d.n_dist * da.d.n_model > (int64_t)db.d.n_dist * db.d.n_model : da.n_masked > db.n_masked; });
            // K splits of the group: simulated once per (stage, batch size)
            std::vector<int>& splits = e->group_splits[stage * 100000 + B];
            if (splits.empty() && stage == 0) {        // (the model describes the self-pipelined 4x4x4 kernel)
                std::vector<SplitProblem> sp;
                for (size_t q : by_size) {
                    ItemHost* it = e->items[q];
                    const ItemDev& d = it->dev;
                    if (!(stage == 0 ? it->has_dm : it->has_cinv)) continue;
                    const int M = stage == 0 ? d.d.n_dist : d.n_masked, K = stage == 0 ? d.n_model_pad : d.n_masked_pad;
                    const int ldd = stage == 0 ? d.n_dist_pad : d.n_masked_pad;
                    int max_split = 1;
                    while (max_split < 8 && (int64_t)max_split * 2 * B <= e->slab_rows) max_split *= 2;
                    // (a triangular problem pairs its row tiles: every block covers about one full K range)
                    sp.push_back({gemm_tiles(M, B, stage == 1), (K + GEMM_BK - 1) / GEMM_BK, (int64_t)B * ldd * 8, max_split,
                                  (M + GEMM_BM - 1) / GEMM_BM, (B + GEMM_BN - 1) / GEMM_BN});
                }
                // (the one-block-per-CU model: 288 against 317 us for the distortion launch at B = 256 with the per-XCD model's
                // choice, 101 against 94 at B = 64 - fitted on these shapes in round 2 and kept for them)
                splits = choose_group_splits(sp);
            }
            if (splits.empty()) splits.push_back(0);
            size_t gi = 0;
            for (size_t q : by_size) {
                ItemHost* it = e->items[q];
                const ItemDev& d = it->dev;
                if (!(stage == 0 ? it->has_dm : it->has_cinv)) continue;
                const int forced = gi < splits.size() ? splits[gi] : 0;
                ++gi;
                GemmArgs g{};
                if (stage == 0) {
                    g.A = it->dm.p; g.lda = d.n_model_pad; g.X = it->vec.p; g.ldx = d.n_model_pad; g.D = it->dist.p; g.ldd = d.n_dist_pad;
                    g.M = d.d.n_dist; g.N = B; g.K = d.n_model_pad;
                } else {
                    g.A = it->cinv.p; g.lda = d.n_masked_pad; g.X = it->res.p; g.ldx = d.n_masked_pad; g.D = it->z.p; g.ldd = d.n_masked_pad;
                    g.M = d.n_masked; g.N = B; g.K = d.n_masked_pad;
                }
                int per_xcd = 0;
                const int own = stage == 0 ? gemm_tiles(g.M, B, false) : gemm_tiles(g.M, B, true);
                const int ns = plan_gemm(e, g, 1, e->slab_rows, nullptr, stage == 1, tiles_total - own, &per_xcd, forced);
                (stage == 0 ? dslabs : slabs).z[q] = ns;
                per_xcd_total += per_xcd;
                G.p[G.n] = g; G.seq_end[G.n] = per_xcd_total; ++G.n;
            }
            if (G.n > 0) {
                ScopedTimer t(e, stage == 0 ? KC_DISTORTION : KC_INVCOV);
                launch_gemm_group(e, stage == 0 ? KC_DISTORTION : KC_INVCOV, G, per_xcd_total, 1);
            }
            if (stage == 0)
                for (auto* it : e->items) if (it->has_csr) launch_csr(e, it, B);       // CSR matrices: 8 walkers per pass
            if (stage == 0) {
                ScopedTimer t(e, KC_POST);
                hipLaunchKernelGGL(k_post_all, dim3((max_dist + 255) / 256, B, (unsigned)e->items.size()), dim3(256), 0, e->cur, D, B, dslabs);
            }
        }
    } else {
    if (e->items.size() > 1) HIP_OK(hipEventRecord(e->ev_fork, e->stream));
    // small batches are latency-bound: the items run on forked streams; the item with the largest distortion product is
    // the critical path and is enqueued first, on the main stream
    std::vector<size_t> order(e->items.size());
    for (size_t i = 0; i < order.size(); ++i) order[i] = i;
    std::stable_sort(order.begin(), order.end(), [&](size_t a, size_t b) {
        return (int64_t)e->items[a]->dev.d.n_dist * e->items[a]->dev.d.n_model > (int64_t)e->items[b]->dev.d.n_dist * e->items[b]->dev.d.n_model; });
    for (size_t oi = 0; oi < order.size(); ++oi) {
        const size_t q = order[oi];
        ItemHost* it = e->items[q];
        const ItemDev& d = it->dev;
        e->cur = oi == 0 ? e->stream : e->aux[oi - 1];
        if (oi > 0) HIP_OK(hipStreamWaitEvent(e->cur, e->ev_fork, 0));
        metal_products(it);
        // a single walker is latency-bound: its distortion product assembles x while staging it and finishes
        // each row with the post step, instead of three launches
        const bool fuse = B == 1 && it->has_dm && gemv1_applies(1, d.n_model_pad) && !e->no_fuse;
        if (!fuse) {
            ScopedTimer t(e, KC_ASSEMBLE);
            hipLaunchKernelGGL(k_assemble, dim3((d.d.n_model + 255) / 256, B), dim3(256), 0, e->cur, D, (int)q);
        }
        int dist_slabs = 1;
        if (it->has_dm)
            dist_slabs = launch_product(e, KC_DISTORTION, it->dm.p, d.n_model_pad, 0, d.d.n_dist, d.n_model_pad,
                                        it->vec.p, d.n_model_pad, 0, B, it->dist.p, d.n_dist_pad, 0, 1, e->slab_rows,
                                        nullptr, fuse ? (int)q : -1);
        else if (it->has_csr) launch_csr(e, it, B);
        if (!fuse) {
            ScopedTimer t(e, KC_POST);
            hipLaunchKernelGGL(k_post, dim3((d.d.n_dist + 255) / 256, B), dim3(256), 0, e->cur, D, (int)q, B, dist_slabs);
        }
        if (it->has_cinv && !e->gcinv.p)
            slabs.z[q] = launch_product(e, KC_INVCOV, it->cinv.p, d.n_masked_pad, 0, d.n_masked, d.n_masked_pad,
                                        it->res.p, d.n_masked_pad, 0, B, it->z.p, d.n_masked_pad, 0, 1, e->slab_rows,
                                        nullptr, -1, true);
        if (oi > 0) HIP_OK(hipEventRecord(e->ev_join[oi - 1], e->cur));
    }
    e->cur = e->stream;
    for (size_t q = 1; q < e->items.size(); ++q) HIP_OK(hipStreamWaitEvent(e->stream, e->ev_join[q - 1], 0));
    }
    e->cur = e->stream;
    if (grouped && cinv_tape_applies(e, B)) {
        vmx_engine::QuadList* ql = cinv_work_list(e, B);
        if (!ql) return -2;
        {
            ScopedTimer t(e, KC_INVCOV);
            cinv_launch_list(e, ql, B);
        }
        ScopedTimer t(e, KC_CHI2);
        hipLaunchKernelGGL(k_chi2_parts, dim3((B + 3) / 4), dim3(256), 0, e->stream, D, B, (const double*)ql->part.p,
                           (const int32_t*)ql->nt_off.p, 0);
        HIP_OK(hipGetLastError());
        e->last_B = B;
        e->last_full = true;
        return 0;
    }
    slabs.g = 1;
    if (e->gcinv.p)
        slabs.g = launch_product(e, KC_INVCOV, e->gcinv.p, e->g_ld, 0, e->g_n, e->g_ld, e->gres.p, e->g_ld, 0, B,
                                 e->gz.p, e->g_ld, 0, 1, e->slab_rows, nullptr, -1, true);
    {
        ScopedTimer t(e, KC_CHI2);
        hipLaunchKernelGGL(k_chi2, dim3(B), dim3(CHI2_THREADS), 0, e->stream, D, B, slabs);
    }
    HIP_OK(hipGetLastError());
    e->last_B = B;
    e->last_full = true;
    return 0;
}

// The products and the output kernel of vmx_marg_coeff_device for the B walkers run_chain has just taken up to their vectors:
// folded = true: y = G dx from the quadratic form's dx (q_x), out = c0[mock(b)] - y; false: y = M . residual of the full chain.
// Split-K slabs in fixed order; everything on the engine's stream, into buffers made outside (marg_workspace).
static int marg_products(vmx_engine* e, const EngineDev& D, int B, bool folded)
{
    const vmx_engine::MargReq& r = *e->marg_req;
    MargOutArgs A{};
    int n = 0, off = 0;
    e->cur = e->stream;
    for (size_t q = 0; q < e->items.size(); ++q) {
        ItemHost* it = e->items[q];
        if (it->n_templates <= 0) continue;
        const ItemDev& d = it->dev;
        const int nt = it->n_templates, ldt = vmx_pad(nt);
        MargOutItem& m = A.p[n++];
        m.item = (int)q; m.n = nt; m.ld = ldt; m.off = off; m.y = it->mg_y.p;
        off += nt;
        if (folded) {
            m.slabs = launch_product(e, KC_MATVEC, it->mg_g.p, d.nq_pad, 0, nt, d.nq_pad, it->q_x.p, d.nq_pad, 0, B,
                                     it->mg_y.p, ldt, 0, 1, e->marg_slab_rows);
            m.c0 = it->mg_c0.p;
        } else {
            m.slabs = launch_product(e, KC_MATVEC, it->marg.p, d.n_masked_pad, 0, nt, d.n_masked_pad, it->res.p, d.n_masked_pad, 0, B,
                                     it->mg_y.p, ldt, 0, 1, e->marg_slab_rows);
            m.c0 = nullptr;
        }
    }
    A.out = r.out; A.ld_out = r.ld_out; A.status_out = r.status; A.finish = folded ? 1 : 0;
    if (n > 0) {
        ScopedTimer t(e, KC_POST);
        hipLaunchKernelGGL(k_marg_out, dim3(B, n), dim3(256), 0, e->stream, D, A, B);
    }
    HIP_OK(hipGetLastError());
    return 0;
}

// run the chain for B walkers: replay a captured graph when one exists (or can be captured), else launch eagerly
static int run_chain_cached(vmx_engine* e, int B, int tab_mode, bool zero_copy = false, bool quad = false)
{
    if (e->n_xtab == 0) tab_mode = 0;
    // (the covariance tape of the full chain is built - allocations, uploads - outside any stream capture)
    if (!quad && B > 8 && e->items.size() <= VMX_MAX_GROUP && cinv_tape_applies(e, B) && !cinv_work_list(e, B)) return -2;
    if (!e->use_graphs || e->profiling) return run_chain(e, B, tab_mode, zero_copy, nullptr, nullptr, nullptr, quad);
    const int key = (((B * 4 + tab_mode) * 2 + (zero_copy ? 1 : 0)) * 2 + (e->direct ? 1 : 0)) * 2 + (quad ? 1 : 0);
    auto it = e->graphs.find(key);
    if (it == e->graphs.end()) {
        if (e->graphs.size() >= 64) return run_chain(e, B, tab_mode, zero_copy, nullptr, nullptr, nullptr, quad);
        hipGraph_t graph = nullptr;
        HIP_OK(hipStreamBeginCapture(e->stream, hipStreamCaptureModeThreadLocal));
        const int rc = run_chain(e, B, tab_mode, zero_copy, nullptr, nullptr, nullptr, quad);
        hipError_t err = hipStreamEndCapture(e->stream, &graph);
        if (rc || err != hipSuccess || graph == nullptr) {
            if (graph) (void)hipGraphDestroy(graph);
            std::fprintf(stderr, "[vegamx] stream capture failed (%s): falling back to eager launches\n",
                         err != hipSuccess ? hipGetErrorString(err) : "launch error");
            (void)hipGetLastError();
            e->use_graphs = false;      // capture is not available: stay on eager launches
            return run_chain(e, B, tab_mode, zero_copy, nullptr, nullptr, nullptr, quad);
        }
        hipGraphExec_t exec = nullptr;
        err = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
        (void)hipGraphDestroy(graph);
        if (err != hipSuccess) {
            std::fprintf(stderr, "[vegamx] graph instantiation failed (%s): falling back to eager launches\n", hipGetErrorString(err));
            e->use_graphs = false;
            return run_chain(e, B, tab_mode, zero_copy, nullptr, nullptr, nullptr, quad);
        }
        it = e->graphs.emplace(key, exec).first;
        vmx_engine::ChainFacts& captured = e->graph_route[key];       // (of the capture: the launches the graph replays)
        captured.route = e->last_route;
        captured.taps = e->last_taps;
        captured.fft_form = e->last_fft_form;
        captured.tab2_kt = e->last_tab2_kt;
    }
    HIP_OK(hipGraphLaunch(it->second, e->stream));
    e->last_B = B;
    e->last_full = !quad;
    e->last_form = quad ? (e->quad_factored ? 2 : 1) : 0;       // (a replayed graph runs no host code: run_chain set this at capture only)
    const vmx_engine::ChainFacts& facts = e->graph_route[key];
    e->last_route = facts.route;
    e->last_taps = facts.taps;
    e->last_fft_form = facts.fft_form;
    e->last_tab_level = tab_mode;          // (vmx_debug_read 4 [4], [2]: of this chain, not of the last one captured)
    e->last_tab2_kt = facts.tab2_kt;
    return 0;
}

// G = M X^T [n_templates][nq_pad] of an item with a marginalisation map, from the gathered X = (S DM')^T [nq][n_masked_pad] that
// quad_build has just made for Q' / F (allocated once: static like them, and lanes hold views)
static int marg_fold_matrix(vmx_engine* e, ItemHost* it, const double* X)
{
    if (it->n_templates <= 0) return 0;
    const ItemDev& d = it->dev;
    if (it->mg_g.p == nullptr && it->mg_g.alloc((size_t)it->n_templates * d.nq_pad, true)) return -2;
    launch_product(e, KC_OTHER, X, d.n_masked_pad, 0, d.nq, d.n_masked_pad, it->marg.p, d.n_masked_pad, 0, it->n_templates,
                   it->mg_g.p, d.nq_pad, 0, 1, it->n_templates);
    return 0;
}

// Build (or refresh) the static tensors of the quadratic form of chi2: the reference point is evaluated with the full
// chain (its pre-distortion vectors x0 and its model m0 come from the engine's own kernels), then per item
//   X = (S DM')^T,  W = X C^-1,  Q' = W X^T (stored in half form),  g_k = W (d_k - S m0),  c0_k = (d_k - S m0)^T C^-1 (d_k - S m0)
// for the data vector (k = 0) and every mock of the pool, all with the engine's product kernels.  Returns 0, or a
// negative code; a reference point the model cannot be evaluated at switches the form off (the full chain then runs).
static int quad_build(vmx_engine* e)
{
    drop_lane(e);           // (the tensors of the form are re-made: a second lane would keep views of the old ones)
    HIP_OK(hipStreamSynchronize(e->stream));
    const int P = e->n_params;
    std::vector<double> tref(e->theta_ref);
    if (!e->blind_scale.empty())
        for (int i = 0; i < P; ++i) tref[i] = e->blind_scale[i] == 1.0 ? tref[i] + e->blind_shift[i] : e->blind_scale[i] * tref[i] + e->blind_shift[i];
    HIP_OK(hipMemcpy(e->theta.p, tref.data(), (size_t)P * sizeof(double), hipMemcpyHostToDevice));
    e->no_fuse = true;
    const int rc = run_chain(e, 1, false);
    e->no_fuse = false;
    if (rc) return rc;
    HIP_OK(hipStreamSynchronize(e->stream));
    int32_t st = 0;
    HIP_OK(hipMemcpy(&st, e->status.p, sizeof(int32_t), hipMemcpyDeviceToHost));
    if (st) {
        std::fprintf(stderr, "[vegamx] the reference point of the quadratic chi2 form cannot be evaluated (status %d): full chain only\n", st);
        e->quad_eligible = false;
        return 0;
    }
    e->cur = e->stream;
    // Which form: Q' costs nq^2 flops per walker and item (half form), the factored form 2 n_masked nq.  The tape of the Q'
    // product runs at 0.7 of the MFMA peak and needs no reduction of slabs, the factored product is a plain grouped launch:
    // it has to win by a third to be taken (nq > 2.67 n_masked: a model grid finer than the data grid, COEFMOD >= 2).
    {
        double cost_q = 0.0, cost_f = 0.0;
        for (auto* it : e->items) {
            int na = 0;
            for (int q = 0; q < it->dev.n_bb[VMX_BB_POST_ADD]; ++q) na += it->dev.bb[VMX_BB_POST_ADD][q].n_coef;
            const double nq = it->dev.d.n_model + na;
            cost_q += nq * nq; cost_f += 2.0 * it->dev.n_masked * nq;
        }
        const bool fact = e->quad_kind == 2 || (e->quad_kind == 0 && cost_f < 0.75 * cost_q);
        if (fact != e->quad_factored) { e->quad_factored = fact; e->quad_mat_dirty = true; }
    }
    // The Q' form's quadratic term over a root of Q': Q' = F^T F with F = U S DM' [n_masked][nq] has rank <= n_masked, and an
    // orthogonal Qt turns F into a lower-trapezoidal L = Qt^T F - dx^T Q' dx = || L dx ||^2 exactly, for n_masked nq - n_masked^2 / 2
    // multiply-adds per walker instead of the half triangle's nq^2 / 2.  Built when that is the smaller number for the items together
    // (which tape a batch size takes is priced in quad_build_tape); the linear and constant terms stay those of Q'.
    bool want_root = !e->quad_factored && !e->no_quad_root && e->items.size() <= VMX_MAX_GROUP;
    {
        double tri = 0.0, trap = 0.0;
        for (auto* it : e->items) {
            int na = 0;
            for (int q = 0; q < it->dev.n_bb[VMX_BB_POST_ADD]; ++q) na += it->dev.bb[VMX_BB_POST_ADD][q].n_coef;
            const double nq = it->dev.d.n_model + na, nm = it->dev.n_masked;
            if (nm > nq) want_root = false;
            tri += 0.5 * nq * nq; trap += nm * nq - 0.5 * nm * nm;
        }
        if (!e->force_quad_root && !(trap < tri)) want_root = false;
    }
    bool root_ok = want_root, rebuilt = false;
    for (auto* it : e->items) {
        ItemDev& d = it->dev;
        const int nm = d.n_masked, nmp = d.n_masked_pad;
        int na = 0;
        std::vector<int64_t> boff;
        for (int q = 0; q < d.n_bb[VMX_BB_POST_ADD]; ++q) {
            const BBTermDev& term = d.bb[VMX_BB_POST_ADD][q];
            for (int c = 0; c < term.n_coef; ++c) { d.q_slot[na++] = term.slot[c]; boff.push_back(term.basis_off + (int64_t)c * d.d.n_dist); }
        }
        d.q_na = na; d.nq = d.d.n_model + na; d.nq_pad = vmx_pad(d.nq);
        {
            // k_xi_assemble_quad's lean path: both components are plain spline sums with the standard bias evolution
            bool plain = d.d.pipe_peak != d.d.pipe_smooth;
            bool lean = plain;
            for (int pq : {d.d.pipe_peak, d.d.pipe_smooth}) {
                const PipeDev& P = e->pipes[pq];
                if (P.d.tracer[0].evol_kind != VMX_EVOL_STD || P.d.tracer[1].evol_kind != VMX_EVOL_STD ||
                    P.d.uv_shotnoise || P.odd_rel || P.odd_asy || P.poly_basis >= 0) { plain = false; lean = false; }
                if (P.d.radiation) plain = false;
            }
            // ... on the same bins (each pipeline carries its own copy of the coordinates)
            const PipeDev& Pp = e->pipes[d.d.pipe_peak];
            const PipeDev& Ps = e->pipes[d.d.pipe_smooth];
            if (Pp.split_evol != Ps.split_evol || Pp.n != Ps.n) { plain = false; lean = false; }
            for (const std::vector<double>* h : {&e->h_r, &e->h_mu_c, &e->h_lnrelz, &e->h_lnrelz2, &e->h_growth})
                if ((plain || lean) && std::memcmp(h->data() + Pp.coord_off, h->data() + Ps.coord_off, (size_t)Pp.n * sizeof(double)) != 0) { plain = false; lean = false; }
            d.plain_pair = plain ? 1 : 0;
            it->lean_pair = lean;
        }
        const int nq = d.nq, nqp = d.nq_pad;
        // (Q' [nq][nq_pad], its factor F [n_masked][nq_pad] and the gathered rows X [nq][n_masked_pad] are operands of k_gemm_nt44)
        REQUIRE(gemm44_addressable(nq, nqp) && gemm44_addressable(nq, nmp) && gemm44_addressable(nm, nqp),
                "quadratic form: " GEMM44_LIMIT_MSG);
        // reference vector x0' = [vec(theta_ref) ; (1 + bao) c_j(theta_ref)]
        std::vector<double> x0((size_t)nqp, 0.0);
        HIP_OK(hipMemcpy(x0.data(), it->vec.p, (size_t)d.d.n_model * sizeof(double), hipMemcpyDeviceToHost));
        for (int j = 0; j < na; ++j) x0[d.d.n_model + j] = (e->direct ? 1.0 : 1.0 + tref[d.d.bao_amp_slot]) * tref[d.q_slot[j]];
        if (it->q_x0.upload(x0.data(), x0.size())) return -2;

        DevBuf<int32_t> midx;
        if (midx.upload(it->mask_idx.data(), it->mask_idx.size())) return -2;
        DevBuf<double>& cfull = it->q_cfull;       // (kept: the linear terms of mocks that arrive later need it, vmx_fit_migrad)
        if (it->has_cinv) {
            if (cfull.n < (size_t)nm * nmp && cfull.alloc((size_t)nm * nmp, true)) return -2;
            hipLaunchKernelGGL(k_sym_from_half, dim3((nm + 255) / 256, nm), dim3(256), 0, e->stream, cfull.p, it->cinv.p, nm, nmp);
        }
        if (it->q_m0.n < (size_t)nmp && it->q_m0.alloc((size_t)nmp, true)) return -2;
        hipLaunchKernelGGL(k_mask_gather, dim3((nm + 255) / 256), dim3(256), 0, e->stream, it->q_m0.p, (const double*)(e->model.p + d.model_off), midx.p, nm);
        if (e->quad_factored && (e->quad_mat_dirty || it->q_f.p == nullptr)) {
            // F = U X^T with C^-1 = U^T U: the Cholesky factor of the inverse covariance on the host (vmx_plan.h; n^3 / 3 flops,
            // a second for n = 3180 - set-up, redone only when the covariance changes)
            std::vector<double> hu((size_t)nm * nmp, 0.0);
            if (it->has_cinv) {
                std::vector<double> hc((size_t)nm * nmp);
                HIP_OK(hipStreamSynchronize(e->stream));
                HIP_OK(hipMemcpy(hc.data(), cfull.p, hc.size() * sizeof(double), hipMemcpyDeviceToHost));
                if (!vmx_plan::cholesky_lower(hc.data(), nm, nmp)) {
                    std::fprintf(stderr, "[vegamx] the inverse covariance of an item is not positive definite: chi2 keeps the Q' form\n");
                    e->quad_kind = 1;
                    return quad_build(e);
                }
                for (int i = 0; i < nm; ++i)
                    for (int m = 0; m <= i; ++m) hu[(size_t)m * nmp + i] = hc[(size_t)i * nmp + m];       // U = L^T
            } else
                for (int i = 0; i < nm; ++i) hu[(size_t)i * nmp + i] = 1.0;
            if (it->q_u.p == nullptr && it->q_u.alloc((size_t)nm * nmp, true)) return -2;
            HIP_OK(hipMemcpy(it->q_u.p, hu.data(), hu.size() * sizeof(double), hipMemcpyHostToDevice));
            DevBuf<double> X;
            DevBuf<int64_t>& bo = it->q_basis_off;
            boff.push_back(0);
            if (bo.upload(boff.data(), boff.size())) return -2;
            if (X.alloc((size_t)nq * nmp, true)) return -2;
            hipLaunchKernelGGL(k_quad_gather, dim3((nm + 255) / 256, nq), dim3(256), 0, e->stream, X.p, nmp,
                               it->has_dm ? it->dm.p : (const double*)nullptr, d.n_model_pad, midx.p, nm, (int)d.d.n_model, nq,
                               e->bb_basis.p, bo.p, (int)d.d.n_dist, it->has_csr ? 1 : 0);
            if (it->has_csr)
                hipLaunchKernelGGL(k_quad_gather_csr, dim3(nm), dim3(256), 0, e->stream, X.p, nmp, it->csr_ptr.p, it->csr_idx.p,
                                   it->csr_val.p, midx.p, nm);
            // F[m][j] = sum_i X[j][i] U[m][i]  (allocated once: captured graphs hold the pointer)
            if (it->q_f.p == nullptr && it->q_f.alloc((size_t)nm * nqp, true)) return -2;
            launch_product(e, KC_OTHER, X.p, nmp, 0, nq, nmp, it->q_u.p, nmp, 0, nm, it->q_f.p, nqp, 0, 1, nm);
            if (marg_fold_matrix(e, it, X.p)) return -2;
            HIP_OK(hipStreamSynchronize(e->stream));        // X is released here
        }
        if (!e->quad_factored && (e->quad_mat_dirty || it->q_mat.p == nullptr)) {
            DevBuf<double> X, qfull;
            DevBuf<int64_t>& bo = it->q_basis_off;
            boff.push_back(0);
            if (bo.upload(boff.data(), boff.size())) return -2;
            if (X.alloc((size_t)nq * nmp, true)) return -2;
            hipLaunchKernelGGL(k_quad_gather, dim3((nm + 255) / 256, nq), dim3(256), 0, e->stream, X.p, nmp,
                               it->has_dm ? it->dm.p : (const double*)nullptr, d.n_model_pad, midx.p, nm, (int)d.d.n_model, nq,
                               e->bb_basis.p, bo.p, (int)d.d.n_dist, it->has_csr ? 1 : 0);
            if (it->has_csr)
                hipLaunchKernelGGL(k_quad_gather_csr, dim3(nm), dim3(256), 0, e->stream, X.p, nmp, it->csr_ptr.p, it->csr_idx.p,
                                   it->csr_val.p, midx.p, nm);
            // (allocated once: captured graphs hold these pointers, and the sizes never change)
            if (it->q_w.p == nullptr && it->q_w.alloc((size_t)nq * nmp, true)) return -2;
            if (it->has_cinv)
                launch_product(e, KC_OTHER, cfull.p, nmp, 0, nm, nmp, X.p, nmp, 0, nq, it->q_w.p, nmp, 0, 1, nq);
            else
                HIP_OK(hipMemcpyAsync(it->q_w.p, X.p, (size_t)nq * nmp * sizeof(double), hipMemcpyDeviceToDevice, e->stream));
            if (qfull.alloc((size_t)nq * nqp, true)) return -2;
            launch_product(e, KC_OTHER, X.p, nmp, 0, nq, nmp, it->q_w.p, nmp, 0, nq, qfull.p, nqp, 0, 1, nq);
            if (it->q_mat.p == nullptr && it->q_mat.alloc((size_t)nq * nqp, true)) return -2;
            hipLaunchKernelGGL(k_half_from_full, dim3((nqp + 255) / 256, nq), dim3(256), 0, e->stream, it->q_mat.p, qfull.p, nq, nqp);
            if (marg_fold_matrix(e, it, X.p)) return -2;
            rebuilt = true;
            DevBuf<double> U, qr_part, qr_v, qr_row;
            std::vector<double> hu;
            if (root_ok) {
                // F = U X^T with C^-1 = U^T U, by the factored form's own steps (the Cholesky factor on the host, vmx_plan.h) ...
                hu.assign((size_t)nm * nmp, 0.0);
                if (it->has_cinv) {
                    std::vector<double> hc((size_t)nm * nmp);
                    HIP_OK(hipStreamSynchronize(e->stream));
                    HIP_OK(hipMemcpy(hc.data(), cfull.p, hc.size() * sizeof(double), hipMemcpyDeviceToHost));
                    if (!vmx_plan::cholesky_lower(hc.data(), nm, nmp)) {
                        std::fprintf(stderr, "[vegamx] the inverse covariance of an item is not positive definite: chi2 keeps the Q' form\n");
                        root_ok = false;
                    }
                    for (int i = 0; i < nm && root_ok; ++i)
                        for (int m = 0; m <= i; ++m) hu[(size_t)m * nmp + i] = hc[(size_t)i * nmp + m];       // U = L^T
                } else
                    for (int i = 0; i < nm; ++i) hu[(size_t)i * nmp + i] = 1.0;
            }
            if (root_ok) {
                if (U.upload(hu.data(), hu.size())) return -2;
                // (allocated once: captured graphs and lanes hold the pointer)
                if (it->q_root.p == nullptr && it->q_root.alloc((size_t)nm * nqp, true)) return -2;
                launch_product(e, KC_OTHER, X.p, nmp, 0, nq, nmp, U.p, nmp, 0, nm, it->q_root.p, nqp, 0, 1, nm);
                // ... and F -> L in place by Householder reflectors from the last column on (k_qr_dot / k_qr_apply, vmx_device.h):
                // backward stable whatever the condition of F, no atomics, fixed orders - L is the same bit for bit on every rebuild
                const int chunks_max = (nm + QR_CH - 1) / QR_CH;
                if (qr_part.alloc((size_t)chunks_max * nqp, true) || qr_v.alloc((size_t)nmp, true) || qr_row.alloc((size_t)nqp, true)) return -2;
                for (int t = 0; t + 1 < nm; ++t) {
                    const int r = nm - 1 - t, j = nq - 1 - t, chunks = r / QR_CH + 1;
                    const dim3 grid((unsigned)(j / 256 + 1), (unsigned)chunks);
                    hipLaunchKernelGGL(k_qr_dot, grid, dim3(256), 0, e->stream, (const double*)it->q_root.p, nqp, r, j, qr_part.p, qr_v.p, qr_row.p);
                    hipLaunchKernelGGL(k_qr_apply, grid, dim3(256), 0, e->stream, it->q_root.p, nqp, r, j, chunks, (const double*)qr_part.p,
                                       (const double*)qr_v.p, (const double*)qr_row.p);
                }
                HIP_OK(hipGetLastError());
            }
            HIP_OK(hipStreamSynchronize(e->stream));        // X / qfull are released here
        }
        // linear terms for the data vector and every mock of the pool
        const int rows = 1 + it->n_mocks;
        DevBuf<double> R0, T;
        if (R0.alloc((size_t)rows * nmp, true)) return -2;
        hipLaunchKernelGGL(k_quad_rows, dim3((nm + 255) / 256, rows), dim3(256), 0, e->stream, R0.p, nmp,
                           (const double*)(e->model.p + d.model_off), midx.p, it->data.p,
                           it->n_mocks ? it->mock_pool.p : (const double*)nullptr, nm, rows);
        if (it->q_lin.alloc((size_t)rows * nqp, true) || it->q_c0.alloc(rows, true)) return -2;
        if (e->quad_factored) {
            // u0 = U r0 per data vector / mock
            if (it->q_u0.alloc((size_t)rows * nmp, true)) return -2;
            launch_product(e, KC_OTHER, it->q_u.p, nmp, 0, nm, nmp, R0.p, nmp, 0, rows, it->q_u0.p, nmp, 0, 1, rows);
            if (it->q_y.n < (size_t)e->fact_slab_rows * nmp && it->q_y.alloc((size_t)e->fact_slab_rows * nmp, true)) return -2;
            d.q_u0 = it->q_u0.p; d.q_y = it->q_y.p;
        } else
        launch_product(e, KC_OTHER, it->q_w.p, nmp, 0, nq, nmp, R0.p, nmp, 0, rows, it->q_lin.p, nqp, 0, 1, rows);
        if (e->quad_factored) {}
        else if (it->has_cinv) {
            if (T.alloc((size_t)rows * nmp, true)) return -2;
            launch_product(e, KC_OTHER, cfull.p, nmp, 0, nm, nmp, R0.p, nmp, 0, rows, T.p, nmp, 0, 1, rows);
            hipLaunchKernelGGL(k_rowdot, dim3(rows), dim3(256), 0, e->stream, it->q_c0.p, R0.p, T.p, nmp, nm);
        } else {
            hipLaunchKernelGGL(k_rowdot, dim3(rows), dim3(256), 0, e->stream, it->q_c0.p, R0.p, R0.p, nmp, nm);
        }
        if (it->n_templates > 0) {
            // c0 = M r0 per data vector / mock, beside q_lin / q_c0 (reallocated only when the pool's size changed)
            const int ldt = vmx_pad(it->n_templates);
            if (it->mg_c0.n != (size_t)rows * ldt && it->mg_c0.alloc((size_t)rows * ldt, true)) return -2;
            launch_product(e, KC_OTHER, it->marg.p, nmp, 0, it->n_templates, nmp, R0.p, nmp, 0, rows, it->mg_c0.p, ldt, 0, 1, rows);
        }
        it->q_rows = rows;
        if (it->q_x.n < (size_t)e->max_batch * nqp && it->q_x.alloc((size_t)e->max_batch * nqp, true)) return -2;
        if (!e->quad_factored && it->q_z.n < (size_t)e->slab_rows * nqp && it->q_z.alloc((size_t)e->slab_rows * nqp, true)) return -2;
        HIP_OK(hipGetLastError());
        HIP_OK(hipStreamSynchronize(e->stream));
        it->h_q_c0.resize(rows);
        HIP_OK(hipMemcpy(it->h_q_c0.data(), it->q_c0.p, (size_t)rows * sizeof(double), hipMemcpyDeviceToHost));
        d.q_x0 = it->q_x0.p; d.q_lin = it->q_lin.p; d.q_c0 = it->q_c0.p; d.q_x = it->q_x.p; d.q_z = it->q_z.p;
    }
    std::vector<ItemDev> items;
    for (auto* it : e->items) items.push_back(it->dev);
    HIP_OK(hipMemcpy(e->d_items.p, items.data(), items.size() * sizeof(ItemDev), hipMemcpyHostToDevice));
    if (rebuilt || e->quad_factored) {
        // (tapes were planned with or without the roots: plan them again when that changed - the graphs are dropped below anyway)
        const bool have = root_ok && !e->quad_factored;
        if (have != e->quad_root) {
            for (auto& q : e->quad_lists) delete q.second;
            e->quad_lists.clear();
        }
        e->quad_root = have;
    }
    e->quad_mat_dirty = false;
    e->quad_lin_dirty = false;
    e->last_B = 0;                  // the reference evaluation is not a caller's evaluation
    // graphs captured before hold the previous per-mock buffers (q_lin / q_c0 grow with the pool): capture again
    for (auto& g : e->graphs) (void)hipGraphExecDestroy(g.second);
    e->graphs.clear(); e->graph_route.clear();
    return 0;
}

// chi2-only evaluations take the quadratic form when it applies; refreshes its tensors when data or covariances changed
static int quad_ready(vmx_engine* e, bool* use, int B)
{
    *use = false;
    if (!e->quad_eligible || e->theta_ref.empty() || e->direct) return 0;
    if (e->quad_mat_dirty || e->quad_lin_dirty) {
        if (quad_build(e)) return -2;
        if (!e->quad_eligible) return 0;
    }
    // (device allocations must not happen inside a stream capture: the work list of this batch size is built here)
    if (B > 8 && e->items.size() <= VMX_MAX_GROUP && !quad_work_list(e, B)) return -2;
    *use = true;
    return 0;
}

// The second lane of an engine: every static tensor borrowed (DevBuf copies are views), the per-batch workspace, the
// tables of the batch's shared parameters, the work lists' partial-sum buffers, stream and events its own.
static vmx_engine* clone_lane(vmx_engine* e)
{
    auto* L = new vmx_engine(*e);
    // what the copy must not share (or free)
    L->lanes.clear(); L->n_lanes = 1; L->lane_calls = 0;
    L->sample_stores.clear();
    L->chain_stores.clear(); L->chain_store = nullptr;      // (the stores belong to the engine they were created on, not to its lanes)
    L->fitws = nullptr; L->ensws = nullptr; L->nsws = nullptr; L->smcws = nullptr; L->lane_wait = nullptr; L->ev_rows = nullptr; L->ev_lane = nullptr; L->call_mock = nullptr;
    L->stream = nullptr; L->cur = nullptr; L->aux.clear(); L->ev_join.clear(); L->ev_fork = nullptr;
    L->graphs.clear(); L->graph_route.clear(); L->quad_lists.clear(); L->cinv_lists.clear(); L->host_allocs.clear(); L->spans.clear(); L->span_used = 0; L->profiling = false;
    L->pin_theta = nullptr; L->pin_chi2 = nullptr; L->pin_status = nullptr; L->pin_done = nullptr; L->pin_part = nullptr;
    L->dpin_theta = nullptr; L->dpin_chi2 = nullptr; L->dpin_status = nullptr; L->dpin_done = nullptr; L->dpin_part = nullptr;
    L->host_key_valid = false; L->pending_key.clear();
    std::map<MetalHost*, MetalHost*> metal_map;
    L->metals.clear();
    for (auto* m : e->metals) { auto* c = new MetalHost(*m); metal_map[m] = c; L->metals.push_back(c); }
    L->items.clear();
    for (auto* it : e->items) {
        auto* c = new ItemHost(*it);
        for (auto*& m : c->metals) m = metal_map[m];
        L->items.push_back(c);
    }
    auto fail_out = [&]() -> vmx_engine* { delete L; return nullptr; };
    if (hipStreamCreate(&L->stream) != hipSuccess) return fail_out();
    L->cur = L->stream;
    for (size_t q = 1; q < L->items.size(); ++q) {
        hipStream_t st = nullptr; hipEvent_t ev = nullptr;
        if (hipStreamCreate(&st) != hipSuccess || hipEventCreateWithFlags(&ev, hipEventDisableTiming) != hipSuccess) return fail_out();
        L->aux.push_back(st); L->ev_join.push_back(ev);
    }
    if (hipEventCreateWithFlags(&L->ev_fork, hipEventDisableTiming) != hipSuccess) return fail_out();
    // per-batch workspace (sizes as in vmx_finalize)
    const int Bm = e->max_batch, n_pipe = (int)e->pipes.size();
    const size_t ncols = (size_t)Bm * n_pipe, acols = (size_t)Bm * std::max(e->n_active, 1);
    for (auto* b : {&L->theta, &L->scal, &L->metal_bias, &L->pl, &L->coef, &L->xi, &L->xim, &L->model, &L->chi2, &L->xtab, &L->xtab_k,
                    &L->xtab_key, &L->gres, &L->gz, &L->mv_part, &L->pk_direct}) b->forget();
    for (auto* b : {&L->status, &L->k_live, &L->coef_win}) b->forget();
    L->gemm_trace.forget(); L->pk_trace.forget(); L->d_items.forget();
    if (L->theta.alloc((size_t)Bm * e->n_params) || L->scal.alloc(ncols * VMX_NS) ||
        L->metal_bias.alloc((size_t)Bm * 3 * (e->metals.size() + 1)) ||
        L->pl.alloc((size_t)VMX_MAX_ELL * acols * e->nkp) || L->coef.alloc((size_t)VMX_MAX_ELL * acols * e->ncp) ||
        L->xi.alloc((size_t)e->xi_total) || L->xim.alloc((size_t)e->xim_total) ||
        L->model.alloc((size_t)Bm * e->model_size) || L->chi2.alloc(Bm) || L->status.alloc(Bm) || L->k_live.alloc(8)) return fail_out();
    {
        const int32_t empty_window[2] = {0x7fffffff, -1};
        if (L->coef_win.upload(empty_window, 2)) return fail_out();
    }
    if (e->n_xtab > 0) {
        std::vector<double> key((size_t)2 * e->n_xtab * VMX_XTAB_KEY + 1, std::nan(""));
        if (L->xtab.alloc(((size_t)e->n_xtab * 2 * e->n_rows + 128) * e->nkp, true) || L->xtab_k.alloc((size_t)e->n_xtab * 4 * e->nkp, true) ||
            L->xtab_key.upload(key.data(), key.size())) return fail_out();
    }
    if (e->gcinv.p && (L->gres.alloc((size_t)Bm * e->g_ld, true) || L->gz.alloc((size_t)e->slab_rows * e->g_ld, true))) return fail_out();
    std::vector<ItemDev> items;
    for (auto* it : L->items) {
        ItemDev& d = it->dev;
        for (auto* b : {&it->vec, &it->dist, &it->res, &it->z, &it->marg_out, &it->q_x, &it->q_z, &it->q_y}) {
            const size_t n = b->n;
            b->forget();
            if (n > 0 && b != &it->marg_out && b->alloc(n, true)) return fail_out();
        }
        d.vec = it->vec.p; d.dist = it->dist.p; d.res = it->res.p; d.z = it->z.p; d.q_x = it->q_x.p; d.q_z = it->q_z.p; d.q_y = it->q_y.p;
        items.push_back(d);
    }
    if (L->d_items.upload(items.data(), items.size())) return fail_out();
    EngineDev& D = L->dev;
    D.xtab = L->xtab.p; D.xtab_key = L->xtab_key.p; D.xtab_k = L->xtab_k.p;
    D.items = L->d_items.p;
    D.theta = L->theta.p; D.scal = L->scal.p; D.metal_bias = L->metal_bias.p; D.pl = L->pl.p; D.coef = L->coef.p;
    D.xi = L->xi.p; D.xim = L->xim.p; D.model = L->model.p; D.chi2 = L->chi2.p; D.status = L->status.p; D.k_live = L->k_live.p;
    D.coef_win = L->coef_win.p; D.pk_trace = nullptr; D.gres = L->gres.p; D.gz = L->gz.p; D.pk_direct = nullptr;
    L->direct = false;
    if (hipStreamSynchronize(e->stream) != hipSuccess) return fail_out();
    return L;
}

// vmx_eval_device and its variants.  d_mock: this call's walkers are compared with those rows of the mock pools (device
// pointer, [B]; nullptr: the rows of vmx_set_mock_index); eager: no captured graph for small batches (a caller whose batch size
// changes from call to call - the fit driver - would capture one per size).
static int eval_device_impl(vmx_engine* e, const double* d_theta, int32_t B, double* d_chi2, double* d_model, int32_t* d_status,
                            const int32_t* d_mock, bool eager)
{
    e->host_key_valid = false;          // (device-resident walkers may rebuild the tables: the host no longer knows their key)
    bool quad = false;
    if (!d_model && quad_ready(e, &quad, B)) return -2;
    e->last_stream = e->stream;
    // two lanes: independent chi2-only batches alternate between this engine's workspace and its clone's, each on its own
    // stream - the kernels of one batch fill the first and last block rounds of the other's (every kernel of a B = 256
    // chain spends 20 - 30 % of its launch there).  Anything else waits for the second lane first.
    const bool two_lanes = e->n_lanes > 1 && quad && !d_model && e->blind_scale.empty() && B >= 64 && !e->direct &&
                           !(e->profiling && e->prof_mask == 0xffffffffu);
    struct MockScope {          // the per-call rows apply to the engine (or lane) that runs this call, and to this call only
        vmx_engine* x; MockScope(vmx_engine* x_, const int32_t* m) : x(x_) { x->call_mock = m; } ~MockScope() { x->call_mock = nullptr; }
    };
    if (!two_lanes) wait_lane(e);
    else if (const int which = (int)(e->lane_calls++ % e->n_lanes)) {
        while ((int)e->lanes.size() < which) {
            vmx_engine* made = clone_lane(e);
            if (!made) return fail(-2, "could not create another lane");
            e->lanes.push_back(made);
        }
        vmx_engine* L = e->lanes[which - 1];
        L->const_hint = e->const_hint;
        bool lq = false;
        if (quad_ready(L, &lq, B)) return -2;       // (its work lists: the tensors are the borrowed ones)
        if (!lq) return fail(-2, "the second lane cannot take the quadratic form");
        const int tab = (B >= 16 && L->n_xtab > 0) ? L->const_hint : 0;
        if (e->lane_wait) HIP_OK(hipStreamWaitEvent(L->stream, e->lane_wait, 0));
        MockScope scope(L, d_mock);
        if (run_chain(L, B, tab, false, d_theta, d_chi2, d_status, true)) return -2;
        e->last_stream = L->stream;
        return 0;
    }
    MockScope scope(e, d_mock);
    if (!e->blind_scale.empty()) {
        // parameter-level blinding: the walkers are transformed in the engine's own copy
        HIP_OK(hipMemcpyAsync(e->theta.p, d_theta, (size_t)B * e->n_params * sizeof(double), hipMemcpyDeviceToDevice, e->stream));
        const int n = B * e->n_params;
        hipLaunchKernelGGL(k_theta_affine, dim3((n + 255) / 256), dim3(256), 0, e->stream, e->theta.p, e->d_blind.p, e->n_params, n);
        const int tab = (B >= 16 && e->n_xtab > 0) ? e->const_hint : 0;
        if (eager ? run_chain(e, B, tab, false, nullptr, nullptr, nullptr, quad) : run_chain_cached(e, B, B >= 16 ? e->const_hint : 0, false, quad)) return -2;
        if (d_chi2) HIP_OK(hipMemcpyAsync(d_chi2, e->chi2.p, (size_t)B * sizeof(double), hipMemcpyDeviceToDevice, e->stream));
        if (d_status) HIP_OK(hipMemcpyAsync(d_status, e->status.p, (size_t)B * sizeof(int32_t), hipMemcpyDeviceToDevice, e->stream));
    } else if (B >= 64 || !e->use_graphs || e->profiling || eager) {
        // large batches: eager launches cost nothing next to the kernels, and they let the chain read / write the
        // caller's buffers directly (a captured graph would pin their addresses)
        const int tab = (B >= 16 && e->n_xtab > 0) ? e->const_hint : 0;
        if (run_chain(e, B, tab, false, d_theta, d_chi2, d_status, quad)) return -2;
    } else {
        HIP_OK(hipMemcpyAsync(e->theta.p, d_theta, (size_t)B * e->n_params * sizeof(double), hipMemcpyDeviceToDevice, e->stream));
        if (run_chain_cached(e, B, B >= 16 ? e->const_hint : 0, false, quad)) return -2;
        if (d_chi2) HIP_OK(hipMemcpyAsync(d_chi2, e->chi2.p, (size_t)B * sizeof(double), hipMemcpyDeviceToDevice, e->stream));
        if (d_status) HIP_OK(hipMemcpyAsync(d_status, e->status.p, (size_t)B * sizeof(int32_t), hipMemcpyDeviceToDevice, e->stream));
    }
    if (d_model) HIP_OK(hipMemcpyAsync(d_model, e->model.p, (size_t)B * e->model_size * sizeof(double), hipMemcpyDeviceToDevice, e->stream));
    return 0;
}

int vmx_eval_device(vmx_engine* e, const double* d_theta, int32_t B, double* d_chi2, double* d_model,
                    int32_t* d_status)
{
    REQUIRE(e && e->finalized && d_theta, "vmx_eval_device");
    REQUIRE(B > 0 && B <= e->max_batch, "batch exceeds max_batch");
    HIP_OK(hipSetDevice(e->device));
    return eval_device_impl(e, d_theta, B, d_chi2, d_model, d_status, nullptr, false);
}

int vmx_eval_device_mocks(vmx_engine* e, const double* d_theta, int32_t B, double* d_chi2, int32_t* d_status,
                          const int32_t* d_mock_index)
{
    REQUIRE(e && e->finalized && d_theta && d_mock_index, "vmx_eval_device_mocks");
    REQUIRE(B > 0 && B <= e->max_batch, "batch exceeds max_batch");
    HIP_OK(hipSetDevice(e->device));
    return eval_device_impl(e, d_theta, B, d_chi2, nullptr, d_status, d_mock_index, true);
}

// ---- fits where the walkers live (vmx_fit.h)
static_assert(sizeof(vmx_fit_stage) == sizeof(vmx_migrad::StageSpec) && sizeof(vmx_fit_spec) == sizeof(vmx_migrad::Spec),
              "include/vegamx.h and vmx_migrad.h describe the same fit");
static_assert(VMX_FIT_MAXN == vmx_migrad::MAXN && VMX_FIT_MAX_STAGES == vmx_migrad::MAX_STAGES, "fit limits");

// the table level (vmx_set_constant_nl_hint) that batches whose rows differ only in the columns `varies` allow, as vmx_eval derives
// it from host walkers
static int derived_const_hint(const vmx_engine* e, const std::vector<char>& varies)
{
    int hint = e->n_xtab > 0 ? (e->no_tab2 ? 1 : 2) : 0;
    for (int slot : e->const_slots) if (varies[slot]) hint = 0;
    for (int slot : e->const_slots2) if (hint == 2 && varies[slot]) hint = 1;
    return hint;
}

int vmx_derived_const_hint(vmx_engine* e, const int32_t* varies)
{
    REQUIRE(e && e->finalized && varies, "vmx_derived_const_hint");
    std::vector<char> v(e->n_params, 0);
    for (int c = 0; c < e->n_params; ++c) v[c] = varies[c] != 0;
    return derived_const_hint(e, v);
}

namespace {

// The engine as one call's likelihood (vmx_fit_migrad and the three samplers): chi2-only device evaluations of a driver's rows,
// eager launches, in chunks, two lanes when the quadratic form serves them, at the table level the caller states or the columns
// that vary allow.  Open it once every argument has been checked; however the call ends, the engine is then as it was.
struct LikelihoodSession {
    vmx_engine* e;
    int hint, chunk, lanes;                 // what the call runs with (the stats report them)
    int saved_hint, saved_lanes;
    bool saved_ring;
    // the three option integers of a call (the samplers refuse a negative chunk or lanes, the fits read them as "default")
    static int check(const std::string& fn, int hint, int chunk, int lanes, bool refuse_negative)
    {
        REQUIRE(hint >= -1 && hint <= 2, fn + ": const_hint -1 (derive it), 0, 1 or 2");
        REQUIRE(!refuse_negative || (chunk >= 0 && lanes >= 0), fn + ": chunk, lanes");
        return 0;
    }
    // hint -1: derived from `varies`; chunk <= 0: default_chunk; lanes <= 0: 2
    LikelihoodSession(vmx_engine* e_, int hint_, int chunk_, int lanes_, int default_chunk, const std::vector<char>& varies)
        : e(e_), hint(hint_ < 0 ? derived_const_hint(e_, varies) : hint_),
          chunk(std::max(1, std::min(chunk_ > 0 ? chunk_ : default_chunk, e_->max_batch))),
          saved_hint(e_->const_hint), saved_lanes(e_->n_lanes), saved_ring(e_->ring_allowed)
    {
        const int want = lanes_ > 0 ? std::min(lanes_, VMX_MAX_LANES) : 2;
        e->const_hint = hint;
        if (want > e->n_lanes) { e->n_lanes = want; e->ring_allowed = false; }
        e->lane_calls = 0;
        lanes = e->n_lanes;
    }
    LikelihoodSession(const LikelihoodSession&) = delete;
    ~LikelihoodSession()
    {
        wait_lane(e);
        e->lane_wait = nullptr;
        e->const_hint = saved_hint; e->n_lanes = saved_lanes; e->ring_allowed = saved_ring; e->lane_calls = 0;
        e->last_stream = e->stream;
    }
    // The engine's chain over the first `total` rows of `theta` into chi2 / status (mock: the rows' mocks, or nullptr); e->stream then
    // waits for the second lane, so that the driver's next kernel reads every chunk's answer.  rows_from_kernel: a kernel on
    // e->stream wrote the rows and the host has not waited since, so the second lane's stream waits for them at lane_wait;
    // otherwise nothing is recorded and nothing waits unless the lane ran.  Returns the engine calls made, negative on failure.
    int evaluate(const double* theta, int total, double* chi2, int32_t* status, const int32_t* mock, bool rows_from_kernel)
    {
        hipStream_t st = e->stream, lane_stream = nullptr;
        if (rows_from_kernel) {
            if (!e->ev_rows) HIP_OK(hipEventCreateWithFlags(&e->ev_rows, hipEventDisableTiming));
            HIP_OK(hipEventRecord(e->ev_rows, st));
            e->lane_wait = e->ev_rows;
        }
        int calls = 0;
        for (int off = 0; off < total; off += chunk, ++calls) {
            const int B = std::min(chunk, total - off);
            if (eval_device_impl(e, theta + (size_t)off * e->n_params, B, chi2 + off, nullptr, status + off, mock ? mock + off : nullptr, true)) return -2;
            if (e->last_stream != st) lane_stream = e->last_stream;
        }
        if (lane_stream) {
            if (!e->ev_lane) HIP_OK(hipEventCreateWithFlags(&e->ev_lane, hipEventDisableTiming));
            HIP_OK(hipEventRecord(e->ev_lane, lane_stream));
            HIP_OK(hipStreamWaitEvent(st, e->ev_lane, 0));
        }
        return calls;
    }
};

// The sampled box of the three samplers (fn: the caller, for the messages): n of the engine's columns, none twice, each with
// finite limits lo < hi, beside the fixed row and a finite log_norm.  varies[p]: column p is sampled; inv[p]: as which, or -1.
extern "C++" template <typename Spec>      // (the three specs start alike; this stretch of the file has C linkage)
static int check_box(const std::string& fn, const vmx_engine* e, const Spec* spec, int max_n, std::vector<char>& varies, std::vector<int32_t>& inv)
{
    const int P = e->n_params;
    REQUIRE(spec->n_params == P && spec->theta_fixed && spec->col && spec->lo && spec->hi, fn + ": parameter columns, limits and the fixed row");
    REQUIRE(spec->n >= 1 && spec->n <= max_n, fn + ": 1 .. " + std::to_string(max_n) + " sampled columns");
    varies.assign(P, 0);
    inv.assign(P, -1);
    for (int i = 0; i < spec->n; ++i) {
        REQUIRE(spec->col[i] >= 0 && spec->col[i] < P, fn + ": parameter column");
        REQUIRE(!varies[spec->col[i]], fn + ": a column is listed twice");
        varies[spec->col[i]] = 1;
        inv[spec->col[i]] = i;
        REQUIRE(std::isfinite(spec->lo[i]) && std::isfinite(spec->hi[i]) && spec->lo[i] < spec->hi[i], fn + ": limits");
    }
    REQUIRE(std::isfinite(spec->log_norm), fn + ": log_norm");
    return 0;
}

}  // namespace

int vmx_fit_migrad(vmx_engine* e, const vmx_fit_spec* spec, int32_t n_fits, const double* theta0, const int32_t* mock_row,
                   const vmx_fit_options* opt, vmx_fit_result* results, vmx_fit_stats* stats)
{
    REQUIRE(e && e->finalized && spec && theta0 && results && n_fits > 0, "vmx_fit_migrad");
    REQUIRE(spec->n_stages >= 1 && spec->n_stages <= VMX_FIT_MAX_STAGES && spec->n_params == e->n_params, "vmx_fit_migrad: stages / parameter columns");
    REQUIRE(spec->iterate >= 1 && spec->maxfcn > 0 && spec->up > 0.0 && spec->tol > 0.0, "vmx_fit_migrad: iterate, maxfcn, up, tol");
    int max_req = 1, n_max = 1;
    for (int s = 0; s < spec->n_stages; ++s) {
        const vmx_fit_stage& st = spec->stage[s];
        const vmx_fit_result& r = results[s];
        REQUIRE(r.x && r.ext && r.V && r.fval && r.edm && r.flags && r.nfcn && r.n_iter, "vmx_fit_migrad: result arrays of every stage");
        n_max = std::max(n_max, (int)st.n);
        REQUIRE(st.n >= 1 && st.n <= VMX_FIT_MAXN, "vmx_fit_migrad: 1 .. 32 free parameters per stage");
        for (int i = 0; i < st.n; ++i) {
            REQUIRE(st.col[i] >= 0 && st.col[i] < e->n_params, "vmx_fit_migrad: parameter column");
            for (int j = 0; j < i; ++j) REQUIRE(st.col[j] != st.col[i], "vmx_fit_migrad: a column is listed twice");
            REQUIRE(!(st.has_lo[i] && st.has_hi[i]) || st.hi[i] > st.lo[i], "vmx_fit_migrad: limits");
            REQUIRE(st.err[i] > 0.0, "vmx_fit_migrad: step sizes must be positive");
        }
        max_req = std::max(max_req, vmx_migrad::max_request(st.n));
    }
    const vmx_mock_stream* ms = opt ? opt->mocks : nullptr;
    int wave = 0, n_waves = 0;
    std::vector<int64_t> draw_off;          // column of every item's draws in a mock's row
    if (ms) {
        // mocks made while the fits run: fit f is fitted to pool row f, admitted with its wave
        REQUIRE(ms->n_mocks == n_fits && ms->draws && ms->n_drawn && !e->gcinv.p, "vmx_fit_migrad: a mock stream makes one mock per fit (no global covariance)");
        int64_t off = 0;
        for (auto* it : e->items) {
            REQUIRE(it->has_factor && it->has_mask, "vmx_fit_migrad: vmx_item_set_mock_factor for every item first");
            draw_off.push_back(off);
            off += it->dev.n_masked;
        }
        REQUIRE(ms->stride >= off, "vmx_fit_migrad: the draws of a mock are its items' side by side");
        wave = ms->wave > 0 ? ms->wave : 64;
        n_waves = (n_fits + wave - 1) / wave;
        if (mock_row) for (int f = 0; f < n_fits; ++f) REQUIRE(mock_row[f] == f, "vmx_fit_migrad: with a mock stream fit f takes pool row f");
    }
    else if (mock_row)
        for (int f = 0; f < n_fits; ++f)
            for (auto* it : e->items) REQUIRE(mock_row[f] < 0 || mock_row[f] < it->n_mocks, "vmx_fit_migrad: mock row exceeds the pool");
    const int opt_hint = opt ? opt->const_hint : -1;
    if (LikelihoodSession::check("vmx_fit_migrad", opt_hint, 0, 0, false)) return -1;
    std::vector<char> varies(e->n_params, 0);
    if (opt_hint < 0) {
        // a column varies when a stage frees it or the fits' rows differ in it
        for (int s = 0; s < spec->n_stages; ++s)
            for (int i = 0; i < spec->stage[s].n; ++i) varies[spec->stage[s].col[i]] = 1;
        for (int f = 1; f < n_fits; ++f)
            for (int c = 0; c < e->n_params; ++c)
                if (theta0[(size_t)f * e->n_params + c] != theta0[c]) varies[c] = 1;
    }
    HIP_OK(hipSetDevice(e->device));
    const auto t_begin = std::chrono::steady_clock::now();
    wait_lane(e);
    HIP_OK(hipStreamSynchronize(e->stream));

    const int F = n_fits, P = e->n_params;
    const size_t cap = (size_t)F * max_req;
    std::vector<int32_t> own_rows;
    if (ms) {
        // pools of n_fits rows, to be filled wave by wave (rows that have not arrived are zeros: nothing reads them before their
        // fits are admitted); the quadratic form's per-mock terms are sized for them by the build the first evaluation triggers
        // (a run of the same size as the last one finds its pools, the form's per-mock rows and the second lane as they are: the
        // waves overwrite the rows their fits read, nothing reads a row before its wave has come)
        bool resized = false;
        for (auto* it : e->items)
            if (it->mock_pool.n < (size_t)n_fits * it->dev.n_masked || it->n_mocks != n_fits || !it->dev.mock_pool) resized = true;
        if (resized) drop_lane(e);
        for (size_t q = 0; q < e->items.size(); ++q) {
            ItemHost* it = e->items[q];
            const size_t need = (size_t)n_fits * it->dev.n_masked;
            if (resized) {
                if (it->mock_pool.n < need && it->mock_pool.alloc(need, true)) return -2;
                it->n_mocks = n_fits;
                it->dev.mock_pool = it->mock_pool.p;
                HIP_OK(hipMemcpy(e->d_items.p + q, &it->dev, sizeof(ItemDev), hipMemcpyHostToDevice));
                e->quad_lin_dirty = true;
            }
            const size_t rows = (size_t)wave * it->dev.n_masked_pad;
            if (ensure(it->mc_z, rows) || ensure(it->mc_noise, rows) || ensure(it->mc_r0, rows) || ensure(it->mc_t, rows)) return -2;
            HIP_OK(hipMemset(it->mc_z.p, 0, rows * sizeof(double)));       // (the pad columns of the draws stay zero)
            // (... and those of the residual rows: k_mock_rows writes the columns below n_masked, the products and row dots of a
            // wave read all n_masked_pad, and 0 . NaN is no zero; mc_noise and mc_t are read below n_masked only)
            HIP_OK(hipMemset(it->mc_r0.p, 0, rows * sizeof(double)));
        }
        own_rows.resize(n_fits);
        for (int f = 0; f < n_fits; ++f) own_rows[f] = f;
        mock_row = own_rows.data();
    }
    if (!e->fitws) e->fitws = new FitWorkspace();
    FitWorkspace& W = *e->fitws;
    const int fit_cap = n_max <= 4 ? 4 : n_max <= 8 ? 8 : n_max <= 16 ? 16 : 32;
    const size_t state_bytes = fit_state_bytes(fit_cap);
    // (W.state carries structs - phases, counts - among its doubles: exempt from poison, and cleared whole below)
    if (ensure_structs(W.state, (size_t)F * state_bytes / sizeof(double)) || ensure(W.done, F) || ensure(W.spec, 1) || ensure(W.base, (size_t)F * P) || ensure(W.theta, cap * P) || ensure(W.chi2, cap) ||
        ensure(W.mock_row, F) || ensure(W.count, F) || ensure(W.offset, (size_t)F + 1) || ensure(W.mock, cap) || ensure(W.status, cap)) return -2;
    for (int s = 0; s < spec->n_stages; ++s) {
        const size_t n = spec->stage[s].n;
        if (ensure(W.ox[s], F * n) || ensure(W.oext[s], F * n) || ensure(W.oV[s], F * n * n) || ensure(W.ofval[s], F) || ensure(W.oedm[s], F) ||
            ensure(W.oflags[s], F) || ensure(W.oiter[s], F) || ensure(W.onfcn[s], F)) return -2;
    }
    if (!W.pin_word) {
        HIP_OK(hipHostMalloc((void**)&W.pin_word, 16 * sizeof(int32_t), hipHostMallocMapped));
        HIP_OK(hipHostGetDevicePointer((void**)&W.dpin_word, W.pin_word, 0));
    }
    hipStream_t st = e->stream;
    HIP_OK(hipMemsetAsync(W.state.p, 0, (size_t)F * state_bytes, st));       // (all zeros = a fit at its start)
    HIP_OK(hipMemsetAsync(W.done.p, 0, (size_t)F * sizeof(int32_t), st));
    HIP_OK(hipMemsetAsync(W.offset.p, 0, ((size_t)F + 1) * sizeof(int32_t), st));
    HIP_OK(hipMemcpyAsync(W.spec.p, spec, sizeof(vmx_fit_spec), hipMemcpyHostToDevice, st));
    HIP_OK(hipMemcpyAsync(W.base.p, theta0, (size_t)F * P * sizeof(double), hipMemcpyHostToDevice, st));
    if (mock_row) HIP_OK(hipMemcpyAsync(W.mock_row.p, mock_row, (size_t)F * sizeof(int32_t), hipMemcpyHostToDevice, st));

    FitDev D{};
    D.state = W.state.p; D.spec = W.spec.p; D.base = W.base.p; D.mock_row = mock_row ? W.mock_row.p : nullptr;
    for (int s = 0; s < spec->n_stages; ++s)
        D.out[s] = vmx_migrad::StageOut{W.ox[s].p, W.oext[s].p, W.oV[s].p, W.ofval[s].p, W.oedm[s].p, W.oflags[s].p, W.onfcn[s].p, W.oiter[s].p};
    D.count = W.count.p; D.offset = W.offset.p; D.done = W.done.p; D.theta = W.theta.p; D.mock = W.mock.p; D.chi2 = W.chi2.p;
    D.host_word = W.dpin_word; D.F = F; D.P = P; D.admitted = ms ? 0 : F;

    // the engine as the fits' objective, the round's rows in chunks of 512 unless the caller says otherwise
    LikelihoodSession L(e, opt_hint, opt ? opt->chunk : 0, opt ? opt->lanes : 0, 512, varies);
    const int chunk = L.chunk;

    vmx_fit_stats S{};
    const size_t emit_lds = (size_t)((P + 1) & ~1) * sizeof(int32_t) + vmx_migrad::MAXN * sizeof(double);
    if (fit_round(fit_cap, D, st, emit_lds, true)) return -2;
    const auto t_loop = std::chrono::steady_clock::now();
    double wait_s = 0.0;
    size_t gap_used = 0;
    int next_wave = 0;
    double producer_wait_s = 0.0, wave_host_s = 0.0;
    bool quad_form = false;
    if (ms && quad_ready(e, &quad_form, chunk)) return -2;       // (the form's tensors, with room for every mock's terms)
    for (;;) {
        if (ms && next_wave < n_waves) {
            // Wave `next_wave` joins at this round - a fixed schedule (one wave per round from the start), so that the rounds'
            // batches, hence every bit of every chi2, do not depend on how fast the draws arrive; the host waits for the producer
            // when it is behind.  The wave's mocks = fiducial + L . draws with the chain's product kernels (reference
            // vega/data.py:751-753), then their rows of the quadratic form's linear terms and constants, all on the stream
            // ahead of the round's bookkeeping.
            const int a = next_wave * wave, b = std::min(n_fits, a + wave), cnt = b - a;
            const auto t_p0 = std::chrono::steady_clock::now();
            const double limit = ms->timeout_seconds > 0.0 ? ms->timeout_seconds : 600.0;
            while (*ms->n_drawn < b) {
                if (std::chrono::duration<double>(std::chrono::steady_clock::now() - t_p0).count() > limit)
                    return fail(-2, "vmx_fit_migrad: the producer of the mock draws stalled");
                std::this_thread::sleep_for(std::chrono::microseconds(20));
            }
            producer_wait_s += std::chrono::duration<double>(std::chrono::steady_clock::now() - t_p0).count();
            std::atomic_thread_fence(std::memory_order_acquire);
            e->cur = st;
            for (size_t q = 0; q < e->items.size(); ++q) {
                ItemHost* it = e->items[q];
                const ItemDev& d = it->dev;
                const int nm = d.n_masked, nmp = d.n_masked_pad;
                HIP_OK(hipMemcpy2DAsync(it->mc_z.p, (size_t)nmp * sizeof(double), ms->draws + (size_t)a * ms->stride + draw_off[q],
                                        (size_t)ms->stride * sizeof(double), (size_t)nm * sizeof(double), cnt, hipMemcpyHostToDevice, st));
                launch_product(e, KC_OTHER, it->mc_chol.p, nmp, 0, nm, nmp, it->mc_z.p, nmp, 0, cnt, it->mc_noise.p, nmp, 0, 1, cnt);
                hipLaunchKernelGGL(k_mock_rows, dim3((nm + 255) / 256, cnt), dim3(256), 0, st, it->mock_pool.p + (size_t)a * nm,
                                   quad_form ? it->mc_r0.p : (double*)nullptr, nmp, (const double*)it->mc_noise.p, (const double*)it->mc_fid.p,
                                   (const double*)it->q_m0.p, nm, cnt);
                if (!quad_form) continue;
                if (e->quad_factored)
                    launch_product(e, KC_OTHER, it->q_u.p, nmp, 0, nm, nmp, it->mc_r0.p, nmp, 0, cnt, it->q_u0.p + (size_t)(1 + a) * nmp, nmp, 0, 1, cnt);
                else {
                    launch_product(e, KC_OTHER, it->q_w.p, nmp, 0, d.nq, nmp, it->mc_r0.p, nmp, 0, cnt, it->q_lin.p + (size_t)(1 + a) * d.nq_pad, d.nq_pad, 0, 1, cnt);
                    if (it->has_cinv) {
                        launch_product(e, KC_OTHER, it->q_cfull.p, nmp, 0, nm, nmp, it->mc_r0.p, nmp, 0, cnt, it->mc_t.p, nmp, 0, 1, cnt);
                        hipLaunchKernelGGL(k_rowdot, dim3(cnt), dim3(256), 0, st, it->q_c0.p + 1 + a, (const double*)it->mc_r0.p, (const double*)it->mc_t.p, nmp, nm);
                    } else
                        hipLaunchKernelGGL(k_rowdot, dim3(cnt), dim3(256), 0, st, it->q_c0.p + 1 + a, (const double*)it->mc_r0.p, (const double*)it->mc_r0.p, nmp, nm);
                }
            }
            HIP_OK(hipGetLastError());
            next_wave += 1;
            D.admitted = b;
            wave_host_s += std::chrono::duration<double>(std::chrono::steady_clock::now() - t_p0).count();
        }
        {
            const auto t_r0 = std::chrono::steady_clock::now();
            if (fit_round(fit_cap, D, st, emit_lds, false)) return -2;
            S.seconds_enqueuing_rounds += std::chrono::duration<double>(std::chrono::steady_clock::now() - t_r0).count();
        }
        if (gap_used + 2 > W.ev_gap.size()) {
            hipEvent_t a = nullptr, b = nullptr;
            HIP_OK(hipEventCreate(&a)); HIP_OK(hipEventCreate(&b));
            W.ev_gap.push_back(a); W.ev_gap.push_back(b);
        }
        HIP_OK(hipEventRecord(W.ev_gap[gap_used], st));
        const auto t_w0 = std::chrono::steady_clock::now();
        HIP_OK(hipStreamSynchronize(st));
        wait_s += std::chrono::duration<double>(std::chrono::steady_clock::now() - t_w0).count();
        const int total = W.pin_word[0];
        if (total <= 0 && (!ms || next_wave >= n_waves)) break;
        if (total <= 0) { HIP_OK(hipEventRecord(W.ev_gap[gap_used + 1], st)); gap_used += 2; continue; }      // (nothing asked for yet: the next wave joins)
        if ((size_t)total > cap) return fail(-2, "vmx_fit_migrad: a round asked for more rows than its buffers hold");
        HIP_OK(hipEventRecord(W.ev_gap[gap_used + 1], st));
        gap_used += 2;
        S.rounds += 1;
        S.evaluations += total;
        const auto t_c0 = std::chrono::steady_clock::now();
        // (the host has just waited for the stream: the rows are there for either lane)
        const int calls = L.evaluate(W.theta.p, total, W.chi2.p, W.status.p, mock_row ? W.mock.p : nullptr, false);
        if (calls < 0) return -2;
        S.engine_calls += calls;
        for (int off = 0; off < total; off += chunk) {
            const int B = std::min(chunk, total - off);
            int bin = 0;
            while (bin < 7 && B > (1 << (2 * bin))) ++bin;          // 1, 2..4, 5..16, 17..64, 65..256, 257..1024, 1025..4096, more
            S.calls_by_batch[bin] += 1;
            S.evaluations_by_batch[bin] += B;
        }
        S.seconds_enqueuing_calls += std::chrono::duration<double>(std::chrono::steady_clock::now() - t_c0).count();
    }
    S.fits_unfinished = W.pin_word[1];
    S.seconds_waiting_for_draws = producer_wait_s;
    S.seconds_enqueuing_waves = wave_host_s - producer_wait_s;
    if (ms && quad_form)        // (the host copy of the constants serves the single-walker chain of vmx_eval)
        for (auto* it : e->items)
            if (!e->quad_factored && it->h_q_c0.size() == (size_t)it->q_rows)
                HIP_OK(hipMemcpy(it->h_q_c0.data(), it->q_c0.p, it->h_q_c0.size() * sizeof(double), hipMemcpyDeviceToHost));
    const auto t_done = std::chrono::steady_clock::now();
    for (int s = 0; s < spec->n_stages; ++s) {
        const size_t n = spec->stage[s].n;
        const vmx_fit_result& r = results[s];
        HIP_OK(hipMemcpy(r.x, W.ox[s].p, F * n * sizeof(double), hipMemcpyDeviceToHost));
        HIP_OK(hipMemcpy(r.ext, W.oext[s].p, F * n * sizeof(double), hipMemcpyDeviceToHost));
        HIP_OK(hipMemcpy(r.V, W.oV[s].p, F * n * n * sizeof(double), hipMemcpyDeviceToHost));
        HIP_OK(hipMemcpy(r.fval, W.ofval[s].p, F * sizeof(double), hipMemcpyDeviceToHost));
        HIP_OK(hipMemcpy(r.edm, W.oedm[s].p, F * sizeof(double), hipMemcpyDeviceToHost));
        HIP_OK(hipMemcpy(r.flags, W.oflags[s].p, F * sizeof(int32_t), hipMemcpyDeviceToHost));
        HIP_OK(hipMemcpy(r.nfcn, W.onfcn[s].p, F * sizeof(int64_t), hipMemcpyDeviceToHost));
        HIP_OK(hipMemcpy(r.n_iter, W.oiter[s].p, F * sizeof(int32_t), hipMemcpyDeviceToHost));
    }
    double idle_ms = 0.0;
    for (size_t i = 0; i + 1 < gap_used; i += 2) {
        float t = 0.f;
        if (hipEventElapsedTime(&t, W.ev_gap[i], W.ev_gap[i + 1]) == hipSuccess) idle_ms += t;
    }
    const auto t_end = std::chrono::steady_clock::now();
    S.seconds = std::chrono::duration<double>(t_end - t_begin).count();
    S.seconds_setup = std::chrono::duration<double>(t_loop - t_begin).count();
    S.seconds_rounds = std::chrono::duration<double>(t_done - t_loop).count();
    S.seconds_host_waiting = wait_s;
    S.gpu_idle_seconds_between_rounds = idle_ms * 1e-3;
    if (stats) *stats = S;
    return 0;
}

// ---- posterior sampling where the walkers live (vmx_ensemble.h)
// what makes a run of E = G T ensembles G ladders of T rungs (vmx_ensemble_run_pt): the ladder, the sweeps, where the counts go
// (betas [T]; with `adapt`, vmx_ensemble_run_pt_adapt: betas [G][T], written back through betas_out with the call's history and
// the guard's counts)
struct EnsPtRun {
    int32_t G, T; const double* betas; int32_t swap_every; int64_t* swaps;
    const vmx_ensemble_adapt* adapt = nullptr; double* betas_out = nullptr; double* beta_hist = nullptr; int64_t* adapt_skipped = nullptr;
};
static int ensemble_run(const char* who, vmx_engine* e, const vmx_ensemble_spec* spec, int32_t E, int32_t W, const uint64_t* streams,
                        const int32_t* mock_row, double* x, double* lnL, int64_t* accepted, int64_t step0, int32_t n_steps,
                        int32_t thin, double* chain, double* chain_lnL, const vmx_ensemble_options* opt,
                        vmx_ensemble_stats* stats, int64_t* per_ensemble, const vmx_ensemble_moves* moves,
                        const EnsPtRun* pt = nullptr, const vmx_ensemble_cov* cov = nullptr, int64_t* fallbacks = nullptr);

// One ensemble is the set of one, on the stream of its spec
static int chain_store_check(const std::string& name, const vmx_chain_store* s, int32_t E, int32_t W, int32_t n, int64_t rows);
static int chain_store_take(vmx_chain_store* s, const double* chain, const double* chain_lnl, int64_t rows, hipStream_t st);

int vmx_ensemble_run(vmx_engine* e, const vmx_ensemble_spec* spec, int32_t W, double* x, double* lnL, int64_t* accepted,
                     int64_t step0, int32_t n_steps, int32_t thin, double* chain, double* chain_lnL,
                     const vmx_ensemble_options* opt, vmx_ensemble_stats* stats)
{
    REQUIRE(spec, "vmx_ensemble_run");
    return ensemble_run("vmx_ensemble_run", e, spec, 1, W, &spec->stream, nullptr, x, lnL, accepted, step0, n_steps, thin, chain,
                        chain_lnL, opt, stats, nullptr, nullptr);
}

int vmx_ensemble_run_many(vmx_engine* e, const vmx_ensemble_spec* spec, int32_t E, int32_t W, const uint64_t* streams,
                          const int32_t* mock_row, double* x, double* lnL, int64_t* accepted, int64_t step0, int32_t n_steps,
                          int32_t thin, double* chain, double* chain_lnL, const vmx_ensemble_options* opt,
                          vmx_ensemble_stats* stats, int64_t* per_ensemble)
{
    return ensemble_run("vmx_ensemble_run_many", e, spec, E, W, streams, mock_row, x, lnL, accepted, step0, n_steps, thin, chain,
                        chain_lnL, opt, stats, per_ensemble, nullptr);
}

// The same run with the walkers' moves drawn from a mixture (k_ens_half_moves); without moves it is vmx_ensemble_run_many
int vmx_ensemble_run_many_moves(vmx_engine* e, const vmx_ensemble_spec* spec, int32_t E, int32_t W, const uint64_t* streams,
                                const int32_t* mock_row, double* x, double* lnL, int64_t* accepted, int64_t step0, int32_t n_steps,
                                int32_t thin, double* chain, double* chain_lnL, const vmx_ensemble_options* opt,
                                vmx_ensemble_stats* stats, int64_t* per_ensemble, const vmx_ensemble_moves* moves)
{
    if (!moves)
        return ensemble_run("vmx_ensemble_run_many", e, spec, E, W, streams, mock_row, x, lnL, accepted, step0, n_steps, thin, chain,
                            chain_lnL, opt, stats, per_ensemble, nullptr);
    return ensemble_run("vmx_ensemble_run_many_moves", e, spec, E, W, streams, mock_row, x, lnL, accepted, step0, n_steps, thin,
                        chain, chain_lnL, opt, stats, per_ensemble, moves);
}

// The same run with the covariance move as the mixture's fourth member (k_ens_half_cov); without it, vmx_ensemble_run_many_moves
int vmx_ensemble_run_many_cov(vmx_engine* e, const vmx_ensemble_spec* spec, int32_t E, int32_t W, const uint64_t* streams,
                              const int32_t* mock_row, double* x, double* lnL, int64_t* accepted, int64_t step0, int32_t n_steps,
                              int32_t thin, double* chain, double* chain_lnL, const vmx_ensemble_options* opt,
                              vmx_ensemble_stats* stats, int64_t* per_ensemble, const vmx_ensemble_moves* moves,
                              const vmx_ensemble_cov* cov, int64_t* fallbacks)
{
    const std::string name("vmx_ensemble_run_many_cov");
    if (cov) {
        REQUIRE(std::isfinite(cov->weight) && cov->weight >= 0.0, name + ": the cov weight must be finite and not negative");
        REQUIRE(std::isfinite(cov->scale) && cov->scale > 0.0, name + ": the cov scale must be positive and finite");
        REQUIRE(cov->flags == 0 && cov->reserved == 0, name + ": flags and reserved must be 0");
    }
    if (!cov || !(cov->weight > 0.0)) {
        const int rc = vmx_ensemble_run_many_moves(e, spec, E, W, streams, mock_row, x, lnL, accepted, step0, n_steps, thin, chain,
                                                   chain_lnL, opt, stats, per_ensemble, moves);
        if (rc == 0 && fallbacks) std::fill(fallbacks, fallbacks + E, (int64_t)0);
        return rc;
    }
    REQUIRE(moves, name + ": a cov weight comes beside the weights of the other moves");
    return ensemble_run("vmx_ensemble_run_many_cov", e, spec, E, W, streams, mock_row, x, lnL, accepted, step0, n_steps, thin,
                        chain, chain_lnL, opt, stats, per_ensemble, moves, nullptr, cov, fallbacks);
}

// The factor stage of k_ens_half_cov alone, on halves the caller gives
int vmx_ensemble_cov_factor(vmx_engine* e, int32_t E, int32_t H, int32_t n, const double* x, double* mean, double* factor, int32_t* flag)
{
    const std::string name("vmx_ensemble_cov_factor");
    REQUIRE(e && x && mean && factor && flag, name);
    REQUIRE(E >= 1 && H >= 2 && n >= 1 && n <= VMX_ENS_MAXN, name + ": E >= 1, H >= 2, 1 <= n <= VMX_ENS_MAXN");
    REQUIRE((int64_t)E * H * n <= INT32_MAX, name + ": E H n is too large");
    HIP_OK(hipSetDevice(e->device));
    const size_t Ex = (size_t)E;
    DevBuf<double> dx, dmean, dfactor;
    DevBuf<int32_t> dflag;
    if (dx.alloc(Ex * H * n, false) || dmean.alloc(Ex * n, false) || dfactor.alloc(Ex * n * n, false) || dflag.alloc(Ex, false)) return -2;
    hipStream_t st = e->stream;
    HIP_OK(hipMemcpyAsync(dx.p, x, Ex * H * n * sizeof(double), hipMemcpyHostToDevice, st));
    // (the block of a run with this half)
    const dim3 grid(E), block(std::min(ENS_THREADS, std::max(64, (H + 63) / 64 * 64)));
    hipLaunchKernelGGL(k_ens_cov_factor, grid, block, 0, st, dx.p, H, n, dmean.p, dfactor.p, dflag.p);
    HIP_OK(hipGetLastError());
    HIP_OK(hipMemcpyAsync(mean, dmean.p, Ex * n * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_OK(hipMemcpyAsync(factor, dfactor.p, Ex * n * n * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_OK(hipMemcpyAsync(flag, dflag.p, Ex * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    return 0;
}

// G ladders of T rungs: the run of G T ensembles with the rung's beta in every decision (k_ens_half_pt) and a swap sweep between
// the rungs of a ladder after every swap_every-th step (k_ens_swap), on the main stream between the deciding half-step and the
// next proposal - no host wait, no likelihood row
static_assert(VMX_PT_MAXT == vmx_ens::PT_MAXT, "parallel tempering limits");
int vmx_ensemble_run_pt(vmx_engine* e, const vmx_ensemble_spec* spec, int32_t G, int32_t T, int32_t W, const double* betas,
                        const uint64_t* streams, const int32_t* mock_row, double* x, double* lnL, int64_t* accepted, int64_t step0,
                        int32_t n_steps, int32_t thin, int32_t swap_every, double* chain, double* chain_lnL,
                        const vmx_ensemble_options* opt, vmx_ensemble_stats* stats, int64_t* per_ensemble,
                        const vmx_ensemble_moves* moves, int64_t* swaps)
{
    const std::string name("vmx_ensemble_run_pt");
    REQUIRE(G >= 1, name + ": at least one ladder");
    REQUIRE(T >= 1 && T <= VMX_PT_MAXT, name + ": 1 <= T <= VMX_PT_MAXT rungs");
    REQUIRE(betas && vmx_ens::ladder_ok(betas, T), name + ": the ladder must start at 1, be finite, strictly decreasing and not negative");
    REQUIRE(swap_every >= 0, name + ": swap_every >= 0");
    REQUIRE(W >= 1 && (int64_t)G * T <= INT32_MAX && (int64_t)G * T * W <= INT32_MAX, name + ": G T W exceeds the engine's row count");
    std::vector<int32_t> rung_mock;         // (every rung of a ladder reads the ladder's mock)
    if (mock_row) {
        rung_mock.resize((size_t)G * T);
        for (int g = 0; g < G; ++g) std::fill(rung_mock.begin() + (size_t)g * T, rung_mock.begin() + (size_t)(g + 1) * T, mock_row[g]);
    }
    const EnsPtRun pt{G, T, betas, swap_every, swaps};
    return ensemble_run("vmx_ensemble_run_pt", e, spec, G * T, W, streams, mock_row ? rung_mock.data() : nullptr, x, lnL, accepted, step0,
                        n_steps, thin, chain, chain_lnL, opt, stats, per_ensemble, moves, &pt);
}

// The ladders of vmx_ensemble_run_pt, each with betas of its own that k_ens_swap_adapt moves after every sweep (vmx_ensemble.h, the
// fourth part): the same run, the same stream order - the k_ens_half_pt(record | propose) behind the sweep reads the new betas -
// and the same single host wait
int vmx_ensemble_run_pt_adapt(vmx_engine* e, const vmx_ensemble_spec* spec, int32_t G, int32_t T, int32_t W, double* betas,
                              const uint64_t* streams, const int32_t* mock_row, double* x, double* lnL, int64_t* accepted,
                              int64_t step0, int32_t n_steps, int32_t thin, int32_t swap_every, double* chain, double* chain_lnL,
                              const vmx_ensemble_options* opt, vmx_ensemble_stats* stats, int64_t* per_ensemble,
                              const vmx_ensemble_moves* moves, int64_t* swaps, const vmx_ensemble_adapt* adapt, double* beta_hist,
                              int64_t* adapt_skipped)
{
    const std::string name("vmx_ensemble_run_pt_adapt");
    REQUIRE(G >= 1, name + ": at least one ladder");
    REQUIRE(T >= 3 && T <= VMX_PT_MAXT, name + ": 3 <= T <= VMX_PT_MAXT rungs (an adaptive ladder moves the rungs between the first and the last)");
    REQUIRE(swap_every >= 1, name + ": swap_every >= 1 (the ladder adapts after a sweep)");
    REQUIRE(adapt, name + ": the adaptation settings");
    REQUIRE(vmx_ens::adapt_ok(T, swap_every, adapt->lag, adapt->time), name + ": lag and time must be finite and positive");
    REQUIRE(adapt->flags == 0 && adapt->reserved == 0, name + ": flags and reserved must be 0");
    REQUIRE(betas, name + ": the ladders");
    for (int g = 0; g < G; ++g)
        REQUIRE(vmx_ens::ladder_ok(betas + (size_t)g * T, T), name + ": every ladder must start at 1, be finite, strictly decreasing and not negative");
    REQUIRE(W >= 1 && (int64_t)G * T <= INT32_MAX && (int64_t)G * T * W <= INT32_MAX, name + ": G T W exceeds the engine's row count");
    std::vector<int32_t> rung_mock;         // (every rung of a ladder reads the ladder's mock)
    if (mock_row) {
        rung_mock.resize((size_t)G * T);
        for (int g = 0; g < G; ++g) std::fill(rung_mock.begin() + (size_t)g * T, rung_mock.begin() + (size_t)(g + 1) * T, mock_row[g]);
    }
    EnsPtRun pt{G, T, betas, swap_every, swaps};
    pt.adapt = adapt; pt.betas_out = betas; pt.beta_hist = beta_hist; pt.adapt_skipped = adapt_skipped;
    return ensemble_run("vmx_ensemble_run_pt_adapt", e, spec, G * T, W, streams, mock_row ? rung_mock.data() : nullptr, x, lnL, accepted,
                        step0, n_steps, thin, chain, chain_lnL, opt, stats, per_ensemble, moves, &pt);
}

// What every ensemble run refuses before anything runs: the box, the walkers, the steps, the sizes, the start and the mocks of E
// ensembles of W walkers, and the options of the engine's calls.  stretch: the run reads the stretch scale spec->a.
static int ensemble_check(const std::string& name, vmx_engine* e, const vmx_ensemble_spec* spec, int32_t E, int32_t W, const uint64_t* streams,
                          const int32_t* mock_row, const double* x, const double* lnL, const int64_t* accepted, int64_t step0,
                          int32_t n_steps, int32_t thin, const vmx_ensemble_options* opt, bool stretch, std::vector<char>& varies,
                          std::vector<int32_t>& inv)
{
    REQUIRE(e && e->finalized && spec && x && lnL && accepted, name);
    REQUIRE(E >= 1, name + ": at least one ensemble");
    REQUIRE(streams, name + ": a Philox stream for every ensemble");
    if (check_box(name, e, spec, VMX_ENS_MAXN, varies, inv)) return -1;
    const int n = spec->n, P = e->n_params;
    REQUIRE(W >= 2 * n && W % 2 == 0, name + ": an even number of walkers, at least twice the sampled columns");
    REQUIRE(!stretch || (spec->a > 1.0 && std::isfinite(spec->a)), name + ": the stretch scale a must exceed 1");
    REQUIRE(thin >= 1 && n_steps >= 0 && step0 >= 0, name + ": thin >= 1, n_steps >= 0, step0 >= 0");
    const int64_t rows = (step0 + n_steps) / thin - step0 / thin;
    // sizes: the engine's rows are counted in int32, the largest array (the chain, or the rows themselves) in size_t
    REQUIRE((int64_t)E * W <= INT32_MAX, name + ": E W exceeds the engine's row count");
    const size_t EW = (size_t)E * W, per_row = (size_t)std::max(n, P) * sizeof(double);
    REQUIRE(EW <= SIZE_MAX / per_row && (rows <= 0 || EW * per_row <= SIZE_MAX / (size_t)rows), name + ": the chain is too large");
    for (size_t w = 0; w < EW; ++w) {
        REQUIRE(std::isfinite(lnL[w]), name + ": a start walker has a non-finite lnL");
        for (int i = 0; i < n; ++i) {
            const double v = x[w * n + i];
            REQUIRE(v >= spec->lo[i] && v <= spec->hi[i], name + ": a start walker lies outside the box");
        }
    }
    if (mock_row)
        for (int q = 0; q < E; ++q)
            for (auto* it : e->items) {
                REQUIRE(it->n_mocks > 0 && it->dev.mock_pool, name + ": mock rows, but an item has no mock pool");
                REQUIRE(mock_row[q] >= 0 && mock_row[q] < it->n_mocks, name + ": mock row outside the pool");
            }
    return LikelihoodSession::check(name, opt ? opt->const_hint : -1, opt ? opt->chunk : 0, opt ? opt->lanes : 0, true);
}

// E independent ensembles advanced together (k_ens_half): the E H proposal rows of a half-step as one stream of chunks for the
// engine, every row with the mock of its ensemble
static int ensemble_run(const char* who, vmx_engine* e, const vmx_ensemble_spec* spec, int32_t E, int32_t W, const uint64_t* streams,
                        const int32_t* mock_row, double* x, double* lnL, int64_t* accepted, int64_t step0, int32_t n_steps,
                        int32_t thin, double* chain, double* chain_lnL, const vmx_ensemble_options* opt,
                        vmx_ensemble_stats* stats, int64_t* per_ensemble, const vmx_ensemble_moves* moves, const EnsPtRun* pt,
                        const vmx_ensemble_cov* cov, int64_t* fallbacks)
{
    const std::string name(who);
    std::vector<char> varies;
    std::vector<int32_t> inv;
    if (ensemble_check(name, e, spec, E, W, streams, mock_row, x, lnL, accepted, step0, n_steps, thin, opt, true, varies, inv)) return -1;
    const int n = spec->n, P = e->n_params;
    const int H = W / 2;
    EnsMovesDev M{};
    EnsCovDev Cv{};
    REQUIRE(!cov || (moves && !pt), name + ": the cov move comes with the moves' weights and without a ladder");
    if (moves) {
        const double* p = moves->weights;
        const double pc = cov ? cov->weight : 0.0;      // (the caller has checked the cov struct; + 0.0 changes no sum)
        REQUIRE(std::isfinite(p[0]) && std::isfinite(p[1]) && std::isfinite(p[2]) && p[0] >= 0.0 && p[1] >= 0.0 && p[2] >= 0.0,
                name + ": the moves' weights must be finite and not negative");
        if (cov) {
            const double p4[4] = {p[0], p[1], p[2], pc};
            vmx_ens::move_thresholds4(p4, M.t0, M.t1, Cv.t2);
            REQUIRE(std::isfinite(Cv.t2), name + ": the moves' weights must have a positive, finite sum");
            REQUIRE(H >= 2, name + ": the cov move needs two walkers in the other half, W >= 4");
            Cv.scale = cov->scale;
        } else {
            vmx_ens::move_thresholds(p, M.t0, M.t1);
        }
        REQUIRE(((p[0] + p[1]) + p[2]) + pc > 0.0 && std::isfinite(M.t0) && std::isfinite(M.t1), name + ": the moves' weights must have a positive, finite sum");
        REQUIRE(!(p[1] > 0.0) || H >= 2, name + ": the DE move needs two partners in the other half, W >= 4");
        REQUIRE(!(p[2] > 0.0) || H >= 3, name + ": the snooker move needs three partners in the other half, W >= 6");
        REQUIRE(std::isfinite(moves->gamma0) && moves->gamma0 > 0.0, name + ": gamma0 must be positive and finite");
        REQUIRE(std::isfinite(moves->gamma_s) && moves->gamma_s > 0.0, name + ": gamma_s must be positive and finite");
        REQUIRE(std::isfinite(moves->sigma) && moves->sigma >= 0.0, name + ": sigma must be finite and not negative");
        REQUIRE(moves->flags == 0 && moves->reserved == 0, name + ": flags and reserved must be 0");
        M.gamma0 = moves->gamma0; M.sigma = moves->sigma; M.gamma_s = moves->gamma_s;
    } else if (pt) {
        M.t0 = M.t1 = 1.0;      // (the pure stretch move of k_ens_half_pt: u < 1 always)
    }
    const int64_t rows = (step0 + n_steps) / thin - step0 / thin;
    const size_t EW = (size_t)E * W;
    const int EH = E * H;
    // (an attached chain store takes the recorded rows where they are: the kernels record whether or not the host wants them)
    vmx_chain_store* const store = e->chain_store;
    if (chain_store_check(name, store, E, W, n, rows)) return -1;
    const bool keep_x = chain || store, keep_lnl = chain_lnL || store;

    HIP_OK(hipSetDevice(e->device));
    const auto t_begin = std::chrono::steady_clock::now();
    if (!e->ensws) e->ensws = new EnsWorkspace();
    EnsWorkspace& S = *e->ensws;
    if (ensure(S.x, EW * n) || ensure(S.lnl, EW) || ensure(S.acc, EW) || ensure(S.n_box, EW) || ensure(S.n_fail, EW) ||
        ensure(S.prop, (size_t)EH * n) || ensure(S.factor, EH) || ensure(S.inside, EH) || ensure(S.col, n) || ensure(S.streams, E) ||
        (mock_row && ensure(S.mock, EH)))
        return -2;
    const size_t n_swaps = pt ? (size_t)pt->G * (size_t)(pt->T - 1) * 2 : 0;
    const vmx_ensemble_adapt* const ad = pt ? pt->adapt : nullptr;
    const size_t n_beta = pt ? (ad ? (size_t)pt->G * pt->T : (size_t)pt->T) : 0;
    // (the sweeps of this call: after the steps s in [step0, step0 + n_steps) with (s + 1) % swap_every == 0)
    const int64_t sweep0 = ad ? step0 / pt->swap_every : 0;
    const size_t n_hist = ad && pt->beta_hist ? (size_t)((step0 + n_steps) / pt->swap_every - sweep0) * n_beta : 0;
    if (pt && (ensure(S.beta, n_beta) || (n_swaps && ensure(S.swaps, n_swaps)))) return -2;
    if (cov && ensure(S.cov_fallbacks, E)) return -2;
    if (ad && (ensure(S.adapt_skipped, pt->G) || (n_hist && ensure(S.beta_hist, n_hist)))) return -2;
    if (keep_x && rows > 0 && ensure(S.chain, (size_t)rows * EW * n)) return -2;
    if (keep_lnl && rows > 0 && ensure(S.chain_lnl, (size_t)rows * EW)) return -2;
    hipStream_t st = e->stream;
    EnsDev D{};
    if (S.box.upload(EH, P, n, spec->theta_fixed, spec->lo, spec->hi, inv, st, D.box)) return -2;
    HIP_OK(hipMemcpyAsync(S.x.p, x, EW * n * sizeof(double), hipMemcpyHostToDevice, st));
    HIP_OK(hipMemcpyAsync(S.lnl.p, lnL, EW * sizeof(double), hipMemcpyHostToDevice, st));
    HIP_OK(hipMemcpyAsync(S.acc.p, accepted, EW * sizeof(int64_t), hipMemcpyHostToDevice, st));
    HIP_OK(hipMemsetAsync(S.n_box.p, 0, EW * sizeof(int64_t), st));
    HIP_OK(hipMemsetAsync(S.n_fail.p, 0, EW * sizeof(int64_t), st));
    HIP_OK(hipMemcpyAsync(S.col.p, spec->col, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, st));
    HIP_OK(hipMemcpyAsync(S.streams.p, streams, (size_t)E * sizeof(uint64_t), hipMemcpyHostToDevice, st));
    std::vector<int32_t> row_mock;          // (static for the call: row e H + k reads the mock of ensemble e)
    if (mock_row) {
        row_mock.resize(EH);
        for (int q = 0; q < E; ++q) std::fill(row_mock.begin() + (size_t)q * H, row_mock.begin() + (size_t)(q + 1) * H, mock_row[q]);
        HIP_OK(hipMemcpyAsync(S.mock.p, row_mock.data(), (size_t)EH * sizeof(int32_t), hipMemcpyHostToDevice, st));
    }
    const int32_t* d_mock = mock_row ? S.mock.p : nullptr;

    D.x = S.x.p; D.lnl = S.lnl.p; D.acc = S.acc.p; D.n_box = S.n_box.p; D.n_fail = S.n_fail.p;
    D.prop = S.prop.p; D.factor = S.factor.p; D.inside = S.inside.p;
    D.col = S.col.p;
    D.chain = keep_x && rows > 0 ? S.chain.p : nullptr; D.chain_lnl = keep_lnl && rows > 0 ? S.chain_lnl.p : nullptr;
    D.streams = S.streams.p; D.rows = rows;
    D.W = W; D.n = n; D.P = P; D.thin = thin; D.a = spec->a; D.log_norm = spec->log_norm;
    D.seed = spec->seed; D.step0 = step0;

    // the engine as the sampler's likelihood, at the table level the sampled columns allow
    LikelihoodSession L(e, opt ? opt->const_hint : -1, opt ? opt->chunk : 0, opt ? opt->lanes : 0, e->max_batch, varies);
    vmx_ensemble_stats R{};
    R.const_hint = L.hint;
    R.lanes = L.lanes;
    const auto t_loop = std::chrono::steady_clock::now();
    const int64_t halves = 2 * (int64_t)n_steps;
    // (every loop of the kernel strides by its block: the chain does not depend on this size)
    const dim3 grid(E), block(std::min(ENS_THREADS, std::max(64, (H + 63) / 64 * 64)));
    EnsPtDev Pt{};
    if (pt) {
        HIP_OK(hipMemcpyAsync(S.beta.p, pt->betas, n_beta * sizeof(double), hipMemcpyHostToDevice, st));
        if (n_swaps) HIP_OK(hipMemsetAsync(S.swaps.p, 0, n_swaps * sizeof(int64_t), st));
        Pt.beta = S.beta.p; Pt.swaps = n_swaps ? S.swaps.p : nullptr; Pt.T = pt->T; Pt.stride = ad ? pt->T : 0;
    }
    EnsAdaptDev Ad{};
    if (ad) {
        HIP_OK(hipMemsetAsync(S.adapt_skipped.p, 0, (size_t)pt->G * sizeof(int64_t), st));
        Ad.beta = S.beta.p; Ad.hist = n_hist ? S.beta_hist.p : nullptr; Ad.skipped = S.adapt_skipped.p;
        Ad.lag = ad->lag; Ad.tau = ad->time; Ad.sweep0 = sweep0; Ad.swap_every = pt->swap_every; Ad.G = pt->G;
    }
    if (cov) {
        HIP_OK(hipMemsetAsync(S.cov_fallbacks.p, 0, (size_t)E * sizeof(int64_t), st));
        Cv.fallbacks = S.cov_fallbacks.p;
    }
    const dim3 grid_swap(pt ? pt->G : 1), block_swap(std::min(ENS_THREADS, std::max(64, (W + 63) / 64 * 64)));
    // one half-step with the wrapper that pt / moves choose.  A ladder's, with a sweep due after step s_dec: the swaps come between
    // the decisions and the row and proposals
    auto half = [&](int64_t s_dec, int h_dec, int64_t s_prop, int h_prop) {
        auto half_pt = [&](int what) { hipLaunchKernelGGL(k_ens_half_pt, grid, block, 0, st, D, M, Pt, s_dec, h_dec, s_prop, h_prop, what); };
        if (!pt && !moves) {
            hipLaunchKernelGGL(k_ens_half, grid, block, 0, st, D, s_dec, h_dec, s_prop, h_prop);
        } else if (cov) {
            hipLaunchKernelGGL(k_ens_half_cov, grid, block, 0, st, D, M, Cv, s_dec, h_dec, s_prop, h_prop);
        } else if (!pt) {
            hipLaunchKernelGGL(k_ens_half_moves, grid, block, 0, st, D, M, s_dec, h_dec, s_prop, h_prop);
        } else if (s_dec >= 0 && h_dec == 1 && pt->T > 1 && vmx_ens::swap_due(s_dec, pt->swap_every)) {
            half_pt(ENS_PT_DECIDE);
            if (ad)
                hipLaunchKernelGGL(k_ens_swap_adapt, grid_swap, block_swap, 0, st, D, Pt, Ad, s_dec,
                                   vmx_ens::adapt_due(s_dec, ad->adapt_until) ? 1 : 0);
            else
                hipLaunchKernelGGL(k_ens_swap, grid_swap, block_swap, 0, st, D, Pt, s_dec);
            half_pt(ENS_PT_RECORD | ENS_PT_PROPOSE);
        } else {
            half_pt(ENS_PT_DECIDE | ENS_PT_RECORD | ENS_PT_PROPOSE);
        }
    };
    if (halves > 0) half((int64_t)-1, 0, step0, 0);
    HIP_OK(hipGetLastError());
    for (int64_t q = 0; q < halves; ++q) {
        const int64_t s = step0 + q / 2;
        const int h = (int)(q % 2);
        const int calls = L.evaluate(S.box.theta.p, EH, S.box.chi2.p, S.box.status.p, d_mock, true);
        if (calls < 0) return -2;
        R.engine_calls += calls;
        const int64_t nq = q + 1;
        const int64_t s_next = nq < halves ? step0 + nq / 2 : (int64_t)-1;
        half(s, h, s_next, (int)(nq % 2));
        HIP_OK(hipGetLastError());
    }
    std::vector<int64_t> acc0(accepted, accepted + EW), box(EW), failed(EW);
    if (pt && pt->swaps && n_swaps) {
        if (halves > 0) HIP_OK(hipMemcpyAsync(pt->swaps, S.swaps.p, n_swaps * sizeof(int64_t), hipMemcpyDeviceToHost, st));
        else std::fill(pt->swaps, pt->swaps + n_swaps, (int64_t)0);
    }
    if (ad && halves > 0) {
        HIP_OK(hipMemcpyAsync(pt->betas_out, S.beta.p, n_beta * sizeof(double), hipMemcpyDeviceToHost, st));
        if (n_hist) HIP_OK(hipMemcpyAsync(pt->beta_hist, S.beta_hist.p, n_hist * sizeof(double), hipMemcpyDeviceToHost, st));
        if (pt->adapt_skipped)
            HIP_OK(hipMemcpyAsync(pt->adapt_skipped, S.adapt_skipped.p, (size_t)pt->G * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    } else if (ad && pt->adapt_skipped) {
        std::fill(pt->adapt_skipped, pt->adapt_skipped + pt->G, (int64_t)0);
    }
    if (cov && fallbacks) HIP_OK(hipMemcpyAsync(fallbacks, S.cov_fallbacks.p, (size_t)E * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    HIP_OK(hipMemcpyAsync(x, S.x.p, EW * n * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_OK(hipMemcpyAsync(lnL, S.lnl.p, EW * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_OK(hipMemcpyAsync(accepted, S.acc.p, EW * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    HIP_OK(hipMemcpyAsync(box.data(), S.n_box.p, EW * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    HIP_OK(hipMemcpyAsync(failed.data(), S.n_fail.p, EW * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    if (chain_store_take(store, S.chain.p, S.chain_lnl.p, rows, st)) return -2;
    if (chain && rows > 0) HIP_OK(hipMemcpyAsync(chain, S.chain.p, (size_t)rows * EW * n * sizeof(double), hipMemcpyDeviceToHost, st));
    if (chain_lnL && rows > 0) HIP_OK(hipMemcpyAsync(chain_lnL, S.chain_lnl.p, (size_t)rows * EW * sizeof(double), hipMemcpyDeviceToHost, st));
    R.seconds_enqueuing = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_loop).count();
    HIP_OK(hipStreamSynchronize(st));       // (the call's only wait: the segment is enqueued as a whole)
    if (store) store->rows += rows;
    R.host_synchronisations = 1;
    R.steps = n_steps;
    R.proposals = (int64_t)n_steps * (int64_t)EW;
    for (int q = 0; q < E; ++q) {
        int64_t took = 0, out = 0, bad = 0;
        for (size_t w = (size_t)q * W; w < (size_t)(q + 1) * W; ++w) {
            took += accepted[w] - acc0[w];
            out += box[w];
            bad += failed[w];
        }
        if (per_ensemble) { per_ensemble[3 * q] = took; per_ensemble[3 * q + 1] = out; per_ensemble[3 * q + 2] = bad; }
        R.accepted += took;
        R.rejected_outside_box += out;
        R.rejected_failed_model += bad;
    }
    R.seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_begin).count();
    if (stats) *stats = R;
    return 0;
}

// Ensemble slice sampling (vmx_ensemble.h, the fifth part): E ensembles in rounds.  A round is k_ens_slice_advance - answers,
// machines, and whatever of commit, tuning, chain row and the next half's opening an ensemble without requests is due -
// k_ens_slice_emit - the rows of all ensembles behind each other - one wait for the mapped total, and the engine's chain over
// those rows; the host has waited, so no event guards the rows.  An ensemble that asks for nothing has done its steps and leaves
// the list.  host_synchronisations = rounds + 1: the last wait brings the state back.
static_assert(VMX_SLICE_COUNTS == vmx_ens::SLICE_COUNTS && vmx_ens::SLICE_COUNTS == 8 && VMX_SLICE_MAX_EXPANSIONS == vmx_ens::SLICE_MAX_EXPANSIONS &&
              VMX_SLICE_MAX_CONTRACTIONS == vmx_ens::SLICE_MAX_CONTRACTIONS, "slice sampling limits");
int vmx_ensemble_run_slice(vmx_engine* e, const vmx_ensemble_spec* spec, int32_t E, int32_t W, const uint64_t* streams,
                           const int32_t* mock_row, double* x, double* lnL, int64_t* accepted, int64_t step0, int32_t n_steps,
                           int32_t thin, double* chain, double* chain_lnL, const vmx_ensemble_options* opt, vmx_ensemble_stats* stats,
                           const vmx_ensemble_slice* slice, double* mu, int64_t* slice_counts)
{
    const std::string name("vmx_ensemble_run_slice");
    std::vector<char> varies;
    std::vector<int32_t> inv;
    if (ensemble_check(name, e, spec, E, W, streams, mock_row, x, lnL, accepted, step0, n_steps, thin, opt, false, varies, inv)) return -1;
    REQUIRE(slice && mu, name + ": the slice settings and the scales mu [E]");
    REQUIRE(W >= 4, name + ": two partners in the other half, W >= 4");
    REQUIRE(vmx_ens::slice_ok(W / 2, slice->mu0, slice->tune_steps, slice->max_expansions, slice->max_contractions, slice->flags),
            name + ": mu0 positive and finite, tune_steps >= 0, 1 <= max_expansions <= 32, 1 <= max_contractions <= 64, flags 0");
    for (int q = 0; q < E; ++q) REQUIRE(std::isfinite(mu[q]) && mu[q] > 0.0, name + ": every scale mu must be positive and finite");
    const int n = spec->n, P = e->n_params, H = W / 2;
    const int64_t rows = (step0 + n_steps) / thin - step0 / thin;
    const size_t EW = (size_t)E * W, EH = (size_t)E * H;
    vmx_chain_store* const store = e->chain_store;          // (as in ensemble_run)
    if (chain_store_check(name, store, E, W, n, rows)) return -1;
    const bool keep_x = chain || store, keep_lnl = chain_lnL || store;

    HIP_OK(hipSetDevice(e->device));
    const auto t_begin = std::chrono::steady_clock::now();
    if (!e->ensws) e->ensws = new EnsWorkspace();
    EnsWorkspace& S = *e->ensws;
    if (ensure(S.x, EW * n) || ensure(S.lnl, EW) || ensure(S.acc, EW) || ensure(S.col, n) || ensure(S.streams, E) ||
        ensure(S.sl_wk, EH) || ensure(S.sl_eta, EH * n) || ensure(S.sl_slot, EH) || ensure(S.sl_row, EH) || ensure(S.sl_mu, E) ||
        ensure(S.sl_counts, (size_t)E * vmx_ens::SLICE_COUNTS) || ensure(S.sl_step, (size_t)E * 2) || ensure(S.sl_q, E) ||
        ensure(S.sl_open, E) || ensure(S.sl_active, E) || ensure(S.sl_count, E) ||
        (mock_row && (ensure(S.sl_mock_row, E) || ensure(S.mock, EH))))
        return -2;
    if (keep_x && rows > 0 && ensure(S.chain, (size_t)rows * EW * n)) return -2;
    if (keep_lnl && rows > 0 && ensure(S.chain_lnl, (size_t)rows * EW)) return -2;
    if (!S.pin_word) {
        HIP_OK(hipHostMalloc((void**)&S.pin_word, 16 * sizeof(int32_t), hipHostMallocMapped));
        HIP_OK(hipHostGetDevicePointer((void**)&S.dpin_word, S.pin_word, 0));
    }
    if (S.pin_runs < (size_t)E) {
        if (S.pin_count) { (void)hipHostFree(S.pin_count); S.pin_count = nullptr; }
        if (S.pin_active) { (void)hipHostFree(S.pin_active); S.pin_active = nullptr; }
        S.pin_runs = 0;
        HIP_OK(hipHostMalloc((void**)&S.pin_count, (size_t)E * sizeof(int32_t), hipHostMallocMapped));
        HIP_OK(hipHostGetDevicePointer((void**)&S.dpin_count, S.pin_count, 0));
        HIP_OK(hipHostMalloc((void**)&S.pin_active, (size_t)E * sizeof(int32_t), hipHostMallocDefault));
        S.pin_runs = (size_t)E;
    }
    hipStream_t st = e->stream;
    EnsDev D{};
    if (S.box.upload(EH, P, n, spec->theta_fixed, spec->lo, spec->hi, inv, st, D.box)) return -2;
    HIP_OK(hipMemcpyAsync(S.x.p, x, EW * n * sizeof(double), hipMemcpyHostToDevice, st));
    HIP_OK(hipMemcpyAsync(S.lnl.p, lnL, EW * sizeof(double), hipMemcpyHostToDevice, st));
    HIP_OK(hipMemcpyAsync(S.acc.p, accepted, EW * sizeof(int64_t), hipMemcpyHostToDevice, st));
    HIP_OK(hipMemcpyAsync(S.col.p, spec->col, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, st));
    HIP_OK(hipMemcpyAsync(S.streams.p, streams, (size_t)E * sizeof(uint64_t), hipMemcpyHostToDevice, st));
    HIP_OK(hipMemcpyAsync(S.sl_mu.p, mu, (size_t)E * sizeof(double), hipMemcpyHostToDevice, st));
    if (mock_row) HIP_OK(hipMemcpyAsync(S.sl_mock_row.p, mock_row, (size_t)E * sizeof(int32_t), hipMemcpyHostToDevice, st));
    HIP_OK(hipMemsetAsync(S.sl_counts.p, 0, (size_t)E * vmx_ens::SLICE_COUNTS * sizeof(int64_t), st));
    HIP_OK(hipMemsetAsync(S.sl_step.p, 0, (size_t)E * 2 * sizeof(int64_t), st));
    HIP_OK(hipMemsetAsync(S.sl_q.p, 0, (size_t)E * sizeof(int64_t), st));
    HIP_OK(hipMemsetAsync(S.sl_open.p, 0, (size_t)E * sizeof(int32_t), st));
    const int32_t* d_mock = mock_row ? S.mock.p : nullptr;

    D.x = S.x.p; D.lnl = S.lnl.p; D.acc = S.acc.p;
    D.col = S.col.p;
    D.chain = keep_x && rows > 0 ? S.chain.p : nullptr; D.chain_lnl = keep_lnl && rows > 0 ? S.chain_lnl.p : nullptr;
    D.streams = S.streams.p; D.rows = rows;
    D.W = W; D.n = n; D.P = P; D.thin = thin; D.a = 0.0; D.log_norm = spec->log_norm;
    D.seed = spec->seed; D.step0 = step0;
    EnsSliceDev X{};
    X.wk = S.sl_wk.p; X.eta = S.sl_eta.p; X.slot = S.sl_slot.p; X.row_walker = S.sl_row.p; X.mu = S.sl_mu.p;
    X.counts = S.sl_counts.p; X.step_counts = S.sl_step.p; X.q = S.sl_q.p; X.open = S.sl_open.p;
    X.active = S.sl_active.p; X.count = S.sl_count.p; X.host_count = S.dpin_count; X.host_word = S.dpin_word;
    X.mock_row = mock_row ? S.sl_mock_row.p : nullptr; X.mock = mock_row ? S.mock.p : nullptr;
    X.n_steps = n_steps; X.tune_steps = slice->tune_steps; X.max_e = slice->max_expansions; X.max_c = slice->max_contractions;

    // the engine as the sampler's likelihood, at the table level the sampled columns allow
    LikelihoodSession L(e, opt ? opt->const_hint : -1, opt ? opt->chunk : 0, opt ? opt->lanes : 0, e->max_batch, varies);
    vmx_ensemble_stats R{};
    R.const_hint = L.hint;
    R.lanes = L.lanes;
    double enqueue_s = 0.0;
    // (every loop of the kernels strides by its block: the chain does not depend on this size)
    const dim3 block(std::min(ENS_THREADS, std::max(64, (H + 63) / 64 * 64)));
    int32_t* const active = S.pin_active;
    for (int q = 0; q < E; ++q) active[q] = q;
    int A = n_steps > 0 ? E : 0;
    int64_t rounds = 0, rows_asked = 0;
    while (A > 0) {
        const auto t0 = std::chrono::steady_clock::now();
        // (the list goes up on the stream: the host changes it only after it has waited for the stream)
        X.A = A;
        HIP_OK(hipMemcpyAsync(S.sl_active.p, active, (size_t)A * sizeof(int32_t), hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(k_ens_slice_advance, dim3(A), block, 0, st, D, X);
        hipLaunchKernelGGL(k_ens_slice_emit, dim3(A), block, 0, st, D, X);
        HIP_OK(hipGetLastError());
        enqueue_s += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        HIP_OK(hipStreamSynchronize(st));       // (the round's only wait: the total and the ensembles' counts, mapped words)
        rounds += 1;
        const int total = S.pin_word[0];
        if (total < 0 || (size_t)total > EH) return fail(-2, name + ": a round asked for more rows than its buffers hold");
        if (total > 0) {
            const auto t1 = std::chrono::steady_clock::now();
            const int calls = L.evaluate(S.box.theta.p, total, S.box.chi2.p, S.box.status.p, d_mock, false);
            if (calls < 0) return -2;
            R.engine_calls += calls;
            rows_asked += total;
            enqueue_s += std::chrono::duration<double>(std::chrono::steady_clock::now() - t1).count();
        }
        A = vmx_ens::slice_compact(active, A, S.pin_count);
    }
    std::vector<int64_t> counts((size_t)E * vmx_ens::SLICE_COUNTS, 0);
    HIP_OK(hipMemcpyAsync(x, S.x.p, EW * n * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_OK(hipMemcpyAsync(lnL, S.lnl.p, EW * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_OK(hipMemcpyAsync(accepted, S.acc.p, EW * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    HIP_OK(hipMemcpyAsync(mu, S.sl_mu.p, (size_t)E * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_OK(hipMemcpyAsync(counts.data(), S.sl_counts.p, counts.size() * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    if (chain_store_take(store, S.chain.p, S.chain_lnl.p, rows, st)) return -2;
    if (chain && rows > 0) HIP_OK(hipMemcpyAsync(chain, S.chain.p, (size_t)rows * EW * n * sizeof(double), hipMemcpyDeviceToHost, st));
    if (chain_lnL && rows > 0) HIP_OK(hipMemcpyAsync(chain_lnL, S.chain_lnl.p, (size_t)rows * EW * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    if (store) store->rows += rows;
    R.host_synchronisations = rounds + 1;
    R.steps = n_steps;
    int64_t rows_counted = 0;           // (the machines' own count of their requests: the rows the engine was given, no other)
    for (int q = 0; q < E; ++q) rows_counted += counts[(size_t)q * vmx_ens::SLICE_COUNTS + vmx_ens::SC_ROWS];
    if (rows_counted != rows_asked) return fail(-2, name + ": the engine's rows are not the walkers' requests");
    for (int q = 0; q < E; ++q) {
        const int64_t* c = counts.data() + (size_t)q * vmx_ens::SLICE_COUNTS;
        if (slice_counts) std::memcpy(slice_counts + (size_t)q * vmx_ens::SLICE_COUNTS, c, vmx_ens::SLICE_COUNTS * sizeof(int64_t));
        R.proposals += c[vmx_ens::SC_UPDATES];
        R.accepted += c[vmx_ens::SC_MOVED];
    }
    R.seconds_enqueuing = enqueue_s;
    R.seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_begin).count();
    if (stats) *stats = R;
    return 0;
}

// ---- the chain where it is recorded (vmx_chain.h): the store, and its summary
static_assert(vmx_chain::MAXW * (int)sizeof(double) + vmx_chain::TILE * (int)sizeof(double) <= 48 * 1024, "the summary's LDS");

namespace {

constexpr int CHAIN_THREADS = 256;

// What the three kernels of the summary read: the store's rows [first, first + T) of every ensemble and the scratch
struct ChainDev {
    const double* x;                    // [E][capacity][W][n]
    double* sums;                       // [2][E][W][n]: the series sums, then the series' own means
    double* centred;                    // [E][n][T][W]
    double* mean; double* cov;          // [E][n], [E][n][n] (cov nullptr: not wanted)
    double* tau; int64_t* window;       // [E][n] each
    int64_t capacity, first, T;
    int32_t E, W, n;
    double c;
};

// pair p of the lower triangle, rows first: (0,0) (1,0) (1,1) (2,0) ...
__device__ inline void chain_pair(int p, int& i, int& j)
{
    i = 0;
    while ((i + 1) * (i + 2) / 2 <= p) ++i;
    j = p - i * (i + 1) / 2;
}

// One work-group per ensemble: the series sums and means (a lane per (walker, column), sequential in t), the mean (a lane per
// column, sequential in w), then the covariance in chunks of pairs that fill the tile: a lane per (pair, walker), sequential in t,
// then a lane per pair, sequential in w.  Every loop strides by the block: no sum depends on its size.
__global__ __launch_bounds__(CHAIN_THREADS) void k_chain_moments(ChainDev C)
{
    __shared__ double tile[vmx_chain::TILE];
    const int e = blockIdx.x, W = C.W, n = C.n;
    const int64_t Wn = (int64_t)W * n, T = C.T, count = T * W;
    const double* x = C.x + ((int64_t)e * C.capacity + C.first) * Wn;
    double* S = C.sums + (int64_t)e * Wn;
    double* m = C.sums + ((int64_t)C.E + e) * Wn;
    for (int64_t q = threadIdx.x; q < Wn; q += blockDim.x) {
        const double s = vmx_chain::seq_sum(x + q, T, Wn);
        S[q] = s;
        m[q] = vmx_chain::quotient(s, T);
    }
    __syncthreads();
    double* mean = C.mean + (int64_t)e * n;
    for (int d = threadIdx.x; d < n; d += blockDim.x) mean[d] = vmx_chain::quotient(vmx_chain::seq_sum(S + d, W, n), count);
    __syncthreads();
    if (!C.cov) return;
    double* cov = C.cov + (int64_t)e * n * n;
    const int pairs = n * (n + 1) / 2, chunk = vmx_chain::per_tile(W, pairs);
    for (int p0 = 0; p0 < pairs; p0 += chunk) {
        const int pc = min(chunk, pairs - p0);
        for (int q = threadIdx.x; q < pc * W; q += blockDim.x) {
            const int k = q / W, w = q % W;
            int i, j;
            chain_pair(p0 + k, i, j);
            tile[q] = vmx_chain::product_sum(x + (int64_t)w * n + i, x + (int64_t)w * n + j, mean[i], mean[j], T, Wn);
        }
        __syncthreads();
        for (int k = threadIdx.x; k < pc; k += blockDim.x) {
            int i, j;
            chain_pair(p0 + k, i, j);
            const double v = vmx_chain::quotient(vmx_chain::seq_sum(tile + (int64_t)k * W, W, 1), count - 1);
            cov[i * n + j] = v;
            cov[j * n + i] = v;
        }
        __syncthreads();
    }
}

// The centred series, x[e][first + t][w][d] - m[e][w][d] -> centred[e][d][t][w]: W fastest, so that the lanes of k_chain_acf,
// (walker, lag), read contiguous rows instead of every n-th double of the chain
__global__ __launch_bounds__(CHAIN_THREADS) void k_chain_centre(ChainDev C)
{
    const int64_t Wn = (int64_t)C.W * C.n, per = C.T * Wn, total = (int64_t)C.E * per;
    const double* m = C.sums + (int64_t)C.E * Wn;
    for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < total; g += (int64_t)gridDim.x * blockDim.x) {
        const int64_t e = g / per, q = g % per, t = q / Wn, r = q % Wn;
        const int w = (int)(r / C.n), d = (int)(r % C.n);
        const double v = C.x[(e * C.capacity + C.first) * Wn + q];
        C.centred[((e * C.n + d) * C.T + t) * C.W + w] = vmx_chain::centred(v, m[e * Wn + r]);
    }
}

// One work-group per (ensemble, column): the lags in blocks of `lags`, a lane per (lag, walker) with w fastest and sequential in
// t, rho into the tile, then a lane per lag for f (sequential in w) and thread 0 walks the block's lags in order
// (vmx_chain::window_take); the group leaves at the block in which the window closes.  The series streams from L2: one
// parameter's is T W doubles, more than the LDS at the sizes that matter.
__global__ __launch_bounds__(CHAIN_THREADS) void k_chain_acf(ChainDev C)
{
    __shared__ double tile[vmx_chain::TILE];
    __shared__ double acov0[vmx_chain::MAXW];
    __shared__ double f[vmx_chain::LAG_BLOCK];
    __shared__ int closed;
    const int d = blockIdx.x % C.n, W = C.W;
    const int64_t e = blockIdx.x / C.n, T = C.T;
    const double* cen = C.centred + ((e * C.n + d) * T) * W;
    const int LB = vmx_chain::per_tile(W, vmx_chain::LAG_BLOCK);
    vmx_chain::Window win;              // (thread 0's is the one that walks)
    if (threadIdx.x == 0) closed = 0;
    for (int w = threadIdx.x; w < W; w += blockDim.x) acov0[w] = vmx_chain::lag_sum(cen + w, T, 0, W);
    __syncthreads();
    for (int64_t l0 = 0; l0 < T; l0 += LB) {
        const int lags = (int)min((int64_t)LB, T - l0);
        for (int q = threadIdx.x; q < lags * W; q += blockDim.x) {
            const int k = q / W, w = q % W;
            const int64_t l = l0 + k;
            const double a = l == 0 ? acov0[w] : vmx_chain::lag_sum(cen + w, T, l, W);
            tile[q] = vmx_chain::rho(a, acov0[w]);
        }
        __syncthreads();
        for (int k = threadIdx.x; k < lags; k += blockDim.x) f[k] = vmx_chain::quotient(vmx_chain::seq_sum(tile + (int64_t)k * W, W, 1), W);
        __syncthreads();
        if (threadIdx.x == 0)
            for (int k = 0; k < lags; ++k)
                if (vmx_chain::window_take(win, f[k], T, C.c)) {
                    C.tau[e * C.n + d] = win.tau;
                    C.window[e * C.n + d] = win.window;
                    closed = 1;
                    break;
                }
        __syncthreads();
        if (closed) return;
    }
}

// ---- order statistics and the best row of the store's rows (vmx_chain_select.h)
static_assert(VMX_CHAIN_MAX_RANKS == vmx_select::MAX_RANKS, "ranks of an order-statistics call");
static_assert(vmx_select::MAX_RANKS <= CHAIN_THREADS && vmx_select::MAX_RANKS * vmx_select::BINS * (int)sizeof(uint32_t) <= 32 * 1024,
              "the select's histograms");

struct SelectDev {
    const double* x; const double* lnl; // [E][capacity][W][n], [E][capacity][W]
    uint64_t* keys;                     // [E][n][T W]: the keys of a column, contiguous
    uint64_t* values;                   // [E][n][U]: the bits of the order statistics
    double* best_lnl; double* best_x;   // [E], [E][n] (best_x nullptr: not wanted)
    int64_t* best_index;                // [E]: row W + walker from row 0 of the store, -1 for none
    int64_t capacity, first, T;
    int32_t E, W, n, U;
    uint32_t ranks[vmx_select::MAX_RANKS];      // the U ranks asked, ascending and distinct
};

// The keys of the rows from `first` on, x[e][first + t][w][d] -> keys[e][d][t][w]: the twin of k_chain_centre, so that a
// work-group of k_chain_select streams one contiguous column
__global__ __launch_bounds__(CHAIN_THREADS) void k_chain_keys(SelectDev C)
{
    const int64_t Wn = (int64_t)C.W * C.n, per = C.T * Wn, total = (int64_t)C.E * per;
    for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < total; g += (int64_t)gridDim.x * blockDim.x) {
        const int64_t e = g / per, q = g % per, t = q / Wn, r = q % Wn;
        const int w = (int)(r / C.n), d = (int)(r % C.n);
        C.keys[((e * C.n + d) * C.T + t) * C.W + w] = vmx_select::key(C.x[(e * C.capacity + C.first) * Wn + q]);
    }
}

// One work-group per (ensemble, column): eight passes of 8-bit digits, most significant first.  A pass counts the next digit of
// every key whose leading bits are a prefix still alive among the ranks, one 256-bin histogram in LDS per distinct prefix (integer
// atomics: the counts do not depend on their order; a wave whose keys all fall into one bin adds its count once), then a lane per
// rank walks its histogram to the next digit and lane 0 regroups the prefixes.  The keys stream from L2 eight times.
__global__ __launch_bounds__(CHAIN_THREADS) void k_chain_select(SelectDev C)
{
    using namespace vmx_select;
    __shared__ uint32_t hist[MAX_RANKS * BINS];
    __shared__ uint64_t prefix[MAX_RANKS], group_prefix[MAX_RANKS];
    __shared__ uint32_t left[MAX_RANKS];
    __shared__ int group[MAX_RANKS];
    __shared__ int groups;
    const int tid = threadIdx.x, lane = tid & 63, U = C.U;
    const int64_t N = C.T * C.W;
    const uint64_t* keys = C.keys + (int64_t)blockIdx.x * N;
    if (tid < U) { prefix[tid] = 0; left[tid] = C.ranks[tid]; }
    __syncthreads();
    if (tid == 0) groups = regroup(prefix, U, group, group_prefix);
    __syncthreads();
    for (int p = 0; p < PASSES; ++p) {
        const int G = groups;
        for (int q = tid; q < G * BINS; q += blockDim.x) hist[q] = 0;
        __syncthreads();
        for (int64_t base = 0; base < N; base += blockDim.x) {          // (every lane of a wave takes every turn: the ballots below)
            const int64_t i = base + tid;
            int slot = -1;
            if (i < N) {
                const uint64_t k = keys[i];
                const int at = find_group(group_prefix, G, leading(k, p));
                if (at >= 0) slot = at * BINS + digit(k, p);
            }
            const unsigned long long active = __ballot(slot >= 0);
            if (active) {
                const int leader = __ffsll(active) - 1;
                const int slot0 = __shfl(slot, leader);
                const unsigned long long same = __ballot(slot == slot0);
                if (same == active) {
                    if (lane == leader) atomicAdd(&hist[slot0], (uint32_t)__popcll(same));
                } else if (slot >= 0) {
                    atomicAdd(&hist[slot], 1u);
                }
            }
        }
        __syncthreads();
        if (tid < U) prefix[tid] = (prefix[tid] << 8) | (uint64_t)walk(hist + group[tid] * BINS, left[tid]);
        __syncthreads();
        if (tid == 0) groups = regroup(prefix, U, group, group_prefix);
        __syncthreads();
    }
    if (tid < U) C.values[(int64_t)blockIdx.x * U + tid] = unkey(prefix[tid]);
}

// One work-group per ensemble: the lanes stride over (row, walker) of lnl[e] from `first` on and keep their best candidate, an LDS
// tree reduces them with vmx_select::wins (associative and commutative: the tree's shape does not matter), then the group copies
// the winning position row
__global__ __launch_bounds__(CHAIN_THREADS) void k_chain_best(SelectDev C)
{
    using namespace vmx_select;
    __shared__ double value[CHAIN_THREADS];
    __shared__ int64_t index[CHAIN_THREADS];
    const int tid = threadIdx.x, e = blockIdx.x, W = C.W, n = C.n;
    const double* lnl = C.lnl + (int64_t)e * C.capacity * W;
    double best = 0.0;
    int64_t at = -1;
    for (int64_t q = C.first * W + tid; q < (C.first + C.T) * W; q += CHAIN_THREADS) {
        const double v = lnl[q];
        const int64_t i = v != v ? -1 : q;          // (vmx_select::candidate: a NaN is none)
        if (wins(v, i, best, at)) { best = v; at = i; }
    }
    value[tid] = best;
    index[tid] = at;
    __syncthreads();
    for (int s = CHAIN_THREADS / 2; s > 0; s >>= 1) {
        if (tid < s && wins(value[tid + s], index[tid + s], value[tid], index[tid])) {
            value[tid] = value[tid + s];
            index[tid] = index[tid + s];
        }
        __syncthreads();
    }
    const int64_t won = index[0];
    if (tid == 0) {
        C.best_index[e] = won;
        C.best_lnl[e] = won < 0 ? double_of(CANONICAL_NAN) : value[0];
    }
    if (C.best_x)
        for (int d = tid; d < n; d += CHAIN_THREADS)
            C.best_x[(int64_t)e * n + d] = won < 0 ? double_of(CANONICAL_NAN) : C.x[((int64_t)e * C.capacity * W + won) * n + d];
}

// bytes of `rows` rows of every ensemble must fit size_t: E capacity W n doubles
static bool chain_fits(int64_t E, int64_t W, int64_t n, int64_t rows)
{
    const size_t per = (size_t)E * (size_t)W * (size_t)n * sizeof(double);        // (E <= 2^31, W <= 2^10, n <= 2^6: no overflow)
    return rows == 0 || (size_t)rows <= SIZE_MAX / per;
}

// rows of E blocks between two layouts [E][rows_a][per] and [E][rows_b][per]: one pitched copy
static hipError_t chain_copy(void* dst, int64_t dst_rows, const void* src, int64_t src_rows, int64_t rows, int64_t per, int E,
                             hipMemcpyKind kind, hipStream_t st)
{
    return hipMemcpy2DAsync(dst, (size_t)dst_rows * per * sizeof(double), src, (size_t)src_rows * per * sizeof(double),
                            (size_t)rows * per * sizeof(double), (size_t)E, kind, st);
}

// `count` entries in a fresh allocation (what `b` held is gone); a failure leaves the runtime without a pending error
static int chain_alloc(DevBuf<double>& b, size_t count)
{
    if (b.alloc(count, false)) { (void)hipGetLastError(); return -2; }
    return 0;
}

}  // namespace

int vmx_chain_store_create(vmx_engine* e, int32_t E, int32_t W, int32_t n, int64_t capacity_rows, vmx_chain_store** out)
{
    const std::string name("vmx_chain_store_create");
    REQUIRE(e && out, name);
    REQUIRE(E >= 1 && W >= 2 && W <= vmx_chain::MAXW && n >= 1 && n <= VMX_ENS_MAXN && capacity_rows >= 0,
            name + ": E >= 1, 2 <= W <= 1024, 1 <= n <= VMX_ENS_MAXN, capacity_rows >= 0");
    REQUIRE(chain_fits(E, W, n, capacity_rows), name + ": the store is too large");
    HIP_OK(hipSetDevice(e->device));
    vmx_chain_store* s = new vmx_chain_store();
    s->engine = e; s->E = E; s->W = W; s->n = n; s->capacity = capacity_rows;
    const size_t slots = (size_t)E * (size_t)capacity_rows * (size_t)W;
    if (chain_alloc(s->x, slots * n) || chain_alloc(s->lnl, slots)) { delete s; return -2; }
    e->chain_stores.push_back(s);
    *out = s;
    return 0;
}

int vmx_chain_store_destroy(vmx_chain_store* s)
{
    REQUIRE(s, "vmx_chain_store_destroy");
    vmx_engine* e = s->engine;
    (void)hipSetDevice(e->device);
    (void)hipStreamSynchronize(e->stream);
    if (e->chain_store == s) e->chain_store = nullptr;
    e->chain_stores.erase(std::remove(e->chain_stores.begin(), e->chain_stores.end(), s), e->chain_stores.end());
    delete s;
    return 0;
}

int vmx_chain_store_reserve(vmx_chain_store* s, int64_t capacity_rows)
{
    const std::string name("vmx_chain_store_reserve");
    REQUIRE(s && capacity_rows >= 0, name);
    if (capacity_rows <= s->capacity) return 0;
    REQUIRE(chain_fits(s->E, s->W, s->n, capacity_rows), name + ": the store is too large");
    vmx_engine* e = s->engine;
    HIP_OK(hipSetDevice(e->device));
    const size_t slots = (size_t)s->E * (size_t)capacity_rows * (size_t)s->W;
    DevBuf<double> x, lnl;
    if (chain_alloc(x, slots * s->n) || chain_alloc(lnl, slots)) return -2;
    if (s->rows > 0) {
        HIP_OK(chain_copy(x.p, capacity_rows, s->x.p, s->capacity, s->rows, (int64_t)s->W * s->n, s->E, hipMemcpyDeviceToDevice, e->stream));
        HIP_OK(chain_copy(lnl.p, capacity_rows, s->lnl.p, s->capacity, s->rows, s->W, s->E, hipMemcpyDeviceToDevice, e->stream));
    }
    HIP_OK(hipStreamSynchronize(e->stream));
    std::swap(s->x.p, x.p); std::swap(s->x.n, x.n);
    std::swap(s->lnl.p, lnl.p); std::swap(s->lnl.n, lnl.n);
    s->capacity = capacity_rows;
    return 0;
}

int vmx_chain_store_rows(vmx_chain_store* s, int64_t* rows)
{
    REQUIRE(s && rows, "vmx_chain_store_rows");
    *rows = s->rows;
    return 0;
}

int vmx_chain_store_append(vmx_chain_store* s, int64_t rows, const double* chain, const double* chain_lnl)
{
    const std::string name("vmx_chain_store_append");
    REQUIRE(s && rows >= 0 && (rows == 0 || (chain && chain_lnl)), name);
    REQUIRE(rows <= s->capacity - s->rows, name + ": rows beyond the store's capacity");
    if (rows == 0) return 0;
    vmx_engine* e = s->engine;
    HIP_OK(hipSetDevice(e->device));
    const int64_t Wn = (int64_t)s->W * s->n;
    HIP_OK(chain_copy(s->x.p + s->rows * Wn, s->capacity, chain, rows, rows, Wn, s->E, hipMemcpyHostToDevice, e->stream));
    HIP_OK(chain_copy(s->lnl.p + s->rows * s->W, s->capacity, chain_lnl, rows, rows, s->W, s->E, hipMemcpyHostToDevice, e->stream));
    HIP_OK(hipStreamSynchronize(e->stream));
    s->rows += rows;
    return 0;
}

int vmx_chain_store_fetch(vmx_chain_store* s, int64_t row0, int64_t rows, double* chain, double* chain_lnl)
{
    const std::string name("vmx_chain_store_fetch");
    REQUIRE(s && row0 >= 0 && rows >= 0, name);
    REQUIRE(row0 <= s->rows && rows <= s->rows - row0, name + ": row0 + rows beyond the rows stored");
    if (rows == 0 || (!chain && !chain_lnl)) return 0;
    vmx_engine* e = s->engine;
    HIP_OK(hipSetDevice(e->device));
    const int64_t Wn = (int64_t)s->W * s->n;
    if (chain) HIP_OK(chain_copy(chain, rows, s->x.p + row0 * Wn, s->capacity, rows, Wn, s->E, hipMemcpyDeviceToHost, e->stream));
    if (chain_lnl) HIP_OK(chain_copy(chain_lnl, rows, s->lnl.p + row0 * s->W, s->capacity, rows, s->W, s->E, hipMemcpyDeviceToHost, e->stream));
    HIP_OK(hipStreamSynchronize(e->stream));
    return 0;
}

int vmx_ensemble_set_chain_store(vmx_engine* e, vmx_chain_store* s)
{
    REQUIRE(e, "vmx_ensemble_set_chain_store");
    REQUIRE(!s || s->engine == e, "vmx_ensemble_set_chain_store: the store belongs to another engine");
    e->chain_store = s;
    return 0;
}

// What an ensemble run refuses of the attached store before anything runs
static int chain_store_check(const std::string& name, const vmx_chain_store* s, int32_t E, int32_t W, int32_t n, int64_t rows)
{
    if (!s) return 0;
    REQUIRE(s->E == E && s->W == W && s->n == n, name + ": the attached chain store has another (E, W, n)");
    REQUIRE(rows <= s->capacity - s->rows, name + ": the run's rows exceed the attached chain store's capacity");
    return 0;
}

// The call's block [E][rows][W][n] (and its lnL) behind the store's rows, on the stream behind the half-step kernels; the caller
// counts the rows in once the stream has been waited for
static int chain_store_take(vmx_chain_store* s, const double* chain, const double* chain_lnl, int64_t rows, hipStream_t st)
{
    if (!s || rows <= 0) return 0;
    const int64_t Wn = (int64_t)s->W * s->n;
    HIP_OK(chain_copy(s->x.p + s->rows * Wn, s->capacity, chain, rows, rows, Wn, s->E, hipMemcpyDeviceToDevice, st));
    HIP_OK(chain_copy(s->lnl.p + s->rows * s->W, s->capacity, chain_lnl, rows, rows, s->W, s->E, hipMemcpyDeviceToDevice, st));
    return 0;
}

int vmx_chain_store_summary(vmx_chain_store* s, int64_t first_row, double c, int64_t* count, double* mean, double* covariance,
                            double* tau, int64_t* window)
{
    const std::string name("vmx_chain_store_summary");
    REQUIRE(s, name);
    REQUIRE(first_row >= 0 && first_row < s->rows, name + ": first_row must be a stored row (the summary needs at least one)");
    REQUIRE(c > 0.0 && std::isfinite(c), name + ": c must be positive and finite");
    vmx_engine* e = s->engine;
    HIP_OK(hipSetDevice(e->device));
    const int E = s->E, W = s->W, n = s->n;
    const int64_t T = s->rows - first_row, Wn = (int64_t)W * n;
    const bool acf = tau || window, second = mean || covariance;
    const size_t En = (size_t)E * n;
    if ((s->sums.n < 2 * (size_t)E * Wn && chain_alloc(s->sums, 2 * (size_t)E * Wn)) ||
        (s->out.n < En * (2 + n) && chain_alloc(s->out, En * (2 + n))) || (s->window.n < En && s->window.alloc(En, false) && ((void)hipGetLastError(), true)) ||
        (acf && s->centred.n < En * (size_t)T * W && chain_alloc(s->centred, En * (size_t)T * W)))
        return -2;
    ChainDev C{};
    C.x = s->x.p; C.sums = s->sums.p; C.centred = s->centred.p;
    C.mean = s->out.p; C.cov = second ? s->out.p + En : nullptr; C.tau = s->out.p + En * (1 + n); C.window = s->window.p;
    C.capacity = s->capacity; C.first = first_row; C.T = T; C.E = E; C.W = W; C.n = n; C.c = c;
    hipStream_t st = e->stream;
    hipLaunchKernelGGL(k_chain_moments, dim3(E), dim3(CHAIN_THREADS), 0, st, C);
    if (acf) {
        const int64_t total = (int64_t)E * T * Wn;
        const int blocks = (int)std::min<int64_t>((total + CHAIN_THREADS - 1) / CHAIN_THREADS, 65536);
        hipLaunchKernelGGL(k_chain_centre, dim3(blocks), dim3(CHAIN_THREADS), 0, st, C);
        hipLaunchKernelGGL(k_chain_acf, dim3((unsigned)En), dim3(CHAIN_THREADS), 0, st, C);
    }
    HIP_OK(hipGetLastError());
    if (mean) HIP_OK(hipMemcpyAsync(mean, C.mean, En * sizeof(double), hipMemcpyDeviceToHost, st));
    if (covariance) HIP_OK(hipMemcpyAsync(covariance, C.cov, En * n * sizeof(double), hipMemcpyDeviceToHost, st));
    if (tau) HIP_OK(hipMemcpyAsync(tau, C.tau, En * sizeof(double), hipMemcpyDeviceToHost, st));
    if (window) HIP_OK(hipMemcpyAsync(window, C.window, En * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    if (count) std::fill(count, count + E, T * W);
    return 0;
}

// Scratch of the select through the helpers of the summary's: a fresh allocation when the buffer is too small, and under
// vmx_debug_poison_scratch the fill of a buffer kept from an earlier, larger call too
static int chain_scratch(DevBuf<double>& b, size_t count)
{
    if (b.p && b.n >= count) return poison_fill(b.p, b.n) ? -2 : 0;
    return chain_alloc(b, count);
}

int vmx_chain_store_order_stats(vmx_chain_store* s, int64_t first_row, int32_t n_ranks, const int64_t* ranks, double* values)
{
    const std::string name("vmx_chain_store_order_stats");
    REQUIRE(s && ranks && values, name + ": a store, ranks and values");
    REQUIRE(first_row >= 0 && first_row < s->rows, name + ": first_row must be a stored row");
    REQUIRE(n_ranks >= 1 && n_ranks <= VMX_CHAIN_MAX_RANKS, name + ": 1 <= n_ranks <= VMX_CHAIN_MAX_RANKS");
    const int E = s->E, W = s->W, n = s->n;
    const int64_t T = s->rows - first_row, N = T * W;
    REQUIRE(vmx_select::count_fits(T, W), name + ": (rows - first_row) W must stay below 2^31");
    for (int r = 0; r < n_ranks; ++r) REQUIRE(ranks[r] >= 0 && ranks[r] < N, name + ": a rank outside [0, (rows - first_row) W)");
    int64_t sorted[vmx_select::MAX_RANKS];
    const int U = vmx_select::distinct_ranks(ranks, n_ranks, sorted);
    vmx_engine* e = s->engine;
    HIP_OK(hipSetDevice(e->device));
    const size_t En = (size_t)E * n;
    if (chain_scratch(s->sel_keys, En * (size_t)N) || chain_scratch(s->sel_out, En * (size_t)U)) return -2;
    SelectDev C{};
    C.x = s->x.p; C.lnl = s->lnl.p;
    C.keys = reinterpret_cast<uint64_t*>(s->sel_keys.p); C.values = reinterpret_cast<uint64_t*>(s->sel_out.p);
    C.capacity = s->capacity; C.first = first_row; C.T = T; C.E = E; C.W = W; C.n = n; C.U = U;
    for (int r = 0; r < U; ++r) C.ranks[r] = (uint32_t)sorted[r];
    hipStream_t st = e->stream;
    const int64_t total = (int64_t)En * N;
    const int blocks = (int)std::min<int64_t>((total + CHAIN_THREADS - 1) / CHAIN_THREADS, 65536);
    hipLaunchKernelGGL(k_chain_keys, dim3(blocks), dim3(CHAIN_THREADS), 0, st, C);
    hipLaunchKernelGGL(k_chain_select, dim3((unsigned)En), dim3(CHAIN_THREADS), 0, st, C);
    HIP_OK(hipGetLastError());
    std::vector<double> found(En * (size_t)U);
    HIP_OK(hipMemcpyAsync(found.data(), s->sel_out.p, found.size() * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    // the caller's order and repeats (bytes are copied: a value's bits stay its own)
    int at[vmx_select::MAX_RANKS];
    for (int r = 0; r < n_ranks; ++r) at[r] = (int)(std::lower_bound(sorted, sorted + U, ranks[r]) - sorted);
    for (size_t q = 0; q < En; ++q)
        for (int r = 0; r < n_ranks; ++r) std::memcpy(values + q * n_ranks + r, found.data() + q * U + at[r], sizeof(double));
    return 0;
}

int vmx_chain_store_best(vmx_chain_store* s, int64_t first_row, double* lnl_max, int64_t* row, int32_t* walker, double* position)
{
    const std::string name("vmx_chain_store_best");
    REQUIRE(s && lnl_max && row && walker, name + ": a store, lnl_max, row and walker");
    REQUIRE(first_row >= 0 && first_row < s->rows, name + ": first_row must be a stored row");
    vmx_engine* e = s->engine;
    HIP_OK(hipSetDevice(e->device));
    const int E = s->E, W = s->W, n = s->n;
    const size_t En = (size_t)E * n;
    if (chain_scratch(s->sel_out, (size_t)E + En) ||
        (s->sel_index.n < (size_t)E && s->sel_index.alloc((size_t)E, false) && ((void)hipGetLastError(), true)))
        return -2;
    SelectDev C{};
    C.x = s->x.p; C.lnl = s->lnl.p;
    C.best_lnl = s->sel_out.p; C.best_x = position ? s->sel_out.p + E : nullptr; C.best_index = s->sel_index.p;
    C.capacity = s->capacity; C.first = first_row; C.T = s->rows - first_row; C.E = E; C.W = W; C.n = n;
    hipStream_t st = e->stream;
    hipLaunchKernelGGL(k_chain_best, dim3(E), dim3(CHAIN_THREADS), 0, st, C);
    HIP_OK(hipGetLastError());
    std::vector<int64_t> index((size_t)E);
    HIP_OK(hipMemcpyAsync(lnl_max, C.best_lnl, (size_t)E * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_OK(hipMemcpyAsync(index.data(), C.best_index, (size_t)E * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    if (position) HIP_OK(hipMemcpyAsync(position, C.best_x, En * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    for (int k = 0; k < E; ++k) {
        row[k] = index[k] < 0 ? -1 : index[k] / W;
        walker[k] = index[k] < 0 ? -1 : (int32_t)(index[k] % W);
    }
    return 0;
}

// ---- weighted, ragged sample sets (vmx_chain_weighted.h): the store, its summary, order statistics and best point
static_assert(VMX_SAMPLE_MAX_TARGETS == vmx_wchain::MAX_TARGETS, "targets of an order-statistics call");
static_assert(vmx_wchain::MAX_TARGETS <= CHAIN_THREADS && vmx_wchain::MAX_TARGETS * vmx_select::BINS * (int)sizeof(uint64_t) <= 32 * 1024,
              "the weighted select's histograms");

namespace {

constexpr int WCHAIN_TILE = 4096;       // doubles of LDS for a tree's terms: sets of up to 8192 rows never leave it
constexpr int WCHAIN_STATS = 4;         // w_max, S, s2, M in front of a set's mean and covariance

struct WchainDev {
    const double* x; const double* lnl; const double* w;    // [E][capacity][n], [E][capacity], [E][capacity]
    const int64_t* counts;              // [E]
    uint64_t* m;                        // [E][capacity]: the integer weights
    double* tree;                       // [E][half]: the terms of a tree too long for the LDS
    double* stats;                      // [E][WCHAIN_STATS + n + n n]
    uint64_t* keys;                     // [E][n][capacity]: the keys of a column, contiguous
    const uint64_t* targets;            // [E][U]: non-decreasing per set
    uint64_t* values;                   // [E][n][U]: the bits of the order statistics
    double* best_lnl; double* best_x;   // [E], [E][n] (best_x nullptr: not wanted)
    int64_t* best_index;                // [E]: -1 for none
    int64_t capacity, half;
    int32_t E, n, U;
};

__device__ inline int64_t wchain_stride(int n) { return WCHAIN_STATS + n + (int64_t)n * n; }

// The stride-halving tree (vmx_chain_weighted.h) of term(0) ... term(count - 1), count >= 1, by the whole work-group: the first
// level is formed from the terms themselves, the others in place in buf [padded(count) / 2].  Every thread gets the sum; the
// loops stride by the block, so no sum depends on its size.
extern "C++" template <class F>         // (this stretch of the file has C linkage)
__device__ inline double wchain_tree(F term, int64_t count, double* buf)
{
    const int64_t h = vmx_wchain::padded(count) / 2;
    for (int64_t i = threadIdx.x; i < h; i += blockDim.x) {
        const double a = i < count ? term(i) : 0.0, b = i + h < count ? term(i + h) : 0.0;
        buf[i] = vmx_wchain::add(a, b);
    }
    __syncthreads();
    for (int64_t s = h / 2; s >= 1; s /= 2) {
        for (int64_t i = threadIdx.x; i < s; i += blockDim.x) buf[i] = vmx_wchain::add(buf[i], buf[i + s]);
        __syncthreads();
    }
    const double r = buf[0];
    __syncthreads();
    return r;
}

// One work-group per set: w_max (any order), S and s2 (trees), the integer weights and their sum M (an integer sum: LDS atomics)
__global__ __launch_bounds__(CHAIN_THREADS) void k_wchain_scale(WchainDev C)
{
    __shared__ double tile[WCHAIN_TILE];
    __shared__ double top[CHAIN_THREADS];
    __shared__ unsigned long long total;
    const int tid = threadIdx.x, e = blockIdx.x;
    const int64_t count = C.counts[e];
    const double* w = C.w + (int64_t)e * C.capacity;
    double* st = C.stats + (int64_t)e * wchain_stride(C.n);
    if (count < 1) {
        if (tid == 0) {
            st[0] = 0.0; st[1] = 0.0; st[2] = vmx_wchain::canonical_nan();
            reinterpret_cast<uint64_t*>(st)[3] = 0;
        }
        return;
    }
    double mine = 0.0;
    for (int64_t i = tid; i < count; i += CHAIN_THREADS) mine = vmx_wchain::larger(mine, w[i]);
    top[tid] = mine;
    if (tid == 0) total = 0;
    __syncthreads();
    for (int s = CHAIN_THREADS / 2; s > 0; s >>= 1) {
        if (tid < s) top[tid] = vmx_wchain::larger(top[tid], top[tid + s]);
        __syncthreads();
    }
    const double w_max = top[0];
    double* buf = vmx_wchain::padded(count) / 2 <= WCHAIN_TILE ? tile : C.tree + (int64_t)e * C.half;
    const double S = wchain_tree([=](int64_t i) { return w[i]; }, count, buf);
    const double s2 = wchain_tree([=](int64_t i) { return vmx_wchain::square_term(w[i], S); }, count, buf);
    uint64_t* m = C.m + (int64_t)e * C.capacity;
    unsigned long long part = 0;
    for (int64_t i = tid; i < count; i += CHAIN_THREADS) {
        const uint64_t mi = vmx_wchain::integer_weight(w[i], w_max);
        m[i] = mi;
        part += mi;
    }
    atomicAdd(&total, part);
    __syncthreads();
    if (tid == 0) {
        st[0] = w_max; st[1] = S; st[2] = s2;
        reinterpret_cast<uint64_t*>(st)[3] = total;
    }
}

// One work-group per set, behind k_wchain_scale: the means, a tree per column, then the covariance, a tree per pair i >= j in the
// order of k_chain_moments' pairs, and n_eff into the slot of s2
__global__ __launch_bounds__(CHAIN_THREADS) void k_wchain_moments(WchainDev C)
{
    __shared__ double tile[WCHAIN_TILE];
    __shared__ double mean[VMX_ENS_MAXN];
    const int tid = threadIdx.x, e = blockIdx.x, n = C.n;
    const int64_t count = C.counts[e];
    const double* w = C.w + (int64_t)e * C.capacity;
    const double* x = C.x + (int64_t)e * C.capacity * n;
    double* st = C.stats + (int64_t)e * wchain_stride(n);
    double* out_mean = st + WCHAIN_STATS;
    double* cov = out_mean + n;
    if (count < 1) {
        for (int q = tid; q < n + n * n; q += CHAIN_THREADS) out_mean[q] = vmx_wchain::canonical_nan();
        return;
    }
    const double S = st[1], s2 = st[2];
    __syncthreads();                    // (s2 is read by every thread before thread 0 puts n_eff in its place)
    double* buf = vmx_wchain::padded(count) / 2 <= WCHAIN_TILE ? tile : C.tree + (int64_t)e * C.half;
    for (int d = 0; d < n; ++d) {
        const double sum = wchain_tree([=](int64_t i) { return vmx_wchain::mean_term(w[i], S, x[i * n + d]); }, count, buf);
        if (tid == 0) {
            const double v = vmx_wchain::mean_of(S, sum);
            mean[d] = v;
            out_mean[d] = v;
        }
    }
    __syncthreads();
    for (int i = 0; i < n; ++i)
        for (int j = 0; j <= i; ++j) {
            const double mi = mean[i], mj = mean[j];
            const double sum = wchain_tree([=](int64_t k) { return vmx_wchain::cov_term(w[k], S, x[k * n + i], mi, x[k * n + j], mj); }, count, buf);
            if (tid == 0) {
                const double v = vmx_wchain::covariance_of(S, s2, sum);
                cov[i * n + j] = v;
                cov[j * n + i] = v;
            }
        }
    if (tid == 0) st[2] = vmx_wchain::n_eff_of(S, s2);
}

// The keys of every set's rows, x[e][i][d] -> keys[e][d][i] for i < count[e]: the twin of k_chain_keys
__global__ __launch_bounds__(CHAIN_THREADS) void k_wchain_keys(WchainDev C)
{
    const int64_t per = C.capacity * C.n, total = (int64_t)C.E * per;
    for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < total; g += (int64_t)gridDim.x * blockDim.x) {
        const int64_t e = g / per, q = g % per, i = q / C.n;
        const int d = (int)(q % C.n);
        if (i < C.counts[e]) C.keys[(e * C.n + d) * C.capacity + i] = vmx_select::key(C.x[g]);
    }
}

// One work-group per (set, column), behind k_wchain_scale and k_wchain_keys: k_chain_select with sums of the integer weights in
// the histograms (64-bit integer LDS atomics: the sums do not depend on their order; a wave whose keys all fall into one bin adds
// its weights across the wave by shuffles and adds once) and the walk of vmx_chain_weighted.h.  A set without rows or without
// weight answers the canonical NaN.
__global__ __launch_bounds__(CHAIN_THREADS) void k_wchain_select(WchainDev C)
{
    using namespace vmx_select;
    __shared__ unsigned long long hist[vmx_wchain::MAX_TARGETS * BINS];
    __shared__ uint64_t prefix[vmx_wchain::MAX_TARGETS], group_prefix[vmx_wchain::MAX_TARGETS], left[vmx_wchain::MAX_TARGETS];
    __shared__ int group[vmx_wchain::MAX_TARGETS];
    __shared__ int groups;
    const int tid = threadIdx.x, lane = tid & 63, U = C.U;
    const int64_t e = blockIdx.x / C.n, N = C.counts[e];
    const uint64_t M = reinterpret_cast<const uint64_t*>(C.stats + e * wchain_stride(C.n))[3];
    if (N < 1 || M == 0) {
        if (tid < U) C.values[(int64_t)blockIdx.x * U + tid] = CANONICAL_NAN;
        return;
    }
    const uint64_t* keys = C.keys + (int64_t)blockIdx.x * C.capacity;
    const uint64_t* m = C.m + e * C.capacity;
    if (tid < U) { prefix[tid] = 0; left[tid] = C.targets[e * U + tid]; }
    __syncthreads();
    if (tid == 0) groups = regroup(prefix, U, group, group_prefix);
    __syncthreads();
    for (int p = 0; p < PASSES; ++p) {
        const int G = groups;
        for (int q = tid; q < G * BINS; q += blockDim.x) hist[q] = 0;
        __syncthreads();
        for (int64_t base = 0; base < N; base += blockDim.x) {          // (every lane of a wave takes every turn: the ballots below)
            const int64_t i = base + tid;
            int slot = -1;
            unsigned long long mine = 0;
            if (i < N) {
                const uint64_t k = keys[i];
                const int at = find_group(group_prefix, G, leading(k, p));
                if (at >= 0) { slot = at * BINS + digit(k, p); mine = m[i]; }
            }
            const unsigned long long active = __ballot(slot >= 0);
            if (active) {
                const int leader = __ffsll(active) - 1;
                const int slot0 = __shfl(slot, leader);
                const unsigned long long same = __ballot(slot == slot0);
                if (same == active) {
                    unsigned long long sum = mine;                      // (0 in the lanes without a key)
                    for (int s = 32; s > 0; s >>= 1) sum += __shfl_xor(sum, s);
                    if (lane == leader) atomicAdd(&hist[slot0], sum);
                } else if (slot >= 0) {
                    atomicAdd(&hist[slot], mine);
                }
            }
        }
        __syncthreads();
        if (tid < U) {
            uint64_t l = left[tid];
            prefix[tid] = (prefix[tid] << 8) | (uint64_t)vmx_wchain::walk(reinterpret_cast<const uint64_t*>(hist) + group[tid] * BINS, l);
            left[tid] = l;
        }
        __syncthreads();
        if (tid == 0) groups = regroup(prefix, U, group, group_prefix);
        __syncthreads();
    }
    if (tid < U) C.values[(int64_t)blockIdx.x * U + tid] = unkey(prefix[tid]);
}

// One work-group per set: k_chain_best over the rows [0, count[e])
__global__ __launch_bounds__(CHAIN_THREADS) void k_wchain_best(WchainDev C)
{
    using namespace vmx_select;
    __shared__ double value[CHAIN_THREADS];
    __shared__ int64_t index[CHAIN_THREADS];
    const int tid = threadIdx.x, e = blockIdx.x, n = C.n;
    const int64_t count = C.counts[e];
    const double* lnl = C.lnl + (int64_t)e * C.capacity;
    double best = 0.0;
    int64_t at = -1;
    for (int64_t q = tid; q < count; q += CHAIN_THREADS) {
        const double v = lnl[q];
        const int64_t i = v != v ? -1 : q;          // (vmx_select::candidate: a NaN is none)
        if (wins(v, i, best, at)) { best = v; at = i; }
    }
    value[tid] = best;
    index[tid] = at;
    __syncthreads();
    for (int s = CHAIN_THREADS / 2; s > 0; s >>= 1) {
        if (tid < s && wins(value[tid + s], index[tid + s], value[tid], index[tid])) {
            value[tid] = value[tid + s];
            index[tid] = index[tid + s];
        }
        __syncthreads();
    }
    const int64_t won = index[0];
    if (tid == 0) {
        C.best_index[e] = won;
        C.best_lnl[e] = won < 0 ? double_of(CANONICAL_NAN) : value[0];
    }
    if (C.best_x)
        for (int d = tid; d < n; d += CHAIN_THREADS)
            C.best_x[(int64_t)e * n + d] = won < 0 ? double_of(CANONICAL_NAN) : C.x[((int64_t)e * C.capacity + won) * n + d];
}

// what every reduction of a sample store reads
static WchainDev wchain_dev(const vmx_sample_store* s)
{
    WchainDev C{};
    C.x = s->x.p; C.lnl = s->lnl.p; C.w = s->w.p; C.counts = s->counts.p;
    C.capacity = s->capacity; C.half = vmx_wchain::padded(s->capacity) / 2; C.E = s->E; C.n = s->n;
    return C;
}

// the scratch of k_wchain_scale, and the kernel on `st`
static int wchain_scale(vmx_sample_store* s, WchainDev& C, hipStream_t st)
{
    const size_t E = (size_t)s->E, n = (size_t)s->n;
    if (chain_scratch(s->m, E * (size_t)s->capacity) || chain_scratch(s->tree, E * (size_t)C.half) ||
        chain_scratch(s->stats, E * (WCHAIN_STATS + n + n * n)))
        return -2;
    C.m = reinterpret_cast<uint64_t*>(s->m.p); C.tree = s->tree.p; C.stats = s->stats.p;
    hipLaunchKernelGGL(k_wchain_scale, dim3(s->E), dim3(CHAIN_THREADS), 0, st, C);
    return 0;
}

}  // namespace

int vmx_sample_store_create(vmx_engine* e, int32_t E, int32_t n, int64_t capacity_rows, vmx_sample_store** out)
{
    const std::string name("vmx_sample_store_create");
    REQUIRE(e && out, name);
    REQUIRE(E >= 1 && n >= 1 && n <= VMX_ENS_MAXN && capacity_rows >= 0 && capacity_rows <= vmx_wchain::MAX_COUNT,
            name + ": E >= 1, 1 <= n <= VMX_ENS_MAXN, 0 <= capacity_rows < 2^31");
    REQUIRE(chain_fits(E, 1, n, capacity_rows), name + ": the store is too large");
    HIP_OK(hipSetDevice(e->device));
    vmx_sample_store* s = new vmx_sample_store();
    s->engine = e; s->E = E; s->n = n; s->capacity = capacity_rows;
    const size_t slots = (size_t)E * (size_t)capacity_rows;
    if (chain_alloc(s->x, slots * n) || chain_alloc(s->lnl, slots) || chain_alloc(s->w, slots) ||
        (s->counts.alloc((size_t)E, true) && ((void)hipGetLastError(), true))) {
        delete s;
        return -2;
    }
    s->h_counts.assign((size_t)E, 0);
    s->h_total.assign((size_t)E, 0);
    e->sample_stores.push_back(s);
    *out = s;
    return 0;
}

int vmx_sample_store_destroy(vmx_sample_store* s)
{
    REQUIRE(s, "vmx_sample_store_destroy");
    vmx_engine* e = s->engine;
    (void)hipSetDevice(e->device);
    (void)hipStreamSynchronize(e->stream);
    e->sample_stores.erase(std::remove(e->sample_stores.begin(), e->sample_stores.end(), s), e->sample_stores.end());
    delete s;
    return 0;
}

int vmx_sample_store_put(vmx_sample_store* s, int32_t set, int64_t count, const double* x, const double* lnl, const double* w)
{
    const std::string name("vmx_sample_store_put");
    REQUIRE(s && count >= 0 && (count == 0 || (x && lnl && w)), name);
    REQUIRE(set >= 0 && set < s->E, name + ": the set must be one of the store's");
    REQUIRE(count <= s->capacity, name + ": rows beyond the store's capacity");
    double w_max = 0.0;
    for (int64_t i = 0; i < count; ++i) {
        REQUIRE(vmx_wchain::weight_ok(w[i]), name + ": every weight must be finite and >= 0");
        w_max = vmx_wchain::larger(w_max, w[i]);
    }
    uint64_t total = 0;
    for (int64_t i = 0; i < count; ++i) total += vmx_wchain::integer_weight(w[i], w_max);
    vmx_engine* e = s->engine;
    HIP_OK(hipSetDevice(e->device));
    hipStream_t st = e->stream;
    const int64_t at = (int64_t)set * s->capacity;
    if (count > 0) {
        HIP_OK(hipMemcpyAsync(s->x.p + at * s->n, x, (size_t)count * s->n * sizeof(double), hipMemcpyHostToDevice, st));
        HIP_OK(hipMemcpyAsync(s->lnl.p + at, lnl, (size_t)count * sizeof(double), hipMemcpyHostToDevice, st));
        HIP_OK(hipMemcpyAsync(s->w.p + at, w, (size_t)count * sizeof(double), hipMemcpyHostToDevice, st));
    }
    HIP_OK(hipMemcpyAsync(s->counts.p + set, &count, sizeof(int64_t), hipMemcpyHostToDevice, st));
    HIP_OK(hipStreamSynchronize(st));
    s->h_counts[(size_t)set] = count;
    s->h_total[(size_t)set] = total;
    return 0;
}

int vmx_sample_store_counts(vmx_sample_store* s, int64_t* counts)
{
    REQUIRE(s && counts, "vmx_sample_store_counts");
    std::copy(s->h_counts.begin(), s->h_counts.end(), counts);
    return 0;
}

int vmx_sample_store_fetch(vmx_sample_store* s, int32_t set, double* x, double* lnl, double* w)
{
    const std::string name("vmx_sample_store_fetch");
    REQUIRE(s, name);
    REQUIRE(set >= 0 && set < s->E, name + ": the set must be one of the store's");
    const int64_t count = s->h_counts[(size_t)set], at = (int64_t)set * s->capacity;
    if (count == 0 || (!x && !lnl && !w)) return 0;
    vmx_engine* e = s->engine;
    HIP_OK(hipSetDevice(e->device));
    hipStream_t st = e->stream;
    if (x) HIP_OK(hipMemcpyAsync(x, s->x.p + at * s->n, (size_t)count * s->n * sizeof(double), hipMemcpyDeviceToHost, st));
    if (lnl) HIP_OK(hipMemcpyAsync(lnl, s->lnl.p + at, (size_t)count * sizeof(double), hipMemcpyDeviceToHost, st));
    if (w) HIP_OK(hipMemcpyAsync(w, s->w.p + at, (size_t)count * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    return 0;
}

int vmx_sample_store_summary(vmx_sample_store* s, double* S, double* n_eff, double* mean, double* covariance, uint64_t* total, double* w_max)
{
    const std::string name("vmx_sample_store_summary");
    REQUIRE(s && S && n_eff && mean && covariance && total && w_max, name + ": a store and every output");
    vmx_engine* e = s->engine;
    HIP_OK(hipSetDevice(e->device));
    hipStream_t st = e->stream;
    WchainDev C = wchain_dev(s);
    if (wchain_scale(s, C, st)) return -2;
    hipLaunchKernelGGL(k_wchain_moments, dim3(s->E), dim3(CHAIN_THREADS), 0, st, C);
    HIP_OK(hipGetLastError());
    const size_t E = (size_t)s->E, n = (size_t)s->n, stride = WCHAIN_STATS + n + n * n;
    std::vector<double> got(E * stride);
    HIP_OK(hipMemcpyAsync(got.data(), s->stats.p, got.size() * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    for (size_t k = 0; k < E; ++k) {
        const double* g = got.data() + k * stride;
        w_max[k] = g[0]; S[k] = g[1]; n_eff[k] = g[2];
        std::memcpy(total + k, g + 3, sizeof(uint64_t));
        std::memcpy(mean + k * n, g + WCHAIN_STATS, n * sizeof(double));
        std::memcpy(covariance + k * n * n, g + WCHAIN_STATS + n, n * n * sizeof(double));
    }
    return 0;
}

int vmx_sample_store_order_stats(vmx_sample_store* s, int32_t n_targets, const uint64_t* targets, double* values)
{
    const std::string name("vmx_sample_store_order_stats");
    REQUIRE(s && targets && values, name + ": a store, targets and values");
    REQUIRE(n_targets >= 1 && n_targets <= VMX_SAMPLE_MAX_TARGETS, name + ": 1 <= n_targets <= VMX_SAMPLE_MAX_TARGETS");
    const size_t E = (size_t)s->E, n = (size_t)s->n, U = (size_t)n_targets;
    std::vector<uint64_t> sorted(E * U, 1);
    std::vector<int> place(E * U, 0);
    for (size_t k = 0; k < E; ++k) {
        if (s->h_total[k] == 0) {       // (a set without weight ignores its targets)
            for (size_t r = 0; r < U; ++r) place[k * U + r] = (int)r;
            continue;
        }
        for (size_t r = 0; r < U; ++r)
            REQUIRE(targets[k * U + r] >= 1 && targets[k * U + r] <= s->h_total[k], name + ": a target outside [1, M] of its set");
        vmx_wchain::sort_targets(targets + k * U, n_targets, sorted.data() + k * U, place.data() + k * U);
    }
    vmx_engine* e = s->engine;
    HIP_OK(hipSetDevice(e->device));
    hipStream_t st = e->stream;
    WchainDev C = wchain_dev(s);
    if (chain_scratch(s->keys, E * n * (size_t)s->capacity) || chain_scratch(s->targets, E * U) || chain_scratch(s->out, E * n * U)) return -2;
    C.keys = reinterpret_cast<uint64_t*>(s->keys.p); C.targets = reinterpret_cast<const uint64_t*>(s->targets.p);
    C.values = reinterpret_cast<uint64_t*>(s->out.p); C.U = n_targets;
    HIP_OK(hipMemcpyAsync(s->targets.p, sorted.data(), E * U * sizeof(uint64_t), hipMemcpyHostToDevice, st));
    if (wchain_scale(s, C, st)) return -2;
    const int64_t total = (int64_t)E * s->capacity * s->n;
    const int blocks = (int)std::max<int64_t>(1, std::min<int64_t>((total + CHAIN_THREADS - 1) / CHAIN_THREADS, 65536));
    hipLaunchKernelGGL(k_wchain_keys, dim3(blocks), dim3(CHAIN_THREADS), 0, st, C);
    hipLaunchKernelGGL(k_wchain_select, dim3((unsigned)(E * n)), dim3(CHAIN_THREADS), 0, st, C);
    HIP_OK(hipGetLastError());
    std::vector<double> found(E * n * U);
    HIP_OK(hipMemcpyAsync(found.data(), s->out.p, found.size() * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    // the caller's order and repeats (bytes are copied: a value's bits stay its own)
    for (size_t k = 0; k < E; ++k)
        for (size_t d = 0; d < n; ++d)
            for (size_t r = 0; r < U; ++r)
                std::memcpy(values + (k * n + d) * U + r, found.data() + (k * n + d) * U + place[k * U + r], sizeof(double));
    return 0;
}

int vmx_sample_store_best(vmx_sample_store* s, double* lnl_max, int64_t* index, double* position)
{
    const std::string name("vmx_sample_store_best");
    REQUIRE(s && lnl_max && index, name + ": a store, lnl_max and index");
    vmx_engine* e = s->engine;
    HIP_OK(hipSetDevice(e->device));
    const size_t E = (size_t)s->E, En = E * (size_t)s->n;
    if (chain_scratch(s->out, E + En) || (s->index.n < E && s->index.alloc(E, false) && ((void)hipGetLastError(), true))) return -2;
    WchainDev C = wchain_dev(s);
    C.best_lnl = s->out.p; C.best_x = position ? s->out.p + E : nullptr; C.best_index = s->index.p;
    hipStream_t st = e->stream;
    hipLaunchKernelGGL(k_wchain_best, dim3(s->E), dim3(CHAIN_THREADS), 0, st, C);
    HIP_OK(hipGetLastError());
    HIP_OK(hipMemcpyAsync(lnl_max, C.best_lnl, E * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_OK(hipMemcpyAsync(index, C.best_index, E * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    if (position) HIP_OK(hipMemcpyAsync(position, C.best_x, En * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    return 0;
}

// ---- evidence where the live points live (vmx_nested.h)
static_assert(VMX_NS_MAXN == vmx_ns::MAXN && VMX_NS_MAX_LIVE == vmx_ns::MAX_LIVE, "nested sampling limits");

static_assert(VMX_NS_KNN == vmx_ns::KNN && VMX_NS_MAX_CLUSTERS == vmx_ns::MAX_CLUSTERS, "nested sampling clusters");

// k_ns_knn for n coordinates (the tile's row is the next power of two) and k_ns_cluster, on `st`
static int launch_clustering(const NsClusterDev& C, hipStream_t st)
{
    const dim3 grid((C.m + NS_KNN_THREADS - 1) / NS_KNN_THREADS), block(NS_KNN_THREADS);
    if (C.n <= 1) hipLaunchKernelGGL(k_ns_knn<1>, grid, block, 0, st, C);
    else if (C.n <= 2) hipLaunchKernelGGL(k_ns_knn<2>, grid, block, 0, st, C);
    else if (C.n <= 4) hipLaunchKernelGGL(k_ns_knn<4>, grid, block, 0, st, C);
    else if (C.n <= 8) hipLaunchKernelGGL(k_ns_knn<8>, grid, block, 0, st, C);
    else if (C.n <= 16) hipLaunchKernelGGL(k_ns_knn<16>, grid, block, 0, st, C);
    else hipLaunchKernelGGL(k_ns_knn<32>, grid, block, 0, st, C);
    HIP_OK(hipGetLastError());
    hipLaunchKernelGGL(k_ns_cluster, dim3(1), dim3(NS_THREADS), 0, st, C);
    HIP_OK(hipGetLastError());
    return 0;
}

static int nested_run(const char* who, vmx_engine* e, const vmx_nested_spec* spec, double* live_u, double* live_lnl, int64_t* iteration,
                      int32_t n_iterations, double* dead_u, double* dead_lnl, int32_t* dead_nlive,
                      const vmx_nested_options* opt, vmx_nested_stats* stats, const vmx_nested_clusters* clusters,
                      vmx_nested_phantoms* phantoms = nullptr);

int vmx_nested_run(vmx_engine* e, const vmx_nested_spec* spec, double* live_u, double* live_lnl, int64_t* iteration,
                   int32_t n_iterations, double* dead_u, double* dead_lnl, int32_t* dead_nlive,
                   const vmx_nested_options* opt, vmx_nested_stats* stats)
{
    return nested_run("vmx_nested_run", e, spec, live_u, live_lnl, iteration, n_iterations, dead_u, dead_lnl, dead_nlive, opt, stats,
                      nullptr);
}

int vmx_nested_run_clustered(vmx_engine* e, const vmx_nested_spec* spec, double* live_u, double* live_lnl, int64_t* iteration,
                             int32_t n_iterations, double* dead_u, double* dead_lnl, int32_t* dead_nlive,
                             const vmx_nested_options* opt, vmx_nested_stats* stats, const vmx_nested_clusters* clusters)
{
    REQUIRE(clusters, "vmx_nested_run_clustered: the clusters");
    REQUIRE((clusters->flags & ~(uint32_t)VMX_NS_CLUSTER) == 0, "vmx_nested_run_clustered: flags 0 or VMX_NS_CLUSTER");
    return nested_run("vmx_nested_run_clustered", e, spec, live_u, live_lnl, iteration, n_iterations, dead_u, dead_lnl, dead_nlive, opt,
                      stats, (clusters->flags & VMX_NS_CLUSTER) ? clusters : nullptr);
}

int vmx_nested_run_phantoms(vmx_engine* e, const vmx_nested_spec* spec, double* live_u, double* live_lnl, int64_t* iteration,
                            int32_t n_iterations, double* dead_u, double* dead_lnl, int32_t* dead_nlive,
                            const vmx_nested_options* opt, vmx_nested_stats* stats, const vmx_nested_clusters* clusters,
                            vmx_nested_phantoms* phantoms)
{
    const std::string name("vmx_nested_run_phantoms");
    if (clusters) REQUIRE((clusters->flags & ~(uint32_t)VMX_NS_CLUSTER) == 0, name + ": flags 0 or VMX_NS_CLUSTER");
    const vmx_nested_clusters* cl = clusters && (clusters->flags & VMX_NS_CLUSTER) ? clusters : nullptr;
    if (phantoms) REQUIRE(phantoms->fraction >= 0.0 && phantoms->fraction <= 1.0, name + ": the kept fraction lies in [0, 1]");
    // (fraction 0: the run without phantoms, and nothing in the struct is touched)
    return nested_run("vmx_nested_run_phantoms", e, spec, live_u, live_lnl, iteration, n_iterations, dead_u, dead_lnl, dead_nlive, opt,
                      stats, cl, phantoms && phantoms->fraction > 0.0 ? phantoms : nullptr);
}

int vmx_nested_cluster_points(int32_t device, const double* u, int32_t m, int32_t n, const int32_t* prev_id, int32_t* next_id,
                              int32_t* ids, int32_t* k_used, int32_t* n_clusters, double* means, double* factors)
{
    REQUIRE(u && prev_id && next_id && ids && k_used && n_clusters && means && factors, "vmx_nested_cluster_points");
    REQUIRE(n >= 1 && n <= VMX_NS_MAXN, "vmx_nested_cluster_points: 1 .. 32 coordinates");
    REQUIRE(m >= 2 && m <= VMX_NS_MAX_LIVE, "vmx_nested_cluster_points: 2 .. 4096 points");
    REQUIRE(*next_id >= 1 && *next_id <= 0x7fffffff - VMX_NS_MAX_CLUSTERS, "vmx_nested_cluster_points: next_id >= 1");
    for (int i = 0; i < m; ++i) REQUIRE(prev_id[i] >= 0 && prev_id[i] < *next_id, "vmx_nested_cluster_points: 0 <= prev_id < next_id");
    for (size_t q = 0; q < (size_t)m * n; ++q) REQUIRE(std::isfinite(u[q]), "vmx_nested_cluster_points: a coordinate is not finite");
    HIP_OK(hipSetDevice(device));
    constexpr int MAXC = VMX_NS_MAX_CLUSTERS;
    DevBuf<double> d_u, d_mean, d_cov, d_chol;
    DevBuf<int32_t> d_ids, d_nn, d_slot, d_cid, d_csize, d_info;
    DevBuf<uint8_t> d_lev;
    if (d_u.alloc((size_t)m * n, false) || d_mean.alloc((size_t)MAXC * n) || d_cov.alloc((size_t)MAXC * n * n) ||
        d_chol.alloc((size_t)MAXC * n * n) || d_ids.alloc(m, false) || d_nn.alloc((size_t)m * VMX_NS_KNN, false) ||
        d_slot.alloc(m, false) || d_cid.alloc(MAXC) || d_csize.alloc(MAXC) || d_info.alloc(4) || d_lev.alloc((size_t)m * VMX_NS_KNN, false))
        return -2;
    hipStream_t st = nullptr;
    const int32_t info_in[4] = {0, 0, *next_id, 0};
    HIP_OK(hipMemcpyAsync(d_u.p, u, (size_t)m * n * sizeof(double), hipMemcpyHostToDevice, st));
    HIP_OK(hipMemcpyAsync(d_ids.p, prev_id, (size_t)m * sizeof(int32_t), hipMemcpyHostToDevice, st));
    HIP_OK(hipMemcpyAsync(d_info.p, info_in, sizeof(info_in), hipMemcpyHostToDevice, st));
    HIP_OK(hipStreamSynchronize(st));       // (info_in leaves the stack)
    const NsClusterDev C{d_u.p, nullptr, d_ids.p, d_nn.p, d_lev.p, d_slot.p, d_cid.p, d_csize.p, d_info.p, d_mean.p, d_cov.p, d_chol.p, m, n};
    if (launch_clustering(C, st)) return -2;
    int32_t info[4] = {0, 0, 0, 0};
    HIP_OK(hipMemcpyAsync(info, d_info.p, sizeof(info), hipMemcpyDeviceToHost, st));
    HIP_OK(hipMemcpyAsync(ids, d_ids.p, (size_t)m * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    HIP_OK(hipMemcpyAsync(means, d_mean.p, (size_t)MAXC * n * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_OK(hipMemcpyAsync(factors, d_chol.p, (size_t)MAXC * n * n * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    *k_used = info[0]; *n_clusters = info[1]; *next_id = info[2];
    return 0;
}

static int nested_run(const char* who, vmx_engine* e, const vmx_nested_spec* spec, double* live_u, double* live_lnl, int64_t* iteration,
                      int32_t n_iterations, double* dead_u, double* dead_lnl, int32_t* dead_nlive,
                      const vmx_nested_options* opt, vmx_nested_stats* stats, const vmx_nested_clusters* clusters,
                      vmx_nested_phantoms* phantoms)
{
    const std::string name(who);
    REQUIRE(e && e->finalized && spec && live_u && live_lnl && iteration, name);
    std::vector<char> varies;
    std::vector<int32_t> inv;
    if (check_box(name, e, spec, VMX_NS_MAXN, varies, inv)) return -1;
    const int n = spec->n, P = e->n_params, nlive = spec->nlive, K = spec->K;
    REQUIRE(nlive >= n + 2 && nlive <= VMX_NS_MAX_LIVE, name + ": n + 2 .. 4096 live points");
    REQUIRE(K >= 1 && K <= nlive - n - 1, name + ": 1 .. nlive - n - 1 threads");
    REQUIRE(spec->num_repeats >= 1, name + ": num_repeats >= 1");
    REQUIRE(n_iterations >= 0 && *iteration >= 0, name + ": n_iterations >= 0, iteration >= 0");
    REQUIRE(n_iterations == 0 || (dead_u && dead_lnl && dead_nlive), name + ": the dead record");
    const bool draw = opt && opt->draw_live != 0;
    const bool clustering = clusters != nullptr;
    if (clustering) {
        REQUIRE(clusters->live_cluster && clusters->next_id, name + ": live_cluster, next_id");
        REQUIRE(n_iterations == 0 || clusters->dead_cluster, name + ": the dead record's ids");
        REQUIRE(*clusters->next_id >= 1, name + ": next_id >= 1");
        REQUIRE((int64_t)*clusters->next_id + (int64_t)n_iterations * VMX_NS_MAX_CLUSTERS < 0x7fffffff, name + ": next_id would overflow");
        for (int i = 0; i < nlive; ++i)
            REQUIRE(clusters->live_cluster[i] >= 0 && clusters->live_cluster[i] < *clusters->next_id, name + ": 0 <= live_cluster < next_id");
    }
    const bool recording = phantoms != nullptr;
    const int64_t ph_need = (int64_t)n_iterations * K * (spec->num_repeats - 1);       // (what the call can keep at the most)
    if (recording) {
        REQUIRE(phantoms->flags == 0, name + ": phantoms->flags 0");
        REQUIRE(phantoms->capacity >= ph_need, name + ": phantoms->capacity below n_iterations K (num_repeats - 1)");
        REQUIRE(ph_need == 0 || (phantoms->u && phantoms->lnl && phantoms->birth && phantoms->iteration && phantoms->thread &&
                                 phantoms->repeat && (!clustering || phantoms->cluster)), name + ": the phantom record");
    }
    REQUIRE(!draw || *iteration == 0, name + ": live points are drawn at iteration 0");
    if (!draw)
        for (int i = 0; i < nlive; ++i) {
            REQUIRE(!std::isnan(live_lnl[i]), name + ": a live point has a NaN lnL");
            for (int d = 0; d < n; ++d) {
                const double v = live_u[(size_t)i * n + d];
                REQUIRE(v >= 0.0 && v <= 1.0, name + ": a live point lies outside the unit cube");
            }
        }
    if (LikelihoodSession::check(name, opt ? opt->const_hint : -1, opt ? opt->chunk : 0, opt ? opt->lanes : 0, true)) return -1;
    const size_t cap = (size_t)std::max(nlive, K), rec_rows = (size_t)std::max(n_iterations, 1) * K;

    HIP_OK(hipSetDevice(e->device));
    const auto t_begin = std::chrono::steady_clock::now();
    if (!e->nsws) e->nsws = new NsWorkspace();
    NsWorkspace& S = *e->nsws;
    if (ensure(S.live_u, (size_t)nlive * n) || ensure(S.live_lnl, nlive) || ensure(S.rank, nlive) || ensure(S.surv, nlive) ||
        ensure(S.killed, K) || ensure(S.mean, n) || ensure(S.cov, (size_t)n * n) || ensure(S.chol, (size_t)n * n) || ensure(S.lstar, 1) ||
        ensure_structs(S.th, (size_t)K * sizeof(vmx_ns::Thread) / sizeof(double)) ||        // (vmx_ns::Thread: states and counts; exempt from poison)
        ensure(S.slot, K) || ensure(S.dead_u, rec_rows * n) ||
        ensure(S.dead_lnl, rec_rows) || ensure(S.dead_n, rec_rows) || ensure(S.counters, 1))
        return -2;
    const int m = nlive - K;
    if (clustering &&
        (ensure(S.live_cluster, nlive) || ensure(S.dead_cluster, rec_rows) || ensure(S.nn, (size_t)m * VMX_NS_KNN) ||
         ensure(S.lev, (size_t)m * VMX_NS_KNN) || ensure(S.cslot, m) || ensure(S.tslot, K) || ensure(S.cl_id, VMX_NS_MAX_CLUSTERS) ||
         ensure(S.cl_size, VMX_NS_MAX_CLUSTERS) || ensure(S.cl_info, 4) || ensure(S.cl_mean, (size_t)VMX_NS_MAX_CLUSTERS * n) ||
         ensure(S.cl_cov, (size_t)VMX_NS_MAX_CLUSTERS * n * n) || ensure(S.cl_chol, (size_t)VMX_NS_MAX_CLUSTERS * n * n)))
        return -2;
    const size_t ph_rows = (size_t)std::max<int64_t>(ph_need, 1);
    if (recording &&
        (ensure(S.ph_u, ph_rows * n) || ensure(S.ph_lnl, ph_rows) || ensure(S.ph_birth, ph_rows) || ensure(S.ph_it, ph_rows) ||
         ensure(S.ph_thread, ph_rows) || ensure(S.ph_repeat, ph_rows) || (clustering && ensure(S.ph_cluster, ph_rows)) || ensure(S.ph_count, 1)))
        return -2;
    if (!S.pin_word) {
        HIP_OK(hipHostMalloc((void**)&S.pin_word, 16 * sizeof(int32_t), hipHostMallocMapped));
        HIP_OK(hipHostGetDevicePointer((void**)&S.dpin_word, S.pin_word, 0));
    }
    if (S.pin_lnl_n < (size_t)nlive + K) {
        if (S.pin_lnl) { (void)hipHostFree(S.pin_lnl); S.pin_lnl = nullptr; S.pin_lnl_n = 0; }
        HIP_OK(hipHostMalloc((void**)&S.pin_lnl, ((size_t)nlive + K) * sizeof(double), hipHostMallocMapped));
        HIP_OK(hipHostGetDevicePointer((void**)&S.dpin_lnl, S.pin_lnl, 0));
        S.pin_lnl_n = (size_t)nlive + K;
    }
    hipStream_t st = e->stream;
    if (!draw) {
        HIP_OK(hipMemcpyAsync(S.live_u.p, live_u, (size_t)nlive * n * sizeof(double), hipMemcpyHostToDevice, st));
        HIP_OK(hipMemcpyAsync(S.live_lnl.p, live_lnl, (size_t)nlive * sizeof(double), hipMemcpyHostToDevice, st));
    }
    HIP_OK(hipMemsetAsync(S.counters.p, 0, sizeof(int64_t), st));
    NsDev D{};
    if (S.box.upload(cap, P, n, spec->theta_fixed, spec->lo, spec->hi, inv, st, D.box)) return -2;
    D.live_u = S.live_u.p; D.live_lnl = S.live_lnl.p; D.rank = S.rank.p; D.surv = S.surv.p; D.killed = S.killed.p;
    D.mean = S.mean.p; D.cov = S.cov.p; D.chol = S.chol.p; D.lstar = S.lstar.p;
    D.th = (vmx_ns::Thread*)S.th.p; D.slot = S.slot.p;
    D.dead_u = S.dead_u.p; D.dead_lnl = S.dead_lnl.p; D.dead_n = S.dead_n.p;
    D.host_word = S.dpin_word; D.host_lnl = S.dpin_lnl; D.counters = S.counters.p;
    D.nlive = nlive; D.K = K; D.n = n; D.P = P; D.num_repeats = spec->num_repeats;
    D.log_norm = spec->log_norm; D.seed = spec->seed; D.stream = spec->stream;
    NsClusterRun X{};
    if (clustering) {
        S.info_host[0] = S.info_host[1] = S.info_host[3] = 0;
        S.info_host[2] = *clusters->next_id;
        HIP_OK(hipMemcpyAsync(S.live_cluster.p, clusters->live_cluster, (size_t)nlive * sizeof(int32_t), hipMemcpyHostToDevice, st));
        HIP_OK(hipMemcpyAsync(S.cl_info.p, S.info_host, sizeof(S.info_host), hipMemcpyHostToDevice, st));
        X.cl = NsClusterDev{S.live_u.p, S.surv.p, S.live_cluster.p, S.nn.p, S.lev.p, S.cslot.p, S.cl_id.p, S.cl_size.p, S.cl_info.p,
                            S.cl_mean.p, S.cl_cov.p, S.cl_chol.p, m, n};
        X.dead_cluster = S.dead_cluster.p; X.tslot = S.tslot.p;
    }
    NsPhantomRun F{};
    if (recording) {
        HIP_OK(hipMemsetAsync(S.ph_count.p, 0, sizeof(int64_t), st));
        F = NsPhantomRun{S.ph_u.p, S.ph_lnl.p, S.ph_birth.p, S.ph_it.p, S.ph_thread.p, S.ph_repeat.p, S.ph_cluster.p, S.ph_count.p,
                         ph_need, phantoms->fraction};      // (the device record holds ph_need rows, whatever the host's capacity)
    }
    int64_t ph_count = 0;

    // the engine as the sampler's likelihood, at the table level the sampled columns allow
    LikelihoodSession L(e, opt ? opt->const_hint : -1, opt ? opt->chunk : 0, opt ? opt->lanes : 0, e->max_batch, varies);
    vmx_nested_stats R{};
    R.const_hint = L.hint;
    R.lanes = L.lanes;
    double enqueue_s = 0.0;
    // the first `total` rows (the host has waited for the kernel that wrote them: they are there for either lane)
    auto evaluate = [&](int total) -> int {
        const auto t0 = std::chrono::steady_clock::now();
        const int calls = L.evaluate(S.box.theta.p, total, S.box.chi2.p, S.box.status.p, nullptr, false);
        if (calls < 0) return -2;
        R.engine_calls += calls;
        enqueue_s += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        return 0;
    };
    if (draw) {
        hipLaunchKernelGGL(k_ns_draw_live, dim3(1), dim3(NS_THREADS), 0, st, D);
        HIP_OK(hipGetLastError());
        HIP_OK(hipStreamSynchronize(st));       // (the second lane reads the rows)
        R.host_waits += 1;
        R.rows += nlive;
        if (evaluate(nlive)) return -2;
        hipLaunchKernelGGL(k_ns_live_lnl, dim3(1), dim3(NS_THREADS), 0, st, D);
        HIP_OK(hipGetLastError());
    }
    int done = 0;
    while (done < n_iterations) {
        const int64_t it = *iteration + done;
        if (clustering) {
            X.phase = 0;
            hipLaunchKernelGGL(k_ns_iteration_clustered, dim3(1), dim3(NS_THREADS), 0, st, D, X, it, (int64_t)done);
            HIP_OK(hipGetLastError());
            if (launch_clustering(X.cl, st)) return -2;
            X.phase = 1;
            hipLaunchKernelGGL(k_ns_iteration_clustered, dim3(1), dim3(NS_THREADS), 0, st, D, X, it, (int64_t)done);
        } else hipLaunchKernelGGL(k_ns_iteration, dim3(1), dim3(NS_THREADS), 0, st, D, it, (int64_t)done);
        for (;;) {
            if (recording) {
                if (clustering) hipLaunchKernelGGL(k_ns_advance_phantoms_clustered, dim3(1), dim3(NS_THREADS), 0, st, D, X, F, it, (int64_t)done);
                else hipLaunchKernelGGL(k_ns_advance_phantoms, dim3(1), dim3(NS_THREADS), 0, st, D, F, it, (int64_t)done);
            } else if (clustering) hipLaunchKernelGGL(k_ns_advance_clustered, dim3(1), dim3(NS_THREADS), 0, st, D, X, it, (int64_t)done);
            else hipLaunchKernelGGL(k_ns_advance, dim3(1), dim3(NS_THREADS), 0, st, D, it, (int64_t)done);
            HIP_OK(hipGetLastError());
            HIP_OK(hipStreamSynchronize(st));   // (the round's only wait: the row count, one mapped word)
            R.host_waits += 1;
            if (recording) std::memcpy(&ph_count, S.pin_word + 2, sizeof(int64_t));     // (the phantom rows so far, beside it)
            const int total = S.pin_word[0];
            if (total <= 0) break;
            if ((size_t)total > cap) return fail(-2, name + ": a round asked for more rows than its buffers hold");
            R.rounds += 1;
            R.rows += total;
            if (evaluate(total)) return -2;
        }
        done += 1;
        std::memcpy(live_lnl, S.pin_lnl, (size_t)nlive * sizeof(double));
        if (opt && opt->stop && opt->stop(opt->user, *iteration + done, S.pin_lnl + nlive, live_lnl)) break;
    }
    HIP_OK(hipMemcpyAsync(live_u, S.live_u.p, (size_t)nlive * n * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_OK(hipMemcpyAsync(live_lnl, S.live_lnl.p, (size_t)nlive * sizeof(double), hipMemcpyDeviceToHost, st));
    if (done > 0) {
        HIP_OK(hipMemcpyAsync(dead_u, S.dead_u.p, (size_t)done * K * n * sizeof(double), hipMemcpyDeviceToHost, st));
        HIP_OK(hipMemcpyAsync(dead_lnl, S.dead_lnl.p, (size_t)done * K * sizeof(double), hipMemcpyDeviceToHost, st));
        HIP_OK(hipMemcpyAsync(dead_nlive, S.dead_n.p, (size_t)done * K * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    }
    if (recording && (ph_count < 0 || ph_count > ph_need)) return fail(-2, name + ": the phantom record overran its capacity");
    if (recording && ph_count > 0) {
        const size_t c = (size_t)ph_count;
        HIP_OK(hipMemcpyAsync(phantoms->u, S.ph_u.p, c * n * sizeof(double), hipMemcpyDeviceToHost, st));
        HIP_OK(hipMemcpyAsync(phantoms->lnl, S.ph_lnl.p, c * sizeof(double), hipMemcpyDeviceToHost, st));
        HIP_OK(hipMemcpyAsync(phantoms->birth, S.ph_birth.p, c * sizeof(double), hipMemcpyDeviceToHost, st));
        HIP_OK(hipMemcpyAsync(phantoms->iteration, S.ph_it.p, c * sizeof(int64_t), hipMemcpyDeviceToHost, st));
        HIP_OK(hipMemcpyAsync(phantoms->thread, S.ph_thread.p, c * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        HIP_OK(hipMemcpyAsync(phantoms->repeat, S.ph_repeat.p, c * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        if (clustering) HIP_OK(hipMemcpyAsync(phantoms->cluster, S.ph_cluster.p, c * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    }
    int32_t info_out[4] = {0, 0, 0, 0};
    if (clustering) {
        HIP_OK(hipMemcpyAsync(clusters->live_cluster, S.live_cluster.p, (size_t)nlive * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        HIP_OK(hipMemcpyAsync(info_out, S.cl_info.p, sizeof(info_out), hipMemcpyDeviceToHost, st));
        if (done > 0)
            HIP_OK(hipMemcpyAsync(clusters->dead_cluster, S.dead_cluster.p, (size_t)done * K * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    }
    int64_t own = 0;
    HIP_OK(hipMemcpyAsync(&own, S.counters.p, sizeof(int64_t), hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    R.host_waits += 1;
    *iteration += done;
    if (clustering) *clusters->next_id = info_out[2];
    if (recording) phantoms->count = ph_count;
    R.iterations = done;
    R.rows_own_position = own;
    R.seconds_enqueuing = enqueue_s;
    R.seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_begin).count();
    if (stats) *stats = R;
    return 0;
}

// E independent runs advanced together (vmx_nested.h "a set of runs"): per set round one launch heads the runs whose iteration
// begins, one advances every thread of every active run, one packs the requests of all runs into the engine's rows; the host
// waits once per round.  `phantoms` (vmx_nested_run_many_phantoms): every run keeps its phantom record, the advance launch is
// k_ns_set_advance_phantoms; nullptr: the launches are what they were.
static int nested_run_many(const char* who, vmx_engine* e, const vmx_nested_spec* spec, int32_t E, const uint64_t* streams,
                           const int32_t* mock_row, double* live_u, double* live_lnl, int64_t* iteration, int32_t* status,
                           int32_t n_iterations, double* dead_u, double* dead_lnl, int32_t* dead_nlive, int32_t* iterations_done,
                           const vmx_nested_set_options* opt, vmx_nested_stats* stats, int64_t* per_run,
                           vmx_nested_set_phantoms* phantoms);

int vmx_nested_run_many(vmx_engine* e, const vmx_nested_spec* spec, int32_t E, const uint64_t* streams, const int32_t* mock_row,
                        double* live_u, double* live_lnl, int64_t* iteration, int32_t* status, int32_t n_iterations,
                        double* dead_u, double* dead_lnl, int32_t* dead_nlive, int32_t* iterations_done,
                        const vmx_nested_set_options* opt, vmx_nested_stats* stats, int64_t* per_run)
{
    return nested_run_many("vmx_nested_run_many", e, spec, E, streams, mock_row, live_u, live_lnl, iteration, status, n_iterations,
                           dead_u, dead_lnl, dead_nlive, iterations_done, opt, stats, per_run, nullptr);
}

int vmx_nested_run_many_phantoms(vmx_engine* e, const vmx_nested_spec* spec, int32_t E, const uint64_t* streams, const int32_t* mock_row,
                                 double* live_u, double* live_lnl, int64_t* iteration, int32_t* status, int32_t n_iterations,
                                 double* dead_u, double* dead_lnl, int32_t* dead_nlive, int32_t* iterations_done,
                                 const vmx_nested_set_options* opt, vmx_nested_stats* stats, int64_t* per_run,
                                 vmx_nested_set_phantoms* phantoms)
{
    const std::string name("vmx_nested_run_many_phantoms");
    if (phantoms) REQUIRE(phantoms->fraction >= 0.0 && phantoms->fraction <= 1.0, name + ": the kept fraction lies in [0, 1]");
    // (fraction 0: the set without phantoms, and nothing in the struct is touched)
    return nested_run_many("vmx_nested_run_many_phantoms", e, spec, E, streams, mock_row, live_u, live_lnl, iteration, status,
                           n_iterations, dead_u, dead_lnl, dead_nlive, iterations_done, opt, stats, per_run,
                           phantoms && phantoms->fraction > 0.0 ? phantoms : nullptr);
}

static int nested_run_many(const char* who, vmx_engine* e, const vmx_nested_spec* spec, int32_t E, const uint64_t* streams,
                           const int32_t* mock_row, double* live_u, double* live_lnl, int64_t* iteration, int32_t* status,
                           int32_t n_iterations, double* dead_u, double* dead_lnl, int32_t* dead_nlive, int32_t* iterations_done,
                           const vmx_nested_set_options* opt, vmx_nested_stats* stats, int64_t* per_run,
                           vmx_nested_set_phantoms* phantoms)
{
    const std::string name(who);
    REQUIRE(e && e->finalized && spec && live_u && live_lnl && iteration && status && iterations_done, name);
    REQUIRE(E >= 1, name + ": at least one run");
    REQUIRE(streams, name + ": a Philox stream for every run");
    std::vector<char> varies;
    std::vector<int32_t> inv;
    if (check_box(name, e, spec, VMX_NS_MAXN, varies, inv)) return -1;
    const int n = spec->n, P = e->n_params, nlive = spec->nlive, K = spec->K;
    REQUIRE(nlive >= n + 2 && nlive <= VMX_NS_MAX_LIVE, name + ": n + 2 .. 4096 live points");
    REQUIRE(K >= 1 && K <= nlive - n - 1, name + ": 1 .. nlive - n - 1 threads");
    REQUIRE(spec->num_repeats >= 1, name + ": num_repeats >= 1");
    REQUIRE(n_iterations >= 0, name + ": n_iterations >= 0");
    REQUIRE(n_iterations == 0 || (dead_u && dead_lnl && dead_nlive), name + ": the dead record");
    // sizes: the engine's rows are counted in int32, the largest array (the record, or the rows themselves) in size_t
    REQUIRE((int64_t)E * nlive <= INT32_MAX, name + ": E nlive exceeds the engine's row count");
    const size_t EL = (size_t)E * nlive, EK = (size_t)E * K, rec_iter = (size_t)std::max(n_iterations, 1), rec_rows = rec_iter * K;
    const size_t per_row = (size_t)std::max(n, P) * sizeof(double);
    REQUIRE(EL <= SIZE_MAX / per_row && EK * per_row <= SIZE_MAX / rec_iter, name + ": the record is too large");
    const bool draw = opt && opt->draw_live != 0;
    for (int q = 0; q < E; ++q) {
        REQUIRE(iteration[q] >= 0, name + ": iteration >= 0");
        REQUIRE(!draw || iteration[q] == 0, name + ": live points are drawn at iteration 0");
        if (draw) continue;
        for (size_t i = (size_t)q * nlive; i < (size_t)(q + 1) * nlive; ++i) {
            REQUIRE(!std::isnan(live_lnl[i]), name + ": a live point has a NaN lnL");
            for (int d = 0; d < n; ++d) {
                const double v = live_u[i * n + d];
                REQUIRE(v >= 0.0 && v <= 1.0, name + ": a live point lies outside the unit cube");
            }
        }
    }
    if (mock_row)
        for (int q = 0; q < E; ++q)
            for (auto* it : e->items) {
                REQUIRE(it->n_mocks > 0 && it->dev.mock_pool, name + ": mock rows, but an item has no mock pool");
                REQUIRE(mock_row[q] >= 0 && mock_row[q] < it->n_mocks, name + ": mock row outside the pool");
            }
    const bool recording = phantoms != nullptr;
    int64_t ph_need = 0;                // (what one run can keep in this call at the most: the rows of its part of the device record)
    if (recording) {
        REQUIRE(phantoms->flags == 0, name + ": phantoms->flags 0");
        REQUIRE((double)n_iterations * K * ((double)spec->num_repeats - 1.0) * E * (8.0 * n + 36.0) < 9.0e18, name + ": the phantom record is too large");
        ph_need = vmx_ns::set_phantom_capacity(n_iterations, K, spec->num_repeats);
        REQUIRE(phantoms->capacity >= ph_need, name + ": phantoms->capacity below n_iterations K (num_repeats - 1)");
        REQUIRE(phantoms->count, name + ": phantoms->count [E]");
        REQUIRE(ph_need == 0 || (phantoms->u && phantoms->lnl && phantoms->birth && phantoms->iteration && phantoms->thread &&
                                 phantoms->repeat), name + ": the phantom record");
    }
    if (LikelihoodSession::check(name, opt ? opt->const_hint : -1, opt ? opt->chunk : 0, opt ? opt->lanes : 0, true)) return -1;
    const size_t cap = EL;          // (K < nlive: the draw's rows are the most a launch writes)

    HIP_OK(hipSetDevice(e->device));
    const auto t_begin = std::chrono::steady_clock::now();
    if (!e->nsws) e->nsws = new NsWorkspace();
    NsWorkspace& S = *e->nsws;
    if (ensure(S.live_u, EL * n) || ensure(S.live_lnl, EL) || ensure(S.rank, EL) || ensure(S.surv, EL) || ensure(S.killed, EK) ||
        ensure(S.mean, (size_t)E * n) || ensure(S.cov, (size_t)E * n * n) || ensure(S.chol, (size_t)E * n * n) || ensure(S.lstar, E) ||
        ensure_structs(S.th, EK * sizeof(vmx_ns::Thread) / sizeof(double)) ||       // (vmx_ns::Thread: states and counts; exempt from poison)
        ensure(S.slot, EK) || ensure(S.dead_u, E * rec_rows * n) ||
        ensure(S.dead_lnl, E * rec_rows) || ensure(S.dead_n, E * rec_rows) || ensure(S.counters, E) || ensure(S.set_ctl, (size_t)3 * E) ||
        ensure(S.set_count, E) || ensure(S.streams, E) || ensure(S.it0, E) || (mock_row && (ensure(S.mock_row, E) || ensure(S.mock, cap))))
        return -2;
    const size_t ph_rows = (size_t)E * (size_t)std::max<int64_t>(ph_need, 1);
    if (recording &&
        (ensure(S.ph_u, ph_rows * n) || ensure(S.ph_lnl, ph_rows) || ensure(S.ph_birth, ph_rows) || ensure(S.ph_it, ph_rows) ||
         ensure(S.ph_thread, ph_rows) || ensure(S.ph_repeat, ph_rows) || ensure(S.ph_count, E)))
        return -2;
    if (!S.pin_word) {
        HIP_OK(hipHostMalloc((void**)&S.pin_word, 16 * sizeof(int32_t), hipHostMallocMapped));
        HIP_OK(hipHostGetDevicePointer((void**)&S.dpin_word, S.pin_word, 0));
    }
    const size_t lnl_words = (size_t)E * ((size_t)nlive + K);
    if (S.pin_lnl_n < lnl_words) {
        if (S.pin_lnl) { (void)hipHostFree(S.pin_lnl); S.pin_lnl = nullptr; S.pin_lnl_n = 0; }
        HIP_OK(hipHostMalloc((void**)&S.pin_lnl, lnl_words * sizeof(double), hipHostMallocMapped));
        HIP_OK(hipHostGetDevicePointer((void**)&S.dpin_lnl, S.pin_lnl, 0));
        S.pin_lnl_n = lnl_words;
    }
    if (S.set_runs < (size_t)E) {
        if (S.set_host) { (void)hipHostFree(S.set_host); S.set_host = nullptr; }
        if (S.pin_count) { (void)hipHostFree(S.pin_count); S.pin_count = nullptr; }
        S.set_runs = 0;
        HIP_OK(hipHostMalloc((void**)&S.set_host, (size_t)3 * E * sizeof(int32_t), hipHostMallocDefault));
        HIP_OK(hipHostMalloc((void**)&S.pin_count, (size_t)E * sizeof(int32_t), hipHostMallocMapped));
        HIP_OK(hipHostGetDevicePointer((void**)&S.dpin_count, S.pin_count, 0));
        S.set_runs = (size_t)E;
    }
    hipStream_t st = e->stream;
    if (!draw) {
        HIP_OK(hipMemcpyAsync(S.live_u.p, live_u, EL * n * sizeof(double), hipMemcpyHostToDevice, st));
        HIP_OK(hipMemcpyAsync(S.live_lnl.p, live_lnl, EL * sizeof(double), hipMemcpyHostToDevice, st));
    }
    HIP_OK(hipMemcpyAsync(S.streams.p, streams, (size_t)E * sizeof(uint64_t), hipMemcpyHostToDevice, st));
    HIP_OK(hipMemcpyAsync(S.it0.p, iteration, (size_t)E * sizeof(int64_t), hipMemcpyHostToDevice, st));
    if (mock_row) HIP_OK(hipMemcpyAsync(S.mock_row.p, mock_row, (size_t)E * sizeof(int32_t), hipMemcpyHostToDevice, st));
    HIP_OK(hipMemsetAsync(S.counters.p, 0, (size_t)E * sizeof(int64_t), st));
    NsSetDev X{};
    NsDev& D = X.run0;
    if (S.box.upload(cap, P, n, spec->theta_fixed, spec->lo, spec->hi, inv, st, D.box)) return -2;
    D.live_u = S.live_u.p; D.live_lnl = S.live_lnl.p; D.rank = S.rank.p; D.surv = S.surv.p; D.killed = S.killed.p;
    D.mean = S.mean.p; D.cov = S.cov.p; D.chol = S.chol.p; D.lstar = S.lstar.p;
    D.th = (vmx_ns::Thread*)S.th.p; D.slot = S.slot.p;
    D.dead_u = S.dead_u.p; D.dead_lnl = S.dead_lnl.p; D.dead_n = S.dead_n.p;
    D.host_word = S.dpin_word; D.host_lnl = S.dpin_lnl; D.counters = S.counters.p;
    D.nlive = nlive; D.K = K; D.n = n; D.P = P; D.num_repeats = spec->num_repeats;
    D.log_norm = spec->log_norm; D.seed = spec->seed; D.stream = 0;
    X.active = S.set_ctl.p; X.heading = S.set_ctl.p + E; X.done = S.set_ctl.p + 2 * (size_t)E;
    X.it0 = S.it0.p; X.streams = S.streams.p;
    X.mock_row = mock_row ? S.mock_row.p : nullptr; X.mock = mock_row ? S.mock.p : nullptr;
    X.count = S.set_count.p; X.host_count = S.dpin_count; X.rec_rows = (int32_t)rec_iter;
    const int32_t* d_mock = mock_row ? S.mock.p : nullptr;
    NsPhantomRun F{};
    if (recording) {
        HIP_OK(hipMemsetAsync(S.ph_count.p, 0, (size_t)E * sizeof(int64_t), st));
        F = NsPhantomRun{S.ph_u.p, S.ph_lnl.p, S.ph_birth.p, S.ph_it.p, S.ph_thread.p, S.ph_repeat.p, nullptr, S.ph_count.p,
                         ph_need, phantoms->fraction};      // (run e's part of the device record: the rows from e ph_need)
    }

    // the engine as the sampler's likelihood, at the table level the sampled columns allow
    LikelihoodSession L(e, opt ? opt->const_hint : -1, opt ? opt->chunk : 0, opt ? opt->lanes : 0, e->max_batch, varies);
    vmx_nested_stats R{};
    R.const_hint = L.hint;
    R.lanes = L.lanes;
    double enqueue_s = 0.0;
    std::vector<int64_t> rows_of(E, 0), rounds_of(E, 0);
    std::vector<int32_t> phase(E, vmx_ns::OUT);
    int32_t* active = S.set_host;
    int32_t* heading = S.set_host + E;
    int32_t* done = S.set_host + 2 * (size_t)E;
    for (int q = 0; q < E; ++q) { status[q] = vmx_ns::GOING; done[q] = 0; active[q] = q; }
    int A = E, H = 0;
    // the lists and the iterations done go up on the stream: the host changes them only after it has waited for the stream
    auto put_lists = [&]() -> int {
        X.A = A;
        HIP_OK(hipMemcpyAsync(S.set_ctl.p, S.set_host, (size_t)3 * E * sizeof(int32_t), hipMemcpyHostToDevice, st));
        return 0;
    };
    auto evaluate = [&](int total, bool from_kernel) -> int {
        const auto t0 = std::chrono::steady_clock::now();
        const int calls = L.evaluate(S.box.theta.p, total, S.box.chi2.p, S.box.status.p, d_mock, from_kernel);
        if (calls < 0) return -2;
        R.engine_calls += calls;
        R.rows += total;
        enqueue_s += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        return 0;
    };
    if (draw) {
        if (put_lists()) return -2;
        hipLaunchKernelGGL(k_ns_set_draw_live, dim3(A), dim3(NS_THREADS), 0, st, X);
        HIP_OK(hipGetLastError());
        if (evaluate(E * nlive, true)) return -2;
        hipLaunchKernelGGL(k_ns_set_live_lnl, dim3(A), dim3(NS_THREADS), 0, st, X);
        HIP_OK(hipGetLastError());
        HIP_OK(hipStreamSynchronize(st));       // (the draw's wait: whether every run has a live point with a finite lnL)
        R.host_waits += 1;
        for (int q = 0; q < E; ++q) { rows_of[q] += nlive; status[q] = vmx_ns::start_status(S.pin_count[q]); }
    }
    A = vmx_ns::first_active(status, E, n_iterations, active, phase.data());
    while (A > 0) {
        const auto t0 = std::chrono::steady_clock::now();
        H = vmx_ns::heading_list(active, A, phase.data(), heading);
        if (put_lists()) return -2;
        if (H > 0) hipLaunchKernelGGL(k_ns_set_head, dim3(H), dim3(NS_THREADS), 0, st, X);
        if (recording) hipLaunchKernelGGL(k_ns_set_advance_phantoms, dim3(A), dim3(NS_THREADS), 0, st, X, F);
        else hipLaunchKernelGGL(k_ns_set_advance, dim3(A), dim3(NS_THREADS), 0, st, X);
        hipLaunchKernelGGL(k_ns_set_emit, dim3(A), dim3(NS_THREADS), 0, st, X);
        HIP_OK(hipGetLastError());
        enqueue_s += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        HIP_OK(hipStreamSynchronize(st));       // (the round's only wait: the total and the runs' counts, mapped words)
        R.host_waits += 1;
        R.rounds += 1;
        const int total = S.pin_word[0];
        if (total < 0 || (size_t)total > cap) return fail(-2, name + ": a round asked for more rows than its buffers hold");
        if (total > 0 && evaluate(total, false)) return -2;
        for (int a = 0; a < A; ++a) {
            const int q = active[a];
            const int32_t cnt = S.pin_count[q];
            rounds_of[q] += 1;
            rows_of[q] += cnt;
            if (!vmx_ns::iteration_ended(cnt)) { phase[q] = vmx_ns::WALK; continue; }
            done[q] += 1;
            const double* word = S.pin_lnl + (size_t)q * ((size_t)nlive + K);
            std::memcpy(live_lnl + (size_t)q * nlive, word, (size_t)nlive * sizeof(double));
            const bool stopped = opt && opt->stop && opt->stop(opt->user, q, iteration[q] + done[q], word + nlive, live_lnl + (size_t)q * nlive);
            phase[q] = vmx_ns::after_iteration(stopped, done[q], n_iterations, &status[q]);
        }
        A = vmx_ns::compact_active(active, A, phase.data());
    }
    // the runs that were entered come back; a run without a finite live lnL leaves its arrays as they were
    std::vector<int64_t> own(E, 0);
    for (int q = 0; q < E; ++q) {
        if (status[q] == vmx_ns::NO_FINITE) continue;
        const size_t o = (size_t)q * nlive;
        HIP_OK(hipMemcpyAsync(live_u + o * n, S.live_u.p + o * n, (size_t)nlive * n * sizeof(double), hipMemcpyDeviceToHost, st));
        HIP_OK(hipMemcpyAsync(live_lnl + o, S.live_lnl.p + o, (size_t)nlive * sizeof(double), hipMemcpyDeviceToHost, st));
        if (done[q] == 0) continue;
        const size_t r = (size_t)q * rec_rows, h = (size_t)q * n_iterations * K, rows = (size_t)done[q] * K;
        HIP_OK(hipMemcpyAsync(dead_u + h * n, S.dead_u.p + r * n, rows * n * sizeof(double), hipMemcpyDeviceToHost, st));
        HIP_OK(hipMemcpyAsync(dead_lnl + h, S.dead_lnl.p + r, rows * sizeof(double), hipMemcpyDeviceToHost, st));
        HIP_OK(hipMemcpyAsync(dead_nlive + h, S.dead_n.p + r, rows * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        if (!recording || ph_need == 0) continue;
        // the run's count is on the device: the rows its done[q] iterations can have kept at the most come back in this copy
        // (the kept ones lead them), and the counts behind them
        const size_t c = (size_t)vmx_ns::set_phantom_capacity(done[q], K, spec->num_repeats);
        const size_t dr = (size_t)vmx_ns::set_phantom_row(q, ph_need, 0, 0), hr = (size_t)vmx_ns::set_phantom_row(q, phantoms->capacity, 0, 0);
        HIP_OK(hipMemcpyAsync(phantoms->u + hr * n, S.ph_u.p + dr * n, c * n * sizeof(double), hipMemcpyDeviceToHost, st));
        HIP_OK(hipMemcpyAsync(phantoms->lnl + hr, S.ph_lnl.p + dr, c * sizeof(double), hipMemcpyDeviceToHost, st));
        HIP_OK(hipMemcpyAsync(phantoms->birth + hr, S.ph_birth.p + dr, c * sizeof(double), hipMemcpyDeviceToHost, st));
        HIP_OK(hipMemcpyAsync(phantoms->iteration + hr, S.ph_it.p + dr, c * sizeof(int64_t), hipMemcpyDeviceToHost, st));
        HIP_OK(hipMemcpyAsync(phantoms->thread + hr, S.ph_thread.p + dr, c * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        HIP_OK(hipMemcpyAsync(phantoms->repeat + hr, S.ph_repeat.p + dr, c * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    }
    std::vector<int64_t> ph_count(E, 0);
    if (recording) HIP_OK(hipMemcpyAsync(ph_count.data(), S.ph_count.p, (size_t)E * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    HIP_OK(hipMemcpyAsync(own.data(), S.counters.p, (size_t)E * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    R.host_waits += 1;
    if (recording)
        for (int q = 0; q < E; ++q) {
            if (ph_count[q] < 0 || ph_count[q] > vmx_ns::set_phantom_capacity(done[q], K, spec->num_repeats))
                return fail(-2, name + ": a run's phantom record overran its capacity");
            phantoms->count[q] = ph_count[q];
        }
    for (int q = 0; q < E; ++q) {
        iterations_done[q] = done[q];
        iteration[q] += done[q];
        if (per_run) { per_run[3 * q] = rows_of[q]; per_run[3 * q + 1] = own[q]; per_run[3 * q + 2] = rounds_of[q]; }
        R.iterations += done[q];
        R.rows_own_position += own[q];
    }
    R.seconds_enqueuing = enqueue_s;
    R.seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_begin).count();
    if (stats) *stats = R;
    return 0;
}

// ---- evidence where the particles live (vmx_smc.h)
static_assert(VMX_SMC_MAX_PARTICLES == vmx_smc::MAX_PARTICLES && VMX_NS_MAXN == vmx_smc::MAXN, "SMC limits");

// E independent runs advanced together (k_smc_*): one host round per stage for every run still going, the A N rows of a sweep
// as one stream of chunks for the engine, every row with the mock of its run.  The one body of the four entries: `name` is the
// entry that was called, keep = nullptr the calls without kept populations, E = 1 the single run (smc_run_one).
// rounds_back_to_back (the single run): while every run still going is at beta = 1 and owes posterior rounds, as many of them as
// the call may run are enqueued with one wait; otherwise the host waits once per round.
static int smc_run(const std::string& name, vmx_engine* e, const vmx_smc_spec* spec, int32_t E, const uint64_t* streams,
                   const int32_t* mock_row, double* u, double* lnl, int64_t* stage, double* beta, double* scale, int32_t* status,
                   int32_t n_stages, double* rec, double* rec_lnl, int32_t* rec_anc, int32_t* stages_done,
                   const vmx_smc_keep* keep, const vmx_smc_options* opt, vmx_smc_stats* stats, int64_t* per_run,
                   bool rounds_back_to_back)
{
    REQUIRE(e && e->finalized && spec && u && lnl && stage && beta && scale && status && stages_done, name);
    REQUIRE(E >= 1, name + ": at least one run");
    double* const rec_u = keep ? keep->rec_u : nullptr;
    std::vector<int32_t> owed((size_t)E, 0);
    if (keep && keep->topups_left) owed.assign(keep->topups_left, keep->topups_left + E);
    REQUIRE(!keep || keep->flags == 0, name + ": keep->flags must be 0");
    bool any_owed = false;
    for (int q = 0; q < E; ++q) {
        REQUIRE(owed[q] >= 0, name + ": topups_left >= 0");
        any_owed = any_owed || owed[q] > 0;
    }
    REQUIRE(!any_owed || rec_u, name + ": posterior rounds are owed, but there is no rec_u");
    const bool kept = rec_u != nullptr || any_owed;         // (neither: the kernels of vmx_smc_run_many)
    REQUIRE(streams, name + ": a Philox stream for every run");
    std::vector<char> varies;
    std::vector<int32_t> inv;
    if (check_box(name, e, spec, VMX_NS_MAXN, varies, inv)) return -1;
    const int n = spec->n, P = e->n_params, N = spec->N, sweeps = spec->sweeps;
    REQUIRE(N >= std::max(2 * n + 2, 8) && N <= VMX_SMC_MAX_PARTICLES, name + ": max(2 n + 2, 8) .. 4096 particles");
    REQUIRE(spec->ess > 0.0 && spec->ess < 1.0, name + ": 0 < ess < 1");
    REQUIRE(sweeps >= 1, name + ": sweeps >= 1");
    REQUIRE(n_stages >= 0, name + ": n_stages >= 0");
    REQUIRE(n_stages == 0 || (rec && rec_lnl && rec_anc), name + ": the stage record");
    // sizes: the engine's rows are counted in int32, the largest array (the record, or the rows themselves) in size_t
    REQUIRE((int64_t)E * N <= INT32_MAX, name + ": E N exceeds the engine's row count");
    const size_t EN = (size_t)E * N, rec_rows = (size_t)std::max(n_stages, 1);
    const size_t per_row = (size_t)std::max(std::max(n, P), VMX_SMC_REC) * sizeof(double);
    REQUIRE(EN <= SIZE_MAX / per_row && EN * per_row <= SIZE_MAX / rec_rows, name + ": the record is too large");
    REQUIRE(!rec_u || (EN * rec_rows <= SIZE_MAX / ((size_t)n * sizeof(double))), name + ": the record is too large");
    const bool draw = opt && opt->draw != 0;
    for (int q = 0; q < E; ++q) {
        REQUIRE(stage[q] >= 0 && stage[q] < ((int64_t)1 << 31), name + ": 0 <= stage < 2^31");
        REQUIRE(!draw || stage[q] == 0, name + ": particles are drawn at stage 0");
        if (draw) continue;
        REQUIRE(beta[q] >= 0.0 && beta[q] <= 1.0, name + ": beta in [0, 1]");
        REQUIRE(scale[q] > 0.0 && std::isfinite(scale[q]), name + ": a positive scale");
        bool any = false;
        for (size_t i = (size_t)q * N; i < (size_t)(q + 1) * N; ++i) {
            REQUIRE(!std::isnan(lnl[i]), name + ": a particle has a NaN lnL");
            any = any || lnl[i] > -INFINITY;
            for (int d = 0; d < n; ++d) {
                const double v = u[i * n + d];
                REQUIRE(v >= 0.0 && v <= 1.0, name + ": a particle lies outside the unit cube");
            }
        }
        REQUIRE(any, name + ": no particle has a finite lnL");
    }
    if (mock_row)
        for (int q = 0; q < E; ++q)
            for (auto* it : e->items) {
                REQUIRE(it->n_mocks > 0 && it->dev.mock_pool, name + ": mock rows, but an item has no mock pool");
                REQUIRE(mock_row[q] >= 0 && mock_row[q] < it->n_mocks, name + ": mock row outside the pool");
            }
    if (LikelihoodSession::check(name, opt ? opt->const_hint : -1, opt ? opt->chunk : 0, opt ? opt->lanes : 0, true)) return -1;

    HIP_OK(hipSetDevice(e->device));
    const auto t_begin = std::chrono::steady_clock::now();
    if (!e->smcws) e->smcws = new SmcWorkspace();
    SmcWorkspace& S = *e->smcws;
    if (ensure(S.u, EN * n) || ensure(S.lnl, EN) || ensure(S.u2, EN * n) || ensure(S.lnl2, EN) || ensure(S.w, EN) || ensure(S.cum, EN) ||
        ensure(S.zero, N) || ensure(S.mean, (size_t)E * n) || ensure(S.cov, (size_t)E * n * n) || ensure(S.chol, (size_t)E * n * n) ||
        ensure(S.state, (size_t)E * 2) || ensure(S.prop, EN * n) || ensure(S.uacc, EN) || ensure(S.inside, EN) ||
        ensure(S.rec, E * rec_rows * VMX_SMC_REC) || ensure(S.rec_lnl, rec_rows * EN) || ensure(S.rec_anc, rec_rows * EN) ||
        ensure(S.counters, (size_t)E * 3) || ensure(S.active, E) || ensure(S.streams, E) || ensure(S.stage0, E) ||
        (mock_row && (ensure(S.mock_row, E) || ensure(S.mock, EN))) || (rec_u && ensure(S.rec_u, rec_rows * EN * n)))
        return -2;
    if (S.runs < (size_t)E) {
        if (S.pin) { (void)hipHostFree(S.pin); S.pin = nullptr; }
        if (S.pin_active) { (void)hipHostFree(S.pin_active); S.pin_active = nullptr; }
        S.runs = 0;
        HIP_OK(hipHostMalloc((void**)&S.pin, (size_t)E * 4 * sizeof(double), hipHostMallocMapped));
        HIP_OK(hipHostGetDevicePointer((void**)&S.dpin, S.pin, 0));
        HIP_OK(hipHostMalloc((void**)&S.pin_active, (size_t)E * sizeof(int32_t), hipHostMallocDefault));
        S.runs = (size_t)E;
    }
    hipStream_t st = e->stream;
    std::vector<double> state0((size_t)E * 2);
    for (int q = 0; q < E; ++q) { state0[2 * q] = beta[q]; state0[2 * q + 1] = scale[q]; }
    if (!draw) {
        HIP_OK(hipMemcpyAsync(S.u.p, u, EN * n * sizeof(double), hipMemcpyHostToDevice, st));
        HIP_OK(hipMemcpyAsync(S.lnl.p, lnl, EN * sizeof(double), hipMemcpyHostToDevice, st));
        HIP_OK(hipMemcpyAsync(S.state.p, state0.data(), state0.size() * sizeof(double), hipMemcpyHostToDevice, st));
    }
    HIP_OK(hipMemcpyAsync(S.streams.p, streams, (size_t)E * sizeof(uint64_t), hipMemcpyHostToDevice, st));
    HIP_OK(hipMemcpyAsync(S.stage0.p, stage, (size_t)E * sizeof(int64_t), hipMemcpyHostToDevice, st));
    if (mock_row) HIP_OK(hipMemcpyAsync(S.mock_row.p, mock_row, (size_t)E * sizeof(int32_t), hipMemcpyHostToDevice, st));
    HIP_OK(hipMemsetAsync(S.zero.p, 0, (size_t)N * sizeof(int32_t), st));
    HIP_OK(hipMemsetAsync(S.counters.p, 0, (size_t)E * 3 * sizeof(int64_t), st));
    HIP_OK(hipMemsetAsync(S.rec.p, 0, E * rec_rows * VMX_SMC_REC * sizeof(double), st));
    SmcSetDev X{};
    SmcDev& D = X.run0;
    if (S.box.upload(EN, P, n, spec->theta_fixed, spec->lo, spec->hi, inv, st, D.box)) return -2;
    D.u = S.u.p; D.lnl = S.lnl.p; D.u2 = S.u2.p; D.lnl2 = S.lnl2.p; D.w = S.w.p; D.cum = S.cum.p; D.zero = S.zero.p;
    D.mean = S.mean.p; D.cov = S.cov.p; D.chol = S.chol.p; D.state = S.state.p;
    D.prop = S.prop.p; D.uacc = S.uacc.p; D.inside = S.inside.p;
    D.rec = S.rec.p; D.rec_lnl = S.rec_lnl.p; D.rec_anc = S.rec_anc.p; D.counters = S.counters.p; D.host = S.dpin;
    D.N = N; D.n = n; D.P = P; D.sweeps = sweeps; D.ess = spec->ess; D.log_norm = spec->log_norm;
    D.seed = spec->seed; D.stream = 0;
    X.active = S.active.p; X.streams = S.streams.p; X.stage0 = S.stage0.p;
    X.mock_row = mock_row ? S.mock_row.p : nullptr; X.mock = mock_row ? S.mock.p : nullptr;
    X.rec_rows = (int32_t)rec_rows;
    const int32_t* d_mock = mock_row ? S.mock.p : nullptr;

    // the engine as the sampler's likelihood, at the table level the sampled columns allow
    LikelihoodSession L(e, opt ? opt->const_hint : -1, opt ? opt->chunk : 0, opt ? opt->lanes : 0, e->max_batch, varies);
    vmx_smc_stats R{};
    R.const_hint = L.hint;
    R.lanes = L.lanes;
    double enqueue_s = 0.0;
    std::vector<int64_t> rows_of(E, 0);
    std::vector<int32_t> done(E, 0);
    std::vector<double> b_now(beta, beta + E), scale_now(scale, scale + E);
    int32_t* active = S.pin_active;
    int A = vmx_smc::first_active_kept(beta, owed.data(), E, draw, active, status);
    // the list goes up on the stream: the host changes it only after it has waited for the stream
    auto put_active = [&]() -> int {
        if (A > 0) HIP_OK(hipMemcpyAsync(S.active.p, active, (size_t)A * sizeof(int32_t), hipMemcpyHostToDevice, st));
        return 0;
    };
    // the A N rows a launch has just written
    auto evaluate = [&]() -> int {
        const int calls = L.evaluate(S.box.theta.p, A * N, S.box.chi2.p, S.box.status.p, d_mock, true);
        if (calls < 0) return -2;
        R.engine_calls += calls;
        R.rows += (int64_t)A * N;
        for (int a = 0; a < A; ++a) rows_of[active[a]] += N;
        return 0;
    };
    if (put_active()) return -2;
    if (draw) {
        const auto t0 = std::chrono::steady_clock::now();
        hipLaunchKernelGGL(k_smc_start, dim3(A), dim3(SMC_THREADS), 0, st, X);
        HIP_OK(hipGetLastError());
        if (evaluate()) return -2;
        hipLaunchKernelGGL(k_smc_start_lnl, dim3(A), dim3(SMC_THREADS), 0, st, X);
        HIP_OK(hipGetLastError());
        enqueue_s += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        HIP_OK(hipStreamSynchronize(st));       // (the start's wait: how many particles of every run have a finite lnL)
        R.host_waits += 1;
        for (int a = 0; a < A; ++a) {
            const int q = active[a];
            status[q] = vmx_smc::start_status(S.pin[(size_t)q * 4 + 3]);
            b_now[q] = 0.0;
            scale_now[q] = vmx_smc::start_scale(n);
        }
        const int B = vmx_smc::compact_active(active, A, status);
        if (B != A) { A = B; if (put_active()) return -2; }
    }
    // a round's kernels: the heads, the first proposals, and per sweep the engine and the sweep boundary
    auto enqueue_round = [&](int64_t k) -> int {
        if (kept) hipLaunchKernelGGL(k_smc_stage_kept, dim3(A), dim3(SMC_THREADS), 0, st, X, k, rec_u ? S.rec_u.p : nullptr);
        else hipLaunchKernelGGL(k_smc_stage, dim3(A), dim3(SMC_THREADS), 0, st, X, k);
        hipLaunchKernelGGL(k_smc_move, dim3(A), dim3(SMC_THREADS), 0, st, X, k, -1, 0);
        HIP_OK(hipGetLastError());
        for (int s = 0; s < sweeps; ++s) {
            if (evaluate()) return -2;
            hipLaunchKernelGGL(k_smc_move, dim3(A), dim3(SMC_THREADS), 0, st, X, k, s, s + 1 < sweeps ? s + 1 : -1);
            HIP_OK(hipGetLastError());
        }
        return 0;
    };
    int round = 0;
    while (round < n_stages && A > 0) {
        // posterior rounds need no decision of the host: back to back, as many as the call may run and every run still going owes
        int burst = 1;
        if (rounds_back_to_back) {
            burst = n_stages - round;
            for (int a = 0; a < A; ++a) burst = std::min(burst, b_now[active[a]] >= 1.0 ? owed[active[a]] : 1);
        }
        const auto t0 = std::chrono::steady_clock::now();
        for (int k = 0; k < burst; ++k)
            if (enqueue_round(round + k)) return -2;
        enqueue_s += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        HIP_OK(hipStreamSynchronize(st));       // (the only wait: beta and scale of every run after the last round, mapped words)
        R.host_waits += 1;
        for (int a = 0; a < A; ++a) {
            const int q = active[a];
            const double* word = S.pin + (size_t)q * 4;
            for (int k = 0; k < burst; ++k) status[q] = vmx_smc::run_status_kept(b_now[q], word[0], owed[q]);
            if (status[q] == vmx_smc::NO_FINITE || status[q] == vmx_smc::STUCK) continue;
            b_now[q] = word[0];
            scale_now[q] = word[2];
            done[q] += burst;
        }
        const int B = vmx_smc::compact_active(active, A, status);
        round += burst;
        if (B != A) { A = B; if (put_active()) return -2; }
    }
    // the runs that ended by themselves or are still going come back; a failed run's arrays stay as they were at entry
    std::vector<double> rec_host(E * rec_rows * VMX_SMC_REC, 0.0);
    for (int q = 0; q < E; ++q) {
        if (status[q] == vmx_smc::NO_FINITE || status[q] == vmx_smc::STUCK) { done[q] = 0; continue; }
        const size_t o = (size_t)q * N;
        HIP_OK(hipMemcpyAsync(u + o * n, S.u.p + o * n, (size_t)N * n * sizeof(double), hipMemcpyDeviceToHost, st));
        HIP_OK(hipMemcpyAsync(lnl + o, S.lnl.p + o, (size_t)N * sizeof(double), hipMemcpyDeviceToHost, st));
        if (done[q] == 0) continue;
        const size_t r = (size_t)q * rec_rows, h = (size_t)q * n_stages;
        HIP_OK(hipMemcpyAsync(rec_lnl + h * N, S.rec_lnl.p + r * N, (size_t)done[q] * N * sizeof(double), hipMemcpyDeviceToHost, st));
        HIP_OK(hipMemcpyAsync(rec_anc + h * N, S.rec_anc.p + r * N, (size_t)done[q] * N * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        if (rec_u)
            HIP_OK(hipMemcpyAsync(rec_u + h * N * n, S.rec_u.p + r * N * n, (size_t)done[q] * N * n * sizeof(double), hipMemcpyDeviceToHost, st));
    }
    HIP_OK(hipMemcpyAsync(rec_host.data(), S.rec.p, rec_host.size() * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    R.host_waits += 1;
    for (int q = 0; q < E; ++q) {
        int64_t took = 0, own = 0, bad = 0;     // (a failed run: done = 0)
        for (int k = 0; k < done[q]; ++k) {
            const double* r = rec_host.data() + ((size_t)q * rec_rows + k) * VMX_SMC_REC;
            took += (int64_t)r[3];
            own += (int64_t)r[6];
            bad += (int64_t)r[7];
        }
        if (done[q] > 0)
            std::memcpy(rec + (size_t)q * n_stages * VMX_SMC_REC, rec_host.data() + (size_t)q * rec_rows * VMX_SMC_REC,
                        (size_t)done[q] * VMX_SMC_REC * sizeof(double));
        if (status[q] != vmx_smc::NO_FINITE && status[q] != vmx_smc::STUCK) {
            stage[q] += done[q]; beta[q] = b_now[q]; scale[q] = scale_now[q];
            if (keep && keep->topups_left) keep->topups_left[q] = owed[q];
        }
        stages_done[q] = done[q];
        if (per_run) { per_run[4 * q] = took; per_run[4 * q + 1] = own; per_run[4 * q + 2] = bad; per_run[4 * q + 3] = rows_of[q]; }
        R.accepted += took;
        R.rows_own_position += own;
        R.rejected_failed_model += bad;
        R.stages += done[q];
    }
    R.sweeps = R.stages * sweeps;
    R.seconds_enqueuing = enqueue_s;
    R.seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_begin).count();
    if (stats) *stats = R;
    return 0;
}

// vmx_smc_run (keep = nullptr) and vmx_smc_run_kept: the set of one on spec->stream, the installed data and the caller's own words.
// A run that cannot go on fails the call (-2); nothing of the caller's has been written then, *stats neither.
static int smc_run_one(const std::string& name, vmx_engine* e, const vmx_smc_spec* spec, double* u, double* lnl, int64_t* stage,
                       double* beta, double* scale, int32_t n_stages, double* rec, double* rec_lnl, int32_t* rec_anc,
                       const vmx_smc_keep* keep, const vmx_smc_options* opt, vmx_smc_stats* stats)
{
    int32_t status = 0, stages_done = 0;
    vmx_smc_stats R{};
    const int rc = smc_run(name, e, spec, 1, spec ? &spec->stream : nullptr, nullptr, u, lnl, stage, beta, scale, &status, n_stages, rec,
                           rec_lnl, rec_anc, &stages_done, keep, opt, &R, nullptr, true);
    if (rc) return rc;
    if (status == vmx_smc::STUCK)
        return fail(-2, name + ": the temperature ladder cannot advance: fewer than ess N particles carry weight");
    if (status == vmx_smc::NO_FINITE)           // (after a draw with the start's rows alone evaluated: the start found none)
        return fail(-2, name + (opt && opt->draw && R.rows == spec->N ? ": no start particle has a finite lnL" : ": no particle has a finite lnL"));
    if (stats) *stats = R;
    return 0;
}

int vmx_smc_run(vmx_engine* e, const vmx_smc_spec* spec, double* u, double* lnl, int64_t* stage, double* beta, double* scale,
                int32_t n_stages, double* rec, double* rec_lnl, int32_t* rec_anc, const vmx_smc_options* opt,
                vmx_smc_stats* stats)
{
    return smc_run_one("vmx_smc_run", e, spec, u, lnl, stage, beta, scale, n_stages, rec, rec_lnl, rec_anc, nullptr, opt, stats);
}

int vmx_smc_run_kept(vmx_engine* e, const vmx_smc_spec* spec, double* u, double* lnl, int64_t* stage, double* beta, double* scale,
                     int32_t n_stages, double* rec, double* rec_lnl, int32_t* rec_anc, const vmx_smc_keep* keep,
                     const vmx_smc_options* opt, vmx_smc_stats* stats)
{
    return smc_run_one("vmx_smc_run_kept", e, spec, u, lnl, stage, beta, scale, n_stages, rec, rec_lnl, rec_anc, keep, opt, stats);
}

int vmx_smc_run_many(vmx_engine* e, const vmx_smc_spec* spec, int32_t E, const uint64_t* streams, const int32_t* mock_row,
                     double* u, double* lnl, int64_t* stage, double* beta, double* scale, int32_t* status, int32_t n_stages,
                     double* rec, double* rec_lnl, int32_t* rec_anc, int32_t* stages_done, const vmx_smc_options* opt,
                     vmx_smc_stats* stats, int64_t* per_run)
{
    return smc_run("vmx_smc_run_many", e, spec, E, streams, mock_row, u, lnl, stage, beta, scale, status, n_stages, rec, rec_lnl,
                   rec_anc, stages_done, nullptr, opt, stats, per_run, false);
}

int vmx_smc_run_many_kept(vmx_engine* e, const vmx_smc_spec* spec, int32_t E, const uint64_t* streams, const int32_t* mock_row,
                          double* u, double* lnl, int64_t* stage, double* beta, double* scale, int32_t* status, int32_t n_stages,
                          double* rec, double* rec_lnl, int32_t* rec_anc, int32_t* stages_done, const vmx_smc_keep* keep,
                          const vmx_smc_options* opt, vmx_smc_stats* stats, int64_t* per_run)
{
    return smc_run("vmx_smc_run_many_kept", e, spec, E, streams, mock_row, u, lnl, stage, beta, scale, status, n_stages, rec,
                   rec_lnl, rec_anc, stages_done, keep, opt, stats, per_run, false);
}

void* vmx_stream(vmx_engine* e) { return e ? (void*)e->stream : nullptr; }
void* vmx_last_stream(vmx_engine* e) { return e ? (void*)(e->last_stream ? e->last_stream : e->stream) : nullptr; }

int vmx_set_lanes(vmx_engine* e, int32_t lanes)
{
    REQUIRE(e && e->finalized && lanes >= 1 && lanes <= VMX_MAX_LANES, "vmx_set_lanes: 1 or 2 (after vmx_finalize)");
    HIP_OK(hipSetDevice(e->device));
    if (lanes < e->n_lanes) drop_lane(e);
    e->n_lanes = lanes;
    // (the four-stage ring of the FFTLog product wins 5 us when its launch has the chip to itself; with two batches in flight
    // its 128 KB blocks keep the other lane's kernels off their CUs: 831k against 849k evaluations / s at B = 256)
    e->ring_allowed = lanes == 1;
    e->lane_calls = 0;
    return 0;
}

int vmx_set_direct_pk(vmx_engine* e, const double* pk, int32_t B, int32_t nk)
{
    REQUIRE(e && e->finalized, "vmx_set_direct_pk");
    drop_lane(e);
    HIP_OK(hipSetDevice(e->device));
    HIP_OK(hipStreamSynchronize(e->stream));
    if (!pk) { e->direct = false; e->dev.pk_direct = nullptr; return 0; }
    REQUIRE(B > 0 && B <= e->max_batch && nk == e->nk, "direct_pk shape: [B <= max_batch][nk]");
    for (auto* m : e->metals)
        REQUIRE(!(m->dev.d.in_direct && m->dev.d.pipeline >= 0 && e->pipes[m->dev.d.pipeline].poly_basis >= 0),
                "direct_pk: a metal pair that enters the direct model sits on a static basis of the template's spectra - build the "
                "engine with vmx_set_static_poly(e, 0)");
    // (every check before any state changes: a refused call leaves the engine as it was)
    for (auto& p : e->pipes)
        REQUIRE(!(p.odd_rel || p.odd_asy) || p.odd_dyn_off >= 0,
                "direct_pk: a pipeline with odd-multipole terms needs their operator form (vmx_pipeline_set_odd_operator)");
    if (e->pk_direct.n < (size_t)e->max_batch * e->nkp && e->pk_direct.alloc((size_t)e->max_batch * e->nkp, true)) return -2;
    HIP_OK(hipMemcpy2D(e->pk_direct.p, (size_t)e->nkp * sizeof(double), pk, (size_t)nk * sizeof(double),
                       (size_t)nk * sizeof(double), B, hipMemcpyHostToDevice));
    // the odd-multipole terms read the caller's spectrum too: the walkers' spline coefficients = operator . spectrum
    for (auto& kv : e->odd_op_off) {
        const PipeDev& p = e->pipes[kv.first];
        if (vmx_matvec_device(e, e->odd_op.p + kv.second, 4 * p.odd_ncoef, e->nkp, e->pk_direct.p, B, e->odd_dyn.p + p.odd_dyn_off)) {
            e->direct = false; e->dev.pk_direct = nullptr;      // (a failed product: back to the template)
            return -2;
        }
    }
    e->direct = true;
    e->dev.pk_direct = e->pk_direct.p;       // every kernel of the chain takes its EngineDev from e->dev
    return 0;
}

int vmx_set_linear_spectra(vmx_engine* e, const double* pk_peak, const double* pk_smooth, const double* pk_full, int32_t nk)
{
    REQUIRE(e && e->finalized && pk_peak && pk_smooth && pk_full, "vmx_set_linear_spectra (after vmx_finalize)");
    drop_lane(e);
    REQUIRE(nk == e->nk, "linear spectra must live on the template's k grid");
    for (auto& p : e->pipes) REQUIRE(!p.odd_rel && !p.odd_asy, "the odd-multipole terms hold static splines of the template's spectra");
    HIP_OK(hipSetDevice(e->device));
    HIP_OK(hipStreamSynchronize(e->stream));
    const double* src[3] = {pk_peak, pk_smooth, pk_full};
    for (int i = 0; i < 3; ++i)
        HIP_OK(hipMemcpy(e->pklin.p + (size_t)i * e->nkp, src[i], (size_t)nk * sizeof(double), hipMemcpyHostToDevice));
    if (poly_basis_build(e)) return -2;
    return xi_sum_plan(e);
}

int vmx_item_set_marg_matrix(vmx_engine* e, int32_t item, const double* m, int32_t n_templates, int32_t n_masked)
{
    REQUIRE(e && !e->finalized && m, "vmx_item_set_marg_matrix (before vmx_finalize)");
    REQUIRE(item >= 0 && item < (int)e->items.size(), "item id");
    ItemHost* it = e->items[item];
    REQUIRE(it->has_mask && n_masked == it->dev.n_masked && n_templates > 0, "marginalisation matrix shape: [n_templates][n_masked]");
    HIP_OK(hipSetDevice(e->device));
    if (upload_padded(it->marg, m, n_templates, n_masked, it->dev.n_masked_pad)) return -2;
    it->n_templates = n_templates;
    return 0;
}

int vmx_marg_coeff(vmx_engine* e, int32_t item, double* out, int32_t B)
{
    REQUIRE(e && e->finalized && out, "vmx_marg_coeff");
    wait_lane(e);
    REQUIRE(item >= 0 && item < (int)e->items.size(), "item id");
    ItemHost* it = e->items[item];
    REQUIRE(it->n_templates > 0, "no marginalisation matrix was set for this item");
    REQUIRE(B > 0 && B == e->last_B, "vmx_marg_coeff reads the residuals of the last evaluation: B must be its batch size");
    REQUIRE(e->last_full, "the last evaluation took the quadratic chi2 form, which forms no residuals: evaluate with a model "
                          "output (or switch the form off with vmx_set_quadratic_form(e, NULL))");
    HIP_OK(hipSetDevice(e->device));
    const int ldo = vmx_pad(it->n_templates);
    if (it->marg_out.n < (size_t)e->max_batch * ldo && it->marg_out.alloc((size_t)e->max_batch * ldo, true)) return -2;
    if (vmx_matvec_device(e, it->marg.p, it->n_templates, it->dev.n_masked_pad, it->res.p, B, it->marg_out.p)) return -2;
    HIP_OK(hipStreamSynchronize(e->stream));
    HIP_OK(hipMemcpy2D(out, (size_t)it->n_templates * sizeof(double), it->marg_out.p, (size_t)ldo * sizeof(double),
                       (size_t)it->n_templates * sizeof(double), B, hipMemcpyDeviceToHost));
    return 0;
}

int vmx_marg_layout(vmx_engine* e, int32_t item, int32_t* offset, int32_t* count)
{
    REQUIRE(e && e->finalized, "vmx_marg_layout (after vmx_finalize)");
    REQUIRE(item >= -1 && item < (int)e->items.size(), "item id");
    int off = 0, total = 0;
    for (int q = 0; q < (int)e->items.size(); ++q) {
        if (q == item) off = total;
        total += e->items[q]->n_templates;
    }
    if (item >= 0) {
        if (offset) *offset = off;
        if (count) *count = e->items[item]->n_templates;
    }
    return total;
}

int vmx_marg_coeff_device(vmx_engine* e, const double* d_theta, int32_t B, double* d_out, int32_t ld_out, int32_t* d_status)
{
    REQUIRE(e && e->finalized && d_theta && d_out, "vmx_marg_coeff_device");
    REQUIRE(B > 0 && B <= e->max_batch, "batch exceeds max_batch");
    int total = 0;
    for (auto* it : e->items) total += it->n_templates;
    REQUIRE(total > 0, "no marginalisation matrix was set for any item");
    REQUIRE(ld_out >= total, "vmx_marg_coeff_device: ld_out holds fewer columns than vmx_marg_layout counts");
    HIP_OK(hipSetDevice(e->device));
    wait_lane(e);                       // (one lane: the request rides on the first lane's workspace)
    e->host_key_valid = false;
    bool quad = false;
    if (quad_ready(e, &quad, B)) return -2;
    // the slabs of the products: made at the first call, outside everything that is enqueued (the sizes never change)
    if (e->marg_slab_rows == 0) e->marg_slab_rows = std::max(e->max_batch, std::min(8 * e->max_batch, 4096));
    for (auto* it : e->items) {
        const size_t need = (size_t)e->marg_slab_rows * vmx_pad(it->n_templates);
        if (it->n_templates > 0 && it->mg_y.n < need) {
            HIP_OK(hipStreamSynchronize(e->stream));
            if (it->mg_y.alloc(need, true)) return -2;
        }
    }
    e->last_stream = e->stream;
    const vmx_engine::MargReq req{d_out, ld_out, d_status};
    struct Scope { vmx_engine* x; Scope(vmx_engine* x_, const vmx_engine::MargReq* r) : x(x_) { x->marg_req = r; } ~Scope() { x->marg_req = nullptr; } };
    Scope scope(e, &req);
    const int tab = (B >= 16 && e->n_xtab > 0) ? e->const_hint : 0;
    // eager launches: the first kernel reads the caller's walkers in place (behind a parameter transform: the engine's copy)
    const double* src = d_theta;
    if (!e->blind_scale.empty()) {
        HIP_OK(hipMemcpyAsync(e->theta.p, d_theta, (size_t)B * e->n_params * sizeof(double), hipMemcpyDeviceToDevice, e->stream));
        const int n = B * e->n_params;
        hipLaunchKernelGGL(k_theta_affine, dim3((n + 255) / 256), dim3(256), 0, e->stream, e->theta.p, e->d_blind.p, e->n_params, n);
        src = nullptr;
    }
    if (run_chain(e, B, tab, false, src, nullptr, nullptr, quad)) return -2;
    if (quad) return 0;
    // not served by the quadratic form (global covariance, multiplicative or non-polynomial post-distortion broadband, direct_pk,
    // the form switched off): the full chain has left its residuals, M is applied to them as vmx_marg_coeff does
    return marg_products(e, e->dev, B, false);
}

int vmx_get_mu_nodes(vmx_engine* e, double* mu, double* w, int32_t capacity)
{
    REQUIRE(e && e->nk > 0, "vmx_get_mu_nodes (after vmx_set_template)");
    if (!mu || !w || capacity < e->n_extra) return e->n_extra;
    HIP_OK(hipSetDevice(e->device));
    if (e->n_extra > 0) {
        HIP_OK(hipMemcpy(mu, e->mu.p + e->n_mu, (size_t)e->n_extra * sizeof(double), hipMemcpyDeviceToHost));
        HIP_OK(hipMemcpy(w, e->node_w.p, (size_t)e->n_extra * sizeof(double), hipMemcpyDeviceToHost));
    }
    return e->n_extra;
}

int vmx_set_mu_rule_box(vmx_engine* e, int32_t n, const int32_t* slots, const double* lo, const double* hi)
{
    REQUIRE(e && !e->finalized && n >= 0 && (n == 0 || (slots && lo && hi)), "vmx_set_mu_rule_box (before vmx_finalize)");
    e->rule_slot.clear(); e->rule_lo.clear(); e->rule_hi.clear();
    for (int i = 0; i < n; ++i) {
        REQUIRE(slots[i] >= 0 && lo[i] <= hi[i], "mu-rule box entry");
        e->rule_slot.push_back(slots[i]); e->rule_lo.push_back(lo[i]); e->rule_hi.push_back(hi[i]);
    }
    return 0;
}

int vmx_set_mu_quadrature(vmx_engine* e, int32_t node_rule)
{
    REQUIRE(e && e->finalized, "vmx_set_mu_quadrature (after vmx_finalize)");
    drop_lane(e);
    HIP_OK(hipSetDevice(e->device));
    HIP_OK(hipStreamSynchronize(e->stream));
    e->mu_nodes_on = node_rule != 0 && e->n_extra > 0;
    e->dev.k_node_max = e->mu_nodes_on ? e->k_node_max : 0.0;
    for (auto& g : e->graphs) (void)hipGraphExecDestroy(g.second);      // (captured graphs hold the previous setting)
    e->graphs.clear(); e->graph_route.clear();
    e->quad_lin_dirty = true;       // the reference point (x0', m0) is re-evaluated with the new rule; Q' and W do not depend on it
    return e->mu_nodes_on ? 1 : 0;
}

int vmx_set_static_poly(vmx_engine* e, int32_t enabled)
{
    REQUIRE(e && !e->finalized, "vmx_set_static_poly (before vmx_finalize)");
    e->static_poly = enabled != 0;
    return 0;
}

int vmx_set_quadratic_form_kind(vmx_engine* e, int32_t kind)
{
    REQUIRE(e && e->finalized && kind >= 0 && kind <= 2, "vmx_set_quadratic_form_kind: 0 (cheaper), 1 (Q'), 2 (factored), after vmx_finalize");
    if (kind != e->quad_kind) { e->quad_kind = kind; e->quad_mat_dirty = true; }
    return 0;
}

int vmx_set_quadratic_form(vmx_engine* e, const double* theta_ref)
{
    REQUIRE(e && e->finalized, "vmx_set_quadratic_form (after vmx_finalize)");
    drop_lane(e);
    e->theta_ref.clear();
    if (theta_ref) e->theta_ref.assign(theta_ref, theta_ref + e->n_params);
    e->quad_mat_dirty = true;       // (a new reference point: everything is rebuilt at the next chi2-only evaluation)
    return e->quad_eligible ? 1 : 0;
}

int vmx_set_constant_nl_hint(vmx_engine* e, int32_t enabled)
{
    REQUIRE(e, "vmx_set_constant_nl_hint");
    e->const_hint = enabled <= 0 ? 0 : enabled >= 2 ? 2 : 1;
    if (e->no_tab2 && e->const_hint > 1) e->const_hint = 1;
    return 0;
}

int vmx_sync(vmx_engine* e)
{
    REQUIRE(e, "vmx_sync");
    HIP_OK(hipSetDevice(e->device));
    HIP_OK(hipStreamSynchronize(e->stream));
    for (auto* l : e->lanes) HIP_OK(hipStreamSynchronize(l->stream));
    if (e->profiling) collect_spans(e);
    if (e->gemm_trace.p && e->gemm_trace_blocks && (getenv("VMX_GEMM_TRACE") || getenv("VMX_QUAD_TRACE"))) {
        std::vector<unsigned long long> h(4 * e->gemm_trace_blocks);
        HIP_OK(hipMemcpy(h.data(), e->gemm_trace.p, h.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
        const char* path = getenv("VMX_QUAD_TRACE") ? getenv("VMX_QUAD_TRACE") : getenv("VMX_GEMM_TRACE");
        if (FILE* f = fopen(path, "wb")) { fwrite(h.data(), sizeof(unsigned long long), h.size(), f); fclose(f); }
    }
    if (e->pk_trace.p && e->pk_trace_blocks) {
        std::vector<unsigned long long> h(4 * e->pk_trace_blocks);
        HIP_OK(hipMemcpy(h.data(), e->pk_trace.p, h.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
        if (FILE* f = fopen(getenv("VMX_PK_TRACE"), "wb")) { fwrite(h.data(), sizeof(unsigned long long), h.size(), f); fclose(f); }
    }
    return 0;
}

int vmx_eval(vmx_engine* e, const double* theta, int32_t B, double* chi2, double* model, int32_t* status)
{
    REQUIRE(e && e->finalized && theta, "vmx_eval");
    wait_lane(e);
    REQUIRE(B > 0 && B <= e->max_batch, "batch exceeds max_batch");
    const auto t_begin = std::chrono::steady_clock::now();
    HIP_OK(hipSetDevice(e->device));
    // small batches are latency-bound: the first kernel reads the walkers from the mapped pinned buffer and the last
    // one stores chi2 / status there, which removes three staging copies (~25 us of a ~100 us evaluation)
    const bool zero_copy = B <= 8 && B * ((int)e->pipes.size() + 1) <= 1024 && (size_t)B * e->n_params * sizeof(double) <= 48 * 1024 &&
                           e->dpin_theta && e->dpin_chi2 && e->dpin_status;
    bool quad = false;
    if (!model && quad_ready(e, &quad, B)) return -2;
    if (e->blind_scale.empty()) std::memcpy(e->pin_theta, theta, (size_t)B * e->n_params * sizeof(double));
    else        // parameter-level blinding, applied while staging (same expression as k_theta_affine)
        for (int b = 0; b < B; ++b)
            for (int i = 0; i < e->n_params; ++i) {
                const size_t o = (size_t)b * e->n_params + i;
                e->pin_theta[o] = e->blind_scale[i] == 1.0 ? theta[o] + e->blind_shift[i] : e->blind_scale[i] * theta[o] + e->blind_shift[i];
            }
    if (!zero_copy)
        HIP_OK(hipMemcpyAsync(e->theta.p, e->pin_theta, (size_t)B * e->n_params * sizeof(double), hipMemcpyHostToDevice, e->stream));
    // the D_NL * G table pays off once a batch shares its Arinyo parameters (checked here, on the host copy)
    int tab_mode = (e->n_xtab > 0) ? (e->no_tab2 ? 1 : 2) : 0;
    for (int b = 1; b < B && tab_mode; ++b) {
        for (int slot : e->const_slots)
            if (theta[(size_t)b * e->n_params + slot] != theta[slot]) { tab_mode = 0; break; }
        for (int slot : e->const_slots2)
            if (tab_mode == 2 && theta[(size_t)b * e->n_params + slot] != theta[slot]) { tab_mode = 1; break; }
    }
    // The tables outlive an evaluation (keyed on the shared parameters).  A small batch - a single walker of a minimiser or
    // sampler above all - runs against level-2 tables once those parameters have come twice in a row; a caller that varies
    // them from call to call keeps the per-walker loops (building tables costs more than one small evaluation).
    bool tables_current = false;
    {
        std::vector<double> cur;
        for (int slot : e->const_slots2) cur.push_back(e->pin_theta[slot]);      // (the transformed values: what the device sees)
        tables_current = tab_mode == 2 && e->host_key_valid && cur == e->host_key;
        if (B < 16 && tab_mode) {
            if (tab_mode == 2 && (tables_current || cur == e->pending_key)) tab_mode = 2;
            else { if (tab_mode == 2) e->pending_key = cur; tab_mode = 0; }
        }
        if (tab_mode == 2) { e->host_key = cur; e->host_key_valid = true; }
        else if (tab_mode == 1) e->host_key_valid = false;       // (the device tables now hold level 1)
    }
    const auto t_staged = std::chrono::steady_clock::now();
    // a single walker is latency-bound end to end: eager launches start the first kernel while the later ones are
    // still being enqueued, which a graph launch cannot (measured: 70 against 75 us per evaluation)
    e->host_reduce_items = 0;
    if (B == 1) {
        const bool by_value = zero_copy && e->n_params <= VMX_THETA_ARG_MAX;
        e->skip_xtab_once = tables_current;         // (the host knows the tables hold these parameters: no check launch)
        if (quad && by_value && e->pin_part && e->dpin_part) {
            // the slots the last products may fill (k_gemv1 MODE 2) start from a pattern no computation produces
            for (size_t q = 0; q < e->items.size() && q < VMX_MAX_GROUP; ++q) {
                const int blocks = gemv1_blocks(e->items[q]->dev.nq);
                for (int i = 0; i < blocks && i < 1024; ++i) std::memcpy(&e->pin_part[q * 1024 + i], &VMX_PART_SENTINEL, sizeof(double));
            }
            e->pin_status[0] = -1;
        }
        if (run_chain(e, B, tab_mode, zero_copy, nullptr, nullptr, nullptr, quad, by_value ? e->pin_theta : nullptr)) return -2;
    }
    else if (run_chain_cached(e, B, tab_mode, zero_copy, quad)) return -2;
    if (chi2 && !zero_copy) HIP_OK(hipMemcpyAsync(e->pin_chi2, e->chi2.p, (size_t)B * sizeof(double), hipMemcpyDeviceToHost, e->stream));
    if (status && !zero_copy) HIP_OK(hipMemcpyAsync(e->pin_status, e->status.p, (size_t)B * sizeof(int32_t), hipMemcpyDeviceToHost, e->stream));
    if (model) HIP_OK(hipMemcpyAsync(model, e->model.p, (size_t)B * e->model_size * sizeof(double), hipMemcpyDeviceToHost, e->stream));
    const auto t_enqueued = std::chrono::steady_clock::now();
    bool waited = false;
    if (e->host_reduce_items > 0) {
        // the chain ended with the streaming products of the quadratic form: add up what their blocks left here
        // (fixed order), the constants and the priors - vega_interface.py:316, :423-446
        // The wait is bounded by TIME (~200 us of spinning on the mapped words); when that runs out - a GPU shared with another
        // process, a profiler serialising the launches, a slow first launch - the stream is drained and the words are read
        // again: once the stream is empty they are guaranteed to be written, so only a sentinel that survives the drain is an error.
        double c = 0.0;
        bool complete = false;
        volatile int32_t* st_word = e->pin_status;
        const auto spin_until = std::chrono::steady_clock::now() + std::chrono::microseconds(200);
        for (int attempt = 0; attempt < 2 && !complete; ++attempt) {
            if (attempt == 1) HIP_OK(hipStreamSynchronize(e->stream));
            complete = true;
            c = 0.0;
            for (int q = 0; q < e->host_reduce_items && complete; ++q) {
                const volatile uint64_t* slot = (const volatile uint64_t*)(e->pin_part + (size_t)q * 1024);
                for (int i = 0; i < e->host_reduce_blocks[q] && complete; ++i) {
                    int spin = 0;
                    while (slot[i] == VMX_PART_SENTINEL && attempt == 0) {
                        if ((++spin & 255) == 0 && std::chrono::steady_clock::now() > spin_until) break;
                    }
                    uint64_t bits = slot[i];
                    if (bits == VMX_PART_SENTINEL) { complete = false; break; }
                    double v; std::memcpy(&v, &bits, sizeof(double));
                    c += v;
                }
            }
            for (int spin = 0; complete && *st_word == -1 && attempt == 0;) {
                if ((++spin & 255) == 0 && std::chrono::steady_clock::now() > spin_until) break;
            }
            if (*st_word == -1) complete = false;
        }
        if (!complete) { e->host_reduce_items = 0; return fail(-2, "single-walker chain: the device left a result slot unwritten after the stream drained"); }
        for (int q = 0; q < e->host_reduce_items; ++q) {
            const ItemHost* it = e->items[q];
            const int mock = (it->dev.mock_pool && e->h_mock_index[0] >= 0) ? e->h_mock_index[0] : -1;
            c += it->h_q_c0[mock >= 0 ? 1 + mock : 0];
        }
        for (size_t q = 0; q < e->prior_slot.size(); ++q) {
            const double dlt = e->pin_theta[e->prior_slot[q]] - e->prior_mean[q];
            c += dlt * dlt / (e->prior_sigma[q] * e->prior_sigma[q]);
        }
        int32_t st = *st_word;
        if (!(c == c) || c > 1e300 || c < -1e300) st |= VMX_STATUS_NONFINITE;
        e->pin_status[0] = st;
        e->pin_chi2[0] = st ? 1e100 : c;
        e->host_reduce_items = 0;
        waited = true;
    }
    if (!waited && B == 1 && zero_copy && !model && e->dpin_done && !e->profiling && e->n_params <= VMX_THETA_ARG_MAX) {
        // the last kernel of a single-walker chain publishes a sequence number after chi2 / status (system-scope fence):
        // the host waits on that word in mapped memory - a few microseconds sooner than the stream's completion signal
        const int64_t want = e->done_seq;
        volatile int64_t* word = e->pin_done;
        for (int64_t spin = 0; spin < (int64_t)1 << 26 && !waited; ++spin) waited = *word == want;
    }
    if (!waited && vmx_sync(e)) return -2;
    if (chi2) std::memcpy(chi2, e->pin_chi2, (size_t)B * sizeof(double));
    if (status) std::memcpy(status, e->pin_status, (size_t)B * sizeof(int32_t));
    if (e->trace_host) {
        const auto t_end = std::chrono::steady_clock::now();
        e->host_ns[0] += std::chrono::duration<double, std::nano>(t_staged - t_begin).count();
        e->host_ns[1] += std::chrono::duration<double, std::nano>(t_enqueued - t_staged).count();
        e->host_ns[2] += std::chrono::duration<double, std::nano>(t_end - t_enqueued).count();
        ++e->host_calls;
    }
    return 0;
}

int64_t vmx_debug_read(vmx_engine* e, int32_t what, int32_t index, double* out, int64_t capacity)
{
    if (!e || !e->finalized || !out || e->last_B <= 0) { fail(-1, "invalid argument: vmx_debug_read"); return -1; }
    if (hipSetDevice(e->device) != hipSuccess || hipStreamSynchronize(e->stream) != hipSuccess) { fail(-2, "hip sync"); return -2; }
    wait_lane(e);
    const int B = e->last_B;
    const double* src = nullptr; int64_t count = 0;
    if (what == 0) { src = e->pl.p; count = (int64_t)VMX_MAX_ELL * B * e->n_active * e->nkp; }
    else if (what == 1) {
        if (index < 0 || index >= (int)e->pipes.size()) { fail(-1, "invalid argument: pipeline index"); return -1; }
        if (!e->last_taps) { fail(-1, "the last evaluation (chi2 only, more than 8 walkers, no metal terms) did not store the per-pipeline bins: ask for a model"); return -1; }
        src = e->xi.p + e->pipes[index].xi_off; count = (int64_t)B * e->pipes[index].n_pad;
    } else if (what == 2) { src = e->coef.p; count = (int64_t)VMX_MAX_ELL * B * e->n_active * e->ncp; }
    else if (what == 3) {
        // correlation of metal `index` (global order of vmx_item_add_metal) after its metal matrix
        if (index < 0 || index >= (int)e->metals.size() || e->metals[index]->dev.mat_off < 0) { fail(-1, "invalid argument: metal without matrix"); return -1; }
        int n_model_pad = 0;
        for (auto* it : e->items) for (auto* m : it->metals) if (m == e->metals[index]) n_model_pad = it->dev.n_model_pad;
        src = e->xim.p + e->metals[index]->dev.xim_off; count = (int64_t)B * n_model_pad;
    }
    else if (what == 4) {
        // [0] the number of leading wavenumbers with a live P(k,mu) block in the last evaluation (the rest are exact zeros),
        // [1] the wavenumber up to which the mu sums take the node rule (0: plain loop), [2] nodes per wavenumber of that rule
        if (capacity < 3) { fail(-1, "invalid argument: capacity too small"); return -1; }
        int32_t live[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        if (hipMemcpy(live, e->k_live.p, 8 * sizeof(int32_t), hipMemcpyDeviceToHost) != hipSuccess) { fail(-2, "hipMemcpy"); return -2; }
        // (k_pk_tab2's tiles take the tier of their largest wavenumber: the mean over the wavenumbers on the rule)
        const int kt = e->last_tab_level >= 2 ? e->last_tab2_kt : 0;
        const bool tiered = kt > 0 && !(kt == 64 ? e->zmap64 : e->zmap16).empty();
        out[0] = live[0]; out[1] = e->dev.k_node_max;
        out[2] = vmx_plan::mu_mean_nodes(e->h_k.data(), e->nk, kt, live[1], tiered ? e->mu_tiers : 1, e->mu_tier);
        if (capacity >= 4) out[3] = live[1];
        if (capacity >= 5) out[4] = e->last_tab_level;
        if (capacity >= 7) { out[5] = live[2]; out[6] = live[3]; }
        if (capacity >= 9) out[8] = e->last_form;               // 0: full chain, 1: the quadratic form Q', 2: its factored form
        if (capacity >= 10) out[9] = e->last_route | e->route_setup;        // bins kernels launched (VMX_ROUTE_*)
        if (capacity >= 11) out[10] = e->last_fft_form;         // form of the FFTLog o spline product (VMX_FFT_*)
        if (capacity >= 12) out[11] = e->last_form == 1 && e->last_root ? 1 : 0;      // the Q' form's quadratic term ran over the trapezoidal root
        if (capacity >= 8) { out[7] = live[4]; return capacity >= 12 ? 12 : capacity >= 11 ? 11 : capacity >= 10 ? 10 : capacity >= 9 ? 9 : 8; }       // walkers that left the mu rule's box since vmx_finalize
        return capacity >= 7 ? 7 : capacity >= 5 ? 5 : capacity >= 4 ? 4 : 3;
    }
    else if (what == 5) {
        // the assembled pre-distortion vector of item `index`: the operand the last full-chain evaluation handed to the distortion
        // product (a single walker's fused product assembles it while staging it and leaves nothing behind)
        if (index < 0 || index >= (int)e->items.size()) { fail(-1, "invalid argument: item index"); return -1; }
        const ItemHost* it = e->items[index];
        const bool fused = B == 1 && it->has_dm && gemv1_applies(1, it->dev.n_model_pad) && !e->no_fuse;
        if (!e->last_full || fused) { fail(-1, "the last evaluation (chi2 only, or a single walker's fused distortion product) did not store the pre-distortion vector"); return -1; }
        src = it->vec.p; count = (int64_t)B * it->dev.n_model_pad;
    }
    else if (what == 6) { src = e->scal.p; count = (int64_t)B * (int64_t)e->pipes.size() * VMX_NS; }
    else if (what == 7) {
        static_assert(VMX_DEBUG_NS == VMX_NS, "vegamx.h states the row length of the scalars");
#define VMX_SCALAR_INDEX(name) S_##name,
        const int idx[] = {VMX_NS, VMX_DEBUG_SCALARS(VMX_SCALAR_INDEX)};
#undef VMX_SCALAR_INDEX
        const int64_t n = sizeof(idx) / sizeof(idx[0]);
        if (capacity < n) { fail(-1, "invalid argument: capacity too small"); return -1; }
        for (int64_t i = 0; i < n; ++i) out[i] = idx[i];
        return n;
    }
    else if (what == 8) {
        if (index < 0 || index >= (int)e->pipes.size()) { fail(-1, "invalid argument: pipeline index"); return -1; }
        const PipeDev& P = e->pipes[index];
        const double* arr[8] = {e->cr.p, e->crp.p, e->crt.p, e->cz.p, e->crelz.p, e->clnrelz.p, e->clnrelz2.p, e->cgrowth.p};
        if ((int64_t)8 * P.n > capacity) { fail(-1, "invalid argument: capacity too small"); return -1; }
        for (int a = 0; a < 8; ++a)
            if (hipMemcpy(out + (size_t)a * P.n, arr[a] + P.coord_off, (size_t)P.n * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess) { fail(-2, "hipMemcpy"); return -2; }
        return (int64_t)8 * P.n;
    }
    else if (what == 9) {
        if (index < 0 || index >= (int)e->pipes.size()) { fail(-1, "invalid argument: pipeline index"); return -1; }
        if (capacity < 30) { fail(-1, "invalid argument: capacity too small"); return -1; }
        const EngineDev& D = e->dev;
        const PipeDev& P = e->pipes[index];
        int64_t n = 0;
        out[n++] = D.n_coef; out[n++] = D.ncp; out[n++] = D.same_grid; out[n++] = D.extrapolate; out[n++] = e->n_active;       // (n_active: the columns of the coefficient buffer)
        for (int l = 0; l < VMX_MAX_ELL; ++l) { out[n++] = D.x0[l]; out[n++] = D.h[l]; out[n++] = D.inv_h[l]; out[n++] = D.xlast[l]; }
        out[n++] = P.col; out[n++] = P.n; out[n++] = P.n_pad; out[n++] = P.split_evol; out[n++] = P.poly_basis;
        out[n++] = P.poly_bins_off >= 0 ? 1 : 0; out[n++] = P.odd_x0; out[n++] = P.odd_h; out[n++] = P.odd_ncoef;
        return n;
    }
    else if (what == 10 || what == 11) {
        if (index < 0 || index >= (int)e->items.size()) { fail(-1, "invalid argument: item index"); return -1; }
        const ItemHost* it = e->items[index];
        if (e->last_full || e->last_form == 0 || !it->q_x.p || !it->q_x0.p) { fail(-1, "the last evaluation was not a chi2-only evaluation of the quadratic form: no x' - x0'"); return -1; }
        src = what == 10 ? it->q_x.p : it->q_x0.p; count = (what == 10 ? (int64_t)B : 1) * it->dev.nq_pad;
    }
    else if (what == 12) {
        if (index < 0 || index >= (int)e->pipes.size()) { fail(-1, "invalid argument: pipeline index"); return -1; }
        const PipeDev& P = e->pipes[index];
        if (P.poly_bins_off < 0 || !e->poly_bins.p) { fail(-1, "none: the pipeline has no static basis on its bins"); return -1; }
        src = e->poly_bins.p + P.poly_bins_off; count = (int64_t)3 * P.n_pad;
    }
    else if (what == 13 || what == 14 || what == 18 || what == 19) {
        // the groups of xi_sum_plan (13, 14: lean; 18, 19: static-coordinate): 13 / 18 = {groups, then of group `index`: members, n,
        // n_pad, presum, per member (pipeline, factor kind, factor index)}; 14 / 19 = its pre-summed array [B][n_pad] after an
        // evaluation that summed on the way
        const bool lean = what < 18, describe = what == 13 || what == 18;
        const int ng = (int)(lean ? e->lean_groups.size() : e->static_groups.size());
        if (describe && (index < 0 || index >= ng)) {
            if (capacity < 1) { fail(-1, "invalid argument: capacity too small"); return -1; }
            out[0] = ng;
            return 1;
        }
        if (index < 0 || index >= ng) { fail(-1, "invalid argument: group index"); return -1; }
        // (XiLeanGroup and XiStaticGroup differ in the length of their member array only)
        auto serve = [&](const auto& G) -> int64_t {
            if (describe) {
                if (capacity < 5 + 3 * G.n_members) { fail(-1, "invalid argument: capacity too small"); return -1; }
                int64_t n = 0;
                out[n++] = ng; out[n++] = G.n_members; out[n++] = G.n; out[n++] = G.n_pad; out[n++] = G.presum;
                for (int m = 0; m < G.n_members; ++m) { out[n++] = G.m[m].pipe; out[n++] = G.m[m].fkind; out[n++] = G.m[m].findex; }
                return n;
            }
            if (!(e->last_route & (lean ? VMX_ROUTE_GROUP : VMX_ROUTE_STATIC_GROUP))) { fail(-1, "the last evaluation did not sum its bins on the way: no group array"); return -1; }
            src = e->xi.p + G.out_off; count = (int64_t)B * G.n_pad;
            return 0;
        };
        const int64_t served = lean ? serve(e->lean_groups[index]) : serve(e->static_groups[index]);
        if (served != 0) return served;
    }
    else if (what == 15) { src = e->poly_coef.p; count = (int64_t)VMX_MAX_ELL * (int64_t)e->pk_static.size() * 3 * e->ncp; if (count == 0) { fail(-1, "none: no pipeline has a static coefficient basis"); return -1; } }
    else if (what == 16) {
        if (index < 0 || index >= (int)e->pipes.size()) { fail(-1, "invalid argument: pipeline index"); return -1; }
        const PipeDev& P = e->pipes[index];
        if (!P.odd_rel && !P.odd_asy) { fail(-1, "none: the pipeline has no odd-multipole terms"); return -1; }
        src = e->odd_coef.p + P.odd_off; count = (int64_t)4 * P.odd_ncoef;
    }
    else if (what == 17) { src = e->metal_bias.p; count = (int64_t)B * 3 * (int64_t)e->metals.size(); if (count == 0) { fail(-1, "none: no metal terms"); return -1; } }
    else if (what == 20 || what == 21) {
        // static tensors of the Q' form of item `index`: 20 = the trapezoidal root L [n_masked][nq_pad], 21 = Q' in half form [nq][nq_pad]
        if (index < 0 || index >= (int)e->items.size()) { fail(-1, "invalid argument: item index"); return -1; }
        const ItemHost* it = e->items[index];
        if (e->quad_factored || !it->q_mat.p || (what == 20 && (!e->quad_root || !it->q_root.p))) { fail(-1, "none: the engine holds no such tensor of the Q' form"); return -1; }
        src = what == 20 ? it->q_root.p : it->q_mat.p; count = (int64_t)(what == 20 ? it->dev.n_masked : it->dev.nq) * it->dev.nq_pad;
    }
    else { fail(-1, "invalid argument: what"); return -1; }
    if (count > capacity) { fail(-1, "invalid argument: capacity too small"); return -1; }
    if (hipMemcpy(out, src, (size_t)count * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess) { fail(-2, "hipMemcpy"); return -2; }
    return count;
}

// the device math functions elementwise (tests against extended precision: nothing else launches this)
__global__ __launch_bounds__(256) void k_debug_math(int which, const double* x, double* out, int64_t n)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double v = x[i];
    out[i] = which == 0 ? vmx_log(v) : which == 1 ? vmx_exp(v) : vmx_rsqrt(v);
}

int vmx_debug_math(vmx_engine* e, int32_t which, const double* x, int64_t n, double* out)
{
    REQUIRE(e && x && out && n > 0 && n <= ((int64_t)1 << 30) && which >= 0 && which <= 2, "vmx_debug_math");
    wait_lane(e);
    HIP_OK(hipSetDevice(e->device));
    DevBuf<double> dx, dy;
    if (dx.upload(x, (size_t)n) || dy.alloc((size_t)n, false)) return -2;
    hipLaunchKernelGGL(k_debug_math, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, e->stream, (int)which, dx.p, dy.p, n);
    HIP_OK(hipGetLastError());
    HIP_OK(hipStreamSynchronize(e->stream));
    HIP_OK(hipMemcpy(out, dy.p, (size_t)n * sizeof(double), hipMemcpyDeviceToHost));
    return 0;
}

int vmx_debug_poison_scratch(int on) { return g_poison_scratch.exchange(on ? 1 : 0); }

int vmx_matvec_device(vmx_engine* e, const double* d_A, int32_t rows, int32_t cols, const double* d_x, int32_t B,
                      double* d_y)
{
    REQUIRE(e && d_A && d_x && d_y, "vmx_matvec_device");
    wait_lane(e);
    REQUIRE(rows > 0 && cols > 0 && cols % VMX_PAD == 0, "cols (leading dimension) must be a multiple of 32, zero padded");
    REQUIRE(B > 0, "vmx_matvec_device: B > 0");
    HIP_OK(hipSetDevice(e->device));
    const int ldy = vmx_pad(rows);
    REQUIRE(B <= 8 || (gemm44_addressable(rows, cols) && gemm44_addressable(B, cols)), "vmx_matvec_device with more than 8 vectors: " GEMM44_LIMIT_MSG);
    if (B <= 8) {
        launch_product(e, KC_MATVEC, d_A, cols, 0, rows, cols, d_x, cols, 0, B, d_y, ldy, 0, 1, 0);
    } else {
        const size_t need = (size_t)8 * B * ldy;
        if (e->mv_part.n < need) HIP_OK(hipStreamSynchronize(e->stream));
        if (ensure(e->mv_part, need)) return -2;
        const int ns = launch_product(e, KC_MATVEC, d_A, cols, 0, rows, cols, d_x, cols, 0, B, e->mv_part.p, ldy, 0, 1, 8 * B);
        const int64_t count = (int64_t)B * ldy;
        hipLaunchKernelGGL(k_sum_slabs, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, e->cur, e->mv_part.p, d_y, count, ns);
    }
    HIP_OK(hipGetLastError());
    return 0;
}

int vmx_matmul_host(vmx_engine* e, const double* A, int32_t rows, int32_t cols, const double* X, int32_t B, double* Y)
{
    REQUIRE(e && A && X && Y && rows > 0 && cols > 0 && B > 0, "vmx_matmul_host");
    wait_lane(e);
    HIP_OK(hipSetDevice(e->device));
    HIP_OK(hipStreamSynchronize(e->stream));
    const int ld = vmx_pad(cols), ldy = vmx_pad(rows);
    DevBuf<double> dA, dX, dY;
    if (upload_padded(dA, A, rows, cols, ld) || upload_padded(dX, X, B, cols, ld) || dY.alloc((size_t)B * ldy, true)) return -2;
    if (vmx_matvec_device(e, dA.p, rows, ld, dX.p, B, dY.p)) return -2;
    HIP_OK(hipStreamSynchronize(e->stream));
    HIP_OK(hipMemcpy2D(Y, (size_t)rows * sizeof(double), dY.p, (size_t)ldy * sizeof(double), (size_t)rows * sizeof(double), B,
                       hipMemcpyDeviceToHost));
    return 0;
}

int vmx_set_profiling(vmx_engine* e, int32_t enabled)
{
    REQUIRE(e, "vmx_set_profiling");
    wait_lane(e);
    HIP_OK(hipSetDevice(e->device));
    HIP_OK(hipStreamSynchronize(e->stream));
    if (e->profiling) collect_spans(e);
    e->profiling = enabled != 0;
    e->prof_mask = 0xffffffffu;
    e->prof_stride = 1;
    // create the event pool up front so that no event is created between two launches of a timed run
    while (e->profiling && e->spans.size() < 96) {
        vmx_engine::Span s{};
        HIP_OK(hipEventCreate(&s.a));
        HIP_OK(hipEventCreate(&s.b));
        e->spans.push_back(s);
    }
    return 0;
}

int vmx_set_profiling_mask(vmx_engine* e, uint32_t kernel_class_mask)
{
    REQUIRE(e, "vmx_set_profiling_mask");
    wait_lane(e);
    HIP_OK(hipSetDevice(e->device));
    HIP_OK(hipStreamSynchronize(e->stream));
    if (e->profiling) collect_spans(e);
    // bits 28 - 31: sampling stride minus one (0: every launch of the selected classes is timed; n: every (n + 1)-th - an event
    // pair costs the queue a few microseconds, ~4 % of a B = 256 step when it sits around one kernel of every step)
    e->prof_stride = kernel_class_mask == 0xffffffffu ? 1 : 1 + (int)(kernel_class_mask >> 28);
    e->prof_mask = kernel_class_mask == 0xffffffffu ? kernel_class_mask : (kernel_class_mask & 0x0fffffffu);
    for (auto& c : e->prof_count) c = 0;
    return 0;
}

int vmx_get_timings(vmx_engine* e, double* ms, int64_t* launches, int32_t reset)
{
    REQUIRE(e && ms && launches, "vmx_get_timings");
    wait_lane(e);
    HIP_OK(hipSetDevice(e->device));
    HIP_OK(hipStreamSynchronize(e->stream));
    collect_spans(e);
    for (int i = 0; i < VMX_N_KERNELS; ++i) { ms[i] = e->ms[i]; launches[i] = e->launches[i]; }
    if (reset) for (int i = 0; i < VMX_N_KERNELS; ++i) { e->ms[i] = 0; e->launches[i] = 0; }
    return 0;
}

const char* vmx_kernel_name(int32_t kc) { return (kc >= 0 && kc < VMX_N_KERNELS) ? kKernelNames[kc] : ""; }

}  // extern "C"
