// The affine-invariant ensemble sampler (Goodman & Weare 2010, the "stretch move" of emcee), pinned decision for decision.
//
// The walker loop runs where the walkers are (vmx_ensemble_run, vegamx.hip: one small kernel per half-step decides the half that
// was just evaluated and proposes the next one); vega_amd/ensemble.py restates every expression below in NumPy (the `python`
// driver) and tests/helpers/ensemble_driver.cpp compiles this header with g++ so that tests/test_ensemble_host.py can hold the two
// against each other bit for bit.  No HIP type, no heap.
//
//   random numbers   Random123 Philox4x64-10 (NumPy's np.random.Philox): one block per (walker-in-half i, global step s, half h),
//                    counter (i, s, h, 0) (word 0 least significant), key (seed, stream).  The block equals
//                    np.random.Philox(key=[seed, stream], counter=(c - 1) mod 2**256).random_raw(4) (NumPy increments before it
//                    encrypts).  A uniform double from a word x: (x >> 11) 2**-53.
//   halves           walkers [0, W/2) and [W/2, W); step s updates half 0 against half 1, then half 1 against the updated half 0
//                    (emcee with randomize_split=False).
//   proposal         walker k of the active half, block words x0, x1, x2: partner j = ((x0 >> 32) (W/2)) >> 32 of the other
//                    half; t = (a - 1) u(x1); t = t + 1; z = t t; z = z / a; per sampled column y = c - (c - s) z (c the partner's
//                    position, s the walker's own); factor = (n - 1) log(z).
//   decision         accept iff every y lies in [lo, hi], the engine's status is 0 and chi2 < 1e99, and
//                    (factor + lnL_new) - lnL_old > log(u(x2)), with lnL = log_norm - 0.5 chi2.
//
// Every expression is the separately rounded IEEE operations written above: device code contracts a * b + c into an FMA by
// default, so the functions below switch contraction off (clang) - g++ has no FMA in the baseline x86-64 ISA and is left alone.
#pragma once
#include <cmath>
#include <cstdint>

#ifndef VMX_HD
#if defined(__HIPCC__)
#define VMX_HD __host__ __device__
#else
#define VMX_HD
#endif
#endif

#if defined(__clang__)
#define VMX_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define VMX_NO_CONTRACT
#endif

namespace vmx_ens {

struct Block { uint64_t w[4]; };

VMX_HD inline void mulhilo(uint64_t a, uint64_t b, uint64_t& hi, uint64_t& lo)
{
#if defined(__HIP_DEVICE_COMPILE__)
    lo = a * b;
    hi = __umul64hi(a, b);
#else
    const unsigned __int128 p = (unsigned __int128)a * b;
    lo = (uint64_t)p;
    hi = (uint64_t)(p >> 64);
#endif
}

// Philox4x64 with 10 rounds (Random123 philox4x64_R(10, ctr, key))
VMX_HD inline Block philox4x64_10(uint64_t c0, uint64_t c1, uint64_t c2, uint64_t c3, uint64_t k0, uint64_t k1)
{
    constexpr uint64_t M0 = 0xD2E7470EE14C6C93ull, M1 = 0xCA5A826395121157ull;
    constexpr uint64_t W0 = 0x9E3779B97F4A7C15ull, W1 = 0xBB67AE8584CAA73Bull;
    for (int r = 0; r < 10; ++r) {
        if (r > 0) { k0 += W0; k1 += W1; }
        uint64_t hi0, lo0, hi1, lo1;
        mulhilo(M0, c0, hi0, lo0);
        mulhilo(M1, c2, hi1, lo1);
        const uint64_t n0 = hi1 ^ c1 ^ k0, n2 = hi0 ^ c3 ^ k1;
        c0 = n0; c1 = lo1; c2 = n2; c3 = lo0;
    }
    return Block{{c0, c1, c2, c3}};
}

// the block of walker-in-half i at global step s, half h
VMX_HD inline Block step_block(int64_t i, int64_t s, int h, uint64_t seed, uint64_t stream)
{
    return philox4x64_10((uint64_t)i, (uint64_t)s, (uint64_t)h, 0, seed, stream);
}

VMX_HD inline double u01(uint64_t x) { return (double)(x >> 11) * 0x1.0p-53; }

// partner index in the complementary half of `half` walkers
VMX_HD inline int64_t partner(uint64_t x0, int64_t half) { return (int64_t)(((x0 >> 32) * (uint64_t)half) >> 32); }

VMX_HD inline double stretch_z(double a, uint64_t x1)
{
    VMX_NO_CONTRACT
    double t = (a - 1.0) * u01(x1);
    t = t + 1.0;
    double z = t * t;
    z = z / a;
    return z;
}

// one sampled column of the proposal: c the partner's position, s the walker's own
VMX_HD inline double propose(double c, double s, double z)
{
    VMX_NO_CONTRACT
    const double d = (c - s) * z;
    return c - d;
}

VMX_HD inline double log_factor(int n, double z)
{
    VMX_NO_CONTRACT
    return (double)(n - 1) * log(z);
}

VMX_HD inline double log_lik(double log_norm, double chi2)
{
    VMX_NO_CONTRACT
    const double h = 0.5 * chi2;
    return log_norm - h;
}

VMX_HD inline bool model_ok(int32_t status, double chi2) { return status == 0 && chi2 < 1e99; }

// the Metropolis decision of a proposal (inside: every column in its box; ok: model_ok)
VMX_HD inline bool accept(bool inside, bool ok, double factor, double lnl_new, double lnl_old, uint64_t x2)
{
    VMX_NO_CONTRACT
    if (!inside || !ok) return false;
    const double lhs = (factor + lnl_new) - lnl_old;
    return lhs > log(u01(x2));
}

}  // namespace vmx_ens
