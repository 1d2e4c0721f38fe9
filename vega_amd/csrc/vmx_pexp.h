// pexp: the project's pinned exponential, from separately rounded operations (the device, a host build and NumPy give the same
// bits: vega_amd/smc.py pexp).  It decides the SMC sampler (vmx_smc.h, whose namespace it keeps) and moves the adaptive temperature
// ladders of the ensemble sampler (vmx_ensemble.h, the fourth part), which is why it has a file of its own: vmx_ensemble.h includes
// it after VMX_HD and VMX_NO_CONTRACT are defined, and every other header gets it from there.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>

namespace vmx_smc {

constexpr double INV_LN2 = 1.44269504088896338700e+00;
constexpr double LN2_HI = 6.93147180369123816490e-01;      // (the upper 32 bits of ln 2: k LN2_HI is exact for |k| < 2^20)
constexpr double LN2_LO = 1.90821492927058770002e-10;

VMX_HD inline double pow2(int k)            // 2^k, -1022 <= k <= 1023
{
    const uint64_t b = (uint64_t)(k + 1023) << 52;
    double d;
    memcpy(&d, &b, sizeof d);
    return d;
}

VMX_HD inline double horner(double p, double r, double c)
{
    VMX_NO_CONTRACT
    const double m = p * r;
    return m + c;
}

VMX_HD inline double pexp(double x)
{
    VMX_NO_CONTRACT
    if (x != x) return x;
    if (x > 709.0) return INFINITY;         // (no caller asks for a positive argument)
    if (x < -745.2) return 0.0;
    const double s = x * INV_LN2;
    const double kf = floor(s + 0.5);
    const double h = kf * LN2_HI;
    double r = x - h;
    const double l = kf * LN2_LO;
    r = r - l;
    double p = 1.0 / 6227020800.0;
    p = horner(p, r, 1.0 / 479001600.0);
    p = horner(p, r, 1.0 / 39916800.0);
    p = horner(p, r, 1.0 / 3628800.0);
    p = horner(p, r, 1.0 / 362880.0);
    p = horner(p, r, 1.0 / 40320.0);
    p = horner(p, r, 1.0 / 5040.0);
    p = horner(p, r, 1.0 / 720.0);
    p = horner(p, r, 1.0 / 120.0);
    p = horner(p, r, 1.0 / 24.0);
    p = horner(p, r, 1.0 / 6.0);
    p = horner(p, r, 0.5);
    p = horner(p, r, 1.0);
    p = horner(p, r, 1.0);
    const int k = (int)kf;
    if (k >= -1022) return p * pow2(k);
    const double q = p * pow2(k + 1000);    // (exact; the product below rounds once, into the subnormals)
    return q * 0x1.0p-1000;
}

}  // namespace vmx_smc
