// csrc/dev_exp.h — the device library's double exp() restated for arguments that are converted floats: what the float path of the default NDT
// derivative kernels (ndt_derivatives.hip pair_float_c, GLIBC = false) weighs every (point, voxel) pair with.
//
// Operation for operation the routine the compiler inlines for exp(double) on gfx950 (constants read from the code object):
//   n = rint(x / ln 2);  t = x - n ln2_hi - n ln2_lo (two fma);  p = Horner of degree 11 in t (nine fma on ten coefficients, then two fma ..., 1.0);
//   ldexp(p, int(n));  x > 1024 -> +inf;  x < -1075 -> 0
// so the double it returns has the bits of exp(x).  tests/test_gpu_exp_float_args.py holds that for all 2^32 arguments the kernels can form
// (mrgfe_dbg_exp_float_args sweeps them on the device).
//
// Why restate it: inlined, each Horner step comes out as v_mov_b64 + v_fmac_f64 — the two-operand form overwrites its addend, and the addend is a
// coefficient that sits in a VGPR pair which must survive the loop.  Nine moves per pair and 18 resident VGPRs in a kernel that is bound by VALU
// issue and capped at 168 registers.  Here a step is ONE three-operand v_fma_f64 whose coefficient is a scalar operand (an SGPR pair, set by two
// s_mov_b32 on the scalar unit): no move, no vector register.  A VALU instruction of gfx9 reads at most one scalar operand, so the first step,
// which multiplies by one constant and adds another, stays as the compiler lays it out (one of the two in a VGPR pair): eight of the nine go.
#pragma once

#include <hip/hip_runtime.h>

namespace mrgfe {

// a * b + c with c wave-uniform, as one v_fma_f64 that reads c from scalar registers
__device__ __forceinline__ double fma_scalar_addend(double a, double b, double c)
{
    double r;
    asm("v_fma_f64 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "s"(c));
    return r;
}

__device__ __forceinline__ double exp_float_arg(double x)
{
    const double n = __builtin_rint(x * 0x1.71547652b82fep+0);
    double t = __builtin_fma(n, -0x1.62e42fefa39efp-1, x);
    t = __builtin_fma(n, -0x1.abc9e3b39803fp-56, t);
    double p = __builtin_fma(t, 0x1.ade156a5dcb37p-26, 0x1.28af3fca7ab0cp-22);  // two constants, one scalar operand: left to the compiler
    p = fma_scalar_addend(t, p, 0x1.71dee623fde64p-19);
    p = fma_scalar_addend(t, p, 0x1.a01997c89e6b0p-16);
    p = fma_scalar_addend(t, p, 0x1.a01a014761f6ep-13);
    p = fma_scalar_addend(t, p, 0x1.6c16c1852b7b0p-10);
    p = fma_scalar_addend(t, p, 0x1.1111111122322p-7);
    p = fma_scalar_addend(t, p, 0x1.55555555502a1p-5);
    p = fma_scalar_addend(t, p, 0x1.5555555555511p-3);
    p = fma_scalar_addend(t, p, 0x1.000000000000bp-1);
    p = __builtin_fma(t, p, 1.0);
    p = __builtin_fma(t, p, 1.0);
    double z = __builtin_ldexp(p, static_cast<int>(n));
    z = x > 1024.0 ? __builtin_inf() : z;
    z = x < -1075.0 ? 0.0 : z;
    return z;
}

}  // namespace mrgfe
