// One-direction forward mode for the DALTON gradient kernels (dalton_grad_kernels.hpp): the device
// counterpart of jax.jvp through ode_fun and through the jax.jacfwd(ode_fun) of interrogate_kramer (src/rodeo/interrogate.py:76).
//
// Tangent: a value and ONE derivative, along the direction the lane carries -- of the predicted mean (all blocks) and of the
// parameters.  TJet<N>: a dual number with N partials whose value and partials are Tangents, so that one evaluation of a
// scalar-generic right-hand side
//     template <class T, class TH, int P> static void rhs_generic(const T (&X)[D][P], double t, const TH (&th)[NTHETA], T (&out)[D]);
// with T = TJet<N> (the N leading components of one block seeded) and TH = Tangent yields, for that block,
//     out.v.v = f     out.v.d = f.      out.d[j].v = J_j = d f / d X[b][j]     out.d[j].d = J._j ,
// the directional derivative of the Jacobian: second derivatives of f in one direction.  With T = TH = Tangent it yields f and f.
// alone (interrogate_rodeo / interrogate_schober).
//
// The operator set is dual.hpp's: mixed overloads with a plain double (and, for TJet, with a Tangent: the parameters) that keep
// the structural zeros of a constant out of the arithmetic, and the elementary functions of rodeo_amd.trace._FUNCS.
//
// RTC-safe, and plain C++ as well (dual2.hpp's rule): without a HIP compiler the functions are ordinary inline functions, which
// is how the host test differentiates a few compositions against their analytic derivatives.
#pragma once
#if defined(__HIPCC_RTC__)
#define RK_TG_FN __device__ __forceinline__
#elif defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define RK_TG_FN __host__ __device__ __forceinline__
#else
#include <cmath>
#define RK_TG_FN inline
#endif

namespace rk {

struct Tangent {
    double v, d;
    RK_TG_FN Tangent() : v(0.0), d(0.0) {}
    RK_TG_FN Tangent(double x) : v(x), d(0.0) {}
    RK_TG_FN Tangent(double x, double dx) : v(x), d(dx) {}
};

RK_TG_FN Tangent operator+(const Tangent& a, const Tangent& b) { return Tangent(a.v + b.v, a.d + b.d); }
RK_TG_FN Tangent operator-(const Tangent& a, const Tangent& b) { return Tangent(a.v - b.v, a.d - b.d); }
RK_TG_FN Tangent operator*(const Tangent& a, const Tangent& b) { return Tangent(a.v * b.v, ::fma(a.d, b.v, a.v * b.d)); }
RK_TG_FN Tangent operator/(const Tangent& a, const Tangent& b) {
    const double q = a.v / b.v;
    return Tangent(q, (a.d - q * b.d) / b.v);
}
RK_TG_FN Tangent operator-(const Tangent& a) { return Tangent(-a.v, -a.d); }
RK_TG_FN Tangent operator+(const Tangent& a, double b) { return Tangent(a.v + b, a.d); }
RK_TG_FN Tangent operator+(double a, const Tangent& b) { return Tangent(a + b.v, b.d); }
RK_TG_FN Tangent operator-(const Tangent& a, double b) { return Tangent(a.v - b, a.d); }
RK_TG_FN Tangent operator-(double a, const Tangent& b) { return Tangent(a - b.v, -b.d); }
RK_TG_FN Tangent operator*(const Tangent& a, double b) { return Tangent(a.v * b, a.d * b); }
RK_TG_FN Tangent operator*(double a, const Tangent& b) { return Tangent(a * b.v, a * b.d); }
RK_TG_FN Tangent operator/(const Tangent& a, double b) { return Tangent(a.v / b, a.d / b); }
RK_TG_FN Tangent operator/(double a, const Tangent& b) {
    const double q = a / b.v;
    return Tangent(q, -q / b.v * b.d);
}

// f(a) from f and f' at a.v (dual.hpp's table)
#define RK_TG_FUN(NAME, VEXPR, DFAC)                 \
    RK_TG_FN Tangent NAME(const Tangent& a) {        \
        Tangent r;                                   \
        r.v = VEXPR;                                 \
        r.d = (DFAC) * a.d;                          \
        return r;                                    \
    }
RK_TG_FUN(sin, ::sin(a.v), ::cos(a.v))
RK_TG_FUN(cos, ::cos(a.v), -::sin(a.v))
RK_TG_FUN(exp, ::exp(a.v), r.v)
RK_TG_FUN(log, ::log(a.v), 1.0 / a.v)
RK_TG_FUN(sqrt, ::sqrt(a.v), 0.5 / r.v)
RK_TG_FUN(tanh, ::tanh(a.v), 1.0 - r.v * r.v)
RK_TG_FUN(tan, ::tan(a.v), 1.0 + r.v * r.v)
RK_TG_FUN(sinh, ::sinh(a.v), ::cosh(a.v))
RK_TG_FUN(cosh, ::cosh(a.v), ::sinh(a.v))
RK_TG_FUN(atan, ::atan(a.v), 1.0 / (1.0 + a.v * a.v))
RK_TG_FUN(asin, ::asin(a.v), 1.0 / ::sqrt(1.0 - a.v * a.v))
RK_TG_FUN(acos, ::acos(a.v), -1.0 / ::sqrt(1.0 - a.v * a.v))
RK_TG_FUN(log1p, ::log1p(a.v), 1.0 / (1.0 + a.v))
RK_TG_FUN(expm1, ::expm1(a.v), r.v + 1.0)
#undef RK_TG_FUN

// ---- the Jacobian dual: N partials, every component a Tangent ---------------------------------------------------------------
template <int N>
struct TJet {
    Tangent v;
    Tangent d[N];
    RK_TG_FN TJet() {}
    RK_TG_FN TJet(double x) : v(x) {}
    RK_TG_FN TJet(const Tangent& x) : v(x) {}
};

template <int N>
RK_TG_FN TJet<N> operator+(const TJet<N>& a, const TJet<N>& b) {
    TJet<N> r;
    r.v = a.v + b.v;
#pragma unroll
    for (int i = 0; i < N; ++i) r.d[i] = a.d[i] + b.d[i];
    return r;
}
template <int N>
RK_TG_FN TJet<N> operator-(const TJet<N>& a, const TJet<N>& b) {
    TJet<N> r;
    r.v = a.v - b.v;
#pragma unroll
    for (int i = 0; i < N; ++i) r.d[i] = a.d[i] - b.d[i];
    return r;
}
template <int N>
RK_TG_FN TJet<N> operator*(const TJet<N>& a, const TJet<N>& b) {
    TJet<N> r;
    r.v = a.v * b.v;
#pragma unroll
    for (int i = 0; i < N; ++i) r.d[i] = a.d[i] * b.v + a.v * b.d[i];
    return r;
}
template <int N>
RK_TG_FN TJet<N> operator/(const TJet<N>& a, const TJet<N>& b) {
    TJet<N> r;
    r.v = a.v / b.v;
#pragma unroll
    for (int i = 0; i < N; ++i) r.d[i] = (a.d[i] - r.v * b.d[i]) / b.v;
    return r;
}
template <int N>
RK_TG_FN TJet<N> operator-(const TJet<N>& a) {
    TJet<N> r;
    r.v = -a.v;
#pragma unroll
    for (int i = 0; i < N; ++i) r.d[i] = -a.d[i];
    return r;
}

// mixed operations with a scalar S whose partials are structural zeros: a plain double (a constant) or a Tangent (a parameter)
#define RK_TJET_MIXED(S)                                                                                          \
    template <int N>                                                                                              \
    RK_TG_FN TJet<N> operator+(const TJet<N>& a, S b) { TJet<N> r = a; r.v = a.v + b; return r; }                 \
    template <int N>                                                                                              \
    RK_TG_FN TJet<N> operator+(S a, const TJet<N>& b) { TJet<N> r = b; r.v = a + b.v; return r; }                 \
    template <int N>                                                                                              \
    RK_TG_FN TJet<N> operator-(const TJet<N>& a, S b) { TJet<N> r = a; r.v = a.v - b; return r; }                 \
    template <int N>                                                                                              \
    RK_TG_FN TJet<N> operator-(S a, const TJet<N>& b) { TJet<N> r = -b; r.v = a - b.v; return r; }                \
    template <int N>                                                                                              \
    RK_TG_FN TJet<N> operator*(const TJet<N>& a, S b) {                                                           \
        TJet<N> r;                                                                                                \
        r.v = a.v * b;                                                                                            \
        _Pragma("unroll") for (int i = 0; i < N; ++i) r.d[i] = a.d[i] * b;                                        \
        return r;                                                                                                 \
    }                                                                                                             \
    template <int N>                                                                                              \
    RK_TG_FN TJet<N> operator*(S a, const TJet<N>& b) { return b * a; }                                           \
    template <int N>                                                                                              \
    RK_TG_FN TJet<N> operator/(const TJet<N>& a, S b) {                                                           \
        TJet<N> r;                                                                                                \
        r.v = a.v / b;                                                                                            \
        _Pragma("unroll") for (int i = 0; i < N; ++i) r.d[i] = a.d[i] / b;                                        \
        return r;                                                                                                 \
    }                                                                                                             \
    template <int N>                                                                                              \
    RK_TG_FN TJet<N> operator/(S a, const TJet<N>& b) {                                                           \
        TJet<N> r;                                                                                                \
        r.v = a / b.v;                                                                                            \
        const Tangent fac = -r.v / b.v;                                                                           \
        _Pragma("unroll") for (int i = 0; i < N; ++i) r.d[i] = fac * b.d[i];                                      \
        return r;                                                                                                 \
    }
RK_TJET_MIXED(double)
RK_TJET_MIXED(const Tangent&)
#undef RK_TJET_MIXED

// f(a): value f(a.v) and partials f'(a.v) a.d[i], with f and f' evaluated on Tangents (x = a.v, f0 = f(x))
#define RK_TJET_FUN(NAME, DFAC)                                                  \
    template <int N>                                                             \
    RK_TG_FN TJet<N> NAME(const TJet<N>& a) {                                    \
        const Tangent x = a.v, f0 = NAME(x);                                     \
        (void)x;                                                                 \
        const Tangent fac = DFAC;                                                \
        TJet<N> r;                                                               \
        r.v = f0;                                                                \
        _Pragma("unroll") for (int i = 0; i < N; ++i) r.d[i] = fac * a.d[i];     \
        return r;                                                                \
    }
RK_TJET_FUN(sin, cos(x))
RK_TJET_FUN(cos, -sin(x))
RK_TJET_FUN(exp, f0)
RK_TJET_FUN(log, 1.0 / x)
RK_TJET_FUN(sqrt, 0.5 / f0)
RK_TJET_FUN(tanh, 1.0 - f0 * f0)
RK_TJET_FUN(tan, 1.0 + f0 * f0)
RK_TJET_FUN(sinh, cosh(x))
RK_TJET_FUN(cosh, sinh(x))
RK_TJET_FUN(atan, 1.0 / (1.0 + x * x))
RK_TJET_FUN(asin, 1.0 / sqrt(1.0 - x * x))
RK_TJET_FUN(acos, -1.0 / sqrt(1.0 - x * x))
RK_TJET_FUN(log1p, 1.0 / (1.0 + x))
RK_TJET_FUN(expm1, f0 + 1.0)
#undef RK_TJET_FUN

}  // namespace rk
