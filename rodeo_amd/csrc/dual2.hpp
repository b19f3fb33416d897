// Second-order forward mode for user-supplied observation log-likelihoods: the device counterpart of the
// jax.jacrev / jax.jacfwd(jax.jacrev) calls of src/rodeo/inference/dalton.py:614-617, restricted to what DALTON keeps --
// the gradient and the diagonal Hessian block of ONE block's active components (dalton.py:618).
//
// Dual2<K>: value, K first derivatives g[i] and the K (K + 1) / 2 second derivatives h[idx(i, j)], i <= j.  The operator
// set is dual.hpp's: mixed double / dual overloads that keep the structural zeros of a constant out of the arithmetic, and
// the elementary functions of rodeo_amd.trace._FUNCS through one chain rule.  lgamma exists for plain doubles only (there
// is no digamma / trigamma here; the tracer refuses gammaln of a state-dependent value).
//
// RTC-safe, and plain C++ as well: without a HIP compiler the functions are ordinary inline functions, which is how the
// host test differentiates a few compositions against their analytic derivatives.
#pragma once
#if defined(__HIPCC_RTC__)
#define RK_D2_FN __device__ __forceinline__
#elif defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define RK_D2_FN __host__ __device__ __forceinline__
#else
#include <cmath>
#define RK_D2_FN inline
#endif

namespace rk {

template <int K>
struct Dual2 {
    static constexpr int NH = K * (K + 1) / 2;
    double v;
    double g[K];
    double h[NH];
    // packed index of (i, j), i <= j
    RK_D2_FN static constexpr int idx(int i, int j) { return i * K - i * (i - 1) / 2 + (j - i); }
    RK_D2_FN Dual2() : v(0.0) {
        for (int i = 0; i < K; ++i) g[i] = 0.0;
        for (int i = 0; i < NH; ++i) h[i] = 0.0;
    }
    RK_D2_FN Dual2(double x) : v(x) {
        for (int i = 0; i < K; ++i) g[i] = 0.0;
        for (int i = 0; i < NH; ++i) h[i] = 0.0;
    }
    RK_D2_FN double hess(int i, int j) const { return i <= j ? h[idx(i, j)] : h[idx(j, i)]; }
};

// f(a) from f, f', f'' at a.v:  g = f' a.g ;  h_ij = f' a.h_ij + f'' a.g_i a.g_j
template <int K>
RK_D2_FN Dual2<K> d2_chain(const Dual2<K>& a, double f0, double f1, double f2) {
    Dual2<K> r;
    r.v = f0;
#pragma unroll
    for (int i = 0; i < K; ++i) r.g[i] = f1 * a.g[i];
#pragma unroll
    for (int i = 0; i < K; ++i)
#pragma unroll
        for (int j = i; j < K; ++j) r.h[Dual2<K>::idx(i, j)] = ::fma(f2 * a.g[i], a.g[j], f1 * a.h[Dual2<K>::idx(i, j)]);
    return r;
}

template <int K>
RK_D2_FN Dual2<K> operator+(const Dual2<K>& a, const Dual2<K>& b) {
    Dual2<K> r;
    r.v = a.v + b.v;
#pragma unroll
    for (int i = 0; i < K; ++i) r.g[i] = a.g[i] + b.g[i];
#pragma unroll
    for (int i = 0; i < Dual2<K>::NH; ++i) r.h[i] = a.h[i] + b.h[i];
    return r;
}
template <int K>
RK_D2_FN Dual2<K> operator-(const Dual2<K>& a, const Dual2<K>& b) {
    Dual2<K> r;
    r.v = a.v - b.v;
#pragma unroll
    for (int i = 0; i < K; ++i) r.g[i] = a.g[i] - b.g[i];
#pragma unroll
    for (int i = 0; i < Dual2<K>::NH; ++i) r.h[i] = a.h[i] - b.h[i];
    return r;
}
// (a b)_ij = a_ij b + a b_ij + a_i b_j + a_j b_i
template <int K>
RK_D2_FN Dual2<K> operator*(const Dual2<K>& a, const Dual2<K>& b) {
    Dual2<K> r;
    r.v = a.v * b.v;
#pragma unroll
    for (int i = 0; i < K; ++i) r.g[i] = ::fma(a.g[i], b.v, a.v * b.g[i]);
#pragma unroll
    for (int i = 0; i < K; ++i)
#pragma unroll
        for (int j = i; j < K; ++j) {
            const int e = Dual2<K>::idx(i, j);
            r.h[e] = ::fma(a.h[e], b.v, ::fma(a.v, b.h[e], ::fma(a.g[i], b.g[j], a.g[j] * b.g[i])));
        }
    return r;
}
template <int K>
RK_D2_FN Dual2<K> operator-(const Dual2<K>& a) {
    Dual2<K> r;
    r.v = -a.v;
#pragma unroll
    for (int i = 0; i < K; ++i) r.g[i] = -a.g[i];
#pragma unroll
    for (int i = 0; i < Dual2<K>::NH; ++i) r.h[i] = -a.h[i];
    return r;
}
// 1 / b:  f' = -1 / b^2 ,  f'' = 2 / b^3
template <int K>
RK_D2_FN Dual2<K> d2_recip(const Dual2<K>& b) {
    const double y = 1.0 / b.v;
    return d2_chain<K>(b, y, -y * y, 2.0 * y * y * y);
}
template <int K>
RK_D2_FN Dual2<K> operator/(const Dual2<K>& a, const Dual2<K>& b) { return a * d2_recip<K>(b); }

// mixed operations with a plain double (its derivatives are structural zeros)
template <int K>
RK_D2_FN Dual2<K> operator+(const Dual2<K>& a, double b) { Dual2<K> r = a; r.v = a.v + b; return r; }
template <int K>
RK_D2_FN Dual2<K> operator+(double a, const Dual2<K>& b) { Dual2<K> r = b; r.v = a + b.v; return r; }
template <int K>
RK_D2_FN Dual2<K> operator-(const Dual2<K>& a, double b) { Dual2<K> r = a; r.v = a.v - b; return r; }
template <int K>
RK_D2_FN Dual2<K> operator-(double a, const Dual2<K>& b) { Dual2<K> r = -b; r.v = a - b.v; return r; }
template <int K>
RK_D2_FN Dual2<K> operator*(const Dual2<K>& a, double b) {
    Dual2<K> r;
    r.v = a.v * b;
#pragma unroll
    for (int i = 0; i < K; ++i) r.g[i] = a.g[i] * b;
#pragma unroll
    for (int i = 0; i < Dual2<K>::NH; ++i) r.h[i] = a.h[i] * b;
    return r;
}
template <int K>
RK_D2_FN Dual2<K> operator*(double a, const Dual2<K>& b) { return b * a; }
template <int K>
RK_D2_FN Dual2<K> operator/(const Dual2<K>& a, double b) {
    Dual2<K> r;
    r.v = a.v / b;
#pragma unroll
    for (int i = 0; i < K; ++i) r.g[i] = a.g[i] / b;
#pragma unroll
    for (int i = 0; i < Dual2<K>::NH; ++i) r.h[i] = a.h[i] / b;
    return r;
}
template <int K>
RK_D2_FN Dual2<K> operator/(double a, const Dual2<K>& b) { return d2_recip<K>(b) * a; }

// plain-double overload so that generic code inside namespace rk can call lgamma(x) (dual.hpp has the other functions')
RK_D2_FN double lgamma(double x) { return ::lgamma(x); }

#define RK_D2_FUN(NAME, F0, F1, F2)                       \
    template <int K>                                      \
    RK_D2_FN Dual2<K> NAME(const Dual2<K>& a) {           \
        const double x = a.v;                             \
        const double f0 = F0;                             \
        (void)x;                                          \
        return d2_chain<K>(a, f0, F1, F2);                \
    }
RK_D2_FUN(sin, ::sin(x), ::cos(x), -f0)
RK_D2_FUN(cos, ::cos(x), -::sin(x), -f0)
RK_D2_FUN(tan, ::tan(x), 1.0 + f0 * f0, 2.0 * f0 * (1.0 + f0 * f0))
RK_D2_FUN(exp, ::exp(x), f0, f0)
RK_D2_FUN(log, ::log(x), 1.0 / x, -1.0 / (x * x))
RK_D2_FUN(sqrt, ::sqrt(x), 0.5 / f0, -0.25 / (f0 * x))
RK_D2_FUN(tanh, ::tanh(x), 1.0 - f0 * f0, -2.0 * f0 * (1.0 - f0 * f0))
RK_D2_FUN(sinh, ::sinh(x), ::cosh(x), f0)
RK_D2_FUN(cosh, ::cosh(x), ::sinh(x), f0)
RK_D2_FUN(atan, ::atan(x), 1.0 / (1.0 + x * x), -2.0 * x / ((1.0 + x * x) * (1.0 + x * x)))
RK_D2_FUN(asin, ::asin(x), 1.0 / ::sqrt(1.0 - x * x), x / ((1.0 - x * x) * ::sqrt(1.0 - x * x)))
RK_D2_FUN(acos, ::acos(x), -1.0 / ::sqrt(1.0 - x * x), -x / ((1.0 - x * x) * ::sqrt(1.0 - x * x)))
RK_D2_FUN(log1p, ::log1p(x), 1.0 / (1.0 + x), -1.0 / ((1.0 + x) * (1.0 + x)))
RK_D2_FUN(expm1, ::expm1(x), f0 + 1.0, f0 + 1.0)
#undef RK_D2_FUN

}  // namespace rk
