"""
Host side of rodeo_amd.inference.dalton.daltonng / solve_mv_nn (src/rodeo/inference/dalton.py:547-1039): signatures, the
tracer of the observation log-likelihood, second-order duals (csrc/dual2.hpp) built as plain host C++, and every refusal --
none of it needs a device.
"""
import ctypes as C
import inspect
import os
import shutil
import subprocess
import sys
import numpy as np
import pytest
import rodeo_amd as ra
from rodeo_amd import _lib, trace
import rodeo_amd.inference.dalton  # noqa: F401  (the package binds the name `dalton` to the function)
from rodeo_amd.interrogate import interrogate_chkrebtii, interrogate_kramer
from rodeo_amd.trace import gammaln, trace_obs_source

dmod = sys.modules["rodeo_amd.inference.dalton"]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_ARGS = ["key", "ode_fun", "ode_weight", "ode_init", "t_min", "t_max", "n_steps", "interrogate", "prior_pars", "obs_data",
            "obs_times", "obs_loglik_i", "kalman_type", "params"]                     # dalton.py:851-856 / :955-960
THETA = np.array([0.2, 0.2, 3.0])


def poisson_loglik(obs_data_i, ode_data_i, ind, **params):
    """parameter.md:545-559 with NumPy."""
    eta = 0.1 + 0.5 * ode_data_i[:, 0]
    y = obs_data_i.flatten()
    return np.sum(y * eta - np.exp(eta) - gammaln(y + 1.0))


@pytest.mark.parametrize("name", ["daltonng", "solve_mv_nn"])
def test_reference_signatures(name):
    sig = inspect.signature(getattr(dmod, name))
    assert list(sig.parameters) == REF_ARGS
    assert sig.parameters["kalman_type"].default == "standard"
    assert sig.parameters["params"].kind is inspect.Parameter.VAR_KEYWORD
    assert not hasattr(ra.inference, name)               # imported from rodeo_amd.inference.dalton, not re-exported


def test_tracer_on_the_poisson_function():
    src, active = trace_obs_source(poisson_loglik, 2, 3, 1, (("theta", 3),), "PoissonObs")
    assert active == ((0,), (0,))
    for piece in ("struct PoissonObs", "static constexpr int D = 2;", "static constexpr int P = 3;", "static constexpr int NY = 1;",
                  "static constexpr int NTHETA = 3;", "static constexpr int MO = 1;", "NACT[D] = {1, 1};",
                  "ACT[D][3] = {{0, 0, 0}, {0, 0, 0}};", "template <class T>", "exp((0.1 + (0.5 * X[0][0])))",
                  "lgamma((y[1][0] + 1.0))"):
        assert piece in src, piece
    assert "X[0][1]" not in src and "X[1][2]" not in src
    # the index and a parameter enter as symbols; two components of one block, none of the other
    src2, act2 = trace_obs_source(lambda y, X, i, theta: -0.5 * theta[0] * (y[0, 1] - X[0, 0] * X[0, 2]) ** 2 + i * 0.0, 2, 4, 2,
                                  (("theta", 3),), "Two")
    assert act2 == ((0, 2), ()) and "MO = 2" in src2 and "NACT[D] = {2, 0}" in src2 and "{0, 2, 0}" in src2
    assert "th[0]" in src2 and "ind" in src2


def test_traced_source_compiles_for_the_device():
    """hiprtc builds both forward forms and the observation kernel around the traced struct (no GPU needed)."""
    lib = _lib.load()
    src, active = trace_obs_source(poisson_loglik, 2, 3, 1, (("theta", 3),), "PoissonObsC")
    oid = C.c_int32(0)
    _lib.check(lib.rk_register_obs_source(b"PoissonObsC", src.encode(), 2, 3, 1, 3, 1, C.byref(oid)))
    _lib.check(lib.rk_obs_compile_check(oid.value, _lib.RHS_FITZHUGH_NAGUMO, _lib.INTERROGATE_KRAMER))
    bad = C.c_int32(0)
    _lib.check(lib.rk_register_obs_source(b"Nope", b"struct Nope { int x };", 2, 3, 1, 3, 1, C.byref(bad)))
    assert lib.rk_obs_compile_check(bad.value, _lib.RHS_FITZHUGH_NAGUMO, _lib.INTERROGATE_KRAMER) == _lib.RK_ERR_INVALID
    assert lib.rk_register_obs_source(b"X", b"", 2, 3, 5, 3, 1, C.byref(bad)) == _lib.RK_ERR_INVALID       # n_ycols
    assert lib.rk_register_obs_source(b"X", b"", 2, 3, 1, 3, 4, C.byref(bad)) == _lib.RK_ERR_INVALID       # n_active


def test_gammaln_accepts_floats_and_refuses_state_dependent_symbols():
    from math import lgamma
    assert gammaln(4.0) == lgamma(4.0)
    assert np.allclose(gammaln(np.array([1.0, 2.5])), [lgamma(1.0), lgamma(2.5)])
    with pytest.raises(ValueError, match="digamma"):
        trace_obs_source(lambda y, X, i, **kw: gammaln(X[0, 0] + 1.0), 1, 3, 1, (), "G")
    with pytest.raises(ValueError, match="digamma"):
        trace_obs_source(lambda y, X, i, **kw: np.sum(gammaln(np.exp(X[:, 0]) * y[:, 0])), 2, 3, 1, (), "G")


DUAL2_MAIN = r"""
#include <cstdio>
#include "dual2.hpp"
using namespace rk;
int main() {
    // f(x, y, z) = exp(x * y) / (1 + z * z) + sin(x) * log(y) - 2 / z + sqrt(y) * tanh(z)
    const double x = 0.3, y = 1.7, z = -0.8;
    Dual2<3> X(x), Y(y), Z(z);
    X.g[0] = 1.0; Y.g[1] = 1.0; Z.g[2] = 1.0;
    const Dual2<3> f = exp(X * Y) / (1.0 + Z * Z) + sin(X) * log(Y) - 2.0 / Z + sqrt(Y) * tanh(Z);
    std::printf("%.17g\n", f.v);
    for (int i = 0; i < 3; ++i) std::printf("%.17g\n", f.g[i]);
    for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) std::printf("%.17g\n", f.hess(i, j));
    // one direction: g(x) = x / (x + 2) - expm1(x) * cos(x), and lgamma on a plain double
    Dual2<1> U(x); U.g[0] = 1.0;
    const Dual2<1> g = U / (U + 2.0) - expm1(U) * cos(U);
    std::printf("%.17g\n%.17g\n%.17g\n%.17g\n", g.v, g.g[0], g.h[0], rk::lgamma(4.5));
    // the remaining elementary functions, each through the chain rule at u(x) = x * x + 0.1 (u' = 2 x, u'' = 2)
    const Dual2<1> W = U * U + 0.1;
    const Dual2<1> fs[] = {tan(W), asin(W), acos(W), atan(W), sinh(W), cosh(W), log1p(W)};
    for (const Dual2<1>& r : fs) std::printf("%.17g\n%.17g\n%.17g\n", r.v, r.g[0], r.h[0]);
    return 0;
}
"""


def _host_compiler():
    for c in ("g++", "c++", "clang++", "/opt/rocm/lib/llvm/bin/clang++"):
        path = shutil.which(c) or (c if os.path.isabs(c) and os.path.exists(c) else None)
        if path:
            return path
    raise RuntimeError("no host C++ compiler (the build of this package needs one)")


def test_dual2_on_the_host_against_analytic_derivatives(tmp_path):
    from math import acos, asin, atan, cos, cosh, exp, expm1, lgamma, log, log1p, sin, sinh, sqrt, tan, tanh
    (tmp_path / "main.cpp").write_text(DUAL2_MAIN)
    exe = tmp_path / "dual2_host"
    subprocess.run([_host_compiler(), "-std=c++17", "-O1", "-I", os.path.join(ROOT, "rodeo_amd", "csrc"), str(tmp_path / "main.cpp"),
                    "-o", str(exe), "-lm"], check=True, capture_output=True)
    out = [float(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    x, y, z = 0.3, 1.7, -0.8
    e, q, th, sech2 = exp(x * y), 1.0 + z * z, tanh(z), 1.0 / cosh(z) ** 2
    f = e / q + sin(x) * log(y) - 2.0 / z + sqrt(y) * th
    g = [y * e / q + cos(x) * log(y), x * e / q + sin(x) / y + 0.5 / sqrt(y) * th,
         -2.0 * z * e / q ** 2 + 2.0 / z ** 2 + sqrt(y) * sech2]
    H = np.zeros((3, 3))
    H[0, 0] = y * y * e / q - sin(x) * log(y)
    H[0, 1] = H[1, 0] = (1.0 + x * y) * e / q + cos(x) / y
    H[0, 2] = H[2, 0] = -2.0 * z * y * e / q ** 2
    H[1, 1] = x * x * e / q - sin(x) / y ** 2 - 0.25 * y ** -1.5 * th
    H[1, 2] = H[2, 1] = -2.0 * z * x * e / q ** 2 + 0.5 / sqrt(y) * sech2
    H[2, 2] = e * (-2.0 / q ** 2 + 8.0 * z * z / q ** 3) - 4.0 / z ** 3 - 2.0 * sqrt(y) * th * sech2
    want = [f] + g + list(H.ravel())
    g1 = x / (x + 2.0) - expm1(x) * cos(x)
    d1 = 2.0 / (x + 2.0) ** 2 - exp(x) * cos(x) + expm1(x) * sin(x)
    d2 = -4.0 / (x + 2.0) ** 3 - exp(x) * cos(x) + 2.0 * exp(x) * sin(x) + expm1(x) * cos(x)
    want += [g1, d1, d2, lgamma(4.5)]
    u, du, ddu = x * x + 0.1, 2.0 * x, 2.0
    r = 1.0 - u * u
    for f0, f1, f2 in [(tan(u), 1.0 + tan(u) ** 2, 2.0 * tan(u) * (1.0 + tan(u) ** 2)),
                       (asin(u), r ** -0.5, u * r ** -1.5), (acos(u), -r ** -0.5, -u * r ** -1.5),
                       (atan(u), 1.0 / (1.0 + u * u), -2.0 * u / (1.0 + u * u) ** 2),
                       (sinh(u), cosh(u), sinh(u)), (cosh(u), sinh(u), cosh(u)),
                       (log1p(u), 1.0 / (1.0 + u), -1.0 / (1.0 + u) ** 2)]:
        want += [f0, f1 * du, f2 * du * du + f1 * ddu]                  # (f o u)'' = f'' u'^2 + f' u''
    assert len(out) == len(want)
    for a, b in zip(out, want):
        assert abs(a - b) <= 1e-13 * max(1.0, abs(b)), (a, b)


def _case(p=3, d=2, n_obs=3):
    W = np.zeros((d, 1, p))
    W[:, :, 1] = 1.0
    x0 = np.zeros((d, p))
    prior = ra.ibm_init(0.05, p, np.full(d, 0.1))
    return dict(W=W, x0=x0, prior=prior, y=np.ones((n_obs, d, 1)), times=np.linspace(0.5, 2.0, n_obs))


def _call(fn, c, itg=interrogate_kramer, loglik=poisson_loglik, ode=ra.ode.fitzhugh_nagumo, **kw):
    return fn(None, ode, c["W"], c["x0"], 0.0, 2.0, 40, itg, c["prior"], c["y"], c["times"], loglik,
              **{"theta": THETA, **kw})


@pytest.mark.parametrize("fn", [dmod.daltonng, dmod.solve_mv_nn], ids=["daltonng", "solve_mv_nn"])
def test_refusals_are_raised_without_a_device(fn, monkeypatch):
    import rodeo_amd.solve as solve
    monkeypatch.setattr(solve, "default_device", lambda *a, **k: pytest.fail("a device was asked for"))
    with pytest.raises(NotImplementedError, match="not built"):
        _call(fn, _case(), kalman_type="square-root")
    with pytest.raises(NotImplementedError):
        _call(fn, _case(), kalman_type="other")
    import functools
    with pytest.raises(NotImplementedError, match="chkrebtii"):
        _call(fn, _case(), itg=functools.partial(interrogate_chkrebtii, kalman_type="standard"))
    c = _case()
    c["W"] = np.zeros((2, 2, 3))
    with pytest.raises(NotImplementedError, match="n_bmeas"):
        _call(fn, c)
    for p in (1, 7):
        c = _case(p=3)
        c["W"] = np.zeros((2, 1, p))
        with pytest.raises(NotImplementedError, match="n_bstate"):
            _call(fn, c)
    c = _case(p=6, d=3)
    with pytest.raises(NotImplementedError, match="three or more blocks"):
        _call(fn, c, ode=ra.ode.lorenz63, theta=np.array([28.0, 10.0, 8.0 / 3.0]))
    c = _case(p=3, d=1)
    with pytest.raises(NotImplementedError, match="lane-per-trajectory"):
        _call(fn, c, ode=ra.ode.linear_dense(1, 3))
    with pytest.raises(NotImplementedError, match="blocks"):
        _call(fn, _case(p=3, d=2), ode=ra.ode.higher_order)
    c = _case()
    c["y"] = np.ones((3, 2, 5))
    with pytest.raises(ValueError, match="columns"):
        _call(fn, c)
    c = _case()
    c["times"] = np.array([0.5, 0.5, 2.0])
    with pytest.raises(ValueError, match="strictly increasing"):
        _call(fn, c)
    c = _case()
    c["times"] = np.array([0.5, 1.0, 2.5])
    with pytest.raises(ValueError, match="beyond t_max"):
        _call(fn, c)
    with pytest.raises(ValueError, match="scalar"):
        _call(fn, _case(), loglik=lambda y, X, i, **kw: X[:, 0] * y[:, 0])
    with pytest.raises(ValueError, match="more than 3"):
        _call(fn, _case(p=4), loglik=lambda y, X, i, **kw: -np.sum(X[0, :] ** 2))
    with pytest.raises(ValueError, match="does not depend on the state"):
        _call(fn, _case(), loglik=lambda y, X, i, **kw: np.sum(y) * 1.0)
    with pytest.raises(ValueError, match="digamma"):
        _call(fn, _case(), loglik=lambda y, X, i, **kw: gammaln(X[0, 0]))


def test_a_function_built_anew_per_call_finds_its_model_again_and_a_changed_constant_is_another_model(monkeypatch):
    """The traced models are kept by the hash of the generated source: no growth for a lambda per call; a closed-over value is
    a constant of that source."""
    monkeypatch.setattr(dmod, "_obs_models", {})
    c = _case()

    def model(scale):
        fn = lambda y, X, i, **kw: -scale * np.sum((y[:, 0] - X[:, 0]) ** 2)      # noqa: E731
        return dmod._ng_refusals(ra.ode.fitzhugh_nagumo, c["W"], interrogate_kramer, "standard", c["y"], c["times"], fn, 0.0, 2.0,
                                 40, {"theta": THETA})[2]
    a, b, other = model(0.5), model(0.5), model(0.75)
    assert a is b and other is not a and a["struct"] != other["struct"]
    assert len(dmod._obs_models) == 2 and a["struct"] in a["source"]
