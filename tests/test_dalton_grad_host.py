"""
``dalton_grid_jvp`` / ``dalton_grid_grad`` / ``dalton_grad`` on the host (no GPU): every refusal that comes before any device work
(``default_device`` patched to fail), the staging of the directions (shapes and the batch-minor layout), the empty observation
set, the library's refusals on the configuration alone, csrc/tangent.hpp built as plain host C++ (f, f., J and J. of a few
compositions against analytic values), and the tracer: ``trace_source``'s text is what it was, the gradient kind's text compiles
on the host and with hiprtc.
"""
import ctypes as C
import functools
import hashlib
import os
import shutil
import subprocess
import sys
import numpy as np
import pytest
import rodeo_amd as ra
import rodeo_amd.inference.dalton  # noqa: F401
from rodeo_amd import _lib
from rodeo_amd.interrogate import interrogate_chkrebtii, interrogate_kramer
from rodeo_amd.trace import from_python, grad_from_python, trace_grad_source, trace_source

dmod = sys.modules["rodeo_amd.inference.dalton"]             # (rodeo_amd.inference.dalton, the attribute, is the function)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _fhn(p=3, n_bobs=1, times=(0.1, 0.3), B=None, ode=ra.ode.fitzhugh_nagumo, **over):
    W, init = ra.utils.first_order_pad(ra.ode.fitzhugh_nagumo, 2, p)
    theta = np.array([0.2, 0.2, 3.0]) if B is None else np.array([0.2, 0.2, 3.0]) * (1 + 0.01 * np.arange(B)[:, None])
    sigma = np.array([0.5, 0.3])
    n = len(times)
    D = np.zeros((n, 2, n_bobs, p))
    D[..., 0, 0] = 1.0
    a = dict(key=None, ode_fun=ode, ode_weight=W, ode_init=init(np.array([-1.0, 1.0]), 0.0, theta=theta),
             t_grid=np.array([0.0, 0.1, 0.15, 0.3, 0.4]), interrogate=interrogate_kramer, prior_at=lambda h: ra.ibm_init(h, p, sigma),
             obs_data=np.zeros((n, 2, n_bobs)), obs_times=np.array(times, dtype=float), obs_weight=D,
             obs_var=np.tile(0.01 * np.eye(n_bobs), (n, 2, 1, 1)), tangents=dict(theta=np.eye(3)), theta=theta)
    a.update(over)
    return a


def _grad(**over):
    a = _fhn(**over)
    a.pop("tangents")
    return a


@pytest.fixture
def no_device(monkeypatch):
    """Any attempt to reach the device fails the test: the refusals below come first."""
    def fail(*a, **k):
        raise AssertionError("default_device was reached")
    monkeypatch.setattr(ra.device, "default_device", fail)
    monkeypatch.setattr(ra.solve, "default_device", fail)


def test_names_and_docstrings():
    for name in ("dalton_grid_jvp", "dalton_grid_grad", "dalton_grad", "DaltonGrad"):
        assert hasattr(dmod, name) and not hasattr(ra.inference, name)                      # not re-exported
    assert "1e-8" in dmod.dalton_grid_jvp.__doc__ and "contributes nothing" in dmod.dalton_grid_jvp.__doc__
    assert "NOT bit for bit" in dmod.dalton_grad.__doc__ and "1e-9" in dmod.dalton_grad.__doc__


def test_a_served_call_reaches_the_device(no_device):
    """(the fixture works: what is not refused does ask for a device)"""
    with pytest.raises(AssertionError, match="default_device was reached"):
        dmod.dalton_grid_jvp(**_fhn())
    with pytest.raises(AssertionError, match="default_device was reached"):
        dmod.dalton_grid_grad(**_grad(), wrt=("theta", "ode_init"))
    with pytest.raises(AssertionError, match="default_device was reached"):
        dmod.dalton_grid_jvp(**_fhn(p=2, tangents=dict(ode_init=np.ones((1, 2, 2)))))


@pytest.mark.parametrize("over", [
    dict(kalman_type="square-root"), dict(interrogate=functools.partial(interrogate_chkrebtii, kalman_type="standard")),
    dict(n_bobs=2), dict(n_bobs=3), dict(ode_weight=np.zeros((2, 2, 3))), dict(p=4), dict(p=5), dict(p=6),
    dict(ode=ra.ode.higher_order), dict(tangents=dict(sigma=np.ones((1, 2)))), dict(tangents=dict(ode_weight=np.ones((1, 2)))),
    dict(tangents=dict(obs_data=np.ones((1, 2)))), dict(tangents=dict(prior_pars=np.ones((1, 2))))],
    ids=["square-root", "chkrebtii", "n_bobs=2", "n_bobs=3", "n_bmeas=2", "p=4", "p=5", "p=6", "higher_order", "d/dsigma", "d/dode_weight",
         "d/ddata", "d/dprior"])
def test_what_is_not_built_is_refused_before_any_device_work(no_device, over):
    with pytest.raises(NotImplementedError, match="not built"):
        dmod.dalton_grid_jvp(**_fhn(**over))
    if "tangents" not in over:
        with pytest.raises(NotImplementedError, match="not built"):
            dmod.dalton_grid_grad(**_grad(**over))
    else:
        with pytest.raises(NotImplementedError, match="not built"):
            dmod.dalton_grid_grad(**_grad(), wrt=tuple(over["tangents"]))


def test_lorenz_at_four_and_three_blocks_of_a_traced_function_are_refused(no_device):
    W, init = ra.utils.first_order_pad(ra.ode.lorenz63, 3, 4)
    theta = np.array([28.0, 10.0, 8.0 / 3.0])
    D = np.zeros((1, 3, 1, 4))
    D[..., 0] = 1.0
    with pytest.raises(NotImplementedError, match="not built"):
        dmod.dalton_grid_jvp(None, ra.ode.lorenz63, W, init(np.array([-12.0, -5.0, 38.0]), 0.0, theta=theta), [0.0, 0.1, 0.2],
                             interrogate_kramer, lambda h: ra.ibm_init(h, 4, np.ones(3)), np.zeros((1, 3, 1)), [0.1], D,
                             np.ones((1, 3, 1, 1)), dict(theta=np.eye(3)), theta=theta)


def test_dalton_grad_refuses_like_the_grid_calls(no_device):
    a = _grad()
    t_grid, prior_at = a.pop("t_grid"), a.pop("prior_at")
    args = dict(a, t_min=0.0, t_max=0.4, n_steps=4, prior_pars=prior_at(0.1))
    with pytest.raises(AssertionError, match="default_device was reached"):
        dmod.dalton_grad(**args)
    with pytest.raises(NotImplementedError, match="not built"):
        dmod.dalton_grad(**dict(args, kalman_type="square-root"))
    with pytest.raises(NotImplementedError, match="not built"):
        dmod.dalton_grad(**dict(args, wrt=("sigma",)))
    with pytest.raises(ValueError, match="no parameter"):
        dmod.dalton_grad(**dict(args, wrt=("phi",)))
    with pytest.raises(ValueError, match="strictly increasing"):
        dmod.dalton_grad(**dict(args, obs_times=np.array([0.3, 0.1])))


@pytest.mark.parametrize("tangents,word", [
    (dict(phi=np.ones((1, 3))), "no parameter"), ({}, "K = 0"), (dict(theta=np.zeros((0, 3))), "K = 0"),
    (dict(theta=np.ones((1, 4))), "shape"), (dict(theta=np.ones(3)), "shape"), (dict(ode_init=np.ones((1, 2, 4))), "shape"),
    (dict(ode_init=np.ones((2, 3))), "shape"), (dict(theta=np.ones((2, 1, 3))), "shape"),      # a batch axis on an unbatched call
    (dict(theta=np.array([[1.0, np.nan, 0.0]])), "non-finite"), (dict(ode_init=np.full((1, 2, 3), np.inf)), "non-finite"),
    (dict(theta=np.ones((2, 3)), ode_init=np.ones((3, 2, 3))), "count K"), (dict(theta="abc"), "no array"), ([1.0], "dict")])
def test_bad_directions_are_refused(no_device, tangents, word):
    with pytest.raises(ValueError, match=word):
        dmod.dalton_grid_jvp(**_fhn(tangents=tangents))


def test_bad_wrt_and_init_jac_are_refused(no_device):
    with pytest.raises(ValueError, match="no parameter"):
        dmod.dalton_grid_grad(**_grad(), wrt=("phi",))
    with pytest.raises(ValueError, match="K = 0"):
        dmod.dalton_grid_grad(**_grad(), wrt=())
    with pytest.raises(ValueError, match="twice"):
        dmod.dalton_grid_grad(**_grad(), wrt=("theta", "theta"))
    with pytest.raises(ValueError, match="init_jac"):
        dmod.dalton_grid_grad(**_grad(), wrt=("ode_init",), init_jac=dict(theta=np.zeros((2, 3, 3))))
    with pytest.raises(ValueError, match="shape"):
        dmod.dalton_grid_grad(**_grad(), wrt=("theta",), init_jac=dict(theta=np.zeros((2, 3, 2))))
    with pytest.raises(ValueError, match="shape"):                               # a batched Jacobian on an unbatched call
        dmod.dalton_grid_grad(**_grad(), wrt=("theta",), init_jac=dict(theta=np.zeros((4, 2, 3, 3))))


def test_what_dalton_grid_refuses_is_refused(no_device):
    for times, word in (((0.1, 0.2), "0.2 is no node"), ((0.3, 0.1), "strictly increasing"), ((0.1, np.nan), "non-finite")):
        with pytest.raises(ValueError, match=word):
            dmod.dalton_grid_jvp(**_fhn(times=times))
    with pytest.raises(ValueError, match="strictly increasing"):
        dmod.dalton_grid_jvp(**_fhn(t_grid=[0.0, 0.5, 0.5]))
    with pytest.raises(ValueError, match="callable"):
        dmod.dalton_grid_jvp(**_fhn(prior_at=1.0))
    with pytest.raises(ValueError, match="obs_weight"):
        dmod.dalton_grid_jvp(**_fhn(obs_weight=np.zeros((2, 2, 1, 4))))


def test_an_empty_observation_set_returns_zeros_without_a_launch(no_device):
    value, dvalue = dmod.dalton_grid_jvp(**_fhn(times=(), tangents=dict(theta=np.ones((4, 3)))))
    assert value == 0.0 and isinstance(value, float) and dvalue.shape == (4,) and np.all(dvalue == 0.0)
    value, dvalue = dmod.dalton_grid_jvp(**_fhn(times=(), B=5, tangents=dict(ode_init=np.ones((5, 2, 2, 3)))))
    assert value.shape == (5,) and dvalue.shape == (5, 2) and np.all(value == 0.0) and np.all(dvalue == 0.0)
    res = dmod.dalton_grid_grad(**_grad(times=(), B=5), wrt=("theta", "ode_init"))
    assert np.all(res.value == 0.0) and res.grad["theta"].shape == (5, 3) and res.grad["ode_init"].shape == (5, 2, 3)
    with pytest.raises(ValueError, match="K = 0"):                                # the refusals still come first
        dmod.dalton_grid_jvp(**_fhn(times=(), tangents={}))


# ---- staging ----------------------------------------------------------------------------------------------------------------
def test_directions_are_staged_batch_minor():
    ode, B, d, p = ra.ode.fitzhugh_nagumo, 4, 2, 3
    rng = np.random.default_rng(0)
    th, x0 = rng.standard_normal((5, 3)), rng.standard_normal((5, d, p))
    K, dth, dth_b, dx, dx_b = dmod._stage_directions("t", ode, dict(theta=th, ode_init=x0), B, True, d, p)
    assert (K, dth_b, dx_b) == (5, 0, 0) and dth.shape == (5, 3) and dx.shape == (5, d, p)
    np.testing.assert_array_equal(dth, th)
    np.testing.assert_array_equal(dx, x0)
    thb, x0b = rng.standard_normal((B, 5, 3)), rng.standard_normal((B, 5, d, p))
    K, dth, dth_b, dx, dx_b = dmod._stage_directions("t", ode, dict(theta=thb, ode_init=x0b), B, True, d, p)
    assert (K, dth_b, dx_b) == (5, 1, 1) and dth.shape == (5, 3, B) and dx.shape == (5, d, p, B)
    assert dth.flags.c_contiguous and dx.flags.c_contiguous
    for b in range(B):
        np.testing.assert_array_equal(dth[..., b], thb[b])
        np.testing.assert_array_equal(dx[..., b], x0b[b])
    K, dth, dth_b, dx, dx_b = dmod._stage_directions("t", ode, dict(ode_init=x0), B, True, d, p)      # a missing key: no array at all
    assert dth is None and dth_b == 0 and dx.shape == (5, d, p)


def test_unit_directions_of_grad_and_init_jac():
    a = _grad()
    J = np.arange(18.0).reshape(2, 3, 3)
    tangents, layout = dmod._unit_directions("t", a["ode_fun"], a["ode_weight"], a["ode_init"], ("theta", "ode_init"), dict(theta=J),
                                             dict(theta=a["theta"]))
    assert [(n, k, s) for n, k, s in layout] == [("theta", 0, (3,)), ("ode_init", 3, (2, 3))]
    np.testing.assert_array_equal(tangents["theta"], np.concatenate([np.eye(3), np.zeros((6, 3))]))
    x0 = tangents["ode_init"]
    assert x0.shape == (9, 2, 3)
    for j in range(3):
        np.testing.assert_array_equal(x0[j], J[..., j])                          # direction j of theta moves ode_init by J[..., j]
    np.testing.assert_array_equal(x0[3:].reshape(6, 6), np.eye(6))
    tangents, _ = dmod._unit_directions("t", a["ode_fun"], a["ode_weight"], a["ode_init"], ("theta",), None, dict(theta=a["theta"]))
    assert set(tangents) == {"theta"}


# ---- the library, on the configuration alone -------------------------------------------------------------------------------
def _cfg(rhs=_lib.RHS_FITZHUGH_NAGUMO, d=2, p=3, m=1, itg=_lib.INTERROGATE_KRAMER, kalman=_lib.KALMAN_STANDARD, flags=_lib.FLAG_BATCH_MINOR):
    return _lib.SolveCfg(n_traj=16, n_steps=50, n_block=d, n_bstate=p, n_bmeas=m, rhs_id=rhs, interrogate=itg, kalman_type=kalman,
                         n_theta=3, flags=flags, t_min=0.0, t_max=1.0, seed=0, traj_offset=0)


def _jvp(cfg, n_bobs=1, n_dir=1):
    """rk_dalton_grid_jvp with no handle and no pointers: only the configuration, n_bobs and n_dir can be looked at."""
    lib = _lib.load()
    rc = lib.rk_dalton_grid_jvp(None, C.byref(cfg), None, None, None, None, None, 1, n_bobs, None, n_dir, None, 0, None, 0, None, None)
    return rc, lib.rk_last_error().decode()


@pytest.mark.parametrize("cfg,n_bobs", [
    (_cfg(kalman=_lib.KALMAN_SQRT), 1), (_cfg(itg=_lib.INTERROGATE_CHKREBTII), 1), (_cfg(m=2), 1), (_cfg(), 2), (_cfg(), 3),
    (_cfg(p=4), 1), (_cfg(p=6), 1), (_cfg(rhs=_lib.RHS_LORENZ63, d=3, p=4), 1), (_cfg(rhs=_lib.RHS_HIGHER_ORDER, d=1), 1)])
def test_library_says_not_built(cfg, n_bobs):
    rc, msg = _jvp(cfg, n_bobs)
    assert rc == _lib.RK_ERR_UNSUPPORTED and "dalton_grid_jvp" in msg and "not built" in msg, (rc, msg)


def test_library_calls_bad_sizes_invalid_and_passes_a_served_configuration_on():
    for cfg, n_dir, word in ((_cfg(), 0, "n_dir"), (_cfg(flags=0), 1, "RK_FLAG_BATCH_MINOR"), (_cfg(p=0), 1, "non-positive")):
        rc, msg = _jvp(cfg, 1, n_dir)
        assert rc == _lib.RK_ERR_INVALID and word in msg, (rc, msg)
    for cfg in (_cfg(), _cfg(p=2), _cfg(itg=_lib.INTERROGATE_RODEO), _cfg(itg=_lib.INTERROGATE_SCHOBER), _cfg(rhs=_lib.RHS_LORENZ63, d=3),
                _cfg(rhs=_lib.RHS_LORENZ63, d=3, p=2)):
        rc, msg = _jvp(cfg, 1, 5)
        assert rc == _lib.RK_ERR_INVALID and "null argument" in msg, (rc, msg)


# ---- the tracer -------------------------------------------------------------------------------------------------------------
def _fitz(X, t, theta):
    a, b, c = theta
    V, R = X[0, 0], X[1, 0]
    return np.array([[c * (V - V * V * V / 3 + R)], [-1 / c * (V - a + b * R)]])


def _forced(X, t, theta):
    return np.array([np.sin(theta[0] * t) * X[1, 0] - np.exp(-X[0, 0]) / theta[1], np.tanh(X[0, 0] * X[1, 0]) + X[1, 1] ** 2])


def test_trace_source_emits_what_it_did():
    """The text of the solver's emitter for a fixed function, by its hash: existing hiprtc sources and cache keys do not move."""
    src, ndep, n_bmeas = trace_source(_fitz, 2, 3, (("theta", 3),), "Traced_fixed")
    assert (ndep, n_bmeas) == (1, 1)
    assert "const double (&th)[NTHETA]" in src and "rhs_generic" not in src and "class TH" not in src
    assert hashlib.sha1(src.encode()).hexdigest() == "3387d242e9cb5bbeedd83706c85679a9df15b264"


def test_the_gradient_kind_is_generic_in_the_parameters():
    src, ndep = trace_grad_source(_fitz, 2, 3, (("theta", 3),), "G")
    assert ndep == 1 and "template <class T, class TH, int P>" in src and "const TH (&th)[NTHETA]" in src
    plain = trace_source(_fitz, 2, 3, (("theta", 3),), "G")[0]
    body = [ln for ln in plain.splitlines() if ln.strip().startswith("out[")]
    assert body and all(ln in src for ln in body)                                # the same expressions
    with pytest.raises(ValueError, match="n_bmeas = 1"):
        trace_grad_source(lambda X, t, theta: np.array([[X[0, 0], X[0, 1]]]), 1, 3, (("theta", 3),), "G")


def test_a_traced_function_is_served_through_the_gradient_kind(no_device):
    with pytest.raises(AssertionError, match="default_device was reached"):
        dmod.dalton_grid_jvp(**_fhn(ode=_fitz))
    with pytest.raises(AssertionError, match="default_device was reached"):
        dmod.dalton_grid_jvp(**_fhn(ode=from_python(_fitz, 2, 3, theta=3)))
    g = grad_from_python(_fitz, 2, 3, theta=3)
    assert g.grad_kind and g is grad_from_python(_fitz, 2, 3, theta=3) and g.rhs_id >= _lib.RHS_USER_BASE
    rc, msg = _jvp(_cfg(rhs=g.rhs_id))
    assert rc == _lib.RK_ERR_INVALID and "null argument" in msg, (rc, msg)
    for cfg, word in ((_cfg(rhs=g.rhs_id, p=4), "not built"), (_cfg(rhs=g.rhs_id, d=3), "n_block")):
        rc, msg = _jvp(cfg)
        assert rc == _lib.RK_ERR_UNSUPPORTED and word in msg, (rc, msg)


def test_the_gradient_kind_builds_with_hiprtc_without_a_device():
    lib = _lib.load()
    g = grad_from_python(_forced, 2, 3, theta=2)
    for itg in (_lib.INTERROGATE_RODEO, _lib.INTERROGATE_KRAMER):
        assert lib.rk_dalton_grad_compile_check(g.rhs_id, 3, itg) == _lib.RK_OK, lib.rk_last_error().decode()
    plain = from_python(_forced, 2, 3, theta=2)                                  # the solver's kind has no rhs_generic
    assert lib.rk_dalton_grad_compile_check(plain.rhs_id, 3, _lib.INTERROGATE_KRAMER) == _lib.RK_ERR_INVALID


# ---- tangent.hpp as plain host C++ -------------------------------------------------------------------------------------------
def _host_compiler():
    for c in ("g++", "c++", "clang++", "/opt/rocm/lib/llvm/bin/clang++"):
        path = shutil.which(c) or (c if os.path.isabs(c) and os.path.exists(c) else None)
        if path:
            return path
    raise RuntimeError("no host C++ compiler (the build of this package needs one)")


TANGENT_MAIN = r"""
#include <cstdio>
#define __device__
#define __forceinline__ inline
#include "tangent.hpp"
using namespace rk;
%s
// f(x, y; a) = exp(x * y) / (1 + a * a) + sin(x) * log(y) - 2 / a + sqrt(y) * tanh(a * x), written once on generic scalars
template <class T, class TH>
T fun(const T& x, const T& y, const TH& a) { return exp(x * y) / (1.0 + a * a) + sin(x) * log(y) - 2.0 / a + sqrt(y) * tanh(a * x); }
template <class T>
T rest(const T& w) { return tan(w) + asin(w) * acos(w) - atan(w) / cosh(w) + sinh(w) * log1p(w) - expm1(w) * cos(w); }
int main() {
    const double x = 0.3, y = 1.7, a = -0.8, dx = 0.7, dy = -0.4, da = 1.3;
    // one direction: f and f.
    const Tangent f1 = fun(Tangent(x, dx), Tangent(y, dy), Tangent(a, da));
    std::printf("%%.17g\n%%.17g\n", f1.v, f1.d);
    // the Jacobian dual: f, f., J = (df/dx, df/dy), J.
    TJet<2> X(Tangent(x, dx)), Y(Tangent(y, dy));
    X.d[0] = Tangent(1.0); Y.d[1] = Tangent(1.0);
    const TJet<2> f2 = fun(X, Y, Tangent(a, da));
    std::printf("%%.17g\n%%.17g\n%%.17g\n%%.17g\n%%.17g\n%%.17g\n", f2.v.v, f2.v.d, f2.d[0].v, f2.d[1].v, f2.d[0].d, f2.d[1].d);
    // the remaining elementary functions at w = x * x + 0.1
    const Tangent r1 = rest(Tangent(x, dx) * Tangent(x, dx) + 0.1);
    TJet<1> U(Tangent(x, dx)); U.d[0] = Tangent(1.0);
    const TJet<1> r2 = rest(U * U + 0.1);
    std::printf("%%.17g\n%%.17g\n%%.17g\n%%.17g\n%%.17g\n%%.17g\n", r1.v, r1.d, r2.v.v, r2.v.d, r2.d[0].v, r2.d[0].d);
    // the traced gradient kind: FitzHugh-Nagumo's f, f., J, J. at P = 3
    Tangent th[3] = {Tangent(0.2, 0.5), Tangent(0.2, -1.0), Tangent(3.0, 0.25)};
    TJet<1> S[2][3], out[2];
    const double v[2] = {-1.0, 1.0}, dv[2] = {0.3, -0.2};
    for (int blk = 0; blk < 2; ++blk) {
        for (int b = 0; b < 2; ++b) for (int j = 0; j < 3; ++j) S[b][j] = TJet<1>(Tangent(j == 0 ? v[b] : 0.5, j == 0 ? dv[b] : 0.1));
        S[blk][0].d[0] = Tangent(1.0);
        G::rhs_generic<TJet<1>, Tangent, 3>(S, 0.0, th, out);
        std::printf("%%.17g\n%%.17g\n%%.17g\n%%.17g\n", out[blk].v.v, out[blk].v.d, out[blk].d[0].v, out[blk].d[0].d);
    }
    return 0;
}
"""


def test_tangent_hpp_on_the_host_against_analytic_derivatives(tmp_path):
    """f, f., J and J. of a few compositions, and the emitted gradient-kind text compiled as host C++."""
    import dalton_grad_oracle as dgr
    src, _ = trace_grad_source(_fitz, 2, 3, (("theta", 3),), "G")
    (tmp_path / "main.cpp").write_text(TANGENT_MAIN % src)
    exe = tmp_path / "tangent_host"
    subprocess.run([_host_compiler(), "-std=c++17", "-O1", "-I", os.path.join(ROOT, "rodeo_amd", "csrc"), str(tmp_path / "main.cpp"),
                    "-o", str(exe), "-lm"], check=True, capture_output=True)
    out = [float(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    x, y, a, dx, dy, da = 0.3, 1.7, -0.8, 0.7, -0.4, 1.3

    def fun(x, y, a):
        return np.exp(x * y) / (1 + a * a) + np.sin(x) * np.log(y) - 2 / a + np.sqrt(y) * np.tanh(a * x)

    def grad(x, y, a):                                                           # (df/dx, df/dy, df/da), analytic
        e, q, sech2 = np.exp(x * y), 1 + a * a, 1 / np.cosh(a * x) ** 2
        return np.array([y * e / q + np.cos(x) * np.log(y) + np.sqrt(y) * a * sech2,
                         x * e / q + np.sin(x) / y + 0.5 / np.sqrt(y) * np.tanh(a * x),
                         -2 * a * e / q ** 2 + 2 / a ** 2 + np.sqrt(y) * x * sech2])

    def hess_dir(x, y, a):                                                       # d/de of (df/dx, df/dy) along (dx, dy, da), analytic
        e, q, th, sech2 = np.exp(x * y), 1 + a * a, np.tanh(a * x), 1 / np.cosh(a * x) ** 2
        fxx = y * y * e / q - np.sin(x) * np.log(y) - 2 * np.sqrt(y) * a * a * th * sech2
        fxy = (1 + x * y) * e / q + np.cos(x) / y + 0.5 / np.sqrt(y) * a * sech2
        fxa = -2 * a * y * e / q ** 2 + np.sqrt(y) * sech2 * (1 - 2 * a * x * th)
        fyy = x * x * e / q - np.sin(x) / y ** 2 - 0.25 * y ** -1.5 * th
        fya = -2 * a * x * e / q ** 2 + 0.5 / np.sqrt(y) * x * sech2
        return np.array([fxx * dx + fxy * dy + fxa * da, fxy * dx + fyy * dy + fya * da])
    g = grad(x, y, a)
    fdot = g @ np.array([dx, dy, da])
    want = [fun(x, y, a), fdot, fun(x, y, a), fdot, g[0], g[1], *hess_dir(x, y, a)]
    w, dw = x * x + 0.1, 2 * x * dx

    def rest(w):
        return np.tan(w) + np.arcsin(w) * np.arccos(w) - np.arctan(w) / np.cosh(w) + np.sinh(w) * np.log1p(w) - np.expm1(w) * np.cos(w)

    def rest1(w):
        r = 1 / np.sqrt(1 - w * w)
        return (1 + np.tan(w) ** 2 + r * np.arccos(w) - np.arcsin(w) * r - 1 / ((1 + w * w) * np.cosh(w))
                + np.arctan(w) * np.sinh(w) / np.cosh(w) ** 2 + np.cosh(w) * np.log1p(w) + np.sinh(w) / (1 + w) - np.exp(w) * np.cos(w)
                + np.expm1(w) * np.sin(w))
    h = 1e-5
    rest2 = (rest1(w + h) - rest1(w - h)) / (2 * h)                              # (the one second derivative taken numerically: 1e-9)
    want += [rest(w), rest1(w) * dw, rest(w), rest1(w) * dw, rest1(w) * 2 * x, rest2 * dw * 2 * x + rest1(w) * 2 * dx]
    X = np.array([[-1.0, 0.5, 0.5], [1.0, 0.5, 0.5]])
    dX = np.array([[0.3, 0.1, 0.1], [-0.2, 0.1, 0.1]])
    f, fd, J, Jd = dgr.fhn_tangent(X, np.array([0.2, 0.2, 3.0]), dX, np.array([0.5, -1.0, 0.25]))
    for blk in range(2):
        want += [f[blk], fd[blk], J[blk, 0], Jd[blk, 0]]
    assert len(out) == len(want)
    for k, (got, ref) in enumerate(zip(out, want)):
        tol = 1e-8 if k == 13 else 1e-13
        assert abs(got - ref) <= tol * max(1.0, abs(ref)), (k, got, ref)
