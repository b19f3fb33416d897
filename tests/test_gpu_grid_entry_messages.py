"""
The refusals of the twelve entries of the non-uniform-grid family that lie behind a served configuration and a real handle: the
``rk_grid_in`` without slots, ``out->mean_state = NULL`` and ``RK_MODE_SIM`` without ``x_state``.  The device is needed for the
handle alone: every call is refused before anything is launched (the handle's launch profile stays empty), and every pointer is
one small device buffer that nothing reads.  The expected texts are written out, as the entries had them before their host sides
were put on the shared pieces of csrc/grid_entry.hpp.  Smallest shapes: FitzHugh-Nagumo, n_bstate 3, n_traj 2, n_steps 2.
"""
import ctypes as C
import pytest
import rodeo_amd as ra
from rodeo_amd import _lib
from test_grid_entry_refusals_host import _obs_id

pytestmark = pytest.mark.gpu

MV, SIM = _lib.MODE_MV, _lib.MODE_SIM

# entry -> (the name its messages open with, has an `out`, has RK_MODE_SIM)
ENTRIES = {
    "rk_solve_grid": ("rk_solve_grid", True, True),
    "rk_solve_evidence_grid": ("rk_solve_evidence_grid", False, False),
    "rk_solve_dynamic_grid": ("rk_solve_dynamic_grid", True, True),
    "rk_solve_sim_draws_grid": ("rk_solve_sim_draws_grid", True, False),
    "rk_dalton_grid_sim_draws": ("rk_dalton_grid_sim_draws", True, False),
    "rk_dalton_grid_loglik": ("rk_dalton_grid_loglik", False, False),
    "rk_dalton_grid_solve": ("rk_dalton_grid_solve", True, True),
    "rk_daltonng_grid_loglik": ("rk_daltonng_grid_loglik", False, False),
    "rk_daltonng_grid_solve": ("rk_daltonng_grid_solve", True, False),
    "rk_fenrir_grid_loglik": ("rk_fenrir_grid_loglik (fenrir_grid)", True, False),
    "rk_fenrir_grid_solve_mv": ("rk_fenrir_grid_solve_mv (fenrir_grid)", True, False),
    "rk_dalton_grid_jvp": ("rk_dalton_grid_jvp", False, False),
}
NO_SLOTS = "%s: grid needs t, slot, q, r and n_slots >= 1 (got 0)"
NO_MEAN = "%s: out->mean_state / var_state must not be NULL"
NO_X = "%s: RK_MODE_SIM needs out->x_state"


def _call(name, h, p, cfg, out, mode, grid):
    """One entry with the served base configuration; `p` stands for every array."""
    lib, c, g = _lib.load(), C.byref(cfg), C.byref(grid)
    sin = _lib.SolveIn(ode_weight=p, ode_init=p, prior_weight=p, prior_var=p, theta=p)
    i, o, oid = C.byref(sin), (C.byref(out) if out is not None else None), _obs_id(2, 3)
    rc = {
        "rk_solve_grid": lambda: lib.rk_solve_grid(h, c, i, o, mode, g),
        "rk_solve_evidence_grid": lambda: lib.rk_solve_evidence_grid(h, c, i, g, p, p, p),
        "rk_solve_dynamic_grid": lambda: lib.rk_solve_dynamic_grid(h, c, i, o, mode, g, 0.0, p, p),
        "rk_solve_sim_draws_grid": lambda: lib.rk_solve_sim_draws_grid(h, c, i, o, g, 1, None, 0, p),
        "rk_dalton_grid_sim_draws": lambda: lib.rk_dalton_grid_sim_draws(h, c, i, o, None, None, None, None, 0, 1, g, 1, None, 0, p),
        "rk_dalton_grid_loglik": lambda: lib.rk_dalton_grid_loglik(h, c, i, None, None, None, None, 0, 1, g, p),
        "rk_dalton_grid_solve": lambda: lib.rk_dalton_grid_solve(h, c, i, o, mode, None, None, None, None, 0, 1, g),
        "rk_daltonng_grid_loglik": lambda: lib.rk_daltonng_grid_loglik(h, c, i, oid, None, None, 0, g, p, 4096, p),
        "rk_daltonng_grid_solve": lambda: lib.rk_daltonng_grid_solve(h, c, i, o, mode, oid, None, None, 0, g),
        "rk_fenrir_grid_loglik": lambda: lib.rk_fenrir_grid_loglik(h, c, i, o, None, None, None, None, 0, 1, g, p),
        "rk_fenrir_grid_solve_mv": lambda: lib.rk_fenrir_grid_solve_mv(h, c, i, o, None, None, None, None, 0, 1, g, p),
        "rk_dalton_grid_jvp": lambda: lib.rk_dalton_grid_jvp(h, c, i, None, None, None, None, 0, 1, g, 1, p, 0, p, 0, p, p),
    }[name]()
    return rc, lib.rk_last_error().decode()


def test_the_refusals_behind_a_served_configuration_keep_their_texts():
    dev = ra.default_device()
    buf = dev.alloc(4096)
    p = buf.value
    cfg = _lib.SolveCfg(n_traj=2, n_steps=2, n_block=2, n_bstate=3, n_bmeas=1, rhs_id=_lib.RHS_FITZHUGH_NAGUMO,
                        interrogate=_lib.INTERROGATE_KRAMER, kalman_type=_lib.KALMAN_STANDARD, n_theta=3, flags=_lib.FLAG_BATCH_MINOR,
                        t_min=0.0, t_max=1.0, seed=0, traj_offset=0)
    grid = _lib.GridIn(t=p, slot=p, q=p, r=p, q_batched=0, r_batched=0, n_slots=1)
    no_slots = _lib.GridIn(t=p, slot=p, q=p, r=p, q_batched=0, r_batched=0, n_slots=0)
    full = _lib.SolveOut(mean_state=p, var_state=p, x_state=p)
    no_mean = _lib.SolveOut(mean_state=None, var_state=p, x_state=p)
    no_x = _lib.SolveOut(mean_state=p, var_state=p, x_state=None)
    dev.profile_enable(True, keep=True)
    try:
        for name, (who, has_out, has_sim) in ENTRIES.items():
            got = [(name, "n_slots = 0", NO_SLOTS % who, _call(name, dev.h, p, cfg, full if has_out else None, MV, no_slots))]
            if has_out:
                got.append((name, "mean_state = NULL", NO_MEAN % who, _call(name, dev.h, p, cfg, no_mean, MV, grid)))
            if has_sim:
                got.append((name, "RK_MODE_SIM, x_state = NULL", NO_X % who, _call(name, dev.h, p, cfg, no_x, SIM, grid)))
            for entry, case, want, (rc, msg) in got:
                print("%s, %s: %d %r" % (entry, case, rc, msg))
                assert rc == _lib.RK_ERR_INVALID and msg == want, (entry, case, rc, msg, want)
        assert dev.profile_last() == []                                     # nothing was launched
    finally:
        dev.profile_enable(False)
        dev.free(buf)
