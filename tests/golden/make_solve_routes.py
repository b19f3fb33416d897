"""Writes tests/golden/solve_routes.npz: the route table of tests/test_abi_and_host.py::solve_route_table (columns: rhs_id
(-1 = the traced user right-hand side), n_block, n_bstate, n_bmeas, interrogate, kalman_type, flags, mode, then the return
code and value of rk_solve_layout, of rk_solve_workspace_bytes, and rk_solve_sizes' return code, mean and var bytes).
Needs a built library, no GPU.  Run from the repository root."""
import os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests.test_abi_and_host import solve_route_table

routes = solve_route_table()
np.savez_compressed(os.path.join(ROOT, "tests", "golden", "solve_routes.npz"), routes=routes)
print("written", routes.shape, "layouts", dict(zip(*np.unique(routes[routes[:, 0] > 0, 9], return_counts=True))))
