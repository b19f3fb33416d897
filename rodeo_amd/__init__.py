"""
rodeo_amd -- MI355X-native Kalman filter / smoother time-stepping core with rodeo's API surface
(``rodeo.solve_mv``, ``rodeo.solve_sim``, ``rodeo.kalmantv``, ``rodeo.interrogate``, ``rodeo.prior``;
src/rodeo/__init__.py:3-6).  Host code is plain Python calling hand-written HIP kernels through the C ABI of
include/rodeo_kalman.h (ctypes); there is no CPU fallback.
"""
__version__ = "0.1.0"
from . import interrogate
from . import prior
from . import kalmantv
from . import ode
from . import utils
from . import inference
from .solve import solve_sim, solve_mv, solve_mv_at, SolvePlan
from .evidence import solve_evidence, evidence_scale, evidence_at, Evidence
from .dynamic import solve_mv_dynamic, solve_sim_dynamic, DynamicMV, DynamicSim
from .grid import solve_mv_grid, solve_sim_grid, grid_slots, grid_with_times
from .grid_calib import solve_evidence_grid, solve_mv_dynamic_grid, solve_sim_dynamic_grid
from .draws import solve_sim_draws
from .grid_draws import solve_sim_draws_grid
from .prior.ibm import ibm_init
from .prior.indep_init import indep_init
from .device import Device, DeviceArray, default_device
