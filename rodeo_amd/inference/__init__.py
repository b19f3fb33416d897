"""
Callers of the hot path (SURVEY.md section 8f "next-1"): ``basic`` (src/rodeo/inference/basic.py) and the device-side
Gaussian observation log-posterior reduction used by pseudo-marginal log-posteriors
(docs/examples/parameter.md:188-210, 331-354), and ``pseudo_marginal``: the random-walk Rosenbluth-Metropolis-Hastings
kernels of src/rodeo/inference/pseudo_marginal.py for many chains in lock-step (SURVEY.md section 8f "next-2").
``fenrir``: the Fenrir likelihood (src/rodeo/inference/fenrir.py:261-327, "next-4").  ``dalton``: the DALTON likelihood
for Gaussian observations and its data-adaptive solver (src/rodeo/inference/dalton.py:39-545; ``rodeo_amd.inference.dalton``
holds ``solve_mv`` / ``solve_sim``).  ``magi_logdens``: the MAGI log-density (src/rodeo/inference/magi.py:6-99;
``rodeo_amd.inference.magi`` is its module).  ``daltonng`` and ``solve_mv_nn`` (non-Gaussian observations, dalton.py:547-1039) live in
``rodeo_amd.inference.dalton`` and are imported from there (``from rodeo_amd.inference.dalton import daltonng``); they are not
re-exported here.  ``laplace``: mode, Hessian and normal approximation of a batched log-posterior by central
differences on the device (docs/examples/parameter.md:239-275; ``rodeo_amd.inference.laplace`` is the module, its function
is ``laplace.laplace``; ``laplace.laplace_grad`` is the same fit on the exact gradients of ``fenrir_grad`` / ``dalton_grad``).
"""
from .basic import basic
from .logpost import gauss_obs_logpost, obs_index, sim_logpost, stage_upars
from . import pseudo_marginal
from .fenrir import fenrir
from .dalton import dalton
from . import magi
from .magi import magi_logdens
from . import laplace
