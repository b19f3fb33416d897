"""
Stochastic block solver for ODE initial value problems on MI355X -- the drop-in for ``rodeo.solve``
(src/rodeo/solve.py): same function names, argument order, keywords and return layouts,

    solve_mv (key, ode_fun, ode_weight, ode_init, t_min, t_max, n_steps, interrogate, prior_pars,
              kalman_type="standard", **params) -> (mean (N+1, d, p), var (N+1, d, p, p))     solve.py:208-302
    solve_sim(... same ...)                     -> x (N+1, d, p)                              solve.py:125-205

plus ``solve_mv_at`` (an addition, below): the same posterior at arbitrary times instead of on the whole grid;
and ONE extension: ``ode_init``, ``prior_pars`` (either matrix), ``ode_weight`` and every ODE parameter may carry a
leading batch axis B of independent trajectories (what a rodeo user writes as ``jax.vmap`` of the solver); outputs
then have a leading B as well.  The forward scan, the interrogation and the backward scan of ALL trajectories run
inside fused HIP kernels (rodeo_amd/csrc/solve_small.hip); nothing is computed on the host and there is no CPU
fallback.

Differences from the reference that a caller can see:
  * ``ode_fun`` is a ``rodeo_amd.ode.DeviceODE`` (device code for the right-hand side) or an ordinary Python function,
    which is traced into device code on first use (``rodeo_amd/trace.py``), and ``interrogate`` one
    of the four functions of ``rodeo_amd.interrogate`` (recognised by identity, ``functools.partial`` allowed);
  * ``key`` is an integer seed (or ``None``) for a Philox counter stream instead of a JAX threefry key -- draws have
    the reference's law, not its bit-stream ("parity unpinned" for draws).
"""
import collections
import ctypes as C
import functools
import numpy as np
from . import _lib, interrogate as _itg
from .device import default_device, batch_minor as _bm
from .ode import DeviceODE

_KALMAN = {"standard": _lib.KALMAN_STANDARD, "square-root": _lib.KALMAN_SQRT}
# layouts whose var_state holds the filtered / smoothed moments as tile records (mean_state unused)
TILE_LAYOUTS = (_lib.LAYOUT_TILE3, _lib.LAYOUT_TILE4, _lib.LAYOUT_TILEP)


def _interrogate_id(interrogate):
    fn = interrogate
    bound = {}
    while isinstance(fn, functools.partial):
        bound.update(fn.keywords or {})
        fn = fn.func
    ids = {_itg.interrogate_rodeo: _lib.INTERROGATE_RODEO, _itg.interrogate_schober: _lib.INTERROGATE_SCHOBER,
           _itg.interrogate_kramer: _lib.INTERROGATE_KRAMER, _itg.interrogate_chkrebtii: _lib.INTERROGATE_CHKREBTII}
    if fn not in ids:
        raise TypeError("interrogate must be one of rodeo_amd.interrogate.interrogate_{rodeo,schober,kramer,chkrebtii} "
                        "(optionally wrapped in functools.partial); arbitrary Python callables cannot run inside the "
                        "GPU time loop")
    return ids[fn], bound


def _seed(key):
    """Integer seed from ``key``: None -> 0; ints pass; a 2-word uint32 array (a JAX-style key) is packed."""
    if key is None:
        return 0
    if isinstance(key, (int, np.integer)):
        return int(key) & 0xFFFFFFFFFFFFFFFF
    k = np.asarray(key).astype(np.uint64).ravel()
    if k.size == 2:
        return int((k[0] << np.uint64(32)) | (k[1] & np.uint64(0xFFFFFFFF)))
    raise TypeError("key must be None, an int seed, or a 2-word uint32 array")


def _device_ode(ode_fun, ode_weight, params):
    """``ode_fun`` as a ``DeviceODE``: an ordinary Python right-hand side, like the reference's, is traced once into device
    code (rodeo_amd/trace.py)."""
    if isinstance(ode_fun, DeviceODE):
        return ode_fun
    if not callable(ode_fun):
        raise TypeError("ode_fun must be a rodeo_amd.ode.DeviceODE or a traceable Python function: the time loop "
                        "runs on the GPU and needs device code for the right-hand side (see rodeo_amd/ode.py); "
                        "there is no CPU fallback")
    from .trace import from_python
    skip = {"kalman_type"}
    sizes = {k: int(np.shape(v)[-1]) if np.ndim(v) >= 1 else 1 for k, v in params.items() if k not in skip}
    return from_python(ode_fun, int(np.shape(ode_weight)[-3]), int(np.shape(ode_weight)[-1]), **sizes)


def _shape_rule(ode_fun, ode_weight, ode_init, prior_pars, params):
    """
    The shape and batch-size rule of a solver call, on the host and in one place (``SolvePlan``, ``solve_mv_at``,
    ``dalton_at`` / ``fenrir_at``): ``ode_fun`` is a ``DeviceODE``; returns ``(W, x0, Q, R, theta, Bt, sizes)`` with the arrays
    as float64, ``(theta, Bt)`` from ``pack_params(params)`` and ``sizes`` the leading batch sizes found (empty: unbatched).
    """
    W = np.asarray(ode_weight, dtype=np.float64)
    x0 = np.asarray(ode_init, dtype=np.float64)
    Q, R = (np.asarray(a, dtype=np.float64) for a in prior_pars)
    if W.ndim not in (3, 4) or x0.ndim not in (2, 3) or Q.ndim not in (3, 4) or R.ndim not in (3, 4):
        raise ValueError("ode_weight (d,m,p), ode_init (d,p), prior_pars (d,p,p) [+ optional leading batch axis]")
    d, m, p = W.shape[-3:]
    if x0.shape[-2:] != (d, p) or Q.shape[-3:] != (d, p, p) or R.shape[-3:] != (d, p, p):
        raise ValueError(f"shape mismatch: ode_weight {W.shape}, ode_init {x0.shape}, prior {Q.shape} / {R.shape}")
    theta, Bt = ode_fun.pack_params(params)
    sizes = [a.shape[0] for a, nd in ((W, 4), (x0, 3), (Q, 4), (R, 4)) if a.ndim == nd]
    if Bt is not None:
        sizes.append(Bt)
    if len(set(sizes)) > 1:
        raise ValueError(f"inconsistent batch sizes {sizes}")
    return W, x0, Q, R, theta, Bt, sizes


class SolvePlan:
    """
    Device-resident form of one solver call: inputs uploaded once in the batch-minor layout, outputs allocated once.
    ``filter() / mv() / sim()`` only enqueue kernels on the device's stream (asynchronous); results stay in HBM as
    ``DeviceArray`` until ``*_host()`` is called.  This is what bench.py times.
    """

    def __init__(self, ode_fun, ode_weight, ode_init, t_min, t_max, n_steps, interrogate, prior_pars,
                 kalman_type="standard", device=None, traj_offset=0, store_pred=False, batch_minor=False, **params):
        if kalman_type not in _KALMAN:
            raise NotImplementedError                    # src/rodeo/solve.py:142-143, 240-241
        ode_fun = _device_ode(ode_fun, ode_weight, params)
        self.dev = device if device is not None else default_device()
        self._ode_fun = ode_fun
        itg_id, bound = _interrogate_id(interrogate)
        if itg_id == _lib.INTERROGATE_CHKREBTII:
            kt = bound.get("kalman_type", params.pop("kalman_type", None) if "kalman_type" in params else None)
            if kt is None:
                raise TypeError("interrogate_chkrebtii needs kalman_type bound with functools.partial "
                                "(src/rodeo/interrogate.py:13-15)")
            if kt not in _KALMAN:
                raise NotImplementedError                # src/rodeo/interrogate.py:43-44
            if kt != kalman_type:
                raise NotImplementedError("interrogate_chkrebtii's kalman_type must equal the solver's kalman_type")
        W, x0, Q, R, theta, Bt, sizes = _shape_rule(ode_fun, ode_weight, ode_init, prior_pars, params)
        d, m, p = W.shape[-3:]
        self.batched = bool(sizes)
        B = sizes[0] if sizes else 1
        if (ode_fun.n_block, ode_fun.n_bmeas) != (d, m):
            raise ValueError(f"ODE '{ode_fun.name}' has (n_block, n_bmeas) = ({ode_fun.n_block}, {ode_fun.n_bmeas}) "
                             f"but ode_weight has ({d}, {m})")
        self.B, self.N, self.d, self.p, self.m = B, int(n_steps), d, p, m
        dev = self.dev
        self._W = dev.to_device(_bm(W, W.ndim == 4))
        self._x0 = dev.to_device(_bm(x0, x0.ndim == 3))
        self._Q = dev.to_device(_bm(Q, Q.ndim == 4))
        self._R = dev.to_device(_bm(R, R.ndim == 4))
        self._theta = dev.to_device(_bm(theta, Bt is not None)) if theta.size else None
        self.cfg = _lib.SolveCfg(n_traj=B, n_steps=self.N, n_block=d, n_bstate=p, n_bmeas=m, rhs_id=ode_fun.rhs_id,
                                 interrogate=itg_id, kalman_type=_KALMAN[kalman_type], n_theta=ode_fun.n_theta,
                                 flags=(_lib.FLAG_STORE_PRED if store_pred else 0) |
                                 (_lib.FLAG_BATCH_MINOR if batch_minor else 0), t_min=float(t_min),
                                 t_max=float(t_max), seed=0, traj_offset=int(traj_offset))
        self.inp = _lib.SolveIn(
            ode_weight=self._W.ptr, ode_weight_batched=int(W.ndim == 4),
            ode_init=self._x0.ptr, ode_init_batched=int(x0.ndim == 3),
            prior_weight=self._Q.ptr, prior_weight_batched=int(Q.ndim == 4),
            prior_var=self._R.ptr, prior_var_batched=int(R.ndim == 4),
            theta=self._theta.ptr if self._theta is not None else None, theta_batched=int(Bt is not None))
        self._store_pred = store_pred
        self.layout = None                 # layout of the last launch (RK_LAYOUT_*), RK_LAYOUT_TILE3 for its packed form too
        self.records_layout = None         # ... as the library reported it: RK_LAYOUT_TILE3_PACKED after a packing mv()
        self.smoothed_tile3 = False        # the records are mv()'s smoothed p = 3 tiles: Sigma is read from its upper triangle
        self.last_mode = None              # RK_MODE_* of the last launch
        self._bufs = {}                    # layout -> (mean_state, var_state)
        self._ws = None                    # device scratch for the dense path
        self.mean_state = self.var_state = self.mean_pred = self.var_pred = self.x_state = None
        self._out = _lib.SolveOut()
        self.generation = 0                # bumped by every launch and every update(): lazily read results check it
        self._x_generation = None          # generation of the launch that last wrote x_state; None: the last sampler stored no path
        self._staged = {}                  # slot -> (signature, device arrays) of staged()
        self._ring, self._ring_calls = [], 0     # result_ring()
        self.upars_dev = None              # inference.stage_upars: the unconstrained parameters the log-posterior reads

    def update(self, ode_init=None, prior_pars=None, **params):
        """
        Replace inputs of the same shapes in place (device buffers and outputs are reused) -- what a sampler does between
        two log-density evaluations: new initial values, prior scales and ODE parameters for every trajectory.
        """
        self.generation += 1
        if ode_init is not None:
            x0 = np.asarray(ode_init, dtype=np.float64)
            self._x0.upload(_bm(x0, x0.ndim == 3))
        if prior_pars is not None:
            Q, R = (np.asarray(a, dtype=np.float64) for a in prior_pars)
            self._Q.upload(_bm(Q, Q.ndim == 4))
            self._R.upload(_bm(R, R.ndim == 4))
        if params:
            theta, Bt = self._ode_fun.pack_params(params)
            if self._theta is None:
                raise TypeError("this ODE has no parameters")
            self._theta.upload(_bm(theta, Bt is not None))

    def solve_layout(self, mode, packed_mv=False):
        """rk_solve_layout of this plan for ``mode``.  ``packed_mv`` (mv() at n_bstate = 3) sets RK_FLAG_TILE3_PACKED_MV in the
        plan's cfg, any other query clears it: the flag stands in ``cfg`` exactly while the plan's records may be packed."""
        self.cfg.flags = (self.cfg.flags & ~_lib.FLAG_TILE3_PACKED_MV) | (_lib.FLAG_TILE3_PACKED_MV if packed_mv else 0)
        lay = C.c_int32(0)
        _lib.check(self.dev.lib.rk_solve_layout(C.byref(self.cfg), mode, C.byref(lay)))
        return lay.value

    def _prepare_out(self, mode, path=True, packed_mv=False):
        """Ask the library which layout this call uses and (once) allocate the outputs for it.  ``path=False``: a sampler launch
        that stores no path -- x_state is neither allocated nor handed to the library, and the plan holds no path afterwards.
        RK_LAYOUT_TILE3_PACKED is RK_LAYOUT_TILE3 with records packed in place: ONE buffer serves both, so filter() and mv() on
        one plan keep working in place."""
        self.records_layout = lay = self.solve_layout(mode, packed_mv)
        if lay == _lib.LAYOUT_TILE3_PACKED:
            lay = _lib.LAYOUT_TILE3
        dev, N1, d, p, B = self.dev, self.N + 1, self.d, self.p, self.B
        if lay not in self._bufs:
            if lay == _lib.LAYOUT_TILE3:
                mb, vb = C.c_size_t(0), C.c_size_t(0)
                _lib.check(dev.lib.rk_solve_sizes(C.byref(self.cfg), lay, C.byref(mb), C.byref(vb)))
                self._bufs[lay] = (None, dev.empty((N1, B, d, 3, 4), pad_bytes=vb.value - N1 * B * d * 96))  # + scratch tail
            elif lay == _lib.LAYOUT_TILE4:
                mb, vb = C.c_size_t(0), C.c_size_t(0)
                _lib.check(dev.lib.rk_solve_sizes(C.byref(self.cfg), lay, C.byref(mb), C.byref(vb)))
                self._bufs[lay] = (None, dev.empty((N1, B, d, 20), pad_bytes=vb.value - N1 * B * d * 160))
            elif lay == _lib.LAYOUT_TILEP:                                   # blocked tiles, n_bstate = 5 .. 8: [Sigma | mu]
                self._bufs[lay] = (None, dev.empty((N1, B, d, p * p + p)))
            elif lay == _lib.LAYOUT_TRAJ_MAJOR:
                self._bufs[lay] = (dev.empty((B, N1, d, p)), dev.empty((B, N1, d, p, p)))
            else:
                self._bufs[lay] = (dev.empty((N1, d, p, B)), dev.empty((N1, d, p, p, B)))
        self.layout = lay
        self.mean_state, self.var_state = self._bufs[lay]
        if self._store_pred and self.mean_pred is None:
            if lay == _lib.LAYOUT_TRAJ_MAJOR:                                 # the dense path keeps the reference's own layout
                self.mean_pred, self.var_pred = dev.empty((B, N1, d, p)), dev.empty((B, N1, d, p, p))
            else:
                self.mean_pred, self.var_pred = dev.empty((N1, d, p, B)), dev.empty((N1, d, p, p, B))
        if mode == _lib.MODE_SIM:
            if path and self.x_state is None:
                self.x_state = dev.empty((N1, d, p, B))
            self._x_generation = self.generation if path else None     # (no path: what x_state holds is an earlier draw's)
        wsb = C.c_size_t(0)
        _lib.check(self.dev.lib.rk_solve_workspace_bytes(C.byref(self.cfg), mode, C.byref(wsb)))
        if wsb.value and (self._ws is None or self._ws.nbytes < wsb.value):
            try:
                self._ws = dev.empty((wsb.value // 8,))
            except Exception:
                # The records of the square-root small-block path's two-kernel backward pass are OPTIONAL (include/rodeo_kalman.h:
                # without them the one-kernel form runs, same results, about twice the time) and large -- N d (3 p^2 + p) B
                # doubles, 13 GB at the headline shape with p = 8.  Every other workspace is required: re-raise.
                optional = (self.cfg.kalman_type == _lib.KALMAN_SQRT and self.layout == _lib.LAYOUT_BATCH_MINOR and
                            mode != _lib.MODE_FILTER)
                if not optional:
                    raise
                self._ws = None
        self._out = _lib.SolveOut(
            workspace=self._ws.ptr if self._ws is not None else None,
            workspace_bytes=self._ws.nbytes if self._ws is not None else 0,
            mean_state=self.mean_state.ptr if self.mean_state is not None else None, var_state=self.var_state.ptr,
            mean_pred=self.mean_pred.ptr if self.mean_pred is not None else None,
            var_pred=self.var_pred.ptr if self.var_pred is not None else None,
            x_state=self.x_state.ptr if path and self.x_state is not None else None)

    # ---- launches (asynchronous) ----
    def launch(self, fn, key, mode, *extra, path=True, packed_mv=False):
        """The one way a library entry writes this plan's outputs: ``fn(handle, cfg, in, out, *extra)`` after the bookkeeping
        every such launch owes -- generation, outputs of ``mode``'s layout, last_mode, seed.  ``path=False``: see _prepare_out;
        ``packed_mv``: see solve_layout (mv() alone)."""
        self.generation += 1               # whatever is in the output buffers now belongs to an earlier call
        self._prepare_out(mode, path, packed_mv)
        self.smoothed_tile3 = packed_mv and self.layout == _lib.LAYOUT_TILE3
        self.last_mode = mode
        self.set_seed(key)
        _lib.check(fn(self.dev.h, C.byref(self.cfg), C.byref(self.inp), C.byref(self._out), *extra))

    def set_seed(self, key):
        """The seed of the next launch -- all that an entry which leaves the plan's outputs alone (dalton, daltonng) sets."""
        self.cfg.seed = _seed(key)

    def filter(self, key=None):
        self.launch(self.dev.lib.rk_solve_filter, key, _lib.MODE_FILTER)

    def mv(self, key=None):
        self.launch(self.dev.lib.rk_solve_mv, key, _lib.MODE_MV, packed_mv=self.p == 3)

    def sim(self, key=None):
        self.launch(self.dev.lib.rk_solve_sim, key, _lib.MODE_SIM)

    def sync(self):
        self.dev.sync()

    # ---- staging for the inference callers (observations in, a few doubles per trajectory out) ----
    def staged(self, slot, *arrays):
        """Device copies of ``arrays`` (made C-contiguous), uploaded again only when a shape or a byte differs from the last call
        with this ``slot``: a sampler calls with the same observations once per step.  One slot per caller, so callers that
        alternate on one cached plan do not evict each other."""
        arrays = [np.ascontiguousarray(a) for a in arrays]
        sig = tuple((a.shape, a.tobytes()) for a in arrays)
        if self._staged.get(slot, (None,))[0] != sig:
            self._staged[slot] = (sig, tuple(self.dev.to_device(a) for a in arrays))
        return self._staged[slot][1]

    def result_ring(self):
        """The next of four (B,) result buffers owned by the plan (a device allocation per call cost more than the reduction
        kernel: 0.08 of C4's 0.32 ms per evaluation): overwritten by the FOURTH call after this one, so for callers that read
        the result at once.  A change of B starts a new ring."""
        if self._ring and tuple(self._ring[0].shape) != (self.B,):
            self._ring, self._ring_calls = [], 0
        if len(self._ring) < 4:
            self._ring.append(self.dev.empty((self.B,)))
        self._ring_calls += 1
        return self._ring[(self._ring_calls - 1) % 4]     # call 5 reuses the buffer of call 1, call 6 that of call 2, ...

    def per_traj(self, out):
        """A device array (B,) of per-trajectory values on the host: the array for a batched plan, else a float."""
        vals = out.to_host()
        return vals if self.batched else float(vals[0])

    # ---- results in the reference's layouts ----
    def _host(self, arr):
        a = arr.batch_first()                       # (B, N+1, ...)
        return a if self.batched else a[0]

    def records_mean_var(self, t):
        """(mean, var) views of tile records t (..., d, record) in this plan's layout: RK_LAYOUT_TILE3 rows [Sigma | mu]
        (3, 4); RK_LAYOUT_TILE4 and RK_LAYOUT_TILEP one format, [Sigma row-major (p*p) | mu (p)]."""
        if self.layout == _lib.LAYOUT_TILE3:
            return t[..., 3], t[..., :3]
        p = self.p
        return t[..., p * p:], t[..., :p * p].reshape(t.shape[:-1] + (p, p))

    # ---- smoothed p = 3 tiles on the host: packed records (RK_LAYOUT_TILE3_PACKED, include/rodeo_kalman.h) and the mirror rule ----
    def packed_waves(self):
        """Leading tile-waves (four tiles each, tile = b d + block) whose steps 1 .. N-1 are packed records in var_state; 0 when
        nothing is packed.  The size rule is the library's (rk_tile3_packed_waves)."""
        if self.records_layout != _lib.LAYOUT_TILE3_PACKED:
            return 0
        return int(self.dev.lib.rk_tile3_packed_waves(self.N, self.B * self.d))

    @staticmethod
    def _tile3_fill(t, rec):
        """Natural tiles t (..., 3, 4) from packed records rec (..., 9) = [S00 S01 S02 S11 S12 S22 | mu]: the symmetric Sigma
        (both triangles) and the mean."""
        for slot, (i, j) in enumerate(((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2), (0, 3), (1, 3), (2, 3))):
            t[..., i, j] = rec[..., slot]
            if i < j < 3:
                t[..., j, i] = rec[..., slot]

    def _tile3_mirror(self, t):
        """Sigma's lower triangle from the upper one, in place, for mv()'s smoothed tiles in BOTH layouts: a packed record holds
        no lower triangle, and the natural one differs from the upper in the last bit."""
        if self.smoothed_tile3:
            for i, j in ((0, 1), (0, 2), (1, 2)):
                t[..., j, i] = t[..., i, j]
        return t

    def tile3_unpack(self, raw, waves):
        """``raw`` (N+1, B, d, 3, 4) as downloaded, with the steps 1 .. N-1 of the first ``waves`` tile-waves packed: the natural
        tiles, in place.  The groups of four steps are three whole stripe rows each, so the gather is two reshapes."""
        N, T = self.N, self.B * self.d
        if waves:
            K = ((N - 1) >> 2) + 1                                             # groups 0 .. K-1 hold the steps 1 .. N-1
            grp = raw.reshape(N + 1, T * 12)[1:1 + 3 * K, :waves * 48].reshape(K, 3, waves, 48)
            grp = grp.transpose(0, 2, 1, 3).reshape(K, waves, 4, 4, 9)          # (group, tile-wave, step, tile, slot)
            rec = grp.transpose(0, 2, 1, 3, 4).reshape(4 * K, 4 * waves, 9)[1:N].copy()     # (a view of raw at one tile-wave)
            self._tile3_fill(raw.reshape(N + 1, T, 3, 4)[1:N, :4 * waves], rec)
        return raw

    def tile3_row_host(self, n):
        """The natural tiles (B, d, 3, 4) of time row ``n`` of a RK_LAYOUT_TILE3 plan, whatever the records' layout: a packed
        step lies in one or two stripe rows, and only those are downloaded."""
        N, T, waves = self.N, self.B * self.d, self.packed_waves()
        n = int(n) % (N + 1)
        if not (waves and 1 <= n < N):
            return self._tile3_mirror(self.var_state.slice0_host(n))
        t = self.var_state.slice0_host(n) if 4 * waves < T else np.empty((self.B, self.d, 3, 4))     # (a ragged last tile-wave)
        k, lo = n >> 2, (n & 3) * 36                                            # the step's 4 x 9 doubles inside the group's 3 x 48
        r0, r1 = lo // 48, (lo + 35) // 48
        rows = [self.var_state.slice0_host(3 * k + 1 + r).reshape(-1)[:waves * 48].reshape(waves, 48) for r in range(r0, r1 + 1)]
        rec = np.concatenate(rows, axis=1)[:, lo - 48 * r0:lo - 48 * r0 + 36].reshape(4 * waves, 9)
        self._tile3_fill(t.reshape(T, 3, 4)[:4 * waves], rec)
        return self._tile3_mirror(t)

    def mean_rows_host(self, ind):
        """The posterior means (B, len(ind), d, p) at the time indices ``ind``: only the rows needed are downloaded."""
        rows = []
        for n in ind:
            if self.layout == _lib.LAYOUT_TILE3:
                rows.append(self.tile3_row_host(n)[..., 3])
            elif self.layout in TILE_LAYOUTS:
                rows.append(self.records_mean_var(self.var_state.slice0_host(int(n)))[0])      # (B, d, p) means
            elif self.layout == _lib.LAYOUT_TRAJ_MAJOR:
                rows.append(self.mean_state.to_host()[:, int(n)])
            else:
                rows.append(np.moveaxis(self.mean_state.slice0_host(int(n)), -1, 0))           # (d, p, B) -> (B, d, p)
        return np.stack(rows, axis=1)

    def state_host(self):
        """(mean, var) of the last filter() / mv() in the reference layout (views of one download, no transposes; packed p = 3
        records are gathered into their natural tiles first)."""
        if self.layout in TILE_LAYOUTS:
            raw = self.var_state.to_host()
            if self.layout == _lib.LAYOUT_TILE3:
                raw = self._tile3_mirror(self.tile3_unpack(raw, self.packed_waves()))
            mean, var = self.records_mean_var(np.moveaxis(raw, 1, 0))                          # (B, N+1, d, ...)
            return (mean, var) if self.batched else (mean[0], var[0])
        if self.layout == _lib.LAYOUT_TRAJ_MAJOR:                    # already the reference layout
            mean, var = self.mean_state.to_host(), self.var_state.to_host()
            return (mean, var) if self.batched else (mean[0], var[0])
        return self._host(self.mean_state), self._host(self.var_state)

    def pred_host(self):
        if self.layout == _lib.LAYOUT_TRAJ_MAJOR:
            mean, var = self.mean_pred.to_host(), self.var_pred.to_host()
            return (mean, var) if self.batched else (mean[0], var[0])
        return self._host(self.mean_pred), self._host(self.var_pred)

    def _require_path(self):
        """x_state must hold the path of the last sampler launch (sim(), dalton's solve_sim, sim_logpost with a path)."""
        if self.x_state is None or self._x_generation is None:
            raise RuntimeError("this plan holds no path of its last sampler launch: a path-less sim_logpost stores none, "
                               "and what an earlier sim() left in x_state belongs to another draw; call sim(key) or "
                               "sim_logpost(..., keep_path=True) before reading the path")

    def x_host(self):
        self._require_path()
        return self._host(self.x_state)

    # algorithmic HBM bytes per trajectory-step
    def bytes_per_traj_step(self, kind="mv"):
        d, p = self.d, self.p
        return 3 * d * p * (p + 1) * 8 if kind == "mv" else (2 * d * p * (p + 1) + d * p) * 8


_plan_cache = collections.OrderedDict()     # a few device-resident plans, reused when only the numbers change


def cached_plan(ode_fun, ode_weight, ode_init, t_min, t_max, n_steps, interrogate, prior_pars, kalman_type="standard",
                store_pred=False, batch_minor=False, **params):
    """
    The device-resident ``SolvePlan`` of an earlier call with the same static configuration (ODE, grid, interrogation,
    weight matrix, array shapes, flags) with its inputs replaced in place (``SolvePlan.update``), or a new one.  For the
    callers that bring back a few doubles per trajectory and are called in a loop (``inference.basic``, ``fenrir``):
    rebuilding the plan would cost more than the kernels.  At most four plans are kept.
    """
    W = np.asarray(ode_weight, dtype=np.float64)
    shapes = tuple((k, np.shape(v)) for k, v in sorted(params.items()))
    itg = getattr(interrogate, "func", interrogate), tuple(sorted(getattr(interrogate, "keywords", {}).items()))
    key = (id(ode_fun), W.shape, W.tobytes(), np.shape(ode_init), tuple(np.shape(a) for a in prior_pars), float(t_min),
           float(t_max), int(n_steps), itg, kalman_type, bool(store_pred), bool(batch_minor), shapes)
    plan = _plan_cache.get(key)
    if plan is not None:
        _plan_cache.move_to_end(key)
        plan.update(ode_init=ode_init, prior_pars=prior_pars, **params)
        return plan
    plan = SolvePlan(ode_fun, ode_weight, ode_init, t_min, t_max, n_steps, interrogate, prior_pars, kalman_type,
                     store_pred=store_pred, batch_minor=batch_minor, **params)
    plan._keep_ode = ode_fun                 # the key holds id(ode_fun): keep the object alive with the plan
    _plan_cache[key] = plan
    while len(_plan_cache) > 4:
        _plan_cache.popitem(last=False)
    return plan


def _solve_filter(key, ode_fun, ode_weight, ode_init, t_min, t_max, n_steps, interrogate,
                  prior_weight, prior_var, kalman_funs=None, **params):
    """
    Forward pass (src/rodeo/solve.py:31-122).  Returns the reference's dict:
    ``{"state_pred": (mean, var), "state_filt": (mean, var)}``, each of time length ``n_steps + 1`` with index 0 equal
    to ``(ode_init, 0)``.  ``kalman_funs`` may be the module ``rodeo_amd.kalmantv.standard`` (default).
    """
    kalman_type = "standard"
    if kalman_funs is not None and getattr(kalman_funs, "KALMAN_TYPE", "standard") != "standard":
        kalman_type = kalman_funs.KALMAN_TYPE
    plan = SolvePlan(ode_fun, ode_weight, ode_init, t_min, t_max, n_steps, interrogate, (prior_weight, prior_var),
                     kalman_type, store_pred=True, **params)
    plan.filter(key)
    return {"state_pred": plan.pred_host(), "state_filt": plan.state_host()}


def _pad_two_to_three(ode_weight, ode_init, prior_pars):
    """
    n_bstate = 2 has no MFMA-tile kernels of its own; it runs on the n_bstate = 3 ones with a third state component that
    is decoupled from the other two: Q = diag(Q, 1), R = diag(R, 1), zero weight, zero initial value.  Its cross
    covariances start as exact zeros and stay exact zeros (products with and sums of zeros), the pivoted LU never picks
    its row for the other two columns, and the draws of the first two components use the same normals -- so the leading
    2 x 2 part is the n_bstate = 2 computation, term for term.
    """
    W, x0 = np.asarray(ode_weight, dtype=np.float64), np.asarray(ode_init, dtype=np.float64)
    Q, R = (np.asarray(a, dtype=np.float64) for a in prior_pars)

    def grow(M):                                        # (..., 2, 2) -> (..., 3, 3) with a one in the corner
        out = np.zeros(M.shape[:-2] + (3, 3))
        out[..., :2, :2] = M
        out[..., 2, 2] = 1.0
        return out
    W3 = np.concatenate([W, np.zeros(W.shape[:-1] + (1,))], axis=-1)
    x3 = np.concatenate([x0, np.zeros(x0.shape[:-1] + (1,))], axis=-1)
    return W3, x3, (grow(Q), grow(R))


def _two_state_on_tiles(ode_weight, kalman_type):
    W = np.shape(ode_weight)
    return kalman_type == "standard" and len(W) >= 3 and W[-1] == 2 and W[-2] == 1


def solve_mv(key, ode_fun, ode_weight, ode_init, t_min, t_max, n_steps, interrogate, prior_pars,
             kalman_type="standard", **params):
    """Mean and variance of the stochastic ODE solver (src/rodeo/solve.py:208-302)."""
    if _two_state_on_tiles(ode_weight, kalman_type):
        W3, x3, pp3 = _pad_two_to_three(ode_weight, ode_init, prior_pars)
        m, v = solve_mv(key, ode_fun, W3, x3, t_min, t_max, n_steps, interrogate, pp3, kalman_type, **params)
        return np.ascontiguousarray(m[..., :2]), np.ascontiguousarray(v[..., :2, :2])
    plan = SolvePlan(ode_fun, ode_weight, ode_init, t_min, t_max, n_steps, interrogate, prior_pars, kalman_type,
                     **params)
    plan.mv(key)
    return plan.state_host()


def solve_sim(key, ode_fun, ode_weight, ode_init, t_min, t_max, n_steps, interrogate, prior_pars,
              kalman_type="standard", **params):
    """Draw one sample solution per trajectory (src/rodeo/solve.py:125-205)."""
    if _two_state_on_tiles(ode_weight, kalman_type):
        W3, x3, pp3 = _pad_two_to_three(ode_weight, ode_init, prior_pars)
        return np.ascontiguousarray(solve_sim(key, ode_fun, W3, x3, t_min, t_max, n_steps, interrogate, pp3, kalman_type,
                                              **params)[..., :2])
    plan = SolvePlan(ode_fun, ode_weight, ode_init, t_min, t_max, n_steps, interrogate, prior_pars, kalman_type,
                     **params)
    plan.sim(key)
    return plan.x_host()


# ---- the posterior at arbitrary times ---------------------------------------------------------------------------------
EVAL_AT_NODE_TOL = 1e-10      # a time within this many steps of a node is that node
EVAL_AT_PRIOR_TOL = 1e-10     # Chapman-Kolmogorov residual of prior_at, relative to each matrix's largest entry
EVAL_AT_BSTATE = (3, 5)       # n_bstate served by rk_eval_at (2 runs padded to 3); at 6 the lane kernel spills


def eval_at_nodes(t_eval, t_min, t_max, n_steps):
    """
    Where the times ``t_eval`` sit on the solver's grid t_n = t_min + (t_max - t_min) n / N: ``(node, on_node, h1, h2)``.
    A time within 1e-10 of a step from a node is that node (``on_node``, h1 = h2 = 0); any other lies in
    (t_node, t_node+1) with h1 = t - t_node and h2 = t_node+1 - t.  Empty, non-finite and outside times raise ValueError.
    """
    t = np.asarray(t_eval, dtype=np.float64)
    if t.ndim != 1 or t.size == 0:
        raise ValueError(f"t_eval must be a non-empty 1-D array of times, got shape {t.shape}")
    if not np.all(np.isfinite(t)):
        raise ValueError("t_eval holds a non-finite time")
    if np.any(t < t_min) or np.any(t > t_max):
        raise ValueError(f"t_eval must lie in [t_min, t_max] = [{t_min}, {t_max}], got [{t.min()}, {t.max()}]")
    N = int(n_steps)
    x = (t - t_min) / ((t_max - t_min) / N)
    near = np.rint(x)
    on = np.abs(x - near) <= EVAL_AT_NODE_TOL
    node = np.where(on, np.clip(near, 0, N), np.clip(np.floor(x), 0, N - 1)).astype(np.int64)

    def grid(n):
        return t_min + (t_max - t_min) * n / N
    return node, on, np.where(on, 0.0, t - grid(node)), np.where(on, 0.0, grid(node + 1) - t)


def check_prior_at(first, second, prior_pars, h1, h2):
    """
    Chapman-Kolmogorov consistency of ``first = prior_at(h1)`` and ``second = prior_at(h2)`` with the full step's
    ``prior_pars``: Q2 Q1 = Q and Q2 R1 Q2^T + R2 = R, each to 1e-10 of the block matrix's largest entry (a ``prior_at``
    built with another sigma or another prior fails it).  Raises ValueError; returns the two residuals (relative).
    """
    (Q1, R1), (Q2, R2) = first, second
    Q, R = (np.asarray(a, dtype=np.float64) for a in prior_pars)
    Q2t = np.swapaxes(Q2, -1, -2)
    res = []
    for name, got, want in (("Q2 Q1 = Q", np.matmul(Q2, Q1), Q), ("Q2 R1 Q2^T + R2 = R", np.matmul(np.matmul(Q2, R1), Q2t) + R2, R)):
        scale = np.max(np.abs(want), axis=(-1, -2))
        err = np.max(np.abs(got - want), axis=(-1, -2))
        if not np.all(err <= EVAL_AT_PRIOR_TOL * scale):
            raise ValueError(f"prior_at is inconsistent with prior_pars: {name} fails by {np.max(err / scale):.3e} of the matrix's "
                             f"largest entry at h1 = {h1}, h2 = {h2} (the bar is {EVAL_AT_PRIOR_TOL}); it must be the prior that "
                             "prior_pars was built from, over a step of the given length")
        res.append(float(np.max(err / scale)))
    return tuple(res)


def _prior_at_pair(prior_at, h, d, p, B):
    out = prior_at(float(h))
    try:
        Qh, Rh = (np.asarray(a, dtype=np.float64) for a in out)
    except (TypeError, ValueError):
        raise ValueError("prior_at(dt) must return the pair (wgt_state, var_state)") from None
    for a in (Qh, Rh):
        if a.ndim not in (3, 4) or a.shape[-3:] != (d, p, p) or (a.ndim == 4 and a.shape[0] != B):
            raise ValueError(f"prior_at(dt) must return matrices of shape ({d}, {p}, {p}) or (B, {d}, {p}, {p}) with the call's "
                             f"batch size, got {Qh.shape} and {Rh.shape}")
    return Qh, Rh


def _stack_prior(mats, B):
    """(n_quad, 2, d, p, p) matrices, each (d, p, p) or (B, d, p, p) -> the array rk_eval_at reads and its batched flag."""
    batched = any(m.ndim == 4 for pair in mats for m in pair)
    if not batched:
        return np.array(mats), 0
    full = np.array([[np.broadcast_to(m, (B,) + m.shape[-3:]) for m in pair] for pair in mats])     # (n_quad, 2, B, d, p, p)
    return np.ascontiguousarray(np.moveaxis(full, 2, -1)), 1


def solve_mv_at(key, ode_fun, ode_weight, ode_init, t_min, t_max, n_steps, interrogate, prior_pars, t_eval, prior_at,
                kalman_type="standard", **params):
    """
    Mean and variance of the solver's posterior at the times ``t_eval`` (an addition: the reference's ``solve_mv`` returns
    its grid only).  The first nine arguments are ``solve_mv``'s, with the same meaning and batching rules.

    ``t_eval`` (T,) holds times in [t_min, t_max] in any order, repeats allowed; the output follows it.  A time within
    1e-10 of a step from a grid node is that node and gets ``solve_mv``'s own value, bit for bit.  Any other time t in
    (t_n, t_n+1) gets the closed form that the prior's Markov property gives -- nothing is interrogated between nodes:
    predict from the filtered moments at t_n over h1 = t - t_n, then one ``smooth_mv`` step against the smoothed moments at
    t_n+1 over h2 = t_n+1 - t.  ``prior_at(dt)`` returns the prior ``(wgt_state, var_state)`` for a step of length dt, in
    the shapes ``prior_pars`` may have (for the IBM prior ``lambda h: ibm_init(h, n_deriv, sigma)``): a sub-step's
    transition cannot be recovered from the full step's.  It is called for h1 and h2 of every distinct off-grid time (not
    at all when every time is a node) and checked against ``prior_pars`` (``check_prior_at``).

    Returns ``mean (T, d, p)`` and ``var (T, d, p, p)``, with a leading B under ``solve_mv``'s rule.

    Two plans run on the device, ``filter()`` and ``mv()`` with the same key (``mv()`` overwrites its filter records in
    place, and the counter RNG keys draws by trajectory and step, so interrogate_chkrebtii sees the same draws in both):
    TWO sets of (N+1)-point records are held on the device at once; ``eval_at_kernel`` reads them there and only the T
    records per trajectory are downloaded.  Served: kalman_type "standard", n_bstate 2..5, every route of ``solve_mv`` but the
    dense one; everything else raises before any device work.  ``batch_minor=True`` (a keyword of the plan, not an ODE
    parameter) forces the batch-minor kernels where a tile route exists, as in ``SolvePlan``.
    """
    if kalman_type not in _KALMAN:
        raise NotImplementedError                        # src/rodeo/solve.py:240-241
    if kalman_type != "standard":
        raise NotImplementedError("solve_mv_at: kalman_type='square-root' is not built")
    batch_minor = bool(params.pop("batch_minor", False))
    node, on, h1, h2 = eval_at_nodes(t_eval, t_min, t_max, n_steps)
    W = np.asarray(ode_weight, dtype=np.float64)
    if W.ndim not in (3, 4):
        raise ValueError("ode_weight (d,m,p), ode_init (d,p), prior_pars (d,p,p) [+ optional leading batch axis]")
    ode_fun = _device_ode(ode_fun, W, params)
    W, x0, Q, R, theta, Bt, sizes = _shape_rule(ode_fun, W, ode_init, prior_pars,
                                                 {k: v for k, v in params.items() if k != "kalman_type"})
    d, m, p = W.shape[-3:]
    two = _two_state_on_tiles(W, kalman_type)
    if not (two or EVAL_AT_BSTATE[0] <= p <= EVAL_AT_BSTATE[1]):
        raise NotImplementedError(f"solve_mv_at: n_bstate = {p} is outside the served range 2..{EVAL_AT_BSTATE[1]} (2 with "
                                  "n_bmeas = 1 only; beyond, the lane kernel spills)")
    itg_id, _ = _interrogate_id(interrogate)
    B = sizes[0] if sizes else 1
    cfg = _lib.SolveCfg(n_traj=B, n_steps=int(n_steps), n_block=d, n_bstate=3 if two else p, n_bmeas=m, rhs_id=ode_fun.rhs_id,
                        interrogate=itg_id, kalman_type=_KALMAN[kalman_type], n_theta=ode_fun.n_theta,
                        flags=_lib.FLAG_BATCH_MINOR if batch_minor else 0, t_min=float(t_min), t_max=float(t_max), seed=0,
                        traj_offset=0)
    lay = C.c_int32(0)
    _lib.check(_lib.load().rk_solve_layout(C.byref(cfg), _lib.MODE_MV, C.byref(lay)))
    if lay.value == _lib.LAYOUT_TRAJ_MAJOR:
        raise NotImplementedError("solve_mv_at: the dense (indep_init) route keeps trajectory-major records, which eval_at_kernel "
                                  "does not read")
    # one (Q1, R1, Q2, R2) quadruple per distinct off-grid time
    slot = np.zeros(len(node), dtype=np.int64)
    trans, noise = [], []
    if not np.all(on):
        times = np.asarray(t_eval, dtype=np.float64)
        _, first, inverse = np.unique(times[~on], return_index=True, return_inverse=True)
        slot[~on] = inverse
        for k in first:
            a1, a2 = h1[~on][k], h2[~on][k]
            one, other = _prior_at_pair(prior_at, a1, d, p, B), _prior_at_pair(prior_at, a2, d, p, B)
            check_prior_at(one, other, (Q, R), a1, a2)
            if two:
                one, other = (_pad_two_to_three(W, x0, pair)[2] for pair in (one, other))
            trans.append((one[0], other[0]))
            noise.append((one[1], other[1]))
    else:
        pp = 3 if two else p
        trans = noise = [(np.zeros((d, pp, pp)),) * 2]                   # one slot that no query reads
    if two:
        W, x0, (Q, R) = _pad_two_to_three(W, x0, (Q, R))
    mean, var = _eval_at_device(key, ode_fun, W, x0, t_min, t_max, n_steps, interrogate, (Q, R), kalman_type, node, on, slot,
                                _stack_prior(trans, B), _stack_prior(noise, B), batch_minor, params)
    if two:
        return np.ascontiguousarray(mean[..., :2]), np.ascontiguousarray(var[..., :2, :2])
    return mean, var


def _eval_at_device(key, ode_fun, W, x0, t_min, t_max, n_steps, interrogate, prior_pars, kalman_type, node, on, slot, trans,
                    noise, batch_minor, params):
    """The device side of ``solve_mv_at``: the two plans, the query upload, rk_eval_at and the download of T records."""
    plans = [SolvePlan(ode_fun, W, x0, t_min, t_max, n_steps, interrogate, prior_pars, kalman_type, batch_minor=batch_minor,
                       **params) for _ in range(2)]
    filt, smooth = plans
    filt.filter(key)
    smooth.mv(key)
    if filt.layout != smooth.layout:
        raise NotImplementedError(f"solve_mv_at: filter and mv records in different layouts ({filt.layout}, {smooth.layout})")
    dev = filt.dev
    query = dev.to_device(np.stack([node, on.astype(np.int64), slot], axis=1).astype(np.int32))
    trans_dev, noise_dev = dev.to_device(trans[0]), dev.to_device(noise[0])
    T = len(node)
    mean, var = dev.empty((filt.B, T, filt.d, filt.p)), dev.empty((filt.B, T, filt.d, filt.p, filt.p))
    q = _lib.EvalAtIn(n_query=T, n_quad=int(trans[0].shape[0]), query=query.ptr, trans=trans_dev.ptr, trans_batched=trans[1],
                      noise=noise_dev.ptr, noise_batched=noise[1])
    # (the smoother's records may be the packed form of the filter's layout: rk_eval_at takes that id and reads `filt` as natural)
    _lib.check(dev.lib.rk_eval_at(dev.h, C.byref(filt.cfg), smooth.records_layout, C.byref(filt._out), C.byref(smooth._out), C.byref(q),
                                  mean.ptr, var.ptr))
    m, v = mean.to_host(), var.to_host()
    return (m, v) if filt.batched else (m[0], v[0])
