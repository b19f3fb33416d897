"""Times of inference.magi_logdens on the headline shape (1024 parameter sets, 4000 steps, d = 2, p = 3, n_active = 2,
tests/magi_oracle.headline), split into its three parts: the host ode_expand loop (one call per parameter set), the
upload of x_0 and the measured components, and the kernel (device events around the launch)."""
import sys, os, time, numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import rodeo_amd as ra
from rodeo_amd.device import batch_minor
import magi_oracle

data, expand, omega, (Q, R) = magi_oracle.headline()
B = omega.shape[0]
dev = ra.device.default_device()
for kalman_type, pars in (("standard", (Q, R)), ("square-root", (Q, np.linalg.cholesky(R)))):
    for rep in range(3):
        dev.sync(); t0 = time.perf_counter()
        states = np.stack([expand(data, omega=omega[b]) for b in range(B)])
        t1 = time.perf_counter()
        x0 = dev.to_device(batch_minor(states[:, 0], True))
        xm = dev.to_device(batch_minor(states[:, 1:, :, :2], True))
        dev.sync(); t2 = time.perf_counter()
        dev.profile_enable(True)
        ll = ra.inference.magi_logdens(data, expand, 2, pars, kalman_type, omega=omega)
        dev.sync(); t3 = time.perf_counter()
        prof = {k: round(v, 4) for k, v in dev.profile_last()}
        print("%s: expand ms %.2f  upload ms %.2f (%.1f MB)  magi_logdens wall ms %.2f  kernel" % (
            kalman_type, (t1 - t0) * 1e3, (t2 - t1) * 1e3, (x0.nbytes + xm.nbytes) / 1e6, (t3 - t2) * 1e3), prof,
            "logdens[:2]", ll[:2], flush=True)
        del x0, xm
