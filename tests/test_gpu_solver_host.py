"""The host side the six solvers beside DORT share (smrt_amd/csrc/solver_host.hpp), through every entry point of each:
one-shot run, split upload / launch / download with a pair list, a refused upload, the context afterwards, the event times
and the release.  Both sides of every comparison are the same kernels on the same inputs, so equality is exact; what the
kernels compute is held to the reference by the solvers' own parity tests."""
import types

import numpy as np
import pytest

from smrt_amd._native import DortContext, PackedBatch, PackedLrmParams
from smrt_amd.core.error import SMRTError

pytestmark = pytest.mark.gpu

THETA = np.deg2rad([30.0, 50.0])
ALTIMETER = types.SimpleNamespace(altitude=800e3, pulse_bandwidth=320e6, antenna_gain=1.0, beamwidth_alongtrack=1.3,
                                  beamwidth_acrosstrack=1.3, off_nadir_angle=0.0, nominal_gate=3, ngate=8)


def small_batch(mode):
    """2 snowpacks of 1 and 3 layers (so that the first is padded to n_layers_max), 1 frequency, 2 angles, 4 streams."""
    return PackedBatch([1, 3], [[10.0, 10.0, 10.0], [0.2, 0.5, 10.0]], [[0.35, 0.35, 0.35], [0.25, 0.3, 0.4]],
                       [[260.0, 260.0, 260.0], [255.0, 260.0, 265.0]], [[2e-4, 2e-4, 2e-4], [1e-4, 2e-4, 3e-4]], None, [13.5e9], THETA,
                       mode=mode, n_max_stream=4, m_max=2)


# prefix of the DortContext methods, sensor mode, arguments after the batch, length of the kernel_ms tuple
SOLVERS = {
    "first_order": ("first_order", "A", lambda: (), 2),
    "second_order": ("second_order", "A", lambda: (), 2),
    "successive_order": ("successive_order", "P", lambda: (2,), 2),
    "successive_order_active": ("so_active", "A", lambda: (THETA, 2), 3),
    "multifresnel": ("multifresnel", "P", lambda: (np.cos(THETA),), 2),
    "nadir_lrm_altimetry": ("lrm", "A", lambda: (PackedLrmParams(ALTIMETER, oversampling=2),), 3),
}


def arrays(out):
    return {k: v for k, v in vars(out).items() if isinstance(v, np.ndarray)}


@pytest.mark.parametrize("solver", list(SOLVERS))
def test_every_entry_point_of_a_solver_on_one_context(solver):
    prefix, mode, make_args, n_ms = SOLVERS[solver]
    call = lambda ctx, role, *a, **kw: getattr(ctx, f"{prefix}_{role}")(*a, **kw)  # noqa: E731
    batch, args = small_batch(mode), make_args()
    ctx = DortContext(0)
    # (a) one shot, every pair
    first = arrays(call(ctx, "run", batch, *args))
    assert first and all(len(v) == 2 for v in first.values())
    # (b) split form with a pair list: row i is row pairs[i] of (a)
    pairs = [1, 0]
    call(ctx, "upload", batch, *args, pairs=pairs)
    call(ctx, "launch")
    call(ctx, "sync")
    listed = arrays(call(ctx, "download"))
    assert listed.keys() == first.keys()
    for name, want in first.items():
        np.testing.assert_array_equal(listed[name], want[pairs], err_msg=name)
    # (c) an upload refused on the host, before any device work
    with pytest.raises(SMRTError, match="pair index out of bounds"):
        call(ctx, "upload", batch, *args, pairs=[2])
    # (d) the context is as usable as before
    again = arrays(call(ctx, "run", batch, *args))
    for name, want in first.items():
        np.testing.assert_array_equal(again[name], want, err_msg=name)
    # (e) the event times of that launch
    ms = call(ctx, "kernel_ms")
    assert isinstance(ms, tuple) and len(ms) == n_ms
    assert all(np.isfinite(t) and t >= 0 for t in ms), ms
    # (f)
    ctx.close()
