"""Batches for the comparison of the two prep stages of the LDS-resident passive pipeline (per pair / per layer):
tests/test_prep_layer_cpu.py (emulator) and tests/test_gpu_prep_layer.py (device) use the same ones.

Row counts.  A layer has as many streams as Gauss-Legendre nodes below its critical angle against the most refringent
layer of the snowpack (streams.py:136-223).  At 37 GHz and 260 K next to a layer of ice fraction 0.56, with 32 streams per
hemisphere, the fractions below give 16, 17, 24, 25 and 32 streams: 32, 34, 48, 50 and 64 rows -- both sides of the two
class boundaries (0, 32], (32, 48], (48, 64] and the largest size (the tests assert these counts)."""
import numpy as np

from smrt_amd._native import PackedBatch

FV = {32: 0.03, 34: 0.10, 48: 0.43, 50: 0.46, 64: 0.56}   # rows -> ice fraction (next to a layer of 0.56)
FREQUENCY, THETA = 37e9, np.deg2rad([53.0])
ST_NORM, ST_ALBEDO, ST_INPUT = 2, 3, 5


def _pack(layers, n_max_stream=32, **kw):
    """layers: per snowpack a list of (thickness, ice fraction, temperature, correlation length)."""
    S, Lmax = len(layers), max(len(x) for x in layers)
    a = np.zeros((4, S, Lmax))
    a[0], a[1], a[2], a[3] = 0.1, 0.3, 260.0, 1e-4   # (padding beyond a snowpack's layers: never read)
    for s, lay in enumerate(layers):
        a[:, s, :len(lay)] = np.array(lay).T
    return PackedBatch([len(x) for x in layers], a[0], a[1], a[2], a[3], None, [FREQUENCY], THETA, n_max_stream=n_max_stream, **kw)


def edge_batch(n_max_stream=32):
    """Five pairs: all three size classes in one pair; one layer; 34 / 50 / 64 rows; a layer that fails (a correlation length of 1 cm: the
    renormalisation or the Cholesky factorisation rejects it) between two good ones; a pair the setup rejects (dry snow above
    the freezing point).  Returns (batch, expected rows per layer or None)."""
    L = lambda rows, th=0.2, T=260.0, cl=1e-4: (th, FV[rows], T, cl)   # noqa: E731
    layers = [[L(32), L(48), L(64)],
              [L(64, th=5.0)],
              [L(34), L(50), L(64)],
              [L(48), (0.2, 0.3, 260.0, 1e-2), L(64)],
              [L(32), L(64, T=280.0)]]
    rows = [[32, 48, 64], [64], [34, 50, 64], [48, None, 64], None]
    return _pack(layers, n_max_stream), rows


def coherent_batch():
    """One pair whose middle layer (0.3 mm) is coherent at 37 GHz and is merged into the interface on top of the last one."""
    return _pack([[(0.2, FV[48], 260.0, 1e-4), (3e-4, 0.4, 260.0, 1e-4), (0.5, FV[64], 260.0, 1e-4)]], process_coherent_layers=True)


def prune_batch():
    """Two pairs of four layers under prune_deep_snowpack: the first is cut after its second layer, the second is kept whole."""
    deep = [(2.0, FV[48], 260.0, 3e-4), (20.0, FV[64], 260.0, 3e-4), (1.0, FV[50], 260.0, 1e-4), (1.0, FV[64], 260.0, 1e-4)]
    shallow = [(0.05, FV[32], 260.0, 1e-4), (0.05, FV[34], 260.0, 1e-4), (0.05, FV[48], 260.0, 1e-4), (0.05, FV[64], 260.0, 1e-4)]
    return _pack([deep, shallow], prune_deep_snowpack=True)


def same_bits(a, b):
    """Equal bit for bit (NaN payloads included)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()
