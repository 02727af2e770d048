"""Batches for the item lists of the launches per size class of rows (smrt_amd/csrc/dort_class_lists.hpp):
tests/test_class_lists_cpu.py (emulator) and tests/test_gpu_class_lists.py (device) use the same ones.

Row counts as in prep_layer_cases: at 37 GHz and 260 K next to a layer of ice fraction 0.56, with 32 streams per hemisphere, the
fractions of FV give 32, 34, 48, 50 and 64 rows; the second frequency (19 GHz) sees nearly the same permittivities.  With 20
streams the rows stay within (0, 40] -- the class (48, 64] is empty --, with 8 within (0, 16]."""
import numpy as np

from prep_layer_cases import FV, THETA
from smrt_amd._native import PackedBatch

FREQUENCIES = [37e9, 19e9]
CLASSES = ((0, 32), (32, 48), (48, 64))


def ragged_batch(n_max_stream=32):
    """Three snowpacks x two frequencies with 1, 3 and 5 layers: items beyond a snowpack exist, and with 32 streams every class
    holds items of several pairs."""
    L = lambda rows: (0.2, FV[rows], 260.0, 1e-4)   # noqa: E731
    layers = [[L(64)], [L(32), L(48), L(64)], [L(34), L(50), L(64), L(32), L(48)]]
    S, Lmax = len(layers), 5
    a = np.zeros((4, S, Lmax))
    a[0], a[1], a[2], a[3] = 0.1, 0.3, 260.0, 1e-4   # (padding beyond a snowpack's layers: never read)
    for s, lay in enumerate(layers):
        a[:, s, :len(lay)] = np.array(lay).T
    return PackedBatch([len(x) for x in layers], a[0], a[1], a[2], a[3], None, FREQUENCIES, THETA, n_max_stream=n_max_stream)


PAIR_LIST = [4, 0, 0, 5, 3]   # of the six pairs of ragged_batch: pair 0 twice, pairs 1 and 2 skipped


def class_counts(rows):
    """Items per class of an array of row counts (0: no item)."""
    rows = np.asarray(rows)
    return [int(((rows > lo) & (rows <= hi)).sum()) for lo, hi in CLASSES]
