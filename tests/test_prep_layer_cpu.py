"""The per-layer prep (pair setup + one workgroup per item and size class, dort_prep_layer.hpp) against the per-pair prep
kernel under the CPU emulator: the staging area each leaves -- L+, B, d, the block inverses, n -- and the outputs of the
pipeline behind it are equal bit for bit, status words and the rows of failed pairs included."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from prep_layer_cases import ST_ALBEDO, ST_INPUT, ST_NORM, coherent_batch, edge_batch, prune_batch, same_bits
from smrt_amd._native import SmrtBatch

EMU_DIR = os.path.join(ROOT, "tests", "hostemu")
LIB = os.path.join(EMU_DIR, "libprep_layer_host.so")


@pytest.fixture(scope="module")
def emu():
    csrc = os.path.join(ROOT, "smrt_amd", "csrc")
    srcs = [os.path.join(EMU_DIR, f) for f in ("prep_layer_host.cpp", "emu_lib.cpp", "emu_runtime.hpp")] + sorted(
        os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith(".hpp"))
    if not os.path.exists(LIB) or any(os.path.getmtime(s) > os.path.getmtime(LIB) for s in srcs):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-I", EMU_DIR, "-o", LIB, srcs[0]])
    lib = C.CDLL(LIB)
    P = C.POINTER
    lib.smrt_emu_prep_run.argtypes = [P(SmrtBatch), C.c_int, C.c_int] + [P(C.c_double), P(C.c_int32)] + [P(C.c_double)] * 4 + [P(C.c_int)]
    return lib


def run(lib, batch, per_layer, order=0):
    s = batch.struct
    n, Lmax, N = batch.n_pairs, int(s.n_layers_max), 2 * int(s.n_max_stream)
    LD = (N + 1) | 1
    r = dict(out=np.empty((n,) + batch.out_shape()), status=np.full(n, -9, np.int32), L=np.zeros((n, Lmax, N * LD)),
             B=np.zeros((n, Lmax, N * LD)), d=np.zeros((n, Lmax, N)), inv=np.zeros((n, Lmax, 1024)), n=np.zeros((n, Lmax), np.int32))
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))  # noqa: E731
    rc = lib.smrt_emu_prep_run(C.byref(s), per_layer, order, dp(r["out"]), r["status"].ctypes.data_as(C.POINTER(C.c_int32)),
                               dp(r["L"]), dp(r["B"]), dp(r["d"]), dp(r["inv"]), r["n"].ctypes.data_as(C.POINTER(C.c_int)))
    assert rc == 0
    return r


def both(lib, batch, order=0):
    a, b = run(lib, batch, 0, order), run(lib, batch, 1, order)
    for key in a:
        assert same_bits(a[key], b[key]), key
    return b


def test_per_layer_prep_equals_per_pair_prep_at_the_class_edges(emu):
    batch, rows = edge_batch()
    r = both(emu, batch)
    for p, want in enumerate(rows):
        if want is None:   # rejected by the setup kernel: status and NaN rows as fail_pair leaves them
            assert r["status"][p] == ST_INPUT and np.isnan(r["out"][p]).all()
            continue
        for l, n in enumerate(want):
            if n is None:   # the layer that fails between good ones
                assert -r["n"][p, l] in (ST_NORM, ST_ALBEDO)
                assert r["status"][p] == -r["n"][p, l] and np.isnan(r["out"][p]).all()
            else:
                assert r["n"][p, l] == n, (p, l, r["n"][p])
        if None not in want:
            assert r["status"][p] == 0 and np.isfinite(r["out"][p]).all()


def test_per_layer_prep_equals_per_pair_prep_with_a_coherent_layer(emu):
    r = both(emu, coherent_batch(), order=1)
    assert r["status"][0] == 0 and list(r["n"][0]) == [48, 64, 0]   # the thin layer is gone: two items staged


def test_per_layer_prep_equals_per_pair_prep_under_prune_deep_snowpack(emu):
    r = both(emu, prune_batch())
    assert (r["status"] == 0).all()
    assert list(r["n"][0]) == [48, 64, 0, 0] and list(r["n"][1]) == [32, 34, 48, 64]   # below the cut nothing is staged
