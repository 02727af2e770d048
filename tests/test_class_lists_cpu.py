"""The item lists of the launches per size class of rows (dort_class_lists.hpp) under the CPU emulator, built as the upload
builds them (count in the cost kernel's body, offsets on the host, fill per dispatch position) and walked as the kernels walk
them: every list equals today's block order filtered by the rows the setup stage records (order included), the segments of the
chunks are contiguous and disjoint, and their union is exactly the items with rows > 0."""
import ctypes as C

import numpy as np
import pytest

from class_list_cases import CLASSES, PAIR_LIST, class_counts, ragged_batch
from host_build import host_library
from prep_layer_cases import coherent_batch, edge_batch
from smrt_amd._native import SmrtBatch


@pytest.fixture(scope="module")
def emu():
    lib = host_library("libclass_lists_host.so", "class_lists_host.cpp")
    P = C.POINTER
    lib.smrt_emu_class_lists.restype = C.c_longlong
    lib.smrt_emu_class_lists.argtypes = [P(SmrtBatch), P(C.c_longlong), C.c_longlong, C.c_longlong, P(C.c_int), C.c_int, P(C.c_int),
                                         P(C.c_longlong), P(C.c_longlong), P(C.c_int), P(C.c_longlong), P(C.c_int), P(C.c_longlong)]
    return lib


def build(lib, batch, chunk_pairs, pairs=None, dispatch=None, order=0):
    """Runs the driver and checks the list properties; returns (rows the setup stage recorded [pairs][Lmax], per chunk and class
    the listed items)."""
    n = batch.n_pairs if pairs is None else len(pairs)
    Lmax = int(batch.struct.n_layers_max)
    chunks = -(-n // chunk_pairs)
    pm = None if pairs is None else np.ascontiguousarray(pairs, dtype=np.int64)
    dp = None if dispatch is None else np.ascontiguousarray(dispatch, dtype=np.int32)
    rows = np.full((n, Lmax), -5, np.int32)
    seg_off, seg_cnt, full_cnt = (np.full((chunks, 3), -1, np.int64) for _ in range(3))
    listed = np.full(n * Lmax, -1, np.int32)
    full = np.full((chunks, 3, chunk_pairs * Lmax), -1, np.int32)
    misses = C.c_longlong(-1)
    ip = lambda a, t: None if a is None else a.ctypes.data_as(C.POINTER(t))  # noqa: E731
    total = lib.smrt_emu_class_lists(C.byref(batch.struct), ip(pm, C.c_longlong), n, chunk_pairs, ip(dp, C.c_int), order, ip(rows, C.c_int),
                                     ip(seg_off, C.c_longlong), ip(seg_cnt, C.c_longlong), ip(listed, C.c_int), ip(full_cnt, C.c_longlong),
                                     ip(full, C.c_int), C.byref(misses))
    assert total >= 0 and misses.value == 0
    # contiguous and disjoint: ordered by (chunk, class), each segment starting where the one before ends
    assert list(seg_off.ravel()) == list(np.concatenate([[0], np.cumsum(seg_cnt.ravel())[:-1]])) and seg_cnt.sum() == total
    out = []
    for c in range(chunks):
        cn = min(chunk_pairs, n - c * chunk_pairs)
        seen = []
        for k in range(3):
            got = listed[seg_off[c, k]:seg_off[c, k] + seg_cnt[c, k]]
            # today's block order, filtered by the rows the setup stage recorded
            assert list(got) == list(full[c, k, :full_cnt[c, k]]), (c, k)
            lo, hi = CLASSES[k]
            r = rows[c * chunk_pairs:c * chunk_pairs + cn].ravel()[got]
            assert ((r > lo) & (r <= hi)).all()
            seen += list(got)
        # the union over the classes: exactly the chunk's items with rows > 0, each once
        want = np.flatnonzero(rows[c * chunk_pairs:c * chunk_pairs + cn].ravel() > 0)
        assert sorted(seen) == list(want) and len(set(seen)) == len(seen)
        out.append(seen)
    return rows, out


@pytest.mark.parametrize("n_max_stream,populated", [(32, (True, True, True)), (20, (True, True, False)), (8, (True, False, False))])
def test_lists_of_a_ragged_batch(emu, n_max_stream, populated):
    batch = ragged_batch(n_max_stream)
    rows, _ = build(emu, batch, chunk_pairs=6)
    assert tuple(c > 0 for c in class_counts(rows)) == populated, class_counts(rows)
    assert (rows > 0).sum() == 2 * (1 + 3 + 5)
    if n_max_stream == 32:
        assert list(rows[2]) == [34, 50, 64, 32, 48] and list(rows[0]) == [64, 0, 0, 0, 0]


def test_lists_follow_the_dispatch_order_in_every_chunk(emu):
    """Chunks of four pairs (the last holds two), each with its own permutation of its pair slots."""
    batch = ragged_batch()
    dispatch = [2, 0, 3, 1, 1, 0]
    rows, listed = build(emu, batch, chunk_pairs=4, dispatch=dispatch, order=1)
    Lmax = 5
    for c, seen in enumerate(listed):
        # within a class the pairs appear in dispatch order, the layers of a pair ascending
        slots = dispatch[4 * c:4 * c + 4]
        for k, (lo, hi) in enumerate(CLASSES):
            want = [s * Lmax + l for s in slots for l in range(Lmax) if lo < rows[4 * c + s, l] <= hi]
            got = [i for i in seen if lo < rows[4 * c:].ravel()[i] <= hi]
            assert got == want, (c, k)


def test_lists_of_a_pair_list_with_a_repeated_and_a_skipped_pair(emu):
    batch = ragged_batch()
    rows, _ = build(emu, batch, chunk_pairs=5, pairs=PAIR_LIST)
    assert list(rows[1]) == list(rows[2]) == [64, 0, 0, 0, 0]   # pair 0 (snowpack 0) twice
    assert (rows[3] > 0).sum() == 5 and (rows[0] > 0).sum() == 3


def test_lists_with_one_pair_per_chunk_and_an_empty_chunk(emu):
    """Chunks of one pair; the chunk of the pair the setup stage rejects has three empty segments."""
    batch, _ = edge_batch()
    rows, listed = build(emu, batch, chunk_pairs=1)
    assert listed[4] == [] and (rows[4] == 0).all()          # dry snow above the freezing point: ST_INPUT, nothing listed
    assert sorted(listed[3]) == [0, 1, 2]                    # the layer that fails later in the layer kernel IS listed
    assert [len(x) for x in listed] == [3, 1, 3, 3, 0]


def test_lists_with_a_coherent_layer(emu):
    """process_coherent_layers: the lists hold the pair's own layer indices after the thin layer is merged away."""
    rows, listed = build(emu, coherent_batch(), chunk_pairs=1)
    assert list(rows[0]) == [48, 64, 0] and sorted(listed[0]) == [0, 1]
