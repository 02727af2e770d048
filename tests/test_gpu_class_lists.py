"""The launches per size class of rows over the item lists built at upload (DortContext.set_class_lists) against today's
full-grid launches on the device: outputs, status words and the per-layer diagnostics are equal bit for bit, and no listed item
is found in another class (launch_info()["class_list_misses"] == 0).

The issue's case "SMRT_DORT_LANES=3 with so few pairs that a chunk is empty or holds one pair" cannot be reached through the
library: it lowers the number of concurrent passes until each has 1024 pairs, and splits a batch into equal chunks.  Three
passes with a short last chunk stand for it here; chunks of one pair and an empty chunk are in tests/test_class_lists_cpu.py."""
import numpy as np
import pytest

from class_list_cases import PAIR_LIST, class_counts, ragged_batch
from conftest import load_golden, packed_batch_from_fixture
from prep_layer_cases import FV, ST_ALBEDO, ST_INPUT, ST_NORM, _pack, edge_batch
from smrt_amd._native import DortContext

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = DortContext(0)
    yield c
    c.close()


def both(ctx, batch, pairs=None):
    res = {}
    try:
        for lists in (False, True):
            ctx.set_class_lists(lists)
            ctx.upload(batch, pairs=pairs)
            ctx.launch()
            res[lists] = ctx.download()
            info = ctx.launch_info()
            assert info["class_lists"] == lists and info["prep"] == "per_layer" and info["diagonalisation"] == "symmetric"
            assert info["class_list_misses"] == 0
            res[lists].info = info
    finally:
        ctx.set_class_lists("default")
    a, b = res[False], res[True]
    for key in ("values", "status", "layers", "streams"):
        assert np.array_equal(getattr(a, key), getattr(b, key), equal_nan=True), key
        assert getattr(a, key).tobytes() == getattr(b, key).tobytes(), key
    assert a.info["class_list_items"] is None
    return b


@pytest.mark.parametrize("n_max_stream,populated", [(32, (True, True, True)), (20, (True, True, False)), (8, (True, False, False))])
def test_lists_equal_full_grids_on_a_ragged_batch(ctx, n_max_stream, populated):
    o = both(ctx, ragged_batch(n_max_stream))
    assert (o.status == 0).all() and np.isfinite(o.values).all()
    rows = 2 * o.layers[:, :, 4].astype(int)   # (layers[..., 4]: streams of the layer, 0 beyond the snowpack)
    counts = class_counts(rows)
    assert tuple(c > 0 for c in counts) == populated, counts
    assert o.info["class_list_items"] == sum(counts) == 2 * (1 + 3 + 5)


def test_lists_equal_full_grids_on_a_pair_list(ctx):
    o = both(ctx, ragged_batch(), pairs=PAIR_LIST)
    assert (o.status == 0).all()
    assert o.values[1].tobytes() == o.values[2].tobytes()   # the repeated pair
    assert o.info["class_list_items"] == 3 + 1 + 1 + 5 + 1


def test_lists_equal_full_grids_with_a_rejected_pair_and_a_failing_layer(ctx):
    """prep_layer_cases.edge_batch: the setup stage rejects pair 4 (none of its items is listed); a layer of pair 3 fails in
    the layer kernel (listed; the eigensolver's kernels find nothing staged for it and leave -- not a miss)."""
    batch, _ = edge_batch()
    o = both(ctx, batch)
    assert o.status[4] == ST_INPUT and o.status[3] in (ST_NORM, ST_ALBEDO) and (o.status[:3] == 0).all()
    assert o.info["class_list_items"] == 3 + 1 + 3 + 3


def test_lists_over_three_concurrent_passes_with_a_short_last_chunk(ctx, monkeypatch):
    monkeypatch.setenv("SMRT_DORT_LANES", "3")
    rng = np.random.default_rng(11)
    rows = np.array([32, 34, 48, 50, 64])
    layers = [[(0.2, FV[int(r)], 260.0, 1e-4) for r in rng.choice(rows, 2)] for _ in range(3074)]
    o = both(ctx, _pack(layers, 32))
    assert o.info["chunks"] == 3 and o.info["chunk_pairs"] * 3 > 3074 and (o.status == 0).all()
    assert o.info["class_list_items"] == 2 * 3074


def test_golden_fixture_through_the_lists(ctx):
    """cfg2_iba_L20_n32_sp0 (tests/test_gpu_parity.py::test_passive_golden) at that test's tolerance."""
    d = load_golden("cfg2_iba_L20_n32_sp0")
    ctx.set_class_lists(True)
    try:
        out = ctx.run(packed_batch_from_fixture(d))
        info = ctx.launch_info()
    finally:
        ctx.set_class_lists("default")
    assert info["class_lists"] and info["class_list_misses"] == 0 and info["class_list_items"] > 0
    assert (out.status == 0).all(), out.status
    assert np.abs(out.values - d["result"]).max() < 1e-6   # K: TB_TOL of tests/test_gpu_parity.py
