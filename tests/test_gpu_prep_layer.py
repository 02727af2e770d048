"""The per-layer prep against the per-pair prep kernel on the device, through DortContext.set_prep: outputs, status words and
the per-layer diagnostics are equal bit for bit -- at the class edges (32 / 34 / 48 / 50 / 64 rows), with 12 and 24 streams,
with a coherent layer, under prune_deep_snowpack, and over concurrent pipeline passes with a short last chunk."""
import numpy as np
import pytest

from prep_layer_cases import (FREQUENCY, FV, ST_ALBEDO, ST_INPUT, ST_NORM, THETA, _pack, coherent_batch, edge_batch, prune_batch,
                              same_bits)
from smrt_amd._native import DortContext

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = DortContext(0)
    yield c
    c.close()


def both(ctx, batch):
    res = {}
    try:
        for prep in ("per_pair", "per_layer"):
            ctx.set_prep(prep)
            ctx.upload(batch)
            assert ctx.launch_info()["prep"] == prep
            ctx.launch()
            res[prep] = ctx.download()
            res["info"] = ctx.launch_info()   # (set_prep below drops the upload)
    finally:
        ctx.set_prep("default")
    a, b = res["per_pair"], res["per_layer"]
    for key in ("values", "status", "layers", "streams"):
        assert same_bits(getattr(a, key), getattr(b, key)), key
    b.info = res["info"]
    return b


@pytest.mark.parametrize("n_max_stream", [32, 24, 12])
def test_per_layer_prep_equals_per_pair_prep_at_the_class_edges(ctx, n_max_stream):
    batch, rows = edge_batch(n_max_stream)
    o = both(ctx, batch)
    assert o.status[4] == ST_INPUT and np.isnan(o.values[4]).all()
    assert o.status[3] in (ST_NORM, ST_ALBEDO) and np.isnan(o.values[3]).all()
    assert (o.status[:3] == 0).all() and np.isfinite(o.values[:3]).all()
    if n_max_stream == 32:   # the stream counts the batch was built for (layers[..., 4]: streams of the layer)
        for p in (0, 1, 2):
            assert [2 * int(x) for x in o.layers[p, :len(rows[p]), 4]] == rows[p]
    else:   # 24 streams: rows in all three classes again; 12 streams: the (0, 32] class alone, and row counts that are no multiple of 16
        counts = 2 * o.layers[:3, :, 4].astype(int)
        assert counts.max() == 2 * n_max_stream and (counts[counts > 0] % 16 != 0).any()


def test_per_layer_prep_equals_per_pair_prep_with_a_coherent_layer(ctx):
    o = both(ctx, coherent_batch())
    assert o.status[0] == 0


def test_per_layer_prep_equals_per_pair_prep_under_prune_deep_snowpack(ctx):
    o = both(ctx, prune_batch())
    assert (o.status == 0).all() and o.info["prune_rounds"] == 4


def test_per_layer_prep_over_three_concurrent_passes_with_a_short_last_chunk(ctx):
    """3074 pairs: three passes of 1025 pairs would cover 3075 -- the last chunk is one pair short, and each pass works in its
    own region of the staging area (records included)."""
    rng = np.random.default_rng(7)
    rows = np.array([32, 34, 48, 50, 64])
    layers = [[(0.2, FV[int(r)], 260.0, 1e-4) for r in rng.choice(rows, 2)] for _ in range(3074)]
    batch = _pack(layers, 32)
    o = both(ctx, batch)
    info = o.info
    assert info["chunks"] == 3 and info["chunk_pairs"] * 3 > 3074 and (o.status == 0).all()
