"""The iterative second-order solver on the GPU at the shapes where its own choices can go wrong (the edge FIXTURES --
more than 64 streams, every mode count of the four register tables -- run with every other fixture in
tests/test_gpu_second_order.py; the conditions that make them able to fail: test_second_order_cpu.py:
test_edge_fixtures_are_sensitive):

* two frequencies x 45 snowpacks x 3 angles through the solver's own packing: the substrate's rows by GLOBAL pair, the
  layer count by `pair % S`, a second block of the walk -- whole, in chunks, as listed pairs, and both;
* 130 streams per layer: three trips of a lane over the streams, unequal sets on both sides of 64;
* a layer left with one stream: reported by status, NaN in the order-2 rows of that pair and of no other;
* one angle and five: the common angle bit for bit.

The batches, their restatement (computed once per run of the suite) and the CPU twins of these tests on the host build are
in tests/test_second_order_cpu.py.  Tolerance: SIGMA_RTOL = 1e-8 of the pair's largest co-polarised total."""
import numpy as np
import pytest

import test_second_order_cpu as T
from smrt_amd import make_model, sensor_list
from smrt_amd.core.error import SMRTError

pytestmark = pytest.mark.gpu
LISTED = [89, 3, 3, 46, 44, 45]   # a pair twice, both sides of the frequency boundary (pairs 44 | 45), a Transparent one (44)


@pytest.fixture(scope="module")
def ctx():
    from smrt_amd.rtsolver.dort import get_context

    return get_context(None)


@pytest.fixture(scope="module")
def whole(ctx):
    """The two-frequency batch in one piece, interlayer term off and on."""
    return {interlayer: T.edge_group("frequencies").run(ctx, interlayer) for interlayer in (False, True)}


@pytest.mark.parametrize("interlayer", [False, True], ids=["plain", "interlayer"])
def test_two_frequencies_and_rough_substrates_match_the_restatement(whole, interlayer):
    out = whole[interlayer]
    assert out.values.shape == (90, 7, 3, 2, 2)
    T.assert_batch_matches(out, T.edge_batch("frequencies"), T.edge_reference("frequencies"), interlayer, "GPU, two frequencies")


def workspace_budget(batch, rows, rows_per_chunk, interlayer):
    """Bytes that leave room for exactly `rows_per_chunk` rows of the chunk buffers next to the buffers of a run of `rows`
    pairs: the formulas of smrt_second_order_upload_pairs (second_order.hip), for a batch with substrate modes."""
    b = batch.struct
    L, nt, nmax, m_max = int(b.n_layers_max), int(b.n_theta), int(b.n_max_stream), int(b.m_max)
    substrate = batch.n_pairs * L * nt * nmax * m_max * 12 * 8
    fixed = nmax * 8 + substrate + rows * L * nt * 5 * 8 + rows * 28 * nt * 8 + rows * (L + 1) * nt * 4 * 8
    slots = 2 + (L if interlayer else 0)
    per_row = L * 4 + L * 2 * nmax * 8 + L * nt * slots * 4 * 8
    return fixed + rows_per_chunk * per_row


def same_bits(a, b, rows=None):
    rows = slice(None) if rows is None else rows
    return (np.array_equal(a.values, b.values[rows], equal_nan=True) and np.array_equal(a.layer_backscatter, b.layer_backscatter[rows], equal_nan=True)
            and np.array_equal(a.status, b.status[rows]))


@pytest.mark.parametrize("interlayer", [False, True], ids=["plain", "interlayer"])
def test_chunks_and_listed_pairs_give_the_bits_of_the_whole_batch(whole, ctx, interlayer):
    """The rows of a chunk and the rows of a listed run are not the global pairs: the substrate's modes, the layer counts
    and the frequencies are found by global pair all the same.  (test_rough_pairs_of_the_frequency_batch_are_told_apart: no
    two rough pairs of this batch could be taken for one another.)"""
    group, one = T.edge_group("frequencies"), whole[interlayer]
    assert not np.isnan(one.values).any()
    chunked = group.run(ctx, interlayer, workspace_budget(group.batch, 90, 20, interlayer))   # 5 chunks
    assert same_bits(chunked, one)
    listed = group.run(ctx, interlayer, pairs=LISTED)
    assert listed.values.shape[0] == len(LISTED) and same_bits(listed, one, LISTED)
    for rows_per_chunk in (1, 4):   # 6 chunks of one row; a chunk of 4 rows and one of 2
        both = group.run(ctx, interlayer, workspace_budget(group.batch, len(LISTED), rows_per_chunk, interlayer), pairs=LISTED)
        assert same_bits(both, one, LISTED), rows_per_chunk


def test_many_streams_in_a_batch_match_the_restatement(ctx):
    T.assert_stream_counts_straddle(T.edge_reference("streams"))
    out = T.edge_group("streams").run(ctx, True)
    T.assert_batch_matches(out, T.edge_batch("streams"), T.edge_reference("streams"), True, "GPU, 130 streams")


def test_a_layer_with_one_stream_is_reported_by_status(ctx):
    """Through the C ABI, so that nothing on the host looks at the streams first."""
    batch, extras = T.pack_c_abi(T.edge_batch("two_streams"), True)
    out = ctx.second_order_run(batch, extras)
    first = ctx.first_order_run(batch)
    T.assert_one_stream_is_reported(out, first.values, first.layer_backscatter)
    good = ctx.second_order_run(batch, extras, pairs=[0, 2])
    assert not good.status.any()
    assert np.array_equal(good.values, out.values[[0, 2]]) and np.array_equal(good.layer_backscatter, out.layer_backscatter[[0, 2]])


def test_model_run_with_a_layer_of_one_stream():
    """What Model.run makes of the status (iterative_first_order: _solve_indexed and _Solution): error_handling="exception"
    raises the message of the status; "nan" hands the device's rows on as they are -- NaN in the three order-2
    contributions and hence in the total of that snowpack, its first-order contributions those of iterative_first_order."""
    from smrt_amd import _native

    sps = [T.build_snowpack(c, T.api()) for c in T.edge_batch("two_streams")]
    sensor = sensor_list.active(13e9, [25.0, 40.0])
    options = dict(n_max_stream=2, m_max=3, compute_scattering_interlayer=True, return_contributions=True)
    with pytest.raises(SMRTError) as error:
        make_model("iba", "iterative_second_order", rtsolver_options=options).run(sensor, sps)
    assert str(error.value) == _native.STATUS_MESSAGES[T.ST_INPUT]
    with pytest.raises(SMRTError, match="fewer than two streams"):
        make_model("iba", "iterative_second_order", rtsolver_options=options).run(sensor, sps[1])
    res = make_model("iba", "iterative_second_order", rtsolver_options=dict(error_handling="nan", **options)).run(sensor, sps)
    data = np.asarray(res.data.values, float)
    assert list(res.data.dims)[1:] == ["contribution", "theta_inc", "polarization_inc", "polarization"] and data.shape == (3, 8, 2, 2, 2)
    assert np.isfinite(data[[0, 2]]).all() and data[[0, 2], 5].all()
    assert np.isnan(data[1, 0]).all() and np.isnan(data[1, 5:]).all() and np.isfinite(data[1, 1:5]).all()
    first = make_model("iba", "iterative_first_order", rtsolver_options=dict(return_contributions=True)).run(sensor, sps)
    assert np.array_equal(np.asarray(first.data.values, float)[:, 1:5], data[:, 1:5])


def test_the_common_angle_does_not_depend_on_the_angle_count(ctx):
    T.assert_common_angle_is_the_same(lambda case: T.run_case(case, ctx))
