"""rtsolver/solver_base.py without a GPU and without the library: the group loop, the plan bookkeeping and the refusing packer,
on a minimal solver and a context that records what it is handed and answers zeros (as tests/test_host_logic.py does for DORT)."""
import re
import threading

import numpy as np
import pytest

from smrt_amd import make_model, sensor_list
from smrt_amd._native import STATUS_MESSAGES, BatchOutput
from smrt_amd.core.error import SMRTError
from smrt_amd.core.model import SimulationPlan
from smrt_amd.core.snowpack import Snowpack, substrate_kind
from smrt_amd.inputs.make_medium import make_snowpack, make_soil
from smrt_amd.rtsolver import dort
from smrt_amd.rtsolver.solver_base import RefusingPacker, SolverBase
from smrt_amd.substrate.transparent import Transparent


class RecordingContext:
    """Stands where rtsolver/dort.py:get_context returns the GPU context: every row of the output holds 100 x the number of the
    call + the pair it stands for; `bad` = {call: status word of its first row}."""

    def __init__(self, bad=None):
        self.lock, self.pairs, self.bad = threading.RLock(), [], bad or {}

    def run(self, batch, pairs=None):
        call = len(self.pairs)
        self.pairs.append(None if pairs is None else list(pairs))
        rows = np.arange(batch.n_pairs) if pairs is None else np.asarray(pairs)
        out = BatchOutput(batch, len(rows))
        for a in (out.values, out.status, out.layers, out.streams):
            a[...] = 0
        out.streams[:, :3] = 2.0, 0.9, 0.5
        out.values[...] = (100 * call + rows).reshape((-1,) + (1,) * (out.values.ndim - 1))
        out.status[0] = self.bad.get(call, 0)
        return out


class Packer(RefusingPacker):
    SUBSTRATES_ON_HOST, INTERFACES_ON_HOST, IBA_SCALARS_ON_HOST, EVALUATE_ON_HOST = "no substrate", "no interface", "no scalars", "no emmodel"


class Solver(SolverBase):
    """A transparent substrate is replaced by none before packing; the launch raises on demand."""

    NAME = "minimal"
    devices = None
    process_coherent_layers = False   # (read by DORT's result code)

    def __init__(self, error_handling="exception", fail_in_launch=False):
        self.error_handling, self.fail_in_launch = error_handling, fail_in_launch
        self.packer = Packer(n_max_stream=4, error_handling=error_handling)
        self.facts_seen = []

    def _check_sensor(self, sensor):
        pass

    def _sensor_key(self, sensor):
        return tuple(np.round(sensor.theta_deg, 12))

    def _packer(self):
        return self.packer

    def _snowpack_key(self, sp, on_host):
        if isinstance(sp.substrate, Transparent):
            sp = Snowpack(layers=sp.layers, interfaces=sp.interfaces, substrate=None)
        return sp, substrate_kind(sp.substrate)

    def _prepare_group(self, ctx, g):
        facts = g.packer._plan_facts
        if facts is not None:
            self.facts_seen += [(sp is given, facts.get(id(sp)), facts.get(id(given))) for sp, given in zip(g.sps, g.given)]
        SolverBase._prepare_group(self, ctx, g)

    def _launch(self, ctx, g):
        if self.fail_in_launch:
            raise RuntimeError("inside the loop")
        return ctx.run(g.batch, pairs=g.pairs)


@pytest.fixture()
def ctx(monkeypatch):
    context = RecordingContext()
    monkeypatch.setattr(dort, "get_context", lambda device=None: context)
    return context


def snowpacks():
    kw = dict(density=[300.0, 350.0], temperature=[260.0, 265.0], corr_length=[2e-4, 3e-4])
    soil = make_soil("flat", complex(5.0, 0.5), 270.0)
    return [make_snowpack([0.3, 1.0], "exponential", **kw), make_snowpack([0.2, 2.0], "exponential", substrate=soil, **kw),
            make_snowpack([0.5, 0.7], "exponential", **kw)]


def test_groups_pairs_and_the_order_of_the_results(ctx):
    """Two sensor keys x (no substrate, Flat substrate) = four groups, in the order of first appearance of their keys."""
    p0, p1, p2 = snowpacks()
    a, b = sensor_list.passive(19e9, 40), sensor_list.passive(37e9, 40)
    c, c2 = sensor_list.passive(19e9, 55), sensor_list.passive(37e9, 55)
    sims = [(c, p0), (a, p0), (a, p1), (a, p2), (c2, p2), (b, p0), (c, p1), (b, p2)]
    solver = Solver()
    results = solver.solve_batch(sims, "iba")
    # (55, none): frequencies x snowpacks = 2 x 2 of which two are asked for; the three other groups are whole batches
    assert ctx.pairs == [[0, 3], None, None, None] and solver.launches == 4 and solver.launch_info == []
    expected = [0, 200, 300, 201, 3, 202, 100, 203]   # 100 x the call + frequency index x number of snowpacks + snowpack index
    assert len(results) == len(sims)
    for res, value, (sensor, _) in zip(results, expected, sims):
        assert np.all(res.data.values == value) and list(res.data.coords["theta"]) == list(sensor.theta_deg)


def test_an_empty_batch_is_an_empty_list(ctx):
    assert Solver().solve_batch([], "iba") == [] and ctx.pairs == []


def test_a_bad_status_in_the_second_group_raises_its_message_or_returns(ctx):
    p0, p1, _ = snowpacks()
    sensor = sensor_list.passive(37e9, 55)
    status = sorted(STATUS_MESSAGES)[0]
    ctx.bad = {1: status}
    with pytest.raises(SMRTError, match=re.escape(STATUS_MESSAGES[status])):
        Solver().solve_batch([(sensor, p0), (sensor, p1)], "iba")
    assert len(ctx.pairs) == 2
    ctx.bad = {3: status}
    assert len(Solver(error_handling="nan").solve_batch([(sensor, p0), (sensor, p1)], "iba")) == 2
    ctx.bad = {5: 12345}   # (a word the library has no text for)
    with pytest.raises(SMRTError, match="the minimal solver failed with status 12345"):
        Solver().solve_batch([(sensor, p0), (sensor, p1)], "iba")


def plan_of(sensor, sps):
    return SimulationPlan([sensor], sps, np.zeros(len(sps), int), np.arange(len(sps)), dimensions=[("snowpack", list(range(len(sps))))])


def test_the_plan_facts_are_cleared_when_the_loop_raises(ctx):
    solver = Solver(fail_in_launch=True)
    with pytest.raises(RuntimeError, match="inside the loop"):
        solver.solve_plan(make_model("iba", "dort"), plan_of(sensor_list.passive(37e9, 55), snowpacks()))
    assert solver.facts_seen and solver.packer._plan_facts is None and solver.packer._plan_model is None


def test_a_replaced_snowpack_has_the_facts_of_the_one_it_stands_for(ctx):
    p0, _, p2 = snowpacks()
    p2.substrate = Transparent()
    solver = Solver()
    res = solver.solve_plan(make_model("iba", "dort"), plan_of(sensor_list.passive(37e9, 55), [p0, p2]))
    assert res.data.dims[0] == "snowpack" and solver.launches == 1      # (the transparent substrate is none: one group)
    (same0, packed0, given0), (same2, packed2, given2) = solver.facts_seen
    assert same0 and not same2
    assert packed0 is given0 is not None and packed2 is given2 is not None and packed2 is not packed0
    assert solver.packer._plan_facts is None


def test_the_refusing_packer_raises_each_of_its_messages():
    packer = Packer()
    for method, message in ((packer._substrates_on_host, "no substrate"), (packer._interfaces_on_host, "no interface"),
                            (packer._iba_scalars_on_host, "no scalars"), (packer._evaluate_on_host, "no emmodel")):
        with pytest.raises(SMRTError, match="^" + message + "$"):
            method(None, [], [], key=None)
