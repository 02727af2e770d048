"""Iterative first-order backscatter solver, MI355X-native (drop-in for smrt/rtsolver/iterative_first_order.py).

The zeroth and first order of the iterative solution of the radiative transfer equation (Ulaby et al. 2014, eqs. 11.62,
11.74, 11.75; refraction factor of Tsang et al. 2007, eqs. 22a/b): for radar simulations of weakly scattering snow it is
far cheaper than DORT -- closed form per (snowpack, frequency, incidence angle): no eigenproblem, no linear system -- and
it splits the backscatter by mechanism and by layer:

* ``order0_backscatter``: surface, interfaces and substrate, attenuated by the snow above them;
* ``order1_direct_backscatter``: one volume backscatter, upwards;
* ``order1_double_bounce``: one volume scattering and one specular reflection at the boundary below the layer;
* ``order1_reflected_backscatter``: one volume backscatter between two specular reflections.

    m = make_model("iba", "iterative_first_order", rtsolver_options={"return_contributions": True})
    res = m.run(sensor_list.active(17.25e9, [20, 30, 45]), snowpacks)
    res.sigmaVV_dB(contribution="order1_double_bounce")

Limits: backscatter only (active sensors, theta == theta_inc), V and H only, no atmosphere, no multiple scattering --
reliable for single scattering albedos below about 0.5 (compare with DORT to estimate what is missing).

The arithmetic runs in two HIP kernels through the C ABI (include/smrt_dort.h: smrt_first_order_*): the layer
electromagnetics once per (pair, layer), the recursion per (pair, incidence angle).  Flat interfaces, Flat / Reflector / no
substrate and the phase functions of the IBA and Rayleigh families are evaluated on the device; any other interface or
substrate object and any other emmodel are evaluated here through the reference's protocols and handed over as numbers.
Packing of layers, kinds and host scalars is DORT's (rtsolver/dort.py).

Deliberate difference from the reference: its two warnings -- single scattering albedo above 0.5, optically shallow
snowpack (tau < 5) without substrate -- are emitted ONCE PER RUN with the number of simulations concerned and the worst
value, not once per layer and simulation.
"""
import numpy as np

from .._native import PackedFirstOrderExtras
from ..core.error import SMRTError, smrt_warn
from ..core.foreign import result_factory
from ..core.result import LabeledArray, make_result
from ..core.snowpack import substrate_kind
from ..interface.flat import Flat
from .dort import DORT, get_context
from .solver_base import LayeredSolution, SolverBase, check_error_handling

CONTRIBUTIONS = ["total", "order0_backscatter", "order1_direct_backscatter", "order1_double_bounce",
                 "order1_reflected_backscatter"]
POLA = ["V", "H"]


class IterativeFirstOrder(SolverBase):
    """error_handling: "exception" (default) raises on an invalid simulation, "nan" returns NaN for it and goes on.
    return_contributions: False (default) returns the total backscatter, True adds a leading `contribution` dimension
    ("total" first, then the four mechanisms).  `devices` (list of GPU indices; the first is used) is smrt_amd's own knob."""

    _broadcast_capability = {"theta_inc", "polarization_inc", "theta", "polarization"}
    NAME = "iterative_first_order"   # in the messages; a solver built on this one (iterative_second_order) sets its own

    def __init__(self, error_handling="exception", return_contributions=False, devices=None):
        self.error_handling = check_error_handling(error_handling)
        self.return_contributions = bool(return_contributions)
        self.devices = devices

    # ---- grouping, packing, launching ----------------------------------------------------------------------------
    @classmethod
    def _check_sensor(cls, sensor):
        if sensor.mode != "A":
            raise SMRTError(f"the {cls.NAME} solver is only suitable for active microwave. Use an adequate sensor "
                            "falling in this category.")
        if np.ndim(sensor.frequency) != 0:
            raise SMRTError(f"the {cls.NAME} solver does not broadcast the frequency: split the sensor first "
                            "(Model.run does)")
        if not np.array_equal(sensor.theta_deg, sensor.theta_inc_deg):
            raise SMRTError(f"the {cls.NAME} solver computes the backscatter (theta == theta_inc)")

    @staticmethod
    def _sensor_key(sensor):
        return tuple(np.round(sensor.theta_inc_deg, 12))

    def _packer(self):
        return _Packer(n_max_stream=2, m_max=0, error_handling=self.error_handling, devices=self.devices)

    def _snowpack_key(self, sp, on_host):
        self._refuse_atmosphere(sp)
        return sp, (substrate_kind(sp.substrate, "A"), on_host)

    def _solve_indexed(self, sensors, packs, sens_idx, pack_idx, emmodel_names, packer=None):
        sol = SolverBase._solve_indexed(self, sensors, packs, sens_idx, pack_idx, emmodel_names, packer)
        sol.warn()
        return sol

    def _prepare_group(self, ctx, g):
        g.packer.host_emmodels = None
        SolverBase._prepare_group(self, ctx, g)
        g.extras = self._extras(ctx.first_order_layers, g.batch, g.packer, g.sensor0, g.sps, g.u_freq)

    def _context(self):
        return get_context((self.devices or [None])[0])   # (this module's name: the CPU tests put a stand-in here)

    def _launch(self, ctx, g):
        return self._run_group(ctx, g.batch, g.extras, g.pairs, g.packer, g.sensor0, g.sps, g.u_freq)

    # the two places a solver built on this one (iterative_second_order) differs in: the device call and the result axis
    def _run_group(self, ctx, batch, extras, pairs, packer, sensor0, sps, freqs):
        return ctx.first_order_run(batch, extras, pairs=pairs)

    def _solution(self, sensors, packs, sens_idx, pack_idx):
        return _Solution(self, sensors, packs, sens_idx, pack_idx)

    # ---- what the host evaluates (include/smrt_dort.h: smrt_first_order_extras) ------------------------------------
    @classmethod
    def _rows(cls, value, n):
        """[2, n] from a diagonal reflection / transmission 'matrix' of the interface protocol (0 -> zeros)."""
        a = np.asarray(getattr(value, "values", value), float)
        if a.ndim == 0:
            return np.full((2, n), float(a))
        if a.ndim == 2 and a.shape[0] >= 2 and a.shape[1] == n:
            return a[:2]
        raise SMRTError(f"the {cls.NAME} solver needs diagonal specular / coherent matrices [npol, n_mu], got {a.shape}")

    @staticmethod
    def _dense(value, n):
        """[n, 2, 2] from a diffuse reflection matrix at one azimuth: dense [p, p, dphi, mu_s, mu_i] (its diagonal in the
        cosines), diagonal [p, mu], or 0."""
        a = np.asarray(getattr(value, "values", value), float)
        out = np.zeros((n, 2, 2))
        if a.ndim == 0:
            if float(a) != 0.0:
                raise SMRTError("a scalar diffuse reflection must be zero")
        elif a.ndim == 5:
            out[:] = np.transpose(np.diagonal(a[:2, :2, 0], axis1=-2, axis2=-1), (2, 0, 1))
        elif a.ndim == 2:
            out[:, 0, 0], out[:, 1, 1] = a[0], a[1]
        else:
            raise SMRTError(f"unsupported layout of a diffuse reflection matrix: {a.shape}")
        return out

    @classmethod
    def boundary_values(cls, obj, frequency, eps_above, eps_below, mu_above, mu_below, substrate=False):
        """[n_theta, 10] of one interface (between eps_above and eps_below) or substrate (under eps_above) object: specular
        reflection (V, H), coherent transmission down (V, H) and up (V, H), 2 x 2 diffuse reflection at (mu, mu, pi)."""
        n = len(mu_above)
        v = np.zeros((n, 10))
        args = (frequency, eps_above) if substrate else (frequency, eps_above, eps_below)
        v[:, 0:2] = cls._rows(obj.specular_reflection_matrix(*args, mu_above, 2), n).T
        if not substrate:
            v[:, 2:4] = cls._rows(obj.coherent_transmission_matrix(frequency, eps_above, eps_below, mu_above, 2), n).T
            v[:, 4:6] = cls._rows(obj.coherent_transmission_matrix(frequency, eps_below, eps_above, mu_below, 2), n).T
        if callable(getattr(obj, "diffuse_reflection_matrix", None)):
            v[:, 6:10] = cls._dense(obj.diffuse_reflection_matrix(*args, mu_above, mu_above, np.pi, 2), n).reshape(n, 4)
        return v

    @staticmethod
    def snell_from_air(eps, mu0):
        eps = complex(eps)
        return np.sqrt(eps - (1.0 - np.asarray(mu0) ** 2) + 0j).real / np.sqrt(eps).real

    def _extras(self, layers_of, batch, packer, sensor0, sps, freqs):
        """The PackedFirstOrderExtras of a packed group, or None when the device evaluates everything.  The effective
        permittivities the host evaluations need are the caller's own when the group's emmodels are evaluated on the host
        (batch.host_layer); otherwise `layers_of(batch)` -- DortContext.first_order_layers: one run of the solver without
        extras, of which only layer_out [n_pairs, Lmax, 5] is read -- gives the device's."""
        rough = [[i for i, itf in enumerate(sp.interfaces) if not isinstance(itf, Flat)] for sp in sps]
        host_sub = [sp.substrate is not None and substrate_kind(sp.substrate, "A") == "host" for sp in sps]
        ems = packer.host_emmodels
        if not any(rough) and not any(host_sub) and ems is None:
            return None
        F, S, Lmax = len(freqs), len(sps), int(batch.struct.n_layers_max)
        mu0 = np.cos(np.atleast_1d(sensor0.theta_inc))
        T = len(mu0)
        if ems is not None:
            lay = batch.host_layer.reshape(F, S, Lmax, 4)
            eps = lay[..., 2] + 1j * lay[..., 3]
        else:
            lay = np.asarray(layers_of(batch)).reshape(F, S, Lmax, 5)
            self.launches += 1
            eps = lay[..., 0] + 1j * lay[..., 1]
        interfaces = phases = None
        if any(rough) or any(host_sub):
            nslots = max(len(r) + int(h) for r, h in zip(rough, host_sub))
            slot = -np.ones((F, S, Lmax + 1), np.int32)
            values = np.zeros((F, S, nslots, T, 10))
            for fi, f in enumerate(freqs):
                for s, sp in enumerate(sps):
                    L = sp.nlayer
                    e = [1.0 + 0j] + list(eps[fi, s, :L])
                    mus = [mu0] + [self.snell_from_air(x, mu0) for x in e[1:]]
                    for k, i in enumerate(rough[s]):
                        slot[fi, s, i] = k
                        values[fi, s, k] = self.boundary_values(sp.interfaces[i], float(f), e[i], e[i + 1], mus[i], mus[i + 1])
                    if host_sub[s]:
                        k = len(rough[s])
                        slot[fi, s, L] = k
                        values[fi, s, k] = self.boundary_values(sp.substrate, float(f), e[L], None, mus[L], None, substrate=True)
            interfaces = (slot, values)
        if ems is not None:
            phases = np.zeros((F, S, Lmax, T, 4, 2, 2))
            for (fi, s), layer_ems in ems.items():
                for l, em in enumerate(layer_ems):
                    if batch.host_layer.reshape(F, S, Lmax, 4)[fi, s, l, 0] == 0.0:
                        continue
                    mu = self.snell_from_air(eps[fi, s, l], mu0)
                    for t in range(T):
                        both = np.array([-mu[t], mu[t]])
                        p = em.phase(both, both, np.pi, 2)
                        p = np.asarray(getattr(p, "values", p), float)[:2, :2, 0]
                        # P(-mu, mu), P(mu, -mu), P(mu, mu), P(-mu, -mu): [scattered, incident]
                        phases[fi, s, l, t] = p[:, :, 0, 1], p[:, :, 1, 0], p[:, :, 1, 1], p[:, :, 0, 0]
        return PackedFirstOrderExtras(F * S, Lmax, T, interfaces=interfaces, phase_samples=phases)


class _Packer(DORT):
    """DORT's packing of layers, kinds and host scalars for this solver: the dense matrices DORT evaluates on its streams
    (rough interfaces / substrates, phase matrices of host emmodels) are not made -- the per-angle numbers this solver
    needs instead are evaluated by IterativeFirstOrder._extras -- and the emmodel objects of a host group are kept."""

    host_emmodels = None

    def _substrates_on_host(self, *args, **kwargs):
        return None

    def _interfaces_on_host(self, *args, **kwargs):
        return None

    def _evaluate_on_host(self, sensor0, sps, freqs, entries, nl, Lmax, sensor_of):
        import copy

        F, S = len(freqs), len(sps)
        hl = np.zeros((F, S, Lmax, 4))
        hl[..., 2] = 1.0
        one = np.array([1.0, 0.55, 0.1])
        self.host_emmodels = {}
        for fi, f in enumerate(freqs):
            sensor = sensor_of.get(float(f))
            if sensor is None:
                sensor = copy.copy(sensor0)
                sensor.frequency = float(f)
            for s, sp in enumerate(sps):
                ems = [self._emmodel_instance(entries[s][l], sensor, layer) for l, layer in enumerate(sp.layers)]
                self.host_emmodels[(fi, s)] = ems
                for l, em in enumerate(ems):
                    ks = em.ks(one, 2) if callable(getattr(em, "ks", None)) else em.ks
                    ka = em.ka(one, 2) if callable(getattr(em, "ka", None)) else em.ka
                    eps = complex(em.effective_permittivity())
                    hl[fi, s, l] = self._isotropic(ks, "ks"), self._isotropic(ka, "ka"), eps.real, eps.imag
        return hl, np.zeros((F, S, Lmax), np.int32), np.zeros((F, S, Lmax, 1, 2, 6, 6))


class _Solution(LayeredSolution):
    """Outputs of the device batches of one call, addressable per simulation and stackable as one Result."""

    def __init__(self, solver, sensors, packs, sens_idx, pack_idx):
        LayeredSolution.__init__(self, solver, sensors, packs, sens_idx, pack_idx)
        self.no_substrate = []

    def add_group(self, sel, out, sp0, columns=None, no_substrate=None):
        LayeredSolution.add_group(self, sel, out, sp0, columns)
        self.no_substrate.append(sp0.substrate is None if no_substrate is None else no_substrate)

    def warn(self):
        """The reference's two warnings, once per run."""
        albedo = np.concatenate([o.diag[:, 0] for o in self.outputs])
        high = albedo > 0.5
        if high.any():
            smrt_warn(f"Warning : scattering albedo might be too high for iterative method in {int(high.sum())} simulation(s) "
                      f"(largest: {np.nanmax(albedo):.2f}). Limit is around 0.5.")
        tau = np.concatenate([o.diag[:, 1] for o, none in zip(self.outputs, self.no_substrate) if none] or [np.zeros(0)])
        shallow = tau < 5
        if shallow.any():
            smrt_warn(f"The solver has detected that {int(shallow.sum())} snowpack(s) are optically shallow (smallest "
                      f"tau={np.nanmin(tau):g}) and no substrate has been set, meaning that the space under the snowpack is "
                      "vacuum and that the snowpack is shallow enough to affect the signal measured at the surface. This is "
                      "usually not wanted. Either increase the thickness of the snowpack or set a substrate. If wanted, add a "
                      "transparent substrate to suppress this warning")

    def _coords(self, sensor):
        coords = [("theta_inc", sensor.theta_inc_deg), ("polarization_inc", POLA), ("polarization", POLA)]
        return ([("contribution", CONTRIBUTIONS)] if self.solver.return_contributions else []) + coords

    def _values(self, values):
        """[..., 4, n, 2, 2] -> the total, or [..., 5, n, 2, 2] with the total first."""
        total = values[..., 0, :, :, :] + values[..., 1, :, :, :] + values[..., 2, :, :, :] + values[..., 3, :, :, :]
        if not self.solver.return_contributions:
            return total
        return np.concatenate([total[..., None, :, :, :], values], axis=-4)

    def result(self, i):
        sensor = self.sensors[self.sens_idx[i]]
        out, row = self.outputs[self.group_of[i]], self.row_of[i]
        make, labelled = result_factory(sensor)
        other, L = self._other(i, labelled)
        other["backscatter_layer"] = labelled(out.layer_backscatter[row][:L + 1].copy(),
                                              [("layer", np.arange(-1, L))] + self._coords(sensor)[-3:], name="backscatter_layer")
        return make(sensor, self._values(out.values[row]), self._coords(sensor), other_data=other)

    def stacked_result(self, plan):
        grid = self._grid(plan)
        if grid is None:
            return None
        sensor0, lead, shape = grid
        out, order = self.outputs[0], self.row_of
        values = self._values(out.values[order])
        data = LabeledArray(values.reshape(shape + values.shape[1:]), lead + self._coords(sensor0))
        other, nl, Lmax = self._stacked_layers(lead, shape)
        lb = out.layer_backscatter[order][:, :Lmax + 1].copy()
        lb[np.arange(Lmax + 1)[None, :] > nl[:, None]] = np.nan
        other["backscatter_layer"] = LabeledArray(lb.reshape(shape + lb.shape[1:]), lead + [("layer", np.arange(-1, Lmax))]
                                                  + self._coords(sensor0)[-3:], name="backscatter_layer")
        return make_result(sensor0, data, other_data=other)
