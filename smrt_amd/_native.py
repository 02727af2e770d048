"""ctypes binding of libsmrt_dort.so (include/smrt_dort.h).

This is the ONLY way the package computes anything: there is no CPU fallback.  If the shared library is missing or no
MI355X is visible, `DortContext()` raises `SMRTError`.
"""
from __future__ import annotations

import ctypes as C
import os
import threading

import numpy as np

from .core.error import SMRTError

_HERE = os.path.dirname(os.path.abspath(__file__))
# SMRT_DORT_LIB: an alternative build of the same library (profiling / ablation builds made by tools/), never a fallback
LIB_PATH = os.environ.get("SMRT_DORT_LIB") or os.path.join(_HERE, "csrc", "libsmrt_dort.so")

EM_CODES = {"iba": 0, "dmrt_qca_shortrange": 1, "dmrt_qcacp_shortrange": 2, "nonscattering": 3, "host": 4,
            "iba_inverted": 5, "iba_host": 6, "rayleigh_host": 7}   # include/smrt_dort.h: SMRT_EM_*
MS_CODES = {"exponential": 0, "sticky_hard_spheres": 1, "independent_sphere": 2, "teubner_strey": 3,   # SMRT_MS_*
            # the models on the unified parameters are reparametrisations (core/layer.py: device_microstructure_params)
            "unified_scaled_exponential": 0, "unified_sticky_hard_spheres": 1, "unified_teubner_strey": 3,
            "exponential_complex_k": 4, "sticky_hard_spheres_complex_k": 5, "independent_sphere_complex_k": 6,
            "teubner_strey_complex_k": 7}   # SMRT_MS_*_COMPLEX_K: layers of the strong-contrast-expansion emmodels
SUBSTRATE_CODES = {"flat": 1, "reflector": 2, "host": 3, "soil_wegmuller": 4, "soil_qnh": 5, "rough_choudhury79": 6}
SOIL_KINDS = ("soil_wegmuller", "soil_qnh", "rough_choudhury79")   # SMRT_SUBSTRATE_SOIL_WEGMULLER .. _ROUGH_CHOUDHURY
NORM_CODES = {False: 0, None: 0, True: 1, "auto": 1, "forced": 2}
STATUS_MESSAGES = {
    1: "The eigen-decomposition did not converge in DORT.",
    2: "The re-normalization of the phase function exceeds the predefined threshold of 30%. This is likely because "
       "of a too large grain size or a bug in the phase function.",
    3: "The diagonalization failed in DORT: single scattering albedo >= 1 in a layer (too large grain size for the "
       "emmodel?).",
    4: "The boundary-condition system is singular.",
    5: "Invalid layer properties (temperature above the freezing point, fewer than two streams in a layer, or -- for an "
       "emmodel evaluated on the host -- a negative ka / permittivity or a stream count that differs from the device's).",
    6: "process_coherent_layers: the last layer is coherent, or two successive layers are coherent; this is not supported.",
    7: "snowpack optically too deep for the successive_order workspace: N sublayers",
    8: "The multi-Fresnel chain gave a non-finite brightness temperature (a reflectivity of 1, e.g. at a grazing angle, divides "
       "by zero).",
}
# status 5 of a pair on a Choudhury substrate whose layer inputs are sound: the device has no other reason left
CHOUDHURY_OUT_OF_RANGE = ("Invalid input (status 5): the Choudhury reflectivity is outside its validity range, ksigma must be "
                          "<= 0.1 (ksigma << 1) -- or invalid layer properties")


def status_message(batch, status, default=None):
    """The text of a pair's status word; status 5 of a batch on a Choudhury substrate names the model's validity range."""
    if status == 5 and int(batch.struct.substrate_kind) == SUBSTRATE_CODES["rough_choudhury79"]:
        return CHOUDHURY_OUT_OF_RANGE
    return default if default is not None else STATUS_MESSAGES.get(status)


class SmrtBatch(C.Structure):
    """struct smrt_batch of include/smrt_dort.h."""

    _fields_ = [
        ("n_snowpacks", C.c_int32),
        ("n_layers_max", C.c_int32),
        ("n_frequencies", C.c_int32),
        ("n_theta", C.c_int32),
        ("emmodel", C.c_int32),
        ("microstructure", C.c_int32),
        ("mode", C.c_int32),
        ("n_max_stream", C.c_int32),
        ("m_max", C.c_int32),
        ("phase_normalization", C.c_int32),
        ("rayleigh_jeans", C.c_int32),
        ("substrate_kind", C.c_int32),
        ("n_layers", C.POINTER(C.c_int32)),
        ("thickness", C.POINTER(C.c_double)),
        ("frac_volume", C.POINTER(C.c_double)),
        ("temperature", C.POINTER(C.c_double)),
        ("micro_p1", C.POINTER(C.c_double)),
        ("micro_p2", C.POINTER(C.c_double)),
        ("frequency", C.POINTER(C.c_double)),
        ("theta", C.POINTER(C.c_double)),
        ("phi", C.c_double),
        ("substrate_p1", C.POINTER(C.c_double)),
        ("substrate_p2", C.POINTER(C.c_double)),
        ("substrate_temperature", C.POINTER(C.c_double)),
        ("atm_tb_down", C.POINTER(C.c_double)),
        ("atm_tb_up", C.POINTER(C.c_double)),
        ("atm_transmittance", C.POINTER(C.c_double)),
        ("prune_optical_depth", C.c_double),
        ("layer_kind", C.POINTER(C.c_int32)),
        ("host_layer", C.POINTER(C.c_double)),
        ("host_streams", C.POINTER(C.c_int32)),
        ("host_phase", C.POINTER(C.c_double)),
        ("process_coherent_layers", C.c_int32),
        ("host_substrate", C.POINTER(C.c_double)),
        ("host_substrate_coh", C.POINTER(C.c_double)),
        ("host_interface_slot", C.POINTER(C.c_int32)),
        ("host_interface", C.POINTER(C.c_double)),
        ("host_interface_coh", C.POINTER(C.c_double)),
        ("host_interface_slots", C.c_int32),
        ("liquid_water", C.POINTER(C.c_double)),
        ("host_iba_coeff", C.POINTER(C.c_double)),
        ("rough_kind", C.POINTER(C.c_int32)),
        ("rough_params", C.POINTER(C.c_double)),
    ]


# rough boundaries the device evaluates itself (SMRT_ROUGH_*): the device_kind of the interface / substrate classes
ROUGH_CODES = {"geometrical_optics": 1, "geometrical_optics_backscatter": 2, "iem_fung92": 3}
ROUGH_M_MAX = 4   # SMRT_ROUGH_M_MAX


def rough_matrix_bytes(n_pairs, slots, has_substrate, n_max_stream, modes):
    """Bytes of the dense matrices the device builds for the rough boundaries of n_pairs pairs (include/smrt_dort.h)."""
    ne = 3 * int(n_max_stream)
    return 8 * int(n_pairs) * int(modes) * ne * ne * (4 * int(slots) + (1 if has_substrate else 0))


def _dptr(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


class PackedBatch:
    """Host-side packed batch: S snowpacks x F frequencies (pair p = f * S + s, frequency-major like
    Model.prepare_simulations, smrt/core/model.py:485-502)."""

    def __init__(self, n_layers, thickness, frac_volume, temperature, micro_p1, micro_p2, frequency, theta,
                 emmodel="iba", microstructure="exponential", mode="P", n_max_stream=32, m_max=2,
                 phase_normalization="auto", rayleigh_jeans=False, phi=np.pi, substrate=None, atmosphere=None,
                 prune_deep_snowpack=None, layer_kind=None, host_emmodel=None, process_coherent_layers=False,
                 host_interfaces=None, liquid_water=None, host_scalars=None, rough=None):
        """substrate: None or (kind, p1[F][S], p2[F][S], temperature[S]) with kind "flat" (p1 + i p2 = permittivity) or
        "reflector" (p1, p2 = specular reflection V, H); temperature <= 0 or NaN = no emission.  For the kinds
        "soil_wegmuller", "soil_qnh", "rough_choudhury79" (passive mode) two more elements, tail1[S][2] and tail2[S][2]: p1 + i p2
        is the soil permittivity, and the arrays handed to the library are p1 followed by tail1 (roughness_rms, 0 | H, Q) and
        p2 followed by tail2 (0, 0 | Nv, Nh) (include/smrt_dort.h).
        atmosphere: None or (tb_down[F], tb_up[F], transmittance[F]).
        prune_deep_snowpack: None / False, True (= 6, smrt/rtsolver/dort.py:176-177) or the optical depth itself.
        layer_kind: None, or [S][Lmax] integer codes EM_CODES[emmodel] + 16 * MS_CODES[microstructure] for snowpacks
        that mix emmodels / microstructure models (smrt/core/model.py:529-582).
        host_interfaces: None, or (slot[F*S][Lmax] int (-1: Flat), matrices[F*S][slots][modes][4][NE][NE],
        coh[F*S][slots][4][NE]) for rough interfaces evaluated by the caller (include/smrt_dort.h: SMRT_INTERFACE_HOST).
        host_scalars: None, or (host_layer [F*S][Lmax][4] = ks, ka, Re eps_eff, Im eps_eff; iba_coeff [F*S][Lmax]) for layers of
            kind "iba_host" (SMRT_EM_IBA_HOST: IBA's phase function on the device, the layer's scalars from the caller)
        liquid_water: None (dry snow) or [S][Lmax] water / (ice + water) volume of every layer; frac_volume is then the
        volume fraction of ice + water (include/smrt_dort.h).
        host_emmodel: None, or (host_layer[F*S][Lmax][4], host_streams[F*S][Lmax], host_phase[F*S][Lmax][modes][2][NE][NE])
        for the layers of kind "host" (emmodels evaluated by the caller, include/smrt_dort.h)."""
        self.n_layers = np.ascontiguousarray(n_layers, dtype=np.int32)
        S = len(self.n_layers)
        two_d = lambda a: np.ascontiguousarray(np.asarray(a, dtype=np.float64).reshape(S, -1))  # noqa: E731
        self.thickness = two_d(thickness)
        self.frac_volume = two_d(frac_volume)
        self.temperature = two_d(temperature)
        self.micro_p1 = two_d(micro_p1)
        self.micro_p2 = two_d(micro_p2 if micro_p2 is not None else np.zeros_like(self.micro_p1))
        Lmax = self.thickness.shape[1]
        for a in (self.frac_volume, self.temperature, self.micro_p1, self.micro_p2):
            if a.shape != (S, Lmax):
                raise SMRTError("per-layer arrays of a batch must share the shape (n_snowpacks, n_layers_max)")
        if self.n_layers.min() < 1 or self.n_layers.max() > Lmax:
            raise SMRTError("n_layers out of range")
        self.frequency = np.ascontiguousarray(np.atleast_1d(frequency), dtype=np.float64)
        self.theta = np.ascontiguousarray(np.atleast_1d(theta), dtype=np.float64)
        self.mode = mode
        s = SmrtBatch()
        s.n_snowpacks, s.n_layers_max, s.n_frequencies, s.n_theta = S, Lmax, len(self.frequency), len(self.theta)
        s.emmodel = EM_CODES[emmodel]
        s.microstructure = MS_CODES[microstructure]
        s.mode = 0 if mode == "P" else 1
        s.n_max_stream = int(n_max_stream)
        s.m_max = int(m_max)
        s.phase_normalization = NORM_CODES[phase_normalization]
        s.rayleigh_jeans = 1 if rayleigh_jeans else 0
        s.n_layers = self.n_layers.ctypes.data_as(C.POINTER(C.c_int32))
        s.thickness, s.frac_volume, s.temperature = _dptr(self.thickness), _dptr(self.frac_volume), _dptr(self.temperature)
        s.micro_p1, s.micro_p2 = _dptr(self.micro_p1), _dptr(self.micro_p2)
        s.frequency, s.theta = _dptr(self.frequency), _dptr(self.theta)
        s.phi = float(phi)
        if prune_deep_snowpack is True:
            prune_deep_snowpack = 6.0
        s.prune_optical_depth = float(prune_deep_snowpack) if prune_deep_snowpack else 0.0
        s.substrate_kind = 0
        if substrate is not None and substrate[0] == "host":
            # rough substrate, active mode: ("host", R[F*S][modes][NE][NE], Rcoh[F*S][modes][NE]) -- the dense reflection
            # matrices of the bottom boundary per azimuth mode and their specular diagonals (include/smrt_dort.h)
            # passive mode: one mode, Rcoh holds the EMISSIVITY diagonal and a fourth element the temperatures [S]
            FS, nm, ne = S * len(self.frequency), (int(m_max) + 1 if mode == "A" else 1), 3 * int(n_max_stream)
            self.host_substrate = np.ascontiguousarray(np.asarray(substrate[1], np.float64).reshape(FS, nm, ne, ne))
            self.host_substrate_coh = np.ascontiguousarray(np.asarray(substrate[2], np.float64).reshape(FS, nm, ne))
            s.substrate_kind = SUBSTRATE_CODES["host"]
            s.host_substrate, s.host_substrate_coh = _dptr(self.host_substrate), _dptr(self.host_substrate_coh)
            if len(substrate) > 3:
                self.sub_T = np.ascontiguousarray(np.nan_to_num(np.broadcast_to(np.asarray(substrate[3], np.float64), (S,)), nan=0.0))
                s.substrate_temperature = _dptr(self.sub_T)
        elif substrate is not None:
            kind, q1, q2, ts = substrate[:4]
            F = len(self.frequency)
            self.sub_p1 = np.ascontiguousarray(np.broadcast_to(np.asarray(q1, np.float64), (F, S)))
            self.sub_p2 = np.ascontiguousarray(np.broadcast_to(np.asarray(q2, np.float64), (F, S)))
            if kind in SOIL_KINDS:
                if len(substrate) != 6:
                    raise SMRTError(f"a '{kind}' substrate needs its two parameter tails, [n_snowpacks][2] each")
                if mode != "P":
                    raise SMRTError(f"the '{kind}' substrate is evaluated on the device in passive mode only")
                tails = [np.broadcast_to(np.asarray(t, np.float64), (S, 2)).reshape(-1) for t in substrate[4:]]
                # one array each: [F][S] permittivities, then [S][2] parameters (sub_p1 / sub_p2 stay views of the front)
                self.sub_p1_full = np.ascontiguousarray(np.concatenate([self.sub_p1.reshape(-1), tails[0]]))
                self.sub_p2_full = np.ascontiguousarray(np.concatenate([self.sub_p2.reshape(-1), tails[1]]))
                self.sub_p1, self.sub_p2 = self.sub_p1_full[:F * S].reshape(F, S), self.sub_p2_full[:F * S].reshape(F, S)
            self.sub_T = np.ascontiguousarray(np.nan_to_num(np.broadcast_to(np.asarray(ts, np.float64), (S,)), nan=0.0))
            s.substrate_kind = SUBSTRATE_CODES[kind]
            s.substrate_p1, s.substrate_p2, s.substrate_temperature = _dptr(self.sub_p1), _dptr(self.sub_p2), _dptr(self.sub_T)
            if kind in SOIL_KINDS:
                s.substrate_p1, s.substrate_p2 = _dptr(self.sub_p1_full), _dptr(self.sub_p2_full)
        if atmosphere is not None:
            F = len(self.frequency)
            self.atm = [np.ascontiguousarray(np.broadcast_to(np.asarray(a, np.float64), (F,))) for a in atmosphere]
            s.atm_tb_down, s.atm_tb_up, s.atm_transmittance = (_dptr(a) for a in self.atm)
        if layer_kind is not None:
            self.layer_kind = np.ascontiguousarray(np.asarray(layer_kind, dtype=np.int32).reshape(S, Lmax))
            s.layer_kind = self.layer_kind.ctypes.data_as(C.POINTER(C.c_int32))
        if host_emmodel is not None:
            hl, hs, hp = host_emmodel
            FS = S * len(self.frequency)
            modes = 1 if mode == "P" else int(m_max) + 1
            ne = int(n_max_stream) * (2 if mode == "P" else 3)
            self.host_layer = np.ascontiguousarray(np.asarray(hl, np.float64).reshape(FS, Lmax, 4))
            self.host_streams = np.ascontiguousarray(np.asarray(hs, np.int32).reshape(FS, Lmax))
            self.host_phase = np.ascontiguousarray(np.asarray(hp, np.float64).reshape(FS, Lmax, modes, 2, ne, ne))
            s.host_layer, s.host_phase = _dptr(self.host_layer), _dptr(self.host_phase)
            s.host_streams = self.host_streams.ctypes.data_as(C.POINTER(C.c_int32))
        if host_scalars is not None:
            if host_emmodel is not None:
                raise SMRTError("host_emmodel and host_scalars are alternatives (one host_layer array)")
            FS = S * len(self.frequency)
            self.host_layer = np.ascontiguousarray(np.asarray(host_scalars[0], np.float64).reshape(FS, Lmax, 4))
            self.host_iba_coeff = np.ascontiguousarray(np.asarray(host_scalars[1], np.float64).reshape(FS, Lmax))
            s.host_layer, s.host_iba_coeff = _dptr(self.host_layer), _dptr(self.host_iba_coeff)
        s.process_coherent_layers = 1 if process_coherent_layers else 0
        if liquid_water is not None:
            self.liquid_water = two_d(liquid_water)
            if self.liquid_water.shape != (S, Lmax):
                raise SMRTError("per-layer arrays of a batch must share the shape (n_snowpacks, n_layers_max)")
            s.liquid_water = _dptr(self.liquid_water)
        if host_interfaces is not None:
            FS, nm, ne = S * len(self.frequency), (int(m_max) + 1 if mode == "A" else 1), 3 * int(n_max_stream)
            slot = np.asarray(host_interfaces[0], dtype=np.int32).reshape(FS, Lmax)
            nslots = int(np.asarray(host_interfaces[1]).size // (FS * nm * 4 * ne * ne))
            self.host_interface_slot = np.ascontiguousarray(slot)
            self.host_interface = np.ascontiguousarray(np.asarray(host_interfaces[1], np.float64).reshape(FS, nslots, nm, 4, ne, ne))
            self.host_interface_coh = np.ascontiguousarray(np.asarray(host_interfaces[2], np.float64).reshape(FS, nslots, 4, ne))
            s.host_interface_slot = self.host_interface_slot.ctypes.data_as(C.POINTER(C.c_int32))
            s.host_interface, s.host_interface_coh = _dptr(self.host_interface), _dptr(self.host_interface_coh)
            s.host_interface_slots = nslots
        if rough is not None:
            # rough boundaries evaluated on the device: (kind[S][Lmax + 1] int (ROUGH_CODES, 0: not rough),
            # params[S][Lmax + 1][4]); entry l is the interface on top of layer l, entry n_layers the substrate, which then
            # travels as substrate=("flat", Re eps, Im eps, temperature)
            self.rough_kind = np.ascontiguousarray(np.asarray(rough[0], dtype=np.int32).reshape(S, Lmax + 1))
            self.rough_params = np.ascontiguousarray(np.asarray(rough[1], dtype=np.float64).reshape(S, Lmax + 1, 4))
            s.rough_kind = self.rough_kind.ctypes.data_as(C.POINTER(C.c_int32))
            s.rough_params = _dptr(self.rough_params)
        self.struct = s

    @property
    def n_pairs(self):
        return int(self.struct.n_snowpacks) * int(self.struct.n_frequencies)

    @property
    def out_stride(self):
        return (2 if self.mode == "P" else 9) * int(self.struct.n_theta)

    def out_shape(self):
        nt = int(self.struct.n_theta)
        return (2, nt) if self.mode == "P" else (3, 3, nt)


class FirstOrderExtras(C.Structure):
    """struct smrt_first_order_extras of include/smrt_dort.h."""

    _fields_ = [
        ("n_interface_slots", C.c_int32),
        ("reserved", C.c_int32),
        ("host_interface_slot", C.POINTER(C.c_int32)),
        ("host_interface_values", C.POINTER(C.c_double)),
        ("host_phase_samples", C.POINTER(C.c_double)),
    ]


class PackedFirstOrderExtras:
    """What the iterative first-order solver needs beyond a PackedBatch (include/smrt_dort.h: smrt_first_order_extras), for
    a batch of `n_pairs` = F * S pairs, `n_layers_max` layers and `n_theta` incidence angles:
    interfaces: None, or (slot [F*S][Lmax + 1] int (-1: evaluated on the device; entry n_layers of a snowpack: its substrate),
        values [F*S][slots][n_theta][10]) for the interfaces / substrates evaluated by the caller;
    phase_samples: None, or [F*S][Lmax][n_theta][4][2][2] for the layers of kind "host"."""

    def __init__(self, n_pairs, n_layers_max, n_theta, interfaces=None, phase_samples=None):
        x = FirstOrderExtras()
        FS, L, T = int(n_pairs), int(n_layers_max), int(n_theta)
        if interfaces is not None:
            slot = np.asarray(interfaces[0], dtype=np.int32)
            if slot.size != FS * (L + 1):
                raise SMRTError("the interface slot table must have the shape (n_pairs, n_layers_max + 1)")
            self.slot = np.ascontiguousarray(slot.reshape(FS, L + 1))
            values = np.asarray(interfaces[1], np.float64)
            if values.size == 0 or values.size % (FS * T * 10):
                raise SMRTError("the interface values must have the shape (n_pairs, slots, n_theta, 10)")
            nslots = values.size // (FS * T * 10)
            if self.slot.min() < -1 or self.slot.max() >= nslots:
                raise SMRTError("interface slot out of range")
            self.values = np.ascontiguousarray(values.reshape(FS, nslots, T, 10))
            x.n_interface_slots = nslots
            x.host_interface_slot = self.slot.ctypes.data_as(C.POINTER(C.c_int32))
            x.host_interface_values = _dptr(self.values)
        if phase_samples is not None:
            ph = np.asarray(phase_samples, np.float64)
            if ph.size != FS * L * T * 16:
                raise SMRTError("the phase samples must have the shape (n_pairs, n_layers_max, n_theta, 4, 2, 2)")
            self.phase_samples = np.ascontiguousarray(ph.reshape(FS, L, T, 4, 2, 2))
            x.host_phase_samples = _dptr(self.phase_samples)
        self.struct = x


class FirstOrderOutput:
    """Outputs of the first-order solver for `pair_count` pairs: values [4 contributions][n_theta][2][2], status, layers
    [Lmax][5], layer_backscatter [Lmax + 1][n_theta][2][2], diag (largest albedo, optical depth)."""

    def __init__(self, batch, pair_count):
        Lmax, nt = int(batch.struct.n_layers_max), int(batch.struct.n_theta)
        self.values = np.empty((pair_count, 4, nt, 2, 2))
        self.status = np.empty(pair_count, dtype=np.int32)
        self.layers = np.empty((pair_count, Lmax, 5))
        self.layer_backscatter = np.empty((pair_count, Lmax + 1, nt, 2, 2))
        self.diag = np.empty((pair_count, 2))

    def pointers(self):
        return (_dptr(self.values), self.status.ctypes.data_as(C.POINTER(C.c_int32)), _dptr(self.layers),
                _dptr(self.layer_backscatter), _dptr(self.diag))


class SecondOrderExtras(C.Structure):
    """struct smrt_second_order_extras of include/smrt_dort.h."""

    _fields_ = [
        ("compute_scattering_interlayer", C.c_int32),
        ("reserved", C.c_int32),
        ("workspace_budget_bytes", C.c_int64),
        ("first_order", C.POINTER(FirstOrderExtras)),
        ("substrate_diffuse_modes", C.POINTER(C.c_double)),
    ]


class PackedSecondOrderExtras:
    """What the iterative second-order solver needs beyond a PackedBatch (include/smrt_dort.h: smrt_second_order_extras), for a
    batch of `n_pairs` = F * S pairs: the interlayer switch, the workspace budget (None: the library's default), the
    first-order extras (a PackedFirstOrderExtras or None) and, for a substrate with diffuse reflection, substrate_modes
    [F*S][Lmax][n_theta][n_max_stream][m_max][2][2][3]."""

    def __init__(self, batch, interlayer=False, workspace_budget=None, first_order=None, substrate_modes=None):
        x = SecondOrderExtras()
        x.compute_scattering_interlayer = 1 if interlayer else 0
        x.workspace_budget_bytes = int(workspace_budget or 0)
        self.first_order = first_order
        if first_order is not None:
            x.first_order = C.pointer(first_order.struct)
        if substrate_modes is not None:
            b = batch.struct
            shape = (batch.n_pairs, int(b.n_layers_max), int(b.n_theta), int(b.n_max_stream), int(b.m_max), 2, 2, 3)
            modes = np.asarray(substrate_modes, np.float64)
            if modes.size != int(np.prod(shape)):
                raise SMRTError(f"the substrate modes must have the shape {shape}")
            self.substrate_modes = np.ascontiguousarray(modes.reshape(shape))
            x.substrate_diffuse_modes = _dptr(self.substrate_modes)
        self.struct = x


class SecondOrderOutput(FirstOrderOutput):
    """As FirstOrderOutput with values [7 contributions][n_theta][2][2]: the four of the first order, then the three order-2
    mechanisms; layer_backscatter is order 1 + order 2."""

    def __init__(self, batch, pair_count):
        FirstOrderOutput.__init__(self, batch, pair_count)
        self.values = np.empty((pair_count, 7, int(batch.struct.n_theta), 2, 2))


class SuccessiveOrderOutput:
    """Outputs of the successive-order solver for `pair_count` pairs: values [2][n_theta][n_iteration_max + 1] kelvin (the
    last entry of the order axis is the total), status, layers [Lmax][5] and streams [1 + n_max_stream] as DORT's, sublayers
    [Lmax], max_radiance [n_iteration_max] (largest emerging radiance of every order run), orders (orders run)."""

    def __init__(self, batch, pair_count, n_iteration_max):
        Lmax, nt, nmax = int(batch.struct.n_layers_max), int(batch.struct.n_theta), int(batch.struct.n_max_stream)
        self.raw = np.empty((pair_count, n_iteration_max + 1, 2, nt))   # as the device writes it
        self.status = np.empty(pair_count, dtype=np.int32)
        self.layers = np.empty((pair_count, Lmax, 5))
        self.streams = np.empty((pair_count, 1 + nmax))
        self.sublayers = np.empty((pair_count, Lmax), dtype=np.int32)
        self.max_radiance = np.empty((pair_count, n_iteration_max))
        self.orders = np.empty(pair_count, dtype=np.int32)

    @property
    def values(self):
        return np.moveaxis(self.raw, 1, 3)

    def pointers(self):
        i32 = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))  # noqa: E731
        return (_dptr(self.raw), i32(self.status), _dptr(self.layers), _dptr(self.streams), i32(self.sublayers),
                _dptr(self.max_radiance), i32(self.orders))


class SuccessiveOrderActiveOutput:
    """Outputs of the successive-order backscatter solver for `pair_count` pairs: values [3][3][n_theta_inc][n_iteration_max
    + 1] (scattered polarisation, incident polarisation, angle, order; the last entry of the order axis is the total), status,
    layers [Lmax][5] and streams [1 + n_max_stream] as DORT's, sublayers [Lmax], max_radiance [m_max + 2][n_iteration_max] (per
    pass -- coherent, then the modes -- the largest emerging radiance of every order run, NaN after the stop), orders [m_max +
    2] (orders run per pass)."""

    def __init__(self, batch, pair_count, n_iteration_max, n_theta_inc, m_max):
        Lmax, nmax = int(batch.struct.n_layers_max), int(batch.struct.n_max_stream)
        self.values = np.empty((pair_count, 3, 3, n_theta_inc, n_iteration_max + 1))
        self.status = np.empty(pair_count, dtype=np.int32)
        self.layers = np.empty((pair_count, Lmax, 5))
        self.streams = np.empty((pair_count, 1 + nmax))
        self.sublayers = np.empty((pair_count, Lmax), dtype=np.int32)
        self.max_radiance = np.empty((pair_count, m_max + 2, n_iteration_max))
        self.orders = np.empty((pair_count, m_max + 2), dtype=np.int32)

    def pointers(self):
        i32 = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))  # noqa: E731
        return (_dptr(self.values), i32(self.status), _dptr(self.layers), _dptr(self.streams), i32(self.sublayers),
                _dptr(self.max_radiance), i32(self.orders))


class MultiFresnelOutput:
    """Outputs of the multi-Fresnel thermal emission solver for `pair_count` pairs: values [n_theta][2] kelvin (V, H), status
    [n_theta] (one word per element), layers_used, tau_snowpack, layers [Lmax][5] as DORT's; streams [1 + n_theta] holds the
    sensor cosines the way DORT's output holds its air streams (Result.other_data)."""

    def __init__(self, batch, pair_count, mu):
        Lmax, nt = int(batch.struct.n_layers_max), int(batch.struct.n_theta)
        self.values = np.empty((pair_count, nt, 2))
        self.status = np.empty((pair_count, nt), dtype=np.int32)
        self.layers_used = np.empty(pair_count, dtype=np.int32)
        self.tau_snowpack = np.empty(pair_count)
        self.layers = np.empty((pair_count, Lmax, 5))
        order = np.sort(np.asarray(mu, float))[::-1]
        self.streams = np.broadcast_to(np.concatenate([[float(nt)], order]), (pair_count, 1 + nt))

    def pointers(self):
        i32 = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))  # noqa: E731
        return (_dptr(self.values), i32(self.status), i32(self.layers_used), _dptr(self.tau_snowpack), _dptr(self.layers))


class LrmParams(C.Structure):
    """struct smrt_lrm_params of include/smrt_dort.h."""
    _fields_ = [("altitude", C.c_double), ("pulse_bandwidth", C.c_double), ("antenna_gain", C.c_double), ("gamma", C.c_double),
                ("off_nadir_angle", C.c_double), ("nominal_gate", C.c_double), ("pulse_sigma", C.c_double),
                ("ngate", C.c_int32), ("oversampling", C.c_int32), ("n_mu", C.c_int32), ("shift", C.c_int32),
                ("return_contributions", C.c_int32), ("return_oversampled", C.c_int32), ("skip_pfs_convolution", C.c_int32),
                ("reserved", C.c_int32), ("t_inc", C.POINTER(C.c_double)), ("sigma_surface", C.POINTER(C.c_double)),
                ("surface_slope", C.POINTER(C.c_double)), ("interface_values", C.POINTER(C.c_double))]


class PackedLrmParams:
    """What one group of the nadir LRM altimetry solver shares beyond its PackedBatch (include/smrt_dort.h: smrt_lrm_params).
    sensor: an Altimeter (one frequency); t_inc: the times of the incidence samples (None or one value: the fast path);
    sigma_surface / surface_slope: [S] metres / radians or None; interface_values: [F * S][Lmax + 1][1 + n_mu] or None."""

    def __init__(self, sensor, oversampling=10, t_inc=None, return_contributions=False, return_oversampled=False,
                 skip_pfs_convolution=False, sigma_surface=None, surface_slope=None, interface_values=None, pulse_sigma=None):
        s = LrmParams()
        s.altitude, s.pulse_bandwidth, s.antenna_gain = float(sensor.altitude), float(sensor.pulse_bandwidth), float(sensor.antenna_gain)
        beamwidth = (sensor.beamwidth_alongtrack + sensor.beamwidth_acrosstrack) / 2   # a 'circular' antenna pattern
        s.gamma = 2 / 0.6931471805599453 * np.sin(np.deg2rad(beamwidth) / 2) ** 2
        s.off_nadir_angle, s.nominal_gate = float(sensor.off_nadir_angle), float(sensor.nominal_gate)
        s.pulse_sigma = float(pulse_sigma) if pulse_sigma is not None else 0.513 / float(sensor.pulse_bandwidth)
        s.ngate, s.oversampling = int(sensor.ngate), int(oversampling)
        self.t_inc = np.ascontiguousarray(np.atleast_1d(0.0 if t_inc is None else t_inc), dtype=np.float64)
        s.n_mu = len(self.t_inc)
        s.t_inc = _dptr(self.t_inc)
        # the first sub-gate at or after the nominal gate, found as the reference finds it (lrm_waveform_model.py: PFS_PTR_PDF)
        t_gate = np.arange(0, s.ngate * s.oversampling) / (s.pulse_bandwidth * s.oversampling)
        s.shift = int((t_gate - s.nominal_gate / s.pulse_bandwidth >= 0).argmax())
        s.return_contributions, s.return_oversampled = int(bool(return_contributions)), int(bool(return_oversampled))
        s.skip_pfs_convolution = int(bool(skip_pfs_convolution))
        for name, value in (("sigma_surface", sigma_surface), ("surface_slope", surface_slope), ("interface_values", interface_values)):
            if value is not None:
                setattr(self, name, np.ascontiguousarray(value, dtype=np.float64))
                setattr(s, name, _dptr(getattr(self, name)))
        self.struct = s

    @property
    def n_samples(self):
        return self.struct.ngate * (self.struct.oversampling if self.struct.return_oversampled else 1)

    @property
    def n_sub(self):
        return self.struct.ngate * self.struct.oversampling

    @property
    def vertical_rows(self):
        return 2 * self.struct.n_mu + 1 if self.struct.n_mu > 1 else 3 if self.struct.return_contributions else 1

    @property
    def rows(self):
        return 3 if self.struct.return_contributions else self.vertical_rows if self.struct.skip_pfs_convolution else 1


class LrmOutput:
    """Outputs of the nadir LRM altimetry solver for `pair_count` pairs: values [rows][samples], status, z_gate [samples], layers
    [Lmax][5] (Re eps, Im eps, ks, ka, backward scattering / eps), vertical [vertical rows][ngate x oversampling]."""

    def __init__(self, batch, params, pair_count):
        Lmax = int(batch.struct.n_layers_max)
        self.values = np.empty((pair_count, params.rows, params.n_samples))
        self.status = np.empty(pair_count, dtype=np.int32)
        self.z_gate = np.empty((pair_count, params.n_samples))
        self.layers = np.empty((pair_count, Lmax, 5))
        self.vertical = np.empty((pair_count, params.vertical_rows, params.n_sub))

    def pointers(self):
        return (_dptr(self.values), self.status.ctypes.data_as(C.POINTER(C.c_int32)), _dptr(self.z_gate), _dptr(self.layers),
                _dptr(self.vertical))


class SarParams(C.Structure):
    """struct smrt_sar_params of include/smrt_dort.h."""
    _fields_ = [(name, C.c_double) for name in (
        "altitude", "pulse_bandwidth", "nominal_gate", "pulse_repetition_frequency", "wavelength", "velocity", "alpha", "pitch_angle",
        "roll_angle", "sigma_p", "theta_lim", "gamma_x", "gamma_y", "l_gamma", "lz", "pu", "nu_coherent")] + [(name, C.c_int32) for name in (
            "ngate", "ndoppler", "oversampling_time", "oversampling_doppler", "return_oversampled", "n_rows", "n_tables", "reserved")] + [
        ("table_sigma", C.POINTER(C.c_double)), ("table_index", C.POINTER(C.c_int32)), ("boundary_values", C.POINTER(C.c_double)),
        ("row_map", C.POINTER(C.c_int32))] + [(name, C.c_int32) for name in (
            "delay_doppler_model", "slant_range_correction", "delay_window_widening", "reserved2")] + [(name, C.c_double) for name in (
                "h14_pu", "h14_gamma", "burst_duration")]


SAR_MODELS = {"dinardo18": 0, "halimi14": 1}   # include/smrt_dort.h: SMRT_SAR_DINARDO18, SMRT_SAR_HALIMI14

# (sigma_g, A_g) of the Gaussian that stands for the point target response, by "<approximation>:<Doppler window>"
# (smrt/rtsolver/delay_doppler_model/delay_doppler_utils.py: MacArthur 1976, 1978; Brown 1977; Ray et al. 2015; Dinardo et al. 2018;
# the least-squares fits made for SMRT)
PTR_GAUSSIAN_APPROXIMATION = {
    "gaussian-macarthur76:rect": (0.443, 1.0), "gaussian-macarthur78:rect": (0.513, 1.0), "gaussian-brown77:rect": (0.425, 1.0),
    "gaussian-ray15:hamming": (0.5408, 1.0055), "gaussian-dinardo18:hamming": (0.55, 1.0),
    "gaussian-smrt:hamming": (0.54973121, 1.00758253), "gaussian-smrt:rect": (0.36018704, 1.01917462), "gaussian-smrt-test:rect": (0.1, 1),
}


def ptr_gaussian_approximation(ptr, window):
    key = ptr if ":" in ptr else None if window is None else ptr + ":" + window
    if key is None:
        raise SMRTError("doppler_window must be set to use this DDM model. Can be 'rect', 'hamming', or ...")
    if key not in PTR_GAUSSIAN_APPROXIMATION:
        raise SMRTError(f"no Gaussian approximation of the point target response is known as '{key}'")
    return PTR_GAUSSIAN_APPROXIMATION[key]


class PackedSarParams:
    """What one group of the nadir SAR altimetry solver shares beyond its PackedBatch (include/smrt_dort.h: smrt_sar_params): the
    constants of Dinardo et al. 2018 for `sensor` (an Altimeter, one frequency), the distinct sigma_surface of the group
    (table_sigma) with the index of every snowpack into them, boundary_values [S][Lmax + 1][4] and row_map [S][2 (Lmax + 1) + 2]."""

    def __init__(self, sensor, table_sigma, table_index, boundary_values, row_map, n_rows=1, oversampling_time=4, oversampling_doppler=4,
                 return_oversampled=False, ptr_doppler="gaussian-smrt", model="dinardo18", slant_range_correction=True,
                 delay_window_widening=1):
        from .core.globalconstants import C_SPEED

        s = SarParams()
        f, h, B = float(sensor.frequency), float(sensor.altitude), float(sensor.pulse_bandwidth)
        prf, velocity, alpha, ndoppler = float(sensor.pulse_repetition_frequency), float(sensor.velocity), float(sensor.alpha), int(sensor.ndoppler)
        wavelength = C_SPEED / f
        s.delay_doppler_model = SAR_MODELS[model]
        if model == "halimi14":   # (H14 after eq. 3 and eq. 14, 19; the constants of Dinardo18 below are filled and not read)
            beamwidth = (float(sensor.beamwidth_alongtrack) + float(sensor.beamwidth_acrosstrack)) / 2
            s.slant_range_correction, s.delay_window_widening = int(bool(slant_range_correction)), int(delay_window_widening)
            s.h14_pu = wavelength ** 2 * float(sensor.antenna_gain) ** 2 * C_SPEED / (4 * (4 * np.pi) ** 2 * h ** 3) * ndoppler ** 2
            s.h14_gamma = 1 / (2 * np.log(2)) * np.sin(np.deg2rad(beamwidth)) ** 2
            s.burst_duration = ndoppler / prf
            sigma_g, a_g = 1.0, 1.0
        else:
            sigma_g, a_g = ptr_gaussian_approximation(ptr_doppler, sensor.doppler_window)
        lx = (C_SPEED * h * prf) / (2 * velocity * ndoppler * f)            # R15 eq. 14, along track
        ly = np.sqrt(C_SPEED * h / (alpha * B))                              # R15 eq. 21, across track
        lz = C_SPEED / (2 * B)
        gamma_x = 8 * np.log(2) / np.deg2rad(sensor.beamwidth_alongtrack) ** 2     # D18 eq. 27
        gamma_y = 8 * np.log(2) / np.deg2rad(sensor.beamwidth_acrosstrack) ** 2
        k = (float(sensor.antenna_gain) * wavelength * ndoppler) ** 2 * lx * ly / (4 * np.pi * h ** 4) * np.sqrt(2 * np.pi) * a_g ** 2 * sigma_g ** 2
        beta0 = np.sqrt(C_SPEED / (B * h)) * np.sqrt(2)
        beta12 = 1 / (2 * np.pi / wavelength * h * beta0) ** 2 + beta0 ** 2 / 4
        s.altitude, s.pulse_bandwidth, s.nominal_gate, s.pulse_repetition_frequency = h, B, float(sensor.nominal_gate), prf
        s.wavelength, s.velocity, s.alpha = wavelength, velocity, alpha
        s.pitch_angle, s.roll_angle = float(sensor.pitch_angle), float(sensor.roll_angle)
        s.sigma_p, s.theta_lim = sigma_g / B, lz / (alpha * lx)                 # D18 eq. 18
        s.gamma_x, s.gamma_y, s.l_gamma, s.lz = gamma_x, gamma_y, alpha * h / (2 * gamma_y), lz
        s.pu = k / np.sqrt(B) * np.sqrt(2)                                     # R15 eq. 37
        s.nu_coherent = 1 / beta12
        s.ngate, s.ndoppler = int(sensor.ngate), ndoppler
        s.oversampling_time, s.oversampling_doppler = int(oversampling_time), int(oversampling_doppler)
        s.return_oversampled, s.n_rows = int(bool(return_oversampled)), int(n_rows)
        self.table_sigma = np.ascontiguousarray(np.atleast_1d(table_sigma), dtype=np.float64)
        self.table_index = np.ascontiguousarray(table_index, dtype=np.int32)
        self.boundary_values = np.ascontiguousarray(boundary_values, dtype=np.float64)
        self.row_map = np.ascontiguousarray(row_map, dtype=np.int32)
        s.n_tables = len(self.table_sigma)
        s.table_sigma, s.boundary_values = _dptr(self.table_sigma), _dptr(self.boundary_values)
        s.table_index = self.table_index.ctypes.data_as(C.POINTER(C.c_int32))
        s.row_map = self.row_map.ctypes.data_as(C.POINTER(C.c_int32))
        self.struct = s

    @property
    def n_sub(self):
        return self.struct.ngate * self.struct.oversampling_time

    @property
    def shape(self):
        """(rows, delays, Doppler frequencies) of the map of one pair."""
        s = self.struct
        if s.return_oversampled:
            return s.n_rows, s.ngate * s.oversampling_time, s.ndoppler * s.oversampling_doppler
        return s.n_rows, s.ngate, s.ndoppler


class SarOutput:
    """Outputs of the nadir SAR altimetry solver for `pair_count` pairs: values [rows][delays][Doppler], status, z_gate [delays],
    layers [Lmax][5] as the LRM solver's, vertical [ngate x oversampling_time] the volume backscatter per sub-gate, echo
    [Lmax + 1][4] per boundary (two-way travel time, attenuated coherent and incoherent echo, shift in samples)."""

    def __init__(self, batch, params, pair_count):
        Lmax = int(batch.struct.n_layers_max)
        self.values = np.empty((pair_count,) + params.shape)
        self.status = np.empty(pair_count, dtype=np.int32)
        self.z_gate = np.empty((pair_count, params.shape[1]))
        self.layers = np.empty((pair_count, Lmax, 5))
        self.vertical = np.empty((pair_count, params.n_sub))
        self.echo = np.empty((pair_count, Lmax + 1, 4))

    def pointers(self):
        return (_dptr(self.values), self.status.ctypes.data_as(C.POINTER(C.c_int32)), _dptr(self.z_gate), _dptr(self.layers),
                _dptr(self.vertical), _dptr(self.echo))


_lib = None


def load_library():
    """Load libsmrt_dort.so; fail loudly when it is not built (see __graft_entry__.build)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise SMRTError(f"{LIB_PATH} is missing: build it with `python __graft_entry__.py` (hipcc, gfx950). "
                        "smrt_amd has no CPU fallback.")
    lib = C.CDLL(LIB_PATH)
    P = C.POINTER
    lib.smrt_dort_version.restype = C.c_char_p
    lib.smrt_dort_out_stride.argtypes = [P(SmrtBatch)]
    lib.smrt_dort_out_stride.restype = C.c_int32
    lib.smrt_dort_create.argtypes = [P(C.c_void_p), C.c_int32]
    lib.smrt_dort_create.restype = C.c_int32
    lib.smrt_dort_destroy.argtypes = [C.c_void_p]
    lib.smrt_dort_destroy.restype = None
    lib.smrt_dort_last_error.argtypes = [C.c_void_p]
    lib.smrt_dort_last_error.restype = C.c_char_p
    lib.smrt_dort_run.argtypes = [C.c_void_p, P(SmrtBatch), C.c_int64, C.c_int64, P(C.c_double), P(C.c_int32),
                                  P(C.c_double), P(C.c_double)]
    lib.smrt_dort_run.restype = C.c_int32
    lib.smrt_dort_upload.argtypes = [C.c_void_p, P(SmrtBatch), C.c_int64, C.c_int64]
    lib.smrt_dort_upload.restype = C.c_int32
    lib.smrt_dort_run_pairs.argtypes = [C.c_void_p, P(SmrtBatch), P(C.c_int64), C.c_int64, P(C.c_double), P(C.c_int32),
                                        P(C.c_double), P(C.c_double)]
    lib.smrt_dort_run_pairs.restype = C.c_int32
    lib.smrt_dort_upload_pairs.argtypes = [C.c_void_p, P(SmrtBatch), P(C.c_int64), C.c_int64]
    lib.smrt_dort_upload_pairs.restype = C.c_int32
    lib.smrt_dort_ft_even_phase.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_double, C.c_double, C.c_double, C.c_double,
                                            C.c_double, P(C.c_double), C.c_int32, P(C.c_double), C.c_int32, C.c_int32, C.c_int32,
                                            P(C.c_double)]
    lib.smrt_dort_ft_even_phase.restype = C.c_int32
    lib.smrt_dort_rough_matrices.argtypes = [C.c_void_p, P(SmrtBatch), P(C.c_int32), P(C.c_double), P(C.c_double), P(C.c_double),
                                             P(C.c_double)]
    lib.smrt_dort_rough_matrices.restype = C.c_int32
    lib.smrt_dort_rough_info.argtypes = [C.c_void_p, P(C.c_double), C.c_int32]
    lib.smrt_dort_rough_info.restype = C.c_int32
    lib.smrt_dort_pair_cost.argtypes = [C.c_void_p, P(C.c_double)]
    lib.smrt_dort_pair_cost.restype = C.c_int32
    lib.smrt_dort_launch_info.argtypes = [C.c_void_p, P(C.c_int64), C.c_int32]
    lib.smrt_dort_launch_info.restype = C.c_int32
    lib.smrt_dort_comm_library.argtypes = [C.c_char_p, C.c_int32, P(C.c_int32)]
    lib.smrt_dort_comm_library.restype = C.c_int32
    lib.smrt_dort_comm_unique_id.argtypes = [C.c_char_p]
    lib.smrt_dort_comm_unique_id.restype = C.c_int32
    lib.smrt_dort_comm_init.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_char_p]
    lib.smrt_dort_comm_init.restype = C.c_int32
    lib.smrt_dort_comm_init_all.argtypes = [P(C.c_void_p), C.c_int32]
    lib.smrt_dort_comm_init_all.restype = C.c_int32
    lib.smrt_dort_comm_destroy.argtypes = [C.c_void_p]
    lib.smrt_dort_comm_destroy.restype = C.c_int32
    lib.smrt_dort_gather.argtypes = [C.c_void_p, C.c_int32, P(C.c_int64), P(C.c_double), P(C.c_int32)]
    lib.smrt_dort_gather.restype = C.c_int32
    lib.smrt_dort_comm_allreduce_max.argtypes = [C.c_void_p, P(C.c_double), C.c_int32]
    lib.smrt_dort_comm_allreduce_max.restype = C.c_int32
    lib.smrt_dort_abi.argtypes = [P(C.c_int32), C.c_int32]
    lib.smrt_dort_abi.restype = C.c_int32
    lib.smrt_dort_launch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    lib.smrt_dort_launch.restype = C.c_int32
    lib.smrt_dort_sync.argtypes = [C.c_void_p]
    lib.smrt_dort_sync.restype = C.c_int32
    lib.smrt_dort_download.argtypes = [C.c_void_p, P(C.c_double), P(C.c_int32), P(C.c_double), P(C.c_double)]
    lib.smrt_dort_download.restype = C.c_int32
    lib.smrt_dort_last_kernel_ms.argtypes = [C.c_void_p]
    lib.smrt_dort_last_kernel_ms.restype = C.c_double
    lib.smrt_dort_kernel_breakdown.argtypes = [C.c_void_p, C.c_int32, P(C.c_double)]
    lib.smrt_dort_kernel_breakdown.restype = C.c_int32
    lib.smrt_dort_total_kernel_ms.argtypes = [C.c_void_p, P(C.c_int64), C.c_int32]
    lib.smrt_dort_total_kernel_ms.restype = C.c_double
    lib.smrt_dort_set_block_threads.argtypes = [C.c_void_p, C.c_int32]
    lib.smrt_dort_set_block_threads.restype = C.c_int32
    lib.smrt_dort_set_pipeline.argtypes = [C.c_void_p, C.c_int32]
    lib.smrt_dort_set_pipeline.restype = C.c_int32
    lib.smrt_dort_set_diagonalisation.argtypes = [C.c_void_p, C.c_int32]
    lib.smrt_dort_set_diagonalisation.restype = C.c_int32
    lib.smrt_dort_set_prep.argtypes = [C.c_void_p, C.c_int32]
    lib.smrt_dort_set_prep.restype = C.c_int32
    lib.smrt_dort_set_class_lists.argtypes = [C.c_void_p, C.c_int32]
    lib.smrt_dort_set_class_lists.restype = C.c_int32
    lib.smrt_dort_gather_plan.argtypes = [C.c_int32, C.c_int32, C.c_int32, P(C.c_int64), C.c_void_p, C.c_int32,
                                          P(C.c_int64), P(C.c_int64)]
    lib.smrt_dort_gather_plan.restype = C.c_int32
    lib.smrt_dort_finish_reg_lds_bytes.argtypes = [C.c_int32, C.c_int32]
    lib.smrt_dort_finish_reg_lds_bytes.restype = C.c_int32
    lib.smrt_dort_finish_strip_lds_bytes.argtypes = [C.c_int32, C.c_int32, C.c_int32]
    lib.smrt_dort_finish_strip_lds_bytes.restype = C.c_int32
    lib.smrt_dort_jacobi_lds_bytes.argtypes = [C.c_int32, C.c_int32, C.c_int32]
    lib.smrt_dort_jacobi_lds_bytes.restype = C.c_int32
    lib.smrt_dort_sum_n3.argtypes = [C.c_void_p]
    lib.smrt_dort_sum_n3.restype = C.c_double
    lib.smrt_dort_stage_cycles.argtypes = [C.c_void_p, P(C.c_double)]
    lib.smrt_dort_stage_cycles.restype = C.c_int32
    lib.smrt_dort_device_count.argtypes = []
    lib.smrt_dort_device_count.restype = C.c_int32
    lib.smrt_gauss_legendre_positive.argtypes = [C.c_int32, P(C.c_double), P(C.c_double)]
    lib.smrt_gauss_legendre_positive.restype = C.c_int32
    X = P(FirstOrderExtras)
    lib.smrt_first_order_out_stride.argtypes = [P(SmrtBatch)]
    lib.smrt_first_order_out_stride.restype = C.c_int32
    lib.smrt_first_order_run_pairs.argtypes = [C.c_void_p, P(SmrtBatch), X, P(C.c_int64), C.c_int64, P(C.c_double), P(C.c_int32),
                                               P(C.c_double), P(C.c_double), P(C.c_double)]
    lib.smrt_first_order_run_pairs.restype = C.c_int32
    lib.smrt_first_order_upload_pairs.argtypes = [C.c_void_p, P(SmrtBatch), X, P(C.c_int64), C.c_int64]
    lib.smrt_first_order_upload_pairs.restype = C.c_int32
    lib.smrt_first_order_launch.argtypes = [C.c_void_p]
    lib.smrt_first_order_launch.restype = C.c_int32
    lib.smrt_first_order_sync.argtypes = [C.c_void_p]
    lib.smrt_first_order_sync.restype = C.c_int32
    lib.smrt_first_order_download.argtypes = [C.c_void_p, P(C.c_double), P(C.c_int32), P(C.c_double), P(C.c_double), P(C.c_double)]
    lib.smrt_first_order_download.restype = C.c_int32
    lib.smrt_first_order_kernel_ms.argtypes = [C.c_void_p, P(C.c_double)]
    lib.smrt_first_order_kernel_ms.restype = C.c_int32
    lib.smrt_first_order_abi.argtypes = [P(C.c_int32), C.c_int32]
    lib.smrt_first_order_abi.restype = C.c_int32
    X2 = P(SecondOrderExtras)
    lib.smrt_second_order_out_stride.argtypes = [P(SmrtBatch)]
    lib.smrt_second_order_run_pairs.argtypes = [C.c_void_p, P(SmrtBatch), X2, P(C.c_int64), C.c_int64, P(C.c_double), P(C.c_int32),
                                                P(C.c_double), P(C.c_double), P(C.c_double)]
    lib.smrt_second_order_upload_pairs.argtypes = [C.c_void_p, P(SmrtBatch), X2, P(C.c_int64), C.c_int64]
    lib.smrt_second_order_launch.argtypes = [C.c_void_p]
    lib.smrt_second_order_sync.argtypes = [C.c_void_p]
    lib.smrt_second_order_download.argtypes = [C.c_void_p, P(C.c_double), P(C.c_int32), P(C.c_double), P(C.c_double), P(C.c_double)]
    lib.smrt_second_order_kernel_ms.argtypes = [C.c_void_p, P(C.c_double)]
    lib.smrt_second_order_abi.argtypes = [P(C.c_int32), C.c_int32]
    for name in ("out_stride", "run_pairs", "upload_pairs", "launch", "sync", "download", "kernel_ms", "abi"):
        getattr(lib, "smrt_second_order_" + name).restype = C.c_int32
    so_out = [P(C.c_double), P(C.c_int32), P(C.c_double), P(C.c_double), P(C.c_int32), P(C.c_double), P(C.c_int32)]
    lib.smrt_successive_order_out_stride.argtypes = [P(SmrtBatch), C.c_int32]
    lib.smrt_successive_order_out_stride.restype = C.c_int32
    lib.smrt_successive_order_run_pairs.argtypes = [C.c_void_p, P(SmrtBatch), C.c_int32, C.c_double, C.c_int64, P(C.c_int64), C.c_int64] + so_out
    lib.smrt_successive_order_run_pairs.restype = C.c_int32
    lib.smrt_successive_order_upload_pairs.argtypes = [C.c_void_p, P(SmrtBatch), C.c_int32, C.c_double, C.c_int64, P(C.c_int64), C.c_int64]
    lib.smrt_successive_order_upload_pairs.restype = C.c_int32
    lib.smrt_successive_order_launch.argtypes = [C.c_void_p]
    lib.smrt_successive_order_launch.restype = C.c_int32
    lib.smrt_successive_order_sync.argtypes = [C.c_void_p]
    lib.smrt_successive_order_sync.restype = C.c_int32
    lib.smrt_successive_order_download.argtypes = [C.c_void_p] + so_out
    lib.smrt_successive_order_download.restype = C.c_int32
    lib.smrt_successive_order_kernel_ms.argtypes = [C.c_void_p, P(C.c_double)]
    lib.smrt_successive_order_kernel_ms.restype = C.c_int32
    lib.smrt_successive_order_launch_info.argtypes = [C.c_void_p, P(C.c_int64), C.c_int32]
    lib.smrt_successive_order_launch_info.restype = C.c_int32
    soa_in = [C.c_void_p, P(SmrtBatch), C.c_int32, C.c_double, C.c_int32, P(C.c_double), C.c_int32, C.c_int32, C.c_int64, P(C.c_int64),
              C.c_int64]
    lib.smrt_so_active_out_stride.argtypes = [C.c_int32, C.c_int32]
    lib.smrt_so_active_out_stride.restype = C.c_int32
    lib.smrt_so_active_run_pairs.argtypes = soa_in + so_out
    lib.smrt_so_active_run_pairs.restype = C.c_int32
    lib.smrt_so_active_upload_pairs.argtypes = soa_in
    lib.smrt_so_active_upload_pairs.restype = C.c_int32
    lib.smrt_so_active_launch.argtypes = [C.c_void_p]
    lib.smrt_so_active_launch.restype = C.c_int32
    lib.smrt_so_active_sync.argtypes = [C.c_void_p]
    lib.smrt_so_active_sync.restype = C.c_int32
    lib.smrt_so_active_download.argtypes = [C.c_void_p] + so_out
    lib.smrt_so_active_download.restype = C.c_int32
    lib.smrt_so_active_kernel_ms.argtypes = [C.c_void_p, P(C.c_double)]
    lib.smrt_so_active_kernel_ms.restype = C.c_int32
    lib.smrt_so_active_launch_info.argtypes = [C.c_void_p, P(C.c_int64), C.c_int32]
    lib.smrt_so_active_launch_info.restype = C.c_int32
    mf_out = [P(C.c_double), P(C.c_int32), P(C.c_int32), P(C.c_double), P(C.c_double)]
    mf_in = [C.c_void_p, P(SmrtBatch), P(C.c_double), C.c_double, C.c_int32, P(C.c_int64), C.c_int64]
    lib.smrt_multifresnel_out_stride.argtypes = [P(SmrtBatch)]
    lib.smrt_multifresnel_out_stride.restype = C.c_int32
    lib.smrt_multifresnel_run_pairs.argtypes = mf_in + mf_out
    lib.smrt_multifresnel_run_pairs.restype = C.c_int32
    lib.smrt_multifresnel_upload_pairs.argtypes = mf_in
    lib.smrt_multifresnel_upload_pairs.restype = C.c_int32
    lib.smrt_multifresnel_launch.argtypes = [C.c_void_p]
    lib.smrt_multifresnel_launch.restype = C.c_int32
    lib.smrt_multifresnel_sync.argtypes = [C.c_void_p]
    lib.smrt_multifresnel_sync.restype = C.c_int32
    lib.smrt_multifresnel_download.argtypes = [C.c_void_p] + mf_out
    lib.smrt_multifresnel_download.restype = C.c_int32
    lib.smrt_multifresnel_kernel_ms.argtypes = [C.c_void_p, P(C.c_double)]
    lib.smrt_multifresnel_kernel_ms.restype = C.c_int32
    lrm_out = [P(C.c_double), P(C.c_int32), P(C.c_double), P(C.c_double), P(C.c_double)]
    lrm_in = [C.c_void_p, P(SmrtBatch), P(LrmParams), P(C.c_int64), C.c_int64]
    lib.smrt_lrm_out_stride.argtypes = [P(LrmParams)]
    lib.smrt_lrm_run_pairs.argtypes = lrm_in + lrm_out
    lib.smrt_lrm_upload_pairs.argtypes = lrm_in
    lib.smrt_lrm_launch.argtypes = [C.c_void_p]
    lib.smrt_lrm_sync.argtypes = [C.c_void_p]
    lib.smrt_lrm_layers.argtypes = [C.c_void_p, P(C.c_double)]
    lib.smrt_lrm_download.argtypes = [C.c_void_p] + lrm_out
    lib.smrt_lrm_kernel_ms.argtypes = [C.c_void_p, P(C.c_double)]
    lib.smrt_lrm_abi.argtypes = [P(C.c_int32), C.c_int32]
    for name in ("out_stride", "run_pairs", "upload_pairs", "launch", "sync", "layers", "download", "kernel_ms", "abi"):
        getattr(lib, "smrt_lrm_" + name).restype = C.c_int32
    sar_out = [P(C.c_double), P(C.c_int32), P(C.c_double), P(C.c_double), P(C.c_double), P(C.c_double)]
    sar_in = [C.c_void_p, P(SmrtBatch), P(SarParams), P(C.c_int64), C.c_int64]
    lib.smrt_sar_out_stride.argtypes = [P(SarParams)]
    lib.smrt_sar_run_pairs.argtypes = sar_in + sar_out
    lib.smrt_sar_upload_pairs.argtypes = sar_in
    lib.smrt_sar_launch.argtypes = [C.c_void_p]
    lib.smrt_sar_sync.argtypes = [C.c_void_p]
    lib.smrt_sar_download.argtypes = [C.c_void_p] + sar_out
    lib.smrt_sar_kernel_ms.argtypes = [C.c_void_p, P(C.c_double)]
    lib.smrt_sar_abi.argtypes = [P(C.c_int32), C.c_int32]
    for name in ("out_stride", "run_pairs", "upload_pairs", "launch", "sync", "download", "kernel_ms", "abi"):
        getattr(lib, "smrt_sar_" + name).restype = C.c_int32
    check_struct_layout(lib)
    _lib = lib
    return lib


def abi_layout(lib):
    """[sizeof(smrt_batch), offset of every field in declaration order] as the library was compiled (smrt_dort_abi)."""
    n = lib.smrt_dort_abi(None, 0)
    a = (C.c_int32 * n)()
    lib.smrt_dort_abi(a, n)
    return list(a)


def check_struct_layout(lib):
    """The ctypes declaration above must be the struct the library was compiled with: a stale binding would hand over
    a short or shifted struct and the library would read garbage pointers."""
    mine = [C.sizeof(SmrtBatch)] + [getattr(SmrtBatch, name).offset for name, _ in SmrtBatch._fields_]
    theirs = abi_layout(lib)
    if mine != theirs:
        raise SMRTError(f"smrt_batch layout mismatch between smrt_amd/_native.py {mine} and {LIB_PATH} {theirs}: "
                        "rebuild the library or update the binding (include/smrt_dort.h)")
    mine, theirs = first_order_extras_layout(), first_order_abi_layout(lib)
    if mine != theirs:
        raise SMRTError(f"smrt_first_order_extras layout mismatch between smrt_amd/_native.py {mine} and {LIB_PATH} {theirs}: "
                        "rebuild the library or update the binding (include/smrt_dort.h)")
    mine, theirs = second_order_extras_layout(), second_order_abi_layout(lib)
    if mine != theirs:
        raise SMRTError(f"smrt_second_order_extras layout mismatch between smrt_amd/_native.py {mine} and {LIB_PATH} {theirs}: "
                        "rebuild the library or update the binding (include/smrt_dort.h)")
    mine, theirs = lrm_params_layout(), lrm_abi_layout(lib)
    if mine != theirs:
        raise SMRTError(f"smrt_lrm_params layout mismatch between smrt_amd/_native.py {mine} and {LIB_PATH} {theirs}: "
                        "rebuild the library or update the binding (include/smrt_dort.h)")
    mine, theirs = sar_params_layout(), sar_abi_layout(lib)
    if mine != theirs:
        raise SMRTError(f"smrt_sar_params layout mismatch between smrt_amd/_native.py {mine} and {LIB_PATH} {theirs}: "
                        "rebuild the library or update the binding (include/smrt_dort.h)")


def sar_params_layout():
    """[sizeof, field offsets] of the ctypes declaration of smrt_sar_params."""
    return [C.sizeof(SarParams)] + [getattr(SarParams, name).offset for name, _ in SarParams._fields_]


def sar_abi_layout(lib):
    """The same as the library was compiled (smrt_sar_abi)."""
    n = lib.smrt_sar_abi(None, 0)
    a = (C.c_int32 * n)()
    lib.smrt_sar_abi(a, n)
    return list(a)


def lrm_params_layout():
    """[sizeof, field offsets] of the ctypes declaration of smrt_lrm_params."""
    return [C.sizeof(LrmParams)] + [getattr(LrmParams, name).offset for name, _ in LrmParams._fields_]


def lrm_abi_layout(lib):
    """The same as the library was compiled (smrt_lrm_abi)."""
    n = lib.smrt_lrm_abi(None, 0)
    a = (C.c_int32 * n)()
    lib.smrt_lrm_abi(a, n)
    return list(a)


def second_order_extras_layout():
    """[sizeof, field offsets] of the ctypes declaration of smrt_second_order_extras."""
    return [C.sizeof(SecondOrderExtras)] + [getattr(SecondOrderExtras, name).offset for name, _ in SecondOrderExtras._fields_]


def second_order_abi_layout(lib):
    """The same as the library was compiled (smrt_second_order_abi)."""
    n = lib.smrt_second_order_abi(None, 0)
    a = (C.c_int32 * n)()
    lib.smrt_second_order_abi(a, n)
    return list(a)


def first_order_extras_layout():
    """[sizeof, field offsets] of the ctypes declaration of smrt_first_order_extras."""
    return [C.sizeof(FirstOrderExtras)] + [getattr(FirstOrderExtras, name).offset for name, _ in FirstOrderExtras._fields_]


def first_order_abi_layout(lib):
    """The same as the library was compiled (smrt_first_order_abi)."""
    n = lib.smrt_first_order_abi(None, 0)
    a = (C.c_int32 * n)()
    lib.smrt_first_order_abi(a, n)
    return list(a)


EXPORTED_SYMBOLS = [
    "smrt_dort_out_stride", "smrt_dort_create", "smrt_dort_destroy", "smrt_dort_last_error", "smrt_dort_run",
    "smrt_dort_upload", "smrt_dort_upload_pairs", "smrt_dort_run_pairs", "smrt_dort_abi", "smrt_dort_pair_cost", "smrt_dort_ft_even_phase",
    "smrt_dort_launch_info", "smrt_dort_comm_library", "smrt_dort_comm_unique_id", "smrt_dort_comm_init", "smrt_dort_comm_init_all", "smrt_dort_comm_destroy", "smrt_dort_gather",
    "smrt_dort_comm_allreduce_max", "smrt_dort_launch", "smrt_dort_sync", "smrt_dort_download", "smrt_dort_last_kernel_ms", "smrt_dort_kernel_breakdown",
    "smrt_dort_total_kernel_ms", "smrt_dort_set_block_threads", "smrt_dort_set_pipeline", "smrt_dort_set_diagonalisation", "smrt_dort_set_prep", "smrt_dort_set_class_lists", "smrt_dort_sum_n3", "smrt_dort_stage_cycles", "smrt_dort_device_count", "smrt_gauss_legendre_positive",
    "smrt_dort_version", "smrt_dort_finish_reg_lds_bytes", "smrt_dort_finish_strip_lds_bytes", "smrt_dort_jacobi_lds_bytes", "smrt_dort_gather_plan",
    "smrt_first_order_out_stride", "smrt_first_order_run_pairs", "smrt_first_order_upload_pairs", "smrt_first_order_launch",
    "smrt_first_order_sync", "smrt_first_order_download", "smrt_first_order_kernel_ms", "smrt_first_order_abi",
    "smrt_second_order_out_stride", "smrt_second_order_run_pairs", "smrt_second_order_upload_pairs", "smrt_second_order_launch",
    "smrt_second_order_sync", "smrt_second_order_download", "smrt_second_order_kernel_ms", "smrt_second_order_abi",
    "smrt_successive_order_out_stride", "smrt_successive_order_run_pairs", "smrt_successive_order_upload_pairs",
    "smrt_successive_order_launch", "smrt_successive_order_sync", "smrt_successive_order_download",
    "smrt_successive_order_kernel_ms", "smrt_successive_order_launch_info",
    "smrt_so_active_out_stride", "smrt_so_active_run_pairs", "smrt_so_active_upload_pairs", "smrt_so_active_launch",
    "smrt_so_active_sync", "smrt_so_active_download", "smrt_so_active_kernel_ms", "smrt_so_active_launch_info",
    "smrt_multifresnel_out_stride", "smrt_multifresnel_run_pairs", "smrt_multifresnel_upload_pairs", "smrt_multifresnel_launch",
    "smrt_multifresnel_sync", "smrt_multifresnel_download", "smrt_multifresnel_kernel_ms",
    "smrt_lrm_out_stride", "smrt_lrm_run_pairs", "smrt_lrm_upload_pairs", "smrt_lrm_launch", "smrt_lrm_sync", "smrt_lrm_download",
    "smrt_lrm_kernel_ms", "smrt_lrm_abi", "smrt_lrm_layers",
    "smrt_sar_out_stride", "smrt_sar_run_pairs", "smrt_sar_upload_pairs", "smrt_sar_launch", "smrt_sar_sync", "smrt_sar_download",
    "smrt_sar_kernel_ms", "smrt_sar_abi",
    "smrt_dort_rough_matrices", "smrt_dort_rough_info",
]


class RoughMatrices:
    """What the solve reads for the rough boundaries of a batch (include/smrt_dort.h: host_interface*, host_substrate*), as
    the device builder or its CPU build fills it: slot [FS][Lmax] (-1: Flat), itf [FS][slots][modes][4][NE][NE],
    itf_coh [FS][slots][4][NE], sub [FS][modes][NE][NE], sub_coh [FS][modes][NE]."""

    def __init__(self, batch):
        s = batch.struct
        S, Lmax = int(s.n_snowpacks), int(s.n_layers_max)
        FS, ne = batch.n_pairs, 3 * int(s.n_max_stream)
        nm = int(s.m_max) + 1 if batch.mode == "A" else 1
        kinds = batch.rough_kind
        self.slots = max(int(np.count_nonzero(kinds[k, :batch.n_layers[k]])) for k in range(S))
        self.has_substrate = bool(kinds[0, batch.n_layers[0]])
        self.slot = -np.ones((FS, Lmax), np.int32)
        self.itf = np.zeros((FS, self.slots, nm, 4, ne, ne))
        self.itf_coh = np.zeros((FS, self.slots, 4, ne))
        self.sub = np.zeros((FS, nm, ne, ne))
        self.sub_coh = np.zeros((FS, nm, ne))

    def pointers(self):
        return (self.slot.ctypes.data_as(C.POINTER(C.c_int32)), _dptr(self.itf), _dptr(self.itf_coh), _dptr(self.sub),
                _dptr(self.sub_coh))


class BatchOutput:
    def __init__(self, batch, pair_count):
        Lmax, nmax = int(batch.struct.n_layers_max), int(batch.struct.n_max_stream)
        self.values = np.empty((pair_count,) + batch.out_shape(), dtype=np.float64)
        self.status = np.empty(pair_count, dtype=np.int32)
        self.layers = np.empty((pair_count, Lmax, 5), dtype=np.float64)
        self.streams = np.empty((pair_count, 1 + nmax), dtype=np.float64)


class DortContext:
    """One context per GPU (smrt_dort_create / smrt_dort_destroy)."""

    def __init__(self, device=0):
        self._lib = load_library()
        self._h = C.c_void_p()
        rc = self._lib.smrt_dort_create(C.byref(self._h), int(device))
        if rc != 0:
            self._h = C.c_void_p()
            raise SMRTError(f"smrt_dort_create(device={device}) failed with code {rc}: no usable MI355X GPU. "
                            "smrt_amd has no CPU fallback.")
        self.device = int(device)
        # a context is one set of device buffers and one stream: its calls are serialised (ctypes releases the GIL,
        # so two Python threads sharing a cached context would otherwise interleave upload / launch / download)
        self.lock = threading.RLock()

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self._lib.smrt_dort_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc, what):
        if rc != 0:
            raise SMRTError(f"{what} failed: {self._lib.smrt_dort_last_error(self._h).decode()}")

    def set_block_threads(self, n):
        self._check(self._lib.smrt_dort_set_block_threads(self._h, int(n)), "smrt_dort_set_block_threads")

    def set_pipeline(self, split=1):
        """1 (default): prep / Jacobi / finish kernels (passive, Flat interfaces: the strip finish kernels); 3: the
        register-resident finish kernel instead (N <= 64); 5: the strip kernels wherever supported; 4: no pivot-free finish
        kernel; 2: the four-matrix LDS finish kernel; 0: one fused kernel per pair (include/smrt_dort.h)."""
        self._check(self._lib.smrt_dort_set_pipeline(self._h, int(split)), "smrt_dort_set_pipeline")

    DIAGONALISATIONS = ("jacobi", "symmetric")   # SMRT_DIAG_*

    def set_diagonalisation(self, mode="default"):
        """How the layer eigenproblems are diagonalised on the three-kernel pipelines: "jacobi" (one-sided Jacobi on
        B = L+^T L-), "symmetric" (tridiagonalisation + implicit QL on B B^T where it is built: N <= 64) or "default"."""
        code = -1 if mode in (None, "default") else self.DIAGONALISATIONS.index(mode)
        self._check(self._lib.smrt_dort_set_diagonalisation(self._h, code), "smrt_dort_set_diagonalisation")

    PREPS = ("per_pair", "per_layer")   # SMRT_PREP_*

    def set_prep(self, mode="default"):
        """The prep stage of the LDS-resident passive pipelines: "per_pair" (one workgroup per pair), "per_layer" (pair setup,
        then one workgroup per (pair, layer) item in one launch per size class of rows) or "default"."""
        code = -1 if mode in (None, "default") else self.PREPS.index(mode)
        self._check(self._lib.smrt_dort_set_prep(self._h, code), "smrt_dort_set_prep")

    def set_class_lists(self, mode="default"):
        """The launches per size class of rows (per-layer prep, symmetric eigensolver): True, over the item lists of the classes
        built at upload; False, over every item of a pipeline pass (an item of another class leaves at once); or "default"."""
        code = -1 if mode in (None, "default") else int(bool(mode))
        self._check(self._lib.smrt_dort_set_class_lists(self._h, code), "smrt_dort_set_class_lists")

    def run(self, batch: PackedBatch, pair_begin=0, pair_count=-1, pairs=None) -> BatchOutput:
        """One shot (H2D, kernels, D2H) for the pair range, or for the listed pair indices (row i = pairs[i])."""
        if pairs is not None:
            pairs = np.ascontiguousarray(pairs, dtype=np.int64)
            o = BatchOutput(batch, len(pairs))
            with self.lock:
                self._check(self._lib.smrt_dort_run_pairs(
                    self._h, C.byref(batch.struct), pairs.ctypes.data_as(C.POINTER(C.c_int64)), len(pairs),
                    _dptr(o.values), o.status.ctypes.data_as(C.POINTER(C.c_int32)), _dptr(o.layers), _dptr(o.streams)),
                    "smrt_dort_run_pairs")
            return o
        if pair_count < 0:
            pair_count = batch.n_pairs - pair_begin
        o = BatchOutput(batch, pair_count)
        with self.lock:
            self._check(self._lib.smrt_dort_run(self._h, C.byref(batch.struct), pair_begin, pair_count, _dptr(o.values),
                                                o.status.ctypes.data_as(C.POINTER(C.c_int32)), _dptr(o.layers),
                                                _dptr(o.streams)), "smrt_dort_run")
        return o

    def upload(self, batch: PackedBatch, pair_begin=0, pair_count=-1, pairs=None):
        if pairs is not None:
            pairs = np.ascontiguousarray(pairs, dtype=np.int64)
            self._check(self._lib.smrt_dort_upload_pairs(self._h, C.byref(batch.struct),
                                                         pairs.ctypes.data_as(C.POINTER(C.c_int64)), len(pairs)),
                        "smrt_dort_upload_pairs")
            self._resident = (batch, len(pairs))
            return
        if pair_count < 0:
            pair_count = batch.n_pairs - pair_begin
        self._check(self._lib.smrt_dort_upload(self._h, C.byref(batch.struct), pair_begin, pair_count), "smrt_dort_upload")
        self._resident = (batch, pair_count)

    def launch(self, out_dev=None, status_dev=None):
        self._check(self._lib.smrt_dort_launch(self._h, C.c_void_p(out_dev or 0), C.c_void_p(status_dev or 0)),
                    "smrt_dort_launch")

    def sync(self):
        self._check(self._lib.smrt_dort_sync(self._h), "smrt_dort_sync")

    def download(self) -> BatchOutput:
        batch, pair_count = self._resident
        o = BatchOutput(batch, pair_count)
        self._check(self._lib.smrt_dort_download(self._h, _dptr(o.values), o.status.ctypes.data_as(C.POINTER(C.c_int32)),
                                                 _dptr(o.layers), _dptr(o.streams)), "smrt_dort_download")
        return o

    # ---- the solvers beside DORT: each has smrt_<prefix>_{run_pairs, upload_pairs, launch, sync, download, kernel_ms} ----
    # A packer turns a public method's arguments into (the C arguments after the context, the arguments of the output
    # class); the helpers below are what the public methods of every solver are made of.
    def _solver_call(self, symbol, *args):
        """One call into the library under the context's lock.  The convention of include/smrt_dort.h: negative means
        error (a count or 0 is success)."""
        with self.lock:
            rc = getattr(self._lib, symbol)(self._h, *args)
            if rc < 0:
                raise SMRTError(f"{symbol} failed: {self._lib.smrt_dort_last_error(self._h).decode()}")
        return rc

    def _solver_run(self, prefix, output, cargs, oargs):
        o = output(*oargs)
        self._solver_call(f"smrt_{prefix}_run_pairs", *cargs, *o.pointers())
        return o

    def _solver_upload(self, prefix, cargs, oargs):
        with self.lock:
            self._solver_call(f"smrt_{prefix}_upload_pairs", *cargs)
            setattr(self, f"_{prefix}_resident", oargs)

    def _solver_download(self, prefix, output):
        with self.lock:
            o = output(*getattr(self, f"_{prefix}_resident"))
            self._solver_call(f"smrt_{prefix}_download", *o.pointers())
        return o

    def _solver_kernel_ms(self, prefix, n):
        a = np.zeros(n)
        self._solver_call(f"smrt_{prefix}_kernel_ms", _dptr(a))
        return tuple(float(x) for x in a)

    def _solver_launch_info(self, prefix):
        a = np.zeros(4, dtype=np.int64)
        self._solver_call(f"smrt_{prefix}_launch_info", a.ctypes.data_as(C.POINTER(C.c_int64)), 4)   # (returns its number of entries)
        return dict(chunks=int(a[0]), reserved_bytes=int(a[1]), over_budget=int(a[2]), budget=int(a[3]))

    @staticmethod
    def _pair_list(batch, pairs):
        """(pointer, count, output rows) of an optional list of pair indices: (None, -1, every pair) without one."""
        if pairs is None:
            return None, -1, batch.n_pairs
        pairs = np.ascontiguousarray(pairs, dtype=np.int64)
        return pairs.ctypes.data_as(C.POINTER(C.c_int64)), len(pairs), len(pairs)

    # ---- the iterative first-order solver (smrt_first_order_*) ----------------------------------------------------
    @classmethod
    def _first_order_pack(cls, batch, extras, pairs):
        ptr, count, rows = cls._pair_list(batch, pairs)
        return (C.byref(batch.struct), C.byref(extras.struct) if extras is not None else None, ptr, count), (batch, rows)

    def first_order_run(self, batch: PackedBatch, extras=None, pairs=None) -> FirstOrderOutput:
        """One shot (H2D, two kernels, D2H) for every pair of the batch or the listed ones (row i = pairs[i])."""
        return self._solver_run("first_order", FirstOrderOutput, *self._first_order_pack(batch, extras, pairs))

    def first_order_upload(self, batch: PackedBatch, extras=None, pairs=None):
        """Split form (upload once, launch any number of times, sync, download).  Every call takes the context's lock,
        but the resident batch belongs to the context: a thread that uses the split form must hold `self.lock` from its
        upload to its download if another thread may solve on the same (cached) context meanwhile."""
        self._solver_upload("first_order", *self._first_order_pack(batch, extras, pairs))

    def first_order_launch(self):
        self._solver_call("smrt_first_order_launch")

    def first_order_sync(self):
        self._solver_call("smrt_first_order_sync")

    def first_order_download(self, layers_only=False) -> FirstOrderOutput:
        """The outputs of the last launch; layers_only: only `layers` (and `status`) are copied back, the other arrays of
        the returned object are left unset."""
        if not layers_only:
            return self._solver_download("first_order", FirstOrderOutput)
        with self.lock:
            o = FirstOrderOutput(*self._first_order_resident)
            ptrs = o.pointers()
            o.values = o.layer_backscatter = o.diag = None
            self._solver_call("smrt_first_order_download", None, ptrs[1], ptrs[2], None, None)
        return o

    def first_order_layers(self, batch: PackedBatch):
        """[n_pairs, Lmax, 5] layer scalars (Re eps, Im eps, ks, ka, 0) of every pair of the batch as the device computes
        them: one run of the solver without extras of which only layer_out is copied back."""
        with self.lock:
            self.first_order_upload(batch)
            self.first_order_launch()
            return self.first_order_download(layers_only=True).layers

    def first_order_kernel_ms(self):
        """HIP-event ms of the (pair, layer) kernel and of the (pair, angle) kernel of the last launch."""
        return self._solver_kernel_ms("first_order", 2)

    # ---- the iterative second-order solver (smrt_second_order_*): it replaces the resident first-order batch ----------
    def second_order_run(self, batch: PackedBatch, extras=None, pairs=None) -> SecondOrderOutput:
        """One shot (H2D, kernels, D2H) for every pair of the batch or the listed ones (row i = pairs[i])."""
        return self._solver_run("second_order", SecondOrderOutput, *self._first_order_pack(batch, extras, pairs))

    def second_order_upload(self, batch: PackedBatch, extras=None, pairs=None):
        """Split form (upload once, launch any number of times, sync, download); see first_order_upload for the lock."""
        self._solver_upload("second_order", *self._first_order_pack(batch, extras, pairs))

    def second_order_launch(self):
        self._solver_call("smrt_second_order_launch")

    def second_order_sync(self):
        self._solver_call("smrt_second_order_sync")

    def second_order_download(self) -> SecondOrderOutput:
        return self._solver_download("second_order", SecondOrderOutput)

    def second_order_kernel_ms(self):
        """HIP-event ms of the first-order kernels and of the order-2 kernels of the last launch."""
        return self._solver_kernel_ms("second_order", 2)

    # ---- the successive-order solver (smrt_successive_order_*) ----------------------------------------------------
    @classmethod
    def _successive_order_pack(cls, batch, n_iteration_max, relative_tolerance, workspace_budget, pairs):
        ptr, count, rows = cls._pair_list(batch, pairs)
        return ((C.byref(batch.struct), int(n_iteration_max), float(relative_tolerance), int(workspace_budget or 0), ptr, count),
                (batch, rows, int(n_iteration_max)))

    def successive_order_run(self, batch: PackedBatch, n_iteration_max=50, relative_tolerance=0.001, pairs=None,
                             workspace_budget=None) -> SuccessiveOrderOutput:
        """One shot (H2D, kernels chunk after chunk, D2H) for every pair of the batch or the listed ones (row i = pairs[i]).
        workspace_budget: bytes everything reserved on the device stays inside (None: the library's default)."""
        return self._solver_run("successive_order", SuccessiveOrderOutput,
                                *self._successive_order_pack(batch, n_iteration_max, relative_tolerance, workspace_budget, pairs))

    def successive_order_upload(self, batch: PackedBatch, n_iteration_max=50, relative_tolerance=0.001, pairs=None,
                                workspace_budget=None):
        """Split form (upload once, launch any number of times, sync, download); see first_order_upload for the lock."""
        self._solver_upload("successive_order",
                            *self._successive_order_pack(batch, n_iteration_max, relative_tolerance, workspace_budget, pairs))

    def successive_order_launch(self):
        self._solver_call("smrt_successive_order_launch")

    def successive_order_sync(self):
        self._solver_call("smrt_successive_order_sync")

    def successive_order_download(self) -> SuccessiveOrderOutput:
        return self._solver_download("successive_order", SuccessiveOrderOutput)

    def successive_order_kernel_ms(self):
        """HIP-event ms of the preparation kernels and of the sweep kernel of the last launch (summed over its chunks)."""
        return self._solver_kernel_ms("successive_order", 2)

    def successive_order_launch_info(self):
        """dict(chunks, reserved_bytes, over_budget, budget) of the last launch."""
        return self._solver_launch_info("successive_order")

    # ---- the successive-order backscatter solver (smrt_so_active_*) -----------------------------------------------
    @classmethod
    def _so_active_pack(cls, batch, n_iteration_max, relative_tolerance, theta_inc, incident_npol, m_max, workspace_budget, pairs):
        ptr, count, rows = cls._pair_list(batch, pairs)
        theta_inc = np.ascontiguousarray(np.atleast_1d(theta_inc), dtype=np.float64)
        return ((C.byref(batch.struct), int(n_iteration_max), float(relative_tolerance), len(theta_inc), _dptr(theta_inc),
                 int(incident_npol), int(m_max), int(workspace_budget or 0), ptr, count),
                (batch, rows, int(n_iteration_max), len(theta_inc), int(m_max)))

    def so_active_run(self, batch: PackedBatch, theta_inc, n_iteration_max=50, relative_tolerance=0.001, incident_npol=2, m_max=2,
                      pairs=None, workspace_budget=None) -> SuccessiveOrderActiveOutput:
        """One shot (H2D, kernels chunk after chunk, D2H) for every pair of the (active) batch or the listed ones (row i =
        pairs[i]).  theta_inc: incidence angles (rad); workspace_budget: bytes everything reserved on the device stays inside."""
        return self._solver_run("so_active", SuccessiveOrderActiveOutput,
                                *self._so_active_pack(batch, n_iteration_max, relative_tolerance, theta_inc, incident_npol, m_max,
                                                      workspace_budget, pairs))

    def so_active_upload(self, batch: PackedBatch, theta_inc, n_iteration_max=50, relative_tolerance=0.001, incident_npol=2, m_max=2,
                         pairs=None, workspace_budget=None):
        """Split form (upload once, launch any number of times, sync, download); see first_order_upload for the lock."""
        self._solver_upload("so_active", *self._so_active_pack(batch, n_iteration_max, relative_tolerance, theta_inc, incident_npol,
                                                               m_max, workspace_budget, pairs))

    def so_active_launch(self):
        self._solver_call("smrt_so_active_launch")

    def so_active_sync(self):
        self._solver_call("smrt_so_active_sync")

    def so_active_download(self) -> SuccessiveOrderActiveOutput:
        return self._solver_download("so_active", SuccessiveOrderActiveOutput)

    def so_active_kernel_ms(self):
        """HIP-event ms of the preparation kernels, the sweep kernel and the combine kernel of the last launch."""
        return self._solver_kernel_ms("so_active", 3)

    def so_active_launch_info(self):
        """dict(chunks, reserved_bytes, over_budget, budget) of the last launch."""
        return self._solver_launch_info("so_active")

    # ---- the multi-Fresnel thermal emission solver (smrt_multifresnel_*) -------------------------------------------
    @classmethod
    def _multifresnel_pack(cls, batch, mu, prune_deep_snowpack, pairs):
        mu = np.ascontiguousarray(np.atleast_1d(mu), dtype=np.float64)
        if len(mu) != int(batch.struct.n_theta):
            raise SMRTError("one sensor cosine per angle of the batch is needed")
        ptr, count, rows = cls._pair_list(batch, pairs)
        none = prune_deep_snowpack is None
        return ((C.byref(batch.struct), _dptr(mu), 0.0 if none else float(prune_deep_snowpack), 1 if none else 0, ptr, count),
                (batch, rows, mu))

    def multifresnel_run(self, batch: PackedBatch, mu, prune_deep_snowpack=10, pairs=None) -> MultiFresnelOutput:
        """One shot (H2D, two kernels, D2H) for every pair of the batch or the listed ones (row i = pairs[i]).  mu: the
        cosines of the sensor's angles; prune_deep_snowpack: an optical depth, or None for no pruning."""
        return self._solver_run("multifresnel", MultiFresnelOutput, *self._multifresnel_pack(batch, mu, prune_deep_snowpack, pairs))

    def multifresnel_upload(self, batch: PackedBatch, mu, prune_deep_snowpack=10, pairs=None):
        """Split form (upload once, launch any number of times, sync, download); see first_order_upload for the lock."""
        self._solver_upload("multifresnel", *self._multifresnel_pack(batch, mu, prune_deep_snowpack, pairs))

    def multifresnel_launch(self):
        self._solver_call("smrt_multifresnel_launch")

    def multifresnel_sync(self):
        self._solver_call("smrt_multifresnel_sync")

    def multifresnel_download(self) -> MultiFresnelOutput:
        return self._solver_download("multifresnel", MultiFresnelOutput)

    def multifresnel_kernel_ms(self):
        """HIP-event ms of the (pair, layer) kernel and of the (pair, angle) kernel of the last launch."""
        return self._solver_kernel_ms("multifresnel", 2)

    # ---- the nadir LRM altimetry solver (smrt_lrm_*) ----------------------------------------------------------------
    @classmethod
    def _lrm_pack(cls, batch, params, pairs):
        ptr, count, rows = cls._pair_list(batch, pairs)
        return (C.byref(batch.struct), C.byref(params.struct), ptr, count), (batch, params, rows)

    def lrm_run(self, batch: PackedBatch, params, pairs=None) -> LrmOutput:
        """One shot (H2D, three kernels, D2H) for every pair of the batch or the listed ones (row i = pairs[i])."""
        return self._solver_run("lrm", LrmOutput, *self._lrm_pack(batch, params, pairs))

    def lrm_upload(self, batch: PackedBatch, params, pairs=None):
        """Split form (upload once, launch any number of times, sync, download); see first_order_upload for the lock."""
        self._solver_upload("lrm", *self._lrm_pack(batch, params, pairs))

    def lrm_layers(self, batch: PackedBatch, params):
        """The layer scalars [n_pairs, Lmax, 5] of the batch alone: an upload and the (pair, layer) kernel, nothing else."""
        a = np.empty((batch.n_pairs, int(batch.struct.n_layers_max), 5))
        with self.lock:
            self.lrm_upload(batch, params)
            self._solver_call("smrt_lrm_layers", _dptr(a))
        return a

    def lrm_launch(self):
        self._solver_call("smrt_lrm_launch")

    def lrm_sync(self):
        self._solver_call("smrt_lrm_sync")

    def lrm_download(self) -> LrmOutput:
        return self._solver_download("lrm", LrmOutput)

    def lrm_kernel_ms(self):
        """HIP-event ms of the three kernels of the last launch: layer scalars, vertical distribution, waveform."""
        return self._solver_kernel_ms("lrm", 3)

    # ---- the nadir SAR altimetry solver (smrt_sar_*) ----------------------------------------------------------------
    def sar_run(self, batch: PackedBatch, params, pairs=None) -> SarOutput:
        """One shot (H2D, four kernels, D2H) for every pair of the batch or the listed ones (row i = pairs[i])."""
        return self._solver_run("sar", SarOutput, *self._lrm_pack(batch, params, pairs))

    def sar_upload(self, batch: PackedBatch, params, pairs=None):
        """Split form (upload once, launch any number of times, sync, download); see first_order_upload for the lock."""
        self._solver_upload("sar", *self._lrm_pack(batch, params, pairs))

    def sar_launch(self):
        self._solver_call("smrt_sar_launch")

    def sar_sync(self):
        self._solver_call("smrt_sar_sync")

    def sar_download(self) -> SarOutput:
        return self._solver_download("sar", SarOutput)

    def sar_kernel_ms(self):
        """HIP-event ms of the four kernels of the last launch: layer scalars, vertical distribution and echoes, tables, map."""
        return self._solver_kernel_ms("sar", 4)

    def ft_even_phase(self, emmodel, microstructure, frequency, frac_volume, temperature, p1, p2, mu_s, mu_i, m_max, npol):
        """Azimuthal modes of the phase matrix of one layer: array [npol, npol, m_max + 1, len(mu_s), len(mu_i)]."""
        mu_s = np.ascontiguousarray(np.atleast_1d(mu_s), dtype=np.float64)
        mu_i = np.ascontiguousarray(np.atleast_1d(mu_i), dtype=np.float64)
        out = np.empty((npol, npol, m_max + 1, len(mu_s), len(mu_i)))
        with self.lock:
            self._check(self._lib.smrt_dort_ft_even_phase(
                self._h, EM_CODES[emmodel], MS_CODES[microstructure], float(frequency), float(frac_volume), float(temperature),
                float(p1), float(p2), _dptr(mu_s), len(mu_s), _dptr(mu_i), len(mu_i), int(m_max), int(npol), _dptr(out)),
                "smrt_dort_ft_even_phase")
        return out

    # ---- rough boundaries evaluated on the device (smrt_batch.rough_kind) ------------------------------------------------
    rough_on_device = True                 # DORT packs rough_kind / rough_params for a context that says so

    @property
    def rough_workspace_budget(self):
        """Bytes of rough matrices one launch may build; DORT splits a group beyond it.  Half of what the device has free for
        them (the solve's own workspace takes its share of the rest), 4 GiB at the most."""
        v = (C.c_double * 6)()
        self._lib.smrt_dort_rough_info(self._h, v, 6)
        return min(4 << 30, int(0.5 * v[5]))

    def rough_matrices(self, batch: PackedBatch) -> RoughMatrices:
        """The builder alone on every pair of the batch, its matrices copied back (smrt_dort_rough_matrices)."""
        o = RoughMatrices(batch)
        with self.lock:
            rc = self._lib.smrt_dort_rough_matrices(self._h, C.byref(batch.struct), *o.pointers())
            self._check(0 if rc >= 0 else -1, "smrt_dort_rough_matrices")
        return o

    def rough_info(self):
        """Of the last upload: slots, the builder kernels' HIP-event time (ms), bytes of rough matrices built on the device,
        bytes of rough matrices copied from the host (smrt_dort_rough_info); m_max_limit: the capability."""
        v = (C.c_double * 5)()
        self._lib.smrt_dort_rough_info(self._h, v, 5)
        return dict(m_max_limit=int(v[0]), slots=int(v[1]), builder_ms=float(v[2]), built_bytes=int(v[3]), host_matrix_bytes=int(v[4]))

    def pair_cost(self):
        """Sum of N_l^3 per pair of the uploaded batch (before solving it): what the work is sharded by."""
        _, pair_count = self._resident
        cost = np.empty(pair_count)
        self._check(self._lib.smrt_dort_pair_cost(self._h, _dptr(cost)), "smrt_dort_pair_cost")
        return cost

    # ---- multi-GPU: the RCCL gather of the C ABI (smrt_dort_comm_*, smrt_dort_gather) ----------------------------
    PIPELINES = ("fused", "lds_two_slot", "lds_four_slot", "lds_reg", "fused_gmem", "gmem", "big", "gmem_strip", "lds_strip")   # SMRT_PIPELINE_*

    def launch_info(self):
        """smrt_dort_launch_info as a dict: pipeline (name), chunk_pairs, chunks, prune_rounds, staged_items (None when
        unknown), block_threads, n_max, diagonalisation (name), rayleigh_closed_form (bool), prep (name), class_lists (bool: the
        launches per size class run over item lists), class_list_items (None without lists), class_list_misses (always 0)."""
        v = (C.c_int64 * 16)()
        n = self._lib.smrt_dort_launch_info(self._h, v, 16)
        self._check(0 if n > 0 else -1, "smrt_dort_launch_info")
        keys = ("pipeline", "chunk_pairs", "chunks", "prune_rounds", "staged_items", "block_threads", "n_max", "diagonalisation",
                "rayleigh_closed_form", "prep", "class_lists", "class_list_items", "class_list_misses")
        d = {k: int(v[i]) for i, k in enumerate(keys[:n])}
        d["pipeline"] = self.PIPELINES[d["pipeline"]]
        d["diagonalisation"] = self.DIAGONALISATIONS[d["diagonalisation"]]
        d["rayleigh_closed_form"] = bool(d.get("rayleigh_closed_form", 0))
        d["prep"] = self.PREPS[d.get("prep", 0)]
        d["class_lists"] = bool(d.get("class_lists", 0))
        if d.get("class_list_items", -1) < 0:
            d["class_list_items"] = None
        if d.get("staged_items", -1) < 0:
            d["staged_items"] = None
        return d

    @staticmethod
    def comm_library():
        """(path of the RCCL library the gather runs on, its version string) -- smrt_dort_comm_library; SMRT_RCCL_LIB
        pins it."""
        lib = load_library()
        buf, version = C.create_string_buffer(1024), C.c_int32(0)
        if lib.smrt_dort_comm_library(buf, len(buf), C.byref(version)) != 0:
            raise SMRTError("RCCL is not available: " + buf.value.decode(errors="replace"))
        v = int(version.value)
        return buf.value.decode(), "%d.%d.%d" % (v // 10000, v // 100 % 100, v % 100) if v >= 10000 else str(v)

    @staticmethod
    def comm_unique_id():
        lib = load_library()
        buf = C.create_string_buffer(128)
        if lib.smrt_dort_comm_unique_id(buf) != 0:
            raise SMRTError("smrt_dort_comm_unique_id failed (is librccl available?)")
        return buf.raw

    def comm_init(self, world, rank, unique_id):
        self._check(self._lib.smrt_dort_comm_init(self._h, int(world), int(rank), bytes(unique_id)), "smrt_dort_comm_init")
        self.world, self.rank = int(world), int(rank)

    @staticmethod
    def comm_init_all(contexts):
        lib = load_library()
        arr = (C.c_void_p * len(contexts))(*[c._h for c in contexts])
        if lib.smrt_dort_comm_init_all(arr, len(contexts)) != 0:
            raise SMRTError("smrt_dort_comm_init_all failed: " + lib.smrt_dort_last_error(contexts[0]._h).decode())
        for r, c in enumerate(contexts):
            c.world, c.rank = len(contexts), r

    def gather(self, counts, root=0, want_host=True):
        """Collective: rows of the last launch of every rank -> root (rank order).  Returns (values, status) on the
        root (None, None elsewhere, or when want_host is False: the rows then stay on the root's device)."""
        batch, _ = self._resident
        counts = np.ascontiguousarray(counts, dtype=np.int64)
        is_root = self.rank == root and want_host
        total = int(counts.sum())
        values = np.empty((total,) + batch.out_shape()) if is_root else None
        status = np.empty(total, np.int32) if is_root else None
        self._check(self._lib.smrt_dort_gather(self._h, int(root), counts.ctypes.data_as(C.POINTER(C.c_int64)),
                                               _dptr(values) if is_root else None,
                                               status.ctypes.data_as(C.POINTER(C.c_int32)) if is_root else None),
                    "smrt_dort_gather")
        return values, status

    def allreduce_max(self, values):
        a = np.ascontiguousarray(np.atleast_1d(values), dtype=np.float64).copy()
        self._check(self._lib.smrt_dort_comm_allreduce_max(self._h, _dptr(a), len(a)), "smrt_dort_comm_allreduce_max")
        return a

    def barrier(self):
        self._check(self._lib.smrt_dort_comm_allreduce_max(self._h, None, 0), "smrt_dort_comm_allreduce_max")

    def last_kernel_ms(self):
        return float(self._lib.smrt_dort_last_kernel_ms(self._h))

    def total_kernel_ms(self, reset=False):
        n = C.c_int64()
        ms = float(self._lib.smrt_dort_total_kernel_ms(self._h, C.byref(n), 1 if reset else 0))
        return ms, int(n.value)

    STAGE_NAMES = ["setup", "assemble", "cholesky", "LtL", "jacobi", "triangular", "R1", "LU1", "R45", "LU2", "R78",
                   "out"]

    def kernel_breakdown(self, enable=None):
        """Per-kernel HIP-event times: kernel_breakdown(True) instruments the following launches, kernel_breakdown() returns
        {"prep", "jacobi", "finish"} in ms for the last launch ("jacobi": the diagonalisation stage, whichever kernels run
        it -- include/smrt_dort.h)."""
        if enable is not None:
            self._check(min(self._lib.smrt_dort_kernel_breakdown(self._h, 1 if enable else 0, None), 0), "smrt_dort_kernel_breakdown")
            return None
        a = np.zeros(3)
        n = self._lib.smrt_dort_kernel_breakdown(self._h, -1, _dptr(a))   # read only: the instrumentation stays as it is
        self._check(min(n, 0), "smrt_dort_kernel_breakdown")
        return {"prep": float(a[0]), "jacobi": float(a[1]), "finish": float(a[2]), "intervals": int(n)}

    def stage_cycles(self):
        a = np.zeros(16)
        self._check(self._lib.smrt_dort_stage_cycles(self._h, _dptr(a)), "smrt_dort_stage_cycles")
        d = dict(zip(self.STAGE_NAMES, a[: len(self.STAGE_NAMES)]))
        d["_jacobi_sweeps"] = a[12]
        d["_gj_panel"], d["_gj_update"], d["_gj_perm"] = a[13], a[14], a[15]
        return d

    def sum_n3(self):
        return float(self._lib.smrt_dort_sum_n3(self._h))


class GatherOp(C.Structure):
    """smrt_gather_op of include/smrt_dort.h."""
    _fields_ = [("peer", C.c_int32), ("reserved", C.c_int32), ("offset_rows", C.c_int64), ("rows", C.c_int64)]


def gather_plan(world, root, rank, counts):
    """The transfers smrt_dort_gather issues on `rank` (smrt_dort_gather_plan: host arithmetic, needs no GPU):
    ([(peer, offset_rows, rows), ...], own_offset_rows, total_rows)."""
    lib = load_library()
    counts = np.ascontiguousarray(counts, dtype=np.int64)
    ops = (GatherOp * max(int(world), 1))()
    own, total = C.c_int64(0), C.c_int64(0)
    n = lib.smrt_dort_gather_plan(int(world), int(root), int(rank), counts.ctypes.data_as(C.POINTER(C.c_int64)),
                                  C.cast(ops, C.c_void_p), int(world), C.byref(own), C.byref(total))
    if n < 0:
        raise SMRTError("smrt_dort_gather_plan: invalid arguments")
    return [(o.peer, o.offset_rows, o.rows) for o in ops[:n]], own.value, total.value


def device_count():
    """Number of visible GPUs (smrt_dort_device_count); 0 when there is none."""
    return int(load_library().smrt_dort_device_count())


def gauss_legendre_positive(n):
    lib = load_library()
    mu = np.empty(n)
    w = np.empty(n)
    lib.smrt_gauss_legendre_positive(n, _dptr(mu), _dptr(w))
    return mu, w
