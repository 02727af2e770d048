"""Rough boundaries evaluated on the device, without a device: the builder kernels (smrt_amd/csrc/rough_boundary_kernel.hpp)
compiled for the CPU (tests/hostemu/rough_boundary_host.cpp, under the fiber emulator) against DORT.interface_matrices /
substrate_matrices fed by the NumPy evaluators -- matrix by matrix and mode by mode, with the specular diagonals and the slot
table --, and the host logic around them: packing of rough_kind / rough_params, the fall-backs to the host route, the appended
ABI fields, the refusals, a "nan" boundary outside validity.

Bar of the matrices: largest element difference relative to the largest element of the same matrix.  Measured over the
single-snowpack cases of this file (CASES; profiles/rough_device_parity.txt): 1.311e-14; the bar is 100 times that, 1.311e-12
(libm against the device's math library in exp, erfc and cos, summed over 129 samples), below the 1e-10 beyond which the
end-to-end 1e-8 is no longer implied.

Whole batches (BATCH_CASES: several snowpacks x frequencies, ragged layer counts, up to three boundaries per snowpack, the three
kinds in one build) are held to the same bar -- the largest, go_two_tiles at 17 streams, measures 5.562e-14, 23 times inside it
-- and to an exact structure: slot table, unused slots, rows and columns beyond the stream counts.  Pair windows and pair lists
of the upload (smrt_rough_host_build_pairs) are compared by bytes with the whole build; a refused snowpack among good ones is
held to the same status on both routes, and to nothing built where it carries rough boundaries (device route only: the host
route cannot pack those, see REFUSED_MIDDLE)."""
import ctypes as C
import os
import subprocess
import types
import warnings

import numpy as np
import pytest

from conftest import ROUGH_INTERFACE_MODELS, ROUGH_SUBSTRATE_MODELS, load_golden, snowpack_dict
from smrt_amd import _native, make_interface, make_snowpack, make_soil, sensor_list
from smrt_amd.rtsolver.dort import DORT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_DIR = os.path.join(ROOT, "tests", "hostemu")
HOST_LIB = os.path.join(EMU_DIR, "librough_boundary_host.so")
MEASURED = 1.311e-14
MATRIX_RTOL = 100 * MEASURED
assert MATRIX_RTOL <= 1e-10


class HostRoute:
    """The same interface / substrate object without its device_kind: the dense host route evaluates it."""

    def __init__(self, target):
        self._target = target

    def __getattr__(self, name):
        if name in ("device_kind", "device_params", "_target"):
            raise AttributeError(name)
        return getattr(self._target, name)


def host_library():
    csrc = os.path.join(ROOT, "smrt_amd", "csrc")
    sources = [os.path.join(EMU_DIR, "rough_boundary_host.cpp"), os.path.join(EMU_DIR, "emu_runtime.hpp"),
               os.path.join(ROOT, "include", "smrt_dort.h")]
    sources += [os.path.join(csrc, f) for f in ("rough_boundary_kernel.hpp", "dort_physics.hpp", "dort_layout.hpp", "spmd.hpp",
                                                "dort_host_common.hpp")]
    if not os.path.exists(HOST_LIB) or any(os.path.getmtime(s) > os.path.getmtime(HOST_LIB) for s in sources):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-DSMRT_HOST_EMU", "-I", EMU_DIR, "-o", HOST_LIB,
                               sources[0]], cwd=ROOT)
    lib = C.CDLL(HOST_LIB)
    lib.smrt_rough_host_build.restype = C.c_int32
    lib.smrt_rough_host_build_pairs.restype = C.c_int32
    lib.smrt_rough_host_refusal.restype = C.c_char_p
    return lib


@pytest.fixture(scope="module")
def host_lib():
    return host_library()


def host_build(lib, batch, order=0, window=None, pairs=None):
    """The builder on every pair of the batch, on the window (pair_begin, pair_count) or on the listed pairs: into zeroed
    arrays of the whole batch, the slot table at -1."""
    o = _native.RoughMatrices(batch)
    if window is None and pairs is None:
        rc = lib.smrt_rough_host_build(C.byref(batch.struct), C.c_int32(order), *o.pointers())
    else:
        listed = None if pairs is None else np.ascontiguousarray(pairs, dtype=np.int64)
        begin, count = (0, len(listed)) if window is None else window
        rc = lib.smrt_rough_host_build_pairs(C.byref(batch.struct), C.c_int32(order), C.c_longlong(begin), C.c_longlong(count),
                                             None if listed is None else listed.ctypes.data_as(C.POINTER(C.c_longlong)), *o.pointers())
    assert rc == o.slots
    return o


LAYERS3 = dict(thickness=[0.3, 0.5, 100.0], density=[250.0, 320.0, 400.0], temperature=[258.0, 262.0, 266.0],
               corr_length=[1e-4, 3e-4, 2e-4])
CONTRAST = dict(thickness=[0.2, 0.4, 100.0], density=[850.0, 150.0, 300.0], temperature=[260.0, 262.0, 265.0],
                corr_length=[5e-5, 3e-4, 2e-4])
GO = ("geometrical_optics", dict(mean_square_slope=0.03))
GO_NOSHADOW = ("geometrical_optics", dict(mean_square_slope=0.05, shadow_correction=False))
GOB = ("geometrical_optics_backscatter", dict(mean_square_slope=0.05))
IEM = ("iem_fung92", dict(roughness_rms=0.002, corr_length=0.05))


def sensor_of(mode, frequency=36.5e9):
    return sensor_list.active(frequency, 40.0) if mode == "A" else sensor_list.passive(frequency, 40.0)


def batch_snowpack(description, wrap=lambda o: o):
    """description: (layers, {interface index: model}, substrate model or None); a substrate model may carry its permittivity
    as a third element (8 + 1j otherwise)."""
    layers, interfaces, soil = description
    itf = ["flat"] * len(layers["thickness"])
    for i, (name, kw) in interfaces.items():
        itf[i] = wrap(make_interface(name, **kw))
    substrate = None if soil is None else wrap(make_soil(soil[0], soil[2] if len(soil) > 2 else complex(8.0, 1.0), 268.0, **soil[1]))
    return make_snowpack(layers["thickness"], "exponential", density=layers["density"], temperature=layers["temperature"],
                         corr_length=layers["corr_length"], interface=itf, substrate=substrate)


def pack_route(ctx, descriptions, mode, frequencies, on_device, **options):
    """The batch of the snowpacks x frequencies through DORT's own packing, on the device route (the objects as they are, a
    context with the capability) or on the host route (the objects behind HostRoute, a context without it)."""
    freqs = np.asarray(frequencies, float)
    wrap = (lambda o: o) if on_device else HostRoute
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        ctx.rough_on_device = on_device
        try:
            batch = DORT(**options)._pack(sensor_of(mode, float(freqs[0])), [batch_snowpack(d, wrap) for d in descriptions], freqs, "iba")
        finally:
            del ctx.rough_on_device          # (back to what the context says of itself)
    if on_device:
        assert batch.struct.rough_kind and not batch.struct.host_interface_slot and batch.struct.substrate_kind != 3
    else:
        assert not batch.struct.rough_kind
    return batch


def pack_batch(ctx, descriptions, mode, frequencies, **options):
    """(batch of the device route, batch of the host route) of the snowpacks x frequencies."""
    return (pack_route(ctx, descriptions, mode, frequencies, True, **options),
            pack_route(ctx, descriptions, mode, frequencies, False, **options))


def layer_permittivities(ctx, descriptions, device):
    """[F][S][Lmax] effective permittivities of the layers of a packed batch, by the probe the host route places its streams
    with (DORT._layer_permittivities), asked here on its own: neither route is touched."""
    cols = np.stack([device.thickness, device.frac_volume, device.temperature, device.micro_p1, device.micro_p2])
    return DORT(n_max_stream=4)._layer_permittivities([batch_snowpack(d) for d in descriptions], device.frequency, cols, device.n_layers,
                                                      "iba", None, None)


def pack_both(ctx, layers, where, model, mode, frequency=36.5e9, **options):
    """(batch of the device route, batch of the host route) of one snowpack through DORT's own packing."""
    description = (layers, {}, model) if where == "substrate" else (layers, {where: model}, None)
    return pack_batch(ctx, [description], mode, [frequency], **options)


def relative_difference(got, expected):
    """Largest element difference relative to the largest element of the same matrix, over the leading dimensions."""
    worst = 0.0
    lead = expected.shape[:-2] if expected.ndim > 2 else expected.shape[:-1]
    for idx in np.ndindex(*lead):
        a, b = got[idx], expected[idx]
        scale = np.abs(b).max()
        if scale == 0.0:
            assert not a.any(), "the device filled a matrix the NumPy evaluator leaves empty"
            continue
        worst = max(worst, float(np.abs(a - b).max() / scale))
    return worst


def compare(built, host, what):
    worst = 0.0
    if built.slots:
        assert np.array_equal(built.slot, host.host_interface_slot), what
        worst = max(worst, relative_difference(built.itf, host.host_interface), relative_difference(built.itf_coh, host.host_interface_coh))
    if built.has_substrate:
        worst = max(worst, relative_difference(built.sub, host.host_substrate), relative_difference(built.sub_coh, host.host_substrate_coh))
    print(f"{what}: largest difference relative to the largest element of the matrix {worst:.3e}")
    assert worst < MATRIX_RTOL, what
    return worst


CASES = {}
for _name, (_model, _kw) in ROUGH_INTERFACE_MODELS.items():
    CASES[_name] = ("fixture", _name, (_model, _kw))
for _name, (_model, _kw) in ROUGH_SUBSTRATE_MODELS.items():
    CASES[_name] = ("fixture_substrate", _name, (_model, _kw))
CASES.update({
    "contrast_go_inner_n12_active": (CONTRAST, 1, GO, "A", dict(n_max_stream=12, m_max=2)),
    "contrast_go_inner_n12_passive": (CONTRAST, 1, GO, "P", dict(n_max_stream=12)),
    "contrast_iem_inner_n12_active": (CONTRAST, 1, IEM, "A", dict(n_max_stream=12, m_max=2)),
    # (two streams in every layer need nearly equal layers; the air then keeps one stream, so the boundary is the substrate)
    "go_substrate_n2": (dict(LAYERS3, density=[300.0, 320.0, 340.0]), "substrate", GO, "A", dict(n_max_stream=2, m_max=2)),
    "go_inner_n33_passive": (LAYERS3, 1, GO, "P", dict(n_max_stream=33)),
    "go_surface_m0": (LAYERS3, 0, GO, "A", dict(n_max_stream=10, m_max=0)),
    "go_inner_m4": (LAYERS3, 2, GO, "A", dict(n_max_stream=10, m_max=_native.ROUGH_M_MAX)),
    "go_substrate_m4": (LAYERS3, "substrate", GO, "A", dict(n_max_stream=10, m_max=_native.ROUGH_M_MAX)),
    "go_noshadow_surface": (LAYERS3, 0, GO_NOSHADOW, "A", dict(n_max_stream=10, m_max=2)),
    "go_noshadow_substrate": (LAYERS3, "substrate", GO_NOSHADOW, "A", dict(n_max_stream=10, m_max=2)),
    "iem_exponential_1": (LAYERS3, 1, ("iem_fung92", dict(roughness_rms=0.002, corr_length=0.05, series_truncation=1)), "A", dict(n_max_stream=10, m_max=2)),
    "iem_exponential_10": (LAYERS3, 0, ("iem_fung92", dict(roughness_rms=0.002, corr_length=0.05, series_truncation=10)), "P", dict(n_max_stream=10)),
    "iem_gaussian_1": (LAYERS3, 0, ("iem_fung92", dict(roughness_rms=0.002, corr_length=0.05, autocorrelation_function="gaussian", series_truncation=1)), "P", dict(n_max_stream=10)),
    "iem_gaussian_10": (LAYERS3, "substrate", ("iem_fung92", dict(roughness_rms=0.003, corr_length=0.04, autocorrelation_function="gaussian", series_truncation=10)), "A", dict(n_max_stream=10, m_max=2)),
    "gob_surface_passive": (LAYERS3, 0, GOB, "P", dict(n_max_stream=10)),
    "gob_inner_active": (LAYERS3, 1, GOB, "A", dict(n_max_stream=10, m_max=2)),
    "gob_substrate_passive": (LAYERS3, "substrate", GOB, "P", dict(n_max_stream=10)),
})


def resolve(case):
    if case[0] in ("fixture", "fixture_substrate"):
        d = load_golden(case[1])
        sp = snowpack_dict(d)
        layers = {k: list(sp[k]) for k in ("thickness", "density", "temperature", "corr_length")}
        act = str(d["mode"]) == "A"
        options = dict(n_max_stream=int(d["opt_n_max_stream"]), **(dict(m_max=int(d["opt_m_max"])) if act else {}))
        where = "substrate" if case[0] == "fixture_substrate" else int(d["rough_interface"][0])
        return layers, where, case[2], "A" if act else "P", options, float(d["frequency"][0])
    return case + (36.5e9,)


@pytest.mark.parametrize("name", sorted(CASES))
def test_device_source_on_the_cpu_against_the_numpy_evaluators(host_lib, emulated, name):
    layers, where, model, mode, options, frequency = resolve(CASES[name])
    device, host = pack_both(emulated, layers, where, model, mode, frequency, **options)
    compare(host_build(host_lib, device), host, name)


# ---- whole batches: several snowpacks x frequencies, ragged layer counts, several boundaries per snowpack ------------------------
# (clearly different densities inside a case: matrices of a swapped pair differ by far more than the bar)
ONE_LAYER = dict(thickness=[100.0], density=[280.0], temperature=[261.0], corr_length=[1.5e-4])
THREE_LAYERS = dict(thickness=[0.25, 0.6, 100.0], density=[220.0, 340.0, 410.0], temperature=[256.0, 260.0, 264.0],
                    corr_length=[8e-5, 2.5e-4, 1.8e-4])
FOUR_LAYERS = dict(thickness=[0.15, 0.3, 0.5, 100.0], density=[200.0, 300.0, 380.0, 450.0], temperature=[254.0, 258.0, 262.0, 266.0],
                   corr_length=[6e-5, 1.2e-4, 2.2e-4, 3e-4])
TWO_LAYERS = dict(thickness=[0.4, 100.0], density=[260.0, 360.0], temperature=[257.0, 263.0], corr_length=[1e-4, 2e-4])
GO_SHADOW = ("geometrical_optics", dict(mean_square_slope=0.05, shadow_correction=True))
# rough_kind [[3,1,0,0,0],[1,0,3,3,0],[0,2,1,3,2],[0,0,1,0,0]]: one, two, three (adjacent) and no rough interface, a substrate each
# (a soil permittivity per snowpack: sub_p1 / sub_p2 [F][S] read at another pair show)
MIXED_RAGGED = [(ONE_LAYER, {0: IEM}, GO + (6.0 + 0.5j,)), (THREE_LAYERS, {0: GO, 2: IEM}, IEM + (8.0 + 1.0j,)),
                (FOUR_LAYERS, {1: GOB, 2: GO, 3: IEM}, GOB + (11.0 + 2.0j,)), (TWO_LAYERS, {}, GO + (15.0 + 3.0j,))]
INTERFACES_ONLY_RAGGED = [(layers, interfaces, None) for layers, interfaces, _ in MIXED_RAGGED]   # snowpack 3: entirely flat
TWO_FREQUENCIES = [13.4e9, 36.5e9]
ACTIVE, PASSIVE = dict(n_max_stream=10, m_max=2), dict(n_max_stream=10)
# name: (snowpack descriptions, mode, frequencies, options of DORT)
BATCH_CASES = {
    "mixed_ragged_active": (MIXED_RAGGED, "A", TWO_FREQUENCIES, ACTIVE),
    "mixed_ragged_passive": (MIXED_RAGGED, "P", TWO_FREQUENCIES, PASSIVE),
    "interfaces_only_ragged_active": (INTERFACES_ONLY_RAGGED, "A", TWO_FREQUENCIES, ACTIVE),   # has_sub = 0: another task stride
    "interfaces_only_ragged_passive": (INTERFACES_ONLY_RAGGED, "P", TWO_FREQUENCIES, PASSIVE),
    # sub_p1[f * S + s] off the diagonal: three frequencies x three snowpacks, a kind each
    "substrates_only_three_kinds": ([(TWO_LAYERS, {}, GO + (6.0 + 0.5j,)), (THREE_LAYERS, {}, GOB + (8.0 + 1.0j,)),
                                     (dict(TWO_LAYERS, density=[310.0, 430.0]), {}, IEM + (11.0 + 2.0j,))], "P", [13.4e9, 18.7e9, 36.5e9], PASSIVE),
    # 17 x 17 = 289 work items per matrix: the second tile of 256 carries 33
    "go_two_tiles": ([(THREE_LAYERS, {0: GO}, None), (TWO_LAYERS, {1: GO}, None)], "P", TWO_FREQUENCIES, dict(n_max_stream=17)),
    # the same snowpack twice, the surfaces apart in shadow_correction alone: the parameter row of the other snowpack shows
    "no_shadow_and_shadow_together": ([(LAYERS3, {0: GO_NOSHADOW}, None), (LAYERS3, {0: GO_SHADOW}, None)], "A", [36.5e9], ACTIVE),
}


def check_structure(built, device, host, layer_eps, what):
    """Exactly, not at a tolerance: the slot table, the slots a snowpack does not use, and the rows and columns beyond the
    stream counts of the two media of every boundary (the streams of DORT._streams_of on layer_eps [F][S][Lmax])."""
    S, Lmax, nmax = int(device.struct.n_snowpacks), int(device.struct.n_layers_max), int(device.struct.n_max_stream)
    kinds, nl = device.rough_kind, device.n_layers
    assert built.slots == max(int(np.count_nonzero(kinds[k, :nl[k]])) for k in range(S)), what
    assert built.has_substrate == all(bool(kinds[k, nl[k]]) for k in range(S)) == any(bool(kinds[k, nl[k]]) for k in range(S)), what
    if built.slots:
        assert built.slot.tobytes() == host.host_interface_slot.tobytes(), what
    for p in range(device.n_pairs):
        f, k = divmod(p, S)
        L = int(nl[k])
        mus, _, air, _ = DORT._streams_of(layer_eps[f, k, :L], nmax)
        n = [len(mu) for mu in mus]
        rough = [l for l in range(L) if kinds[k, l]]
        row = -np.ones(Lmax, np.int32)
        row[rough] = np.arange(len(rough))
        assert np.array_equal(built.slot[p], row if built.slots else -np.ones(Lmax, np.int32)), (what, p)
        assert not built.itf[p, len(rough):].any() and not built.itf_coh[p, len(rough):].any(), (what, p, "a slot the snowpack does not use")
        for j, l in enumerate(rough):
            n_low, n_up = n[l], (n[l - 1] if l > 0 else len(air))
            for m in range(built.itf.shape[2]):
                P = 2 if m == 0 else 3
                for q, (r, c) in enumerate(((n_low, n_low), (n_up, n_low), (n_up, n_up), (n_low, n_up))):
                    M = built.itf[p, j, m, q]
                    assert M[:P * r, :P * c].any(), (what, p, j, m, q, "an empty matrix")
                    assert not M[P * r:].any() and not M[:, P * c:].any(), (what, p, j, m, q, "beyond the streams")
            for q, c in enumerate((n_low, n_low, n_up, n_up)):
                assert not built.itf_coh[p, j, q, 2 * c:].any(), (what, p, j, q, "beyond the streams")
        for m in range(built.sub.shape[1]):
            P, last = (2 if m == 0 else 3), (n[-1] if built.has_substrate else 0)
            assert built.sub[p, m, :P * last, :P * last].any() == built.has_substrate, (what, p, m)
            assert not built.sub[p, m, P * last:].any() and not built.sub[p, m, :, P * last:].any(), (what, p, m, "beyond the streams")
            assert not built.sub_coh[p, m, P * last:].any(), (what, p, m, "beyond the streams")


class SharedBatches:
    """What the tests of ONE module share of the batch cases, made once through the contexts of that module's own tests and
    left unchanged: the packed batches (the NumPy evaluators of the host route take seconds), the layer permittivities (one
    probe for the cases with the same layers and frequencies) and the whole builds of the CPU harness."""

    def __init__(self):
        self.packed, self.eps, self.built = {}, {}, {}

    def case(self, ctx, name):
        """(device-route batch, host-route batch)"""
        if name not in self.packed:
            descriptions, mode, frequencies, options = BATCH_CASES[name]
            self.packed[name] = pack_batch(ctx, descriptions, mode, frequencies, **options)
        return self.packed[name]

    def layer_eps(self, ctx, name):
        descriptions, _, frequencies, _ = BATCH_CASES[name]
        key = (tuple(id(d[0]) for d in descriptions), tuple(frequencies))
        if key not in self.eps:
            self.eps[key] = layer_permittivities(ctx, descriptions, self.case(ctx, name)[0])
        return self.eps[key]

    def whole(self, lib, ctx, name):
        if name not in self.built:
            self.built[name] = host_build(lib, self.case(ctx, name)[0])
        return self.built[name]


@pytest.fixture(scope="module")
def shared():
    return SharedBatches()


@pytest.mark.parametrize("name", sorted(BATCH_CASES))
def test_batches_on_the_cpu_against_the_numpy_evaluators(host_lib, emulated, shared, name):
    device, host = shared.case(emulated, name)
    built = shared.whole(host_lib, emulated, name)
    check_structure(built, device, host, shared.layer_eps(emulated, name), name)
    compare(built, host, name)


# ---- pair windows and pair lists: the workspace by the position in the upload, the outputs by the global pair ---------------------
def matrices_of(built):
    return dict(slot=built.slot, itf=built.itf, itf_coh=built.itf_coh, sub=built.sub, sub_coh=built.sub_coh)


def check_window(whole, part, named, what):
    """By bytes (every element is written by one lane, the hemispherical reduction has a fixed order, the same binary): the
    pairs named are those of the whole build, every other pair is as the caller handed it -- zeros, -1 in the slot table."""
    differing = 0
    for key, full in matrices_of(whole).items():
        got = matrices_of(part)[key]
        for p in range(full.shape[0]):
            if p in named:
                differing += int(np.count_nonzero(got[p] != full[p]))
            else:
                assert np.all(got[p] == (-1 if key == "slot" else 0)), (what, key, p, "a pair outside the upload was written")
    print(f"{what}: {differing} elements of the {len(named)} pairs differ from the whole build; the other pairs are untouched")
    for key, full in matrices_of(whole).items():
        for p in named:
            assert matrices_of(part)[key][p].tobytes() == full[p].tobytes(), (what, key, p, "differs from the whole build")


WINDOWS = {"window_3_4": dict(window=(3, 4)), "window_7_1": dict(window=(7, 1)), "list_6_1_4_3": dict(pairs=[6, 1, 4, 3])}
MIXED_RAGGED_OF = {"A": "mixed_ragged_active", "P": "mixed_ragged_passive"}


@pytest.mark.parametrize("mode", ["A", "P"])
@pytest.mark.parametrize("name", sorted(WINDOWS))
def test_pair_windows_and_lists_build_the_same_bytes_and_nothing_else(host_lib, emulated, shared, name, mode):
    device, whole = shared.case(emulated, MIXED_RAGGED_OF[mode])[0], shared.whole(host_lib, emulated, MIXED_RAGGED_OF[mode])
    assert device.n_pairs == 8
    w = WINDOWS[name]
    part = host_build(host_lib, device, **w)
    named = set(w["pairs"]) if "pairs" in w else set(range(w["window"][0], sum(w["window"])))
    check_window(whole, part, named, f"{name} of mixed_ragged, mode {mode}")


def test_a_pair_list_in_the_reverse_order_of_the_fibers(host_lib, emulated, shared):
    device, whole = shared.case(emulated, "mixed_ragged_active")[0], shared.whole(host_lib, emulated, "mixed_ragged_active")
    part = host_build(host_lib, device, order=1, pairs=[6, 1, 4, 3])
    check_window(whole, part, {6, 1, 4, 3}, "list_6_1_4_3 of mixed_ragged in the reverse order of the fibers")


# ---- one refused pair among good ones ---------------------------------------------------------------------------------------------
# The light layer of CONTRAST keeps 2 of 4 streams and 1 of 3 (NumPy, DORT._streams_of's rule, 13.4 and 36.5 GHz): n_max_stream 3
# is where it drops below two, and the solve refuses the snowpack (status 5).
# REFUSED_MIDDLE, both routes: the refused snowpack is flat and the batch has no substrates, because the host route cannot pack
# a rough boundary on a snowpack with a one-stream layer -- a KNOWN GAP between the routes: DORT._streams_of / _substrates_on_host
# raise IndexError (their weights need two streams) where the device route refuses the pair with status 5.
# REFUSED_ROUGH, device route only: the refused snowpack carries the three kinds and a rough soil -- the builder's own refusal
# (rough_setup_block clears the air's stream count, rough_task returns for every task of the pair).
REFUSED_N_MAX_STREAM = 3
REFUSED_MIDDLE = [(THREE_LAYERS, {0: GO}, None), (CONTRAST, {}, None), (TWO_LAYERS, {1: IEM}, None)]
REFUSED_ROUGH = [(THREE_LAYERS, {0: GO}, GO), (CONTRAST, {0: IEM, 1: GO, 2: GOB}, IEM), (TWO_LAYERS, {1: IEM}, GOB)]


def pairs_of(obj, rows, built):
    """The rows of a RoughMatrices (built) or of a host-route batch, as compare reads them."""
    if built:
        return types.SimpleNamespace(slots=obj.slots, has_substrate=obj.has_substrate, slot=obj.slot[rows], itf=obj.itf[rows],
                                     itf_coh=obj.itf_coh[rows], sub=obj.sub[rows], sub_coh=obj.sub_coh[rows])
    return types.SimpleNamespace(host_interface_slot=obj.host_interface_slot[rows], host_interface=obj.host_interface[rows],
                                 host_interface_coh=obj.host_interface_coh[rows])


def refused_options(mode):
    return dict(n_max_stream=REFUSED_N_MAX_STREAM, **(dict(m_max=2) if mode == "A" else {}))


@pytest.mark.parametrize("mode", ["P", "A"])
def test_one_refused_snowpack_among_good_ones(host_lib, emulated, shared, mode):
    """Both routes refuse the middle snowpack and nothing else, with the same status; the other snowpacks at the bar."""
    device, host = pack_batch(emulated, REFUSED_MIDDLE, mode, TWO_FREQUENCIES, **refused_options(mode))
    if "refused_middle" not in shared.eps:      # (the same in both modes)
        shared.eps["refused_middle"] = layer_permittivities(emulated, REFUSED_MIDDLE, device)
    eps = shared.eps["refused_middle"]

    def streams_kept(star, light, n):   # (the dense layer on top is the most refringent one)
        sines = np.sqrt(1.0 - _native.gauss_legendre_positive(n)[0] ** 2)
        return int(np.count_nonzero(np.sqrt(star / light).real * sines < 1.0))

    for f in range(2):
        counts = [streams_kept(eps[f, 1, 0], eps[f, 1, 1], n) for n in (REFUSED_N_MAX_STREAM, REFUSED_N_MAX_STREAM + 1)]
        assert counts == [1, 2], "the light layer drops below two streams at REFUSED_N_MAX_STREAM"
    status = emulated.run(device).status
    assert np.array_equal(status, emulated.run(host).status)
    assert status.tolist() == [0, 5, 0, 0, 5, 0], "exactly one snowpack is refused, at both frequencies"
    built = host_build(host_lib, device)
    good = [0, 2, 3, 5]
    assert all(built.itf[p].any() for p in good)
    compare(pairs_of(built, good, True), pairs_of(host, good, False), f"refused middle snowpack, mode {mode}, the other snowpacks")


def check_refused_rough(device, status, built, what):
    """The pairs of REFUSED_ROUGH's middle snowpack: refused by the solve, and nothing built for any of its four boundaries.
    The slot row is the snowpack's own table -- rough_setup_block writes it before the stream counts are known, and the solve
    refuses the pair before it reads a slot --, so that is what it must hold, no more."""
    assert device.rough_kind[1].tolist() == [3, 1, 2, 3] and built.slots == 3 and built.has_substrate
    assert status.tolist() == [0, 5, 0, 0, 5, 0], what
    written = 0
    for p in (1, 4):
        written += sum(int(np.count_nonzero(a[p])) for a in (built.itf, built.itf_coh, built.sub, built.sub_coh))
        assert built.slot[p].tolist() == [0, 1, 2], (what, p)
    print(f"{what}: status {status.tolist()}; {written} elements written for the four rough boundaries of the refused pairs")
    for p in (1, 4):
        for key in ("itf", "itf_coh", "sub", "sub_coh"):
            assert not getattr(built, key)[p].any(), (what, key, p, "the builder built a boundary of a refused pair")
    for p in (0, 2, 3, 5):
        assert built.itf[p].any() and built.sub[p].any() and np.isfinite(built.itf[p]).all() and np.isfinite(built.sub[p]).all(), (what, p)


@pytest.mark.parametrize("mode", ["P", "A"])
def test_the_builder_builds_nothing_for_a_refused_pair_with_rough_boundaries(host_lib, emulated, mode):
    device = pack_route(emulated, REFUSED_ROUGH, mode, TWO_FREQUENCIES, True, **refused_options(mode))
    check_refused_rough(device, emulated.run(device).status, host_build(host_lib, device), f"refused rough snowpack, mode {mode}")


def test_strong_contrast_has_rectangular_transmissions_total_reflection_and_impossible_facets(host_lib, emulated):
    layers, where, model, mode, options = CASES["contrast_go_inner_n12_active"]
    device, host = pack_both(emulated, layers, where, model, mode, **options)
    built = host_build(host_lib, device)
    n = lambda M: int(np.count_nonzero(np.abs(M).sum(axis=0))) // 2     # noqa: E731  (streams: non-empty columns of mode 0)
    n_low, n_up = n(built.itf[0, 0, 0, 0]), n(built.itf[0, 0, 0, 2])
    assert n_low < n_up <= 12, "total reflection: the light layer has fewer streams than the dense layer above it"
    ttop, tbot = built.itf[0, 0, 0, 1], built.itf[0, 0, 0, 3]
    # rectangular: the upward transmission of the interface on top of layer 1 is evaluated on the air's cosines (the
    # reference's choice) and cut to the streams of the layer above, the downward one maps n_up streams onto n_low
    assert n(ttop) == n_low and 0 < int(np.count_nonzero(np.abs(ttop).sum(axis=1))) // 2 < n_low
    # (the most oblique streams of the dense layer transmit nothing at all: whole columns of exact zeros)
    assert n_low <= n(tbot) < n_up and int(np.count_nonzero(np.abs(tbot).sum(axis=1))) // 2 == n_low
    # impossible facets: pairs of directions no facet refracts into each other leave exact zeros inside the transmission
    # (r = -1 there: both transmission amplitudes vanish), which the NumPy evaluator leaves as well
    inside = host.host_interface[0, 0, 0, 3][:2 * n_low, :2 * n_up]
    assert (inside == 0.0).any() and np.array_equal(tbot[:2 * n_low, :2 * n_up] == 0.0, inside == 0.0)


def test_two_orders_of_the_fibers_give_identical_bytes(host_lib, emulated):
    for name in ("rough_go_surface_L3_n10_active", "gob_inner_active", "iem_exponential_1"):
        layers, where, model, mode, options, frequency = resolve(CASES[name])
        device, _ = pack_both(emulated, layers, where, model, mode, frequency, **options)
        a, b = host_build(host_lib, device, 0), host_build(host_lib, device, 1)
        for x, y in ((a.slot, b.slot), (a.itf, b.itf), (a.itf_coh, b.itf_coh), (a.sub, b.sub), (a.sub_coh, b.sub_coh)):
            assert x.tobytes() == y.tobytes(), name


# ---- host logic ---------------------------------------------------------------------------------------------------------------
def test_packing_of_rough_kind_and_rough_params(emulated):
    emulated.rough_on_device = True
    solver = DORT(n_max_stream=8, m_max=1)
    iem = make_interface("iem_fung92", roughness_rms=0.002, corr_length=0.05, autocorrelation_function="gaussian", series_truncation=7)
    go = make_interface("geometrical_optics", mean_square_slope=0.04, shadow_correction=False)
    soil = make_soil("geometrical_optics_backscatter", complex(6.0, 0.5), 265.0, mean_square_slope=0.07)
    two = make_snowpack([0.3, 10.0], "exponential", density=[250, 350], temperature=[260, 265], corr_length=[1e-4, 2e-4],
                        interface=[go, "flat"], substrate=soil)
    three = make_snowpack([0.3, 0.4, 10.0], "exponential", density=[250, 300, 350], temperature=[260, 262, 265], corr_length=[1e-4, 2e-4, 2e-4],
                          interface=["flat", iem, go], substrate=soil)
    batch = solver._pack(sensor_of("A"), [two, three], np.array([13e9, 36.5e9]), "iba")
    assert batch.rough_kind.tolist() == [[1, 0, 2, 0], [0, 3, 1, 2]]
    assert batch.rough_params[0, 0].tolist() == [0.04, 0.0, 0.0, 0.0] and batch.rough_params[0, 2].tolist() == [0.07, 1.0, 0.0, 0.0]
    assert batch.rough_params[1, 1].tolist() == [0.002, 0.05, 1.0, 7.0] and batch.rough_params[1, 3].tolist() == [0.07, 1.0, 0.0, 0.0]
    s = batch.struct
    assert s.substrate_kind == 1 and not s.host_interface_slot and not s.host_substrate
    assert np.array_equal(batch.sub_p1, np.full((2, 2), 6.0)) and np.array_equal(batch.sub_p2, np.full((2, 2), 0.5))
    assert emulated.batches == [], "no probe launch: nothing is placed on the host"


@pytest.mark.parametrize("why", ["mixed", "foreign", "coherent_layers", "no_capability"])
def test_fallback_to_the_host_route(emulated, why):
    emulated.rough_on_device = why != "no_capability"
    options = dict(n_max_stream=6, process_coherent_layers=(why == "coherent_layers"))
    go = make_interface("geometrical_optics", mean_square_slope=0.04)
    iem = make_interface("iem_fung92", roughness_rms=0.002, corr_length=0.05)
    packs = [make_snowpack([0.3, 10.0], "exponential", density=[250, 350], temperature=[260, 265], corr_length=[1e-4, 2e-4],
                           interface=[go, "flat"]),
             make_snowpack([0.3, 10.0], "exponential", density=[250, 350], temperature=[260, 265], corr_length=[1e-4, 2e-4],
                           interface=["flat", HostRoute(iem) if why in ("mixed", "foreign") else iem])]
    if why == "foreign":
        packs = packs[1:]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        batch = DORT(**options)._pack(sensor_of("A"), packs, np.array([36.5e9]), "iba")
    assert not batch.struct.rough_kind and batch.struct.host_interface_slot
    assert (batch.host_interface_slot >= 0).sum() == len(packs)


def test_a_group_beyond_the_workspace_budget_is_split_into_launches(emulated):
    """(The emulated kernels ignore rough_kind: the numbers are those of Flat interfaces, the same however the group is cut.)"""
    emulated.rough_on_device = True
    packs = [make_snowpack([0.2 + 0.1 * k, 10.0], "exponential", density=[250, 350], temperature=[260, 265], corr_length=[1e-4, 2e-4],
                           interface=[make_interface("geometrical_optics", mean_square_slope=0.04), "flat"]) for k in range(3)]
    sensors = [sensor_list.passive(f, 40.0) for f in (19e9, 37e9)]
    sims = [(s, p) for s in sensors for p in packs]
    solver = DORT(n_max_stream=4)
    one = solver.solve_batch(sims, "iba")
    assert solver.launches == 1 and len(emulated.batches) == 1
    emulated.rough_workspace_budget = _native.rough_matrix_bytes(2, 1, False, 4, 1)      # one snowpack, two frequencies
    cut = solver.solve_batch(sims, "iba")
    assert solver.launches == 3 and len(emulated.batches) == 4
    assert [b.struct.n_snowpacks for b, _ in emulated.batches[1:]] == [1, 1, 1]
    for a, b in zip(one, cut):
        assert np.array_equal(np.asarray(a.data.values), np.asarray(b.data.values))


def test_appended_fields_against_the_generated_stub(host_lib):
    import sys

    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import gen_ctypes_stub
    finally:
        sys.path.pop(0)
    fields, functions = gen_ctypes_stub.parse(open(gen_ctypes_stub.HEADER).read())
    assert fields[-2:] == [("rough_kind", "C.POINTER(C.c_int32)"), ("rough_params", "C.POINTER(C.c_double)")]
    assert [f for f, _ in fields] == [f for f, _ in _native.SmrtBatch._fields_]
    assert [f for f, _ in _native.SmrtBatch._fields_][-3] == "host_iba_coeff", "appended after the last field, nothing moved"
    names = [f[0] for f in functions]
    assert "smrt_dort_rough_matrices" in names and "smrt_dort_rough_info" in names
    assert {"smrt_dort_rough_matrices", "smrt_dort_rough_info"} <= set(_native.EXPORTED_SYMBOLS)


def test_refusals(host_lib):
    def batch(**kw):
        rough = kw.pop("rough", ([[3, 0, 0]], np.zeros((1, 3, 4))))
        return _native.PackedBatch([2], [0.3, 10.0], [0.3, 0.4], [260.0, 265.0], [1e-4, 2e-4], None, [36.5e9], [0.6], n_max_stream=4,
                                   rough=rough, **kw)

    def refusal(b):
        why = host_lib.smrt_rough_host_refusal(C.byref(b.struct))
        return None if why is None else why.decode()

    assert refusal(batch()) is None
    ne = 12
    itf = (np.full((1, 2), -1), np.zeros((1, 1, 1, 4, ne, ne)), np.zeros((1, 1, 4, ne)))
    assert "cannot be combined with host_interface_slot or SMRT_SUBSTRATE_HOST" in refusal(batch(host_interfaces=itf))
    sub = ("host", np.zeros((1, 1, ne, ne)), np.zeros((1, 1, ne)), [265.0])
    assert "cannot be combined with host_interface_slot or SMRT_SUBSTRATE_HOST" in refusal(batch(substrate=sub))
    assert "unknown rough_kind entry" in refusal(batch(rough=([[4, 0, 0]], np.zeros((1, 3, 4)))))
    assert "cannot be combined with process_coherent_layers" in refusal(batch(process_coherent_layers=True))
    assert "m_max beyond SMRT_ROUGH_M_MAX" in refusal(batch(mode="A", m_max=_native.ROUGH_M_MAX + 1))
    assert refusal(batch(mode="A", m_max=_native.ROUGH_M_MAX)) is None
    assert "needs substrate_kind = SMRT_SUBSTRATE_FLAT" in refusal(batch(rough=([[0, 0, 1]], np.zeros((1, 3, 4)))))
    b = batch()
    b.struct.rough_params = None
    assert "rough_kind needs rough_params" in refusal(b)


def test_nan_boundary_outside_validity(emulated):
    """warning_handling "nan": the pairs at which the surface is outside the model's range come out NaN, the others stay;
    "print" warns and leaves the numbers."""
    emulated.rough_on_device = True
    solver = DORT(n_max_stream=4)
    freqs = np.array([5e9, 89e9])    # k s = 0.5 and 9 at 5 mm rms height: inside, then outside iem_fung92's k s < 3

    def run(handling):
        iem = make_interface("iem_fung92", roughness_rms=0.005, corr_length=0.001, warning_handling=handling)
        sp = make_snowpack([0.3, 10.0], "exponential", density=[250, 350], temperature=[260, 265], corr_length=[1e-4, 2e-4],
                           interface=[iem, "flat"])
        batch = solver._pack(sensor_of("P"), [sp], freqs, "iba")
        out = _native.BatchOutput(batch, 2)
        out.values[...], out.status[...] = 200.0, 0
        out.layers[...] = 0.0
        out.layers[:, :, 0], out.layers[:, :, 1] = 1.5, 1e-4
        solver._rough_validity(batch, out, None, [sp])
        return out.values

    assert np.isfinite(run("nan")[0]).all() and np.isnan(run("nan")[1]).all()
    with pytest.warns(Warning, match="validity"):
        assert np.isfinite(run("print")).all()
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert np.isfinite(run("silent")).all()


def test_identical_indices_across_a_geometrical_optics_interface_raise_as_on_the_host_route(emulated):
    """diffuse_transmission_matrix raises NotImplementedError between layers of identical index; the device route raises the
    same from the permittivities the launch returns, and the rows a launch refused (no permittivity) are left alone."""
    emulated.rough_on_device = True
    solver = DORT(n_max_stream=4)
    go = make_interface("geometrical_optics", mean_square_slope=0.04)
    sp = make_snowpack([0.3, 10.0], "exponential", density=[300, 300], temperature=[260, 260], corr_length=[1e-4, 1e-4],
                       interface=["flat", go])
    batch = solver._pack(sensor_of("A"), [sp], np.array([36.5e9]), "iba")
    out = _native.BatchOutput(batch, 1)
    out.values[...], out.status[...], out.layers[...] = 1.0, 0, 0.0
    out.layers[:, :, 0], out.layers[:, :, 1] = 1.5, 1e-4
    with pytest.raises(NotImplementedError, match="identical index"):
        solver._rough_validity(batch, out, None, [sp])
    with pytest.raises(NotImplementedError, match="identical index"):
        go.diffuse_transmission_matrix(36.5e9, 1.5 + 1e-4j, 1.5 + 1e-4j, np.array([0.5]), np.array([0.5]), np.array([0.0]), 2)
    out.layers[:, 1, 0] = 1.6
    solver._rough_validity(batch, out, None, [sp])
    out.layers[...] = 0.0          # a pair the solve refused: nothing to judge
    out.status[...] = 5
    solver._rough_validity(batch, out, None, [sp])
    assert np.isfinite(out.values).all()


def test_layers_without_a_permittivity_are_not_judged(emulated):
    """A geometrical_optics surface with rms height and correlation length under "nan": rows whose layers came back empty
    (k = 0 would read as outside the range) keep their numbers."""
    emulated.rough_on_device = True
    solver = DORT(n_max_stream=4)
    go = make_interface("geometrical_optics", roughness_rms=0.05, corr_length=0.5, warning_handling="nan")
    sp = make_snowpack([0.3, 10.0], "exponential", density=[250, 350], temperature=[260, 265], corr_length=[1e-4, 2e-4],
                       interface=["flat", go])
    batch = solver._pack(sensor_of("P"), [sp], np.array([36.5e9]), "iba")
    out = _native.BatchOutput(batch, 1)
    out.values[...], out.status[...], out.layers[...] = 200.0, 0, 0.0
    solver._rough_validity(batch, out, None, [sp])
    assert np.isfinite(out.values).all()
    out.layers[:, 0, 0], out.layers[:, 1, 0] = 1.4, 1.6      # k s = 45, k l = 450: inside
    solver._rough_validity(batch, out, None, [sp])
    assert np.isfinite(out.values).all()


from test_solver_refusals_cpu import ALL as OTHER_SOLVERS, refusal  # noqa: E402,F401  (the fixture of the solvers beside DORT)


@pytest.mark.parametrize("solver", OTHER_SOLVERS)
def test_the_solvers_beside_dort_refuse_rough_kind(refusal, solver):  # noqa: F811
    assert refusal(solver) is None
    assert "read by the DORT solver only" in refusal(solver, rough_kind=True, rough_params=True)
    assert "read by the DORT solver only" in refusal(solver, rough_kind=True)
