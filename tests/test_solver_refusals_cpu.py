"""What the six solvers beside DORT refuse before any device work (smrt_amd/csrc/solver_refusals.hpp and the checks
they share in dort_host_common.hpp), compiled with g++ and reached without a GPU (tests/hostemu/solver_refusals_host.cpp):
one valid batch of the smallest shape, broken one field at a time, and the exact message every solver has always answered
with."""
import ctypes as C

import numpy as np
import pytest

from host_build import host_library
from smrt_amd._native import PackedBatch, SmrtBatch

FO, SO2, SO, SOA, MF, LRM = range(6)
NAMES = ["first_order", "second_order", "successive_order", "successive_order_active", "multifresnel", "nadir_lrm_altimetry"]
ALL = (FO, SO2, SO, SOA, MF, LRM)
ACTIVE = (FO, SO2, SOA, LRM)   # (altimetry takes any mode)

DMRT = "the dmrt short-range emmodels are only compatible with sticky_hard_spheres"
SO_HOST = "the successive_order solver has no route for emmodels evaluated on the host"
SOA_HOST = "the successive_order_backscatter solver has no route for emmodels evaluated on the host"
SO2_HOST = "the iterative second-order solver has no route for emmodels evaluated by the caller (SMRT_EM_HOST)"
MF_DEVICE = "the multi-Fresnel thermal emission solver needs emmodels with a device implementation"
FO_SUBSTRATE = "substrate_kind must be none, flat or reflector: any other substrate travels in smrt_first_order_extras"
SOA_RAYLEIGH = "the Rayleigh-family emmodels have azimuth modes 0 to 2 only: m_max must be at most 2"


@pytest.fixture(scope="module")
def refusal():
    fn = host_library("libsmrt_solver_refusals_host.so", "solver_refusals_host.cpp").smrt_emu_solver_refusal
    fn.argtypes = [C.c_int, C.POINTER(SmrtBatch), C.c_int, C.c_double, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                   C.POINTER(C.c_int64), C.c_int64]
    fn.restype = C.c_char_p

    def ask(solver, pairs=None, n_pairs=None, m_max=2, **broken):
        """The solver's answer to the valid batch (1 snowpack, 2 layers, 1 frequency, 1 angle) with the fields of `broken`
        set on the struct: None = a null pointer, True = some non-null pointer (no refusal reads through one), a list = an
        int32 array."""
        b = PackedBatch([2], [0.1, 1.0], [0.3, 0.4], [260.0, 265.0], [1e-4, 2e-4], None, [13e9], [0.6],
                        mode="A" if solver in ACTIVE else "P", n_max_stream=4, m_max=m_max)
        keep = []
        for name, value in broken.items():
            if name == "n_layers0":
                b.n_layers[0] = value
                continue
            ctype = dict(SmrtBatch._fields_)[name]
            if value is None:
                value = ctype()
            elif value is True:
                value = C.cast(b.struct.thickness, ctype)
            elif isinstance(value, list):
                keep.append(np.array(value, dtype=np.int32))
                value = keep[-1].ctypes.data_as(ctype)
            setattr(b.struct, name, value)
        if pairs is not None:
            keep.append(np.array(pairs, dtype=np.int64))
            pairs = keep[-1].ctypes.data_as(C.POINTER(C.c_int64))
        why = fn(solver, C.byref(b.struct), 2, 1e-3, 1, 2, m_max, 8, 2, pairs, -1 if n_pairs is None else n_pairs)
        return None if why is None else why.decode()

    return ask


def same(message, solvers=ALL):
    return {s: message for s in solvers}


# (fields to break, {solver: message}); a solver that is not named takes the batch
CASES = {
    "valid": ({}, {}),
    "empty batch": (dict(n_snowpacks=0), same("empty batch")),
    "wrong mode": (dict(mode=None), {   # (set per solver below: the other mode)
        FO: "the iterative first-order solver needs an active sensor", SO2: "the iterative first-order solver needs an active sensor",
        SO: "the successive_order solver needs a passive sensor", SOA: "the successive_order_backscatter solver needs an active sensor",
        MF: "the multi-Fresnel thermal emission solver needs a passive sensor"}),
    "unknown emmodel": (dict(emmodel=8), same("unknown emmodel")),
    "wrong mode before unknown emmodel": (dict(mode=None, emmodel=8), {
        FO: "the iterative first-order solver needs an active sensor", SO2: "the iterative first-order solver needs an active sensor",
        SO: "the successive_order solver needs a passive sensor", SOA: "the successive_order_backscatter solver needs an active sensor",
        MF: "the multi-Fresnel thermal emission solver needs a passive sensor", LRM: "unknown emmodel"}),
    "unknown microstructure": (dict(microstructure=4), same("unknown microstructure")),
    "null thickness": (dict(thickness=None), same("null input array")),
    "null theta": (dict(theta=None), {FO: "null input array", SO2: "null input array", SO: "null input array",
                                      SOA: "n_theta_inc must be positive", MF: "the sensor cosines are missing"}),
    "sticky hard spheres without micro_p2": (dict(microstructure=1, micro_p2=None), same("stickiness array missing")),
    "layer_kind without micro_p2": (dict(layer_kind=[0, 0], micro_p2=None), same("stickiness array missing")),
    "n_layers 0": (dict(n_layers0=0), same("n_layers out of range")),
    "n_layers above n_layers_max": (dict(n_layers0=3), same("n_layers out of range")),
    "layer_kind microstructure out of range": (dict(layer_kind=[0, 0 + 16 * 4]), same("invalid layer_kind entry")),
    "layer_kind negative": (dict(layer_kind=[-1, 0]), same("invalid layer_kind entry")),
    "layer_kind emmodel out of range": (dict(layer_kind=[0, 9]), {
        FO: "invalid layer_kind entry", SO2: "invalid layer_kind entry", SO: "invalid layer_kind entry", SOA: "invalid layer_kind entry",
        MF: MF_DEVICE}),
    "dmrt with exponential": (dict(emmodel=1), same(DMRT, (FO, SO2, SO, SOA, MF))),
    "dmrt layer with exponential": (dict(layer_kind=[0, 2]), same(DMRT, (FO, SO2, SO, SOA, MF))),
    "first bad layer answers": (dict(layer_kind=[2, 16 * 5]), {**same(DMRT, (FO, SO2, SO, SOA, MF)), LRM: "invalid layer_kind entry"}),
    "host emmodel": (dict(emmodel=4), {FO: "layers evaluated by the caller need host_layer", SO2: SO2_HOST, SO: SO_HOST, SOA: SOA_HOST,
                                       MF: MF_DEVICE}),
    "host emmodel layer": (dict(layer_kind=[0, 4]), {FO: "layers evaluated by the caller need host_layer", SO2: SO2_HOST, SO: SO_HOST,
                                                     SOA: SOA_HOST, MF: MF_DEVICE}),
    "iba_host emmodel": (dict(emmodel=6), {FO: "layers evaluated by the caller need host_layer",
                                           SO2: "layers evaluated by the caller need host_layer", SO: SO_HOST, SOA: SOA_HOST, MF: MF_DEVICE}),
    "iba_host layer with host_layer": (dict(layer_kind=[6, 0], host_layer=True), {
        FO: "layers of kind SMRT_EM_IBA_HOST need host_iba_coeff", SO2: "layers of kind SMRT_EM_IBA_HOST need host_iba_coeff", SO: SO_HOST,
        SOA: SOA_HOST, MF: MF_DEVICE}),
    "rayleigh_host layer before a dmrt layer": (dict(layer_kind=[7, 1]), {
        FO: DMRT, SO2: DMRT, SO: SO_HOST, SOA: SOA_HOST, MF: MF_DEVICE}),
    "host arrays": (dict(host_iba_coeff=True), {MF: MF_DEVICE}),
    "host_phase": (dict(host_phase=True), {MF: MF_DEVICE, LRM: "the nadir LRM altimetry solver has no route for phase matrices evaluated on the host"}),
    "atmosphere": (dict(atm_tb_down=True), {SO: "the successive_order solver can not handle atmosphere yet.",
                                            MF: "the multi-Fresnel thermal emission solver can not handle atmosphere",
                                            LRM: "the nadir LRM altimetry solver can not handle atmosphere"}),
    "process_coherent_layers": (dict(process_coherent_layers=1), {
        SO: "the successive_order solver does not process coherent layers",
        SOA: "the successive_order_backscatter solver does not process coherent layers",
        MF: "process_coherent_layers is not available in the multi-Fresnel thermal emission solver",
        LRM: "process_coherent_layers is not available in the nadir LRM altimetry solver"}),
    "host interfaces": (dict(host_interface_slot=True), {SO: "the successive_order solver takes flat interfaces only",
                                                         SOA: "the successive_order_backscatter solver takes flat interfaces only",
                                                         MF: "the multi-Fresnel thermal emission solver takes Flat interfaces only"}),
    "host substrate": (dict(substrate_kind=3), {
        FO: FO_SUBSTRATE, SO2: FO_SUBSTRATE, SO: "the successive_order solver takes no substrate, a flat one or a reflector",
        SOA: "the successive_order_backscatter solver takes no substrate or a flat one (a reflector has no third Stokes component)",
        MF: "the multi-Fresnel thermal emission solver takes no substrate or a Flat one"}),
    "negative substrate kind": (dict(substrate_kind=-1), {
        FO: FO_SUBSTRATE, SO2: FO_SUBSTRATE, SO: "the successive_order solver takes no substrate, a flat one or a reflector",
        SOA: "the successive_order_backscatter solver takes no substrate or a flat one (a reflector has no third Stokes component)",
        MF: "the multi-Fresnel thermal emission solver takes no substrate or a Flat one"}),
    "reflector": (dict(substrate_kind=2, substrate_p1=True, substrate_p2=True, substrate_temperature=True), {
        SOA: "the successive_order_backscatter solver takes no substrate or a flat one (a reflector has no third Stokes component)",
        MF: "the multi-Fresnel thermal emission solver takes no substrate or a Flat one"}),
    "flat substrate without arrays": (dict(substrate_kind=1), same("substrate arrays missing", (FO, SO2, SO, SOA, MF))),
    "flat substrate without temperature": (dict(substrate_kind=1, substrate_p1=True, substrate_p2=True), {MF: "substrate arrays missing"}),
    "flat substrate": (dict(substrate_kind=1, substrate_p1=True, substrate_p2=True, substrate_temperature=True), {}),
    "n_max_stream 1": (dict(n_max_stream=1), {SO2: "n_max_stream must be 2 to 1024", SO: "the successive_order solver takes 2 to 64 streams",
                                              SOA: "the successive_order_backscatter solver takes 2 to 64 streams"}),
    "own check before the shared ones": (dict(n_max_stream=65, emmodel=8), {
        FO: "unknown emmodel", SO2: "unknown emmodel", SO: "the successive_order solver takes 2 to 64 streams",
        SOA: "the successive_order_backscatter solver takes 2 to 64 streams", MF: "unknown emmodel", LRM: "unknown emmodel"}),
}


@pytest.mark.parametrize("solver", ALL, ids=NAMES)
def test_every_solver_refuses_a_broken_batch_with_its_own_message(refusal, solver):
    for name, (broken, expected) in CASES.items():
        if "mode" in broken:
            broken = dict(broken, mode=0 if solver in ACTIVE else 1)
        assert refusal(solver, **broken) == expected.get(solver), (NAMES[solver], name)


def test_dmrt_with_more_than_three_azimuth_modes_is_refused_by_the_backscatter_solver(refusal):
    assert refusal(SOA, m_max=3, emmodel=1, microstructure=1) == SOA_RAYLEIGH
    assert refusal(SOA, m_max=3, emmodel=1) == DMRT   # (the microstructure comes first)
    # layer by layer: the first layer's refusal, whatever is wrong with the next
    assert refusal(SOA, m_max=3, layer_kind=[1 + 16, 16 * 4]) == SOA_RAYLEIGH
    assert refusal(SOA, m_max=3, layer_kind=[16 * 4, 1 + 16]) == "invalid layer_kind entry"
    assert refusal(SOA, m_max=2, layer_kind=[1 + 16, 2 + 16]) is None
    assert refusal(SOA, m_max=65) == "m_max must be 0 to 64"
    assert refusal(SO2, m_max=9) == "m_max must be 1 to 8"
    assert refusal(SO, m_max=-1) == "m_max must be non-negative"


@pytest.mark.parametrize("solver", ALL, ids=NAMES)
def test_every_solver_checks_the_pair_list_after_the_batch(refusal, solver):
    assert refusal(solver, pairs=[0], n_pairs=1) is None
    assert refusal(solver, pairs=[0, 0, 0], n_pairs=3) is None          # (a pair may be listed more than once)
    assert refusal(solver, pairs=[0], n_pairs=0) == "empty pair list"
    assert refusal(solver, pairs=[-1], n_pairs=1) == "pair index out of bounds"
    assert refusal(solver, pairs=[1], n_pairs=1) == "pair index out of bounds"   # S * F = 1
    assert refusal(solver, pairs=[0, 1], n_pairs=2) == "pair index out of bounds"
    assert refusal(solver, pairs=[1], n_pairs=1, emmodel=8) == "unknown emmodel"
