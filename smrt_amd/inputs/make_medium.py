"""make_snowpack / make_snow_layer with the reference's signature (smrt/inputs/make_medium.py:158-314) for dry snow,
Flat interfaces, optional Flat / Reflector substrate and SimpleIsotropicAtmosphere."""
import collections.abc

import numpy as np

from ..core.error import SMRTError
from ..core.globalconstants import FREEZING_POINT
from ..core.layer import Layer
from ..core.snowpack import Snowpack
from ..interface.flat import Flat


def _get(x, i):
    if isinstance(x, str) or x is None or not isinstance(x, (collections.abc.Sequence, np.ndarray)):
        return x
    return x[i]


def _check_size(x, n, name):
    if isinstance(x, (collections.abc.Sequence, np.ndarray)) and not isinstance(x, str) and len(x) != n:
        raise SMRTError(f"The length of '{name}' must be the same as the number of layers ({n}).")


def make_interface(inst_class_or_modulename=None, broadcast=True, **kwargs):
    """An interface object from a name ("flat", "iem_fung92", "geometrical_optics", "geometrical_optics_backscatter" -- or
    any module of a registered plugin package), a class or a ready instance; with sequences among the keyword arguments and
    `broadcast`, one instance per element (smrt/core/interface.py:17-52).  Flat is evaluated on the device (Fresnel per
    stream); every other model is evaluated on the host through the interface protocol."""
    import inspect

    from ..core.plugin import import_class

    if inst_class_or_modulename is None or inst_class_or_modulename == "flat":
        cls = Flat
    elif isinstance(inst_class_or_modulename, str):
        cls = import_class("interface", inst_class_or_modulename)
    elif inspect.isclass(inst_class_or_modulename):
        cls = inst_class_or_modulename
    elif callable(getattr(inst_class_or_modulename, "specular_reflection_matrix", None)) or isinstance(inst_class_or_modulename, Flat):
        return inst_class_or_modulename
    else:
        raise SMRTError("The interface must be either the name of a module in the interface directory of a plugin package, "
                        "a class that implements the interface behavior, or an instance of such a class.")
    if broadcast and kwargs:
        lengths = [len(v) for v in kwargs.values() if isinstance(v, (collections.abc.Sequence, np.ndarray)) and not isinstance(v, str)]
        if lengths:
            return [cls(**{k: _get(v, i) for k, v in kwargs.items()}) for i in range(max(lengths))]
    return cls(**kwargs)


def get_permittivity_function(permittivity_model):
    """The soil or bedrock model of a name `<module>_permittivity_<x>` (smrt_amd.permittivity.<module>, or the same module of
    a registered plugin package); the short names of the reference resolve to their `soil_permittivity_` form with a
    DeprecationWarning (smrt/inputs/make_soil.py:276-300).  Anything that is not a name is returned as it is."""
    import importlib
    import warnings

    from ..core.plugin import _BUILTIN, user_plugin_package

    if not isinstance(permittivity_model, str):
        return permittivity_model
    name = permittivity_model
    if name in ("hut_epss", "dobson85", "dobson85_peplinski95", "montpetit2008"):
        warnings.warn(f"The permittivity model '{name}' should be called with the prefix 'soil_permittivity_'. The new "
                      f"recommended name is 'soil_permittivity_{name}'.", DeprecationWarning, stacklevel=3)
        name = "soil_permittivity_" + name
    if name.count("_permittivity_") != 1:
        raise SMRTError(f"The permittivity model {name} has not a valid name. It must match the pattern "
                        "<modulename>_permittivity_<something>.")
    modulename = name.split("_permittivity_")[0]
    for pkg in user_plugin_package + [_BUILTIN]:
        try:
            function = getattr(importlib.import_module(f"{pkg}.permittivity.{modulename}"), name, None)
        except ImportError:
            continue
        if function is not None:
            if name == "soil_permittivity_dobson85":
                function(None, None, None, None, None)   # refused, with the two names that replace it
            return function
    raise SMRTError(f"Unable to find the permittivity model '{name}'")


def make_soil_substrate(substrate_model, permittivity_model=None, temperature=FREEZING_POINT, moisture=None, sand=None,
                        clay=None, dry_matter=None, **kwargs):
    """A soil or bedrock substrate with the reference's signature (smrt/inputs/make_soil.py:60-111): `substrate_model` by
    name ("flat", "reflector", "soil_wegmuller", "soil_qnh", "rough_choudhury79", "iem_fung92", "geometrical_optics",
    "geometrical_optics_backscatter") or class; `permittivity_model` a number, a callable of (frequency[, temperature]) or
    the name of a model of smrt_amd.permittivity.soil / .bedrock -- by default soil_permittivity_dobson85_peplinski95 --
    which reads moisture, sand, clay, dry_matter and the temperature from the substrate.

    make_soil_column and make_soil_layer are not here: a soil LAYER needs a permittivity model on the layer's side (the
    device computes the layers' electromagnetics itself), which is a piece of work of its own."""
    from ..core.plugin import import_class
    from ..permittivity.soil import soil_permittivity_dobson85_peplinski95

    permittivity_model = get_permittivity_function(permittivity_model)
    if permittivity_model is None:
        permittivity_model = soil_permittivity_dobson85_peplinski95
    cls = import_class("substrate", substrate_model) if isinstance(substrate_model, str) else substrate_model
    soil = dict(moisture=moisture, sand=sand, clay=clay, dry_matter=dry_matter)
    return cls(temperature=temperature, permittivity_model=permittivity_model,
               **{k: v for k, v in soil.items() if v is not None}, **kwargs)


make_soil = make_soil_substrate


def make_snow_layer(layer_thickness, microstructure_model, density, temperature=FREEZING_POINT, **kwargs):
    return Layer(layer_thickness, microstructure_model, density, temperature=temperature, **kwargs)


def make_snowpack(thickness, microstructure_model, density, interface=None, surface=None, substrate=None,
                  atmosphere=None, **kwargs):
    """Build a multi-layered snowpack; every parameter can be an array, a list or a constant."""
    if not isinstance(thickness, collections.abc.Iterable):
        raise SMRTError("The thickness argument must be iterable, that is, a list of numbers, numpy array or pandas "
                        "Series or DataFrame.")
    thickness = list(thickness)
    n = len(thickness)
    _check_size(density, n, "density")
    for k, v in kwargs.items():
        _check_size(v, n, k)
    def as_interface(itf):   # None / a name / a class / an instance (smrt/core/interface.py:17-52)
        return make_interface(itf)

    if isinstance(interface, (list, tuple)):
        _check_size(interface, n, "interface")
        if surface is not None:   # smrt/inputs/make_medium.py:207-210
            raise SMRTError("Setting both 'surface' and 'interface' arguments is ambiguous when interface is a list or any "
                            "sequence: its first element already is the surface.")
    sp = Snowpack(substrate=substrate, atmosphere=atmosphere)
    for i, dz in enumerate(thickness):
        if dz <= 0:
            continue
        layer = make_snow_layer(dz, _get(microstructure_model, i), density=_get(density, i),
                                **{k: _get(v, i) for k, v in kwargs.items()})
        # (one interface per layer, on top of it; `surface` replaces the first one, smrt/inputs/make_medium.py:127-133)
        itf = surface if (surface is not None and sp.nlayer == 0) else (_get(interface, i) if isinstance(interface, (list, tuple)) else interface)
        sp.append(layer, interface=as_interface(itf))
    if sp.nlayer == 0:
        raise SMRTError("a snowpack needs at least one layer with a positive thickness")
    sp.all_interfaces_flat()
    sp.layer_facts()   # the per-layer columns the batching solver stacks, packed once here: a FIRST Model.run on a fresh
    return sp          # ensemble costs what a repeated one does (the caches stand until one of these layers is written to)
