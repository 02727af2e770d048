"""Base class of the substrates (smrt/core/interface.py:86-166): a temperature and a permittivity model that is a
constant, a callable of (frequency[, temperature]), or a soil / bedrock model of smrt_amd.permittivity that names the
attributes of the substrate it needs (`required_arguments`: temperature, moisture, sand, clay, dry_matter)."""
import numpy as np

from .error import SMRTError

SOIL_ARGUMENTS = ("moisture", "sand", "clay", "dry_matter")

# substrates the device evaluates in passive mode only: Fresnel times a roughness factor per polarisation
# (include/smrt_dort.h: SMRT_SUBSTRATE_SOIL_WEGMULLER, _SOIL_QNH, _ROUGH_CHOUDHURY); in active mode they are "host" objects
PASSIVE_DEVICE_KINDS = ("soil_wegmuller", "soil_qnh", "rough_choudhury79")
# rough models DORT evaluates on the device, as interfaces and as substrates (include/smrt_dort.h: SMRT_ROUGH_*)
ROUGH_DEVICE_KINDS = ("geometrical_optics", "geometrical_optics_backscatter", "iem_fung92")


class SubstrateBase:
    device_kind = None

    def __init__(self, temperature=None, permittivity_model=None, **kwargs):
        soil = {k: kwargs.pop(k) for k in SOIL_ARGUMENTS if k in kwargs}
        if kwargs:
            raise SMRTError("unexpected substrate arguments: %s" % sorted(kwargs))
        self.temperature = temperature
        self.permittivity_model = permittivity_model
        for arg, value in soil.items():   # kept on the substrate whether or not the model reads them: never dropped without a word
            setattr(self, arg, value)
        if callable(permittivity_model):
            # a model that declares what it reads: those arguments become attributes (smrt/core/interface.py:111-126)
            soil.setdefault("temperature", temperature)
            for arg in getattr(permittivity_model, "required_arguments", []):
                if soil.get(arg) is None:
                    raise SMRTError(f"Parameter {arg} must be specified")
                setattr(self, arg, soil[arg])
            for arg, default in getattr(permittivity_model, "optional_arguments", {}).items():
                setattr(self, arg, soil.get(arg, default))

    def _model_arguments(self):
        """Names of the attributes the permittivity model is called with, or None: a plain callable / a constant."""
        pm = self.permittivity_model
        if not callable(pm) or not hasattr(pm, "required_arguments"):
            return None
        return list(pm.required_arguments) + list(getattr(pm, "optional_arguments", {}))

    def permittivity(self, frequency):
        pm = self.permittivity_model
        if pm is None:
            return None
        if callable(pm):
            names = self._model_arguments()
            if names is not None:
                return complex(pm(frequency, **{a: getattr(self, a) for a in names}))
            try:
                return pm(frequency, self.temperature)
            except TypeError:
                return pm(frequency)
        return pm

    def __add__(self, other):  # substrate + ... is not defined; snowpack + substrate is (core/snowpack.py)
        raise SMRTError("Attempt to add an incorrect object to a substrate: use snowpack + substrate")


def batch_permittivities(substrates, frequencies):
    """[F][S] complex: the permittivity of every substrate at every frequency.  Substrates that share a soil / bedrock model
    of smrt_amd.permittivity are evaluated together, once per frequency, on the columns of their attributes; any other
    permittivity model is asked per (frequency, substrate)."""
    eps = np.empty((len(frequencies), len(substrates)), complex)
    together = {}
    for s, sub in enumerate(substrates):
        names = sub._model_arguments() if isinstance(sub, SubstrateBase) else None
        if names is None:
            for fi, f in enumerate(frequencies):
                e = sub.permittivity(float(f))
                if e is None:
                    raise SMRTError(f"No permittivity_model have been given to the substrate '{type(sub).__name__}'")
                eps[fi, s] = complex(e)
        else:
            together.setdefault(sub.permittivity_model, []).append(s)
    for pm, members in together.items():
        names = substrates[members[0]]._model_arguments()
        columns = {a: np.array([getattr(substrates[s], a) for s in members], float) for a in names}
        for fi, f in enumerate(frequencies):
            eps[fi, members] = pm(float(f), **columns)
    return eps
