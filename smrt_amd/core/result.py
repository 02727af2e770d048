"""Result / PassiveResult / ActiveResult without xarray: a small labelled n-d array with `sel`, and the accessor
surface of smrt/core/result.py:93-680 (TbV/TbH/Tb(channel=)/sigmaVV.../to_dataframe/other_data) plus
concat_results (:768-817)."""
from collections import OrderedDict

import numpy as np

from ..utils import dB
from .error import SMRTError


class LabeledArray:
    """values + ordered named coordinates; `sel(name=value, ...)` drops the selected dimensions."""

    def __init__(self, values, coords, name=None, attrs=None):
        self.values = np.asarray(values)
        self.coords = OrderedDict((k, np.asarray(v)) for k, v in coords)
        self.name = name
        self.attrs = dict(attrs or {})
        if self.values.shape != tuple(len(v) for v in self.coords.values()):
            raise SMRTError(f"shape {self.values.shape} does not match coords "
                            f"{[(k, len(v)) for k, v in self.coords.items()]}")

    @property
    def dims(self):
        return tuple(self.coords.keys())

    @property
    def shape(self):
        return self.values.shape

    @property
    def size(self):
        return self.values.size

    def __getattr__(self, attr):
        coords = self.__dict__.get("coords", {})
        if attr in coords:
            return coords[attr]
        raise AttributeError(attr)

    def _index(self, dim, value):
        c = self.coords[dim]
        if c.dtype.kind in "fc":
            hit = np.nonzero(np.isclose(c, value, rtol=1e-12, atol=0))[0]
        else:
            hit = np.nonzero(c == value)[0]
        if len(hit) == 0:
            raise KeyError(f"{value!r} not found in dimension '{dim}'")
        return int(hit[0])

    def sel(self, drop=True, **kwargs):
        idx = []
        new_coords = []
        for d in self.dims:
            if d in kwargs and not isinstance(kwargs[d], (list, tuple, np.ndarray)):
                idx.append(self._index(d, kwargs[d]))
            elif d in kwargs:
                ii = [self._index(d, v) for v in kwargs[d]]
                idx.append(ii)
                new_coords.append((d, self.coords[d][ii]))
            else:
                idx.append(slice(None))
                new_coords.append((d, self.coords[d]))
        unknown = set(kwargs) - set(self.dims)
        if unknown:
            raise KeyError(f"unknown dimension(s) {sorted(unknown)}")
        vals = self.values
        for axis in reversed(range(len(idx))):  # apply one axis at a time (no fancy-index broadcasting)
            vals = np.take(vals, idx[axis], axis=axis) if not isinstance(idx[axis], slice) else vals
        return LabeledArray(vals, new_coords, name=self.name, attrs=self.attrs)

    def rename(self, name):
        return LabeledArray(self.values, list(self.coords.items()), name=name, attrs=self.attrs)

    def sum(self, dim):
        """The sum along the dimension `dim`, which is dropped."""
        axis = self.dims.index(dim)
        keep = [(k, v) for k, v in self.coords.items() if k != dim]
        return LabeledArray(self.values.sum(axis=axis), keep, name=self.name, attrs=self.attrs)

    def squeeze(self):
        keep = [(k, v) for k, v in self.coords.items() if len(v) != 1]
        return LabeledArray(self.values.reshape([len(v) for _, v in keep]), keep, name=self.name, attrs=self.attrs)

    def __float__(self):
        return float(self.values.reshape(-1)[0]) if self.size == 1 else float(self.values)

    def __array__(self, dtype=None, copy=None):
        return np.asarray(self.values, dtype=dtype)

    def _binary(self, other, op):
        o = other.values if isinstance(other, LabeledArray) else other
        return LabeledArray(op(self.values, o), list(self.coords.items()), name=self.name, attrs=self.attrs)

    def __getitem__(self, key):
        return self.values[key]

    def __len__(self):
        return len(self.values)

    def __iter__(self):
        return iter(self.values)

    def __sub__(self, o):
        return self._binary(o, np.subtract)

    def __rsub__(self, o):
        return self._binary(o, lambda a, b: np.subtract(b, a))

    def __neg__(self):
        return LabeledArray(-self.values, list(self.coords.items()), name=self.name, attrs=self.attrs)

    def __lt__(self, o):
        return self.values < (o.values if isinstance(o, LabeledArray) else o)

    def __le__(self, o):
        return self.values <= (o.values if isinstance(o, LabeledArray) else o)

    def __gt__(self, o):
        return self.values > (o.values if isinstance(o, LabeledArray) else o)

    def __ge__(self, o):
        return self.values >= (o.values if isinstance(o, LabeledArray) else o)

    def __mul__(self, o):
        return self._binary(o, np.multiply)

    __rmul__ = __mul__

    def __add__(self, o):
        return self._binary(o, np.add)

    __radd__ = __add__

    def __truediv__(self, o):
        return self._binary(o, np.divide)

    def to_dataframe(self, name=None):
        import pandas as pd

        name = name or self.name or "value"
        if not self.dims:
            return pd.DataFrame([float(self.values)], columns=[name])
        index = pd.MultiIndex.from_product(list(self.coords.values()), names=list(self.coords.keys()))
        if len(self.dims) == 1:
            index = pd.Index(list(self.coords.values())[0], name=self.dims[0])
        return pd.DataFrame({name: self.values.reshape(-1)}, index=index)

    def __repr__(self):
        return f"LabeledArray(name={self.name!r}, dims={self.dims}, values=\n{self.values})"


NETCDF_VARIABLE = "__xarray_dataarray_variable__"   # the name xarray gives an unnamed DataArray in DataArray.to_netcdf


EXTRA_VARIABLES = ("z_gate",)   # further variables an AltimetryResult writes next to its data


def save_labeled_array(arr, filename, extra=None):
    """Write a LabeledArray as a netCDF-3 file laid out like xarray's DataArray.to_netcdf (one data variable, one
    coordinate variable per dimension, strings as character arrays, attributes on the data variable), so that the
    reference's `open_result` / `xr.open_dataarray` read it.  scipy.io.netcdf_file is the only dependency."""
    from scipy.io import netcdf_file

    with netcdf_file(filename, "w", version=2) as nc:
        for dim, values in arr.coords.items():
            values = np.asarray(values)
            nc.createDimension(dim, len(values))
            if values.dtype.kind in "US":
                width = max(1, max(len(str(v)) for v in values))
                sdim = "string%d" % width
                if sdim not in nc.dimensions:
                    nc.createDimension(sdim, width)
                var = nc.createVariable(dim, "c", (dim, sdim))
                var[:] = np.array([list(str(v).ljust(width, "\0")) for v in values], dtype="S1")
            else:
                var = nc.createVariable(dim, "d" if values.dtype.kind == "f" else "i", (dim,))
                var[:] = values
        data = nc.createVariable(NETCDF_VARIABLE, "d", tuple(arr.coords.keys()))
        data[:] = np.asarray(arr.values, dtype=np.float64)
        for k, v in arr.attrs.items():
            setattr(data, k, v)
        for name, other in (extra or {}).items():   # on (a subset of) the dimensions of the data
            var = nc.createVariable(name, "d", tuple(other.coords.keys()))
            var[:] = np.asarray(other.values, dtype=np.float64)


def load_labeled_array(filename):
    from scipy.io import netcdf_file

    with netcdf_file(filename, "r", mmap=False) as nc:
        names = [n for n in nc.variables if n not in nc.dimensions and n not in EXTRA_VARIABLES]
        if len(names) != 1:
            raise SMRTError(f"'{filename}' does not hold exactly one data variable")
        var = nc.variables[names[0]]
        coords = []
        for dim in var.dimensions:
            c = nc.variables[dim]
            v = c[:].copy()
            if v.dtype.kind == "S" and v.ndim == 2:
                v = np.array([b"".join(row).rstrip(b"\0").decode() for row in v])
            coords.append((dim, v))
        attrs = {k: (v.decode() if isinstance(v, bytes) else v) for k, v in var._attributes.items()}
        data = LabeledArray(var[:].copy(), coords, attrs=attrs)
        for name in EXTRA_VARIABLES:
            if name in nc.variables:
                v = nc.variables[name]
                data.attrs[name] = LabeledArray(v[:].copy(), [(d, data.coords[d]) for d in v.dimensions], name=name)
        return data


def open_result(filename):
    """Read a result written by `Result.save` (or by the reference's, when it was written in a netCDF-3 format)."""
    data = load_labeled_array(filename)
    mode = data.attrs.get("mode")
    if mode not in ("A", "P"):
        mode = "A" if "theta_inc" in data.coords else "P"
    if data.attrs.get("result") == "altimetry":
        z_gate = data.attrs.pop("z_gate", None)
        return AltimetryResult(data, z_gate=z_gate)
    return (ActiveResult if mode == "A" else PassiveResult)(data)


def _strongsqueeze(x):
    x = x.squeeze()
    return float(x) if x.size == 1 else x


def stack_arrays(arrays, dim_name, dim_values):
    """Stack along a new leading dimension.  Arrays of different extents are laid into the union of their coordinates
    and the holes filled with NaN -- results of snowpacks with different layer counts carry per-layer diagnostics of
    different lengths -- which is what the reference gets from xr.concat(..., join="outer") (smrt/core/result.py:811-815)."""
    first = arrays[0]
    if any(a.dims != first.dims for a in arrays[1:]):
        raise SMRTError("cannot concatenate results with different dimensions")
    axes = []
    for d in first.dims:            # the union of the labels of every axis, in order of first appearance
        labels = list(first.coords[d])
        for a in arrays[1:]:
            if len(a.coords[d]) != len(labels) or not np.array_equal(a.coords[d], first.coords[d]):
                known = set(labels)
                labels += [v for v in a.coords[d] if v not in known]
        axes.append(np.asarray(labels))
    same_grid = all(a.shape == tuple(len(ax) for ax in axes) for a in arrays)
    lead = (dim_name, np.asarray(list(dim_values)))
    if same_grid:
        out = np.stack([a.values for a in arrays], axis=0)
    else:
        dtype = np.result_type(np.float64, *[a.values.dtype for a in arrays])
        out = np.full((len(arrays),) + tuple(len(ax) for ax in axes), np.nan, dtype=dtype)
        for k, a in enumerate(arrays):
            where = tuple(np.array([list(ax).index(v) for v in a.coords[d]], dtype=int) for d, ax in zip(first.dims, axes))
            out[(k,) + np.ix_(*where)] = a.values
    return LabeledArray(out, [lead] + list(zip(first.dims, axes)), name=first.name, attrs=first.attrs)


class Result(object):
    """Contain the results of a/many computations and provide convenience accessors."""

    def __init__(self, radiance, coords=None, channel_map=None, other_data=None, mother_df=None):
        if isinstance(radiance, LabeledArray):
            self.data = radiance
        else:
            self.data = LabeledArray(radiance, coords)
        self.other_data = other_data or {}
        self.mother_df = mother_df
        if not hasattr(self, "mode"):
            raise SMRTError("Result base class is abstract, uses a subclass instead.")
        self.data.attrs["mode"] = self.mode
        self.channel_map = channel_map or dict()

    @property
    def coords(self):
        return self.data.coords

    def __getattr__(self, attr):
        data = self.__dict__.get("data")
        if attr != "data" and data is not None and attr in data.coords:
            return data.coords[attr]
        raise AttributeError(f"'{type(self)}' object has no attribute '{attr}'")

    def save(self, filename, netcdf_engine=None):
        """Save the result to disk as a netCDF file (the data array with its coordinates, like the reference's
        Result.save, smrt/core/result.py:138-147); read it back with `open_result`."""
        save_labeled_array(self.data, filename)

    def sel_data(self, channel=None, **kwargs):
        raise NotImplementedError

    def _selection(self, channel, selection):
        """The keyword selection with the configuration of `channel` (frequency, polarization, ... of the sensor's channel
        map) merged in, restricted to the dimensions this result has."""
        if channel is None:
            return dict(selection)
        if channel not in self.channel_map:
            raise SMRTError(f"unknown channel '{channel}' (the result knows {sorted(self.channel_map)})")
        return {**selection, **{k: v for k, v in self.channel_map[channel].items() if k in self.data.dims}}

    def return_as_dataframe(self, name, channel_axis=None, **kwargs):
        """A pandas view of the result: one column `name` indexed by the remaining dimensions (channel_axis=None), one
        column per channel of the sensor ("column"), or the channels as the innermost index level ("index") --
        smrt/core/result.py:152-216.  Built from the arrays, not by joining per-channel frames."""
        import pandas as pd

        def index_of(arr):
            if not arr.dims:
                return pd.RangeIndex(1)
            if len(arr.dims) == 1:
                return pd.Index(arr.coords[arr.dims[0]], name=arr.dims[0])
            return pd.MultiIndex.from_product([arr.coords[d] for d in arr.dims], names=list(arr.dims))

        if channel_axis is None:
            arr = self.sel_data(**kwargs)
            return pd.DataFrame({name: np.reshape(arr.values, -1)}, index=index_of(arr))
        if channel_axis not in ("column", "index"):
            raise SMRTError('channel_axis argument must be None, "column" or "index"')
        if not self.channel_map:
            raise SMRTError("No channel information is given in the result. Unable to index the result by channel.")
        channels = list(self.channel_map)
        arrays = [self.sel_data(channel=ch, **kwargs) for ch in channels]
        if any(a.dims != arrays[0].dims or a.shape != arrays[0].shape for a in arrays[1:]):
            raise SMRTError("the channels of this result do not share their remaining dimensions")
        table = np.column_stack([np.reshape(a.values, -1) for a in arrays])          # rows: remaining dims, columns: channels
        df = pd.DataFrame(table, index=index_of(arrays[0]), columns=channels)
        if channel_axis == "index":
            long = df.stack()
            long.index = long.index.set_names("channel", level=-1)
            if not arrays[0].dims:      # (the one row of a result without remaining dimensions is not an index level)
                long = long.droplevel(0)
            return long.to_frame(name)
        if self.mother_df is not None:  # one row per snowpack, in the order of the run: the user's columns ride along
            df = df.reset_index(drop=True).join(self.mother_df.reset_index(drop=True))
            df.index = self.mother_df.index
        return df

    def to_series(self, **kwargs):
        return self.return_as_dataframe("out", channel_axis="column", **kwargs).iloc[0]

    def optical_depth(self):
        return (self.other_data["ka"] + self.other_data["ks"]) * self.other_data["thickness"]

    def single_scattering_albedo(self):
        return self.other_data["ks"] / self.other_data["ke"]

    def ks(self):
        return self.other_data["ks"]

    def ka(self):
        return self.other_data["ka"]


class PassiveResult(Result):
    mode = "P"

    def sel_data(self, channel=None, **kwargs):
        return self.data.sel(**self._selection(channel, kwargs))

    def Tb(self, channel=None, **kwargs):
        """Brightness temperature; slice with e.g. frequency=37e9, polarization='V' or channel='37V'."""
        return _strongsqueeze(self.sel_data(channel=channel, **kwargs).rename("Tb"))

    def TbV(self, **kwargs):
        return _strongsqueeze(self.data.sel(polarization="V", **kwargs).rename("TbV"))

    def TbH(self, **kwargs):
        return _strongsqueeze(self.data.sel(polarization="H", **kwargs).rename("TbH"))

    def polarization_ratio(self, ratio="H_V", **kwargs):
        return _strongsqueeze(self.data.sel(polarization=ratio[0], **kwargs)
                              / self.data.sel(polarization=ratio[-1], **kwargs))

    def to_dataframe(self, channel_axis="auto", **kwargs):
        if channel_axis == "auto":
            channel_axis = "column" if self.channel_map else None
        return super().return_as_dataframe(name="Tb", channel_axis=channel_axis, **kwargs)

    def Tb_as_dataframe(self, channel_axis=None, **kwargs):
        return self.to_dataframe(channel_axis=None, **kwargs)

    def __repr__(self):
        return f"PassiveResult: TbV={self.TbV()}, TbH={self.TbH()}"


class ActiveResult(Result):
    mode = "A"

    def sel_data(self, channel=None, return_backscatter=False, **kwargs):
        """The selected intensities, or -- return_backscatter="natural" | "dB" -- the backscattering coefficient
        sigma0 = 4 pi cos(theta) I of the selected incidence angles (smrt/core/result.py:430-486)."""
        selection = self._selection(channel, kwargs)
        if not return_backscatter:
            return self.data.sel(**selection)
        angles = [selection.pop(k) for k in ("theta", "theta_inc") if k in selection]
        angles = [a for a in angles if a is not None]
        if len(angles) == 2 and not np.array_equal(np.atleast_1d(angles[0]), np.atleast_1d(angles[1])):
            raise SMRTError("theta and theta_inc must be the same when returning backscatter")
        theta = angles[0] if angles else self.data.coords["theta_inc"]
        several = np.ndim(theta) > 0
        picked = self.data.sel(theta_inc=list(np.atleast_1d(theta)) if several else theta, **selection)
        cos_theta = np.cos(np.deg2rad(np.asarray(theta, float)))
        if several:                 # broadcast along the theta_inc axis that stayed
            shape = [1] * len(picked.dims)
            shape[picked.dims.index("theta_inc")] = -1
            cos_theta = cos_theta.reshape(shape)
        sigma0 = picked * (4 * np.pi * cos_theta)
        if return_backscatter == "dB":
            return LabeledArray(dB(sigma0.values), list(sigma0.coords.items()), name=sigma0.name, attrs=sigma0.attrs)
        return sigma0

    def sigma(self, channel=None, name="sigma", **kwargs):
        return _strongsqueeze(self.sel_data(channel=channel, return_backscatter="natural", **kwargs).rename(name))

    def sigma_dB(self, name="sigma_dB", channel=None, **kwargs):
        return _strongsqueeze(self.sel_data(channel=channel, return_backscatter="dB", **kwargs).rename(name))

    def to_dataframe(self, channel_axis=None, **kwargs):
        if channel_axis == "auto":
            channel_axis = "column" if self.channel_map else None
        return super().return_as_dataframe(name="sigma", channel_axis=channel_axis, return_backscatter="dB", **kwargs)

    def sigmaVV(self, name="sigmaVV", **kwargs):
        return self.sigma(polarization_inc="V", polarization="V", name=name, **kwargs)

    def sigmaHH(self, name="sigmaHH", **kwargs):
        return self.sigma(polarization_inc="H", polarization="H", name=name, **kwargs)

    def sigmaHV(self, name="sigmaHV", **kwargs):
        return self.sigma(polarization_inc="H", polarization="V", name=name, **kwargs)

    def sigmaVH(self, name="sigmaVH", **kwargs):
        return self.sigma(polarization_inc="V", polarization="H", name=name, **kwargs)

    def sigmaVV_dB(self, name="sigmaVV_dB", **kwargs):
        return dB(self.sigmaVV(name=name, **kwargs))

    def sigmaHH_dB(self, name="sigmaHH_dB", **kwargs):
        return dB(self.sigmaHH(name=name, **kwargs))

    def sigmaHV_dB(self, name="sigmaHV_dB", **kwargs):
        return dB(self.sigmaHV(name=name, **kwargs))

    def sigmaVH_dB(self, name="sigmaVH_dB", **kwargs):
        return dB(self.sigmaVH(name=name, **kwargs))

    def __repr__(self):
        return (f"ActiveResult:sigmaVV={self.sigmaVV_dB()} dB, sigmaHH={self.sigmaHH_dB()} dB, "
                f"sigmaHV={self.sigmaHV_dB()} dB")


class AltimetryResult(ActiveResult):
    """The waveform of an altimeter (smrt/core/result.py: AltimetryResult): dimensions (delay, theta_inc, theta), `contribution`
    in front with return_contributions.  `gate` is the gate number of every delay, `z_gate` the depth of every gate in the
    snowpack (NaN below it), with the batch dimensions of the result in front.  A SAR altimeter's result is a delay-Doppler map:
    the dimension `doppler_frequency` follows `delay`, `doppler_bin` is the Doppler beam number of every frequency, and
    `waveform()` is the sum over the Doppler frequencies."""

    def __init__(self, *args, z_gate=None, **kwargs):
        super().__init__(*args, **kwargs)
        self.data.attrs["result"] = "altimetry"
        if z_gate is not None:
            self.z_gate = z_gate

    @property
    def gate(self):
        a = self.data.attrs
        return self.data.coords["delay"] * a["pulse_bandwidth"] + a["nominal_gate"]

    @property
    def doppler_bin(self):
        a = self.data.attrs
        return self.data.coords["doppler_frequency"] / a["pulse_repetition_frequency"] * a["ndoppler"]

    def save(self, filename, netcdf_engine=None):
        z_gate = self.__dict__.get("z_gate")
        save_labeled_array(self.data, filename, extra={"z_gate": z_gate} if z_gate is not None else None)

    def delay_doppler_map(self, name="delay_doppler_map", **kwargs):
        if "doppler_frequency" not in self.data.dims:
            raise SMRTError("this result has no doppler_frequency dimension")
        return self.sigma(name=name, **kwargs)

    def waveform(self, name="waveform", **kwargs):
        """The waveform; with return_contributions the total unless contribution="all" or one of them is asked for."""
        if kwargs.get("contribution") == "all":
            del kwargs["contribution"]
        elif "contribution" not in kwargs and "contribution" in self.data.dims:
            kwargs["contribution"] = "total"
        wf = self.sigma(name=name, **kwargs)
        return wf.sum("doppler_frequency") if "doppler_frequency" in wf.dims else wf

    def contributions(self):
        return self.data.coords["contribution"]

    def __repr__(self):
        return f"AltimetryResult: dims={self.data.dims}, shape={self.data.shape}"


def make_result(sensor, *args, **kwargs):
    """smrt/core/result.py:79-90."""
    if sensor.mode == "A":
        return ActiveResult(*args, channel_map=sensor.channel_map, **kwargs)
    return PassiveResult(*args, channel_map=sensor.channel_map, **kwargs)


def concat_results(result_list, coord):
    """One result out of several along a new leading dimension `coord` = (name, labels) -- the nesting step of Model.run
    (smrt/core/result.py:768-817).  Results of sensors with different channel maps get the union of their channels, each
    tagged with the label of the result it came from."""
    if not (isinstance(coord, tuple) and len(coord) == 2):
        raise SMRTError("unknown type for the coord argument")
    dim_name, labels = coord[0], list(coord[1])
    results = list(result_list)
    if len(labels) != len(results) or not results:
        raise SMRTError(f"{len(results)} results cannot be labelled with {len(labels)} values of '{dim_name}'")
    kind = type(results[0])
    if any(type(r) is not kind for r in results):
        raise SMRTError("The results are not all of the same type")
    maps = [r.channel_map for r in results]
    if all(m == maps[0] for m in maps):
        channel_map = maps[0]
    else:
        channel_map = {}
        for m, label in zip(maps, labels):
            for ch, config in m.items():
                # (the reference files the label under the literal key "dim_name", smrt/core/result.py:798-802: no
                # selection ever uses it, channel maps compare equal to the reference's)
                channel_map[ch] = {**config, "dim_name": label}
    data = stack_arrays([r.data for r in results], dim_name, labels)
    other = {key: stack_arrays([r.other_data[key] for r in results], dim_name, labels) for key in results[0].other_data}
    out = kind(data, channel_map=channel_map, other_data=other)
    if all("z_gate" in r.__dict__ for r in results):
        out.z_gate = stack_arrays([r.z_gate for r in results], dim_name, labels)
    return out
