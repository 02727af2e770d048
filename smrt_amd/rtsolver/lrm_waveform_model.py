"""Waveform models of the nadir_lrm_altimetry solver (counterpart of smrt/rtsolver/lrm_waveform_model.py).  Only Brown 1977 is
offered: circular antenna pattern, Earth curvature after Newkirk and Brown 1992, off-nadir pointing or surface slope through
I0.  The class is a marker -- `waveform_model=Brown1977` or None --: the arithmetic is on the device
(smrt_amd/csrc/nadir_lrm_altimetry_kernel.hpp)."""


class Brown1977(object):
    __name__ = "brown_1977"
