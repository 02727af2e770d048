"""The delay-Doppler model of Dinardo et al. 2018 (counterpart of smrt/rtsolver/delay_doppler_model/dinardo18.py).  The class
names the model in `delay_doppler_model=Dinardo18`; its arithmetic runs on the device
(smrt_amd/csrc/nadir_sar_altimetry_kernel.hpp)."""


class Dinardo18(object):
    pass
