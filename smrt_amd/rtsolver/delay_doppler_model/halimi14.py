"""The delay-Doppler model of Halimi et al. 2014 (counterpart of smrt/rtsolver/delay_doppler_model/halimi14.py).  The class
names the model in `delay_doppler_model=Halimi14`; its arithmetic runs on the device
(smrt_amd/csrc/nadir_sar_altimetry_kernel.hpp: sar_h14_*)."""


class Halimi14(object):
    pass
