"""SAR-mode radar altimeters (counterpart of smrt/inputs/sar_altimeter_list.py): CryoSat-2 in SAR mode, Sentinel-3 SRAL and
CRISTAL, for the nadir_sar_altimetry solver.

    from smrt_amd.inputs import sar_altimeter_list
    sensor = sar_altimeter_list.cryosat2_sarm()

Frequencies in Hz, altitudes in m, bandwidths in Hz, velocities in m/s, beam widths and pitch / roll in degrees."""
from ..core.error import SMRTError
from ..core.sensor import make_multi_channel_altimeter, sar_altimeter  # noqa: F401  (part of this module's surface)


def _circular(params):
    beamwidth = (params["beamwidth_alongtrack"] + params["beamwidth_acrosstrack"]) / 2
    return dict(params, beamwidth_alongtrack=beamwidth, beamwidth_acrosstrack=beamwidth)


def cryosat2_sarm(pitch_angle_deg=0, roll_angle_deg=0, force_circular_antenna=False):
    """CryoSat-2 in SAR mode, Hamming window, no zero padding (the nominal gate is an estimate)."""
    params = dict(frequency=13.575e9, altitude=717_242, pulse_bandwidth=320e6, pulse_repetition_frequency=17825, velocity=7435,
                  ngate=128, ndoppler=64, nominal_gate=44, beamwidth_alongtrack=1.08, beamwidth_acrosstrack=1.2,
                  doppler_window="hamming", antenna_gain=1)
    if force_circular_antenna:
        params = _circular(params)
    return sar_altimeter(channel="Ku", **params, pitch_angle_deg=pitch_angle_deg, roll_angle_deg=roll_angle_deg)


def sentinel3_sarm(band, surface, pitch_angle_deg=0, roll_angle_deg=0):
    """Sentinel-3 SRAL in SAR mode; band "Ku" or "C", surface "landice", "ocean" or "seaice" (the Doppler window of the C band)."""
    if surface == "landice":
        doppler_window = "rect"
    elif surface in ("ocean", "seaice"):
        doppler_window = "hamming"
    else:
        raise SMRTError("Invalid surface. Must be landice, ocean or seaice.")
    if band == "Ku":
        params = dict(frequency=13.575e9, altitude=814_500, pulse_bandwidth=320e6, pulse_repetition_frequency=17825, velocity=7450,
                      ngate=128, ndoppler=64, nominal_gate=44, beamwidth_alongtrack=1.35, beamwidth_acrosstrack=1.35,
                      doppler_window="hamming", antenna_gain=1)
    elif band == "C":
        params = dict(frequency=5.41e9, altitude=814_500, pulse_bandwidth=290e6, pulse_repetition_frequency=2 * 78.5, velocity=7450,
                      ngate=128, ndoppler=2, nominal_gate=44, beamwidth_alongtrack=3.4, beamwidth_acrosstrack=3.4, antenna_gain=1,
                      doppler_window=doppler_window)
    else:
        raise SMRTError("Invalid band. Must be Ku or C.")
    return sar_altimeter(channel=band, **params, pitch_angle_deg=pitch_angle_deg, roll_angle_deg=roll_angle_deg)


def cristal(band, pitch_angle_deg=0, roll_angle_deg=0, force_circular_antenna=False):
    """CRISTAL; band "Ku" or "Ka" (the channel is named "Ku" for both, as in the reference)."""
    if band == "Ku":
        params = dict(frequency=13.575e9, altitude=699_000, pulse_bandwidth=500e6, pulse_repetition_frequency=17825, velocity=7524,
                      ngate=256, ndoppler=128, nominal_gate=44, beamwidth_alongtrack=1.08, beamwidth_acrosstrack=1.2,
                      doppler_window="hamming", antenna_gain=1)
    elif band == "Ka":
        params = dict(frequency=35.75e9, altitude=699_000, pulse_bandwidth=500e6, pulse_repetition_frequency=17825, velocity=7524,
                      ngate=256, ndoppler=64, nominal_gate=44, beamwidth_alongtrack=1.08 * 13.5 / 35.7,
                      beamwidth_acrosstrack=1.2 * 13.5 / 35.7, doppler_window="hamming", antenna_gain=1)
    else:
        raise SMRTError("Invalid band. Must be Ku or Ka.")
    if force_circular_antenna:
        params = _circular(params)
    return sar_altimeter(channel="Ku", **params, pitch_angle_deg=pitch_angle_deg, roll_angle_deg=roll_angle_deg)
