"""Low-rate-mode radar altimeters (counterpart of smrt/inputs/lrm_altimeter_list.py): ENVISAT RA-2, Sentinel-3 SRAL, SARAL /
AltiKa, CryoSat-2 in LRM and ASIRAS in low altitude mode, for the nadir_lrm_altimetry solver.

    from smrt_amd.inputs import lrm_altimeter_list
    sensor = lrm_altimeter_list.envisat_ra2("Ku")

Frequencies in Hz, altitudes in m, bandwidths in Hz, beam widths and pitch / roll in degrees."""
from ..core.error import SMRTError
from ..core.sensor import lrm_altimeter, make_multi_channel_altimeter  # noqa: F401  (part of this module's surface)


def _pointing(pitch_angle_deg, roll_angle_deg):
    return dict(pitch_angle_deg=pitch_angle_deg, roll_angle_deg=roll_angle_deg)


def envisat_ra2(channel=None, pitch_angle_deg=0, roll_angle_deg=0):
    """ENVISAT RA-2; channel "Ku", "S", a list of them or None for both."""
    config = {
        "Ku": dict(frequency=13.575e9, altitude=800e3, pulse_bandwidth=320e6, ngate=128, nominal_gate=45,
                   beamwidth_alongtrack=1.29, beamwidth_acrosstrack=1.29, **_pointing(pitch_angle_deg, roll_angle_deg)),
        "S": dict(frequency=3.2e9, altitude=800e3, pulse_bandwidth=160e6, ngate=128, nominal_gate=32,
                  beamwidth_alongtrack=5.5, beamwidth_acrosstrack=5.5, **_pointing(pitch_angle_deg, roll_angle_deg)),
    }
    return make_multi_channel_altimeter(config, channel)


def sentinel3_sral(channel=None, pitch_angle_deg=0, roll_angle_deg=0):
    """Sentinel-3 SRAL in LRM; channel "Ku" only."""
    config = {
        "Ku": dict(frequency=13.575e9, altitude=814e3, pulse_bandwidth=320e6, nominal_gate=44, ngate=128,
                   beamwidth_alongtrack=1.35, beamwidth_acrosstrack=1.35, antenna_gain=1, **_pointing(pitch_angle_deg, roll_angle_deg)),
    }
    return make_multi_channel_altimeter(config, channel)


def saral_altika(pitch_angle_deg=0, roll_angle_deg=0):
    """SARAL / AltiKa (Ka band)."""
    return lrm_altimeter(channel="Ka", frequency=35.75e9, altitude=800e3, pulse_bandwidth=480e6, nominal_gate=51, ngate=128,
                         beamwidth_alongtrack=0.605, beamwidth_acrosstrack=0.605, antenna_gain=1,
                         **_pointing(pitch_angle_deg, roll_angle_deg))


def cryosat2_lrm(pitch_angle_deg=0, roll_angle_deg=0):
    """CryoSat-2 in LRM (beam 1.08 degrees along track, 1.2 across; the nominal gate is an estimate)."""
    return lrm_altimeter(channel="Ku", frequency=13.575e9, altitude=720e3, pulse_bandwidth=320e6, nominal_gate=50, ngate=128,
                         beamwidth_alongtrack=1.08, beamwidth_acrosstrack=1.2, antenna_gain=1,
                         **_pointing(pitch_angle_deg, roll_angle_deg))


def asiras_lam(altitude=None, pitch_angle_deg=0, roll_angle_deg=0):
    """ASIRAS in low altitude mode, at the altitude of the aircraft (beam 2.2 x 9.8 degrees: the Brown model takes their mean)."""
    if altitude is None:
        raise SMRTError("Aircraft altitude must be defined")
    return lrm_altimeter(channel="Ku", frequency=13.5e9, pulse_bandwidth=1e9, altitude=altitude, nominal_gate=41, ngate=256,
                         beamwidth_alongtrack=2.2, beamwidth_acrosstrack=9.8, antenna_gain=1,
                         **_pointing(pitch_angle_deg, roll_angle_deg))
