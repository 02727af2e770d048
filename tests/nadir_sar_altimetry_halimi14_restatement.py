"""NumPy restatement of the nadir SAR altimetry solver with the delay-Doppler model of Halimi et al. 2014, written from the
equations (H14 eq. 3-7, 11-15, 19) with DIRECT sums (numpy.convolve; the reference multiplies FFTs), and the case table of the
fixtures tests/golden/nadir_sar_altimetry_halimi14_*.npz.  It stands in for the reference where the reference does not exist
(the GPU tests); tests/test_nadir_sar_altimetry_halimi14_cpu.py holds it to every fixture.

The model.  The flat-surface impulse response at delay tau and Doppler frequency f_n is Pu Nb^2 / pi exp(-4 c tau / (alpha gamma h))
(phi_{n+1} - phi_n) with phi_n = arctan(y_n / sqrt(rho^2 - y_n^2)), y_n = h lambda f_n / (2 v), rho^2 = h c tau / alpha, zero where
the circle of radius rho does not reach the Doppler line.  It is convolved along Doppler with sinc^2(f / (prf / ndoppler)) (times
the frequency step), along the delay with sinc^2(tau B) convolved first with the Gaussian height distribution (times the delay
step, twice), scaled by Nb / prf, and every Doppler column is moved up by floor(idelta_r1 (n - Nb / 2 + 1/2)^2) samples (the slant
range correction).  All three convolutions keep the part of the full convolution that starts (K - 1) // 2 samples in, K the length
of the kernel: 'same' relative to the data.  The map of the volume and of every boundary is this ONE table: convolved with the
volume backscatter, shifted to the boundary and scaled by its incoherent and by its coherent echo.

Pinned, as the reference computes it: the difference along Doppler in the LAST column is phi_0 - phi_1 (negative), not the cyclic
phi_0 - phi_last; the delay kernel has 2 (N // 2) - 1 samples whatever the widening; the Gaussian is sampled, not integrated.
"""
import numpy as np

from nadir_lrm_altimetry_restatement import fresnel_power_v, layer_scalars, vertical_distribution
from nadir_sar_altimetry_restatement import (C_SPEED, DEFAULTS, REL_BAR, axes, coherent_square_decay, contribution_names,  # noqa: F401
                                             make_sensor, prune, solver_options)

_GO = dict(roughness_rms=0.005, corr_length=0.10)
_GO_ROUGH = dict(roughness_rms=0.02, corr_length=0.25)
_IEM = dict(kind="iem_fung92", roughness_rms=5e-4, corr_length=1e-2)
_L1 = dict(thickness=[1.0], density=[300.0], temperature=[260.0], corr_length=[2e-4])
_L3 = dict(thickness=[0.3, 0.5, 1.0], density=[280.0, 350.0, 420.0], temperature=[255.0, 258.0, 260.0], corr_length=[1.5e-4, 2.5e-4, 3e-4])
_SOIL = dict(permittivity_model=complex(5.0, 0.5), temperature=270.0, roughness_rms=0.01, corr_length=0.15)
_S16 = dict(ngate=16, nominal_gate=5, ndoppler=16)


def _h14(**ddm_options):
    return dict(delay_doppler_model="halimi14", delay_doppler_model_options=ddm_options)


# ndoppler >= 16 everywhere: below it the reference warns that the model is not suitable
CASES = [
    dict(name="n16_d16_os1", sensor=_S16, interface=[_GO], sigma_surface=0.0,
         options=dict(oversampling_time=1, oversampling_doppler=1, **_h14()), **_L1),
    # odd N: the delay kernel has 2 (63 // 2) - 1 = N - 2 samples; Nb = 60 is no multiple of 64
    dict(name="n63_d60", sensor=dict(ngate=63, nominal_gate=20, ndoppler=20), interface=[_GO, _GO_ROUGH, _GO], sigma_surface=0.2,
         options=dict(oversampling_time=1, oversampling_doppler=3, return_contributions="basic", **_h14()), **_L3),
    # N = 260, one past a workgroup of 256
    dict(name="n65_d68_os4_full_oversampled", sensor=dict(ngate=65, nominal_gate=20, ndoppler=34), interface=[_GO, _GO_ROUGH], sigma_surface=0.2,
         thickness=[0.4, 1.0], density=[300.0, 380.0], temperature=[258.0, 260.0], corr_length=[2e-4, 3e-4],
         options=dict(oversampling_time=4, oversampling_doppler=2, return_contributions="full coherent", return_oversampled=True, **_h14())),
    dict(name="widening2", sensor=_S16, interface=[_GO, _GO_ROUGH, _GO], substrate=_SOIL, sigma_surface=0.2,
         options=dict(return_contributions="basic coherent", **_h14(delay_window_widening=2)), **_L3),
    dict(name="plrm", sensor=_S16, interface=[_GO], sigma_surface=0.2,
         options=dict(return_contributions="basic", **_h14(slant_range_correction=False, ptr_time="sinc^2", ptr_doppler="sinc^2")), **_L1),
    # the slant range correction of the outer Doppler columns exceeds the window: those columns are zero
    dict(name="shifted_out", sensor=_S16, interface=[_GO], sigma_surface=0.1, options=_h14(), **_L1),
    # the Gaussian (2 sigma / c = 6.7e-11 s) is narrower than the sample spacing (7.8e-10 s)
    dict(name="narrow_pdf", sensor=_S16, interface=[_GO], sigma_surface=0.01, options=_h14(), **_L1),
    # 16 x 12 gates: the circle reaches the outermost Doppler line inside the widened window, where the last column of the
    # impulse response, phi_0 - phi_1, is negative
    dict(name="last_column", sensor=_S16, interface=[_GO], sigma_surface=0.2,
         options=dict(oversampling_time=1, oversampling_doppler=1, **_h14(delay_window_widening=12)), **_L1),
    # interfaces without a mean square slope, which Dinardo18 refuses
    dict(name="iem_surface", sensor=_S16, interface=[_IEM, _IEM], sigma_surface=0.2, thickness=[0.3, 1.0], density=[300.0, 380.0],
         temperature=[258.0, 260.0], corr_length=[2e-4, 3e-4], options=dict(return_contributions="full", **_h14())),
    dict(name="cryosat2_sarm", sensor="cryosat2_sarm", interface=[_GO, _GO_ROUGH, _GO], sigma_surface=0.2, options=_h14(),
         thickness=[0.5, 2.0, 10.0], density=[300.0, 380.0, 450.0], temperature=[255.0, 258.0, 260.0], corr_length=[2e-4, 3e-4, 3e-4]),
    # the second boundary lands on the last sample of the window (31): 8 x 4 sub-gates, its shift is asserted by the fixture maker
    dict(name="last_sample", sensor=dict(ngate=8, nominal_gate=3, ndoppler=16), interface=[_GO, _GO_ROUGH], sigma_surface=0.2,
         thickness=[2.92, 1.0], density=[300.0, 350.0], temperature=[258.0, 260.0], corr_length=[2e-4, 2e-4],
         options=dict(return_contributions="full", **_h14())),
]
TABLE_STORED_UP_TO = 1 << 16     # samples: the reference's own delay_doppler_map is in the fixture of every case but the full-size one


def case_by_name(name):
    return next(c for c in CASES if c["name"] == name)


def model_options(case):
    o = dict(slant_range_correction=True, delay_window_widening=1)
    o.update({k: v for k, v in case["options"]["delay_doppler_model_options"].items() if k in o})
    return o


def build_snowpack(case, api):
    """The snowpack of a case with the constructors of `api` (the package under test or the reference)."""
    def interface(kw):
        kw = dict(kw)
        return api.make_interface(kw.pop("kind", "geometrical_optics_backscatter"), **kw)

    substrate = api.make_soil("geometrical_optics_backscatter", **case["substrate"]) if "substrate" in case else None
    sp = api.make_snowpack(case["thickness"], "exponential", density=case["density"], temperature=case["temperature"],
                           corr_length=case["corr_length"], interface=[interface(kw) for kw in case["interface"]], substrate=substrate)
    sp.terrain_info = api.TerrainInfo(sigma_surface=case.get("sigma_surface", 0.0))
    return sp


def same(full, data_length, kernel_length):
    """The part of a full convolution scipy.signal.fftconvolve(data, kernel, mode="same") keeps."""
    start = (kernel_length - 1) // 2
    return full[start:start + data_length]


def compensation_shifts(sensor, ost, osd):
    """Rows every Doppler column moves up (H14 eq. 19 in samples, with the Earth's curvature), as floats."""
    Nb = sensor.ndoppler * osd
    f1 = 1 / (sensor.ndoppler / sensor.pulse_repetition_frequency) / osd
    wavelength = C_SPEED / sensor.frequency
    delta_r1 = f1 ** 2 * (sensor.alpha * sensor.altitude * wavelength ** 2 / (8 * sensor.velocity ** 2))
    idelta_r1 = delta_r1 * (2 / C_SPEED * sensor.pulse_bandwidth * ost)
    return np.floor(idelta_r1 * (np.arange(Nb) - Nb // 2 + 0.5) ** 2)


def impulse_response(sensor, ost, osd, widening=1):
    """The flat-surface impulse response [N x widening, Nb] (H14 eq. 14 in the Nb^2 convention), NaN replaced by 0."""
    h, B, alpha = sensor.altitude, sensor.pulse_bandwidth, sensor.alpha
    wavelength = C_SPEED / sensor.frequency
    tau = (np.arange(sensor.ngate * widening * ost) / ost - sensor.nominal_gate) / B
    _, fd = axes(sensor, ost, osd)
    y = h * wavelength / (2 * sensor.velocity) * fd[None, :]
    x = (h * tau / alpha * C_SPEED)[:, None] - y ** 2
    inside = x > 0
    phi = np.where(inside, np.arctan(y / np.sqrt(np.where(inside, x, 1.0))), np.nan)
    dphi = np.empty_like(phi)
    dphi[:, :-1] = phi[:, 1:] - phi[:, :-1]
    dphi[:, -1] = phi[:, 0] - phi[:, 1]          # (as halimi14.py:diff_cyclic: not phi_0 - phi_last)
    beamwidth = (sensor.beamwidth_alongtrack + sensor.beamwidth_acrosstrack) / 2
    gamma = np.sin(np.deg2rad(beamwidth)) ** 2 / (2 * np.log(2))
    pu = wavelength ** 2 * sensor.antenna_gain ** 2 * C_SPEED / (4 * (4 * np.pi) ** 2 * h ** 3)
    fsir = pu * sensor.ndoppler ** 2 / np.pi * np.exp(-4 * C_SPEED * tau / (alpha * gamma * h))[:, None] * dphi
    return np.where(np.isnan(fsir), 0.0, fsir)


def delay_kernel(sensor, ost, sigma_surface):
    """sinc^2(tau B) on 2 (N // 2) - 1 samples, convolved with the sampled Gaussian height distribution when sigma_surface > 0."""
    half = sensor.ngate * ost // 2
    dtau = 1 / (ost * sensor.pulse_bandwidth)
    ctau = np.arange(-half + 1, half) * dtau
    ptr = np.sinc(ctau * sensor.pulse_bandwidth) ** 2
    if not sigma_surface > 0:
        return ptr
    s = 2 * sigma_surface / C_SPEED
    pdf = np.exp(-ctau ** 2 / (2 * s ** 2)) / (np.sqrt(2 * np.pi) * s)
    return same(np.convolve(ptr, pdf), len(ptr), len(pdf)) * dtau


def halimi14_table(sensor, ost, osd, sigma_surface, slant_range_correction=True, delay_window_widening=1):
    """The delay-Doppler map [N, Nb] of a surface of unit backscatter."""
    N, Nb = sensor.ngate * ost, sensor.ndoppler * osd
    fsir = impulse_response(sensor, ost, osd, delay_window_widening)
    NW = len(fsir)
    _, fd = axes(sensor, ost, osd)
    ptr_f = np.sinc(fd / (sensor.pulse_repetition_frequency / sensor.ndoppler)) ** 2
    along = np.array([same(np.convolve(row, ptr_f), Nb, Nb) for row in fsir]) * (sensor.pulse_repetition_frequency / Nb)
    kernel = delay_kernel(sensor, ost, sigma_surface)
    dtau = 1 / (ost * sensor.pulse_bandwidth)
    ddm = np.array([same(np.convolve(along[:, c], kernel), NW, len(kernel)) for c in range(Nb)]).T * dtau
    ddm = ddm * (Nb / sensor.pulse_repetition_frequency)
    if slant_range_correction:
        moved = np.zeros_like(ddm)
        for c, up in enumerate(compensation_shifts(sensor, ost, osd)):
            if up < NW:
                moved[:NW - int(up), c] = ddm[int(up):, c]
        ddm = moved
    return ddm[:N]


def solve_case(case, api):
    """dict(ddm [rows, delays, Doppler] (with contributions: them, then the total), contributions, delay, doppler_frequency, gate,
    doppler_bin, z_gate, vertical [N], t_interface, echo [2, boundaries] (coherent, incoherent), shift, table [N, Nb])."""
    opt = dict(DEFAULTS, **solver_options(case))
    sensor, sp = make_sensor(case, api), build_snowpack(case, api)
    ost, osd, B, f = opt["oversampling_time"], opt["oversampling_doppler"], sensor.pulse_bandwidth, float(sensor.frequency)
    L, with_substrate = prune(case, sensor, opt)
    cut = {k: (v[:L] if k in ("thickness", "density", "temperature", "corr_length") else v) for k, v in case.items()}
    _, ke, bs, layers = layer_scalars(cut, f, sp)
    eps = np.array([lay.eps_eff for lay in layers])
    thickness = np.asarray(cut["thickness"], float)
    N, ND, step = sensor.ngate * ost, sensor.ndoppler * osd, B * ost
    # boundaries: transmission, coherent and incoherent echo at the local incidence of the antenna (no mean square slope is read)
    mu_i = np.ones(1) * np.cos(sensor.pitch_angle) * np.cos(sensor.roll_angle)
    k0, beta12 = 2 * np.pi * f / C_SPEED, coherent_square_decay(sensor)
    above = np.concatenate([[1.0 + 0j], eps[:-1]])
    trans, echo = np.empty(L), np.zeros((2, L + 1))

    def one(obj, e1, e2, substrate):
        mu = np.sqrt(1 - (1 - mu_i) / (e1.real if substrate else e1)).real
        d = obj.diffuse_reflection_matrix(*((f, e1) if substrate else (f, e1, e2)), mu, mu, np.pi, 2)
        d = np.asarray(getattr(d, "values", d), float)
        incoherent = float((np.diagonal(d[0, 0, 0]) if d.ndim == 5 else d[0])[0]) / e1.real
        below = complex(obj.permittivity(f)) if substrate else e2
        coherent = fresnel_power_v(e1, below, mu)[0] * np.exp(-4 * (k0 * obj.roughness_rms) ** 2 - (1 - mu[0] ** 2) / beta12) / beta12 / (4 * np.pi)
        return coherent, incoherent

    for k, itf in enumerate(list(sp.interfaces[:L])):
        t = itf.coherent_transmission_matrix(f, above[k], eps[k], np.ones(1), 2)
        trans[k] = np.asarray(getattr(t, "values", t), float)[0, 0]
        echo[0, k], echo[1, k] = one(itf, above[k], eps[k], False)
    if with_substrate:
        echo[0, L], echo[1, L] = one(sp.substrate, eps[-1], None, True)
    speed_eps = np.sqrt(eps).real ** 2
    vertical, z_gate = vertical_distribution(thickness, speed_eps, ke, bs, trans, np.zeros((L + 1, 1)), step, N, False)
    vertical = vertical[0]
    z_gate[0] = 1e-25
    t_interface = np.concatenate([[0.0], 2 * np.cumsum(thickness / (C_SPEED / np.sqrt(eps).real))])
    attenuation = np.exp(-np.concatenate([[0.0], np.cumsum(2 * ke * thickness)])) * np.concatenate([[1.0], np.cumprod(trans ** 2)])
    echo = echo * attenuation
    shift = np.round(t_interface * step).astype(int)
    # the maps: one table for the volume and every boundary
    table = halimi14_table(sensor, ost, osd, case.get("sigma_surface", 0.0), **model_options(case))
    volume = np.array([np.convolve(table[:, c], vertical)[:N] for c in range(ND)]).T

    def shifted(k):
        out = np.zeros_like(table)
        out[k:] = table[:N - k]
        return out

    coh, inc = np.zeros((L + 1, N, ND)), np.zeros((L + 1, N, ND))
    for k in range(L + 1):
        if echo[0, k] > 0 or echo[1, k] > 0:
            assert 0 <= shift[k] < N, "a boundary with a positive echo lies later than the window"
            inc[k], coh[k] = shifted(shift[k]) * max(echo[1, k], 0.0), shifted(shift[k]) * max(echo[0, k], 0.0)
    mode = opt["return_contributions"]
    nb = L + with_substrate      # the reference counts the substrate among its interfaces only when there is one
    names = contribution_names(mode, nb)
    total = inc.sum(axis=0) + coh.sum(axis=0) + volume
    if not names:
        rows = [total]
    elif names[0] == "surface":
        rows = [inc[0] + coh[0], inc[1:].sum(axis=0) + coh[1:].sum(axis=0), volume, total]
    elif names[0] == "incoherent surface":
        rows = [inc[0], coh[0], inc[1:].sum(axis=0), coh[1:].sum(axis=0), volume, total]
    elif names[0] == "interface 0":     # (the reference leaves the coherent echo out of these rows: it is in the total only)
        rows = list(inc[:nb]) + [volume, total]
    else:
        rows = list(inc[:nb]) + list(coh[:nb]) + [volume, total]
    ddm = np.array(rows)
    tau, fd = axes(sensor, ost, osd)
    if not opt["return_oversampled"]:
        ddm = ddm.reshape(len(rows), sensor.ngate, ost, sensor.ndoppler, osd).mean(axis=(2, 4))
        tau, z_gate, fd = tau.reshape(-1, ost).mean(axis=1), z_gate[::ost], fd.reshape(-1, osd).mean(axis=1)
    return dict(ddm=ddm, contributions=names, delay=tau, doppler_frequency=fd, gate=tau * B + sensor.nominal_gate,
                doppler_bin=fd / sensor.pulse_repetition_frequency * sensor.ndoppler, z_gate=z_gate, vertical=vertical,
                t_interface=t_interface, echo=echo, shift=shift, table=table)
