#!/usr/bin/env python
"""Rates of the nadir LRM altimetry solver: 4096 snowpacks of 30 layers, envisat_ra2("Ku"), default options (the slow path with
theta_inc_sampling = 8, 1280 sub-gates).  Four steps, each a child process under its own `timeout`: the NumPy restatement on the
host (no GPU), then -- unless --host-only -- the resident-input rate (median of the HIP-event times of the three kernels over
`steps` launches after `warmup`), the rate with H2D + D2H, and Model.run.  Writes profiles/nadir_lrm_altimetry_rate.txt; a step
that was not run or did not finish is recorded as "not measured"; every line names the processor it was measured on.  No rate is
a gate.
    python tools/bench_nadir_lrm_altimetry.py [--host-only] [--out=FILE] [steps] [warmup] [snowpacks]"""
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
REFERENCE_MS = 10.5    # the reference, one core, 30 layers, envisat_ra2("Ku"), default options: measured once where it is installed
OUT = os.path.join(ROOT, "profiles", "nadir_lrm_altimetry_rate.txt")
LAYERS = 30


def snowpacks(n, seed=0):
    from smrt_amd.inputs.make_medium import make_snowpack

    rng = np.random.RandomState(seed)
    return [make_snowpack(list(rng.uniform(0.05, 0.6, LAYERS)), "exponential", density=list(rng.uniform(250.0, 450.0, LAYERS)),
                          temperature=list(rng.uniform(245.0, 265.0, LAYERS)), corr_length=list(rng.uniform(1e-4, 3e-4, LAYERS)))
            for _ in range(n)]


def packed(n):
    from smrt_amd._native import PackedLrmParams
    from smrt_amd.inputs import lrm_altimeter_list
    from smrt_amd.rtsolver.nadir_lrm_altimetry import NadirLRMAltimetry

    solver, sensor, sps = NadirLRMAltimetry(), lrm_altimeter_list.envisat_ra2("Ku"), snowpacks(n)
    batch = solver._packer()._pack(sensor, sps, np.array([float(sensor.frequency)]), "iba")
    return batch, PackedLrmParams(sensor, oversampling=10, t_inc=solver._t_inc(sensor))


def step_host(n, steps, warmup):
    import types

    from nadir_lrm_altimetry_restatement import solve_case
    from smrt_amd.inputs import lrm_altimeter_list
    from smrt_amd.inputs.make_medium import make_interface, make_snowpack, make_soil

    api = types.SimpleNamespace(make_snowpack=make_snowpack, make_soil=make_soil, make_interface=make_interface, lrm_altimeter_list=lrm_altimeter_list)
    rng = np.random.RandomState(0)
    case = dict(name="bench", sensor="envisat_ra2_Ku", thickness=list(rng.uniform(0.05, 0.6, LAYERS)), density=list(rng.uniform(250.0, 450.0, LAYERS)),
                temperature=list(rng.uniform(245.0, 265.0, LAYERS)), corr_length=list(rng.uniform(1e-4, 3e-4, LAYERS)))
    solve_case(case, api)
    t0 = time.perf_counter()
    for _ in range(20):
        solve_case(case, api)
    return dict(ms_per_solve=(time.perf_counter() - t0) / 20 * 1e3)


def step_resident(n, steps, warmup):
    from smrt_amd._native import DortContext

    batch, params = packed(n)
    ctx = DortContext(0)
    ctx.lrm_upload(batch, params)
    times = []
    for k in range(warmup + steps):
        ctx.lrm_launch()
        ctx.lrm_sync()
        if k >= warmup:
            times.append(ctx.lrm_kernel_ms())
    med = np.median(np.array(times), axis=0)
    assert np.all(ctx.lrm_download().status == 0)
    return dict(kernel_ms=[float(x) for x in med], solves_per_s=n / (med.sum() * 1e-3), spread_ms=float(np.ptp(np.array(times).sum(axis=1))))


def step_transfers(n, steps, warmup):
    from smrt_amd._native import DortContext

    batch, params = packed(n)
    ctx = DortContext(0)
    times = []
    for k in range(warmup + steps):
        t0 = time.perf_counter()
        out = ctx.lrm_run(batch, params)
        if k >= warmup:
            times.append(time.perf_counter() - t0)
    assert np.all(out.status == 0)
    return dict(solves_per_s=n / float(np.median(times)))


def step_model(n, steps, warmup):
    from smrt_amd import make_model
    from smrt_amd.inputs import lrm_altimeter_list

    m, sensor, sps = make_model("iba", "nadir_lrm_altimetry"), lrm_altimeter_list.envisat_ra2("Ku"), snowpacks(n)
    times = []
    for k in range(max(1, warmup) + max(2, steps // 3)):
        t0 = time.perf_counter()
        res = m.run(sensor, sps)
        if k >= max(1, warmup):
            times.append(time.perf_counter() - t0)
    assert np.all(np.isfinite(res.data.values))
    return dict(solves_per_s=n / float(np.median(times)))


STEPS = dict(host=step_host, resident=step_resident, transfers=step_transfers, model=step_model)


def host_cpu():
    try:
        with open("/proc/cpuinfo") as fh:
            return next(line.split(":", 1)[1].strip() for line in fh if line.startswith("model name"))
    except (OSError, StopIteration):
        import platform

        return platform.processor() or platform.machine()


def gpu_name():
    try:
        import torch

        props = torch.cuda.get_device_properties(0)
        return f"{props.name}, {getattr(props, 'gcnArchName', '').split(':')[0]}"
    except Exception:
        return "GPU 0"


def describe(name, r):
    """One line of the file from the JSON of a step, figures rounded to what a timing of this kind resolves."""
    if name == "host":
        return f"{r['ms_per_solve']:.1f} ms per solve ({1e3 / r['ms_per_solve']:.0f} solves/s)"
    if name == "resident":
        k = r["kernel_ms"]
        return (f"{r['solves_per_s']:.3g} solves/s; kernels: layer scalars {k[0]:.2f} ms, vertical distribution {k[1]:.2f} ms, "
                f"waveform {k[2]:.2f} ms per launch (median), spread of the launch total {r['spread_ms']:.2f} ms")
    return f"{r['solves_per_s']:.3g} solves/s"


def main():
    out_path = next((a.split("=", 1)[1] for a in sys.argv[1:] if a.startswith("--out=")), OUT)
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    if "--step" in sys.argv:
        name = sys.argv[sys.argv.index("--step") + 1]
        args = [a for a in args if a != name]
        steps, warmup, n = (int(a) for a in args[:3])
        print(json.dumps(STEPS[name](n, steps, warmup)))
        return
    steps, warmup, n = (int(a) for a in (args + ["10", "2", "4096"][len(args):])[:3])
    lines = ["nadir LRM altimetry solver: rates (tools/bench_nadir_lrm_altimetry.py)",
             f"batch: {n} snowpacks x {LAYERS} layers, envisat_ra2('Ku'), default options (theta_inc_sampling=8, oversampling_time=10)",
             f"yardstick: the reference takes {REFERENCE_MS} ms per (snowpack, frequency) solve on one CPU core (measured once, same case, on "
             "the machine that has the reference installed)"]
    for name in ("host", "resident", "transfers", "model"):
        if name != "host" and "--host-only" in sys.argv:
            lines.append(f"{name}: not measured")
            continue
        cmd = ["timeout", "-k", "10", "300", sys.executable, os.path.abspath(__file__), "--step", name, str(steps), str(warmup), str(n)]
        proc = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        if proc.returncode != 0:
            lines.append(f"{name}: not measured (the step ended with status {proc.returncode})")
            if name != "host":
                break       # nothing more is started on the GPU after a step that failed
            continue
        where = f"NumPy restatement, one core of {host_cpu()}" if name == "host" else gpu_name()
        what = dict(host="host", resident="resident inputs", transfers="with H2D and D2H", model="Model.run")[name]
        lines.append(f"{what} ({where}): {describe(name, json.loads(proc.stdout.strip().splitlines()[-1]))}")
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
