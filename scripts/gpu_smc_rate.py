#!/usr/bin/env python
"""Moves / s of the SMC sampler's two drivers (vega_amd/smc.py) on the synthetic joint problem (BASELINE configs[2]: the bench's
joint workload) with 6 sampled parameters, and in the same process the yardsticks at equal size: the ensemble sampler's device
driver at W = N walkers, the nested sampler's device driver at num_live = N, and a bare ``chi2_batch_device`` loop over the same N
rows in the same chunks.  Per N: stages, the share of rows that were real evaluations (a proposal outside the cube asks for the
particle's own position), host waits.  ``--linear``: the four linear broadband coefficients of the auto problem (the exact-evidence
case of the GPU tests), likelihood evaluations and seconds to ``log Z +- err`` for SMC and for the nested sampler.  Prints one JSON
line per N.  Not a test.

    python scripts/gpu_smc_rate.py --particles 512 1024 --stages 6
    python scripts/gpu_smc_rate.py --linear

The share of the sampler's own kernels: run the device driver alone under the profiler, then summarise its kernel statistics

    rocprofv3 --kernel-trace --stats --output-format csv -d trace_dir -- python scripts/gpu_smc_rate.py --device-only --particles 1024 --stages 2
    python scripts/gpu_smc_rate.py --kernel-stats trace_dir
"""
import argparse
import csv
import json
import sys
import time
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
for p in (REPO, REPO / 'tests'):
    if str(p) not in sys.path:
        sys.path.insert(0, str(p))

SAMPLED = ['ap', 'at', 'bias_eta_LYA', 'beta_LYA', 'beta_QSO', 'bias_hcd']


def kernel_stats(folder):
    """Share of k_smc_* in the kernel time of a ``rocprofv3 --kernel-trace --stats`` run."""
    total, mine, calls, rows = 0.0, {}, {}, 0
    for path in Path(folder).rglob('*kernel_stats.csv'):
        with open(path, newline='') as f:
            for row in csv.DictReader(f):
                ns = float(row['TotalDurationNs'])
                total += ns
                rows += 1
                name = row['Name']
                for key in ('k_smc_stage', 'k_smc_move', 'k_smc_start_lnl', 'k_smc_start'):
                    if key in name:
                        mine[key] = mine.get(key, 0.0) + ns
                        calls[key] = calls.get(key, 0) + int(row['Calls'])
                        break
    if not rows:
        raise SystemExit(f'no *kernel_stats.csv under {folder}')
    out = {'kernel_seconds': total * 1e-9, 'share_of_kernel_time': {k: v / total for k, v in mine.items()},
           'microseconds_per_launch': {k: v * 1e-3 / calls[k] for k, v in mine.items()}, 'launches': calls}
    print(json.dumps(out), flush=True)


def linear_case(args):
    """SMC and the nested sampler side by side on the exact-evidence problem of tests/test_*_gpu.py."""
    import numpy as np
    from conftest import GOLDEN
    from test_nested_gpu import _linear_gaussian
    from vega_amd import NestedSampler, SMCSampler, VegaInterface
    vega = VegaInterface('configs/auto/main.ini', search_dirs=[GOLDEN], max_batch=256)
    names, mean, cov, F, lnl_max = _linear_gaussian(vega)
    sd = np.sqrt(np.diag(cov))
    truth = lnl_max + 0.5 * np.linalg.slogdet(2 * np.pi * cov)[1] - np.sum(np.log(20 * sd))
    sp = {'limits': {n: (m - 10 * s, m + 10 * s) for n, m, s in zip(names, mean, sd)}, 'values': dict(zip(names, mean)),
          'errors': dict(zip(names, sd))}
    SMCSampler(vega, particles=1024, seed=1, sample_params=sp).run(stages=1)                     # (warm-up)
    NestedSampler(vega, num_live=256, threads=64, seed=1, sample_params=sp).run(iterations=1)
    for seed in range(args.seeds):
        s = SMCSampler(vega, particles=1024, seed=seed, sample_params=sp).run()
        n = NestedSampler(vega, num_live=256, threads=64, seed=seed, sample_params=sp).run()
        (zs, es), (zn, en) = s.log_evidence(), n.log_evidence()
        print(json.dumps({'seed': seed, 'log_z_true': truth,
                          'smc': {'log_z': zs, 'err': es, 'pull': (zs - truth) / es, 'stages': s.stage, 'rows': s.stats['rows'],
                                  'seconds': s.stats['seconds']},
                          'nested': {'log_z': zn, 'err': en, 'pull': (zn - truth) / en, 'iterations': n.iteration,
                                     'rows': n.stats['rows'], 'seconds': n.stats['seconds']}}), flush=True)
    vega.close()


def main():
    pars = argparse.ArgumentParser()
    pars.add_argument('--particles', type=int, nargs='+', default=[512, 1024])
    pars.add_argument('--stages', type=int, default=6, help='stages per run (24 sweeps each); runs repeat under fresh seeds')
    pars.add_argument('--min-seconds', type=float, default=1.0, help='every timed window holds at least so much')
    pars.add_argument('--max-batch', type=int, default=256)
    pars.add_argument('--device-only', action='store_true')
    pars.add_argument('--linear', action='store_true')
    pars.add_argument('--seeds', type=int, default=2)
    pars.add_argument('--kernel-stats', default=None, metavar='DIR')
    args = pars.parse_args()
    if args.kernel_stats:
        return kernel_stats(args.kernel_stats)
    import numpy as np
    import torch
    torch.cuda.init()
    if args.linear:
        return linear_case(args)
    from conftest import synth_joint_problem
    from vega_amd import EnsembleSampler, NestedSampler, SMCSampler, VegaInterface
    from vega_amd.nested import map_cube
    vega = VegaInterface(None, problem=synth_joint_problem(), max_batch=args.max_batch)
    from vega_amd.defaults import DEFAULT_VALUES
    sp = {'limits': {n: DEFAULT_VALUES[n][0] for n in SAMPLED}, 'values': {n: vega.params[n] for n in SAMPLED}, 'errors': {}}
    for N in args.particles:
        kw = dict(particles=N, sample_params=sp)
        SMCSampler(vega, seed=1, **kw).run(stages=1)                                   # (warm-up: lanes, tables, code)
        # runs of `stages` stages under fresh seeds until the timed window holds `min_seconds`
        tot = dict(rows=0, seconds=0.0, seconds_enqueuing=0.0, rows_own_position=0, accepted=0, stages=0, host_waits=0,
                   engine_calls=0)
        runs = 0
        while tot['seconds'] < args.min_seconds:
            s = SMCSampler(vega, seed=2 + runs, **kw).run(stages=args.stages)
            for key in tot:
                tot[key] += s.stats[key]
            runs += 1
        moves = tot['rows'] - runs * N
        out = {'particles': N, 'sweeps': s.sweeps, 'sampled': len(SAMPLED), 'max_batch': args.max_batch, 'runs': runs,
               'stages': tot['stages'], 'rows': tot['rows'], 'device_moves_per_s': tot['rows'] / tot['seconds'],
               'device_seconds': tot['seconds'], 'device_seconds_enqueuing': tot['seconds_enqueuing'],
               'host_waits': tot['host_waits'], 'engine_calls': tot['engine_calls'], 'lanes': s.stats['lanes'],
               'share_of_rows_that_were_real_evaluations': 1.0 - tot['rows_own_position'] / tot['rows'],
               'acceptance': tot['accepted'] / max(moves, 1), 'device_const_hint': int(vega.engine.derived_const_hint(s.cols))}
        if not args.device_only:
            rows_p, sec_p, k = 0, 0.0, 0
            while sec_p < args.min_seconds:
                p = SMCSampler(vega, seed=2 + k, driver='python', **kw).run(stages=args.stages)
                rows_p, sec_p, k = rows_p + p.stats['rows'], sec_p + p.stats['seconds'], k + 1
            out['python_moves_per_s'] = rows_p / sec_p
            out['python_seconds'] = sec_p
            out['device_over_python'] = out['device_moves_per_s'] / out['python_moves_per_s']
            # the ensemble sampler's device driver at W = N walkers
            EnsembleSampler(vega, N, seed=1, sample_params=sp).run(2, start='prior')
            e = EnsembleSampler(vega, N, seed=2, sample_params=sp)
            e.run(20, start='prior')
            done, dt = 0, 0.0
            while dt < args.min_seconds:
                t0 = time.perf_counter()
                e.run(500, start='prior')
                dt += time.perf_counter() - t0
                done += 500 * N
            out['ensemble_proposals_per_s'] = done / dt
            out['ensemble_seconds'] = dt
            # the nested sampler's device driver at num_live = N
            NestedSampler(vega, num_live=N, seed=1, sample_params=sp).run(iterations=1)
            ns = NestedSampler(vega, num_live=N, seed=2, sample_params=sp).run(iterations=20)
            out['nested_rows_per_s'] = ns.stats['rows'] / ns.stats['seconds']
            out['nested_seconds'] = ns.stats['seconds']
            out['nested_share_of_rows_that_were_real_evaluations'] = 1.0 - ns.stats['rows_own_position'] / ns.stats['rows']
            # the engine alone on the same N rows: chunks of max_batch, two lanes, the same table level
            eng = vega.engine
            theta = np.repeat(vega._theta(None)[None, :], N, axis=0)
            theta[:, s.cols] = map_cube(s.lo, s.hi, s.u)
            t = torch.from_numpy(theta).cuda()
            chunks = [t[k:k + args.max_batch].contiguous() for k in range(0, N, args.max_batch)]
            hint = out['device_const_hint']
            eng.set_constant_nl_hint(hint > 0, hint >= 2)
            eng.set_lanes(2)
            for c in chunks:
                vega.chi2_batch_device(c)
            torch.cuda.synchronize()
            reps, dt = 0, 0.0
            while dt < args.min_seconds:
                t0 = time.perf_counter()
                for _ in range(200):
                    for c in chunks:
                        vega.chi2_batch_device(c)
                torch.cuda.synchronize()
                dt += time.perf_counter() - t0
                reps += 200
            eng.set_lanes(1)
            eng.set_constant_nl_hint(False)
            out['bare_chi2_batch_device_rows_per_s'] = reps * N / dt
            out['bare_seconds'] = dt
            out['device_over_bare'] = out['device_moves_per_s'] / out['bare_chi2_batch_device_rows_per_s']
            out['device_over_ensemble'] = out['device_moves_per_s'] / out['ensemble_proposals_per_s']
            out['device_over_nested'] = out['device_moves_per_s'] / out['nested_rows_per_s']
        print(json.dumps(out), flush=True)
    vega.close()


if __name__ == '__main__':
    main()
