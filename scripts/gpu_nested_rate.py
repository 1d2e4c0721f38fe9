#!/usr/bin/env python
"""Likelihood rows / s of the nested sampler's two drivers (vega_amd/nested.py) and of a bare ``chi2_batch_device`` loop over
batches of ``threads`` rows, on the synthetic joint problem (BASELINE configs[2]: the bench's joint workload) with 6 sampled
parameters.  Per num_live: rounds, the share of rows that were real evaluations (a thread whose point left the cube asks for its own
position), the mean rows of a round against ``threads`` (the tail in which finished threads wait for the slowest), host waits.
Prints one JSON line per num_live.  Not a test.

    python scripts/gpu_nested_rate.py --num-live 512 1024 --iterations 20

``--boost B`` runs the device driver with ``boost_posterior = B`` (B >= num_repeats keeps every inner point) and adds the kept
phantom points, also per million engine rows; ``--terminate`` then runs a second sampler to termination and adds the Kish sample
size 1 / sum p^2 of its boosted chain against its unboosted one

    python scripts/gpu_nested_rate.py --device-only --num-live 512 --iterations 20 --boost 30 --terminate

The share of the sampler's own kernels: run the device driver alone under the profiler, then summarise its kernel statistics

    rocprofv3 --kernel-trace --stats --output-format csv -d trace_dir -- python scripts/gpu_nested_rate.py --device-only --num-live 512 --iterations 4
    python scripts/gpu_nested_rate.py --kernel-stats trace_dir
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
    """Share of k_ns_* in the kernel time of a ``rocprofv3 --kernel-trace --stats`` run."""
    total, mine, calls, rows = 0.0, {}, {}, 0
    for path in Path(folder).rglob('*kernel_stats.csv'):
        with open(path, newline='') as f:
            for row in csv.DictReader(f):
                ns = float(row['TotalDurationNs'])
                total += ns
                rows += 1
                name = row['Name']
                for key in ('k_ns_advance_phantoms', 'k_ns_iteration', 'k_ns_advance', 'k_ns_draw_live', 'k_ns_live_lnl'):
                    if key in name:
                        mine[key] = mine.get(key, 0.0) + ns
                        calls[key] = calls.get(key, 0) + int(row['Calls'])
                        break
    if not rows:
        raise SystemExit(f'no *kernel_stats.csv under {folder}')
    out = {'kernel_seconds': total * 1e-9, 'share_of_kernel_time': {k: v / total for k, v in mine.items()},
           'microseconds_per_launch': {k: v * 1e-3 / calls[k] for k, v in mine.items()}, 'launches': calls}
    print(json.dumps(out), flush=True)


def main():
    pars = argparse.ArgumentParser()
    pars.add_argument('--num-live', type=int, nargs='+', default=[512, 1024])
    pars.add_argument('--iterations', type=int, default=20)
    pars.add_argument('--python-iterations', type=int, default=6)
    pars.add_argument('--max-batch', type=int, default=256)
    pars.add_argument('--threads', type=int, default=None, help='default: the sampler\'s own (min(num_live / 2, max_batch))')
    pars.add_argument('--device-only', action='store_true')
    pars.add_argument('--boost', type=float, default=0.0, help='boost_posterior of the device run (0: off)')
    pars.add_argument('--terminate', action='store_true', help='with --boost: a run to termination and its sample sizes')
    pars.add_argument('--kernel-stats', default=None, metavar='DIR')
    args = pars.parse_args()
    if args.kernel_stats:
        return kernel_stats(args.kernel_stats)
    import numpy as np
    import torch
    torch.cuda.init()
    from conftest import synth_joint_problem
    from vega_amd import NestedSampler, VegaInterface
    from vega_amd.nested import map_cube
    vega = VegaInterface(None, problem=synth_joint_problem(), max_batch=args.max_batch)
    from vega_amd.defaults import DEFAULT_VALUES
    sp = {'limits': {n: DEFAULT_VALUES[n][0] for n in SAMPLED}, 'values': {n: vega.params[n] for n in SAMPLED}, 'errors': {}}
    for nlive in args.num_live:
        kw = dict(num_live=nlive, threads=args.threads, sample_params=sp)
        boost = dict(boost_posterior=args.boost) if args.boost > 0.0 else {}
        NestedSampler(vega, seed=1, **kw, **boost).run(iterations=1)                   # (warm-up: lanes, tables, code)
        s = NestedSampler(vega, seed=2, **kw, **boost).run(iterations=args.iterations)
        st = s.stats
        out = {'num_live': nlive, 'threads': s.threads, 'num_repeats': s.num_repeats, 'sampled': len(SAMPLED),
               'max_batch': args.max_batch, 'iterations': st['iterations'], 'rounds': st['rounds'], 'rows': st['rows'],
               'device_rows_per_s': st['rows'] / st['seconds'], 'device_seconds': st['seconds'],
               'device_seconds_enqueuing': st['seconds_enqueuing'], 'host_waits': st['host_waits'],
               'engine_calls': st['engine_calls'],
               'share_of_rows_that_were_real_evaluations': 1.0 - st['rows_own_position'] / st['rows'],
               'mean_rows_per_round_over_threads': (st['rows'] - nlive) / max(st['rounds'], 1) / s.threads,
               'rows_per_slice_step': (st['rows'] - nlive) / (st['iterations'] * s.threads * s.num_repeats),
               'device_const_hint': int(vega.engine.derived_const_hint(s.cols))}
        if boost:
            kept = int(s.phantoms()['lnl'].size)
            out.update(boost_posterior=args.boost, kept_fraction=s.phantom_state.fraction, phantom_points=kept,
                       phantom_points_per_million_rows=kept / st['rows'] * 1e6, calls=st['calls'])
            if args.terminate:
                full = NestedSampler(vega, seed=2, **kw, **boost).run()
                w, w0 = full.samples()[2], full.samples(boost=False)[2]
                rows = full.stats['rows']
                out['terminated'] = {'iterations': full.iteration, 'rows': rows, 'rows_per_s': rows / full.stats['seconds'],
                                     'phantom_points': int(full.phantoms()['lnl'].size),
                                     'phantom_points_per_million_rows': full.phantoms()['lnl'].size / rows * 1e6,
                                     'base_samples_per_million_rows': w0.size / rows * 1e6,
                                     'sample_size_boosted': float(1.0 / np.sum(w**2)), 'sample_size_base': float(1.0 / np.sum(w0**2)),
                                     'sample_size_ratio': float(np.sum(w0**2) / np.sum(w**2)),
                                     'log_z': full.log_evidence(), 'log_z_boosted': full.boost_log_evidence()}
        if not args.device_only:
            p = NestedSampler(vega, seed=2, driver='python', **kw).run(iterations=args.python_iterations)
            out['python_rows_per_s'] = p.stats['rows'] / p.stats['seconds']
            out['device_over_python'] = out['device_rows_per_s'] / out['python_rows_per_s']
            # the engine alone on batches of `threads` rows: chunks of max_batch, two lanes, the same table level
            eng = vega.engine
            theta = np.repeat(vega._theta(None)[None, :], s.threads, axis=0)
            theta[:, s.cols] = map_cube(s.lo, s.hi, s.live_u[:s.threads])
            t = torch.from_numpy(theta).cuda()
            hint = out['device_const_hint']
            eng.set_constant_nl_hint(hint > 0, hint >= 2)
            eng.set_lanes(2)
            vega.chi2_batch_device(t)
            torch.cuda.synchronize()
            reps = 200
            t0 = time.perf_counter()
            for _ in range(reps):
                vega.chi2_batch_device(t)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            eng.set_lanes(1)
            eng.set_constant_nl_hint(False)
            out['bare_chi2_batch_device_rows_per_s'] = reps * s.threads / dt
            out['device_over_bare'] = out['device_rows_per_s'] / out['bare_chi2_batch_device_rows_per_s']
        print(json.dumps(out), flush=True)
    vega.close()


if __name__ == '__main__':
    main()
