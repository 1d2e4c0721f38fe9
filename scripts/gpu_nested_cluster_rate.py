#!/usr/bin/env python
"""Likelihood rows / s, rows per slice step and rounds of the device nested sampler with clustering on and off
(vega_amd/nested.py: ``NestedSampler(clustering=...)``), on the synthetic joint problem (BASELINE configs[2]: the bench's joint
workload) with 6 sampled parameters - a single-mode posterior, so what is measured is what clustering costs where it cannot help.
Per num_live and run: one JSON line.  The clustering-off lines are the device lines of scripts/gpu_nested_rate.py (same problem,
same seeds, same iterations).  Not a test.

    python scripts/gpu_nested_cluster_rate.py --num-live 512 1024 --iterations 20 --runs 2

The two clustering kernels per launch: run the clustering-on driver alone under the profiler, then summarise

    rocprofv3 --kernel-trace --stats --output-format csv -d trace_dir -- python scripts/gpu_nested_cluster_rate.py --on-only --num-live 512 --iterations 4 --runs 1
    python scripts/gpu_nested_cluster_rate.py --kernel-stats trace_dir
"""
import argparse
import csv
import json
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
for p in (REPO, REPO / 'tests'):
    if str(p) not in sys.path:
        sys.path.insert(0, str(p))

SAMPLED = ['ap', 'at', 'bias_eta_LYA', 'beta_LYA', 'beta_QSO', 'bias_hcd']
KERNELS = ('k_ns_knn', 'k_ns_cluster', 'k_ns_iteration', 'k_ns_advance')


def kernel_stats(folder):
    """Share of k_ns_* in the kernel time of a ``rocprofv3 --kernel-trace --stats`` run, and microseconds per launch."""
    total, mine, calls, rows = 0.0, {}, {}, 0
    for path in Path(folder).rglob('*kernel_stats.csv'):
        with open(path, newline='') as f:
            for row in csv.DictReader(f):
                ns = float(row['TotalDurationNs'])
                total += ns
                rows += 1
                for key in KERNELS:
                    if key in row['Name']:
                        mine[key] = mine.get(key, 0.0) + ns
                        calls[key] = calls.get(key, 0) + int(row['Calls'])
    if not rows:
        raise SystemExit(f'no *kernel_stats.csv under {folder}')
    out = {'kernel_seconds': total * 1e-9, 'share_of_kernel_time': {k: v / total for k, v in mine.items()},
           'microseconds_per_launch': {k: v * 1e-3 / calls[k] for k, v in mine.items()}, 'launches': calls}
    print(json.dumps(out), flush=True)


def main():
    pars = argparse.ArgumentParser()
    pars.add_argument('--num-live', type=int, nargs='+', default=[512, 1024])
    pars.add_argument('--iterations', type=int, default=20)
    pars.add_argument('--runs', type=int, default=2)
    pars.add_argument('--max-batch', type=int, default=256)
    pars.add_argument('--threads', type=int, default=None, help='default: the sampler\'s own (min(num_live / 2, max_batch))')
    pars.add_argument('--on-only', action='store_true')
    pars.add_argument('--kernel-stats', default=None, metavar='DIR')
    args = pars.parse_args()
    if args.kernel_stats:
        return kernel_stats(args.kernel_stats)
    import torch
    torch.cuda.init()
    from conftest import synth_joint_problem
    from vega_amd import NestedSampler, VegaInterface
    from vega_amd.defaults import DEFAULT_VALUES
    vega = VegaInterface(None, problem=synth_joint_problem(), max_batch=args.max_batch)
    sp = {'limits': {n: DEFAULT_VALUES[n][0] for n in SAMPLED}, 'values': {n: vega.params[n] for n in SAMPLED}, 'errors': {}}
    for nlive in args.num_live:
        kw = dict(num_live=nlive, threads=args.threads, sample_params=sp)
        for clustering in ((True,) if args.on_only else (False, True)):
            NestedSampler(vega, seed=1, clustering=clustering, **kw).run(iterations=1)         # (warm-up: lanes, tables, code)
            for run in range(args.runs):
                s = NestedSampler(vega, seed=2, clustering=clustering, **kw).run(iterations=args.iterations)
                st = s.stats
                out = {'num_live': nlive, 'clustering': clustering, 'run': run, 'threads': s.threads, 'num_repeats': s.num_repeats,
                       'iterations': st['iterations'], 'rounds': st['rounds'], 'rows': st['rows'],
                       'device_rows_per_s': st['rows'] / st['seconds'], 'device_seconds': st['seconds'],
                       'seconds_per_round': st['seconds'] / max(st['rounds'], 1),
                       'rows_per_slice_step': (st['rows'] - nlive) / (st['iterations'] * s.threads * s.num_repeats)}
                if clustering:
                    found = s.clusters()
                    out['ids'] = len(found)
                    out['heaviest_mass'] = found[0]['mass']
                print(json.dumps(out), flush=True)
    vega.close()


if __name__ == '__main__':
    main()
