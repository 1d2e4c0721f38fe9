#!/usr/bin/env python
"""Likelihood rows / s of a set of nested-sampling runs advanced together (vega_amd/nested.py: NestedSet, vmx_nested_run_many) on
the synthetic joint problem (BASELINE configs[2]: the bench's joint workload) with 6 sampled parameters, and in the same process
the path a caller had before: a loop of E single ``NestedSampler`` runs on the same streams, one after the other.  Per shape
(E x nlive / K): rows evaluated per second of both, their ratio, the host waits of both and the mean fill of a round (rows per
round with rows, over max_batch).  Every timed window holds at least ``--min-seconds``; the windows of the two paths alternate
under fresh seeds, and ``--repeats`` windows give the range.  Prints one JSON line per shape.  Not a test.

    python scripts/gpu_nested_set_rate.py --shapes 16x128/32 8x256/64 4x512/128 --iterations 4

``--boost B``: both paths run with ``boost_posterior = B`` (30: every inner point is kept; the set then advances through
k_ns_set_advance_phantoms) and the line also carries the phantom points kept per set.  ``--kish``: instead of rates, one set per
shape to termination with ``--boost`` and the Kish sample size 1 / sum w^2 of every run's boosted and base chain

    python scripts/gpu_nested_set_rate.py --set-only --boost 30 --shapes 16x128/32 8x256/64 4x512/128 --iterations 4
    python scripts/gpu_nested_set_rate.py --kish --boost 30 --shapes 16x128/32

The per-launch times of the set's kernels: run the set alone under the profiler, then summarise its kernel statistics

    rocprofv3 --kernel-trace --stats --output-format csv -d trace_dir -- python scripts/gpu_nested_set_rate.py --set-only --shapes 16x128/32 --iterations 2 --repeats 1
    python scripts/gpu_nested_set_rate.py --kernel-stats trace_dir
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
KERNELS = ('k_ns_set_head', 'k_ns_set_advance_phantoms', 'k_ns_set_advance', 'k_ns_set_emit', 'k_ns_set_draw_live', 'k_ns_set_live_lnl', 'k_ns_iteration',
           'k_ns_advance', 'k_ns_draw_live', 'k_ns_live_lnl')


def kernel_stats(folder):
    """Share and per-launch time of the nested kernels in a ``rocprofv3 --kernel-trace --stats`` run."""
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
                        break
    if not rows:
        raise SystemExit(f'no *kernel_stats.csv under {folder}')
    print(json.dumps({'kernel_seconds': total * 1e-9, 'share_of_kernel_time': {k: v / total for k, v in mine.items()},
                      'microseconds_per_launch': {k: v * 1e-3 / calls[k] for k, v in mine.items()}, 'launches': calls}), flush=True)


def main():
    pars = argparse.ArgumentParser()
    pars.add_argument('--shapes', nargs='+', default=['16x128/32', '8x256/64', '4x512/128'], help='ExNLIVE/K: runs x live points / threads')
    pars.add_argument('--iterations', type=int, default=4, help='iterations per run (30 slice steps per thread each); sets repeat under fresh seeds')
    pars.add_argument('--min-seconds', type=float, default=1.0, help='every timed window holds at least so much')
    pars.add_argument('--repeats', type=int, default=3, help='windows per path and shape')
    pars.add_argument('--max-batch', type=int, default=256)
    pars.add_argument('--set-only', action='store_true')
    pars.add_argument('--boost', type=float, default=0.0, help='boost_posterior of both paths (0: off, the kernels of before)')
    pars.add_argument('--kish', action='store_true', help='one set per shape to termination: the Kish sample sizes, boosted and base')
    pars.add_argument('--kernel-stats', default=None, metavar='DIR')
    args = pars.parse_args()
    if args.kernel_stats:
        return kernel_stats(args.kernel_stats)
    import torch
    torch.cuda.init()
    from conftest import synth_joint_problem
    from vega_amd import NestedSampler, NestedSet, VegaInterface
    from vega_amd.defaults import DEFAULT_VALUES
    vega = VegaInterface(None, problem=synth_joint_problem(), max_batch=args.max_batch)
    sp = {'limits': {n: DEFAULT_VALUES[n][0] for n in SAMPLED}, 'values': {n: vega.params[n] for n in SAMPLED}, 'errors': {}}
    keys = ('rows', 'seconds', 'host_waits', 'engine_calls', 'iterations', 'rounds')
    boost = {'boost_posterior': args.boost} if args.boost > 0.0 else {}
    if args.kish:
        import numpy as np
        for shape in args.shapes:
            runs, rest = shape.lower().split('x')
            E, (nlive, K) = int(runs), (int(v) for v in rest.split('/'))
            s = NestedSet(vega, E, num_live=nlive, threads=K, seed=1, sample_params=sp, **boost).run()
            kish = [[float(1.0 / np.sum(part[2]**2)) for part in s.samples(boost=b)] for b in ((False, True) if boost else (False,))]
            out = {'runs': E, 'num_live': nlive, 'threads': K, 'boost_posterior': args.boost, 'iterations': s.iteration.tolist(),
                   'rows': int(s.stats['rows']), 'seconds': s.stats['seconds'], 'kish_base': [round(v, 1) for v in kish[0]]}
            if boost:
                out.update(kish_boosted=[round(v, 1) for v in kish[1]], phantoms=[int(s.phantoms(e)['lnl'].size) for e in range(E)],
                           boosted_over_base=[round(b / a, 2) for a, b in zip(*kish)],
                           log_z_boost_minus_log_z=[round(float(a - b), 3) for a, b in zip(s.boost_log_evidence(), s.log_evidence()[0])])
            print(json.dumps(out), flush=True)
        vega.close()
        return

    def window_set(E, nlive, K, seed):
        """Sets of E runs under fresh seeds until the window is full: totals.  (A set's rounds include the one that ends each
        iteration; the rounds with rows are those of the longest run.)"""
        tot, k = dict.fromkeys(keys, 0), 0
        while tot['seconds'] < args.min_seconds:
            s = NestedSet(vega, E, num_live=nlive, threads=K, seed=seed + k, sample_params=sp, **boost).run(args.iterations)
            for key in keys:
                tot[key] += s.stats[key]
            tot['lanes'] = s.stats['lanes']
            if boost:
                tot['phantoms'] = tot.get('phantoms', 0) + sum(int(s.phantoms(e)['lnl'].size) for e in range(E))
            k += 1
        return tot, k

    def window_loop(E, nlive, K, seed):
        """The same runs one after the other: E single samplers on the streams 0 .. E - 1 per set."""
        tot, k = dict.fromkeys(keys, 0), 0
        while tot['seconds'] < args.min_seconds:
            for stream in range(E):
                s = NestedSampler(vega, num_live=nlive, threads=K, seed=seed + k, stream=stream, sample_params=sp, **boost).run(args.iterations)
                for key in keys:
                    tot[key] += s.stats[key]
            k += 1
        return tot, k

    for shape in args.shapes:
        runs, rest = shape.lower().split('x')
        E, (nlive, K) = int(runs), (int(v) for v in rest.split('/'))
        NestedSet(vega, E, num_live=nlive, threads=K, seed=1, sample_params=sp, **boost).run(1)      # (warm-up: lanes, tables, code, buffers)
        if not args.set_only:
            NestedSampler(vega, num_live=nlive, threads=K, seed=1, sample_params=sp, **boost).run(1)
        rates = {'set': [], 'loop': []}
        last = {}
        for r in range(args.repeats):
            seed = 100 + 1000 * r
            for path, window in (('set', window_set),) + (() if args.set_only else (('loop', window_loop),)):
                tot, k = window(E, nlive, K, seed)
                rates[path].append(tot['rows'] / tot['seconds'])
                last[path] = dict(tot, sets=k)

        def fill(tot, drawn):
            """Mean rows of a round over max_batch, the drawn live points left out."""
            return (tot['rows'] - drawn * tot['sets']) / max(tot['rounds'], 1) / args.max_batch

        out = {'runs': E, 'num_live': nlive, 'threads': K, 'sampled': len(SAMPLED), 'num_repeats': 5 * len(SAMPLED),
               'max_batch': args.max_batch, 'iterations_per_run': args.iterations, 'windows': args.repeats,
               'set_rows_per_s': [min(rates['set']), max(rates['set'])],
               'set_host_waits_per_set': last['set']['host_waits'] / last['set']['sets'],
               'set_engine_calls_per_set': last['set']['engine_calls'] / last['set']['sets'],
               'set_rounds_per_set': last['set']['rounds'] / last['set']['sets'], 'set_fill_per_round': fill(last['set'], E * nlive),
               'lanes': last['set']['lanes'], 'set_window_seconds': last['set']['seconds']}
        if boost:
            out.update(boost_posterior=args.boost, set_phantoms_per_set=last['set']['phantoms'] / last['set']['sets'])
        if not args.set_only:
            out.update({'loop_rows_per_s': [min(rates['loop']), max(rates['loop'])],
                        'loop_host_waits_per_set': last['loop']['host_waits'] / last['loop']['sets'],
                        'loop_engine_calls_per_set': last['loop']['engine_calls'] / last['loop']['sets'],
                        'loop_fill_per_round': fill(last['loop'], E * nlive),
                        'loop_window_seconds': last['loop']['seconds'],
                        'set_over_loop': [min(rates['set']) / max(rates['loop']), max(rates['set']) / min(rates['loop'])],
                        'set_over_loop_of_medians': sorted(rates['set'])[len(rates['set']) // 2] / sorted(rates['loop'])[len(rates['loop']) // 2]})
        print(json.dumps(out), flush=True)
    vega.close()


if __name__ == '__main__':
    main()
