#!/usr/bin/env python
"""Moves / s of a set of SMC runs advanced together (vega_amd/smc.py: SMCSet, vmx_smc_run_many) on the synthetic joint problem
(BASELINE configs[2]: the bench's joint workload) with 6 sampled parameters, and in the same process the path a caller had before:
a loop of E single ``SMCSampler`` runs on the same streams, one after the other.  Per shape (E, N): rows evaluated per second of
both, their ratio, the host waits of both, stage rounds, engine calls.  Every timed window holds at least ``--min-seconds``; the
windows of the two paths alternate under fresh seeds, and ``--repeats`` windows give the range.  Prints one JSON line per shape.
Not a test.

    python scripts/gpu_smc_set_rate.py --shapes 16x256 8x512 4x1024 --stages 6

The per-launch times of the E-block kernels: run the set alone under the profiler, then summarise its kernel statistics

    rocprofv3 --kernel-trace --stats --output-format csv -d trace_dir -- python scripts/gpu_smc_set_rate.py --set-only --shapes 16x256 --stages 2 --repeats 1
    python scripts/gpu_smc_set_rate.py --kernel-stats trace_dir
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
KERNELS = ('k_smc_stage', 'k_smc_move', 'k_smc_start_lnl', 'k_smc_start')       # (k_smc_stage: k_smc_stage_kept too)


def kernel_stats(folder):
    """Share and per-launch time of the SMC kernels in a ``rocprofv3 --kernel-trace --stats`` run."""
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
    pars.add_argument('--shapes', nargs='+', default=['16x256', '8x512', '4x1024'], help='ExN: runs x particles')
    pars.add_argument('--stages', type=int, default=6, help='stage rounds per set (24 sweeps each); sets repeat under fresh seeds')
    pars.add_argument('--min-seconds', type=float, default=1.0, help='every timed window holds at least so much')
    pars.add_argument('--repeats', type=int, default=3, help='windows per path and shape')
    pars.add_argument('--max-batch', type=int, default=256)
    pars.add_argument('--set-only', action='store_true')
    pars.add_argument('--kernel-stats', default=None, metavar='DIR')
    args = pars.parse_args()
    if args.kernel_stats:
        return kernel_stats(args.kernel_stats)
    import torch
    torch.cuda.init()
    from conftest import synth_joint_problem
    from vega_amd import SMCSampler, SMCSet, VegaInterface
    from vega_amd.defaults import DEFAULT_VALUES
    vega = VegaInterface(None, problem=synth_joint_problem(), max_batch=args.max_batch)
    sp = {'limits': {n: DEFAULT_VALUES[n][0] for n in SAMPLED}, 'values': {n: vega.params[n] for n in SAMPLED}, 'errors': {}}
    keys = ('rows', 'seconds', 'host_waits', 'engine_calls', 'stages')

    def window_set(E, N, seed):
        """Sets of E runs under fresh seeds until the window is full: totals."""
        tot, k = dict.fromkeys(keys, 0), 0
        while tot['seconds'] < args.min_seconds:
            s = SMCSet(vega, E, particles=N, seed=seed + k, sample_params=sp).run(args.stages)
            for key in keys:
                tot[key] += s.stats[key]
            tot['rounds'] = tot.get('rounds', 0) + s.stats['rounds']
            tot['lanes'] = s.stats['lanes']
            k += 1
        return tot, k

    def window_loop(E, N, seed):
        """The same runs one after the other: E single samplers on the streams 0 .. E - 1 per set."""
        tot, k = dict.fromkeys(keys, 0), 0
        while tot['seconds'] < args.min_seconds:
            for stream in range(E):
                s = SMCSampler(vega, particles=N, seed=seed + k, stream=stream, sample_params=sp).run(stages=args.stages)
                for key in keys:
                    tot[key] += s.stats[key]
            k += 1
        return tot, k

    for shape in args.shapes:
        E, N = (int(v) for v in shape.lower().split('x'))
        SMCSet(vega, E, particles=N, seed=1, sample_params=sp).run(1)                  # (warm-up: lanes, tables, code, buffers)
        if not args.set_only:
            SMCSampler(vega, particles=N, seed=1, sample_params=sp).run(stages=1)
        rates = {'set': [], 'loop': []}
        last = {}
        for r in range(args.repeats):
            seed = 100 + 1000 * r
            for path, window in (('set', window_set),) + (() if args.set_only else (('loop', window_loop),)):
                tot, k = window(E, N, seed)
                rates[path].append(tot['rows'] / tot['seconds'])
                last[path] = dict(tot, sets=k)
        out = {'runs': E, 'particles': N, 'sampled': len(SAMPLED), 'sweeps': 4 * len(SAMPLED), 'max_batch': args.max_batch,
               'stages_per_run': args.stages, 'windows': args.repeats,
               'set_moves_per_s': [min(rates['set']), max(rates['set'])],
               'set_host_waits_per_set': last['set']['host_waits'] / last['set']['sets'],
               'set_engine_calls_per_set': last['set']['engine_calls'] / last['set']['sets'],
               'set_rounds_per_set': last['set']['rounds'] / last['set']['sets'], 'lanes': last['set']['lanes'],
               'set_window_seconds': last['set']['seconds']}
        if not args.set_only:
            out.update({'loop_moves_per_s': [min(rates['loop']), max(rates['loop'])],
                        'loop_host_waits_per_set': last['loop']['host_waits'] / last['loop']['sets'],
                        'loop_engine_calls_per_set': last['loop']['engine_calls'] / last['loop']['sets'],
                        'loop_window_seconds': last['loop']['seconds'],
                        'set_over_loop': [min(rates['set']) / max(rates['loop']), max(rates['set']) / min(rates['loop'])],
                        'set_over_loop_of_medians': sorted(rates['set'])[len(rates['set']) // 2] / sorted(rates['loop'])[len(rates['loop']) // 2]})
        print(json.dumps(out), flush=True)
    vega.close()


if __name__ == '__main__':
    main()
