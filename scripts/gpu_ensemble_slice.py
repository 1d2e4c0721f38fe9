#!/usr/bin/env python
"""Ensemble slice sampling (``moves='slice'``) beside the stretch move and the DE 0.8 / snooker 0.2 mixture on the synthetic joint
problem (the bench's joint workload), every figure taken in this process:

1. sampling efficiency at the 6, 15 and 18 sampled parameters of scripts/gpu_ensemble_moves.py, from the same start, seed and
   walkers: tau_max in steps, likelihood rows per update and N / tau per 1000 likelihood rows = 1000 / (tau rows-per-update); a
   chain shorter than 50 tau after the burn-in is marked as a lower bound; for slice also the final mu, the share of box answers
   among the trial points and the capped updates;
2. likelihood rows / s over the wall time of ``run()`` at W = 512 and 1024 against the stretch move's device driver at the same W
   and the nested device driver at nlive = W, alternating repeats; the mean rows of a round as a share of max_batch, the host's
   enqueue seconds; and E = 8 ensembles of W = 64 as one set against eight single runs;
3. ``--kernel-stats DIR``: the two kernels' microseconds per launch and share of kernel time from a
   ``rocprofv3 --kernel-trace --stats --output-format csv -d DIR`` run of ``--only-rate``.

Prints one JSON line per measurement.  Not a test.

    python scripts/gpu_ensemble_slice.py --walkers 128 --steps 4000 --steps-wide 80000 --slice-steps 6000
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
WIDE = ['ap', 'at', 'beta_LYA']
MOVES = [('stretch', None), ('de 0.8 snooker 0.2', [('de', 0.8), ('snooker', 0.2)]), ('slice', 'slice')]


def kernel_stats(folder):
    """Share of k_ens_slice_* in the kernel time of a ``rocprofv3 --kernel-trace --stats`` run."""
    total, mine, calls, rows = 0.0, {}, {}, 0
    for path in Path(folder).rglob('*kernel_stats.csv'):
        with open(path, newline='') as f:
            for row in csv.DictReader(f):
                ns = float(row['TotalDurationNs'])
                total += ns
                rows += 1
                for key in ('k_ens_slice_advance', 'k_ens_slice_emit', 'k_ens_half'):
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
    pars.add_argument('--walkers', type=int, default=128)
    pars.add_argument('--steps', type=int, default=4000, help='steps of the stretch move and the mixture, 6 sampled')
    pars.add_argument('--steps-wide', type=int, default=30000, help='... at 15 and 18 sampled')
    pars.add_argument('--slice-steps', type=int, default=3000, help='steps of the slice sampler, every problem')
    pars.add_argument('--tune-steps', type=int, default=100)
    pars.add_argument('--thin-wide', type=int, default=10, help='the stretch move and the mixture at 15 and 18 sampled record every thin-th step')
    pars.add_argument('--problems', type=int, nargs='*', default=[6, 15, 18])
    pars.add_argument('--rate-walkers', type=int, nargs='*', default=[512, 1024])
    pars.add_argument('--rate-steps', type=int, default=20)
    pars.add_argument('--nested-iterations', type=int, default=10)
    pars.add_argument('--repeats', type=int, default=3)
    pars.add_argument('--max-batch', type=int, default=256)
    pars.add_argument('--only-rate', action='store_true')
    pars.add_argument('--no-rate', action='store_true')
    pars.add_argument('--only-slice', action='store_true', help='part 1 without the stretch move and the mixture')
    pars.add_argument('--kernel-stats', default=None, metavar='DIR')
    args = pars.parse_args()
    if args.kernel_stats:
        return kernel_stats(args.kernel_stats)
    import numpy as np
    import torch
    torch.cuda.init()
    from conftest import synth_joint_problem
    from vega_amd import EnsembleSampler, EnsembleSet, NestedSampler, VegaInterface
    from vega_amd.defaults import DEFAULT_VALUES
    vega = VegaInterface(None, problem=synth_joint_problem(), max_batch=args.max_batch)
    sp = {'limits': {n: DEFAULT_VALUES[n][0] for n in SAMPLED}, 'values': {n: vega.params[n] for n in SAMPLED},
          'errors': {n: DEFAULT_VALUES[n][1] for n in SAMPLED}}
    # the broadband coefficients: the model is linear in them; their scale from the second difference of chi2 at unit offsets
    bb = [n for n in vega.param_names if ' add post ' in n]
    base = vega._theta(None)
    rows = np.repeat(base[None, :], 1 + 2 * len(bb), axis=0)
    for i, n in enumerate(bb):
        rows[1 + 2 * i, vega.param_names.index(n)] += 1.0
        rows[2 + 2 * i, vega.param_names.index(n)] += 2.0
    c = np.asarray(vega.chi2_batch(rows), dtype=np.float64)
    sd = np.array([1.0 / np.sqrt((c[2 + 2 * i] - 2 * c[1 + 2 * i] + c[0]) / 2.0) for i in range(len(bb))])
    wide = {'limits': dict({n: sp['limits'][n] for n in WIDE}, **{n: (vega.params[n] - 50 * s, vega.params[n] + 50 * s) for n, s in zip(bb, sd)}),
            'values': dict({n: sp['values'][n] for n in WIDE}, **{n: vega.params[n] for n in bb}),
            'errors': dict({n: sp['errors'][n] for n in WIDE}, **dict(zip(bb, sd)))}
    every = {key: dict(sp[key], **{n: wide[key][n] for n in bb}) for key in ('limits', 'values', 'errors')}
    W = args.walkers
    problems = {6: (sp, args.steps), len(WIDE) + len(bb): (wide, args.steps_wide), len(SAMPLED) + len(bb): (every, args.steps_wide)}
    for n_sampled in [] if args.only_rate else args.problems:
        params, steps_other = problems[n_sampled]
        for name, moves in MOVES[2:] if args.only_slice else MOVES:
            steps = args.slice_steps if moves == 'slice' else steps_other
            thin = 1 if moves == 'slice' or n_sampled == 6 else args.thin_wide
            kw = dict(tune_steps=args.tune_steps) if moves == 'slice' else {}
            s = EnsembleSampler(vega, W, seed=5, thin=thin, sample_params=params, moves=moves, **kw).run(steps)
            burn = steps // 3
            tau = thin * s.get_autocorr_time(discard=burn // thin)         # (in steps)
            sl = s.stats.get('slice')
            # likelihood rows per update: the stretch and mixture moves spend one row per proposal, in the box or not
            per_update = sl['rows_per_update'] if sl else 1.0
            out = {'problem': f'joint, {n_sampled} sampled', 'moves': name, 'W': W, 'steps': steps, 'burn': burn, 'thin': thin,
                   'tau_max': float(tau.max()), 'tau_is_lower_bound': bool(tau.max() * 50 > steps - burn),
                   'rows_per_update': per_update, 'n_eff_per_1000_rows': 1000.0 / (float(tau.max()) * per_update),
                   'moved_or_accepted_fraction': float(s.acceptance_fraction.mean()), 'seconds': s.stats['seconds'],
                   'rows_per_s': s.stats['proposals'] * per_update / s.stats['seconds']}
            if sl:
                out.update(mu=s.stats['mu'], box_share_of_trial_points=sl['box'] / max(sl['box'] + sl['rows'], 1), capped=sl['capped'],
                           failed=sl['failed'], expansions_per_update=sl['expansions'] / sl['updates'],
                           contractions_per_update=sl['contractions'] / sl['updates'], rounds_per_half=s.stats['rounds'] / (2 * steps))
            else:
                out.update(outside_box=s.stats['rejected_outside_box'] / s.stats['proposals'])
            print(json.dumps(out), flush=True)
    for Wr in [] if args.no_rate else args.rate_walkers:
        nested_kw = dict(num_live=Wr, sample_params=sp)
        EnsembleSampler(vega, Wr, seed=1, sample_params=sp).run(3)                                   # (warm-up: lanes, tables, code)
        EnsembleSampler(vega, Wr, seed=1, sample_params=sp, moves='slice').run(2)
        NestedSampler(vega, seed=1, **nested_kw).run(iterations=1)
        found = {'stretch': [], 'slice': [], 'nested': []}
        extra = {}
        for _ in range(args.repeats):           # (alternating: other work shares the host)
            s = EnsembleSampler(vega, Wr, seed=2, sample_params=sp).run(1)
            t0 = time.perf_counter()
            s.run(10 * args.rate_steps)
            found['stretch'].append(10 * args.rate_steps * Wr / (time.perf_counter() - t0))
            s = EnsembleSampler(vega, Wr, seed=2, sample_params=sp, moves='slice', tune_steps=args.tune_steps).run(1)
            before = dict(rows=s.stats['slice']['rows'], rounds=s.stats['rounds'], enq=s.stats['seconds_enqueuing'])
            t0 = time.perf_counter()
            s.run(args.rate_steps)
            dt = time.perf_counter() - t0
            n_rows, rounds = s.stats['slice']['rows'] - before['rows'], s.stats['rounds'] - before['rounds']
            found['slice'].append(n_rows / dt)
            extra = {'slice_mean_rows_per_round_over_max_batch': n_rows / rounds / args.max_batch,
                     'slice_mean_rows_per_round_over_half': n_rows / rounds / (Wr // 2), 'slice_rounds_per_half': rounds / (2 * args.rate_steps),
                     'slice_seconds_enqueuing': s.stats['seconds_enqueuing'] - before['enq'], 'slice_seconds_wall': dt,
                     'slice_rows_per_update': s.stats['slice']['rows_per_update']}
            t0 = time.perf_counter()
            ns = NestedSampler(vega, seed=2, **nested_kw).run(iterations=args.nested_iterations)
            found['nested'].append(ns.stats['rows'] / (time.perf_counter() - t0))
        print(json.dumps(dict({'rate_W': Wr, 'max_batch': args.max_batch, 'sampled': len(SAMPLED),
                               'rows_per_s_wall': {k: [round(v) for v in vals] for k, vals in found.items()}}, **extra)), flush=True)
    if not args.no_rate:
        kw = dict(seed=2, sample_params=sp, moves='slice', tune_steps=args.tune_steps)
        EnsembleSet(vega, 8, 64, **kw).run(2)
        together, apart = [], []
        for _ in range(args.repeats):
            t0 = time.perf_counter()
            both = EnsembleSet(vega, 8, 64, **kw).run(args.rate_steps)
            together.append(both.stats['slice']['rows'] / (time.perf_counter() - t0))
            t0, n_rows = time.perf_counter(), 0
            for e in range(8):
                n_rows += EnsembleSampler(vega, 64, stream=e, **kw).run(args.rate_steps).stats['slice']['rows']
            apart.append(n_rows / (time.perf_counter() - t0))
        print(json.dumps({'set': 'E = 8 x W = 64', 'steps': args.rate_steps, 'rows_per_s_wall_set': [round(v) for v in together],
                          'rows_per_s_wall_eight_single_runs': [round(v) for v in apart],
                          'set_mean_rows_per_round': both.stats['slice']['rows'] / both.stats['rounds']}), flush=True)
    vega.close()


if __name__ == '__main__':
    main()
