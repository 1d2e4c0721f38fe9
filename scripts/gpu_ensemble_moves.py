#!/usr/bin/env python
"""The ensemble sampler's moves beside each other on the synthetic joint problem (the bench's joint workload): integrated
autocorrelation time, acceptance and effective samples per likelihood row of the stretch, DE and snooker moves and the DE 0.8 /
snooker 0.2 mixture from the same start, seed, walkers and steps - at the 6 sampled parameters of scripts/gpu_ensemble_rate.py and
at 15 (ap, at, beta_LYA and the 12 additive broadband coefficients) - and the proposals / s of a device segment for every move.
``--moves`` picks the moves by name from those below and from the covariance move's (``cov``, ``cov 0.8 snooker 0.2``; they report
the factor fallbacks too); ``--rate-sampled 18`` takes the segment's rate over the six and the twelve coefficients.
Prints one JSON line per measurement.  Not a test.

    python scripts/gpu_ensemble_moves.py --walkers 128 --steps 4000 --steps-wide 30000 --rate-walkers 512 1024
    python scripts/gpu_ensemble_moves.py --moves cov "cov 0.8 snooker 0.2" "de 0.8 snooker 0.2" --steps-wide 80000 --steps-all 80000 --thin 10
"""
import argparse
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
MOVES = [('stretch', None), ('de', 'de'), ('snooker', 'snooker'), ('de 0.8 snooker 0.2', [('de', 0.8), ('snooker', 0.2)])]
COV_MOVES = [('cov', 'cov'), ('cov 0.8 snooker 0.2', [('cov', 0.8), ('snooker', 0.2)])]


def main():
    pars = argparse.ArgumentParser()
    pars.add_argument('--walkers', type=int, default=128)
    pars.add_argument('--steps', type=int, default=4000)
    pars.add_argument('--steps-wide', type=int, default=30000)
    pars.add_argument('--rate-walkers', type=int, nargs='*', default=[512, 1024])
    pars.add_argument('--rate-steps', type=int, default=200)
    pars.add_argument('--repeats', type=int, default=3)
    pars.add_argument('--max-batch', type=int, default=256)
    pars.add_argument('--only-rate', action='store_true')
    pars.add_argument('--only-wide', action='store_true')
    pars.add_argument('--thin', type=int, default=1, help='record every thin-th step (tau is reported in steps)')
    pars.add_argument('--steps-all', type=int, default=0, help='> 0: also the six and the twelve coefficients together (18)')
    pars.add_argument('--moves', nargs='*', default=None, help='the moves to run, by name (default: the four without cov)')
    pars.add_argument('--only-narrow', action='store_true', help='of the tau problems, the six parameters alone')
    pars.add_argument('--factor-calls', type=int, default=0,
                      help='> 0: so many calls of the covariance move\'s factor stage alone at every rate W, n = 6, 18 and 64')
    pars.add_argument('--rate-sampled', type=int, choices=(6, 18), default=6, help='the sampled parameters of the rate part')
    args = pars.parse_args()
    known = dict(MOVES + COV_MOVES)
    moves_run = MOVES if args.moves is None else [(name, known[name]) for name in args.moves]
    import numpy as np
    import torch
    torch.cuda.init()
    from conftest import synth_joint_problem
    from vega_amd import EnsembleSampler, VegaInterface
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
    problems = [] if args.only_rate else [('joint, 6 sampled', sp, args.steps), (f'joint, {len(WIDE) + len(bb)} sampled', wide, args.steps_wide)]
    if args.only_narrow:
        problems = problems[:1]
    elif args.steps_all > 0 and problems:
        problems.append((f'joint, {len(SAMPLED) + len(bb)} sampled', every, args.steps_all))
    for label, params, steps in problems[1:] if args.only_wide else problems:
        for name, moves in moves_run:
            s = EnsembleSampler(vega, W, seed=5, thin=args.thin, sample_params=params, moves=moves).run(steps)
            burn = steps // 3
            tau = args.thin * s.get_autocorr_time(discard=burn // args.thin)
            n_rows = (steps - burn) * W
            out = {'problem': label, 'moves': name, 'W': W, 'steps': steps, 'burn': burn, 'tau_max': float(tau.max()),
                   'tau_mean': float(tau.mean()), 'tau_over_window': float(tau.max() * 50 / (steps - burn)),
                   'acceptance': float(s.acceptance_fraction.mean()), 'n_eff_per_1000_rows': 1000.0 / float(tau.max()),
                   'n_eff': n_rows / float(tau.max()), 'outside_box': s.stats['rejected_outside_box'],
                   'failed_model': s.stats['rejected_failed_model'], 'proposals_per_s': s.stats['proposals'] / s.stats['seconds'],
                   'thin': args.thin, 'mean': [float(v) for v in s.get_chain(discard=burn // args.thin, flat=True).mean(axis=0)[:6]]}
            if 'moves' in s.stats:
                out['per_move'] = dict(s.stats['moves'])
            if 'cov' in s.stats:
                out['cov'] = dict(s.stats['cov'])
            out['at_least_50_tau'] = bool(steps - burn >= 50 * float(tau.max()))
            print(json.dumps(out), flush=True)
    rate_sp = sp if args.rate_sampled == 6 else every
    for Wr in args.rate_walkers:
        for name, moves in moves_run:
            EnsembleSampler(vega, Wr, seed=1, sample_params=rate_sp, moves=moves).run(3)            # (warm-up: lanes, tables, code)
        # proposals / s three ways: over the library's own clock (the device segment), over the wall time of run() (with the
        # host's share: the start excluded, it is drawn before), and over that plus reading the per-move counts
        rates, wall, counted = ({name: [] for name, _ in moves_run} for _ in range(3))
        for _ in range(args.repeats):           # (alternating the moves: other work shares the host)
            for name, moves in moves_run:
                s = EnsembleSampler(vega, Wr, seed=2, sample_params=rate_sp, moves=moves).run(1)
                t0 = time.perf_counter()
                s.run(args.rate_steps)
                t1 = time.perf_counter()
                if moves is not None:
                    dict(s.stats['moves'])
                t2 = time.perf_counter()
                done = args.rate_steps * Wr
                rates[name].append(done / (s.stats['seconds'] * args.rate_steps / (args.rate_steps + 1)))
                wall[name].append(done / (t1 - t0))
                counted[name].append(done / (t2 - t0))
        print(json.dumps({'rate_W': Wr, 'steps': args.rate_steps, 'sampled': len(rate_sp['limits']), 'max_batch': args.max_batch,
                          'proposals_per_s': {name: [round(v) for v in vals] for name, vals in rates.items()},
                          'proposals_per_s_wall': {name: [round(v) for v in vals] for name, vals in wall.items()},
                          'proposals_per_s_wall_with_counts': {name: [round(v) for v in vals] for name, vals in counted.items()}}),
              flush=True)
    for Wr in args.rate_walkers if args.factor_calls > 0 else []:
        for n in (6, 18, 64):
            half = np.random.default_rng(n).normal(size=(1, Wr // 2, n))
            vega.engine.ensemble_cov_factor(half)
            t0 = time.perf_counter()
            for _ in range(args.factor_calls):
                vega.engine.ensemble_cov_factor(half)
            print(json.dumps({'factor_H': Wr // 2, 'n': n, 'calls': args.factor_calls,
                              'wall_us_per_call_with_copies': 1e6 * (time.perf_counter() - t0) / args.factor_calls}), flush=True)
    vega.close()


if __name__ == '__main__':
    main()
