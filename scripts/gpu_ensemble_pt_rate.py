#!/usr/bin/env python
"""Parallel tempering of the ensemble sampler (vega_amd/ensemble.py: TemperedEnsemble, vmx_ensemble_run_pt) on the synthetic joint
problem (BASELINE configs[2]: the bench's joint workload) with max_batch 256, at the 6 sampled parameters of
scripts/gpu_ensemble_rate.py and at 15 (ap, at, beta_LYA and the 12 additive broadband coefficients, as
scripts/gpu_ensemble_moves.py takes them), under the DE 0.8 / snooker 0.2 mixture:

(a) proposals / s of a ladder of T = 8 rungs of W = 64 walkers with a swap sweep after every step against ``EnsembleSet`` with
    E = 8, W = 64 - the same rows through the engine, so the difference is the swap kernel's launch per step and the split
    half-step around it;
(b) the integrated autocorrelation time of the cold rung against that of a single ensemble of W = 64 from the same start;
(c) ``log_evidence()`` (stepping stones; thermodynamic integration beside it) against ``SMCSampler`` and ``NestedSampler`` on
    the same box.

The rates are host clocks around calls that end in a device synchronisation, after a warm-up of every shape, over windows of at
least ``--seconds`` (the step count from a short probe), ``--runs`` times with the variants alternating.  Prints one JSON line per
problem.  Not a test.

    python scripts/gpu_ensemble_pt_rate.py --seconds 1.0 --runs 2 --steps 3000
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
MIXTURE = [('de', 0.8), ('snooker', 0.2)]


def main():
    pars = argparse.ArgumentParser()
    pars.add_argument('--seconds', type=float, default=1.0)
    pars.add_argument('--runs', type=int, default=2)
    pars.add_argument('--steps', type=int, default=3000, help='steps of the runs of (b) and (c)')
    pars.add_argument('--ntemps', type=int, default=8)
    pars.add_argument('--walkers', type=int, default=64)
    pars.add_argument('--max-batch', type=int, default=256)
    pars.add_argument('--only', choices=['all', '6', '15'], default='all')
    pars.add_argument('--no-evidence', action='store_true', help='skip the SMC and nested runs of (c)')
    args = pars.parse_args()
    import numpy as np
    import torch
    torch.cuda.init()
    from conftest import synth_joint_problem
    from vega_amd import EnsembleSampler, EnsembleSet, NestedSampler, SMCSampler, TemperedEnsemble, VegaInterface
    from vega_amd.defaults import DEFAULT_VALUES
    vega = VegaInterface(None, problem=synth_joint_problem(), max_batch=args.max_batch)
    vega.freeze_metals()
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
    T, W = args.ntemps, args.walkers

    def clock(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    problems = [('6', sp), ('15', wide)]
    for label, params in problems:
        if args.only not in ('all', label):
            continue
        kw = dict(seed=2, sample_params=params, moves=MIXTURE)
        ladder = TemperedEnsemble(vega, W, ntemps=T, **kw).run(1)
        plain = EnsembleSet(vega, T, W, **kw).run(1)
        ladder.run(3), plain.run(3)                                     # (warm-up: lanes, tables, code)
        out = {'sampled': len(params['limits']), 'T': T, 'W': W, 'max_batch': args.max_batch, 'betas': [float(b) for b in ladder.betas]}
        steps = {}
        for key, s in (('ladder', ladder), ('set', plain)):
            dt, _ = clock(lambda: s.run(20))
            steps[key] = max(20, int(np.ceil(20 * args.seconds / dt * 1.15)))
        rates = {'ladder': [], 'set': []}
        for _ in range(args.runs):
            for key, s in (('ladder', ladder), ('set', plain)):
                s._chain.clear(), s._chain_lnl.clear()                  # (the records of the rate runs are not kept)
                dt, _ = clock(lambda: s.run(steps[key]))
                rates[key].append(steps[key] * T * W / dt)
        out['rate_steps'] = steps
        out['proposals_per_s'] = {key: [round(v) for v in vals] for key, vals in rates.items()}
        out['ladder_over_set'] = round(float(np.mean(rates['ladder']) / np.mean(rates['set'])), 4)
        # (b) and (c): one run of the ladder and of the single ensemble, from starts of their own
        burn = args.steps // 3
        dt, run = clock(lambda: TemperedEnsemble(vega, W, ntemps=T, **kw).run(args.steps))
        _, one = clock(lambda: EnsembleSampler(vega, W, **kw).run(args.steps))
        out['steps'], out['burn'], out['ladder_seconds'] = args.steps, burn, round(dt, 3)
        out['tau_cold_rung'] = float(run.get_autocorr_time(rung=0, discard=burn).max())
        out['tau_single'] = float(one.get_autocorr_time(discard=burn).max())
        out['swap_fraction'] = [round(float(v), 4) for v in run.swap_fraction[0]]
        out['acceptance_by_rung'] = [round(float(run.rung(t).acceptance_fraction.mean()), 4) for t in range(T)]
        out['log_z_ss'] = [float(v) for v in run.log_evidence('ss', discard=burn)]
        out['log_z_ti'] = [float(v) for v in run.log_evidence('ti', discard=burn)]
        out['ladder_rows'] = args.steps * T * W
        if not args.no_evidence:
            dt, smc = clock(lambda: SMCSampler(vega, particles=1024, seed=2, sample_params=params).run())
            out['log_z_smc'], out['smc_rows'], out['smc_seconds'] = [float(v) for v in smc.log_evidence()], smc.stats['rows'], round(dt, 3)
            dt, ns = clock(lambda: NestedSampler(vega, num_live=512, threads=64, seed=2, sample_params=params).run())
            out['log_z_nested'], out['nested_rows'], out['nested_seconds'] = [float(v) for v in ns.log_evidence()], ns.stats['rows'], round(dt, 3)
        print(json.dumps(out), flush=True)
    vega.close()


if __name__ == '__main__':
    main()
