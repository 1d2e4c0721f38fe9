#!/usr/bin/env python
"""Adaptive temperature ladders of the ensemble sampler (vega_amd/ensemble.py: TemperedEnsemble(adapt=True),
vmx_ensemble_run_pt_adapt) on the synthetic joint problem (BASELINE configs[2]: the bench's joint workload) with max_batch 256, at
the 6 sampled parameters of scripts/gpu_ensemble_pt_rate.py, under the DE 0.8 / snooker 0.2 mixture:

(a) proposals / s of an adapting ladder of T = 8 rungs of W = 64 walkers with a swap sweep after every step against the fixed
    ladder of the same build - the same rows through the engine and the same launches, so the difference is the one thread
    that moves the ladder behind the last pair of rungs, the LDS counts and the per-ladder betas;
(b) the evidence of an adapted ladder (``--ntemps-evidence`` rungs, the first half of ``--steps`` adapting): the ladder it finds,
    the swap fractions of the frozen phase and both evidences, beside ``SMCSampler`` on the same box.

The rates are host clocks around calls that end in a device synchronisation, after a warm-up of every shape, over windows of at
least ``--seconds`` (the step count from a short probe), ``--runs`` times with the variants alternating.  Prints one JSON line.
Not a test.

    python scripts/gpu_ensemble_adapt_rate.py --seconds 1.0 --runs 2 --steps 3000
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
MIXTURE = [('de', 0.8), ('snooker', 0.2)]


def main():
    pars = argparse.ArgumentParser()
    pars.add_argument('--seconds', type=float, default=1.0)
    pars.add_argument('--runs', type=int, default=2)
    pars.add_argument('--steps', type=int, default=3000, help='steps of the run of (b), the first half adapting')
    pars.add_argument('--ntemps', type=int, default=8)
    pars.add_argument('--ntemps-evidence', type=int, default=16)
    pars.add_argument('--beta-min', type=float, default=None, help='beta_min of the ladder (b) starts from')
    pars.add_argument('--walkers', type=int, default=64)
    pars.add_argument('--max-batch', type=int, default=256)
    pars.add_argument('--lag', type=float, default=10000.0)
    pars.add_argument('--time', type=float, default=100.0)
    pars.add_argument('--no-rate', action='store_true')
    pars.add_argument('--no-evidence', action='store_true')
    pars.add_argument('--no-smc', action='store_true')
    args = pars.parse_args()
    import numpy as np
    import torch
    torch.cuda.init()
    from conftest import synth_joint_problem
    from vega_amd import SMCSampler, TemperedEnsemble, VegaInterface
    from vega_amd.defaults import DEFAULT_VALUES
    vega = VegaInterface(None, problem=synth_joint_problem(), max_batch=args.max_batch)
    vega.freeze_metals()
    sp = {'limits': {n: DEFAULT_VALUES[n][0] for n in SAMPLED}, 'values': {n: vega.params[n] for n in SAMPLED},
          'errors': {n: DEFAULT_VALUES[n][1] for n in SAMPLED}}
    T, W = args.ntemps, args.walkers
    adapt = dict(adapt=True, adaptation_lag=args.lag, adaptation_time=args.time)

    def clock(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    kw = dict(seed=2, sample_params=sp, moves=MIXTURE)
    out = {'sampled': len(SAMPLED), 'T': T, 'W': W, 'max_batch': args.max_batch, 'lag': args.lag, 'time': args.time}
    if not args.no_rate:
        runs = {'adapting': TemperedEnsemble(vega, W, ntemps=T, **kw, **adapt).run(1), 'fixed': TemperedEnsemble(vega, W, ntemps=T, **kw).run(1)}
        for s in runs.values():
            s.run(3)                                                    # (warm-up: lanes, tables, code)
        steps = {}
        for key, s in runs.items():
            dt, _ = clock(lambda: s.run(20))
            steps[key] = max(20, int(np.ceil(20 * args.seconds / dt * 1.15)))
        rates = {key: [] for key in runs}
        for _ in range(args.runs):
            for key, s in runs.items():
                s._chain.clear(), s._chain_lnl.clear(), s._beta_hist.clear()        # (the records of the rate runs are not kept)
                dt, _ = clock(lambda: s.run(steps[key]))
                rates[key].append(steps[key] * T * W / dt)
        out['rate_steps'] = steps
        out['proposals_per_s'] = {key: [round(v) for v in vals] for key, vals in rates.items()}
        out['adapting_over_fixed'] = round(float(np.mean(rates['adapting']) / np.mean(rates['fixed'])), 4)
        out['rate_ladder'] = [float(b) for b in runs['adapting'].current_betas[0]]
        out['rate_skipped'] = int(runs['adapting'].stats['adapt_skipped'][0])
    if not args.no_evidence:
        Te, half = args.ntemps_evidence, args.steps // 2
        dt, run = clock(lambda: TemperedEnsemble(vega, W, ntemps=Te, beta_min=args.beta_min, adapt_steps=half, **kw, **adapt).run(args.steps))
        out.update(evidence_T=Te, steps=args.steps, adapt_steps=half, ladder_seconds=round(dt, 3), ladder_rows=args.steps * Te * W,
                   start_ladder=[float(b) for b in run.betas], ladder=[float(b) for b in run.current_betas[0]],
                   adapt_skipped=int(run.stats['adapt_skipped'][0]),
                   swap_fraction=[round(float(v), 4) for v in run.swap_fraction[0]],
                   frozen_swap_fraction=[round(float(v), 4) for v in run.frozen_swap_fraction[0]],
                   mean_lnl_by_rung=[float(v) for v in run.get_log_lik(discard=run.frozen_rows[0], rung=None)[0].mean(axis=(1, 2))],
                   log_z_ss=[float(v) for v in run.log_evidence('ss')], log_z_ti=[float(v) for v in run.log_evidence('ti')])
        if not args.no_smc:
            dt, smc = clock(lambda: SMCSampler(vega, particles=1024, seed=2, sample_params=sp).run())
            out['log_z_smc'], out['smc_rows'], out['smc_seconds'] = [float(v) for v in smc.log_evidence()], smc.stats['rows'], round(dt, 3)
    print(json.dumps(out), flush=True)
    vega.close()


if __name__ == '__main__':
    main()
