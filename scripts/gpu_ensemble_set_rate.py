#!/usr/bin/env python
"""Proposals / s of many ensembles advanced together (vega_amd/ensemble.py: EnsembleSet, vmx_ensemble_run_many) against the same
ensembles one after another through the single sampler (vmx_ensemble_run), on the synthetic joint problem (BASELINE configs[2]: the
bench's joint workload) with 6 sampled parameters and max_batch 256:

(a) E = 16 ensembles of W = 64 walkers, one Monte-Carlo mock each, as one set;
(b) the same 16 ensembles one after another, every mock installed as the engine's data in turn (the time to install counts and
    is also reported on its own);
(c) E = 4 ensembles of W = 256 on shared data as one set (``together = True``) against four sequential single runs.

Every figure is a host clock around calls that end in a device synchronisation, after a warm-up of every shape, over windows of
at least ``--seconds`` (the step count is set from a short probe), ``--runs`` times with the variants alternating.  Prints one
JSON line.  ``--only set``: nothing but (a), for a kernel trace of its own.  Not a test.

    python scripts/gpu_ensemble_set_rate.py --seconds 1.0 --runs 2
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


def main():
    pars = argparse.ArgumentParser()
    pars.add_argument('--seconds', type=float, default=1.0)
    pars.add_argument('--runs', type=int, default=2)
    pars.add_argument('--max-batch', type=int, default=256)
    pars.add_argument('--only', choices=['all', 'set'], default='all')
    pars.add_argument('--steps', type=int, default=0, help='fixed step count instead of the probe')
    args = pars.parse_args()
    import numpy as np
    import torch
    torch.cuda.init()
    from conftest import synth_joint_problem
    from vega_amd import EnsembleSampler, EnsembleSet, VegaInterface
    from vega_amd.defaults import DEFAULT_VALUES
    from vega_amd.montecarlo import MonteCarlo
    vega = VegaInterface(None, problem=synth_joint_problem(), max_batch=args.max_batch)
    vega.freeze_metals()
    eng = vega.engine
    sp = {'limits': {n: DEFAULT_VALUES[n][0] for n in SAMPLED}, 'values': {n: vega.params[n] for n in SAMPLED},
          'errors': {n: DEFAULT_VALUES[n][1] for n in SAMPLED}}
    E_mock, W_mock, E_rep, W_rep = 16, 64, 4, 256
    mocks = MonteCarlo(vega).create_mocks(vega.compute_model(), E_mock, seed=1)
    for name, pool in mocks.items():
        eng.set_mock_pool(name, pool)

    def clock(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    def mock_set(steps):
        return EnsembleSet(vega, E_mock, W_mock, mock_rows=np.arange(E_mock), seed=2, sample_params=sp).run(steps)

    def mock_sequence(steps):
        """What a user can do without the set: every mock installed as the data, then a single run of its own."""
        install = 0.0
        try:
            for m in range(E_mock):
                t0 = time.perf_counter()
                for name, pool in mocks.items():
                    eng.set_data(name, pool[m])
                install += time.perf_counter() - t0
                EnsembleSampler(vega, W_mock, seed=2, stream=m, sample_params=sp).run(steps)
        finally:
            t0 = time.perf_counter()
            for name in mocks:
                eng.set_data(name, vega.data[name].masked_data_vec)
            install += time.perf_counter() - t0
        return install

    def replica_set(steps):
        return EnsembleSet(vega, E_rep, W_rep, seed=2, sample_params=sp).run(steps)

    def replica_sequence(steps):
        for r in range(E_rep):
            EnsembleSampler(vega, W_rep, seed=2, stream=r, sample_params=sp).run(steps)

    def steps_for(fn):
        """Warm the shapes up, then the step count that fills the window, from a probe of 20 steps."""
        fn(3)
        if args.steps > 0:
            return args.steps
        dt, _ = clock(lambda: fn(20))
        return max(20, int(np.ceil(20 * args.seconds / dt * 1.15)))

    out = {'sampled': len(SAMPLED), 'max_batch': args.max_batch, 'runs': args.runs, 'window_seconds': args.seconds}
    variants = [('a_set_16x64_mocks', mock_set, E_mock * W_mock)]
    if args.only == 'all':
        variants += [('b_sequence_16x64_mocks', mock_sequence, E_mock * W_mock), ('c_set_4x256', replica_set, E_rep * W_rep),
                     ('c_sequence_4x256', replica_sequence, E_rep * W_rep)]
    steps = {key: steps_for(fn) for key, fn, _ in variants}
    rates = {key: [] for key, _, _ in variants}
    installs = []
    for _ in range(args.runs):
        for key, fn, per in variants:
            dt, got = clock(lambda: fn(steps[key]))
            rates[key].append(steps[key] * per / dt)
            if key.startswith('b_'):
                installs.append(got / dt)
            if key.startswith('a_'):
                out['a_engine_calls_per_half'] = got.stats['engine_calls'] / (2 * steps[key])
                out['a_seconds_enqueuing_share'] = got.stats['seconds_enqueuing'] / got.stats['seconds']
                out['a_const_hint'] = int(eng.derived_const_hint(got.cols))
    for key in rates:
        out[key + '_steps'] = steps[key]
        out[key + '_proposals_per_s'] = [round(r) for r in rates[key]]
    if args.only == 'all':
        out['b_install_share_of_time'] = [round(v, 4) for v in installs]
        out['a_over_b'] = round(float(np.mean(rates['a_set_16x64_mocks']) / np.mean(rates['b_sequence_16x64_mocks'])), 3)
        out['c_set_over_sequence'] = round(float(np.mean(rates['c_set_4x256']) / np.mean(rates['c_sequence_4x256'])), 3)
    print(json.dumps(out), flush=True)
    vega.close()


if __name__ == '__main__':
    main()
