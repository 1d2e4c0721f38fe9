#!/usr/bin/env python
"""Proposals / s of the ensemble sampler's two drivers (vega_amd/ensemble.py) and of a bare ``chi2_batch_device`` loop over the
same batches, on the synthetic joint problem (BASELINE configs[2]: the bench's joint workload), for W walkers = halves of W / 2
rows in chunks of max_batch.  Prints one JSON line per W.  Not a test.

    python scripts/gpu_ensemble_rate.py --walkers 512 1024 --steps 40
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
    pars.add_argument('--walkers', type=int, nargs='+', default=[512, 1024])
    pars.add_argument('--steps', type=int, default=40)
    pars.add_argument('--python-steps', type=int, default=10)
    pars.add_argument('--max-batch', type=int, default=256)
    args = pars.parse_args()
    import numpy as np
    import torch
    torch.cuda.init()
    from conftest import synth_joint_problem
    from vega_amd import EnsembleSampler, VegaInterface
    vega = VegaInterface(None, problem=synth_joint_problem(), max_batch=args.max_batch)
    from vega_amd.defaults import DEFAULT_VALUES
    sp = {'limits': {n: DEFAULT_VALUES[n][0] for n in SAMPLED}, 'values': {n: vega.params[n] for n in SAMPLED},
          'errors': {n: DEFAULT_VALUES[n][1] for n in SAMPLED}}
    for W in args.walkers:
        out = {'W': W, 'sampled': len(SAMPLED), 'max_batch': args.max_batch}
        EnsembleSampler(vega, W, seed=1, sample_params=sp).run(3)                       # (warm-up: lanes, tables, code)
        s = EnsembleSampler(vega, W, seed=2, sample_params=sp).run(args.steps)
        out['device_proposals_per_s'] = s.stats['proposals'] / s.stats['seconds']
        out['device_seconds_enqueuing'] = s.stats['seconds_enqueuing']
        out['device_const_hint'] = int(s.vega.engine.derived_const_hint(s.cols))
        p = EnsembleSampler(vega, W, seed=2, driver='python', sample_params=sp).run(args.python_steps)
        out['python_proposals_per_s'] = p.stats['proposals'] / p.stats['seconds']
        # the engine alone on the same batches: W / 2 rows per half in chunks of max_batch, two lanes, the same table level,
        # one host synchronisation per half-step as the python driver (none in between for the bare loop's own chunks)
        eng = vega.engine
        theta = np.repeat(vega._theta(None)[None, :], W // 2, axis=0)
        theta[:, s.cols] = s.x[:W // 2]
        t = torch.from_numpy(theta).cuda()
        hint = out['device_const_hint']
        eng.set_constant_nl_hint(hint > 0, hint >= 2)
        eng.set_lanes(2)
        vega.chi2_batch_device(t)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(2 * args.steps):
            vega.chi2_batch_device(t)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        eng.set_lanes(1)
        eng.set_constant_nl_hint(False)
        out['bare_chi2_batch_device_rows_per_s'] = 2 * args.steps * (W // 2) / dt
        out['device_over_bare'] = out['device_proposals_per_s'] / out['bare_chi2_batch_device_rows_per_s']
        print(json.dumps(out), flush=True)
    vega.close()


if __name__ == '__main__':
    main()
