#!/usr/bin/env python
"""What the per-mock posteriors cost behind the run itself: ``sample_mocks(summaries='host')`` - the whole chain copied to the host
at the end of every call, mean / sd / covariance in NumPy and one FFT per (mock, walker, parameter) for tau - against
``sample_mocks(summaries='device', keep_chains=False)`` - the recorded rows kept in a chain store on the device and reduced there
(vmx_chain_store_summary), a few hundred bytes per mock crossing to the host.  On the synthetic joint problem (BASELINE
configs[2]: the bench's joint workload) with 6 sampled parameters, max_batch 256, W = 32 walkers and ``--steps`` steps (1000),
for every M of ``--mocks`` (256, 1024), both paths in one process after a warm-up of both.

Per path and M one JSON line, every figure a host clock around calls that end in a device synchronisation:
  total_s           the whole ``sample_mocks`` call (the mocks are drawn beforehand and passed in)
  run_s             the library's own clock over its ensemble calls (``stats['seconds']``): for the host path it includes the copy
                    of the chain to the host, for the device path the device-to-device copy into the store
  copy_back_s       host path only: its run_s minus the device path's - the same half-steps, with and without the copy
  summary_s         total_s - run_s - setup_s: NumPy moments and FFTs (host), vmx_chain_store_summary (device)
  setup_s           what both paths do alike around the run (pools to the engine, start positions and their chi2): measured on
                    the device path as total_s - run_s - device_summary_s
  device_summary_s  device path only: ``summary()`` called once more on the finished run, on its own clock
``--only device``: nothing but the device path, for a kernel trace of its own.  Not a test.

    python scripts/gpu_chain_summary_rate.py --mocks 256 1024 --steps 1000
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
    pars.add_argument('--mocks', type=int, nargs='+', default=[256, 1024])
    pars.add_argument('--steps', type=int, default=1000)
    pars.add_argument('--walkers', type=int, default=32)
    pars.add_argument('--max-batch', type=int, default=256)
    pars.add_argument('--only', choices=['all', 'device'], default='all')
    args = pars.parse_args()
    import numpy as np
    import torch
    torch.cuda.init()
    from conftest import synth_joint_problem
    from vega_amd import VegaInterface
    from vega_amd.defaults import DEFAULT_VALUES
    from vega_amd.montecarlo import MonteCarlo
    vega = VegaInterface(None, problem=synth_joint_problem(), max_batch=args.max_batch)
    vega.freeze_metals()
    sp = {'limits': {n: DEFAULT_VALUES[n][0] for n in SAMPLED}, 'values': {n: vega.params[n] for n in SAMPLED},
          'errors': {n: DEFAULT_VALUES[n][1] for n in SAMPLED}}
    mc = MonteCarlo(vega)
    fiducial = vega.compute_model()

    def clock(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    def path(mocks, steps, device):
        kw = dict(summaries='device', keep_chains=False) if device else dict(summaries='host', keep_chains=False)
        return mc.sample_mocks(mocks=mocks, walkers=args.walkers, steps=steps, seed=2, sample_params=sp, **kw)

    warm = mc.create_mocks(fiducial, 8, seed=1)
    for device in ((True,) if args.only == 'device' else (True, False)):
        path(warm, 30, device)
    for M in args.mocks:
        mocks = mc.create_mocks(fiducial, M, seed=1)
        base = dict(mocks=M, walkers=args.walkers, steps=args.steps, sampled=len(SAMPLED), max_batch=args.max_batch,
                    chain_bytes=M * args.steps * args.walkers * len(SAMPLED) * 8)
        total, run = clock(lambda: path(mocks, args.steps, True))
        first = mc.mc_posteriors['burn']
        again, _ = clock(lambda: run.summary(discard=first))
        dev = dict(base, path='device', total_s=round(total, 3), run_s=round(run.stats['seconds'], 3),
                   device_summary_s=round(again, 4), setup_s=round(total - run.stats['seconds'] - again, 3),
                   summary_s=round(again, 4), proposals_per_s=round(run.stats['proposals'] / run.stats['seconds']),
                   host_synchronisations=run.stats['host_synchronisations'],
                   tau_max=round(float(np.max(mc.mc_posteriors['tau'])), 2))
        print(json.dumps(dev), flush=True)
        run_dev, setup = run.stats['seconds'], total - run.stats['seconds'] - again
        run.discard_chain()
        del run
        if args.only == 'device':
            continue
        total, run = clock(lambda: path(mocks, args.steps, False))
        host = dict(base, path='host', total_s=round(total, 3), run_s=round(run.stats['seconds'], 3),
                    copy_back_s=round(run.stats['seconds'] - run_dev, 3), setup_s=round(setup, 3),
                    summary_s=round(total - run.stats['seconds'] - setup, 3),
                    proposals_per_s=round(run.stats['proposals'] / run.stats['seconds']),
                    tau_max=round(float(np.max(mc.mc_posteriors['tau'])), 2))
        print(json.dumps(host), flush=True)
        del run
    vega.close()


if __name__ == '__main__':
    main()
