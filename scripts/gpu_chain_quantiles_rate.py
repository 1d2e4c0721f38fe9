#!/usr/bin/env python
"""What the quantiles and the best point of every mock cost: on the device, where the recorded rows are
(vmx_chain_store_order_stats, vmx_chain_store_best through ``EnsembleSet.quantiles`` / ``best``), against the host's way - the
whole chain fetched from the store, then ``np.quantile`` and an argmax per mock.  On the synthetic joint problem (BASELINE
configs[2]) with 6 sampled parameters, max_batch 256, W = 32 walkers and ``--steps`` steps (1000), for every M of ``--mocks``
(256, 1024); the set runs once per M with ``sample_mocks(summaries='device', keep_chains=False)``, both ways then read the same
store, in one process after a warm-up of both.

Per M one JSON line, every figure a host clock around calls that end in a device synchronisation:
  device_first_s    five quantiles plus ``best`` on the rows after the burn-in, the first call (it allocates the scratch of keys)
  device_s          the same call once more (the scratch is there)
  host_fetch_s      ``get_chain()`` + ``get_log_lik()``: the chain to the host
  host_numpy_s      ``np.quantile(method='linear')`` over the flattened rows of every mock, and the argmax of lnL
  host_s            the two together - what the call replaces
  max_abs_diff      the largest |device - numpy| over the quantiles (rounding of the interpolation; the order statistics are exact)
``--corner ROWS``: a single ensemble (E = 1, the same W and n) with a synthetic chain of ROWS rows appended to a store of its
own - only n work-groups run the select - the same two calls and clocks.  ``--only device``: nothing but the device calls, for a
kernel trace of its own.  Not a test.

    python scripts/gpu_chain_quantiles_rate.py --mocks 256 1024 --steps 1000 --corner 100000
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
Q5 = [0.025, 0.16, 0.5, 0.84, 0.975]


def main():
    pars = argparse.ArgumentParser()
    pars.add_argument('--mocks', type=int, nargs='*', default=[256, 1024])
    pars.add_argument('--steps', type=int, default=1000)
    pars.add_argument('--walkers', type=int, default=32)
    pars.add_argument('--max-batch', type=int, default=256)
    pars.add_argument('--corner', type=int, default=0)
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
    n = len(SAMPLED)

    def clock(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    def device_way(run, first):
        return run.quantiles(Q5, first), run.best(first)

    def host_numpy(chain, lnl, first):
        E = chain.shape[0]
        q = np.quantile(chain[:, first:].reshape(E, -1, n), Q5, axis=1, method='linear')
        flat = lnl[:, first:].reshape(E, -1)
        at = np.argmax(flat, axis=1)
        return np.moveaxis(q, 0, 2), flat[np.arange(E), at], chain[:, first:].reshape(E, -1, n)[np.arange(E), at]

    def both(run, first, base):
        first_s, _ = clock(lambda: device_way(run, first))
        again_s, (q, top) = clock(lambda: device_way(run, first))
        out = dict(base, device_first_s=round(first_s, 5), device_s=round(again_s, 5))
        if args.only == 'all':
            fetch_s, (chain, lnl) = clock(lambda: (run.get_chain(), run.get_log_lik()))
            numpy_s, (q_ref, top_ref, at_ref) = clock(lambda: host_numpy(chain, lnl, first))
            assert np.array_equal(top['lnl_max'], top_ref) and np.array_equal(top['best'], at_ref)
            out.update(host_fetch_s=round(fetch_s, 4), host_numpy_s=round(numpy_s, 4), host_s=round(fetch_s + numpy_s, 4),
                       max_abs_diff=float(np.max(np.abs(q - q_ref))))
        print(json.dumps(out), flush=True)

    def run_of(mocks, steps):
        return mc.sample_mocks(mocks=mocks, walkers=args.walkers, steps=steps, seed=2, sample_params=sp, summaries='device', keep_chains=False)

    warm = run_of(mc.create_mocks(fiducial, 8, seed=1), 30)
    device_way(warm, 10)
    if args.only == 'all':
        host_numpy(warm.get_chain(), warm.get_log_lik(), 10)
    warm.discard_chain()
    for M in args.mocks:
        run = run_of(mc.create_mocks(fiducial, M, seed=1), args.steps)
        first = mc.mc_posteriors['burn']
        both(run, first, dict(mocks=M, walkers=args.walkers, steps=args.steps, sampled=n, rows_used=args.steps - first,
                              chain_bytes=M * args.steps * args.walkers * n * 8, run_s=round(run.stats['seconds'], 3)))
        run.discard_chain()
        del run
    if args.corner > 0:
        from vega_amd.ensemble import EnsembleSet
        rows = args.corner
        rng = np.random.default_rng(3)
        one = EnsembleSet(vega, 1, args.walkers, seed=2, sample_params=sp, chain='device')
        one._store = vega.engine.chain_store(1, args.walkers, n, rows)
        one._store.append(1.0 + 0.05 * rng.standard_normal((1, rows, args.walkers, n)), -rng.random((1, rows, args.walkers)))
        both(one, 0, dict(corner=True, mocks=1, walkers=args.walkers, rows_used=rows, sampled=n, chain_bytes=rows * args.walkers * n * 8))
        one.discard_chain()
    vega.close()


if __name__ == '__main__':
    main()
