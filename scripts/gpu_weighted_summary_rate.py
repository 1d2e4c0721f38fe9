#!/usr/bin/env python
"""What the weighted summary, five weighted quantiles and the best point of every mock cost: in a sample store on the device
(vmx_sample_store_*, ``Engine.sample_store``) against the host's way - the loop of ``MonteCarlo._sample_mocks`` (``w @ pts`` and
the reliability-weights covariance per mock) plus ``np.quantile(weights=, method='inverted_cdf')`` per mock and parameter and an
argmax.  Synthetic weighted sets in the two shapes the samplers produce, n = 6: ``--shapes 256x25000 1024x4096`` (a boosted nested
set, a recycled SMC set; log-normal weights of width 2, ragged by up to 10 %), after a warm-up of both ways on a small store.

Per shape one JSON line, every figure a host clock around calls that end in a device synchronisation:
  put_s             the upload of every set (the rows are on the host: it counts against the device path)
  summary_s         ``store.summary()``, the second call (the first allocates the scratch: summary_first_s)
  quantiles_best_s  five quantiles plus ``best``, the second call (quantiles_best_first_s: with the scratch of keys)
  device_s          put + summary + quantiles and best
  host_moments_s    the loop of ``_sample_mocks``
  host_quantiles_s  ``np.quantile(weights=, method='inverted_cdf')`` per mock and parameter, and the argmax of lnL
  host_s            the two together
  equal_quantiles   whether every device quantile is NumPy's, bit for bit (the float weights against the integer ones)
``--nested-mocks M``: one real ``sample_mocks_nested(boost_posterior=...)`` call on the synthetic joint problem with M mocks,
``summaries='device', weighted_quantiles=Q5``, and the host's way over its kept chains.  ``--only device``: nothing but the device
calls, for a kernel trace of its own.  Not a test.

    python scripts/gpu_weighted_summary_rate.py --shapes 256x25000 1024x4096 --nested-mocks 16
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
    pars.add_argument('--shapes', nargs='*', default=['256x25000', '1024x4096'])
    pars.add_argument('--nested-mocks', type=int, default=0)
    pars.add_argument('--num-live', type=int, default=128)
    pars.add_argument('--threads', type=int, default=32)
    pars.add_argument('--boost', type=float, default=5.0)
    pars.add_argument('--max-iterations', type=int, default=None)
    pars.add_argument('--max-batch', type=int, default=256)
    pars.add_argument('--only', choices=['all', 'device'], default='all')
    args = pars.parse_args()
    import numpy as np
    import torch
    torch.cuda.init()
    from conftest import synth_joint_problem
    from vega_amd import VegaInterface
    vega = VegaInterface(None, problem=synth_joint_problem(), max_batch=args.max_batch)
    vega.freeze_metals()
    eng = vega.engine
    n = len(SAMPLED)

    def clock(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    def synthetic(E, rows, seed=3):
        rng = np.random.default_rng(seed)
        sets = []
        for e in range(E):
            count = rows - int(rng.integers(0, max(rows // 10, 1)))
            w = np.exp(2.0 * rng.standard_normal(count))
            sets.append((1.0 + 0.05 * rng.standard_normal((count, n)), -rng.random(count), w / w.sum()))
        return sets

    def put_all(store, sets):
        for e, (x, lnl, w) in enumerate(sets):
            store.put(e, x, lnl, w)

    def select(store, total):
        return store.weighted_quantiles(Q5, total=total), store.best()

    def host_moments(sets):
        out = []
        for pts, _, w in sets:
            mean = w @ pts
            dev = pts - mean
            out.append((mean, (w[:, None] * dev).T @ dev / (1.0 - np.sum(w * w))))
        return out

    def host_quantiles(sets):
        q = np.array([[np.quantile(pts[:, d], Q5, weights=w, method='inverted_cdf') for d in range(n)] for pts, _, w in sets])
        return q, [(lnl.max(), pts[int(np.argmax(lnl))]) for pts, lnl, _ in sets]

    def both(sets, base):
        store = eng.sample_store(len(sets), n, max(len(s[2]) for s in sets))
        put_s, _ = clock(lambda: put_all(store, sets))
        first_s, summ = clock(store.summary)
        summary_s, summ = clock(store.summary)
        sel_first_s, _ = clock(lambda: select(store, summ['total']))
        sel_s, (q, top) = clock(lambda: select(store, summ['total']))
        out = dict(base, put_s=round(put_s, 5), summary_first_s=round(first_s, 5), summary_s=round(summary_s, 5),
                   quantiles_best_first_s=round(sel_first_s, 5), quantiles_best_s=round(sel_s, 5),
                   device_s=round(put_s + summary_s + sel_s, 5), n_eff_median=float(np.median(summ['n_eff'])))
        if args.only == 'all':
            mom_s, mom = clock(lambda: host_moments(sets))
            q_s, (q_ref, top_ref) = clock(lambda: host_quantiles(sets))
            sd = np.sqrt(np.array([np.diag(c) for _, c in mom]))
            out.update(host_moments_s=round(mom_s, 4), host_quantiles_s=round(q_s, 4), host_s=round(mom_s + q_s, 4),
                       equal_quantiles=bool(q.tobytes() == q_ref.tobytes()),
                       quantiles_differing=int(np.sum(q != q_ref)),
                       mean_diff_in_sd=float(np.max(np.abs(summ['mean'] - np.array([m for m, _ in mom])) / sd)),
                       equal_best=bool(all(top['lnl_max'][e] == t[0] for e, t in enumerate(top_ref))))
        print(json.dumps(out), flush=True)
        store.close()

    warm = synthetic(4, 300)
    store = eng.sample_store(4, n, 300)
    put_all(store, warm)
    select(store, store.summary()['total'])
    store.close()
    if args.only == 'all':
        host_moments(warm), host_quantiles(warm)
    for shape in args.shapes:
        E, rows = (int(v) for v in shape.split('x'))
        both(synthetic(E, rows), dict(sets=E, rows=rows, sampled=n, bytes=E * rows * (n + 2) * 8))
    if args.nested_mocks > 0:
        from vega_amd.defaults import DEFAULT_VALUES
        from vega_amd.montecarlo import MonteCarlo
        sp = {'limits': {k: DEFAULT_VALUES[k][0] for k in SAMPLED}, 'values': {k: vega.params[k] for k in SAMPLED},
              'errors': {k: DEFAULT_VALUES[k][1] for k in SAMPLED}}
        mc = MonteCarlo(vega)
        mocks = mc.create_mocks(vega.compute_model(), args.nested_mocks, seed=1)
        run_s, run = clock(lambda: mc.sample_mocks_nested(mocks=mocks, seed=2, sample_params=sp, num_live=args.num_live, threads=args.threads,
                                                          boost_posterior=args.boost, max_iterations=args.max_iterations))
        sets = [s for s in mc.mc_chains if s is not None]
        both(sets, dict(nested=True, sets=len(sets), rows=int(np.mean([len(s[2]) for s in sets])), sampled=n, run_s=round(run_s, 3),
                        num_live=args.num_live, threads=args.threads, boost=args.boost))
    vega.close()


if __name__ == '__main__':
    main()
