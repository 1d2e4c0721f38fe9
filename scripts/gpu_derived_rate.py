#!/usr/bin/env python
"""Rows / s of the marginalisation coefficients as derived columns (vega_amd/interface.py: marg_coeff_batch_device, the fold
coeff = c0 - G dx of include/vegamx.h: vmx_marg_coeff_device) against the route a caller had before it,
``chi2_batch(return_marg_coeff=True)`` (full chain, host entry, a copy back per item and chunk), on the same rows in one process:
the `rtmax` marginalisation problem of the tests (200 templates, 1590 fitted bins, nq = 2500 + broadband), rows scattered by 2 %
over the sampled parameters, the table level those columns allow.  A warm-up, then ``--windows`` timed windows of at least
``--min-seconds`` each per route; the spread over the windows is printed.  Also: what the fold adds to the set-up of the quadratic
form (the same problem with and without its map, rebuilt ``--rebuilds`` times each).  Prints one JSON line.
Not a test.

    python scripts/gpu_derived_rate.py --rows 4096 --max-batch 256

The product G dx alone: run the new entry under the profiler, then summarise the trace (median per dispatch: the few set-up
products of the same kernel do not move it)

    rocprofv3 --kernel-trace --stats --output-format csv -d trace_dir -- python scripts/gpu_derived_rate.py --device-only
    python scripts/gpu_derived_rate.py --kernel-stats trace_dir
"""
import argparse
import csv
import json
import statistics
import sys
import tempfile
import time
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
for p in (REPO, REPO / 'tests'):
    if str(p) not in sys.path:
        sys.path.insert(0, str(p))


def kernel_stats(folder):
    """Median and count per kernel of a ``rocprofv3 --kernel-trace`` run, the chain's kernels in order of their share."""
    per = {}
    rows = 0
    for path in Path(folder).rglob('*kernel_trace.csv'):
        with open(path, newline='') as f:
            for row in csv.DictReader(f):
                rows += 1
                per.setdefault(row['Kernel_Name'], []).append((int(row['End_Timestamp']) - int(row['Start_Timestamp'])) * 1e-3)
    if not rows:
        raise SystemExit(f'no *kernel_trace.csv under {folder}')
    total = sum(sum(v) for v in per.values())
    table = sorted(per.items(), key=lambda kv: -sum(kv[1]))[:14]
    out = {'kernel_seconds': total * 1e-6,
           'kernels': [{'name': k[:96], 'dispatches': len(v), 'median_us': statistics.median(v), 'share': sum(v) / total}
                       for k, v in table]}
    print(json.dumps(out), flush=True)


def windows(fn, rows_per_call, n_windows, min_seconds, sync):
    """rows / s of ``fn`` over ``n_windows`` windows of at least ``min_seconds``."""
    rates = []
    for _ in range(n_windows):
        calls, dt = 0, 0.0
        t0 = time.perf_counter()
        while dt < min_seconds:
            fn()
            calls += 1
            sync()
            dt = time.perf_counter() - t0
        rates.append(calls * rows_per_call / dt)
    return {'rows_per_s': statistics.mean(rates), 'min': min(rates), 'max': max(rates), 'windows': n_windows}


def main():
    pars = argparse.ArgumentParser()
    pars.add_argument('--rows', type=int, default=4096)
    pars.add_argument('--max-batch', type=int, default=256)
    pars.add_argument('--windows', type=int, default=5)
    pars.add_argument('--min-seconds', type=float, default=0.5)
    pars.add_argument('--rebuilds', type=int, default=3)
    pars.add_argument('--device-only', action='store_true')
    pars.add_argument('--kernel-stats', default=None, metavar='DIR')
    args = pars.parse_args()
    if args.kernel_stats:
        return kernel_stats(args.kernel_stats)
    import numpy as np
    import torch
    torch.cuda.init()
    from conftest import marginalization_problem, MARGINALIZATION_CASES
    from vega_amd import VegaInterface, synthetic
    name = 'lyalya_lyalya'
    with tempfile.TemporaryDirectory() as tmp:
        prob = marginalization_problem(Path(tmp), MARGINALIZATION_CASES['rtmax'])
        vega = VegaInterface(None, problem=prob, max_batch=args.max_batch)
        eng = vega.engine
        limits = {k: tuple(v) for k, v in prob.sample_params['limits'].items()}
        theta = synthetic.walkers(eng.low.theta0, eng.names, args.rows, varied=list(limits), seed=1, limits=limits)
        cols = np.array([vega.param_names.index(n) for n in limits], dtype=np.int32)
        hint = int(eng.derived_const_hint(cols))
        t_dev = torch.from_numpy(theta).cuda()
        item = prob.items[name]
        out = {'rows': args.rows, 'max_batch': args.max_batch, 'templates': int(item.marg_diff2coeff.shape[0]), 'const_hint': hint,
               'quadratic_form': bool(eng.quadratic_form)}
        eng.set_constant_nl_hint(hint > 0, hint >= 2)
        # warm-up: the fold, tables, code
        block = vega.marg_coeff_batch_device(t_dev)
        torch.cuda.synchronize()
        out['form'] = eng.last_form()
        out['device'] = windows(lambda: vega.marg_coeff_batch_device(t_dev), args.rows, args.windows, args.min_seconds,
                                torch.cuda.synchronize)
        if not args.device_only:
            eng.set_constant_nl_hint(False)         # (vmx_eval derives the level from the host rows itself)
            host = vega.chi2_batch(theta, return_marg_coeff=True)[1][name]
            out['max_difference_over_scale'] = float(np.abs(block.cpu().numpy() - host).max() / np.abs(host).max())
            out['host_route'] = windows(lambda: vega.chi2_batch(theta, return_marg_coeff=True), args.rows, args.windows,
                                        args.min_seconds, lambda: None)
            out['device_over_host_route'] = out['device']['rows_per_s'] / out['host_route']['rows_per_s']
            out['device_over_host_route_worst_windows'] = out['device']['min'] / out['host_route']['max']
            # what the fold adds to the set-up of the quadratic form: the same problem without its map, in this process
            chunk = t_dev[:args.max_batch].contiguous()

            def rebuild_seconds(v):
                times = []
                for _ in range(args.rebuilds):
                    v.engine.set_quadratic_form(True)       # (a new reference point: every tensor is rebuilt at the next call)
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    v.chi2_batch_device(chunk)
                    torch.cuda.synchronize()
                    times.append(time.perf_counter() - t0)
                return times
            rebuild_seconds(vega)
            with_fold = rebuild_seconds(vega)
            vega.close()
            item.marg_diff2coeff = None
            bare = VegaInterface(None, problem=prob, max_batch=args.max_batch)
            rebuild_seconds(bare)
            without = rebuild_seconds(bare)
            bare.close()
            out['quad_build_seconds_with_fold'] = [round(t, 5) for t in with_fold]
            out['quad_build_seconds_without_map'] = [round(t, 5) for t in without]
            out['fold_adds_seconds'] = statistics.median(with_fold) - statistics.median(without)
        else:
            vega.close()
    print(json.dumps(out), flush=True)


if __name__ == '__main__':
    main()
